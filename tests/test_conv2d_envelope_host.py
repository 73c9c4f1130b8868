"""The tables of tests/conv2d_envelope.py on the host: a correct stand-in passes every row, twelve planted defects do not.

Stand-in: conv2d_envelope.Host -- float32 torch convolution, pooling and interpolation with one rounding to T behind the argument
checks of csrc/adm_convg.hip restated in Python, the output-size rule as fixed (the window must fit the padded image), reading
and writing through the request's pointers as the library does.  It must be accepted where the table says accepted, within the
unchanged bounds, and refuse with nothing written where the table says refused.
Defects: each of PLANTED fails the row named beside it, with the check named beside that; the same row passes without the defect.
Besides: what the tables must contain (every shape the envelope names, the kernel pick of every conv row, at least five
Frobenius-checked cases per pick), and ops.conv2d / ops.pool2d refusing the truncation family before they build a tensor.
"""
import pytest
import torch

import conv2d_envelope as c2
import inception_replay as ir

CPU = "cpu"
TYPES = [torch.bfloat16, torch.float16]
_ids = {torch.bfloat16: "bf16", torch.float16: "f16"}


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("label", c2.FAMILY_LABELS)
def test_every_row_holds_for_the_stand_in(label, T):
    outcomes, failures = c2.walk(c2.Host(), label, T, CPU)
    assert not failures, "\n".join(failures)
    rows = c2.rows_of(label)
    assert len(outcomes) == len(rows) and [o[1] for o in outcomes] == [r["expect"] for r in rows]


def _elems(d):
    oh, ow = ir.conv_out_hw(d)
    return d["n"] * oh * ow * d["cout"]


def test_the_conv2d_table_holds_what_the_envelope_names():
    acc = [r for f in c2.CONV_ACCEPTED for r in c2.rows_of(f)]
    assert 80 <= len(acc) <= 140 and all(r["expect"] == "accepted" for r in acc)
    names = [(f, r["name"]) for f in c2.FAMILY_LABELS for r in c2.rows_of(f)]
    assert len(names) == len(set(names))
    for r in acc:
        d = r["d"]
        assert d["n"] <= 3 and d["h"] * d["w"] <= 400 and d["cin_pad"] <= 96 and d["cout"] <= 260 and _elems(d) < ir.FULL_BELOW, r["name"]
        assert max(d["h"], d["w"]) <= 20 or min(d["h"], d["w"]) == 1, r["name"]      # longer than 20: the prime pixel counts only
        assert r["pick"] == ir.conv_kernel_pick(d["cout"]), r["name"]
    # the pick by cout
    by_pick = {p: sorted(r["d"]["cout"] for r in c2.rows_of("conv2d cout") if r["pick"] == p) for p in c2.PICKS}
    assert by_pick == {c2.K2: [4, 8, 28, 32], c2.L41: [36, 64, 132, 192, 260], c2.L22: [68, 128, 196, 256]}
    # K-steps on every pick
    for p in c2.PICKS:
        steps = sorted(r["d"]["kh"] * r["d"]["kw"] * r["d"]["cin_pad"] // 32 for r in c2.rows_of("conv2d K-steps") if r["pick"] == p)
        assert steps == [1, 2, 2, 3, 4, 5, 6, 7, 27, 49, 196], p
        ms = sorted(r["d"]["n"] * r["d"]["h"] * r["d"]["w"] for r in c2.rows_of("conv2d M") if r["pick"] == p)
        assert ms == [1, 63, 64, 65, 127, 128, 129, 255, 256, 257], p
    assert any(r["d"]["n"] == 3 and r["d"]["h"] * r["d"]["w"] == 43 for r in c2.rows_of("conv2d M"))
    geo = [r["d"] for r in c2.rows_of("conv2d geometry")]
    assert {(d["kh"], d["kw"]) for d in geo} >= {(1, 1), (3, 3), (5, 5), (2, 2), (1, 7), (7, 1), (1, 3), (3, 1), (14, 14)}
    assert {d["stride"] for d in geo} >= {1, 2, 3, 14} and {(d["ph"], d["pw"]) for d in geo} >= {(0, 0), (1, 1), (0, 3), (3, 0), (2, 1)}
    assert any(d["stride"] in (2, 3) and (d["h"] + 2 * d["ph"] - d["kh"]) % d["stride"] for d in geo)
    assert any(d["h"] == d["w"] == 2 and d["kh"] == 5 and d["ph"] == 2 for d in geo) and any(d["h"] == 1 for d in geo) and any(d["w"] == 1 for d in geo)
    lay = [r["d"] for r in c2.rows_of("conv2d layout")]
    assert {(d["cin"], d["cin_pad"]) for d in lay} >= {(3, 32), (31, 32), (32, 32), (3, 64), (31, 64), (32, 64), (33, 64)}
    assert {d["in_stride"] - d["cin_pad"] for d in lay if not d["in_off"]} >= {0, 8, 40} and any(d["in_off"] for d in lay)
    assert {d["out_off"] for d in lay if d["out_stride"] == d["cout"] + 16} >= {0, 4, 12} and any(d["out_stride"] % 8 == 4 for d in lay)
    assert {(d["has_bias"], d["relu"]) for d in lay} == {(a, b) for a in (True, False) for b in (True, False)}
    # the Frobenius check keeps at least five cases per pick
    for p in c2.PICKS:
        assert sum(1 for r in acc if r["pick"] == p and _elems(r["d"]) >= c2.FRO_MIN_ELEMS) >= 5, p


def test_the_other_tables_hold_what_the_envelope_names():
    pool = [r for r in c2.rows_of("pool2d")]
    got = {(r["d"]["k"], r["d"]["stride"], r["d"]["pad"], r["d"]["h"], r["d"]["w"], r["d"]["mode"]) for r in pool}
    assert got == {(k, s, p, h, w, m) for k in (1, 2, 3, 5) for s in (1, 2, 3) for p in range(k) for h, w in c2.POOL_MAPS for m in ("max", "avg")}
    assert {r["d"]["c"] for r in pool} == {8, 24, 64} and any(r["d"]["in_off"] for r in pool) and any(r["d"]["out_off"] for r in pool)
    for r in pool:      # refused exactly where the window does not fit the padded image
        d = r["d"]
        assert (r["expect"] == "accepted") == (d["h"] + 2 * d["pad"] >= d["k"] and d["w"] + 2 * d["pad"] >= d["k"]), r["name"]
    assert sum(r["expect"] == "refused" for r in pool) > 0
    gap = [r["d"] for r in c2.rows_of("global_avgpool_f32") if r["expect"] == "accepted"]
    assert {d["h"] * d["w"] for d in gap} == {1, 2, 63, 64, 65, 289} and {d["c"] for d in gap} >= {8, 40, 2048} and {d["n"] for d in gap} == {1, 3, 33}
    assert any(d["n"] == 33 and d["c"] == 64 for d in gap)
    rs = [r["d"] for r in c2.rows_of("resize")]
    assert len(rs) == 3 * 3 * len(c2.RESIZE_PAIRS) * 2 and {(d["kind"], d["half_pixel"], d["cpad"]) for d in rs} == {(k, h, c) for k in range(3) for h in range(3) for c in (8, 32)}
    for f in ("conv2d refusals", "pool2d refusals", "resize refusals"):
        assert all(r["expect"] == "refused" for r in c2.rows_of(f)), f
    for f in ("conv2d refusals", "pool2d refusals"):
        assert sum(r["name"].startswith("trunc") for r in c2.rows_of(f)) >= 4, f


def test_c_division_truncates_and_the_allocation_covers_it():
    # h = 2, k = 3, stride 2: the floor formula says 0 rows, C says 1
    assert (2 - 3) // 2 + 1 == 0 and c2.c_out_size(2, 3, 2, 0) == 1 and c2.c_out_size(1, 3, 3, 0) == 1 and c2.c_out_size(2, 3, 1, 0) == 0
    assert c2.c_out_size(7, 3, 2, 1) == (7 + 2 - 3) // 2 + 1 and c2.alloc_size(2, 3, 1, 0) == 1 and not c2.fits(2, 3, 0) and c2.fits(2, 5, 2)


# (defect, what it is, family, the row it must fail -- a name or, for the rotating pool rows, its prefix --, the failing check)
PLANTED = [
    ("a", "oh by truncating division", "conv2d refusals", "trunc h2k3s2", "accepted .status 0., the table says refused"),
    ("a", "oh by truncating division", "conv2d refusals", "trunc w1k3s3", "accepted .status 0., the table says refused"),
    ("a", "oh by truncating division", "pool2d refusals", "trunc h1k3s3 avg", "accepted .status 0., the table says refused"),
    ("a", "oh by truncating division", "pool2d", "max5/3/1@1x1", "accepted .status 0., the table says refused"),
    ("b", "last K-step dropped at steps 1", "conv2d K-steps", "K1/132", "worst err/bound"),
    ("b", "last K-step dropped at steps 2", "conv2d K-steps", "K2:1x2c32/68", "worst err/bound"),
    ("b", "last K-step dropped at steps 2", "conv2d K-steps", "K2:1x1c64/28", "worst err/bound"),
    ("c", "ring stages 0 and 2 swapped", "conv2d K-steps", "K3/68", "worst err/bound"),
    ("c", "ring stages 0 and 2 swapped", "conv2d K-steps", "K5/132", "worst err/bound"),
    ("d", "taps transposed", "conv2d geometry", "1x7", "worst err/bound"),
    ("d", "taps transposed", "conv2d geometry", "3x1", "worst err/bound"),
    ("e", "pad_h on both axes", "conv2d geometry", "p0,3", "worst err/bound"),
    ("e", "pad_h on both axes", "conv2d geometry", "p2,1", "worst err/bound"),
    ("f", "channel mask rounded to 16", "conv2d cout", "cout4", "not finite"),
    ("f", "channel mask rounded to 16", "conv2d cout", "cout132", "not finite"),
    ("f", "channel mask rounded to 16", "conv2d cout", "cout68", "not finite"),
    ("g", "out_off ignored", "conv2d layout", "out_off4", "not finite|outside its channel slice"),
    ("h", "channels cin_pad .. in_stride read", "conv2d layout", "in_stride+8/32", "not finite"),
    ("h", "channels cin_pad .. in_stride read", "conv2d layout", "in_off8", "not finite"),
    ("i", "last pixel of a 64-pixel tile dropped", "conv2d M", "M64/32", "not finite"),
    ("i", "last pixel of a 64-pixel tile dropped", "conv2d M", "M129/128", "not finite"),
    ("j", "truncated output", "conv2d cout", "cout256", "fro/u"),
    ("j", "truncated output", "conv2d M", "M63/32", "fro/u"),
    ("k", "avg pooling divides by k k", "pool2d", "avg3/1/1@9x9", "worst err/bound"),
    ("l", "bicubic out == 1 samples the centre", "resize", "f32_nhwc hp2 7x5>1x1 c8", "worst err/bound"),
    ("l", "bicubic out == 1 samples the centre", "resize", "u8_nhwc hp2 7x5>1x9 c32", "worst err/bound"),
]


def _row(label, name):
    rows = c2.rows_of(label)
    i = next(i for i, r in enumerate(rows) if r["name"] == name or r["name"].startswith(name + "c"))
    return i, rows[i]


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("defect,what,label,name,message", PLANTED, ids=[f"{p[0]}: {p[1]}, {p[2]} {p[3]}" for p in PLANTED])
def test_planted_defects_fail(defect, what, label, name, message, T):
    i, r = _row(label, name)
    assert c2.try_row(c2.Host(), label, r, T, CPU, 100 + i)[0] == r["expect"]       # the same row passes without the defect
    with pytest.raises(AssertionError, match=message):
        c2.try_row(c2.Host(defect), label, r, T, CPU, 100 + i)


def test_every_defect_is_planted_and_truncation_passes_the_per_element_bound():
    assert {p[0] for p in PLANTED} == set(c2.DEFECTS) and len(c2.DEFECTS) == 12
    # j is seen by the Frobenius check alone: a case below the element threshold passes with it
    i, r = _row("conv2d M", "M1/32")
    assert _elems(r["d"]) < c2.FRO_MIN_ELEMS and c2.try_row(c2.Host("j"), "conv2d M", r, torch.float16, CPU, 100 + i)[3] is False


@pytest.mark.parametrize("name,kw", c2.TRUNCATION, ids=[t[0] for t in c2.TRUNCATION])
def test_ops_refuse_the_truncation_family_before_building_a_tensor(name, kw):
    from autodiffusion_amd import ops
    x = torch.zeros(1, kw["h"], kw["w"], 32, dtype=torch.float16)
    with pytest.raises(ops.AdmError, match="conv2d: empty output"):
        ops.conv2d(x, torch.zeros(8, 9, 32, dtype=torch.float16), None, 3, 3, kw["stride"])
    with pytest.raises(ops.AdmError, match="pool2d: empty output"):
        ops.pool2d(x, 3, kw["stride"], 0, "max")
