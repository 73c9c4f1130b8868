"""Every launch the Inception-v3 extractor makes (csrc/adm_convg.hip), replayed against float64 in fp16 and bf16.

InceptionV3 runs on oracle.inception.fill_params() weights through the entry points the code base uses -- features ("tf1" and
"pt"), features_all, forward with output blocks 0..3 -- at the batches the evaluator, candidate scoring and bench.py use (320,
256, 100, 64, 1) and at the ADM output sizes (64, 128, 256) plus a non-square 512x509, under tests/inception_replay.Recorder.
Each distinct record is launched again through the same ops entry point with fresh seeded operands and compared element by
element with the float64 restatement of tests/inception_replay.py, within the per-element and Frobenius bounds derived there
(tested on the host by tests/test_inception_replay_host.py).  A coverage guard fails if a family of launches the network is
known to reach is missing.  The LDS-free kernel that ADM_CG_NO_LDS selects replays the batch-100 records in a child process.
Last, one forward of the assembled network at batch 2 with every call's own tensors kept: each layer against the restatement of
that one call on its captured input, and the BatchNorm fold against the oracle parameters.
"""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

import inception_replay as ir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float16, torch.bfloat16)
BATCHES = (320, 256, 100, 64, 1)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import ops as _ops
    return _ops


def _u8(n, h, w, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, device=DEV, dtype=torch.uint8)


def _run_network(dt, p):
    """The extractor through every entry point, at every batch and input size the code base feeds it."""
    from autodiffusion_amd.inception import InceptionV3
    m = InceptionV3(dtype=dt).to(DEV)
    m.load_state_dict(p)
    for n, (h, w) in zip(BATCHES, ((64, 64), (128, 128), (256, 256), (64, 64), (512, 509))):
        m.features(_u8(n, h, w, n))
    m.features(_u8(100, 64, 64, 7), "pt")
    m.features(_u8(1, 512, 509, 8), "pt")
    m.features_all(_u8(320, 256, 256, 9))
    m.features_all(_u8(64, 128, 128, 10), "pt")
    del m
    g = torch.Generator(device=DEV).manual_seed(11)
    for blocks in ([0], [0, 1], [0, 1, 2], [0, 1, 2, 3]):
        f = InceptionV3(blocks, dtype=dt).to(DEV)
        f.load_state_dict(p)
        f(torch.rand((1, 3, 128, 128), generator=g, device=DEV))
        if len(blocks) == 4:
            f(torch.rand((256, 3, 64, 64), generator=g, device=DEV))
            f(torch.rand((64, 3, 512, 509), generator=g, device=DEV))
        del f
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def recorded(ops):
    from oracle import inception as oi
    t0 = time.time()
    p = oi.fill_params()
    with pytest.MonkeyPatch.context() as mp:
        rec = ir.Recorder(mp)
        for dt in DTYPES:
            _run_network(dt, p)
    torch.cuda.synchronize()
    print(f"\nrecorded {sum(rec.counts.values())} calls ({rec.counts}), {len(rec.records)} distinct, in {time.time() - t0:.0f} s")
    for kind in ("f16", "bf16"):
        per = {n: sum(1 for r in rec.records if r[1] == kind and ir.record_dict(r)["n"] == n) for n in BATCHES}
        print(f"{kind}: distinct records per batch {per}")
    return rec


def _of(recorded, op):
    recs = sorted(r for r in recorded.records if r[0] == op)
    assert recs, f"the recorder captured no {op} launch"
    return recs


# ------------------------------------------------------------------ coverage guard
def test_recorded_launches_cover_every_known_family(recorded):
    fams = set()
    for r in recorded.records:
        fams |= ir.families(r)
    for kind in ("f16", "bf16"):
        print(f"{kind}: {len([r for r in recorded.records if r[1] == kind])} distinct launches; families {sorted(f for k, f in fams if k == kind)}")
    missing = [(k, f) for k in ("f16", "bf16") for f in ir.REQUIRED_FAMILIES if (k, f) not in fams]
    assert not missing, f"the extractor no longer reaches (or the recorder missed) {missing}"
    batches = {(r[1], ir.record_dict(r)["n"]) for r in recorded.records if r[0] == "conv2d"}
    assert batches == {(k, n) for k in ("f16", "bf16") for n in BATCHES}, batches
    sizes = {(ir.record_dict(r)["h"], ir.record_dict(r)["w"]) for r in recorded.records if r[0] == "resize"}
    assert sizes >= {(64, 64), (128, 128), (256, 256), (512, 509)}, sizes
    # every op of adm_convg.hip that is recorded is replayed below: a new one must get a restatement, not be dropped
    assert {r[0] for r in recorded.records} <= ir.REPLAYED, {r[0] for r in recorded.records} - ir.REPLAYED


# ------------------------------------------------------------------ replay
def test_conv_launches_match_float64(ops, recorded):
    t0 = time.time()
    recs = _of(recorded, "conv2d")
    fam_worst, fails, replayed = {}, [], 0
    for dt in DTYPES:
        kind = ir.DTYPE_KIND[dt]
        for i, rec in enumerate(r for r in recs if r[1] == kind):
            worst, fro, report = ir.replay_conv(ops, rec, 1000 + i, DEV)
            replayed += 1
            u = ir.U[dt]
            ok = worst <= 1.0 and fro <= ir.fro_bound(1, u)
            print(f"conv2d {ir.conv_label(rec)}: worst err/bound {worst:.3f}, fro/u {fro / u:.3f}{'' if ok else '  FAIL ' + report}")
            for f in ir.families(rec):
                fam_worst[f] = tuple(max(a, b) for a, b in zip(fam_worst.get(f, (0.0, 0.0)), (worst, fro / u)))
            if not ok:
                fails.append((ir.conv_label(rec), worst, fro / u, report))
        torch.cuda.empty_cache()
    for k in ("f16", "bf16"):
        print(f"{k}: {sum(1 for r in recs if r[1] == k)} distinct conv2d launches replayed; worst err/bound "
              f"{max(v[0] for f, v in fam_worst.items() if f[0] == k):.3f}")
    for f in sorted(fam_worst):
        print(f"worst (err/bound, fro/u) {f}: {fam_worst[f][0]:.3f} {fam_worst[f][1]:.3f}")
    print(f"conv2d replay: {replayed} launches, {time.time() - t0:.0f} s")
    assert replayed == len(recs)
    assert not fails, fails


def _simple_replay(name, recs, fn):
    t0 = time.time()
    results = []
    for i, rec in enumerate(recs):
        w = fn(rec, i)
        results.append(max(w) if isinstance(w, tuple) else w)
        print(f"{rec[0]} {rec[1]} {ir.record_dict(rec)}: worst err/bound {w}{'' if results[-1] <= 1.0 else '  FAIL'}")
    for k in ("f16", "bf16"):
        ws = [w for r, w in zip(recs, results) if r[1] == k]
        print(f"worst err/bound ('{k}', '{name}'): {max(ws) if ws else float('nan'):.3f} over {len(ws)} launches")
    print(f"{name} replay: {len(results)} launches, {time.time() - t0:.0f} s")
    assert len(results) == len(recs)
    fails = [(r, w) for r, w in zip(recs, results) if not w <= 1.0]
    assert not fails, fails


def test_pool_launches_match_float64(ops, recorded):
    _simple_replay("pool2d", _of(recorded, "pool2d"), lambda rec, i: ir.replay_pool(ops, rec, 2000 + i, DEV))


def test_global_avgpool_launches_match_float64(ops, recorded):
    _simple_replay("gap", _of(recorded, "gap"), lambda rec, i: ir.replay_gap(ops, rec, 3000 + i, DEV))


def test_resize_launches_match_float64(ops, recorded):
    """The recorded launches (uint8 NHWC, fp32 NCHW), and each fp32 NCHW one again as fp32 NHWC: no entry point of the package
    uses that kind, the library exports it."""
    recs = _of(recorded, "resize")
    nhwc = sorted({ir._rec("resize", r[1], dict(ir.record_dict(r), kind=2)) for r in recs if ir.record_dict(r)["kind"] == 1})
    assert nhwc and {ir.record_dict(r)["kind"] for r in recs} == {0, 1}
    _simple_replay("resize", recs + nhwc, lambda rec, i: ir.replay_resize(ops, rec, 4000 + i, DEV))


# ------------------------------------------------------------------ the LDS-free path
_CHILD = r"""
import json, os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import torch
import inception_replay as ir
from autodiffusion_amd import ops
assert os.environ.get("ADM_CG_NO_LDS") == "1"
recs = [(r[0], r[1]) + tuple((k, v) for k, v in r[2:]) for r in json.load(open(sys.argv[1]))]
bad, top = 0, 0.0
for i, rec in enumerate(recs):
    dt = ir.KIND_DTYPE[rec[1]]
    worst, fro, report = ir.replay_conv(ops, rec, 5000 + i, "cuda:0")
    top = max(top, worst)
    if not (worst <= 1.0 and fro <= ir.fro_bound(1, ir.U[dt])):
        bad += 1
        print(f"FAIL {ir.conv_label(rec)}: worst err/bound {worst:.3f}, fro/u {fro / ir.U[dt]:.3f} {report}")
print(f"REPLAYED {len(recs)} worst {top:.3f}")
sys.exit(1 if bad else 0)
"""


def test_lds_free_kernels_match_float64_in_a_child_process(recorded, tmp_path):
    """ADM_CG_NO_LDS is read once per process: a fresh child replays the batch-100 conv records of both types on convg_kernel<4>
    (and <2>) within the same bounds."""
    t0 = time.time()
    recs = [r for r in _of(recorded, "conv2d") if ir.record_dict(r)["n"] == 100]
    picks = {(r[1], ir.conv_kernel_pick(ir.record_dict(r)["cout"], no_lds=True)) for r in recs}
    assert picks == {(k, f"convg_kernel<{t}>") for k in ("f16", "bf16") for t in (2, 4)}, picks
    path = tmp_path / "records.json"
    path.write_text(json.dumps(recs))
    env = dict(os.environ, ADM_CG_NO_LDS="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ROOT), str(path)], capture_output=True, text=True, timeout=900, env=env,
                       cwd=ROOT)
    print(r.stdout[-4000:])
    print(f"LDS-free replay: {len(recs)} launches, {time.time() - t0:.0f} s")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert f"REPLAYED {len(recs)} " in r.stdout


# ------------------------------------------------------------------ the assembled network, layer by layer
POOLS = ([("max", 3, 2, 0)] * 2 + [("avg", 3, 1, 1)] * 3 + [("max", 3, 2, 0)] + [("avg", 3, 1, 1)] * 4 + [("max", 3, 2, 0)]
         + [("avg", 3, 1, 1), ("max", 3, 1, 1)])   # stem x 2, Mixed_5b-d, 6a, 6b-e, 7a, 7b (average), 7c (the FID graph's max)


@pytest.mark.parametrize("dt", DTYPES)
def test_assembled_network_layer_by_layer(ops, dt):
    from autodiffusion_amd.inception import CONVS, InceptionV3
    from oracle import inception as oi
    t0 = time.time()
    p = oi.fill_params()
    m = InceptionV3([0, 1, 2, 3], dtype=dt).to(DEV)
    m.load_state_dict(p)
    x = torch.rand((2, 3, 96, 80), generator=torch.Generator().manual_seed(15)).to(DEV)
    with pytest.MonkeyPatch.context() as mp:
        rec = ir.Recorder(mp, keep=True)
        m(x)
    torch.cuda.synchronize()
    names = {m._packed[n][0].data_ptr(): n for n in m._packed}
    cins = {c[0]: c[1] for c in CONVS}
    u = ir.U[dt]
    seen, pools, fails, worst_of, fold = [], [], [], {}, {}
    for r, t in rec.calls:
        d = ir.record_dict(r)
        if r[0] == "conv2d":
            name = names[t["w_packed"].data_ptr()]
            seen.append(name)
            oh, ow = ir.conv_out_hw(d)
            worst, fro, report = ir.compare_conv(t["x"], t["w_packed"], t["bias"], d, dt, t["out"], torch.arange(d["n"] * oh * ow))
            werr, pad_zero, berr = ir.fold_errors(t["w_packed"], t["bias"], p, name, dt)
            in_pad_zero = bool((t["x"][..., cins[name]:d["cin_pad"]] == 0).all())
            ok = worst <= 1.0 and fro <= ir.fro_bound(1, u) and werr <= 1.0 and berr <= 1.0 and pad_zero and in_pad_zero and d["cin"] == cins[name]
            print(f"{name} {ir.conv_label(r)}: worst err/bound {worst:.3f}, fro/u {fro / u:.3f}; fold: weights {werr:.3f} ulp, bias "
                  f"{berr:.3f} of its bound{'' if ok else '  FAIL ' + report}")
            res = worst
            fold["weights (ulp_T)"], fold["bias (of its bound)"] = max(fold.get("weights (ulp_T)", 0.0), werr), max(fold.get("bias (of its bound)", 0.0), berr)
        elif r[0] == "pool2d":
            pools.append((d["mode"], d["k"], d["stride"], d["pad"]))
            res = ir.compare_pool(t["x"], d, dt, t["out"])
            ok = res <= 1.0
        elif r[0] == "gap":
            res = ir.compare_gap(t["x"], t["out"])
            ok = res <= 1.0
        else:
            res = ir.compare_resize(t["x"], d, dt, t["out"], range(d["n"]))
            ok = res <= 1.0 and torch.equal(t["x"], x)
        worst_of[r[0]] = max(worst_of.get(r[0], 0.0), res)
        if not ok:
            fails.append((r, res))
    print(f"{dt} layer by layer: worst err/bound per op {worst_of}, fold {fold}, {len(rec.calls)} calls, {time.time() - t0:.0f} s")
    assert sorted(seen) == sorted(c[0] for c in CONVS) and len(seen) == 94
    assert pools == POOLS, pools
    assert set(worst_of) == ir.REPLAYED
    assert not fails, fails
