"""adm_conv, the attention kernels and the GroupNorm kernels at their tile edges, launched through the library symbols on guarded
operands (tests/guarded.py), in both torsos.

Every pointer a kernel takes -- activations, packed weights, bias, affine, residual, fold operands, fused statistics, split-K
workspace, lse, delta_ws, GroupNorm partial sums, statistics and k1 / k0 -- is a carve: outputs start as NaN between sentinel
margins, inputs lie between NaN margins.  After the launch the margins are intact, every output element is finite, and the result
is within the bounds of tests/launch_replay.py against its float64 restatements (every element on maps of <= 256 pixels).  The
persistent-walk cases give the tile loops of the staged and the LDS-resident conv kernels more tiles than one round of blocks and
a partly filled last round.  tests/test_guarded_host.py holds the same cases, and the defects the carves must catch, on the host.

Not seen here: an over-read whose value is discarded (see tests/guarded.py).
"""
import pytest
import torch

import guarded as gd
import launch_replay as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TYPES = [torch.bfloat16, torch.float16]
_ids = {torch.bfloat16: "bf16", torch.float16: "f16"}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import ops as _ops
    return _ops


def _hold(label, T, result):
    worst, fro, ok = result
    u = lr.U[T]
    print(f"{label} {_ids[T]}: worst err/bound {worst:.3f}" + ("" if fro is None else f", fro/u {fro / u:.3f}"))
    assert ok, (label, worst, None if fro is None else fro / u)


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("case", gd.CONV_CASES, ids=lambda d: d["label"])
def test_conv_guarded(ops, case, T):
    _hold(case["label"], T, gd.run_conv(gd.Hip(ops), ops, case, T, DEV, 11))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("which", [0, 1, 2], ids=["staged 3x3", "staged 1x1 at 8x8", "resident 1x1"])
def test_conv_persistent_walk(ops, which, T):
    """More tiles than one round of the persistent grid, and a last round that is partly filled: the tile switch, the next-tile
    fetch and the exit of a block that finds no further tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case, tiles, slots = gd.walk_cases(cus)[which]
    # a condition, not a measurement: the staged kernels hold at most 2 blocks per CU, the resident kernel one
    assert tiles > slots and tiles % slots != 0 and tiles % cus != 0, (tiles, slots, cus)
    print(f"{case['label']}: {tiles} tiles on {cus} CUs (n {case['n']})")
    _hold(case["label"], T, gd.run_conv(gd.Hip(ops), ops, case, T, DEV, 12))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("t,heads,d,new_order", gd.ATTN_LSE_CASES)
def test_attention_lse_guarded(ops, t, heads, d, new_order, T):
    _hold(f"adm_attention_lse t {t} heads {heads} d {d} new_order {new_order}", T,
          gd.run_attention_lse(gd.Hip(ops), 2, t, heads, d, new_order, T, DEV, 13 + t))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("label,tq,tk,rows,heads,d,alias", gd.ATTN_CROSS_CASES, ids=[c[0] for c in gd.ATTN_CROSS_CASES])
def test_attention_cross_guarded(ops, label, tq, tk, rows, heads, d, alias, T):
    _hold("adm_attention_cross " + label, T, gd.run_attention_cross(gd.Hip(ops), 2, tq, tk, rows, heads, d, alias, T, DEV, 14))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("t", gd.ATTN_1H512_T)
def test_attention_1h512_guarded(ops, t, T):
    _hold(f"adm_attention_1h512 t {t}", T, gd.run_attention_1h512(gd.Hip(ops), 2, t, T, DEV, 15 + t))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("t,heads,d", gd.ATTN_BWD_CASES)
def test_attention_bwd_guarded(ops, t, heads, d, T):
    _hold(f"adm_attention_bwd t {t} heads {heads} d {d}", T, gd.run_attention_bwd(gd.Hip(ops), 2, t, heads, d, True, T, DEV, 16 + t))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("case", gd.GN_FWD_CASES, ids=[c[0] for c in gd.GN_FWD_CASES])
def test_groupnorm_forward_guarded(ops, case, T):
    label, mode, n, h, w, c0, c1, film_pad, slabs = case
    slabs = gd.gn_slabs(h * w) if slabs is None else slabs
    _hold("GroupNorm " + label, T, gd.run_gn_forward(gd.Hip(ops), mode, n, h, w, c0, c1, film_pad, slabs, T, DEV, 17))


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("case", gd.GN_BWD_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_groupnorm_backward_guarded(ops, case, T):
    n, h, w, c, dy_half, has_add, add_half, silu, norm_add = case
    _hold(f"GroupNorm backward {case}", T,
          gd.run_gn_backward(gd.Hip(ops), n, h, w, c, silu, dy_half, has_add, add_half, norm_add, T, DEV, 18))
