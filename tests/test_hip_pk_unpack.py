"""The fp32 transforms inside the MFMA loops: adm_conv's GroupNorm affine (+ SiLU) prologue on the 8-wave tiles (prologue 1, 2
and the skip-connection fold), which runs as single-issue fp32 instructions, and the P / dS step of adm_attention_bwd, which
was measured in that form too and stayed packed (profiles/pk_unpack/README.md), in both torsos.

Each case launches the library symbol on guarded operands (tests/guarded.py), compares every output element with the float64
restatement of tests/launch_replay.py within its per-element bound and its Frobenius bound, and launches a second time into a
second output that must equal the first bit for bit.

Conv: the affine differs between the images of a launch (a tile that holds two images must give each its own table), and b is
large, about 3: a padding pixel that went through the transform would enter the taps as SiLU(b) ~ 3 (b for prologue 1) instead
of 0, and every border output would miss its bound by orders of magnitude -- the restatement pads with exact zeros.
test_conv_padding_stays_exactly_zero reads the staged padding out directly, through one-hot weights.  Shapes,
the smallest at which this code can go wrong:
  N=2 16x16 32 -> 32     one 256-pixel tile per image, zero padding on all four sides, one K chunk
  N=2 16x16 96 -> 192    three chunks: an odd count through the double-buffered halo, on the 192-wide tile
  N=3  8x8  64 -> 128    128-pixel tiles of two images: the last tile holds one real and one absent image, and the last
                         staging pass has spare slots
  N=1 32x32 64 -> 128    four tiles with interior halos
  fold: N=2 16x16 64 -> 64 with a 32-channel skip connection folded in (fold0)
Attention backward, D=64, n=2: T=64 with 1 head (one tile), T=80 with 2 heads (ragged last tile), T=256 with 2 heads, in both
qkv orders.
"""
import pytest
import torch

import guarded as gd
import launch_replay as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TYPES = [torch.bfloat16, torch.float16]
_ids = {torch.bfloat16: "bf16", torch.float16: "f16"}

CONV_SHAPES = [
    # label, n, hw, cin, cout
    ("one tile", 2, 16, 32, 32),
    ("odd chunks 192-wide", 2, 16, 96, 192),
    ("absent image", 3, 8, 64, 128),
    ("four tiles", 1, 32, 64, 128),
]
ATTN_BWD_CASES = [(64, 1), (80, 2), (256, 2)]   # (t, heads), D = 64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodiffusion_amd import ops as _ops
    return _ops


def _conv_twice(ops, d, T, seed):
    """The case launched twice on guarded operands -> (worst err / bound over EVERY output pixel, the same over the border pixels
    alone, relative Frobenius error, second launch bitwise equal)."""
    g = gd.Guarded(DEV)
    t, packed, w32p, out = gd.conv_operands(ops, d, T, seed, DEV, g)
    n, cin = d["n"], d["c0"] + d["c1"]
    # per-image affine with a large b (in place: the operands are carves)
    t["b"].copy_(3.0 + 0.5 * torch.randn(n, cin, device=DEV))
    assert not torch.equal(t["a"][0], t["a"][-1]) or n == 1
    out2 = g.out("out (second launch)", tuple(out.shape), T, gd.margin_rows(d["cout"]))
    be = gd.Hip(ops)
    be.conv(d, T, t, packed, w32p, out, g)
    be.conv(d, T, t, packed, w32p, out2, g)
    g.check()
    h, w = d["h"], d["w"]
    img, oy, ox = (v.reshape(-1) for v in torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing="ij"))
    ref, bound = lr.conv_restate(d, T, t, img, oy, ox)
    got = out[img.to(DEV), oy.to(DEV), ox.to(DEV)].double()
    assert torch.isfinite(got).all(), d["label"]
    err = (got - ref).abs()
    ratio = (err / bound).amax(1)
    border = ((oy == 0) | (oy == h - 1) | (ox == 0) | (ox == w - 1)).to(DEV)
    fro = ((err ** 2).sum() / (ref ** 2).sum()).sqrt().item()
    return ratio.max().item(), ratio[border].max().item(), fro, torch.equal(out.view(torch.int16), out2.view(torch.int16))


def _hold_conv(ops, d, T, seed):
    worst, worst_border, fro, same = _conv_twice(ops, d, T, seed)
    u = lr.U[T]
    print(f"{d['label']} {_ids[T]}: worst err/bound {worst:.3f} (border pixels {worst_border:.3f}), fro/u {fro / u:.3f}, "
          f"second launch {'bitwise equal' if same else 'DIFFERS'}")
    assert worst <= 1.0, (d["label"], worst, worst_border)
    assert fro <= lr.fro_bound(lr.conv_roundings(d), u), (d["label"], fro / u)
    assert same, d["label"]


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("prologue", [1, 2], ids=["affine", "affine+silu"])
@pytest.mark.parametrize("label,n,hw,cin,cout", CONV_SHAPES, ids=[c[0] for c in CONV_SHAPES])
def test_conv_prologue_single_issue(ops, label, n, hw, cin, cout, prologue, T):
    d = gd.conv_dict(f"3x3 pro{prologue} {label} n{n} {hw}x{hw} {cin}->{cout}", n, hw, hw, cin, cout, taps=9, prologue=prologue)
    _hold_conv(ops, d, T, 31 + prologue)


PAD_SHAPES = [("one tile", 2, 16, 32, 32), ("absent image", 3, 8, 64, 128)]


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("prologue", [1, 2], ids=["affine", "affine+silu"])
@pytest.mark.parametrize("label,n,hw,cin,cout", PAD_SHAPES, ids=[c[0] for c in PAD_SHAPES])
def test_conv_padding_stays_exactly_zero(ops, label, n, hw, cin, cout, prologue, T):
    """The staged halo read out directly: output channel co has one weight, 1.0, at input channel co % cin of tap co % 9, and no
    bias, so out[pixel, co] IS the transformed value the kernel staged at pixel + tap (one exact product, rounded back to the
    type it already has).  With a = 0 every in-image pixel transforms to act(b), b ~ 3, whatever x holds; a tap that falls
    outside the image must read an exact zero, where a transformed pad would read act(b) too."""
    d = gd.conv_dict(f"3x3 pro{prologue} padding probe {label}", n, hw, hw, cin, cout, taps=9, prologue=prologue)
    g = gd.Guarded(DEV)
    t, packed, w32p, out = gd.conv_operands(ops, d, T, 43, DEV, g)
    co = torch.arange(cout, device=DEV)
    w = torch.zeros(cout, cin, 3, 3, device=DEV)
    w[co, co % cin, (co % 9) // 3, (co % 9) % 3] = 1.0
    packed.copy_(ops.pack_conv_weight(w, T))
    t["bias"].zero_()
    t["a"].zero_()
    t["b"].copy_(3.0 + 0.5 * torch.rand(n, cin, device=DEV))
    gd.Hip(ops).conv(d, T, t, packed, w32p, out, g)
    g.check()
    yy, xx = torch.meshgrid(torch.arange(hw, device=DEV), torch.arange(hw, device=DEV), indexing="ij")
    ty, tx = yy[:, :, None] + (co % 9) // 3 - 1, xx[:, :, None] + (co % 9) % 3 - 1          # [hw, hw, cout]: the tap's source pixel
    outside = ((ty < 0) | (ty >= hw) | (tx < 0) | (tx >= hw))[None].expand(n, -1, -1, -1)
    o = out.float()
    assert outside.any() and (~outside).any()
    print(f"{d['label']} {_ids[T]}: {int(outside.sum())} padding taps, max |value| there {o[outside].abs().max().item():g}; "
          f"min |value| of the in-image taps {o[~outside].abs().min().item():.3f}")
    assert (o[outside] == 0).all(), d["label"]
    assert (o[~outside].abs() > 2.0).all(), d["label"]    # the probe is live: act(b) >= silu(3) = 2.86 (b itself for prologue 1)


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
def test_conv_fold_prologue_single_issue(ops, T):
    d = gd.conv_dict("3x3 pro2 + fold n2 16x16 64->64 skip 32", 2, 16, 16, 64, 64, taps=9, prologue=2, fc0=32)
    _hold_conv(ops, d, T, 37)


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("new_order", [False, True], ids=["legacy", "new_order"])
@pytest.mark.parametrize("t,heads", ATTN_BWD_CASES)
def test_attention_bwd_single_issue(ops, t, heads, new_order, T):
    n, d, c = 2, 64, heads * 64
    be = gd.Hip(ops)
    g = gd.Guarded(DEV)
    torch.manual_seed(41 + t)
    qkv = g.inp("qkv", torch.randn(n, t, 3 * c, device=DEV).to(T), gd.margin_rows(3 * c))
    dout = g.inp("dout", torch.randn(n, t, c, device=DEV).to(T), gd.margin_rows(c))
    out = g.out("out", (n, t, c), T, gd.margin_rows(c))
    lse = g.out("lse", (n, heads, t), gd.F32)
    be.attention_lse(qkv, out, lse, heads, d, new_order)
    g.check()
    g2 = gd.Guarded(DEV)
    o_in, lse_in = g2.inp("out", out, gd.margin_rows(c)), g2.inp("lse", lse)
    runs = []
    for k in range(2):
        delta = g2.out(f"delta_ws {k}", (n, heads, t), gd.F32)
        dqkv = g2.out(f"dqkv {k}", (n, t, 3 * c), T, gd.margin_rows(3 * c))
        be.attention_bwd(qkv, o_in, dout, lse_in, delta, dqkv, heads, d, new_order)
        runs.append((delta, dqkv))
    g.check()
    g2.check()
    worst = gd.compare_attention_bwd(qkv, o_in, dout, runs[0][1], heads, new_order, T, range(n))
    same = (torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))
            and torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)))
    print(f"adm_attention_bwd t {t} heads {heads} new_order {new_order} {_ids[T]}: worst err/bound {worst:.3f}, "
          f"second launch {'bitwise equal' if same else 'DIFFERS'}")
    assert worst <= 1.0, (t, heads, new_order, worst)
    assert same, (t, heads, new_order)
