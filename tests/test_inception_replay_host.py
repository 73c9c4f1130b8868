"""Host checks of tests/inception_replay.py: each float64 restatement against the plain torch op, the pixel sampler, the
kernel-pick function, and the bounds themselves -- they admit a correct implementation (an fp32-accumulate, round-to-nearest
torch emulation of each op stays <= 1.0 of the per-element bound and <= 0.6 u Frobenius) and reject defects (each must exceed
its bound, per element or Frobenius)."""
import pytest
import torch
import torch.nn.functional as F

import inception_replay as ir

F16, BF16 = torch.float16, torch.bfloat16


def D(n, h, w, cin, cout, kh, kw, stride=1, ph=0, pw=0, relu=True, has_bias=True, out_stride=None, out_off=0):
    cp = (cin + 31) // 32 * 32
    return dict(n=n, h=h, w=w, in_stride=cp, cin=cin, cin_pad=cp, cout=cout, kh=kh, kw=kw, stride=stride, ph=ph, pw=pw, relu=relu,
                has_bias=has_bias, out_stride=out_stride or cout, out_off=out_off)


# the network's layer shapes (stem, 3x3 padded, 5x5 on the 48(64)-channel tensor, 1x7, the strided 288 -> 384, the 8x8 level's
# 3x3 and its K = 2048 1x1) on maps and batches that fit a CPU
SHAPES = [D(2, 19, 19, 3, 32, 3, 3, stride=2), D(2, 17, 17, 32, 64, 3, 3, ph=1, pw=1), D(2, 12, 12, 48, 64, 5, 5, ph=2, pw=2),
          D(2, 17, 17, 128, 128, 1, 7, pw=3), D(1, 17, 17, 288, 384, 3, 3, stride=2), D(2, 8, 8, 448, 384, 3, 3, ph=1, pw=1),
          D(2, 8, 8, 2048, 320, 1, 1), D(2, 9, 9, 160, 192, 7, 1, ph=3, relu=False, has_bias=False)]


def operands(d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(d["n"], d["h"], d["w"], d["in_stride"])
    x[..., :d["cin"]] = ir.round_t(torch.randn(d["n"], d["h"], d["w"], d["cin"], generator=g), dtype)
    w32 = torch.randn(d["cout"], d["cin"], d["kh"], d["kw"], generator=g) * (d["cin"] * d["kh"] * d["kw"]) ** -0.5
    scale = 1 + 0.2 * torch.randn(d["cout"], generator=g)
    bias = 0.3 * torch.randn(d["cout"], generator=g) if d["has_bias"] else None
    return x, w32, scale, bias


def truncate_t(v, dtype):
    """fp32 -> T toward zero (as float32)."""
    r = v.to(dtype)
    bits = r.view(torch.int16)
    bits = torch.where(r.float().abs() > v.abs(), bits - 1, bits)   # sign-magnitude: one step toward zero
    return bits.view(dtype).float()


def emulate_conv(x, wq, bias, d, dtype, out_round=None):
    """The kernel's arithmetic in torch: fp32 accumulation of T operands, fp32 bias, ReLU, one rounding to T -> NHWC float32."""
    cout, taps, cp = wq.shape
    w4 = wq.reshape(cout, d["kh"], d["kw"], cp).permute(0, 3, 1, 2).contiguous()
    y = F.conv2d(x[..., :cp].permute(0, 3, 1, 2).contiguous(), w4, bias, stride=d["stride"], padding=(d["ph"], d["pw"]))
    if d["relu"]:
        y = F.relu(y)
    y = y.permute(0, 2, 3, 1).contiguous()
    return (out_round or (lambda v: ir.round_t(v, dtype)))(y)


def all_pixels(d):
    oh, ow = ir.conv_out_hw(d)
    return torch.arange(d["n"] * oh * ow)


# ------------------------------------------------------------------ restatements against the plain torch ops
@pytest.mark.parametrize("d", SHAPES, ids=lambda d: f"{d['cin']}-{d['cout']}-{d['kh']}x{d['kw']}s{d['stride']}")
def test_conv_restatement_is_torch_conv2d(d):
    x, w32, scale, bias = operands(d, F16)
    wq = ir.reference_weights(w32, scale, d["cin_pad"], F16)
    z, s = ir.conv_restate(x, wq, bias, d, all_pixels(d))
    w4 = ir.round_t(w32 * scale.view(-1, 1, 1, 1), F16).double()
    ref = F.conv2d(x[..., :d["cin"]].permute(0, 3, 1, 2).double(), w4, None if bias is None else bias.double(), stride=d["stride"],
                   padding=(d["ph"], d["pw"])).permute(0, 2, 3, 1).reshape(-1, d["cout"])
    assert z.shape == ref.shape
    assert (z - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    sref = F.conv2d(x[..., :d["cin"]].permute(0, 3, 1, 2).double().abs(), w4.abs(), None, stride=d["stride"],
                    padding=(d["ph"], d["pw"])).permute(0, 2, 3, 1).reshape(-1, d["cout"])
    assert (s - sref).abs().max().item() <= 1e-12 * sref.abs().max().item()


@pytest.mark.parametrize("k,stride,pad,mode", [(3, 2, 0, "max"), (3, 1, 1, "avg"), (3, 1, 1, "max"), (2, 2, 0, "avg")])
def test_pool_restatement_is_torch_pooling(k, stride, pad, mode):
    x = ir.round_t(torch.randn(2, 13, 11, 16, generator=torch.Generator().manual_seed(1)), F16)
    ref, bound = ir.pool_restate(x, k, stride, pad, mode, F16)
    xn = x.permute(0, 3, 1, 2).double()
    want = (F.max_pool2d(xn, k, stride, pad) if mode == "max" else F.avg_pool2d(xn, k, stride, pad, count_include_pad=False))
    assert (ref - want.permute(0, 2, 3, 1)).abs().max().item() <= 1e-14
    assert (bound is None) == (mode == "max")


def test_gap_restatement_is_the_mean():
    x = ir.round_t(torch.randn(3, 8, 8, 24, generator=torch.Generator().manual_seed(2)), BF16)
    ref, bound = ir.gap_restate(x)
    assert (ref - x.double().permute(0, 3, 1, 2).mean((2, 3))).abs().max().item() <= 1e-15 and (bound > 0).all()


@pytest.mark.parametrize("size", [(64, 64), (128, 128), (256, 256), (299, 299), (512, 509)])
def test_resize_restatement_is_the_oracle_prepare_in_both_modes(size):
    """fp32 coordinates by the kernel's own expression, float64 interpolation: within fp32 noise (measured 2e-7) of the oracle's fp32
    prepare (F.interpolate / the TensorFlow-1 formula) on outputs in [-1, 1]; a coordinate rounded twice is 1.7e-6 .. 3.6e-6 off."""
    from oracle import inception as oi
    h, w = size
    g = torch.Generator().manual_seed(h)
    u8 = torch.randint(0, 256, (2, h, w, 3), generator=g, dtype=torch.uint8)
    ref, _ = ir.resize_restate(u8, 0, False, 1 / 128.0, -1.0, 299, 299, F16)
    assert (ref.permute(0, 3, 1, 2) - oi.prepare(u8, "tf1").double()).abs().max().item() <= 5e-7
    f = torch.rand((2, 3, h, w), generator=g)
    ref, _ = ir.resize_restate(f, 1, True, 2.0, -1.0, 299, 299, F16)
    assert (ref.permute(0, 3, 1, 2) - oi.prepare(f, "pt").double()).abs().max().item() <= 5e-7
    ref2, _ = ir.resize_restate(f.permute(0, 2, 3, 1).contiguous(), 2, True, 2.0, -1.0, 299, 299, F16)
    assert torch.equal(ref, ref2)


# ------------------------------------------------------------------ sampler, kernel pick, records
@pytest.mark.parametrize("n,oh,ow,cout", [(320, 8, 8, 384), (100, 17, 17, 192), (64, 35, 35, 96), (32, 73, 71, 64)])
def test_sampler_hits_both_ends_of_every_64_run_and_the_border_ring(n, oh, ow, cout):
    m = ir.sample_pixels(n, oh, ow, cout, 5)
    tot = n * oh * ow
    assert tot * cout > ir.FULL_BELOW and m.numel() < tot
    have = set(m.tolist())
    assert all(0 <= v < tot for v in have) and m.tolist() == sorted(have)
    for m0 in range(0, tot, 64):
        assert m0 in have and min(m0 + 63, tot - 1) in have
    for img in ir.ring_images(n, 5):
        for y in range(oh):
            for x in range(ow):
                if y in (0, oh - 1) or x in (0, ow - 1):
                    assert (img * oh + y) * ow + x in have
    assert ir.ring_images(n, 5)[0] == 0 and ir.ring_images(n, 5)[-1] == n - 1
    assert torch.equal(ir.sample_pixels(2, 8, 8, 320, 5), torch.arange(128))   # small: the whole tensor


def test_kernel_pick_agrees_with_a_table_of_the_networks_couts():
    from autodiffusion_amd.inception import CONVS
    table = {32: "convg_kernel<2>", 48: "convg_lds_kernel<4,1>", 64: "convg_lds_kernel<4,1>", 80: "convg_lds_kernel<2,2>",
             96: "convg_lds_kernel<2,2>", 128: "convg_lds_kernel<2,2>", 160: "convg_lds_kernel<4,1>", 192: "convg_lds_kernel<4,1>",
             320: "convg_lds_kernel<4,1>", 384: "convg_lds_kernel<2,2>", 448: "convg_lds_kernel<4,1>"}
    couts = {c[2] for c in CONVS}
    assert couts == set(table)
    for c in couts:
        assert ir.conv_kernel_pick(c) == table[c], c
        assert ir.conv_kernel_pick(c, no_lds=True) == ("convg_kernel<2>" if c == 32 or (c + 31) // 32 % 2 else "convg_kernel<4>"), c
    assert ir.conv_kernel_pick(192, no_lds=True) == "convg_kernel<4>" and ir.conv_kernel_pick(96, no_lds=True) == "convg_kernel<2>"


def test_families_of_a_record():
    rec = ir._rec("conv2d", "f16", D(100, 35, 35, 192, 48, 1, 1, out_stride=64))
    assert ir.families(rec) == {("f16", f) for f in ("convg_lds_kernel<4,1>", "1x1", "cout 48", "sliced output", "M % 256 != 0")}
    assert ir.record_dict(rec)["out_stride"] == 64 and hash(rec) is not None


# ------------------------------------------------------------------ the bounds admit a correct implementation
@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("d", SHAPES, ids=lambda d: f"{d['cin']}-{d['cout']}-{d['kh']}x{d['kw']}s{d['stride']}")
def test_conv_bounds_admit_the_fp32_emulation(d, dtype):
    x, w32, scale, bias = operands(d, dtype)
    wq = ir.reference_weights(w32, scale, d["cin_pad"], dtype)
    worst, fro, _ = ir.compare_conv(x, wq, bias, d, dtype, emulate_conv(x, wq, bias, d, dtype), all_pixels(d))
    print(f"{dtype} {d['cin']}->{d['cout']} {d['kh']}x{d['kw']}: worst err/bound {worst:.3f}, fro/u {fro / ir.U[dtype]:.3f}")
    assert worst <= 1.0 and fro <= ir.fro_bound(1, ir.U[dtype])


def emulate_avgpool(x, k, stride, pad, dtype, include_pad=False):
    y = F.avg_pool2d(x.permute(0, 3, 1, 2).float(), k, stride, pad, count_include_pad=include_pad).permute(0, 2, 3, 1)
    return ir.round_t(y, dtype)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_pool_and_gap_bounds_admit_the_fp32_emulation(dtype):
    x = ir.round_t(torch.randn(2, 17, 15, 32, generator=torch.Generator().manual_seed(3)), dtype)
    for k, stride, pad in ((3, 1, 1), (2, 2, 0)):
        d = dict(n=2, h=17, w=15, c=32, k=k, stride=stride, pad=pad, mode="avg")
        assert ir.compare_pool(x, d, dtype, emulate_avgpool(x, k, stride, pad, dtype)) <= 1.0
    d = dict(n=2, h=17, w=15, c=32, k=3, stride=2, pad=0, mode="max")
    assert ir.compare_pool(x, d, dtype, F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 0).permute(0, 2, 3, 1)) == 0.0
    x[..., 5] = 0                                                     # a channel ReLU has emptied: bound 0, result exactly 0
    assert ir.compare_gap(x, x.float().mean((1, 2))) <= 1.0
    assert ir.compare_gap(x, x.float().mean((1, 2)) + 1e-6) == float("inf")


def emulate_resize(images, kind, half_pixel, scale, shift, oh, ow, dtype, coord_shift=0.0):
    """The kernel's fp32 arithmetic in torch: fp32 coordinates, the two lerps, scale and shift, one rounding to T."""
    px = (images.permute(0, 2, 3, 1) if kind == 1 else images).float()

    def coords(size_in, size_out):
        i0, i1, f = ir.resize_coords(size_in, size_out, half_pixel, px.device)
        if coord_shift:
            s = (i0.float() + f.float() + coord_shift).clamp_min(0.0)
            i0 = s.to(torch.int64).clamp(max=size_in - 1)
            i1, f = (i0 + 1).clamp(max=size_in - 1), s - i0.float()
        return i0, i1, f.float()
    y0, y1, fy = coords(px.shape[1], oh)
    x0, x1, fx = coords(px.shape[2], ow)
    fy, fx = fy.view(1, -1, 1, 1), fx.view(1, 1, -1, 1)
    top = px[:, y0][:, :, x0] * (1 - fx) + px[:, y0][:, :, x1] * fx
    bot = px[:, y1][:, :, x0] * (1 - fx) + px[:, y1][:, :, x1] * fx
    v = (top * (1 - fy) + bot * fy) * torch.tensor(scale, dtype=torch.float32) + torch.tensor(shift, dtype=torch.float32)
    return F.pad(ir.round_t(v, dtype), (0, 29))


RESIZES = [dict(n=2, h=64, w=64, kind=0, half_pixel=False, scale=1 / 128.0, shift=-1.0),
           dict(n=1, h=512, w=509, kind=0, half_pixel=True, scale=2 / 255.0, shift=-1.0),
           dict(n=2, h=256, w=256, kind=1, half_pixel=True, scale=2.0, shift=-1.0),
           dict(n=1, h=128, w=131, kind=2, half_pixel=False, scale=2.0, shift=-1.0)]


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("d", RESIZES, ids=lambda d: f"{d['h']}-kind{d['kind']}-{'hp' if d['half_pixel'] else 'tf1'}")
def test_resize_bound_admits_the_fp32_emulation(d, dtype):
    d = dict(d, oh=299, ow=299, cpad=32)
    for constant in (False, True):
        images = ir.resize_images(d, constant, 4, "cpu")
        got = emulate_resize(images, d["kind"], d["half_pixel"], d["scale"], d["shift"], 299, 299, dtype)
        assert ir.compare_resize(images, d, dtype, got, range(d["n"])) <= 1.0


# ------------------------------------------------------------------ ... and reject defects
REJECT = D(2, 35, 35, 288, 384, 3, 3, stride=2)   # the layer the issue measured the old tolerance on


def _conv_case(dtype=F16, d=REJECT):
    x, w32, scale, bias = operands(d, dtype)
    return x, w32, scale, bias, ir.reference_weights(w32, scale, d["cin_pad"], dtype)


def _rejected(worst, fro, dtype=F16):
    return worst > 1.0 or fro > ir.fro_bound(1, ir.U[dtype])


def test_rejects_an_output_rounded_through_bf16_in_an_fp16_run():
    x, _, _, bias, wq = _conv_case()
    out = emulate_conv(x, wq, bias, REJECT, F16, out_round=lambda v: ir.round_t(ir.round_t(v, BF16), F16))
    worst, fro, _ = ir.compare_conv(x, wq, bias, REJECT, F16, out, all_pixels(REJECT))
    assert worst > 1.0 and fro > ir.fro_bound(1, ir.U[F16]), (worst, fro / ir.U[F16])


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_rejects_a_truncated_output(dtype):
    """Truncation stays inside the per-element bound (its error is below one ulp_T): the Frobenius bound catches it."""
    x, _, _, bias, wq = _conv_case(dtype)
    out = emulate_conv(x, wq, bias, REJECT, dtype, out_round=lambda v: truncate_t(v, dtype))
    worst, fro, _ = ir.compare_conv(x, wq, bias, REJECT, dtype, out, all_pixels(REJECT))
    print(f"truncation {dtype}: worst err/bound {worst:.3f}, fro/u {fro / ir.U[dtype]:.3f}")
    assert fro > ir.fro_bound(1, ir.U[dtype])


def test_rejects_weights_packed_through_bf16():
    x, w32, scale, bias, wq = _conv_case()
    wbad = ir.round_t(ir.reference_weights(w32, scale, REJECT["cin_pad"], BF16), F16)
    worst, fro, _ = ir.compare_conv(x, wq, bias, REJECT, F16, emulate_conv(x, wbad, bias, REJECT, F16), all_pixels(REJECT))
    assert _rejected(worst, fro), (worst, fro / ir.U[F16])
    assert fro > ir.fro_bound(1, ir.U[F16])


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_packing_check_admits_both_correct_roundings_and_rejects_truncation_and_bf16(dtype):
    g = torch.Generator().manual_seed(9)
    w32, scale = torch.randn(96, 48, 3, 3, generator=g) * 0.05, 1 + 0.2 * torch.randn(96, generator=g)
    twice = ir.reference_weights(w32, scale, 64, dtype).to(dtype)                       # fl32(w s), then to T
    exact = (w32.double() * scale.double().view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(96, 9, 48)
    up, down = twice.clone(), twice.clone()                                             # the T neighbours of `twice`
    bits = twice.view(torch.int16)
    up, down = (bits + 1).view(dtype), (bits - 1).view(dtype)
    cands = torch.stack([t[..., :48].double() for t in (down, twice, up)])
    once = torch.gather(cands, 0, (cands - exact).abs().argmin(0, keepdim=True))[0]     # the nearest T value of the exact product
    once = torch.cat([once.to(dtype), twice[..., 48:]], 2)
    assert ir.packing_errors(twice, w32, scale, dtype) == 0 and ir.packing_errors(once, w32, scale, dtype) == 0
    print(f"{dtype}: one rounding differs from two on {int((once != twice).sum())} of {exact.numel()} weights")
    trunc = torch.cat([truncate_t(exact.float(), dtype).to(dtype), twice[..., 48:]], 2)
    assert ir.packing_errors(trunc, w32, scale, dtype) > exact.numel() // 4
    one_off = twice.clone()
    one_off[5, 3, 7] = up[5, 3, 7] if (up[5, 3, 7].double() - exact[5, 3, 7]).abs() > (down[5, 3, 7].double() - exact[5, 3, 7]).abs() else down[5, 3, 7]
    assert ir.packing_errors(one_off, w32, scale, dtype) == 1                           # one weight, one ulp: no slack
    pad = twice.clone()
    pad[0, 0, 50] = 1e-3
    assert ir.packing_errors(pad, w32, scale, dtype) == 1
    if dtype == F16:
        through_bf16 = ir.reference_weights(w32, scale, 64, BF16).to(F16)
        assert ir.packing_errors(through_bf16, w32, scale, F16) > exact.numel() // 2


@pytest.mark.parametrize("d", [D(2, 17, 17, 128, 128, 1, 7, pw=3), D(2, 8, 8, 448, 384, 3, 3, ph=1, pw=1), REJECT],
                         ids=["1x7", "3x3", "3x3s2"])
def test_rejects_one_tap_dropped_at_one_border_pixel_of_one_image(d):
    """A single (pixel, tap) lost -- an off-by-one in the window test at the map's edge -- must exceed the per-element bound there:
    the Frobenius norm does not see one pixel."""
    x, _, _, bias, wq = _conv_case(F16, d)
    out = emulate_conv(x, wq, bias, d, F16)
    oh, ow = ir.conv_out_hw(d)
    img, oy, ox, tap = d["n"] - 1, oh - 1, ow // 2, 0          # last row of the last image; tap (ky 0, kx 0) lies in the image
    iy, ix = oy * d["stride"] - d["ph"], ox * d["stride"] - d["pw"]
    assert 0 <= iy < d["h"] and 0 <= ix < d["w"]
    m = torch.tensor([(img * oh + oy) * ow + ox])
    z, _ = ir.conv_restate(x, wq, bias, d, m)
    contrib = wq[:, tap, :].double() @ x[img, iy, ix, :d["cin_pad"]].double()
    bad = (z[0] - contrib).clamp_min(0) if d["relu"] else z[0] - contrib
    out[img, oy, ox] = ir.round_t(bad.float(), F16)
    worst, fro, report = ir.compare_conv(x, wq, bias, d, F16, out, ir.sample_pixels(d["n"], oh, ow, 1 << 22, 0))
    assert worst > 1.0, (worst, report)
    assert f"img {img} y {oy} x {ox}" in report


def test_rejects_a_slice_shifted_by_four_channels():
    d = D(2, 8, 8, 64, 96, 1, 1, out_stride=256, out_off=128)
    x, _, _, bias, wq = _conv_case(F16, d)
    good = emulate_conv(x, wq, bias, d, F16)
    for shift, ok in ((0, True), (4, False)):
        parent = torch.full((2, 8, 8, 256), ir.SENTINEL, dtype=F16)
        parent[..., 128 + shift:224 + shift] = good.to(F16)
        assert ir.sentinel_intact(parent, 128, 96) == ok
        worst, fro, _ = ir.compare_conv(x, wq, bias, d, F16, parent[..., 128:224], all_pixels(d))
        assert (worst <= 1.0 and fro <= ir.fro_bound(1, ir.U[F16])) == ok


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_rejects_count_include_pad_and_a_wrong_max(dtype):
    x = ir.round_t(torch.randn(2, 8, 8, 16, generator=torch.Generator().manual_seed(6)), dtype)
    d = dict(n=2, h=8, w=8, c=16, k=3, stride=1, pad=1, mode="avg")
    assert ir.compare_pool(x, d, dtype, emulate_avgpool(x, 3, 1, 1, dtype, include_pad=True)) > 1.0
    d["mode"] = "max"
    good = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()
    assert ir.compare_pool(x, d, dtype, good) == 0.0
    good[1, 7, 7, 3] = ir.round_t(good[1, 7, 7, 3] * (1 + 2 * ir.U[dtype]), dtype) + (good[1, 7, 7, 3] == 0) * 1e-3   # one ulp off
    assert ir.compare_pool(x, d, dtype, good) > 1.0
    assert ir.compare_pool(x, dict(d, mode="avg"), dtype, good) > 1.0   # a max where the network averages (Mixed_7b / 7c)


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("d", RESIZES, ids=lambda d: f"{d['h']}-kind{d['kind']}-{'hp' if d['half_pixel'] else 'tf1'}")
def test_rejects_the_other_resize_convention_and_a_shifted_coordinate(d, dtype):
    d = dict(d, oh=299, ow=299, cpad=32)
    images = ir.resize_images(d, False, 4, "cpu")
    other = emulate_resize(images, d["kind"], not d["half_pixel"], d["scale"], d["shift"], 299, 299, dtype)
    assert ir.compare_resize(images, d, dtype, other, range(d["n"])) > 1.0
    moved = emulate_resize(images, d["kind"], d["half_pixel"], d["scale"], d["shift"], 299, 299, dtype, coord_shift=0.5)
    assert ir.compare_resize(images, d, dtype, moved, range(d["n"])) > 1.0
    good = emulate_resize(images, d["kind"], d["half_pixel"], d["scale"], d["shift"], 299, 299, dtype)
    good[0, 5, 5, 7] = 1e-3                                         # a pad channel that is not exactly zero
    assert ir.compare_resize(images, d, dtype, good, range(d["n"])) == float("inf")


def test_fold_check_admits_the_fp32_fold_and_rejects_a_bf16_one():
    from autodiffusion_amd.inception import BN_EPS
    g = torch.Generator().manual_seed(8)
    name = "L"
    p = {name + ".conv.weight": torch.randn(96, 48, 3, 3, generator=g) * 0.05, name + ".bn.weight": 1 + 0.2 * torch.randn(96, generator=g),
         name + ".bn.bias": 0.1 * torch.randn(96, generator=g), name + ".bn.running_mean": 0.1 * torch.randn(96, generator=g),
         name + ".bn.running_var": 1 + 0.5 * torch.rand(96, generator=g)}
    scale = p[name + ".bn.weight"] / torch.sqrt(p[name + ".bn.running_var"] + BN_EPS)          # inception.py's fp32 fold
    bias = p[name + ".bn.bias"] - p[name + ".bn.running_mean"] * scale
    for dtype in (F16, BF16):
        wq = ir.reference_weights(p[name + ".conv.weight"], scale, 64, dtype).to(dtype)
        werr, pad_zero, berr = ir.fold_errors(wq, bias, p, name, dtype)
        assert werr <= 1.0 and pad_zero and berr <= 1.0, (werr, berr)
    wbad = ir.round_t(ir.reference_weights(p[name + ".conv.weight"], scale, 64, BF16), F16).to(F16)
    assert ir.fold_errors(wbad, bias, p, name, F16)[0] > 1.0
    assert ir.fold_errors(wq, bias * (1 + 1e-5), p, name, BF16)[2] > 1.0
    wq[3, 2, 50] = 1e-3
    assert not ir.fold_errors(wq, bias, p, name, BF16)[1]
