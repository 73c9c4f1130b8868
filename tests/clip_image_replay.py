"""float64 restatement of adm_resize_bilinear's bicubic mode (half_pixel == 2: torch F.interpolate(mode="bicubic",
align_corners=True)) with a per-element bound, in the style of tests/inception_replay.py::resize_restate; shared by
tests/test_clip_image_host.py (the restatement against torch's CPU interpolate, named defects outside the bound) and
tests/test_hip_clip_image.py (the kernel against the restatement).

The coordinate is the kernel's own fp32 value: r = fl((in - 1) / (out - 1)) (0 where out == 1), s = fl(o r), i = floor(s),
t = s - i (exact).  Everything after it -- the cubic convolution coefficients with A = -0.75, the sixteen border-clamped taps,
value * scale + shift -- is float64.

Bound, u32 = 2^-24, derived and not measured:
  one rounding to the 16-bit output                                    0.5 ulp_T(ref)
  a coefficient in fp32: t + 1, 1 - t, 2 - t round once (<= u32 each, |dc/dx| <= 1.25 on the four pieces), then five Horner
  operations on intermediates below 8 (half an ulp there: 4 u32), the first ones doubled twice by the multiplications with
  x <= 2: 4 u32 (4 + 4 + 2 + 2 + 1) + 1.25 u32 < DC = 54 u32 per coefficient
  sum |c| <= S1 = 1.375 per axis (t = 1 / 2: 2 (0.59375 + 0.09375)), so eight perturbed coefficients move the value by at most
  2 * 4 * S1 * DC * max|p|  (second order: 16 DC^2, below 1e-11)
  the 16 products and their two-level accumulation: <= 9 roundings on the way of any term (1 + 3 in the row, 1 + 4 across the
  rows): 9 u32 * sum |cy cx p| <= 9 u32 S1^2 max|p|
  scale and shift: 2 u32 (|scale| S1^2 max|p| + |shift|)
"""
import torch

from launch_replay import ulp_t

U32 = 2.0 ** -24
DC = 54.0 * U32
S1 = 1.375


def cubic_coeffs(t, a=-0.75):
    """float64 [.., 4]: weights of the taps floor(s) - 1 .. floor(s) + 2 at the fraction t."""
    def inner(x):
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0

    def outer(x):
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    return torch.stack([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)], dim=-1)


def bicubic_coords(size_in: int, size_out: int, dev, align_corners=True):
    """(floor index int64 [out], fraction float64 [out]) from the fp32 coordinate the kernel computes."""
    f32 = torch.float32
    o = torch.arange(size_out, dtype=f32, device=dev)
    if align_corners:
        r = (torch.tensor(float(size_in - 1), dtype=f32, device=dev) / torch.tensor(float(size_out - 1), dtype=f32, device=dev)
             if size_out > 1 else torch.zeros((), dtype=f32, device=dev))
        s = o * r
    else:   # the defect: half-pixel centres (bicubic does not clamp them at 0)
        s = (o + 0.5) * (torch.tensor(float(size_in), dtype=f32, device=dev) / float(size_out)) - 0.5
    i = torch.floor(s)
    return i.to(torch.int64), (s - i).double()


def bicubic_restate(images, kind: int, scale: float, shift: float, oh: int, ow: int, dtype, a=-0.75, align_corners=True,
                    clamp=True):
    """float64 bicubic resize of 3-channel images (kind 0: uint8 NHWC, 1: fp32 NCHW, 2: fp32 NHWC) -> (ref, bound) [n, oh, ow, 3].
    ``a``, ``align_corners`` and ``clamp`` (False: taps beyond the border read zero) exist to state the defects the bound excludes."""
    px = (images.permute(0, 2, 3, 1) if kind == 1 else images).double()
    dev = px.device
    h, w = px.shape[1], px.shape[2]
    iy, ty = bicubic_coords(h, oh, dev, align_corners)
    ix, tx = bicubic_coords(w, ow, dev, align_corners)
    cy, cx = cubic_coeffs(ty, a), cubic_coeffs(tx, a)          # [oh, 4], [ow, 4]
    ref = torch.zeros((px.shape[0], oh, ow, 3), dtype=torch.float64, device=dev)
    for i in range(4):
        yi = iy - 1 + i
        row_ok = ((yi >= 0) & (yi < h)).double() if not clamp else torch.ones_like(ty)
        rows = px[:, yi.clamp(0, h - 1)]                        # [n, oh, w, 3]
        acc = torch.zeros_like(ref)
        for j in range(4):
            xj = ix - 1 + j
            col_ok = ((xj >= 0) & (xj < w)).double() if not clamp else torch.ones_like(tx)
            acc = acc + rows[:, :, xj.clamp(0, w - 1)] * (cx[:, j] * col_ok).view(1, 1, -1, 1)
        ref = ref + acc * (cy[:, i] * row_ok).view(1, -1, 1, 1)
    sc = torch.tensor(scale, dtype=torch.float32).double().item()     # the kernel takes fp32 scale and shift
    sh = torch.tensor(shift, dtype=torch.float32).double().item()
    ref = ref * sc + sh
    pmax = px.abs().max().item()
    fp32 = (8 * S1 * DC + 16 * DC * DC + 9 * U32 * S1 * S1) * abs(sc) * pmax + 2 * U32 * (abs(sc) * S1 * S1 * pmax + abs(sh))
    return ref, 0.5 * ulp_t(ref, dtype) + fp32
