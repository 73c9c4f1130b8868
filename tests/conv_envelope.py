"""The envelope of adm_conv: every kernel family at every map shape of a grid, most of which no model launches.

The contract: whatever adm_conv accepts, it computes on every element within the replay's bounds; whatever
it cannot compute, it refuses before the first launch and writes nothing.  tests/test_hip_conv_envelope.py walks this table on
the library symbol, tests/test_conv_envelope_host.py on the host emulation; guarded.try_conv holds one case.

Maps      all (h, w) with h, w in MAP_SIZES: 121 maps of at most 4096 pixels -- one pixel, one row, one column, odd sizes, sizes
          that are no multiple of a tile, maps narrower and wider than the 16-pixel tile row, maps of 64 / 128 / 256 pixels whose
          shape is not the 8x8 / 8x16 / 16x16 the models launch.
Batch     N = 5: the last tile of the kernels that put 2 or 4 whole images into a tile is ragged for both.
Channels  the smallest that reach each kernel: c0 = 32, cout = 40 unless the family needs more.
Families  FAMILIES: (label, conv_dict keywords, must-accept maps, even maps only).

Must-accept: a condition on the automatic choice (variant 0), so that no fix can shrink the envelope below what is in use.  The
maps are those the recorded models and guarded.CONV_CASES launch (squares of 8, 16, 32 and 64, 8x16, 16x32, 32x16) and 48x48 and
16x64 beside them; the split-K families on 8x8 and 16x16, where the models and CONV_CASES split K.
"""
import guarded as gd

MAP_SIZES = (1, 2, 3, 4, 8, 12, 16, 24, 32, 48, 64)
MAPS = [(h, w) for h in MAP_SIZES for w in MAP_SIZES]
N = 5
HOST_N = 2      # the host emulation's batch: what it checks -- the operand builders and the restatement at these shapes -- has no tiles

IN_USE = [(8, 8), (16, 16), (16, 32), (32, 16), (32, 32), (48, 48), (64, 64), (16, 64)]
IN_USE_16 = [m for m in IN_USE if m != (8, 8)]       # those of at least 16x16
IN_USE_1X1 = IN_USE + [(8, 16)]                      # the CLIP text transformer's token map
HEAD_MAPS = [(16, 16), (32, 32), (64, 64)]


def _resident_or_staged(h, w):
    """cout 264 at variant 0: the resident kernel takes the maps of whole 64-pixel tiles, the 192-wide staged tile the rest."""
    return 10 if (h * w) % 64 == 0 else 5


# (label, conv_dict keywords, must-accept maps, even maps only); `expect` may be a function of the map
FAMILIES = [
    ("1x1 staged", dict(taps=1, expect=6), IN_USE_1X1, False),
    ("1x1 variant 5", dict(taps=1, variant=5, expect=5), (), False),
    ("1x1 variant 6", dict(taps=1, variant=6, expect=6), (), False),
    ("1x1 variant 3", dict(taps=1, variant=3, cout=8, expect=3), (), False),
    ("3x3 staged", dict(expect=6), IN_USE, False),
    ("3x3 variant 5", dict(variant=5, expect=5), (), False),
    ("3x3 variant 6", dict(variant=6, expect=6), (), False),
    ("3x3 variant 3", dict(variant=3, cout=8, expect=3), (), False),
    ("1x1 fp32 NCHW head", dict(taps=1, cout=6, out_mode=1, out_scale=2.0 ** -10, expect=3), HEAD_MAPS, False),
    ("3x3 fp32 NCHW head", dict(cout=6, out_mode=1, out_scale=2.0 ** -10, expect=3), HEAD_MAPS, False),
    ("1x1 + residual + statistics", dict(taps=1, res=True, stats=True, expect=6), IN_USE, False),
    ("3x3 + residual + statistics", dict(res=True, stats=True, expect=6), IN_USE, False),
    # the 16-wide tile holds four 64-pixel images under one statistics group: not offered there
    ("1x1 variant 3 + statistics", dict(taps=1, variant=3, cout=8, stats=True, expect=3), (), False),
    ("3x3 GroupNorm + SiLU prologue", dict(prologue=2, expect=6), IN_USE, False),
    ("1x1 GroupNorm + SiLU prologue, concat input", dict(taps=1, prologue=2, c1=32, expect=6), IN_USE_1X1, False),
    ("split-K 1x1 ksplit 2", dict(taps=1, c0=128, ksplit=2, expect=6), [(8, 8), (16, 16)], False),
    ("split-K 3x3 ksplit 2 + residual + statistics", dict(c0=128, ksplit=2, res=True, stats=True, expect=6), [(8, 8), (16, 16)], False),
    ("skip-connection fold", dict(prologue=2, fc0=32, fc1=32, expect=6), IN_USE, False),
    ("GroupNorm-backward epilogue", dict(prologue=3, expect=6), IN_USE_16, False),
    ("in_up", dict(in_up=1, expect=6), IN_USE_16, True),
    ("in_up + res_up", dict(in_up=1, res=True, res_up=1, expect=6), IN_USE_16, True),
    ("up_phase 5 + statistics", dict(up_phase=5, stats=True, expect=6), IN_USE_16, False),
    ("resident 1x1 cout 264", dict(taps=1, c0=64, cout=264, expect=_resident_or_staged), IN_USE_1X1, False),
    ("resident 1x1 variant 10 cout 72", dict(taps=1, variant=10, cout=72, c0=64, expect=10), (), False),
    ("resident 1x1 variant 10 GEGLU cout 208", dict(taps=1, variant=10, cout=208, c0=64, geglu=1, expect=10), (), False),
    # the upsampled read exists in the 3x3 kernels only: a 1x1 request with it is refused whichever kernel its shape would pick
    ("1x1 cout 264 + in_up", dict(taps=1, c0=64, cout=264, in_up=1, expect=5), (), True),
    ("variant 7", dict(variant=7, expect=7), (), False),
    ("variant 8", dict(variant=8, expect=8), (), False),
]
FAMILY_LABELS = [f[0] for f in FAMILIES]


def family_maps(label):
    even = next(f for f in FAMILIES if f[0] == label)[3]
    return [(h, w) for h, w in MAPS if not even or (h % 2 == 0 and w % 2 == 0)]   # an odd map is no well-formed in_up request


def case(label, h, w, n=N):
    """-> (the conv_dict of family `label` at map h x w, whether it must be accepted)."""
    _, kw, must, _ = next(f for f in FAMILIES if f[0] == label)
    kw = dict(kw)
    if callable(kw.get("expect")):
        kw["expect"] = kw["expect"](h, w)
    d = gd.conv_dict(label, n, h, w, kw.pop("c0", 32), kw.pop("cout", 40), **kw)
    d["has_w_packed32"] = d["variant"] == 7
    return d, (h, w) in must


def matrix_line(label, kind, outcomes):
    """One line of the printed matrix: outcomes = [((h, w), "accepted" | "refused" | "FAILED", worst | None, fro / u | None)]."""
    maps = {o: [f"{h}x{w}" for (h, w), oo, _, _ in outcomes if oo == o] for o in ("accepted", "refused", "FAILED")}
    worst = max([x for _, o, x, _ in outcomes if o == "accepted"], default=0.0)
    fro = max([x for _, o, _, x in outcomes if o == "accepted"], default=0.0)
    failed = f" | FAILED {len(maps['FAILED'])}: {' '.join(maps['FAILED'])}" if maps["FAILED"] else ""
    return (f"ENVELOPE {label} | {kind} | accepted {len(maps['accepted'])}: {' '.join(maps['accepted']) or '-'} | "
            f"refused {len(maps['refused'])}: {' '.join(maps['refused']) or '-'} | worst err/bound {worst:.3f} | worst fro/u {fro:.3f}{failed}")


def walk(be, ops, label, T, device, n=N):
    """Every map of one family through guarded.try_conv -> (outcomes, the failed checks' messages).  A failed check does not end
    the walk -- the matrix stays whole --; anything else (a status that is neither 0 nor a refusal, a HIP error) does."""
    import launch_replay as lr
    outcomes, failures = [], []
    for i, (h, w) in enumerate(family_maps(label)):
        d, must = case(label, h, w, n)
        try:
            o, worst, fro = gd.try_conv(be, ops, d, T, device, 100 + i, must)
        except AssertionError as e:
            o, worst, fro = "FAILED", None, None
            failures.append(f"{label} {h}x{w}: {e}")
        outcomes.append(((h, w), o, worst, None if fro is None else fro / lr.U[T]))
    return outcomes, failures
