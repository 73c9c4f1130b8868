"""The envelope table of tests/conv_envelope.py on the host: emulation and planted defects.

Emulation: every case of the table -- 28 families x up to 121 maps, 1-pixel maps, single rows and columns among them -- runs
with the float64 restatement written through the carves (tests/test_guarded_host.py's Emulated, at a batch of 2) and passes
guarded.try_conv's conditions for an accepted launch: the operand builders and the restatement cope with every shape of the grid.
Defects: a launch that leaves the columns >= 16 of a wider map unwritten, a refusal after part of the output was written, a
refused must-accept case, and statistics slabs offered for a request that is then refused each fail the check meant for them.
"""
import pytest
import torch

import conv_envelope as ce
import guarded as gd
from test_guarded_host import Emulated

CPU = "cpu"
TYPES = [torch.bfloat16, torch.float16]
_ids = {torch.bfloat16: "bf16", torch.float16: "f16"}


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("label", ce.FAMILY_LABELS)
def test_every_case_holds_for_the_restatement(label, T):
    outcomes, failures = ce.walk(Emulated(), None, label, T, CPU, n=ce.HOST_N)
    assert not failures, "\n".join(failures)
    assert len(outcomes) == len(ce.family_maps(label)) and all(o == "accepted" for _, o, _, _ in outcomes)


def test_the_table_is_the_grid_and_holds_the_must_accept_set():
    assert len(ce.MAPS) == 121 and max(h * w for h, w in ce.MAPS) == 4096 and len(set(ce.FAMILY_LABELS)) == len(ce.FAMILIES)
    musts = 0
    for label, kw, must, even in ce.FAMILIES:
        maps = ce.family_maps(label)
        assert len(maps) == (81 if even else 121), label
        assert set(must) <= set(maps), label                      # the must-accept set is a subset of the table
        assert not must or kw.get("variant", 0) == 0, label       # and a condition on the automatic choice only
        for h, w in maps:
            d, m = ce.case(label, h, w)
            assert d["n"] == ce.N == 5 and m == ((h, w) in must)
            musts += m
    assert musts == sum(len(f[2]) for f in ce.FAMILIES) > 0
    for label in ("3x3 staged", "3x3 + residual + statistics", "3x3 GroupNorm + SiLU prologue", "skip-connection fold"):
        assert set(next(f for f in ce.FAMILIES if f[0] == label)[2]) == set(ce.IN_USE), label
    for label in ("1x1 staged", "resident 1x1 cout 264"):
        assert set(next(f for f in ce.FAMILIES if f[0] == label)[2]) == set(ce.IN_USE) | {(8, 16)}, label


# (the defect, the family and map it is planted in, whether the case is a must-accept one, the failing check's message)
PLANTED = [
    ("columns >= 16 unwritten", "1x1 staged", (8, 32), False, "not finite"),
    ("columns >= 16 unwritten", "1x1 fp32 NCHW head", (4, 64), False, "not finite"),
    ("columns >= 16 unwritten", "split-K 1x1 ksplit 2", (2, 32), False, "not finite"),
    ("refused after a partial write", "3x3 staged", (24, 24), False, "the refused launch wrote 8 of"),
    ("refused after a partial write", "1x1 + residual + statistics", (4, 48), False, "the refused launch wrote 8 of"),
    ("refused", "3x3 staged", (16, 64), True, "a must-accept case was refused"),
    ("refused", "resident 1x1 cout 264", (8, 16), True, "a must-accept case was refused"),
    ("slabs offered, then refused", "3x3 + residual + statistics", (24, 32), False, "adm_conv_stat_slabs answers 1 and adm_conv refuses"),
    ("slabs offered, then refused", "GroupNorm-backward epilogue", (8, 8), False, "adm_conv_stat_slabs answers 1 and adm_conv refuses"),
]


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("defect,label,hw,must,message", PLANTED, ids=[f"{p[0]}, {p[1]} {p[2][0]}x{p[2][1]}" for p in PLANTED])
def test_planted_defects_fail(defect, label, hw, must, message, T):
    d, m = ce.case(label, *hw, n=ce.HOST_N)
    assert m == must
    assert gd.try_conv(Emulated(), None, d, T, CPU, 7, m)[0] == "accepted"      # the same case passes without the defect
    with pytest.raises(AssertionError, match=message):
        gd.try_conv(Emulated(defect), None, d, T, CPU, 7, m)


def test_a_clean_refusal_passes_and_a_wrong_variant_fails():
    d, _ = ce.case("3x3 staged", 24, 24, n=ce.HOST_N)
    assert gd.try_conv(Emulated("refused"), None, d, torch.bfloat16, CPU, 7) == ("refused", None, None)
    with pytest.raises(AssertionError, match="adm_conv_pick_variant answers 6"):
        gd.try_conv(_Answers(6), None, dict(d, expect=5), torch.bfloat16, CPU, 7)


class _Answers(Emulated):
    """An emulation whose adm_conv_pick_variant answer is fixed."""

    def __init__(self, variant):
        super().__init__()
        self.variant = variant

    def conv_try(self, d, T, t, packed, w32p, out, g):
        accepted, stats, slabs, _ = super().conv_try(d, T, t, packed, w32p, out, g)
        return accepted, stats, slabs, self.variant
