"""adm_conv over the envelope table of tests/conv_envelope.py: 28 kernel families x 121 map shapes (1x1 ... 64x64, most of which
no model launches) x both torsos, every request through the library symbol on guarded operands (tests/guarded.py).

Exactly two outcomes pass (guarded.try_conv):
  accepted  status 0: all margins intact, every element of the output (and of out_stats and the split-K workspace) finite -- on
            the whole tensor --, worst err / bound <= 1 and the Frobenius error within launch_replay.fro_bound against the float64
            restatement: the bounds of tests/test_hip_launch_replay.py, unchanged
  refused   ADM_E_ARG / ADM_E_SHAPE / ADM_E_ALIGN: the output, out_stats and the workspace are NaN in every element still and all
            margins are intact -- nothing was launched
Any other status or exception fails the case.  Per case besides: adm_conv_stat_slabs answers > 0 exactly where the request with
out_stats is accepted, adm_conv_pick_variant answers the variant the table names, and no must-accept case (the maps in use, on
the automatic variant) is refused.  Each test prints its family's accepted / refused matrix (profiles/conv_envelope/ holds a run).

tests/test_conv_envelope_host.py runs the same table on the host emulation and plants the defects these checks must catch.
"""
import pytest
import torch

import conv_envelope as ce
import guarded as gd

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


@pytest.mark.parametrize("T", TYPES, ids=_ids.get)
@pytest.mark.parametrize("label", ce.FAMILY_LABELS)
def test_conv_envelope(ops, label, T):
    outcomes, failures = ce.walk(gd.Hip(ops), ops, label, T, DEV)
    print(ce.matrix_line(label, _ids[T], outcomes))
    assert not failures, "\n".join(failures)
    assert len(outcomes) == len(ce.family_maps(label))
