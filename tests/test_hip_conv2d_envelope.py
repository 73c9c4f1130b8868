"""adm_conv2d, adm_pool2d, adm_global_avgpool_f32 and adm_resize_bilinear over the tables of tests/conv2d_envelope.py, both
torsos, every request through the library symbol on guarded operands (tests/guarded.py's carves, NaN around every input).

Exactly what the table says passes:
  accepted  status 0: all margins and the parent's sentinel intact, every output element finite, worst err / bound <= 1 against
            the float64 restatements of tests/inception_replay.py (tests/clip_image_replay.py for the bicubic mode), whole tensor,
            bounds unchanged; conv cases of at least conv2d_envelope.FRO_MIN_ELEMS elements also within launch_replay.fro_bound
  refused   ADM_E_ARG / ADM_E_SHAPE / ADM_E_ALIGN: the output is NaN in every element still, margins and sentinel intact
An accepted-table row that is refused fails, a refusal row answered 0 fails, any other status fails.  Each test prints its
family's accepted / refused matrix and, for the conv families, a line per kernel pick (profiles/conv2d_envelope/ holds a run).

tests/test_conv2d_envelope_host.py runs the same tables on a host stand-in and plants the defects these checks must catch.
"""
import pytest
import torch

import conv2d_envelope as c2

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
@pytest.mark.parametrize("label", c2.FAMILY_LABELS)
def test_conv2d_envelope(ops, label, T):
    outcomes, failures = c2.walk(c2.Hip(ops), label, T, DEV)
    print(c2.matrix_line(label, _ids[T], outcomes))
    for line in c2.pick_lines(label, _ids[T], outcomes):
        print(line)
    assert not failures, "\n".join(failures)
    rows = c2.rows_of(label)
    assert len(outcomes) == len(rows) and [o[1] for o in outcomes] == [r["expect"] for r in rows]
