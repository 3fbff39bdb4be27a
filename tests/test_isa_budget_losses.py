"""Resource audit of the loss-family kernels (csrc/dib_losses.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950) for the 14 kinds x 4 LANES instantiations
of dib_loss_ex_kernel: no scratch, no AGPRs, 16 bytes of LDS (dib_block_sum_256's four floats).  The kernels are streams over
pred / y / g_pred: what they need is waves in flight.
  element-wise kinds (bce_logits, bce, mse, mae, mape, msle, huber, log_cosh, poisson, kl_divergence): 21 ... 51 VGPRs, occupancy 8
  cce (probabilities) 25 ... 55 VGPRs, occupancy 8;  sparse_cce 46 ... 66, occupancy 8 / 7 at 64 lanes
  cosine_similarity 48 ... 77 and cce_logits 58 ... 74 VGPRs (three sums and a butterfly live): occupancy 8 / 8 / 7 / 6 at 1 / 4 / 16 / 64 lanes
The guards allow compiler drift below a register step but not the loss of it."""
import re

import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)

ELEMENTWISE = (0, 1, 3, 4, 5, 6, 7, 8, 9, 10)   # include/dib_hip.h / dib_losses.h DIB_LOSS_* of the element-wise kinds
CLASS_AXIS = (11, 12, 13, 14)
LANES = (1, 4, 16, 64)
# kind -> most VGPRs at 1 / 4 / 16 / 64 lanes (the occupancy step the instantiation sits under today: 64 -> 8, 72 -> 7, 80 -> 6)
CLASS_AXIS_VGPRS = {11: (64, 64, 72, 80), 12: (64, 64, 72, 80), 13: (64, 64, 64, 64), 14: (64, 64, 64, 72)}
OCCUPANCY = {64: 8, 72: 7, 80: 6}


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ELEMENTWISE + CLASS_AXIS)
def test_loss_kernels_use_no_scratch_and_keep_their_occupancy(kernels, kind, lanes):
    fam = family(kernels, "dib_loss_ex_kernel")
    assert len(fam) == len(ELEMENTWISE + CLASS_AXIS) * len(LANES), sorted(fam)
    hits = [k for k in fam if re.search(r"dib_loss_ex_kernelILi%dELi%dEE" % (kind, lanes), k)]
    assert len(hits) == 1, (kind, lanes, sorted(fam))
    k = fam[hits[0]]
    assert k["ScratchSize"] == 0 and k["NumAgprs"] == 0 and k["LDSByteSize"] == 16, k
    cap = 64 if kind in ELEMENTWISE else CLASS_AXIS_VGPRS[kind][LANES.index(lanes)]
    assert k["NumVgprs"] <= cap and k["Occupancy"] >= OCCUPANCY[cap], (k, cap)
