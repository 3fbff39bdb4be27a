"""Resource audit of the optimizer-family kernels (csrc/dib_optimizers.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch, no AGPRs, no LDS and
occupancy 8 for every instantiation - the kernels are HBM streams (parameter, gradient and 1 to 3 state slots per element), what
they need is waves in flight, not registers:
  dib_opt_kernel<DibOptSgdMomentum>              26 VGPRs      dib_opt_kernel<DibOptAdagrad>   41 VGPRs
  dib_opt_kernel<DibOptRmsprop<c, m>>  43 / 49 / 43 / 49       dib_opt_kernel<DibOptAdadelta>  61 VGPRs (two sqrt and a divide live)
  dib_opt_kernel<DibOptAdamax>                   44 VGPRs      dib_opt_kernel<DibOptNadam>     50 VGPRs
  dib_opt_kernel<DibOptAmsgrad>                  49 VGPRs      dib_opt_init_kernel 16, dib_opt_advance_kernel 19
The guards allow compiler drift below the 64-VGPR step but not the loss of it (occupancy 8 needs <= 64)."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)

RULES = ["DibOptSgdMomentum", "DibOptRmspropILb0ELb0EE", "DibOptRmspropILb0ELb1EE", "DibOptRmspropILb1ELb0EE",
         "DibOptRmspropILb1ELb1EE", "DibOptAdagrad", "DibOptAdadelta", "DibOptAdamax", "DibOptNadam", "DibOptAmsgrad"]


@pytest.mark.parametrize("name", ["dib_opt_kernelI%d%s" % (len(r.split("I")[0]), r) for r in RULES] +
                         ["dib_opt_init_kernel", "dib_opt_advance_kernel"])
def test_optimizer_kernels_use_no_scratch_and_keep_occupancy_8(kernels, name):
    kernels = family(kernels, "dib_opt_")
    assert len(kernels) == 12, sorted(kernels)   # one instantiation per rule (four of RMSprop), the state fill, the advance
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= 64 and k["Occupancy"] == 8, k
