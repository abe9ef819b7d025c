"""The 2D 9-point stencil with nine weights (conv9) on the CPU oracle: one step against the plain-PyTorch
reference, the --weights flag, and slabs against a single slab."""

import numpy as np
import pytest

import mpi_cuda_process_amd as mm
from mpi_cuda_process_amd import models
from mpi_cuda_process_amd.__main__ import _parser, _problem
from mpi_cuda_process_amd.ops import FieldLayout, alloc_field, apply_stencil, init_field, reference

# nine distinct weights, none a power of two, two negative, sum |w| = 0.94: a swapped, transposed or
# mirrored weight changes bits, and values cannot grow
W9 = (0.07, 0.13, -0.02, 0.17, 0.26, 0.09, 0.05, -0.04, 0.11)
ROUGH = models.InitCondition(kind="random", seed=5, lo=-50.0, hi=150.0)


@pytest.mark.parametrize("h,w,dtype", [(37, 70, "f32"), (33, 131, "f64")])
def test_cpu_oracle_matches_torch_reference(h, w, dtype):
    """Default weights (sum |w| = 1) on the default [0, 1) init: eleven roundings of values at most 1, so
    the reference alone stays inside the project's tolerances."""
    prob = models.conv9(h=h, w=w, dtype=dtype, init=models.InitCondition())
    lay = FieldLayout.make(prob)
    src, dst = alloc_field(lay, "cpu"), alloc_field(lay, "cpu")
    init_field(prob, lay, src)
    apply_stencil(prob, lay, src, dst)
    u, got = src[lay.owned, 0, :lay.nx], dst[lay.owned, 0, :lay.nx]
    ref = reference.conv9(u.double(), prob.w9)
    err = (got.double() - ref).abs().max().item()
    assert err < (2e-6 if dtype == "f32" else 1e-13), err
    assert (got != u).any()


def _cli(text):
    return _problem(_parser().parse_args(["--stencil", "conv9", "--h", "8", "--w", "8", "--weights", text]))


@pytest.mark.parametrize("text", ["1,2,3,4,5,6,7", "1,2,3,4,5,6,7,8", "1,2,3,4,5,6,7,8,9,10", "1,2,3,4,nan,6,7,8,9",
                                  "1,2,3,4,five,6,7,8,9"])
def test_cli_rejects_bad_weights(text):
    with pytest.raises(SystemExit) as e:
        _cli(text)
    assert text in str(e.value) and "nine" in str(e.value)


def test_cli_weights_round_trip():
    assert _cli(",".join(repr(v) for v in W9)).w9 == W9


def test_engine_three_slabs_equal_one():
    """A residual interval (4) that does not divide the step count (11)."""
    prob = models.conv9(h=40, w=90, init=ROUGH, w9=W9)
    out = []
    for ranks in (1, 3):
        with mm.Simulation(prob, device="cpu", ranks=ranks, residual_every=4) as sim:
            sim.init()
            sim.run(11)
            sim.synchronize()
            out.append((sim.gather(), sim.residual))
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] > 0 and abs(out[0][1] - out[1][1]) <= 1e-9 * out[0][1]
