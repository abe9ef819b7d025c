"""The 3D 7-point star with seven weights (star7) on the CPU oracle: the direction convention, one and
five steps against the plain-PyTorch reference, the --weights flag, and slabs against a single slab."""

import numpy as np
import pytest

import mpi_cuda_process_amd as mm
from mpi_cuda_process_amd import models
from mpi_cuda_process_amd.__main__ import _parser, _problem
from mpi_cuda_process_amd.ops import FieldLayout, alloc_field, apply_stencil, reference

# seven distinct weights, none a power of two, one negative, sum |w| <= 1: a swapped direction changes bits
W = dict(c0=0.28, wxm=0.17, wxp=-0.03, wym=0.11, wyp=0.07, wzm=0.19, wzp=0.05)
ROUGH = models.InitCondition(kind="random", seed=5, lo=-50.0, hi=150.0)


def _run(prob, steps, **kw):
    with mm.Simulation(prob, device="cpu", **kw) as sim:
        sim.init()
        sim.run(steps)
        sim.synchronize()
        return sim.gather().reshape(prob.nz, prob.ny, prob.nx)


def test_unit_impulse_pins_the_direction_convention():
    """wxm multiplies u(x-1), so it lands at x+1 of the impulse (that cell's x-1 neighbour is the impulse)."""
    prob = models.star7(n=7, dtype="f64", **W)
    lay = FieldLayout.make(prob)
    src, dst = alloc_field(lay, "cpu"), alloc_field(lay, "cpu")
    src.zero_()
    src[lay.owned][3, 3, 3] = 1.0
    apply_stencil(prob, lay, src, dst)
    got = dst[lay.owned, :, :lay.nx].numpy()
    want = np.zeros((7, 7, 7))  # indexed (z, y, x)
    want[3, 3, 3] = W["c0"]
    want[3, 3, 4], want[3, 3, 2] = W["wxm"], W["wxp"]
    want[3, 4, 3], want[3, 2, 3] = W["wym"], W["wyp"]
    want[4, 3, 3], want[2, 3, 3] = W["wzm"], W["wzp"]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("steps", [1, 5])
def test_cpu_oracle_matches_torch_reference(dtype, steps):
    """Default weights (sum |w| = 1) on the default [0, 1) init: seven roundings of values at most 1."""
    import torch

    prob = models.star7(nx=37, ny=11, nz=9, dtype=dtype)
    u0 = torch.from_numpy(_run(prob, 0).astype(np.float64))
    got = torch.from_numpy(_run(prob, steps).astype(np.float64))
    ref = reference.run("star7", u0, steps, **prob.coef_kwargs())
    err = (got - ref).abs().max().item()
    assert err < (2e-6 if dtype == "f32" else 1e-13), err
    assert (got != u0).any()


@pytest.mark.parametrize("text", ["0.3,0.2,0.2,0.1,0.1,0.05", "0.3,0.2,0.2,0.1,0.1,0.05,0.05,0.0", "0.3,0.2,x,0.1,0.1,0.05,0.05"])
def test_cli_rejects_bad_weights(text):
    with pytest.raises(SystemExit) as e:
        _problem(_parser().parse_args(["--stencil", "star7", "--n", "8", "--weights", text]))
    assert text in str(e.value)


def test_engine_three_slabs_temporal_three_equal_one():
    prob = models.star7(nx=45, ny=13, nz=31, init=ROUGH, **W)
    assert np.array_equal(_run(prob, 11, ranks=1, temporal=1), _run(prob, 11, ranks=3, temporal=3))
