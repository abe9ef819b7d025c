"""The 3D radius-2 star (star13) on the CPU oracle: one step against the plain-PyTorch reference, the
two-cell held frame, and the radius carried through the slab engine (ghost planes = 2 x temporal)."""

import numpy as np
import pytest
import torch

import mpi_cuda_process_amd as mm
from mpi_cuda_process_amd import models
from mpi_cuda_process_amd.ops import FieldLayout, alloc_field, apply_stencil, init_field, reference

# distinct weights, none a power of two, one negative
W = dict(c0=0.31, c1=0.13, c2=-0.011)
ROUGH = models.InitCondition(kind="random", seed=5, lo=-50.0, hi=150.0)


def _one_step(prob):
    lay = FieldLayout.make(prob)
    src, dst = alloc_field(lay, "cpu"), alloc_field(lay, "cpu")
    init_field(prob, lay, src)
    apply_stencil(prob, lay, src, dst)
    return src[lay.owned, :, :lay.nx].clone(), dst[lay.owned, :, :lay.nx].clone()


def _run(prob, steps, **kw):
    with mm.Simulation(prob, device="cpu", **kw) as sim:
        sim.init()
        sim.run(steps)
        sim.synchronize()
        return sim.gather().reshape(prob.nz, prob.ny, prob.nx), sim.residual


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", [(9, 7, 6), (70, 13, 8)], ids=lambda s: "x".join(map(str, s)))
def test_cpu_oracle_matches_torch_reference(dtype, shape):
    """Default weights (sum |w| = 1.1) on the default [0, 1) init: at most 14 roundings of values <= 1.1."""
    prob = models.star13(nx=shape[0], ny=shape[1], nz=shape[2], dtype=dtype)
    assert prob.radius == 2 and (prob.c0, prob.c1, prob.c2) == (0.25, 4.0 * 0.1 / 3.0, -0.1 / 12.0)
    u, got = _one_step(prob)
    ref = reference.step("star13", u.double(), **prob.coef_kwargs())
    err = (got.double() - ref).abs().max().item()
    assert err < (2e-6 if dtype == "f32" else 1e-13), err
    assert (got != u).any()


def test_held_frame_is_two_cells_thick():
    u, got = _one_step(models.star13(nx=11, ny=10, nz=9, init=ROUGH, **W))
    frame = torch.ones_like(u, dtype=torch.bool)
    frame[2:-2, 2:-2, 2:-2] = False
    assert torch.equal(got[frame], u[frame])
    # the first free layer moves on every axis
    assert (got[2, 2:-2, 2:-2] != u[2, 2:-2, 2:-2]).any() and (got[2:-2, 2, 2:-2] != u[2:-2, 2, 2:-2]).any()
    assert (got[2:-2, 2:-2, 2] != u[2:-2, 2:-2, 2]).any()
    u, got = _one_step(models.star13(nx=4, ny=9, nz=9, init=ROUGH, **W))
    assert torch.equal(got, u)


def test_engine_four_slabs_temporal_two_equal_one():
    prob = models.star13(nx=40, ny=11, nz=33, init=ROUGH, **W)
    ref, rr = _run(prob, 7, ranks=1, temporal=1, residual_every=3)
    got, rg = _run(prob, 7, ranks=4, temporal=2, residual_every=3)
    assert np.array_equal(ref, got) and rr > 0 and abs(rr - rg) <= 1e-9 * max(1.0, rr)


def test_engine_slabs_cut_inside_the_z_frame():
    """nz = 9 over 4 ranks: slabs of 3, 2, 2, 2 planes, the outer ones thinner than or equal to the frame."""
    prob = models.star13(nx=13, ny=8, nz=9, init=ROUGH, **W)
    assert np.array_equal(_run(prob, 5, ranks=1, temporal=1)[0], _run(prob, 5, ranks=4, temporal=1)[0])


@pytest.mark.parametrize("kw,text", [(dict(py=2, ranks=4), "slabs only"),
                                     (dict(ranks=4, temporal=2), "fewer than the 4 ghost planes")])
def test_engine_rejects(kw, text):
    with pytest.raises(RuntimeError, match=text):
        mm.Simulation(models.star13(nx=16, ny=16, nz=12), device="cpu", **kw)
