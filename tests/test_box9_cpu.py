"""The 2D 9-point stencil (box9) on the CPU oracle: one step against the plain-PyTorch reference,
the held boundary, and the slab engine against a single slab."""

import numpy as np
import pytest
import torch

import mpi_cuda_process_amd as mm
from mpi_cuda_process_amd import models
from mpi_cuda_process_amd.ops import FieldLayout, alloc_field, apply_stencil, init_field, reference

# weights that are no powers of two, c0 negative (power-of-two weights hide operation-order mistakes)
W = dict(c0=-0.2, c1=0.25, c2=0.05)
ROUGH = models.InitCondition(kind="random", seed=5, lo=-50.0, hi=150.0)


def _one_step(prob):
    lay = FieldLayout.make(prob)
    src = alloc_field(lay, "cpu")
    dst = alloc_field(lay, "cpu")
    init_field(prob, lay, src)
    apply_stencil(prob, lay, src, dst)
    return src[lay.owned, 0, :lay.nx], dst[lay.owned, 0, :lay.nx]


@pytest.mark.parametrize("h,w,dtype", [(37, 70, "f32"), (33, 130, "f64")])
def test_cpu_oracle_matches_torch_reference(h, w, dtype):
    """Default weights on the default [0, 1) random init, where the project's tolerances belong."""
    prob = models.box9(h=h, w=w, dtype=dtype, init=models.InitCondition())
    u, got = _one_step(prob)
    ref = reference.step("box9", u.double(), **prob.coef_kwargs())
    err = (got.double() - ref).abs().max().item()
    assert err < (2e-6 if dtype == "f32" else 1e-13), err
    assert (got != u).any()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_boundary_cells_are_held_bitwise(dtype):
    u, got = _one_step(models.box9(h=37, w=70, dtype=dtype, init=ROUGH, **W))
    for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
        assert torch.equal(got[edge], u[edge])
    assert (got[1:-1, 1:-1] != u[1:-1, 1:-1]).any()


def test_engine_three_slabs_equal_one():
    prob = models.box9(h=40, w=90, init=ROUGH, **W)
    out = []
    for ranks in (1, 3):
        with mm.Simulation(prob, device="cpu", ranks=ranks) as sim:
            sim.init()
            sim.run(11)
            sim.synchronize()
            out.append(sim.gather())
    assert np.array_equal(out[0], out[1])
