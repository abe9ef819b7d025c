"""The 2D 9-point stencil with nine weights (conv9) on the MI355X: conv9_tbk's single step and the naive
kernel against the CPU oracle, its fused sweeps against naive single steps, and the slab engine."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mpi_cuda_process_amd as mm  # noqa: E402
from mpi_cuda_process_amd import models  # noqa: E402
from mpi_cuda_process_amd.ops import (FieldLayout, alloc_field, apply_stencil, init_field,  # noqa: E402
                                      reference, set_kernel_variant)

# nine distinct weights, none a power of two, two negative, sum |w| = 0.94: a swapped, transposed or
# mirrored weight changes bits, and values cannot grow
W9 = (0.07, 0.13, -0.02, 0.17, 0.26, 0.09, 0.05, -0.04, 0.11)
ROUGH = models.InitCondition(kind="random", seed=5, lo=-50.0, hi=150.0)


def _ids(p):
    return p.describe().replace(" ", "_")


def _one_step(prob, device, variant="auto"):
    lay = FieldLayout.make(prob)
    src = alloc_field(lay, device)
    dst = alloc_field(lay, device)
    init_field(prob, lay, src)
    set_kernel_variant(variant)
    try:
        apply_stencil(prob, lay, src, dst)
    finally:
        set_kernel_variant("auto")
    return src[lay.owned, 0, :lay.nx].cpu(), dst[lay.owned, 0, :lay.nx].cpu()


# one partial x segment, width no multiple of the lane vector, fewer rows than a chunk (small grids march
# 8 rows per chunk), fp32 and fp64; several segments with a ragged last one and five chunks with a ragged
# last one (their middle segments and chunks take the loop copy without the hold selects)
SINGLE = [dict(h=5, w=70), dict(h=7, w=131, dtype="f64"), dict(h=37, w=300, dtype="f64"), dict(h=37, w=1000)]


@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: "x".join(str(v) for v in s.values()))
@pytest.mark.parametrize("variant", ["tuned", "naive"])
def test_single_step_bitwise_vs_cpu_oracle(hip, shape, variant):
    prob = models.conv9(init=ROUGH, w9=W9, **shape)
    _, got = _one_step(prob, "cuda", variant)
    _, want = _one_step(prob, "cpu")
    assert torch.equal(got, want), "max diff %g" % (got.double() - want.double()).abs().max().item()


@pytest.mark.parametrize("shape", SINGLE[:2], ids=lambda s: "x".join(str(v) for v in s.values()))
def test_naive_matches_torch_reference(hip, shape):
    """Default weights (sum |w| = 1) on the default [0, 1) random init, where the project's tolerances belong."""
    prob = models.conv9(init=models.InitCondition(), **shape)
    u, got = _one_step(prob, "cuda", "naive")
    ref = reference.step("conv9", u.double(), **prob.coef_kwargs())
    err = (got.double() - ref).abs().max().item()
    assert err < (2e-6 if prob.dtype == "f32" else 1e-13), err


# K = 8: five 240-column segments with a ragged end, six 8-row chunks with a ragged end; fp64, three
# 112-column segments; narrower than one wave's owned span; fewer rows than K
DEEP = [models.conv9(h=45, w=1000, init=ROUGH, w9=W9), models.conv9(h=45, w=300, dtype="f64", init=ROUGH, w9=W9),
        models.conv9(h=19, w=70, init=ROUGH, w9=W9), models.conv9(h=5, w=130, dtype="f64", init=ROUGH, w9=W9)]


@pytest.mark.parametrize("prob", DEEP, ids=_ids)
@pytest.mark.parametrize("k", [2, 3, 4, 6, 8])
def test_fused_steps_bitwise(hip, prob, k):
    """K fused steps per sweep (conv9_tbk) == K naive single steps, bitwise, with the last step's residual."""
    lay = FieldLayout.make(prob, halo=k)
    src = alloc_field(lay, "cuda")
    init_field(prob, lay, src)
    fused = alloc_field(lay, "cuda")
    res = torch.zeros((), dtype=torch.float64, device="cuda")
    apply_stencil(prob, lay, src, fused, steps=k, resid=res)
    set_kernel_variant("naive")
    try:
        cur = alloc_field(lay, "cuda")
        cur.copy_(src)
        ref_res = torch.zeros((), dtype=torch.float64, device="cuda")
        for i in range(k):
            nxt = alloc_field(lay, "cuda")
            nxt.copy_(cur)
            apply_stencil(prob, lay, cur, nxt, resid=ref_res if i == k - 1 else None)
            cur = nxt
    finally:
        set_kernel_variant("auto")
    torch.cuda.synchronize()
    o = lay.owned
    assert torch.equal(fused[o, 0, :lay.nx], cur[o, 0, :lay.nx])
    assert res.item() > 0 and abs(res.item() - ref_res.item()) <= 1e-9 * max(1.0, ref_res.item())


def _sim(prob, steps, **kw):
    with mm.Simulation(prob, device="hip", **kw) as sim:
        sim.init()
        sim.run(steps)
        sim.synchronize()
        return sim.gather(), sim.residual


@pytest.mark.parametrize("dtype,k", [("f32", 8), ("f64", 6)])
def test_engine_deep_temporal(hip, dtype, k):
    """Region launches on slabs with ghost rows and the sweep plan's shallower tails."""
    prob = models.conv9(h=200, w=700, dtype=dtype, init=ROUGH, w9=W9)
    ref, rr = _sim(prob, 37, ranks=1, temporal=1, residual_every=9)
    got, rg = _sim(prob, 37, ranks=4, temporal=k, residual_every=9)
    assert np.array_equal(ref, got) and rr > 0 and abs(rr - rg) <= 1e-9 * max(1.0, rr)
