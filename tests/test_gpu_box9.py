"""The 2D 9-point stencil (box9) on the MI355X: box9_wave and the naive kernel against the CPU oracle,
the fused box9_tbk sweeps against naive single steps, and the slab engine with deep temporal blocking."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mpi_cuda_process_amd as mm  # noqa: E402
from mpi_cuda_process_amd import models  # noqa: E402
from mpi_cuda_process_amd.ops import (FieldLayout, alloc_field, apply_stencil, init_field,  # noqa: E402
                                      reference, set_kernel_variant)

# weights that are no powers of two, c0 negative (power-of-two weights hide operation-order mistakes)
W = dict(c0=-0.2, c1=0.25, c2=0.05)
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


# one partial wave segment; several segments with a ragged end; fp64
SINGLE = [dict(h=37, w=70), dict(h=23, w=1500), dict(h=37, w=300, dtype="f64")]


@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: "x".join(str(v) for v in s.values()))
@pytest.mark.parametrize("variant", ["tuned", "naive"])
def test_single_step_bitwise_vs_cpu_oracle(hip, shape, variant):
    prob = models.box9(init=ROUGH, **shape, **W)
    _, got = _one_step(prob, "cuda", variant)
    _, want = _one_step(prob, "cpu")
    assert torch.equal(got, want), "max diff %g" % (got.double() - want.double()).abs().max().item()


@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: "x".join(str(v) for v in s.values()))
def test_naive_matches_torch_reference(hip, shape):
    """Default weights on the default [0, 1) random init, where the project's tolerances belong."""
    prob = models.box9(init=models.InitCondition(), **shape)
    u, got = _one_step(prob, "cuda", "naive")
    ref = reference.step("box9", u.double(), **prob.coef_kwargs())
    err = (got.double() - ref).abs().max().item()
    assert err < (2e-6 if prob.dtype == "f32" else 1e-13), err


# K = 8: five 240-column segments; three 112-column segments; one segment narrower than a wave; a
# grid shorter than the K = 8 pipeline
DEEP = [models.box9(h=45, w=1000, init=ROUGH, **W), models.box9(h=33, w=300, dtype="f64", init=ROUGH, **W),
        models.box9(h=19, w=70, init=ROUGH, **W), models.box9(h=5, w=130, dtype="f64", init=ROUGH, **W)]


@pytest.mark.parametrize("prob", DEEP, ids=_ids)
@pytest.mark.parametrize("k", [2, 3, 4, 6, 8])
def test_fused_steps_bitwise(hip, prob, k):
    """K fused steps per sweep (box9_tbk) == K naive single steps, bitwise, with the last step's residual."""
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
    assert torch.equal(fused[o, :, :lay.nx], cur[o, :, :lay.nx])
    assert res.item() > 0 and abs(res.item() - ref_res.item()) <= 1e-9 * max(1.0, ref_res.item())


def _sim(prob, steps, **kw):
    with mm.Simulation(prob, device="hip", **kw) as sim:
        sim.init()
        sim.run(steps)
        sim.synchronize()
        return sim.gather(), sim.residual


@pytest.mark.parametrize("dtype,k", [("f32", 8), ("f64", 4)])
def test_engine_deep_temporal(hip, dtype, k):
    """Region launches on slabs with ghost rows and the sweep plan's shallower tails."""
    prob = models.box9(h=200, w=700, dtype=dtype, init=ROUGH, **W)
    ref, rr = _sim(prob, 37, ranks=1, temporal=1, residual_every=9)
    got, rg = _sim(prob, 37, ranks=4, temporal=k, residual_every=9)
    assert np.array_equal(ref, got) and rr > 0 and abs(rr - rg) <= 1e-9 * max(1.0, rr)
