"""The 3D radius-2 star (star13) on the MI355X: star13_tbk's single step and the naive kernel against the
CPU oracle, its fused K = 2 sweep against naive single steps, and the slab engine with 4 ghost planes."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mpi_cuda_process_amd as mm  # noqa: E402
from mpi_cuda_process_amd import models  # noqa: E402
from mpi_cuda_process_amd.ops import (FieldLayout, alloc_field, apply_stencil, init_field,  # noqa: E402
                                      reference, set_kernel_variant)

# distinct weights, none a power of two, one negative
W = dict(c0=0.31, c1=0.13, c2=-0.011)
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
    return src[lay.owned, :, :lay.nx].cpu(), dst[lay.owned, :, :lay.nx].cpu()


# star13_tbk at K = 1: segments of 62 lanes x 16 B (248 fp32 / 124 fp64 columns), strips of 4 rows.
# One free row and plane in one partial segment; three fp64 segments with a ragged end and a ragged last
# strip (23 = 5 x 4 + 3); five segments, three strips; a pure copy (ny < 5)
SINGLE = [dict(nx=70, ny=5, nz=5), dict(nx=300, ny=23, nz=9, dtype="f64"), dict(nx=1000, ny=9, nz=6),
          dict(nx=70, ny=4, nz=7)]


@pytest.mark.parametrize("shape", SINGLE, ids=lambda s: "x".join(str(v) for v in s.values()))
@pytest.mark.parametrize("variant", ["tuned", "naive"])
def test_single_step_bitwise_vs_cpu_oracle(hip, shape, variant):
    prob = models.star13(init=ROUGH, **shape, **W)
    _, got = _one_step(prob, "cuda", variant)
    _, want = _one_step(prob, "cpu")
    assert torch.equal(got, want), "max diff %g" % (got.double() - want.double()).abs().max().item()


@pytest.mark.parametrize("shape", SINGLE[:2], ids=lambda s: "x".join(str(v) for v in s.values()))
def test_naive_matches_torch_reference(hip, shape):
    """Default weights (sum |w| = 1.1) on the default [0, 1) init: at most 14 roundings of values <= 1.1."""
    prob = models.star13(init=models.InitCondition(), **shape)
    u, got = _one_step(prob, "cuda", "naive")
    ref = reference.step("star13", u.double(), **prob.coef_kwargs())
    err = (got.double() - ref).abs().max().item()
    assert err < (2e-6 if prob.dtype == "f32" else 1e-13), err


# K = 2: fp32 segments of 60 lanes x 8 B (120 columns), fp64 of 60 x 16 B (120), strips of 4 (fp64 3) rows
# on a base 8 rows wider. Many segments and strips with a ragged one; fp64; narrower than a wave and fewer rows than a
# trapezoid's base; a grid shorter than the K = 2 pipeline (5 planes against 8 of priming); five z chunks
# (small grids march zc = 8 planes)
DEEP = [models.star13(nx=1000, ny=21, nz=12, init=ROUGH, **W), models.star13(nx=300, ny=40, nz=11, dtype="f64", init=ROUGH, **W),
        models.star13(nx=70, ny=7, nz=19, init=ROUGH, **W), models.star13(nx=130, ny=30, nz=5, dtype="f64", init=ROUGH, **W),
        models.star13(nx=70, ny=9, nz=40, init=ROUGH, **W)]


@pytest.mark.parametrize("prob", DEEP, ids=_ids)
@pytest.mark.parametrize("k", [2])
def test_fused_steps_bitwise(hip, prob, k):
    """K fused steps per sweep (star13_tbk) == K naive single steps, bitwise, with the last step's residual."""
    lay = FieldLayout.make(prob, halo=2 * k)
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


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_engine_deep_temporal(hip, dtype):
    """Region launches on slabs with 4 ghost planes and the sweep plan's shallower tails."""
    prob = models.star13(nx=200, ny=37, nz=64, dtype=dtype, init=ROUGH, **W)
    ref, rr = _sim(prob, 37, ranks=1, temporal=1, residual_every=9)
    got, rg = _sim(prob, 37, ranks=4, temporal=2, residual_every=9)
    assert np.array_equal(ref, got) and rr > 0 and abs(rr - rg) <= 1e-9 * max(1.0, rr)
