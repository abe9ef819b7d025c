"""Life-like rules on the MI355X: life_rule_bits (every depth) and the naive kernel against the
integer torch reference, exactly, with the change count of the last generation; and through the
engine across slabs."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mpi_cuda_process_amd as m  # noqa: E402
from mpi_cuda_process_amd.ops import (FieldLayout, alloc_field, apply_stencil, field_to_dense,  # noqa: E402
                                      init_field, reference, set_kernel_variant)

# the last two are bitwise complements: between them every one of the 18 table entries is once 0 and
# once 1, birth from 0 neighbours and both outcomes at 8 included
RULES = ["B36/S23", "B3678/S34678", "B0257/S1468", "B13468/S02357"]


def _problem(h, w, rule):
    # density 0.5, so that 0 and 8 live neighbours occur on boards this small
    return m.life2d(h=h, w=w, rule=rule, init=m.InitCondition(kind="life", density=0.5, seed=7))


def _start(prob, halo):
    lay = FieldLayout.make(prob, halo=halo)
    src = alloc_field(lay, "cuda")
    init_field(prob, lay, src)
    return lay, src


@functools.lru_cache(maxsize=None)
def _generations(h, w, rule):
    """Generations 0..16 of the board by reference.life, computed once per (shape, rule)."""
    prob = _problem(h, w, rule)
    lay, src = _start(prob, 1)
    gens = [field_to_dense(lay, src)]
    for _ in range(16):
        gens.append(reference.life(gens[-1], rule))
    return gens


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("shape", [(37, 70), (23, 1986)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("variant", ["tuned", "naive"])
def test_single_step(hip, variant, shape, rule):
    """37x70: one partial segment; 23x1986: the second segment owns one computed cell and the held
    last column."""
    prob = _problem(*shape, rule)
    lay, src = _start(prob, 1)
    dst = alloc_field(lay, "cuda")
    set_kernel_variant(variant)
    try:
        apply_stencil(prob, lay, src, dst)
    finally:
        set_kernel_variant("auto")
    gens = _generations(*shape, rule)
    assert 0 < int(gens[1].sum()) < gens[1].numel()
    assert torch.equal(field_to_dense(lay, dst), gens[1])


FUSED = [((45, 2100), r) for r in RULES] + [(s, r) for s in [(19, 70), (5, 130)] for r in RULES[2:]]


@pytest.mark.parametrize("shape,rule", FUSED, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
@pytest.mark.parametrize("k", [2, 3, 4, 6, 8, 12, 16])
def test_fused_generations(hip, k, shape, rule):
    """45x2100: two ragged segments; 5x130: a grid shorter than the K = 16 pipeline."""
    prob = _problem(*shape, rule)
    lay, src = _start(prob, k)
    dst = alloc_field(lay, "cuda")
    res = torch.zeros((), dtype=torch.float64, device="cuda")
    apply_stencil(prob, lay, src, dst, steps=k, resid=res)
    gens = _generations(*shape, rule)
    assert torch.equal(field_to_dense(lay, dst), gens[k])
    assert res.item() == int((gens[k] != gens[k - 1]).sum())


def _sim(prob, steps, **kw):
    with m.Simulation(prob, device="hip", residual_every=9, **kw) as sim:
        sim.init()
        u0 = sim.gather()
        sim.run(steps)
        sim.synchronize()
        return u0, sim.gather(), sim.residual


def test_engine_slabs_and_depth(hip):
    prob = m.life2d(h=200, w=2100, rule="B36/S23", density=0.5)
    u0, one, r1 = _sim(prob, 37, ranks=1, temporal=1)
    _, got, r4 = _sim(prob, 37, ranks=4, temporal=12)
    want = reference.run("life", torch.from_numpy(u0).cuda(), 37, rule="B36/S23").cpu().numpy()
    assert np.array_equal(got, one) and np.array_equal(got, want) and r1 == r4 and r1 > 0
