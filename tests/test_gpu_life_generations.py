"""Generations rules (B/S/C) on the MI355X: life_gen_bits (every C-plane count and depth) and the naive
kernel against the integer torch reference, exactly, with the change count of the last generation; and
through the engine across slabs."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mpi_cuda_process_amd as m  # noqa: E402
from footprint_helper import run_case  # noqa: E402
from mpi_cuda_process_amd.ops import (FieldLayout, alloc_field, apply_stencil, dense_to_field,  # noqa: E402
                                      field_to_dense, reference, set_kernel_variant)

# C = 3, 4 | 5, 8 | 9 | 17, 32: both ends of 2, 3 and 5 state planes and the first of 4; the first two
# tables are bitwise complements (every one of the 18 entries once 0 and once 1, B0 included)
RULES = ["B0257/S1468/C3", "B13468/S02357/C4", "B2/S345/C5", "B36/S23/C8", "B2/S345/C9", "B3/S23/C17",
         "B34678/S234/C32"]
FUSED_RULES = [RULES[0], RULES[3], RULES[4], RULES[6]]  # 2, 3, 4 and 5 planes
DEPTHS = [2, 3, 4, 6, 8]


@functools.lru_cache(maxsize=None)
def _generations(h, w, rule):
    """Generations 0..8 by reference.life of a seeded board: state 1 with probability 0.5, the other
    states uniform, frame included, so that every state, the wrap, N = 0 and N = 8 all occur."""
    c = m.native().life_rule_states(rule)
    gen = torch.Generator().manual_seed(11)
    other = torch.randint(0, c - 1, (h, 1, w), generator=gen)
    other = torch.where(other >= 1, other + 1, other)  # 0, 2 .. C-1
    board = torch.where(torch.rand((h, 1, w), generator=gen) < 0.5, torch.ones_like(other), other).to(torch.uint8)
    assert set(board.unique().tolist()) == set(range(c))
    gens = [board.cuda()]
    for _ in range(max(DEPTHS)):
        gens.append(reference.life(gens[-1], rule))
    return gens


def _start(h, w, rule, halo):
    prob = m.life2d(h=h, w=w, rule=rule)
    lay = FieldLayout.make(prob, halo=halo)
    src = dense_to_field(prob, _generations(h, w, rule)[0], lay, alloc_field(lay, "cuda"))
    return prob, lay, src, alloc_field(lay, "cuda")


@pytest.mark.parametrize("variant,rule", [(v, r) for r in RULES for v in ("tuned", "naive")] + [("auto", "B3/S23/C33")])
@pytest.mark.parametrize("shape", [(37, 70), (23, 1986)], ids=lambda s: "%dx%d" % s)
def test_single_step(hip, variant, shape, rule):
    """37x70: one partial segment; 23x1986: the second segment owns one computed cell and the held last
    column. 33 states are past life_gen_bits and take the naive kernel under auto."""
    prob, lay, src, dst = _start(*shape, rule, 1)
    set_kernel_variant(variant)
    try:
        apply_stencil(prob, lay, src, dst)
    finally:
        set_kernel_variant("auto")
    assert torch.equal(field_to_dense(lay, dst), _generations(*shape, rule)[1])


@pytest.mark.parametrize("rule", FUSED_RULES)
@pytest.mark.parametrize("shape", [(45, 2100), (5, 130)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("k", DEPTHS)
def test_fused_generations(hip, k, shape, rule):
    """45x2100: two ragged segments; 5x130: a grid shorter than the pipeline."""
    prob, lay, src, dst = _start(*shape, rule, k)
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
    prob = m.life2d(h=200, w=2100, rule="B2/S345/C4", density=0.5)
    u0, one, r1 = _sim(prob, 37, ranks=1, temporal=1)
    _, got, r4 = _sim(prob, 37, ranks=4, temporal=max(DEPTHS))
    want = reference.run("life", torch.from_numpy(u0).cuda(), 37, rule=prob.rule).cpu().numpy()
    assert np.array_equal(got, one) and np.array_equal(got, want) and r1 == r4 and r1 > 0


def test_deepest_instance_footprint(hip):
    """life_gen_bits<8, 5>: no stray write, no dependence on anything outside its window."""
    set_kernel_variant("tuned")
    try:
        run_case("cuda", kind="life", dtype="u8", k=8, nx=2100, ny=1, nz=23, geometry="slab", rule=RULES[-1])
    finally:
        set_kernel_variant("auto")
