"""Generations rules (B/S/C) on the CPU tier: the three-part rule text, the CPU backend against the
integer torch reference, and /C2 as the plain Life-like rule."""

import numpy as np
import pytest
import torch

import mpi_cuda_process_amd as m
from mpi_cuda_process_amd.ops import reference


@pytest.mark.parametrize("rule", ["B2/S/C3", "b2/s345/c4", "B34678/S234/C24"])
def test_rule_text_round_trip(rule):
    nat = m.native()
    birth, survive = nat.life_rule_parse(rule)
    side = rule.upper().split("/")
    assert birth == sum(1 << int(d) for d in side[0][1:]) and survive == sum(1 << int(d) for d in side[1][1:])
    assert nat.life_rule_states(rule) == int(side[2][1:])
    assert nat.life_rule_format(birth, survive, nat.life_rule_states(rule)) == rule.upper()


def test_two_states_format_as_a_plain_rule():
    nat = m.native()
    assert nat.life_rule_states("B36/S23/C2") == 2 and nat.life_rule_states("B36/S23") == 2
    assert nat.life_rule_format(*nat.life_rule_parse("B36/S23/C2"), 2) == "B36/S23"
    assert m.life2d(rule="B3/S23/C2").conway and not m.life2d(rule="B3/S23/C3").conway
    assert m.life2d(rule="B2/S345/C4").describe().endswith(" B2/S345/C4")


@pytest.mark.parametrize("bad", ["B2/S/C1", "B2/S/C257", "B2/S/C", "B2/S/C3x"])
def test_bad_rule_text_is_named(bad):
    with pytest.raises(RuntimeError, match="'%s'" % bad):
        m.native().life_rule_parse(bad)
    with pytest.raises(ValueError, match="'%s'" % bad):
        m.life2d(rule=bad)


def _run(prob, steps):
    with m.Simulation(prob, device="cpu") as sim:
        sim.init()
        u0 = sim.gather()
        sim.run(steps)
        return u0, sim.gather()


# the first two tables are bitwise complements: every one of the 18 entries is once 0 and once 1
@pytest.mark.parametrize("rule", ["B0257/S1468/C3", "B13468/S02357/C4", "B2/S345/C9", "B3/S23/C40"])
@pytest.mark.parametrize("steps", [1, 7])
def test_cpu_backend_matches_reference(rule, steps):
    prob = m.life2d(h=37, w=70, rule=rule, init=m.InitCondition(kind="life", density=0.5, seed=3))
    u0, got = _run(prob, steps)
    want = reference.run("life", torch.from_numpy(u0), steps, rule=rule)
    assert int(want.max()) >= 2 and np.array_equal(got, want.numpy())


def test_c2_is_the_plain_rule():
    init = m.InitCondition(kind="life", density=0.5, seed=4)
    _, a = _run(m.life2d(h=37, w=70, init=init, rule="B36/S23"), 9)
    _, b = _run(m.life2d(h=37, w=70, init=init, rule="B36/S23/C2"), 9)
    assert a.any() and np.array_equal(a, b)
