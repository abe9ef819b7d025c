"""Life-like rules (any B/S outer-totalistic Moore rule) on the CPU tier: the rule parser, the CPU
backend against the integer torch reference, Conway unchanged, and the `life --rule` command line."""

import os
import subprocess

import numpy as np
import pytest
import torch

import mpi_cuda_process_amd as m
from mpi_cuda_process_amd.ops import reference
from mpi_cuda_process_amd.utils import format_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the last two are bitwise complements: between them every table entry is once 0 and once 1
RULES = ["B36/S23", "B3678/S34678", "B0257/S1468", "B13468/S02357"]


@pytest.mark.parametrize("rule", RULES + ["B2/S", "b3/s23"])
def test_rule_text_round_trip(rule):
    birth, survive = m.native().life_rule_parse(rule)
    side = rule.upper().split("/")
    assert birth == sum(1 << int(d) for d in side[0][1:]) and survive == sum(1 << int(d) for d in side[1][1:])
    assert m.native().life_rule_format(birth, survive) == rule.upper()


@pytest.mark.parametrize("bad", ["B9/S2", "3/23", ""])
def test_bad_rule_text_is_named(bad):
    with pytest.raises(RuntimeError, match="'%s'" % bad):
        m.native().life_rule_parse(bad)
    with pytest.raises(ValueError):
        m.life2d(rule=bad)


def _run(prob, steps, **kw):
    with m.Simulation(prob, device="cpu", **kw) as sim:
        sim.init()
        u0 = sim.gather()
        sim.run(steps)
        return u0, sim.gather()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("steps", [1, 5])
def test_cpu_backend_matches_reference(rule, steps):
    prob = m.life2d(h=37, w=70, rule=rule, init=m.InitCondition(kind="life", density=0.5, seed=3))
    u0, got = _run(prob, steps)
    want = reference.run("life", torch.from_numpy(u0), steps, rule=rule)
    assert 0 < int(want.sum()) < want.numel() and np.array_equal(got, want.numpy())


def test_conway_rule_is_the_default():
    init = m.InitCondition(kind="life", density=0.5, seed=4)
    _, a = _run(m.life2d(h=37, w=70, init=init), 9)
    _, b = _run(m.life2d(h=37, w=70, init=init, rule="B3/S23"), 9)
    assert a.any() and np.array_equal(a, b)
    assert m.life2d().describe() == "life 256x256 u8" and m.life2d(rule="B36/S23").describe().endswith(" B36/S23")


def test_life_cli_rule():
    p = subprocess.run([os.path.join(ROOT, "build", "bin", "life"), "--backend", "cpu", "--print", "--rule",
                        "B36/S23", "--init", "life", "--h", "30", "--w", "40", "--steps", "9", "--quiet"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=120,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    assert p.returncode == 0, p.stderr.decode()
    _, want = _run(m.life2d(h=30, w=40, rule="B36/S23"), 9)
    _, conway = _run(m.life2d(h=30, w=40), 9)
    assert p.stdout.decode() == format_array(want) and not np.array_equal(want, conway)
