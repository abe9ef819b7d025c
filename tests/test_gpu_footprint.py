"""What a tuned kernel launch writes and what it depends on, on the MI355X (footprint_helper.py):
the region's planes bitwise equal to K single steps, a NaN sentinel intact everywhere else in dst
(guards, slack, ghost planes, owned planes outside the region, pad), src untouched, and finite poison
in every src location outside the launch's window (pad columns, out-of-grid ghost planes, planes
beyond K of the region, slack, guards) without effect on any owned cell. Every kind, dtype and fused
depth hip_supports_steps accepts, as the whole grid, as three region launches on a middle slab and as
the ``second=`` pair of boundary regions."""

import pytest

pytestmark = pytest.mark.gpu

from footprint_helper import (ENGINE_CASES, cases, engine_keeps_pad_and_outer_ghosts_zero,  # noqa: E402
                              run_case)
from mpi_cuda_process_amd.ops import set_kernel_variant  # noqa: E402

CASES = cases()


def _run(record_property, **case):
    set_kernel_variant("tuned")
    try:
        pad = run_case("cuda", **case)
    finally:
        set_kernel_variant("auto")
    record_property("pad", "+".join(sorted(pad)) or "none")


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[t for t, _ in CASES])
def test_launch_footprint(hip, record_property, case):
    """Default dispatch: heat7 / heat7_tbk / heat7_tb2 / heat7_wtk / heat7_wxk (fp64 K = 5 at 2050-cell
    rows in one cell per lane), box27 / box27_tb2 / box27_tbk / box27_wxk, jacobi5 / jacobi5_tb2 /
    jacobi5_tbk (REF), box9_wave / box9_tbk, conv9_tbk, star7_tbk, life / life_tb2 / life_bits and
    life_rule_bits (B36/S23, a B0 rule)."""
    _run(record_property, **case)


def _pick(kind, dtype, ks):
    return [(t, c) for t, c in CASES if c["kind"] == kind and c["dtype"] == dtype and c["k"] in ks and not c["ref"]]


# the knob settings of the bitwise suites (test_gpu_temporal.py) that force a kernel family or tile
FORCED = ([(t + "-ry" + ry, c, {"MDFX_TB_RY": ry}) for ry in ("1", "2") for dt in ("f32", "f64") for t, c in _pick("heat7", dt, (2,))] +
          [(t + "-ry" + ry, c, {"MDFX_TB_RY": ry}) for ry in ("1", "2") for dt in ("f32", "f64") for t, c in _pick("box27", dt, (2,))] +
          [(t + "-wtk-wb" + wb, c, {"MDFX_H7_WXK": "0", "MDFX_WTK_WB": wb}) for wb, ks in (("4", (3, 4)), ("8", (3,)))
           for t, c in _pick("heat7", "f64", ks)] +
          [(t + "-wxk", c, {"MDFX_H7_WXK": "1"}) for t, c in _pick("heat7", "f64", (3,))])


@pytest.mark.parametrize("case,knobs", [(c, k) for _, c, k in FORCED], ids=[t for t, _, _ in FORCED])
def test_forced_family_footprint(hip, record_property, knob, case, knobs):
    """MDFX_TB_RY 1 / 2 rows per tile (heat7_tb2 / heat7_tbk, box27_tb2 / box27_tbk), heat7_wtk in bands
    of 4 / 8 waves (fp64, MDFX_H7_WXK=0), and heat7_wxk's fp64 K = 3 below 2048-cell rows."""
    for name, value in knobs.items():
        knob(name, value)
    _run(record_property, **case)


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("kind,dtype,nx,ny", ENGINE_CASES, ids=lambda v: str(v).replace("/", ""))
def test_engine_keeps_pad_and_outer_ghosts_zero(hip, kind, dtype, nx, ny, ranks, tmp_path):
    engine_keeps_pad_and_outer_ghosts_zero("hip", kind, dtype, nx, ny, ranks, tmp_path)
