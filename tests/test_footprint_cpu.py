"""The footprint checks of tests/test_gpu_footprint.py against the CPU oracle (single steps and the
CPU backend's fused sweeps): the helper, the poison values and the expected planes are proven
without a GPU, and the oracle's own footprint, which the GPU comparisons lean on, is pinned."""

import pytest
import torch

from footprint_helper import (ENGINE_CASES, GUARD_BYTES, SENTINEL, Footprint, cases,
                              engine_keeps_pad_and_outer_ghosts_zero, guarded_field, make_problem,
                              poison_like, run_case)
from mpi_cuda_process_amd.ops import FieldLayout

# a row narrower than a wave with a large pad, and a row without pad; every kind, dtype and depth
CASES = cases(shapes_3d=[(70, 9, 11), ("nopad", 5, 12)], shapes_2d=[(70, 19), ("nopad", 5)], life_wide=False,
              wide_f64=False)


@pytest.mark.parametrize("case", [c for _, c in CASES], ids=[t for t, _ in CASES])
def test_oracle_footprint(case):
    pad = run_case("cpu", **case)
    assert pad <= {"untouched"}  # the oracle writes columns [0, nx) only


@pytest.mark.parametrize("dtype", ["f32", "f64", "u8"])
def test_guarded_field_layout(dtype):
    prob = make_problem("life" if dtype == "u8" else "heat7", dtype, 70, 1 if dtype == "u8" else 5, 9)
    lay = FieldLayout.make(prob, 2, 7, halo=2)
    view, flat, start = guarded_field(lay, "cpu")
    es = flat.element_size()
    assert view.data_ptr() % 256 == 0 and view.data_ptr() == flat.data_ptr() + start * es
    assert tuple(view.shape) == (lay.planes, lay.ny, lay.pitch)
    assert start * es >= GUARD_BYTES and flat.numel() * es - start * es - lay.nbytes >= GUARD_BYTES
    p = poison_like(flat, dtype)
    if dtype == "u8":
        assert bool((p == 1).all())
    else:
        assert bool(torch.isfinite(p).all()) and 0.99e18 <= float(p.abs().min()) and float(p.abs().max()) < 2e18
        assert bool((p > 0).any()) and bool((p < 0).any()) and bool((p[1:] != p[:-1]).all())
        # 27 of them times a zero weight are exactly 0, and the sentinel is a NaN
        assert float((p[:27].sum() * 0).abs()) == 0.0
        s = torch.zeros(1, dtype=flat.dtype)
        s.view(torch.int32 if dtype == "f32" else torch.int64).fill_(SENTINEL[dtype])
        assert bool(torch.isnan(s).all())


def test_src_fill_places_poison():
    """Owned and in-grid ghost planes within K of the region keep init_field's data in columns
    [0, nx); pad, out-of-grid ghosts, planes beyond the window, slack and guards hold the poison."""
    k = 2
    prob = make_problem("heat7", "f32", 70, 5, 4 * k + 4)
    fp = Footprint(prob, k, k + 1, 3 * k + 4, "cpu")
    lay = fp.lay
    fp._fill_src([(k, 2 * k)])  # the lower boundary region: window = storage planes [0, 3K)
    pv = fp._span(fp.poison, fp.start)
    iv = fp._span(fp.init, fp.start)
    assert torch.equal(fp.src[:3 * k, :, :lay.nx], iv[:3 * k, :, :lay.nx])
    assert torch.equal(fp.src[:, :, lay.nx:], pv[:, :, lay.nx:]) and torch.equal(fp.src[3 * k:], pv[3 * k:])
    n = lay.planes * lay.plane
    assert torch.equal(fp.src_flat[:fp.start], fp.poison[:fp.start])
    assert torch.equal(fp.src_flat[fp.start + n:], fp.poison[fp.start + n:])
    # a whole grid: every ghost plane is outside the grid
    fw = Footprint(make_problem("heat7", "f32", 70, 5, 6), k, 0, 6, "cpu")
    fw._fill_src([(k, k + 6)])
    pw = fw._span(fw.poison, fw.start)
    assert torch.equal(fw.src[:k], pw[:k]) and torch.equal(fw.src[k + 6:], pw[k + 6:])


@pytest.mark.parametrize("ranks", [1, 3])
@pytest.mark.parametrize("kind,dtype,nx,ny", ENGINE_CASES, ids=lambda v: str(v).replace("/", ""))
def test_engine_keeps_pad_and_outer_ghosts_zero(kind, dtype, nx, ny, ranks, tmp_path):
    engine_keeps_pad_and_outer_ghosts_zero("cpu", kind, dtype, nx, ny, ranks, tmp_path)
