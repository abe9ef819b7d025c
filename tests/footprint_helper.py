"""Memory-footprint checks of one region launch, shared by the GPU and the CPU tier
(test_gpu_footprint.py, test_footprint_cpu.py).

A field lives inside a larger flat tensor with a guard block in front of and behind its
``layout.nbytes`` bytes (the allocation slack included). Before a launch every byte of ``dst`` holds a
NaN sentinel (u8: 0xA5) and every byte of ``src`` a launch has no business with holds finite poison
(distinct values around 1e18 of both signs, u8: alive): the pad columns of every plane, ghost planes
outside the global grid, planes outside ``[lz_begin - K, lz_end + K)``, the slack and the guards.
After the launch, all bitwise:

1. the region's planes, columns [0, nx), hold K steps of the global grid (and the residual, where
   asked for, is that of step K within the project's 1e-9 * max(1, want));
2. every other element of ``dst`` still holds the sentinel (``dst`` is refilled before every launch, so
   planes an earlier launch of the same slab produced count as outside), except that a pad element of
   a written plane may hold a copy of ``src``'s pad element at the same position;
3. ``src``, guards included, is what it was.

The expected planes come from single steps over a zero-filled whole-grid layout (the CPU oracle, or
the naive kernel for K > 1 on the GPU): the same owned and real ghost data as ``src``, zeros
wherever the poison is.
"""

import functools

import torch

from mpi_cuda_process_amd import models, native
from mpi_cuda_process_amd.ops import (TORCH_DTYPE, FieldLayout, alloc_field, apply_stencil, init_field,
                                      kernel_variant, set_kernel_variant)

GUARD_BYTES = 4096
INT_VIEW = {"f32": torch.int32, "f64": torch.int64, "u8": torch.uint8}
# quiet NaNs with a payload no computation produces
SENTINEL = {"f32": 0x7FE5A5A5, "f64": 0x7FFDA5A5A5A5A5A5, "u8": 0xA5}

# weights with sum |w| <= 1 (tests/test_gpu_star7.py, tests/test_gpu_conv9.py): unowned lanes that
# evolve poison over K levels cannot grow it
STAR7_W = dict(c0=0.28, wxm=0.17, wxp=-0.03, wym=0.11, wyp=0.07, wzm=0.19, wzp=0.05)
CONV9_W = (0.07, 0.13, -0.02, 0.17, 0.26, 0.09, 0.05, -0.04, 0.11)
ROUGH = models.InitCondition(kind="random", seed=5, lo=-50.0, hi=150.0)
LIFE_RULES = {"B3/S23": "conway", "B36/S23": "highlife", "B0257/S1468": "b0"}


def guarded_field(lay, device):
    """(view, flat, start): the (planes, ny, pitch) field view apply_stencil accepts, the whole flat
    tensor around it, and the view's first element in it. At least GUARD_BYTES lie in front of the
    field and behind its nbytes; the field starts 256-byte aligned."""
    dt = TORCH_DTYPE[lay.dtype]
    es = torch.empty((), dtype=dt).element_size()
    assert lay.nbytes % es == 0 and GUARD_BYTES % es == 0
    flat = torch.empty((2 * GUARD_BYTES + 256 + lay.nbytes) // es, dtype=dt, device=device)
    start = (GUARD_BYTES + (-(flat.data_ptr() + GUARD_BYTES)) % 256) // es
    view = flat[start:start + lay.planes * lay.plane].view(lay.planes, lay.ny, lay.pitch)
    assert view.data_ptr() % 256 == 0 and view.is_contiguous()
    assert start * es >= GUARD_BYTES and (flat.numel() - start) * es - lay.nbytes >= GUARD_BYTES
    return view, flat, start


def poison_like(flat, dtype):
    """Finite poison for every element of ``flat``: u8 alive; floats (1 + j / 8192) * 1e18 with j the
    index mod 8191 and the sign from the index mod 3, so neighbours differ and 27 of them sum to
    below 6e19 (far from overflow, and exactly 0 once multiplied by a zero weight)."""
    if dtype == "u8":
        return torch.ones_like(flat)
    i = torch.arange(flat.numel(), device=flat.device)
    v = (1.0 + (i % 8191).double() / 8192.0) * 1e18
    return torch.where(i % 3 == 1, -v, v).to(flat.dtype)


def make_problem(kind, dtype, nx, ny, nz, rule="B3/S23", ref=False):
    if kind == "heat7":
        return models.heat3d(nx=nx, ny=ny, nz=nz, dtype=dtype)
    if kind == "box27":
        return models.box27(nx=nx, ny=ny, nz=nz, dtype=dtype)
    if kind == "star7":
        return models.star7(nx=nx, ny=ny, nz=nz, dtype=dtype, init=ROUGH, **STAR7_W)
    if kind == "jacobi5":
        # ref_precision at r = 0.2 (sum |w| = 1 as at the default 0.25): at a power-of-two rate the mixed
        # update is the plain one and never reaches the mixed kernels (StencilSpec::mixed_update)
        return models.mdf2d(h=nz, w=nx, dtype=dtype, r=0.2 if ref else 0.25, ref_precision=ref, init=ROUGH)
    if kind == "box9":
        return models.box9(h=nz, w=nx, dtype=dtype, init=ROUGH)
    if kind == "conv9":
        return models.conv9(h=nz, w=nx, dtype=dtype, init=ROUGH, w9=CONV9_W)
    return models.life2d(h=nz, w=nx, rule=rule, init=models.InitCondition(kind="life", density=0.5, seed=7))


@functools.lru_cache(maxsize=64)
def generations(prob, k, device):
    """Dense generations 0..k of the whole grid, on ``device``: the CPU oracle's single steps, on the
    GPU for k > 1 the naive kernel's (as the fused bitwise tests)."""
    dev = "cpu" if k == 1 else device
    lay = FieldLayout.make(prob, halo=1)
    cur = alloc_field(lay, dev)
    init_field(prob, lay, cur)
    gens = [cur[lay.owned, :, :lay.nx].clone()]
    selected = kernel_variant()
    set_kernel_variant("naive")
    try:
        for _ in range(k):
            nxt = cur.clone()
            apply_stencil(prob, lay, cur, nxt)
            cur = nxt
            gens.append(cur[lay.owned, :, :lay.nx].clone())
    finally:
        set_kernel_variant(selected)
    return [g.to(device) for g in gens]


def _residual(prob, a, b):
    if prob.dtype == "u8":
        return float((a != b).sum().item())
    return float(((a.double() - b.double()) ** 2).sum().item())


class Footprint:
    """One slab of ``prob`` (global planes [z0, z1), ``k`` ghost planes) with a guarded src and dst."""

    def __init__(self, prob, k, z0, z1, device):
        self.prob, self.k, self.device = prob, k, device
        self.lay = lay = FieldLayout.make(prob, z0, z1, halo=k)
        self.idt = INT_VIEW[prob.dtype]
        self.src, self.src_flat, self.start = guarded_field(lay, device)
        self.dst, self.dst_flat, dstart = guarded_field(lay, device)
        self.dstart = dstart
        self.poison = poison_like(self.src_flat, prob.dtype)
        self.src_flat.copy_(self.poison)
        init_field(prob, lay, self.src)  # owned planes and ghosts by global index; zeros elsewhere
        self.init = self.src_flat.clone()
        self.written = []  # storage planes of the current launch's regions
        self.gens = generations(prob, k, device)
        self.pad = set()

    def _span(self, flat, start):
        n = self.lay.planes * self.lay.plane
        return flat[start:start + n].view(self.lay.planes, self.lay.ny, self.lay.pitch)

    def _fill_src(self, regions):
        """Real data on the in-grid planes within K of a region, columns [0, nx); poison elsewhere."""
        lay, k = self.lay, self.k
        keep = torch.zeros_like(self.src_flat, dtype=torch.bool)
        kv = self._span(keep, self.start)
        for lo, hi in regions:
            for lz in range(max(lo - k, 0), min(hi + k, lay.planes)):
                if 0 <= lz - lay.halo + lay.z0 < lay.nz:
                    kv[lz, :, :lay.nx] = True
        self.src_flat.copy_(torch.where(keep, self.init, self.poison))

    def launch(self, regions, resid):
        """One apply_stencil call over one region or a ``second=`` pair, then the three assertions."""
        prob, lay, k = self.prob, self.lay, self.k
        self._fill_src(regions)
        # every launch starts from a dst that is sentinel throughout, so a plane an earlier launch
        # produced counts as outside this one (an interior launch that rewrote a boundary plane, even
        # with the right values, would race with the halo stream in the engine)
        self.dst_flat.view(self.idt).fill_(SENTINEL[prob.dtype])
        self.written = []
        before = self.src_flat.view(self.idt).clone()
        res = torch.zeros((), dtype=torch.float64, device=self.device) if resid else None
        apply_stencil(prob, lay, self.src, self.dst, regions[0][0], regions[0][1], steps=k, resid=res,
                      second=regions[1] if len(regions) > 1 else None)
        if self.device != "cpu":
            torch.cuda.synchronize()
        # 3. src untouched
        assert torch.equal(self.src_flat.view(self.idt), before), "the launch wrote into src"
        # 1. the region holds K steps of the global grid
        want_res = 0.0
        for lo, hi in regions:
            g0 = lo - lay.halo + lay.z0
            want = self.gens[k][g0:g0 + hi - lo]
            got = self.dst[lo:hi, :, :lay.nx]
            assert torch.equal(got.view(self.idt), want.view(self.idt)), \
                "planes [%d, %d): %d cells differ" % (lo, hi, int((got.view(self.idt) != want.view(self.idt)).sum()))
            want_res += _residual(prob, want, self.gens[k - 1][g0:g0 + hi - lo])
            self.written += list(range(lo, hi))
        if resid:
            assert abs(res.item() - want_res) <= 1e-9 * max(1.0, want_res), (res.item(), want_res)
        # 2. nothing else was written
        self.check_untouched()

    def check_untouched(self):
        lay = self.lay
        sent = SENTINEL[self.prob.dtype]
        di = self.dst_flat.view(self.idt)
        outside = torch.ones_like(di, dtype=torch.bool)
        self._span(outside, self.dstart)[self.written] = False
        bad = outside & (di != sent)
        if bool(bad.any()):
            at = torch.nonzero(bad).flatten()[:8] - self.dstart
            where = [(int(i) // lay.plane, int(i) % lay.plane // lay.pitch, int(i) % lay.pitch) if 0 <= i < lay.planes * lay.plane
                     else int(i) for i in at]
            raise AssertionError("%d elements outside the written planes %s changed; first (plane, row, x) or flat "
                                 "offsets: %s" % (int(bad.sum()), sorted(set(self.written)), where))
        if lay.pitch > lay.nx:
            pad = self._span(di, self.dstart)[self.written][:, :, lay.nx:]
            spad = self.src.view(self.idt)[self.written][:, :, lay.nx:]
            kept, copied = pad == sent, pad == spad
            assert bool((kept | copied).all()), "%d pad elements of the written planes hold computed values" % \
                int((~(kept | copied)).sum())
            self.pad.add("untouched" if bool(kept.all()) else "copied" if bool(copied.all()) else "mixed")


def run_case(device, kind, dtype, k, nx, ny, nz, geometry, rule="B3/S23", ref=False):
    """Geometry "whole": the whole grid as one region (every ghost plane outside the grid). "slab": a
    middle slab of 2K + 3 planes, K + 1 planes above the grid's first and K below its last, as three
    launches (lower K planes, upper K planes, interior), each into a dst that is sentinel throughout and
    checked on its own. "pair": both boundary
    regions of that slab in one call. ``nz`` is the whole grid's height; the slab cases take 4K + 4.
    Returns the pad behaviours seen ("untouched", "copied", "mixed"; empty for rows without pad)."""
    if geometry == "whole":
        fp = Footprint(make_problem(kind, dtype, nx, ny, nz, rule, ref), k, 0, nz, device)
        fp.launch([(k, k + nz)], resid=True)
        return fp.pad
    z0, n = k + 1, 2 * k + 3
    fp = Footprint(make_problem(kind, dtype, nx, ny, z0 + n + k, rule, ref), k, z0, z0 + n, device)
    lower, upper, inner = (k, 2 * k), (k + n - k, k + n), (2 * k, k + n - k)
    if geometry == "pair":
        fp.launch([lower, upper], resid=True)
    else:
        for r in (lower, upper, inner):
            fp.launch([r], resid=False)
    return fp.pad


# (kind, dtypes, depths) of the issue's table; life rows per rule
TABLE = [("heat7", ("f32", "f64"), (1, 2, 3, 4, 5)), ("box27", ("f32", "f64"), (1, 2, 3)),
         ("jacobi5", ("f32", "f64", "f32ref"), (1, 2, 3, 4, 6, 8)), ("box9", ("f32", "f64"), (1, 2, 3, 4, 6, 8)),
         ("conv9", ("f32", "f64"), (1, 2, 3, 4, 6, 8)), ("star7", ("f32", "f64"), (1, 2, 3, 4)),
         ("life", tuple(LIFE_RULES), (1, 2, 3, 4, 6, 8, 12, 16))]
# (nx, ny, whole-grid nz): narrower than a wave with a large pad; several waves and a ragged tail; more
# than one wxk segment and block; "nopad": a row without pad (256 cells, 512 in fp64), whose right
# neighbour at x = nx-1 is the next row's first cell or, on the last row, the slack
SHAPES_3D = [(70, 9, 11), (300, 13, 9), (1030, 7, 8), ("nopad", 5, 12)]
# 2D: (w, h); h = 5 is shorter than every fused pipeline (h < 2K + 3 from K = 2 on)
SHAPES_2D = [(70, 19), (300, 33), (1030, 45), ("nopad", 5)]
GEOMETRIES = ("whole", "slab", "pair")


def cases(shapes_3d=SHAPES_3D, shapes_2d=SHAPES_2D, life_wide=True, wide_f64=True):
    """Every (kind, dtype, K, shape, geometry) of the table that hip_supports_steps accepts at the
    extent that geometry launches, as (test id, run_case keywords). "whole" launches nz planes; "slab"
    and "pair" launch on a slab of a grid of 4K + 4 planes (the query takes a whole grid of that
    height with K ghost planes: the predicates look at the row geometry and the halo). The filter
    leaves out box27 at K = 2 on 1030-cell rows, f32 and f64, in all three geometries: box27_tb2 /
    box27_tbk keep a row within one block (1024 cells, fp64 512), and box27 has no other two-step
    kernel."""
    out = []
    for kind, dts, depths in TABLE:
        for dt in dts:
            rule, ref, dtype = "B3/S23", dt == "f32ref", dt.replace("ref", "")
            if kind == "life":
                rule, dtype = dt, "u8"
            if kind in ("heat7", "box27", "star7"):
                shapes = list(shapes_3d)
                if kind == "heat7" and dtype == "f64" and wide_f64:
                    shapes.append((2050, 6, 9))  # K = 5 in rows of one cell per lane
            else:
                shapes = [(w, 1, h) for w, h in shapes_2d] + ([(2100, 1, 23)] if kind == "life" and life_wide else [])
            for nx, ny, nz in shapes:
                if nx == "nopad":
                    nx = 512 if dtype == "f64" else 256
                for k in depths:
                    for geometry in GEOMETRIES:
                        planes = nz if geometry == "whole" else 4 * k + 4
                        if not native().hip_supports_steps(kind, dtype, nx, ny, planes, k, k, ref, rule):
                            continue
                        tag = "%s-%s-%dx%dx%d-k%d-%s" % (kind, LIFE_RULES[dt] if kind == "life" else dt, nx, ny, nz, k,
                                                         geometry)
                        out.append((tag, dict(kind=kind, dtype=dtype, k=k, nx=nx, ny=ny, nz=nz, rule=rule, ref=ref,
                                              geometry=geometry)))
    return out


# ---- the engine upholds the kernels' precondition ---------------------------------------------------

ENGINE_CASES = [("heat7", "f32", 520, 6), ("heat7", "f64", 520, 6), ("box27", "f32", 300, 5), ("box27", "f64", 70, 5),
                ("star7", "f32", 70, 7), ("jacobi5", "f32", 300, 1), ("jacobi5", "f64", 70, 1), ("box9", "f32", 300, 1),
                ("conv9", "f64", 130, 1), ("life", "u8", 300, 1), ("life", "B36/S23", 300, 1)]


def _assert_pad_and_outer_ghosts_zero(sim, when):
    nx, nz = sim.problem.nx, sim.problem.nz
    idt = INT_VIEW[sim.problem.dtype]
    for i in range(sim.num_local):
        lay = sim.layout(i)
        for current in (True, False):
            v = sim.view(i, current).view(idt)
            assert int((v[:, :, nx:] != 0).sum()) == 0, "%s: slab %d pad columns are not all zero bits" % (when, i)
            for lz in range(v.shape[0]):
                gz = lz - lay["halo"] + lay["z0"]
                if gz < 0 or gz >= nz:
                    assert int((v[lz] != 0).sum()) == 0, "%s: slab %d ghost plane gz = %d is not zero" % (when, i, gz)


def engine_keeps_pad_and_outer_ghosts_zero(device, kind, dtype, nx, ny, ranks, tmp_path):
    """init() + run() at the kind's default fused depth with a residual interval, then a checkpoint
    round trip into a fresh engine and a further run: every pad column and every ghost plane outside
    the global grid of both buffers of every slab is still zero, bitwise. (The kernels hold Dirichlet
    cells with zero weights over whatever those locations contain: docs/DESIGN.md.)"""
    import mpi_cuda_process_amd as mm

    rule = dtype if kind == "life" and dtype != "u8" else "B3/S23"
    dtype = "u8" if kind == "life" else dtype
    k = native().hip_fused_depth(kind, dtype, nx, False, rule=rule)
    prob = make_problem(kind, dtype, nx, ny, 4 * k * 3 + 1, rule)
    opts = dict(device=device, ranks=ranks, temporal=k, residual_every=k + 2)
    with mm.Simulation(prob, **opts) as sim:
        sim.init()
        sim.synchronize()
        _assert_pad_and_outer_ghosts_zero(sim, "after init")
        sim.run(2 * k + 3)
        sim.synchronize()
        assert sim.residual > 0
        _assert_pad_and_outer_ghosts_zero(sim, "after run")
        sim.save_checkpoint(str(tmp_path))
        want = sim.gather()
    with mm.Simulation(prob, **opts) as sim:
        sim.load_checkpoint(str(tmp_path))
        sim.synchronize()
        assert (sim.gather() == want).all()
        _assert_pad_and_outer_ghosts_zero(sim, "after restore")
        sim.run(k + 1)
        sim.synchronize()
        _assert_pad_and_outer_ghosts_zero(sim, "after the restored run")
