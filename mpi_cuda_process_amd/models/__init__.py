"""Problem ("model") families of the stencil engine.

A :class:`Problem` names the stencil, the grid, the element type, the update coefficients and
the default initial condition. Families (reference parity in brackets):

* :func:`mdf2d`   — 2D 5-point heat / Jacobi, Dirichlet edges = 100, interior 0
  [MDF_kernel.cu:10-22 update, :88-99 initial grid]
* :func:`life2d`  — Conway's Game of Life, Moore-8, B3/S23, dead frame, density 0.15
  [kernel.cu:10-68 update, :131-146 initial grid]; ``rule="B36/S23"`` runs any other Life-like
  (outer-totalistic) rule, ``rule="B2/S345/C4"`` a Generations rule with C cell states (0 dead,
  1 alive, 2 .. C-1 dying; Brian's Brain ``B2/S/C3``, Star Wars ``B2/S345/C4``)
* :func:`heat3d`  — 3D 7-point heat / Jacobi (headline benchmark, BASELINE.json configs 2, 3, 5)
* :func:`box27`   — 3D 27-point weighted stencil (BASELINE.json config 4)
* :func:`box9`    — 2D 9-point weighted stencil (centre, edge and corner weights), Dirichlet edges
* :func:`star7`   — 3D 7-point star with seven independent weights (anisotropic grids and conductivities,
  constant-velocity advection-diffusion, decay), Dirichlet faces
* :func:`conv9`   — 2D 9-point stencil with nine independent weights (any 3x3 linear update: upwind
  advection-diffusion, anisotropic conductivities, a full diffusion tensor, blur, sharpening), Dirichlet edges
* :func:`star13`  — 3D radius-2 star, the 13 points of the fourth-order Laplacian (seismic, wave and
  high-accuracy diffusion codes); the held frame is two cells thick

2D grids are stored as ``nx = w, ny = 1, nz = h``: rows are the slab axis, exactly like the
reference's row split (MDF_kernel.cu:30,54).
"""

from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Optional

KINDS = ("jacobi5", "life", "heat7", "box27", "box9", "star7", "conv9", "star13")
KINDS_2D = ("jacobi5", "life", "box9", "conv9")

# the default weights of conv9, row-major: a diffusion with a positive cross term; non-negative, summing to 1
CONV9_DEFAULT = (0.06, 0.10, 0.02, 0.14, 0.36, 0.14, 0.02, 0.10, 0.06)


@dataclass(frozen=True)
class InitCondition:
    kind: str = "random"  # constant | dirichlet | random | life | compat (GoL glibc rand, host)
    seed: int = 1
    lo: float = 0.0
    hi: float = 1.0
    value: float = 0.0
    edge: float = 100.0
    interior: float = 0.0
    density: float = 0.15


@dataclass(frozen=True)
class Problem:
    kind: str
    nx: int
    ny: int
    nz: int
    dtype: str = "f32"
    r: float = -1.0  # 5/7-pt rate; < 0 -> 1/(2d) (Jacobi)
    c0: float = 0.25
    c1: float = 1.0 / 20.0
    c2: float = 1.0 / 40.0
    c3: float = 3.0 / 160.0
    # star7 only: the neighbour weights (wxm multiplies u(x-1), wxp multiplies u(x+1), ...); c0 is the centre
    wxm: float = 0.20
    wxp: float = 0.20
    wym: float = 0.10
    wyp: float = 0.10
    wzm: float = 0.05
    wzp: float = 0.05
    # conv9 only: nine weights, row-major; w9[3*(dz+1) + (dx+1)] multiplies u(z+dz, x+dx) (z the row, x along it)
    w9: tuple = CONV9_DEFAULT
    # 2D MDF: evaluate the update exactly as the reference does (fp32 sum, fp64 scale and add;
    # MDF_kernel.cu:20) instead of wholly in the field type; single-step sweeps only
    ref_precision: bool = False
    # Life only: the rule in B/S notation (digits = neighbour counts that give birth / let a cell
    # survive), any of the 2^18 outer-totalistic Moore rules, optionally with /C<n>: a Generations rule
    # with n = 2 .. 256 cell states (``states``); parsed by the native core, and the text carries the
    # state count through coef_kwargs() to every native call
    rule: str = "B3/S23"
    init: InitCondition = field(default_factory=InitCondition)

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError("unknown stencil kind %r (one of %s)" % (self.kind, ", ".join(KINDS)))
        if self.kind in KINDS_2D and self.ny != 1:
            raise ValueError("2D problems use ny == 1 (nx = width, nz = height)")
        if self.kind == "life" and self.dtype != "u8":
            raise ValueError("life cells are u8")
        if self.kind != "life" and self.dtype not in ("f32", "f64"):
            raise ValueError("stencil dtype must be f32 or f64")
        if self.rule != "B3/S23":
            if self.kind != "life":
                raise ValueError("rule applies to kind 'life' only")
            from .._native import native

            try:
                native().life_rule_parse(self.rule)
            except RuntimeError as e:
                raise ValueError(str(e)) from None
        object.__setattr__(self, "w9", tuple(float(v) for v in self.w9))
        if len(self.w9) != 9:
            raise ValueError("w9 takes nine weights, row-major (got %d)" % len(self.w9))
        for n in (self.nx, self.ny, self.nz):
            if n < 1:
                raise ValueError("grid extents must be positive")

    @property
    def dims(self) -> int:
        return 2 if self.kind in KINDS_2D else 3

    @property
    def radius(self) -> int:
        """How far the stencil reaches along each axis: ghost planes per fused step, and the thickness
        of the held frame."""
        return 2 if self.kind == "star13" else 1

    @property
    def cells(self) -> int:
        return self.nx * self.ny * self.nz

    @property
    def rate(self) -> float:
        if self.r >= 0:
            return self.r
        return 0.25 if self.kind in ("jacobi5", "box9", "conv9") else 1.0 / 6.0

    @property
    def bytes_per_cell_per_step(self) -> int:
        """Minimum HBM traffic of one sweep (one read + one write of every cell)."""
        return 2 * {"f32": 4, "f64": 8, "u8": 1}[self.dtype]

    def with_init(self, **kw) -> "Problem":
        return replace(self, init=replace(self.init, **kw))

    def coef_kwargs(self) -> dict:
        return dict(r=self.r, c0=self.c0, c1=self.c1, c2=self.c2, c3=self.c3, ref_precision=self.ref_precision,
                    rule=self.rule, wxm=self.wxm, wxp=self.wxp, wym=self.wym, wyp=self.wyp, wzm=self.wzm,
                    wzp=self.wzp, w9=self.w9)

    @property
    def states(self) -> int:
        """Cell states: 2, or the C of a Generations rule B/S/C."""
        return native_states(self.rule) if self.kind == "life" else 2

    @property
    def conway(self) -> bool:
        return self.kind != "life" or (native_rule(self.rule) == (0x008, 0x00C) and self.states == 2)

    def describe(self) -> str:
        shape = "%dx%d" % (self.nz, self.nx) if self.dims == 2 else "%dx%dx%d" % (self.nx, self.ny, self.nz)
        return "%s %s %s" % (self.kind, shape, self.dtype) + ("" if self.conway else " " + self.rule)


def native_rule(rule: str) -> tuple:
    """(birth, survive) 9-bit masks of a rule text, through the native parser."""
    from .._native import native

    return tuple(native().life_rule_parse(rule))


def native_states(rule: str) -> int:
    """The number of cell states of a rule text (2 without a /C part), through the native parser."""
    from .._native import native

    return int(native().life_rule_states(rule))


def mdf2d(h: int = 256, w: int = 256, dtype: str = "f32", r: float = 0.25,
          init: Optional[InitCondition] = None, ref_precision: bool = False) -> Problem:
    """2D 5-point MDF (finite-difference) heat / Jacobi problem, Dirichlet edges 100.
    ``ref_precision`` pins the reference's mixed fp32/fp64 evaluation of the update."""
    return Problem("jacobi5", nx=w, ny=1, nz=h, dtype=dtype, r=r, ref_precision=ref_precision,
                   init=init or InitCondition(kind="dirichlet", edge=100.0, interior=0.0))


def life2d(h: int = 256, w: int = 256, density: float = 0.15, seed: int = 1,
           init: Optional[InitCondition] = None, rule: str = "B3/S23") -> Problem:
    """Game of Life on an h x w board with a dead frame: Conway's rule, or any Life-like ``rule``
    (HighLife "B36/S23", Day & Night "B3678/S34678", Seeds "B2/S", ...), or a Generations rule
    "B<n>/S<n>/C<states>" whose cells age through states 2 .. C-1 before they die (cells hold 0 .. C-1;
    the ``life`` initial condition writes 0 and 1)."""
    return Problem("life", nx=w, ny=1, nz=h, dtype="u8", rule=rule,
                   init=init or InitCondition(kind="life", density=density, seed=seed))


def heat3d(n: int = 512, nx: Optional[int] = None, ny: Optional[int] = None, nz: Optional[int] = None,
           dtype: str = "f32", r: float = -1.0, init: Optional[InitCondition] = None) -> Problem:
    """3D 7-point heat / Jacobi problem on an nx x ny x nz grid (default n^3)."""
    return Problem("heat7", nx=nx or n, ny=ny or n, nz=nz or n, dtype=dtype, r=r,
                   init=init or InitCondition(kind="random", seed=1))


def box27(n: int = 512, nx: Optional[int] = None, ny: Optional[int] = None, nz: Optional[int] = None,
          dtype: str = "f32", c0: float = 0.25, c1: float = 1.0 / 20.0, c2: float = 1.0 / 40.0,
          c3: float = 3.0 / 160.0, init: Optional[InitCondition] = None) -> Problem:
    """3D 27-point weighted stencil u' = c0 u + c1 faces + c2 edges + c3 corners."""
    return Problem("box27", nx=nx or n, ny=ny or n, nz=nz or n, dtype=dtype, c0=c0, c1=c1, c2=c2,
                   c3=c3, init=init or InitCondition(kind="random", seed=1))


def box9(h: int = 256, w: int = 256, dtype: str = "f32", c0: float = 1.0 / 3.0, c1: float = 2.0 / 15.0,
         c2: float = 1.0 / 30.0, init: Optional[InitCondition] = None) -> Problem:
    """2D 9-point weighted stencil u' = c0 u + c1 edges + c2 corners on an h x w grid, Dirichlet edges
    100. The default weights are u + (1/30) * (4 edges + corners - 20 u): the compact fourth-order
    ("Mehrstellen") Laplacian's 4 : 1 proportion; they sum to 1."""
    return Problem("box9", nx=w, ny=1, nz=h, dtype=dtype, c0=c0, c1=c1, c2=c2,
                   init=init or InitCondition(kind="dirichlet", edge=100.0, interior=0.0))


def star7(n: int = 256, nx: Optional[int] = None, ny: Optional[int] = None, nz: Optional[int] = None,
          dtype: str = "f32", c0: float = 0.30, wxm: float = 0.20, wxp: float = 0.20, wym: float = 0.10,
          wyp: float = 0.10, wzm: float = 0.05, wzp: float = 0.05, init: Optional[InitCondition] = None) -> Problem:
    """3D 7-point star u' = c0 u + wxm u(x-1) + wxp u(x+1) + wym u(y-1) + wyp u(y+1) + wzm u(z-1) +
    wzp u(z+1) on an nx x ny x nz grid (default n^3), Dirichlet faces. The default is an anisotropic
    diffusion whose weights sum to 1. Weights must be finite; sum |w| <= 1 keeps the max-norm from
    growing."""
    return Problem("star7", nx=nx or n, ny=ny or n, nz=nz or n, dtype=dtype, c0=c0, wxm=wxm, wxp=wxp, wym=wym,
                   wyp=wyp, wzm=wzm, wzp=wzp, init=init or InitCondition(kind="random", seed=1))


def conv9(h: int = 256, w: int = 256, dtype: str = "f32", w9=CONV9_DEFAULT,
          init: Optional[InitCondition] = None) -> Problem:
    """2D 9-point stencil with nine independent weights on an h x w grid, Dirichlet edges 100:
    u'(z, x) = sum over dz, dx in {-1, 0, 1} of w9[3*(dz+1) + (dx+1)] * u(z+dz, x+dx), ``w9`` row-major
    (z is the row, x runs along it). The default is a diffusion with a positive cross term whose weights
    sum to 1. Weights must be finite; sum |w| <= 1 keeps the max-norm from growing."""
    return Problem("conv9", nx=w, ny=1, nz=h, dtype=dtype, w9=tuple(w9),
                   init=init or InitCondition(kind="dirichlet", edge=100.0, interior=0.0))


def star13(n: int = 256, nx: Optional[int] = None, ny: Optional[int] = None, nz: Optional[int] = None,
           dtype: str = "f32", c0: Optional[float] = None, c1: Optional[float] = None, c2: Optional[float] = None,
           r: Optional[float] = None, init: Optional[InitCondition] = None) -> Problem:
    """3D radius-2 star u' = c0 u + c1 (the 6 neighbours at distance 1) + c2 (the 6 at distance 2 along the
    axes) on an nx x ny x nz grid (default n^3). ``r`` sets the explicit fourth-order heat step
    u + r Lap4(u): c0 = 1 - 7.5 r, c1 = 4 r / 3, c2 = -r / 12 (the default is r = 0.1: weights summing to 1,
    sum |w| = 1.1); ``c0, c1, c2`` given explicitly win over it. Weights must be finite.

    A cell is held (copied through) iff one of its coordinates is within 2 of a face, so no update reads
    outside the grid, and a grid with an extent below 5 never changes. The ``dirichlet`` initial condition
    still paints a one-cell frame: the second layer is held at its interior value."""
    r = 0.1 if r is None else r
    return Problem("star13", nx=nx or n, ny=ny or n, nz=nz or n, dtype=dtype,
                   c0=1.0 - 7.5 * r if c0 is None else c0, c1=4.0 * r / 3.0 if c1 is None else c1,
                   c2=-r / 12.0 if c2 is None else c2, init=init or InitCondition(kind="random", seed=1))


def from_name(kind: str, **kw) -> Problem:
    aliases = {"5": "jacobi5", "mdf": "jacobi5", "jacobi5": "jacobi5", "life": "life", "gol": "life",
               "7": "heat7", "heat7": "heat7", "jacobi7": "heat7", "27": "box27", "box27": "box27",
               "9": "box9", "9pt": "box9", "box9": "box9", "star7": "star7", "s7": "star7",
               "conv9": "conv9", "c9": "conv9", "3x3": "conv9", "star13": "star13", "13": "star13", "s13": "star13"}
    k = aliases.get(str(kind))
    if k is None:
        raise ValueError("unknown stencil %r" % kind)
    return {"jacobi5": mdf2d, "life": life2d, "heat7": heat3d, "box27": box27, "box9": box9,
            "star7": star7, "conv9": conv9, "star13": star13}[k](**kw)


__all__ = ["Problem", "InitCondition", "mdf2d", "life2d", "heat3d", "box27", "box9", "star7", "conv9", "star13", "from_name", "KINDS"]
