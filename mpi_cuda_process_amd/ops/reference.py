"""Plain-PyTorch reference implementations of every stencil (the test oracle for the HIP kernels).

Each function takes a dense global grid ``u`` of shape ``(nz, ny, nx)`` (2D problems:
``(h, 1, w)``) and returns one updated grid. Global-boundary cells are held (Dirichlet /
dead frame), exactly the engine's semantics. These use ordinary tensor ops (no fused multiply-add),
so against the kernels they agree to rounding, not bitwise; the CPU oracle in the native core is
the bitwise reference.
"""

from __future__ import annotations

import torch


def heat7(u: torch.Tensor, r: float = 1.0 / 6.0) -> torch.Tensor:
    out = u.clone()
    if min(u.shape) < 3:
        return out
    c = u[1:-1, 1:-1, 1:-1]
    s = (((((u[1:-1, 1:-1, :-2] + u[1:-1, 1:-1, 2:]) + u[1:-1, :-2, 1:-1]) + u[1:-1, 2:, 1:-1])
          + u[:-2, 1:-1, 1:-1]) + u[2:, 1:-1, 1:-1])
    out[1:-1, 1:-1, 1:-1] = c + r * (s - 6.0 * c)
    return out


def jacobi5(u: torch.Tensor, r: float = 0.25) -> torch.Tensor:
    """2D 5-point; ``u`` is (h, 1, w) or (h, w)."""
    squeeze = u.dim() == 2
    g = u if squeeze else u[:, 0, :]
    out = g.clone()
    if min(g.shape) >= 3:
        c = g[1:-1, 1:-1]
        s = ((g[1:-1, :-2] + g[1:-1, 2:]) + g[:-2, 1:-1]) + g[2:, 1:-1]
        out[1:-1, 1:-1] = c + r * (s - 4.0 * c)
    return out if squeeze else out.unsqueeze(1)


def box27(u: torch.Tensor, c0: float = 0.25, c1: float = 1.0 / 20.0, c2: float = 1.0 / 40.0,
          c3: float = 3.0 / 160.0) -> torch.Tensor:
    out = u.clone()
    if min(u.shape) < 3:
        return out
    nz, ny, nx = u.shape
    faces = torch.zeros_like(u[1:-1, 1:-1, 1:-1])
    edges = torch.zeros_like(faces)
    corners = torch.zeros_like(faces)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = abs(dz) + abs(dy) + abs(dx)
                if k == 0:
                    continue
                v = u[1 + dz:nz - 1 + dz, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]
                (faces if k == 1 else edges if k == 2 else corners).add_(v)
    out[1:-1, 1:-1, 1:-1] = c0 * u[1:-1, 1:-1, 1:-1] + c1 * faces + c2 * edges + c3 * corners
    return out


def box9(u: torch.Tensor, c0: float = 1.0 / 3.0, c1: float = 2.0 / 15.0, c2: float = 1.0 / 30.0) -> torch.Tensor:
    """2D 9-point; ``u`` is (h, 1, w) or (h, w)."""
    squeeze = u.dim() == 2
    g = u if squeeze else u[:, 0, :]
    out = g.clone()
    if min(g.shape) >= 3:
        edges = (g[1:-1, :-2] + g[1:-1, 2:]) + (g[:-2, 1:-1] + g[2:, 1:-1])
        corners = (g[:-2, :-2] + g[:-2, 2:]) + (g[2:, :-2] + g[2:, 2:])
        out[1:-1, 1:-1] = c0 * g[1:-1, 1:-1] + c1 * edges + c2 * corners
    return out if squeeze else out.unsqueeze(1)


def star7(u: torch.Tensor, c0: float = 0.30, wxm: float = 0.20, wxp: float = 0.20, wym: float = 0.10,
          wyp: float = 0.10, wzm: float = 0.05, wzp: float = 0.05) -> torch.Tensor:
    """3D 7-point star with seven weights; ``u`` is (nz, ny, nx). wxm multiplies u(x-1), wxp u(x+1)."""
    out = u.clone()
    if min(u.shape) < 3:
        return out
    out[1:-1, 1:-1, 1:-1] = (c0 * u[1:-1, 1:-1, 1:-1] + wxm * u[1:-1, 1:-1, :-2] + wxp * u[1:-1, 1:-1, 2:]
                             + wym * u[1:-1, :-2, 1:-1] + wyp * u[1:-1, 2:, 1:-1]
                             + wzm * u[:-2, 1:-1, 1:-1] + wzp * u[2:, 1:-1, 1:-1])
    return out


def conv9(u: torch.Tensor, w9=(0.06, 0.10, 0.02, 0.14, 0.36, 0.14, 0.02, 0.10, 0.06)) -> torch.Tensor:
    """2D 9-point stencil with nine weights, row-major: ``w9[3*(dz+1) + (dx+1)]`` multiplies u(z+dz, x+dx);
    ``u`` is (h, 1, w) or (h, w), edges held."""
    squeeze = u.dim() == 2
    v = u if squeeze else u[:, 0, :]
    out = v.clone()
    h, w = v.shape
    if h >= 3 and w >= 3:
        acc = torch.zeros_like(v[1:-1, 1:-1])
        for dz in (-1, 0, 1):
            for dx in (-1, 0, 1):
                acc = acc + w9[3 * (dz + 1) + (dx + 1)] * v[1 + dz:h - 1 + dz, 1 + dx:w - 1 + dx]
        out[1:-1, 1:-1] = acc
    return out if squeeze else out.unsqueeze(1)


def star13(u: torch.Tensor, c0: float = 0.25, c1: float = 2.0 / 15.0, c2: float = -1.0 / 120.0) -> torch.Tensor:
    """3D radius-2 star (fourth-order Laplacian points); ``u`` is (nz, ny, nx), any dtype. Cells within 2 of
    a face are held."""
    out = u.clone()
    if min(u.shape) < 5:
        return out
    c = u[2:-2, 2:-2, 2:-2]
    near = (u[2:-2, 2:-2, 1:-3] + u[2:-2, 2:-2, 3:-1] + u[2:-2, 1:-3, 2:-2] + u[2:-2, 3:-1, 2:-2]
            + u[1:-3, 2:-2, 2:-2] + u[3:-1, 2:-2, 2:-2])
    far = (u[2:-2, 2:-2, :-4] + u[2:-2, 2:-2, 4:] + u[2:-2, :-4, 2:-2] + u[2:-2, 4:, 2:-2]
           + u[:-4, 2:-2, 2:-2] + u[4:, 2:-2, 2:-2])
    out[2:-2, 2:-2, 2:-2] = c0 * c + c1 * near + c2 * far
    return out


def life(u: torch.Tensor, rule: str = "B3/S23") -> torch.Tensor:
    """Game of Life with a held frame, Conway's B3/S23, any Life-like ``rule`` or a Generations rule
    B/S/C with C cell states (0 dead, 1 alive, 2 .. C-1 dying); ``u`` is (h, 1, w) or (h, w) uint8.
    Integer arithmetic: the count of neighbours in state 1, a lookup in the rule's two 9-bit masks, and
    for the cells that advance (a live cell that does not survive, a dying cell) (s + 1) % C."""
    from ..models import native_rule, native_states

    birth, survive = native_rule(rule)
    states = native_states(rule)
    squeeze = u.dim() == 2
    g = (u if squeeze else u[:, 0, :]).to(torch.int32)
    out = g.clone()
    if min(g.shape) >= 3:
        h, w = g.shape
        one = (g == 1).to(torch.int32)
        n = torch.zeros_like(g[1:-1, 1:-1])
        for dz in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dz == 0 and dx == 0:
                    continue
                n += one[1 + dz:h - 1 + dz, 1 + dx:w - 1 + dx]
        s = g[1:-1, 1:-1]
        table = torch.where(s == 1, torch.full_like(n, survive), torch.full_like(n, birth))
        stays = ((table >> n) & 1) == 1  # born, or survives
        out[1:-1, 1:-1] = torch.where((s <= 1) & stays, torch.ones_like(s),
                                      torch.where(s == 0, s, (s + 1) % states))
    out = out.to(torch.uint8)
    return out if squeeze else out.unsqueeze(1)


def step(kind: str, u: torch.Tensor, **coef) -> torch.Tensor:
    if kind == "heat7":
        r = coef.get("r", -1.0)
        return heat7(u, 1.0 / 6.0 if r is None or r < 0 else r)
    if kind == "jacobi5":
        r = coef.get("r", -1.0)
        return jacobi5(u, 0.25 if r is None or r < 0 else r)
    if kind == "box27":
        return box27(u, coef.get("c0", 0.25), coef.get("c1", 0.05), coef.get("c2", 0.025),
                     coef.get("c3", 3.0 / 160.0))
    if kind == "box9":
        return box9(u, coef.get("c0", 1.0 / 3.0), coef.get("c1", 2.0 / 15.0), coef.get("c2", 1.0 / 30.0))
    if kind == "star7":
        return star7(u, coef.get("c0", 0.30), coef.get("wxm", 0.20), coef.get("wxp", 0.20), coef.get("wym", 0.10),
                     coef.get("wyp", 0.10), coef.get("wzm", 0.05), coef.get("wzp", 0.05))
    if kind == "conv9":
        return conv9(u, **({"w9": coef["w9"]} if "w9" in coef else {}))
    if kind == "star13":
        return star13(u, coef.get("c0", 0.25), coef.get("c1", 2.0 / 15.0), coef.get("c2", -1.0 / 120.0))
    if kind == "life":
        return life(u, coef.get("rule", "B3/S23"))
    raise ValueError(kind)


def run(kind: str, u: torch.Tensor, steps: int, **coef) -> torch.Tensor:
    for _ in range(steps):
        u = step(kind, u, **coef)
    return u


def residual(u_old: torch.Tensor, u_new: torch.Tensor) -> float:
    d = u_new.to(torch.float64) - u_old.to(torch.float64)
    return float(torch.sqrt((d * d).sum()))
