"""The device dispatcher's choice of kernel (host-side policy, no GPU): hip_kernel_name names the kernel
family a one-region launch runs, and hip_supports_steps is "that name is not empty".

The expected names of TABLE were written down from the launch chain of hip_stencil as it stood before
the choice moved into one function (one `if` arm per kernel), not from what hip_kernel_name returns.
"""

import itertools

import pytest

import mpi_cuda_process_amd as m

RADIUS = {"star13": 2}
KINDS_3D = ("heat7", "box27", "star7", "star13")
CONWAY, HIGHLIFE, GEN4, GEN33 = "B3/S23", "B36/S23", "B2/S345/C4", "B2/S/C33"


def row(kind, dtype, nx, steps, want, *, rule=CONWAY, ref=False, r=-1.0, knob=None, variant="auto", halo=None):
    ny = 9 if kind in KINDS_3D else 1
    label = "%s-%s-nx%d-K%d" % (kind, dtype, nx, steps)
    for extra in (rule if kind == "life" else "", "ref" if ref else "", "r%g" % r if r >= 0 else "",
                  "%s=%s" % knob if knob else "", variant if variant != "auto" else "",
                  "halo%d" % halo if halo is not None else ""):
        if extra:
            label += "-" + extra
    return pytest.param(kind, dtype, rule, ref, r, nx, ny, 12, steps, halo, knob, variant, want, id=label)


H7_OFF, H7_ON = ("MDFX_H7_WXK", 0), ("MDFX_H7_WXK", 1)
TABLE = [
    # single steps: the tuned one-pass kernels, or every stencil's one-cell-per-lane kernel
    row("heat7", "f32", 256, 1, "heat7_zw"),
    row("heat7", "f32", 256, 1, "naive", variant="naive"),
    row("heat7", "f64", 256, 1, "heat7_zw", variant="tuned"),
    row("life", "u8", 256, 1, "naive", variant="naive"),
    # heat7 K = 2: heat7_tbk while the padded row fits one block (1024 fp32 / 512 fp64 cells), else heat7_tb2
    row("heat7", "f32", 1024, 2, "heat7_tbk"),
    row("heat7", "f32", 1025, 2, "heat7_tb2"),
    row("heat7", "f64", 512, 2, "heat7_tbk"),
    row("heat7", "f64", 1024, 2, "heat7_tb2"),
    # heat7 K = 3: fp32 always heat7_wxk; fp64 heat7_wtk below 2048-cell rows unless MDFX_H7_WXK says otherwise
    row("heat7", "f32", 1024, 3, "heat7_wxk"),
    row("heat7", "f32", 1024, 3, "heat7_wxk", knob=H7_OFF),
    row("heat7", "f64", 1024, 3, "heat7_wtk"),
    row("heat7", "f64", 2048, 3, "heat7_wxk"),
    row("heat7", "f64", 1024, 3, "heat7_wtk", knob=H7_OFF),
    row("heat7", "f64", 2048, 3, "heat7_wtk", knob=H7_OFF),
    row("heat7", "f64", 1024, 3, "heat7_wxk", knob=H7_ON),
    row("heat7", "f64", 2048, 3, "heat7_wxk", knob=H7_ON),
    # K = 4: fp64 runs heat7_wxk at every width by default; K = 5: heat7_wxk only, whatever the knob
    row("heat7", "f64", 1024, 4, "heat7_wxk"),
    row("heat7", "f64", 1024, 4, "heat7_wtk", knob=H7_OFF),
    row("heat7", "f32", 1024, 5, "heat7_wxk"),
    row("heat7", "f64", 1024, 5, "heat7_wxk"),
    row("heat7", "f64", 1024, 5, "heat7_wxk", knob=H7_OFF),
    row("heat7", "f32", 1024, 6, ""),
    row("heat7", "f32", 1024, 3, "", halo=2),
    # box27: K = 2 keeps the row within one block, K = 3 takes any row
    row("box27", "f32", 256, 1, "box27_zw"),
    row("box27", "f32", 1024, 2, "box27_tb2"),
    row("box27", "f64", 512, 2, "box27_tb2"),
    row("box27", "f32", 1025, 2, ""),
    row("box27", "f32", 2048, 3, "box27_wxk"),
    row("box27", "f64", 256, 3, "box27_wxk"),
    row("box27", "f32", 256, 4, ""),
    # jacobi5: K = 2 through jacobi5_tb2 unless ref_precision can change a bit (fp32, r no power of two)
    row("jacobi5", "f32", 300, 1, "jacobi5_wave"),
    row("jacobi5", "f32", 300, 2, "jacobi5_tb2"),
    row("jacobi5", "f32", 300, 2, "jacobi5_tb2", ref=True),
    row("jacobi5", "f32", 300, 2, "jacobi5_tbk", ref=True, r=0.2),
    row("jacobi5", "f64", 300, 2, "jacobi5_tb2", ref=True, r=0.2),
    row("jacobi5", "f64", 300, 3, "jacobi5_tbk"),
    row("jacobi5", "f32", 300, 8, "jacobi5_tbk"),
    row("jacobi5", "f32", 300, 5, ""),
    # one launcher per family for every depth
    row("box9", "f32", 300, 1, "box9_tbk"),
    row("box9", "f64", 300, 8, "box9_tbk"),
    row("box9", "f32", 300, 5, ""),
    row("conv9", "f64", 300, 1, "conv9_tbk"),
    row("conv9", "f32", 300, 6, "conv9_tbk"),
    row("star7", "f32", 300, 1, "star7_tbk"),
    row("star7", "f64", 300, 4, "star7_tbk"),
    row("star7", "f32", 300, 5, ""),
    row("star13", "f32", 300, 1, "star13_tbk", halo=2),
    row("star13", "f64", 300, 2, "star13_tbk"),
    row("star13", "f32", 300, 3, ""),
    # life: Conway's own kernels, any other two-state rule, Generations rules of up to 32 states
    row("life", "u8", 300, 1, "life_wave"),
    row("life", "u8", 300, 2, "life_tb2"),
    row("life", "u8", 300, 3, "life_bits"),
    row("life", "u8", 300, 16, "life_bits"),
    row("life", "u8", 300, 5, ""),
    row("life", "u8", 300, 1, "life_rule_bits", rule=HIGHLIFE),
    row("life", "u8", 300, 2, "life_rule_bits", rule=HIGHLIFE),
    row("life", "u8", 300, 3, "life_rule_bits", rule=HIGHLIFE),
    row("life", "u8", 300, 12, "life_rule_bits", rule=HIGHLIFE),
    row("life", "u8", 300, 1, "life_gen_bits", rule=GEN4),
    row("life", "u8", 300, 2, "life_gen_bits", rule=GEN4),
    row("life", "u8", 300, 3, "life_gen_bits", rule=GEN4),
    row("life", "u8", 300, 12, "", rule=GEN4),
    row("life", "u8", 300, 1, "naive", rule=GEN33),
    row("life", "u8", 300, 2, "", rule=GEN33),
]

EVERY_KERNEL = {"naive", "heat7_zw", "heat7_tb2", "heat7_tbk", "heat7_wtk", "heat7_wxk", "box27_zw", "box27_tb2",
                "box27_wxk", "jacobi5_wave", "jacobi5_tb2", "jacobi5_tbk", "box9_tbk", "conv9_tbk", "star7_tbk",
                "star13_tbk", "life_wave", "life_tb2", "life_bits", "life_rule_bits", "life_gen_bits", ""}


def test_table_names_every_kernel():
    assert {p.values[-1] for p in TABLE} == EVERY_KERNEL


@pytest.mark.parametrize("kind,dtype,rule,ref,r,nx,ny,nz,steps,halo,knobset,variant,want", TABLE)
def test_kernel_name(mdfx, knob, kind, dtype, rule, ref, r, nx, ny, nz, steps, halo, knobset, variant, want):
    n = mdfx.native()
    if halo is None:
        halo = RADIUS.get(kind, 1) * steps
    if knobset:
        knob(*knobset)
    n.set_kernel_variant(variant)
    try:
        assert n.hip_kernel_name(kind, dtype, nx, ny, nz, halo, steps, ref, rule, r=r) == want
        if r < 0:
            assert n.hip_supports_steps(kind, dtype, nx, ny, nz, halo, steps, ref, rule) == (want != "")
    finally:
        n.set_kernel_variant("auto")


SPECS = [(kind, dtype, False, CONWAY) for kind in ("heat7", "box27", "star7", "star13", "jacobi5", "box9", "conv9")
         for dtype in ("f32", "f64")]
SPECS += [("jacobi5", "f32", True, CONWAY)] + [("life", "u8", False, rule) for rule in (CONWAY, HIGHLIFE, GEN4, GEN33)]
NX = (64, 70, 256, 257, 300, 512, 513, 768, 1024, 1025, 1030, 2047, 2048, 2050, 4096)


@pytest.mark.parametrize("h7,b27", list(itertools.product((None, 0, 1), repeat=2)))
def test_supported_is_a_named_kernel(mdfx, knob, h7, b27):
    """hip_supports_steps is hip_kernel_name != "" for every stencil, dtype, rule, row width, grid depth,
    sweep depth 1 .. 17, a halo that covers the sweep and one plane less, under every knob setting."""
    n = mdfx.native()
    for name, v in (("MDFX_H7_WXK", h7), ("MDFX_B27_WXK", b27)):
        if v is not None:
            knob(name, v)
    named = 0
    for kind, dtype, ref, rule in SPECS:
        for nx, ny, nz, steps in itertools.product(NX, (5, 9) if kind in KINDS_3D else (1,), (5, 12, 45), range(1, 18)):
            full = RADIUS.get(kind, 1) * steps
            for halo in (full, full - 1):
                if halo < 1:  # (no such layout)
                    continue
                name = n.hip_kernel_name(kind, dtype, nx, ny, nz, halo, steps, ref, rule)
                assert n.hip_supports_steps(kind, dtype, nx, ny, nz, halo, steps, ref, rule) == (name != ""), (
                    kind, dtype, ref, rule, nx, ny, nz, steps, halo)
                assert name in EVERY_KERNEL
                named += name != ""
    assert named > 0
