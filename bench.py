#!/usr/bin/env python3
"""Headline benchmark: GCells/s of the 3D 7-point Jacobi stencil on a 1024^3 fp32 grid,
slab-decomposed over N MI355X GPUs (one process per GPU, device-resident halo exchange over xGMI).

    python bench.py                              # N = 1
    python bench.py --gpus 8                     # launches 8 worker processes itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run (no --full) does only what the headline figure needs: it builds the engine in its
default configuration (z slabs, the transport's default schedule, hipGraph replay in one process and
eager launches across processes), runs W warm-up steps and, on a GPU, untimed settling passes of K
steps each until at least 100 steps have run ("settle_steps" in the JSON: the device's first steps
on a fresh grid are 2 - 4 % slower than its steady state, which the median repetition of --full
reports), times exactly K steps once, writes its outputs if --dump-outputs is given and prints the
JSON line. Everything else described below (the N > 1 correctness gate, the timed trials that pick
transport / graph mode / rounds / overlap / pencils, the three timed repetitions, the verification
of the timed run against the naive kernels, the N > 1 diagnostic pass and the measured copy
yardstick) runs only with --full; the JSON fields they fill are null without it.

--dump-outputs DIR writes, after the timed steps, the field the timed engine holds after its last
timed step (step W + settle_steps + K of a plain run) as DIR/field.npy (float32; float64 for
--dtype f64): the whole grid (nz, ny, nx) in C order when it has at most 4 Mi cells, else its values
at 4 Mi cell indices drawn once from a fixed seed (numpy default_rng(1).integers(0, cells, 4 Mi),
sorted; flat index = (z * ny + y) * nx + x), so two builds run with the same arguments write
comparable arrays. With --residual-every the last
residual is written as DIR/residual.npy (float64).

Launch. Under a launcher (RANK / WORLD_SIZE set) this process is one rank and WORLD_SIZE must equal
--gpus. Without one, --gpus N > 1 spawns N child processes of this script with the launcher
variables set (before this process touches the GPU) and exits with the worst child status; N
larger than the visible GPU count is an error, never a silent 1-GPU run.

Correctness gate (N > 1). Before timing, every rank runs a small decomposed problem of the same
stencil (256 x 256 x 64N, 6 fused sweeps, residual included) through the SAME transport, and
compares its owned planes bitwise against a full-grid single-slab run on its own GPU. Any mismatch
on any rank aborts the run non-zero. With --transport auto every device transport (rccl, ipc) is
gated, the ones that pass get short timed trials and the fastest is timed; the JSON names it. If
neither passes, the host-staged transport (faces through host memory over gloo) is gated as a
last resort, so a node whose xGMI paths fail still yields a correct (slow, labelled) number.

The grid is fixed as N grows (strong scaling, the BASELINE.json config "3D 7-pt Jacobi 1024^3 fp32
slab-decomposed across 8xMI355X"). Data is synthetic: a uniform random initial grid generated on
the device from a counter-based hash of the global cell index (seed 1). Every timed step is a full
Jacobi update of every cell (boundary planes + halo exchange + interior), nothing is skipped or
cached. By default five consecutive Jacobi steps are fused into one pass over memory (temporal
blocking, --temporal 5 through heat7_wxk in rows of 2 cells per lane at 1024-cell rows; bitwise
identical to five single steps, tests/test_gpu_temporal.py): every step is still computed in full,
the fused kernel keeps u^{t+1}..u^{t+4} on chip. A step count that is not a multiple of 5 ends with
a shorter fused sweep.
--temporal 1 measures one sweep per step. Timing: W untimed warmup steps, then exactly K steps bracketed by barrier +
torch.cuda.synchronize() on both sides; the slowest rank's time is reported (--full: three such
repetitions by default, the median reported and all three listed). GCells/s = nx*ny*nz*K / t / 1e9
for the whole job.

Verification of the timed run itself. After timing, every rank re-runs the exact step sequence of
the timed engine (init, warm-up, every timed repetition) on the FULL grid as one slab on its own
device with the naive single-step kernels, and compares its owned cells bitwise; the verdict is
all-reduced into the JSON ("verified"), and any difference exits non-zero without a number. So the
reported run, not only the small gate, is checked against an independent computation (N = 1
included: the fused heat7_wxk sweeps against naive single steps on the whole 1024^3 grid).

Rank 0 prints one JSON line. The DRAM fields report the
traffic actually required per time step (one read + one write of every cell per fused sweep, i.e.
divided by the temporal depth) against the 6.29 TB/s copy roof of MI355X_MICROARCH.md
(pct_of_hbm_copy_roof) and against torch's copy_ of one GPU's share of the field timed in the same
process after the timed region (measured_copy_TBps, pct_of_measured_copy: a K-step sweep moves
exactly a copy's bytes per K steps, so 100 % is the achievable-bandwidth bound of the layout).
"""

from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

_T_START = time.time()  # (the JSON's wall_s: the whole process, torch import included)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# hipGraph replay on one hardware queue (set before anything starts the HIP runtime; see
# mpi_cuda_process_amd/__init__.py)
os.environ.setdefault("DEBUG_HIP_FORCE_GRAPH_QUEUES", "1")

import torch  # noqa: E402  (importing torch does not initialise the GPU)

METRIC = "GCells/s (whole node), 3D 7-pt Jacobi 1024^3 fp32 at 1/2/4/8 MI355X"
HBM_MEASURED_TBPS = 6.29  # float4 copy, MI355X_MICROARCH.md (8.0 spec)
LAUNCH_VARS = ("RANK", "WORLD_SIZE", "OMPI_COMM_WORLD_RANK", "PMI_RANK")


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--gpus", type=int, default=1, help="ranks (one process and one GPU each)")
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--n", type=int, default=1024, help="cube edge (default 1024)")
    p.add_argument("--nx", type=int, default=0)
    p.add_argument("--ny", type=int, default=0)
    p.add_argument("--nz", type=int, default=0)
    p.add_argument("--stencil", default="heat7", choices=["heat7", "box27", "jacobi5", "life"])
    p.add_argument("--dtype", default="f32", choices=["f32", "f64", "u8"])
    p.add_argument("--transport", default="auto",
                   help="auto|rccl|ipc|ipc_sdma|torch|staged (distributed), loopback (1 process); with "
                        "--rank-proxy: ipc_sdma models the SDMA pulls (proxy_sdma)")
    p.add_argument("--virtual-ranks", type=int, default=0,
                   help="split the grid into P slabs inside ONE process (loopback transport)")
    p.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                   help="replay 2-sweep cycles as hipGraphs; auto = on in one process and off across processes, "
                        "with --full gate and time both and keep the faster")
    p.add_argument("--rounds", default="auto", choices=["auto", "1", "2"],
                   help="minimum rounds of resident blocks per fused sweep; auto = the engine's default (1 on one "
                        "GPU), with --full a timed trial of 1 and 2 with several ranks (2 leaves CUs for exchange "
                        "kernels mid-sweep)")
    p.add_argument("--trial-steps", type=int, default=48,
                   help="steps of each short timed trial that picks transport / graph mode / rounds / "
                        "overlap (auto); every candidate is timed twice, interleaved, and its faster run counts")
    p.add_argument("--temporal", type=int, default=0,
                   help="time steps fused per memory sweep (temporal blocking); 0 = auto (native "
                        "hip_fused_depth): 5 (fp32; fp64 from 2048-cell rows, else 4) for the 3D 7-point where heat7_wxk's x segments "
                        "cover the row, 3 for the 27-point at 1024-cell rows and in fp64, else 2; 8 (2D "
                        "MDF) / 12 (Life)")
    p.add_argument("--ref-precision", action="store_true",
                   help="jacobi5: the reference program's mixed fp32/fp64 update (MDF_kernel.cu:20)")
    p.add_argument("--no-overlap", action="store_true", help="one full sweep after the exchange (no trial)")
    p.add_argument("--overlap", action="store_true",
                   help="only the overlapped schedule (interior || boundary + exchange; no trial)")
    p.add_argument("--residual-every", type=int, default=0)
    p.add_argument("--py", type=int, default=0,
                   help="ranks along y of a (z, y) pencil decomposition (1 = z slabs; 0 = auto: z slabs, with --full "
                        "at 4+ GPUs the 3D 7-point tries slabs and 2-along-y pencils and times the faster)")
    p.add_argument("--variant", default="auto", choices=["auto", "tuned", "naive"])
    p.add_argument("--device", default="auto", choices=["auto", "hip", "cpu"])
    p.add_argument("--repeats", type=int, default=0,
                   help="timed repetitions of --steps steps each, back to back; the median is reported and "
                        "every one is listed (0 = auto: 1, or 3 with --full or --rank-proxy)")
    p.add_argument("--full", action="store_true",
                   help="also run everything beyond the headline figure: the N > 1 correctness gate, the timed "
                        "trials of transport / graph mode / rounds / overlap / pencils, three timed repetitions, "
                        "the verification of the timed run, the N > 1 diagnostic pass and the copy yardstick")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="after the timed steps write the field of the last timed step (a fixed seeded sample of "
                        "a large grid) as DIR/field.npy")
    p.add_argument("--trial-budget", type=float, default=150.0,
                   help="seconds the gate + trial phase may take before the second (interleaved) trial pass "
                        "is skipped (all ranks agree on the slowest rank's clock)")
    p.add_argument("--no-diagnose", action="store_true",
                   help="N > 1: skip the profiled pass after verification (per-rank phases, face pull rates)")
    p.add_argument("--no-verify", action="store_true",
                   help="skip the check of the timed run against a full-grid naive run on each rank's device")
    p.add_argument("--timeout", type=float, default=120.0,
                   help="watchdog (s): a rank whose streams make no progress for this long aborts the "
                        "transport and exits non-zero")
    p.add_argument("--gate-n", type=int, default=0, help="edge of the correctness-gate grid (0 = auto)")
    p.add_argument("--no-gate", action="store_true", help="skip the N > 1 correctness gate")
    p.add_argument("--verbose", action="store_true", help="per-rank phase trace on stderr")
    p.add_argument("--rank-proxy", type=int, default=0, metavar="N",
                   help="per-GPU proxy of an N-GPU run on ONE GPU: only rank --proxy-rank's slab of the N-way "
                        "split, its halo exchange looped back through the ipc mailbox copies and counters; "
                        "reports per-GPU GCells/s (a proxy, never the headline)")
    p.add_argument("--proxy-rank", type=int, default=-1,
                   help="which slab the proxy runs (default: a middle rank, two neighbours)")
    p.add_argument("--share-gpu", action="store_true",
                   help="allow more ranks than GPUs (processes share devices; tests of the ipc/staged paths "
                        "only: the ipc exchange's device spin waits assume one engine process per GPU and the "
                        "transport refuses shared GPUs without this)")
    a = p.parse_args(argv)
    if a.repeats <= 0:
        a.repeats = 3 if (a.full or a.rank_proxy > 0) else 1
    return a


_T0 = time.time()
_VERBOSE = False


def trace(msg):
    if _VERBOSE:
        print("[bench rank %s +%.2fs] %s" % (os.environ.get("RANK", "0"), time.time() - _T0, msg),
              file=sys.stderr, flush=True)


def launched() -> bool:
    return any(v in os.environ for v in LAUNCH_VARS)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(a, argv) -> int:
    """Spawn --gpus worker processes of this script (one per GPU) and wait for them."""
    n = a.gpus
    ndev = torch.cuda.device_count() if a.device != "cpu" else 0  # counts without initialising HIP
    if a.device == "hip" and ndev == 0:
        print("bench: --device hip but no GPU is visible", file=sys.stderr)
        return 2
    if ndev > 0 and n > ndev and not a.share_gpu:
        print("bench: --gpus %d but only %d GPU(s) are visible; refusing to run fewer GPUs than asked "
              "(--share-gpu lets ranks share devices)" % (n, ndev), file=sys.stderr)
        return 2
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    worst, first_fail = 0, None
    live = set(range(n))
    while live:
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is None:
                continue
            live.discard(r)
            if rc != 0:
                worst = worst or rc
                if first_fail is None:
                    first_fail = time.time()
        if first_fail is not None and live and time.time() - first_fail > 30:
            for r in live:  # peers of a failed rank block in collectives: end them
                procs[r].kill()
            for r in live:
                procs[r].wait()
            worst = worst or 1
            break
        time.sleep(0.05)
    if worst:
        print("bench: a rank exited with status %d" % worst, file=sys.stderr)
        return 1
    return 0


def make_problem(a, nx, ny, nz):
    from mpi_cuda_process_amd import box27, heat3d, life2d, mdf2d

    if a.stencil == "heat7":
        return heat3d(nx=nx, ny=ny, nz=nz, dtype=a.dtype)
    if a.stencil == "box27":
        return box27(nx=nx, ny=ny, nz=nz, dtype=a.dtype)
    if a.stencil == "jacobi5":
        return mdf2d(h=nz, w=nx, dtype=a.dtype, ref_precision=a.ref_precision)
    return life2d(h=nz, w=nx)


# the deepest fused sweep a (z, y) pencil layout has: heat7_wxk's pencil copies fuse 3 or 4 steps
# (the 5-step sweep in rows of 2 cells per lane is for z slabs)
PENCIL_MAX_DEPTH = 4


def depth_for_layout(temporal, py, hip):
    """Fused depth of a candidate with `py` ranks along y, given the slab depth `temporal`."""
    return min(temporal, PENCIL_MAX_DEPTH) if (hip and py > 1) else temporal


def pick_temporal(a, prob, nslab, hip):
    from mpi_cuda_process_amd import native

    if a.temporal > 0:
        return a.temporal
    # the deepest measured-win fused depth (native hip_fused_depth: 5 for the fp32 3D 7-point and for
    # fp64 rows of 2048+ cells, 4 for shorter fp64 rows, through heat7_wxk where its x segments cover
    # the row; 3 for the 27-point at 1024-cell rows and in fp64, else 2; 8 (MDF) / 12 (Life) for the
    # 2D ones; profiles/archive/r03_wxk/, r06_session_b/), made shallower until every slab is at
    # least 4 sweeps deep
    want = native().hip_fused_depth(prob.kind, prob.dtype, prob.nx, prob.ref_precision) if hip else \
        {"jacobi5": 8, "life": 12}.get(a.stencil, 2)
    while want > 1 and prob.nz < 4 * want * nslab:
        want = {5: 4, 3: 2}.get(want, want // 2)
    if want > 1 and (not hip or native().hip_supports_steps(prob.kind, prob.dtype, prob.nx, prob.ny, prob.nz,
                                                            want, want, prob.ref_precision)):
        if hip:  # (the depth for the residual interval, native interval_depth)
            return native().hip_auto_depth(prob.kind, prob.dtype, prob.nx, prob.ny, prob.nz, want,
                                           a.residual_every, prob.ref_precision, nslab)
        return want
    return 1


def run_gate(a, hip, transport, temporal, world, rank, graph=False, py=1):
    """Bitwise check of the decomposed engine (same transport, same fused depth, same graph mode)
    against a full-grid single-slab run on this rank's own device. Returns (passed, record)."""
    import numpy as np
    import torch.distributed as dist

    from mpi_cuda_process_amd import Simulation

    n = a.gate_n or (256 if hip else 32)
    per = max(64 if hip else 8, 4 * temporal)
    if a.stencil in ("jacobi5", "life"):
        prob = make_problem(a, n, 1, per * world)
    else:
        prob = make_problem(a, n, n, per * world)
    steps = 6 * temporal
    kw = dict(device="hip" if hip else "cpu", temporal=temporal, residual_every=steps,
              timeout_s=a.timeout if hip else 0.0)
    err = ""
    tag = transport + ("+graph" if graph else "") + ("+py%d" % py if py > 1 else "")
    ok = False
    try:
        fault = os.environ.get("MDFX_FAULT", "")
        if fault.startswith("gate:") and transport in fault[5:].split(","):
            # fault injection for the fallback test: this transport's gate fails on every rank
            raise RuntimeError("injected gate failure (MDFX_FAULT=%s)" % fault)
        with Simulation(prob, distributed=True, transport=transport, graph=graph, py=py, share_gpu=a.share_gpu,
                        **kw) as sim:
            trace("gate: engine up")
            sim.init()
            sim.prepare_graphs()  # the timed run's path: cycles captured before any step
            sim.run(steps)
            trace("gate: steps enqueued")
            sim.synchronize()
            trace("gate: steps done")
            mine = sim.read_local(0)
            res = sim.residual
            lay = sim.layout(0)
        with Simulation(prob, ranks=1, distributed=False, **kw) as ref:
            ref.init()
            ref.run(steps)
            ref.synchronize()
            full = ref.read_local(0)
            rres = ref.residual
        own = full[lay["z0"]:lay["z1"], lay["y0"]:lay["y1"]]
        ok = bool(np.array_equal(mine, own)) and abs(res - rres) <= 1e-9 * max(1.0, abs(rres))
        if not ok:
            err = "rank %d: owned planes or residual differ from the full-grid run (residual %r vs %r)" % (
                rank, res, rres)
    except Exception as e:  # noqa: BLE001 - reported and agreed on below
        err = "rank %d: %s: %s" % (rank, type(e).__name__, e)
    t = torch.tensor([0.0 if ok else 1.0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    bad = int(t.item())
    if err:
        print("bench gate [%s]: %s" % (tag, err), file=sys.stderr, flush=True)
    rec = {"grid": [prob.nx, prob.ny, prob.nz], "steps": steps, "transport": transport, "graph": graph, "py": py,
           "ranks_failed": bad, "passed": bad == 0}
    return bad == 0, rec


def _owned(sim, i, nx):
    """Owned cells of local part i as a zero-copy (nzl, nyl, nx) view of the current buffer."""
    lay = sim.layout(i)
    h, hy = lay["halo"], lay["hy"]
    return sim.view(i)[h:h + lay["nzl"], hy:hy + lay["nyl"], :nx]


def inject_timed_fault(sim, rank, world):
    """MDFX_FAULT=ghost@<r>:timed (tests): once the timed run's warm-up is done, rank r adds 1 to one
    cell of its lower ghost plane, as a broken or racy exchange would leave it. The gate and the
    trials ran clean before, so only the verification of the timed run can catch it."""
    f = os.environ.get("MDFX_FAULT", "")
    if not (f.startswith("ghost@") and f.endswith(":timed")):
        return False
    if int(f[6:-6]) != rank or rank == 0 or world < 2:
        return False
    sim.synchronize()
    lay = sim.layout(0)
    v = sim.view(0)
    v[lay["halo"] - 1, lay["hy"] + lay["nyl"] // 2, sim.problem.nx // 2] += 1
    if v.is_cuda:
        torch.cuda.synchronize()
    print("[bench rank %d] injected a ghost-plane fault into the timed run (MDFX_FAULT=%s)" % (rank, f),
          file=sys.stderr, flush=True)
    return True


def verify_timed(a, sim, prob, hip, env, rank, world, seq):
    """Check the timed run itself, not only the gate: rank r re-runs the exact step sequence of the
    timed engine (init, then run(n) for every n in `seq`) on the FULL grid as one slab on its own
    device with the naive single-step kernels (HIP) or the CPU oracle, and compares its owned cells
    bitwise (and the last residual, when one was evaluated). The verdict is all-reduced; returns the
    JSON record. The reference program never read its result back (MDF_kernel.cu:164,177)."""
    import torch.distributed as dist

    from mpi_cuda_process_amd import Simulation, native

    parts = [(sim.layout(i), _owned(sim, i, prob.nx)) for i in range(sim.num_local)]
    res_mine = sim.residual
    diff, err, oom = float("inf"), "", False
    if hip:
        # the reference holds two full-grid buffers next to this rank's own: skip (and say so) where
        # they do not fit the device, e.g. 3072^3 fp32 or 2048^3 fp64 on ONE GPU
        from mpi_cuda_process_amd.ops import FieldLayout

        # every rank on this device builds its own reference at once (--share-gpu: several per device)
        dev = torch.cuda.current_device()
        sharing = 1
        if env:
            devs = [None] * world
            dist.all_gather_object(devs, (socket.gethostname(), dev))
            sharing = sum(1 for d in devs if d == (socket.gethostname(), dev))
        need = sharing * (2 * FieldLayout.make(prob, halo=1).nbytes + (1 << 30))
        free = torch.cuda.mem_get_info()[0]
        ok = torch.tensor([1.0 if free >= need else 0.0], dtype=torch.float64)
        if env:
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if ok.item() == 0.0:
            return {"ranks": world, "passed": True, "skipped": "the full-grid reference needs %.0f GB per device "
                    "(%d rank(s) on it), %.0f GB free on rank %d" % (need / 1e9, sharing, free / 1e9, rank)}
    if hip:
        native().set_kernel_variant("naive")
    try:
        kw = dict(device="hip" if hip else "cpu", temporal=1, residual_every=a.residual_every,
                  timeout_s=a.timeout if hip else 0.0)
        with Simulation(prob, ranks=1, distributed=False, **kw) as ref:
            ref.init()
            for n in seq:
                ref.run(n)
            ref.synchronize()
            rl = ref.layout(0)
            diff = 0.0
            for lay, mine in parts:
                full = ref.view(0)[rl["halo"] + lay["z0"]:rl["halo"] + lay["z1"], lay["y0"]:lay["y1"], :prob.nx]
                if not torch.equal(mine, full):
                    d = (mine.double() - full.double()).abs()
                    diff = max(diff, float(d.nan_to_num(nan=float("inf")).max()))
            if res_mine >= 0 and abs(res_mine - ref.residual) > 1e-9 * max(1.0, abs(ref.residual)):
                err = "residual %r vs %r" % (res_mine, ref.residual)
    except torch.OutOfMemoryError as e:  # a resource limit, not a mismatch: reported as skipped below
        err, oom = "%s: %s" % (type(e).__name__, e), True
    except Exception as e:  # noqa: BLE001 - reported and agreed on below
        err = "%s: %s" % (type(e).__name__, e)
        oom = "out of memory" in str(e).lower() or "hipErrorOutOfMemory" in str(e)
    finally:
        if hip:
            native().set_kernel_variant(a.variant)
    t = torch.tensor([1.0 if (err and oom) else 0.0], dtype=torch.float64)
    if env:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if t.item() > 0:
        if err and oom:
            print("bench verify: rank %d could not allocate the full-grid reference: %s" % (rank, err),
                  file=sys.stderr, flush=True)
        return {"ranks": world, "passed": True, "skipped": "a rank could not allocate the full-grid reference "
                "(out of memory)"}
    if err or diff != 0.0:
        print("bench verify: rank %d: owned cells differ from the full-grid run by up to %g %s" % (rank, diff, err),
              file=sys.stderr, flush=True)
    t = torch.tensor([diff if not err else float("inf"), 1.0 if (err or diff != 0.0) else 0.0], dtype=torch.float64)
    if env:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return {"ranks": world, "max_abs_diff": float(t[0].item()), "passed": t[1].item() == 0.0,
            "steps": [int(n) for n in seq],
            "reference": "full grid, one slab on each rank's own device, %s" % (
                "naive single-step HIP kernels" if hip else "CPU oracle")}


def diagnose(sim, temporal, env, world, rank, sweeps=4):
    """N > 1, after the timed run and its verification (outside the timed region): where a rank's
    time per sweep goes, and what its halo links deliver. Every rank runs `sweeps` profiled sweeps
    (Solver phase timing: hipEvents on the boundary / compute / halo streams, one host sync per
    sweep) and then times exchange_ghosts() alone (the current faces re-sent: the ghosts do not
    change) five times. Returns (phases, links), one entry per rank, gathered on every rank.

    phases (us per sweep): boundary = the boundary launch(es) before the interior sweep; interior =
    the interior sweep (with the folded lower boundary when folded); exchange = from the end of the
    boundary launch to the end of the exchange on the halo stream; exposed = how long the exchange
    ran on after the sweep's last kernel ended (the part not hidden); step = the whole sweep.
    links: the faces this rank pulls (peer rank, bytes), the best host-timed exchange of all of
    them at once (an upper bound: it includes one host synchronisation), and bytes / time per face."""
    import torch.distributed as dist

    nat = sim.native
    rec_p, rec_l = {"rank": rank}, {"rank": rank}
    try:
        sim.set_options(profile=True)
        nat.reset_phases()
        sim.run(sweeps * temporal)
        sim.synchronize()
        ph = nat.phase_times()
        sim.set_options(profile=False)
        n = max(1, int(ph["sweeps"]))
        rec_p.update({k + "_us": round(ph[k + "_ms"] / n * 1e3, 1)
                      for k in ("boundary", "interior", "exchange", "exposed", "step")})
        rec_p["sweeps"] = n
        faces = [sp for sp in nat.halo_spans(0, nat.current_index) if sp["peer"] >= 0]
        ts = []
        for _ in range(5):
            if env:
                dist.barrier()
            t0 = time.perf_counter()
            nat.exchange_ghosts()
            ts.append(time.perf_counter() - t0)
        best = min(ts)
        rec_l.update({"peers": [int(sp["peer"]) for sp in faces], "face_bytes": [int(sp["bytes"]) for sp in faces],
                      "exchange_us": round(best * 1e6, 1),
                      "GBps_per_face": round(max([sp["bytes"] for sp in faces] or [0]) / best / 1e9, 2)})
    except Exception as e:  # noqa: BLE001 - a diagnostic never fails the run
        rec_p["error"] = rec_l["error"] = "%s: %s" % (type(e).__name__, e)
    allp, alll = [rec_p], [rec_l]
    if env:
        allp, alll = [None] * world, [None] * world
        dist.all_gather_object(allp, rec_p)
        dist.all_gather_object(alll, rec_l)
    return allp, alll


def measure_copy_tbps(field_bytes):
    """torch's device copy_ of one field into another of `field_bytes` (the bytes a fused sweep moves:
    one read and one write of every cell), best of 3 after a warm-up, in TB/s. The achievable-copy
    yardstick the JSON's pct_of_measured_copy is taken against (run after the timed region)."""
    import torch

    n = max(1, int(field_bytes) // 16)
    try:
        src = torch.empty(n, 4, dtype=torch.float32, device="cuda")
        dst = torch.empty_like(src)
    except RuntimeError:
        return None
    src.fill_(1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for i in range(4):
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 1e3
        if i > 0:
            best = t if best is None else min(best, t)
    del src, dst
    torch.cuda.empty_cache()
    return 2.0 * n * 16 / best / 1e12


# a GPU's first steps on a fresh grid run 2 - 4 % slower than the steady state it reaches within
# about a hundred steps (1024^3 fp32: the repetitions of --full fall from 0.415 to 0.395 ms per step)
SETTLE_MIN_STEPS = 100
DUMP_MAX_CELLS = 4 << 20  # cells written by --dump-outputs (16 MiB of fp32, 32 MiB of fp64)
DUMP_SEED = 1


def dump_outputs(a, sim, prob, env, world, rank):
    """--dump-outputs: the field after the last timed step as <dir>/field.npy on rank 0 (the whole
    grid up to DUMP_MAX_CELLS cells, else its values at a fixed seeded sample of cell indices), and
    the last residual as <dir>/residual.npy when one was evaluated. Every rank reads its own owned
    cells from its current buffer; nothing is recomputed."""
    import numpy as np
    import torch.distributed as dist

    nx, ny, nz = prob.nx, prob.ny, prob.nz
    cells = nx * ny * nz
    if cells <= DUMP_MAX_CELLS:
        idx, shape = np.arange(cells, dtype=np.int64), (nz, ny, nx)
    else:
        idx = np.sort(np.random.default_rng(DUMP_SEED).integers(0, cells, DUMP_MAX_CELLS, dtype=np.int64))
        shape = (DUMP_MAX_CELLS,)
    z, y, x = idx // (ny * nx), (idx // nx) % ny, idx % nx
    sim.synchronize()
    pieces = []
    for i in range(sim.num_local):
        lay = sim.layout(i)
        own = _owned(sim, i, nx)
        sel = np.nonzero((z >= lay["z0"]) & (z < lay["z1"]) & (y >= lay["y0"]) & (y < lay["y1"]))[0]
        at = [torch.as_tensor(c[sel] - o, device=own.device) for c, o in ((z, lay["z0"]), (y, lay["y0"]), (x, 0))]
        pieces.append((sel, own[at[0], at[1], at[2]].cpu().numpy()))
    if env:
        allp = [None] * world
        dist.all_gather_object(allp, pieces)
        pieces = [p for ps in allp for p in ps]
    if rank != 0:
        return
    out = np.full(len(idx), np.nan, dtype=np.float64 if a.dtype == "f64" else np.float32)
    for sel, vals in pieces:
        out[sel] = vals
    os.makedirs(a.dump_outputs, exist_ok=True)
    np.save(os.path.join(a.dump_outputs, "field.npy"), out.reshape(shape))
    if sim.residual >= 0 and a.residual_every > 0:
        np.save(os.path.join(a.dump_outputs, "residual.npy"), np.array([sim.residual], dtype=np.float64))


def run_proxy(a):
    """--rank-proxy N: time exactly one rank's per-step work of an N-GPU strong-scaling run on one
    GPU (its slab plus K ghost planes per side, both boundary regions on the halo stream, the
    interior on the compute stream, the ipc exchange sequence looped back onto itself). Prints one
    JSON line labelled as a proxy: per-GPU GCells/s of that slab and the implied N-GPU figure."""
    from mpi_cuda_process_amd import Simulation, native

    if not torch.cuda.is_available():
        print("bench: --rank-proxy needs a HIP device", file=sys.stderr)
        return 2
    if a.dump_outputs:
        print("bench: --dump-outputs is not available with --rank-proxy", file=sys.stderr)
        return 2
    n = a.rank_proxy
    r = a.proxy_rank if a.proxy_rank >= 0 else (n // 2 if n > 1 else 0)
    torch.cuda.set_device(0)
    native().set_kernel_variant(a.variant)
    nx, ny, nz = a.nx or a.n, a.ny or a.n, a.nz or a.n
    if a.stencil in ("jacobi5", "life"):
        ny = 1
    prob = make_problem(a, nx, ny, nz)
    py = max(1, a.py)
    temporal = pick_temporal(a, prob, max(1, n // py), True)
    if py > 1:
        temporal = depth_for_layout(temporal, py, True)
    graphs = {"on": [True], "off": [False]}.get(a.graph, [False, True])
    overlaps = [True, False] if (n > 1 and not a.no_overlap and not a.overlap) else [not a.no_overlap]
    rounds = [int(a.rounds)] if a.rounds != "auto" else ([2, 1] if n > 1 else [0])
    sdma = a.transport in ("ipc_sdma", "proxy_sdma")
    sim = Simulation(prob, device="hip", ranks=n, proxy_rank=r, temporal=temporal, graph=graphs[0],
                     residual_every=a.residual_every, timeout_s=a.timeout,
                     transport="proxy_sdma" if sdma else "proxy", py=py)
    lay = sim.layout(0)
    slab_cells = (lay["z1"] - lay["z0"]) * (lay["y1"] - lay["y0"]) * prob.nx

    def timed(steps):
        sim.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.run(steps)
        sim.synchronize()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    trials = []
    cands = [(g, rr, ov) for g in graphs for rr in rounds for ov in overlaps]
    chosen = cands[0]
    if len(cands) > 1:
        n_trial = max(2, a.trial_steps)
        best_t = {}
        for _pass in range(2):
            for c in cands:
                g, rr, ov = c
                sim.set_options(graph=g, min_rounds=rr, overlap=ov)
                sim.init()
                sim.prepare_graphs()
                sim.run(a.warmup)  # the timed run's own warm-up: same buffer parity and replay state
                best_t[c] = min(best_t.get(c, 1e30), timed(n_trial) / n_trial * 1e3)
        for g, rr, ov in cands:
            trials.append({"graph": g, "min_rounds": rr, "overlap": ov, "ms_per_step": round(best_t[(g, rr, ov)], 4)})
        chosen = cands[min(range(len(trials)), key=lambda i: trials[i]["ms_per_step"])]
    sim.set_options(graph=chosen[0], min_rounds=chosen[1], overlap=chosen[2])
    sim.init()
    sim.prepare_graphs()
    sim.run(a.warmup)
    timed(0)
    replays0, captures0 = sim.graph_replays, sim.graph_captures
    dts = [timed(a.steps) for _ in range(max(1, a.repeats))]
    best = statistics.median(dts)  # (the median repetition, as the whole-node bench reports)
    per_gpu = slab_cells * a.steps / best / 1e9
    timed_vs_trial = (round(best / a.steps * 1e3 / min(t["ms_per_step"] for t in trials), 3) if trials else None)
    model = {"heat7": "3D 7-pt Jacobi", "box27": "3D 27-pt", "jacobi5": "2D 5-pt MDF", "life": "2D Game of Life"}[a.stencil]
    dram_tbps = per_gpu * prob.bytes_per_cell_per_step / temporal / 1e3
    rec = {
        "metric": "PROXY per-GPU GCells/s, rank %d of a %d-GPU %s split, %s %dx%dx%d %s (one GPU; not a "
                  "whole-node measurement)" % (r, n, "slab" if py == 1 else "%dx%d (z, y) pencil" % (n // py, py),
                                               model, nx, ny, nz, a.dtype),
        "value": round(per_gpu, 3),
        "unit": "GCells/s per GPU",
        "proxy": True,
        "n_gpus": 1,
        "proxied_n_gpus": n,
        "proxy_rank": r,
        "implied_node_gcells": round(per_gpu * n, 3),
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(best / a.steps * 1e3, 4),
        "higher_is_better": True,
        "dtype": {"f32": "fp32", "f64": "fp64", "u8": "u8"}[a.dtype],
        "data": "synthetic (uniform random grid from a counter hash of the global index, seed 1)",
        "config": {"model": "%s %dx%dx%d %s" % (model, nx, ny, nz, a.dtype), "slab_planes": [lay["z0"], lay["z1"]],
                   "rows": [lay["y0"], lay["y1"]], "py": py,
                   "ghost_planes": lay["halo"], "temporal_block": temporal, "transport": sim.transport,
                   "face_copy": "sdma" if sdma else native().face_copy_mode(),
                   "ipc_protocol": "direct" if native().ipc_direct_ok(lay["bytes"]) else "mailbox",
                   "graph": (sim.graph_replays - replays0) > 0, "graph_requested": chosen[0],
                   "graph_replays_timed": sim.graph_replays - replays0,
                   "graph_captures_timed": sim.graph_captures - captures0,
                   "min_rounds": chosen[1], "overlap": chosen[2], "trials": trials,
                   "timed_vs_trial": timed_vs_trial,
                   "repeats_ms_per_step": [round(d / a.steps * 1e3, 4) for d in dts]},
        "achieved_dram_TBps": round(dram_tbps, 3),
        "pct_of_hbm_copy_roof": round(100.0 * dram_tbps / HBM_MEASURED_TBPS, 1),
    }
    copy_tbps = measure_copy_tbps(slab_cells * prob.bytes_per_cell_per_step // 2)
    rec["measured_copy_TBps"] = round(copy_tbps, 3) if copy_tbps else None
    rec["pct_of_measured_copy"] = round(100.0 * dram_tbps / copy_tbps, 1) if copy_tbps else None
    print(json.dumps(rec), flush=True)
    sim.close()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse(argv)
    global _VERBOSE
    _VERBOSE = a.verbose
    if a.rank_proxy > 0:
        return run_proxy(a)
    if a.gpus > 1 and not launched() and not os.environ.get("MDFX_FORCE_DIST"):
        return self_launch(a, argv)

    import torch.distributed as dist

    from mpi_cuda_process_amd import Simulation, native
    from mpi_cuda_process_amd.parallel.dist import init_distributed

    force = os.environ.get("MDFX_FORCE_DIST", "") == "1"  # distributed path even at WORLD_SIZE 1 (tests)
    # the control plane's collectives are bounded too: a rank that hangs (e.g. never joins RCCL)
    # makes its peers' gloo calls raise after the watchdog plus a margin, and the run exits non-zero
    env = init_distributed("gloo", timeout_s=max(60.0, a.timeout + 60.0), force=force) \
        if (int(os.environ.get("WORLD_SIZE", "1")) > 1 or force) else None
    world = dist.get_world_size() if env else 1
    rank = dist.get_rank() if env else 0
    if env and world > 1 and a.gpus != world:
        print("bench: --gpus %d but the launcher started WORLD_SIZE %d ranks" % (a.gpus, world), file=sys.stderr)
        return 2
    want_hip = a.device != "cpu"
    ndev = torch.cuda.device_count() if want_hip else 0
    if env and want_hip and ndev > 0 and world > ndev and not a.share_gpu:
        if rank == 0:
            print("bench: %d ranks but only %d GPU(s) visible" % (world, ndev), file=sys.stderr)
        return 2
    hip = want_hip and torch.cuda.is_available()
    if a.device == "hip" and not hip:
        print("bench: --device hip but no HIP device is usable", file=sys.stderr)
        return 2
    device_id = -1
    if hip:
        device_id = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()
        torch.cuda.set_device(device_id)
    native().set_kernel_variant(a.variant)

    nx, ny, nz = a.nx or a.n, a.ny or a.n, a.nz or a.n
    if a.stencil in ("jacobi5", "life"):
        ny = 1  # 2D grids: nx = width, nz = height
    prob = make_problem(a, nx, ny, nz)
    # (z, y) pencils: py ranks along y. Auto: at 4+ processes the 3D 7-point (whose fused sweep
    # takes y ghost rows) tries 2 along y next to the z slabs, on every transport
    full = a.full  # gate, trials, verification, diagnostics, copy yardstick (a plain run: none of them)
    if a.py > 0:
        pys = [a.py]
    else:
        pys = [1, 2] if (full and env and world >= 4 and world % 2 == 0 and a.stencil == "heat7") else [1]
    temporal = pick_temporal(a, prob, max(1, world, a.virtual_ranks) // max(pys), hip)
    timeout = a.timeout if hip else 0.0

    slab_depth = temporal

    def depth_for(q):
        return depth_for_layout(slab_depth, q, hip)

    # ---- transport / graph mode: correctness gate (N > 1), then short timed trials ---------
    # Every (transport, graph) candidate that passes the bitwise gate gets a short timed trial on
    # the full problem; the fastest is timed for real. With one candidate there is no trial.
    transports = [a.transport]
    if env and a.transport == "auto" and full:
        # rccl (p2p kernels), ipc (pulls by the runtime's blit kernels), ipc_sdma (pulls by the
        # SDMA engines: no CUs taken from the interior sweep, lower bandwidth on one device)
        # (rccl_fold: rccl with the folded lower boundary, which rccl does not run by default; gated
        # and verified like any other candidate, Transport::fold_by_default)
        transports = ["rccl", "rccl_fold", "ipc", "ipc_sdma"] if hip else ["torch"]
    elif not env:
        transports = [a.transport if a.transport in ("loopback", "host") else "auto"]
    # (a plain run: the engine's own transport for "auto"; replayed cycles in one process, which
    # the trials of --full pick there, eager launches across processes, where no gate has run)
    graphs = {"on": [True], "off": [False]}.get(a.graph, [False, True] if (hip and full) else [hip and not env])
    # (captured cycles never fold and pencils never fold, so rccl_fold is an eager z-slab candidate)
    cands = [(t, g, q) for t in transports for q in pys for g in graphs if not (t == "rccl_fold" and (g or q > 1))]
    if hip and a.graph == "auto" and len(graphs) > 1:
        # rccl steps are captured only under HIP >= 7.2 (RcclTransport::graph_capturable); under the
        # runtime PyTorch bundles a graph candidate would just repeat the eager one
        from mpi_cuda_process_amd import native as _nat
        if not _nat().hip_runtime_version() >= 70200000:
            cands = [(t, g, q) for t, g, q in cands if not (t.startswith("rccl") and g)]
    if a.rounds != "auto":
        rounds = [int(a.rounds)]
    else:
        rounds = [2, 1] if (full and hip and env and world > 1) else [0]
    gate = None
    t_sel0 = time.time()  # gate + trials start (the --trial-budget clock)
    if full and env and world > 1 and not a.no_gate:
        recs, ok = [], []
        for t, g, q in cands:
            if g and (t, False, q) in cands and (t, False, q) not in ok:
                continue  # a transport whose eager run failed is not tried with graphs
            if t == "rccl_fold" and ("rccl", False, q) in cands and ("rccl", False, q) not in ok:
                continue  # nor rccl folded when plain rccl failed
            trace("gate %s graph=%s py=%d" % (t, g, q))
            passed, rec = run_gate(a, hip, t, depth_for(q), world, rank, graph=g, py=q)
            trace("gate %s graph=%s py=%d passed=%s" % (t, g, q, passed))
            recs.append(rec)
            if passed:
                ok.append((t, g, q))
        if not ok and a.transport == "auto" and hip:
            # last resort: faces staged through host memory over the gloo group. Slow, but a
            # correct number rather than none when neither device transport works on this node
            trace("gate staged (fallback)")
            passed, rec = run_gate(a, hip, "staged", temporal, world, rank, graph=False)
            recs.append(rec)
            if passed:
                ok.append(("staged", False, 1))
        gate = {"passed": bool(ok), "runs": recs}
        if not ok:
            if rank == 0:
                print("bench: correctness gate FAILED for every transport tried (%s); not timing"
                      % ", ".join(sorted(set(t for t, _, _ in cands))), file=sys.stderr)
            dist.barrier()
            dist.destroy_process_group()
            return 3
        cands = ok

    # the round count and the overlap mode need no gate of their own (scheduling only; the
    # overlapped == serialised equality is a test). Several processes: interior || boundary +
    # exchange (overlap) against one full sweep after the exchange, whichever the trial finds faster.
    overlaps = [True, False] if (full and hip and env and world > 1 and not a.no_overlap and not a.overlap) \
        else [not a.no_overlap]
    cands = [(t, g, r, ov, q) for t, g, q in cands for r in rounds for ov in overlaps]
    kw = dict(device="hip" if hip else "cpu", overlap=not a.no_overlap,
              residual_every=a.residual_every, timeout_s=timeout, temporal=temporal)

    def make_sim(transport, graph, rounds=0, overlap=True, py=1):
        if env:
            sim = Simulation(prob, distributed=True, transport=transport, graph=graph, py=py, share_gpu=a.share_gpu,
                             **dict(kw, temporal=depth_for(py)))
        else:
            sim = Simulation(prob, ranks=a.virtual_ranks or 1, distributed=False, transport=transport, graph=graph,
                             py=py, **dict(kw, temporal=depth_for(py)))
        sim.set_options(min_rounds=rounds, overlap=overlap)
        return sim

    def barrier():
        if env:
            dist.barrier()

    def timed(sim, steps):
        def sync():
            sim.synchronize()
            if hip:
                torch.cuda.synchronize()
        barrier()
        sync()
        t0 = time.perf_counter()
        sim.run(steps)
        sync()
        t1 = time.perf_counter()
        barrier()
        dt = t1 - t0
        if env:
            t = torch.tensor([dt], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    trials = []
    trial_passes = 0
    sim, sim_t = None, None
    if len(cands) > 1:
        # two interleaved passes over the candidates (sorted by transport, so each transport's engine
        # is built once per pass); a candidate's faster pass counts
        n_trial = max(2, a.trial_steps)
        best_t = {}
        for _pass in range(2):
            if _pass > 0:
                # the second (interleaved) pass only while the selection phase is inside its budget,
                # judged by the slowest rank's clock so every rank takes the same branch
                el = torch.tensor([time.time() - t_sel0], dtype=torch.float64)
                if env:
                    dist.all_reduce(el, op=dist.ReduceOp.MAX)
                if el.item() > a.trial_budget:
                    trace("trial budget spent after %.1f s: one pass" % el.item())
                    break
            trial_passes = _pass + 1
            for t, g, rr, ov, q in cands:
                if sim is not None and sim_t != (t, q):
                    sim.close()
                    sim = None
                if sim is None:
                    sim, sim_t = make_sim(t, g, rr, ov, q), (t, q)
                sim.set_options(graph=g, min_rounds=rr, overlap=ov)
                # exactly the timed run's sequence: fresh grid, captures, its own warm-up (so the trial
                # starts on the same buffer parity and replay history as the run it picks)
                sim.init()
                sim.prepare_graphs()  # capture before timing (no-op with graphs off)
                sim.run(a.warmup)
                dt = timed(sim, n_trial)
                trace("trial %s graph=%s rounds=%s overlap=%s py=%d: %.3f ms/step" % (t, g, rr, ov, q,
                                                                                    dt / n_trial * 1e3))
                key = (t, g, rr, ov, q)
                best_t[key] = min(best_t.get(key, 1e30), dt / n_trial * 1e3)
        for t, g, rr, ov, q in cands:
            trials.append({"transport": t, "graph": g, "min_rounds": rr, "overlap": ov, "py": q,
                           "ms_per_step": round(best_t[(t, g, rr, ov, q)], 4)})
        chosen = cands[min(range(len(trials)), key=lambda i: trials[i]["ms_per_step"])]
        if sim_t != (chosen[0], chosen[4]):
            sim.close()
            sim = None
    else:
        chosen = cands[0]
    if sim is None:
        sim = make_sim(*chosen)
    temporal = depth_for(chosen[4])
    sim.set_options(graph=chosen[1], min_rounds=chosen[2], overlap=chosen[3])
    trace("engine up (%s, graph=%s, rounds=%s, overlap=%s)" % (sim.transport, chosen[1], chosen[2], chosen[3]))
    sim.init()  # every timed run starts from the same initial grid
    # capture both parities' graph cycles now: whatever --warmup is, the timed region only replays
    n_graphs = sim.prepare_graphs()
    trace("init done (%d graph cycles captured)" % n_graphs)
    sim.run(a.warmup)
    trace("warmup enqueued")
    # a plain run has no trials before it and one repetition: the settling passes (untimed
    # repetitions of --steps steps) put the timed one where --full's median repetition is
    settle_steps = 0
    if hip and not full and a.steps > 0:
        settle_steps = a.steps * -(-SETTLE_MIN_STEPS // a.steps)
        for _ in range(settle_steps // a.steps):
            sim.run(a.steps)
    timed(sim, 0)
    trace("warmup done")
    inject_timed_fault(sim, rank, world)
    replays0, captures0 = sim.graph_replays, sim.graph_captures
    repeats = max(1, a.repeats)
    dts = []
    for _ in range(repeats):
        dts.append(timed(sim, a.steps))
        trace("timed %.4f s" % dts[-1])
    best = statistics.median(dts)  # the median repetition (back to back, same engine)
    if a.dump_outputs:
        trace("writing the outputs of the last timed step")
        dump_outputs(a, sim, prob, env, world, rank)
    verified = None
    if full and not a.no_verify:
        trace("verifying the timed run")
        verified = verify_timed(a, sim, prob, hip, env, rank, world, [a.warmup] + [a.steps] * repeats)
        trace("verified: %s" % verified)
        if not verified["passed"]:
            if rank == 0:
                print("bench: timed-run verification FAILED (max |diff| %g over %d ranks; the gate %s): not "
                      "reporting a number" % (verified["max_abs_diff"], world,
                                              "passed" if gate and gate["passed"] else "was not run"),
                      file=sys.stderr, flush=True)
            sim.close()
            if env:
                dist.barrier()
                dist.destroy_process_group()
            return 4

    phases = links = None
    if full and env and world > 1 and not a.no_diagnose:
        trace("diagnostic pass")
        phases, links = diagnose(sim, temporal, env, world, rank)

    devices = [device_id]
    if env:
        allp = [None] * world
        dist.all_gather_object(allp, device_id)
        devices = allp
    cells = prob.cells
    gcells = cells * a.steps / best / 1e9
    ms = best / a.steps * 1e3
    # the timed run against the trial that chose its configuration: well above 1 means the timed
    # run landed in a slower state than its trial measured (reported, and warned about)
    timed_vs_trial = round(ms / min(t["ms_per_step"] for t in trials), 3) if trials else None
    if timed_vs_trial is not None and timed_vs_trial > 1.2 and rank == 0:
        print("bench: WARNING: the timed run took %.2fx its trial's time per step" % timed_vs_trial,
              file=sys.stderr, flush=True)
    nproc = world if env else 1
    # per physical GPU: ranks that share a device (--share-gpu) count once
    ngpu_phys = len(set(devices)) if hip else nproc
    per_gpu = gcells / max(ngpu_phys, 1)
    # DRAM actually required per time step: one read + one write of every cell per sweep, and a
    # sweep advances `temporal` steps
    dram_tbps = per_gpu * prob.bytes_per_cell_per_step / temporal / 1e3
    if rank == 0:
        sim_transport = sim.transport
        decomp = "slab-z%d" % world if chosen[4] == 1 else "pencil-z%dy%d" % (world // chosen[4], chosen[4])
        par = ("%s (1 process/GPU, %s halo, %s schedule)" % (decomp, sim_transport, sim.schedule)
               if env else ("slab-z%d virtual in 1 process (%s)" % (a.virtual_ranks, sim_transport)
                            if a.virtual_ranks > 1 else "single GPU" if hip else "cpu"))
        model = {"heat7": "3D 7-pt Jacobi", "box27": "3D 27-pt", "jacobi5": "2D 5-pt MDF",
                 "life": "2D Game of Life"}[a.stencil]
        rec = {
            "metric": METRIC if (a.stencil == "heat7" and a.dtype == "f32" and (nx, ny, nz) == (1024,) * 3)
            else "GCells/s (whole node), %s %dx%dx%d %s" % (model, nx, ny, nz, a.dtype),
            "value": round(gcells, 3),
            "unit": "GCells/s",
            "n_gpus": nproc,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms, 4),
            "higher_is_better": True,
            "full": full,
            "settle_steps": settle_steps,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": {"f32": "fp32", "f64": "fp64", "u8": "u8"}[a.dtype],
            "data": "synthetic (uniform random grid from a counter hash of the global index, seed 1)",
            "config": {
                "model": "%s %dx%dx%d %s" % (model, nx, ny, nz, a.dtype),
                "global_batch": 1,
                "seq_len": nz,
                "grid": [nx, ny, nz],
                "parallelism": par,
                "ranks": nproc,
                "devices": devices,
                "distinct_devices": len(set(devices)) if hip else 0,
                "transport": sim_transport,
                "comm_size": nproc if sim_transport.startswith("rccl") else 0,
                "kernel_variant": native().kernel_variant(),
                # effective mode: true only if captured cycles actually replayed in the timed region
                "graph": (sim.graph_replays - replays0) > 0,
                "graph_requested": chosen[1],
                "graph_replays_timed": sim.graph_replays - replays0,
                "graph_captures_timed": sim.graph_captures - captures0,
                "min_rounds": chosen[2] or ("2 (auto)" if nproc > 1 or a.virtual_ranks > 1 else "1 (auto)"),
                "trials": trials,
                "trial_passes": trial_passes,
                "overlap": chosen[3],
                "timed_vs_trial": timed_vs_trial,
                "schedule": sim.schedule,
                "repeats_ms_per_step": [round(d / a.steps * 1e3, 4) for d in dts],
                "verified": verified,
                "face_copy": ("sdma" if sim_transport == "ipc_sdma" else native().face_copy_mode())
                if sim_transport in ("ipc", "ipc_sdma") else None,
                "ipc_protocol": (("direct" if native().ipc_direct_ok(sim.layout(0)["bytes"]) else "mailbox")
                                 if sim_transport in ("ipc", "ipc_sdma") else None),
                "temporal_block": temporal,
                "py": chosen[4],
                "gate": gate,
                "phases": phases,
                "links": links,
            },
            "per_gpu_gcells": round(per_gpu, 3),
            "dram_bytes_per_step_per_gpu": int(cells / max(ngpu_phys, 1) * prob.bytes_per_cell_per_step / temporal),
            "achieved_dram_TBps_per_gpu": round(dram_tbps, 3) if hip else None,
            "pct_of_hbm_copy_roof": round(100.0 * dram_tbps / HBM_MEASURED_TBPS, 1) if hip else None,
        }
        # the achievable-copy yardstick: torch copy_ of one GPU's share of the field (outside the timed
        # region; a fused sweep moves exactly these bytes per `temporal` steps)
        copy_tbps = measure_copy_tbps(cells / max(ngpu_phys, 1) * prob.bytes_per_cell_per_step / 2) \
            if (hip and full) else None
        rec["measured_copy_TBps"] = round(copy_tbps, 3) if copy_tbps else None
        rec["pct_of_measured_copy"] = round(100.0 * dram_tbps / copy_tbps, 1) if copy_tbps else None
        rec["wall_s"] = round(time.time() - _T_START, 2)  # the whole bench process so far (gate, trials, timing, checks)
        print(json.dumps(rec), flush=True)
    sim.close()
    if env:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
