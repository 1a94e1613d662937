#!/usr/bin/env python3
"""bench.py -- parcel moment-RHS evaluations per second of the MI355X coalescence kernel.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--parcels P] [--workload cfg3a|cfg3b|cfg2]
                    [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path (cloudy_coal_rhs: normalise -> closure inversion -> moments ->
finite 2-D integrals -> Q/R/S -> de-normalise) over one device-resident batch of synthetic parcels.
Headline workload (BASELINE.json configs[2], SURVEY.md 8(d) "cfg3a"): 1e7 parcels per GPU, two Gamma modes,
order-2 polynomial CoalescenceTensors (the exact pieces of Long's kernel), 6 prognostic moments, fp64,
thresholds (Inf, Inf).

A plain run sets up, warms up, times exactly K steps and prints the line: value = parcels x K / wall, ms_per_step =
wall / K.  --dump-outputs DIR then writes what the last timed step computed (see _dump_outputs).  --full adds everything
else: HIP-event kernel times and rooflines, the conservation diagnostic through the RCCL communicator, the variants (the
same batch with the reference example's finite threshold (5e-10 kg, Inf), "cfg3b", the Simpson / incomplete-gamma path;
other precisions, configurations and integrators) and the CPU baselines.

Multi-GPU: one process per GPU (torch.distributed, backend nccl = RCCL); parcels shard with no data-path
collective (weak scaling: every rank owns --parcels parcels).  The only collective is the all-reduce of the
nmom tendency sums for the mass-conservation diagnostic, outside the per-step path.

Rank 0 prints ONE JSON line (see the keys at the bottom).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20260723
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
FP64_VALU_PEAK_TFLOPS = 78.6  # half the guide's 157.3 TF fp32 vector peak: a wave64 fp64 FMA issues in 4 cycles per SIMD


def _measured_latest():
    """PMC-derived per-launch figures committed by tools/summarize_profiles.py (profiles/measured_latest.json)."""
    try:
        with open(os.path.join(ROOT, "profiles", "measured_latest.json")) as f:
            return json.load(f)
    except Exception:
        return {}
NORMS = (1e6, 1e-9)    # every reference example, e.g. box_single_gamma.jl:25
INF = float("inf")


# ------------------------------------------------------------------------------------------------
# synthetic Gamma-mixture batches; the generator is shared by tests and smoke()
# ------------------------------------------------------------------------------------------------
def _gamma_mode(rng, n, n_lo, n_hi, k_lo, k_hi, x_lo, x_hi):
    nn = 10.0 ** rng.uniform(np.log10(n_lo), np.log10(n_hi), n)
    k = rng.uniform(k_lo, k_hi, n)
    xbar = 10.0 ** rng.uniform(np.log10(x_lo), np.log10(x_hi), n)
    th = xbar / k
    # get_moments, ParticleDistributions.jl:293-299
    return np.stack([nn, nn * k * th, nn * k * (k + 1.0) * th * th])


def synth_moments(n_modes, n, seed=SEED, degenerate_frac=0.01):
    """(3*n_modes, n) physical moments: cloud, rain, (drizzle-size third) Gamma modes, ~1 % degenerate parcels."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    specs = [(1e6, 1e9, 0.5, 8.0, 1e-11, 1e-9), (1.0, 1e5, 1.0, 6.0, 1e-9, 1e-7), (1e-3, 1e2, 1.0, 6.0, 1e-7, 1e-5),
             (1e-6, 1e-1, 1.0, 6.0, 1e-5, 1e-3)]
    mom = np.concatenate([_gamma_mode(rng, n, *specs[i]) for i in range(n_modes)], axis=0)
    nd = int(n * degenerate_frac)
    if nd > 0:
        idx = rng.choice(n, nd, replace=False)
        kind = rng.integers(0, 4, nd)
        for mode in range(n_modes):
            r = 3 * mode
            z = idx[kind == 0]          # empty mode: M0 <= eps -> fallback (0, 1, 1)
            mom[r:r + 3, z] = 0.0
            s = idx[kind == 1]          # zero variance: M2/M1 == M1/M0 -> k = +Inf -> clamp 10
            mom[r + 2, s] = mom[r + 1, s] ** 2 / mom[r, s]
            g = idx[kind == 2]          # negative variance -> k < 0 -> clamp eps
            mom[r + 2, g] = 0.5 * mom[r + 1, g] ** 2 / mom[r, g]
            h = idx[kind == 3]          # very narrow: k just above the upper clamp
            mom[r + 2, h] = mom[r + 1, h] ** 2 / mom[r, h] * (1.0 + 1.0 / 25.0)
    return np.ascontiguousarray(mom)


def workload_spec(name):
    """-> (n_modes, kernel pieces, thresholds) of a named workload, physical units."""
    long_k = dict(x_threshold=5.236e-10, below=9.44e9, above=5.78)  # box_gamma_mixture_long.jl:20
    if name == "cfg2":   # 1 Gamma mode, Golovin b = 5 (box_single_gamma.jl:19), thr (Inf,)
        return dict(n_modes=1, kernel="golovin", thresholds=(INF,), default_parcels=1_000_000)
    if name == "cfg3a":  # 2 Gamma modes, Long pieces order 2, thr (Inf, Inf)
        return dict(n_modes=2, kernel="long", long=long_k, thresholds=(INF, INF), default_parcels=10_000_000)
    if name == "cfg3b":  # same, reference thresholds (box_gamma_mixture_long.jl:36)
        return dict(n_modes=2, kernel="long", long=long_k, thresholds=(5e-10, INF), default_parcels=10_000_000)
    if name == "cfg4":   # BASELINE configs[3] in the reference's formulation: 3 Gamma modes, hydrodynamic kernel as an
        # order-4 fitted tensor (box_gamma_mixture_hydro.jl:22-23), thresholds of box_gamma_mixture_3modes.jl:29
        return dict(n_modes=3, kernel="hydro", thresholds=(1e-9, 1e-7, INF), default_parcels=12_500_000)
    if name == "moving4":  # box_gamma_mix_moving.jl:13-30: 4 Gamma modes, Golovin b = 5, MovingThreshold percentiles 0.99
        return dict(n_modes=4, kernel="golovin", thresholds=(0.99, 0.99, 0.99, 1.0), moving=True,
                    default_parcels=2_500_000)
    raise ValueError(f"unknown workload {name}")


def kernel_matrix(spec):
    """[N, N, P, P] un-normalised coefficient tensors (physical units)."""
    N = spec["n_modes"]
    eps = float(np.finfo(np.float64).eps) / NORMS[0]  # forced constant term C_1_1 = eps (normalised), KernelTensors.jl:115
    if spec["kernel"] == "golovin":
        c = np.array([[eps, 5.0], [5.0, 0.0]])  # CoalescenceTensor(LinearKernelFunction(5.0), 1, 1e-6): C_1_1 = eps
        return np.broadcast_to(c, (N, N, 2, 2)).copy()
    if spec["kernel"] == "hydro":
        import __graft_entry__ as ge

        pkg = ge.load_package()
        t = pkg.CoalescenceTensor(pkg.HydrodynamicKernelFunction(1e2 * np.pi), 4, 1e-6)  # least-squares fit (host)
        return np.broadcast_to(t.c, (N, N, 5, 5)).copy()
    lk = spec["long"]
    kc = np.zeros((N, N, 3, 3))
    for j in range(N):
        for k in range(N):
            kc[j, k, 0, 0] = eps
            if j == 0 and k == 0:   # CoalescenceTensor(kernel_func, 2, 5e-10): below-threshold piece b (x^2 + y^2)
                kc[j, k, 0, 2] = kc[j, k, 2, 0] = lk["below"]
            else:                   # CoalescenceTensor(kernel_func, 2, 1e-6, 5e-10): a (x + y)
                kc[j, k, 0, 1] = kc[j, k, 1, 0] = lk["above"]
    return kc


def make_workload(name, n_parcels, seed=SEED):
    """Product-side objects of a workload: moments, CoalescenceData, ODE parameters (no oracle involved)."""
    import __graft_entry__ as ge

    pkg = ge.load_package()
    spec = workload_spec(name)
    N = spec["n_modes"]
    kc = kernel_matrix(spec)
    kernels = tuple(tuple(pkg.CoalescenceTensor(kc[j, k]) for k in range(N)) for j in range(N))
    NProgMoms = (3,) * N
    ts = pkg.MovingThreshold() if spec.get("moving") else pkg.FixedThreshold()
    coal_data = pkg.CoalescenceData(kernels, NProgMoms, spec["thresholds"], NORMS, ts)
    pdists = tuple(pkg.GammaPrimitiveParticleDistribution(1.0, 1.0, 1.0) for _ in range(N))
    par = pkg.ODEParameters(pdists, coal_data, NProgMoms, NORMS)
    return dict(name=name, spec=spec, mom=synth_moments(N, n_parcels, seed), coal_data=coal_data,
                dist_types=[1] * N, par=par, kernel_c=kc, NProgMoms=NProgMoms)


def oracle_params(name):
    """co_params of the CPU oracle for a workload (checker / cpu_baseline only)."""
    from oracle import cloudy_oracle as O

    spec = workload_spec(name)
    return O.make_params([O.GAMMA] * spec["n_modes"], kernel_matrix(spec), spec["thresholds"], norms=NORMS,
                         threshold_style=O.MOVING_THRESHOLD if spec.get("moving") else O.FIXED_THRESHOLD)


# ------------------------------------------------------------------------------------------------
RANK_DONE_MARK = "bench.py rank done"     # last stderr line of a rank that ran to the end (see _spawn_ranks)
EXIT_RANK_FAILED, EXIT_FEWER_DEVICES, EXIT_LAUNCH_TIMEOUT = 5, 4, 6


def _rank_log_dir():
    d = os.environ.get("CLOUDY_BENCH_LOG_DIR") or os.path.join(ROOT, "bench_rank_logs")
    os.makedirs(d, exist_ok=True)
    return d


def _tail(path, n=12):
    try:
        with open(path, errors="replace") as f:
            return [l.rstrip("\n") for l in f.readlines()[-n:]]
    except OSError:
        return []


def _spawn_ranks(n_gpus, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher (WORLD_SIZE unset): this parent -- which never touches the
    GPU, never imports torch and never loads libcloudy_hip.so -- starts N fresh child processes of this script, one rank
    per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set as torch.distributed.run would) and relays rank 0's JSON line.

    VERDICT r5 item 1: the parent POLLS all children.  The first rank that exits non-zero -- or exits 0 without having
    written the end-of-run mark, i.e. before the last barrier -- ends the run: the siblings (blocked in a collective that
    will never complete) are terminated, and the parent exits non-zero with ONE line naming the rank, its exit code and
    its last stderr lines.  Every rank has its own `rank<k>.out` / `rank<k>.err` under CLOUDY_BENCH_LOG_DIR (default
    bench_rank_logs/); a wall-clock limit (CLOUDY_BENCH_LAUNCH_TIMEOUT, default 1500 s: inside the driver's 1800 s) covers a
    rank that hangs without dying.  No re-exec anywhere: children are fresh processes."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    logs = _rank_log_dir()
    limit = float(os.environ.get("CLOUDY_BENCH_LAUNCH_TIMEOUT", "1500"))
    procs, files = [], []
    for r in range(n_gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_gpus), LOCAL_WORLD_SIZE=str(n_gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CLOUDY_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        fo = open(os.path.join(logs, f"rank{r}.out"), "w")
        fe = open(os.path.join(logs, f"rank{r}.err"), "w")
        files += [fo, fe]
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, stdout=fo, stderr=fe,
                                      start_new_session=True))
    t0 = time.monotonic()
    reason, code = None, 0
    live = set(range(n_gpus))
    while live and reason is None:
        for r in sorted(live):
            rc = procs[r].poll()
            if rc is None:
                continue
            live.discard(r)
            err_tail = _tail(os.path.join(logs, f"rank{r}.err"))
            if rc != 0:
                why = next((l for l in reversed(err_tail) if l.strip() and l.strip() != RANK_DONE_MARK), "(no stderr output)")
                reason, code = f"rank {r} exited with code {rc}: {why.strip()[:300]}", (rc if rc in (3, EXIT_FEWER_DEVICES) else EXIT_RANK_FAILED)
                break
            if RANK_DONE_MARK not in err_tail:
                reason, code = (f"rank {r} exited with code 0 before the end of the run (no '{RANK_DONE_MARK}' line in "
                                f"{logs}/rank{r}.err)"), EXIT_RANK_FAILED
                break
        if reason is None and live:
            if time.monotonic() - t0 > limit:
                reason, code = (f"ranks {sorted(live)} still running after {limit:.0f} s (CLOUDY_BENCH_LAUNCH_TIMEOUT); "
                                f"terminated"), EXIT_LAUNCH_TIMEOUT
                break
            time.sleep(0.1)
    if reason is not None:
        import signal

        for r in sorted(live):                      # the siblings: blocked in a collective that will never complete
            try:
                os.killpg(procs[r].pid, signal.SIGTERM)
            except (ProcessLookupError, PermissionError):
                pass
        t1 = time.monotonic()
        for r in sorted(live):
            try:
                procs[r].wait(timeout=max(0.1, 5.0 - (time.monotonic() - t1)))
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(procs[r].pid, signal.SIGKILL)
                except (ProcessLookupError, PermissionError):
                    pass
                procs[r].wait()
    for f in files:
        f.close()
    # rank 0's stderr (the full result object) and stdout (the line) are relayed; the other ranks' logs stay in their files
    sys.stderr.write("".join(l + "\n" for l in _tail(os.path.join(logs, "rank0.err"), 400) if l.strip() != RANK_DONE_MARK))
    if reason is not None:
        sys.stderr.write(f"bench.py --gpus {n_gpus}: FAILED: {reason} (per-rank logs: {logs}/rank<k>.err)\n")
        sys.stderr.flush()
        raise SystemExit(code or EXIT_RANK_FAILED)
    with open(os.path.join(logs, "rank0.out")) as f:
        sys.stdout.write(f.read())
    sys.stdout.flush()
    return 0


_COMM = {"comm": None, "collective": None, "own_gpu_per_rank": True, "fallback": False}


def _fault(point, rank):
    """Failure injection for the launcher tests (tests/test_sharding.py): CLOUDY_BENCH_FAULT="<what>@<point>:<rank>", what in
    {raise, exit0, hang}, point in {after_init, before_barrier}.  Never set outside the tests."""
    spec = os.environ.get("CLOUDY_BENCH_FAULT", "")
    if not spec:
        return
    what, _, where = spec.partition("@")
    pt, _, rk = where.partition(":")
    if pt != point or int(rk or -1) != rank:
        return
    if what == "raise":
        raise RuntimeError(f"injected failure on rank {rank} at {point} (CLOUDY_BENCH_FAULT)")
    if what == "exit0":
        os._exit(0)
    if what == "hang":
        time.sleep(10_000)


def _dist_setup(n_gpus):
    """torch.distributed as the CONTROL plane of a multi-rank run (barrier, max-over-ranks of the timing contract, the
    courier of the 128-byte RCCL id); -> (rank, world, local_rank, dist or None, torch or None).
    VERDICT r4 item 5 (ii): the control group is gloo (CPU tensors over MASTER_ADDR:MASTER_PORT) so that each rank opens
    exactly ONE RCCL communicator -- the one inside libcloudy_hip.so that carries the path's only collective
    (cloudy_moment_sums_allreduce).  CLOUDY_BENCH_BACKEND=nccl restores torch's own RCCL group as the courier.
    VERDICT r5 item 1: every collective of the control plane has a timeout (CLOUDY_BENCH_DIST_TIMEOUT, default 300 s; a dead
    peer is then an error on the survivors, not torch's 30 minutes), and FEWER VISIBLE DEVICES THAN LOCAL RANKS IS AN ERROR
    (exit code 4) unless CLOUDY_BENCH_ALLOW_SHARED_GPU=1 (the 1-GPU test boxes): ranks are never mapped onto a shared GPU
    silently -- that would print a 1x "scaling curve" with exit code 0."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1:
        return 0, 1, 0, None, None
    import datetime

    import torch  # imported BEFORE libcloudy_hip.so so that both share one HIP runtime (same SONAME)
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    backend = os.environ.get("CLOUDY_BENCH_BACKEND", "gloo")
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    n_vis = torch.cuda.device_count()               # (counting devices does not initialise the GPU)
    dry = os.environ.get("CLOUDY_BENCH_DRY_CONTROL_PLANE") == "1"
    if n_vis < local_world and not dry:
        if os.environ.get("CLOUDY_BENCH_ALLOW_SHARED_GPU") != "1":
            sys.stderr.write(f"bench.py rank {rank}: {n_vis} HIP device(s) visible for {local_world} local rank(s): one GPU per "
                             "rank is required (CLOUDY_BENCH_ALLOW_SHARED_GPU=1 lets ranks share devices on a test box)\n")
            sys.stderr.flush()
            raise SystemExit(EXIT_FEWER_DEVICES)
        if n_vis < 1:
            raise SystemExit("bench.py needs a HIP device: the coalescence RHS has no CPU fallback")
    n_dev = max(n_vis, 1)
    _COMM["own_gpu_per_rank"] = local_world <= n_dev
    timeout = datetime.timedelta(seconds=float(os.environ.get("CLOUDY_BENCH_DIST_TIMEOUT", "300")))
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, timeout=timeout,
                                device_id=torch.device("cuda", local_rank))
    else:
        local_rank = local_rank % n_dev             # only with CLOUDY_BENCH_ALLOW_SHARED_GPU=1 is this ever a wrap-around
        if not dry:
            torch.cuda.set_device(local_rank)       # (torch.cuda.synchronize() of the timing bracket looks at this device)
        dist.init_process_group(backend=backend, rank=rank, world_size=world, timeout=timeout)
    _fault("after_init", rank)
    return rank, world, local_rank, dist, torch


def _dry_control_plane(args, rank, world, dist, torch, json_out):
    """CLOUDY_BENCH_DRY_CONTROL_PLANE=1 (launcher tests on a box without a GPU): the control plane of a multi-rank run and
    nothing else -- rendezvous, the barrier + max-over-ranks bracket around K stub steps, the gather of the per-rank
    records, the final barrier, rank 0's line -- with NO GPU work; the line says so ("data": "dry-run ...", value null) and
    is not a measurement."""
    _fault("before_barrier", rank)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001)
    dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    recs = _gather_objects({"rank": rank, "pid": os.getpid(), "device": None, "pci_bus_id": None, "kernel_ms": None}, dist)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        out = {"metric": "parcel moment-RHS evals/sec at 1e7 parcels; achieved HBM GB/s vs 8 TB/s peak", "value": None,
               "unit": "parcel-RHS/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": 1e3 * float(t.item()) / max(args.steps, 1), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "f64", "data": "dry-run of the control plane: NO GPU work, not a measurement",
               "config": {"workload": "none (CLOUDY_BENCH_DRY_CONTROL_PLANE=1)"}, "per_rank_devices": recs}
        emit(out, json_out, side_file=False)     # (a dry run never overwrites a measured bench_variants.json)
    return 0


def _gather_objects(obj, dist):
    """[obj of rank 0, obj of rank 1, ...] on every rank (small JSON-able records; gloo or nccl control group)."""
    if dist is None:
        return [obj]
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, obj)
    return parts


def _comm_setup(pkg, world, local_rank, dist, torch):
    """The RCCL communicator behind the C ABI (cloudy_comm_create -> ncclCommInitRank inside libcloudy_hip.so) for the one
    collective of the path, the all-reduce of the moment sums.  torch.distributed is only the courier of the 128-byte
    unique id (and the barrier / max-over-ranks of the timing contract).  All ranks agree on the outcome: if any rank
    fails to form the communicator (e.g. several ranks share ONE GPU on a test box: RCCL refuses duplicate devices),
    every rank falls back to summing host-side partial sums through torch.distributed."""
    if os.environ.get("CLOUDY_BENCH_NO_RCCL_ABI") == "1":
        _COMM["collective"] = "torch.distributed (CLOUDY_BENCH_NO_RCCL_ABI=1)" if dist is not None else "none"
        return
    ok, why = 1, ""
    try:
        if dist is None:
            _COMM["comm"] = pkg.Communicator(1, 0, pkg.Communicator.unique_id(), local_rank)
        elif _COMM["own_gpu_per_rank"]:
            # ncclCommInitRank with more than one rank has never run on hardware from inside this library (no multi-GPU
            # box was available to any round): it runs under a watchdog, so that a rendezvous that never completes costs
            # the C-ABI collective (fallback below, "collective_fallback": true in the line, NON-ZERO exit code) and not
            # the bench line
            import threading

            box = {}
            c_rank, c_world, uid = pkg.Communicator.exchange_unique_id()   # (torch collectives stay on this thread)

            def make():
                try:
                    box["comm"] = pkg.Communicator(c_world, c_rank, uid, local_rank)
                except Exception as e:   # noqa: BLE001
                    box["err"] = f"{type(e).__name__}: {e}"

            limit = float(os.environ.get("CLOUDY_BENCH_COMM_TIMEOUT", "180"))
            th = threading.Thread(target=make, daemon=True)
            th.start()
            th.join(limit)
            if th.is_alive():
                ok, why = 0, f"cloudy_comm_create did not return within {limit:.0f} s"
                _COMM["hung"] = True
            elif "err" in box:
                ok, why = 0, box["err"]
            else:
                _COMM["comm"] = box["comm"]
        else:
            ok, why = 0, "several ranks share one GPU (RCCL refuses duplicate devices)"
    except Exception as e:   # noqa: BLE001 -- any failure means the fallback, reported in the JSON line
        ok, why = 0, f"{type(e).__name__}: {e}"
    if dist is not None:
        flag = torch.tensor([ok], dtype=torch.int32, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0 and _COMM["comm"] is not None:
            _COMM["comm"].close()
            _COMM["comm"] = None
            why = why or "another rank could not form the communicator"
    if _COMM["comm"] is not None:
        v = pkg.lib().cloudy_comm_rccl_version()
        _COMM["collective"] = (f"ncclAllReduce(sum, f64, nmom) inside libcloudy_hip.so (cloudy_moment_sums_allreduce), "
                               f"RCCL {v // 10000}.{v // 100 % 100}.{v % 100}, {world} rank(s)")
    else:
        _COMM["fallback"] = True
        _COMM["collective"] = (f"FALLBACK torch.distributed all_reduce of host-side sums ({dist.get_backend() if dist else 'n/a'}); "
                               f"C-ABI RCCL communicator not formed: {why}")


def _time_steps(pkg, plan, m, dm, steps, dist, torch):
    """EXACTLY `steps` launches between barrier+sync brackets; returns wall seconds (max over ranks)."""
    L = pkg.lib()
    n, ld = m.shape[1], m.shape[1]
    if dist is not None:
        torch.cuda.synchronize()
        dist.barrier()
    pkg._lib.check(L.cloudy_stream_synchronize(None))
    t0 = time.perf_counter()
    for _ in range(steps):
        pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, ld, m.ptr, dm.ptr, None))
    pkg._lib.check(L.cloudy_stream_synchronize(None))
    if dist is not None:
        torch.cuda.synchronize()
    # Round 6: a rank's clock stops when ITS K steps are done; the closing barrier of the bracket comes after it, and the MAX over
    # ranks below is the job's time (every rank started from the opening barrier).  Before, the closing barrier -- a gloo barrier
    # over TCP, 0.3-2 ms for 8 ranks -- sat INSIDE the timed region: 1-6 % of 200 steps of 0.16 ms, a third of the driver's 20 steps,
    # charged to a path that has no collective.
    dt = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
        t = torch.tensor([dt], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


WARM_SECONDS = 0.15      # back-to-back launches before anything is timed (see _sustained_ms)
TIMED_MS = 40.0          # ... and at least this much GPU time inside the timed region


def _sustained_ms(pkg, launch, min_reps=5, max_reps=400):
    """Milliseconds per call of launch() at the clock the GPU SUSTAINS: >= WARM_SECONDS of back-to-back calls first, then
    HIP events (on the launch stream) around enough calls to cover >= TIMED_MS.  Round 4 finding (profiles/r04_time_warm.txt): the
    variants used to be timed over 3-5 launches right after their input had been generated and copied by the host -- the
    GPU idle for 0.1-1 s -- and a 1-ms kernel then runs at a clock it leaves within tens of ms: the fused SSPRK33
    integrator measured 1.14 ms that way and 0.89 ms sustained, moving4 1.63 / 1.37, cfg3b 2.35 / 2.04 (the headline,
    which always had its ~80 ms of warm-up, 0.158 / 0.158).  VERDICT r3 read the difference as idle issue slots."""
    L = pkg.lib()
    t0, calls = time.perf_counter(), 0
    while True:
        for _ in range(4):
            launch()
        pkg._lib.check(L.cloudy_stream_synchronize(None))
        calls += 4
        el = time.perf_counter() - t0
        if el >= WARM_SECONDS:
            break
    per_ms = 1e3 * el / calls
    reps = int(min(max(min_reps, TIMED_MS / max(per_ms, 1e-3)), max_reps))
    with _EventTimer(pkg) as tm:
        for _ in range(reps):
            launch()
    return tm.ms / reps


def _event_ms(pkg, plan, m, dm, iters, warm=True):
    """Average launch duration of cloudy_coal_rhs from HIP events recorded on the launch stream (cloudy_time_coal_rhs),
    after the sustained-clock warm-up of _sustained_ms; at least `iters` launches and >= TIMED_MS of GPU time."""
    import ctypes as C

    L = pkg.lib()
    n = m.shape[1]
    if warm:
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < WARM_SECONDS:
            for _ in range(4):
                pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, n, m.ptr, dm.ptr, None))
            pkg._lib.check(L.cloudy_stream_synchronize(None))
            calls += 4
        per_ms = 1e3 * (time.perf_counter() - t0) / calls
        iters = int(min(max(iters, TIMED_MS / max(per_ms, 1e-3)), 2000))
    ms = C.c_float()
    pkg._lib.check(L.cloudy_time_coal_rhs(plan.handle, n, n, m.ptr, dm.ptr, None, iters, C.byref(ms)))
    return float(ms.value)


def _gather(x, dist, torch):
    """[x of rank 0, x of rank 1, ...] (all ranks get the list)."""
    if dist is None:
        return [float(x)]
    dev = "cuda" if dist.get_backend() == "nccl" else "cpu"
    mine = torch.tensor([float(x)], dtype=torch.float64, device=dev)
    parts = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, mine)
    return [float(t.item()) for t in parts]


DUMP_MAX_BYTES = 48 << 20   # --dump-outputs: what one run writes at most (the cap is 64 MB)


def _dump_outputs(out_dir, dm, name="dm"):
    """--dump-outputs: the tendencies dM/dt of the last timed step -- what the caller of cloudy_coal_rhs receives -- as
    <out_dir>/<name>.npy, (planes, parcels) in the batch's own precision.  A batch larger than DUMP_MAX_BYTES is sampled: a
    fixed set of parcel columns (seeded, sorted; the same for every run with the same --workload / --parcels)."""
    os.makedirs(out_dir, exist_ok=True)
    planes, n = dm.shape
    a = dm.to_numpy()
    cap = DUMP_MAX_BYTES // (planes * a.dtype.itemsize)
    if n > cap:
        idx = np.sort(np.random.Generator(np.random.Philox(key=SEED + 1)).choice(n, cap, replace=False))
        a = a[:, idx]
    np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def _run_workload(pkg, name, n_parcels, steps, warmup, rank, dist, torch, full=True, dump_dir=None):
    """Warm-up + exactly `steps` timed launches; with `full`, the HIP-event kernel time and the conservation diagnostic"""
    wl = make_workload(name, n_parcels, seed=SEED + 1000 * rank)
    plan = wl["coal_data"].plan(wl["dist_types"])
    m = pkg.DeviceArray.from_numpy(wl["mom"])
    dm = pkg.DeviceArray.zeros(*wl["mom"].shape)
    rhs = pkg.make_box_model_rhs(pkg.AnalyticalCoalStyle(), pkg.MovingThreshold() if wl["spec"].get("moving") else None)
    # W untimed warm-up steps through the operator boundary -- and at least ~80 ms of back-to-back launches: after
    # idling the GPU needs tens of ms of continuous work to reach its sustained clocks (a 0.17 ms launch measured
    # 0.24 / 0.19 / 0.17 ms per step over the first 10 / 50 / 200 launches, round 1).
    t_w = time.perf_counter()
    done = 0
    while done < max(warmup, 1) or (time.perf_counter() - t_w) < 0.08:
        for _ in range(8):
            rhs(dm, m, wl["par"], 0.0)
        pkg._lib.check(pkg.lib().cloudy_stream_synchronize(None))
        done += 8
    wall = _time_steps(pkg, plan, m, dm, steps, dist, torch)
    if dump_dir:
        _dump_outputs(dump_dir, dm)
    if not full:
        return dict(wl=wl, plan=plan, wall=wall, nmom=plan.nmom)
    ev_ms = _event_ms(pkg, plan, m, dm, steps)
    # conservation diagnostic: sum over parcels and modes of dM1 must vanish (mass is conserved)
    if _COMM["comm"] is not None:     # local plane sums + ncclAllReduce on the launch stream, inside the library
        gsums = _COMM["comm"].allreduce_moment_sums(plan, dm)
    else:
        sums = pkg.moment_sums(plan, dm)
        gsums = pkg.allreduce_sums(sums) if dist is not None else sums
    tot = pkg.mode_sums(gsums, wl["NProgMoms"])
    # mode 0 only loses mass (it collects nothing), so |sum_p dM1_mode0| is the gross mass-transfer rate.
    # (With ~1 % degenerate parcels in the batch, whose clamped closures give tendencies up to 1e30, the batch sum is
    # dominated by a few parcels and the residual is below one ulp of it; the per-parcel figure is the sharper one.)
    gross = abs(float(gsums[1]))
    # (a slice of the full-size result: no extra, smaller launch of the same kernel -- the rocprofv3 stats of a kernel name
    # then average launches of ONE size)
    ds = dm.columns_to_numpy(min(100_000, n_parcels))
    nm = plan.nmom // 3
    net = sum(ds[3 * i + 1] for i in range(nm))
    mag = sum(np.abs(ds[3 * i + 1]) for i in range(nm))
    per_parcel = float(np.max(np.abs(net) / np.maximum(mag, 1e-300)))
    return dict(wl=wl, plan=plan, wall=wall, event_ms=ev_ms, mass_rate_sum=float(tot[1]), mass_rate_gross=gross,
                mass_per_parcel=per_parcel, nmom=plan.nmom)


# the reference's only published performance statements for this path: BenchmarkTools minimum-time CEILINGS asserted in
# its CI (test/unit_tests/performance_tests.jl:66-112, one CPU of a CliMA Buildkite slurm node), per call, Julia
REFERENCE_CI_CEILINGS_NS = {
    "update_dist_from_moments (each closure family)": 200,                                # performance_tests.jl:66
    "get_moments": 60,                                                                    # :67-73
    "moment_source_helper(Exponential(10,1), 1.0, 0.0, 1.2)": 16_000,                     # :76-82
    "moment_source_helper(Gamma(5,10,2), 1.0, 0.0, 1.2)": 27_000,                         # :83-89
    "moment_source_helper(Monodisperse(1,0.5), 1.0, 0.0, 1.2)": 60,                       # :92
    "get_standard_N_q((mono, lognormal, gamma))": 250_000,                                # :94-99
    "integrate_SimpsonEvenFast(90, dx, y)": 1_200,                                        # :106-112
}


_CPUS = None


def _usable_cpus():
    """CPUs this process may really use: the affinity mask capped by the cgroup CPU quota (a pod sees every logical CPU
    of the host in nproc but may be throttled to a fraction of them -- an OpenMP team of nproc threads then runs at a
    few per cent efficiency)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]          # cgroup v2
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())    # cgroup v1
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    return n, quota


def _time_oracle(O, p, mom, out, n_threads, reps=1):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        O.rhs_coal_batch(p, mom, n_threads=n_threads, out=out)
        best = min(best, time.perf_counter() - t0)
    return best


def _cpu_baseline(name, target_seconds=12.0):
    """The C oracle (kind 'port' of the reference algorithm; julia is not installed) on the host cores: a bounded sample
    of the same batch, timed single-threaded and on the thread count that measures fastest (output pre-faulted, threads
    bound to cores), with the parallel efficiency of that team."""
    # libgomp reads these when it is first loaded (the oracle is the first OpenMP user of this process)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    os.environ.setdefault("OMP_DYNAMIC", "false")
    global _CPUS
    if _CPUS is None:
        _CPUS = _usable_cpus()   # before libgomp loads: with OMP_PROC_BIND it pins this thread to the first place
    nproc, quota = _CPUS
    from oracle import cloudy_oracle as O

    p = oracle_params(name)
    n_modes = workload_spec(name)["n_modes"]
    hw = min(O.max_threads(), nproc)
    try:
        import psutil

        phys = psutil.cpu_count(logical=False) or hw
    except Exception:
        phys = hw
    # single thread: ~1.5 s sample
    probe = synth_moments(n_modes, 2000, SEED)
    out = np.zeros_like(probe)
    per1 = max(_time_oracle(O, p, probe, out, 1, reps=2) / probe.shape[1], 1e-9)
    n1 = int(min(max(1.5 / per1, 2000), 4_000_000))
    mom1 = synth_moments(n_modes, n1, SEED)
    out1 = np.zeros_like(mom1)            # pre-faulted: first touch is not in the timed call
    t1 = _time_oracle(O, p, mom1, out1, 1, reps=1)
    rate1 = n1 / t1
    # candidate team sizes (physical cores, logical CPUs, the cgroup quota): short probes, keep the fastest
    # (three candidates at most: the probes are part of the ~30 s the default run spends on CPU baselines)
    cands = sorted({c for c in (hw, min(phys, hw), int(quota) if quota and quota >= 1 else hw) if 1 <= c <= hw})
    pool = synth_moments(n_modes, int(min(max(0.4 * hw * rate1, 4000), 4_000_000)), SEED)   # generated once, tiled below
    probes = {}
    for c in cands:
        n_c = int(min(max(0.4 * c * rate1, 4000), pool.shape[1]))
        mom_c = np.ascontiguousarray(pool[:, :n_c])
        out_c = np.zeros_like(mom_c)
        warm = np.ascontiguousarray(pool[:, :min(max(200 * c, 1000), n_c)])
        _time_oracle(O, p, warm, np.zeros_like(warm), c)   # spawns / resizes the OpenMP team outside the timed call
        probes[c] = n_c / _time_oracle(O, p, mom_c, out_c, c, reps=1)
    # the team the baseline is quoted on: the one with the highest measured throughput (its parallel efficiency is
    # reported beside it as metadata; an oversubscribed team that happens to win is still the fastest this host offers)
    best_c = max(probes, key=probes.get)
    cap = 40_000_000
    try:
        import psutil

        cap = int(min(cap, psutil.virtual_memory().available / (8 * 3 * 8 * 3 * n_modes)))  # 3 arrays, 1/8 of free RAM
    except Exception:
        cap = 20_000_000
    n = int(min(max(target_seconds * probes[best_c], 2000), cap))
    mom = np.ascontiguousarray(np.tile(pool, (1, -(-n // pool.shape[1])))[:, :n])   # the same batch, repeated
    out = np.zeros_like(mom)
    dt = _time_oracle(O, p, mom, out, best_c)
    rate = n / dt
    return dict(value=rate, unit="parcel-RHS/s", cores=best_c, kind="port",
                sample=f"{n} parcels of the {name} batch, oracle/cloudy_oracle.c (C restatement of the Julia "
                       f"reference; julia is not installed), OpenMP x{best_c} bound to cores, output pre-faulted, "
                       f"{dt:.1f} s",
                one_thread={"value": rate1, "unit": "parcel-RHS/s", "sample": f"{n1} parcels, {t1:.1f} s",
                            "us_per_parcel": 1e6 / rate1},
                parallel_efficiency=rate / (best_c * rate1),
                nproc=nproc, physical_cores=phys, cgroup_cpu_quota=quota,
                team_probe_parcels_per_s={str(c): v for c, v in probes.items()},
                reference_ci_ceilings_ns=REFERENCE_CI_CEILINGS_NS,
                reference_ci_ceilings_source="test/unit_tests/performance_tests.jl:66-112 (BenchmarkTools minimum time, "
                                             "1 CPU of the reference's CI; upper bounds, not measurements)")


CLOCK_HZ = 2.4e9          # MI355X peak engine clock (MI355X_MICROARCH.md)
N_SIMD = 256 * 4          # 256 CUs x 4 SIMDs; one wave64 VALU instruction occupies a SIMD's 16 lanes for 4 cycles


class _EventTimer:
    """milliseconds of everything launched on the default stream inside the `with` block, by HIP events recorded on that
    stream (cloudy_timer_begin / cloudy_timer_end)"""

    def __init__(self, pkg):
        self.pkg, self.ms = pkg, None

    def __enter__(self):
        import ctypes as C

        self._t = C.c_void_p()
        self.pkg._lib.check(self.pkg.lib().cloudy_timer_begin(None, C.byref(self._t)))
        return self

    def __exit__(self, *exc):
        import ctypes as C

        ms = C.c_float()
        self.pkg._lib.check(self.pkg.lib().cloudy_timer_end(self._t, None, C.byref(ms)))
        self.ms = float(ms.value)
        return False


def _hbm_roofline(kernel, bytes_per_launch, kernel_ms, measured=None, key=None):
    """HBM roofline block of a streaming variant: algorithmic bytes per launch over the HIP-event launch duration"""
    gbs = bytes_per_launch / (kernel_ms * 1e-3) / 1e9
    out = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
           "kernel": kernel, "kernel_ms": kernel_ms, "algorithmic_bytes_per_launch": bytes_per_launch,
           "traffic_from_profiles": None}
    k = ((measured or {}).get("kernels") or {}).get(key) if key else None
    if k and k.get("hbm_bytes_per_launch"):
        out["traffic_from_profiles"] = k["hbm_bytes_per_launch"]
    return out


def _valu_roofline(measured, key, n_items, kernel_ms):
    """fp64-VALU roofline block of a compute-bound variant: useful fp64 flops per item from the committed rocprofv3
    counters (SQ_INSTS_VALU_{FMA,MUL,ADD}_F64 x 64 x active-lane fraction, tools/summarize_profiles.py) over the kernel
    time measured in this run; None when the committed profile does not hold the kernel."""
    k = (measured.get("kernels") or {}).get(key)
    if not k or not kernel_ms:
        return None
    tf = k["fp64_flops_per_item"] * n_items / (kernel_ms * 1e-3) / 1e12
    # second figure: issued VALU instructions against the issue limit of the SIMDs (a wave64 instruction holds a SIMD for
    # 4 cycles): "0.34 of the FMA peak" next to "0.9 of the issue slots" says the kernel is instruction-count bound
    wave_insts = k["valu_insts_per_item"] * n_items / 64.0
    issue = wave_insts * 4.0 / (N_SIMD * CLOCK_HZ * kernel_ms * 1e-3)
    # the 4-cycles-per-wave64-instruction model holds for the fp64 kernels (0.80 ... 0.96 measured, and
    # SQ_ACTIVE_INST_VALU x 4 / SIMD cycles agrees); the single-precision kernels measure 1.05 ... 1.13 with it -- some of their
    # instructions (transcendental, packed) do not occupy the SIMD for 4 cycles -- so no modelled fraction is reported for them
    single = str(k.get("kernel", "")).endswith(("_f32fast", "_f32"))
    if single or issue > 1.0:
        issue = None
    return {"bound": "fp64-valu", "achieved": tf, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": tf / FP64_VALU_PEAK_TFLOPS, "kernel": k["kernel"], "kernel_ms": kernel_ms,
            "fp64_flops_per_item": k["fp64_flops_per_item"],
            "valu_insts_per_item": k["valu_insts_per_item"], "active_lane_fraction": k["lane_utilisation"],
            "valu_issue_frac": issue,
            "note": "flops / VALU instructions per item and lane utilisation from the committed counter passes "
                    "(profiles/measured_latest.json); kernel time from this run by HIP events; valu_issue_frac = issued "
                    "wave64 VALU instructions x 4 cycles / (1024 SIMDs x 2.4 GHz x kernel time), fp64 kernels only (null for "
                    "single-precision kernels: the 4-cycle model does not hold for them)"}


CFG4Q_PARCELS = 12_500_000


def cfg4q_par(pkg, quad_order=10):
    """BASELINE configs[3] as worded: 3 Gamma modes, HydrodynamicKernelFunction(1e2 pi) (box_gamma_mixture_hydro.jl:22)
    evaluated by a 10-point Gauss rule per distribution (NumericalCoalStyle plan), 9 moments."""
    kf = pkg.get_normalized_kernel_func(pkg.HydrodynamicKernelFunction(1e2 * np.pi), NORMS)
    pd = tuple(pkg.GammaPrimitiveParticleDistribution(1.0, 1.0, 1.0) for _ in range(3))
    return pkg.ODEParameters(pd, None, (3, 3, 3), NORMS, kernel_func=kf, quad_order=quad_order, quad_mode=pkg.QUAD_FIXED)


def _cfg4q_variant(pkg, rank, world, measured, n=CFG4Q_PARCELS, reps=3):
    import ctypes as C

    par = cfg4q_par(pkg)
    plan = pkg.numerical_plan([1, 1, 1], par.kernel_func, NORMS, 10, quad_mode=pkg.QUAD_FIXED)
    mom = synth_moments(3, n, SEED + 1000 * rank)
    m, dm = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(9, n)
    L = pkg.lib()
    for _ in range(2):
        pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, n, m.ptr, dm.ptr, None))
    ms = _event_ms(pkg, plan, m, dm, reps)
    d = dm.to_numpy()[:, :200_000]
    net = d[1] + d[4] + d[7]
    mag = np.abs(d[1]) + np.abs(d[4]) + np.abs(d[7])
    ok = np.isfinite(net)
    out = {"workload": f"cfg4q: {n} parcels/GPU, 3 Gamma modes, hydrodynamic kernel FUNCTION (E = 1e2 pi) by a 10-point "
                       "Gauss rule per distribution (NumericalCoalStyle plan: per-parcel generalised Gauss-Laguerre "
                       "nodes, tensor-product pair sums, weighting_fn split), 9 moments, fp64",
           "value": n * world / (ms * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": ms,
           "kernel": "cloudy_jit_quad_n3q10_hydro_f64" if plan.specialized else "coal_rhs_quad_kernel<3, 2, double>",
           "hbm_GBs": 2 * 9 * 8 * n / (ms * 1e-3) / 1e9,
           "mass_residual_per_parcel_max": float(np.max(np.abs(net[ok]) / np.maximum(mag[ok], 1e-300)))}
    rl = _valu_roofline(measured, "cfg4q", n, ms)
    if rl:
        out["roofline"] = rl
    # BASELINE configs[3] at its FULL size on this one GPU (1e8 parcels = the eight ranks' shards side by side: 7.2 GB in,
    # 7.2 GB out) -- the N = 1 point of the 8-GPU configuration.  (Eight copies of this rank's shard: a 1e8-parcel draw
    # on the host would take a minute; tests/test_gpu_numerical.py runs the eight DIFFERENT shards and checks that each,
    # evaluated alone, equals the same parcels inside the full batch bit for bit.)
    if world == 1 and os.environ.get("CLOUDY_BENCH_SKIP_FULL") != "1":
        try:
            n_full = 8 * n
            mf, df = pkg.DeviceArray(9, n_full), pkg.DeviceArray(9, n_full)
            for g in range(8):
                mf.set_columns(g * n, mom)
            ms_full = _event_ms(pkg, plan, mf, df, 3)
            out["full_1e8_on_one_gpu"] = {"workload": f"configs[3] at its full {n_full} parcels in ONE launch on one GPU",
                                          "value": n_full / (ms_full * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": ms_full,
                                          "ratio_to_8_launches_of_one_shard": ms_full / (8 * ms)}
            del mf, df
        except Exception as e:   # noqa: BLE001 -- e.g. a smaller device: the variant is optional
            out["full_1e8_on_one_gpu"] = {"skipped": f"{type(e).__name__}: {e}"}
    # the Numerical drivers' time stepping fused around this RHS (cloudy_ssprk33_steps, quad_ssprk33_body): one SSPRK33
    # step = 3 evaluations per call, state in registers
    dt_step = 1e-3
    dts = 1e-3 * _sustained_ms(pkg, lambda: pkg._lib.check(
        L.cloudy_ssprk33_steps(plan.handle, n, n, m.ptr, dm.ptr, C.c_double(dt_step), 1, None)), min_reps=reps)
    out["fused_ssprk33"] = {"workload": "cloudy_ssprk33_steps on the same plan and batch: 1 SSPRK33 step (3 RHS evaluations) per call",
                            "value": 3 * n * world / dts, "unit": "parcel-RHS/s", "ms_per_call": 1e3 * dts}
    return out


def _first_call_ms(pkg, make_plan, warm_plan, m, dm):
    """HIP-event time of the FIRST cloudy_coal_rhs call of a fresh converged-mode plan on a batch -- no cost hints yet, the
    workgroups take their parcels in memory order (what a caller pays who re-shards or reshuffles its parcels
    between calls, and what the first call of every plan pays) -- at the sustained clock: `warm_plan` (the same configuration,
    hints in place) runs back to back first."""
    L = pkg.lib()
    n = m.shape[1]
    fresh = make_plan()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_SECONDS:
        pkg._lib.check(L.cloudy_coal_rhs(warm_plan.handle, n, n, m.ptr, dm.ptr, None))
        pkg._lib.check(L.cloudy_stream_synchronize(None))
    with _EventTimer(pkg) as tm:
        pkg._lib.check(L.cloudy_coal_rhs(fresh.handle, n, n, m.ptr, dm.ptr, None))
    return tm.ms


def _cfg4q_converged_variant(pkg, rank, world, measured, fixed_ms, n=CFG4Q_PARCELS, reps=3, q=8):
    """The same batch through a CLOUDY_QUAD_CONVERGED plan (csrc/quad_conv.hpp): the integrals split along the kink of the
    hydrodynamic kernel -- closed forms (incomplete beta) for Q and R, one adaptive Gauss-Kronrod rule per mode for the
    weighting_fn split -- reaching the reference's adaptive quadgk answer to <= 1e-8 of scale (guaranteed; 5.5e-10 measured) where the 10-point rule has
    ~1e-3 (tests/test_numerical_oracle.py).  Reports the cost ratio to the 10-point rule."""
    import ctypes as C

    par = cfg4q_par(pkg)
    plan = pkg.numerical_plan([1, 1, 1], par.kernel_func, NORMS, q, quad_mode=pkg.QUAD_CONVERGED)
    mom = synth_moments(3, n, SEED + 1000 * rank)
    m, dm = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(9, n)
    L = pkg.lib()
    for _ in range(2):
        pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, n, m.ptr, dm.ptr, None))
    ms = _event_ms(pkg, plan, m, dm, reps)
    d = dm.to_numpy()[:, :200_000]
    net = d[1] + d[4] + d[7]
    mag = np.abs(d[1]) + np.abs(d[4]) + np.abs(d[7])
    ok = np.isfinite(net)
    out = {"workload": f"cfg4q_converged: the cfg4q batch ({n} parcels/GPU, 3 Gamma modes, hydrodynamic kernel function) "
                       "in converged mode -- the DEFAULT of the NumericalCoalStyle drop-in: region integrals in closed form, an "
                       "adaptive Gauss-Kronrod (7, 15) rule per mode for the weighting_fn split (panels walked from large sizes "
                       "down, |K15 - G7| <= 1e-7 of the accumulated value, ended by a rigorous bound of what is left), all "
                       "the rules of a parcel walked in one loop; error vs nested "
                       "adaptive quadrature of the reference integrals <= 1e-8 of scale guaranteed, 5.5e-10 measured (10-point rule: 3e-4 ... 1e-2)",
           "value": n * world / (ms * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": ms,
           "kernel": f"cloudy_jit_quad_n3c{q}_hydro_f64" if plan.specialized else "coal_rhs_quad_kernel<3, 2, double, true>",
           "cost_ratio_to_10pt_rule": ms / fixed_ms if fixed_ms else None,
           "hbm_GBs": 2 * 9 * 8 * n / (ms * 1e-3) / 1e9,
           "mass_residual_per_parcel_max": float(np.max(np.abs(net[ok]) / np.maximum(mag[ok], 1e-300)))}
    rl = _valu_roofline(measured, "cfg4q_converged", n, ms)
    if rl:
        out["roofline"] = rl
    out["first_call_ms"] = _first_call_ms(pkg, lambda: pkg.NumericalPlan([1, 1, 1], par.kernel_func, NORMS, q, quad_mode=pkg.QUAD_CONVERGED),
                                          plan, m, dm)
    out["first_call_note"] = ("kernel_ms is the steady state (parcels ranked by the cost each had in the plan's previous call); "
                              "first_call_ms is one call of a fresh plan of the same configuration: no hints, memory order")
    return out



def lognorm_example_moments(n, seed=SEED):
    """Physical moments of n boxes of test/examples/Numerical/n_particles_lognorm.jl:17-24 -- two Lognormal modes, particle
    numbers (1e7, 1e5) per m^3, mass scales (1e-10, 1e-9) kg, sigma = ln 2 -- with the numbers and mass scales of each box drawn
    within a factor 2 of the example's (sigma stays ln 2): get_moments of LognormalPrimitiveParticleDistribution(n, ln m, ln 2),
    M_q = n exp(q mu + q^2 sigma^2 / 2) (ParticleDistributions.jl:193-207)."""
    rng = np.random.Generator(np.random.Philox(key=seed + 77))
    sg2 = np.log(2.0) ** 2
    rows = []
    for n0, m0 in ((1e7, 1e-10), (1e5, 1e-9)):
        nn = n0 * 2.0 ** rng.uniform(-1.0, 1.0, n)
        mu = np.log(m0 * 2.0 ** rng.uniform(-1.0, 1.0, n))
        rows += [nn, nn * np.exp(mu + 0.5 * sg2), nn * np.exp(2.0 * mu + 2.0 * sg2)]
    return np.ascontiguousarray(np.stack(rows))


def _converged_variant(pkg, rank, world, measured, key, dists, kernel_func, mom, what, kname):
    """One NumericalCoalStyle plan in converged mode (the default of the drop-in) on a device-resident batch: HIP-event time of
    cloudy_coal_rhs at the sustained clock, mass residual, fp64-VALU roofline from the committed counter passes."""
    n = mom.shape[1]
    N = len(dists)
    plan = pkg.numerical_plan(dists, pkg.get_normalized_kernel_func(kernel_func, NORMS), NORMS, 8, quad_mode=pkg.QUAD_CONVERGED)
    m, dm = pkg.DeviceArray.from_numpy(mom), pkg.DeviceArray.zeros(3 * N, n)
    L = pkg.lib()
    for _ in range(2):
        pkg._lib.check(L.cloudy_coal_rhs(plan.handle, n, n, m.ptr, dm.ptr, None))
    ms = _event_ms(pkg, plan, m, dm, 3)
    d = dm.to_numpy()[:, :200_000]
    net = sum(d[3 * i + 1] for i in range(N))
    mag = sum(np.abs(d[3 * i + 1]) for i in range(N))
    ok = np.isfinite(net)
    out = {"workload": what, "value": n * world / (ms * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": ms,
           "kernel": kname if plan.specialized else "coal_rhs_quad_kernel<..., true>",
           "hbm_GBs": 2 * 3 * N * 8 * n / (ms * 1e-3) / 1e9,
           "mass_residual_per_parcel_max": float(np.max(np.abs(net[ok]) / np.maximum(mag[ok], 1e-300)))}
    rl = _valu_roofline(measured, key, n, ms)
    if rl:
        out["roofline"] = rl
    kfn = pkg.get_normalized_kernel_func(kernel_func, NORMS)
    out["first_call_ms"] = _first_call_ms(pkg, lambda: pkg.NumericalPlan(dists, kfn, NORMS, 8, quad_mode=pkg.QUAD_CONVERGED), plan, m, dm)
    return out


def _cpu_baseline_cfg4q(n_threads, target_seconds=6.0):
    """The same-rule C oracle (oracle/cloudy_oracle_quad.c) on a bounded sample of the cfg4q batch, on the team size the
    headline baseline found fastest."""
    from oracle import cloudy_oracle as O

    p = O.make_params([O.GAMMA] * 3, np.zeros((1, 1)), (INF, INF, INF), norms=NORMS)
    kf = O.get_normalized_kernel_func(O.kernel_func(O.KF_HYDRODYNAMIC, 1e2 * np.pi), NORMS)
    probe = synth_moments(3, 2000 * n_threads, SEED)
    out = np.zeros_like(probe)
    O.rhs_coal_numerical_batch(p, kf, 10, probe, n_threads=n_threads, out=out)
    t0 = time.perf_counter()
    O.rhs_coal_numerical_batch(p, kf, 10, probe, n_threads=n_threads, out=out)
    per = max((time.perf_counter() - t0) / probe.shape[1], 1e-9)
    n = int(min(max(target_seconds / per, 2000), 20_000_000))
    mom = synth_moments(3, n, SEED)
    out = np.zeros_like(mom)
    t0 = time.perf_counter()
    O.rhs_coal_numerical_batch(p, kf, 10, mom, n_threads=n_threads, out=out)
    dt = time.perf_counter() - t0
    return dict(value=n / dt, unit="parcel-RHS/s", cores=n_threads, kind="port",
                sample=f"{n} parcels of the cfg4q batch, oracle/cloudy_oracle_quad.c (the reference's NumericalCoalStyle "
                       f"structure with the same fixed 10-point rule; the reference's adaptive quadgk is ~1e3 x more "
                       f"density evaluations), OpenMP x{n_threads}, {dt:.1f} s")


def _cpu_baseline_cfg4q_converged(n_threads, target_seconds=6.0, reference_parcel=True):
    """cpu_baseline of the converged variant: the same-rule C oracle (oracle/cloudy_oracle_quad.c, closed forms + the
    adaptive Gauss-Kronrod rule at the kernels' tolerance) on a bounded sample of the cfg4q batch on the host cores -- and,
    as context, ONE parcel through oracle/cloudy_oracle_adaptive.c at rtol = 1e-8: the reference's actual algorithm for this
    style (nested adaptive quadgk of the integrands of Coalescence.jl:644-708), which takes seconds per parcel."""
    from oracle import cloudy_oracle as O

    p = O.make_params([O.GAMMA] * 3, np.zeros((1, 1)), (INF, INF, INF), norms=NORMS)
    kf = O.get_normalized_kernel_func(O.kernel_func(O.KF_HYDRODYNAMIC, 1e2 * np.pi), NORMS)
    probe = synth_moments(3, 500 * n_threads, SEED)
    out = np.zeros_like(probe)
    O.rhs_coal_numerical_converged_batch(p, kf, 8, probe, n_threads=n_threads, out=out)
    t0 = time.perf_counter()
    O.rhs_coal_numerical_converged_batch(p, kf, 8, probe, n_threads=n_threads, out=out)
    per = max((time.perf_counter() - t0) / probe.shape[1], 1e-9)
    n = int(min(max(target_seconds / per, 500), 5_000_000))
    mom = synth_moments(3, n, SEED)
    out = np.zeros_like(mom)
    t0 = time.perf_counter()
    O.rhs_coal_numerical_converged_batch(p, kf, 8, mom, n_threads=n_threads, out=out)
    dt = time.perf_counter() - t0
    # the reference's own algorithm on one ordinary parcel of the batch (all shapes in [1.5, 8]; smaller shapes take minutes)
    t_ref = None
    if reference_parcel:
        ntk = O.update_dist_batch(p, mom[:, :200])
        i = next((j for j in range(ntk.shape[1]) if all(1.5 <= ntk[3 * m + 2, j] <= 8 for m in range(3))), 0)
        pd = [O.make_dist(O.GAMMA, ntk[3 * m, i], ntk[3 * m + 1, i], ntk[3 * m + 2, i]) for m in range(3)]
        kfn = O.kernel_func(O.KF_HYDRODYNAMIC, kf.p[0])
        t0 = time.perf_counter()
        O.get_coal_ints_numerical_adaptive(pd, kfn, 1e-8, 1e-8)
        t_ref = time.perf_counter() - t0
    return dict(value=n / dt, unit="parcel-RHS/s", cores=n_threads, kind="port",
                sample=f"{n} parcels of the cfg4q batch, oracle/cloudy_oracle_quad.c in converged mode (the same rule as the "
                       f"kernel: closed forms + adaptive Gauss-Kronrod at tolerance {O.CONV_TOL:g}), OpenMP x{n_threads}, {dt:.1f} s",
                reference_algorithm_seconds_per_parcel=t_ref,
                reference_algorithm_note="ONE parcel of the batch through oracle/cloudy_oracle_adaptive.c at rtol = 1e-8, one "
                                         "thread: the reference's own algorithm for NumericalCoalStyle (nested adaptive "
                                         "quadgk of Coalescence.jl:644-708, ~1e5 density evaluations per integral); measured "
                                         "4-9 s per parcel in round 4; timed only with --all-cpu-baselines")


def _kernel_label(plan, n_modes, P):
    """Name of the kernel behind cloudy_coal_rhs for this plan, as rocprofv3 shows it (jit.hpp: jit_suffix)."""
    sfx = f"_n{n_modes}p{P}_f64"
    if plan.all_inf:
        return ("cloudy_jit_allinf2" + sfx + " (coal_rhs_allinf2_body compiled for this plan at plan creation)"
                if plan.specialized else f"coal_rhs_allinf2_kernel<{n_modes}, {P}, double>")
    return ("cloudy_jit_sorted" + sfx + " (coal_rhs_sorted_body compiled for this plan at plan creation)"
            if plan.specialized else f"coal_rhs_sorted_kernel<{n_modes}, {P}, ...>")


def _headline_roofline(workload, plan, n_local, nmom, event_ms, per_rank_ms, traffic, measured):
    """HBM roofline for plans whose thresholds are all Inf (the kernel streams 2 x nmom x 8 B per parcel and does
    ~300 VALU instructions on it); fp64-VALU roofline for plans with a Simpson pass (13-33 k VALU instructions per
    parcel: the HBM fraction of such a kernel says nothing)."""
    bytes_per_launch = 2 * nmom * 8 * n_local
    label = _kernel_label(plan, plan.n_modes, plan.tensor_p)
    hbm = lambda ms: bytes_per_launch / (ms * 1e-3) / 1e9
    if plan.all_inf:
        a = hbm(event_ms)
        return {"bound": "hbm", "achieved": a, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": a / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": "2 x FETCH_SIZE + WRITE_SIZE of this kernel at this batch size from the committed rocprofv3 "
                                  "--pmc passes (profiles/measured_latest.json); not collected in this run",
                "kernel": label, "kernel_ms": event_ms,
                "algorithmic_bytes_per_launch": bytes_per_launch,
                "per_rank": [{"rank": r, "kernel_ms": ms, "achieved": hbm(ms), "frac": hbm(ms) / HBM_PEAK_GBS}
                             for r, ms in enumerate(per_rank_ms)]}
    flops = measured.get(f"{workload}_fp64_flops_per_parcel")
    if flops is None and workload == "cfg3b" and measured.get("cfg3b_fp64_flops_per_launch"):
        flops = measured["cfg3b_fp64_flops_per_launch"] / measured["n_parcels"]
    tf = (lambda ms: flops * n_local / (ms * 1e-3) / 1e12) if flops else (lambda ms: None)
    a = tf(event_ms)
    return {"bound": "fp64-valu", "achieved": a, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": a / FP64_VALU_PEAK_TFLOPS if a else None, "traffic": None, "kernel": label, "kernel_ms": event_ms,
            "fp64_flops_per_parcel": flops, "hbm_GBs": hbm(event_ms),
            "note": "fp64 flops per parcel from the committed SQ_INSTS_VALU_{FMA,MUL,ADD}_F64 counters x active-lane "
                    "fraction (profiles/measured_latest.json)",
            "per_rank": [{"rank": r, "kernel_ms": ms, "achieved": tf(ms),
                          "frac": tf(ms) / FP64_VALU_PEAK_TFLOPS if flops else None} for r, ms in enumerate(per_rank_ms)]}



# ------------------------------------------------------------------------------------------------
# The contract line.  VERDICT r4: the round-4 line had grown to 20 KB (19 prose-heavy variant objects) and the driver could
# no longer parse it.  The LAST stdout line is now a compact strict-JSON object (<= 4 KB, no NaN/Infinity); everything else
# -- the full variant objects with their workload descriptions, rooflines and baselines -- goes to a side file
# (bench_variants.json beside this script, named in the line) and to stderr.
# ------------------------------------------------------------------------------------------------
LINE_LIMIT = 4096
VARIANTS_FILE = "bench_variants.json"


def _finite(x):
    """strict JSON: non-finite floats become null, numpy scalars become Python numbers (recursively)"""
    if isinstance(x, dict):
        return {str(k): _finite(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_finite(v) for v in x]
    if isinstance(x, (np.floating, float)):
        x = float(x)
        return x if np.isfinite(x) else None
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.bool_,)):
        return bool(x)
    return x


def _sig(x, digits=6):
    """numbers of the compact line carry 6 significant digits"""
    if isinstance(x, float):
        return float(f"{x:.{digits}g}") if np.isfinite(x) else None
    return x


def _clip(s, n):
    s = "" if s is None else str(s)
    return s if len(s) <= n else s[: n - 3] + "..."


def compact_line(full, variants_file=VARIANTS_FILE):
    """The one contract line from the full result object: headline keys, a trimmed roofline / cpu_baseline, and per
    variant only {value, kernel_ms, frac}.  Pure function of `full` (tests/test_host_abi.py runs it on canned numbers)."""
    full = _finite(full)
    rl = full.get("roofline") or {}
    roof = {k: _sig(rl.get(k)) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic")}
    roof["kernel"] = _clip((rl.get("kernel") or "").split(" ")[0], 64)
    roof["kernel_ms"] = _sig(rl.get("kernel_ms"))
    if rl.get("algorithmic_bytes_per_launch") is not None:
        roof["algorithmic_bytes_per_launch"] = rl["algorithmic_bytes_per_launch"]
    if rl.get("per_rank"):     # the slowest rank must be visible in a SCALE record: one kernel_ms per rank, rank order
        roof["per_rank_kernel_ms"] = [_sig(r.get("kernel_ms"), 5) for r in rl["per_rank"]]
    cb = full.get("cpu_baseline")
    cpu = None
    if cb:
        cpu = {"value": _sig(cb.get("value")), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
               "sample": _clip(cb.get("sample"), 200)}
        if cb.get("one_thread"):
            cpu["one_thread_value"] = _sig(cb["one_thread"].get("value"))
    cfg = full.get("config") or {}
    variants = {}
    for name, v in (full.get("variants") or {}).items():
        r = v.get("roofline") or {}
        e = {"value": _sig(v.get("value")), "kernel_ms": _sig(v.get("kernel_ms", v.get("ms_per_call")), 5),
             "frac": _sig(r.get("frac"), 4)}
        if v.get("unit") not in (None, "parcel-RHS/s"):
            e["unit"] = v["unit"]
        if v.get("first_call_ms") is not None:   # converged-mode plans: the hint-less first call beside the steady state
            e["first_call_ms"] = _sig(v["first_call_ms"], 5)
        variants[name] = e
    line = {
        "metric": full.get("metric"), "value": _sig(full.get("value"), 8), "unit": full.get("unit"),
        "n_gpus": full.get("n_gpus"), "steps": full.get("steps"), "warmup": full.get("warmup"),
        "ms_per_step": _sig(full.get("ms_per_step"), 8), "higher_is_better": full.get("higher_is_better", True),
        "scaling": full.get("scaling"), "vs_baseline": full.get("vs_baseline"), "dtype": full.get("dtype"),
        "data": full.get("data"),
        "config": {"workload": _clip(cfg.get("workload"), 260), "parcels_per_gpu": cfg.get("parcels_per_gpu"),
                   "global_parcels": cfg.get("global_parcels"), "sharding": _clip(cfg.get("sharding"), 60)},
        "roofline": roof, "cpu_baseline": cpu,
        "collective": _clip(full.get("collective"), 200), "collective_fallback": bool(full.get("collective_fallback")),
        "mass_rate_residual": _sig(full.get("mass_rate_residual"), 4),
        "variants": variants, "variants_file": variants_file,
        "process_wall_s": {k: _sig(v, 4) for k, v in (full.get("process_wall_s") or {}).items()},
    }
    if "launch" in cfg:
        line["config"]["launch"] = _clip(cfg["launch"], 120)
    prd = full.get("per_rank_devices")
    if prd and (full.get("n_gpus") or 1) > 1:   # a SCALE record shows which devices the ranks ran on (rank order)
        line["devices"] = [_clip(d.get("pci_bus_id"), 16) if d.get("pci_bus_id") else None for d in prd]
        line["distinct_devices"] = full.get("distinct_devices")
        if full.get("ranks_share_a_gpu"):
            line["ranks_share_a_gpu"] = True
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    # a last guard: drop the optional parts, widest first, rather than print a line the driver cannot parse
    for drop in ("process_wall_s", "devices", "variants"):
        if len(text) <= LINE_LIMIT:
            break
        line.pop(drop, None)
        text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    if len(text) > LINE_LIMIT:
        raise ValueError(f"bench line is {len(text)} bytes (> {LINE_LIMIT})")
    return text


def emit(full, json_out, side_file=True):
    """full object -> side file + stderr; the compact line -> the real stdout, last."""
    full = _finite(full)
    path = os.path.join(ROOT, VARIANTS_FILE) if side_file else os.devnull
    try:
        with open(path, "w") as f:
            json.dump(full, f, indent=1, allow_nan=False)
            f.write("\n")
    except OSError as e:   # a read-only checkout: the line still goes out
        print(f"bench.py: could not write {path}: {e}", file=sys.stderr)
    print("bench.py full result" + (" (also in " + VARIANTS_FILE + ")" if side_file else "") + ":\n"
          + json.dumps(full, allow_nan=False), file=sys.stderr)
    sys.stderr.flush()
    json_out.write(compact_line(full, VARIANTS_FILE if side_file else None) + "\n")
    json_out.flush()


def _one_process(args):
    """`python bench.py --one-process --gpus N`: ONE process drives the N visible GPUs -- the pattern a single Julia process
    uses -- instead of one rank per GPU: a plan, a state and a tendency array per device, the launches of a
    step issued device after device (they run concurrently: each on its own device's NULL stream) and awaited together; the
    conservation sums through cloudy_comm_create_all (ncclCommInitAll inside libcloudy_hip.so) with the per-device
    cloudy_moment_sums_allreduce calls bracketed by cloudy_comm_group_start / _end.  Weak scaling as the ranked run: every
    GPU owns the full per-GPU batch.  (the driver's scaling sweep uses the ranked launch.)"""
    import ctypes as C

    import __graft_entry__ as ge

    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)          # RCCL's banner goes to stderr, the line stays alone on stdout
    pkg = ge.load_package()
    L = pkg.lib()
    N = args.gpus
    if pkg.device_count() < N:
        raise SystemExit(f"--one-process --gpus {N}: only {pkg.device_count()} HIP device(s) visible")
    spec = workload_spec(args.workload)
    n = args.parcels or spec["default_parcels"]
    devs = []
    for g in range(N):
        pkg._lib.check(L.cloudy_set_device(g))
        wl = make_workload(args.workload, n, seed=SEED + 1000 * g)
        plan = pkg.Plan([1] * spec["n_modes"], kernel_matrix(spec), spec["thresholds"], NORMS,
                        pkg.MovingThreshold() if spec.get("moving") else pkg.FixedThreshold(), device=g)
        devs.append(dict(plan=plan, m=pkg.DeviceArray.from_numpy(wl["mom"]), dm=pkg.DeviceArray.zeros(*wl["mom"].shape),
                         sums=pkg.DeviceArray(plan.nmom, 1)))
    nmom = devs[0]["plan"].nmom

    def step():
        for g, d in enumerate(devs):
            pkg._lib.check(L.cloudy_coal_rhs(d["plan"].handle, n, n, d["m"].ptr, d["dm"].ptr, None))

    def sync_all():
        for g in range(N):
            pkg._lib.check(L.cloudy_set_device(g))
            pkg._lib.check(L.cloudy_stream_synchronize(None))

    t0 = time.perf_counter()
    done = 0
    while done < max(args.warmup, 1) or time.perf_counter() - t0 < WARM_SECONDS:
        step()
        done += 1
        if done % 8 == 0:
            sync_all()
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync_all()
    wall = time.perf_counter() - t0
    # the one collective of the path, from one thread driving N communicators
    comms = (C.c_void_p * N)()
    pkg._lib.check(L.cloudy_comm_create_all(N, None, comms))
    pkg._lib.check(L.cloudy_comm_group_start())
    for g, d in enumerate(devs):
        pkg._lib.check(L.cloudy_moment_sums_allreduce(d["plan"].handle, comms[g], n, n, nmom, d["dm"].ptr, d["sums"].ptr, None))
    pkg._lib.check(L.cloudy_comm_group_end())
    sync_all()
    gs = [d["sums"].to_numpy().reshape(-1) for d in devs]
    assert all(np.array_equal(gs[0], x) for x in gs), "the all-reduced sums differ between devices"
    for g in range(N):
        L.cloudy_comm_destroy(comms[g])
    v = pkg.lib().cloudy_comm_rccl_version()
    np_modes = [3] * spec["n_modes"]
    mass = sum(gs[0][3 * k + 1] for k in range(spec["n_modes"]))
    gross = sum(abs(gs[0][3 * k + 1]) for k in range(spec["n_modes"]))
    out = {"metric": "parcel moment-RHS evals/sec at 1e7 parcels; achieved HBM GB/s vs 8 TB/s peak",
           "value": n * N * args.steps / wall, "unit": "parcel-RHS/s", "n_gpus": N, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": 1e3 * wall / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f64", "data": "synthetic",
           "config": {"workload": f"{args.workload}: {n} parcels/GPU", "global_parcels": n * N,
                      "launch": "ONE process driving all GPUs (cloudy_comm_create_all + cloudy_comm_group_start/_end)"},
           "collective": f"ncclAllReduce(sum, f64, {nmom}) per device inside one group, RCCL {v // 10000}.{v // 100 % 100}.{v % 100}, {N} device(s)",
           "mass_rate_residual": abs(mass) / max(gross, 1e-300), "np_modes": np_modes}
    if args.dump_outputs:   # device 0's tendencies of the last timed step (the all-reduce above only reads them)
        pkg._lib.check(L.cloudy_set_device(0))
        _dump_outputs(args.dump_outputs, devs[0]["dm"])
    emit(out, json_out)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--parcels", type=int, default=0, help="parcels per GPU (default: the workload's size)")
    ap.add_argument("--workload", default="cfg3a")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the tendencies of the last timed step to DIR/dm.npy (a fixed sample of large batches)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: HIP-event kernel times and rooflines, the "
                         "conservation diagnostic through the RCCL communicator, the variants and the CPU baselines")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full) skip the CPU baselines")
    ap.add_argument("--no-variants", action="store_true", help="(with --full) skip the variants")
    ap.add_argument("--all-cpu-baselines", action="store_true",
                    help="(with --full) also time the cfg3b and cfg4q (10-point rule) oracles and one parcel of the reference's "
                         "own nested quadgk algorithm (--full alone times the headline + the converged-mode baseline: ~30 s of CPU)")
    ap.add_argument("--one-process", action="store_true",
                    help="one process drives all --gpus devices (cloudy_comm_create_all) instead of one rank per GPU")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.one_process:
        return _one_process(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _spawn_ranks(args.gpus, sys.argv[1:])   # before anything touches the GPU
    if int(os.environ.get("WORLD_SIZE", "1")) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={os.environ.get('WORLD_SIZE', '1')}: launch one rank per GPU")

    t_start = time.perf_counter()
    # The contract is ONE JSON line on stdout.  RCCL prints a version banner to the C-level stdout when a communicator is
    # formed (ours, or torch's nccl backend): keep a private handle on the real stdout for the line and point fd 1 at
    # stderr for everything else this process and its libraries print.
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    rank, world, local_rank, dist, torch = _dist_setup(args.gpus)
    if dist is not None and os.environ.get("CLOUDY_BENCH_DRY_CONTROL_PLANE") == "1":
        rc = _dry_control_plane(args, rank, world, dist, torch, json_out)
        _rank_done()
        return rc
    import __graft_entry__ as ge

    pkg = ge.load_package()
    if pkg.device_count() < 1:
        raise SystemExit("bench.py needs a HIP device: the coalescence RHS has no CPU fallback")
    pkg._lib.check(pkg.lib().cloudy_set_device(local_rank))
    _fault("before_barrier", rank)
    if args.full:   # the communicator serves the conservation diagnostic only: the timed path has no collective
        _comm_setup(pkg, world, local_rank, dist, torch)

    spec = workload_spec(args.workload)
    n_local = args.parcels or spec["default_parcels"]
    res = _run_workload(pkg, args.workload, n_local, args.steps, args.warmup, rank, dist, torch, full=args.full,
                        dump_dir=args.dump_outputs if rank == 0 else None)
    t_headline = time.perf_counter()
    nmom = res["nmom"]
    bytes_per_eval = 2 * nmom * 8  # read nmom moments + write nmom tendencies, fp64
    total = n_local * world
    value = total * args.steps / res["wall"]
    # which device each rank ran on -- a SCALE record must show N distinct devices
    import ctypes as _C

    _bus = _C.create_string_buffer(64)
    _rc = pkg.lib().cloudy_device_pci_bus_id(local_rank, _bus, 64)
    per_rank_dev = _gather_objects({"rank": rank, "pid": os.getpid(), "device": local_rank,
                                    "pci_bus_id": _bus.value.decode() if _rc == 0 else None,
                                    "kernel_ms": res.get("event_ms")}, dist)
    if not args.full:
        return _plain_result(args, rank, world, dist, json_out, spec, n_local, nmom, value, res, per_rank_dev,
                             t_start, t_headline)
    achieved = bytes_per_eval * n_local / (res["event_ms"] * 1e-3) / 1e9
    per_rank_ms = _gather(res["event_ms"], dist, torch)   # every rank's HIP-event average of its own launches

    measured = _measured_latest()
    traffic = None
    # 2 x FETCH_SIZE + WRITE_SIZE of the committed PMC passes -- quoted only for the batch size AND the kernel sources they were
    # collected on (a changed kernel must not print last round's bytes): cloudy_source_hash(1) = FNV-1a of
    # kernels.hpp + device_math.hpp + the all-Inf body inside the library, recorded by tools/summarize_profiles.py
    src_hash = f"{pkg.lib().cloudy_source_hash(1):016x}"
    traffic_note = None
    if args.workload == "cfg3a" and measured.get("n_parcels") == n_local:
        if measured.get("source_hash_allinf") == src_hash:
            traffic = measured.get("cfg3a_hbm_bytes_per_launch")
        else:
            traffic_note = (f"null: profiles/measured_latest.json was collected on kernel sources {measured.get('source_hash_allinf')}, "
                            f"this library holds {src_hash}")

    variants = {}
    # multi-rank runs (the driver's scaling sweep) time the headline and the threshold workload only; the other variants
    # are single-GPU characterisations and run at N = 1
    more_variants = not args.no_variants and args.workload == "cfg3a" and world == 1
    if not args.no_variants and args.workload == "cfg3a":
        v = _run_workload(pkg, "cfg3b", n_local, max(3, args.steps // 10), 1, rank, dist, torch)
        v_steps = max(3, args.steps // 10)
        variants["cfg3b"] = {
            "workload": "same batch, thresholds (5e-10 kg, Inf): Simpson / incomplete-gamma path "
                        "(box_gamma_mixture_long.jl:36); fp64-VALU bound, not HBM bound",
            "value": n_local * world * v_steps / v["wall"], "unit": "parcel-RHS/s",
            "ms_per_step": 1e3 * v["wall"] / v_steps, "kernel_ms": v["event_ms"],
            "hbm_GBs": bytes_per_eval * n_local / (v["event_ms"] * 1e-3) / 1e9,
            "mass_rate_residual": abs(v["mass_rate_sum"]) / max(v["mass_rate_gross"], 1e-300) if rank == 0 else None,
            "mass_residual_per_parcel_max": v["mass_per_parcel"],
        }
        rl = _valu_roofline(measured, "cfg3b", n_local, v["event_ms"])
        if rl:
            variants["cfg3b"]["roofline"] = rl
        elif measured.get("n_parcels") == n_local and measured.get("cfg3b_fp64_flops_per_launch"):
            tf = measured["cfg3b_fp64_flops_per_launch"] / (v["event_ms"] * 1e-3) / 1e12
            variants["cfg3b"]["roofline"] = {
                "bound": "fp64-valu", "achieved": tf, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": tf / FP64_VALU_PEAK_TFLOPS,
                "note": "fp64 flops per launch from the committed SQ_INSTS_VALU_{FMA,MUL,ADD}_F64 counters x active-lane "
                        "fraction (profiles/measured_latest.json); not HBM bound"}

    if more_variants:
        # fused on-device SSPRK33 (cloudy_ssprk33_steps): 3 RHS evaluations per step, state in registers
        import ctypes as C

        wl = res["wl"]
        plan = res["plan"]
        u = pkg.DeviceArray.from_numpy(wl["mom"])
        L = pkg.lib()
        n_steps, dt = 4, 1e-3
        dts = 1e-3 * _sustained_ms(pkg, lambda: pkg._lib.check(
            L.cloudy_ssprk33_steps(plan.handle, n_local, n_local, u.ptr, u.ptr, C.c_double(dt), n_steps, None)))
        variants["cfg3a_fused_ssprk33"] = {
            "workload": f"cloudy_ssprk33_steps: {n_steps} SSPRK33 steps per call (3 RHS evaluations each) with the state "
                        "in registers; one read + one write of the state per call",
            "value": 3 * n_steps * n_local * world / dts, "unit": "parcel-RHS/s", "ms_per_call": 1e3 * dts,
            "hbm_GBs": bytes_per_eval * n_local / dts / 1e9,
        }
        rl = _valu_roofline(measured, "cfg3a_fused_ssprk33", n_local, 1e3 * dts)   # flops per parcel per CALL (12 evaluations)
        if rl:
            variants["cfg3a_fused_ssprk33"]["roofline"] = rl

    if more_variants:
        # BASELINE configs[0] as worded -- "Golovin kernel, 3 prognostic moments, CPU Tsit5" -- as a batch: cloudy_tsit5_steps
        # (the Tsit5 tableau with the caller's fixed dt, 6 RHS evaluations per step, state and stage derivatives in registers)
        # on 1e7 single-mode Golovin boxes, the kernel compiled for the plan on the first call (cloudy_jit_tsit5_n1p2_f64)
        import ctypes as C

        n0, steps0 = 10_000_000, 4
        wl0 = make_workload("cfg2", n0, seed=SEED + 1000 * rank)
        plan0 = wl0["coal_data"].plan(wl0["dist_types"])
        u0 = pkg.DeviceArray.from_numpy(wl0["mom"])
        o0 = pkg.DeviceArray.zeros(*wl0["mom"].shape)
        ms0 = _sustained_ms(pkg, lambda: pkg._lib.check(
            pkg.lib().cloudy_tsit5_steps(plan0.handle, n0, n0, u0.ptr, o0.ptr, C.c_double(1e-3), steps0, None)))
        evals0 = 6 * steps0 + 1
        variants["cfg0_tsit5"] = {
            "workload": f"cloudy_tsit5_steps: {n0} single-mode Golovin boxes (the cfg2 plan), {steps0} fixed Tsit5 steps per call "
                        f"= {evals0} RHS evaluations, one read + one write of the state per call",
            "value": evals0 * n0 * world / (ms0 * 1e-3), "unit": "parcel-RHS/s", "ms_per_call": ms0,
            "kernel": "cloudy_jit_tsit5_n1p2_f64" if plan0.specialized else "tsit5_kernel<1, 2, 0, double>",
            "hbm_GBs": 2 * plan0.nmom * 8 * n0 / (ms0 * 1e-3) / 1e9,
        }
        rl = _valu_roofline(measured, "cfg0_tsit5", n0, ms0)   # flops per parcel per CALL
        if rl:
            variants["cfg0_tsit5"]["roofline"] = rl
        del u0, o0

    if more_variants:
        # the same launches with the ahead-of-time kernels (desc.specialize = -1): plan constants from kernel arguments,
        # dense tensors -- what every plan falls back to when hiprtc is unavailable
        wl = res["wl"]
        plan_aot = wl["coal_data"].plan(wl["dist_types"], specialize=-1)
        m_a = pkg.DeviceArray.from_numpy(wl["mom"])
        dm_a = pkg.DeviceArray.zeros(nmom, n_local)
        for _ in range(50):
            pkg._lib.check(pkg.lib().cloudy_coal_rhs(plan_aot.handle, n_local, n_local, m_a.ptr, dm_a.ptr, None))
        ms_a = _event_ms(pkg, plan_aot, m_a, dm_a, args.steps)
        variants["cfg3a_aot_kernels"] = {
            "workload": "cfg3a through coal_rhs_allinf2_kernel<2, 3, double> (no plan-time specialisation)",
            "value": n_local * world / (ms_a * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": ms_a,
            "hbm_GBs": bytes_per_eval * n_local / (ms_a * 1e-3) / 1e9,
            "headline_plan_specialized": bool(res["plan"].specialized),
            "roofline": _hbm_roofline("coal_rhs_allinf2_kernel<2, 3, double>", bytes_per_eval * n_local, ms_a, measured,
                                      "cfg3a_aot_kernels"),
        }
        del m_a, dm_a

    if more_variants:
        # CLOUDY_F32 plan: float planes in HBM (48 B per evaluation), fp64 arithmetic in registers
        wl = res["wl"]
        plan32 = wl["coal_data"].plan(wl["dist_types"], dtype=1)
        m32 = pkg.DeviceArray.from_numpy(wl["mom"].astype(np.float32))
        dm32 = pkg.DeviceArray.zeros(nmom, n_local, np.float32)
        for _ in range(3):
            pkg._lib.check(pkg.lib().cloudy_coal_rhs(plan32.handle, n_local, n_local, m32.ptr, dm32.ptr, None))
        ms32 = _event_ms(pkg, plan32, m32, dm32, args.steps)
        variants["cfg3a_f32_planes"] = {
            "workload": "cfg3a with CLOUDY_F32 planes (float in HBM, fp64 arithmetic): BASELINE configs[4] fp32 path",
            "value": n_local * world / (ms32 * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": ms32,
            "hbm_GBs": 2 * nmom * 4 * n_local / (ms32 * 1e-3) / 1e9,
            "roofline": _hbm_roofline("cloudy_jit_allinf2_n2p3_f32", 2 * nmom * 4 * n_local, ms32, measured, "cfg3a_f32_planes"),
        }
        # CLOUDY_F32_FAST on the headline plan: float planes AND packed single-precision arithmetic (csrc/allinf_f32.hpp)
        planp = wl["coal_data"].plan(wl["dist_types"], dtype=2)
        msp = _event_ms(pkg, planp, m32, dm32, args.steps)
        variants["cfg3a_f32_fast_packed"] = {
            "workload": "cfg3a with CLOUDY_F32_FAST: float planes and packed single-precision arithmetic (v_pk_fma_f32, four "
                        "parcels per lane); error vs the fp64 oracle reported in tests/test_gpu_parity.py",
            "value": n_local * world / (msp * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": msp,
            "hbm_GBs": 2 * nmom * 4 * n_local / (msp * 1e-3) / 1e9,
            "roofline": _hbm_roofline("cloudy_jit_allinf4_n2p3_f32fast", 2 * nmom * 4 * n_local, msp, measured, "cfg3a_f32_fast_packed"),
        }
        # CLOUDY_F32_FAST on the threshold workload (single-precision Simpson / incomplete-gamma pass)
        wlb = make_workload("cfg3b", n_local, seed=SEED + 1000 * rank)
        planf = wlb["coal_data"].plan(wlb["dist_types"], dtype=2)
        for _ in range(3):
            pkg._lib.check(pkg.lib().cloudy_coal_rhs(planf.handle, n_local, n_local, m32.ptr, dm32.ptr, None))
        msf = _event_ms(pkg, planf, m32, dm32, max(3, args.steps // 10))
        variants["cfg3b_f32_fast"] = {
            "workload": "cfg3b with CLOUDY_F32_FAST: float planes, single-precision arithmetic in the per-node "
                        "Simpson / incomplete-gamma pass (error vs the fp64 oracle bounded at 5e-6 of the term scale "
                        "in tests/test_gpu_parity.py)",
            "value": n_local * world / (msf * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": msf,
        }
        rl = _valu_roofline(measured, "cfg3b_f32_fast", n_local, msf)
        if rl:
            variants["cfg3b_f32_fast"]["roofline"] = rl
        del m32, dm32

    if more_variants:
        # the other BASELINE configurations, a few launches each
        for vname, vn in (("cfg2", 1_000_000), ("cfg4", 12_500_000), ("moving4", 2_500_000)):
            wlv = make_workload(vname, vn, seed=SEED + 1000 * rank)
            planv = wlv["coal_data"].plan(wlv["dist_types"])
            mv = pkg.DeviceArray.from_numpy(wlv["mom"])
            dmv = pkg.DeviceArray.zeros(planv.nmom, vn)
            reps = 200 if vname == "cfg2" else 3
            for _ in range(200 if vname == "cfg2" else 3):
                pkg._lib.check(pkg.lib().cloudy_coal_rhs(planv.handle, vn, vn, mv.ptr, dmv.ptr, None))
            msv = _event_ms(pkg, planv, mv, dmv, reps)
            spv = workload_spec(vname)
            variants[vname] = {
                "workload": f"{vname}: {vn} parcels/GPU, {spv['n_modes']} Gamma mode(s), kernel {spv['kernel']}, "
                            f"{'MovingThreshold percentiles' if spv.get('moving') else 'thresholds'} "
                            f"{spv['thresholds']}, {planv.nmom} moments, fp64",
                "value": vn * world / (msv * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": msv,
                "hbm_GBs": 2 * planv.nmom * 8 * vn / (msv * 1e-3) / 1e9,
            }
            rl = _valu_roofline(measured, vname, vn, msv)
            if vname == "cfg2":
                # thresholds Inf: streaming, 48 B per parcel -- but the 48 MB working set of 1e6 parcels stays in the 256 MB
                # Infinity Cache between launches: NOT an HBM measurement, so no fraction of the HBM peak
                rl = _hbm_roofline(_kernel_label(planv, 1, 2).split(" ")[0], 2 * planv.nmom * 8 * vn, msv, measured, "cfg2")
                rl.update({"bound": "infinity-cache", "frac": None, "peak": None,
                           "note": "working set (48 MB) resident in the 256 MB Infinity Cache: `achieved` is cache bandwidth, no HBM fraction"})
            if rl:
                variants[vname]["roofline"] = rl
            del mv, dmv

    if more_variants:
        # CLOUDY_F64_RELAXED (opt-in): fp64 planes and arithmetic, the incomplete-gamma series / continued fraction of the
        # threshold kernels stopped at 1e-11 (<= 1e-9 of scale against the oracle: tests/test_gpu_parity.py)
        for vname, vn in (("cfg3b", n_local), ("cfg4", 12_500_000)):
            wlv = make_workload(vname, vn, seed=SEED + 1000 * rank)
            planv = wlv["coal_data"].plan(wlv["dist_types"], dtype=3)
            mv = pkg.DeviceArray.from_numpy(wlv["mom"])
            dmv = pkg.DeviceArray.zeros(planv.nmom, vn)
            msv = _event_ms(pkg, planv, mv, dmv, 3)
            variants[vname + "_f64_relaxed"] = {
                "workload": f"{vname} with CLOUDY_F64_RELAXED (series / continued fraction of P(a, z) cut at 1e-11)",
                "value": vn * world / (msv * 1e-3), "unit": "parcel-RHS/s", "kernel_ms": msv,
                "speedup_vs_default_dtype": (variants[vname]["kernel_ms"] / msv) if vname in variants and "kernel_ms" in variants[vname] else None,
            }
            rl = _valu_roofline(measured, vname + "_f64_relaxed", vn, msv)
            if rl:
                variants[vname + "_f64_relaxed"]["roofline"] = rl
            del mv, dmv

    if more_variants:
        # BASELINE configs[4]: Long's kernel pieces (cfg3b thresholds) + sedimentation flux, float planes
        n5 = 12_500_000
        wl5 = make_workload("cfg3b", n5, seed=SEED + 1000 * rank)
        vel = ((50.0, 1.0 / 6),)   # rainshaft_gamma_mixture.jl:44
        m5 = pkg.DeviceArray.from_numpy(wl5["mom"].astype(np.float32))
        cs5, sf5 = pkg.DeviceArray.zeros(nmom, n5, np.float32), pkg.DeviceArray.zeros(nmom, n5, np.float32)
        for vname, dt_code in (("cfg5_f32_planes", 1), ("cfg5_f32_fast", 2)):
            plan5 = wl5["coal_data"].plan(wl5["dist_types"], vel=vel, dtype=dt_code)
            L = pkg.lib()
            ms5 = _sustained_ms(pkg, lambda: pkg._lib.check(
                L.cloudy_rainshaft_sources(plan5.handle, n5, n5, m5.ptr, cs5.ptr, sf5.ptr, None)))
            variants[vname] = {
                "workload": f"cfg5: {n5} cells/GPU, cfg3b tensors and thresholds + sedimentation flux vel={vel}, "
                            "float planes in HBM (6 moments in, 6 coalescence sources + 6 fluxes out = 72 B/cell), "
                            + ("fp64 arithmetic" if dt_code == 1 else "single-precision Simpson pass")
                            + "; checked against the fp64 oracle in tests/test_gpu_parity.py",
                "value": n5 * world / (ms5 * 1e-3), "unit": "cell-RHS/s", "kernel_ms": ms5,
            }
            rl = _valu_roofline(measured, vname, n5, ms5)
            if rl:
                variants[vname]["roofline"] = rl
        del m5, cs5, sf5
        # the rainshaft drivers' time integration fused into one launch (cloudy_rainshaft_ssprk33_steps), fp64:
        # (i) throughput on 5e5 independent columns of 20 cells, (ii) latency of the reference example itself
        # (rainshaft_gamma_mixture.jl: ONE column of 20 cells, 1000 SSPRK33 steps of dt = 1 s)
        nz, ncol, nst = 20, 500_000, 2
        wlr = make_workload("cfg3b", nz * ncol, seed=SEED + 1000 * rank)
        planr = wlr["coal_data"].plan(wlr["dist_types"], vel=vel)
        ur = pkg.DeviceArray.from_numpy(wlr["mom"])
        outr = pkg.DeviceArray.zeros(nmom, nz * ncol)
        L = pkg.lib()

        def _col_steps(n_columns, n_steps, dt, sync=True):
            pkg._lib.check(L.cloudy_rainshaft_ssprk33_steps(planr.handle, nz, n_columns, nz * ncol, ur.ptr, outr.ptr,
                                                            150.0, dt, n_steps, None))
            if sync:
                pkg._lib.check(L.cloudy_stream_synchronize(None))

        msr = _sustained_ms(pkg, lambda: _col_steps(ncol, nst, 1e-3, sync=False), min_reps=3)
        variants["rainshaft_ssprk33_columns"] = {
            "workload": f"cloudy_rainshaft_ssprk33_steps: {ncol} columns x {nz} cells/GPU, cfg3b tensors and thresholds "
                        f"+ sedimentation vel={vel}, {nst} SSPRK33 steps (3 RHS evaluations each) in one launch, fp64",
            "value": 3 * nst * nz * ncol * world / (msr * 1e-3), "unit": "cell-RHS/s", "ms_per_call": msr,
        }
        rl = _valu_roofline(measured, "rainshaft_ssprk33_columns", nz * ncol, msr)   # flops per cell per CALL (6 evaluations)
        if rl:
            variants["rainshaft_ssprk33_columns"]["roofline"] = rl
        # ONE evaluation of the same right-hand side outside the fused integrator -- make_rainshaft_rhs(...)'s rhs!(dm, m, par, t),
        # the drop-in boundary of the rainshaft drivers (rainshaft_helpers.jl:45-89): since round 5 one launch of the column body
        # without the update (before: cell kernel + flux-divergence launch, 2.9 GB of HBM traffic per 1e7 cells instead of 1.45)
        fluxr = pkg.DeviceArray.zeros(nmom, nz * ncol)

        def _col_rhs():
            pkg._lib.check(L.cloudy_rainshaft_rhs(planr.handle, nz, ncol, nz * ncol, ur.ptr, 150.0, fluxr.ptr, outr.ptr, None))

        msu = _sustained_ms(pkg, _col_rhs, min_reps=3)
        variants["rainshaft_rhs"] = {
            "workload": f"cloudy_rainshaft_rhs on the same batch: ONE evaluation of the column right-hand side in one launch (cell sources, "
                        f"fluxes, divergence), fp64; the fused integrator above spends {msr / (3 * nst):.3f} ms per evaluation, update included",
            "value": nz * ncol * world / (msu * 1e-3), "unit": "cell-RHS/s", "ms_per_call": msu,
        }
        rl = _valu_roofline(measured, "rainshaft_rhs", nz * ncol, msu)
        if rl:
            variants["rainshaft_rhs"]["roofline"] = rl
        del fluxr
        z = (np.arange(nz) + 0.5) * 150.0
        at = ((z >= 0.5 * z.max() - 75.0) & (z < 0.75 * z.max() - 75.0)).astype(float)
        kg = np.array([[2.220446049250313e-16 / 1e6, 5.0], [5.0, 0.0]])   # CoalescenceTensor(LinearKernelFunction(5), 1)
        cd1 = pkg.CoalescenceData(pkg.CoalescenceTensor(kg), (3, 3), (2e-10, float("inf")), NORMS)
        plan1 = cd1.plan([1, 1], vel=vel)
        u1 = pkg.DeviceArray.from_numpy(np.outer([1e7, 1e-3, 2e-13, 0.0, 0.0, 0.0], at))
        o1 = pkg.DeviceArray.zeros(6, nz)
        for rep in range(2):
            t0 = time.perf_counter()
            pkg._lib.check(L.cloudy_rainshaft_ssprk33_steps(plan1.handle, nz, 1, nz, u1.ptr, o1.ptr, 150.0, 1.0, 1000,
                                                            None))
            pkg._lib.check(L.cloudy_stream_synchronize(None))
            ms1 = 1e3 * (time.perf_counter() - t0)
        variants["rainshaft_reference_example"] = {
            "workload": "rainshaft_gamma_mixture.jl end to end: 1 column x 20 cells, two Gamma modes, Golovin b = 5, "
                        "thr (2e-10, Inf), vel ((50, 1/6),), 1000 SSPRK33 steps of dt = 1 s in one launch",
            "value": ms1, "unit": "ms per solve", "higher_is_better": False,
            "column_mass_left": float(o1.to_numpy()[[1, 4]].sum() / 5e-3),
        }
        del ur, outr

    if more_variants:
        variants["cfg4q"] = _cfg4q_variant(pkg, rank, world, measured)
        variants["cfg4q_converged"] = _cfg4q_converged_variant(pkg, rank, world, measured, variants["cfg4q"]["kernel_ms"])
        # the default operator under the reference's other kernel functions and closures
        variants["cfg4q_converged_long"] = _converged_variant(
            pkg, rank, world, measured, "cfg4q_converged_long", [1, 1, 1], pkg.LongKernelFunction(5.236e-10, 9.44e9, 5.78),
            synth_moments(3, CFG4Q_PARCELS, SEED + 1000 * rank),
            f"the cfg4q batch ({CFG4Q_PARCELS} parcels/GPU, 3 Gamma modes) under LongKernelFunction(5.236e-10, 9.44e9, 5.78) "
            "(box_gamma_mixture_long.jl:20) in converged mode: two-phase walk, incomplete-beta table between x_t and 2 x_t",
            "cloudy_jit_quad_n3c8_long_f64")
        n_ln = 2_000_000
        variants["numerical_lognorm_example"] = _converged_variant(
            pkg, rank, world, measured, "numerical_lognorm_example", [3, 3], pkg.LinearKernelFunction(5.0),
            lognorm_example_moments(n_ln, SEED + 1000 * rank),
            f"test/examples/Numerical/n_particles_lognorm.jl as a batch: {n_ln} boxes/GPU of two Lognormal modes (n = 1e7 / 1e5 "
            "per m^3, mass scales 1e-10 / 1e-9 kg, each within a factor 2; sigma = ln 2), LinearKernelFunction(5.0), converged "
            "mode: the Lognormal mode's T_m by the trapezoidal inner rule", "cloudy_jit_quad_n2c8_linear_f64")

    t_variants = time.perf_counter()
    # every collective is behind us: ranks > 0 leave now, rank 0 times the CPU baseline on the host cores alone (once, after
    # the timed region, for any N -- a multi-GPU line carries its baseline too) and prints the line
    if _COMM["comm"] is not None:
        _COMM["comm"].close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
        dist = None
    hung = bool(_COMM.get("hung"))
    if hung and rank != 0:
        # a thread of this rank is still inside ncclCommInitRank: no interpreter shutdown to wait on it -- and the exit code
        # says so (a rank that hung in communicator set-up must not exit 0)
        sys.stderr.write(f"bench.py rank {rank}: RCCL communicator set-up hung; host-sum fallback was used; exit 3\n")
        sys.stderr.flush()
        os._exit(3)
    cpu = None
    if rank == 0 and not args.no_cpu_baseline:
        # ~30 s of CPU in the default run: the headline baseline + ONE quadrature baseline (the default
        # NumericalCoalStyle operator); the others behind --all-cpu-baselines
        cpu = _cpu_baseline(args.workload, target_seconds=8.0)
        if "cfg4q_converged" in variants:
            variants["cfg4q_converged"]["cpu_baseline"] = _cpu_baseline_cfg4q_converged(
                cpu["cores"], target_seconds=5.0, reference_parcel=args.all_cpu_baselines)
        if args.all_cpu_baselines:
            if "cfg3b" in variants:
                variants["cfg3b"]["cpu_baseline"] = _cpu_baseline("cfg3b", target_seconds=10.0)
            if "cfg4q" in variants:
                variants["cfg4q"]["cpu_baseline"] = _cpu_baseline_cfg4q(cpu["cores"], target_seconds=6.0)

    if rank == 0:
        out = _headline_keys(args, world, spec, n_local, nmom, value, res["wall"])
        out.update({
            "roofline": dict(_headline_roofline(args.workload, res["plan"], n_local, nmom, res["event_ms"], per_rank_ms,
                                                traffic, measured), **({"traffic_note": traffic_note} if traffic_note else {})),
            "cpu_baseline": cpu,
            "per_rank_devices": per_rank_dev,
            "ranks_share_a_gpu": not _COMM["own_gpu_per_rank"],
            "distinct_devices": len({d.get("pci_bus_id") for d in per_rank_dev if d.get("pci_bus_id")}),
            "collective": _COMM["collective"],
            "collective_fallback": bool(_COMM["fallback"]),
            "mass_rate_residual": abs(res["mass_rate_sum"]) / max(res["mass_rate_gross"], 1e-300),
            "mass_residual_per_parcel_max": res["mass_per_parcel"],
            "variants": variants,
            # where this process spent its wall time: the timed region is steps x ms_per_step; the rest is set-up
            # (imports, synthetic data, plan creation incl. ~1 s of hiprtc, warm-up, diagnostics), the other
            # workloads under "variants", and the CPU baseline
            "process_wall_s": {"setup_and_headline": t_headline - t_start, "timed_region": res["wall"],
                               "variants": t_variants - t_headline, "cpu_baseline": time.perf_counter() - t_variants},
        })
        emit(out, json_out)
        if hung:
            sys.stderr.write("bench.py rank 0: RCCL communicator set-up hung; the line carries collective_fallback = true; exit 3\n")
            sys.stderr.flush()
            os._exit(3)   # (as the other ranks above: a thread is still inside ncclCommInitRank)
    _rank_done()
    return 0


def _headline_keys(args, world, spec, n_local, nmom, value, wall):
    """the keys of the line that mean the same in a plain run and in a --full run"""
    return {
        "metric": "parcel moment-RHS evals/sec at 1e7 parcels; achieved HBM GB/s vs 8 TB/s peak",
        "value": value,
        "unit": "parcel-RHS/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * wall / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"{args.workload}: {n_local} parcels/GPU, {spec['n_modes']}-mode Gamma mixture, "
                               f"order-{2 if spec['kernel'] == 'long' else 1} polynomial CoalescenceTensor, "
                               f"{nmom} moments, thresholds {spec['thresholds']}, norms {NORMS}",
                   "parcels_per_gpu": n_local, "global_parcels": n_local * world, "sharding": f"parcel ranges x{world}"},
    }


def _plain_result(args, rank, world, dist, json_out, spec, n_local, nmom, value, res, per_rank_dev, t_start, t_headline):
    """The end of a plain run (no --full): the headline keys, which devices the ranks ran on, no side file"""
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        out = _headline_keys(args, world, spec, n_local, nmom, value, res["wall"])
        out.update({
            "per_rank_devices": per_rank_dev,
            "ranks_share_a_gpu": not _COMM["own_gpu_per_rank"],
            "distinct_devices": len({d.get("pci_bus_id") for d in per_rank_dev if d.get("pci_bus_id")}),
            "collective": "none: the conservation diagnostic, kernel times, variants and CPU baselines run with --full",
            "process_wall_s": {"setup_and_headline": t_headline - t_start, "timed_region": res["wall"]},
        })
        emit(out, json_out, side_file=False)
    _rank_done()
    return 0


def _rank_done():
    """the end-of-run mark _spawn_ranks looks for: a rank that exits 0 without it left before the last barrier"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.stderr.write(RANK_DONE_MARK + "\n")
        sys.stderr.flush()


def _main_guarded():
    """main() with ONE line of reason on stderr when a rank dies of an exception (a failed control-plane collective after a
    peer's death included), and an exit that does not wait on torch.distributed's destructors."""
    try:
        return main() or 0
    except SystemExit:
        raise
    except BaseException as e:   # noqa: BLE001
        import traceback

        traceback.print_exc()
        msg = (str(e).strip().splitlines() or [""])[0]
        sys.stderr.write(f"bench.py rank {os.environ.get('RANK', '0')}: FAILED: {type(e).__name__}: {msg[:300]}\n")
        sys.stderr.flush()
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            os._exit(EXIT_RANK_FAILED)
        return EXIT_RANK_FAILED


if __name__ == "__main__":
    sys.exit(_main_guarded())
