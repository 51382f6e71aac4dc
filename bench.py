#!/usr/bin/env python3
"""bench.py — headline benchmark of the hot path: Monte Carlo DC-OPF scenarios/sec, IEEE RTS-24.

  python bench.py --gpus N --steps K --warmup W
  N > 1 without a launcher: bench.py starts the N ranks itself (`launch_ranks`: N fresh child processes, one per GPU, before anything in the
  parent has touched torch or the GPU; rank 0's JSON line is the parent's stdout, the parent's exit code is the first failing rank's).
  Under a launcher (the driver's  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N) the ranks are the launcher's;
  WORLD_SIZE must then equal --gpus.

A "step" is one pass of the fused hot path (sample -> DC-OPF interior point -> accumulate) over one
batch of `--batch` (default 1e6 = BASELINE.json configs[1]) synthetic scenarios PER GPU, followed
by the convergence check's all-reduce of the index accumulators when N > 1 (weak scaling: the
per-GPU batch is fixed; `--scaling strong --total T` fixes the work per step instead: BASELINE configs[2]).
Scenarios are generated in-kernel by the counter-based sampler, so there is no input to stage: the
timed region starts with everything it needs resident in HBM (the case tables, ~5 KB).
Prints ONE JSON line on rank 0.

What the `roofline` object means here: the dominant kernel issues no MFMA; it is bound by the
fp64 VALU pipe and the CU's LDS pipe together.  `achieved` / `frac` price the fp64 operations the kernel EXECUTES
(static schedule of the sparse block LDL' + per-element work) against the fp64 vector peak, the same definition for
every workload; `frac_dense_equiv` keeps SURVEY.md 8d's dense-equivalent count beside it.  Pipe utilisations and HBM
traffic cannot be read by a program about itself: they come from the committed rocprofv3 PMC passes of this very
command (profiles/<current>/pmc_summary.json) and say so in `counters_source`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6         # MI355X fp64 vector = matrix peak: 256 CU x 4 SIMD x 16 FMA/clk x 2 x 2.4 GHz
GPU_CLOCK_HZ = 2.4e9


def dense_flop_per_iter(nb):
    """algorithmic flops of one Newton step on the dense reduced system of order n_r = 2 nb - 1."""
    n = 2 * nb - 1
    return n ** 3 / 3.0 + 2.0 * n * n + 1.5e3


EXIT_WORLD_MISMATCH = 7         # WORLD_SIZE of the launcher != --gpus
EXIT_TOO_FEW_GPUS = 6           # --gpus exceeds the GPUs of the node (and --share-device was not asked for)
EXIT_RANKS_DIVERGED = 8         # a rank finished cleanly while its peers were still running long after: they wait for it in a collective it never entered


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _die_with_parent():
    """preexec of a rank process: SIGTERM when the parent goes away (a killed bench.py must not leave ranks on the GPUs)."""
    import ctypes
    import signal
    try:
        ctypes.CDLL("libc.so.6", use_errno=True).prctl(1, signal.SIGTERM, 0, 0, 0)       # PR_SET_PDEATHSIG
    except OSError:
        pass


def launch_ranks(n, argv, poll=0.05, grace=5.0, script=None, straggler_s=120.0):
    """`bench.py --gpus N` called plainly: the analogue of opening the reference's parfor pool (nsqMain.m:257-263, seqMain.m:112-133).
    The parent has imported neither torch nor the package and holds no GPU state; it starts N FRESH processes of this very script with the
    same arguments plus RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / a free MASTER_PORT (never a re-exec of itself), lets rank 0
    write the JSON line to the parent's stdout (the other ranks' stdout goes to stderr), and waits.  The first rank that leaves with a
    non-zero code (86 = a guarded collective stalled, 3 = communicator refused, 4 = rank-count mismatch, 5 = duplicate GPUs, 6 = too few
    GPUs) ends the run: the remaining ranks are terminated by pid and the parent exits with that code.  A rank that leaves with code 0 while
    others are still running `straggler_s` seconds later (every rank ends after the same last collective) is a divergence, not a success: the
    rest is stopped and the parent exits with code 8."""
    import signal
    import subprocess
    port = _free_port()
    script = script or os.path.abspath(__file__)
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n), "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "RELMC_BENCH_LAUNCHER": "bench.py"})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, script] + list(argv), env=env, stdout=None if r == 0 else sys.stderr,
                                      preexec_fn=_die_with_parent))

    def stop_all(*_):
        for p in procs:
            if p.poll() is None:
                p.terminate()
        t_end = time.time() + grace
        for p in procs:
            try:
                p.wait(max(0.0, t_end - time.time()))
            except subprocess.TimeoutExpired:
                p.kill(); p.wait()

    def on_signal(signum, _frame):
        stop_all()
        sys.exit(128 + signum)
    signal.signal(signal.SIGTERM, on_signal)
    signal.signal(signal.SIGINT, on_signal)
    code = 0
    first_clean_exit = None
    while True:
        running = 0
        for r, p in enumerate(procs):
            rc = p.poll()
            if rc is None:
                running += 1
            elif rc != 0 and code == 0:
                code = rc if rc > 0 else 128 - rc
                print(f"bench.py: rank {r} of {n} (pid {p.pid}) left with code {rc}: stopping the other ranks", file=sys.stderr, flush=True)
            elif rc == 0 and first_clean_exit is None:
                first_clean_exit = (time.time(), r)
        if not code and running and first_clean_exit is not None and time.time() - first_clean_exit[0] > straggler_s:
            code = EXIT_RANKS_DIVERGED
            print(f"bench.py: rank {first_clean_exit[1]} of {n} finished {straggler_s:.0f} s ago and {running} rank(s) are still running: the ranks took "
                  f"different paths (a collective one of them never entered); stopping them", file=sys.stderr, flush=True)
        if code or not running:
            break
        time.sleep(poll)
    stop_all()
    return code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1_000_000, help="scenarios per GPU per step (weak scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--total", type=int, default=100_000_000, help="strong scaling: scenarios per step over all GPUs (BASELINE configs[2]: 1e8)")
    ap.add_argument("--workload", choices=["nsq24", "rts96", "seq"], default="nsq24",
                    help="nsq24 = BASELINE configs[1] (the headline, default); rts96 = configs[4] shape; seq = configs[3] shape")
    ap.add_argument("--years", type=int, default=125, help="seq workload: simulated years per GPU per step")
    ap.add_argument("--backend", default="nccl", help="process-group backend (nccl = RCCL; gloo only to exercise the N > 1 path on a 1-GPU box)")
    ap.add_argument("--comm", choices=["auto", "native", "torch", "host"], default="auto",
                    help="who all-reduces relmc_acc when N > 1: auto (default) = native, and if RCCL refuses to build the communicator (an error, not a hang) "
                         "every rank agrees over the rendezvous to fall back to `host` and the line says so in comm.fallback; native = the library's own RCCL communicator (relmc_comm_*: the north star's "
                         "single RCCL all-reduce over xGMI, no host staging; the 128-byte id travels over a gloo group, torch holds NO nccl group in the "
                         "process: one RCCL user); torch = torch.distributed's collective on the process group; host = torch's collective registered "
                         "with the library as the host transport (relmc_comm_set_host_allreduce).  native / host run the multi-rank nsqMain loop "
                         "below the C ABI (relmc_nsq_run)")
    ap.add_argument("--comm-timeout", type=float, default=120.0, help="wall-clock guard (seconds) of communicator init and of every collective: on expiry the "
                                                                       "rank prints who it is and what it waited for and exits non-zero (0 = off)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the RTS-96 / sequential / HL1 rates measured beside the headline (outside the timed region)")
    ap.add_argument("--no-sustained", action="store_true", help="skip the sustained-rate leg (one stream of --sustained-samples scenarios, outside the timed region)")
    ap.add_argument("--sustained-samples", type=int, default=300_000_000, help="scenarios of the sustained-rate leg (>= 2.5e8: more than 4 s of continuous GPU work)")
    ap.add_argument("--share-device", action="store_true", help="testing only: every rank uses GPU 0")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--policy", choices=["emulate", "physical"], default="emulate")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-time-to-cov", action="store_true", help="skip the nsqMain runs (profiling: only identical launches)")
    ap.add_argument("--cpu-sample", type=int, default=0, help="scenarios of the CPU baseline sample (0 = auto)")
    ap.add_argument("--dump-acc", default="", help="testing: rank 0 writes the merged accumulators of the timed steps to this file")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="rank 0 writes what the last timed step returned (its all-reduced relmc_acc; the seq workload adds the annual indices) "
                         "to DIR/<name>.npy, float64")
    args = ap.parse_args()

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and "RANK" not in os.environ:
        if args.gpus > 1:
            # no launcher: this process becomes one (it has not imported torch and never touches a GPU)
            sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    elif int(env_world or "1") != args.gpus:
        print(f"bench.py: the launcher started WORLD_SIZE={env_world or '1'} ranks but --gpus says {args.gpus}: refusing to report one as the other "
              f"(call `python bench.py --gpus {args.gpus}` plainly, or give the launcher --nproc-per-node {args.gpus})", file=sys.stderr, flush=True)
        sys.exit(EXIT_WORLD_MISMATCH)

    import torch
    import torch.distributed as dist
    from powersystemsreliabilityassessment_amd import api, case24, case96, dist as rdist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if os.environ["MASTER_ADDR"] in ("127.0.0.1", "localhost", "::1"):
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")  # ONE node: RCCL's bootstrap sockets over loopback (the container's hostname may not resolve); xGMI carries the data
        if args.comm in ("native", "auto") and args.backend != "gloo":
            if rank == 0 and args.backend != ap.get_default("backend"):
                print(f"bench.py: --backend {args.backend} is not used with --comm {args.comm}: the process group is gloo (rendezvous, barriers, max of the elapsed "
                      f"time), the library's own RCCL communicator carries the all-reduce (ONE RCCL user per process); --comm torch honours --backend", file=sys.stderr, flush=True)
    n_dev = torch.cuda.device_count()                          # counts devices without initialising one
    if n_dev < 1:
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))        # ranks on THIS node (an external multi-node launcher sets it; WORLD_SIZE is global)
    if local_world > n_dev and not args.share_device:
        print(f"bench.py: rank {rank}: {local_world} ranks on this node (--gpus {world}) but it has {n_dev} GPU{'s' if n_dev != 1 else ''} (torch.cuda.device_count()); "
              f"--share-device puts every rank on GPU 0 (testing only)", file=sys.stderr, flush=True)
        sys.exit(EXIT_TOO_FEW_GPUS)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    if args.share_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    # --comm native: ONE RCCL user in the process (the library's communicator), so torch gets a gloo group for the rendezvous,
    # the barriers and the max over ranks of the elapsed time
    pg_backend = "gloo" if args.comm in ("native", "auto") else args.backend
    if args.share_device and world > 1 and pg_backend == "nccl":
        pg_backend = "gloo"          # RCCL refuses two ranks on one device ("Duplicate GPU detected"): the rehearsal's process group is gloo
        if rank == 0:
            print("bench.py: --share-device: the process group is gloo (RCCL does not accept two ranks on one GPU)", file=sys.stderr, flush=True)
    guard = lambda what: rdist.Watchdog(args.comm_timeout, what, rank=rank, world=world, device=local_rank)
    if world > 1:
        # gloo announces its connections on the C stdout ("[Gloo] Rank 0 is connected to ..."): stdout carries ONE line, the JSON one, so file
        # descriptor 1 points at stderr while the group is built
        sys.stdout.flush()
        fd1 = os.dup(1)
        os.dup2(2, 1)
        try:
            # the rendezvous gets three times the collectives' limit: on a fresh box the ranks' first `import torch` takes minutes and need not end together
            with rdist.Watchdog(3.0 * args.comm_timeout, f"torch.distributed.init_process_group({pg_backend})", rank=rank, world=world, device=local_rank):
                if pg_backend == "nccl":
                    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
                else:
                    dist.init_process_group(pg_backend, rank=rank, world_size=world)
                dist.barrier() if pg_backend != "nccl" else None          # gloo connects lazily: make it speak now
        finally:
            os.dup2(fd1, 1)
            os.close(fd1)

    def sync():
        if world > 1:
            dist.barrier(device_ids=[local_rank]) if pg_backend == "nccl" else dist.barrier()
        torch.cuda.synchronize()

    policy = api.REFERENCE_EMULATE if args.policy == "emulate" else api.PHYSICAL
    opts = api.mpoption(policy)
    sq = None
    if args.workload == "rts96":
        case = case96.rts96()
    else:
        case = case24.rts24()
    eng = api.Engine(case, device=local_rank)
    eng.comm_set_timeout(args.comm_timeout)
    comm = None
    comm_fallback = None
    if world > 1 and args.comm != "torch":
        err = ""
        if args.comm == "auto":
            # the deadline is bench.py's here (a helper thread around relmc_comm_init): a stall must end in the fallback, not in the library's exit
            eng.comm_set_timeout(0)
            comm, err = rdist.NativeComm.try_init(eng, rank, world, args.comm_timeout if args.comm_timeout > 0 else 0)
            eng.comm_set_timeout(args.comm_timeout)
            if err:
                print(f"bench.py: rank {rank}: communicator init failed: {err}", file=sys.stderr, flush=True)
        else:
            try:
                # native: RCCL through the C ABI, the unique id travels over the gloo group; host: torch's collective as the library's transport
                comm = rdist.NativeComm(eng, rank, world) if args.comm == "native" else rdist.HostComm(eng, rank, world, device)
            except api.RelmcError as e:
                print(f"bench.py: rank {rank}: communicator init failed: {e}", file=sys.stderr, flush=True)
                sys.exit(3)          # no hang, no retry: every rank reports what RCCL said and leaves with a non-zero code
        if args.comm == "auto":
            # did every rank get its communicator?  One gather over the rendezvous; if any did not, ALL fall back to the host collective
            # (torch's gloo all-reduce registered as the library's transport: host-staged, always available) -- loudly, and the line records it
            box_ = [None] * world
            with guard("all_gather of the communicator-init outcomes"):
                dist.all_gather_object(box_, err)
            if any(box_):
                stalled_any = any("stalled" in m for m in box_ if m)
                if comm is not None and not stalled_any:
                    comm.close()
                elif comm is not None or "stalled" in err:
                    # a context whose communicator cannot be destroyed safely (a peer is stuck inside RCCL) or whose init call is still
                    # running on the abandoned thread is left alone for good: the pair stays referenced for the life of the process (no
                    # finaliser may reach ncclCommDestroy; the process leaves through os._exit below), the fallback gets a context of its own
                    rdist.keep_forever(comm, eng)
                    eng = api.Engine(case, device=local_rank)
                    eng.comm_set_timeout(args.comm_timeout)
                comm_fallback = next(m for m in box_ if m)
                print(f"bench.py: rank {rank}: falling back to --comm host (the library's loop over torch's gloo collective): {comm_fallback}", file=sys.stderr, flush=True)
                comm = rdist.HostComm(eng, rank, world, device)
    ar_seconds, ar_calls = [0.0], [0]

    def allreduce(acc):
        t_ = time.perf_counter()
        if comm is not None:
            out_ = comm.allreduce_acc(acc)                       # guarded inside the library (relmc_comm_set_timeout)
        elif world > 1:
            with guard("torch.distributed.all_reduce of relmc_acc"):
                out_ = rdist.allreduce_acc(acc, device)
        else:
            out_ = acc
        ar_seconds[0] += time.perf_counter() - t_; ar_calls[0] += 1
        return out_

    # which GPU every rank drives (PCI bus id from the library's own context): the line proves N DISTINCT devices
    devices = [eng.pci_bus_id()]
    if world > 1:
        box_ = [None] * world
        with guard("all_gather of the ranks' PCI bus ids"):
            dist.all_gather_object(box_, devices[0])
        devices = [str(x) for x in box_]
        if len(set(devices)) != world and not args.share_device:
            print(f"bench.py: rank {rank}: the {world} ranks drive only {len(set(devices))} distinct GPUs: {devices}", file=sys.stderr, flush=True)
            sys.exit(5)

    B = args.batch
    if args.workload in ("nsq24", "rts96"):
        def step(k):
            if args.scaling == "strong":
                lo, cnt = rdist.shard_range(k * args.total, args.total, rank, world)
            else:
                lo, cnt = (k * world + rank) * B, B        # global scenario index space: step k, rank r owns [(k*world + r)*B, +B)
            acc = eng.nsq_accumulate(args.seed, lo, cnt, opts)
            ms = eng.last_kernel_ms()
            return allreduce(acc), ms, cnt, {}             # the convergence check's single all-reduce
        unit = "scenarios/s"
        if args.workload == "nsq24":
            metric = "Monte Carlo DC-OPF scenarios/sec (RTS-24 HL2 non-sequential)"
            per = f"{B:d} samples per GPU per step (BASELINE configs[1])" if args.scaling == "weak" else f"{args.total:d} samples per step over all GPUs (BASELINE configs[2])"
            workload = "HL2 non-sequential MCS, IEEE RTS-24 DC-OPF load shedding, " + per
        else:
            metric = "Monte Carlo DC-OPF scenarios/sec (RTS-96 HL2 non-sequential)"
            workload = (f"HL2 non-sequential MCS, IEEE RTS-96 (73 buses, 120 branches, 99 generator rows) DC-OPF load shedding, "
                        f"{B if args.scaling == 'weak' else args.total} samples per {'GPU per ' if args.scaling == 'weak' else ''}step (BASELINE configs[4] shape)")
    else:
        import numpy as np
        from powersystemsreliabilityassessment_amd import seq as rseq
        sq = rseq.SeqEngine(eng)
        Y = args.years

        def step(k):
            e, d, n_, ncont, acc = sq.seq_years(args.seed, (k * world + rank) * Y, Y)
            ms = eng.last_kernel_ms()
            trip = np.column_stack([e, d, n_])
            if comm is not None:
                trip = comm.allgather_rows(trip, [Y] * world)   # relmc_comm_allreduce_f64: every rank fills its own rows of a zeroed matrix
            elif world > 1:
                with guard("torch.distributed.all_gather of the annual indices"):
                    trip = rdist.allgather_years(trip, [Y] * world, device)
            n_rank = int(acc.n)
            return allreduce(acc), ms, n_rank, {"year_ens": trip[:, 0], "year_dlc": trip[:, 1], "year_nlc": trip[:, 2]}
        unit, metric = "hourly DC-OPFs/s", "Monte Carlo hourly DC-OPF evaluations/sec (RTS-24 HL2 sequential)"
        workload = f"HL2 sequential MCS, RTS-24, {Y} simulated years x 8736 h per GPU per step, contingency hours only (BASELINE configs[3] shape)"

    for k in range(args.warmup):
        step(k)
    sync()
    t0 = time.perf_counter()
    total, kernel_ms, units_rank = None, [], 0
    for k in range(args.steps):
        acc, ms, u, arrays = step(args.warmup + k)
        kernel_ms.append(ms); units_rank += u
        total = acc if total is None else rdist.merge(total, acc)
    sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, acc, arrays, case)
    kernel_ms_per_rank = [sum(kernel_ms) / len(kernel_ms)]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device if pg_backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        box = [None] * world
        dist.all_gather_object(box, kernel_ms_per_rank[0])
        kernel_ms_per_rank = [float(x) for x in box]
    # the collective as the run saw it: who carried it, how many ranks IT reports, what one all-reduce of relmc_acc cost
    import ctypes as _C
    from powersystemsreliabilityassessment_amd import _abi as _rabi
    if comm is not None:
        ci = comm.info()
        comm_info = {"backend": comm.kind, "nranks_seen": ci["nranks_seen"], "allreduce_calls": ci["allreduce_calls"],
                     "allreduce_us_avg": 1e6 * ci["allreduce_seconds"] / max(1, ci["allreduce_calls"])}
    else:
        comm_info = {"backend": ("torch-" + pg_backend) if world > 1 else "none", "nranks_seen": dist.get_world_size() if world > 1 else 1,
                     "allreduce_calls": ar_calls[0] if world > 1 else 0, "allreduce_us_avg": (1e6 * ar_seconds[0] / max(1, ar_calls[0])) if world > 1 else 0.0}
    comm_info["allreduce_bytes"] = _C.sizeof(_rabi.Acc)
    comm_info["devices"] = devices
    comm_info["timeout_s"] = args.comm_timeout
    if comm_fallback:
        comm_info["fallback"] = "native communicator refused, host collective used instead: " + comm_fallback
    if comm_info["nranks_seen"] != world:
        print(f"bench.py: rank {rank}: the communicator reports {comm_info['nranks_seen']} ranks, the launcher {world}", file=sys.stderr, flush=True)
        sys.exit(4)

    # wall-time to EENS CoV < 1 % over all ranks (second half of BASELINE.json's metric), outside the timed region
    ttc_multi = None
    if world > 1 and args.workload == "nsq24" and not args.no_time_to_cov:
        sync()
        # convergence check every 32 768 samples per rank = four full rounds of the 16-lane tile's grid (8 192 scenario rows): whole-round launches
        # are the efficient ones (a launch costs as many rounds as its busiest wavefront walks), and one all-reduce per check
        ttc_batch = 32_768 * world
        t1 = time.perf_counter()
        # with a communicator in the context the loop runs below the C ABI (relmc_nsq_run shards and all-reduces); otherwise in Python
        idx, tot, hist = rdist.nsq_run_distributed(lambda s, lo, n: eng.nsq_accumulate(s, lo, n, opts), case.nb, case.ncomp, seed=args.seed,
                                                   beta_limit=0.01, max_samples=50_000_000, batch=ttc_batch, device=device,
                                                   allreduce=allreduce, engine=eng if comm is not None else None, mpopt=opts)
        sync()
        ttc_multi = {"seconds": time.perf_counter() - t1, "samples": int(tot.n), "beta": idx["beta"], "edns_mw": idx["edns"], "batch": ttc_batch,
                     "loop": "relmc_nsq_run (below the C ABI)" if comm is not None else "dist.nsq_run_distributed (Python)"}
        if comm is not None:
            # the reference's own checkpoint spacing (nsqMain.m:60: 100 samples) over all ranks: relmc_nsq_run evaluates stretches of checkpoints,
            # every rank its slice, ONE all-reduce of the per-checkpoint sums + accumulators per stretch, and stops at the one-rank run's checkpoint.
            # An extra beside the headline: a failure here (every rank takes the same path, so it is every rank's) is recorded, not fatal.
            try:
                eng.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=args.seed, mpopt=opts)
                sync()
                c0 = comm.info()["allreduce_calls"]
                t1 = time.perf_counter()
                r100 = eng.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=args.seed, mpopt=opts)
                sync()
                ttc_multi["checkpoints_of_100"] = {"seconds": time.perf_counter() - t1, "samples": r100.current_iteration, "beta": r100.current_beta, "edns_mw": r100.accumulated_edns,
                                                   "converged": r100.converged, "checkpoints": len(r100.beta_history), "beta_history_head": [float(x) for x in r100.beta_history[:3]],
                                                   "beta_history_tail": [float(x) for x in r100.beta_history[-3:]], "n_fail": int(r100.acc.n_fail),
                                                   "host_collective_callbacks" if comm.kind.startswith("host") else "collectives": comm.info()["allreduce_calls"] - c0}
            except Exception as ex:       # noqa: BLE001 - reported in the line
                ttc_multi["checkpoints_of_100"] = {"error": f"{type(ex).__name__}: {ex}"[:300]}
    # the reference's unique-state database over N ranks (nsqMain.m:220-278): every rank keeps the database of ITS slices, so a state two
    # ranks meet is solved twice.  Measured here, in the line: rows solved per rank against the rows one database holds for the same samples
    db_multi = None
    if world > 1 and args.workload == "nsq24" and not args.no_time_to_cov and comm is not None:
        sync()
        t1 = time.perf_counter()
        rdb = eng.nsqMain(beta_limit=0.0017, max_iterations=50_000_000, samples_per_batch=1_000_000, seed=args.seed, mpopt=opts, distinct_states="database")
        sync()
        dtdb = time.perf_counter() - t1
        box_ = [None] * world
        with guard("all_gather of the ranks' database sizes"):
            dist.all_gather_object(box_, int(eng.db_size()[0]))
        if rank == 0:
            eng.db_reset()                                            # one database over the same samples: what a single rank would have solved
            for lo_ in range(0, rdb.current_iteration, 1_000_000):
                eng.nsq_db_batch(args.seed, lo_, min(1_000_000, rdb.current_iteration - lo_), opts)
            rows_one = int(eng.db_size()[0])
            db_multi = {"what": "relmc_nsq_run with distinct_states = database over all ranks, batches of 1e6 samples split over the ranks, to the reference's beta < 0.0017",
                        "per_rank_database": True, "seconds": dtdb, "samples": rdb.current_iteration, "beta": rdb.current_beta, "edns_mw": rdb.accumulated_edns,
                        "rows_per_rank": [int(x) for x in box_], "rows_single_database": rows_one,
                        "redundant_solves_x": sum(int(x) for x in box_) / max(1, rows_one),
                        "note": "state ownership is not sharded: the path is bound by the sort / lookup of the samples (6e8-1e9 samples/s per GPU), which does shard; "
                                "the redundant solves are the price of no exchange step (DESIGN.md 4)"}
        sync()

    if rank == 0:
        n_total = int(total.n)
        mean_iters = total.sum_iters / n_total
        avg_kernel_s = sum(kernel_ms) / len(kernel_ms) * 1e-3
        units_per_launch = units_rank / args.steps                      # what ONE launch of the dominant kernel processes on this rank
        fl_exec = sparse_flop_per_iteration(eng, case)
        fl_dense = dense_flop_per_iter(case.nb)
        achieved = units_per_launch * mean_iters * fl_exec / avg_kernel_s / 1e12
        achieved_dense = units_per_launch * mean_iters * fl_dense / avg_kernel_s / 1e12
        kname = "relmc_eval_kernel<2>" if args.workload == "seq" else "relmc_eval_kernel<0>"
        roof = {"bound": "fp64-valu+lds-pipe (no MFMA issued)", "achieved": achieved, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": achieved / FP64_PEAK_TFLOPS, "frac_executed": achieved / FP64_PEAK_TFLOPS,
                "frac_dense_equiv": achieved_dense / FP64_PEAK_TFLOPS,
                "flop_model": "achieved/frac = fp64 operations the kernel executes per Newton step (static sparse block-LDL' schedule + per-element work, "
                              "bench.sparse_flop_per_iteration) x measured mean IPM iterations; frac_dense_equiv = SURVEY 8d's dense reduced order-(2nb-1) count "
                              "(above 1 on RTS-96: that count is avoidable work)",
                "flop_per_iteration_executed": fl_exec, "flop_per_iteration_dense_equiv": fl_dense, "mean_ipm_iterations": mean_iters,
                "kernel": kname, "kernel_ms_avg": avg_kernel_s * 1e3, "units_per_launch": units_per_launch}
        from powersystemsreliabilityassessment_amd import _lib as _rlib
        code_hash = _rlib.code_object_sha256()
        roof.update(counters_from_profile(args.workload, units_per_launch, torch.cuda.get_device_properties(local_rank).multi_processor_count,
                                          kernel_ms_avg=avg_kernel_s * 1e3, code_hash=code_hash))
        out = {
            "metric": metric, "value": n_total / elapsed, "unit": unit, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload, "policy": args.policy, "seed": args.seed,
                       "solver_schedule": schedule_summary(eng, case),
                       "parallelism": f"scenario-index{' / year' if args.workload == 'seq' else ''} sharding x{world}, 1 all-reduce of relmc_acc per step "
                                      f"({comm.kind + ' through the C ABI' if comm is not None else 'torch.distributed ' + (pg_backend if world > 1 else '(single rank: no collective)')})"},
            "roofline": roof,
            "binary": {"library": os.path.relpath(_rlib.LIB_PATH, ROOT), "code_object_sha256": code_hash, "version": _rlib.load().relmc_version().decode()},
            "comm": comm_info, "kernel_ms_per_rank": kernel_ms_per_rank,
            "indices": {"n": n_total, "edns_mw": total.sum_dns / n_total, "plc": total.n_fail / n_total,
                        "n_singular": int(total.n_singular), "n_nonconverged": int(total.n_nonconverged),
                        "second_attempts_rank0": list(eng.retry_stats())},     # units re-evaluated under a further elimination order, converged
        }
        if args.workload == "nsq24":
            idx = rdist.indices_from_acc(total, case.nb, case.ncomp)
            out["indices"].update({"lole_h_per_yr": idx["lole"], "beta": idx["beta"]})
        if ttc_multi is not None:
            out["time_to_cov_1pct"] = ttc_multi
        if db_multi is not None:
            out["distinct_state_path"] = db_multi
        out["launcher"] = "bench.py --gpus N (self-started ranks)" if os.environ.get("RELMC_BENCH_LAUNCHER") == "bench.py" else ("external (RANK / WORLD_SIZE from the environment)" if world > 1 else "none (single rank)")
        if world > 1:
            out["omitted"] = {"keys": None,
                              "why": "N > 1 lines are scaling rows: the CPU baseline, the other BASELINE configurations and the sustained-rate leg are measured on rank 0 at N = 1 only"}
        if world == 1 and args.workload == "nsq24" and not args.no_time_to_cov:
            # the reference checks beta every 100 samples (nsqMain.m:60, 299-312): the same spacing here (relmc_nsq_run evaluates stretches of
            # checkpoints per launch and stops at the reference's checkpoint), and a coarse spacing of 1e5 samples beside it
            eng.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=args.seed, mpopt=opts)        # first call: buffers
            t1 = time.perf_counter()
            r = eng.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=args.seed, mpopt=opts)
            dt = time.perf_counter() - t1
            t1 = time.perf_counter()
            rb = eng.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100_000, seed=args.seed, mpopt=opts)
            dtb = time.perf_counter() - t1
            out["time_to_cov_1pct"] = {"seconds": dt, "samples": r.current_iteration, "beta": r.current_beta,
                                       "edns_mw": r.accumulated_edns, "batch": 100, "converged": r.converged,
                                       "checkpoints_of_100000": {"seconds": dtb, "samples": rb.current_iteration, "beta": rb.current_beta}}
            # the reference's own speed trick (nsqMain.m:220-278), reported beside the headline, never as `value`: the persistent
            # unique-state database on the device (known states bump a count, only new states are solved)
            eng.db_reset(); eng.nsq_db_batch(args.seed, 0, B, opts); eng.db_reset()                   # warm-up: allocations
            rates = []
            for k in range(4):
                t1 = time.perf_counter(); _, st = eng.nsq_db_batch(args.seed, k * B, B, opts); dt = time.perf_counter() - t1
                rates.append({"batch": k, "ms": dt * 1e3, "samples_per_s": B / dt, "rows": int(st.rows), "new_rows": int(st.new_rows)})
            t1 = time.perf_counter()
            r1 = eng.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=args.seed, mpopt=opts, distinct_states="database")
            dt1 = time.perf_counter() - t1
            t1 = time.perf_counter()
            r2 = eng.nsqMain(beta_limit=0.0017, max_iterations=50_000_000, samples_per_batch=1_000_000, seed=args.seed, mpopt=opts, distinct_states="database")
            dt2 = time.perf_counter() - t1
            out["distinct_state_path"] = {
                "what": "persistent unique-state database on the device (relmc_nsq_db_batch), 1e6-sample batches from an empty database",
                "batches": rates,
                "time_to_cov_1pct_seconds": dt1, "samples": r1.current_iteration, "beta": r1.current_beta, "rows": r1.database_row_count,
                "time_to_reference_beta_limit_0.0017": {"seconds": dt2, "samples": r2.current_iteration, "beta": r2.current_beta,
                                                        "rows": r2.database_row_count, "edns_mw": r2.accumulated_edns}}
        if world == 1 and args.workload == "nsq24" and not args.no_sustained:
            out["sustained"] = sustained_rate(eng, opts, args.seed, args.sustained_samples)
        if world == 1 and args.workload == "nsq24" and not args.no_secondary:
            out["secondary"] = secondary_workloads(eng, local_rank, opts, args.seed)
        if world == 1 and args.workload == "nsq24" and not args.no_secondary:
            out["screened"] = screened_rates(eng, local_rank, policy, args.seed, B)
        if world == 1 and not args.no_cpu_baseline and args.workload == "nsq24":
            out["cpu_baseline"] = cpu_baseline(case, policy, args.seed, args.cpu_sample)
        if "omitted" in out:          # what a full N = 1 line carries and this one does not, from what was actually emitted
            out["omitted"]["keys"] = [k for k in ("cpu_baseline", "secondary", "screened", "sustained", "time_to_cov_1pct", "distinct_state_path") if k not in out]
        if args.dump_acc:
            ints, dbls = total.to_arrays()
            with open(args.dump_acc, "w") as fh:
                json.dump({"ints": ints.tolist(), "dbls": [float(x).hex() for x in dbls]}, fh)
        print(json.dumps(out), flush=True)
    if comm is not None:
        comm.close()
    if world > 1:
        dist.destroy_process_group()
    if rdist.abandoned_threads() or rdist.kept_forever():
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(0)              # a helper thread is still inside a stalled RCCL call: do not wait for it at interpreter exit


def dump_outputs(out_dir, acc, arrays, case):
    """The last timed step's result as DIR/<name>.npy (float64): the relmc_acc fields, trimmed to the case's components and buses, plus the
    workload's own arrays.  The scenario indices of a step depend on (--seed, --warmup, --steps, --batch / --total / --years, --gpus) only,
    so two builds run with the same arguments can be compared output for output."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    counts = [acc.n, acc.n_fail, acc.n_singular, acc.n_infeasible, acc.n_nonconverged, acc.sum_iters, acc.n_screened]
    out = {"acc_counts": np.array(counts, dtype=np.float64),                # n, n_fail, n_singular, n_infeasible, n_nonconverged, sum_iters, n_screened
           "acc_comp_fail": np.array(acc.comp_fail[:case.ncomp], dtype=np.float64),
           "acc_sum_dns": np.array([acc.sum_dns, acc.sum_dns2], dtype=np.float64),
           "acc_sum_nodal": np.array(acc.sum_nodal[:case.nb], dtype=np.float64)}
    out.update({k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()})
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def sustained_rate(eng, opts, seed, n):
    """The headline's rate held over seconds, not over a 0.35 s burst: ONE relmc_nsq_accumulate call over `n` fresh scenarios (the index range
    starts at 2^40, far from the timed steps), outside the timed region.  The library walks the range in launches of its own size; `kernel_ms_per_1e6`
    is the HIP-event time of all of them per 1e6 scenarios, `value` the wall-clock rate of the call."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    acc = eng.nsq_accumulate(seed, 1 << 40, n, opts)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"what": "one relmc_nsq_accumulate call, every sample solved, same kernel and options as the timed steps", "seconds": dt, "samples": int(acc.n),
            "value": acc.n / dt, "unit": "scenarios/s", "kernel_ms_per_1e6": eng.last_kernel_ms() / (acc.n / 1e6),
            "edns_mw": acc.sum_dns / acc.n, "mean_ipm_iterations": acc.sum_iters / acc.n, "n_nonconverged": int(acc.n_nonconverged)}


def secondary_workloads(eng24, device, opts, seed, steps=3):
    """The other BASELINE.json configs on this GPU, measured OUTSIDE the timed region (1 warm-up + `steps` steps each, wall-clocked between
    synchronisations like the headline): configs[4] shape (RTS-96, 1e6 samples per step), configs[3] shape (sequential RTS-24, 125 years x 8736 h
    per step = the contingency hours' DC-OPFs), configs[0] (HL1 copper sheet, 1e5 iterations x 8736-h load curve per step)."""
    import numpy as np
    import torch
    from powersystemsreliabilityassessment_amd import api, case96, hl1, seq as rseq
    res = {}

    def timed(fn):
        fn(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); outs = []; kms = []
        for k in range(1, steps + 1):
            outs.append(fn(k)); kms.append(eng_cur[0].last_kernel_ms())
        torch.cuda.synchronize()
        return outs, (time.perf_counter() - t0) / steps, sum(kms) / len(kms)

    def line(eng, case, accs, dt, kms, units, unit, workload, kernel):
        n = sum(int(a.n) for a in accs); it = sum(int(a.sum_iters) for a in accs)
        mean_it = it / max(1, n)
        fl = sparse_flop_per_iteration(eng, case)
        ach = (n / len(accs)) * mean_it * fl / (kms * 1e-3) / 1e12
        return {"workload": workload, "value": units / dt, "unit": unit, "ms_per_step": dt * 1e3, "kernel": kernel, "kernel_ms_avg": kms, "steps": steps,
                "mean_ipm_iterations": mean_it, "flop_per_iteration_executed": fl, "achieved_tflops_executed": ach, "frac_executed": ach / FP64_PEAK_TFLOPS,
                "n_nonconverged": sum(int(a.n_nonconverged) for a in accs), "solver_schedule": schedule_summary(eng, case)}

    # configs[4] shape: RTS-96
    c96 = case96.rts96()
    e96 = api.Engine(c96, device=device)
    eng_cur = [e96]
    B = 1_000_000
    accs, dt, kms = timed(lambda k: e96.nsq_accumulate(seed, k * B, B, opts))
    res["rts96"] = line(e96, c96, accs, dt, kms, B, "scenarios/s", f"HL2 non-sequential MCS, IEEE RTS-96 DC-OPF load shedding, {B} samples per step (BASELINE configs[4] shape)",
                        "relmc_eval_kernel<0, Tile96>")
    e96.close()
    # configs[3] shape: sequential RTS-24
    sq = rseq.SeqEngine(eng24)
    eng_cur = [eng24]
    Y = 125
    outs, dt, kms = timed(lambda k: sq.seq_years(seed, k * Y, Y, opts)[4])
    lp = sum(int(a.n) for a in outs) / len(outs)
    res["seq"] = line(eng24, eng24.case, outs, dt, kms, lp, "hourly DC-OPFs/s", f"HL2 sequential MCS, RTS-24, {Y} simulated years x 8736 h per step, contingency hours only "
                      "(BASELINE configs[3] shape)", "relmc_eval_kernel<2, Tile24>")
    res["seq"]["years_per_s"] = Y / dt
    # configs[0]: HL1 copper sheet (GeneratingAdequacy path): one fleet state per iteration swept over the 8736-h load curve
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    N1 = 100_000
    rs, dt, kms = timed(lambda k: hl1.run_non_sequential_mc(gens, load, N1, seed=seed + k, engine=eng24))
    res["hl1"] = {"workload": f"HL1 copper-sheet non-sequential MCS on IEEE RTS-24, {N1} iterations x 8736-h load curve per step (BASELINE configs[0])",
                  "value": N1 / dt, "unit": "iterations/s", "ms_per_step": dt * 1e3, "kernel": "relmc_hl1_kernel", "kernel_ms_avg": kms, "steps": steps,
                  "lole_h_per_yr": float(np.mean([r.lole_hours_yr for r in rs])), "eue_mwh_per_yr": float(np.mean([r.eue_mwh_yr for r in rs])),
                  "exact_lole_eue": [9.3941, 1176.29], "includes": "per-iteration LOLE history copied to the host (the reference's convergence history, :202-204); the fleet and the load curve are loaded once"}
    return res


def screened_rates(eng24, device, policy, seed, B, steps=3):
    """The same workloads with the zero-curtailment pre-screen (relmc_solver_opts.screen = 1, csrc/relmc_screen.hip), OUTSIDE the timed
    region and never as `value`: a sample whose LP optimum is proven 0 by an explicit dispatch is counted without being solved (the reference's outputs
    for it are (0, zeros) by mc_simulation.m:57-59, 65); every accumulator but the iteration sum equals the unscreened run's (tests/test_screen.py).
    Wall-clocked between synchronisations like the headline: 1 warm-up + `steps` steps each."""
    import torch
    from powersystemsreliabilityassessment_amd import api, case96, seq as rseq
    so = api.mpoption(policy, screen=1)

    def timed(fn, eng):
        # warm-up over the very ranges that are timed: a unit the primary elimination order does not converge on (6.7e-7 of the RTS-96 samples) makes the
        # library build the further orders' images at first need (tens of ms, once per context) -- at 4 ms per step that would be the measurement
        for k in range(0, steps + 1):
            fn(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter(); outs = []; kms = []
        for k in range(1, steps + 1):
            outs.append(fn(k)); kms.append(eng.last_kernel_ms())
        torch.cuda.synchronize()
        return outs, (time.perf_counter() - t0) / steps, sum(kms) / len(kms)

    def line(accs, dt, kms, units, unit, workload):
        n = sum(int(a.n) for a in accs); ns = sum(int(a.n_screened) for a in accs)
        return {"workload": workload, "value": units / dt, "unit": unit, "ms_per_step": dt * 1e3, "device_ms_avg": kms, "steps": steps, "n_screened_frac": ns / max(1, n),
                "solved_per_step": (n - ns) / len(accs), "mean_ipm_iterations_of_the_solved": sum(int(a.sum_iters) for a in accs) / max(1, n - ns),
                "n_nonconverged": sum(int(a.n_nonconverged) for a in accs)}

    res = {"what": "relmc_solver_opts.screen = 1: zero-curtailment certificate (proportional dispatch of the units in service through the base-topology PTDF, one or two lines out "
                   "through the outage system) in a pre-pass, one thread per sample; only the uncovered samples reach the interior point.  Outputs other than the iteration "
                   "statistics are those of the unscreened run (tests/test_screen.py); `value` above stays every-sample-solved"}
    accs, dt, kms = timed(lambda k: eng24.nsq_accumulate(seed, (1 << 41) + k * B, B, so), eng24)
    res["nsq24"] = line(accs, dt, kms, B, "scenarios/s", f"HL2 non-sequential MCS, IEEE RTS-24, {B} samples per step (BASELINE configs[1]) behind the pre-screen")
    nd = []
    accs, dt, kms = timed(lambda k: (lambda r: (nd.append(r[1]), r[0])[1])(eng24.nsq_accumulate_distinct(seed, (1 << 41) + k * B, B, so)), eng24)
    res["nsq24_distinct"] = line(accs, dt, kms, B, "scenarios/s", f"the same {B} samples per step: pre-screen, then the reference's per-batch dedupe (nsqMain.m:220-229) of the uncovered samples "
                                                                   "(relmc_nsq_accumulate_distinct): only their distinct states are solved")
    res["nsq24_distinct"]["distinct_states_solved_per_step"] = sum(nd[-steps:]) / steps
    del res["nsq24_distinct"]["mean_ipm_iterations_of_the_solved"]        # sum_iters counts a distinct state's iterations once per sample that shares it
    res["nsq24_distinct"]["uncovered_samples_per_step"] = res["nsq24_distinct"].pop("solved_per_step")
    eng24.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=seed, mpopt=so)
    t1 = time.perf_counter()
    r = eng24.nsqMain(beta_limit=0.01, max_iterations=5_000_000, samples_per_batch=100, seed=seed, mpopt=so)
    res["time_to_cov_1pct"] = {"seconds": time.perf_counter() - t1, "samples": r.current_iteration, "beta": r.current_beta, "batch": 100, "n_screened_frac": r.n_screened / max(1, r.current_iteration)}
    eng24.db_reset(); eng24.nsq_db_batch(seed, 0, B, so); eng24.db_reset()
    t1 = time.perf_counter(); _, st = eng24.nsq_db_batch(seed, 0, B, so); dtb = time.perf_counter() - t1
    eng24.db_reset()
    t1 = time.perf_counter()
    r2 = eng24.nsqMain(beta_limit=0.0017, max_iterations=50_000_000, samples_per_batch=1_000_000, seed=seed, mpopt=so, distinct_states="database")
    res["distinct_state_path"] = {"first_batch_from_empty_ms": dtb * 1e3, "first_batch_rows": int(st.rows),
                                  "time_to_reference_beta_limit_0.0017": {"seconds": time.perf_counter() - t1, "samples": r2.current_iteration, "beta": r2.current_beta,
                                                                          "rows": r2.database_row_count, "n_screened_frac": r2.n_screened / max(1, r2.current_iteration)}}
    eng24.db_reset()
    sq = rseq.SeqEngine(eng24)
    Y = 125
    outs, dt, kms = timed(lambda k: sq.seq_years(seed, (1 << 20) + k * Y, Y, so)[4], eng24)
    lp = sum(int(a.n) for a in outs) / len(outs)
    res["seq"] = line(outs, dt, kms, lp, "hourly DC-OPFs/s", f"HL2 sequential MCS, RTS-24, {Y} simulated years x 8736 h per step, contingency hours only, behind the pre-screen")
    res["seq"]["years_per_s"] = Y / dt
    e96 = api.Engine(case96.rts96(), device=device)
    accs, dt, kms = timed(lambda k: e96.nsq_accumulate(seed, (1 << 41) + k * B, B, so), e96)
    res["rts96"] = line(accs, dt, kms, B, "scenarios/s", f"HL2 non-sequential MCS, IEEE RTS-96, {B} samples per step behind the pre-screen")
    e96.close()
    return res


def schedule_summary(eng, case):
    """Which static pass program the kernel interprets: passes per Newton step and where its elimination order comes from."""
    import ctypes as C
    out = (C.c_int32 * 9)()
    eng.L.relmc_debug_schedule(eng._h, out)
    tuned = getattr(case, "elim_order", None) is not None
    return {"update_inversion_backsubstitution_passes": [int(out[0]), int(out[1]), int(out[2])], "off_diagonal_blocks": int(out[3]), "tasks": int(out[8]),
            "elimination_order": "tuned offline against the library's scheduler (relmc_tune_order; the order ships with the package's case)" if tuned
                                 else "the library's rule (level, then fill)"}


def sparse_flop_per_iteration(eng, case):
    """Floating-point operations one Newton iteration of the shipped sparse solver executes per scenario: the static
    schedule's task counts (43 flop per 2x2 block update, 29 per right-hand-side update, 21 per pivot inversion, 14 per
    back-substitution task) plus the per-element work on lines, injections and buses (about 60 / 70 / 30 flop each)."""
    import ctypes as C
    out = (C.c_int32 * 9)()
    eng.L.relmc_debug_schedule(eng._h, out)
    noff, ntask = out[3], out[8]
    nblock = ntask - case.nb - 2 * noff
    return 43.0 * nblock + 29.0 * noff + 21.0 * case.nb + 14.0 * noff + 60.0 * case.nl + 70.0 * case.ninj + 30.0 * case.nb


def counters_from_profile(workload, units_per_launch, n_cu, kernel_ms_avg=None, code_hash=None, profiles_dir=None):
    """Pipe utilisations and HBM traffic of the dominant kernel from the committed rocprofv3 PMC passes of this command
    (profiles/<current>/pmc_summary[_<workload>].json; separate --pmc runs, FETCH_SIZE doubled per MI355X_MICROARCH.md).
    SQ cycle counters tick once per 4 clocks per wavefront; GRBM_GUI_ACTIVE sums the 8 XCDs."""
    none = {"traffic": None, "lds_pipe_busy": None, "lds_conflict_frac": None, "valu_busy": None, "waves_per_simd": None,
            "mfma_fp64_ops": None, "counters_source": "no committed profile for this workload", "counters_stale": True,
            "counters_stale_why": "no committed profile for this workload"}
    pdir = profiles_dir or os.path.join(ROOT, "profiles")
    try:
        with open(os.path.join(pdir, "current.txt")) as fh:
            name = fh.read().strip()
        fn = "pmc_summary.json" if workload == "nsq24" else f"pmc_summary_{workload}.json"
        with open(os.path.join(pdir, name, fn)) as fh:
            summ = json.load(fh)
    except (OSError, ValueError):
        return none
    # the workload's production kernel = the eval-kernel entry that did the work (MODE 5, the one short order-calibration launch of
    # relmc_case_load, and MODE 4, the rows re-evaluated under a further elimination order, are eval kernels too)
    ev = [k for k in summ if "eval_kernel" in k and "pmc_sq" in summ[k] and "pmc_lds" in summ[k]]
    if not ev:
        return none
    k = summ[max(ev, key=lambda q: summ[q]["pmc_sq"]["sums"].get("SQ_INSTS_VALU", 0.0))]
    try:
        sq, lds = k["pmc_sq"]["sums"], k["pmc_lds"]["sums"]
        n_disp = max(1, k["pmc_lds"]["dispatches"])
        cyc = lds["GRBM_GUI_ACTIVE"] / 8.0                                  # kernel-active clocks of the profiled launches (summed over them)
        res = {"lds_pipe_busy": lds["SQ_LDS_IDX_ACTIVE"] / (n_cu * cyc),
               "lds_conflict_frac": lds["SQ_LDS_BANK_CONFLICT"] / lds["SQ_LDS_IDX_ACTIVE"],
               "valu_busy": 4.0 * sq["SQ_ACTIVE_INST_VALU"] / (4.0 * n_cu * cyc),
               "waves_per_simd": lds["SQ_WAVES"] / n_disp / (4.0 * n_cu),      # resident wavefronts: the persistent grid fills the device once
               "mfma_fp64_ops": lds.get("SQ_INSTS_VALU_MFMA_MOPS_F64"),
               "lds_instructions_per_unit": sq["SQ_INSTS_LDS"] / summ.get("units_per_profiled_launch", units_per_launch) / max(1, k["pmc_sq"]["dispatches"]),
               "valu_instructions_per_unit": sq["SQ_INSTS_VALU"] / summ.get("units_per_profiled_launch", units_per_launch) / max(1, k["pmc_sq"]["dispatches"])}
        t = summ.get("hbm_traffic")
        res["traffic"] = t["bytes_per_scenario"] * units_per_launch if t else None
        res["traffic_unit"] = "bytes per launch (HBM, PMC FETCH_SIZE x2 + WRITE_SIZE)"
        res["counters_source"] = f"from_profile: profiles/{name}/{fn} (rocprofv3 --pmc passes of `bench.py --workload {workload} --steps 1 --warmup 0`, not measured in this run)"
        # is the profile about THIS binary, and does the kernel still take the time it took under the profiler?  (scripts/summarize_profile.py
        # records the code-object hash the profiled bench line printed and the minimum launch duration of the kernel trace)
        why = []
        ph, pmin = summ.get("code_object_sha256"), summ.get("kernel_ms_min")
        res["profile_code_object_sha256"], res["profile_kernel_ms_min"] = ph, pmin
        if not ph:
            why.append("the profile summary records no code-object hash")
        elif code_hash is not None and ph != code_hash:
            why.append(f"profiled code object {ph[:12]} != this library's {code_hash[:12]}")
        if pmin and kernel_ms_avg is not None:
            pmin_l = pmin * units_per_launch / max(1, summ.get("units_per_traced_launch", units_per_launch))
            if abs(kernel_ms_avg - pmin_l) > 0.03 * pmin_l:
                why.append(f"kernel_ms_avg {kernel_ms_avg:.3f} is more than 3 % off the profile's minimum launch {pmin_l:.3f} ms")
        res["counters_stale"] = bool(why)
        if why:
            res["counters_stale_why"] = "; ".join(why)
        return res
    except (KeyError, ZeroDivisionError, TypeError):
        return none


def cpu_baseline(case, policy, seed, n_sample):
    """The CPU restatement (oracle/relmc_oracle.c: MATPOWER formulation, dense LU KKT solve) timed on
    the host cores of this box on a bounded sample of the same scenario stream.  Reported baseline
    only — never the thing measured as `value`."""
    from oracle import coracle
    orc = coracle.Oracle(case)
    cores = min(orc.max_threads(), len(os.sched_getaffinity(0)))
    quota = None
    try:                                       # container CPU quota (cgroup v2): the box shows 256 CPUs but grants fewer
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = max(1, int(round(int(q) / int(per))))
            cores = min(cores, quota)
    except (OSError, ValueError):
        pass
    t0 = time.perf_counter()
    orc.nsq_accumulate(seed, 0, 200 * cores, policy, nthreads=cores, memo=False)     # calibration
    rate = 200 * cores / (time.perf_counter() - t0)
    n = n_sample or int(max(2000, min(2_000_000, rate * 12.0)))                      # ~12 s of CPU work
    t0 = time.perf_counter()
    acc = orc.nsq_accumulate(seed, 0, n, policy, nthreads=cores, memo=False)
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    n1 = 1500
    orc.nsq_accumulate(seed, 0, n1, policy, nthreads=1, memo=False)                  # single-core figure as well
    dt1 = time.perf_counter() - t1
    # wall-time to EENS CoV < 1 % on the CPU: the reference's own algorithm — the nsqMain loop with its
    # unique-state database, batches of 100 as nsqMain.m:62 — restated in C, new states evaluated on all granted cores
    t2 = time.perf_counter()
    d = orc.nsq_database(seed, 0.01, 5_000_000, 100, policy=policy, nthreads=cores, max_rows=200_000)
    dt2 = time.perf_counter() - t2
    model = ""
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                model = ln.split(":", 1)[1].strip(); break
    except OSError:
        pass
    try:
        load1 = os.getloadavg()[0]
    except OSError:
        load1 = None
    return {"value": n / dt, "unit": "scenarios/s", "cores": cores, "kind": "port", "single_core_value": n1 / dt1, "cpu_quota": quota,
            "box": {"cpu_model": model, "cpus_visible": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)), "cgroup_quota_cpus": quota, "loadavg_1min_before": load1,
                    "threads_used": cores, "per_thread_value": n / dt / cores,
                    "note": "the box is shared: the granted cores run at whatever clock and cache share the neighbours leave (round 2: 43.3 k/s, round 3: 36.2 k/s on the same "
                            "16 granted threads); single_core_value x threads bounds what contention took"},
            "sample": f"first {n} scenarios of the same seed, every scenario solved (no state memo), "
                      f"{dt:.1f} s on {cores} OpenMP threads (host CPUs visible {os.cpu_count()}, cgroup quota {quota})",
            "edns_mw": acc.sum_dns / acc.n,
            "time_to_cov_1pct": {"seconds": dt2, "samples": d["iterations"], "beta": float(d["beta_history"][-1]), "unique_states_solved": int(len(d["count"])),
                                 "edns_mw": float(d["edns_history"][-1]),
                                 "how": "nsqMain loop in the reference's database form (oracle orc_nsq_database, batches of 100, only new states solved), "
                                        f"{cores} threads; solving every sample instead would take samples / value = {d['iterations'] / (n / dt):.1f} s"}}


if __name__ == "__main__":
    main()
