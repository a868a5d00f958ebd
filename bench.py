#!/usr/bin/env python
"""Headline benchmark: point-cloud pairs/sec of the VCR-Net registration hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W

N > 1: one process per GPU over RCCL.  Either launched by torch.distributed.run (RANK / WORLD_SIZE in the
environment) or plainly as above, in which case this process only spawns the N rank processes (fresh children started
BEFORE anything here touches the GPU), waits for them and exits with their worst code; rank 0 prints the line.  A rank
that dies or a run that passes --deadline-s takes every other rank down with it: the parent prints one JSON line with
an "error" field, leaves each rank's stderr in gpurun_out/rank<r>.err and exits non-zero -- it never hangs.
--strong: --batch is the GLOBAL batch, split evenly over the ranks (BASELINE configs[3]: --gpus 8 --points 2048
--batch 128 --strong = 16 pairs per GPU); the default is weak scaling (--batch pairs per GPU).

One "step" = one pass of the whole hot path (VCRNet.forward: LPDNet kNN-graph embedding -> Transformer
virtual-correspondence block -> soft correspondences -> SVD rigid solve) over one batch of 16 synthetic pairs of
N=1024 points PER GPU (BASELINE.json configs[1]; weak scaling), inputs already resident in HBM, plus -- for N > 1 --
the RCCL all-gather of the per-rank (R, t).  A plain run sets up, runs --warmup steps, times ONE block of exactly
--steps steps (barrier + synchronize on both sides, MAX over ranks) and prints ONE JSON line on rank 0: `value`
(pairs/s) and `ms_per_step` come from that block.

--full adds everything beyond that headline, as the run did before the split: the K-step block is repeated until
>= 12 s of GPU time have been spent (--min-seconds) so that external samplers see the load, the MEDIAN block is
reported and every block's time is listed; the per-launch HIP events behind `roofline` / `stages` are recorded inside
those same timed blocks, on every 5th step (--trace-every: ~35 event records cost ~2 % of a step that carries them);
one GPU also gets `other_configs`, and every run the `parity_ledger` and (one GPU) the `cpu_baseline`.

--dump-outputs DIR: after the timed steps, what the last of them returned (vcrnetIter's six tensors, and with N > 1
the gathered poses) is written as DIR/<name>.npy in float32 / float64 by rank 0; the inputs are seeded, so two builds
run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16, help="pairs per GPU (with --strong: pairs in total)")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling: --batch is the global batch, sharded evenly over the ranks")
    ap.add_argument("--deadline-s", type=float, default=1200.0,
                    help="N > 1: overall wall-clock limit; when it passes every rank is killed, their stacks are in "
                         "gpurun_out/rank<r>.err and one JSON line with an \"error\" field is printed")
    ap.add_argument("--init-timeout-s", type=float, default=120.0, help="torch.distributed rendezvous / collective timeout")
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--partial", action="store_true",
                    help="partial-overlap mode (BASELINE configs[2]): clouds cropped to int(points*0.7507) points, "
                         "key pruning + selectCom/getCopair heads; combine with --points 1024 --batch 24 --iters 3")
    ap.add_argument("--iters", type=int, default=1, help="vcrnetIter refinement passes per step (one C call)")
    ap.add_argument("--emb-nn", default="lpdnet", choices=["lpdnet", "dgcnn", "pointnet"],
                    help="feature extractor (--emb_nn of the reference; dgcnn / pointnet use seeded weights)")
    ap.add_argument("--regime", default="default", choices=["default", "seed4321", "trained", "randemb"],
                    help="point in weight space (vcrnet_amd.weights.regime_weights; lpdnet only): default = seed 1234 + the "
                         "LPD-pretrained emb_nn (the headline), randemb = a random feature extractor -- what the ordered kNN "
                         "search's per-cloud guard must cope with")
    ap.add_argument("--full", action="store_true",
                    help="also measure what is not the headline: repeated timed blocks (--min-seconds), the per-launch "
                         "events behind roofline / stages, other_configs, the parity ledger and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64, rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget-s", type=float, default=100.0,
                    help="wall-clock budget of the CPU-baseline thread sweep (each thread count: one warm-up, then up "
                         "to 5 timed runs while the budget lasts)")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="SURVEY 8d protocol without a budget: every thread count, B = --batch, median of 5")
    ap.add_argument("--min-seconds", type=float, default=None,
                    help="repeat the timed K-step block for this long (default: 12 with --full, else one block)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full on one GPU appends `other_configs` (BASELINE configs[2] -- also with every pass recomputing "
                         "both clouds --, configs[3]'s per-GPU share, configs[4] and the bf16x3+sdpa line, --other-seconds of timed blocks each) AFTER the headline has "
                         "been measured; this switch leaves them out")
    ap.add_argument("--other-seconds", type=float, default=2.0, help="timed seconds per entry of `other_configs`")
    ap.add_argument("--stages", action="store_true", help="print the per-launch table to stderr (needs --full)")
    ap.add_argument("--trace-every", type=int, default=5,
                    help="record the per-launch HIP events (roofline / stage table) on every N-th step of each timed "
                         "block: the ~35 event records cost ~2 %% of a step they are recorded in; 1 = every step")
    ap.add_argument("--linear-mode", default="fp32", choices=["fp32", "bf16x3", "bf16x3+sdpa"],
                    help="fp32: linears and attention on v_mfma_f32_32x32x2_f32 (default, the headline).  bf16x3: the "
                         "linears' products as exact 3-way bf16 splits on the bf16 matrix pipe (fp32-equivalent "
                         "accuracy); bf16x3+sdpa: the attention products too.  Both are labelled in `dtype`")
    ap.add_argument("--linear-mfma", type=int, default=0, choices=[0, 16, 32],
                    help="MFMA shape of the fp32 linears: 0 = the library's choice, 16 = v_mfma_f32_16x16x4_f32, 32 = 32x32x2")
    ap.add_argument("--knn-waves", type=int, default=0, choices=[0, 1, 8],
                    help="feature-space kNN kernel: 8 = 16-query waves (16x16x4 MFMA), 1 = 32-query waves, 0 = the library's choice")
    ap.add_argument("--sdpa-variant", type=int, default=0, choices=[0, 1, 2],
                    help="fp32 attention-output kernel: 0 = the library's choice, 1 = the tile kernel, 2 = the persistent kernel")
    ap.add_argument("--no-iter-reuse", action="store_true",
                    help="--iters > 1: every pass recomputes both clouds (as the reference does) instead of reusing what the first "
                         "pass computed from the unchanged target cloud; same bits")
    ap.add_argument("--no-merge-encdec", action="store_true",
                    help="enc.qkv / dec.qkv and the two self-attentions as separate launches (default: one GEMM + one grouped launch)")
    ap.add_argument("--linear-bk", type=int, default=0, choices=[0, 16, 32], help="k-slab of the fp32 linears (0 = the library's choice)")
    ap.add_argument("--linear-bm", type=int, default=0, choices=[0, 96, 128], help="tile height of the fp32 linears (0 = the library's choice)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl == RCCL on ROCm); gloo only "
                                                      "for exercising the multi-rank control flow on a 1-GPU box")
    a = ap.parse_args(argv)
    if a.stages and not a.full:
        ap.error("--stages prints the per-launch events that only --full records")
    if a.min_seconds is None:
        a.min_seconds = 12.0 if a.full else 0.0
    return a


def model_args(partial=False, emb_nn="lpdnet"):
    from vcrnet_amd import synth
    return SimpleNamespace(emb_dims=512, cycle=False, emb_nn=emb_nn, pointer="transformer", vcp_nn="topK",
                           partial=partial, overlap2=synth.OVERLAP2_0575 if partial else 0.75, t3d=False, tfea=False,
                           n_blocks=1, dropout=0.0, ff_dims=1024, n_heads=4)


# ---- N > 1 without torchrun: spawn the ranks ourselves -------------------------------------------------------------

def _error_line(a, msg, logs=()):
    """The one JSON line of a failed multi-rank run (same keys the driver parses, value null, plus `error`)."""
    tails = {}
    for r, path in enumerate(logs):
        try:
            with open(path, errors="replace") as f:
                tails[str(r)] = f.read()[-600:]
        except OSError:
            pass
    return json.dumps({"metric": "point-cloud pairs/sec (N=%d, batch %d%s)" % (a.points, a.batch, "" if a.strong else " per GPU"),
                       "value": None, "unit": "pairs/s", "n_gpus": a.gpus, "steps": a.steps, "warmup": a.warmup,
                       "error": msg, "rank_stderr_tail": tails})


def spawn_ranks(a) -> int:
    """Start a.gpus fresh rank processes of this script (one per GPU, LOCAL_RANK = rank) and watch them.  The parent
    never initialises the GPU (torch.cuda.device_count() does not, and nothing else here touches HIP) and never
    re-executes itself.  Fail fast: the first rank that exits non-zero, or the deadline, ends the run -- the other ranks
    (blocked in a collective by then) are killed by PID, stderr of every rank stays in gpurun_out/rank<r>.err."""
    ndev = torch.cuda.device_count()
    if a.backend == "nccl" and a.gpus > ndev:
        print(f"bench.py: --gpus {a.gpus} but {ndev} GPU(s) visible: one process per GPU", file=sys.stderr)
        print(_error_line(a, f"--gpus {a.gpus} but {ndev} GPU(s) visible"), flush=True)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    logdir = os.environ.get("VCR_BENCH_LOGDIR", os.path.join(ROOT, "gpurun_out"))
    os.makedirs(logdir, exist_ok=True)
    procs, logs, files = [], [], []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        logs.append(os.path.join(logdir, f"rank{r}.err"))
        files.append(open(logs[-1], "w"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env, stderr=files[-1]))
    deadline = time.monotonic() + a.deadline_s
    failure = None
    while failure is None:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            failure = "rank %d exited with code %d" % bad[0]
        elif all(c == 0 for c in codes):
            break
        elif time.monotonic() > deadline:
            failure = "deadline of %.0f s passed (ranks still running: %s)" % (
                a.deadline_s, [r for r, c in enumerate(codes) if c is None])
        else:
            time.sleep(0.1)
    if failure is not None:
        for p in procs:                        # exact PIDs of our own children
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    for f in files:
        f.close()
    if failure is not None:
        print(f"bench.py: {failure}; see {logdir}/rank*.err", file=sys.stderr)
        print(_error_line(a, failure, logs), flush=True)
        return 1
    for r, path in enumerate(logs):            # a clean run still forwards what the ranks said
        with open(path, errors="replace") as f:
            txt = f.read()
        if txt.strip():
            sys.stderr.write(f"--- rank {r} stderr ---\n{txt}")
    return 0


# ---- CPU baseline ----------------------------------------------------------------------------------------------------

def cpu_baseline(w, B, N, k, partial=False, iters=1, budget_s=100.0, full=False, one_thread_full_s=30.0):
    """The CPU oracle (a port of the reference's PyTorch CPU path) timed on this box's host cores: the
    bench workload's own batch size, thread counts {1, 8, 16, 32, 64, nproc}, one warm-up then the median of up to 5
    runs each.  The default run is bounded by `budget_s` (the 1-thread leg starts on a 2-pair sample and adds ONE run at
    the full batch size when that sample predicts it takes <= `one_thread_full_s`); `full` lifts the bound.  `value` = the best thread count's pairs/s; the whole table is kept."""
    import oracle
    from vcrnet_amd import synth
    ncpu = os.cpu_count() or 1
    kind = "object" if N < 2048 else "uniform"
    cfg = oracle.OracleConfig(k=k, partial=partial, overlap2=synth.OVERLAP2_0575 if partial else 0.75)
    full_B = B if N <= 1024 else min(B, 4)
    data = {}

    def sample(nb):
        if nb not in data:
            src, tgt, _, _, _ = synth.make_batch(0, nb, N, partial=partial, kind=kind)
            data[nb] = (torch.from_numpy(src), torch.from_numpy(tgt))
        return data[nb]

    threads = sorted({t for t in (1, 8, 16, 32, 64, ncpu) if t <= ncpu})
    share = budget_s / len(threads)                                    # every thread count gets an equal slice
    table = {}
    prev = torch.get_num_threads()
    try:
        for th in threads:
            nb = full_B if (full or th > 1) else min(full_B, 2)
            s, t = sample(nb)
            torch.set_num_threads(th)
            leg = time.perf_counter()
            oracle.vcrnet_iter(w, s, t, cfg, iters=iters)              # warm-up
            warm = time.perf_counter() - leg
            ts = []
            for _ in range(5):
                if not full and ts and (time.perf_counter() - leg) + warm > share:
                    break
                t0 = time.perf_counter()
                oracle.vcrnet_iter(w, s, t, cfg, iters=iters)
                ts.append(time.perf_counter() - t0)
            table[th] = {"pairs_per_s": nb / float(np.median(ts)), "sample_pairs": nb, "runs": len(ts)}
            if nb < full_B and float(np.median(ts)) * full_B / nb <= one_thread_full_s:
                # the 1-thread leg at the workload's own batch size when the sample says one run fits (warmed up above)
                s, t = sample(full_B)
                t0 = time.perf_counter()
                oracle.vcrnet_iter(w, s, t, cfg, iters=iters)
                table[th] = {"pairs_per_s": full_B / (time.perf_counter() - t0), "sample_pairs": full_B, "runs": 1}
    finally:
        torch.set_num_threads(prev)
    best = max(table, key=lambda th: table[th]["pairs_per_s"])
    # "cores" = the threads the reported value actually ran on (the best of the sweep); "host_cpus" = what the box has
    return {"value": table[best]["pairs_per_s"], "unit": "pairs/s", "cores": best, "threads": best, "host_cpus": ncpu, "kind": "port",
            "one_thread": table.get(1, {}).get("pairs_per_s"),
            "by_threads": {str(th): table[th] for th in sorted(table)},
            "sample": f"oracle.vcrnet_iter(iters={iters}{', partial' if partial else ''}), N={N}, k={k}, fp32, "
                      f"B={full_B} pairs per run (1-thread leg: {table.get(1, {}).get('sample_pairs', '-')}), one warm-up "
                      f"then median of <=5 runs per thread count, {'no budget' if full else f'{budget_s:.0f} s budget'}; "
                      f"best = {best} threads of os.cpu_count()={ncpu}"}


def parity_ledger(mode):
    """The accuracy trade the throughput is bought with, next to it: profiles/accuracy_ledger.txt (written by
    tests/test_hip_ledger.py on the GPU box) holds, per weight regime and fixture, the error of the HIP path AND of the
    fp32 reference against the reference's float64 twin.  Condensed for this run's arithmetic mode: the ratio HIP error /
    reference's own error of the final embeddings (rms) per whole-mode fixture, the worst pose errors, and the discrete
    selections of the partial path that differ from the twin's (HIP vs the fp32 reference).  A ratio of 1 = as accurate as
    ATen's fp32; the linears' single 512-step accumulation chain (LINEAR_BLOCKED_ACC = 0, csrc/linear.hip) is what
    puts the embeddings above 1 -- the blocked variant measures 1.0x at -1.6 % of the headline."""
    import hashlib
    import re
    path = os.path.join(ROOT, "profiles", "accuracy_ledger.txt")
    try:
        raw = open(path, "rb").read()
    except OSError:
        return None
    from vcrnet_amd import build as vb
    whole, flips = {}, {"hip": [0, 0, 0], "ref32": [0, 0, 0], "hip_vs_ref32": [0, 0, 0]}
    taken_on = None
    num = r"([0-9.eE+-]+)"
    for ln in raw.decode(errors="replace").splitlines():
        m = re.match(r"# kernel_sources_sha16=(\w+)", ln)
        if m:
            taken_on = m.group(1)
            continue
        f = ln.split("|")
        head = f[0].split()
        if len(head) >= 4 and head[0] == "whole" and head[3] == mode:
            R = re.search(f"hip {num} ref32 {num}", f[1]); t = re.search(f"hip {num} ref32 {num}", f[2])
            e = re.search(f"hip {num}/{num} ref32 {num}/{num}", f[3])
            whole[f"{head[1]}/{head[2]}"] = {
                "emb_rms_hip_over_ref32": round(float(e.group(2)) / float(e.group(4)), 3),
                "R_err_hip": float(R.group(1)), "R_err_ref32": float(R.group(2)),
                "t_err_hip": float(t.group(1)), "t_err_ref32": float(t.group(2))}
        elif len(head) >= 5 and head[0] == "partial" and head[4] == mode:
            m = re.search(r"hip (\d+)/(\d+)/(\d+)\s+ref32 (\d+)/(\d+)/(\d+)", f[1])
            v = re.search(r"hip vs ref32 (\d+)/(\d+)/(\d+)", f[2])
            for i in range(3):
                flips["hip"][i] += int(m.group(1 + i)); flips["ref32"][i] += int(m.group(4 + i))
                flips["hip_vs_ref32"][i] += int(v.group(1 + i))
    if not whole:
        return None
    ratios = [v["emb_rms_hip_over_ref32"] for v in whole.values()]
    return {"source": "profiles/accuracy_ledger.txt", "source_sha16": hashlib.sha256(raw).hexdigest()[:16],
            "ledger_kernel_sources": taken_on or "(unrecorded: a ledger of round 5)",
            "this_build_kernel_sources": vb.sources_sha16(), "arithmetic": mode,
            "yardstick": "the reference model in float64 on the same weights and inputs (tests/golden/*_twin.npz)",
            "emb_rms_hip_over_ref32": {"worst": max(ratios), "median": float(np.median(ratios)), "by_fixture": whole},
            "worst_R_err": {"hip": max(v["R_err_hip"] for v in whole.values()), "ref32": max(v["R_err_ref32"] for v in whole.values())},
            "worst_t_err": {"hip": max(v["t_err_hip"] for v in whole.values()), "ref32": max(v["t_err_ref32"] for v in whole.values())},
            "partial_selection_flips_vs_twin_keys_overlap_pairs": flips,
            "linear_accumulation": "one k-ascending chain per output (LINEAR_BLOCKED_ACC = 0); blocked: 1.0x at -1.6 %, BK 32 only: 1.10x at -0.9 %"}


def workload_label(a, Nfull, N, B, kind, world=1):
    if a.partial:
        base = ("BASELINE configs[2]" if (Nfull, B, a.iters) == (1024, 24, 3) else "partial-overlap (configs[2] recipe)") + \
            ": partial-to-partial overlap 0.575 (clouds cropped %d -> %d points), " % (Nfull, N)
    elif kind == "uniform":
        base = ("BASELINE configs[4]: kNN/EdgeConv stress, " if (N, a.k) == (4096, 40) else
                "BASELINE configs[3] (global batch 128 sharded over 8 GPUs): " if (N == 2048 and a.strong and
                                                                                    (a.batch, world) == (128, 8)) else
                "BASELINE configs[3] (one GPU's share): " if N == 2048 else "") + "synthetic random clouds U(-0.5,0.5)^3, "
    else:
        base = ("BASELINE configs[1]: " if (N, B) == (1024, 16) else "configs[1] recipe: ") + \
            "ModelNet40-like whole-to-whole registration, "
    clouds = ("uniform random clouds" if kind == "uniform" else "synthetic object clouds") + \
        " with the reference's transform recipe"
    emb = {"lpdnet": "LPDNet", "dgcnn": "DGCNN", "pointnet": "PointNet"}[a.emb_nn]
    wts = "LPD-pretrained emb_nn + seeded Transformer weights" if a.emb_nn == "lpdnet" else "seeded weights"
    if a.emb_nn == "lpdnet" and a.regime != "default":
        wts = f"weight regime '{a.regime}' (vcrnet_amd.weights.regime_weights)"
    return base + "N=%d, batch=%d pairs per GPU, %s(k=%d)+Transformer+VcpTopK+SVD, iter=%d, fp32; %s; %s" % (
        N, B, emb, a.k, a.iters, clouds, wts)


def setup_rank(a):
    """Process-level setup of one rank: stdout discipline, device, process group.  Returns the context `measure` needs."""
    # stdout carries exactly ONE line, the JSON: libraries that chat on file descriptor 1 (gloo's "Rank 0 is connected
    # ...", RCCL's version banner) are sent to stderr for the life of the process; the line goes out through a copy
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if os.environ.get("VCR_BENCH_HANG_RANK") in (str(rank), "all"):     # fault injection for the deadline tests
        time.sleep(1e6)
    ndev = torch.cuda.device_count()
    if a.backend == "nccl" and world > ndev:
        raise SystemExit(f"{world} ranks but {ndev} GPUs: one process per GPU")
    local = local % max(1, ndev)
    if world > 1:
        # a hung collective must not hang the run: past the deadline every thread's stack goes to stderr
        # (gpurun_out/rank<r>.err when bench.py spawned the ranks) and the process exits non-zero
        import faulthandler
        faulthandler.dump_traceback_later(a.deadline_s, exit=True)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    rccl_log = None
    if world > 1 and rank == 0 and a.backend == "nccl":
        # "RCCL over xGMI only" must be shown, not assumed: rank 0's RCCL writes its INIT / GRAPH debug lines to a file
        # (set before the library initialises) and measure() parses the transports of its channels into multi_gpu.transport
        from vcrnet_amd import shard
        import tempfile
        for logdir in (os.environ.get("VCR_BENCH_LOGDIR", os.path.join(ROOT, "gpurun_out")), tempfile.gettempdir()):
            try:                                                     # (a read-only checkout must not cost the run: the log moves)
                os.makedirs(logdir, exist_ok=True)
                rccl_log = os.path.join(logdir, "rank0.rccl.log")
                with open(rccl_log, "w"):
                    pass
                break
            except OSError:
                rccl_log = None
        if rccl_log:
            for k_, v_ in shard.rccl_debug_env(rccl_log).items():
                os.environ.setdefault(k_, v_)
            rccl_log = os.environ["NCCL_DEBUG_FILE"]
    if world > 1:
        import datetime
        import torch.distributed as dist
        tmo = datetime.timedelta(seconds=a.init_timeout_s)
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(a.backend, timeout=tmo)
    if os.environ.get("VCR_BENCH_FAIL_RANK") == str(rank):     # fault injection for tests/test_hip_multi.py
        print(f"rank {rank}: injected failure", file=sys.stderr, flush=True)
        os._exit(3)

    # (tests: a canned RCCL log stands in for the one a multi-GPU box would write)
    rccl_log = os.environ.get("VCR_BENCH_RCCL_LOG", rccl_log) if rank == 0 else None
    return SimpleNamespace(json_fd=json_fd, world=world, rank=rank, dev=dev, dist=dist, ndev=ndev, rccl_log=rccl_log)


def rccl_version():
    """RCCL's version as this process sees it (torch.cuda.nccl.version() -> the library torch loaded)."""
    try:
        return ".".join(str(x) for x in torch.cuda.nccl.version())
    except Exception as e:          # noqa: BLE001 -- a diagnostic field must not fail the run
        return f"unavailable ({type(e).__name__})"


def measure(a, ctx, min_seconds):
    """One workload (the flags in `a`) on this rank: build the module, warm up, time K-step blocks for `min_seconds`,
    return the JSON line as a dict on rank 0 (None elsewhere)."""
    world, rank, dev, dist = ctx.world, ctx.rank, ctx.dev, ctx.dist
    import vcrnet_amd  # noqa: F401
    from vcrnet_amd import native, shard, synth, weights, workmodel
    from vcrnet_amd.module import VCRNet, vcrnetIter

    w = (weights.regime_weights(a.regime, lpd=weights.load_lpd_fixture()) if a.emb_nn == "lpdnet"
         else weights.generate_weights(1234, emb_nn=a.emb_nn))
    net = VCRNet(model_args(a.partial, a.emb_nn))
    net.load_state_dict(w)
    net.emb_nn.k = a.k
    net.linear_mode = a.linear_mode
    net.merge_encdec = not a.no_merge_encdec
    net.linear_mfma, net.linear_bk, net.knn_waves = a.linear_mfma, a.linear_bk, a.knn_waves
    net.linear_bm = a.linear_bm
    net.sdpa_variant = a.sdpa_variant
    net.iter_reuse = not a.no_iter_reuse
    net = net.to(dev).eval()

    B, N = a.batch, a.points
    if a.strong:
        if a.batch % world:
            raise SystemExit(f"--strong: --batch {a.batch} does not divide over {world} ranks")
        B = a.batch // world
    # each rank owns B consecutive items of the global batch (weak scaling: B = --batch; strong: --batch / ranks);
    # inputs live in HBM
    # object-like clouds have 2048 points (the ModelNet40 convention); larger N (configs 3/4) use uniform clouds
    # built on the device from base clouds + host-drawn permutations / poses (vcr_make_pairs_f32; untimed)
    kind = "object" if N < 2048 else "uniform"
    src, tgt, _, _, _ = synth.make_batch_device(rank * B, B, N, partial=a.partial, kind=kind, device=dev)
    Nfull, N = N, src.shape[2]                     # partial mode crops the clouds (1024 -> 768)
    assert src.shape == (B, 3, N) and src.is_cuda, src.shape

    gather_ev = []            # (start, end) HIP events around the collective, on the stream the forward was enqueued on
    last = {}                 # --dump-outputs: what the latest step returned (references only, nothing is copied)

    def step(trace=None):
        net.launch_trace = trace                # profiling hook of the module: per-launch HIP events on traced steps
        with torch.no_grad():
            out = vcrnetIter(net, src, tgt, iter=a.iters)      # the public entry point SURVEY 8d names (one C call)
        pose = torch.cat((out[2].view(B, 9), out[3]), 1)
        if world > 1:
            if trace is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            pose = shard.all_gather_poses(pose, world)
            if trace is not None:
                e1.record()
                gather_ev.append((e0, e1))
        if a.dump_outputs:
            last.update(out=out, pose=pose)
        return pose

    # one-time initialisation, not a warm-up step: the first call loads the code objects, packs / folds the weights,
    # sizes the workspace and (N > 1) opens the RCCL communicator
    step()
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        step()
    # steps of a block that carry per-launch events -- never the first ones behind the fence (the queue is empty there and
    # the device may have idled: a traced step must look like every other step of the block); --full only
    traced_steps = list(range(min(2, a.steps - 1), a.steps, max(1, a.trace_every))) if a.full else []
    traces = {i: native.LaunchTrace() for i in traced_steps}
    nt = len(traced_steps)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if world > 1:   # sanity: the gathered poses must hold every rank's block in rank order
        g = step()
        mine = g[rank * B:(rank + 1) * B]
        own = step()[rank * B:(rank + 1) * B]
        assert g.shape == (world * B, 12) and torch.allclose(mine, own)

    def timed_block():
        fence()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(traces[i].trace if i in traces else None)
        fence()
        el = time.perf_counter() - t0
        own_blocks.append(el)
        if world > 1:
            tt = torch.tensor([el], dtype=torch.float64, device=dev if a.backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
        return el

    # EXACTLY K steps per block; blocks repeat until min_seconds of load (every rank must agree on the count, so the
    # decision uses the MAX-reduced times, identical on all ranks)
    own_blocks = []
    blocks = [timed_block()]
    while sum(blocks) < min_seconds and len(blocks) < 1000:
        blocks.append(timed_block())
    elapsed = float(np.median(blocks))
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last["out"], last["pose"] if world > 1 else None)
    multi = None
    if world > 1:
        # what the first real 8-GPU run needs to explain itself: every rank's own median step time (before the MAX), the
        # collective's share (HIP events around the all-gather on traced steps; the first records also absorb the wait
        # for the slowest rank), what this rank sees of the machine
        torch.cuda.synchronize()
        ag = [e0.elapsed_time(e1) for e0, e1 in gather_ev]
        mine = torch.tensor([float(np.median(own_blocks)) / a.steps * 1e3, float(np.median(ag)) if ag else 0.0,
                             float(max(ag)) if ag else 0.0], dtype=torch.float64,
                            device=dev if a.backend == "nccl" else "cpu")
        allr = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per = torch.stack(allr).cpu().numpy()
        multi = {"world_size": dist.get_world_size(), "backend": dist.get_backend(),
                 "rccl_version": rccl_version() if a.backend == "nccl" else None,
                 "n_devices_visible": ctx.ndev, "device_of_rank0": torch.cuda.get_device_name(dev),
                 "per_rank_ms_per_step": [round(float(x), 4) for x in per[:, 0]],
                 "per_rank_ms_per_step_min": float(per[:, 0].min()), "per_rank_ms_per_step_max": float(per[:, 0].max()),
                 "all_gather_ms": float(np.median(per[:, 1])), "all_gather_ms_per_rank": [round(float(x), 4) for x in per[:, 1]],
                 "all_gather_ms_worst": float(per[:, 2].max()),
                 "all_gather_timed_with": ("HIP events on the forward's stream around shard.all_gather_poses, traced steps; "
                                           "median per rank, then median over ranks"
                                           + ("" if a.backend == "nccl" else
                                              f"; backend {a.backend}: the poses are staged through the host, so this is a "
                                              "device-to-host copy + a CPU collective, not RCCL"))}
        if not nt:                              # no traced steps (a plain run): the collective was not timed
            for k_ in ("all_gather_ms", "all_gather_ms_per_rank", "all_gather_ms_worst"):
                multi[k_] = None
        # which transport carried the collective (rank 0's RCCL debug log, see setup_rank): xgmi_only is True only when
        # every channel is P2P and the topology RCCL detected lists XGMI links; False as soon as a NET/ or SHM/ transport
        # appears; None when there is no log to read (gloo, or RCCL wrote nothing)
        if ctx.rccl_log:
            from vcrnet_amd import shard
            try:
                with open(ctx.rccl_log, errors="replace") as f:
                    multi["transport"] = dict(shard.parse_rccl_log(f.read()), log=os.path.relpath(ctx.rccl_log, ROOT))
            except OSError as e:
                multi["transport"] = {"xgmi_only": None, "error": f"{type(e).__name__}: {e}"}
        else:
            multi["transport"] = {"xgmi_only": None, "note": "no RCCL log (backend %s)" % a.backend}
        multi["xgmi_only"] = multi["transport"].get("xgmi_only")

    # per-launch durations from the HIP events recorded inside the (last) timed block
    fam_ms, fam_flops, fam_bytes, fam_gather, rows = {}, {}, {}, {}, {}
    for tr in traces.values():
        for name, ms in tr.launches():
            fam = name.split(":")[0]
            fl, by = workmodel.launch_work(name, B, N, a.k, overlap2=net._overlap2)
            gb = workmodel.gather_bytes(name, B, N, a.k)
            fam_ms[fam] = fam_ms.get(fam, 0.0) + ms
            fam_flops[fam] = fam_flops.get(fam, 0.0) + fl
            fam_bytes[fam] = fam_bytes.get(fam, 0.0) + by
            fam_gather[fam] = fam_gather.get(fam, 0.0) + gb
            r = rows.setdefault(name, [0.0, fl, by, 0, gb])
            r[0] += ms; r[3] += 1
        tr.close()
    if rank == 0 and nt:                        # the per-launch figures: only a run with traced steps (--full) has them
        dom = max(fam_ms, key=fam_ms.get)
        bound = workmodel.FAMILY_BOUND[dom]
        if bound == "mfma":
            ach = fam_flops[dom] / (fam_ms[dom] * 1e-3) / 1e12
            peak = workmodel.PEAK_MFMA_F32_TFLOPS
            split = (dom == "linear" and a.linear_mode != "fp32") or (dom == "sdpa" and a.linear_mode == "bf16x3+sdpa")
            if split:
                peak = workmodel.PEAK_MFMA_BF16_TFLOPS / 6.0    # six bf16 MFMA products per fp32-equivalent MAC
            roof = {"bound": "mfma", "kernel": dom, "achieved": ach, "peak": peak,
                    "unit": "TFLOP/s", "frac": ach / peak, "traffic": None}
            if not split:
                # what a register-only fp32 MFMA loop holds on all 256 CUs after 2 s of load, with the shader clock read inside the
                # kernel (round 4, three boxes): the pipe is NOT power-limited -- `frac` above is priced against the nominal peak
                roof["peak_recorded"] = {"register_only_mfma_loop": 153.5, "unit": "TFLOP/s", "shader_clock_ghz": 2.39,
                                         "source": "profiles/rounds4-5/r4c_mfma_f32_clock.txt",
                                         "note": "a RECORDED constant (round 4, two boxes, 2 s of load), not measured in this run: "
                                                 "the same kernels ran at 2.15-2.38 GHz from run to run on one box"}
            if split:
                roof["note"] = "fp32-equivalent FLOPs; peak = 2500 TFLOP/s dense bf16 / 6 MFMAs per split product"
        else:
            ach = fam_bytes[dom] / (fam_ms[dom] * 1e-3) / 1e9
            roof = {"bound": "hbm", "kernel": dom, "achieved": ach, "peak": workmodel.PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": ach / workmodel.PEAK_HBM_GBS, "traffic": None}
        # HBM traffic per launch of that kernel comes from SEPARATE rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE)
        # of this same command, condensed by profiles/summarize.py; null when no summary is committed.
        import glob
        from vcrnet_amd import build as vb

        def _pmc_rank(path):                               # the summary taken on THIS build's kernel sources, else the latest one
            meta = json.load(open(path)).get("_meta", {})
            return (meta.get("kernel_sources_sha16") == vb.sources_sha16(), meta.get("date_utc", ""), path)
        # (summaries of the exact-split line carry "bf16x3" in their name: each arithmetic mode reads its own passes)
        pmcs = sorted((p_ for p_ in glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary.json"))
                       if ("bf16x3" in os.path.basename(p_)) == (a.linear_mode != "fp32")), key=_pmc_rank)
        if pmcs and (B, N, a.k, a.partial, a.iters, a.emb_nn) == (16, 1024, 20, False, 1, "lpdnet"):
            kname = {"linear": "linear_glds" if a.linear_mode == "fp32" else "linear_bf16x3_kernel",
                     "sdpa": "sdpa_persist_kernel" if a.linear_mode != "bf16x3+sdpa" else "sdpa_bf16x3_kernel",
                     "edgeconv": "edgeconv_dg_pipe_kernel<20>", "softcorr": "pairscore_kernel<0>"}.get(dom)
            # a family can be several template instantiations (linear: plain / statistics-out / LayerNorm-in):
            # launch-weighted mean over the entries whose name starts with the family's kernel name
            ents = [e for k_, e in json.load(open(pmcs[-1])).items()
                    if kname and k_.startswith(kname) and isinstance(e, dict) and "hbm_bytes_per_launch" in e]
            if ents:
                nd = [e["FETCH_SIZE"]["dispatches"] for e in ents]
                roof["traffic"] = sum(e["hbm_bytes_per_launch"] * n for e, n in zip(ents, nd)) / sum(nd)
                roof["traffic_source"] = os.path.relpath(pmcs[-1], ROOT)
                # were those counters taken on this code?  (the summary records a hash of csrc/ + include/; no .git on the box)
                meta = json.load(open(pmcs[-1])).get("_meta", {})
                roof["traffic_source_kernel_sources"] = (
                    "identical to this build" if meta.get("kernel_sources_sha16") == vb.sources_sha16() else
                    "summary taken on kernel sources %s, this build is %s: the counters predate later kernel commits"
                    % (meta.get("kernel_sources_sha16", "(unrecorded)"), vb.sources_sha16()))
        total_ms = sum(fam_ms.values())
        roof["launches_per_step"] = sum(r[3] for n, r in rows.items() if n.startswith(dom + ":")) // nt
        roof["avg_launch_ms"] = fam_ms[dom] / max(1, roof["launches_per_step"] * nt)
        roof["timed_with"] = f"HIP events on {nt} of the {a.steps} steps of the last timed block"
        # gbs = HBM-compulsory bytes (each distinct row once) over the launch time; l2_gather_gbs = the k-fold
        # neighbour re-reads the EdgeConv kernels pull through L2 -- or, gathermax at the path's sizes, out of LDS -- (not
        # HBM traffic: never priced against 8 TB/s)
        stages = {f: {"ms_per_step": fam_ms[f] / nt, "share": fam_ms[f] / total_ms,
                      "tflops": fam_flops[f] / (fam_ms[f] * 1e-3) / 1e12, "gbs": fam_bytes[f] / (fam_ms[f] * 1e-3) / 1e9,
                      **({"l2_gather_gbs": fam_gather[f] / (fam_ms[f] * 1e-3) / 1e9} if fam_gather[f] else {})}
                  for f in sorted(fam_ms, key=fam_ms.get, reverse=True)}
        # the kNN + EdgeConv (emb_nn) stage that BASELINE.json's north_star prices against the HBM roofline:
        # algorithmic bytes 2*N*(7448 + 784*k) per pair AND PER ITERATION (kernel-boundary traffic,
        # gathers included), time = its launches inside the timed region (all iterations)
        emb_sites = ("pointwise:", "knn:", "edgeconv:", "gathermax:", "linear:dg1_pq", "linear:sn1_pq", "linear:conv3",
                     "linear:dg_c")
        emb_ms = sum(r[0] for n, r in rows.items() if n.startswith(emb_sites)) / nt
        # (vcrnetIter with target reuse: the passes after the first run this stage on the SOURCE clouds only -- the algorithmic
        #  bytes count the clouds the launches really processed, 2 per pair in the first pass and 1 in each later one)
        reuse = a.iters > 1 and a.emb_nn == "lpdnet" and bool(getattr(net, "iter_reuse", False)) and any(n.endswith("@src") for n in rows)
        clouds = (2 + (a.iters - 1)) if reuse else 2 * a.iters
        emb_bytes = 1.0 * N * (7448 + 784 * a.k) * B * clouds
        emb_gf = 0.5 * clouds * sum(workmodel.launch_work(n, B, N, a.k)[0] for n in
                               ("linear:dg1_pq", "edgeconv:dg1_dg2", "linear:sn1_pq", "linear:conv3")) / 1e9
        emb_stage = None if a.emb_nn != "lpdnet" else {"ms_per_step": emb_ms, "algorithmic_bytes_per_pair": emb_bytes / B / a.iters, "iters": a.iters,
                     "clouds_processed_per_pair": clouds,
                     "achieved_gbs": emb_bytes / (emb_ms * 1e-3) / 1e9,
                     "hbm_frac": emb_bytes / (emb_ms * 1e-3) / 1e9 / workmodel.PEAK_HBM_GBS,
                     "knn_ms_per_step": sum(r[0] for n, r in rows.items() if n.startswith("knn:")) / nt,
                     "note": "fp32 1x1 convs of this stage are MFMA-bound (SURVEY section 7): %.1f GF per step alone "
                             "need %.2f ms at the fp32 matrix peak, i.e. <= %.2f of the HBM roofline"
                             % (emb_gf, emb_gf / workmodel.PEAK_MFMA_F32_TFLOPS,
                                emb_bytes / (emb_gf / workmodel.PEAK_MFMA_F32_TFLOPS * 1e-3) / 1e9 / workmodel.PEAK_HBM_GBS)}
        if a.stages:
            for n, r in sorted(rows.items(), key=lambda kv: -kv[1][0]):
                ms = r[0] / r[3]
                print(f"{n:28s} {ms:8.3f} ms  {r[1] / ms / 1e9:8.2f} TF/s  {r[2] / ms / 1e6:9.1f} GB/s"
                      + (f"  (+{r[4] / ms / 1e6:8.1f} GB/s neighbour gathers, L2 / LDS)" if r[4] else ""), file=sys.stderr)
    if rank == 0:
        if not nt:                              # (with traces, `reuse` also checks that the launches ran on the source alone)
            reuse = a.iters > 1 and a.emb_nn == "lpdnet" and bool(getattr(net, "iter_reuse", False))
        pairs = B * world * a.steps
        line = {
            "metric": "point-cloud pairs/sec (N=%d, batch %d per GPU)" % (Nfull, B) if not a.strong else
            "point-cloud pairs/sec (N=%d, global batch %d over %d GPU(s))" % (Nfull, a.batch, world), "value": pairs / elapsed, "unit": "pairs/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if a.strong else "weak", "vs_baseline": None,
            "dtype": {"fp32": "f32", "bf16x3": "f32 (linears as exact bf16x3 splits, fp32 accumulate)",
                      "bf16x3+sdpa": "f32 (linears and attention as exact bf16x3 splits, fp32 accumulate)"}[a.linear_mode],
            "data": "synthetic",
            "config": {"workload": workload_label(a, Nfull, N, B, kind, world),
                       "num_points": N, "batch_per_gpu": B, "global_batch": B * world, "k": a.k, "iters": a.iters,
                       "parallelism": f"dp{world} (pairs sharded per rank" + (
                           ")" if world == 1 else ", RCCL all-gather of R,t)" if a.backend == "nccl" else
                           f", {a.backend} all-gather of R,t staged through the host -- NOT RCCL)"),
                       "entry_point": "vcrnet_amd.module.vcrnetIter(net, src, tgt, iter) -> vcr_vcrnet_iter_f32",
                       **({"iter_target_reuse": "the target cloud does not change between the passes of one vcrnetIter call: what the "
                           "first pass computes from it alone (its embedding, the encoder and the decoder's first sublayer on its "
                           "rows, its K | V projection) is kept for the later passes of THAT call -- nothing is carried from one "
                           "timed step to the next; bit-identical to recomputing (--no-iter-reuse)"} if reuse else {})},
            "timed_blocks": {"count": len(blocks), "steps_per_block": a.steps, "reported": "median",
                             "seconds": [round(b, 6) for b in blocks[:64]],
                             "per_launch_events": f"steps {traced_steps} of every block (a step that carries the ~35 event "
                                                  "records runs ~2 % longer: the stage times sum to that step, not to ms_per_step)"
                                                  if nt else "none (--full records them)"},
        }
        if nt:
            line.update({
                "roofline": roof,
                # the traced launches' HIP-event durations, summed, over the timed block's ms_per_step: what share of a step the
                # launch table explains.  Below ~0.97 the steps are not back-to-back kernels (host-bound enqueue, idle gaps) or
                # traced steps run at another clock than untraced ones -- the per-launch rates then overstate the steady state
                "accounted_frac": (total_ms / nt) / (elapsed / a.steps * 1e3),
                "stages": stages,
                "flops_per_pair_reference": workmodel.reference_flops_per_pair(N, a.k)["total"],
            })
            if emb_stage is not None:      # the stage BASELINE prices exists only for the kNN-graph LPDNet embedding
                line["knn_edgeconv_stage"] = emb_stage
        if multi is not None:
            line["multi_gpu"] = multi
        line["_weights"], line["_Nfull"], line["_B"] = w, Nfull, B          # for the caller's CPU baseline; stripped
        return line
    return None


DUMP_BYTES = 64 << 20
DUMP_NAMES = ("src_k", "corr_k", "rotation_ab", "translation_ab", "rotation_ba", "translation_ba")   # vcrnetIter's returns


def dump_outputs(path, out, pose_all=None):
    """--dump-outputs: vcrnetIter's six returns of the last timed step (and, N > 1, the poses gathered over the ranks) as
    <path>/<name>.npy, float32 / float64 as computed (integer tensors as float64).  Outputs beyond DUMP_BYTES in all are
    thinned to a fixed, seeded sample of their flat elements (written with its indices, <name>.index.npy)."""
    os.makedirs(path, exist_ok=True)
    arrs = {n: t for n, t in zip(DUMP_NAMES, out) if t is not None}
    if pose_all is not None:
        arrs["poses_all_ranks"] = pose_all
    arrs = {n: t.detach().cpu().numpy() for n, t in arrs.items()}
    arrs = {n: v if v.dtype in (np.float32, np.float64) else v.astype(np.float64) for n, v in arrs.items()}
    share = DUMP_BYTES // (2 * len(arrs)) - 128    # a sampled array also writes its indices; 128 = an .npy header
    for n, v in arrs.items():
        if v.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(v.size, share // 8, replace=False))
            np.save(os.path.join(path, n + ".index.npy"), idx.astype(np.float64))
            v = v.reshape(-1)[idx]
        np.save(os.path.join(path, n + ".npy"), v)


# the BASELINE configs that are not the headline, and the labelled split-arithmetic line, as bench.py flag overrides
OTHER_CONFIGS = [
    ("configs[2]", dict(partial=True, points=1024, batch=24, iters=3)),
    # the same with every pass recomputing both clouds, as the reference's loop does (the default reuses, inside ONE
    # vcrnetIter call, what the first pass computed from the unchanged target cloud; bit-identical; nothing crosses a step)
    ("configs[2], --no-iter-reuse", dict(partial=True, points=1024, batch=24, iters=3, no_iter_reuse=True)),
    ("configs[3] (one GPU's share)", dict(points=2048, batch=16)),
    ("configs[4]", dict(points=4096, k=40, batch=32)),
    ("configs[1], --linear-mode bf16x3+sdpa", dict(linear_mode="bf16x3+sdpa")),
]


def is_headline(a):
    d = parse([])
    return all(getattr(a, k) == getattr(d, k) for k in ("gpus", "batch", "points", "k", "partial", "iters", "emb_nn", "strong", "regime",
                                                        "linear_mode", "linear_mfma", "linear_bk", "linear_bm", "knn_waves", "sdpa_variant", "no_iter_reuse",
                                                        "no_merge_encdec"))


def run_rank(a):
    ctx = setup_rank(a)
    line = measure(a, ctx, a.min_seconds)
    if ctx.rank == 0:
        w, Nfull, B = line.pop("_weights"), line.pop("_Nfull"), line.pop("_B")
        if ctx.world == 1 and is_headline(a) and a.full and not a.no_other_configs:
            # measured AFTER the headline (which is untouched by them), same process, same protocol, shorter blocks
            others = []
            for tag, over in OTHER_CONFIGS:
                b = argparse.Namespace(**vars(a))
                for k_, v_ in over.items():
                    setattr(b, k_, v_)
                b.stages, b.dump_outputs = False, None
                t0 = time.perf_counter()
                o = measure(b, ctx, a.other_seconds)
                for k_ in ("_weights", "_Nfull", "_B"):
                    o.pop(k_)
                r = o["roofline"]
                others.append({"baseline_config": tag, "workload": o["config"]["workload"], "value": o["value"],
                               "unit": o["unit"], "ms_per_step": o["ms_per_step"], "steps": o["steps"],
                               "timed_blocks": o["timed_blocks"]["count"], "dtype": o["dtype"],
                               "roofline": {k_: r[k_] for k_ in ("kernel", "bound", "achieved", "peak", "unit", "frac")},
                               "accounted_frac": o["accounted_frac"],
                               **({"iter_target_reuse": True} if "iter_target_reuse" in o["config"] else {}),
                               "knn_edgeconv_stage": {k_: o["knn_edgeconv_stage"][k_] for k_ in
                                                      ("ms_per_step", "hbm_frac", "achieved_gbs", "knn_ms_per_step")},
                               "wall_s": round(time.perf_counter() - t0, 2)})
                torch.cuda.empty_cache()
            line["other_configs"] = others
        if a.full:
            line["parity_ledger"] = parity_ledger(a.linear_mode)
        if ctx.world == 1 and a.full and not a.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(w, B, Nfull, a.k, a.partial, a.iters, a.cpu_budget_s, a.cpu_baseline_full)
        os.write(ctx.json_fd, (json.dumps(line) + "\n").encode())
    if ctx.world > 1:
        ctx.dist.barrier()
        ctx.dist.destroy_process_group()


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(a))               # plain `python bench.py --gpus N`: this process only launches the ranks
    run_rank(a)


if __name__ == "__main__":
    main()
