#!/usr/bin/env python3
"""bench.py — headline benchmark of the SAC-COT hot path on MI355X (contract: see the task brief / DESIGN.md §6).

    python bench.py --gpus N --steps K --warmup W [--config C2] [--scaling weak|strong] [--shard ab|replicated]
                    [--dump-outputs DIR] [--full]
    (N > 1: launched by the driver as  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...)

A plain run sets up, warms up, times the K steps and prints the headline line (`value`, `ms_per_step`, the workload, how the
timed frames ran).  `--full` adds everything else this script measures or checks, in the same line: the waited form, the
identical-frame and 256-frame streams, per-stage brackets and rooflines and, on one GPU, the cold call, host I/O, varying-n,
no-dense-S, native multi-device and calls-in-flight legs, the CPU baseline and the parity of every scene with the CPU restatement.
`--dump-outputs DIR` writes what the last timed step delivered to its caller (R.npy, t.npy, mask.npy, winner.npy) after the timed
steps; the scenes are seeded, so two builds can be compared output for output.

A *step* is one full pass of the hot path over one synthetic correspondence set already resident in HBM:
stage A (compat graph) -> B (top-T triangles) -> C1 (Kabsch) -> C2 (score + arg-max) -> C3 (winner + inlier mask).
Workload at N = 1: BASELINE.json configs[2] ("3DMatch indoor pair, N~5k correspondences, 50k triangles, 1xMI355X") —
the configuration BASELINE.json's `metric` is quoted on ("N=5k corrs") — as a synthetic scene of that shape (the
reference ships no data).

N > 1 (one process per GPU, RCCL through torch.distributed "nccl"), `--shard ab` (the default for strong scaling
and for graphs of 8192 correspondences and more, see --shard): stage A by row
blocks, stage B by contiguous row ranges, stage C by blocks of the merged list; four collectives per step — all-gather
of the bit rows, 1 KiB all-reduce of the pruning-sample histogram, all-gather of the candidate blobs, all-gather of
the 16-byte winner key pairs.  `--shard replicated` is round 1's form (A and B on every rank, one or two collectives).
`--scaling weak` (default; what the driver's N = 1, 2, 4, 8 sweep runs): every GPU scores the config's T triangles of
the SAME scene, T_total = T x N.  `--scaling strong`: T_total = the config's T, so `--config C3 --gpus 8 --scaling
strong` is BASELINE configs[3] as specified (200k triangles over 8 GPUs) and C4 likewise.

`value` = hypotheses scored per second by the whole job = T_total * K / wall time of the K timed steps (barrier +
synchronize on both sides, MAX over ranks): the end-to-end rate, stages A, B and the mask included.
The K steps are a STREAM of DISTINCT frames (r05: --scenes 32 device-resident scenes of the config's shape whose inlier ratio —
hence edge and triangle counts — differs from frame to frame; frame f registers scene f mod 32) and --frames-in-flight 2 (r04c; one
rank, or ranks that replicate stages A and B): step k + 1 is enqueued before the host waits for step k's winner, the way a
registration pipeline feeds the library; every step runs every kernel on its inputs and delivers its winner, statistics, (R, t) and
mask like any other call, and every frame's outputs are compared with the waited form's and (checker leg) with the CPU restatement
of its scene.  `how_the_timed_frames_ran` counts the frames the library had to repeat inside the timed region.  The form of rounds
1 - 3 (a step begins when the previous winner has reached the host: ~19 us of idle GPU per step) is timed right after it over the
same frames and reported as `waited`; round 4's headline form (one scene repeated) as `stream_identical_frames`; `stream_long`
runs the distinct stream over 256 frames for the rates of the fallbacks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3   # same guide: fp32 vector peak = dense f32-input MFMA peak
F16_MFMA_PEAK_TFLOPS = 2500.0  # same guide: BF16 / FP16 MFMA, ~2.5 PF dense (the F16 forms take the BF16 forms' cycles)
STAGES = ("stage", "compat", "triangles", "kabsch", "score", "argmax", "mask")


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


import contextlib


@contextlib.contextmanager
def stdout_to_stderr():
    """fd 1 -> fd 2 while a library that prints to stdout is at work (RCCL announces its version there when a
    communicator is created): stdout carries exactly one JSON line."""
    sys.stdout.flush()
    keep = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(keep, 1)
        os.close(keep)


GPU_CLOCK_HZ = 2.4e9       # same guide: peak engine clock
N_SIMD = 256 * 4


def executed_tests(n: int, info: dict) -> float:
    """(hypothesis, correspondence) pairs the Gram filter's launch really evaluates (sc_debug_last): rows near the call's reference
    frame walk the near correspondences only (whole 256-correspondence units), the others every unit of the padded list."""
    near_units = (info["gram_near_corr"] + 255) // 256
    n_pad = ((n + 1023) // 1024) * 1024
    return float(info["gram_near_hyp"]) * near_units * 256 + float(info["gram_rows"] - info["gram_near_hyp"]) * n_pad


def issue_model(n: int, n_local: int, us: float, info: dict) -> dict:
    """The C2 filter kernel against its OWN issue limits, so that `roofline.frac` — an fp32-EQUIVALENT rate —
    is not read as a utilisation.  A step = the MFMAs that produce one accumulator tile plus the vector instructions that
    consume it:  linear filter: 1 MFMA (8 hypotheses x 32 correspondences, 256 tests), 26 vector instructions on the path
    without an undecided test;  Gram filter: 3 chained MFMAs (32 hypotheses x 32 correspondences, 1024 tests), 29.
    `cycles_per_step`: measured — duration of the whole C2 stage x the NOMINAL clock / steps per SIMD (it includes the exact
    pass, set-up and tail; under this load the chip holds 1.9 - 2.1 GHz, so real cycles are ~15 % fewer).
    `bound_matrix_cycles`: 32 cycles per MFMA.  `bound_vector_cycles`: the SIMD's issue port — 8 cycles per MFMA + 4 per vector
    instruction (MI355X_MICROARCH.md, 'costs add'); profiles/r03_pmc_gram_variants_C4.txt: the Gram kernel really issues 44 vector
    instructions per step (queueing of undecided tests, staging, per-wave set-up on top of the 29) and its duration moves by
    4.6 cycles per instruction added or removed — it is bound by that port, not by the matrix pipe."""
    gram = info.get("c2_kernel") == 2
    windows = (n + 1023) // 1024
    hyp_per_wave, mfma_per_step, valu = (32, 3, 29.0) if gram else (8, 1, 26.0)
    steps = (n_local / float(hyp_per_wave)) * windows * 32          # accumulator tiles of the launch
    if gram and info.get("gram_rows"):                               # the cut: the tiles the launch really evaluates
        steps = executed_tests(n, info) / (32.0 * hyp_per_wave)
    per_simd = steps / N_SIMD
    cyc = us * 1e-6 * GPU_CLOCK_HZ / max(per_simd, 1.0)
    matrix = 32.0 * mfma_per_step
    vector = 8.0 * mfma_per_step + 4.0 * valu
    bound = max(matrix, vector)
    return {"filter": "gram" if gram else "linear", "tests_per_step": 32 * hyp_per_wave, "cycles_per_step": round(cyc, 1),
            "mfma_per_step": mfma_per_step, "valu_per_step": valu, "bound_matrix_cycles": matrix,
            "bound_vector_cycles": round(vector, 1), "frac_of_issue_bound": round(bound / cyc, 3),
            "clock_hz_nominal": GPU_CLOCK_HZ, "undecided_entries": info.get("filter_undecided"),
            "recounts": info.get("filter_recounts")}


def dump_outputs(d: str, Rt, mask, rc: int, st: dict) -> None:
    """--dump-outputs: the outputs of the last timed step as its caller receives them — (R, t) and the inlier mask from device
    memory, the winner (status, rank of the winning hypothesis, its inlier count) from the returned statistics."""
    os.makedirs(d, exist_ok=True)
    Rt = Rt.cpu().numpy()
    np.save(os.path.join(d, "R.npy"), Rt[:9].reshape(3, 3))
    np.save(os.path.join(d, "t.npy"), Rt[9:].copy())
    np.save(os.path.join(d, "mask.npy"), mask.cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "winner.npy"), np.array([rc, st["best_rank"], st["best_count"]], dtype=np.float64))


def spawn_ranks(n: int, deadline_s: float = 1500.0) -> int:
    """`python bench.py --gpus N` started WITHOUT a launcher (WORLD_SIZE unset): start the N ranks as fresh child
    processes — this parent has not touched the GPU (torch is not even imported yet) and never does; no re-exec.  The
    children get the environment torch.distributed.run would give them; rank 0 prints the one JSON line, which passes
    through; the exit code is the worst of the children's.
    The children are SUPERVISED: a rank that dies early (import error, HIP initialisation, an assert) would
    leave its peers blocked in the rendezvous or in a collective until the backend's own timeout — minutes of a held GPU
    lease and no JSON line.  So the parent polls all of them; on the first non-zero exit, or at the overall deadline, the
    others are terminated (killed after a grace period) and that code is returned.  The rendezvous port is picked by
    bind-then-close, which another process can take before rank 0 binds it: a start that fails within the first seconds with
    an address-in-use message on rank 0's stderr is repeated once on a fresh port."""
    import socket
    import subprocess
    import tempfile
    import time

    def free_port() -> int:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            return sk.getsockname()[1]

    def stop(procs) -> None:
        for pr in procs:
            if pr.poll() is None:
                pr.terminate()
        t_end = time.monotonic() + 10.0
        for pr in procs:
            try:
                pr.wait(timeout=max(0.1, t_end - time.monotonic()))
            except subprocess.TimeoutExpired:
                pr.kill()
                pr.wait()

    for attempt in range(2):
        port = free_port()
        procs, errs = [], []
        t0 = time.monotonic()
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            # rank 0's stderr goes through a file so that an address-in-use failure can be recognised; it is replayed below
            ef = tempfile.TemporaryFile(mode="w+b") if r == 0 else None
            errs.append(ef)
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stderr=ef if ef is not None else None))
        rc = 0
        while True:
            codes = [pr.poll() for pr in procs]
            bad = [abs(c) for c in codes if c not in (None, 0)]
            if bad:
                rc = max(bad)
                stop(procs)
                break
            if all(c == 0 for c in codes):
                break
            if time.monotonic() - t0 > deadline_s:
                print(f"bench.py: ranks still running after {deadline_s:.0f} s: terminating them", file=sys.stderr)
                stop(procs)
                rc = 124
                break
            time.sleep(0.05)
        text = b""
        if errs[0] is not None:
            errs[0].seek(0)
            text = errs[0].read()
            errs[0].close()
        in_use = rc != 0 and time.monotonic() - t0 < 60.0 and (b"EADDRINUSE" in text or b"ddress already in use" in text)
        if in_use and attempt == 0:
            print("bench.py: the rendezvous port was taken before rank 0 bound it: starting the ranks once more", file=sys.stderr)
            continue
        sys.stderr.buffer.write(text)
        sys.stderr.flush()
        return rc
    return 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="C2", help="synthetic scene template (default: the headline config C2)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--shard", choices=("auto", "ab", "replicated"), default="auto",
                    help="N > 1: shard stages A and B too (ab) or replicate them (round 1's form); auto = ab from 8192 correspondences "
                         "on, replicated below: there one rank's emulated step is 0.219 / 0.232 / 0.256 ms replicated (stage B pruned "
                         "by the estimated bound) against 0.271 / 0.276 / 0.305 ms sharded at 2 / 4 / 8 ranks weak-scaling C2, 0.329 / "
                         "0.283 / 0.270 against 0.378 / 0.316 / 0.318 strong-scaling C4 (profiles/r04_emulated_world_scaling.txt, copies "
                         "standing in for the collectives), and the replicated form needs one 16-byte collective per step instead of three")
    ap.add_argument("--frames-in-flight", type=int, choices=(1, 2), default=2,
                    help="2 (default) = a STREAM of frames — step k + 1 is enqueued (sc_register_device_async; replicated ranks: host-free "
                         "sc_hypothesize_device + all-gather + sc_finalize_gathered_device_async; a second context on the same stream) before "
                         "step k's winner is waited for (sc_wait), so the GPU runs the steps back to back; 1 = every step ends with its winner "
                         "on the host before the next begins (rounds 1 - 3; still reported as `waited`).  --shard ab waits every step")
    ap.add_argument("--scenes", type=int, default=32,
                    help="distinct synthetic scenes of the config's shape the frames cycle through (seeds cfg.seed + k, inlier ratio drawn "
                         "in [2/3, 4/3] of the config's: C2 0.10 .. 0.20, so edge counts move by ~1.6 x and triangle counts by ~4 x from "
                         "frame to frame); frame f registers scene f mod SCENES.  1 = every frame the config's own scene (rounds 1 - 4)")
    ap.add_argument("--hot-timing-every", type=int, default=8,
                    help="SC_FLAG_TIMING_HOT (the dominant kernel's duration from its dispatch packets' timestamps) on every N-th timed frame (0: none)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline (see the module docstring); a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the last timed step's (R, t), inlier mask and winner as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline or CPU parity")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: only the timed loop and the per-stage passes (no cold call, host-I/O, varying-N, no-dense-S or CPU "
                         "legs): what the rocprofv3 kernel-stats and PMC passes profile")
    ap.add_argument("--no-dense-s", action="store_true", help="SC_FLAG_NO_DENSE_S in the timed loop (bit rows only)")
    ap.add_argument("--debug", default="", help="sc_debug knobs for experiments: key=value,key=value")
    ap.add_argument("--split-sample", choices=("auto", "on", "off"), default="auto",
                    help="--shard replicated only: on = shard stage B's CERTIFYING pruning sample (one extra 1 KiB all-reduce); auto / off: every rank takes the whole ESTIMATING sample (SC_FLAG_EST_BOUND)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args.gpus)
    if os.environ.get("SC_BENCH_SUPERVISION_TEST") and "WORLD_SIZE" in os.environ:
        # tests/test_shard_gloo.py: rank 1 dies at once, the others would wait for it forever — the parent must end them
        if int(os.environ.get("RANK", "0")) == 1:
            return 7
        __import__("time").sleep(3600)

    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge
    pkg = ge.load_package()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch one rank per GPU", file=sys.stderr)
        return 2
    # SC_BENCH_REHEARSAL=1: every rank on cuda:0 over gloo — runs the whole N > 1 code path on a one-GPU box; its
    # timings mean nothing (RCCL is not in it).  (Read by this script, not by the library.)
    rehearsal = os.environ.get("SC_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)  # "nccl" is RCCL on ROCm

    cfg, scenes = pkg.synth.make_stream_scenes(args.config, max(1, args.scenes))
    scene, K = scenes[0], len(scenes)   # scenes[0] is the config's own scene (what the stage passes, the CPU baseline and the other legs use)
    T_total = cfg.T * world if args.scaling == "weak" else cfg.T
    kw = cfg.params()
    kw["max_triangles"] = T_total
    block = max(64, min(1000, T_total // (world * 8)))       # blocks of the selected list dealt round-robin
    base_flags = pkg.SC_FLAG_NO_DENSE_S if args.no_dense_s else 0
    knobs = dict(kv.split("=") for kv in args.debug.split(",") if kv)

    def mk(flags):
        return pkg.make_params(shard_rank=rank, shard_world=world, shard_block=block, flags=base_flags | flags, **kw)

    # ---- cold call: a fresh context, host arrays in, outputs back (workspace allocation, first launches) ----------
    cold_ms = None
    if world == 1 and args.full and not args.headline_only:
        r0 = pkg.Registrar(local_rank)
        tc = time.perf_counter()
        r0.register(scene.src, scene.tgt, params=pkg.make_params(flags=base_flags, **kw))
        cold_ms = (time.perf_counter() - tc) * 1e3
        r0.close()

    reg = pkg.Registrar(local_rank)  # raises without the HIP library / a GPU: there is no fallback
    if knobs:
        reg.set_debug(**{k: int(v) for k, v in knobs.items()})
    reg.set_stream(torch.cuda.current_stream().cuda_stream)  # same stream as torch, so the collectives are ordered
    d_srcs = [torch.from_numpy(sc_.src).to(dev) for sc_ in scenes]
    d_tgts = [torch.from_numpy(sc_.tgt).to(dev) for sc_ in scenes]
    d_src, d_tgt = d_srcs[0], d_tgts[0]
    torch.cuda.synchronize()

    # auto: A and B sharded too (phase API, three or four collectives per step) on graphs of 8192 correspondences and more; below,
    # the replicated form — every rank runs the single-GPU stages A and B for the job's T, pruned by the estimated bound
    # (SC_FLAG_EST_BOUND on sc_hypothesize_device, r04b), and scores its share: ONE 16-byte all-gather per step.  Emulated per-rank
    # step, replicated against sharded: C2 weak 0.219 / 0.232 / 0.256 ms at 2 / 4 / 8 ranks against 0.271 / 0.276 / 0.305; C4 strong
    # 0.329 / 0.283 / 0.270 against 0.378 / 0.316 / 0.318; C3 (20 000 correspondences) strong at 8: 0.86 against 0.55 — sharded there.
    sharded_ab = world > 1 and (args.shard == "ab" or (args.shard == "auto" and cfg.n >= 8192))
    split = (not sharded_ab) and args.split_sample == "on"   # (auto: the estimated bound instead — every rank takes the whole, cheap sample)
    rep_est = [True]   # replicated form: stage B pruned by the estimated bound until it fails once
    if sharded_ab:
        ss = pkg.shard.ShardedStep(pkg, reg, cfg.n, mk(pkg.SC_FLAG_TIMING_HOT), rank, world, dev)
        d_Rt, d_mask = ss.Rt, ss.mask

        def step(prm, k=0):
            return ss.step(d_srcs[k % K].data_ptr(), d_tgts[k % K].data_ptr(), prm)
    else:
        d_key = torch.zeros(2, dtype=torch.int64, device=dev)  # winner key pair (include/saccot.h)
        d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
        d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
        d_hist = torch.zeros(pkg.SC_HIST_WORDS, dtype=torch.int32, device=dev)
        d_all = torch.zeros(2 * world, dtype=torch.int64, device=dev)  # every rank's key pair (one all-gather)

        def step(prm, k=0, g=None, Rt=None, mask=None):
            """one frame (scene k mod K), complete on return: its winner is on the host"""
            g = g or reg
            Rt = d_Rt if Rt is None else Rt
            mask = d_mask if mask is None else mask
            ps, pt = d_srcs[k % K].data_ptr(), d_tgts[k % K].data_ptr()
            if world == 1:
                # the drop-in entry with everything resident in HBM: sc_register_device (a repeated shape is enqueued without a
                # host wait in the middle of the call — include/saccot.h; `fast_path` below says how the timed calls ran)
                return g.register_device(ps, pt, cfg.n, prm, Rt.data_ptr(), mask.data_ptr())
            if split:
                g.hypothesize_begin_device(ps, pt, cfg.n, prm, d_hist.data_ptr())
                pkg.shard.allreduce_hist(d_hist)
                g.hypothesize_end_device(d_hist.data_ptr(), d_key.data_ptr())
                pkg.shard.allgather_best(d_key, d_all)
                return g.finalize_gathered_device(d_all.data_ptr(), world, Rt.data_ptr(), mask.data_ptr())
            # stages A and B replicated, stage B pruned by the ESTIMATED bound (SC_FLAG_EST_BOUND, r04b: what sc_register_device does
            # on one GPU): every rank runs the same deterministic stages on the same scenes in the same order, so every rank gets
            # SC_EBOUND together — the select found the bound too high, or (a host-free call) a count outgrew what the launches
            # covered: this frame again without the flag; estimates that FAIL twice switch the flag off for good
            def run(q):
                g.hypothesize_device(ps, pt, cfg.n, q, d_key.data_ptr())
                pkg.shard.allgather_best(d_key, d_all)  # ONE collective (16 bytes per rank); the reduction runs in the kernel
                return g.finalize_gathered_device(d_all.data_ptr(), world, Rt.data_ptr(), mask.data_ptr())

            q = type(prm).from_buffer_copy(prm)
            if rep_est[0]:
                q.flags |= pkg.SC_FLAG_EST_BOUND
            rc, st_ = run(q)
            if rc == pkg.SC_EBOUND:     # (only with the flag)
                note_ebound(g)
                rc, st_ = run(prm)
            return rc, st_

    est_fails = [0]

    def note_ebound(g):
        """SC_EBOUND came back: was it the ESTIMATE (sc_debug_last.prune_bound == 2) or a host-free call's cover?  (Off the fast path:
        sc_debug_last synchronises.  Deterministic and the same on every rank: stages A and B are replicated.)"""
        if g.debug_last()["prune_bound"] == 2:
            est_fails[0] += 1
            if est_fails[0] >= 2:
                rep_est[0] = False

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    p_hot = mk(pkg.SC_FLAG_TIMING_HOT)
    p_plain = mk(0)
    HE = max(0, args.hot_timing_every)

    def p_of(f):   # SC_FLAG_TIMING_HOT on every HE-th timed frame: the flag's two dispatch-packet timestamps are not free
        return p_hot if HE and f % HE == 0 else p_plain
    W = args.warmup
    # Warm-up: the W frames BEFORE frame 0 of the cycle (scenes K - W .. K - 1), so that no timed frame repeats the frame its context
    # saw last.  No fallback of any kind: a failure here is the result (every rank runs the same sequence of collectives, so an
    # exception on one rank must end the job, not change that rank's path).
    for i in range(W):
        step(p_hot, K - W + i)
    hot_score = 0.0
    n_hot = [0]
    n_hot_timed = 0
    # The interpreter's cyclic garbage collector stays out of every timed region of this process: a generation-2 pass costs ~40 ms
    # here — 170 steps' worth — and landed in the varying-n leg in round 4 (20 calls: 2.4 ms per call on average, median 0.24).  Nothing the
    # timed code allocates is cyclic; what exists so far is frozen, reference counting keeps freeing the rest.
    import gc
    gc.collect(); gc.freeze(); gc.disable()
    # A STREAM of frames: one rank (sc_register_device_async) or replicated ranks (r04c: host-free sc_hypothesize_device, the
    # all-gather, sc_finalize_gathered_device_async).  The sharded form (--shard ab) and the split sample wait every step.
    pipelined = args.frames_in_flight == 2 and not sharded_ab and not split
    waited = None
    stream_identical = None
    stream_long = None
    counters = None
    # every frame's outputs in a slot of its scene's: checked against the waited form below and, in the checker leg, against the CPU
    # restatement of every scene
    Rt_all = torch.zeros(K, 12, dtype=torch.float32, device=dev)
    mask_all = torch.zeros(K, cfg.n, dtype=torch.uint8, device=dev)
    CTRS = ("n_frames", "n_fast_ok", "n_fast_repeat", "n_est_ok", "n_est_fail", "n_hostfree_grow")

    def ctr_now(gs):   # (sc_debug_last synchronises: only between the timed regions)
        return [sum(g_.debug_last()[c_] for g_ in gs) for c_ in CTRS]

    def ctr_diff(a, b, extra_repeats=0):
        d = dict(zip(CTRS, [y - x for x, y in zip(a, b)]))
        return {"frames": d["n_frames"] - extra_repeats, "host_free": d["n_fast_ok"], "host_free_then_repeated": d["n_fast_repeat"],
                "waited": d["n_frames"] - d["n_fast_ok"] - d["n_fast_repeat"] - extra_repeats,
                "bound_estimated_and_verified": d["n_est_ok"], "estimate_failed_call_repeated": d["n_est_fail"],
                "buffers_grown_inside_host_free_enqueues": d["n_hostfree_grow"]}

    if pipelined:
        # two contexts on ONE stream: strictly serial on the GPU, nothing overlaps on the device; the host is off the critical path
        regB = pkg.Registrar(local_rank)
        if knobs:
            regB.set_debug(**{k: int(v) for k, v in knobs.items()})
        regB.set_stream(torch.cuda.current_stream().cuda_stream)
        pair = [reg, regB]
        for i in range(max(W, 2)):   # the second context's own history: other scenes than the first one's (every rank alike)
            rcb, _ = step(p_hot, K // 2 + i, regB)
        # (the device addresses of every scene and of its output slot, taken once: indexing a tensor inside the timed loop costs
        # microseconds per frame, and its first use ~0.1 ms — that was the first timed step's 0.33 ms)
        ptrs = [(d_srcs[k].data_ptr(), d_tgts[k].data_ptr(), Rt_all[k].data_ptr(), mask_all[k].data_ptr()) for k in range(K)]
        if world == 1:
            def enqueue(f, k):
                a_ = ptrs[k]
                pair[f & 1].register_device_async(a_[0], a_[1], cfg.n, p_of(f), a_[2], a_[3])
            # (a frame whose host-free enqueue turns out void is repeated inside sc_wait)
        else:
            rs = pkg.shard.ReplicatedStream(pkg, pair, cfg.n, p_hot, world, lambda k_: torch.zeros(k_, dtype=torch.int64, device=dev),
                                            ptr=lambda t_: t_ if isinstance(t_, int) else t_.data_ptr())
            rs.estimate = rep_est[0]

            def enqueue(f, k):
                rs.enqueue(f, *ptrs[k])

        def run_stream(frames, scene_of, timed_hot=False):
            """`frames` frames, frame f + 1 enqueued before frame f's winner is waited for -> (wall s, per-frame (scene, rc, rank,
            count, edges, triangles), winner-to-winner times, frames the CALLER had to repeat, sum of us_score)"""
            res, ts, n_redo, hot = [], [], 0, 0.0
            n_hot[0] = 0
            fence()
            t0 = time.perf_counter()
            enqueue(0, scene_of(0))
            tl = t0
            for f in range(1, frames + 1):
                if f < frames:
                    enqueue(f, scene_of(f))
                if world == 1:
                    rc, st = pair[(f - 1) & 1].wait()     # frame f - 1: status, statistics; (R, t) and mask complete
                else:
                    r0_ = rs.redone
                    rc, st = rs.collect(f - 1)            # (SC_EBOUND: the frame again, certifying — every rank alike)
                    n_redo += rs.redone - r0_
                tn_ = time.perf_counter()
                ts.append(tn_ - tl); tl = tn_         # (winner to winner)
                if HE and (f - 1) % HE == 0:
                    hot += st["us_score"]; n_hot[0] += 1
                res.append((scene_of(f - 1), rc, st["best_rank"], st["best_count"], st["edges"], st["tri_total"]))
            fence()
            return time.perf_counter() - t0, res, ts, n_redo, hot, st

        c0 = ctr_now(pair)
        dt, res, step_s, n_redo, hot_score, st = run_stream(args.steps, lambda f: f % K)
        n_hot_timed = n_hot[0]
        rc = res[-1][1]
        c1 = ctr_now(pair)
        counters = ctr_diff(c0, c1, n_redo)
        counters["frames_repeated"] = counters["host_free_then_repeated"] + counters["estimate_failed_call_repeated"] if world == 1 else n_redo
        per_scene = {}
        for k_, rc_, rk_, cn_, _, _ in res:
            if per_scene.setdefault(k_, (rc_, rk_, cn_)) != (rc_, rk_, cn_):
                print(f"bench.py: two frames of scene {k_} disagree: {per_scene[k_]} vs {(rc_, rk_, cn_)}", file=sys.stderr)
                return 1
        if args.dump_outputs and rank == 0:
            k_last = (args.steps - 1) % K   # (the frame's outputs are in its scene's slot)
            dump_outputs(args.dump_outputs, Rt_all[k_last], mask_all[k_last], rc, st)
        if args.full:
            got_stream = (Rt_all.cpu().numpy().copy(), mask_all.cpu().numpy().copy())
            # ---- the waited form: the same frames, each begun only when the previous winner has reached the host
            w_s = []
            fence()
            tw0 = time.perf_counter()
            for f in range(args.steps):
                ts0 = time.perf_counter()
                a_ = ptrs[f % K]
                if world == 1:
                    rcw, stw = reg.register_device(a_[0], a_[1], cfg.n, p_hot, a_[2], a_[3])
                else:
                    rcw, stw = rs.waited(0, *a_)
                w_s.append(time.perf_counter() - ts0)
                if per_scene[f % K] != (rcw, stw["best_rank"], stw["best_count"]):
                    print(f"bench.py: waited and streamed frames of scene {f % K} disagree: {(rcw, stw['best_rank'], stw['best_count'])} vs {per_scene[f % K]}", file=sys.stderr)
                    return 1
            fence()
            dtw = time.perf_counter() - tw0
            got_waited = (Rt_all.cpu().numpy(), mask_all.cpu().numpy())
            seen = sorted(per_scene)
            if not (np.array_equal(got_stream[0][seen].view(np.uint32), got_waited[0][seen].view(np.uint32)) and np.array_equal(got_stream[1][seen], got_waited[1][seen])):
                print("bench.py: (R, t) or mask of a streamed frame differs from the waited call's", file=sys.stderr)
                return 1
            if world > 1:
                twm = torch.tensor([dtw], dtype=torch.float64, device=dev)
                dist.all_reduce(twm, op=dist.ReduceOp.MAX)
                dtw = float(twm.item())
            waited = {"ms_per_step": dtw / args.steps * 1e3, "ms_per_step_median": float(np.median(w_s)) * 1e3,
                      "hypotheses_per_s": T_total * args.steps / dtw,
                      "note": "the same frames, each begun only when the previous winner has reached the host (--frames-in-flight 1: "
                              "the headline form of rounds 1 - 3, there on one repeated scene)"}
        if args.full and not args.headline_only:
            # ---- r04's headline form beside it: every frame the SAME scene (the config's own), streamed
            dti, resi, si, _, _, _ = run_stream(args.steps, lambda f: 0)
            if world > 1:
                tim = torch.tensor([dti], dtype=torch.float64, device=dev)
                dist.all_reduce(tim, op=dist.ReduceOp.MAX)
                dti = float(tim.item())
            stream_identical = {"ms_per_step": dti / args.steps * 1e3, "ms_per_step_median": float(np.median(si)) * 1e3,
                                "hypotheses_per_s": T_total * args.steps / dti,
                                "note": "the same stream with every frame the config's own scene (round 4's headline form): the covers of "
                                        "the host-free enqueue, the estimate and the choice of stage C2's kernel only ever see their best case there"}
            # ---- the distinct-frame stream over many cycles of the scenes: rates of the fallbacks (repeated frames, failed estimates)
            n_long = max(256, 8 * K) if K > 1 else 64
            c2_ = ctr_now(pair)
            dtl, resl, sl_, n_redo_l, _, _ = run_stream(n_long, lambda f: f % K)
            c3_ = ctr_now(pair)
            for k_, rc_, rk_, cn_, _, _ in resl:
                if per_scene.setdefault(k_, (rc_, rk_, cn_)) != (rc_, rk_, cn_):
                    print(f"bench.py: two frames of scene {k_} disagree (long stream): {per_scene[k_]} vs {(rc_, rk_, cn_)}", file=sys.stderr)
                    return 1
            if world > 1:
                tlm = torch.tensor([dtl], dtype=torch.float64, device=dev)
                dist.all_reduce(tlm, op=dist.ReduceOp.MAX)
                dtl = float(tlm.item())
            stream_long = {"frames": n_long, "ms_per_step": dtl / n_long * 1e3, "ms_per_step_median": float(np.median(sl_)) * 1e3,
                           "ms_per_step_max": float(np.max(sl_)) * 1e3, "hypotheses_per_s": T_total * n_long / dtl,
                           "how_the_frames_ran": ctr_diff(c2_, c3_, n_redo_l),
                           "edges_min_max": [int(min(r_[4] for r_ in resl)), int(max(r_[4] for r_ in resl))],
                           "triangles_enumerated_min_max": [int(min(r_[5] for r_ in resl)), int(max(r_[5] for r_ in resl))],
                           "inliers_of_the_winner_min_max": [int(min(r_[3] for r_ in resl)), int(max(r_[3] for r_ in resl))]}
        regB.close()
    else:
        step_s, per_scene = [], {}
        fence()
        t0 = time.perf_counter()
        for f in range(args.steps):
            ts0 = time.perf_counter()
            rc, st = step(p_of(f), f % K)
            step_s.append(time.perf_counter() - ts0)   # (every step ends with the winner on the host: its own wall time is meaningful)
            if HE and f % HE == 0:
                hot_score += st["us_score"]; n_hot_timed += 1
        fence()
        dt = time.perf_counter() - t0
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, d_Rt, d_mask, rc, st)
    # (the line's `config` and `winner`, the stage passes, the CPU baseline and the legs below: the config's own scene, scenes[0];
    # make it the context's last call)
    rc, st = step(p_hot, 0)
    if args.full:
        # ---- per-stage times of THE SAME code path: one bracket per pass (SC_FLAG_TIMING_ONE: two event records per call,
        # speculative launches on), a few passes per stage; then one fully bracketed pass for the key kernel alone
        n_diag = max(3, min(8, args.steps))
        avg = {}
        for k, name in enumerate(STAGES):
            prm = mk(pkg.SC_FLAG_TIMING_ONE | pkg.SC_TIMING_STAGE(k))
            acc = []
            for _ in range(n_diag):
                _, sd = step(prm)
                acc.append(sd["us_" + name])
            avg[name] = float(np.median(acc))
        p_all = mk(pkg.SC_FLAG_TIMING)
        tk = []
        for _ in range(5):
            _, sd = step(p_all)
            tk.append(sd["us_trikeys"])
        tk = float(np.median(tk))   # (a mean of three once carried a 40 us outlier into roofline_other)
    fence()
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    if args.full:
        if n_hot_timed:
            us_score = hot_score / n_hot_timed  # the roofline duration of the dominant kernel: measured inside the timed steps
        else:                                   # (--hot-timing-every 0: from eight calls after them)
            us_score = sum(step(p_hot, f % K)[1]["us_score"] for f in range(8)) / 8
            step(p_hot, 0)
        c2_info = reg.debug_last()         # which C2 kernel the last call ran, the filter's hand-overs
        # the filter kernel alone (its own dispatch timestamps; us_score spans filter + exact pass): eight more calls, outside the timed region
        us_filter = []
        for _ in range(8 if (world == 1 and c2_info["c2_kernel"] in (1, 2)) else 0):   # (one rank only: no collective may depend on a measurement)
            step(p_hot)
            us_filter.append(reg.debug_last()["us_c2_filter"])
        us_filter = [u for u in us_filter if u > 0.0]
        us_filter = sum(us_filter) / len(us_filter) if us_filter else None

    out = None
    if rank == 0:
        n = cfg.n
        ms_per_step = dt / args.steps * 1e3
        value = T_total * args.steps / dt
        n_local = st["tri_scored"]
        dense = not args.no_dense_s
        mode = "shard_ab" if sharded_ab else ("replicated_AB" if world > 1 else "single")
        out = {
            "metric": "triangle-hypotheses scored/sec (end-to-end: compat graph + ranked triangles + SVD + scoring + mask)",
            "value": value, "unit": "hypotheses/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "ms_per_step_median": float(np.median(step_s)) * 1e3,
            "ms_per_step_min_max": [round(float(np.min(step_s)) * 1e3, 4), round(float(np.max(step_s)) * 1e3, 4)],
            "ms_of_each_timed_step": [round(float(x) * 1e3, 4) for x in step_s[:64]],
            "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "f32", "data": "synthetic" + (" (REHEARSAL: all ranks on one GPU over gloo)" if rehearsal else ""),
            "config": {"workload": f"{cfg.name}: N={n} synthetic correspondences (L={cfg.L}, tau={cfg.tau}; "
                                   + (f"a stream of {K} DISTINCT scenes, seeds {cfg.seed} + k, inlier ratio {cfg.rho * 2 / 3:.0%} .. {cfg.rho * 4 / 3:.0%}: frame f registers scene f mod {K}"
                                      if K > 1 else f"{cfg.rho:.0%} inliers, one scene repeated")
                                   + f"), T_total={T_total} ranked triangles scored per step ({n_local} on this GPU)",
                       "n_corr": n, "triangles_total": T_total, "triangles_this_gpu": n_local, "scenes": K,
                       "edges": st["edges"], "triangles_enumerated": st["tri_total"],
                       "edges_note": "`edges`, `triangles_enumerated`, `winner`, `stage_us`, the rooflines' counts: the config's own scene (scene 0 of the stream)",
                       "parallelism": f"{mode}{world}", "dense_S": dense},
            "winner": {"rank": st["best_rank"], "inliers": st["best_count"], "status": rc},
            "how_the_timed_frames_ran": counters,
            "how_the_timed_frames_ran_note": "cumulative counters of the two contexts over the timed frames (sc_debug_last): host_free = enqueued without a "
                                             "host wait and valid at its end; host_free_then_repeated = a count outgrew what the launches covered (or "
                                             "another assumption failed): the frame ran again the waiting way INSIDE the timed region; estimate_failed = "
                                             "stage B's estimated pruning bound was too high: repeated with a certifying sample",
            "step_form": ("stream of DISTINCT frames: step k + 1 enqueued before step k's winner is waited for ("
                          + ("sc_register_device_async" if world == 1 else "host-free sc_hypothesize_device, all-gather, sc_finalize_gathered_device_async")
                          + " / sc_wait, two contexts on one stream; serial on the GPU)") if pipelined else "waited: a step begins when the previous winner is on the host",
        }
        if sharded_ab:
            out["config"]["bytes_received_per_step"] = ss.bytes_exchanged()
        elif world > 1:
            out["config"]["pruning_sample"] = "sharded + 1 KiB all-reduce" if split else "replicated"

    if rank == 0 and args.full:
        rows_local = n if not sharded_ab else int(ss.plan.rows_per_rank)
        # ---- rooflines (algorithmic bytes / flops per launch: DESIGN.md §5)
        compat_bytes = (4 * rows_local * n if dense else 0) + rows_local * n / 8 + 24 * n
        compat_gbs = compat_bytes / (max(avg["compat"], 1e-3) * 1e-6) / 1e9
        score_flops = 27.0 * n_local * n                               # 27 flop per (hypothesis, corr)
        score_tflops = score_flops / (max(us_score, 1e-3) * 1e-6) / 1e12
        roof_compat = {"kernel": "compat_tiles_kernel", "bound": "hbm" if dense else "valu", "achieved": round(compat_gbs, 1),
                       "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(compat_gbs / HBM_PEAK_GBS, 4),
                       "traffic": None, "algorithmic_bytes": int(compat_bytes), "avg_us": round(avg["compat"], 2),
                       "note": "duration: HIP-event bracket around this kernel alone, on the hot path (one bracket per pass)"
                               + ("" if dense else "; SC_FLAG_NO_DENSE_S: bit rows only, the kernel is arithmetic-bound")}
        filtered = c2_info["c2_kernel"] in (1, 2)                     # what the library says it ran (sc_debug_last), not a guess
        fk = {0: "score_kernel", 1: "score_filter_kernel + score_exact_kernel", 2: "score_gram_kernel + score_exact_kernel"}[c2_info["c2_kernel"]]
        # for the filtered path `frac` is the kernel's OWN bound — the f16 MFMA flops it executes (linear filter:
        # one 32x32x16 MFMA = 32768 flop per 256 tests = 128 per test; Gram filter: three per 1024 tests = 96 per test) over the
        # dense f16 MFMA peak — not the fp32-equivalent yardstick (27 algorithmic flop per test over the fp32 vector peak), which
        # an f16 matrix-pipe kernel can pass 1.0 of; that number stays as `fp32_equivalent`, and the distance from the SIMD's
        # issue port, which is what really bounds the kernel, as `issue_model`.
        mfma_per_test = {1: 128.0, 2: 96.0}.get(c2_info["c2_kernel"], 0.0)
        # r04b: the Gram filter EVALUATES only part of the n_local x n tests — the rest are decided by the triangle inequality
        # against the call's reference frame — so its executed flops are counted on what it evaluates
        tests_exec = executed_tests(n, c2_info) if c2_info["c2_kernel"] == 2 and c2_info.get("gram_rows") else float(n_local) * n
        mfma_tflops = mfma_per_test * tests_exec / (max(us_score, 1e-3) * 1e-6) / 1e12
        # what bounds the filtered stage is the SIMD's ISSUE PORT, which the MFMAs share with the vector instructions that
        # test and count their results — so `peak` is the f16 MFMA rate this kernel's instruction mix allows when that port is
        # saturated (issue_model: per step, mfma_per_step MFMAs of 32 768 flop in bound_vector_cycles cycles of each of the 1024
        # SIMDs at the nominal clock), and `frac` = achieved / peak = issue_model.frac_of_issue_bound.  The dense matrix-pipe peak and
        # the fp32-equivalent yardstick stay beside it.
        im = issue_model(n, n_local, us_score, c2_info) if filtered else None
        peak_issue = (im["mfma_per_step"] * 32768.0 / max(im["bound_matrix_cycles"], im["bound_vector_cycles"]) * GPU_CLOCK_HZ * N_SIMD / 1e12) if im else None
        roof_score = {"kernel": fk,
                      "bound": "mfma" if filtered else "valu",
                      "achieved": round(mfma_tflops if filtered else score_tflops, 2),
                      "peak": round(peak_issue, 1) if filtered else FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                      "frac": round(mfma_tflops / peak_issue if filtered else score_tflops / FP32_PEAK_TFLOPS, 4),
                      "peak_note": ("the f16 MFMA rate at which this kernel's own instruction mix saturates the SIMD's issue port (the port the "
                                    "MFMAs share with the vector instructions that consume their results: `issue_model`), not the dense "
                                    "matrix-pipe peak — that one is `mfma_dense`") if filtered else None,
                      "mfma_dense": {"achieved": round(mfma_tflops, 2), "peak": F16_MFMA_PEAK_TFLOPS,
                                     "frac": round(mfma_tflops / F16_MFMA_PEAK_TFLOPS, 4)} if filtered else None,
                      "fp32_equivalent": {"achieved": round(score_tflops, 2), "peak": FP32_PEAK_TFLOPS,
                                          "frac": round(score_tflops / FP32_PEAK_TFLOPS, 4),
                                          "note": "SURVEY 8(d)'s definition: 27 flop x T x N over the fp32 vector peak.  > 1 where the filter DECIDES "
                                                  "tests without evaluating them (the triangle inequality against the call's reference frame: `tests`)"
                                                  " — every count still equals the fp32 chain's; a yardstick against the plain kernel, not a utilisation"} if filtered else None,
                      "traffic": None, "algorithmic_flops": score_flops, "avg_us": round(us_score, 2),
                      "kernel_us": {fk.split(" + ")[0]: round(us_filter, 2), "score_exact_kernel (+ the gap between the two)": round(us_score - us_filter, 2)}
                                   if (filtered and us_filter) else None,
                      "tests": {"decided": float(n_local) * n, "evaluated": tests_exec,
                                "evaluated_frac": round(tests_exec / max(float(n_local) * n, 1.0), 4),
                                "decided_per_s": round(float(n_local) * n / (max(us_score, 1e-3) * 1e-6), 1),
                                "near_hypotheses": c2_info.get("gram_near_hyp"), "near_correspondences": c2_info.get("gram_near_corr"),
                                "rows": c2_info.get("gram_rows")} if c2_info["c2_kernel"] == 2 else None,
                      "issue_model": im,
                      "note": ("`achieved` = f16 MFMA flops EXECUTED per second over the whole C2 stage (filter + exact pass); the stage is "
                               "LATENCY-bound, not throughput-bound: a workgroup lives ~13 us, of which the steps are a third (per-workgroup "
                               "prologue, first LDS-DMA, DPP tail over 2 - 4 units of work: DESIGN.md 5). " if filtered else "") +
                              ({1: "stage C2 = fp16-split matrix-pipe filter on the residual VECTOR (4.75 vector instructions + 1/256 MFMA per "
                                   "test) + exact fp32 pass over the undecided tests; counts identical to the fp32 kernel. ",
                                2: "stage C2 = Gram-form matrix-pipe filter in the frame of a voted reference hypothesis (the MFMA "
                                   "evaluates the SQUARED residual: 1.6 vector instructions + 3/1024 MFMA per evaluated test; hypotheses near "
                                   "the frame skip every correspondence the triangle inequality rules out: `tests`) + exact fp32 pass over the "
                                   "undecided tests; counts identical to the fp32 kernel. ", 0: "fp32 vector kernel. "}[c2_info["c2_kernel"]]) +
                              "not HBM-bound (~8 MB moved); duration from HIP events inside the timed steps (SC_FLAG_TIMING_HOT: the "
                              "dispatch packets' own timestamps), taken on every %d-th timed frame (a launch that carries events costs "
                              "the frame ~1 us: --hot-timing-every)" % max(1, HE)}
        # HBM bytes per launch from the committed rocprofv3 --pmc passes of this same command (tools/pmc_collect.sh,
        # FETCH_SIZE doubled per the gfx950 correction, WRITE_SIZE as is); PMC counters cannot be read from inside the
        # process, so `traffic` is the committed measurement of this code state, valid for the headline workload only
        pmc_all, pmc_src = {}, None
        pmc_path = os.path.join(ROOT, "profiles", "pmc_summary.json")
        if os.path.exists(pmc_path) and args.config == "C2" and world == 1 and dense and not knobs:
            try:
                pmc_all = json.load(open(pmc_path))
                pmc_src = "profiles/pmc_summary.json (rocprofv3 --pmc passes of this command; see profiles/README.md)"
            except Exception:
                pmc_all = {}
        M, E = st["tri_total"], st["edges"]
        tk_bytes = 12 * M + 32 * M / 1.37 + 12 * E                # keys + {third vertex, edge} written, ~M/1.37 event records read
        tk_gbs = tk_bytes / (max(tk, 1e-3) * 1e-6) / 1e9
        roof_tk = {"kernel": "tri_keys_events_kernel", "bound": "hbm", "achieved": round(tk_gbs, 1), "peak": HBM_PEAK_GBS,
                   "unit": "GB/s", "frac": round(tk_gbs / HBM_PEAK_GBS, 4), "traffic": None,
                   "algorithmic_bytes": int(tk_bytes), "avg_us": round(tk, 2),
                   "note": "stage B key kernel (lane per member-word event): gather / latency bound, HBM roofline quoted "
                           "because SURVEY §8d asks; duration from a fully bracketed pass (speculation off there)"}
        roofs = sorted([roof_compat, roof_score, roof_tk], key=lambda r: -r["avg_us"])
        for r in roofs:
            pk = r["kernel"].split(" + ")[0]  # (the filtered C2 stage: the filter kernel's own traffic)
            if pmc_all.get(pk, {}).get("hbm_bytes_per_launch") is not None:
                r["traffic"] = pmc_all[pk]["hbm_bytes_per_launch"]
                r["traffic_source"] = pmc_src
        dominant, other = roofs[0], roofs[1:]

        out.update({
            "score_stage_hyp_per_s": n_local * world / ((avg["kabsch"] + avg["score"] + avg["argmax"]) * 1e-6),
            "stage_us": {k: round(v, 2) for k, v in avg.items()} | {"trikeys": round(tk, 2)},
            # the stage as a whole — triangles enumerated per second and the bytes the row asks for (bit matrix once,
            # 12 per enumerated triangle, 16 per selected one) over the stage's bracket; data-dependent gathers, no fraction target
            "stage_b": {"triangles_enumerated": st["tri_total"], "us": round(avg["triangles"], 2),
                        "triangles_enumerated_per_s": round(st["tri_total"] / (max(avg["triangles"], 1e-3) * 1e-6), 1),
                        "algorithmic_bytes": int(n * n / 8 + 12 * st["tri_total"] + 16 * st["tri_scored"] * (world if not sharded_ab else 1)),
                        "achieved_GBs": round((n * n / 8 + 12 * st["tri_total"] + 16 * st["tri_scored"]) / (max(avg["triangles"], 1e-3) * 1e-6) / 1e9, 1),
                        "note": "the graph is pruned by a bound on the T-th key before it is enumerated (DESIGN 5.0): `triangles_enumerated` is what "
                                "the pruned graph holds, a fraction of the graph's triangles; the stage is ten dependent launches of gathers, latency-bound"},
            "stage_us_note": "one HIP-event bracket per pass on the hot path (SC_FLAG_TIMING_ONE), median of the passes; `triangles` includes its "
                             "read-backs" + (" and the collectives between the phases" if sharded_ab else ""),
            "host_gap_us": round(ms_per_step * 1e3 - sum(avg.values()), 1),
            "host_gap_note": "step minus the sum of the stage brackets (taken on waited calls): the ramps between the stages; in the waited "
                             "form also the launch of the first kernel into an idle queue, the winner's way back to the host, Python between the calls",
            "stream_long": stream_long, "stream_identical_frames": stream_identical,
            "waited": waited,
            "bytes_moved_algorithmic": st.get("bytes_moved"),
            "roofline": dominant, "roofline_other": other,
        })

        if world == 1 and args.headline_only:
            pass
        elif world == 1:
            # ---- ms to best (R,t): SURVEY §8d metric (2) = host arrays in -> outputs back on the host (sc_register)
            reg.set_stream(None)
            p1 = pkg.make_params(flags=base_flags, **kw)
            reg.register(scene.src, scene.tgt, params=p1)
            th0 = time.perf_counter()
            for _ in range(20):
                reg.register(scene.src, scene.tgt, params=p1)
            out["ms_to_best_Rt"] = (time.perf_counter() - th0) / 20 * 1e3
            out["ms_to_best_Rt_note"] = "host wall of sc_register: H2D of the correspondences, A..C3, D2H of (R,t,mask)"
            out["cold_call_ms"] = cold_ms
            # a sequence of DIFFERENT sizes on one context: the speculative launches miss, buffers were sized by other inputs
            seq = [n, int(0.8 * n), int(0.6 * n), int(0.9 * n)]
            for m in seq:
                reg.register(scene.src[:m], scene.tgt[:m], params=p1)
            tv0 = time.perf_counter()
            per_call = []
            for _ in range(5):
                for m in seq:
                    tc0 = time.perf_counter()
                    reg.register(scene.src[:m], scene.tgt[:m], params=p1)
                    per_call.append(round((time.perf_counter() - tc0) * 1e3, 3))
                    if per_call[-1] > 2.0:
                        print(f"bench.py: varying-n call {len(per_call) - 1} (n = {m}) took {per_call[-1]} ms: {reg.debug_last()} "
                              f"{reg._lib.sc_last_error(reg._h).decode()}", file=sys.stderr)
            out["ms_per_call_varying_n"] = {"sizes": seq, "ms": (time.perf_counter() - tv0) / 20 * 1e3,
                                            "ms_median": float(np.median(per_call)), "ms_max": float(np.max(per_call))}
            # ---- the same workload without the dense matrix (nothing on the path reads S)
            if dense:
                reg.set_stream(torch.cuda.current_stream().cuda_stream)
                p_nd = pkg.make_params(flags=pkg.SC_FLAG_NO_DENSE_S, **kw)
                p_ndc = pkg.make_params(flags=pkg.SC_FLAG_NO_DENSE_S | pkg.SC_FLAG_TIMING_ONE | pkg.SC_TIMING_STAGE(1), **kw)
                for _ in range(3):
                    reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p_nd, d_Rt.data_ptr(), d_mask.data_ptr())
                torch.cuda.synchronize(); tn0 = time.perf_counter()
                for _ in range(20):
                    reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p_nd, d_Rt.data_ptr(), d_mask.data_ptr())
                torch.cuda.synchronize(); nd_ms = (time.perf_counter() - tn0) / 20 * 1e3
                ndc = 0.0
                for _ in range(5):
                    _, sd = reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p_ndc, d_Rt.data_ptr(), d_mask.data_ptr())
                    ndc += sd["us_compat"] / 5
                out["no_dense_S"] = {"ms_per_step": nd_ms, "hypotheses_per_s": T_total / (nd_ms * 1e-3), "us_compat": round(ndc, 2),
                                     "note": "SC_FLAG_NO_DENSE_S: stage A writes the bit rows only; identical results"}
                p_chk = pkg.make_params(flags=base_flags, **kw)
                reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p_chk, d_Rt.data_ptr(), d_mask.data_ptr())
                torch.cuda.synchronize()
            # ---- the native multi-device entry on ONE device: what its orchestration costs the host.
            # sc_create_multi_loopback(dev, 1) runs the rank machinery (worker thread, phase API, all four collectives) over a
            # real single-rank RCCL communicator.  Against it: sc_register (same host I/O, unsharded path) and the phase API
            # at world 1 driven from this script (same kernels as the multi entry, no worker thread, no RCCL calls).
            try:
                reg.set_stream(None)
                with stdout_to_stderr():
                    mm = pkg.MultiRegistrar((local_rank,), loopback_ranks=1)
                    for _ in range(3):
                        gm = mm.register(scene.src, scene.tgt, params=p1)
                # (every call below returns with its result on the host, so each is timed by itself; MEDIANS of 24, and the host-array
                # form measured again right here — round 5's means of separate legs once gave a negative difference of differences)
                def med_ms(fn, reps=24):
                    ts_ = []
                    for _ in range(reps):
                        t0_ = time.perf_counter(); r_ = fn(); ts_.append(time.perf_counter() - t0_)
                    return float(np.median(ts_)) * 1e3, r_
                multi_ms, gm = med_ms(lambda: mm.register(scene.src, scene.tgt, params=p1))
                mm.close()
                for _ in range(3):
                    reg.register(scene.src, scene.tgt, params=p1)
                host_ms, _ = med_ms(lambda: reg.register(scene.src, scene.tgt, params=p1))
                reg.set_stream(torch.cuda.current_stream().cuda_stream)
                ss1 = pkg.shard.ShardedStep(pkg, reg, n, pkg.make_params(shard_block=block, flags=base_flags, **kw), 0, 1, dev)
                for _ in range(3):
                    ss1.step(d_src.data_ptr(), d_tgt.data_ptr())
                torch.cuda.synchronize()
                phase_ms, _ = med_ms(lambda: ss1.step(d_src.data_ptr(), d_tgt.data_ptr()))
                for _ in range(3):
                    step(p_hot, 0)
                torch.cuda.synchronize()
                dev0_ms, _ = med_ms(lambda: step(p_hot, 0))   # the device-resident waited step on the same scene
                host_io_ms = host_ms - dev0_ms   # what host arrays in / out add to the device-resident (waited) step
                out["native_multi"] = {
                    "sc_register_multi_loopback1_ms": multi_ms, "sc_register_ms": host_ms,
                    "phase_api_world1_device_resident_ms": phase_ms, "single_device_resident_ms": dev0_ms,
                    "orchestration_us": round((multi_ms - phase_ms - host_io_ms) * 1e3, 1),
                    "same_result": bool(gm["stats"]["best_rank"] == st["best_rank"] and np.array_equal(gm["mask"], d_mask.cpu().numpy())),
                    "note": "orchestration_us = sc_register_multi (one rank, real single-rank RCCL communicator: worker thread, "
                            "barriers, 3 ncclAllGather — plus 1 ncclAllReduce on graphs of 8192 correspondences and more) minus the same phases driven directly minus the host "
                            "I/O of sc_register; N > 1 over RCCL is unmeasured on hardware"}
            except Exception as ex:  # RCCL not loadable on this box: report, do not fail the headline
                out["native_multi"] = {"error": str(ex)}
            reg.set_stream(None)
            # ---- throughput with several independent registrations in flight ON THE GPU: one context and one stream per frame in
            # flight, ONE host thread (sc_register_device_async ring; r04c — rounds 2 - 4b used a host thread per context and waited
            # calls).  The path is a chain of ~16 dependent launches, most of them far from filling the chip, so frames that overlap
            # fill each other's gaps.  NOT the headline (`value` is frames back to back on ONE stream: nothing overlaps there); what a
            # service that registers a stream of frames can get out of the card.
            out["calls_in_flight"] = {"note": "independent registrations OVERLAPPING on the GPU: one context and one stream each, one host thread "
                                              "(sc_register_device_async / sc_wait ring), 64 frames per line — the stream's DISTINCT scenes, every winner compared with the timed stream's; hypotheses/s of all of them together; not `value`"}
            p2 = pkg.make_params(flags=base_flags, **kw)
            for nfl in (2, 3, 4):
                regs2 = [pkg.Registrar(local_rank) for _ in range(nfl)]
                streams2 = [torch.cuda.Stream(device=dev) for _ in range(nfl)]
                outs2 = [(torch.zeros(12, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)) for _ in range(nfl)]
                for g, s2 in zip(regs2, streams2):
                    g.set_stream(s2.cuda_stream)
                # (r05: the stream's DISTINCT frames — frame k registers scene k mod K; every winner against the timed stream's)
                sp2 = [(d_srcs[k_].data_ptr(), d_tgts[k_].data_ptr()) for k_ in range(K)]
                for j_, (g, o2) in enumerate(zip(regs2, outs2)):
                    for w_ in range(3):
                        a2 = sp2[(K - 3 * nfl + 3 * j_ + w_) % K]
                        g.register_device(a2[0], a2[1], n, p2, o2[0].data_ptr(), o2[1].data_ptr())
                KF = 64
                same = True
                torch.cuda.synchronize(); tp0 = time.perf_counter()
                for k in range(KF + nfl - 1):
                    if k < KF:
                        i = k % nfl
                        regs2[i].register_device_async(sp2[k % K][0], sp2[k % K][1], n, p2, outs2[i][0].data_ptr(), outs2[i][1].data_ptr())
                    if k >= nfl - 1:
                        kd = k - nfl + 1
                        rc2_, s2_ = regs2[kd % nfl].wait()
                        want2 = per_scene.get(kd % K)
                        same = same and (want2 is None or want2 == (rc2_, s2_["best_rank"], s2_["best_count"]))
                torch.cuda.synchronize(); tp = time.perf_counter() - tp0
                out["calls_in_flight"][str(nfl)] = {"ms_per_call": tp / KF * 1e3, "hypotheses_per_s": T_total * KF / tp, "same_winner": bool(same)}
                for g in regs2:
                    g.close()
        else:
            out["ms_to_best_Rt"] = ms_per_step
            out["ms_to_best_Rt_note"] = "N > 1: the device-resident step (inputs already in every GPU's HBM)"

        if world == 1 and not args.no_cpu_baseline and not args.headline_only:
            O = ge.load_oracle()
            tmax = min(O.max_threads(), os.cpu_count() or 1)
            ref = O.register(scene.src, scene.tgt, threads=tmax, **kw)  # warm-up pass, also the parity check
            # the thread count the restatement runs fastest with on this host (more threads are not always faster:
            # stage B merges one 512 KiB histogram per thread and pass) — two passes each, best kept
            best_t, threads = None, tmax
            for cand in sorted({tmax, max(1, tmax // 2), max(1, tmax // 4), min(tmax, 16)}, reverse=True):
                tq = time.perf_counter()
                for _ in range(2):
                    O.register(scene.src, scene.tgt, threads=cand, **kw)
                tq = (time.perf_counter() - tq) / 2
                if best_t is None or tq < best_t:
                    best_t, threads = tq, cand
            got_mask = d_mask.cpu().numpy()
            got_Rt = d_Rt.cpu().numpy()
            out["parity_vs_cpu_restatement"] = bool(
                np.array_equal(got_mask, ref["mask"]) and st["best_rank"] == ref["best_rank"]
                and got_Rt.tobytes() == np.concatenate([ref["R"].ravel(), ref["t"]]).astype(np.float32).tobytes())
            if pipelined and per_scene:
                # every scene of the stream against the CPU restatement: winner, its rank and count, (R, t) bit for bit, the mask — of the
                # outputs the STREAMED frames left in their scenes' slots (the timed frames, the waited ones and the long stream all
                # wrote them, and were compared with one another above)
                sR, sM = Rt_all.cpu().numpy(), mask_all.cpu().numpy()
                bad = []
                for k_ in sorted(per_scene):
                    r_ = O.register(scenes[k_].src, scenes[k_].tgt, threads=threads, **kw)
                    same = (per_scene[k_] == (r_["rc"], r_["best_rank"], r_["best_count"]) and np.array_equal(sM[k_], r_["mask"])
                            and sR[k_].tobytes() == np.concatenate([r_["R"].ravel(), r_["t"]]).astype(np.float32).tobytes())
                    if not same:
                        bad.append(k_)
                out["stream_parity_vs_cpu_restatement"] = {"scenes_checked": len(per_scene), "scenes_that_differ": bad, "all_equal": not bad,
                                                           "frames_behind_them": args.steps * 2 + (stream_long["frames"] if stream_long else 0)}
                if bad:
                    print(f"bench.py: scenes {bad} of the stream differ from the CPU restatement", file=sys.stderr)
            t1 = time.perf_counter()
            n1 = 0
            while True:                                                     # one core: a bounded sample (~5 s)
                O.register(scene.src, scene.tgt, threads=1, **kw)
                n1 += 1
                e1 = time.perf_counter() - t1
                if e1 >= 5.0 or n1 >= 3:
                    break
            passes, tc0 = 0, time.perf_counter()
            while True:                                                     # all cores: >= 8 s of full passes
                O.register(scene.src, scene.tgt, threads=threads, **kw)
                passes += 1
                el = time.perf_counter() - tc0
                if el >= 8.0 or passes >= 40:
                    break
            out["cpu_baseline"] = {"value": T_total * passes / el, "unit": "hypotheses/s", "cores": threads,
                                   "kind": "port", "ms_per_pass": el / passes * 1e3,
                                   "one_core": {"value": T_total * n1 / e1, "ms_per_pass": e1 / n1 * 1e3, "passes": n1},
                                   "cpu_model": cpu_model(),
                                   "host_threads_available": tmax,
                                   "sample": f"{passes} full passes on {threads} threads — the fastest of {tmax}, {tmax // 2}, "
                                             f"{tmax // 4}, 16 on this host — (+ {n1} on one) of the same workload "
                                             f"(N={n}, T={T_total}) through oracle/saccot_oracle.c — this repo's CPU "
                                             "restatement (the reference has no CPU path); OpenMP over rows in stages A "
                                             "and B and over hypotheses in C; a reported baseline, not a target"}
    if rank == 0:
        print(json.dumps(out))

    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    reg.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
