#!/usr/bin/env python3
"""What the absolute poses of a pair list's sets cost (include/saccot.h, sc_pairs_sync), poses and outputs resident in HBM.

  python tools/pairs_sync_bench.py [--shapes 64,512,2048] [--repeats 20] [--warmup 3] [--out profiles/pairs_sync.txt]
                                   [--prepend FILE ...] [--trace DIR]

The three lists of tools/pairs_cycles_bench.py (64 sets with all 2016 pairs; 512 sets with 20 pairs a set; 2048 sets with 200 704
pairs), each with exact poses (relative poses of random absolute poses, rounded to fp32) and noisy ones (every pose followed by a
turn of 0 - 0.3 degrees and a shift of 0 - 3e-3).  rot_tol = trans_tol = 1e-4, anchor 0, max_rounds 32, every pair used, weight 1.
Per list, in microseconds:
  host_us      what the CALL costs the host thread before it returns: the adjacency build and the enqueue (a host clock, the stream
               idle).
  device_us    device time of one sc_pairs_sync_device call: an event pair on the context's stream, with the stream held busy in
               front of the first event for longer than host_us (a spin kernel), so that every operation of the call is queued
               before the first one starts; median of `repeats` after `warmup`.
  cycles_us    one sc_pairs_cycles_device call (max_rounds 16) on the same list and poses, gated the same way.
  host_solve   the same rounds by ONE host thread in C++ (tools/pairs_sync_host.cpp, compiled here with g++ -O2
               -ffp-contract=off): build_ms and solve_ms; its rounds and the checksum of its poses must equal the GPU's.
  bound_us     one round against its bytes: entries x (8 + 8 + 104 + 96) read — the entry, the pair's weight, the neighbour's state,
               the oriented pose — plus 120 written per set (its state and tallies), at 6.3 TB/s.
`--trace DIR` adds the launches' own times: DIR holds the kernel trace of a run of its own of this tool WITH THE SAME ARGUMENTS,
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pairs_sync_bench.py ... --out ''
Per kernel the dispatches are taken in time order; a list's are the next `calls` of them; the warm-up ones are dropped and the medians
reported: prepare, round 1, the median working round after it, one idle round (the launches behind round K return at once) and finish.
Prints one JSON line per row, then a table; --out receives the text of every --prepend file, then both.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
import pairs_cycles_bench as PCB  # noqa: E402  (the lists, the rotations, the trace reader)

KERNELS = ("sync_prepare_kernel", "sync_round_kernel", "sync_finish_kernel")
TOL, MAX_ROUNDS = 1e-4, 32
HBM_BYTES_PER_US = 6.3e6  # 6.3 TB/s achievable


def noisy(rt, seed, deg=0.3, trans=3e-3):
    rng = np.random.default_rng(seed)
    N = PCB.rotations(rng, len(rt), 0.0, np.deg2rad(deg))
    d = rng.normal(size=(len(rt), 3)); d *= (rng.uniform(0, trans, len(rt)) / np.linalg.norm(d, axis=1))[:, None]
    out = rt.astype(np.float64)
    out[:, :9] = (N @ out[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
    out[:, 9:] = (N @ rt[:, 9:].astype(np.float64)[:, :, None])[:, :, 0] + d
    return out.astype(np.float32)


def host_solve(n_sets, pairs, rt, thr):
    exe = os.path.join(ROOT, "tools", "pairs_sync_host")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.array([n_sets, len(pairs), MAX_ROUNDS, 0], np.uint32).tobytes() + np.array(thr, np.float64).tobytes() + pairs.tobytes() + rt.tobytes())
    try:
        return json.loads(subprocess.check_output([exe, f.name]).decode())
    finally:
        os.unlink(f.name)


def checksum(sets):
    known = sets["status"] == 0
    return int(np.bitwise_xor.reduce(np.ascontiguousarray(sets["X"][known]).view(np.uint64).reshape(-1))) if known.any() else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64,512,2048")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_sync.txt"))
    ap.add_argument("--prepend", action="append", default=[])
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    trace = None
    if a.trace:
        PCB.KERNELS = KERNELS
        trace = PCB.trace_durations(a.trace)
    taken = {k: 0 for k in KERNELS}
    reach_of = {64: None, 512: 10, 2048: 98}
    sp = pkg.make_sync_params(TOL, TOL, max_rounds=MAX_ROUNDS)
    thr = pkg.sync_thresholds(sp)
    cp = pkg.make_cycle_params(PCB.ROT_TOL, PCB.TRANS_TOL, max_rounds=PCB.MAX_ROUNDS)
    reg = pkg.Registrar(0)
    stream = torch.cuda.Stream(device=dev)
    reg.set_stream(stream.cuda_stream)
    rows = []

    def gated(fn, host_us):
        """device time of what fn enqueues: the stream is kept busy in front of the first event until fn has returned"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int((3 * host_us + 2000) * 2400))  # cycles of a spin kernel: three times the host's share, at 2.4 GHz at most
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    try:
        for S in (int(x) for x in a.shapes.split(",")):
            pairs, exact, _R, _t = PCB.make_list(S, reach_of.get(S, 10), 100 + S)
            P = len(pairs)
            entries = 2 * P
            d_set = torch.zeros(S * 160, dtype=torch.uint8, device=dev); d_pair = torch.zeros(P * 32, dtype=torch.uint8, device=dev)
            d_sum = torch.zeros(32, dtype=torch.uint8, device=dev)
            d_res = torch.zeros(P * 48, dtype=torch.uint8, device=dev); d_csum = torch.zeros(32, dtype=torch.uint8, device=dev)
            for kind, rt in (("exact", exact), ("noisy", noisy(exact, 300 + S))):
                d_pose = torch.from_numpy(rt).to(dev)
                torch.cuda.synchronize()
                one = lambda: reg.pairs_sync_device(S, pairs, sp, d_pose.data_ptr(), 48, 0, 4, 0, d_set.data_ptr(), d_pair.data_ptr(), d_sum.data_ptr())  # noqa: E731
                cyc = lambda: reg.pairs_cycles_device(S, pairs, cp, d_pose.data_ptr(), 48, 0, d_res.data_ptr(), d_csum.data_ptr())  # noqa: E731
                one(); torch.cuda.synchronize()
                summ = np.frombuffer(d_sum.cpu().numpy().tobytes(), pkg.SYNC_SUMMARY_DTYPE)[0]
                sets = np.frombuffer(d_set.cpu().numpy().tobytes(), pkg.SYNC_SET_DTYPE)
                res = np.frombuffer(d_pair.cpu().numpy().tobytes(), pkg.SYNC_PAIR_DTYPE)
                host = host_solve(S, pairs, rt, thr)
                assert (host["rounds"], host["converged"], host["known"]) == (int(summ["rounds"]), int(summ["converged"]), int(summ["known"])), (host, summ)
                assert host["checksum"] == checksum(sets), "the host thread's poses are not the GPU's"
                t_host = []
                for it in range(a.warmup + a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); one(); t_host.append((time.perf_counter() - t0) * 1e6)
                host_us = med(t_host[a.warmup:])
                t_dev = [gated(one, host_us) for it in range(a.warmup + a.repeats)][a.warmup:]
                cyc(); torch.cuda.synchronize()
                t_cyc = [gated(cyc, host_us) for it in range(a.warmup + a.repeats)][a.warmup:]
                torch.cuda.synchronize()
                row = dict(sets=S, pairs=P, poses=kind, rounds=int(summ["rounds"]), converged=int(summ["converged"]), known=int(summ["known"]),
                           max_r2=float(res["r2"].max()), max_e2=float(res["e2"].max()), host_us=host_us, device_us=med(t_dev),
                           device_min_max=[round(min(t_dev), 1), round(max(t_dev), 1)], cycles_us=med(t_cyc), host_build_ms=host["build_ms"],
                           host_solve_ms=host["solve_ms"], bound_us=round((entries * (8 + 8 + 104 + 96) + S * 120) / HBM_BYTES_PER_US, 2))
                calls = 1 + 2 * (a.warmup + a.repeats)  # of sc_pairs_sync_device per row: the check, the host clock's, the gated ones
                if trace is not None:
                    def take(kernel, per_call):
                        mine = trace[kernel][taken[kernel]: taken[kernel] + calls * per_call]
                        taken[kernel] += calls * per_call
                        return np.array(mine).reshape(calls, per_call)[1 + a.warmup:] if len(mine) == calls * per_call else None
                    prep, rnd, fin = take(KERNELS[0], 1), take(KERNELS[1], MAX_ROUNDS), take(KERNELS[2], 1)
                    if prep is not None and rnd is not None and fin is not None:
                        K = row["rounds"]
                        row.update(prepare_us=round(float(np.median(prep)), 2), round1_us=round(float(np.median(rnd[:, 0])), 2),
                                   working_round_us=round(float(np.median(rnd[:, 1:K])), 2) if K > 1 else None,
                                   idle_round_us=round(float(np.median(rnd[:, K:])), 2) if K < MAX_ROUNDS else None,
                                   finish_us=round(float(np.median(fin)), 2))
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/pairs_sync_bench.py: one sc_pairs_sync_device call, max_rounds 32, tolerances 1e-4"
                 + (" (the launches' own times: a kernel trace taken in a run of its own)" if trace else " (no kernel trace: the launches' own times are not measured)"))
    cols = ["sets", "pairs", "poses", "rounds", "converged", "host_us", "device_us", "cycles_us", "host_build_ms", "host_solve_ms", "bound_us"]
    if trace is not None:
        cols += ["prepare_us", "round1_us", "working_round_us", "idle_round_us", "finish_us"]
    table = ["  ".join(f"{c:>16}" for c in cols)] + ["  ".join(f"{str(r.get(c, '-')):>16}" for c in cols) for r in rows]
    print("\n".join(table))
    lines += table + [json.dumps(r) for r in rows]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
