#!/usr/bin/env python3
"""What the loop-consistency check of a pair list costs (include/saccot.h, sc_pairs_cycles), poses and outputs resident in HBM.

  python tools/pairs_cycles_bench.py [--shapes 64,512,2048] [--repeats 20] [--warmup 3] [--out profiles/pairs_cycles.txt]
                                     [--prepend FILE ...] [--trace DIR]

Three lists: 64 sets with all 2016 pairs; 512 sets, every set paired with its 10 successors on a ring (20 pairs a set, 5120 pairs);
2048 sets, every set with its 98 successors (200 704 pairs).  The poses are relative poses of random absolute poses rounded to
fp32, stored in random directions, the list shuffled; each list runs clean (round 1 drops nothing: K = 1) and with 10 % of the
poses turned by 5 - 90 degrees (round 1 drops them, round 2 confirms: K = 2); the 16 launches of the rounds are enqueued either way.  rot_tol 0.5 degrees, trans_tol 0.01, min_ok 1, max_rounds 16.  Per list, in microseconds:
  host_us      what the CALL costs the host thread before it returns: the adjacency build and the enqueue (a host clock, the stream
               idle).  The device waits for it when nothing else is queued.
  device_us    device time of one sc_pairs_cycles_device call: an event pair on the context's stream, with the stream held busy in
               front of the first event for longer than host_us (a spin kernel), so that every operation of the call is queued
               before the first one starts; median of `repeats` after `warmup`.
  info_us      one sc_pose_info_pairs_slots_device call on the same list and poses, the call it sits next to in the chain, gated the
               same way: every set 32 points, every pair's 32 correspondences the identity (so every one is an inlier).
  host_loop    round 1's counts by ONE host thread over the same adjacency in C++ (tools/pairs_cycles_host.cpp, compiled here with
               g++ -O2 -ffp-contract=off): build_ms and loop_ms; its triangle counts and checksum must equal the GPU's.
`--trace DIR` adds the launches' own times: DIR holds the kernel trace of a run of its own of this tool WITH THE SAME ARGUMENTS,
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pairs_cycles_bench.py ... --out ''
Per kernel the dispatches are taken in time order; a list's are the next `calls` of them; the warm-up ones are dropped and the medians
reported: prepare, round 1, round 2, the later rounds (they return at once on a stable list) and finish, and the triangles per
second round 1 implies (every triangle is composed three times, once by each of its pairs: 3 x triangles / round-1 time).
Prints one JSON line per row, then a table; --out receives the text of every --prepend file, then both.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

KERNELS = ("cycles_prepare_kernel", "cycles_round_kernel", "cycles_finish_kernel")
ROT_TOL, TRANS_TOL, MAX_ROUNDS = float(np.deg2rad(0.5)), 0.01, 16
PTS = 32  # points a set, for the pose_info call


def rotations(rng, n, lo=0.0, hi=np.pi):
    axis = rng.normal(size=(n, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(lo, hi, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)


def make_list(n_sets, reach, seed):
    """-> (pairs (P, 2) uint32, clean poses (P, 12) float32, R (S, 3, 3), t (S, 3)); reach None: all pairs"""
    rng = np.random.default_rng(seed)
    if reach is None:
        a, b = np.triu_indices(n_sets, 1)
    else:
        a = np.repeat(np.arange(n_sets), reach)
        b = (a + np.tile(np.arange(1, reach + 1), n_sets)) % n_sets
    pairs = np.stack([a, b], axis=1)
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    pairs = pairs[rng.permutation(len(pairs))]
    R, t = rotations(rng, n_sets), rng.uniform(-1, 1, (n_sets, 3))
    Rab = np.swapaxes(R[pairs[:, 1]], 1, 2) @ R[pairs[:, 0]]
    tab = (np.swapaxes(R[pairs[:, 1]], 1, 2) @ (t[pairs[:, 0]] - t[pairs[:, 1]])[:, :, None])[:, :, 0]
    return pairs.astype(np.uint32), np.concatenate([Rab.reshape(-1, 9), tab], axis=1).astype(np.float32), R, t


def corrupted(rt, seed, share=0.1):
    rng = np.random.default_rng(seed)
    which = rng.choice(len(rt), int(round(share * len(rt))), replace=False)
    W = rotations(rng, len(which), np.deg2rad(5.0), np.deg2rad(90.0))
    out = rt.copy()
    out[which, :9] = (W @ rt[which, :9].astype(np.float64).reshape(-1, 3, 3)).reshape(-1, 9)
    return out


def trace_durations(folder):
    found = {k: [] for k in KERNELS}
    for f in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    found[k].append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    return {k: [d for _, d in sorted(v)] for k, v in found.items()}


def host_loop(n_sets, pairs, rt, thr):
    exe = os.path.join(ROOT, "tools", "pairs_cycles_host")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(np.array([n_sets, len(pairs)], np.uint32).tobytes() + np.array(thr, np.float64).tobytes() + pairs.tobytes() + rt.tobytes())
    try:
        return json.loads(subprocess.check_output([exe, f.name]).decode())
    finally:
        os.unlink(f.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64,512,2048")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_cycles.txt"))
    ap.add_argument("--prepend", action="append", default=[])
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    trace = trace_durations(a.trace) if a.trace else None
    taken = {k: 0 for k in KERNELS}
    reach_of = {64: None, 512: 10, 2048: 98}
    cp = pkg.make_cycle_params(ROT_TOL, TRANS_TOL, max_rounds=MAX_ROUNDS)
    thr = pkg.cycles_thresholds(cp)
    p = pkg.make_params(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=2000)
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
            pairs, clean, R, t = make_list(S, reach_of.get(S, 10), 100 + S)
            P = len(pairs)
            # the points: one world cloud seen from every set, so that a pair's pose maps its source points onto its target points
            world = np.random.default_rng(S).uniform(-1, 1, (PTS, 3))
            pts = (np.swapaxes(R, 1, 2)[:, None] @ (world[None] - t[:, None])[:, :, :, None])[:, :, :, 0].reshape(-1, 3).astype(np.float32)
            set_off = (np.arange(S + 1) * PTS).astype(np.uint32)
            d_pts = torch.from_numpy(pts).to(dev)
            ident = np.stack([np.arange(PTS), np.arange(PTS)], axis=1).astype(np.int32)
            d_corr = torch.from_numpy(np.tile(ident, (P, 1))).to(dev)
            count = np.zeros((P, 2), np.uint32); count[:, 0] = PTS
            d_count = torch.from_numpy(count.view(np.int32)).to(dev)
            d_info = torch.zeros(P * 320, dtype=torch.uint8, device=dev)
            d_res = torch.zeros(P * 48, dtype=torch.uint8, device=dev); d_sum = torch.zeros(32, dtype=torch.uint8, device=dev)
            for kind, rt in (("clean", clean), ("corrupted", corrupted(clean, 200 + S))):
                d_pose = torch.from_numpy(rt).to(dev)
                torch.cuda.synchronize()
                one = lambda: reg.pairs_cycles_device(S, pairs, cp, d_pose.data_ptr(), 48, 0, d_res.data_ptr(), d_sum.data_ptr())  # noqa: E731
                info = lambda: reg.pose_info_pairs_slots_device(d_pts.data_ptr(), set_off, pairs, 1, p, d_corr.data_ptr(), d_count.data_ptr(),  # noqa: E731
                                                                d_pose.data_ptr(), 48, d_info.data_ptr())
                one(); torch.cuda.synchronize()
                summ = np.frombuffer(d_sum.cpu().numpy().tobytes(), pkg.CYCLE_SUMMARY_DTYPE)[0]
                res = np.frombuffer(d_res.cpu().numpy().tobytes(), pkg.CYCLE_RESULT_DTYPE)
                host = host_loop(S, pairs, rt, thr)
                assert (host["triangles"], host["consistent"]) == (int(summ["triangles"]), int(summ["consistent"])), (host, summ)
                assert host["checksum"] == int(res["cycles"].astype(np.uint64).sum() * 3 + res["ok"].astype(np.uint64).sum())
                t_host = []
                for it in range(a.warmup + a.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); one(); t_host.append((time.perf_counter() - t0) * 1e6)
                host_us = med(t_host[a.warmup:])
                t_dev = [gated(one, host_us) for it in range(a.warmup + a.repeats)][a.warmup:]
                info(); torch.cuda.synchronize()
                t_info = [gated(info, 500.0) for it in range(a.warmup + a.repeats)][a.warmup:]
                torch.cuda.synchronize()
                row = dict(sets=S, pairs=P, poses=kind, triangles=int(summ["triangles"]), consistent=int(summ["consistent"]), rounds=int(summ["rounds"]),
                           alive=int(summ["alive"]), host_us=host_us, device_us=med(t_dev), device_min_max=[round(min(t_dev), 1), round(max(t_dev), 1)],
                           info_us=med(t_info), host_build_ms=host["build_ms"], host_loop_ms=host["loop_ms"])
                calls = 1 + 2 * (a.warmup + a.repeats)  # of sc_pairs_cycles_device per row: the check, the host clock's, the gated ones
                if trace is not None:
                    def take(kernel, per_call):
                        mine = trace[kernel][taken[kernel]: taken[kernel] + calls * per_call]
                        taken[kernel] += calls * per_call
                        return np.array(mine).reshape(calls, per_call)[1 + a.warmup:] if len(mine) == calls * per_call else None
                    prep, rnd, fin = take(KERNELS[0], 1), take(KERNELS[1], MAX_ROUNDS), take(KERNELS[2], 1)
                    if prep is not None and rnd is not None and fin is not None:
                        row.update(prepare_us=round(float(np.median(prep)), 2), round1_us=round(float(np.median(rnd[:, 0])), 2),
                                   round2_us=round(float(np.median(rnd[:, 1])), 2), later_rounds_us=round(float(np.median(rnd[:, 2:].sum(axis=1))), 2),
                                   finish_us=round(float(np.median(fin)), 2))
                        row["round1_triangles_per_s"] = round(3.0 * row["triangles"] / (row["round1_us"] * 1e-6), 0)
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/pairs_cycles_bench.py: one sc_pairs_cycles_device call, max_rounds 16"
                 + (" (the launches' own times: a kernel trace taken in a run of its own)" if trace else " (no kernel trace: the launches' own times are not measured)"))
    lines += [json.dumps(r) for r in rows]
    fmt = lambda r, k: "-" if r.get(k) is None else f"{r[k]:.2f}"  # noqa: E731
    table = ["", f"{'sets':>5} {'pairs':>7} {'poses':>9} {'triangles':>10} {'rounds':>6} | {'host us':>9} {'device us (min .. max)':>30} {'info us':>9} | "
                 f"{'host loop ms':>12} {'build ms':>9} | {'prepare':>8} {'round 1':>9} {'round 2':>9} {'later':>8} {'finish':>7} {'tri/s round 1':>14}"]
    for r in rows:
        d = f"{r['device_us']:.1f} ({r['device_min_max'][0]:.1f} .. {r['device_min_max'][1]:.1f})"
        table.append(f"{r['sets']:>5} {r['pairs']:>7} {r['poses']:>9} {r['triangles']:>10} {r['rounds']:>6} | {r['host_us']:>9.1f} {d:>30} {r['info_us']:>9.1f} | "
                     f"{r['host_loop_ms']:>12.3f} {r['host_build_ms']:>9.3f} | {fmt(r, 'prepare_us'):>8} {fmt(r, 'round1_us'):>9} {fmt(r, 'round2_us'):>9} "
                     f"{fmt(r, 'later_rounds_us'):>8} {fmt(r, 'finish_us'):>7} {r.get('round1_triangles_per_s', '-'):>14}")
    print("\n".join(table))
    lines += table
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
