#!/usr/bin/env python3
"""What the Gauss-Newton pose-graph solve of a pair list's sets costs (include/saccot.h, sc_pairs_solve), everything resident in HBM.

  python tools/pairs_solve_bench.py [--lists 64,512,2048,ring40,strip200] [--repeats 10] [--warmup 2] [--out profiles/pairs_solve.txt]
                                    [--prepend FILE ...] [--trace DIR]

The three lists of tools/pairs_cycles_bench.py (64 sets with all 2016 pairs; 512 sets with 20 pairs a set; 2048 sets with 200 704
pairs), a bare ring of 40 sets and an odometry strip of 200 sets with 40 closures, all with noisy poses (every pose followed by a
turn of 0 - 0.01 rad and a shift of 0 - 0.02) and identity information matrices (d_info NULL).  The start is the result of one
sc_pairs_sync_device call (max_rounds 32, tolerances 1e-4) on the same list; the solve runs at its defaults (max_outer 8, max_inner
64) with rot_tol = trans_tol = 1e-6 and cg_tol = 1e-3.  Per list, in microseconds:
  host_us      what the CALL costs the host thread before it returns: the adjacency build and the enqueue (a host clock, the stream
               idle).
  device_us    device time of one sc_pairs_solve_device call: an event pair on the context's stream, with the stream held busy in
               front of the first event for longer than host_us (a spin kernel); median of `repeats` after `warmup`.
  sync_us      the sc_pairs_sync_device call beside it, gated the same way.
  K, stop, inner_total   from the call's summary.
  ops, working   stream operations the call issues (a copy, a memset, 5 + max_outer * (4 + 2 * max_inner) launches) against the
               launches that did work: 4 + J * 4 + 2 * inner_total + 1 at most (a step's last product launch may only find the solve
               ended).
  bound_us     one product launch against its bytes: entries x 336 (W_p and the neighbour's six doubles) at 6.3 TB/s.
`--trace DIR` adds product_us: DIR holds the kernel trace of a run of its own of this tool WITH THE SAME ARGUMENTS,
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pairs_solve_bench.py ... --out ''
and product_us is the median of the longer half of solve_product_kernel's dispatches of a list (the shorter ones returned at once).
Not here: the same solve by one host thread (there is no tools/pairs_solve_host.cpp yet).
Prints one JSON line per row, then a table; --out receives the text of every --prepend file, then both.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
import pairs_cycles_bench as PCB  # noqa: E402  (the lists, the rotations, the trace reader)

KERNELS = ("solve_product_kernel",)
HBM_BYTES_PER_US = 6.3e6  # 6.3 TB/s achievable
NOISE_RAD, NOISE_TRANS = 0.01, 0.02


def noisy(rt, seed):
    rng = np.random.default_rng(seed)
    N = PCB.rotations(rng, len(rt), 0.0, NOISE_RAD)
    d = rng.normal(size=(len(rt), 3)); d *= (rng.uniform(0, NOISE_TRANS, len(rt)) / np.linalg.norm(d, axis=1))[:, None]
    out = rt.astype(np.float64)
    out[:, :9] = (N @ out[:, :9].reshape(-1, 3, 3)).reshape(-1, 9)
    out[:, 9:] = (N @ rt[:, 9:].astype(np.float64)[:, :, None])[:, :, 0] + d
    return out.astype(np.float32)


def from_pairs(n_sets, pairs, seed):
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs)
    R, t = PCB.rotations(rng, n_sets), rng.uniform(-1, 1, (n_sets, 3))
    Rab = np.swapaxes(R[pairs[:, 1]], 1, 2) @ R[pairs[:, 0]]
    tab = (np.swapaxes(R[pairs[:, 1]], 1, 2) @ (t[pairs[:, 0]] - t[pairs[:, 1]])[:, :, None])[:, :, 0]
    return pairs.astype(np.uint32), np.concatenate([Rab.reshape(-1, 9), tab], axis=1).astype(np.float32)


def make(name):
    """-> (n_sets, pairs, clean poses)"""
    if name == "ring40":
        return (40,) + from_pairs(40, [(i, (i + 1) % 40) for i in range(40)], 40)
    if name == "strip200":
        rng = np.random.default_rng(200)
        pairs = [(i, i + 1) for i in range(199)]
        seen = set(pairs)
        while len(pairs) < 239:
            i, k = sorted(int(v) for v in rng.integers(0, 200, 2))
            if k - i >= 10 and (i, k) not in seen:
                seen.add((i, k)); pairs.append((i, k))
        return (200,) + from_pairs(200, pairs, 201)
    S = int(name)
    pairs, rt, _R, _t = PCB.make_list(S, {64: None, 512: 10, 2048: 98}.get(S, 10), 100 + S)
    return S, pairs, rt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", default="64,512,2048,ring40,strip200")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_solve.txt"))
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
    taken = 0
    sp = pkg.make_sync_params(1e-4, 1e-4, max_rounds=32)
    vp = pkg.make_solve_params(1e-6, 1e-6, 1e-3)
    ops = 2 + 5 + vp.max_outer * (4 + 2 * vp.max_inner)
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
        for name in a.lists.split(","):
            S, pairs, exact = make(name)
            P = len(pairs)
            entries = 2 * P
            rt = noisy(exact, 300 + S)
            d_pose = torch.from_numpy(rt).to(dev)
            d_sset = torch.zeros(S * 160, dtype=torch.uint8, device=dev); d_spair = torch.zeros(P * 32, dtype=torch.uint8, device=dev)
            d_ssum = torch.zeros(32, dtype=torch.uint8, device=dev)
            d_set = torch.zeros(S * 160, dtype=torch.uint8, device=dev); d_pair = torch.zeros(P * 48, dtype=torch.uint8, device=dev)
            d_sum = torch.zeros(64, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            sync = lambda: reg.pairs_sync_device(S, pairs, sp, d_pose.data_ptr(), 48, 0, 4, 0, d_sset.data_ptr(), d_spair.data_ptr(), d_ssum.data_ptr())  # noqa: E731
            one = lambda: reg.pairs_solve_device(S, pairs, vp, d_pose.data_ptr(), 48, 0, 4, 0, 288, d_sset.data_ptr(), 160, d_set.data_ptr(),  # noqa: E731
                                                 d_pair.data_ptr(), d_sum.data_ptr())
            sync(); one(); torch.cuda.synchronize()
            summ = np.frombuffer(d_sum.cpu().numpy().tobytes(), pkg.SOLVE_SUMMARY_DTYPE)[0]
            ssum = np.frombuffer(d_ssum.cpu().numpy().tobytes(), pkg.SYNC_SUMMARY_DTYPE)[0]
            t_host = []
            for it in range(a.warmup + a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); one(); t_host.append((time.perf_counter() - t0) * 1e6)
            host_us = med(t_host[a.warmup:])
            t_dev = [gated(one, host_us) for it in range(a.warmup + a.repeats)][a.warmup:]
            t_sync = [gated(sync, host_us) for it in range(a.warmup + a.repeats)][a.warmup:]
            torch.cuda.synchronize()
            K, stop, inner = int(summ["outer"]), int(summ["stop"]), int(summ["inner_total"])
            J = K + 1 if stop == pkg.SC_SOLVE_STOP_ROSE else K
            row = dict(list=name, sets=S, pairs=P, sync_rounds=int(ssum["rounds"]), sync_converged=int(ssum["converged"]), K=K, stop=stop, inner_total=inner,
                       cost0=float(summ["cost0"]), cost=float(summ["cost"]), host_us=host_us, device_us=med(t_dev),
                       device_min_max=[round(min(t_dev), 1), round(max(t_dev), 1)], sync_us=med(t_sync), ops=ops, working=4 + 4 * J + 2 * inner + J + 1,
                       bound_us=round(entries * 336 / HBM_BYTES_PER_US, 3))
            calls = 1 + 2 * (a.warmup + a.repeats)
            if trace is not None:
                per = vp.max_outer * vp.max_inner
                mine = np.array(trace[KERNELS[0]][taken: taken + calls * per]); taken += calls * per
                if len(mine) == calls * per:
                    mine = np.sort(mine.reshape(calls, per)[1 + a.warmup:], axis=1)[:, per - max(inner, 1):]  # the dispatches that worked
                    row["product_us"] = round(float(np.median(mine)), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/pairs_solve_bench.py: one sc_pairs_solve_device call behind sc_pairs_sync_device; max_outer 8, max_inner 64, tolerances 1e-6, cg_tol 1e-3"
                 + (" (product_us: a kernel trace taken in a run of its own)" if trace else " (no kernel trace: the launches' own times are not measured)"))
    cols = ["list", "sets", "pairs", "K", "stop", "inner_total", "host_us", "device_us", "sync_us", "ops", "working", "bound_us"] + (["product_us"] if trace else [])
    table = ["  ".join(f"{c:>12}" for c in cols)] + ["  ".join(f"{str(r.get(c, '-')):>12}" for c in cols) for r in rows]
    print("\n".join(table))
    lines += table + [json.dumps(r) for r in rows]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
