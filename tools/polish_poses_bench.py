#!/usr/bin/env python3
"""What refitting K poses on a frame costs (include/saccot.h, sc_polish_poses) beside sc_polish's polish launch on the same K poses,
everything resident in HBM.

  python tools/polish_poses_bench.py [--configs C2,C1] [--poses 1,8,64] [--max-iter 16] [--repeats 30] [--warmup 5]
                                     [--out profiles/polish_poses.txt] [--prepend FILE ...]

Per config: the config's own scene, registered once with SC_FLAG_TIMING: the frame every timed call then runs on.  Per K, so that both
launches do the same work, the poses handed to sc_polish_poses_device are the frame's fp32 hypotheses that sc_polish(candidates = K)
selects — the CPU restatement's hypotheses at the ranks of the candidates' records —, no selection, the same max_iter; the tool checks
that the records then agree with sc_polish_cand bit for bit (Rt, score0, score, iters) and reports it.  Device time, median of
`repeats` after `warmup`, in microseconds, the two calls ALTERNATING in one loop of one session:
  polish_launch_us   the HIP-event bracket around sc_polish_device's polish launch (us_score of its sc_stats), candidates = K;
  poses_us           a HIP-event pair on the context's stream around one sc_polish_poses_device call (no mask);
  poses_mask_us      the same with d_mask given (K x n bytes);
  poses_b2b_us       ten such calls (no mask) between one event pair, per call: the GPU never waits for the host's next enqueue;
  sel_mask_us, sel_alive_us   the first again with a selection that admits every correspondence — SEL_MASK over n ones, SEL_ALIVE over
                     n labels of -1 —: the same refits on the same bits, plus what evaluating the selection per index costs.
Both brackets hold one launch between two event records.  Prints one JSON line per (config, K), then a table; --out receives the
text of every --prepend file (the compiler's resource lines, taken without a GPU), then both.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def pair(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C1")
    ap.add_argument("--poses", default="1,8,64")
    ap.add_argument("--max-iter", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polish_poses.txt"))
    ap.add_argument("--prepend", action="append", default=[])
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    O = ge.load_oracle()
    dev = torch.device("cuda:0")
    threads = min(O.max_threads(), 16)
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    span = lambda v: [round(float(min(v)), 1), round(float(max(v)), 1)]  # noqa: E731
    rows = []
    for name in a.configs.split(","):
        cfg, sc = pkg.synth.make_config_scene(name)
        n, kw = cfg.n, cfg.params()
        # the frame's hypotheses in ranked order, on the CPU restatement (bit for bit the frame's: tests/test_gpu_parity.py)
        S, bits, deg = O.compat(sc.src, sc.tgt, kw["sigma"], kw["t_cmp"], kw["min_len"], kw["tau"], threads=threads)
        tri, _, _ = O.triangles(S, bits, deg, kw["max_triangles"], kw["rank_mode"], threads=threads)
        hyp = O.kabsch3(sc.src, sc.tgt, tri, threads=threads)
        del S, bits
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            d_src, d_tgt = torch.from_numpy(sc.src).to(dev), torch.from_numpy(sc.tgt).to(dev)
            d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_ones = torch.ones(n, dtype=torch.uint8, device=dev); d_minus = torch.full((n,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            p = pkg.make_params(**kw, flags=pkg.SC_FLAG_TIMING)
            for _ in range(a.warmup):
                rc, fs = reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                assert rc == 0, rc
            for K in (int(x) for x in a.poses.split(",")):
                q = pkg.make_polish_params(candidates=K, max_iter=a.max_iter)
                qp = pkg.make_polish_poses_params(max_iter=a.max_iter)
                d_cand = torch.zeros(K * 64, dtype=torch.uint8, device=dev); d_k = torch.zeros(1, dtype=torch.int32, device=dev)
                rc, _ = reg.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr(), d_cand.data_ptr(), d_k.data_ptr())
                assert rc == 0, rc
                torch.cuda.synchronize()
                found = int(d_k.cpu()[0])
                assert found == K, f"{name}: {found} candidates for K = {K}"
                cand = np.frombuffer(d_cand.cpu().numpy().tobytes(), pkg.api.POLISH_CAND_DTYPE)
                poses = np.ascontiguousarray(hyp[cand["rank"]])
                d_pose = torch.from_numpy(poses).to(dev)
                d_pol = torch.zeros(K * 64, dtype=torch.uint8, device=dev); d_pmask = torch.zeros(K * n, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                polish = lambda: reg.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr(), d_cand.data_ptr(), d_k.data_ptr())[1]["us_score"]  # noqa: E731
                plain = lambda: reg.polish_poses_device(qp, d_pose.data_ptr(), 48, K, 0, d_pol.data_ptr(), 0)  # noqa: E731
                masked = lambda: reg.polish_poses_device(qp, d_pose.data_ptr(), 48, K, 0, d_pol.data_ptr(), d_pmask.data_ptr())  # noqa: E731
                qm = pkg.make_polish_poses_params(max_iter=a.max_iter, sel_mode=pkg.SC_POLISH_POSES_SEL_MASK)
                qa = pkg.make_polish_poses_params(max_iter=a.max_iter, sel_mode=pkg.SC_POLISH_POSES_SEL_ALIVE)
                d_pol2 = torch.zeros(K * 64, dtype=torch.uint8, device=dev)
                sel_mask = lambda: reg.polish_poses_device(qm, d_pose.data_ptr(), 48, K, d_ones.data_ptr(), d_pol2.data_ptr(), 0)  # noqa: E731
                sel_alive = lambda: reg.polish_poses_device(qa, d_pose.data_ptr(), 48, K, d_minus.data_ptr(), d_pol2.data_ptr(), 0)  # noqa: E731
                t_pol, t_pose, t_mask, t_b2b, t_sm, t_sa = [], [], [], [], [], []
                for it in range(a.warmup + a.repeats):  # alternating: the two launches meet the same neighbours on the machine
                    v = (polish(), pair(torch, stream, plain), pair(torch, stream, masked),
                         pair(torch, stream, lambda: [plain() for _ in range(10)]) / 10, pair(torch, stream, sel_mask),
                         pair(torch, stream, sel_alive))
                    if it >= a.warmup:
                        for t, x in zip((t_pol, t_pose, t_mask, t_b2b, t_sm, t_sa), v):
                            t.append(x)
                torch.cuda.synchronize()
                rec = np.frombuffer(d_pol.cpu().numpy().tobytes(), pkg.POLISH_BATCH_RESULT_DTYPE)
                agree = bool(all(rec[f].tobytes() == cand[f].tobytes() for f in ("Rt", "score0", "score", "iters")) and (rec["status"] == 0).all())
                assert d_pol2.cpu().numpy().tobytes() == rec.tobytes(), "a selection that admits everything changed a record"
                row = dict(config=name, n=n, K=K, max_iter=a.max_iter, records_agree_with_sc_polish=agree, refits=int(rec["iters"].sum()),
                           polish_launch_us=med(t_pol), polish_launch_min_max=span(t_pol), poses_us=med(t_pose), poses_min_max=span(t_pose),
                           poses_mask_us=med(t_mask), poses_b2b_us=med(t_b2b), sel_mask_us=med(t_sm), sel_alive_us=med(t_sa), poses_over_polish=round(med(t_pose) / med(t_pol), 4))
                rows.append(row)
                print(json.dumps(row), flush=True)
        finally:
            reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/polish_poses_bench.py: one sc_polish_poses_device call beside sc_polish_device's polish launch, the same K poses")
    lines += [json.dumps(r) for r in rows]
    table = ["", f"{'config':>6} {'n':>6} {'K':>3} | {'polish launch us (min .. max)':>32} {'poses us (min .. max)':>28} {'with mask':>10} {'b2b':>8} {'SEL_MASK':>9} {'SEL_ALIVE':>10} "
                 f"{'poses/polish':>13} {'refits':>7}  agree"]
    for r in rows:
        pl = f"{r['polish_launch_us']:.1f} ({r['polish_launch_min_max'][0]:.1f} .. {r['polish_launch_min_max'][1]:.1f})"
        ps = f"{r['poses_us']:.1f} ({r['poses_min_max'][0]:.1f} .. {r['poses_min_max'][1]:.1f})"
        table.append(f"{r['config']:>6} {r['n']:>6} {r['K']:>3} | {pl:>32} {ps:>28} {r['poses_mask_us']:>10.1f} {r['poses_b2b_us']:>8.1f} {r['sel_mask_us']:>9.1f} {r['sel_alive_us']:>10.1f} "
                     f"{r['poses_over_polish']:>13.4f} {r['refits']:>7}  {r['records_agree_with_sc_polish']}")
    print("\n".join(table))
    lines += table
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
