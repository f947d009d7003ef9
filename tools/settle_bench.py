#!/usr/bin/env python3
"""What relabelling and refitting K poses to their fixed point costs (include/saccot.h, sc_settle_poses), everything resident in HBM.

  python tools/settle_bench.py [--configs C2,C3] [--poses 2,8,16,64] [--max-iter 16] [--repeats 20] [--warmup 3]
                               [--batch-sizes 128,512] [--batches 64,1024,4096] [--out profiles/settle.txt] [--prepend FILE ...]

The frame form.  Per config (C2: bench.py's shape, n = 5 000; C3: n = 20 000, scored here on one GPU with T = 50 000): a two-motion
scene of the config's size, extent, tau and inlier ratio (synth.make_scene_motions; three fifths of the inliers follow motion 0),
registered once: the frame every timed call then runs on.  The K poses are the two true motions perturbed (a seeded rotation of
about 0.2 tau / L radians and a translation of about 0.2 tau), half of them around each motion.  Per K the three ways to run the loop
alternate in ONE session, each timed by a HIP event pair on the context's stream, median of `repeats` after `warmup`, microseconds:
  fused_us      (a) one sc_settle_poses_frame_device call (max_iter as given): ONE launch; `rounds` and `stop` are its d_rounds;
  composed_us   (b) the loop of the header's equality 1 with exactly R = rounds (+ 1 after FIXED) rounds — sc_assign_poses_frame_device
                (BEST) + sc_polish_poses_device(SEL_LABEL, max_iter 1, STATUS) — and the last assign, enqueued back to back without
                a host read: what a caller who KNEW R would enqueue;
  blind_us      (c) the same with max_iter rounds: what a host-free caller enqueues today.
  per_round_us  fused_us over the rounds the fused call executed (R, plus the labelling pass after MAX_ITER counted as one).
(b) and (c) are built from entries the fused call does not touch.  The poses (b) ends in are compared with (a)'s, bit for bit.
The batch form, beside one sc_register_instances_batch_device call (tools/instances_batch_bench.py's scenes: B two-motion problems of
n correspondences, max_instances 4, min_score 4): one sc_settle_poses_batch_device call on that call's records (stride 80, K = 4).
Prints one JSON line per row, then tables; --out receives the text of every --prepend file (the compiler's resource lines, taken
without a GPU), then both.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

MAX_INSTANCES, MIN_SCORE, DISTINCT = 4, 4, 32
STOP_FIXED = 0


def pair(torch, stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def perturbed(motions, K, tau, L, seed):
    """K poses: pose i is motion i % 2 with a small seeded rotation and translation composed on the left"""
    rng = np.random.default_rng(seed)
    out = np.zeros((K, 12), np.float32)
    for i in range(K):
        R, t = (np.asarray(x, np.float64) for x in motions[i % len(motions)])
        w = rng.normal(size=3) * 0.2 * tau / L
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        dR = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th**2 * (Kx @ Kx)
        out[i, :9] = (dR @ R.reshape(3, 3)).ravel()
        out[i, 9:] = dR @ t.reshape(3) + rng.normal(size=3) * 0.2 * tau
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--poses", default="2,8,16,64")
    ap.add_argument("--max-iter", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-sizes", default="128,512")
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "settle.txt"))
    ap.add_argument("--prepend", action="append", default=[])
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    med = lambda v: round(float(np.median(v)), 1)  # noqa: E731
    PDT = pkg.api.POLISH_BATCH_RESULT_DTYPE
    rows, brows = [], []
    for name in [c for c in a.configs.split(",") if c]:
        cfg = pkg.synth.CONFIGS[name]
        sc = pkg.synth.make_scene_motions(cfg.n, [0.6 * cfg.rho, 0.4 * cfg.rho], cfg.L, cfg.tau, cfg.seed)
        n, kw = cfg.n, dict(cfg.params(), max_triangles=min(cfg.T, 50_000))
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            d_src, d_tgt = torch.from_numpy(sc.src).to(dev), torch.from_numpy(sc.tgt).to(dev)
            d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            rc, _ = reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, pkg.make_params(**kw), d_Rt.data_ptr(), d_mask.data_ptr())
            assert rc == 0, rc
            torch.cuda.synchronize()
            for K in (int(x) for x in a.poses.split(",")):
                poses = perturbed(sc.motions, K, cfg.tau, cfg.L, 77 + K)
                d_pose = torch.from_numpy(poses).to(dev)
                d_pol = torch.zeros(K * 64, dtype=torch.uint8, device=dev)
                d_label = torch.zeros(n, dtype=torch.int32, device=dev); d_rounds = torch.zeros(2, dtype=torch.int32, device=dev)
                d_ping = [torch.zeros(K * 64, dtype=torch.uint8, device=dev) for _ in range(2)]
                d_lab2 = torch.zeros(n, dtype=torch.int32, device=dev); d_asg = torch.zeros(K * 32, dtype=torch.uint8, device=dev)
                sp = pkg.make_settle_params(max_iter=a.max_iter)
                fused = lambda: reg.settle_poses_frame_device(sp, d_pose.data_ptr(), 48, K, 0, d_pol.data_ptr(), d_label.data_ptr(), 0,  # noqa: E731
                                                              d_rounds.data_ptr())
                fused()
                torch.cuda.synchronize()
                R, stop = (int(x) for x in d_rounds.cpu().numpy().view(np.uint32))
                Rc = R + (1 if stop == STOP_FIXED else 0)
                AP, PP = pkg.make_assign_params, pkg.make_polish_poses_params

                def composed(rounds):
                    cur, stride, flag = d_pose, 48, 0
                    for i in range(rounds):
                        nxt = d_ping[i % 2]
                        reg.assign_poses_frame_device(AP(flags=flag), cur.data_ptr(), stride, K, 0, d_lab2.data_ptr(), 0, d_asg.data_ptr())
                        reg.polish_poses_device(PP(max_iter=1, sel_mode=pkg.SC_POLISH_POSES_SEL_LABEL, flags=flag), cur.data_ptr(), stride, K,
                                                d_lab2.data_ptr(), nxt.data_ptr(), 0)
                        cur, stride, flag = nxt, 64, 1
                    reg.assign_poses_frame_device(AP(flags=flag), cur.data_ptr(), stride, K, 0, d_lab2.data_ptr(), 0, d_asg.data_ptr())
                    return cur

                last = composed(Rc)
                torch.cuda.synchronize()
                got = np.frombuffer(d_pol.cpu().numpy().tobytes(), PDT)
                same = bool(Rc == 0 or np.frombuffer(last.cpu().numpy().tobytes(), PDT)["Rt"].tobytes() == got["Rt"].tobytes())
                same = same and bool(np.array_equal(d_lab2.cpu().numpy(), d_label.cpu().numpy()))
                t = {"a": [], "b": [], "c": []}
                for it in range(a.warmup + a.repeats):  # the three alternate
                    t["a"].append(pair(torch, stream, fused))
                    t["b"].append(pair(torch, stream, lambda: composed(Rc)))
                    t["c"].append(pair(torch, stream, lambda: composed(a.max_iter)))
                fa, fb, fc = (med(t[x][a.warmup:]) for x in "abc")
                executed = R + 1  # FIXED: the uncounted round; MAX_ITER: the last labelling pass
                row = dict(config=name, n=n, K=K, max_iter=a.max_iter, rounds=R, stop=stop, labelled=int((d_label.cpu().numpy() >= 0).sum()),
                           fused_us=fa, fused_min_max=[round(min(t["a"][a.warmup:]), 1), round(max(t["a"][a.warmup:]), 1)], composed_us=fb,
                           blind_us=fc, per_round_us=round(fa / executed, 1), composed_over_fused=round(fb / fa, 3),
                           blind_over_fused=round(fc / fa, 3), same_bits=same)
                rows.append(row)
                print(json.dumps(row), flush=True)
        finally:
            reg.close()
    # ---- the batch form beside sc_register_instances_batch_device
    if a.batch_sizes and a.batches:
        p = pkg.make_params(sigma=0.05, t_cmp=0.9, tau=0.05, min_len=0.05, max_triangles=2000)
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            for n in (int(x) for x in a.batch_sizes.split(",")):
                scenes = [pkg.synth.make_scene_motions(n, [0.18, 0.12], 1.0, 0.05, 9500 + n + k) for k in range(DISTINCT)]
                for B in (int(x) for x in a.batches.split(",")):
                    src = np.concatenate([scenes[b % DISTINCT].src for b in range(B)]).astype(np.float32)
                    tgt = np.concatenate([scenes[b % DISTINCT].tgt for b in range(B)]).astype(np.float32)
                    d_src, d_tgt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
                    off = (np.arange(B + 1, dtype=np.uint64) * n).astype(np.uint32)
                    d_res = torch.zeros(MAX_INSTANCES * B * 80, dtype=torch.uint8, device=dev)
                    d_label = torch.zeros(B * n, dtype=torch.int32, device=dev); d_lab2 = torch.zeros(B * n, dtype=torch.int32, device=dev)
                    d_nfound = torch.zeros(B, dtype=torch.int32, device=dev)
                    d_pol = torch.zeros(MAX_INSTANCES * B * 64, dtype=torch.uint8, device=dev)
                    d_rounds = torch.zeros(2 * B, dtype=torch.int32, device=dev)
                    sp = pkg.make_settle_params(max_iter=a.max_iter)
                    torch.cuda.synchronize()
                    ins = lambda: reg.register_instances_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, MAX_INSTANCES, MIN_SCORE,  # noqa: E731
                                                                      d_res.data_ptr(), d_label.data_ptr(), d_nfound.data_ptr())
                    stl = lambda: reg.settle_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, p, sp, d_res.data_ptr(), 80,  # noqa: E731
                                                                MAX_INSTANCES, d_pol.data_ptr(), d_lab2.data_ptr(), d_rounds.data_ptr())
                    t_ins, t_stl = [], []
                    for it in range(a.warmup + a.repeats):  # the two alternate
                        t_ins.append(pair(torch, stream, ins))
                        t_stl.append(pair(torch, stream, stl))
                    torch.cuda.synchronize()
                    rr = d_rounds.cpu().numpy().view(np.uint32).reshape(B, 2)
                    row = dict(n=n, B=B, K=MAX_INSTANCES, instances_us=med(t_ins[a.warmup:]), settle_us=med(t_stl[a.warmup:]),
                               rounds_mean=round(float(rr[:, 0].mean()), 2), rounds_max=int(rr[:, 0].max()),
                               fixed=int((rr[:, 1] == STOP_FIXED).sum()))
                    row["over_instances"] = round(row["settle_us"] / row["instances_us"], 4)
                    row["ns_per_problem_round"] = round(1e3 * row["settle_us"] / (B * (row["rounds_mean"] + 1)), 1)
                    brows.append(row)
                    print(json.dumps(row), flush=True)
        finally:
            reg.close()
    lines = []
    for path in a.prepend:
        lines += open(path).read().rstrip("\n").split("\n") + [""]
    lines.append("---- tools/settle_bench.py: K poses settled on a scored frame; (a) fused, (b) composed with exactly R rounds, (c) composed blind")
    lines += [json.dumps(r) for r in rows]
    table = ["", f"{'config':>6} {'n':>6} {'K':>3} | {'rounds':>6} {'stop':>4} | {'(a) fused us (min .. max)':>30} {'(b) composed':>13} {'(c) blind':>10} | "
                 f"{'per round':>9} {'b / a':>6} {'c / a':>6} {'same bits':>9}"]
    for r in rows:
        t = f"{r['fused_us']:.1f} ({r['fused_min_max'][0]:.1f} .. {r['fused_min_max'][1]:.1f})"
        table.append(f"{r['config']:>6} {r['n']:>6} {r['K']:>3} | {r['rounds']:>6} {r['stop']:>4} | {t:>30} {r['composed_us']:>13.1f} {r['blind_us']:>10.1f} | "
                     f"{r['per_round_us']:>9.1f} {r['composed_over_fused']:>6.2f} {r['blind_over_fused']:>6.2f} {str(r['same_bits']):>9}")
    table += ["", "---- one sc_settle_poses_batch_device call beside one sc_register_instances_batch_device call, K = 4 planes"]
    table += [json.dumps(r) for r in brows]
    table += ["", f"{'n':>4} {'B':>5} | {'instances us':>13} {'settle us':>10} {'settle/instances':>17} | {'rounds mean':>11} {'max':>4} {'fixed':>6} {'ns/problem/round':>17}"]
    for r in brows:
        table.append(f"{r['n']:>4} {r['B']:>5} | {r['instances_us']:>13.1f} {r['settle_us']:>10.1f} {r['over_instances']:>17.4f} | {r['rounds_mean']:>11.2f} "
                     f"{r['rounds_max']:>4} {r['fixed']:>6} {r['ns_per_problem_round']:>17.1f}")
    print("\n".join(table))
    lines += table
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
