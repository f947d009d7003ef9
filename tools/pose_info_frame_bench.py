#!/usr/bin/env python3
"""What the information matrices of a frame's poses cost (include/saccot.h, sc_pose_info_frame), everything resident in HBM.

  python tools/pose_info_frame_bench.py [--sizes 5000,20000,1048576] [--poses 1,8,64] [--repeats 20] [--warmup 3]
                                        [--out profiles/pose_info_frame.txt] [--append FILE ...]

Per n: one scene of bench.py's C2 shape (rho = 0.15, L = 3, tau = 0.10, T = 50 000, weight ranking; n = 5000 IS C2), registered once
with sc_register_device: the frame every timed call then runs on.  Device time by a HIP event pair on the context's stream, median of
`repeats` after `warmup`, in microseconds:
  frame      one sc_register_device call (the frame itself, waited);
  peel       one sc_peel_device round — every repeat is the NEXT round of the frame, as a caller's loop would run them;
  polish     one sc_polish_device call, candidates 8, max_iter 16;
  info       one sc_pose_info_frame_device call on n_poses of the polished records (stride 64, the 8 records repeated), no selection.
From 2^17 correspondences on the frame is registered with SC_FLAG_NO_DENSE_S (the dense score matrix would not fit) and T = 2000.  A
size whose FRAME the library refuses (the n x n bit rows of stage A outgrow the workspace cap long before n = 2^24) is reported as
not measured, with the library's words: there is then no frame to take a pose's matrix on.
Prints one JSON line per (n, n_poses), then a table; --out receives both, followed by the text of every --append file (the
headline's bench.py lines, taken in the same session).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def timed(torch, stream, fn, warmup, repeats):
    out = []
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000,1048576")
    ap.add_argument("--poses", default="1,8,64")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_info_frame.txt"))
    ap.add_argument("--append", action="append", default=[])
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    cfg = pkg.synth.CONFIGS["C2"]
    q = pkg.make_polish_params(candidates=8, max_iter=16)
    ip = pkg.make_pose_info_params()
    med = lambda v: float(np.median(v))  # noqa: E731
    rows, lines = [], []
    for n in (int(x) for x in a.sizes.split(",")):
        big = n >= (1 << 17)
        kw = dict(cfg.params(), max_triangles=2000 if big else cfg.T)
        p = pkg.make_params(**kw, flags=pkg.api.SC_FLAG_NO_DENSE_S if big else 0)
        sc = pkg.synth.make_scene(n, cfg.rho, cfg.L, cfg.tau, cfg.seed)
        reg = pkg.Registrar(0)
        stream = torch.cuda.Stream(device=dev)
        reg.set_stream(stream.cuda_stream)
        try:
            d_src, d_tgt = torch.from_numpy(sc.src).to(dev), torch.from_numpy(sc.tgt).to(dev)
            d_Rt = torch.zeros(12, dtype=torch.float32, device=dev); d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
            d_cand = torch.zeros(8 * 64, dtype=torch.uint8, device=dev); d_k = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def frame():
                rc, _ = reg.register_device(d_src.data_ptr(), d_tgt.data_ptr(), n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                assert rc == 0, rc

            try:
                t_frame = timed(torch, stream, frame, a.warmup if not big else 1, a.repeats if not big else 3)
            except (pkg.SacCotError, AssertionError) as e:
                lines.append(json.dumps(dict(n=n, not_measured=f"the frame is refused: {e}")))
                print(lines[-1], flush=True)
                continue
            t_pol = timed(torch, stream, lambda: reg.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr(), d_cand.data_ptr(), d_k.data_ptr()),
                          a.warmup, a.repeats)
            torch.cuda.synchronize()
            K = int(d_k.cpu()[0])
            cand = np.frombuffer(d_cand.cpu().numpy().tobytes(), pkg.api.POLISH_CAND_DTYPE)
            for n_poses in (int(x) for x in a.poses.split(",")):
                poses = cand[np.arange(n_poses) % max(K, 1)]
                d_pose = torch.from_numpy(np.frombuffer(poses.tobytes(), np.uint8).copy()).to(dev)
                d_info = torch.zeros(n_poses * 320, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                t_inf = timed(torch, stream, lambda: reg.pose_info_frame_device(ip, d_pose.data_ptr(), 64, n_poses, 0, d_info.data_ptr()),
                              a.warmup, a.repeats)
                torch.cuda.synchronize()
                rec = np.frombuffer(d_info.cpu().numpy().tobytes(), pkg.POSE_INFO_RESULT_DTYPE)
                row = dict(n=n, n_poses=n_poses, candidates=K, statuses_ok=int((rec["status"] == 0).sum()),
                           inliers_mean=round(float(rec["inliers"].mean()), 1),
                           counts_agree=bool(np.array_equal(rec["inliers"], poses["score"])), frame_us=round(med(t_frame), 1),
                           polish_us=round(med(t_pol), 1), info_us=round(med(t_inf), 1),
                           info_us_min_max=[round(float(min(t_inf)), 1), round(float(max(t_inf)), 1)],
                           info_over_polish=round(med(t_inf) / med(t_pol), 4), info_over_frame=round(med(t_inf) / med(t_frame), 4))
                rows.append(row)
            # the rounds last: every repeat peels the next one (a round that finds nothing more still runs its launches)
            t_peel = timed(torch, stream, lambda: reg.peel_device(d_Rt.data_ptr(), d_mask.data_ptr()), 1, min(a.repeats, 8))
            for row in rows:
                if row["n"] == n:
                    row["peel_us"] = round(med(t_peel), 1)
                    row["info_over_peel"] = round(row["info_us"] / med(t_peel), 4)
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
        finally:
            reg.close()
    table = [""]
    table.append(f"{'n':>8} {'poses':>5} | {'frame us':>10} {'peel us':>9} {'polish us':>10} {'info us':>10} {'info/polish':>12} {'info/frame':>11} "
                 f"{'inliers mean':>13}  counts agree")
    for r in rows:
        table.append(f"{r['n']:>8} {r['n_poses']:>5} | {r['frame_us']:>10.1f} {r['peel_us']:>9.1f} {r['polish_us']:>10.1f} {r['info_us']:>10.1f} "
                     f"{r['info_over_polish']:>12.4f} {r['info_over_frame']:>11.4f} {r['inliers_mean']:>13.1f}  {r['counts_agree']}")
    print("\n".join(table))
    lines += table
    for path in a.append:
        lines.append("")
        lines.append(f"---- {os.path.basename(path)}")
        lines += open(path).read().rstrip("\n").split("\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
