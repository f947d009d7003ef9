#!/usr/bin/env python3
"""What a round of sc_peel costs (include/saccot.h): the C2-shaped two-motion scene, inputs resident in HBM.

  python tools/peel_bench.py [--steps 50] [--warmup 5] [--config C2]

After `warmup` frames, `steps` x (frame, round 1, round 2):
  wall_us        median wall time of sc_peel_device per round, by the host clock (the call waits for its winner);
  bracket_us     the same rounds behind frames that ask for SC_FLAG_TIMING: the HIP-event brackets around the round's launches
                 (compact = the claim + compact launch, score, argmax, mask = the winner / mask launch), in a loop of its own;
  instances      wall time of register_instances (two motions) against what a caller does without sc_peel: sc_register, compaction
                 of the unclaimed correspondences on the host, sc_register again.
Prints one JSON line.  The yardstick the round is held against is bench.py --full's stage_us.score + argmax + mask.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def med(x):
    return round(float(np.median(x)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="C2")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    cfg = pkg.synth.CONFIGS[a.config]
    sc = pkg.synth.make_scene_motions(cfg.n, [0.6 * cfg.rho, 0.4 * cfg.rho], cfg.L, cfg.tau, cfg.seed)
    dev = torch.device("cuda:0")
    ds, dt = torch.from_numpy(sc.src).to(dev), torch.from_numpy(sc.tgt).to(dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
    d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    kw = cfg.params()
    out = dict(config=a.config, n=cfg.n, T=cfg.T, steps=a.steps, warmup=a.warmup, c2_kernel_of_a_round="plain fp32 (launch_score) on the compacted planes")
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        for timed in (False, True):
            p = pkg.make_params(flags=pkg.SC_FLAG_TIMING if timed else 0, **kw)
            wall = {1: [], 2: []}
            frame_wall, counts = [], []
            br = {1: {k: [] for k in ("us_stage", "us_score", "us_argmax", "us_mask", "us_total")}, 2: None}
            br[2] = {k: [] for k in br[1]}
            for it in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                rc, st = r.register_device(ds.data_ptr(), dt.data_ptr(), cfg.n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                t1 = time.perf_counter()
                assert rc == 0
                row = [st["best_count"]]
                for rnd in (1, 2):
                    t2 = time.perf_counter()
                    rc, ps = r.peel_device(d_Rt.data_ptr(), d_mask.data_ptr())
                    t3 = time.perf_counter()
                    assert rc == 0
                    row.append(ps["best_count"])
                    if it >= a.warmup:
                        wall[rnd].append((t3 - t2) * 1e6)
                        for k in br[rnd]:
                            br[rnd][k].append(ps[k])
                if it >= a.warmup:
                    frame_wall.append((t1 - t0) * 1e6)
                counts = row
            torch.cuda.synchronize()
            if not timed:
                out["best_counts"] = counts
                out["frame_wall_us"] = med(frame_wall)
                out["wall_us"] = {f"round{k}": med(v) for k, v in wall.items()}
                out["fast_path_of_last_frame"] = r.debug_last()["fast_path"]
            else:
                out["bracket_us"] = {f"round{k}": dict(compact=med(v["us_stage"]), score=med(v["us_score"]), argmax=med(v["us_argmax"]),
                                                       mask=med(v["us_mask"]), total=med(v["us_total"])) for k, v in br.items()}
        # frame + rounds in one call against two whole calls with a host compaction in between
        p = pkg.make_params(**kw)
        one, two = [], []
        for it in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            res = r.register_instances(sc.src, sc.tgt, max_instances=2, min_score=0, params=p)
            t1 = time.perf_counter()
            assert len(res["score"]) == 2
            if it >= a.warmup:
                one.append((t1 - t0) * 1e6)
        for it in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            f = r.register(sc.src, sc.tgt, params=p)
            rest = f["mask"] == 0
            s2, t2 = np.ascontiguousarray(sc.src[rest]), np.ascontiguousarray(sc.tgt[rest])
            g = r.register(s2, t2, params=p)
            t1 = time.perf_counter()
            assert g["status"] == 0
            if it >= a.warmup:
                two.append((t1 - t0) * 1e6)
        out["instances"] = dict(register_instances_2_motions_wall_us=med(one), two_sc_register_with_host_compaction_wall_us=med(two),
                                second_motion_inliers=[int(res["score"][1]), int(g["stats"]["best_count"])])
    finally:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
