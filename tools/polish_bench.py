#!/usr/bin/env python3
"""What sc_polish costs (include/saccot.h): the configs' own scenes, inputs resident in HBM.

  python tools/polish_bench.py [--steps 50] [--warmup 5] [--configs C1,C2] [--candidates 8] [--max-iter 16]

Per config, after `warmup` frames, `steps` x (frame, polish):
  frame_wall_us   median wall time of sc_register_device by the host clock (the frame of the same session);
  wall_us         median wall time of sc_polish_device (the call waits for its winner);
  bracket_us      the same behind frames that ask for SC_FLAG_TIMING, in a loop of its own: the HIP-event brackets around the three
                  launches (select = candidate selection, polish = every refit of every candidate, mask = winner + mask);
  refine_us       what ONE refit costs as refine_kernel runs it: the us_mask bracket of a frame with SC_FLAG_REFINE minus the same
                  bracket of a frame without (both with SC_FLAG_TIMING);
  iters           refits that changed (R, t), per candidate, and the frame's and the polished best_count.
Prints one JSON line per config.
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


def run(pkg, torch, name, a):
    cfg, sc = pkg.synth.make_config_scene(name)
    dev = torch.device("cuda:0")
    ds, dt = torch.from_numpy(sc.src).to(dev), torch.from_numpy(sc.tgt).to(dev)
    d_Rt = torch.zeros(12, dtype=torch.float32, device=dev)
    d_mask = torch.zeros(cfg.n, dtype=torch.uint8, device=dev)
    d_cand = torch.zeros(a.candidates * 16, dtype=torch.int32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = cfg.params()
    q = pkg.make_polish_params(a.candidates, a.max_iter)
    out = dict(config=name, n=cfg.n, T=cfg.T, steps=a.steps, warmup=a.warmup, candidates=a.candidates, max_iter=a.max_iter)
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        for timed in (False, True):
            p = pkg.make_params(flags=pkg.SC_FLAG_TIMING if timed else 0, **kw)
            frame_wall, wall = [], []
            br = {k: [] for k in ("us_stage", "us_score", "us_mask", "us_total")}
            for it in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                rc, fs = r.register_device(ds.data_ptr(), dt.data_ptr(), cfg.n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                t1 = time.perf_counter()
                assert rc == 0
                rc, ps = r.polish_device(q, d_Rt.data_ptr(), d_mask.data_ptr(), d_cand.data_ptr(), d_n.data_ptr())
                t2 = time.perf_counter()
                assert rc == 0
                if it >= a.warmup:
                    frame_wall.append((t1 - t0) * 1e6)
                    wall.append((t2 - t1) * 1e6)
                    for k in br:
                        br[k].append(ps[k])
            torch.cuda.synchronize()
            if not timed:
                cand = np.frombuffer(d_cand.cpu().numpy().tobytes(), dtype=pkg.api.POLISH_CAND_DTYPE)[: int(d_n.cpu()[0])]
                out.update(frame_wall_us=med(frame_wall), wall_us=med(wall), fast_path_of_last_frame=r.debug_last()["fast_path"],
                           frame_best_count=fs["best_count"], polished_best_count=ps["best_count"], polished_best_rank=ps["best_rank"],
                           iters=[int(c["iters"]) for c in cand], score0=[int(c["score0"]) for c in cand], score=[int(c["score"]) for c in cand])
            else:
                out["bracket_us"] = dict(select=med(br["us_stage"]), polish=med(br["us_score"]), mask=med(br["us_mask"]), total=med(br["us_total"]))
        # one refit as refine_kernel runs it: the mask bracket with and without SC_FLAG_REFINE
        m = {}
        for flag in (0, pkg.SC_FLAG_REFINE):
            p = pkg.make_params(flags=pkg.SC_FLAG_TIMING | flag, **kw)
            v = []
            for it in range(a.warmup + a.steps):
                rc, fs = r.register_device(ds.data_ptr(), dt.data_ptr(), cfg.n, p, d_Rt.data_ptr(), d_mask.data_ptr())
                assert rc == 0
                if it >= a.warmup:
                    v.append(fs["us_mask"])
            m[flag] = med(v)
        out["refine_us"] = dict(mask_bracket=m[0], mask_bracket_with_refine=m[pkg.SC_FLAG_REFINE], one_refit=round(m[pkg.SC_FLAG_REFINE] - m[0], 2))
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="C1,C2")
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--max-iter", type=int, default=16)
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    for name in a.configs.split(","):
        print(json.dumps(run(pkg, torch, name, a)), flush=True)


if __name__ == "__main__":
    main()
