#!/usr/bin/env python3
"""What the gate of sc_match_guided costs and what it saves (include/saccot.h): 5000 x 5300 keypoints with descriptors, resident in HBM.

  python tools/match_guided_bench.py [--steps 50] [--warmup 5] [--dims 33,352] [--parent-lib PATH] [--rounds 2]

Device time by HIP events around one call on the context's stream (memset + distance + finish launches), median over --steps calls
after --warmup.  Per descriptor length D, k = 1, plain and mutual:
  plain_us          sc_match_device of this tree, in this process;
  plain_rounds      the same in fresh child processes, alternating between --parent-lib (a libsaccot.so built from the parent commit)
                    and this tree's library, --rounds times each: the two must agree within the spread of the rounds;
  guided_open_us    sc_match_guided_device with a gate that admits everything: the price of the gate (points staged, 32 residuals
                    per thread and tile, the finiteness scan; no tile drops out).  Its output is checked against sc_match_device's;
  guided_random_us  gate = 0.05 of the scene's extent, keypoints in random order: hardly a tile drops out, cells do;
  guided_morton_us  the same scene with both sets sorted along a Morton curve (the targets by their position in the source frame):
                    whole tiles drop out.  tiles_kept: the share of (row block, column tile) pairs with an admissible cell.
Prints one JSON line; --table also prints the rows as text.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NS, NT, GATE, OPEN = 5000, 5300, 0.05, 1e18


def med(x):
    return round(float(np.median(x)), 2)


def events_us(torch, fn, steps, warmup):
    out = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def scene(D, seed=1):
    """source keypoints in the unit cube, a random pose, the first third of the targets posed copies of source rows (point noise 0.01,
    descriptor noise 0.3), the rest random in the posed cube; in random order"""
    rng = np.random.default_rng(seed)
    src = rng.random((NS, 3))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = rng.standard_normal(3) * 0.5
    tgt = rng.random((NT, 3)) @ q.T + t
    fsrc = rng.standard_normal((NS, D)).astype(np.float32)
    ftgt = rng.standard_normal((NT, D)).astype(np.float32)
    m = NT // 3
    rows = rng.permutation(NS)[:m]
    tgt[:m] = src[rows] @ q.T + t + 0.01 * rng.standard_normal((m, 3))
    ftgt[:m] = fsrc[rows] + np.float32(0.3) * rng.standard_normal((m, D)).astype(np.float32)
    perm = rng.permutation(NT)
    Rt = np.concatenate([q.ravel(), t]).astype(np.float32)
    return src.astype(np.float32), fsrc, tgt[perm].astype(np.float32), ftgt[perm], Rt, q, t


def morton_order(p):
    """rows of p (in the unit cube, roughly) along a Morton curve of 10 bits an axis"""
    g = np.clip((p * 1024).astype(np.int64), 0, 1023)
    code = np.zeros(len(p), np.int64)
    for b in range(10):
        for c in range(3):
            code |= ((g[:, c] >> b) & 1) << (3 * b + c)
    return np.argsort(code, kind="stable")


def tiles_kept(src, tgt, q, t, gate):
    """the share of (128-row block, 64-column tile) pairs that hold a pair of points within the gate (fp64: a figure, not the rule)"""
    posed = src.astype(np.float64) @ q.T + t
    kept = total = 0
    for r0 in range(0, len(src), 128):
        d2 = ((posed[r0:r0 + 128, None, :] - tgt[None, :, :].astype(np.float64)) ** 2).sum(axis=2).min(axis=0)
        hit = d2 < gate * gate
        n_tiles = (len(tgt) + 63) // 64
        kept += sum(bool(hit[c0 * 64:(c0 + 1) * 64].any()) for c0 in range(n_tiles))
        total += n_tiles
    return round(kept / total, 4)


class PlainLib:
    """sc_match_device of ONE libsaccot.so through ctypes of its own: the parent commit's library has no sc_match_guided entries, so
    the package's loader (which declares every prototype) cannot open it"""

    def __init__(self, path, stream):
        import ctypes as C
        self.C, self.L, self.h = C, C.CDLL(path), C.c_void_p()
        vp = C.c_void_p
        self.L.sc_create.argtypes = [C.c_int, C.POINTER(vp)]
        self.L.sc_destroy.argtypes = [vp]; self.L.sc_destroy.restype = None
        self.L.sc_set_stream.argtypes = [vp, vp]
        self.L.sc_match_device.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp]
        if self.L.sc_create(0, C.byref(self.h)) != 0 or self.L.sc_set_stream(self.h, vp(stream if stream else 1)) != 0:
            raise SystemExit("sc_create / sc_set_stream failed")

    def match_device(self, da, ns, db, nt, mp, d_corr, d_d2, d_cnt):
        if self.L.sc_match_device(self.h, da, ns, db, nt, self.C.byref(mp), d_corr, d_d2, d_cnt) != 0:
            raise SystemExit("sc_match_device failed")

    def close(self):
        self.L.sc_destroy(self.h)


def run_plain(pkg, torch, dims, steps, warmup, lib_path):
    dev = torch.device("cuda:0")
    out = {}
    r = PlainLib(lib_path, torch.cuda.current_stream().cuda_stream)
    try:
        for D in dims:
            _, fsrc, _, ftgt, _, _, _ = scene(D)
            da, db = torch.from_numpy(fsrc).to(dev), torch.from_numpy(ftgt).to(dev)
            d_corr = torch.zeros((NS, 2), dtype=torch.int32, device=dev); d_d2 = torch.zeros(NS, dtype=torch.float32, device=dev)
            d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
            for name, mutual in (("plain", False), ("mutual", True)):
                mp = pkg.api.make_match_params(D, mutual=mutual)
                us = events_us(torch, lambda: r.match_device(da.data_ptr(), NS, db.data_ptr(), NT, mp, d_corr.data_ptr(), d_d2.data_ptr(),
                                                             d_cnt.data_ptr()), steps, warmup)
                out[f"{D}_{name}"] = dict(us=med(us), min_us=round(min(us), 2), n=d_cnt.cpu().tolist()[0])
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dims", default="33,352")
    ap.add_argument("--parent-lib", default=None, help="a libsaccot.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--lib", default=None, help="(child) measure sc_match_device of this library only")
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = ge.load_package()
    dims = [int(x) for x in a.dims.split(",")]
    if a.lib:  # a child: the plain matcher of one library, nothing else
        print(json.dumps(run_plain(pkg, torch, dims, a.steps, a.warmup, os.path.abspath(a.lib))))
        return
    out = dict(ns=NS, nt=NT, gate=GATE, steps=a.steps, warmup=a.warmup, by_dim={})
    # the plain matcher of both libraries, each in processes of its own, alternating
    rounds = []
    libs = ([("parent", a.parent_lib)] if a.parent_lib else []) + [("tree", pkg.api.LIB_PATH)]
    for k in range(a.rounds):
        for who, lib in libs:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--steps", str(a.steps), "--warmup", str(a.warmup),
                                  "--dims", a.dims], capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(f"the {who} child failed ({res.returncode}): {res.stderr[-2000:]}")
            rounds.append(dict(lib=who, round=k, **{key: v["us"] for key, v in json.loads(res.stdout.strip().splitlines()[-1]).items()}))
    out["plain_rounds"] = rounds
    own = run_plain(pkg, torch, dims, a.steps, a.warmup, pkg.api.LIB_PATH)
    dev = torch.device("cuda:0")
    r = pkg.Registrar(0)
    try:
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        for D in dims:
            src, fsrc, tgt, ftgt, Rt, q, t = scene(D)
            so, to = morton_order(src), morton_order((tgt.astype(np.float64) - t) @ q)
            orders = dict(random=(src, fsrc, tgt, ftgt), morton=(src[so], fsrc[so], tgt[to], ftgt[to]))
            row = dict(tiles_kept_random=tiles_kept(src, tgt, q, t, GATE), tiles_kept_morton=tiles_kept(src[so], tgt[to], q, t, GATE))
            d_Rt = torch.from_numpy(Rt).to(dev)
            d_corr = torch.zeros((NS, 2), dtype=torch.int32, device=dev); d_d2 = torch.zeros(NS, dtype=torch.float32, device=dev)
            d_g2 = torch.zeros(NS, dtype=torch.float32, device=dev); d_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
            for name, mutual in (("plain", False), ("mutual", True)):
                mp = pkg.api.make_match_params(D, mutual=mutual)
                cell = dict(plain_us=own[f"{D}_{name}"]["us"], n_plain=own[f"{D}_{name}"]["n"])
                for what, order, gate in (("open", "random", OPEN), ("random", "random", GATE), ("morton", "morton", GATE)):
                    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in orders[order]]
                    gp = pkg.make_guide_params(gate)
                    us = events_us(torch, lambda: r.match_guided_device(d[0].data_ptr(), d[1].data_ptr(), NS, d[2].data_ptr(), d[3].data_ptr(), NT,
                                                                        mp, gp, d_Rt.data_ptr(), d_corr.data_ptr(), d_d2.data_ptr(),
                                                                        d_g2.data_ptr(), d_cnt.data_ptr()), a.steps, a.warmup)
                    n, flag = d_cnt.cpu().tolist()
                    assert flag == 0
                    cell[f"guided_{what}_us"] = med(us); cell[f"guided_{what}_min_us"] = round(min(us), 2); cell[f"n_{what}"] = n
                    if what == "open":  # the same answer as the plain matcher's
                        corr = d_corr.cpu().numpy()[:n].copy()
                        r.match_device(d[1].data_ptr(), NS, d[3].data_ptr(), NT, mp, d_corr.data_ptr(), d_d2.data_ptr(), d_cnt.data_ptr())
                        torch.cuda.synchronize()
                        assert d_cnt.cpu().tolist() == [n, 0] and np.array_equal(d_corr.cpu().numpy()[:n], corr)
                row[name] = cell
            out["by_dim"][str(D)] = row
    finally:
        r.close()
    print(json.dumps(out))
    if a.table:
        for rr in rounds:
            print("plain rounds:", rr)
        for D, row in out["by_dim"].items():
            for name in ("plain", "mutual"):
                c = row[name]
                print(f"D {D:>4} {name:>6}: sc_match {c['plain_us']:9.2f} us | guided open {c['guided_open_us']:9.2f} | gate 0.05 random "
                      f"{c['guided_random_us']:9.2f} (tiles kept {row['tiles_kept_random']}) | Morton {c['guided_morton_us']:9.2f} "
                      f"(tiles kept {row['tiles_kept_morton']}) | n {c['n_plain']} / {c['n_open']} / {c['n_random']} / {c['n_morton']}")


if __name__ == "__main__":
    main()
