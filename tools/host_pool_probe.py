#!/usr/bin/env python3
"""What the host forms hold and what they cost when one context interleaves them: the sequence of
tests/test_gpu_host_pool.py on ONE context, twice.

  python tools/host_pool_probe.py [--lib PATH] [--repeats 20] [--table]

Per step: workspace_bytes behind the step in pass 1 and in pass 2 (read through an sc_register call of the frame's scene, with
no_fast = 1, as the tests read it; the frame's own workspace is warmed first, so what moves is the host forms'), and — in pass 2,
when every buffer has its size — the median wall time of the host-form call over --repeats calls, copies and the wait for the
stream included.  --lib: a libsaccot.so of the same ABI to measure in place of this tree's (one built from the parent commit).
Prints one JSON line; --table also prints the rows as text.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="measure this libsaccot.so (same ABI) and not the tree's")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package()
    if a.lib:
        pkg.api.LIB_PATH = os.path.abspath(a.lib)  # (before the first load)
    from test_gpu_host_pool import _steps
    steps = _steps(pkg)
    frame = next(s for s in steps if s.name == "a frame")
    r = pkg.Registrar(0)
    rows = []
    try:
        r.set_debug(no_fast=1)
        base = [frame.call(r)["stats"]["workspace_bytes"] for _ in range(4)][-1]
        for n_pass in (1, 2):
            for i, s in enumerate(steps):  # (a frame step finds the frame of the read of workspace_bytes before it: the same scene)
                us = None
                if n_pass == 2 and s is not frame:
                    t = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        s.call(r)
                        t.append((time.perf_counter() - t0) * 1e6)
                    us = round(float(np.median(t)), 1)
                else:
                    s.call(r)
                held = frame.call(r)["stats"]["workspace_bytes"]
                if n_pass == 1:
                    rows.append(dict(step=s.name, held_pass1=held - base))
                else:
                    rows[i].update(held_pass2=held - base, median_us=us)
    finally:
        r.close()
    if a.table:
        print(f"{'step':52} {'pass 1':>10} {'pass 2':>10} {'median us':>10}   (bytes held beyond the frame's own {base})")
        for row in rows:
            print(f"{row['step']:52} {row['held_pass1']:10d} {row['held_pass2']:10d} {'' if row['median_us'] is None else row['median_us']:>10}")
    print(json.dumps(dict(lib=a.lib or "tree", frame_bytes=base, repeats=a.repeats, rows=rows)))


if __name__ == "__main__":
    main()
