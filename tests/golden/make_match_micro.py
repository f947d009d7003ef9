"""Generator of match_micro.npz: one 64 x 80 x 33 matching problem with planted ties, and what the restatement
(tests/match_ref.py) returns for it in every mode.  Run from the repository root:  python tests/golden/make_match_micro.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import match_ref  # noqa: E402
import __graft_entry__ as ge  # noqa: E402

MODES = {"k1": dict(knn=1), "k4": dict(knn=4), "mutual": dict(knn=1, mutual=True), "ratio": dict(knn=1, ratio=0.8),
         "both": dict(knn=1, mutual=True, ratio=0.9)}


def inputs():
    S = ge.load_package().synth
    ns, nt, D, seed = 64, 80, 33, 4242
    a = S.gauss(seed, 1, np.arange(ns * D, dtype=np.uint64).reshape(ns, D)).astype(np.float32)
    b = S.gauss(seed, 2, np.arange(nt * D, dtype=np.uint64).reshape(nt, D)).astype(np.float32)
    noise = S.gauss(seed, 3, np.arange(ns * D, dtype=np.uint64).reshape(ns, D)).astype(np.float32)
    for i in range(0, 40):                      # counterparts: source row i near target row 79 - i (half of them very near)
        b[79 - i] = a[i] + noise[i] * np.float32(0.05 if i % 2 else 0.6)
    b[3] = b[70]; b[11] = b[70]                 # one target row three times: ties go to the lowest index
    a[50] = a[9]; a[51] = a[9]                  # one source row three times: a mutual pair keeps only the first
    b[20] = a[60]                               # an exact match, distance 0
    return a, b


def build():
    a, b = inputs()
    out = dict(fsrc=a, ftgt=b)
    for name, kw in MODES.items():
        corr, d2 = match_ref.match(a, b, **kw)
        out["corr_" + name] = corr
        out["d2_" + name] = d2
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "match_micro.npz"), **build())
    print("wrote", os.path.join(HERE, "match_micro.npz"))
