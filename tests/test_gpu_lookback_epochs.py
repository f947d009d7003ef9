"""GPU: the wrap of the 12-bit look-back epoch (lb_next, sc_capi.hip) through the public API — until now only tools/soak.py got there.

One Registrar, more than 4095 sc_match calls of 700 x 64 descriptors (three finishing tiles, one look-back launch a call) on one
descriptor area, so the epoch runs through 4095, the area is wiped and epoch 1 comes again.  Every call uses one of seven descriptor
sets in mutual or ratio mode, picked by a fixed seeded sequence, and must equal its set's reference: the sets keep different numbers
of matches per tile (tests/test_kernel_probe_ref.py asserts it on match_ref), so a descriptor left from 4095 launches earlier holds a
WRONG prefix — with identical calls it would hold exactly the right one, and a missing wipe would go unseen.  Every 256th call is
followed by a C0 registration, which takes its own look-back launches on the same area and equals the CPU restatement."""
import numpy as np
import pytest

import kernel_probe as kp
import match_ref

pytestmark = pytest.mark.gpu


def test_epochs_wrap_under_changing_calls(pkg, O):
    sets = [kp.epoch_set(s) for s in range(kp.EPOCH_SETS)]
    refs = {(s, m): match_ref.match(*sets[s], **kp.EPOCH_MODES[m]) for s in range(kp.EPOCH_SETS) for m in range(len(kp.EPOCH_MODES))}
    cfg, scene = pkg.synth.make_config_scene("C0")
    assert cfg.n == 500
    ref = O.register(scene.src, scene.tgt, threads=1, **cfg.params())
    r = pkg.Registrar(0)

    def registration(tag):
        got = r.register(scene.src, scene.tgt, flags=pkg.SC_FLAG_EXACT_TOTAL, **cfg.params())
        assert got["status"] == ref["rc"] == 0, tag
        assert got["stats"]["edges"] == ref["edges"] and got["stats"]["tri_total"] == ref["tri_total"], tag
        assert got["stats"]["best_rank"] == ref["best_rank"] and got["stats"]["best_count"] == ref["best_count"], tag
        assert np.array_equal(got["mask"], ref["mask"]), tag
        assert np.array_equal(got["R"].view(np.uint32), ref["R"].view(np.uint32)) and np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), tag

    try:
        registration("first")      # the state area has its final size from here on: no wipe but the wrap's
        seq = kp.epoch_sequence()
        assert len(seq) >= 4300
        for k, (s, m) in enumerate(seq):
            got = r.match(*sets[s], **kp.EPOCH_MODES[m])
            exp_c, exp_d = refs[(int(s), int(m))]
            assert got["n"] == len(exp_c), (k, s, m, got["n"], len(exp_c))
            assert np.array_equal(got["corr"], exp_c), (k, s, m)
            assert got["d2"].view(np.uint32).tobytes() == exp_d.view(np.uint32).tobytes(), (k, s, m)
            if (k + 1) % 256 == 0:
                registration(f"after call {k}")
    finally:
        r.close()
