"""GPU: the row statistics (sc_rows.hip: launch_row_stats, and launch_row_stats_scan with its look-back of two values) on symmetric
bit matrices with zero diagonal and zero pad columns, through tests/native/kernel_probe.hip.  Expected, all from popcounts of the bit
matrix (tests/kernel_probe.py ref_rows): deg, deg+, every wpre word, the cleared rows, rowcost, edge_off, ebase, cost_pre, the pinned
total — and the sentinel in whatever a launch was not given or does not own."""
import numpy as np
import pytest

import kernel_probe as kp
from kernel_probe import u32, u64

pytestmark = pytest.mark.gpu


def _unfused(bits, n, ld, full):
    L = kp.load()
    W = ld // 64
    d_bits = kp.DevBuf.of(bits)
    o = dict(deg=kp.DevBuf(n * 4), degp=kp.DevBuf(n * 4), wpre=kp.DevBuf(n * W * 4), zero=kp.DevBuf(n * W * 8), rowcost=kp.DevBuf(n * 4))
    rc = L.kp_row_stats(d_bits.ptr, n, ld, o["deg"].ptr, o["degp"].ptr, o["wpre"].ptr, o["zero"].ptr if full else None,
                        o["rowcost"].ptr if full else None, kp.stream())
    assert rc == 0
    kp.sync()
    assert d_bits.guard_ok() and all(b.guard_ok() for b in o.values())
    assert np.array_equal(d_bits.read(u64).reshape(n, W), bits)
    return dict(deg=o["deg"].read(u32), degp=o["degp"].read(u32), wpre=o["wpre"].read(u32).reshape(n, W), zero=o["zero"].read(u64),
                rowcost=o["rowcost"].read(u32))


def _fused(bits, n, ld, full, lb, epoch):
    L = kp.load()
    W = ld // 64
    d_bits = kp.DevBuf.of(bits)
    o = dict(deg=kp.DevBuf(n * 4), degp=kp.DevBuf(n * 4), wpre=kp.DevBuf(n * W * 4), zero=kp.DevBuf(n * W * 8), edge_off=kp.DevBuf((n + 1) * 8),
             ebase=kp.DevBuf(n * 4), cost_pre=kp.DevBuf((n + 1) * 8))
    host = kp.Pinned()
    rc = L.kp_row_stats_scan(d_bits.ptr, n, ld, o["deg"].ptr, o["degp"].ptr, o["wpre"].ptr, o["zero"].ptr if full else None, o["edge_off"].ptr,
                             o["ebase"].ptr, o["cost_pre"].ptr if full else None, lb.ticket, lb.err, lb.desc.ptr, lb.desc.nbytes, epoch, host.ptr,
                             kp.stream())
    assert rc == 0
    kp.sync()
    assert d_bits.guard_ok() and all(b.guard_ok() for b in o.values()) and lb.clean()
    return dict(deg=o["deg"].read(u32), degp=o["degp"].read(u32), wpre=o["wpre"].read(u32).reshape(n, W), zero=o["zero"].read(u64),
                edge_off=o["edge_off"].read(u64), ebase=o["ebase"].read(u32), cost_pre=o["cost_pre"].read(u64), host=host.get())


@pytest.mark.parametrize("n", kp.ROWS_N)
def test_row_statistics(n):
    L = kp.load()
    lb = kp.LbState(L.kp_row_stats_scan_state_bytes(n))      # one state area for every launch of this test: an epoch each
    assert lb.desc.nbytes == 2 * 8 * ((n + kp.RS_ROWS - 1) // kp.RS_ROWS)
    epoch = 0
    for density in kp.ROWS_DENSITIES:
        bits, ld = kp.bit_matrix(n, density, seed=n)
        ref = kp.ref_rows(bits, n, ld)
        tag = (n, density)
        print(tag, "edges", ref["total"], "largest row cost", int(ref["cost"].max()))
        assert int(ref["cost"].max()) < 2 ** 32, "no legal size saturates rowcost"
        if density == "full":
            assert (ref["deg"] == n - 1).all()
        unf = None
        for full in (True, False):
            got = _unfused(bits, n, ld, full)
            for name in ("deg", "degp", "wpre"):
                assert np.array_equal(got[name], ref[name]), (tag, name, full)
            if full:
                assert not got["zero"].any() and np.array_equal(got["rowcost"], ref["rowcost"]), tag
                unf = got
            else:
                assert (got["zero"] == u64(kp.SENT64)).all() and (got["rowcost"] == u32(kp.SENT32)).all(), tag
        for full in (True, False):
            epoch += 1
            got = _fused(bits, n, ld, full, lb, epoch)
            for name in ("deg", "degp", "wpre", "edge_off", "ebase"):
                assert np.array_equal(got[name], ref[name]), (tag, name, full)
            assert got["host"] == ref["total"] == int(got["edge_off"][n]), tag
            if full:
                assert not got["zero"].any(), tag
                assert np.array_equal(got["cost_pre"], ref["cost_pre"]), tag
                assert np.array_equal(got["cost_pre"], kp.ref_scan(unf["rowcost"])), (tag, "fused cost_pre != scan of the unfused rowcost")
            else:
                assert (got["zero"] == u64(kp.SENT64)).all() and (got["cost_pre"] == u64(kp.SENT64)).all(), tag
