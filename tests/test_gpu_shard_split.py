"""GPU: where launch_shard_split (sc_rows.hip) puts the cuts, for every rank of world 1, 2, 3, 8 and 64, on synthetic cost prefixes,
through tests/native/kernel_probe.hip.  Expected: boundary l is np.searchsorted(cost_pre, total * l // world, "left") with Python
integers, own_edge the edge_off of those rows, and a world's ranges tile [0, n).  (Any split that tiles the rows passes the "sharded
equals unsharded" tests of the registrations; only this pins the cuts.)"""
import numpy as np
import pytest

import kernel_probe as kp
from kernel_probe import u32, u64

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", kp.SPLIT_N)
@pytest.mark.parametrize("shape", kp.SPLIT_SHAPES)
def test_shard_split_cuts(n, shape):
    L = kp.load()
    cost = kp.split_costs(shape, n, seed=n)
    cost_pre = np.concatenate([[0], np.cumsum(cost, dtype=u64)]).astype(u64)
    edge_off = np.concatenate([[0], np.cumsum(kp.rng(n).integers(0, 50, n), dtype=u64)]).astype(u64)
    jobs = [(rank, world) for world in kp.SPLIT_WORLDS for rank in range(world)]
    d_cost, d_edge = kp.DevBuf.of(cost_pre), kp.DevBuf.of(edge_off)
    d_row, d_own = kp.DevBuf(len(jobs) * 8), kp.DevBuf(len(jobs) * 16)
    for k, (rank, world) in enumerate(jobs):
        assert L.kp_shard_split(d_cost.ptr, d_edge.ptr, n, rank, world, d_row.ptr + 8 * k, d_own.ptr + 16 * k, kp.stream()) == 0
    kp.sync()
    rows, edges = d_row.read(u32).reshape(-1, 2), d_own.read(u64).reshape(-1, 2)
    assert all(b.guard_ok() for b in (d_cost, d_edge, d_row, d_own))
    assert np.array_equal(d_cost.read(u64), cost_pre) and np.array_equal(d_edge.read(u64), edge_off)
    for k, (rank, world) in enumerate(jobs):
        exp_rows, exp_edges = kp.ref_split(cost_pre, edge_off, n, rank, world)
        assert rows[k].tolist() == exp_rows and edges[k].tolist() == exp_edges, (shape, n, rank, world, rows[k], exp_rows)
    for world in kp.SPLIT_WORLDS:     # the world's ranges tile [0, n)
        r = np.array([rows[k] for k, (rank, w) in enumerate(jobs) if w == world])
        assert r[0, 0] == 0 and r[-1, 1] == n and (r[1:, 0] == r[:-1, 1]).all() and (r[:, 0] <= r[:, 1]).all(), (shape, n, world)
    print(shape, n, "world 8 rows", [rows[k].tolist() for k, (rank, w) in enumerate(jobs) if w == 8])
