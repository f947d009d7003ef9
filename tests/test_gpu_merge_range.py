"""GPU: sc_merge_poses (frame and batch forms) at the ends of the fp32 range, past one pass of the overlap launch's word loop and
across the decide launch's rounds.

tests/test_gpu_merge_frame.py and test_gpu_merge_batch.py run the entry on unit-scale scenes of at most 1500 correspondences and on
K = 1, 2, 4, 8, 33, 64 and 1024 poses.  Here the frames are those of tests/test_gpu_pose_frame_range.py — test_range_oracle.scene_small
times 2^k, far from the origin, with rows at +-3e38, tau at the ends of its range, the truncated score modes, scene_big at k = 62 and
-56 —, the batch problems those of tests/test_gpu_pose_batch_range.py; the shape cases hold 2048, 2049 and 2113 correspondences
(merge_overlap_kernel streams 32 words of a bit row at a time: a second pass, its partial last chunk, the accumulators carried across
the barrier pair), and the decide lists hold K = 65, 127, 128, 129 and 130 poses on a frame of 129 — a later round that is partial,
ties in strength across the round boundary, and a min_count above every count.

tests/test_settle_merge_range_ref.py owns the cases and the expected values (tests/merge_ref.py) and asserts on the reference alone
that the cases are what they are used for.  Every comparison is bit for bit: the 64 bytes of every record, every parent, every cell
of the overlap table, both count words.  No tolerances.  Every call runs in its host form and in its device form; the two must agree
byte for byte.
"""
import numpy as np
import pytest

import batch_ref
import test_batch_range_ref as R
import test_pose_range_ref as P
import test_settle_merge_range_ref as S
from conftest import nan_equal_bits
from test_gpu_merge_batch import _assert_batch
from test_gpu_merge_frame import _assert_same, _device
from test_gpu_pose_frame_range import _frame
from test_range_oracle import pow2

pytestmark = pytest.mark.gpu

SC_OK, SC_EINVAL, SC_ENOHYP = 0, -1, -5
_GPU = {}  # (name, list) -> {(rule, compact): the GPU's own result}: what the metamorphic check compares


def _key(rule, compact):
    return tuple(sorted(rule.items())), compact


def _pose_args(pkg, rt, st):
    """a list as the call takes it: bare floats at stride 48, or records of 64 bytes under the status flag"""
    return (rt, 48, 0) if st is None else (P.records64(rt, st), 64, pkg.SC_MERGE_STATUS)


def _merge(pkg, reg, rt, st, n, exp, rule, compact, masked, what, bare=False):
    """one sc_merge_poses_frame call, host form then device form, against the reference -> the host form's result"""
    pose, stride, flags = _pose_args(pkg, rt, st)
    flags |= pkg.SC_MERGE_COMPACT if compact else 0
    sel_mode, sel = (pkg.SC_ASSIGN_SEL_MASK, P.third_off(n)) if masked else (pkg.SC_ASSIGN_SEL_NONE, None)
    got = reg.merge_poses_frame(pose, sel_mode=sel_mode, sel=sel, flags=flags, **rule)
    _assert_same(got, exp, what)
    mp = pkg.make_merge_params(sel_mode=sel_mode, flags=flags, **rule)
    _assert_same(_device(pkg, reg, mp, pose.tobytes(), stride, len(pose), sel), got, what + " device form")
    if bare:                                                             # d_overlap and d_count NULL: the same records and parents
        dev = _device(pkg, reg, mp, pose.tobytes(), stride, len(pose), sel, want_overlap=False, want_count=False)
        assert dev[2] is None and dev[3] is None and dev[0].tobytes() == got[0].tobytes() and np.array_equal(dev[1], got[1]), what
    return got


def _run(pkg, O, reg, name, which):
    """one list of one frame -> what the metamorphic check keeps of it (None: the case leaves no frame)"""
    if not _frame(pkg, O, reg, name):
        assert name in S.NO_FRAME
        rt, st = P.frame_poses(pkg, O, name)
        with pytest.raises(pkg.SacCotError) as e:
            reg.merge_poses_frame(rt[:1])
        assert e.value.status == SC_EINVAL and "no frame" in str(e.value), name
        return None
    assert name not in S.NO_FRAME
    n = len(P.frame_case(pkg, O, name)[0])
    rt, st = S.frame_lists(pkg, O, name)[which]
    keep = {}
    for rule in S.MERGE_RULES:
        for compact in (False, True):
            exp = S.merge_ref(pkg, O, name, which, rule, compact)
            keep[_key(rule, compact)] = _merge(pkg, reg, rt, st, n, exp, rule, compact, False, f"{name} merge {which} {rule} compact={compact}")
    _merge(pkg, reg, rt, st, n, S.merge_ref(pkg, O, name, which, masked=True), S.PLAIN, False, True, f"{name} merge {which} mask", bare=True)
    return keep


CASES = [(name, which) for name in S.FRAME_CASES for which in S.merge_lists(name)]


@pytest.mark.parametrize("name,which", CASES)
def test_merge_equals_its_reference_at_the_ends_of_the_range(pkg, O, reg, name, which):
    keep = _run(pkg, O, reg, name, which)
    assert (keep is None) == (name in S.NO_FRAME)
    if keep is None:
        return                                                           # (only the cases test_pose_range_ref.NO_FRAME names come here)
    _GPU[name, which] = keep
    if P.frame_in_window(name) and which == "K65":                       # the case is not trivial on the GPU either
        rec, parent, x, count = keep[_key(S.PLAIN, False)]
        assert count.tolist() == [14, 61] and parent[5] == parent[1] != 5 and int(rec["count"].max()) >= 100


def _shape_frame(pkg, O, reg, n):
    sc = S.shape_scene(pkg, n)
    kw, frame = S.shape_frame(pkg, O, n)
    f = reg.register(sc.src, sc.tgt, params=pkg.make_params(**kw, flags=pkg.SC_FLAG_EXACT_TOTAL))
    assert f["status"] == frame["rc"] == SC_OK and np.array_equal(f["mask"], frame["mask"])
    assert nan_equal_bits(f["R"], frame["R"]) and nan_equal_bits(f["t"], frame["t"])


@pytest.mark.parametrize("n", S.SHAPE_NS)
def test_merge_past_one_pass_of_the_overlap_word_loop(pkg, O, reg, n):
    """n = 2049: the second pass holds one word (and 31 past the row's end); n = 2113: two words, 65 rows, and what they add is in
    the table.  K = 33: three tiles of the overlap launch, one of them off the diagonal."""
    _shape_frame(pkg, O, reg, n)
    poses = S.shape_poses(pkg, n, S.SHAPE_K_MERGE)
    for rule in S.MERGE_RULES:
        for compact in (False, True):
            exp = S.shape_merge_ref(pkg, O, n, rule, compact)
            got = _merge(pkg, reg, poses, None, n, exp, rule, compact, False, f"n={n} {rule} compact={compact}", bare=n == S.SHAPE_NS[-1])
    assert S.shape_merge_ref(pkg, O, n)[3].tolist() == [6, S.SHAPE_K_MERGE] and int(got[2].max()) >= 100


@pytest.mark.parametrize("K", S.DECIDE_KS)
def test_merge_across_the_rounds_of_the_decide_launch(pkg, O, reg, K):
    """K = 65: round two holds one rank; 127 / 128 / 129: the end of round two, a third round of one rank; 130 with 72 copies of
    the strongest pose: ties across rank 63 | 64 go to the lowest pose number; min_count above every count: nothing is kept"""
    _shape_frame(pkg, O, reg, S.DECIDE_N)
    poses = S.decide_poses(pkg, O, K)
    for rule in S.MERGE_RULES + [S.nothing_kept_rule(pkg, O, K)]:
        for compact in (False, True):
            exp = S.decide_ref(pkg, O, K, rule, compact)
            got = _merge(pkg, reg, poses, None, S.DECIDE_N, exp, rule, compact, False, f"K={K} {rule} compact={compact}")
    assert got[3].tolist() == [0, K] and (got[1] == -1).all() and np.array_equal(got[0]["count"], S.decide_ref(pkg, O, K)[0]["count"])
    if K == S.TIE_K:
        rec, parent, x, count = reg.merge_poses_frame(poses)
        tied = sorted(S.TIE_BELOW + (S.TIE_AT,) + S.TIE_ABOVE)
        assert (parent[tied] == tied[0]).all() and rec[tied[0]]["status"] == SC_OK


@pytest.mark.parametrize("gid", list(S.BATCH_LAUNCHES))
def test_the_batch_form_equals_its_reference_at_the_ends_of_the_range(pkg, O, reg, gid):
    kw, names = S.BATCH_LAUNCHES[gid]
    for K in S.MERGE_BATCH_KS:
        _, problems, rt, st = S.batch_input(pkg, O, gid, K)
        assert len(problems) <= 40 and max(len(s) for s, _ in problems) <= 512
        pose = np.frombuffer(bytes([0xA5]) * (80 * K * len(names)), batch_ref.RESULT_DTYPE).copy().reshape(K, len(names))   # motion-major
        pose["Rt"], pose["status"] = rt, st
        off = np.concatenate([[0], np.cumsum([len(s) for s, _ in problems])]).astype(np.uint32)
        src, tgt = np.concatenate([s for s, _ in problems]), np.concatenate([t for _, t in problems])
        for rule in S.MERGE_BATCH_RULES:
            for compact in (False, True):
                exp = S.merge_batch_ref(pkg, O, gid, K, rule, compact)
                flags = pkg.SC_MERGE_COMPACT if compact else 0
                for soa in (False, True):
                    a, b = (np.ascontiguousarray(src.T), np.ascontiguousarray(tgt.T)) if soa else (src, tgt)
                    p = pkg.make_params(**kw, layout=pkg.SC_SOA if soa else pkg.SC_AOS)
                    got = reg.merge_poses_batch(a, b, off, p, pose, flags=flags, **rule)
                    _assert_batch(got, exp, f"{gid} K={K} {rule} compact={compact} soa={soa}")
                if K == 16:                                              # the device form at stride 80: the same bytes
                    import torch
                    d_src, d_tgt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
                    d_pose = torch.from_numpy(pose.view(np.uint8).reshape(-1).copy()).cuda()
                    d_out = torch.full((K * len(names) * 64,), 0xAB, dtype=torch.uint8, device="cuda")
                    d_parent = torch.full((K * len(names),), 0x2B2B2B2B, dtype=torch.int32, device="cuda")
                    d_count = torch.full((2 * len(names),), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    reg.merge_poses_batch_device(d_src.data_ptr(), d_tgt.data_ptr(), off, pkg.make_params(**kw), pkg.make_merge_params(flags=flags, **rule),
                                                 d_pose.data_ptr(), 80, K, d_out.data_ptr(), d_parent.data_ptr(), d_count.data_ptr())
                    torch.cuda.synchronize()
                    assert d_out.cpu().numpy().tobytes() == exp[0].tobytes() and d_parent.cpu().numpy().tobytes() == exp[1].tobytes(), (gid, rule, compact)
                    assert d_count.cpu().numpy().view(np.uint32).tobytes() == exp[2].tobytes(), (gid, rule, compact)


def test_inside_the_window_the_gpu_equals_itself_at_unit_scale(pkg, O, reg):
    """Without the reference: at the k of test_batch_range_ref.polish_metamorphic_ks every record's status, index, count and score,
    the parents, the overlap table, the count words and R's bits are those at k = 0, and t is multiplied by 2^k exactly
    (tests/test_settle_merge_range_ref.py: the reference is covariant on these lists at these k)."""
    def gpu(k, which):
        name = f"a:{k}"
        if (name, which) not in _GPU:
            _GPU[name, which] = _run(pkg, O, reg, name, which)
        return _GPU[name, which]
    ks = R.polish_metamorphic_ks()
    assert len(ks) >= 3
    for which in S.MERGE_LISTS:
        g0 = gpu(0, which)
        for k in ks:
            g = gpu(k, which)
            for rule in S.MERGE_RULES:
                for compact in (False, True):
                    m, m0 = g[_key(rule, compact)], g0[_key(rule, compact)]
                    S.assert_merge_covariant(m, m0, pow2(k), S.scaling_rows(which, len(m[0])), compact, (k, which, rule, compact))
        assert int(g0[_key(S.PLAIN, False)][0]["count"].max()) >= 100
