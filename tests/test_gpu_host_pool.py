"""GPU: the host forms' shared staging pool (sc_ctx.hpp, HostArrays).

Every host form stages its k-th array in slot k of one pool, so on a context that interleaves them every slot shrinks, grows and
changes owner.  One context A runs sixteen host forms in a row, twice; every call is repeated on a fresh Registrar of its own, and A's
outputs are compared with the fresh context's by the assertions of the entry's own test file — its `_assert_*` helper, bit for bit
on the fields that helper reads (what the header leaves unspecified, such as the slot entries past a problem's count, is excluded
exactly as there).  Both passes on A are held against the same fresh outputs, so pass 2 equals pass 1 on those fields.
"""
import numpy as np
import pytest

import assign_ref as AR
import cycles_ref as CR
import match_batch_ref as M
import test_gpu_assign_batch as T_ASG_B
import test_gpu_assign_frame as T_ASG_F
import test_gpu_batch as T_BATCH
import test_gpu_instances_batch as T_INST
import test_gpu_match_batch as T_MATCH
import test_gpu_merge_batch as T_MRG_B
import test_gpu_merge_frame as T_MRG_F
import test_gpu_pairs_cycles as T_CYC
import test_gpu_polish_batch as T_POL_B
import test_gpu_polish_poses as T_PPOSE
import test_gpu_pose_info as T_INFO_B
import test_gpu_pose_info_frame as T_INFO_F
import test_gpu_settle_batch as T_STL_B
import test_gpu_settle_frame as T_STL_F

pytestmark = pytest.mark.gpu

SC_OK, SC_ENOMEM = 0, -2
N_FRAME = 1000  # not a multiple of 64


def _split(a, off):
    """a packed per-correspondence array as the references give it: one array per problem"""
    return [a[int(off[b]): int(off[b + 1])] for b in range(len(off) - 1)]


def _records(pkg, scenes):
    """sc_register_batch-shaped input records: every problem's own motion, SC_OK"""
    rec = np.zeros(len(scenes), pkg.BATCH_RESULT_DTYPE)
    for b, s in enumerate(scenes):
        rec["Rt"][b] = AR.rt_of(s.R_gt, s.t_gt)
        rec["n"][b] = len(s.src)
    return rec


class Step:
    """call(reg) -> the outputs on `reg`; ref (default: call) -> what a fresh context is asked for; check(got, fresh) -> the entry's
    own assertions; frame: the call needs the scored frame of step 11"""
    def __init__(self, name, call, check, ref=None, frame=False):
        self.name, self.call, self.check, self.ref, self.frame = name, call, check, ref or call, frame


def _steps(pkg):
    p = T_STL_B._params(pkg)
    P1 = T_STL_B._scenes(pkg)                                                       # 3, 64, 65 and 512 correspondences
    P2 = [pkg.synth.make_scene(64, .4, 1.0, AR.TAU, 7700 + i) for i in range(2)]    # two problems of 64
    s1, t1, o1 = T_STL_B._pack(P1)
    s2, t2, o2 = T_STL_B._pack(P2)
    pose_stl, pose_mrg, pose_asg = T_STL_B._poses(pkg, P2, 2), T_MRG_B._poses(pkg, P1, 16), T_ASG_B._poses(pkg, P1, 2)
    rec1, rec2 = _records(pkg, P1), _records(pkg, P2)
    feats = M.feature_scenes()[:2]                                                  # the two smallest tables
    fp = pkg.make_params(**M.KW)
    k24 = CR.k24()
    cp = T_CYC._params(pkg, k24)
    sc = AR.scene(pkg, N_FRAME)
    gt = AR.rt_of(sc.R_gt, sc.t_gt)
    fparams = T_ASG_F._params(pkg)
    many, two = AR.many(gt, 64, 200 + N_FRAME), AR.perturbed(gt, 2, 100 + N_FRAME, 1e-2, 2e-2)
    sel = (np.arange(N_FRAME) % 3 != 0).astype(np.uint8)
    pq = pkg.make_polish_params(candidates=1, max_iter=16)

    def features_exp(fresh):
        return [dict(g, rec=dict({f: g["stats"][f] for f in T_MATCH.FIELDS[1:]}, status=g["status"],
                                 Rt=np.concatenate([g["R"].ravel(), g["t"]]))) for g in fresh]

    def frame_check(got, fresh):
        assert got["status"] == fresh["status"] == SC_OK
        assert got["R"].tobytes() == fresh["R"].tobytes() and got["t"].tobytes() == fresh["t"].tobytes()
        assert np.array_equal(got["mask"], fresh["mask"])

    return [
        Step("sc_register_batch(P1)", lambda r: r.register_batch_raw(s1, t1, o1, p),
             lambda g, f: T_BATCH._assert_batch((g[0], g[1], o1), (f[0], _split(f[1], o1)), "register_batch")),
        Step("sc_settle_poses_batch(P2, K = 2)", lambda r: r.settle_poses_batch(s2, t2, o2, p, pose_stl),
             lambda g, f: T_STL_B._assert_batch(g, (f[0], _split(f[1], o2), f[2]), o2, "settle_batch")),
        Step("sc_merge_poses_batch(P1, K = 16)", lambda r: r.merge_poses_batch(s1, t1, o1, p, pose_mrg),
             lambda g, f: T_MRG_B._assert_batch(g, f, "merge_batch")),
        Step("sc_register_instances_batch(P2)", lambda r: r.register_instances_batch_raw(s2, t2, o2, p, 4, 4),
             lambda g, f: T_INST._assert_batch(g + (o2,), (f[0], _split(f[1], o2), f[2]), "instances_batch")),
        Step("sc_polish_batch(P1)", lambda r: r.polish_batch_raw(s1, t1, o1, p, pq, rec1),
             lambda g, f: T_POL_B._assert_polish(g[0], g[1], o1, (f[0], _split(f[1], o1)), "polish_batch")),
        Step("sc_pose_info_batch(P2)", lambda r: r.pose_info_batch_raw(s2, t2, o2, p, rec2),
             lambda g, f: T_INFO_B._assert_info(g, f, "pose_info_batch")),
        Step("sc_assign_poses_batch(P1)", lambda r: r.assign_poses_batch(s1, t1, o1, p, pose_asg),
             lambda g, f: T_ASG_B._assert_batch(g, (_split(f[0], o1), f[1]), o1, "assign_batch")),
        Step("sc_match_batch", lambda r: r.match_batch([(a[1], a[3]) for a in feats], knn=1),
             lambda g, f: T_MATCH._assert_match(g, [(x["corr"], x["d2"], x["n"], int(x["nonfinite"])) for x in f], "match_batch")),
        Step("sc_register_batch_features", lambda r: r.register_batch_features([a[:4] for a in feats], params=fp, knn=1, mutual=True),
             lambda g, f: T_MATCH._assert_features(g, features_exp(f), "register_batch_features")),
        Step("sc_pairs_cycles", lambda r: r.pairs_cycles(k24.n_sets, k24.pairs, k24.rt, cp),
             lambda g, f: T_CYC._assert_same(g, f, "pairs_cycles")),
        Step("a frame", lambda r: r.register(sc.src, sc.tgt, params=fparams), frame_check),
        Step("sc_assign_poses_frame(K = 64)", lambda r: r.assign_poses_frame(many),
             lambda g, f: T_ASG_F._assert_same(g, f, "assign_frame"), frame=True),
        Step("sc_assign_poses_frame(K = 64), no d2", lambda r: r.assign_poses_frame(many, want_d2=False),
             lambda g, f: T_ASG_F._assert_same(g, f, "assign_frame, no d2"), ref=lambda r: r.assign_poses_frame(many), frame=True),
        Step("sc_settle_poses_frame(K = 2), a mask", lambda r: r.settle_poses_frame(two, sel_mode=pkg.SC_ASSIGN_SEL_MASK, sel=sel),
             lambda g, f: T_STL_F._assert_same(g, f, "settle_frame, a mask"), frame=True),
        Step("sc_settle_poses_frame(K = 2), no d2, no rounds", lambda r: r.settle_poses_frame(two, want_d2=False, want_rounds=False),
             lambda g, f: T_STL_F._assert_same(g, f, "settle_frame, bare"), ref=lambda r: r.settle_poses_frame(two), frame=True),
        Step("sc_merge_poses_frame(K = 64)", lambda r: r.merge_poses_frame(many),
             lambda g, f: T_MRG_F._assert_same(g, f, "merge_frame"), frame=True),
        Step("sc_merge_poses_frame(K = 64), no overlap", lambda r: r.merge_poses_frame(many, want_overlap=False),
             lambda g, f: T_MRG_F._assert_same(g, f, "merge_frame, no overlap"), ref=lambda r: r.merge_poses_frame(many), frame=True),
        Step("sc_polish_poses(K = 2)", lambda r: r.polish_poses(two),
             lambda g, f: T_PPOSE._assert_pol(g, f, "polish_poses"), frame=True),
        Step("sc_pose_info_frame(K = 64)", lambda r: r.pose_info_frame(many),
             lambda g, f: T_INFO_F._assert_info(g, f, "pose_info_frame"), frame=True),
    ]


def _fresh(pkg, steps):
    """every step's outputs on a Registrar of its own (a frame step: behind the frame of step 11 on that Registrar)"""
    frame = next(s for s in steps if s.name == "a frame")
    out = {}
    for s in steps:
        r = pkg.Registrar(0)
        try:
            if s.frame:
                assert frame.call(r)["status"] == SC_OK
            out[s.name] = s.ref(r)
        finally:
            r.close()
    return out


def test_interleaved_host_forms_equal_fresh_contexts_and_hold_no_more_the_second_time(pkg):
    steps = _steps(pkg)
    fresh = _fresh(pkg, steps)
    frame = next(s for s in steps if s.name == "a frame")
    a = pkg.Registrar(0)
    try:
        a.set_debug(no_fast=1)  # (the same input takes the same path every time: what moves afterwards is the host forms')
        for _ in range(4):
            frame.call(a)       # the frame's own workspace has settled
        held = []
        for n_pass in (1, 2):
            for s in steps:
                print("pass", n_pass, s.name)
                s.check(s.call(a), fresh[s.name])
            held.append(frame.call(a)["stats"]["workspace_bytes"])
        print("workspace_bytes after pass 1 and pass 2", held)
        assert held[0] == held[1] > 0  # a repeated sequence allocates nothing
    finally:
        a.close()


def test_a_cap_that_admits_the_warm_pool_but_not_the_offsets_is_enomem_and_the_context_stays_usable(pkg):
    """sc_assign_poses_batch on a context whose pool other host forms have warmed — sc_register_batch slots 0 - 3, sc_settle_poses_batch
    0 - 2, 4, 5 and 7, sc_match_batch 6: every slot its five arrays take (0, 1, 2, 4, 6) holds 64 KiB at least, more than they need —
    but whose asg_off does not exist yet.  With max_workspace = 1 no slot has to grow, so what is refused is the entry's own buffer.
    (SC_ENOMEM is all that can be seen from here: that the refusal comes from the `also` room of HostArrays::run, in front of the
    first copy, is the code's order, not something this test observes.)"""
    steps = {s.name: s for s in _steps(pkg)}
    asg = steps["sc_assign_poses_batch(P1)"]
    fresh = _fresh(pkg, [steps["a frame"], asg])
    P1 = T_STL_B._scenes(pkg)
    s1, t1, o1 = T_STL_B._pack(P1)
    pose = T_ASG_B._poses(pkg, P1, 2)
    a = pkg.Registrar(0)
    try:
        for name in ("sc_register_batch(P1)", "sc_settle_poses_batch(P2, K = 2)", "sc_match_batch"):
            steps[name].call(a)
        with pytest.raises(pkg.SacCotError) as e:
            a.assign_poses_batch(s1, t1, o1, T_STL_B._params(pkg, max_workspace=1), pose)
        print(e.value)
        assert e.value.status == SC_ENOMEM
        asg.check(asg.call(a), fresh[asg.name])  # the same call under the default cap
    finally:
        a.close()
