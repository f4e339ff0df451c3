"""GPU: the streamed joint values.  ancsh_joint_values_rec against its mirror (tests/joint_values_mirror.py, validated on its own in
tests/test_joint_values_cpu.py) inside redzone.guarded() -- the four trees, the eight-part chain and a two-instance library, exact and moved
records, with and without refined poses, behind a 12- and a 20-column articulation block, and the special cases --, then
AncshPipeline(joint_values=True) through posed streams: the block equals pose.joint_values.joint_values_batch on the step's own outputs byte
for byte and everything else equals the same pipeline without the option; with refine=pack_refine(joints=...) the refined groups report the
kept poses and their gap is the joint step's hinge gap; a library under the F16x2 range guard, whose f32 graph carries the block too.

Tolerance of the kernel against the mirror: link, kind, parent_part, q_true and the NaN pattern are exact; every other column lies behind dot
products, a square root and an atan2 whose device and host implementations differ in the last bits, at magnitudes of at most pi: 1e-9
absolute, the bar tests/test_joint_states_gpu.py sets for such columns."""
import numpy as np
import pytest

import joint_step_mirror as JS
import joint_values_mirror as JV
import redzone
import reprojection_mirror as RP
from test_joint_values_cpu import art_block, group, problem, special_cases, tail
from test_refine_joints_cpu import joint_problem, joints_table, kept_gaps, moved_record
from test_reprojection_cpu import object_links, object_mesh4, posed_object
from test_reprojection_gpu import B_, _bytes, _pipe, _stream_batches, _t

pytestmark = pytest.mark.gpu
TOL = 1e-9
EXACT = [0, 1, 2, 3]                                                     # link, kind, parent_part, q_true


def _call(dev, kin, render, scene, rig, norm_factor, record, art, pose=None, refined=None):
    """The entry on host arrays inside a redzone arena -> wide read back; twice, the same bytes."""
    from articulated_pose_amd.pose.joint_values import joint_values_batch
    f = lambda a: None if a is None else _t(np.asarray(a, np.float64), dev)
    first = None
    for _ in range(2):
        with redzone.guarded():
            wide = joint_values_batch(f(kin), f(render), f(scene), f(rig), _t(np.asarray(norm_factor, np.float32), dev), f(record), f(art), pose=f(pose),
                                      refined=f(refined))
            got = wide.cpu().numpy()
        assert first is None or _bytes(got, first)
        first = got
    return got


def _against_the_mirror(dev, label, **args):
    got = _call(dev, **args)
    want = JV.joint_values(**args)
    ld = np.shape(args["art"])[2]
    assert got.shape == want.shape and _bytes(got[:, :, :ld], np.asarray(args["art"], np.float64)), label      # bit for bit, NaN payloads included
    g, w = tail(got), tail(want)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (label, np.argwhere(np.isnan(g) != np.isnan(w))[:8])
    assert np.array_equal(g[:, :, EXACT], w[:, :, EXACT], equal_nan=True), label
    diff = np.nan_to_num(np.abs(g - w), nan=0.0).reshape(-1, 24).max(0)
    print(label, "max |kernel - mirror| per column:", " ".join("%.2g" % d for d in diff))
    assert (diff <= TOL).all(), (label, diff)
    return got


@pytest.mark.parametrize("name", ["K2-revolute-two-link-part", "K3-revolute", "K2-prismatic", "K3-both-two-link-part", "chain", "library"])
def test_kernel_equals_the_mirror(dev, name):
    """Exact and moved records, refined = None and a second moved record with one part's rows NaN, a 12- and a 20-column block."""
    K, kin, ps, render, scene, rigs, nf, rec = problem(name)
    n = len(rec)
    rs = np.random.RandomState(7)
    second = moved_record(rs, rec, 0.02)
    refined = np.concatenate([second.reshape(n, K, 2, 13), rs.normal(size=(n, K, 2, 5))], 3)
    refined[0, K - 1] = np.nan                                           # frame 0: the last part's kept poses (a child everywhere)
    base = dict(kin=kin, render=render, scene=scene, rig=rigs, norm_factor=nf)
    for ld, record, ref in ((12, rec, None), (20, moved_record(rs, rec, 0.02), refined), (12, np.concatenate([rec, rs.normal(size=(n, K, 9))], 2), refined),
                            (20, moved_record(rs, rec, 0.02), None)):
        art = art_block(rs, n, K, ld)
        got = _against_the_mirror(dev, "%s ld=%d refined=%s" % (name, ld, ref is not None), record=record, art=art, pose=ps, refined=ref, **base)
        assert np.isfinite(group(got, 0)).any() and np.isnan(group(got, 2)).all() == (ref is None)
        if ref is not None:
            assert np.isnan(group(got, 2)[0, K - 1]).all() and np.isnan(group(got, 3)[0, K - 1]).all() and np.isfinite(group(got, 3)[1, K - 1]).all()


def test_special_cases_equal_the_mirror(dev):
    for case, (args, check) in special_cases().items():
        got = _against_the_mirror(dev, case, **args)
        assert check(got), (case, tail(got))
    from articulated_pose_amd.pose.joint_values import joint_values_batch
    args = {k: (None if v is None else _t(np.asarray(v, np.float32 if k == "norm_factor" else np.float64), dev)) for k, v in special_cases()["base-row"][0].items()}
    order = ("kin", "render", "scene", "rig", "norm_factor", "record", "art")
    call = lambda **over: joint_values_batch(*[dict(args, **over)[k] for k in order], pose=dict(args, **over)["pose"], refined=dict(args, **over)["refined"])
    assert call().shape == (3, 3, 36)
    for over, what in ((dict(art=args["art"][:, :, :11].contiguous()), "art must be"), (dict(pose=args["pose"][:2].contiguous()), "pose must be"),
                       (dict(refined=args["refined"][..., :17].contiguous()), "refined must be"), (dict(kin=args["kin"][:671].contiguous()), "kin must be"),
                       (dict(rig=args["rig"][:, :-1].contiguous()), "rig must be"), (dict(record=args["record"][:, :, :25].contiguous()), "record must be"),
                       (dict(norm_factor=args["norm_factor"].double()), "norm_factor must be")):
        with pytest.raises(ValueError, match=what):
            call(**over)
    with pytest.raises(RuntimeError):
        call(scene=args["scene"].cpu())


# ---- the streams --------------------------------------------------------------------------------------------------------------------------------
def _eager(dev, kin, rt, sc, rigs, nf, ps, record, art, refined):
    from articulated_pose_amd.pose.joint_values import joint_values_batch
    f = lambda a: None if a is None else _t(np.ascontiguousarray(a, np.float64), dev)
    return joint_values_batch(f(kin), f(rt), f(sc), f(rigs), _t(np.asarray(nf, np.float32), dev), f(record), f(art), pose=f(ps), refined=f(refined)).cpu().numpy()


def _streams(K, dtype, feed, ld, **kw):
    """The pipeline with the option and the same one without -> ([results], the first one's record layout, its step's ABI calls)."""
    from test_fit_quality_gpu import _launch_names
    results, layout, names = [], None, None
    for on in (True, False):
        P = _pipe(K, dtype, joint_values=on, **kw)
        assert P.opts.art_width == ld + (24 if on else 0) and P.opts.joint_values is on
        calls = _launch_names(P.prepare())
        names = names or calls
        assert calls.count("ancsh_joint_values_rec") == int(on) and (not on or calls[-1] == "ancsh_joint_values_rec")
        for sl in P.slots:                                               # the whole batch's block, padding frames included
            assert sl.out["articulation"].shape == (B_, K, ld + (24 if on else 0))
            assert sl.graph32 is None or sl.out32["articulation"].shape == sl.out["articulation"].shape
        results.append(list(P.stream_posed_batches(feed, flags=bool(kw.get("range_guard")), articulation=True)))
        layout = layout or P.record_layout
        del P
    return results, layout, names


def _check_stream(dev, results, layout, batches, kin, K, ld, refined, at=3):
    """Every retired batch: the block equals the eager operator on the step's own outputs byte for byte; its leading columns, the record and every
    other element equal the pipeline built without the option; `at`: the block's place in the result tuple (stream.RESULT_ORDER).  -> the blocks' 24
    columns, one array per batch."""
    got, off = results
    assert len(got) == len(off) == len(batches)
    out = []
    for k, (g, o, (crops, nf, ps, rt, sc, rigs)) in enumerate(zip(got, off, batches)):
        art, rec = g[at], g[2]
        assert len(g) == len(o) and g[:2] == o[:2] and art.shape == (3, K, ld + 24) and o[at].shape == (3, K, ld)
        assert _bytes(art[:, :, :ld], o[at]) and _bytes(rec, o[2]) and all(_bytes(a, b) for i, (a, b) in enumerate(zip(g, o)) if i > 2 and i != at), k
        kept = np.ascontiguousarray(layout.block(rec, "refinement")).reshape(3, K, 2, 18) if refined else None
        want = _eager(dev, kin, rt, sc, rigs, nf, ps, rec[:, :, :26], art[:, :, :ld], kept)
        assert _bytes(art, want), (k, np.argwhere(np.ascontiguousarray(art).view(np.uint64) != want.view(np.uint64))[:8])
        out.append(tail(art))
    return out


def test_posed_stream_equals_the_eager_operator_and_the_plain_pipeline(dev):
    """stream_posed_batches, K = 3, uint16, two slots, three batches of three frames in a batch_size = 4 pipeline (each is padded; the third
    reuses a slot), joint_states=True: a 44-column block.  Without refine= the refined groups are NaN."""
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(41)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=500 + 3 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, layout, names = _streams(K, dtype, feed, 20, render_mesh=mesh, kinematics=kin, joint_states=True)
    blocks = _check_stream(dev, results, layout, batches, kin, K, 20, False)
    for t, (crops, nf, ps, rt, sc, rigs) in zip(blocks, batches):
        assert np.isnan(t[:, :, 14:]).all() and np.isnan(t[:, :2]).all()                # MAPS[3]: link 1 is part 2's, link 3 belongs to no part
        assert (t[:, 2, :3] == [1.0, 1.0, 0.0]).all() and _bytes(t[:, 2, 3], ps[:, 1])
    from articulated_pose_amd.pose.joint_values import joint_value_table
    print("\n".join(joint_value_table([g[3] for g in results[0]], K)))


def test_posed_stream_with_the_joint_step_reports_the_kept_poses(dev):
    """The same stream with refine=joints_table(): the launch comes behind ancsh_refine_rec and reads the slot's kept poses; the refined groups
    are finite wherever the kept poses are, and their gap in the cloud's unit is the hinge gap of the streamed refinement columns."""
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(41)
    kin, _ = posed_object(rs, K, dtype)
    mesh = object_mesh4()
    table = joints_table(iters=2)
    batches = _stream_batches(rs, K, dtype, kin, mesh, dev)
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=500 + 3 * k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, layout, names = _streams(K, dtype, feed, 12, render_mesh=mesh, kinematics=kin, refine=table)
    assert names[-2:] == ["ancsh_refine_rec", "ancsh_joint_values_rec"]
    blocks = _check_stream(dev, results, layout, batches, kin, K, 12, True)
    seen = 0
    for t, g, (crops, nf, ps, rt, sc, rigs) in zip(blocks, results[0], batches):
        columns = np.ascontiguousarray(layout.block(g[2], "refinement"))
        kept = columns.reshape(3, K, 2, 18)[..., :13]
        ok = np.isfinite(kept).all(3)                                    # (frame, part, pose)
        for v in range(2):
            both = ok[:, 2, v] & ok[:, 0, v]                             # the revolute joint: link 1 of part 2 on part 0
            assert np.array_equal(np.isfinite(t[:, 2, 14 + 5 * v:19 + 5 * v]).all(1), both), (v, t[:, 2, 14:], ok)
        # joint_step_mirror.hinge_gaps on the streamed columns (what kept_gaps reads, which takes every frame's joint to be active): a joint is
        # active exactly where the refined group is finite, and there its gap is gap * norm_factor
        rec2 = np.concatenate([kept[:, :, 0], kept[:, :, 1]], 2)
        tables, _ = RP.scene_tables(rt, sc, rigs, nf, rec2, np.zeros((3, 5), np.int32), 0)
        gaps = JS.hinge_gaps(kin, sc, tables, nf, rec2, K)
        mine = np.stack([t[:, 2, 14 + 3], t[:, 2, 19 + 3]], 1) * nf.astype(np.float64)[:, None]
        for f, v in np.ndindex(3, 2):
            assert (1 in gaps[f][v]) == bool(np.isfinite(mine[f, v])), (f, v, gaps[f][v], mine[f, v])
            if 1 in gaps[f][v]:
                seen += 1
                assert abs(mine[f, v] - gaps[f][v][1]) <= TOL, (f, v, mine[f, v], gaps[f][v][1])
    print("streamed frames and poses whose revolute joint has both sides kept:", seen, "of", 6 * len(batches))
    # the same on frames whose fit is known: test_refine_joints_cpu.joint_problem's split record through the eager loop, every joint active
    from articulated_pose_amd.depth import refine_frames
    prob, rec, split = joint_problem(K, dtype)
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = prob
    columns = refine_frames(mesh, render, scene, rigs, nf, split, frames, dtype, joints_table(), device=dev, kinematics=kin)
    wide = _eager(dev, kin, render, scene, rigs, nf, None, split, np.zeros((3, K, 12)), columns.reshape(3, K, 2, 18))
    mine = np.stack([tail(wide)[:, 2, 14 + 3], tail(wide)[:, 2, 19 + 3]], 1) * nf.astype(np.float64)[:, None]
    gaps = kept_gaps(prob, columns, K)
    print("hinge gap of the kept poses:", mine.ravel(), "\njoint_step_mirror.hinge_gaps:", gaps.ravel())
    assert np.isfinite(mine).all() and (np.abs(mine - gaps) <= TOL).all(), (mine, gaps)
    assert np.isnan(tail(wide)[:, :, 3]).all() and np.isnan(tail(wide)[:, :, 5::5]).all()      # no pose table: no q_true, no q_err


def test_library_stream_under_the_range_guard(dev):
    """A two-instance library (two meshes, two kinematic tables with different joint origins), arithmetic f16x2 under the range guard, one cloud
    forced over f16's range by its norm factor: retire() hands out the f32 graph's rows for it -- record and block alike, so the block still
    equals the eager operator on the record that came with it."""
    from articulated_pose_amd.depth import pack_mesh, pack_mesh_library, pose_scene_tables
    K, dtype = 3, "uint16"
    rs = np.random.RandomState(47)
    kin0, _ = posed_object(rs, K, dtype)
    kin1, _ = posed_object(np.random.RandomState(48), K, dtype)
    kin1[:32] = kin0[:32]                                                # one camera
    kins = np.stack([kin0, kin1])
    mesh = object_mesh4()
    lib = pack_mesh_library([mesh, pack_mesh([(0.9 * v, f) for v, f in object_links()])])
    batches = []
    for k, (crops, nf, ps, rt, sc, rigs) in enumerate(_stream_batches(rs, K, dtype, kin0, mesh, dev, nbatches=2)):
        ps[:, 28] = [(k + f) % 2 for f in range(3)]
        rt, sc = pose_scene_tables(kins, ps, dev)
        if k == 1:
            nf = nf.copy()
            nf[1] = 1e6
        batches.append((crops, nf, ps, rt, sc, rigs))
    feed = [(crops, nf, dict(pose=ps, rig=rigs, seed=70 + k), "t%d" % k) for k, (crops, nf, ps, rt, sc, rigs) in enumerate(batches)]
    results, layout, names = _streams(K, dtype, feed, 12, render_mesh=lib, kinematics=kins, arithmetic="f16x2", range_guard=True)
    flags = [np.asarray(g[3]) for g in results[0]]
    print("range flags per batch:", [f.tolist() for f in flags])
    assert flags[1][1] != 0
    blocks = _check_stream(dev, results, layout, batches, kins, K, 12, False, at=4)
    for t, (crops, nf, ps, rt, sc, rigs) in zip(blocks, batches):
        assert (t[:, 2, :3] == [1.0, 1.0, 0.0]).all() and _bytes(t[:, 2, 3], ps[:, 1])
