"""GPU: out-of-bounds evidence for the whole C ABI (VERDICT r04 "what's weak" 9).  Every output, scratch and slot buffer the host layer
allocates -- with torch.empty, zeros, ones, full or one of their *_like forms: the calls tests/redzone.py intercepts -- is carved out of a
sentinel-guarded allocation (4 KB of 0xA5 before and after) while the existing parity checks run: the operators on their seeded random
shapes, the conv / chain / fused-SA entry points on ragged row counts, the whole forward of both networks, the pose fit on ragged and
empty parts, the metric / input / loss kernels; every render-and-compare entry on crops of odd sizes that end at the pixel capacity, the
refine loop as a whole, the joint states, and the streamed step of AncshPipeline per input kind with every slot buffer guarded.  A write
past any buffer fails the test.  An `empty` body is pre-filled with NaN / -1, so an element a kernel failed to write shows up in the
parity check itself; a `zeros` / `full` body keeps the caller's fill (the result must equal the unguarded one), so there an unwritten
element does not show.  Which buffers are guarded is asserted by name (Arena.owns), not by a count.  Negative controls: an `empty` and a
`zeros` output one row too small ARE caught."""
import contextlib

import numpy as np
import pytest
import torch

from helpers import cloud
from redzone import Arena, RedzoneError, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from articulated_pose_amd import tf_ops
    return tf_ops


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_negative_control_a_row_too_few_is_caught(dev):
    """ancsh_group_point told that `out` holds m rows per cloud while the buffer holds m - 1: the last row lands in the redzone."""
    from articulated_pose_amd import _lib
    rng = np.random.RandomState(0)
    b, n, c, m, ns = 2, 100, 7, 9, 16
    pts, idx = T(rng.randn(b, n, c).astype(np.float32), dev), T(rng.randint(0, n, (b, m, ns)).astype(np.int32), dev)
    with pytest.raises(RedzoneError, match="PAST the buffer"):
        with guarded():
            out = torch.empty((b * m - 1, ns, c), dtype=torch.float32, device=dev)          # one row short
            _lib.call("ancsh_group_point", b, n, c, m, ns, _lib.ptr(pts), _lib.ptr(idx), _lib.ptr(out))
    with guarded() as arena:                                                                    # the exact size passes
        out = torch.empty((b * m, ns, c), dtype=torch.float32, device=dev)
        _lib.call("ancsh_group_point", b, n, c, m, ns, _lib.ptr(pts), _lib.ptr(idx), _lib.ptr(out))
        assert arena.check() == 1 and not torch.isnan(out).any()
    with pytest.raises(RedzoneError, match="BEFORE the buffer"):                               # and a write in front of a buffer
        with guarded():
            out = torch.empty((4, 4), dtype=torch.float32, device=dev)
            torch.as_strided(out, (1,), (1,), storage_offset=out.storage_offset() - 1).fill_(1.0)


@pytest.mark.parametrize("seed", range(0, 40, 3))
def test_operator_sweep_under_redzones(ops, oracle, dev, seed):
    import test_ops_sweep_gpu as S
    with guarded() as arena:
        S.test_fps_and_gather(ops, oracle, dev, seed)
        S.test_ball_query_and_group(ops, oracle, dev, seed)
        S.test_three_nn_and_interpolate(ops, oracle, dev, seed)
        S.test_conv1x1(oracle, dev, seed)
        assert arena.check() >= 8


@pytest.mark.parametrize("seed", [1, 6, 11, 33])
def test_unaligned_buffers(ops, oracle, dev, seed):
    """The operator entry points promise no alignment: the same checks with every buffer 4 bytes off a 16-byte boundary
    (the float4 / dwordx3 paths must take their scalar fallbacks, not fault or write a rounded-down address)."""
    import test_ops_sweep_gpu as S
    with guarded(misalign=4):
        S.test_fps_and_gather(ops, oracle, dev, seed)
        rng = np.random.RandomState(2000 + seed)
        b, n, m, ns = 3, 1000 + seed, 77, 24
        x, q = cloud(rng, b, n, "uniform"), cloud(rng, b, m, "uniform")
        gi, gc = ops.query_ball_point(0.3, ns, T(x, dev), T(q, dev))
        wi, wc = oracle.query_ball_point(0.3, ns, x, q)
        np.testing.assert_array_equal(gi.cpu().numpy(), wi)
        np.testing.assert_array_equal(gc.cpu().numpy(), wc)
        for c in (3, 7, 64):
            pts = rng.randn(b, n, c).astype(np.float32)
            np.testing.assert_array_equal(ops.group_point(T(pts, dev), gi).cpu().numpy(), oracle.group_point(pts, wi))
        S.test_three_nn_and_interpolate(ops, oracle, dev, seed)


@pytest.mark.parametrize("K,N,B", [(3, 777, 5), (2, 1000, 3), (4, 2048, 2), (3, 1024, 8), (7, 640, 2), (8, 512, 1), (1, 512, 3)])
def test_network_forward_under_redzones(dev, K, N, B):
    """Both forwards (layer API and the grouped / chained launches) with every activation, index and scratch buffer guarded; outputs
    equal to the unguarded run bit for bit (so no NaN body pattern survives in any head tensor).  K = 7 has the widest head blocks the
    tail chain takes (29 columns; the 10 joint columns start at column 57 of 68), K = 8 goes layer by layer, K = 1 has 1-column blocks."""
    from articulated_pose_amd.network import Network
    from articulated_pose_amd.paired import PairedNetworks
    from articulated_pose_amd.weights import synthetic_weights
    from test_network_gpu import synth_cloud
    P = torch.from_numpy(synth_cloud(np.random.RandomState(K * 10 + B), B, N)).to(dev)
    a = Network(K, synthetic_weights(K, seed=0), "ancsh", dev)
    n = Network(K, synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1), "npcs", dev)
    plain = [a.predict(P), n.predict(P)]
    with guarded() as arena:
        alone = [a.predict(P), n.predict(P)]
        pair = PairedNetworks([a, n]).predict(P)
        assert arena.check() > 40
    for g in range(2):
        for k in plain[g]:
            assert torch.equal(alone[g][k], plain[g][k]) and torch.equal(pair[g][k], plain[g][k]), (g, k)


@pytest.mark.parametrize("misalign", [0, 4])
def test_head_activations_under_redzones(dev, oracle, misalign):
    """every launch of tests/test_heads_gpu.py with each output guarded, and with each output 4 bytes off a 16-byte boundary (the entry
    promises no alignment): ragged row counts around the 256-thread block, K = 1..8, outputs absent one at a time and all but one"""
    import test_heads_gpu as HG
    n = 0
    for K, mixed in HG.CASES:
        with guarded(misalign=misalign) as arena:
            HG.test_head_activations_match_float64(dev, K, mixed)
            HG.test_optional_outputs(dev, K, mixed)
            n += arena.check()
    with guarded(misalign=misalign) as arena:
        HG.test_saturating_elementwise_logits(dev, oracle)
        for K, mixed in [(1, 1), (3, 1), (8, 0), (8, 1)]:
            HG.test_saturating_and_non_finite_softmax_rows(dev, oracle, K, mixed)
        n += arena.check()
    assert n > 5000


def test_split16_forward_k7_under_redzones(dev, monkeypatch):
    """the split-16 tail with the widest head blocks it takes (K = 7: 29 of its 32 padded columns, the joint block at column 57 of 68)"""
    import test_bf16x3_gpu as BX
    with guarded() as arena:
        BX.test_split16_forward_k7(dev, monkeypatch, "f16x2")
        assert arena.check() > 20


def test_chains_on_ragged_rows_under_redzones(dev):
    """the tail chains (one- and two-tile), the mid-section chains and the grouped conv launches on row counts that are not multiples
    of their 32-row tiles, unaligned inputs included"""
    import test_mid_chain_gpu as MC
    import test_mlp_gpu as M
    import test_network_gpu as NW
    with guarded() as arena:
        for rows, cin, ldx, offset in [(1, 131, 132, 0), (33, 131, 131, 0), (257, 131, 132, 1)]:
            M.test_mlp_chain_program_equals_layer_by_layer(dev, rows, cin, ldx, offset)
        for rows, ldx in [(1000, 132), (33, 131)]:
            M.test_mlp_chain_grouped_one_tile_equals_layer_by_layer(dev, rows, ldx)
        for G, B in [(1, 1), (2, 3), (3, 5)]:
            MC.test_mid_chains_equal_layer_by_layer(dev, G, B)
        MC.test_each_chain_against_its_layers(dev)
        NW.test_grouped_conv_equals_plain_bitwise(dev)
        assert arena.check() > 30


@pytest.mark.parametrize("seed", [0, 3, 5, 6, 9, 12, 17, 21])
def test_pose_fit_under_redzones(dev, seed):
    """PoseSolver.solve on the sweep's ragged problems (parts of two dozen points, K = 2 / 3 / 4, odd budgets) and with a part nobody
    is predicted as (empty part -> NaN rows, best = -1): every model, mask, score, record and scratch array guarded; results equal to
    the unguarded solve."""
    from articulated_pose_amd.pose import PoseSolver
    from articulated_pose_amd.pose.parallel_ancsh_pose import draws_from_seed
    from test_pose_sweep_gpu import _problem
    c, p, K, na, nb = _problem(seed)
    W = p["instance_per_point"].copy()
    if seed % 4 == 1:
        W[:, K - 1] = -1.0                                  # nobody in the last part
    counts = np.bincount(np.argmax(W, 1), minlength=K)
    da, db = draws_from_seed(500 + seed, np.maximum(counts, 1), na, nb)
    args = (c["P"][None], p["nocs_per_point"][None], W[None], p["joint_axis_per_point"][None], p["joint_cls_gt"][None], da[None], db[None])
    keys = ("record", "best_a", "best_b", "score_b", "inliers_a", "inliers_b", "tie_a", "tie_b", "counts", "labels")
    plain = PoseSolver(K, 0.1, na, nb, dev).solve(*args)
    plain = {k: plain[k].cpu().numpy() for k in keys}
    with guarded() as arena:
        sol = PoseSolver(K, 0.1, na, nb, dev).solve(*args)
        assert arena.check() >= 20
    for k in keys:
        np.testing.assert_array_equal(sol[k].cpu().numpy(), plain[k], err_msg=k)
    if seed % 4 == 1:
        assert np.isnan(plain["record"][0, K - 1]).all() and plain["best_a"][0, K - 1, 0] == -1


@pytest.mark.parametrize("seed", range(0, 40, 7))
def test_eval_kernel_sweep_under_redzones(dev, seed):
    """ancsh_joint_params (both variants), ancsh_articulation_rec and ancsh_part_extents on the placed-vote cases of
    tests/test_eval_kernels_sweep_gpu.py, every output guarded: st, joint, the block, its three debug outputs, extents, boundaries, counts"""
    import test_eval_kernels_sweep_gpu as S
    with guarded() as arena:
        S.sweep(dev, seed)
        assert arena.check() >= 8


def test_metric_input_and_loss_kernels_under_redzones(dev, oracle):
    import test_eval_scripts_gpu as E
    import test_input_gpu as I
    import test_joint_params_gpu as J
    import test_loss_gpu as L
    import test_metrics_gpu as Mx
    with guarded() as arena:
        Mx.test_iou_3d_random_vs_oracle_and_amodal_boxes(dev)
        Mx.test_scalar_metrics_golden(dev)
        for tag in J.cases():
            J.test_joint_params_match_reference_lines(dev, tag)
        J.test_joint_params_edge_cases(dev)
        I.test_input_sample_batch_equals_reference_records(dev)
        I.test_input_sample_device_rng_invariants(dev, oracle)
        for cfg in [(3, 257, 3, True, "L2"), (5, 64, 4, True, "L1")]:
            L.test_losses_match_oracle(dev, *cfg)
        for cfg in [(3, 257, 3, 9), (1, 2048, 8, 24)]:
            E.test_part_extents_kernel(dev, *cfg)
        assert arena.check() > 10


# ---- the buffers that come from torch.zeros / torch.full --------------------------------------------------------------------------------------
import redzone_cases as RC      # noqa: E402


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _host(named):
    """{name: tensor | tuple of tensors | None} -> {name: numpy array} (a tuple's members under name.0, name.1, ...)."""
    out = {}
    for name, v in named.items():
        for k, t in enumerate(v if isinstance(v, (tuple, list)) else [v]):
            if t is not None:
                out["%s.%d" % (name, k) if isinstance(v, (tuple, list)) else name] = t.cpu().numpy()
    return out


def _tensors(named):
    return [(name, t) for name, v in named.items() for t in (v if isinstance(v, (tuple, list)) else [v]) if t is not None]


def _assert_same_bytes(got, want):
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert _same(got[name], want[name]), (name, np.argwhere(got[name].reshape(-1).view(np.uint8) != want[name].reshape(-1).view(np.uint8))[:8].ravel())


def test_negative_control_a_zeros_output_a_row_too_short_is_caught(dev):
    """ancsh_refine_rec told that `wide` holds B * K rows of ld + 36 doubles while the torch.zeros buffer holds one (frame, part) row fewer:
    the last row (496 bytes, well inside the 4096 of the guard) lands in the redzone.  The exact size passes, and the buffer is the arena's."""
    from articulated_pose_amd import _lib
    from articulated_pose_amd.pose.refinement import refine_rec
    rng = np.random.RandomState(0)
    B, K, ld = 2, 3, 26
    best, carried = T(rng.randn(B, K, 2, 18), dev), T(rng.randn(B, K, ld), dev)
    with pytest.raises(RedzoneError, match="PAST the buffer"):
        with guarded():
            wide = torch.zeros((B * K - 1, ld + 36), dtype=torch.float64, device=dev)         # one row short
            _lib.call("ancsh_refine_rec", B, K, _lib.ptr(best), _lib.ptr(carried), ld, _lib.ptr(wide))
    want = refine_rec(best, carried).cpu().numpy()
    with guarded() as arena:
        wide = torch.zeros((B, K, ld + 36), dtype=torch.float64, device=dev)
        assert arena.owns(wide) and (wide == 0).all()
        _lib.call("ancsh_refine_rec", B, K, _lib.ptr(best), _lib.ptr(carried), ld, _lib.ptr(wide))
        assert arena.check() == 1
    assert _same(wide.cpu().numpy(), want) and _same(want[:, :, :ld], carried.cpu().numpy())


# ---- render-and-compare: every entry once, then the loop -----------------------------------------------------------------------------------
def _rc_inputs(dev, case):
    """What the entries only read, staged once outside any arena."""
    from articulated_pose_amd.depth import mesh_to_device
    from test_coverage_cpu import coverage_table
    from test_refinement_cpu import refine_table
    from test_refinement_gpu import _flat
    from test_reprojection_gpu import _t
    from test_silhouette_cpu import silhouette_table
    mesh, kin, render, scene, rigs, nf, geom, cap, frames = case["prob"]
    od, ol = _flat(case["prob"], case["dtype"])
    wide = np.concatenate([case["per"], np.random.RandomState(1).normal(size=case["per"].shape[:2] + (7,))], 2)      # ld = 33
    joints = dict(weight=1.0, axis_length=0.5)
    tables = dict(plain=refine_table(iters=1, min_pixels=1), sil=silhouette_table(iters=1, min_pixels=1),
                  cov=coverage_table(iters=1, min_pixels=1, joints=joints), loop=coverage_table(iters=2, min_pixels=1, joints=joints))
    d = {k: _t(np.array(v), dev) for k, v in dict(tables, od=od, ol=ol, render=render, scene=scene, rig=rigs, nf=nf, rec=wide, geom=geom, kin=kin).items()}
    d["mesh"] = mesh_to_device(mesh, dev)
    return d


def _rc_entries(dev, case, d, pixels=contextlib.nullcontext):
    """Every render-and-compare entry once on buffers allocated HERE (inside the caller's arena, or outside any), in the order the captured step
    issues them: the table builder, the renderer, the comparison, both fields, the three pass variants, the joint step, a second and last
    pass into the buffers' second rows, the record builder.  pixels(): the context the renderer's targets are allocated in (the renderer
    wants its depth plane 16-byte aligned, labels and z-buffer 8-byte).  -> {name: tensor or tuple of tensors}."""
    from articulated_pose_amd.depth import render_depth
    from articulated_pose_amd.pose.refinement import (coverage_field, field_buffer, refine_buffers, refine_joint_step, refine_pass, refine_rec,
                                                      silhouette_field)
    from articulated_pose_amd.pose.reprojection import predicted_buffers, predicted_frames, reproject_compare, reproject_scene_build
    K, dtype, cap = case["K"], case["dtype"], case["prob"][7]
    with pixels():
        (tables, pred), spare = predicted_frames(RC.B, cap, dtype, dev), predicted_buffers(cap, dtype, dev)
    plain = refine_buffers(RC.B, K, dev, passes=2)
    sil = refine_buffers(RC.B, K, dev, passes=2, silhouette=True, pixel_capacity=cap)
    full = refine_buffers(RC.B, K, dev, passes=2, silhouette=True, joints=True, pixel_capacity=cap, coverage=True)
    field = field_buffer(K, cap, dev)
    own = reproject_scene_build(d["render"], d["scene"], d["rig"], d["nf"], d["rec"], d["geom"], cap)       # the pair it allocates itself
    build = lambda src: reproject_scene_build(d["render"], d["scene"], d["rig"], d["nf"], src, d["geom"], cap, out=tables)
    draw = lambda into: render_depth(d["mesh"], tables[1], tables[0], dtype, out=into[:2], scratch=into[2])
    build(d["rec"])
    draw(pred)
    draw(spare)
    compared = reproject_compare(d["od"], d["ol"], pred[0], pred[1], d["geom"], d["scene"], d["rec"])
    for f in (field, sil.field, full.field):
        silhouette_field(d["od"], d["ol"], d["geom"], d["scene"], K, out=f)
    coverage_field(pred, tables[1], d["scene"], K, out=full.cover)
    head = (d["mesh"], d["od"], d["ol"], pred, d["geom"], d["scene"], tables[0], d["nf"])
    refine_pass(*head, d["plain"], 0, False, d["rec"], plain.work[0], plain.best, plain.sums[0])
    refine_pass(*head, d["sil"], 0, False, d["rec"], sil.work[0], sil.best, sil.sums[0], field=sil.field)
    refine_pass(*head, d["cov"], 0, False, d["rec"], full.work[0], full.best, full.sums[0], field=full.field, cover=full.cover)
    refine_joint_step(d["kin"], d["scene"], tables[0], d["nf"], d["cov"], 0, False, d["rec"], full.sums[0], full.work[0], full.best, full.state,
                      full.obj[0], full.xi[0])
    recs = [refine_rec(b.best, d["rec"]) for b in (plain, sil)]
    for b, par, kw in ((plain, "plain", {}), (sil, "sil", dict(field=sil.field)), (full, "cov", dict(field=full.field, cover=full.cover))):
        build(b.work[0])                                                 # pass 1, the last: the poses pass 0 left, into every buffer's second row
        draw(pred)
        if b is full:
            coverage_field(pred, tables[1], d["scene"], K, out=full.cover)
        refine_pass(*head, d[par], 1, True, b.work[0], b.work[1], b.best, b.sums[1], **kw)
    full.obj[1].copy_(full.obj[0])
    refine_joint_step(d["kin"], d["scene"], tables[0], d["nf"], d["cov"], 1, True, full.work[0], full.sums[1], full.work[1], full.best, full.state,
                      full.obj[1], full.xi[1])
    recs.append(refine_rec(full.best, d["rec"]))
    named = dict(tables=tables, pred=pred, spare=spare, own=own, compared=compared, field=field, recs=recs)
    for tag, b in (("plain", plain), ("sil", sil), ("full", full)):
        named.update({"%s.%s" % (tag, name): getattr(b, name) for name in b._fields})
    return named


@pytest.mark.parametrize("misalign", [0, 12])
@pytest.mark.parametrize("K,dtype,shapes", RC.CASES, ids=RC.IDS)
def test_render_and_compare_entries_under_redzones(dev, K, dtype, shapes, misalign):
    """ancsh_reproject_scene_build, the renderer, ancsh_reproject_compare_rec, both field entries, ancsh_refine_pass / _sil / _cov,
    ancsh_refine_joint_step and ancsh_refine_rec, one call each (and a second pass into row 1 of sums, obj and xi), on tests/redzone_cases.py's
    crops: B = 2, K = 1, 3, 8, 17 x 31 and 7 x 9 pixels or 7 x 9 and one, odd starts, the last crop ending at pixel_capacity -- so a wrong half
    offset v * pixel_capacity or a wrong NSUMS writes its first byte into a guard.  Every buffer comes from predicted_frames,
    predicted_buffers, refine_buffers or field_buffer inside the arena and is the arena's by name; every byte equals the same calls' outside
    it.  misalign = 12: float64 and int64 buffers 8 bytes off a 16-byte boundary, the others 12 -- the least the entries' checks accept --,
    but for the renderer's targets, which live in an arena of their own at misalign 0."""
    case = RC.problem(K, dtype, shapes)
    d = _rc_inputs(dev, case)
    want = _host(_rc_entries(dev, case, d))
    with guarded(misalign=misalign) as arena:
        pix = Arena() if misalign else arena
        named = _rc_entries(dev, case, d, pix.patched)
        for name, t in _tensors(named):
            assert pix.owns(t) if name in ("tables", "pred", "spare") else arena.owns(t), name
        assert misalign == 0 or all(t.data_ptr() % 16 == (8 if t.element_size() == 8 else 12) for _, t in _tensors(named) if not pix.owns(t))
        got = _host(named)
        assert (pix.check() if misalign else 0) + arena.check() >= len(_tensors(named))
    _assert_same_bytes(got, want)
    # the rows are not empty: pixels were used in every frame by every variant, and the comparison saw every frame's parts
    for tag in ("plain", "sil", "full"):
        s = got[tag + ".sums"]
        assert s.shape == (2, RC.B, K, 2, dict(plain=32, sil=36, full=40)[tag]) and all((s[0, f, :, :, 28] > 0).any() for f in range(RC.B)), tag
    assert (got["compared"][:, :, 33] > 0).any(1).all() and (got["pred.1"] != 255).any() and (got["full.cover"] != 0).any()
    assert got["full.xi"].shape == (2, RC.B, 2, 48) and got["full.obj"].shape == (2, RC.B, 2, 8) and got["recs.2"].shape == (RC.B, K, 33 + 36)


def _rc_loop(dev, case, d, pixels=contextlib.nullcontext):
    """reprojection_batch, then refine_batch for iters = 2 with the silhouette and coverage terms and the joint step, on buffers allocated HERE
    (pixels(): as in _rc_entries)."""
    from articulated_pose_amd.pose.refinement import refine_batch, refine_buffers
    from articulated_pose_amd.pose.reprojection import predicted_frames, reprojection_batch
    K, dtype, cap = case["K"], case["dtype"], case["prob"][7]
    with pixels():
        tables, pred = predicted_frames(RC.B, cap, dtype, dev)
    bufs = refine_buffers(RC.B, K, dev, passes=3, silhouette=True, joints=True, pixel_capacity=cap, coverage=True)
    args = (d["mesh"], d["render"], d["scene"], d["rig"], d["nf"], d["geom"], (d["od"], d["ol"]), d["rec"], dtype, tables, pred)
    reproj = reprojection_batch(*args)
    wide = refine_batch(*args, d["loop"], 2, bufs, kin=d["kin"])
    return dict(dict(("bufs." + name, getattr(bufs, name)) for name in bufs._fields), tables=tables, pred=pred, reproj=reproj, wide=wide)


@pytest.mark.parametrize("misalign", [0, 12])
@pytest.mark.parametrize("K,dtype,shapes", RC.CASES, ids=RC.IDS)
def test_refine_loop_under_redzones(dev, K, dtype, shapes, misalign):
    """pose.reprojection.reprojection_batch and pose.refinement.refine_batch (iters = 2, every term on, a kinematic table, so the joint step
    runs behind every pass and every pass keeps its rows of sums, obj and xi) as the captured step calls them: every member of the
    RefineBuffers record, the predicted tables and the pixel triple is an arena's (misalign = 12: as above), and every byte equals the
    unguarded run's."""
    from articulated_pose_amd.pose.refinement import RefineBuffers
    case = RC.problem(K, dtype, shapes)
    d = _rc_inputs(dev, case)
    want = _host(_rc_loop(dev, case, d))
    with guarded(misalign=misalign) as arena:
        pix = Arena() if misalign else arena
        named = _rc_loop(dev, case, d, pix.patched)
        assert all(named["bufs." + name] is not None for name in RefineBuffers._fields)
        for name, t in _tensors(named):
            assert pix.owns(t) if name in ("tables", "pred") else arena.owns(t), name
        got = _host(named)
        assert (pix.check() if misalign else 0) + arena.check() >= len(_tensors(named))
    _assert_same_bytes(got, want)
    s = got["bufs.sums"]
    assert s.shape == (3, RC.B, K, 2, 40) and all((s[p, f, :, :, 28] > 0).any() for p in range(3) for f in range(RC.B))
    assert got["wide"].shape == (RC.B, K, 33 + 36) and got["reproj"].shape == (RC.B, K, 33 + 15) and _same(got["wide"][:, :, :33], got["reproj"][:, :, :33])
    assert np.isfinite(got["wide"][:, :, 33:]).any() and (got["bufs.obj"][:, :, :, 3] > 0).any()


# ---- the joint states --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 8])
@pytest.mark.parametrize("b,n,K", [(3, 100, 3), (2, 64, 2), (1, 7, 1), (2, 257, 4)])
def test_joint_states_under_redzones(dev, b, n, K, misalign):
    """ancsh_joint_state_rec on tests/test_joint_states_gpu.py's shapes (which these are): the (b, K, 20) block in an `empty` and in a `zeros`
    buffer of the arena, equal to the unguarded launch; and that file's whole check of the shape, ancsh_part_extents' outputs guarded too."""
    import test_joint_states_gpu as JS
    from articulated_pose_amd import _lib
    assert (b, n, K) in JS.SHAPES and len(JS.SHAPES) == 4
    p = JS._problem(b, n, K)
    plain = JS._run(p).cpu().numpy()
    P, nocs, mask, rec, art = JS._dev(p["P"]), JS._dev(p["nocs"]), JS._dev(p["mask"]), JS._dev(p["rec"], torch.float64), JS._dev(p["art"], torch.float64)
    with guarded(misalign=misalign) as arena:
        wide = JS._run(p)
        zeroed = torch.zeros((b, K, 20), dtype=torch.float64, device=dev)
        assert arena.owns(wide) and arena.owns(zeroed)
        _lib.call("ancsh_joint_state_rec", b, n, K, _lib.ptr(P), p["ldp"], _lib.ptr(nocs), _lib.ptr(mask), _lib.ptr(rec), _lib.ptr(art), _lib.ptr(zeroed))
        got = wide.cpu().numpy(), zeroed.cpu().numpy()
        JS.test_kernel_against_mirror_and_part_extents(dev, b, n, K)
        assert arena.check() >= 7
    assert _same(got[0], plain) and _same(got[1], plain)


# ---- the streamed step -------------------------------------------------------------------------------------------------------------------------
# (render and scene are the slot's own only where the step builds them, from poses; elsewhere they are side inputs copied in from the host)
SLOT_BUFFERS = ("P", "joint_cls", "pred_nocs", "pred_mask", "pred_axis", "flags", "perm", "raw_rows", "src_rows", "hdr", "pix", "mask", "zbuf",
                "apix", "amask", "scratch", "counts", "link_counts", "render", "scene", "bounds", "gt_built", "frame_built")
ALWAYS = {"raw": ("P", "joint_cls", "pred_nocs", "pred_mask", "pred_axis", "flags", "raw_rows", "hdr"),
          "depth": ("P", "pred_nocs", "pred_mask", "pred_axis", "flags", "raw_rows", "hdr", "pix", "mask", "scratch", "counts"),
          "annotated": ("P", "pred_nocs", "pred_mask", "pred_axis", "flags", "perm", "raw_rows", "src_rows", "hdr", "pix", "mask", "apix", "amask",
                        "scratch", "counts", "link_counts", "gt_built", "frame_built")}
ALWAYS["posed"] = ALWAYS["library"] = ALWAYS["annotated"] + ("zbuf", "render", "scene", "bounds")


def _flatten(x):
    """A retired tuple's arrays, nested tuples and lists opened, in order; anything else (tags, seeds) as it is."""
    if isinstance(x, (tuple, list)):
        return [y for v in x for y in _flatten(v)]
    return [x]


def _stream(spec, slots, dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    pipe = AncshPipeline(spec["K"], spec["weights"][0], spec["weights"][1], spec["B"], spec["N"], dev, slots=slots, **spec["options"])
    return pipe, [_flatten(item) for item in getattr(pipe, spec["method"])(spec["feed"], *spec["args"], **spec["asked"])]


@pytest.mark.parametrize("kind,slots,dtype", RC.STREAM_CASES, ids=RC.STREAM_IDS)
def test_streamed_step_under_redzones(dev, kind, slots, dtype):
    """AncshPipeline constructed, prepared (its eager passes, both graphs' capture and first replays) and streamed inside the arena, once per
    input kind -- raw xyz clouds, depth frames with masks, annotated depth frames, posed frames of one mesh, posed frames of a library -- with
    every option the kind takes (tests/redzone_cases.py; the CPU test holds the flags), on the batches of the kind's own stream test, one of
    whose clouds leaves f16's range so that the f32 step retires too; one slot and four.  Every slot buffer, the predicted frames' tables
    and triple, the refine loop's record of buffers and the step's record outputs are the arena's by name; everything the stream returns
    equals, byte for byte, what a pipeline built outside the arena returns."""
    spec = RC.stream_kind(kind, dtype, dev)
    plain, want = _stream(spec, slots, dev)
    reruns = plain.f32_reruns
    del plain
    with guarded() as arena:
        pipe, got = _stream(spec, slots, dev)
        assert pipe.f32_reruns == reruns >= 1 and len(pipe.slots) == slots
        for i, sl in enumerate(pipe.slots):
            named = {name: getattr(sl, name, None) for name in SLOT_BUFFERS if kind in ("posed", "library") or name not in ("render", "scene")}
            assert all(named[name] is not None for name in ALWAYS[kind]), [name for name in ALWAYS[kind] if named[name] is None]
            named.update(reproj_tables=sl.reproj_tables, reproj_pix=sl.reproj_pix)
            for name in ("dense", "dense32", "rowlab", "rowlab32", "img", "img32", "aimg", "aimg32"):
                named[name] = getattr(sl, name, None)
            if sl.refine_bufs is not None:
                named.update({"refine_bufs." + name: getattr(sl.refine_bufs, name) for name in sl.refine_bufs._fields})
            for out, tag in ((sl.out, "out"), (sl.out32, "out32")):     # the step's records and blocks: allocated inside the capture
                named.update({"%s.%s" % (tag, name): v for name, v in out.items() if name.startswith("record") or name == "articulation"})
            if kind in ("posed", "library"):
                assert all(named[name] is not None for name in ("reproj_tables", "reproj_pix", "aimg", "aimg32", "refine_bufs.cover", "refine_bufs.state"))
                assert "out.record_refined" in named and "out32.record_refined" in named
            for name, t in _tensors(named):
                assert arena.owns(t), (i, name)
        del pipe
    assert len(got) == len(want) == len(spec["feed"])
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and g[:2] == w[:2], k
        for j, (a, b) in enumerate(zip(g[2:], w[2:])):
            assert _same(a, b), (k, j)
    assert any(np.isfinite(g[2]).any() for g in got)
