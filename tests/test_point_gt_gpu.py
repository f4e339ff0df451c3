"""GPU: the per-point ground truth of a streamed batch (ancsh_point_gt_rec, pose.point_gt.point_gt_batch, AncshPipeline / ShardedPipeline
point_ground_truth=True): bit-equal to the entries it fuses (ancsh_input_sample, then ancsh_test_losses and ancsh_joint_params on the
gathered tensors), against the reference's own joint numbers (tests/golden/joint_params.npz) at the bars tests/test_joint_params_gpu.py
holds the offline path to, against the loss oracle at tests/test_loss_gpu.py's bar, and through the captured stream, the keyed header, the
network's own joint association, the range guard and two gloo ranks."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import check_record_layout, passthrough_pose_problem
from redzone import guarded
from test_joint_params_cpu import G as GOLDEN, cases, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOAD = np.frombuffer(np.array([0x7ff8000000000abc], np.uint64).tobytes(), np.float64)[0]       # a NaN with a payload
W21 = 21


def _same(a, b):
    """byte equality (NaN-safe)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0", dt).contiguous()


def random_channels(rs, n, K, jcls=None):
    """(n, 15) channels 3..17 of a packed row: cls (some -1), nocs_p, nocs_g, heatmap, unitvec, orient, joint_cls."""
    ch = rs.uniform(0.0, 1.0, (n, 15)).astype(np.float32)
    ch[:, 0] = rs.randint(0, K, n)
    ch[rs.uniform(size=n) < 0.1, 0] = -1.0
    ch[:, 8:14] = rs.normal(size=(n, 6))
    ch[:, 14] = rs.randint(0, K, n) if jcls is None else jcls
    return ch


# ---- the kernel against the entries it fuses ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(N, K, G):
    """B = 3 ragged clouds (n_raw = 1, N - 1, 3N + 5), a random perm with entries >= n_raw, random heads, blocks, frames and records."""
    rs = np.random.RandomState(1000 * K + N + G)
    B, JC = 3, 3
    clouds = []
    for c, n_raw in enumerate((1, N - 1, 3 * N + 5)):
        rows = np.concatenate([rs.uniform(-1, 1, (n_raw, 3)).astype(np.float32), random_channels(rs, n_raw, K)], 1)
        if c == 2 and K > 1:
            rows[rows[:, 17] == K - 1, 17] = 0.0                    # joint class K - 1 has no points in cloud 2
        clouds.append(rows)
    from articulated_pose_amd.dataset import tiled_size
    perms = [rs.randint(0, tiled_size(c.shape[0], N), N).astype(np.int32) for c in clouds]
    assert (perms[0] >= 1).any() and (perms[1] >= N - 1).any()
    h = lambda ch: rs.normal(size=(B, N, ch)).astype(np.float32)
    ancsh = {"W": rs.uniform(0, 1, (B, N, K)).astype(np.float32), "nocs_per_point": h(3 * K), "gocs_per_point": h(G), "heatmap_per_point": h(1),
             "unitvec_per_point": h(3), "joint_axis_per_point": h(3), "index_per_point": rs.uniform(0, 1, (B, N, JC)).astype(np.float32)}
    npcs = {"W": rs.uniform(0, 1, (B, N, K)).astype(np.float32), "nocs_per_point": h(3 * K)}
    art = rs.normal(size=(B, K, 20))
    frame = rs.normal(size=(B, 13))
    rec = rs.normal(size=(B, K, 51))
    rec[1, K - 1, 7] = PAYLOAD
    rec[2, 0, 25] = np.nan
    return dict(clouds=clouds, perms=perms, ancsh=ancsh, npcs=npcs, art=art, frame=frame, rec=rec, N=N, K=K, G=G)


def _launch(p, ld=26, ld_art=12, order=(0, 1, 2), type_l="L2", frame=None, art=None):
    """point_gt_batch on problem p with its clouds in `order` -> (block, joint_gt) on the host, in that order."""
    from articulated_pose_amd.pose.point_gt import point_gt_batch
    order = list(order)
    clouds = [p["clouds"][c] for c in order]
    off = np.zeros(len(order) + 1, np.int32)
    off[1:] = np.cumsum([c.shape[0] for c in clouds])
    sel = lambda d: {k: _dev(v[order]) for k, v in d.items()}
    art = p["art"] if art is None else art
    frame = p["frame"] if frame is None else frame
    with guarded():                                                 # both outputs inside red zones (tests/redzone.py)
        wide, jg = point_gt_batch(_dev(np.concatenate(clouds)), _dev(off, torch.int32), _dev(np.stack([p["perms"][c] for c in order]), torch.int32),
                                  sel(p["ancsh"]), sel(p["npcs"]), _dev(art[order][:, :, :ld_art], torch.float64), _dev(frame[order], torch.float64),
                                  _dev(p["rec"][order][:, :, :ld], torch.float64), type_l, debug=True)
        torch.cuda.synchronize()
        out = wide.cpu().numpy(), jg.cpu().numpy()
    return out


def _offline(p, type_l="L2"):
    """ancsh_input_sample on the same perm, then ancsh_test_losses for both networks and ancsh_joint_params(axis_mean=1): -> (the
    (B, K, 13) columns +8..+20 as float64, joint_gt (B, K-1, 6))."""
    from articulated_pose_amd.dataset import create_unit_data_batch
    from articulated_pose_amd.loss import compute_loss
    from articulated_pose_amd.pose.joint_params import joint_params_gt_batch
    N, K, G = p["N"], p["K"], p["G"]
    gt = create_unit_data_batch(p["clouds"], N, [1.0] * 3, K, perms=p["perms"])
    mixed = G == 3 * K
    a = {k: _dev(v) for k, v in p["ancsh"].items()}
    la = compute_loss(a, gt, K, mixed, type_l)
    ln = compute_loss(dict(a, W=_dev(p["npcs"]["W"]), nocs_per_point=_dev(p["npcs"]["nocs_per_point"])), gt, K, False, type_l)
    B = 3
    want = np.full((B, K, 13), np.nan)
    f64 = lambda t: t.double().cpu().numpy()
    want[:, :, 0], want[:, :, 1] = f64(la["miou_loss"]), f64(ln["miou_loss"])
    cls, jcls = gt["cls_gt"].cpu().numpy().astype(np.int32), gt["joint_cls_gt"].cpu().numpy().astype(np.int32)
    for j in range(K):
        want[:, j, 2], want[:, j, 3] = (cls == j).sum(1), (jcls == j).sum(1)
    want[:, :, 4] = f64(la["nocs_loss"])[:, None]
    if mixed:
        want[:, :, 5] = f64(la["gocs_loss"])[:, None]
    for k, key in enumerate(("heatmap_loss", "unitvec_loss", "orient_loss")):
        want[:, :, 6 + k] = f64(la[key])[:, None]
    want[:, :, 9:12] = f64(la["index_loss"])[:, None, :]
    want[:, :, 12] = f64(ln["nocs_loss"])[:, None]
    jp = joint_params_gt_batch(dict(nocs_gt_g=gt["nocs_gt_g"].contiguous(), heatmap_gt=gt["heatmap_gt"].contiguous(), unitvec_gt=gt["unitvec_gt"].contiguous(),
                                    joint_axis_gt=gt["orient_gt"].contiguous(), joint_cls_gt=gt["joint_cls_gt"].contiguous()), K, np.ones(B), np.tile(np.eye(4), (B, 1, 1)))
    torch.cuda.synchronize()
    return want, torch.cat([jp["joint_pt"], jp["joint_axis"]], 2).cpu().numpy()


SHAPES = [(64, 1, 3), (64, 2, 6), (257, 2, 3), (257, 4, 12), (1000, 1, 3), (1000, 2, 6), (1000, 4, 3), (64, 4, 12), (257, 1, 3)]


@pytest.mark.parametrize("N,K,G", SHAPES, ids=lambda v: str(v))
def test_bit_equal_to_the_fused_entries(dev, N, K, G):
    p = _problem(N, K, G)
    ld = (26, 39, 38, 51)[(N + K) % 4]
    got, jg = _launch(p, ld=ld, ld_art=12 if K % 2 else 20)
    want, jwant = _offline(p)
    assert got.shape == (3, K, ld + W21) and _same(got[:, :, :ld], p["rec"][:, :, :ld])      # the carried row, NaN payloads included
    assert _same(got[:, :, ld + 8:], want), (got[:, :, ld + 8:] - want)
    assert _same(jg, jwant)
    assert np.isnan(got[:, 0, ld:ld + 8]).all()
    if K > 1:
        assert np.isnan(jg[2, K - 2]).all() and np.isnan(got[2, K - 1, ld:ld + 8]).all()      # the joint class without points
        assert np.isfinite(got[1, 1:, ld:ld + 8]).any()
    assert np.isnan(got[:, :, ld + 13]).all() == (G != 3 * K)            # gocs_loss needs the per-part global NOCS head
    # the same bytes on a second run and wherever the cloud lies in the batch
    again, _ = _launch(p, ld=ld, ld_art=12 if K % 2 else 20)
    assert _same(again, got)
    moved, jm = _launch(p, ld=ld, ld_art=12 if K % 2 else 20, order=(2, 0, 1))
    assert _same(moved, got[[2, 0, 1]]) and _same(jm, jg[[2, 0, 1]])
    alone, _ = _launch(p, ld=ld, ld_art=12 if K % 2 else 20, order=(1,))
    assert _same(alone[0], got[1])


@pytest.mark.parametrize("ld", [26, 39, 38, 51])
def test_carried_columns_and_nan_rules(dev, ld):
    p = _problem(64, 4, 12)
    base, _ = _launch(p, ld=ld)
    assert _same(base[:, :, :ld], p["rec"][:, :, :ld]) and base[1, 3, 7].view(np.uint64) == 0x7ff8000000000abc
    frame, art = p["frame"].copy(), p["art"].copy()
    frame[1, 4] = np.nan                                           # a NaN in a frame blanks +0..+7 of that cloud
    art[0, 2, 10] = np.nan                                         # a NaN in a predicted joint blanks +0 and +1 of that row
    got, _ = _launch(p, ld=ld, frame=frame, art=art)
    assert np.isnan(got[1, :, ld:ld + 8]).all() and _same(got[1, :, ld + 8:], base[1, :, ld + 8:]) and _same(got[2], base[2])
    assert np.isnan(got[0, 2, ld:ld + 2]).all() and _same(got[0, 2, ld + 2:], base[0, 2, ld + 2:])
    assert _same(got[0, [0, 1, 3]], base[0, [0, 1, 3]])


# ---- against the reference's own lines -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", cases())
def test_against_the_reference_numbers(dev, tag):
    from articulated_pose_amd.pose.point_gt import pack_joint_frame, point_gt_batch
    with np.load(GOLDEN) as z:
        c = load(z, tag)
    N, K = c["mask_pred"].shape
    rows = np.zeros((N, 18), np.float32)
    rows[:, 7:10], rows[:, 10], rows[:, 11:14], rows[:, 14:17], rows[:, 17] = c["nocs_gt_g"], c["heatmap_gt"], c["unitvec_gt"], c["orient_gt"], c["joint_cls_gt"]
    one = lambda a: _dev(a[None])
    ancsh = {"W": one(c["mask_pred"]), "nocs_per_point": one(c["nocs"]), "gocs_per_point": one(c["gocs"]), "heatmap_per_point": one(c["heatmap_pred"][:, None]),
             "unitvec_per_point": one(c["unitvec_pred"]), "joint_axis_per_point": one(c["orient_pred"]), "index_per_point": one(c["index_per_point"])}
    npcs = {"W": one(c["mask_pred"]), "nocs_per_point": one(c["nocs"])}
    art = np.full((1, K, 12), np.nan)
    art[0, 1:, 6:9], art[0, 1:, 9:12] = c["cam_p_pred"], c["cam_l_pred"]
    frame = pack_joint_frame([list(c["gt_rt"])], [list(c["gt_s"])])
    wide, jg = point_gt_batch(_dev(rows), _dev(np.array([0, N]), torch.int32), _dev(np.arange(N)[None], torch.int32), ancsh, npcs,
                              _dev(art, torch.float64), _dev(frame, torch.float64), _dev(np.zeros((1, K, 26)), torch.float64), debug=True)
    got, jg = wide.cpu().numpy()[0], jg.cpu().numpy()[0]
    np.testing.assert_array_equal(jg[:, :3], c["joint_p_gt"])
    np.testing.assert_array_equal(jg[:, 3:], c["joint_l_gt"])
    for name, a, b, tol in (("p_gt", got[1:, 28:31], c["cam_p_gt"], 2e-6), ("l_gt", got[1:, 31:34], c["cam_l_gt"], 1e-6),
                            ("angle_err", got[1:, 26], c["angle_err"], 1e-4), ("dist_err", got[1:, 27], c["dist_err"], 1e-5)):
        print("point_gt %s %s: max |kernel - reference| = %.3g" % (tag, name, np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=0, atol=tol)


# ---- the losses against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("type_l", ["L2", "L1"])
@pytest.mark.parametrize("N,K,G", [(257, 2, 6), (1000, 4, 3)], ids=lambda v: str(v))
def test_losses_against_the_oracle(dev, N, K, G, type_l):
    from oracle import loss_oracle as LO
    p = _problem(N, K, G)
    got, _ = _launch(p, type_l=type_l)
    for c in range(3):
        g = p["clouds"][c][p["perms"][c] % p["clouds"][c].shape[0]][None]      # the gathered rows (1, N, 18)
        gt = dict(cls_gt=g[:, :, 3].astype(np.int32), nocs_gt=g[:, :, 4:7], nocs_gt_g=g[:, :, 7:10], heatmap_gt=g[:, :, 10], unitvec_gt=g[:, :, 11:14],
                  orient_gt=g[:, :, 14:17], joint_cls_gt=g[:, :, 17].astype(np.int32), joint_cls_mask=(g[:, :, 17] > 0).astype(np.float32),
                  mask_array=np.eye(K, dtype=np.float32)[g[:, :, 3].astype(np.int8)])
        pa = {k: v[c:c + 1] for k, v in p["ancsh"].items()}
        la = LO.loss_dict(pa, gt, K, G == 3 * K, type_l)
        ln = LO.loss_dict(dict(pa, W=p["npcs"]["W"][c:c + 1], nocs_per_point=p["npcs"]["nocs_per_point"][c:c + 1]), gt, K, False, type_l)
        want = {34: la["miou_loss"][0], 35: ln["miou_loss"][0], 38: la["nocs_loss"][0], 40: la["heatmap_loss"][0], 41: la["unitvec_loss"][0],
                42: la["orient_loss"][0], 46: ln["nocs_loss"][0]}
        if G == 3 * K:
            want[39] = la["gocs_loss"][0]
        for col, w in want.items():
            a = got[c, :, col]
            print("point_gt loss col %d cloud %d: max |kernel - oracle| = %.3g" % (col, c, np.abs(a - w).max()))
            np.testing.assert_allclose(a, np.broadcast_to(w, a.shape), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(got[c, 0, 43:46], la["index_loss"][0], rtol=1e-5, atol=1e-6)


# ---- the stream ----------------------------------------------------------------------------------------------------------------------------
K_, B_, N_ = 3, 4, 512


def widen(batches, rs, K=K_):
    """(n, 4) clouds [x y z joint_cls] -> (n, 18) rows with random ground-truth channels; column 17 keeps the joint label."""
    return [([np.concatenate([c[:, :3], random_channels(rs, c.shape[0], K, jcls=c[:, 3])], 1).astype(np.float32) for c in b[0]],) + tuple(b[1:])
            for b in batches]


def random_frames(rs, n):
    return rs.normal(size=(n, 13))


def _batches(pb, count, rs):
    from test_articulation_gpu import _stream_batches
    return _stream_batches(pb, K_, B_, N_, count, rs)              # a short batch at k = 0, a NaN cloud in batch 5


def _pipe(pb, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    kw = dict(dict(couple=True, slots=2, niter_a=64, niter_b=8, seed=11, lm_schedule="throughput", raw_capacity=B_ * 3 * N_, articulation=True), **kw)
    return AncshPipeline(K_, pb["w_ancsh"], pb["w_npcs"], B_, N_, "cuda:0", **kw)


def _check_slot(pipe, k, rows, frame, seed, cloud_base=0, f32=False):
    """rows = batch k's retired records; its slot still holds that batch's raw rows, header, perm, heads, block, frames and carried record:
    point_gt_batch on them gives the streamed 21 columns byte for byte, and the perm is the sampler mirror's."""
    import stream_mirror as SM
    from articulated_pose_amd.pose.point_gt import point_gt_batch
    sl = pipe.slots[k % len(pipe.slots)]
    sl.stream.synchronize()
    out = sl.out32 if f32 else sl.out
    carried = out["record_gt"] if pipe.ground_truth else out["record_wide"] if pipe.fit_quality else out["record"]
    ld, n = carried.shape[2], len(rows)
    L = pipe.record_layout
    assert out[L.carried("point_gt")[0]] is carried and L.carried("point_gt")[1] == ld and L.key == "record_point_gt" and L.width == rows.shape[2]
    assert out["record"].shape == (pipe.B, pipe.K, 26) and out["record_point_gt"].shape == (pipe.B, pipe.K, ld + W21) == (pipe.B, pipe.K, rows.shape[2])
    dev_fr = sl.frame.cpu().numpy()
    assert np.isnan(dev_fr[n:]).all() and (_same(dev_fr[:n], frame) if frame is not None else np.isnan(dev_fr).all())
    off = sl.header(pipe.B)[1]
    want = point_gt_batch(sl.raw_rows, off, sl.perm, out["ancsh"], out["npcs"], out["articulation"], sl.frame, carried)
    torch.cuda.synchronize()
    assert _same(out["record_point_gt"].cpu().numpy()[:n], want.cpu().numpy()[:n])
    o, perm = off.cpu().numpy(), sl.perm.cpu().numpy()
    for c in range(n):
        assert np.array_equal(perm[c], SM.sample_perm(seed, cloud_base + c, int(o[c + 1] - o[c]), pipe.N)), (k, c)
    return ld, want.cpu().numpy()[:n]


@pytest.mark.parametrize("fit_quality,ground_truth", [(False, False), (True, True)], ids=["record", "widest"])
def test_stream_keeps_the_record_and_adds_the_columns(dev, fit_quality, ground_truth):
    from test_gt_errors_gpu import _random_gt
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 6, np.random.RandomState(2))
    rs = np.random.RandomState(7)
    wide = widen(plain, rs)
    gts = [_random_gt(rs, len(b[0]), K_) for b in plain]
    frames = [None if k == 3 else random_frames(rs, len(b[0])) for k, b in enumerate(plain)]
    kw = dict(fit_quality=fit_quality, ground_truth=ground_truth)
    with_gt = lambda bs, fr: [(b[0], b[1]) + ((g,) if ground_truth else ()) + ((f,) if fr else ()) for b, g, f in zip(bs, gts, frames)]
    base = list(_pipe(pb, **kw).stream_batches(with_gt(plain, False), articulation=True))
    pipe = _pipe(pb, point_ground_truth=True, **kw).prepare()
    ld = 26 + (13 if fit_quality else 0) + (12 if ground_truth else 0)
    assert pipe.slots[0].outputs["record"].host[0].shape == (B_, K_, ld + W21) and pipe.slots[0].raw_rows.shape[1] == 18
    L = check_record_layout(pipe, ["pose"] + ["fit_quality"] * fit_quality + ["gt_errors"] * ground_truth + ["point_gt"])
    n = 0
    for k, ((t0, s0, r0, a0), (t1, s1, r1, a1)) in enumerate(zip(base, pipe.stream_batches(with_gt(wide, True), articulation=True))):
        assert (t0, s0) == (t1, s1) == (k, 11 + 2 * k) and r1.shape == (len(plain[k][0]), K_, ld + W21)
        assert _same(r0, r1[..., :ld]) and _same(a0, a1)           # the record and the block of the pipeline without the option
        assert L.width == r1.shape[2] and _same(L.block(r1, "point_gt"), r1[..., ld:]) and _same(L.block(r1, "pose"), r0[..., :26])
        got_ld, want = _check_slot(pipe, k, r1, frames[k], 11 + 2 * k)
        assert got_ld == ld and _same(r1, want)
        assert (r1[:, :, ld + 10].sum(1) <= N_).all() and (r1[:, :, ld + 11].sum(1) == N_).all()
        if frames[k] is None:
            assert np.isnan(r1[:, :, ld:ld + 8]).all()
        elif k == 5:                                                # the NaN cloud: a poisoned record has no predicted joint
            assert np.isnan(r1[1, :, ld:ld + 2]).all()
        n += 1
    assert n == 6
    with pytest.raises(ValueError, match=r"frame must be \(%d, 13\)" % len(plain[1][0])):
        pipe.submit(wide[1][0], wide[1][1], frame=np.zeros((len(plain[1][0]) + 1, 13)))
    with pytest.raises(ValueError, match="18"):
        pipe.submit(plain[1][0], plain[1][1])


def test_stream_keyed_at_a_cloud_base(dev):
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 3, np.random.RandomState(4))
    rs = np.random.RandomState(8)
    wide = widen(plain, rs)
    base, pipe = _pipe(pb, keyed=True), _pipe(pb, keyed=True, point_ground_truth=True)
    for k, ((c4, nf), (c18, _)) in enumerate(zip(plain, wide)):
        fr = random_frames(rs, len(c4))
        base.submit(c4, nf, cloud_base=40 + k)
        pipe.submit(c18, nf, cloud_base=40 + k, frame=fr)
        (_, s0, r0), (_, s1, r1) = base.retire(), pipe.retire()
        assert s0 == s1 and _same(r0, r1[..., :26])
        _, want = _check_slot(pipe, k, r1, fr, s1, cloud_base=40 + k)
        assert _same(r1, want)


def test_stream_with_the_predicted_joint_association(dev):
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 3, np.random.RandomState(5))
    rs = np.random.RandomState(9)
    wide = widen(plain, rs)
    frames = [random_frames(rs, len(b[0])) for b in plain]
    base = list(_pipe(pb, joint_source="predicted").stream_batches(plain))
    pipe = _pipe(pb, joint_source="predicted", point_ground_truth=True)
    for k, ((_, s0, r0), (_, s1, r1)) in enumerate(zip(base, pipe.stream_batches([b + (f,) for b, f in zip(wide, frames)]))):
        assert s0 == s1 and _same(r0, r1[..., :26])
        _, want = _check_slot(pipe, k, r1, frames[k], s1)
        assert _same(r1, want) and (r1[:, :, 26 + 11].sum(1) == N_).all()


def test_range_guard_takes_the_f32_rows(dev):
    """One cloud forced over f16's range by its norm factor, as tests/test_gt_errors_gpu.py does: its 47 columns are the f32 graph's."""
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    plain = _batches(pb, 4, np.random.RandomState(9))
    hot = []
    for k, (clouds, nf) in enumerate(plain):
        h = np.zeros(len(clouds), bool)
        if k % 2 == 1:
            nf[0] = 1e6
            h[0] = True
        hot.append(h)
    rs = np.random.RandomState(6)
    batches = [b + (random_frames(rs, len(b[0])),) for b in widen(plain, rs)]
    mk = lambda arith, guard: _pipe(pb, arithmetic=arith, range_guard=guard, point_ground_truth=True)
    f32 = list(mk("f32", False).stream_batches(batches))
    f16 = list(mk("f16x2", False).stream_batches(batches))
    guarded_pipe = mk("f16x2", True)
    assert guarded_pipe.slots[0].outputs["record"].host32[0].shape == (B_, K_, 47)
    got = list(guarded_pipe.stream_batches(batches, flags=True))
    assert guarded_pipe.f32_reruns == 2
    for (tag, _, rec, words), (_, _, r32), (_, _, r16), h in zip(got, f32, f16, hot):
        assert ((words != 0) == h).all() and rec.shape[2] == 47, tag
        assert _same(rec[h], r32[h]) and _same(rec[~h], r16[~h]), tag


def test_launch_budget(dev):
    """The option adds ancsh_point_gt_rec -- one ABI call, no other new name -- behind the articulation launches; the rest of the
    sequence is the plain pipeline's."""
    from test_fit_quality_gpu import _launch_names
    pb = passthrough_pose_problem(K_, 6, N_, seed=3)
    for kw in (dict(joint_states=True, fit_quality=True, ground_truth=True, dense=True), dict()):
        plain = _launch_names(_pipe(pb, slots=1, **kw).prepare())
        on = _launch_names(_pipe(pb, slots=1, point_ground_truth=True, **kw).prepare())
        new = [x for x in on if x not in plain]
        assert "ancsh_point_gt_rec" in new and len(new) <= 2 and len(on) - len(plain) <= 2
        at = on.index("ancsh_point_gt_rec")
        assert [x for x in on if x not in new] == plain
        assert on[at - 1] == ("ancsh_joint_state_rec" if kw else "ancsh_articulation_rec")
        if kw:
            assert on[at + 1] == "ancsh_raw_point_labels"


# ---- two gloo ranks --------------------------------------------------------------------------------------------------------------------------
def sharded_point_gt_problem():
    """tests/test_joint_states_gpu.py's global batches widened to 18 columns, with frames in front of the tag; batch 2 travels without."""
    from test_joint_states_gpu import sharded_problem
    pb, batches, K, G, N, kw = sharded_problem()
    rs = np.random.RandomState(41)
    wide = widen(batches, rs, K)
    return pb, [(c, nf, None if k == 2 else random_frames(rs, len(c)), tag) for k, (c, nf, tag) in enumerate(wide)], K, G, N, kw


_SHARDED = r'''
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import articulated_pose_amd  # noqa: F401
from articulated_pose_amd import dist as D
sys.path.insert(0, sys.argv[1] + "/tests")
world, out = int(sys.argv[2]), sys.argv[3]
if D.wants_self_launch(world):
    sys.exit(D.launch_local_ranks(world, [sys.executable] + sys.argv, timeout=300))
import torch.distributed as dist
from test_point_gt_gpu import sharded_point_gt_problem
pb, batches, K, G, N, kw = sharded_point_gt_problem()
group, note = D.init_groups("gloo", "cuda:0")
sp = D.ShardedPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=3 * 3 * N, articulation=True, point_ground_truth=True, **kw)
got = list(sp.stream_batches(batches))
if dist.get_rank() != 0:
    assert all(r is None for _, _, r in got)
    got = None
dist.barrier()
dist.destroy_process_group()
if got is not None:
    np.savez(out, tags=np.array([t for t, _, _ in got]), counts=np.array([len(r) for _, _, r in got]), records=np.concatenate([r for _, _, r in got]))
'''


def test_sharded_rows_equal_one_pipeline(dev, tmp_path):
    """Two self-launched gloo ranks on one GPU (as tests/test_gt_errors_gpu.py runs them): every rank gets its shard's clouds and frames,
    and rank 0's gathered (n_valid, K, 47) rows equal one AncshPipeline stream's, byte for byte."""
    from articulated_pose_amd.pipeline import AncshPipeline
    pb, batches, K, G, N, kw = sharded_point_gt_problem()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], G, N, "cuda:0", raw_capacity=G * 3 * N, articulation=True, point_ground_truth=True, **kw)
    one = list(pipe.stream_batches(batches))
    del pipe
    script = tmp_path / "sharded_point_gt.py"
    script.write_text(_SHARDED)
    out = tmp_path / "pgt2.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, str(script), ROOT, "2", str(out)], env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    two = np.load(out)
    assert list(two["tags"]) == [t for t, _, _ in one] and list(two["counts"]) == [len(r) for _, _, r in one]
    assert two["records"].shape[1:] == (K, 47) and _same(two["records"], np.concatenate([r for _, _, r in one]))
    recs = np.split(two["records"], np.cumsum(two["counts"])[:-1])
    assert np.isnan(recs[2][:, :, 26:34]).all() and np.isfinite(recs[1][:, 1:, 28:34]).any() and np.isfinite(recs[2][:, :, 34:38]).all()
