"""CPU (no GPU): the fit-quality entry (ancsh_fit_quality_rec) is exported without a new ABI number and checks its arguments before any
launch; the constructors refuse what it cannot use before anything touches a device; the numpy mirror the GPU tests compare against
(tests/fit_quality_mirror.py) agrees with the reference's own verifiers on the golden problems (tests/golden/fit_quality.npz: masks and
scores exactly, norms within 16 roundings); and ShardedPipeline gathers the 39-wide records of two gloo ranks in global cloud order.

Norms, mirror against reference: the largest difference over the golden problems is 1.17 in units of 2^-53 M (M = max|tgt| + |s| (|x_0| +
|x_1| + |x_2|) + max|t| per point), against the bound of 16 (the test prints it)."""
import ctypes
import datetime
import os

import numpy as np
import pytest
import torch.distributed as dist

from fit_quality_mirror import WIDTH, fit_quality_reference, five, partition, residual_norms
from test_dist_cpu import _run_ranks
from test_sharded_stream_cpu import CAP, _batches, _expected, _FakeStreamPipeline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_quality.npz")
P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_entry_is_exported_and_the_abi_number_stays():
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    L = _lib.lib()
    assert "ancsh_fit_quality_rec" in declared_symbols() and hasattr(L, "ancsh_fit_quality_rec")
    assert len(_lib.SIGNATURES["ancsh_fit_quality_rec"]) == 11
    assert L.ancsh_abi_version() == 14


def test_bad_arguments_are_rejected_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    call = lambda b=1, K=3, th=0.1, wide=P8, off=P8: L.ancsh_fit_quality_rec(b, K, off, P8, P8, P8, th, P8, P8, wide, None)
    assert call(K=0) == -1 and b"K=0" in L.ancsh_last_error()
    assert call(K=17) == -1 and b"K=17" in L.ancsh_last_error()
    assert call(wide=None) == -1 and b"null pointer" in L.ancsh_last_error()
    assert call(off=None) == -1 and b"null pointer" in L.ancsh_last_error()
    for th in (0.0, -0.1, float("inf"), float("nan")):
        assert call(th=th) == -1 and b"inlier_th" in L.ancsh_last_error(), th
    assert call(b=-1) == -1 and b"b=-1" in L.ancsh_last_error()
    assert L.ancsh_fit_quality_rec(0, 3, None, None, None, None, 0.1, None, None, None, None) == 0       # nothing to do: nothing enqueued


def test_constructor_guards():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    from articulated_pose_amd.pose.quality import FIT_QUALITY_WIDTH, check_fit_quality
    assert FIT_QUALITY_WIDTH == WIDTH
    assert check_fit_quality(True, 0.1) is True and check_fit_quality(False, -1.0) is False and check_fit_quality(0, 0.1) is False
    for th in (0.0, -0.1, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="inlier_th"):
            check_fit_quality(True, th)
    # the constructors call it before they build a network or touch a device ("cpu" never reaches a kernel)
    with pytest.raises(ValueError, match="fit_quality=True .* inlier_th"):
        AncshPipeline(3, {}, {}, 2, 64, "cpu", inlier_th=0.0, fit_quality=True)
    with pytest.raises(ValueError, match="fit_quality=True .* inlier_th"):
        ShardedPipeline(3, {}, {}, 2, 64, "cpu", raw_capacity=1024, inlier_th=-1.0, fit_quality=True)
    with pytest.raises(ValueError, match="fit_quality=True .* raw_capacity"):
        ShardedPipeline(3, {}, {}, 2, 64, "cpu", fit_quality=True)


def test_mirror_against_the_reference_verifiers():
    g = np.load(GOLDEN)
    th = float(g["th"])
    worst = 0.0

    def check(src, tgt, m, norms, mask):
        nonlocal worst
        rho = residual_norms(src, tgt, m)
        assert np.abs(norms - th).min() > 1e-9                    # the stored inputs keep clear of the threshold
        assert np.array_equal(rho < th, mask)
        M = np.abs(tgt).max(1).astype(np.float64) + abs(m[9]) * np.abs(src).astype(np.float64).sum(1) + np.abs(m[10:13]).max()
        units = np.abs(rho - norms) / (2.0 ** -53 * M)
        worst = max(worst, units.max())
        assert (units <= 16).all(), units.max()
        f = five(rho, th)
        assert f[0] == np.sum(mask) and f[4] == rho.max() and f[3] == np.sort(rho)[[(len(rho) - 1) // 2, len(rho) // 2]].sum() / 2
        return f

    counts = []
    for i in range(int(g["n_single"])):
        f = check(g["s%d_source" % i], g["s%d_target" % i], g["s%d_model" % i], g["s%d_norms" % i], g["s%d_inliers" % i])
        assert f[0] == int(g["s%d_score" % i])
        counts.append(int(f[0]))
    assert counts[7] == 0 and counts[8] == 64 and 0 < counts[6] < 1024
    for i in range(int(g["n_joint"])):
        a, b = g["j%d_parts" % i]
        f0 = check(g["s%d_source" % a], g["s%d_target" % a], g["s%d_model" % a], g["j%d_norms0" % i], g["j%d_inliers0" % i])
        f1 = check(g["s%d_source" % b], g["s%d_target" % b], g["s%d_model" % b], g["j%d_norms1" % i], g["j%d_inliers1" % i])
        # the reference divides by res.shape[0], the 3 rows of its (3, n) residual, not by the points: reproduced, not corrected
        assert (f0[0] / 3 + f1[0] / 3) / 2 == float(g["j%d_score" % i])
    print("fit quality: max |mirror norm - reference norm| = %.3g x 2^-53 M" % worst)


def test_mirror_rows_and_nan_rules():
    """The mirror on a hand-made batch: the layout, the score column's joint, an empty part, a NaN pose, a part beyond the buffer, K = 1."""
    rs = np.random.RandomState(5)
    B, N, K = 2, 50, 3
    P = rs.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    nocs = rs.uniform(0, 1, (B, N, 3 * K)).astype(np.float32)
    mask = rs.uniform(0, 1, (B, N, K)).astype(np.float32)
    mask[0, :, 2] = -1.0                                                # cloud 0: part 2 has no point
    off, src, tgt = partition(P, nocs, mask)
    assert off[-1] == B * N and off[3] == off[2] and src.shape == tgt.shape == (B * N, 3)
    lab = np.argmax(mask[1], 1)
    assert np.array_equal(tgt[off[4]:off[5]], P[1][lab == 1]) and np.array_equal(src[off[4]:off[5]], nocs[1][lab == 1, 3:6])
    rec = rs.normal(size=(B, K, 26))
    rec[1, 0, 20] = np.nan                                              # cloud 1, part 0: the nonlinear pose is poisoned
    best = rs.randint(0, 50, (B * K, 2)).astype(np.int32)
    score = rs.uniform(0, 1, B * (K - 1))
    w = fit_quality_reference(off, src, tgt, rec, 0.1, best, score)
    assert w.shape == (B, K, WIDTH) and np.array_equal(w[:, :, :26].view(np.int64), rec.view(np.int64))
    assert np.array_equal(w[:, :, 26].ravel(), np.diff(off)) and np.array_equal(w[:, :, 27].ravel(), best[:, 1])
    assert np.array_equal(w[:, :, 33], score.reshape(B, K - 1)[:, [0, 0, 1]])
    assert w[0, 2, 26] == 0 and np.isnan(w[0, 2, 28:33]).all() and np.isnan(w[0, 2, 34:39]).all()
    assert np.isfinite(w[1, 0, 28:33]).all() and np.isnan(w[1, 0, 34:39]).all() and np.isfinite(w[1, 1:, 28:39]).all()
    rho = residual_norms(src[off[1]:off[2]], tgt[off[1]:off[2]], rec[0, 1, 13:])
    assert np.array_equal(w[0, 1, 34:39], [np.sum(rho < 0.1), rho.mean(), np.sqrt((rho * rho).mean()), np.median(rho), rho.max()])
    w = fit_quality_reference(off, src, tgt, rec, 0.1)                  # neither winner's score: NaN columns
    assert np.isnan(w[:, :, 27]).all() and np.isnan(w[:, :, 33]).all()
    big = np.zeros((8193, 3), np.float32)
    rec1 = rs.normal(size=(1, 1, 26))
    w = fit_quality_reference(np.array([0, 8193]), big, big, rec1, 0.1, None, None)
    assert w[0, 0, 26] == 8193 and np.isnan(w[0, 0, 27:]).all()         # clamped; K = 1: no score
    w = fit_quality_reference(np.array([0, 8192]), big, big, rec1, 0.1, None, None)
    assert np.isfinite(w[0, 0, 28:33]).all() and np.isfinite(w[0, 0, 34:39]).all() and np.isnan(w[0, 0, 33])


# ---- ShardedPipeline, two gloo ranks, a stand-in per-rank pipeline ------------------------------------------------------------------------
class _FakeWidePipeline(_FakeStreamPipeline):
    """The stand-in stream with 39-wide records: _FakeStreamPipeline's 26 columns, then column c = 1000 * global cloud index + c."""

    def __init__(self, *a, fit_quality=False, **kw):
        assert fit_quality                                              # what ShardedPipeline(fit_quality=True) must pass
        super().__init__(*a, **kw)

    def retire(self, flags=False):
        out = super().retire(flags)
        return out[:2] + (_widen(out[2]),) + out[3:]


def _widen(rec):
    wide = np.zeros(rec.shape[:2] + (WIDTH,))
    wide[:, :, :26] = rec
    wide[:, :, 26:] = 1000 * rec[:, :, :1] + np.arange(26, WIDTH)
    return wide


def _wide_worker(rank, world, port, G, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import articulated_pose_amd  # noqa: F401
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from articulated_pose_amd.dist import ShardedPipeline
    K = 3
    sp = ShardedPipeline(K, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeWidePipeline, raw_capacity=CAP, seed=10, fit_quality=True)
    assert sp.record_width == WIDTH
    calls = []
    real = dist.gather
    dist.gather = lambda *a, **kw: (calls.append(tuple(a[0].shape)), real(*a, **kw))[1]
    try:
        got = list(sp.stream_batches(_batches(G, [G, G - 1, 1, G])))
    finally:
        dist.gather = real
    assert calls == [(sp.n_max, K, WIDTH)] * 4                         # still one gather a batch
    if rank == sp.dst:
        q.put(got)
    else:
        assert all(g[2] is None for g in got)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_stream_gathers_wide_records_in_global_order():
    G, K = 5, 3
    got = _run_ranks(_wide_worker, (G,), world=2)
    batches = _batches(G, [G, G - 1, 1, G])
    assert len(got) == len(batches)
    for k, (item, (clouds, nf, tag)) in enumerate(zip(got, batches)):
        assert item[0] == tag and item[1] == 10 + 2 * k and len(item) == 3
        assert item[2].shape == (len(clouds), K, WIDTH) and item[2].flags.c_contiguous
        np.testing.assert_array_equal(item[2], _widen(_expected(clouds, nf, 10 + 2 * k, K)))
