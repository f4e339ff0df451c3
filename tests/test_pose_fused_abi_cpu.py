"""CPU tests (no GPU) of the whole-fit entries (ancsh_pose_fit_rec and its _dseed / _dkey / _kind forms, include/ancsh_hip.h): the
symbols and signatures, and the host-side argument checks of BOTH stages -- null pointers, the record's geometry, the tie windows,
lm_schedule, the key pointers -- which all run before anything is launched, so they can be called without a device."""
import ctypes

import pytest

NAMES = ("ancsh_pose_fit_rec", "ancsh_pose_fit_rec_dseed", "ancsh_pose_fit_rec_dkey")
P8 = ctypes.c_void_p(8)
REC = ctypes.c_void_p(64)


def _L():
    from articulated_pose_amd import _lib
    return _lib.lib()


def _args(key, kind=False, **kw):
    """a call's arguments: every pointer the non-NULL dummy 8 (never dereferenced: the checks fail first), overridable by name"""
    a = dict(nprob_a=6, off=P8, src=P8, tgt=P8, inlier_th_a=0.1, niter_a=8, draws_a=None, key_a=key, max_n=16, out_model_a=P8, out_inliers_a=P8,
             out_best_a=P8, scratch_scores_a=P8, scratch_quads=None, rows=0, tie_stats_a=None, tie_window_a=0.0, nprob_b=4, rng0=P8, rng1=P8,
             joint_dir=P8, inlier_th_b=0.1, niter_b=8, draws_b=None, key_b=key, out_model_b=P8, out_inliers_b=P8, out_best_b=P8, out_score_b=P8,
             scratch_scores_b=P8, scratch_models_b=P8, lm_stat=None, lm_schedule=0, tie_stats_b=None, tie_window_b=0.0, record=None, K=3)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return list(a.values()) + ([None] if kind else []) + [None]


def _keys(name):
    return 0 if name in ("ancsh_pose_fit_rec", "ancsh_pose_fit_rec_kind") else P8


def test_symbols_and_signatures():
    from articulated_pose_amd import _lib
    L = _L()
    for n in NAMES:
        for sfx in ("", "_kind"):
            assert isinstance(getattr(L, n + sfx), ctypes._CFuncPtr)
            assert len(_lib.SIGNATURES[n + sfx]) == len(_args(0, kind=bool(sfx)))
        assert _lib.SIGNATURES[n + "_kind"] == _lib.SIGNATURES[n][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["ancsh_pose_fit_rec_dkey"] == _lib.SIGNATURES["ancsh_pose_fit_rec_dseed"]
    # the union of the two entries' arguments: src / tgt / max_n / record / K once
    assert len(_lib.SIGNATURES["ancsh_pose_fit_rec"]) == len(_lib.SIGNATURES["ancsh_ransac_single_rec"]) + len(_lib.SIGNATURES["ancsh_ransac_joint_rec"]) - 6


@pytest.mark.parametrize("name", [n + s for n in NAMES for s in ("", "_kind")])
def test_both_stages_checks_run_before_any_launch(name):
    L = _L()
    fn, key, kind = getattr(L, name), _keys(name), name.endswith("_kind")
    bad = lambda msg, **kw: fn(*_args(key, kind, **kw)) == -1 and msg in L.ancsh_last_error()
    # null pointers of either stage
    for p in ("off", "src", "tgt", "out_model_a", "out_inliers_a", "out_best_a", "scratch_scores_a"):
        assert bad(b"ransac_single: null pointer", **{p: None}), p
    for p in ("rng0", "rng1", "joint_dir", "out_model_b", "out_inliers_b", "out_best_b", "out_score_b", "scratch_scores_b", "scratch_models_b"):
        assert bad(b"ransac_joint: null pointer", **{p: None}), p
    # sizes, thresholds, the LDS bounds of both refits
    assert bad(b"ransac_single: bad sizes", niter_a=0) and bad(b"ransac_joint: bad sizes", niter_b=0) and bad(b"bad sizes", max_n=0)
    assert bad(b"nprob_a" if "dkey" in name else b"ransac_single: bad sizes", nprob_a=-3)          # the key block's own count check comes first
    assert bad(b"inlier_th must be positive", inlier_th_a=0.0) and bad(b"inlier_th must be positive", inlier_th_b=-1.0)
    assert bad(b"max_n 4000 > 3072", max_n=4000) and bad(b"max_n 7000 > 6144", max_n=7000)
    assert bad(b"32-byte aligned", scratch_quads=P8)
    # lm_schedule
    assert bad(b"unknown lm_schedule 3", lm_schedule=3) and bad(b"unknown lm_schedule -1", lm_schedule=-1)
    # the record's geometry: nprob_a a multiple of K, nprob_b of K - 1
    geometry = b"must be a multiple of K" if "dkey" in name else b"record needs"              # the key block's count check says the same, first
    assert bad(geometry, record=REC, nprob_a=5) and bad(geometry, record=REC, nprob_b=3)
    # the tie windows of both stages
    assert bad(b"tie_window", tie_stats_a=P8, tie_window_a=0.2) and bad(b"tie_window", tie_stats_b=P8, tie_window_b=-1.0)
    # the eight-lane schedule is accepted as far as the checks go: the next failure is a later one
    assert bad(b"ransac_joint: null pointer", lm_schedule=2, rng0=None)


@pytest.mark.parametrize("name", ["ancsh_pose_fit_rec_dseed", "ancsh_pose_fit_rec_dkey", "ancsh_pose_fit_rec_dseed_kind", "ancsh_pose_fit_rec_dkey_kind"])
def test_device_key_pointers_are_required(name):
    L = _L()
    fn, kind = getattr(L, name), name.endswith("_kind")
    what = b"null key pointer" if "dkey" in name else b"null seed pointer"
    assert fn(*_args(P8, kind, key_a=None)) == -1 and what in L.ancsh_last_error()
    assert fn(*_args(P8, kind, key_b=None)) == -1 and what in L.ancsh_last_error()
    if "dkey" in name:          # the key block needs the problem counts of one cloud, with or without a record
        assert fn(*_args(P8, kind, nprob_a=5)) == -1 and b"multiple of K" in L.ancsh_last_error()
        assert fn(*_args(P8, kind, nprob_b=3)) == -1 and b"multiple of K - 1" in L.ancsh_last_error()


@pytest.mark.parametrize("name", [n + s for n in NAMES for s in ("", "_kind")])
def test_empty_problems_return_ok_before_any_launch(name):
    L = _L()
    fn, key, kind = getattr(L, name), _keys(name), name.endswith("_kind")
    nothing = {k: None for k in ("off", "src", "tgt", "out_model_a", "out_inliers_a", "out_best_a", "scratch_scores_a", "rng0", "rng1", "joint_dir",
                                 "out_model_b", "out_inliers_b", "out_best_b", "out_score_b", "scratch_scores_b", "scratch_models_b")}
    assert fn(*_args(key, kind, nprob_a=0, nprob_b=0, **nothing)) == 0
    assert fn(*_args(key, kind, nprob_a=0, nprob_b=0, record=REC, K=1, **nothing)) == 0          # a K = 1 caller's record is not held to K >= 2
    # ... but the sizes and the schedule are still examined
    assert fn(*_args(key, kind, nprob_a=0, nprob_b=0, lm_schedule=9, **nothing)) == -1 and b"lm_schedule" in L.ancsh_last_error()
    assert fn(*_args(key, kind, nprob_a=0, nprob_b=0, niter_a=0, **nothing)) == -1 and b"bad sizes" in L.ancsh_last_error()
