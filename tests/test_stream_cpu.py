"""Streaming pipeline, host side (no GPU): the new ABI entries refuse bad arguments before any launch, and the numpy mirror of the
sampler's keyed bijection (tests/stream_mirror.py, include/ancsh_hip.h) is a permutation that respects the tiling rule."""
import ctypes

import numpy as np

from stream_mirror import permutation, sample_perm, tiled_size

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


def _sample(L, nclouds=2, nchan=4, jcls_col=3, seed=P8):
    return L.ancsh_input_sample_stream(nclouds, 16, nchan, P8, 100, P8, P8, jcls_col, seed, P8, P8, None, None)


def test_stream_entries_reject_bad_arguments_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    assert L.ancsh_abi_version() >= 8
    assert _sample(L, nchan=3) == -1 and b"nchan=3" in L.ancsh_last_error()
    for col in (2, 4, -1):
        assert _sample(L, jcls_col=col) == -1 and b"jcls_col" in L.ancsh_last_error()
    assert _sample(L, seed=None) == -1 and b"null seed" in L.ancsh_last_error()
    assert _sample(L, nclouds=65536) == -1 and b"65535" in L.ancsh_last_error()
    assert L.ancsh_input_sample_stream(2, 16, 4, None, 100, P8, P8, 3, P8, P8, P8, None, None) == -1
    assert L.ancsh_input_sample_stream(2, 16, 4, P8, -1, P8, P8, 3, P8, P8, P8, None, None) == -1 and b"capacity" in L.ancsh_last_error()
    assert L.ancsh_ransac_single_rec_dseed(2, P8, P8, P8, 0.1, 10, None, None, 100, P8, P8, P8, P8, P8, 100, None, 0, None, 0.0,
                                           None) == -1 and b"null seed" in L.ancsh_last_error()
    assert L.ancsh_ransac_joint_rec_dseed(2, P8, P8, P8, P8, P8, 0.1, 10, None, None, 100, P8, P8, P8, P8, P8, P8, None, 0, None, 0,
                                          None, 0.0, None) == -1 and b"null seed" in L.ancsh_last_error()


def test_bijection_mirror_is_a_permutation_of_the_tiled_cloud():
    for T in range(1, 4097):
        p = permutation(T * 7919, T % 5, T)
        assert np.array_equal(np.sort(p), np.arange(T)), T


def test_first_rows_respect_the_tiling_rule():
    for N in (1, 5, 512, 1024):
        for n_raw in sorted({1, 2, 7, 100, N - 1, N, N + 1, 3 * N} - {0}):
            T = tiled_size(n_raw, N)
            assert T >= N and T % n_raw == 0
            for seed in (0, 1, 2 ** 64 - 1):
                p = sample_perm(seed, 3, n_raw, N)
                assert len(np.unique(p)) == N and p.min() >= 0 and p.max() < T
                assert np.bincount(p % n_raw, minlength=n_raw).max() <= N // n_raw + 1


def test_keys_depend_on_seed_and_cloud():
    a, b, c = sample_perm(0, 0, 3000, 1024), sample_perm(1, 0, 3000, 1024), sample_perm(0, 1, 3000, 1024)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_streaming_pipeline_argument_errors_need_no_gpu():
    import pytest
    from articulated_pose_amd.dataset import check_raw_clouds
    ok = np.zeros((10, 4), np.float32)
    with pytest.raises(ValueError):
        check_raw_clouds([np.zeros((0, 4), np.float32)], [1.0])
    with pytest.raises(ValueError):
        check_raw_clouds([np.zeros((10, 18), np.float32)], [1.0])
    with pytest.raises(ValueError):
        check_raw_clouds([ok], [float("nan")])
    with pytest.raises(ValueError):
        check_raw_clouds([ok] * 3, [1.0] * 3, max_clouds=2)
    with pytest.raises(ValueError):
        check_raw_clouds([], [])
    clouds, nf = check_raw_clouds([ok, ok.astype(np.float64)], [1.0, 2.0])
    assert all(c.dtype == np.float32 for c in clouds) and nf.tolist() == [1.0, 2.0]
