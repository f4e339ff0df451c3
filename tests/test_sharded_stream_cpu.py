"""CPU tests of the sharded stream (no GPU): the key block's C entries and host checks, and dist.ShardedPipeline.submit / retire /
stream_batches over self-launched gloo ranks with a stand-in per-rank pipeline -- the split of every global batch, the validation that
raises on every rank, the gather of records in global cloud order on dst, and the world-1 pass-through."""
import collections
import datetime
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_dist_cpu import _run_ranks

NEW_SYMBOLS = ("ancsh_input_sample_stream_keyed", "ancsh_ransac_single_rec_dkey", "ancsh_ransac_joint_rec_dkey")


def test_key_entries_are_bound_and_exported():
    import ctypes
    import subprocess
    from articulated_pose_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in exported, name
    L = _lib.lib()
    assert L.ancsh_abi_version() >= 10
    # the _dkey entries take the _dseed entries' arguments with the key block's address in place of the seed's
    assert _lib.SIGNATURES["ancsh_ransac_single_rec_dkey"] == _lib.SIGNATURES["ancsh_ransac_single_rec_dseed"]
    assert _lib.SIGNATURES["ancsh_ransac_joint_rec_dkey"] == _lib.SIGNATURES["ancsh_ransac_joint_rec_dseed"]
    assert _lib.SIGNATURES["ancsh_input_sample_stream_keyed"] == _lib.SIGNATURES["ancsh_input_sample_stream"]
    assert isinstance(L.ancsh_ransac_single_rec_dkey, ctypes._CFuncPtr)


def test_key_entries_refuse_bad_arguments_before_launch():
    """The checks run before any launch: a NULL key block, and a problem count that is not whole clouds (K is the problem count of one
    cloud in the key's problem base, so the _dkey entries need it even without a record)."""
    from articulated_pose_amd import _lib
    L = _lib.lib()
    p = 256                                   # a non-null address that is never dereferenced: every call below is refused first
    assert L.ancsh_input_sample_stream_keyed(2, 64, 4, p, 100, p, p, 3, None, p, p, None, None) == -1
    assert b"null key" in L.ancsh_last_error()
    single = lambda nprob, key, K: L.ancsh_ransac_single_rec_dkey(nprob, p, p, p, 0.1, 8, None, key, 16, p, p, p, p, None, 64, None, K,
                                                                  None, 0.0, None)
    joint = lambda nprob, key, K: L.ancsh_ransac_joint_rec_dkey(nprob, p, p, p, p, p, 0.1, 8, None, key, 16, p, p, p, p, p, p, None, 0,
                                                                None, K, None, 0.0, None)
    assert single(6, None, 3) == -1 and b"null key" in L.ancsh_last_error()
    assert joint(4, None, 3) == -1 and b"null key" in L.ancsh_last_error()
    assert single(7, p, 3) == -1 and b"multiple of K" in L.ancsh_last_error()
    assert single(6, p, 0) == -1
    assert single(1 << 20, p, 1) == -1
    assert joint(5, p, 3) == -1 and b"multiple of K - 1" in L.ancsh_last_error()
    assert joint(4, p, 1) == -1


def test_key_block_layout_and_bounds():
    from articulated_pose_amd.dataset import STREAM_KEY_PROBLEMS, check_stream_key, stream_key_words
    w = stream_key_words(2 ** 64 - 3, 17)
    assert w.dtype == np.int32 and w.shape == (4,) and w.nbytes == 16
    assert int(w[:2].view(np.uint64)[0]) == 2 ** 64 - 3 and w[2] == 17 and w[3] == 0
    assert check_stream_key(0, 32, 4) == 0
    K, B = 4, 32
    last = STREAM_KEY_PROBLEMS // K - B - 1                 # (base + B) * K = 2^20 - K: the largest base that keeps the tag bits clear
    assert check_stream_key(last, B, K) == last
    for bad in (last + 1, -1):
        with pytest.raises(ValueError):
            check_stream_key(bad, B, K)


def test_keyed_needs_streaming():
    from articulated_pose_amd.pipeline import AncshPipeline
    with pytest.raises(ValueError, match="raw_capacity"):
        AncshPipeline(3, None, None, 4, 64, "cpu", keyed=True)


class _FakeStreamPipeline(object):
    """AncshPipeline's streaming interface on CPU (submit / retire / stream_batches, with its checks): the 'record' of local cloud j is
    [global index cloud_base + j, seed, first x of the cloud, its norm factor] in columns 0..3, its flag word is global index + 1."""

    def __init__(self, K, wa, wn, n_local, N, device, slots=1, raw_capacity=None, keyed=False, seed=0):
        assert raw_capacity is not None and keyed           # what ShardedPipeline(raw_capacity=...) must pass
        self.K, self.B, self.raw_capacity, self.seed = K, n_local, raw_capacity, seed
        self.slots = [object() for _ in range(slots)]
        self._inflight, self._submitted = collections.deque(), 0

    def submit(self, clouds, norm_factors, seed=None, tag=None, cloud_base=0):
        from articulated_pose_amd.dataset import check_raw_clouds, check_stream_key
        cloud_base = check_stream_key(cloud_base, self.B, self.K)
        clouds, nf = check_raw_clouds(clouds, norm_factors, self.B)
        if sum(c.shape[0] for c in clouds) + (self.B - len(clouds)) * clouds[0].shape[0] > self.raw_capacity:
            raise ValueError("raw_capacity")
        if len(self._inflight) == len(self.slots):
            raise RuntimeError("all slots hold unretired batches")
        seed = self.seed + 2 * self._submitted if seed is None else int(seed)
        g = cloud_base + np.arange(len(clouds))
        rec = np.zeros((len(clouds), self.K, 26))
        rec[:, :, 0], rec[:, :, 1] = g[:, None], seed
        rec[:, :, 2], rec[:, :, 3] = np.array([c[0, 0] for c in clouds])[:, None], nf[:, None]
        self._inflight.append((tag, seed, rec, (g + 1).astype(np.int32)))
        self._submitted += 1

    def retire(self, flags=False):
        if not self._inflight:
            raise RuntimeError("retire(): no batch in flight")
        tag, seed, rec, words = self._inflight.popleft()
        return (tag, seed, rec, words) if flags else (tag, seed, rec)

    def stream_batches(self, batches, flags=False):
        for k, item in enumerate(batches):
            if len(self._inflight) == len(self.slots):
                yield self.retire(flags)
            self.submit(item[0], item[1], tag=item[2] if len(item) > 2 else k)
        while self._inflight:
            yield self.retire(flags)


def _expected(clouds, nf, seed, K):
    n = len(clouds)
    rec = np.zeros((n, K, 26))
    rec[:, :, 0], rec[:, :, 1] = np.arange(n)[:, None], seed
    rec[:, :, 2], rec[:, :, 3] = np.array([c[0, 0] for c in clouds], np.float32)[:, None], np.asarray(nf, np.float32)[:, None]
    return rec


def _batches(G, sizes, seed=0):
    """One global batch per entry of `sizes` (its clouds), ragged raw clouds with distinct first x values."""
    rs = np.random.RandomState(seed)
    out = []
    for k, n in enumerate(sizes):
        clouds = [rs.uniform(-1, 1, (int(rs.randint(3, 40)), 4)).astype(np.float32) for _ in range(n)]
        for i, c in enumerate(clouds):
            c[0, 0] = 1000 * k + i
        out.append((clouds, rs.uniform(0.5, 2.0, n).astype(np.float32), "b%d" % k))
    return out


CAP = 200        # raw rows per rank: every shard of _batches fits (<= 4 clouds of < 40 rows, plus padding)


def _stream_worker(rank, world, port, G, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import articulated_pose_amd  # noqa: F401
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from articulated_pose_amd.dist import ShardedPipeline, balanced_range
    K, seed0 = 3, 10
    sp = ShardedPipeline(K, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP, seed=seed0)
    assert sp.pipe.B == sp.hi - sp.lo and sp.pipe.raw_capacity == CAP
    # an even batch, a ragged one, one shorter than the world (trailing ranks hold nothing), full ones
    sizes = [G, G - 1, 1, G, world - 1 if world > 2 else 1, G, 2, G]
    batches = _batches(G, sizes)
    lo1 = balanced_range(G, world, 1)[0]
    bad = 4                                                  # its cloud lo1 (rank 1's first) is empty: every rank must refuse the batch
    batches[bad] = (list(batches[bad - 1][0]), batches[bad - 1][1], "bad")
    batches[bad][0][lo1] = np.zeros((0, 4), np.float32)
    got, errors = [], []
    gen = sp.stream_batches(batches)
    try:
        for item in gen:
            got.append(item)
    except ValueError as e:
        errors.append(str(e))
    assert len(errors) == 1 and "cloud %d" % lo1 in errors[0]         # raised here, on every rank, before any collective
    got += list(sp.stream_batches(batches[bad + 1:]))                  # the stream goes on: the batches in flight come first
    ok = [b for b in batches if b[2] != "bad"]
    assert [g[0] for g in got] == [b[2] for b in ok]
    assert [g[1] for g in got] == [seed0 + 2 * k for k in range(len(ok))]
    # a shard beyond rank 1's raw_capacity: ValueError on every rank too; so is a full in-flight window (RuntimeError)
    big = [np.ones((3, 4), np.float32) for _ in range(G)]
    big[lo1] = np.ones((CAP + 1, 4), np.float32)
    try:
        sp.submit(big, np.ones(G, np.float32))
        raise AssertionError("not refused")
    except ValueError as e:
        assert "rank 1's shard" in str(e)
    extra = _batches(G, [G, 1, G], seed=1)
    for clouds, nf, tag in extra[:2]:
        sp.submit(clouds, nf, tag=tag)
    try:
        sp.submit(*extra[2][:2])
        raise AssertionError("not refused")
    except RuntimeError:
        pass
    direct = [sp.retire(flags=True), sp.retire(flags=True)]
    try:
        sp.retire()
        raise AssertionError("not refused")
    except RuntimeError:
        pass
    if rank == sp.dst:
        q.put(([(t, s, r) for t, s, r in got], [(t, s, r, w) for t, s, r, w in direct]))
    else:
        assert all(r is None for _, _, r in got) and all(r is None and w is None for _, _, r, w in direct)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,G", [(2, 6), (2, 7), (3, 7)])
def test_sharded_stream_gathers_global_order(world, G):
    """Two / three gloo ranks stream the same global batches: dst receives every batch's records in global cloud order with its tag
    and seed (seed + 2k, k counting accepted batches), whatever the split -- even, ragged, or short enough to leave ranks empty."""
    got, direct = _run_ranks(_stream_worker, (G,), world=world)
    K, seed0 = 3, 10
    sizes = [G, G - 1, 1, G, world - 1 if world > 2 else 1, G, 2, G]
    batches = [b for k, b in enumerate(_batches(G, sizes)) if k != 4]
    assert len(got) == len(batches)
    for k, ((tag, seed, rec), (clouds, nf, want_tag)) in enumerate(zip(got, batches)):
        assert tag == want_tag and seed == seed0 + 2 * k
        assert rec.shape == (len(clouds), K, 26) and rec.dtype == np.float64
        np.testing.assert_array_equal(rec, _expected(clouds, nf, seed, K))
    extra = _batches(G, [G, 1, G], seed=1)
    for j, (tag, seed, rec, words) in enumerate(direct):
        clouds, nf, want_tag = extra[j]
        assert tag == want_tag and seed == seed0 + 2 * (len(batches) + j)
        np.testing.assert_array_equal(rec, _expected(clouds, nf, seed, K))
        np.testing.assert_array_equal(words, np.arange(len(clouds)) + 1)


def test_sharded_stream_without_a_group_is_the_local_stream():
    from articulated_pose_amd.dist import ShardedPipeline
    G, K = 5, 2
    sp = ShardedPipeline(K, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP, seed=3)
    assert (sp.world, sp.lo, sp.hi) == (1, 0, G) and isinstance(sp.pipe, _FakeStreamPipeline)
    batches = _batches(G, [G, 3, 1, G, 2])
    ref = _FakeStreamPipeline(K, None, None, G, 8, "cpu", slots=2, raw_capacity=CAP, keyed=True, seed=3)
    for flags in (False, True):
        a, b = list(sp.stream_batches(batches, flags)), list(ref.stream_batches(batches, flags))
        assert len(a) == len(b) == len(batches)
        for x, y in zip(a, b):
            assert x[:2] == y[:2] and all(np.array_equal(u, v) for u, v in zip(x[2:], y[2:]))
    with pytest.raises(RuntimeError):
        ShardedPipeline(K, None, None, G, 8, "cpu", pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP).retire()
