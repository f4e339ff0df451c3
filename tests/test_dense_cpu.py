"""CPU tests of the per-raw-point labels (no GPU): the ancsh_raw_point_labels entry is declared, exported and bound and refuses bad
arguments before any launch; AncshPipeline / ShardedPipeline refuse dense=True where it cannot run; and ShardedPipeline gathers every raw
row's (label, values) on dst in global cloud order (self-launched gloo ranks, stand-in per-rank pipeline)."""
import ctypes
import datetime
import os

import numpy as np
import pytest
import torch.distributed as dist

from test_dist_cpu import _run_ranks
from test_sharded_stream_cpu import CAP, _batches, _expected, _FakeStreamPipeline

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_dense_entry_is_declared_exported_and_bound():
    import subprocess
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert "ancsh_raw_point_labels" in declared_symbols()
    assert "ancsh_raw_point_labels" in exported and "ancsh_raw_point_labels" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ancsh_raw_point_labels"]) == 16
    assert _lib.lib().ancsh_abi_version() >= 12


def _call(L, B=2, N=1024, K=3, G=9, nchan=4, cap=100, null=None):
    p = dict(rows=P8, offsets=P8, nf=P8, P=P8, W=P8, nocs=P8, gocs=P8, labels=P8, values=P8)
    if null:
        p[null] = None
    return L.ancsh_raw_point_labels(B, N, K, G, nchan, p["rows"], cap, p["offsets"], p["nf"], p["P"], p["W"], p["nocs"], p["gocs"],
                                    p["labels"], p["values"], None)


def test_dense_entry_rejects_bad_arguments_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    for kw, msg in ((dict(B=-1), b"bad shape"), (dict(N=0), b"bad shape"), (dict(B=65536), b"65535"), (dict(K=0, G=3), b"K=0"),
                    (dict(K=9, G=27), b"K=9"), (dict(G=6), b"3 or 3K"), (dict(K=1, G=6), b"3 or 3K"), (dict(nchan=2), b"nchan"),
                    (dict(cap=-1), b"capacity"), (dict(cap=1 << 30), b"capacity")):
        assert _call(L, **kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for name in ("rows", "offsets", "nf", "P", "W", "nocs", "gocs", "labels", "values"):
        assert _call(L, null=name) == -1 and b"null pointer" in L.ancsh_last_error(), name
    assert _call(L, B=0) == 0 and _call(L, cap=0) == 0          # nothing to label: nothing enqueued (P8 never dereferenced)


def test_dense_construction_checks():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    with pytest.raises(ValueError, match="raw_capacity"):          # refused before any device work: "cpu" never reaches a kernel
        AncshPipeline(3, None, None, 2, 512, "cpu", dense=True)
    with pytest.raises(ValueError, match="raw_capacity"):
        ShardedPipeline(3, None, None, 4, 512, "cpu", dense=True)


def test_dense_op_refuses_bad_shapes_without_launching():
    import torch
    from articulated_pose_amd.dataset import raw_point_labels
    with pytest.raises(RuntimeError, match="MI355X"):
        raw_point_labels(np.zeros((8, 4), np.float32), np.array([0, 8], np.int32), np.ones(1, np.float32),
                         torch.zeros((1, 16, 3)), {"W": None, "nocs_per_point": None}, {"gocs_per_point": None})


def _fake_dense(clouds, cloud_base):
    """The stand-in's rows of local clouds: label = global cloud index * 100 + row, values = [x y z, global index, row, -x, 7]."""
    lab, val = [], []
    for j, c in enumerate(clouds):
        g, r = cloud_base + j, np.arange(c.shape[0])
        lab.append((g * 100 + r).astype(np.int32))
        v = np.empty((c.shape[0], 7), np.float32)
        v[:, :3], v[:, 3], v[:, 4], v[:, 5], v[:, 6] = c[:, :3], g, r, -c[:, 0], 7.0
        val.append(v)
    off = np.zeros(len(clouds) + 1, np.int64)
    np.cumsum([c.shape[0] for c in clouds], out=off[1:])
    return np.concatenate(lab), np.concatenate(val), off


class _FakeDensePipeline(_FakeStreamPipeline):
    """The stand-in stream with per-raw-row outputs (_fake_dense of its valid clouds, padding dropped)."""

    def __init__(self, *a, dense=False, **kw):
        assert dense                                              # what ShardedPipeline(dense=True) must pass
        super().__init__(*a, **kw)
        self._rows = []

    def submit(self, clouds, norm_factors, seed=None, tag=None, cloud_base=0):
        super().submit(clouds, norm_factors, seed=seed, tag=tag, cloud_base=cloud_base)
        self._rows.append(_fake_dense([np.asarray(c, np.float32) for c in clouds], cloud_base))

    def retire(self, flags=False, dense=False):
        out = super().retire(flags)
        rows = self._rows.pop(0)
        return out + (rows,) if dense else out

    def stream_batches(self, batches, flags=False, dense=False):
        for k, item in enumerate(batches):
            if len(self._inflight) == len(self.slots):
                yield self.retire(flags, dense)
            self.submit(item[0], item[1], tag=item[2] if len(item) > 2 else k)
        while self._inflight:
            yield self.retire(flags, dense)


def _dense_worker(rank, world, port, G, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import articulated_pose_amd  # noqa: F401
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from articulated_pose_amd.dist import ShardedPipeline
    K = 3
    sp = ShardedPipeline(K, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeDensePipeline, raw_capacity=CAP, seed=10, dense=True)
    calls = []
    real = dist.gather
    dist.gather = lambda *a, **kw: (calls.append(tuple(a[0].shape)), real(*a, **kw))[1]
    try:
        # a full batch, a short one, one cloud (every rank but the first holds none), full again; then with the flag words
        got = list(sp.stream_batches(_batches(G, [G, G - 1, 1, G]), dense=True))
        got += list(sp.stream_batches(_batches(G, [G, 2], seed=1), flags=True, dense=True))
    finally:
        dist.gather = real
    assert len(calls) == 2 * 4 + 3 * 2                          # records + dense rows per batch (flags add their own gather)
    assert all(c == (sp.n_max, K, 26) for c in calls[0:8:2]) and all(len(c) == 2 and c[1] == 8 for c in calls[1:8:2])
    if rank == sp.dst:
        q.put(got)
    else:
        assert all(g[2] is None and g[-1] is None for g in got)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,G", [(2, 5), (2, 6), (3, 4)])
def test_sharded_stream_gathers_dense_rows_in_global_order(world, G):
    got = _run_ranks(_dense_worker, (G,), world=world)
    K = 3
    batches = _batches(G, [G, G - 1, 1, G]) + _batches(G, [G, 2], seed=1)
    assert len(got) == len(batches)
    for k, (item, (clouds, nf, tag)) in enumerate(zip(got, batches)):
        seed = 10 + 2 * k
        assert item[0] == tag and item[1] == seed and len(item) == (5 if k >= 4 else 4)
        np.testing.assert_array_equal(item[2], _expected(clouds, nf, seed, K))
        labels, values, off = item[-1]
        want = _fake_dense(clouds, 0)
        assert labels.dtype == np.int32 and values.dtype == np.float32 and off.dtype == np.int64
        assert labels.flags.c_contiguous and values.flags.c_contiguous
        np.testing.assert_array_equal(off, want[2])
        np.testing.assert_array_equal(labels, want[0])
        assert np.array_equal(values.view(np.int32), want[1].view(np.int32))
        if k >= 4:
            np.testing.assert_array_equal(item[3], np.arange(len(clouds)) + 1)


def test_dense_refused_on_a_pipeline_built_without_it_and_world_one_passes_through():
    from articulated_pose_amd.dist import ShardedPipeline
    sp = ShardedPipeline(3, None, None, 4, 8, "cpu", slots=2, pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP)
    with pytest.raises(RuntimeError, match="dense=True"):
        sp.retire(dense=True)
    with pytest.raises(RuntimeError, match="dense=True"):
        next(sp.stream_batches(_batches(4, [4]), dense=True))
    G = 5
    sp = ShardedPipeline(3, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeDensePipeline, raw_capacity=CAP, dense=True)
    assert sp.world == 1 and isinstance(sp.pipe, _FakeDensePipeline)
    batches = _batches(G, [G, 3, 1])
    for item, (clouds, _, _) in zip(sp.stream_batches(batches, dense=True), batches):
        for a, b in zip(item[-1], _fake_dense(clouds, 0)):
            np.testing.assert_array_equal(a, b)
