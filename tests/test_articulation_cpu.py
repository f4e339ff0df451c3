"""CPU tests of the streamed articulation block (no GPU): the ancsh_articulation_rec entry is declared, exported and bound and refuses bad
arguments before any launch; AncshPipeline / ShardedPipeline refuse articulation=True where it cannot run; and ShardedPipeline packs the
record and the block into ONE gather per batch and splits them back on dst in global cloud order (self-launched gloo ranks, stand-in
per-rank pipeline)."""
import ctypes
import datetime
import os

import numpy as np
import pytest
import torch.distributed as dist

from test_dist_cpu import _run_ranks
from test_sharded_stream_cpu import CAP, _batches, _expected, _FakeStreamPipeline

P8 = ctypes.c_void_p(8)       # a non-null pointer that is never dereferenced: every call below fails its checks first


def test_articulation_entry_is_declared_exported_and_bound():
    import subprocess
    from articulated_pose_amd import _lib
    from test_abi_cpu import declared_symbols
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert "ancsh_articulation_rec" in declared_symbols()
    assert "ancsh_articulation_rec" in exported and "ancsh_articulation_rec" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ancsh_articulation_rec"]) == 20
    assert _lib.lib().ancsh_abi_version() >= 11


def _call(L, b=2, n=512, K=3, G=9, JC=3, null=None, **over):
    ptrs = dict(gocs=P8, nocs=P8, mask=P8, heatmap=P8, unitvec=P8, axis=P8, index=P8, npcs_nocs=P8, npcs_mask=P8, record=P8, art=P8)
    if null:
        ptrs[null] = None
    p = ptrs
    return L.ancsh_articulation_rec(b, n, K, G, JC, p["gocs"], p["nocs"], p["mask"], p["heatmap"], p["unitvec"], p["axis"], p["index"],
                                    p["npcs_nocs"], p["npcs_mask"], p["record"], p["art"], None, None, None, None)


def test_articulation_entry_rejects_bad_arguments_before_launch():
    from articulated_pose_amd import _lib
    L = _lib.lib()
    for kw, msg in ((dict(b=-1), b"bad sizes"), (dict(n=0), b"bad sizes"), (dict(K=0, G=3), b"bad sizes"), (dict(K=9, G=27), b"K <= 8"),
                    (dict(G=5), b"3 or 3K"), (dict(JC=0), b"joint_channels"), (dict(JC=9), b"joint_channels"),
                    (dict(n=4097), b"LDS")):
        assert _call(L, **kw) == -1, kw
        assert msg in L.ancsh_last_error(), (kw, L.ancsh_last_error())
    for name in ("gocs", "nocs", "mask", "heatmap", "unitvec", "axis", "index", "npcs_nocs", "npcs_mask", "record", "art"):
        assert _call(L, null=name) == -1 and b"null pointer" in L.ancsh_last_error(), name
    assert _call(L, b=0, null="art") == 0                       # an empty batch enqueues nothing
    assert _call(L, n=4096, null="art") == -1 and b"null pointer" in L.ancsh_last_error()      # the LDS bound admits 4096


def test_articulation_construction_checks():
    from articulated_pose_amd.dist import ShardedPipeline
    from articulated_pose_amd.pipeline import AncshPipeline
    with pytest.raises(ValueError, match="couple=True"):
        AncshPipeline(3, None, None, 2, 512, "cpu", couple=False, articulation=True)
    with pytest.raises(ValueError, match="num_points"):
        AncshPipeline(3, None, None, 2, 4097, "cpu", articulation=True)
    with pytest.raises(ValueError, match="raw_capacity"):
        ShardedPipeline(3, None, None, 4, 512, "cpu", articulation=True)


class _FakeArticulationPipeline(_FakeStreamPipeline):
    """The stand-in stream with an articulation block: block of local cloud j = [global index, seed, -(first x)] in columns 0..2, 7 elsewhere."""

    def __init__(self, *a, articulation=False, **kw):
        assert articulation                                        # what ShardedPipeline(articulation=True) must pass
        super().__init__(*a, **kw)

    def retire(self, flags=False, articulation=False):
        out = super().retire(flags)
        if not articulation:
            return out
        rec = out[2]
        art = np.full(rec.shape[:2] + (12,), 7.0)
        art[:, :, 0], art[:, :, 1], art[:, :, 2] = rec[:, :, 0], rec[:, :, 1], -rec[:, :, 2]
        return out + (art,)


def _expected_art(clouds, seed, K):
    rec = _expected(clouds, np.ones(len(clouds)), seed, K)
    art = np.full((len(clouds), K, 12), 7.0)
    art[:, :, 0], art[:, :, 1], art[:, :, 2] = rec[:, :, 0], rec[:, :, 1], -rec[:, :, 2]
    return art


def _art_worker(rank, world, port, G, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import articulated_pose_amd  # noqa: F401
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from articulated_pose_amd.dist import ShardedPipeline
    K = 3
    sp = ShardedPipeline(K, None, None, G, 8, "cpu", slots=2, pipeline_factory=_FakeArticulationPipeline, raw_capacity=CAP, seed=10,
                         articulation=True)
    calls = []
    real = dist.gather
    dist.gather = lambda *a, **kw: (calls.append(tuple(a[0].shape)), real(*a, **kw))[1]
    try:
        got = list(sp.stream_batches(_batches(G, [G, G - 1, 1, G]), articulation=True))
        got += list(sp.stream_batches(_batches(G, [G, 2], seed=1), flags=True, articulation=True))
    finally:
        dist.gather = real
    assert calls[:4] == [(sp.n_max, K, 38)] * 4                # one packed gather per batch (flags add their own, as before)
    if rank == sp.dst:
        q.put(got)
    else:
        assert all(g[2] is None and g[-1] is None for g in got)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,G", [(2, 5), (2, 6)])
def test_sharded_stream_packs_and_splits_the_block(world, G):
    got = _run_ranks(_art_worker, (G,), world=world)
    K = 3
    batches = _batches(G, [G, G - 1, 1, G]) + _batches(G, [G, 2], seed=1)
    assert len(got) == len(batches)
    for k, (item, (clouds, nf, tag)) in enumerate(zip(got, batches)):
        seed = 10 + 2 * k
        assert item[0] == tag and item[1] == seed and len(item) == (5 if k >= 4 else 4)
        rec, art = item[2], item[-1]
        assert rec.shape == (len(clouds), K, 26) and art.shape == (len(clouds), K, 12) and rec.flags.c_contiguous and art.flags.c_contiguous
        np.testing.assert_array_equal(rec, _expected(clouds, nf, seed, K))
        np.testing.assert_array_equal(art, _expected_art(clouds, seed, K))
        if k >= 4:
            np.testing.assert_array_equal(item[3], np.arange(len(clouds)) + 1)


def test_articulation_refused_on_a_pipeline_built_without_it():
    from articulated_pose_amd.dist import ShardedPipeline
    sp = ShardedPipeline(3, None, None, 4, 8, "cpu", slots=2, pipeline_factory=_FakeStreamPipeline, raw_capacity=CAP)
    with pytest.raises(RuntimeError, match="articulation=True"):
        sp.retire(articulation=True)
    with pytest.raises(RuntimeError, match="articulation=True"):
        next(sp.stream_batches(_batches(4, [4]), articulation=True))
