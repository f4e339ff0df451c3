"""F16x2 range guard on the MI355X: the guarded kernels compute the unguarded kernels' outputs bit for bit and flag exactly the (cloud,
network) pairs with a converted activation beyond +-65504; AncshPipeline(arithmetic="f16x2", range_guard=True) refits flagged clouds in
f32, in the streaming and the step() paths; the arithmetic goes down the layers explicitly, not through the module globals."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import passthrough_pose_problem

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
ABOVE = float(np.nextafter(np.float32(F16_MAX), np.float32(np.inf)))


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---- kernel level: every guarded entry point against its unguarded form ----------------------------------------------------------
class _Layers(object):
    """F16x2-packed (k, n) layers with zero kernels: every epilogue value is relu(bias * scale + shift) = `bias` (scale 1, shift 0), so a
    chosen value reaches every hidden layer's split; the inputs' own split sites see the inputs."""

    def __init__(self, dev, shapes, bias=0.0):
        from articulated_pose_amd import pointnet_util
        self.keep, self.ptrs = [], []
        for k, n in shapes:
            w = pointnet_util._split_pack(torch.zeros((k, n), dtype=torch.float32, device=dev), "f16x2")
            b = torch.full((n,), bias, dtype=torch.float32, device=dev)
            s = torch.ones((n,), dtype=torch.float32, device=dev)
            h = torch.zeros((n,), dtype=torch.float32, device=dev)
            self.keep += [w, b, s, h]
            self.ptrs += [w.data_ptr(), b.data_ptr(), s.data_ptr(), h.data_ptr()]

    def table(self, ngroups):
        t = (ctypes.c_void_p * (len(self.ptrs) * ngroups))(*(self.ptrs * ngroups))
        self.keep.append(t)
        return ctypes.cast(t, ctypes.c_void_p)


def _run_entry(dev, name, B, value, where, cloud, bias=0.0):
    """Launch entry `name` (ngroups = 2) unguarded and guarded on the same inputs, with `value` planted at the input site (where="input")
    of cloud `cloud`, or as every hidden layer's epilogue value (where="epilogue": every cloud).  -> (unguarded out, guarded out, flags)."""
    from articulated_pose_amd import _lib
    f = dict(dtype=torch.float32, device=dev)
    G = 2
    rs = np.random.RandomState(5)
    if where == "epilogue":
        bias = value
    outs = []
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    if name == "sa":
        n, m = 1024, 512
        xyz = torch.from_numpy(rs.uniform(-0.5, 0.5, (B, n, 3)).astype(np.float32)).to(dev)
        if where == "input":
            xyz[cloud, 0, 0] = value                               # every neighbourhood of the cloud reads source point 0
        new_xyz = torch.zeros((B, m, 3), **f)
        idx = torch.zeros((B, m, 64), dtype=torch.int32, device=dev)
        L = _Layers(dev, [(3, 64), (64, 64), (64, 128)], bias)
        args = lambda out: (G, B, n, m, 64, 0, 64, 64, 128, _lib.ptr(xyz), None, _lib.ptr(new_xyz), _lib.ptr(idx), L.table(G), _lib.ptr(out))
        shape = (G * B, m, 128)
        entry = "ancsh_sa_module_fused_f16x2_grouped"
    elif name == "sa_partial":
        n, m = 512, 128
        xyz = torch.from_numpy(rs.uniform(-0.5, 0.5, (B, n, 3)).astype(np.float32)).to(dev)
        if where == "input":
            xyz[cloud, 0, 1] = value
        partial = torch.zeros((G * B, n, 128), **f)
        new_xyz = torch.zeros((B, m, 3), **f)
        idx = torch.zeros((B, m, 64), dtype=torch.int32, device=dev)
        L = _Layers(dev, [(3, 128), (128, 128), (128, 256)], bias)
        args = lambda out: (G, B, n, m, 64, 128, 128, 256, _lib.ptr(xyz), _lib.ptr(partial), _lib.ptr(new_xyz), _lib.ptr(idx), L.table(G),
                            _lib.ptr(out))
        shape = (G * B, m, 256)
        entry = "ancsh_sa_module_fused_partial_f16x2_grouped"
    elif name == "sa3":
        npts = 128
        xyz = torch.from_numpy(rs.uniform(-0.5, 0.5, (B, npts, 3)).astype(np.float32)).to(dev)
        feats = torch.from_numpy(rs.uniform(0, 1, (G * B, npts, 256)).astype(np.float32)).to(dev)
        if where == "input":
            feats[B + cloud, 70, 200] = value                       # group 1 (network-major rows) of the cloud
        L = _Layers(dev, [(259, 256), (256, 512), (512, 1024)], bias)
        args = lambda out: (G, B, npts, 256, 256, 512, 1024, _lib.ptr(xyz), _lib.ptr(feats), L.table(G), _lib.ptr(out))
        shape = (G * B, npts // 64, 1024)
        entry = "ancsh_sa3_chain_grouped_f16x2"
    elif name == "fp1":
        npts = 128
        skip = torch.from_numpy(rs.uniform(0, 1, (G * B, npts, 256)).astype(np.float32)).to(dev)
        if where == "input":
            skip[cloud, 3, 9] = value                               # group 0
        init = torch.zeros((G * B, 256), **f)
        L = _Layers(dev, [(256, 256), (256, 256)], bias)
        args = lambda out: (G, B, npts, 256, 256, 256, _lib.ptr(skip), _lib.ptr(init), L.table(G), _lib.ptr(out))
        shape = (G * B * npts, 256)
        entry = "ancsh_fp1_chain_grouped_f16x2"
    elif name == "fp2":
        m, n = 128, 512
        points2 = torch.from_numpy(rs.uniform(0, 1, (G * B, m, 256)).astype(np.float32)).to(dev)
        idx = torch.from_numpy(rs.randint(0, m, (B, n, 3)).astype(np.int32)).to(dev)
        weight = torch.full((B, n, 3), 1.0 / 3.0, **f)
        points1 = torch.from_numpy(rs.uniform(0, 1, (G * B, n, 128)).astype(np.float32)).to(dev)
        if where == "input":
            points1[B + cloud, 400, 17] = value                     # group 1
        L = _Layers(dev, [(384, 256), (256, 128)], bias)
        args = lambda out: (G, B, m, n, 256, 128, 256, 128, _lib.ptr(points2), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(points1), L.table(G),
                            _lib.ptr(out))
        shape = (G * B * n, 128)
        entry = "ancsh_fp2_chain_grouped_f16x2"
    else:                                                           # the tail chain
        n, m = 512, 512
        points2 = torch.from_numpy(rs.uniform(0, 1, (G * B, m, 128)).astype(np.float32)).to(dev)
        idx = torch.from_numpy(rs.randint(0, m, (B, n, 3)).astype(np.int32)).to(dev)
        weight = torch.full((B, n, 3), 1.0 / 3.0, **f)
        xyz = torch.from_numpy(rs.uniform(-0.5, 0.5, (B, n, 3)).astype(np.float32)).to(dev)
        if where == "input":
            xyz[cloud, 100, 2] = value                              # both groups read the shared xyz
        shapes = [(131, 128), (128, 128), (128, 128), (128, 128), (128, 32), (128, 128), (128, 128), (128, 32)]
        L = _Layers(dev, shapes, bias)
        entry = "ancsh_mlp_chain_grouped_fp_f16x2"
        shape = (G, B * n, 64)

        def args(out):
            ops = []
            for i, (k, nn) in enumerate(shapes):
                head = nn == 32
                ops += [k, nn, 1, 0, 64 if head else 0]
            c_ops = (ctypes.c_int * len(ops))(*ops)
            tabs = []
            for g in range(G):
                ptrs = []
                col = 0
                for i, (k, nn) in enumerate(shapes):
                    head = nn == 32
                    ptrs += L.ptrs[4 * i:4 * i + 4] + [out[g, :, col:].data_ptr() if head else None]
                    col += 32 if head else 0
                tabs.append((ctypes.c_void_p * len(ptrs))(*ptrs))
            nops = (ctypes.c_int * G)(len(shapes), len(shapes))
            ops_tab = (ctypes.c_void_p * G)(ctypes.cast(c_ops, ctypes.c_void_p), ctypes.cast(c_ops, ctypes.c_void_p))
            ptr_tab = (ctypes.c_void_p * G)(*[ctypes.cast(t, ctypes.c_void_p) for t in tabs])
            L.keep += [c_ops, tabs, nops, ops_tab, ptr_tab]
            return (G, B, n, m, 128, _lib.ptr(points2), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(xyz), ctypes.cast(nops, ctypes.c_void_p),
                    ctypes.cast(ops_tab, ctypes.c_void_p), ctypes.cast(ptr_tab, ctypes.c_void_p))
    for guarded in (False, True):
        out = torch.full(shape, -7.0, **f)
        if guarded:
            _lib.call(entry + "_guarded", *args(out), _lib.ptr(flags), 0)
        else:
            _lib.call(entry, *args(out))
        outs.append(out)
    torch.cuda.synchronize()
    return outs[0].cpu().numpy(), outs[1].cpu().numpy(), flags.cpu().numpy()


ENTRIES = ("sa", "sa_partial", "sa3", "fp1", "fp2", "tail")
INPUT_GROUPS = {"sa": 3, "sa_partial": 3, "sa3": 2, "fp1": 1, "fp2": 2, "tail": 3}     # the groups whose input holds the planted value


@pytest.mark.parametrize("name", ENTRIES)
def test_guarded_entry_in_range_is_bit_identical_and_clean(dev, name):
    plain, guarded, flags = _run_entry(dev, name, 3, 0.25, "input", 1, bias=0.5)
    assert _same(plain, guarded) and not flags.any()


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("value,flagged", [(F16_MAX, False), (-F16_MAX, False), (ABOVE, True), (-1e6, True), (np.inf, True), (np.nan, False)])
def test_guarded_entry_input_edges(dev, name, value, flagged):
    """an input split site of every kernel family: exactly the planted (cloud, group) bits, outputs equal the unguarded launch's"""
    B, cloud = 3, 1
    plain, guarded, flags = _run_entry(dev, name, B, value, "input", cloud)
    assert _same(plain, guarded)
    want = np.zeros(B, np.int32)
    if flagged:
        want[cloud] = INPUT_GROUPS[name]
    assert flags.tolist() == want.tolist()


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("value,flagged", [(F16_MAX, False), (ABOVE, True), (np.inf, True), (np.nan, False)])
def test_guarded_entry_epilogue_edges(dev, name, value, flagged):
    """a hidden layer's epilogue split of every kernel family (every cloud, both groups)"""
    B = 2
    plain, guarded, flags = _run_entry(dev, name, B, value, "epilogue", 0)
    assert _same(plain, guarded)
    assert flags.tolist() == [3 * int(flagged)] * B


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------
K, B, N = 3, 4, 512
BIG = 2.0e5           # norm factor: absolute xyz beyond 65504 in layer3's and the tail's inputs; the ball-query levels see offsets only


def _raw_batches(pb, count, rs, every=5):
    """ragged raw clouds of the passthrough problem; cloud (k % B) of every `every`-th batch gets the norm factor BIG"""
    Pn, cls = pb["P"], pb["cls"]
    out, hot = [], []
    for k in range(count):
        clouds = []
        for _ in range(B):
            src = rs.randint(Pn.shape[0])
            n = int(rs.randint(N // 2, 2 * N))
            idx = rs.randint(0, N, n)
            clouds.append(np.concatenate([Pn[src][idx], cls[src][idx, None]], 1).astype(np.float32))
        nf = rs.uniform(0.9, 1.1, B).astype(np.float32)
        h = np.zeros(B, bool)
        if k % every == 0:
            h[k % B] = True
            nf[k % B] = BIG
        out.append((clouds, nf))
        hot.append(h)
    return out, hot


def _pipe(pb, arithmetic, slots, guard=False, **kw):
    from articulated_pose_amd.pipeline import AncshPipeline
    return AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, "cuda:0", couple=True, slots=slots, niter_a=64, niter_b=8, seed=11,
                         lm_schedule="throughput", arithmetic=arithmetic, range_guard=guard, raw_capacity=B * 2 * N, **kw)


@pytest.mark.parametrize("slots", [1, 4])
def test_stream_refits_flagged_clouds_in_f32(dev, slots):
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches, hot = _raw_batches(pb, 40, np.random.RandomState(slots))
    f32 = list(_pipe(pb, "f32", slots).stream_batches(batches))
    for (_t, _s, rec), h in zip(f32, hot):
        # the f32 path fits an overflowing cloud: its record is not the poisoned (all-NaN) record of a non-finite cloud.  (At coordinates
        # of 1e5 the synthetic problem's fits degenerate, and some fields of the record are NaN by themselves.)
        assert all(np.isfinite(rec[b]).any() for b in np.flatnonzero(h))
    f16 = list(_pipe(pb, "f16x2", slots).stream_batches(batches))
    pipe = _pipe(pb, "f16x2", slots, guard=True)
    got = list(pipe.stream_batches(batches, flags=True))
    assert len(got) == len(batches)
    reruns = 0
    for (tag, seed, rec, words), (_, _, r32), (_, _, r16), h in zip(got, f32, f16, hot):
        assert ((words != 0) == h).all(), (tag, words, h)
        assert (words[h] == 3).all()                               # both networks saw the overflow
        assert _same(rec[~h], r16[~h]), tag
        assert _same(rec[h], r32[h]), tag
        reruns += bool(h.any())
    assert pipe.f32_reruns == reruns == 8
    assert all(len(x) == 3 for x in pipe.stream_batches(batches[:2]))      # the default keeps the 3-tuples


def test_replay_resets_the_flags(dev):
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches, hot = _raw_batches(pb, 2, np.random.RandomState(0), every=2)
    assert hot[0].any() and not hot[1].any()
    pipe = _pipe(pb, "f16x2", 1, guard=True)
    words = [w for _t, _s, _r, w in pipe.stream_batches(batches, flags=True)]      # one slot: the second batch replays the same graph
    assert words[0].any() and not words[1].any()
    assert pipe.f32_reruns == 1


def test_step_path_flags_and_rerun_f32(dev):
    from articulated_pose_amd.pipeline import AncshPipeline
    pb = passthrough_pose_problem(K, B, N, seed=4)
    P = pb["P"].copy()
    P[2] *= np.float32(BIG)
    jc = pb["cls"].astype(np.int32)
    kw = dict(couple=True, slots=1, niter_a=64, niter_b=8, seed=5, lm_schedule="throughput")
    ref = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, arithmetic="f32", **kw)
    ref.load_inputs(P, jc)
    ref.prepare()
    _, r = ref.step()
    ref.synchronize()
    want = r["record"].cpu().numpy().copy()
    pipe = AncshPipeline(K, pb["w_ancsh"], pb["w_npcs"], B, N, dev, arithmetic="f16x2", range_guard=True, **kw)
    pipe.load_inputs(P, jc)
    pipe.prepare()
    sl, out = pipe.step()
    sl.stream.synchronize()
    assert out["range_flags"].cpu().numpy().tolist() == [0, 0, 3, 0]
    o32 = pipe.rerun_f32(sl)
    sl.stream.synchronize()
    assert _same(o32["record"].cpu().numpy(), want)


def test_nonfinite_clouds_under_the_guard(dev):
    """a NaN cloud and an inf cloud (flagged, refit in f32, poisoned there): both records poisoned, the neighbours equal the unguarded
    F16x2 records"""
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches, _ = _raw_batches(pb, 1, np.random.RandomState(9), every=1000)
    clouds, nf = batches[0]
    clouds = [c.copy() for c in clouds]
    clouds[0][5, 0] = np.nan
    clouds[2][:, 1] = np.inf
    item = [(clouds, nf)]
    f16 = list(_pipe(pb, "f16x2", 1).stream_batches(item))[0][2]
    f32 = list(_pipe(pb, "f32", 1).stream_batches(item))[0][2]
    pipe = _pipe(pb, "f16x2", 1, guard=True)
    _t, _s, rec, words = list(pipe.stream_batches(item, flags=True))[0]
    assert words[2] != 0 and words[1] == 0 and words[3] == 0
    for b in range(B):              # every record is the one its flag word selects (the NaN cloud may flag: NaN geometry can make inf)
        assert _same(rec[b], f32[b] if words[b] else f16[b]), b
    assert np.isnan(rec[0]).all() and np.isnan(rec[2]).all()      # both poisoned, under either arithmetic


def test_two_arithmetics_in_one_process(dev):
    """an f32 and a guarded F16x2 pipeline driven alternately each equal their own single-pipeline run; the module globals are untouched"""
    from articulated_pose_amd import pointnet_util
    before = (pointnet_util.SA_BF16X3, pointnet_util.SPLIT_SCHEME)
    pb = passthrough_pose_problem(K, 6, N, seed=3)
    batches, _ = _raw_batches(pb, 6, np.random.RandomState(2), every=3)
    alone32 = list(_pipe(pb, "f32", 2).stream_batches(batches))
    alone16 = list(_pipe(pb, "f16x2", 2, guard=True).stream_batches(batches))
    p32, p16 = _pipe(pb, "f32", 2), _pipe(pb, "f16x2", 2, guard=True)
    for k, (clouds, nf) in enumerate(batches):
        p32.submit(clouds, nf, tag=k)
        p16.submit(clouds, nf, tag=k)
        a, b = p32.retire(), p16.retire()
        assert _same(a[2], alone32[k][2]) and _same(b[2], alone16[k][2]), k
    assert (pointnet_util.SA_BF16X3, pointnet_util.SPLIT_SCHEME) == before
