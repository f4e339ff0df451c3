"""Every split-16 kernel (csrc/sa_bf16x3.hip, mid_bf16x3.hip, tail_bf16x3.hip on csrc/bx3.h), both schemes, launched directly through the C
ABI on small ragged and 8-cloud shapes and compared with a float64 evaluation of the same operation (tests/split16_ref.py).

Per case:
  * accuracy: err = max |out - float64| / max |float64| against the same figure err_f32 of the project's f32 entry point of the same chain
    on the same inputs (an f32 torch evaluation where the f32 entry does not take the shape): err <= bar * max(err_f32, 2^-23), bar = 4
    (F16x2) / 2 (Bf16x3) -- tests/test_split16_emulation_cpu.py says where the bars come from.  Every case's figures go to
    split16_kernel_errors.json in the report directory (REPORT_DIR below);
  * batch-composition invariance: with 8 clouds or more, three (group, cloud) pairs launched alone (G = 1, B = 1) give the batched
    launch's rows bit for bit -- whatever the XCD-aware tile maps did with them;
  * grouped = separate: a G-group launch equals G launches of one group, bit for bit (with G = 4 the last group carries the first one's
    parameters);
  * red zones: outputs live in sentinel-guarded buffers (tests/redzone.py): guards untouched, the columns between a head block and the
    next one (or out_ld) untouched, every in-range element written and finite;
  * a second launch gives the same bytes.
Index and weight inputs come from the project's operators (ball query with its first-index padding, three_nn_weights with its m < 3
slots); activations are O(1) with post-ReLU-like columns (exact zeros) and a few columns of 1e-5 .. 1e-3 (F16x2's hi term subnormal or
nearly so); bias and shift are non-zero and a quarter of the BN scales negative."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import split16_ref as R
from redzone import Arena, guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("f16x2", "bf16x3")
_VP = ctypes.c_void_p
_REPORT = {}
REPORT_DIR = os.path.join(ROOT, "test_reports")            # where the error report goes (git-ignored, created on demand)


def _record(family, scheme, shape, err, err_f32, yardstick):
    ratio = err / max(err_f32, R.FLOOR)
    _REPORT["%s %s %s" % (family, scheme, shape)] = dict(family=family, scheme=scheme, shape=list(shape), err=err, err_f32=err_f32, ratio=ratio,
                                                         yardstick=yardstick)
    print("%s %s %s: err %.3e err_f32 %.3e (%s) ratio %.2f" % (family, scheme, shape, err, err_f32, yardstick, ratio))
    worst = {}
    for c in _REPORT.values():
        key = "%s %s" % (c["family"], c["scheme"])
        worst[key] = max(worst.get(key, 0.0), c["ratio"])
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "split16_kernel_errors.json"), "w") as fh:
        json.dump(dict(bars=R.BARS, floor=R.FLOOR, worst_ratio=worst, cases=list(_REPORT.values())), fh, indent=1)
    return ratio


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _acts(rng, shape):
    """O(1) activations; every fourth channel post-ReLU-like (non-negative, exact zeros), one channel in 16 of magnitude 1e-5 .. 1e-3"""
    a = rng.randn(*shape).astype(np.float32)
    c = np.arange(shape[-1])
    a[..., c % 4 == 1] = np.maximum(a[..., c % 4 == 1], 0.0)
    tiny = c % 16 == 7
    a[..., tiny] = (np.exp(rng.uniform(np.log(1e-5), np.log(1e-3), a[..., tiny].shape)) * rng.choice([-1.0, 1.0], a[..., tiny].shape)).astype(np.float32)
    return a


def _layers(rng, dev, dims, k_first=None):
    """layers dims[0] -> dims[1] -> ...: kernels N(0, 1 / k), bias and shift 0.1 N(0, 1), BN scale U(0.5, 1.5) with a quarter negative.
    k_first: the first kernel has k_first rows (the kernels take its LAST dims[0] ones: fa_layer1)"""
    out = []
    for i, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
        rows = k_first if i == 0 and k_first else k
        out.append(dict(w=_T(rng.randn(rows, n) / np.sqrt(k), dev), b=_T(0.1 * rng.randn(n), dev),
                        scale=_T(rng.uniform(0.5, 1.5, n) * rng.choice([1.0, 1.0, 1.0, -1.0], n), dev), shift=_T(0.1 * rng.randn(n), dev)))
    return out


def _nets(rng, dev, G, dims, k_first=None):
    nets = [_layers(rng, dev, dims, k_first) for _ in range(G)]
    if G == 4:
        nets[3] = nets[0]                                      # two groups with identical parameters
    return nets


def _table(nets, groups, row0s, scheme):
    """the `const float *const *params` of a launch over `groups`: per group and layer {kernel, bias, scale, shift}; scheme None = the f32
    packing.  The kernel rows row0.. are taken as the call sites take them (pointnet_util._bf16x3_weight / tf_util.packed_weight)."""
    from articulated_pose_amd import pointnet_util, tf_util
    ptrs = []
    for g in groups:
        for L, r0 in zip(nets[g], row0s):
            w = tf_util.packed_weight(L, r0) if scheme is None else pointnet_util._bf16x3_weight(L, r0, scheme)
            ptrs += [w.data_ptr(), L["b"].data_ptr(), L["scale"].data_ptr(), L["shift"].data_ptr()]
    arr = (_VP * len(ptrs))(*ptrs)
    return arr, ctypes.cast(arr, _VP)


def _name(entry, scheme):
    from articulated_pose_amd import pointnet_util
    return pointnet_util.split_name(entry, scheme)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sel(x, G, B, groups, b0, b1):
    """rows of the network-major x (G * B, ...) for `groups` and clouds b0 .. b1 - 1, network-major, contiguous"""
    v = x.view((G, B) + tuple(x.shape[1:]))
    return torch.cat([v[g, b0:b1] for g in groups], dim=0).contiguous()


# ---- the families: run(scheme, groups, b0, b1, arena) -> [out per group] (scheme None: the f32 entry; "ref64" / "ref32": torch) ----------
class _SA(object):
    def __init__(self, dev, G, B, n, m, partial):
        from articulated_pose_amd import tf_ops
        from articulated_pose_amd.tf_ops.tf_sampling import farthest_point_sample_gather
        rng = np.random.RandomState(1000 * G + 100 * B + n + m + int(partial))
        self.family, self.shape, self.dev, self.G, self.B, self.n, self.m = ("sa2_partial" if partial else "sa1"), (G, B, n, m), dev, G, B, n, m
        self.mlp = (128, 128, 256) if partial else (64, 64, 128)
        self.xyz = _T(rng.uniform(-0.5, 0.5, (B, n, 3)), dev)
        _, self.new_xyz = farthest_point_sample_gather(m, self.xyz)
        self.idx, _ = tf_ops.query_ball_point(0.3, 64, self.xyz, self.new_xyz)          # short balls are padded with their first index
        assert tuple(self.idx.shape) == (B, m, 64) and int(self.idx.min()) >= 0 and int(self.idx.max()) < n
        self.nets = _nets(rng, dev, G, (3,) + self.mlp)
        self.partial = _T(_acts(rng, (G * B, n, 128)), dev) if partial else None
        self.f32_entry = True

    def run(self, scheme, groups, b0, b1, arena):
        from articulated_pose_amd import _lib
        nb, ng = b1 - b0, len(groups)
        xyz, new_xyz, idx = self.xyz[b0:b1].contiguous(), self.new_xyz[b0:b1].contiguous(), self.idx[b0:b1].contiguous()
        keep, params = _table(self.nets, groups, (0, 0, 0), scheme)
        out = arena.empty((ng * nb, self.m, self.mlp[2]), dtype=torch.float32, device=self.dev)
        if self.partial is None:
            entry = "ancsh_sa_module_fused_grouped" if scheme is None else _name("ancsh_sa_module_fused_bf16x3_grouped", scheme)
            _lib.call(entry, ng, nb, self.n, self.m, 64, 0, *self.mlp, _lib.ptr(xyz), None, _lib.ptr(new_xyz), _lib.ptr(idx), params, _lib.ptr(out))
        else:
            part = _sel(self.partial, self.G, self.B, groups, b0, b1)
            entry = "ancsh_sa_module_fused_partial_grouped" if scheme is None else _name("ancsh_sa_module_fused_partial_bf16x3_grouped", scheme)
            _lib.call(entry, ng, nb, self.n, self.m, 64, *self.mlp, _lib.ptr(xyz), _lib.ptr(part), _lib.ptr(new_xyz), _lib.ptr(idx), params, _lib.ptr(out))
        torch.cuda.synchronize()
        return list(out.view(ng, nb, self.m, self.mlp[2]))

    def ref(self, g, dt):
        part = None if self.partial is None else self.partial.view(self.G, self.B, self.n, 128)[g]
        return R.sa_level(self.xyz, self.new_xyz, self.idx, self.nets[g], part, dt)


class _SA3(object):
    family = "sa3"

    def __init__(self, dev, G, B, npts):
        rng = np.random.RandomState(3000 + 100 * G + 10 * B + npts)
        self.shape, self.dev, self.G, self.B, self.npts = (G, B, npts), dev, G, B, npts
        self.xyz = _T(rng.uniform(-1, 1, (B, npts, 3)), dev)
        self.feats = _T(_acts(rng, (G * B, npts, 256)), dev)
        self.nets = _nets(rng, dev, G, (259, 256, 512, 1024))
        self.f32_entry = True

    def run(self, scheme, groups, b0, b1, arena):
        from articulated_pose_amd import _lib
        nb, ng, npts = b1 - b0, len(groups), self.npts
        xyz, feats = self.xyz[b0:b1].contiguous(), _sel(self.feats, self.G, self.B, groups, b0, b1)
        keep, params = _table(self.nets, groups, (0, 0, 0), scheme)
        tile = 32 if scheme is None else 64
        out = arena.empty((ng * nb, npts // tile, 1024), dtype=torch.float32, device=self.dev)
        entry = "ancsh_sa3_chain_grouped" if scheme is None else _name("ancsh_sa3_chain_grouped_bf16x3", scheme)
        _lib.call(entry, ng, nb, npts, 256, 256, 512, 1024, _lib.ptr(xyz), _lib.ptr(feats), params, _lib.ptr(out))
        torch.cuda.synchronize()
        if scheme is None:                                       # maxima of 32-row tiles -> of 64-row tiles (max is exact in any order)
            out = out.view(ng * nb, npts // 64, 2, 1024).max(dim=2).values
        return list(out.view(ng, nb, npts // 64, 1024))

    def ref(self, g, dt):
        return R.sa3(self.xyz, self.feats.view(self.G, self.B, self.npts, 256)[g], self.nets[g], dt)


class _FP1(object):
    family = "fp1"

    def __init__(self, dev, G, B, npts):
        rng = np.random.RandomState(4000 + 100 * G + 10 * B + npts)
        self.shape, self.dev, self.G, self.B, self.npts = (G, B, npts), dev, G, B, npts
        self.skip = _T(_acts(rng, (G * B, npts, 256)), dev)
        self.init = _T(rng.randn(G * B, 256), dev)               # the single-source share of the first product: any f32 row per cloud
        self.nets = _nets(rng, dev, G, (256, 256, 256), k_first=1280)      # fa_layer1's first kernel has 1280 rows; the chain takes rows 1024..
        self.f32_entry = True

    def run(self, scheme, groups, b0, b1, arena):
        from articulated_pose_amd import _lib
        nb, ng, npts = b1 - b0, len(groups), self.npts
        skip, init = _sel(self.skip, self.G, self.B, groups, b0, b1), _sel(self.init, self.G, self.B, groups, b0, b1)
        keep, params = _table(self.nets, groups, (1024, 0), scheme)
        out = arena.empty((ng * nb * npts, 256), dtype=torch.float32, device=self.dev)
        entry = "ancsh_fp1_chain_grouped" if scheme is None else _name("ancsh_fp1_chain_grouped_bf16x3", scheme)
        _lib.call(entry, ng, nb, npts, 256, 256, 256, _lib.ptr(skip), _lib.ptr(init), params, _lib.ptr(out))
        torch.cuda.synchronize()
        return list(out.view(ng, nb, npts, 256))

    def ref(self, g, dt):
        return R.fp1(self.skip.view(self.G, self.B, self.npts, 256)[g], self.init.view(self.G, self.B, 256)[g], self.nets[g], 1024, dt).view(self.B, self.npts, 256)


def _three_nn(fine, coarse):
    from articulated_pose_amd.tf_ops import tf_interpolate
    _d, idx, w = tf_interpolate.three_nn_weights(fine, coarse)                   # m < 3: the missing slots are (index 0, weight 0)
    assert int(idx.min()) >= 0 and int(idx.max()) < coarse.shape[1] and bool(torch.isfinite(w).all())
    return idx.contiguous(), w.contiguous()


class _FP2(object):
    family = "fp2"

    def __init__(self, dev, G, B, m, n):
        rng = np.random.RandomState(5000 + 100 * G + 10 * B + m + n)
        self.shape, self.dev, self.G, self.B, self.m, self.n = (G, B, m, n), dev, G, B, m, n
        self.idx, self.weight = _three_nn(_T(rng.uniform(-1, 1, (B, n, 3)), dev), _T(rng.uniform(-1, 1, (B, m, 3)), dev))
        self.points2 = _T(_acts(rng, (G * B, m, 256)), dev)
        self.points1 = _T(_acts(rng, (G * B, n, 128)), dev)
        self.nets = _nets(rng, dev, G, (384, 256, 128))
        self.f32_entry = True

    def run(self, scheme, groups, b0, b1, arena):
        from articulated_pose_amd import _lib
        nb, ng = b1 - b0, len(groups)
        p2, p1 = _sel(self.points2, self.G, self.B, groups, b0, b1), _sel(self.points1, self.G, self.B, groups, b0, b1)
        idx, weight = self.idx[b0:b1].contiguous(), self.weight[b0:b1].contiguous()
        keep, params = _table(self.nets, groups, (0, 0), scheme)
        out = arena.empty((ng * nb * self.n, 128), dtype=torch.float32, device=self.dev)
        entry = "ancsh_fp2_chain_grouped" if scheme is None else _name("ancsh_fp2_chain_grouped_bf16x3", scheme)
        _lib.call(entry, ng, nb, self.m, self.n, 256, 128, 256, 128, _lib.ptr(p2), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(p1), params, _lib.ptr(out))
        torch.cuda.synchronize()
        return list(out.view(ng, nb, self.n, 128))

    def ref(self, g, dt):
        return R.fp2(self.points2.view(self.G, self.B, self.m, 256)[g], self.idx, self.weight, self.points1.view(self.G, self.B, self.n, 128)[g],
                     self.nets[g], dt).view(self.B, self.n, 128)


def _tail_weights(K, mixed, seed):
    """the variable store of one network with a quarter of its BN scales negative"""
    from articulated_pose_amd.weights import synthetic_weights
    w = synthetic_weights(K, mixed_pred=mixed, early_split_nocs=mixed, seed=seed)
    rng = np.random.RandomState(seed + 99)
    for k in sorted(w):
        if k.endswith("/bn/gamma"):
            w[k] = (w[k] * rng.choice([1.0, 1.0, 1.0, -1.0], w[k].shape)).astype(np.float32)
    return w


class _Tail(object):
    """kinds[g] = (K, mixed): the architecture module's own program of that network (mixed: with the [L h+] branch); or descr[g] = a
    hand-made [(layer, relu, out_col | None)] with lds[g] its row stride"""
    family = "tail"

    def __init__(self, dev, G, B, n, m, kinds=None, descr=None, lds=None):
        rng = np.random.RandomState(6000 + 100 * G + 10 * B + n + m)
        self.shape, self.dev, self.G, self.B, self.n, self.m = (G, B, n, m), dev, G, B, n, m
        self.xyz = _T(rng.uniform(-0.5, 0.5, (B, n, 3)), dev)
        self.idx, self.weight = _three_nn(self.xyz, _T(rng.uniform(-0.5, 0.5, (B, m, 3)), dev))
        self.points2 = _T(_acts(rng, (G * B, m, 128)), dev)
        self.kinds = kinds
        if kinds is not None:
            self.stores = [_tail_weights(K, mixed, 40 + 7 * g + K) for g, (K, mixed) in enumerate(kinds)]
            self.shape = self.shape + tuple("K%d%s" % (K, "a" if mixed else "n") for K, mixed in kinds)
            descr, lds = [], []
            # The programs' structure, read back from the builder's own tables as architecture._tail_program's add() lays them out: per op
            # five ints {k, n, act, flags, out_ld} and five pointers {kernel, bias, scale, shift, out | NULL}, out = logits + the block's first
            # column; `keep` holds the op's layer dict.  run() below re-emits the same tables (add()'s bf16x3 branch) for its sub-launches.
            for g in range(G):
                ops, ptrs, logits, ld, keep = self._build(g, 64, None)
                descr.append([(keep[i], ops[5 * i + 2] == 1, None if not ptrs[5 * i + 4] else (ptrs[5 * i + 4] - logits.data_ptr()) // 4)
                              for i in range(len(keep))])
                lds.append(ld)
        self.descr, self.lds = descr, lds
        self.f32_entry = kinds is not None and n % 128 == 0      # ancsh_mlp_chain_grouped_fp takes n % 128 == 0

    def _build(self, g, rows, scheme):
        """architecture._tail_program of network g (scheme None: the f32 program)"""
        from articulated_pose_amd import architecture, tf_util
        K, mixed = self.kinds[g]
        tf_util.set_variables(self.stores[g])
        with tf_util.variable_scope("SPFN"):
            return architecture._tail_program(rows, K, mixed, mixed, self.dev, bf16x3=scheme is not None, scheme=scheme)

    def valid(self, g):
        """the columns of group g's logits that a head block writes"""
        mask = torch.zeros(self.lds[g], dtype=torch.bool, device=self.dev)
        for L, _relu, col in self.descr[g]:
            if col is not None:
                mask[col:col + L["w"].shape[1]] = True
        return mask

    def run(self, scheme, groups, b0, b1, arena):
        from articulated_pose_amd import _lib, architecture, pointnet_util
        nb, ng, n = b1 - b0, len(groups), self.n
        p2 = _sel(self.points2, self.G, self.B, groups, b0, b1).view(ng * nb, self.m, 128)
        idx, weight, xyz = self.idx[b0:b1].contiguous(), self.weight[b0:b1].contiguous(), self.xyz[b0:b1].contiguous()
        fp = (nb, n, self.m, p2, idx, weight, xyz)
        whole = self.kinds is not None and list(groups) == list(range(self.G)) and (b0, b1) == (0, self.B)
        if whole:                                                # the builder's own tables through the call site's launch helper
            with guarded():                                      # the builder allocates its logits itself: red zones checked on exit
                progs = [self._build(g, nb * n, scheme) for g in groups]
                if scheme is None:
                    architecture.run_tail_programs(None, nb * n, progs, fp=fp)
                else:
                    architecture.run_tail_programs_bf16x3(progs, fp, pointnet_util.Arithmetic(3, scheme))
            return [p[2] for p in progs]
        assert scheme is not None
        outs, c_ops, c_ptrs = [], [], []
        for g in groups:                                         # the same programs re-emitted for this launch's rows
            logits = arena.empty((nb * n, self.lds[g]), dtype=torch.float32, device=self.dev)
            ops, ptrs = [], []
            for L, relu, col in self.descr[g]:
                k, c = L["w"].shape
                par = (architecture._bf16x3_head_params(L, scheme) if col is not None else
                       (pointnet_util._bf16x3_weight(L, 0, scheme), L["b"], L["scale"], L["shift"]))
                ops += [k, c, 1 if relu else 0, 0, self.lds[g] if col is not None else 0]
                ptrs += [v.data_ptr() for v in par] + [logits[:, col:].data_ptr() if col is not None else None]
            outs.append(logits)
            c_ops.append((ctypes.c_int * len(ops))(*ops))
            c_ptrs.append((_VP * len(ptrs))(*ptrs))
        nops = (ctypes.c_int * ng)(*[len(self.descr[g]) for g in groups])
        ops_tab = (_VP * ng)(*[ctypes.cast(o, _VP) for o in c_ops])
        ptr_tab = (_VP * ng)(*[ctypes.cast(o, _VP) for o in c_ptrs])
        _lib.call(_name("ancsh_mlp_chain_grouped_fp_bf16x3", scheme), ng, nb, n, self.m, 128, _lib.ptr(p2), _lib.ptr(idx), _lib.ptr(weight), _lib.ptr(xyz),
                  ctypes.cast(nops, _VP), ctypes.cast(ops_tab, _VP), ctypes.cast(ptr_tab, _VP))
        torch.cuda.synchronize()
        return [o.view(nb, n, -1) for o in outs]

    def ref(self, g, dt):
        heads = R.tail(self.points2.view(self.G, self.B, self.m, 128)[g], self.idx, self.weight, self.xyz, self.descr[g], dt)
        out = torch.full((self.B * self.n, self.lds[g]), float("nan"), dtype=dt, device=self.dev)
        for col, v in heads:
            out[:, col:col + v.shape[1]] = v
        return out.view(self.B, self.n, -1)


# ---- the assertions of one case ----------------------------------------------------------------------------------------------------
def _check(case, scheme):
    G, B = case.G, case.B
    arena = Arena()
    valid = getattr(case, "valid", None)
    per_cloud = lambda t, nb=B: t.reshape((nb, -1) + tuple(t.shape[-1:]))
    out = [per_cloud(o) for o in case.run(scheme, range(G), 0, B, arena)]
    arena.check()                                                # guards before and behind every output (rows beyond the last tile included)
    for g, o in enumerate(out):
        if valid is None:
            assert bool(torch.isfinite(o).all()), (g, "an element not written or not finite")
        else:
            m = valid(g)
            assert bool(torch.isfinite(o[..., m]).all()), (g, "a head column not written or not finite")
            assert bool((o[..., ~m].contiguous().view(torch.int32) == -1).all()), (g, "a column between the head blocks was written")
    again = [per_cloud(o) for o in case.run(scheme, range(G), 0, B, arena)]
    for g in range(G):
        assert _bits(out[g], again[g]), ("repeat launch", g)
    if G > 1:
        for g in range(G):
            alone = per_cloud(case.run(scheme, [g], 0, B, arena)[0])
            assert _bits(out[g], alone), ("grouped != separate", g)
    if G * B >= 8:
        for g, b in sorted({(G - 1, B - 1), (0, 0), (G // 2, B // 2)}):
            alone = per_cloud(case.run(scheme, [g], b, b + 1, arena)[0], 1)
            assert _bits(out[g][b:b + 1], alone), ("batch composition", g, b)
    arena.check()
    # accuracy against float64, measured in units of the f32 path's own error
    pick = (lambda g, t: t) if valid is None else (lambda g, t: t[..., valid(g)])
    flat = lambda ts: torch.cat([pick(g, t).reshape(-1).double() for g, t in enumerate(ts)])
    want = flat([case.ref(g, torch.float64) for g in range(G)])
    if case.f32_entry:
        f32, yardstick = flat([per_cloud(o) for o in case.run(None, range(G), 0, B, arena)]), "f32 entry"
        arena.check()
    else:
        f32, yardstick = flat([case.ref(g, torch.float32) for g in range(G)]), "f32 torch"
    err, err_f32 = R.rel_err(flat(out), want), R.rel_err(f32, want)
    _record(case.family, scheme, case.shape, err, err_f32, yardstick)
    assert err <= R.BARS[scheme] * max(err_f32, R.FLOOR), (case.family, scheme, case.shape, err, err_f32)


# (G, B, n, m): ragged, 1..4 groups; (3, 8, 256, 8) and (2, 16, 128, 4) take the XCD-aware map (clouds % 8 == 0, m % 4 == 0), (2, 8, 256, 6) must not
SA1 = [(1, 1, 3, 1), (2, 3, 100, 5), (1, 5, 300, 7), (2, 2, 64, 64), (4, 4, 200, 12), (3, 8, 256, 8), (2, 16, 128, 4), (2, 8, 256, 6)]
SA2 = [(1, 1, 3, 1), (2, 5, 300, 7), (3, 3, 64, 13), (2, 8, 128, 8)]
MID = [(1, 1, 64), (2, 3, 128), (4, 2, 192), (2, 8, 64), (3, 8, 128)]                # (G, B, npts)
# (G, B, m, n): m = 1, 2 leave three_nn_weights' empty slots; (2, 4, 128, 512) and (3, 8, 64, 192) take the tile map (8 / 24 clouds)
FP2 = [(1, 1, 1, 64), (2, 3, 2, 128), (4, 2, 128, 64), (2, 5, 128, 512), (1, 8, 128, 64), (2, 4, 128, 512), (3, 8, 64, 192)]
# (G, B, n, m), the networks' (K, with the [L h+] branch): K = 1, 2, 5 and 7 (the widest head blocks the tail takes; K = 8 below) in both
# kinds.  The tail's XCD-aware map needs b % 8 == 0 and n % 256 == 0 and permutes only with two or more workgroups per cloud: none of the
# first six shapes does, (2, 8, 512, 32) (n / 256 = 2) does.
TAIL = [((1, 1, 64, 16), [(5, False)]), ((2, 3, 192, 64), [(1, True), (1, False)]), ((2, 5, 1024, 512), [(2, True), (2, False)]),
        ((1, 8, 64, 64), [(1, True)]), ((2, 8, 128, 32), [(5, True), (7, False)]), ((2, 4, 512, 128), [(7, True), (5, False)]),
        ((2, 8, 512, 32), [(2, False), (5, True)])]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("G,B,n,m", SA1)
def test_sa_level(dev, scheme, G, B, n, m):
    _check(_SA(dev, G, B, n, m, False), scheme)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("G,B,n,m", SA2)
def test_sa_level_partial_sums(dev, scheme, G, B, n, m):
    _check(_SA(dev, G, B, n, m, True), scheme)


@pytest.mark.parametrize("G,B,npts", MID)
def test_sa3_chain(dev, G, B, npts):
    _check(_SA3(dev, G, B, npts), "f16x2")


def test_sa3_chain_bf16x3_refuses_before_any_launch(dev):
    """three bf16 planes of a 64 x 512 tile exceed the LDS: -1 with the limit named, nothing written -- production falls back to the f32 chain on it"""
    case, arena = _SA3(dev, 2, 3, 128), Arena()
    with pytest.raises(ValueError, match="LDS"):
        case.run("bf16x3", range(2), 0, 3, arena)
    raw, off, nbytes, _what = arena.blocks[0]
    assert bool((raw[off:off + nbytes] == 0xFF).all())
    arena.check()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("G,B,npts", MID)
def test_fp1_chain(dev, scheme, G, B, npts):
    _check(_FP1(dev, G, B, npts), scheme)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("G,B,m,n", FP2)
def test_fp2_chain(dev, scheme, G, B, m, n):
    _check(_FP2(dev, G, B, m, n), scheme)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape,kinds", TAIL, ids=["-".join(map(str, s)) for s, _k in TAIL])
def test_tail_chain(dev, scheme, shape, kinds):
    _check(_Tail(dev, *shape, kinds=kinds), scheme)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_tail_chain_narrow_head_blocks(dev, scheme):
    """a hand-made program with head blocks of 1, 31 and 32 columns in rows of 72: column 1 (between the first two blocks) and columns
    66 .. 71 (between the last block and out_ld) stay untouched"""
    rng = np.random.RandomState(77)
    hid = lambda k=128: _layers(rng, dev, (k, 128))[0]
    head = lambda n: dict(_layers(rng, dev, (128, n))[0], scale=torch.ones(n, device=dev), shift=torch.zeros(n, device=dev))
    descr = [[(hid(131), True, None), (hid(), True, None), (hid(), True, None), (hid(), True, None), (head(1), False, 0), (head(31), False, 2),
              (hid(), False, None), (head(32), False, 33), (hid(), True, None), (hid(), True, None), (head(1), True, 65)]]
    _check(_Tail(dev, 1, 3, 128, 40, descr=descr, lds=[72]), scheme)


def test_tail_k8_is_refused_by_the_builder(dev):
    """K = 8 has a 33-column head block in either kind of network: the tail kernels take head blocks of at most 32 columns (the entry refuses
    wider ones: test_bf16x3_tail_rejects_other_program_shapes).  The architecture module says so before anything is launched and cannot
    build such a program; K = 8 forwards keep the layer-by-layer f32 tail.  K = 7 is the widest the split-16 tail takes (TAIL above)."""
    from articulated_pose_amd import architecture
    for mixed in (True, False):
        assert architecture._head_dims(8, mixed, mixed)[1] is False and architecture._head_dims(7, mixed, mixed)[1] is True
        case = _Tail.__new__(_Tail)
        case.kinds, case.stores, case.dev = [(8, mixed)], [_tail_weights(8, mixed, 5)], dev
        with pytest.raises(AssertionError):
            case._build(0, 64, None)                             # the f32 chain program: its own width check
        with pytest.raises(RuntimeError, match="32"):
            case._build(0, 64, "f16x2")                          # the split-16 program: a 33-column kernel does not pad to 32 columns
