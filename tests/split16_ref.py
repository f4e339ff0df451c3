"""References for the split-16 kernels (csrc/bx3.h, sa_bf16x3.hip, mid_bf16x3.hip, tail_bf16x3.hip); test infrastructure, importable
without a GPU.

Two halves:

  * plain references of the six kernel families in torch, written from the kernels' head comments and independent of the packing, the
    tile maps and the group arithmetic.  `dt` selects the precision: torch.float64 is the reference, torch.float32 the "f32 evaluation in
    yet another order" where a family has no f32 entry point of the same form.  A layer is a dict {"w" (k, n), "b", "scale", "shift"} of
    f32 tensors (tf_util.get_layer's form) and computes act((x . w + b) * scale + shift).  Operands the kernels form in f32 before the first
    product -- the centred coordinates, the three-point interpolation -- are formed in f32, unfused, in the kernels' order, and only then
    converted: reference and kernel start from the same numbers.

  * a numpy emulation of the two arithmetics exactly as bx3.h states them, with a switch that drops any one product of any one layer
    (the mutants of tests/test_split16_emulation_cpu.py).
"""
import numpy as np
import torch

FLOOR = 2.0 ** -23          # floor of the f32 yardstick: one f32 ulp of the output scale
BARS = {"f16x2": 4.0, "bf16x3": 2.0}      # err <= BARS[scheme] * max(err_f32, FLOOR); justified by tests/test_split16_emulation_cpu.py


# ---- plain references ------------------------------------------------------------------------------------------------------------
def layer(x, L, relu, dt, init=None):
    """act((x . w [+ init] + b) * scale + shift) in precision dt; init: accumulator start, broadcast against the product"""
    y = x.to(dt) @ L["w"].to(dt)
    if init is not None:
        y = y + init.to(dt)
    y = (y + L["b"].to(dt)) * L["scale"].to(dt) + L["shift"].to(dt)
    return torch.relu(y) if relu else y


def rel_err(got, want):
    """max |got - want| / max |want| over the whole case"""
    return float((got.double() - want.double()).abs().max()) / float(want.double().abs().max())


def sa_level(xyz, new_xyz, idx, layers, partial, dt):
    """One network's set-abstraction level.  xyz (B, n, 3), new_xyz (B, m, 3), idx (B, m, 64); partial None or (B, n, c1): the first layer's
    partial sums over the feature channels per SOURCE point, gathered like the coordinates.  -> (B, m, c3)."""
    B = xyz.shape[0]
    bi = torch.arange(B, device=xyz.device).view(B, 1, 1)
    ii = idx.long()
    g = xyz[bi, ii] - new_xyz.unsqueeze(2)                       # f32, one rounding per coordinate: the kernel's dx, dy, dz
    x = layer(g, layers[0], True, dt, None if partial is None else partial[bi, ii])
    x = layer(x, layers[1], True, dt)
    x = layer(x, layers[2], True, dt)
    return x.max(dim=2).values


def sa3(xyz, feats, layers, dt):
    """layer3 of one network: xyz (B, npts, 3), feats (B, npts, 256) -> (B, npts / 64, 1024), the maximum over every 64-row tile"""
    B, npts, _ = feats.shape
    x = torch.cat([xyz, feats], dim=2)
    for L in layers:
        x = layer(x, L, True, dt)
    return x.view(B, npts // 64, 64, -1).max(dim=2).values


def fp1(skip, init, layers, w_row0, dt):
    """fa_layer1 of one network: skip (B, npts, 256), init (B, 256) = the cloud's single-source share of the first product; the first
    layer's kernel rows w_row0.. -> (B * npts, 256)"""
    first = dict(layers[0], w=layers[0]["w"][w_row0:])
    x = layer(skip, first, True, dt, init.unsqueeze(1))
    x = layer(x, layers[1], True, dt)
    return x.reshape(-1, x.shape[-1])


def interpolate_f32(points2, idx, weight):
    """p[i1] * w1 + p[i2] * w2 + p[i3] * w3 in f32, every operation rounded, in that order.  points2 (B, m, c), idx / weight (B, n, 3)"""
    B = points2.shape[0]
    bi = torch.arange(B, device=points2.device).view(B, 1)
    ii = idx.long()
    t = [points2[bi, ii[:, :, q]] * weight[:, :, q:q + 1] for q in range(3)]
    return (t[0] + t[1]) + t[2]


def fp2(points2, idx, weight, points1, layers, dt):
    """fa_layer2 of one network: [interpolated (256) | skip (128)] -> 256 -> 128; -> (B * n, 128)"""
    x = torch.cat([interpolate_f32(points2, idx, weight), points1], dim=2)
    x = layer(x, layers[0], True, dt)
    x = layer(x, layers[1], True, dt)
    return x.reshape(-1, x.shape[-1])


def tail(points2, idx, weight, xyz, prog, dt):
    """The per-point tail of one network.  prog: [(layer, relu, out_col | None)] of the shape F H H H h+ [L h+] H H h+; rows are
    [interpolated (128) | xyz (3)].  A hidden op that follows a head block reads the trunk (op 3's output), every other op its predecessor.
    -> [(out_col, (rows, n) values)] per head block."""
    x = torch.cat([interpolate_f32(points2, idx, weight), xyz], dim=2).reshape(-1, 131)
    cur, trunk, after_head, outs = x, None, False, []
    for i, (L, relu, col) in enumerate(prog):
        if col is not None:
            outs.append((col, layer(cur, L, relu, dt)))
            after_head = True
            continue
        cur = layer(trunk if after_head else cur, L, relu, dt)
        after_head = False
        if i == 3:
            trunk = cur
    return outs


# ---- the two arithmetics as bx3.h states them ----------------------------------------------------------------------------------------
def _bf16(x):
    """f32 -> the nearest bf16 (ties to even), returned as f32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def split(x, scheme):
    """the scheme's 16-bit terms of f32 x, each as an f32 array: bf16x3 -> (hi, mid, lo), x = hi + mid + lo exactly; f16x2 -> (hi, mid),
    hi = f16(x), mid = f16((x - hi) * 2^11) kept scaled"""
    x = np.ascontiguousarray(x, np.float32)
    if scheme == "bf16x3":
        hi = _bf16(x)
        r1 = x - hi
        mid = _bf16(r1)
        return hi, mid, _bf16(r1 - mid)
    hi = x.astype(np.float16).astype(np.float32)
    return hi, ((x - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)


# products in issue order: (weight plane, activation plane, accumulator)
PRODUCTS = {"bf16x3": ((1, 1, 0), (2, 0, 0), (0, 2, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0)),      # smallest first, one accumulator
            "f16x2": ((1, 0, 1), (0, 1, 1), (0, 0, 0))}                                        # A1 += w_mid a_hi, A1 += w_hi a_mid, A0 += w_hi a_hi


def _fma32(a, b, c):
    """fma in f32: one rounding (the product of two f32 is exact in f64)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emu_layer(x, L, relu, scheme, drop=None, init=None):
    """One layer in the scheme's arithmetic.  x (rows, k) f32; L: numpy {"w", "b", "scale", "shift"}.  Per k-block of 16 channels, in
    sequence, every product of PRODUCTS[scheme] adds its 16-term dot product (16-bit x 16-bit terms: exact) to its f32 accumulator with
    one rounding; the epilogue is the kernels' folded BN: fma(A0, scale, fma(A1, scale * 2^-11, fma(bias, scale, shift))).
    drop: index of a product to leave out (a mutant); init: f32 start of accumulator 0."""
    w = np.asarray(L["w"], np.float32)
    k, n = w.shape
    kb = (k + 15) // 16
    xp = np.zeros((x.shape[0], kb * 16), np.float32)
    xp[:, :k] = x
    wp = np.zeros((kb * 16, n), np.float32)
    wp[:k] = w
    xa = [np.ascontiguousarray(p.astype(np.float64).reshape(-1, kb, 16).transpose(1, 0, 2)) for p in split(xp, scheme)]
    wa = [p.astype(np.float64).reshape(kb, 16, n) for p in split(wp, scheme)]
    prods = [(pw, pa, pc) for t, (pw, pa, pc) in enumerate(PRODUCTS[scheme]) if t != drop]
    blocks = [np.matmul(xa[pa], wa[pw]) for pw, pa, _ in prods]                          # [product][k-block] (rows, n), exact in f64
    acc = [np.zeros((x.shape[0], n), np.float32) for _ in range(2)]
    if init is not None:
        acc[0] = acc[0] + np.asarray(init, np.float32)
    for b in range(kb):
        for (_pw, _pa, pc), blk in zip(prods, blocks):
            acc[pc] = (acc[pc].astype(np.float64) + blk[b]).astype(np.float32)
    sc = np.asarray(L["scale"], np.float32)[None]
    shf = _fma32(np.asarray(L["b"], np.float32)[None], sc, np.asarray(L["shift"], np.float32)[None])
    if scheme == "f16x2":
        y = _fma32(acc[0], sc, _fma32(acc[1], sc * np.float32(1.0 / 2048.0), shf))
    else:
        y = _fma32(acc[0], sc, shf)
    return np.maximum(y, np.float32(0.0)) if relu else y


def emu_chain(x, layers, relus, scheme, drop=None):
    """a chain of layers in the scheme's arithmetic; drop = (layer index, product index) or None"""
    for i, (L, r) in enumerate(zip(layers, relus)):
        x = emu_layer(x, L, r, scheme, drop[1] if drop is not None and drop[0] == i else None)
    return x


def np_chain(x, layers, relus, dtype):
    """the same chain in plain numpy arithmetic of `dtype` (float64: the reference; float32: the yardstick)"""
    x = np.asarray(x, dtype)
    for L, r in zip(layers, relus):
        x = (x @ np.asarray(L["w"], dtype) + np.asarray(L["b"], dtype)) * np.asarray(L["scale"], dtype) + np.asarray(L["shift"], dtype)
        if r:
            x = np.maximum(x, dtype(0))
    return x


def f32_chain_kseq(x, layers, relus):
    """the chain in the arithmetic of the project's f32 kernels (the yardstick of tests/test_split16_kernels_gpu.py, pinned bit for bit
    against the CPU oracle elsewhere): per output one fmaf chain from 0, k ascending; t = acc + bias; y = fmaf(t, scale, shift)"""
    x = np.asarray(x, np.float32)
    for L, r in zip(layers, relus):
        w = np.asarray(L["w"], np.float32)
        acc = np.zeros((x.shape[0], w.shape[1]), np.float32)
        for k in range(w.shape[0]):
            acc = _fma32(x[:, k:k + 1], w[k][None], acc)
        y = _fma32(acc + np.asarray(L["b"], np.float32)[None], np.asarray(L["scale"], np.float32)[None], np.asarray(L["shift"], np.float32)[None])
        x = np.maximum(y, np.float32(0.0)) if r else y
    return x
