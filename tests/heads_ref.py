"""Float64 reference of ancsh_head_activations (csrc/heads.hip) and the inputs its tests run on (test infrastructure, imported by
tests/test_heads_cpu.py and tests/test_heads_gpu.py).  It never imports the package: the formulas are those of heads.hip:1-5, the column
layout that of heads.hip:35-36 -- [W (K) | nocs (3K) | scale (K) | trans (3K) | confi (1) | axis (3) | unitvec (3) | heatmap (1) |
joint_cls (3)], scale and trans only when mixed_pred."""
import collections

import numpy as np

# the entry point's output arguments, in its argument order
OUTPUTS = ("W", "nocs", "confi", "heatmap", "unitvec", "axis", "joint_cls", "gocs", "scale", "trans")
BLOCKS = ("W", "nocs", "scale", "trans", "confi", "axis", "unitvec", "heatmap", "joint_cls")      # the logits blocks, in column order
KIND = dict(W="softmax", nocs="sigmoid", scale="sigmoid", trans="tanh", confi="sigmoid", axis="tanh", unitvec="tanh", heatmap="sigmoid",
            joint_cls="softmax")
KINDS = ("sigmoid", "tanh", "softmax")
FLOOR = 2.0 ** -23       # one ulp of an output near 1: what the kernel is allowed where the oracle happens to be exact


def need(K, mixed):
    return (8 * K if mixed else 4 * K) + 11


def layout(K, mixed):
    """-> OrderedDict block -> (first column, width)"""
    widths = dict(W=K, nocs=3 * K, scale=K if mixed else 0, trans=3 * K if mixed else 0, confi=1, axis=3, unitvec=3, heatmap=1, joint_cls=3)
    out, col = collections.OrderedDict(), 0
    for b in BLOCKS:
        if widths[b]:
            out[b] = (col, widths[b])
            col += widths[b]
    assert col == need(K, mixed)
    return out


def split(logits, K, mixed):
    """logits (rows, >= need) -> {block: its raw columns}"""
    return {b: np.ascontiguousarray(logits[:, c:c + w]) for b, (c, w) in layout(K, mixed).items()}


def act64(x, kind):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "sigmoid":
            e = np.exp(-np.abs(x))                                # never overflows
            return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        if kind == "tanh":
            return np.tanh(x)
        e = np.exp(x - x.max(axis=-1, keepdims=True))             # NaN / +inf / an all -inf row -> NaN row, like the f32 formula
        return e / e.sum(axis=-1, keepdims=True)


def reference(logits, K, mixed):
    """float32 logits (rows, >= need) -> {output: float64 array}; gocs / scale / trans only when mixed"""
    raw = split(np.asarray(logits, np.float32), K, mixed)
    out = {b: act64(v, KIND[b]) for b, v in raw.items()}
    if mixed:
        out["gocs"] = out["nocs"] * np.repeat(out["scale"], 3, axis=1) + out["trans"]
    return out


def oracle_error(oracle, logits, K, mixed):
    """E per kind: max |oracle.activation (f32: expf / tanhf, IEEE division) - float64 reference| over the case's own inputs"""
    raw, ref = split(np.asarray(logits, np.float32), K, mixed), reference(logits, K, mixed)
    E = dict.fromkeys(KINDS, 0.0)
    for b, v in raw.items():
        d = np.abs(oracle.activation(v, KIND[b]).astype(np.float64) - ref[b])
        E[KIND[b]] = max(E[KIND[b]], float(np.nanmax(d)) if d.size else 0.0)
    return E


def bounds(E, factor=2.0):
    """What the kernel may err by per kind: room for a device libm that rounds a call differently from glibc, with two or three roundings per
    output.  On the MI355X the kernel's error is 0.9 to 1.03 E for every kind and every K (it is E itself for most), so twice E is ample.
    No factor separates an approximate exp from the exact one by size alone: with __expf in the sigmoid the largest error over the module's
    cases is 8.89e-8 against 8.88e-8 (E = 8.9e-8), because the hardware exponential is itself good to about an ulp."""
    return {k: max(factor * E[k], FLOOR) for k in KINDS}


def gocs_bound(bnd):
    """gocs = nocs * scale + trans against float64: both factors are <= 1, so the product errs by at most the two sigmoid errors; plus
    the tanh error; plus the two roundings of values <= 2 (2 * 2^-24 * 2)"""
    return 2 * bnd["sigmoid"] + bnd["tanh"] + 2.0 ** -22


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
STRIPE = 0.5
SPAN = dict(softmax=30.0, sigmoid=20.0, tanh=10.0)       # where the kind still moves: exp(-30) ~ 1e-13, tanh(10) = 1 - 4e-9


def make_logits(rng, rows, K, mixed, ld=None):
    """(rows, ld) float32.  Block number i of BLOCKS draws only from the stripes [(9 m + i) * STRIPE, (9 m + i + 1) * STRIPE), m any
    integer: nine disjoint combs, each covering the whole span of its kind, so no value of one block can occur in another and a block
    read at the wrong offset cannot pass.  Columns beyond need(K, mixed) are NaN: a read of the padding shows."""
    n = need(K, mixed)
    ld = n if ld is None else ld
    x = np.full((rows, ld), np.nan, np.float32)
    for b, (c, w) in layout(K, mixed).items():
        i, span = BLOCKS.index(b), SPAN[KIND[b]]
        m = rng.randint(-int(span / (9 * STRIPE)), int(span / (9 * STRIPE)), (rows, w))
        x[:, c:c + w] = ((9 * m + i + rng.uniform(0.0, 0.999, (rows, w))) * STRIPE).astype(np.float32)
    return x


def block_of(v):
    """index into BLOCKS of the stripe a finite value lies in"""
    return np.floor(np.asarray(v, np.float64) / STRIPE).astype(np.int64) % 9


def top2_margin(p):
    """(rows, c) probabilities -> the gap between the two largest per row (inf for one column)"""
    if p.shape[1] < 2:
        return np.full(p.shape[0], np.inf)
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2]


SATURATING = tuple(s * v for v in (1e-8, 20.0, 87.0, 88.0, 88.8, 104.0, 200.0, 3e38) for s in (-1.0, 1.0))
