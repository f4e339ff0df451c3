"""GPU: ancsh_head_activations (csrc/heads.hip) on its own, on logits built here, against the float64 reference of tests/heads_ref.py.

The kernel writes every tensor the product hands out, and the forward tests hold it to 1e-4 only: an approximate exp or division (about 1e-6)
would pass them.  Here the tolerance per kind (sigmoid / tanh / softmax) is max(2 E, 2^-23), E = the error of the f32 CPU oracle (plain expf /
tanhf, IEEE division) against float64 on the very inputs of the case: the factor covers a device libm that rounds a call differently from glibc
(measured: the kernel errs by at most 1.03 E), the floor an oracle that happens to be exact.  Measured on the MI355X over all cases: E <= 8.9e-8 /
5.6e-8 / 1.9e-7, kernel 8.9e-8 / 5.4e-8 / 1.9e-7 (sigmoid / tanh / softmax).  What this does NOT catch is __expf in place of expf: the hardware
exponential is good to about an ulp, and the sigmoid's error with it is 8.89e-8 against 8.88e-8 -- no bound on the size of the error tells them apart.  Every case also pins argmax(W) / argmax(joint index) (where the
reference's two largest probabilities are further apart than the bound), gocs = float32(nocs * repeat(scale, 3)) + trans bit for bit from the
kernel's own outputs (multiply, then add, no contraction; scale o / 3 with channel o), and the column layout (each logits block draws from its own
stripes of the axis, the padding is NaN).  K = 1..8 x mixed, ragged row counts around the 256-thread block, four row strides, logits as a column
slice 4 bytes off a 16-byte boundary; every output NULL on its own and alone; saturating, denormal and non-finite logits.
tests/test_redzone_gpu.py runs all of it once more with every output guarded, and once with every output 4 bytes off."""
import functools

import numpy as np
import pytest
import torch

import heads_ref as H

pytestmark = pytest.mark.gpu

CASES = [(K, m) for K in range(1, 9) for m in (0, 1)]
ROWS = (1, 63, 255, 256, 257, 1000)
MIXED_ONLY = ("gocs", "scale", "trans")
SENTINEL = 1234.5


def width(o, K):
    return dict(W=K, nocs=3 * K, confi=1, heatmap=1, unitvec=3, axis=3, joint_cls=3, gocs=3 * K, scale=K, trans=3 * K)[o]


def launch(dev, x, K, mixed, col0=0, present=None, sentinel=()):
    """One call on the host matrix x (rows, ld); logits = x[:, col0:] (row stride ld).  Outputs come from torch.empty (the redzone arena sees
    them) pre-filled with NaN, `present` names the non-NULL ones (default: all the case has), `sentinel` those pre-filled with SENTINEL."""
    from articulated_pose_amd import _lib
    rows, ld = x.shape
    assert ld - col0 >= H.need(K, mixed)                      # the last row's logits end inside the buffer
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    names = [o for o in H.OUTPUTS if (mixed or o not in MIXED_ONLY or o in sentinel) and (present is None or o in present)]
    out = {}
    for o in names:
        out[o] = torch.empty((rows, width(o, K)), dtype=torch.float32, device=dev)
        out[o].fill_(SENTINEL if o in sentinel else float("nan"))
    _lib.call("ancsh_head_activations", rows, K, mixed, _lib.ptr(xd[:, col0:]), ld, *[_lib.ptr(out.get(o)) for o in H.OUTPUTS])
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def case(K, mixed, rows):
    """the logits of a case (rows, need), their float64 reference and the oracle's error on them: computed once, shared, read-only"""
    from oracle import oracle as O
    x = H.make_logits(np.random.RandomState(1000 * K + 100 * mixed + rows), rows, K, mixed)
    ref, E = H.reference(x, K, mixed), H.oracle_error(O, x, K, mixed)
    x.flags.writeable = False
    return x, ref, E


def padded(x, ld, col0=0):
    """x inside a (rows, ld) matrix of NaN, from column col0"""
    y = np.full((x.shape[0], ld), np.nan, np.float32)
    y[:, col0:col0 + x.shape[1]] = x
    return y


def check(out, ref, E, K, mixed, worst, tag):
    """every output of one launch against the float64 reference; worst[kind] = the largest error seen"""
    bnd = H.bounds(E)
    got = {o: t.cpu().numpy() for o, t in out.items()}
    assert set(got) == set(ref), tag
    for o in ref:
        assert got[o].shape == ref[o].shape and not np.isnan(got[o]).any(), (tag, o)
        err = float(np.abs(got[o] - ref[o]).max())
        if o == "gocs":
            assert err <= H.gocs_bound(bnd), (tag, o, err)
            continue
        worst[H.KIND[o]] = max(worst[H.KIND[o]], err)
        assert err <= bnd[H.KIND[o]], (tag, o, err, bnd[H.KIND[o]], E[H.KIND[o]])
    for o in ("W", "joint_cls"):
        clear = H.top2_margin(ref[o]) > bnd["softmax"]
        assert 1.0 - clear.mean() <= 0.01, (tag, o)
        np.testing.assert_array_equal(got[o].argmax(1)[clear], ref[o].argmax(1)[clear], err_msg="%s %s" % (tag, o))
    if mixed:
        want = (got["nocs"] * np.repeat(got["scale"], 3, axis=1)).astype(np.float32) + got["trans"]
        np.testing.assert_array_equal(got["gocs"], want, err_msg=tag)


@pytest.mark.parametrize("K,mixed", CASES)
def test_head_activations_match_float64(dev, K, mixed):
    need = H.need(K, mixed)
    worst, Emax = dict.fromkeys(H.KINDS, 0.0), dict.fromkeys(H.KINDS, 0.0)
    for rows in ROWS:
        x, ref, E = case(K, mixed, rows)
        Emax = {k: max(Emax[k], E[k]) for k in H.KINDS}
        for ld in (need, need + 1, need + 3, need + 32):
            check(launch(dev, padded(x, ld), K, mixed), ref, E, K, mixed, worst, (K, mixed, rows, ld))
        for col0 in (1, 3):                                   # a column slice of a wider tensor, 4 and 12 bytes off a 16-byte boundary
            check(launch(dev, padded(x, need + col0 + 2, col0), K, mixed, col0), ref, E, K, mixed, worst, (K, mixed, rows, "slice", col0))
    print("head_activations K=%d mixed=%d: " % (K, mixed) +
          "; ".join("%s E %.3g gpu %.3g bound %.3g" % (k, Emax[k], worst[k], H.bounds(Emax)[k]) for k in H.KINDS))


@pytest.mark.parametrize("K,mixed", CASES)
def test_optional_outputs(dev, K, mixed):
    """include/ancsh_hip.h: any output may be NULL.  Each output NULL on its own, and all NULL but one: what is present equals the all-present
    launch bit for bit.  mixed_pred = 0 with gocs / scale / trans pointers given leaves those buffers alone."""
    rows = 257
    x, _ref, _E = case(K, mixed, rows)
    x = padded(x, H.need(K, mixed) + 1)
    base = launch(dev, x, K, mixed)
    assert not any(torch.isnan(t).any() for t in base.values())
    for o in base:
        rest = launch(dev, x, K, mixed, present=[p for p in base if p != o])
        assert set(rest) == set(base) - {o}
        for p in rest:
            assert torch.equal(rest[p], base[p]), (o, "absent", p)
        alone = launch(dev, x, K, mixed, present=[o])
        assert torch.equal(alone[o], base[o]), (o, "alone")
    if not mixed:
        got = launch(dev, x, K, 0, sentinel=MIXED_ONLY)
        for o in MIXED_ONLY:
            assert bool((got[o] == SENTINEL).all()), o
        for p in base:
            assert torch.equal(got[p], base[p]), p


SIGMOID_OUT, TANH_OUT = ("nocs", "scale", "confi", "heatmap"), ("trans", "axis", "unitvec")


def test_saturating_elementwise_logits(dev, oracle):
    """+-{1e-8, 20, 87, 88, 88.8, 104, 200, 3e38} in every column: sigmoid in [0, 1], monotone, never NaN, within the absolute bound (its
    denormal results too: sigmoid(-88) = 6e-39, which the oracle returns; at -88.8 the oracle returns 0); tanh exactly +-1 from +-20 on."""
    K, mixed = 3, 1
    v = np.sort(np.array(H.SATURATING, np.float32))
    x = np.repeat(v[:, None], H.need(K, mixed), axis=1)
    ref, bnd = H.reference(x, K, mixed), H.bounds(H.oracle_error(oracle, x, K, mixed))
    got = {o: t.cpu().numpy() for o, t in launch(dev, x, K, mixed).items()}
    for o in SIGMOID_OUT:
        g = got[o]
        assert not np.isnan(g).any() and (g >= 0).all() and (g <= 1).all(), o
        assert (np.diff(g, axis=0) >= 0).all(), o
        assert g[0, 0] == 0 and g[-1, 0] == 1, o
        assert np.abs(g - ref[o]).max() <= bnd["sigmoid"], (o, np.abs(g - ref[o]).max())
    for o in TANH_OUT:
        g = got[o]
        np.testing.assert_array_equal(g[np.abs(v) >= 20], np.sign(x[np.abs(v) >= 20, :g.shape[1]]), err_msg=o)
        assert np.abs(g - ref[o]).max() <= bnd["tanh"], (o, np.abs(g - ref[o]).max())
    third = np.float32(1) / np.float32(3)                       # equal logits, 3e38 included: exp(0) / 3
    np.testing.assert_array_equal(got["W"], np.full_like(got["W"], third))
    np.testing.assert_array_equal(got["joint_cls"], np.full_like(got["joint_cls"], third))
    np.testing.assert_array_equal(got["gocs"], (got["nocs"] * np.repeat(got["scale"], 3, axis=1)).astype(np.float32) + got["trans"])


def softmax_rows(rng, c):
    """-> (one-hot rows, their hot column), (finite rows with a spread of 3e38), (rows that must come out all NaN) for a c-column softmax"""
    hot = rng.uniform(-5, 5, (c, c)).astype(np.float32)
    for j in range(c):
        hot[j, j] = np.delete(hot[j], j).max() + np.float32(200) if c > 1 else hot[j, j]
    spread = [np.zeros(c, np.float32) for _ in range(3)]
    spread[0][0] = 3e38
    spread[1][-1] = -3e38
    spread[2][:2] = 3e38
    bad = []
    for j in range(c):
        for val in (np.nan, np.inf):
            r = rng.uniform(-5, 5, c).astype(np.float32)
            r[j] = val
            bad.append(r)
    bad.append(np.full(c, -np.inf, np.float32))
    return hot, np.array(spread, np.float32), np.array(bad, np.float32)


@pytest.mark.parametrize("K,mixed", [(1, 1), (2, 0), (3, 1), (5, 0), (7, 1), (8, 0), (8, 1)])
def test_saturating_and_non_finite_softmax_rows(dev, oracle, K, mixed):
    """A logit 200 above the others gives exactly 1 and 0; a spread of 3e38 inside a finite row stays finite and sums to 1; NaN or +inf anywhere
    in a row, or a row of -inf, gives an all-NaN row of that softmax (as the oracle does) and leaves every other row, and every other output of
    the poisoned row, as in a launch without it."""
    rng = np.random.RandomState(K)
    lay = H.layout(K, mixed)
    blocks = [("W", K), ("joint_cls", 3)]
    parts = {b: softmax_rows(rng, c) for b, c in blocks}
    rows = sum(len(p) for b, _c in blocks for p in parts[b])
    clean = np.array(H.make_logits(rng, rows, K, mixed))
    x, where, r = clean.copy(), {}, 0
    changed = {b: np.zeros(rows, bool) for b, _c in blocks}    # the rows whose logits of block b were rewritten
    for b, c in blocks:
        c0 = lay[b][0]
        for name, p in zip(("hot", "spread", "bad"), parts[b]):
            x[r:r + len(p), c0:c0 + c] = p
            where[b, name] = slice(r, r + len(p))
            changed[b][r:r + len(p)] = True
            r += len(p)
    got = {o: t.cpu().numpy() for o, t in launch(dev, x, K, mixed).items()}
    base = {o: t.cpu().numpy() for o, t in launch(dev, clean, K, mixed).items()}
    for b, c in blocks:
        raw = x[:, lay[b][0]:lay[b][0] + c]
        bad = np.zeros(rows, bool)
        bad[where[b, "bad"]] = True
        bnd = H.bounds(H.oracle_error(oracle, x[~bad], K, mixed))["softmax"]
        if c > 1:
            np.testing.assert_array_equal(got[b][where[b, "hot"]], np.eye(c, dtype=np.float32), err_msg=b)
        sp = got[b][where[b, "spread"]]
        assert np.isfinite(sp).all() and np.abs(sp.sum(1, dtype=np.float64) - 1).max() <= c * bnd, (b, sp)
        assert np.abs(got[b][~bad] - H.act64(raw[~bad], "softmax")).max() <= bnd, b
        assert np.isnan(got[b][bad]).all() and np.isnan(oracle.activation(raw[bad], "softmax")).all(), b
    for o in got:                                               # every row whose logits for o were not rewritten has the clean launch's bits
        same = ~changed.get(o, np.zeros(rows, bool))
        assert not np.isnan(base[o]).any(), o
        np.testing.assert_array_equal(got[o][same], base[o][same], err_msg=o)


def test_refusals(dev):
    from articulated_pose_amd import _lib
    x = torch.zeros((4, 100), device=dev)
    for K, mixed, ld, msg in ((0, 1, 100, "outside 1..8"), (9, 0, 100, "outside 1..8"), (8, 1, 74, "ld 74 < 75"), (1, 0, 14, "ld 14 < 15")):
        with pytest.raises(ValueError, match=msg):
            _lib.call("ancsh_head_activations", 4, K, mixed, _lib.ptr(x), ld, *([None] * 10))
    with pytest.raises(ValueError, match="null logits"):
        _lib.call("ancsh_head_activations", 4, 3, 1, None, 100, *([None] * 10))
    _lib.call("ancsh_head_activations", 0, 3, 1, None, 100, *([None] * 10))          # no rows: nothing to read
