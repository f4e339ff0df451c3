"""Guards the float64 reference that tests/test_heads_gpu.py holds ancsh_head_activations to (tests/heads_ref.py): a reference that shares a
mistake with the kernel proves nothing.  Against the f32 CPU oracle on the module's inputs, against torch's float64 activations on the
saturating list, and -- the column layout -- against the way net_oracle.forward splits its head outputs."""
import numpy as np
import pytest
import torch

import heads_ref as H

U = 2.0 ** -24      # half an ulp of a result in [0.5, 1): one rounding


def f32_formula_bound(kind, c):
    """Worst case of the oracle's f32 formulas against exact arithmetic, glibc's expf within 1 ulp and tanhf within 2 (its documented
    bounds).  The sample maxima over 100 000 draws of N(0, 10^2) are 8.9e-8 (sigmoid), 1.0e-7 (tanh) and 3.3e-7 (softmax over 8 columns at
    scales 1 to 60), and move by a few per cent (softmax: 30 %) with the seed, so they cannot serve as bounds themselves.
      sigmoid s = 1 / (1 + e): e's 2 U relative error reaches s scaled by s (1 - s) <= 1/4, the sum and the quotient round once each: 2.5 U
      tanh: 2 ulp of a value in [0.5, 1]: 2 U
      softmax p = e / sum over c columns: e errs by 2 U, the sum by 2 U + (c - 1) U, the quotient by U, and the f32 difference x - max by
      U |d| in the exponent, which reaches p scaled by |d| exp(-|d|) <= 0.37: (5.5 + (c - 1)) U"""
    return {"sigmoid": 2.5 * U, "tanh": 2 * U, "softmax": (5.5 + (c - 1)) * U}[kind]


@pytest.mark.parametrize("K,mixed", [(K, m) for K in range(1, 9) for m in (0, 1)])
def test_reference_agrees_with_the_f32_oracle_and_margins_hold(oracle, K, mixed):
    x = H.make_logits(np.random.RandomState(100 * K + mixed), 1000, K, mixed, H.need(K, mixed) + 3)
    assert np.isnan(x[:, H.need(K, mixed):]).all() and np.isfinite(x[:, :H.need(K, mixed)]).all()
    for i, b in enumerate(H.BLOCKS):                                    # every block inside its own stripes
        if b in H.layout(K, mixed):
            c, w = H.layout(K, mixed)[b]
            assert (H.block_of(x[:, c:c + w]) == i).all(), b
    E = H.oracle_error(oracle, x, K, mixed)
    for k in H.KINDS:
        assert E[k] <= f32_formula_bound(k, max(K, 3)), (k, E[k])
    # at most 1 % of the rows have their two largest probabilities closer than what the kernel may err by (the argmax is compared elsewhere only)
    ref, bnd = H.reference(x, K, mixed), H.bounds(E)
    for b in ("W", "joint_cls"):
        clear = H.top2_margin(ref[b]) > bnd["softmax"]
        assert 1.0 - clear.mean() <= 0.01, b
        np.testing.assert_array_equal(oracle.activation(H.split(x, K, mixed)[b], "softmax").argmax(1)[clear], ref[b].argmax(1)[clear])
    print("heads reference K=%d mixed=%d: E sigmoid %.3g tanh %.3g softmax %.3g" % (K, mixed, E["sigmoid"], E["tanh"], E["softmax"]))


def test_reference_on_the_saturating_list_equals_torch_float64(oracle):
    v = np.array(H.SATURATING, np.float32)
    t = torch.from_numpy(v).double()
    assert np.abs(H.act64(v, "sigmoid") - torch.sigmoid(t).numpy()).max() <= 1e-15
    assert np.abs(H.act64(v, "tanh") - torch.tanh(t).numpy()).max() <= 1e-15
    rows = np.array([[a, b, c] for a in v for b in v[::3] for c in v[1::5]], np.float32)
    assert np.abs(H.act64(rows, "softmax") - torch.softmax(torch.from_numpy(rows).double(), 1).numpy()).max() <= 1e-15
    assert np.abs(H.act64(v[None], "softmax") - torch.softmax(t[None], 1).numpy()).max() <= 1e-15
    # NaN anywhere, +inf anywhere, all -inf: an all-NaN row, from the reference and from the oracle alike
    for bad in ([np.nan, 0, 1], [0, np.nan, 1], [0, 1, np.nan], [np.inf, 0, 1], [0, 1, np.inf], [np.inf, np.inf, 0], [-np.inf] * 3, [np.inf, -np.inf, 0]):
        bad = np.array([bad], np.float32)
        assert np.isnan(H.act64(bad, "softmax")).all() and np.isnan(oracle.activation(bad, "softmax")).all(), bad
    one = H.act64(np.array([[-np.inf, 3.0, -np.inf]], np.float32), "softmax")          # -inf beside a finite logit is an ordinary zero
    np.testing.assert_array_equal(one, [[0.0, 1.0, 0.0]])


@pytest.mark.parametrize("K,mixed", [(3, 0), (3, 1), (7, 0), (7, 1)])
def test_reference_layout_is_the_oracle_forwards(oracle, monkeypatch, K, mixed):
    """One logits matrix through net_oracle.forward's own unpacking of its head layers (every layer before the heads stubbed out; head layer
    i returns the i-th block of the matrix, in the order the product concatenates the head kernels: fc2_0.. then fc4_0..) and through the
    reference's split: equal tensors."""
    from oracle import net_oracle
    rows = 40
    x = H.make_logits(np.random.RandomState(K), rows, K, mixed)
    widths = [K, 3 * K] + ([K, 3 * K] if mixed else []) + [1]
    cols, c = {}, 0
    for name, ws in (("nocs_net/fc2_", widths), ("joint_net/fc4_", [3, 3, 1, 3])):
        for i, w in enumerate(ws):
            cols["SPFN/%s%d" % (name, i)] = (c, w)
            c += w
    assert c == H.need(K, mixed)

    def conv(weights, scope, inp, act=True):
        if scope in cols:
            c0, w = cols[scope]
            return np.ascontiguousarray(x[None, :, c0:c0 + w])
        return inp
    monkeypatch.setattr(net_oracle, "conv", conv)
    monkeypatch.setattr(net_oracle, "sa_module", lambda *a: (None, None, {}))
    monkeypatch.setattr(net_oracle, "fp_module", lambda *a: None)
    got = net_oracle.forward({}, np.zeros((1, rows, 3), np.float32), K, mixed_pred=bool(mixed), early_split_nocs=bool(mixed))
    raw = H.split(x, K, mixed)
    want = {b: oracle.activation(v, H.KIND[b]) for b, v in raw.items()}
    names = dict(W="W", nocs="nocs_per_point", confi="confi_per_point", heatmap="heatmap_per_point", unitvec="unitvec_per_point",
                 axis="joint_axis_per_point", joint_cls="index_per_point", scale="global_scale", trans="global_translation")
    assert set(got) == set(names[b] for b in raw) | ({"gocs_per_point"} if mixed else set())
    for b in raw:
        np.testing.assert_array_equal(got[names[b]][0], want[b], err_msg=b)
    if mixed:
        np.testing.assert_array_equal(got["gocs_per_point"][0], want["nocs"] * np.repeat(want["scale"], 3, axis=1) + want["trans"])
        ref = H.reference(x, K, mixed)
        assert np.abs(got["gocs_per_point"][0] - ref["gocs"]).max() <= H.gocs_bound(H.bounds(H.oracle_error(oracle, x, K, mixed), 1.0))
