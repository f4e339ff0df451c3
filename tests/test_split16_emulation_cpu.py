"""Where the accuracy bars of tests/test_split16_kernels_gpu.py come from -- without touching the code under test.

For the layer widths of each split-16 kernel family a 64-row tile goes through the chain in float64 (the reference), in the arithmetic of
the project's f32 kernels (one fmaf chain per output, k ascending: split16_ref.f32_chain_kseq -- the yardstick of the GPU test), in numpy's
own f32 matmul (reported only), in the faithful emulation of each scheme as csrc/bx3.h states it (split16_ref.emu_chain: the 16-term dot
product of a k-block exact, one f32 rounding per product and k-block, k-blocks in sequence) and in every single-product mutant (one
product of one layer left out).  Weights N(0, 1 / k), BN scale U(0.5, 1.5), bias and shift 0.1 N(0, 1); inputs N(0, 1), the three-channel
inputs of the set-abstraction levels U(-0.5, 0.5).

    ratio = (max |out - float64| / max |float64|) / max(the same for the f32 chain, 2^-23)

The bars are F16x2 4x and Bf16x3 2x (split16_ref.BARS): the issue that introduced these tests derived them from an emulation that summed
a layer's products in numpy's order -- faithful F16x2 0.7 .. 1.3 x and Bf16x3 0.36 .. 0.65 x the f32 evaluation's error, mutants >= 300 x and
4 .. 23 x -- i.e. with a factor two of head room under the bar and every mutant above it.

FIGURES of THIS emulation (k-blocks accumulated in sequence, one rounding per product and k-block; seeds 0 .. 5 per family, 64-row tiles;
`python tests/test_split16_emulation_cpu.py` prints them, the test itself runs seed 0):

    scheme family   faithful       smallest mutant   (layer, product) of the smallest mutants
    f16x2  sa1      0.59 .. 1.17   618 .. 976        (0, 0) (0, 1) (1, 0) (2, 0)
    f16x2  sa2      0.47 .. 0.94   428 .. 708        (0, 0) (0, 1) (1, 0)
    f16x2  sa3      0.29 .. 0.48   246 .. 374        (0, 0) (0, 1) (1, 0)
    f16x2  fp1      0.26 .. 0.49   331 .. 568        (0, 1) (1, 0) (1, 1)
    f16x2  fp2      0.31 .. 0.48   353 .. 467        (0, 0) (1, 0) (1, 1)
    f16x2  tail     0.42 .. 1.13   436 .. 543        (0, 0) (0, 1) (1, 0) (1, 1) (2, 0) (3, 0)
    bf16x3 sa1      0.59 .. 1.24   7.8 .. 12.9       (0, 0) (0, 1) (1, 1)
    bf16x3 sa2      0.63 .. 1.15   5.1 .. 9.1        (0, 0) (0, 1) (0, 2) (2, 1)
    bf16x3 sa3      0.56 .. 1.03   2.9 .. 4.3        (0, 1) (0, 2) (1, 2) (2, 1) (2, 2)
    bf16x3 fp1      0.60 .. 1.04   3.9 .. 7.0        (0, 1) (0, 2) (1, 1) (1, 2)
    bf16x3 fp2      0.52 .. 0.92   4.0 .. 5.5        (0, 0) (0, 1) (0, 2)
    bf16x3 tail     0.64 .. 0.96   5.7 .. 7.2        (0, 2) (1, 1) (1, 2) (2, 1) (2, 2)

F16x2: the separation holds as stated -- faithful at most 1.17 x (half the bar is 2), every mutant at least 246 x: the bar stays 4 x.
Bf16x3: six roundings of the accumulator per k-block against the f32 chain's sixteen put a single layer at 0.6 x the f32 chain's error
(rms); over a chain, as a ratio of two maxima, the faithful emulation scatters 0.52 .. 1.24 x: inside the bar in every draw, inside HALF
the bar (1.0) in 31 of 36.  No mutant escapes: the smallest is 2.9 x (layer3's widths, a 2^-16 product of its first layer).  By the issue's
rule for this case the Bf16x3 bar stays 2 x; what this emulation supports is a head room of 2 / 1.24 = 1.6, not 2.

Asserted per family and scheme, on seed 0: the faithful chain is at most HALF the bar and every mutant is ABOVE the bar.  On seed 0 the
Bf16x3 faithful chain is at most 0.88 x; over seeds 0 .. 5 it is not always under half the bar (five draws, up to 1.24 x, see above).
"""
import numpy as np
import pytest

import split16_ref as R

FAMILIES = {"sa1": (3, 64, 64, 128), "sa2": (3, 128, 128, 256), "sa3": (259, 256, 512, 1024), "fp1": (256, 256, 256), "fp2": (384, 256, 128),
            "tail": (131, 128, 128, 128, 32)}


def problem(name, seed=0, rows=64):
    dims = FAMILIES[name]
    rng = np.random.RandomState(1000 * seed + 7 * len(name) + dims[1])
    layers = [dict(w=(rng.randn(k, n) / np.sqrt(k)).astype(np.float32), b=(0.1 * rng.randn(n)).astype(np.float32),
                   scale=rng.uniform(0.5, 1.5, n).astype(np.float32), shift=(0.1 * rng.randn(n)).astype(np.float32))
              for k, n in zip(dims[:-1], dims[1:])]
    relus = [True] * len(layers)
    if name == "tail":
        relus[-1] = False                                        # a head block is linear
    x = (rng.uniform(-0.5, 0.5, (rows, 3)) if dims[0] == 3 else rng.randn(rows, dims[0])).astype(np.float32)
    return x, layers, relus


def figures(name, scheme, seed=0, mutants=True):
    """-> dict(faithful ratio, {(layer, product): mutant ratio}, numpy-f32 ratio)"""
    x, layers, relus = problem(name, seed)
    want = R.np_chain(x, layers, relus, np.float64)
    scale = np.abs(want).max()
    err = lambda got: float(np.abs(got.astype(np.float64) - want).max() / scale)
    yard = max(err(R.f32_chain_kseq(x, layers, relus)), R.FLOOR)
    out = dict(faithful=err(R.emu_chain(x, layers, relus, scheme)) / yard, numpy_f32=err(R.np_chain(x, layers, relus, np.float32)) / yard, mutants={})
    if mutants:
        for li in range(len(layers)):
            for t in range(len(R.PRODUCTS[scheme])):
                out["mutants"][(li, t)] = err(R.emu_chain(x, layers, relus, scheme, (li, t))) / yard
    return out


@pytest.mark.parametrize("scheme", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_bar_separates_faithful_from_mutants(name, scheme):
    bar = R.BARS[scheme]
    f = figures(name, scheme)
    lo = min(f["mutants"], key=f["mutants"].get)
    print("%s %s: faithful %.2f x the f32 chain's error (numpy's f32 matmul: %.2f), smallest mutant (layer %d, product %d) %.2f x; bar %.0f x"
          % (name, scheme, f["faithful"], f["numpy_f32"], lo[0], lo[1], f["mutants"][lo], bar))
    assert f["faithful"] <= bar / 2, (name, scheme, f["faithful"])
    escaped = {k: v for k, v in f["mutants"].items() if not v > bar}
    assert not escaped, (name, scheme, escaped)


def test_split_terms_are_what_bx3_states():
    """the emulation's operand split: bf16x3 exact with three bf16 terms, f16x2 hi = f16(x) and a scaled mid that stays below 2^15"""
    rng = np.random.RandomState(3)
    x = (rng.randn(4096) * np.exp(rng.uniform(-12, 8, 4096))).astype(np.float32)
    hi, mid, lo = R.split(x, "bf16x3")
    assert np.array_equal(hi.astype(np.float64) + mid + lo, x.astype(np.float64))
    for t in (hi, mid, lo):
        assert not (t.view(np.uint32) & 0xffff).any()                                       # 16-bit terms
    hi, mid = R.split(x, "f16x2")
    assert np.array_equal(hi, x.astype(np.float16).astype(np.float32)) and np.abs(mid).max() <= 32768
    normal = np.abs(x) >= 2.0 ** -14
    assert np.abs(hi.astype(np.float64) + mid.astype(np.float64) / 2048 - x)[normal].max() <= 2.0 ** -22 * np.abs(x[normal]).max()


if __name__ == "__main__":       # the figures of the docstring: python tests/test_split16_emulation_cpu.py
    for scheme in ("f16x2", "bf16x3"):
        for name in sorted(FAMILIES):
            fs = [figures(name, scheme, seed) for seed in range(6)]
            lo = [min(f["mutants"].items(), key=lambda kv: kv[1]) for f in fs]
            print("    %-6s %-5s faithful %.2f..%.2f   smallest mutant %.1f..%.1f (layer, product) %s" %
                  (scheme, name, min(f["faithful"] for f in fs), max(f["faithful"] for f in fs), min(v for _k, v in lo), max(v for _k, v in lo),
                   sorted(set(k for k, _v in lo))))
