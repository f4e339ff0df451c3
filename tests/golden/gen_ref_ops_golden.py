#!/usr/bin/env python
"""Generator of tests/golden/ref_ops.json: digests (helpers.digest) of what the reference's OWN operator code computes on the seeded
inputs of the tests that hold this build to it (test_oracle_cpu, test_ops_gpu, test_nonfinite_gpu; the inputs come from those
modules' own builders, so the two cannot drift apart).

Needs what `make -C oracle ref` builds from the reference sources into oracle/_ref (never committed):
  libancsh_ref_interp.so   threenn_cpu / threeinterpolate_cpu host loops      -> the CPU entries, on any machine
  libancsh_ref_gfx950.so   tf_sampling_g.cu / tf_grouping_g.cu kernels        -> the GPU entries, only where a GPU is present
    python tests/golden/gen_ref_ops_golden.py [OUT.json]
merges what this machine can compute into OUT (default: tests/golden/ref_ops.json) and keeps the other entries."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
sys.dont_write_bytecode = True

from helpers import digest  # noqa: E402
from oracle import oracle as O  # noqa: E402


def cpu_entries():
    import test_oracle_cpu as TC
    import test_ops_gpu as TG
    import test_nonfinite_gpu as TN
    assert O.have_ref_interp(), "oracle/_ref/libancsh_ref_interp.so is not built (make -C oracle ref)"
    out = {}
    for n, m in TC.THREE_NN_SHAPES:
        for kind in TC.THREE_NN_KINDS:
            d, i = O.ref_three_nn(*TC.three_nn_inputs(kind, n, m))
            out["three_nn/%s/%d/%d/dist" % (kind, n, m)], out["three_nn/%s/%d/%d/idx" % (kind, n, m)] = digest(d), digest(i)
    for b, m, c, n in TC.INTERPOLATE_CASES:
        pts, x1, x2, w2, i2 = TC.interpolate_inputs(b, m, c, n)
        key = "three_interpolate/%d/%d/%d/%d" % (b, m, c, n)
        d, i = O.ref_three_nn(x1, x2)
        out[key + "/dist"], out[key + "/idx"] = digest(d), digest(i)
        out[key + "/out"] = digest(O.ref_three_interpolate(pts, i, O.three_weights(d)))
        out[key + "/out_arbitrary"] = digest(O.ref_three_interpolate(pts, i2, w2))
    for n, m in TG.REF_LOOP_SHAPES:
        for kind in TG.REF_LOOP_KINDS:
            x1, x2, pts = TG.ref_loop_inputs(n, m, kind)
            key = "loops/%s/%d/%d" % (kind, n, m)
            d, i = O.ref_three_nn(x1, x2)
            out[key + "/dist"], out[key + "/idx"] = digest(d), digest(i)
            out[key + "/out"] = digest(O.ref_three_interpolate(pts, i, O.three_weights(d)))
    for n, m in TN.THREE_NN_SHAPES:
        d, i = O.ref_three_nn(*TN.three_nn_inputs(n, m))
        out["nonfinite_three_nn/%d/%d/dist" % (n, m)], out["nonfinite_three_nn/%d/%d/idx" % (n, m)] = digest(d), digest(i)
    return out


def gpu_entries():
    import torch
    import test_ops_gpu as TG
    import test_nonfinite_gpu as TN
    so = os.path.join(ROOT, "oracle", "_ref", "libancsh_ref_gfx950.so")
    assert os.path.exists(so), "oracle/_ref/libancsh_ref_gfx950.so is not built (make -C oracle ref)"
    ref = ctypes.CDLL(so)
    dev = torch.device("cuda:0")
    vp = ctypes.c_void_p
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=dev)

    def fps(x, m):
        b, n, _ = x.shape
        xt, out, temp = T(x), Z((b, m)), Z((32, n), torch.float32)
        assert ref.ref_farthest_point_sample(b, n, m, vp(xt.data_ptr()), vp(temp.data_ptr()), vp(out.data_ptr())) == 0
        return out

    def ball(x, q, r, ns):
        b, n, _ = x.shape
        m = q.shape[1]
        xt, qt, idx, cnt = T(x), T(q), Z((b, m, ns)), Z((b, m))
        assert ref.ref_query_ball_point(b, n, m, ctypes.c_float(r), ns, vp(xt.data_ptr()), vp(qt.data_ptr()), vp(idx.data_ptr()),
                                        vp(cnt.data_ptr())) == 0
        return idx, cnt

    out = {}
    for n, m in TG.FPS_SHAPES:
        for kind in TG.FPS_KINDS:
            out["fps_kernel/%s/%d/%d" % (kind, n, m)] = digest(fps(TG.fps_kernel_inputs(kind, n, m), m))
    for n, m, r, ns in TG.BALL_SHAPES:
        for kind in TG.BALL_KINDS:
            x, q, feats = TG.ball_kernel_inputs(O, kind, n, m, r, ns)
            key = "ball_kernel/%s/%d/%d/%g/%d" % (kind, n, m, r, ns)
            idx, cnt = ball(x, q, r, ns)
            ft, g = T(feats), Z((5, m, ns, 16), torch.float32)
            assert ref.ref_group_point(5, n, 16, m, ns, vp(ft.data_ptr()), vp(idx.data_ptr()), vp(g.data_ptr())) == 0
            out[key + "/idx"], out[key + "/cnt"], out[key + "/group"] = digest(idx), digest(cnt), digest(g)
    out["fps_large/coarse"] = digest(fps(TG.fps_large_inputs("coarse"), 40))
    for n, m in TG.PROB_SHAPES:
        p, r = TG.prob_sample_inputs(n, m)
        pt, rt, temp, idx = T(p), T(r), Z((3, n), torch.float32), Z((3, m))
        assert ref.ref_prob_sample(3, n, m, vp(pt.data_ptr()), vp(rt.data_ptr()), vp(temp.data_ptr()), vp(idx.data_ptr())) == 0
        out["prob_sample/%d/%d/cdf" % (n, m)], out["prob_sample/%d/%d/idx" % (n, m)] = digest(temp), digest(idx)
    for n, m, k in TG.TOP_K_SHAPES:
        dist, _ = TG.top_k_inputs(n, m, k)
        dt, ri, ro = T(dist), Z((2, m, n)), Z((2, m, n), torch.float32)
        assert ref.ref_selection_sort(2, n, m, k, vp(dt.data_ptr()), vp(ri.data_ptr()), vp(ro.data_ptr())) == 0
        out["top_k/%d/%d/%d/idx" % (n, m, k)], out["top_k/%d/%d/%d/dist" % (n, m, k)] = digest(ri), digest(ro)
    for n, m in TN.FPS_SHAPES:
        for what in TN.WHATS:
            out["nonfinite_fps/%s/%d/%d" % (what, n, m)] = digest(fps(TN.fps_inputs(what, n, m), m))
    for n, m, r, ns in TN.BALL_SHAPES:
        for what in TN.WHATS:
            idx, cnt = ball(*TN.ball_inputs(O, what, n, m, r, ns), r, ns)
            key = "nonfinite_ball/%s/%d/%d/%g/%d" % (what, n, m, r, ns)
            out[key + "/idx"], out[key + "/cnt"] = digest(idx), digest(cnt)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ref_ops.json")
    got = json.load(open(path)) if os.path.exists(path) else {}
    got.update(cpu_entries())
    import torch
    if torch.cuda.is_available():
        got.update(gpu_entries())
    with open(path, "w") as f:
        json.dump(dict(sorted(got.items())), f, indent=0)
        f.write("\n")
    print("%d digests in %s" % (len(got), path))
