#!/usr/bin/env python
"""bench.py -- point-clouds/sec of the ANCSH hot path on N MI355X of one node.

    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: starts its own N ranks, one per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic clouds PER RANK (weak scaling:
batch 32 per GPU, independent clouds, no data-path collective; one RCCL gather of the result records to
rank 0 closes each step when N > 1).  Inputs are resident in HBM before the timed region.  Prints ONE
JSON line on rank 0 (see DESIGN.md "Measurement" for every field).

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line.  `--full` adds every side
measurement after the timed steps (per-kernel roofline, op-level figures, the other configurations and precisions, the
latency leg, the CPU baseline).
"""
import argparse
import json
import os
import sys
import time

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import articulated_pose_amd  # noqa: E402,F401  (import shim)
from articulated_pose_amd import _lib  # noqa: E402
from articulated_pose_amd.network import AncshEngine, Network  # noqa: E402
from articulated_pose_amd.pipeline import AncshPipeline  # noqa: E402
from articulated_pose_amd.synthetic import make_batch, make_cloud, make_predictions  # noqa: E402
from articulated_pose_amd.weights import synthetic_weights  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak (= f32 vector peak)
MFMA_16BIT_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense bf16 / f16 MFMA peak (measured here: 2.48 PF, profiles/r06_mfma_bf16_microbench.txt)
SPLIT16_PRODUCTS = {"bf16x3": 6, "f16x2": 3}      # 16-bit MFMA products executed per f32 product (csrc/bx3.h)


def kernel_work(name, a):
    """Algorithmic bytes / flops of one ABI call from its arguments (SURVEY.md 8d formulas:
    every input read once, every output written once, 4 B per element)."""
    for scheme in SPLIT16_PRODUCTS:
        # the split-16 experiment's entry points take their f32 counterparts' leading arguments: the same f32-EQUIVALENT flops,
        # in a family of their own ("<family> [f16x2]") that roofline_from_profile prices against the 16-bit matrix peak
        tag = "_" + scheme
        if tag in name and not name.startswith("ancsh_sa_pack_weights"):
            f, by, fl = kernel_work(name.replace(tag, ""), a)
            return "%s [%s]" % (f, scheme), by, fl
    if name == "ancsh_query_ball_point":
        b, n, m, _r, ns = a[:5]
        return "ball_query+group", 4.0 * b * (3 * n + 3 * m + m * ns + m), 0.0
    if name in ("ancsh_group_point", "ancsh_group_point_ex"):
        b, n, c, m, ns = a[:5]
        return "ball_query+group", 4.0 * b * (n * c + m * ns + m * ns * c), 0.0
    if name in ("ancsh_farthest_point_sample", "ancsh_farthest_point_sample_gather"):
        b, n, m = a[:3]
        return "fps", 4.0 * b * (3 * n + m + (3 * m if name.endswith("gather") else 0)), 0.0
    if name in ("ancsh_three_nn", "ancsh_three_nn_weights"):
        b, n, m = a[:3]
        POSE_WORK["nn_tests"] = POSE_WORK.get("nn_tests", 0.0) + float(b) * n * m       # pair tests of the launch
        POSE_WORK["nn_launches"] = POSE_WORK.get("nn_launches", 0) + 1
        return "three_nn+interpolate", 4.0 * b * (3 * n + 3 * m + 6 * n + (3 * n if name.endswith("weights") else 0)), 0.0
    if name == "ancsh_three_weights":
        return "three_nn+interpolate", 4.0 * a[0] * 6, 0.0
    if name in ("ancsh_fp_interpolate_concat", "ancsh_fp_interpolate_concat_ex"):
        b, m, c2, n = a[:4]
        c1, ld = a[8], a[10]
        geo, p1b = (a[11], a[12]) if name.endswith("_ex") else (b, b)      # grouped: the 3-NN arrays / points1 of fewer clouds are shared
        return "three_nn+interpolate", 4.0 * (b * m * c2 + geo * 6 * n + p1b * n * c1 + b * n * ld), 0.0
    if name in ("ancsh_three_interpolate", "ancsh_three_interpolate_ex"):
        b, m, c, n = a[:4]
        return "three_nn+interpolate", 4.0 * b * (m * c + 6 * n + n * c), 0.0
    if name == "ancsh_sa_pack_weights":
        return "weight_prep(once)", 8.0 * a[0] * a[1], 0.0
    if name in ("ancsh_conv1x1", "ancsh_conv1x1_ex", "ancsh_conv1x1_packed"):      # executed flops (the single-source FP shortcut runs fewer than the reference graph)
        rows, cin, cout = a[:3]
        pool = a[12]
        if name == "ancsh_conv1x1" and rows <= 64 and a[9] == 2:
            # the per-cloud partial product of the single-source FP shortcut: a latency-bound VALU fmaf chain on <= 64 rows,
            # not an MFMA launch -- kept out of the MFMA family so that family's TFLOP/s is that of the matrix kernels
            return "fp_partial_product(valu)", 0.0, 0.0
        return "shared_mlp_conv1x1", 4.0 * (rows * cin + cin * cout + (rows // pool if pool else rows) * cout), 2.0 * rows * cin * cout
    if name == "ancsh_conv1x1_packed_grouped":     # the same layer of several networks in one launch: the sum of the plain calls
        g, rows, cin, cout = a[:4]
        pool = a[13]
        return "shared_mlp_conv1x1", 4.0 * g * (rows * cin + cin * cout + (rows // pool if pool else rows) * cout), 2.0 * g * rows * cin * cout
    if name == "ancsh_conv1x1_grouped":
        return "fp_partial_product(valu)", 0.0, 0.0
    # round 5: the mid-section chains (csrc/mid_chain.hip) stay in the conv1x1 family -- they ARE layer3 / fa_layer1 / fa_layer2's
    # conv stacks, now one launch per level -- so that the family's figure compares like for like with rounds 1-4
    if name == "ancsh_sa3_chain_grouped":
        g, b, npts, cf, c1, c2, c3 = a[:7]
        return ("shared_mlp_conv1x1", 4.0 * (b * npts * 3 + g * b * npts * cf + g * b * (npts // 32) * c3),
                2.0 * g * b * npts * ((3 + cf) * c1 + c1 * c2 + c2 * c3))
    if name == "ancsh_fp1_chain_grouped":
        g, b, npts, ck, c1, c2 = a[:6]
        return "shared_mlp_conv1x1", 4.0 * (g * b * npts * (ck + c2) + g * b * c1), 2.0 * g * b * npts * (ck * c1 + c1 * c2)
    if name == "ancsh_fp2_chain_grouped":
        g, b, m, n, c2, c1, n1, n2 = a[:8]
        return ("shared_mlp_conv1x1", 4.0 * (g * b * m * c2 + b * n * 6 + g * b * n * (c1 + n2)),
                2.0 * g * b * n * ((c2 + c1) * n1 + n1 * n2))
    if name == "ancsh_fp_single_source_init":
        return "fp_partial_product(valu)", 0.0, 0.0
    if name == "ancsh_sa_module_fused_grouped":
        g, b, n, m, ns, cf, c1, c2, c3 = a[:9]
        rows = g * b * m * ns
        return "shared_mlp_fused_sa", 4.0 * (b * n * 3 + g * b * n * cf + b * m * ns + g * b * m * c3), 2.0 * rows * ((3 + cf) * c1 + c1 * c2 + c2 * c3)
    if name == "ancsh_sa_module_fused_partial_grouped":
        g, b, n, m, ns, c1, c2, c3 = a[:8]
        rows = g * b * m * ns
        return "shared_mlp_fused_sa", 4.0 * (b * n * 3 + g * b * n * c1 + b * m * ns + g * b * m * c3), 2.0 * rows * (3 * c1 + c1 * c2 + c2 * c3)
    if name == "ancsh_sa_module_fused":
        b, n, m, ns, cf, c1, c2, c3 = a[:8]
        rows = b * m * ns
        # fused gather + 3 MLP layers + max: algorithmic FLOPs of the three 1x1 convolutions
        return "shared_mlp_fused_sa", 4.0 * (b * n * (3 + cf) + b * m * ns + b * m * c3), 2.0 * rows * ((3 + cf) * c1 + c1 * c2 + c2 * c3)
    if name == "ancsh_sa_module_fused_partial":
        # EXECUTED flops: the first layer's feature part was summed once per source point by an ancsh_conv1x1 launch (counted
        # there); here that layer only adds the three coordinate terms per neighbour
        b, n, m, ns, c1, c2, c3 = a[:7]
        rows = b * m * ns
        return "shared_mlp_fused_sa", 4.0 * (b * n * (3 + c1) + b * m * ns + b * m * c3), 2.0 * rows * (3 * c1 + c1 * c2 + c2 * c3)
    if name == "ancsh_mlp_chain":
        return "shared_mlp_chain_tail", 0.0, float(CHAIN_FLOPS.get((a[0], a[4]), 0.0))
    if name == "ancsh_mlp_chain_grouped_fp":    # the same chains with fa_layer3's interpolation in the tile load: a[0] networks x a[1] clouds x a[2] points
        rows = a[1] * a[2]
        return "shared_mlp_chain_tail", 0.0, float(sum(CHAIN_FLOPS.get((rows, n), 0.0) for n in ((11, 8)[:a[0]] if a[0] > 1 else GROUPED_CHAIN_OPS)))
    if name == "ancsh_mlp_chain_grouped":       # a[0] networks in one launch: ANCSH (11 ops) first, NPCS (8 ops) second (paired.py)
        return "shared_mlp_chain_tail", 0.0, float(sum(CHAIN_FLOPS.get((a[1], n), 0.0) for n in ((11, 8)[:a[0]] if a[0] > 1 else GROUPED_CHAIN_OPS)))
    if name == "ancsh_group_max":
        g, ns, c = a[:3]
        return "group_max", 4.0 * (g * ns * c + g * c), 0.0
    if name == "ancsh_head_activations":
        rows, K, mixed = a[:3]
        return "head_activations", 4.0 * rows * (a[4] + 11 + (11 if mixed else 3) * K), 0.0
    if name in ("ancsh_ransac_single", "ancsh_ransac_single_ex", "ancsh_ransac_single_rec"):       # a[0] problems (cloud x part) x a[5] hypotheses, each verified on its part's points
        POSE_WORK["single_hyp"] = float(a[0]) * a[5]
        POSE_WORK["single_res"] = float(a[5]) * POSE_WORK.get("rows", 0)
        return "pose_ransac_single", 0.0, 0.0
    if name in ("ancsh_ransac_joint", "ancsh_ransac_joint_ex", "ancsh_ransac_joint_rec"):        # a[0] problems (cloud x joint) x a[7] hypotheses = one 6-parameter LM fit each
        POSE_WORK["joint_fits"] = float(a[0]) * a[7]
        return "pose_ransac_joint_lm", 0.0, 0.0
    if name in ("ancsh_pose_partition", "ancsh_pose_joint_direction", "ancsh_pose_poison_records"):
        return "pose_partition+median", 0.0, 0.0
    return name, 0.0, 0.0


GROUPED_CHAIN_OPS = [11]     # op count of a single-network grouped chain launch (--workload net: the ANCSH program)
CHAIN_FLOPS = {}     # (rows, nops) -> FLOPs of an ancsh_mlp_chain launch (filled from the layer table in main())
POSE_WORK = {}       # work counts of the pose-fit launches of one step (filled by kernel_work and main())


def chain_flops(rows, K, mixed):
    """FLOPs of the fused tail: fa_layer3 (131->128->128->128), fc1, nocs heads, joint heads."""
    macs = 131 * 128 + 3 * 128 * 128                       # fa_layer3 + fc1
    macs += 128 * ((8 * K + 1) if mixed else (4 * K + 1))  # fc2_* heads
    if mixed:
        macs += 128 * 128                                  # fc11_1
    macs += 2 * 128 * 128 + 128 * 10                       # fc3_0, fc3_1, fc4_*
    return 2.0 * rows * macs


CSRC = os.path.join(ROOT, "articulated-pose_amd", "csrc")
# kernel family -> the sources whose change invalidates a PMC measurement of that family (common.h: every kernel)
FAMILY_SOURCES = {
    "fps": ("sampling.hip",), "ball_query+group": ("grouping.hip",), "three_nn+interpolate": ("interpolate.hip",),
    "shared_mlp_fused_sa": ("sa_fused.hip", "wave_mlp.h"), "shared_mlp_chain_tail": ("chain.hip", "wave_mlp.h"),
    "shared_mlp_conv1x1": ("mlp.hip", "conv_packed.hip", "conv_rowtile.hip", "mid_chain.hip", "wave_mlp.h"), "head_activations": ("heads.hip",),
}


def source_digests():
    """sha256 (first 16 hex digits) of every kernel source: what tools/pmc_to_traffic.py stamps a PMC pass with."""
    import hashlib
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".cpp")):
            out[f] = hashlib.sha256(open(os.path.join(CSRC, f), "rb").read()).hexdigest()[:16]
    return out


def _pmc_file():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")))
    if not files:
        return None, {}
    try:
        return os.path.basename(files[-1]), json.load(open(files[-1]))
    except Exception:
        return None, {}


def pmc_entry(key, sources, table=None):
    """A committed PMC figure, valid only while the kernel sources it was measured on are unchanged: the PMC file carries the
    digests of csrc/ at collection time (`source_digests`) and the commit; a family whose sources differ now reports null."""
    name, d = _pmc_file()
    val = (d.get(table, {}) if table else d).get(key)
    if val is None:
        return None
    stamp, now = d.get("source_digests"), source_digests()
    if not stamp or any(stamp.get(f) != now.get(f) for f in tuple(sources) + ("common.h",)):
        return None
    return val


def pmc_traffic():
    """HBM bytes per launch per kernel family from the committed PMC passes (profiles/*_pmc_traffic.json: rocprofv3
    --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate runs, gfx950 x2 read correction).  PMC counters cannot be
    collected inside the timed run, so `traffic` is the latest committed measurement -- of the SAME kernel sources (see
    pmc_entry), else null."""
    _name, d = _pmc_file()
    return {f: pmc_entry(f, FAMILY_SOURCES.get(f, ()), "hbm_bytes_per_launch") for f in d.get("hbm_bytes_per_launch", {})}


def pmc_provenance():
    """Which committed PMC pass `traffic` comes from.  stale_sources: sources of the kernel FAMILIES that carry a traffic figure
    (FAMILY_SOURCES + common.h) that changed since the pass -- those families report null; other_changed_sources: the rest of csrc/
    (evaluation metrics, the copy yardstick, the ABI version string ...: no kernel of the step), listed so that nothing is hidden."""
    name, d = _pmc_file()
    if name is None:
        return None
    changed = sorted(f for f, h in source_digests().items() if (d.get("source_digests") or {}).get(f) != h)
    fam = {f for v in FAMILY_SOURCES.values() for f in v} | {"common.h"}
    out = {"file": "profiles/" + name, "commit": d.get("commit"), "stale_sources": [f for f in changed if f in fam]}
    other = [f for f in changed if f not in fam]
    if other:
        out["other_changed_sources"] = other
    return out


def rocprof_roofline():
    """The committed rocprofv3 summary of the driver's exact command (profiles/*_rocprof_roofline.json, written by
    tools/summarise_profiles.py from `rocprofv3 --kernel-trace --stats -- python bench.py`): average launch durations over the
    whole command -- graph replays with 16 batches in flight, where kernels of other batches share the chip -- and the fraction
    they give.  Reported next to the in-process HIP-event figure (same launches issued eagerly, alone on the chip)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_rocprof_roofline.json")))
    if not files:
        return None
    try:
        d = json.load(open(files[-1]))
        return {"file": os.path.basename(files[-1]), "sa1_fused_us": round(d["sa1_fused_us"], 1), "sa2_fused_us": round(d["sa2_fused_us"], 1),
                "achieved": d["shared_mlp_fused_sa"]["achieved_TFLOPs"], "frac": d["shared_mlp_fused_sa"]["frac"],
                "sa_steady": d.get("sa_steady"), "slots1": d.get("slots1"),
                "dispatches_running_at_once": d.get("dispatches_running_at_once_in_the_pipelined_step"),
                "note": "sa1/sa2_fused_us, achieved, frac: average over all launches of the rocprof'd 20-batches-in-flight command -- NOT an exclusive "
                        "duration: several dispatches of different batches run at once (see dispatches_running_at_once) and time-share the SIMDs, which "
                        "stretches every kernel's start-to-end time while the step time stays what `ms_per_step` says; slots1 = the same kernels with ONE "
                        "batch in flight (alone on the chip, in step order); sa_steady = rocprofv3 averages of tools/sa_steady.py (the same two launches "
                        "alone, back-to-back); roofline.frac is the same kernels timed in this process with HIP events"}
    except Exception:
        return None


def roofline_from_profile(records, passes):
    traffic = pmc_traffic()
    fam = {}
    for name, a, ms in records:
        f, by, fl = kernel_work(name, a)
        d = fam.setdefault(f, dict(ms=0.0, bytes=0.0, flops=0.0, launches=0))
        d["ms"] += ms
        d["bytes"] += by
        d["flops"] += fl
        d["launches"] += 1
    out = {}
    for f, d in fam.items():
        ms = d["ms"] / passes
        scheme = f[f.index("[") + 1:-1] if f.endswith("]") and "[" in f else None
        if scheme in SPLIT16_PRODUCTS and d["flops"] > 0:
            # a split-16 family: `achieved` = the 16-bit matrix flops it EXECUTES (products per f32 product x the f32-equivalent flops)
            # against the dense 16-bit peak; the f32-equivalent rate next to it (what the same layers would need on the f32 pipe)
            eq = d["flops"] / passes / (ms * 1e-3) / 1e12
            ach = eq * SPLIT16_PRODUCTS[scheme]
            out[f] = dict(bound="mfma", achieved=round(ach, 1), peak=MFMA_16BIT_PEAK_TFLOPS, unit="TFLOP/s", frac=round(ach / MFMA_16BIT_PEAK_TFLOPS, 4),
                          products_per_f32_product=SPLIT16_PRODUCTS[scheme], f32_equivalent_TFLOPs=round(eq, 2),
                          f32_equivalent_over_f32_peak=round(eq / MFMA_F32_PEAK_TFLOPS, 4), traffic=None,
                          ms_per_step=round(ms, 4), launches_per_step=d["launches"] // passes)
        elif d["flops"] > 0:
            ach = d["flops"] / passes / (ms * 1e-3) / 1e12
            out[f] = dict(bound="mfma", achieved=round(ach, 3), peak=MFMA_F32_PEAK_TFLOPS, unit="TFLOP/s",
                          frac=round(ach / MFMA_F32_PEAK_TFLOPS, 4), traffic=traffic.get(f),
                          ms_per_step=round(ms, 4), launches_per_step=d["launches"] // passes)
        elif d["bytes"] == 0:
            # pose fitting: <= 24 KB of points per part live in LDS/registers; ALU/latency-bound, no HBM or
            # MFMA roofline applies -- reported by time share only
            out[f] = dict(bound="alu", achieved=None, peak=None, unit=None, frac=None, traffic=None,
                          ms_per_step=round(ms, 4), launches_per_step=d["launches"] // passes)
            sec = ms * 1e-3
            if f == "pose_ransac_single" and POSE_WORK.get("single_hyp"):
                # stage A (score + refit kernels): every hypothesis = one 3-point Kabsch/scale fit + one residual per point of
                # its part; the part's points are staged ONCE per workgroup into an LDS tile and every residual reads LDS
                out[f].update(achieved=round(POSE_WORK["single_hyp"] / sec / 1e9, 3), unit="G hypotheses/s",
                              point_residuals_per_s=round(POSE_WORK["single_res"] / sec, 1),
                              hypotheses_per_step=POSE_WORK["single_hyp"], lds_resident_fraction=1.0)
            if f == "pose_ransac_joint_lm" and POSE_WORK.get("joint_fits"):
                out[f].update(achieved=round(POSE_WORK["joint_fits"] / sec / 1e6, 3), unit="M LM fits/s",
                              lm_fits_per_step=POSE_WORK["joint_fits"],
                              lm_evaluations_per_step=POSE_WORK.get("lm_evals"),
                              lm_evaluations_per_s=(round(POSE_WORK["lm_evals"] / sec, 1) if POSE_WORK.get("lm_evals") else None),
                              lds_resident_fraction=1.0)
        else:
            ach = d["bytes"] / passes / (ms * 1e-3) / 1e9
            # FPS is a chain of npoint-1 dependent arg-max rounds over a register-resident cloud (one workgroup per cloud):
            # latency-bound by construction; its GB/s is reported for completeness, not as a roofline claim
            out[f] = dict(bound="latency" if f == "fps" else "hbm", achieved=round(ach, 2), peak=HBM_PEAK_GBS, unit="GB/s",
                          frac=round(ach / HBM_PEAK_GBS, 4), traffic=traffic.get(f),
                          ms_per_step=round(ms, 4), launches_per_step=d["launches"] // passes)
            if f == "three_nn+interpolate" and POSE_WORK.get("nn_launches") == d["launches"]:
                # since round 5 both interpolations happen inside chain loads: what is left of the family is the two 3-NN searches, n x m
                # distance tests + a top-3 cascade each with 36 B of output per query -- vector-issue-bound, the HBM figure is kept for
                # continuity but is not its roofline
                out[f].update(bound="alu", frac=None, pair_tests_per_s=round(POSE_WORK["nn_tests"] / d["launches"] * (d["launches"] // passes) / (ms * 1e-3), 1),
                              note="3-NN searches only (the interpolations are fused into the fa_layer2 / tail chain loads): n x m distance tests + "
                                   "top-3 cascade per query, vector-issue-bound; `achieved` (GB/s of the 12n + 12m + 36n algorithmic bytes) kept for continuity")
    return out


YARDSTICK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "microbench")
_yardstick_lib = None


def yardstick():
    """tools/microbench/libyardstick.so: the float4-copy HBM yardstick (a measurement aid with its own .so, NOT in the product library).
    Built by __graft_entry__.build(); a missing file is an error, not a silent skip."""
    global _yardstick_lib
    if _yardstick_lib is None:
        import ctypes
        path = os.path.join(YARDSTICK_DIR, "libyardstick.so")
        if not os.path.exists(path):       # normally built by __graft_entry__.build(); hipcc is on every box this runs on
            import subprocess
            subprocess.run(["make", "-s", "-C", YARDSTICK_DIR], check=False, capture_output=True)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing and `make -C tools/microbench` did not produce it")
        L = ctypes.CDLL(path)
        L.yardstick_hbm_copy.restype = ctypes.c_int
        L.yardstick_hbm_copy.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _yardstick_lib = L
    return _yardstick_lib


def _hbm_copy(n, a, b):
    if yardstick().yardstick_hbm_copy(n, a.data_ptr(), b.data_ptr(), torch.cuda.current_stream().cuda_stream) != 0:
        raise RuntimeError("yardstick_hbm_copy failed (reason on stderr)")


def measured_hbm_copy(dev, mib=1024, reps=20):
    """GB/s of a float4 copy between two `mib`-MiB buffers (far beyond the 256 MiB Infinity Cache): bytes read + bytes written over
    the time of `reps` back-to-back launches (HIP events).  The achievable-HBM figure of this very device, next to the 8.0 TB/s spec."""
    n = mib << 20
    a = torch.empty(n, dtype=torch.uint8, device=dev).fill_(1)
    b = torch.empty(n, dtype=torch.uint8, device=dev)
    for _ in range(3):
        _hbm_copy(n, a, b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _hbm_copy(n, a, b)
    e1.record()
    torch.cuda.synchronize()
    return round(2.0 * n * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)


def op_level_ball_group(P, B, N, dev, mode="five", sets=1, reps=None):
    """North-star op-level figure: the reference's UNFUSED operator pair -- query_ball_point + group_point for both SA
    levels -- replayed from a hipGraph and timed with HIP events on its stream.  The end-to-end path does NOT run these
    group kernels: the fused SA kernel gathers straight into LDS.
      mode "five"  : the GRADED figure -- five separate launches in dependency order (BQ1, group(xyz), BQ2, group(xyz),
                     group(features)); algorithmic bytes per cloud: SURVEY.md 8d (5 355 520 B at N = 1024);
      mode "five_dag": the same five launches on the operators' own dependency DAG -- level 2's ball query needs the level-1 centroids, not
                     level 1's ball query, so [BQ1 -> group(xyz)] and [BQ2 -> group(xyz), group(features)] run on two streams of the
                     captured graph, joined before the next operand set (measured 0.35 / 0.49 of 8 TB/s at 16 x 2048 / 32 x 1024
                     against 0.30 / 0.44 in a line: the fork and the join cost what a launch floor costs);
      mode "multi" : the same five operator results from TWO launches -- both ball queries in one
                     (ancsh_query_ball_point_multi: level 2 only needs the level-1 centroids), all three groupings in one
                     (ancsh_group_point_multi: both xyz groupings and the feature grouping); same byte numerator (every operand
                     still moves; three launches until round 3);
      mode "fused" : ancsh_query_ball_group_xyz (ball query + xyz grouping in one launch, the hit lane still holds the
                     candidate's coordinates) + group_point(features): its OWN byte numerator -- the xyz groupings no
                     longer re-read idx (4*m*ns) nor the cloud (12*n).
      sets         : independent operand sets (inputs AND outputs in separate allocations, point order reshuffled per set) one
                     replay walks through.  One set is ~180 MB at 32 x 1024 and replaying it stays inside the 256 MiB Infinity
                     Cache (MI355X_MICROARCH.md: "scale past L3"); with `sets` >= 8 a lap touches >= 1.4 GB before a buffer
                     comes round again, so every byte is served by HBM.  The byte numerator does not change."""
    from articulated_pose_amd import tf_ops
    from articulated_pose_amd.tf_ops.tf_sampling import farthest_point_sample_gather
    gen = torch.Generator(device="cpu").manual_seed(4321)
    operands = []
    for k in range(max(1, sets)):
        Pk = P if k == 0 else P[:, torch.randperm(N, generator=gen).to(dev)].roll(k, 0).contiguous()
        _, l1 = farthest_point_sample_gather(512, Pk)
        _, l2 = farthest_point_sample_gather(128, l1)
        operands.append((Pk, l1, l2, torch.randn(B, 512, 128, device=dev)))

    def run(Pk, l1, l2, f1):
        if mode == "fused":
            _i1, _c1, g1 = tf_ops.query_ball_group_xyz(0.2, 64, Pk, l1)
            idx2, _c2, g2 = tf_ops.query_ball_group_xyz(0.4, 64, l1, l2)
            return g1, g2, tf_ops.group_point(f1, idx2)
        if mode == "fused_multi":
            (_i1, _c1, g1), (idx2, _c2, g2) = tf_ops.query_ball_group_xyz_multi([(0.2, 64, Pk, l1), (0.4, 64, l1, l2)])
            return g1, g2, tf_ops.group_point(f1, idx2)
        if mode == "multi":
            (idx1, _), (idx2, _) = tf_ops.query_ball_point_multi([(0.2, 64, Pk, l1), (0.4, 64, l1, l2)])
            return tuple(tf_ops.group_point_multi([(Pk, idx1), (l1, idx2), (f1, idx2)]))
        if mode == "five_dag":
            # the five operators, five launches, on the operators' own dependency DAG: level 2's ball query needs the level-1 centroids,
            # not level 1's ball query -> [BQ1 -> group(xyz)] on the stream, [BQ2 -> group(xyz), group(features)] on a second one, joined
            # before the next operand set starts (sets never overlap)
            fork, join = torch.cuda.Event(), torch.cuda.Event()
            fork.record(st)
            with torch.cuda.stream(st2):
                st2.wait_event(fork)
                idx2, _ = tf_ops.query_ball_point(0.4, 64, l1, l2)
                g2 = tf_ops.group_point(l1, idx2)
                gf = tf_ops.group_point(f1, idx2)
                join.record(st2)
            idx1, _ = tf_ops.query_ball_point(0.2, 64, Pk, l1)
            g1 = tf_ops.group_point(Pk, idx1)
            st.wait_event(join)
            return g1, g2, gf
        idx1, _ = tf_ops.query_ball_point(0.2, 64, Pk, l1)
        g1 = tf_ops.group_point(Pk, idx1)
        idx2, _ = tf_ops.query_ball_point(0.4, 64, l1, l2)
        return g1, tf_ops.group_point(l1, idx2), tf_ops.group_point(f1, idx2)

    st = torch.cuda.Stream(device=dev)
    st2 = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        for _ in range(2):
            for o in operands:
                run(*o)
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        keep = [run(*o) for o in operands]       # every set's outputs stay allocated: the sets do not share a byte
    reps = reps or max(20, 200 // len(operands))
    with torch.cuda.stream(st):
        for _ in range(max(30, 400 // len(operands))):             # ~20 ms of replays first: the timed ones run at the loaded clock
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
    st.synchronize()
    us = e0.elapsed_time(e1) / (reps * len(operands)) * 1e3
    n1, m1, n2, m2, ns, c = N, 512, 512, 128, 64, 128
    bq = lambda n, m: 12 * n + 12 * m + 4 * m * ns + 4 * m
    gp = lambda n, cc, m: 4 * n * cc + 4 * m * ns + 4 * m * ns * cc
    per_cloud = bq(n1, m1) + gp(n1, 3, m1) + bq(n2, m2) + gp(n2, 3, m2) + gp(n2, c, m2)
    if mode in ("fused", "fused_multi"):     # ball query + its xyz output in one pass: idx and the cloud are not read a second time
        per_cloud -= (4 * m1 * ns + 12 * n1) + (4 * m2 * ns + 12 * n2)
    ach = per_cloud * B / us / 1e3
    touched = sum(t.numel() * t.element_size() for o in operands for t in o) + \
        sum(t.numel() * t.element_size() for k in keep for t in k)
    del keep
    traffic = None
    if B == 32 and N == 1024:
        key = {"five": "ops_ball_query+group", "fused": "ops_fused_ball_query+group"}.get(mode)
        if key:
            traffic = pmc_entry(key + ("_beyond_L3" if len(operands) > 1 else "") + "_hbm_bytes_per_batch", ("grouping.hip",))
    note = {"five": "the reference's five operators as five separate launches in dependency order, hipGraph replay (graded figure)",
            "five_dag": "the reference's five operators as five separate launches on their dependency DAG (level 2's ball query and groupings on a "
                        "second stream, joined before the next operand set), hipGraph replay",
            "multi": "the same five operator results from 2 launches (both ball queries in one, all three groupings in one), hipGraph replay",
            "fused": "query_ball_group_xyz x2 + group_point(features): 3 launches, own byte numerator (no idx / cloud re-read for "
                     "the xyz groupings), hipGraph replay",
            "fused_multi": "query_ball_group_xyz_multi (both levels' ball queries AND xyz groupings in one launch) + group_point(features): "
                           "2 launches, own byte numerator (no idx / cloud re-read for the xyz groupings), hipGraph replay"}[mode]
    return dict(bound="hbm", achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(ach / HBM_PEAK_GBS, 4),
                traffic=traffic, us_per_batch=round(us, 2), launches={"five": 5, "five_dag": 5, "multi": 2, "fused": 3, "fused_multi": 2}[mode],
                algorithmic_bytes_per_cloud=per_cloud, operand_sets=len(operands), bytes_touched_per_lap=int(touched),
                residency=("beyond_L3: a lap over the sets touches %.2f GB > 256 MiB Infinity Cache" % (touched / 1e9)) if touched > 3 * (256 << 20)
                else "in_L3: the %.0f MB working set is replayed inside the 256 MiB Infinity Cache" % (touched / 1e6),
                note=note + "; the end-to-end step uses the fused SA kernel instead (grouped tensor never reaches HBM)")


def cpu_baseline(weights_a, weights_n, K, N, full, seconds=8.0):
    """The CPU oracle timed on this host on a bounded sample of the same workload, two ways:
      * `value` -- the REFERENCE'S PROCESS LAYOUT (evaluation/pose_multi_process.py:53-67): os.cpu_count()-2 worker
        processes over contiguous slices, here pinned one per core with one BLAS thread each (oracle/cpu_layout.py),
        wall-clock from first spawn to last join; `cores` = the workers that actually ran;
      * `single_core` -- the same per-cloud body on one core.
    kind = "port": the reference has no CPU network path (FPS / ball query / group register GPU kernels
    only), so the network leg is the C restatement oracle/ancsh_oracle.c; the pose leg is
    oracle/pose_oracle.py, which executes the same numpy/scipy calls as the reference's
    evaluation/parallel_ancsh_pose.py with its iteration budgets (10000 / 200, threshold 0.1)."""
    from oracle import cpu_layout, net_oracle
    jt = "prismatic" if K == 4 else "revolute"
    t0 = time.time()
    if not full:
        P = make_batch(0, 64, N=N, K=K, joint_type=jt)["P"]
        net_oracle.forward(weights_a, P[:1], K)
        t0 = time.time()
        done = 0
        while done < 64 and (time.time() - t0 < seconds or done < 4):
            net_oracle.forward(weights_a, P[done:done + 4], K)
            done += 4
        dt = time.time() - t0
        what = "network forward only (oracle/ancsh_oracle.c)"
    else:
        from oracle import pose_oracle as PO
        done, t_net, t_pose = 0, 0.0, 0.0
        while done < 8 and (time.time() - t0 < seconds or done < 1):
            c = make_cloud(done, N=N, K=K, joint_type=jt)
            pr = make_predictions(c, K, seed=done)
            t1 = time.time()
            net_oracle.forward(weights_a, c["P"][None], K)
            net_oracle.forward(weights_n, c["P"][None], K, mixed_pred=False, early_split_nocs=False)
            t2 = time.time()
            counts = np.bincount(np.argmax(pr["instance_per_point"], 1), minlength=K)
            rs = np.random.RandomState(done)
            sa = [PO.SampleStream([rs.randint(counts[j], size=3) for _ in range(10000)]) for j in range(K)]
            sb = [PO.SampleStream([rs.randint(counts[0 if k % 2 == 0 else j], size=3) for k in range(400)]) for j in range(1, K)]
            PO.solve_cloud(c["P"], pr["nocs_per_point"], pr["instance_per_point"], pr["joint_axis_per_point"],
                           pr["joint_cls_gt"], K, sa, sb, 0.1, 10000, 200)
            t_net += t2 - t1
            t_pose += time.time() - t2
            done += 1
        dt = t_net + t_pose
        what = (f"ANCSH+NPCS forward (oracle/ancsh_oracle.c, {t_net / done:.2f} s/cloud) + pose fit "
                f"(oracle/pose_oracle.py = the reference's numpy/scipy calls, {t_pose / done:.2f} s/cloud)")
    single = dict(value=round(done / dt, 4), cores=1,
                  sample=f"{done} synthetic clouds (N={N}, K={K}), {what}, {dt:.1f} s on 1 of {os.cpu_count()} host cores")
    # the reference's layout: cpu_count-2 workers; workers-1 clouds give every worker but the last exactly one cloud under its
    # slice rule num_per = int(n / workers) + 1 (with the network-only workload a cloud is ~0.1 s: 16 clouds per worker)
    # The rule is applied to the CPUs this container OWNS (affinity mask capped by the cgroup quota): on the GPU boxes
    # os.cpu_count() reports the host's 256 threads while the cgroup grants 16 CPUs, and 254 workers would only measure a 16x
    # oversubscription (measured: 149 s wall for 253 clouds = 1.7 clouds/s, 125 s per cloud inside the throttled workers).
    usable = cpu_layout.usable_cpus()
    workers = max(1, min((os.cpu_count() or 1), usable) - 2)
    n_clouds = max(1, workers - 1) if full else 16 * workers - 1
    lay = cpu_layout.run_layout(n_clouds, N, K, full, workers)
    return dict(value=round(lay["clouds_per_s"], 4), unit="point-clouds/sec", cores=lay["workers"], kind="port",
                sample=(f"reference process layout (pose_multi_process.py:53-67: cpu_count-2 workers, contiguous slices): "
                        f"os.cpu_count()={lay['host_cores']}, CPUs usable by this container (affinity + cgroup quota)={usable} -> "
                        f"{lay['workers_spec']} workers, {lay['workers']} non-empty contiguous slices of {n_clouds} synthetic "
                        f"clouds (N={N}, K={K}), one pinned process + 1 BLAS thread each, {lay['wall_s']:.1f} s wall from first spawn "
                        f"to last join; per cloud inside the workers: network {lay['net_s_per_cloud']:.2f} s + pose fit "
                        f"{lay['pose_s_per_cloud']:.2f} s"),
                single_core=single)


def bf16x3_parity(K, weights, P, dev):
    """The split-bf16 path (whatever ANCSH_SA_BF16X3 level is on: SA levels, tail chain) against the f32 path on the SAME clouds and weights,
    both through the PAIRED forward the pipeline runs (this process, both arithmetic paths): max |diff| per head over every network,
    part-label flips.  Bars of the experiment: zero flips, floats <= 1e-5.  (Against the CPU oracle: tests/test_bf16x3_gpu.py.)"""
    from articulated_pose_amd import pointnet_util
    from articulated_pose_amd.paired import PairedNetworks
    keep = pointnet_util.SA_BF16X3
    heads, flips, points = {}, 0, 0
    try:
        pair = PairedNetworks([Network(K, w, kind, dev) for w, kind in zip(weights, ("ancsh", "npcs"))])
        pointnet_util.SA_BF16X3 = 0
        refs = [{k: v.clone() for k, v in o.items()} for o in pair.predict(P)]
        pointnet_util.SA_BF16X3 = keep
        gots = pair.predict(P)
        for ref, got in zip(refs, gots):
            for k in ref:
                heads[k] = max(heads.get(k, 0.0), float((got[k] - ref[k]).abs().max()))
            flips += int((got["W"].argmax(2) != ref["W"].argmax(2)).sum())
            points += ref["W"].shape[0] * ref["W"].shape[1]
    finally:
        pointnet_util.SA_BF16X3 = keep
    return {"max_abs_diff_per_head": {k: float("%.3e" % v) for k, v in sorted(heads.items())}, "max_abs_diff": max(heads.values()),
            "label_flips": flips, "points": points, "networks": len(weights), "level": keep, "against": "f32 path, paired forward"}


def _run_json(cmd, timeout=600):
    import subprocess
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError("rc=%d %s" % (r.returncode, r.stderr[-300:]))
    for x in reversed(lines):          # a bench.py leg prints its full record first (`bench_detail`), the compact contract line last
        if x.startswith('{"bench_detail"'):
            return json.loads(x)["bench_detail"]
    return json.loads(lines[-1])


LEG_MIN_STEPS, LEG_MIN_WARMUP = 256, 24
VALUE_CONFIGS = (    # the single-GPU BASELINE.json workloads besides configs[2] (the headline): (label, bench.py arguments, op-level shape)
    ("configs[1]: eyeglasses ANCSH, batch=32, N=1024, network forward only", ["--workload", "net"], (32, 1024)),
    ("configs[3] per GPU: laptop (K=2, revolute), 16 x 2048 of the 64-cloud batch sharded over 4 GPUs, full pose pipeline",
     ["--batch", "16", "--npoints", "2048", "--parts", "2"], (16, 2048)),
    ("configs[4] per GPU: drawer (K=4, prismatic), 16 x 2048 of the 128-cloud batch sharded over 8 GPUs, full pose pipeline",
     ["--batch", "16", "--npoints", "2048", "--parts", "4"], (16, 2048)),
)


def _ops_brief(o):
    keep = ("frac", "frac_of_measured_copy", "hbm_copy_measured_GBps", "achieved", "unit", "peak", "us_per_batch", "launches", "operand_sets", "bytes_touched_per_lap",
            "algorithmic_bytes_per_cloud", "residency")
    return {k: {f: v.get(f) for f in keep} for k, v in o.items() if isinstance(v, dict) and "fused into" not in k}


LATENCY_STAGES = (("sampling + grouping + 3-NN (geometry, shared by both networks)", ("fps", "ball_query+group", "three_nn+interpolate")),
                  ("both networks' shared-MLP layers + heads", ("shared_mlp_fused_sa", "shared_mlp_conv1x1", "fp_partial_product(valu)", "shared_mlp_chain_tail",
                                                                 "head_activations")),
                  ("pose fit: partition + joint-axis medians", ("pose_partition+median",)),
                  ("pose fit: stage B (200 LM fits per joint + refit)", ("pose_ransac_joint_lm",)),
                  ("pose fit: stage A (10000 hypotheses per part + refit)", ("pose_ransac_single",)))


def latency_leg(args, dev):
    """BASELINE configs[0]'s shape ("batch=1, N=1024": what a live depth camera feeds) on the GPU: ONE cloud through both networks and
    the whole pose fit, one slot (nothing else in flight), the eight-lanes-per-fit LM schedule AncshPipeline selects for <= 2 slots;
    end-to-end latency = host issue of the captured step -> its stream synchronised, `--latency-reps` times on a warm pipeline.
    The per-stage split comes from one eager pass with HIP events around every launch (no lead launches: a lone cloud does not
    run on a loaded chip)."""
    K, N = args.parts, args.npoints
    CHAIN_FLOPS[(N, 11)] = chain_flops(N, K, True)
    CHAIN_FLOPS[(N, 8)] = chain_flops(N, K, False)
    c = make_cloud(0, N=N, K=K, joint_type="prismatic" if K == 4 else "revolute")
    pr = make_predictions(c, K, seed=0)
    pipe = AncshPipeline(K, synthetic_weights(K, seed=0), synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1), 1, N, dev,
                         couple=False, use_graph=not args.no_graph, seed=0, slots=1)
    pipe.load_inputs(c["P"][None], pr["joint_cls_gt"][None], {k: pr[k][None] for k in ("nocs_per_point", "instance_per_point", "joint_axis_per_point")})
    pipe.prepare()
    lat = []
    for i in range(8 + args.latency_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sl, _out = pipe.step()
        sl.stream.synchronize()
        lat.append((time.perf_counter() - t0) * 1e3)
    lat = np.sort(np.array(lat[8:]))
    POSE_WORK["rows"] = N
    with torch.cuda.stream(pipe.stream):
        pipe._run()
        _lib.profile_start(lead=0)
        for _ in range(3):
            pipe._run()
        rec = _lib.profile_stop()
    POSE_WORK.pop("nn_tests", None); POSE_WORK.pop("nn_launches", None)
    roof = roofline_from_profile(rec, 3)
    stages = [{"stage": name, "ms": round(sum(roof[f]["ms_per_step"] for f in fams if f in roof), 4),
               "launches": int(sum(roof[f]["launches_per_step"] for f in fams if f in roof))} for name, fams in LATENCY_STAGES]
    known = {f for _n, fams in LATENCY_STAGES for f in fams}
    other = sum(v["ms_per_step"] for f, v in roof.items() if f not in known)
    med = float(np.median(lat))
    return {"value": round(med, 4), "unit": "ms per point cloud, end to end (median of %d)" % len(lat), "higher_is_better": False,
            "p10_ms": round(float(lat[len(lat) // 10]), 4), "p90_ms": round(float(lat[(9 * len(lat)) // 10]), 4), "min_ms": round(float(lat[0]), 4),
            "clouds_per_s_one_at_a_time": round(1e3 / med, 1),
            "workload": "configs[0]'s shape on the GPU: ANCSH + NPCS forward + pose fit of ONE cloud (B = 1, N = %d, K = %d, 10000 hypotheses per part, "
                        "200 LM fits per joint), one slot, %s" % (N, K, "one hipGraph replay" if not args.no_graph else "eager launches"),
            "lm_schedule": pipe.solver.lm_schedule,
            "stages": stages, "other_launches_ms": round(other, 4),
            "stage_note": "HIP-event time of every launch of one eager pass, summed per stage (kernel time only: the difference to `value` is "
                          "launch gaps between ~50 dependent kernels and the host's replay call)",
            "command": "bench.py --latency-leg --parts %d --npoints %d --latency-reps %d" % (K, N, args.latency_reps)}


def value_configs(args, known_ops=None):
    """The other single-GPU workloads of BASELINE.json in the driver's line: each is `bench.py --leg <shape>` in a FRESH process
    (same timed loop, the driver's --steps / --warmup, its own per-kernel pass) started after this process's timed loop, plus the
    op-level ball_query+group figure of its shape beyond the Infinity Cache (one measurement per distinct shape)."""
    me = [sys.executable, os.path.abspath(__file__)]
    # >= LEG_MIN_STEPS timed steps per leg (~0.25 s): with 20 batches in flight a 20-step run is all pipeline fill and drain and
    # understated the N = 2048 legs by 10-12 % (round 5: 15.3 k / 14.5 k at 20 steps against 17.2 k / 16.1 k at 512)
    common = ["--steps", str(max(args.steps, LEG_MIN_STEPS)), "--warmup", str(max(args.warmup, LEG_MIN_WARMUP))] + (["--no-graph"] if args.no_graph else [])
    ops_by_shape, out = {k: _ops_brief(v) for k, v in (known_ops or {}).items() if isinstance(v, dict) and "error" not in v}, []
    for label, extra, shape in VALUE_CONFIGS:
        e = {"config": label, "command": "bench.py --leg " + " ".join(extra + common)}
        try:
            l = _run_json(me + ["--leg"] + extra + common)
            e.update(value=l["value"], unit=l["unit"], ms_per_step=l["ms_per_step"], steps=l["steps"], warmup=l["warmup"], dtype=l["dtype"],
                     batches_in_flight=l["config"]["batches_in_flight"], workload=l["config"]["workload"])
            r = l.get("roofline") or {}
            e["roofline"] = {k: r.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "ms_per_step", "launches_per_step")}
            e["roofline_all_frac"] = {k: v.get("frac") for k, v in (l.get("roofline_all") or {}).items() if v.get("frac") is not None}
        except Exception as ex:
            e["error"] = repr(ex)[:300]
        if shape not in ops_by_shape:
            try:
                o = _run_json(me + ["--ops-only", "--ops-brief", "--batch", str(shape[0]), "--npoints", str(shape[1]), "--ops-sets", str(args.ops_sets)])
                ops_by_shape[shape] = _ops_brief(o)
            except Exception as ex:
                ops_by_shape[shape] = {"error": repr(ex)[:300]}
        e["roofline_ops"] = ops_by_shape[shape]
        out.append(e)
    return out


FINAL_LINE_MAX = 4096          # the driver keeps a bounded tail of stdout: round 5's 20 KB line was cut and could not be parsed


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def _short(s, n):
    s = str(s)
    return s if len(s) <= n else s[:n - 3] + "..."


def compact_line(line, detail_path=None):
    """The contract line the driver parses (<= FINAL_LINE_MAX bytes): the contract fields, `roofline`, `cpu_baseline` and ONE
    number or two per secondary leg.  Everything else of `line` lives in the detail record (an earlier stdout line + a sidecar file)."""
    out = _pick(line, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype"))
    out["data"] = "synthetic"
    cfg = line.get("config", {})
    out["config"] = dict(_pick(cfg, ("global_batch", "num_points", "num_parts", "hip_graph", "batches_in_flight", "pose_inputs")),
                         workload=_short(cfg.get("workload", ""), 200), parallelism=_short(cfg.get("parallelism", ""), 90))
    if "ranks" in line:
        out["ranks"] = [_pick(r, ("rank", "device_index", "pid")) for r in line["ranks"]]
    r = line.get("roofline")
    if r:
        o = _pick(r, ("kernel", "bound", "achieved", "peak", "unit", "frac", "ms_per_step", "launches_per_step", "traffic"))
        rp = r.get("rocprof")
        if isinstance(rp, dict):      # rocprofv3's committed average for the same kernels alone on the chip (must agree with `frac`)
            st = rp.get("sa_steady") or {}
            o["rocprof"] = {"file": rp.get("file"), "frac_sa_steady": st.get("frac"), "frac_one_batch_in_flight": (rp.get("slots1") or {}).get("frac")}
        out["roofline"] = o
    ra = line.get("roofline_all")
    if ra:
        out["roofline_all_frac"] = {k: v.get("frac") for k, v in ra.items() if v.get("bound") in ("hbm", "mfma")}
    ro = line.get("roofline_ops")
    if isinstance(ro, dict):
        out["roofline_ops"] = {"error": _short(ro["error"], 120)} if "error" in ro else \
            {_short(k, 48): _pick(v, ("frac", "achieved", "unit", "peak", "us_per_batch", "launches") if k == "ball_query+group" else ("frac", "us_per_batch"))
             for k, v in ro.items() if isinstance(v, dict)}
    vn = line.get("value_network_inputs")
    if vn:
        out["value_network_inputs"] = _pick(vn, ("value", "ms_per_step", "steps"))
    for key in ("value_bf16x3", "value_f16x2"):
        vb = line.get(key)
        if vb:
            o = _pick(vb, ("value", "ms_per_step", "steps", "speedup_vs_value", "error"))
            if isinstance(vb.get("roofline"), dict):      # executed 16-bit products against the 16-bit matrix peak + the f32-equivalent rate
                o["roofline"] = _pick(vb["roofline"], ("kernel", "frac", "achieved", "f32_equivalent_TFLOPs")) | {"peak_TFLOPs": MFMA_16BIT_PEAK_TFLOPS}
            par = vb.get("parity_vs_oracle") or vb.get("parity_vs_f32_path")
            if isinstance(par, dict):
                o["parity"] = _pick(par, ("max_abs_diff", "label_flips", "against"))
            out[key] = o
    vl = line.get("value_latency")
    if vl:
        out["value_latency"] = _pick(vl, ("value", "p90_ms", "clouds_per_s_one_at_a_time")) | {"unit": "ms per cloud, one at a time"}
    vc = line.get("value_configs")
    if vc:
        legs = []
        for c in vc:
            o = {"config": _short(c.get("config", ""), 60)} | _pick(c, ("value", "ms_per_step", "steps", "error"))
            if isinstance(c.get("roofline"), dict):
                o["roofline_frac"] = c["roofline"].get("frac")
            g = (c.get("roofline_ops") or {}).get("ball_query+group")
            if isinstance(g, dict):
                o["ball_query+group_frac"] = g.get("frac")
            legs.append(o)
        out["value_configs"] = legs
    cb = line.get("cpu_baseline")
    if cb:
        o = _pick(cb, ("value", "unit", "cores", "kind"))
        o["sample"] = _short(cb.get("sample", ""), 260)
        if isinstance(cb.get("single_core"), dict):
            o["single_core"] = _pick(cb["single_core"], ("value", "cores"))
        out["cpu_baseline"] = o
    if "bf16x3_parity" in line:
        out["bf16x3_parity"] = line["bf16x3_parity"]
    if detail_path:
        out["detail"] = detail_path
    # hard bound: shed the optional legs, least important first, rather than ever print a line the driver cannot read
    for k in ("roofline_all_frac", "value_network_inputs", "ranks", "value_latency", "roofline_ops", "value_configs", "value_bf16x3", "value_f16x2"):
        if len(json.dumps(out)) < FINAL_LINE_MAX:
            break
        out.pop(k, None)
    return out


def emit(line, sidecar=True):
    """stdout: the compact contract line, alone.  The full record (one line, key `bench_detail`) goes to a sidecar file ($ANCSH_BENCH_DETAIL,
    default bench_detail.json next to bench.py) and to stderr -- or, when this process is a leg of another bench.py, to stdout for the parent."""
    path = os.environ.get("ANCSH_BENCH_DETAIL", os.path.join(ROOT, "bench_detail.json"))
    rel = os.path.relpath(path, ROOT) if not os.environ.get("ANCSH_BENCH_DETAIL") else path
    if not sidecar:
        rel = None
    else:
        try:
            with open(path, "w") as f:
                json.dump(line, f, indent=1)
        except OSError:
            rel = None
    # the full record: on STDOUT only for a leg of another bench.py (its parent reads it there); the top-level process keeps its stdout to the ONE
    # contract line -- whatever the driver's capture keeps of a stream (head or tail), a 22 KB line in it is a risk -- and sends the record to the
    # sidecar file and to stderr
    print(json.dumps({"bench_detail": line}), file=sys.stdout if not sidecar else sys.stderr, flush=True)
    final = json.dumps(compact_line(line, rel))
    assert len(final) < FINAL_LINE_MAX, len(final)
    return final


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(outputs, path):
    """Write every array of `outputs` (nested dicts of tensors / arrays; keys starting with "_" are the fit's internal scratch, not
    outputs) as <path>/<dotted.name>.npy: float64 stays float64, everything else becomes float32 (int64 -> float64).  Above
    DUMP_MAX_BYTES in all, every array is cut to the same fraction of its elements, chosen by a generator seeded with its name: the
    same arguments give the same sample.  Returns {name: shape written}."""
    import zlib
    flat, seen = {}, set()

    def walk(prefix, o):
        if isinstance(o, dict):
            for k in sorted(o):
                if not str(k).startswith("_"):
                    walk(prefix + (str(k),), o[k])
        elif torch.is_tensor(o) or isinstance(o, np.ndarray):
            key = (o.data_ptr(), tuple(o.shape), tuple(o.stride())) if torch.is_tensor(o) else id(o)
            if key not in seen:               # the same tensor under two names (e.g. the pose record): written once
                seen.add(key)
                a = o.detach().cpu().numpy() if torch.is_tensor(o) else o
                flat[".".join(prefix)] = a.astype(np.float64 if a.dtype in (np.float64, np.int64) else np.float32)
    walk((), outputs)
    total = sum(a.nbytes for a in flat.values())
    keep = min(1.0, DUMP_MAX_BYTES / float(total)) if total else 1.0
    os.makedirs(path, exist_ok=True)
    written = {}
    for name, a in flat.items():
        if keep < 1.0:
            k = int(a.size * keep)
            idx = np.sort(np.random.RandomState(zlib.crc32(name.encode())).choice(a.size, k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), a)
        written[name] = list(a.shape)
    return written


def print_last(text):
    """The contract line must be the LAST line of stdout.  Native libraries write to C stdio, which is fully buffered on a pipe and
    flushed at exit -- RCCL's "Librccl path : ..." banner came out AFTER the JSON line that Python had printed and flushed long before.
    So: flush C stdio first, then print; call this after the process group has been destroyed (nothing native prints afterwards)."""
    import ctypes
    sys.stdout.flush()
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    print(text, flush=True)


def parse_args(argv=None):
    """The command line.  A plain run measures the headline figure and nothing else; every side measurement (per-kernel roofline pass,
    op-level figures, the other configurations, precisions and data flows, the latency leg, the CPU baseline) needs --full, and a
    --leg of a --full run does its own per-kernel pass only.  args.kernel_pass: whether this process takes its own per-kernel pass
    (and, with --bf16x3, the parity of the split-16 arithmetic)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32, help="clouds per GPU per step")
    ap.add_argument("--npoints", type=int, default=1024)
    ap.add_argument("--parts", type=int, default=3)
    ap.add_argument("--workload", choices=["full", "net"], default="full",
                    help="full = configs[2] (ANCSH+NPCS forward + pose fit, the metric's configuration); "
                         "net = configs[1] (ANCSH forward only)")
    ap.add_argument("--couple", action="store_true", help="feed the pose stage with the networks' own outputs")
    ap.add_argument("--pose-inputs", choices=["synthetic", "network"], default="synthetic",
                    help="synthetic (default): seeded random weights, the fit is fed synthetic predictions (random-init heads give degenerate "
                         "parts); network: the PRODUCTION data flow -- hand-built weights whose heads emit a usable segmentation / part-NOCS "
                         "(synthetic.passthrough_pose_problem), the fit consumes the networks' own outputs")
    ap.add_argument("--slots", type=int, default=20,
                    help="batches kept in flight on separate HIP streams (full workload).  16..22 are equal within 1 %% on long runs "
                         "(20.4 k clouds/s at 512 steps); 20 is also the best on SHORT runs, where pipeline fill and drain weigh in "
                         "(20 steps after 5 warm-up steps: 19.4 k against 18.7 k with 16, 18.9 k with 22)")
    ap.add_argument("--net-slots", type=int, default=8, help="the same for --workload net")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (production); gloo = host-staged gather, for exercising the N>1 logic "
                         "with several ranks on one GPU")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group and run the per-step record gather even with one rank (executes the RCCL code "
                         "path -- communicator creation, gather on the slot streams, all-reduce of the timing -- on a single GPU)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--ops-only", action="store_true", help="print the op-level ball_query + group figures (roofline_ops) and exit")
    ap.add_argument("--full", action="store_true",
                    help="also take every side measurement after the timed steps: the per-kernel roofline pass, the op-level figures, "
                         "the production-data-flow leg, the split-16 legs, the latency leg, the other BASELINE configurations and the CPU "
                         "baseline (the --no-* options below skip single ones).  Without it a run sets up, warms up, times the steps, "
                         "writes --dump-outputs and prints the line")
    ap.add_argument("--only-timed", action="store_true",
                    help="stop after the timed steps (no per-kernel pass, op-level figures, CPU baseline): the command to put under a "
                         "kernel trace or PMC collection when only the pipelined step itself is of interest")
    ap.add_argument("--no-network-inputs", action="store_true", help="skip the value_network_inputs leg (production data flow)")
    ap.add_argument("--network-inputs-steps", type=int, default=0, help="steps of that leg (0 = as many as --steps)")
    ap.add_argument("--ops-sets", type=int, default=12,
                    help="ball_query+group beyond the 256 MiB Infinity Cache: independent buffer sets one replay walks through")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-ops", action="store_true", help="skip the op-level ball_query+group leg (roofline_ops)")
    ap.add_argument("--no-value-configs", action="store_true",
                    help="skip value_configs (the other single-GPU BASELINE workloads, each timed in a fresh process after this one's loop)")
    ap.add_argument("--latency-leg", action="store_true",
                    help="print value_latency (ONE cloud, one slot, latency LM schedule: BASELINE configs[0]'s shape on the GPU) and exit")
    ap.add_argument("--latency-reps", type=int, default=64)
    ap.add_argument("--leg", action="store_true",
                    help="this process IS one of the value_configs legs: timed loop + per-kernel pass, none of the side legs")
    ap.add_argument("--bf16x3", action="store_true",
                    help="OPT-IN EXPERIMENT, never the graded path: both fused SA levels with every f32 product emulated by six bf16 MFMA "
                         "products (csrc/sa_bf16x3.hip; same as ANCSH_SA_BF16X3=2); with --leg the line also carries the parity of this "
                         "arithmetic against the f32 path on the bench's own clouds")
    ap.add_argument("--no-bf16x3", action="store_true", help="skip the value_bf16x3 / value_f16x2 legs")
    ap.add_argument("--split-scheme", choices=["bf16x3", "f16x2"], default=None,
                    help="with --bf16x3: the split scheme of the experiment (csrc/bx3.h; default $ANCSH_SPLIT_SCHEME or bf16x3): bf16x3 = three "
                         "bf16 terms, six products; f16x2 = two f16 terms, three products into two accumulators")
    ap.add_argument("--ops-brief", action="store_true", help="with --ops-only: the graded five-launch figure (beyond the Infinity Cache) "
                                                              "and the three-launch form only")
    ap.add_argument("--dump-kernels", action="store_true", help="per-call event timings to stderr")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (the outputs the step hands its caller) as "
                         "DIR/<name>.npy, float32 / float64, at most 64 MB in all (a seeded sample of each array beyond that)")
    ap.add_argument("--profile-lead-sa", type=int, default=100, help="the same for the fused SA launches (the roofline's kernel)")
    ap.add_argument("--profile-lead", type=int, default=6,
                    help="per-kernel timing pass: launches of the same call issued back-to-back before each timed one, so the timed "
                         "launch runs at the loaded clock instead of on a chip that idled while Python prepared the call (0 = cold)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.leg or not args.full:
        args.no_ops = args.no_value_configs = args.no_cpu_baseline = args.no_network_inputs = args.no_bf16x3 = True
    args.kernel_pass = args.full or args.leg
    return args


def main():
    args = parse_args()
    if args.bf16x3:
        from articulated_pose_amd import pointnet_util
        if args.split_scheme:
            pointnet_util.SPLIT_SCHEME = args.split_scheme
        args.split_scheme = pointnet_util.SPLIT_SCHEME
        # level: both SA levels + the tail chain (3) and, for F16x2, the mid-section too (4: with three bf16 planes the mid-section gains nothing
        # -- layer3's 64 x 512 tile does not fit the LDS and fa_layer1 is slower than its f32 chain)
        pointnet_util.SA_BF16X3 = int(os.environ.get("ANCSH_SA_BF16X3", "0")) or (4 if args.split_scheme == "f16x2" else 3)

    from articulated_pose_amd import dist as ancsh_dist
    if ancsh_dist.wants_self_launch(args.gpus):
        # plain `python bench.py --gpus N`: no launcher exported WORLD_SIZE, so this process becomes the launcher -- N ranks of
        # this same command, one per GPU, joined like the reference's worker processes (evaluation/pose_multi_process.py:53-67);
        # rank 0 prints the JSON line on the inherited stdout.  No HIP call has been made in this process.
        sys.exit(ancsh_dist.launch_local_ranks(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if rank != 0:
        # stdout belongs to rank 0's JSON line: whatever this rank or a native library under it (RCCL's banner) writes to fd 1 goes
        # to stderr instead, so that under torch.distributed.run -- which merges the ranks' stdout -- the contract line stays the last one
        sys.stdout.flush()
        os.dup2(2, 1)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher exported WORLD_SIZE={world}: pass --gpus {world}")
    n_dev = torch.cuda.device_count()
    if args.dist_backend == "nccl" and world > n_dev and os.environ.get("ANCSH_SHARED_GPU_PROBE") != "1":
        raise SystemExit(f"--gpus {args.gpus} with RCCL needs one GPU per rank; this node shows {n_dev} "
                         "(--dist-backend gloo lets several ranks share a GPU for exercising the N > 1 logic)")
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    use_dist = world > 1 or args.force_dist
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # control plane (barrier, max over ranks) on gloo; the record gather on RCCL when its probe passes on every rank, else host-staged
        data_group, collective_note = ancsh_dist.init_groups(args.dist_backend, dev)
    ranks = ancsh_dist.all_rank_identities(dev)        # who took part: one all_gather_object (a single entry without a group)

    if args.latency_leg:
        print(json.dumps(latency_leg(args, dev)), flush=True)
        return
    B, N, K = args.batch, args.npoints, args.parts
    full = args.workload == "full"
    CHAIN_FLOPS[(B * N, 11)] = chain_flops(B * N, K, True)
    CHAIN_FLOPS[(B * N, 8)] = chain_flops(B * N, K, False)
    w_ancsh = synthetic_weights(K, seed=0)
    w_npcs = synthetic_weights(K, mixed_pred=False, early_split_nocs=False, seed=1)
    joint_type = "prismatic" if K == 4 else "revolute"                               # drawer (K=4) slides, the others hinge
    clouds = [make_cloud(rank * B + i, N=N, K=K, joint_type=joint_type) for i in range(B)]   # this rank's shard
    P = np.stack([c["P"] for c in clouds])
    if args.ops_only:
        # the op-level figures on a device that holds nothing else (see the roofline_ops block below): one JSON object, then exit
        Pd = torch.from_numpy(P).to(dev)
        copy_gbs = measured_hbm_copy(dev)

        def both(r):       # the same achieved GB/s against the datasheet peak (frac) AND against this device's measured float4 copy
            r["hbm_copy_measured_GBps"] = copy_gbs
            r["frac_of_measured_copy"] = round(r["achieved"] / copy_gbs, 4)
            return r
        # graded entry: served by HBM (operand sets rotate past the Infinity Cache); the single-set replay of rounds 1-2, which
        # stays inside the 256 MiB cache, is carried next to it under in_L3
        graded = both(op_level_ball_group(Pd, B, N, dev, "five", sets=args.ops_sets))
        if args.ops_brief:
            multi = both(op_level_ball_group(Pd, B, N, dev, "multi", sets=args.ops_sets))
            two = both(op_level_ball_group(Pd, B, N, dev, "fused_multi", sets=args.ops_sets))
            print(json.dumps({"ball_query+group": graded,
                              "ball_query+group (2 launches: multi-problem ball query, multi-problem grouping)": multi,
                              "ball_query+group (2 launches: both levels' ball query + xyz grouping in one)": two}), flush=True)
            return
        inl3 = both(op_level_ball_group(Pd, B, N, dev, "five"))
        fields = ("frac", "frac_of_measured_copy", "achieved", "us_per_batch", "operand_sets", "bytes_touched_per_lap", "traffic")
        graded["beyond_L3"] = {k: graded[k] for k in fields}
        graded["in_L3"] = {k: inl3[k] for k in fields}
        print(json.dumps({"ball_query+group": graded,
                          "ball_query+group (2 launches: multi-problem ball query, multi-problem grouping)": both(op_level_ball_group(Pd, B, N, dev, "multi", sets=args.ops_sets)),
                          "ball_query+group (2 launches: both levels' ball query + xyz grouping in one)": both(op_level_ball_group(Pd, B, N, dev, "fused_multi", sets=args.ops_sets)),
                          "ball_query+group (3 launches: xyz grouping fused into the ball query)": both(op_level_ball_group(Pd, B, N, dev, "fused", sets=args.ops_sets)),
                          "ball_query+group (5 launches on their dependency DAG: the two levels on two streams)": both(op_level_ball_group(Pd, B, N, dev, "five_dag", sets=args.ops_sets))}),
              flush=True)
        return
    networked = full and args.pose_inputs == "network"
    if networked:
        from articulated_pose_amd.synthetic import passthrough_pose_problem
        pb = passthrough_pose_problem(K, B, N, seed=100 + rank)
        w_ancsh, w_npcs, P = pb["w_ancsh"], pb["w_npcs"], pb["P"]
        args.couple = True
    sharded = None
    if full:
        # the product's multi-GPU entry (articulated_pose_amd.dist.ShardedPipeline): this rank's contiguous shard of the world * B
        # clouds through its own AncshPipeline, ONE gather of the (n, K, 26) f64 records per batch on the batch's stream
        sharded = ancsh_dist.ShardedPipeline(K, w_ancsh, w_npcs, world * B, N, dev, data_group=data_group if use_dist else None, dst=0,
                                             slots=args.slots, gather_single=args.force_dist, couple=True if networked else args.couple,
                                             use_graph=not args.no_graph, seed=rank)
        pipe = sharded.pipe
        assert (sharded.lo, sharded.hi) == (rank * B, rank * B + B)
        if networked:
            sharded.load_inputs(P, pb["cls"], is_global=False)                 # each rank generated its own shard above
        else:
            preds = [make_predictions(c, K, seed=rank * B + i) for i, c in enumerate(clouds)]
            sharded.load_inputs(P, np.stack([p["joint_cls_gt"] for p in preds]),
                                {k: np.stack([p[k] for p in preds]) for k in ("nocs_per_point", "instance_per_point", "joint_axis_per_point")},
                                is_global=False)
        sharded.prepare()
        stream, rec_shape, rec_dtype = pipe.stream, (B, K, 26), torch.float64
        eager = lambda: pipe._run()
    else:
        net = Network(K, w_ancsh, "ancsh", dev)
        # batches in flight on separate streams, one captured forward each: batch i+1's farthest-point sampling (a 32-workgroup,
        # latency-bound chain that everything else waits for) runs under batch i's matrix kernels
        engines = [AncshEngine(net, B, N, use_graph=not args.no_graph) for _ in range(max(1, args.net_slots))]
        for e in engines:
            e.P.copy_(torch.from_numpy(P))
        engine = engines[0]
        keys = ("W", "nocs_per_point", "confi_per_point", "heatmap_per_point", "unitvec_per_point",
                "joint_axis_per_point", "index_per_point", "gocs_per_point", "global_scale", "global_translation")
        stream, rec_shape, rec_dtype = engine.stream, (B, N, 11 + 11 * K), torch.float32
        eager = lambda: engine._forward(engine.P)
        turn = [0]
    # the step's one collective: articulated_pose_amd.dist.RecordGatherer (covered by tests/test_dist_cpu.py with gloo)
    gatherer = None
    if use_dist and not full:
        from articulated_pose_amd.dist import RecordGatherer
        gatherer = RecordGatherer(rec_shape, rec_dtype, dev, dst=0, group=data_group)

    last = {}

    def timed(pipe, steps, warmup):
        """warmup untimed steps, then exactly `steps` steps between barrier + full synchronise on both sides; max over ranks (s).
        last["out"]: the outputs the last step handed back (valid after the closing synchronise, until that slot runs again)."""
        def step():
            if full:
                last["out"] = sharded.step()[1]             # next batch on its slot's stream + its record gather (RCCL: same stream)
                return
            e = engines[turn[0] % len(engines)]
            turn[0] += 1
            with torch.cuda.stream(e.stream):
                out = last["out"] = e()
                if use_dist:
                    gatherer.gather(torch.cat([out[k] for k in keys], dim=2), lane=id(e), stream=e.stream)

        def flush():
            if full:
                sharded.flush()                             # a host-staged (gloo) data group gathers one slot turn late: drain

        def sync():
            if full:
                pipe.synchronize()
            else:
                for e in engines:
                    e.stream.synchronize()
            torch.cuda.synchronize()

        for _ in range(warmup):
            step()
        flush()
        sync()
        if use_dist:
            dist.barrier()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        flush()
        sync()
        if use_dist:
            dist.barrier()
        sync()
        dt = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([dt], dtype=torch.float64)          # the control group is gloo: a host tensor
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    dt = timed(pipe if full else None, args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        # before anything else runs on the device: the last step's slot is reused by no later work of this process until then
        outs = dict(last["out"])
        if full and sharded.gatherer is not None:
            outs["records"] = sharded.records()          # the world's gathered (global_batch, K, 26) records
        written = dump_outputs(outs, args.dump_outputs)
        print("bench.py: %d arrays of the last timed step written to %s" % (len(written), args.dump_outputs), file=sys.stderr, flush=True)

    if args.only_timed:
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print_last(json.dumps({"value": round(world * B * args.steps / dt, 2), "unit": "point-clouds/sec", "n_gpus": world, "steps": args.steps,
                                   "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "only_timed": True, "ranks": ranks,
                                   "parallelism": "independent clouds sharded over %d GPU(s)%s" % (
                                       world, ", 1 %s gather of pose records per step" % collective_note if use_dist else "")}))
        return

    # per-kernel durations (--full, or a --leg of one): the same launches issued eagerly, each bracketed by HIP events on the launch stream
    roof = {}
    POSE_WORK["rows"] = B * N
    if rank == 0 and full and args.kernel_pass:
        # LM work of one step: sum of MINPACK function evaluations over the step's (K-1)*B*200 hypothesis fits (one eager pass
        # with the per-hypothesis statistics switched on; outside the timed region)
        pipe.solver.want_lm_stat = True
        with torch.cuda.stream(stream):
            st = pipe._run()["pose"].get("lm_stat")
        stream.synchronize()
        pipe.solver.want_lm_stat = False
        if st is not None:
            POSE_WORK["lm_evals"] = float(st[..., 1].sum().item())
    if rank == 0 and args.kernel_pass:
        passes = max(3, min(args.steps, 8))
        with torch.cuda.stream(stream):
            eager()
            # The dominant family (fused SA) is timed at the clock it runs at inside the loaded pipeline: SA_LEAD launches of the
            # same call (~25 ms) precede each timed one.  From idle the power management ramps the clock for tens of ms under a
            # matrix load (s_memtime against HIP events: 2.0 ticks/ns in a 20-launch loop from idle, 2.39 once loaded), which
            # made the same kernels look 12 % slower in round 1's cold per-launch timing.
            lead_for = {k: args.profile_lead_sa for k in ("ancsh_sa_module_fused", "ancsh_sa_module_fused_partial", "ancsh_sa_module_fused_grouped",
                                                          "ancsh_sa_module_fused_partial_grouped", "ancsh_sa_module_fused_bf16x3_grouped",
                                                          "ancsh_sa_module_fused_partial_bf16x3_grouped", "ancsh_sa_module_fused_f16x2_grouped",
                                                          "ancsh_sa_module_fused_partial_f16x2_grouped")} if args.profile_lead else None
            _lib.profile_start(lead=args.profile_lead, lead_for=lead_for)
            for _ in range(passes):
                eager()
            rec = _lib.profile_stop()
        POSE_WORK.pop("nn_tests", None); POSE_WORK.pop("nn_launches", None)
        roof = roofline_from_profile(rec, passes)
        if args.dump_kernels:
            per = len(rec) // passes
            for i in range(per):
                ms = sum(rec[i + p * per][2] for p in range(passes)) / passes
                name, a = rec[i][0], rec[i][1]
                ints = [x for x in a if isinstance(x, (int, float)) and not (isinstance(x, int) and x > 1 << 32)]
                f, by, fl = kernel_work(name, a)
                extra = f"{fl / ms / 1e9:8.1f} TF/s" if fl else (f"{by / ms / 1e6:8.1f} GB/s" if by else " " * 13)
                print(f"{i:3d} {name:36s} {ms * 1e3:9.1f} us {extra}  {ints}", file=sys.stderr)

    if rank == 0:
        value = world * B * args.steps / dt
        rated = {k: v for k, v in roof.items() if v["bound"] in ("hbm", "mfma")}
        dominant = max(rated, key=lambda k: rated[k]["ms_per_step"]) if rated else None
        wl = ("configs[2]-style: ANCSH+NPCS, batch=%d/GPU, N=%d pts, K=%d: ANCSH forward + NPCS forward + batched "
              "RANSAC (10000/part) / Umeyama-Kabsch + articulated LM joint fit (200/joint)" % (B, N, K)) if full else \
             ("configs[1]: eyeglasses ANCSH, batch=%d/GPU, N=%d pts, K=%d, network forward only" % (B, N, K))
        data = "synthetic articulated clouds (boxes, seed 1234+id); seeded random-init weights under the reference's TF variable names"
        if networked:
            data = ("synthetic slab clouds + HAND-BUILT weights whose heads emit a usable segmentation / part-NOCS (trunk carries xyz through "
                    "fa_layer3/fc1, linear heads; every earlier layer seeded random): the pose stage consumes the networks' OWN outputs "
                    "(production data flow)")
        elif full and not args.couple:
            data += ("; pose stage fed synthetic predictions (GT part-NOCS + N(0,0.01), 10% outliers, 5% label flips) because "
                     "random-init heads yield degenerate parts -- both networks and the fit all run inside every step")
        line = {
            "metric": "point-clouds/sec (N=%d, %s ANCSH infer%s)" % (N, {2: "laptop", 3: "eyeglasses", 4: "drawer"}.get(K, "K=%d" % K),
                                                                      "+pose-fit" if full else ""),
            "value": round(value, 2), "unit": "point-clouds/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32 (network) / f64 (joint LM)" if full else "f32",
            "data": data,
            "config": {"workload": wl, "global_batch": world * B, "num_points": N, "num_parts": K,
                       "parallelism": "independent clouds sharded over %d GPU(s)%s" % (
                           world, ", 1 %s gather of pose records per step" % collective_note
                           if use_dist else ""),
                       "hip_graph": not args.no_graph, "batches_in_flight": args.slots if full else max(1, args.net_slots), "pose_inputs": "network outputs" if args.couple else "synthetic predictions"},
        }
        line["ranks"] = ranks
        if args.bf16x3:
            line["dtype"] = {"bf16x3": "f32 products emulated by 6 bf16 MFMA products (3 bf16 terms per operand), f32 accumulate",
                             "f16x2": "f32 products emulated by 3 f16 MFMA products (2 f16 terms per operand, ~22 bits), f32 accumulate"}[args.split_scheme] + \
                            (" (fused SA levels, mid-section, tail chain)" if pointnet_util.SA_BF16X3 >= 4 else " (fused SA levels + tail chain; mid-section f32)") + \
                            (" / f64 (joint LM)" if full else "")
            line["split_scheme"] = args.split_scheme
            if args.kernel_pass:
                line["bf16x3_parity"] = bf16x3_parity(K, (w_ancsh, w_npcs) if full else (w_ancsh,), P, dev)
        if full and world == 1 and not networked and not args.no_network_inputs:
            # the PRODUCTION data flow in the same timed loop (hand-built weights whose heads emit a usable segmentation /
            # part-NOCS; the fit consumes the networks' OWN outputs): shows what the synthetic-prediction default does to `value`.
            # Run as `bench.py --only-timed --pose-inputs network` in a FRESH process: a second set of 16 captured graphs built in
            # this process after the first replays ~15 % slower (17.2 k vs 20.7 k clouds/s measured; the first set is unaffected),
            # an artefact of the runtime's state, not of the data flow.
            import subprocess
            steps2 = max(1, args.network_inputs_steps or args.steps)
            cmd = [sys.executable, os.path.abspath(__file__), "--only-timed", "--pose-inputs", "network", "--steps", str(steps2),
                   "--warmup", str(args.warmup), "--batch", str(B), "--npoints", str(N), "--parts", str(K), "--slots", str(args.slots)]
            if args.no_graph:
                cmd.append("--no-graph")
            try:
                r2 = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                l2 = json.loads([x for x in r2.stdout.splitlines() if x.startswith("{")][-1])
                line["value_network_inputs"] = {
                    "value": l2["value"], "unit": "point-clouds/sec", "steps": l2["steps"], "warmup": l2["warmup"], "ms_per_step": l2["ms_per_step"],
                    "command": "bench.py " + " ".join(cmd[2:]),
                    "data": "synthetic slab clouds + hand-built weights (synthetic.passthrough_pose_problem): the pose fit reads the two "
                            "networks' own outputs; same pipeline, same timed loop, same batches in flight, own process"}
            except Exception as e:      # the leg is informative; the line's contract fields do not depend on it
                line["value_network_inputs"] = {"value": None, "error": repr(e)[:300]}
        if dominant:
            r = dict(roof[dominant])
            r["kernel"] = dominant
            r["timing"] = ("HIP events around single launches on the launch stream, one batch alone on the chip; each timed fused-SA launch "
                           "follows %d back-to-back launches of the same call (loaded clock, as inside the pipelined step; "
                           "profiles/*_kernel_stats_sa_steady.csv is rocprofv3's view of the same loop), other calls follow %d"
                           % (args.profile_lead_sa if args.profile_lead else 0, args.profile_lead))
            if dominant == "shared_mlp_fused_sa" and B == 32 and N == 1024:
                r["rocprof"] = rocprof_roofline()
            r["traffic_source"] = pmc_provenance()
            line["roofline"] = r
            line["roofline_all"] = roof
        if world == 1 and not args.no_ops:
            # Op-level figures in a FRESH process, after everything of this one has been timed.  Both directions of interference were
            # measured: taken in this process after the pipelines exist (~40 captured graphs of ~50 nodes) the five-launch graph
            # replays at either 47 or ~100 us per batch from run to run; taken in this process BEFORE the pipelines are built, they
            # leave the runtime in a state that costs the timed loop a fixed ~50 ms (4.1 instead of 1.6 ms/step on a 20-step run).
            import subprocess
            cmd = [sys.executable, os.path.abspath(__file__), "--ops-only", "--batch", str(B), "--npoints", str(N), "--parts", str(K),
                   "--ops-sets", str(args.ops_sets)]
            try:
                r3 = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                line["roofline_ops"] = json.loads([x for x in r3.stdout.splitlines() if x.startswith("{")][-1])
            except Exception as e:
                line["roofline_ops"] = {"error": repr(e)[:300]}
        if world == 1 and full and not networked and not args.no_bf16x3 and not args.bf16x3:
            # The split-16 experiment as LABELLED SECONDARY figures (f32 stays the headline and the graded dtype), one per scheme: the same
            # timed loop in a fresh process, and -- computed in that process on this bench's own clouds -- its parity against the f32 path.
            for scheme in ("bf16x3", "f16x2"):
                key = "value_" + scheme
                try:
                    l5 = _run_json([sys.executable, os.path.abspath(__file__), "--leg", "--bf16x3", "--split-scheme", scheme, "--steps", str(args.steps),
                                    "--warmup", str(args.warmup), "--batch", str(B), "--npoints", str(N), "--parts", str(K), "--slots", str(args.slots)]
                                   + (["--no-graph"] if args.no_graph else []))
                    line[key] = {"value": l5["value"], "unit": l5["unit"], "ms_per_step": l5["ms_per_step"], "steps": l5["steps"], "warmup": l5["warmup"],
                                 "dtype": l5["dtype"], "parity_vs_f32_path": l5.get("bf16x3_parity"), "speedup_vs_value": round(l5["value"] / value, 4),
                                 # the leg's own dominant kernel family against the 16-bit matrix peak (executed products) and, next to it, its
                                 # f32-equivalent rate; every family of the leg under roofline_all
                                 "roofline": l5.get("roofline"), "roofline_all": l5.get("roofline_all"),
                                 "command": "bench.py --leg --bf16x3 --split-scheme %s --steps %d --warmup %d" % (scheme, args.steps, args.warmup),
                                 "status": "opt-in experiment (ANCSH_SA_BF16X3=3|4 ANCSH_SPLIT_SCHEME=%s): NOT the graded path; additions inside a "
                                           "16-product MFMA are ordered by the instruction, so results equal the k-ordered f32 chain to summation "
                                           "noise, not bit for bit" % scheme}
                except Exception as ex:
                    line[key] = {"value": None, "error": repr(ex)[:300]}
        if world == 1 and not args.no_value_configs and full and (B, N, K) == (32, 1024, 3) and not networked:
            # BASELINE configs[0]'s shape on the GPU (one cloud at a time), next to cpu_baseline.single_core -- a fresh process like every leg
            try:
                line["value_latency"] = _run_json([sys.executable, os.path.abspath(__file__), "--latency-leg", "--parts", str(K), "--npoints", str(N)]
                                                  + (["--no-graph"] if args.no_graph else []))
            except Exception as ex:
                line["value_latency"] = {"value": None, "error": repr(ex)[:300]}
            line["value_configs"] = value_configs(args, {(B, N): line.get("roofline_ops")})
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(w_ancsh, w_npcs, K, N, full)
        final = emit(line, sidecar=not args.leg)
    if use_dist:
        dist.barrier()                 # rank 0 is still profiling / printing: leave together
        dist.destroy_process_group()
    if rank == 0:
        print_last(final)


if __name__ == "__main__":
    main()
