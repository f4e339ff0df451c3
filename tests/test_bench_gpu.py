"""bench.py end to end: the N=1 line's contract fields, and the N>1 code path (torch.distributed.run, two ranks) on the
one GPU a test box has -- `--dist-backend gloo` stages the per-step record gather through host memory, everything else
(sharding by rank, one gather per step per batch in flight, barrier + max-over-ranks timing, rank-0 JSON) is the code
the driver launches with RCCL on an 8-GPU node."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


FINAL_LINE_MAX = 4096


def _final(stdout):
    """The contract line = the LAST stdout line: parseable, small enough for the driver's bounded capture (round 5's 20 KB line was
    cut and `BENCH_r05.json.parsed` came out null)."""
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert lines and lines[-1].startswith("{"), "last stdout line is not the JSON line: %r" % stdout[-600:]
    assert len(lines[-1]) < FINAL_LINE_MAX, len(lines[-1])
    return json.loads(lines[-1])


def _last_json(stdout, stderr=""):
    """The full record (`bench_detail`: stderr + the sidecar file of a top-level run), after checking the contract line itself -- which must be
    the ONLY JSON on stdout."""
    final = _final(stdout)
    assert not [l for l in stdout.splitlines() if l.startswith('{"bench_detail"')], "the full record must not be on stdout"
    det = [l for l in stderr.splitlines() if l.startswith('{"bench_detail"')]
    assert det, stderr[-2000:]
    full = json.loads(det[-1])["bench_detail"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype"):
        assert final[k] == full[k], k
    assert final["data"] == "synthetic" and final["config"]["workload"]
    return full


def _free_port():
    """A rendezvous port that was free a moment ago (never a fixed number: whatever else runs on the box may sit on it)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def test_bench_single_gpu_line(dev):
    r = subprocess.run([sys.executable, "bench.py", "--steps", "8", "--warmup", "2", "--slots", "2", "--full", "--no-cpu-baseline"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in line, k
    final = _final(r.stdout)
    fr = final["roofline"]
    assert fr["bound"] in ("hbm", "mfma") and fr["kernel"] and 0 < fr["frac"] < 1 and fr["peak"] > 0 and "traffic" in fr
    assert final["roofline_ops"]["ball_query+group"]["frac"] == line["roofline_ops"]["ball_query+group"]["frac"]
    assert [c["value"] > 0 for c in final["value_configs"]] == [True] * 3 and all(c["steps"] >= 256 for c in final["value_configs"])
    assert final["value_latency"]["value"] > 0 and final["value_bf16x3"]["value"] > 0 and final["value_network_inputs"]["value"] > 0
    assert final["value_f16x2"]["value"] > final["value"] and final["value_f16x2"]["parity"]["label_flips"] == 0
    with open(os.path.join(ROOT, final["detail"])) as f:
        assert json.load(f)["value"] == final["value"]
    assert line["n_gpus"] == 1 and line["steps"] == 8 and line["value"] > 0 and line["scaling"] == "weak"
    assert abs(line["value"] - 32 * 1000.0 / line["ms_per_step"]) / line["value"] < 1e-3
    roof = line["roofline"]
    assert roof["bound"] in ("hbm", "mfma") and 0 < roof["frac"] < 1 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    # who took part, and the production-data-flow leg next to `value`
    assert len(line["ranks"]) == 1 and line["ranks"][0]["rank"] == 0 and line["ranks"][0]["device_index"] == 0
    vn = line["value_network_inputs"]
    assert vn["value"] > 0 and abs(vn["value"] - 32 * 1000.0 / vn["ms_per_step"]) / vn["value"] < 1e-3
    # the graded op-level figure is the one served by HBM; the in-cache replay is carried next to it
    g = line["roofline_ops"]["ball_query+group"]
    assert g["operand_sets"] >= 8 and g["bytes_touched_per_lap"] > 4 * (256 << 20) and g["residency"].startswith("beyond_L3")
    assert g["in_L3"]["operand_sets"] == 1 and 0 < g["beyond_L3"]["frac"] < 1 and g["beyond_L3"]["frac"] == g["frac"]


def test_bench_self_launches_two_ranks(dev):
    """`python bench.py --gpus 2` WITHOUT torch.distributed.run: the command starts its own two ranks (here sharing the one GPU
    of the test box, host-staged gloo gather) and the line lists both."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "2", "--slots", "3", "--dist-backend", "gloo",
                        "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 64 and line["value"] > 0
    assert [x["rank"] for x in line["ranks"]] == [0, 1] and line["ranks"][0]["pid"] != line["ranks"][1]["pid"]
    assert all(x["device_index"] == 0 and x["device_name"] for x in line["ranks"])


def test_bench_eight_ranks_preflight_on_one_gpu(dev):
    """The driver's 8-GPU command shape, `python bench.py --gpus N` with N > 2, with the ranks sharing the test box's one GPU
    (host-staged gloo gather): all ranks are listed, the global batch is N x 32, the line's arithmetic holds.  At most six processes
    may hold one GPU at a time, and this test's own process is one of them, so the command runs with N = 4 ranks here; the eight-rank
    launch itself (eight ranks forming the group, ragged shards gathered in order, a dying rank reported) is
    tests/test_dist_cpu.py::test_eight_rank_preflight_gloo.  What an 8-GPU node adds to this is hardware (RCCL over xGMI), not code."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "4", "--warmup", "1", "--slots", "2", "--dist-backend", "gloo",
                        "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    assert line["n_gpus"] == 4 and line["config"]["global_batch"] == 128 and line["value"] > 0
    assert [x["rank"] for x in line["ranks"]] == list(range(4)) and len({x["pid"] for x in line["ranks"]}) == 4
    assert abs(line["value"] - 128 * 1000.0 / line["ms_per_step"]) / line["value"] < 1e-3


def test_bench_rccl_refuses_more_ranks_than_gpus(dev):
    """RCCL needs one GPU per rank: on a one-GPU box `--gpus 2` (nccl) must fail loudly in every rank, and the launcher must
    return that failure instead of hanging."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("box has several GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "one GPU per rank" in r.stderr


def test_bench_falls_back_to_gloo_when_rccl_cannot_start(dev):
    """Two ranks on ONE GPU with the RCCL backend requested (ANCSH_SHARED_GPU_PROBE=1 lifts bench.py's one-GPU-per-rank check): RCCL
    refuses to build a communicator over a duplicate GPU on every rank, the ranks agree over the gloo control group, the gather is
    staged through the host, the job completes and the line SAYS what happened -- a node whose RCCL cannot start still yields a
    measurement instead of a crash."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("box has several GPUs: RCCL would simply work")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(ANCSH_SHARED_GPU_PROBE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "2", "--slots", "3", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 64 and line["value"] > 0
    par = line["config"]["parallelism"]
    assert "gloo (host-staged): the RCCL probe failed" in par and "rank 0" in par, par


def test_bench_two_ranks_on_one_gpu_gloo(dev):
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "6",
                        "--warmup", "2", "--slots", "3", "--dist-backend", "gloo", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 64 and line["value"] > 0
    assert abs(line["value"] - 64 * 1000.0 / line["ms_per_step"]) / line["value"] < 1e-3
    assert [x["rank"] for x in line["ranks"]] == [0, 1]
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "bench_2ranks_gloo_one_gpu.json"), "w") as f:
            f.write(json.dumps(line) + "\n")


def test_bench_rccl_code_path_single_rank(dev):
    """`--force-dist` on one GPU: process group with the nccl (= RCCL) backend, the per-step gather enqueued on the slot streams
    behind graph replays, barrier + all-reduce of the timing, destroy -- the calls the 8-GPU launch makes, with one rank."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--steps", "6", "--warmup", "2", "--slots", "3", "--force-dist", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    assert line["n_gpus"] == 1 and line["value"] > 0 and "1 RCCL gather" in line["config"]["parallelism"]


def test_plain_run_takes_only_the_headline(dev):
    """The driver times `python3 bench.py --gpus 1 --steps 20 --warmup 5` several times per change: such a plain run sets up, warms
    up, times the steps and prints the line -- the same headline fields as a --full run, no side leg -- and the fresh process spends
    at most 30 s beyond its warm-up and timed steps."""
    import time
    steps, warmup = 20, 5
    t0 = time.time()
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json(r.stdout, r.stderr)
    assert line["metric"] == "point-clouds/sec (N=1024, eyeglasses ANCSH infer+pose-fit)" and line["unit"] == "point-clouds/sec"
    assert line["higher_is_better"] is True and line["dtype"] == "f32 (network) / f64 (joint LM)"
    assert line["steps"] == steps and line["warmup"] == warmup and line["config"]["batches_in_flight"] == 20
    assert abs(line["value"] - 32 * 1000.0 / line["ms_per_step"]) / line["value"] < 1e-3
    side = ("roofline", "roofline_all", "roofline_ops", "value_network_inputs", "value_bf16x3", "value_f16x2", "value_latency",
            "value_configs", "cpu_baseline", "bf16x3_parity")
    assert [k for k in side if k in line] == []
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    assert outside < 30.0, (wall, line["ms_per_step"])


def test_driver_command_is_not_slowed_by_the_side_measurements(dev):
    """The driver's command with every side measurement, `python3 bench.py --gpus 1 --steps 20 --warmup 5 --full`.  The line's extra
    legs (op-level figures, the production-data-flow leg, the per-kernel pass, the other BASELINE configs, the split-bf16 figure, the
    CPU baseline) must not leak into the timed loop: on a 20-step run a fixed cost shows at once (taking the op-level graphs in the same
    process BEFORE the pipeline cost the timed loop ~50 ms: 4.1 instead of 1.6 ms/step).  The full line's ms_per_step has to agree with
    the bare timed loop of a fresh process, every leg has to be there, and the whole command has to stay a one-minute affair."""
    import time
    args = ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    t0 = time.time()
    full = subprocess.run([sys.executable, "bench.py"] + args + ["--full"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    wall = time.time() - t0
    assert full.returncode == 0, full.stderr[-3000:]
    bare = subprocess.run([sys.executable, "bench.py"] + args + ["--only-timed"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert bare.returncode == 0, bare.stderr[-3000:]
    lf, lb = _last_json(full.stdout, full.stderr), _final(bare.stdout)          # --only-timed prints one short line, no detail record
    assert lf["steps"] == 20 and lf["warmup"] == 5 and lf["config"]["batches_in_flight"] == 20
    assert lf["ms_per_step"] <= 1.25 * lb["ms_per_step"], (lf["ms_per_step"], lb["ms_per_step"])
    g = lf["roofline_ops"]["ball_query+group"]
    assert 0.2 < g["frac"] < 1 and 0.2 < g["in_L3"]["frac"] < 1
    assert g["hbm_copy_measured_GBps"] > 3000 and g["frac"] < g["frac_of_measured_copy"] < 1.2
    # every single-GPU BASELINE workload is in the line: configs[1], configs[3] / GPU, configs[4] / GPU
    vc = lf["value_configs"]
    assert [e["config"].split(":")[0] for e in vc] == ["configs[1]", "configs[3] per GPU", "configs[4] per GPU"]
    for e in vc:
        assert "error" not in e, e
        assert e["value"] > 0 and e["ms_per_step"] > 0 and e["steps"] >= 256 and 0 < e["roofline"]["frac"] < 1      # legs amortise pipeline fill and drain
        ops = e["roofline_ops"]["ball_query+group"]
        assert 0.1 < ops["frac"] < 1 and ops["residency"].startswith("beyond_L3")
    assert vc[0]["value"] > lf["value"]                                 # the network alone is faster than network + fit
    # the split-bf16 experiment as a labelled secondary figure, with its parity computed on the bench's own clouds
    vb = lf["value_bf16x3"]
    assert vb["value"] > 0 and "NOT the graded path" in vb["status"] and "bf16" in vb["dtype"]
    assert vb["parity_vs_f32_path"]["label_flips"] == 0 and vb["parity_vs_f32_path"]["max_abs_diff"] <= 1e-5
    vh = lf["value_f16x2"]
    assert vh["value"] > vb["value"] * 0.95 and "f16" in vh["dtype"] and "NOT the graded path" in vh["status"]
    assert vh["parity_vs_f32_path"]["label_flips"] == 0 and vh["parity_vs_f32_path"]["max_abs_diff"] <= 1e-5
    # each split-16 leg prices its own dominant family: executed 16-bit products against the 16-bit matrix peak, f32-equivalent rate beside it
    for v, scheme, prod in ((vb, "bf16x3", 6), (vh, "f16x2", 3)):
        rr = v["roofline"]
        assert rr["kernel"] == "shared_mlp_fused_sa [%s]" % scheme and rr["bound"] == "mfma" and rr["peak"] == 2500.0 and rr["products_per_f32_product"] == prod
        assert 0.1 < rr["frac"] < 1 and abs(rr["achieved"] - prod * rr["f32_equivalent_TFLOPs"]) < 1.0
        assert rr["f32_equivalent_TFLOPs"] > lf["roofline"]["achieved"]                 # faster than the f32 kernels on the same layers
        assert "shared_mlp_chain_tail [%s]" % scheme in v["roofline_all"]
    assert lf["dtype"].startswith("f32") and lf["cpu_baseline"]["value"] > 0
    # round 5: one cloud at a time (BASELINE configs[0]'s shape on the GPU) with its per-stage split; the conv family = SA2's partial conv + the
    # three mid-section chains; no aten launch in the step (every family of roofline_all is an ancsh_* call); the PMC stamp is current
    vl = lf["value_latency"]
    assert 0.5 < vl["value"] < 5.0 and vl["higher_is_better"] is False and vl["lm_schedule"] == "latency"
    assert len(vl["stages"]) == 5 and all(st["ms"] > 0 for st in vl["stages"]) and sum(st["ms"] for st in vl["stages"]) < 1.2 * vl["value"]
    ra = lf["roofline_all"]
    assert ra["shared_mlp_conv1x1"]["launches_per_step"] == 4 and ra["shared_mlp_conv1x1"]["frac"] > 0.6
    assert ra["three_nn+interpolate"]["bound"] == "alu" and ra["three_nn+interpolate"]["launches_per_step"] == 2
    assert all(not k.startswith("aten") for k in ra)
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "bench_driver_cmd_from_test.json"), "w") as f:
            f.write(json.dumps(dict(lf, wall_s=round(wall, 1))) + "\n")
    assert wall < 90.0, wall
