"""GPU: ancsh_joint_params (pred and ground-truth variants), ancsh_articulation_rec and ancsh_part_extents against the float64 numpy
reference of tests/eval_cases.py, through the product wrappers, on cases whose vote counts and layouts sit on the edges of the ordered
compaction (64-lane waves, 256-point chunks), of the bitonic sort's power-of-two padding (counts 2^k, 2^k + 1, 1..3, 4096 = the 96 KB
dynamic-LDS launch) and of the median (even counts), at K = 1..8, both global-NOCS layouts and joint heads narrower and wider than K.
One seed per case, the message names the case; ANCSH_EVAL_SWEEP_SEEDS=1000 for a one-off long fuzz (seeds repeat the suite's shapes
modulo 40).  Every test runs under redzone.guarded(): an output element a kernel fails to write is a NaN / -1 in the equality checks.

Bars.  Medians, the ground-truth axis mean, extents and counts: exact.  Scale: at most 3 float32 ulps from the reference's
float32(std64(ym)) / float32(std64(xm)) -- each of the two float64 stds is rounded to float32, and a last-bit difference of the float64
std (summation order) can put that rounding on the other side of a boundary: one ulp each, plus one for the float32 division; and 1e-6
relative against the numpy float32 oracle (the bar of tests/test_joint_params_gpu.py).  Translation: 1e-12 absolute from the reference
formula evaluated with the scale the kernel returned (float32 elements, contraction off: only the float64 summation order differs,
4096 * 2^-53 * |element|).  dynam: 1e-12 (tests/test_eval_scripts_gpu.py::test_part_extents_kernel).  Articulation block: NaN pattern
equal, finite entries within 1e-12 * max(1, |want|) (test_articulation_gpu.py::test_against_the_offline_kernels), the reference evaluated
with the kernel's part-0 similarity, which the scale / translation bars have bounded.

The non-finite cases state numpy's rules, which these kernels replace: a NaN vote makes that channel's np.median NaN, a NaN mask entry
is np.argmax's label, a part whose row means are all equal has a two-pass std of exactly 0."""
import os
import warnings

import numpy as np
import pytest
import torch

import eval_cases as EC
from redzone import guarded

pytestmark = pytest.mark.gpu
SEEDS = range(int(os.environ.get("ANCSH_EVAL_SWEEP_SEEDS", "40")))
FIGURES = dict(parts=0, exact=0, worst_ulp=0, worst_t=0.0, seeds=0)


def T(a, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt).contiguous()


def run(case, dev, record=None):
    """the four wrappers on one case -> numpy"""
    from articulated_pose_amd.pose.evaluation import part_extents
    from articulated_pose_amd.pose.joint_params import articulation_batch, joint_params_batch, joint_params_gt_batch
    B, n, K = case["B"], case["n"], case["K"]
    rec = case["record"] if record is None else record
    R0, s0, t0 = rec[:, 0, 13:22].reshape(B, 3, 3), rec[:, 0, 22], rec[:, 0, 23:26]
    pred = {"gocs_per_point": case["gocs"], "nocs_per_point": case["nocs"], "instance_per_point": case["mask"],
            "heatmap_per_point": case["heatmap"], "unitvec_per_point": case["unitvec"], "joint_axis_per_point": case["joint_axis"],
            "index_per_point": case["index"]}
    jp = joint_params_batch(pred, K, s0, R0, t0, device=dev)
    gt = joint_params_gt_batch({"nocs_gt_g": case["gocs"][:, :, :3], "heatmap_gt": case["heatmap"], "unitvec_gt": case["unitvec"],
                                "joint_axis_gt": case["joint_axis"], "joint_cls_gt": case["joint_cls"]}, K, np.ones(B),
                               np.tile(np.eye(4), (B, 1, 1)), device=dev)
    ancsh = {"gocs_per_point": T(case["gocs"], dev), "nocs_per_point": T(case["nocs"], dev), "W": T(case["mask"], dev),
             "heatmap_per_point": T(case["heatmap"][:, :, None], dev), "unitvec_per_point": T(case["unitvec"], dev),
             "joint_axis_per_point": T(case["joint_axis"], dev), "index_per_point": T(case["index"], dev)}
    npcs = {"nocs_per_point": T(case["npcs_nocs"], dev), "W": T(case["npcs_mask"], dev)}
    art, dbg = articulation_batch(ancsh, npcs, T(rec, dev, torch.float64), debug=True)
    ext = part_extents(npcs["nocs_per_point"], npcs["W"], T(case["P"], dev), R0, t0)
    ext_g = part_extents(ancsh["gocs_per_point"], ancsh["W"], T(case["P"], dev), R0, t0)
    got = {k: v.cpu().numpy() for k, v in jp.items()}
    got.update({"gt_" + k: v.cpu().numpy() for k, v in gt.items()})
    got.update(art=art.cpu().numpy(), npcs_extent=ext[0].cpu().numpy(), npcs_dynam=ext[1].cpu().numpy(), npcs_count=ext[2].cpu().numpy(),
               g_extent=ext_g[0].cpu().numpy(), g_dynam=ext_g[1].cpu().numpy(), g_count=ext_g[2].cpu().numpy())
    got.update({"dbg_" + k: v.cpu().numpy() for k, v in dbg.items()})
    return got


def check_medians(case, got, ref):
    for b in range(case["B"]):
        for j in range(1, case["K"]):
            msg = EC.describe(case, b, j)
            np.testing.assert_array_equal(got["joint_pt"][b, j - 1], ref["joint_pt"][b, j - 1], err_msg="joint_pt " + msg)
            np.testing.assert_array_equal(got["joint_axis"][b, j - 1], ref["joint_axis"][b, j - 1], err_msg="joint_axis " + msg)
            np.testing.assert_array_equal(got["gt_joint_pt"][b, j - 1], ref["gt_joint_pt"][b, j - 1], err_msg="gt joint_pt " + msg)
            np.testing.assert_array_equal(got["gt_joint_axis"][b, j - 1], ref["gt_joint_axis"][b, j - 1], err_msg="gt joint_axis (mean) " + msg)
            np.testing.assert_array_equal(got["dbg_joint_nocs"][b, j - 1, :3], ref["joint_pt"][b, j - 1], err_msg="joint_nocs pt " + msg)
            np.testing.assert_array_equal(got["dbg_joint_nocs"][b, j - 1, 3:], ref["joint_axis"][b, j - 1], err_msg="joint_nocs axis " + msg)


def check_similarity(case, got, ref, figures=None):
    """-> (parts, exact, worst ulp, worst translation error) of the finite parts"""
    K, msg = case["K"], EC.describe(case)
    st0 = np.concatenate([got["scale"][:, :1], got["translation"][:, 0]], 1) if K > 1 else np.full((case["B"], 4), np.nan)
    np.testing.assert_array_equal(got["dbg_st0"], st0, err_msg="st0 " + msg)          # K == 1: no joint workgroup, NaN
    fin = np.isfinite(ref["scale"])
    np.testing.assert_array_equal(got["scale"][~fin], ref["scale"][~fin], err_msg="scale (non-finite) " + msg)
    assert np.array_equal(got["scale"], got["scale"].astype(np.float32).astype(np.float64), equal_nan=True), msg     # a float32 value
    d = EC.ulps(got["scale"][fin], ref["scale"][fin])
    want_t = EC.translation(case, got["scale"])
    tfin = np.isfinite(want_t)
    np.testing.assert_array_equal(got["translation"][~tfin], want_t[~tfin], err_msg="translation (non-finite) " + msg)
    dt = np.abs(got["translation"][tfin] - want_t[tfin])
    out = (int(fin.sum()), int((d == 0).sum()), int(d.max()) if d.size else 0, float(dt.max()) if dt.size else 0.0)
    print("%s: scale exact in %d of %d parts, worst %d ulp; translation worst %.3g" % (msg, out[1], out[0], out[2], out[3]))
    assert out[2] <= 3, "scale %d ulp from the reference, %s" % (out[2], msg)
    assert out[3] <= 1e-12, "translation %.3g from the reference at the kernel's scale, %s" % (out[3], msg)
    from oracle import joint_params_oracle as JO                                      # second assertion: the numpy float32 oracle, 1e-6
    for b in range(case["B"]):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            sc = JO.st_and_joints(case["gocs"][b], case["nocs"][b], case["mask"][b], case["heatmap"][b], case["unitvec"][b],
                                  case["joint_axis"][b], np.argmax(case["index"][b], axis=1), K)[0]
        f = fin[b]
        np.testing.assert_allclose(got["scale"][b][f], sc[f], rtol=1e-6, atol=0, err_msg="scale vs oracle " + EC.describe(case, b))
    return out


def check_extents(case, got, ref):
    msg = EC.describe(case)
    for k in ("npcs", "g"):
        np.testing.assert_array_equal(got[k + "_count"], ref[k + "_count"], err_msg=k + " count " + msg)
        np.testing.assert_array_equal(got[k + "_extent"], ref[k + "_extent"], err_msg=k + " extent " + msg)
        want = ref[k + "_dynam"]
        assert np.array_equal(np.isnan(got[k + "_dynam"]), np.isnan(want)), msg
        fin = ~np.isnan(want)
        assert np.all(np.abs(got[k + "_dynam"][fin] - want[fin]) <= 1e-12), k + " dynam " + msg
    np.testing.assert_array_equal(got["dbg_extent"], ref["npcs_extent"], err_msg="articulation extent " + msg)


def check_block(case, got, ref, record=None):
    msg = EC.describe(case)
    c = case if record is None else dict(case, record=record)
    want = EC.articulation(c, ref, st0=got["dbg_st0"])
    art = got["art"]
    assert np.array_equal(np.isnan(art), np.isnan(want)), "NaN pattern " + msg
    fin = np.isfinite(want)
    np.testing.assert_array_equal(art[~fin], want[~fin], err_msg="block (non-finite) " + msg)
    err = np.abs(art[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert np.all(err <= 1e-12), "block %.3g, %s" % (err.max(), msg)
    return want


def check_all(case, got, ref):
    check_medians(case, got, ref)
    out = check_similarity(case, got, ref)
    check_extents(case, got, ref)
    check_block(case, got, ref)
    return out


def sweep(dev, seed):
    """one seed of the sweep, not guarded: tests/test_redzone_gpu.py runs it under its own arena"""
    case = EC.make_case(seed)
    ref = EC.reference(case)
    got = run(case, dev)
    parts, exact, worst, worst_t = check_all(case, got, ref)
    FIGURES["parts"] += parts
    FIGURES["exact"] += exact
    FIGURES["worst_ulp"] = max(FIGURES["worst_ulp"], worst)
    FIGURES["worst_t"] = max(FIGURES["worst_t"], worst_t)
    FIGURES["seeds"] += 1
    if case["B"] >= 2:                                   # a poisoned record: that cloud's block all NaN, its neighbours unchanged
        b = case["B"] // 2
        rec = case["record"].copy()
        rec[b, 0, 13 + seed % 13] = np.nan
        bad = run(case, dev, record=rec)["art"]
        assert np.isnan(bad[b]).all(), EC.describe(case, b)
        keep = np.arange(case["B"]) != b
        np.testing.assert_array_equal(bad[keep], got["art"][keep], err_msg="neighbours of a poisoned cloud " + EC.describe(case, b))


@pytest.mark.parametrize("seed", SEEDS)
def test_sweep(dev, seed):
    with guarded() as arena:
        sweep(dev, seed)
        assert arena.check() >= 8


def test_sweep_figures(dev):
    """prints the sweep's totals (information; the bars are asserted per seed)"""
    print("eval sweep over %(seeds)d seeds: scale exact in %(exact)d of %(parts)d parts, worst %(worst_ulp)d float32 ulp; "
          "worst translation error %(worst_t).3g" % FIGURES)


def test_lds_limits(dev):
    """n = 4096 with one joint holding all 4096 votes: six columns of 4096 floats = 96 KB of dynamic LDS, past the 48 KB a launch gets
    without asking (p2 == npow2: no padding at all).  n = 4097 would need 192 KB: refused with ValueError before any launch."""
    from articulated_pose_amd.pose.joint_params import articulation_batch, joint_params_batch
    with guarded():
        for G, lay in ((3, "permutation"), (6, "tail")):
            case = EC.make_case(12, n=4096, K=2, B=2, G=G, JC=2, counts=[[4096], [4096]], layouts=[[lay], ["run64"]])
            assert [v["count"] for v in case["votes"]] == [4096, 4096]
            check_all(case, run(case, dev), EC.reference(case))
        case = EC.make_case(1, n=4097, K=2, B=1, G=3, JC=2)
        pred = {"gocs_per_point": case["gocs"], "nocs_per_point": case["nocs"], "instance_per_point": case["mask"],
                "heatmap_per_point": case["heatmap"], "unitvec_per_point": case["unitvec"], "joint_axis_per_point": case["joint_axis"],
                "index_per_point": case["index"]}
        with pytest.raises(ValueError, match="too large"):
            joint_params_batch(pred, 2, np.ones(1), np.eye(3)[None], np.zeros((1, 3)), device=dev)
        ancsh = {k: T(v, dev) for k, v in pred.items()}
        ancsh["W"] = ancsh["instance_per_point"]
        with pytest.raises(ValueError, match="too large"):
            articulation_batch(ancsh, {"nocs_per_point": T(case["npcs_nocs"], dev), "W": T(case["npcs_mask"], dev)},
                               T(case["record"], dev, torch.float64))
        torch.cuda.synchronize()


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------

NF_N = (65, 257, 1000)
NF_COUNTS = {65: (33, 34, 64), 257: (129, 130, 256), 1000: (513, 514, 512)}          # odd, even, a power of two
NF_G = {65: 3, 257: 9, 1000: 3}


def _nf_case(n, seed):
    """nine clouds, K = 3: joint 1 of cloud 3 p + c has NF_COUNTS[n][c] votes (the NaN goes to vote position p: first, last, middle)"""
    counts = [[NF_COUNTS[n][c], 1] for _p in range(3) for c in range(3)]
    lays = [[EC.LAYOUTS[(p + c) % 4], "permutation"] for p in range(3) for c in range(3)]
    return EC.make_case(seed, n=n, K=3, B=9, G=NF_G[n], JC=3, counts=counts, layouts=lays)


@pytest.mark.parametrize("source", ["unitvec", "heatmap", "gocs"])
@pytest.mark.parametrize("n", NF_N)
def test_nan_vote_gives_a_nan_median(dev, n, source):
    """np.median of a column with a NaN is NaN: one NaN vote, at the first, the last and a middle vote of an odd, an even and a
    power-of-two count, reaching the votes through unitvec (one channel), heatmap (the three pivot channels) or the global NOCS of the
    point's part (one channel).  The other channels' medians equal the reference."""
    case = _nf_case(n, 100 + n)
    K, G = 3, case["G"]
    lab = EC.labels_of(case["mask"])
    hit = {}
    for v in case["votes"]:
        if v["joint"] != 1:
            continue
        b = v["cloud"]
        i = int(v["idx"][(0, -1, v["count"] // 2)[b // 3]])
        ch = (b + n) % 3
        if source == "unitvec":
            case["unitvec"][b, i, ch] = np.nan
        elif source == "heatmap":
            case["heatmap"][b, i] = np.nan
        else:
            case["gocs"][b, i, ch if G == 3 else 3 * lab[b, i] + ch] = np.nan
        hit[b] = [0, 1, 2] if source == "heatmap" else [ch]
    ref = EC.reference(case)
    with guarded():
        got = run(case, dev)
    for b, chans in hit.items():
        msg = "%s NaN vote through %s, channels %s" % (EC.describe(case, b, 1), source, chans)
        assert np.isnan(ref["joint_pt"][b, 0, chans]).all() and np.isfinite(np.delete(ref["joint_pt"][b, 0], chans)).all(), msg
        assert np.isnan(got["joint_pt"][b, 0, chans]).all(), "joint_pt " + msg
        assert np.isnan(got["dbg_joint_nocs"][b, 0, chans]).all(), "joint_nocs " + msg
        if source != "gocs" or G == 3:                   # the ground-truth variant reads the first triple only
            assert np.isnan(got["gt_joint_pt"][b, 0, chans]).all(), "gt joint_pt " + msg
    check_medians(case, got, ref)


@pytest.mark.parametrize("n", NF_N)
def test_nan_axis_vote_and_infinite_votes(dev, n):
    """a NaN among the joint_axis votes (median NaN; the ground-truth mean NaN too); +-inf votes: the medians equal np.median, an even
    count whose middle two are -inf and +inf gives NaN"""
    counts = [[c, 2] for c in NF_COUNTS[n]] + [[1, 2], [2, 3], [3, 4], [4, 1]]
    case = EC.make_case(200 + n, n=n, K=3, B=7, G=NF_G[n], JC=3, counts=counts)
    rng = np.random.RandomState(n)
    for v in case["votes"]:
        b, idx = v["cloud"], v["idx"]
        if v["joint"] == 1 and b < 3:                    # one NaN axis vote
            case["joint_axis"][b, idx[rng.randint(len(idx))], b] = np.nan
        elif len(idx):                                   # about half the votes +-inf, through the axis and through the unit vector
            sel = idx[rng.rand(len(idx)) < 0.5]
            case["joint_axis"][b, sel] = np.where(rng.rand(len(sel), 3) < 0.5, -np.inf, np.inf)
            case["heatmap"][b, sel] = 0.25               # 1 - heatmap > 0: the offset keeps the unit vector's sign
            case["unitvec"][b, sel] = np.where(rng.rand(len(sel), 3) < 0.5, -np.inf, np.inf)
    two = [v for v in case["votes"] if v["count"] == 2][0]                 # an even count: -inf and +inf in the middle
    case["joint_axis"][two["cloud"], two["idx"]] = np.asarray([[-np.inf] * 3, [np.inf] * 3], np.float32)
    ref = EC.reference(case)
    assert np.isnan(ref["joint_axis"][two["cloud"], two["joint"] - 1]).all()
    for b in range(3):
        assert np.isnan(ref["joint_axis"][b, 0, b]) and np.isnan(ref["gt_joint_axis"][b, 0, b]) and np.isfinite(ref["joint_axis"][b, 0]).sum() == 2
    assert np.isinf(ref["joint_pt"]).any() and np.isinf(ref["joint_axis"]).any()
    with guarded():
        got = run(case, dev)
    check_medians(case, got, ref)


@pytest.mark.parametrize("n", NF_N)
def test_nan_mask_entry_is_the_label(dev, n):
    """np.argmax returns the first NaN: a point whose mask row has a NaN at index k > 0 belongs to part k in the similarity, in the
    extents and counts, and in the choice of its global-NOCS triple (G = 3K); the same for the NPCS mask of the articulation block"""
    case = EC.make_case(300 + n, n=n, K=3, B=3, G=9, JC=3)
    rng = np.random.RandomState(n)
    before = EC.labels_of(case["mask"]).copy(), EC.labels_of(case["npcs_mask"]).copy()
    for name in ("mask", "npcs_mask"):
        for b in range(3):
            for i in range(b, n, 5):
                k = int(rng.randint(1, 3))
                case[name][b, i, k] = np.nan
                if k == 1 and i % 2:
                    case[name][b, i, 2] = np.nan         # two NaNs: the first one
    lab = EC.labels_of(case["mask"])
    assert (lab != before[0]).any() and (EC.labels_of(case["npcs_mask"]) != before[1]).any()
    assert (lab[:, 0::5][0] >= 1).all()
    assert not EC.badly_conditioned(case)
    ref = EC.reference(case)
    with guarded():
        got = run(case, dev)
        check_all(case, got, ref)


@pytest.mark.parametrize("y_constant", [False, True])
@pytest.mark.parametrize("n", NF_N)
def test_part_of_equal_row_means_has_zero_variance(dev, n, y_constant):
    """numpy's two-pass std of bit-equal values is exactly 0: a part whose global-NOCS triple is (0.3, 0.7, 0.2) at every point has
    scale std(ym) / 0 = inf and translation mean(y - inf * x) = -inf; with the part NOCS constant as well, 0 / 0 = NaN.  Part 0 of each
    cloud: 600 points at n = 1000, the whole cloud at n = 257 (and at n = 65, below the size the case is about, for the small end)."""
    case = EC.make_case(400 + n, n=n, K=3, B=2, G=3 if y_constant else 9, JC=3)
    if n < 1000:
        case["mask"][:, :, 0] = 1.0
    else:
        case["mask"][:, :600, 0] = 1.0
    lab = EC.labels_of(case["mask"])
    for b in range(2):
        idx = np.where(lab[b] == 0)[0]
        assert len(idx) >= min(n, 257)
        case["gocs"][b, idx, :3] = np.asarray([0.3, 0.7, 0.2], np.float32)
        if y_constant:
            case["nocs"][b, idx, :3] = np.asarray([0.6, 0.1, 0.9], np.float32)
    ref = EC.reference(case)
    assert np.isnan(ref["scale"][:, 0]).all() if y_constant else np.isposinf(ref["scale"][:, 0]).all()
    assert np.isnan(ref["translation"][:, 0]).all() if y_constant else np.isneginf(ref["translation"][:, 0]).all()
    with guarded():
        got = run(case, dev)
    msg = EC.describe(case)
    np.testing.assert_array_equal(got["scale"][:, 0], ref["scale"][:, 0], err_msg="scale " + msg)
    np.testing.assert_array_equal(got["translation"][:, 0], ref["translation"][:, 0], err_msg="translation " + msg)
    np.testing.assert_array_equal(got["dbg_st0"][:, 0], ref["scale"][:, 0], err_msg="st0 " + msg)
    np.testing.assert_array_equal(got["dbg_st0"][:, 1:], ref["translation"][:, 0], err_msg="st0 " + msg)
    check_medians(case, got, ref)
    check_block(case, got, ref)
