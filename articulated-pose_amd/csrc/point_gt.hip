// point_gt.hip -- what a streamed batch's PER-POINT ground truth says about it: the test-time losses of both networks (lib/network.py:257-316
// over lib/loss.py, the numbers behind test_loss.txt) and step 5 of evaluation.sh, the joint axis angle error and line-to-line distance in
// camera space (evaluation/eval_joint_params.py:189-256), per cloud, in ONE launch behind the articulation launches.  It carries the pose
// record (26 / 39 / 38 / 51 columns) along in columns 0..ld-1 of its (b, K, ld + 21) block.
//
// One workgroup of 256 threads per cloud.  The ground truth is never gathered into tensors: sampled point i of cloud c is raw row
// offsets[c] + perm[c][i] % n_raw of the slot's 18-channel rows (dataset.pack_cloud's layout), read where it lies by ancsh_input_sample's
// rules.  Pass 1 is test_losses_kernel's loop with two networks' heads behind one ground-truth row: thread tid takes points tid, tid + 256,
// ..., float32 element arithmetic, float64 partial sums, xor-shuffle wave sums, four waves added in order -- the statements of loss.hip, so
// every loss is bit-equal to ancsh_test_losses on the gathered tensors.  Pass 2, per joint class j >= 1, is joint_params_kernel's
// axis_mean = 1 path on the ground-truth channels: ordered compaction of the votes into six LDS columns (part_stats.h's layout), the float32
// mean of the orientations in point order, the bitonic sort of the pivot's three columns and the exact medians of nocs_g + unitvec *
// (1 - heatmap) * 0.2 -- bit-equal to ancsh_joint_params.  Its raw rows were read a moment ago by pass 1 and come from L2.  Thread j < K then takes joint j to camera space
// through the ground-truth NAOCS pose of part 0 and compares it with the articulation block's predicted joint, float64 as written.
// No atomics, nothing allocated, every size an argument or read from device memory: capturable, and the same bytes every run.
#include "part_stats.h"

namespace ancsh {

constexpr int PG_KM = 8;
constexpr int PG_NCHAN = 18;                       // x y z | cls | nocs_p 3 | nocs_g 3 | heatmap | unitvec 3 | orient 3 | joint_cls
constexpr int PG_WIDTH = 21;
constexpr int PG_NA = 5 + 3 * PG_KM + 9;           // the ANCSH sums, test_losses_kernel's layout: 5 scalars, (dot, sumW, cnt) x K, the same x 3
constexpr int PG_NB = 1 + 3 * PG_KM;               // the NPCS sums: nocs, (dot, sumW, cnt) x K
constexpr int PG_NACC = PG_NA + PG_NB;

struct PointGtArgs {
    const float *rows;
    const int *offsets, *perm;
    const float *W, *nocs, *gocs, *heatmap, *unitvec, *axis, *index, *npcs_W, *npcs_nocs;
    const double *art, *frame, *record;
    double *wide, *joint_gt;
    long capacity;
    int n, K, G, JC, ld_art, ld, type_l;
};

// loss.hip's dist3 and wave_sum_f64, statement for statement
__device__ __forceinline__ float pg_dist3(const float *a, const float *b, int type_l) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return type_l == 0 ? sqrtf(dx * dx + dy * dy + dz * dz) : fabsf(dx) + fabsf(dy) + fabsf(dz);
}

__device__ __forceinline__ double pg_wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void point_gt_kernel(PointGtArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float pg_vals[];              // 6 * npow2 floats: the votes' columns (K > 1)
    __shared__ double red[4][PG_NACC];
    __shared__ int redj[4][PG_KM];
    __shared__ int wcnt[4];
    __shared__ double sjoint[PG_KM][6];              // row j: the ground-truth joint j in global NOCS, point (3) | axis (3)
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, K = a.K, ld = a.ld, wd = ld + PG_WIDTH;
    const size_t p0 = (size_t)c * n;
    // columns 0..ld-1: the input rows, moved as 64-bit words so that a NaN keeps its payload
    {
        const unsigned long long *rb = reinterpret_cast<const unsigned long long *>(a.record + (size_t)c * K * ld);
        unsigned long long *wb = reinterpret_cast<unsigned long long *>(a.wide + (size_t)c * K * wd);
        for (int e = tid; e < K * ld; e += 256) wb[(e / ld) * wd + e % ld] = rb[e];
    }
    const long r0 = a.offsets[c], r1 = a.offsets[c + 1];
    if (r0 < 0 || r1 <= r0 || r1 > a.capacity) {      // empty or outside the rows buffer (the host refuses both): no ground truth to read
        for (int e = tid; e < K * PG_WIDTH; e += 256) a.wide[((size_t)c * K + e / PG_WIDTH) * wd + ld + e % PG_WIDTH] = NAN;
        if (a.joint_gt)
            for (int e = tid; e < (K - 1) * 6; e += 256) a.joint_gt[(size_t)c * (K - 1) * 6 + e] = NAN;
        return;
    }
    const int n_raw = (int)(r1 - r0);
    const float *rows = a.rows + (size_t)r0 * PG_NCHAN;
    const bool g3k = a.G == 3 * K, idx3 = a.JC == 3;
    // ---- pass 1: the sums behind both networks' losses, and the points per joint class
    double acc[PG_NACC];
    int jcnt[PG_KM];
#pragma unroll
    for (int i = 0; i < PG_NACC; ++i) acc[i] = 0.0;
#pragma unroll
    for (int k = 0; k < PG_KM; ++k) jcnt[k] = 0;
    for (int i = tid; i < n; i += 256) {
        const size_t p = p0 + i;
        int r = a.perm[p] % n_raw;
        if (r < 0) r += n_raw;                        // a sampler's index is never negative; nothing is read outside the cloud either way
        const float *src = rows + (size_t)r * PG_NCHAN;
        const float cls = src[3], jc = src[17];
        const int lab = (int)cls;                     // cls_gt: C truncation, as np.asarray(x, np.int32)
        const int lab8 = (int)(signed char)(int)cls;  // mask_array: one-hot of astype(np.int8) with numpy's negative-index rule
        const int jl = (int)jc;
        const float jm = jc > 0.f ? 1.f : 0.f;        // joint_cls_mask
        const float ng[3] = {src[4], src[5], src[6]}, gg[3] = {src[7], src[8], src[9]};
        const float hg = src[10], ug[3] = {src[11], src[12], src[13]}, og[3] = {src[14], src[15], src[16]};
        float s_nocs = 0.f, s_gocs = 0.f, s_npcs = 0.f;
#pragma unroll
        for (int k = 0; k < PG_KM; ++k) {
            if (k < K) {
                const float m = (lab8 == k || lab8 + K == k) ? 1.f : 0.f;
                s_nocs += m * pg_dist3(a.nocs + p * 3 * K + 3 * k, ng, a.type_l);
                if (g3k) s_gocs += m * pg_dist3(a.gocs + p * 3 * K + 3 * k, gg, a.type_l);
                const float w = a.W[p * K + k];
                acc[5 + 3 * k] += lab == k ? (double)w : 0.0;
                acc[5 + 3 * k + 1] += (double)w;
                acc[5 + 3 * k + 2] += lab == k ? 1.0 : 0.0;
                s_npcs += m * pg_dist3(a.npcs_nocs + p * 3 * K + 3 * k, ng, a.type_l);
                const float wn = a.npcs_W[p * K + k];
                acc[PG_NA + 1 + 3 * k] += lab == k ? (double)wn : 0.0;
                acc[PG_NA + 1 + 3 * k + 1] += (double)wn;
                acc[PG_NA + 1 + 3 * k + 2] += lab == k ? 1.0 : 0.0;
                jcnt[k] += jl == k ? 1 : 0;
            }
        }
        acc[0] += (double)s_nocs;
        acc[1] += (double)s_gocs;
        acc[2] += (double)(fabsf(a.heatmap[p] - hg) * jm);
        acc[3] += (double)(pg_dist3(a.unitvec + p * 3, ug, a.type_l) * jm);
        acc[4] += (double)(pg_dist3(a.axis + p * 3, og, a.type_l) * jm);
        acc[PG_NA] += (double)s_npcs;
        if (idx3) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float w = a.index[p * 3 + k];
                acc[5 + 3 * PG_KM + 3 * k] += jl == k ? (double)w : 0.0;
                acc[5 + 3 * PG_KM + 3 * k + 1] += (double)w;
                acc[5 + 3 * PG_KM + 3 * k + 2] += jl == k ? 1.0 : 0.0;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PG_NACC; ++i) {
        const double s = pg_wave_sum_f64(acc[i]);
        if (lane == 0) red[wave][i] = s;
    }
#pragma unroll
    for (int k = 0; k < PG_KM; ++k) {
        int s = jcnt[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) redj[wave][k] = s;
    }
    // ---- pass 2: the ground-truth joints (eval_joint_params.py:189-199), joint_params_kernel's axis_mean path on the raw rows' channels
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    for (int j = 1; j < K; ++j) {
        int cnt = 0;
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int i = c0 + tid;
            const float *src = rows;
            bool f = false;
            if (i < n) {
                int r = a.perm[p0 + i] % n_raw;
                if (r < 0) r += n_raw;
                src = rows + (size_t)r * PG_NCHAN;
                f = (int)src[17] == j;
            }
            const unsigned long long mm = __ballot(f);
            __syncthreads();
            if (lane == 0) wcnt[wave] = __popcll(mm);
            __syncthreads();
            int start = cnt;
            for (int w = 0; w < wave; ++w) start += wcnt[w];
            if (f) {
                const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(mm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mm, 0));
                const float w1 = 1.0f - src[10];
#pragma unroll
                for (int c3 = 0; c3 < 3; ++c3) {
                    pg_vals[c3 * npow2 + pos] = src[14 + c3];
                    const float off = (src[11 + c3] * w1) * 0.2f;      // unitvec * (1 - heatmap) * thres_r, float32
                    pg_vals[(3 + c3) * npow2 + pos] = src[7 + c3] + off;
                }
            }
            cnt += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        }
        __syncthreads();
        if (tid < 3) {                               // np.mean(orient_gt[idx], axis=0): float32 accumulation row by row, then / count
            const float *v = pg_vals + tid * npow2;
            float s = 0.f;
            int e = 0;
            for (; e + 8 <= cnt; e += 8) {             // eight LDS reads in flight, the additions still one after another in point order
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = v[e + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) s = s + x[u];
            }
            for (; e < cnt; ++e) s = s + v[e];
            sjoint[j][3 + tid] = cnt > 0 ? (double)(s / (float)cnt) : NAN;
        }
        __syncthreads();
        ANCSH_SORT_VOTE_COLUMNS_FROM(pg_vals, npow2, cnt, 3)      // the pivot's three columns: the axis is the mean taken above
        if (tid >= 3 && tid < 6) {
            ANCSH_VOTE_MEDIAN(med, pg_vals, npow2, cnt, p2, tid)
            sjoint[j][tid - 3] = med;
        }
        __syncthreads();                             // the columns are free for the next joint; sjoint[j] is visible
    }
    __syncthreads();                                 // red, redj (and K == 1: nothing else) are visible
    if (tid >= K) return;
    // ---- thread j: row j's 21 columns
    const int j = tid;
    double *o = a.wide + ((size_t)c * K + j) * wd + ld;
    auto total = [&](int i) { return red[0][i] + red[1][i] + red[2][i] + red[3][i]; };
    auto miou = [&](int base) {
        const double dot = total(base), sw = total(base + 1), cn = total(base + 2);
        return (double)(float)(1.0 - dot / (cn + sw - dot + 1e-10));          // DIVISION_EPS, lib/constants.py:1; float32 like ancsh_test_losses' out
    };
    o[8] = miou(5 + 3 * j);
    o[9] = miou(PG_NA + 1 + 3 * j);
    o[10] = total(5 + 3 * j + 2);
    o[11] = (double)(redj[0][j] + redj[1][j] + redj[2][j] + redj[3][j]);
    o[12] = (double)(float)(total(0) / (double)n);
    o[13] = g3k ? (double)(float)(total(1) / (double)n) : NAN;
    o[14] = (double)(float)(total(2) / (double)n);
    o[15] = (double)(float)(total(3) / (double)n);
    o[16] = (double)(float)(total(4) / (double)n);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[17 + k] = idx3 ? miou(5 + 3 * PG_KM + 3 * k) : NAN;
    o[20] = (double)(float)(total(PG_NA) / (double)n);
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = NAN;
        return;
    }
    const double *q = sjoint[j];
    if (a.joint_gt) {
        double *dbg = a.joint_gt + ((size_t)c * (K - 1) + (j - 1)) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) dbg[k] = q[k];
    }
    // ---- camera space (eval_joint_params.py:224-231): p_gt = R (s p) + t, l_gt = R l through the ground-truth NAOCS pose of part 0
    const double *fr = a.frame + (size_t)c * 13, s = fr[9], *t = fr + 10;
    bool blank = false;
#pragma unroll
    for (int k = 0; k < 13; ++k) blank |= fr[k] != fr[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) blank |= q[k] != q[k];                          // a joint class without ground-truth points
    const double sp[3] = {s * q[0], s * q[1], s * q[2]};
    double pg[3], lg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *rk = fr + 3 * k;
        pg[k] = ((sp[0] * rk[0] + sp[1] * rk[1]) + sp[2] * rk[2]) + t[k];
        lg[k] = (q[3] * rk[0] + q[4] * rk[1]) + q[5] * rk[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o[2 + k] = blank ? NAN : pg[k];
        o[5 + k] = blank ? NAN : lg[k];
    }
    // ---- the errors (:244-256): axis_diff_degree (lib/d3_utils.py:137-142: no clamp, min(a, 180 - a)) and dist_between_3d_lines (:165-174)
    const double *ar = a.art + ((size_t)c * K + j) * a.ld_art, *pp = ar + 6, *lp = ar + 9;
    bool dead = blank;
#pragma unroll
    for (int k = 6; k < 12; ++k) dead |= ar[k] != ar[k];                        // an empty predicted joint class, a poisoned record
    constexpr double PI = 3.14159265358979323846;
    const double dotp = (lg[0] * lp[0] + lg[1] * lp[1]) + lg[2] * lp[2];
    const double n1 = sqrt((lg[0] * lg[0] + lg[1] * lg[1]) + lg[2] * lg[2]), n2 = sqrt((lp[0] * lp[0] + lp[1] * lp[1]) + lp[2] * lp[2]);
    const double rd = acos(dotp / (n1 * n2)) * 180.0 / PI, rc = 180.0 - rd;
    const double orth[3] = {lg[1] * lp[2] - lg[2] * lp[1], lg[2] * lp[0] - lg[0] * lp[2], lg[0] * lp[1] - lg[1] * lp[0]};
    const double prod = (orth[0] * (pg[0] - pp[0]) + orth[1] * (pg[1] - pp[1])) + orth[2] * (pg[2] - pp[2]);
    const double on = sqrt((orth[0] * orth[0] + orth[1] * orth[1]) + orth[2] * orth[2]);
    o[0] = dead ? NAN : (rc < rd ? rc : rd);
    o[1] = dead ? NAN : fabs(prod / on);
}

}  // namespace ancsh

extern "C" int ancsh_point_gt_rec(int b, int n, int K, int nchan, const float *rows, long capacity, const int *offsets, const int *perm,
                                  int gocs_channels, int joint_channels, const float *W, const float *nocs, const float *gocs,
                                  const float *heatmap, const float *unitvec, const float *joint_axis, const float *joint_index,
                                  const float *npcs_W, const float *npcs_nocs, const double *art, int ld_art, const double *frame,
                                  const double *record, int ld, int type_l, double *wide, double *joint_gt, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0 && b <= 65535, "point_gt_rec: b=%d (0..65535)", b);
    ANCSH_REQUIRE(K >= 1 && K <= PG_KM, "point_gt_rec: K=%d (1..8)", K);
    ANCSH_REQUIRE(n >= 1 && n <= ANCSH_ARTICULATION_MAX_N, "point_gt_rec: n=%d (1..%d: the joint medians stay in LDS)", n, ANCSH_ARTICULATION_MAX_N);
    ANCSH_REQUIRE(nchan == PG_NCHAN, "point_gt_rec: nchan=%d (18: x y z | cls | nocs_p 3 | nocs_g 3 | heatmap | unitvec 3 | orient 3 | joint_cls)",
                  nchan);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "point_gt_rec: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(gocs_channels == 3 || gocs_channels == 3 * K, "point_gt_rec: gocs must have 3 or 3K = %d channels, got %d", 3 * K,
                  gocs_channels);
    ANCSH_REQUIRE(joint_channels >= 1 && joint_channels <= 8, "point_gt_rec: joint_channels=%d (1..8)", joint_channels);
    ANCSH_REQUIRE(ld_art == 12 || ld_art == 20, "point_gt_rec: ld_art=%d (12: the articulation block, 20: the joint-state block)", ld_art);
    ANCSH_REQUIRE(ld == 26 || ld == 39 || ld == 38 || ld == 51,
                  "point_gt_rec: ld=%d (26: the record, 39: the fit-quality wide record, 38 / 51: either with the ground-truth errors)", ld);
    ANCSH_REQUIRE(type_l == 0 || type_l == 1, "point_gt_rec: type_l=%d (0 = L2, 1 = L1)", type_l);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(rows && offsets && perm && W && nocs && gocs && heatmap && unitvec && joint_axis && joint_index && npcs_W && npcs_nocs && art &&
                  frame && record && wide, "point_gt_rec: null pointer");
    PointGtArgs a;
    a.rows = rows; a.offsets = offsets; a.perm = perm;
    a.W = W; a.nocs = nocs; a.gocs = gocs; a.heatmap = heatmap; a.unitvec = unitvec; a.axis = joint_axis; a.index = joint_index;
    a.npcs_W = npcs_W; a.npcs_nocs = npcs_nocs;
    a.art = art; a.frame = frame; a.record = record; a.wide = wide; a.joint_gt = K > 1 ? joint_gt : nullptr;
    a.capacity = capacity;
    a.n = n; a.K = K; a.G = gocs_channels; a.JC = joint_channels; a.ld_art = ld_art; a.ld = ld; a.type_l = type_l;
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    const size_t lds = K > 1 ? (size_t)6 * npow2 * sizeof(float) : 0;
    if (lds > 32 * 1024) (void)hipFuncSetAttribute((const void *)point_gt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(point_gt_kernel, dim3(b), dim3(256), lds, (hipStream_t)stream, a);
    return check_launch("point_gt_rec");
}
