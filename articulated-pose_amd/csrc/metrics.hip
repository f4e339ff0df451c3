// metrics.hip -- evaluation-side kernels.
//
// iou_3d (lib/d3_utils.py:40-69, called per part by evaluation/compute_miou.py:212-225): two oriented boxes (8 corners each),
// a nres^3 grid over their joint axis-aligned bounds, an inside-box test per grid point and box, IoU = |both| / |either|
// (1 when the union is empty).  The reference builds the 125 000 grid points with itertools.product and tests them with
// numpy, ~25 ms per pair; here ONE WORKGROUP per pair strides over the grid in registers (no point is ever materialised),
// counts by ballot + popcount and reduces 4 waves through LDS.  float64 like the reference: grid coordinates are
// numpy.linspace's (start + i*step, the last one exactly stop), the projections up.u are sums of three products in
// (x, y, z) order and the bounds np.dot(u, u).
#include "common.h"
#include "iou_grid.h"      // BoxFrame, box_frame, inside: shared with gt_errors.hip

namespace ancsh {

__global__ __launch_bounds__(256) void iou_3d_kernel(int nres, const double *__restrict__ bbox1, const double *__restrict__ bbox2,
                                                     double *__restrict__ iou, long *__restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ int red[2][4];
    const int pair = blockIdx.x;
    const double *b1 = bbox1 + (size_t)pair * 24, *b2 = bbox2 + (size_t)pair * 24;
    BoxFrame f1, f2;
    box_frame(b1, f1);
    box_frame(b2, f2);
    double lo[3], hi[3], step[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double mn = b1[c], mx = b1[c];
        for (int k = 0; k < 8; ++k) {
            mn = fmin(mn, fmin(b1[k * 3 + c], b2[k * 3 + c]));
            mx = fmax(mx, fmax(b1[k * 3 + c], b2[k * 3 + c]));
        }
        lo[c] = mn; hi[c] = mx;
        step[c] = (mx - mn) / (double)(nres - 1);          // numpy.linspace: step = delta / div
    }
    const long total = (long)nres * nres * nres;
    int both = 0, either = 0;
    for (long e = threadIdx.x; e < total; e += 256) {
        const int iz = (int)(e % nres), iy = (int)((e / nres) % nres), ix = (int)(e / ((long)nres * nres));
        // linspace: y = arange(num) * step + start, then y[-1] = stop
        const double x = ix == nres - 1 ? hi[0] : (double)ix * step[0] + lo[0];
        const double y = iy == nres - 1 ? hi[1] : (double)iy * step[1] + lo[1];
        const double z = iz == nres - 1 ? hi[2] : (double)iz * step[2] + lo[2];
        const bool i1 = inside(f1, x, y, z), i2 = inside(f2, x, y, z);
        both += (i1 & i2) ? 1 : 0;
        either += (i1 | i2) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { both += __shfl_xor(both, o, 64); either += __shfl_xor(either, o, 64); }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = both; red[1][wave] = either; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long I = (long)red[0][0] + red[0][1] + red[0][2] + red[0][3], U = (long)red[1][0] + red[1][1] + red[1][2] + red[1][3];
        iou[pair] = U == 0 ? 1.0 : (double)I / (double)U;
        if (counts) { counts[pair * 2] = I; counts[pair * 2 + 1] = U; }
    }
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_iou_3d(int npairs, int nres, const double *bbox1, const double *bbox2, double *iou, long *counts, void *stream) {
    ANCSH_REQUIRE(npairs >= 0 && nres >= 2 && nres <= 1024, "iou_3d: npairs=%d nres=%d (2..1024)", npairs, nres);
    if (npairs == 0) return ANCSH_OK;
    ANCSH_REQUIRE(bbox1 && bbox2 && iou, "iou_3d: null pointer");
    hipLaunchKernelGGL(iou_3d_kernel, dim3(npairs), dim3(256), 0, (hipStream_t)stream, nres, bbox1, bbox2, iou, counts);
    return check_launch("iou_3d");
}

// The shared passes of the three evaluation kernels below.  Included HERE, where their helpers used to be defined: the order of the
// functions in the module decides how the compiler inlines them, and joint_params_kernel keeps its instruction stream only in this order.
#include "part_stats.h"

namespace ancsh {

// ---- joint parameters from the per-point heads (evaluation/eval_joint_params.py:143-199) --------------------------------
// Per cloud, the reference (numpy, one sample at a time):
//   * per part j: x = global NOCS, y = part NOCS of the points labelled j (argmax of the mask);
//       scale_j = std(mean(y, axis=1)) / std(mean(x, axis=1)),  translation_j = mean(y - scale_j * x, axis=0)      (:160-171)
//   * per joint j >= 1: the points whose joint class is j vote   joint_pts = nocs_g + unitvec * (1 - heatmap) * 0.2   (:178-181);
//       joint point = per-channel MEDIAN of the votes, joint axis = per-channel median of joint_axis_per_point          (:183-184)
//       (ground-truth variant :192-199: the axis is the MEAN of the votes' orientations).
// One workgroup per (cloud, part) and per (cloud, joint).  float32 element arithmetic in numpy's order (the inputs are float32
// .h5 arrays); medians are exact selections (ordered compaction + bitonic sort per channel, as joint_direction_kernel in
// pose.hip); the reductions behind std / mean run in float64 (numpy: pairwise float32 -- equal to ~1e-7, tests bound 1e-6).
// The passes live in part_stats.h (ANCSH_PART_SIMILARITY, ANCSH_COMPACT_JOINT_VOTES, ANCSH_SORT_VOTE_COLUMNS), shared with articulation_kernel.
__global__ __launch_bounds__(256) void joint_params_kernel(int n, int K, int G, int axis_mean, const float *__restrict__ gocs,
                                                           const float *__restrict__ nocs, const float *__restrict__ mask,
                                                           const float *__restrict__ heatmap, const float *__restrict__ unitvec,
                                                           const float *__restrict__ axis, const int *__restrict__ joint_cls,
                                                           double *__restrict__ st, double *__restrict__ joint) {
    extern __shared__ float jp_vals[];   // 6 * npow2 floats (joint blocks)
    __shared__ double red[4];
    __shared__ int wcnt[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p0 = (size_t)b * n;
    if ((int)blockIdx.y < K) {           // ---- similarity global NOCS -> part NOCS of part j
        if (!nocs || !st) return;
        const int j = blockIdx.y;
        ANCSH_PART_SIMILARITY(n, K, G, j, p0, gocs, nocs, mask, red, st + ((size_t)b * K + j) * 4)
        return;
    }
    // ---- joint j: ordered compaction of the votes (index order), then per-channel median (or mean of the axis)
    const int j = (int)blockIdx.y - K + 1;
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    int cnt = 0;
    ANCSH_COMPACT_JOINT_VOTES(n, K, G, p0, npow2, gocs, mask, heatmap, unitvec, axis, joint_cls[p0 + i] == j, jp_vals, wcnt, lane, wave, cnt)
    __syncthreads();
    double *o = joint + ((size_t)b * (K - 1) + (j - 1)) * 6;
    if (axis_mean && threadIdx.x < 3) {      // np.mean(orient_gt[idx], axis=0): float32 accumulation row by row, then / count
        const float *v = jp_vals + threadIdx.x * npow2;
        float s = 0.f;
        for (int e = 0; e < cnt; ++e) s = s + v[e];
        o[3 + threadIdx.x] = cnt > 0 ? (double)(s / (float)cnt) : NAN;
    }
    __syncthreads();
    ANCSH_SORT_VOTE_COLUMNS(jp_vals, npow2, cnt)
    if (threadIdx.x < 6) {
        ANCSH_VOTE_MEDIAN(med, jp_vals, npow2, cnt, p2, threadIdx.x)
        if (threadIdx.x >= 3) o[threadIdx.x - 3] = med;            // joint point
        else if (!axis_mean) o[3 + threadIdx.x] = med;            // joint axis
    }
}

// ---- amodal-box extents and boundaries of the predicted parts (evaluation/compute_miou.py:196-208, eval_pose_err.py:253-268) ----
// Per cloud and part j (points whose predicted mask row has its first maximum at j):
//   scale_pred_j = 2 * max |nocs_j - 0.5| per channel   (float32, numpy's ops: subtraction, abs, max; the doubling is exact)
//   dynam_j      = min over the part's points of the x coordinate of the point taken back through part 0's pose:
//                  ([P 1] . pinv(rt_0^T))[:, 0] with rt_0 = compose_rt(R0, t0) in FLOAT32 (:25-30) = sum_c (P_c - t0_c) * R0[c][0],
//                  float64 products of the float32-rounded pose (the reference's float32 pinv differs from this inverse by ~1e-7)
//   count_j      = points of the part (0 -> the reference's np.max raises and its bare except drops the frame)
// One workgroup per cloud, all its parts in one pass (part_stats.h); HBM-bound: the mask, the point and the point's own NOCS slot are
// read once.
__global__ __launch_bounds__(256) void part_extents_kernel(int n, int K, int C, const float *__restrict__ nocs, const float *__restrict__ mask,
                                                           const float *__restrict__ P, int ldp, const double *__restrict__ pose0,
                                                           float *__restrict__ scale_pred, double *__restrict__ dynam,
                                                           int *__restrict__ count) {
    constexpr int KM = 8;
    __shared__ float smax[4][KM][3];
    __shared__ double smin[4][KM];
    __shared__ int scnt[4][KM];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p0 = (size_t)b * n;
    const double *ps = pose0 + (size_t)b * 12;                  // R0 row-major (9) | t0 (3)
    ANCSH_POSE0_FIRST_COLUMN(ps, ps + 9, r00, r10, r20, t0, t1, t2, m30)
    ANCSH_PART_EXTENTS_PASS(true, n, K, C, p0, nocs, mask, P, ldp, r00, r10, r20, m30, smax, smin, scnt, lane, wave)
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int j = threadIdx.x;
        const size_t o = (size_t)b * K + j;
        const int c = scnt[0][j] + scnt[1][j] + scnt[2][j] + scnt[3][j];
        count[o] = c;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            scale_pred[o * 3 + k] = c > 0 ? 2.0f * np_maxf(np_maxf(smax[0][j][k], smax[1][j][k]), np_maxf(smax[2][j][k], smax[3][j][k])) : NAN;
        dynam[o] = c > 0 ? np_min(np_min(smin[0][j], smin[1][j]), np_min(smin[2][j], smin[3][j])) : NAN;
    }
}

// ---- articulation block of the streamed step (pred side of compute_miou.py:196-222 and eval_joint_params.py:143-220) ----------------
// Per cloud b, row j of art (b, K, 12) float64, from the pose record's nonlinear R_j (cols 13..21), s_j (22), t_j (23..25):
//   0..2   box size     s_j * scale_pred_j,  scale_pred_j = 2 max |nocs_npcs_j - 0.5| over the NPCS network's part j   (:196-200, 214-217)
//   3..5   box centre   s_j * R_j (1/2, 1/2, 1/2) + t_j: the centre of get_3d_bbox(scale, shift=1/2) taken to camera space  (:217-222)
//   6..8   pivot        R_0 (s_0 (p_j s2 + t2)) + t_0;  p_j = per-channel median of the ANCSH votes of joint class j, (s2, t2) = the ANCSH
//                       part-0 similarity global -> part NOCS                                               (eval_joint_params.py:214-219)
//   9..11  axis         R_0 a_j;  a_j = per-channel median of joint_axis_per_point over the same points, not normalised    (:220)
// Row 0's joint columns are NaN; an empty part or joint class gives NaN in its own columns; a cloud whose part-0 nonlinear pose has a NaN
// (a poisoned record) gets an all-NaN block.  Workgroup (b, 0): every part's box (ANCSH_PART_EXTENTS_PASS); workgroup (b, j >= 1): joint j,
// recomputing part 0's similarity so that nothing waits for another workgroup.  The joint class is the first argmax of the ANCSH
// index_per_point (JC channels: joint j >= JC has no points).  The optional debug outputs joint_nocs (b, K-1, 6), st0 (b, 4) and
// extent (b, K, 3) are bit-equal to ancsh_joint_params' joint / st row 0 and ancsh_part_extents' scale_pred.
__global__ __launch_bounds__(256) void articulation_kernel(int n, int K, int G, int JC, const float *__restrict__ gocs,
                                                           const float *__restrict__ nocs, const float *__restrict__ mask,
                                                           const float *__restrict__ heatmap, const float *__restrict__ unitvec,
                                                           const float *__restrict__ axis, const float *__restrict__ joint_index,
                                                           const float *__restrict__ npcs_nocs, const float *__restrict__ npcs_mask,
                                                           const double *__restrict__ record, double *__restrict__ art,
                                                           double *__restrict__ joint_nocs, double *__restrict__ st0, float *__restrict__ extent) {
    extern __shared__ float art_vals[];   // 6 * npow2 floats (joint blocks)
    __shared__ double red[4];
    __shared__ double sst[4];
    __shared__ int wcnt[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p0 = (size_t)b * n;
    const double *rec = record + (size_t)b * K * 26;
    bool poisoned = false;
    for (int c = 13; c < 26; ++c) poisoned |= rec[c] != rec[c];
    double *ab = art + (size_t)b * K * 12;
    if (blockIdx.y == 0) {               // ---- the boxes of all parts
        constexpr int KM = 8;
        __shared__ float smax[4][KM][3];
        __shared__ int scnt[4][KM];
        double (*smin)[KM] = nullptr;                      // no boundary pass: never written
        const float *P = nullptr;
        ANCSH_PART_EXTENTS_PASS(false, n, K, 3 * K, p0, npcs_nocs, npcs_mask, P, 0, 0.0, 0.0, 0.0, 0.0, smax, smin, scnt, lane, wave)
        __syncthreads();
        if ((int)threadIdx.x < K) {
            const int j = threadIdx.x;
            const int c = scnt[0][j] + scnt[1][j] + scnt[2][j] + scnt[3][j];
            const double *r = rec + j * 26 + 13, s = r[9], *t = r + 10;
            double *o = ab + j * 12;
            const bool dead = poisoned || c == 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float e = c > 0 ? 2.0f * np_maxf(np_maxf(smax[0][j][k], smax[1][j][k]), np_maxf(smax[2][j][k], smax[3][j][k])) : NAN;
                if (extent) extent[((size_t)b * K + j) * 3 + k] = e;
                o[k] = dead ? NAN : s * (double)e;
                o[3 + k] = dead ? NAN : s * ((r[3 * k] * 0.5 + r[3 * k + 1] * 0.5) + r[3 * k + 2] * 0.5) + t[k];
            }
            if (j == 0)
#pragma unroll
                for (int k = 6; k < 12; ++k) o[k] = NAN;
        }
        if (K == 1 && st0 && threadIdx.x < 4) st0[(size_t)b * 4 + threadIdx.x] = NAN;      // no joint workgroup: no similarity either
        return;
    }
    // ---- joint j: part 0's similarity, the votes' medians, then camera space through part 0's pose
    const int j = blockIdx.y;
    ANCSH_PART_SIMILARITY(n, K, G, 0, p0, gocs, nocs, mask, red, sst)
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    int cnt = 0;
    ANCSH_COMPACT_JOINT_VOTES(n, K, G, p0, npow2, gocs, mask, heatmap, unitvec, axis, argmax_first_nan(joint_index + (p0 + i) * JC, JC) == j,
                              art_vals, wcnt, lane, wave, cnt)
    __syncthreads();
    ANCSH_SORT_VOTE_COLUMNS(art_vals, npow2, cnt)          // ends on a barrier: sst is visible too
    __shared__ double smed[6];
    if (threadIdx.x < 6) {
        ANCSH_VOTE_MEDIAN(med, art_vals, npow2, cnt, p2, threadIdx.x)
        smed[threadIdx.x] = med;                           // 0..2 axis, 3..5 pivot
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s2 = sst[0];
        const double *r = rec + 13, s0 = r[9], *t0 = r + 10;     // part 0's nonlinear pose
        double pp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) pp[k] = s0 * (smed[3 + k] * s2 + sst[1 + k]);
        double *o = ab + j * 12;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *rk = r + 3 * k;
            o[6 + k] = poisoned ? NAN : ((pp[0] * rk[0] + pp[1] * rk[1]) + pp[2] * rk[2]) + t0[k];
            o[9 + k] = poisoned ? NAN : (smed[0] * rk[0] + smed[1] * rk[1]) + smed[2] * rk[2];
        }
        if (joint_nocs) {
            double *q = joint_nocs + ((size_t)b * (K - 1) + (j - 1)) * 6;
#pragma unroll
            for (int k = 0; k < 3; ++k) { q[k] = smed[3 + k]; q[3 + k] = smed[k]; }
        }
        if (st0 && j == 1)
#pragma unroll
            for (int k = 0; k < 4; ++k) st0[(size_t)b * 4 + k] = sst[k];
    }
}

}  // namespace ancsh

extern "C" int ancsh_part_extents(int b, int n, int K, int nocs_channels, const float *nocs, const float *mask, const float *P, int ldp,
                                  const double *pose0, float *scale_pred, double *dynam, int *count, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1 && K <= 8 && ldp >= 3, "part_extents: bad sizes b=%d n=%d K=%d ldp=%d", b, n, K, ldp);
    ANCSH_REQUIRE(nocs_channels == 3 || nocs_channels == 3 * K, "part_extents: nocs must have 3 or 3K = %d channels, got %d", 3 * K, nocs_channels);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(nocs && mask && P && pose0 && scale_pred && dynam && count, "part_extents: null pointer");
    hipLaunchKernelGGL(part_extents_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, n, K, nocs_channels, nocs, mask, P, ldp, pose0,
                       scale_pred, dynam, count);
    return check_launch("part_extents");
}

extern "C" int ancsh_joint_params(int b, int n, int K, int gocs_channels, int axis_mean, const float *gocs, const float *nocs,
                                  const float *mask, const float *heatmap, const float *unitvec, const float *joint_axis,
                                  const int *joint_cls, double *st, double *joint, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1 && K <= 8, "joint_params: bad sizes b=%d n=%d K=%d", b, n, K);
    ANCSH_REQUIRE(gocs_channels == 3 || gocs_channels == 3 * K, "joint_params: gocs must have 3 or 3K = %d channels, got %d", 3 * K, gocs_channels);
    ANCSH_REQUIRE(gocs_channels == 3 || mask, "joint_params: per-part global NOCS (3K channels) needs the part mask");
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(gocs && heatmap && unitvec && joint_axis && joint_cls && (joint || K == 1), "joint_params: null pointer");      // K == 1: no joint rows
    ANCSH_REQUIRE(!nocs == !st, "joint_params: nocs and st go together (both or neither)");
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    const size_t lds = (size_t)6 * npow2 * sizeof(float);
    ANCSH_REQUIRE(lds <= 144 * 1024, "joint_params: n %d too large for the LDS-resident medians", n);
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)joint_params_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(joint_params_kernel, dim3(b, K + K - 1), dim3(256), lds, (hipStream_t)stream, n, K, gocs_channels, axis_mean ? 1 : 0,
                       gocs, nocs, mask, heatmap, unitvec, joint_axis, joint_cls, st, joint);
    return check_launch("joint_params");
}

extern "C" int ancsh_articulation_rec(int b, int n, int K, int gocs_channels, int joint_channels, const float *gocs, const float *nocs,
                                      const float *mask, const float *heatmap, const float *unitvec, const float *joint_axis,
                                      const float *joint_index, const float *npcs_nocs, const float *npcs_mask, const double *record,
                                      double *art, double *joint_nocs, double *st0, float *extent, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1 && K <= 8, "articulation_rec: bad sizes b=%d n=%d K=%d (K <= 8)", b, n, K);
    ANCSH_REQUIRE(gocs_channels == 3 || gocs_channels == 3 * K, "articulation_rec: gocs must have 3 or 3K = %d channels, got %d", 3 * K,
                  gocs_channels);
    ANCSH_REQUIRE(joint_channels >= 1 && joint_channels <= 8, "articulation_rec: joint_channels %d (1..8)", joint_channels);
    ANCSH_REQUIRE(n <= ANCSH_ARTICULATION_MAX_N, "articulation_rec: n %d too large for the LDS-resident medians (<= %d)", n,
                  ANCSH_ARTICULATION_MAX_N);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(gocs && nocs && mask && heatmap && unitvec && joint_axis && joint_index && npcs_nocs && npcs_mask && record && art,
                  "articulation_rec: null pointer");
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    const size_t lds = K > 1 ? (size_t)6 * npow2 * sizeof(float) : 0;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)articulation_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(articulation_kernel, dim3(b, K), dim3(256), lds, (hipStream_t)stream, n, K, gocs_channels, joint_channels, gocs, nocs,
                       mask, heatmap, unitvec, joint_axis, joint_index, npcs_nocs, npcs_mask, record, art, joint_nocs, st0, extent);
    return check_launch("articulation_rec");
}
