// gt_errors.hip -- how far the poses of a pose record are from a known answer: per (cloud, part) and for the baseline pose (record columns
// 0..12) and the nonlinear pose (13..25) the evaluation's rpy_err, xyz_err and scale_err (evaluation/parallel_ancsh_pose.py, the end of
// solver_ransac_nonlinear), the 3-D IoU of the amodal boxes (compute_miou.py:150-229) and the relative rotation error of the joint
// (eval_pose_err.py:304-312, 327); for the nonlinear pose also the relative translation error (:316-326).  One launch behind the fit; it
// carries the record (or the fit-quality wide record) along in columns 0..ld-1 of its (b, K, ld + 12) block.
//
// The IoU is the work: b * K * 2 box pairs, nres^3 grid points each, float64.  ONE WORKGROUP OF 1024 THREADS PER (cloud, part, pose): at
// 32 x 3 that is 192 workgroups of 16 waves (four per SIMD) on 256 CUs, four times the waves iou_3d_kernel puts behind a pair.  A pair
// is not split over workgroups: its two counts would have to meet in memory the ABI does not have (the output is the only buffer, and no
// workgroup may wait for another), while four waves per SIMD already hide the f64 pipe's latency.  Inside a workgroup a thread owns
// (ix, iy) COLUMNS of the grid and walks iz: the part of the three projections that does not depend on z -- (ux * u[0] + uy * u[1]) of
// `inside`, the first two terms of a sum that is evaluated left to right -- is computed once per column and box instead of once per
// point, which halves the f64 operations of a point (about 30 instead of 57) and keeps every inside test bit for bit the one of
// iou_3d_kernel (iou_grid.h: same expressions, same order, no contraction).  Counts are integers, reduced by butterfly shuffles and
// through LDS: the same bytes every run and wherever the cloud lies in the batch.
//
// Every workgroup recomputes what it needs: waves 0..3 make the one pass over the cloud's n points that gives every part's extent, point
// count and boundary (part_stats.h, ANCSH_PART_EXTENTS_PASS fed the float32-rounded nonlinear part-0 pose by ANCSH_POSE0_FIRST_COLUMN:
// the statements of ancsh_part_extents and ancsh_joint_state_rec, so scale_pred, dynam and count are bit-equal to theirs), sixteen
// threads build the sixteen corners, everybody counts, thread 0 does the 3 x 3 arithmetic in float64 as written (-ffp-contract=off).
// No atomics, nothing allocated, every size an argument: capturable.
#include "iou_grid.h"
#include "part_stats.h"

namespace ancsh {

constexpr int GE_THREADS = 1024;
constexpr int GE_WAVES = GE_THREADS / 64;
constexpr int GE_WIDTH = 12;
constexpr int GE_GT = 19;

// rot_diff_degree (lib/d3_utils.py:144-148) of two row-major 3 x 3 matrices: tr(A B^T) = sum_ac A_ac B_ac, row by row, each row's three
// products added left to right; arccos((tr - 1) / 2) mod 2 pi, / pi * 180.  No clamp, like the reference: a trace above 3 gives NaN.
__device__ __forceinline__ double ge_rot_diff_degree(const double *A, const double *B) {
#pragma clang fp contract(off)
    constexpr double PI = 3.14159265358979323846;
    const double d0 = (A[0] * B[0] + A[1] * B[1]) + A[2] * B[2];
    const double d1 = (A[3] * B[3] + A[4] * B[4]) + A[5] * B[5];
    const double d2 = (A[6] * B[6] + A[7] * B[7]) + A[8] * B[8];
    const double tr = (d0 + d1) + d2;
    return fmod(acos((tr - 1.0) / 2.0), 2.0 * PI) / PI * 180.0;
}

// out = A^T B of two row-major 3 x 3 matrices: out[a][c] = (A[0][a] B[0][c] + A[1][a] B[1][c]) + A[2][a] B[2][c] (joint_state_kernel's Rrel)
__device__ __forceinline__ void ge_relative(const double *A, const double *B, double *out) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * a + c] = (A[a] * B[c] + A[3 + a] * B[3 + c]) + A[6 + a] * B[6 + c];
}

__global__ __launch_bounds__(GE_THREADS) void gt_error_kernel(int n, int K, int nres, const float *__restrict__ P, int ldp,
                                                              const float *__restrict__ npcs_nocs, const float *__restrict__ npcs_mask,
                                                              const double *__restrict__ record, int ld, const double *__restrict__ gt,
                                                              double *__restrict__ wide) {
#pragma clang fp contract(off)
    constexpr int KM = 8;
    __shared__ float smax[4][KM][3];
    __shared__ double smin[4][KM];
    __shared__ int scnt[4][KM];
    __shared__ double cor[2][8][3];            // the corners of the ground-truth box (0) and of the predicted box (1), reference's order
    __shared__ int red[2][GE_WAVES];
    const int q = blockIdx.x & 1, p = blockIdx.x >> 1, c = p / K, j = p - c * K;       // pose q of part j of cloud c
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t p0 = (size_t)c * n;
    const double *rec0 = record + (size_t)c * K * ld, *rec = rec0 + (size_t)j * ld;
    const double *g0 = gt + (size_t)c * K * GE_GT, *g = g0 + j * GE_GT;
    double *o = wide + (size_t)p * (ld + GE_WIDTH);
    // columns 0..ld-1: the input row, moved as 64-bit words so that a NaN keeps its payload (the baseline pose's workgroup does it)
    if (q == 0 && tid < ld) reinterpret_cast<unsigned long long *>(o)[tid] = reinterpret_cast<const unsigned long long *>(rec)[tid];
    // ---- the part pass (waves 0..3): extents, counts and the boundary in the nonlinear part-0 frame, as ancsh_joint_state_rec makes them
    if (tid < 256) {
        const double *R0n = rec0 + 13, *T0n = rec0 + 23;
        ANCSH_POSE0_FIRST_COLUMN(R0n, T0n, r00, r10, r20, t00, t01, t02, m30)
        ANCSH_PART_EXTENTS_PASS(true, n, K, 3 * K, p0, npcs_nocs, npcs_mask, P, ldp, r00, r10, r20, m30, smax, smin, scnt, lane, wave)
    }
    __syncthreads();
    const int cnt = scnt[0][j] + scnt[1][j] + scnt[2][j] + scnt[3][j];
    float sp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        sp[k] = cnt > 0 ? 2.0f * np_maxf(np_maxf(smax[0][j][k], smax[1][j][k]), np_maxf(smax[2][j][k], smax[3][j][k])) : NAN;
    const double *m = rec + 13 * q, *m0 = rec0 + 13 * q;        // pose q of part j and of part 0: R (9, row-major) | s | t (3)
    bool dead = false, dead0 = false, gbox = false;             // a NaN in the pose, in part 0's, in the ground truth the box reads
#pragma unroll
    for (int e = 0; e < 13; ++e) {
        dead |= m[e] != m[e];
        dead0 |= m0[e] != m0[e];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) gbox |= g[e] != g[e];
    const bool box = !dead && !gbox && cnt > 0;                 // uniform over the workgroup
    // ---- the sixteen corners: get_3d_bbox(extent, shift = 1/2) * s, through . R^T + t; the predicted R and t rounded to float32 first
    if (tid < 16 && box) {
        const int which = tid >> 3, k = tid & 7;
        const double sg[3] = {(k & 2) ? -1.0 : 1.0, (k & 4) ? -1.0 : 1.0, (k & 1) ? -1.0 : 1.0};
        double R[9], t[3], bb[3];
        const double s = which ? m[9] : g[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = which ? (double)(float)m[e] : g[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            t[e] = which ? (double)(float)m[10 + e] : g[10 + e];
            const double ext = which ? (double)sp[e] : g[13 + e];
            bb[e] = (sg[e] * (ext / 2.0) + 0.5) * s;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) cor[which][k][e] = ((R[3 * e] * bb[0] + R[3 * e + 1] * bb[1]) + R[3 * e + 2] * bb[2]) + t[e];
    }
    __syncthreads();
    // ---- the grid: iou_3d_kernel's bounds, coordinates and inside tests; a thread owns columns (ix, iy) and walks iz
    int both = 0, either = 0;
    if (box) {
        const double *b1 = &cor[0][0][0], *b2 = &cor[1][0][0];
        BoxFrame f1, f2;
        box_frame(b1, f1);
        box_frame(b2, f2);
        double lo[3], hi[3], step[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double mn = b1[a], mx = b1[a];
            for (int k = 0; k < 8; ++k) {
                mn = fmin(mn, fmin(b1[k * 3 + a], b2[k * 3 + a]));
                mx = fmax(mx, fmax(b1[k * 3 + a], b2[k * 3 + a]));
            }
            lo[a] = mn; hi[a] = mx;
            step[a] = (mx - mn) / (double)(nres - 1);          // numpy.linspace: step = delta / div
        }
        const int columns = nres * nres;
        for (int col = tid; col < columns; col += GE_THREADS) {
            const int ix = col / nres, iy = col - ix * nres;
            // linspace: y = arange(num) * step + start, then y[-1] = stop
            const double x = ix == nres - 1 ? hi[0] : (double)ix * step[0] + lo[0];
            const double y = iy == nres - 1 ? hi[1] : (double)iy * step[1] + lo[1];
            // the z-free part of `inside`'s projections: (ux * u[0] + uy * u[1]), to which uz * u[2] is added last
            const double ux1 = x - f1.o[0], uy1 = y - f1.o[1], ux2 = x - f2.o[0], uy2 = y - f2.o[1];
            const double a11 = ux1 * f1.u1[0] + uy1 * f1.u1[1], a12 = ux1 * f1.u2[0] + uy1 * f1.u2[1], a13 = ux1 * f1.u3[0] + uy1 * f1.u3[1];
            const double a21 = ux2 * f2.u1[0] + uy2 * f2.u1[1], a22 = ux2 * f2.u2[0] + uy2 * f2.u2[1], a23 = ux2 * f2.u3[0] + uy2 * f2.u3[1];
            for (int iz = 0; iz < nres; ++iz) {
                const double z = iz == nres - 1 ? hi[2] : (double)iz * step[2] + lo[2];
                const double uz1 = z - f1.o[2], uz2 = z - f2.o[2];
                const double p11 = a11 + uz1 * f1.u1[2], p12 = a12 + uz1 * f1.u2[2], p13 = a13 + uz1 * f1.u3[2];
                const double p21 = a21 + uz2 * f2.u1[2], p22 = a22 + uz2 * f2.u2[2], p23 = a23 + uz2 * f2.u3[2];
                const bool i1 = (p11 > 0.0) & (p11 < f1.d1) & (p12 > 0.0) & (p12 < f1.d2) & (p13 > 0.0) & (p13 < f1.d3);
                const bool i2 = (p21 > 0.0) & (p21 < f2.d1) & (p22 > 0.0) & (p22 < f2.d2) & (p23 > 0.0) & (p23 < f2.d3);
                both += (i1 & i2) ? 1 : 0;
                either += (i1 | i2) ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { both += __shfl_xor(both, d, 64); either += __shfl_xor(either, d, 64); }
    if (lane == 0) { red[0][wave] = both; red[1][wave] = either; }
    __syncthreads();
    if (tid != 0) return;
    // ---- thread 0: this pose's columns
    double *e = o + ld + 5 * q;
    int I = 0, U = 0;
    for (int w = 0; w < GE_WAVES; ++w) { I += red[0][w]; U += red[1][w]; }
    const double dx = m[10] - g[10], dy = m[11] - g[11], dz = m[12] - g[12];
    e[0] = dead ? NAN : ge_rot_diff_degree(m, g);
    e[1] = dead ? NAN : sqrt((dx * dx + dy * dy) + dz * dz);
    e[2] = dead ? NAN : fabs(m[9] - g[9]);
    e[3] = !box ? NAN : (U == 0 ? 1.0 : (double)I / (double)U);
    const bool rel = j > 0 && !dead && !dead0;
    double rg[9], rp[9];
    if (rel) {
        ge_relative(g0, g, rg);
        ge_relative(m0, m, rp);
    }
    e[4] = rel ? ge_rot_diff_degree(rg, rp) : NAN;
    if (q == 0) {
        o[ld + 11] = (double)cnt;
        return;
    }
    // ---- the nonlinear pose's relative translation error: the boundary slide dynam_j - canon_j (ancsh_joint_state_rec's column 18) along
    // part 0's x axis against the NAOCS ground truth's t_j - t_0
    const double dynam = cnt > 0 ? np_min(np_min(smin[0][j], smin[1][j]), np_min(smin[2][j], smin[3][j])) : NAN;
    const float canon = -sp[0] / 2.0f + 0.5f;                  // float32, like - scale_pred[0] / 2 + 0.5
    const double d = dynam - (double)canon;
    const double e0 = (g[16] - g0[16]) - d * m0[0], e1 = (g[17] - g0[17]) - d * m0[3], e2 = (g[18] - g0[18]) - d * m0[6];
    o[ld + 10] = rel ? sqrt((e0 * e0 + e1 * e1) + e2 * e2) : NAN;
}

}  // namespace ancsh

extern "C" int ancsh_gt_error_rec(int b, int n, int K, int nres, const float *P, int ldp, const float *npcs_nocs, const float *npcs_mask,
                                  const double *record, int ld, const double *gt, double *wide, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0, "gt_error_rec: b=%d (>= 0)", b);
    ANCSH_REQUIRE(K >= 1 && K <= 8, "gt_error_rec: K=%d (1..8)", K);
    ANCSH_REQUIRE(n >= 1, "gt_error_rec: n=%d (>= 1)", n);
    ANCSH_REQUIRE(ldp >= 3, "gt_error_rec: ldp=%d (>= 3: a row of P starts with the point)", ldp);
    ANCSH_REQUIRE(ld == 26 || ld == 39, "gt_error_rec: ld=%d (26: the record, 39: the fit-quality wide record)", ld);
    ANCSH_REQUIRE(nres >= 2 && nres <= 64, "gt_error_rec: nres=%d (2..64)", nres);
    ANCSH_REQUIRE((long)b * K <= 0x7fffffffL / (2 * (39 + GE_WIDTH)), "gt_error_rec: b * K = %ld rows overflow an int", (long)b * K);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(P && npcs_nocs && npcs_mask && record && gt && wide, "gt_error_rec: null pointer");
    hipLaunchKernelGGL(gt_error_kernel, dim3(b * K * 2), dim3(GE_THREADS), 0, (hipStream_t)stream, n, K, nres, P, ldp, npcs_nocs, npcs_mask,
                       record, ld, gt, wide);
    return check_launch("gt_error_rec");
}
