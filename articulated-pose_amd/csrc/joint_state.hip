// joint_state.hip -- the joint states of a streamed batch (pred side of evaluation/eval_pose_err.py:253-268, 304-321): per cloud and
// child part j the relative rotation R_0^T R_j as an angle (unsigned, and signed about the joint axis), the relative translation t_j - t_0,
// its slide along the joint axis, and the boundary slide dynam_j - canon_j; one launch behind ancsh_articulation_rec, whose (b, K, 12) block
// it carries along in columns 0..11 of its own (b, K, 20) block.
//
// One workgroup of 256 threads per cloud.  The per-point part is ancsh_part_extents' pass (part_stats.h, ANCSH_PART_EXTENTS_PASS with the
// boundary on, fed the float32-rounded part-0 pose by ANCSH_POSE0_FIRST_COLUMN): the same statements, so dynam, scale_pred and count are
// bit-equal to that kernel's.  It reads the NPCS mask, the point and the point's own NOCS slot once; each wave reduces its parts' extents
// by butterfly shuffles and leaves one partial per part in LDS, and after ONE barrier thread j < K combines the four partials and does part
// j's 3x3 arithmetic in float64 (-ffp-contract=off: the sums below are evaluated as written, left to right).  No atomics, nothing
// allocated, every size an argument: capturable, and the same bytes every run.
#include "part_stats.h"

namespace ancsh {

__global__ __launch_bounds__(256) void joint_state_kernel(int n, int K, const float *__restrict__ P, int ldp, const float *__restrict__ npcs_nocs,
                                                          const float *__restrict__ npcs_mask, const double *__restrict__ record,
                                                          const double *__restrict__ art, double *__restrict__ wide) {
    constexpr int KM = 8;
    constexpr double DEG = 180.0 / 3.14159265358979323846;
    __shared__ float smax[4][KM][3];
    __shared__ double smin[4][KM];
    __shared__ int scnt[4][KM];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p0 = (size_t)b * n;
    const double *rec = record + (size_t)b * K * 26;
    const double *R0 = rec + 13, *T0 = rec + 23;                // part 0's nonlinear R (row-major) and t
    // columns 0..11: the articulation block, moved as 64-bit words so that a NaN keeps its payload
    const unsigned long long *ab = reinterpret_cast<const unsigned long long *>(art + (size_t)b * K * 12);
    unsigned long long *wb = reinterpret_cast<unsigned long long *>(wide + (size_t)b * K * 20);
    for (int e = threadIdx.x; e < K * 12; e += 256) wb[(e / 12) * 20 + e % 12] = ab[e];
    ANCSH_POSE0_FIRST_COLUMN(R0, T0, r00, r10, r20, t00, t01, t02, m30)
    ANCSH_PART_EXTENTS_PASS(true, n, K, 3 * K, p0, npcs_nocs, npcs_mask, P, ldp, r00, r10, r20, m30, smax, smin, scnt, lane, wave)
    __syncthreads();
    if ((int)threadIdx.x >= K) return;
    const int j = threadIdx.x;
    double *o = wide + ((size_t)b * K + j) * 20;
    const double *rj = rec + j * 26 + 13, *tj = rj + 10;
    bool dead = false;                                         // a NaN in part 0's nonlinear pose or in part j's own
    for (int c = 0; c < 13; ++c) dead |= R0[c] != R0[c] || rj[c] != rj[c];
    // ---- column 19, and 18: the boundary slide dynam_j - canon_j (eval_pose_err.py:263-266, 320), for row 0 too
    const int cnt = scnt[0][j] + scnt[1][j] + scnt[2][j] + scnt[3][j];
    const float sp0 = cnt > 0 ? 2.0f * np_maxf(np_maxf(smax[0][j][0], smax[1][j][0]), np_maxf(smax[2][j][0], smax[3][j][0])) : NAN;
    const double dynam = cnt > 0 ? np_min(np_min(smin[0][j], smin[1][j]), np_min(smin[2][j], smin[3][j])) : NAN;
    const float canon = -sp0 / 2.0f + 0.5f;                    // float32, like - scale_pred[0] / 2 + 0.5
    o[18] = dead ? NAN : dynam - (double)canon;
    o[19] = (double)cnt;
    if (j == 0 || dead) {
#pragma unroll
        for (int c = 12; c < 18; ++c) o[c] = NAN;
        return;
    }
    // ---- Rrel = R_0^T R_j, its trace part c and its antisymmetric part v (the rotation axis times the sine)
    double rr[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) rr[a][c] = (R0[a] * rj[c] + R0[3 + a] * rj[3 + c]) + R0[6 + a] * rj[6 + c];
    const double cs = (((rr[0][0] + rr[1][1]) + rr[2][2]) - 1.0) / 2.0;
    const double v[3] = {0.5 * (rr[2][1] - rr[1][2]), 0.5 * (rr[0][2] - rr[2][0]), 0.5 * (rr[1][0] - rr[0][1])};
    o[12] = atan2(sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), cs) * DEG;
    // ---- the joint axis in camera space, u, and in part 0's frame, R_0^T u (NaN / zero axis: NaN from here on)
    const double *ax = art + ((size_t)b * K + j) * 12 + 9;
    const double len = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
    const double u[3] = {ax[0] / len, ax[1] / len, ax[2] / len};
    double va = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) va += v[a] * ((R0[a] * u[0] + R0[3 + a] * u[1]) + R0[6 + a] * u[2]);
    o[13] = atan2(va, cs) * DEG;
    // ---- t_j - t_0 (eval_pose_err.py:318) and its part along the axis
    const double d[3] = {tj[0] - T0[0], tj[1] - T0[1], tj[2] - T0[2]};
    o[14] = d[0]; o[15] = d[1]; o[16] = d[2];
    o[17] = (d[0] * u[0] + d[1] * u[1]) + d[2] * u[2];
}

}  // namespace ancsh

extern "C" int ancsh_joint_state_rec(int b, int n, int K, const float *P, int ldp, const float *npcs_nocs, const float *npcs_mask,
                                     const double *record, const double *art, double *wide, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0, "joint_state_rec: b=%d (>= 0)", b);
    ANCSH_REQUIRE(K >= 1 && K <= 8, "joint_state_rec: K=%d (1..8)", K);
    ANCSH_REQUIRE(n >= 1, "joint_state_rec: n=%d (>= 1)", n);
    ANCSH_REQUIRE(ldp >= 3, "joint_state_rec: ldp=%d (>= 3: a row of P starts with the point)", ldp);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(P && npcs_nocs && npcs_mask && record && art && wide, "joint_state_rec: null pointer");
    hipLaunchKernelGGL(joint_state_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, n, K, P, ldp, npcs_nocs, npcs_mask, record, art, wide);
    return check_launch("joint_state_rec");
}
