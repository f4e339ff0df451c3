// umeyama_fit.h -- estimateSimilarityUmeyama (lib/aligning.py:580-622) for one (source, target) point set per workgroup of 256 threads,
// float64, stated ONCE for umeyama_kernel (pose_glue.hip, behind ancsh_umeyama) and gt_pose_kernel (gt_pose.hip, behind ancsh_gt_pose_build),
// with the block reductions both use.  The passes are STATEMENT MACROS (as csrc/part_stats.h and ANCSH_JD_COMPACT): expanded in place
// they give umeyama_kernel the statements it had before the second kernel, and the second kernel the same statements in the same order
// -- thread t takes rows t, t + 256, ..., block_sum<6> then block_sum<10>, horn_quat / quat_to_mat on one lane -- so both write the
// same bits for the same rows.  Each macro names every variable it reads or declares.
#pragma once
#include "common.h"
#include "pose_math.h"

namespace ancsh {
namespace pose {

// ---- block reductions (256 threads = 4 waves) -----------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sums K doubles across the workgroup; every thread receives every total.  red: LDS, >= K*nwaves doubles.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *red, int nwaves) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < K; ++i) red[wave * K + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double s = 0.0;
        for (int w = 0; w < nwaves; ++w) s += red[w * K + i];
        v[i] = s;
    }
}

}  // namespace pose
}  // namespace ancsh

// ANCSH_UMEYAMA_SUMS: every thread of the workgroup.  n (int, > 0) rows; SRC(i, c) / TGT(i, c): coordinate c of source / target row i
// (function-like macros or functions, float); red: >= 40 doubles of LDS.  Declares sums[6], sm[3], tm[3] (the means) and acc[10]
// (Cov * n, row-major target x source, then sum |s - sm|^2), the same on every thread.
#define ANCSH_UMEYAMA_SUMS(n, SRC, TGT, red)                                                                                          \
    double sums[6] = {0, 0, 0, 0, 0, 0};                                                                                              \
    for (int i = threadIdx.x; i < n; i += 256)                                                                                        \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) { sums[c] += SRC(i, c); sums[3 + c] += TGT(i, c); }                             \
    block_sum<6>(sums, red, 4);                                                                                                       \
    double sm[3], tm[3];                                                                                                              \
    _Pragma("unroll") for (int c = 0; c < 3; ++c) { sm[c] = sums[c] / n; tm[c] = sums[3 + c] / n; }                                   \
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   /* Cov*n (9) + sum |s - sm|^2 */                                               \
    for (int i = threadIdx.x; i < n; i += 256) {                                                                                      \
        double sc[3], tc[3];                                                                                                          \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) { sc[c] = SRC(i, c) - sm[c]; tc[c] = TGT(i, c) - tm[c]; }                       \
        _Pragma("unroll") for (int a = 0; a < 3; ++a)                                                                                 \
            _Pragma("unroll") for (int b = 0; b < 3; ++b) acc[a * 3 + b] += tc[a] * sc[b];                                            \
        acc[9] += sc[0] * sc[0] + sc[1] * sc[1] + sc[2] * sc[2];                                                                      \
    }                                                                                                                                 \
    block_sum<10>(acc, red, 4);

// ANCSH_UMEYAMA_SOLVE: one lane, behind ANCSH_UMEYAMA_SUMS in the same scope: the whole tail of umeyama_kernel, its 32 output doubles
// included -- o[0..2] Scales, o[3..11] Rotation (the TRANSPOSE of the src -> tgt rotation R = U diag(1,1,d) Vh), o[12..14] Translation,
// o[15..30] OutTransform, o[31] 0.  pose_math.h lets the compiler contract this float64 arithmetic, and which multiply-adds it fuses
// depends on every use of a value: a kernel that wants umeyama_kernel's bits expands the same statements with the same uses and reads
// what it needs back from o (gt_pose_kernel hands it 32 doubles of LDS).
#define ANCSH_UMEYAMA_SOLVE(n, o)                                                                                                     \
    double M[9], q[4], R[9];                                                                                                          \
    _Pragma("unroll") for (int a = 0; a < 9; ++a) M[a] = acc[a] / n;                                                                  \
    horn_quat(M, q);                                                                                                                  \
    quat_to_mat(q, R);                       /* R = U diag(1,1,d) Vh */                                                               \
    /* sum of the (sign-corrected) singular values = tr(R^T Cov) */                                                                   \
    double trace = 0.0;                                                                                                               \
    _Pragma("unroll") for (int a = 0; a < 3; ++a)                                                                                     \
        _Pragma("unroll") for (int b = 0; b < 3; ++b) trace += R[a * 3 + b] * M[a * 3 + b];                                           \
    const double varP = acc[9] / n;                                                                                                   \
    const double s = trace / varP;                                                                                                    \
    o[0] = o[1] = o[2] = s;                                                                                                           \
    /* Rotation = (U Vh)^T ; Translation = tmean - smean . (s * Rotation) = tmean - s * R smean */                                    \
    _Pragma("unroll") for (int a = 0; a < 3; ++a)                                                                                     \
        _Pragma("unroll") for (int b = 0; b < 3; ++b) o[3 + a * 3 + b] = R[b * 3 + a];                                                \
    double T[3];                                                                                                                      \
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                                                                   \
        T[a] = tm[a] - s * (R[a * 3] * sm[0] + R[a * 3 + 1] * sm[1] + R[a * 3 + 2] * sm[2]);                                          \
        o[12 + a] = T[a];                                                                                                             \
    }                                                                                                                                 \
    /* OutTransform = [[s*R, T],[0,0,0,1]] row-major 4x4 */                                                                           \
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {                                                                                   \
        _Pragma("unroll") for (int b = 0; b < 3; ++b) o[15 + a * 4 + b] = s * R[a * 3 + b];                                           \
        o[15 + a * 4 + 3] = T[a];                                                                                                     \
    }                                                                                                                                 \
    o[27] = 0; o[28] = 0; o[29] = 0; o[30] = 1; o[31] = 0;
