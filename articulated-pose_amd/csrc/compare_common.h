// compare_common.h -- what render-and-compare's files (reprojection.hip scores a pose record, refinement.hip acts on it, joint_values.hip reads
// the joint values off it) share: which pixel belongs to which part, when a pose counts, the predicted map of a link under a pose, the short
// formulas they spell -- each in the parenthesisation and operand order its callers had (float64 is evaluated as written and the Python mirrors
// follow it operation by operation) -- and the C entries' argument checks.
#pragma once
#include "depth_annotate_common.h"

namespace ancsh {

__device__ __forceinline__ bool finite(double v) { return fabs(v) < __builtin_inf(); }         // NaN fails the comparison
// a pose of the record, 13 values [R (9) | s | t (3)]: usable when every value is finite
__device__ __forceinline__ bool pose_ok(const double *__restrict__ p) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 13; ++k) ok = ok && finite(p[k]);
    return ok;
}

// the part of link l of a scene of nl links and K parts, or -1: the link is not used or its part lies outside [0, K)
__device__ __forceinline__ int scene_link_part(const double *__restrict__ sc, int l, int nl, int K) {
    const double pv = sc[AN_HEAD + AN_LINK * l + 1];
    return scene_rank(sc, l, nl) >= 0 && pv >= 0.0 && pv < (double)K ? (int)pv : -1;
}
// thread tid < 16 fills its link's entry of the block's link-to-part table; the caller syncs before it reads
__device__ __forceinline__ void scene_part_table(const double *__restrict__ sc, int K, int tid, int *s_part) {
    if (tid < AN_LINKS) s_part[tid] = scene_link_part(sc, tid, scene_nlinks(sc), K);
}
// the part of a pixel, or -1: its label names a used link (s_part: scene_part_table's) and its depth passes depth_ok
template <typename T>
__device__ __forceinline__ int pixel_part(T d, unsigned char lab, const int *s_part) {
    return lab < AN_LINKS && depth_ok(d) ? s_part[lab] : -1;
}

// the centre a step turns a pose about: s R (0.5, 0.5, 0.5) + t
__device__ __forceinline__ void pose_centre(const double *__restrict__ pose, double *c) {
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = pose[9] * ((pose[3 * a] * 0.5 + pose[3 * a + 1] * 0.5) + pose[3 * a + 2] * 0.5) + pose[10 + a];
}
// the ray of pixel (row, col) through the scene's camera: a point at depth z is (z su, z sv, z)
__device__ __forceinline__ void pixel_ray(const double *__restrict__ sc, double row, double col, double &su, double &sv) {
    su = (sc[7] * col + sc[8] * row) + sc[9];
    sv = (sc[10] * col + sc[11] * row) + sc[12];
}

// C = A o B of 3 x 4 maps, row-major, in ancsh_pose_scene_build's written order
__device__ __forceinline__ void rp_compose(const double *A, const double *B, double *C) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
            C[4 * i + j] = j == 3 ? v + A[4 * i + 3] : v;
        }
    }
}
// the predicted map of link l of part j under a 13-value pose, steps 1..5 of ancsh_reproject_scene_build (include/ancsh_hip.h): rt, sc, rg =
// the frame's render table, scene table and rig row; R = the 12 values written.  The caller has checked l, j, the pose and nf.
__device__ __forceinline__ void predicted_link_map(const double *__restrict__ rt, const double *__restrict__ sc, const double *__restrict__ rg,
                                                   int K, int l, int j, const double *__restrict__ pose, double nf, double *R) {
    const double *L = sc + AN_HEAD + AN_LINK * l;
    double Rl[12], M[12], N[12], Q[12], P[12], T1[12], T2[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rl[k] = rt[ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * l + k], M[k] = L[2 + k];
    rp_compose(M, Rl, N);                                               // 1. model -> canonical coordinates
    const double *pt = rg + ANCSH_RIG_HEAD + j * ANCSH_RIG_PART(K);
    double o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = ((((0.0 - pt[a]) - pt[3 + a]) * pt[6 + a]) + 0.5) - pt[9 + a];        // nocs_p of c = 0
    if (rg[3] != 0.0) {                                                 // 2. canonical -> part NOCS, with the sapien rotation
        const double *Rr = rg + ANCSH_RIG_ROT;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Q[4 * a + k] = Rr[3 * a + k] * pt[6 + k];
            Q[4 * a + 3] = ((Rr[3 * a] * (o[0] - 0.5) + Rr[3 * a + 1] * (o[1] - 0.5)) + Rr[3 * a + 2] * (o[2] - 0.5)) + 0.5;
        }
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int k = 0; k < 3; ++k) Q[4 * a + k] = a == k ? pt[6 + k] : 0.0;
            Q[4 * a + 3] = o[a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {                                       // 3. part NOCS -> the scaled cloud: [s R | t]
#pragma unroll
        for (int k = 0; k < 3; ++k) P[4 * a + k] = pose[9] * pose[3 * a + k];
        P[4 * a + 3] = pose[10 + a];
    }
    rp_compose(Q, N, T1);
    rp_compose(P, T1, T2);
#pragma unroll
    for (int a = 0; a < 3; ++a)                                         // 4. / norm factor, 5. (x, y, z) -> (x', y', z) = (x, -y, z)
#pragma unroll
        for (int k = 0; k < 4; ++k) R[4 * a + k] = a == 1 ? -(T2[4 * a + k] / nf) : T2[4 * a + k] / nf;
}

// ---- the entries' argument checks: each sets the error and returns false; an entry calls them through ANCSH_CHECK, who = its name
#define ANCSH_ALIGNED "%s: a pointer is not aligned: the depth buffers to their element, 4-byte values 4-byte, 8-byte values 8-byte aligned"
#define ANCSH_CHECK(ok) do { if (!(ok)) return ANCSH_EINVAL; } while (0)
template <typename... A>
inline bool refuse(const char *fmt, A... a) { return set_error(fmt, a...), false; }
// the batch: 0 <= nframes <= 32767 (why = what the bound protects, in the entry's words) and 1 <= K <= 8
inline bool batch_ok(const char *who, int nframes, int K, const char *why) {
    if (nframes < 0) return refuse("%s: bad shape nframes=%d", who, nframes);
    if (nframes > 32767) return refuse("%s: %d frames %s; split the batch", who, nframes, why);
    return (K >= 1 && K <= 8) || refuse("%s: K=%d must be in [1, 8]", who, K);
}
inline bool depth_item(const char *who, int depth_type, size_t &item) {      // item = the size of a depth value in bytes
    item = depth_type == ANCSH_DEPTH_U16 ? 2 : 4;
    return depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32 ||
           refuse("%s: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", who, depth_type);
}
inline bool capacity_ok(const char *who, long n) { return (n >= 0 && n < (1L << 29)) || refuse("%s: pixel_capacity=%ld pixels out of range", who, n); }
inline bool record_ld_ok(const char *who, const char *name, int ld) {
    return ld >= 26 || refuse("%s: %s=%d, a record row holds at least the 26 pose columns", who, name, ld);
}
inline bool pass_ok(const char *who, int pass, int is_last) {
    if (pass < 0 || pass > ANCSH_REFINE_MAX_ITERS) return refuse("%s: pass=%d must be in [0, %d]", who, pass, ANCSH_REFINE_MAX_ITERS);
    return is_last == 0 || is_last == 1 || refuse("%s: is_last=%d must be 0 or 1", who, is_last);
}
template <size_t N, typename... P>                                      // every pointer is a multiple of N bytes (a null pointer is)
inline bool all_aligned(P... p) { return ((... | (size_t)p) & (N - 1)) == 0; }
template <typename... P>                                                // ... of a depth value's size
inline bool depth_aligned(size_t item, P... p) { return item == 2 ? all_aligned<2>(p...) : all_aligned<4>(p...); }

}  // namespace ancsh
