// scene_build.hip -- the two per-frame tables of a rendered, annotated frame built on the GPU (gfx950): an object's kinematic table (once
// per object) and one pose per frame (joint values and a view matrix) -> the render table ancsh_render_depth_labels reads and the scene
// table ancsh_depth_annotate_stream reads, where they read them.
//
// Reference: tools/render_synthetic.py:140-158, 206-217 takes the link poses from pybullet's forward kinematics on the host, and
// depth.pack_render_scene / depth.pack_frame_scene compose each link's maps with pinv / inv on 4 x 4 matrices, one frame at a time.  For
// rigid matrices both reduce to closed forms (include/ancsh_hip.h, ancsh_pose_scene_build, states them in full): with A_l = (V W_l)[:3, :]
// the render map is -A_l, and the scene map is [-Rc_l Ra^T | (-Rc_l Ra^T) ta + offset_l].
// ONE launch, one thread per (frame, link): the thread composes its link's world pose from the leaf upwards, so it keeps one 3 x 4 map and
// no per-link array; thread l of a frame also copies value l of either table's head.  float64 arithmetic evaluated as written (the library
// is built with -ffp-contract=off); the only values that are not a pure sequence of IEEE operations are sincos' two results.
// A LIBRARY of instances (ancsh_pose_scene_build_lib): a stack of tables, the instance of a frame in its pose's value 28; both kernels are
// wrappers around sb_frame_link.
#include "common.h"

namespace ancsh {

constexpr int SB_LINKS = ANCSH_SCENE_MAX_LINKS, SB_THREADS = 256;
constexpr int SB_KIN_HEAD = ANCSH_KIN_HEAD, SB_KIN_LINK = ANCSH_KIN_LINK;

// C = A o B of 3 x 4 rigid maps, row-major: C[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j], + A[i][3] for j = 3
__device__ __forceinline__ void sb_compose(const double *A, const double *B, double *C) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
            C[4 * i + j] = j == 3 ? v + A[4 * i + 3] : v;
        }
    }
}

// X_l = T_l o J_l(q): link l's frame in its parent's (link 0: in the world) at joint value q
__device__ __forceinline__ void sb_link_map(const double *__restrict__ kl, int l, double q, double *X) {
    const int kind = l == 0 ? 0 : (int)kl[3];
    const double a0 = kl[16], a1 = kl[17], a2 = kl[18];
    double J[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (kind == 1) {                                                    // revolute: c I + s [a]x + (1 - c) a a^T
        double s, c;
        sincos(q, &s, &c);
        const double a[3] = {a0, a1, a2};
        const double K[9] = {0.0, -a2, a1, a2, 0.0, -a0, -a1, a0, 0.0};
        const double u = 1.0 - c;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) J[4 * i + j] = (c * (i == j ? 1.0 : 0.0) + s * K[3 * i + j]) + (u * a[i]) * a[j];
    } else if (kind == 2) {                                             // prismatic: the translation q a
        J[3] = q * a0;
        J[7] = q * a1;
        J[11] = q * a2;
    }
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = kl[4 + k];
    sb_compose(T, J, X);
}

// thread l of a frame: link l's maps and value l of either head, from the object's table `kin` and the frame's pose `ps` into the frame's
// tables rt and sc -- both kernels' body.  r9: what the render table's value 9 reads (0 for one object, the instance for a library)
__device__ __forceinline__ void sb_frame_link(const double *__restrict__ kin, const double *__restrict__ ps, int l, double r9,
                                              double *__restrict__ rt, double *__restrict__ sc) {
    // the heads, value l of each: the scene's verbatim; the render's {P00..P12, depth_scale, z_min, nlinks, r9, 0 ..}
    sc[l] = kin[l];
    rt[l] = l < 6 ? kin[16 + l] : l == 6 ? kin[6] : l == 7 ? kin[22] : l == 8 ? kin[14] : l == 9 ? r9 : 0.0;
    double *R = rt + ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * l, *S = sc + ANCSH_SCENE_HEAD + ANCSH_SCENE_LINK * l;
    const double nlv = kin[14];
    const int nl = nlv >= 1.0 && nlv <= (double)SB_LINKS ? (int)nlv : 0;        // NaN fails both comparisons
    if (l >= nl) {                                                      // a link the object does not have reads 0
#pragma unroll
        for (int k = 0; k < ANCSH_RENDER_LINK; ++k) R[k] = 0.0;
#pragma unroll
        for (int k = 0; k < ANCSH_SCENE_LINK; ++k) S[k] = 0.0;
        return;
    }
    const double *kl = kin + SB_KIN_HEAD + SB_KIN_LINK * l;
    double W[12], X[12], C[12];
    sb_link_map(kl, l, ps[l], W);
    // from the leaf upwards: W <- X_p o W for p = parent(l), parent(p), ..., 0.  A parent is < its child (the host checks it; a table that
    // breaks the rule ends the walk), so the walk ends after at most 15 steps
    int cur = l;
    for (int p = (int)kl[2]; p >= 0 && p < cur; ) {
        const double *kp = kin + SB_KIN_HEAD + SB_KIN_LINK * p;
        sb_link_map(kp, p, ps[p], X);
        sb_compose(X, W, C);
#pragma unroll
        for (int k = 0; k < 12; ++k) W[k] = C[k];
        cur = p;
        p = (int)kp[2];
    }
    double V[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) V[k] = ps[16 + k];
    sb_compose(V, W, C);                                                // A_l = V o W_l = [Ra | ta]
#pragma unroll
    for (int k = 0; k < 12; ++k) R[k] = -C[k];                          // the render map
    S[0] = kl[0];
    S[1] = kl[1];
    const double *Rc = kl + 19, *off = kl + 28;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                       // the scene map: M[:, :3] = -Rc Ra^T, M[:, 3] = M[:, :3] ta + offset
        double m[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) m[j] = -((Rc[3 * i] * C[4 * j] + Rc[3 * i + 1] * C[4 * j + 1]) + Rc[3 * i + 2] * C[4 * j + 2]);
        S[2 + 4 * i] = m[0];
        S[3 + 4 * i] = m[1];
        S[4 + 4 * i] = m[2];
        S[5 + 4 * i] = ((m[0] * C[3] + m[1] * C[7]) + m[2] * C[11]) + off[i];
    }
}

__global__ __launch_bounds__(SB_THREADS) void pose_scene_build_kernel(int nframes, const double *__restrict__ kin,
                                                                      const double *__restrict__ pose, double *__restrict__ render,
                                                                      double *__restrict__ scene) {
    const int t = (int)(blockIdx.x * SB_THREADS + threadIdx.x), f = t / SB_LINKS, l = t % SB_LINKS;
    if (f >= nframes) return;
    sb_frame_link(kin, pose + (size_t)f * ANCSH_POSE_WIDTH, l, 0.0, render + (size_t)f * ANCSH_RENDER_WIDTH,
                  scene + (size_t)f * ANCSH_SCENE_WIDTH);
}

// the library's: frame f reads the table of the instance its pose names, pose[28]; a value that names none zeroes both tables
__global__ __launch_bounds__(SB_THREADS) void pose_scene_build_lib_kernel(int nframes, const double *__restrict__ kin, int ninst,
                                                                          const double *__restrict__ pose, double *__restrict__ render,
                                                                          double *__restrict__ scene) {
    const int t = (int)(blockIdx.x * SB_THREADS + threadIdx.x), f = t / SB_LINKS, l = t % SB_LINKS;
    if (f >= nframes) return;
    const double *ps = pose + (size_t)f * ANCSH_POSE_WIDTH;
    double *rt = render + (size_t)f * ANCSH_RENDER_WIDTH, *sc = scene + (size_t)f * ANCSH_SCENE_WIDTH;
    const int i = instance_index(ps[28], ninst);
    if (i < 0) {                                                        // thread l: value l of both heads and link l of both tables
        rt[l] = 0.0;
        sc[l] = 0.0;
        double *R = rt + ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * l, *S = sc + ANCSH_SCENE_HEAD + ANCSH_SCENE_LINK * l;
#pragma unroll
        for (int k = 0; k < ANCSH_RENDER_LINK; ++k) R[k] = 0.0;
#pragma unroll
        for (int k = 0; k < ANCSH_SCENE_LINK; ++k) S[k] = 0.0;
        return;
    }
    sb_frame_link(kin + (size_t)i * ANCSH_KIN_WIDTH, ps, l, (double)i, rt, sc);
}

}  // namespace ancsh

using namespace ancsh;

// what both entries check, under the entry's name
static int pose_scene_check(const char *name, int nframes, const double *kin, const double *pose, const double *render, const double *scene) {
    ANCSH_REQUIRE(nframes >= 0, "%s: bad shape nframes=%d", name, nframes);
    ANCSH_REQUIRE(nframes <= 65535, "%s: %d frames exceed the 65535-frame range of the entries that read the tables; split the batch", name,
                  nframes);
    ANCSH_REQUIRE(kin && pose && render && scene, "%s: null pointer", name);
    ANCSH_REQUIRE(((size_t)kin & 7) == 0 && ((size_t)pose & 7) == 0 && ((size_t)render & 7) == 0 && ((size_t)scene & 7) == 0,
                  "%s: kin, pose, render and scene must be 8-byte aligned", name);
    return ANCSH_OK;
}

extern "C" int ancsh_pose_scene_build(int nframes, const double *kin, const double *pose, double *render, double *scene, void *stream) {
    if (const int rc = pose_scene_check("pose_scene_build", nframes, kin, pose, render, scene)) return rc;
    if (nframes == 0) return ANCSH_OK;
    const unsigned blocks = (unsigned)(((long)nframes * SB_LINKS + SB_THREADS - 1) / SB_THREADS);
    hipLaunchKernelGGL(pose_scene_build_kernel, dim3(blocks), dim3(SB_THREADS), 0, (hipStream_t)stream, nframes, kin, pose, render, scene);
    return check_launch("pose_scene_build");
}

extern "C" int ancsh_pose_scene_build_lib(int nframes, const double *kin, int ninst, const double *pose, double *render, double *scene,
                                          void *stream) {
    if (const int rc = pose_scene_check("pose_scene_build_lib", nframes, kin, pose, render, scene)) return rc;
    ANCSH_REQUIRE(ninst >= 1 && ninst <= ANCSH_LIBRARY_MAX_INSTANCES, "pose_scene_build_lib: ninst=%d instances must be in [1, %d]", ninst,
                  ANCSH_LIBRARY_MAX_INSTANCES);
    if (nframes == 0) return ANCSH_OK;
    const unsigned blocks = (unsigned)(((long)nframes * SB_LINKS + SB_THREADS - 1) / SB_THREADS);
    hipLaunchKernelGGL(pose_scene_build_lib_kernel, dim3(blocks), dim3(SB_THREADS), 0, (hipStream_t)stream, nframes, kin, ninst, pose, render,
                       scene);
    return check_launch("pose_scene_build_lib");
}
