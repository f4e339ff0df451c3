// joint_values.hip -- the joint values q of a posed frame read off its part poses (gfx950): ancsh_pose_scene_build's forward kinematics
// inverted on the predicted link maps.  Row (f, j) reports part j's bridging joint -- the lowest revolute or prismatic link of part j whose
// parent link belongs to another part -- under four pose groups (the record's two poses, the kept refined poses): the joint value, its error
// against the submitted one, how far the two sides of the joint are from lying on one axis (an angle and a gap) and the ratio of the two
// sides' scales; ONE launch at the step's end, whose (nframes, K, art_ld) articulation block it carries along in front of its own 24 columns
// (ancsh_joint_state_rec's idiom).  include/ancsh_hip.h states every formula and the order of every sum.
//
// One thread per (frame, part, group).  A link's predicted map is ancsh_reproject_scene_build's (compare_common.h's predicted_link_map: the
// same statements), child and parent each under the pose of their own part from the thread's group.  float64 arithmetic evaluated as written
// (the library is built with -ffp-contract=off).  No atomics, nothing allocated, every size an argument: capturable, the same bytes every
// run.  A few hundred double operations per thread: the launch sits on the floor of a dependent graph node.
#include "compare_common.h"

namespace ancsh {

constexpr int JV_THREADS = 256, JV_WIDTH = ANCSH_JOINT_VALUES_WIDTH, JV_GROUPS = 4, JV_HEAD = 4, JV_COLS = 5;
static_assert(JV_HEAD + JV_GROUPS * JV_COLS == JV_WIDTH, "4 head columns and 5 per pose group");

__device__ __forceinline__ double jv_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// sqrt((sum of the 9 squares of M) / 3), the squares added in row-major order: the scale of a map [M | tau]
__device__ __forceinline__ double jv_sigma(const double *B) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) s = s + B[4 * a + k] * B[4 * a + k];
    return sqrt(s / 3.0);
}

__global__ __launch_bounds__(JV_THREADS) void joint_values_kernel(int nframes, int K, const double *__restrict__ kin, int ninst,
                                                                  const double *__restrict__ pose, const double *__restrict__ render,
                                                                  const double *__restrict__ scene, const double *__restrict__ rig, int rig_ld,
                                                                  const float *__restrict__ norm_factor, const double *__restrict__ record, int ld,
                                                                  const double *__restrict__ refined, const double *__restrict__ art, int art_ld,
                                                                  double *__restrict__ wide) {
    constexpr double PI = 3.14159265358979323846, TWO_PI = 6.28318530717958647692;
    const long t = (long)blockIdx.x * JV_THREADS + threadIdx.x;
    if (t >= (long)nframes * K * JV_GROUPS) return;
    const int g = (int)(t % JV_GROUPS), j = (int)((t / JV_GROUPS) % K), f = (int)(t / ((long)JV_GROUPS * K));
    const size_t rowi = (size_t)f * K + j;
    double *out = wide + rowi * (size_t)(art_ld + JV_WIDTH);
    double *head = out + art_ld, *o = head + JV_HEAD + JV_COLS * g;
    const double qnan = __builtin_nan("");
    if (g == 0) {                                                       // the carried row, moved as 64-bit words so that a NaN keeps its payload
        const unsigned long long *ab = reinterpret_cast<const unsigned long long *>(art + rowi * (size_t)art_ld);
        unsigned long long *wb = reinterpret_cast<unsigned long long *>(out);
        for (int k = 0; k < art_ld; ++k) wb[k] = ab[k];
    }
    const double *sc = scene + (size_t)f * AN_SCENE, *rt = render + (size_t)f * ANCSH_RENDER_WIDTH, *rg = rig + (size_t)f * rig_ld;
    const double nf = (double)norm_factor[f];
    const double iv = rt[9];
    const int inst = iv >= 0.0 && iv < (double)ninst && (double)(int)iv == iv ? (int)iv : -1;
    // the bridging joint of part j.  Every index read from a table is checked before it is used: l < nl <= 16, p < l, inst < ninst
    const int nl = scene_nlinks(sc);
    int l = -1, p = -1, b = -1;
    double kd = 0.0;
    if (inst >= 0 && finite(nf) && nf != 0.0) {
        const double *kt = kin + (size_t)inst * ANCSH_KIN_WIDTH + ANCSH_KIN_HEAD;
        for (int c = 1; c < nl && l < 0; ++c) {
            if (scene_link_part(sc, c, nl, K) != j) continue;
            const double pd = kt[ANCSH_KIN_LINK * c + 2], kc = kt[ANCSH_KIN_LINK * c + 3];
            if (!(kc == 1.0 || kc == 2.0)) continue;
            const int pc = pd >= 0.0 && pd < (double)c && (double)(int)pd == pd ? (int)pd : -1;
            const int bc = pc >= 0 ? scene_link_part(sc, pc, nl, K) : -1;
            if (bc < 0 || bc == j) continue;
            l = c, p = pc, b = bc, kd = kc;
        }
    }
    if (l < 0) {                                                        // no such joint, or a frame without a norm factor or an instance: all NaN
        if (g == 0)
            for (int k = 0; k < JV_HEAD; ++k) head[k] = qnan;
        for (int k = 0; k < JV_COLS; ++k) o[k] = qnan;
        return;
    }
    const double *kl = kin + (size_t)inst * ANCSH_KIN_WIDTH + ANCSH_KIN_HEAD + ANCSH_KIN_LINK * l;
    const double q_true = pose ? pose[(size_t)f * ANCSH_POSE_WIDTH + l] : qnan;
    if (g == 0) head[0] = (double)l, head[1] = kd, head[2] = (double)b, head[3] = q_true;
    // the group's poses: child and parent each take their own part's
    const double *pc, *pp;
    if (g < 2) {
        pc = record + rowi * (size_t)ld + 13 * g;
        pp = record + ((size_t)f * K + b) * (size_t)ld + 13 * g;
    } else {
        pc = refined ? refined + (rowi * 2 + (g - 2)) * 18 : nullptr;
        pp = refined ? refined + (((size_t)f * K + b) * 2 + (g - 2)) * 18 : nullptr;
    }
    bool ok = pc && pose_ok(pc) && pose_ok(pp);
    double q = qnan, q_err = qnan, off_axis = qnan, gap = qnan, ratio = qnan;
    if (ok) {
        double Bl[12], Bp[12];
        predicted_link_map(rt, sc, rg, K, l, j, pc, nf, Bl);
        predicted_link_map(rt, sc, rg, K, p, b, pp, nf, Bp);
        const double sl = jv_sigma(Bl), sp = jv_sigma(Bp), ss = sp * sl;
        const double *T = kl + 4;
        const double a[3] = {kl[16], kl[17], kl[18]}, org[3] = {T[3], T[7], T[11]};
        double E[3][3], G[3][3], d[3], ra[3], w[3], u[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) E[i][k] = ((Bp[i] * Bl[k] + Bp[4 + i] * Bl[4 + k]) + Bp[8 + i] * Bl[8 + k]) / ss;       // M_p^T M_l / (sigma_p sigma_l)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) G[i][k] = (T[i] * E[0][k] + T[4 + i] * E[1][k]) + T[8 + i] * E[2][k];                 // Rt^T E
        const double v[3] = {(G[2][1] - G[1][2]) / 2.0, (G[0][2] - G[2][0]) / 2.0, (G[1][0] - G[0][1]) / 2.0};
        const double c = (((G[0][0] + G[1][1]) + G[2][2]) - 1.0) / 2.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            d[i] = Bl[4 * i + 3] - (jv_dot(Bp + 4 * i, org) + Bp[4 * i + 3]);                                                 // tau_l - (M_p org + tau_p)
            ra[i] = jv_dot(T + 4 * i, a);                                                                                     // Rt a
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = jv_dot(Bp + 4 * i, ra);
        const double len = sqrt(jv_dot(w, w));
#pragma unroll
        for (int i = 0; i < 3; ++i) u[i] = w[i] / len;
        ok = finite(sl) && sl != 0.0 && finite(sp) && sp != 0.0 && finite(len) && len != 0.0;
        if (ok) {
            if (kd == 1.0) {
                double Ga[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) Ga[i] = jv_dot(G[i], a);
                const double x[3] = {a[1] * Ga[2] - a[2] * Ga[1], a[2] * Ga[0] - a[0] * Ga[2], a[0] * Ga[1] - a[1] * Ga[0]};
                q = atan2(jv_dot(a, v), c);
                off_axis = atan2(sqrt(jv_dot(x, x)), jv_dot(a, Ga));
                gap = sqrt(jv_dot(d, d));
            } else {
                q = jv_dot(d, u);
                off_axis = atan2(sqrt(jv_dot(v, v)), c);
                const double r[3] = {d[0] - q * u[0], d[1] - q * u[1], d[2] - q * u[2]};
                gap = sqrt(jv_dot(r, r));
            }
            ratio = sl / sp;
            q_err = q - q_true;
            if (kd == 1.0) {                                            // into [-pi, pi] by one conditional -+ 2 pi
                if (q_err > PI) q_err = q_err - TWO_PI;
                else if (q_err < -PI) q_err = q_err + TWO_PI;
            }
        }
    }
    o[0] = q, o[1] = q_err, o[2] = off_axis, o[3] = gap, o[4] = ratio;
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_joint_values_rec(int nframes, int K, const double *kin, int ninst, const double *pose, const double *render,
                                      const double *scene, const double *rig, int rig_ld, const float *norm_factor, const double *record, int ld,
                                      const double *refined, const double *art, int art_ld, double *wide, void *stream) {
    ANCSH_CHECK(batch_ok("joint_values_rec", nframes, K, "exceed the 32767-frame range of ancsh_reproject_scene_build"));
    ANCSH_REQUIRE(ninst >= 1, "joint_values_rec: ninst=%d kinematic tables must be >= 1", ninst);
    ANCSH_REQUIRE(rig_ld == ANCSH_RIG_WIDTH(K), "joint_values_rec: rig_ld=%d, a rig of K=%d parts is %d wide", rig_ld, K, ANCSH_RIG_WIDTH(K));
    ANCSH_CHECK(record_ld_ok("joint_values_rec", "ld", ld));
    ANCSH_REQUIRE(art_ld == 12 || art_ld == 20, "joint_values_rec: art_ld=%d must be 12 (ancsh_articulation_rec) or 20 (ancsh_joint_state_rec)",
                  art_ld);
    ANCSH_REQUIRE(kin && render && scene && rig && norm_factor && record && art && wide, "joint_values_rec: null pointer");
    ANCSH_REQUIRE(all_aligned<4>(norm_factor) && all_aligned<8>(kin, pose, render, scene, rig, record, refined, art, wide), ANCSH_ALIGNED,
                  "joint_values_rec");
    ANCSH_REQUIRE(art != wide, "joint_values_rec: art and wide overlap (the rows have different widths: wide is a buffer of its own)");
    if (nframes == 0) return ANCSH_OK;
    const unsigned blocks = (unsigned)(((long)nframes * K * JV_GROUPS + JV_THREADS - 1) / JV_THREADS);
    hipLaunchKernelGGL(joint_values_kernel, dim3(blocks), dim3(JV_THREADS), 0, (hipStream_t)stream, nframes, K, kin, ninst, pose, render, scene, rig,
                       rig_ld, norm_factor, record, ld, refined, art, art_ld, wide);
    return check_launch("joint_values_rec");
}
