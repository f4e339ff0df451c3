// refinement.hip -- render-and-compare ICP of a pose record (gfx950): the loop that acts on what reprojection.hip only scores.  Each (frame,
// part, pose) is refined on its own: the part's rendered surface under the working pose is compared with the observed depth pixel by pixel
// (point-to-plane on same-pixel pairs), one damped Gauss-Newton step moves R and t (s is carried), the caller re-renders and repeats.  Two
// entries (include/ancsh_hip.h states both in full):
//   ancsh_refine_pass : ONE launch, one workgroup per (part, pose, frame) on reproject_compare_kernel's grid.  The threads stride the crop; a
//       pixel that is the part in both frames reads the z-buffer key the renderer left (float depth << 32 | triangle), rebuilds the winning
//       triangle's normal in the scaled cloud's space and adds its terms of A = sum J J^T, b = sum J r, sum r^2 in pixel order; a wave adds
//       its lanes with the fixed xor-shuffle tree, the four waves are added in wave order through LDS: no atomics, the same bytes every run.
//       Thread 0 computes the truncated cost, keeps the best pose so far, solves the 6 x 6 system by Cholesky and writes the updated pose.
//   ancsh_refine_rec  : ONE launch, the carried record row bit for bit and the 36 columns of the two best blocks behind it.
// The silhouette term, two more entries: ancsh_silhouette_field (ONE launch in front of the loop: per crop pixel and part the offset to the
// nearest pixel observed for the part) and ancsh_refine_pass_sil (the pass kernel's SIL instance: a predicted pixel of the part where the
// camera saw neither the part nor anything nearer adds one row that pulls it towards that nearest observed pixel, and is charged in the cost).
// The joint step, one more entry: ancsh_refine_joint_step (ONE launch behind each pass, one wave per (pose, frame): the parts' normal
// equations from `sums` and the rows that keep each revolute and prismatic joint's two sides on one axis, solved together by Cholesky in
// LDS; the poses and the best block the pass wrote are overwritten, the best-of is kept per object).  The pass kernel does not know of it.
// The coverage term, two more entries: ancsh_coverage_field (ONE launch behind the renderer in every pass: the field kernel on the predicted
// pair, per crop pixel and part the offset to the nearest pixel PREDICTED for the part) and ancsh_refine_pass_cov (the pass kernel's COV
// instance: an observed pixel of the part that the prediction leaves bare adds one row that pulls the nearest predicted pixel over it).
// The scale unknown, one more entry: ancsh_refine_pass_scale (the pass kernel's SCALE instance: the coverage instance plus one column -- every
// row also adds its derivative by a relative change sigma of the part's size about its centre, thread 0 solves 7 x 7 and s moves with R and t).
// float64 arithmetic evaluated as written (the library is built with -ffp-contract=off).
#include "compare_common.h"

namespace ancsh {

constexpr int RF_LINKS = ANCSH_SCENE_MAX_LINKS, RF_THREADS = 256, RF_WAVES = RF_THREADS / 64, RF_WIDTH = ANCSH_REFINE_WIDTH;
constexpr int RF_RENDER = ANCSH_RENDER_WIDTH, RF_BEST = ANCSH_REFINE_WIDTH / 2, RF_SUMS = ANCSH_REFINE_SUMS;
constexpr int RF_ACC = 30;                                              // A (21) | b (6) | sum r^2 | n_used | n_obs: what the block adds up
constexpr int RF_SIL_ACC = 33, RF_SIL_SUMS = ANCSH_REFINE_SIL_SUMS;     // ... | sum m^2 | n_sil | n_far: with the silhouette term
constexpr int RF_COV_ACC = 36, RF_COV_SUMS = ANCSH_REFINE_COV_SUMS;     // ... | sum m_c^2 | n_cov | n_cfar: with the coverage term as well
constexpr int RF_SCALE_ACC = 44, RF_SCALE_SUMS = ANCSH_REFINE_SCALE_SUMS;     // ... | A_0s .. A_5s | A_ss | b_s: with the scale unknown as well
constexpr int SF_THREADS = 256, SF_BAND = 16, SF_CHUNK = 256, SF_SPLIT = 8, SF_STEP = 8, SF_ILP = 8, SF_NONE = 0x7fffffff, SF_SENTINEL = -32768;

__device__ __forceinline__ double rf_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// a camera point (x', y', z) -> the scaled cloud: nf * (x', -y', z)
__device__ __forceinline__ void rf_cloud(double x, double y, double z, double nf, double *o) {
    o[0] = nf * x;
    o[1] = nf * (-y);
    o[2] = nf * z;
}

// the tail of a step, shared by the pass and the joint step: xi = (w, dt) as clamped -> the unit quaternion of w, its matrix, and the pose
// turned about the centre c and moved by dt; s is carried
__device__ __forceinline__ void rf_pose_step(const double *xi, const double *__restrict__ pose, const double *c, double *out) {
    const double hx = xi[0] / 2.0, hy = xi[1] / 2.0, hz = xi[2] / 2.0;  // the unit quaternion (1, w / 2) / |(1, w / 2)|
    const double qn = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / qn, x = hx / qn, yq = hy / qn, z = hz / qn;
    double dR[9];
    dR[0] = 1.0 - 2.0 * (yq * yq + z * z);
    dR[1] = 2.0 * (x * yq - w * z);
    dR[2] = 2.0 * (x * z + w * yq);
    dR[3] = 2.0 * (x * yq + w * z);
    dR[4] = 1.0 - 2.0 * (x * x + z * z);
    dR[5] = 2.0 * (yq * z - w * x);
    dR[6] = 2.0 * (x * z - w * yq);
    dR[7] = 2.0 * (yq * z + w * x);
    dR[8] = 1.0 - 2.0 * (x * x + yq * yq);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * a + k] = (dR[3 * a] * pose[k] + dR[3 * a + 1] * pose[3 + k]) + dR[3 * a + 2] * pose[6 + k];
    out[9] = pose[9];
    const double u[3] = {pose[10] - c[0], pose[11] - c[1], pose[12] - c[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) out[10 + a] = (rf_dot(dR + 3 * a, u) + c[a]) + xi[3 + a];
}

// the 6 x 6 solve, the clamp, the quaternion and the update of one pose, all by one thread in the header's written order.  S = the block's
// sums (A | b | ...), pose = the 13 values, c = the centre -> out (13 values); false (out untouched): the solve failed
__device__ __forceinline__ bool rf_solve_update(const double *S, const double *__restrict__ pose, const double *c, double damping,
                                                double max_angle, double max_dist, double *out) {
    double A[6][6], L[6][6], y[6], xi[6];
    int at = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = S[at++];
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k][k] = A[k][k] + (damping * A[k][k] + 1e-12);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            if (i == j) {
                ok = ok && s > 0.0 && finite(s);
                L[i][i] = sqrt(s);
            } else
                L[i][j] = s / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                       // L y = -b
        double s = 0.0 - S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                                      // L^T xi = y
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * xi[k];
        xi[i] = s / L[i][i];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && finite(xi[k]);
    if (!ok) return false;
    const double wn = sqrt(rf_dot(xi, xi)), dn = sqrt(rf_dot(xi + 3, xi + 3));
    if (wn > max_angle || dn > max_dist) {                              // one factor for the whole step: the smaller of the two ratios
        double f = 1.0;
        if (wn > max_angle) f = max_angle / wn;
        if (dn > max_dist && max_dist / dn < f) f = max_dist / dn;
#pragma unroll
        for (int k = 0; k < 6; ++k) xi[k] = xi[k] * f;
    }
    rf_pose_step(xi, pose, c, out);
    return true;
}

// the scale instance's step: rf_pose_step with a seventh value sigma = xi[6], x' = c + (1 + sigma) dR (x - c) + d
__device__ __forceinline__ void rf_pose_step_scale(const double *xi, const double *__restrict__ pose, const double *c, double *out) {
    const double hx = xi[0] / 2.0, hy = xi[1] / 2.0, hz = xi[2] / 2.0;
    const double qn = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / qn, x = hx / qn, yq = hy / qn, z = hz / qn;
    double dR[9];
    dR[0] = 1.0 - 2.0 * (yq * yq + z * z);
    dR[1] = 2.0 * (x * yq - w * z);
    dR[2] = 2.0 * (x * z + w * yq);
    dR[3] = 2.0 * (x * yq + w * z);
    dR[4] = 1.0 - 2.0 * (x * x + z * z);
    dR[5] = 2.0 * (yq * z - w * x);
    dR[6] = 2.0 * (x * z - w * yq);
    dR[7] = 2.0 * (yq * z + w * x);
    dR[8] = 1.0 - 2.0 * (x * x + yq * yq);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * a + k] = (dR[3 * a] * pose[k] + dR[3 * a + 1] * pose[3 + k]) + dR[3 * a + 2] * pose[6 + k];
    const double grow = 1.0 + xi[6];
    out[9] = pose[9] * grow;
    const double u[3] = {pose[10] - c[0], pose[11] - c[1], pose[12] - c[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) out[10 + a] = (grow * rf_dot(dR + 3 * a, u) + c[a]) + xi[3 + a];
}

// the 7 x 7 solve of the scale instance in rf_solve_update's order: rows 0..5 as there, row 6 the scale row (S[36..41] = A_0s .. A_5s, S[42] =
// A_ss, S[43] = b_s); the clamp with max_step beside the two others, then sigma alone held to s0's band.  false (out untouched): it failed
__device__ __forceinline__ bool rf_solve_update_scale(const double *S, const double *__restrict__ pose, const double *c, double damping,
                                                      double max_angle, double max_dist, double max_step, double max_total, double s0,
                                                      double *out) {
    double A[7][7], L[7][7], y[7], xi[7], rhs[7];
    int at = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = S[at++];
#pragma unroll
    for (int a = 0; a < 6; ++a) A[a][6] = A[6][a] = S[RF_COV_ACC + a], rhs[a] = S[21 + a];
    A[6][6] = S[RF_COV_ACC + 6];
    rhs[6] = S[RF_COV_ACC + 7];
#pragma unroll
    for (int k = 0; k < 7; ++k) A[k][k] = A[k][k] + (damping * A[k][k] + 1e-12);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            if (i == j) {
                ok = ok && s > 0.0 && finite(s);
                L[i][i] = sqrt(s);
            } else
                L[i][j] = s / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {                                       // L y = -b
        double s = 0.0 - rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {                                      // L^T xi = y
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; ++k) s = s - L[k][i] * xi[k];
        xi[i] = s / L[i][i];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) ok = ok && finite(xi[k]);
    if (!ok) return false;
    const double wn = sqrt(rf_dot(xi, xi)), dn = sqrt(rf_dot(xi + 3, xi + 3)), sn = fabs(xi[6]);
    if (wn > max_angle || dn > max_dist || sn > max_step) {             // one factor for all seven: the smallest of the ratios that apply
        double f = 1.0;
        if (wn > max_angle) f = max_angle / wn;
        if (dn > max_dist && max_dist / dn < f) f = max_dist / dn;
        if (sn > max_step && max_step / sn < f) f = max_step / sn;
#pragma unroll
        for (int k = 0; k < 7; ++k) xi[k] = xi[k] * f;
    }
    const double lo = s0 / (1.0 + max_total), hi = s0 * (1.0 + max_total), grown = pose[9] * (1.0 + xi[6]);
    if (grown > hi) xi[6] = hi / pose[9] - 1.0;                         // sigma alone: the kept s stays in the fitted s's band
    else if (grown < lo) xi[6] = lo / pose[9] - 1.0;
    const double kept = pose[9] * (1.0 + xi[6]);
    if (!(pose[9] > 0.0 && finite(kept) && kept > 0.0)) return false;
    rf_pose_step_scale(xi, pose, c, out);
    return true;
}

// the scale instance's two further kernel arguments, absent from the three other instances' signatures
__device__ __forceinline__ const double *rf_fitted() { return nullptr; }
__device__ __forceinline__ const double *rf_fitted(const double *fitted, int) { return fitted; }
__device__ __forceinline__ int rf_fitted_ld() { return 0; }
__device__ __forceinline__ int rf_fitted_ld(const double *, int ld) { return ld; }

// TERMS 1: ancsh_refine_pass_sil -- the overhang pixels add their rows (field: ancsh_silhouette_field's words), params holds 16 values and a
// sums row 36; TERMS 0: ancsh_refine_pass, instruction for instruction what it was before the term existed; TERMS 2: ancsh_refine_pass_cov --
// the gap pixels add their rows as well (cover: ancsh_coverage_field's words), params holds 32 values and a sums row 40; TERMS 3:
// ancsh_refine_pass_scale -- every row adds the scale column too, params holds 48 values and a sums row 48, and FIT = (fitted, ld_fitted)
template <typename T, int TERMS, typename... FIT>
__global__ __launch_bounds__(RF_THREADS) void refine_pass_kernel(int nframes, int K, const float *__restrict__ verts, const int *__restrict__ tris,
                                                                 const int *__restrict__ tri_link, int V, int ntri,
                                                                 const T *__restrict__ obs_depth, const unsigned char *__restrict__ obs_labels,
                                                                 long pixel_capacity, const unsigned long long *__restrict__ pred_zbuf,
                                                                 const T *__restrict__ pred_depth, const unsigned char *__restrict__ pred_labels,
                                                                 const int *__restrict__ geom, const double *__restrict__ scene,
                                                                 const double *__restrict__ pred_render, const float *__restrict__ norm_factor,
                                                                 const double *__restrict__ params, const int *__restrict__ field,
                                                                 const int *__restrict__ cover, int pass, int is_last,
                                                                 const double *__restrict__ pose_in, int ld_in, double *__restrict__ pose_out,
                                                                 double *__restrict__ best, double *__restrict__ sums, FIT... fit) {
    constexpr bool SIL = TERMS >= 1, COV = TERMS >= 2, SCL = TERMS == 3;
    constexpr int NACC = SCL ? RF_SCALE_ACC : COV ? RF_COV_ACC : SIL ? RF_SIL_ACC : RF_ACC;
    constexpr int NSUMS = SCL ? RF_SCALE_SUMS : COV ? RF_COV_SUMS : SIL ? RF_SIL_SUMS : RF_SUMS;
    __shared__ int s_part[RF_LINKS];
    __shared__ double s_red[RF_WAVES][NACC], s_tot[NACC];
    const int j = blockIdx.x, v = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const double *sc = scene + (size_t)f * AN_SCENE;
    const double *pose = pose_in + ((size_t)f * K + j) * ld_in + 13 * v;
    double *po = pose_out + ((size_t)f * K + j) * 26 + 13 * v;
    double *bb = best + (((size_t)f * K + j) * 2 + v) * RF_BEST, *ss = sums + (((size_t)f * K + j) * 2 + v) * NSUMS;
    const double nf = (double)norm_factor[f], qnan = __builtin_nan("");
    double s0 = 1.0;                                                    // the fitted s of this (frame, part, pose): not finite or not > 0 reads as a NaN pose
    if constexpr (SCL) s0 = rf_fitted(fit...)[((size_t)f * K + j) * rf_fitted_ld(fit...) + 13 * v + 9];
    if (!pose_ok(pose) || !finite(nf) || nf == 0.0 || (SCL && !(finite(s0) && s0 > 0.0))) {      // uniform over the block: NaN in the best block, the pose as it came
        if (tid < 13) po[tid] = pose[tid];
        if (tid < RF_BEST) bb[tid] = qnan;
        if (tid < NSUMS) ss[tid] = tid == RF_SUMS - 1 || tid == RF_SIL_SUMS - 1 || tid == RF_COV_SUMS - 1 ? 0.0 : qnan;
        return;
    }
    scene_part_table(sc, K, tid, s_part);
    __syncthreads();
    const double max_dist = params[1], min_cos = params[2];
    double c[3];
    pose_centre(pose, c);
    long start;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);       // [start, start + n) lies inside [0, pixel_capacity)
    const int row0 = geom[(size_t)f * DEPTH_GEOM + 3], col0 = geom[(size_t)f * DEPTH_GEOM + 4];
    const T *pd = pred_depth + (size_t)v * pixel_capacity;              // the pose's half of the predicted buffers, 2 * pixel_capacity long
    const unsigned char *pl = pred_labels + (size_t)v * pixel_capacity;
    const unsigned long long *pz = pred_zbuf + (size_t)v * pixel_capacity;
    const double *rt = pred_render + ((size_t)v * nframes + f) * RF_RENDER;
    const double scale = sc[6];
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
    for (long a = start + tid; a < start + n; a += RF_THREADS) {
        const T od = obs_depth[a], qd = pd[a];
        const unsigned long long key = pz[a];
        const int op = pixel_part(od, obs_labels[a], s_part);
        const int qp = pixel_part(qd, pl[a], s_part);
        const bool o = op == j, p = qp == j;
        acc[29] += o ? 1.0 : 0.0;
        if constexpr (SIL) {
            if (p && !o) {                                              // an OVERHANG pixel, unless another part hides the prediction here
                const double zp = (double)__uint_as_float((unsigned)(key >> 32));
                if (op >= 0 && !((double)od * scale > zp)) continue;
                const int fw = field[(size_t)j * pixel_capacity + a], di = (short)(fw & 0xffff), dj = (short)((unsigned)fw >> 16);
                if (di == SF_SENTINEL) continue;
                if ((double)(di * di + dj * dj) <= params[10] * params[10]) continue;
                const long e = a - start;
                const int ri = row0 + (int)(e / w), ci = col0 + (int)(e % w);
                const double row = (double)ri, col = (double)ci, row2 = (double)(ri + di), col2 = (double)(ci + dj);
                double su, sv, su2, sv2, pp[3], p2[3];
                pixel_ray(sc, row, col, su, sv);
                pixel_ray(sc, row2, col2, su2, sv2);
                rf_cloud(zp * su, zp * sv, zp, nf, pp);
                rf_cloud(zp * su2, zp * sv2, zp, nf, p2);
                const double dv[3] = {pp[0] - p2[0], pp[1] - p2[1], pp[2] - p2[2]};
                const double m = sqrt(rf_dot(dv, dv));
                if (!(m > 0.0)) continue;
                if (m > params[9]) {                                    // FAR: no row, charged dist^2
                    acc[32] += 1.0;
                    continue;
                }
                const double wt = params[8], g[3] = {dv[0] / m, dv[1] / m, dv[2] / m}, r = wt * m;
                const double pc[3] = {pp[0] - c[0], pp[1] - c[1], pp[2] - c[2]};
                const double J[6] = {wt * (pc[1] * g[2] - pc[2] * g[1]), wt * (pc[2] * g[0] - pc[0] * g[2]), wt * (pc[0] * g[1] - pc[1] * g[0]),
                                     wt * g[0], wt * g[1], wt * g[2]};
                int at = 0;
#pragma unroll
                for (int x = 0; x < 6; ++x)
#pragma unroll
                    for (int y = x; y < 6; ++y) acc[at++] += J[x] * J[y];
#pragma unroll
                for (int x = 0; x < 6; ++x) acc[21 + x] += J[x] * r;
                if constexpr (SCL) {
                    const double Js = wt * rf_dot(g, pc);
#pragma unroll
                    for (int x = 0; x < 6; ++x) acc[RF_COV_ACC + x] += J[x] * Js;
                    acc[RF_COV_ACC + 6] += Js * Js;
                    acc[RF_COV_ACC + 7] += Js * r;
                }
                acc[30] += m * m;
                acc[31] += 1.0;
                continue;
            }
        }
        if constexpr (COV) {
            if (o && !p) {                                              // a GAP pixel, unless the prediction puts another part in front of it
                if (qp >= 0 && !((double)__uint_as_float((unsigned)(key >> 32)) > (double)od * scale)) continue;
                const int cw = cover[((size_t)j * 2 + v) * pixel_capacity + a], di = (short)(cw & 0xffff), dj = (short)((unsigned)cw >> 16);
                if (di == SF_SENTINEL) continue;
                if ((double)(di * di + dj * dj) <= params[26] * params[26]) continue;
                const long e = a - start;
                const int li = (int)(e / w), lj = (int)(e % w);
                if (li + di < 0 || (long)(li + di) * w >= n || lj + dj < 0 || lj + dj >= w) continue;      // never with the field's own words
                const double z2 = (double)__uint_as_float((unsigned)(pz[start + (long)(li + di) * w + (lj + dj)] >> 32));
                const int ri = row0 + li, ci = col0 + lj;
                const double row = (double)ri, col = (double)ci, row2 = (double)(ri + di), col2 = (double)(ci + dj);
                double su, sv, su2, sv2, pn[3], pt[3];
                pixel_ray(sc, row, col, su, sv);
                pixel_ray(sc, row2, col2, su2, sv2);
                rf_cloud(z2 * su2, z2 * sv2, z2, nf, pn);
                rf_cloud(z2 * su, z2 * sv, z2, nf, pt);
                const double dv[3] = {pn[0] - pt[0], pn[1] - pt[1], pn[2] - pt[2]};
                const double m = sqrt(rf_dot(dv, dv));
                if (!(m > 0.0)) continue;
                if (m > params[25]) {                                   // FAR: no row, charged dist_c^2
                    acc[35] += 1.0;
                    continue;
                }
                const double wt = params[24], g[3] = {dv[0] / m, dv[1] / m, dv[2] / m}, r = wt * m;
                const double pc[3] = {pn[0] - c[0], pn[1] - c[1], pn[2] - c[2]};
                const double J[6] = {wt * (pc[1] * g[2] - pc[2] * g[1]), wt * (pc[2] * g[0] - pc[0] * g[2]), wt * (pc[0] * g[1] - pc[1] * g[0]),
                                     wt * g[0], wt * g[1], wt * g[2]};
                int at = 0;
#pragma unroll
                for (int x = 0; x < 6; ++x)
#pragma unroll
                    for (int y = x; y < 6; ++y) acc[at++] += J[x] * J[y];
#pragma unroll
                for (int x = 0; x < 6; ++x) acc[21 + x] += J[x] * r;
                if constexpr (SCL) {
                    const double Js = wt * rf_dot(g, pc);
#pragma unroll
                    for (int x = 0; x < 6; ++x) acc[RF_COV_ACC + x] += J[x] * Js;
                    acc[RF_COV_ACC + 6] += Js * Js;
                    acc[RF_COV_ACC + 7] += Js * r;
                }
                acc[33] += m * m;
                acc[34] += 1.0;
                continue;
            }
        }
        if (!(o && p)) continue;
        const unsigned t = (unsigned)key;
        if (t >= (unsigned)ntri) continue;                              // a predicted pixel has a winner; a key that names none is skipped
        const int ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2], l = tri_link[t];
        if (l < 0 || l >= RF_LINKS || ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;
        const long e = a - start;
        const double row = (double)(row0 + (int)(e / w)), col = (double)(col0 + (int)(e % w));
        double su, sv, q[3], pp[3], vt[3][3];
        pixel_ray(sc, row, col, su, sv);
        const double zo = (double)od * scale, zp = (double)__uint_as_float((unsigned)(key >> 32));
        rf_cloud(zo * su, zo * sv, zo, nf, q);
        rf_cloud(zp * su, zp * sv, zp, nf, pp);
        const double *R = rt + ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * l;
        const int idx[3] = {ia, ib, ic};
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                   // render_vertex's transform, then the same map into the cloud
            const float *vp = verts + 3 * (size_t)idx[k];
            const double v0 = vp[0], v1 = vp[1], v2 = vp[2];
            double m[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) m[b] = ((R[4 * b] * v0 + R[4 * b + 1] * v1) + R[4 * b + 2] * v2) + R[4 * b + 3];
            rf_cloud(m[0], m[1], m[2], nf, vt[k]);
        }
        const double e1[3] = {vt[1][0] - vt[0][0], vt[1][1] - vt[0][1], vt[1][2] - vt[0][2]};
        const double e2[3] = {vt[2][0] - vt[0][0], vt[2][1] - vt[0][1], vt[2][2] - vt[0][2]};
        double nn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = sqrt(rf_dot(nn, nn));
        if (!(len > 0.0 && finite(len))) continue;
#pragma unroll
        for (int b = 0; b < 3; ++b) nn[b] = nn[b] / len;
        double nq = rf_dot(nn, q);
        if (nq > 0.0) {                                                 // the normal faces the camera
#pragma unroll
            for (int b = 0; b < 3; ++b) nn[b] = -nn[b];
            nq = -nq;
        }
        const double d[3] = {pp[0] - q[0], pp[1] - q[1], pp[2] - q[2]};
        if (!(sqrt(rf_dot(d, d)) <= max_dist)) continue;
        if (!(fabs(nq) / sqrt(rf_dot(q, q)) >= min_cos)) continue;
        const double r = rf_dot(nn, d);
        const double pc[3] = {pp[0] - c[0], pp[1] - c[1], pp[2] - c[2]};
        const double J[6] = {pc[1] * nn[2] - pc[2] * nn[1], pc[2] * nn[0] - pc[0] * nn[2], pc[0] * nn[1] - pc[1] * nn[0], nn[0], nn[1], nn[2]};
        int at = 0;
#pragma unroll
        for (int x = 0; x < 6; ++x)
#pragma unroll
            for (int y = x; y < 6; ++y) acc[at++] += J[x] * J[y];
#pragma unroll
        for (int x = 0; x < 6; ++x) acc[21 + x] += J[x] * r;
        if constexpr (SCL) {                                            // the point moves as c + (1 + sigma)(pp - c): d r / d sigma = n . (pp - c)
            const double Js = rf_dot(nn, pc);
#pragma unroll
            for (int x = 0; x < 6; ++x) acc[RF_COV_ACC + x] += J[x] * Js;
            acc[RF_COV_ACC + 6] += Js * Js;
            acc[RF_COV_ACC + 7] += Js * r;
        }
        acc[27] += r * r;
        acc[28] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < NACC; ++k) {                                    // a fixed tree: xor shuffles, then the waves in order
        double s = acc[k];
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) s_red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < NACC) s_tot[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    __syncthreads();
    // sum m^2, n_sil, n_far lie behind C and solved, the coverage's three behind [35]
    if constexpr (SCL) {                                                // ... and the scale column's eight behind [39]
        if (tid < NACC) ss[tid < RF_ACC ? tid : tid < RF_SIL_ACC ? tid + 2 : tid < RF_COV_ACC ? tid + 3 : tid + 4] = s_tot[tid];
    } else if (tid < NACC) ss[tid < RF_ACC ? tid : tid < RF_SIL_ACC ? tid + 2 : tid + 3] = s_tot[tid];
    if (tid != 0) return;
    const double n_used = s_tot[28], n_obs = s_tot[29];
    double C, n_rows = n_used;
    if constexpr (COV) {
        C = (((s_tot[27] + (max_dist * max_dist) * (n_obs - n_used)) + (params[8] * params[8]) * (s_tot[30] + (params[9] * params[9]) * s_tot[32])) +
             (params[24] * params[24]) * (s_tot[33] + (params[25] * params[25]) * s_tot[35])) / n_obs;
        n_rows = (n_used + s_tot[31]) + s_tot[34];
        ss[RF_SIL_SUMS - 1] = ss[RF_COV_SUMS - 1] = 0.0;
    } else if constexpr (SIL) {
        C = ((s_tot[27] + (max_dist * max_dist) * (n_obs - n_used)) + (params[8] * params[8]) * (s_tot[30] + (params[9] * params[9]) * s_tot[32])) / n_obs;
        n_rows = n_used + s_tot[31];
        ss[RF_SIL_SUMS - 1] = 0.0;
    } else
        C = (s_tot[27] + (max_dist * max_dist) * (n_obs - n_used)) / n_obs;               // n_obs = 0: 0 / 0 = NaN
    ss[30] = C;
    double solved = pass == 0 ? 0.0 : bb[17];
    if (pass == 0 || C < bb[14]) {                                      // strictly lower: ties stay with the earlier pass; NaN never wins
#pragma unroll
        for (int k = 0; k < 13; ++k) bb[k] = pose[k];
        if (pass == 0) bb[13] = C;
        bb[14] = C;
        bb[15] = n_used;
        bb[16] = (double)pass;
    }
    double nw[13];
    bool ok = false;
    if (!is_last && n_rows >= params[5]) {
        if constexpr (SCL) ok = rf_solve_update_scale(s_tot, pose, c, params[3], params[4], max_dist, params[32], params[33], s0, nw);
        else ok = rf_solve_update(s_tot, pose, c, params[3], params[4], max_dist, nw);
    }
    ss[31] = ok ? 1.0 : 0.0;
    bb[17] = ok ? solved + 1.0 : solved;
#pragma unroll
    for (int k = 0; k < 13; ++k) po[k] = ok ? nw[k] : pose[k];
}

__global__ __launch_bounds__(RF_THREADS) void refine_rec_kernel(long rows, const double *__restrict__ best, const double *__restrict__ carried,
                                                                int ld, double *__restrict__ wide) {
    const long total = rows * (ld + RF_WIDTH), e = (long)blockIdx.x * RF_THREADS + threadIdx.x;
    if (e >= total) return;
    const long r = e / (ld + RF_WIDTH);
    const int k = (int)(e - r * (ld + RF_WIDTH));
    wide[e] = k < ld ? carried[r * ld + k] : best[r * RF_WIDTH + (k - ld)];     // the carried row bit for bit, the two best blocks behind it
}

// ancsh_silhouette_field: per crop pixel and part the offset (di, dj) to the nearest pixel OBSERVED for the part, ordered by (squared pixel
// distance, row, column), all in integers.  Separable: g(i, c) = the nearest observed row of column c from row i (ties: the upper row), then
// the minimum over the columns of (jj - c)^2 + g^2.  One workgroup per (part, row-band worker, frame): worker y takes the bands y, y +
// SF_SPLIT, ... of SF_BAND rows; per band and per chunk of SF_CHUNK columns one thread per column walks its column (up from the band to the
// first observed row above, through the band, down to the first below) and leaves g in LDS; then a thread takes SF_ILP pixels of one row
// at a time and scans the chunk's columns in ascending order, one LDS read of g for all of them, an empty column skipped.  A pixel's
// running best of a further chunk is read back from its own output word (the same thread wrote it).  No atomics; every word of a crop is
// written exactly once per chunk by one thread, nothing outside the crops is touched.  Frame row f reads scene row f % scene_rows:
// ancsh_coverage_field runs it over the 2 * nframes predicted frames, whose row v * nframes + f is frame f's scene.
template <typename T>
__global__ __launch_bounds__(SF_THREADS) void silhouette_field_kernel(int K, const T *__restrict__ obs_depth, const unsigned char *__restrict__ obs_labels,
                                                                      long pixel_capacity, const int *__restrict__ geom,
                                                                      const double *__restrict__ scene, int scene_rows, int *__restrict__ field) {
    __shared__ int s_part[RF_LINKS];
    __shared__ int s_g[SF_BAND][SF_CHUNK];
    const int j = blockIdx.x, f = blockIdx.z, tid = threadIdx.x;
    const double *sc = scene + (size_t)(f % scene_rows) * AN_SCENE;
    scene_part_table(sc, K, tid, s_part);
    __syncthreads();
    long start;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);       // [start, start + n) lies inside [0, pixel_capacity); 0: no crop
    if (n == 0) return;
    const int h = (int)(n / w);
    int *out = field + (size_t)j * pixel_capacity;                      // part j's plane; written at [start, start + n) only
    const bool wide = h > 32767 || w > 32767;                           // an offset would not fit its 16 bits: the sentinel everywhere
    const int none = (int)(((unsigned)SF_SENTINEL & 0xffffu) | ((unsigned)SF_SENTINEL << 16));
    auto seen = [&](int r, int c) {
        const long a = start + (long)r * w + c;                         // pixel_part's rule, the label first: most pixels need no depth
        const unsigned char lab = obs_labels[a];
        return lab < RF_LINKS && s_part[lab] == j && depth_ok(obs_depth[a]);
    };
    for (int i0 = (int)blockIdx.y * SF_BAND; i0 < h; i0 += SF_BAND * SF_SPLIT) {
        const int nb = h - i0 < SF_BAND ? h - i0 : SF_BAND;
        if (wide) {
            for (long e = tid; e < (long)nb * w; e += SF_THREADS) out[start + (long)i0 * w + e] = none;
            continue;
        }
        for (int c0 = 0; c0 < w; c0 += SF_CHUNK) {
            const int nc = w - c0 < SF_CHUNK ? w - c0 : SF_CHUNK;
            __syncthreads();                                            // the last chunk's readers are done with s_g
            if (tid < nc) {
                const int c = c0 + tid;
                int last = -1, next = -1;
                for (int r1 = i0; r1 > 0 && last < 0; r1 -= SF_STEP) {  // SF_STEP rows at a time, their loads in flight together, until one is seen
                    bool s[SF_STEP];
#pragma unroll
                    for (int u = 0; u < SF_STEP; ++u) s[u] = r1 - 1 - u >= 0 && seen(r1 - 1 - u, c);
#pragma unroll
                    for (int u = SF_STEP - 1; u >= 0; --u)
                        if (s[u]) last = r1 - 1 - u;                    // the nearest one is assigned last
                }
                bool in[SF_BAND];
#pragma unroll
                for (int k = 0; k < SF_BAND; ++k) in[k] = k < nb && seen(i0 + k, c);
#pragma unroll
                for (int k = 0; k < SF_BAND; ++k) {
                    if (in[k]) last = i0 + k;
                    if (k < nb) s_g[k][tid] = last;                     // the nearest observed row at or above, or -1
                }
                for (int r1 = i0 + nb; r1 < h && next < 0; r1 += SF_STEP) {
                    bool s[SF_STEP];
#pragma unroll
                    for (int u = 0; u < SF_STEP; ++u) s[u] = r1 + u < h && seen(r1 + u, c);
#pragma unroll
                    for (int u = SF_STEP - 1; u >= 0; --u)
                        if (s[u]) next = r1 + u;
                }
                for (int k = nb - 1; k >= 0; --k) {
                    const int r = i0 + k, up = s_g[k][tid];
                    if (up == r) next = r;
                    int g = SF_NONE;
                    if (up >= 0 && next >= 0) g = r - up <= next - r ? up - r : next - r;      // equal distances: the upper row
                    else if (up >= 0) g = up - r;
                    else if (next >= 0) g = next - r;
                    s_g[k][tid] = g;
                }
            }
            __syncthreads();
            // one work item = SF_ILP pixels of ONE row, columns x, x + groups, ...: a column's g is read once for all of them, an empty
            // column costs one comparison, and neighbouring lanes write neighbouring words
            const int groups = (w + SF_ILP - 1) / SF_ILP;
            for (int q = tid; q < nb * groups; q += SF_THREADS) {       // nb * groups <= 16 * 4096
                const int k = q / groups, x = q - k * groups;
                const long a0 = start + (long)(i0 + k) * w;
                int bdi[SF_ILP], bdj[SF_ILP];
                unsigned bd2[SF_ILP];
#pragma unroll
                for (int u = 0; u < SF_ILP; ++u) {
                    const int jj = x + u * groups;
                    bdi[u] = bdj[u] = SF_SENTINEL;
                    bd2[u] = 0xffffffffu;                               // above every real distance: 2 * 32767^2 < 2^31
                    if (c0 > 0 && jj < w) {
                        const int fw = out[a0 + jj];
                        bdi[u] = (short)(fw & 0xffff);
                        bdj[u] = (short)((unsigned)fw >> 16);
                        if (bdi[u] != SF_SENTINEL) bd2[u] = (unsigned)(bdi[u] * bdi[u]) + (unsigned)(bdj[u] * bdj[u]);
                    }
                }
                for (int t = 0; t < nc; ++t) {
                    const int g = s_g[k][t];
                    if (g == SF_NONE) continue;
                    const unsigned gg = (unsigned)__mul24(g, g);        // |g|, |dj| <= 32767: the 24-bit multiply is exact
#pragma unroll
                    for (int u = 0; u < SF_ILP; ++u) {
                        const int dj = c0 + t - (x + u * groups);       // a column past the crop's width is computed and never written
                        const unsigned d2 = gg + (unsigned)__mul24(dj, dj);
                        if (d2 < bd2[u] || (d2 == bd2[u] && g < bdi[u])) {      // equal rows: the earlier (lower) column stays
                            bd2[u] = d2;
                            bdi[u] = g;
                            bdj[u] = dj;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < SF_ILP; ++u)
                    if (x + u * groups < w) out[a0 + x + u * groups] = (int)(((unsigned)bdi[u] & 0xffffu) | ((unsigned)bdj[u] << 16));
            }
        }
    }
}

// ancsh_refine_joint_step: the parts of one object solved together through their joints, ONE wave per (pose v, frame f), launched behind the
// pass.  The pass left every part's 6 x 6 normal equations in `sums`; this kernel adds the rows that keep each revolute or prismatic joint's
// two sides on one axis, solves the 6 K system by Cholesky in LDS, clamps the step by one factor, overwrites the poses the pass wrote, and keeps
// the best-of per OBJECT (state: its shadow of the best block; obj: the object's row).  include/ancsh_hip.h states every formula and order.
constexpr int JS_THREADS = 64, JS_PARTS = 8, JS_N = 6 * JS_PARTS, JS_LD = JS_N + 1, JS_ROWS = 9, JS_COLS = 12, JS_OBJ = ANCSH_REFINE_OBJ;

// link map l of a render table: x (model frame) -> the scaled cloud, nf * F (R x + t)
__device__ __forceinline__ void js_point(const double *__restrict__ R, const double *x, double nf, double *o) {
    double m[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) m[b] = ((R[4 * b] * x[0] + R[4 * b + 1] * x[1]) + R[4 * b + 2] * x[2]) + R[4 * b + 3];
    rf_cloud(m[0], m[1], m[2], nf, o);
}

// ... a direction: normalise(F R d); false: its length is 0 or not finite
__device__ __forceinline__ bool js_dir(const double *__restrict__ R, const double *d, double *o) {
    double m[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) m[b] = (R[4 * b] * d[0] + R[4 * b + 1] * d[1]) + R[4 * b + 2] * d[2];
    m[1] = -m[1];
    const double len = sqrt(rf_dot(m, m));
#pragma unroll
    for (int b = 0; b < 3; ++b) o[b] = m[b] / len;
    return len > 0.0 && finite(len);
}

// three rows r0 + G xi of one joint into LDS: G = sc [-[e]x | id I] for the child's part (columns 0..5), sc [[h]x | -id I] for the parent's
__device__ __forceinline__ void js_rows(double (*G)[JS_COLS], double *r0, const double *e, const double *h, const double *r, double sc, double id) {
    const double ea[3] = {sc * e[0], sc * e[1], sc * e[2]}, ha[3] = {sc * h[0], sc * h[1], sc * h[2]};
    G[0][0] = 0.0, G[0][1] = ea[2], G[0][2] = -ea[1], G[1][0] = -ea[2], G[1][1] = 0.0, G[1][2] = ea[0], G[2][0] = ea[1], G[2][1] = -ea[0], G[2][2] = 0.0;
    G[0][6] = 0.0, G[0][7] = -ha[2], G[0][8] = ha[1], G[1][6] = ha[2], G[1][7] = 0.0, G[1][8] = -ha[0], G[2][6] = -ha[1], G[2][7] = ha[0], G[2][8] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int k = 0; k < 3; ++k) G[a][3 + k] = a == k ? id : 0.0, G[a][9 + k] = a == k ? -id : 0.0;
        r0[a] = sc * r[a];
    }
}

__global__ __launch_bounds__(JS_THREADS) void refine_joint_step_kernel(int nframes, int K, const double *__restrict__ kin, int ninst,
                                                                       const double *__restrict__ scene, const double *__restrict__ pred_render,
                                                                       const float *__restrict__ norm_factor, const double *__restrict__ params,
                                                                       int pass, int is_last, const double *__restrict__ pose_in, int ld_in,
                                                                       const double *__restrict__ sums, int sums_ld, double *__restrict__ pose_out,
                                                                       double *__restrict__ best, double *__restrict__ state,
                                                                       double *__restrict__ obj, double *__restrict__ xi_out) {
    __shared__ double s_H[JS_N][JS_LD], s_g[JS_N], s_x[JS_N];           // 48 x 49 doubles: 18.4 KB; the odd row length spreads a column over the banks
    __shared__ double s_G[RF_LINKS][JS_ROWS][JS_COLS], s_r0[RF_LINKS][JS_ROWS], s_rr[RF_LINKS], s_gap[RF_LINKS];      // 13.5 KB
    __shared__ double s_c[JS_PARTS][3], s_n[JS_PARTS];
    __shared__ int s_part[RF_LINKS], s_live[JS_PARTS], s_rows[RF_LINKS], s_pa[RF_LINKS], s_pb[RF_LINKS], s_fail;
    const int v = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, n = 6 * K;
    const double *sc = scene + (size_t)f * AN_SCENE, *rt = pred_render + ((size_t)v * nframes + f) * RF_RENDER;
    const double nf = (double)norm_factor[f], qnan = __builtin_nan("");
    const double max_dist = params[1], damping = params[3], max_angle = params[4], min_pixels = params[5], weight = params[16], axis_len = params[17];
    const bool nf_ok = finite(nf) && nf != 0.0;
    const size_t part0 = ((size_t)f * K) * 2 + v;                       // part j's row of best, state and sums: (part0 + 2 j) * its width
    if (tid < RF_LINKS) {                                               // scene_part_table's line, with this kernel's own tables
        s_part[tid] = scene_link_part(sc, tid, scene_nlinks(sc), K);
        s_rows[tid] = 0;
        s_rr[tid] = s_gap[tid] = 0.0;
    }
    if (tid == 0) s_fail = 0;
    if (tid < JS_PARTS) {
        bool live = false;
        double nj = 0.0;
        if (tid < K) {
            const double *pose = pose_in + ((size_t)f * K + tid) * ld_in + 13 * v, *S = sums + (part0 + 2 * (size_t)tid) * sums_ld;
            live = nf_ok && pose_ok(pose);
            if (live) {
                pose_centre(pose, s_c[tid]);
                nj = S[28];
                if (sums_ld == RF_SIL_SUMS || sums_ld == RF_COV_SUMS) nj = nj + S[33];
                if (sums_ld == RF_COV_SUMS) nj = nj + S[37];
            }
        }
        s_live[tid] = live ? 1 : 0;
        s_n[tid] = nj;
    }
    __syncthreads();
    // nbar: the mean rows of the live parts that solve on their own
    double nsum = 0.0, ncount = 0.0;
    for (int j = 0; j < K; ++j)
        if (s_live[j] && s_n[j] >= min_pixels) nsum = nsum + s_n[j], ncount = ncount + 1.0;
    const bool has_nbar = ncount > 0.0;
    const double w2n = has_nbar ? (weight * weight) * (nsum / ncount) : 0.0;
    // lane l: link l's joint.  Every index read from a table is checked before it is used
    const int nl = scene_nlinks(sc);
    const double iv = rt[9];                                            // common.h's instance_index, written out: its floor test moved this kernel's
    const int inst = iv >= 0.0 && iv < (double)ninst && (double)(int)iv == iv ? (int)iv : -1;      // registers and cost it 0.5 %
    if (tid >= 1 && tid < nl && inst >= 0) {
        const int l = tid;
        const double *kl = kin + (size_t)inst * ANCSH_KIN_WIDTH + ANCSH_KIN_HEAD + ANCSH_KIN_LINK * l;
        const double pd = kl[2], kd = kl[3];
        const int p = pd >= 0.0 && pd < (double)l && (double)(int)pd == pd ? (int)pd : -1;
        const int a = s_part[l], b = p >= 0 ? s_part[p] : -1;
        if ((kd == 1.0 || kd == 2.0) && a >= 0 && b >= 0 && a != b && s_live[a] && s_live[b]) {
            const double *Rl = rt + ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * l, *Rp = rt + ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * p, *T = kl + 4;
            const double zero[3] = {0.0, 0.0, 0.0}, org[3] = {T[3], T[7], T[11]}, ax[3] = {kl[16], kl[17], kl[18]};
            double xc[3], xp[3], uc[3], up[3], axp[3];
            js_point(Rl, zero, nf, xc);
            js_point(Rp, org, nf, xp);
#pragma unroll
            for (int i = 0; i < 3; ++i) axp[i] = (T[4 * i] * ax[0] + T[4 * i + 1] * ax[1]) + T[4 * i + 2] * ax[2];
            bool ok = js_dir(Rl, ax, uc);
            ok = js_dir(Rp, axp, up) && ok;
            const double e[3] = {xc[0] - s_c[a][0], xc[1] - s_c[a][1], xc[2] - s_c[a][2]};
            const double h[3] = {xp[0] - s_c[b][0], xp[1] - s_c[b][1], xp[2] - s_c[b][2]};
            const double r[3] = {xc[0] - xp[0], xc[1] - xp[1], xc[2] - xp[2]}, du[3] = {uc[0] - up[0], uc[1] - up[1], uc[2] - up[2]};
            double(*G)[JS_COLS] = s_G[l];
            double *r0 = s_r0[l];
            int rows = 6;
            js_rows(G, r0, e, h, r, 1.0, 1.0);
            js_rows(G + 3, r0 + 3, uc, up, du, axis_len, 0.0);
            if (kd == 2.0) {                                            // prismatic: the position rows projected off the axis, a second direction
                double P[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) P[i][k] = (i == k ? 1.0 : 0.0) - up[i] * up[k];
                for (int cidx = 0; cidx <= JS_COLS; ++cidx) {           // column 12: the residual
                    const double g0 = cidx < JS_COLS ? G[0][cidx] : r0[0], g1 = cidx < JS_COLS ? G[1][cidx] : r0[1], g2 = cidx < JS_COLS ? G[2][cidx] : r0[2];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const double pg = (P[i][0] * g0 + P[i][1] * g1) + P[i][2] * g2;
                        if (cidx < JS_COLS) G[i][cidx] = pg;
                        else r0[i] = pg;
                    }
                }
                const double a0 = fabs(ax[0]), a1 = fabs(ax[1]), a2 = fabs(ax[2]);
                const int k = a1 < a0 ? (a2 < a1 ? 2 : 1) : (a2 < a0 ? 2 : 0);                // the smallest |a_k|, ties: the lowest index
                const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
                double bx[3] = {ax[1] * ek[2] - ax[2] * ek[1], ax[2] * ek[0] - ax[0] * ek[2], ax[0] * ek[1] - ax[1] * ek[0]}, bxp[3], vc[3], vp[3];
                const double bl = sqrt(rf_dot(bx, bx));
                ok = ok && bl > 0.0 && finite(bl);
#pragma unroll
                for (int i = 0; i < 3; ++i) bx[i] = bx[i] / bl;
#pragma unroll
                for (int i = 0; i < 3; ++i) bxp[i] = (T[4 * i] * bx[0] + T[4 * i + 1] * bx[1]) + T[4 * i + 2] * bx[2];
                ok = js_dir(Rl, bx, vc) && ok;
                ok = js_dir(Rp, bxp, vp) && ok;
                const double dv[3] = {vc[0] - vp[0], vc[1] - vp[1], vc[2] - vp[2]};
                js_rows(G + 6, r0 + 6, vc, vp, dv, axis_len, 0.0);
                rows = 9;
            }
            double rr = 0.0;
            for (int i = 0; i < rows; ++i) {
                ok = ok && finite(r0[i]);
                rr = rr + r0[i] * r0[i];
            }
            if (ok) {                                                   // a joint whose rows are not finite is not active
                s_rows[l] = rows;
                s_pa[l] = a;
                s_pb[l] = b;
                s_rr[l] = rr;
                s_gap[l] = rf_dot(r0, r0);
            }
        }
    }
    __syncthreads();
    double njoints = 0.0, sumr = 0.0, gap = 0.0;
    for (int l = 1; l < RF_LINKS; ++l)
        if (s_rows[l]) njoints = njoints + 1.0, sumr = sumr + s_rr[l], gap = gap + s_gap[l];
    // the object's cost
    double num = 0.0, den = 0.0, moved = 0.0;
    for (int j = 0; j < K; ++j) {
        if (!s_live[j]) continue;
        const double *S = sums + (part0 + 2 * (size_t)j) * sums_ld;
        if (S[29] > 0.0) num = num + S[30] * S[29], den = den + S[29];
        if (S[31] == 1.0) moved = 1.0;
    }
    const bool coupled = njoints > 0.0 && has_nbar;
    if (coupled) num = num + w2n * sumr;
    const double Cobj = den > 0.0 ? num / den : qnan;
    bool solved = false;
    double fclamp = 1.0;
    if (coupled && !is_last) {                                          // uniform over the wave
        for (int e = tid; e < JS_N * JS_LD; e += JS_THREADS) (&s_H[0][0])[e] = 0.0;
        __syncthreads();
        for (int e = tid; e < 36 * K; e += JS_THREADS) {                // the parts' own blocks, damped as the pass damps them
            const int j = e / 36, a = (e % 36) / 6, b = e % 6, lo = a < b ? a : b, hi = a < b ? b : a;
            const double *S = sums + (part0 + 2 * (size_t)j) * sums_ld;
            double h = a == b ? 1.0 : 0.0;
            if (s_live[j]) {
                h = s_n[j] >= min_pixels ? S[6 * lo - (lo * (lo - 1)) / 2 + (hi - lo)] : 0.0;
                if (a == b) h = h + (damping * h + 1e-12);
            }
            s_H[6 * j + a][6 * j + b] = h;
        }
        if (tid < n) {
            const int j = tid / 6;
            s_g[tid] = s_live[j] && s_n[j] >= min_pixels ? sums[(part0 + 2 * (size_t)j) * sums_ld + 21 + tid % 6] : 0.0;
        }
        __syncthreads();
        for (int l = 1; l < RF_LINKS; ++l) {                            // + weight^2 nbar G^T G, joint after joint; an element's rows in order
            const int rows = s_rows[l];
            if (!rows) continue;
            const int a = s_pa[l], b = s_pb[l];
            for (int e = tid; e < JS_COLS * JS_COLS + JS_COLS; e += JS_THREADS) {
                const int p = e / JS_COLS, q = e % JS_COLS;
                double t = 0.0;
                if (p < JS_COLS) {
                    for (int r = 0; r < rows; ++r) t = t + s_G[l][r][p] * s_G[l][r][q];
                    double *h = &s_H[p < 6 ? 6 * a + p : 6 * b + (p - 6)][q < 6 ? 6 * a + q : 6 * b + (q - 6)];
                    *h = *h + w2n * t;
                } else {
                    for (int r = 0; r < rows; ++r) t = t + s_G[l][r][q] * s_r0[l][r];
                    double *g = &s_g[q < 6 ? 6 * a + q : 6 * b + (q - 6)];
                    *g = *g + w2n * t;
                }
            }
            __syncthreads();
        }
        for (int jc = 0; jc < n; ++jc) {                                // Cholesky in place, column after column; lane i owns row i
            double s = 0.0;
            if (tid >= jc && tid < n) {
                s = s_H[tid][jc];
                for (int k = 0; k < jc; ++k) s = s - s_H[tid][k] * s_H[jc][k];
                if (tid == jc) {
                    if (!(s > 0.0 && finite(s))) s_fail = 1;
                    s_H[jc][jc] = sqrt(s);
                }
            }
            __syncthreads();
            if (tid > jc && tid < n) s_H[tid][jc] = s / s_H[jc][jc];
            __syncthreads();
        }
        double s = tid < n ? 0.0 - s_g[tid] : 0.0;                      // L y = -g: y_k as soon as it is final, k ascending
        for (int k = 0; k < n; ++k) {
            if (tid == k) s_x[k] = s / s_H[k][k];
            __syncthreads();
            if (tid > k && tid < n) s = s - s_H[tid][k] * s_x[k];
        }
        __syncthreads();
        s = tid < n ? s_x[tid] : 0.0;                                   // L^T xi = y: xi_k as soon as it is final, k descending
        __syncthreads();
        for (int k = n - 1; k >= 0; --k) {
            if (tid == k) s_x[k] = s / s_H[k][k];
            __syncthreads();
            if (tid < k) s = s - s_H[k][tid] * s_x[k];
        }
        __syncthreads();
        solved = !s_fail;
        for (int k = 0; k < n; ++k) solved = solved && finite(s_x[k]);
        if (solved) {
            for (int j = 0; j < K; ++j) {                               // one factor for the whole object
                if (!s_live[j]) continue;
                const double wn = sqrt(rf_dot(s_x + 6 * j, s_x + 6 * j)), dn = sqrt(rf_dot(s_x + 6 * j + 3, s_x + 6 * j + 3));
                if (wn > max_angle && max_angle / wn < fclamp) fclamp = max_angle / wn;
                if (dn > max_dist && max_dist / dn < fclamp) fclamp = max_dist / dn;
            }
            if (tid < K && s_live[tid]) {
                const double *pose = pose_in + ((size_t)f * K + tid) * ld_in + 13 * v;
                double xi[6], nw[13];
#pragma unroll
                for (int k = 0; k < 6; ++k) xi[k] = fclamp < 1.0 ? s_x[6 * tid + k] * fclamp : s_x[6 * tid + k];
                rf_pose_step(xi, pose, s_c[tid], nw);
                double *po = pose_out + ((size_t)f * K + tid) * 26 + 13 * v;
#pragma unroll
                for (int k = 0; k < 13; ++k) po[k] = nw[k];
            }
        }
    }
    if (xi_out && tid < JS_N) xi_out[((size_t)f * 2 + v) * JS_N + tid] = solved && tid < n ? (fclamp < 1.0 ? s_x[tid] * fclamp : s_x[tid]) : 0.0;
    if (solved) moved = 1.0;
    // best-of, per object: every lane reads the object's row before lane 0 rewrites it
    double *ob = obj + ((size_t)f * 2 + v) * JS_OBJ;
    const double cost_start = pass == 0 ? Cobj : ob[0], cost_best = pass == 0 ? Cobj : ob[1], prev_pass = pass == 0 ? 0.0 : ob[2];
    const double prev_solved = pass == 0 ? 0.0 : ob[3];
    const bool take = pass == 0 || Cobj < cost_best;                    // strictly lower: ties stay with the earlier pass; NaN never wins
    const double best_pass = take ? (double)pass : prev_pass, passes_solved = prev_solved + moved;
    __syncthreads();
    if (tid == 0) {
        ob[0] = cost_start;
        ob[1] = take ? Cobj : cost_best;
        ob[2] = best_pass;
        ob[3] = passes_solved;
        ob[4] = Cobj;
        ob[5] = njoints;
        ob[6] = solved ? 1.0 : 0.0;
        ob[7] = njoints > 0.0 ? sqrt(gap / njoints) : qnan;
    }
    if (tid < K) {
        const double *pose = pose_in + ((size_t)f * K + tid) * ld_in + 13 * v, *S = sums + (part0 + 2 * (size_t)tid) * sums_ld;
        double *st = state + (part0 + 2 * (size_t)tid) * RF_BEST, *bb = best + (part0 + 2 * (size_t)tid) * RF_BEST;
        const bool live = s_live[tid] != 0;
        if (take) {
#pragma unroll
            for (int k = 0; k < 13; ++k) st[k] = pose[k];
            if (pass == 0) st[13] = live ? S[30] : qnan;
            st[14] = live ? S[30] : qnan;
            st[15] = live ? S[28] : qnan;
        }
        st[16] = best_pass;
        st[17] = passes_solved;
#pragma unroll
        for (int k = 0; k < RF_BEST; ++k) bb[k] = live ? st[k] : qnan;   // a part that is not live reads NaN, as the pass leaves it
    }
}

}  // namespace ancsh

using namespace ancsh;

// the three passes' checks and launch: who = the entry's name in its messages; TERMS = 1: with the field, the 16-value table and the 36-value
// sums; 2: with cover, the 32-value table and the 40-value sums as well; 3: with fitted / ld_fitted, the 48-value table and the 48-value sums
template <int TERMS>
static int refine_pass_call(const char *who, int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V,
                            int T, const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                            const unsigned long long *pred_zbuf, const void *pred_depth, const unsigned char *pred_labels, const int *geom,
                            const double *scene, const double *pred_render, const float *norm_factor, const double *params, const int *field,
                            const int *cover, const double *fitted, int ld_fitted, int pass, int is_last, const double *pose_in, int ld_in,
                            double *pose_out, double *best, double *sums, void *stream) {
    ANCSH_CHECK(batch_ok(who, nframes, K, "exceed the 32767-frame range of ancsh_reproject_scene_build"));
    size_t item;
    ANCSH_CHECK(depth_item(who, depth_type, item));
    ANCSH_CHECK(capacity_ok(who, pixel_capacity));
    ANCSH_REQUIRE(T >= 0 && T < (1 << 24), "%s: T=%d triangles must be in [0, 2^24)", who, T);
    ANCSH_REQUIRE(V >= 0 && V < (1 << 24), "%s: V=%d vertices must be in [0, 2^24)", who, V);
    ANCSH_CHECK(pass_ok(who, pass, is_last));
    ANCSH_CHECK(record_ld_ok(who, "ld_in", ld_in));
    if (TERMS == 3) ANCSH_CHECK(record_ld_ok(who, "ld_fitted", ld_fitted));
    ANCSH_REQUIRE(verts && tris && tri_link && obs_depth && obs_labels && pred_zbuf && pred_depth && pred_labels && geom && scene &&
                      pred_render && norm_factor && params && pose_in && pose_out && best && sums && (field || TERMS < 1) && (cover || TERMS < 2) &&
                      (fitted || TERMS < 3), "%s: null pointer", who);
    ANCSH_REQUIRE(depth_aligned(item, obs_depth, pred_depth) && all_aligned<4>(verts, tris, tri_link, geom, norm_factor, field, cover) &&
                      all_aligned<8>(pred_zbuf, scene, pred_render, params, pose_in, pose_out, best, sums, fitted), ANCSH_ALIGNED, who);
    ANCSH_REQUIRE(pose_in != pose_out, "%s: pose_in and pose_out overlap (a workgroup reads its pose while another writes: two buffers)", who);
    if (nframes == 0) return ANCSH_OK;
    const dim3 grid(K, 2, nframes);
    if constexpr (TERMS == 3) {
        if (depth_type == ANCSH_DEPTH_U16)
            hipLaunchKernelGGL((refine_pass_kernel<unsigned short, TERMS, const double *, int>), grid, dim3(RF_THREADS), 0, (hipStream_t)stream,
                               nframes, K, verts, tris, tri_link, V, T, (const unsigned short *)obs_depth, obs_labels, pixel_capacity, pred_zbuf,
                               (const unsigned short *)pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, field, cover, pass,
                               is_last, pose_in, ld_in, pose_out, best, sums, fitted, ld_fitted);
        else
            hipLaunchKernelGGL((refine_pass_kernel<float, TERMS, const double *, int>), grid, dim3(RF_THREADS), 0, (hipStream_t)stream, nframes, K,
                               verts, tris, tri_link, V, T, (const float *)obs_depth, obs_labels, pixel_capacity, pred_zbuf,
                               (const float *)pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, field, cover, pass, is_last,
                               pose_in, ld_in, pose_out, best, sums, fitted, ld_fitted);
    } else if (depth_type == ANCSH_DEPTH_U16)
        hipLaunchKernelGGL((refine_pass_kernel<unsigned short, TERMS>), grid, dim3(RF_THREADS), 0, (hipStream_t)stream, nframes, K, verts, tris,
                           tri_link, V, T, (const unsigned short *)obs_depth, obs_labels, pixel_capacity, pred_zbuf,
                           (const unsigned short *)pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, field, cover, pass,
                           is_last, pose_in, ld_in, pose_out, best, sums);
    else
        hipLaunchKernelGGL((refine_pass_kernel<float, TERMS>), grid, dim3(RF_THREADS), 0, (hipStream_t)stream, nframes, K, verts, tris, tri_link, V,
                           T, (const float *)obs_depth, obs_labels, pixel_capacity, pred_zbuf, (const float *)pred_depth, pred_labels, geom,
                           scene, pred_render, norm_factor, params, field, cover, pass, is_last, pose_in, ld_in, pose_out, best, sums);
    return check_launch(who);
}

extern "C" int ancsh_refine_pass(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                 const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                                 const unsigned long long *pred_zbuf, const void *pred_depth, const unsigned char *pred_labels, const int *geom,
                                 const double *scene, const double *pred_render, const float *norm_factor, const double *params, int pass,
                                 int is_last, const double *pose_in, int ld_in, double *pose_out, double *best, double *sums, void *stream) {
    return refine_pass_call<0>("refine_pass", nframes, K, depth_type, verts, tris, tri_link, V, T, obs_depth, obs_labels, pixel_capacity,
                               pred_zbuf, pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, nullptr, nullptr, nullptr, 0, pass,
                               is_last, pose_in, ld_in, pose_out, best, sums, stream);
}

extern "C" int ancsh_refine_pass_sil(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                     const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                                     const unsigned long long *pred_zbuf, const void *pred_depth, const unsigned char *pred_labels,
                                     const int *geom, const double *scene, const double *pred_render, const float *norm_factor,
                                     const double *params, const int *field, int pass, int is_last, const double *pose_in, int ld_in,
                                     double *pose_out, double *best, double *sums, void *stream) {
    return refine_pass_call<1>("refine_pass_sil", nframes, K, depth_type, verts, tris, tri_link, V, T, obs_depth, obs_labels, pixel_capacity,
                               pred_zbuf, pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, field, nullptr, nullptr, 0, pass,
                               is_last, pose_in, ld_in, pose_out, best, sums, stream);
}

extern "C" int ancsh_refine_pass_cov(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                     const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                                     const unsigned long long *pred_zbuf, const void *pred_depth, const unsigned char *pred_labels,
                                     const int *geom, const double *scene, const double *pred_render, const float *norm_factor,
                                     const double *params, const int *field, const int *cover, int pass, int is_last, const double *pose_in,
                                     int ld_in, double *pose_out, double *best, double *sums, void *stream) {
    return refine_pass_call<2>("refine_pass_cov", nframes, K, depth_type, verts, tris, tri_link, V, T, obs_depth, obs_labels, pixel_capacity,
                               pred_zbuf, pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, field, cover, nullptr, 0, pass,
                               is_last, pose_in, ld_in, pose_out, best, sums, stream);
}

extern "C" int ancsh_refine_pass_scale(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                       const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                                       const unsigned long long *pred_zbuf, const void *pred_depth, const unsigned char *pred_labels,
                                       const int *geom, const double *scene, const double *pred_render, const float *norm_factor,
                                       const double *params, const int *field, const int *cover, const double *fitted, int ld_fitted, int pass,
                                       int is_last, const double *pose_in, int ld_in, double *pose_out, double *best, double *sums,
                                       void *stream) {
    return refine_pass_call<3>("refine_pass_scale", nframes, K, depth_type, verts, tris, tri_link, V, T, obs_depth, obs_labels, pixel_capacity,
                               pred_zbuf, pred_depth, pred_labels, geom, scene, pred_render, norm_factor, params, field, cover, fitted, ld_fitted,
                               pass, is_last, pose_in, ld_in, pose_out, best, sums, stream);
}

extern "C" int ancsh_refine_joint_step(int nframes, int K, const double *kin, int ninst, const double *scene, const double *pred_render,
                                       const float *norm_factor, const double *params, int pass, int is_last, const double *pose_in, int ld_in,
                                       const double *sums, int sums_ld, double *pose_out, double *best, double *state, double *obj, double *xi,
                                       void *stream) {
    ANCSH_CHECK(batch_ok("refine_joint_step", nframes, K, "exceed the 32767-frame range of ancsh_refine_pass"));
    ANCSH_REQUIRE(ninst >= 1 && ninst <= 65535, "refine_joint_step: ninst=%d kinematic tables must be in [1, 65535]", ninst);
    ANCSH_CHECK(pass_ok("refine_joint_step", pass, is_last));
    ANCSH_CHECK(record_ld_ok("refine_joint_step", "ld_in", ld_in));
    ANCSH_REQUIRE(sums_ld == ANCSH_REFINE_SUMS || sums_ld == ANCSH_REFINE_SIL_SUMS || sums_ld == ANCSH_REFINE_COV_SUMS,
                  "refine_joint_step: sums_ld=%d must be %d (ancsh_refine_pass), %d (ancsh_refine_pass_sil) or %d (ancsh_refine_pass_cov)", sums_ld,
                  ANCSH_REFINE_SUMS, ANCSH_REFINE_SIL_SUMS, ANCSH_REFINE_COV_SUMS);
    ANCSH_REQUIRE(kin && scene && pred_render && norm_factor && params && pose_in && sums && pose_out && best && state && obj,
                  "refine_joint_step: null pointer");
    ANCSH_REQUIRE(all_aligned<4>(norm_factor) && all_aligned<8>(kin, scene, pred_render, params, pose_in, sums, pose_out, best, state, obj, xi),
                  ANCSH_ALIGNED, "refine_joint_step");
    ANCSH_REQUIRE(pose_in != pose_out, "refine_joint_step: pose_in and pose_out overlap (the poses the pass evaluated are read while the new ones are "
                  "written: two buffers)");
    ANCSH_REQUIRE(best != state, "refine_joint_step: best and state overlap (state is the object's shadow of the best block: a buffer of its own)");
    if (nframes == 0) return ANCSH_OK;
    hipLaunchKernelGGL(refine_joint_step_kernel, dim3(2, nframes), dim3(JS_THREADS), 0, (hipStream_t)stream, nframes, K, kin, ninst, scene,
                       pred_render, norm_factor, params, pass, is_last, pose_in, ld_in, sums, sums_ld, pose_out, best, state, obj, xi);
    return check_launch("refine_joint_step");
}

// both fields' checks and launch: the kernel over `halves` * nframes frames of buffers of `halves` * pixel_capacity pixels, frame row v * nframes
// + f reading scene row f
static int field_call(const char *who, const char *why, int halves, int nframes, int K, int depth_type, const void *depth,
                      const unsigned char *labels, long pixel_capacity, const int *geom, const double *scene, int *field, void *stream) {
    ANCSH_CHECK(batch_ok(who, nframes, K, why));
    size_t item;
    ANCSH_CHECK(depth_item(who, depth_type, item));
    ANCSH_CHECK(capacity_ok(who, pixel_capacity));
    ANCSH_REQUIRE(depth && labels && geom && scene && field, "%s: null pointer", who);
    ANCSH_REQUIRE(depth_aligned(item, depth) && all_aligned<4>(geom, field) && all_aligned<8>(scene), ANCSH_ALIGNED, who);
    if (nframes == 0) return ANCSH_OK;
    const dim3 grid(K, SF_SPLIT, halves * nframes);                     // <= 2 * 32767 frames: within the grid's 65535
    if (depth_type == ANCSH_DEPTH_U16)
        hipLaunchKernelGGL(silhouette_field_kernel<unsigned short>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, K,
                           (const unsigned short *)depth, labels, halves * pixel_capacity, geom, scene, nframes, field);
    else
        hipLaunchKernelGGL(silhouette_field_kernel<float>, grid, dim3(SF_THREADS), 0, (hipStream_t)stream, K, (const float *)depth, labels,
                           halves * pixel_capacity, geom, scene, nframes, field);
    return check_launch(who);
}

extern "C" int ancsh_silhouette_field(int nframes, int K, int depth_type, const void *obs_depth, const unsigned char *obs_labels,
                                      long pixel_capacity, const int *geom, const double *scene, int *field, void *stream) {
    return field_call("silhouette_field", "exceed the 32767-frame range of ancsh_refine_pass_sil", 1, nframes, K, depth_type, obs_depth, obs_labels,
                      pixel_capacity, geom, scene, field, stream);
}

extern "C" int ancsh_coverage_field(int nframes, int K, int depth_type, const void *pred_depth, const unsigned char *pred_labels,
                                    long pixel_capacity, const int *geom_out, const double *scene, int *cover, void *stream) {
    return field_call("coverage_field", "exceed the 32767-frame range of ancsh_refine_pass_cov", 2, nframes, K, depth_type, pred_depth, pred_labels,
                      pixel_capacity, geom_out, scene, cover, stream);
}

extern "C" int ancsh_refine_rec(int nframes, int K, const double *best, const double *carried, int ld, double *wide, void *stream) {
    ANCSH_CHECK(batch_ok("refine_rec", nframes, K, "exceed the 32767-frame range of ancsh_refine_pass"));
    ANCSH_CHECK(record_ld_ok("refine_rec", "ld", ld));
    ANCSH_REQUIRE(ld <= 4096, "refine_rec: ld=%d, a record row holds at most 4096 columns", ld);
    ANCSH_REQUIRE(best && carried && wide, "refine_rec: null pointer");
    ANCSH_REQUIRE(all_aligned<8>(best, carried, wide), ANCSH_ALIGNED, "refine_rec");
    ANCSH_REQUIRE(carried != wide, "refine_rec: carried and wide overlap (the rows have different widths: wide is a buffer of its own)");
    if (nframes == 0) return ANCSH_OK;
    const long rows = (long)nframes * K, total = rows * (ld + RF_WIDTH);               // < 2^15 * 8 * 2^13 = 2^31
    hipLaunchKernelGGL(refine_rec_kernel, dim3((unsigned)((total + RF_THREADS - 1) / RF_THREADS)), dim3(RF_THREADS), 0, (hipStream_t)stream, rows,
                       best, carried, ld, wide);
    return check_launch("refine_rec");
}
