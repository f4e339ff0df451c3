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
// float64 arithmetic evaluated as written (the library is built with -ffp-contract=off).
#include "depth_annotate_common.h"

namespace ancsh {

constexpr int RF_LINKS = ANCSH_SCENE_MAX_LINKS, RF_THREADS = 256, RF_WAVES = RF_THREADS / 64, RF_WIDTH = ANCSH_REFINE_WIDTH;
constexpr int RF_RENDER = ANCSH_RENDER_WIDTH, RF_BEST = ANCSH_REFINE_WIDTH / 2, RF_SUMS = ANCSH_REFINE_SUMS;
constexpr int RF_ACC = 30;                                              // A (21) | b (6) | sum r^2 | n_used | n_obs: what the block adds up

__device__ __forceinline__ bool rf_finite(double v) { return fabs(v) < __builtin_inf(); }      // NaN fails the comparison

__device__ __forceinline__ bool rf_pose_ok(const double *__restrict__ p) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 13; ++k) ok = ok && rf_finite(p[k]);
    return ok;
}

template <typename T>
__device__ __forceinline__ int rf_pixel_part(T d, unsigned char lab, const int *s_part) {      // reprojection.hip's rp_pixel_part
    return lab < RF_LINKS && depth_ok(d) ? s_part[lab] : -1;
}

__device__ __forceinline__ double rf_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// a camera point (x', y', z) -> the scaled cloud: nf * (x', -y', z)
__device__ __forceinline__ void rf_cloud(double x, double y, double z, double nf, double *o) {
    o[0] = nf * x;
    o[1] = nf * (-y);
    o[2] = nf * z;
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
                ok = ok && s > 0.0 && rf_finite(s);
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
    for (int k = 0; k < 6; ++k) ok = ok && rf_finite(xi[k]);
    if (!ok) return false;
    const double wn = sqrt(rf_dot(xi, xi)), dn = sqrt(rf_dot(xi + 3, xi + 3));
    if (wn > max_angle || dn > max_dist) {                              // one factor for the whole step: the smaller of the two ratios
        double f = 1.0;
        if (wn > max_angle) f = max_angle / wn;
        if (dn > max_dist && max_dist / dn < f) f = max_dist / dn;
#pragma unroll
        for (int k = 0; k < 6; ++k) xi[k] = xi[k] * f;
    }
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
    return true;
}

template <typename T>
__global__ __launch_bounds__(RF_THREADS) void refine_pass_kernel(int nframes, int K, const float *__restrict__ verts, const int *__restrict__ tris,
                                                                 const int *__restrict__ tri_link, int V, int ntri,
                                                                 const T *__restrict__ obs_depth, const unsigned char *__restrict__ obs_labels,
                                                                 long pixel_capacity, const unsigned long long *__restrict__ pred_zbuf,
                                                                 const T *__restrict__ pred_depth, const unsigned char *__restrict__ pred_labels,
                                                                 const int *__restrict__ geom, const double *__restrict__ scene,
                                                                 const double *__restrict__ pred_render, const float *__restrict__ norm_factor,
                                                                 const double *__restrict__ params, int pass, int is_last,
                                                                 const double *__restrict__ pose_in, int ld_in, double *__restrict__ pose_out,
                                                                 double *__restrict__ best, double *__restrict__ sums) {
    __shared__ int s_part[RF_LINKS];
    __shared__ double s_red[RF_WAVES][RF_ACC], s_tot[RF_ACC];
    const int j = blockIdx.x, v = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const double *sc = scene + (size_t)f * AN_SCENE;
    const double *pose = pose_in + ((size_t)f * K + j) * ld_in + 13 * v;
    double *po = pose_out + ((size_t)f * K + j) * 26 + 13 * v;
    double *bb = best + (((size_t)f * K + j) * 2 + v) * RF_BEST, *ss = sums + (((size_t)f * K + j) * 2 + v) * RF_SUMS;
    const double nf = (double)norm_factor[f], qnan = __builtin_nan("");
    if (!rf_pose_ok(pose) || !rf_finite(nf) || nf == 0.0) {             // uniform over the block: NaN in the best block, the pose as it came
        if (tid < 13) po[tid] = pose[tid];
        if (tid < RF_BEST) bb[tid] = qnan;
        if (tid < RF_SUMS) ss[tid] = tid == RF_SUMS - 1 ? 0.0 : qnan;
        return;
    }
    if (tid < RF_LINKS) {
        const int nl = scene_nlinks(sc);
        const double pv = sc[AN_HEAD + AN_LINK * tid + 1];
        s_part[tid] = scene_rank(sc, tid, nl) >= 0 && pv >= 0.0 && pv < (double)K ? (int)pv : -1;
    }
    __syncthreads();
    const double max_dist = params[1], min_cos = params[2];
    double c[3];                                                        // the centre: s R (0.5, 0.5, 0.5) + t
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = pose[9] * ((pose[3 * a] * 0.5 + pose[3 * a + 1] * 0.5) + pose[3 * a + 2] * 0.5) + pose[10 + a];
    long start;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);       // [start, start + n) lies inside [0, pixel_capacity)
    const int row0 = geom[(size_t)f * DEPTH_GEOM + 3], col0 = geom[(size_t)f * DEPTH_GEOM + 4];
    const T *pd = pred_depth + (size_t)v * pixel_capacity;              // the pose's half of the predicted buffers, 2 * pixel_capacity long
    const unsigned char *pl = pred_labels + (size_t)v * pixel_capacity;
    const unsigned long long *pz = pred_zbuf + (size_t)v * pixel_capacity;
    const double *rt = pred_render + ((size_t)v * nframes + f) * RF_RENDER;
    const double scale = sc[6];
    double acc[RF_ACC];
#pragma unroll
    for (int k = 0; k < RF_ACC; ++k) acc[k] = 0.0;
    for (long a = start + tid; a < start + n; a += RF_THREADS) {
        const T od = obs_depth[a], qd = pd[a];
        const unsigned long long key = pz[a];
        const bool o = rf_pixel_part(od, obs_labels[a], s_part) == j, p = rf_pixel_part(qd, pl[a], s_part) == j;
        acc[29] += o ? 1.0 : 0.0;
        if (!(o && p)) continue;
        const unsigned t = (unsigned)key;
        if (t >= (unsigned)ntri) continue;                              // a predicted pixel has a winner; a key that names none is skipped
        const int ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2], l = tri_link[t];
        if (l < 0 || l >= RF_LINKS || ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;
        const long e = a - start;
        const double row = (double)(row0 + (int)(e / w)), col = (double)(col0 + (int)(e % w));
        const double su = (sc[7] * col + sc[8] * row) + sc[9], sv = (sc[10] * col + sc[11] * row) + sc[12];
        const double zo = (double)od * scale, zp = (double)__uint_as_float((unsigned)(key >> 32));
        double q[3], pp[3], vt[3][3];
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
        if (!(len > 0.0 && rf_finite(len))) continue;
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
        acc[27] += r * r;
        acc[28] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < RF_ACC; ++k) {                                  // a fixed tree: xor shuffles, then the waves in order
        double s = acc[k];
#pragma unroll
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) s_red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < RF_ACC) s_tot[tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    __syncthreads();
    if (tid < RF_ACC) ss[tid] = s_tot[tid];
    if (tid != 0) return;
    const double n_used = s_tot[28], n_obs = s_tot[29];
    const double C = (s_tot[27] + (max_dist * max_dist) * (n_obs - n_used)) / n_obs;      // n_obs = 0: 0 / 0 = NaN
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
    if (!is_last && n_used >= params[5]) ok = rf_solve_update(s_tot, pose, c, params[3], params[4], max_dist, nw);
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

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_refine_pass(int nframes, int K, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                 const void *obs_depth, const unsigned char *obs_labels, long pixel_capacity,
                                 const unsigned long long *pred_zbuf, const void *pred_depth, const unsigned char *pred_labels, const int *geom,
                                 const double *scene, const double *pred_render, const float *norm_factor, const double *params, int pass,
                                 int is_last, const double *pose_in, int ld_in, double *pose_out, double *best, double *sums, void *stream) {
    ANCSH_REQUIRE(nframes >= 0, "refine_pass: bad shape nframes=%d", nframes);
    ANCSH_REQUIRE(nframes <= 32767, "refine_pass: %d frames exceed the 32767-frame range of ancsh_reproject_scene_build; split the batch", nframes);
    ANCSH_REQUIRE(K >= 1 && K <= 8, "refine_pass: K=%d must be in [1, 8]", K);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32,
                  "refine_pass: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 29), "refine_pass: pixel_capacity=%ld pixels out of range", pixel_capacity);
    ANCSH_REQUIRE(T >= 0 && T < (1 << 24), "refine_pass: T=%d triangles must be in [0, 2^24)", T);
    ANCSH_REQUIRE(V >= 0 && V < (1 << 24), "refine_pass: V=%d vertices must be in [0, 2^24)", V);
    ANCSH_REQUIRE(pass >= 0 && pass <= ANCSH_REFINE_MAX_ITERS, "refine_pass: pass=%d must be in [0, %d]", pass, ANCSH_REFINE_MAX_ITERS);
    ANCSH_REQUIRE(is_last == 0 || is_last == 1, "refine_pass: is_last=%d must be 0 or 1", is_last);
    ANCSH_REQUIRE(ld_in >= 26, "refine_pass: ld_in=%d, a record row holds at least the 26 pose columns", ld_in);
    ANCSH_REQUIRE(verts && tris && tri_link && obs_depth && obs_labels && pred_zbuf && pred_depth && pred_labels && geom && scene &&
                      pred_render && norm_factor && params && pose_in && pose_out && best && sums,
                  "refine_pass: null pointer");
    const size_t item = depth_type == ANCSH_DEPTH_U16 ? 2 : 4;
    ANCSH_REQUIRE(((size_t)obs_depth & (item - 1)) == 0 && ((size_t)pred_depth & (item - 1)) == 0 && ((size_t)verts & 3) == 0 &&
                      ((size_t)tris & 3) == 0 && ((size_t)tri_link & 3) == 0 && ((size_t)geom & 3) == 0 && ((size_t)norm_factor & 3) == 0 &&
                      ((size_t)pred_zbuf & 7) == 0 && ((size_t)scene & 7) == 0 && ((size_t)pred_render & 7) == 0 && ((size_t)params & 7) == 0 &&
                      ((size_t)pose_in & 7) == 0 && ((size_t)pose_out & 7) == 0 && ((size_t)best & 7) == 0 && ((size_t)sums & 7) == 0,
                  "refine_pass: the depth buffers must be aligned to their element, verts, tris, tri_link, geom and norm_factor 4-byte, "
                  "pred_zbuf, scene, pred_render, params, pose_in, pose_out, best and sums 8-byte aligned");
    ANCSH_REQUIRE(pose_in != pose_out, "refine_pass: pose_in and pose_out overlap (a workgroup reads its pose while another writes: two buffers)");
    if (nframes == 0) return ANCSH_OK;
    const dim3 grid(K, 2, nframes);
    if (depth_type == ANCSH_DEPTH_U16)
        hipLaunchKernelGGL(refine_pass_kernel<unsigned short>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, nframes, K, verts, tris, tri_link,
                           V, T, (const unsigned short *)obs_depth, obs_labels, pixel_capacity, pred_zbuf, (const unsigned short *)pred_depth,
                           pred_labels, geom, scene, pred_render, norm_factor, params, pass, is_last, pose_in, ld_in, pose_out, best, sums);
    else
        hipLaunchKernelGGL(refine_pass_kernel<float>, grid, dim3(RF_THREADS), 0, (hipStream_t)stream, nframes, K, verts, tris, tri_link, V, T,
                           (const float *)obs_depth, obs_labels, pixel_capacity, pred_zbuf, (const float *)pred_depth, pred_labels, geom, scene,
                           pred_render, norm_factor, params, pass, is_last, pose_in, ld_in, pose_out, best, sums);
    return check_launch("refine_pass");
}

extern "C" int ancsh_refine_rec(int nframes, int K, const double *best, const double *carried, int ld, double *wide, void *stream) {
    ANCSH_REQUIRE(nframes >= 0, "refine_rec: bad shape nframes=%d", nframes);
    ANCSH_REQUIRE(nframes <= 32767, "refine_rec: %d frames exceed the 32767-frame range of ancsh_refine_pass; split the batch", nframes);
    ANCSH_REQUIRE(K >= 1 && K <= 8, "refine_rec: K=%d must be in [1, 8]", K);
    ANCSH_REQUIRE(ld >= 26 && ld <= 4096, "refine_rec: ld=%d, a record row holds at least the 26 pose columns and at most 4096", ld);
    ANCSH_REQUIRE(best && carried && wide, "refine_rec: null pointer");
    ANCSH_REQUIRE(((size_t)best & 7) == 0 && ((size_t)carried & 7) == 0 && ((size_t)wide & 7) == 0,
                  "refine_rec: best, carried and wide must be 8-byte aligned");
    ANCSH_REQUIRE(carried != wide, "refine_rec: carried and wide overlap (the rows have different widths: wide is a buffer of its own)");
    if (nframes == 0) return ANCSH_OK;
    const long rows = (long)nframes * K, total = rows * (ld + RF_WIDTH);               // < 2^15 * 8 * 2^13 = 2^31
    hipLaunchKernelGGL(refine_rec_kernel, dim3((unsigned)((total + RF_THREADS - 1) / RF_THREADS)), dim3(RF_THREADS), 0, (hipStream_t)stream, rows,
                       best, carried, ld, wide);
    return check_launch("refine_rec");
}
