// reprojection.hip -- render-and-compare of a pose record (gfx950): the object's own mesh put where the fitted poses say, and the pixels of that
// predicted frame scored against the frame the annotation read.  Two entries around the unchanged renderer (include/ancsh_hip.h states both
// in full):
//   ancsh_reproject_scene_build : per frame its render table, scene table, rig, norm factor and the record's two poses per part -> two
//       render tables (baseline pose, nonlinear pose) and two geometry rows, which ancsh_render_depth_labels[_lib] renders as 2 * nframes
//       frames.  ONE launch, one thread per (frame, variant, link), as scene_build.hip's builder: the thread composes its link's five maps
//       and also copies value l of the head and of the geometry row.
//   ancsh_reproject_compare_rec : the observed crops and the two predicted crops -> 15 columns behind the carried record row: pixel counts,
//       silhouette IoU and depth residuals per part and pose.  ONE launch, one workgroup per (part, variant, frame): its threads stride the
//       crop, a thread's terms are added in pixel order, a wave's with shuffles in a fixed tree, the four waves' in wave order through LDS.
//       uint16 depths are summed as int64 quanta (exact in any order), float32 depths as float64 in that fixed order: no atomics, the same
//       bytes every run.
// float64 arithmetic evaluated as written (the library is built with -ffp-contract=off).  The compare kernel reads the crops pixel by pixel:
// K workgroups share a crop through the L2, and a crop is a few thousand pixels -- the launch sits near the floor of a dependent graph node.
#include "compare_common.h"

namespace ancsh {

constexpr int RP_LINKS = ANCSH_SCENE_MAX_LINKS, RP_THREADS = 256, RP_WIDTH = ANCSH_REPROJECTION_WIDTH;
constexpr int RP_RENDER = ANCSH_RENDER_WIDTH;

__global__ __launch_bounds__(RP_THREADS) void reproject_scene_build_kernel(int nframes, int K, const double *__restrict__ render,
                                                                           const double *__restrict__ scene, const double *__restrict__ rig,
                                                                           int rig_ld, const float *__restrict__ norm_factor,
                                                                           const double *__restrict__ record, int ld,
                                                                           const int *__restrict__ geom, long pixel_capacity,
                                                                           double *__restrict__ render_out, int *__restrict__ geom_out) {
    const int t = (int)(blockIdx.x * RP_THREADS + threadIdx.x), l = t % RP_LINKS, v = (t / RP_LINKS) & 1, f = t / (2 * RP_LINKS);
    if (f >= nframes) return;
    const double *rt = render + (size_t)f * RP_RENDER, *sc = scene + (size_t)f * AN_SCENE;
    const size_t row = (size_t)v * nframes + f;
    double *out = render_out + row * RP_RENDER;
    out[l] = rt[l];                                                     // the head, value l: bit for bit
    if (l < DEPTH_GEOM) {                                               // the geometry row, value l: the frame's own, in the variant's half
        int g = geom[(size_t)f * DEPTH_GEOM + l];
        if (l == 0 && g >= 0) {
            const long a = (long)g + (long)v * pixel_capacity;
            g = (int)(a < 0x7fffffffL ? a : 0x7fffffffL);               // a start beyond the buffers stays beyond them: the renderer refuses it
        }
        geom_out[row * DEPTH_GEOM + l] = g;
    }
    double *R = out + ANCSH_RENDER_HEAD + ANCSH_RENDER_LINK * l;
    const int nl = scene_nlinks(sc);
    if (l >= nl) {                                                      // a link the object does not have reads 0, as in the frame's own table
#pragma unroll
        for (int k = 0; k < ANCSH_RENDER_LINK; ++k) R[k] = 0.0;
        return;
    }
    const double nf = (double)norm_factor[f];
    const int j = scene_link_part(sc, l, nl, K);
    const double *pose = record + ((size_t)f * K + (j < 0 ? 0 : j)) * ld + 13 * v;
    if (j < 0 || !pose_ok(pose) || !finite(nf) || nf == 0.0) {          // the renderer drops a triangle whose vertex is not finite
        const double q = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < ANCSH_RENDER_LINK; ++k) R[k] = q;
        return;
    }
    predicted_link_map(rt, sc, rig + (size_t)f * rig_ld, K, l, j, pose, nf, R);      // steps 1..5: compare_common.h, shared with joint_values.hip
}

__device__ __forceinline__ long rp_quantum(unsigned short p, unsigned short o) { return (long)p - (long)o; }
__device__ __forceinline__ double rp_diff(float p, float o) { return (double)p - (double)o; }

template <typename V>
__device__ __forceinline__ V rp_block_sum(V v, V *s_red) {             // a fixed tree: xor shuffles, then the waves in order; uniform result
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    V t = s_red[0];
#pragma unroll
    for (int k = 1; k < RP_THREADS / 64; ++k) t += s_red[k];
    return t;
}

template <typename V>
__device__ __forceinline__ V rp_block_max(V v, V *s_red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const V u = __shfl_xor(v, o);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    V t = s_red[0];
#pragma unroll
    for (int k = 1; k < RP_THREADS / 64; ++k) t = s_red[k] > t ? s_red[k] : t;
    return t;
}

template <typename T>
__global__ __launch_bounds__(RP_THREADS) void reproject_compare_kernel(int K, const T *__restrict__ obs_depth,
                                                                       const unsigned char *__restrict__ obs_labels, long pixel_capacity,
                                                                       const T *__restrict__ pred_depth,
                                                                       const unsigned char *__restrict__ pred_labels,
                                                                       const int *__restrict__ geom, const double *__restrict__ scene,
                                                                       const double *__restrict__ carried, int ld, double *__restrict__ wide) {
    constexpr bool QUANTA = sizeof(T) == 2;
    __shared__ int s_part[RP_LINKS];
    __shared__ long s_li[RP_THREADS / 64];
    __shared__ double s_d[RP_THREADS / 64];
    const int j = blockIdx.x, v = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const double *sc = scene + (size_t)f * AN_SCENE;
    scene_part_table(sc, K, tid, s_part);
    const double *in = carried + ((size_t)f * K + j) * ld;
    double *out = wide + ((size_t)f * K + j) * (ld + RP_WIDTH);
    if (v == 0)
        for (int k = tid; k < ld; k += RP_THREADS) out[k] = in[k];      // the carried row, bit for bit
    __syncthreads();
    long start;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);       // [start, start + n) lies inside [0, pixel_capacity)
    const T *pd = pred_depth + (size_t)v * pixel_capacity;              // the variant's half of the predicted buffers, 2 * pixel_capacity long
    const unsigned char *pl = pred_labels + (size_t)v * pixel_capacity;
    long n_obs = 0, n_pred = 0, n_both = 0, q_abs = 0, q_sum = 0, q_sq = 0, q_max = 0;
    double d_abs = 0.0, d_sum = 0.0, d_sq = 0.0, d_max = 0.0;
    for (long a = start + tid; a < start + n; a += RP_THREADS) {
        const T od = obs_depth[a], qd = pd[a];
        const bool o = pixel_part(od, obs_labels[a], s_part) == j, p = pixel_part(qd, pl[a], s_part) == j;
        n_obs += o;
        n_pred += p;
        if (o && p) {
            ++n_both;
            if constexpr (QUANTA) {
                const long dq = rp_quantum(qd, od), m = dq < 0 ? -dq : dq;
                q_abs += m;
                q_sum += dq;
                q_sq += dq * dq;
                q_max = m > q_max ? m : q_max;
            } else {
                const double d = rp_diff(qd, od) * sc[6], m = fabs(d);
                d_abs += m;
                d_sum += d;
                d_sq += d * d;
                d_max = m > d_max ? m : d_max;
            }
        }
    }
    n_obs = rp_block_sum(n_obs, s_li);
    n_pred = rp_block_sum(n_pred, s_li);
    n_both = rp_block_sum(n_both, s_li);
    double mean_abs, rms, mx, mean;
    const double nb = (double)n_both, scale = sc[6];
    if constexpr (QUANTA) {
        q_abs = rp_block_sum(q_abs, s_li);
        q_sum = rp_block_sum(q_sum, s_li);
        q_sq = rp_block_sum(q_sq, s_li);
        q_max = rp_block_max(q_max, s_li);
        mean_abs = ((double)q_abs * scale) / nb;
        rms = sqrt((double)q_sq / nb) * scale;
        mx = (double)q_max * scale;
        mean = ((double)q_sum * scale) / nb;
    } else {
        d_abs = rp_block_sum(d_abs, s_d);
        d_sum = rp_block_sum(d_sum, s_d);
        d_sq = rp_block_sum(d_sq, s_d);
        d_max = rp_block_max(d_max, s_d);
        mean_abs = d_abs / nb;
        rms = sqrt(d_sq / nb);
        mx = d_max;
        mean = d_sum / nb;
    }
    if (tid == 0) {
        const double q = __builtin_nan("");
        const bool ok0 = pose_ok(in), ok1 = pose_ok(in + 13), ok = v == 0 ? ok0 : ok1;
        double *o = out + ld + 1 + 7 * v;
        if (v == 0) out[ld] = ok0 || ok1 ? (double)n_obs : q;
        const long uni = n_obs + n_pred - n_both;
        o[0] = ok ? (double)n_pred : q;
        o[1] = ok ? (double)n_both : q;
        o[2] = ok && uni > 0 ? nb / (double)uni : q;
        const bool dok = ok && n_both > 0;
        o[3] = dok ? mean_abs : q;
        o[4] = dok ? rms : q;
        o[5] = dok ? mx : q;
        o[6] = dok ? mean : q;
    }
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_reproject_scene_build(int nframes, int K, const double *render, const double *scene, const double *rig, int rig_ld,
                                           const float *norm_factor, const double *record, int ld, const int *geom, long pixel_capacity,
                                           double *render_out, int *geom_out, void *stream) {
    ANCSH_CHECK(batch_ok("reproject_scene_build", nframes, K, "give more than the 65535 predicted frames the renderer takes"));
    ANCSH_REQUIRE(rig_ld == ANCSH_RIG_WIDTH(K), "reproject_scene_build: rig_ld=%d, a rig of K=%d parts is %d wide", rig_ld, K, ANCSH_RIG_WIDTH(K));
    ANCSH_CHECK(record_ld_ok("reproject_scene_build", "ld", ld));
    ANCSH_CHECK(capacity_ok("reproject_scene_build", pixel_capacity));
    ANCSH_REQUIRE(render && scene && rig && norm_factor && record && geom && render_out && geom_out, "reproject_scene_build: null pointer");
    ANCSH_REQUIRE(all_aligned<8>(render, scene, rig, record, render_out) && all_aligned<4>(norm_factor, geom, geom_out), ANCSH_ALIGNED,
                  "reproject_scene_build");
    if (nframes == 0) return ANCSH_OK;
    const unsigned blocks = (unsigned)(((long)nframes * 2 * RP_LINKS + RP_THREADS - 1) / RP_THREADS);
    hipLaunchKernelGGL(reproject_scene_build_kernel, dim3(blocks), dim3(RP_THREADS), 0, (hipStream_t)stream, nframes, K, render, scene, rig,
                       rig_ld, norm_factor, record, ld, geom, pixel_capacity, render_out, geom_out);
    return check_launch("reproject_scene_build");
}

extern "C" int ancsh_reproject_compare_rec(int nframes, int K, int depth_type, const void *obs_depth, const unsigned char *obs_labels,
                                           long pixel_capacity, const void *pred_depth, const unsigned char *pred_labels, const int *geom,
                                           const double *scene, const double *carried, int ld, double *wide, void *stream) {
    ANCSH_CHECK(batch_ok("reproject_compare_rec", nframes, K, "exceed the 32767-frame range of ancsh_reproject_scene_build"));
    size_t item;
    ANCSH_CHECK(depth_item("reproject_compare_rec", depth_type, item));
    ANCSH_CHECK(capacity_ok("reproject_compare_rec", pixel_capacity));
    ANCSH_CHECK(record_ld_ok("reproject_compare_rec", "ld", ld));
    ANCSH_REQUIRE(obs_depth && obs_labels && pred_depth && pred_labels && geom && scene && carried && wide, "reproject_compare_rec: null pointer");
    ANCSH_REQUIRE(depth_aligned(item, obs_depth, pred_depth) && all_aligned<4>(geom) && all_aligned<8>(scene, carried, wide), ANCSH_ALIGNED,
                  "reproject_compare_rec");
    ANCSH_REQUIRE(carried != wide, "reproject_compare_rec: carried and wide overlap (the rows have different widths: wide is a buffer of its own)");
    if (nframes == 0) return ANCSH_OK;
    const dim3 grid(K, 2, nframes);
    if (depth_type == ANCSH_DEPTH_U16)
        hipLaunchKernelGGL(reproject_compare_kernel<unsigned short>, grid, dim3(RP_THREADS), 0, (hipStream_t)stream, K,
                           (const unsigned short *)obs_depth, obs_labels, pixel_capacity, (const unsigned short *)pred_depth, pred_labels, geom,
                           scene, carried, ld, wide);
    else
        hipLaunchKernelGGL(reproject_compare_kernel<float>, grid, dim3(RP_THREADS), 0, (hipStream_t)stream, K, (const float *)obs_depth,
                           obs_labels, pixel_capacity, (const float *)pred_depth, pred_labels, geom, scene, carried, ld, wide);
    return check_launch("reproject_compare_rec");
}
