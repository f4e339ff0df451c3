// pose.hip -- batched pose fitting for gfx950: per-part RANSAC similarity fit (stage A), per-joint
// RANSAC with articulated Levenberg-Marquardt refinement (stage B) and their full-inlier refits.  Part
// partitioning, joint-direction medians and Umeyama alignment are in pose_glue.hip.
//
// Reference (all host Python, one process per CPU core, ~10 s per cloud):
//   evaluation/parallel_ancsh_pose.py:20-33    ransac
//   evaluation/parallel_ancsh_pose.py:35-54    single_transformation_{estimator,verifier}
//   evaluation/parallel_ancsh_pose.py:56-68    objective_eval
//   evaluation/parallel_ancsh_pose.py:106-194  joint_transformation_{estimator,verifier}
//   lib/d3_utils.py:150-163,206-246            Rodrigues, Kabsch, transform_pts, scale_pts
//
// CDNA4 mapping (this is ALU/latency-bound work on <= 24 KB of points per part, not HBM-bound):
//   * hypotheses are the parallel axis: one lane = one hypothesis.  The part's points sit in LDS; every
//     lane walks the same point at the same time, so the verifier's LDS reads are broadcasts
//     (conflict-free) and its inner loop is pure VALU;
//   * the winner is chosen by a deterministic arg-max over the per-hypothesis score array (strictly
//     greater wins => earliest iteration on ties, as the reference's `>` at :28);
//   * refits run one workgroup per problem: masks, means, 3x3 moment sums and the O(n^2) pairwise
//     scale sums are block reductions over LDS-resident inliers; the big LM shares MINPACK's control
//     flow across the workgroup (every thread holds the same 6x6 system);
//   * sample indices are an INPUT (`draws`), so a run is reproducible against numpy's randint stream;
//     with draws == NULL a counter-based device generator (splitmix64 of seed/problem/iteration) is used.
#include "common.h"
#include "pose_math.h"
#include "umeyama_fit.h"
#include "pose_shared.h"

namespace ancsh {
namespace pose {

constexpr int MODEL_A = 13;   // R(9) s t(3)
constexpr int MODEL_B = 26;   // R0(9) s0 t0(3) R1(9) s1 t1(3)

// The generator key of a sampling kernel, by key mode KM:
//   KEY_VALUE (the by-value entries): `arg` is the key itself;
//   KEY_DSEED (the *_dseed entries): `arg` is the address of a uint64 in device memory, read here once per kernel -- a captured graph
//             then replays with whatever the host last wrote there -- plus `add` (1 in the stage-B kernels: the by-value caller passes
//             seed + 1 itself);
//   KEY_DKEY  (the *_dkey entries): `arg` is a DKey: the address of an ancsh_stream_key, whose seed is read as KEY_DSEED reads its
//             uint64, and the problems per cloud (K in stage A, K - 1 in stage B).  The generator's problem index is shifted by
//             key.cloud_base * parts (key_problem_base), so a cloud draws the samples of its GLOBAL index whichever launch serves it;
//             `prob` itself -- offsets, draws, scores, scratch, the record -- stays local.
// The two older modes keep their kernel argument (one uint64) and a problem base of constant 0: their code is unchanged.
enum { KEY_VALUE = 0, KEY_DSEED = 1, KEY_DKEY = 2 };
struct DKey {
    const ancsh_stream_key *key;
    int parts;
};
template <int KM> struct KeyArgT { typedef unsigned long long type; };
template <> struct KeyArgT<KEY_DKEY> { typedef DKey type; };
template <int KM> using KeyArg = typename KeyArgT<KM>::type;

template <int KM>
__device__ __forceinline__ unsigned long long kernel_seed(unsigned long long arg, unsigned add) {
    return KM != KEY_VALUE ? *(const unsigned long long *__restrict__)arg + add : arg;      // an ancsh_stream_key starts with its seed
}
template <int KM>
__device__ __forceinline__ unsigned long long kernel_seed(DKey arg, unsigned add) {
    return arg.key->seed + add;
}
template <int KM>
__device__ __forceinline__ int key_problem_base(unsigned long long) { return 0; }
template <int KM>
__device__ __forceinline__ int key_problem_base(DKey arg) { return arg.key->cloud_base * arg.parts; }

// ---- block reductions (256 threads = 4 waves): wave_sum and block_sum, umeyama_fit.h ----------------------

// ---- similarity model from a point set held as arrays (thread-local, tiny n) --------------------------
// transform_pts on 3 sampled points: Kabsch rotation, pairwise scale, mean translation.
__device__ __forceinline__ void estimate_single3(const float s[3][3], const float t[3][3], float R[9], float &scale,
                                                 float tr[3]) {
    double sm[3], tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sm[c] = ((double)s[0][c] + s[1][c] + s[2][c]) / 3.0;
        tm[c] = ((double)t[0][c] + t[1][c] + t[2][c]) / 3.0;
    }
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) M[a * 3 + b] += (t[i][a] - tm[a]) * (s[i][b] - sm[b]);
    double q[4], Rd[9];
    horn_quat_fast(M, q);
    quat_to_mat(q, Rd);
    double ab = 0.0, aa = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j) {
            double ds = 0.0, dt = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double u = (double)s[i][c] - s[j][c], v = (double)t[i][c] - t[j][c];
                ds += u * u;
                dt += v * v;
            }
            ab += 2.0 * sqrt(ds) * sqrt(dt);   // ordered pairs (i,j) and (j,i); i == j contributes 0
            aa += 2.0 * ds;
        }
    const double sc = ab / (aa + 1e-6);
    scale = (float)sc;
#pragma unroll
    for (int a = 0; a < 9; ++a) R[a] = (float)Rd[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            acc += (double)t[i][a] - (double)scale * (Rd[a * 3 + 0] * s[i][0] + Rd[a * 3 + 1] * s[i][1] + Rd[a * 3 + 2] * s[i][2]);
        tr[a] = (float)(acc / 3.0);
    }
}

// single_transformation_verifier for one point, float32 like the reference's numpy expression
// target - scale*matmul(rotation, source) - translation ; sqrt(sum(res^2)) < th
__device__ __forceinline__ float residual_sq_f32(const float R[9], float sc, const float tr[3], float sx, float sy, float sz,
                                                 float tx, float ty, float tz) {
#pragma clang fp contract(off)   // products and differences individually rounded, as numpy evaluates them
    const float rx = __builtin_fmaf(R[2], sz, __builtin_fmaf(R[1], sy, R[0] * sx));
    const float ry = __builtin_fmaf(R[5], sz, __builtin_fmaf(R[4], sy, R[3] * sx));
    const float rz = __builtin_fmaf(R[8], sz, __builtin_fmaf(R[7], sy, R[6] * sx));
    const float ex = (tx - sc * rx) - tr[0], ey = (ty - sc * ry) - tr[1], ez = (tz - sc * rz) - tr[2];
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ bool inlier_f32(const float R[9], float sc, const float tr[3], float sx, float sy, float sz,
                                           float tx, float ty, float tz, float th_sq) {
    // reference: sqrt(sum) < th in float32.  sqrt is monotone and correctly rounded, so this equals
    // sum < T with T = min{x : sqrtf(x) >= th} (sq_threshold_f32, computed once on the host): no sqrt per point.
    return residual_sq_f32(R, sc, tr, sx, sy, sz, tx, ty, tz) < th_sq;
}

// Optional extra outputs of the two finish kernels (round 5; every pointer may be null):
//   record (B, K, 26) float64 -- the pose record of evaluation/parallel_ancsh_pose.py:330-353 per part, [baseline R(9) s t(3) |
//     nonlinear R(9) s t(3)]: stage A's problem p = b * K + j fills columns 0..12 of row p (and 13..25 when K == 1: the reference's
//     nonlinear entry of a one-part object is its baseline), stage B's problem p = b * (K - 1) + q fills columns 13..25 of row
//     b * K + q + 1 (and, q == 0, of row b * K: part 0 is reported from joint 1's fit, :327-329) -- no assembly launches afterwards;
//   tie (nprob, 2) int32 -- how implementation-sensitive the fit is: [0] points of the part(s) whose residual norm under the WINNING
//     hypothesis lies within +-window of the threshold (the verifiers' `sqrt(sum(res**2)) < th`, :48-54,186-194: an implementation
//     whose model differs in the last bits may count such a point on the other side), [1] DEGENERATE CONTENDERS: hypotheses -- the
//     winner included -- whose score is within one inlier of the winning score and whose 3-point sample repeats an index
//     (np.random.randint draws with replacement, :38,110-111); stage A (round 6) counts only those that WOULD CHANGE THE CONSENSUS SET
//     (the winner itself, or a contender whose inlier mask differs from the winner's).  Such a sample's centred points are collinear, its 3 x 3 covariance has
//     rank 1, and the rotation the reference takes from np.linalg.svd is LAPACK's completion of a null space that rounding noise
//     selects: implementation-defined in the reference itself (include/ancsh_hip.h has the measured figures).
constexpr int TIE_MAX_CAND = 16;       // degenerate contenders (the lowest-numbered besides the winner) examined one by one in stage A's finish kernel
struct FitExtras {
    double *record;
    int K;
    int *tie;
    float lo_f, hi_f;        // stage A: squared-norm window [lo, hi)
    double lo_d, hi_d;       // stage B
    const int *draws;        // stage B: the sample streams (stage A's finish kernel already takes them)
    unsigned long long seed;
};

// the same predicate for two points at once on packed f32 (identical per-element roundings: every packed instruction
// is the IEEE operation applied to each half); returns how many of the two are inliers
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int inlier2_f32(const float R[9], float sc, const float tr[3], f32x2 sx, f32x2 sy, f32x2 sz,
                                           f32x2 tx, f32x2 ty, f32x2 tz, float th_sq) {
#pragma clang fp contract(off)
    const f32x2 rx = __builtin_elementwise_fma((f32x2)R[2], sz, __builtin_elementwise_fma((f32x2)R[1], sy, R[0] * sx));
    const f32x2 ry = __builtin_elementwise_fma((f32x2)R[5], sz, __builtin_elementwise_fma((f32x2)R[4], sy, R[3] * sx));
    const f32x2 rz = __builtin_elementwise_fma((f32x2)R[8], sz, __builtin_elementwise_fma((f32x2)R[7], sy, R[6] * sx));
    const f32x2 ex = (tx - sc * rx) - tr[0], ey = (ty - sc * ry) - tr[1], ez = (tz - sc * rz) - tr[2];
    const f32x2 s = (ex * ex + ey * ey) + ez * ez;
    return (s.x < th_sq ? 1 : 0) + (s.y < th_sq ? 1 : 0);
}

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pose.hip: the packed-f32 clamp counting (v_pk_mul_f32 ... clamp, DX10_CLAMP semantics) is written for gfx950 only"
#endif
// the same predicate, COUNTED on packed f32: cnt += (s < th ? 1.0f : 0.0f) per half, as  clamp((th - s) * 2^126)  -- one v_pk_fma_f32
// with the clamp modifier + v_pk_add_f32: two packed instructions per two points instead of two compares, two selects
// and an add with their VCC wait states.  Exact: th - s > 0 iff s < th (the difference of two distinct floats of this magnitude is
// never zero and far above the denormal range), any positive difference times 2^126 is >= 1, +inf (padding) and NaN clamp to 0
// (DX10_CLAMP), and the counts stay below 2^24.
__device__ __forceinline__ void inlier2_count_f32(const float R[9], float sc, const float tr[3], f32x2 sx, f32x2 sy, f32x2 sz,
                                                  f32x2 tx, f32x2 ty, f32x2 tz, float th_sq, f32x2 &cnt) {
#pragma clang fp contract(off)
    const f32x2 rx = __builtin_elementwise_fma((f32x2)R[2], sz, __builtin_elementwise_fma((f32x2)R[1], sy, R[0] * sx));
    const f32x2 ry = __builtin_elementwise_fma((f32x2)R[5], sz, __builtin_elementwise_fma((f32x2)R[4], sy, R[3] * sx));
    const f32x2 rz = __builtin_elementwise_fma((f32x2)R[8], sz, __builtin_elementwise_fma((f32x2)R[7], sy, R[6] * sx));
    const f32x2 ex = (tx - sc * rx) - tr[0], ey = (ty - sc * ry) - tr[1], ez = (tz - sc * rz) - tr[2];
    const f32x2 s = (ex * ex + ey * ey) + ez * ez;
    // one = clamp(fma(s, -2^126, th_sq * 2^126)): the fused product-sum is the exactly rounded (th_sq - s) * 2^126 (th_sq * 2^126 is exact
    // and finite for th_sq < 4, the launcher's guard), so its sign is that of th_sq - s without the separate subtraction
    const f32x2 nbig = {-0x1p126f, -0x1p126f};
    const f32x2 tbig = {th_sq * 0x1p126f, th_sq * 0x1p126f};
    f32x2 one;
    asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(one) : "v"(s), "v"(nbig), "v"(tbig));
    cnt = cnt + one;
}

__device__ __forceinline__ void load_draw3(const int *draws, unsigned long long seed, int prob, int kbase, int niter, int h, int k0,
                                           int stride, int n, int idx[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int v = draws ? draws[((size_t)prob * niter + h) * stride + k0 + k] : device_draw(seed, prob + kbase, h, k0 + k, n);
        idx[k] = v < 0 ? 0 : (v >= n ? n - 1 : v);
    }
}

// ================================ stage A ==========================================================
#ifndef A_CHUNK_N
#define A_CHUNK_N 2048
#endif
constexpr int A_CHUNK = A_CHUNK_N;   // points staged per LDS pass (24 B each)

template <int KM>
__global__ __launch_bounds__(256) void ransac_single_score_kernel(const int *__restrict__ off, const float *__restrict__ src,
                                                                  const float *__restrict__ tgt, float th, int niter,
                                                                  const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                                  int *__restrict__ scores) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 0);
    const int kbase = key_problem_base<KM>(seed_arg);
    // structure-of-arrays tile so that ds_read_b128 hands each lane 4 consecutive points per coordinate and the residual
    // arithmetic runs on packed-f32 (v_pk_mul/fma/add_f32: two points per lane per instruction)
    __shared__ __attribute__((aligned(16))) float pl[6][A_CHUNK];
    const int prob = blockIdx.y, h = blockIdx.x * 256 + threadIdx.x;
    const int r0 = off[prob], n = off[prob + 1] - r0;
    const bool live = h < niter && n > 0;
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sc = 0.f, tr[3] = {0, 0, 0};
    if (live) {
        int id[3];
        load_draw3(draws, seed, prob, kbase, niter, h, 0, 3, n, id);
        float s3[3][3], t3[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s3[i][c] = src[(size_t)(r0 + id[i]) * 3 + c];
                t3[i][c] = tgt[(size_t)(r0 + id[i]) * 3 + c];
            }
        estimate_single3(s3, t3, R, sc, tr);
    }
    int cnt = 0;
    for (int base = 0; base < n; base += A_CHUNK) {
        const int m = (n - base) < A_CHUNK ? (n - base) : A_CHUNK;
        const int m4 = (m + 3) & ~3;
        __syncthreads();
        for (int e = threadIdx.x; e < m4 * 3; e += 256) {
            const int i = e / 3, c = e - i * 3;
            const bool in = i < m;
            // rows past the part's end are padded with a point that can never be an inlier (target at +inf)
            pl[c][i] = in ? src[(size_t)(r0 + base) * 3 + e] : 0.f;
            pl[3 + c][i] = in ? tgt[(size_t)(r0 + base) * 3 + e] : __builtin_inff();
        }
        __syncthreads();
        if (live) {
            // software pipelined: the six ds_read_b128 of the NEXT four points are issued before the arithmetic on the current four,
            // so the LDS latency hides under ~50 packed instructions instead of being waited out at the top of every trip
            const float4 *px = (const float4 *)pl[0], *py = (const float4 *)pl[1], *pz = (const float4 *)pl[2];
            const float4 *pa = (const float4 *)pl[3], *pb = (const float4 *)pl[4], *pc = (const float4 *)pl[5];
            const int nq = m4 >> 2;
            auto score4 = [&](const float4 &x, const float4 &y, const float4 &z, const float4 &a, const float4 &b, const float4 &c) {
                cnt += inlier2_f32(R, sc, tr, f32x2{x.x, x.y}, f32x2{y.x, y.y}, f32x2{z.x, z.y}, f32x2{a.x, a.y}, f32x2{b.x, b.y},
                                   f32x2{c.x, c.y}, th);
                cnt += inlier2_f32(R, sc, tr, f32x2{x.z, x.w}, f32x2{y.z, y.w}, f32x2{z.z, z.w}, f32x2{a.z, a.w}, f32x2{b.z, b.w},
                                   f32x2{c.z, c.w}, th);
            };
            // two register sets in ping-pong (no copies): set 1 is read while set 0 is scored and vice versa; reads past the last
            // quad re-read it (loads stay unconditional), an odd last quad is scored once
            float4 x0 = px[0], y0 = py[0], z0 = pz[0], a0 = pa[0], b0 = pb[0], c0 = pc[0];
            for (int q = 0; q < nq; q += 2) {
                const int q1 = q + 1 < nq ? q + 1 : q, q2 = q + 2 < nq ? q + 2 : q1;
                const float4 x1 = px[q1], y1 = py[q1], z1 = pz[q1], a1 = pa[q1], b1 = pb[q1], c1 = pc[q1];
                __builtin_amdgcn_sched_barrier(0);              // keep the reads above the arithmetic (the scheduler sinks them to their use)
                score4(x0, y0, z0, a0, b0, c0);
                __builtin_amdgcn_sched_barrier(0);
                x0 = px[q2]; y0 = py[q2]; z0 = pz[q2]; a0 = pa[q2]; b0 = pb[q2]; c0 = pc[q2];
                __builtin_amdgcn_sched_barrier(0);
                if (q + 1 < nq) score4(x1, y1, z1, a1, b1, c1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (h < niter) scores[(size_t)prob * niter + h] = cnt;
}

// ---- the same scores with the part's points in SCALAR registers ------------------------------------------------------------
// Every lane of a wave tests the SAME point (lane = hypothesis), so the points are wave-uniform operands: they are read with
// scalar loads (s_load_dwordx8 through the scalar cache) from a "quad" copy of the part -- four points per 96-byte record
// {x[4], y[4], z[4]} of the source, {x[4], y[4], z[4]} of the target, so that two neighbouring points form an aligned SGPR pair =
// one packed-f32 operand -- and enter v_pk_mul/fma/add_f32 as the instruction's single scalar source.  No LDS, no barrier, no
// staging pass per workgroup; the kernel is pure vector-ALU work.
// part p starts at quad 2 * (ceil(off[p] / 8) + p): parts never overlap and each owns an even number of quads
__device__ __forceinline__ int quad_start(int r0, int prob) { return 2 * ((r0 + 7) / 8 + prob); }

__global__ __launch_bounds__(256) void soa_quads_kernel(const int *__restrict__ off, const float *__restrict__ src,
                                                        const float *__restrict__ tgt, float *__restrict__ quads, int cap_quads) {
    const int prob = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int r0 = off[prob], n = off[prob + 1] - r0;
    if (i >= ((n + 7) & ~7)) return;           // whole PAIRS of quads: the scoring loop takes two quads per trip, unconditionally
    if (quad_start(r0, prob) + (i >> 2) >= cap_quads) return;
    float *q = quads + ((size_t)quad_start(r0, prob) + (i >> 2)) * 24 + (i & 3);
    const bool in = i < n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[c * 4] = in ? src[(size_t)(r0 + i) * 3 + c] : 0.f;
        q[12 + c * 4] = in ? tgt[(size_t)(r0 + i) * 3 + c] : __builtin_inff();      // padding: a point that is never an inlier
    }
}

#ifndef POSE_SCORE_WAVES
#define POSE_SCORE_WAVES 0          /* experiment: > 0 caps the scoring kernel's registers at 512 / POSE_SCORE_WAVES per lane so that its waves fit NEXT TO resident SA waves */
#endif
#if POSE_SCORE_WAVES > 0
#define POSE_SCORE_ATTR __attribute__((amdgpu_waves_per_eu(POSE_SCORE_WAVES)))
#else
#define POSE_SCORE_ATTR
#endif
template <int KM>
__global__ __launch_bounds__(256) POSE_SCORE_ATTR void ransac_single_score_sreg_kernel(const int *__restrict__ off, const float *__restrict__ src,
                                                                       const float *__restrict__ tgt, const float *__restrict__ quads,
                                                                       int cap_quads, float th, int niter, const int *__restrict__ draws,
                                                                       KeyArg<KM> seed_arg, int *__restrict__ scores) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 0);
    const int kbase = key_problem_base<KM>(seed_arg);
    const int prob = blockIdx.y, h = blockIdx.x * 256 + threadIdx.x;
    const int r0 = off[prob], n = off[prob + 1] - r0;
    // lanes without a hypothesis (past niter) score the identity model and drop the result: no divergence inside the point loop
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sc = 0.f, tr[3] = {0, 0, 0};
    if (h < niter && n > 0) {
        int id[3];
        load_draw3(draws, seed, prob, kbase, niter, h, 0, 3, n, id);
        float s3[3][3], t3[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s3[i][c] = src[(size_t)(r0 + id[i]) * 3 + c];
                t3[i][c] = tgt[(size_t)(r0 + id[i]) * 3 + c];
            }
        estimate_single3(s3, t3, R, sc, tr);
    }
    typedef float f32x8 __attribute__((ext_vector_type(8)));
    const int q0 = quad_start(r0, prob);
    const f32x8 *Q = reinterpret_cast<const f32x8 *>(quads + (size_t)q0 * 24);
    int nq = ((n + 7) >> 3) * 2;                       // even: the part's copy is padded to whole quad pairs
    nq = min(nq, (cap_quads - q0) & ~1);               // never past the caller's buffer (a capacity the caller got wrong)
    f32x2 cnt2 = {0.f, 0.f};                           // inlier counts of the even / odd points (exact small integers)
    auto score4 = [&](const f32x8 &v0, const f32x8 &v1, const f32x8 &v2) {      // x0..3 y0..3 | z0..3 a0..3 | b0..3 c0..3
        inlier2_count_f32(R, sc, tr, f32x2{v0[0], v0[1]}, f32x2{v0[4], v0[5]}, f32x2{v1[0], v1[1]}, f32x2{v1[4], v1[5]},
                          f32x2{v2[0], v2[1]}, f32x2{v2[4], v2[5]}, th, cnt2);
        inlier2_count_f32(R, sc, tr, f32x2{v0[2], v0[3]}, f32x2{v0[6], v0[7]}, f32x2{v1[2], v1[3]}, f32x2{v1[6], v1[7]},
                          f32x2{v2[2], v2[3]}, f32x2{v2[6], v2[7]}, th, cnt2);
    };
    // two SGPR sets in ping-pong.  Scalar loads return out of order, so the only wait there is is lgkmcnt(0) = "everything issued
    // so far": each trip is  issue(next) ; score(current, which arrived before that issue) ; wait  -- the wait sits AFTER the
    // arithmetic, where the load it covers has had a whole score4 (~220 clocks) to come back from the scalar cache.  The read
    // past the last pair re-reads it (loads stay unconditional).
    constexpr int LGKM0 = 0xC07F;                      // s_waitcnt lgkmcnt(0), vmcnt / expcnt untouched
    if (nq > 0) {
        f32x8 a0 = Q[0], a1 = Q[1], a2 = Q[2];
        __builtin_amdgcn_s_waitcnt(LGKM0);
        for (int q = 0; q < nq; q += 2) {
            const int q2 = q + 2 < nq ? q + 2 : q;
            const f32x8 b0 = Q[q * 3 + 3], b1 = Q[q * 3 + 4], b2 = Q[q * 3 + 5];
            __builtin_amdgcn_sched_barrier(0);
            score4(a0, a1, a2);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(LGKM0);
            a0 = Q[q2 * 3]; a1 = Q[q2 * 3 + 1]; a2 = Q[q2 * 3 + 2];
            __builtin_amdgcn_sched_barrier(0);
            score4(b0, b1, b2);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(LGKM0);
        }
    }
    if (h < niter) scores[(size_t)prob * niter + h] = n > 0 ? (int)(cnt2.x + cnt2.y) : 0;
}

// arg-max with earliest-iteration tie-break over a score array, whole workgroup; result broadcast.
template <class T>
__device__ __forceinline__ int block_argmax_first(const T *sc, int niter, T *best_out, void *lds) {
    T bv = (T)-1;
    int bi = 0x7fffffff;
    for (int h = threadIdx.x; h < niter; h += blockDim.x) {
        const T v = sc[h];
        if (v > bv) { bv = v; bi = h; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    T *rv = (T *)lds;
    int *ri = (int *)(rv + 8);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) { rv[wave] = bv; ri[wave] = bi; }
    __syncthreads();
    bv = rv[0]; bi = ri[0];
    for (int w = 1; w < nw; ++w)
        if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
    __syncthreads();
    *best_out = bv;
    return bi;
}

// scale_pts' pair sums (lib/d3_utils.py:237-246) over the n LDS-resident points: A_ij = |s_i - s_j|, b_ij = |t_i - t_j| in
// FLOAT32 as numpy evaluates them on its float32 arrays ((dx^2 + dy^2) + dz^2, then sqrt; v_sqrt_f32 is within 1 ulp).
//   pr[0] += sum A*b, pr[1] += sum A*A, pr[2] += sum b*b   over all ordered pairs (i, j).
// Decomposition: wave w owns the column segment j in [w*seg, (w+1)*seg), lane l the rows l, l+64, ...: the j loop and its
// LDS addresses are WAVE-UNIFORM (scalar loop, broadcast reads), every thread does ~n*n/256 pairs.  A row segment (<= ~128
// terms of O(1)) is summed in float32 -- the reference sums all n^2 terms in float32 (sdot) -- and row segments in float64.
// Was: every thread one full row in float64 with an IEEE double sqrt per pair, 1.33 rows per thread on average but 2 for the
// slowest: 164 of the single-part refit kernel's 195 us.
__device__ __forceinline__ void pair_sums(const float (*cs)[3], const float (*ct)[3], int n, double (&pr)[3]) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int seg = (n + nw - 1) / nw;
    const int j0 = wave * seg, j1 = min(n, j0 + seg);
    constexpr int RB = 6;                              // rows a lane keeps in registers per pass: one LDS read of point j feeds RB pairs
    for (int ib = lane; ib < n; ib += 64 * RB) {
        float sx[RB], sy[RB], sz[RB], tx[RB], ty[RB], tz[RB], ab[RB], aa[RB], bb[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = min(ib + 64 * r, n - 1);     // rows past the end are computed on a clamped copy and dropped below
            sx[r] = cs[i][0]; sy[r] = cs[i][1]; sz[r] = cs[i][2];
            tx[r] = ct[i][0]; ty[r] = ct[i][1]; tz[r] = ct[i][2];
            ab[r] = aa[r] = bb[r] = 0.f;
        }
        for (int j = j0; j < j1; ++j) {
            const float cx = cs[j][0], cy = cs[j][1], cz = cs[j][2], dx = ct[j][0], dy = ct[j][1], dz = ct[j][2];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float ux = sx[r] - cx, uy = sy[r] - cy, uz = sz[r] - cz;
                const float vx = tx[r] - dx, vy = ty[r] - dy, vz = tz[r] - dz;
                const float A = __builtin_amdgcn_sqrtf((ux * ux + uy * uy) + uz * uz);
                const float b = __builtin_amdgcn_sqrtf((vx * vx + vy * vy) + vz * vz);
                ab[r] += A * b;
                aa[r] += A * A;
                bb[r] += b * b;
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (ib + 64 * r < n) { pr[0] += (double)ab[r]; pr[1] += (double)aa[r]; pr[2] += (double)bb[r]; }
    }
}

// Full-inlier similarity refit of inliers compacted in LDS (cs/ct: n_in x 3 floats): transform_pts.
// Every thread returns the same model.  red: >= 16*4 doubles of LDS.
__device__ __forceinline__ void refit_similarity(const float (*cs)[3], const float (*ct)[3], int n_in, double *red,
                                                 double R[9], double &scale, double tr[3]) {
    double sums[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n_in; i += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { sums[c] += cs[i][c]; sums[3 + c] += ct[i][c]; }
    }
    block_sum<6>(sums, red, 4);
    double sm[3], tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { sm[c] = sums[c] / n_in; tm[c] = sums[3 + c] / n_in; }
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n_in; i += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) M[a * 3 + b] += (ct[i][a] - tm[a]) * (cs[i][b] - sm[b]);
    block_sum<9>(M, red, 4);
    double q[4];
    horn_quat(M, q);
    quat_to_mat(q, R);
    double pr[3] = {0, 0, 0};   // sum A*b, sum A*A (, sum b*b) over ordered pairs
    pair_sums(cs, ct, n_in, pr);
    block_sum<3>(pr, red, 4);
    scale = pr[0] / (pr[1] + 1e-6);
    const double sf = (double)(float)scale;   // the reference's scale is a float32 (float32 inputs)
#pragma unroll
    for (int a = 0; a < 3; ++a) tr[a] = tm[a] - sf * (R[a * 3 + 0] * sm[0] + R[a * 3 + 1] * sm[1] + R[a * 3 + 2] * sm[2]);
}

// ordered compaction of flagged points into LDS arrays; returns the count (uniform).
__device__ __forceinline__ int compact_flagged(bool flag, int i, int n, const float *src, const float *tgt, size_t row0,
                                               float (*cs)[3], float (*ct)[3], int base, int *wcnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int start = base;
    for (int w = 0; w < wave; ++w) start += wcnt[w];
    const int total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (flag) {
        const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cs[pos][c] = src[(row0 + i) * 3 + c];
            ct[pos][c] = tgt[(row0 + i) * 3 + c];
        }
    }
    return base + total;
}

// Stage A's refit of problem `prob` by one 256-thread workgroup (smem: the launch's dynamic LDS, single_finish_lds(max_n) bytes).  A
// device function of (problem index, arguments) so that two kernels can run it: ransac_single_finish_kernel below (prob = blockIdx.x)
// and pose_lm_finish_a_kernel, whose blocks behind the LM fits take one part each.  Every branch around a barrier is block-uniform.
template <int KM>
__device__ __forceinline__ void ransac_single_finish_run(int prob, unsigned char *smem, const int *__restrict__ off,
                                                         const float *__restrict__ src, const float *__restrict__ tgt, float th, int niter,
                                                         const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                         const int *__restrict__ scores, int max_n, double *__restrict__ out_model,
                                                         unsigned char *__restrict__ out_inliers, int *__restrict__ out_best,
                                                         const FitExtras &E) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 0);
    const int kbase = key_problem_base<KM>(seed_arg);
    double *red = (double *)smem;                       // 64 doubles
    int *wcnt = (int *)(red + 64);                      // 4 ints for compact_flagged + 4 for the tie counts
    float(*cs)[3] = (float(*)[3])(wcnt + 8);
    float(*ct)[3] = cs + max_n;
    const int r0 = off[prob], n = off[prob + 1] - r0;
    double *om = out_model + (size_t)prob * MODEL_A;
    if (n <= 0 || n > max_n) {   // empty part: the reference raises (randint(0)); report instead of dying
        if (threadIdx.x < MODEL_A) om[threadIdx.x] = NAN;
        if (E.record && threadIdx.x < (E.K == 1 ? 2 * MODEL_A : MODEL_A)) E.record[(size_t)prob * 26 + threadIdx.x] = NAN;
        if (E.tie && threadIdx.x < 2) E.tie[prob * 2 + threadIdx.x] = 0;
        if (threadIdx.x == 0) { out_best[prob * 2] = -1; out_best[prob * 2 + 1] = n <= 0 ? 0 : -2; }
        for (int i = threadIdx.x; i < n; i += 256) out_inliers[r0 + i] = 0;      // every row's flag is written by this kernel
        return;
    }
    int best_score;
    const int best = block_argmax_first<int>(scores + (size_t)prob * niter, niter, &best_score, red);
    // re-derive the winning hypothesis (same device function => same bits as when it was scored)
    int id[3];
    load_draw3(draws, seed, prob, kbase, niter, best, 0, 3, n, id);
    float s3[3][3], t3[3][3], R[9], sc, tr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s3[i][c] = src[(size_t)(r0 + id[i]) * 3 + c];
            t3[i][c] = tgt[(size_t)(r0 + id[i]) * 3 + c];
        }
    estimate_single3(s3, t3, R, sc, tr);
    int n_in = 0, n_border = 0, n_near = 0;             // the tie counts: per-wave partial sums (wave-uniform)
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        bool f = false, border = false;
        if (i < n) {
            const float *ps = src + (size_t)(r0 + i) * 3, *pt = tgt + (size_t)(r0 + i) * 3;
            const float rs = residual_sq_f32(R, sc, tr, ps[0], ps[1], ps[2], pt[0], pt[1], pt[2]);
            f = rs < th;
            border = rs >= E.lo_f && rs < E.hi_f;
            out_inliers[r0 + i] = f ? 1 : 0;
        }
        n_border += __popcll(__ballot(border));
        n_in = compact_flagged(f, i, n, src, tgt, (size_t)r0, cs, ct, n_in, wcnt);
    }
    if (E.tie) {                                        // block-uniform
        // [1]: degenerate contenders (repeated-index sample, score within one inlier of the winner's) THAT WOULD CHANGE THE CONSENSUS SET:
        // the winner itself when its sample is degenerate, and every other such hypothesis whose inlier mask differs from the winner's
        // in at least one point.  (Round 5 counted every degenerate contender: 24.5 % of the fits at N = 1024, almost all of them
        // hypotheses with the winner's own mask, which cannot change the refit whoever scores them.)
        // The winner's degeneracy comes from its own sample (id[], block-uniform) and the winner never takes a slot; the slots go to the
        // LOWEST-NUMBERED other contenders, found by an ordered compaction per 256-hypothesis step (ballot + mbcnt prefix within a wave,
        // the four wave counts through LDS), so the sign is exact and the count does not depend on which lanes ran first.
        const bool winner_degenerate = id[0] == id[1] || id[0] == id[2] || id[1] == id[2];
        __shared__ int s_cand[TIE_MAX_CAND];
        const int *sp = scores + (size_t)prob * niter;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        int found = 0;                                  // other contenders below the current step (block-uniform)
        for (int h0 = 0; h0 < niter; h0 += 256) {       // block-uniform trip count
            const int h = h0 + threadIdx.x;
            bool cand = false;
            if (h < niter && h != best && sp[h] >= best_score - 1) {
                int d3[3];
                load_draw3(draws, seed, prob, kbase, niter, h, 0, 3, n, d3);
                cand = d3[0] == d3[1] || d3[0] == d3[2] || d3[1] == d3[2];
            }
            const unsigned long long m = __ballot(cand);
            __syncthreads();                            // every thread is done reading wcnt[0..3] (previous step / compact_flagged)
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int start = found;
            for (int w = 0; w < wave; ++w) start += wcnt[w];
            if (cand) {
                const int slot = start + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                if (slot < TIE_MAX_CAND) s_cand[slot] = h;
            }
            found += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        }
        __syncthreads();
        const int ncand = found < TIE_MAX_CAND ? found : TIE_MAX_CAND;
        n_near = found - ncand + (winner_degenerate ? 1 : 0);   // contenders beyond the slots counted as changing (conservative)
        for (int c = 0; c < ncand; ++c) {               // block-uniform trip count
            const int h = s_cand[c];
            int d3[3];
            load_draw3(draws, seed, prob, kbase, niter, h, 0, 3, n, d3);
            float hs[3][3], ht[3][3], hR[9], hsc, htr[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    hs[i][cc] = src[(size_t)(r0 + d3[i]) * 3 + cc];
                    ht[i][cc] = tgt[(size_t)(r0 + d3[i]) * 3 + cc];
                }
            estimate_single3(hs, ht, hR, hsc, htr);
            int differs = 0;
            for (int i = threadIdx.x; i < n; i += 256) {          // the same thread wrote out_inliers[r0 + i] above
                const float *ps = src + (size_t)(r0 + i) * 3, *pt = tgt + (size_t)(r0 + i) * 3;
                const bool f = residual_sq_f32(hR, hsc, htr, ps[0], ps[1], ps[2], pt[0], pt[1], pt[2]) < th;
                differs |= (int)(f != (out_inliers[r0 + i] != 0));
            }
            n_near += __syncthreads_or(differs) ? 1 : 0;
        }
        if ((threadIdx.x & 63) == 0) wcnt[4 + (threadIdx.x >> 6)] = n_border;
        __syncthreads();
        if (threadIdx.x == 0) {
            E.tie[prob * 2] = wcnt[4] + wcnt[5] + wcnt[6] + wcnt[7];
            // NEGATIVE when the winner's own sample is degenerate: that fit's consensus set is implementation-defined for certain
            // (r06_pose_tie_rate_K3.txt: 3 fits of 624, all 3 on another set than the reference arithmetic), where a positive count
            // only says that a degenerate hypothesis came close (22.9 % of the fits, 1 flip among them)
            E.tie[prob * 2 + 1] = winner_degenerate ? -n_near : n_near;               // block-uniform by construction
        }
    }
    __syncthreads();
    double Rd[9], scale, trd[3];
    if (n_in > 0) {
        refit_similarity(cs, ct, n_in, red, Rd, scale, trd);
    } else {
#pragma unroll
        for (int a = 0; a < 9; ++a) Rd[a] = NAN;
        scale = NAN; trd[0] = trd[1] = trd[2] = NAN;
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 9; ++a) om[a] = Rd[a];
        om[9] = (double)(float)scale;
#pragma unroll
        for (int a = 0; a < 3; ++a) om[10 + a] = trd[a];
        out_best[prob * 2] = best;
        out_best[prob * 2 + 1] = best_score;
        if (E.record) {
            double *rec = E.record + (size_t)prob * 26;
#pragma unroll
            for (int a = 0; a < MODEL_A; ++a) rec[a] = om[a];
            if (E.K == 1) {
#pragma unroll
                for (int a = 0; a < MODEL_A; ++a) rec[MODEL_A + a] = om[a];
            }
        }
    }
}

template <int KM>
__global__ __launch_bounds__(256) void ransac_single_finish_kernel(const int *__restrict__ off, const float *__restrict__ src,
                                                                   const float *__restrict__ tgt, float th, int niter,
                                                                   const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                                   const int *__restrict__ scores, int max_n,
                                                                   double *__restrict__ out_model,
                                                                   unsigned char *__restrict__ out_inliers,
                                                                   int *__restrict__ out_best, FitExtras E) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ransac_single_finish_run<KM>(blockIdx.x, smem, off, src, tgt, th, niter, draws, seed_arg, scores, max_n, out_model, out_inliers, out_best, E);
}

// ================================ stage B ==========================================================
// Forward-difference normal equations of the articulated objective (objective_eval, isweight=False):
//   residuals  y0_i - Rod(x0_i, r0)   (depend on params 0..2)
//              y1_i - Rod(x1_i, r1)   (depend on params 3..5)
//              wj x [Rod(J, r0) - Rod(J, r1)]   (all six)
// One `PartFd` handles one rotation vector: base rod + 3 perturbed rods (MINPACK's h_j = eps|x_j|), the
// 3x3 diagonal block of A = J^T J, its 3 entries of g = J^T f, and d Rod(J)/d r for the joint rows.
// Only one part is live at a time, which keeps a whole LM solve inside the VGPR budget.
struct PartFd {
    Rod b, p[3];
    double rh[3];
    double blk[6];     // packed symmetric 3x3 : (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
    double gv[3];
    double ju[3];      // Rod(J, r)
    double jd[3][3];   // jd[c][q] = (Rod(J, r + h_q e_q)[c] - Rod(J, r)[c]) / h_q

    // the point rows' half of begin(): all a prismatic problem needs (its constraint rows never rotate the joint direction)
    __device__ __forceinline__ void begin_points(const double r[3]) {
        b = rod_prepare(r[0], r[1], r[2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double h = fd_step(r[q]);
            rh[q] = fast_rcp(h);
            p[q] = rod_prepare(r[0] + (q == 0 ? h : 0.0), r[1] + (q == 1 ? h : 0.0), r[2] + (q == 2 ? h : 0.0));
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) blk[i] = 0.0;
        gv[0] = gv[1] = gv[2] = 0.0;
    }
    __device__ __forceinline__ void begin(const double r[3], const double J[3]) {
        begin_points(r);
        rod_apply(b, J[0], J[1], J[2], ju[0], ju[1], ju[2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            double qx, qy, qz;
            rod_apply(p[q], J[0], J[1], J[2], qx, qy, qz);
            jd[0][q] = qx; jd[1][q] = qy; jd[2][q] = qz;     // finished in joint_finish (needs f of the joint row)
        }
    }
    // one point row-triple: f = y - Rod(x, r); a[c][q] = ((y - Rod_q(x)) - f) / h_q
    __device__ __forceinline__ void point(double px, double py, double pz, double yx, double yy, double yz) {
        double ox, oy, oz;
        rod_apply(b, px, py, pz, ox, oy, oz);
        const double f0 = yx - ox, f1 = yy - oy, f2 = yz - oz;
        double a[3][3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            double qx, qy, qz;
            rod_apply(p[q], px, py, pz, qx, qy, qz);
            a[0][q] = ((yx - qx) - f0) * rh[q];
            a[1][q] = ((yy - qy) - f1) * rh[q];
            a[2][q] = ((yz - qz) - f2) * rh[q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int r = 0; r <= q; ++r) blk[q * (q + 1) / 2 + r] += a[0][q] * a[0][r] + a[1][q] * a[1][r] + a[2][q] * a[2][r];
            gv[q] += a[0][q] * f0 + a[1][q] * f1 + a[2][q] * f2;
        }
    }
};

// combine the two parts and the joint rows into the packed 6x6 system
__device__ __forceinline__ void assemble_normal(const PartFd &p0, const double blk0[6], const double g0[3], const PartFd &p1,
                                                const double blk1[6], const double g1[3], double wj, double A[21], double g[6]) {
    // joint rows: f = u - w ; d f/d r0_q = (Rod_q(J; r0) - w - f)/h = (jd0 - u)/h ; d f/d r1_q = (u - Rod_q(J; r1) - f)/h = (w - jd1)/h
    double f[3], a[3][6];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = p0.ju[c] - p1.ju[c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            a[c][q] = (((p0.jd[c][q] - p1.ju[c]) - f[c])) * p0.rh[q];
            a[c][3 + q] = (((p0.ju[c] - p1.jd[c][q]) - f[c])) * p1.rh[q];
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double v = wj * (a[0][i] * a[0][j] + a[1][i] * a[1][j] + a[2][i] * a[2][j]);
            if (i < 3) v += blk0[i * (i + 1) / 2 + j];
            else if (j >= 3) v += blk1[(i - 3) * (i - 2) / 2 + (j - 3)];
            A[i * (i + 1) / 2 + j] = v;
        }
        g[i] = wj * (a[0][i] * f[0] + a[1][i] * f[1] + a[2][i] * f[2]) + (i < 3 ? g0[i] : g1[i - 3]);
    }
}

// ---- the prismatic objective (objective_eval_r, :70-81, isweight=False) -------------------------------------------------------------
// The point rows are the revolute problem's; the wj joint rows give way to THREE rows r0 - r1 of weight 1: a slider does not turn
// against its base at all.  The joint direction does not enter (a NaN direction is never read).  The rows' Jacobian is the forward
// difference MINPACK forms, not the constants +-1: row c moves only with r0_c and r1_c,
//   d0[c] = (((r0_c + h0_c) - r1_c) - f_c) / h0_c,   d1[c] = ((r0_c - (r1_c + h1_c)) - f_c) / h1_c,   f_c = r0_c - r1_c,
// (every other entry is (f_c - f_c) / h = 0 exactly), with the steps and reciprocals of the point rows (PartFd::begin_points).
__device__ __forceinline__ double prismatic_cost(const double x[6]) {
    const double a = x[0] - x[3], b = x[1] - x[4], c = x[2] - x[5];
    return a * a + b * b + c * c;
}
__device__ __forceinline__ void assemble_normal_prismatic(const double x[6], const double blk0[6], const double g0[3],
                                                          const double blk1[6], const double g1[3], double A[21], double g[6]) {
    double f[3], d0[3], d1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double h0 = fd_step(x[c]), h1 = fd_step(x[3 + c]);
        f[c] = x[c] - x[3 + c];
        d0[c] = (((x[c] + h0) - x[3 + c]) - f[c]) * fast_rcp(h0);
        d1[c] = ((x[c] - (x[3 + c] + h1)) - f[c]) * fast_rcp(h1);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            if (i < 3) v = (i == j ? d0[i] * d0[i] : 0.0) + blk0[i * (i + 1) / 2 + j];
            else if (j >= 3) v = (i == j ? d1[i - 3] * d1[i - 3] : 0.0) + blk1[(i - 3) * (i - 2) / 2 + (j - 3)];
            else if (i - 3 == j) v = d1[j] * d0[j];
            A[i * (i + 1) / 2 + j] = v;
        }
        g[i] = i < 3 ? d0[i] * f[i] + g0[i] : d1[i - 3] * f[i - 3] + g1[i - 3];
    }
}

// Thread-local articulated problem on 3 + 3 sampled points.  PRISM: the prismatic objective above (J, wj unused).
template <bool PRISM>
struct HypProblemT {
    double x0[3][3], y0[3][3], x1[3][3], y1[3][3], J[3], wj;

    __device__ __forceinline__ double cost(const double x[6]) const {
        const Rod r0 = rod_prepare(x[0], x[1], x[2]), r1 = rod_prepare(x[3], x[4], x[5]);
        double s = 0.0, ox, oy, oz;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            rod_apply(r0, x0[i][0], x0[i][1], x0[i][2], ox, oy, oz);
            const double a = y0[i][0] - ox, b = y0[i][1] - oy, c = y0[i][2] - oz;
            s += a * a + b * b + c * c;
            rod_apply(r1, x1[i][0], x1[i][1], x1[i][2], ox, oy, oz);
            const double d = y1[i][0] - ox, e = y1[i][1] - oy, f = y1[i][2] - oz;
            s += d * d + e * e + f * f;
        }
        if constexpr (PRISM) {
            return s + prismatic_cost(x);
        } else {
            double ux, uy, uz, wx, wy, wz;
            rod_apply(r0, J[0], J[1], J[2], ux, uy, uz);
            rod_apply(r1, J[0], J[1], J[2], wx, wy, wz);
            s += wj * ((ux - wx) * (ux - wx) + (uy - wy) * (uy - wy) + (uz - wz) * (uz - wz));
            return s;
        }
    }
    __device__ __forceinline__ void normal(const double x[6], double A[21], double g[6]) const {
        PartFd p0, p1;
        if constexpr (PRISM) p0.begin_points(x); else p0.begin(x, J);
#pragma unroll
        for (int i = 0; i < 3; ++i) p0.point(x0[i][0], x0[i][1], x0[i][2], y0[i][0], y0[i][1], y0[i][2]);
        if constexpr (PRISM) p1.begin_points(x + 3); else p1.begin(x + 3, J);
#pragma unroll
        for (int i = 0; i < 3; ++i) p1.point(x1[i][0], x1[i][1], x1[i][2], y1[i][0], y1[i][1], y1[i][2]);
        if constexpr (PRISM) assemble_normal_prismatic(x, p0.blk, p0.gv, p1.blk, p1.gv, A, g);
        else assemble_normal(p0, p0.blk, p0.gv, p1, p1.blk, p1.gv, wj, A, g);
    }
};
typedef HypProblemT<false> HypProblem;

// scale_pts both ways on 3 points: s = <A,b>/(<A,A>+1e-6), s_inv = <A,b>/(<b,b>+1e-6); float32 results
__device__ __forceinline__ void scales3(const float s[3][3], const float t[3][3], float &sc, float &sc_inv) {
    double ab = 0.0, aa = 0.0, bb = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j) {
            double ds = 0.0, dt = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double u = (double)s[i][c] - s[j][c], v = (double)t[i][c] - t[j][c];
                ds += u * u;
                dt += v * v;
            }
            ab += 2.0 * sqrt(ds) * sqrt(dt);
            aa += 2.0 * ds;
            bb += 2.0 * dt;
        }
    sc = (float)(ab / (aa + 1e-6));
    sc_inv = (float)(ab / (bb + 1e-6));
}

// centred source / pre-scaled centred target of 3 samples (float32 like the reference's arrays)
__device__ __forceinline__ void center_part3(const float s[3][3], const float t[3][3], float sc_inv, double xc[3][3],
                                             double yc[3][3]) {
    float sm[3], tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sm[c] = ((s[0][c] + s[1][c]) + s[2][c]) / 3.0f;
        tm[c] = ((sc_inv * t[0][c] + sc_inv * t[1][c]) + sc_inv * t[2][c]) / 3.0f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xc[i][c] = (double)(s[i][c] - sm[c]);
            yc[i][c] = (double)(sc_inv * t[i][c] - tm[c]);
        }
    }
}

// ... and the Kabsch rotation vector between them (the LM start point)
__device__ __forceinline__ void prep_part3(const float s[3][3], const float t[3][3], float sc_inv, double xc[3][3],
                                           double yc[3][3], double rv[3]) {
    center_part3(s, t, sc_inv, xc, yc);
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // rotate_pts re-centres its (already centred) inputs; the means are ~1e-8 and do not move R
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) M[a * 3 + b] += yc[i][a] * xc[i][b];
    double q[4];
    horn_quat_fast(M, q);
    quat_to_rotvec(q, rv);
}

// joint_transformation_verifier for one point (float64: the model rotation is float64 in the reference)
__device__ __forceinline__ double residual_sq_f64(const double R[9], double sc, const double tr[3], float sx, float sy, float sz,
                                                  float tx, float ty, float tz) {
    const double rx = R[0] * sx + R[1] * sy + R[2] * sz, ry = R[3] * sx + R[4] * sy + R[5] * sz,
                 rz = R[6] * sx + R[7] * sy + R[8] * sz;
    const double ex = ((double)tx - sc * rx) - tr[0], ey = ((double)ty - sc * ry) - tr[1], ez = ((double)tz - sc * rz) - tr[2];
    return ex * ex + ey * ey + ez * ez;
}
__device__ __forceinline__ bool inlier_f64(const double R[9], double sc, const double tr[3], float sx, float sy, float sz,
                                           float tx, float ty, float tz, double th) {
    return residual_sq_f64(R, sc, tr, sx, sy, sz, tx, ty, tz) < th;     // th = exact squared threshold (sq_threshold_f64)
}

// Stage B runs every hypothesis' articulated LM fit (joint_transformation_estimator, :106-184) as three kernels, because
// the fits' lengths are heavy-tailed (measured on the bench workload: mean 45 function evaluations, mean over waves of
// the slowest of 64 consecutive hypotheses 271, degenerate samples up to MINPACK's maxfev = 4200):
//   1. ransac_joint_init_kernel   (lock-step, thread per hypothesis): per-part scales + Kabsch start point -> models[0..9]
//   2. ransac_joint_lm_kernel     (one wave per HYP_CHUNK hypotheses): lanes run lm6_trip; a lane whose fit has terminated
//                                  takes the wave's next unstarted hypothesis, so SIMD time follows the SUM of the fit
//                                  lengths, not 64 x the slowest.  The order in which hypotheses run does not enter any
//                                  result (each is a function of its own draw only).
//   3. ransac_joint_model_kernel  (lock-step): rotations / translations of both parts from the fitted rotation vectors.
// Scratch layout per hypothesis (MODEL_B doubles) between the kernels: [0..5] rotation vectors, [6..7] 1/scale per part,
// [8..9] scale per part; kernel 3 overwrites the slot with the final model.
struct HypSamples {
    float s0[3][3], t0[3][3], s1[3][3], t1[3][3];
};
__device__ __forceinline__ void load_hyp_samples(const float *__restrict__ src, const float *__restrict__ tgt, const int *draws,
                                                 unsigned long long seed, int prob, int kbase, int niter, int h, int a0, int n0, int a1,
                                                 int n1, HypSamples &q) {
    int i0[3], i1[3];
    load_draw3(draws, seed, prob, kbase, niter, h, 0, 6, n0, i0);
    load_draw3(draws, seed, prob, kbase, niter, h, 3, 6, n1, i1);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            q.s0[i][c] = src[(size_t)(a0 + i0[i]) * 3 + c];
            q.t0[i][c] = tgt[(size_t)(a0 + i0[i]) * 3 + c];
            q.s1[i][c] = src[(size_t)(a1 + i1[i]) * 3 + c];
            q.t1[i][c] = tgt[(size_t)(a1 + i1[i]) * 3 + c];
        }
}

template <int KM>
__global__ __launch_bounds__(64) void ransac_joint_init_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                               const float *__restrict__ src, const float *__restrict__ tgt,
                                                               int niter, const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                               double *__restrict__ scores, double *__restrict__ models) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 1);
    const int kbase = key_problem_base<KM>(seed_arg);
    const int prob = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
    const int a0 = rng0[prob * 2], n0 = rng0[prob * 2 + 1] - a0;
    const int a1 = rng1[prob * 2], n1 = rng1[prob * 2 + 1] - a1;
    if (h >= niter) return;
    double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
    if (n0 <= 0 || n1 <= 0) {
        scores[(size_t)prob * niter + h] = -1.0;
        for (int i = 0; i < MODEL_B; ++i) mo[i] = NAN;
        return;
    }
    HypSamples q;
    load_hyp_samples(src, tgt, draws, seed, prob, kbase, niter, h, a0, n0, a1, n1, q);
    float sc0, sc0i, sc1, sc1i;
    scales3(q.s0, q.t0, sc0, sc0i);
    scales3(q.s1, q.t1, sc1, sc1i);
    double xc[3][3], yc[3][3], x[6];
    prep_part3(q.s0, q.t0, sc0i, xc, yc, x);
    prep_part3(q.s1, q.t1, sc1i, xc, yc, x + 3);
#pragma unroll
    for (int i = 0; i < 6; ++i) mo[i] = x[i];
    mo[6] = sc0i; mo[7] = sc1i; mo[8] = sc0; mo[9] = sc1;
}

constexpr int HYP_CHUNK = 256;    // hypotheses handed to one wave of a full launch
constexpr int HYP_CHUNK_SMALL = 64;   // ... of a launch too small to fill the chip with 256 per wave (scheduling only: same bits)
constexpr long HYP_SMALL_LAUNCH = 8192;   // fits per launch up to which the small chunk is used
constexpr int HYP_REFILL = 16;    // idle lanes that trigger a refill (a refill costs the whole wave ~1 trip of latency)

// The joint kind (0 revolute, non-zero prismatic) is a property of the problem, and prob = blockIdx.y (blockIdx.x in the finish
// kernel): every lane of a block runs the same objective.  Each LM kernel's body is therefore a function of <key mode, PRISM>; the
// kernels of the entries without a kind array instantiate PRISM = false alone (registers, scratch and occupancy as before kinds existed:
// profiles/r14_pose_resource_usage_{before,after,diff}.txt), and the *_kind_kernel twins take the block-uniform branch on joint_kind[prob].
template <int KM, bool PRISM>
__device__ __forceinline__ void ransac_joint_lm_run(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                    const float *__restrict__ src, const float *__restrict__ tgt,
                                                    const float *__restrict__ joint_dir, int niter,
                                                    const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                    double *__restrict__ models, int *__restrict__ lm_stat, int chunk, int prob,
                                                    int chunk_idx) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 1);
    const int kbase = key_problem_base<KM>(seed_arg);
    const int a0 = rng0[prob * 2], n0 = rng0[prob * 2 + 1] - a0;
    const int a1 = rng1[prob * 2], n1 = rng1[prob * 2 + 1] - a1;
    if (n0 <= 0 || n1 <= 0) return;
    const int c1 = min(niter, (chunk_idx + 1) * chunk);
    int next = chunk_idx * chunk;               // wave-uniform: first hypothesis of the chunk not yet handed out
    HypProblemT<PRISM> P;
    if constexpr (!PRISM) {
        P.J[0] = joint_dir[prob * 3]; P.J[1] = joint_dir[prob * 3 + 1]; P.J[2] = joint_dir[prob * 3 + 2];
        P.wj = 3.0;   // min(3,3) copies of the joint axis (:134)
    }
    Lm6 S;
    bool active = false;
    int h = 0;
    for (;;) {
        const unsigned long long idle = __ballot(!active);
        const int n_idle = __popcll(idle);
        if (next < c1 && (n_idle >= HYP_REFILL || n_idle >= c1 - next || n_idle == 64)) {
            if (!active) {
                const int mine = next + __builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0));
                if (mine < c1) {
                    h = mine;
                    const double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
                    HypSamples q;
                    load_hyp_samples(src, tgt, draws, seed, prob, kbase, niter, h, a0, n0, a1, n1, q);
                    center_part3(q.s0, q.t0, (float)mo[6], P.x0, P.y0);
                    center_part3(q.s1, q.t1, (float)mo[7], P.x1, P.y1);
#pragma unroll
                    for (int i = 0; i < 6; ++i) S.x[i] = mo[i];
                    lm6_begin(P, S);
                    active = true;
                }
            }
            next += n_idle;
        } else if (n_idle == 64) {
            break;
        }
        if (active && lm6_trip(P, S, 1e-4, 1e-8, 1e-8, 4200)) {
            double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
#pragma unroll
            for (int i = 0; i < 6; ++i) mo[i] = S.x[i];
#ifdef LM_COUNT
            if (lm_stat) { lm_stat[((size_t)prob * niter + h) * 2] = S.info | (S.trips << 4) | (S.nchol << 17); lm_stat[((size_t)prob * niter + h) * 2 + 1] = S.nfev; }
#else
            if (lm_stat) { lm_stat[((size_t)prob * niter + h) * 2] = S.info; lm_stat[((size_t)prob * niter + h) * 2 + 1] = S.nfev; }
#endif
            active = false;
        }
    }
}

template <int KM>
__global__ __launch_bounds__(64) void ransac_joint_lm_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                             const float *__restrict__ src, const float *__restrict__ tgt,
                                                             const float *__restrict__ joint_dir, int niter,
                                                             const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                             double *__restrict__ models, int *__restrict__ lm_stat, int chunk) {
    ransac_joint_lm_run<KM, false>(rng0, rng1, src, tgt, joint_dir, niter, draws, seed_arg, models, lm_stat, chunk, blockIdx.y, blockIdx.x);
}

template <int KM>
__global__ __launch_bounds__(64) void ransac_joint_lm_kind_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                  const float *__restrict__ src, const float *__restrict__ tgt,
                                                                  const float *__restrict__ joint_dir, int niter,
                                                                  const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                                  double *__restrict__ models, int *__restrict__ lm_stat, int chunk,
                                                                  const int *__restrict__ joint_kind) {
    if (joint_kind[blockIdx.y] != 0) ransac_joint_lm_run<KM, true>(rng0, rng1, src, tgt, joint_dir, niter, draws, seed_arg, models, lm_stat, chunk, blockIdx.y, blockIdx.x);
    else ransac_joint_lm_run<KM, false>(rng0, rng1, src, tgt, joint_dir, niter, draws, seed_arg, models, lm_stat, chunk, blockIdx.y, blockIdx.x);
}

// ---- joint LM fits || stage A's refit in ONE launch ------------------------------------------------------------------------
// The LM launch is 64 waves of which all but one are gone after a fifth of its duration (the longest MINPACK trajectory sets it), and
// with few hardware queues a batch's launches run one after another on ONE in-order queue: whatever follows the LM kernel waits for its
// tail with the chip almost empty.  Stage A's refit (one 256-thread workgroup per part, indifferent to occupancy) shares nothing with
// stage B but the partition, so it rides in the same grid instead of holding the queue for a launch of its own:
//   blocks [0, n_lm)               : four waves, one LM chunk each -- chunk_id = blockIdx.x * 4 + wave, (prob, chunk in problem) =
//                                    (chunk_id / chunks_per_prob, chunk_id % chunks_per_prob); a wave past the last chunk returns.  The
//                                    LM code has no workgroup barrier and no LDS: waves are as independent as in ransac_joint_lm_kernel,
//                                    and a fit is a function of its own draw only, so the bytes are that kernel's;
//   blocks [n_lm, n_lm + nprob_a)  : ransac_single_finish_run of part blockIdx.x - n_lm (its scores come from the scoring launch that
//                                    precedes this one on the stream).
// LM blocks come first so the long pole starts at once.  The role test reads blockIdx.x alone: block-uniform, so the refit's barriers
// are safe.  Dynamic LDS is the refit's (the LM blocks ignore it).  Registers are the LM code's (one wave per SIMD either way).
struct LmArgs {
    const int *rng0, *rng1;
    const float *joint_dir;
    int niter;
    const int *draws;
    double *models;
    int *lm_stat;
    int chunk, chunks_per_prob, n_chunks, n_lm;
};
struct FinishAArgs {
    const int *off;
    float th;
    int niter;
    const int *draws, *scores;
    int max_n;
    double *out_model;
    unsigned char *out_inliers;
    int *out_best;
};

template <int KM, bool KIND>
__device__ __forceinline__ void pose_lm_finish_a_run(unsigned char *smem, const float *__restrict__ src, const float *__restrict__ tgt,
                                                     const LmArgs &L, KeyArg<KM> seed_b, const int *__restrict__ joint_kind,
                                                     const FinishAArgs &A, KeyArg<KM> seed_a, const FitExtras &EA) {
    if ((int)blockIdx.x >= L.n_lm) {                   // block-uniform
        ransac_single_finish_run<KM>((int)blockIdx.x - L.n_lm, smem, A.off, src, tgt, A.th, A.niter, A.draws, seed_a, A.scores, A.max_n,
                                     A.out_model, A.out_inliers, A.out_best, EA);
        return;
    }
    const int chunk_id = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
    if (chunk_id >= L.n_chunks) return;
    const int prob = chunk_id / L.chunks_per_prob, chunk_idx = chunk_id - prob * L.chunks_per_prob;
    if constexpr (KIND) {
        if (joint_kind[prob] != 0) {
            ransac_joint_lm_run<KM, true>(L.rng0, L.rng1, src, tgt, L.joint_dir, L.niter, L.draws, seed_b, L.models, L.lm_stat, L.chunk, prob, chunk_idx);
            return;
        }
    }
    ransac_joint_lm_run<KM, false>(L.rng0, L.rng1, src, tgt, L.joint_dir, L.niter, L.draws, seed_b, L.models, L.lm_stat, L.chunk, prob, chunk_idx);
}

template <int KM>
__global__ __launch_bounds__(256) void pose_lm_finish_a_kernel(const float *__restrict__ src, const float *__restrict__ tgt, LmArgs L,
                                                               KeyArg<KM> seed_b, FinishAArgs A, KeyArg<KM> seed_a, FitExtras EA) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    pose_lm_finish_a_run<KM, false>(smem, src, tgt, L, seed_b, nullptr, A, seed_a, EA);
}

template <int KM>
__global__ __launch_bounds__(256) void pose_lm_finish_a_kind_kernel(const float *__restrict__ src, const float *__restrict__ tgt, LmArgs L,
                                                                    KeyArg<KM> seed_b, const int *__restrict__ joint_kind, FinishAArgs A,
                                                                    KeyArg<KM> seed_a, FitExtras EA) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    pose_lm_finish_a_run<KM, true>(smem, src, tgt, L, seed_b, joint_kind, A, seed_a, EA);
}

// ---- lane-group-cooperative LM --------------------------------------------------------------------------------------------
// The kernel above keeps one fit in one lane: its duration is the LONGEST fit of the batch (1500-evaluation trajectories,
// ~1.6 ms), every one of its ~2000 instructions per evaluation issued for a single live lane.  Here EIGHT lanes share a fit.
// All eight hold the same Lm6 state and run the same MINPACK control flow (so no broadcast is ever needed and divergence only
// exists between groups); the two expensive callbacks are split across the group's lanes and recombined through a 0.9 KB
// group-private LDS record in a fixed order, so that every lane ends up with bit-identical A, g and cost:
//   normal(): role q8 = lane & 7 < 6 owns forward-difference column q8 (part q8 / 3, parameter q8 % 3): one perturbed
//             Rodrigues rotation instead of six, its 9 + 3 Jacobian entries; then every lane assembles the 6x6 system
//             from the six columns with the arithmetic of PartFd::point / assemble_normal above;
//   cost():   roles 0..5 own one (part, point) residual triple each, role 6 the joint-axis residual; the seven partial
//             sums are added in the serial order.
constexpr int COOP_G = 8;                 // lanes per fit
constexpr int COOP_XCH = 112;             // doubles per group record: col 54 | jd 18 | rh 6 | f 18 | ju 6 | cost 7
constexpr int COOP_HYP_PER_WAVE = 32;     // hypotheses handed to one wave (8 at a time, refilled)

__device__ __forceinline__ void group_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// PRISM (the prismatic objective, see assemble_normal_prismatic): role 6's share of cost() is the three constraint rows r0 - r1
// (weight 1), and normal() needs no jd / ju exchange -- the constraint rows' entries come from x, which every lane holds.  The group
// record keeps its layout and size; a prismatic fit simply leaves the jd, rh and ju slots unused (one record layout for both kinds,
// one 7 KB array per block handed in by the kernel).
template <bool PRISM>
struct HypProblemCoopT {
    double x0[3][3], y0[3][3], x1[3][3], y1[3][3], J[3], wj;
    double *xch;      // this group's LDS record
    int role;         // lane & 7

    __device__ __forceinline__ double cost(const double x[6]) const {
        // role -> (part, point): 0..2 = part 0, 3..5 = part 1, 6 / 7 = joint axis
        const bool joint = role >= 6;
        const bool p1 = role >= 3 && role < 6;
        const int i = joint ? 0 : (p1 ? role - 3 : role);
        double partial;
        if (!joint) {
            const Rod r = p1 ? rod_prepare(x[3], x[4], x[5]) : rod_prepare(x[0], x[1], x[2]);
            const double px = p1 ? (i == 0 ? x1[0][0] : i == 1 ? x1[1][0] : x1[2][0]) : (i == 0 ? x0[0][0] : i == 1 ? x0[1][0] : x0[2][0]);
            const double py = p1 ? (i == 0 ? x1[0][1] : i == 1 ? x1[1][1] : x1[2][1]) : (i == 0 ? x0[0][1] : i == 1 ? x0[1][1] : x0[2][1]);
            const double pz = p1 ? (i == 0 ? x1[0][2] : i == 1 ? x1[1][2] : x1[2][2]) : (i == 0 ? x0[0][2] : i == 1 ? x0[1][2] : x0[2][2]);
            const double tx = p1 ? (i == 0 ? y1[0][0] : i == 1 ? y1[1][0] : y1[2][0]) : (i == 0 ? y0[0][0] : i == 1 ? y0[1][0] : y0[2][0]);
            const double ty = p1 ? (i == 0 ? y1[0][1] : i == 1 ? y1[1][1] : y1[2][1]) : (i == 0 ? y0[0][1] : i == 1 ? y0[1][1] : y0[2][1]);
            const double tz = p1 ? (i == 0 ? y1[0][2] : i == 1 ? y1[1][2] : y1[2][2]) : (i == 0 ? y0[0][2] : i == 1 ? y0[1][2] : y0[2][2]);
            double ox, oy, oz;
            rod_apply(r, px, py, pz, ox, oy, oz);
            const double a = tx - ox, b = ty - oy, c = tz - oz;
            partial = a * a + b * b + c * c;
        } else if constexpr (PRISM) {
            partial = prismatic_cost(x);
        } else {
            const Rod r0 = rod_prepare(x[0], x[1], x[2]), r1 = rod_prepare(x[3], x[4], x[5]);
            double ux, uy, uz, wx, wy, wz;
            rod_apply(r0, J[0], J[1], J[2], ux, uy, uz);
            rod_apply(r1, J[0], J[1], J[2], wx, wy, wz);
            partial = (ux - wx) * (ux - wx) + (uy - wy) * (uy - wy) + (uz - wz) * (uz - wz);
        }
        double *cs = xch + 102;
        if (role < 7) cs[role] = partial;
        group_lds_fence();
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { s += cs[k]; s += cs[3 + k]; }     // the serial order: part 0 point k, part 1 point k
        if constexpr (PRISM) s += cs[6]; else s += wj * cs[6];
        group_lds_fence();                                             // the record is reused by the next callback
        return s;
    }

    __device__ __forceinline__ void normal(const double x[6], double A[21], double g[6]) const {
        double *col = xch, *jdx = xch + 54, *rhx = xch + 72, *fx = xch + 78, *jux = xch + 96;
        {   // ---- this lane's forward-difference column (roles 6, 7 shadow roles 0, 1 without writing) ----
            const int cr = role < 6 ? role : role - 6;
            const bool p1 = cr >= 3;
            const int q = p1 ? cr - 3 : cr;
            const double r0 = p1 ? x[3] : x[0], r1 = p1 ? x[4] : x[1], r2 = p1 ? x[5] : x[2];
            const Rod b = rod_prepare(r0, r1, r2);
            const double h = fd_step(q == 0 ? r0 : q == 1 ? r1 : r2);
            const double rh = fast_rcp(h);
            const Rod pr = rod_prepare(r0 + (q == 0 ? h : 0.0), r1 + (q == 1 ? h : 0.0), r2 + (q == 2 ? h : 0.0));
            const bool wr = role < 6;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double px = p1 ? x1[i][0] : x0[i][0], py = p1 ? x1[i][1] : x0[i][1], pz = p1 ? x1[i][2] : x0[i][2];
                const double yx = p1 ? y1[i][0] : y0[i][0], yy = p1 ? y1[i][1] : y0[i][1], yz = p1 ? y1[i][2] : y0[i][2];
                double ox, oy, oz, qx, qy, qz;
                rod_apply(b, px, py, pz, ox, oy, oz);
                const double f0 = yx - ox, f1 = yy - oy, f2 = yz - oz;
                rod_apply(pr, px, py, pz, qx, qy, qz);
                if (wr) {
                    col[cr * 9 + i * 3 + 0] = ((yx - qx) - f0) * rh;
                    col[cr * 9 + i * 3 + 1] = ((yy - qy) - f1) * rh;
                    col[cr * 9 + i * 3 + 2] = ((yz - qz) - f2) * rh;
                    if (q == 0) { fx[(p1 ? 9 : 0) + i * 3] = f0; fx[(p1 ? 9 : 0) + i * 3 + 1] = f1; fx[(p1 ? 9 : 0) + i * 3 + 2] = f2; }
                }
            }
            if constexpr (!PRISM) {
                double ux, uy, uz, vx, vy, vz;
                rod_apply(b, J[0], J[1], J[2], ux, uy, uz);
                rod_apply(pr, J[0], J[1], J[2], vx, vy, vz);
                if (wr) {
                    jdx[cr * 3] = vx; jdx[cr * 3 + 1] = vy; jdx[cr * 3 + 2] = vz;
                    rhx[cr] = rh;
                    if (q == 0) { jux[(p1 ? 3 : 0)] = ux; jux[(p1 ? 3 : 0) + 1] = uy; jux[(p1 ? 3 : 0) + 2] = uz; }
                }
            }
        }
        group_lds_fence();
        // ---- every lane: the same assembly as PartFd::point (per part) + assemble_normal ----
        double blk[2][6], gv[2][3];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int e = 0; e < 6; ++e) blk[p][e] = 0.0;
            gv[p][0] = gv[p][1] = gv[p][2] = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double a[3][3];
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[c][q] = col[(p * 3 + q) * 9 + i * 3 + c];
                const double f0 = fx[p * 9 + i * 3], f1 = fx[p * 9 + i * 3 + 1], f2 = fx[p * 9 + i * 3 + 2];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
#pragma unroll
                    for (int r = 0; r <= q; ++r) blk[p][q * (q + 1) / 2 + r] += a[0][q] * a[0][r] + a[1][q] * a[1][r] + a[2][q] * a[2][r];
                    gv[p][q] += a[0][q] * f0 + a[1][q] * f1 + a[2][q] * f2;
                }
            }
        }
        if constexpr (PRISM) {
            assemble_normal_prismatic(x, blk[0], gv[0], blk[1], gv[1], A, g);
        } else {
        double f[3], a[3][6];
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = jux[c] - jux[3 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                a[c][q] = ((jdx[q * 3 + c] - jux[3 + c]) - f[c]) * rhx[q];
                a[c][3 + q] = ((jux[c] - jdx[(3 + q) * 3 + c]) - f[c]) * rhx[3 + q];
            }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double v = wj * (a[0][i] * a[0][j] + a[1][i] * a[1][j] + a[2][i] * a[2][j]);
                if (i < 3) v += blk[0][i * (i + 1) / 2 + j];
                else if (j >= 3) v += blk[1][(i - 3) * (i - 2) / 2 + (j - 3)];
                A[i * (i + 1) / 2 + j] = v;
            }
            g[i] = wj * (a[0][i] * f[0] + a[1][i] * f[1] + a[2][i] * f[2]) + (i < 3 ? gv[0][i] : gv[1][i - 3]);
        }
        }
        group_lds_fence();                                             // the record is reused by the next callback
    }
};
typedef HypProblemCoopT<false> HypProblemCoop;

template <int KM, bool PRISM>
__device__ __forceinline__ void ransac_joint_lm_coop_run(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                         const float *__restrict__ src, const float *__restrict__ tgt,
                                                         const float *__restrict__ joint_dir, int niter,
                                                         const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                         double *__restrict__ models, int *__restrict__ lm_stat,
                                                         double (*xch)[COOP_XCH]) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 1);
    const int kbase = key_problem_base<KM>(seed_arg);
    const int prob = blockIdx.y, lane = threadIdx.x;
    const int a0 = rng0[prob * 2], n0 = rng0[prob * 2 + 1] - a0;
    const int a1 = rng1[prob * 2], n1 = rng1[prob * 2 + 1] - a1;
    if (n0 <= 0 || n1 <= 0) return;
    const int c1 = min(niter, (int)(blockIdx.x + 1) * COOP_HYP_PER_WAVE);
    int next = blockIdx.x * COOP_HYP_PER_WAVE;          // wave-uniform: first hypothesis of the chunk not yet handed out
    const int grp = lane / COOP_G;
    const unsigned long long leaders = 0x0101010101010101ull;        // lane 0 of every group
    HypProblemCoopT<PRISM> P;
    if constexpr (!PRISM) {
        P.J[0] = joint_dir[prob * 3]; P.J[1] = joint_dir[prob * 3 + 1]; P.J[2] = joint_dir[prob * 3 + 2];
        P.wj = 3.0;   // min(3,3) copies of the joint axis (:134)
    }
    P.xch = xch[grp];
    P.role = lane & (COOP_G - 1);
    Lm6 S;
    bool active = false;
    int h = 0;
    for (;;) {
        const unsigned long long idle = __ballot(!active) & leaders;     // one bit per idle group
        const int n_idle = __popcll(idle);
        if (next < c1 && n_idle > 0) {
            if (!active) {
                const int mine = next + __popcll(idle & ((1ull << (grp * COOP_G)) - 1ull));
                if (mine < c1) {
                    h = mine;
                    const double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
                    HypSamples q;
                    load_hyp_samples(src, tgt, draws, seed, prob, kbase, niter, h, a0, n0, a1, n1, q);
                    center_part3(q.s0, q.t0, (float)mo[6], P.x0, P.y0);
                    center_part3(q.s1, q.t1, (float)mo[7], P.x1, P.y1);
#pragma unroll
                    for (int i = 0; i < 6; ++i) S.x[i] = mo[i];
                    lm6_begin(P, S);
                    active = true;
                }
            }
            next += n_idle;
        } else if (n_idle == 64 / COOP_G) {
            break;
        }
        if (active && lm6_trip(P, S, 1e-4, 1e-8, 1e-8, 4200)) {
            if (P.role == 0) {
                double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
#pragma unroll
                for (int i = 0; i < 6; ++i) mo[i] = S.x[i];
                if (lm_stat) { lm_stat[((size_t)prob * niter + h) * 2] = S.info; lm_stat[((size_t)prob * niter + h) * 2 + 1] = S.nfev; }
            }
            active = false;
        }
    }
}

template <int KM>
__global__ __launch_bounds__(64) void ransac_joint_lm_coop_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                  const float *__restrict__ src, const float *__restrict__ tgt,
                                                                  const float *__restrict__ joint_dir, int niter,
                                                                  const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                                  double *__restrict__ models, int *__restrict__ lm_stat) {
    __shared__ double xch[64 / COOP_G][COOP_XCH];
    ransac_joint_lm_coop_run<KM, false>(rng0, rng1, src, tgt, joint_dir, niter, draws, seed_arg, models, lm_stat, xch);
}

template <int KM>
__global__ __launch_bounds__(64) void ransac_joint_lm_coop_kind_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                       const float *__restrict__ src, const float *__restrict__ tgt,
                                                                       const float *__restrict__ joint_dir, int niter,
                                                                       const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                                       double *__restrict__ models, int *__restrict__ lm_stat,
                                                                       const int *__restrict__ joint_kind) {
    __shared__ double xch[64 / COOP_G][COOP_XCH];      // one record array serves whichever body the block runs
    if (joint_kind[blockIdx.y] != 0) ransac_joint_lm_coop_run<KM, true>(rng0, rng1, src, tgt, joint_dir, niter, draws, seed_arg, models, lm_stat, xch);
    else ransac_joint_lm_coop_run<KM, false>(rng0, rng1, src, tgt, joint_dir, niter, draws, seed_arg, models, lm_stat, xch);
}

template <int KM>
__global__ __launch_bounds__(64) void ransac_joint_model_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                const float *__restrict__ src, const float *__restrict__ tgt,
                                                                int niter, const int *__restrict__ draws, KeyArg<KM> seed_arg,
                                                                double *__restrict__ models) {
    const unsigned long long seed = kernel_seed<KM>(seed_arg, 1);
    const int kbase = key_problem_base<KM>(seed_arg);
    const int prob = blockIdx.y, h = blockIdx.x * 64 + threadIdx.x;
    const int a0 = rng0[prob * 2], n0 = rng0[prob * 2 + 1] - a0;
    const int a1 = rng1[prob * 2], n1 = rng1[prob * 2 + 1] - a1;
    if (h >= niter || n0 <= 0 || n1 <= 0) return;
    double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
    HypSamples q;
    load_hyp_samples(src, tgt, draws, seed, prob, kbase, niter, h, a0, n0, a1, n1, q);
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = mo[i];
    const float sc0 = (float)mo[8], sc1 = (float)mo[9];
    double R0[9], R1[9], tr0[3], tr1[3];
    rotvec_to_mat(x, R0);
    rotvec_to_mat(x + 3, R1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double u = 0.0, v = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u += (double)q.t0[i][a] - (double)sc0 * (R0[a * 3] * q.s0[i][0] + R0[a * 3 + 1] * q.s0[i][1] + R0[a * 3 + 2] * q.s0[i][2]);
            v += (double)q.t1[i][a] - (double)sc1 * (R1[a * 3] * q.s1[i][0] + R1[a * 3 + 1] * q.s1[i][1] + R1[a * 3 + 2] * q.s1[i][2]);
        }
        tr0[a] = u / 3.0;
        tr1[a] = v / 3.0;
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) { mo[a] = R0[a]; mo[13 + a] = R1[a]; }
    mo[9] = sc0; mo[22] = sc1;
#pragma unroll
    for (int a = 0; a < 3; ++a) { mo[10 + a] = tr0[a]; mo[23 + a] = tr1[a]; }
}

// joint_transformation_verifier for every hypothesis: ONE WAVE per hypothesis, lanes stride over the
// points of both parts (coalesced 12-B rows from L2), inlier counts by ballot/popcount.
__global__ __launch_bounds__(256) void ransac_joint_verify_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                 const float *__restrict__ src, const float *__restrict__ tgt,
                                                                 double th, int niter, const double *__restrict__ models,
                                                                 double *__restrict__ scores) {
    const int prob = blockIdx.y, lane = threadIdx.x & 63;
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= niter) return;
    const int a0 = rng0[prob * 2], n0 = rng0[prob * 2 + 1] - a0;
    const int a1 = rng1[prob * 2], n1 = rng1[prob * 2 + 1] - a1;
    if (n0 <= 0 || n1 <= 0) return;                       // score already -1
    const double *mo = models + ((size_t)prob * niter + h) * MODEL_B;
    double R0[9], R1[9], tr0[3], tr1[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) { R0[a] = mo[a]; R1[a] = mo[13 + a]; }
    const double sc0 = mo[9], sc1 = mo[22];
#pragma unroll
    for (int a = 0; a < 3; ++a) { tr0[a] = mo[10 + a]; tr1[a] = mo[23 + a]; }
    int c0 = 0, c1 = 0;
    for (int i = lane; i < n0; i += 64) {
        const float *ps = src + (size_t)(a0 + i) * 3, *pt = tgt + (size_t)(a0 + i) * 3;
        c0 += inlier_f64(R0, sc0, tr0, ps[0], ps[1], ps[2], pt[0], pt[1], pt[2], th) ? 1 : 0;
    }
    for (int i = lane; i < n1; i += 64) {
        const float *ps = src + (size_t)(a1 + i) * 3, *pt = tgt + (size_t)(a1 + i) * 3;
        c1 += inlier_f64(R1, sc1, tr1, ps[0], ps[1], ps[2], pt[0], pt[1], pt[2], th) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); }
    // (sum(inl0)/res0.shape[0] + sum(inl1)/res1.shape[0])/2 with res.shape[0] == 3 (sic, :192)
    if (lane == 0) scores[(size_t)prob * niter + h] = ((double)c0 / 3.0 + (double)c1 / 3.0) / 2.0;
}

// Workgroup-cooperative articulated problem over LDS-resident inliers (final refit :32 -> :106-184).
// PRISM: the prismatic objective; its three constraint rows are added once after block_sum, as assemble_normal adds the joint rows.
template <bool PRISM>
struct BlockProblemT {
    const float (*x0)[3];
    const float (*y0)[3];
    const float (*x1)[3];
    const float (*y1)[3];
    int n0, n1;
    double J[3], wj;
    double *red;

    __device__ __forceinline__ double cost(const double x[6]) const {
        const Rod r0 = rod_prepare(x[0], x[1], x[2]), r1 = rod_prepare(x[3], x[4], x[5]);
        double s[1] = {0.0}, ox, oy, oz;
        for (int i = threadIdx.x; i < n0; i += 256) {
            rod_apply(r0, x0[i][0], x0[i][1], x0[i][2], ox, oy, oz);
            const double a = y0[i][0] - ox, b = y0[i][1] - oy, c = y0[i][2] - oz;
            s[0] += a * a + b * b + c * c;
        }
        for (int i = threadIdx.x; i < n1; i += 256) {
            rod_apply(r1, x1[i][0], x1[i][1], x1[i][2], ox, oy, oz);
            const double a = y1[i][0] - ox, b = y1[i][1] - oy, c = y1[i][2] - oz;
            s[0] += a * a + b * b + c * c;
        }
        block_sum<1>(s, red, 4);
        if constexpr (PRISM) {
            return s[0] + prismatic_cost(x);
        } else {
            double ux, uy, uz, wx, wy, wz;
            rod_apply(r0, J[0], J[1], J[2], ux, uy, uz);
            rod_apply(r1, J[0], J[1], J[2], wx, wy, wz);
            return s[0] + wj * ((ux - wx) * (ux - wx) + (uy - wy) * (uy - wy) + (uz - wz) * (uz - wz));
        }
    }
    __device__ __forceinline__ void normal(const double x[6], double A[21], double g[6]) const {
        PartFd p0, p1;
        if constexpr (PRISM) p0.begin_points(x); else p0.begin(x, J);
        for (int i = threadIdx.x; i < n0; i += 256) p0.point(x0[i][0], x0[i][1], x0[i][2], y0[i][0], y0[i][1], y0[i][2]);
        if constexpr (PRISM) p1.begin_points(x + 3); else p1.begin(x + 3, J);
        for (int i = threadIdx.x; i < n1; i += 256) p1.point(x1[i][0], x1[i][1], x1[i][2], y1[i][0], y1[i][1], y1[i][2]);
        double v[18];
#pragma unroll
        for (int i = 0; i < 6; ++i) { v[i] = p0.blk[i]; v[9 + i] = p1.blk[i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) { v[6 + i] = p0.gv[i]; v[15 + i] = p1.gv[i]; }
        block_sum<18>(v, red, 4);
        if constexpr (PRISM) assemble_normal_prismatic(x, v, v + 6, v + 9, v + 15, A, g);
        else assemble_normal(p0, v, v + 6, p1, v + 9, v + 15, wj, A, g);
    }
};
typedef BlockProblemT<false> BlockProblem;

// pairwise scale sums of one part over LDS-resident inliers -> (s, s_inv) as float32
__device__ __forceinline__ void block_scales(const float (*cs)[3], const float (*ct)[3], int n, double *red, float &sc,
                                             float &sc_inv) {
    double pr[3] = {0, 0, 0};
    pair_sums(cs, ct, n, pr);
    block_sum<3>(pr, red, 4);
    sc = (float)(pr[0] / (pr[1] + 1e-6));
    sc_inv = (float)(pr[0] / (pr[2] + 1e-6));
}

// centre source, pre-scale + centre target IN PLACE (float32 like the reference's arrays); returns
// the uncentred means (for the translation) and the Kabsch rotation vector.
__device__ __forceinline__ void block_prep_part(float (*cs)[3], float (*ct)[3], int n, float sc_inv, double *red,
                                                double smean[3], double tmean[3], double rv[3]) {
    double sums[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int c = 0; c < 3; ++c) { sums[c] += cs[i][c]; sums[3 + c] += ct[i][c]; }
    block_sum<6>(sums, red, 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) { smean[c] = sums[c] / n; tmean[c] = sums[3 + c] / n; }
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += 256) {
        float xc[3], yc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xc[c] = cs[i][c] - (float)smean[c];
            yc[c] = sc_inv * ct[i][c] - (float)((double)sc_inv * tmean[c]);
            cs[i][c] = xc[c];
            ct[i][c] = yc[c];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) M[a * 3 + b] += (double)yc[a] * xc[b];
    }
    block_sum<9>(M, red, 4);
    double q[4];
    horn_quat(M, q);
    quat_to_rotvec(q, rv);
}

// PRISM: the refit minimises the prismatic objective.  The *_kind_kernel below runs the whole body of one kind or the other per block
// (not a branch at the refit alone): the revolute half is then the instruction stream of the kernel without kinds, to the last bit of
// the f64 code that is compiled with contraction on.
template <int KM, bool PRISM>
__device__ __forceinline__ void ransac_joint_finish_run(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                        const float *__restrict__ src, const float *__restrict__ tgt,
                                                        const float *__restrict__ joint_dir, double th, int niter,
                                                        const double *__restrict__ scores,
                                                        const double *__restrict__ models, int max_n,
                                                        double *__restrict__ out_model,
                                                        unsigned char *__restrict__ out_inliers,
                                                        int *__restrict__ out_best, double *__restrict__ out_score, const FitExtras &E,
                                                        unsigned char *smem) {
    double *red = (double *)smem;                      // 24*4 doubles
    int *wcnt = (int *)(red + 128);
    float(*c0s)[3] = (float(*)[3])(wcnt + 8);
    float(*c0t)[3] = c0s + max_n;
    float(*c1s)[3] = c0t + max_n;
    float(*c1t)[3] = c1s + max_n;
    const int prob = blockIdx.x;
    const int a0 = rng0[prob * 2], n0 = rng0[prob * 2 + 1] - a0;
    const int a1 = rng1[prob * 2], n1 = rng1[prob * 2 + 1] - a1;
    double *om = out_model + (size_t)prob * MODEL_B;
    unsigned char *oi0 = out_inliers + (size_t)prob * 2 * max_n, *oi1 = oi0 + max_n;
    // the record rows this joint fit reports (see FitExtras): part q + 1 always, part 0 from the cloud's first joint
    double *rec1 = nullptr, *rec0 = nullptr;
    if (E.record) {
        const int cloud = prob / (E.K - 1), q = prob - cloud * (E.K - 1);
        rec1 = E.record + ((size_t)cloud * E.K + q + 1) * 26 + MODEL_A;
        if (q == 0) rec0 = E.record + (size_t)cloud * E.K * 26 + MODEL_A;
    }
    if (n0 <= 0 || n1 <= 0 || n0 > max_n || n1 > max_n) {
        if (threadIdx.x < MODEL_B) om[threadIdx.x] = NAN;
        if (threadIdx.x < MODEL_A) { if (rec1) rec1[threadIdx.x] = NAN; if (rec0) rec0[threadIdx.x] = NAN; }
        if (E.tie && threadIdx.x < 2) E.tie[prob * 2 + threadIdx.x] = 0;
        if (threadIdx.x == 0) { out_best[prob] = -1; out_score[prob] = -1.0; }
        for (int i = threadIdx.x; i < 2 * max_n; i += 256) oi0[i] = 0;             // the whole (2, max_n) mask is written here:
        return;                                                                     // callers need not pre-clear it
    }
    for (int i = n0 + threadIdx.x; i < max_n; i += 256) oi0[i] = 0;
    for (int i = n1 + threadIdx.x; i < max_n; i += 256) oi1[i] = 0;
    double best_score;
    const int best = block_argmax_first<double>(scores + (size_t)prob * niter, niter, &best_score, red);
    const double *bm = models + ((size_t)prob * niter + best) * MODEL_B;
    double R0[9], R1[9], tr0[3], tr1[3];
#pragma unroll
    for (int a = 0; a < 9; ++a) { R0[a] = bm[a]; R1[a] = bm[13 + a]; }
    const double hs0 = bm[9], hs1 = bm[22];
#pragma unroll
    for (int a = 0; a < 3; ++a) { tr0[a] = bm[10 + a]; tr1[a] = bm[23 + a]; }
    int m0 = 0, m1 = 0, n_border = 0, n_near = 0;
    for (int base = 0; base < n0; base += 256) {
        const int i = base + threadIdx.x;
        bool f = false, border = false;
        if (i < n0) {
            const float *ps = src + (size_t)(a0 + i) * 3, *pt = tgt + (size_t)(a0 + i) * 3;
            const double rs = residual_sq_f64(R0, hs0, tr0, ps[0], ps[1], ps[2], pt[0], pt[1], pt[2]);
            f = rs < th;
            border = rs >= E.lo_d && rs < E.hi_d;
            oi0[i] = f ? 1 : 0;
        }
        n_border += __popcll(__ballot(border));
        m0 = compact_flagged(f, i, n0, src, tgt, (size_t)a0, c0s, c0t, m0, wcnt);
    }
    for (int base = 0; base < n1; base += 256) {
        const int i = base + threadIdx.x;
        bool f = false, border = false;
        if (i < n1) {
            const float *ps = src + (size_t)(a1 + i) * 3, *pt = tgt + (size_t)(a1 + i) * 3;
            const double rs = residual_sq_f64(R1, hs1, tr1, ps[0], ps[1], ps[2], pt[0], pt[1], pt[2]);
            f = rs < th;
            border = rs >= E.lo_d && rs < E.hi_d;
            oi1[i] = f ? 1 : 0;
        }
        n_border += __popcll(__ballot(border));
        m1 = compact_flagged(f, i, n1, src, tgt, (size_t)a1, c1s, c1t, m1, wcnt);
    }
    if (E.tie) {                                       // block-uniform; one inlier of either part moves the joint score by 1/6 (:192)
        const unsigned long long tseed = kernel_seed<KM>(E.seed, 1);
        // KEY_DKEY: E.seed holds the ancsh_stream_key's address and E.K the parts per cloud (the entry checks K >= 2)
        const int tbase = KM == KEY_DKEY ? ((const ancsh_stream_key *)E.seed)->cloud_base * (E.K - 1) : 0;
        const double *sp = scores + (size_t)prob * niter;
        const double near = best_score - (1.0 / 6.0 + 1e-9);
        for (int h = threadIdx.x; h < niter + 255 - (niter + 255) % 256; h += 256) {
            bool degenerate = false;
            if (h < niter && sp[h] >= near) {
                int i0[3], i1[3];
                load_draw3(E.draws, tseed, prob, tbase, niter, h, 0, 6, n0, i0);
                load_draw3(E.draws, tseed, prob, tbase, niter, h, 3, 6, n1, i1);
                degenerate = i0[0] == i0[1] || i0[0] == i0[2] || i0[1] == i0[2] || i1[0] == i1[1] || i1[0] == i1[2] || i1[1] == i1[2];
            }
            n_near += __popcll(__ballot(degenerate));
        }
        if ((threadIdx.x & 63) == 0) { wcnt[4 + (threadIdx.x >> 6)] = n_border; red[8 + (threadIdx.x >> 6)] = (double)n_near; }
        __syncthreads();
        if (threadIdx.x == 0) {
            E.tie[prob * 2] = wcnt[4] + wcnt[5] + wcnt[6] + wcnt[7];
            E.tie[prob * 2 + 1] = (int)(red[8] + red[9] + red[10] + red[11]);
        }
    }
    __syncthreads();
    if (m0 == 0 || m1 == 0) {   // the reference would produce NaNs (mean of an empty selection)
        if (threadIdx.x < MODEL_B) om[threadIdx.x] = NAN;
        if (threadIdx.x < MODEL_A) { if (rec1) rec1[threadIdx.x] = NAN; if (rec0) rec0[threadIdx.x] = NAN; }
        if (threadIdx.x == 0) { out_best[prob] = best; out_score[prob] = best_score; }
        return;
    }
    float sc0, sc0i, sc1, sc1i;
    block_scales(c0s, c0t, m0, red, sc0, sc0i);
    block_scales(c1s, c1t, m1, red, sc1, sc1i);
    double sm0[3], tm0[3], sm1[3], tm1[3], x[6];
    block_prep_part(c0s, c0t, m0, sc0i, red, sm0, tm0, x);
    block_prep_part(c1s, c1t, m1, sc1i, red, sm1, tm1, x + 3);
    __syncthreads();
    if constexpr (PRISM) {                             // 3 (m0 + m1) + 3 rows: no min(m0, m1) copies, no joint direction
        BlockProblemT<true> P;
        P.x0 = c0s; P.y0 = c0t; P.x1 = c1s; P.y1 = c1t;
        P.n0 = m0; P.n1 = m1;
        P.red = red;
        lmdif6(P, x, 1e-4, 1e-8, 1e-8, 4200, nullptr);
    } else {
        BlockProblem P;
        P.x0 = c0s; P.y0 = c0t; P.x1 = c1s; P.y1 = c1t;
        P.n0 = m0; P.n1 = m1;
        P.J[0] = joint_dir[prob * 3]; P.J[1] = joint_dir[prob * 3 + 1]; P.J[2] = joint_dir[prob * 3 + 2];
        P.wj = (double)(m0 < m1 ? m0 : m1);
        P.red = red;
        lmdif6(P, x, 1e-4, 1e-8, 1e-8, 4200, nullptr);
    }
    rotvec_to_mat(x, R0);
    rotvec_to_mat(x + 3, R1);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 9; ++a) { om[a] = R0[a]; om[13 + a] = R1[a]; }
        om[9] = sc0; om[22] = sc1;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // mean(target - scale*R*source) over the inliers
            om[10 + a] = tm0[a] - (double)sc0 * (R0[a * 3] * sm0[0] + R0[a * 3 + 1] * sm0[1] + R0[a * 3 + 2] * sm0[2]);
            om[23 + a] = tm1[a] - (double)sc1 * (R1[a * 3] * sm1[0] + R1[a * 3 + 1] * sm1[1] + R1[a * 3 + 2] * sm1[2]);
        }
        out_best[prob] = best;
        out_score[prob] = best_score;
#pragma unroll
        for (int a = 0; a < MODEL_A; ++a) {
            if (rec1) rec1[a] = om[MODEL_A + a];
            if (rec0) rec0[a] = om[a];
        }
    }
}

template <int KM>
__global__ __launch_bounds__(256) void ransac_joint_finish_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                  const float *__restrict__ src, const float *__restrict__ tgt,
                                                                  const float *__restrict__ joint_dir, double th, int niter,
                                                                  const double *__restrict__ scores,
                                                                  const double *__restrict__ models, int max_n,
                                                                  double *__restrict__ out_model,
                                                                  unsigned char *__restrict__ out_inliers,
                                                                  int *__restrict__ out_best, double *__restrict__ out_score, FitExtras E) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ransac_joint_finish_run<KM, false>(rng0, rng1, src, tgt, joint_dir, th, niter, scores, models, max_n, out_model, out_inliers, out_best,
                                       out_score, E, smem);
}

template <int KM>
__global__ __launch_bounds__(256) void ransac_joint_finish_kind_kernel(const int *__restrict__ rng0, const int *__restrict__ rng1,
                                                                       const float *__restrict__ src, const float *__restrict__ tgt,
                                                                       const float *__restrict__ joint_dir, double th, int niter,
                                                                       const double *__restrict__ scores,
                                                                       const double *__restrict__ models, int max_n,
                                                                       double *__restrict__ out_model,
                                                                       unsigned char *__restrict__ out_inliers,
                                                                       int *__restrict__ out_best, double *__restrict__ out_score, FitExtras E,
                                                                       const int *__restrict__ joint_kind) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (joint_kind[blockIdx.x] != 0)
        ransac_joint_finish_run<KM, true>(rng0, rng1, src, tgt, joint_dir, th, niter, scores, models, max_n, out_model, out_inliers, out_best,
                                          out_score, E, smem);
    else
        ransac_joint_finish_run<KM, false>(rng0, rng1, src, tgt, joint_dir, th, niter, scores, models, max_n, out_model, out_inliers, out_best,
                                           out_score, E, smem);
}

}  // namespace pose
}  // namespace ancsh

using namespace ancsh;
using namespace ancsh::pose;

// ================================ the host side =====================================================
// The nineteen fit entries of include/ancsh_hip.h -- ancsh_ransac_single{,_ex,_rec,_rec_dseed,_rec_dkey}, ancsh_ransac_joint{,_ex,_rec,
// _rec_dseed,_rec_dkey,_rec_kind,_rec_dseed_kind,_rec_dkey_kind} and ancsh_pose_fit_rec{,_dseed,_dkey}{,_kind} -- are adapters: each
// fills a FitCall from its parameters and hands it to pose_fit(), which runs every argument check of the stages that are present and
// then, through one switch on the key mode, the launches.  A new argument of the fit is a new field, read where it is needed.

// T = min{x >= 0 : sqrt(x) >= th} in the given precision (host libm sqrt is correctly rounded, like the
// reference's numpy sqrt), so that  sqrt(s) < th  <=>  s < T  exactly.
static float sq_threshold_f32(float th) {
    float t = th * th;
    while (sqrtf(t) >= th && t > 0.f) t = nextafterf(t, 0.f);
    while (sqrtf(t) < th) t = nextafterf(t, INFINITY);
    return t;
}
static double sq_threshold_f64(double th) {
    double t = th * th;
    while (sqrt(t) >= th && t > 0.0) t = nextafter(t, 0.0);
    while (sqrt(t) < th) t = nextafter(t, INFINITY);
    return t;
}

// The generator key of one stage as the entry received it (key modes: KeyArg above).  KEY_VALUE: `value`; KEY_DSEED / KEY_DKEY: `dev`, a
// uint64 / an ancsh_stream_key in device memory.
struct FitKey { int mode; unsigned long long value; const void *dev; };
// the 64 bits that travel by value: the key itself or the address (FitExtras.seed of stage B in every mode)
static unsigned long long key_word(const FitKey &k) { return k.mode == KEY_VALUE ? k.value : (unsigned long long)(uintptr_t)k.dev; }
// the kernels' key argument; parts: the stage's problems per cloud (K in stage A, K - 1 in stage B), which only KEY_DKEY reads
template <int KM>
static KeyArg<KM> key_arg(const FitKey &k, int parts) {
    if constexpr (KM == KEY_DKEY) return DKey{(const ancsh_stream_key *)k.dev, parts};
    else return key_word(k);
}

// The two stages' own arguments, in the order of the entries' parameter lists.  present = false: the entry has no such stage, and none
// of its rules is examined -- which is not nprob == 0: an empty stage of a whole-fit entry still has its sizes and schedule checked.
struct StageA {
    bool present;
    int nprob; const int *off; float th; int niter; const int *draws;
    double *out_model; unsigned char *out_inliers; int *out_best, *scores;
    float *quads; long rows;      // quads NULL: the LDS-staged scoring kernel
    int *tie; float tie_window;
};
struct StageB {
    bool present;
    int nprob; const int *rng0, *rng1; const float *joint_dir; double th; int niter; const int *draws;
    double *out_model; unsigned char *out_inliers; int *out_best; double *out_score, *scores, *models;
    int *lm_stat, lm_schedule, *tie; double tie_window;
    const int *joint_kind;        // NULL: every problem revolute, the kernels without a kind
};
struct FitCall {
    const char *who;              // the entry's name in messages
    const float *src, *tgt; int max_n; double *record; int K; void *stream;
    StageA a; FitKey key_a;
    StageB b; FitKey key_b;
};
static bool whole_fit(const FitCall &c) { return c.a.present && c.b.present; }
static int key_mode(const FitCall &c) { return c.a.present ? c.key_a.mode : c.key_b.mode; }

// min_K: 1 for the per-part fits (nprob = B * K), 2 for the joint fits (nprob = B * (K - 1)).  The tie window is an ABSOLUTE half-width
// on the residual norm: a point counts when th - w <= |res| < th + w, evaluated on the squared norm the verifiers already compute.
static int make_extras(const FitCall &c, int nprob, int min_K, int *tie, double th, double window, FitExtras &E) {
    E.record = c.record; E.K = c.K; E.tie = tie;
    if (c.record)
        ANCSH_REQUIRE(c.K >= min_K && nprob % (c.K - (min_K - 1)) == 0, "%s: record needs K >= %d and nprob (%d) a multiple of %s (K = %d)", c.who, min_K,
                      nprob, min_K == 1 ? "K" : "K - 1", c.K);
    if (tie) {
        ANCSH_REQUIRE(window >= 0.0 && window < th, "%s: tie_window %g must be in [0, inlier_th)", c.who, window);
        const double lo = (th - window) * (th - window), hi = (th + window) * (th + window);
        E.lo_f = (float)lo; E.hi_f = (float)hi; E.lo_d = lo; E.hi_d = hi;
    }
    return ANCSH_OK;
}

static long single_quads_needed(long rows, int nprob) { return 2 * ((rows + 7) / 8 + nprob) + 2; }     // quads (24 floats each)
extern "C" long ancsh_ransac_single_quads_floats(long rows, int nprob) {
    if (rows < 0 || nprob < 0) return -1;
    return 24 * single_quads_needed(rows, nprob);
}

// The rules of the device key modes.  An entry of one stage examines its pointer and its counts whatever nprob is; a whole-fit entry lets a
// stage without problems pass (nprob_b == 0 is how a K = 1 caller gets there) and names the count it rejects nprob_a / nprob_b.
// KEY_DKEY needs K even without a record: it is the problem count of one cloud.  cloud_base lives in device memory, so
// (cloud_base + B) * K < 2^20 -- which keeps the draw keys clear of the sampler's tag bits -- is the caller's to check where it writes
// the block (AncshPipeline.submit, dataset.check_stream_key).
static int check_keys(const FitCall &c) {
    const StageA &a = c.a; const StageB &b = c.b;
    const bool whole = whole_fit(c); const int mode = key_mode(c);
    if (mode == KEY_VALUE) return ANCSH_OK;
    ANCSH_REQUIRE((!a.present || c.key_a.dev || (whole && a.nprob <= 0)) && (!b.present || c.key_b.dev || (whole && b.nprob <= 0)),
                  "%s: null %s pointer", c.who, mode == KEY_DSEED ? "seed" : "key");
    if (mode != KEY_DKEY) return ANCSH_OK;
    if (a.present)
        ANCSH_REQUIRE(c.K >= 1 && a.nprob >= 0 && a.nprob % c.K == 0 && a.nprob < (1 << 20), "%s: nprob%s (%d) must be a multiple of K (%d) below 2^20",
                      c.who, whole ? "_a" : "", a.nprob, c.K);
    if (b.present)
        ANCSH_REQUIRE((whole && b.nprob == 0) || (c.K >= 2 && b.nprob >= 0 && b.nprob % (c.K - 1) == 0 && b.nprob < (1 << 20)),
                      "%s: nprob%s (%d) must be a multiple of K - 1 (K = %d >= 2) below 2^20", c.who, whole ? "_b" : "", b.nprob, c.K);
    return ANCSH_OK;
}

// joint_kind of the *_kind entries: NULL is "all revolute".  A host-side array (pinned or registered host memory) is checked here --
// every entry 0 or 1 -- because here the host can see it; a device array is not read by the host (no synchronisation), and the kernels
// take any non-zero entry as prismatic.
static int check_joint_kind(const char *who, int nprob, const int *joint_kind) {
    if (!joint_kind || nprob <= 0) return ANCSH_OK;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, joint_kind) != hipSuccess) { (void)hipGetLastError(); return ANCSH_OK; }
    if (at.type != hipMemoryTypeHost) return ANCSH_OK;
    for (int p = 0; p < nprob; ++p)
        ANCSH_REQUIRE(joint_kind[p] == 0 || joint_kind[p] == 1, "%s: joint_kind[%d] = %d (0 revolute, 1 prismatic)", who, p, joint_kind[p]);
    return ANCSH_OK;
}

// Stage A's argument checks.  nprob == 0 passes after the size checks: the stage is then a no-op.
static int ransac_single_check(const FitCall &c) {
    const StageA &a = c.a;
    ANCSH_REQUIRE(a.nprob >= 0 && a.niter > 0 && c.max_n > 0, "ransac_single: bad sizes nprob=%d niter=%d max_n=%d", a.nprob, a.niter, c.max_n);
    ANCSH_REQUIRE(c.max_n <= 6144, "ransac_single: max_n %d > 6144 (refit keeps the inliers in LDS)", c.max_n);
    if (a.nprob == 0) return ANCSH_OK;
    ANCSH_REQUIRE(a.off && c.src && c.tgt && a.out_model && a.out_inliers && a.out_best && a.scores, "ransac_single: null pointer");
    ANCSH_REQUIRE(a.th > 0.f, "ransac_single: inlier_th must be positive");
    const float th_sq = sq_threshold_f32(a.th);
    if (a.quads && th_sq >= 0x1p-100f && th_sq < 4.0f) {
        ANCSH_REQUIRE(a.rows >= 0 && a.rows < (1L << 30), "ransac_single_ex: rows=%ld out of range", a.rows);
        ANCSH_REQUIRE((((uintptr_t)a.quads) & 31) == 0, "ransac_single_ex: scratch_quads must be 32-byte aligned");
    }
    return ANCSH_OK;
}

// Stage B's argument checks.  nprob == 0 passes after the size checks.
static int ransac_joint_check(const FitCall &c) {
    const StageB &b = c.b;
    ANCSH_REQUIRE(b.lm_schedule >= ANCSH_LM_AUTO && b.lm_schedule <= ANCSH_LM_LATENCY, "ransac_joint: unknown lm_schedule %d", b.lm_schedule);
    ANCSH_REQUIRE(b.nprob >= 0 && b.niter > 0 && c.max_n > 0, "ransac_joint: bad sizes");
    ANCSH_REQUIRE(c.max_n <= 3072, "ransac_joint: max_n %d > 3072 (refit keeps both parts' inliers in LDS)", c.max_n);
    if (b.nprob == 0) return ANCSH_OK;
    ANCSH_REQUIRE(b.rng0 && b.rng1 && c.src && c.tgt && b.joint_dir && b.out_model && b.out_inliers && b.out_best && b.out_score &&
                      b.scores && b.models, "ransac_joint: null pointer");
    ANCSH_REQUIRE(b.th > 0.0, "ransac_joint: inlier_th must be positive");
    return ANCSH_OK;
}

static int lm_chunk(int nprob, int niter) { return (long)nprob * niter <= HYP_SMALL_LAUNCH ? HYP_CHUNK_SMALL : HYP_CHUNK; }
static size_t single_finish_lds(int max_n) { return 64 * sizeof(double) + 8 * sizeof(int) + (size_t)2 * max_n * 3 * sizeof(float); }

// launch_lds (pose_shared.h) of one of two twin kernels: with joint_kind (the *_kind entries) the twin that branches, block-uniformly,
// on the problem's kind and takes the array as one more, last argument; without it the revolute-only kernel, untouched
template <class Kernel, class KindKernel, class... Args>
static void launch_twin(Kernel plain, KindKernel kind, const int *joint_kind, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (joint_kind) launch_lds(kind, grid, block, lds, st, args..., joint_kind);
    else launch_lds(plain, grid, block, lds, st, args...);
}

// stage A's hypothesis scores.  th_sq: the squared threshold (the kernels compare squared residuals)
template <int KM>
static void launch_score_a(const FitCall &c, KeyArg<KM> key, float th_sq, hipStream_t st) {
    const StageA &a = c.a;
    // the scalar-register kernel counts inliers as clamp((th_sq - s) * 2^126): exact while th_sq - s cannot be denormal, i.e. for any
    // threshold a fit would use; a squared threshold below 2^-100 or >= 4 (th_sq * 2^126 must stay finite) takes the compare-based kernel
    // (same scores by construction)
    if (a.quads && th_sq >= 0x1p-100f && th_sq < 4.0f) {
        const int cap = (int)single_quads_needed(a.rows, a.nprob);
        hipLaunchKernelGGL(soa_quads_kernel, dim3((c.max_n + 7 + 255) / 256, a.nprob), dim3(256), 0, st, a.off, c.src, c.tgt, a.quads, cap);
        hipLaunchKernelGGL(ransac_single_score_sreg_kernel<KM>, dim3((a.niter + 255) / 256, a.nprob), dim3(256), 0, st, a.off, c.src, c.tgt,
                           (const float *)a.quads, cap, th_sq, a.niter, a.draws, key, a.scores);
    } else {
        hipLaunchKernelGGL(ransac_single_score_kernel<KM>, dim3((a.niter + 255) / 256, a.nprob), dim3(256), 0, st, a.off, c.src, c.tgt, th_sq,
                           a.niter, a.draws, key, a.scores);
    }
}

// stage A's own chain: scores, then winner and refit
template <int KM>
static int launch_stage_a(const FitCall &c, KeyArg<KM> key, const FitExtras &E) {
    const StageA &a = c.a; hipStream_t st = (hipStream_t)c.stream;
    const float th_sq = sq_threshold_f32(a.th);
    launch_score_a<KM>(c, key, th_sq, st);
    launch_lds(ransac_single_finish_kernel<KM>, dim3(a.nprob), dim3(256), single_finish_lds(c.max_n), st, a.off, c.src, c.tgt, th_sq, a.niter,
               a.draws, key, a.scores, c.max_n, a.out_model, a.out_inliers, a.out_best, E);
    return check_launch("ransac_single");
}

// what follows stage B's LM fits: models, verification, refit (th_sq: the squared threshold)
template <int KM>
static void launch_tail_b(const FitCall &c, KeyArg<KM> key, double th_sq, const FitExtras &E, hipStream_t st) {
    const StageB &b = c.b;
    hipLaunchKernelGGL(ransac_joint_model_kernel<KM>, dim3((b.niter + 63) / 64, b.nprob), dim3(64), 0, st, b.rng0, b.rng1, c.src, c.tgt, b.niter,
                       b.draws, key, b.models);
    hipLaunchKernelGGL(ransac_joint_verify_kernel, dim3((b.niter + 3) / 4, b.nprob), dim3(256), 0, st, b.rng0, b.rng1, c.src, c.tgt, th_sq,
                       b.niter, b.models, b.scores);
    const size_t lds = 128 * sizeof(double) + 8 * sizeof(int) + (size_t)4 * c.max_n * 3 * sizeof(float);
    launch_twin(ransac_joint_finish_kernel<KM>, ransac_joint_finish_kind_kernel<KM>, b.joint_kind, dim3(b.nprob), dim3(256), lds, st, b.rng0,
                b.rng1, c.src, c.tgt, b.joint_dir, th_sq, b.niter, b.scores, b.models, c.max_n, b.out_model, b.out_inliers, b.out_best,
                b.out_score, E);
}

// stage B's own chain: hypotheses, LM fits, tail
template <int KM>
static int launch_stage_b(const FitCall &c, KeyArg<KM> key, const FitExtras &E) {
    const StageB &b = c.b; hipStream_t st = (hipStream_t)c.stream;
    hipLaunchKernelGGL(ransac_joint_init_kernel<KM>, dim3((b.niter + 63) / 64, b.nprob), dim3(64), 0, st, b.rng0, b.rng1, c.src, c.tgt, b.niter,
                       b.draws, key, b.scores, b.models);
    // Two schedules of the same fits (identical MINPACK state machine, results equal to ~1e-7, not to the last bit: the eight-lane
    // callbacks are a different instruction stream and the f64 code is compiled with contraction on):
    //   * lane per fit: least SIMD time per fit -- the throughput schedule, and what ANCSH_LM_AUTO ALWAYS takes, so that a cloud's
    //     result does not depend on how many clouds share the launch.  Only the number of hypotheses handed to a wave follows the
    //     launch size (a small launch spreads over 4x more waves); the order in which hypotheses run enters no result;
    //   * eight lanes per fit (ANCSH_LM_LATENCY, explicit only): the long fits that set the launch's duration run ~1.25x faster
    //     (measured on 64 x 200 fits: 1.27 vs 1.6 ms; the tail is MINPACK's serial lmpar on rank-deficient samples, which no lane
    //     split shortens) at ~5 % lower pipeline throughput.
    if (b.lm_schedule == ANCSH_LM_LATENCY) {
        launch_twin(ransac_joint_lm_coop_kernel<KM>, ransac_joint_lm_coop_kind_kernel<KM>, b.joint_kind,
                    dim3((b.niter + COOP_HYP_PER_WAVE - 1) / COOP_HYP_PER_WAVE, b.nprob), dim3(64), 0, st, b.rng0, b.rng1, c.src, c.tgt,
                    b.joint_dir, b.niter, b.draws, key, b.models, b.lm_stat);
    } else {
        const int chunk = lm_chunk(b.nprob, b.niter);
        launch_twin(ransac_joint_lm_kernel<KM>, ransac_joint_lm_kind_kernel<KM>, b.joint_kind, dim3((b.niter + chunk - 1) / chunk, b.nprob),
                    dim3(64), 0, st, b.rng0, b.rng1, c.src, c.tgt, b.joint_dir, b.niter, b.draws, key, b.models, b.lm_stat, chunk);
    }
    launch_tail_b<KM>(c, key, sq_threshold_f64(b.th), E, st);
    return check_launch("ransac_joint");
}

// Both stages on one stream, the LM fits and stage A's refit in ONE kernel: soa_quads, score_sreg, joint_init, pose_lm_finish_a (LM fits ||
// stage A refit), joint_model, joint_verify, joint_finish -- seven launches where the two stages' own chains issue eight, and their bytes.
template <int KM>
static int launch_fused(const FitCall &c, KeyArg<KM> key_a, KeyArg<KM> key_b, const FitExtras &EA, const FitExtras &EB) {
    const StageA &a = c.a; const StageB &b = c.b;
    LmArgs L;
    L.chunk = lm_chunk(b.nprob, b.niter);                               // the same rule as the LM launch of its own
    L.chunks_per_prob = (b.niter + L.chunk - 1) / L.chunk;
    const long n_chunks = (long)L.chunks_per_prob * b.nprob;
    ANCSH_REQUIRE((n_chunks + 3) / 4 + a.nprob < (1L << 31), "pose_fit: %ld LM chunks + %d parts exceed one grid", n_chunks, a.nprob);
    hipStream_t st = (hipStream_t)c.stream;                             // every check has passed: nothing above launches
    const float th_a = sq_threshold_f32(a.th);
    launch_score_a<KM>(c, key_a, th_a, st);
    hipLaunchKernelGGL(ransac_joint_init_kernel<KM>, dim3((b.niter + 63) / 64, b.nprob), dim3(64), 0, st, b.rng0, b.rng1, c.src, c.tgt, b.niter,
                       b.draws, key_b, b.scores, b.models);
    L.rng0 = b.rng0; L.rng1 = b.rng1; L.joint_dir = b.joint_dir; L.niter = b.niter; L.draws = b.draws; L.models = b.models; L.lm_stat = b.lm_stat;
    L.n_chunks = (int)n_chunks;
    L.n_lm = (int)((n_chunks + 3) / 4);                                 // four waves, one chunk each, per LM block
    FinishAArgs A;
    A.off = a.off; A.th = th_a; A.niter = a.niter; A.draws = a.draws; A.scores = a.scores; A.max_n = c.max_n;
    A.out_model = a.out_model; A.out_inliers = a.out_inliers; A.out_best = a.out_best;
    const size_t lds = single_finish_lds(c.max_n);
    const dim3 grid(L.n_lm + a.nprob);
    // these twins take joint_kind in the middle of their arguments, so the pick is written out
    if (b.joint_kind) launch_lds(pose_lm_finish_a_kind_kernel<KM>, grid, dim3(256), lds, st, c.src, c.tgt, L, key_b, b.joint_kind, A, key_a, EA);
    else launch_lds(pose_lm_finish_a_kernel<KM>, grid, dim3(256), lds, st, c.src, c.tgt, L, key_b, A, key_a, EA);
    launch_tail_b<KM>(c, key_b, sq_threshold_f64(b.th), EB, st);
    return check_launch("pose_fit");
}

// The fused chain when both stages have problems and the schedule is not the eight-lane one (ANCSH_LM_LATENCY: another LM kernel);
// otherwise the stages' own chains, stage B first, as PoseSolver.solve issues the two calls.
template <int KM>
static int launch_fit(const FitCall &c, const FitExtras &EA, const FitExtras &EB) {
    const KeyArg<KM> key_a = key_arg<KM>(c.key_a, c.K), key_b = key_arg<KM>(c.key_b, c.K - 1);
    const bool run_a = c.a.present && c.a.nprob != 0, run_b = c.b.present && c.b.nprob != 0;
    if (run_a && run_b && c.b.lm_schedule != ANCSH_LM_LATENCY) return launch_fused<KM>(c, key_a, key_b, EA, EB);
    if (int rc = run_b ? launch_stage_b<KM>(c, key_b, EB) : ANCSH_OK) return rc;
    return run_a ? launch_stage_a<KM>(c, key_a, EA) : ANCSH_OK;
}

// The one checked path: every argument check of the stages that are present, before any launch.
static int pose_fit(const FitCall &c) {
    const StageA &a = c.a; const StageB &b = c.b;
    if (int rc = check_keys(c)) return rc;
    if (int rc = b.present ? check_joint_kind(c.who, b.nprob, b.joint_kind) : ANCSH_OK) return rc;
    // record columns and tie counts.  In a whole fit a stage without problems writes nothing: its record geometry and window are not examined
    FitExtras EA{}, EB{};                                   // all zero: no record, no tie counts, an empty window (no point is "borderline")
    if (a.present && !(whole_fit(c) && a.nprob == 0))
        if (int rc = make_extras(c, a.nprob, 1, a.tie, (double)a.th, (double)a.tie_window, EA)) return rc;
    if (b.present && !(whole_fit(c) && b.nprob == 0))
        if (int rc = make_extras(c, b.nprob, 2, b.tie, b.th, b.tie_window, EB)) return rc;
    EB.draws = b.draws; EB.seed = key_word(c.key_b);       // stage B's finish kernel re-draws the contenders' samples for the tie count
    if (int rc = a.present ? ransac_single_check(c) : ANCSH_OK) return rc;
    if (int rc = b.present ? ransac_joint_check(c) : ANCSH_OK) return rc;
    switch (key_mode(c)) {
    case KEY_DSEED: return launch_fit<KEY_DSEED>(c, EA, EB);
    case KEY_DKEY: return launch_fit<KEY_DKEY>(c, EA, EB);
    default: return launch_fit<KEY_VALUE>(c, EA, EB);
    }
}

// ---- the entries.  A stage's fields are filled in the order of StageA / StageB, which is the order of the parameters ------------------
extern "C" int ancsh_ransac_single(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter, const int *draws,
        unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers, int *out_best, int *scratch_scores, void *stream) {
    return pose_fit(FitCall{"ransac_single", src, tgt, max_n, nullptr, 0, stream,
                            StageA{true, nprob, off, inlier_th, niter, draws, out_model, out_inliers, out_best, scratch_scores},
                            FitKey{KEY_VALUE, seed}});
}

// ancsh_ransac_single with the hypotheses scored from SCALAR registers, out of a quad copy of the parts in scratch_quads: the same bits
extern "C" int ancsh_ransac_single_ex(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter, const int *draws,
        unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers, int *out_best, int *scratch_scores, float *scratch_quads,
        long rows, void *stream) {
    ANCSH_REQUIRE(scratch_quads, "ransac_single_ex: scratch_quads is NULL (ancsh_ransac_single is the call without it)");
    return pose_fit(FitCall{"ransac_single_ex", src, tgt, max_n, nullptr, 0, stream,
                            StageA{true, nprob, off, inlier_th, niter, draws, out_model, out_inliers, out_best, scratch_scores, scratch_quads, rows},
                            FitKey{KEY_VALUE, seed}});
}

// ancsh_ransac_single_ex (scratch_quads != NULL) / ancsh_ransac_single (NULL) that ALSO writes each fit straight into the pose record
// and / or reports how tie-sensitive it is (FitExtras above; include/ancsh_hip.h).  Everything else bit for bit as before.
extern "C" int ancsh_ransac_single_rec(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter, const int *draws,
        unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers, int *out_best, int *scratch_scores, float *scratch_quads,
        long rows, double *record, int K, int *tie_stats, float tie_window, void *stream) {
    return pose_fit(FitCall{"ransac_single_rec", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob, off, inlier_th, niter, draws, out_model, out_inliers, out_best, scratch_scores, scratch_quads, rows,
                                    tie_stats, tie_window}, FitKey{KEY_VALUE, seed}});
}

// ... with the generator key read from device memory (include/ancsh_hip.h): the kernels are the by-value ones instantiated with KEY_DSEED,
// the key travels as the address in the same 64-bit argument
extern "C" int ancsh_ransac_single_rec_dseed(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
        const int *draws, const unsigned long long *seed, int max_n, double *out_model, unsigned char *out_inliers, int *out_best,
        int *scratch_scores, float *scratch_quads, long rows, double *record, int K, int *tie_stats, float tie_window, void *stream) {
    return pose_fit(FitCall{"ransac_single_rec_dseed", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob, off, inlier_th, niter, draws, out_model, out_inliers, out_best, scratch_scores, scratch_quads, rows,
                                    tie_stats, tie_window}, FitKey{KEY_DSEED, 0, seed}});
}

// ... with the key block of include/ancsh_hip.h (ancsh_stream_key): the KEY_DKEY instantiations, whose generator problem index is
// prob + key->cloud_base * K (stage A) / prob + key->cloud_base * (K - 1) (stage B)
extern "C" int ancsh_ransac_single_rec_dkey(int nprob, const int *off, const float *src, const float *tgt, float inlier_th, int niter,
        const int *draws, const ancsh_stream_key *key, int max_n, double *out_model, unsigned char *out_inliers, int *out_best, int *scratch_scores,
        float *scratch_quads, long rows, double *record, int K, int *tie_stats, float tie_window, void *stream) {
    return pose_fit(FitCall{"ransac_single_rec_dkey", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob, off, inlier_th, niter, draws, out_model, out_inliers, out_best, scratch_scores, scratch_quads, rows,
                                    tie_stats, tie_window}, FitKey{KEY_DKEY, 0, key}});
}

extern "C" int ancsh_ransac_joint(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt, const float *joint_dir,
        double inlier_th, int niter, const int *draws, unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
        int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, void *stream) {
    return pose_fit(FitCall{"ransac_joint", src, tgt, max_n, nullptr, 0, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, ANCSH_LM_AUTO}, FitKey{KEY_VALUE, seed}});
}

extern "C" int ancsh_ransac_joint_ex(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt, const float *joint_dir,
        double inlier_th, int niter, const int *draws, unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
        int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, void *stream) {
    return pose_fit(FitCall{"ransac_joint_ex", src, tgt, max_n, nullptr, 0, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule}, FitKey{KEY_VALUE, seed}});
}

extern "C" int ancsh_ransac_joint_rec(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt, const float *joint_dir,
        double inlier_th, int niter, const int *draws, unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
        int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
        int *tie_stats, double tie_window, void *stream) {
    return pose_fit(FitCall{"ransac_joint_rec", src, tgt, max_n, record, K, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule, tie_stats, tie_window}, FitKey{KEY_VALUE, seed}});
}

extern "C" int ancsh_ransac_joint_rec_dseed(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt, const float *joint_dir,
        double inlier_th, int niter, const int *draws, const unsigned long long *seed, int max_n, double *out_model, unsigned char *out_inliers,
        int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
        int *tie_stats, double tie_window, void *stream) {
    return pose_fit(FitCall{"ransac_joint_rec_dseed", src, tgt, max_n, record, K, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule, tie_stats, tie_window}, FitKey{KEY_DSEED, 0, seed}});
}

extern "C" int ancsh_ransac_joint_rec_dkey(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt, const float *joint_dir,
        double inlier_th, int niter, const int *draws, const ancsh_stream_key *key, int max_n, double *out_model, unsigned char *out_inliers,
        int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
        int *tie_stats, double tie_window, void *stream) {
    return pose_fit(FitCall{"ransac_joint_rec_dkey", src, tgt, max_n, record, K, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule, tie_stats, tie_window}, FitKey{KEY_DKEY, 0, key}});
}

// The three record entries with a joint kind per problem (ABI 14, include/ancsh_hip.h): joint_kind NULL = the entry without it.
extern "C" int ancsh_ransac_joint_rec_kind(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt, const float *joint_dir,
        double inlier_th, int niter, const int *draws, unsigned long long seed, int max_n, double *out_model, unsigned char *out_inliers,
        int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule, double *record, int K,
        int *tie_stats, double tie_window, const int *joint_kind, void *stream) {
    return pose_fit(FitCall{"ransac_joint_rec_kind", src, tgt, max_n, record, K, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule, tie_stats, tie_window, joint_kind},
                            FitKey{KEY_VALUE, seed}});
}

extern "C" int ancsh_ransac_joint_rec_dseed_kind(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
        const float *joint_dir, double inlier_th, int niter, const int *draws, const unsigned long long *seed, int max_n, double *out_model,
        unsigned char *out_inliers, int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule,
        double *record, int K, int *tie_stats, double tie_window, const int *joint_kind, void *stream) {
    return pose_fit(FitCall{"ransac_joint_rec_dseed_kind", src, tgt, max_n, record, K, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule, tie_stats, tie_window, joint_kind},
                            FitKey{KEY_DSEED, 0, seed}});
}

extern "C" int ancsh_ransac_joint_rec_dkey_kind(int nprob, const int *rng0, const int *rng1, const float *src, const float *tgt,
        const float *joint_dir, double inlier_th, int niter, const int *draws, const ancsh_stream_key *key, int max_n, double *out_model,
        unsigned char *out_inliers, int *out_best, double *out_score, double *scratch_scores, double *scratch_models, int *lm_stat, int lm_schedule,
        double *record, int K, int *tie_stats, double tie_window, const int *joint_kind, void *stream) {
    return pose_fit(FitCall{"ransac_joint_rec_dkey_kind", src, tgt, max_n, record, K, stream, StageA{}, FitKey{},
                            StageB{true, nprob, rng0, rng1, joint_dir, inlier_th, niter, draws, out_model, out_inliers, out_best, out_score,
                                    scratch_scores, scratch_models, lm_stat, lm_schedule, tie_stats, tie_window, joint_kind},
                            FitKey{KEY_DKEY, 0, key}});
}

// ---- the whole fit in one call: ancsh_ransac_single_rec*'s arguments without record / K, ancsh_ransac_joint_rec*'s without src / tgt /
// max_n / record / K, then record, K and, in the *_kind entries, joint_kind.  Both stages are present, with or without problems.
extern "C" int ancsh_pose_fit_rec(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a, const int *draws_a,
        unsigned long long key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a, int *scratch_scores_a,
        float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0, const int *rng1, const float *joint_dir,
        double inlier_th_b, int niter_b, const int *draws_b, unsigned long long key_b, double *out_model_b, unsigned char *out_inliers_b,
        int *out_best_b, double *out_score_b, double *scratch_scores_b, double *scratch_models_b, int *lm_stat, int lm_schedule, int *tie_stats_b,
        double tie_window_b, double *record, int K, void *stream) {
    return pose_fit(FitCall{"pose_fit_rec", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob_a, off, inlier_th_a, niter_a, draws_a, out_model_a, out_inliers_a, out_best_a, scratch_scores_a,
                                    scratch_quads, rows, tie_stats_a, tie_window_a}, FitKey{KEY_VALUE, key_a},
                            StageB{true, nprob_b, rng0, rng1, joint_dir, inlier_th_b, niter_b, draws_b, out_model_b, out_inliers_b, out_best_b,
                                    out_score_b, scratch_scores_b, scratch_models_b, lm_stat, lm_schedule, tie_stats_b, tie_window_b},
                            FitKey{KEY_VALUE, key_b}});
}

extern "C" int ancsh_pose_fit_rec_dseed(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const unsigned long long *key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0, const int *rng1,
        const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const unsigned long long *key_b, double *out_model_b,
        unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b, double *scratch_models_b, int *lm_stat,
        int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K, void *stream) {
    return pose_fit(FitCall{"pose_fit_rec_dseed", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob_a, off, inlier_th_a, niter_a, draws_a, out_model_a, out_inliers_a, out_best_a, scratch_scores_a,
                                    scratch_quads, rows, tie_stats_a, tie_window_a}, FitKey{KEY_DSEED, 0, key_a},
                            StageB{true, nprob_b, rng0, rng1, joint_dir, inlier_th_b, niter_b, draws_b, out_model_b, out_inliers_b, out_best_b,
                                    out_score_b, scratch_scores_b, scratch_models_b, lm_stat, lm_schedule, tie_stats_b, tie_window_b},
                            FitKey{KEY_DSEED, 0, key_b}});
}

extern "C" int ancsh_pose_fit_rec_dkey(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const ancsh_stream_key *key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0, const int *rng1,
        const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const ancsh_stream_key *key_b, double *out_model_b,
        unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b, double *scratch_models_b, int *lm_stat,
        int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K, void *stream) {
    return pose_fit(FitCall{"pose_fit_rec_dkey", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob_a, off, inlier_th_a, niter_a, draws_a, out_model_a, out_inliers_a, out_best_a, scratch_scores_a,
                                    scratch_quads, rows, tie_stats_a, tie_window_a}, FitKey{KEY_DKEY, 0, key_a},
                            StageB{true, nprob_b, rng0, rng1, joint_dir, inlier_th_b, niter_b, draws_b, out_model_b, out_inliers_b, out_best_b,
                                    out_score_b, scratch_scores_b, scratch_models_b, lm_stat, lm_schedule, tie_stats_b, tie_window_b},
                            FitKey{KEY_DKEY, 0, key_b}});
}

extern "C" int ancsh_pose_fit_rec_kind(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, unsigned long long key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0, const int *rng1,
        const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, unsigned long long key_b, double *out_model_b,
        unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b, double *scratch_models_b, int *lm_stat,
        int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K, const int *joint_kind, void *stream) {
    return pose_fit(FitCall{"pose_fit_rec_kind", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob_a, off, inlier_th_a, niter_a, draws_a, out_model_a, out_inliers_a, out_best_a, scratch_scores_a,
                                    scratch_quads, rows, tie_stats_a, tie_window_a}, FitKey{KEY_VALUE, key_a},
                            StageB{true, nprob_b, rng0, rng1, joint_dir, inlier_th_b, niter_b, draws_b, out_model_b, out_inliers_b, out_best_b,
                                    out_score_b, scratch_scores_b, scratch_models_b, lm_stat, lm_schedule, tie_stats_b, tie_window_b, joint_kind},
                            FitKey{KEY_VALUE, key_b}});
}

extern "C" int ancsh_pose_fit_rec_dseed_kind(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const unsigned long long *key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0, const int *rng1,
        const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const unsigned long long *key_b, double *out_model_b,
        unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b, double *scratch_models_b, int *lm_stat,
        int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K, const int *joint_kind, void *stream) {
    return pose_fit(FitCall{"pose_fit_rec_dseed_kind", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob_a, off, inlier_th_a, niter_a, draws_a, out_model_a, out_inliers_a, out_best_a, scratch_scores_a,
                                    scratch_quads, rows, tie_stats_a, tie_window_a}, FitKey{KEY_DSEED, 0, key_a},
                            StageB{true, nprob_b, rng0, rng1, joint_dir, inlier_th_b, niter_b, draws_b, out_model_b, out_inliers_b, out_best_b,
                                    out_score_b, scratch_scores_b, scratch_models_b, lm_stat, lm_schedule, tie_stats_b, tie_window_b, joint_kind},
                            FitKey{KEY_DSEED, 0, key_b}});
}

extern "C" int ancsh_pose_fit_rec_dkey_kind(int nprob_a, const int *off, const float *src, const float *tgt, float inlier_th_a, int niter_a,
        const int *draws_a, const ancsh_stream_key *key_a, int max_n, double *out_model_a, unsigned char *out_inliers_a, int *out_best_a,
        int *scratch_scores_a, float *scratch_quads, long rows, int *tie_stats_a, float tie_window_a, int nprob_b, const int *rng0, const int *rng1,
        const float *joint_dir, double inlier_th_b, int niter_b, const int *draws_b, const ancsh_stream_key *key_b, double *out_model_b,
        unsigned char *out_inliers_b, int *out_best_b, double *out_score_b, double *scratch_scores_b, double *scratch_models_b, int *lm_stat,
        int lm_schedule, int *tie_stats_b, double tie_window_b, double *record, int K, const int *joint_kind, void *stream) {
    return pose_fit(FitCall{"pose_fit_rec_dkey_kind", src, tgt, max_n, record, K, stream,
                            StageA{true, nprob_a, off, inlier_th_a, niter_a, draws_a, out_model_a, out_inliers_a, out_best_a, scratch_scores_a,
                                    scratch_quads, rows, tie_stats_a, tie_window_a}, FitKey{KEY_DKEY, 0, key_a},
                            StageB{true, nprob_b, rng0, rng1, joint_dir, inlier_th_b, niter_b, draws_b, out_model_b, out_inliers_b, out_best_b,
                                    out_score_b, scratch_scores_b, scratch_models_b, lm_stat, lm_schedule, tie_stats_b, tie_window_b, joint_kind},
                            FitKey{KEY_DKEY, 0, key_b}});
}
