// pose_glue.hip -- what surrounds the pose fit of pose.hip: the ordered partition of a cloud by part label, the NaN poisoning of a
// non-finite cloud's records, the joint-direction medians, Umeyama alignment and the 5-point Umeyama RANSAC.
//
// Reference (host Python):
//   evaluation/parallel_ancsh_pose.py:238-341  per-cloud orchestration (argmax labels, per-part gathers, joint-axis medians)
//   lib/aligning.py:17-32,485-547,580-622      estimateSimilarityTransform, getRANSACInliers, estimateSimilarityUmeyama
#include "common.h"
#include "pose_math.h"
#include "umeyama_fit.h"
#include "pose_shared.h"

namespace ancsh {
namespace pose {

// ================================ glue kernels =====================================================
// labels = argmax(W, axis=1) (first maximum wins, np.argmax); ordered partition of the cloud's points
// by label; gather of the per-part source (own part-NOCS slot) / target (camera point) arrays
// (evaluation/parallel_ancsh_pose.py:238-242,259-260).
__global__ __launch_bounds__(256) void partition_kernel(int n, int K, const float *__restrict__ W, const float *__restrict__ P,
                                                        const float *__restrict__ nocs, int *__restrict__ labels,
                                                        int *__restrict__ part_index, int *__restrict__ off,
                                                        float *__restrict__ src, float *__restrict__ tgt,
                                                        int *__restrict__ counts, int *__restrict__ rng0, int *__restrict__ rng1) {
    __shared__ int wcnt[4];
    __shared__ int part_start[17];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *Wb = W + (size_t)b * n * K;
    int base = 0;
    for (int j = 0; j < K; ++j) {
        if (threadIdx.x == 0) { off[b * K + j] = b * n + base; part_start[j] = b * n + base; }
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int i = c0 + threadIdx.x;
            bool f = false;
            if (i < n) {
                int lab = 0;
                float bv = Wb[(size_t)i * K];
                for (int k = 1; k < K; ++k) {
                    const float v = Wb[(size_t)i * K + k];
                    if (v > bv) { bv = v; lab = k; }
                }
                f = lab == j;
                if (f && labels) labels[(size_t)b * n + i] = lab;
            }
            const unsigned long long m = __ballot(f);
            __syncthreads();
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int start = base;
            for (int w = 0; w < wave; ++w) start += wcnt[w];
            if (f) {
                const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                const size_t row = (size_t)b * n + pos;
                part_index[row] = i;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    src[row * 3 + c] = nocs[((size_t)b * n + i) * 3 * K + 3 * j + c];
                    tgt[row * 3 + c] = P[((size_t)b * n + i) * 3 + c];
                }
            }
            base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        }
    }
    if (threadIdx.x == 0 && b == gridDim.x - 1) off[gridDim.x * K] = gridDim.x * n;
    // optional by-products the joint stage consumes (:274-283): points per part and the [start, end) row ranges of part 0 /
    // part j for every joint j = 1..K-1 -- written here instead of by slicing / stacking `off` in separate launches
    if (threadIdx.x == 0) part_start[K] = (b + 1) * n;
    __syncthreads();
    if ((int)threadIdx.x < K && counts) counts[b * K + threadIdx.x] = part_start[threadIdx.x + 1] - part_start[threadIdx.x];
    if ((int)threadIdx.x >= 1 && (int)threadIdx.x < K && rng0 && rng1) {
        const int q = b * (K - 1) + (int)threadIdx.x - 1;
        rng0[q * 2] = part_start[0]; rng0[q * 2 + 1] = part_start[1];
        rng1[q * 2] = part_start[threadIdx.x]; rng1[q * 2 + 1] = part_start[threadIdx.x + 1];
    }
}

// A cloud with a non-finite value anywhere in the fit's inputs has no defined pose (the reference's own np.linalg.svd raises
// LinAlgError on it, np.argmax / np.median of NaN rows are arbitrary): its (K, 26) record rows become NaN, whatever the fit kernels
// made of it -- a poisoned cloud never yields a silently finite answer.  One workgroup per cloud; axis may be NULL.
// IDX (the predicted joint association): the (n, jc) index head is scanned as well; the plain instantiation never reads index / jc.
template <bool IDX>
__global__ __launch_bounds__(1024) void poison_records_kernel(int n, int K, const float *__restrict__ P, const float *__restrict__ nocs,
                                                              const float *__restrict__ W, const float *__restrict__ axis,
                                                              double *__restrict__ record, int jc, const float *__restrict__ index) {
    const int b = blockIdx.x;
    bool bad = false;
    // 1024 threads, eight independent loads in flight per thread: the scan is a handful of memory latencies, not a per-element loop
    const auto scan = [&](const float *p, long cnt) {
        for (long i0 = threadIdx.x; i0 < cnt; i0 += 8 * 1024) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[i0 + u * 1024 < cnt ? i0 + u * 1024 : i0];
#pragma unroll
            for (int u = 0; u < 8; ++u) bad = bad | !(fabsf(v[u]) <= 3.4028234664e38f);      // NaN and +-Inf fail the compare
        }
    };
    scan(P + (size_t)b * n * 3, (long)n * 3);
    scan(nocs + (size_t)b * n * 3 * K, (long)n * 3 * K);
    scan(W + (size_t)b * n * K, (long)n * K);
    if (axis) scan(axis + (size_t)b * n * 3, (long)n * 3);
    if (IDX) scan(index + (size_t)b * n * jc, (long)n * jc);
    if (__syncthreads_or(bad))
        for (int i = threadIdx.x; i < K * 26; i += 1024) record[(size_t)b * K * 26 + i] = __builtin_nan("");
}

// ---- the passes of the joint-direction medians, shared by joint_direction_kernel and joint_direction_pred_kernel.  STATEMENT MACROS
// (as csrc/part_stats.h): expanded in place they give joint_direction_kernel the instruction stream it had before the second kernel.
// ANCSH_JD_COMPACT: ordered compaction of cloud b's points whose IS_J (a boolean expression of the point index i, evaluated only for
// i < n) holds into three LDS columns of npow2 floats (joint_axis rows, in point order); cnt ends as their number on every thread.
#define ANCSH_JD_COMPACT(IS_J)                                                                                                        \
    for (int c0 = 0; c0 < n; c0 += 256) {                                                                                             \
        const int i = c0 + threadIdx.x;                                                                                               \
        const bool f = i < n && (IS_J);                                                                                               \
        const unsigned long long m = __ballot(f);                                                                                     \
        __syncthreads();                                                                                                              \
        if (lane == 0) wcnt[wave] = __popcll(m);                                                                                      \
        __syncthreads();                                                                                                              \
        int start = cnt;                                                                                                              \
        for (int w = 0; w < wave; ++w) start += wcnt[w];                                                                              \
        if (f) {                                                                                                                      \
            const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));       \
            _Pragma("unroll") for (int c = 0; c < 3; ++c) vals[c * npow2 + pos] = axis[((size_t)b * n + i) * 3 + c];                 \
        }                                                                                                                             \
        cnt += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];                                                                                 \
    }
// ANCSH_JD_MEDIAN: +inf padding to the next power of two, a bitonic sort of each column, and np.median of each (the middle element or
// the float32 mean of the middle two; NaN without a point) into out[b, j - 1, :]
#define ANCSH_JD_MEDIAN                                                                                                               \
    int p2 = 1;                                                                                                                       \
    while (p2 < cnt) p2 <<= 1;                                                                                                        \
    for (int e = cnt + threadIdx.x; e < p2; e += 256)                                                                                 \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) vals[c * npow2 + e] = INFINITY;                                                 \
    __syncthreads();                                                                                                                  \
    for (int k = 2; k <= p2; k <<= 1)                                                                                                 \
        for (int s = k >> 1; s > 0; s >>= 1) {                                                                                        \
            for (int e = threadIdx.x; e < p2; e += 256) {                                                                             \
                const int partner = e ^ s;                                                                                            \
                if (partner > e) {                                                                                                    \
                    const bool up = (e & k) == 0;                                                                                     \
                    _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                                                   \
                        float *v = vals + c * npow2;                                                                                  \
                        const float a = v[e], bb = v[partner];                                                                       \
                        if ((a > bb) == up) { v[e] = bb; v[partner] = a; }                                                            \
                    }                                                                                                                 \
                }                                                                                                                     \
            }                                                                                                                         \
            __syncthreads();                                                                                                          \
        }                                                                                                                             \
    if (threadIdx.x < 3) {                                                                                                            \
        const float *v = vals + threadIdx.x * npow2;                                                                                  \
        float med = NAN;                                                                                                              \
        if (cnt > 0) med = (cnt & 1) ? v[cnt / 2] : (v[cnt / 2 - 1] + v[cnt / 2]) * 0.5f;                                             \
        out[((size_t)b * (K - 1) + (j - 1)) * 3 + threadIdx.x] = med;                                                                 \
    }

// jt_axis = np.median(joint_axis_per_point[joint_cls == j], 0)  (:295): one workgroup per (cloud, joint)
__global__ __launch_bounds__(256) void joint_direction_kernel(int n, int K, const float *__restrict__ axis,
                                                              const int *__restrict__ joint_cls, float *__restrict__ out) {
    extern __shared__ float vals[];   // 3 * npow2 floats
    __shared__ int wcnt[4];
    const int b = blockIdx.x, j = blockIdx.y + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    int cnt = 0;
    ANCSH_JD_COMPACT(joint_cls[(size_t)b * n + i] == j)
    ANCSH_JD_MEDIAN
}

// np.argmax of one row of jc floats: the first maximum, and the first NaN when the row holds one (numpy treats NaN as the maximum)
__device__ __forceinline__ int np_argmax_row(const float *r, int jc) {
    int c = 0;
    float best = r[0];
    for (int k = 1; k < jc && best == best; ++k) {
        const float v = r[k];
        if (!(v <= best)) { best = v; c = k; }     // v > best, or v is NaN
    }
    return c;
}

// jt_axis = np.median(joint_axis_per_point[np.argmax(index_per_point, 1) == j], 0)  (lib/parallel_ancsh_pose.py:339-343,366): the joint
// association from the ANCSH network's index head (jc channels per point) instead of a label array, the argmax taken while compacting --
// the bytes of joint_direction_kernel fed np.argmax(index, -1).  One workgroup per (cloud, joint).
__global__ __launch_bounds__(256) void joint_direction_pred_kernel(int n, int K, int jc, const float *__restrict__ axis,
                                                                   const float *__restrict__ index, float *__restrict__ out) {
    extern __shared__ float vals[];   // 3 * npow2 floats
    __shared__ int wcnt[4];
    const int b = blockIdx.x, j = blockIdx.y + 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    int cnt = 0;
    ANCSH_JD_COMPACT(np_argmax_row(index + ((size_t)b * n + i) * jc, jc) == j)
    ANCSH_JD_MEDIAN
}

// estimateSimilarityUmeyama (lib/aligning.py:580-622) for a batch of (source, target) point sets, float64.
// out (nprob, 29): Scales(3) | Rotation(9, the reference's TRANSPOSED matrix) | Translation(3) | OutTransform(4x4 row-major minus last row -> 12) ... see header
#define UMK_SRC(i, c) src[(size_t)(r0 + (i)) * 3 + (c)]
#define UMK_TGT(i, c) tgt[(size_t)(r0 + (i)) * 3 + (c)]
__global__ __launch_bounds__(256) void umeyama_kernel(const int *__restrict__ off, const float *__restrict__ src,
                                                      const float *__restrict__ tgt, double *__restrict__ out) {
    __shared__ double red[64];
    const int prob = blockIdx.x, r0 = off[prob], n = off[prob + 1] - r0;
    double *o = out + (size_t)prob * 32;
    if (n <= 0) {
        if (threadIdx.x < 32) o[threadIdx.x] = NAN;
        return;
    }
    ANCSH_UMEYAMA_SUMS(n, UMK_SRC, UMK_TGT, red)        // the arithmetic is stated in umeyama_fit.h, for this kernel and gt_pose_kernel
    if (threadIdx.x != 0) return;
    ANCSH_UMEYAMA_SOLVE(n, o)
}

// estimateSimilarityTransform (lib/aligning.py:17-32): 5-point Umeyama RANSAC (getRANSACInliers :485-507 with
// evaluateModel :540-547 and set_config :88-103), <= 100 iterations with the reference's SEQUENTIAL early stop,
// then Umeyama on the winner's inliers.  One workgroup per problem: thread h evaluates hypothesis h against all
// points (every hypothesis is independent), thread 0 then replays the reference's in-order bookkeeping
// (strictly-better inlier ratio wins; stop as soon as the best residual drops under StopThreshold) to find which
// hypothesis the sequential loop would have kept; the workgroup refits on its inliers.
// Quirk kept: nInliers = np.count_nonzero(InlierIdx) counts non-zero INDICES, so point 0 never counts (:544).
__device__ __forceinline__ void umeyama_small(const double (*s)[3], const double (*t)[3], int n, double T[12]) {
    double sm[3] = {0, 0, 0}, tm[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) { sm[c] += s[i][c]; tm[c] += t[i][c]; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { sm[c] /= n; tm[c] /= n; }
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var = 0.0;
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) M[a * 3 + b] += (t[i][a] - tm[a]) * (s[i][b] - sm[b]);
            var += (s[i][a] - sm[a]) * (s[i][a] - sm[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) M[a] /= n;
    var /= n;
    double q[4], R[9];
    horn_quat(M, q);
    quat_to_mat(q, R);
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) tr += R[a] * M[a];
    const double sc = tr / var;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) T[a * 4 + b] = sc * R[a * 3 + b];
        T[a * 4 + 3] = tm[a] - sc * (R[a * 3] * sm[0] + R[a * 3 + 1] * sm[1] + R[a * 3 + 2] * sm[2]);
    }
}

__global__ __launch_bounds__(128) void ransac_umeyama5_kernel(const int *__restrict__ off, const float *__restrict__ src,
                                                              const float *__restrict__ tgt, int niter,
                                                              const int *__restrict__ draws, unsigned long long seed,
                                                              double *__restrict__ out, int *__restrict__ status) {
    __shared__ double red[64];
    __shared__ double h_res[128], h_ratio[128];
    __shared__ double Tsel[12];
    __shared__ double thr[2];
    __shared__ int sel;
    const int prob = blockIdx.x, r0 = off[prob], n = off[prob + 1] - r0, h = threadIdx.x;
    double *o = out + (size_t)prob * 32;
    if (n <= 0 || niter > 128) {
        if (h < 32) o[h] = NAN;
        if (h == 0) status[prob] = -1;
        return;
    }
    // set_config: PassT = max(TargetNorm/SourceNorm, SourceNorm/TargetNorm) of the mean point norms; StopT = PassT/100
    double nm[2] = {0, 0};
    for (int i = h; i < n; i += 128) {
        const float *ps = src + (size_t)(r0 + i) * 3, *pt = tgt + (size_t)(r0 + i) * 3;
        nm[0] += sqrt((double)ps[0] * ps[0] + (double)ps[1] * ps[1] + (double)ps[2] * ps[2]);
        nm[1] += sqrt((double)pt[0] * pt[0] + (double)pt[1] * pt[1] + (double)pt[2] * pt[2]);
    }
    block_sum<2>(nm, red, 2);
    if (h == 0) {
        const double ts = (nm[1] / n) / (nm[0] / n), st = (nm[0] / n) / (nm[1] / n);
        thr[0] = st > ts ? st : ts;
        thr[1] = thr[0] / 100.0;
    }
    __syncthreads();
    const double passT = thr[0], stopT = thr[1];
    double T[12];
    if (h < niter) {
        double s5[5][3], t5[5][3];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            int v = draws ? draws[((size_t)prob * niter + h) * 5 + k] : device_draw(seed, prob, h, k, n);
            v = v < 0 ? 0 : (v >= n ? n - 1 : v);
#pragma unroll
            for (int c = 0; c < 3; ++c) { s5[k][c] = src[(size_t)(r0 + v) * 3 + c]; t5[k][c] = tgt[(size_t)(r0 + v) * 3 + c]; }
        }
        umeyama_small(s5, t5, 5, T);
        double rs = 0.0;
        int cnt = 0;
        for (int i = 0; i < n; ++i) {
            const float *ps = src + (size_t)(r0 + i) * 3, *pt = tgt + (size_t)(r0 + i) * 3;
            double e2 = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double e = (double)pt[a] - (T[a * 4] * ps[0] + T[a * 4 + 1] * ps[1] + T[a * 4 + 2] * ps[2] + T[a * 4 + 3]);
                e2 += e * e;
            }
            rs += e2;                                   // Residual = norm(ResidualVec) = sqrt(sum of squared norms)
            if (sqrt(e2) < passT && i != 0) ++cnt;      // count_nonzero(InlierIdx): index 0 is never counted
        }
        h_res[h] = sqrt(rs);
        h_ratio[h] = (double)cnt / (double)n;
    }
    __syncthreads();
    if (h == 0) {
        double bestRes = 1e10, bestRatio = 0.0;
        int best = -1;                                   // -1: BestInlierIdx stays arange(n)
        for (int i = 0; i < niter; ++i) {
            if (h_ratio[i] > bestRatio) { bestRes = h_res[i]; bestRatio = h_ratio[i]; best = i; }
            if (bestRes < stopT) break;
        }
        sel = best;
        thr[0] = bestRatio;
    }
    __syncthreads();
    const int best = sel;
    const double bestRatio = thr[0];
    if (best >= 0 && h == best)
#pragma unroll
        for (int a = 0; a < 12; ++a) Tsel[a] = T[a];
    __syncthreads();
    if (bestRatio < 0.1) {                              // "[ WARN ] - Something is wrong. Small BestInlierRatio" -> 4 x None
        if (h < 32) o[h] = NAN;
        if (h == 0) status[prob] = 1;
        return;
    }
    // Umeyama over the winner's inliers (true inliers INCLUDING index 0: InlierIdx[0] holds it)
    double sums[7] = {0, 0, 0, 0, 0, 0, 0};
    auto is_in = [&](int i) {
        if (best < 0) return true;
        const float *ps = src + (size_t)(r0 + i) * 3, *pt = tgt + (size_t)(r0 + i) * 3;
        double e2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double e = (double)pt[a] - (Tsel[a * 4] * ps[0] + Tsel[a * 4 + 1] * ps[1] + Tsel[a * 4 + 2] * ps[2] + Tsel[a * 4 + 3]);
            e2 += e * e;
        }
        return sqrt(e2) < passT;
    };
    for (int i = h; i < n; i += 128)
        if (is_in(i)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { sums[c] += src[(size_t)(r0 + i) * 3 + c]; sums[3 + c] += tgt[(size_t)(r0 + i) * 3 + c]; }
            sums[6] += 1.0;
        }
    block_sum<7>(sums, red, 2);
    const double m = sums[6];
    double sm[3], tm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { sm[c] = sums[c] / m; tm[c] = sums[3 + c] / m; }
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = h; i < n; i += 128)
        if (is_in(i)) {
            double sc[3], tc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { sc[c] = src[(size_t)(r0 + i) * 3 + c] - sm[c]; tc[c] = tgt[(size_t)(r0 + i) * 3 + c] - tm[c]; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[a * 3 + b] += tc[a] * sc[b];
            acc[9] += sc[0] * sc[0] + sc[1] * sc[1] + sc[2] * sc[2];
        }
    block_sum<10>(acc, red, 2);
    if (h != 0) return;
    double M[9], q[4], R[9];
#pragma unroll
    for (int a = 0; a < 9; ++a) M[a] = acc[a] / m;
    horn_quat(M, q);
    quat_to_mat(q, R);
    double trace = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) trace += R[a] * M[a];
    const double s = trace / (acc[9] / m);
    o[0] = o[1] = o[2] = s;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) o[3 + a * 3 + b] = R[b * 3 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double Tv = tm[a] - s * (R[a * 3] * sm[0] + R[a * 3 + 1] * sm[1] + R[a * 3 + 2] * sm[2]);
        o[12 + a] = Tv;
#pragma unroll
        for (int b = 0; b < 3; ++b) o[15 + a * 4 + b] = s * R[a * 3 + b];
        o[15 + a * 4 + 3] = Tv;
    }
    o[27] = 0; o[28] = 0; o[29] = 0; o[30] = 1; o[31] = bestRatio;
    status[prob] = 0;
}

}  // namespace pose
}  // namespace ancsh

using namespace ancsh;
using namespace ancsh::pose;

extern "C" int ancsh_pose_partition(int b, int n, int K, const float *W, const float *P, const float *nocs, int *labels,
                                    int *part_index, int *off, float *src, float *tgt, int *counts, int *rng0, int *rng1,
                                    void *stream) {
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1 && K <= 16, "pose_partition: bad shape b=%d n=%d K=%d", b, n, K);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(W && P && nocs && part_index && off && src && tgt, "pose_partition: null pointer");
    ANCSH_REQUIRE((rng0 == nullptr) == (rng1 == nullptr), "pose_partition: rng0 and rng1 go together");
    hipLaunchKernelGGL(partition_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, n, K, W, P, nocs, labels, part_index, off,
                       src, tgt, counts, rng0, rng1);
    return check_launch("pose_partition");
}

extern "C" int ancsh_pose_poison_records(int b, int n, int K, const float *P, const float *nocs, const float *W, const float *joint_axis,
                                         double *record, void *stream) {
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1 && K <= 16, "pose_poison_records: bad shape b=%d n=%d K=%d", b, n, K);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(P && nocs && W && record, "pose_poison_records: null pointer");
    hipLaunchKernelGGL(poison_records_kernel<false>, dim3(b), dim3(1024), 0, (hipStream_t)stream, n, K, P, nocs, W, joint_axis, record, 0,
                       nullptr);
    return check_launch("pose_poison_records");
}

extern "C" int ancsh_pose_poison_records_pred(int b, int n, int K, const float *P, const float *nocs, const float *W,
                                              const float *joint_axis, int joint_channels, const float *joint_index, double *record,
                                              void *stream) {
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1 && K <= 16, "pose_poison_records_pred: bad shape b=%d n=%d K=%d", b, n, K);
    ANCSH_REQUIRE(joint_channels >= 1 && joint_channels <= 64, "pose_poison_records_pred: joint_channels=%d must be in [1,64]",
                  joint_channels);
    ANCSH_REQUIRE(P && nocs && W && joint_index && record, "pose_poison_records_pred: null pointer");
    if (b == 0) return ANCSH_OK;
    hipLaunchKernelGGL(poison_records_kernel<true>, dim3(b), dim3(1024), 0, (hipStream_t)stream, n, K, P, nocs, W, joint_axis, record,
                       joint_channels, joint_index);
    return check_launch("pose_poison_records_pred");
}

extern "C" int ancsh_pose_joint_direction(int b, int n, int K, const float *joint_axis, const int *joint_cls, float *out,
                                          void *stream) {
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 1, "pose_joint_direction: bad shape");
    ANCSH_REQUIRE(n <= 8192, "pose_joint_direction: n %d > 8192", n);
    if (b == 0 || K == 1) return ANCSH_OK;
    ANCSH_REQUIRE(joint_axis && joint_cls && out, "pose_joint_direction: null pointer");
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    launch_lds(joint_direction_kernel, dim3(b, K - 1), dim3(256), (size_t)3 * npow2 * sizeof(float), (hipStream_t)stream, n, K, joint_axis,
               joint_cls, out);
    return check_launch("pose_joint_direction");
}

extern "C" int ancsh_pose_joint_direction_pred(int b, int n, int K, int joint_channels, const float *joint_axis, const float *joint_index,
                                               float *out, void *stream) {
    ANCSH_REQUIRE(b >= 0 && n > 0 && K >= 2 && K <= 16, "pose_joint_direction_pred: bad shape b=%d n=%d K=%d (K >= 2: a joint)", b, n, K);
    ANCSH_REQUIRE(n <= 8192, "pose_joint_direction_pred: n %d > 8192", n);
    ANCSH_REQUIRE(joint_channels >= 1 && joint_channels <= 64, "pose_joint_direction_pred: joint_channels=%d must be in [1,64]",
                  joint_channels);
    ANCSH_REQUIRE(joint_axis && joint_index && out, "pose_joint_direction_pred: null pointer");
    if (b == 0) return ANCSH_OK;
    int npow2 = 1;
    while (npow2 < n) npow2 <<= 1;
    launch_lds(joint_direction_pred_kernel, dim3(b, K - 1), dim3(256), (size_t)3 * npow2 * sizeof(float), (hipStream_t)stream, n, K,
               joint_channels, joint_axis, joint_index, out);
    return check_launch("pose_joint_direction_pred");
}

extern "C" int ancsh_umeyama(int nprob, const int *off, const float *src, const float *tgt, double *out, void *stream) {
    ANCSH_REQUIRE(nprob >= 0, "umeyama: negative nprob");
    if (nprob == 0) return ANCSH_OK;
    ANCSH_REQUIRE(off && src && tgt && out, "umeyama: null pointer");
    hipLaunchKernelGGL(umeyama_kernel, dim3(nprob), dim3(256), 0, (hipStream_t)stream, off, src, tgt, out);
    return check_launch("umeyama");
}

extern "C" int ancsh_estimate_similarity_transform(int nprob, const int *off, const float *src, const float *tgt, int niter,
                                                   const int *draws, unsigned long long seed, double *out, int *status,
                                                   void *stream) {
    ANCSH_REQUIRE(nprob >= 0 && niter > 0 && niter <= 128, "estimate_similarity_transform: niter %d outside 1..128", niter);
    if (nprob == 0) return ANCSH_OK;
    ANCSH_REQUIRE(off && src && tgt && out && status, "estimate_similarity_transform: null pointer");
    hipLaunchKernelGGL(ransac_umeyama5_kernel, dim3(nprob), dim3(128), 0, (hipStream_t)stream, off, src, tgt, niter, draws, seed,
                       out, status);
    return check_launch("estimate_similarity_transform");
}
