// fit_quality.hip -- how good the poses of a pose record are: per (cloud, part) the points of the part, the stage-A winner's consensus
// count, the stage-B winner's score and, for the baseline pose (record columns 0..12) and the nonlinear pose (13..25), the verifier's
// residual norm of EVERY point of the part (evaluation/parallel_ancsh_pose.py:51-52, 189-192) reduced to five numbers: inliers at
// inlier_th, mean, RMS, median, max.  One launch behind the fit and the record poison; it carries the record along in columns 0..25 of its
// (b, K, 39) block.
//
// One workgroup of 256 threads per (cloud, part); it reads the packed src / tgt rows ancsh_pose_partition wrote (the rows both fit stages
// read).  Pass 1 reads every row once and computes both poses' residuals: count, sum, sum of squares and max accumulate lane-strided, are
// reduced over the wave by xor butterflies and over the four waves in LDS in a fixed order, so the bytes do not depend on the run, on b or
// on where the part lies in the batch.  The baseline residuals' bit patterns stay in LDS (8192 x 8 B); a non-negative double orders like
// its bit pattern read as a 64-bit unsigned, so the median is an exact radix select over them (eight 8-bit digit histograms, integer LDS
// atomics: order-independent), the upper middle of an even part being the smallest residual above the lower one.  Pass 2 writes the
// nonlinear residuals over the buffer and selects again.  No atomics in global memory, no workgroup waits for another, nothing allocated,
// every size an argument or read on the device: capturable.
#include "common.h"

namespace ancsh {

constexpr int FQ_MAX_N = ANCSH_FIT_QUALITY_MAX_N;
constexpr int FQ_THREADS = 256;
constexpr int FQ_WIDTH = 39;

// The verifier's residual norm of one point under the pose m = [R (9, row-major) | s | t (3)], float64, evaluated as written:
//   y_c = (R_c0 x_0 + R_c1 x_1) + R_c2 x_2,  r_c = (tgt_c - s y_c) - t_c,  rho = sqrt((r_0^2 + r_1^2) + r_2^2)
__device__ __forceinline__ double fq_residual(const double *m, double x0, double x1, double x2, double g0, double g1, double g2) {
#pragma clang fp contract(off)
    const double y0 = (m[0] * x0 + m[1] * x1) + m[2] * x2;
    const double y1 = (m[3] * x0 + m[4] * x1) + m[5] * x2;
    const double y2 = (m[6] * x0 + m[7] * x1) + m[8] * x2;
    const double r0 = (g0 - m[9] * y0) - m[10];
    const double r1 = (g1 - m[9] * y1) - m[11];
    const double r2 = (g2 - m[9] * y2) - m[12];
    return sqrt((r0 * r0 + r1 * r1) + r2 * r2);
}

struct FqAcc {
    int inl;
    double sum, sq, mx;
};

__device__ __forceinline__ void fq_add(FqAcc &a, double rho, double th) {
#pragma clang fp contract(off)
    a.inl += rho < th ? 1 : 0;
    a.sum += rho;
    a.sq += rho * rho;
    a.mx = fmax(a.mx, rho);
}

struct FqShared {
    unsigned long long buf[FQ_MAX_N];      // one pose's residual norms, as bit patterns
    unsigned hist[256];
    unsigned wtot[4];
    int w_inl[2][4];
    double w_sum[2][4], w_sq[2][4], w_mx[2][4];
    unsigned long long next;               // the smallest key above the lower middle
    unsigned le;                           // keys <= the lower middle
    unsigned digit, rank;
};

// the wave's totals of one accumulator into LDS (xor butterfly: every lane ends with the same sum, added in the same order every run)
__device__ __forceinline__ void fq_wave_totals(FqShared &S, int p, FqAcc a, int lane, int wave) {
#pragma unroll
    for (int m = 32; m; m >>= 1) {
        a.inl += __shfl_xor(a.inl, m);
        a.sum += __shfl_xor(a.sum, m);
        a.sq += __shfl_xor(a.sq, m);
        a.mx = fmax(a.mx, __shfl_xor(a.mx, m));
    }
    if (lane == 0) {
        S.w_inl[p][wave] = a.inl;
        S.w_sum[p][wave] = a.sum;
        S.w_sq[p][wave] = a.sq;
        S.w_mx[p][wave] = a.mx;
    }
}

// The key of rank k (0-based, ascending) among S.buf[0..n): eight passes from the top byte down, each a 256-bin histogram of the keys
// that share the prefix found so far and an inclusive scan of it over the 256 threads.  Called by the whole workgroup, n >= 1, k < n.
__device__ unsigned long long fq_select(FqShared &S, int n, unsigned k, int tid, int lane, int wave) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        S.hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += FQ_THREADS) {
            const unsigned long long key = S.buf[i];
            if ((key & mask) == prefix) atomicAdd(&S.hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned c = S.hist[tid];
        unsigned inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) S.wtot[wave] = inc;
        __syncthreads();
        unsigned excl = inc - c;
        for (int w = 0; w < wave; ++w) excl += S.wtot[w];
        if (k >= excl && k < excl + c) {       // exactly one thread: the bins' counts add up to the keys under the prefix, and k is below that
            S.digit = (unsigned)tid;
            S.rank = k - excl;
        }
        __syncthreads();
        prefix |= (unsigned long long)S.digit << shift;
        mask |= 0xFFull << shift;
        k = S.rank;
    }
    return prefix;
}

// np.median of S.buf[0..n), n >= 1: the middle order statistic, or (a + b) / 2 of the two middle ones
__device__ double fq_median(FqShared &S, int n, int tid, int lane, int wave) {
    const unsigned long long lo = fq_select(S, n, (unsigned)(n - 1) >> 1, tid, lane, wave);
    if (n & 1) return __longlong_as_double((long long)lo);
    // even: rank n / 2 is the lower middle again when more than n / 2 keys are <= it, else the smallest key above it
    if (tid == 0) {
        S.le = 0;
        S.next = ~0ull;
    }
    __syncthreads();
    unsigned le = 0;
    unsigned long long next = ~0ull;
    for (int i = tid; i < n; i += FQ_THREADS) {
        const unsigned long long key = S.buf[i];
        if (key <= lo) ++le;
        else if (key < next) next = key;
    }
    atomicAdd(&S.le, le);
    atomicMin(&S.next, next);
    __syncthreads();
    const unsigned long long hi = S.le > (unsigned)(n >> 1) ? lo : S.next;
    return (__longlong_as_double((long long)lo) + __longlong_as_double((long long)hi)) / 2.0;
}

__global__ __launch_bounds__(FQ_THREADS) void fit_quality_kernel(int K, const int *__restrict__ off, const float *__restrict__ src,
                                                                 const float *__restrict__ tgt, const double *__restrict__ record,
                                                                 double inlier_th, const int *__restrict__ best_a,
                                                                 const double *__restrict__ score_b, double *__restrict__ wide) {
    __shared__ FqShared S;
    const int p = blockIdx.x, c = p / K, j = p - c * K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *rec = record + (size_t)p * 26;
    double *o = wide + (size_t)p * FQ_WIDTH;
    // columns 0..25: the record's row, moved as 64-bit words so that a NaN keeps its payload
    if (tid < 26) reinterpret_cast<unsigned long long *>(o)[tid] = reinterpret_cast<const unsigned long long *>(rec)[tid];
    const int r0 = off[p], n = off[p + 1] - r0;
    double m[2][13];
    bool dead[2] = {false, false};
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 13; ++e) {
            m[q][e] = rec[13 * q + e];
            dead[q] |= m[q][e] != m[q][e];
        }
    if (tid == 0) {
        o[26] = (double)n;
        o[27] = best_a ? (double)best_a[2 * p + 1] : NAN;
        o[33] = score_b && K > 1 ? score_b[(size_t)c * (K - 1) + (j > 0 ? j - 1 : 0)] : NAN;
    }
    // nothing to measure: an empty part, or one beyond the buffer (clamped here: off is not the host's to read)
    if (n < 1 || n > FQ_MAX_N) {
        dead[0] = dead[1] = true;
    }
    if (dead[0] && dead[1]) {
        if (tid < 5) {
            o[28 + tid] = NAN;
            o[34 + tid] = NAN;
        }
        return;
    }
    const float *s = src + (size_t)r0 * 3, *g = tgt + (size_t)r0 * 3;
    // ---- pass 1: both poses' residuals from one read of the rows; the baseline's stay in LDS
    FqAcc a0 = {0, 0.0, 0.0, 0.0}, a1 = {0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += FQ_THREADS) {
        const double x0 = s[3 * i], x1 = s[3 * i + 1], x2 = s[3 * i + 2], g0 = g[3 * i], g1 = g[3 * i + 1], g2 = g[3 * i + 2];
        if (!dead[0]) {
            const double rho = fq_residual(m[0], x0, x1, x2, g0, g1, g2);
            fq_add(a0, rho, inlier_th);
            S.buf[i] = (unsigned long long)__double_as_longlong(rho);
        }
        if (!dead[1]) fq_add(a1, fq_residual(m[1], x0, x1, x2, g0, g1, g2), inlier_th);
    }
    fq_wave_totals(S, 0, a0, lane, wave);
    fq_wave_totals(S, 1, a1, lane, wave);
    __syncthreads();
    if (tid < 2) {                             // thread q: pose q's count, mean, RMS and max from the four wave totals, in wave order
#pragma clang fp contract(off)
        const int q = tid;
        double *oq = o + 28 + 6 * q;
        if (dead[q]) {
            oq[0] = oq[1] = oq[2] = oq[4] = NAN;
        } else {
            oq[0] = (double)(((S.w_inl[q][0] + S.w_inl[q][1]) + S.w_inl[q][2]) + S.w_inl[q][3]);
            oq[1] = (((S.w_sum[q][0] + S.w_sum[q][1]) + S.w_sum[q][2]) + S.w_sum[q][3]) / (double)n;
            oq[2] = sqrt((((S.w_sq[q][0] + S.w_sq[q][1]) + S.w_sq[q][2]) + S.w_sq[q][3]) / (double)n);
            oq[4] = fmax(fmax(S.w_mx[q][0], S.w_mx[q][1]), fmax(S.w_mx[q][2], S.w_mx[q][3]));
        }
    }
    // ---- the medians: the baseline's from the buffer, then the nonlinear residuals over it (pass 2) and theirs
    double med0 = NAN, med1 = NAN;
    if (!dead[0]) med0 = fq_median(S, n, tid, lane, wave);
    if (!dead[1]) {
        __syncthreads();                       // every thread is done reading the baseline's keys
        for (int i = tid; i < n; i += FQ_THREADS)
            S.buf[i] = (unsigned long long)__double_as_longlong(
                fq_residual(m[1], s[3 * i], s[3 * i + 1], s[3 * i + 2], g[3 * i], g[3 * i + 1], g[3 * i + 2]));
        med1 = fq_median(S, n, tid, lane, wave);
    }
    if (tid == 0) {
        o[31] = med0;
        o[37] = med1;
    }
}

}  // namespace ancsh

extern "C" int ancsh_fit_quality_rec(int b, int K, const int *off, const float *src, const float *tgt, const double *record,
                                     double inlier_th, const int *best_a, const double *score_b, double *wide, void *stream) {
    using namespace ancsh;
    ANCSH_REQUIRE(b >= 0, "fit_quality_rec: b=%d (>= 0)", b);
    ANCSH_REQUIRE(K >= 1 && K <= 16, "fit_quality_rec: K=%d (1..16)", K);
    ANCSH_REQUIRE(inlier_th > 0.0 && inlier_th <= 1.7976931348623157e308, "fit_quality_rec: inlier_th=%g (finite, > 0)", inlier_th);
    ANCSH_REQUIRE((long)b * K <= 0x7fffffffL / FQ_WIDTH, "fit_quality_rec: b * K = %ld rows (39 doubles each) overflow an int", (long)b * K);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(off && src && tgt && record && wide, "fit_quality_rec: null pointer");
    hipLaunchKernelGGL(fit_quality_kernel, dim3(b * K), dim3(FQ_THREADS), 0, (hipStream_t)stream, K, off, src, tgt, record, inlier_th, best_a,
                       score_b, wide);
    return check_launch("fit_quality_rec");
}
