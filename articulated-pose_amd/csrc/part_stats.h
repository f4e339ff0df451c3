// part_stats.h -- per-part and per-joint statistics of one cloud, shared by the evaluation kernels of metrics.hip (joint_params_kernel,
// part_extents_kernel, articulation_kernel), by joint_state_kernel of joint_state.hip, gt_error_kernel of gt_errors.hip and the joint pass
// of point_gt.hip (workgroups of 256 threads, four waves of 64).  The passes stand in for numpy calls and follow numpy at the edges:
// np.argmax labels (argmax_first_nan), np.median of a column with a NaN (vote_above, ANCSH_VOTE_MEDIAN), np.std in two passes.
// The passes are STATEMENT MACROS, not inline functions: a force-inlined device function is simplified on its own before it is inlined,
// and that alone changes the code the compiler makes of the kernels that existed before this header (measured: part_extents_kernel
// 3830 -> 3642 instructions with its unchanged body behind one inline call).  Expanded in place, the macros give those kernels the
// instruction streams they had (profiles/r10_articulation_isa_compare.txt).  Each macro names every variable it reads or writes.
#pragma once
#include "common.h"

namespace ancsh {

// np.argmax of a row of C floats: the first maximum, or the first NaN (numpy and torch.argmax rank NaN above every number).  Every label
// of the evaluation kernels -- a point's part from its mask row, its joint class from the joint-index head -- is taken with this rule.
__device__ __forceinline__ int argmax_first_nan(const float *m, int C) {
    float best = m[0];
    if (best != best) return 0;
    int c = 0;
    for (int k = 1; k < C; ++k) {
        const float v = m[k];
        if (v != v) return k;
        if (v > best) { best = v; c = k; }
    }
    return c;
}

// a > b in numpy's sort order: NaN above +inf (NaNs equal among themselves)
__device__ __forceinline__ bool vote_above(float a, float b) { return a > b || (a != a && b == b); }

__device__ __forceinline__ double block_sum_f64(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// np.max / np.min PROPAGATE a NaN (compute_miou.py:196-208 takes np.max(abs(nocs - 0.5)) per part: a NaN prediction gives a NaN extent);
// fmaxf / fmin would drop it
__device__ __forceinline__ float np_maxf(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : fmin(a, b)); }

}  // namespace ancsh

// ---- similarity global NOCS -> part NOCS of part j (evaluation/eval_joint_params.py:160-171) ------------------------------------
//   x = global NOCS (G = 3 shared or 3K per-part channels), y = part NOCS (3K) of the points whose mask row has its first maximum at j
//   (every point is part 0 when mask is NULL):  scale_j = std(mean(y, axis=1)) / std(mean(x, axis=1)),
//   translation_j = mean(y - scale_j * x, axis=0).  Reductions in float64 through red (4 doubles of LDS); std in two passes, so that a part
//   whose row means are all the same float32 value has a std of exactly 0 (scale inf or NaN, as numpy's).  A NaN in a mask row is the
//   point's label (np.argmax: the first NaN).
// Thread 0 stores scale, translation (NaN for an empty part) to the four doubles at OUT (an expression, evaluated by thread 0 only).
#define ANCSH_PART_SIMILARITY(n, K, G, j, p0, gocs, nocs, mask, red, OUT)                                                              \
    double sx = 0, sxx = 0, sy = 0, syy = 0, m = 0;                                                                               \
    for (int i = threadIdx.x; i < n; i += 256) {                                                                                  \
        const int c = mask ? argmax_first_nan(mask + (p0 + i) * K, K) : 0;                                                        \
        if (c != j) continue;                                                                                                     \
        const float *x = gocs + (p0 + i) * G + (G == 3 ? 0 : 3 * j), *y = nocs + (p0 + i) * 3 * K + 3 * j;                       \
        const float xm = ((x[0] + x[1]) + x[2]) / 3.0f, ym = ((y[0] + y[1]) + y[2]) / 3.0f;    /* np.mean(., axis=1), float32 */ \
        sx += xm; sy += ym; m += 1.0;                                                                                             \
    }                                                                                                                             \
    sx = block_sum_f64(sx, red); sy = block_sum_f64(sy, red); m = block_sum_f64(m, red);                                          \
    /* two passes like np.std: the deviations from the mean, not sxx / m - (sx / m)^2, whose cancellation leaves a part of bit-equal */ \
    /* row means a variance of some 1e-17 instead of 0 (m equal float32 values sum exactly in float64, and (m v) / m == v) */     \
    const double mx = sx / m, my = sy / m;                                                                                        \
    for (int i = threadIdx.x; i < n; i += 256) {                                                                                  \
        const int c = mask ? argmax_first_nan(mask + (p0 + i) * K, K) : 0;                                                        \
        if (c != j) continue;                                                                                                     \
        const float *x = gocs + (p0 + i) * G + (G == 3 ? 0 : 3 * j), *y = nocs + (p0 + i) * 3 * K + 3 * j;                       \
        const float xm = ((x[0] + x[1]) + x[2]) / 3.0f, ym = ((y[0] + y[1]) + y[2]) / 3.0f;                                       \
        const double dx = (double)xm - mx, dy = (double)ym - my;                                                                  \
        sxx += dx * dx; syy += dy * dy;                                                                                           \
    }                                                                                                                             \
    sxx = block_sum_f64(sxx, red); syy = block_sum_f64(syy, red);                                                                 \
    const float scale = (float)sqrt(syy / m) / (float)sqrt(sxx / m);                        /* float32 / float32 (np.std) */      \
    double t[3] = {0, 0, 0};                                                                                                      \
    for (int i = threadIdx.x; i < n; i += 256) {                                                                                  \
        const int c = mask ? argmax_first_nan(mask + (p0 + i) * K, K) : 0;                                                        \
        if (c != j) continue;                                                                                                     \
        const float *x = gocs + (p0 + i) * G + (G == 3 ? 0 : 3 * j), *y = nocs + (p0 + i) * 3 * K + 3 * j;                       \
        _Pragma("unroll") for (int c3 = 0; c3 < 3; ++c3) t[c3] += (double)(y[c3] - scale * x[c3]);                               \
    }                                                                                                                             \
    for (int c3 = 0; c3 < 3; ++c3) t[c3] = block_sum_f64(t[c3], red);                                                             \
    if (threadIdx.x == 0) {                                                                                                       \
        double *o = (OUT);                                                                                                        \
        o[0] = m > 0 ? (double)scale : NAN;                                                                                       \
        for (int c3 = 0; c3 < 3; ++c3) o[1 + c3] = m > 0 ? t[c3] / m : NAN;                                                       \
    }

// ---- the votes of joint j (eval_joint_params.py:176-184): ordered compaction, in point order, into six LDS columns of npow2 floats
//   columns 0..2 = joint_axis_per_point, 3..5 = nocs_g + unitvec * (1 - heatmap) * 0.2 (float32, numpy's order; nocs_g = the point's
//   predicted part's triple when G = 3K).  IS_J: a boolean expression of the point's global index (p0 + i), true for a vote of joint j.
//   cnt (an int the caller set to 0) ends as the number of votes, the same on every thread.  wcnt: 4 ints of LDS.
#define ANCSH_COMPACT_JOINT_VOTES(n, K, G, p0, npow2, gocs, mask, heatmap, unitvec, axis, IS_J, jp_vals, wcnt, lane, wave, cnt)        \
    for (int c0 = 0; c0 < n; c0 += 256) {                                                                                             \
        const int i = c0 + threadIdx.x;                                                                                               \
        const bool f = i < n && (IS_J);                                                                                               \
        const unsigned long long mm = __ballot(f);                                                                                    \
        __syncthreads();                                                                                                              \
        if (lane == 0) wcnt[wave] = __popcll(mm);                                                                                     \
        __syncthreads();                                                                                                              \
        int start = cnt;                                                                                                              \
        for (int w = 0; w < wave; ++w) start += wcnt[w];                                                                              \
        if (f) {                                                                                                                      \
            const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(mm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mm, 0));     \
            const int c = (mask && G != 3) ? argmax_first_nan(mask + (p0 + i) * K, K) : 0;                                            \
            const float *g = gocs + (p0 + i) * G + (G == 3 ? 0 : 3 * c);                                                              \
            const float w1 = 1.0f - heatmap[p0 + i];                                                                                  \
            _Pragma("unroll") for (int c3 = 0; c3 < 3; ++c3) {                                                                        \
                jp_vals[c3 * npow2 + pos] = axis[(p0 + i) * 3 + c3];                                                                  \
                const float off = (unitvec[(p0 + i) * 3 + c3] * w1) * 0.2f;      /* unitvec * (1 - heatmap) * thres_r, float32 */     \
                jp_vals[(3 + c3) * npow2 + pos] = g[c3] + off;                                                                        \
            }                                                                                                                         \
        }                                                                                                                             \
        cnt += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];                                                                                 \
    }

// pads the six columns' [cnt, p2 = next power of two) with +inf and bitonic-sorts each column in place, in numpy's order (vote_above: NaN
// above +inf -- with a plain `a > b` a NaN answers "no" both ways and the network no longer sorts the column); ends on a barrier.  A column
// with a NaN vote ends with a NaN in slot p2 - 1, which is how ANCSH_VOTE_MEDIAN finds it.  Declares p2.
#define ANCSH_SORT_VOTE_COLUMNS(jp_vals, npow2, cnt)                                                                                  \
    int p2 = 1;                                                                                                                   \
    while (p2 < cnt) p2 <<= 1;                                                                                                    \
    for (int e = cnt + threadIdx.x; e < p2; e += 256)                                                                             \
        _Pragma("unroll") for (int c = 0; c < 6; ++c) jp_vals[c * npow2 + e] = INFINITY;                                          \
    __syncthreads();                                                                                                              \
    for (int k = 2; k <= p2; k <<= 1)                                                                                             \
        for (int s = k >> 1; s > 0; s >>= 1) {                                                                                    \
            for (int e = threadIdx.x; e < p2; e += 256) {                                                                         \
                const int partner = e ^ s;                                                                                        \
                if (partner > e) {                                                                                                \
                    const bool up = (e & k) == 0;                                                                                 \
                    _Pragma("unroll") for (int c = 0; c < 6; ++c) {                                                               \
                        float *v = jp_vals + c * npow2;                                                                           \
                        const float a = v[e], bb = v[partner];                                                                    \
                        if (vote_above(a, bb) == up) { v[e] = bb; v[partner] = a; }                                               \
                    }                                                                                                             \
                }                                                                                                                 \
            }                                                                                                                     \
            __syncthreads();                                                                                                      \
        }

// the same network on columns C0..5 only (C0 a literal): for a caller that takes no median of the columns below C0 (the ground-truth joint
// axis is a mean, point_gt.hip).  A column's order never depends on another column, so columns C0..5 end as the macro above leaves them.
#define ANCSH_SORT_VOTE_COLUMNS_FROM(jp_vals, npow2, cnt, C0)                                                                         \
    int p2 = 1;                                                                                                                   \
    while (p2 < cnt) p2 <<= 1;                                                                                                    \
    for (int e = cnt + threadIdx.x; e < p2; e += 256)                                                                             \
        _Pragma("unroll") for (int c = (C0); c < 6; ++c) jp_vals[c * npow2 + e] = INFINITY;                                       \
    __syncthreads();                                                                                                              \
    for (int k = 2; k <= p2; k <<= 1)                                                                                             \
        for (int s = k >> 1; s > 0; s >>= 1) {                                                                                    \
            for (int e = threadIdx.x; e < p2; e += 256) {                                                                         \
                const int partner = e ^ s;                                                                                        \
                if (partner > e) {                                                                                                \
                    const bool up = (e & k) == 0;                                                                                 \
                    _Pragma("unroll") for (int c = (C0); c < 6; ++c) {                                                            \
                        float *v = jp_vals + c * npow2;                                                                           \
                        const float a = v[e], bb = v[partner];                                                                    \
                        if (vote_above(a, bb) == up) { v[e] = bb; v[partner] = a; }                                               \
                    }                                                                                                             \
                }                                                                                                                 \
            }                                                                                                                     \
            __syncthreads();                                                                                                      \
        }

// med = np.median of sorted column c: the middle element, or the float32 mean of the middle two; NaN without votes, and NaN when any vote of
// the column is a NaN (the sort left it in the last of the p2 padded slots)
#define ANCSH_VOTE_MEDIAN(med, jp_vals, npow2, cnt, p2, c)                                                                            \
    const float *med##_v = jp_vals + (c) * npow2;                                                                                     \
    float med = NAN;                                                                                                                  \
    if (cnt > 0 && med##_v[p2 - 1] == med##_v[p2 - 1])                                                                                \
        med = (cnt & 1) ? med##_v[cnt / 2] : (med##_v[cnt / 2 - 1] + med##_v[cnt / 2]) * 0.5f;

// ---- part 0's pose as the boundary pass reads it (eval_pose_err.py:253-268): R = 9 doubles row-major, t = 3 doubles, rounded to float32
// like compose_rt (:25-30); declares r00 r10 r20 = the first column of R, t0 t1 t2 = the rounded translation and m30 = the inverse's
// translation entry, float32 like the pinv's
#define ANCSH_POSE0_FIRST_COLUMN(R, t, r00, r10, r20, t0, t1, t2, m30)                                                                \
    const double r00 = (double)(float)(R)[0], r10 = (double)(float)(R)[3], r20 = (double)(float)(R)[6];                               \
    const double t0 = (double)(float)(t)[0], t1 = (double)(float)(t)[1], t2 = (double)(float)(t)[2];                                  \
    const double m30 = (double)(float)(-(t0 * r00 + t1 * r10 + t2 * r20));

// ---- one pass over a cloud: every part's amodal-box extent max |nocs_j - 0.5| per channel (compute_miou.py:196-200), its point count
// and, when DYNAM (a literal true / false), its boundary: the min over the part's points of the x coordinate taken back through part 0's
// pose (:202-203; r00 r10 r20 m30 = the inverse's first column).  Part j = the points whose mask row has its first maximum at j; nocs:
// C = 3 or 3K channels.  Each wave's partials land in smax[wave][j][3] / smin[wave][j] / scnt[wave][j] (LDS, KM = 8 parts) for j < K;
// the caller combines the four waves after a barrier.
#define ANCSH_PART_EXTENTS_PASS(DYNAM, n, K, C, p0, nocs, mask, P, ldp, r00, r10, r20, m30, smax, smin, scnt, lane, wave)            \
    {                                                                                                                                 \
        /* one pass over the cloud: every part's running extents in registers (the part index only selects, it never addresses) */   \
        float m[KM][3];                                                                                                               \
        double mn[KM];                                                                                                                \
        int cnt[KM];                                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < KM; ++j) { m[j][0] = m[j][1] = m[j][2] = -INFINITY; mn[j] = INFINITY; cnt[j] = 0; }    \
        for (int i = threadIdx.x; i < n; i += 256) {                                                                                  \
            const int c = argmax_first_nan(mask + (p0 + i) * K, K);                                                                  \
            const float *q = nocs + (p0 + i) * C + (C == 3 ? 0 : 3 * c);                                                              \
            const float a0 = fabsf(q[0] - 0.5f), a1 = fabsf(q[1] - 0.5f), a2 = fabsf(q[2] - 0.5f);                                    \
            double v = 0.0;                                                                                                           \
            if (DYNAM) {                                                                                                              \
                const float *x = P + (p0 + i) * ldp;                                                                                  \
                /* numpy: [x y z 1] . M[:, 0] accumulated left to right in float64 */                                                 \
                v = (((double)x[0] * r00 + (double)x[1] * r10) + (double)x[2] * r20) + m30;                                           \
            }                                                                                                                         \
            _Pragma("unroll") for (int j = 0; j < KM; ++j) {                                                                          \
                const bool mine = c == j;                                                                                             \
                m[j][0] = mine ? np_maxf(m[j][0], a0) : m[j][0];                                                                      \
                m[j][1] = mine ? np_maxf(m[j][1], a1) : m[j][1];                                                                      \
                m[j][2] = mine ? np_maxf(m[j][2], a2) : m[j][2];                                                                      \
                if (DYNAM) mn[j] = mine ? np_min(mn[j], v) : mn[j];                                                                   \
                cnt[j] += mine ? 1 : 0;                                                                                               \
            }                                                                                                                         \
        }                                                                                                                             \
        _Pragma("unroll") for (int j = 0; j < KM; ++j) {                                                                              \
            if (j >= K) break;                                  /* K is uniform: the unused parts cost nothing past this point */     \
            _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) {                                                                      \
                m[j][0] = np_maxf(m[j][0], __shfl_xor(m[j][0], o, 64)); m[j][1] = np_maxf(m[j][1], __shfl_xor(m[j][1], o, 64));       \
                m[j][2] = np_maxf(m[j][2], __shfl_xor(m[j][2], o, 64));                                                               \
                if (DYNAM) mn[j] = np_min(mn[j], __shfl_xor(mn[j], o, 64));                                                           \
                cnt[j] += __shfl_xor(cnt[j], o, 64);                                                                                  \
            }                                                                                                                         \
            if (lane == 0) {                                                                                                          \
                smax[wave][j][0] = m[j][0]; smax[wave][j][1] = m[j][1]; smax[wave][j][2] = m[j][2];                                   \
                if (DYNAM) smin[wave][j] = mn[j];                                                                                     \
                scnt[wave][j] = cnt[j];                                                                                               \
            }                                                                                                                         \
        }                                                                                                                             \
    }
