// gt_pose.hip -- the ground-truth poses of a streamed batch, step 1 of evaluation.sh (evaluation/compute_gt_pose.py:80-89, run once with
// --nocs ANCSH and once with --nocs NAOCS): per part, estimateSimilarityUmeyama between the sampled points' ground-truth part NOCS /
// NAOCS and the sampled points themselves, in ONE launch directly behind the sampler.  It writes the (b, K, 19) table ancsh_gt_error_rec
// reads and the (b, 13) table ancsh_point_gt_rec reads.
//
// One workgroup of 256 threads per (part j, cloud c).  Nothing is gathered into tensors: sampled point i of cloud c is raw row
// offsets[c] + perm[c][i] % n_raw of the slot's 18-channel rows (ancsh_point_gt_rec's rules), its target is P[c][i].  Pass 1 walks the
// n samples in chunks of 256, counts the points of ALL K parts (the empty-part rule needs them) and compacts part j's (sample index,
// raw row) pairs, in sample order, into two LDS lists: per-wave ballots and popcounts, ANCSH_JD_COMPACT's scheme.  Pass 2 is
// umeyama_kernel's arithmetic (umeyama_fit.h) over that list, once for nocs_p and once for nocs_g: thread t takes compacted rows t,
// t + 256, ..., block_sum<6> then block_sum<10>, horn_quat / quat_to_mat and umeyama_kernel's whole output row on lane 0, into LDS -- the
// bits ancsh_umeyama writes for the rows gathered into a contiguous problem; the tables' columns are then picked from that row.  No
// atomics, nothing allocated, every size an argument or read from device memory, no workgroup waits for another and each writes its own
// row only: capturable, and the same bytes every run wherever the cloud lies in the batch.
#include "umeyama_fit.h"

namespace ancsh {
namespace pose {

constexpr int GP_KM = 8;
constexpr int GP_NCHAN = 18;                       // x y z | cls | nocs_p 3 | nocs_g 3 | heatmap | unitvec 3 | orient 3 | joint_cls
constexpr int GP_MAX_N = ANCSH_ARTICULATION_MAX_N;
constexpr int GP_GT = 19, GP_FRAME = 13;

struct GtPoseArgs {
    const float *rows;
    const int *offsets, *perm;
    const float *P;
    const double *extent;
    double *gt, *frame;
    long capacity;
    int n, K, ldp, ld_extent;
};

// Entry e of [R (9, row-major src -> tgt) | s | t (3)] of one fit, from umeyama_kernel's 32 output doubles o (Scales 0..2, the TRANSPOSED
// rotation 3..11, Translation 12..14), as the tables hold it: every R and t entry rounded to float32 once and widened (compose_rt's
// float32 matrix), the scale as computed; NaN when one of the 13 is not finite
__device__ __forceinline__ double gp_entry(const double *o, int e) {
    bool finite = isfinite(o[0]);
#pragma unroll
    for (int k = 3; k < 15; ++k) finite = finite && isfinite((double)(float)o[k]);
    const double v = e < 9 ? (double)(float)o[3 + (e % 3) * 3 + e / 3] : e == 9 ? o[0] : (double)(float)o[12 + (e - 10)];
    return finite ? v : NAN;
}

#define GP_NOCS_P(i, c) rows[(size_t)s_row[i] * GP_NCHAN + 4 + (c)]
#define GP_NOCS_G(i, c) rows[(size_t)s_row[i] * GP_NCHAN + 7 + (c)]
#define GP_POINT(i, c) ar.P[(p0 + s_samp[i]) * ar.ldp + (c)]

__global__ __launch_bounds__(256) void gt_pose_kernel(GtPoseArgs ar) {
    __shared__ int s_samp[GP_MAX_N], s_row[GP_MAX_N];      // part j's sampled points in sample order: the sample index, the raw row
    __shared__ double red[64];
    __shared__ double sol[2][32];                           // umeyama_kernel's output row of each fit
    __shared__ int wcnt[4];
    __shared__ int redk[4][GP_KM];
    const int j = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = ar.n, K = ar.K;
    const size_t p0 = (size_t)c * n;
    double *g = ar.gt ? ar.gt + ((size_t)c * K + j) * GP_GT : nullptr;
    double *fr = ar.frame && j == 0 ? ar.frame + (size_t)c * GP_FRAME : nullptr;
    if (!g && !fr) return;                              // gt == NULL: only part 0's workgroup has a row to write
    const long r0 = ar.offsets[c], r1 = ar.offsets[c + 1];
    if (r0 < 0 || r1 <= r0 || r1 > ar.capacity) {          // empty or outside the rows buffer (the host refuses both): NaN throughout
        if (g && tid < GP_GT) g[tid] = NAN;
        if (fr && tid < GP_FRAME) fr[tid] = NAN;
        return;
    }
    // columns 13..15: the extent row, moved as 64-bit words so that a NaN keeps its payload
    if (g && tid < 3) {
        if (ar.extent)
            reinterpret_cast<unsigned long long *>(g)[13 + tid] =
                reinterpret_cast<const unsigned long long *>(ar.extent + ((size_t)c * K + j) * ar.ld_extent)[tid];
        else
            g[13 + tid] = NAN;
    }
    const int n_raw = (int)(r1 - r0);
    const float *rows = ar.rows + (size_t)r0 * GP_NCHAN;
    // ---- pass 1: the points of every part, and part j's in sample order
    int pc[GP_KM];
#pragma unroll
    for (int k = 0; k < GP_KM; ++k) pc[k] = 0;
    int cnt = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        int r = 0, lab = -1;
        if (i < n) {
            r = ar.perm[p0 + i] % n_raw;
            if (r < 0) r += n_raw;                        // a sampler's index is never negative; nothing is read outside the cloud either way
            lab = (int)rows[(size_t)r * GP_NCHAN + 3];    // cls_gt: C truncation, as np.asarray(x, np.int32)
        }
#pragma unroll
        for (int k = 0; k < GP_KM; ++k) pc[k] += lab == k ? 1 : 0;
        const bool f = i < n && lab == j;
        const unsigned long long m = __ballot(f);
        __syncthreads();
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int start = cnt;
        for (int w = 0; w < wave; ++w) start += wcnt[w];
        if (f) {
            const int pos = start + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
            s_samp[pos] = i;                              // pos < n <= GP_MAX_N
            s_row[pos] = r;
        }
        cnt += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    }
#pragma unroll
    for (int k = 0; k < GP_KM; ++k) {
        int s = pc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) redk[wave][k] = s;
    }
    __syncthreads();                                    // redk and the two lists are visible
    bool empty = false;
    for (int k = 0; k < K; ++k) empty |= redk[0][k] + redk[1][k] + redk[2][k] + redk[3][k] == 0;
    if (empty) {                                        // a part without a sampled point: the reference skips the record, the cloud is missing
        if (g && tid < GP_GT && (tid < 13 || tid >= 16)) g[tid] = NAN;
        if (fr && tid < GP_FRAME) fr[tid] = NAN;
        return;
    }
    // ---- pass 2: the two fits over the list (cnt >= 1 here): umeyama_kernel's statements, its 32 outputs into LDS
    if (g) {                                            // U_p = estimateSimilarityUmeyama(nocs_p, P)
        ANCSH_UMEYAMA_SUMS(cnt, GP_NOCS_P, GP_POINT, red)
        if (tid == 0) {
            double *o = sol[0];
            ANCSH_UMEYAMA_SOLVE(cnt, o)
        }
    }
    {                                                   // U_g = estimateSimilarityUmeyama(nocs_g, P)
        ANCSH_UMEYAMA_SUMS(cnt, GP_NOCS_G, GP_POINT, red)
        if (tid == 0) {
            double *o = sol[1];
            ANCSH_UMEYAMA_SOLVE(cnt, o)
        }
    }
    __syncthreads();                                    // both solutions are visible
    // ---- the row: thread e < 13 column e of U_p, thread 16..18 U_g's translation; part 0's frame: thread 32 + e column e of U_g
    if (g && tid < 13) g[tid] = gp_entry(sol[0], tid);
    if (g && tid >= 16 && tid < GP_GT) g[tid] = gp_entry(sol[1], tid - 6);
    if (fr && tid >= 32 && tid < 32 + GP_FRAME) fr[tid - 32] = gp_entry(sol[1], tid - 32);
}

}  // namespace pose
}  // namespace ancsh

extern "C" int ancsh_gt_pose_build(int b, int n, int K, int nchan, const float *rows, long capacity, const int *offsets, const int *perm,
                                   const float *P, int ldp, const double *extent, int ld_extent, double *gt, double *frame, void *stream) {
    using namespace ancsh;
    using namespace ancsh::pose;
    ANCSH_REQUIRE(b >= 0 && b <= 65535, "gt_pose_build: b=%d (0..65535)", b);
    ANCSH_REQUIRE(K >= 1 && K <= GP_KM, "gt_pose_build: K=%d (1..8)", K);
    ANCSH_REQUIRE(nchan == GP_NCHAN, "gt_pose_build: nchan=%d (18: x y z | cls | nocs_p 3 | nocs_g 3 | heatmap | unitvec 3 | orient 3 | joint_cls)",
                  nchan);
    ANCSH_REQUIRE(n >= 1 && n <= GP_MAX_N, "gt_pose_build: n=%d (1..%d: a part's sample list stays in LDS)", n, GP_MAX_N);
    ANCSH_REQUIRE(ldp >= 3, "gt_pose_build: ldp=%d (>= 3)", ldp);
    ANCSH_REQUIRE(!extent || ld_extent >= 3, "gt_pose_build: ld_extent=%d (>= 3)", ld_extent);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "gt_pose_build: capacity=%ld rows out of range", capacity);
    if (b == 0) return ANCSH_OK;
    ANCSH_REQUIRE(rows && offsets && perm && P, "gt_pose_build: null pointer");
    ANCSH_REQUIRE(gt || frame, "gt_pose_build: gt and frame are both NULL (nothing to build)");
    GtPoseArgs ar;
    ar.rows = rows; ar.offsets = offsets; ar.perm = perm; ar.P = P; ar.extent = extent; ar.gt = gt; ar.frame = frame;
    ar.capacity = capacity;
    ar.n = n; ar.K = K; ar.ldp = ldp; ar.ld_extent = ld_extent;
    hipLaunchKernelGGL(gt_pose_kernel, dim3(K, b), dim3(256), 0, (hipStream_t)stream, ar);
    return check_launch("gt_pose_build");
}
