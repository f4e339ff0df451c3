// depth_annotate.hip -- rendered depth frames annotated on the GPU (gfx950): depth crops + link-label crops + one scene table per frame ->
// the 7-column annotated rows [x y z | cx cy cz | part] that ancsh_point_gt_build reads.
//
// Reference: tools/preprocess_data.py:259-320 -- per link s the pixels with label == s (np.where, row-major, :262-263), their camera points
// cloud_cam_real (:293-296, gt_points) and, from a second camera point with the image row flipped (:288-291), the chain camera -> world ->
// link -> URDF frame (:298-320, gt_coords) -- and lib/dataset.py:475-485, which concatenates the links group by group of parts_map.  The
// host folds the chain into one 3 x 4 map per link (depth.pack_frame_scene); here a ragged batch of crops is TWO launches on depth.hip's
// grid and chunking, every size read from device memory (include/ancsh_hip.h, ancsh_depth_annotate_stream):
//   count   : block (x, b) writes the per-link histogram of the valid pixels of chunk x of cloud b's crop -> scratch[(b * chunks + x) * 16 ..];
//   scatter : block (x, b) derives the per-link totals of the clouds <= b from the histograms (a cloud with a used link below the minimum
//             has no rows), the start of (link, chunk) from them -- cloud_base + the totals of the links of smaller rank + the link's counts
//             in earlier chunks --, ranks every pixel among its own link with per-link wave ballots in lane (= pixel) order, and writes
//             its rows.  A stable counting sort by link: the rows of a part are neighbours, as ancsh_point_gt_build expects.  No atomics,
//             no workgroup waits for another: the output is a pure function of the input.
// float64 arithmetic evaluated as written (the library is built with -ffp-contract=off), one rounding to float32 per output.
#include "depth_annotate_common.h"

namespace ancsh {

template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void annotate_count_kernel(const T *__restrict__ depth, const unsigned char *__restrict__ labels,
                                                                       long pixel_capacity, const int *__restrict__ geom,
                                                                       const double *__restrict__ scene, int chunks, int *__restrict__ scratch) {
    constexpr int V = 16 / sizeof(T);
    __shared__ int s_rank[AN_LINKS];
    __shared__ int s_hist[AN_LINKS][DEPTH_THREADS];                     // a column per thread: no two threads share a counter
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *sc = scene + (size_t)b * AN_SCENE;
    if (tid < AN_LINKS) s_rank[tid] = scene_rank(sc, tid, scene_nlinks(sc));
#pragma unroll
    for (int l = 0; l < AN_LINKS; ++l) s_hist[l][tid] = 0;
    __syncthreads();
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, b, pixel_capacity, start, w);
    depth_chunk(start, n, x, chunks, lo, hi);
    if (hi > lo) {
        const long g0 = lo / V, ng = (hi - 1) / V - g0 + 1;
        for (long g = tid; g < ng; g += DEPTH_THREADS) {
            T d[V];
            int lab[V];
            annotate_group<T>(depth, labels, (g0 + g) * V, lo, hi, pixel_capacity, s_rank, d, lab);
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (lab[k] >= 0) ++s_hist[lab[k]][tid];
        }
    }
    __syncthreads();
    for (int l = wave; l < AN_LINKS; l += DEPTH_WAVES) {               // a wave sums a link's 256 columns
        int v = 0;
#pragma unroll
        for (int k = 0; k < DEPTH_WAVES; ++k) v += s_hist[l][lane + 64 * k];
#pragma unroll
        for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) scratch[((size_t)b * chunks + x) * AN_LINKS + l] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void annotate_scatter_kernel(int nclouds, const T *__restrict__ depth,
                                                                         const unsigned char *__restrict__ labels, long pixel_capacity,
                                                                         const int *__restrict__ geom, const double *__restrict__ scene,
                                                                         int chunks, const int *__restrict__ scratch, float *__restrict__ rows,
                                                                         long capacity, int *__restrict__ offsets, int *__restrict__ counts,
                                                                         int *__restrict__ link_counts) {
    constexpr int V = 16 / sizeof(T);
    __shared__ long s_red[DEPTH_WAVES];
    __shared__ double s_scene[AN_SCENE];
    __shared__ int s_rank[AN_LINKS], s_tot[AN_LINKS], s_head[AN_LINKS];
    __shared__ long s_total;
    __shared__ long s_base[2][AN_LINKS];                                // the next row of every link, double-buffered like s_cnt
    __shared__ int s_cnt[2][DEPTH_WAVES][AN_LINKS];
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *sc = scene + (size_t)b * AN_SCENE;
    if (tid < AN_SCENE) s_scene[tid] = sc[tid];
    if (tid < AN_LINKS) s_rank[tid] = scene_rank(sc, tid, scene_nlinks(sc));
    // rows in front of this cloud: max(rows, 1) of every earlier cloud (an empty cloud owns one NaN row); of this cloud: the per-link
    // totals and the counts of the chunks in front of this one
    long before = 0;
    for (int c = tid; c <= b; c += DEPTH_THREADS) {
        const int *h = scratch + (size_t)c * chunks * AN_LINKS;
        int tot[AN_LINKS], head[AN_LINKS];
#pragma unroll
        for (int l = 0; l < AN_LINKS; ++l) tot[l] = head[l] = 0;
        for (int k = 0; k < chunks; ++k) {
            if (c == b && k == x) {
#pragma unroll
                for (int l = 0; l < AN_LINKS; ++l) head[l] = tot[l];
            }
#pragma unroll
            for (int l = 0; l < AN_LINKS; ++l) tot[l] += h[k * AN_LINKS + l];
        }
        const long t = scene_cloud_rows(scene + (size_t)c * AN_SCENE, tot);
        if (c < b) before += t > 1 ? t : 1;
        else {
            s_total = t;
#pragma unroll
            for (int l = 0; l < AN_LINKS; ++l) s_tot[l] = tot[l], s_head[l] = head[l];
        }
    }
    const long cloud_base = depth_block_sum(before, s_red);             // its barriers publish s_scene, s_rank, s_tot, s_head, s_total
    const long total = s_total;
    if (tid < AN_LINKS) {
        // the link's first row in this chunk: behind the links of smaller rank and behind its own pixels of the earlier chunks
        const int rk = s_rank[tid];
        long rel = s_head[tid];
        for (int l = 0; l < AN_LINKS; ++l)
            if (s_rank[l] >= 0 && s_rank[l] < rk) rel += s_tot[l];
        s_base[0][tid] = cloud_base + rel;                              // read behind the first barrier of the loop below
        if (x == 0) link_counts[(size_t)b * AN_LINKS + tid] = s_tot[tid];
    }
    if (x == 0 && tid == 0) {
        const long end = cloud_base + (total > 1 ? total : 1);
        offsets[b] = (int)(cloud_base < 0x7fffffffL ? cloud_base : 0x7fffffffL);
        counts[b] = (int)total;
        if (b == nclouds - 1) offsets[nclouds] = (int)(end < 0x7fffffffL ? end : 0x7fffffffL);
        if (total == 0 && cloud_base < capacity) {
            const float q = __builtin_nanf("");
#pragma unroll
            for (int a = 0; a < 7; ++a) rows[cloud_base * 7 + a] = q;
        }
    }
    if (total == 0) return;                                             // uniform: no valid pixel, or a used link below the minimum
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, b, pixel_capacity, start, w);
    depth_chunk(start, n, x, chunks, lo, hi);
    if (hi <= lo) return;                                               // uniform
    const int row0 = geom[(size_t)b * DEPTH_GEOM + 3], col0 = geom[(size_t)b * DEPTH_GEOM + 4];
    const double *S = s_scene;
    const unsigned long long below_me = (1ull << lane) - 1ull;
    const long g0 = lo / V, ng = (hi - 1) / V - g0 + 1;
    int buf = 0;
    for (long gb = 0; gb < ng; gb += DEPTH_THREADS, buf ^= 1) {         // uniform trip count: every wave reaches the barrier
        const long g = gb + tid;
        T d[V];
        int lab[V], rk[V];
        if (g < ng) annotate_group<T>(depth, labels, (g0 + g) * V, lo, hi, pixel_capacity, s_rank, d, lab);
        unsigned present = 0;                                           // the links of this wave's pixels
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (g >= ng) lab[k] = -1, d[k] = T(0);
            rk[k] = 0;
            if (lab[k] >= 0) present |= 1u << lab[k];
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) present |= __shfl_xor(present, o);
        int mine = 0;                                                   // lane l: the wave's pixels of link l
        while (present) {                                               // uniform over the wave: at most nlinks iterations
            const int l = __ffs(present) - 1;
            present &= present - 1;
            int below = 0, all = 0;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const unsigned long long bal = __ballot(lab[k] == l);
                below += __popcll(bal & below_me);
                all += __popcll(bal);
            }
            int own = 0;
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (lab[k] == l) rk[k] = below + own++;                 // the pixels of earlier lanes, then the lane's own earlier pixels
            if (lane == l) mine = all;
        }
        if (lane < AN_LINKS) s_cnt[buf][wave][lane] = mine;
        __syncthreads();                                                // s_cnt and s_base are double-buffered: one barrier per step
        if (tid < AN_LINKS) {
            long next = s_base[buf][tid];
#pragma unroll
            for (int k = 0; k < DEPTH_WAVES; ++k) next += s_cnt[buf][k][tid];
            s_base[buf ^ 1][tid] = next;
        }
        const long p0 = (g0 + g) * V - start;                           // crop position of the group's first pixel; < 0 only in front of lo
        int i = p0 >= 0 ? (int)(p0 / w) : 0, j = (int)(p0 - (long)i * w);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int l = lab[k];
            if (l >= 0) {
                long r = s_base[buf][l] + rk[k];
#pragma unroll
                for (int q = 0; q < DEPTH_WAVES; ++q)
                    if (q < wave) r += s_cnt[buf][q][l];
                if (r < capacity) {
                    const double row = (double)(row0 + i), col = (double)(col0 + j);
                    const double z = (double)d[k] * S[6];
                    const double px = z * ((S[0] * col + S[1] * row) + S[2]), py = z * ((S[3] * col + S[4] * row) + S[5]);
                    const double qx = z * ((S[7] * col + S[8] * row) + S[9]), qy = z * ((S[10] * col + S[11] * row) + S[12]);
                    const double *L = S + AN_HEAD + AN_LINK * l, *M = L + 2;
                    float *o = rows + r * 7;
                    o[0] = (float)px, o[1] = (float)py, o[2] = (float)z;
#pragma unroll
                    for (int a = 0; a < 3; ++a) o[3 + a] = (float)(((M[4 * a] * qx + M[4 * a + 1] * qy) + M[4 * a + 2] * z) + M[4 * a + 3]);
                    o[6] = (float)L[1];
                }
            }
            if (++j == w) j = 0, ++i;
        }
    }
}

template <typename T>
static void annotate_launch(int nclouds, const void *depth, const unsigned char *labels, long pixel_capacity, const int *geom,
                            const double *scene, float *rows, long capacity, int *offsets, int *counts, int *link_counts, int *scratch,
                            hipStream_t st) {
    const long chunks = depth_chunks(pixel_capacity, nclouds);          // depth.hip's grid
    const dim3 grid((unsigned)chunks, nclouds);
    hipLaunchKernelGGL(annotate_count_kernel<T>, grid, dim3(DEPTH_THREADS), 0, st, (const T *)depth, labels, pixel_capacity, geom, scene,
                       (int)chunks, scratch);
    hipLaunchKernelGGL(annotate_scatter_kernel<T>, grid, dim3(DEPTH_THREADS), 0, st, nclouds, (const T *)depth, labels, pixel_capacity, geom,
                       scene, (int)chunks, scratch, rows, capacity, offsets, counts, link_counts);
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_depth_annotate_stream(int nclouds, int depth_type, const void *depth, const unsigned char *labels, long pixel_capacity,
                                           const int *geom, const double *scene, float *rows, long capacity, int *offsets, int *counts,
                                           int *link_counts, int *scratch, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0, "depth_annotate_stream: bad shape nclouds=%d", nclouds);
    ANCSH_REQUIRE(nclouds <= 65535, "depth_annotate_stream: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32,
                  "depth_annotate_stream: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 30), "depth_annotate_stream: pixel_capacity=%ld pixels out of range",
                  pixel_capacity);
    ANCSH_REQUIRE(capacity >= pixel_capacity && capacity < (1L << 30),
                  "depth_annotate_stream: capacity=%ld rows must be in [pixel_capacity=%ld, 2^30)", capacity, pixel_capacity);
    ANCSH_REQUIRE(depth && labels && geom && scene && rows && offsets && counts && link_counts && scratch,
                  "depth_annotate_stream: null pointer");
    ANCSH_REQUIRE(((size_t)depth & 15) == 0 && ((size_t)labels & 7) == 0 && ((size_t)scene & 7) == 0,
                  "depth_annotate_stream: depth must be 16-byte aligned, labels and scene 8-byte aligned (the crops inside them may start "
                  "anywhere)");
    if (nclouds == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        annotate_launch<unsigned short>(nclouds, depth, labels, pixel_capacity, geom, scene, rows, capacity, offsets, counts, link_counts,
                                        scratch, (hipStream_t)stream);
    else
        annotate_launch<float>(nclouds, depth, labels, pixel_capacity, geom, scene, rows, capacity, offsets, counts, link_counts, scratch,
                               (hipStream_t)stream);
    return check_launch("depth_annotate_stream");
}
