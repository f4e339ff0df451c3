// depth_annotated_images.hip -- the inverse of depth_annotate.hip's stable counting sort (gfx950): what lies per ROW of an annotated frame --
// the networks' label and values (ancsh_raw_point_labels) and the ground truth of the 18-column rows (ancsh_point_gt_build) -- back on the
// pixel grid of the crop it came from: per frame a predicted part image and NOCS map and the true ones (include/ancsh_hip.h,
// ancsh_depth_annotated_images).  ONE launch on depth.hip's grid and chunking, every size read from device memory.
//
// Block (x, b) owns chunk x of cloud b's crop, as in the annotation's two passes.  From the histograms the count pass left in scratch it
// derives, for its own cloud only (offsets[b] is given: no loop over the earlier clouds), the first row of every link in its chunk --
// offsets[b] + the totals of the links of smaller rank + the link's counts in the earlier chunks.  Per step of 256 groups it ranks every
// valid pixel among its own link with per-link wave ballots in lane (= pixel) order, exactly as annotate_scatter_kernel does, which gives
// the row the scatter pass wrote the pixel to; the rows of the step go to LDS (-1: not a valid pixel, a frame without rows, or a row cut
// at capacity), and the block stores the step's four images as contiguous spans.  Everything travels as its bits (NaN payloads survive).
// No atomics, no workgroup waits for another: the output is a pure function of the input.
#include "depth_annotate_common.h"

namespace ancsh {

constexpr int AI_VALUES = 7, AI_GT_VALUES = 6, AI_GT_LABEL = 3, AI_GT_FIRST = 4;    // per pixel; the columns of an 18-column row

template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void annotated_images_kernel(
    const T *__restrict__ depth, const unsigned char *__restrict__ link_labels, long pixel_capacity, const int *__restrict__ geom,
    const double *__restrict__ scene, int chunks, const int *__restrict__ scratch, const int *__restrict__ offsets,
    const int *__restrict__ counts, const unsigned *__restrict__ labels, const unsigned *__restrict__ values,
    const float *__restrict__ gt_rows, int gt_nchan, long capacity, const int *__restrict__ dest, unsigned *__restrict__ img_labels,
    unsigned *__restrict__ img_values, unsigned *__restrict__ img_gt_labels, unsigned *__restrict__ img_gt_values, long image_capacity) {
    constexpr int V = 16 / sizeof(T), STEP = DEPTH_THREADS * V;
    __shared__ int s_rank[AN_LINKS], s_tot[AN_LINKS], s_head[AN_LINKS];
    __shared__ long s_base[2][AN_LINKS];                                // the next row of every link, double-buffered like s_cnt
    __shared__ int s_cnt[2][DEPTH_WAVES][AN_LINKS];
    __shared__ int s_src[STEP];
    const int b = blockIdx.y, x = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, b, pixel_capacity, start, w);
    const long d0 = dest[b];
    if (n == 0 || d0 < 0 || n > image_capacity - d0) return;            // uniform: a silenced cloud, a refused crop, an image past the buffer
    depth_chunk(start, n, x, chunks, lo, hi);
    if (hi <= lo) return;                                               // uniform
    const double *sc = scene + (size_t)b * AN_SCENE;
    const bool has_rows = counts[b] > 0;                                // uniform: no valid pixel, or a used link below the minimum
    if (tid < AN_LINKS) {
        s_rank[tid] = scene_rank(sc, tid, scene_nlinks(sc));
        const int *h = scratch + (size_t)b * chunks * AN_LINKS + tid;   // this link's column of the cloud's histograms
        int tot = 0, head = 0;
        for (int k = 0; k < chunks; ++k) {
            if (k == x) head = tot;
            tot += h[k * AN_LINKS];
        }
        s_tot[tid] = tot, s_head[tid] = head;
    }
    __syncthreads();
    if (tid < AN_LINKS) {
        // the link's first row in this chunk: behind the links of smaller rank and behind its own pixels of the earlier chunks
        const int rk = s_rank[tid];
        long rel = s_head[tid];
        for (int l = 0; l < AN_LINKS; ++l)
            if (s_rank[l] >= 0 && s_rank[l] < rk) rel += s_tot[l];
        s_base[0][tid] = (long)offsets[b] + rel;                        // read behind the first barrier of the loop below
    }
    const unsigned long long below_me = (1ull << lane) - 1ull;
    const long g0 = lo / V, ng = (hi - 1) / V - g0 + 1;
    int buf = 0;
    for (long gb = 0; gb < ng; gb += DEPTH_THREADS, buf ^= 1) {         // uniform trip count: every wave reaches the barriers
        const long g = gb + tid;
        T d[V];
        int lab[V], rk[V];
        if (g < ng) annotate_group<T>(depth, link_labels, (g0 + g) * V, lo, hi, pixel_capacity, s_rank, d, lab);
        unsigned present = 0;                                           // the links of this wave's pixels
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (g >= ng || !has_rows) lab[k] = -1;
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
        __syncthreads();                                                // s_cnt and s_base are double-buffered; also: the previous step's
        if (tid < AN_LINKS) {                                           // readers of s_src are done
            long next = s_base[buf][tid];
#pragma unroll
            for (int k = 0; k < DEPTH_WAVES; ++k) next += s_cnt[buf][k][tid];
            s_base[buf ^ 1][tid] = next;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int l = lab[k];
            long r = -1;
            if (l >= 0) {
                r = s_base[buf][l] + rk[k];
#pragma unroll
                for (int q = 0; q < DEPTH_WAVES; ++q)
                    if (q < wave) r += s_cnt[buf][q][l];
            }
            s_src[tid * V + k] = r >= 0 && r < capacity ? (int)r : -1;
        }
        __syncthreads();                                                // s_src is published
        const long a0 = (g0 + gb) * V;                                  // the step's window of the pixel buffer, cut to the chunk
        const long pa = a0 > lo ? a0 : lo, pb = a0 + STEP < hi ? a0 + STEP : hi;
        const int *src = s_src + (pa - a0);
        const long q0 = d0 + (pa - start), np = pb - pa;
        const unsigned nan_bits = (unsigned)ANCSH_LABEL_NAN_BITS;
        depth_store_span(img_labels + q0, np, [&](long e) { const int s = src[e]; return s >= 0 ? labels[s] : 0xffffffffu; });
        depth_store_span(img_values + q0 * AI_VALUES, np * AI_VALUES, [&](long e) {
            const int p = (int)(e / AI_VALUES), s = src[p];
            return s >= 0 ? values[(size_t)s * AI_VALUES + (e - p * AI_VALUES)] : nan_bits;
        });
        depth_store_span(img_gt_labels + q0, np, [&](long e) {
            const int s = src[e];
            if (s < 0) return 0xffffffffu;
            const float v = gt_rows[(size_t)s * gt_nchan + AI_GT_LABEL];
            return (v - v) == 0.f ? (unsigned)(int)v : 0xffffffffu;     // finite: the part as an integer
        });
        depth_store_span(img_gt_values + q0 * AI_GT_VALUES, np * AI_GT_VALUES, [&](long e) {
            const int p = (int)(e / AI_GT_VALUES), s = src[p];
            return s >= 0 ? __float_as_uint(gt_rows[(size_t)s * gt_nchan + AI_GT_FIRST + (e - p * AI_GT_VALUES)]) : nan_bits;
        });
    }
}

template <typename T>
static void annotated_images_launch(int nclouds, const void *depth, const unsigned char *link_labels, long pixel_capacity, const int *geom,
                                    const double *scene, const int *offsets, const int *counts, const int *scratch, const int *labels,
                                    const float *values, const float *gt_rows, int gt_nchan, long capacity, const int *dest, int *img_labels,
                                    float *img_values, int *img_gt_labels, float *img_gt_values, long image_capacity, hipStream_t st) {
    const long chunks = depth_chunks(pixel_capacity, nclouds);          // the count pass's chunking: scratch[(b * chunks + x) * 16 ..] is its layout
    hipLaunchKernelGGL(annotated_images_kernel<T>, dim3((unsigned)chunks, nclouds), dim3(DEPTH_THREADS), 0, st, (const T *)depth, link_labels,
                       pixel_capacity, geom, scene, (int)chunks, scratch, offsets, counts, (const unsigned *)labels, (const unsigned *)values,
                       gt_rows, gt_nchan, capacity, dest, (unsigned *)img_labels, (unsigned *)img_values, (unsigned *)img_gt_labels,
                       (unsigned *)img_gt_values, image_capacity);
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_depth_annotated_images(int nclouds, int depth_type, const void *depth, const unsigned char *link_labels,
                                            long pixel_capacity, const int *geom, const double *scene, const int *offsets, const int *counts,
                                            const int *scratch, const int *labels, const float *values, const float *gt_rows, int gt_nchan,
                                            long capacity, const int *dest, int *img_labels, float *img_values, int *img_gt_labels,
                                            float *img_gt_values, long image_capacity, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0, "depth_annotated_images: bad shape nclouds=%d", nclouds);
    ANCSH_REQUIRE(nclouds <= 65535, "depth_annotated_images: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32,
                  "depth_annotated_images: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 30), "depth_annotated_images: pixel_capacity=%ld pixels out of range",
                  pixel_capacity);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "depth_annotated_images: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(gt_nchan >= 10, "depth_annotated_images: gt_nchan=%d must be >= 10 (the part in column 3, part NOCS and NAOCS in 4..9)",
                  gt_nchan);
    ANCSH_REQUIRE(image_capacity >= 0 && image_capacity < (1L << 30), "depth_annotated_images: image_capacity=%ld pixels out of range",
                  image_capacity);
    ANCSH_REQUIRE(depth && link_labels && geom && scene && offsets && counts && scratch && labels && values && gt_rows && dest &&
                      img_labels && img_values && img_gt_labels && img_gt_values,
                  "depth_annotated_images: null pointer");
    ANCSH_REQUIRE(((size_t)depth & 15) == 0 && ((size_t)link_labels & 7) == 0 && ((size_t)scene & 7) == 0,
                  "depth_annotated_images: depth must be 16-byte aligned, link_labels and scene 8-byte aligned (the crops inside them may "
                  "start anywhere)");
    if (nclouds == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        annotated_images_launch<unsigned short>(nclouds, depth, link_labels, pixel_capacity, geom, scene, offsets, counts, scratch, labels,
                                                values, gt_rows, gt_nchan, capacity, dest, img_labels, img_values, img_gt_labels,
                                                img_gt_values, image_capacity, (hipStream_t)stream);
    else
        annotated_images_launch<float>(nclouds, depth, link_labels, pixel_capacity, geom, scene, offsets, counts, scratch, labels, values,
                                       gt_rows, gt_nchan, capacity, dest, img_labels, img_values, img_gt_labels, img_gt_values,
                                       image_capacity, (hipStream_t)stream);
    return check_launch("depth_annotated_images");
}
