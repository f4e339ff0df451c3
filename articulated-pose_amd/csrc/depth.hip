// depth.hip -- the depth front end of the streaming pipeline (gfx950): masked depth crops -> packed camera-space rows.
//
// Reference: tools/preprocess_data.py:259-298 -- a label mask picks the pixels (np.where, row-major), projMat back-projects them into
// camera space (cloud_cam_real).  Here a ragged batch of crops is TWO launches in front of the xyz sampler (input.hip), every size read
// from device memory (include/ancsh_hip.h, ancsh_depth_unproject_stream):
//   count   : block (x, b) counts the valid pixels of chunk x of cloud b's crop -> scratch[b * chunks + x];
//   scatter : block (x, b) sums the counts in front of its chunk (one block reduction over <= (b + 1) * chunks ints), recomputes validity
//             and writes its rows in pixel order.  No atomics, no workgroup waits for another: the order is a pure function of the input.
// A lane reads 16 bytes of depth (8 uint16 / 4 float32 pixels) and the matching mask bytes per step; the groups are aligned in the pixel
// buffer, not in the crop, so a crop may start at any pixel.  The data is a few MB per batch: the two launches, not HBM, are the cost.
#include "depth_common.h"

namespace ancsh {

// the V = 16 / sizeof(T) pixels [a0, a0 + V) of the buffer (a0 a multiple of V) -> d[], and the bit set of those that are valid pixels of
// [lo, hi).  A group that reaches past the buffer's end is read pixel by pixel.
template <typename T>
__device__ __forceinline__ unsigned depth_group(const T *__restrict__ depth, const unsigned char *__restrict__ mask, long a0, long lo, long hi,
                                                long pixel_capacity, T (&d)[16 / sizeof(T)]) {
    constexpr int V = 16 / sizeof(T);
    union { uint4 q; T e[V]; } u;
    union { uint2 q; unsigned char e[8]; } m;
    if (a0 + V <= pixel_capacity) {
        u.q = *reinterpret_cast<const uint4 *>(depth + a0);
        if (!mask) m.q = make_uint2(~0u, ~0u);
        else if (V == 8) m.q = *reinterpret_cast<const uint2 *>(mask + a0);
        else m.q = make_uint2(*reinterpret_cast<const unsigned *>(mask + a0), 0u);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool in = a0 + k < pixel_capacity;
            u.e[k] = in ? depth[a0 + k] : T(0);
            m.e[k] = in && (!mask || mask[a0 + k]) ? 1 : 0;
        }
    }
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        d[k] = u.e[k];
        const long a = a0 + k;
        if (a >= lo && a < hi && m.e[k] && depth_ok(u.e[k])) bits |= 1u << k;
    }
    return bits;
}

template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void depth_count_kernel(const T *__restrict__ depth, const unsigned char *__restrict__ mask,
                                                                    long pixel_capacity, const int *__restrict__ geom, int chunks,
                                                                    int *__restrict__ scratch) {
    constexpr int V = 16 / sizeof(T);
    __shared__ long s_red[DEPTH_WAVES];
    const int b = blockIdx.y, x = blockIdx.x;
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, b, pixel_capacity, start, w);
    depth_chunk(start, n, x, chunks, lo, hi);
    long c = 0;
    if (hi > lo) {
        const long g0 = lo / V, ng = (hi - 1) / V - g0 + 1;
        for (long g = threadIdx.x; g < ng; g += DEPTH_THREADS) {
            T d[V];
            c += __popc(depth_group<T>(depth, mask, (g0 + g) * V, lo, hi, pixel_capacity, d));
        }
    }
    const long t = depth_block_sum(c, s_red);
    if (threadIdx.x == 0) scratch[(size_t)b * chunks + x] = (int)t;
}

template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void depth_scatter_kernel(int nclouds, const T *__restrict__ depth,
                                                                      const unsigned char *__restrict__ mask, long pixel_capacity,
                                                                      const int *__restrict__ geom, const float *__restrict__ cam, int chunks,
                                                                      const int *__restrict__ scratch, float *__restrict__ rows, long capacity,
                                                                      int *__restrict__ offsets, int *__restrict__ counts) {
    constexpr int V = 16 / sizeof(T);
    __shared__ long s_red[DEPTH_WAVES];
    __shared__ long s_own[2];
    __shared__ int s_wave[2][DEPTH_WAVES];
    const int b = blockIdx.y, x = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // rows in front of this chunk: max(count, 1) of every earlier cloud (an empty cloud owns one NaN row), and this cloud's earlier chunks
    long before = 0;
    for (int c = threadIdx.x; c <= b; c += DEPTH_THREADS) {
        const int *s = scratch + (size_t)c * chunks;
        long tot = 0, head = 0;
        for (int k = 0; k < chunks; ++k) {
            if (k == x) head = tot;
            tot += s[k];
        }
        if (c < b) before += tot > 1 ? tot : 1;
        else s_own[0] = tot, s_own[1] = head;
    }
    const long cloud_base = depth_block_sum(before, s_red);             // its barriers publish s_own
    const long total = s_own[0];
    long base = cloud_base + s_own[1];
    if (x == 0 && threadIdx.x == 0) {
        const long end = cloud_base + (total > 1 ? total : 1);
        offsets[b] = (int)(cloud_base < 0x7fffffffL ? cloud_base : 0x7fffffffL);
        counts[b] = (int)total;
        if (b == nclouds - 1) offsets[nclouds] = (int)(end < 0x7fffffffL ? end : 0x7fffffffL);
        if (total == 0 && cloud_base < capacity) {
            const float q = __builtin_nanf("");
            rows[cloud_base * 3] = q, rows[cloud_base * 3 + 1] = q, rows[cloud_base * 3 + 2] = q;
        }
    }
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, b, pixel_capacity, start, w);
    depth_chunk(start, n, x, chunks, lo, hi);
    if (hi <= lo) return;                                               // uniform
    const int row0 = geom[(size_t)b * DEPTH_GEOM + 3], col0 = geom[(size_t)b * DEPTH_GEOM + 4];
    const float *A = cam + (size_t)b * DEPTH_CAM;
    const float A00 = A[0], A01 = A[1], A02 = A[2], A10 = A[3], A11 = A[4], A12 = A[5], scale = A[6];
    const long g0 = lo / V, ng = (hi - 1) / V - g0 + 1;
    int buf = 0;
    for (long gb = 0; gb < ng; gb += DEPTH_THREADS, buf ^= 1) {         // uniform trip count: every wave reaches the barrier
        const long g = gb + threadIdx.x;
        T d[V];
        const unsigned bits = g < ng ? depth_group<T>(depth, mask, (g0 + g) * V, lo, hi, pixel_capacity, d) : 0u;
        const int c = __popc(bits);
        int incl = c;                                                   // inclusive scan over the wave, in lane (= pixel) order
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[buf][wave] = incl;
        __syncthreads();                                                // s_wave is double-buffered: one barrier per step
        int wave_base = 0, step = 0;
#pragma unroll
        for (int k = 0; k < DEPTH_WAVES; ++k) {
            const int v = s_wave[buf][k];
            if (k < wave) wave_base += v;
            step += v;
        }
        if (bits) {
            long r = base + wave_base + (incl - c);
            const long p0 = (g0 + g) * V - start;                       // crop position of the group's first pixel; < 0 only in front of lo
            int i = p0 >= 0 ? (int)(p0 / w) : 0, j = (int)(p0 - (long)i * w);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (bits >> k & 1u) {
                    const float row = (float)(row0 + i), col = (float)(col0 + j);
                    const float z = (float)d[k] * scale;
                    const float gx = fmaf(A01, row, fmaf(A00, col, A02)), gy = fmaf(A11, row, fmaf(A10, col, A12));
                    if (r < capacity) rows[r * 3] = z * gx, rows[r * 3 + 1] = z * gy, rows[r * 3 + 2] = z;
                    ++r;
                }
                if (++j == w) j = 0, ++i;
            }
        }
        base += step;
    }
}

template <typename T>
static void depth_launch(int nclouds, const void *depth, const unsigned char *mask, long pixel_capacity, const int *geom, const float *cam,
                         float *rows, long capacity, int *offsets, int *counts, int *scratch, hipStream_t st) {
    const long chunks = depth_chunks(pixel_capacity, nclouds);
    const dim3 grid((unsigned)chunks, nclouds);
    hipLaunchKernelGGL(depth_count_kernel<T>, grid, dim3(DEPTH_THREADS), 0, st, (const T *)depth, mask, pixel_capacity, geom, (int)chunks,
                       scratch);
    hipLaunchKernelGGL(depth_scatter_kernel<T>, grid, dim3(DEPTH_THREADS), 0, st, nclouds, (const T *)depth, mask, pixel_capacity, geom, cam,
                       (int)chunks, scratch, rows, capacity, offsets, counts);
}

// ---- the inverse of the compaction: per-row labels / values -> per-pixel images (include/ancsh_hip.h, ancsh_depth_label_images) ----------
// Block (x, b) on the count / scatter passes' grid and chunking.  Its first row is offsets[b] + the counts of cloud b's earlier chunks, read
// from the scratch the count pass left.  Per step of 256 groups: validity and the wave scan exactly as depth_scatter_kernel ranks its rows ->
// the source row of every pixel of the step in LDS (-1: not a valid pixel, or a row cut at capacity); then the block stores the step's
// labels and values as two contiguous spans.  labels / values travel as their bits (NaN payloads survive).
template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void depth_label_images_kernel(const T *__restrict__ depth, const unsigned char *__restrict__ mask,
                                                                           long pixel_capacity, const int *__restrict__ geom, int chunks,
                                                                           const int *__restrict__ scratch, const int *__restrict__ offsets,
                                                                           const unsigned *__restrict__ labels,
                                                                           const unsigned *__restrict__ values, long capacity,
                                                                           const int *__restrict__ dest, unsigned *__restrict__ img_labels,
                                                                           unsigned *__restrict__ img_values, long image_capacity) {
    constexpr int V = 16 / sizeof(T), STEP = DEPTH_THREADS * V;
    __shared__ int s_wave[DEPTH_WAVES];
    __shared__ int s_src[STEP];
    const int b = blockIdx.y, x = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, b, pixel_capacity, start, w);
    const long d0 = dest[b];
    if (n == 0 || d0 < 0 || n > image_capacity - d0) return;            // uniform: a silenced cloud, an empty crop, an image past the buffer
    depth_chunk(start, n, x, chunks, lo, hi);
    if (hi <= lo) return;                                               // uniform
    long base = offsets[b];
    for (int k = 0; k < x; ++k) base += scratch[(size_t)b * chunks + k];        // <= 63 broadcast loads
    const long g0 = lo / V, ng = (hi - 1) / V - g0 + 1;
    for (long gb = 0; gb < ng; gb += DEPTH_THREADS) {                   // uniform trip count: every wave reaches the barriers
        const long g = gb + threadIdx.x;
        T d[V];
        const unsigned bits = g < ng ? depth_group<T>(depth, mask, (g0 + g) * V, lo, hi, pixel_capacity, d) : 0u;
        const int c = __popc(bits);
        int incl = c;                                                   // inclusive scan over the wave, in lane (= pixel) order
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();                                                // also: the previous step's readers of s_src are done
        int wave_base = 0, step = 0;
#pragma unroll
        for (int k = 0; k < DEPTH_WAVES; ++k) {
            const int v = s_wave[k];
            if (k < wave) wave_base += v;
            step += v;
        }
        long r = base + wave_base + (incl - c);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool on = bits >> k & 1u;
            s_src[threadIdx.x * V + k] = on && r >= 0 && r < capacity ? (int)r : -1;
            r += on;
        }
        __syncthreads();                                                // s_src is published; s_wave may be rewritten
        const long a0 = (g0 + gb) * V;                                  // the step's window of the pixel buffer, cut to the chunk
        const long pa = a0 > lo ? a0 : lo, pb = a0 + STEP < hi ? a0 + STEP : hi;
        const int *src = s_src + (pa - a0);
        const long q0 = d0 + (pa - start);
        depth_store_span(img_labels + q0, pb - pa, [&](long e) { const int s = src[e]; return s >= 0 ? labels[s] : 0xffffffffu; });
        depth_store_span(img_values + q0 * 7, (pb - pa) * 7, [&](long e) {
            const int p = (int)(e / 7), s = src[p];
            return s >= 0 ? values[(size_t)s * 7 + (e - p * 7)] : (unsigned)ANCSH_LABEL_NAN_BITS;
        });
        base += step;
    }
}

template <typename T>
static void depth_label_images_launch(int nclouds, const void *depth, const unsigned char *mask, long pixel_capacity, const int *geom,
                                      const int *offsets, const int *scratch, const int *labels, const float *values, long capacity,
                                      const int *dest, int *img_labels, float *img_values, long image_capacity, hipStream_t st) {
    const long chunks = depth_chunks(pixel_capacity, nclouds);          // the count pass's chunking: scratch[b * chunks + x] is its layout
    hipLaunchKernelGGL(depth_label_images_kernel<T>, dim3((unsigned)chunks, nclouds), dim3(DEPTH_THREADS), 0, st, (const T *)depth, mask,
                       pixel_capacity, geom, (int)chunks, scratch, offsets, (const unsigned *)labels, (const unsigned *)values, capacity, dest,
                       (unsigned *)img_labels, (unsigned *)img_values, image_capacity);
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_depth_unproject_stream(int nclouds, int depth_type, const void *depth, const unsigned char *mask, long pixel_capacity,
                                            const int *geom, const float *cam, float *rows, long capacity, int *offsets, int *counts,
                                            int *scratch, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0, "depth_unproject_stream: bad shape nclouds=%d", nclouds);
    ANCSH_REQUIRE(nclouds <= 65535, "depth_unproject_stream: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32,
                  "depth_unproject_stream: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 30), "depth_unproject_stream: pixel_capacity=%ld pixels out of range",
                  pixel_capacity);
    ANCSH_REQUIRE(capacity >= pixel_capacity, "depth_unproject_stream: capacity=%ld rows is below pixel_capacity=%ld", capacity,
                  pixel_capacity);
    ANCSH_REQUIRE(depth && geom && cam && rows && offsets && counts && scratch, "depth_unproject_stream: null pointer");
    ANCSH_REQUIRE(((size_t)depth & 15) == 0 && ((size_t)mask & 7) == 0,
                  "depth_unproject_stream: depth must be 16-byte aligned and mask 8-byte aligned (the crops inside them may start anywhere)");
    if (nclouds == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        depth_launch<unsigned short>(nclouds, depth, mask, pixel_capacity, geom, cam, rows, capacity, offsets, counts, scratch,
                                     (hipStream_t)stream);
    else
        depth_launch<float>(nclouds, depth, mask, pixel_capacity, geom, cam, rows, capacity, offsets, counts, scratch, (hipStream_t)stream);
    return check_launch("depth_unproject_stream");
}

extern "C" int ancsh_depth_label_images(int nclouds, int depth_type, const void *depth, const unsigned char *mask, long pixel_capacity,
                                        const int *geom, const int *offsets, const int *scratch, const int *labels, const float *values,
                                        long capacity, const int *dest, int *img_labels, float *img_values, long image_capacity,
                                        void *stream) {
    ANCSH_REQUIRE(nclouds >= 0, "depth_label_images: bad shape nclouds=%d", nclouds);
    ANCSH_REQUIRE(nclouds <= 65535, "depth_label_images: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32,
                  "depth_label_images: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 30), "depth_label_images: pixel_capacity=%ld pixels out of range",
                  pixel_capacity);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "depth_label_images: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(image_capacity >= 0 && image_capacity < (1L << 30), "depth_label_images: image_capacity=%ld pixels out of range",
                  image_capacity);
    ANCSH_REQUIRE(depth && geom && offsets && scratch && labels && values && dest && img_labels && img_values,
                  "depth_label_images: null pointer");
    ANCSH_REQUIRE(((size_t)depth & 15) == 0 && ((size_t)mask & 7) == 0,
                  "depth_label_images: depth must be 16-byte aligned and mask 8-byte aligned (the crops inside them may start anywhere)");
    if (nclouds == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        depth_label_images_launch<unsigned short>(nclouds, depth, mask, pixel_capacity, geom, offsets, scratch, labels, values, capacity,
                                                  dest, img_labels, img_values, image_capacity, (hipStream_t)stream);
    else
        depth_label_images_launch<float>(nclouds, depth, mask, pixel_capacity, geom, offsets, scratch, labels, values, capacity, dest,
                                         img_labels, img_values, image_capacity, (hipStream_t)stream);
    return check_launch("depth_label_images");
}
