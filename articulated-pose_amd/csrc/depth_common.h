// depth_common.h -- what the depth front end's two entries share (depth.hip: object masks -> xyz rows; depth_annotate.hip: link labels ->
// annotated rows; their inverses, rows -> images): the crop geometry, the chunking of a crop over the grid, the validity of a depth value, the
// block sum and the span store of the image kernels.
#pragma once
#include "common.h"

namespace ancsh {

constexpr int DEPTH_THREADS = 256, DEPTH_WAVES = DEPTH_THREADS / 64;
constexpr int DEPTH_CHUNKS = ANCSH_DEPTH_MAX_CHUNKS;
constexpr int DEPTH_GEOM = 5, DEPTH_CAM = 7;            // ints / floats per cloud

__device__ __forceinline__ bool depth_ok(unsigned short d) { return d != 0; }
__device__ __forceinline__ bool depth_ok(float d) { return d > 0.f && d < __builtin_inff(); }       // NaN fails both

// cloud b's crop: its first pixel `start`, width w and pixel count (0: a crop the host would have refused -- h or w < 1, or outside the
// pixel buffer; such a cloud is handled like one without a valid pixel)
__device__ __forceinline__ long depth_crop(const int *__restrict__ geom, int b, long pixel_capacity, long &start, int &w) {
    const int *g = geom + (size_t)b * DEPTH_GEOM;
    start = g[0];
    const int h = g[1];
    w = g[2];
    if (start < 0 || h < 1 || w < 1) return 0;
    const long n = (long)h * w;
    return n <= pixel_capacity - start ? n : 0;
}

// the pixels [lo, hi) of the buffer that chunk x of `chunks` owns
__device__ __forceinline__ void depth_chunk(long start, long n, int x, int chunks, long &lo, long &hi) {
    const long per = (n + chunks - 1) / chunks;
    lo = start + (long)x * per;
    hi = start + ((long)(x + 1) * per < n ? (long)(x + 1) * per : n);
    if (lo > hi) lo = hi;
}

__device__ __forceinline__ long depth_block_sum(long v, long *s_red) {      // sum over the block, uniform result
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                                    // s_red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long t = 0;
#pragma unroll
    for (int k = 0; k < DEPTH_WAVES; ++k) t += s_red[k];
    return t;
}

// the grid is a function of (pixel_capacity, nclouds) alone: ~2048 pixels of an even share per chunk, at most DEPTH_CHUNKS chunks a cloud
static long depth_chunks(long pixel_capacity, int nclouds) {
    const long chunks = (pixel_capacity / nclouds + 2047) / 2048;
    return chunks < 1 ? 1 : chunks > DEPTH_CHUNKS ? DEPTH_CHUNKS : chunks;
}

// `total` dwords at `out`, dword e = value(e): whole 16-byte vectors where the address allows, single dwords in front of and behind them.
// Consecutive lanes store consecutive addresses either way.
template <typename F>
__device__ __forceinline__ void depth_store_span(unsigned *__restrict__ out, long total, F value) {
    long head = (long)(((16 - ((size_t)out & 15)) & 15) >> 2);
    head = head < total ? head : total;
    const long body = (total - head) >> 2;
    for (long e = threadIdx.x; e < head; e += DEPTH_THREADS) out[e] = value(e);
    uint4 *o4 = reinterpret_cast<uint4 *>(out + head);
    for (long v = threadIdx.x; v < body; v += DEPTH_THREADS) {
        const long e = head + 4 * v;
        o4[v] = make_uint4(value(e), value(e + 1), value(e + 2), value(e + 3));
    }
    for (long e = head + 4 * body + threadIdx.x; e < total; e += DEPTH_THREADS) out[e] = value(e);
}

}  // namespace ancsh
