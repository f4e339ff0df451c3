// input.hip -- the sampling step in front of the network, on the GPU (gfx950).
//
// Reference: lib/dataset.py:290-351 (create_unit_data_from_hdf5, after the per-part arrays are concatenated): a cloud
// with fewer raw points than num_points is TILED (np.concatenate([arr] * tile_n), :290-317), a random permutation picks
// num_points rows (:341-351), the coordinates are scaled by the category's norm_factor (:346), the part label becomes a
// one-hot mask_array (:357) and joint_cls_mask = (joint_cls > 0) (:353-355) -- one numpy fancy-index per array per
// cloud on the host.  Here a whole ragged batch is ONE launch: row i of cloud b reads raw row perm[b][i] % n_raw[b]
// (the tiled array is never materialised: tiled[t] == raw[t % n_raw]) and writes every output.
// HBM-bound: 4*nchan B read + 4*(nchan + n_parts + 1) B written per sampled point; the raw rows of one cloud
// (<= a few hundred KB) are L2-resident while its num_points rows are gathered.
#include "common.h"

namespace ancsh {

// one thread per (sampled row, channel group): lanes of a wave cover consecutive channels of consecutive rows, so the
// output streams are written coalesced; the gathered source row is 4*nchan contiguous bytes.
__global__ __launch_bounds__(256) void input_sample_kernel(int num_points, int nchan, const float *__restrict__ rows,
                                                           const int *__restrict__ offsets, const int *__restrict__ perm,
                                                           const float *__restrict__ norm_factor, int cls_col, int jcls_col,
                                                           int n_parts, float *__restrict__ P, float *__restrict__ chan_out,
                                                           float *__restrict__ mask_array, float *__restrict__ joint_cls_mask) {
    const int b = blockIdx.y;
    const int r0 = offsets[b];
    const int n_raw = offsets[b + 1] - r0;
    if (n_raw <= 0) return;                                // an empty cloud leaves its outputs untouched
    const float nf = norm_factor[b];
    const int cout = nchan - 3;                            // channels besides xyz
    const int width = nchan + n_parts + 1;                 // work items per sampled row: nchan copies, n_parts mask entries, 1 joint mask
    const long total = (long)num_points * width;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / width), k = (int)(e - (long)i * width);
        const size_t o = (size_t)b * num_points + i;
        const int t = perm[o];                             // index into the (virtually) tiled cloud
        const float *src = rows + (size_t)(r0 + t % n_raw) * nchan;
        if (k < 3) {
            P[o * 3 + k] = src[k] * nf;
        } else if (k < nchan) {
            chan_out[o * cout + (k - 3)] = src[k];
        } else if (k < nchan + n_parts) {
            const int lab = (int)(signed char)(int)src[cls_col];      // astype(np.int8) like the reference (:357)
            mask_array[o * n_parts + (k - nchan)] = (lab == k - nchan || lab + n_parts == k - nchan) ? 1.f : 0.f;
        } else {
            joint_cls_mask[o] = (jcls_col >= 0 && src[jcls_col] > 0.f) ? 1.f : 0.f;
        }
    }
}

// ---- the streaming sampler: graph-capturable, every size read from device memory (include/ancsh_hip.h) -------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {     // the pose generator's finaliser (pose_shared.h)
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the sampler's keys: bits 60..63 set, which no pose draw key (problem << 40 | iteration << 8 | k) has below 2^20 problems
constexpr unsigned long long SAMPLE_TAG = 0xF000000000000000ull;

// pi(i): a 4-round Feistel network on 2h bits (round r: L, R = R, L ^ (splitmix64(key[r] ^ R) & mask)), cycle-walked into [0, T):
// a bijection of [0, 2^2h) restricted to the cycle of i until it lands below T, so a bijection of [0, T).  2^2h < 4T: < 4 walks
// on average.
__device__ __forceinline__ unsigned long long feistel_index(unsigned long long i, unsigned long long T, int h,
                                                            const unsigned long long key[4]) {
    const unsigned long long mask = (1ull << h) - 1ull;
    unsigned long long x = i;
    do {
        unsigned long long L = x >> h, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned long long t = L ^ (splitmix64(key[r] ^ R) & mask);
            L = R;
            R = t;
        }
        x = (L << h) | R;
    } while (x >= T);
    return x;
}

// one thread per sampled row; the gathered source row (16 B for nchan = 4) of a cloud of a few thousand rows is L2-resident.
// KEYED: `seed` is the address of an ancsh_stream_key (its seed first) and the round keys use the global cloud index cloud_base + b;
// unkeyed, the base is a constant 0 and the code is that of the plain entry.
// XYZ: rows without a joint-class channel (nchan >= 3; a 12-byte row is not 16-byte aligned, so the three coordinates are read as the
// scalar loads below) and no joint_cls output; jcls_col / joint_cls are never read.  P and perm_out are those of the 4-column kernel.
template <bool KEYED, bool XYZ = false>
__global__ __launch_bounds__(256) void input_sample_stream_kernel(int num_points, int nchan, const float *__restrict__ rows,
                                                                  long capacity, const int *__restrict__ offsets,
                                                                  const float *__restrict__ norm_factor, int jcls_col,
                                                                  const unsigned long long *__restrict__ seed, float *__restrict__ P,
                                                                  int *__restrict__ joint_cls, int *__restrict__ perm_out) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_points) return;
    const long r0 = offsets[b], r1 = offsets[b + 1];
    if (r0 < 0 || r1 <= r0 || r1 > capacity) return;     // empty or outside the rows buffer (the host refuses both): outputs untouched
    const unsigned long long n_raw = (unsigned long long)(r1 - r0), n = (unsigned long long)num_points;
    const unsigned long long T = n_raw >= n ? n_raw : (n / n_raw + 1) * n_raw;      // the tiled size (lib/dataset.py:290-293)
    int w = 0;
    while ((1ull << w) < T) w += 2;
    const unsigned long long s = *seed;
    const int cb = KEYED ? b + ((const ancsh_stream_key *)seed)->cloud_base : b;
    unsigned long long key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) key[r] = splitmix64(s ^ splitmix64(SAMPLE_TAG | ((unsigned long long)cb << 8) | (unsigned)r));
    const unsigned long long t = feistel_index((unsigned long long)i, T, w / 2, key);
    const float *src = rows + (size_t)(r0 + (long)(t % n_raw)) * nchan;
    const float nf = norm_factor[b];
    const size_t o = (size_t)b * num_points + i;
    P[o * 3] = src[0] * nf;
    P[o * 3 + 1] = src[1] * nf;
    P[o * 3 + 2] = src[2] * nf;
    if (!XYZ) joint_cls[o] = (int)src[jcls_col];        // C truncation, as np.asarray(x, np.int32)
    if (perm_out) perm_out[o] = (int)t;
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_input_sample(int nclouds, int num_points, int nchan, const float *rows, const int *offsets, const int *perm,
                                  const float *norm_factor, int cls_col, int jcls_col, int n_parts, float *P, float *chan_out,
                                  float *mask_array, float *joint_cls_mask, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0 && num_points > 0, "input_sample: bad shape nclouds=%d num_points=%d", nclouds, num_points);
    ANCSH_REQUIRE(nchan >= 3, "input_sample: rows need at least the 3 coordinate channels (nchan=%d)", nchan);
    ANCSH_REQUIRE(cls_col >= 3 && cls_col < nchan, "input_sample: cls_col=%d must name a channel in [3,%d)", cls_col, nchan);
    ANCSH_REQUIRE(jcls_col < nchan && (jcls_col < 0 || jcls_col >= 3), "input_sample: jcls_col=%d out of range", jcls_col);
    ANCSH_REQUIRE(n_parts > 0 && n_parts <= 64, "input_sample: n_parts=%d must be in [1,64]", n_parts);
    ANCSH_REQUIRE(nclouds <= 65535, "input_sample: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    if (nclouds == 0) return ANCSH_OK;
    ANCSH_REQUIRE(rows && offsets && perm && norm_factor && P && mask_array && joint_cls_mask && (nchan == 3 || chan_out),
                  "input_sample: null pointer");
    const long total = (long)num_points * (nchan + n_parts + 1);
    long bx = (total + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(input_sample_kernel, dim3((unsigned)bx, nclouds), dim3(256), 0, (hipStream_t)stream, num_points, nchan, rows,
                       offsets, perm, norm_factor, cls_col, jcls_col, n_parts, P, chan_out, mask_array, joint_cls_mask);
    return check_launch("input_sample");
}

extern "C" int ancsh_input_sample_stream(int nclouds, int num_points, int nchan, const float *rows, long capacity, const int *offsets,
                                         const float *norm_factor, int jcls_col, const unsigned long long *seed, float *P,
                                         int *joint_cls, int *perm_out, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0 && num_points > 0 && num_points < (1 << 30), "input_sample_stream: bad shape nclouds=%d num_points=%d",
                  nclouds, num_points);
    ANCSH_REQUIRE(nchan >= 4, "input_sample_stream: rows need x y z and the joint-class channel (nchan=%d < 4)", nchan);
    ANCSH_REQUIRE(jcls_col >= 3 && jcls_col < nchan, "input_sample_stream: jcls_col=%d must name a channel in [3,%d)", jcls_col, nchan);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "input_sample_stream: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(nclouds <= 65535, "input_sample_stream: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(seed, "input_sample_stream: null seed pointer");
    ANCSH_REQUIRE(rows && offsets && norm_factor && P && joint_cls, "input_sample_stream: null pointer");
    if (nclouds == 0) return ANCSH_OK;
    hipLaunchKernelGGL(input_sample_stream_kernel<false>, dim3((num_points + 255) / 256, nclouds), dim3(256), 0, (hipStream_t)stream, num_points,
                       nchan, rows, capacity, offsets, norm_factor, jcls_col, seed, P, joint_cls, perm_out);
    return check_launch("input_sample_stream");
}

extern "C" int ancsh_input_sample_stream_keyed(int nclouds, int num_points, int nchan, const float *rows, long capacity,
                                               const int *offsets, const float *norm_factor, int jcls_col, const ancsh_stream_key *key,
                                               float *P, int *joint_cls, int *perm_out, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0 && num_points > 0 && num_points < (1 << 30), "input_sample_stream_keyed: bad shape nclouds=%d num_points=%d",
                  nclouds, num_points);
    ANCSH_REQUIRE(nchan >= 4, "input_sample_stream_keyed: rows need x y z and the joint-class channel (nchan=%d < 4)", nchan);
    ANCSH_REQUIRE(jcls_col >= 3 && jcls_col < nchan, "input_sample_stream_keyed: jcls_col=%d must name a channel in [3,%d)", jcls_col,
                  nchan);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "input_sample_stream_keyed: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(nclouds <= 65535, "input_sample_stream_keyed: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(key, "input_sample_stream_keyed: null key pointer");
    ANCSH_REQUIRE(rows && offsets && norm_factor && P && joint_cls, "input_sample_stream_keyed: null pointer");
    if (nclouds == 0) return ANCSH_OK;
    hipLaunchKernelGGL(input_sample_stream_kernel<true>, dim3((num_points + 255) / 256, nclouds), dim3(256), 0, (hipStream_t)stream,
                       num_points, nchan, rows, capacity, offsets, norm_factor, jcls_col, &key->seed, P, joint_cls, perm_out);
    return check_launch("input_sample_stream_keyed");
}

// the xyz-only twins (rows of nchan >= 3 channels, x y z first; no joint-class channel, no joint_cls output): the kernel above with XYZ
extern "C" int ancsh_input_sample_stream_xyz(int nclouds, int num_points, int nchan, const float *rows, long capacity, const int *offsets,
                                             const float *norm_factor, const unsigned long long *seed, float *P, int *perm_out,
                                             void *stream) {
    ANCSH_REQUIRE(nclouds >= 0 && num_points > 0 && num_points < (1 << 30), "input_sample_stream_xyz: bad shape nclouds=%d num_points=%d",
                  nclouds, num_points);
    ANCSH_REQUIRE(nchan >= 3, "input_sample_stream_xyz: rows need x y z (nchan=%d < 3)", nchan);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "input_sample_stream_xyz: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(nclouds <= 65535, "input_sample_stream_xyz: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(seed, "input_sample_stream_xyz: null seed pointer");
    ANCSH_REQUIRE(rows && offsets && norm_factor && P, "input_sample_stream_xyz: null pointer");
    if (nclouds == 0) return ANCSH_OK;
    hipLaunchKernelGGL((input_sample_stream_kernel<false, true>), dim3((num_points + 255) / 256, nclouds), dim3(256), 0, (hipStream_t)stream,
                       num_points, nchan, rows, capacity, offsets, norm_factor, 0, seed, P, nullptr, perm_out);
    return check_launch("input_sample_stream_xyz");
}

extern "C" int ancsh_input_sample_stream_xyz_keyed(int nclouds, int num_points, int nchan, const float *rows, long capacity,
                                                   const int *offsets, const float *norm_factor, const ancsh_stream_key *key, float *P,
                                                   int *perm_out, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0 && num_points > 0 && num_points < (1 << 30),
                  "input_sample_stream_xyz_keyed: bad shape nclouds=%d num_points=%d", nclouds, num_points);
    ANCSH_REQUIRE(nchan >= 3, "input_sample_stream_xyz_keyed: rows need x y z (nchan=%d < 3)", nchan);
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "input_sample_stream_xyz_keyed: capacity=%ld rows out of range", capacity);
    ANCSH_REQUIRE(nclouds <= 65535, "input_sample_stream_xyz_keyed: %d clouds exceed the 65535-cloud grid range; split the batch", nclouds);
    ANCSH_REQUIRE(key, "input_sample_stream_xyz_keyed: null key pointer");
    ANCSH_REQUIRE(rows && offsets && norm_factor && P, "input_sample_stream_xyz_keyed: null pointer");
    if (nclouds == 0) return ANCSH_OK;
    hipLaunchKernelGGL((input_sample_stream_kernel<true, true>), dim3((num_points + 255) / 256, nclouds), dim3(256), 0, (hipStream_t)stream,
                       num_points, nchan, rows, capacity, offsets, norm_factor, 0, &key->seed, P, nullptr, perm_out);
    return check_launch("input_sample_stream_xyz_keyed");
}
