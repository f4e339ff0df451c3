// depth_sensor.hip -- a depth sensor's defects applied to the clean crops the renderer writes (gfx950): range-dependent noise, holes, dropout
// at depth discontinuities and disparity quantisation (include/ancsh_hip.h, ancsh_depth_sensor_model).  ONE launch on depth.hip's grid and
// chunking, every size read from device memory.
//
// Block (x, f) owns chunk x of frame f's crop, as in the annotation's passes.  A thread takes one pixel per step, consecutive lanes
// consecutive pixels: the pixel, its label and -- only when the edge term is on -- its four neighbours inside the crop are read from the CLEAN
// input, so the result does not depend on the order in which pixels are written and the input and output buffers must not overlap.  A
// pixel's four draws are splitmix64 of a key made of (tag 0xE, the frame's GLOBAL index, the pixel's index in the crop, the draw): no
// state, no atomics, no workgroup waits for another.  The arithmetic is float64 without contraction and without a transcendental function:
// the output is a pure function of the input, byte for byte the one tests/depth_sensor_mirror.py computes on the host.
#include "depth_common.h"
#include "pose_shared.h"

namespace ancsh {

constexpr int SN_SCENE = ANCSH_SCENE_WIDTH, SN_DEPTH_SCALE = 6;
constexpr unsigned long long SN_TAG = 0xE000000000000000ull;
constexpr unsigned char SN_BACKGROUND = 255;

struct SensorTable {                        // the launch's table, in registers (uniform)
    double a0, a1, a2, z0, p_hole, p_edge, edge_rel, qd, steps, z_near, z_far;
};

__device__ __forceinline__ double sensor_uniform(unsigned long long r) { return (double)(r >> 11) * 0x1p-53; }

__device__ __forceinline__ bool sensor_store(double v, unsigned short &out) {      // -> false: the pixel is dropped
    const double q = rint(v);
    if (!(q >= 1.0 && q <= 65535.0)) return false;
    out = (unsigned short)q;
    return true;
}
__device__ __forceinline__ bool sensor_store(double v, float &out) {
    out = (float)v;
    return depth_ok(out);
}

// KEYED: `seed` is the address of an ancsh_stream_key (its seed first) and the draws use the global frame index cloud_base + f; unkeyed, the
// base is a constant 0.
template <typename T, bool KEYED>
__global__ __launch_bounds__(DEPTH_THREADS) void depth_sensor_kernel(const T *__restrict__ depth_in, const unsigned char *__restrict__ labels_in,
                                                                     long pixel_capacity, const int *__restrict__ geom,
                                                                     const double *__restrict__ scene, const double *__restrict__ sensor,
                                                                     const unsigned long long *__restrict__ seed, int chunks,
                                                                     T *__restrict__ depth_out, unsigned char *__restrict__ labels_out) {
    const int f = blockIdx.y, x = blockIdx.x;
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);
    if (n == 0) return;                                                 // uniform: a crop the host would have refused writes nothing
    depth_chunk(start, n, x, chunks, lo, hi);
    if (hi <= lo) return;                                               // uniform
    const SensorTable t = {sensor[0], sensor[1], sensor[2], sensor[3], sensor[4], sensor[5], sensor[6], sensor[7], sensor[8], sensor[9], sensor[10]};
    const double depth_scale = scene[(size_t)f * SN_SCENE + SN_DEPTH_SCALE];
    const unsigned long long s = seed[0];
    const unsigned long long g = (unsigned)(KEYED ? f + ((const ancsh_stream_key *)seed)->cloud_base : f);
    const unsigned long long frame_key = SN_TAG | (g << 36);
    for (long a = lo + threadIdx.x; a < hi; a += DEPTH_THREADS) {
        const T stored = depth_in[a];
        const unsigned char label = labels_in[a];
        T out_d = stored;
        unsigned char out_l = label;
        if (label != SN_BACKGROUND && depth_ok(stored)) {               // a surface pixel; every other pixel is copied verbatim
            const long p = a - start;
            const double z = (double)stored * depth_scale;
            const unsigned long long pixel_key = frame_key | ((unsigned long long)p << 4);
            bool keep = t.z_near <= z && z <= t.z_far;
            if (keep) keep = !(sensor_uniform(pose::splitmix64(s ^ pose::splitmix64(pixel_key | 0ull))) < t.p_hole);
            if (keep && t.p_edge > 0.0) {
                const long i = p / w, j = p - i * w;
                const double reach = t.edge_rel * z;
                bool edge = false;
                const long nb[4] = {a - w, a + w, a - 1, a + 1};
                const bool in[4] = {i > 0, (i + 1) * (long)w < n, j > 0, j + 1 < w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (in[k]) {
                        const T dn = depth_in[nb[k]];
                        if (labels_in[nb[k]] == SN_BACKGROUND || !depth_ok(dn)) edge = true;
                        else if (fabs((double)dn * depth_scale - z) > reach) edge = true;
                    }
                if (edge) keep = !(sensor_uniform(pose::splitmix64(s ^ pose::splitmix64(pixel_key | 1ull))) < t.p_edge);
            }
            if (keep) {
                const unsigned long long r2 = pose::splitmix64(s ^ pose::splitmix64(pixel_key | 2ull));
                const unsigned long long r3 = pose::splitmix64(s ^ pose::splitmix64(pixel_key | 3ull));
                const unsigned long long S = (r2 >> 32) + (r2 & 0xFFFFFFFFull) + (r3 >> 32) + (r3 & 0xFFFFFFFFull);
                const double nrm = ((double)S * 0x1p-32 - 2.0) * 1.7320508075688772;
                const double dz = z - t.z0;
                const double sigma = (t.a0 + t.a1 * dz) + t.a2 * (dz * dz);
                const double z1 = z + sigma * nrm;
                double z2 = z1;
                if (t.qd > 0.0) {
                    const double dq = rint((t.qd / z1) * t.steps) / t.steps;
                    if (dq > 0.0) z2 = t.qd / dq;
                    else keep = false;
                }
                if (keep && __double_as_longlong(z2) != __double_as_longlong(z)) keep = sensor_store(z2 / depth_scale, out_d);
            }
            if (!keep) out_d = T(0), out_l = SN_BACKGROUND;
        }
        depth_out[a] = out_d;
        labels_out[a] = out_l;
    }
}

template <typename T>
static void depth_sensor_launch(bool keyed, int nframes, const void *depth_in, const unsigned char *labels_in, long pixel_capacity,
                                const int *geom, const double *scene, const double *sensor, const void *seed, void *depth_out,
                                unsigned char *labels_out, hipStream_t st) {
    const long chunks = depth_chunks(pixel_capacity, nframes);
    const dim3 grid((unsigned)chunks, nframes), block(DEPTH_THREADS);
    if (keyed)
        hipLaunchKernelGGL((depth_sensor_kernel<T, true>), grid, block, 0, st, (const T *)depth_in, labels_in, pixel_capacity, geom, scene, sensor,
                           (const unsigned long long *)seed, (int)chunks, (T *)depth_out, labels_out);
    else
        hipLaunchKernelGGL((depth_sensor_kernel<T, false>), grid, block, 0, st, (const T *)depth_in, labels_in, pixel_capacity, geom, scene, sensor,
                           (const unsigned long long *)seed, (int)chunks, (T *)depth_out, labels_out);
}

static bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const size_t pa = (size_t)a, pb = (size_t)b;
    return pa < pb + nb && pb < pa + na;
}

static int depth_sensor_entry(const char *what, bool keyed, int nframes, int depth_type, const void *depth_in, const unsigned char *labels_in,
                              long pixel_capacity, const int *geom, const double *scene, const double *sensor, const void *seed,
                              void *depth_out, unsigned char *labels_out, void *stream) {
    ANCSH_REQUIRE(nframes >= 0, "%s: bad shape nframes=%d", what, nframes);
    ANCSH_REQUIRE(nframes <= 65535, "%s: %d frames exceed the 65535-frame grid range; split the batch", what, nframes);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32, "%s: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)",
                  what, depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 30), "%s: pixel_capacity=%ld pixels out of range", what, pixel_capacity);
    ANCSH_REQUIRE(depth_in && labels_in && geom && scene && sensor && seed && depth_out && labels_out, "%s: null pointer", what);
    ANCSH_REQUIRE(((size_t)depth_in & 15) == 0 && ((size_t)depth_out & 15) == 0 && ((size_t)labels_in & 7) == 0 && ((size_t)labels_out & 7) == 0 &&
                      ((size_t)scene & 7) == 0 && ((size_t)sensor & 7) == 0 && ((size_t)seed & 7) == 0,
                  "%s: depth_in and depth_out must be 16-byte aligned; labels_in, labels_out, scene, sensor and the %s 8-byte aligned", what,
                  keyed ? "key" : "seed");
    const size_t nd = (size_t)pixel_capacity * (depth_type == ANCSH_DEPTH_U16 ? 2 : 4), nl = (size_t)pixel_capacity;
    ANCSH_REQUIRE(!ranges_overlap(depth_in, nd, depth_out, nd) && !ranges_overlap(depth_in, nd, labels_out, nl) &&
                      !ranges_overlap(labels_in, nl, depth_out, nd) && !ranges_overlap(labels_in, nl, labels_out, nl) &&
                      !ranges_overlap(depth_out, nd, labels_out, nl),
                  "%s: the input and output pixel buffers overlap (a pixel's neighbours are read from the clean input while others are written)",
                  what);
    if (nframes == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        depth_sensor_launch<unsigned short>(keyed, nframes, depth_in, labels_in, pixel_capacity, geom, scene, sensor, seed, depth_out, labels_out,
                                            (hipStream_t)stream);
    else
        depth_sensor_launch<float>(keyed, nframes, depth_in, labels_in, pixel_capacity, geom, scene, sensor, seed, depth_out, labels_out,
                                   (hipStream_t)stream);
    return check_launch(what);
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_depth_sensor_model(int nframes, int depth_type, const void *depth_in, const unsigned char *labels_in, long pixel_capacity,
                                        const int *geom, const double *scene, const double *sensor, const unsigned long long *seed,
                                        void *depth_out, unsigned char *labels_out, void *stream) {
    return depth_sensor_entry("depth_sensor_model", false, nframes, depth_type, depth_in, labels_in, pixel_capacity, geom, scene, sensor, seed,
                              depth_out, labels_out, stream);
}

extern "C" int ancsh_depth_sensor_model_keyed(int nframes, int depth_type, const void *depth_in, const unsigned char *labels_in,
                                              long pixel_capacity, const int *geom, const double *scene, const double *sensor,
                                              const ancsh_stream_key *key, void *depth_out, unsigned char *labels_out, void *stream) {
    return depth_sensor_entry("depth_sensor_model_keyed", true, nframes, depth_type, depth_in, labels_in, pixel_capacity, geom, scene, sensor, key,
                              depth_out, labels_out, stream);
}
