// render.hip -- depth and link-label frames of articulated triangle meshes rendered on the GPU (gfx950): the mesh, one render table per frame
// (the pixel map, the depth scale and every link's model -> camera map) and the depth entries' geometry rows -> the depth crops and label
// crops ancsh_depth_annotate_stream reads, where it reads them.
//
// Reference: tools/render_synthetic.py:180-225 renders one frame at a time with pybullet's getCameraImage on the host.  Pixel parity with
// that rasteriser is no goal (its two back ends differ from each other); the contract is geometric -- this is the exact inverse of the
// camera model ancsh_depth_annotate_stream applies to a frame's coordinate point (scene[7..12], depth.coord_unprojection_from_projmat) --
// and is stated in full in include/ancsh_hip.h (ancsh_render_depth_labels).  THREE launches on a ragged batch of crops:
//   clear   : block (x, f) sets the z-buffer keys of chunk x of frame f's crop to the empty key (depth.hip's grid and chunking);
//   raster  : one wave per (triangle, frame): every lane transforms the triangle's three vertices (float64, as written), the wave sweeps
//             the triangle's bounding box clipped to the crop, 64 pixels a step; a covered pixel (int64 edge functions on 1/256-pixel
//             fixed point) takes ONE 64-bit integer atomic minimum on its key, (bits of (float)depth) << 32 | triangle index;
//   resolve : block (x, f) turns the keys of its chunk into depth values and label bytes, background where the key is empty.
// The minimum of a set does not depend on the order of its elements: the output is a pure function of the input, byte for byte.
// float64 arithmetic evaluated as written (the library is built with -ffp-contract=off).
// A LIBRARY of instances (ancsh_render_depth_labels_lib, ancsh_render_centre_crops_lib): the meshes concatenated, tri_off naming each
// instance's triangle range, and the instance of a frame in its table's value 9.  The raster and the centring kernels of either kind are
// wrappers around one device function each (render_raster_wave, render_centre_block); clear and resolve serve both unchanged.
#include "depth_common.h"

namespace ancsh {

constexpr int RN_LINKS = ANCSH_SCENE_MAX_LINKS, RN_HEAD = ANCSH_RENDER_HEAD, RN_LINK = ANCSH_RENDER_LINK, RN_WIDTH = ANCSH_RENDER_WIDTH;
constexpr unsigned long long RN_EMPTY = ~0ull;                         // no real key reaches it: the bits of a float32 are its upper half
constexpr long RN_FIXED_LIMIT = 1L << 25;                               // |X|, |Y| of a kept vertex, in 1/256 pixel

// the table's integers and its near bound, read defensively: a table that is not one renders background
__device__ __forceinline__ int render_nlinks(const double *__restrict__ rt) {
    const double v = rt[8], z_min = rt[7];
    return v >= 1.0 && v <= (double)RN_LINKS && z_min > 0.0 ? (int)v : 0;      // NaN fails every comparison
}

// the triangle range [t_lo, t_hi) of a library frame's instance, render[9]: empty for a value that is no integer in [0, ninst) and for offsets
// that are no range inside [0, T].  One table value and two offsets per wave (raster) or block (centring); nothing is read per pixel
__device__ __forceinline__ void render_instance_range(const double *__restrict__ rt, const int *__restrict__ tri_off, int ninst, int T,
                                                      int &t_lo, int &t_hi) {
    const int i = instance_index(rt[9], ninst);
    t_lo = t_hi = 0;
    if (i < 0) return;
    const int a = tri_off[i], b = tri_off[i + 1];
    if (a < 0 || b < a || b > T) return;
    t_lo = a;
    t_hi = b;
}

__global__ __launch_bounds__(DEPTH_THREADS) void render_clear_kernel(long pixel_capacity, const int *__restrict__ geom, int chunks,
                                                                     unsigned long long *__restrict__ zbuf) {
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, blockIdx.y, pixel_capacity, start, w);
    depth_chunk(start, n, blockIdx.x, chunks, lo, hi);
    for (long a = lo + threadIdx.x; a < hi; a += DEPTH_THREADS) zbuf[a] = RN_EMPTY;      // [lo, hi) lies inside [0, pixel_capacity)
}

struct RenderVertex {
    long X, Y;          // the pixel position in 1/256 pixel: X along the columns, Y along the rows
    double iz;          // 1 / z
    bool ok;
};

// vertex `v` of a link with the map R (row-major 3 x 4) -> its fixed-point pixel and 1 / z; ok = false drops the triangle
__device__ __forceinline__ RenderVertex render_vertex(const float *__restrict__ v, const double *__restrict__ R, const double *__restrict__ rt) {
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    double q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((R[4 * a] * v0 + R[4 * a + 1] * v1) + R[4 * a + 2] * v2) + R[4 * a + 3];
    const double z = q[2], s = q[0] / z, t = q[1] / z;
    const double col = (rt[0] * s + rt[1] * t) + rt[2], row = (rt[3] * s + rt[4] * t) + rt[5];
    const double X = rint(256.0 * col), Y = rint(256.0 * row);
    RenderVertex o;
    // z >= z_min > 0; a NaN or an infinity anywhere fails one of these comparisons
    o.ok = z >= rt[7] && z < __builtin_inf() && fabs(X) < (double)RN_FIXED_LIMIT && fabs(Y) < (double)RN_FIXED_LIMIT;
    o.X = o.ok ? (long)X : 0;
    o.Y = o.ok ? (long)Y : 0;
    o.iz = 1.0 / z;
    return o;
}

__device__ __forceinline__ long render_edge(long ax, long ay, long bx, long by, long px, long py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }
__device__ __forceinline__ long floor_div256(long v) { return v >> 8; }                  // arithmetic shift: floor for either sign
__device__ __forceinline__ long ceil_div256(long v) { return -((-v) >> 8); }

// one wave rasterises triangle t (uniform over the wave, in [0, T)) into frame f's crop: both raster kernels' body
__device__ __forceinline__ void render_raster_wave(const float *__restrict__ verts, const int *__restrict__ tris,
                                                   const int *__restrict__ tri_link, int V, int t, int f, long pixel_capacity,
                                                   const int *__restrict__ geom, const double *__restrict__ rt,
                                                   unsigned long long *__restrict__ zbuf) {
    const int lane = threadIdx.x & 63;
    const int nl = render_nlinks(rt);
    long start;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);
    if (nl == 0 || n == 0) return;
    const int h = (int)(n / w), row0 = geom[(size_t)f * DEPTH_GEOM + 3], col0 = geom[(size_t)f * DEPTH_GEOM + 4];
    const int ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2], l = tri_link[t];
    if (l < 0 || l >= nl || ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return;
    const double *R = rt + RN_HEAD + RN_LINK * l;
    const RenderVertex a = render_vertex(verts + 3 * (size_t)ia, R, rt), b = render_vertex(verts + 3 * (size_t)ib, R, rt),
                       c = render_vertex(verts + 3 * (size_t)ic, R, rt);
    if (!(a.ok && b.ok && c.ok)) return;                                // no clipping: the triangle is dropped whole
    const long area2 = render_edge(a.X, a.Y, b.X, b.Y, c.X, c.Y);
    if (area2 == 0) return;
    // the sample points (256 (row0 + i), 256 (col0 + j)) inside the bounding box, clipped to the crop
    const long minX = lmin(a.X, lmin(b.X, c.X)), maxX = lmax(a.X, lmax(b.X, c.X)), minY = lmin(a.Y, lmin(b.Y, c.Y)), maxY = lmax(a.Y, lmax(b.Y, c.Y));
    const long c_lo = lmax(ceil_div256(minX), (long)col0), c_hi = lmin(floor_div256(maxX), (long)col0 + w - 1);
    const long r_lo = lmax(ceil_div256(minY), (long)row0), r_hi = lmin(floor_div256(maxY), (long)row0 + h - 1);
    if (c_lo > c_hi || r_lo > r_hi) return;
    const unsigned ncols = (unsigned)(c_hi - c_lo + 1), count = (unsigned)(r_hi - r_lo + 1) * ncols;     // <= h * w < 2^30
    const double darea = (double)area2;
    for (unsigned k = lane; k < count; k += 64) {
        const unsigned dr = k / ncols, dc = k - dr * ncols;
        const long r = r_lo + dr, cc = c_lo + dc, px = 256 * cc, py = 256 * r;
        // every factor is below 2^26 inside the bounding box: the edge values are exact in int64 and in float64
        const long ea = render_edge(b.X, b.Y, c.X, c.Y, px, py), eb = render_edge(c.X, c.Y, a.X, a.Y, px, py),
                   ec = render_edge(a.X, a.Y, b.X, b.Y, px, py);
        const bool in = area2 > 0 ? (ea >= 0 && eb >= 0 && ec >= 0) : (ea <= 0 && eb <= 0 && ec <= 0);
        if (!in) continue;
        const double la = (double)ea / darea, lb = (double)eb / darea, lc = (double)ec / darea;
        const double invz = (la * a.iz + lb * b.iz) + lc * c.iz;
        const float d = (float)(1.0 / invz);
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)t;
        // (r - row0, cc - col0) is a pixel of the crop, and the crop lies inside [0, pixel_capacity)
        atomicMin(zbuf + (start + (r - row0) * w + (cc - col0)), key);
    }
}

__global__ __launch_bounds__(DEPTH_THREADS) void render_raster_kernel(const float *__restrict__ verts, const int *__restrict__ tris,
                                                                      const int *__restrict__ tri_link, int V, int T,
                                                                      long pixel_capacity, const int *__restrict__ geom,
                                                                      const double *__restrict__ render,
                                                                      unsigned long long *__restrict__ zbuf) {
    const int f = blockIdx.y;
    const int t = (int)(blockIdx.x * DEPTH_WAVES + (threadIdx.x >> 6));                  // uniform over the wave
    if (t >= T) return;
    render_raster_wave(verts, tris, tri_link, V, t, f, pixel_capacity, geom, render + (size_t)f * RN_WIDTH, zbuf);
}

// the library's: the wave for LOCAL triangle j of frame f handles global triangle tri_off[i] + j of the frame's instance i.  f is
// blockIdx.y, so the instance, its range and the early exit are uniform over the wave (and the block)
__global__ __launch_bounds__(DEPTH_THREADS) void render_raster_lib_kernel(const float *__restrict__ verts, const int *__restrict__ tris,
                                                                          const int *__restrict__ tri_link, int V, int T,
                                                                          const int *__restrict__ tri_off, int ninst, long pixel_capacity,
                                                                          const int *__restrict__ geom, const double *__restrict__ render,
                                                                          unsigned long long *__restrict__ zbuf) {
    const int f = blockIdx.y;
    const int j = (int)(blockIdx.x * DEPTH_WAVES + (threadIdx.x >> 6));                  // uniform over the wave
    const double *rt = render + (size_t)f * RN_WIDTH;
    int t_lo, t_hi;
    render_instance_range(rt, tri_off, ninst, T, t_lo, t_hi);
    if (j >= t_hi - t_lo) return;                                       // 0 <= t_lo <= t_hi <= T: t_lo + j stays inside [0, T)
    render_raster_wave(verts, tris, tri_link, V, t_lo + j, f, pixel_capacity, geom, rt, zbuf);
}

__device__ __forceinline__ unsigned short render_quantise(double v, unsigned short) {    // uint16: rint, kept in 1..65535
    const double q = rint(v);
    return q >= 1.0 && q <= 65535.0 ? (unsigned short)q : (unsigned short)0;
}
__device__ __forceinline__ float render_quantise(double v, float) {                      // float32: kept when finite and positive
    const float q = (float)v;
    return q > 0.f && q < __builtin_inff() ? q : 0.f;
}

template <typename T>
__global__ __launch_bounds__(DEPTH_THREADS) void render_resolve_kernel(long pixel_capacity, const int *__restrict__ geom,
                                                                       const double *__restrict__ render, int chunks,
                                                                       const int *__restrict__ tri_link, int ntri,
                                                                       const unsigned long long *__restrict__ zbuf, T *__restrict__ depth,
                                                                       unsigned char *__restrict__ labels) {
    const int f = blockIdx.y;
    long start, lo, hi;
    int w;
    const long n = depth_crop(geom, f, pixel_capacity, start, w);
    depth_chunk(start, n, blockIdx.x, chunks, lo, hi);
    const double scale = render[(size_t)f * RN_WIDTH + 6];
    for (long a = lo + threadIdx.x; a < hi; a += DEPTH_THREADS) {       // [lo, hi) lies inside [0, pixel_capacity)
        const unsigned long long key = zbuf[a];
        T d = T(0);
        unsigned char lab = 255;
        const unsigned t = (unsigned)key;
        if (key != RN_EMPTY && t < (unsigned)ntri) {
            const double df = (double)__uint_as_float((unsigned)(key >> 32));
            d = render_quantise(df / scale, T(0));
            const int l = tri_link[t];
            if (d != T(0)) lab = (unsigned char)l;
        }
        depth[a] = d;
        labels[a] = lab;
    }
}

// tri_off == nullptr: one object, every frame draws all ntri triangles; otherwise a library of ninst instances whose largest holds tmax
template <typename T>
static void render_launch(int nframes, const float *verts, const int *tris, const int *tri_link, int V, int ntri, const int *tri_off,
                          int ninst, int tmax, const int *geom, const double *render, void *depth, unsigned char *labels,
                          unsigned long long *zbuf, long pixel_capacity, hipStream_t st) {
    const long chunks = depth_chunks(pixel_capacity, nframes);          // depth.hip's grid
    const dim3 grid((unsigned)chunks, nframes);
    hipLaunchKernelGGL(render_clear_kernel, grid, dim3(DEPTH_THREADS), 0, st, pixel_capacity, geom, (int)chunks, zbuf);
    if (tri_off) {
        if (tmax > 0)
            hipLaunchKernelGGL(render_raster_lib_kernel, dim3((unsigned)((tmax + DEPTH_WAVES - 1) / DEPTH_WAVES), nframes), dim3(DEPTH_THREADS),
                               0, st, verts, tris, tri_link, V, ntri, tri_off, ninst, pixel_capacity, geom, render, zbuf);
    } else if (ntri > 0)
        hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)((ntri + DEPTH_WAVES - 1) / DEPTH_WAVES), nframes), dim3(DEPTH_THREADS), 0, st,
                           verts, tris, tri_link, V, ntri, pixel_capacity, geom, render, zbuf);
    hipLaunchKernelGGL(render_resolve_kernel<T>, grid, dim3(DEPTH_THREADS), 0, st, pixel_capacity, geom, render, (int)chunks, tri_link, ntri,
                       zbuf, (T *)depth, labels);
}

// ---- crops centred on the projected object (ancsh_render_centre_crops) ---------------------------------------------------------------------
// Block f owns frame f: its threads stride over the triangles, every referenced vertex goes through render_vertex -- the raster kernel's own
// transform --, a wave reduces the four bounds of its counted vertices with shuffles and takes ONE integer atomic per bound on the frame's
// scratch row; the block's first thread then turns the row into the crop's origin.  Minimum and maximum do not depend on the order of
// their operands: the origin is a pure function of the input.
constexpr int RN_CENTRE = ANCSH_CROP_CENTRE;
constexpr int RN_INT_MAX = 2147483647, RN_INT_MIN = -2147483647 - 1;

// the block centres frame f's crop on the vertices of the triangles [t_lo, t_hi) (uniform over the block): both centring kernels' body.
// library == false: one object, the range is [0, T); true: the range of the frame's instance, read once the frame is known to be centred
template <bool library>
__device__ __forceinline__ void render_centre_block(const float *__restrict__ verts, const int *__restrict__ tris,
                                                    const int *__restrict__ tri_link, int V, int T, const int *__restrict__ tri_off, int ninst,
                                                    const double *__restrict__ render, int *__restrict__ geom, int *__restrict__ bounds) {
    const int f = blockIdx.x;
    int *g = geom + (size_t)f * DEPTH_GEOM, *b = bounds + (size_t)f * 4;
    if (threadIdx.x < 4) atomicExch(b + threadIdx.x, (threadIdx.x & 1) ? RN_INT_MIN : RN_INT_MAX);      // {Xmin Xmax Ymin Ymax}: the empty bounds
    if (!(g[3] == RN_CENTRE && g[4] == RN_CENTRE)) return;              // uniform over the block: a frame with a real origin is left alone
    __threadfence();
    __syncthreads();
    const double *rt = render + (size_t)f * RN_WIDTH;
    const int nl = render_nlinks(rt);
    int t_lo = 0, t_hi = T;
    if (library) render_instance_range(rt, tri_off, ninst, T, t_lo, t_hi);
    int xmin = RN_INT_MAX, xmax = RN_INT_MIN, ymin = RN_INT_MAX, ymax = RN_INT_MIN;
    for (int t = t_lo + (int)threadIdx.x; t < t_hi && nl > 0; t += DEPTH_THREADS) {     // t_hi <= T < 2^24: the sum cannot wrap
        const int l = tri_link[t];
        if (l < 0 || l >= nl) continue;
        const double *R = rt + RN_HEAD + RN_LINK * l;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = tris[3 * (size_t)t + k];
            if (i < 0 || i >= V) continue;                              // vertices count one by one, not per dropped triangle
            const RenderVertex a = render_vertex(verts + 3 * (size_t)i, R, rt);
            if (!a.ok) continue;
            const int X = (int)a.X, Y = (int)a.Y;                       // |X|, |Y| < 2^25
            xmin = X < xmin ? X : xmin;
            xmax = X > xmax ? X : xmax;
            ymin = Y < ymin ? Y : ymin;
            ymax = Y > ymax ? Y : ymax;
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const int x0 = __shfl_xor(xmin, o), x1 = __shfl_xor(xmax, o), y0 = __shfl_xor(ymin, o), y1 = __shfl_xor(ymax, o);
        xmin = x0 < xmin ? x0 : xmin;
        xmax = x1 > xmax ? x1 : xmax;
        ymin = y0 < ymin ? y0 : ymin;
        ymax = y1 > ymax ? y1 : ymax;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(b + 0, xmin);
        atomicMax(b + 1, xmax);
        atomicMin(b + 2, ymin);
        atomicMax(b + 3, ymax);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const int x0 = atomicAdd(b + 0, 0), x1 = atomicAdd(b + 1, 0), y0 = atomicAdd(b + 2, 0), y1 = atomicAdd(b + 3, 0);
        int row0 = 0, col0 = 0;
        if (x0 <= x1) {                                                 // a vertex counted; |sum| < 2^26, the shift is arithmetic: floor
            col0 = ((x0 + x1) >> 9) - (g[2] >> 1);
            row0 = ((y0 + y1) >> 9) - (g[1] >> 1);
        }
        g[3] = row0;
        g[4] = col0;
    }
}

__global__ __launch_bounds__(DEPTH_THREADS) void render_centre_kernel(const float *__restrict__ verts, const int *__restrict__ tris,
                                                                      const int *__restrict__ tri_link, int V, int T,
                                                                      const double *__restrict__ render, int *__restrict__ geom,
                                                                      int *__restrict__ bounds) {
    render_centre_block<false>(verts, tris, tri_link, V, T, nullptr, 0, render, geom, bounds);
}

__global__ __launch_bounds__(DEPTH_THREADS) void render_centre_lib_kernel(const float *__restrict__ verts, const int *__restrict__ tris,
                                                                          const int *__restrict__ tri_link, int V, int T,
                                                                          const int *__restrict__ tri_off, int ninst,
                                                                          const double *__restrict__ render, int *__restrict__ geom,
                                                                          int *__restrict__ bounds) {
    render_centre_block<true>(verts, tris, tri_link, V, T, tri_off, ninst, render, geom, bounds);
}

}  // namespace ancsh

using namespace ancsh;

// what both centring entries check, under the entry's name
static int render_centre_check(const char *name, int nframes, const float *verts, const int *tris, const int *tri_link, int V, int T,
                               const double *render, const int *geom, const int *bounds) {
    ANCSH_REQUIRE(nframes >= 0, "%s: bad shape nframes=%d", name, nframes);
    ANCSH_REQUIRE(nframes <= 65535, "%s: %d frames exceed the 65535-frame grid range; split the batch", name, nframes);
    ANCSH_REQUIRE(T >= 0 && T < (1 << 24), "%s: T=%d triangles must be in [0, 2^24)", name, T);
    ANCSH_REQUIRE(V >= 0 && V < (1 << 24), "%s: V=%d vertices must be in [0, 2^24)", name, V);
    ANCSH_REQUIRE(verts && tris && tri_link && render && geom && bounds, "%s: null pointer", name);
    ANCSH_REQUIRE(((size_t)render & 7) == 0 && ((size_t)geom & 3) == 0 && ((size_t)bounds & 3) == 0,
                  "%s: render must be 8-byte aligned, geom and bounds 4-byte aligned", name);
    return ANCSH_OK;
}

// what both library entries check of the library itself
static int render_library_check(const char *name, const int *tri_off, int ninst) {
    ANCSH_REQUIRE(ninst >= 1 && ninst <= ANCSH_LIBRARY_MAX_INSTANCES, "%s: ninst=%d instances must be in [1, %d]", name, ninst,
                  ANCSH_LIBRARY_MAX_INSTANCES);
    ANCSH_REQUIRE(tri_off && ((size_t)tri_off & 3) == 0, "%s: tri_off must be a 4-byte aligned device pointer", name);
    return ANCSH_OK;
}

extern "C" int ancsh_render_centre_crops(int nframes, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                         const double *render, int *geom, int *bounds, void *stream) {
    if (const int rc = render_centre_check("render_centre_crops", nframes, verts, tris, tri_link, V, T, render, geom, bounds)) return rc;
    if (nframes == 0) return ANCSH_OK;
    hipLaunchKernelGGL(render_centre_kernel, dim3(nframes), dim3(DEPTH_THREADS), 0, (hipStream_t)stream, verts, tris, tri_link, V, T, render,
                       geom, bounds);
    return check_launch("render_centre_crops");
}

extern "C" int ancsh_render_centre_crops_lib(int nframes, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                             const int *tri_off, int ninst, const double *render, int *geom, int *bounds, void *stream) {
    if (const int rc = render_centre_check("render_centre_crops_lib", nframes, verts, tris, tri_link, V, T, render, geom, bounds)) return rc;
    if (const int rc = render_library_check("render_centre_crops_lib", tri_off, ninst)) return rc;
    if (nframes == 0) return ANCSH_OK;
    hipLaunchKernelGGL(render_centre_lib_kernel, dim3(nframes), dim3(DEPTH_THREADS), 0, (hipStream_t)stream, verts, tris, tri_link, V, T,
                       tri_off, ninst, render, geom, bounds);
    return check_launch("render_centre_crops_lib");
}

// what both rendering entries check, under the entry's name
static int render_depth_check(const char *name, int nframes, int depth_type, const float *verts, const int *tris, const int *tri_link, int V,
                              int T, const int *geom, const double *render, const void *depth, const unsigned char *labels,
                              const unsigned long long *zbuf, long pixel_capacity) {
    ANCSH_REQUIRE(nframes >= 0, "%s: bad shape nframes=%d", name, nframes);
    ANCSH_REQUIRE(nframes <= 65535, "%s: %d frames exceed the 65535-frame grid range; split the batch", name, nframes);
    ANCSH_REQUIRE(depth_type == ANCSH_DEPTH_U16 || depth_type == ANCSH_DEPTH_F32,
                  "%s: depth_type=%d must be ANCSH_DEPTH_U16 (0) or ANCSH_DEPTH_F32 (1)", name, depth_type);
    ANCSH_REQUIRE(pixel_capacity >= 0 && pixel_capacity < (1L << 30), "%s: pixel_capacity=%ld pixels out of range", name, pixel_capacity);
    ANCSH_REQUIRE(T >= 0 && T < (1 << 24), "%s: T=%d triangles must be in [0, 2^24)", name, T);
    ANCSH_REQUIRE(V >= 0 && V < (1 << 24), "%s: V=%d vertices must be in [0, 2^24)", name, V);
    ANCSH_REQUIRE(verts && tris && tri_link && geom && render && depth && labels && zbuf, "%s: null pointer", name);
    ANCSH_REQUIRE(((size_t)depth & 15) == 0 && ((size_t)labels & 7) == 0 && ((size_t)render & 7) == 0 && ((size_t)zbuf & 7) == 0,
                  "%s: depth must be 16-byte aligned, labels, render and zbuf 8-byte aligned (the crops inside them may start anywhere)", name);
    return ANCSH_OK;
}

extern "C" int ancsh_render_depth_labels(int nframes, int depth_type, const float *verts, const int *tris, const int *tri_link, int V, int T,
                                         const int *geom, const double *render, void *depth, unsigned char *labels,
                                         unsigned long long *zbuf, long pixel_capacity, void *stream) {
    if (const int rc = render_depth_check("render_depth_labels", nframes, depth_type, verts, tris, tri_link, V, T, geom, render, depth, labels,
                                          zbuf, pixel_capacity))
        return rc;
    if (nframes == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        render_launch<unsigned short>(nframes, verts, tris, tri_link, V, T, nullptr, 0, 0, geom, render, depth, labels, zbuf, pixel_capacity,
                                      (hipStream_t)stream);
    else
        render_launch<float>(nframes, verts, tris, tri_link, V, T, nullptr, 0, 0, geom, render, depth, labels, zbuf, pixel_capacity,
                             (hipStream_t)stream);
    return check_launch("render_depth_labels");
}

extern "C" int ancsh_render_depth_labels_lib(int nframes, int depth_type, const float *verts, const int *tris, const int *tri_link, int V,
                                             int T, const int *tri_off, int ninst, int Tmax, const int *geom, const double *render,
                                             void *depth, unsigned char *labels, unsigned long long *zbuf, long pixel_capacity,
                                             void *stream) {
    if (const int rc = render_depth_check("render_depth_labels_lib", nframes, depth_type, verts, tris, tri_link, V, T, geom, render, depth,
                                          labels, zbuf, pixel_capacity))
        return rc;
    if (const int rc = render_library_check("render_depth_labels_lib", tri_off, ninst)) return rc;
    ANCSH_REQUIRE(Tmax >= 0 && Tmax <= T, "render_depth_labels_lib: Tmax=%d, the largest instance's triangle count, must be in [0, T=%d]", Tmax, T);
    if (nframes == 0) return ANCSH_OK;
    if (depth_type == ANCSH_DEPTH_U16)
        render_launch<unsigned short>(nframes, verts, tris, tri_link, V, T, tri_off, ninst, Tmax, geom, render, depth, labels, zbuf,
                                      pixel_capacity, (hipStream_t)stream);
    else
        render_launch<float>(nframes, verts, tris, tri_link, V, T, tri_off, ninst, Tmax, geom, render, depth, labels, zbuf, pixel_capacity,
                             (hipStream_t)stream);
    return check_launch("render_depth_labels_lib");
}
