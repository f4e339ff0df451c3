// point_gt_build.hip -- the per-point ground truth of annotated clouds, built on the GPU in front of the streaming sampler (gfx950).
//
// Reference: lib/dataset.py:434-700 (create_data_shape2motion / create_data_mobility, after the two h5py lookups) and :371-379 (the sapien
// rotation): per part on the host, numpy float64 -- the part NOCS and NAOCS maps, each point's offset to every joint line of its part
// (lib/d3_utils.py:192-203), the thresholded heat-map, unit vector, joint direction and joint label, then .astype(np.float32).  Here one
// launch turns a ragged batch of 7-column rows [x y z | c (3) | part] and a per-cloud rig table (include/ancsh_hip.h has its layout) into
// the 18-column rows dataset.pack_cloud packs, where the sampler, the pose fit and ancsh_point_gt_rec read them.
// HBM-bound: 28 B read and 72 B written per row.  A workgroup takes tiles of 256 rows of one cloud; the cloud's rig sits in LDS (rows of a
// part are neighbours, so a wave's rig reads are broadcasts), a tile's rows go through LDS both ways so that global memory sees 16-byte
// accesses of consecutive lanes: a wave's 64 output rows are 4608 contiguous bytes, not 18 strided dwords per lane.  float64 arithmetic
// evaluated as the reference writes it (no contraction: the library is built with -ffp-contract=off), one rounding to float32 per output.
#include "common.h"

namespace ancsh {

constexpr int PGB_ROWS = 256;                              // rows of a tile = threads of a workgroup
constexpr int PGB_IN = 7, PGB_OUT = 18;
constexpr int PGB_RIG_MAX = ANCSH_RIG_WIDTH(8);

// n floats between global memory g (4-byte aligned) and LDS s, whose element i lies at s[mis + i] with mis = the position of g inside
// its 16-byte line: the body moves as aligned float4 on both sides, at most 3 floats in front and 3 behind as dwords.
template <bool TO_GLOBAL>
__device__ __forceinline__ void tile_copy(float *__restrict__ g, float *__restrict__ s, int n, int mis, int tid) {
    int head = (4 - mis) & 3;
    if (head > n) head = n;
    if (tid < head) {
        if (TO_GLOBAL) g[tid] = s[mis + tid];
        else s[mis + tid] = g[tid];
    }
    const int nvec = (n - head) >> 2;
    for (int v = tid; v < nvec; v += PGB_ROWS) {
        const int i = head + 4 * v;                        // (mis + i) % 4 == 0 whenever a body exists
        if (TO_GLOBAL) *reinterpret_cast<float4 *>(g + i) = *reinterpret_cast<const float4 *>(s + mis + i);
        else *reinterpret_cast<float4 *>(s + mis + i) = *reinterpret_cast<const float4 *>(g + i);
    }
    const int t = head + 4 * nvec + tid;
    if (t < n) {
        if (TO_GLOBAL) g[t] = s[mis + t];
        else s[mis + t] = g[t];
    }
}

__global__ __launch_bounds__(PGB_ROWS) void point_gt_build_kernel(int K, const float *__restrict__ src, long capacity,
                                                                  const int *__restrict__ offsets, const double *__restrict__ rig,
                                                                  int rig_ld, float *__restrict__ rows) {
    __shared__ double s_rig[PGB_RIG_MAX];
    __shared__ __attribute__((aligned(16))) float s_row[PGB_ROWS * PGB_OUT + 4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long r0 = offsets[b], r1 = offsets[b + 1];
    if (r0 < 0 || r1 <= r0 || r1 > capacity) return;      // empty or outside the buffers (the host refuses both): nothing is written
    const long tiles = (r1 - r0 + PGB_ROWS - 1) / PGB_ROWS;
    if ((long)blockIdx.x >= tiles) return;
    for (int i = tid; i < rig_ld; i += PGB_ROWS) s_rig[i] = rig[(size_t)b * rig_ld + i];
    const int part_w = ANCSH_RIG_PART(K);
    const float qnan = __int_as_float(0x7fc00000);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long first = r0 + tile * PGB_ROWS;
        const int cnt = (int)(r1 - first < PGB_ROWS ? r1 - first : PGB_ROWS);
        const float *gin = src + (size_t)first * PGB_IN;
        float *gout = rows + (size_t)first * PGB_OUT;
        const int mis_in = (int)(((size_t)gin >> 2) & 3), mis_out = (int)(((size_t)gout >> 2) & 3);
        __syncthreads();                                   // the rig is in LDS; the previous tile has left s_row
        tile_copy<false>(const_cast<float *>(gin), s_row, cnt * PGB_IN, mis_in, tid);
        __syncthreads();
        float in[PGB_IN];
        bool leads = false;                                // the first row of its part: the cloud's first row, or another part in front of it
        if (tid < cnt) {
#pragma unroll
            for (int q = 0; q < PGB_IN; ++q) in[q] = s_row[mis_in + tid * PGB_IN + q];
            if (tid > 0) leads = s_row[mis_in + (tid - 1) * PGB_IN + 6] != in[6];
            else leads = first == r0 || gin[-1] != in[6];  // the last value of row first - 1 >= r0
        }
        __syncthreads();
        if (tid < cnt) {
            float o[PGB_OUT];
            o[0] = in[0]; o[1] = in[1]; o[2] = in[2];
            const float part = in[6];
            if (part >= 0.f && part < (float)K && part == floorf(part)) {
                const double *G = s_rig + ANCSH_RIG_GMAP, *pt = s_rig + ANCSH_RIG_HEAD + (int)part * part_w;
                const double thres = s_rig[0];
                const bool le = s_rig[2] != 0.0, rot = s_rig[3] != 0.0;
                double g0[3], p0[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double cc = (double)in[3 + a] - pt[a];
                    g0[a] = ((cc - G[a]) * G[3 + a] + 0.5) - G[6 + a];
                    p0[a] = ((cc - pt[3 + a]) * pt[6 + a] + 0.5) - pt[9 + a];
                }
                double heat = 0.0, u[3] = {0.0, 0.0, 0.0}, ori[3] = {0.0, 0.0, 0.0}, jc = s_rig[1];
                int nj = (int)pt[14];
                nj = nj < 0 ? 0 : (nj > K ? K : nj);
                for (int k = 0; k < nj; ++k) {             // in order: a later entry overwrites an earlier one
                    const double *e = pt + 15 + ANCSH_RIG_ENTRY * k;
                    double off[3];
                    const bool constant = e[7] == 1.0, origin = e[7] == 2.0;
                    if (constant) {                        // sapien prismatic
                        off[0] = off[1] = off[2] = 0.5 * thres;
                    } else {                               // the offset to the line (P0, l): the point's, or (sapien revolute) the origin's
                        const double d0 = (origin ? 0.0 : g0[0]) - e[0], d1 = (origin ? 0.0 : g0[1]) - e[1], d2 = (origin ? 0.0 : g0[2]) - e[2];
                        const double dot = (d0 * e[3] + d1 * e[4]) + d2 * e[5];
                        off[0] = dot * e[3] / e[8] - d0;
                        off[1] = dot * e[4] / e[8] - d1;
                        off[2] = dot * e[5] / e[8] - d2;
                    }
                    const double h = sqrt((off[0] * off[0] + off[1] * off[1]) + off[2] * off[2]);
                    // a NaN h selects nothing; an origin entry reaches the part's first row only
                    const bool sel = constant ? h > 0.0 : ((le ? h <= thres : h < thres) && (!origin || leads));
                    if (sel) {
                        const double den = h + 1e-7;
                        heat = 1.0 - h / thres;
                        u[0] = off[0] / den; u[1] = off[1] / den; u[2] = off[2] / den;
                        ori[0] = e[3]; ori[1] = e[4]; ori[2] = e[5];
                        jc = e[6];
                    }
                }
                if (rot) {                                 // the sapien base-joint rotation: v R^T about the cube's centre / the origin
                    const double *R = s_rig + ANCSH_RIG_ROT;
                    double t[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) t[a] = (R[3 * a] * (p0[0] - 0.5) + R[3 * a + 1] * (p0[1] - 0.5)) + R[3 * a + 2] * (p0[2] - 0.5) + 0.5;
                    p0[0] = t[0]; p0[1] = t[1]; p0[2] = t[2];
#pragma unroll
                    for (int a = 0; a < 3; ++a) t[a] = (R[3 * a] * (g0[0] - 0.5) + R[3 * a + 1] * (g0[1] - 0.5)) + R[3 * a + 2] * (g0[2] - 0.5) + 0.5;
                    g0[0] = t[0]; g0[1] = t[1]; g0[2] = t[2];
#pragma unroll
                    for (int a = 0; a < 3; ++a) t[a] = (R[3 * a] * u[0] + R[3 * a + 1] * u[1]) + R[3 * a + 2] * u[2];
                    u[0] = t[0]; u[1] = t[1]; u[2] = t[2];
#pragma unroll
                    for (int a = 0; a < 3; ++a) t[a] = (R[3 * a] * ori[0] + R[3 * a + 1] * ori[1]) + R[3 * a + 2] * ori[2];
                    ori[0] = t[0]; ori[1] = t[1]; ori[2] = t[2];
                }
                o[3] = (float)pt[12];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    o[4 + a] = (float)p0[a];
                    o[7 + a] = (float)g0[a];
                    o[11 + a] = (float)u[a];
                    o[14 + a] = (float)ori[a];
                }
                o[10] = (float)heat;
                o[17] = (float)(pt[13] >= 0.0 ? pt[13] : jc);
            } else {                                       // not a part of this rig: the rig is never indexed
                o[3] = o[17] = -1.f;
#pragma unroll
                for (int q = 4; q < 17; ++q) o[q] = qnan;
            }
#pragma unroll
            for (int q = 0; q < PGB_OUT; ++q) s_row[mis_out + tid * PGB_OUT + q] = o[q];
        }
        __syncthreads();
        tile_copy<true>(gout, s_row, cnt * PGB_OUT, mis_out, tid);
    }
}

}  // namespace ancsh

using namespace ancsh;

extern "C" int ancsh_point_gt_build(int nclouds, int K, const float *src, long capacity, const int *offsets, const double *rig, int rig_ld,
                                    float *rows, void *stream) {
    ANCSH_REQUIRE(nclouds >= 0 && nclouds <= 65535, "point_gt_build: nclouds=%d must be in [0, 65535] (the grid's range; split the batch)",
                  nclouds);
    ANCSH_REQUIRE(K >= 1 && K <= 8, "point_gt_build: K=%d must be in [1, 8]", K);
    ANCSH_REQUIRE(rig_ld == ANCSH_RIG_WIDTH(K), "point_gt_build: rig_ld=%d, a rig of K=%d parts is %d wide", rig_ld, K, ANCSH_RIG_WIDTH(K));
    ANCSH_REQUIRE(capacity >= 0 && capacity < (1L << 30), "point_gt_build: capacity=%ld rows out of range", capacity);
    if (nclouds == 0) return ANCSH_OK;
    ANCSH_REQUIRE(src && offsets && rig && rows, "point_gt_build: null pointer");
    if (capacity == 0) return ANCSH_OK;
    // x: tiles of the largest cloud the buffers admit, capped as ancsh_raw_point_labels caps its grid (a larger cloud loops over its
    // tiles); fixed by (capacity, nclouds), so one captured graph serves every batch
    long gx = (capacity + PGB_ROWS - 1) / PGB_ROWS;
    const long cap = (4096 + nclouds - 1) / nclouds;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(point_gt_build_kernel, dim3((unsigned)gx, nclouds), dim3(PGB_ROWS), 0, (hipStream_t)stream, K, src, capacity, offsets,
                       rig, rig_ld, rows);
    return check_launch("point_gt_build");
}
