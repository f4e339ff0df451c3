// depth_annotate_common.h -- what the annotation (depth_annotate.hip: link labels -> annotated rows) and its inverse (depth_annotated_images.hip:
// rows -> images) share: the scene table's integers, the rows of a cloud and the validity of a labelled pixel.
#pragma once
#include "depth_common.h"

namespace ancsh {

constexpr int AN_LINKS = ANCSH_SCENE_MAX_LINKS, AN_HEAD = ANCSH_SCENE_HEAD, AN_LINK = ANCSH_SCENE_LINK, AN_SCENE = ANCSH_SCENE_WIDTH;

// the scene's integers, read defensively (the host refuses what these clamp): a table that is not one keeps the kernels inside their buffers
__device__ __forceinline__ int scene_nlinks(const double *__restrict__ sc) {
    const double v = sc[14];
    return v >= 1.0 && v <= (double)AN_LINKS ? (int)v : 0;
}
__device__ __forceinline__ int scene_rank(const double *__restrict__ sc, int l, int nl) {       // -1: not a used link
    if (l >= nl) return -1;
    const double v = sc[AN_HEAD + AN_LINK * l];
    return v >= 0.0 && v < (double)AN_LINKS ? (int)v : -1;
}

// the rows of a cloud with the per-link totals tot[]: their sum over the used links, or 0 when one of them is below the minimum
__device__ __forceinline__ long scene_cloud_rows(const double *__restrict__ sc, const int (&tot)[AN_LINKS]) {
    const int nl = scene_nlinks(sc);
    const double min_px = sc[13];
    long total = 0;
    bool ok = true;
#pragma unroll
    for (int l = 0; l < AN_LINKS; ++l)
        if (scene_rank(sc, l, nl) >= 0) {
            if ((double)tot[l] < min_px) ok = false;
            total += tot[l];
        }
    return ok ? total : 0;
}

// the V = 16 / sizeof(T) pixels [a0, a0 + V) of the buffer (a0 a multiple of V) -> d[] and lab[]: the link of a valid pixel of [lo, hi) --
// its label names a used link (s_rank: 16 ranks, -1 = not used) and its depth passes depth_ok --, -1 otherwise.  A group that reaches past
// the buffer's end is read pixel by pixel.
template <typename T>
__device__ __forceinline__ void annotate_group(const T *__restrict__ depth, const unsigned char *__restrict__ labels, long a0, long lo, long hi,
                                               long pixel_capacity, const int *s_rank, T (&d)[16 / sizeof(T)], int (&lab)[16 / sizeof(T)]) {
    constexpr int V = 16 / sizeof(T);
    union { uint4 q; T e[V]; } u;
    union { uint2 q; unsigned char e[8]; } m;
    if (a0 + V <= pixel_capacity) {
        u.q = *reinterpret_cast<const uint4 *>(depth + a0);
        if (V == 8) m.q = *reinterpret_cast<const uint2 *>(labels + a0);
        else m.q = make_uint2(*reinterpret_cast<const unsigned *>(labels + a0), 0u);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool in = a0 + k < pixel_capacity;
            u.e[k] = in ? depth[a0 + k] : T(0);
            m.e[k] = in ? labels[a0 + k] : (unsigned char)255;
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        d[k] = u.e[k];
        const long a = a0 + k;
        const int l = m.e[k];
        lab[k] = a >= lo && a < hi && l < AN_LINKS && s_rank[l] >= 0 && depth_ok(u.e[k]) ? l : -1;
    }
}

}  // namespace ancsh
