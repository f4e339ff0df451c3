// iou_grid.h -- the inside-box test of iou_3d (lib/d3_utils.py:39-53), shared by iou_3d_kernel (metrics.hip) and gt_error_kernel
// (gt_errors.hip).  The definitions are the ones metrics.hip held, moved here word for word and included where they stood, so
// iou_3d_kernel compiles to the instruction stream it had.  float64 like the reference: the projections up.u are sums of three products
// in (x, y, z) order, the bounds np.dot(u, u).
#pragma once
#include "common.h"

namespace ancsh {

struct BoxFrame {
    double o[3], u1[3], u2[3], u3[3], d1, d2, d3;
};

__device__ __forceinline__ void box_frame(const double *bb, BoxFrame &f) {      // bb: 8 x 3 corners, reference's order
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f.o[c] = bb[4 * 3 + c];
        f.u1[c] = bb[5 * 3 + c] - bb[4 * 3 + c];
        f.u2[c] = bb[7 * 3 + c] - bb[4 * 3 + c];
        f.u3[c] = bb[0 * 3 + c] - bb[4 * 3 + c];
    }
    f.d1 = f.u1[0] * f.u1[0] + f.u1[1] * f.u1[1] + f.u1[2] * f.u1[2];
    f.d2 = f.u2[0] * f.u2[0] + f.u2[1] * f.u2[1] + f.u2[2] * f.u2[2];
    f.d3 = f.u3[0] * f.u3[0] + f.u3[1] * f.u3[1] + f.u3[2] * f.u3[2];
}

__device__ __forceinline__ bool inside(const BoxFrame &f, double x, double y, double z) {
    const double ux = x - f.o[0], uy = y - f.o[1], uz = z - f.o[2];
    const double p1 = ux * f.u1[0] + uy * f.u1[1] + uz * f.u1[2];
    const double p2 = ux * f.u2[0] + uy * f.u2[1] + uz * f.u2[2];
    const double p3 = ux * f.u3[0] + uy * f.u3[1] + uz * f.u3[2];
    return (p1 > 0.0) & (p1 < f.d1) & (p2 > 0.0) & (p2 < f.d2) & (p3 > 0.0) & (p3 < f.d3);
}

}  // namespace ancsh
