// pose_math_probe.hip -- TEST INFRASTRUCTURE ONLY: calls the closed-form device functions of the product header
// articulated-pose_amd/csrc/pose_math.h with chosen arguments, one thread per case, so that tests/test_pose_math_gpu.py can hold
// them to high-precision references (tests/golden/pose_math.npz).  Built by `make -C oracle probe` into
// oracle/_build/libancsh_pose_probe.so with the product's flags; nothing in the product package loads it and it adds nothing to the
// product library or its ABI.
//
// Every entry has the same shape:  int ancsh_probe_<name>(int n, const double *in, double *out)  with HOST arrays of n * NI and
// n * NO doubles.  It copies the cases to the device, runs one bounds-checked grid-stride kernel that reads case i from
// in[i * NI ..] and writes out[i * NO ..], and copies the results back.  Returns 0 or the hipError_t that stopped it.
#include <hip/hip_runtime.h>

#include "../articulated-pose_amd/csrc/pose_math.h"

using namespace ancsh::pose;

namespace {

template <int NI, int NO, class F>
__global__ void probe_kernel(int n, const double *__restrict__ in, double *__restrict__ out, F f) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        double a[NI], o[NO];
        for (int k = 0; k < NI; ++k) a[k] = in[i * NI + k];
        f(a, o);
        for (int k = 0; k < NO; ++k) out[i * NO + k] = o[k];
    }
}

template <int NI, int NO, class F>
int run(int n, const double *in, double *out, F f) {
    if (n <= 0) return 0;
    double *din = nullptr, *dout = nullptr;
    const size_t bi = (size_t)n * NI * sizeof(double), bo = (size_t)n * NO * sizeof(double);
    hipError_t e = hipMalloc(&din, bi);
    if (e == hipSuccess) e = hipMalloc(&dout, bo);
    if (e == hipSuccess) e = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, bo);
    if (e == hipSuccess) {
        const int threads = 64, blocks = (n + threads - 1) / threads < 1024 ? (n + threads - 1) / threads : 1024;
        probe_kernel<NI, NO, F><<<blocks, threads>>>(n, din, dout, f);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);      // waits for the kernel
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    return (int)e;
}

struct HornJacobi { __device__ void operator()(const double *a, double *o) const { horn_quat(a, o); } };
struct HornFast { __device__ void operator()(const double *a, double *o) const { horn_quat_fast(a, o); } };
struct QuatToMat { __device__ void operator()(const double *a, double *o) const { quat_to_mat(a, o); } };
struct QuatToRotvec { __device__ void operator()(const double *a, double *o) const { quat_to_rotvec(a, o); } };
struct RotvecToMat { __device__ void operator()(const double *a, double *o) const { rotvec_to_mat(a, o); } };
struct Rodrigues {                      // in: rotation vector, point
    __device__ void operator()(const double *a, double *o) const {
        const Rod r = rod_prepare(a[0], a[1], a[2]);
        rod_apply(r, a[3], a[4], a[5], o[0], o[1], o[2]);
    }
};
struct SinCos { __device__ void operator()(const double *a, double *o) const { sincos_compact(a[0], o[0], o[1]); } };
struct Rcp { __device__ void operator()(const double *a, double *o) const { o[0] = fast_rcp(a[0]); } };
struct Rsqrt { __device__ void operator()(const double *a, double *o) const { o[0] = fast_rsqrt(a[0]); } };
struct CholSolve {                      // in: A (21, packed lower), par, b (6); out: x (6), ok
    __device__ void operator()(const double *a, double *o) const {
        double L[21];
        const bool ok = chol6(a, a[21], L);
        chol6_solve(L, a + 22, o);
        o[6] = ok ? 1.0 : 0.0;
    }
};
struct Lmpar {                          // in: A (21, packed lower), g (6), delta; out: par, z (6)
    __device__ void operator()(const double *a, double *o) const {
        double par = 0.0;
        lmpar6(a, a + 21, a[27], par, o + 1);
        o[0] = par;
    }
};

}  // namespace

extern "C" {
int ancsh_probe_horn_quat(int n, const double *in, double *out) { return run<9, 4>(n, in, out, HornJacobi()); }
int ancsh_probe_horn_quat_fast(int n, const double *in, double *out) { return run<9, 4>(n, in, out, HornFast()); }
int ancsh_probe_quat_to_mat(int n, const double *in, double *out) { return run<4, 9>(n, in, out, QuatToMat()); }
int ancsh_probe_quat_to_rotvec(int n, const double *in, double *out) { return run<4, 3>(n, in, out, QuatToRotvec()); }
int ancsh_probe_rotvec_to_mat(int n, const double *in, double *out) { return run<3, 9>(n, in, out, RotvecToMat()); }
int ancsh_probe_rodrigues(int n, const double *in, double *out) { return run<6, 3>(n, in, out, Rodrigues()); }
int ancsh_probe_sincos(int n, const double *in, double *out) { return run<1, 2>(n, in, out, SinCos()); }
int ancsh_probe_rcp(int n, const double *in, double *out) { return run<1, 1>(n, in, out, Rcp()); }
int ancsh_probe_rsqrt(int n, const double *in, double *out) { return run<1, 1>(n, in, out, Rsqrt()); }
int ancsh_probe_chol_solve(int n, const double *in, double *out) { return run<28, 7>(n, in, out, CholSolve()); }
int ancsh_probe_lmpar(int n, const double *in, double *out) { return run<28, 7>(n, in, out, Lmpar()); }
}
