// pose_shared.h -- what pose.hip and pose_glue.hip share: the counter-based sample generator (the RANSAC fit and the 5-point Umeyama
// RANSAC draw point indices from it when the caller passes no `draws`) and the launch with dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>

namespace ancsh {
namespace pose {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ int device_draw(unsigned long long seed, int prob, int iter, int k, int n) {
    const unsigned long long h = splitmix64(seed ^ splitmix64(((unsigned long long)prob << 40) ^ ((unsigned long long)iter << 8) ^ (unsigned)k));
    return (int)(h % (unsigned long long)n);
}

// a launch with dynamic LDS: above 48 KB the kernel's limit is raised first
template <class Kernel, class... Args>
static void launch_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

}  // namespace pose
}  // namespace ancsh
