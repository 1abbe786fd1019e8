// gsr_mlp.h -- what the deformation network's fused layers (gsr_deform.hip, gsr_resblock.hip, gsr_head.hip)
// share: MFMA accumulator types and layout, the persistent grid's size, and the host side of a launch.
#pragma once
#include <type_traits>

#include "gsr_common.h"

namespace gsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// row of accumulator register r of a 32 x 32 MFMA result (the column is lane & 31)
__device__ inline int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// persistent workgroups that walk P rows in tiles of `rows`: one per tile, at most max_blocks (> 0) or auto_cap
inline int persistent_blocks(int P, int rows, int max_blocks, int auto_cap) {
    const int tiles = div_up(P, rows), cap = max_blocks > 0 ? max_blocks : auto_cap;
    return tiles < cap ? tiles : cap;
}

// f(std::integral_constant<int, N>()) for the kernels templated on a tile count N = n in 1 .. 3, else 4
template <class F>
hipError_t dispatch_tiles(int n, F &&f) {
    switch (n) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 4>());
    }
}

// a launch with `lds` bytes of dynamic LDS, which may exceed the 64 KB a kernel gets without asking
template <class... P, class... A>
hipError_t launch_lds(void (*kernel)(P...), dim3 grid, int threads, size_t lds, hipStream_t s, const A &...args) {
    hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<grid, threads, lds, s>>>(args...);
    return hipGetLastError();
}

}  // namespace gsr
