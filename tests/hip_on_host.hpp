// HIP on host threads, for the emulation harnesses (jpeg_encode_emulated.cpp, jpeg_decode_emulated.cpp, png_decode_emulated.cpp):
// enough of the device language for kernels cut out of a .hip file, and for a device header included as it stands
// (csrc/png_inflate.hpp), to compile with the host compiler and run thread for thread -- one std::thread per GPU thread and a
// barrier for __syncthreads, workgroups one after another.  Include it before the kernels.
#pragma once
#include <algorithm>
#include <barrier>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>
struct d3 { unsigned x = 1, y = 1, z = 1; };
static thread_local d3 threadIdx, blockIdx, blockDim;
static std::barrier<> *g_bar;
#define __global__ static
#define __device__ static
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
static void __syncthreads() { g_bar->arrive_and_wait(); }
static uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static uint32_t atomicMin(uint32_t *p, uint32_t v)
{
    uint32_t o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
    return o;
}
static uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
using std::min; using std::max;
struct uint4 { uint32_t x, y, z, w; };
static uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return {a, b, c, d}; }
static unsigned uwip_cdiv(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }
// block-wide helpers of device_utils.hpp, restated with a shared array
static uint32_t g_vals[256];
static uint32_t block256_incl_scan_u32(uint32_t v, uint32_t *)
{
    __syncthreads(); g_vals[threadIdx.x] = v; __syncthreads();
    uint32_t s = 0; for (unsigned i = 0; i <= threadIdx.x; ++i) s += g_vals[i];
    __syncthreads(); return s;
}
static uint32_t block256_sum_u32(uint32_t v, uint32_t *)
{
    __syncthreads(); g_vals[threadIdx.x] = v; __syncthreads();
    uint32_t s = 0; for (unsigned i = 0; i < 256; ++i) s += g_vals[i];
    __syncthreads(); return s;
}
// the grid, workgroup by workgroup; sync: the kernel uses __syncthreads (or atomics), so its threads run at the same time --
// otherwise a plain loop over them
template <class F> static void launch(unsigned gx, unsigned gy, unsigned bs, bool sync, F f)
{
    for (unsigned by = 0; by < gy; ++by) for (unsigned bx = 0; bx < gx; ++bx) {
        if (!sync) {
            for (unsigned t = 0; t < bs; ++t) { threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by; blockDim.x = bs; f(); }
            continue;
        }
        std::barrier<> bar(bs); g_bar = &bar;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < bs; ++t) th.emplace_back([=, &bar] { g_bar = &bar; threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by; blockDim.x = bs; f(); });
        for (auto &t : th) t.join();
    }
}
