// HIP on host threads, for the emulation harnesses (*_emulated.cpp): enough of the device language for kernels cut out of a
// .hip file, and for a device header included as it stands (csrc/png_inflate.hpp), to compile with the host compiler and run
// thread for thread -- one std::thread per GPU thread and a barrier for __syncthreads, workgroups one after another -- and the
// back end (HostThreads) on which a codec's own host sequence runs them.  Include it before the kernels.
#pragma once
#include <algorithm>
#include <barrier>
#include <cassert>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>
struct dim3 {
    unsigned x = 1, y = 1, z = 1;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
using d3 = dim3;
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
// the grid, workgroup by workgroup; sync: the kernel uses __syncthreads (or atomics), so its threads run at the same time: one
// host thread per GPU thread walks through all the workgroups, and a barrier between two of them keeps a fast thread out of
// the next workgroup's shared memory -- otherwise a plain loop over the threads
template <class F> static void launch(unsigned gx, unsigned gy, unsigned bs, bool sync, F f)
{
    if (!sync) {
        for (unsigned by = 0; by < gy; ++by) for (unsigned bx = 0; bx < gx; ++bx)
            for (unsigned t = 0; t < bs; ++t) { threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by; blockDim.x = bs; f(); }
        return;
    }
    std::barrier<> bar(bs); g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < bs; ++t)
        th.emplace_back([=, &bar] {
            threadIdx.x = t; blockDim.x = bs;
            for (unsigned by = 0; by < gy; ++by) for (unsigned bx = 0; bx < gx; ++bx) {
                blockIdx.x = bx; blockIdx.y = by;
                f();
                bar.arrive_and_wait();
            }
        });
    for (auto &t : th) t.join();
}

// The back end of the codecs' host sequences (csrc/uwip_internal.hpp has the device's, uwip_device) on host threads: the
// emulation harnesses hand it to the unit's own encode_sequence / decode_sequence, so the sanitizers check the array sizes,
// the grid sizes and the order of the launches that ship.
struct HostThreads {
    using dim3 = ::dim3;
    // every array is a heap block of its exact size, so that the address sanitizer sees an index one past any of them,
    // filled with garbage: what a kernel reads it must have been given
    std::map<std::string, std::vector<uint8_t>> arrays;
    // kernels (by the name of the launch) that neither meet at a barrier nor use atomics: their threads run as a plain loop
    std::set<std::string> barrier_free;
    // the harness's look at a launch before it runs: taps on the arrays so far, a cap on the grid
    std::function<void(const std::string &, dim3 &)> before_launch;
    template <class T> T *array(const char *name, size_t count)
    {
        std::vector<uint8_t> &v = arrays[name];
        v = std::vector<uint8_t>(count * sizeof(T), 0xDD);
        return reinterpret_cast<T *>(v.data());
    }
    template <class T> const T *get(const char *name) const
    {
        const auto it = arrays.find(name);
        return it == arrays.end() ? nullptr : reinterpret_cast<const T *>(it->second.data());
    }
    void fill(void *p, int value, size_t bytes) { if (bytes) std::memset(p, value, bytes); }
    void copy(void *dst, const void *src, size_t bytes) { if (bytes) std::memcpy(dst, src, bytes); }
    template <class... P, class... A> void launch(const char *name, void (*kernel)(P...), dim3 grid, unsigned block, A... args)
    {
        if (before_launch) before_launch(name, grid);
        assert(grid.z == 1);
        ::launch(grid.x, grid.y, block, !barrier_free.count(name), [=] { kernel(args...); });
    }
};
