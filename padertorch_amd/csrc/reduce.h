// The reduction and vector helpers the glue kernels share (tcn, tasnet, dprnn, orpit, td_loss, norm, pit_loss, tas_coders).
//
// The summation discipline of the library (DESIGN.md "Summation discipline"): every sum over rows, frames or workgroups is fp64, uses
// no atomics and is added in ONE FIXED ORDER, so two runs and a graph replay agree bit for bit:
//   inside a thread      the thread's elements ascending;
//   inside a wave        wave_sum: the 64-lane xor butterfly, offsets 32, 16, 8, 4, 2, 1;
//   inside a workgroup   block_sums: the four waves' totals through LDS, combined ((0 + 1) + 2) + 3;
//   across workgroups    every workgroup writes its partial ("slab") to the caller's workspace and colreduce_kernel adds the slabs of a
//                        column in four interleaved chains s = g, g + 4, ... (ascending), combined ((0 + 1) + 2) + 3.
// A kernel that adds its partials in another order (sequentially, or in a 256-way tree) says so where it is defined and stays there.
#pragma once
#include <initializer_list>

#include "common.h"

namespace ptmi {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// V consecutive floats: one float4 (V == 4, 16-byte aligned) or one float.
template <int V>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&o)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    } else {
        o[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const float (&o)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
        p[0] = o[0];
    }
}

// Sum of s[n] over the workgroup's 256 threads, returned to every thread: lanes by butterfly, then waves 0..3 in order.
template <int N>
__device__ __forceinline__ void block_sums(double (&s)[N]) {
    __shared__ double red[4][N];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const double v = wave_sum(s[n]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][n] = v;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] = ((red[0][n] + red[1][n]) + red[2][n]) + red[3][n];
}

// What colreduce_kernel does with the total of column j.
struct StorePlain {                // out[j]
    float* __restrict__ out;
    __device__ __forceinline__ void operator()(long long j, double tot) const { out[j] = (float)tot; }
};

struct StoreTwice {                // out[j] and, where given, out2[j]: the same sum for a second parameter, without a second pass
    float* __restrict__ out;
    float* __restrict__ out2;
    __device__ __forceinline__ void operator()(long long j, double tot) const {
        const float v = (float)tot;
        out[j] = v;
        if (out2) out2[j] = v;
    }
};

// taps > 0: column j = k C + c of a depthwise slab goes to out[c taps + k] (k < taps: d weight [C, taps]) or out[C taps + c] (d bias);
// taps == 0: out[j].
struct StoreDepthwise {
    float* __restrict__ out;
    int C, taps;
    __device__ __forceinline__ void operator()(long long j, double tot) const {
        long long o = j;
        if (taps > 0) {
            const long long k = j / C, c = j % C;
            o = k < taps ? c * taps + k : (long long)C * taps + c;
        }
        out[o] = (float)tot;
    }
};

// store(j, sum_s ws[s][j]) for j < width: four chains s = g, g + 4, ... (ascending), combined ((0 + 1) + 2) + 3.
// Grid: (width + 63) / 64 workgroups of 256 threads.
template <class Store>
static __global__ __launch_bounds__(256) void colreduce_kernel(const double* __restrict__ ws, long long slabs, long long width,
                                                               const Store store) {
    __shared__ double red[4][64];
    const int jx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long j = (long long)blockIdx.x * 64 + jx;
    double s = 0.;
    if (j < width)
        for (long long sl = g; sl < slabs; sl += 4) s += ws[sl * width + j];
    red[g][jx] = s;
    __syncthreads();
    if (g == 0 && j < width) store(j, ((red[0][jx] + red[1][jx]) + red[2][jx]) + red[3][jx]);
}

template <class Store>
inline int colreduce(const double* ws, long long slabs, long long width, Store store, hipStream_t st) {
    hipLaunchKernelGGL(colreduce_kernel<Store>, dim3((unsigned)((width + 63) / 64)), dim3(256), 0, st, ws, slabs, width, store);
    return launch_status();
}

// Every pointer is 16-byte aligned (a null pointer counts as aligned: an absent operand does not decide the vector width).
inline bool aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

// Samples per workgroup of a streaming pass over batch rows of T samples: ~2048 workgroups per call when the input allows it;
// 1024..65536 samples each.
inline long long pick_chunk(long long batch, long long T) {
    long long chunk = (batch * T + 2047) / 2048;
    chunk = (chunk + 1023) / 1024 * 1024;
    if (chunk < 1024) chunk = 1024;
    if (chunk > 65536) chunk = 65536;
    return chunk;
}

// kernel<4> (16 bytes per lane) or kernel<1>, 256 threads
#define PTMI_LAUNCH_VEC(kernel, vec, grid, st, ...)                                     \
    do {                                                                                \
        if (vec)                                                                        \
            hipLaunchKernelGGL((kernel<4>), grid, dim3(256), 0, st, __VA_ARGS__);       \
        else                                                                            \
            hipLaunchKernelGGL((kernel<1>), grid, dim3(256), 0, st, __VA_ARGS__);       \
    } while (0)

}  // namespace ptmi
