// Fast Griffin-Lim phase retrieval (FGLA) for gfx950: the elementwise kernels and the device-side stop.
//
// Replaces padertorch/contrib/mk/synthesis/parametric/griffin_lim.py:55-56 (the projection onto the given magnitudes, P_A),
// :137-142 (momentum update and RMSE) and :149 (the stop) - there ~10 elementwise complex passes and one host sync per iteration.
// One iteration here is   istft_kernel(P) -> audio,  an update launch (the forward STFT + gl_update_kernel below, or the fused
// gl_stft_update_kernel of stft.hip),  gl_finish_kernel  (DESIGN.md "Griffin-Lim").
//
// Device state of one retrieval (int32 words, all written with plain vector stores):
//   state[0] done             set by gl_finish_kernel when rmse < atol; every later update / finish launch returns without writing
//   state[1] num_iterations   iterations that ran
//   state[2] nparts           partial sums the last update launch left
// Sums: each workgroup (fused: each wavefront) leaves ONE fp64 partial at a slot fixed by its index; gl_finish_kernel adds them in one
// fixed order in fp64 (256 interleaved chains ascending, then block_sums) - no atomics, two runs agree bit for bit.
#include <algorithm>

#include "common.h"
#include "phasor.h"
#include "reduce.h"

namespace ptmi {

constexpr int kGlMaxParts = 16384;     // slots of the partial-sum buffer (ptmi_gl_partials_elems)
constexpr int kGlPerThread = 4;        // bins per thread and pass of the elementwise kernels

// P = a * y / |y|  (angle(0) := 0: y == 0 -> (a, 0); |y|^2 below the normal range: mag_phasor's rescaled branch)
__global__ __launch_bounds__(256) void gl_project_kernel(const float* __restrict__ a, const cpx* __restrict__ y, cpx* __restrict__ P,
                                                         long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float mag;
        cpx u;
        mag_phasor(y[i], mag, u);
        const float av = a[i];
        P[i] = cpx{av * u.x, av * u.y};
    }
}

// d a = Re(conj(u) g), u = y / |y| a constant
__global__ __launch_bounds__(256) void gl_project_backward_kernel(const cpx* __restrict__ g, const cpx* __restrict__ y,
                                                                  float* __restrict__ da, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float mag;
        cpx u;
        mag_phasor(y[i], mag, u);
        const cpx gv = g[i];
        da[i] = u.x * gv.x + u.y * gv.y;
    }
}

// griffin_lim.py:137-142 on a computed x_ = STFT(iSTFT(P)):  y = x_ + alpha (x_ - x);  x <- x_;  P <- a y / |y|;  partial of (|x_| - a)^2.
// Workgroup w owns the bins [w * per_block, (w + 1) * per_block) - a fixed slice, so its partial does not depend on the grid's timing.
__global__ __launch_bounds__(256) void gl_update_kernel(const cpx* __restrict__ xnew, cpx* __restrict__ x, const float* __restrict__ a,
                                                        cpx* __restrict__ P, long long n, long long per_block, float alpha,
                                                        double* __restrict__ partials, int32_t* __restrict__ state) {
    if (state[0] != 0) return;          // stopped: leave x, P, the partials and nparts as the last live iteration left them
    const long long lo = (long long)blockIdx.x * per_block, hi = min(lo + per_block, n);
    double s[1] = {0.};
    for (long long i0 = lo + threadIdx.x; i0 < hi; i0 += 256 * kGlPerThread) {
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < kGlPerThread; ++e) {
            const long long i = i0 + 256 * e;
            if (i < hi) {
                const cpx xn = xnew[i], xo = x[i];
                const float av = a[i];
                const cpx y{xn.x + alpha * (xn.x - xo.x), xn.y + alpha * (xn.y - xo.y)};
                float mag;
                cpx u;
                mag_phasor(y, mag, u);
                x[i] = xn;
                P[i] = cpx{av * u.x, av * u.y};
                const float d = sqrtf(xn.x * xn.x + xn.y * xn.y) - av;
                acc += d * d;
            }
        }
        s[0] += (double)acc;
    }
    block_sums(s);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s[0];
        if (blockIdx.x == 0) state[2] = (int32_t)gridDim.x;
    }
}

// rmse[it] = sqrt(sum of the partials / count); the stop (griffin_lim.py:149: `diff < atol`, false for a NaN).  One workgroup.
__global__ __launch_bounds__(256) void gl_finish_kernel(const double* __restrict__ partials, double count, double atol, int it,
                                                        float* __restrict__ rmse, int32_t* __restrict__ state) {
    if (state[0] != 0) return;
    const int nparts = min(max(state[2], 0), kGlMaxParts);
    double s[1] = {0.};
    for (int i = threadIdx.x; i < nparts; i += 256) s[0] += partials[i];
    block_sums(s);
    if (threadIdx.x == 0) {
        const double diff = sqrt(s[0] / count);
        rmse[it] = (float)diff;
        state[1] = it + 1;
        if (diff < atol) state[0] = 1;
    }
}

static unsigned gl_grid(long long n) {
    return (unsigned)std::min<long long>((n + 256 * kGlPerThread - 1) / (256 * kGlPerThread), 4096);
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_gl_partials_elems(void) { return kGlMaxParts; }

int ptmi_gl_project(const float* a, const float* y, int64_t n, float* P, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!a || !y || !P || n < 0, PTMI_E_INVALID);
    if (n == 0) return PTMI_OK;
    hipLaunchKernelGGL(gl_project_kernel, dim3(gl_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                       reinterpret_cast<const cpx*>(y), reinterpret_cast<cpx*>(P), (long long)n);
    return launch_status();
}

int ptmi_gl_project_backward(const float* g, const float* y, int64_t n, float* da, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!g || !y || !da || n < 0, PTMI_E_INVALID);
    if (n == 0) return PTMI_OK;
    hipLaunchKernelGGL(gl_project_backward_kernel, dim3(gl_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const cpx*>(g), reinterpret_cast<const cpx*>(y), da, (long long)n);
    return launch_status();
}

int ptmi_gl_update(const float* xnew, float* x, const float* a, int64_t n, float alpha, float* P, double* partials, int32_t* state,
                   ptmi_stream_t stream) {
    PTMI_RETURN_IF(!xnew || !x || !a || !P || !partials || !state || n <= 0, PTMI_E_INVALID);
    // fixed slices of whole passes: at most 4096 (<= kGlMaxParts) workgroups
    const long long pass = 256 * kGlPerThread;
    long long per_block = ((n + 4095) / 4096 + pass - 1) / pass * pass;
    const long long blocks = (n + per_block - 1) / per_block;
    hipLaunchKernelGGL(gl_update_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const cpx*>(xnew), reinterpret_cast<cpx*>(x), a, reinterpret_cast<cpx*>(P), (long long)n, per_block,
                       alpha, partials, state);
    return launch_status();
}

int ptmi_gl_finish(const double* partials, int64_t count, double atol, int32_t iteration, float* rmse, int32_t* state,
                   ptmi_stream_t stream) {
    PTMI_RETURN_IF(!partials || !rmse || !state || count <= 0 || iteration < 0, PTMI_E_INVALID);
    hipLaunchKernelGGL(gl_finish_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), partials, (double)count, atol,
                       (int)iteration, rmse, state);
    return launch_status();
}

}  // extern "C"
