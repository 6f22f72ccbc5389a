// The convolutions of the BigVGAN generator (inference) for gfx950: everything in nvidia_bigvgan/bigvgan.py that is not the anti-aliased
// activation (csrc/anti_alias.hip).  fp32, activations [B, C, T] with T contiguous - the layout of anti_alias_forward, so nothing is
// transposed between an activation and a convolution - zero padding, no atomics, every sum in one fixed order, nothing read on the host.
//
//   bigvgan_taps         the second half of a dilated Conv1d on the GEMM path.  The channel mixing is a ptmi_gemm_planes call per batch
//                        entry, P_b [K C_out, T] = Wtaps [K C_out, C_in] x_b [C_in, T] (row k C_out + co: tap k of output channel co); this
//                        kernel adds the K shifted rows: y[b,co,t] = bias[co] + sum_k P[b,k,co,t + (k - (K-1)/2) d], zero outside [0, T).
//                        A thread owns four consecutive t; a tap whose shift is a multiple of four is one 16-byte load (T % 4 == 0).
//   bigvgan_conv_direct  the same Conv1d without P, for narrow layers: plain fp32 FMAs, ci ascending then k ascending, summed per chunk of
//                        kDirCi input channels and the chunk sums added in ascending order.  A workgroup owns
//                        kDirCo output channels x kDirTile samples of one batch entry and walks C_in in chunks of kDirCi: the chunk's
//                        weights [ci][k][co] and the chunk's x rows with their (K-1) d / 2 halo are staged in LDS, a thread keeps
//                        kDirCo x 2 accumulators (one x value from LDS feeds 16 FMAs, the weights come as four 16-byte broadcasts).
//   both end in          v = scale (conv + bias + residual); out = v or out += v: the `x = xt + x` of an AMP block, and - the last
//                        convolution of every block writing with scale = 1 / num_kernels into one accumulator - the mean over blocks.
//   bigvgan_ola          ConvTranspose1d(C_in, C_out, k, u, padding = (k - u) / 2) behind its GEMM G_b [C_out k, T] = W^T x_b: gather-form
//                        overlap-add, bias and crop.  out[b,co,t'] = bias[co] + sum_f G[b, co k + kk, f] over f u + kk - p = t', f ascending:
//                        at most ceil(k / u) terms.  Lanes run along t'; the lanes of one kk read consecutive f.
//   bigvgan_post         conv_post (C -> 1 channel, K taps) and the final tanh / clamp in one launch: c ascending, k ascending.
#include <algorithm>

#include "common.h"

namespace ptmi {

constexpr int kTapsTile = 1024;       // samples of a row one workgroup of bigvgan_taps covers (256 threads x 4)
constexpr int kTapsMaxK = 63;
constexpr int kDirTile = 512;         // samples per workgroup of bigvgan_conv_direct (256 threads x 2)
constexpr int kDirPer = kDirTile / 256;
constexpr int kDirCo = 16;            // output channels per workgroup
constexpr int kDirCi = 8;             // input channels per staged chunk
constexpr int kDirMaxK = 11;          // taps the weight chunk in LDS is sized for
constexpr int kDirMaxHalo = 64;       // (K - 1) d / 2 the x chunk in LDS is sized for
constexpr int kDirMaxC = 128;         // above this width the matrix cores win whatever K is (ops/bigvgan.py has the measured crossover)
constexpr int kDirXw = kDirTile + 2 * kDirMaxHalo;
constexpr int kOlaMaxStride = 8;
constexpr int kPostMaxK = 11;

struct Epilogue {
    const float* bias;         // [C_out] or NULL
    const float* residual;     // [B, C_out, T] or NULL
    float scale;
    int accumulate;
};

__device__ __forceinline__ void epilogue_store(const Epilogue& E, float acc, int co, long long idx, float* out) {
    float v = acc;
    if (E.bias) v += E.bias[co];
    if (E.residual) v += E.residual[idx];
    v *= E.scale;
    out[idx] = E.accumulate ? out[idx] + v : v;
}

// ------------------------------------------------------------------------------------------------------------ taps (GEMM path)
template <int VEC>
static __global__ __launch_bounds__(256) void bigvgan_taps_kernel(const float* __restrict__ P, int C_out, int T, int K, int d, long long quads,
                                                                  int qt, const Epilogue E, float* out) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const long long row = q / qt;                            // b C_out + co
    const int t0 = (int)(q - row * qt) * 4;
    const long long b = row / C_out;
    const int co = (int)(row - b * C_out), h = (K - 1) / 2;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
        const float* __restrict__ p = P + ((b * K + k) * C_out + co) * (long long)T;
        const int ts = t0 + (k - h) * d;                     // the tap reads p[ts .. ts + 3]
        if (ts >= T || ts + 3 < 0) continue;
        if (VEC == 4 && (ts & 3) == 0) {                     // T % 4 == 0: an aligned group of four lies inside the row as a whole
            const float4 v = *reinterpret_cast<const float4*>(p + ts);
            acc[0] += v.x, acc[1] += v.y, acc[2] += v.z, acc[3] += v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ts + j >= 0 && ts + j < T) acc[j] += p[ts + j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (t0 + j < T) epilogue_store(E, acc[j], co, row * T + t0 + j, out);
}

// ------------------------------------------------------------------------------------------------------------ direct path
static __global__ __launch_bounds__(256) void bigvgan_conv_direct_kernel(const float* __restrict__ x, const float* __restrict__ w, int C_in,
                                                                         int C_out, int T, int K, int d, const Epilogue E, float* out) {
    __shared__ __align__(16) float ws[kDirCi * kDirMaxK * kDirCo];
    __shared__ __align__(16) float xs[kDirCi * kDirXw];
    const int t0 = blockIdx.x * kDirTile, co0 = blockIdx.y * kDirCo;
    const long long b = blockIdx.z;
    const int halo = (K - 1) / 2 * d, width = kDirTile + 2 * halo;          // width <= kDirXw (checked on the host)
    float acc[kDirPer][kDirCo];
#pragma unroll
    for (int j = 0; j < kDirPer; ++j)
#pragma unroll
        for (int c = 0; c < kDirCo; ++c) acc[j][c] = 0.f;
    for (int c0 = 0; c0 < C_in; c0 += kDirCi) {
        const int nci = min(kDirCi, C_in - c0);
        __syncthreads();                                                    // the last chunk's readers are done
        for (int i = threadIdx.x; i < nci * width; i += 256) {
            const int ci = i / width, p = i - ci * width, t = t0 - halo + p;
            xs[ci * kDirXw + p] = (t >= 0 && t < T) ? x[(b * C_in + c0 + ci) * (long long)T + t] : 0.f;
        }
        for (int i = threadIdx.x; i < nci * K * kDirCo; i += 256) {
            const int cl = i % kDirCo, k = (i / kDirCo) % K, ci = i / (kDirCo * K);
            ws[(ci * kDirMaxK + k) * kDirCo + cl] = co0 + cl < C_out ? w[((long long)(co0 + cl) * C_in + c0 + ci) * K + k] : 0.f;
        }
        __syncthreads();
        // the chunk's kDirCi K terms in a sum of their own, then one addition to the total: a single chain over all C_in K terms (1408 at
        // 128 channels and 11 taps) strays further from the exact sum than the blocked order torch's fp32 convolution shows
        float part[kDirPer][kDirCo];
#pragma unroll
        for (int j = 0; j < kDirPer; ++j)
#pragma unroll
            for (int c = 0; c < kDirCo; ++c) part[j][c] = 0.f;
        for (int ci = 0; ci < nci; ++ci) {
            for (int k = 0; k < K; ++k) {
                const float4* __restrict__ wp = reinterpret_cast<const float4*>(ws + (ci * kDirMaxK + k) * kDirCo);
                const float4 w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3];
                const float wv[kDirCo] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w, w3.x, w3.y, w3.z, w3.w};
#pragma unroll
                for (int j = 0; j < kDirPer; ++j) {
                    const float xv = xs[ci * kDirXw + (int)threadIdx.x + 256 * j + k * d];
#pragma unroll
                    for (int c = 0; c < kDirCo; ++c) part[j][c] = fmaf(wv[c], xv, part[j][c]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kDirPer; ++j)
#pragma unroll
            for (int c = 0; c < kDirCo; ++c) acc[j][c] += part[j][c];
    }
#pragma unroll
    for (int c = 0; c < kDirCo; ++c) {
        if (co0 + c >= C_out) break;
#pragma unroll
        for (int j = 0; j < kDirPer; ++j) {
            const int t = t0 + (int)threadIdx.x + 256 * j;
            if (t < T) epilogue_store(E, acc[j][c], co0 + c, (b * C_out + co0 + c) * (long long)T + t, out);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ overlap-add
static __global__ __launch_bounds__(256) void bigvgan_ola_kernel(const float* __restrict__ G, const float* __restrict__ bias, int C_out, int T,
                                                                 int k, int u, int pad, int Tout, float* __restrict__ out) {
    const int tp = blockIdx.x * 256 + threadIdx.x;
    if (tp >= Tout) return;
    const int co = blockIdx.y;
    const long long b = blockIdx.z;
    const int s = tp + pad, f0 = s / u, kk0 = s - f0 * u;
    const float* __restrict__ g = G + (b * C_out + co) * (long long)k * T;
    float acc = 0.f;
    for (int j = (k - 1 - kk0) / u; j >= 0; --j) {           // f = f0 - j ascending
        const int f = f0 - j;
        if (f >= 0 && f < T) acc += g[(long long)(kk0 + j * u) * T + f];
    }
    out[(b * C_out + co) * (long long)Tout + tp] = bias ? acc + bias[co] : acc;
}

// ------------------------------------------------------------------------------------------------------------ conv_post
// NaN comes out as NaN under the clamp: both comparisons are false for it (fminf / fmaxf would return the bound).
__device__ __forceinline__ float clamp_unit(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

static __global__ __launch_bounds__(256) void bigvgan_post_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, int C, int T, int K, int use_tanh,
                                                                  float* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const long long b = blockIdx.y;
    const int h = (K - 1) / 2;
    const int klo = max(0, h - t), khi = min(K, T - t + h);                 // taps with 0 <= t + k - h < T
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ xr = x + (b * C + c) * (long long)T + (t - h);
        const float* __restrict__ wr = w + c * K;
        for (int k = klo; k < khi; ++k) acc = fmaf(wr[k], xr[k], acc);
    }
    if (bias) acc += bias[0];
    out[b * T + t] = use_tanh ? tanhf(acc) : clamp_unit(acc);
}

static int conv_args_ok(int64_t B, int32_t C_in, int32_t C_out, int64_t T, int32_t K, int32_t d) {
    return B >= 0 && C_in > 0 && C_out > 0 && T >= 0 && K >= 1 && (K & 1) && d >= 1;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_bigvgan_direct_max_channels(void) { return kDirMaxC; }

int32_t ptmi_bigvgan_tile(int32_t direct) { return direct ? kDirTile : kTapsTile; }

int32_t ptmi_bigvgan_direct_ok(int32_t C_in, int32_t K, int32_t dilation) {
    return C_in >= 1 && C_in <= kDirMaxC && K >= 1 && (K & 1) && K <= kDirMaxK && dilation >= 1 &&
           (int64_t)(K - 1) / 2 * dilation <= kDirMaxHalo;
}

int64_t ptmi_bigvgan_ola_out_len(int64_t T, int32_t k, int32_t u) {
    if (T < 1 || u < 1 || u > kOlaMaxStride || k < u) return -1;
    return (T - 1) * u - 2 * ((k - u) / 2) + k;
}

int ptmi_bigvgan_taps(const float* P, const float* bias, const float* residual, int64_t B, int32_t C_out, int64_t T, int32_t K,
                      int32_t dilation, float scale, int32_t accumulate, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!P || !out || !conv_args_ok(B, 1, C_out, T, K, dilation) || K > kTapsMaxK, PTMI_E_INVALID);
    PTMI_RETURN_IF(T >= (1ll << 30) || (int64_t)dilation * K >= (1ll << 30), PTMI_E_INVALID);
    if (B == 0 || T == 0) return PTMI_OK;
    const int qt = (int)((T + 3) / 4);
    const long long quads = (long long)B * C_out * qt;
    PTMI_RETURN_IF((quads + 255) / 256 >= (1ll << 31), PTMI_E_INVALID);
    const Epilogue E{bias, residual, scale, accumulate ? 1 : 0};
    const dim3 grid((unsigned)((quads + 255) / 256));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (T % 4 == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0)
        hipLaunchKernelGGL(bigvgan_taps_kernel<4>, grid, dim3(256), 0, st, P, (int)C_out, (int)T, (int)K, (int)dilation, quads, qt, E, out);
    else
        hipLaunchKernelGGL(bigvgan_taps_kernel<1>, grid, dim3(256), 0, st, P, (int)C_out, (int)T, (int)K, (int)dilation, quads, qt, E, out);
    return launch_status();
}

int ptmi_bigvgan_conv_direct(const float* x, const float* weight, const float* bias, const float* residual, int64_t B, int32_t C_in,
                             int32_t C_out, int64_t T, int32_t K, int32_t dilation, float scale, int32_t accumulate, float* out,
                             ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !weight || !out || !conv_args_ok(B, C_in, C_out, T, K, dilation), PTMI_E_INVALID);
    PTMI_RETURN_IF(!ptmi_bigvgan_direct_ok(C_in, K, dilation), PTMI_E_INVALID);
    PTMI_RETURN_IF(T >= (1ll << 30) || B > 65535 || (C_out + kDirCo - 1) / kDirCo > 65535, PTMI_E_INVALID);
    if (B == 0 || T == 0) return PTMI_OK;
    const Epilogue E{bias, residual, scale, accumulate ? 1 : 0};
    const dim3 grid((unsigned)((T + kDirTile - 1) / kDirTile), (unsigned)((C_out + kDirCo - 1) / kDirCo), (unsigned)B);
    hipLaunchKernelGGL(bigvgan_conv_direct_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, weight, (int)C_in, (int)C_out,
                       (int)T, (int)K, (int)dilation, E, out);
    return launch_status();
}

int ptmi_bigvgan_ola(const float* G, const float* bias, int64_t B, int32_t C_out, int64_t T, int32_t k, int32_t u, float* out,
                     ptmi_stream_t stream) {
    PTMI_RETURN_IF(!G || !out || B < 0 || C_out < 1 || C_out > 65535 || B > 65535 || T < 0, PTMI_E_INVALID);
    PTMI_RETURN_IF(u < 1 || u > kOlaMaxStride || k < u || k > (1 << 20), PTMI_E_INVALID);
    if (B == 0 || T == 0) return PTMI_OK;
    const int64_t Tout = ptmi_bigvgan_ola_out_len(T, k, u);
    PTMI_RETURN_IF(Tout < 1 || Tout + k >= (1ll << 30), PTMI_E_INVALID);
    const dim3 grid((unsigned)((Tout + 255) / 256), (unsigned)C_out, (unsigned)B);
    hipLaunchKernelGGL(bigvgan_ola_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), G, bias, (int)C_out, (int)T, (int)k, (int)u,
                       (int)((k - u) / 2), (int)Tout, out);
    return launch_status();
}

int ptmi_bigvgan_post(const float* x, const float* weight, const float* bias, int64_t B, int32_t C, int64_t T, int32_t K, int32_t use_tanh,
                      float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !weight || !out || !conv_args_ok(B, C, 1, T, K, 1) || K > kPostMaxK, PTMI_E_INVALID);
    PTMI_RETURN_IF(T >= (1ll << 30) || B > 65535 || (int64_t)C * K >= (1ll << 30), PTMI_E_INVALID);
    if (B == 0 || T == 0) return PTMI_OK;
    const dim3 grid((unsigned)((T + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(bigvgan_post_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, weight, bias, (int)C, (int)T, (int)K,
                       use_tanh ? 1 : 0, out);
    return launch_status();
}

}  // extern "C"
