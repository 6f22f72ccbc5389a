// TasNet learned-basis coders (padertorch/contrib/examples/source_separation/tasnet/tas_coders.py:9-135:
// TasEncoder = Conv1d(1, N, L, stride) + ReLU, TasDecoder = ConvTranspose1d(N, 1, L, stride)) and the
// "mask x encoded -> decode" tail of TasNet.forward (tasnet/model.py:119-129), forward and backward.
//
// Layouts: signals x [B, T], features [B, N, E] (E = encoded frames, contiguous), masks [K, B, N, E],
// weights W [N, L] (the [N, 1, L] parameter of either module), all fp32 and contiguous.
//
// Three kernel families cover every forward and backward of the three operators:
//   analysis   out[b,n,tau] = act(sum_l W[n,l] x[b, tau s + l] + bias[n])      one thread per tau, loops over n:
//              stores coalesced along tau; samples at or beyond T read as zero (the reference's F.pad, never
//              copied).  With the masks: A_k = analysis(gy[k,b]) stays in registers and leaves as
//              dm[k] = e A_k and de = sum_k m[k] A_k (m, e read once, dm, de written once).
//   synthesis  y[b,t] = sum_n sum_{tau s + l = t} p[b,n,tau] W[n,l] (+ bias)   gather form: one thread owns one
//              output sample, so there is no atomic and no ordering question; p = e, m[k] e (K outputs per
//              thread, m e is never stored) or g (w > 0) (the encoder's ReLU backward) formed on the fly.
//   wgrad      dW[n,l] = sum_{b,tau} g[b,n,tau] x[b, tau s + l], sum_{b,tau} g[b,n,tau] (the encoder's bias
//              gradient) and sum_{b,t} x[b,t] (the decoder's) from one pass: a workgroup owns 256 (n, l) pairs
//              and one (b, tau range), stages g and the x segment in LDS, and writes its partial sums to the
//              caller's workspace; a second kernel adds the partials in (b, tau range) order.
// All sums have a fixed order (l ascending; n, tau ascending; lanes by reduce.h's wave_sum; partials ascending): results are
// bit-reproducible.
#include <algorithm>

#include "reduce.h"

namespace ptmi {

constexpr int kTasNC = 16;          // feature rows per analysis workgroup
constexpr int kTasMaxKT = 4;        // masks held in registers at once
constexpr int kTasGs = 8192;        // wgrad: floats of the staged g tile
constexpr int kTasXs = 4096;        // wgrad: floats of the staged x segment
constexpr int kTasSynLds = 12288;   // synthesis: the weights are staged in LDS up to this many floats

struct TasAnaArgs {
    const float* x;       // [KT rows of] [B, T]: row k at x + k * xk
    const float* w;       // [N, L]
    const float* bias;    // [N] or null
    const float* mask;    // [K, B, N, E] or null
    const float* enc;     // [B, N, E]    (with mask)
    float* out;           // [B, N, E]; with mask: de
    float* dmask;         // [K, B, N, E] (with mask)
    long long T, E, xk;   // xk = B * T
    int N, L, s, K, relu;
};

// L <= LP <= 32: the thread's window of every signal lives in registers, the weights of the workgroup's
// kTasNC rows in LDS (zero-padded to LP, read as broadcasts).
template <int LP, int KT>
__global__ __launch_bounds__(256) void tas_analysis_reg_kernel(const TasAnaArgs A) {
    __shared__ float ws[kTasNC][LP];
    const int b = blockIdx.z, n0 = blockIdx.y * kTasNC;
    for (int i = threadIdx.x; i < kTasNC * LP; i += 256) {
        const int n = n0 + i / LP, l = i % LP;
        ws[i / LP][l] = (n < A.N && l < A.L) ? A.w[(long long)n * A.L + l] : 0.f;
    }
    __syncthreads();
    const long long tau = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tau >= A.E) return;
    float xv[KT][LP];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const float* __restrict__ xr = A.x + k * A.xk + (long long)b * A.T;
#pragma unroll
        for (int l = 0; l < LP; ++l) {
            const long long t = tau * A.s + l;
            xv[k][l] = (l < A.L && t < A.T && k < A.K) ? xr[t] : 0.f;
        }
    }
    const int n1 = min(n0 + kTasNC, A.N);
    const long long kstride = (long long)gridDim.z * A.N * A.E;
    for (int n = n0; n < n1; ++n) {
        float acc[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) acc[k] = 0.f;
#pragma unroll
        for (int l = 0; l < LP; ++l) {
            const float wv = ws[n - n0][l];
#pragma unroll
            for (int k = 0; k < KT; ++k) acc[k] = fmaf(wv, xv[k][l], acc[k]);
        }
        const long long o = ((long long)b * A.N + n) * A.E + tau;
        if (A.mask) {
            const float e = A.enc[o];
            float de = 0.f;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                if (k < A.K) {
                    de = fmaf(A.mask[k * kstride + o], acc[k], de);
                    A.dmask[k * kstride + o] = e * acc[k];
                }
            }
            A.out[o] = de;
        } else {
            float v = acc[0] + (A.bias ? A.bias[n] : 0.f);
            A.out[o] = (A.relu && v < 0.f) ? 0.f : v;
        }
    }
}

// Any L, any K: the same sums in the same order, the signal read through the caches.
__global__ __launch_bounds__(256) void tas_analysis_generic_kernel(const TasAnaArgs A) {
    const int b = blockIdx.z, n0 = blockIdx.y * kTasNC;
    const long long tau = (long long)blockIdx.x * 256 + threadIdx.x;
    if (tau >= A.E) return;
    const int n1 = min(n0 + kTasNC, A.N);
    const long long kstride = (long long)gridDim.z * A.N * A.E;
    const long long t0 = tau * A.s;
    for (int n = n0; n < n1; ++n) {
        const float* __restrict__ wr = A.w + (long long)n * A.L;
        const long long o = ((long long)b * A.N + n) * A.E + tau;
        float de = 0.f;
        const float e = A.mask ? A.enc[o] : 0.f;
        for (int k = 0; k < A.K; ++k) {
            const float* __restrict__ xr = A.x + k * A.xk + (long long)b * A.T;
            float acc = 0.f;
            for (int l = 0; l < A.L; ++l) acc = fmaf(wr[l], (t0 + l < A.T) ? xr[t0 + l] : 0.f, acc);
            if (A.mask) {
                de = fmaf(A.mask[k * kstride + o], acc, de);
                A.dmask[k * kstride + o] = e * acc;
            } else {
                const float v = acc + (A.bias ? A.bias[n] : 0.f);
                A.out[o] = (A.relu && v < 0.f) ? 0.f : v;
            }
        }
        if (A.mask) A.out[o] = de;
    }
}

struct TasSynArgs {
    const float* p;      // [B, N, E]
    const float* mask;   // [K, B, N, E] or null
    const float* gate;   // [B, N, E] or null: p counts where gate > 0
    const float* w;      // [N, L]
    const float* bias;   // [1] or null
    float* y;            // [K, B, Ty]
    long long E, Ty;
    int N, L, s, K;
};

// One thread per output sample t of row b (and of up to KT masks): tau from ceil((t - L + 1) / s) to t / s.
template <int KT, bool LDSW>
__global__ __launch_bounds__(256) void tas_synthesis_kernel(const TasSynArgs A) {
    extern __shared__ __align__(16) float wl[];
    if (LDSW) {
        for (int i = threadIdx.x; i < A.N * A.L; i += 256) wl[i] = A.w[i];
        __syncthreads();
    }
    const int b = blockIdx.y, k0 = blockIdx.z * KT;
    const long long B = gridDim.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= A.Ty) return;
    const long long tau_lo = t >= A.L ? (t - A.L) / A.s + 1 : 0;
    const long long tau_hi = min(A.E - 1, t / A.s);
    const long long kstride = B * A.N * A.E;
    float acc[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) acc[k] = 0.f;
    for (int n = 0; n < A.N; ++n) {
        const long long row = ((long long)b * A.N + n) * A.E;
        for (long long tau = tau_lo; tau <= tau_hi; ++tau) {
            const int l = (int)(t - tau * A.s);
            const float wv = LDSW ? wl[n * A.L + l] : A.w[(long long)n * A.L + l];
            float pv = A.p[row + tau];
            if (A.gate) pv = A.gate[row + tau] > 0.f ? pv : 0.f;
            if (A.mask) {
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k0 + k < A.K) acc[k] = fmaf(A.mask[(k0 + k) * kstride + row + tau] * pv, wv, acc[k]);
            } else {
                acc[0] = fmaf(pv, wv, acc[0]);
            }
        }
    }
    const float bv = A.bias ? A.bias[0] : 0.f;
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k0 + k < A.K) A.y[((k0 + k) * B + b) * A.Ty + t] = acc[k] + bv;
}

struct TasWgArgs {
    const float* g;      // [B, N, E]
    const float* mask;   // [K, B, N, E] or null: g counts as mask[k] g, x as x[k]
    const float* gate;   // [B, N, E] or null: g counts where gate > 0
    const float* x;      // [K, B, T]
    float* ws;           // [B * nchunks][N L + N + 1]
    long long T, E;
    int N, L, s, K, tc, nchunks, xlds;
};

// Workgroup (pair block, tau chunk, b): thread <-> pair (n, l) = p0 + threadIdx.x; the rows n of the pair block's
// g tile and the signal segment [tau0 s, (tau0 + tc - 1) s + L) come through LDS (XLDS; a segment that does not
// fit is read through the caches).
template <bool XLDS>
__global__ __launch_bounds__(256) void tas_wgrad_kernel(const TasWgArgs A) {
    __shared__ float gs[kTasGs];
    __shared__ float xs[XLDS ? kTasXs : 1];
    __shared__ float red[4];
    const int b = blockIdx.z, c = blockIdx.y;
    const long long B = gridDim.z;
    const long long P = (long long)A.N * A.L;
    const long long p0 = (long long)blockIdx.x * 256;
    const int nf = (int)(p0 / A.L);
    const int nl = (int)(min(p0 + 255, P - 1) / A.L);
    const int rows = nl - nf + 1;
    const long long tau0 = (long long)c * A.tc;
    const int tc = (int)min((long long)A.tc, A.E - tau0);
    const int ld = A.tc | 1;
    const long long seg0 = tau0 * A.s;
    const long long seg = (long long)(tc - 1) * A.s + A.L;
    const long long pr = p0 + threadIdx.x;
    const bool live = pr < P;
    const int n = live ? (int)(pr / A.L) : nf, l = live ? (int)(pr % A.L) : 0;
    const int r = n - nf;
    // the samples this workgroup alone counts for sum x: up to the next chunk's first sample; the last chunk to the end
    const long long own1 = (c == A.nchunks - 1) ? A.T : min(A.T, (tau0 + tc) * A.s);
    float acc = 0.f, gsum = 0.f, xsum = 0.f;
    for (int k = 0; k < A.K; ++k) {
        const float* __restrict__ xr = A.x + ((long long)k * B + b) * A.T;
        __syncthreads();
        for (int i = threadIdx.x; i < rows * tc; i += 256) {
            const int rr = i / tc, tt = i % tc;
            const long long o = ((long long)b * A.N + nf + rr) * A.E + tau0 + tt;
            float v = A.g[o];
            if (A.gate) v = A.gate[o] > 0.f ? v : 0.f;
            if (A.mask) v *= A.mask[(long long)k * B * A.N * A.E + o];
            gs[rr * ld + tt] = v;
        }
        if (XLDS)
            for (long long i = threadIdx.x; i < seg; i += 256) xs[i] = (seg0 + i < A.T) ? xr[seg0 + i] : 0.f;
        if (blockIdx.x == 0)
            for (long long t = seg0 + threadIdx.x; t < own1; t += 256) xsum += xr[t];
        __syncthreads();
        if (live) {
            for (int tt = 0; tt < tc; ++tt) {
                const long long t = (long long)tt * A.s + l;
                const float xv = XLDS ? xs[t] : ((seg0 + t < A.T) ? xr[seg0 + t] : 0.f);
                acc = fmaf(gs[r * ld + tt], xv, acc);
            }
            if (l == 0)
                for (int tt = 0; tt < tc; ++tt) gsum += gs[r * ld + tt];
        }
    }
    float* slab = A.ws + ((long long)b * A.nchunks + c) * (P + A.N + 1);
    if (live) {
        slab[pr] = acc;
        if (l == 0) slab[P + n] = gsum;
    }
    if (blockIdx.x == 0) {
        const float v = wave_sum(xsum);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) slab[P + A.N] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// out[j] = sum_c ws[c][j], c ascending.
__global__ __launch_bounds__(256) void tas_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, long long width,
                                                               long long slabs) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= width) return;
    float v = 0.f;
    for (long long c = 0; c < slabs; ++c) v += ws[c * width + j];
    out[j] = v;
}

// tau values per wgrad workgroup: the g tile of the pair block's rows and (when it can) the x segment fit the LDS arrays
static void wgrad_plan(int N, int L, int s, long long E, int* tc, int* xlds) {
    const int rows = (int)std::min<long long>(N, 255 / L + 2);      // 256 consecutive (n, l) pairs touch at most this many rows
    long long t = std::min<long long>(256, kTasGs / rows - 1);
    *xlds = 0;
    if (L <= kTasXs) {
        const long long tx = (kTasXs - L) / s + 1;
        if (tx >= 8 || tx >= E) {
            *xlds = 1;
            t = std::min(t, tx);
        }
    }
    t = std::max<long long>(1, std::min(t, E));
    *tc = (int)t;
}

template <int LP>
static void launch_analysis_reg(const TasAnaArgs& A, dim3 grid, hipStream_t st) {
    switch (A.mask ? A.K : 1) {
        case 1: hipLaunchKernelGGL((tas_analysis_reg_kernel<LP, 1>), grid, dim3(256), 0, st, A); break;
        case 2: hipLaunchKernelGGL((tas_analysis_reg_kernel<LP, 2>), grid, dim3(256), 0, st, A); break;
        case 3: hipLaunchKernelGGL((tas_analysis_reg_kernel<LP, 3>), grid, dim3(256), 0, st, A); break;
        default: hipLaunchKernelGGL((tas_analysis_reg_kernel<LP, 4>), grid, dim3(256), 0, st, A);
    }
}

static int launch_analysis(const TasAnaArgs& A, long long B, hipStream_t st) {
    const long long tiles = (A.E + 255) / 256;
    PTMI_RETURN_IF(tiles > 0x7fffffffLL || B > 65535 || (A.N + kTasNC - 1) / kTasNC > 65535, PTMI_E_UNSUPPORTED);
    const dim3 grid((unsigned)tiles, (unsigned)((A.N + kTasNC - 1) / kTasNC), (unsigned)B);
    if (A.L <= 32 && A.K <= kTasMaxKT) {
        if (A.L <= 8) launch_analysis_reg<8>(A, grid, st);
        else if (A.L <= 16) launch_analysis_reg<16>(A, grid, st);
        else if (A.L <= 24) launch_analysis_reg<24>(A, grid, st);
        else launch_analysis_reg<32>(A, grid, st);
    } else {
        hipLaunchKernelGGL(tas_analysis_generic_kernel, grid, dim3(256), 0, st, A);
    }
    return launch_status();
}

template <int KT>
static void launch_synthesis(const TasSynArgs& A, dim3 grid, hipStream_t st) {
    const long long nw = (long long)A.N * A.L;
    if (nw <= kTasSynLds)
        hipLaunchKernelGGL((tas_synthesis_kernel<KT, true>), grid, dim3(256), (size_t)nw * sizeof(float), st, A);
    else
        hipLaunchKernelGGL((tas_synthesis_kernel<KT, false>), grid, dim3(256), 0, st, A);
}

static bool tas_geometry_ok(int64_t B, int32_t N, int32_t L, int32_t s, int64_t E) {
    return B >= 1 && N >= 1 && L >= 1 && s >= 1 && E >= 1;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_tas_analysis(const float* x, const float* weight, const float* bias, float* out, int64_t B, int64_t T, int32_t N,
                      int32_t L, int32_t stride, int64_t E, int32_t relu, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !weight || !out, PTMI_E_INVALID);
    PTMI_RETURN_IF(!tas_geometry_ok(B, N, L, stride, E) || T < 1, PTMI_E_INVALID);
    TasAnaArgs A{};
    A.x = x;
    A.w = weight;
    A.bias = bias;
    A.out = out;
    A.T = T;
    A.E = E;
    A.xk = B * T;
    A.N = N;
    A.L = L;
    A.s = stride;
    A.K = 1;
    A.relu = relu;
    return launch_analysis(A, B, static_cast<hipStream_t>(stream));
}

int ptmi_tas_masked_decode_backward(const float* gy, const float* mask, const float* encoded, const float* weight, float* dmask,
                                    float* dencoded, int32_t K, int64_t B, int64_t T, int32_t N, int32_t L, int32_t stride,
                                    int64_t E, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gy || !mask || !encoded || !weight || !dmask || !dencoded, PTMI_E_INVALID);
    PTMI_RETURN_IF(!tas_geometry_ok(B, N, L, stride, E) || T < 1 || K < 1, PTMI_E_INVALID);
    TasAnaArgs A{};
    A.x = gy;
    A.w = weight;
    A.mask = mask;
    A.enc = encoded;
    A.out = dencoded;
    A.dmask = dmask;
    A.T = T;
    A.E = E;
    A.xk = B * T;
    A.N = N;
    A.L = L;
    A.s = stride;
    A.K = K;
    return launch_analysis(A, B, static_cast<hipStream_t>(stream));
}

int ptmi_tas_synthesis(const float* p, const float* mask, const float* gate, const float* weight, const float* bias, float* y,
                       int32_t K, int64_t B, int32_t N, int32_t L, int32_t stride, int64_t E, int64_t T_out,
                       ptmi_stream_t stream) {
    PTMI_RETURN_IF(!p || !weight || !y, PTMI_E_INVALID);
    PTMI_RETURN_IF(!tas_geometry_ok(B, N, L, stride, E) || T_out < 1 || K < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((!mask && K != 1) || (mask && gate), PTMI_E_INVALID);
    const long long tiles = (T_out + 255) / 256;
    const int kt = K < kTasMaxKT ? K : kTasMaxKT;
    const long long kchunks = (K + kt - 1) / kt;
    PTMI_RETURN_IF(tiles > 0x7fffffffLL || B > 65535 || kchunks > 65535, PTMI_E_UNSUPPORTED);
    TasSynArgs A{};
    A.p = p;
    A.mask = mask;
    A.gate = gate;
    A.w = weight;
    A.bias = bias;
    A.y = y;
    A.E = E;
    A.Ty = T_out;
    A.N = N;
    A.L = L;
    A.s = stride;
    A.K = K;
    const dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)kchunks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (kt) {
        case 1: launch_synthesis<1>(A, grid, st); break;
        case 2: launch_synthesis<2>(A, grid, st); break;
        case 3: launch_synthesis<3>(A, grid, st); break;
        default: launch_synthesis<4>(A, grid, st);
    }
    return launch_status();
}

int64_t ptmi_tas_wgrad_workspace_elems(int64_t B, int32_t N, int32_t L, int32_t stride, int64_t E) {
    if (!tas_geometry_ok(B, N, L, stride, E)) return PTMI_E_INVALID;
    int tc, xlds;
    wgrad_plan(N, L, stride, E, &tc, &xlds);
    return B * ((E + tc - 1) / tc) * ((int64_t)N * L + N + 1);
}

int ptmi_tas_wgrad(const float* g, const float* mask, const float* gate, const float* x, int32_t K, int64_t B, int64_t T,
                   int32_t N, int32_t L, int32_t stride, int64_t E, float* workspace, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!g || !x || !workspace || !out, PTMI_E_INVALID);
    PTMI_RETURN_IF(!tas_geometry_ok(B, N, L, stride, E) || T < 1 || K < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((!mask && K != 1) || (mask && gate), PTMI_E_INVALID);
    TasWgArgs A{};
    A.g = g;
    A.mask = mask;
    A.gate = gate;
    A.x = x;
    A.ws = workspace;
    A.T = T;
    A.E = E;
    A.N = N;
    A.L = L;
    A.s = stride;
    A.K = K;
    wgrad_plan(N, L, stride, E, &A.tc, &A.xlds);
    const long long chunks = (E + A.tc - 1) / A.tc;
    const long long P = (long long)N * L;
    const long long pblocks = (P + 255) / 256;
    PTMI_RETURN_IF(pblocks > 0x7fffffffLL || chunks > 65535 || B > 65535, PTMI_E_UNSUPPORTED);
    A.nchunks = (int)chunks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)pblocks, (unsigned)chunks, (unsigned)B);
    if (A.xlds)
        hipLaunchKernelGGL(tas_wgrad_kernel<true>, grid, dim3(256), 0, st, A);
    else
        hipLaunchKernelGGL(tas_wgrad_kernel<false>, grid, dim3(256), 0, st, A);
    int rc = launch_status();
    if (rc) return rc;
    const long long width = P + N + 1;
    hipLaunchKernelGGL(tas_wgrad_reduce_kernel, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, st, workspace, out, width,
                       B * chunks);
    return launch_status();
}

}  // extern "C"
