// The convolution blocks of padertorch/contrib/je/modules/conv.py (Conv1d, CNN1d) and the pools of conv_utils.py (Pool1d) on channels-last
// rows: an activation [B, C, T] is held as rows [B T, C] (row b T + t), so every channel product of a layer is ONE planes GEMM over all
// examples, P [B T_in, G K C_out] = x W_taps^T (ops.gemm; G = 2 with a gate convolution), and the kernels here do the rest of a block:
//
//   taps      z[b, t, co] = bias[co] + sum_k P[b, t s + k d - front, k C_out + co], k ascending, rows outside [0, T_in) are zero: stride s,
//             dilation d and the front / end padding are index arithmetic, no padded copy exists.  The same for the gate rows g.  Without
//             a normalisation behind the convolution the epilogue out = act(z) sigmoid(g) + residual is part of this launch.
//   stats     masked column statistics: sum and sum of squares per channel over t < len_b, over (b, t) ("batch") or per example
//             ("sequence"); then mean, rstd, power and count as modules/normalization.normalize defines them (clamped variance, eps).
//   apply     out = act(n) sigmoid(g) + residual, n = gamma (z - mean) rstd + beta, n = 0 behind the length.
//   apply_backward   the two masked column sums (d n, d n xhat) and the PReLU slope's sum, then ONE elementwise pass for dz and dg.
//   dtaps     dP in gather form: dP[b, u, k C_out + co] = dz[b, (u + front - k d) / s, co] where the division is exact and in range.
//   pool      max (int64 indices into the PADDED axis, as nn.MaxPool1d(return_indices=True) behind Pad / Trim gives them) and average
//             pooling, forward and backward (a gather over the windows that hold a position).
//
// Thread map of the elementwise kernels: a thread per (row, V channels), V = 4 (16-byte accesses) when the channel count and every
// leading dimension are multiples of 4 and the pointers are 16-byte aligned, else V = 1; neighbouring lanes on neighbouring channels.
// Sums (reduce.h): a thread adds its rows ascending in fp64, the four row lanes of a workgroup are combined ((0 + 1) + 2) + 3, every
// workgroup writes its slab and colreduce_kernel adds the slabs.  No atomics, no workgroup waits for another, nothing is read on the host.
// Row counts and leading dimensions are 64-bit.
#include "reduce.h"

namespace ptmi {

enum { kActIdentity = 0, kActRelu = 1, kActLeaky = 2, kActElu = 3, kActTanh = 4, kActSigmoid = 5, kActPrelu = 6 };

constexpr int kJcSlabRows = 256;        // rows of one example per workgroup of the column reductions

__device__ __forceinline__ long long jc_len(const void* lengths, int is64, long long b, long long T) {
    if (!lengths) return T;
    const long long n = is64 ? static_cast<const long long*>(lengths)[b] : (long long)static_cast<const int*>(lengths)[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

__device__ __forceinline__ float jc_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

__device__ __forceinline__ float jc_act(float v, int act, float p) {
    switch (act) {
        case kActRelu: return v < 0.f ? 0.f : v;
        case kActLeaky:
        case kActPrelu: return v < 0.f ? p * v : v;
        case kActElu: return v > 0.f ? v : p * expm1f(v);
        case kActTanh: return tanhf(v);
        case kActSigmoid: return jc_sigmoid(v);
        default: return v;
    }
}

// d act / d v at the pre-activation v
__device__ __forceinline__ float jc_dact(float v, int act, float p) {
    switch (act) {
        case kActRelu: return v > 0.f ? 1.f : 0.f;
        case kActLeaky:
        case kActPrelu: return v > 0.f ? 1.f : p;
        case kActElu: return v > 0.f ? 1.f : p * expf(v);
        case kActTanh: {
            const float t = tanhf(v);
            return 1.f - t * t;
        }
        case kActSigmoid: {
            const float s = jc_sigmoid(v);
            return s * (1.f - s);
        }
        default: return 1.f;
    }
}

// What follows the convolution (or, pre_activation, what precedes it): the normalisation's operands and the activation.
struct JcEpilogue {
    const float* __restrict__ stats;        // [groups][4][C]: mean, rstd, power, count; null: no normalisation
    const float* __restrict__ gamma;        // [C] or null (1)
    const float* __restrict__ beta;         // [C] or null (0)
    const void* lengths;                    // [B] or null; only read with stats
    const float* __restrict__ slope;        // the PReLU's one parameter (device), or null
    int is64, per_example, act;
    float act_p;
    long long T;                            // rows per example
    int C;
};

__device__ __forceinline__ float jc_param(const JcEpilogue& E) { return E.slope ? E.slope[0] : E.act_p; }

// n of one element: the normalised value (0 behind the length), or z itself
__device__ __forceinline__ float jc_norm(const JcEpilogue& E, long long b, bool valid, int c, float z, float& xhat) {
    xhat = z;
    if (!E.stats) return z;
    const float* st = E.stats + (E.per_example ? b : 0) * 4 * (long long)E.C;
    xhat = (z - st[c]) * st[E.C + c];
    const float n = (E.gamma ? E.gamma[c] : 1.f) * xhat + (E.beta ? E.beta[c] : 0.f);
    return valid ? n : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- taps (+ epilogue)
struct JcGeom {
    long long B, Tin, Tout, ldP, ldr;
    int Cout, K, stride, dil, front, G;
};

template <int V>
__global__ __launch_bounds__(256) void je_conv_taps_kernel(const float* __restrict__ P, const float* __restrict__ bias,
                                                           const float* __restrict__ gate_bias, const float* __restrict__ residual,
                                                           float* __restrict__ z, float* __restrict__ gz, float* __restrict__ out,
                                                           const JcGeom G, const int act, const float act_p,
                                                           const float* __restrict__ slope) {
    const int CG = G.Cout / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= G.B * G.Tout * CG) return;
    const int c = (int)(i % CG) * V;
    const long long r = i / CG, t = r % G.Tout, b = r / G.Tout;
    float acc[2][V];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (q >= G.G) break;
        const float* bq = q ? gate_bias : bias;
#pragma unroll
        for (int v = 0; v < V; ++v) acc[q][v] = bq ? bq[c + v] : 0.f;
        for (int k = 0; k < G.K; ++k) {
            const long long u = t * G.stride + (long long)k * G.dil - G.front;
            if (u < 0 || u >= G.Tin) continue;
            float p[V];
            load_vec<V>(P + (b * G.Tin + u) * G.ldP + ((long long)q * G.K + k) * G.Cout + c, p);
#pragma unroll
            for (int v = 0; v < V; ++v) acc[q][v] += p[v];
        }
    }
    store_vec<V>(z + r * G.Cout + c, acc[0]);
    if (G.G == 2) store_vec<V>(gz + r * G.Cout + c, acc[1]);
    if (!out) return;
    const float p = slope ? slope[0] : act_p;
    float res[V], o[V];
    if (residual) load_vec<V>(residual + r * G.ldr + c, res);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float a = jc_act(acc[0][v], act, p);
        if (G.G == 2) a *= jc_sigmoid(acc[1][v]);
        o[v] = residual ? a + res[v] : a;
    }
    store_vec<V>(out + r * G.Cout + c, o);
}

// dP [B Tin, G K Cout] from dz / dgz [B Tout, Cout], every element written
template <int V>
__global__ __launch_bounds__(256) void je_conv_dtaps_kernel(const float* __restrict__ dz, const float* __restrict__ dgz,
                                                            float* __restrict__ dP, const JcGeom G) {
    const long long width = (long long)G.G * G.K * G.Cout, WG = width / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= G.B * G.Tin * WG) return;
    const long long col = (i % WG) * V, r = i / WG, u = r % G.Tin, b = r / G.Tin;
    const int co = (int)(col % G.Cout), k = (int)((col / G.Cout) % G.K), q = (int)(col / ((long long)G.K * G.Cout));
    float o[V];
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = 0.f;
    const long long num = u + G.front - (long long)k * G.dil;
    if (num >= 0 && num % G.stride == 0 && num / G.stride < G.Tout)
        load_vec<V>((q ? dgz : dz) + (b * G.Tout + num / G.stride) * G.Cout + co, o);
    store_vec<V>(dP + r * width + col, o);
}

// ---------------------------------------------------------------------------------------------------------------- column reductions
// One element's part in the backward pass.
struct JcPoint {
    float dn, dgz, xhat, slope_term;
};

__device__ __forceinline__ JcPoint jc_point(const JcEpilogue& E, long long b, bool valid, int c, float z, bool has_g, float g, float dout,
                                            float p) {
    JcPoint o;
    const float n = jc_norm(E, b, valid, c, z, o.xhat);
    const float s = has_g ? jc_sigmoid(g) : 1.f;
    o.dn = valid ? dout * s * jc_dact(n, E.act, p) : 0.f;
    o.dgz = has_g ? dout * jc_act(n, E.act, p) * s * (1.f - s) : 0.f;
    o.slope_term = (E.act == kActPrelu && n < 0.f) ? dout * s * n : 0.f;
    return o;
}

// Slab sums of three quantities per column over the rows t < len_b of one chunk of one example.  MODE 0: (x, x^2, 0) of x = z;
// MODE 1: (dn, dn xhat, PReLU slope term).  ws[slab][3][groups][C] with slab = b spe + chunk ("batch": one group) or slab = chunk
// ("sequence": group b).  Grid: (B spe, (C + 63) / 64).
template <int MODE>
__global__ __launch_bounds__(256) void je_conv_reduce_kernel(const float* __restrict__ z, const long long ldz, const float* __restrict__ g,
                                                             const float* __restrict__ dout, const JcEpilogue E, const long long B,
                                                             const long long spe, double* __restrict__ ws) {
    __shared__ double red[4][3][64];
    const int jx = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + jx;
    const long long b = blockIdx.x / spe, chunk = blockIdx.x % spe;
    const long long len = jc_len(E.lengths, E.is64, b, E.T);
    long long end = (chunk + 1) * kJcSlabRows;
    if (end > len) end = len;
    double s0 = 0., s1 = 0., s2 = 0.;
    if (c < E.C) {
        const float p = MODE ? jc_param(E) : 0.f;
        for (long long t = chunk * kJcSlabRows + rg; t < end; t += 4) {
            const long long r = b * E.T + t;
            const float zv = z[r * ldz + c];
            if constexpr (MODE == 0) {
                s0 += (double)zv;
                s1 += (double)zv * (double)zv;
            } else {
                const JcPoint o = jc_point(E, b, true, c, zv, g != nullptr, g ? g[r * E.C + c] : 0.f, dout[r * E.C + c], p);
                s0 += (double)o.dn;
                s1 += (double)o.dn * (double)o.xhat;
                s2 += (double)o.slope_term;
            }
        }
    }
    red[rg][0][jx] = s0, red[rg][1][jx] = s1, red[rg][2][jx] = s2;
    __syncthreads();
    if (rg == 0 && c < E.C) {
        const long long groups = E.per_example ? B : 1;
        const long long slab = E.per_example ? chunk : blockIdx.x, grp = E.per_example ? b : 0;
        double* w = ws + slab * (3 * groups * E.C);
#pragma unroll
        for (int q = 0; q < 3; ++q) w[(q * groups + grp) * E.C + c] = ((red[0][q][jx] + red[1][q][jx]) + red[2][q][jx]) + red[3][q][jx];
    }
}

struct StoreDouble {
    double* __restrict__ out;
    __device__ __forceinline__ void operator()(long long j, double tot) const { out[j] = tot; }
};

// stats [groups][4][C] = mean, rstd, power, count from sums [3][groups][C] (modules/normalization.py: clamped variance, eps inside)
__global__ __launch_bounds__(256) void je_conv_finalize_kernel(const double* __restrict__ sums, const void* lengths, int is64, long long B,
                                                               long long T, int C, int per_example, double eps, float* __restrict__ stats) {
    const long long groups = per_example ? B : 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= groups * C) return;
    const long long grp = i / C;
    const int c = (int)(i % C);
    long long n = 0;
    if (per_example)
        n = jc_len(lengths, is64, grp, T);
    else
        for (long long b = 0; b < B; ++b) n += jc_len(lengths, is64, b, T);
    const double denom = n < 1 ? 1. : (double)n;
    const double mean = sums[grp * C + c] / denom, power = sums[(groups + grp) * C + c] / denom;
    double var = power - mean * mean;
    if (var < 0.) var = 0.;
    float* st = stats + grp * 4 * C;
    st[c] = (float)mean;
    st[C + c] = (float)(1. / sqrt(var + eps));
    st[2 * C + c] = (float)power;
    st[3 * C + c] = (float)n;
}

static int jc_reduce(int mode, const float* z, long long ldz, const float* g, const float* dout, const JcEpilogue& E, long long B,
                     double* ws, double* sums, hipStream_t st) {
    const long long spe = (E.T + kJcSlabRows - 1) / kJcSlabRows, groups = E.per_example ? B : 1;
    PTMI_RETURN_IF(B * spe > 0x7fffffffLL || (E.C + 63) / 64 > 65535, PTMI_E_UNSUPPORTED);
    const dim3 grid((unsigned)(B * spe), (unsigned)((E.C + 63) / 64));
    if (mode == 0)
        hipLaunchKernelGGL((je_conv_reduce_kernel<0>), grid, dim3(256), 0, st, z, ldz, g, dout, E, B, spe, ws);
    else
        hipLaunchKernelGGL((je_conv_reduce_kernel<1>), grid, dim3(256), 0, st, z, ldz, g, dout, E, B, spe, ws);
    int rc = launch_status();
    if (rc) return rc;
    return colreduce(ws, E.per_example ? spe : B * spe, 3 * groups * E.C, StoreDouble{sums}, st);
}

// ---------------------------------------------------------------------------------------------------------------- apply, its backward
template <int V>
__global__ __launch_bounds__(256) void je_conv_apply_kernel(const float* __restrict__ z, const long long ldz, const float* __restrict__ g,
                                                            const float* __restrict__ residual, const long long ldr, const JcEpilogue E,
                                                            const long long B, float* __restrict__ out) {
    const int CG = E.C / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * E.T * CG) return;
    const int c = (int)(i % CG) * V;
    const long long r = i / CG, t = r % E.T, b = r / E.T;
    const bool valid = !(E.stats && E.lengths) || t < jc_len(E.lengths, E.is64, b, E.T);
    const float p = jc_param(E);
    float zv[V], gv[V], res[V], o[V];
    load_vec<V>(z + r * ldz + c, zv);
    if (g) load_vec<V>(g + r * E.C + c, gv);
    if (residual) load_vec<V>(residual + r * ldr + c, res);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        float xhat;
        float a = jc_act(jc_norm(E, b, valid, c + v, zv[v], xhat), E.act, p);
        if (g) a *= jc_sigmoid(gv[v]);
        o[v] = residual ? a + res[v] : a;
    }
    store_vec<V>(out + r * E.C + c, o);
}

// dz = rstd gamma (dn - sum(dn) / n - xhat sum(dn xhat) / n) below the length and 0 behind it (fixed statistics: rstd gamma dn; no
// normalisation: dn), and dgz.
template <int V>
__global__ __launch_bounds__(256) void je_conv_apply_backward_kernel(const float* __restrict__ dout, const float* __restrict__ z,
                                                                     const long long ldz, const float* __restrict__ g, const JcEpilogue E,
                                                                     const long long B, const double* __restrict__ sums, const int fixed,
                                                                     float* __restrict__ dz, float* __restrict__ dgz) {
    const int CG = E.C / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * E.T * CG) return;
    const int c = (int)(i % CG) * V;
    const long long r = i / CG, t = r % E.T, b = r / E.T;
    const bool valid = !(E.stats && E.lengths) || t < jc_len(E.lengths, E.is64, b, E.T);
    const float p = jc_param(E);
    const long long groups = E.per_example ? B : 1, grp = E.per_example ? b : 0;
    float dv[V], zv[V], gv[V], o[V], og[V];
    load_vec<V>(dout + r * E.C + c, dv);
    load_vec<V>(z + r * ldz + c, zv);
    if (g) load_vec<V>(g + r * E.C + c, gv);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const JcPoint q = jc_point(E, b, valid, c + v, zv[v], g != nullptr, g ? gv[v] : 0.f, dv[v], p);
        float d = q.dn;
        if (E.stats) {
            const float* st = E.stats + grp * 4 * (long long)E.C;
            const float scale = st[E.C + c + v] * (E.gamma ? E.gamma[c + v] : 1.f);
            if (fixed) {
                d = scale * q.dn;
            } else {
                const double n = st[3 * E.C + c + v] < 1.f ? 1. : (double)st[3 * E.C + c + v];
                const float m1 = (float)(sums[grp * E.C + c + v] / n), m2 = (float)(sums[(groups + grp) * E.C + c + v] / n);
                d = valid ? scale * (q.dn - m1 - q.xhat * m2) : 0.f;
            }
        }
        o[v] = d, og[v] = q.dgz;
    }
    store_vec<V>(dz + r * E.C + c, o);
    if (g) store_vec<V>(dgz + r * E.C + c, og);
}

// ---------------------------------------------------------------------------------------------------------------- pools
struct JcPool {
    long long B, Tin, Tout, ldx;
    int C, size, stride, front;
};

// the padded axis holds zeros in front of and behind the Tin values
template <bool MAX>
__global__ __launch_bounds__(256) void je_pool_forward_kernel(const float* __restrict__ x, const JcPool G, float* __restrict__ y,
                                                              long long* __restrict__ index) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= G.B * G.Tout * G.C) return;
    const int c = (int)(i % G.C);
    const long long r = i / G.C, j = r % G.Tout, b = r / G.Tout;
    float best = -INFINITY, sum = 0.f;
    long long at = j * G.stride;
    for (int k = 0; k < G.size; ++k) {
        const long long p = j * G.stride + k, u = p - G.front;
        const float v = (u >= 0 && u < G.Tin) ? x[(b * G.Tin + u) * G.ldx + c] : 0.f;
        if constexpr (MAX) {
            if (v > best || v != v) best = v, at = p;        // the first of equal values; a NaN beats every number (nn.MaxPool1d)
        } else {
            sum += v;
        }
    }
    if constexpr (MAX) {
        y[i] = best;
        index[i] = at;
    } else {
        y[i] = sum / (float)G.size;
    }
}

// dx [B Tin, C] contiguous, every element written: the windows j with j stride <= p < j stride + size, ascending
template <bool MAX>
__global__ __launch_bounds__(256) void je_pool_backward_kernel(const float* __restrict__ dy, const long long* __restrict__ index,
                                                               const JcPool G, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= G.B * G.Tin * G.C) return;
    const int c = (int)(i % G.C);
    const long long r = i / G.C, u = r % G.Tin, b = r / G.Tin;
    const long long p = u + G.front;
    long long lo = p - G.size + 1;
    lo = lo <= 0 ? 0 : (lo + G.stride - 1) / G.stride;
    long long hi = p / G.stride;
    if (hi > G.Tout - 1) hi = G.Tout - 1;
    float s = 0.f;
    for (long long j = lo; j <= hi; ++j) {
        const long long o = (b * G.Tout + j) * G.C + c;
        if constexpr (MAX) {
            if (index[o] == p) s += dy[o];
        } else {
            s += dy[o] / (float)G.size;
        }
    }
    dx[i] = s;
}

static bool jc_geom(const int64_t* g, JcGeom& G) {
    if (!g) return false;
    G.B = g[0], G.Tin = g[1], G.Tout = g[2], G.Cout = (int)g[3], G.K = (int)g[4], G.stride = (int)g[5], G.dil = (int)g[6];
    G.front = (int)g[7], G.G = (int)g[8], G.ldP = g[9], G.ldr = g[10];
    return G.B >= 1 && G.Tin >= 1 && G.Tout >= 1 && g[3] >= 1 && g[3] <= 0x3fffffff && g[4] >= 1 && g[4] <= 4096 && g[5] >= 1 &&
           g[5] <= 0x3fffffff && g[6] >= 1 && g[6] <= 0x3fffffff && g[7] >= 0 && g[7] <= 0x3fffffff && (G.G == 1 || G.G == 2) &&
           G.ldP >= (long long)G.G * G.K * G.Cout && G.ldr >= G.Cout &&
           // the last window ends inside the padded axis: (Tout - 1) s + (K - 1) d - front is a row of the input or of its end pad
           (G.Tout - 1) * G.stride - G.front < G.Tin;
}

static bool jc_blocks(long long threads, unsigned& blocks) {
    const long long n = (threads + 255) / 256;
    if (n < 1 || n > 0x7fffffffLL) return false;
    blocks = (unsigned)n;
    return true;
}

static JcEpilogue jc_epilogue(const float* stats, const float* gamma, const float* beta, const void* lengths, int32_t is64,
                              const float* slope, int32_t per_example, int32_t act, float act_p, int64_t T, int64_t C) {
    JcEpilogue E;
    E.stats = stats, E.gamma = stats ? gamma : nullptr, E.beta = stats ? beta : nullptr, E.lengths = stats ? lengths : nullptr;
    E.slope = act == kActPrelu ? slope : nullptr;
    E.is64 = is64, E.per_example = stats ? per_example : 0, E.act = act, E.act_p = act_p, E.T = T, E.C = (int)C;
    return E;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_je_conv_workspace_elems(int64_t B, int64_t T, int64_t C) {
    if (B < 1 || T < 1 || C < 1) return 0;
    return B * ((T + kJcSlabRows - 1) / kJcSlabRows) * 3 * C;
}

int ptmi_je_conv_taps(const float* P, const float* bias, const float* gate_bias, const float* residual, const float* slope, float* z,
                      float* gz, float* out, const int64_t* geom, int32_t act, float act_p, ptmi_stream_t stream) {
    JcGeom G;
    PTMI_RETURN_IF(!P || !z || !jc_geom(geom, G) || (G.G == 2 && !gz) || act < kActIdentity || act > kActPrelu, PTMI_E_INVALID);
    PTMI_RETURN_IF(act == kActPrelu && out && !slope, PTMI_E_INVALID);
    const bool vec = G.Cout % 4 == 0 && G.ldP % 4 == 0 && (!residual || G.ldr % 4 == 0) &&
                     aligned16({P, bias, gate_bias, residual, z, gz, out});
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks(G.B * G.Tout * (G.Cout / (vec ? 4 : 1)), blocks), PTMI_E_UNSUPPORTED);
    PTMI_LAUNCH_VEC(je_conv_taps_kernel, vec, dim3(blocks), static_cast<hipStream_t>(stream), P, bias, gate_bias, residual, z, gz, out, G,
                    act, act_p, act == kActPrelu ? slope : nullptr);
    return launch_status();
}

int ptmi_je_conv_dtaps(const float* dz, const float* dgz, float* dP, const int64_t* geom, ptmi_stream_t stream) {
    JcGeom G;
    PTMI_RETURN_IF(!dz || !dP || !jc_geom(geom, G) || (G.G == 2 && !dgz), PTMI_E_INVALID);
    const bool vec = G.Cout % 4 == 0 && aligned16({dz, dgz, dP});
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks(G.B * G.Tin * ((long long)G.G * G.K * G.Cout / (vec ? 4 : 1)), blocks), PTMI_E_UNSUPPORTED);
    PTMI_LAUNCH_VEC(je_conv_dtaps_kernel, vec, dim3(blocks), static_cast<hipStream_t>(stream), dz, dgz, dP, G);
    return launch_status();
}

int ptmi_je_conv_stats(const float* x, int64_t ldx, const void* lengths, int32_t lengths_int64, int64_t B, int64_t T, int64_t C,
                       int32_t per_example, float eps, double* workspace, double* sums, float* stats, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !workspace || !sums || !stats || B < 1 || T < 1 || C < 1 || C > 0x3fffffff || ldx < C, PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    JcEpilogue E = jc_epilogue(nullptr, nullptr, nullptr, nullptr, lengths_int64, nullptr, per_example, kActIdentity, 0.f, T, C);
    E.lengths = lengths, E.per_example = per_example;
    int rc = jc_reduce(0, x, ldx, nullptr, nullptr, E, B, workspace, sums, st);
    if (rc) return rc;
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks((per_example ? B : 1) * C, blocks), PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(je_conv_finalize_kernel, dim3(blocks), dim3(256), 0, st, sums, lengths, lengths_int64, (long long)B, (long long)T,
                       (int)C, per_example, (double)eps, stats);
    return launch_status();
}

int ptmi_je_conv_apply(const float* z, int64_t ldz, const float* g, const float* residual, int64_t ldr, const float* stats,
                       const float* gamma, const float* beta, const void* lengths, int32_t lengths_int64, const float* slope, float* out,
                       int64_t B, int64_t T, int64_t C, int32_t per_example, int32_t act, float act_p, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!z || !out || B < 1 || T < 1 || C < 1 || C > 0x3fffffff || ldz < C || (residual && ldr < C), PTMI_E_INVALID);
    PTMI_RETURN_IF(act < kActIdentity || act > kActPrelu || (act == kActPrelu && !slope), PTMI_E_INVALID);
    const JcEpilogue E = jc_epilogue(stats, gamma, beta, lengths, lengths_int64, slope, per_example, act, act_p, T, C);
    const bool vec = C % 4 == 0 && ldz % 4 == 0 && (!residual || ldr % 4 == 0) && aligned16({z, g, residual, out});
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks(B * T * (C / (vec ? 4 : 1)), blocks), PTMI_E_UNSUPPORTED);
    PTMI_LAUNCH_VEC(je_conv_apply_kernel, vec, dim3(blocks), static_cast<hipStream_t>(stream), z, (long long)ldz, g, residual,
                    (long long)ldr, E, (long long)B, out);
    return launch_status();
}

int ptmi_je_conv_apply_backward(const float* dout, const float* z, int64_t ldz, const float* g, const float* stats, const float* gamma,
                                const float* beta, const void* lengths, int32_t lengths_int64, const float* slope, float* dz, float* dgz,
                                float* dparams, double* workspace, double* sums, int64_t B, int64_t T, int64_t C, int32_t per_example,
                                int32_t fixed_stats, int32_t act, float act_p, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dout || !z || !dz || (g && !dgz) || B < 1 || T < 1 || C < 1 || C > 0x3fffffff || ldz < C, PTMI_E_INVALID);
    PTMI_RETURN_IF(act < kActIdentity || act > kActPrelu || (act == kActPrelu && !slope), PTMI_E_INVALID);
    const JcEpilogue E = jc_epilogue(stats, gamma, beta, lengths, lengths_int64, slope, per_example, act, act_p, T, C);
    const bool sums_needed = (stats && !fixed_stats) || dparams;
    PTMI_RETURN_IF(sums_needed && (!workspace || !sums), PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    if (sums_needed) {
        rc = jc_reduce(1, z, ldz, g, dout, E, B, workspace, sums, st);
        if (rc) return rc;
    }
    const bool vec = C % 4 == 0 && ldz % 4 == 0 && aligned16({dout, z, g, dz, dgz});
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks(B * T * (C / (vec ? 4 : 1)), blocks), PTMI_E_UNSUPPORTED);
    PTMI_LAUNCH_VEC(je_conv_apply_backward_kernel, vec, dim3(blocks), st, dout, z, (long long)ldz, g, E, (long long)B, sums, fixed_stats,
                    dz, dgz);
    rc = launch_status();
    if (rc || !dparams) return rc;
    // dparams [2 C + 1] = d gamma | d beta | d slope: the groups' sums in order
    const long long groups = E.per_example ? B : 1;
    rc = colreduce(sums + groups * C, groups, C, StorePlain{dparams}, st);
    if (rc) return rc;
    rc = colreduce(sums, groups, C, StorePlain{dparams + C}, st);
    if (rc) return rc;
    return colreduce(sums + 2 * groups * C, groups * C, 1, StorePlain{dparams + 2 * C}, st);
}

static bool jc_pool(const int64_t* g, JcPool& G) {
    if (!g) return false;
    G.B = g[0], G.Tin = g[1], G.Tout = g[2], G.C = (int)g[3], G.size = (int)g[4], G.stride = (int)g[5], G.front = (int)g[6], G.ldx = g[7];
    return G.B >= 1 && G.Tin >= 1 && G.Tout >= 1 && g[3] >= 1 && g[3] <= 0x3fffffff && g[4] >= 1 && g[4] <= 0x3fffffff && g[5] >= 1 &&
           g[5] <= 0x3fffffff && g[6] >= 0 && g[6] <= 0x3fffffff && G.ldx >= G.C && (G.Tout - 1) * G.stride - G.front < G.Tin;
}

int ptmi_je_pool_forward(const float* x, float* y, int64_t* index, const int64_t* geom, int32_t max_pool, ptmi_stream_t stream) {
    JcPool G;
    PTMI_RETURN_IF(!x || !y || !jc_pool(geom, G) || (max_pool && !index), PTMI_E_INVALID);
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks(G.B * G.Tout * G.C, blocks), PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (max_pool)
        hipLaunchKernelGGL((je_pool_forward_kernel<true>), dim3(blocks), dim3(256), 0, st, x, G, y, reinterpret_cast<long long*>(index));
    else
        hipLaunchKernelGGL((je_pool_forward_kernel<false>), dim3(blocks), dim3(256), 0, st, x, G, y, static_cast<long long*>(nullptr));
    return launch_status();
}

int ptmi_je_pool_backward(const float* dy, const int64_t* index, float* dx, const int64_t* geom, int32_t max_pool, ptmi_stream_t stream) {
    JcPool G;
    PTMI_RETURN_IF(!dy || !dx || !jc_pool(geom, G) || (max_pool && !index), PTMI_E_INVALID);
    unsigned blocks;
    PTMI_RETURN_IF(!jc_blocks(G.B * G.Tin * G.C, blocks), PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (max_pool)
        hipLaunchKernelGGL((je_pool_backward_kernel<true>), dim3(blocks), dim3(256), 0, st, dy, reinterpret_cast<const long long*>(index), G,
                           dx);
    else
        hipLaunchKernelGGL((je_pool_backward_kernel<false>), dim3(blocks), dim3(256), 0, st, dy, static_cast<const long long*>(nullptr), G,
                           dx);
    return launch_status();
}

}  // extern "C"
