// The non-GEMM part of a Conv-TasNet block (padertorch/modules/convnet.py:114-161: _Conv1DBlock = norm, 1x1 conv, PReLU, pad,
// depthwise dilated conv, PReLU, norm, 1x1 conv, residual; norms of padertorch/contrib/jensheit/norm.py:10-70), forward and backward.
//
// Layout: every activation is [B, T, C] contiguous fp32, CHANNELS INNERMOST: lanes run along channels (coalesced, 16 B per lane when
// C % 4 == 0 and the pointers allow it), a depthwise tap at t + k d is a whole-row offset, cLN is a row norm, gLN a norm per example.
//
// Workgroup = 256 threads = 4 waves; a wave is 64 channel groups (of V = 4 or 1 channels) wide and owns 16 of the workgroup's 64 rows.
//   depthwise forward   v = prelu_a2(bias[h] + sum_k w[h,k] p[t + k d - front, h]), p = prelu_a1(u), p = 0 outside [0, T): p and the
//                       second pre-activation live in registers only; the launch leaves per-workgroup sums of v and v^2 behind, a
//                       second kernel turns them into the gLN (mean, rstd) of every example.
//   depthwise backward  kernel Z recomputes the pre-activation z from u, writes gz = gv prelu_a2'(z) and the partial sums of
//                       d weight[h,k], d bias[h], d a2; kernel U gathers gu = prelu_a1'(u) sum_k w[h,k] gz[t - k d + front] and the
//                       partial sums of d a1.
//   channel norm        statistics (per example: partial sums + finalize; per row: one wave per row), apply, and backward (per-channel
//                       and per-group partial sums, finalize, dx).
// Sums: per-thread, per-workgroup and final accumulators are fp64; no atomics; partials are added in the fixed order that reduce.h
// defines (rows ascending inside a thread): results are bit-reproducible.  No allocation, no synchronisation: capturable.
#include <algorithm>

#include "reduce.h"

namespace ptmi {

constexpr int kTcnRows = 64;              // rows per workgroup
constexpr int kTcnR = kTcnRows / 4;       // rows per thread
constexpr int kTcnChunk = 8192;           // elements per workgroup of the per-example statistics pass

// Per-channel sums of the workgroup: the four waves' values of column cx * V + e, added in wave order by wave 0.
template <int V>
__device__ __forceinline__ void tcn_wave_columns(const double (&acc)[V], bool live, double* __restrict__ out) {
    __shared__ double cols[4][64 * V];
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < V; ++e) cols[ty][cx * V + e] = acc[e];
    __syncthreads();
    if (ty == 0 && live) {
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = ((cols[0][cx * V + e] + cols[1][cx * V + e]) + cols[2][cx * V + e]) + cols[3][cx * V + e];
    }
}

struct TcnDwArgs {
    const float* u;        // [B, T, H]
    const float* a1;       // [1] slope in front of the taps
    const float* w;        // [H, K]
    const float* bias;     // [H] or null
    const float* a2;       // [1] slope behind them
    const float* gv;       // [B, T, H]  (backward)
    float* v;              // [B, T, H]  (forward)
    float* gz;             // [B, T, H]  (backward: written by Z, read by U)
    float* gu;             // [B, T, H]  (backward)
    double* wcol;          // [B tiles][(K + 1) H] per-channel partial sums (backward)
    double* wsca;          // [B tiles cblocks][2] scalar partial sums
    long long T;
    int H, K, d, front;
};

// z[i][e] = bias + sum_k w[k] prelu_a1(u[t0 + i + k d - front]) for the thread's kTcnR rows (k ascending)
template <int V>
__device__ __forceinline__ void tcn_preactivation(const TcnDwArgs& A, const float* __restrict__ ub, int c0, long long t0, float a1,
                                                  float (&z)[kTcnR][V]) {
    float bv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) bv[e] = A.bias ? A.bias[c0 + e] : 0.f;
#pragma unroll
    for (int i = 0; i < kTcnR; ++i)
#pragma unroll
        for (int e = 0; e < V; ++e) z[i][e] = bv[e];
    for (int k = 0; k < A.K; ++k) {
        float wv[V];
#pragma unroll
        for (int e = 0; e < V; ++e) wv[e] = A.w[(long long)(c0 + e) * A.K + k];
        const long long off = (long long)k * A.d - A.front;
#pragma unroll
        for (int i = 0; i < kTcnR; ++i) {
            const long long s = t0 + i + off;
            if (t0 + i < A.T && s >= 0 && s < A.T) {
                float x[V];
                load_vec<V>(ub + s * A.H, x);
#pragma unroll
                for (int e = 0; e < V; ++e) z[i][e] = fmaf(wv[e], x[e] > 0.f ? x[e] : a1 * x[e], z[i][e]);
            }
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void tcn_dw_forward_kernel(const TcnDwArgs A) {
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = (blockIdx.y * 64 + cx) * V;
    const bool live = c0 < A.H;
    const long long b = blockIdx.z;
    const long long t0 = (long long)blockIdx.x * kTcnRows + ty * kTcnR;
    const float a1 = A.a1[0], a2 = A.a2[0];
    double s[2] = {0., 0.};
    if (live && t0 < A.T) {
        const float* __restrict__ ub = A.u + b * A.T * A.H + c0;
        float* __restrict__ vb = A.v + b * A.T * A.H + c0;
        float z[kTcnR][V];
        tcn_preactivation<V>(A, ub, c0, t0, a1, z);
#pragma unroll
        for (int i = 0; i < kTcnR; ++i) {
            if (t0 + i < A.T) {
                float o[V];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    o[e] = z[i][e] > 0.f ? z[i][e] : a2 * z[i][e];
                    s[0] += (double)o[e];
                    s[1] += (double)o[e] * (double)o[e];
                }
                store_vec<V>(vb + (t0 + i) * A.H, o);
            }
        }
    }
    block_sums<2>(s);
    if (threadIdx.x < 2) A.wsca[(((long long)b * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * 2 + threadIdx.x] = s[threadIdx.x];
}

template <int V>
__global__ __launch_bounds__(256) void tcn_dw_backward_z_kernel(const TcnDwArgs A) {
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = (blockIdx.y * 64 + cx) * V;
    const bool live = c0 < A.H;
    const long long b = blockIdx.z;
    const long long t0 = (long long)blockIdx.x * kTcnRows + ty * kTcnR;
    const float a1 = A.a1[0], a2 = A.a2[0];
    const float* __restrict__ ub = A.u + b * A.T * A.H + c0;
    double* __restrict__ col = A.wcol + ((long long)b * gridDim.x + blockIdx.x) * (long long)(A.K + 1) * A.H + c0;
    float z[kTcnR][V];          // becomes gz
    double s[1] = {0.};         // d a2
    double db[V];
#pragma unroll
    for (int e = 0; e < V; ++e) db[e] = 0.;
    const bool work = live && t0 < A.T;
    if (work) {
        tcn_preactivation<V>(A, ub, c0, t0, a1, z);
#pragma unroll
        for (int i = 0; i < kTcnR; ++i) {
            if (t0 + i < A.T) {
                float g[V];
                load_vec<V>(A.gv + (b * A.T + t0 + i) * A.H + c0, g);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float zz = z[i][e];
                    s[0] += zz > 0.f ? 0. : (double)g[e] * (double)zz;
                    z[i][e] = zz > 0.f ? g[e] : a2 * g[e];
                    db[e] += (double)z[i][e];
                }
                store_vec<V>(A.gz + (b * A.T + t0 + i) * A.H + c0, z[i]);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) z[i][e] = 0.f;
            }
        }
    }
    for (int k = 0; k < A.K; ++k) {
        double acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.;
        if (work) {
            const long long off = (long long)k * A.d - A.front;
#pragma unroll
            for (int i = 0; i < kTcnR; ++i) {
                const long long r = t0 + i + off;
                if (t0 + i < A.T && r >= 0 && r < A.T) {
                    float x[V];
                    load_vec<V>(ub + r * A.H, x);
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] += (double)z[i][e] * (double)(x[e] > 0.f ? x[e] : a1 * x[e]);
                }
            }
        }
        tcn_wave_columns<V>(acc, live, col + (long long)k * A.H);
    }
    tcn_wave_columns<V>(db, live, col + (long long)A.K * A.H);
    block_sums<1>(s);
    if (threadIdx.x == 0) A.wsca[(((long long)b * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * 2 + 1] = s[0];
}

template <int V>
__global__ __launch_bounds__(256) void tcn_dw_backward_u_kernel(const TcnDwArgs A) {
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = (blockIdx.y * 64 + cx) * V;
    const bool live = c0 < A.H;
    const long long b = blockIdx.z;
    const long long t0 = (long long)blockIdx.x * kTcnRows + ty * kTcnR;
    const float a1 = A.a1[0];
    double s[1] = {0.};         // d a1
    if (live && t0 < A.T) {
        const float* __restrict__ gzb = A.gz + b * A.T * A.H + c0;
        float gp[kTcnR][V];
#pragma unroll
        for (int i = 0; i < kTcnR; ++i)
#pragma unroll
            for (int e = 0; e < V; ++e) gp[i][e] = 0.f;
        for (int k = 0; k < A.K; ++k) {
            float wv[V];
#pragma unroll
            for (int e = 0; e < V; ++e) wv[e] = A.w[(long long)(c0 + e) * A.K + k];
            const long long off = A.front - (long long)k * A.d;
#pragma unroll
            for (int i = 0; i < kTcnR; ++i) {
                const long long r = t0 + i + off;
                if (t0 + i < A.T && r >= 0 && r < A.T) {
                    float g[V];
                    load_vec<V>(gzb + r * A.H, g);
#pragma unroll
                    for (int e = 0; e < V; ++e) gp[i][e] = fmaf(wv[e], g[e], gp[i][e]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kTcnR; ++i) {
            if (t0 + i < A.T) {
                float x[V], o[V];
                load_vec<V>(A.u + (b * A.T + t0 + i) * A.H + c0, x);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    o[e] = x[e] > 0.f ? gp[i][e] : a1 * gp[i][e];
                    s[0] += x[e] > 0.f ? 0. : (double)gp[i][e] * (double)x[e];
                }
                store_vec<V>(A.gu + (b * A.T + t0 + i) * A.H + c0, o);
            }
        }
    }
    block_sums<1>(s);
    if (threadIdx.x == 0) A.wsca[(((long long)b * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * 2] = s[0];
}

// One workgroup per group g: (s1, s2) = sum of the group's `slabs` partial pairs (thread-strided, ascending, then the workgroup sum).
// mode 0: out[g] = (mean, rstd) = (s1 / count, 1 / sqrt(s2 / count - mean^2 + eps));  mode 1: out[g] = (s1, s2) / count.
__global__ __launch_bounds__(256) void tcn_group_finalize_kernel(const double* __restrict__ ws, long long slabs, double count, float eps,
                                                                 int mode, float* __restrict__ out) {
    const double* __restrict__ p = ws + (long long)blockIdx.x * slabs * 2;
    double s[2] = {0., 0.};
    for (long long i = threadIdx.x; i < slabs; i += 256) {
        s[0] += p[2 * i];
        s[1] += p[2 * i + 1];
    }
    block_sums<2>(s);
    if (threadIdx.x == 0) {
        const double m = s[0] / count;
        if (mode == 0) {
            const double var = fmax(s[1] / count - m * m, 0.);
            out[2 * blockIdx.x] = (float)m;
            out[2 * blockIdx.x + 1] = (float)(1. / sqrt(var + (double)eps));
        } else {
            out[2 * blockIdx.x] = (float)m;
            out[2 * blockIdx.x + 1] = (float)(s[1] / count);
        }
    }
}

struct TcnNormArgs {
    const float* x;        // [B, T, C]
    const float* gy;       // [B, T, C]  (backward)
    const float* stats;    // [G, 2] (mean, rstd)
    const float* gsum;     // [G, 2] (mean of gy gamma, mean of gy gamma xhat)  (dx)
    const float* gamma;    // [C]
    const float* beta;     // [C]
    float* y;              // [B, T, C]: the output, or dx
    double* wcol;          // [B tiles][2 C]
    double* wsca;          // [B tiles cblocks][2]
    long long T;
    int C, rows;           // rows != 0: a group is a row (cLN); else an example (gLN)
};

// Per-example partial sums of x and x^2 over the flattened [T C] range: workgroup (chunk, b).
template <int V>
__global__ __launch_bounds__(256) void tcn_norm_stats_example_kernel(const float* __restrict__ x, long long n, double* __restrict__ ws) {
    const float* __restrict__ xb = x + (long long)blockIdx.y * n;
    const long long i0 = (long long)blockIdx.x * kTcnChunk;
    const long long i1 = min(i0 + kTcnChunk, n);
    double s[2] = {0., 0.};
    for (long long i = i0 + (long long)threadIdx.x * V; i < i1; i += 256 * V) {
        float v[V];
        load_vec<V>(xb + i, v);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            s[0] += (double)v[e];
            s[1] += (double)v[e] * (double)v[e];
        }
    }
    block_sums<2>(s);
    if (threadIdx.x < 2) ws[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = s[threadIdx.x];
}

// One wave per row.  mode 0: out[row] = (mean, rstd) of x;  mode 1: out[row] = (mean of gy gamma, mean of gy gamma xhat).
template <int V>
__global__ __launch_bounds__(256) void tcn_norm_row_kernel(const TcnNormArgs A, long long nrows, float eps, int mode, float* __restrict__ out) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;           // wave-uniform; no workgroup barrier below
    const int lane = threadIdx.x & 63;
    float m = 0.f, rs = 0.f;
    if (mode == 1) m = A.stats[2 * row], rs = A.stats[2 * row + 1];
    double s1 = 0., s2 = 0.;
    for (int c = lane * V; c < A.C; c += 64 * V) {
        float v[V];
        load_vec<V>(A.x + row * A.C + c, v);
        if (mode == 0) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                s1 += (double)v[e];
                s2 += (double)v[e] * (double)v[e];
            }
        } else {
            float g[V], ga[V];
            load_vec<V>(A.gy + row * A.C + c, g);
            load_vec<V>(A.gamma + c, ga);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float gx = g[e] * ga[e];
                s1 += (double)gx;
                s2 += (double)gx * (double)((v[e] - m) * rs);
            }
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        const double mean = s1 / A.C;
        if (mode == 0) {
            const double var = fmax(s2 / A.C - mean * mean, 0.);
            out[2 * row] = (float)mean;
            out[2 * row + 1] = (float)(1. / sqrt(var + (double)eps));
        } else {
            out[2 * row] = (float)mean;
            out[2 * row + 1] = (float)(s2 / A.C);
        }
    }
}

// mode 0: y = gamma (x - mean) rstd + beta;  mode 1 (dx): y = rstd (gy gamma - gsum[0] - xhat gsum[1])
// Contraction is off and the fused multiply-adds are written out: left to the compiler, <4> fused some of its packed lanes and not
// others, so dx differed in its last bit between <1> and <4> and between neighbouring channels.  gy gamma is rounded before gsum[0] is
// taken off, as it was rounded before it went into that mean: fused, a group of one element got the product's rounding residual
// times rstd for its dx instead of 0.
template <int V>
__global__ __launch_bounds__(256) void tcn_norm_pointwise_kernel(const TcnNormArgs A, int mode) {
#pragma clang fp contract(off)
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = (blockIdx.y * 64 + cx) * V;
    if (c0 >= A.C) return;              // no barrier in this kernel
    const long long b = blockIdx.z;
    const long long t0 = (long long)blockIdx.x * kTcnRows + ty * kTcnR;
    float ga[V], be[V];
    load_vec<V>(A.gamma + c0, ga);
    if (mode == 0) load_vec<V>(A.beta + c0, be);
#pragma unroll 4
    for (int i = 0; i < kTcnR; ++i) {
        if (t0 + i >= A.T) break;
        const long long row = b * A.T + t0 + i;
        const long long g = A.rows ? row : b;
        const float m = A.stats[2 * g], rs = A.stats[2 * g + 1];
        float x[V], o[V];
        load_vec<V>(A.x + row * A.C + c0, x);
        if (mode == 0) {
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = fmaf(ga[e], (x[e] - m) * rs, be[e]);
        } else {
            const float g1 = A.gsum[2 * g], g2 = A.gsum[2 * g + 1];
            float gy[V];
            load_vec<V>(A.gy + row * A.C + c0, gy);
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = rs * fmaf(-((x[e] - m) * rs), g2, gy[e] * ga[e] - g1);
        }
        store_vec<V>(A.y + row * A.C + c0, o);
    }
}

// Partial sums of the backward pass: d gamma[c] = sum gy xhat, d beta[c] = sum gy per channel, and per workgroup
// (sum gy gamma, sum gy gamma xhat) for the per-example group sums.
template <int V>
__global__ __launch_bounds__(256) void tcn_norm_backward_reduce_kernel(const TcnNormArgs A) {
    const int cx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c0 = (blockIdx.y * 64 + cx) * V;
    const bool live = c0 < A.C;
    const long long b = blockIdx.z;
    const long long t0 = (long long)blockIdx.x * kTcnRows + ty * kTcnR;
    double dg[V], db[V], s[2] = {0., 0.};
#pragma unroll
    for (int e = 0; e < V; ++e) dg[e] = db[e] = 0.;
    if (live) {
        float ga[V];
        load_vec<V>(A.gamma + c0, ga);
#pragma unroll 4
        for (int i = 0; i < kTcnR; ++i) {
            if (t0 + i >= A.T) break;
            const long long row = b * A.T + t0 + i;
            const long long g = A.rows ? row : b;
            const float m = A.stats[2 * g], rs = A.stats[2 * g + 1];
            float x[V], gy[V];
            load_vec<V>(A.x + row * A.C + c0, x);
            load_vec<V>(A.gy + row * A.C + c0, gy);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float xh = (x[e] - m) * rs;
                const float gx = gy[e] * ga[e];
                dg[e] += (double)gy[e] * (double)xh;
                db[e] += (double)gy[e];
                s[0] += (double)gx;
                s[1] += (double)gx * (double)xh;
            }
        }
    }
    double* __restrict__ col = A.wcol + ((long long)b * gridDim.x + blockIdx.x) * 2 * (long long)A.C + c0;
    tcn_wave_columns<V>(dg, live, col);
    tcn_wave_columns<V>(db, live, col + A.C);
    block_sums<2>(s);
    if (threadIdx.x < 2) A.wsca[(((long long)b * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y) * 2 + threadIdx.x] = s[threadIdx.x];
}

struct TcnGrid {
    long long tiles, cblocks;
    dim3 grid;
    bool ok;
};

static TcnGrid tcn_grid(int64_t B, int64_t T, int32_t C, int V) {
    TcnGrid g;
    g.tiles = (T + kTcnRows - 1) / kTcnRows;
    g.cblocks = ((C + V - 1) / V + 63) / 64;
    g.ok = g.tiles <= 0x7fffffffLL && g.cblocks <= 65535 && B <= 65535;
    g.grid = dim3((unsigned)g.tiles, (unsigned)g.cblocks, (unsigned)B);
    return g;
}

static long long tcn_scalar_slabs(int64_t B, int64_t T, int32_t C) {
    return B * ((T + kTcnRows - 1) / kTcnRows) * ((C + 63) / 64);          // V = 1: the most channel blocks a launch can have
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_tcn_depthwise_workspace_elems(int64_t B, int64_t T, int32_t H, int32_t K) {
    if (B < 1 || T < 1 || H < 1 || K < 1) return PTMI_E_INVALID;
    const long long tiles = (T + kTcnRows - 1) / kTcnRows;
    return B * tiles * (long long)(K + 1) * H + 2 * tcn_scalar_slabs(B, T, H);
}

int ptmi_tcn_depthwise_forward(const float* u, const float* slope_in, const float* weight, const float* bias, const float* slope_out,
                               float* v, float* stats, double* workspace, int64_t B, int64_t T, int32_t H, int32_t K,
                               int32_t dilation, float eps, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!u || !slope_in || !weight || !slope_out || !v || !stats || !workspace, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || T < 1 || H < 1 || K < 1 || dilation < 1, PTMI_E_INVALID);
    const bool vec = H % 4 == 0 && aligned16({u, v});
    const TcnGrid g = tcn_grid(B, T, H, vec ? 4 : 1);
    PTMI_RETURN_IF(!g.ok, PTMI_E_UNSUPPORTED);
    TcnDwArgs A{};
    A.u = u, A.a1 = slope_in, A.w = weight, A.bias = bias, A.a2 = slope_out, A.v = v;
    A.wsca = workspace;
    A.T = T, A.H = H, A.K = K, A.d = dilation;
    A.front = (int)(((long long)dilation * (K - 1)) / 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    PTMI_LAUNCH_VEC(tcn_dw_forward_kernel, vec, g.grid, st, A);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(tcn_group_finalize_kernel, dim3((unsigned)B), dim3(256), 0, st, workspace, g.tiles * g.cblocks,
                       (double)T * (double)H, eps, 0, stats);
    return launch_status();
}

int ptmi_tcn_depthwise_backward(const float* gv, const float* u, const float* slope_in, const float* weight, const float* bias,
                                const float* slope_out, float* gz, float* gu, float* dparams, double* workspace, int64_t B,
                                int64_t T, int32_t H, int32_t K, int32_t dilation, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gv || !u || !slope_in || !weight || !slope_out || !gz || !gu || !dparams || !workspace, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || T < 1 || H < 1 || K < 1 || dilation < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((long long)(K + 1) * H > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    const bool vec = H % 4 == 0 && aligned16({gv, u, gz, gu});
    const TcnGrid g = tcn_grid(B, T, H, vec ? 4 : 1);
    PTMI_RETURN_IF(!g.ok, PTMI_E_UNSUPPORTED);
    const long long width = (long long)(K + 1) * H;
    TcnDwArgs A{};
    A.u = u, A.a1 = slope_in, A.w = weight, A.bias = bias, A.a2 = slope_out, A.gv = gv, A.gz = gz, A.gu = gu;
    A.wcol = workspace;
    A.wsca = workspace + B * g.tiles * width;
    A.T = T, A.H = H, A.K = K, A.d = dilation;
    A.front = (int)(((long long)dilation * (K - 1)) / 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    PTMI_LAUNCH_VEC(tcn_dw_backward_z_kernel, vec, g.grid, st, A);
    if ((rc = launch_status())) return rc;
    PTMI_LAUNCH_VEC(tcn_dw_backward_u_kernel, vec, g.grid, st, A);
    if ((rc = launch_status())) return rc;
    if ((rc = colreduce(A.wcol, B * g.tiles, width, StoreDepthwise{dparams, H, K}, st))) return rc;
    return colreduce(A.wsca, B * g.tiles * g.cblocks, 2LL, StoreDepthwise{dparams + width, 0, 0}, st);
}

int64_t ptmi_tcn_norm_workspace_elems(int64_t B, int64_t T, int32_t C) {
    if (B < 1 || T < 1 || C < 1) return PTMI_E_INVALID;
    const long long tiles = (T + kTcnRows - 1) / kTcnRows;
    const long long chunks = (T * C + kTcnChunk - 1) / kTcnChunk;
    return std::max<long long>(2 * B * chunks, B * tiles * 2 * C + 2 * tcn_scalar_slabs(B, T, C));
}

int ptmi_tcn_norm_stats(const float* x, float* stats, double* workspace, int64_t B, int64_t T, int32_t C, int32_t rows, float eps,
                        ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !stats || B < 1 || T < 1 || C < 1, PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = C % 4 == 0 && aligned16({x});
    if (rows) {
        const long long nrows = B * T;
        PTMI_RETURN_IF((nrows + 3) / 4 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
        TcnNormArgs A{};
        A.x = x, A.T = T, A.C = C, A.rows = 1;
        PTMI_LAUNCH_VEC(tcn_norm_row_kernel, vec, dim3((unsigned)((nrows + 3) / 4)), st, A, nrows, eps, 0, stats);
        return launch_status();
    }
    PTMI_RETURN_IF(!workspace, PTMI_E_INVALID);
    const long long n = T * C;
    const long long chunks = (n + kTcnChunk - 1) / kTcnChunk;
    PTMI_RETURN_IF(chunks > 0x7fffffffLL || B > 65535, PTMI_E_UNSUPPORTED);
    PTMI_LAUNCH_VEC(tcn_norm_stats_example_kernel, vec, dim3((unsigned)chunks, (unsigned)B), st, x, n, workspace);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(tcn_group_finalize_kernel, dim3((unsigned)B), dim3(256), 0, st, workspace, chunks, (double)n, eps, 0, stats);
    return launch_status();
}

int ptmi_tcn_norm_apply(const float* x, const float* stats, const float* gamma, const float* beta, float* y, int64_t B, int64_t T,
                        int32_t C, int32_t rows, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !stats || !gamma || !beta || !y || B < 1 || T < 1 || C < 1, PTMI_E_INVALID);
    const bool vec = C % 4 == 0 && aligned16({x, y, gamma, beta});
    const TcnGrid g = tcn_grid(B, T, C, vec ? 4 : 1);
    PTMI_RETURN_IF(!g.ok, PTMI_E_UNSUPPORTED);
    TcnNormArgs A{};
    A.x = x, A.stats = stats, A.gamma = gamma, A.beta = beta, A.y = y, A.T = T, A.C = C, A.rows = rows ? 1 : 0;
    PTMI_LAUNCH_VEC(tcn_norm_pointwise_kernel, vec, g.grid, static_cast<hipStream_t>(stream), A, 0);
    return launch_status();
}

int ptmi_tcn_norm_backward(const float* gy, const float* x, const float* stats, const float* gamma, float* dx, float* dparams,
                           float* gsum, double* workspace, int64_t B, int64_t T, int32_t C, int32_t rows, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gy || !x || !stats || !gamma || !dx || !dparams || !gsum || !workspace, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || T < 1 || C < 1, PTMI_E_INVALID);
    const bool vec = C % 4 == 0 && aligned16({gy, x, dx, gamma});
    const TcnGrid g = tcn_grid(B, T, C, vec ? 4 : 1);
    const long long nrows = B * T;
    PTMI_RETURN_IF(!g.ok || (nrows + 3) / 4 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    TcnNormArgs A{};
    A.x = x, A.gy = gy, A.stats = stats, A.gsum = gsum, A.gamma = gamma, A.y = dx, A.T = T, A.C = C, A.rows = rows ? 1 : 0;
    A.wcol = workspace;
    A.wsca = workspace + B * g.tiles * 2 * C;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    PTMI_LAUNCH_VEC(tcn_norm_backward_reduce_kernel, vec, g.grid, st, A);
    if ((rc = launch_status())) return rc;
    if ((rc = colreduce(A.wcol, B * g.tiles, 2LL * C, StoreDepthwise{dparams, 0, 0}, st))) return rc;
    if (rows)
        PTMI_LAUNCH_VEC(tcn_norm_row_kernel, vec, dim3((unsigned)((nrows + 3) / 4)), st, A, nrows, 0.f, 1, gsum);
    else
        hipLaunchKernelGGL(tcn_group_finalize_kernel, dim3((unsigned)B), dim3(256), 0, st, A.wsca, g.tiles * g.cblocks,
                           (double)T * (double)C, 0.f, 1, gsum);
    if ((rc = launch_status())) return rc;
    PTMI_LAUNCH_VEC(tcn_norm_pointwise_kernel, vec, g.grid, st, A, 1);
    return launch_status();
}

}  // extern "C"
