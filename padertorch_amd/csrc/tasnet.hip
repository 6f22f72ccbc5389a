// The glue of the TasNet model (padertorch/contrib/examples/source_separation/tasnet/model.py:69-152) between its large pieces, forward
// and backward: the layer norm behind the encoder, the PReLU in front of the output projection, the mask head behind it and the mean
// subtraction behind the decoder.
//
// Layouts: the coders work on [B, N, E] (CHANNELS FIRST, frames innermost), the separator and both 1x1 convolutions on [B, E, C]
// (CHANNELS LAST).  The entry norm and the mask head are the two places where the layout changes, and each does it once, through an
// LDS tile of 32 frames x TC channels, tile[c][33]:
//   the channels-first side moves V = 4 (or 1) consecutive frames of one channel per lane; a 32-lane half of a wave covers 8 frame quads
//     x 4 channels: its four dword accesses tile[c][4 q + j] fall on the banks (c + 4 q + j) % 32, all different;
//   the channels-last side moves V = 4 (or 1) consecutive channels of one frame per lane; a half covers 8 channel quads x 4 frames:
//     tile[c0 + 4 i + j][e + de] falls on (4 i + de + j + const) % 32, all different.  (With the 4 frames of a half the global access is
//     128 contiguous bytes per frame.)  V = 1: 32 consecutive frames / channels per half, banks (c + e) % 32.
// V = 4 on a side needs that side's innermost extent to be a multiple of 4 and its pointers 16-byte aligned; each side is chosen
// on its own, per launch, and the arithmetic per element is the same in all four combinations.
//
// Sums: fp64 in threads, workgroups and finalize kernels; no atomics; partials go to a caller's workspace and are added in the fixed
// order that reduce.h defines: results are bit-reproducible.  No allocation, no synchronisation: capturable.
// The lengths of the entry norm are device data.
#include <algorithm>

#include "reduce.h"

namespace ptmi {

constexpr int kTnE = 32;                  // frames per tile
constexpr int kTnLd = kTnE + 1;           // tile[c][33]
constexpr int kTnFwdC = 256;              // channels per tile of the entry norm's forward (33.8 KB)
constexpr int kTnBwdC = 128;              // ... of its backward, which holds two tiles
constexpr int kTnHeadC = 64;              // ... of the mask head
constexpr int kTnChunk = 8192;            // elements per workgroup of the PReLU kernels
constexpr int kTnCenterChunk = 2048;      // samples per workgroup of the centring kernels

// ---- the tile's two sides.  f(c, e, v): c < nc the channel inside the tile, e < ne the (first) frame inside it, v the V values.
// Channels-first side into the tile: f fills v with V consecutive frames of channel c.
template <int V, class F>
__device__ __forceinline__ void tn_cf_in(float (*tile)[kTnLd], int nc, int ne, F f) {
    constexpr int per_row = kTnE / V;
    for (int q = threadIdx.x; q < nc * per_row; q += 256) {
        const int e = (q % per_row) * V, c = q / per_row;
        if (e < ne) {
            float v[V];
            f(c, e, v);
#pragma unroll
            for (int j = 0; j < V; ++j) tile[c][e + j] = v[j];
        }
    }
}

// ... and out of it: f stores the V consecutive frames v of channel c.
template <int V, class F>
__device__ __forceinline__ void tn_cf_out(float (*tile)[kTnLd], int nc, int ne, F f) {
    constexpr int per_row = kTnE / V;
    for (int q = threadIdx.x; q < nc * per_row; q += 256) {
        const int e = (q % per_row) * V, c = q / per_row;
        if (e < ne) {
            float v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = tile[c][e + j];
            f(c, e, v);
        }
    }
}

// The channels-last side's map of item q of a tile of TC channels: (channel, frame).  V = 4: 8 channel quads x 4 frames per half wave.
template <int V, int TC>
__device__ __forceinline__ void tn_cl_item(int q, int& c, int& e) {
    if constexpr (V == 4) {
        constexpr int nseg = TC / 32;
        const int r = q >> 5;
        c = (r % nseg) * 32 + (q & 7) * 4;
        e = (r / nseg) * 4 + ((q >> 3) & 3);
    } else {
        c = q % TC;
        e = q / TC;
    }
}

// Channels-last side into the tile: f fills v with V consecutive channels of frame e.
template <int V, int TC, class F>
__device__ __forceinline__ void tn_cl_in(float (*tile)[kTnLd], int nc, int ne, F f) {
    for (int q = threadIdx.x; q < TC * kTnE / V; q += 256) {
        int c, e;
        tn_cl_item<V, TC>(q, c, e);
        if (c < nc && e < ne) {
            float v[V];
            f(c, e, v);
#pragma unroll
            for (int j = 0; j < V; ++j) tile[c + j][e] = v[j];
        }
    }
}

template <int V, int TC, class F>
__device__ __forceinline__ void tn_cl_out(float (*tile)[kTnLd], int nc, int ne, F f) {
    for (int q = threadIdx.x; q < TC * kTnE / V; q += 256) {
        int c, e;
        tn_cl_item<V, TC>(q, c, e);
        if (c < nc && e < ne) {
            float v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = tile[c + j][e];
            f(c, e, v);
        }
    }
}

// Live frames of example b: lengths[b] clipped to [0, E]; no lengths: E.
__device__ __forceinline__ long long tn_live(const void* lengths, int is64, long long b, long long E) {
    if (!lengths) return E;
    const long long n = is64 ? static_cast<const long long*>(lengths)[b] : (long long)static_cast<const int*>(lengths)[b];
    return n < 0 ? 0 : (n > E ? E : n);
}

// ------------------------------------------------------------------------------------------------ a. entry norm
struct TnNormArgs {
    const float* w;        // [B, N, E]
    const float* gy;       // [B, E, N]  (backward)
    const float* gamma;    // [N]
    const float* beta;     // [N]        (forward)
    const void* lengths;   // [B] int32 / int64, or null
    const float* stats_in; // [B E, 2]   (backward)
    float* stats;          // [B E, 2]   (forward): (mean, rstd); (0, 0) on a dead row
    float* y;              // [B, E, N]  (forward)
    float* dw;             // [B, N, E]  (backward)
    double* wcol;          // [B tiles][2 N]: per-channel partial sums (backward)
    long long E;
    int N, is64;
    float eps;
};

// Workgroup (frame tile, b).  N <= kTnFwdC: w is read once and stays in the tile; else stage one sums every channel block's rows and
// stage two reads the blocks again.  A frame's sums: 8 threads, channels part, part + 8, ... ascending, then parts 0..7 in order.
template <int VF, int VL>
__global__ __launch_bounds__(256) void tasnet_entry_norm_forward_kernel(const TnNormArgs A) {
#pragma clang fp contract(off)
    __shared__ float tile[kTnFwdC][kTnLd];
    __shared__ double part[8][kTnE][2];
    __shared__ float smean[kTnE], srstd[kTnE];
    const long long b = blockIdx.y, e0 = (long long)blockIdx.x * kTnE;
    const int ne = (int)min((long long)kTnE, A.E - e0);
    const long long live = tn_live(A.lengths, A.is64, b, A.E);
    const float* __restrict__ wb = A.w + b * A.N * A.E + e0;
    const int nblk = (A.N + kTnFwdC - 1) / kTnFwdC;
    const int fe = threadIdx.x & 31, fp = threadIdx.x >> 5;
    double s1 = 0., s2 = 0.;
    for (int cb = 0; cb < nblk; ++cb) {
        const int c0 = cb * kTnFwdC, nc = min(kTnFwdC, A.N - c0);
        if (cb) __syncthreads();
        tn_cf_in<VF>(tile, nc, ne, [&](int c, int e, float (&v)[VF]) { load_vec<VF>(wb + (long long)(c0 + c) * A.E + e, v); });
        __syncthreads();
        if (fe < ne)
            for (int c = fp; c < nc; c += 8) {
                const double x = (double)tile[c][fe];
                s1 += x;
                s2 += x * x;
            }
    }
    part[fp][fe][0] = s1, part[fp][fe][1] = s2;
    __syncthreads();
    if (threadIdx.x < kTnE) {
        double t1 = part[0][fe][0], t2 = part[0][fe][1];
#pragma unroll
        for (int p = 1; p < 8; ++p) t1 += part[p][fe][0], t2 += part[p][fe][1];
        const double m = t1 / (double)A.N;
        const double var = fmax(t2 / (double)A.N - m * m, 0.);
        const bool on = e0 + fe < live;
        const float mean = on ? (float)m : 0.f, rstd = on ? (float)(1. / sqrt(var + (double)A.eps)) : 0.f;
        smean[fe] = mean, srstd[fe] = rstd;
        if (fe < ne) {
            A.stats[2 * (b * A.E + e0 + fe)] = mean;
            A.stats[2 * (b * A.E + e0 + fe) + 1] = rstd;
        }
    }
    __syncthreads();
    float* __restrict__ yb = A.y + (b * A.E + e0) * A.N;
    for (int cb = 0; cb < nblk; ++cb) {
        const int c0 = cb * kTnFwdC, nc = min(kTnFwdC, A.N - c0);
        if (nblk > 1) {
            __syncthreads();
            tn_cf_in<VF>(tile, nc, ne, [&](int c, int e, float (&v)[VF]) { load_vec<VF>(wb + (long long)(c0 + c) * A.E + e, v); });
            __syncthreads();
        }
        tn_cl_out<VL, kTnFwdC>(tile, nc, ne, [&](int c, int e, float (&v)[VL]) {
            const bool on = e0 + e < live;
            const float m = smean[e], rs = srstd[e];
            float ga[VL], be[VL];
            load_vec<VL>(A.gamma + c0 + c, ga);
            load_vec<VL>(A.beta + c0 + c, be);
#pragma unroll
            for (int j = 0; j < VL; ++j) v[j] = on ? fmaf(ga[j], (v[j] - m) * rs, be[j]) : 0.f;
            store_vec<VL>(yb + (long long)e * A.N + c0 + c, v);
        });
    }
}

// Workgroup (frame tile, b); two tiles of kTnBwdC channels: gy (channels last) and w (channels first).  Stage one, per channel block:
// per frame c1 = sum_n gy gamma, c2 = sum_n gy gamma xhat (as the forward's row sums), per channel the tile's 32 frames of gy xhat and
// gy (two threads of 16 frames each, ascending, then half 0 + half 1) to the workspace.  Stage two: dw (one block: the tiles are kept).
template <int VF, int VL>
__global__ __launch_bounds__(256) void tasnet_entry_norm_backward_kernel(const TnNormArgs A) {
#pragma clang fp contract(off)
    __shared__ float tg[kTnBwdC][kTnLd];
    __shared__ float tw[kTnBwdC][kTnLd];
    __shared__ double part[8][kTnE][2];
    __shared__ double half[kTnBwdC][2];
    __shared__ float smean[kTnE], srstd[kTnE], sg1[kTnE], sg2[kTnE];
    const long long b = blockIdx.y, e0 = (long long)blockIdx.x * kTnE;
    const int ne = (int)min((long long)kTnE, A.E - e0);
    const long long live = tn_live(A.lengths, A.is64, b, A.E);
    const float* __restrict__ wb = A.w + b * A.N * A.E + e0;
    const float* __restrict__ gb = A.gy + (b * A.E + e0) * A.N;
    const int nblk = (A.N + kTnBwdC - 1) / kTnBwdC;
    const int fe = threadIdx.x & 31, fp = threadIdx.x >> 5;
    if (threadIdx.x < kTnE) {
        const bool on = fe < ne && e0 + fe < live;
        smean[fe] = on ? A.stats_in[2 * (b * A.E + e0 + fe)] : 0.f;
        srstd[fe] = on ? A.stats_in[2 * (b * A.E + e0 + fe) + 1] : 0.f;
    }
    const int nlive = (int)max(0LL, min((long long)ne, live - e0));      // live frames of this tile: frames [0, nlive)
    auto fill = [&](int c0, int nc) {
        tn_cf_in<VF>(tw, nc, ne, [&](int c, int e, float (&v)[VF]) { load_vec<VF>(wb + (long long)(c0 + c) * A.E + e, v); });
        tn_cl_in<VL, kTnBwdC>(tg, nc, ne, [&](int c, int e, float (&v)[VL]) { load_vec<VL>(gb + (long long)e * A.N + c0 + c, v); });
    };
    double* __restrict__ col = A.wcol + (b * gridDim.x + blockIdx.x) * 2 * (long long)A.N;
    double s1 = 0., s2 = 0.;
    for (int cb = 0; cb < nblk; ++cb) {
        const int c0 = cb * kTnBwdC, nc = min(kTnBwdC, A.N - c0);
        __syncthreads();
        fill(c0, nc);
        __syncthreads();
        if (fe < nlive) {
            const float m = smean[fe], rs = srstd[fe];
            for (int c = fp; c < nc; c += 8) {
                const float gx = tg[c][fe] * A.gamma[c0 + c];
                const float xh = (tw[c][fe] - m) * rs;
                s1 += (double)gx;
                s2 += (double)gx * (double)xh;
            }
        }
        // per channel: thread (c, h) sums frames 16 h .. 16 h + 15 of the live part
        const int c = threadIdx.x & (kTnBwdC - 1), h = threadIdx.x >> 7;
        double dg = 0., db = 0.;
        if (c < nc)
            for (int e = 16 * h; e < min(16 * h + 16, nlive); ++e) {
                const float xh = (tw[c][e] - smean[e]) * srstd[e];
                dg += (double)tg[c][e] * (double)xh;
                db += (double)tg[c][e];
            }
        if (h == 1) half[c][0] = dg, half[c][1] = db;
        __syncthreads();
        if (h == 0 && c < nc) {
            col[c0 + c] = dg + half[c][0];
            col[A.N + c0 + c] = db + half[c][1];
        }
    }
    part[fp][fe][0] = s1, part[fp][fe][1] = s2;
    __syncthreads();
    if (threadIdx.x < kTnE) {
        double t1 = part[0][fe][0], t2 = part[0][fe][1];
#pragma unroll
        for (int p = 1; p < 8; ++p) t1 += part[p][fe][0], t2 += part[p][fe][1];
        sg1[fe] = (float)(t1 / (double)A.N), sg2[fe] = (float)(t2 / (double)A.N);
    }
    __syncthreads();
    float* __restrict__ db_ = A.dw + b * A.N * A.E + e0;
    for (int cb = 0; cb < nblk; ++cb) {
        const int c0 = cb * kTnBwdC, nc = min(kTnBwdC, A.N - c0);
        if (nblk > 1) {
            __syncthreads();
            fill(c0, nc);
            __syncthreads();
        }
        tn_cf_out<VF>(tw, nc, ne, [&](int c, int e, float (&v)[VF]) {
            const float ga = A.gamma[c0 + c];
#pragma unroll
            for (int j = 0; j < VF; ++j) {
                const float rs = srstd[e + j];
                const float xh = (v[j] - smean[e + j]) * rs;
                v[j] = e + j < nlive ? rs * fmaf(-xh, sg2[e + j], tg[c][e + j] * ga - sg1[e + j]) : 0.f;
            }
            store_vec<VF>(db_ + (long long)(c0 + c) * A.E + e, v);
        });
    }
}

// ------------------------------------------------------------------------------------------------ b. PReLU on rows
// mode 0: y = x > 0 ? x : a x.  mode 1: y = gx = x > 0 ? g : a g, and the workgroup's sum of g x over x <= 0 (the tie convention of
// tcn_dw_backward_z_kernel: prelu'(0) = a, and the tie counts for d a, where it adds g 0).
template <int V>
__global__ __launch_bounds__(256) void tasnet_prelu_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           const float* __restrict__ slope, float* __restrict__ y, long long n,
                                                           double* __restrict__ ws, int mode) {
    const float a = slope[0];
    const long long i0 = (long long)blockIdx.x * kTnChunk;
    const long long i1 = min(i0 + kTnChunk, n);
    double s[1] = {0.};
    for (long long i = i0 + (long long)threadIdx.x * V; i < i1; i += 256 * V) {
        float xv[V], o[V];
        load_vec<V>(x + i, xv);
        if (mode == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = xv[j] > 0.f ? xv[j] : a * xv[j];
        } else {
            float gv[V];
            load_vec<V>(g + i, gv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                s[0] += xv[j] > 0.f ? 0. : (double)gv[j] * (double)xv[j];
                o[j] = xv[j] > 0.f ? gv[j] : a * gv[j];
            }
        }
        store_vec<V>(y + i, o);
    }
    if (mode == 1) {
        block_sums<1>(s);
        if (threadIdx.x == 0) ws[blockIdx.x] = s[0];
    }
}

// One workgroup per row r: sum of its `slabs` partials (thread-strided, ascending, then the workgroup sum), times scale.
__global__ __launch_bounds__(256) void tasnet_sum_finalize_kernel(const double* __restrict__ ws, long long slabs, double scale,
                                                                  float* __restrict__ out) {
    const double* __restrict__ p = ws + (long long)blockIdx.x * slabs;
    double s[1] = {0.};
    for (long long i = threadIdx.x; i < slabs; i += 256) s[0] += p[i];
    block_sums<1>(s);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(s[0] * scale);
}

// ------------------------------------------------------------------------------------------------ c. mask head
enum { kActSigmoid = 0, kActRelu, kActLeakyRelu, kActElu, kActTanh, kActIdentity, kActCount };

__device__ __forceinline__ float tn_act(int act, float z) {
    switch (act) {
        case kActSigmoid: return 1.f / (1.f + expf(-z));
        case kActRelu: return z > 0.f ? z : (z != z ? z : 0.f);           // a NaN stays a NaN
        case kActLeakyRelu: return z > 0.f ? z : 0.01f * z;
        case kActElu: return z > 0.f ? z : expm1f(z);
        case kActTanh: return tanhf(z);
        default: return z;
    }
}

// d act / d z from the saved output m
__device__ __forceinline__ float tn_dact(int act, float m) {
    switch (act) {
        case kActSigmoid: return m * (1.f - m);
        case kActRelu: return m > 0.f ? 1.f : 0.f;
        case kActLeakyRelu: return m > 0.f ? 1.f : 0.01f;
        case kActElu: return m > 0.f ? 1.f : m + 1.f;
        case kActTanh: return 1.f - m * m;
        default: return 1.f;
    }
}

struct TnHeadArgs {
    const float* z;        // [B, E, C], C = A + K N  (forward)
    const float* gm;       // [K, B, N, E]  (backward)
    const float* gadd;     // [B, A, E] or null (zeros)  (backward)
    float* m;              // [K, B, N, E]: written (forward), read (backward)
    float* add;            // [B, A, E]  (forward)
    float* gz;             // [B, E, C]  (backward)
    long long B, E;
    int N, K, A, C, act;
};

// The channels-first row of column c of z: additional[b, c] for c < A, else m[k, b, n] with c - A = k N + n.
__device__ __forceinline__ long long tn_head_row(const TnHeadArgs& A, long long b, int c) {
    const int k = (c - A.A) / A.N, n = (c - A.A) % A.N;
    return (((long long)k * A.B + b) * A.N + n) * A.E;
}

// Workgroup (frame tile, channel block, b).
template <int VF, int VL>
__global__ __launch_bounds__(256) void tasnet_mask_head_kernel(const TnHeadArgs A, int backward) {
#pragma clang fp contract(off)
    __shared__ float tile[kTnHeadC][kTnLd];
    const long long b = blockIdx.z, e0 = (long long)blockIdx.x * kTnE;
    const int c0 = blockIdx.y * kTnHeadC;
    const int ne = (int)min((long long)kTnE, A.E - e0), nc = min(kTnHeadC, A.C - c0);
    if (!backward) {
        const float* __restrict__ zb = A.z + (b * A.E + e0) * A.C + c0;
        tn_cl_in<VL, kTnHeadC>(tile, nc, ne, [&](int c, int e, float (&v)[VL]) { load_vec<VL>(zb + (long long)e * A.C + c, v); });
        __syncthreads();
        tn_cf_out<VF>(tile, nc, ne, [&](int c, int e, float (&v)[VF]) {
            const int cc = c0 + c;
            if (cc < A.A) {
                store_vec<VF>(A.add + (b * A.A + cc) * A.E + e0 + e, v);
            } else {
#pragma unroll
                for (int j = 0; j < VF; ++j) v[j] = tn_act(A.act, v[j]);
                store_vec<VF>(A.m + tn_head_row(A, b, cc) + e0 + e, v);
            }
        });
    } else {
        tn_cf_in<VF>(tile, nc, ne, [&](int c, int e, float (&v)[VF]) {
            const int cc = c0 + c;
            if (cc < A.A) {
                if (A.gadd) {
                    load_vec<VF>(A.gadd + (b * A.A + cc) * A.E + e0 + e, v);
                } else {
#pragma unroll
                    for (int j = 0; j < VF; ++j) v[j] = 0.f;
                }
            } else {
                const long long at = tn_head_row(A, b, cc) + e0 + e;
                float mv[VF];
                load_vec<VF>(A.gm + at, v);
                load_vec<VF>(A.m + at, mv);
#pragma unroll
                for (int j = 0; j < VF; ++j) v[j] = v[j] * tn_dact(A.act, mv[j]);
            }
        });
        __syncthreads();
        float* __restrict__ gzb = A.gz + (b * A.E + e0) * A.C + c0;
        tn_cl_out<VL, kTnHeadC>(tile, nc, ne, [&](int c, int e, float (&v)[VL]) { store_vec<VL>(gzb + (long long)e * A.C + c, v); });
    }
}

// ------------------------------------------------------------------------------------------------ d. centre and crop
// Row (i, j), i < I, j < J: reads n samples at in + (i in_si + j in_sj) in_len, writes out_len at out + (i out_si + j out_sj) out_len.
// Forward: (i, j) = (k, b), in [K, B, T'] -> out [B, K, n]; backward: in [B, K, n] -> out [K, B, T'], zeros behind n.
struct TnCenterArgs {
    const float* in;
    float* out;
    double* ws;            // [I J][chunks]
    long long J, in_si, in_sj, out_si, out_sj, n, in_len, out_len, chunks;
};

__device__ __forceinline__ void tn_center_rows(const TnCenterArgs& A, const float*& src, float*& dst) {
    const long long i = blockIdx.y / A.J, j = blockIdx.y % A.J;
    src = A.in + (i * A.in_si + j * A.in_sj) * A.in_len;
    dst = A.out + (i * A.out_si + j * A.out_sj) * A.out_len;
}

// Workgroup (chunk, row): the chunk's sum (chunks past n write nothing: the apply kernel reads the first `chunks` only).
template <int V>
__global__ __launch_bounds__(256) void tasnet_center_sum_kernel(const TnCenterArgs A) {
    const float* src;
    float* dst;
    tn_center_rows(A, src, dst);
    const long long t0 = (long long)blockIdx.x * kTnCenterChunk, t1 = min(t0 + kTnCenterChunk, A.n);
    double s[1] = {0.};
    // a thread owns the quads t, t + 1024, ... whatever V is: the partial does not depend on the alignment of the row
    for (long long t = t0 + (long long)threadIdx.x * 4; t < t1; t += 1024) {
        if constexpr (V == 4) {
            float v[4];
            load_vec<4>(src + t, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) s[0] += (double)v[j];
        } else {
            for (int j = 0; j < 4 && t + j < t1; ++j) s[0] += (double)src[t + j];
        }
    }
    block_sums<1>(s);
    if (threadIdx.x == 0) A.ws[(long long)blockIdx.y * A.chunks + blockIdx.x] = s[0];
}

// Workgroup (chunk of out_len, row): the row's mean from its partials (thread-strided, ascending, then the workgroup sum: the same
// value in every workgroup of the row), out = in - mean below n, 0 from n on.
template <int V>
__global__ __launch_bounds__(256) void tasnet_center_apply_kernel(const TnCenterArgs A) {
    const float* src;
    float* dst;
    tn_center_rows(A, src, dst);
    const double* __restrict__ p = A.ws + (long long)blockIdx.y * A.chunks;
    double s[1] = {0.};
    for (long long i = threadIdx.x; i < A.chunks; i += 256) s[0] += p[i];
    block_sums<1>(s);
    const float mean = (float)(s[0] / (double)A.n);
    const long long t0 = (long long)blockIdx.x * kTnCenterChunk, t1 = min(t0 + kTnCenterChunk, A.out_len);
    for (long long t = t0 + (long long)threadIdx.x * V; t < t1; t += 256 * V) {
        float v[V];
        if (t < A.n) {                      // V == 4: n and out_len are multiples of 4, a quad lies on one side
            load_vec<V>(src + t, v);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = v[j] - mean;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = 0.f;
        }
        store_vec<V>(dst + t, v);
    }
}

// kernel<VF, VL>: VF the vector width of the channels-first side, VL of the channels-last side
#define TN_LAUNCH2(kernel, vf, vl, grid, st, ...)                                           \
    do {                                                                                    \
        if (vf && vl)                                                                       \
            hipLaunchKernelGGL((kernel<4, 4>), grid, dim3(256), 0, st, __VA_ARGS__);        \
        else if (vf)                                                                        \
            hipLaunchKernelGGL((kernel<4, 1>), grid, dim3(256), 0, st, __VA_ARGS__);        \
        else if (vl)                                                                        \
            hipLaunchKernelGGL((kernel<1, 4>), grid, dim3(256), 0, st, __VA_ARGS__);        \
        else                                                                                \
            hipLaunchKernelGGL((kernel<1, 1>), grid, dim3(256), 0, st, __VA_ARGS__);        \
    } while (0)

static long long tn_tiles(int64_t E) { return (E + kTnE - 1) / kTnE; }

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_tasnet_entry_norm_workspace_elems(int64_t B, int32_t N, int64_t E) {
    if (B < 1 || N < 1 || E < 1) return PTMI_E_INVALID;
    return B * tn_tiles(E) * 2 * (long long)N;
}

int ptmi_tasnet_entry_norm_forward(const float* w, const float* gamma, const float* beta, const void* lengths, int32_t lengths_int64,
                                   float* y, float* stats, int64_t B, int32_t N, int64_t E, float eps, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!w || !gamma || !beta || !y || !stats || B < 1 || N < 1 || E < 1, PTMI_E_INVALID);
    const long long tiles = tn_tiles(E);
    PTMI_RETURN_IF(tiles > 0x7fffffffLL || B > 65535, PTMI_E_UNSUPPORTED);
    const bool vf = E % 4 == 0 && aligned16({w});
    const bool vl = N % 4 == 0 && aligned16({y, gamma, beta});
    TnNormArgs A{};
    A.w = w, A.gamma = gamma, A.beta = beta, A.lengths = lengths, A.is64 = lengths_int64, A.y = y, A.stats = stats;
    A.E = E, A.N = N, A.eps = eps;
    TN_LAUNCH2(tasnet_entry_norm_forward_kernel, vf, vl, dim3((unsigned)tiles, (unsigned)B), static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int ptmi_tasnet_entry_norm_backward(const float* gy, const float* w, const float* stats, const float* gamma, const void* lengths,
                                    int32_t lengths_int64, float* dw, float* dparams, double* workspace, int64_t B, int32_t N,
                                    int64_t E, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gy || !w || !stats || !gamma || !dw || !dparams || !workspace || B < 1 || N < 1 || E < 1, PTMI_E_INVALID);
    const long long tiles = tn_tiles(E);
    PTMI_RETURN_IF(tiles > 0x7fffffffLL || B > 65535, PTMI_E_UNSUPPORTED);
    const bool vf = E % 4 == 0 && aligned16({w, dw});
    const bool vl = N % 4 == 0 && aligned16({gy});
    TnNormArgs A{};
    A.w = w, A.gy = gy, A.gamma = gamma, A.lengths = lengths, A.is64 = lengths_int64, A.stats_in = stats, A.dw = dw;
    A.wcol = workspace, A.E = E, A.N = N;
    hipStream_t st = static_cast<hipStream_t>(stream);
    TN_LAUNCH2(tasnet_entry_norm_backward_kernel, vf, vl, dim3((unsigned)tiles, (unsigned)B), st, A);
    int rc = launch_status();
    if (rc) return rc;
    return colreduce(workspace, B * tiles, 2LL * N, StorePlain{dparams}, st);
}

int64_t ptmi_tasnet_prelu_workspace_elems(int64_t n) {
    if (n < 1) return PTMI_E_INVALID;
    return (n + kTnChunk - 1) / kTnChunk;
}

int ptmi_tasnet_prelu_forward(const float* x, const float* slope, float* y, int64_t n, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !slope || !y || n < 1, PTMI_E_INVALID);
    const long long chunks = (n + kTnChunk - 1) / kTnChunk;
    PTMI_RETURN_IF(chunks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    const bool vec = n % 4 == 0 && aligned16({x, y});
    PTMI_LAUNCH_VEC(tasnet_prelu_kernel, vec, dim3((unsigned)chunks), static_cast<hipStream_t>(stream), x, (const float*)nullptr, slope, y,
              (long long)n, (double*)nullptr, 0);
    return launch_status();
}

int ptmi_tasnet_prelu_backward(const float* g, const float* x, const float* slope, float* gx, float* dslope, double* workspace,
                               int64_t n, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!g || !x || !slope || !gx || !dslope || !workspace || n < 1, PTMI_E_INVALID);
    const long long chunks = (n + kTnChunk - 1) / kTnChunk;
    PTMI_RETURN_IF(chunks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    const bool vec = n % 4 == 0 && aligned16({g, x, gx});
    hipStream_t st = static_cast<hipStream_t>(stream);
    PTMI_LAUNCH_VEC(tasnet_prelu_kernel, vec, dim3((unsigned)chunks), st, x, g, slope, gx, (long long)n, workspace, 1);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(tasnet_sum_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, chunks, 1., dslope);
    return launch_status();
}

static int tn_head(TnHeadArgs A, int backward, bool vf, bool vl, ptmi_stream_t stream) {
    PTMI_RETURN_IF(A.B < 1 || A.E < 1 || A.N < 1 || A.K < 1 || A.A < 0 || A.act < 0 || A.act >= kActCount, PTMI_E_INVALID);
    const long long C = (long long)A.A + (long long)A.K * A.N;
    const long long tiles = tn_tiles(A.E), cblocks = (C + kTnHeadC - 1) / kTnHeadC;
    PTMI_RETURN_IF(C > 0x7fffffffLL || tiles > 0x7fffffffLL || cblocks > 65535 || A.B > 65535, PTMI_E_UNSUPPORTED);
    A.C = (int)C;
    vf = vf && A.E % 4 == 0;
    vl = vl && C % 4 == 0;
    TN_LAUNCH2(tasnet_mask_head_kernel, vf, vl, dim3((unsigned)tiles, (unsigned)cblocks, (unsigned)A.B), static_cast<hipStream_t>(stream),
               A, backward);
    return launch_status();
}

int ptmi_tasnet_mask_head_forward(const float* z, float* m, float* additional, int64_t B, int64_t E, int32_t N, int32_t K, int32_t A,
                                  int32_t activation, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!z || !m || (A > 0 && !additional), PTMI_E_INVALID);
    TnHeadArgs H{};
    H.z = z, H.m = m, H.add = additional, H.B = B, H.E = E, H.N = N, H.K = K, H.A = A, H.act = activation;
    return tn_head(H, 0, aligned16({m, additional}), aligned16({z}), stream);
}

int ptmi_tasnet_mask_head_backward(const float* gm, const float* m, const float* g_additional, float* gz, int64_t B, int64_t E,
                                   int32_t N, int32_t K, int32_t A, int32_t activation, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gm || !m || !gz, PTMI_E_INVALID);
    TnHeadArgs H{};
    H.gm = gm, H.m = const_cast<float*>(m), H.gadd = g_additional, H.gz = gz, H.B = B, H.E = E, H.N = N, H.K = K, H.A = A;
    H.act = activation;
    return tn_head(H, 1, aligned16({gm, m, g_additional}), aligned16({gz}), stream);
}

int64_t ptmi_tasnet_center_workspace_elems(int64_t K, int64_t B, int64_t T_in, int64_t T_out) {
    if (K < 1 || B < 1 || T_in < 1 || T_out < 1 || T_out > T_in) return PTMI_E_INVALID;
    return K * B * ((T_out + kTnCenterChunk - 1) / kTnCenterChunk);
}

int ptmi_tasnet_center(const float* in, float* out, double* workspace, int64_t K, int64_t B, int64_t T_in, int64_t T_out,
                       int32_t backward, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!in || !out || !workspace || K < 1 || B < 1 || T_in < 1 || T_out < 1 || T_out > T_in, PTMI_E_INVALID);
    TnCenterArgs A{};
    A.in = in, A.out = out, A.ws = workspace, A.J = B, A.n = T_out;
    A.chunks = (T_out + kTnCenterChunk - 1) / kTnCenterChunk;
    if (!backward) {            // [K, B, T_in] -> [B, K, T_out]
        A.in_si = B, A.in_sj = 1, A.in_len = T_in, A.out_si = 1, A.out_sj = K, A.out_len = T_out;
    } else {                    // [B, K, T_out] -> [K, B, T_in]
        A.in_si = 1, A.in_sj = K, A.in_len = T_out, A.out_si = B, A.out_sj = 1, A.out_len = T_in;
    }
    const long long out_chunks = (A.out_len + kTnCenterChunk - 1) / kTnCenterChunk;
    PTMI_RETURN_IF(out_chunks > 0x7fffffffLL || K * B > 65535, PTMI_E_UNSUPPORTED);
    const bool vec = T_in % 4 == 0 && T_out % 4 == 0 && aligned16({in, out});
    hipStream_t st = static_cast<hipStream_t>(stream);
    PTMI_LAUNCH_VEC(tasnet_center_sum_kernel, vec, dim3((unsigned)A.chunks, (unsigned)(K * B)), st, A);
    int rc = launch_status();
    if (rc) return rc;
    PTMI_LAUNCH_VEC(tasnet_center_apply_kernel, vec, dim3((unsigned)out_chunks, (unsigned)(K * B)), st, A);
    return launch_status();
}

}  // extern "C"
