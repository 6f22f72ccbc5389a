// WaveNet vocoder (padertorch/modules/wavenet/wavenet.py, padertorch/ops/mu_law.py, nv-wavenet's sampling loop): the kernels that are not
// GEMMs.  Activations are [B, T, C] with channels innermost (as csrc/tcn.hip); every 1x1 convolution is a planes GEMM (ops/gemm.py).
//
//   mu_law_encode / _decode      the companding in fp64 per element, codes clamped to [0, Q - 1]
//   wavenet_embed                codes and x0[b, t, :] = embed[code] in one launch; dEmbed by per-class row scans (no atomics)
//   wavenet_ola                  the overlap-add of the conditioning ConvTranspose1d behind its GEMM (gather form), bias and crop fused;
//                                its adjoint is the framing gather
//   wavenet_gate                 the per-layer gated activation on P = x W^T, the conditioning read and acts written as strided slices
//   wavenet_colsum               column sums in the library's fixed order (reduce.h): every bias gradient
//   wavenet_generate             the autoregressive sampling loop: one workgroup owns kEx sequences for the whole run and synchronises
//                                with __syncthreads() alone - no workgroup ever waits for another one
#include <math.h>

#include "reduce.h"

namespace ptmi {
namespace {

// ------------------------------------------------------------------------------------------------------------ mu-law
__device__ __forceinline__ int mu_law_code(float x, int Q) {
    const double mu = (double)(Q - 1);
    const double ax = fabs((double)x);
    const double sgn = x > 0.f ? 1. : (x < 0.f ? -1. : 0.);
    const double xm = sgn * log1p(mu * ax) / log1p(mu);
    const double v = (xm + 1.) / 2. * mu + 0.5;
    long long c = (long long)v;            // truncation, as .long()
    if (!(v == v)) c = 0;
    return (int)(c < 0 ? 0 : (c > Q - 1 ? Q - 1 : c));
}

static __global__ __launch_bounds__(256) void mu_law_encode_kernel(const float* __restrict__ x, long long n, int Q, long long* __restrict__ codes) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) codes[i] = mu_law_code(x[i], Q);
}

template <typename T>
static __global__ __launch_bounds__(256) void mu_law_decode_kernel(const T* __restrict__ codes, long long n, int Q, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double mu = (double)(Q - 1);
    double c = (double)codes[i];
    c = c < 0. ? 0. : (c > mu ? mu : c);
    const double s = 2. * (c / mu) - 1.;
    const double mag = (1. / mu) * (pow(1. + mu, fabs(s)) - 1.);
    out[i] = (float)(s > 0. ? mag : (s < 0. ? -mag : 0.));
}

// ------------------------------------------------------------------------------------------------------------ embedding
// 256 rows per workgroup: a code per thread, then the rows' R channels copied with consecutive lanes on consecutive floats.
static __global__ __launch_bounds__(256) void embed_forward_kernel(const float* __restrict__ audio, const float* __restrict__ embed, long long n,
                                                                   int A, int R, long long* __restrict__ codes, float* __restrict__ x0) {
    __shared__ int code[256];
    const long long r0 = (long long)blockIdx.x * 256;
    const long long row = r0 + threadIdx.x;
    if (row < n) {
        const int c = mu_law_code(audio[row], A);
        code[threadIdx.x] = c;
        codes[row] = c;
    }
    __syncthreads();
    const long long rows = n - r0 < 256 ? n - r0 : 256;
    for (long long i = threadIdx.x; i < rows * R; i += 256) {
        const int rr = (int)(i / R), ch = (int)(i % R);
        x0[r0 * R + i] = embed[(long long)code[rr] * R + ch];
    }
}

constexpr int kEmbedRows = 1024;   // rows one workgroup of the embedding's backward scans (256 per wave)

// Workgroup (a, s): the rows of slab s whose code is a, ascending inside every wave, the waves combined ((0 + 1) + 2) + 3;
// ws[s][a][r] holds the partial, colreduce adds the slabs.
static __global__ __launch_bounds__(256) void embed_backward_kernel(const float* __restrict__ dx, const long long* __restrict__ codes, long long n,
                                                                    int A, int R, double* __restrict__ ws) {
    __shared__ double red[4][256];
    const int a = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.y * kEmbedRows + w * 256;
    double acc[4] = {0., 0., 0., 0.};
    for (int q = 0; q < 4; ++q) {
        const long long row = base + q * 64 + lane;
        const bool hit = row < n && codes[row] == a;
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int i = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float* p = dx + (base + q * 64 + i) * R;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                if (kk * 64 + lane < R) acc[kk] += (double)p[kk * 64 + lane];
        }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) red[w][kk * 64 + lane] = acc[kk];
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int r = kk * 64 + lane;
            if (r < R) ws[((long long)blockIdx.y * A + a) * R + r] = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ column sums
constexpr int kColsumRows = 256;

static __global__ __launch_bounds__(256) void colsum_slab_kernel(const float* __restrict__ x, long long rows, int width, long long ld,
                                                                 double* __restrict__ ws) {
    __shared__ double red[4][64];
    const int jx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long j = (long long)blockIdx.x * 64 + jx;
    const long long r0 = (long long)blockIdx.y * kColsumRows;
    const long long r1 = r0 + kColsumRows < rows ? r0 + kColsumRows : rows;
    double s = 0.;
    if (j < width)
        for (long long r = r0 + g; r < r1; r += 4) s += (double)x[r * ld + j];
    red[g][jx] = s;
    __syncthreads();
    if (g == 0 && j < width) ws[(long long)blockIdx.y * width + j] = ((red[0][jx] + red[1][jx]) + red[2][jx]) + red[3][jx];
}

// ------------------------------------------------------------------------------------------------------------ overlap-add
// G [B Tf, C window] (column co window + k) -> out [B, Tout, C]: out[b, t', co] = bias[co] + sum_f G[b, f, co, t' + front - f stride],
// f ascending.  Lanes run along t' (the reads of one f are consecutive in k).
static __global__ __launch_bounds__(256) void ola_forward_kernel(const float* __restrict__ G, const float* __restrict__ bias, int C, long long Tf,
                                                                 int window, int stride, long long front, long long Tout,
                                                                 float* __restrict__ out) {
    const long long tp = (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    const int co = blockIdx.y * 4 + (threadIdx.x >> 6);
    const long long b = blockIdx.z;
    if (tp >= Tout || co >= C) return;
    const long long t = tp + front;
    long long f_hi = t / stride;
    if (f_hi > Tf - 1) f_hi = Tf - 1;
    long long f_lo = t - window + 1 <= 0 ? 0 : (t - window + 1 + stride - 1) / stride;
    float acc = bias[co];
    for (long long f = f_lo; f <= f_hi; ++f) acc += G[((b * Tf + f) * C + co) * window + (t - f * stride)];
    out[(b * Tout + tp) * C + co] = acc;
}

// dG[b, f, co, k] = dout[b, f stride + k - front, co] inside [0, Tout), else 0.
static __global__ __launch_bounds__(256) void ola_backward_kernel(const float* __restrict__ dout, int C, long long Tf, int window, int stride,
                                                                  long long front, long long Tout, long long total, float* __restrict__ dG) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % window);
    const long long q = i / window;
    const int co = (int)(q % C);
    const long long bf = q / C;
    const long long f = bf % Tf, b = bf / Tf;
    const long long tp = f * stride + k - front;
    dG[i] = (tp >= 0 && tp < Tout) ? dout[(b * Tout + tp) * C + co] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ gate
__device__ __forceinline__ float sigmoid_accurate(float v) { return 1.f / (1.f + expf(-v)); }

// One thread per (row, V channels r): z[r] and z[R + r] from P [B T, 4R], the bias and the conditioning slice (row stride ldc),
// acts = tanh * sigmoid to the slice with row stride lda.
template <int V>
static __global__ __launch_bounds__(256) void gate_forward_kernel(const float* __restrict__ P, const float* __restrict__ bias,
                                                                  const float* __restrict__ cond, long long ldc, long long rows, long long T,
                                                                  int R, int d, float* __restrict__ acts, long long lda) {
    const int per = R / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * per) return;
    const long long row = i / per;
    const int r = (int)(i % per) * V;
    const long long t = row % T;
    float zt[V], zs[V], a[V], c[V], o[V];
    load_vec<V>(P + row * 4 * R + 2 * R + r, zt);
    load_vec<V>(P + row * 4 * R + 3 * R + r, zs);
    if (t >= d) {
        load_vec<V>(P + (row - d) * 4 * R + r, a);
        load_vec<V>(P + (row - d) * 4 * R + R + r, c);
#pragma unroll
        for (int v = 0; v < V; ++v) zt[v] += a[v], zs[v] += c[v];
    }
    load_vec<V>(bias + r, a);
    load_vec<V>(bias + R + r, c);
#pragma unroll
    for (int v = 0; v < V; ++v) zt[v] += a[v], zs[v] += c[v];
    load_vec<V>(cond + row * ldc + r, a);
    load_vec<V>(cond + row * ldc + R + r, c);
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = tanhf(zt[v] + a[v]) * sigmoid_accurate(zs[v] + c[v]);
    store_vec<V>(acts + row * lda + r, o);
}

// dz recomputed from P, bias and cond; written to the dcond slice (row stride ldd).
template <int V>
static __global__ __launch_bounds__(256) void gate_backward_dz_kernel(const float* __restrict__ dacts, long long lda, const float* __restrict__ P,
                                                                      const float* __restrict__ bias, const float* __restrict__ cond,
                                                                      long long ldc, long long rows, long long T, int R, int d,
                                                                      float* __restrict__ dz, long long ldd) {
    const int per = R / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * per) return;
    const long long row = i / per;
    const int r = (int)(i % per) * V;
    const long long t = row % T;
    float zt[V], zs[V], a[V], c[V], g[V];
    load_vec<V>(P + row * 4 * R + 2 * R + r, zt);
    load_vec<V>(P + row * 4 * R + 3 * R + r, zs);
    if (t >= d) {
        load_vec<V>(P + (row - d) * 4 * R + r, a);
        load_vec<V>(P + (row - d) * 4 * R + R + r, c);
#pragma unroll
        for (int v = 0; v < V; ++v) zt[v] += a[v], zs[v] += c[v];
    }
    load_vec<V>(bias + r, a);
    load_vec<V>(bias + R + r, c);
#pragma unroll
    for (int v = 0; v < V; ++v) zt[v] += a[v], zs[v] += c[v];
    load_vec<V>(cond + row * ldc + r, a);
    load_vec<V>(cond + row * ldc + R + r, c);
    load_vec<V>(dacts + row * lda + r, g);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float ta = tanhf(zt[v] + a[v]), sg = sigmoid_accurate(zs[v] + c[v]);
        a[v] = g[v] * sg * (1.f - ta * ta);
        c[v] = g[v] * ta * sg * (1.f - sg);
    }
    store_vec<V>(dz + row * ldd + r, a);
    store_vec<V>(dz + row * ldd + R + r, c);
}

// dP [B T, 4R] in gather form: dP[b, t, j] = dz[b, t + d, j] (0 past the end), dP[b, t, 2R + j] = dz[b, t, j], j < 2R.
template <int V>
static __global__ __launch_bounds__(256) void gate_backward_dp_kernel(const float* __restrict__ dz, long long ldd, long long rows, long long T, int R,
                                                                      int d, float* __restrict__ dP) {
    const int per = 2 * R / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * per) return;
    const long long row = i / per;
    const int j = (int)(i % per) * V;
    const long long t = row % T;
    float now[V], later[V];
    load_vec<V>(dz + row * ldd + j, now);
    if (t + d < T) {
        load_vec<V>(dz + (row + d) * ldd + j, later);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) later[v] = 0.f;
    }
    store_vec<V>(dP + row * 4 * R + j, later);
    store_vec<V>(dP + row * 4 * R + 2 * R + j, now);
}

// ------------------------------------------------------------------------------------------------------------ sampling loop
constexpr int kEx = 4;                    // sequences per workgroup
constexpr int kLdsBytes = 64 * 1024;      // what a workgroup may use without asking for more

__host__ __device__ inline int gen_work_floats(int R, int S, int A) { return kEx * (2 * R + 2 * R + R + (S > A ? S : A) + A + 256); }

inline bool gen_ring_in_lds(int R, int S, int A, long long ring_rows) {
    return (long long)gen_work_floats(R, S, A) * 4 + ring_rows * kEx * R * 4 + 64 <= kLdsBytes;
}

// out(e, j, init[j] + sum_k Wt[k N + j] in[e][k]) for j < N and all kEx sequences: a thread owns column j, so one (coalesced) weight
// load serves kEx FMAs, k ascending - the value of a sequence does not depend on its neighbours.  The loop is bound by the latency of
// its weight loads, so a pass over n <= 128 (64) columns cuts k into 2 (4) ranges for the threads it would leave idle; the partial
// sums meet in `part` [ranges][kEx][256 / ranges] and are added in ascending order of the range.  Every thread must call it.
template <class Out>
__device__ __forceinline__ void matvec(const float* __restrict__ Wt, const float* __restrict__ init, int N, int K, const float* in, int in_stride,
                                       float* part, Out out) {
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int n = N - j0 < 256 ? N - j0 : 256;
        const int ranges = n <= 64 ? 4 : (n <= 128 ? 2 : 1);          // (only the last pass can be short: `part` is used once per call)
        const int cols = 256 / ranges;
        const int jj = threadIdx.x % cols, q = threadIdx.x / cols;
        const int j = j0 + jj;
        const int kq = (K + ranges - 1) / ranges;
        const int k0 = q * kq, k1 = k0 + kq < K ? k0 + kq : K;
        float acc[kEx];
        const float b0 = (init && q == 0 && jj < n) ? init[j] : 0.f;
#pragma unroll
        for (int e = 0; e < kEx; ++e) acc[e] = b0;
        if (jj < n) {
#pragma unroll 4
            for (int k = k0; k < k1; ++k) {      // (unrolled 16 times the step took more than twice as long: profiles/wavenet.txt)
                const float w = Wt[(long long)k * N + j];
#pragma unroll
                for (int e = 0; e < kEx; ++e) acc[e] = fmaf(w, in[e * in_stride + k], acc[e]);
            }
        }
        if (ranges == 1) {
            if (jj < n) {
#pragma unroll
                for (int e = 0; e < kEx; ++e) out(e, j, acc[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < kEx; ++e) part[(q * kEx + e) * cols + jj] = acc[e];
            __syncthreads();
            if (q == 0 && jj < n) {
#pragma unroll
                for (int e = 0; e < kEx; ++e) {
                    float v = part[e * cols + jj];
                    for (int qq = 1; qq < ranges; ++qq) v += part[(qq * kEx + e) * cols + jj];
                    out(e, j, v);
                }
            }
        }
    }
}

// packed (floats), per layer l at l * layer_stride: Wg [2R (k: x[t - d] | x[t])][2R], bg [2R], Wrs [R][S + R] (skip | residual; the last
// layer's residual columns are zero), brs [S + R]; behind the layers Wo [S][A], We [A][A].
static __global__ __launch_bounds__(256) void generate_kernel(const float* __restrict__ packed, const float* __restrict__ embed,
                                                              const float* __restrict__ cond, const float* __restrict__ u,
                                                              const int* __restrict__ layer_meta, const int* __restrict__ seq_meta, int nseq,
                                                              long long Tc, int L, int R, int S, int A, int ring_rows, int ring_in_lds,
                                                              long long t0, int nsteps, long long Tmax, float* __restrict__ ring_global,
                                                              int* __restrict__ last_code, long long* __restrict__ y,
                                                              float* __restrict__ logits) {
    extern __shared__ float smem[];
    __shared__ int code[kEx];
    __shared__ int sb[kEx], son[kEx], slen[kEx];
    const int tid = threadIdx.x;
    const int SA = S > A ? S : A;
    float* xin = smem;                       // [kEx][2R]: x[t - d] | x[t] of the current layer
    float* zbuf = xin + kEx * 2 * R;         // [kEx][2R]
    float* acts = zbuf + kEx * 2 * R;        // [kEx][R]
    float* skip = acts + kEx * R;            // [kEx][SA]: the skip sum, later the logits
    float* obuf = skip + kEx * SA;           // [kEx][A]
    float* part = obuf + kEx * A;            // [kEx][256]: partial sums of a short matvec pass
    float* ring_lds = part + kEx * 256;
    const long long ring_floats = (long long)ring_rows * kEx * R;
    float* ring_mine = ring_global + blockIdx.x * ring_floats;
    float* ring = ring_in_lds ? ring_lds : ring_mine;
    const long long layer_stride = 4LL * R * R + 2 * R + (long long)R * (S + R) + (S + R);
    const int seq0 = blockIdx.x * kEx;

    if (tid < kEx) {
        const int s = seq0 + tid < nseq ? seq0 + tid : nseq - 1;      // a partial group computes its last sequence again and writes nothing
        code[tid] = last_code[seq0 + tid];
        sb[tid] = seq_meta[3 * s], son[tid] = seq_meta[3 * s + 1], slen[tid] = seq_meta[3 * s + 2];
    }
    if (ring_in_lds)
        for (long long i = tid; i < ring_floats; i += 256) ring_lds[i] = ring_mine[i];
    __syncthreads();

    for (int step = 0; step < nsteps; ++step) {
        const long long t = t0 + step;
        for (int i = tid; i < kEx * R; i += 256) {
            const int e = i / R, r = i % R;
            xin[e * 2 * R + R + r] = embed[(long long)code[e] * R + r];
        }
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            const int d = layer_meta[2 * l];
            const long long slot = layer_meta[2 * l + 1] + t % d;
            const float* Wg = packed + l * layer_stride;
            const float* bg = Wg + 4LL * R * R;
            const float* Wrs = bg + 2 * R;
            const float* brs = Wrs + (long long)R * (S + R);
            for (int i = tid; i < kEx * R; i += 256) {              // the ring holds this layer's input of d steps ago in the slot it now takes
                const int e = i / R, r = i % R;
                float* p = ring + slot * kEx * R + i;
                xin[e * 2 * R + r] = t >= d ? *p : 0.f;
                *p = xin[e * 2 * R + R + r];
            }
            __syncthreads();
            matvec(Wg, bg, 2 * R, 2 * R, xin, 2 * R, part, [&](int e, int j, float v) {
                long long tc = t < slen[e] ? t : slen[e] - 1;
                zbuf[e * 2 * R + j] = v + cond[((long long)sb[e] * Tc + son[e] + tc) * (2LL * R * L) + l * 2 * R + j];
            });
            __syncthreads();
            for (int i = tid; i < kEx * R; i += 256) {
                const int e = i / R, r = i % R;
                acts[i] = tanhf(zbuf[e * 2 * R + r]) * sigmoid_accurate(zbuf[e * 2 * R + R + r]);
            }
            __syncthreads();
            matvec(Wrs, brs, S + R, R, acts, R, part, [&](int e, int j, float v) {
                if (j < S)
                    skip[e * SA + j] = l == 0 ? v : skip[e * SA + j] + v;
                else
                    xin[e * 2 * R + R + (j - S)] += v;
            });
            __syncthreads();
        }
        for (int i = tid; i < kEx * S; i += 256) {
            const int e = i / S, s = i % S;
            skip[e * SA + s] = fmaxf(skip[e * SA + s], 0.f);
        }
        __syncthreads();
        const float* Wo = packed + L * layer_stride;
        const float* We = Wo + (long long)S * A;
        matvec(Wo, nullptr, A, S, skip, SA, part, [&](int e, int j, float v) { obuf[e * A + j] = fmaxf(v, 0.f); });
        __syncthreads();
        matvec(We, nullptr, A, A, obuf, A, part, [&](int e, int j, float v) {
            skip[e * SA + j] = v;
            if (logits && seq0 + e < nseq && t < slen[e]) logits[((long long)(seq0 + e) * Tmax + t) * A + j] = v;
        });
        __syncthreads();
        // inverse-CDF draw, one wave per sequence: lane i owns the classes [i per, (i + 1) per); running sums in one fixed order
        {
            const int e = tid >> 6, lane = tid & 63;
            const float* lg = skip + e * SA;
            const int per = (A + 63) / 64;
            const int a0 = lane * per, a1 = a0 + per < A ? a0 + per : A;
            float m = -INFINITY;
            for (int a = a0; a < a1; ++a) m = fmaxf(m, lg[a]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            float mine = 0.f;
            for (int a = a0; a < a1; ++a) mine += expf(lg[a] - m);
            float incl = mine;                                      // inclusive scan over the lanes
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const float up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            const float total = __shfl(incl, 63, 64);
            const long long tc = t < slen[e] ? t : slen[e] - 1;
            const float target = u[(long long)sb[e] * Tc + son[e] + tc] * total;
            float run = incl - mine;
            int pick = A - 1;
            bool found = false;
            for (int a = a0; a < a1; ++a) {
                run += expf(lg[a] - m);
                if (!found && run >= target) pick = a, found = true;
            }
            if (!found) pick = A - 1;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const int other = __shfl_xor(pick, o, 64);
                pick = other < pick ? other : pick;
            }
            if (lane == 0) {
                code[e] = pick;
                if (seq0 + e < nseq && t < slen[e]) y[(long long)(seq0 + e) * Tmax + t] = pick;
            }
        }
        __syncthreads();
    }
    if (tid < kEx) last_code[seq0 + tid] = code[tid];
    if (ring_in_lds)
        for (long long i = tid; i < ring_floats; i += 256) ring_mine[i] = ring_lds[i];
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace
}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_mu_law_encode(const float* x, int64_t n, int32_t mu_quantization, int64_t* codes, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !codes || n < 0 || mu_quantization < 2, PTMI_E_INVALID);
    if (n == 0) return PTMI_OK;
    hipLaunchKernelGGL(mu_law_encode_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, x, (long long)n, mu_quantization,
                       (long long*)codes);
    return launch_status();
}

int ptmi_mu_law_decode(const void* codes, int32_t codes_are_float, int64_t n, int32_t mu_quantization, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!codes || !out || n < 0 || mu_quantization < 2, PTMI_E_INVALID);
    if (n == 0) return PTMI_OK;
    if (codes_are_float)
        hipLaunchKernelGGL(mu_law_decode_kernel<float>, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, (const float*)codes, (long long)n,
                           mu_quantization, out);
    else
        hipLaunchKernelGGL(mu_law_decode_kernel<long long>, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, (const long long*)codes,
                           (long long)n, mu_quantization, out);
    return launch_status();
}

int ptmi_wavenet_embed_forward(const float* audio, const float* embed, int64_t n, int32_t A, int32_t R, int64_t* codes, float* x0,
                               ptmi_stream_t stream) {
    PTMI_RETURN_IF(!audio || !embed || !codes || !x0 || n < 0 || A < 2 || R < 1, PTMI_E_INVALID);
    if (n == 0) return PTMI_OK;
    hipLaunchKernelGGL(embed_forward_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, audio, embed, (long long)n, A, R,
                       (long long*)codes, x0);
    return launch_status();
}

int64_t ptmi_wavenet_embed_workspace_elems(int64_t n, int32_t A, int32_t R) {
    return (n + kEmbedRows - 1) / kEmbedRows * (int64_t)A * R;
}

int ptmi_wavenet_embed_backward(const float* dx0, const int64_t* codes, int64_t n, int32_t A, int32_t R, float* dembed, double* workspace,
                                ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dx0 || !codes || !dembed || !workspace || n < 1 || A < 2 || R < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(R > 256 || A > 65535, PTMI_E_UNSUPPORTED);
    const long long slabs = (n + kEmbedRows - 1) / kEmbedRows;
    PTMI_RETURN_IF(slabs > 65535, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(embed_backward_kernel, dim3(A, (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, dx0, (const long long*)codes,
                       (long long)n, A, R, workspace);
    if (const int rc = launch_status()) return rc;
    return colreduce(workspace, slabs, (long long)A * R, StorePlain{dembed}, (hipStream_t)stream);
}

int64_t ptmi_wavenet_colsum_workspace_elems(int64_t rows, int32_t width) { return (rows + kColsumRows - 1) / kColsumRows * (int64_t)width; }

int ptmi_wavenet_colsum(const float* x, int64_t rows, int32_t width, int64_t ld, float* out, double* workspace, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !out || !workspace || rows < 1 || width < 1 || ld < width, PTMI_E_INVALID);
    const long long slabs = (rows + kColsumRows - 1) / kColsumRows;
    PTMI_RETURN_IF(slabs > 65535, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(colsum_slab_kernel, dim3((unsigned)((width + 63) / 64), (unsigned)slabs), dim3(256), 0, (hipStream_t)stream, x,
                       (long long)rows, width, (long long)ld, workspace);
    if (const int rc = launch_status()) return rc;
    return colreduce(workspace, slabs, (long long)width, StorePlain{out}, (hipStream_t)stream);
}

int ptmi_wavenet_ola_forward(const float* G, const float* bias, int64_t B, int32_t C, int64_t Tf, int32_t window, int32_t stride,
                             int64_t front, int64_t Tout, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!G || !bias || !out || B < 1 || C < 1 || Tf < 1 || window < 1 || stride < 1 || front < 0 || Tout < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(front + Tout > (Tf - 1) * stride + window, PTMI_E_INVALID);
    PTMI_RETURN_IF(B > 65535 || (C + 3) / 4 > 65535, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(ola_forward_kernel, dim3((unsigned)((Tout + 63) / 64), (unsigned)((C + 3) / 4), (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, G, bias, C, (long long)Tf, window, stride, (long long)front, (long long)Tout, out);
    return launch_status();
}

int ptmi_wavenet_ola_backward(const float* dout, int64_t B, int32_t C, int64_t Tf, int32_t window, int32_t stride, int64_t front,
                              int64_t Tout, float* dG, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dout || !dG || B < 1 || C < 1 || Tf < 1 || window < 1 || stride < 1 || front < 0 || Tout < 1, PTMI_E_INVALID);
    const long long total = (long long)B * Tf * C * window;
    hipLaunchKernelGGL(ola_backward_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, dout, C, (long long)Tf, window, stride,
                       (long long)front, (long long)Tout, total, dG);
    return launch_status();
}

int ptmi_wavenet_gate_forward(const float* P, const float* bias, const float* cond, int64_t ldc, int64_t B, int64_t T, int32_t R,
                              int32_t dilation, float* acts, int64_t lda, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!P || !bias || !cond || !acts || B < 1 || T < 1 || R < 1 || dilation < 1 || ldc < 2 * R || lda < R, PTMI_E_INVALID);
    const long long rows = (long long)B * T;
    const bool vec = R % 4 == 0 && ldc % 4 == 0 && lda % 4 == 0 && aligned16({P, bias, cond, acts});
    PTMI_LAUNCH_VEC(gate_forward_kernel, vec, dim3(blocks_of(rows * (vec ? R / 4 : R))), (hipStream_t)stream, P, bias, cond, (long long)ldc, rows,
                    (long long)T, R, dilation, acts, (long long)lda);
    return launch_status();
}

int ptmi_wavenet_gate_backward(const float* dacts, int64_t lda, const float* P, const float* bias, const float* cond, int64_t ldc, int64_t B,
                               int64_t T, int32_t R, int32_t dilation, float* dz, int64_t ldd, float* dP, float* dbias, double* workspace,
                               ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dacts || !P || !bias || !cond || !dz || B < 1 || T < 1 || R < 1 || dilation < 1 || ldc < 2 * R || lda < R || ldd < 2 * R,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(dbias && !workspace, PTMI_E_INVALID);
    const long long rows = (long long)B * T;
    const bool vec = R % 4 == 0 && ldc % 4 == 0 && lda % 4 == 0 && ldd % 4 == 0 && aligned16({dacts, P, bias, cond, dz, dP});
    PTMI_LAUNCH_VEC(gate_backward_dz_kernel, vec, dim3(blocks_of(rows * (vec ? R / 4 : R))), (hipStream_t)stream, dacts, (long long)lda, P, bias,
                    cond, (long long)ldc, rows, (long long)T, R, dilation, dz, (long long)ldd);
    if (const int rc = launch_status()) return rc;
    if (dP) {
        PTMI_LAUNCH_VEC(gate_backward_dp_kernel, vec, dim3(blocks_of(rows * (vec ? 2 * R / 4 : 2 * R))), (hipStream_t)stream, dz, (long long)ldd,
                        rows, (long long)T, R, dilation, dP);
        if (const int rc = launch_status()) return rc;
    }
    if (dbias) return ptmi_wavenet_colsum(dz, rows, 2 * R, ldd, dbias, workspace, stream);
    return PTMI_OK;
}

int32_t ptmi_wavenet_generate_ex(void) { return kEx; }

int32_t ptmi_wavenet_generate_ring_in_lds(int32_t R, int32_t S, int32_t A, int64_t ring_rows) { return gen_ring_in_lds(R, S, A, ring_rows) ? 1 : 0; }

int ptmi_wavenet_generate(const float* packed, const float* embed, const float* cond, const float* u, const int32_t* layer_meta,
                          const int32_t* seq_meta, int32_t nseq, int64_t Tc, int32_t L, int32_t R, int32_t S, int32_t A, int32_t ring_rows,
                          int64_t t0, int32_t nsteps, int64_t Tmax, float* ring, int32_t* last_code, int64_t* y, float* logits,
                          ptmi_stream_t stream) {
    PTMI_RETURN_IF(!packed || !embed || !cond || !u || !layer_meta || !seq_meta || !ring || !last_code || !y, PTMI_E_INVALID);
    PTMI_RETURN_IF(nseq < 1 || Tc < 1 || L < 1 || R < 1 || S < 1 || A < 2 || ring_rows < 1 || t0 < 0 || nsteps < 0 || t0 + nsteps > Tmax,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(R > 256 || S > 1024 || A > 1024, PTMI_E_UNSUPPORTED);
    if (nsteps == 0) return PTMI_OK;
    const int in_lds = gen_ring_in_lds(R, S, A, ring_rows) ? 1 : 0;
    const size_t lds = (size_t)gen_work_floats(R, S, A) * 4 + (in_lds ? (size_t)ring_rows * kEx * R * 4 : 0);
    hipLaunchKernelGGL(generate_kernel, dim3((unsigned)((nseq + kEx - 1) / kEx)), dim3(256), lds, (hipStream_t)stream, packed, embed, cond, u,
                       layer_meta, seq_meta, nseq, (long long)Tc, L, R, S, A, ring_rows, in_lds, (long long)t0, nsteps, (long long)Tmax, ring,
                       last_code, (long long*)y, logits);
    return launch_status();
}

}  // extern "C"
