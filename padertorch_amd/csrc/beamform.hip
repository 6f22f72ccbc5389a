// Mask-based MVDR beamforming (the use of the mask estimators after training: mask_estimator/evaluate.py:110-137 and
// contrib/jensheit/evaluation.py:14-45, whose arithmetic lives in the third-party pb_bss / paderbox).
//
//   psd     Phi_k[b,f,d,e] = sum_t m_k[b,t,f] Y[b,d,t,f] conj(Y[b,e,t,f]) / max(sum_t m_k[b,t,f], 1e-10),  m_k = median_c mask_k[b,c,t,f]
//   souden  X = Phi_n^-1 Phi_s (Gaussian elimination with partial pivoting), M = X / max(Re trace X, DBL_MIN), w = M[:, ref]
//   apply   Z[b,t,f] = sum_c conj(w[b,f,c]) X_in[b,c,t,f]
//
// Layout: Y and X_in [B, C, T, F] complex64 (interleaved), masks [B, C, T, F] or [B, T, F] fp32, Phi [B, F, C, C] complex128,
// w [B, F, C] complex64; frames [B] int32 (frames t >= frames[b] contribute nothing, are never loaded and come out as zero).
//
// Conventions of orpit.hip / td_loss.hip: fp32 data and fp32 products, every running sum fp64, no atomics, partials in a caller-owned
// workspace of doubles added in ONE fixed order (bit-reproducible), no allocation and no synchronisation (capturable).  In the two
// streaming kernels a lane owns one frequency bin and a wavefront reads 64 consecutive bins (512 contiguous bytes of Y per channel and
// frame); the four waves of a workgroup share the frames of its time chunk.
#include <float.h>

#include "reduce.h"

namespace ptmi {

constexpr int kBfMaxChannels = 8;
constexpr int kBfSoudenLanes = 16;   // bins per workgroup of the solve: 2 C C complex128 per bin live in LDS (32 KiB at C = 8)

// ---- PSD ----------------------------------------------------------------------------------------------------------------------------
struct BfPsdArgs {
    const float2* Y;          // [B, C, T, F]
    const float* mask[2];     // MODE 1: [B, T, F]; MODE 2: [B, C, T, F]; MODE 0: unused (m = 1)
    const int32_t* frames;    // [B] or null
    double* ws;               // [B][nfb][S][M (C C + 1)][64]
    long long T, F, chunk;    // chunk: frames per workgroup
    int S;
};

// Compare-exchange network (odd-even transposition, C rounds): v ascending.  C is a compile-time constant and every index is one after
// unrolling, so the values stay in registers.
template <int C>
__device__ __forceinline__ float median_of(float (&v)[C]) {
#pragma unroll
    for (int r = 0; r < C; ++r)
#pragma unroll
        for (int i = r & 1; i + 1 < C; i += 2) {
            const float lo = fminf(v[i], v[i + 1]), hi = fmaxf(v[i], v[i + 1]);
            v[i] = lo;
            v[i + 1] = hi;
        }
    if constexpr (C % 2 == 1)
        return v[C / 2];
    else
        return __fmul_rn(__fadd_rn(v[C / 2 - 1], v[C / 2]), 0.5f);     // numpy: the mean of the two middle values
}

// Accumulators of one mask: [0, C) the real diagonal, then (re, im) of the pairs d < e in row order, then sum_t m.
// MODE 0: no mask (m = 1), 1: masks already reduced over the channels, 2: the channel median is taken here.
// Grid (nfb, B, S), 256 threads: wave w takes frames t0 + w, t0 + w + 4, ... of the workgroup's chunk; the waves' partials are added
// through LDS in the order ((0 + 1) + 2) + 3 and the workgroup's slab goes to the workspace.
// A wave loads U of its frames (all their rows of Y and of the masks) before it does arithmetic on any: with up to 2 (C C + 1) fp64
// accumulators a lane the occupancy is one or two waves per SIMD, and the bytes in flight have to come from each wave.
template <int C, int M, int MODE>
__global__ __launch_bounds__(256) void bf_psd_kernel(const BfPsdArgs A) {
    constexpr int NA = C * C + 1, TOT = M * NA, G = 13, U = TOT > 100 ? 2 : 4;
    constexpr int MC = MODE == 2 ? C : 1;      // mask values a frame loads per mask
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.y, s = blockIdx.z, f = (long long)blockIdx.x * 64 + lane;
    const bool live = f < A.F;
    long long nf = A.frames ? (long long)A.frames[b] : A.T;
    nf = nf < 0 ? 0 : (nf > A.T ? A.T : nf);
    const long long t0 = s * A.chunk, t1 = min(t0 + A.chunk, nf);
    double acc[TOT];
#pragma unroll
    for (int i = 0; i < TOT; ++i) acc[i] = 0.0;
    if (live) {
        for (long long t = t0 + wave; t < t1; t += 4 * U) {
            float2 y[U][C];
            float mv[U][M][MC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long tu = min(t + 4 * u, t1 - 1);       // (a frame past the chunk: a valid address, the values are not used)
#pragma unroll
                for (int c = 0; c < C; ++c) y[u][c] = A.Y[((b * C + c) * A.T + tu) * A.F + f];
                if constexpr (MODE != 0) {
#pragma unroll
                    for (int k = 0; k < M; ++k)
#pragma unroll
                        for (int c = 0; c < MC; ++c)
                            mv[u][k][c] = A.mask[k][(MODE == 2 ? (b * C + c) * A.T + tu : b * A.T + tu) * A.F + f];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (t + 4 * u >= t1) break;
                float m[M];
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    if constexpr (MODE == 0)
                        m[k] = 1.f;
                    else if constexpr (MODE == 1)
                        m[k] = mv[u][k][0];
                    else
                        m[k] = median_of<C>(mv[u][k]);
                }
#pragma unroll
                for (int d = 0; d < C; ++d) {
                    const float p = fmaf(y[u][d].x, y[u][d].x, __fmul_rn(y[u][d].y, y[u][d].y));
#pragma unroll
                    for (int k = 0; k < M; ++k) acc[k * NA + d] += (double)__fmul_rn(m[k], p);
                }
                int i = C;
#pragma unroll
                for (int d = 0; d < C; ++d)
#pragma unroll
                    for (int e = d + 1; e < C; ++e, i += 2) {      // Y_d conj(Y_e)
                        const float re = fmaf(y[u][d].x, y[u][e].x, __fmul_rn(y[u][d].y, y[u][e].y));
                        const float im = fmaf(y[u][d].y, y[u][e].x, -__fmul_rn(y[u][d].x, y[u][e].y));
#pragma unroll
                        for (int k = 0; k < M; ++k) {
                            acc[k * NA + i] += (double)__fmul_rn(m[k], re);
                            acc[k * NA + i + 1] += (double)__fmul_rn(m[k], im);
                        }
                    }
#pragma unroll
                for (int k = 0; k < M; ++k) acc[k * NA + NA - 1] += (double)m[k];
            }
        }
    }
    __shared__ double red[3][G][64];
    double* out = A.ws + (((b * gridDim.x + blockIdx.x) * A.S + s) * TOT) * 64 + lane;
#pragma unroll
    for (int g0 = 0; g0 < TOT; g0 += G) {
        if (wave > 0) {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (g0 + j < TOT) red[wave - 1][j][lane] = acc[g0 + j];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (g0 + j < TOT) out[(long long)(g0 + j) * 64] = ((acc[g0 + j] + red[0][j][lane]) + red[1][j][lane]) + red[2][j][lane];
        }
        __syncthreads();
    }
}

// Phi[k, b, f] from the S slabs of a bin in ascending order; both triangles from the one sum.  Grid (nfb, B, M), 64 threads.
__global__ __launch_bounds__(64) void bf_psd_finish_kernel(const double* __restrict__ ws, double* __restrict__ psd, long long B, long long F,
                                                           int C, int M, int S, int normalize) {
    const int lane = threadIdx.x, k = blockIdx.z;
    const long long b = blockIdx.y, f = (long long)blockIdx.x * 64 + lane;
    if (f >= F) return;
    const int NA = C * C + 1, TOT = M * NA;
    const double* base = ws + ((b * gridDim.x + blockIdx.x) * S) * (long long)TOT * 64 + lane;
    auto total = [&](int i) {
        double v = 0.0;
        for (int s = 0; s < S; ++s) v += base[((long long)s * TOT + k * NA + i) * 64];
        return v;
    };
    const double den = normalize ? fmax(total(NA - 1), 1e-10) : 1.0;
    double* P = psd + ((k * B + b) * F + f) * (long long)C * C * 2;
    int i = C;
    for (int d = 0; d < C; ++d) {
        P[(d * C + d) * 2] = total(d) / den;
        P[(d * C + d) * 2 + 1] = 0.0;
        for (int e = d + 1; e < C; ++e, i += 2) {
            const double re = total(i) / den, im = total(i + 1) / den;
            P[(d * C + e) * 2] = re;
            P[(d * C + e) * 2 + 1] = im;
            P[(e * C + d) * 2] = re;
            P[(e * C + d) * 2 + 1] = -im;
        }
    }
}

static void bf_psd_plan(long long B, long long T, long long F, long long* chunk, int* S) {
    const long long nfb = (F + 63) / 64;
    long long want = (512 + B * nfb - 1) / (B * nfb);      // ~512 workgroups when the frames allow it, at least 16 frames each
    const long long most = (T + 15) / 16;
    if (want > most) want = most;
    if (want < 1) want = 1;
    *chunk = (T + want - 1) / want;
    *S = (int)((T + *chunk - 1) / *chunk);
}

template <int C, int M>
static int launch_bf_psd(const BfPsdArgs& A, int mode, dim3 grid, hipStream_t st) {
    if (mode == 2)
        hipLaunchKernelGGL((bf_psd_kernel<C, M, 2>), grid, dim3(256), 0, st, A);
    else if (mode == 1)
        hipLaunchKernelGGL((bf_psd_kernel<C, M, 1>), grid, dim3(256), 0, st, A);
    else
        hipLaunchKernelGGL((bf_psd_kernel<C, 1, 0>), grid, dim3(256), 0, st, A);
    return launch_status();
}

template <int C>
static int dispatch_bf_psd(const BfPsdArgs& A, int M, int mode, dim3 grid, hipStream_t st) {
    return M == 2 ? launch_bf_psd<C, 2>(A, mode, grid, st) : launch_bf_psd<C, 1>(A, mode, grid, st);
}

// ---- Souden MVDR ----------------------------------------------------------------------------------------------------------------------
// One lane per (b, f), fp64.  The lane's two C x C matrices live in LDS ([element][lane]: no bank conflicts, indices may be dynamic
// without scratch); no lane reads another lane's values, so there is no barrier.
__global__ __launch_bounds__(kBfSoudenLanes) void bf_souden_kernel(const double* __restrict__ ps, const double* __restrict__ pn,
                                                                   float2* __restrict__ w_all, double* __restrict__ numden, long long BF,
                                                                   int C, int want_numden) {
    extern __shared__ double sm[];
    constexpr int L = kBfSoudenLanes;
    const int lane = threadIdx.x;
    const long long bin = (long long)blockIdx.x * L + lane;
    if (bin >= BF) return;
    const int CC = C * C;
    double* a = sm + lane;                  // a[((r C + c) 2 + part) L]: Phi_n, eliminated in place
    double* x = sm + 2 * CC * L + lane;     // Phi_s, then X
    const double* Ps = ps + bin * CC * 2;
    const double* Pn = pn + bin * CC * 2;
    for (int i = 0; i < 2 * CC; ++i) {
        a[i * L] = Pn[i];
        x[i * L] = Ps[i];
    }
#define BF_A(r, c, p) a[(((r) * C + (c)) * 2 + (p)) * L]
#define BF_X(r, c, p) x[(((r) * C + (c)) * 2 + (p)) * L]
    unsigned zero = 0;                      // bit k: the pivot of column k is exactly zero, its unknowns are zero
    for (int k = 0; k < C; ++k) {
        int p = k;
        double best = fabs(BF_A(k, k, 0)) + fabs(BF_A(k, k, 1));
        for (int r = k + 1; r < C; ++r) {
            const double v = fabs(BF_A(r, k, 0)) + fabs(BF_A(r, k, 1));
            if (v > best) {
                best = v;
                p = r;
            }
        }
        if (best == 0.0) {
            zero |= 1u << k;
            continue;
        }
        if (p != k) {
            for (int c = 0; c < C; ++c)
                for (int q = 0; q < 2; ++q) {
                    double t = BF_A(k, c, q);
                    BF_A(k, c, q) = BF_A(p, c, q);
                    BF_A(p, c, q) = t;
                    t = BF_X(k, c, q);
                    BF_X(k, c, q) = BF_X(p, c, q);
                    BF_X(p, c, q) = t;
                }
        }
        const double pr = BF_A(k, k, 0), pi = BF_A(k, k, 1), pd = pr * pr + pi * pi;
        for (int r = k + 1; r < C; ++r) {
            const double ar = BF_A(r, k, 0), ai = BF_A(r, k, 1);
            const double lr = (ar * pr + ai * pi) / pd, li = (ai * pr - ar * pi) / pd;      // a[r][k] / a[k][k]
            for (int c = k + 1; c < C; ++c) {
                const double ur = BF_A(k, c, 0), ui = BF_A(k, c, 1);
                BF_A(r, c, 0) -= lr * ur - li * ui;
                BF_A(r, c, 1) -= lr * ui + li * ur;
            }
            for (int c = 0; c < C; ++c) {
                const double ur = BF_X(k, c, 0), ui = BF_X(k, c, 1);
                BF_X(r, c, 0) -= lr * ur - li * ui;
                BF_X(r, c, 1) -= lr * ui + li * ur;
            }
        }
    }
    for (int k = C - 1; k >= 0; --k) {
        const double pr = BF_A(k, k, 0), pi = BF_A(k, k, 1), pd = pr * pr + pi * pi;
        for (int c = 0; c < C; ++c) {
            double sr = 0.0, si = 0.0;
            if (!((zero >> k) & 1u)) {
                sr = BF_X(k, c, 0);
                si = BF_X(k, c, 1);
                for (int j = k + 1; j < C; ++j) {
                    const double ur = BF_A(k, j, 0), ui = BF_A(k, j, 1), vr = BF_X(j, c, 0), vi = BF_X(j, c, 1);
                    sr -= ur * vr - ui * vi;
                    si -= ur * vi + ui * vr;
                }
                const double qr = (sr * pr + si * pi) / pd, qi = (si * pr - sr * pi) / pd;
                sr = qr;
                si = qi;
            }
            BF_X(k, c, 0) = sr;
            BF_X(k, c, 1) = si;
        }
    }
    double lambda = 0.0;
    for (int k = 0; k < C; ++k) lambda += BF_X(k, k, 0);
    const double den = fmax(lambda, DBL_MIN);
    for (int i = 0; i < CC; ++i) {
        const double re = x[(2 * i) * L] / den, im = x[(2 * i + 1) * L] / den;
        x[(2 * i) * L] = re;
        x[(2 * i + 1) * L] = im;
        w_all[bin * CC + i] = make_float2((float)re, (float)im);
    }
    if (!want_numden) return;
    // Re(w_r^H Phi w_r) for w_r = M[:, r], Phi = Phi_s | Phi_n (read again: the solve has overwritten them)
    for (int r = 0; r < C; ++r) {
        double num = 0.0, dn = 0.0;
        for (int d = 0; d < C; ++d) {
            double sr = 0.0, si = 0.0, nr = 0.0, ni = 0.0;
            for (int e = 0; e < C; ++e) {
                const double vr = BF_X(e, r, 0), vi = BF_X(e, r, 1);
                const double a0 = Ps[(d * C + e) * 2], a1 = Ps[(d * C + e) * 2 + 1];
                const double b0 = Pn[(d * C + e) * 2], b1 = Pn[(d * C + e) * 2 + 1];
                sr += a0 * vr - a1 * vi;
                si += a0 * vi + a1 * vr;
                nr += b0 * vr - b1 * vi;
                ni += b0 * vi + b1 * vr;
            }
            const double wr = BF_X(d, r, 0), wi = BF_X(d, r, 1);
            num += wr * sr + wi * si;
            dn += wr * nr + wi * ni;
        }
        numden[(bin * C + r) * 2] = num;
        numden[(bin * C + r) * 2 + 1] = dn;
    }
#undef BF_A
#undef BF_X
}

// One workgroup per example: ref_in < 0: the sums of numden over the bins (a thread adds its bins f = x, x + 256, ... ascending, then
// block_sums), ref = argmax_r num_r / max(den_r, DBL_MIN), first maximum; then the gather w[b, f, :] = w_all[b, f, :, ref].
__global__ __launch_bounds__(256) void bf_pick_kernel(const double* __restrict__ numden, const float2* __restrict__ w_all,
                                                      float2* __restrict__ w, int32_t* __restrict__ ref_out, long long F, int C, int ref_in) {
    const long long b = blockIdx.x;
    __shared__ int sref;
    if (ref_in < 0) {
        double s[2 * kBfMaxChannels];
#pragma unroll
        for (int i = 0; i < 2 * kBfMaxChannels; ++i) s[i] = 0.0;
        for (long long f = threadIdx.x; f < F; f += 256) {
            const double* nd = numden + (b * F + f) * C * 2;
#pragma unroll
            for (int i = 0; i < 2 * kBfMaxChannels; ++i)
                if (i < 2 * C) s[i] += nd[i];
        }
        block_sums(s);
        if (threadIdx.x == 0) {
            int best = 0;
            double best_ratio = 0.0;
#pragma unroll
            for (int r = 0; r < kBfMaxChannels; ++r) {
                const double ratio = s[2 * r] / fmax(s[2 * r + 1], DBL_MIN);
                if (r < C && (r == 0 || ratio > best_ratio)) {
                    best = r;
                    best_ratio = ratio;
                }
            }
            sref = best;
        }
    } else if (threadIdx.x == 0) {
        sref = ref_in;
    }
    __syncthreads();
    const int ref = sref;
    if (threadIdx.x == 0) ref_out[b] = ref;
    for (long long i = threadIdx.x; i < F * C; i += 256) w[b * F * C + i] = w_all[(b * F * C + i) * C + ref];
}

// ---- apply --------------------------------------------------------------------------------------------------------------------------
// Grid (nfb, ceil(T / 32), B), 256 threads: a lane holds its bin's C weights in registers, wave w takes frames t0 + w, t0 + w + 4, ...;
// 8-byte loads and stores, 512 contiguous bytes per wave and row.
template <int C>
__global__ __launch_bounds__(256) void bf_apply_kernel(const float2* __restrict__ w, const float2* __restrict__ X,
                                                       const int32_t* __restrict__ frames, float2* __restrict__ Z, long long T, long long F) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.z, f = (long long)blockIdx.x * 64 + lane;
    if (f >= F) return;
    long long nf = frames ? (long long)frames[b] : T;
    nf = nf < 0 ? 0 : (nf > T ? T : nf);
    const long long t0 = (long long)blockIdx.y * 32, t1 = min(t0 + 32, T);
    float2 wv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) wv[c] = w[(b * F + f) * C + c];
    for (long long t = t0 + wave; t < t1; t += 4) {
        float2 z = make_float2(0.f, 0.f);
        if (t < nf) {
            float2 xv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) xv[c] = X[((b * C + c) * T + t) * F + f];
#pragma unroll
            for (int c = 0; c < C; ++c) {       // conj(w) x
                z.x = fmaf(wv[c].x, xv[c].x, fmaf(wv[c].y, xv[c].y, z.x));
                z.y = fmaf(wv[c].x, xv[c].y, fmaf(-wv[c].y, xv[c].x, z.y));
            }
        }
        Z[(b * T + t) * F + f] = z;
    }
}

template <int C>
static int launch_bf_apply(const float* w, const float* X, const int32_t* frames, float* Z, long long B, long long T, long long F,
                           hipStream_t st) {
    const dim3 grid((unsigned)((F + 63) / 64), (unsigned)((T + 31) / 32), (unsigned)B);
    hipLaunchKernelGGL((bf_apply_kernel<C>), grid, dim3(256), 0, st, reinterpret_cast<const float2*>(w), reinterpret_cast<const float2*>(X),
                       frames, reinterpret_cast<float2*>(Z), T, F);
    return launch_status();
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_bf_psd_workspace_elems(int64_t B, int32_t C, int64_t T, int64_t F, int32_t M) {
    if (B < 1 || C < 1 || T < 1 || F < 1 || M < 1 || M > 2) return PTMI_E_INVALID;
    if (C > kBfMaxChannels) return PTMI_E_UNSUPPORTED;
    long long chunk;
    int S;
    bf_psd_plan(B, T, F, &chunk, &S);
    return B * ((F + 63) / 64) * S * (int64_t)M * (C * C + 1) * 64;
}

int ptmi_bf_psd(const float* Y, const float* mask0, const float* mask1, const int32_t* frames, int64_t B, int32_t C, int64_t T, int64_t F,
                int32_t M, int32_t mask_mode, int32_t normalize, double* workspace, double* psd, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!Y || !workspace || !psd, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || C < 1 || T < 1 || F < 1 || M < 1 || M > 2 || mask_mode < 0 || mask_mode > 2, PTMI_E_INVALID);
    PTMI_RETURN_IF(mask_mode == 0 ? M != 1 : (!mask0 || (M == 2 && !mask1)), PTMI_E_INVALID);
    PTMI_RETURN_IF(C > kBfMaxChannels || B > 65535 || T > 2147483647LL / 64, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    BfPsdArgs A{};
    A.Y = reinterpret_cast<const float2*>(Y);
    A.mask[0] = mask0;
    A.mask[1] = mask1;
    A.frames = frames;
    A.ws = workspace;
    A.T = T;
    A.F = F;
    bf_psd_plan(B, T, F, &A.chunk, &A.S);
    const unsigned nfb = (unsigned)((F + 63) / 64);
    const dim3 grid(nfb, (unsigned)B, (unsigned)A.S);
    int rc;
    switch (C) {
        case 1: rc = dispatch_bf_psd<1>(A, M, mask_mode, grid, st); break;
        case 2: rc = dispatch_bf_psd<2>(A, M, mask_mode, grid, st); break;
        case 3: rc = dispatch_bf_psd<3>(A, M, mask_mode, grid, st); break;
        case 4: rc = dispatch_bf_psd<4>(A, M, mask_mode, grid, st); break;
        case 5: rc = dispatch_bf_psd<5>(A, M, mask_mode, grid, st); break;
        case 6: rc = dispatch_bf_psd<6>(A, M, mask_mode, grid, st); break;
        case 7: rc = dispatch_bf_psd<7>(A, M, mask_mode, grid, st); break;
        default: rc = dispatch_bf_psd<8>(A, M, mask_mode, grid, st); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(bf_psd_finish_kernel, dim3(nfb, (unsigned)B, (unsigned)M), dim3(64), 0, st, workspace, psd, (long long)B, (long long)F,
                       C, M, A.S, normalize);
    return launch_status();
}

int ptmi_bf_souden(const double* psd_target, const double* psd_noise, int64_t B, int64_t F, int32_t C, int32_t ref_channel, float* w_all,
                   double* numden, float* w, int32_t* ref_out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!psd_target || !psd_noise || !w_all || !w || !ref_out || (ref_channel < 0 && !numden), PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || F < 1 || C < 1 || ref_channel >= C, PTMI_E_INVALID);
    PTMI_RETURN_IF(C > kBfMaxChannels || B > 2147483647LL || B * F > 2147483647LL * kBfSoudenLanes, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long BF = B * F;
    const size_t lds = (size_t)4 * C * C * kBfSoudenLanes * sizeof(double);
    hipLaunchKernelGGL(bf_souden_kernel, dim3((unsigned)((BF + kBfSoudenLanes - 1) / kBfSoudenLanes)), dim3(kBfSoudenLanes), lds, st,
                       psd_target, psd_noise, reinterpret_cast<float2*>(w_all), numden, BF, C, ref_channel < 0);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(bf_pick_kernel, dim3((unsigned)B), dim3(256), 0, st, numden, reinterpret_cast<const float2*>(w_all),
                       reinterpret_cast<float2*>(w), ref_out, (long long)F, C, ref_channel);
    return launch_status();
}

int ptmi_bf_apply(const float* w, const float* X, const int32_t* frames, int64_t B, int32_t C, int64_t T, int64_t F, float* Z,
                  ptmi_stream_t stream) {
    PTMI_RETURN_IF(!w || !X || !Z, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || C < 1 || T < 1 || F < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(C > kBfMaxChannels || B > 65535 || (T + 31) / 32 > 65535, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (C) {
        case 1: return launch_bf_apply<1>(w, X, frames, Z, B, T, F, st);
        case 2: return launch_bf_apply<2>(w, X, frames, Z, B, T, F, st);
        case 3: return launch_bf_apply<3>(w, X, frames, Z, B, T, F, st);
        case 4: return launch_bf_apply<4>(w, X, frames, Z, B, T, F, st);
        case 5: return launch_bf_apply<5>(w, X, frames, Z, B, T, F, st);
        case 6: return launch_bf_apply<6>(w, X, frames, Z, B, T, F, st);
        case 7: return launch_bf_apply<7>(w, X, frames, Z, B, T, F, st);
        default: return launch_bf_apply<8>(w, X, frames, Z, B, T, F, st);
    }
}

}  // extern "C"
