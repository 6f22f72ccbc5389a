// Mask-based MVDR beamforming (the use of the mask estimators after training: mask_estimator/evaluate.py:110-137 and
// contrib/jensheit/evaluation.py:14-45, whose arithmetic lives in the third-party pb_bss / paderbox).
//
//   psd     Phi_k[b,f,d,e] = sum_t m_k[b,t,f] Y[b,d,t,f] conj(Y[b,e,t,f]) / max(sum_t m_k[b,t,f], 1e-10),  m_k = median_c mask_k[b,c,t,f]
//   souden  X = Phi_n^-1 Phi_s (Gaussian elimination with partial pivoting), M = X / max(Re trace X, DBL_MIN), w = M[:, ref]
//   apply   Z[b,t,f] = sum_c conj(w[b,f,c]) X_in[b,c,t,f]
//   eig     gev: Phi_n = L L^H, A = L^-1 Phi_s L^-H, cyclic complex Jacobi, v of the largest eigenvalue, w = L^-H v (w^H Phi_n w = 1);
//           pca: the same Jacobi on Phi_s, |w| = 1; gauge: the largest component real and positive
//   ban     w sqrt(|w^H Phi_n Phi_n w|) / max(|w^H Phi_n w|, DBL_MIN)
//   phase   w'_f = w_f exp(-i arg(sum_c w_f,c conj(w'_{f-1},c))) along the bins, as a scan of unit phasors
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

// ---- GEV / PCA ------------------------------------------------------------------------------------------------------------------------
// One bin's principal (generalized) eigenvector in fp64, on three C x C complex matrices of the bin that are addressed as
// m[((r C + c) 2 + part) L] (the [element][lane] layout of bf_souden_kernel with L lanes; L = 1 on the host):
//   l   Phi_n, then its Cholesky factor in the lower triangle (mode gev only)
//   a   Phi_s, then A = L^-1 Phi_s L^-H (gev) or Phi_s itself (pca), then what the Jacobi rotations leave of it
//   v   the accumulated rotations
// Returns the sweeps done and leaves w in a[(2 c + part) L], c < C.  Every product is an explicit fma or stands alone, so the host and
// the device build of this function round alike.
#define BF_M(m, r, c, p) m[(((r) * C + (c)) * 2 + (p)) * L]

// Cholesky of the lower triangle in place; false when a pivot is not > 0 (zero, indefinite, NaN).
__host__ __device__ inline bool bf_cholesky(double* l, int C, int L) {
    for (int j = 0; j < C; ++j) {
        double d = BF_M(l, j, j, 0);
        for (int k = 0; k < j; ++k) d = fma(-BF_M(l, j, k, 0), BF_M(l, j, k, 0), fma(-BF_M(l, j, k, 1), BF_M(l, j, k, 1), d));
        if (!(d > 0.0)) return false;
        const double dj = sqrt(d);
        BF_M(l, j, j, 0) = dj;
        BF_M(l, j, j, 1) = 0.0;
        for (int i = j + 1; i < C; ++i) {
            double sr = BF_M(l, i, j, 0), si = BF_M(l, i, j, 1);
            for (int k = 0; k < j; ++k) {      // - L_ik conj(L_jk)
                const double ar = BF_M(l, i, k, 0), ai = BF_M(l, i, k, 1), br = BF_M(l, j, k, 0), bi = BF_M(l, j, k, 1);
                sr = fma(-ar, br, fma(-ai, bi, sr));
                si = fma(-ai, br, fma(ar, bi, si));
            }
            BF_M(l, i, j, 0) = sr / dj;
            BF_M(l, i, j, 1) = si / dj;
        }
    }
    return true;
}

// a <- L^-1 a L^-H by two triangular solves (not an inverse).
__host__ __device__ inline void bf_whiten(const double* l, double* a, int C, int L) {
    for (int c = 0; c < C; ++c)                // X = L^-1 a, column by column
        for (int i = 0; i < C; ++i) {
            double sr = BF_M(a, i, c, 0), si = BF_M(a, i, c, 1);
            for (int k = 0; k < i; ++k) {      // - L_ik X_kc
                const double ar = BF_M(l, i, k, 0), ai = BF_M(l, i, k, 1), br = BF_M(a, k, c, 0), bi = BF_M(a, k, c, 1);
                sr = fma(-ar, br, fma(ai, bi, sr));
                si = fma(-ar, bi, fma(-ai, br, si));
            }
            const double d = BF_M(l, i, i, 0);
            BF_M(a, i, c, 0) = sr / d;
            BF_M(a, i, c, 1) = si / d;
        }
    for (int r = 0; r < C; ++r)                // A L^H = X, row by row
        for (int j = 0; j < C; ++j) {
            double sr = BF_M(a, r, j, 0), si = BF_M(a, r, j, 1);
            for (int k = 0; k < j; ++k) {      // - A_rk conj(L_jk)
                const double ar = BF_M(a, r, k, 0), ai = BF_M(a, r, k, 1), br = BF_M(l, j, k, 0), bi = BF_M(l, j, k, 1);
                sr = fma(-ar, br, fma(-ai, bi, sr));
                si = fma(-ai, br, fma(ar, bi, si));
            }
            const double d = BF_M(l, j, j, 0);
            BF_M(a, r, j, 0) = sr / d;
            BF_M(a, r, j, 1) = si / d;
        }
}

// a <- (a + a^H) / 2: exactly Hermitian, a real diagonal (an exactly Hermitian a is left as it is).
__host__ __device__ inline void bf_hermitian(double* a, int C, int L) {
    for (int p = 0; p < C; ++p) {
        BF_M(a, p, p, 1) = 0.0;
        for (int q = p + 1; q < C; ++q) {
            const double re = 0.5 * (BF_M(a, p, q, 0) + BF_M(a, q, p, 0)), im = 0.5 * (BF_M(a, p, q, 1) - BF_M(a, q, p, 1));
            BF_M(a, p, q, 0) = re;
            BF_M(a, p, q, 1) = im;
            BF_M(a, q, p, 0) = re;
            BF_M(a, q, p, 1) = -im;
        }
    }
}

// Cyclic complex Jacobi on the Hermitian a (pairs p < q in row order): a <- J^H a J, v <- v J with J_pp = J_qq = c, J_pq = s e,
// J_qp = -s conj(e), e = a_pq / |a_pq|, t = s / c the smaller root of t^2 + 2 tau t - 1 = 0, tau = (a_qq - a_pp) / (2 |a_pq|).
// Both triangles are written from the one new value, so a stays exactly Hermitian.  A sweep starts while
// off(a)^2 = 2 sum_{p<q} |a_pq|^2 > (2^-52)^2 ||a||_F^2 (the norm is invariant: taken once), at most kBfMaxSweeps times.
constexpr int kBfMaxSweeps = 16;

__host__ __device__ inline int bf_jacobi(double* __restrict__ a, double* __restrict__ v, int C, int L, double fro2) {
    for (int r = 0; r < C; ++r)
        for (int c = 0; c < C; ++c) {
            BF_M(v, r, c, 0) = r == c ? 1.0 : 0.0;
            BF_M(v, r, c, 1) = 0.0;
        }
    const double limit = (DBL_EPSILON * DBL_EPSILON) * fro2;
    int sweeps = 0;
    for (; sweeps < kBfMaxSweeps; ++sweeps) {
        double off2 = 0.0;
        for (int p = 0; p < C; ++p)
            for (int q = p + 1; q < C; ++q) off2 = fma(BF_M(a, p, q, 0), BF_M(a, p, q, 0), fma(BF_M(a, p, q, 1), BF_M(a, p, q, 1), off2));
        if (2.0 * off2 <= limit) break;
        for (int p = 0; p < C; ++p)
            for (int q = p + 1; q < C; ++q) {
                const double xr = BF_M(a, p, q, 0), xi = BF_M(a, p, q, 1), g = hypot(xr, xi);
                if (!(g > 0.0)) continue;
                const double ig = 1.0 / g, er = xr * ig, ei = xi * ig;      // (one division for e and tau: the chain is the kernel's time)
                const double tau = (BF_M(a, q, q, 0) - BF_M(a, p, p, 0)) * (0.5 * ig);
                const double t = (tau < 0.0 ? -1.0 : 1.0) / (fabs(tau) + sqrt(fma(tau, tau, 1.0)));
                const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
                const double sr = s * er, si = s * ei;      // s e
                for (int k = 0; k < C; ++k) {
                    // x_kp' = c x_kp - s conj(e) x_kq, x_kq' = s e x_kp + c x_kq for x = a (k != p, q; rows p, q: the conjugates) and
                    // x = v.  All eight values are read before the first store: one LDS round trip a k, not four.
                    const double pr = BF_M(a, k, p, 0), pi = BF_M(a, k, p, 1), qr = BF_M(a, k, q, 0), qi = BF_M(a, k, q, 1);
                    const double ur = BF_M(v, k, p, 0), ui = BF_M(v, k, p, 1), wr = BF_M(v, k, q, 0), wi = BF_M(v, k, q, 1);
                    if (k != p && k != q) {
                        const double npr = fma(c, pr, fma(-sr, qr, -(si * qi))), npi = fma(c, pi, fma(-sr, qi, si * qr));
                        const double nqr = fma(c, qr, fma(sr, pr, -(si * pi))), nqi = fma(c, qi, fma(sr, pi, si * pr));
                        BF_M(a, k, p, 0) = npr;
                        BF_M(a, k, p, 1) = npi;
                        BF_M(a, p, k, 0) = npr;
                        BF_M(a, p, k, 1) = -npi;
                        BF_M(a, k, q, 0) = nqr;
                        BF_M(a, k, q, 1) = nqi;
                        BF_M(a, q, k, 0) = nqr;
                        BF_M(a, q, k, 1) = -nqi;
                    }
                    BF_M(v, k, p, 0) = fma(c, ur, fma(-sr, wr, -(si * wi)));
                    BF_M(v, k, p, 1) = fma(c, ui, fma(-sr, wi, si * wr));
                    BF_M(v, k, q, 0) = fma(c, wr, fma(sr, ur, -(si * ui)));
                    BF_M(v, k, q, 1) = fma(c, wi, fma(sr, ui, si * ur));
                }
                BF_M(a, p, p, 0) = fma(-t, g, BF_M(a, p, p, 0));
                BF_M(a, q, q, 0) = fma(t, g, BF_M(a, q, q, 0));
                BF_M(a, p, q, 0) = 0.0;
                BF_M(a, p, q, 1) = 0.0;
                BF_M(a, q, p, 0) = 0.0;
                BF_M(a, q, p, 1) = 0.0;
            }
    }
    return sweeps;
}

// gev != 0: l holds Phi_n and a Phi_s; else a holds the matrix whose principal eigenvector is wanted.  -> w in a[(2 c + part) L],
// *lambda; returns the Jacobi sweeps.  A Cholesky pivot that is not > 0, or an all-zero a, gives w = 0 and lambda = 0.
__host__ __device__ inline int bf_eig_bin(double* l, double* a, double* v, int C, int L, int gev, double* lambda) {
    bool ok = !gev || bf_cholesky(l, C, L);
    if (ok && gev) bf_whiten(l, a, C, L);
    bf_hermitian(a, C, L);
    double fro2 = 0.0;
    for (int i = 0; i < 2 * C * C; ++i) fro2 = fma(a[i * L], a[i * L], fro2);
    ok = ok && fro2 != 0.0;
    int sweeps = 0, top = 0;
    if (ok) {
        sweeps = bf_jacobi(a, v, C, L, fro2);
        for (int k = 1; k < C; ++k)
            if (BF_M(a, k, k, 0) > BF_M(a, top, top, 0)) top = k;
        *lambda = BF_M(a, top, top, 0);
        if (gev)                                // w = L^-H v, in place in the column
            for (int i = C - 1; i >= 0; --i) {
                double sr = BF_M(v, i, top, 0), si = BF_M(v, i, top, 1);
                for (int j = i + 1; j < C; ++j) {       // - conj(L_ji) w_j
                    const double ar = BF_M(l, j, i, 0), ai = BF_M(l, j, i, 1), br = BF_M(v, j, top, 0), bi = BF_M(v, j, top, 1);
                    sr = fma(-ar, br, fma(-ai, bi, sr));
                    si = fma(-ar, bi, fma(ai, br, si));
                }
                const double d = BF_M(l, i, i, 0);
                BF_M(v, i, top, 0) = sr / d;
                BF_M(v, i, top, 1) = si / d;
            }
        int big = 0;                            // the gauge: the component of largest squared magnitude (first maximum) real, positive
        double best = -1.0;
        for (int i = 0; i < C; ++i) {
            const double m = fma(BF_M(v, i, top, 0), BF_M(v, i, top, 0), BF_M(v, i, top, 1) * BF_M(v, i, top, 1));
            if (m > best) {
                best = m;
                big = i;
            }
        }
        const double h = hypot(BF_M(v, big, top, 0), BF_M(v, big, top, 1));
        const double gr = BF_M(v, big, top, 0) / h, gi = BF_M(v, big, top, 1) / h;      // w <- w conj(g)
        for (int i = 0; i < C; ++i) {
            const double wr = BF_M(v, i, top, 0), wi = BF_M(v, i, top, 1);
            a[(2 * i) * L] = i == big ? h : fma(wr, gr, wi * gi);
            a[(2 * i + 1) * L] = i == big ? 0.0 : fma(wi, gr, -(wr * gi));
        }
    } else {
        *lambda = 0.0;
        for (int i = 0; i < 2 * C; ++i) a[i * L] = 0.0;
    }
    return sweeps;
}
#undef BF_M

// Blind analytic normalisation of one bin: w <- w sqrt(|w^H Phi_n Phi_n w|) / max(|w^H Phi_n w|, DBL_MIN), on the stored complex64
// vector, in fp64.  Explicit fmas only: the eigen kernel and the stand-alone kernel give the same bits.  The channel loops are
// unrolled to kBfMaxChannels and guarded, so w and Phi_n w stay in registers.
__device__ __forceinline__ void bf_ban_bin(float2 (&w)[kBfMaxChannels], const double* __restrict__ Pn, int C) {
    double ur[kBfMaxChannels], ui[kBfMaxChannels];
#pragma unroll
    for (int d = 0; d < kBfMaxChannels; ++d) {
        ur[d] = 0.0;
        ui[d] = 0.0;
#pragma unroll
        for (int e = 0; e < kBfMaxChannels; ++e)
            if (d < C && e < C) {
                const double p0 = Pn[(d * C + e) * 2], p1 = Pn[(d * C + e) * 2 + 1], wr = (double)w[e].x, wi = (double)w[e].y;
                ur[d] = fma(p0, wr, fma(-p1, wi, ur[d]));
                ui[d] = fma(p0, wi, fma(p1, wr, ui[d]));
            }
    }
    double nr = 0.0, ni = 0.0, dr = 0.0, di = 0.0;      // w^H (Phi_n u) and w^H u, u = Phi_n w
#pragma unroll
    for (int d = 0; d < kBfMaxChannels; ++d) {
        double vr = 0.0, vi = 0.0;
#pragma unroll
        for (int e = 0; e < kBfMaxChannels; ++e)
            if (d < C && e < C) {
                const double p0 = Pn[(d * C + e) * 2], p1 = Pn[(d * C + e) * 2 + 1];
                vr = fma(p0, ur[e], fma(-p1, ui[e], vr));
                vi = fma(p0, ui[e], fma(p1, ur[e], vi));
            }
        if (d < C) {
            const double wr = (double)w[d].x, wi = (double)w[d].y;
            nr = fma(wr, vr, fma(wi, vi, nr));
            ni = fma(wr, vi, fma(-wi, vr, ni));
            dr = fma(wr, ur[d], fma(wi, ui[d], dr));
            di = fma(wr, ui[d], fma(-wi, ur[d], di));
        }
    }
    const double scale = sqrt(hypot(nr, ni)) / fmax(hypot(dr, di), DBL_MIN);
#pragma unroll
    for (int d = 0; d < kBfMaxChannels; ++d)
        if (d < C) w[d] = make_float2((float)((double)w[d].x * scale), (float)((double)w[d].y * scale));
}

// One lane per (b, f) as in bf_souden_kernel, three matrices a lane: 768 C C bytes of LDS a workgroup of kBfEigLanes = 16 lanes,
// 48 KiB at C = 8.  Why 16: the kernel is a chain of dependent fp64 and LDS operations per lane on a few hundred to a few thousand
// bins, so its time is one lane's latency and what counts is how many CUs the bins reach: 513 bins make 33 workgroups on 33 CUs
// (a full wave a workgroup: 9); three workgroups fit the 160 KiB of a CU at C = 8, and a row of 16 doubles covers 32 banks once.
constexpr int kBfEigLanes = 16;

__global__ __launch_bounds__(kBfEigLanes) void bf_eig_kernel(const double* __restrict__ ps, const double* __restrict__ pn,
                                                             float2* __restrict__ w, double* __restrict__ lambda,
                                                             int32_t* __restrict__ sweeps, long long BF, int C, int gev, int ban) {
    extern __shared__ double sm[];
    constexpr int L = kBfEigLanes;
    const int lane = threadIdx.x;
    const long long bin = (long long)blockIdx.x * L + lane;
    if (bin >= BF) return;
    const int CC = C * C;
    double* l = sm + lane;
    double* a = sm + 2 * CC * L + lane;
    double* v = sm + 4 * CC * L + lane;
    const double* Ps = ps + bin * CC * 2;
    const double* Pn = pn ? pn + bin * CC * 2 : nullptr;
    for (int i = 0; i < 2 * CC; ++i) {
        a[i * L] = Ps[i];
        if (gev) l[i * L] = Pn[i];
    }
    double lam;
    const int n = bf_eig_bin(l, a, v, C, L, gev, &lam);
    float2 wf[kBfMaxChannels];
#pragma unroll
    for (int c = 0; c < kBfMaxChannels; ++c)
        wf[c] = c < C ? make_float2((float)a[(2 * c) * L], (float)a[(2 * c + 1) * L]) : make_float2(0.f, 0.f);
    if (ban) bf_ban_bin(wf, Pn, C);             // Phi_n from global memory again: the factorisation has overwritten it
#pragma unroll
    for (int c = 0; c < kBfMaxChannels; ++c)
        if (c < C) w[bin * C + c] = wf[c];
    lambda[bin] = lam;
    if (sweeps) sweeps[bin] = n;
}

// Grid ceil(B F / 256), 256 threads: a lane normalises one bin.
__global__ __launch_bounds__(256) void bf_ban_kernel(const float2* __restrict__ w, const double* __restrict__ pn, float2* __restrict__ out,
                                                     long long BF, int C) {
    const long long bin = (long long)blockIdx.x * 256 + threadIdx.x;
    if (bin >= BF) return;
    float2 wf[kBfMaxChannels];
#pragma unroll
    for (int c = 0; c < kBfMaxChannels; ++c) wf[c] = c < C ? w[bin * C + c] : make_float2(0.f, 0.f);
    bf_ban_bin(wf, pn + bin * C * C * 2, C);
#pragma unroll
    for (int c = 0; c < kBfMaxChannels; ++c)
        if (c < C) out[bin * C + c] = wf[c];
}

// ---- phase correction -----------------------------------------------------------------------------------------------------------------
// w'_f = c_f w_f with c_0 = 1 and c_f = c_{f-1} conj(d_f / |d_f|), d_f = sum_c w_f,c conj(w_{f-1},c) on the stored vectors; a d_f that is
// exactly zero STARTS AGAIN at c_f = 1 (the serial definition: the rotation is by arg 0 = 0 against a zero or orthogonal corrected
// neighbour).  That is a segmented inclusive scan of unit phasors: an element is (restart, phasor), and
//   (r1, p1) then (r2, p2)  =  r2 ? (1, p2) : (r1, p1 p2).
// One workgroup per example, ONE fixed order for any F: thread x owns the K = ceil(F / 256) consecutive bins from x K, combines them
// ascending, the 256 totals go through a Hillis-Steele scan in LDS (8 steps, distances 1, 2, .. 128, earlier operand on the left),
// and the thread walks its bins again from the total of the threads before it.
struct BfPhasor {
    double re, im;
    int restart;
};

__device__ __forceinline__ BfPhasor bf_then(const BfPhasor& x, const BfPhasor& y) {
    if (y.restart) return y;
    return BfPhasor{fma(x.re, y.re, -(x.im * y.im)), fma(x.re, y.im, x.im * y.re), x.restart};
}

// (restart, conj(d_f / |d_f|)) of bin f >= 1
__device__ __forceinline__ BfPhasor bf_phasor(const float2* __restrict__ w, long long f, int C) {
    double dr = 0.0, di = 0.0;
    for (int c = 0; c < C; ++c) {               // w_f conj(w_{f-1})
        const float2 x = w[f * C + c], y = w[(f - 1) * C + c];
        dr = fma((double)x.x, (double)y.x, fma((double)x.y, (double)y.y, dr));
        di = fma((double)x.y, (double)y.x, fma(-(double)x.x, (double)y.y, di));
    }
    if (dr == 0.0 && di == 0.0) return BfPhasor{1.0, 0.0, 1};
    const double h = hypot(dr, di);
    return BfPhasor{dr / h, -di / h, 0};
}

__global__ __launch_bounds__(256) void bf_phase_kernel(const float2* __restrict__ w_all, float2* __restrict__ out_all, long long F, int C) {
    __shared__ double sre[2][256], sim[2][256];
    __shared__ int srs[2][256];
    const int x = threadIdx.x;
    const float2* w = w_all + (long long)blockIdx.x * F * C;
    float2* out = out_all + (long long)blockIdx.x * F * C;
    const long long K = (F + 255) / 256, f0 = x * K, f1 = min(f0 + K, F);
    BfPhasor tot{1.0, 0.0, 0};                  // bin 0 is (0, 1): c_0 = 1
    for (long long f = max(f0, 1LL); f < f1; ++f) tot = bf_then(tot, bf_phasor(w, f, C));
    int cur = 0;
    sre[0][x] = tot.re;
    sim[0][x] = tot.im;
    srs[0][x] = tot.restart;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        BfPhasor me{sre[cur][x], sim[cur][x], srs[cur][x]};
        if (x >= d) me = bf_then(BfPhasor{sre[cur][x - d], sim[cur][x - d], srs[cur][x - d]}, me);
        cur ^= 1;
        sre[cur][x] = me.re;
        sim[cur][x] = me.im;
        srs[cur][x] = me.restart;
        __syncthreads();
    }
    BfPhasor run = x == 0 ? BfPhasor{1.0, 0.0, 0} : BfPhasor{sre[cur][x - 1], sim[cur][x - 1], srs[cur][x - 1]};
    for (long long f = f0; f < f1; ++f) {
        if (f >= 1) run = bf_then(run, bf_phasor(w, f, C));
        for (int c = 0; c < C; ++c) {
            const float2 v = w[f * C + c];
            out[f * C + c] = make_float2((float)fma((double)v.x, run.re, -((double)v.y * run.im)),
                                         (float)fma((double)v.x, run.im, (double)v.y * run.re));
        }
    }
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

int ptmi_bf_eig(const double* psd_target, const double* psd_noise, int64_t B, int64_t F, int32_t C, int32_t mode, int32_t ban, float* w,
                double* lambda, int32_t* sweeps, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!psd_target || !w || !lambda || mode < 0 || mode > 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((mode == 0 || ban) && !psd_noise, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || F < 1 || C < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(C > kBfMaxChannels || B > 2147483647LL || B * F > 2147483647LL * kBfEigLanes, PTMI_E_UNSUPPORTED);
    const long long BF = B * F;
    const size_t lds = (size_t)6 * C * C * kBfEigLanes * sizeof(double);
    hipLaunchKernelGGL(bf_eig_kernel, dim3((unsigned)((BF + kBfEigLanes - 1) / kBfEigLanes)), dim3(kBfEigLanes), lds,
                       static_cast<hipStream_t>(stream), psd_target, psd_noise, reinterpret_cast<float2*>(w), lambda, sweeps, BF, C,
                       mode == 0, ban != 0);
    return launch_status();
}

int ptmi_bf_ban(const float* w, const double* psd_noise, int64_t B, int64_t F, int32_t C, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!w || !psd_noise || !out, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || F < 1 || C < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(C > kBfMaxChannels || B > 2147483647LL || B * F > 2147483647LL * 256, PTMI_E_UNSUPPORTED);
    const long long BF = B * F;
    hipLaunchKernelGGL(bf_ban_kernel, dim3((unsigned)((BF + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float2*>(w), psd_noise, reinterpret_cast<float2*>(out), BF, C);
    return launch_status();
}

int ptmi_bf_phase(const float* w, int64_t B, int64_t F, int32_t C, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!w || !out, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || F < 1 || C < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(C > kBfMaxChannels || B > 2147483647LL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(bf_phase_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float2*>(w), reinterpret_cast<float2*>(out), (long long)F, C);
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
