// The angular-margin softmax head of the d-vector speaker model and the batch norm in front of it (include/ptmi.h: ptmi_aam_*,
// ptmi_batch_norm_rows_*).
//
// Replaces padertorch/contrib/tcl/speaker_embeddings/loss.py:64-103 (AngularPenaltySMLoss.forward: normalise the class weights and
// the embeddings, logits [B, C], target gather, the "all other classes" matrix, exp / sum / log) and the nn.BatchNorm1d(E, affine=False)
// of dvectors.py:69,94.  The logits [B, C] are never written: the forward is a GEMM with a log-sum-exp epilogue, the backward recomputes
// the cosines from the normalised operands and the saved row log-sum-exp, the way attn_dkv_kernel / attn_dq_kernel recompute
// probabilities.  fp32 in and out; every product runs on the matrix cores as v_mfma_f32_16x16x4_f32, bit for bit a k-ordered fmaf
// chain (a scale of 30-64 in front of the cosine rules out one 16-bit product).  Lane maps as in attention.hip: operand
// A[row = l & 15][k = l >> 4], operand B[k = l >> 4][col = l & 15], result C[row = 4 (l >> 4) + r][col = l & 15] in register r, so one row
// of a result tile lies in 16 neighbouring lanes and its maximum / sum is four xor steps (8, 4, 2, 1).
//
//   aam_prepare_kernel   a wave per row of W and of e: ||row|| in fp32 (the lane's elements ascending, then the 64-lane butterfly),
//                        W_hat written IN PLACE, e_hat and 1 / max(||e||, 1e-12) out of place.  A launch of its own: normalising W while
//                        other workgroups read the same rows would race, and normalising a normalised row again is not bit-stable.
//   aam_forward_kernel   a workgroup OWNS kAamBN = 32 classes (W_hat rows staged once in LDS, E zero-padded to a multiple of 16, row stride
//                        + 4 words) and STREAMS the batch in tiles of kAamBM = 64 rows (16 per wave, read from e_hat as A operands).
//                        Per batch row and class tile: the maximum of s cos over the tile's non-target classes, the sum of
//                        exp(s cos - max) over them -> part [tiles][B]; the lane that holds the target class writes cos_y [B].
//   aam_finish_kernel    a wave per batch row: lane j combines tiles j, j + 64, ... ascending (running maximum), the 64 lanes by the
//                        butterfly 32 .. 1; margin, clamp and acos in fp64; -L, the row log-sum-exp, n and dn/dcos_y.
//   aam_mean_kernel      -mean(L): fp64, thread t rows t, t + 256, ... ascending, block_sums.
//   aam_dw_kernel        owns kAamBN classes, streams the batch: dl tile [64][32] through LDS, dW[c, :] = sum_b dl[b, c] e_hat[b, :] in
//                        registers (wave w owns the 16-column blocks w, w + 4, ... of E), every element written once.
//   aam_de_kernel        owns kAamBM rows, streams the class tiles of ITS RANGE of classes through LDS: g = sum_c dl[b, c] W_hat[c, :] ->
//                        workspace [ranges][B][E] (a few row tiles alone would leave the device idle: ptmi_aam_de_splits ranges).
//   aam_de_finish_kernel a wave per row: the ranges ascending, then de = (g - e_hat (e_hat . g)) / ||e||.
// dl[b, c] = s p[b, c] gout_b (c != y), (p_y - 1) (dn/dcos_y) gout_b (c = y), p = exp(s cos - lse).  No atomics; every sum has one order.
//
// Labels are device data (int32 / int64).  A label outside [0, C): that row's loss is NaN, its lse +inf (so its dl is 0 everywhere) and
// nothing is indexed with it.  Departure from the reference: the log-sum-exp carries a running maximum, so where the reference's
// exp(64 cos) leaves fp32 this stays finite.
#include <math.h>

#include "reduce.h"

namespace ptmi {

constexpr int kAamBN = 32;            // classes of a class tile
constexpr int kAamBM = 64;            // batch rows of a batch tile (16 per wave)
constexpr int kAamPLD = kAamBN + 4;   // row stride of a dl image
constexpr int kAamMaxE = 512;
constexpr int kAamMaxSplits = 64;

typedef float aam_f32x4 __attribute__((ext_vector_type(4)));

struct AamArgs {
    const float *w_hat, *e_hat, *e_rnorm, *lse, *n, *dn, *gout;
    const void* labels;
    int labels64, gout_mean;
    long long B, C;
    int E, EP;
    float s;
};

__device__ __forceinline__ long long aam_label(const AamArgs& A, long long b) {
    return A.labels64 ? static_cast<const long long*>(A.labels)[b] : (long long)static_cast<const int*>(A.labels)[b];
}

__device__ __forceinline__ float aam_row_max(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float aam_row_sum(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// S[r][c] = W_hat[c0 + r][c], r < kAamBN, c < EP, zero behind C and behind E; all 256 threads.
__device__ __forceinline__ void aam_stage(float* __restrict__ S, const AamArgs& A, long long c0) {
    const int EP = A.EP, LD = EP + 4;
    for (int idx = threadIdx.x; idx < kAamBN * EP; idx += 256) {
        const int r = idx / EP, c = idx - r * EP;
        const long long row = c0 + r;
        S[r * LD + c] = (row < A.C && c < A.E) ? A.w_hat[row * A.E + c] : 0.f;
    }
}

// acc[nb][r] = sum_k e_hat[row0 + 4 (lane >> 4) + r][k] S[16 nb + (lane & 15)][k], k ascending; rows behind B give 0.
__device__ __forceinline__ void aam_cos(aam_f32x4 (&acc)[2], const AamArgs& A, long long row0, const float* __restrict__ S, int lane) {
    const int LD = A.EP + 4;
    const long long r = row0 + (lane & 15);
    const bool rok = r < A.B;
    const float* __restrict__ er = A.e_hat + (rok ? r : 0) * A.E;
    const float* __restrict__ p0 = S + (lane & 15) * LD + (lane >> 4);
    const float* __restrict__ p1 = p0 + 16 * LD;
    acc[0] = aam_f32x4{0.f, 0.f, 0.f, 0.f};
    acc[1] = aam_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < A.EP; k += 16) {
        float a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = k + 4 * j + (lane >> 4);
            a[j] = (rok && c < A.E) ? er[c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], p0[k + 4 * j], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], p1[k + 4 * j], acc[1], 0, 0, 0);
        }
    }
}

// ------------------------------------------------------------------------------------------------ prepare
__global__ __launch_bounds__(256) void aam_prepare_kernel(float* w, const float* __restrict__ e, float* __restrict__ e_hat,
                                                          float* __restrict__ e_rnorm, long long B, long long C, int E) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= C + B) return;
    const bool is_w = row < C;
    const float* src = is_w ? w + row * E : e + (row - C) * E;          // (a row of W is read and written through both)
    float* dst = is_w ? w + row * E : e_hat + (row - C) * E;
    float ss = 0.f;
    for (int c = lane; c < E; c += 64) ss = fmaf(src[c], src[c], ss);
    const float d = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    for (int c = lane; c < E; c += 64) dst[c] = src[c] / d;
    if (!is_w && lane == 0) e_rnorm[row - C] = 1.f / d;
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void aam_forward_kernel(const AamArgs A, float* __restrict__ part_max, float* __restrict__ part_sum,
                                                          float* __restrict__ cos_y) {
    extern __shared__ __attribute__((aligned(16))) float aam_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long tile = blockIdx.x, c0 = tile * kAamBN;
    aam_stage(aam_lds, A, c0);
    __syncthreads();
    for (long long b0 = 0; b0 < A.B; b0 += kAamBM) {
        const long long row0 = b0 + wave * 16;
        if (row0 >= A.B) break;                             // (no barrier below: a wave may leave alone)
        aam_f32x4 acc[2];
        aam_cos(acc, A, row0, aam_lds, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long i = row0 + (lane >> 4) * 4 + r;
            const long long y = i < A.B ? aam_label(A, i) : -1;
            float v[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const long long c = c0 + nb * 16 + (lane & 15);
                if (c < A.C && c == y) cos_y[i] = acc[nb][r];
                v[nb] = (c < A.C && c != y && i < A.B) ? A.s * acc[nb][r] : -INFINITY;
            }
            const float mx = aam_row_max(fmaxf(v[0], v[1]));
            const float p = (v[0] == -INFINITY ? 0.f : expf(v[0] - mx)) + (v[1] == -INFINITY ? 0.f : expf(v[1] - mx));
            const float sum = aam_row_sum(p);
            if ((lane & 15) == 0 && i < A.B) part_max[tile * A.B + i] = mx, part_sum[tile * A.B + i] = sum;
        }
    }
}

// (m, s) <- (m, s) + (m2, s2): sums of exp(x - m)
__device__ __forceinline__ void aam_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mn));
    m = mn;
}

__global__ __launch_bounds__(256) void aam_finish_kernel(const AamArgs A, const float* __restrict__ part_max, const float* __restrict__ part_sum,
                                                         const float* __restrict__ cos_y, long long tiles, int loss_type, double margin,
                                                         double eps, float* __restrict__ loss_rows, float* __restrict__ lse_out,
                                                         float* __restrict__ n_out, float* __restrict__ dn_out) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= A.B) return;
    float m = -INFINITY, s = 0.f;
    for (long long t = lane; t < tiles; t += 64) aam_merge(m, s, part_max[t * A.B + b], part_sum[t * A.B + b]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        aam_merge(m, s, m2, s2);
    }
    if (lane != 0) return;
    const long long y = aam_label(A, b);
    if (y < 0 || y >= A.C) {                                // no class: NaN loss, and exp(x - lse) = 0 in the backward
        loss_rows[b] = NAN, lse_out[b] = INFINITY, n_out[b] = 0.f, dn_out[b] = 0.f;
        return;
    }
    const double c = (double)cos_y[b], sc = (double)A.s;
    double n, dn;
    if (loss_type == 0) {                                   // aam
        n = sc * (c - margin), dn = sc;
    } else {
        const double lo = -1. + eps, hi = 1. - eps;
        const bool inside = c >= lo && c <= hi;             // the clamp passes no gradient outside its range
        const double cc = c < lo ? lo : (c > hi ? hi : c);
        const double theta = acos(cc), root = sqrt(1. - cc * cc);
        if (loss_type == 1) {                               // arcface
            n = sc * cos(theta + margin), dn = inside ? sc * sin(theta + margin) / root : 0.;
        } else {                                            // sphereface
            n = sc * cos(margin * theta), dn = inside ? sc * margin * sin(margin * theta) / root : 0.;
        }
    }
    const double md = (double)m;
    const double top = (m == -INFINITY || n > md) ? n : md;
    const double tot = exp(n - top) + (m == -INFINITY ? 0. : (double)s * exp(md - top));
    const double lse = top + log(tot);
    loss_rows[b] = (float)(lse - n), lse_out[b] = (float)lse, n_out[b] = (float)n, dn_out[b] = (float)dn;
}

__global__ __launch_bounds__(256) void aam_mean_kernel(const float* __restrict__ loss_rows, long long B, float* __restrict__ out) {
    double s[1] = {0.};
    for (long long b = threadIdx.x; b < B; b += 256) s[0] += (double)loss_rows[b];
    block_sums(s);
    if (threadIdx.x == 0) out[0] = (float)(s[0] / (double)B);
}

// ------------------------------------------------------------------------------------------------ backward
// dl of the result-tile element (row i, class c) whose cosine is cs
__device__ __forceinline__ float aam_dl(const AamArgs& A, long long i, long long c, float cs) {
    if (i >= A.B || c >= A.C) return 0.f;
    const float g = A.gout_mean ? A.gout[0] / (float)A.B : A.gout[i];
    const float lse = A.lse[i];
    if (c == aam_label(A, i)) return (expf(A.n[i] - lse) - 1.f) * A.dn[i] * g;
    return A.s * expf(A.s * cs - lse) * g;
}

template <int NCB>
__global__ __launch_bounds__(256) void aam_dw_kernel(const AamArgs A, float* __restrict__ dw) {
    extern __shared__ __attribute__((aligned(16))) float aam_lds[];
    const int LD = A.EP + 4;
    float* __restrict__ S = aam_lds;
    float* __restrict__ P = aam_lds + kAamBN * LD;          // dl [kAamBM][kAamPLD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c0 = (long long)blockIdx.x * kAamBN;
    aam_stage(S, A, c0);
    aam_f32x4 acc[2][NCB];
#pragma unroll
    for (int j = 0; j < NCB; ++j) acc[0][j] = acc[1][j] = aam_f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long b0 = 0; b0 < A.B; b0 += kAamBM) {
        __syncthreads();                                    // W_hat is staged / the image before has been read
        const long long row0 = b0 + wave * 16;
        aam_f32x4 cs[2];
        aam_cos(cs, A, row0, S, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                P[(wave * 16 + (lane >> 4) * 4 + r) * kAamPLD + nb * 16 + (lane & 15)] =
                    aam_dl(A, row0 + (lane >> 4) * 4 + r, c0 + nb * 16 + (lane & 15), cs[nb][r]);
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kAamBM / 4; ++kk) {
            const int krow = 4 * kk + (lane >> 4);
            const float a0 = P[krow * kAamPLD + (lane & 15)], a1 = P[krow * kAamPLD + 16 + (lane & 15)];
            const long long gi = b0 + krow;
#pragma unroll
            for (int j = 0; j < NCB; ++j) {
                const int col = (wave + 4 * j) * 16 + (lane & 15);
                const float bv = (gi < A.B && col < A.E) ? A.e_hat[gi * A.E + col] : 0.f;
                acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int j = 0; j < NCB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long c = c0 + cb * 16 + (lane >> 4) * 4 + r;
                const int col = (wave + 4 * j) * 16 + (lane & 15);
                if (c < A.C && col < A.E) dw[c * A.E + col] = acc[cb][j][r];
            }
}

template <int NDB>
__global__ __launch_bounds__(256) void aam_de_kernel(const AamArgs A, float* __restrict__ ws, long long tiles, long long tiles_per_split) {
    extern __shared__ __attribute__((aligned(16))) float aam_lds[];
    const int LD = A.EP + 4;
    float* __restrict__ S = aam_lds;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* __restrict__ Pw = aam_lds + kAamBN * LD + wave * 16 * kAamPLD;      // the wave's dl [16][kAamPLD]
    const long long row0 = (long long)blockIdx.x * kAamBM + wave * 16, split = blockIdx.y;
    const long long t0 = split * tiles_per_split, t1 = t0 + tiles_per_split < tiles ? t0 + tiles_per_split : tiles;
    aam_f32x4 acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[db] = aam_f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long t = t0; t < t1; ++t) {
        const long long c0 = t * kAamBN;
        __syncthreads();                                    // the tile before has been read
        aam_stage(S, A, c0);
        __syncthreads();
        aam_f32x4 cs[2];
        aam_cos(cs, A, row0, S, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                Pw[((lane >> 4) * 4 + r) * kAamPLD + nb * 16 + (lane & 15)] =
                    aam_dl(A, row0 + (lane >> 4) * 4 + r, c0 + nb * 16 + (lane & 15), cs[nb][r]);
        __syncthreads();                                    // the image is complete
#pragma unroll 2
        for (int kk = 0; kk < kAamBN / 4; ++kk) {
            const float a = Pw[(lane & 15) * kAamPLD + 4 * kk + (lane >> 4)];
            const float* __restrict__ p = S + (4 * kk + (lane >> 4)) * LD + (lane & 15);
#pragma unroll
            for (int db = 0; db < NDB; ++db)
                if (db * 16 < A.EP) acc[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, p[db * 16], acc[db], 0, 0, 0);
        }
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long i = row0 + (lane >> 4) * 4 + r;
            const int col = db * 16 + (lane & 15);
            if (i < A.B && col < A.E) ws[(split * A.B + i) * A.E + col] = acc[db][r];
        }
}

__global__ __launch_bounds__(256) void aam_de_finish_kernel(const AamArgs A, const float* __restrict__ ws, long long splits,
                                                            float* __restrict__ de) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= A.B) return;
    float g[kAamMaxE / 64], dot = 0.f;
#pragma unroll
    for (int j = 0; j < kAamMaxE / 64; ++j) {
        const int col = lane + 64 * j;
        g[j] = 0.f;
        if (col < A.E) {
            for (long long sp = 0; sp < splits; ++sp) g[j] += ws[(sp * A.B + b) * A.E + col];
            dot = fmaf(A.e_hat[b * A.E + col], g[j], dot);
        }
    }
    dot = wave_sum(dot);
    const float rn = A.e_rnorm[b];
#pragma unroll
    for (int j = 0; j < kAamMaxE / 64; ++j) {
        const int col = lane + 64 * j;
        if (col < A.E) de[b * A.E + col] = (g[j] - A.e_hat[b * A.E + col] * dot) * rn;
    }
}

// ------------------------------------------------------------------------------------------------ batch norm over the rows of [B, E]
// Workgroup: 64 columns; thread (column t & 63, row group t >> 6) adds rows g, g + 4, ... ascending in fp64, the four groups ((0 + 1) + 2) + 3.
__device__ __forceinline__ double bn_colsum(double v, double (&red)[4][64], int cx, int g) {
    __syncthreads();
    red[g][cx] = v;
    __syncthreads();
    return ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

__global__ __launch_bounds__(256) void bn_rows_forward_kernel(const float* __restrict__ x, float* __restrict__ y, double* __restrict__ stats,
                                                              float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ count,
                                                              long long B, int E, int training, double momentum, double eps) {
    __shared__ double red[4][64];
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const bool ok = c < E;
    double mean = 0., rstd = 0.;
    if (training) {
        double s = 0.;
        if (ok)
            for (long long row = g; row < B; row += 4) s += (double)x[row * E + c];
        mean = bn_colsum(s, red, cx, g) / (double)B;
        double q = 0.;
        if (ok)
            for (long long row = g; row < B; row += 4) {
                const double d = (double)x[row * E + c] - mean;
                q += d * d;
            }
        const double var = bn_colsum(q, red, cx, g) / (double)B;
        rstd = 1. / sqrt(var + eps);
        if (ok && g == 0 && rmean && rvar) {
            rmean[c] = (float)((1. - momentum) * (double)rmean[c] + momentum * mean);
            rvar[c] = (float)((1. - momentum) * (double)rvar[c] + momentum * var * (double)B / (double)(B - 1));
        }
        if (count && blockIdx.x == 0 && threadIdx.x == 0) count[0] += 1;
    } else if (ok) {
        mean = (double)rmean[c], rstd = 1. / sqrt((double)rvar[c] + eps);
    }
    if (!ok) return;
    if (g == 0) stats[c] = mean, stats[E + c] = rstd;
    for (long long row = g; row < B; row += 4) y[row * E + c] = (float)(((double)x[row * E + c] - mean) * rstd);
}

__global__ __launch_bounds__(256) void bn_rows_backward_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                               const double* __restrict__ stats, float* __restrict__ dx, long long B, int E,
                                                               int training) {
    __shared__ double red[4][64];
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const bool ok = c < E;
    const double mean = ok ? stats[c] : 0., rstd = ok ? stats[E + c] : 0.;
    double m1 = 0., m2 = 0.;
    if (training) {
        double s1 = 0., s2 = 0.;
        if (ok)
            for (long long row = g; row < B; row += 4) {
                const double gv = (double)gy[row * E + c];
                s1 += gv;
                s2 += gv * (((double)x[row * E + c] - mean) * rstd);
            }
        m1 = bn_colsum(s1, red, cx, g) / (double)B;
        m2 = bn_colsum(s2, red, cx, g) / (double)B;
    }
    if (!ok) return;
    for (long long row = g; row < B; row += 4) {
        const double xh = ((double)x[row * E + c] - mean) * rstd;
        dx[row * E + c] = (float)(rstd * ((double)gy[row * E + c] - m1 - xh * m2));
    }
}

static int aam_ep(int E) { return (E + 15) / 16 * 16; }

static int aam_shape(AamArgs& A, int64_t B, int64_t C, int32_t E, const void* labels, int32_t labels_int64, float s) {
    PTMI_RETURN_IF(B < 1 || C < 2 || E < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(E > kAamMaxE || B > (1LL << 31) || C > (1LL << 31), PTMI_E_UNSUPPORTED);
    A.B = B, A.C = C, A.E = E, A.EP = aam_ep(E), A.labels = labels, A.labels64 = labels_int64, A.s = s;
    return PTMI_OK;
}

// Dynamic LDS above the default limit has to be told to the kernel (an attribute of the function: no synchronisation).
static int aam_allow_lds(const void* fn, size_t bytes) {
    if (bytes > 64 * 1024)
        PTMI_RETURN_IF(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess, PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

static long long aam_tiles(long long C) { return (C + kAamBN - 1) / kAamBN; }

template <int N>
static int aam_launch_dw(const AamArgs& A, float* dw, size_t lds, hipStream_t st) {
    int rc = aam_allow_lds(reinterpret_cast<const void*>(aam_dw_kernel<N>), lds);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    hipLaunchKernelGGL((aam_dw_kernel<N>), dim3((unsigned)aam_tiles(A.C)), dim3(256), lds, st, A, dw);
    return launch_status();
}

template <int N>
static int aam_launch_de(const AamArgs& A, float* ws, long long splits, size_t lds, hipStream_t st) {
    int rc = aam_allow_lds(reinterpret_cast<const void*>(aam_de_kernel<N>), lds);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const long long tiles = aam_tiles(A.C), per = (tiles + splits - 1) / splits;
    hipLaunchKernelGGL((aam_de_kernel<N>), dim3((unsigned)((A.B + kAamBM - 1) / kAamBM), (unsigned)splits), dim3(256), lds, st, A, ws, tiles, per);
    return launch_status();
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_aam_max_features(void) { return kAamMaxE; }

int32_t ptmi_aam_class_tile(void) { return kAamBN; }

int32_t ptmi_aam_row_tile(void) { return kAamBM; }

int64_t ptmi_aam_de_splits(int64_t B, int64_t C) {
    if (B < 1 || C < 1) return 0;
    const long long tiles = aam_tiles(C), row_tiles = (B + kAamBM - 1) / kAamBM;
    long long want = (512 + row_tiles - 1) / row_tiles;     // about two workgroups per compute unit
    if (want > kAamMaxSplits) want = kAamMaxSplits;
    if (want > tiles) want = tiles;
    const long long per = (tiles + want - 1) / want;
    return (tiles + per - 1) / per;                          // no empty range
}

int ptmi_aam_prepare(float* weight, const float* e, float* e_hat, float* e_rnorm, int64_t B, int64_t C, int32_t E, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!weight || !e || !e_hat || !e_rnorm || B < 1 || C < 2 || E < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(E > kAamMaxE || B > (1LL << 31) || C > (1LL << 31), PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(aam_prepare_kernel, dim3((unsigned)((B + C + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), weight, e, e_hat,
                       e_rnorm, (long long)B, (long long)C, E);
    return launch_status();
}

int ptmi_aam_forward(const float* w_hat, const float* e_hat, const void* labels, int32_t labels_int64, int64_t B, int64_t C, int32_t E,
                     int32_t loss_type, float s, double m, double eps, float* part_max, float* part_sum, float* cos_y, float* loss_rows,
                     float* lse, float* n, float* dn, float* loss_mean, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!w_hat || !e_hat || !labels || !part_max || !part_sum || !cos_y || !loss_rows || !lse || !n || !dn, PTMI_E_INVALID);
    PTMI_RETURN_IF(loss_type < 0 || loss_type > 2, PTMI_E_INVALID);
    AamArgs A = {};
    A.w_hat = w_hat, A.e_hat = e_hat;
    int rc = aam_shape(A, B, C, E, labels, labels_int64, s);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)kAamBN * (A.EP + 4) * sizeof(float);
    rc = aam_allow_lds(reinterpret_cast<const void*>(aam_forward_kernel), lds);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const long long tiles = aam_tiles(C);
    hipLaunchKernelGGL(aam_forward_kernel, dim3((unsigned)tiles), dim3(256), lds, st, A, part_max, part_sum, cos_y);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    hipLaunchKernelGGL(aam_finish_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, A, part_max, part_sum, cos_y, tiles, loss_type, m,
                       eps, loss_rows, lse, n, dn);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK || !loss_mean, rc);
    hipLaunchKernelGGL(aam_mean_kernel, dim3(1), dim3(256), 0, st, loss_rows, (long long)B, loss_mean);
    return launch_status();
}

int ptmi_aam_backward(const float* w_hat, const float* e_hat, const float* e_rnorm, const void* labels, int32_t labels_int64, const float* lse,
                      const float* n, const float* dn, const float* gout, int32_t gout_mean, int64_t B, int64_t C, int32_t E, float s,
                      float* dw, float* de, float* workspace, int64_t splits, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!w_hat || !e_hat || !labels || !lse || !n || !dn || !gout || (!dw && !de), PTMI_E_INVALID);
    PTMI_RETURN_IF(de && (!e_rnorm || !workspace || splits != ptmi_aam_de_splits(B, C)), PTMI_E_INVALID);
    AamArgs A = {};
    A.w_hat = w_hat, A.e_hat = e_hat, A.e_rnorm = e_rnorm, A.lse = lse, A.n = n, A.dn = dn, A.gout = gout, A.gout_mean = gout_mean;
    int rc = aam_shape(A, B, C, E, labels, labels_int64, s);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t tile_bytes = (size_t)kAamBN * (A.EP + 4) * sizeof(float), image_bytes = (size_t)kAamBM * kAamPLD * sizeof(float);
    if (dw) {
        const size_t lds = tile_bytes + image_bytes;
        rc = A.EP <= 64 ? aam_launch_dw<1>(A, dw, lds, st)
                        : (A.EP <= 128 ? aam_launch_dw<2>(A, dw, lds, st) : (A.EP <= 256 ? aam_launch_dw<4>(A, dw, lds, st) : aam_launch_dw<8>(A, dw, lds, st)));
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
    }
    if (de) {
        const size_t lds = tile_bytes + image_bytes;
        rc = A.EP <= 64 ? aam_launch_de<4>(A, workspace, splits, lds, st)
                        : (A.EP <= 128 ? aam_launch_de<8>(A, workspace, splits, lds, st)
                                       : (A.EP <= 256 ? aam_launch_de<16>(A, workspace, splits, lds, st) : aam_launch_de<32>(A, workspace, splits, lds, st)));
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
        hipLaunchKernelGGL(aam_de_finish_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, A, workspace, (long long)splits, de);
        rc = launch_status();
    }
    return rc;
}

int ptmi_batch_norm_rows_forward(const float* x, float* y, double* stats, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                 int64_t B, int32_t E, int32_t training, double momentum, double eps, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !y || !stats || B < 1 || E < 1 || (!training && (!running_mean || !running_var)), PTMI_E_INVALID);
    PTMI_RETURN_IF(training && B < 2, PTMI_E_INVALID);
    hipLaunchKernelGGL(bn_rows_forward_kernel, dim3((unsigned)((E + 63) / 64)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, stats,
                       running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), (long long)B, E, training, momentum, eps);
    return launch_status();
}

int ptmi_batch_norm_rows_backward(const float* gy, const float* x, const double* stats, float* dx, int64_t B, int32_t E, int32_t training,
                                  ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gy || !x || !stats || !dx || B < 1 || E < 1, PTMI_E_INVALID);
    hipLaunchKernelGGL(bn_rows_backward_kernel, dim3((unsigned)((E + 63) / 64)), dim3(256), 0, static_cast<hipStream_t>(stream), gy, x, stats, dx,
                       (long long)B, E, training);
    return launch_status();
}

}  // extern "C"
