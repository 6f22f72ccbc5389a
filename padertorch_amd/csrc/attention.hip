// Fused scaled-dot-product attention and the transformer layer's glue (include/ptmi.h: ptmi_attn_*, ptmi_transformer_*).
//
// Replaces padertorch/contrib/je/modules/transformer.py:12-38 (scaled_dot_product_attention: scores, log-masks, softmax, weights @ v),
// :234-243 (add_positional_encoding) and the Normalization + residual pairs of TransformerLayer.forward (:151-174).
//
// Attention.  fp32 in, fp32 out; every product runs on the matrix cores as v_mfma_f32_16x16x4_f32, which is bit for bit a k-ordered
// fmaf chain, so the kernels carry plain fp32 arithmetic.  A workgroup is 4 waves and OWNS kAtBM = 64 rows (16 per wave), held in
// registers as MFMA A operands; the other side STREAMS through LDS in tiles of kAtBN = 32 rows:
//   attn_forward_kernel    owns queries, streams K and V: S = Q K^T, online softmax (running maximum m and sum l per row), O += P V
//   attn_weights_kernel    owns queries, streams K twice: the row sum of exp(s - lse), then the normalised weights
//   attn_dq_kernel         owns queries, streams K and V: dS = P (dO V^T - delta) scale, dQ += dS K
//   attn_dkv_kernel        owns keys, streams Q and dO:  dV += P^T dO, dK += dS^T Q
// so nothing is summed across workgroups and there are no atomics.  Lane maps (16x16x4 f32): operand A[row = l & 15][k = l >> 4],
// operand B[k = l >> 4][col = l & 15], result C[row = 4 (l >> 4) + r][col = l & 15] in register r.  A score tile therefore has one row in
// 16 neighbouring lanes: row maxima and sums are four xor steps (8, 4, 2, 1), one fixed order.  A probability tile becomes the next
// product's A operand through a per-wave LDS image.  The head size is zero-padded to DP = 16, 32, 64 or 128 columns inside LDS and
// the registers; key tiles wholly behind the length or above the causal diagonal are not visited.
//
// Masks, as transformer.py:29-36 combines them (y + log(mask > 0)): element (i, j) is visible iff j < min(Tk, lengths[b]) (lengths
// given), j <= i + Tk - Tq (causal: get_causal_mask, :259-260) and mask[b, h, i, j] != 0 (bytes, any strides).  A row without a visible
// key is NaN in out, lse and the weights (softmax of all -inf), written as such; it contributes nothing to the gradients.
#include <math.h>

#include "reduce.h"

namespace ptmi {

constexpr int kAtBM = 64;          // rows a workgroup owns (16 per wave)
constexpr int kAtBN = 32;          // rows of a streamed tile
constexpr int kAtPLD = kAtBN + 4;  // row stride of a wave's probability image
constexpr int kAtMaxHead = 128;
constexpr int kAtSlabRows = 256;   // rows per slab of the gamma / beta column sums

typedef float at_f32x4 __attribute__((ext_vector_type(4)));

struct AtMask {
    const void* lengths;
    int lengths64, causal;
    const uint8_t* mask;
    long long ms[4];
    long long Tq, Tk;
};

struct AtArgs {
    const float *q, *k, *v, *o, *dout, *lse, *delta;
    float *out, *lse_out, *dq, *dk, *dv, *w;
    long long qs[3], ks[3], vs[3], os[3], gs[3], dqs[3], dks[3], dvs[3];        // (batch, head, time) strides; unit stride on the head column
    int B, H, dh, dvn;
    float scale;
    AtMask M;
};

__device__ __forceinline__ long long at_klen(const AtMask& M, long long b) {
    long long n = M.Tk;
    if (M.lengths) {
        const long long len = M.lengths64 ? static_cast<const long long*>(M.lengths)[b] : (long long)static_cast<const int*>(M.lengths)[b];
        n = len < 0 ? 0 : (len < n ? len : n);
    }
    return n;
}

__device__ __forceinline__ bool at_visible(const AtMask& M, long long klen, long long b, int h, long long i, long long j) {
    if (i >= M.Tq || j >= klen) return false;
    if (M.causal && j > i + M.Tk - M.Tq) return false;
    if (M.mask && !M.mask[b * M.ms[0] + h * M.ms[1] + i * M.ms[2] + j * M.ms[3]]) return false;
    return true;
}

// One past the last key any query of rows [i0, i1) can see / the first query that can see a key >= j0.
__device__ __forceinline__ long long at_key_end(const AtMask& M, long long klen, long long i1) {
    long long e = klen;
    if (M.causal) {
        const long long c = i1 + M.Tk - M.Tq;          // the last query i1 - 1 sees keys j <= i1 - 1 + Tk - Tq
        e = c < e ? c : e;
    }
    return e < 0 ? 0 : e;
}

__device__ __forceinline__ long long at_query_begin(const AtMask& M, long long j0) {
    if (!M.causal) return 0;
    const long long s = j0 - (M.Tk - M.Tq);
    return s < 0 ? 0 : s;
}

// The wave's 16 owned rows as A operands: a[s] = X[row0 + (lane & 15)][4 s + (lane >> 4)], zero outside the rows and the d columns.
template <int NDB>
__device__ __forceinline__ void at_load_rows(float (&a)[NDB * 4], const float* __restrict__ base, long long st, long long row0,
                                             long long nrows, int d, int lane) {
    const long long r = row0 + (lane & 15);
    const int c0 = lane >> 4;
#pragma unroll
    for (int s = 0; s < NDB * 4; ++s) {
        const int c = 4 * s + c0;
        a[s] = (r < nrows && c < d) ? base[r * st + c] : 0.f;
    }
}

// A streamed tile into LDS: S[r][c] = X[row0 + r][c], r < kAtBN, c < DP, zero outside; all 256 threads.
template <int NDB>
__device__ __forceinline__ void at_stage(float* __restrict__ S, const float* __restrict__ base, long long st, long long row0, long long nrows,
                                         int d) {
    constexpr int DP = NDB * 16, LD = DP + 4;
    for (int idx = threadIdx.x; idx < kAtBN * DP; idx += 256) {
        const int r = idx / DP, c = idx % DP;
        const long long row = row0 + r;
        S[r * LD + c] = (row < nrows && c < d) ? base[row * st + c] : 0.f;
    }
}

// acc[r] = sum_k X[owned row 4 (lane >> 4) + r][k] S[16 nb + (lane & 15)][k]
template <int NDB>
__device__ __forceinline__ at_f32x4 at_dot(const float (&a)[NDB * 4], const float* __restrict__ S, int nb, int lane) {
    constexpr int LD = NDB * 16 + 4;
    at_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ p = S + (nb * 16 + (lane & 15)) * LD + (lane >> 4);
#pragma unroll
    for (int s = 0; s < NDB * 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], p[4 * s], acc, 0, 0, 0);
    return acc;
}

// acc[db][r] += sum_n P[row 4 (lane >> 4) + r][n] S[n][16 db + (lane & 15)] with P the wave's [16][kAtPLD] image
template <int NDB>
__device__ __forceinline__ void at_acc(at_f32x4 (&acc)[NDB], const float* __restrict__ P, const float* __restrict__ S, int lane) {
    constexpr int LD = NDB * 16 + 4;
#pragma unroll
    for (int kk = 0; kk < kAtBN / 4; ++kk) {
        const float a = P[(lane & 15) * kAtPLD + 4 * kk + (lane >> 4)];
        const float* __restrict__ p = S + (4 * kk + (lane >> 4)) * LD + (lane & 15);
#pragma unroll
        for (int db = 0; db < NDB; ++db) acc[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, p[db * 16], acc[db], 0, 0, 0);
    }
}

// Over the 16 lanes that hold one row of a result tile: xor 8, 4, 2, 1.
__device__ __forceinline__ float at_row_max(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float at_row_sum(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------ forward
template <int NDB>
__global__ __launch_bounds__(256) void attn_forward_kernel(const AtArgs A) {
    constexpr int LD = NDB * 16 + 4;
    __shared__ float Ks[kAtBN * LD], Vs[kAtBN * LD], Ps[4][16 * kAtPLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y;
    const long long b = blockIdx.z, tile0 = (long long)blockIdx.x * kAtBM, q0 = tile0 + wave * 16;
    const long long Tq = A.M.Tq, Tk = A.M.Tk;
    const long long klen = at_klen(A.M, b);
    const long long kend = at_key_end(A.M, klen, tile0 + kAtBM < Tq ? tile0 + kAtBM : Tq);
    const long long ntiles = (kend + kAtBN - 1) / kAtBN;
    const float* __restrict__ kb = A.k + b * A.ks[0] + h * A.ks[1];
    const float* __restrict__ vb = A.v + b * A.vs[0] + h * A.vs[1];
    float a[NDB * 4];
    at_load_rows<NDB>(a, A.q + b * A.qs[0] + h * A.qs[1], A.qs[2], q0, Tq, A.dh, lane);
    at_f32x4 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) o[db] = at_f32x4{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = -INFINITY, l[r] = 0.f;
    float* __restrict__ Pw = Ps[wave];
    for (long long t = 0; t < ntiles; ++t) {
        __syncthreads();                                    // the tile before has been read
        at_stage<NDB>(Ks, kb, A.ks[2], t * kAtBN, Tk, A.dh);
        at_stage<NDB>(Vs, vb, A.vs[2], t * kAtBN, Tk, A.dvn);
        __syncthreads();
        at_f32x4 s[2];
        s[0] = at_dot<NDB>(a, Ks, 0, lane);
        s[1] = at_dot<NDB>(a, Ks, 1, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long i = q0 + (lane >> 4) * 4 + r;
            float sv[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const long long j = t * kAtBN + nb * 16 + (lane & 15);
                sv[nb] = at_visible(A.M, klen, b, h, i, j) ? s[nb][r] * A.scale : -INFINITY;
            }
            const float mnew = fmaxf(m[r], at_row_max(fmaxf(sv[0], sv[1])));
            float alpha = 1.f, p0 = 0.f, p1 = 0.f;
            if (mnew != -INFINITY) {                        // (a row that has seen no key yet keeps m = -inf, l = 0: no inf - inf)
                alpha = expf(m[r] - mnew);
                p0 = sv[0] == -INFINITY ? 0.f : expf(sv[0] - mnew);
                p1 = sv[1] == -INFINITY ? 0.f : expf(sv[1] - mnew);
            }
            l[r] = l[r] * alpha + at_row_sum(p0 + p1);
            m[r] = mnew;
#pragma unroll
            for (int db = 0; db < NDB; ++db) o[db][r] *= alpha;
            Pw[((lane >> 4) * 4 + r) * kAtPLD + (lane & 15)] = p0;
            Pw[((lane >> 4) * 4 + r) * kAtPLD + 16 + (lane & 15)] = p1;
        }
        __syncthreads();                                    // the probability image is complete
        at_acc<NDB>(o, Pw, Vs, lane);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = q0 + (lane >> 4) * 4 + r;
        if (i >= Tq) continue;
        const bool dead = !(l[r] > 0.f);                    // no visible key: softmax of all -inf, NaN as in the reference
        float* __restrict__ orow = A.out + b * A.os[0] + h * A.os[1] + i * A.os[2];
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const int c = db * 16 + (lane & 15);
            if (c < A.dvn) orow[c] = dead ? NAN : o[db][r] / l[r];
        }
        if ((lane & 15) == 0) A.lse_out[((long long)b * A.H + h) * Tq + i] = dead ? NAN : m[r] + logf(l[r]);
    }
}

// ------------------------------------------------------------------------------------------------ weights
template <int NDB>
__global__ __launch_bounds__(256) void attn_weights_kernel(const AtArgs A) {
    constexpr int LD = NDB * 16 + 4;
    __shared__ float Ks[kAtBN * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y;
    const long long b = blockIdx.z, tile0 = (long long)blockIdx.x * kAtBM, q0 = tile0 + wave * 16;
    const long long Tq = A.M.Tq, Tk = A.M.Tk;
    const long long klen = at_klen(A.M, b);
    const long long kend = at_key_end(A.M, klen, tile0 + kAtBM < Tq ? tile0 + kAtBM : Tq);
    const long long ntiles = (kend + kAtBN - 1) / kAtBN, alltiles = (Tk + kAtBN - 1) / kAtBN;
    const float* __restrict__ kb = A.k + b * A.ks[0] + h * A.ks[1];
    float a[NDB * 4];
    at_load_rows<NDB>(a, A.q + b * A.qs[0] + h * A.qs[1], A.qs[2], q0, Tq, A.dh, lane);
    float lse[4], z[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = q0 + (lane >> 4) * 4 + r;
        lse[r] = i < Tq ? A.lse[((long long)b * A.H + h) * Tq + i] : 0.f;
        z[r] = 0.f;
    }
    // pass 0: z = sum_j exp(s - lse) (1 up to the rounding of lse); pass 1: the weights exp(s - lse) / z, zeros in the tiles not visited
    for (int pass = 0; pass < 2; ++pass) {
        const long long tiles = pass ? alltiles : ntiles;
        for (long long t = 0; t < tiles; ++t) {
            at_f32x4 s[2] = {at_f32x4{0.f, 0.f, 0.f, 0.f}, at_f32x4{0.f, 0.f, 0.f, 0.f}};
            if (t < ntiles) {
                __syncthreads();
                at_stage<NDB>(Ks, kb, A.ks[2], t * kAtBN, Tk, A.dh);
                __syncthreads();
                s[0] = at_dot<NDB>(a, Ks, 0, lane);
                s[1] = at_dot<NDB>(a, Ks, 1, lane);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long i = q0 + (lane >> 4) * 4 + r;
                float p[2];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const long long j = t * kAtBN + nb * 16 + (lane & 15);
                    p[nb] = (t < ntiles && at_visible(A.M, klen, b, h, i, j)) ? expf(s[nb][r] * A.scale - lse[r]) : 0.f;
                }
                if (pass == 0) {
                    z[r] += at_row_sum(p[0] + p[1]);
                } else if (i < Tq) {
                    float* __restrict__ wrow = A.w + (((long long)b * A.H + h) * Tq + i) * Tk;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const long long j = t * kAtBN + nb * 16 + (lane & 15);
                        if (j < Tk) wrow[j] = isnan(lse[r]) ? NAN : p[nb] / z[r];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// delta[b, h, i] = sum_c dout[b, h, i, c] out[b, h, i, c], ascending c; one thread per row.
__global__ __launch_bounds__(256) void attn_delta_kernel(const AtArgs A, float* __restrict__ delta) {
    const long long Tq = A.M.Tq;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)A.B * A.H * Tq) return;
    const long long i = idx % Tq, bh = idx / Tq;
    const long long b = bh / A.H;
    const int h = (int)(bh % A.H);
    const float* __restrict__ orow = A.o + b * A.os[0] + h * A.os[1] + i * A.os[2];
    const float* __restrict__ grow = A.dout + b * A.gs[0] + h * A.gs[1] + i * A.gs[2];
    float s = 0.f;
    for (int c = 0; c < A.dvn; ++c) s = fmaf(grow[c], orow[c], s);
    delta[idx] = s;
}

template <int NDB>
__global__ __launch_bounds__(256) void attn_dq_kernel(const AtArgs A) {
    constexpr int LD = NDB * 16 + 4;
    __shared__ float Ks[kAtBN * LD], Vs[kAtBN * LD], Ps[4][16 * kAtPLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y;
    const long long b = blockIdx.z, tile0 = (long long)blockIdx.x * kAtBM, q0 = tile0 + wave * 16;
    const long long Tq = A.M.Tq, Tk = A.M.Tk;
    const long long klen = at_klen(A.M, b);
    const long long kend = at_key_end(A.M, klen, tile0 + kAtBM < Tq ? tile0 + kAtBM : Tq);
    const long long ntiles = (kend + kAtBN - 1) / kAtBN;
    const float* __restrict__ kb = A.k + b * A.ks[0] + h * A.ks[1];
    const float* __restrict__ vb = A.v + b * A.vs[0] + h * A.vs[1];
    float qa[NDB * 4], ga[NDB * 4];
    at_load_rows<NDB>(qa, A.q + b * A.qs[0] + h * A.qs[1], A.qs[2], q0, Tq, A.dh, lane);
    at_load_rows<NDB>(ga, A.dout + b * A.gs[0] + h * A.gs[1], A.gs[2], q0, Tq, A.dvn, lane);
    float lse[4], delta[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = q0 + (lane >> 4) * 4 + r;
        const long long row = ((long long)b * A.H + h) * Tq + i;
        lse[r] = i < Tq ? A.lse[row] : 0.f;
        delta[r] = i < Tq ? A.delta[row] : 0.f;
    }
    at_f32x4 dq[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) dq[db] = at_f32x4{0.f, 0.f, 0.f, 0.f};
    float* __restrict__ Pw = Ps[wave];
    for (long long t = 0; t < ntiles; ++t) {
        __syncthreads();
        at_stage<NDB>(Ks, kb, A.ks[2], t * kAtBN, Tk, A.dh);
        at_stage<NDB>(Vs, vb, A.vs[2], t * kAtBN, Tk, A.dvn);
        __syncthreads();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const at_f32x4 s = at_dot<NDB>(qa, Ks, nb, lane);
            const at_f32x4 dp = at_dot<NDB>(ga, Vs, nb, lane);
            const long long j = t * kAtBN + nb * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long i = q0 + (lane >> 4) * 4 + r;
                float ds = 0.f;
                if (at_visible(A.M, klen, b, h, i, j) && !isnan(lse[r])) ds = expf(s[r] * A.scale - lse[r]) * (dp[r] - delta[r]) * A.scale;
                Pw[((lane >> 4) * 4 + r) * kAtPLD + nb * 16 + (lane & 15)] = ds;
            }
        }
        __syncthreads();
        at_acc<NDB>(dq, Pw, Ks, lane);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = q0 + (lane >> 4) * 4 + r;
        if (i >= Tq) continue;
        float* __restrict__ row = A.dq + b * A.dqs[0] + h * A.dqs[1] + i * A.dqs[2];
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const int c = db * 16 + (lane & 15);
            if (c < A.dh) row[c] = dq[db][r];
        }
    }
}

template <int NDB>
__global__ __launch_bounds__(256) void attn_dkv_kernel(const AtArgs A) {
    constexpr int LD = NDB * 16 + 4;
    __shared__ float Qs[kAtBN * LD], Gs[kAtBN * LD], Ps[4][2][16 * kAtPLD], lse_s[kAtBN], delta_s[kAtBN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y;
    const long long b = blockIdx.z, tile0 = (long long)blockIdx.x * kAtBM, k0 = tile0 + wave * 16;
    const long long Tq = A.M.Tq, Tk = A.M.Tk;
    const long long klen = at_klen(A.M, b);
    const float* __restrict__ qb = A.q + b * A.qs[0] + h * A.qs[1];
    const float* __restrict__ gb = A.dout + b * A.gs[0] + h * A.gs[1];
    float ka[NDB * 4], va[NDB * 4];
    at_load_rows<NDB>(ka, A.k + b * A.ks[0] + h * A.ks[1], A.ks[2], k0, Tk, A.dh, lane);
    at_load_rows<NDB>(va, A.v + b * A.vs[0] + h * A.vs[1], A.vs[2], k0, Tk, A.dvn, lane);
    at_f32x4 dk[NDB], dv[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) dk[db] = dv[db] = at_f32x4{0.f, 0.f, 0.f, 0.f};
    float* __restrict__ Pp = Ps[wave][0];
    float* __restrict__ Pd = Ps[wave][1];
    // keys behind the length take no gradient: the workgroup visits no query tile then
    const long long first = tile0 < klen ? at_query_begin(A.M, tile0) / kAtBN : (Tq + kAtBN - 1) / kAtBN;
    for (long long t = first; t * kAtBN < Tq; ++t) {
        __syncthreads();
        at_stage<NDB>(Qs, qb, A.qs[2], t * kAtBN, Tq, A.dh);
        at_stage<NDB>(Gs, gb, A.gs[2], t * kAtBN, Tq, A.dvn);
        if (threadIdx.x < kAtBN) {
            const long long i = t * kAtBN + threadIdx.x;
            const long long row = ((long long)b * A.H + h) * Tq + i;
            lse_s[threadIdx.x] = i < Tq ? A.lse[row] : 0.f;
            delta_s[threadIdx.x] = i < Tq ? A.delta[row] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const at_f32x4 s = at_dot<NDB>(ka, Qs, nb, lane);          // S^T: [key][query]
            const at_f32x4 dp = at_dot<NDB>(va, Gs, nb, lane);         // (dO V^T)^T
            const int qi = nb * 16 + (lane & 15);
            const long long i = t * kAtBN + qi;
            const float lse = lse_s[qi], delta = delta_s[qi];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long j = k0 + (lane >> 4) * 4 + r;
                float p = 0.f, ds = 0.f;
                if (at_visible(A.M, klen, b, h, i, j) && !isnan(lse)) {          // (a row without a visible key has lse = delta = NaN)
                    p = expf(s[r] * A.scale - lse);
                    ds = p * (dp[r] - delta) * A.scale;
                }
                Pp[((lane >> 4) * 4 + r) * kAtPLD + qi] = p;
                Pd[((lane >> 4) * 4 + r) * kAtPLD + qi] = ds;
            }
        }
        __syncthreads();
        at_acc<NDB>(dv, Pp, Gs, lane);
        at_acc<NDB>(dk, Pd, Qs, lane);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long j = k0 + (lane >> 4) * 4 + r;
        if (j >= Tk) continue;
        float* __restrict__ krow = A.dk + b * A.dks[0] + h * A.dks[1] + j * A.dks[2];
        float* __restrict__ vrow = A.dv + b * A.dvs[0] + h * A.dvs[1] + j * A.dvs[2];
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
            const int c = db * 16 + (lane & 15);
            if (c < A.dh) krow[c] = dk[db][r];
            if (c < A.dvn) vrow[c] = dv[db][r];
        }
    }
}

// ------------------------------------------------------------------------------------------------ glue
// out[b, t, 2 i] = x + cos(t / 10000^(2 i / d)), out[b, t, 2 i + 1] = x + sin(same); thread (t, i) walks the batch.  The angle is taken
// as the reference's fp32 tensors take it: freq[i] = 10000^(2 i / d) is the caller's float32 table (the reference evaluates it with torch's
// float32 pow, which the caller repeats on the host once per d), then one correctly rounded fp32 division and the accurate cosf / sinf.
// (out may be x: no __restrict__)
__global__ __launch_bounds__(256) void transformer_posenc_kernel(const float* x, float* out, const float* __restrict__ freq, long long B,
                                                                 long long T, int d) {
#pragma clang fp contract(off)
    const int half = d / 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * half) return;
    const long long t = idx / half;
    const int i = (int)(idx % half);
    const float angle = __fdiv_rn((float)t, freq[i]);
    const float c = cosf(angle), s = sinf(angle);
    for (long long b = 0; b < B; ++b) {
        const long long at = (b * T + t) * d + 2 * i;
        const float x0 = x[at], x1 = x[at + 1];
        out[at] = x0 + c;
        out[at + 1] = x1 + s;
    }
}

__device__ __forceinline__ bool tf_valid(const void* lengths, int lengths64, long long row, long long T) {
    if (!lengths) return true;
    const long long b = row / T, t = row % T;
    const long long len = lengths64 ? static_cast<const long long*>(lengths)[b] : (long long)static_cast<const int*>(lengths)[b];
    return t < len;
}

// One wave per row (b, t).  norm_first: y = LN(z) + res; else u = z + res, y = LN(u).  LN(v) = gamma (v - mean) rstd + beta over the N
// channels for t < lengths[b], zeros behind; stats = (mean, rstd), (0, 0) behind the length.
__global__ __launch_bounds__(256) void transformer_norm_residual_forward_kernel(const float* __restrict__ z, const float* __restrict__ res,
                                                                                const float* __restrict__ gamma,
                                                                                const float* __restrict__ beta, const void* lengths,
                                                                                int lengths64, float* __restrict__ y, float* __restrict__ u,
                                                                                float* __restrict__ stats, long long rows, long long T, int N,
                                                                                float eps, int norm_first) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* __restrict__ zr = z + row * N;
    const float* __restrict__ rr = res + row * N;
    const bool valid = tf_valid(lengths, lengths64, row, T);
    float mean = 0.f, rstd = 0.f;
    if (valid) {
        double s1 = 0.;
        for (int n = lane; n < N; n += 64) s1 += (double)(norm_first ? zr[n] : zr[n] + rr[n]);
        const double m = wave_sum(s1) / (double)N;
        double s2 = 0.;
        for (int n = lane; n < N; n += 64) {
            const double dlt = (double)(norm_first ? zr[n] : zr[n] + rr[n]) - m;
            s2 += dlt * dlt;
        }
        const double var = wave_sum(s2) / (double)N;
        mean = (float)m, rstd = (float)(1. / sqrt(var + (double)eps));
    }
    if (lane == 0) stats[2 * row] = mean, stats[2 * row + 1] = rstd;
    for (int n = lane; n < N; n += 64) {
        const float in = norm_first ? zr[n] : zr[n] + rr[n];
        const float v = valid ? fmaf(gamma[n], (in - mean) * rstd, beta[n]) : 0.f;
        y[row * N + n] = norm_first ? v + rr[n] : v;
        if (!norm_first) u[row * N + n] = in;
    }
}

// dv = rstd (gy gamma - mean_n(gy gamma) - xhat mean_n(gy gamma xhat)) on valid rows, 0 behind the length; v the normalised tensor.
__global__ __launch_bounds__(256) void transformer_norm_residual_backward_kernel(const float* __restrict__ gy, const float* __restrict__ v,
                                                                                 const float* __restrict__ stats,
                                                                                 const float* __restrict__ gamma, const void* lengths,
                                                                                 int lengths64, float* __restrict__ dv, long long rows,
                                                                                 long long T, int N) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* __restrict__ vr = v + row * N;
    const float* __restrict__ gr = gy + row * N;
    const bool valid = tf_valid(lengths, lengths64, row, T);
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float c1 = 0.f, c2 = 0.f;
    if (valid) {
        double s1 = 0., s2 = 0.;
        for (int n = lane; n < N; n += 64) {
            const float g = gr[n] * gamma[n];
            const float xh = (vr[n] - mean) * rstd;
            s1 += (double)g;
            s2 += (double)g * (double)xh;
        }
        c1 = (float)(wave_sum(s1) / (double)N), c2 = (float)(wave_sum(s2) / (double)N);
    }
    for (int n = lane; n < N; n += 64) {
        float o = 0.f;
        if (valid) {
            const float xh = (vr[n] - mean) * rstd;
            o = rstd * fmaf(-xh, c2, gr[n] * gamma[n] - c1);
        }
        dv[row * N + n] = o;
    }
}

// ws[slab][c] = sum over the slab's valid rows of gy xhat, ws[slab][N + c] = ... of gy; workgroup (column block of 64, slab), thread
// (column, row group of 4), rows ascending, the four groups combined ((0 + 1) + 2) + 3.
__global__ __launch_bounds__(256) void transformer_norm_colsum_kernel(const float* __restrict__ gy, const float* __restrict__ v,
                                                                      const float* __restrict__ stats, const void* lengths, int lengths64,
                                                                      double* __restrict__ ws, long long rows, long long T, int N) {
    __shared__ double red[4][64][2];
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const long long r0 = (long long)blockIdx.y * kAtSlabRows, r1 = min(r0 + (long long)kAtSlabRows, rows);
    double s1 = 0., s2 = 0.;
    if (c < N)
        for (long long row = r0 + g; row < r1; row += 4)
            if (tf_valid(lengths, lengths64, row, T)) {
                const float gv = gy[row * N + c];
                const float xh = (v[row * N + c] - stats[2 * row]) * stats[2 * row + 1];
                s1 += (double)gv * (double)xh;
                s2 += (double)gv;
            }
    red[g][cx][0] = s1, red[g][cx][1] = s2;
    __syncthreads();
    if (g == 0 && c < N) {
        ws[blockIdx.y * 2LL * N + c] = ((red[0][cx][0] + red[1][cx][0]) + red[2][cx][0]) + red[3][cx][0];
        ws[blockIdx.y * 2LL * N + N + c] = ((red[0][cx][1] + red[1][cx][1]) + red[2][cx][1]) + red[3][cx][1];
    }
}

static void at_strides(long long (&dst)[3], const int64_t* src) { dst[0] = src[0], dst[1] = src[1], dst[2] = src[2]; }

static int at_mask(AtMask& M, int64_t Tq, int64_t Tk, const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask,
                   const int64_t* mask_strides) {
    PTMI_RETURN_IF(mask && !mask_strides, PTMI_E_INVALID);
    M.lengths = lengths, M.lengths64 = lengths_int64, M.causal = causal, M.mask = mask, M.Tq = Tq, M.Tk = Tk;
    for (int i = 0; i < 4; ++i) M.ms[i] = mask ? mask_strides[i] : 0;
    return PTMI_OK;
}

static int at_ndb(int d) { return d <= 16 ? 1 : (d <= 32 ? 2 : (d <= 64 ? 4 : 8)); }

#define PTMI_AT_LAUNCH(kernel, ndb, grid, st, ...)                                          \
    do {                                                                                    \
        switch (ndb) {                                                                      \
            case 1: hipLaunchKernelGGL((kernel<1>), grid, dim3(256), 0, st, __VA_ARGS__); break; \
            case 2: hipLaunchKernelGGL((kernel<2>), grid, dim3(256), 0, st, __VA_ARGS__); break; \
            case 4: hipLaunchKernelGGL((kernel<4>), grid, dim3(256), 0, st, __VA_ARGS__); break; \
            default: hipLaunchKernelGGL((kernel<8>), grid, dim3(256), 0, st, __VA_ARGS__); break; \
        }                                                                                   \
    } while (0)

static int at_shape(int32_t B, int32_t H, int64_t Tq, int64_t Tk, int32_t dh, int32_t dv) {
    PTMI_RETURN_IF(B < 1 || H < 1 || Tq < 1 || Tk < 1 || dh < 1 || dv < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(dh > kAtMaxHead || dv > kAtMaxHead || B > 65535 || H > 65535 || Tq > (1LL << 36) || Tk > (1LL << 36), PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_attn_tile(void) { return kAtBM; }

int32_t ptmi_attn_key_tile(void) { return kAtBN; }

int32_t ptmi_attn_max_head(void) { return kAtMaxHead; }

int ptmi_attn_forward(const float* q, const float* k, const float* v, const int64_t* strides, int32_t B, int32_t H, int64_t Tq, int64_t Tk,
                      int32_t dh, int32_t dv, float scale, const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask,
                      const int64_t* mask_strides, float* out, float* lse, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!q || !k || !v || !strides || !out || !lse, PTMI_E_INVALID);
    int rc = at_shape(B, H, Tq, Tk, dh, dv);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    AtArgs A = {};
    A.q = q, A.k = k, A.v = v, A.out = out, A.lse_out = lse, A.B = B, A.H = H, A.dh = dh, A.dvn = dv, A.scale = scale;
    at_strides(A.qs, strides), at_strides(A.ks, strides + 3), at_strides(A.vs, strides + 6), at_strides(A.os, strides + 9);
    rc = at_mask(A.M, Tq, Tk, lengths, lengths_int64, causal, mask, mask_strides);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const dim3 grid((unsigned)((Tq + kAtBM - 1) / kAtBM), (unsigned)H, (unsigned)B);
    PTMI_AT_LAUNCH(attn_forward_kernel, at_ndb(dh > dv ? dh : dv), grid, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int ptmi_attn_weights(const float* q, const float* k, const float* lse, const int64_t* strides, int32_t B, int32_t H, int64_t Tq, int64_t Tk,
                      int32_t dh, float scale, const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask,
                      const int64_t* mask_strides, float* weights, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!q || !k || !lse || !strides || !weights, PTMI_E_INVALID);
    int rc = at_shape(B, H, Tq, Tk, dh, 1);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    AtArgs A = {};
    A.q = q, A.k = k, A.lse = lse, A.w = weights, A.B = B, A.H = H, A.dh = dh, A.dvn = 1, A.scale = scale;
    at_strides(A.qs, strides), at_strides(A.ks, strides + 3);
    rc = at_mask(A.M, Tq, Tk, lengths, lengths_int64, causal, mask, mask_strides);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const dim3 grid((unsigned)((Tq + kAtBM - 1) / kAtBM), (unsigned)H, (unsigned)B);
    PTMI_AT_LAUNCH(attn_weights_kernel, at_ndb(dh), grid, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int ptmi_attn_backward(const float* q, const float* k, const float* v, const float* out, const float* dout, const float* lse,
                       const int64_t* strides, int32_t B, int32_t H, int64_t Tq, int64_t Tk, int32_t dh, int32_t dv, float scale,
                       const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask, const int64_t* mask_strides,
                       float* delta, float* dq, float* dk, float* dv_out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!q || !k || !v || !out || !dout || !lse || !strides || !delta || !dq || !dk || !dv_out, PTMI_E_INVALID);
    int rc = at_shape(B, H, Tq, Tk, dh, dv);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    AtArgs A = {};
    A.q = q, A.k = k, A.v = v, A.o = out, A.dout = dout, A.lse = lse, A.delta = delta, A.dq = dq, A.dk = dk, A.dv = dv_out;
    A.B = B, A.H = H, A.dh = dh, A.dvn = dv, A.scale = scale;
    at_strides(A.qs, strides), at_strides(A.ks, strides + 3), at_strides(A.vs, strides + 6), at_strides(A.os, strides + 9);
    at_strides(A.gs, strides + 12), at_strides(A.dqs, strides + 15), at_strides(A.dks, strides + 18), at_strides(A.dvs, strides + 21);
    rc = at_mask(A.M, Tq, Tk, lengths, lengths_int64, causal, mask, mask_strides);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long nrows = (long long)B * H * Tq;
    hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, A, delta);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const int ndb = at_ndb(dh > dv ? dh : dv);
    PTMI_AT_LAUNCH(attn_dkv_kernel, ndb, dim3((unsigned)((Tk + kAtBM - 1) / kAtBM), (unsigned)H, (unsigned)B), st, A);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    PTMI_AT_LAUNCH(attn_dq_kernel, ndb, dim3((unsigned)((Tq + kAtBM - 1) / kAtBM), (unsigned)H, (unsigned)B), st, A);
    return launch_status();
}

int ptmi_transformer_posenc(const float* x, float* out, const float* freq, int64_t B, int64_t T, int32_t d, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !out || !freq || B < 1 || T < 1 || d < 2 || (d & 1), PTMI_E_INVALID);
    const long long n = (long long)T * (d / 2);
    hipLaunchKernelGGL(transformer_posenc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out,
                       freq, (long long)B, (long long)T, d);
    return launch_status();
}

int64_t ptmi_transformer_norm_workspace_elems(int64_t rows, int32_t N) {
    return (rows + kAtSlabRows - 1) / kAtSlabRows * 2 * (int64_t)N;
}

int ptmi_transformer_norm_residual_forward(const float* z, const float* res, const float* gamma, const float* beta, const void* lengths,
                                           int32_t lengths_int64, int64_t B, int64_t T, int32_t N, float eps, int32_t norm_first, float* y,
                                           float* u, float* stats, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!z || !res || !gamma || !beta || !y || !stats || (!norm_first && !u) || B < 1 || T < 1 || N < 1, PTMI_E_INVALID);
    const long long rows = (long long)B * T;
    hipLaunchKernelGGL(transformer_norm_residual_forward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), z, res, gamma, beta, lengths, lengths_int64, y, u, stats, rows, (long long)T, N, eps,
                       norm_first);
    return launch_status();
}

int ptmi_transformer_norm_residual_backward(const float* gy, const float* v, const float* stats, const float* gamma, const void* lengths,
                                            int32_t lengths_int64, int64_t B, int64_t T, int32_t N, float* dv, float* dparams,
                                            double* workspace, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gy || !v || !stats || !gamma || !dv || (dparams && !workspace) || B < 1 || T < 1 || N < 1, PTMI_E_INVALID);
    const long long rows = (long long)B * T;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(transformer_norm_residual_backward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, gy, v, stats, gamma,
                       lengths, lengths_int64, dv, rows, (long long)T, N);
    int rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK || !dparams, rc);
    const long long slabs = (rows + kAtSlabRows - 1) / kAtSlabRows;
    hipLaunchKernelGGL(transformer_norm_colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)slabs), dim3(256), 0, st, gy, v, stats, lengths,
                       lengths_int64, workspace, rows, (long long)T, N);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    return colreduce(workspace, slabs, 2LL * N, StorePlain{dparams}, st);
}

}  // extern "C"
