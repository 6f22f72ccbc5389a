// The contrast of contrastive predictive coding and its cross-entropy (include/ptmi.h: ptmi_cpc_*).
//
// Replaces padertorch/contrib/mk/modules/contrastive.py:343-471 (CPC1d.contrast: per prediction step a dense logit tensor [b, K, T_s], log
// masks added on top) and the CrossEntropyLoss / argmax / "> -inf" count of review (:515-540).  Nothing of size K is written: per query
// the kernels keep the log-sum-exp, the target's score, whether the target is the first maximal key and the number of visible keys; the
// backward recomputes the scores from the saved log-sum-exp.  Operands stay in the model's layout, z [b, d, t] and z_hat [b, S d, t] with
// time contiguous (strides of the other two axes are arguments); slice s of z_hat is the query of step s.  fp32; every product of the
// 'time' / 'all' kernels runs on the matrix cores as v_mfma_f32_16x16x4_f32, bit for bit a k-ordered fmaf chain.  Lane maps as in
// attention.hip: A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15], C[row = 4 (l >> 4) + r][col = l & 15] in register r.
//
// Geometry of step s (T_s = t - |s|): query q reads z_hat_s[.., q + max(-s, 0)]; key index k in [0, t) reads z[.., (k + max(s, 0)) mod t]
// (the reference's torch.roll: wrapped keys are keys); the target of query q is key q of the same batch entry; a key of the query's own
// entry with 0 < |k - q| <= dist - 1 is -inf (dist > 1).  'time': the t keys of the query's entry; 'all': the b t keys i' t + k.
//
//   cpc_forward_kernel        a workgroup of 4 waves OWNS kCpcBM = 64 queries of one (step, entry): the tile sits in LDS for the whole
//                             kernel as R[feature][64] (column rotated by 16 (feature & 3): the four k rows of an A operand fall into four
//                             bank groups).  Key tiles of kCpcBN = 32 indices STREAM through LDS in chunks of 128 features as
//                             X[feature][32 + 4]: the global loads run along time, the transpose is the LDS read.  Every lane keeps the
//                             running maximum / sum / first maximum / count of ITS two columns and four rows; the 16 lanes of a row are
//                             merged once at the end by the four xor steps.  With a logits pointer the tile epilogue also stores the
//                             masked scaled scores [b, K, T_s].  'time' and 'all' differ in the range of key entries visited.
//   cpc_backward_kernel<.., 0>  owns 64 queries like the forward; per key tile the scores again, dscore = g (exp(score - lse) - [target])
//                             / temperature (0 where masked) as an image P[64][32 + 4] in LDS, then dz_hat^T[feature][query] +=
//                             X^T[feature][key] P^T[key][query] in registers (the wave's 16 queries x all features).  Written once, along
//                             time; the frames a step trims are written as zeros by the first tile.
//   cpc_backward_kernel<.., 1>  the same code with the roles swapped: owns 64 FRAMES of z of one entry (for step s frame kappa is key index
//                             (kappa - max(s, 0)) mod t), loops over the steps, the query entries and the query tiles inside, and writes
//                             dz once.  No atomics, no sums across workgroups.
//   cpc_batch_forward_kernel  'batch': per time position tau a b x b block, b <= 64; a workgroup takes kCpcTT = 8 positions, keeps the 8 blocks
//                             in LDS [8][b][b + 1] and accumulates them over staged groups of 4 features (plain fmaf chains, feature
//                             ascending); then a thread per (tau, query) adds log_batch_mask, applies the negative_ratio rule on the whole
//                             row (key j stays iff #{i : score_i >= score_j} >= kk or j is the target) and reduces it.
//   cpc_batch_backward_kernel owns 8 FRAMES, loops over the steps inside: the blocks again, dscore in their place, then per group of 4
//                             features dz_hat (direct) and dz (the owning thread adds step after step into its own element).
#include <math.h>

#include "common.h"

namespace ptmi {

constexpr int kCpcBM = 64;            // owned rows of a workgroup (16 per wave)
constexpr int kCpcBN = 32;            // rows of a streamed tile
constexpr int kCpcDC = 128;           // features of a streamed chunk
constexpr int kCpcLD = kCpcBN + 4;    // row stride of the streamed chunk and of the dscore image
constexpr int kCpcMaxD = 512;
constexpr int kCpcMaxB = 64;
constexpr int kCpcMaxSteps = 16;
constexpr int kCpcTT = 8;             // 'batch': time positions of a workgroup
constexpr int kCpcFG = 4;             // 'batch': features of a staged group
constexpr int kCpcBS = kCpcFG * kCpcTT + 8;   // 'batch': row stride of a staged group

typedef float cpc_f32x4 __attribute__((ext_vector_type(4)));

struct CpcArgs {
    const float *z, *zh, *g, *lse, *log_batch_mask;
    long long z_sb, z_sd, zh_sb, zh_sd;
    int b, d, dp, t, S, dist, all, keep;
    float temp;
    int step[kCpcMaxSteps];
    long long off[kCpcMaxSteps];      // first row of the step in the flat [sum_s b T_s] outputs
    long long loff[kCpcMaxSteps];     // first element of the step in the flat dense logits
};

__device__ __forceinline__ int cpc_abs(int v) { return v < 0 ? -v : v; }

// R[f][(c + 16 (f & 3)) & 63] = src[f sd + (x + add) mod t], x = start + c < limit, f < d; zero elsewhere.  All 256 threads.
__device__ __forceinline__ void cpc_stage_owned(float* __restrict__ R, const float* __restrict__ src, long long sd, int d, int dp, int start,
                                                int limit, int add, int t) {
    for (int idx = threadIdx.x; idx < dp * kCpcBM; idx += 256) {
        const int f = idx >> 6, c = idx & 63, x = start + c;
        R[f * kCpcBM + ((c + 16 * (f & 3)) & 63)] = (f < d && x < limit) ? src[f * sd + (x + add) % t] : 0.f;
    }
}

// X[fl][c] = src[(c0 + fl) sd + (x + add) mod t], x = start + c < limit, fl < len; zero elsewhere.
__device__ __forceinline__ void cpc_stage_stream(float* __restrict__ X, const float* __restrict__ src, long long sd, int d, int c0, int len,
                                                 int start, int limit, int add, int t) {
    for (int idx = threadIdx.x; idx < len * kCpcBN; idx += 256) {
        const int fl = idx >> 5, c = idx & 31, f = c0 + fl, x = start + c;
        X[fl * kCpcLD + c] = (f < d && x < limit) ? src[f * sd + (x + add) % t] : 0.f;
    }
}

// acc[nb][r] += sum_f R[f][16 wave + 4 (lane >> 4) + r] X[f - c0][16 nb + (lane & 15)], f = c0 .. c0 + len ascending (len a multiple of 4)
__device__ __forceinline__ void cpc_scores(cpc_f32x4 (&acc)[2], const float* __restrict__ R, const float* __restrict__ X, int c0, int len,
                                           int wave, int lane) {
    const int kr = lane >> 4;
    const float* __restrict__ pa = R + (c0 + kr) * kCpcBM + ((wave * 16 + (lane & 15) + 16 * kr) & 63);
    const float* __restrict__ pb = X + kr * kCpcLD + (lane & 15);
    for (int kk = 0; kk < len; kk += 4) {
        const float a = pa[kk * kCpcBM];
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pb[kk * kCpcLD], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pb[kk * kCpcLD + 16], acc[1], 0, 0, 0);
    }
}

// the band with a hole around the target, in key-index space, for a key of the query's own entry
__device__ __forceinline__ bool cpc_masked(const CpcArgs& A, bool same, int q, int k) {
    return same && A.dist > 1 && k != q && cpc_abs(k - q) <= A.dist - 1;
}

// (m, s) <- (m, s) + (m2, s2): sums of exp(x - m)
__device__ __forceinline__ void cpc_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mn));
    m = mn;
}

// ------------------------------------------------------------------------------------------------ 'time' / 'all' forward
__global__ __launch_bounds__(256) void cpc_forward_kernel(const CpcArgs A, float* __restrict__ stats, long long total,
                                                          float* __restrict__ logits) {
    extern __shared__ __attribute__((aligned(16))) float cpc_lds[];
    float* __restrict__ R = cpc_lds;
    float* __restrict__ X = cpc_lds + A.dp * kCpcBM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int si = blockIdx.z, s = A.step[si], Ts = A.t - cpc_abs(s), i = blockIdx.y, q0 = blockIdx.x * kCpcBM;
    if (q0 >= Ts) return;
    const int qoff = s < 0 ? -s : 0, sh = s > 0 ? s : 0, t = A.t;
    cpc_stage_owned(R, A.zh + i * A.zh_sb + (long long)si * A.d * A.zh_sd, A.zh_sd, A.d, A.dp, q0, Ts, qoff, t);
    float m[4], sum[4], best[4], tgt[4];
    int bi[4], cnt[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = best[r] = tgt[r] = -INFINITY, sum[r] = 0.f, bi[r] = 0x7fffffff, cnt[r] = 0;
    const int ib0 = A.all ? 0 : i, ib1 = A.all ? A.b : i + 1;
    const long long K = A.all ? (long long)A.b * t : t;
    for (int ib = ib0; ib < ib1; ++ib) {
        const float* __restrict__ zb = A.z + ib * A.z_sb;
        const bool same = ib == i;
        for (int k0 = 0; k0 < t; k0 += kCpcBN) {
            cpc_f32x4 acc[2] = {cpc_f32x4{0.f, 0.f, 0.f, 0.f}, cpc_f32x4{0.f, 0.f, 0.f, 0.f}};
            for (int c0 = 0; c0 < A.dp; c0 += kCpcDC) {
                const int len = A.dp - c0 < kCpcDC ? A.dp - c0 : kCpcDC;
                __syncthreads();                            // the owned tile is staged / the chunk before has been read
                cpc_stage_stream(X, zb, A.z_sd, A.d, c0, len, k0, t, sh, t);
                __syncthreads();
                cpc_scores(acc, R, X, c0, len, wave, lane);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + wave * 16 + (lane >> 4) * 4 + r;
                float v[2];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    const int k = k0 + nb * 16 + (lane & 15);
                    const bool in = q < Ts && k < t;
                    v[nb] = (in && !cpc_masked(A, same, q, k)) ? acc[nb][r] / A.temp : -INFINITY;
                    const int kf = A.all ? ib * t + k : k;
                    if (logits && in) logits[A.loff[si] + ((long long)i * K + kf) * Ts + q] = v[nb];
                    if (in && same && k == q) tgt[r] = v[nb];
                    cnt[r] += v[nb] > -INFINITY ? 1 : 0;
                    if (v[nb] > best[r]) best[r] = v[nb], bi[r] = kf;
                }
                const float mn = fmaxf(m[r], fmaxf(v[0], v[1]));
                sum[r] = (m[r] == -INFINITY ? 0.f : sum[r] * expf(m[r] - mn)) + (v[0] == -INFINITY ? 0.f : expf(v[0] - mn)) +
                         (v[1] == -INFINITY ? 0.f : expf(v[1] - mn));
                m[r] = mn;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) {
            cpc_merge(m[r], sum[r], __shfl_xor(m[r], o, 64), __shfl_xor(sum[r], o, 64));
            const float ob = __shfl_xor(best[r], o, 64);
            const int oi = __shfl_xor(bi[r], o, 64);
            if (ob > best[r] || (ob == best[r] && oi < bi[r])) best[r] = ob, bi[r] = oi;     // ties: the lowest key index (torch.argmax)
            cnt[r] += __shfl_xor(cnt[r], o, 64);
            tgt[r] = fmaxf(tgt[r], __shfl_xor(tgt[r], o, 64));                               // one lane holds it, the others -inf
        }
        const int q = q0 + wave * 16 + (lane >> 4) * 4 + r;
        if ((lane & 15) == 0 && q < Ts) {
            const long long row = A.off[si] + (long long)i * Ts + q;
            const float lse = m[r] + logf(sum[r]);
            stats[row] = lse - tgt[r];
            stats[total + row] = bi[r] == (A.all ? i * t + q : q) ? 1.f : 0.f;
            stats[2 * total + row] = __int_as_float(cnt[r]);
            stats[3 * total + row] = lse;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 'time' / 'all' backward
// OWN_KEYS = 0: owns queries of (step blockIdx.z, entry blockIdx.y), streams key tiles, writes dz_hat.
// OWN_KEYS = 1: owns frames of z of entry blockIdx.y, streams the query tiles of every step (and entry), writes dz.
// NDB: 16-feature blocks of the output a wave holds (>= dp / 16; 8 per chunk).
template <int NDB, int OWN_KEYS>
__global__ __launch_bounds__(256) void cpc_backward_kernel(const CpcArgs A, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float cpc_lds[];
    float* __restrict__ R = cpc_lds;
    float* __restrict__ X = cpc_lds + A.dp * kCpcBM;
    const int xrows = A.dp < kCpcDC ? A.dp : kCpcDC;
    float* __restrict__ P = X + xrows * kCpcLD;             // dscore [owned 64][kCpcLD]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int own = blockIdx.y, o0 = blockIdx.x * kCpcBM, t = A.t;
    constexpr int NCH = (NDB + 7) / 8, NJ = NDB < 8 ? NDB : 8;
    const bool one_chunk = A.dp <= kCpcDC;
    cpc_f32x4 acc[NCH][NJ];
#pragma unroll
    for (int cb = 0; cb < NCH; ++cb)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[cb][j] = cpc_f32x4{0.f, 0.f, 0.f, 0.f};
    if (OWN_KEYS) {
        cpc_stage_owned(R, A.z + own * A.z_sb, A.z_sd, A.d, A.dp, o0, t, 0, t);
    } else {
        const int s = A.step[blockIdx.z], Ts = t - cpc_abs(s);
        if (o0 >= Ts && o0 > 0) return;                     // (tile 0 stays: it writes the trimmed frames even where T_s = 0)
        cpc_stage_owned(R, A.zh + own * A.zh_sb + (long long)blockIdx.z * A.d * A.zh_sd, A.zh_sd, A.d, A.dp, o0, Ts, s < 0 ? -s : 0, t);
    }
    const int si0 = OWN_KEYS ? 0 : blockIdx.z, si1 = OWN_KEYS ? A.S : blockIdx.z + 1;
    for (int si = si0; si < si1; ++si) {
        const int s = A.step[si], Ts = t - cpc_abs(s), qoff = s < 0 ? -s : 0, sh = s > 0 ? s : 0;
        const int e0 = A.all ? 0 : own, e1 = A.all ? A.b : own + 1;
        const int slimit = OWN_KEYS ? Ts : t;               // streamed rows: queries / key indices
        for (int e = e0; e < e1; ++e) {
            const bool same = e == own;
            const int qe = OWN_KEYS ? e : own;              // the queries' entry
            const float* __restrict__ src =
                OWN_KEYS ? A.zh + e * A.zh_sb + (long long)si * A.d * A.zh_sd : A.z + e * A.z_sb;
            const long long ssd = OWN_KEYS ? A.zh_sd : A.z_sd;
            const int sadd = OWN_KEYS ? qoff : sh;
            const long long row0 = A.off[si] + (long long)qe * Ts;
            for (int x0 = 0; x0 < slimit; x0 += kCpcBN) {
                cpc_f32x4 sc[2] = {cpc_f32x4{0.f, 0.f, 0.f, 0.f}, cpc_f32x4{0.f, 0.f, 0.f, 0.f}};
                for (int c0 = 0; c0 < A.dp; c0 += kCpcDC) {
                    const int len = A.dp - c0 < kCpcDC ? A.dp - c0 : kCpcDC;
                    __syncthreads();                        // the owned tile is staged / chunk and image before have been read
                    cpc_stage_stream(X, src, ssd, A.d, c0, len, x0, slimit, sadd, t);
                    __syncthreads();
                    cpc_scores(sc, R, X, c0, len, wave, lane);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int orow = wave * 16 + (lane >> 4) * 4 + r, o = o0 + orow;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        const int col = nb * 16 + (lane & 15), x = x0 + col;
                        const int q = OWN_KEYS ? x : o;
                        const int k = OWN_KEYS ? (o < t ? (o - sh + t) % t : t) : x;
                        float ds = 0.f;
                        if (q < Ts && k < t && !cpc_masked(A, same, q, k)) {
                            const float p = expf(sc[nb][r] / A.temp - A.lse[row0 + q]);
                            ds = A.g[row0 + q] * (p - ((same && k == q) ? 1.f : 0.f)) / A.temp;
                        }
                        P[orow * kCpcLD + col] = ds;
                    }
                }
#pragma unroll
                for (int cb = 0; cb < NCH; ++cb) {
                    const int c0 = cb * kCpcDC;
                    if (c0 < A.dp) {
                        const int len = A.dp - c0 < kCpcDC ? A.dp - c0 : kCpcDC;
                        __syncthreads();                    // the image is complete / the chunk before has been read
                        if (!one_chunk) {
                            cpc_stage_stream(X, src, ssd, A.d, c0, len, x0, slimit, sadd, t);
                            __syncthreads();
                        }
                        // out^T[feature][owned] += X^T[feature][streamed] P^T[streamed][owned]
#pragma unroll 2
                        for (int kk = 0; kk < kCpcBN; kk += 4) {
                            const float bv = P[(wave * 16 + (lane & 15)) * kCpcLD + kk + (lane >> 4)];
#pragma unroll
                            for (int j = 0; j < NJ; ++j)
                                if (j * 16 < len) {
                                    const int fl = j * 16 + (lane & 15);
                                    acc[cb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fl < len ? X[fl * kCpcLD + kk + (lane >> 4)] : 0.f, bv,
                                                                                      acc[cb][j], 0, 0, 0);
                                }
                        }
                    }
                }
            }
        }
    }
    // C[row = feature 4 (lane >> 4) + r][col = owned lane & 15]: stores run along time
    const int o = o0 + wave * 16 + (lane & 15);
    if (OWN_KEYS) {
        float* __restrict__ dst = out + (long long)own * A.d * t;
#pragma unroll
        for (int cb = 0; cb < NCH; ++cb)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = cb * kCpcDC + j * 16 + (lane >> 4) * 4 + r;
                    if (f < A.d && o < t) dst[(long long)f * t + o] = acc[cb][j][r];
                }
    } else {
        const int si = blockIdx.z, s = A.step[si], Ts = t - cpc_abs(s), qoff = s < 0 ? -s : 0;
        float* __restrict__ dst = out + ((long long)own * A.S + si) * A.d * t;
#pragma unroll
        for (int cb = 0; cb < NCH; ++cb)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = cb * kCpcDC + j * 16 + (lane >> 4) * 4 + r;
                    if (f < A.d && o < Ts) dst[(long long)f * t + o + qoff] = acc[cb][j][r];
                }
        if (o0 == 0) {                                      // the frames the step trims: in front (s < 0) or behind (s > 0)
            const int n = t - Ts, first = s < 0 ? 0 : Ts;
            for (int idx = threadIdx.x; idx < A.d * n; idx += 256) dst[(long long)(idx / n) * t + first + idx % n] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 'batch'
// sc[tl][i][j] = sum_f z_hat_s[i, f, tau + qoff] z[j, f, tau + sh], tau = tau0 + tl (0 where tau is outside [0, T_s)); all 256 threads.
__device__ __forceinline__ void cpc_batch_blocks(const CpcArgs& A, int si, int tau0, float* __restrict__ sc, float* __restrict__ Qs,
                                                 float* __restrict__ Zs) {
    const int b = A.b, s = A.step[si], Ts = A.t - cpc_abs(s), qoff = s < 0 ? -s : 0, sh = s > 0 ? s : 0;
    const float* __restrict__ zh = A.zh + (long long)si * A.d * A.zh_sd;
    const int n = kCpcTT * b * b;
    for (int f0 = 0; f0 < A.d; f0 += kCpcFG) {
        __syncthreads();                                    // the group before has been read
        for (int idx = threadIdx.x; idx < b * kCpcFG * kCpcTT; idx += 256) {
            const int tl = idx & 7, fl = (idx >> 3) & 3, x = idx >> 5, f = f0 + fl, tau = tau0 + tl;
            const bool ok = f < A.d && tau >= 0 && tau < Ts;
            Qs[x * kCpcBS + fl * kCpcTT + tl] = ok ? zh[x * A.zh_sb + f * A.zh_sd + tau + qoff] : 0.f;
            Zs[x * kCpcBS + fl * kCpcTT + tl] = ok ? A.z[x * A.z_sb + f * A.z_sd + tau + sh] : 0.f;
        }
        __syncthreads();
        for (int o = threadIdx.x; o < n; o += 256) {
            const int tl = o & 7, p = o >> 3, i = p / b, j = p - i * b;
            float* __restrict__ cell = sc + (tl * b + i) * (b + 1) + j;
            float v = f0 ? *cell : 0.f;
#pragma unroll
            for (int fl = 0; fl < kCpcFG; ++fl) v = fmaf(Qs[i * kCpcBS + fl * kCpcTT + tl], Zs[j * kCpcBS + fl * kCpcTT + tl], v);
            *cell = v;
        }
    }
    __syncthreads();
}

// The row (tl, i) of sc becomes the reference's logits: / temperature, + log_batch_mask[i], -inf for the keys the negative_ratio rule drops.
__device__ __forceinline__ void cpc_batch_row(const CpcArgs& A, float* __restrict__ row, int i) {
    const int b = A.b;
    for (int j = 0; j < b; ++j) row[j] = row[j] / A.temp + (A.log_batch_mask ? A.log_batch_mask[i * b + j] : 0.f);
    if (A.keep <= 1) return;                                // kk = 1: the threshold is the row's maximum, every key stays
    unsigned long long drop = 0ull;
    for (int j = 0; j < b; ++j) {
        int ge = 0;
        for (int i2 = 0; i2 < b; ++i2) ge += row[i2] >= row[j] ? 1 : 0;
        if (ge < A.keep && j != i) drop |= 1ull << j;
    }
    for (int j = 0; j < b; ++j)
        if ((drop >> j) & 1ull) row[j] = -INFINITY;
}

__global__ __launch_bounds__(256) void cpc_batch_forward_kernel(const CpcArgs A, float* __restrict__ stats, long long total,
                                                                float* __restrict__ logits) {
    extern __shared__ __attribute__((aligned(16))) float cpc_lds[];
    const int b = A.b, si = blockIdx.y, s = A.step[si], Ts = A.t - cpc_abs(s), tau0 = blockIdx.x * kCpcTT;
    if (tau0 >= Ts) return;
    float* __restrict__ sc = cpc_lds;
    float* __restrict__ Qs = sc + kCpcTT * b * (b + 1);
    float* __restrict__ Zs = Qs + b * kCpcBS;
    cpc_batch_blocks(A, si, tau0, sc, Qs, Zs);
    for (int rix = threadIdx.x; rix < kCpcTT * b; rix += 256) {
        const int tl = rix & 7, i = rix >> 3, tau = tau0 + tl;
        if (tau >= Ts) continue;
        float* __restrict__ row = sc + (tl * b + i) * (b + 1);
        cpc_batch_row(A, row, i);
        float m = -INFINITY, sum = 0.f;
        int arg = 0, cnt = 0;
        for (int j = 0; j < b; ++j) {
            if (row[j] > m) m = row[j], arg = j;            // strict: the first maximal key
            cnt += row[j] > -INFINITY ? 1 : 0;
            if (logits) logits[A.loff[si] + ((long long)i * b + j) * Ts + tau] = row[j];
        }
        for (int j = 0; j < b; ++j) sum += row[j] == -INFINITY ? 0.f : expf(row[j] - m);
        const float lse = m + logf(sum);
        const long long r = A.off[si] + (long long)i * Ts + tau;
        stats[r] = lse - row[i];
        stats[total + r] = arg == i ? 1.f : 0.f;
        stats[2 * total + r] = __int_as_float(cnt);
        stats[3 * total + r] = lse;
    }
}

__global__ __launch_bounds__(256) void cpc_batch_backward_kernel(const CpcArgs A, float* __restrict__ dzh, float* __restrict__ dz) {
    extern __shared__ __attribute__((aligned(16))) float cpc_lds[];
    const int b = A.b, t = A.t, u0 = blockIdx.x * kCpcTT;
    float* __restrict__ sc = cpc_lds;
    float* __restrict__ Qs = sc + kCpcTT * b * (b + 1);
    float* __restrict__ Zs = Qs + b * kCpcBS;
    for (int si = 0; si < A.S; ++si) {
        const int s = A.step[si], Ts = t - cpc_abs(s), qoff = s < 0 ? -s : 0, sh = s > 0 ? s : 0, tau0 = u0 - sh;
        cpc_batch_blocks(A, si, tau0, sc, Qs, Zs);
        for (int rix = threadIdx.x; rix < kCpcTT * b; rix += 256) {
            const int tl = rix & 7, i = rix >> 3, tau = tau0 + tl;
            float* __restrict__ row = sc + (tl * b + i) * (b + 1);
            if (tau < 0 || tau >= Ts) {
                for (int j = 0; j < b; ++j) row[j] = 0.f;
                continue;
            }
            cpc_batch_row(A, row, i);
            const long long r = A.off[si] + (long long)i * Ts + tau;
            const float lse = A.lse[r], g = A.g[r];
            for (int j = 0; j < b; ++j) row[j] = row[j] == -INFINITY ? 0.f : g * (expf(row[j] - lse) - (j == i ? 1.f : 0.f)) / A.temp;
        }
        const float* __restrict__ zh = A.zh + (long long)si * A.d * A.zh_sd;
        for (int f0 = 0; f0 < A.d; f0 += kCpcFG) {
            __syncthreads();                                // dscore is complete / the group before has been read
            for (int idx = threadIdx.x; idx < b * kCpcFG * kCpcTT; idx += 256) {
                const int tl = idx & 7, fl = (idx >> 3) & 3, x = idx >> 5, f = f0 + fl, tau = tau0 + tl;
                const bool ok = f < A.d && tau >= 0 && tau < Ts;
                Qs[x * kCpcBS + fl * kCpcTT + tl] = ok ? zh[x * A.zh_sb + f * A.zh_sd + tau + qoff] : 0.f;
                Zs[x * kCpcBS + fl * kCpcTT + tl] = ok ? A.z[x * A.z_sb + f * A.z_sd + tau + sh] : 0.f;
            }
            __syncthreads();
            for (int idx = threadIdx.x; idx < b * kCpcFG * kCpcTT; idx += 256) {
                const int tl = idx & 7, fl = (idx >> 3) & 3, x = idx >> 5, f = f0 + fl, tau = tau0 + tl, u = u0 + tl;
                if (f >= A.d || u >= t) continue;
                float dq = 0.f, dk = 0.f;
                for (int y = 0; y < b; ++y) {
                    dq = fmaf(sc[(tl * b + x) * (b + 1) + y], Zs[y * kCpcBS + fl * kCpcTT + tl], dq);
                    dk = fmaf(sc[(tl * b + y) * (b + 1) + x], Qs[y * kCpcBS + fl * kCpcTT + tl], dk);
                }
                float* __restrict__ qrow = dzh + ((long long)x * A.S * A.d + (long long)si * A.d + f) * t;
                if (tau >= 0 && tau < Ts) qrow[tau + qoff] = dq;
                if ((s < 0 && u < -s) || (s > 0 && u >= Ts)) qrow[u] = 0.f;      // a frame the step trims
                float* __restrict__ cell = dz + ((long long)x * A.d + f) * t + u;
                *cell = (si ? *cell : 0.f) + dk;            // this thread owns the element in every step
            }
        }
        __syncthreads();                                    // before the next step's blocks overwrite sc
    }
}

// geom (host): b, d, t, z_sb, z_sd, zh_sb, zh_sd, S, steps[S]
static int cpc_args(CpcArgs& A, const float* z_hat, const float* z, const int64_t* geom, int32_t mode, float temperature, int32_t dist,
                    long long& total) {
    PTMI_RETURN_IF(!z_hat || !z || !geom || mode < 0 || mode > 2 || !(temperature > 0.f), PTMI_E_INVALID);
    const int64_t b = geom[0], d = geom[1], t = geom[2], S = geom[7];
    PTMI_RETURN_IF(b < 1 || d < 1 || t < 1 || S < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(d > kCpcMaxD || S > kCpcMaxSteps || b * t >= (1LL << 31) || b * S * d * t >= (1LL << 40), PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(mode == 2 && b > kCpcMaxB, PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(b > 65535, PTMI_E_UNSUPPORTED);
    A.z = z, A.zh = z_hat, A.z_sb = geom[3], A.z_sd = geom[4], A.zh_sb = geom[5], A.zh_sd = geom[6];
    A.b = (int)b, A.d = (int)d, A.dp = (int)((d + 3) / 4 * 4), A.t = (int)t, A.S = (int)S, A.dist = dist, A.all = mode == 1, A.keep = 1;
    A.temp = temperature;
    const long long K = mode == 0 ? t : (mode == 1 ? b * t : b);
    long long off = 0, loff = 0;
    for (int i = 0; i < S; ++i) {
        const int64_t s = geom[8 + i], Ts = t - (s < 0 ? -s : s);
        PTMI_RETURN_IF(Ts < 1, PTMI_E_INVALID);
        A.step[i] = (int)s, A.off[i] = off, A.loff[i] = loff;
        off += b * Ts, loff += b * K * Ts;
    }
    total = off;
    return PTMI_OK;
}

static int cpc_allow_lds(const void* fn, size_t bytes) {
    if (bytes > 64 * 1024)
        PTMI_RETURN_IF(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess, PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

static size_t cpc_batch_lds(int b) { return ((size_t)kCpcTT * b * (b + 1) + 2 * (size_t)b * kCpcBS) * sizeof(float); }

template <int NDB>
static int cpc_launch_backward(const CpcArgs& A, float* dz_hat, float* dz, hipStream_t st) {
    const int xrows = A.dp < kCpcDC ? A.dp : kCpcDC;
    const size_t lds = ((size_t)A.dp * kCpcBM + (size_t)xrows * kCpcLD + (size_t)kCpcBM * kCpcLD) * sizeof(float);
    const unsigned tiles = (unsigned)((A.t + kCpcBM - 1) / kCpcBM);
    if (dz_hat) {
        int rc = cpc_allow_lds(reinterpret_cast<const void*>(cpc_backward_kernel<NDB, 0>), lds);
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
        hipLaunchKernelGGL((cpc_backward_kernel<NDB, 0>), dim3(tiles, (unsigned)A.b, (unsigned)A.S), dim3(256), lds, st, A, dz_hat);
        rc = launch_status();
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
    }
    if (dz) {
        int rc = cpc_allow_lds(reinterpret_cast<const void*>(cpc_backward_kernel<NDB, 1>), lds);
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
        hipLaunchKernelGGL((cpc_backward_kernel<NDB, 1>), dim3(tiles, (unsigned)A.b, 1), dim3(256), lds, st, A, dz);
        return launch_status();
    }
    return PTMI_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_cpc_max_features(void) { return kCpcMaxD; }

int32_t ptmi_cpc_max_batch(void) { return kCpcMaxB; }

int32_t ptmi_cpc_max_steps(void) { return kCpcMaxSteps; }

int32_t ptmi_cpc_query_tile(void) { return kCpcBM; }

int32_t ptmi_cpc_key_tile(void) { return kCpcBN; }

int ptmi_cpc_forward(const float* z_hat, const float* z, const int64_t* geom, int32_t mode, float temperature, int32_t dist,
                     const float* log_batch_mask, int32_t keep, float* stats, float* logits, ptmi_stream_t stream) {
    CpcArgs A = {};
    long long total = 0;
    int rc = cpc_args(A, z_hat, z, geom, mode, temperature, dist, total);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    PTMI_RETURN_IF(!stats || (mode == 2 && keep < 1), PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == 2) {
        A.log_batch_mask = log_batch_mask, A.keep = keep;
        const size_t lds = cpc_batch_lds(A.b);
        rc = cpc_allow_lds(reinterpret_cast<const void*>(cpc_batch_forward_kernel), lds);
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
        hipLaunchKernelGGL(cpc_batch_forward_kernel, dim3((unsigned)((A.t + kCpcTT - 1) / kCpcTT), (unsigned)A.S), dim3(256), lds, st, A, stats,
                           total, logits);
        return launch_status();
    }
    const int xrows = A.dp < kCpcDC ? A.dp : kCpcDC;
    const size_t lds = ((size_t)A.dp * kCpcBM + (size_t)xrows * kCpcLD) * sizeof(float);
    rc = cpc_allow_lds(reinterpret_cast<const void*>(cpc_forward_kernel), lds);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    hipLaunchKernelGGL(cpc_forward_kernel, dim3((unsigned)((A.t + kCpcBM - 1) / kCpcBM), (unsigned)A.b, (unsigned)A.S), dim3(256), lds, st, A,
                       stats, total, logits);
    return launch_status();
}

int ptmi_cpc_backward(const float* z_hat, const float* z, const int64_t* geom, int32_t mode, float temperature, int32_t dist,
                      const float* log_batch_mask, int32_t keep, const float* lse, const float* g, float* dz_hat, float* dz,
                      ptmi_stream_t stream) {
    CpcArgs A = {};
    long long total = 0;
    int rc = cpc_args(A, z_hat, z, geom, mode, temperature, dist, total);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    PTMI_RETURN_IF(!lse || !g || (mode == 2 && (keep < 1 || !dz_hat || !dz)), PTMI_E_INVALID);
    A.lse = lse, A.g = g;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == 2) {
        A.log_batch_mask = log_batch_mask, A.keep = keep;
        const size_t lds = cpc_batch_lds(A.b);
        rc = cpc_allow_lds(reinterpret_cast<const void*>(cpc_batch_backward_kernel), lds);
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
        hipLaunchKernelGGL(cpc_batch_backward_kernel, dim3((unsigned)((A.t + kCpcTT - 1) / kCpcTT)), dim3(256), lds, st, A, dz_hat, dz);
        return launch_status();
    }
    return A.dp <= 32    ? cpc_launch_backward<2>(A, dz_hat, dz, st)
           : A.dp <= 64  ? cpc_launch_backward<4>(A, dz_hat, dz, st)
           : A.dp <= 128 ? cpc_launch_backward<8>(A, dz_hat, dz, st)
           : A.dp <= 256 ? cpc_launch_backward<16>(A, dz_hat, dz, st)
                         : cpc_launch_backward<32>(A, dz_hat, dz, st);
}

}  // extern "C"
