// The pairwise KL divergence between B diagonal Gaussian posteriors and K Gaussian prior components (include/ptmi.h: ptmi_gkl_*).
//
// Replaces padertorch/ops/losses/kl_divergence.py:17-60 (a batched general inverse(), a [K, B, D] difference tensor, a batched matmul and
// the temporaries autograd keeps).  Nothing of size B K D is written.  mu, sigma [B, D]; m [K, D]; the prior's scale is either
// scale_tril T [K, D, D] (FULL: only the lower triangle is read) or a diagonal s [K, D].  fp32, D <= 64, padded to DP = 16 NB.
// With L = T^-1, c_d = sum_i L[i, d]^2, diff = m - mu, y = L diff:
//
//   kl[b, k] = sum_d log T_dd - sum_d log sigma_bd + 1/2 (sum_d c_d sigma_bd^2 + |y|^2 - D)          (diagonal: L = diag(1 / s))
//
// Products run on the matrix cores as v_mfma_f32_16x16x4_f32.  Lane maps as in cpc_contrast.hip: A[row = l & 15][k = l >> 4],
// B[k = l >> 4][col = l & 15], C[row = 4 (l >> 4) + r][col = l & 15] in register r.  Below g = l >> 4, cl = l & 15.
//
//   gkl_prepare_kernel         a workgroup per component: T staged in LDS padded with an identity diagonal, inverted by forward
//                              substitution (a thread per column of L), writes L [K, DP, DP], c [K, DP], logdet [K].
//   gkl_forward_kernel         a workgroup of 4 waves OWNS 64 rows b: mu sits in registers in the A layout, sigma^2 in the C layout.  The
//                              components STREAM through two LDS slots (L_k [DP][DP + 4], m_k, c_k): the next one is fetched into
//                              registers in front of the MFMAs and put into LDS behind them, one barrier per component.  y = diff L^T
//                              takes DP / 4 MFMAs per 16 columns; y^2 + c sigma^2 is reduced over the 16 column lanes; lane cl keeps
//                              the value of component 16 j + cl and the tile stores 16 contiguous components at a time.
//   gkl_backward_rows_kernel   the same streaming; y again, G y through a wave-private LDS image into the A layout, then
//                              dmu^T += (G y) L accumulated in the MFMA accumulators over all k; dsigma's sum_k G c in registers.  G
//                              arrives in [64][16] blocks.  Every element of dmu / dsigma is written once.
//   gkl_backward_comps_kernel  grid (component, row split): L_k stays in LDS, the row tiles stream through LDS as diff and sigma^2
//                              images.  y in the C layout IS the A operand of the outer product dL += (G y)^T diff when the MFMA's four
//                              k indices are taken as rows 4 j + r (register r): no transpose.  Partials [S, K, ...] : dL, w = sum_b G y,
//                              v = sum_b G sigma^2, gs = sum_b G (diagonal: sum_b G diff, sum_b G (sigma^2 + diff^2), gs).
//   gkl_finish_kernel          a workgroup per component: the S partials summed in order, dL += L o v, then
//                              dT = -tril(L^T dL L^T) + diag(gs / T_dd), dm = L^T w (diagonal: ds, dm elementwise).
// No atomics, nothing read on the host: capturable.
#include <math.h>

#include "common.h"

namespace ptmi {

constexpr int kGklMaxD = 64;
constexpr int kGklBM = 64;             // rows a row-owning workgroup owns / rows of a streamed row tile
constexpr int kGklSplitRows = 1024;    // rows of one (component, split) workgroup
constexpr int kGklGB = 16;             // components of a G block / of a kl store
constexpr int kGklGLD = kGklGB + 1;
constexpr long long kGklMaxRows = 1LL << 25, kGklMaxComps = 1LL << 25;

typedef float gkl_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gkl_sum16(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float gkl_sum_groups(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

__device__ __forceinline__ void gkl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a component in LDS: L [DP][DP + 4] (FULL), m [DP], c [DP]
template <int NB, bool FULL>
struct GklSlot {
    static constexpr int DP = 16 * NB, LD = DP + 4, MAT = FULL ? DP * LD : 0, SIZE = MAT + 2 * DP;
    float l[FULL ? NB * NB : 1], m, c;

    __device__ __forceinline__ void fetch(const float* __restrict__ L, const float* __restrict__ mean, const float* __restrict__ c_, int k,
                                          int D) {
        const int tid = threadIdx.x;
        if (FULL) {
            const float* __restrict__ src = L + (long long)k * DP * DP;
#pragma unroll
            for (int j = 0; j < NB * NB; ++j) l[j] = src[j * 256 + tid];
        }
        m = tid < D ? mean[(long long)k * D + tid] : 0.f;
        c = tid < DP ? c_[(long long)k * DP + tid] : 0.f;
    }

    __device__ __forceinline__ void put(float* __restrict__ slot) const {
        const int tid = threadIdx.x;
        if (FULL) {
#pragma unroll
            for (int j = 0; j < NB * NB; ++j) {
                const int idx = j * 256 + tid;
                slot[(idx / DP) * LD + idx % DP] = l[j];
            }
        }
        if (tid < DP) slot[MAT + tid] = m, slot[MAT + DP + tid] = c;
    }
};

// acc[nb][r] = y[row 4 g + r][i = 16 nb + cl] = sum_d a(d) L[i][d]; a(kk) is the lane's diff at d = 4 kk + g of row cl
template <int NB, typename F>
__device__ __forceinline__ void gkl_y(gkl_f32x4 (&acc)[NB], const float* __restrict__ Lk, int g, int cl, F a) {
    constexpr int DP = 16 * NB, LD = DP + 4;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = gkl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < DP / 4; ++kk) {
        const float av = a(kk);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Lk[(16 * nb + cl) * LD + 4 * kk + g], acc[nb], 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------ component preparation
__global__ __launch_bounds__(256) void gkl_prepare_kernel(const float* __restrict__ scale, int full, int D, int DP, float* __restrict__ L,
                                                          float* __restrict__ c, float* __restrict__ logdet) {
    extern __shared__ __attribute__((aligned(16))) float gkl_lds[];
    const int k = blockIdx.x, tid = threadIdx.x, LD = DP + 1;
    float lg = 0.f;
    if (!full) {
        if (tid < DP) {
            const float sv = tid < D ? scale[(long long)k * D + tid] : 1.f;
            c[(long long)k * DP + tid] = tid < D ? 1.f / (sv * sv) : 0.f;
            lg = logf(sv);
        }
    } else {
        float* __restrict__ T = gkl_lds;
        float* __restrict__ X = gkl_lds + DP * LD;
        const float* __restrict__ src = scale + (long long)k * D * D;
        for (int idx = tid; idx < DP * DP; idx += 256) {
            const int i = idx / DP, d = idx % DP;
            T[i * LD + d] = (i < D && d < D) ? (d <= i ? src[i * D + d] : 0.f) : (i == d ? 1.f : 0.f);
        }
        __syncthreads();
        if (tid < DP) {                                     // column tid of L: T x = e_tid
            float cj = 0.f;
            for (int i = 0; i < DP; ++i) {
                float x = 0.f;
                if (i >= tid) {
                    float sum = i == tid ? 1.f : 0.f;
                    for (int l = tid; l < i; ++l) sum = fmaf(-T[i * LD + l], X[l * LD + tid], sum);
                    x = sum / T[i * LD + i];
                }
                X[i * LD + tid] = x;
                cj = fmaf(x, x, cj);
            }
            c[(long long)k * DP + tid] = cj;
            lg = logf(T[tid * LD + tid]);
        }
        __syncthreads();
        float* __restrict__ dst = L + (long long)k * DP * DP;
        for (int idx = tid; idx < DP * DP; idx += 256) dst[idx] = X[(idx / DP) * LD + idx % DP];
    }
    if (tid < 64) {                                         // DP <= 64: the first wave holds every diagonal element
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) lg += __shfl_xor(lg, o, 64);
        if (tid == 0) logdet[k] = lg;
    }
}

// ------------------------------------------------------------------------------------------------ pairwise forward, row-owning
template <int NB, bool FULL>
__global__ __launch_bounds__(256) void gkl_forward_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                          const float* __restrict__ mean, const float* __restrict__ L,
                                                          const float* __restrict__ c, const float* __restrict__ logdet, int B, int K, int D,
                                                          float* __restrict__ kl) {
    typedef GklSlot<NB, FULL> Slot;
    constexpr int DP = Slot::DP;
    extern __shared__ __attribute__((aligned(16))) float gkl_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, cl = lane & 15;
    const long long row0 = (long long)blockIdx.x * kGklBM + wave * 16;
    float muC[FULL ? 1 : NB][4], s2C[NB][4], lsig[4], muA[FULL ? DP / 4 : 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long b = row0 + 4 * g + r;
        float ls = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int d = 16 * nb + cl;
            const bool ok = b < B && d < D;
            const float sg = ok ? sigma[b * D + d] : 1.f;
            s2C[nb][r] = ok ? sg * sg : 0.f;
            if (!FULL) muC[nb][r] = ok ? mu[b * D + d] : 0.f;
            ls += logf(sg);
        }
        lsig[r] = gkl_sum16(ls);
    }
    if (FULL) {
#pragma unroll
        for (int kk = 0; kk < DP / 4; ++kk) {
            const long long b = row0 + cl;
            const int d = 4 * kk + g;
            muA[kk] = (b < B && d < D) ? mu[b * D + d] : 0.f;
        }
    }
    Slot P;
    P.fetch(L, mean, c, 0, D);
    P.put(gkl_lds);
    __syncthreads();
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
        const float* __restrict__ Lk = gkl_lds + (k & 1) * Slot::SIZE;
        const float* __restrict__ mk = Lk + Slot::MAT;
        const float* __restrict__ ck = mk + DP;
        if (k + 1 < K) P.fetch(L, mean, c, k + 1, D);
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (FULL) {
            gkl_f32x4 acc[NB];
            gkl_y<NB>(acc, Lk, g, cl, [&](int kk) { return mk[4 * kk + g] - muA[kk]; });
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float cc = ck[16 * nb + cl];
#pragma unroll
                for (int r = 0; r < 4; ++r) q[r] = fmaf(acc[nb][r], acc[nb][r], fmaf(cc, s2C[nb][r], q[r]));
            }
        } else {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float cc = ck[16 * nb + cl], mm = mk[16 * nb + cl];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float df = mm - muC[nb][r];
                    q[r] = fmaf(cc, fmaf(df, df, s2C[nb][r]), q[r]);
                }
            }
        }
        const float ld = logdet[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = ld - lsig[r] + 0.5f * (gkl_sum16(q[r]) - (float)D);
            if (cl == (k & (kGklGB - 1))) out[r] = v;
        }
        if ((k & (kGklGB - 1)) == kGklGB - 1 || k == K - 1) {
            const int col = (k & ~(kGklGB - 1)) + cl;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long b = row0 + 4 * g + r;
                if (b < B && col < K) kl[b * K + col] = out[r];
            }
        }
        if (k + 1 < K) P.put(gkl_lds + ((k + 1) & 1) * Slot::SIZE);
        __syncthreads();                                    // slot k + 1 is complete; slot k has been read
    }
}

// ------------------------------------------------------------------------------------------------ backward, row-owning
template <int NB, bool FULL>
__global__ __launch_bounds__(256) void gkl_backward_rows_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                const float* __restrict__ mean, const float* __restrict__ L,
                                                                const float* __restrict__ c, const float* __restrict__ G, int B, int K,
                                                                int D, float* __restrict__ dmu, float* __restrict__ dsigma) {
    typedef GklSlot<NB, FULL> Slot;
    constexpr int DP = Slot::DP, LD = Slot::LD, YS = FULL ? 16 * LD : 0;
    extern __shared__ __attribute__((aligned(16))) float gkl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, cl = lane & 15;
    float* __restrict__ Ys = gkl_lds + 2 * Slot::SIZE + wave * YS;             // the wave's image of G y [16][LD]
    float* __restrict__ Gs = gkl_lds + 2 * Slot::SIZE + 4 * YS;                // two blocks [64][17]
    const long long tile0 = (long long)blockIdx.x * kGklBM, row0 = tile0 + wave * 16;
    float muC[FULL ? 1 : NB][4], muA[FULL ? DP / 4 : 1];
    if (FULL) {
#pragma unroll
        for (int kk = 0; kk < DP / 4; ++kk) {
            const long long b = row0 + cl;
            const int d = 4 * kk + g;
            muA[kk] = (b < B && d < D) ? mu[b * D + d] : 0.f;
        }
    } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long b = row0 + 4 * g + r;
                const int d = 16 * nb + cl;
                muC[nb][r] = (b < B && d < D) ? mu[b * D + d] : 0.f;
            }
    }
    gkl_f32x4 accm[NB];
    float accs[NB][4], gsum[4] = {0.f, 0.f, 0.f, 0.f}, pg[4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        accm[nb] = gkl_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) accs[nb][r] = 0.f;
    }
    auto fetch_g = [&](int k0) {                            // G[tile rows][k0 .. k0 + 16): thread -> (row idx >> 4, column idx & 15)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = j * 256 + tid, col = k0 + (idx & 15);
            const long long b = tile0 + (idx >> 4);
            pg[j] = (b < B && col < K) ? G[b * K + col] : 0.f;
        }
    };
    auto put_g = [&](int k0) {
        float* __restrict__ dst = Gs + ((k0 >> 4) & 1) * kGklBM * kGklGLD;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = j * 256 + tid;
            dst[(idx >> 4) * kGklGLD + (idx & 15)] = pg[j];
        }
    };
    Slot P;
    P.fetch(L, mean, c, 0, D);
    P.put(gkl_lds);
    fetch_g(0);
    put_g(0);
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const float* __restrict__ Lk = gkl_lds + (k & 1) * Slot::SIZE;
        const float* __restrict__ mk = Lk + Slot::MAT;
        const float* __restrict__ ck = mk + DP;
        const bool next = k + 1 < K, next_g = next && ((k + 1) & (kGklGB - 1)) == 0;
        if (next) P.fetch(L, mean, c, k + 1, D);
        if (next_g) fetch_g(k + 1);
        float gv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gv[r] = Gs[((k >> 4) & 1) * kGklBM * kGklGLD + (wave * 16 + 4 * g + r) * kGklGLD + (k & (kGklGB - 1))];
            gsum[r] += gv[r];
        }
        if (FULL) {
            gkl_f32x4 acc[NB];
            gkl_y<NB>(acc, Lk, g, cl, [&](int kk) { return mk[4 * kk + g] - muA[kk]; });
            gkl_wave_sync();                                // the image of the component before has been read
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ys[(4 * g + r) * LD + 16 * nb + cl] = gv[r] * acc[nb][r];
            gkl_wave_sync();
            // (G z)[row][d] += sum_i (G y)[row][i] L[i][d]
#pragma unroll
            for (int kk = 0; kk < DP / 4; ++kk) {
                const float av = Ys[cl * LD + 4 * kk + g];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    accm[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Lk[(4 * kk + g) * LD + 16 * nb + cl], accm[nb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const float cc = ck[16 * nb + cl];
            const float mm = FULL ? 0.f : mk[16 * nb + cl];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gc = gv[r] * cc;
                accs[nb][r] += gc;
                if (!FULL) accm[nb][r] = fmaf(gc, mm - muC[nb][r], accm[nb][r]);
            }
        }
        if (next) P.put(gkl_lds + ((k + 1) & 1) * Slot::SIZE);
        if (next_g) put_g(k + 1);
        __syncthreads();                                    // slot and block k + 1 are complete; slot k has been read
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long b = row0 + 4 * g + r;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int d = 16 * nb + cl;
            if (b < B && d < D) {
                const float sg = sigma[b * D + d];
                dmu[b * D + d] = -accm[nb][r];
                dsigma[b * D + d] = sg * accs[nb][r] - gsum[r] / sg;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, component-owning
template <int NB, bool FULL>
__global__ __launch_bounds__(256) void gkl_backward_comps_kernel(const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                 const float* __restrict__ mean, const float* __restrict__ L,
                                                                 const float* __restrict__ c, const float* __restrict__ G, int B, int K,
                                                                 int D, float* __restrict__ ws) {
    typedef GklSlot<NB, FULL> Slot;
    constexpr int DP = Slot::DP, LD = Slot::LD, WS = (FULL ? DP * DP : 0) + 3 * DP;
    extern __shared__ __attribute__((aligned(16))) float gkl_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, cl = lane & 15;
    const int k = blockIdx.x;
    const long long b_begin = (long long)blockIdx.y * kGklSplitRows;
    const long long b_end = b_begin + kGklSplitRows < B ? b_begin + kGklSplitRows : B;
    float* __restrict__ Lk = gkl_lds;
    float* __restrict__ mk = Lk + Slot::MAT;
    float* __restrict__ Dt = gkl_lds + Slot::SIZE;          // diff [64][LD]
    float* __restrict__ St = Dt + kGklBM * LD;              // sigma^2 [64][LD]
    float* __restrict__ Gt = St + kGklBM * LD;              // G[., k] [64]
    {
        Slot P;
        P.fetch(L, mean, c, k, D);
        P.put(Lk);
    }
    gkl_f32x4 accL[FULL ? NB : 1][FULL ? NB : 1];
    float vec0[NB], vec1[NB], gs = 0.f;                     // FULL: w, v; diagonal: sum G diff, sum G (sigma^2 + diff^2)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) vec0[nb] = vec1[nb] = 0.f;
    if (FULL) {
#pragma unroll
        for (int ib = 0; ib < NB; ++ib)
#pragma unroll
            for (int db = 0; db < NB; ++db) accL[ib][db] = gkl_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (long long t0 = b_begin; t0 < b_end; t0 += kGklBM) {
        __syncthreads();                                    // the component is staged / the tile before has been read
#pragma unroll
        for (int j = 0; j < 4 * NB; ++j) {
            const int idx = j * 256 + tid, row = idx / DP, d = idx % DP;
            const long long b = t0 + row;
            const bool ok = b < b_end && d < D;
            const float sg = ok ? sigma[b * D + d] : 0.f;
            Dt[row * LD + d] = ok ? mk[d] - mu[b * D + d] : 0.f;
            St[row * LD + d] = sg * sg;
        }
        if (tid < kGklBM) Gt[tid] = t0 + tid < b_end ? G[(t0 + tid) * K + k] : 0.f;
        __syncthreads();
        const float* __restrict__ drow = Dt + (wave * 16 + 4 * g) * LD + cl;   // + r LD + 16 db: the C layout of the wave's rows
        const float* __restrict__ srow = St + (wave * 16 + 4 * g) * LD + cl;
        float gv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) gv[r] = Gt[wave * 16 + 4 * g + r], gs += gv[r];
        if (FULL) {
            gkl_f32x4 acc[NB];
            const float* __restrict__ arow = Dt + (wave * 16 + cl) * LD + g;
            gkl_y<NB>(acc, Lk, g, cl, [&](int kk) { return arow[4 * kk]; });
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[nb][r] *= gv[r], vec0[nb] += acc[nb][r];
            // dL[i][d] += sum_rows (G y)[row][i] diff[row][d]; step r contracts the rows 4 j + r, j = 0..3: the C layout is the A operand
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int db = 0; db < NB; ++db) {
                    const float bv = drow[r * LD + 16 * db];
                    vec1[db] = fmaf(gv[r], srow[r * LD + 16 * db], vec1[db]);
#pragma unroll
                    for (int ib = 0; ib < NB; ++ib)
                        accL[ib][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[ib][r], bv, accL[ib][db], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int db = 0; db < NB; ++db) {
                    const float df = drow[r * LD + 16 * db];
                    vec0[db] = fmaf(gv[r], df, vec0[db]);
                    vec1[db] = fmaf(gv[r], fmaf(df, df, srow[r * LD + 16 * db]), vec1[db]);
                }
        }
    }
    // the four waves' partials in wave order: matrices in the diff image, vectors in the sigma^2 image
    gs = gkl_sum_groups(gs);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) vec0[nb] = gkl_sum_groups(vec0[nb]), vec1[nb] = gkl_sum_groups(vec1[nb]);
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) St[wave * 3 * DP + 16 * nb + cl] = vec0[nb], St[wave * 3 * DP + DP + 16 * nb + cl] = vec1[nb];
        St[wave * 3 * DP + 2 * DP + cl] = cl == 0 ? gs : 0.f;
        if (DP > 16 && cl == 0)
            for (int d = 16; d < DP; ++d) St[wave * 3 * DP + 2 * DP + d] = 0.f;
    }
    if (FULL) {
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
#pragma unroll
                    for (int db = 0; db < NB; ++db)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float* __restrict__ cell = Dt + (16 * ib + 4 * g + r) * DP + 16 * db + cl;
                            *cell = (w ? *cell : 0.f) + accL[ib][db][r];
                        }
            }
            __syncthreads();
        }
    } else {
        __syncthreads();
    }
    float* __restrict__ dst = ws + ((long long)blockIdx.y * K + k) * WS;
    if (FULL)
        for (int idx = tid; idx < DP * DP; idx += 256) dst[idx] = Dt[idx];
    for (int idx = tid; idx < 3 * DP; idx += 256)
        dst[(FULL ? DP * DP : 0) + idx] = (St[idx] + St[3 * DP + idx]) + (St[6 * DP + idx] + St[9 * DP + idx]);
}

// ------------------------------------------------------------------------------------------------ component finish
__global__ __launch_bounds__(256) void gkl_finish_kernel(const float* __restrict__ ws, int S, int K, int D, int DP, int full,
                                                         const float* __restrict__ L, const float* __restrict__ scale,
                                                         float* __restrict__ dm, float* __restrict__ dscale) {
    extern __shared__ __attribute__((aligned(16))) float gkl_lds[];
    const int k = blockIdx.x, tid = threadIdx.x, LD = DP + 1, MAT = full ? DP * DP : 0, WS = MAT + 3 * DP;
    float* __restrict__ vec = gkl_lds;                      // [3][DP]
    float* __restrict__ Lk = vec + 3 * DP;                  // [DP][LD]
    float* __restrict__ A = Lk + DP * LD;
    float* __restrict__ M = A + DP * LD;
    const float* __restrict__ part = ws + (long long)k * WS;
    const long long step = (long long)K * WS;
    for (int idx = tid; idx < 3 * DP; idx += 256) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += part[s * step + MAT + idx];
        vec[idx] = sum;
    }
    if (!full) {
        __syncthreads();
        if (tid < D) {
            const float sv = scale[(long long)k * D + tid], r2 = 1.f / (sv * sv);
            dm[(long long)k * D + tid] = vec[tid] * r2;
            dscale[(long long)k * D + tid] = vec[2 * DP] / sv - vec[DP + tid] * r2 / sv;
        }
        return;
    }
    for (int idx = tid; idx < DP * DP; idx += 256) {
        float sum = 0.f;
        for (int s = 0; s < S; ++s) sum += part[s * step + idx];
        const int i = idx / DP, d = idx % DP;
        Lk[i * LD + d] = L[(long long)k * DP * DP + idx];
        A[i * LD + d] = sum;
    }
    __syncthreads();
    for (int idx = tid; idx < DP * DP; idx += 256) {        // dL = tril(sum + L o v)
        const int i = idx / DP, d = idx % DP;
        A[i * LD + d] = d <= i ? fmaf(Lk[i * LD + d], vec[DP + d], A[i * LD + d]) : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < DP * DP; idx += 256) {        // M = dL L^T (L[j][d] = 0 for d > j)
        const int j = idx / DP, i = idx % DP;
        float sum = 0.f;
        for (int d = 0; d <= j; ++d) sum = fmaf(A[i * LD + d], Lk[j * LD + d], sum);
        M[i * LD + j] = sum;
    }
    __syncthreads();
    const float gs = vec[2 * DP];
    for (int idx = tid; idx < D * D; idx += 256) {          // dT = -tril(L^T M) + diag(gs / T_dd)
        const int a = idx / D, j = idx % D;
        float v = 0.f;
        if (j <= a) {
            float sum = 0.f;
            for (int i = a; i < DP; ++i) sum = fmaf(Lk[i * LD + a], M[i * LD + j], sum);
            v = -sum;
            if (j == a) v += gs / scale[(long long)k * D * D + idx];
        }
        dscale[(long long)k * D * D + idx] = v;
    }
    if (tid < D) {                                          // dm = L^T w
        float sum = 0.f;
        for (int i = tid; i < DP; ++i) sum = fmaf(Lk[i * LD + tid], vec[i], sum);
        dm[(long long)k * D + tid] = sum;
    }
}

static int gkl_dims(int64_t B, int64_t K, int32_t D) {
    PTMI_RETURN_IF(B < 1 || K < 1 || D < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(D > kGklMaxD || B > kGklMaxRows || K > kGklMaxComps, PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

static int gkl_dp(int D) { return (D + 15) / 16 * 16; }

static int64_t gkl_splits(int64_t B) { return (B + kGklSplitRows - 1) / kGklSplitRows; }

template <int NB, bool FULL>
static int gkl_launch_forward(const float* mu, const float* sigma, const float* m, const float* L, const float* c, const float* logdet, int B,
                              int K, int D, float* kl, hipStream_t st) {
    const size_t lds = 2 * (size_t)GklSlot<NB, FULL>::SIZE * sizeof(float);
    hipLaunchKernelGGL((gkl_forward_kernel<NB, FULL>), dim3((unsigned)((B + kGklBM - 1) / kGklBM)), dim3(256), lds, st, mu, sigma, m, L, c,
                       logdet, B, K, D, kl);
    return launch_status();
}

template <int NB, bool FULL>
static int gkl_launch_backward(const float* mu, const float* sigma, const float* m, const float* L, const float* c, const float* G, int B,
                               int K, int D, float* ws, float* dmu, float* dsigma, hipStream_t st) {
    typedef GklSlot<NB, FULL> Slot;
    const size_t rows_lds = (2 * (size_t)Slot::SIZE + (FULL ? 4 * 16 * Slot::LD : 0) + 2 * kGklBM * kGklGLD) * sizeof(float);
    hipLaunchKernelGGL((gkl_backward_rows_kernel<NB, FULL>), dim3((unsigned)((B + kGklBM - 1) / kGklBM)), dim3(256), rows_lds, st, mu, sigma,
                       m, L, c, G, B, K, D, dmu, dsigma);
    int rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const size_t comps_lds = ((size_t)Slot::SIZE + 2 * kGklBM * Slot::LD + kGklBM) * sizeof(float);
    hipLaunchKernelGGL((gkl_backward_comps_kernel<NB, FULL>), dim3((unsigned)K, (unsigned)gkl_splits(B)), dim3(256), comps_lds, st, mu,
                       sigma, m, L, c, G, B, K, D, ws);
    return launch_status();
}

#define GKL_DISPATCH(fn, ...)                                                                \
    (full ? (nb == 1   ? fn<1, true>(__VA_ARGS__)                                            \
             : nb == 2 ? fn<2, true>(__VA_ARGS__)                                            \
             : nb == 3 ? fn<3, true>(__VA_ARGS__)                                            \
                       : fn<4, true>(__VA_ARGS__))                                           \
          : (nb == 1   ? fn<1, false>(__VA_ARGS__)                                           \
             : nb == 2 ? fn<2, false>(__VA_ARGS__)                                           \
             : nb == 3 ? fn<3, false>(__VA_ARGS__)                                           \
                       : fn<4, false>(__VA_ARGS__)))

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_gkl_max_features(void) { return kGklMaxD; }

int32_t ptmi_gkl_row_tile(void) { return kGklBM; }

int32_t ptmi_gkl_split_rows(void) { return kGklSplitRows; }

int64_t ptmi_gkl_workspace_elems(int64_t B, int64_t K, int32_t D, int32_t full) {
    if (gkl_dims(B, K, D) != PTMI_OK) return 0;
    const int64_t dp = gkl_dp(D);
    return gkl_splits(B) * K * ((full ? dp * dp : 0) + 3 * dp);
}

int ptmi_gkl_prepare(const float* scale, int32_t full, int64_t K, int32_t D, float* L, float* c, float* logdet, ptmi_stream_t stream) {
    int rc = gkl_dims(1, K, D);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    PTMI_RETURN_IF(!scale || !c || !logdet || (full && !L), PTMI_E_INVALID);
    const int dp = gkl_dp(D);
    const size_t lds = full ? 2 * (size_t)dp * (dp + 1) * sizeof(float) : 0;
    hipLaunchKernelGGL(gkl_prepare_kernel, dim3((unsigned)K), dim3(256), lds, static_cast<hipStream_t>(stream), scale, (int)full, (int)D, dp,
                       L, c, logdet);
    return launch_status();
}

int ptmi_gkl_forward(const float* mu, const float* sigma, const float* m, const float* L, const float* c, const float* logdet, int32_t full,
                     int64_t B, int64_t K, int32_t D, float* kl, ptmi_stream_t stream) {
    int rc = gkl_dims(B, K, D);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    PTMI_RETURN_IF(!mu || !sigma || !m || !c || !logdet || !kl || (full && !L), PTMI_E_INVALID);
    const int nb = gkl_dp(D) / 16;
    return GKL_DISPATCH(gkl_launch_forward, mu, sigma, m, L, c, logdet, (int)B, (int)K, (int)D, kl, static_cast<hipStream_t>(stream));
}

int ptmi_gkl_backward(const float* mu, const float* sigma, const float* m, const float* scale, const float* L, const float* c,
                      const float* G, int32_t full, int64_t B, int64_t K, int32_t D, float* ws, float* dmu, float* dsigma, float* dm,
                      float* dscale, ptmi_stream_t stream) {
    int rc = gkl_dims(B, K, D);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    PTMI_RETURN_IF(!mu || !sigma || !m || !scale || !c || !G || !ws || !dmu || !dsigma || !dm || !dscale || (full && !L), PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int dp = gkl_dp(D), nb = dp / 16;
    rc = GKL_DISPATCH(gkl_launch_backward, mu, sigma, m, L, c, G, (int)B, (int)K, (int)D, ws, dmu, dsigma, st);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const size_t lds = (3 * (size_t)dp + (full ? 3 * (size_t)dp * (dp + 1) : 0)) * sizeof(float);
    hipLaunchKernelGGL(gkl_finish_kernel, dim3((unsigned)K), dim3(256), lds, st, ws, (int)gkl_splits(B), (int)K, (int)D, dp, (int)full, L,
                       scale, dm, dscale);
    return launch_status();
}

}  // extern "C"
