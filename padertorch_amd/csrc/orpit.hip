// One-and-Rest PIT (padertorch/contrib/examples/source_separation/or_pit/model.py): the loss of `review` (:319-350, through
// one_and_rest_permutation_invariant_loss :11-98 with pt.log_mse_loss) and the flag head (:187-218).
//
// The loss of one iteration pairs estimate row 0 with ONE alive target and row 1 with the SUM of the other alive targets.  Every
// candidate is a closed form of sums over time:  C[m][j] = sum e_m t_j,  See[m] = sum e_m^2  and the targets' Gram matrix
// G[j][l] = sum t_j t_l  (||e_1 - sum_{j in S} t_j||^2 = See_1 - 2 sum_{j in S} C[1][j] + sum_{j,l in S} G[j][l]).  So one streaming
// pass over the M + K rows of an example (rect_stats) serves all candidates, a one-thread-per-example kernel (select) takes the
// first minimum, updates the alive mask ON THE DEVICE and writes the coefficients of the gradient, and one more streaming pass
// (rect_lincomb) forms  d loss / d e_m = g (a_m e_m + sum_j bmat[m][j] t_j).  The Gram matrix does not depend on the estimates: it
// is computed in the first iteration of a step only.
//
// The flag head reads the separator's additional output [B, A, E] and, in the weighted modes, mask [K, B, N, E] and encoded
// [B, N, E] directly: mask * encoded (the reference's encoded_out) is never stored.
//
// Conventions of td_loss.hip / tasnet.hip: fp32 data, fp64 accumulation of exact products, no atomics, the order of addition inside a
// workgroup that reduce.h defines, per-workgroup partials in a caller-owned workspace of doubles added in ascending order by a second
// stage (bit-reproducible), no allocation and no synchronisation (capturable), float4 loads with a scalar path for rows that are not
// 16-byte aligned.
#include "reduce.h"

namespace ptmi {

constexpr int kRectMax = 8;

struct RectArgs {
    const float* est;
    const float* tgt;
    long long T;
    long long eb, em, tb, tk;   // strides in elements; time is contiguous
    long long chunk;            // samples per workgroup (multiple of 4)
    int M, K, nchunks, vec, gram;
    double* ws;                 // [B][nchunks][M K + M + K K]
};

// One workgroup per (chunk, example, group of ME estimate rows).  Workspace row: C[M][K] | See[M] | G[K][K]; the Gram matrix is
// accumulated as its upper triangle by the workgroups of the first row group and written out symmetric.
template <int ME, int K>
__global__ __launch_bounds__(256) void rect_stats_kernel(const RectArgs A) {
    constexpr int KK = K > 0 ? K : 1;
    constexpr int NG = K > 0 ? K * (K + 1) / 2 : 1;
    const int b = blockIdx.y, c = blockIdx.x, m0 = blockIdx.z * ME;
    const bool gram = A.gram && blockIdx.z == 0;
    const long long t0 = (long long)c * A.chunk;
    const long long t1 = min(t0 + A.chunk, A.T);
    double cc[ME][KK], see[ME], g[NG];
#pragma unroll
    for (int m = 0; m < ME; ++m) {
        see[m] = 0.0;
#pragma unroll
        for (int j = 0; j < KK; ++j) cc[m][j] = 0.0;
    }
#pragma unroll
    for (int s = 0; s < NG; ++s) g[s] = 0.0;
    const float* __restrict__ e = A.est + (long long)b * A.eb + (long long)m0 * A.em;
    const float* __restrict__ t = A.tgt + (long long)b * A.tb;
    auto add = [&](const float (&ev)[ME], const float (&tv)[KK]) {
        double td[KK];
#pragma unroll
        for (int j = 0; j < K; ++j) td[j] = (double)tv[j];
#pragma unroll
        for (int m = 0; m < ME; ++m) {
            const double ed = (double)ev[m];
            see[m] = fma(ed, ed, see[m]);
#pragma unroll
            for (int j = 0; j < K; ++j) cc[m][j] = fma(ed, td[j], cc[m][j]);
        }
        if (gram) {
            int s = 0;
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int l = j; l < K; ++l, ++s) g[s] = fma(td[j], td[l], g[s]);
        }
    };
    if (A.vec) {
        for (long long i = t0 + 4 * threadIdx.x; i < t1; i += 4 * 256) {
            if (i + 4 <= t1) {
                float4 ev4[ME], tv4[KK];
#pragma unroll
                for (int m = 0; m < ME; ++m) ev4[m] = *reinterpret_cast<const float4*>(e + m * A.em + i);
#pragma unroll
                for (int j = 0; j < K; ++j) tv4[j] = *reinterpret_cast<const float4*>(t + j * A.tk + i);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float ev[ME], tv[KK];
#pragma unroll
                    for (int m = 0; m < ME; ++m) ev[m] = reinterpret_cast<const float*>(&ev4[m])[q];
#pragma unroll
                    for (int j = 0; j < K; ++j) tv[j] = reinterpret_cast<const float*>(&tv4[j])[q];
                    add(ev, tv);
                }
            } else {   // the (< 4 sample) tail of the row when T % 4 != 0
                for (long long ii = i; ii < t1; ++ii) {
                    float ev[ME], tv[KK];
#pragma unroll
                    for (int m = 0; m < ME; ++m) ev[m] = e[m * A.em + ii];
#pragma unroll
                    for (int j = 0; j < K; ++j) tv[j] = t[j * A.tk + ii];
                    add(ev, tv);
                }
            }
        }
    } else {
        for (long long i = t0 + threadIdx.x; i < t1; i += 256) {
            float ev[ME], tv[KK];
#pragma unroll
            for (int m = 0; m < ME; ++m) ev[m] = e[m * A.em + i];
#pragma unroll
            for (int j = 0; j < K; ++j) tv[j] = t[j * A.tk + i];
            add(ev, tv);
        }
    }
    constexpr int NL = ME * K + ME + (K > 0 ? K * (K + 1) / 2 : 0);   // values this workgroup reduces
    __shared__ double red[4][NL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        int s = 0;
#pragma unroll
        for (int m = 0; m < ME; ++m)
#pragma unroll
            for (int j = 0; j < K; ++j, ++s) {
                const double v = wave_sum(cc[m][j]);
                if (lane == 0) red[wave][s] = v;
            }
#pragma unroll
        for (int m = 0; m < ME; ++m, ++s) {
            const double v = wave_sum(see[m]);
            if (lane == 0) red[wave][s] = v;
        }
        if (K > 0) {
#pragma unroll
            for (int x = 0; x < NG; ++x, ++s) {
                const double v = wave_sum(g[x]);
                if (lane == 0) red[wave][s] = v;
            }
        }
    }
    __syncthreads();
    const int M = A.M;
    double* w = A.ws + ((long long)b * A.nchunks + c) * ((long long)M * K + M + K * K);
    const int x = threadIdx.x;
    auto tot = [&](int s) { return ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s]; };
    if (x < ME * K) w[(m0 + x / KK) * K + x % KK] = tot(x);
    if (x < ME) w[M * K + m0 + x] = tot(ME * K + x);
    if (gram && x < K * K) {
        const int j = min(x / KK, x % KK), l = max(x / KK, x % KK);
        w[M * K + M + x] = tot(ME * K + ME + j * K - j * (j - 1) / 2 + (l - j));
    }
}

// out[b, s] = sum_c ws[b, c, s] in chunk order for s < NS of a workspace row of NW values.
__global__ void rect_reduce_kernel(const double* __restrict__ ws, double* __restrict__ stats, double* __restrict__ gram, int nchunks,
                                   int NS, int NG) {
    const int b = blockIdx.x, NW = NS + NG;
    for (int s = threadIdx.x; s < (gram ? NW : NS); s += blockDim.x) {
        double v = 0.0;
        for (int c = 0; c < nchunks; ++c) v += ws[((long long)b * nchunks + c) * NW + s];
        if (s < NS)
            stats[(long long)b * NS + s] = v;
        else
            gram[(long long)b * NG + (s - NS)] = v;
    }
}

template <int ME, int K>
static int launch_rect_stats(const RectArgs& A, long long batch, hipStream_t st) {
    hipLaunchKernelGGL((rect_stats_kernel<ME, K>), dim3((unsigned)A.nchunks, (unsigned)batch, (unsigned)(A.M / ME)), dim3(256), 0, st, A);
    return launch_status();
}

template <int ME>
static int dispatch_rect_stats(const RectArgs& A, long long batch, hipStream_t st) {
    switch (A.K) {
        case 0: return launch_rect_stats<ME, 0>(A, batch, st);
        case 1: return launch_rect_stats<ME, 1>(A, batch, st);
        case 2: return launch_rect_stats<ME, 2>(A, batch, st);
        case 3: return launch_rect_stats<ME, 3>(A, batch, st);
        case 4: return launch_rect_stats<ME, 4>(A, batch, st);
        case 5: return launch_rect_stats<ME, 5>(A, batch, st);
        case 6: return launch_rect_stats<ME, 6>(A, batch, st);
        case 7: return launch_rect_stats<ME, 7>(A, batch, st);
        default: return launch_rect_stats<ME, 8>(A, batch, st);
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------
// One thread per example; M = 2.  stats: C[2][K] | See[2], gram [K][K].
__global__ void orpit_select_kernel(const double* __restrict__ stats, const double* __restrict__ gram, const int32_t* __restrict__ alive_in,
                                    int32_t* __restrict__ alive_out, float* __restrict__ loss, int32_t* __restrict__ choice,
                                    float* __restrict__ coef_a, float* __restrict__ coef_b, double n, int B, int K) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* C = stats + (long long)b * (2 * K + 2);
    const double* G = gram + (long long)b * K * K;
    const double see0 = C[2 * K], see1 = C[2 * K + 1];
    const double ln10 = 2.302585092994045684;
    bool live[kRectMax];
    int R = 0;
    double row1 = 0.0, gall = 0.0;     // sum_{j alive} C[1][j], sum_{j, l alive} G[j][l]
    for (int j = 0; j < K; ++j) {
        live[j] = alive_in[(long long)b * K + j] != 0;
        R += live[j];
    }
    for (int j = 0; j < K; ++j) {
        if (!live[j]) continue;
        row1 += C[K + j];
        for (int l = 0; l < K; ++l)
            if (live[l]) gall += G[j * K + l];
    }
    int best = -1;
    double best_loss = 0.0, sse0 = see0, sse1 = see1, w1 = 1.0;
    if (R >= 2) {
        w1 = 1.0 / (R - 1);
        for (int i = 0; i < K; ++i) {
            if (!live[i]) continue;
            double gi = 0.0;            // sum_{l alive} G[i][l]
            for (int l = 0; l < K; ++l)
                if (live[l]) gi += G[i * K + l];
            const double s0 = see0 - 2.0 * C[i] + G[i * K + i];
            const double s1 = see1 - 2.0 * (row1 - C[K + i]) + (gall - 2.0 * gi + G[i * K + i]);
            const double cand = log10(s0 / n) + w1 * log10(s1 / n);
            // the first minimum wins; a NaN candidate wins over every number (torch.min)
            if (best < 0 || cand < best_loss || (cand != cand && best_loss == best_loss)) {
                best = i;
                best_loss = cand;
                sse0 = s0;
                sse1 = s1;
            }
        }
    } else if (R == 1) {
        for (int i = 0; i < K; ++i)
            if (live[i]) best = i;
        sse0 = see0 - 2.0 * C[best] + G[best * K + best];
        best_loss = log10(sse0 / n) + log10(see1 / n);
    } else {
        best_loss = log10(see0 / n) + log10(see1 / n);
    }
    loss[b] = (float)best_loss;
    choice[b] = best;
    const double a0 = 2.0 / (ln10 * sse0), a1 = 2.0 * w1 / (ln10 * sse1);
    coef_a[2 * b] = (float)a0;
    coef_a[2 * b + 1] = (float)a1;
    for (int j = 0; j < K; ++j) {
        coef_b[(2LL * b) * K + j] = j == best ? (float)-a0 : 0.f;
        coef_b[(2LL * b + 1) * K + j] = (R >= 2 && live[j] && j != best) ? (float)-a1 : 0.f;
        alive_out[(long long)b * K + j] = (live[j] && j != best) ? 1 : 0;
    }
}

// ---- gradient pass ----------------------------------------------------------------------------------------------------------------
struct RectLinArgs {
    const float* est;
    const float* tgt;
    const float* g;      // [B] or null (= 1)
    const float* A;      // [B][M]
    const float* Bc;     // [B][M][K]
    float* out;
    long long T;
    long long eb, em, tb, tk, ob, om;
    long long chunk;
    int M, vec;
};

// out[b, m, t] = g[b] (A[b,m] est[b,m,t] + sum_j Bc[b,m,j] tgt[b,j,t])
template <int ME, int K>
__global__ __launch_bounds__(256) void rect_lincomb_kernel(const RectLinArgs P) {
    constexpr int KK = K > 0 ? K : 1;
    const int b = blockIdx.y, m0 = blockIdx.z * ME;
    const long long t0 = (long long)blockIdx.x * P.chunk;
    const long long t1 = min(t0 + P.chunk, P.T);
    const float g = P.g ? P.g[b] : 1.f;
    float a[ME], bc[ME][KK];
#pragma unroll
    for (int m = 0; m < ME; ++m) {
        a[m] = g * P.A[(long long)b * P.M + m0 + m];
#pragma unroll
        for (int j = 0; j < K; ++j) bc[m][j] = g * P.Bc[((long long)b * P.M + m0 + m) * K + j];
    }
    const float* __restrict__ e = P.est + (long long)b * P.eb + (long long)m0 * P.em;
    const float* __restrict__ t = P.tgt + (long long)b * P.tb;
    float* __restrict__ o = P.out + (long long)b * P.ob + (long long)m0 * P.om;
    auto scalar = [&](long long x) {
        float tv[KK];
#pragma unroll
        for (int j = 0; j < K; ++j) tv[j] = t[j * P.tk + x];
#pragma unroll
        for (int m = 0; m < ME; ++m) {
            float v = a[m] * e[m * P.em + x];
#pragma unroll
            for (int j = 0; j < K; ++j) v = fmaf(bc[m][j], tv[j], v);
            o[m * P.om + x] = v;
        }
    };
    if (P.vec) {
        for (long long x = t0 + 4 * threadIdx.x; x + 4 <= t1; x += 4 * 256) {
            float4 tv[KK];
#pragma unroll
            for (int j = 0; j < K; ++j) tv[j] = *reinterpret_cast<const float4*>(t + j * P.tk + x);
#pragma unroll
            for (int m = 0; m < ME; ++m) {
                const float4 ev = *reinterpret_cast<const float4*>(e + m * P.em + x);
                float r[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = a[m] * reinterpret_cast<const float*>(&ev)[q];
#pragma unroll
                    for (int j = 0; j < K; ++j) v = fmaf(bc[m][j], reinterpret_cast<const float*>(&tv[j])[q], v);
                    r[q] = v;
                }
                *reinterpret_cast<float4*>(o + m * P.om + x) = make_float4(r[0], r[1], r[2], r[3]);
            }
        }
        const long long tail0 = t1 - ((t1 - t0) & 3);    // the (< 4 sample) tail of the row when T % 4 != 0
        if (threadIdx.x < t1 - tail0) scalar(tail0 + threadIdx.x);
    } else {
        for (long long x = t0 + threadIdx.x; x < t1; x += 256) scalar(x);
    }
}

template <int ME, int K>
static int launch_rect_lincomb(const RectLinArgs& P, long long batch, hipStream_t st) {
    const unsigned nchunks = (unsigned)((P.T + P.chunk - 1) / P.chunk);
    hipLaunchKernelGGL((rect_lincomb_kernel<ME, K>), dim3(nchunks, (unsigned)batch, (unsigned)(P.M / ME)), dim3(256), 0, st, P);
    return launch_status();
}

template <int ME>
static int dispatch_rect_lincomb(const RectLinArgs& P, int K, long long batch, hipStream_t st) {
    switch (K) {
        case 0: return launch_rect_lincomb<ME, 0>(P, batch, st);
        case 1: return launch_rect_lincomb<ME, 1>(P, batch, st);
        case 2: return launch_rect_lincomb<ME, 2>(P, batch, st);
        case 3: return launch_rect_lincomb<ME, 3>(P, batch, st);
        case 4: return launch_rect_lincomb<ME, 4>(P, batch, st);
        case 5: return launch_rect_lincomb<ME, 5>(P, batch, st);
        case 6: return launch_rect_lincomb<ME, 6>(P, batch, st);
        case 7: return launch_rect_lincomb<ME, 7>(P, batch, st);
        default: return launch_rect_lincomb<ME, 8>(P, batch, st);
    }
}

// ---- flag head ----------------------------------------------------------------------------------------------------------------------
struct FlagArgs {
    const float* additional;   // [B, A, E]
    const float* weight;       // [A]
    const float* bias;         // [1]
    const float* mask;         // [K, B, N, E] (weighted modes)
    const float* encoded;      // [B, N, E] or null
    float* pre;                // [B, E]
    float* w;                  // [B, E] (weighted modes)
    double* ws;
    long long B, E;
    int A, N, K, k, weighted, nblk;
};

// A workgroup is 64 lanes x 4 waves: a lane owns V consecutive frames, the waves share the rows (a, then n) among them and their
// partial sums are added in wave order.  pre and w are stored; the workgroup's partial (sum pre w, sum w) goes to the workspace.
template <int V>
__global__ __launch_bounds__(256) void flag_forward_kernel(const FlagArgs P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.y, e0 = ((long long)blockIdx.x * 64 + lane) * V;
    const bool live = e0 < P.E;           // (V == 4: E is a multiple of 4, a quad is live or dead as a whole)
    double accp[V], accw[V];
#pragma unroll
    for (int q = 0; q < V; ++q) accp[q] = accw[q] = 0.0;
    if (live) {
        for (int a = wave; a < P.A; a += 4) {
            float x[V];
            load_vec<V>(P.additional + (b * P.A + a) * P.E + e0, x);
            const double wa = (double)P.weight[a];
#pragma unroll
            for (int q = 0; q < V; ++q) accp[q] = fma(wa, (double)x[q], accp[q]);
        }
        if (P.weighted) {
            const float* m = P.mask + ((long long)P.k * P.B + b) * P.N * P.E + e0;
            const float* en = P.encoded ? P.encoded + b * P.N * P.E + e0 : nullptr;
            for (int n = wave; n < P.N; n += 4) {
                float mv[V], ev[V];
                load_vec<V>(m + (long long)n * P.E, mv);
                if (en) load_vec<V>(en + (long long)n * P.E, ev);
#pragma unroll
                for (int q = 0; q < V; ++q) {
                    const double p = en ? (double)mv[q] * (double)ev[q] : (double)mv[q];
                    accw[q] = fma(p, p, accw[q]);
                }
            }
        }
    }
    __shared__ double shp[4][64 * V], shw[4][64 * V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
        shp[wave][lane * V + q] = accp[q];
        shw[wave][lane * V + q] = accw[q];
    }
    __syncthreads();
    if (wave != 0) return;
    double num = 0.0, den = 0.0;
    if (live) {
        const double bias = (double)P.bias[0];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const int s = lane * V + q;
            const double pre = bias + (((shp[0][s] + shp[1][s]) + shp[2][s]) + shp[3][s]);
            const double w = P.weighted ? (((shw[0][s] + shw[1][s]) + shw[2][s]) + shw[3][s]) / P.N : 1.0;
            P.pre[b * P.E + e0 + q] = (float)pre;
            if (P.weighted) P.w[b * P.E + e0 + q] = (float)w;
            num += pre * w;
            den += w;
        }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    if (lane == 0) {
        double* o = P.ws + (b * P.nblk + blockIdx.x) * 2;
        o[0] = num;
        o[1] = den;
    }
}

// flag[b] = sigmoid(num / den), stat[b] = (num / den, den); the partials of a row in block order.
__global__ void flag_final_kernel(const double* __restrict__ ws, float* __restrict__ flag, double* __restrict__ stat, int B, int nblk) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double num = 0.0, den = 0.0;
    for (int c = 0; c < nblk; ++c) {
        num += ws[((long long)b * nblk + c) * 2];
        den += ws[((long long)b * nblk + c) * 2 + 1];
    }
    const double x = num / den;
    flag[b] = (float)(1.0 / (1.0 + exp(-x)));
    stat[2 * b] = x;
    stat[2 * b + 1] = den;
}

struct FlagBwdArgs {
    const float* gflag;        // [B]
    const float* gpre;         // [B, E] or null
    const float* flag;         // [B]
    const double* stat;        // [B, 2]
    const float* pre;          // [B, E]
    const float* w;            // [B, E] (weighted modes)
    const float* additional;
    const float* weight;
    const float* mask;
    const float* encoded;
    float* dadditional;        // [B, A, E]
    float* dmask;              // [K, B, N, E] (weighted modes)
    float* dencoded;           // [B, N, E] (weighted modes, encoded given)
    double* ws;                // [B][nblk][A + 1]
    long long B, E;
    int A, N, K, k, weighted, nblk;
};

template <int V>
__global__ __launch_bounds__(256) void flag_backward_kernel(const FlagBwdArgs P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.y, e0 = ((long long)blockIdx.x * 64 + lane) * V;
    const bool live = e0 < P.E;
    const double f = (double)P.flag[b], x = P.stat[2 * b], den = P.stat[2 * b + 1];
    const double gx = (double)P.gflag[b] * f * (1.0 - f);
    float dpre[V], dw[V];      // d / d pre[b, e], 2 / N * d / d w[b, e]
#pragma unroll
    for (int q = 0; q < V; ++q) dpre[q] = dw[q] = 0.f;
    if (live) {
        float pv[V], wv[V], gp[V];
        load_vec<V>(P.pre + b * P.E + e0, pv);
        if (P.weighted) load_vec<V>(P.w + b * P.E + e0, wv);
        if (P.gpre) load_vec<V>(P.gpre + b * P.E + e0, gp);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const double wq = P.weighted ? (double)wv[q] : 1.0;
            dpre[q] = (float)(gx * wq / den + (P.gpre ? (double)gp[q] : 0.0));
            dw[q] = P.weighted ? (float)(gx * ((double)pv[q] - x) / den * 2.0 / P.N) : 0.f;
        }
    }
    double* part = P.ws + (b * P.nblk + blockIdx.x) * (P.A + 1);
    for (int a = wave; a < P.A; a += 4) {       // every row a belongs to one wave: its partial needs no second wave
        double s = 0.0;
        if (live) {
            float xv[V], o[V];
            load_vec<V>(P.additional + (b * P.A + a) * P.E + e0, xv);
            const float wa = P.weight[a];
#pragma unroll
            for (int q = 0; q < V; ++q) {
                o[q] = wa * dpre[q];
                s = fma((double)xv[q], (double)dpre[q], s);
            }
            store_vec<V>(P.dadditional + (b * P.A + a) * P.E + e0, o);
        }
        s = wave_sum(s);
        if (lane == 0) part[a] = s;
    }
    if (wave == 0) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < V; ++q) s += (double)dpre[q];
        s = wave_sum(s);
        if (lane == 0) part[P.A] = s;
    }
    if (!P.weighted || !live) return;
    const long long slice = P.B * P.N * P.E, row = b * P.N * P.E + e0;
    float zero[V];
#pragma unroll
    for (int q = 0; q < V; ++q) zero[q] = 0.f;
    for (int n = wave; n < P.N; n += 4) {
        const long long at = row + (long long)n * P.E;
        float mv[V], ev[V], dm[V], de[V];
        load_vec<V>(P.mask + P.k * slice + at, mv);
        if (P.encoded) load_vec<V>(P.encoded + at, ev);
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const float en = P.encoded ? ev[q] : 1.f;
            dm[q] = dw[q] * mv[q] * en * en;
            de[q] = dw[q] * mv[q] * mv[q] * en;
        }
        for (int kk = 0; kk < P.K; ++kk) store_vec<V>(P.dmask + kk * slice + at, kk == P.k ? dm : zero);
        if (P.encoded) store_vec<V>(P.dencoded + at, de);
    }
}

// dparams[a] = sum over the partials in order (a < A: d weight, a == A: d bias).
__global__ void flag_params_kernel(const double* __restrict__ ws, float* __restrict__ dparams, long long nparts, int A) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a > A) return;
    double v = 0.0;
    for (long long c = 0; c < nparts; ++c) v += ws[c * (A + 1) + a];
    dparams[a] = (float)v;
}

static int flag_vec(long long E, std::initializer_list<const void*> ptrs) {
    return E % 4 == 0 && aligned16(ptrs);          // (an absent operand is a null pointer and counts as aligned)
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_td_rect_workspace_elems(int64_t batch, int32_t M, int32_t K, int64_t T) {
    if (batch < 1 || M < 1 || K < 0 || T < 1) return PTMI_E_INVALID;
    const long long chunk = pick_chunk(batch, T);
    return batch * ((T + chunk - 1) / chunk) * ((int64_t)M * K + M + (int64_t)K * K);
}

int ptmi_td_rect_stats(const float* est, const float* tgt, int64_t batch, int32_t M, int32_t K, int64_t T, const int64_t* strides,
                       double* workspace, double* stats, double* gram, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!est || (!tgt && K > 0) || !strides || !workspace || !stats, PTMI_E_INVALID);
    PTMI_RETURN_IF(batch < 1 || M < 1 || K < 0 || T < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(M > kRectMax || K > kRectMax || batch > 65535, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    RectArgs A{};
    A.est = est;
    A.tgt = tgt;
    A.T = T;
    A.eb = strides[0];
    A.em = strides[1];
    A.tb = strides[2];
    A.tk = strides[3];
    A.chunk = pick_chunk(batch, T);
    A.M = M;
    A.K = K;
    A.nchunks = (int)((T + A.chunk - 1) / A.chunk);
    A.gram = gram != nullptr && K > 0;
    A.vec = T >= 4 && aligned16({est}) && (K == 0 || aligned16({tgt})) && A.eb % 4 == 0 && A.em % 4 == 0 &&
            (K == 0 || (A.tb % 4 == 0 && A.tk % 4 == 0));
    A.ws = workspace;
    int rc = M % 2 == 0 ? dispatch_rect_stats<2>(A, batch, st) : dispatch_rect_stats<1>(A, batch, st);
    if (rc) return rc;
    hipLaunchKernelGGL(rect_reduce_kernel, dim3((unsigned)batch), dim3(64), 0, st, workspace, stats, A.gram ? gram : nullptr, A.nchunks,
                       M * K + M, K * K);
    return launch_status();
}

int ptmi_orpit_select(const double* stats, const double* gram, const int32_t* alive_in, int32_t* alive_out, float* loss,
                      int32_t* choice, float* coef_a, float* coef_b, int64_t batch, int32_t K, int64_t n, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!stats || !loss || !choice || !coef_a, PTMI_E_INVALID);
    PTMI_RETURN_IF(K > 0 && (!gram || !alive_in || !alive_out || !coef_b), PTMI_E_INVALID);
    PTMI_RETURN_IF(batch < 1 || K < 0 || n < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(K > kRectMax || batch > 65535, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(orpit_select_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), stats,
                       gram, alive_in, alive_out, loss, choice, coef_a, coef_b, (double)n, (int)batch, K);
    return launch_status();
}

int ptmi_td_rect_lincomb(const float* est, const float* tgt, const float* g, const float* coef_a, const float* coef_b, int64_t batch,
                         int32_t M, int32_t K, int64_t T, const int64_t* strides, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!est || (K > 0 && (!tgt || !coef_b)) || !coef_a || !strides || !out, PTMI_E_INVALID);
    PTMI_RETURN_IF(batch < 1 || M < 1 || K < 0 || T < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(M > kRectMax || K > kRectMax || batch > 65535, PTMI_E_UNSUPPORTED);
    RectLinArgs P{};
    P.est = est;
    P.tgt = tgt;
    P.g = g;
    P.A = coef_a;
    P.Bc = coef_b;
    P.out = out;
    P.T = T;
    P.eb = strides[0];
    P.em = strides[1];
    P.tb = strides[2];
    P.tk = strides[3];
    P.ob = strides[4];
    P.om = strides[5];
    P.chunk = pick_chunk(batch, T);
    P.M = M;
    P.vec = aligned16({est, out}) && (K == 0 || aligned16({tgt})) && P.eb % 4 == 0 && P.em % 4 == 0 &&
            P.ob % 4 == 0 && P.om % 4 == 0 && (K == 0 || (P.tb % 4 == 0 && P.tk % 4 == 0));
    hipStream_t st = static_cast<hipStream_t>(stream);
    return M % 2 == 0 ? dispatch_rect_lincomb<2>(P, K, batch, st) : dispatch_rect_lincomb<1>(P, K, batch, st);
}

int64_t ptmi_orpit_flag_workspace_elems(int64_t B, int32_t A, int64_t E) {
    if (B < 1 || A < 1 || E < 1) return PTMI_E_INVALID;
    return B * ((E + 63) / 64) * ((int64_t)A + 2);     // enough for either direction and either vector width
}

int ptmi_orpit_flag_forward(const float* additional, const float* weight, const float* bias, const float* mask, const float* encoded,
                            float* pre, float* w, float* flag, double* stat, double* workspace, int64_t B, int32_t A, int64_t E,
                            int32_t N, int32_t K, int32_t k, int32_t weighted, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!additional || !weight || !bias || !pre || !flag || !stat || !workspace, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || A < 1 || E < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(weighted && (!mask || !w || N < 1 || K < 1 || k < 0 || k >= K), PTMI_E_INVALID);
    PTMI_RETURN_IF(B > 65535, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FlagArgs P{};
    P.additional = additional;
    P.weight = weight;
    P.bias = bias;
    P.mask = weighted ? mask : nullptr;
    P.encoded = weighted ? encoded : nullptr;
    P.pre = pre;
    P.w = w;
    P.ws = workspace;
    P.B = B;
    P.E = E;
    P.A = A;
    P.N = N;
    P.K = K;
    P.k = k;
    P.weighted = weighted != 0;
    const int vec = flag_vec(E, {additional, pre, P.mask, P.encoded, weighted ? w : nullptr});
    P.nblk = (int)((E + 64 * (vec ? 4 : 1) - 1) / (64 * (vec ? 4 : 1)));
    const dim3 grid((unsigned)P.nblk, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(flag_forward_kernel<4>, grid, dim3(256), 0, st, P);
    else
        hipLaunchKernelGGL(flag_forward_kernel<1>, grid, dim3(256), 0, st, P);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(flag_final_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, workspace, flag, stat, (int)B, P.nblk);
    return launch_status();
}

int ptmi_orpit_flag_backward(const float* gflag, const float* gpre, const float* flag, const double* stat, const float* pre, const float* w,
                             const float* additional, const float* weight, const float* mask, const float* encoded, float* dadditional,
                             float* dparams, float* dmask, float* dencoded, double* workspace, int64_t B, int32_t A, int64_t E, int32_t N,
                             int32_t K, int32_t k, int32_t weighted, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gflag || !flag || !stat || !pre || !additional || !weight || !dadditional || !dparams || !workspace, PTMI_E_INVALID);
    PTMI_RETURN_IF(B < 1 || A < 1 || E < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(weighted && (!mask || !w || !dmask || (encoded && !dencoded) || N < 1 || K < 1 || k < 0 || k >= K), PTMI_E_INVALID);
    PTMI_RETURN_IF(B > 65535, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    FlagBwdArgs P{};
    P.gflag = gflag;
    P.gpre = gpre;
    P.flag = flag;
    P.stat = stat;
    P.pre = pre;
    P.w = w;
    P.additional = additional;
    P.weight = weight;
    P.mask = weighted ? mask : nullptr;
    P.encoded = weighted ? encoded : nullptr;
    P.dadditional = dadditional;
    P.dmask = dmask;
    P.dencoded = dencoded;
    P.ws = workspace;
    P.B = B;
    P.E = E;
    P.A = A;
    P.N = N;
    P.K = K;
    P.k = k;
    P.weighted = weighted != 0;
    const int vec = flag_vec(E, {gpre, pre, weighted ? w : nullptr, additional, P.mask, P.encoded, dadditional, weighted ? dmask : nullptr,
                                 P.encoded ? dencoded : nullptr});
    P.nblk = (int)((E + 64 * (vec ? 4 : 1) - 1) / (64 * (vec ? 4 : 1)));
    const dim3 grid((unsigned)P.nblk, (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(flag_backward_kernel<4>, grid, dim3(256), 0, st, P);
    else
        hipLaunchKernelGGL(flag_backward_kernel<1>, grid, dim3(256), 0, st, P);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(flag_params_kernel, dim3((unsigned)((A + 1 + 63) / 64)), dim3(64), 0, st, workspace, dparams, (long long)B * P.nblk, A);
    return launch_status();
}

}  // extern "C"
