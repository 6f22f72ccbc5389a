// BigVGAN's anti-aliased periodic activation (Activation1d) for gfx950, forward and backward, in one pass over HBM.
//
// Replaces padertorch/contrib/mk/synthesis/vocoder/nvidia_bigvgan/alias_free_activation/torch/{resample,filter,act}.py with
// activations.py (Snake, SnakeBeta): ~a dozen passes over a signal of doubled length there.  Per row x[0..T) (rows = B * C, channel =
// row % C, fp32, time contiguous):
//   up     u[n] = r sum_j xp[j] f[n + pl - j r],  xp[j] = x[clamp(j - p, 0, T-1)], j in [0, T + 2p),  n in [0, U = r T)
//          p = k / r - 1,  pl = p r + (k - r) / 2                                  (a transposed convolution of stride r)
//   act    a(u) = u + sin^2(alpha' u) / (beta' + 1e-9),  alpha' = alpha or exp(alpha)
//   down   y[m] = sum_i g[i] a[clamp(m d + i - left, 0, U-1)],  m in [0, M)
// Three switches: a null up filter / a null down filter turn the stage into the identity (ratio 1, one tap of 1.0f - exact), act = 0
// makes a(u) = u.  So the same two kernels serve Activation1d, UpSample1d, DownSample1d / LowPassFilter1d and a lone Snake.
//
// Tiling (DESIGN.md "Anti-aliased activation").  Forward: a workgroup owns `tile` outputs of one row, stages the x samples they depend on
// (zero where the transposed convolution has no input), computes a(u) for the (tile - 1) d + dk points under them ONCE into LDS - the
// sine is the cost, so no point is evaluated twice inside a tile - and then runs the down filter out of LDS.  Backward: a workgroup owns
// `tile` samples of dx, stages x and dy, recomputes u, forms du = (dL/da) a'(u) in LDS and gathers dx from it.  Every sum is a gather:
// no atomics.  The clamps are handled by writing the sums over the UNCLAMPED index (n' in the padded a, j in the padded x) and letting
// the edge samples n = 0, U-1 and t = 0, T-1 add up all the unclamped indices that map onto them.
// Parameter gradients: the workgroup that owns dx[t0, t0 + tile) owns the points n in [r t0, r (t0 + tile)) - a partition of [0, U) - and
// leaves its two fp64 sums at ws[(row * tiles + tile) * 2]; aa_param_finish_kernel adds them per channel in a fixed order (reduce.h).
//
// The default hyper-parameters (ratios 2 / 2, 12 / 12 taps, padded) are a compile-time specialisation (AaCfg<true>); everything else the
// reference constructors accept, up to kAaMaxTaps taps and ratio kAaMaxRatio, runs through the same code with run-time values.
#include <algorithm>

#include "common.h"
#include "reduce.h"

namespace ptmi {

constexpr int kAaMaxTaps = 64;
constexpr int kAaMaxRatio = 8;

template <bool DEF>
struct AaCfg;

template <>
struct AaCfg<true> {
    static constexpr int kTile = 1024;                                   // outputs (forward) / dx samples (backward) per workgroup
    static constexpr int kR = 2, kK = 12, kD = 2, kDk = 12;
    static constexpr int kPmax = kK / kR - 1;
};

template <>
struct AaCfg<false> {
    static constexpr int kTile = 256;
    static constexpr int kR = kAaMaxRatio, kK = kAaMaxTaps, kD = kAaMaxRatio, kDk = kAaMaxTaps;
    static constexpr int kPmax = kAaMaxTaps - 1;                         // ratio 1, 64 taps
};

// LDS capacities (floats), from the worst case of the index ranges below (r = 1 maximises the x range, d = 1 the dy range)
template <bool DEF>
struct AaCaps {
    using C = AaCfg<DEF>;
    static constexpr int kMinR = DEF ? 2 : 1;
    // forward
    static constexpr int kFwdA = (C::kTile - 1) * C::kD + C::kDk;
    static constexpr int kFwdX = (kFwdA - 1 + C::kK - 1) / kMinR + 2;
    // backward
    static constexpr int kBwdU = (C::kTile + 2 * C::kPmax - 1) * C::kR + C::kK;
    static constexpr int kBwdX = (kBwdU - 1 + C::kK - 1) / kMinR + 2;
    static constexpr int kBwdDy = (kBwdU + 2 * C::kDk) / kMinR + 2;
};

struct AaGeom {
    int T, U, M, C;            // row lengths: input, up-sampled, output; channels
    int r, k, p, pl;           // up stage
    int d, dk, left;           // down stage
    int tiles;                 // workgroups per row
    int act, logscale;
};

__host__ __device__ __forceinline__ int aa_floordiv(int a, int b) {
    const int q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

__host__ __device__ __forceinline__ int aa_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool DEF>
struct AaView {                // the geometry with the default's values folded in at compile time
    int T, U, M, r, k, p, pl, d, dk, left;
    __device__ __forceinline__ explicit AaView(const AaGeom& G) {
        T = G.T, U = G.U, M = G.M;
        if constexpr (DEF) {
            r = 2, k = 12, p = 5, pl = 15, d = 2, dk = 12, left = 5;
        } else {
            r = G.r, k = G.k, p = G.p, pl = G.pl, d = G.d, dk = G.dk, left = G.left;
        }
    }
};

struct AaParams {
    float alpha, inv;          // alpha', 1 / (beta' + 1e-9)
};

// The channel's parameters, computed by ONE thread and handed on through LDS (the caller's next __syncthreads publishes them).  The
// log-scale exponential is taken in fp64 and rounded once, so alpha' and beta' are the correctly rounded values (expf may be 1 ulp
// off, and beta' enters d beta three times: 1 / beta'^2, times beta'); one thread per workgroup pays for it.
__device__ __forceinline__ void aa_stage_params(const AaGeom& G, const float* __restrict__ alpha, const float* __restrict__ beta, int c,
                                                AaParams* __restrict__ sp) {
    if (threadIdx.x != 0) return;
    AaParams P{0.f, 0.f};
    if (G.act) {
        float a = alpha[c], b = beta[c];
        if (G.logscale) a = (float)exp((double)a), b = (float)exp((double)b);
        P.alpha = a;
        P.inv = 1.0f / (b + 1e-9f);
    }
    *sp = P;
}

// sin and cos of an fp32 argument of any size.  The sine decides this kernel's cost (two points per output), so up to |a| = 1e5 it is a
// three-constant Cody-Waite reduction by pi / 2 with FMAs and two degree-4 polynomials in r^2 on [-pi/4, pi/4]: about 25 VALU
// instructions against ~140 for the library's sinf, at most 1.52 ulp (7.2e-8 absolute) from the exact value on |a| < 1e5 (checked on
// the host against long double; the library documents 2 ulp).  Beyond that - and for infinities - the library's Payne-Hanek path runs.
__device__ __forceinline__ void aa_sincos(float a, float& sn, float& cs) {
    if (fabsf(a) > 1e5f) {
        sincosf(a, &sn, &cs);
        return;
    }
    const float k = rintf(a * 0.636619747f);
    float r = fmaf(k, -1.57079601e+00f, a);
    r = fmaf(k, -3.13916473e-07f, r);
    r = fmaf(k, -5.39030253e-15f, r);
    const int q = (int)k;
    const float s = r * r;
    float c = 2.44677067e-5f;
    c = fmaf(c, s, -1.38877297e-3f);
    c = fmaf(c, s, 4.16666567e-2f);
    c = fmaf(c, s, -5.00000000e-1f);
    c = fmaf(c, s, 1.0f);
    float p = 2.86567956e-6f;
    p = fmaf(p, s, -1.98559923e-4f);
    p = fmaf(p, s, 8.33338592e-3f);
    p = fmaf(p, s, -1.66666672e-1f);
    p = fmaf(p, r * s, r);
    sn = (q & 1) ? c : p;
    cs = (q & 1) ? p : c;
    if (q & 2) sn = -sn;
    if ((q + 1) & 2) cs = -cs;
}

// taps into LDS; an absent stage is one tap of 1
__device__ __forceinline__ void aa_stage_taps(const float* __restrict__ f, int k, float* __restrict__ fs) {
    if ((int)threadIdx.x < k) fs[threadIdx.x] = f ? f[threadIdx.x] : 1.f;
}

// xs[i] = xp[jlo + i] (0 outside [0, T + 2p): the transposed convolution has no input there)
template <bool DEF>
__device__ __forceinline__ void aa_stage_x(const AaView<DEF>& V, const float* __restrict__ xrow, int jlo, int nx, float* __restrict__ xs) {
    for (int i = threadIdx.x; i < nx; i += 256) {
        const int j = jlo + i;
        xs[i] = (j < 0 || j >= V.T + 2 * V.p) ? 0.f : xrow[aa_clamp(j - V.p, 0, V.T - 1)];
    }
}

// u[n], 0 <= n < U, from the staged x: the taps of phase (n + pl) mod r, newest input first
template <bool DEF>
__device__ __forceinline__ float aa_upsample_at(const AaView<DEF>& V, int n, const float* __restrict__ fs, const float* __restrict__ xs,
                                                int jlo) {
    const int s = n + V.pl, q = s / V.r, ph = s - q * V.r;
    float acc = 0.f;
    if constexpr (DEF) {
#pragma unroll
        for (int t = 0; t < 6; ++t) acc = fmaf(fs[ph + t * 2], xs[q - t - jlo], acc);
    } else {
        for (int t = 0, tap = ph; tap < V.k; ++t, tap += V.r) acc = fmaf(fs[tap], xs[q - t - jlo], acc);
    }
    return (float)V.r * acc;
}

template <bool DEF, int VEC>
__global__ __launch_bounds__(256) void aa_forward_kernel(const float* __restrict__ x, const float* __restrict__ up_taps,
                                                         const float* __restrict__ down_taps, const float* __restrict__ alpha,
                                                         const float* __restrict__ beta, float* __restrict__ y, const AaGeom G) {
    using Caps = AaCaps<DEF>;
    constexpr int kTile = AaCfg<DEF>::kTile, kPer = kTile / 256;
    __shared__ float fs[kAaMaxTaps], gs[kAaMaxTaps];
    __shared__ AaParams sparams;
    __shared__ __align__(16) float xs[Caps::kFwdX];
    __shared__ __align__(16) float as[Caps::kFwdA];
    const AaView<DEF> V(G);
    const long long row = blockIdx.x / G.tiles;
    const int tile = (int)(blockIdx.x - row * G.tiles);
    const int m0 = tile * kTile, mcount = min(kTile, V.M - m0);
    const int nb = m0 * V.d - V.left, na = (mcount - 1) * V.d + V.dk;           // a[clamp(nb + i)], i < na, lies under this tile
    const int nlo = aa_clamp(nb, 0, V.U - 1), nhi = aa_clamp(nb + na - 1, 0, V.U - 1);
    const int jlo = aa_floordiv(nlo + V.pl - (V.k - 1), V.r), jhi = (nhi + V.pl) / V.r;
    aa_stage_taps(up_taps, V.k, fs);
    aa_stage_taps(down_taps, V.dk, gs);
    aa_stage_x(V, x + row * V.T, jlo, jhi - jlo + 1, xs);
    aa_stage_params(G, alpha, beta, (int)(row % G.C), &sparams);
    __syncthreads();
    const AaParams P = sparams;
    for (int i = threadIdx.x; i < na; i += 256) {
        const float u = aa_upsample_at(V, aa_clamp(nb + i, 0, V.U - 1), fs, xs, jlo);
        float a = u;
        if (G.act) {
            float s, c;
            aa_sincos(u * P.alpha, s, c);
            a = u + P.inv * (s * s);
        }
        as[i] = a;
    }
    __syncthreads();
    float* __restrict__ yrow = y + row * V.M;
    float out[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int mm = VEC == 4 ? (int)threadIdx.x * 4 + e : (int)threadIdx.x + 256 * e;
        float acc = 0.f;
        if (mm < mcount) {
            const float* __restrict__ ap = as + mm * V.d;
            if constexpr (DEF) {
#pragma unroll
                for (int i = 0; i < 12; ++i) acc = fmaf(gs[i], ap[i], acc);
            } else {
                for (int i = 0; i < V.dk; ++i) acc = fmaf(gs[i], ap[i], acc);
            }
        }
        out[e] = acc;
    }
    if constexpr (VEC == 4) {              // M % 4 == 0: a group of four outputs lies inside the row or outside it as a whole
        if ((int)threadIdx.x * 4 < mcount) *reinterpret_cast<float4*>(yrow + m0 + threadIdx.x * 4) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int mm = (int)threadIdx.x + 256 * e;
            if (mm < mcount) yrow[m0 + mm] = out[e];
        }
    }
}

// dL/da'[n'] on the padded (unclamped) index n' in [-left, (M-1) d + dk - 1 - left]: sum_m g[n' + left - m d] dy[m]; dys[i] = dy[mlo + i],
// 0 outside [0, M)
template <bool DEF>
__device__ __forceinline__ float aa_down_adjoint_at(const AaView<DEF>& V, int np, const float* __restrict__ gs,
                                                    const float* __restrict__ dys, int mlo) {
    const int s = np + V.left, q = s / V.d, ph = s - q * V.d;                   // s >= 0
    float acc = 0.f;
    if constexpr (DEF) {
#pragma unroll
        for (int t = 0; t < 6; ++t) acc = fmaf(gs[ph + t * 2], dys[q - t - mlo], acc);
    } else {
        for (int t = 0, tap = ph; tap < V.dk; ++t, tap += V.d) acc = fmaf(gs[tap], dys[q - t - mlo], acc);
    }
    return acc;
}

template <bool DEF, int VEC>
__global__ __launch_bounds__(256) void aa_backward_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ up_taps, const float* __restrict__ down_taps,
                                                          const float* __restrict__ alpha, const float* __restrict__ beta,
                                                          float* __restrict__ dx, double* __restrict__ ws, const AaGeom G) {
    using Caps = AaCaps<DEF>;
    constexpr int kTile = AaCfg<DEF>::kTile, kPer = kTile / 256;
    __shared__ float fs[kAaMaxTaps], gs[kAaMaxTaps];
    __shared__ AaParams sparams;
    __shared__ __align__(16) float xs[Caps::kBwdX];
    __shared__ __align__(16) float dys[Caps::kBwdDy];
    __shared__ __align__(16) float dus[Caps::kBwdU];
    const AaView<DEF> V(G);
    const long long row = blockIdx.x / G.tiles;
    const int tile = (int)(blockIdx.x - row * G.tiles);
    const int t0 = tile * kTile, tcount = min(kTile, V.T - t0);
    // padded-x indices j whose gradient lands in this tile, and the points n they touch (dus[i] = du[nb + i], 0 outside [0, U))
    const int jlo_d = t0 == 0 ? 0 : t0 + V.p, jhi_d = t0 + tcount == V.T ? V.T - 1 + 2 * V.p : t0 + tcount - 1 + V.p;
    const int nb = jlo_d * V.r - V.pl, nu = (jhi_d - jlo_d) * V.r + V.k;
    const int nlo = max(nb, 0), nhi = min(nb + nu - 1, V.U - 1);
    const int jlo = aa_floordiv(nlo + V.pl - (V.k - 1), V.r), jhi = (nhi + V.pl) / V.r;
    // padded-a indices n' under [nlo, nhi] (the edge points collect their whole pad) and the dy they read
    const int pend = max(V.U - 1, (V.M - 1) * V.d + V.dk - 1 - V.left);
    const int nplo = nlo == 0 ? -V.left : nlo, nphi = nhi == V.U - 1 ? pend : nhi;
    const int mlo = aa_floordiv(nplo + V.left - (V.dk - 1), V.d), mhi = (nphi + V.left) / V.d;
    aa_stage_taps(up_taps, V.k, fs);
    aa_stage_taps(down_taps, V.dk, gs);
    aa_stage_x(V, x + row * V.T, jlo, jhi - jlo + 1, xs);
    {
        const float* __restrict__ dyrow = dy + row * V.M;
        for (int i = threadIdx.x; i < mhi - mlo + 1; i += 256) {
            const int m = mlo + i;
            dys[i] = (m < 0 || m >= V.M) ? 0.f : dyrow[m];
        }
    }
    aa_stage_params(G, alpha, beta, (int)(row % G.C), &sparams);
    __syncthreads();
    const AaParams P = sparams;
    const int own_lo = t0 * V.r, own_hi = (t0 + tcount) * V.r;                 // points whose parameter gradient this workgroup owns
    double sums[2] = {0., 0.};
    for (int i = threadIdx.x; i < nu; i += 256) {
        const int n = nb + i;
        float du = 0.f;
        if (n >= 0 && n < V.U) {
            const float u = aa_upsample_at(V, n, fs, xs, jlo);
            const int a = n == 0 ? -V.left : n, b = n == V.U - 1 ? pend : n;
            float da = 0.f;
            for (int np = a; np <= b; ++np) da += aa_down_adjoint_at(V, np, gs, dys, mlo);
            du = da;
            if (G.act) {
                float s, c;
                aa_sincos(u * P.alpha, s, c);
                const float s2 = 2.f * s * c;                                   // sin 2 theta
                du = da * (1.f + P.alpha * P.inv * s2);
                if (ws && n >= own_lo && n < own_hi) {
                    sums[0] += (double)(da * (u * s2 * P.inv));
                    sums[1] -= (double)(da * ((s * P.inv) * (s * P.inv)));
                }
            }
        }
        dus[i] = du;
    }
    if (ws) {                                                                   // uniform over the launch
        block_sums(sums);
        if (threadIdx.x == 0) {
            ws[2 * (long long)blockIdx.x] = sums[0];
            ws[2 * (long long)blockIdx.x + 1] = sums[1];
        }
    }
    __syncthreads();
    float* __restrict__ dxrow = dx + row * V.T;
    float out[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int tt = VEC == 4 ? (int)threadIdx.x * 4 + e : (int)threadIdx.x + 256 * e;
        float acc = 0.f;
        if (tt < tcount) {
            const int t = t0 + tt;
            const int ja = t == 0 ? 0 : t + V.p, jb = t == V.T - 1 ? V.T - 1 + 2 * V.p : t + V.p;
            for (int j = ja; j <= jb; ++j) {
                const float* __restrict__ dp = dus + (j * V.r - V.pl - nb);
                if constexpr (DEF) {
#pragma unroll
                    for (int i = 0; i < 12; ++i) acc = fmaf(fs[i], dp[i], acc);
                } else {
                    for (int i = 0; i < V.k; ++i) acc = fmaf(fs[i], dp[i], acc);
                }
            }
        }
        out[e] = (float)V.r * acc;
    }
    if constexpr (VEC == 4) {
        if ((int)threadIdx.x * 4 < tcount) *reinterpret_cast<float4*>(dxrow + t0 + threadIdx.x * 4) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int tt = (int)threadIdx.x + 256 * e;
            if (tt < tcount) dxrow[t0 + tt] = out[e];
        }
    }
}

// Channel c's parameter gradients: the partials of its B * tiles workgroups, lanes ascending then block_sums (one fixed order), times the
// log-scale factor; a shared parameter (Snake: dbeta == null) receives both sums.  Grid: C workgroups.
__global__ __launch_bounds__(256) void aa_param_finish_kernel(const double* __restrict__ ws, long long B, int C, int tiles,
                                                              const float* __restrict__ alpha, const float* __restrict__ beta,
                                                              int logscale, float* __restrict__ dalpha, float* __restrict__ dbeta) {
    const int c = blockIdx.x;
    double s[2] = {0., 0.};
    for (long long i = threadIdx.x; i < B * tiles; i += 256) {
        const long long b = i / tiles, tl = i - b * tiles;
        const double* __restrict__ p = ws + 2 * ((b * C + c) * tiles + tl);
        s[0] += p[0];
        s[1] += p[1];
    }
    block_sums(s);
    if (threadIdx.x == 0) {
        if (logscale) {
            s[0] *= exp((double)alpha[c]);
            s[1] *= exp((double)beta[c]);
        }
        if (dbeta) {
            dalpha[c] = (float)s[0];
            dbeta[c] = (float)s[1];
        } else {
            dalpha[c] = (float)(s[0] + s[1]);
        }
    }
}

// Validates the hyper-parameters and fills the geometry; `by_input`: tiles over T (backward) instead of M (forward).
static int aa_geom(int64_t B, int32_t C, int64_t T, bool up, int32_t r, int32_t k, bool down, int32_t d, int32_t dk, int32_t padding,
                   int32_t act, int32_t logscale, bool by_input, AaGeom* G, bool* def) {
    if (!up) r = 1, k = 1;
    if (!down) d = 1, dk = 1, padding = 1;
    PTMI_RETURN_IF(B < 0 || C <= 0 || T < 0, PTMI_E_INVALID);
    PTMI_RETURN_IF(r < 1 || r > kAaMaxRatio || d < 1 || d > kAaMaxRatio || k < r || k > kAaMaxTaps || dk < 1 || dk > kAaMaxTaps,
                   PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(T * r >= (1ll << 30), PTMI_E_UNSUPPORTED);
    G->T = (int)T, G->U = (int)(T * r), G->C = C;
    G->r = r, G->k = k, G->p = k / r - 1, G->pl = G->p * r + (k - r) / 2;
    G->d = d, G->dk = dk, G->left = padding ? dk / 2 - (dk % 2 == 0 ? 1 : 0) : 0;
    if (T == 0)
        G->M = 0;
    else if (padding)
        G->M = (G->U + d - 1) / d;
    else
        G->M = G->U >= dk ? (G->U - dk) / d + 1 : 0;
    G->act = act ? 1 : 0, G->logscale = logscale ? 1 : 0;
    *def = up && down && padding && r == 2 && k == 12 && d == 2 && dk == 12;
    const int tile = *def ? AaCfg<true>::kTile : AaCfg<false>::kTile;
    const long long len = by_input ? G->T : G->M;
    G->tiles = (int)((len + tile - 1) / tile);
    PTMI_RETURN_IF(B * C * (long long)G->tiles >= (1ll << 31), PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_anti_alias_tile(int32_t default_geometry) { return default_geometry ? AaCfg<true>::kTile : AaCfg<false>::kTile; }

int64_t ptmi_anti_alias_out_len(int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio, int32_t down_taps, int32_t padding) {
    AaGeom G;
    bool def;
    if (aa_geom(1, 1, T, up_taps > 0, up_ratio, up_taps, down_taps > 0, down_ratio, down_taps, padding, 0, 0, false, &G, &def) != PTMI_OK)
        return -1;
    return G.M;
}

int64_t ptmi_anti_alias_workspace_elems(int64_t B, int32_t C, int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio,
                                        int32_t down_taps, int32_t padding) {
    AaGeom G;
    bool def;
    if (aa_geom(B, C, T, up_taps > 0, up_ratio, up_taps, down_taps > 0, down_ratio, down_taps, padding, 0, 0, true, &G, &def) != PTMI_OK)
        return -1;
    return std::max<int64_t>(2 * B * C * G.tiles, 1);
}

int ptmi_anti_alias_forward(const float* x, const float* up_filter, const float* down_filter, const float* alpha, const float* beta,
                            int64_t B, int32_t C, int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio, int32_t down_taps,
                            int32_t padding, int32_t act, int32_t logscale, float* y, ptmi_stream_t stream) {
    AaGeom G;
    bool def;
    PTMI_RETURN_IF(!x || !y || (act && (!alpha || !beta)), PTMI_E_INVALID);
    const int rc = aa_geom(B, C, T, up_filter != nullptr, up_ratio, up_taps, down_filter != nullptr, down_ratio, down_taps, padding, act,
                           logscale, false, &G, &def);
    if (rc != PTMI_OK) return rc;
    if (B == 0 || G.M == 0) return PTMI_OK;
    const dim3 grid((unsigned)(B * C * G.tiles));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (def) {
        const bool vec = G.M % 4 == 0 && aligned16({y});
        if (vec)
            hipLaunchKernelGGL((aa_forward_kernel<true, 4>), grid, dim3(256), 0, st, x, up_filter, down_filter, alpha, beta, y, G);
        else
            hipLaunchKernelGGL((aa_forward_kernel<true, 1>), grid, dim3(256), 0, st, x, up_filter, down_filter, alpha, beta, y, G);
    } else {
        hipLaunchKernelGGL((aa_forward_kernel<false, 1>), grid, dim3(256), 0, st, x, up_filter, down_filter, alpha, beta, y, G);
    }
    return launch_status();
}

int ptmi_anti_alias_backward(const float* dy, const float* x, const float* up_filter, const float* down_filter, const float* alpha,
                             const float* beta, int64_t B, int32_t C, int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio,
                             int32_t down_taps, int32_t padding, int32_t act, int32_t logscale, float* dx, float* dalpha, float* dbeta,
                             double* workspace, ptmi_stream_t stream) {
    AaGeom G;
    bool def;
    PTMI_RETURN_IF(!dy || !x || !dx || (act && (!alpha || !beta)), PTMI_E_INVALID);
    PTMI_RETURN_IF((dalpha && (!act || !workspace)) || (dbeta && !dalpha), PTMI_E_INVALID);
    const int rc = aa_geom(B, C, T, up_filter != nullptr, up_ratio, up_taps, down_filter != nullptr, down_ratio, down_taps, padding, act,
                           logscale, true, &G, &def);
    if (rc != PTMI_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B == 0 || T == 0) {
        if (dalpha) PTMI_RETURN_IF(zero_words_async(dalpha, C, st) != hipSuccess, PTMI_E_INVALID);
        if (dbeta) PTMI_RETURN_IF(zero_words_async(dbeta, C, st) != hipSuccess, PTMI_E_INVALID);
        return PTMI_OK;
    }
    double* ws = dalpha ? workspace : nullptr;
    const dim3 grid((unsigned)(B * C * G.tiles));
    if (def) {
        const bool vec = G.T % 4 == 0 && aligned16({dx});
        if (vec)
            hipLaunchKernelGGL((aa_backward_kernel<true, 4>), grid, dim3(256), 0, st, dy, x, up_filter, down_filter, alpha, beta, dx, ws, G);
        else
            hipLaunchKernelGGL((aa_backward_kernel<true, 1>), grid, dim3(256), 0, st, dy, x, up_filter, down_filter, alpha, beta, dx, ws, G);
    } else {
        hipLaunchKernelGGL((aa_backward_kernel<false, 1>), grid, dim3(256), 0, st, dy, x, up_filter, down_filter, alpha, beta, dx, ws, G);
    }
    int rc2 = launch_status();
    if (rc2 != PTMI_OK || !dalpha) return rc2;
    hipLaunchKernelGGL(aa_param_finish_kernel, dim3((unsigned)C), dim3(256), 0, st, ws, (long long)B, (int)C, G.tiles, alpha, beta,
                       G.logscale, dalpha, dbeta);
    return launch_status();
}

}  // extern "C"
