// The mask estimator's loss (padertorch/contrib/jensheit/mask_estimator_example/model.py:128-237, add_losses): binary cross-entropy on
// logits, per example pooled by mean / median / min / max and, with the observation's power, the power-weighted mean - forward and
// backward, for the whole padded batch at once.  DESIGN.md "Mask loss".
//
//   logits, target [B, C, T, F] (unit stride on F, the other strides free), num_frames [B] on the device: frames t >= num_frames[b]
//   are never loaded.  A workgroup takes `rows_per_wg` rows (c, t) of one example (grid = (chunks, B)), a wave one row at a time, the
//   lanes stride over F (one float or one float4 each).
//
//   stats pass    sum l, sum l w, sum w per workgroup (fp64: thread ascending, wave butterfly, block_sums) -> workspace slabs ->
//                 colreduce; for a selection also the histogram of the keys' top 11 bits (LDS integer atomics, the non-empty bins
//                 added to the example's global histogram with integer atomics: counts do not depend on the order)
//   selection     radix select over key(l), the order-preserving 32-bit integer of the fp32 loss, 11 + 11 + 10 bits: scan (one
//                 workgroup per example: the bin that holds the rank, the rank inside it), histogram of the next digit over the
//                 elements that match the prefix, scan, histogram, scan.  The last scan leaves the key of the selected ELEMENT and
//                 the number m of elements with that key.  median: rank (n - 1) / 2, min: 0, max: n - 1.
//   finalize      pooled, weighted, and what the backward pass needs: stat [B, 4] float64, sel [B, 2] int32 (key, m)
//   backward      one pass: d logits = (g_pooled / n [mean] or g_pooled / m on key(l) == key [selection]) + g_weighted w / sum w, times
//                 sigmoid(x) - t; zeros behind num_frames.
//
// The loss is recomputed in every pass by element_loss(), written with explicit single-rounding intrinsics so that no pass contracts
// it differently from another: the keys of two passes are the same bits.
#include "reduce.h"

namespace ptmi {
namespace {

constexpr int kTopBits = 11, kBins = 1 << kTopBits;       // histogram bins (the widest digit)
constexpr unsigned kNanKey = 0xFFFFFFFFu;

enum Reduction { kMean = 0, kMedian = 1, kMin = 2, kMax = 3 };
enum Power { kNoPower = 0, kRealPower = 1, kComplexPower = 2 };

struct MaskGeo {
    long long ls[3], ts[3], ps[3];      // element strides of logits, target, power over (b, c, t); complex elements for a complex power
    int C, T, F, rows_per_wg;
};

// max(x, 0) - x t + log1p(exp(-|x|)), every operation rounded once and in this order.
__device__ __forceinline__ float element_loss(float x, float t) {
    return __fadd_rn(__fmaf_rn(-x, t, fmaxf(x, 0.f)), log1pf(expf(-fabsf(x))));
}

__device__ __forceinline__ float element_dloss(float x, float t) {       // sigmoid(x) - t
    const float e = expf(-fabsf(x));
    const float s = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    return s - t;
}

// Ascending in the value; every NaN is the largest key, -0 is +0.
__device__ __forceinline__ unsigned loss_key(float l) {
    if (l != l) return kNanKey;
    unsigned u = __float_as_uint(l);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float key_loss(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ int frames_of(const int32_t* __restrict__ num_frames, int b, int T) {
    if (!num_frames) return T;
    const int n = num_frames[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

// V weights at p: |.|^2 of V complex values, or V floats.
template <int V, int PW>
__device__ __forceinline__ void load_power(const float* __restrict__ p, long long f, float (&w)[V]) {
    if constexpr (PW == kComplexPower) {
#pragma unroll
        for (int h = 0; h < V; h += (V == 4 ? 2 : 1)) {
            if constexpr (V == 4) {
                const float4 z = *reinterpret_cast<const float4*>(p + 2 * (f + h));
                w[h] = __fmaf_rn(z.x, z.x, __fmul_rn(z.y, z.y));
                w[h + 1] = __fmaf_rn(z.z, z.z, __fmul_rn(z.w, z.w));
            } else {
                const float re = p[2 * f], im = p[2 * f + 1];
                w[h] = __fmaf_rn(re, re, __fmul_rn(im, im));
            }
        }
    } else {
        load_vec<V>(p + f, w);
    }
}

// The rows of this workgroup's chunk that belong to wave `wave`, ascending: fn(c, t) for every valid one.
template <class Fn>
__device__ __forceinline__ void for_rows(const MaskGeo& g, int nf, Fn fn) {
    const long long rows = (long long)g.C * g.T, r0 = (long long)blockIdx.x * g.rows_per_wg;
    for (int i = threadIdx.x >> 6; i < g.rows_per_wg; i += 4) {
        const long long r = r0 + i;
        if (r >= rows) break;
        const int c = (int)(r / g.T), t = (int)(r % g.T);
        if (t < nf) fn(c, t);
    }
}

__device__ __forceinline__ void flush_hist(const unsigned* hist, unsigned* __restrict__ ghist) {
    for (int i = threadIdx.x; i < kBins; i += 256)
        if (hist[i]) atomicAdd(&ghist[i], hist[i]);
}

// state [B, 4] uint32: prefix (the selected key's leading bits), rank inside the prefix, "a NaN was seen", elements in the selected bin
//
// Sums of a chunk -> ws[chunk][b][3]; HIST: the chunk's keys' top bits -> ghist [B, kBins].  Grid (chunks, B), 256 threads.
template <int V, int PW, bool HIST>
static __global__ __launch_bounds__(256) void mask_stats_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                const float* __restrict__ power, const int32_t* __restrict__ num_frames,
                                                                const MaskGeo g, double* __restrict__ ws, unsigned* __restrict__ ghist,
                                                                unsigned* __restrict__ state) {
    __shared__ unsigned hist[HIST ? kBins : 1];
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nf = frames_of(num_frames, b, g.T);
    if constexpr (HIST) {
        for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0u;
        __syncthreads();
    }
    double s[3] = {0., 0., 0.};
    bool nan = false;
    for_rows(g, nf, [&](int c, int t) {
        const float* lp = logits + b * g.ls[0] + c * g.ls[1] + t * g.ls[2];
        const float* tp = target + b * g.ts[0] + c * g.ts[1] + t * g.ts[2];
        const float* pp = PW == kNoPower ? nullptr : power + (b * g.ps[0] + c * g.ps[1] + t * g.ps[2]) * (PW == kComplexPower ? 2 : 1);
        for (int f = lane * V; f < g.F; f += 64 * V) {
            float x[V], y[V], w[V];
            load_vec<V>(lp + f, x);
            load_vec<V>(tp + f, y);
            if constexpr (PW != kNoPower) load_power<V, PW>(pp, f, w);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float l = element_loss(x[v], y[v]);
                s[0] += (double)l;
                if constexpr (PW != kNoPower) {
                    s[1] += (double)l * (double)w[v];
                    s[2] += (double)w[v];
                }
                if constexpr (HIST) {
                    const unsigned k = loss_key(l);
                    nan |= k == kNanKey;
                    atomicAdd(&hist[k >> (32 - kTopBits)], 1u);
                }
            }
        }
    });
    block_sums(s);
    if (threadIdx.x < 3) ws[((long long)blockIdx.x * gridDim.y + b) * 3 + threadIdx.x] = s[threadIdx.x];
    if constexpr (HIST) {
        const int any = __syncthreads_or(nan);
        if (any && threadIdx.x == 0) atomicOr(&state[4 * b + 2], 1u);
        flush_hist(hist, ghist + (long long)b * kBins);
    }
}

// Histogram of digit (key >> lo) & mask over the elements with key >> hi == state[b].prefix.  Grid (chunks, B).
template <int V>
static __global__ __launch_bounds__(256) void mask_hist_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                               const int32_t* __restrict__ num_frames, const MaskGeo g, int hi, int lo,
                                                               unsigned mask, unsigned* __restrict__ ghist,
                                                               const unsigned* __restrict__ state) {
    __shared__ unsigned hist[kBins];
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nf = frames_of(num_frames, b, g.T);
    const unsigned prefix = state[4 * b];
    for (int i = threadIdx.x; i < kBins; i += 256) hist[i] = 0u;
    __syncthreads();
    for_rows(g, nf, [&](int c, int t) {
        const float* lp = logits + b * g.ls[0] + c * g.ls[1] + t * g.ls[2];
        const float* tp = target + b * g.ts[0] + c * g.ts[1] + t * g.ts[2];
        for (int f = lane * V; f < g.F; f += 64 * V) {
            float x[V], y[V];
            load_vec<V>(lp + f, x);
            load_vec<V>(tp + f, y);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const unsigned k = loss_key(element_loss(x[v], y[v]));
                if ((k >> hi) == prefix) atomicAdd(&hist[(k >> lo) & mask], 1u);
            }
        }
    });
    __syncthreads();
    flush_hist(hist, ghist + (long long)b * kBins);
}

// One workgroup per example: the bin of ghist[b] that holds the rank; prefix <- prefix << bits | bin, rank <- rank inside the bin.
// first != 0: the rank is made here from the example's length and the reduction.  Leaves ghist[b] zeroed for the next pass.
static __global__ __launch_bounds__(256) void mask_scan_kernel(unsigned* __restrict__ ghist, unsigned* __restrict__ state,
                                                               const int32_t* __restrict__ num_frames, int C, int T, int F,
                                                               int reduction, int first, int bits) {
    __shared__ unsigned hist[kBins];
    __shared__ unsigned long long part[256];
    constexpr int per = kBins / 256;
    const int b = blockIdx.x;
    unsigned* gh = ghist + (long long)b * kBins;
    unsigned long long mine = 0;
    for (int i = 0; i < per; ++i) {
        const int j = threadIdx.x * per + i;
        hist[j] = gh[j];
        gh[j] = 0u;
        mine += hist[j];
    }
    part[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long rank;
    if (first) {
        const unsigned long long n = (unsigned long long)C * frames_of(num_frames, b, T) * F;
        rank = n == 0 ? 0 : (reduction == kMedian ? (n - 1) / 2 : (reduction == kMin ? 0 : n - 1));
    } else {
        rank = state[4 * b + 1];
    }
    unsigned long long cum = 0;
    int seg = 0;
    while (seg < 255 && cum + part[seg] <= rank) cum += part[seg++];
    int j = seg * per;
    while (j < seg * per + per - 1 && cum + hist[j] <= rank) cum += hist[j++];
    state[4 * b] = first ? (unsigned)j : ((state[4 * b] << bits) | (unsigned)j);
    state[4 * b + 1] = (unsigned)(rank - cum);
    state[4 * b + 3] = hist[j];
}

// pooled, weighted, stat [B, 4] = (sum l, sum l w, sum w, n), sel [B, 2] = (key, m).  One thread per example.
static __global__ void mask_finalize_kernel(const double* __restrict__ sums, const unsigned* __restrict__ state,
                                            const int32_t* __restrict__ num_frames, int B, int C, int T, int F, int reduction,
                                            int weighted_given, float* __restrict__ pooled, float* __restrict__ weighted,
                                            double* __restrict__ stat, int32_t* __restrict__ sel) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double n = (double)C * (double)frames_of(num_frames, b, T) * (double)F;
    const double sl = sums[3 * b], slw = sums[3 * b + 1], sw = sums[3 * b + 2];
    stat[4 * b] = sl, stat[4 * b + 1] = slw, stat[4 * b + 2] = sw, stat[4 * b + 3] = n;
    const float nanf_ = __uint_as_float(0x7FC00000u);
    if (reduction == kMean) {
        pooled[b] = (float)(sl / n);
        sel[2 * b] = 0, sel[2 * b + 1] = 0;
    } else {
        const bool bad = n == 0. || state[4 * b + 2] != 0u;
        const unsigned key = bad ? kNanKey : state[4 * b];
        pooled[b] = bad ? nanf_ : key_loss(key);
        sel[2 * b] = (int32_t)key;
        sel[2 * b + 1] = bad ? 1 : (int32_t)state[4 * b + 3];
    }
    if (weighted_given) weighted[b] = (float)(slw / sw);
}

struct StoreDouble {
    double* __restrict__ out;
    __device__ __forceinline__ void operator()(long long j, double tot) const { out[j] = tot; }
};

// d logits [B, C, T, F] dense.  Grid (chunks, B).
template <int V, int PW>
static __global__ __launch_bounds__(256) void mask_backward_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                                   const float* __restrict__ power, const int32_t* __restrict__ num_frames,
                                                                   const MaskGeo g, const float* __restrict__ g_pooled,
                                                                   const float* __restrict__ g_weighted, const double* __restrict__ stat,
                                                                   const int32_t* __restrict__ sel, int reduction, float* __restrict__ out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int nf = frames_of(num_frames, b, g.T);
    const double gp = g_pooled ? (double)g_pooled[b] : 0.;
    const unsigned key = (unsigned)sel[2 * b];
    const float ca = (float)(gp / (reduction == kMean ? stat[4 * b + 3] : (double)sel[2 * b + 1]));
    const float cw = PW != kNoPower && g_weighted ? (float)((double)g_weighted[b] / stat[4 * b + 2]) : 0.f;
    const bool select = reduction != kMean, pooled_given = g_pooled != nullptr, weighted_given = PW != kNoPower && g_weighted;
    const long long rows = (long long)g.C * g.T, r0 = (long long)blockIdx.x * g.rows_per_wg;
    for (int i = threadIdx.x >> 6; i < g.rows_per_wg; i += 4) {
        const long long r = r0 + i;
        if (r >= rows) break;
        const int c = (int)(r / g.T), t = (int)(r % g.T);
        float* op = out + ((long long)b * rows + r) * g.F;
        if (t >= nf) {
            float z[V];
#pragma unroll
            for (int v = 0; v < V; ++v) z[v] = 0.f;
            for (int f = lane * V; f < g.F; f += 64 * V) store_vec<V>(op + f, z);
            continue;
        }
        const float* lp = logits + b * g.ls[0] + c * g.ls[1] + t * g.ls[2];
        const float* tp = target + b * g.ts[0] + c * g.ts[1] + t * g.ts[2];
        const float* pp = PW == kNoPower ? nullptr : power + (b * g.ps[0] + c * g.ps[1] + t * g.ps[2]) * (PW == kComplexPower ? 2 : 1);
        for (int f = lane * V; f < g.F; f += 64 * V) {
            float x[V], y[V], w[V], d[V];
            load_vec<V>(lp + f, x);
            load_vec<V>(tp + f, y);
            if constexpr (PW != kNoPower) load_power<V, PW>(pp, f, w);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float coef = 0.f;
                if (pooled_given && (!select || loss_key(element_loss(x[v], y[v])) == key)) coef = ca;
                if constexpr (PW != kNoPower)
                    if (weighted_given) coef += cw * w[v];
                d[v] = coef == 0.f ? 0.f : coef * element_dloss(x[v], y[v]);
            }
            store_vec<V>(op + f, d);
        }
    }
}

inline int rows_per_wg(int F) {
    const int r = (8192 + F - 1) / F;
    return r < 1 ? 1 : r;
}

inline long long chunks_of(int C, int T, int F) {
    const int r = rows_per_wg(F);
    return ((long long)C * T + r - 1) / r;
}

// doubles in front of the integer words of the workspace
inline long long sum_elems(long long B, int C, int T, int F) { return (chunks_of(C, T, F) + 1) * B * 3; }

inline bool mask_args_ok(int64_t B, int32_t C, int32_t T, int32_t F) {
    return B >= 1 && B <= 65535 && C >= 1 && T >= 1 && F >= 1 && (long long)C * T * F < (1ll << 31) && chunks_of(C, T, F) < (1ll << 31);
}

MaskGeo make_geo(const int64_t* st, int32_t C, int32_t T, int32_t F) {
    MaskGeo g;
    for (int i = 0; i < 3; ++i) g.ls[i] = st[i], g.ts[i] = st[3 + i], g.ps[i] = st[6 + i];
    g.C = C, g.T = T, g.F = F, g.rows_per_wg = rows_per_wg(F);
    return g;
}

bool vec_ok(const MaskGeo& g, const float* logits, const float* target, const float* power, int power_kind, const float* out) {
    if (g.F % 4 || !aligned16({logits, target, power, out})) return false;
    for (int i = 0; i < 3; ++i) {
        if (g.ls[i] % 4 || g.ts[i] % 4) return false;
        if (power_kind == kRealPower && g.ps[i] % 4) return false;
        if (power_kind == kComplexPower && g.ps[i] % 2) return false;
    }
    return true;
}

template <int V, bool HIST>
void launch_stats(int pk, dim3 grid, hipStream_t st, const float* logits, const float* target, const float* power, const int32_t* nf,
                  const MaskGeo& g, double* ws, unsigned* ghist, unsigned* state) {
    if (pk == kNoPower)
        hipLaunchKernelGGL((mask_stats_kernel<V, kNoPower, HIST>), grid, dim3(256), 0, st, logits, target, power, nf, g, ws, ghist, state);
    else if (pk == kRealPower)
        hipLaunchKernelGGL((mask_stats_kernel<V, kRealPower, HIST>), grid, dim3(256), 0, st, logits, target, power, nf, g, ws, ghist, state);
    else
        hipLaunchKernelGGL((mask_stats_kernel<V, kComplexPower, HIST>), grid, dim3(256), 0, st, logits, target, power, nf, g, ws, ghist,
                           state);
}

template <int V>
void launch_backward(int pk, dim3 grid, hipStream_t st, const float* logits, const float* target, const float* power, const int32_t* nf,
                     const MaskGeo& g, const float* gp, const float* gw, const double* stat, const int32_t* sel, int reduction, float* out) {
    if (pk == kNoPower)
        hipLaunchKernelGGL((mask_backward_kernel<V, kNoPower>), grid, dim3(256), 0, st, logits, target, power, nf, g, gp, gw, stat, sel,
                           reduction, out);
    else if (pk == kRealPower)
        hipLaunchKernelGGL((mask_backward_kernel<V, kRealPower>), grid, dim3(256), 0, st, logits, target, power, nf, g, gp, gw, stat, sel,
                           reduction, out);
    else
        hipLaunchKernelGGL((mask_backward_kernel<V, kComplexPower>), grid, dim3(256), 0, st, logits, target, power, nf, g, gp, gw, stat,
                           sel, reduction, out);
}

}  // namespace
}  // namespace ptmi

using namespace ptmi;

extern "C" int64_t ptmi_mask_loss_workspace_elems(int64_t B, int32_t C, int32_t T, int32_t F) {
    if (!mask_args_ok(B, C, T, F)) return 0;
    return sum_elems(B, C, T, F) + (B * (kBins + 4) + 1) / 2;
}

extern "C" int ptmi_mask_loss_forward(const float* logits, const float* target, const void* power, int32_t power_kind,
                                      const int32_t* num_frames, const int64_t* strides, int64_t B, int32_t C, int32_t T, int32_t F,
                                      int32_t reduction, double* workspace, float* pooled, float* weighted, double* stat, int32_t* sel,
                                      ptmi_stream_t stream) {
    PTMI_RETURN_IF(!logits || !target || !strides || !workspace || !pooled || !stat || !sel, PTMI_E_INVALID);
    PTMI_RETURN_IF(!mask_args_ok(B, C, T, F) || reduction < kMean || reduction > kMax, PTMI_E_INVALID);
    PTMI_RETURN_IF(power_kind < kNoPower || power_kind > kComplexPower || (power_kind != kNoPower && (!power || !weighted)), PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MaskGeo g = make_geo(strides, C, T, F);
    const float* pw = static_cast<const float*>(power_kind == kNoPower ? nullptr : power);
    const bool vec = vec_ok(g, logits, target, pw, power_kind, nullptr);
    const long long chunks = chunks_of(C, T, F);
    const dim3 grid((unsigned)chunks, (unsigned)B);
    double* sums = workspace + chunks * B * 3;
    unsigned* ghist = reinterpret_cast<unsigned*>(workspace + sum_elems(B, C, T, F));
    unsigned* state = ghist + B * kBins;
    const bool select = reduction != kMean;
    if (select) {
        hipError_t e = zero_words_async(ghist, (size_t)B * (kBins + 4), st);
        PTMI_RETURN_IF(e != hipSuccess, static_cast<int>(e));
        if (vec)
            launch_stats<4, true>(power_kind, grid, st, logits, target, pw, num_frames, g, workspace, ghist, state);
        else
            launch_stats<1, true>(power_kind, grid, st, logits, target, pw, num_frames, g, workspace, ghist, state);
    } else if (vec) {
        launch_stats<4, false>(power_kind, grid, st, logits, target, pw, num_frames, g, workspace, ghist, state);
    } else {
        launch_stats<1, false>(power_kind, grid, st, logits, target, pw, num_frames, g, workspace, ghist, state);
    }
    int rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    rc = colreduce(workspace, chunks, B * 3, StoreDouble{sums}, st);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    if (select) {
        const int hi[3] = {0, 32 - kTopBits, 32 - 2 * kTopBits}, bits[3] = {kTopBits, kTopBits, 32 - 2 * kTopBits};
        for (int p = 0; p < 3; ++p) {
            if (p > 0) {
                const int lo = hi[p] - bits[p];
                PTMI_LAUNCH_VEC(mask_hist_kernel, vec, grid, st, logits, target, num_frames, g, hi[p], lo, (1u << bits[p]) - 1u, ghist,
                                (const unsigned*)state);
                rc = launch_status();
                PTMI_RETURN_IF(rc != PTMI_OK, rc);
            }
            hipLaunchKernelGGL(mask_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, ghist, state, num_frames, C, T, F, reduction,
                               (int)(p == 0), bits[p]);
            rc = launch_status();
            PTMI_RETURN_IF(rc != PTMI_OK, rc);
        }
    }
    hipLaunchKernelGGL(mask_finalize_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, (const double*)sums,
                       (const unsigned*)state, num_frames, (int)B, C, T, F, reduction, (int)(power_kind != kNoPower), pooled, weighted, stat,
                       sel);
    return launch_status();
}

extern "C" int ptmi_mask_loss_backward(const float* logits, const float* target, const void* power, int32_t power_kind,
                                       const int32_t* num_frames, const int64_t* strides, const float* g_pooled, const float* g_weighted,
                                       const double* stat, const int32_t* sel, int64_t B, int32_t C, int32_t T, int32_t F,
                                       int32_t reduction, float* dlogits, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!logits || !target || !strides || !stat || !sel || !dlogits, PTMI_E_INVALID);
    PTMI_RETURN_IF(!mask_args_ok(B, C, T, F) || reduction < kMean || reduction > kMax, PTMI_E_INVALID);
    PTMI_RETURN_IF(power_kind < kNoPower || power_kind > kComplexPower || (power_kind != kNoPower && !power), PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MaskGeo g = make_geo(strides, C, T, F);
    const float* pw = static_cast<const float*>(power_kind == kNoPower ? nullptr : power);
    const dim3 grid((unsigned)chunks_of(C, T, F), (unsigned)B);
    if (vec_ok(g, logits, target, pw, power_kind, dlogits))
        launch_backward<4>(power_kind, grid, st, logits, target, pw, num_frames, g, g_pooled, g_weighted, stat, sel, reduction, dlogits);
    else
        launch_backward<1>(power_kind, grid, st, logits, target, pw, num_frames, g, g_pooled, g_weighted, stat, sel, reduction, dlogits);
    return launch_status();
}
