// The feature extractor of padertorch/contrib/je/modules/features.py:142-206 (NormalizedLogMelExtractor.forward) and the augmentations
// of contrib/je/modules/augment.py as three memory-bound kernels (include/ptmi.h: ptmi_je_logmel_front, ptmi_je_feature_shape,
// ptmi_je_feature_tail).  fp32, forward only: the reference runs all of it under no_grad.  Every random quantity is drawn on the host
// (ops/je_features.py, contrib/je/modules/augment.py) and arrives as a small per-example table.
//
//   jf_front_kernel  stacked STFT [B, C, T, F, 2] -> log-mel [B, C, M, T] (+ cos / sin of the inter-channel phase differences).
//                    A workgroup owns one (example, channel) and kJfFrontTile = 32 frames.  The tile is ONE contiguous run of 32 F
//                    complex values: read with 16-byte loads (a leading / trailing 8-byte element where the run starts or ends on an odd
//                    element), scaled and superposed with the partner example in the complex domain, squared, and written as power
//                    rows [32][PS] into LDS (PS = F rounded up to 4, + 8, then up to 4 mod 64: b128 reads of 16 neighbouring frames hit
//                    64 different banks).  Then a lane owns (filter, frame) pairs, frame fastest: it walks the filter's few 4-bin groups
//                    of ITS frame's row with b128 LDS reads and stores along T - the transpose happens in LDS, the store is contiguous.
//                    Static filterbank: the band-compressed weights of ptmi_mel_apply (read through the scalar cache: a half wave shares
//                    a filter).  Warped filterbank: a prologue thread per filter turns the example's three edge frequencies into the
//                    bin range, the two slopes and 1 / (sum + 1e-6) in LDS; the triangle weights are evaluated in registers, so no
//                    [B, M, F] matrix exists anywhere.  Workgroups with blockIdx.y >= C own a channel PAIR instead: two gathered complex
//                    values per (filter, frame) at the filter's peak bin -> cos, sin of atan2(cross, dot) = (dot, cross) / hypot.
//                    The product is banded (a handful of bins per filter) and ends in a transpose: a matrix instruction would multiply
//                    zeros for > 90 % of a 16 x 16 x 4 tile and the kernel is bound by the one read of x, so it is plain fmaf.
//   jf_shape_kernel  log-mel [B, C, M, T] -> [B, C (1 + d + dd), M, T']: time warp, Gaussian blur, deltas.  A workgroup owns one (b, c)
//                    plane and kJfShapeTile = 64 output frames.  It gathers (and linearly interpolates) the frames t0 - h .. t1 + h,
//                    h = (k - 1) / 2 + 2, reflected at the plane's edges, into the LDS image A [M][WA]; blurs along T into B [M][WB],
//                    along M (reflected) back into A; and writes the static channel and both Savitzky-Golay derivatives from A.
//   jf_tail_kernel   [B, C', M, T] (+ IPD channels) -> [B, C' + 2 P, M, T]: (x - mean) rstd, clamp, length mask, mixup with the
//                    partner example (normalised the same way from ITS raw features), additive noise, time and frequency masks.
//                    Elementwise over a plane, 16-byte accesses when M T % 4 == 0; a partner whose weight is 0 is never read.
#include <math.h>

#include "common.h"

namespace ptmi {

constexpr int kJfFrontTile = 32;
constexpr int kJfShapeTile = 64;
constexpr int kJfMaxF = 1025, kJfMaxM = 256, kJfMaxC = 8, kJfMaxK = 9, kJfMaxPairs = kJfMaxC * (kJfMaxC - 1);
constexpr size_t kJfLdsLimit = 160 * 1024, kJfLdsDefault = 64 * 1024;

struct JfFrontArgs {
    const float* x;
    const float *gain, *pgain, *lambda, *w, *edges;
    const int32_t *partner, *lo, *cnt, *off, *max_bin;
    float *logmel, *ipd_cos, *ipd_sin;
    long long T;
    int C, F, M, PS, n_pairs;
    float eps, bin_hz, inv_F;
    uint8_t pair_ref[kJfMaxPairs], pair_other[kJfMaxPairs];
};

// gain x_b + (lambda partner_gain) x_partner: one complex value
__device__ __forceinline__ float2 jf_superpose(float2 v, float2 w, float g, float pg) {
    return make_float2(g * v.x + pg * w.x, g * v.y + pg * w.y);
}

__device__ __forceinline__ float jf_triangle(float f, float l, float r, float il, float ir) {
    return fmaxf(0.f, fminf((f - l) * il, (r - f) * ir));
}

__global__ __launch_bounds__(256) void jf_front_kernel(const JfFrontArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.z, t0 = blockIdx.x * kJfFrontTile, tid = threadIdx.x;
    const int nt = (int)min((long long)kJfFrontTile, A.T - t0);
    const float g = A.gain ? A.gain[b] : 1.f;
    const int pb = A.partner ? min(max(A.partner[b], 0), (int)gridDim.z - 1) : -1;
    const float pg = pb >= 0 ? A.lambda[b] * A.pgain[b] : 0.f;
    const bool mix = pg != 0.f;                                   // a partner of weight 0 is never read
    const float2* X = reinterpret_cast<const float2*>(A.x);
    const float2 zero = make_float2(0.f, 0.f);

    if ((int)blockIdx.y >= A.C) {                                 // a channel pair: phase differences at the filters' peak bins
        const int p = blockIdx.y - A.C, cr = A.pair_ref[p], co = A.pair_other[p];
        for (int o = tid; o < A.M * kJfFrontTile; o += 256) {
            const int m = o / kJfFrontTile, tt = o % kJfFrontTile;
            if (tt >= nt) continue;
            const int k = min(max(A.max_bin[m], 0), A.F - 1);
            const long long fr = ((long long)b * A.C * A.T + t0 + tt) * A.F + k, pfr = ((long long)pb * A.C * A.T + t0 + tt) * A.F + k;
            const long long sr = (long long)cr * A.T * A.F, so = (long long)co * A.T * A.F;
            const float2 zr = jf_superpose(X[fr + sr], mix ? X[pfr + sr] : zero, g, pg);
            const float2 zo = jf_superpose(X[fr + so], mix ? X[pfr + so] : zero, g, pg);
            const float cross = zo.y * zr.x - zo.x * zr.y, dot = zo.x * zr.x + zo.y * zr.y;
            const float h = hypotf(cross, dot);
            const long long at = (((long long)b * A.n_pairs + p) * A.M + m) * A.T + t0 + tt;
            A.ipd_cos[at] = h > 0.f ? dot / h : 1.f;              // atan2(0, 0) = 0
            A.ipd_sin[at] = h > 0.f ? cross / h : 0.f;
        }
        return;
    }

    const int c = blockIdx.y, PS = A.PS;
    float* rows = reinterpret_cast<float*>(smem);                 // [kJfFrontTile][PS] power
    float* fl = rows + kJfFrontTile * PS;                         // warped filters: left, right, 1 / (centre - left), 1 / (right - centre),
    float *fr = fl + A.M, *fil = fr + A.M, *fir = fil + A.M, *finv = fir + A.M;      // 1 / (sum + 1e-6)
    int* fg0 = reinterpret_cast<int*>(finv + A.M);                // first 4-bin group, number of groups
    int* fng = fg0 + A.M;

    if (A.edges && tid < A.M) {
        const float* e = A.edges + (long long)b * (A.M + 2) + tid;
        const float l = e[0], ce = e[1], r = e[2], il = 1.f / (ce - l), ir = 1.f / (r - ce);
        const int k0 = min(max((int)floorf(l / A.bin_hz), 0), A.F - 1), k1 = min(max((int)ceilf(r / A.bin_hz), k0), A.F - 1);
        float s = 0.f;
        for (int k = k0; k <= k1; ++k) s += jf_triangle((float)k * A.bin_hz, l, r, il, ir);
        fl[tid] = l;
        fr[tid] = r;
        fil[tid] = il;
        fir[tid] = ir;
        finv[tid] = 1.f / (s + 1e-6f);
        fg0[tid] = k0 / 4;
        fng[tid] = k1 / 4 - k0 / 4 + 1;
    }
    for (int i = tid; i < kJfFrontTile * (PS - A.F); i += 256) rows[(i / (PS - A.F)) * PS + A.F + i % (PS - A.F)] = 0.f;

    // the tile of x[b, c]: n consecutive complex values from `start`; (head) 8-byte element, 16-byte pairs, (tail) 8-byte element
    const float2* src = X + (((long long)b * A.C + c) * A.T + t0) * A.F;
    const float2* psrc = X + (((long long)(mix ? pb : b) * A.C + c) * A.T + t0) * A.F;
    const int n = nt * A.F, head = (int)((reinterpret_cast<uintptr_t>(src) >> 3) & 1);
    const bool paired = ((reinterpret_cast<uintptr_t>(psrc + head)) & 15) == 0;
    auto put = [&](int e, float2 v, float2 w) {
        const float2 z = jf_superpose(v, w, g, pg);
        const int f = (int)(((float)e + 0.5f) * A.inv_F);         // e / F: e < 2^16, the quotient is 0.5 / F away from an integer
        rows[f * PS + e - f * A.F] = z.x * z.x + z.y * z.y;
    };
    if (head && tid == 0) put(0, src[0], mix ? psrc[0] : zero);
    const int pairs = (n - head) / 2;
    for (int i = tid; i < pairs; i += 256) {
        const int e = head + 2 * i;
        const float4 v = *reinterpret_cast<const float4*>(src + e);
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (mix) {
            if (paired) {
                w = *reinterpret_cast<const float4*>(psrc + e);
            } else {
                const float2 w0 = psrc[e], w1 = psrc[e + 1];
                w = make_float4(w0.x, w0.y, w1.x, w1.y);
            }
        }
        put(e, make_float2(v.x, v.y), make_float2(w.x, w.y));
        put(e + 1, make_float2(v.z, v.w), make_float2(w.z, w.w));
    }
    if (((n - head) & 1) && tid == 255) put(n - 1, src[n - 1], mix ? psrc[n - 1] : zero);
    __syncthreads();

    const float4* W4 = reinterpret_cast<const float4*>(A.w);
    for (int o = tid; o < A.M * kJfFrontTile; o += 256) {
        const int m = o / kJfFrontTile, tt = o % kJfFrontTile;
        if (tt >= nt) continue;
        const float4* pr = reinterpret_cast<const float4*>(rows + tt * PS);
        float acc = 0.f;
        if (A.edges) {
            const float l = fl[m], r = fr[m], il = fil[m], ir = fir[m];
            const int g0 = fg0[m];
            for (int i = 0; i < fng[m]; ++i) {
                const float4 p = pr[g0 + i];
                const float f0 = (float)(4 * (g0 + i)) * A.bin_hz, f1 = (float)(4 * (g0 + i) + 1) * A.bin_hz,
                            f2 = (float)(4 * (g0 + i) + 2) * A.bin_hz, f3 = (float)(4 * (g0 + i) + 3) * A.bin_hz;
                acc = fmaf(p.x, jf_triangle(f0, l, r, il, ir), acc);
                acc = fmaf(p.y, jf_triangle(f1, l, r, il, ir), acc);
                acc = fmaf(p.z, jf_triangle(f2, l, r, il, ir), acc);
                acc = fmaf(p.w, jf_triangle(f3, l, r, il, ir), acc);
            }
            acc *= finv[m];
        } else {
            const float4* pw = pr + A.lo[m];
            const float4* w = W4 + A.off[m];
            for (int i = 0; i < A.cnt[m]; ++i) {
                const float4 p0 = pw[2 * i], p1 = pw[2 * i + 1], w0 = w[2 * i], w1 = w[2 * i + 1];
                acc = fmaf(p0.x, w0.x, acc);
                acc = fmaf(p0.y, w0.y, acc);
                acc = fmaf(p0.z, w0.z, acc);
                acc = fmaf(p0.w, w0.w, acc);
                acc = fmaf(p1.x, w1.x, acc);
                acc = fmaf(p1.y, w1.y, acc);
                acc = fmaf(p1.z, w1.z, acc);
                acc = fmaf(p1.w, w1.w, acc);
            }
        }
        // the fp64 logarithm of the fp32 sum, rounded once: an all-zero frame gives the float nearest to log(eps) (logf is 1 ulp off there)
        A.logmel[(((long long)b * A.C + c) * A.M + m) * A.T + t0 + tt] = (float)log((double)(acc + A.eps));
    }
}

struct JfShapeArgs {
    const float *x, *frac, *taps;
    const int32_t *floor_, *seq;
    float* out;
    long long T, To;
    int C, M, k, d, dd, WA, WB;
    float kd[5], kdd[5];
};

__global__ __launch_bounds__(256) void jf_shape_kernel(const JfShapeArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * kJfShapeTile;
    const int nt = (int)min((long long)kJfShapeTile, A.To - t0);
    const int hb = A.taps ? (A.k - 1) / 2 : 0, hd = (A.d || A.dd) ? 2 : 0, h = hb + hd;
    const int wa = kJfShapeTile + 2 * h, wb = kJfShapeTile + 2 * hd, WA = A.WA, WB = A.WB;
    float* Ab = reinterpret_cast<float*>(smem);                   // [M][WA]: column j <-> frame t0 - h + j
    float* Bb = Ab + A.M * WA;                                    // [M][WB]: column j <-> frame t0 - hd + j
    const float* plane = A.x + ((long long)b * A.C + c) * A.M * A.T;

    const float inv_wa = 1.f / (float)wa, inv_wb = 1.f / (float)wb;
    for (int o = tid; o < A.M * wa; o += 256) {
        const int m = (int)(((float)o + 0.5f) * inv_wa), j = o - m * wa;
        long long u = t0 - h + j;
        u = u < 0 ? -u : (u >= A.To ? 2 * (A.To - 1) - u : u);    // reflect; a column further out feeds no output: clamped only
        u = min(max(u, 0LL), A.To - 1);
        const float* row = plane + (long long)m * A.T;
        float v;
        if (A.floor_) {
            const long long i0 = min(max((long long)A.floor_[b * A.To + u], 0LL), A.T - 1);
            const float fc = A.frac[b * A.To + u];                // tau - floor(tau); 0: tau is an integer, ceil = floor
            const long long i1 = min(i0 + (fc > 0.f ? 1 : 0), A.T - 1);
            v = fc > 0.f ? fc * row[i1] + (1.f - fc) * row[i0] : row[i0];
        } else {
            v = row[u];
        }
        Ab[m * WA + j] = v;
    }
    if (hb) {
        float tap[kJfMaxK];
#pragma unroll
        for (int i = 0; i < kJfMaxK; ++i) tap[i] = i < A.k ? A.taps[b * A.k + i] : 0.f;
        __syncthreads();
        for (int o = tid; o < A.M * wb; o += 256) {
            const int m = (int)(((float)o + 0.5f) * inv_wb), j = o - m * wb;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < kJfMaxK; ++i)
                if (i < A.k) acc = fmaf(tap[i], Ab[m * WA + j + i], acc);
            Bb[m * WB + j] = acc;
        }
        __syncthreads();
        for (int o = tid; o < A.M * wb; o += 256) {
            const int m = (int)(((float)o + 0.5f) * inv_wb), j = o - m * wb;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < kJfMaxK; ++i)
                if (i < A.k) {
                    int mm = m + i - hb;
                    mm = mm < 0 ? -mm : (mm >= A.M ? 2 * (A.M - 1) - mm : mm);
                    acc = fmaf(tap[i], Bb[mm * WB + j], acc);
                }
            Ab[m * WA + j] = acc;
        }
    }
    __syncthreads();

    const int n_out = A.C * (1 + A.d + A.dd);
    const long long len = A.seq ? (long long)A.seq[b] : A.To;
    for (int o = tid; o < A.M * kJfShapeTile; o += 256) {
        const int m = o / kJfShapeTile, tt = o % kJfShapeTile;
        if (tt >= nt) continue;
        const long long t = t0 + tt;
        const float* s = Ab + m * WA + tt;                        // s[hd] is frame t, s[0 .. 4] are t - 2 .. t + 2
        float* out = A.out + (((long long)b * n_out + c) * A.M + m) * A.To + t;
        const long long step = (long long)A.C * A.M * A.To;
        out[0] = s[hd];
        const bool inner = t >= 2 && t < A.To - 2 && t < len - 2;
        if (A.d) out[step] = inner ? A.kd[0] * s[0] + A.kd[1] * s[1] + A.kd[2] * s[2] + A.kd[3] * s[3] + A.kd[4] * s[4] : 0.f;
        if (A.dd)
            out[step * (1 + A.d)] = inner ? A.kdd[0] * s[0] + A.kdd[1] * s[1] + A.kdd[2] * s[2] + A.kdd[3] * s[3] + A.kdd[4] * s[4] : 0.f;
    }
}

struct JfTailArgs {
    const float *x, *mean, *rstd, *ipd_cos, *ipd_sin, *lambda, *noise_scale, *noise;
    const int32_t *partner, *seq, *t_on, *t_off, *f_on, *f_off;
    float* out;
    long long T, mean_sc, mean_sf;
    int B, C, P, M, n_t, n_f, has_clamp;
    float clamp;
};

template <int V>
__global__ __launch_bounds__(256) void jf_tail_kernel(const JfTailArgs A) {
    const int b = blockIdx.z, ch = blockIdx.y;
    const long long plane = (long long)A.M * A.T, i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i0 >= plane) return;
    const bool feat = ch < A.C;
    // the plane of channel ch of example e: a feature channel of x, or a cos / sin plane
    auto src = [&](int e) {
        if (feat) return A.x + ((long long)e * A.C + ch) * plane;
        return ch < A.C + A.P ? A.ipd_cos + ((long long)e * A.P + ch - A.C) * plane : A.ipd_sin + ((long long)e * A.P + ch - A.C - A.P) * plane;
    };
    const float lam = A.partner ? A.lambda[b] : 1.f;
    const int pb = lam != 1.f ? min(max(A.partner[b], 0), A.B - 1) : b;      // a partner of weight 0 is never read
    const long long at = ((long long)b * (A.C + 2 * A.P) + ch) * plane + i0;
    float v[V], w[V], nz[V];
    if (V == 4) {
        *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(src(b) + i0);
        *reinterpret_cast<float4*>(w) = lam != 1.f ? *reinterpret_cast<const float4*>(src(pb) + i0) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(nz) = A.noise ? *reinterpret_cast<const float4*>(A.noise + at) : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        v[0] = src(b)[i0];
        w[0] = lam != 1.f ? src(pb)[i0] : 0.f;
        nz[0] = A.noise ? A.noise[at] : 0.f;
    }
    const long long len = A.seq ? A.seq[b] : A.T, plen = A.seq ? A.seq[pb] : A.T;
    const float ns = A.noise ? A.noise_scale[b] : 0.f;
    int m = (int)(i0 / A.T);
    long long t = i0 - (long long)m * A.T;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        float a = v[j], p = w[j];
        if (feat) {
            const long long st = ch * A.mean_sc + m * A.mean_sf;
            if (A.mean) a -= A.mean[st], p -= A.mean[st];
            if (A.rstd) a *= A.rstd[st], p *= A.rstd[st];
            if (A.has_clamp) a = fminf(fmaxf(a, -A.clamp), A.clamp), p = fminf(fmaxf(p, -A.clamp), A.clamp);
            a = t < len ? a : 0.f;
            p = t < plen ? p : 0.f;
        }
        if (lam != 1.f) a = lam * a + (1.f - lam) * p;
        if (A.noise) a = fmaf(ns, nz[j], a);
        bool keep = true;
        for (int i = 0; i < A.n_t; ++i) keep = keep && (t < A.t_on[i * A.B + b] || t >= A.t_off[i * A.B + b]);
        for (int i = 0; i < A.n_f; ++i) keep = keep && (m < A.f_on[i * A.B + b] || m >= A.f_off[i * A.B + b]);
        v[j] = keep ? a : 0.f;
        if (++t == A.T) t = 0, ++m;
    }
    if (V == 4)
        *reinterpret_cast<float4*>(A.out + at) = *reinterpret_cast<float4*>(v);
    else
        A.out[at] = v[0];
}

template <typename K>
static int jf_lds_opt_in(K kernel, size_t lds) {
    PTMI_RETURN_IF(lds > kJfLdsLimit, PTMI_E_UNSUPPORTED);
    if (lds > kJfLdsDefault)
        PTMI_RETURN_IF(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess,
                       PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

static bool jf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_je_front_tile(void) { return kJfFrontTile; }
int32_t ptmi_je_shape_tile(void) { return kJfShapeTile; }

int ptmi_je_logmel_front(const float* x, int64_t B, int32_t C, int64_t T, int32_t F, const float* gain, const int32_t* partner,
                         const float* partner_gain, const float* lambda, const int32_t* mel_lo, const int32_t* mel_cnt, const int32_t* mel_off,
                         const float* mel_w, const float* edges_hz, float bin_hz, const int32_t* max_bin, int32_t M, const int32_t* pair_ref,
                         const int32_t* pair_other, int32_t n_pairs, float eps, float* logmel, float* ipd_cos, float* ipd_sin,
                         ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !logmel || B < 0 || T < 0 || C < 1 || F < 1 || M < 1 || n_pairs < 0, PTMI_E_INVALID);
    PTMI_RETURN_IF(!edges_hz && (!mel_lo || !mel_cnt || !mel_off || !mel_w), PTMI_E_INVALID);
    PTMI_RETURN_IF(edges_hz && !(bin_hz > 0.f), PTMI_E_INVALID);
    PTMI_RETURN_IF(partner && (!partner_gain || !lambda), PTMI_E_INVALID);
    PTMI_RETURN_IF(n_pairs > 0 && (!pair_ref || !pair_other || !max_bin || !ipd_cos || !ipd_sin), PTMI_E_INVALID);
    PTMI_RETURN_IF((reinterpret_cast<uintptr_t>(x) & 7) || (!edges_hz && !jf_aligned16(mel_w)), PTMI_E_INVALID);
    PTMI_RETURN_IF(F > kJfMaxF || M > kJfMaxM || C > kJfMaxC || n_pairs > kJfMaxPairs || B > 65535, PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(T > 0x7fffffffLL / kJfMaxM, PTMI_E_UNSUPPORTED);
    if (B == 0 || T == 0) return PTMI_OK;
    JfFrontArgs A{};
    A.x = x, A.gain = gain, A.pgain = partner_gain, A.lambda = lambda, A.w = mel_w, A.edges = edges_hz, A.partner = partner;
    A.lo = mel_lo, A.cnt = mel_cnt, A.off = mel_off, A.max_bin = max_bin, A.logmel = logmel, A.ipd_cos = ipd_cos, A.ipd_sin = ipd_sin;
    A.T = T, A.C = C, A.F = F, A.M = M, A.n_pairs = n_pairs, A.eps = eps, A.bin_hz = bin_hz, A.inv_F = 1.f / (float)F;
    for (int p = 0; p < n_pairs; ++p) {
        PTMI_RETURN_IF(pair_ref[p] < 0 || pair_ref[p] >= C || pair_other[p] < 0 || pair_other[p] >= C, PTMI_E_INVALID);
        A.pair_ref[p] = (uint8_t)pair_ref[p], A.pair_other[p] = (uint8_t)pair_other[p];
    }
    A.PS = ((F + 3) & ~3) + 8;
    A.PS += (4 - A.PS % 64 + 64) % 64;
    const size_t lds = sizeof(float) * ((size_t)kJfFrontTile * A.PS + 7 * (size_t)M);
    const int rc = jf_lds_opt_in(jf_front_kernel, lds);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const dim3 grid((unsigned)((T + kJfFrontTile - 1) / kJfFrontTile), (unsigned)(C + n_pairs), (unsigned)B);
    hipLaunchKernelGGL(jf_front_kernel, grid, dim3(256), lds, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int ptmi_je_feature_shape(const float* x, int64_t B, int32_t C, int32_t M, int64_t T, const int32_t* time_floor, const float* time_frac,
                          int64_t T_out, const float* taps, int32_t k, int32_t add_deltas, int32_t add_delta_deltas, const float* delta_kernel,
                          const float* delta_delta_kernel, int32_t delta_width, const int32_t* seq_len, float* out, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !out || B < 0 || T < 1 || T_out < 0 || C < 1 || M < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((time_floor == nullptr) != (time_frac == nullptr) || (!time_floor && T_out != T), PTMI_E_INVALID);
    PTMI_RETURN_IF((add_deltas && !delta_kernel) || (add_delta_deltas && !delta_delta_kernel), PTMI_E_INVALID);
    PTMI_RETURN_IF(taps && (k < 1 || k % 2 == 0), PTMI_E_INVALID);
    PTMI_RETURN_IF(M > kJfMaxM || C > kJfMaxC || B > 65535 || (taps && k > kJfMaxK), PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF((add_deltas || add_delta_deltas) && delta_width != 5, PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(taps && (T_out < (k + 1) / 2 || M < (k + 1) / 2), PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(T > 0x7fffffffLL / kJfMaxM || T_out > 0x7fffffffLL / kJfMaxM, PTMI_E_UNSUPPORTED);
    if (B == 0 || T_out == 0) return PTMI_OK;
    JfShapeArgs A{};
    A.x = x, A.frac = time_frac, A.taps = taps, A.floor_ = time_floor, A.seq = seq_len, A.out = out;
    A.T = T, A.To = T_out, A.C = C, A.M = M, A.k = taps ? k : 1, A.d = add_deltas ? 1 : 0, A.dd = add_delta_deltas ? 1 : 0;
    for (int i = 0; i < 5; ++i) A.kd[i] = add_deltas ? delta_kernel[i] : 0.f, A.kdd[i] = add_delta_deltas ? delta_delta_kernel[i] : 0.f;
    const int hd = (A.d || A.dd) ? 2 : 0, hb = (A.k - 1) / 2;
    A.WA = (kJfShapeTile + 2 * (hb + hd)) | 1;
    A.WB = (kJfShapeTile + 2 * hd) | 1;
    const size_t lds = sizeof(float) * (size_t)M * (A.WA + (taps ? A.WB : 0));
    const int rc = jf_lds_opt_in(jf_shape_kernel, lds);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    const dim3 grid((unsigned)((T_out + kJfShapeTile - 1) / kJfShapeTile), (unsigned)C, (unsigned)B);
    hipLaunchKernelGGL(jf_shape_kernel, grid, dim3(256), lds, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int ptmi_je_feature_tail(const float* x, int64_t B, int32_t C, int32_t M, int64_t T, const float* mean, const float* rstd,
                         int64_t stat_stride_c, int64_t stat_stride_f, int32_t has_clamp, float clamp, const float* ipd_cos,
                         const float* ipd_sin, int32_t n_pairs, const int32_t* partner, const float* lambda, const float* noise_scale,
                         const float* noise, const int32_t* time_onset, const int32_t* time_offset, int32_t n_time_masks,
                         const int32_t* freq_onset, const int32_t* freq_offset, int32_t n_freq_masks, const int32_t* seq_len, float* out,
                         ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !out || B < 0 || T < 0 || C < 1 || M < 1 || n_pairs < 0 || n_time_masks < 0 || n_freq_masks < 0, PTMI_E_INVALID);
    PTMI_RETURN_IF(n_pairs > 0 && (!ipd_cos || !ipd_sin), PTMI_E_INVALID);
    PTMI_RETURN_IF((partner == nullptr) != (lambda == nullptr) || (noise == nullptr) != (noise_scale == nullptr), PTMI_E_INVALID);
    PTMI_RETURN_IF((n_time_masks > 0 && (!time_onset || !time_offset)) || (n_freq_masks > 0 && (!freq_onset || !freq_offset)), PTMI_E_INVALID);
    PTMI_RETURN_IF(M > kJfMaxM || C > 3 * kJfMaxC || n_pairs > kJfMaxPairs || B > 65535 || T > 0x7fffffffLL / kJfMaxM, PTMI_E_UNSUPPORTED);
    if (B == 0 || T == 0) return PTMI_OK;
    JfTailArgs A{};
    A.x = x, A.mean = mean, A.rstd = rstd, A.ipd_cos = ipd_cos, A.ipd_sin = ipd_sin, A.lambda = lambda, A.noise_scale = noise_scale;
    A.noise = noise, A.partner = partner, A.seq = seq_len, A.t_on = time_onset, A.t_off = time_offset, A.f_on = freq_onset;
    A.f_off = freq_offset, A.out = out, A.T = T, A.mean_sc = stat_stride_c, A.mean_sf = stat_stride_f, A.B = (int)B, A.C = C, A.P = n_pairs;
    A.M = M, A.n_t = n_time_masks, A.n_f = n_freq_masks, A.has_clamp = has_clamp, A.clamp = clamp;
    const long long plane = (long long)M * T;
    const bool vec = plane % 4 == 0 && jf_aligned16(x) && jf_aligned16(out) && jf_aligned16(ipd_cos) && jf_aligned16(ipd_sin) && jf_aligned16(noise);
    const long long per_block = 256LL * (vec ? 4 : 1);
    const dim3 grid((unsigned)((plane + per_block - 1) / per_block), (unsigned)(C + 2 * n_pairs), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(jf_tail_kernel<4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), A);
    else
        hipLaunchKernelGGL(jf_tail_kernel<1>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

}  // extern "C"
