// The sequence glue of padertorch/contrib/je/modules: the (b T, 1, len_b) sequence table of a padded batch, reverse_sequence
// (rnn.py:130-154) and the masked reductions over time of reduce.py (Sum, Mean, Max, TakeLast, AutoPool), forward and backward.
//
// A pooled tensor is read in place as [B, M, T, I] through four strides (M: the axes between the batch and the time axis, I: the axes
// behind it, each collapsed by the caller); a "row" is one (b, m, i).  Two thread maps: a wavefront per row (lanes over t: the time axis
// is the contiguous one) or a thread per row (neighbouring threads on neighbouring (m, i): time is strided).  The results are [B, M, I],
// the input gradient a fresh contiguous [B, M, T, I] written WHOLE (zeros behind the length: no fill launch).
//
// Sums are fp64 in one fixed order (reduce.h): a thread's elements ascending, then the butterfly of the wave.  d alpha of AutoPool sums
// over b and t: every row writes its fp64 partial to the workspace [B][C], colreduce_kernel adds the B slabs.  No atomics, no allocation,
// no synchronisation; lengths are device data, clipped to [0, T].
#include "reduce.h"

namespace ptmi {

enum { kPoolSum = 0, kPoolMean = 1, kPoolMax = 2, kPoolLast = 3, kPoolAuto = 4 };

struct PoolGeom {
    long long B, M, T, I;
    long long sb, sm, st, si;
};

__device__ __forceinline__ long long sq_len(const void* lengths, int is64, long long b, long long T) {
    if (!lengths) return T;
    const long long n = is64 ? static_cast<const long long*>(lengths)[b] : (long long)static_cast<const int*>(lengths)[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

__global__ __launch_bounds__(256) void seq_table_kernel(const void* lengths, int is64, int B, int T, int* table) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    table[3 * b] = b * T, table[3 * b + 1] = 1, table[3 * b + 2] = (int)sq_len(lengths, is64, b, T);
}

// out [B, T, F] contiguous from x [B, T, F] (any strides).  mode 0: out[b, t] = x[b, t] (a copy into the rows' layout); mode 1:
// reverse_sequence: out[b, t] = x[b, len_b - 1 - t] for t < len_b and x[b, (len_b - 1 - t) mod T] * 0 behind (the reference multiplies
// by the mask: a NaN or an infinity there stays NaN); mode 2: its backward: plain zeros behind the length.
__global__ __launch_bounds__(256) void seq_gather_kernel(const float* __restrict__ x, long long sb, long long st, long long sf,
                                                         const void* lengths, int is64, float* __restrict__ out, long long total,
                                                         long long T, long long F, int mode) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long f = i % F, bt = i / F, t = bt % T, b = bt / T;
    float v;
    if (mode == 0) {
        v = x[b * sb + t * st + f * sf];
    } else {
        const long long len = sq_len(lengths, is64, b, T);
        long long src = len - 1 - t;
        if (t < len) {
            v = x[b * sb + src * st + f * sf];
        } else if (mode == 1) {
            src = ((src % T) + T) % T;
            v = x[b * sb + src * st + f * sf] * 0.f;
        } else {
            v = 0.f;
        }
    }
    out[i] = v;
}

template <bool WAVE>
__device__ __forceinline__ double sq_sum(double v) {
    if constexpr (WAVE) return wave_sum(v);
    return v;
}

// a is better than b: larger, a NaN beats every number (torch.max propagates NaN), the earlier position wins a tie
__device__ __forceinline__ bool sq_better(float a, long long ia, float b, long long ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ia < ib);
    return a > b || (a == b && ia < ib);
}

template <bool WAVE>
__device__ __forceinline__ void sq_max(float& v, long long& idx) {
    if constexpr (WAVE) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const long long oi = __shfl_xor(idx, o, 64);
            if (sq_better(ov, oi, v, idx)) v = ov, idx = oi;
        }
    }
}

template <bool WAVE>
__device__ __forceinline__ bool sq_row(const PoolGeom& G, long long& rowid, int& lane, long long& b, long long& m, long long& i) {
    rowid = WAVE ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x * 256 + threadIdx.x;
    lane = WAVE ? (threadIdx.x & 63) : 0;
    if (rowid >= G.B * G.M * G.I) return false;
    i = rowid % G.I;
    m = (rowid / G.I) % G.M;
    b = rowid / (G.I * G.M);
    return true;
}

// max over t < len of alpha x and the sum of exp(alpha x - max): the stable softmax's two row statistics
template <bool WAVE>
__device__ __forceinline__ void sq_softmax_stats(const float* __restrict__ xr, long long st, long long len, int lane, float a, float& mx,
                                                 double& den) {
    constexpr int STEP = WAVE ? 64 : 1;
    mx = -INFINITY;
    for (long long t = lane; t < len; t += STEP) mx = fmaxf(mx, a * xr[t * st]);
    if constexpr (WAVE) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    double s = 0.;
    for (long long t = lane; t < len; t += STEP) s += (double)expf(a * xr[t * st] - mx);
    den = sq_sum<WAVE>(s);
}

template <bool WAVE>
__global__ __launch_bounds__(256) void seq_pool_forward_kernel(const float* __restrict__ x, const PoolGeom G, const void* lengths, int is64,
                                                               int mode, const float* __restrict__ alpha, float alpha0,
                                                               float* __restrict__ y, long long* __restrict__ index) {
    constexpr int STEP = WAVE ? 64 : 1;
    long long rowid, b, m, i;
    int lane;
    if (!sq_row<WAVE>(G, rowid, lane, b, m, i)) return;
    const float* __restrict__ xr = x + b * G.sb + m * G.sm + i * G.si;
    const long long T = G.T, len = sq_len(lengths, is64, b, T);
    float res = 0.f;
    if (mode == kPoolSum || mode == kPoolMean) {
        double s = 0.;
        for (long long t = lane; t < len; t += STEP) s += (double)xr[t * G.st];
        s = sq_sum<WAVE>(s);
        if (mode == kPoolSum)
            res = (float)s;
        else if (lengths)
            res = (float)s / ((float)len + 1e-6f);          // reduce.py:42 as written
        else
            res = (float)(s / (double)T);
    } else if (mode == kPoolMax) {
        float v = -INFINITY;
        long long idx = 0x7fffffffffffffffLL;
        for (long long t = lane; t < len; t += STEP) {
            const float c = xr[t * G.st];
            if (sq_better(c, t, v, idx)) v = c, idx = t;
        }
        sq_max<WAVE>(v, idx);
        if (idx >= T) idx = 0;                              // no step at all: -inf at position 0, as max over a row of -inf
        res = v;
        if (lane == 0) index[rowid] = idx;
    } else if (mode == kPoolLast) {
        long long t = len - 1;
        if (t < 0) t = T - 1;                               // (index -1 of the reference's gather)
        res = xr[t * G.st];
    } else {
        const float a = alpha ? alpha[m] : alpha0;
        float mx;
        double den;
        sq_softmax_stats<WAVE>(xr, G.st, len, lane, a, mx, den);
        double num = 0.;
        for (long long t = lane; t < len; t += STEP) {
            const float c = xr[t * G.st];
            num += (double)expf(a * c - mx) * (double)c;
        }
        num = sq_sum<WAVE>(num);
        res = (float)(num / den);                           // no step: 0 / 0 = NaN as in the reference
    }
    if (lane == 0) y[rowid] = res;
}

// dx [B, M, T, I] contiguous, every element written.  sum: g below the length; mean: g / (len + 1e-6) (no lengths: g / T); max and last:
// g at the saved / the last position; autopool: g w_t (1 + alpha (x_t - y)) with w recomputed, and the row's part of d alpha, g (sum_t w_t
// x_t^2 - y^2), to ws[rowid] (ws null: not asked for).
template <bool WAVE>
__global__ __launch_bounds__(256) void seq_pool_backward_kernel(const float* __restrict__ x, const PoolGeom G, const void* lengths, int is64,
                                                                int mode, const float* __restrict__ alpha, float alpha0,
                                                                const float* __restrict__ g, const float* __restrict__ y,
                                                                const long long* __restrict__ index, float* __restrict__ dx,
                                                                double* __restrict__ ws) {
    constexpr int STEP = WAVE ? 64 : 1;
    long long rowid, b, m, i;
    int lane;
    if (!sq_row<WAVE>(G, rowid, lane, b, m, i)) return;
    const long long T = G.T, len = sq_len(lengths, is64, b, T);
    float* __restrict__ dr = dx + ((b * G.M + m) * T) * G.I + i;
    const float gv = g[rowid];
    if (mode == kPoolSum || mode == kPoolMean) {
        float v = gv;
        if (mode == kPoolMean) v = lengths ? gv / ((float)len + 1e-6f) : (float)((double)gv / (double)T);
        for (long long t = lane; t < T; t += STEP) dr[t * G.I] = t < len ? v : 0.f;
    } else if (mode == kPoolMax || mode == kPoolLast) {
        long long at = mode == kPoolMax ? index[rowid] : (len - 1 < 0 ? T - 1 : len - 1);
        for (long long t = lane; t < T; t += STEP) dr[t * G.I] = t == at ? gv : 0.f;
    } else {
        const float* __restrict__ xr = x + b * G.sb + m * G.sm + i * G.si;
        const float a = alpha ? alpha[m] : alpha0;
        const float yv = y[rowid];
        float mx;
        double den;
        sq_softmax_stats<WAVE>(xr, G.st, len, lane, a, mx, den);
        const float rden = (float)(1. / den);
        double s2 = 0.;
        for (long long t = lane; t < T; t += STEP) {
            float v = 0.f;
            if (t < len) {
                const float c = xr[t * G.st];
                const float w = expf(a * c - mx) * rden;
                v = gv * w * (1.f + a * (c - yv));
                s2 += (double)w * (double)c * (double)c;
            }
            dr[t * G.I] = v;
        }
        if (ws) {
            s2 = sq_sum<WAVE>(s2);
            if (lane == 0) ws[rowid] = (double)gv * (s2 - (double)yv * (double)yv);
        }
    }
}

static bool sq_geom(const int64_t* dims, const int64_t* strides, PoolGeom& G) {
    if (!dims || !strides) return false;
    G.B = dims[0], G.M = dims[1], G.T = dims[2], G.I = dims[3];
    G.sb = strides[0], G.sm = strides[1], G.st = strides[2], G.si = strides[3];
    return G.B >= 1 && G.M >= 1 && G.T >= 1 && G.I >= 1;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_seq_table(const void* lengths, int32_t lengths_int64, int32_t B, int32_t T, int32_t* table, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!table || B < 1 || T < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((long long)B * T > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(seq_table_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), lengths,
                       lengths_int64, B, T, table);
    return launch_status();
}

int ptmi_seq_gather(const float* x, const int64_t* x_strides, const void* lengths, int32_t lengths_int64, float* out, int64_t B, int64_t T,
                    int64_t F, int32_t mode, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !x_strides || !out || B < 1 || T < 1 || F < 1 || mode < 0 || mode > 2, PTMI_E_INVALID);
    const long long total = (long long)B * T * F;
    PTMI_RETURN_IF((total + 255) / 256 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(seq_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       (long long)x_strides[0], (long long)x_strides[1], (long long)x_strides[2], lengths, lengths_int64, out, total,
                       (long long)T, (long long)F, mode);
    return launch_status();
}

int ptmi_seq_pool_forward(const float* x, const int64_t* dims, const int64_t* strides, const void* lengths, int32_t lengths_int64,
                          int32_t mode, const float* alpha, float alpha0, float* y, int64_t* index, int32_t wave_per_row,
                          ptmi_stream_t stream) {
    PoolGeom G;
    PTMI_RETURN_IF(!x || !y || !sq_geom(dims, strides, G) || mode < kPoolSum || mode > kPoolAuto, PTMI_E_INVALID);
    PTMI_RETURN_IF(mode == kPoolMax && !index, PTMI_E_INVALID);
    PTMI_RETURN_IF(alpha && G.I != 1, PTMI_E_INVALID);
    const long long rows = G.B * G.M * G.I;
    const long long per = wave_per_row ? 4 : 256, blocks = (rows + per - 1) / per;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (wave_per_row)
        hipLaunchKernelGGL((seq_pool_forward_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, x, G, lengths, lengths_int64, mode,
                           alpha, alpha0, y, reinterpret_cast<long long*>(index));
    else
        hipLaunchKernelGGL((seq_pool_forward_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, x, G, lengths, lengths_int64, mode,
                           alpha, alpha0, y, reinterpret_cast<long long*>(index));
    return launch_status();
}

int ptmi_seq_pool_backward(const float* x, const int64_t* dims, const int64_t* strides, const void* lengths, int32_t lengths_int64,
                           int32_t mode, const float* alpha, float alpha0, const float* g, const float* y, const int64_t* index,
                           float* dx, double* workspace, float* dalpha, int32_t wave_per_row, ptmi_stream_t stream) {
    PoolGeom G;
    PTMI_RETURN_IF(!g || !dx || !sq_geom(dims, strides, G) || mode < kPoolSum || mode > kPoolAuto, PTMI_E_INVALID);
    PTMI_RETURN_IF(mode == kPoolMax && !index, PTMI_E_INVALID);
    PTMI_RETURN_IF(mode == kPoolAuto && (!x || !y), PTMI_E_INVALID);
    PTMI_RETURN_IF((dalpha != nullptr) != (workspace != nullptr) || (dalpha && (mode != kPoolAuto || !alpha || G.I != 1)), PTMI_E_INVALID);
    const long long rows = G.B * G.M * G.I;
    const long long per = wave_per_row ? 4 : 256, blocks = (rows + per - 1) / per;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (wave_per_row)
        hipLaunchKernelGGL((seq_pool_backward_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, x, G, lengths, lengths_int64, mode,
                           alpha, alpha0, g, y, reinterpret_cast<const long long*>(index), dx, workspace);
    else
        hipLaunchKernelGGL((seq_pool_backward_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, x, G, lengths, lengths_int64, mode,
                           alpha, alpha0, g, y, reinterpret_cast<const long long*>(index), dx, workspace);
    int rc = launch_status();
    if (rc || !dalpha) return rc;
    return colreduce(workspace, G.B, G.M, StorePlain{dalpha}, st);          // ws [B][C]: the B slabs of every class
}

}  // extern "C"
