// The glue of padertorch/contrib/mk/modules/transformer.py around the fused attention (include/ptmi.h: ptmi_mk_*): the per-head query /
// key preparation between the projections and the scores, and the row norms of the pre-norm / post-norm blocks with the residual add.
// (The attention itself, with the additive float bias of :691-724, is the BIAS = true instantiation in attention.hip.)
//
// q/k preparation (MultiheadAttention.project :681-689 and forward :754-756).  The projection output is [B, T, H, dh] as it lies; a head
// row (b, t, h) is dh <= 128 consecutive floats and is owned by a 16-LANE GROUP: lane l holds the pairs p = l, l + 16, l + 32, l + 48
// (columns 2p, 2p + 1, one float2 each), so the rotary rotation of a pair stays inside a lane and a row's sum of squares is the lane's
// own terms ascending, then four xor steps 8, 4, 2, 1 - the order attention.hip uses for its row maxima.  A workgroup is 16 groups; the
// first `blocks0` workgroups of a launch work on q, the rest on k (Tq != Tk under cross attention), so one launch prepares both.
//   RMS       y = x rsqrt(mean(x^2) + eps) w[dh]                                  (nn.RMSNorm over dh)
//   rotation  z[2i] = y[2i] cos a - y[2i+1] sin a, z[2i+1] = y[2i+1] cos a + y[2i] sin a, a = (t + 1) theta[2i] in fp32, accurate
//             cosf / sinf (RoPE.forward :253-270: positions start at 1, theta is the module's buffer)
//   L2        o = z / max(||z||, 1e-12)                                          (F.normalize)
// each optional, in this order.  Saved for backward: the inverse RMS and the inverse L2 norm per row, only the ones in use.  The
// backward is one launch: a workgroup walks a slab of kQkSlabRows rows in 8 passes, recomputes the stages from x and the saved scalars
// (the rotation's transpose is the rotation by -a), writes dx and keeps its lanes' RMS-weight terms in fp64 registers, rows ascending;
// the 16 groups are then added through LDS in group order into ws[slab][dh] and colreduce adds the slabs (reduce.h's fixed order).
//
// Row norms (TransformerEncoderLayer.forward :1002-1023).  One WAVE per row of [rows, N], lanes stride the columns by 64; with a second
// operand the kernel writes s = a + res and y = norm(s) in one pass, so x + sublayer(x) followed by the next norm is one launch.
//   layer  (s - mean) rstd w + b, eps 1e-5 (nn.LayerNorm);  rms  s rsqrt(mean(s^2) + eps) w (nn.RMSNorm);  dyt  tanh(alpha s) w + b
// Statistics are fp64 wave sums.  Backward: one launch for ds (the incoming gradient of s itself is added in the same pass), the
// weight / bias gradients as slab column sums + colreduce like transformer_norm_colsum_kernel, and for dyt the scalar alpha gradient as
// one fp64 partial per workgroup (lanes ascending, wave_sum, waves in order), added by colreduce in slab order.
#include <math.h>

#include "reduce.h"

namespace ptmi {

constexpr int kQkMaxHead = 128;    // = kAtMaxHead: 4 pairs per lane
constexpr int kQkSlabRows = 128;   // rows per workgroup of the backward (8 passes of 16)
constexpr int kRnSlabRows = 256;   // rows per slab of the row norm's column sums
constexpr int kRnBlockRows = 32;   // rows per workgroup of the row norm's backward (8 per wave)

enum { kRnLayer = 0, kRnRms = 1, kRnDyt = 2 };

struct QkSide {
    const float* x;
    const float* g;
    const float* w;
    float* out;
    float* irms;
    float* il2;
    long long rows, T;
};

struct QkArgs {
    QkSide s[2];
    const float* theta;
    double* ws;
    long long blocks0;
    int H, dh, l2;
    float eps;
};

__device__ __forceinline__ float qk_row_sum(float v) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The lane's pairs of row `row` (zeros outside the row count and the head size).
__device__ __forceinline__ void qk_load(float (&v)[8], const float* __restrict__ base, long long row, bool live, int dh, int l) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = 2 * (l + 16 * m);
        float2 t = make_float2(0.f, 0.f);
        if (live && c < dh) t = *reinterpret_cast<const float2*>(base + row * dh + c);
        v[2 * m] = t.x, v[2 * m + 1] = t.y;
    }
}

__device__ __forceinline__ void qk_store(float* __restrict__ base, const float (&v)[8], long long row, bool live, int dh, int l) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = 2 * (l + 16 * m);
        if (live && c < dh) *reinterpret_cast<float2*>(base + row * dh + c) = make_float2(v[2 * m], v[2 * m + 1]);
    }
}

__device__ __forceinline__ float qk_sumsq(const float (&v)[8]) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += v[i] * v[i];
    return qk_row_sum(ss);
}

// cos / sin of the lane's pairs at position t (0-based): the angle is the fp32 product (t + 1) theta, as the reference's tensors form it.
__device__ __forceinline__ void qk_angles(float (&cs)[4], float (&sn)[4], const float* __restrict__ theta, long long t, int dh, int l) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = 2 * (l + 16 * m);
        const float a = c < dh ? (float)(t + 1) * theta[c] : 0.f;
        cs[m] = cosf(a), sn[m] = sinf(a);
    }
}

__global__ __launch_bounds__(256) void mk_qk_prep_forward_kernel(const QkArgs A) {
#pragma clang fp contract(off)
    const int which = (long long)blockIdx.x >= A.blocks0;
    const QkSide S = which ? A.s[1] : A.s[0];
    const long long row = ((long long)blockIdx.x - (which ? A.blocks0 : 0)) * 16 + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const bool live = row < S.rows;
    float v[8];
    qk_load(v, S.x, row, live, A.dh, l);
    if (S.w) {
        const float r = 1.f / sqrtf(qk_sumsq(v) / (float)A.dh + A.eps);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = 2 * (l + 16 * (i >> 1)) + (i & 1);
            v[i] = c < A.dh ? v[i] * r * S.w[c] : 0.f;
        }
        if (live && l == 0) S.irms[row] = r;
    }
    if (A.theta) {
        float cs[4], sn[4];
        qk_angles(cs, sn, A.theta, (row / A.H) % S.T, A.dh, l);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float y0 = v[2 * m], y1 = v[2 * m + 1];
            v[2 * m] = y0 * cs[m] - y1 * sn[m];
            v[2 * m + 1] = y1 * cs[m] + y0 * sn[m];
        }
    }
    if (A.l2) {
        const float inv = 1.f / fmaxf(sqrtf(qk_sumsq(v)), 1e-12f);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= inv;
        if (live && l == 0) S.il2[row] = inv;
    }
    qk_store(S.out, v, row, live, A.dh, l);
}

__global__ __launch_bounds__(256) void mk_qk_prep_backward_kernel(const QkArgs A) {
#pragma clang fp contract(off)
    __shared__ double red[16][kQkMaxHead];
    const int which = (long long)blockIdx.x >= A.blocks0;
    const QkSide S = which ? A.s[1] : A.s[0];
    const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const long long row0 = ((long long)blockIdx.x - (which ? A.blocks0 : 0)) * kQkSlabRows;
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.;
    for (int pass = 0; pass < kQkSlabRows / 16; ++pass) {
        const long long row = row0 + pass * 16 + grp;
        const bool live = row < S.rows;
        float x[8], g[8], w[8], z[8];
        qk_load(x, S.x, row, live, A.dh, l);
        qk_load(g, S.g, row, live, A.dh, l);
        float r = 0.f;
        if (S.w) {
            r = live ? S.irms[row] : 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = 2 * (l + 16 * (i >> 1)) + (i & 1);
                w[i] = c < A.dh ? S.w[c] : 0.f;
                z[i] = x[i] * r * w[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) z[i] = x[i];
        }
        float cs[4], sn[4];
        if (A.theta) {
            qk_angles(cs, sn, A.theta, (row / A.H) % S.T, A.dh, l);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float y0 = z[2 * m], y1 = z[2 * m + 1];
                z[2 * m] = y0 * cs[m] - y1 * sn[m];
                z[2 * m + 1] = y1 * cs[m] + y0 * sn[m];
            }
        }
        if (A.l2) {                                         // o = z inv: dz = inv (g - o (g . o)); behind the clamp dz = g inv
            const float inv = live ? S.il2[row] : 0.f;
            float dot = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) dot += g[i] * (z[i] * inv);
            dot = qk_row_sum(dot);
            const bool clamped = !(inv < 1e12f);
#pragma unroll
            for (int i = 0; i < 8; ++i) g[i] = clamped ? g[i] * inv : inv * (g[i] - (z[i] * inv) * dot);
        }
        if (A.theta) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float g0 = g[2 * m], g1 = g[2 * m + 1];
                g[2 * m] = g0 * cs[m] + g1 * sn[m];
                g[2 * m + 1] = g1 * cs[m] - g0 * sn[m];
            }
        }
        if (S.w) {                                          // y = x r w, r = (mean(x^2) + eps)^-1/2: dx = r w g - x r^3 / dh sum(g w x)
            float dot = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) dot += g[i] * w[i] * x[i];
            dot = qk_row_sum(dot) * (r * r * r / (float)A.dh);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                acc[i] += (double)g[i] * (double)(x[i] * r);
                g[i] = r * w[i] * g[i] - x[i] * dot;
            }
        }
        qk_store(S.out, g, row, live, A.dh, l);
    }
    if (S.w) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[grp][2 * (l + 16 * (i >> 1)) + (i & 1)] = acc[i];
        __syncthreads();
        if ((int)threadIdx.x < A.dh) {
            double s = 0.;
            for (int gi = 0; gi < 16; ++gi) s += red[gi][threadIdx.x];
            A.ws[(long long)blockIdx.x * A.dh + threadIdx.x] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ row norms
struct RnArgs {
    const float *a, *res, *w, *b, *alpha, *gy, *gs, *stats_in;
    float *s, *y, *stats, *ds;
    double* ws;
    long long rows;
    int N, kind;
    float eps;
};

__global__ __launch_bounds__(256) void mk_row_norm_forward_kernel(const RnArgs A) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, N = A.N;
    if (row >= A.rows) return;
    const float* __restrict__ ar = A.a + row * N;
    const float* __restrict__ rr = A.res ? A.res + row * N : nullptr;
    float mean = 0.f, rstd = 0.f;
    if (A.kind != kRnDyt) {
        double m = 0.;
        if (A.kind == kRnLayer) {
            double s1 = 0.;
            for (int n = lane; n < N; n += 64) s1 += (double)(rr ? ar[n] + rr[n] : ar[n]);
            m = wave_sum(s1) / (double)N;
        }
        double s2 = 0.;
        for (int n = lane; n < N; n += 64) {
            const double d = (double)(rr ? ar[n] + rr[n] : ar[n]) - m;
            s2 += d * d;
        }
        mean = (float)m, rstd = (float)(1. / sqrt(wave_sum(s2) / (double)N + (double)A.eps));
        if (lane == 0) A.stats[2 * row] = mean, A.stats[2 * row + 1] = rstd;
    }
    const float alpha = A.kind == kRnDyt ? A.alpha[0] : 0.f;
    for (int n = lane; n < N; n += 64) {
        const float v = rr ? ar[n] + rr[n] : ar[n];
        const float h = A.kind == kRnDyt ? tanhf(alpha * v) : (v - mean) * rstd;
        float o = A.w ? h * A.w[n] : h;
        if (A.b) o += A.b[n];
        A.y[row * N + n] = o;
        if (rr) A.s[row * N + n] = v;
    }
}

// ds = gs + the norm's adjoint in gy.  layer / rms: rstd (gy w - c1 - xhat c2), c1 = mean(gy w) (0 for rms), c2 = mean(gy w xhat);
// dyt: gy w (1 - t^2) alpha, and the workgroup's share of d alpha = sum gy w (1 - t^2) s.
__global__ __launch_bounds__(256) void mk_row_norm_backward_kernel(const RnArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, N = A.N;
    const float alpha = A.kind == kRnDyt ? A.alpha[0] : 0.f;
    double da[1] = {0.};
    for (int it = 0; it < kRnBlockRows / 4; ++it) {
        const long long row = (long long)blockIdx.x * kRnBlockRows + it * 4 + wave;
        if (row >= A.rows) break;
        const float* __restrict__ sr = A.a + row * N;
        const float* __restrict__ gr = A.gy + row * N;
        float mean = 0.f, rstd = 0.f, c1 = 0.f, c2 = 0.f;
        if (A.kind != kRnDyt) {
            mean = A.stats_in[2 * row], rstd = A.stats_in[2 * row + 1];
            double s1 = 0., s2 = 0.;
            for (int n = lane; n < N; n += 64) {
                const float g = A.w ? gr[n] * A.w[n] : gr[n];
                s1 += (double)g;
                s2 += (double)g * (double)((sr[n] - mean) * rstd);
            }
            c1 = A.kind == kRnLayer ? (float)(wave_sum(s1) / (double)N) : 0.f;
            c2 = (float)(wave_sum(s2) / (double)N);
        }
        for (int n = lane; n < N; n += 64) {
            const float g = A.w ? gr[n] * A.w[n] : gr[n];
            float o;
            if (A.kind == kRnDyt) {
                const float t = tanhf(alpha * sr[n]);
                const float u = g * (1.f - t * t);
                o = u * alpha;
                da[0] += (double)u * (double)sr[n];
            } else {
                const float xh = (sr[n] - mean) * rstd;
                o = rstd * fmaf(-xh, c2, g - c1);
            }
            A.ds[row * N + n] = A.gs ? o + A.gs[row * N + n] : o;
        }
    }
    if (A.kind == kRnDyt) {
        block_sums(da);
        if (threadIdx.x == 0) A.ws[blockIdx.x] = da[0];
    }
}

// ws[slab][c] = sum over the slab's rows of gy h (h = xhat, or tanh(alpha s)), ws[slab][N + c] = ... of gy; the layout and order of
// transformer_norm_colsum_kernel.
__global__ __launch_bounds__(256) void mk_row_norm_colsum_kernel(const RnArgs A) {
    __shared__ double red[4][64][2];
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6, N = A.N;
    const int c = blockIdx.x * 64 + cx;
    const long long r0 = (long long)blockIdx.y * kRnSlabRows, r1 = min(r0 + (long long)kRnSlabRows, A.rows);
    const float alpha = A.kind == kRnDyt ? A.alpha[0] : 0.f;
    double s1 = 0., s2 = 0.;
    if (c < N)
        for (long long row = r0 + g; row < r1; row += 4) {
            const float gv = A.gy[row * N + c], sv = A.a[row * N + c];
            const float h = A.kind == kRnDyt ? tanhf(alpha * sv) : (sv - A.stats_in[2 * row]) * A.stats_in[2 * row + 1];
            s1 += (double)gv * (double)h;
            s2 += (double)gv;
        }
    red[g][cx][0] = s1, red[g][cx][1] = s2;
    __syncthreads();
    if (g == 0 && c < N) {
        A.ws[blockIdx.y * 2LL * N + c] = ((red[0][cx][0] + red[1][cx][0]) + red[2][cx][0]) + red[3][cx][0];
        A.ws[blockIdx.y * 2LL * N + N + c] = ((red[0][cx][1] + red[1][cx][1]) + red[2][cx][1]) + red[3][cx][1];
    }
}

static int qk_shape(int64_t B, int64_t Tq, int64_t Tk, int32_t H, int32_t dh, long long per_block) {
    PTMI_RETURN_IF(B < 1 || Tq < 1 || Tk < 0 || H < 1 || dh < 2 || (dh & 1), PTMI_E_INVALID);
    PTMI_RETURN_IF(dh > kQkMaxHead, PTMI_E_UNSUPPORTED);
    const long long rows = B * (Tq + Tk) * H;
    PTMI_RETURN_IF(rows / per_block + 2 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    return PTMI_OK;
}

static long long rn_colsum_slabs(long long rows) { return (rows + kRnSlabRows - 1) / kRnSlabRows; }
static long long rn_blocks(long long rows) { return (rows + kRnBlockRows - 1) / kRnBlockRows; }

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_mk_qk_prep_forward(const float* q, const float* k, const float* wq, const float* wk, const float* theta, int64_t B, int64_t Tq,
                            int64_t Tk, int32_t H, int32_t dh, float eps, int32_t l2, float* q_out, float* k_out, float* q_irms,
                            float* k_irms, float* q_il2, float* k_il2, ptmi_stream_t stream) {
    const bool has_k = Tk > 0;
    PTMI_RETURN_IF(!q || !q_out || (has_k && (!k || !k_out)) || (wq && !q_irms) || (has_k && !wq != !wk) || (has_k && wk && !k_irms) ||
                       (l2 && (!q_il2 || (has_k && !k_il2))),
                   PTMI_E_INVALID);
    const int rc = qk_shape(B, Tq, Tk, H, dh, 16);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    QkArgs A = {};
    A.s[0] = QkSide{q, nullptr, wq, q_out, q_irms, q_il2, (long long)B * Tq * H, (long long)Tq};
    A.s[1] = QkSide{k, nullptr, wk, k_out, k_irms, k_il2, (long long)B * Tk * H, (long long)(has_k ? Tk : 1)};
    A.theta = theta, A.H = H, A.dh = dh, A.l2 = l2, A.eps = eps;
    A.blocks0 = (A.s[0].rows + 15) / 16;
    const long long blocks = A.blocks0 + (A.s[1].rows + 15) / 16;
    hipLaunchKernelGGL(mk_qk_prep_forward_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int64_t ptmi_mk_qk_prep_workspace_elems(int64_t B, int64_t Tq, int64_t Tk, int32_t H, int32_t dh) {
    return ((B * Tq * H + kQkSlabRows - 1) / kQkSlabRows + (B * Tk * H + kQkSlabRows - 1) / kQkSlabRows) * (int64_t)dh;
}

int ptmi_mk_qk_prep_backward(const float* gq, const float* gk, const float* q, const float* k, const float* wq, const float* wk,
                             const float* theta, const float* q_irms, const float* k_irms, const float* q_il2, const float* k_il2,
                             int64_t B, int64_t Tq, int64_t Tk, int32_t H, int32_t dh, int32_t l2, float* dq, float* dk, float* dwq,
                             float* dwk, double* workspace, ptmi_stream_t stream) {
    const bool has_k = Tk > 0;
    PTMI_RETURN_IF(!gq || !q || !dq || (has_k && (!gk || !k || !dk)) || (wq && (!q_irms || !dwq || !workspace)) || (has_k && !wq != !wk) ||
                       (has_k && wk && (!k_irms || !dwk)) || (l2 && (!q_il2 || (has_k && !k_il2))),
                   PTMI_E_INVALID);
    int rc = qk_shape(B, Tq, Tk, H, dh, kQkSlabRows);
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    QkArgs A = {};
    A.s[0] = QkSide{q, gq, wq, dq, const_cast<float*>(q_irms), const_cast<float*>(q_il2), (long long)B * Tq * H, (long long)Tq};
    A.s[1] = QkSide{k, gk, wk, dk, const_cast<float*>(k_irms), const_cast<float*>(k_il2), (long long)B * Tk * H, (long long)(has_k ? Tk : 1)};
    A.theta = theta, A.ws = workspace, A.H = H, A.dh = dh, A.l2 = l2;
    const long long slabs0 = (A.s[0].rows + kQkSlabRows - 1) / kQkSlabRows, slabs1 = (A.s[1].rows + kQkSlabRows - 1) / kQkSlabRows;
    A.blocks0 = slabs0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mk_qk_prep_backward_kernel, dim3((unsigned)(slabs0 + slabs1)), dim3(256), 0, st, A);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK || !wq, rc);
    rc = colreduce(workspace, slabs0, (long long)dh, StorePlain{dwq}, st);
    PTMI_RETURN_IF(rc != PTMI_OK || !has_k, rc);
    return colreduce(workspace + slabs0 * dh, slabs1, (long long)dh, StorePlain{dwk}, st);
}

int ptmi_mk_row_norm_forward(int32_t kind, const float* a, const float* res, const float* weight, const float* bias, const float* alpha,
                             int64_t rows, int32_t N, float eps, float* s, float* y, float* stats, ptmi_stream_t stream) {
    PTMI_RETURN_IF(kind < kRnLayer || kind > kRnDyt || !a || !y || (res && !s) || (kind == kRnDyt ? !alpha : !stats) || rows < 1 || N < 1 ||
                       (kind == kRnRms && bias),
                   PTMI_E_INVALID);
    PTMI_RETURN_IF((rows + 3) / 4 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    RnArgs A = {};
    A.a = a, A.res = res, A.w = weight, A.b = bias, A.alpha = alpha, A.s = s, A.y = y, A.stats = stats, A.rows = rows, A.N = N, A.kind = kind;
    A.eps = eps;
    hipLaunchKernelGGL(mk_row_norm_forward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

int64_t ptmi_mk_row_norm_workspace_elems(int64_t rows, int32_t N) { return rn_colsum_slabs(rows) * 2 * (int64_t)N + rn_blocks(rows); }

int ptmi_mk_row_norm_backward(int32_t kind, const float* gy, const float* gs, const float* s, const float* stats, const float* weight,
                              const float* alpha, int64_t rows, int32_t N, float* ds, float* dparams, float* dalpha, double* workspace,
                              ptmi_stream_t stream) {
    PTMI_RETURN_IF(kind < kRnLayer || kind > kRnDyt || !gy || !s || !ds || (kind == kRnDyt ? (!alpha || !dalpha) : !stats) || !workspace ||
                       rows < 1 || N < 1,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(rn_blocks(rows) > 0x7fffffffLL || rn_colsum_slabs(rows) > 65535, PTMI_E_UNSUPPORTED);
    RnArgs A = {};
    A.a = s, A.gy = gy, A.gs = gs, A.stats_in = stats, A.w = weight, A.alpha = alpha, A.ds = ds, A.rows = rows, A.N = N, A.kind = kind;
    const long long slabs = rn_colsum_slabs(rows), blocks = rn_blocks(rows);
    double* ws_alpha = workspace + slabs * 2 * N;
    A.ws = ws_alpha;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(mk_row_norm_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A);
    int rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    if (kind == kRnDyt) {
        rc = colreduce(ws_alpha, blocks, 1LL, StorePlain{dalpha}, st);
        PTMI_RETURN_IF(rc != PTMI_OK, rc);
    }
    PTMI_RETURN_IF(!dparams, PTMI_OK);
    A.ws = workspace;
    hipLaunchKernelGGL(mk_row_norm_colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)slabs), dim3(256), 0, st, A);
    rc = launch_status();
    PTMI_RETURN_IF(rc != PTMI_OK, rc);
    return colreduce(workspace, slabs, 2LL * N, StorePlain{dparams}, st);
}

}  // extern "C"
