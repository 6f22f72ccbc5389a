// Permutation-invariant training loss (MSE and ideal-phase-sensitive variants) for gfx950.
//
// Replaces padertorch/ops/losses/source_separation.py:34-124 (pit_loss, loss_fn = mse_loss: K!
// index_select copies + K! mse kernels + stack + min) and the per-example python loop of
// padertorch/contrib/examples/source_separation/pit/model.py:117-140 with
//   1. ONE streaming pass over mask / observation / target / cos-phase that accumulates the
//      K x K pairwise sums of squared errors of every example (HBM-bound: 7196 B per frame at
//      K=2, F=257; fp32 partials per thread, wave shuffles (reduce.h's wave_sum) + LDS across the 4 waves, fp64 from the
//      workgroup partial upwards, fixed reduction order -> bitwise reproducible),
//   2. a tiny kernel that walks the K! permutations in itertools order on the K x K matrix (first
//      minimum wins, like torch.min) and forms the batch means,
//   3. a streaming backward that scatters 2 (est - tgt_perm) / n for the winning permutation.
#include "reduce.h"

namespace ptmi {

constexpr int kTChunk = 8;   // frames per workgroup in the streaming kernels
constexpr int kMaxK = 8;     // 8! = 40320 permutations is the most the assign kernel walks

struct PitArgs {
    const float* est;
    const float* obs;
    const float* tgt;
    const float* scl;
    const int32_t* row_frames;
    long long t_len;
    long long est_bs, est_ts, obs_bs, obs_ts, tgt_bs, tgt_ts;   // element strides of (b, t)
    int K, F, nvar, nchunks;
};

// partial[b, chunk, v, i, j] (fp64) <- sum over the chunk's (t, f) of (est_i - tgt^v_j)^2
template <int K>
__global__ __launch_bounds__(256) void pit_pairwise_kernel(const PitArgs A, double* __restrict__ partial) {
    const int b = blockIdx.x / A.nchunks;
    const int c = blockIdx.x - b * A.nchunks;
    const long long T_b = A.row_frames ? (long long)A.row_frames[b] : A.t_len;
    const long long t0 = (long long)c * kTChunk;
    long long t1 = t0 + kTChunk;
    if (t1 > T_b) t1 = T_b;
    const int F = A.F;
    const int nvar = A.nvar;

    float acc[2][K][K];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) acc[v][i][j] = 0.f;

    const long long n = (t1 > t0) ? (t1 - t0) * F : 0;
    for (long long idx = threadIdx.x; idx < n; idx += 256) {
        const long long tt = idx / F;
        const int f = (int)(idx - tt * F);
        const long long t = t0 + tt;
        const float o = A.obs ? A.obs[b * A.obs_bs + t * A.obs_ts + f] : 1.f;
        const float* __restrict__ er = A.est + b * A.est_bs + t * A.est_ts + f;
        const long long toff = b * A.tgt_bs + t * A.tgt_ts + f;
        float e[K], g[K], h[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            e[i] = er[i * F] * o;
            g[i] = A.tgt[toff + i * F];
            h[i] = A.scl ? g[i] * A.scl[toff + i * F] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float d0 = e[i] - g[j];
                acc[0][i][j] += d0 * d0;
                const float d1 = e[i] - h[j];
                acc[1][i][j] += d1 * d1;
            }
    }

    __shared__ float red[4][2 * K * K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float s = wave_sum(acc[v][i][j]);
                if (lane == 0) red[wave][(v * K + i) * K + j] = s;
            }
    __syncthreads();
    if (threadIdx.x < nvar * K * K) {
        const double s = (double)red[0][threadIdx.x] + (double)red[1][threadIdx.x] +
                         (double)red[2][threadIdx.x] + (double)red[3][threadIdx.x];
        partial[((long long)b * A.nchunks + c) * (nvar * K * K) + threadIdx.x] = s;
    }
}

// Any K: one (i, j) pair per blockIdx.y.
__global__ __launch_bounds__(256) void pit_pairwise_generic_kernel(const PitArgs A, double* __restrict__ partial) {
    const int K = A.K, F = A.F;
    const int b = blockIdx.x / A.nchunks;
    const int c = blockIdx.x - b * A.nchunks;
    const int i = blockIdx.y / K, j = blockIdx.y - i * K;
    const long long T_b = A.row_frames ? (long long)A.row_frames[b] : A.t_len;
    const long long t0 = (long long)c * kTChunk;
    long long t1 = t0 + kTChunk;
    if (t1 > T_b) t1 = T_b;
    float a0 = 0.f, a1 = 0.f;
    const long long n = (t1 > t0) ? (t1 - t0) * F : 0;
    for (long long idx = threadIdx.x; idx < n; idx += 256) {
        const long long tt = idx / F;
        const int f = (int)(idx - tt * F);
        const long long t = t0 + tt;
        const float o = A.obs ? A.obs[b * A.obs_bs + t * A.obs_ts + f] : 1.f;
        const float e = A.est[b * A.est_bs + t * A.est_ts + (long long)i * F + f] * o;
        const long long off = b * A.tgt_bs + t * A.tgt_ts + (long long)j * F + f;
        const float g = A.tgt[off];
        const float h = A.scl ? g * A.scl[off] : 0.f;
        a0 += (e - g) * (e - g);
        a1 += (e - h) * (e - h);
    }
    __shared__ float red[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) {
        red[wave][0] = a0;
        red[wave][1] = a1;
    }
    __syncthreads();
    if (threadIdx.x < A.nvar) {
        const int v = threadIdx.x;
        const double s = (double)red[0][v] + (double)red[1][v] + (double)red[2][v] + (double)red[3][v];
        partial[((long long)b * A.nchunks + c) * (A.nvar * K * K) + (v * K + i) * K + j] = s;
    }
}

// sse[b, e] = sum_c partial[b, c, e] in chunk order (deterministic).
__global__ void pit_reduce_kernel(const double* __restrict__ partial, double* __restrict__ sse, int nchunks,
                                  int per, const int32_t* row_frames, long long t_len) {
    const int b = blockIdx.x;
    const long long T_b = row_frames ? (long long)row_frames[b] : t_len;
    const int used = (int)((T_b + kTChunk - 1) / kTChunk);
    for (int e = threadIdx.x; e < per; e += blockDim.x) {
        double s = 0.0;
        for (int c = 0; c < used && c < nchunks; ++c) s += partial[((long long)b * nchunks + c) * per + e];
        sse[(long long)b * per + e] = s;
    }
}

// One thread per (b, v): walk permutations in lexicographic (itertools) order.
__global__ void pit_assign_kernel(const double* __restrict__ sse, int batch, int nvar, int K, int F,
                                  long long t_len, const int32_t* row_frames, float* __restrict__ loss,
                                  int32_t* __restrict__ perm_out, float* ex_loss, float* scratch) {
    const int total = batch * nvar;
    for (int id = threadIdx.x; id < total; id += blockDim.x) {
        const int b = id / nvar;
        const double* m = sse + (long long)id * K * K;
        const long long T_b = row_frames ? (long long)row_frames[b] : t_len;
        const double denom = (double)T_b * K * F;
        int p[kMaxK], best[kMaxK];
        for (int j = 0; j < K; ++j) p[j] = best[j] = j;
        float best_loss = 0.f;
        bool first = true;
        while (true) {
            double s = 0.0;
            for (int j = 0; j < K; ++j) s += m[p[j] * K + j];     // estimate p[j] vs target j
            const float cand = (float)(s / denom);                 // fp32 candidates like the reference
            if (first || cand < best_loss) {
                best_loss = cand;
                for (int j = 0; j < K; ++j) best[j] = p[j];
                first = false;
            }
            // next lexicographic permutation
            int i = K - 2;
            while (i >= 0 && p[i] > p[i + 1]) --i;
            if (i < 0) break;
            int j = K - 1;
            while (p[j] < p[i]) --j;
            int tmp = p[i]; p[i] = p[j]; p[j] = tmp;
            for (int lo = i + 1, hi = K - 1; lo < hi; ++lo, --hi) { tmp = p[lo]; p[lo] = p[hi]; p[hi] = tmp; }
        }
        for (int j = 0; j < K; ++j) perm_out[(long long)id * K + j] = best[j];
        scratch[id] = best_loss;
        if (ex_loss) ex_loss[id] = best_loss;
    }
    __syncthreads();
    if ((int)threadIdx.x < nvar) {
        // torch.mean(torch.stack(per_example)) : fp32 data, sequential fp64 accumulation here
        double s = 0.0;
        for (int b = 0; b < batch; ++b) s += (double)scratch[b * nvar + threadIdx.x];
        loss[threadIdx.x] = (float)(s / batch);
    }
}

struct PitBwdArgs {
    const float* est;
    const float* obs;
    const float* tgt;
    const float* scl;
    const int32_t* perm;
    const float* gscale;
    const int32_t* row_frames;
    float* grad;
    long long batch, t_len;
    long long est_bs, est_ts, obs_bs, obs_ts, tgt_bs, tgt_ts;
    int K, F, nvar, nchunks;
};

__global__ __launch_bounds__(256) void pit_backward_kernel(const PitBwdArgs A) {
    const int b = blockIdx.x / A.nchunks;
    const int c = blockIdx.x - b * A.nchunks;
    const int K = A.K, F = A.F;
    const long long T_b = A.row_frames ? (long long)A.row_frames[b] : A.t_len;
    const long long t0 = (long long)c * kTChunk;
    long long t1 = t0 + kTChunk;
    if (t1 > A.t_len) t1 = A.t_len;
    // inverse permutation: for estimate i the target index j with perm[j] == i
    __shared__ int inv[2][32];
    __shared__ float coef[2];
    if (threadIdx.x < A.nvar * K) {
        const int v = threadIdx.x / K, j = threadIdx.x - v * K;
        inv[v][A.perm[((long long)b * A.nvar + v) * K + j]] = j;
    }
    if (threadIdx.x < A.nvar)
        coef[threadIdx.x] = T_b > 0 ? A.gscale[threadIdx.x] * (float)(2.0 / ((double)A.batch * T_b * K * F)) : 0.f;
    __syncthreads();
    const long long n = (t1 > t0) ? (t1 - t0) * K * F : 0;
    for (long long idx = threadIdx.x; idx < n; idx += 256) {
        const long long tk = idx / F;           // (t - t0) * K + i
        const int f = (int)(idx - tk * F);
        const long long tt = tk / K;
        const int i = (int)(tk - tt * K);
        const long long t = t0 + tt;
        const long long eoff = b * A.est_bs + t * A.est_ts + (long long)i * F + f;
        float gval = 0.f;
        if (t < T_b) {
            const float o = A.obs ? A.obs[b * A.obs_bs + t * A.obs_ts + f] : 1.f;
            const float e = A.est[eoff] * o;
            for (int v = 0; v < A.nvar; ++v) {
                const long long off = b * A.tgt_bs + t * A.tgt_ts + (long long)inv[v][i] * F + f;
                float g = A.tgt[off];
                if (v == 1) g *= A.scl[off];
                gval += coef[v] * (e - g);
            }
            gval *= o;
        }
        A.grad[eoff] = gval;
    }
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_pit_workspace_elems(int64_t batch, int64_t t_len, int32_t K, int32_t F) {
    (void)F;
    const int64_t nchunks = (t_len + kTChunk - 1) / kTChunk;
    return batch * nchunks * 2 * K * K + batch * 2;
}

int ptmi_pit_pairwise_sse(const float* est, const float* obs, const float* tgt, const float* tgt_scale,
                          int64_t batch, int64_t t_len, const int64_t* strides, int32_t K, int32_t F,
                          const int32_t* row_frames, double* workspace, double* sse,
                          ptmi_stream_t stream) {
    PTMI_RETURN_IF(!est || !tgt || !workspace || !sse || !strides, PTMI_E_INVALID);
    PTMI_RETURN_IF(batch < 0 || t_len < 0 || K < 1 || F < 1, PTMI_E_INVALID);
    if (batch == 0) return PTMI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PitArgs A{};
    A.est = est;
    A.obs = obs;
    A.tgt = tgt;
    A.scl = tgt_scale;
    A.row_frames = row_frames;
    A.t_len = t_len;
    A.est_bs = strides[0]; A.est_ts = strides[1];
    A.obs_bs = strides[2]; A.obs_ts = strides[3];
    A.tgt_bs = strides[4]; A.tgt_ts = strides[5];
    A.K = K;
    A.F = F;
    A.nvar = tgt_scale ? 2 : 1;
    A.nchunks = (int)((t_len + kTChunk - 1) / kTChunk);
    const int per = A.nvar * K * K;
    if (A.nchunks > 0) {
        const long long blocks = (long long)batch * A.nchunks;
        PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
        switch (K) {
            case 1: hipLaunchKernelGGL(pit_pairwise_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, A, workspace); break;
            case 2: hipLaunchKernelGGL(pit_pairwise_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, A, workspace); break;
            case 3: hipLaunchKernelGGL(pit_pairwise_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, st, A, workspace); break;
            case 4: hipLaunchKernelGGL(pit_pairwise_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, A, workspace); break;
            default:
                PTMI_RETURN_IF(K * K > 65535, PTMI_E_UNSUPPORTED);
                hipLaunchKernelGGL(pit_pairwise_generic_kernel, dim3((unsigned)blocks, (unsigned)(K * K)), dim3(256), 0, st, A, workspace);
        }
        int rc = launch_status();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(pit_reduce_kernel, dim3((unsigned)batch), dim3(64), 0, st, workspace, sse, A.nchunks, per,
                       row_frames, (long long)t_len);
    return launch_status();
}

int ptmi_pit_assign(const double* sse, int64_t batch, int32_t nvar, int32_t K, int32_t F, int64_t t_len,
                    const int32_t* row_frames, float* loss, int32_t* perm, float* ex_loss,
                    ptmi_stream_t stream) {
    PTMI_RETURN_IF(!sse || !loss || !perm, PTMI_E_INVALID);
    PTMI_RETURN_IF(batch < 1 || nvar < 1 || nvar > 2 || K < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(K > kMaxK, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the per-(b, v) fp32 candidates live in the caller's ex_loss when given, else in a
    // stream-ordered allocation freed right after the launch (no hidden persistent workspace).
    float* scratch = ex_loss;
    if (!scratch) {
        hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&scratch), sizeof(float) * batch * nvar, st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(pit_assign_kernel, dim3(1), dim3(256), 0, st, sse, (int)batch, (int)nvar, (int)K, (int)F,
                       (long long)t_len, row_frames, loss, perm, ex_loss, scratch);
    int rc = launch_status();
    if (!ex_loss) (void)hipFreeAsync(scratch, st);
    return rc;
}

int ptmi_pit_backward(const float* est, const float* obs, const float* tgt, const float* tgt_scale,
                      const int32_t* perm, const float* gscale, int64_t batch, int64_t t_len,
                      const int64_t* strides, int32_t K, int32_t F, int32_t nvar, const int32_t* row_frames,
                      float* grad, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!est || !tgt || !perm || !gscale || !grad || !strides, PTMI_E_INVALID);
    PTMI_RETURN_IF(nvar < 1 || nvar > 2 || (nvar == 2 && !tgt_scale) || K < 1 || K > 32, PTMI_E_INVALID);
    if (batch == 0 || t_len == 0) return PTMI_OK;
    PitBwdArgs A{};
    A.est = est;
    A.obs = obs;
    A.tgt = tgt;
    A.scl = tgt_scale;
    A.perm = perm;
    A.gscale = gscale;
    A.row_frames = row_frames;
    A.grad = grad;
    A.batch = batch;
    A.t_len = t_len;
    A.est_bs = strides[0]; A.est_ts = strides[1];
    A.obs_bs = strides[2]; A.obs_ts = strides[3];
    A.tgt_bs = strides[4]; A.tgt_ts = strides[5];
    A.K = K;
    A.F = F;
    A.nvar = nvar;
    A.nchunks = (int)((t_len + kTChunk - 1) / kTChunk);
    const long long blocks = (long long)batch * A.nchunks;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(pit_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), A);
    return launch_status();
}

}  // extern "C"
