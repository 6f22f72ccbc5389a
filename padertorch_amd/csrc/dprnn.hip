// The dual-path RNN separator (padertorch/modules/dual_path_rnn.py) between its GEMMs: the recurrence of one LSTM layer over a table
// of many short independent sequences, the layer norm + mask + residual behind a block's projection, segmentation and overlap-add.
//
// Layout: the chunked activation is [B, S, K, N] (channels last, chunk-major) and a "position" is a row (b, s, k) of it.  A sequence
// is (base row, step stride, step count): an intra-chunk sequence walks rows base + t, an inter-chunk sequence rows base + t K.
// Nothing is transposed.
//
// The recurrence: one workgroup owns kDpR = 4 sequences of one direction from their first step to their last.
// W_hh lives in the registers of the workgroup (4 HP threads x HP words, HP = H rounded up to 32 / 64 / 128), h travels between steps
// through LDS, c (forward) and dc (backward) stay in a register of the thread that owns (sequence, unit).  Products and sums are fp32
// FMAs: exact fp32 arithmetic.  No flag, no spin, no ordering between workgroups: a workgroup reads and writes only the rows of its own
// sequences.  H > 128 (4 H^2 words fit neither the registers nor the LDS of a workgroup) runs on two kernels of the same decomposition
// that stream W_hh from the L2 every step, up to H = 1536 (the LDS of a CU).
//
// Sums over rows (d gamma, d beta, bias gradients): fp64, per-slab partials in the caller's workspace, added by a second kernel in the
// fixed order that reduce.h defines: no atomics, bit-reproducible.  No allocation, no synchronisation: every launcher is capturable; chunk counts and
// sequence tables are device data.
#include <algorithm>

#include "lstm_common.h"
#include "reduce.h"

namespace ptmi {

constexpr int kDpR = 4;              // sequences per workgroup of the recurrence
constexpr int kDpSlabRows = 128;     // rows per workgroup of the column sums

typedef float f32x2 __attribute__((ext_vector_type(2)));

// The value of lane ^ 1 / lane ^ 2 inside a quad of lanes (DPP quad_perm [1, 0, 3, 2] / [2, 3, 0, 1]): no LDS traffic.
__device__ __forceinline__ float dp_quad_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dp_quad_xor2(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}

// The masked weight is this register pair from here on (without it the compiler keeps the raw loads and repeats the masking in the loop).
__device__ __forceinline__ void dp_pin(f32x2& v) { asm volatile("" : "+v"(v)); }
// The sums so far are complete here and no later LDS read starts before.
__device__ __forceinline__ void dp_fence(f32x2 (&acc)[2][4]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(acc[a][q])::"memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ------------------------------------------------------------------------------------------------ a. chunk counts and tables
// S_b = (len_b + (K - P) - 1) // P + 1 clipped to [0, S] (dual_path_rnn.py:146-149); no lengths: S.
__device__ __forceinline__ int dp_chunks(const void* lengths, int is64, int b, int S, int K, int P) {
    if (!lengths) return S;
    const long long n = is64 ? static_cast<const long long*>(lengths)[b] : (long long)static_cast<const int*>(lengths)[b];
    const long long a = n + (K - P) - 1;
    const long long q = a >= 0 ? a / P : -((-a + P - 1) / P);          // floor
    const long long sb = q + 1;
    return (int)(sb < 0 ? 0 : (sb > S ? S : sb));
}

// sb [B]; intra [B S][3] = (base, 1, s < S_b ? K : 0); inter [B K][3] = (base, K, S_b)
__global__ __launch_bounds__(256) void dprnn_tables_kernel(const void* lengths, int is64, int B, int S, int K, int P, int* sb,
                                                           int* intra, int* inter) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nintra = (long long)B * S, ninter = (long long)B * K;
    if (i < B) sb[i] = dp_chunks(lengths, is64, (int)i, S, K, P);
    if (i < nintra) {
        const int b = (int)(i / S), s = (int)(i % S);
        intra[3 * i] = (int)(i * K), intra[3 * i + 1] = 1, intra[3 * i + 2] = s < dp_chunks(lengths, is64, b, S, K, P) ? K : 0;
    }
    if (i < ninter) {
        const int b = (int)(i / K), k = (int)(i % K);
        inter[3 * i] = b * S * K + k, inter[3 * i + 1] = K, inter[3 * i + 2] = dp_chunks(lengths, is64, b, S, K, P);
    }
}

// ------------------------------------------------------------------------------------------------ b. the recurrence
struct DpLstmArgs {
    float* gates;            // [rows, D 4H]: forward in: x W_ih^T + b_ih, out: the activated gates (i, f, g, o); backward in: those,
                             //   out: d gates (pre-activation)
    const float* w_hh[2];    // [4H, H] per direction
    const float* b_hh[2];    // [4H] per direction (forward)
    float* h;                // [rows, D H]: forward out; backward in
    float* c;                // [rows, D H]: forward out; backward in
    const float* dh;         // [rows, D H]  (backward)
    float* hprev;            // [rows, D H]  (backward out): h of the step before, 0 at a first step and off the steps
    const int* table;        // [nseq][3]
    int nseq, H, D, cap;     // cap: rows base + t stride, t < cap, belong to the sequence; those from count on are zero-filled
};

struct DpSeq {
    int base, stride, count, cap;
};

__device__ __forceinline__ DpSeq dp_seq(const DpLstmArgs& A, int seq) {
    DpSeq s{0, 0, 0, 0};
    if (seq < A.nseq) {
        s.base = A.table[3 * seq], s.stride = A.table[3 * seq + 1], s.count = A.table[3 * seq + 2], s.cap = A.cap;
        s.count = s.count < 0 ? 0 : (s.count > A.cap ? A.cap : s.count);
    }
    return s;
}

// Row of processing step p of a sequence in direction d (the reverse direction starts at the sequence's own last step).
__device__ __forceinline__ long long dp_row(const DpSeq& s, int d, int p) {
    return (long long)s.base + (long long)(d ? s.count - 1 - p : p) * s.stride;
}

// Forward.  Thread (u, kq) = (tid / 4, tid % 4): holds W_hh[g H + u][k] for the four gates g and the quarter k in [kq HP/4, (kq+1) HP/4)
// (HP registers), multiplies them with h of the four sequences (one float4 per k from LDS, the same address for the 16 units of a
// quarter: a broadcast), adds the four quarters by two quad exchanges and then owns (sequence kq, unit u): gates, cell update, h.
// One barrier per step: h is double-buffered.
template <int HP>
__global__ __launch_bounds__(4 * HP) void dprnn_lstm_forward_kernel(const DpLstmArgs A) {
    constexpr int KQ = HP / 4;                 // k per quarter
    constexpr int LDQ = KQ * 4 + 4;            // words per quarter of sh (+ 4: the four quarters start on different banks)
    __shared__ __attribute__((aligned(16))) float sh[2][4 * LDQ];      // [buffer][kq][k][r]
    __shared__ DpSeq sseq[kDpR];
    const int tid = threadIdx.x, u = tid >> 2, kq = tid & 3, d = blockIdx.y, H = A.H;
    if (tid < kDpR) sseq[tid] = dp_seq(A, blockIdx.x * kDpR + tid);
    for (int i = tid; i < 2 * 4 * LDQ; i += 4 * HP) (&sh[0][0])[i] = 0.f;
    f32x2 w[2][KQ];                            // gates (i, f) and (g, o) in pairs: one packed FMA serves two gates
    const float* __restrict__ W = A.w_hh[d];
    const unsigned last = 4u * H * H - 1u;     // H <= 128: every index fits 32 bits
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int k = 0; k < KQ; ++k)
        {
            const bool ok = u < H && kq * KQ + k < H;          // (an unconditional load of a clamped 32-bit index: no branch per weight)
            const float v = W[min((unsigned)((g * H + u) * H + kq * KQ + k), last)];
            w[g >> 1][k][g & 1] = ok ? v : 0.f;
        }
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int k = 0; k < KQ; ++k) dp_pin(w[g][k]);
    float bias[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[g] = u < H ? A.b_hh[d][g * H + u] : 0.f;
    __syncthreads();
    const DpSeq me = sseq[kq];                 // the sequence whose cell (kq, u) this thread owns
    int maxT = 0;
#pragma unroll
    for (int r = 0; r < kDpR; ++r) maxT = max(maxT, sseq[r].count);
    const long long ldg = (long long)A.D * 4 * H, ldh = (long long)A.D * H;
    float c = 0.f;
    for (int t = 0; t < maxT; ++t) {
        const bool on = t < me.count && u < H;
        const long long row = dp_row(me, d, t);
        float gx[4] = {0.f, 0.f, 0.f, 0.f};
        if (on) {
#pragma unroll
            for (int g = 0; g < 4; ++g) gx[g] = A.gates[row * ldg + (long long)d * 4 * H + g * H + u];
        }
        const float* __restrict__ hq = &sh[t & 1][kq * LDQ];
        f32x2 acc[2][4];                       // [gate pair][sequence]
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[g][r] = f32x2{0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(hq + 4 * k);
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                acc[g][0] = __builtin_elementwise_fma(w[g][k], f32x2{hv.x, hv.x}, acc[g][0]);
                acc[g][1] = __builtin_elementwise_fma(w[g][k], f32x2{hv.y, hv.y}, acc[g][1]);
                acc[g][2] = __builtin_elementwise_fma(w[g][k], f32x2{hv.z, hv.z}, acc[g][2]);
                acc[g][3] = __builtin_elementwise_fma(w[g][k], f32x2{hv.w, hv.w}, acc[g][3]);
            }
        }
        // the four quarters of a quad, reduce-scatter: lane kq ends with the full sum of sequence kq.  First exchange (lane ^ 1): a lane
        // keeps the sequences of its own parity and hands the other two over; second (lane ^ 2): it keeps its own.
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const bool odd = kq & 1, high = kq & 2;
            const float s0 = acc[g >> 1][0][g & 1], s1 = acc[g >> 1][1][g & 1], s2 = acc[g >> 1][2][g & 1], s3 = acc[g >> 1][3][g & 1];
            const float lo = (odd ? s1 : s0) + dp_quad_xor1(odd ? s0 : s1);      // sequence (kq & 1)
            const float hi = (odd ? s3 : s2) + dp_quad_xor1(odd ? s2 : s3);      // sequence (kq & 1) + 2
            pre[g] = (high ? hi : lo) + dp_quad_xor2(high ? lo : hi);
        }
        if (on) {
            const float gi = sigmoidf_(gx[0] + bias[0] + pre[0]);
            const float gf = sigmoidf_(gx[1] + bias[1] + pre[1]);
            const float gg = tanhf_(gx[2] + bias[2] + pre[2]);
            const float go = sigmoidf_(gx[3] + bias[3] + pre[3]);
            c = gf * c + gi * gg;
            const float hh = go * tanhf_(c);
            float* __restrict__ gr = A.gates + row * ldg + (long long)d * 4 * H + u;
            gr[0] = gi, gr[H] = gf, gr[2 * H] = gg, gr[3 * H] = go;
            A.c[row * ldh + d * H + u] = c;
            A.h[row * ldh + d * H + u] = hh;
            sh[(t + 1) & 1][(u / KQ) * LDQ + (u % KQ) * 4 + kq] = hh;
        }
        __syncthreads();
    }
    // rows of the sequences that belong to no step: h = 0 (the projection behind reads every row)
    for (int r = 0; r < kDpR; ++r) {
        const DpSeq s = sseq[r];
        const int n = (s.cap - s.count) * H;
        for (int i = tid; i < n; i += 4 * HP) {
            const long long row = (long long)s.base + (long long)(s.count + i / H) * s.stride;
            A.h[row * ldh + d * H + i % H] = 0.f;
        }
    }
}

// Backward.  Two thread maps per step:
//   cell: thread (r, u) = (tid / HP, tid % HP) owns dc of (sequence r, unit u): reads the saved gates, c, the step's dh and the recurrent
//     part (16 partials from LDS), writes d gates to memory (in place) and to LDS, and h of the step before to hprev;
//   product: thread (jb, ug) = (tid / (HP/4), tid % (HP/4)) holds W_hh[j][4 ug + a] for a < 4 and the HP/4 gate columns j of block jb of
//     16 (HP registers) and writes its partial of dh_prev[r][4 ug + a] = sum_j dgates[r][j] W_hh[j][4 ug + a] to LDS.
template <int HP>
__global__ __launch_bounds__(4 * HP) void dprnn_lstm_backward_kernel(const DpLstmArgs A) {
    constexpr int JB = HP / 4;                 // gate columns per block (16 blocks)
    constexpr int LDJ = JB * 4 + 4;            // words per block of sdg
    __shared__ __attribute__((aligned(16))) float sdg[16 * LDJ];            // [jb][jj][r]
    __shared__ __attribute__((aligned(16))) float spart[16][kDpR][HP];      // [jb][r][u]
    __shared__ DpSeq sseq[kDpR];
    const int tid = threadIdx.x, d = blockIdx.y, H = A.H;
    const int r = tid / HP, u = tid % HP;      // cell map
    const int jb = tid / JB, ug = tid % JB;    // product map
    if (tid < kDpR) sseq[tid] = dp_seq(A, blockIdx.x * kDpR + tid);
    for (int i = tid; i < 16 * kDpR * HP; i += 4 * HP) (&spart[0][0][0])[i] = 0.f;
    f32x2 w[2][JB];                            // outputs (0, 1) and (2, 3) in pairs: one packed FMA serves two outputs
    const float* __restrict__ W = A.w_hh[d];
    const unsigned last = 4u * H * H - 1u;     // H <= 128: every index fits 32 bits
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
        // padded gate column jb JB + jj = g HP + unit
        const int jp = jb * JB + jj, g = jp / HP, ju = jp % HP;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bool ok = ju < H && 4 * ug + a < H;          // (an unconditional load of a clamped 32-bit index: no branch per weight)
            const float v = W[min((unsigned)((g * H + ju) * H + 4 * ug + a), last)];
            w[a >> 1][jj][a & 1] = ok ? v : 0.f;
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) dp_pin(w[a][jj]);
    __syncthreads();
    const DpSeq me = sseq[r];
    int maxT = 0;
#pragma unroll
    for (int q = 0; q < kDpR; ++q) maxT = max(maxT, sseq[q].count);
    const long long ldg = (long long)A.D * 4 * H, ldh = (long long)A.D * H;
    float dc = 0.f;
    for (int t = 0; t < maxT; ++t) {
        const bool on = t < me.count && u < H;
        const int p = me.count - 1 - t;        // processing step, last first
        float dgv[4] = {0.f, 0.f, 0.f, 0.f};
        if (on) {
            const long long row = dp_row(me, d, p);
            float* __restrict__ gr = A.gates + row * ldg + (long long)d * 4 * H + u;
            const float gi = gr[0], gf = gr[H], gg = gr[2 * H], go = gr[3 * H];
            const float cc = A.c[row * ldh + d * H + u];
            float cp = 0.f, hp = 0.f;
            if (p > 0) {
                const long long prow = dp_row(me, d, p - 1);
                cp = A.c[prow * ldh + d * H + u];
                hp = A.h[prow * ldh + d * H + u];
            }
            float dh = A.dh[row * ldh + d * H + u];
#pragma unroll
            for (int q = 0; q < 16; ++q) dh += spart[q][r][u];
            const float tc = tanhf_(cc);
            const float dcc = dc + dh * go * (1.f - tc * tc);
            dgv[0] = dcc * gg * gi * (1.f - gi);
            dgv[1] = dcc * cp * gf * (1.f - gf);
            dgv[2] = dcc * gi * (1.f - gg * gg);
            dgv[3] = dh * tc * go * (1.f - go);
            dc = dcc * gf;
            gr[0] = dgv[0], gr[H] = dgv[1], gr[2 * H] = dgv[2], gr[3 * H] = dgv[3];
            A.hprev[row * ldh + d * H + u] = hp;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int jp = g * HP + u;
            sdg[(jp / JB) * LDJ + (jp % JB) * 4 + r] = dgv[g];
        }
        __syncthreads();
        f32x2 acc[2][4];                       // [output pair][sequence]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[a][q] = f32x2{0.f, 0.f};
        const float* __restrict__ dq = &sdg[jb * LDJ];
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            if (jj % 8 == 0) dp_fence(acc);    // keeps the JB LDS reads from being hoisted in front of the FMAs all at once (registers)
            const f32x4 v = *reinterpret_cast<const f32x4*>(dq + 4 * jj);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                acc[a][0] = __builtin_elementwise_fma(w[a][jj], f32x2{v.x, v.x}, acc[a][0]);
                acc[a][1] = __builtin_elementwise_fma(w[a][jj], f32x2{v.y, v.y}, acc[a][1]);
                acc[a][2] = __builtin_elementwise_fma(w[a][jj], f32x2{v.z, v.z}, acc[a][2]);
                acc[a][3] = __builtin_elementwise_fma(w[a][jj], f32x2{v.w, v.w}, acc[a][3]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4*>(&spart[jb][q][4 * ug]) = f32x4{acc[0][q].x, acc[0][q].y, acc[1][q].x, acc[1][q].y};
        __syncthreads();
    }
    // rows that belong to no step: d gates = 0 and hprev = 0 (the weight-gradient GEMMs read every row)
    for (int q = 0; q < kDpR; ++q) {
        const DpSeq s = sseq[q];
        const int n = (s.cap - s.count) * 5 * H;
        for (int i = tid; i < n; i += 4 * HP) {
            const long long row = (long long)s.base + (long long)(s.count + i / (5 * H)) * s.stride;
            const int j = i % (5 * H);
            if (j < 4 * H)
                A.gates[row * ldg + (long long)d * 4 * H + j] = 0.f;
            else
                A.hprev[row * ldh + d * H + j - 4 * H] = 0.f;
        }
    }
}

// ---- H > 128: W_hh (4 H^2 words) exceeds the registers and the LDS of a workgroup, so these two kernels stream it from the L2 every
// step; the decomposition is the same (kDpR sequences per workgroup, h through LDS, no word waited for across workgroups).  256
// threads; thread tid owns the cells (r, u) = item / H, item % H for item = tid, tid + 256, ...: a cell keeps its thread from step to
// step, so its c is read back from the row the same thread wrote a step earlier, and its dc lives in an LDS word only it touches.
// What bounds H is the LDS of a CU: the backward kernel holds d gates, dh and dc of its kDpR sequences, 6 kDpR H words (160 KB:
// H <= 1706; kDpMaxStreamH leaves room).
constexpr int kDpMaxStreamH = 1536;

__global__ __launch_bounds__(256) void dprnn_lstm_forward_stream_kernel(const DpLstmArgs A) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];          // sh [2][kDpR][H]
    __shared__ DpSeq sseq[kDpR];
    const int tid = threadIdx.x, d = blockIdx.y, H = A.H;
    if (tid < kDpR) sseq[tid] = dp_seq(A, blockIdx.x * kDpR + tid);
    for (int i = tid; i < 2 * kDpR * H; i += 256) dyn[i] = 0.f;
    __syncthreads();
    int maxT = 0;
#pragma unroll
    for (int r = 0; r < kDpR; ++r) maxT = max(maxT, sseq[r].count);
    const float* __restrict__ W = A.w_hh[d];
    const float* __restrict__ bh = A.b_hh[d];
    const long long ldg = (long long)A.D * 4 * H, ldh = (long long)A.D * H;
    for (int t = 0; t < maxT; ++t) {
        const float* __restrict__ hin = dyn + (t & 1) * kDpR * H;
        float* __restrict__ hout = dyn + ((t + 1) & 1) * kDpR * H;
        for (int item = tid; item < kDpR * H; item += 256) {
            const int r = item / H, u = item % H;
            const DpSeq me = sseq[r];
            if (t >= me.count) continue;
            const long long row = dp_row(me, d, t);
            float* __restrict__ gr = A.gates + row * ldg + (long long)d * 4 * H + u;
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float* __restrict__ wr = W + ((long long)g * H + u) * H;
                float a = 0.f;
                for (int k = 0; k < H; ++k) a = fmaf(wr[k], hin[r * H + k], a);
                pre[g] = gr[g * H] + bh[g * H + u] + a;
            }
            const float gi = sigmoidf_(pre[0]), gf = sigmoidf_(pre[1]), gg = tanhf_(pre[2]), go = sigmoidf_(pre[3]);
            const float cp = t > 0 ? A.c[dp_row(me, d, t - 1) * ldh + d * H + u] : 0.f;      // this thread's own store of the step before
            const float c = gf * cp + gi * gg;
            const float hh = go * tanhf_(c);
            gr[0] = gi, gr[H] = gf, gr[2 * H] = gg, gr[3 * H] = go;
            A.c[row * ldh + d * H + u] = c;
            A.h[row * ldh + d * H + u] = hh;
            hout[r * H + u] = hh;
        }
        __syncthreads();
    }
    for (int r = 0; r < kDpR; ++r) {
        const DpSeq s = sseq[r];
        const int n = (s.cap - s.count) * H;
        for (int i = tid; i < n; i += 256) {
            const long long row = (long long)s.base + (long long)(s.count + i / H) * s.stride;
            A.h[row * ldh + d * H + i % H] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void dprnn_lstm_backward_stream_kernel(const DpLstmArgs A) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];          // sdg [kDpR][4 H] | sdh [kDpR][H] | sdc [kDpR][H]
    __shared__ DpSeq sseq[kDpR];
    const int tid = threadIdx.x, d = blockIdx.y, H = A.H;
    float* __restrict__ sdg = dyn;
    float* __restrict__ sdh = dyn + kDpR * 4 * H;
    float* __restrict__ sdc = dyn + kDpR * 5 * H;
    if (tid < kDpR) sseq[tid] = dp_seq(A, blockIdx.x * kDpR + tid);
    for (int i = tid; i < kDpR * 6 * H; i += 256) dyn[i] = 0.f;
    __syncthreads();
    int maxT = 0;
#pragma unroll
    for (int r = 0; r < kDpR; ++r) maxT = max(maxT, sseq[r].count);
    const float* __restrict__ W = A.w_hh[d];
    const long long ldg = (long long)A.D * 4 * H, ldh = (long long)A.D * H;
    for (int t = 0; t < maxT; ++t) {
        for (int item = tid; item < kDpR * H; item += 256) {
            const int r = item / H, u = item % H;
            const DpSeq me = sseq[r];
            float dgv[4] = {0.f, 0.f, 0.f, 0.f};
            if (t < me.count) {
                const int p = me.count - 1 - t;
                const long long row = dp_row(me, d, p);
                float* __restrict__ gr = A.gates + row * ldg + (long long)d * 4 * H + u;
                const float gi = gr[0], gf = gr[H], gg = gr[2 * H], go = gr[3 * H];
                const float cc = A.c[row * ldh + d * H + u];
                float cp = 0.f, hp = 0.f;
                if (p > 0) {
                    const long long prow = dp_row(me, d, p - 1);
                    cp = A.c[prow * ldh + d * H + u];
                    hp = A.h[prow * ldh + d * H + u];
                }
                const float dh = A.dh[row * ldh + d * H + u] + sdh[item];
                const float tc = tanhf_(cc);
                const float dcc = sdc[item] + dh * go * (1.f - tc * tc);
                dgv[0] = dcc * gg * gi * (1.f - gi);
                dgv[1] = dcc * cp * gf * (1.f - gf);
                dgv[2] = dcc * gi * (1.f - gg * gg);
                dgv[3] = dh * tc * go * (1.f - go);
                sdc[item] = dcc * gf;
                gr[0] = dgv[0], gr[H] = dgv[1], gr[2 * H] = dgv[2], gr[3 * H] = dgv[3];
                A.hprev[row * ldh + d * H + u] = hp;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) sdg[r * 4 * H + g * H + u] = dgv[g];
        }
        __syncthreads();
        // dh of the step before: thread (r, k) walks the 4 H gate columns; W_hh[j][k] is contiguous over k.  (sdh is read in the phase
        // above only, behind the barrier at the end of the step.)
        for (int item = tid; item < kDpR * H; item += 256) {
            const int r = item / H, k = item % H;
            float a = 0.f;
            for (int j = 0; j < 4 * H; ++j) a = fmaf(sdg[r * 4 * H + j], W[(long long)j * H + k], a);
            sdh[item] = a;
        }
        __syncthreads();
    }
    for (int q = 0; q < kDpR; ++q) {
        const DpSeq s = sseq[q];
        const int n = (s.cap - s.count) * 5 * H;
        for (int i = tid; i < n; i += 256) {
            const long long row = (long long)s.base + (long long)(s.count + i / (5 * H)) * s.stride;
            const int j = i % (5 * H);
            if (j < 4 * H)
                A.gates[row * ldg + (long long)d * 4 * H + j] = 0.f;
            else
                A.hprev[row * ldh + d * H + j - 4 * H] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ c. layer norm + mask + residual
// Row (b, s, k) is valid iff s < sb[b] (sb null: every row).
__device__ __forceinline__ bool dp_valid(const int* sb, long long row, int S, int K) {
    if (!sb) return true;
    const long long bs = row / K;
    return (int)(bs % S) < sb[bs / S];
}

// One wave per row: y = valid ? gamma (z - mean) rstd + beta : 0, plus the residual row.  stats = (mean, rstd), (0, 0) if not valid.
__global__ __launch_bounds__(256) void dprnn_norm_residual_forward_kernel(const float* __restrict__ z, const float* __restrict__ res,
                                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                          const int* __restrict__ sb, float* __restrict__ y,
                                                                          float* __restrict__ stats, long long rows, int N, int S, int K,
                                                                          float eps) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* __restrict__ zr = z + row * N;
    const bool valid = dp_valid(sb, row, S, K);
    float mean = 0.f, rstd = 0.f;
    if (valid) {
        double s1 = 0.;
        for (int n = lane; n < N; n += 64) s1 += (double)zr[n];
        const double m = wave_sum(s1) / (double)N;
        double s2 = 0.;
        for (int n = lane; n < N; n += 64) {
            const double dlt = (double)zr[n] - m;
            s2 += dlt * dlt;
        }
        const double var = wave_sum(s2) / (double)N;
        mean = (float)m, rstd = (float)(1. / sqrt(var + (double)eps));
    }
    if (lane == 0) stats[2 * row] = mean, stats[2 * row + 1] = rstd;
    for (int n = lane; n < N; n += 64) {
        const float v = valid ? fmaf(gamma[n], (zr[n] - mean) * rstd, beta[n]) : 0.f;
        y[row * N + n] = v + res[row * N + n];
    }
}

// One wave per row: dz = rstd (gy gamma - mean_n(gy gamma) - xhat mean_n(gy gamma xhat)) on valid rows, 0 else; dres = gy.
__global__ __launch_bounds__(256) void dprnn_norm_residual_backward_kernel(const float* __restrict__ gy, const float* __restrict__ z,
                                                                           const float* __restrict__ stats,
                                                                           const float* __restrict__ gamma, const int* __restrict__ sb,
                                                                           float* __restrict__ dz, float* __restrict__ dres,
                                                                           long long rows, int N, int S, int K) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* __restrict__ zr = z + row * N;
    const float* __restrict__ gr = gy + row * N;
    const bool valid = dp_valid(sb, row, S, K);
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float c1 = 0.f, c2 = 0.f;
    if (valid) {
        double s1 = 0., s2 = 0.;
        for (int n = lane; n < N; n += 64) {
            const float g = gr[n] * gamma[n];
            const float xh = (zr[n] - mean) * rstd;
            s1 += (double)g;
            s2 += (double)g * (double)xh;
        }
        c1 = (float)(wave_sum(s1) / (double)N), c2 = (float)(wave_sum(s2) / (double)N);
    }
    for (int n = lane; n < N; n += 64) {
        const float g = gr[n];
        float v = 0.f;
        if (valid) {
            const float xh = (zr[n] - mean) * rstd;
            v = rstd * fmaf(-xh, c2, g * gamma[n] - c1);
        }
        dz[row * N + n] = v;
        dres[row * N + n] = g;
    }
}

// Column sums over a slab of kDpSlabRows rows, workgroup (column block of 64, slab); thread (column, row group of 4).
//   mode 0: ws[slab][c] = sum_rows x[row][c]                                             (width C)
//   mode 1: ws[slab][c] = sum_valid gy xhat, ws[slab][C + c] = sum_valid gy   (x = gy)   (width 2 C)
__global__ __launch_bounds__(256) void dprnn_colsum_kernel(const float* __restrict__ x, long long ld, const float* __restrict__ z,
                                                           const float* __restrict__ stats, const int* __restrict__ sb,
                                                           double* __restrict__ ws, long long rows, int C, int S, int K, int mode) {
    __shared__ double red[4][64][2];
    const int cx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    const long long r0 = (long long)blockIdx.y * kDpSlabRows, r1 = min(r0 + kDpSlabRows, rows);
    double s1 = 0., s2 = 0.;
    if (c < C)
        for (long long row = r0 + g; row < r1; row += 4) {
            if (mode == 0) {
                s1 += (double)x[row * ld + c];
            } else if (dp_valid(sb, row, S, K)) {
                const float gv = x[row * ld + c];
                const float xh = (z[row * C + c] - stats[2 * row]) * stats[2 * row + 1];
                s1 += (double)gv * (double)xh;
                s2 += (double)gv;
            }
        }
    red[g][cx][0] = s1, red[g][cx][1] = s2;
    __syncthreads();
    if (g == 0 && c < C) {
        const long long width = mode ? 2LL * C : C;
        ws[blockIdx.y * width + c] = ((red[0][cx][0] + red[1][cx][0]) + red[2][cx][0]) + red[3][cx][0];
        if (mode) ws[blockIdx.y * width + C + c] = ((red[0][cx][1] + red[1][cx][1]) + red[2][cx][1]) + red[3][cx][1];
    }
}

// ------------------------------------------------------------------------------------------------ d. segment / overlap-add
// seg[b, s, k, :] = x[b, s P + k - (K - P), :] inside [0, L), 0 outside (the K - P zero frames in front and behind, end='pad').
__global__ __launch_bounds__(256) void dprnn_segment_kernel(const float* __restrict__ x, long long xs_b, long long xs_l, long long xs_n,
                                                            float* __restrict__ seg, long long total, long long L, int N, int S, int K,
                                                            int P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i % N);
    const long long pos = i / N;
    const int k = (int)(pos % K);
    const long long bs = pos / K;
    const long long s = bs % S, b = bs / S;
    const long long l = s * P + k - (K - P);
    seg[i] = (l >= 0 && l < L) ? x[b * xs_b + l * xs_l + n * xs_n] : 0.f;
}

// out[b, l, :] = sum over the chunks s (ascending) that hold frame l: seg[b, s, l + front - s P, :]; l < L_out (front = K - P: unpadded).
__global__ __launch_bounds__(256) void dprnn_overlap_add_kernel(const float* __restrict__ seg, long long ss_b, long long ss_s,
                                                                long long ss_k, long long ss_n, float* __restrict__ out,
                                                                long long total, long long L_out, int N, int S, int K, int P, int front) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i % N);
    const long long bl = i / N;
    const long long l = bl % L_out, b = bl / L_out;
    const long long q = l + front;                      // position in the padded signal: chunk s holds [s P, s P + K)
    long long s0 = q - K + 1 <= 0 ? 0 : (q - K + P) / P;        // ceil((q - K + 1) / P)
    long long s1 = q / P;
    if (s1 > S - 1) s1 = S - 1;
    float acc = 0.f;
    for (long long s = s0; s <= s1; ++s) acc += seg[b * ss_b + s * ss_s + (q - s * P) * ss_k + n * ss_n];
    out[i] = acc;
}

static int dp_hp(int H) { return H <= 32 ? 32 : (H <= 64 ? 64 : 128); }

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_dprnn_tables(const void* lengths, int32_t lengths_int64, int32_t B, int32_t S, int32_t K, int32_t P, int32_t* chunks,
                      int32_t* intra, int32_t* inter, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!chunks || !intra || !inter || B < 1 || S < 1 || K < 1 || P < 1 || P > K, PTMI_E_INVALID);
    PTMI_RETURN_IF((long long)B * S * K > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    const long long n = std::max<long long>((long long)B * S, (long long)B * K);
    hipLaunchKernelGGL(dprnn_tables_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), lengths,
                       lengths_int64, B, S, K, P, chunks, intra, inter);
    return launch_status();
}

int32_t ptmi_chunk_lstm_max_hidden(void) { return kDpMaxStreamH; }

int32_t ptmi_chunk_lstm_max_resident_hidden(void) { return 128; }

int32_t ptmi_chunk_lstm_tile(void) { return kDpR; }

static int dp_lstm(const DpLstmArgs& A, int backward, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!A.gates || !A.w_hh[0] || !A.h || !A.c || !A.table || A.nseq < 1 || A.H < 1 || A.cap < 1 || A.D < 1 || A.D > 2,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(A.D == 2 && !A.w_hh[1], PTMI_E_INVALID);
    PTMI_RETURN_IF(A.H > kDpMaxStreamH, PTMI_E_UNSUPPORTED);
    const dim3 grid((unsigned)((A.nseq + kDpR - 1) / kDpR), (unsigned)A.D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (A.H > 128) {            // W_hh does not fit on chip: streamed from the L2
        const size_t lds = (size_t)kDpR * (backward ? 6 : 2) * A.H * sizeof(float);
        const void* fn = backward ? reinterpret_cast<const void*>(dprnn_lstm_backward_stream_kernel)
                                  : reinterpret_cast<const void*>(dprnn_lstm_forward_stream_kernel);
        if (lds > 64 * 1024)     // above the default limit of dynamic LDS the kernel has to be told (an attribute of the function: no sync)
            PTMI_RETURN_IF(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess, PTMI_E_UNSUPPORTED);
        if (backward)
            hipLaunchKernelGGL(dprnn_lstm_backward_stream_kernel, grid, dim3(256), lds, st, A);
        else
            hipLaunchKernelGGL(dprnn_lstm_forward_stream_kernel, grid, dim3(256), lds, st, A);
        return launch_status();
    }
    const int hp = dp_hp(A.H);
#define DP_LAUNCH(HP)                                                                                   \
    do {                                                                                                \
        if (backward)                                                                                   \
            hipLaunchKernelGGL((dprnn_lstm_backward_kernel<HP>), grid, dim3(4 * HP), 0, st, A);         \
        else                                                                                            \
            hipLaunchKernelGGL((dprnn_lstm_forward_kernel<HP>), grid, dim3(4 * HP), 0, st, A);          \
    } while (0)
    if (hp == 32)
        DP_LAUNCH(32);
    else if (hp == 64)
        DP_LAUNCH(64);
    else
        DP_LAUNCH(128);
#undef DP_LAUNCH
    return launch_status();
}

int ptmi_chunk_lstm_forward(float* gates, const float* w_hh, const float* w_hh_reverse, const float* b_hh, const float* b_hh_reverse,
                            float* h, float* c, const int32_t* table, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                            ptmi_stream_t stream) {
    PTMI_RETURN_IF(!b_hh || (ndir == 2 && !b_hh_reverse), PTMI_E_INVALID);
    DpLstmArgs A{};
    A.gates = gates, A.w_hh[0] = w_hh, A.w_hh[1] = w_hh_reverse, A.b_hh[0] = b_hh, A.b_hh[1] = b_hh_reverse, A.h = h, A.c = c;
    A.table = table, A.nseq = nseq, A.H = H, A.D = ndir, A.cap = cap;
    return dp_lstm(A, 0, stream);
}

int ptmi_chunk_lstm_backward(float* gates, const float* dh, const float* w_hh, const float* w_hh_reverse, const float* h, const float* c,
                             float* hprev, const int32_t* table, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                             ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dh || !hprev, PTMI_E_INVALID);
    DpLstmArgs A{};
    A.gates = gates, A.dh = dh, A.w_hh[0] = w_hh, A.w_hh[1] = w_hh_reverse, A.h = const_cast<float*>(h), A.c = const_cast<float*>(c);
    A.hprev = hprev, A.table = table, A.nseq = nseq, A.H = H, A.D = ndir, A.cap = cap;
    return dp_lstm(A, 1, stream);
}

static long long dp_slabs(int64_t rows) { return (rows + kDpSlabRows - 1) / kDpSlabRows; }

int64_t ptmi_dprnn_colsum_workspace_elems(int64_t rows, int32_t C) {
    if (rows < 1 || C < 1) return PTMI_E_INVALID;
    return dp_slabs(rows) * 2 * (long long)C;
}

int ptmi_dprnn_colsum(const float* x, int64_t ld, float* out, float* out2, double* workspace, int64_t rows, int32_t C,
                      ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !out || !workspace || rows < 1 || C < 1 || ld < C, PTMI_E_INVALID);
    const long long slabs = dp_slabs(rows);
    PTMI_RETURN_IF(slabs > 65535, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dprnn_colsum_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)slabs), dim3(256), 0, st, x, (long long)ld,
                       (const float*)nullptr, (const float*)nullptr, (const int*)nullptr, workspace, (long long)rows, C, 1, 1, 0);
    int rc = launch_status();
    if (rc) return rc;
    return colreduce(workspace, slabs, (long long)C, StoreTwice{out, out2}, st);          // out2: b_hh beside b_ih
}

int ptmi_dprnn_norm_residual_forward(const float* z, const float* residual, const float* gamma, const float* beta,
                                     const int32_t* chunks, float* y, float* stats, int64_t rows, int32_t N, int32_t S, int32_t K,
                                     float eps, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!z || !residual || !gamma || !beta || !y || !stats || rows < 1 || N < 1 || S < 1 || K < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF((rows + 3) / 4 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(dprnn_norm_residual_forward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), z, residual, gamma, beta, chunks, y, stats, (long long)rows, N, S, K, eps);
    return launch_status();
}

int ptmi_dprnn_norm_residual_backward(const float* gy, const float* z, const float* stats, const float* gamma, const int32_t* chunks,
                                      float* dz, float* dresidual, float* dparams, double* workspace, int64_t rows, int32_t N,
                                      int32_t S, int32_t K, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gy || !z || !stats || !gamma || !dz || !dresidual || !dparams || !workspace || rows < 1 || N < 1 || S < 1 || K < 1,
                   PTMI_E_INVALID);
    const long long slabs = dp_slabs(rows);
    PTMI_RETURN_IF((rows + 3) / 4 > 0x7fffffffLL || slabs > 65535, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dprnn_norm_residual_backward_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, gy, z, stats, gamma,
                       chunks, dz, dresidual, (long long)rows, N, S, K);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(dprnn_colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)slabs), dim3(256), 0, st, gy, (long long)N, z, stats,
                       chunks, workspace, (long long)rows, N, S, K, 1);
    rc = launch_status();
    if (rc) return rc;
    return colreduce(workspace, slabs, 2LL * N, StoreTwice{dparams, nullptr}, st);
}

int64_t ptmi_dprnn_num_chunks(int64_t L, int32_t K, int32_t P) {
    if (L < 1 || K < 1 || P < 1 || P > K) return PTMI_E_INVALID;
    const long long padded = L + 2LL * (K - P);
    return padded <= K ? 1 : (padded - K + P - 1) / P + 1;
}

int ptmi_dprnn_segment(const float* x, const int64_t* x_strides, float* seg, int64_t B, int64_t L, int32_t N, int32_t S, int32_t K,
                       int32_t P, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !x_strides || !seg || B < 1 || L < 1 || N < 1 || S < 1 || K < 1 || P < 1 || P > K, PTMI_E_INVALID);
    const long long total = (long long)B * S * K * N;
    PTMI_RETURN_IF((total + 255) / 256 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(dprnn_segment_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                       (long long)x_strides[0], (long long)x_strides[1], (long long)x_strides[2], seg, total, (long long)L, N, S, K, P);
    return launch_status();
}

int ptmi_dprnn_overlap_add(const float* seg, const int64_t* seg_strides, float* out, int64_t B, int64_t L_out, int32_t N, int32_t S,
                           int32_t K, int32_t P, int32_t front, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!seg || !seg_strides || !out || B < 1 || L_out < 1 || N < 1 || S < 1 || K < 1 || P < 1 || P > K || front < 0,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(L_out + front > (long long)(S - 1) * P + K, PTMI_E_INVALID);        // every frame lies in a chunk
    const long long total = (long long)B * L_out * N;
    PTMI_RETURN_IF((total + 255) / 256 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(dprnn_overlap_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       seg, (long long)seg_strides[0], (long long)seg_strides[1], (long long)seg_strides[2], (long long)seg_strides[3],
                       out, total, (long long)L_out, N, S, K, P, front);
    return launch_status();
}

}  // extern "C"
