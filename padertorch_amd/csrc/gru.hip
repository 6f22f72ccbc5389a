// One torch.nn.GRU layer over a table of independent sequences (padertorch/contrib/je/modules/rnn.py: RNN / GRU), between its GEMMs.
//
// The decomposition is that of csrc/dprnn.hip: a sequence is (base row, step stride, step count), one workgroup
// owns kGruR = 4 sequences of one direction from their first step to their last, W_hh [3H, H] lives in the registers of the workgroup
// (HP = H rounded up to 32 / 64 / 128), h travels between steps through double-buffered LDS, products and sums are fp32 FMAs.  No flag,
// no spin, no ordering between workgroups.  H > 128 runs on two kernels that stream W_hh from the L2 every step.
//
// What differs from the LSTM: three gates (r, z, n), and the candidate multiplies r into the recurrent product,
//     q = h W_hn^T + b_hn,   n = tanh(x W_in^T + b_in + r q),   h' = (1 - z) n + z h,
// so the forward saves q beside the activated gates and the backward writes TWO gradient operands that differ in their n block:
//     gates <- (dr_pre, dz_pre, dn_pre)        for dW_ih, db_ih, dx
//     q     <-                  dn_pre r       the n block of the operand for dW_hh, db_hh (its r and z blocks are those of gates)
// The state that crosses a step of the backward is dh alone: dh_prev = dh z + dr_pre W_hr + dz_pre W_hz + (dn_pre r) W_hn.
//
// `flip` runs direction d in the opposite sense of time (direction 0 from the last step to the first): RNN(reverse=True).
// A sequence whose rows base + t stride, t < cap, do not all lie inside [0, rows) is skipped entirely: nothing is read or written
// outside the buffers whatever the table holds.  No allocation, no synchronisation: every launcher is capturable.
#include <algorithm>

#include "lstm_common.h"
#include "reduce.h"

namespace ptmi {

constexpr int kGruR = 4;                 // sequences per workgroup
constexpr int kGruMaxStreamH = 1792;     // 5 kGruR H words of LDS in the streamed kernels: 140 KB of the 160 KB of a CU

__device__ __forceinline__ float gru_quad_xor1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float gru_quad_xor2(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ void gru_pin(float& v) { asm volatile("" : "+v"(v)); }
// The sums so far are complete here and no later LDS read starts before (keeps the reads of a whole block from being hoisted in front of
// the FMAs all at once: registers).
__device__ __forceinline__ void gru_fence(float (&acc)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(acc[a][q])::"memory");
    __builtin_amdgcn_sched_barrier(0);
}

struct GruArgs {
    float* gates;            // [rows, D 3H]: forward in: x W_ih^T + b_ih, out: the activated (r, z, n); backward in: those, out: (dr_pre, dz_pre, dn_pre)
    float* q;                // [rows, D H]: forward out: h W_hn^T + b_hn; backward in: that, out: dn_pre r
    const float* w_hh[2];    // [3H, H] per direction
    const float* b_hh[2];    // [3H] per direction or null (forward)
    float* h;                // [rows, D H]: forward out; backward in
    const float* dh;         // [rows, D H]  (backward)
    float* hprev;            // [rows, D H]  (backward out): h of the step before, 0 at a first step and off the steps
    const int* table;        // [nseq][3]
    long long rows;
    int nseq, H, D, cap, flip;
};

struct GruSeq {
    int base, stride, count, cap;
};

__device__ __forceinline__ GruSeq gru_seq(const GruArgs& A, int seq) {
    GruSeq s{0, 0, 0, 0};
    if (seq < A.nseq) {
        const int base = A.table[3 * seq], stride = A.table[3 * seq + 1], count = A.table[3 * seq + 2];
        const long long lastrow = (long long)base + (long long)(A.cap - 1) * stride;
        if (base >= 0 && base < A.rows && lastrow >= 0 && lastrow < A.rows) {
            s.base = base, s.stride = stride, s.cap = A.cap;
            s.count = count < 0 ? 0 : (count > A.cap ? A.cap : count);
        }
    }
    return s;
}

// Row of processing step p of a sequence walked backwards in time (rev) or forwards: backwards starts at the sequence's own last step.
__device__ __forceinline__ long long gru_row(const GruSeq& s, int rev, int p) {
    return (long long)s.base + (long long)(rev ? s.count - 1 - p : p) * s.stride;
}

// Zeros on the rows count .. cap of the tile's sequences: `wg` words per row at column offset d wg of g (leading dimension D wg; g null:
// none) and H words at d H of each of h0, h1 (null: none).
__device__ __forceinline__ void gru_zero_tail(const GruSeq* sseq, int tid, int nthreads, int d, int D, int H, float* g, int wg, float* h0,
                                              float* h1) {
    const int per = (g ? wg : 0) + (h0 ? H : 0) + (h1 ? H : 0);
    for (int r = 0; r < kGruR; ++r) {
        const GruSeq s = sseq[r];
        const long long n = (long long)(s.cap - s.count) * per;
        for (long long i = tid; i < n; i += nthreads) {
            const long long row = (long long)s.base + (long long)(s.count + i / per) * s.stride;
            int j = (int)(i % per);
            if (g) {
                if (j < wg) {
                    g[row * D * wg + (long long)d * wg + j] = 0.f;
                    continue;
                }
                j -= wg;
            }
            if (h0) {
                if (j < H) {
                    h0[row * D * H + d * H + j] = 0.f;
                    continue;
                }
                j -= H;
            }
            h1[row * D * H + d * H + j] = 0.f;
        }
    }
}

// Forward.  Thread (u, kq) = (tid / 4, tid % 4) holds W_hh[g H + u][k] for the three gates and the quarter k in [kq HP/4, (kq+1) HP/4)
// (3 HP / 4 registers), multiplies them with h of the four sequences (one float4 per k from LDS: a broadcast), adds the four quarters by
// two quad exchanges and then owns (sequence kq, unit u): gates, q, h (its own h of the step before stays in a register).
template <int HP>
__global__ __launch_bounds__(4 * HP) void gru_forward_kernel(const GruArgs A) {
    constexpr int KQ = HP / 4;
    constexpr int LDQ = KQ * 4 + 4;
    __shared__ __attribute__((aligned(16))) float sh[2][4 * LDQ];      // [buffer][kq][k][r]
    __shared__ GruSeq sseq[kGruR];
    const int tid = threadIdx.x, u = tid >> 2, kq = tid & 3, d = blockIdx.y, H = A.H, rev = d ^ A.flip;
    if (tid < kGruR) sseq[tid] = gru_seq(A, blockIdx.x * kGruR + tid);
    for (int i = tid; i < 2 * 4 * LDQ; i += 4 * HP) (&sh[0][0])[i] = 0.f;
    float w[3][KQ];
    const float* __restrict__ W = A.w_hh[d];
    const unsigned last = 3u * H * H - 1u;     // H <= 128: every index fits 32 bits
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const bool ok = u < H && kq * KQ + k < H;
            const float v = W[min((unsigned)((g * H + u) * H + kq * KQ + k), last)];
            w[g][k] = ok ? v : 0.f;
            gru_pin(w[g][k]);
        }
    float bias[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) bias[g] = (u < H && A.b_hh[d]) ? A.b_hh[d][g * H + u] : 0.f;
    __syncthreads();
    const GruSeq me = sseq[kq];
    int maxT = 0;
#pragma unroll
    for (int r = 0; r < kGruR; ++r) maxT = max(maxT, sseq[r].count);
    const long long ldg = (long long)A.D * 3 * H, ldh = (long long)A.D * H;
    float hown = 0.f;
    for (int t = 0; t < maxT; ++t) {
        const bool on = t < me.count && u < H;
        const long long row = gru_row(me, rev, t);
        float gx[3] = {0.f, 0.f, 0.f};
        if (on) {
#pragma unroll
            for (int g = 0; g < 3; ++g) gx[g] = A.gates[row * ldg + (long long)d * 3 * H + g * H + u];
        }
        const float* __restrict__ hq = &sh[t & 1][kq * LDQ];
        float acc[3][4];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[g][r] = 0.f;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const f32x4 hv = *reinterpret_cast<const f32x4*>(hq + 4 * k);
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                acc[g][0] = fmaf(w[g][k], hv.x, acc[g][0]);
                acc[g][1] = fmaf(w[g][k], hv.y, acc[g][1]);
                acc[g][2] = fmaf(w[g][k], hv.z, acc[g][2]);
                acc[g][3] = fmaf(w[g][k], hv.w, acc[g][3]);
            }
        }
        // the four quarters of a quad, reduce-scatter: lane kq ends with the full sum of sequence kq
        float pre[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const bool odd = kq & 1, high = kq & 2;
            const float lo = (odd ? acc[g][1] : acc[g][0]) + gru_quad_xor1(odd ? acc[g][0] : acc[g][1]);
            const float hi = (odd ? acc[g][3] : acc[g][2]) + gru_quad_xor1(odd ? acc[g][2] : acc[g][3]);
            pre[g] = (high ? hi : lo) + gru_quad_xor2(high ? lo : hi);
        }
        if (on) {
            const float gr = sigmoidf_(gx[0] + bias[0] + pre[0]);
            const float gz = sigmoidf_(gx[1] + bias[1] + pre[1]);
            const float qq = pre[2] + bias[2];
            const float gn = tanhf_(fmaf(gr, qq, gx[2]));
            const float hh = fmaf(gz, hown - gn, gn);          // (1 - z) n + z h
            float* __restrict__ go = A.gates + row * ldg + (long long)d * 3 * H + u;
            go[0] = gr, go[H] = gz, go[2 * H] = gn;
            A.q[row * ldh + d * H + u] = qq;
            A.h[row * ldh + d * H + u] = hh;
            hown = hh;
            sh[(t + 1) & 1][(u / KQ) * LDQ + (u % KQ) * 4 + kq] = hh;
        }
        __syncthreads();
    }
    gru_zero_tail(sseq, tid, 4 * HP, d, A.D, H, nullptr, 0, A.h, nullptr);
}

// Backward.  Two thread maps per step:
//   cell: thread (r, u) = (tid / HP, tid % HP) owns dh of (sequence r, unit u): reads the saved gates, q, the step's dh and the recurrent
//     part (12 partials from LDS), writes both operands to memory (in place) and the W_hh operand to LDS, and h of the step before to hprev;
//   product: thread (jb, ug) = (tid / (HP/4), tid % (HP/4)), jb < 12, holds W_hh[j][4 ug + a] for a < 4 and the HP/4 gate columns j of
//     block jb (HP registers) and writes its partial of dh_prev[r][4 ug + a] to LDS.  The last HP threads have no block.
template <int HP>
__global__ __launch_bounds__(4 * HP) void gru_backward_kernel(const GruArgs A) {
    constexpr int JB = HP / 4;
    constexpr int LDJ = JB * 4 + 4;
    constexpr int NB = 12;                     // 3 HP padded gate columns in blocks of JB
    __shared__ __attribute__((aligned(16))) float sdg[NB * LDJ];            // [jb][jj][r]
    __shared__ __attribute__((aligned(16))) float spart[NB][kGruR][HP];     // [jb][r][u]
    __shared__ GruSeq sseq[kGruR];
    const int tid = threadIdx.x, d = blockIdx.y, H = A.H, rev = d ^ A.flip;
    const int r = tid / HP, u = tid % HP;      // cell map
    const int jb = tid / JB, ug = tid % JB;    // product map
    const bool prod = jb < NB;
    if (tid < kGruR) sseq[tid] = gru_seq(A, blockIdx.x * kGruR + tid);
    for (int i = tid; i < NB * kGruR * HP; i += 4 * HP) (&spart[0][0][0])[i] = 0.f;
    float w[4][JB];
    const float* __restrict__ W = A.w_hh[d];
    const unsigned last = 3u * H * H - 1u;
#pragma unroll
    for (int jj = 0; jj < JB; ++jj) {
        const int jp = jb * JB + jj, g = jp / HP, ju = jp % HP;       // padded gate column jp = g HP + unit
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bool ok = prod && ju < H && 4 * ug + a < H;
            const float v = W[min((unsigned)((g * H + ju) * H + 4 * ug + a), last)];
            w[a][jj] = ok ? v : 0.f;
            gru_pin(w[a][jj]);
        }
    }
    __syncthreads();
    const GruSeq me = sseq[r];
    int maxT = 0;
#pragma unroll
    for (int q = 0; q < kGruR; ++q) maxT = max(maxT, sseq[q].count);
    const long long ldg = (long long)A.D * 3 * H, ldh = (long long)A.D * H;
    float carry = 0.f;                         // dh z of the step behind
    for (int t = 0; t < maxT; ++t) {
        const bool on = t < me.count && u < H;
        const int p = me.count - 1 - t;        // processing step, last first
        float dgv[3] = {0.f, 0.f, 0.f};
        if (on) {
            const long long row = gru_row(me, rev, p);
            float* __restrict__ go = A.gates + row * ldg + (long long)d * 3 * H + u;
            const float gr = go[0], gz = go[H], gn = go[2 * H];
            const float qq = A.q[row * ldh + d * H + u];
            const float hp = p > 0 ? A.h[gru_row(me, rev, p - 1) * ldh + d * H + u] : 0.f;
            float dh = A.dh[row * ldh + d * H + u] + carry;
#pragma unroll
            for (int b = 0; b < NB; ++b) dh += spart[b][r][u];
            const float dn_pre = dh * (1.f - gz) * (1.f - gn * gn);
            const float dz_pre = dh * (hp - gn) * gz * (1.f - gz);
            const float dr_pre = dn_pre * qq * gr * (1.f - gr);
            const float dnr = dn_pre * gr;
            carry = dh * gz;
            dgv[0] = dr_pre, dgv[1] = dz_pre, dgv[2] = dnr;
            go[0] = dr_pre, go[H] = dz_pre, go[2 * H] = dn_pre;
            A.q[row * ldh + d * H + u] = dnr;
            A.hprev[row * ldh + d * H + u] = hp;
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int jp = g * HP + u;
            sdg[(jp / JB) * LDJ + (jp % JB) * 4 + r] = dgv[g];
        }
        __syncthreads();
        if (prod) {
            float acc[4][4];                   // [output][sequence]
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[a][q] = 0.f;
            const float* __restrict__ dq = &sdg[jb * LDJ];
#pragma unroll
            for (int jj = 0; jj < JB; ++jj) {
                if (jj % 8 == 0) gru_fence(acc);
                const f32x4 v = *reinterpret_cast<const f32x4*>(dq + 4 * jj);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    acc[a][0] = fmaf(w[a][jj], v.x, acc[a][0]);
                    acc[a][1] = fmaf(w[a][jj], v.y, acc[a][1]);
                    acc[a][2] = fmaf(w[a][jj], v.z, acc[a][2]);
                    acc[a][3] = fmaf(w[a][jj], v.w, acc[a][3]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<f32x4*>(&spart[jb][q][4 * ug]) = f32x4{acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
        }
        __syncthreads();
    }
    // rows that belong to no step: both operands and hprev = 0 (the weight-gradient GEMMs read every row)
    gru_zero_tail(sseq, tid, 4 * HP, d, A.D, H, A.gates, 3 * H, A.q, A.hprev);
}

// ---- H > 128: W_hh is streamed from the L2 every step, coalesced; kGruNT = 1024 threads; a cell (r, u) = item / H, item % H belongs to
// thread item % kGruNT in every phase.
//   forward:  a wavefront per row j of W_hh (lanes over k, the four sequences share every weight it loads); the four sums are
//             reduce-scattered inside the quads and added across them (6 exchanges), lanes 0..3 write pre[r][j] to LDS; then the cells.
//   backward: thread (js, k) loads W_hh[j][k] for the rows j = js, js + JS, ... once for the four sequences (neighbouring threads on
//             neighbouring k) and writes its partial of dh_prev[r][k] to LDS; JS = max(1, 1024 / H) row classes keep all threads busy.
// What bounds H is the LDS of a CU.  Forward: h double-buffered (2 H) and the recurrent products (3 H); backward: the W_hh operand (3 H),
// the partials of dh (JS H <= max(H, 1024)) and the carried dh z (H), each for kGruR sequences: 5 kGruR H words = 80 H bytes from H =
// 1024 on (160 KB: H <= 2048; kGruMaxStreamH leaves room).
constexpr int kGruNT = 1024;

static int gru_row_classes(int H) { return std::max(1, kGruNT / H); }

__global__ __launch_bounds__(kGruNT) void gru_forward_stream_kernel(const GruArgs A) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];          // sh [2][kGruR][H] | spre [kGruR][3 H]
    __shared__ GruSeq sseq[kGruR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = blockIdx.y, H = A.H, rev = d ^ A.flip;
    float* __restrict__ spre = dyn + 2 * kGruR * H;
    if (tid < kGruR) sseq[tid] = gru_seq(A, blockIdx.x * kGruR + tid);
    for (int i = tid; i < 2 * kGruR * H; i += kGruNT) dyn[i] = 0.f;
    __syncthreads();
    int maxT = 0;
#pragma unroll
    for (int r = 0; r < kGruR; ++r) maxT = max(maxT, sseq[r].count);
    const float* __restrict__ W = A.w_hh[d];
    const float* __restrict__ bh = A.b_hh[d];
    const long long ldg = (long long)A.D * 3 * H, ldh = (long long)A.D * H;
    const bool odd = lane & 1, high = lane & 2;
    for (int t = 0; t < maxT; ++t) {
        const float* __restrict__ hin = dyn + (t & 1) * kGruR * H;
        float* __restrict__ hout = dyn + ((t + 1) & 1) * kGruR * H;
        for (int j = wave; j < 3 * H; j += kGruNT / 64) {
            const float* __restrict__ wr = W + (long long)j * H;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            for (int k = lane; k < H; k += 64) {
                const float w = wr[k];
                a0 = fmaf(w, hin[k], a0), a1 = fmaf(w, hin[H + k], a1), a2 = fmaf(w, hin[2 * H + k], a2), a3 = fmaf(w, hin[3 * H + k], a3);
            }
            // lane q of a quad ends with the quad's sum of sequence q (as in the resident kernel), then the 16 quads are added
            const float lo = (odd ? a1 : a0) + gru_quad_xor1(odd ? a0 : a1);
            const float hi = (odd ? a3 : a2) + gru_quad_xor1(odd ? a2 : a3);
            float v = (high ? hi : lo) + gru_quad_xor2(high ? lo : hi);
#pragma unroll
            for (int o = 4; o <= 32; o <<= 1) v += __shfl_xor(v, o, 64);
            if (lane < kGruR) spre[lane * 3 * H + j] = v;
        }
        __syncthreads();
        for (int item = tid; item < kGruR * H; item += kGruNT) {
            const int r = item / H, u = item % H;
            const GruSeq me = sseq[r];
            if (t >= me.count) continue;
            const long long row = gru_row(me, rev, t);
            float* __restrict__ go = A.gates + row * ldg + (long long)d * 3 * H + u;
            float pre[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) pre[g] = spre[r * 3 * H + g * H + u] + (bh ? bh[g * H + u] : 0.f);
            const float gr = sigmoidf_(go[0] + pre[0]);
            const float gz = sigmoidf_(go[H] + pre[1]);
            const float gn = tanhf_(fmaf(gr, pre[2], go[2 * H]));
            const float hh = fmaf(gz, hin[item] - gn, gn);
            go[0] = gr, go[H] = gz, go[2 * H] = gn;
            A.q[row * ldh + d * H + u] = pre[2];
            A.h[row * ldh + d * H + u] = hh;
            hout[item] = hh;
        }
        __syncthreads();
    }
    gru_zero_tail(sseq, tid, kGruNT, d, A.D, H, nullptr, 0, A.h, nullptr);
}

__global__ __launch_bounds__(kGruNT) void gru_backward_stream_kernel(const GruArgs A, const int JS) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];          // sdg [kGruR][3 H] | scarry [kGruR][H] | spart [JS][kGruR][H]
    __shared__ GruSeq sseq[kGruR];
    const int tid = threadIdx.x, d = blockIdx.y, H = A.H, rev = d ^ A.flip;
    float* __restrict__ sdg = dyn;
    float* __restrict__ scarry = dyn + kGruR * 3 * H;
    float* __restrict__ spart = dyn + kGruR * 4 * H;
    if (tid < kGruR) sseq[tid] = gru_seq(A, blockIdx.x * kGruR + tid);
    for (int i = tid; i < kGruR * (4 + JS) * H; i += kGruNT) dyn[i] = 0.f;
    __syncthreads();
    int maxT = 0;
#pragma unroll
    for (int r = 0; r < kGruR; ++r) maxT = max(maxT, sseq[r].count);
    const float* __restrict__ W = A.w_hh[d];
    const long long ldg = (long long)A.D * 3 * H, ldh = (long long)A.D * H;
    for (int t = 0; t < maxT; ++t) {
        for (int item = tid; item < kGruR * H; item += kGruNT) {
            const int r = item / H, u = item % H;
            const GruSeq me = sseq[r];
            float dgv[3] = {0.f, 0.f, 0.f};
            if (t < me.count) {
                const int p = me.count - 1 - t;
                const long long row = gru_row(me, rev, p);
                float* __restrict__ go = A.gates + row * ldg + (long long)d * 3 * H + u;
                const float gr = go[0], gz = go[H], gn = go[2 * H];
                const float qq = A.q[row * ldh + d * H + u];
                const float hp = p > 0 ? A.h[gru_row(me, rev, p - 1) * ldh + d * H + u] : 0.f;
                float dh = A.dh[row * ldh + d * H + u] + scarry[item];
                for (int s = 0; s < JS; ++s) dh += spart[s * kGruR * H + item];
                const float dn_pre = dh * (1.f - gz) * (1.f - gn * gn);
                const float dz_pre = dh * (hp - gn) * gz * (1.f - gz);
                const float dr_pre = dn_pre * qq * gr * (1.f - gr);
                const float dnr = dn_pre * gr;
                scarry[item] = dh * gz;
                dgv[0] = dr_pre, dgv[1] = dz_pre, dgv[2] = dnr;
                go[0] = dr_pre, go[H] = dz_pre, go[2 * H] = dn_pre;
                A.q[row * ldh + d * H + u] = dnr;
                A.hprev[row * ldh + d * H + u] = hp;
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) sdg[r * 3 * H + g * H + u] = dgv[g];
        }
        __syncthreads();
        // the recurrent part of dh of the step before.  (spart is read in the phase above only, behind the barrier at the end of the step.)
        for (int it = tid; it < JS * H; it += kGruNT) {
            const int js = it / H, k = it % H;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
            for (int j = js; j < 3 * H; j += JS) {
                const float w = W[(long long)j * H + k];
                a0 = fmaf(sdg[j], w, a0), a1 = fmaf(sdg[3 * H + j], w, a1), a2 = fmaf(sdg[6 * H + j], w, a2), a3 = fmaf(sdg[9 * H + j], w, a3);
            }
            float* __restrict__ sp = spart + (long long)js * kGruR * H + k;
            sp[0] = a0, sp[H] = a1, sp[2 * H] = a2, sp[3 * H] = a3;
        }
        __syncthreads();
    }
    gru_zero_tail(sseq, tid, kGruNT, d, A.D, H, A.gates, 3 * H, A.q, A.hprev);
}

static int gru_hp(int H) { return H <= 32 ? 32 : (H <= 64 ? 64 : 128); }

static int gru_launch(const GruArgs& A, int backward, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!A.gates || !A.q || !A.w_hh[0] || !A.h || !A.table || A.nseq < 1 || A.H < 1 || A.cap < 1 || A.D < 1 || A.D > 2 || A.rows < 1,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(A.D == 2 && !A.w_hh[1], PTMI_E_INVALID);
    PTMI_RETURN_IF(A.D == 2 && ((A.b_hh[0] == nullptr) != (A.b_hh[1] == nullptr)), PTMI_E_INVALID);
    PTMI_RETURN_IF(A.H > kGruMaxStreamH, PTMI_E_UNSUPPORTED);
    const dim3 grid((unsigned)((A.nseq + kGruR - 1) / kGruR), (unsigned)A.D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (A.H > 128) {
        const int JS = gru_row_classes(A.H);
        const size_t lds = (size_t)kGruR * (backward ? 4 + JS : 5) * A.H * sizeof(float);
        const void* fn = backward ? reinterpret_cast<const void*>(gru_backward_stream_kernel)
                                  : reinterpret_cast<const void*>(gru_forward_stream_kernel);
        if (lds > 64 * 1024)     // above the default limit of dynamic LDS the kernel has to be told (an attribute of the function: no sync)
            PTMI_RETURN_IF(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess, PTMI_E_UNSUPPORTED);
        if (backward)
            hipLaunchKernelGGL(gru_backward_stream_kernel, grid, dim3(kGruNT), lds, st, A, JS);
        else
            hipLaunchKernelGGL(gru_forward_stream_kernel, grid, dim3(kGruNT), lds, st, A);
        return launch_status();
    }
    const int hp = gru_hp(A.H);
#define GRU_LAUNCH(HP)                                                                          \
    do {                                                                                        \
        if (backward)                                                                           \
            hipLaunchKernelGGL((gru_backward_kernel<HP>), grid, dim3(4 * HP), 0, st, A);        \
        else                                                                                    \
            hipLaunchKernelGGL((gru_forward_kernel<HP>), grid, dim3(4 * HP), 0, st, A);         \
    } while (0)
    if (hp == 32)
        GRU_LAUNCH(32);
    else if (hp == 64)
        GRU_LAUNCH(64);
    else
        GRU_LAUNCH(128);
#undef GRU_LAUNCH
    return launch_status();
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int32_t ptmi_chunk_gru_max_hidden(void) { return kGruMaxStreamH; }

int32_t ptmi_chunk_gru_max_resident_hidden(void) { return 128; }

int32_t ptmi_chunk_gru_tile(void) { return kGruR; }

int ptmi_chunk_gru_forward(float* gates, const float* w_hh, const float* w_hh_reverse, const float* b_hh, const float* b_hh_reverse,
                           float* q, float* h, const int32_t* table, int64_t rows, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                           int32_t flip, ptmi_stream_t stream) {
    GruArgs A{};
    A.gates = gates, A.q = q, A.w_hh[0] = w_hh, A.w_hh[1] = w_hh_reverse, A.b_hh[0] = b_hh, A.b_hh[1] = b_hh_reverse, A.h = h;
    A.table = table, A.rows = rows, A.nseq = nseq, A.H = H, A.D = ndir, A.cap = cap, A.flip = flip ? 1 : 0;
    return gru_launch(A, 0, stream);
}

int ptmi_chunk_gru_backward(float* gates, float* q, const float* dh, const float* w_hh, const float* w_hh_reverse, const float* h,
                            float* hprev, const int32_t* table, int64_t rows, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                            int32_t flip, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dh || !hprev, PTMI_E_INVALID);
    GruArgs A{};
    A.gates = gates, A.q = q, A.dh = dh, A.w_hh[0] = w_hh, A.w_hh[1] = w_hh_reverse, A.h = const_cast<float*>(h), A.hprev = hprev;
    A.table = table, A.rows = rows, A.nseq = nseq, A.H = H, A.D = ndir, A.cap = cap, A.flip = flip ? 1 : 0;
    return gru_launch(A, 1, stream);
}

}  // extern "C"
