// Packed-sequence (B)LSTM recurrence for gfx950 (MI355X): forward and backward-through-time.
//
// Replaces the recurrent part of torch.nn.LSTM on a PackedSequence as used by
// padertorch/contrib/examples/source_separation/pit/model.py:60-66,97 and contrib/tcl/dc.py:32-34,61
// (PyTorch semantics: gate order i,f,g,o; two bias vectors; zero initial state).
//
// The input projections X W_ih^T + b (60 % of the LSTM FLOPs) are ONE dense GEMM per layer for
// both directions and stay on the BLAS library.  What is hand-written is the part that is
// sequential in time:
//     gates = gx[t] + h_{t-1} W_hh^T
//     i,f,o = sigmoid, g = tanh, c_t = f c_{t-1} + i g, h_t = o tanh(c_t)      (fused epilogue)
// and the mirrored step of the backward pass (dh_rec = dgates_{t+1} W_hh, then the gate
// derivatives), both directions in one launch.  Two execution forms with the same results:
//   * lstm_{fwd,bwd}_step_kernel (this file): one launch per timestep, the product in exact fp32 on the matrix
//     cores (v_mfma_f32_16x16x4_f32, K split over the wavefronts of a workgroup, LDS reduce; MIOpen spends 4
//     launches, 2 GEMMs + 2 pointwise, per step and direction here); no residency requirement;
//   * the persistent kernels of csrc/lstm_split.hip (default): ONE launch per layer and pass, split 16-bit MFMA
//     products, the steps chained through hand-off planes that carry their own "ready" (data-as-flag).  All
//     workgroups of a launch must be co-resident.  This file holds their host side: fwd_plan / bwd_plan decide per
//     configuration whether they run and with which tile and grid - every geometry rule is written there, once -,
//     and ptmi_lstm_{forward,backward}_persistent check their contract (include/ptmi.h) in full before they
//     enqueue anything.
// Environment: PTMI_LSTM_F32 (the persistent entries refuse, so that the callers run the exact-fp32
// step-per-launch kernels: the A/B reference), PTMI_LSTM_DBG (timing ablations; the persistent kernels' bits are listed in
// csrc/lstm_split.hip, the step kernels': 1 no recurrent product, 2 no MFMA, 4 the other tile, 8 both row tiles: results
// void), PTMI_LSTM_MAX_POLLS (watchdog budget of the persistent kernels).
//
// Layouts (rows = packed time-major rows of the PackedSequence, row(t, b) = offs[t] + b):
//   gx / gates / dgates  [rows][ndir][4][H]   (pre-activations in, activations out: in place)
//   hy, c, dhy           [rows][ndir][H]
//   w_hh_pad             [ndir][4H][KP]       KP = H rounded up to 16, zero padded
//   w_hh_t               [ndir][H][4H]
#include <stdio.h>
#include <stdlib.h>

#include "common.h"
#include "lstm_common.h"

namespace ptmi {

// Per-direction bookkeeping of ONE timestep, computed on the host and passed as kernel arguments
// (a scalar load of batch_sizes[t] / offsets[t] from memory costs a cold round trip per launch).
struct StepMeta {
    long long row0[2];   // first packed row of this step's time index
    long long prow0[2];  // first packed row of the neighbouring time index (see kernels)
    long long qrow0[2];  // backward only: first row of the forward-sense predecessor
    int nb[2];           // active sequences at this time index
    int nprev[2];        // of those, how many are also active at the neighbouring time index
    int npv[2];          // backward only: how many have a forward-sense predecessor
};

struct LstmArgs {
    float* gx;
    float* hy;
    float* c;
    const float* w;
    int H, KP, ndir, dbg;
    StepMeta m;
    const float* c0;   // [ndir, max_batch, H] initial cell state of every sequence, or null (= 0)
    int max_batch;
};

// One forward timestep.  grid = (ceil(H / JT), ndir, ceil(maxB / 32)), NW * 64 threads.
// Workgroup tile: 32 batch rows x (4 gates x JT hidden units) = 32 x NC outputs, NC = 4 JT (16 or 32).
// K (= H, padded to KP) is split over the NW wavefronts; every wavefront issues the float4 loads of
// its whole K slice (CH 16-wide blocks) up front so that the L2 latency is paid once, not per block.
template <int JT, int NW, int CH>
__global__ __launch_bounds__(NW * 64) void lstm_fwd_step_kernel(const LstmArgs A) {
    constexpr int NC = 4 * JT;          // gate columns per workgroup
    constexpr int NT = NC / 16;         // MFMA tiles along the gate columns
    static_assert(NC % 16 == 0, "gate columns must fill MFMA tiles");
    const int dir = blockIdx.y;
    const int j0 = blockIdx.x * JT;
    const int m0 = blockIdx.z * 32;
    const int nb = A.m.nb[dir];
    if (m0 >= nb) return;
    const long long row0 = A.m.row0[dir];
    const int nprev = A.m.nprev[dir];
    const long long prow0 = A.m.prow0[dir];
    const int H = A.H, G = 4 * H;
    const long long ld_g = (long long)A.ndir * G, ld_h = (long long)A.ndir * H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g4 = lane >> 4, r = lane & 15;

    __shared__ float red[NW][32][NC + 1];
    const bool has_rec = nprev > m0 && !(A.dbg & 1);
    const int mtiles = (min(nprev, m0 + 32) - m0 + 15) >> 4;   // 1 or 2 live row tiles

    // epilogue operands first: their latency hides behind the GEMM
    const int bl = tid / JT, u = tid - bl * JT;
    const int b = m0 + bl;
    const bool act = tid < 32 * JT && b < nb && j0 + u < H;
    float pre[4] = {0.f, 0.f, 0.f, 0.f};
    float cprev = 0.f;
    float* gp = A.gx + (row0 + b) * ld_g + (long long)dir * G + j0 + u;
    if (act) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[q] = gp[q * H];
        if (b < nprev) cprev = A.c[(prow0 + b) * ld_h + dir * H + j0 + u];
        else if (A.c0) cprev = A.c0[((long long)dir * A.max_batch + b) * H + j0 + u];   // first step of sequence b
    }

    if (has_rec) {
        f32x4 acc[2][NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nblk = A.KP >> 4;
        const int per = (nblk + NW - 1) / NW;
        const int kb0 = wave * per;
        const int kb1 = min(nblk, kb0 + per);
        const float* ap[2];
        bool av[2];
        const float* bp[NT];
        bool bv[NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int i = m0 + mt * 16 + r;
            av[mt] = i < nprev;
            ap[mt] = A.hy + (prow0 + (av[mt] ? i : 0)) * ld_h + dir * H + 4 * g4;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int cidx = nt * 16 + r;
            const int gate = cidx / JT, uu = cidx - gate * JT;
            bv[nt] = j0 + uu < H;
            bp[nt] = A.w + ((long long)dir * G + gate * H + (bv[nt] ? j0 + uu : 0)) * A.KP + 4 * g4;
        }
        const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = kb0; kc < kb1; kc += CH) {
            f32x4 a[CH][2], bq[CH][NT];
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int kb = kc + i;
                const bool in = kb < kb1;
                const bool kin = in && (kb * 16 + 4 * g4 < H);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    a[i][mt] = (kin && av[mt]) ? *reinterpret_cast<const f32x4*>(ap[mt] + kb * 16) : zero;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    bq[i][nt] = (in && bv[nt]) ? *reinterpret_cast<const f32x4*>(bp[nt] + kb * 16) : zero;
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                if (kc + i < kb1 && !(A.dbg & 2)) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][0][q], bq[i][nt][q], acc[0][nt], 0, 0, 0);
                            if (mtiles > 1 || (A.dbg & 8))
                                acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][1][q], bq[i][nt][q], acc[1][nt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // C layout of mfma_f32_16x16x4: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int q = 0; q < 4; ++q) red[wave][mt * 16 + g4 * 4 + q][nt * 16 + r] = acc[mt][nt][q];
        __syncthreads();
        if (tid < 32 * JT) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cidx = q * JT + u;
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) s += red[w][bl][cidx];
                pre[q] += s;
            }
        }
    }
    if (act) {
        const float ig = sigmoidf_(pre[0]);
        const float fg = sigmoidf_(pre[1]);
        const float gg = tanhf_(pre[2]);
        const float og = sigmoidf_(pre[3]);
        const float cn = fg * cprev + ig * gg;
        const float h = og * tanhf_(cn);
        gp[0] = ig;
        gp[H] = fg;
        gp[2 * H] = gg;
        gp[3 * H] = og;
        const long long o = (row0 + b) * ld_h + dir * H + j0 + u;
        A.c[o] = cn;
        A.hy[o] = h;
    }
}

struct LstmBwdArgs {
    const float* gates;
    const float* c;
    const float* dhy;
    const float* wt;
    float* dg;
    float* dcs;
    int H, ndir;
    StepMeta m;
    const float* c0;
    int max_batch;
};

// One backward timestep.  grid = (ceil(H / 16), ceil(maxB / 16), ndir), NW * 64 threads.
// Workgroup tile: 16 batch rows x 16 hidden units of dh_rec = dgates_{next} W_hh, K = 4H split
// over NW wavefronts (each issues its whole K slice of float4 loads up front).
template <int NW, int CH>
__global__ __launch_bounds__(NW * 64) void lstm_bwd_step_kernel(const LstmBwdArgs A) {
    const int dir = blockIdx.z;
    const int n0 = blockIdx.x * 16;
    const int m0 = blockIdx.y * 16;
    const int nb = A.m.nb[dir];
    if (m0 >= nb) return;
    const long long row0 = A.m.row0[dir];
    // "next" = the time index the previous launch processed (its dgates feed dh_rec);
    // "pv"   = the forward pass' predecessor (for c_{t-1})
    const int nnext = A.m.nprev[dir], npv = A.m.npv[dir];
    const long long nrow0 = A.m.prow0[dir], prow0 = A.m.qrow0[dir];
    const int H = A.H, G = 4 * H;
    const long long ld_g = (long long)A.ndir * G, ld_h = (long long)A.ndir * H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g4 = lane >> 4, r = lane & 15;

    __shared__ float red[NW][16][17];
    const bool has_rec = nnext > m0;
    const int bl = (tid >> 4) & 15, jl = tid & 15;
    const int b = m0 + bl, j = n0 + jl;
    const bool act = tid < 256 && b < nb && j < H;

    // epilogue operands first
    float dh = 0.f, dc = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, cn = 0.f, cprev = 0.f;
    const long long oh = (row0 + b) * ld_h + dir * H + j;
    const long long og_ = (row0 + b) * ld_g + (long long)dir * G + j;
    float* dcs = A.dcs + ((long long)b * A.ndir + dir) * H + j;
    if (act) {
        dh = A.dhy[oh];
        if (b < nnext) dc = *dcs;      // rows without a successor step start from dc = 0 (no memset needed)
        ig = A.gates[og_];
        fg = A.gates[og_ + H];
        gg = A.gates[og_ + 2 * H];
        og = A.gates[og_ + 3 * H];
        cn = A.c[oh];
        if (b < npv) cprev = A.c[(prow0 + b) * ld_h + dir * H + j];
        else if (A.c0) cprev = A.c0[((long long)dir * A.max_batch + b) * H + j];
    }

    if (has_rec) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nblk = G >> 4;
        const int per = (nblk + NW - 1) / NW;
        const int kb0 = wave * per;
        const int kb1 = min(nblk, kb0 + per);
        const bool av = m0 + r < nnext;
        const bool bv = n0 + r < H;
        const float* ap = A.dg + (nrow0 + (av ? m0 + r : 0)) * ld_g + (long long)dir * G + 4 * g4;
        const float* bp = A.wt + ((long long)dir * H + (bv ? n0 + r : 0)) * G + 4 * g4;
        const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kc = kb0; kc < kb1; kc += CH) {
            f32x4 a[CH], bq[CH];
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const bool in = kc + i < kb1;
                a[i] = (in && av) ? *reinterpret_cast<const f32x4*>(ap + (kc + i) * 16) : zero;
                bq[i] = (in && bv) ? *reinterpret_cast<const f32x4*>(bp + (kc + i) * 16) : zero;
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][q], bq[i][q], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][g4 * 4 + q][r] = acc[q];
        __syncthreads();
        if (tid < 256 && b < nnext) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += red[w][bl][jl];
            dh += s;
        }
    }
    if (act) {
        const float tc = tanhf_(cn);
        const float d_o = dh * tc;
        dc += dh * og * (1.f - tc * tc);
        const float d_i = dc * gg;
        const float d_g = dc * ig;
        const float d_f = dc * cprev;
        *dcs = dc * fg;
        float* dgp = A.dg + og_;
        dgp[0] = d_i * ig * (1.f - ig);
        dgp[H] = d_f * fg * (1.f - fg);
        dgp[2 * H] = d_g * (1.f - gg * gg);
        dgp[3 * H] = d_o * og * (1.f - og);
    }
}

static void neighbour(const int32_t* bs, const int64_t* offs, int T, int t, int tn, int* n, long long* row) {
    *n = 0;
    *row = 0;
    if (tn >= 0 && tn < T) {
        *n = bs[tn] < bs[t] ? bs[tn] : bs[t];
        *row = offs[tn];
    }
}

// Enqueue the T forward step kernels on `st` (eagerly, or into a stream capture).
static int enqueue_forward(float* gates, float* hy, float* c, const float* c0, const float* w_hh_pad, const int32_t* batch_sizes,
                           const int64_t* offsets, int T, int max_batch, int H, int KP, int ndir, hipStream_t st) {
    const char* dbg_env = getenv("PTMI_LSTM_DBG");
    const int dbg = dbg_env ? atoi(dbg_env) : 0;
    LstmArgs A{gates, hy, c, w_hh_pad, H, KP, ndir, dbg, {}, c0, max_batch};
    // JT = 8 (32 gate columns per workgroup) reads h_{t-1} from half as many workgroups as JT = 4;
    // measured faster at H = 600 (9.4 vs 10.3 us per step, B = 32) because the step is bound by
    // operand traffic, not by the matrix cores.  JT = 4 only when H is too small to fill the chip.
    const unsigned mz = (unsigned)((max_batch + 31) / 32);
    bool small_tiles = (long long)((H + 7) / 8) * ndir * mz < 64;
    if (dbg & 4) small_tiles = !small_tiles;
    for (int s = 0; s < T; ++s) {
        for (int d = 0; d < ndir; ++d) {
            const int t = d == 0 ? s : T - 1 - s;          // direction 1 walks time backwards
            A.m.nb[d] = batch_sizes[t];
            A.m.row0[d] = offsets[t];
            neighbour(batch_sizes, offsets, T, t, d == 0 ? t - 1 : t + 1, &A.m.nprev[d], &A.m.prow0[d]);
        }
        if (small_tiles)
            hipLaunchKernelGGL((lstm_fwd_step_kernel<4, 8, 5>), dim3((unsigned)((H + 3) / 4), (unsigned)ndir, mz),
                               dim3(512), 0, st, A);
        else
            hipLaunchKernelGGL((lstm_fwd_step_kernel<8, 8, 5>), dim3((unsigned)((H + 7) / 8), (unsigned)ndir, mz),
                               dim3(512), 0, st, A);
    }
    return launch_status();
}

static int enqueue_backward(const float* gates, const float* c, const float* c0, const float* dhy, const float* w_hh_t,
                            float* dgates, float* dc_state, const int32_t* batch_sizes, const int64_t* offsets,
                            int T, int max_batch, int H, int ndir, hipStream_t st) {
    LstmBwdArgs A{gates, c, dhy, w_hh_t, dgates, dc_state, H, ndir, {}, c0, max_batch};
    const dim3 grid((unsigned)((H + 15) / 16), (unsigned)((max_batch + 15) / 16), (unsigned)ndir);
    for (int s = 0; s < T; ++s) {
        for (int d = 0; d < ndir; ++d) {
            const int t = d == 0 ? T - 1 - s : s;          // reverse of the forward order
            A.m.nb[d] = batch_sizes[t];
            A.m.row0[d] = offsets[t];
            neighbour(batch_sizes, offsets, T, t, d == 0 ? t + 1 : t - 1, &A.m.nprev[d], &A.m.prow0[d]);
            neighbour(batch_sizes, offsets, T, t, d == 0 ? t - 1 : t + 1, &A.m.npv[d], &A.m.qrow0[d]);
        }
        hipLaunchKernelGGL((lstm_bwd_step_kernel<16, 10>), grid, dim3(1024), 0, st, A);
    }
    return launch_status();
}

}  // namespace ptmi

using namespace ptmi;

// compute units of the current device (the residency limits of the persistent kernels derive from it)
static int cu_count() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// Per-device word that counts timed-out persistent launches (set once by the host binding; see ptmi_lstm_set_error_sink).
static unsigned* g_error_sink[64] = {};
static unsigned* error_sink() {
    int dev = 0;
    return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) ? g_error_sink[dev] : nullptr;
}

extern "C" {

int ptmi_lstm_forward(float* gates, float* hy, float* c, const float* c0, const float* w_hh_pad, const int32_t* batch_sizes,
                      const int64_t* offsets, int32_t T, int32_t max_batch, int32_t H, int32_t KP,
                      int32_t ndir, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gates || !hy || !c || !w_hh_pad || !batch_sizes || !offsets, PTMI_E_INVALID);
    PTMI_RETURN_IF(T < 0 || max_batch < 1 || H < 1 || (ndir != 1 && ndir != 2), PTMI_E_INVALID);
    PTMI_RETURN_IF(H % 4 != 0 || KP % 16 != 0 || KP < H, PTMI_E_UNSUPPORTED);
    return enqueue_forward(gates, hy, c, c0, w_hh_pad, batch_sizes, offsets, T, max_batch, H, KP, ndir,
                           static_cast<hipStream_t>(stream));
}

int ptmi_lstm_backward(const float* gates, const float* c, const float* c0, const float* dhy, const float* w_hh_t, float* dgates,
                       float* dc_state, const int32_t* batch_sizes, const int64_t* offsets, int32_t T,
                       int32_t max_batch, int32_t H, int32_t ndir, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!gates || !c || !dhy || !w_hh_t || !dgates || !dc_state || !batch_sizes || !offsets,
                   PTMI_E_INVALID);
    PTMI_RETURN_IF(T < 0 || max_batch < 1 || H < 1 || (ndir != 1 && ndir != 2), PTMI_E_INVALID);
    PTMI_RETURN_IF(H % 4 != 0, PTMI_E_UNSUPPORTED);
    return enqueue_backward(gates, c, c0, dhy, w_hh_t, dgates, dc_state, batch_sizes, offsets, T, max_batch, H, ndir,
                            static_cast<hipStream_t>(stream));
}

// ---- host side of the persistent recurrence (kernels: csrc/lstm_split.hip) -----------------------------------------------

int64_t ptmi_lstm_flags_elems(int32_t T, int32_t ndir, int32_t max_batch) {
    (void)T;
    return (int64_t)ndir * ((max_batch + 15) / 16) * kSlots + 8;   // kSlots reserved words per chain of 16 rows + error words
}

static int round32(int n) { return (n + 31) / 32 * 32; }

// tile-major hand-off copy: [T][16-row tiles][ndir][cols / 16] tiles of 16 x 16 floats
static int64_t lstm_tile_elems(int32_t T, int32_t ndir, int32_t max_batch, int32_t cols) {
    return (int64_t)T * ((max_batch + 15) / 16) * ndir * cols * 16;
}

// the words behind the backward planes: [ndir][4H] bias sums, 8 words (word 0: max |dgates|), reserved + error words
static int64_t bwd_tail_elems(int32_t T, int32_t ndir, int32_t max_batch, int32_t H) {
    return (int64_t)ndir * 4 * H + 8 + ptmi_lstm_flags_elems(T, ndir, max_batch);
}

int64_t ptmi_lstm_scratch_elems(int32_t T, int32_t ndir, int32_t max_batch, int32_t H, int32_t backward) {
    // [tile-major hand-off copy (columns rounded up to 32) | backward: bias gradient [ndir][4H] + 8 words | reserved words | 8 error words]
    return backward ? lstm_tile_elems(T, ndir, max_batch, round32(4 * H)) + bwd_tail_elems(T, ndir, max_batch, H)
                    : lstm_tile_elems(T, ndir, max_batch, round32(H)) + ptmi_lstm_flags_elems(T, ndir, max_batch);
}

int ptmi_lstm_set_error_sink(uint32_t* word) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    PTMI_RETURN_IF(dev < 0 || dev >= 64, PTMI_E_UNSUPPORTED);
    g_error_sink[dev] = word;
    return PTMI_OK;
}

int ptmi_lstm_split_enabled(void) { return getenv("PTMI_LSTM_F32") ? 0 : 1; }

// What a plan can be made for at all (the queries answer 0 for everything else; the entries refuse it with a code of their own).
static bool plannable(int T, int ndir, int max_batch, int64_t rows, int H) {
    return T >= 1 && max_batch >= 1 && rows >= 1 && H >= 1 && H % 4 == 0 && (ndir == 1 || ndir == 2) && ptmi_lstm_split_enabled();
}

// The persistent BACKWARD launch of one configuration.  Everything the launcher and the queries know about its geometry is here.
struct BwdPlan {
    bool ok;           // the persistent kernels run this configuration (else: the step-per-launch kernels)
    int G32;           // hand-off columns per direction, 4H rounded up to 32; 0: no persistent kernel for a layer of this width
    int mtl;           // 16-row tiles per workgroup
    int ntiles;        // row tiles (16 mtl rows) of the whole batch
    int nx;            // unit tiles (16 hidden units) = workgroups of a chain (direction x row tile)
    int per_launch;    // row tiles per launch
    bool planes;       // the launch can emit dgates^T as bf16 planes
};

static BwdPlan bwd_plan(int T, int ndir, int max_batch, int64_t rows, int H) {
    BwdPlan p{};
    if (!plannable(T, ndir, max_batch, rows, H)) return p;
    constexpr int NW = 8, CB = 10;            // lstm_bwd_split_kernel: wavefronts, resident k blocks of 32 per wavefront
    const int G32 = round32(4 * H);
    if ((G32 / 32 + NW - 1) / NW > CB) return p;
    p.G32 = G32;
    // One workgroup per CU must be resident (at most 240 per launch: a margin of 16).  Row tiles are independent recurrences,
    // so a batch whose tiles do not fit at once runs as several launches over groups of tiles; before that,
    // 16-row chains become 32-row chains (MTL = 2: one launch up to batch 64 at H = 600; 7.5 us per step instead of 2 x 5.0).
    const int resident = cu_count() - 16;
    p.nx = (H + 15) / 16;
    if ((long long)p.nx * ndir > resident || p.nx > kSlots) return p;
    const int nt16 = (max_batch + 15) / 16, fit = resident / (p.nx * ndir);
    p.mtl = nt16 > fit ? 2 : 1;
    p.ntiles = (nt16 + p.mtl - 1) / p.mtl;
    p.per_launch = std::min(p.ntiles, fit);
    p.planes = rows == (int64_t)T * max_batch && max_batch % 16 == 0;          // equal lengths, whole 16-row tiles
    p.ok = true;
    return p;
}

// The persistent FORWARD launch of one configuration.
struct FwdPlan {
    bool ok;           // as in BwdPlan
    int KP32;          // hand-off columns per direction, H rounded up to 32; 0: no persistent kernel for a layer of this width
    int jt, mtl;       // workgroup tile: jt hidden units x 16 mtl rows
    int ntiles;        // row tiles (16 mtl rows) of the whole batch
    int jx;            // unit tiles = workgroups of a chain
    int per_launch;    // row tiles per launch
    int fills;         // what the launch writes into this layer's BACKWARD scratch on the side (the `prefilled` of the backward
                       // call): 2 = the pattern into its planes and zeros into the words behind them, 0 = nothing
};

static FwdPlan fwd_plan(int T, int ndir, int max_batch, int64_t rows, int H) {
    FwdPlan p{};
    if (!plannable(T, ndir, max_batch, rows, H)) return p;
    constexpr int NW = 8, CB = 3;             // lstm_fwd_daf_kernel: wavefronts, resident k blocks of 32 per wavefront
    const int KP32 = round32(H);
    if ((KP32 / 32 + NW - 1) / NW > CB) return p;
    p.KP32 = KP32;
    const int cus = cu_count();
    // Workgroup tile (rows x hidden units), measured forward us per step at H = 600, T = 253:
    //   B <= 16: 16 x 8 (4.9);  B <= 32: two independent chains of 16 x 12 on separate CUs (200 workgroups:
    //   5.4; 16 x 16 on 152: 5.8; 32 x 8: 6.6; 16 x 8 with 300 workgroups sharing CUs: 8.3);
    //   B > 32: 32 x 12 (B = 64: 32 x 16 8.8, 32 x 8 11.6).
    // One 16-row tile per workgroup: 16 units (38 instead of 50 workgroups per chain at H = 600) measured 2.55 against 2.48 us
    // per step for 12 - they only step in where 12-unit tiles do not fit one workgroup per CU, 8 where those do not either.
    p.jt = max_batch <= 16 ? 8 : 12;
    p.mtl = max_batch <= 32 ? 1 : 2;
    if (p.jt == 12 && (long long)((H + 11) / 12) * ndir > cus) p.jt = 16;
    if (p.jt == 16 && (long long)((H + 15) / 16) * ndir > cus) p.jt = 8;
    p.ntiles = (max_batch + 16 * p.mtl - 1) / (16 * p.mtl);
    p.jx = (H + p.jt - 1) / p.jt;
    // 8-unit tiles (512 threads at <= 128 VGPRs) fit 2 per CU, with a margin below 2 x; 12 / 16-unit tiles need the whole
    // register file: one workgroup per CU
    const int cap = p.jt >= 12 ? cus : cus * 7 / 4;
    if ((long long)p.jx * ndir > cap || p.jx > kSlots) return p;
    // row tiles are independent recurrences: a batch whose tiles do not all fit runs as several launches
    p.per_launch = std::min(p.ntiles, cap / (p.jx * ndir));
    // the data-as-flag kernels exist for these tiles, and run one workgroup per CU
    if (!fwd_split_instantiated(p.jt, p.mtl) || (long long)p.jx * ndir * p.per_launch > cus) return p;
    p.ok = true;
    // the fill of the backward planes: ONE forward launch (all row tiles resident at once) whose workgroups have a wavefront
    // without elements, and a backward kernel that reads the pattern for this width
    if ((long long)p.jx * ndir * p.ntiles <= cus && 16 * p.mtl * p.jt <= 7 * 64 && bwd_plan(T, ndir, max_batch, rows, H).G32) p.fills = 2;
    return p;
}

int32_t ptmi_lstm_handoff_cols(int32_t H, int32_t backward) {        // (a rule of the layer's width alone)
    return backward ? bwd_plan(1, 1, 1, 1, H).G32 : fwd_plan(1, 1, 1, 1, H).KP32;
}

int ptmi_lstm_forward_fills(int32_t T, int32_t ndir, int32_t max_batch, int32_t H) {
    return fwd_plan(T, ndir, max_batch, (int64_t)T * max_batch, H).fills;
}

int32_t ptmi_lstm_backward_planes_ok(int32_t T, int32_t ndir, int32_t max_batch, int64_t rows, int32_t H) {
    const BwdPlan p = bwd_plan(T, ndir, max_batch, rows, H);
    return p.ok && p.planes ? 1 : 0;
}

static int env_int(const char* name, int fallback) {
    const char* v = getenv(name);
    return v ? atoi(v) : fallback;
}

int ptmi_lstm_forward_persistent(float* gates, float* hy, float* c, const float* c0, const float* w_hh_pad,
                                 const uint32_t* w_hh_amax, const int32_t* batch_sizes_dev, const int64_t* offsets_dev,
                                 const uint64_t* step_masks, uint32_t* flags, int32_t T, int32_t max_batch, int64_t rows,
                                 int32_t H, int32_t KP, int32_t ndir, int32_t prefilled, uint32_t* backward_scratch,
                                 ptmi_stream_t stream) {
    // the contract (include/ptmi.h), in full before the first enqueue
    PTMI_RETURN_IF(!gates || !hy || !c || !w_hh_pad || !batch_sizes_dev || !offsets_dev || !flags, PTMI_E_INVALID);
    PTMI_RETURN_IF(T < 1 || max_batch < 1 || H < 1 || (ndir != 1 && ndir != 2) || rows < 1, PTMI_E_INVALID);
    const bool uniform = rows == (int64_t)T * max_batch;         // batch sizes never grow: equal lengths
    // row slots: every (time index, slot) row exists in the buffers; at most 64 slots (one mask word per step and kind)
    PTMI_RETURN_IF(step_masks && (c0 || !uniform || max_batch > 64), PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(H % 4 != 0 || KP != (H + 15) / 16 * 16, PTMI_E_UNSUPPORTED);
    const FwdPlan P = fwd_plan(T, ndir, max_batch, rows, H);
    PTMI_RETURN_IF(!P.ok, PTMI_E_UNSUPPORTED);                      // the caller falls back to the step-per-launch kernels
    const long long hy_bytes = rows * ndir * H * 4;
    PTMI_RETURN_IF(hy_bytes > 0x7fffffffLL, PTMI_E_UNSUPPORTED);

    hipStream_t st = static_cast<hipStream_t>(stream);
    // scratch = [hand-off planes of hy | reserved words | 8 error words]: every 16-bit value of the planes starts as 0xFFFF (no value can
    // be), the words behind them as zero - one launch, unless the caller has filled the planes
    const int64_t plane_elems = lstm_tile_elems(T, ndir, max_batch, P.KP32), flag_elems = ptmi_lstm_flags_elems(T, ndir, max_batch);
    float* const hyt = reinterpret_cast<float*>(flags);
    flags += plane_elems;
    if (!prefilled) {
        int fe = daf_fill_and_zero(hyt, (size_t)plane_elems, flags, (size_t)flag_elems, st);
        if (fe) return fe;
    } else {
        hipError_t e = zero_words_async(flags, (size_t)flag_elems, st);
        if (e != hipSuccess) return (int)e;
    }
    LstmPersistArgs A{gates, hy, c, w_hh_pad, batch_sizes_dev, offsets_dev, flags, T, H, KP, ndir,
                      (unsigned)P.jx, (unsigned)env_int("PTMI_LSTM_MAX_POLLS", 1 << 22), (int)hy_bytes, (unsigned)(flag_elems - 8),
                      env_int("PTMI_LSTM_DBG", 0), 0, P.ntiles, c0, max_batch, hyt, (max_batch + 15) / 16, w_hh_amax, P.KP32};
    A.err_sink = error_sink();
    A.uniform = uniform ? 1 : 0;
    A.masks = reinterpret_cast<const unsigned long long*>(step_masks);
    if (backward_scratch && P.fills) {     // this layer's backward planes get their pattern here, the words behind them zeros
        A.fill_ptr = reinterpret_cast<uint4*>(backward_scratch);
        A.fill_n16 = (unsigned long long)lstm_tile_elems(T, ndir, max_batch, bwd_plan(T, ndir, max_batch, rows, H).G32) / 4;
        A.zero_n16 = (unsigned long long)bwd_tail_elems(T, ndir, max_batch, H) / 4;          // a multiple of 4 words (kSlots is)
    }
    const int cus = cu_count();
    for (int t0 = 0; t0 < P.ntiles; t0 += P.per_launch) {
        A.tile0 = t0;
        A.nx = P.jx;
        A.nt = std::min(P.per_launch, P.ntiles - t0);
        // the workgroups of a chain (direction x row tile) on 8 / chains neighbouring XCDs, as in the backward kernel (a chain's
        // hand-off rows then live in the L2s of those XCDs only): a 1-D grid; else (unit tile, direction, row tile)
        const int chains = ndir * A.nt;
        A.span = (chains <= 8 && 8 % chains == 0 && (P.jx + 8 / chains - 1) / (8 / chains) * 8 <= cus) ? 8 / chains : 0;
        const dim3 grid = A.span ? dim3((unsigned)((P.jx + A.span - 1) / A.span * 8))
                                 : dim3((unsigned)P.jx, (unsigned)ndir, (unsigned)A.nt);
        int rc = launch_fwd_split(A, P.jt, P.mtl, grid, st);
        if (rc) return rc;
    }
    return PTMI_OK;
}

// the half k block behind the last packed row (rows % 32 == 16) of every column tile and plane: zero
__global__ void zero_tp_tail_kernel(uint4* planes, long long tiles, int kb_total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // (tile, plane, chunk 32..63)
    if (i >= tiles * 64) return;
    const long long tile = i >> 6;
    const int plane = (int)(i >> 5) & 1, ch = 32 + (int)(i & 31);
    planes[((tile * kb_total + kb_total - 1) * 2 + plane) * 64 + ch] = make_uint4(0u, 0u, 0u, 0u);
}

int ptmi_lstm_backward_persistent(const float* gates, const float* c, const float* c0, const float* dhy, const float* dc_n,
                                  const float* w_hh_t, float* dgates, uint16_t* dgates_t, const int32_t* batch_sizes_dev,
                                  const int64_t* offsets_dev, const uint64_t* step_masks, uint32_t* flags, float* dc_carry,
                                  int32_t T, int32_t max_batch, int64_t rows, int32_t H, int32_t ndir, int32_t s_begin,
                                  int32_t s_end, int32_t prefilled, ptmi_stream_t stream) {
    // the contract (include/ptmi.h), in full before the first enqueue
    PTMI_RETURN_IF(!gates || !c || !dhy || !w_hh_t || !batch_sizes_dev || !offsets_dev || !flags, PTMI_E_INVALID);
    PTMI_RETURN_IF(T < 1 || max_batch < 1 || H < 1 || (ndir != 1 && ndir != 2) || rows < 1, PTMI_E_INVALID);
    PTMI_RETURN_IF(!dgates && !dgates_t, PTMI_E_INVALID);
    PTMI_RETURN_IF(dgates_t && (reinterpret_cast<uintptr_t>(dgates_t) & 15) != 0, PTMI_E_INVALID);
    PTMI_RETURN_IF(s_begin < 0 || s_end > T || s_begin >= s_end, PTMI_E_INVALID);
    const bool whole = s_begin == 0 && s_end == T;
    PTMI_RETURN_IF(!whole && (!dc_carry || dc_n), PTMI_E_INVALID);
    const bool uniform = rows == (int64_t)T * max_batch;
    PTMI_RETURN_IF(dc_n && step_masks, PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(step_masks && (c0 || !uniform || max_batch > 64 || !whole), PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF(H % 4 != 0, PTMI_E_UNSUPPORTED);
    const BwdPlan P = bwd_plan(T, ndir, max_batch, rows, H);
    PTMI_RETURN_IF(!P.ok, PTMI_E_UNSUPPORTED);                      // the caller falls back to the step-per-launch kernels
    PTMI_RETURN_IF(dgates_t && !P.planes, PTMI_E_UNSUPPORTED);
    const long long dg_bytes = rows * ndir * 4 * H * 4;
    PTMI_RETURN_IF(dg_bytes > 0x7fffffffLL, PTMI_E_UNSUPPORTED);

    hipStream_t st = static_cast<hipStream_t>(stream);
    // scratch = [hand-off planes of dgates | bias gradient [ndir][4H] | 8 words, word 0: max |dgates| | reserved words | 8 error words].
    // The first range sets it up in one launch - the planes start as the fill pattern, the words behind them as zero -, unless the
    // caller (prefilled = 1: planes) or the forward launch (2: the words too, FwdPlan::fills) has; a later range continues on the
    // first one's bias sums and maximum.
    const int64_t plane_elems = lstm_tile_elems(T, ndir, max_batch, P.G32), tail_elems = bwd_tail_elems(T, ndir, max_batch, H);
    float* const dgt = reinterpret_cast<float*>(flags);
    flags += plane_elems;
    float* const dbias = reinterpret_cast<float*>(flags);
    if (s_begin == 0 && !prefilled) {
        int fe = daf_fill_and_zero(dgt, (size_t)plane_elems, flags, (size_t)tail_elems, st);
        if (fe) return fe;
    } else if (s_begin == 0 && prefilled != 2) {
        hipError_t e = zero_words_async(flags, (size_t)tail_elems, st);
        if (e != hipSuccess) return (int)e;
    }
    flags += ndir * 4 * H;
    uint32_t* const dg_amax = flags;
    flags += 8;
    const int nt16 = (max_batch + 15) / 16;
    LstmPersistBwdArgs A{gates, c, dhy, w_hh_t, dgates, batch_sizes_dev, offsets_dev, flags, T, H, ndir,
                         (unsigned)P.nx, (unsigned)env_int("PTMI_LSTM_MAX_POLLS", 1 << 22), (int)dg_bytes,
                         (unsigned)(ptmi_lstm_flags_elems(T, ndir, max_batch) - 8), 0, P.ntiles, env_int("PTMI_LSTM_DBG", 0), c0, max_batch,
                         0, 0, 0, dgt, nt16, dbias, dg_amax, P.G32};
    A.err_sink = error_sink();
    A.uniform = uniform ? 1 : 0;
    A.masks = reinterpret_cast<const unsigned long long*>(step_masks);
    A.dcn = dc_n;
    A.s_begin = s_begin;
    A.s_end = s_end;
    A.dc_carry = dc_carry;
    if (dgates_t) {
        // the planes hold the rows of THIS launch's step range: (s_end - s_begin) * max_batch packed rows per direction, from
        // time index T - s_end on (forward direction: processed last to first) / s_begin on (reverse direction)
        const int64_t range_rows = (int64_t)(s_end - s_begin) * max_batch;
        A.dgtp = reinterpret_cast<uint4*>(dgates_t);
        A.tp_kb = (int)((range_rows + 31) / 32);
        A.tp_dir_stride = (long long)(4 * H / 16) * A.tp_kb * 2 * 64;
        A.tp_row0[0] = (long long)(T - s_end) * max_batch;
        A.tp_row0[1] = (long long)s_begin * max_batch;
        if (range_rows % 32 != 0) {
            const long long tiles = (long long)ndir * (4 * H / 16);
            hipLaunchKernelGGL(zero_tp_tail_kernel, dim3((unsigned)((tiles * 64 + 255) / 256)), dim3(256), 0, st, A.dgtp, tiles, A.tp_kb);
            int rc = launch_status();
            if (rc) return rc;
        }
    }
    for (int t0 = 0; t0 < P.ntiles; t0 += P.per_launch) {
        A.tile0 = t0;
        A.nx = P.nx;
        A.nt = std::min(P.per_launch, P.ntiles - t0);
        const int chains = A.nt * ndir;
        A.span = (chains <= 8 && 8 % chains == 0) ? 8 / chains : 0;        // XCDs per chain (chain_tile)
        const unsigned nwg = A.span ? (unsigned)((P.nx + A.span - 1) / A.span * 8) : (unsigned)(P.nx * chains);
        int rc = launch_bwd_split(A, P.mtl, nwg, st);
        if (rc) return rc;
    }
    return PTMI_OK;
}

}  // extern "C"
