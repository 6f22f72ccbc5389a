// Shared pieces of the (B)LSTM recurrence: the gate non-linearities (csrc/lstm.hip: step-per-launch kernels, csrc/lstm_split.hip:
// persistent kernels) and the argument blocks / launch interface between the host side of the persistent recurrence (csrc/lstm.hip)
// and its kernels (csrc/lstm_split.hip).
#pragma once
#include "common.h"

namespace ptmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Gate non-linearities on the hardware transcendentals (v_exp_f32 / v_rcp_f32, about 1 ulp each): they
// sit on the serial chain of every time step, where the library expf / tanhf / IEEE division cost about
// 0.4 us per step.  Absolute error < 2e-7 (checked against torch's CPU LSTM in tests/test_gpu_lstm.py).
__device__ __forceinline__ float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float tanhf_(float x) {
    const float t = __builtin_amdgcn_exp2f(-2.8853900817779268f * fabsf(x));       // exp(-2|x|)
    return copysignf((1.f - t) * __builtin_amdgcn_rcpf(1.f + t), x);
}

// (expected, hy_bytes / dg_bytes and ntiles of the two blocks are read by no kernel any more.  They keep their places: without them
//  the compiler schedules the argument loads, and with them registers, differently in every persistent kernel.)
struct LstmPersistArgs {
    float* gx;
    float* hy;
    float* c;
    const float* w;
    const int32_t* bs;       // device [T]
    const int64_t* offs;     // device [T]
    unsigned* flags;         // device: the words behind the hand-off planes (zeroed per call), the last 8 of them the error words
    int T, H, KP, ndir;
    unsigned expected;       // producer workgroups per chain (direction x row tile)
    unsigned max_polls;
    int hy_bytes;
    unsigned err_off;        // index of the error words in flags
    int dbg;                 // PTMI_LSTM_DBG timing ablations (bits: csrc/lstm_split.hip)
    int tile0, ntiles;       // first row tile of this launch / row tiles of the whole batch
    const float* c0;         // [ndir, max_batch, H] initial cell state or null
    int max_batch;
    float* hyt;              // tile-major copy of hy for the hand-off: [T][16-row tile][dir][KP / 16][16 rows][16]
    int nt16;                // 16-row tiles of the whole batch
    const unsigned* w_amax;  // split kernels: float bits of max |W_hh| (device) or null
    int KP32;                // split kernels: H rounded up to 32
    unsigned* err_sink = nullptr;   // per-device count of timed-out launches (ptmi_lstm_set_error_sink) or null
    // split kernels, 1-D grid with the workgroups of a chain on `span` neighbouring XCDs (chain_tile below); span 0: the
    // 3-D grid (unit tile, direction, row tile) in dispatch order
    int nx = 0, nt = 0, span = 0;
    int uniform = 0;         // split kernels: all sequences have the same length (bs[t] = max_batch, offs[t] = t max_batch)
    // data-as-flag forward kernel: `fill_n16` 16-byte units from `fill_ptr` on (the hand-off planes of this layer's BACKWARD
    // scratch) get the fill pattern from an otherwise idle wavefront, a slice per workgroup and step
    uint4* fill_ptr = nullptr;
    unsigned long long fill_n16 = 0;
    // ... and the `zero_n16` 16-byte units BEHIND them (the backward scratch's bias sums, maximum word, reserved words and error words)
    // get zeros the same way (round 6): the backward launch then has nothing to enqueue in front of its recurrence kernel
    unsigned long long zero_n16 = 0;
    // Row-slot batches (data-as-flag kernels; layout = uniform [T][max_batch] rows, max_batch <= 64 slots): several sequences lie END TO
    // END in one row slot, so "row b is alive at step t" and "row b has a predecessor" are no prefix rules any more.  masks[3 t + 0]
    // = rows alive at time index t, + 1 = rows whose sequence STARTS at t (no predecessor in the forward direction), + 2 = rows whose
    // sequence ENDS at t (no predecessor in the reverse direction); bit b = row b.  Null: the PackedSequence rules (bs / offs).
    const unsigned long long* masks = nullptr;
};

// Most workgroups a chain (direction x row tile) may have.  The scratch still reserves this many words per chain behind the
// planes (ptmi_lstm_flags_elems: the slots of the former flag protocol, unread by today's kernels) in front of its 8 error words.
constexpr int kSlots = 128;

struct LstmPersistBwdArgs {
    const float* gates;
    const float* c;
    const float* dhy;
    const float* wt;
    float* dg;
    const int32_t* bs;
    const int64_t* offs;
    unsigned* flags;
    int T, H, ndir;
    unsigned expected;
    unsigned max_polls;
    int dg_bytes;
    unsigned err_off;
    int tile0, ntiles;   // first 16-row tile of this launch / tiles of the whole batch
    int dbg;             // PTMI_LSTM_DBG timing ablations (as in the forward kernel)
    const float* c0;
    int max_batch;
    int nx, nt, span;    // 1-D grid: unit tiles, row tiles of this launch, XCDs per chain (0: plain order)
    float* dgt;          // tile-major copy of dgates for the hand-off: [T][16-row tile][dir][4H / 16][16 rows][16]
    int nt16;            // 16-row tiles of the whole batch
    float* dbias;        // [ndir][4H] sum of dgates over all rows (zeroed by the host call, accumulated atomically)
    unsigned* dg_amax;   // split kernels: float bits of max |dgates| (zeroed by the host call, atomicMax)
    int G32;             // split kernels: 4H rounded up to 32
    unsigned* err_sink = nullptr;   // as in LstmPersistArgs
    // split kernels: this launch runs the processing steps [s_begin, s_end) of the T steps (a recurrence cut into several
    // launches lets the weight-gradient GEMMs of the finished time range start under the rest); the cell-state
    // gradient crosses the cut through dc_carry [ndir][max_batch][H] (written when s_end < T, read when s_begin > 0)
    int s_begin = 0, s_end = -1;
    float* dc_carry = nullptr;
    int uniform = 0;         // as in LstmPersistArgs
    // split kernels, equal lengths, batch a multiple of 16: dgates^T as bf16 (hi, lo) planes for the weight-gradient GEMMs
    // ([ndir][4H / 16][tp_kb][2][64] chunks of 16 B; null: not written); with them `dg` may be null
    uint4* dgtp = nullptr;
    long long tp_dir_stride = 0;      // chunks per direction
    int tp_kb = 0;                    // k blocks (32 packed rows) per column tile
    long long tp_row0[2] = {0, 0};    // first packed row of this launch's step range per direction: the planes' k index 0
    const unsigned long long* masks = nullptr;      // row-slot batches: as in LstmPersistArgs
    // gradient w.r.t. the FINAL cell state c_n [ndir][max_batch][H] (or null): enters the cell-state gradient of every sequence's
    // last step in the direction's forward sense = the first step this pass processes for it
    const float* dcn = nullptr;
};

// Workgroup L of a 1-D grid runs on XCD L % 8 (round-robin dispatch).  A chain = (direction, row tile)
// exchanges its operand rows among its own workgroups every step; they are written through one XCD's L2
// and read over the fabric by the others, which is what bounds the hand-off at batch >= 16.  With
// `span` = 8 / chains XCDs per chain, a chain's workgroups sit on `span` neighbouring XCDs instead of all
// eight, so 1/span of what a workgroup reads is local.  Returns false for the padding workgroups.
__device__ __forceinline__ bool chain_tile(int nx, int nt, int span, int* x, int* y, int* dir, int nchains = 1 << 30) {
    const int L = blockIdx.x;
    int chain;
    if (span > 0) {
        const int xcd = L & 7;
        chain = xcd / span;
        *x = (L >> 3) * span + (xcd - chain * span);
        if (*x >= nx || chain >= nchains) return false;
    } else {
        *x = L % nx;
        chain = L / nx;
    }
    *y = chain % nt;
    *dir = chain / nt;
    return true;
}

// MTL = 16-row tiles per workgroup (2: a batch of 64 stays ONE launch of 32-row chains; the weights in
// registers serve both tiles, the second tile's operands are requested while the first one multiplies).

// csrc/lstm_split.hip
bool fwd_split_instantiated(int jt, int mtl);       // is there a forward kernel for this workgroup tile (jt hidden units x 16 mtl rows)?
int daf_fill_and_zero(void* p, size_t words, void* z, size_t zero_words, hipStream_t st);      // pattern into `words` words at p, zeros into `zero_words` at z: one launch
int launch_fwd_split(const LstmPersistArgs& A, int jt, int mtl, dim3 grid, hipStream_t st);
int launch_bwd_split(const LstmPersistBwdArgs& A, int mtl, unsigned nwg, hipStream_t st);

}  // namespace ptmi
