// fp32-equivalent GEMM on operands that are ALREADY split into fp16 (hi, lo) planes in MFMA-fragment order.
//
// csrc/gemm.hip splits fp32 operands in registers on their way into LDS; that arithmetic (and, for operands whose reduction
// axis is not contiguous, a 4 x 4 transpose in registers) is what bounds it, most of all in the weight-gradient form
// dW = dg^T x where both operands are of that kind (165-175 fp32-equivalent TFLOP/s alone, half of that next to a
// running recurrence).  Here the split happens ONCE per operand in a streaming pass (ptmi_pack_planes_t: read 4 B, write
// 4 B per element, any source orientation), and the GEMM is a plain 16-bit one:
//   operand X, R rows x K (reduction):  tiles [ceil(R / 16)][ceil(K / 32)][plane hi | lo][64 chunks of 16 B]
//   chunk (k group g = 0..3, row r = 0..15) at slot 16 g + r = the 8 fp16 values X[16 t + r][32 kb + 8 g .. + 7]
//   i.e. exactly the register image of one v_mfma_f32_16x16x32_f16 operand: a wavefront's LDS-DMA (global_load_lds, 16 B
//   per lane) of a 1 KB plane tile lands lane-linear in LDS and ds_read_b128 at lane * 16 is the fragment (no bank
//   conflicts, no VALU on the way); rows / k past the matrix are zero in the planes, so the loads need no bounds.
// C (+)= (A B^T) / (s_a s_b) with a b = hi hi + hi lo + lo hi in one fp32 accumulator, as in csrc/gemm.hip (same accuracy).
// Workgroup = 4 wavefronts, 128 x 128 tile (each 64 x 64 = 4 x 4 MFMA tiles), 32-wide k steps, two LDS stages of 32 KB
// (two workgroups per CU), ONE barrier per k step, the 8 LDS-DMA pieces of the next stage dealt out between the MFMA
// groups of the current one; split K through slabs summed in slab order (reproducible, no atomics, nobody waits for a
// sibling workgroup: safe next to the persistent recurrence kernels).  Prototype + measurements: scripts/mb/gemm_planes.hip.
//
// Round 3: gemm_planes_big_kernel - the same arithmetic as a PERSISTENT big-tile kernel for the shapes without split K (input
// projections, LSTM input gradients, linears): 8 wavefronts (2 x 4), wave tile (16 MT) x (16 NT), workgroup tile 256 x 320 /
// 256 x 256 / 128 x 320 / 256 x 192 / 128 x 256 picked per problem so that the tile count fills whole rounds of the CUs
// (N = 4800 = 15 x 320); grid = min(tiles, CUs), every workgroup walks its tiles (XCD-aware, band-major) in ONE flat (tile, k step)
// loop, so the LDS-DMA of the next tile's first stage is in flight while the finished tile is stored and the pipeline never
// drains; LDS-DMA through buffer descriptors (buffer_load_dwordx4 ... lds: one VGPR of lane offset, piece offsets in SGPRs).
// No workgroup waits for another.  Prototype, ablations and the zero-data (DVFS) comparison: scripts/mb/gemm_big.hip, DESIGN 3.9.
#include <algorithm>

#include "common.h"

namespace ptmi {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int PBM = 128, PBN = 128;
constexpr int FR = 64;                  // uint4 (16 B chunks) per plane tile

// s = 2^(13 - e) for max|v| = m 2^e, 1 <= m < 2 (as csrc/gemm.hip::operand_scale; NULL / zero / non-finite maximum: 1)
__device__ __forceinline__ float plane_scale(const unsigned* amax_bits) {
    if (!amax_bits) return 1.f;
    const unsigned e = (*amax_bits >> 23) & 0xffu;
    if (e == 0u || e == 0xffu) return 1.f;
    return __uint_as_float((unsigned)(127 + 13 + 127 - (int)e) << 23);
}

struct PlanesArgs {
    const uint4* A;             // planes of the M-side operand
    const uint4* B;             // planes of the N-side operand
    float* C;
    float* workspace;           // split K: [splits][M][N]
    const unsigned* amax_a;
    const unsigned* amax_b;
    const float* bias;          // [N] or null
    int M, N, KB;               // KB = k blocks of 32 in the planes
    long long ldc;
    int accumulate;
    int kb_per_split;
    int tiles_m, tiles_n;
    // two-part output: rows m >= m_split go to C2 (row m - m_split, same row stride): both directions' dW_ih = [dgates_f | dgates_r]^T x
    // as ONE launch into the two parameters' gradient buffers (m_split a multiple of 16; null: one output)
    float* C2 = nullptr;
    int m_split = 0;
    // fused epilogue of a dense layer with a ReLU behind it (pit/model.py:98-104): C = max(A B^T + bias, 0), and the float bits of max C
    // into *amax_out (zeroed by the host call, atomicMax: non-negative floats order like their bits) - the operand scale of the NEXT
    // GEMM, so that neither the activation nor the maximum is a pass of its own
    int relu = 0;
    unsigned* amax_out = nullptr;
};

// ONE atomicMax per workgroup: the largest of its lanes' non-negative values (inf / nan: the largest finite float, as ptmi_absmax).
// Atomics on one word are served one after the other (~12 ns each, ptmi_absmax): one per wavefront of a 2048-workgroup launch measured
// +90 us per launch.  `red`: one word per wavefront; every thread of the workgroup calls this, once.
__device__ __forceinline__ void block_amax(unsigned* out, unsigned m, unsigned* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < (blockDim.x >> 6); ++w) m = max(m, red[w]);
        if (m != 0u) atomicMax(out, m >= 0x7f800000u ? 0x7f7fffffu : m);
    }
}

// BF16: the planes hold bf16 halves (fp32's exponent range: no operand scale) - the backward recurrence's hand-off copy of the
// gate gradients, whose range is not known before they are computed, and weights packed to match (csrc/lstm_split.hip)
// ONE: only the hi planes are multiplied (one product per element: plain 16-bit operands - the reduced-precision "bf16 mode")
template <bool BF16, bool ONE, bool RELU = false>
__global__ __launch_bounds__(256, 2) void gemm_planes_kernel(const PlanesArgs G) {
#if __HIP_DEVICE_COMPILE__          // (the host pass cannot parse the LDS-DMA builtin; it only needs the stub)
    constexpr int PIECES = 32;      // plane tiles per stage: (8 row tiles + 8 column tiles) x 2 planes
    __shared__ uint4 lds[2 * PIECES * FR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware tile order: workgroup id L runs on XCD L % 8; every XCD gets one contiguous range of tiles (row-major over
    // [tiles_m][tiles_n]), so the workgroups an XCD runs at a time share operand panels through its L2
    const int T = G.tiles_m * G.tiles_n;
    const int q = T / 8, r8 = T % 8, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    if (idx >= (xcd < r8 ? q + 1 : q)) return;
    const int tile = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + idx;
    const int tm = tile / G.tiles_n, tn = tile - tm * G.tiles_n;
    const int kb0 = blockIdx.z * G.kb_per_split, kb1 = min(G.KB, kb0 + G.kb_per_split);
    const int wm = wave >> 1, wn = wave & 1;
    const float inv = 1.f / (plane_scale(G.amax_a) * plane_scale(G.amax_b));      // two dependent loads: long before their use
    const int rta = (G.M + 15) / 16, rtb = (G.N + 15) / 16;
    const uint4* gsrc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = wave * 8 + i;                        // piece: 16 A pieces (row tile, plane), then 16 B pieces
        const bool isa = f < 16;
        const int rt = (f & 15) >> 1, p = f & 1;
        const long long row_tile = min((long long)(isa ? tm : tn) * 8 + rt, (long long)(isa ? rta : rtb) - 1);
        gsrc[i] = (isa ? G.A : G.B) + ((row_tile * G.KB + kb0) * 2 + p) * FR + lane;
    }
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    if (kb0 < kb1) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (!ONE || !(i & 1)) __builtin_amdgcn_global_load_lds(gsrc[i], &lds[(wave * 8 + i) * FR], 16, 0, 0);
    }
    for (int kb = kb0; kb < kb1; ++kb) {
        const int st = (kb - kb0) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wavefront's pieces of stage `st` have landed
        __builtin_amdgcn_s_barrier();                             // everybody's have; everybody is done reading stage st ^ 1
        const uint4* sa = &lds[(st * PIECES + wm * 8) * FR + lane];
        const uint4* sb = &lds[(st * PIECES + 16 + wn * 8) * FR + lane];
        const bool more = kb + 1 < kb1;
        h8 bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bh[j] = __builtin_bit_cast(h8, sb[(j * 2 + 0) * FR]);
            bl[j] = ONE ? bh[j] : __builtin_bit_cast(h8, sb[(j * 2 + 1) * FR]);
        }
        h8 ah = __builtin_bit_cast(h8, sa[0]), al = ONE ? ah : __builtin_bit_cast(h8, sa[FR]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h8 nh = ah, nl = al;
            if (i + 1 < 4) {
                nh = __builtin_bit_cast(h8, sa[((i + 1) * 2 + 0) * FR]);
                nl = ONE ? nh : __builtin_bit_cast(h8, sa[((i + 1) * 2 + 1) * FR]);
            }
            if (more) {         // two pieces of the next stage per MFMA group
#pragma unroll
                for (int pc = 2 * i; pc < 2 * i + 2; ++pc)
                    if (!ONE || !(pc & 1))
                        __builtin_amdgcn_global_load_lds(gsrc[pc] + (long long)(kb + 1 - kb0) * 2 * FR,
                                                         &lds[((st ^ 1) * PIECES + wave * 8 + pc) * FR], 16, 0, 0);
            }
            // D[n = 4 (lane >> 4) + e][m = lane & 15]: the MFMA's "a" operand is the B fragment, so a lane holds four
            // consecutive columns of C; product kind outermost: 4 independent MFMAs between two on one accumulator
            // (p = 2: hi hi, 1: hi lo, 0: lo hi; ONE: p = 2 only)
#pragma unroll
            for (int p = ONE ? 2 : 0; p < 3; ++p)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = BF16 ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, p == 0 ? bl[j] : bh[j]),
                                                                               __builtin_bit_cast(b8, p == 1 ? al : ah), acc[i][j], 0, 0, 0)
                                     : __builtin_amdgcn_mfma_f32_16x16x32_f16(p == 0 ? bl[j] : bh[j], p == 1 ? al : ah, acc[i][j], 0, 0, 0);
            ah = nh;
            al = nl;
        }
    }
    const bool slab = gridDim.z > 1;
    float* const Cz = slab ? G.workspace + (long long)blockIdx.z * G.M * G.N : G.C;
    const long long ldc = slab ? G.N : G.ldc;
    const bool vec = (ldc & 3) == 0 && ((reinterpret_cast<unsigned long long>(Cz) | reinterpret_cast<unsigned long long>(G.C2)) & 15) == 0;
    const bool add = G.accumulate && !slab;
    const int r = lane & 15, g = lane >> 4;
    // this lane's four bias groups (one per column tile j), all requested before any is used
    f4 bv[4];
    {
        const bool bias_on = G.bias != nullptr && !slab;
        const bool bvec = (reinterpret_cast<unsigned long long>(G.bias) & 15) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = tn * PBN + wn * 64 + j * 16 + g * 4;
            bv[j] = f4{0.f, 0.f, 0.f, 0.f};
            if (bias_on && bvec && n + 3 < G.N) {
                bv[j] = *reinterpret_cast<const f4*>(G.bias + n);
            } else if (bias_on) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[j][e] = G.bias[min(n + e, G.N - 1)];
            }
        }
    }
    const bool fuse = RELU && !slab;          // (RELU: an instantiation of its own - the plain kernels compile as they always did)
    unsigned mx = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = tm * PBM + wm * 64 + i * 16 + r;
        if (m >= G.M) continue;
        const bool second = !slab && G.C2 != nullptr && m >= G.m_split;
        float* const rowp = second ? G.C2 + (long long)(m - G.m_split) * ldc : Cz + (long long)m * ldc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = tn * PBN + wn * 64 + j * 16 + g * 4;
            float* o = rowp + n;
            f4 v = acc[i][j] * inv + bv[j];
            if (RELU && fuse) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = v[e] < 0.f ? 0.f : v[e];           // (not fmaxf: a NaN stays a NaN, like torch.relu - ADVICE r4)
                    if (n + e < G.N) mx = max(mx, __float_as_uint(v[e]));
                }
            }
            if (vec && n + 3 < G.N) {
                f4* o4 = reinterpret_cast<f4*>(o);
                *o4 = add ? *o4 + v : v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < G.N) o[e] = add ? o[e] + v[e] : v[e];
            }
        }
    }
    if constexpr (RELU) {
        if (!slab && G.amax_out) {          // (workgroup-uniform)
            __shared__ unsigned red[4];
            block_amax(G.amax_out, mx, red);
        }
    }
#endif
}

struct BigArgs {
    const uint4* A;             // planes of the M-side operand
    const uint4* B;             // planes of the N-side operand
    float* C;
    const unsigned* amax_a;
    const unsigned* amax_b;
    const float* bias;          // [N] or null
    int M, N, KB;               // KB = k blocks of 32 in the planes
    long long ldc;
    int accumulate;
    int tiles_m, tiles_n, band;
    unsigned a_bytes, b_bytes;  // extent of the planes (buffer descriptors; < 2 GB: launch_big)
    // split K (weight-gradient shapes: few output tiles, K = all rows of the batch): work item = (k range, tile), range-major, so
    // that the items an XCD runs at a time share their operand panels' k range; item (z, tile) leaves its partial product in slab z of
    // `slabs` [splits][M][N], summed in slab order by planes_reduce_kernel (reproducible, no atomics, nobody waits for anybody)
    int splits = 1, kb_per_split = 0;
    float* slabs = nullptr;
    float* C2 = nullptr;        // two-part output, as in PlanesArgs
    int m_split = 0;
    int relu = 0;               // as in PlanesArgs (not with split K: planes_reduce_kernel applies it then)
    unsigned* amax_out = nullptr;
};

// Grouped call (ptmi_gemm_planes_bf16_group): operand A in two parts (rows below / from m_split), up to three B segments with planes and
// column counts of their own (one K), and a product per (part, segment) BLOCK that is not skipped - a BLSTM layer's four weight gradients
// {dG_f, dG_b} x {X, H_f, H_b} without (f, H_b) and (b, H_f).  Work item = (k range, block, tile), range-major over the tiles of all
// blocks; every item leaves its partial product in its block's slabs [splits][rows][cols] (at slab_off + z * slab_stride), summed in
// slab order by ONE planes_reduce_kernel(ReduceGroupArgs) launch.  BigArgs' A / a_bytes / KB / splits / kb_per_split / slabs / band hold.
constexpr int GROUP_SEGS = 3, GROUP_BLOCKS = 6;
struct GroupTable {
    const uint4* B[GROUP_SEGS];             // per segment: planes, their extent in bytes, 16-row tiles
    unsigned b_bytes[GROUP_SEGS];
    int rtb[GROUP_SEGS];
    int part_rt0[2], part_rts[2];           // per part of A: first 16-row tile, number of them
    int tile_start[GROUP_BLOCKS + 1];       // per block (the skipped ones left out): first tile; past the last block: INT_MAX,
    int total_tiles;                        //   and the tiles of all blocks
    int tiles_m[GROUP_BLOCKS], tiles_n[GROUP_BLOCKS], part[GROUP_BLOCKS], seg[GROUP_BLOCKS], rows[GROUP_BLOCKS], cols[GROUP_BLOCKS];
    long long slab_off[GROUP_BLOCKS], slab_stride[GROUP_BLOCKS];          // floats, multiples of 4
};
struct GroupBigArgs : BigArgs {
    GroupTable T;
};

// (ARGS = GroupBigArgs: the grouped call's instantiations - bf16 planes, slabs only)
template <bool BF16, int MT, int NT, bool ONE, bool RELU = false, class ARGS = BigArgs>
__global__ __launch_bounds__(512, 2) void gemm_planes_big_kernel(const ARGS G) {
#if __HIP_DEVICE_COMPILE__
    constexpr bool GROUP = __is_same(ARGS, GroupBigArgs);
    constexpr int WM = 2, WN = 4, RA = WM * MT, RB = WN * NT, PIECES = 2 * (RA + RB);
    constexpr int PA = 2 * RA / 8, PB = 2 * RB / 8, PW = PA + PB;          // 1 KB plane tiles every wavefront copies per k step
    static_assert((2 * RA) % 8 == 0 && (2 * RB) % 8 == 0, "pieces per wave");
    __shared__ uint4 lds[2 * PIECES * FR];      // two stages of [A pieces (row tile, plane) | B pieces]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(G.A), 0, G.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(G.B), 0, G.b_bytes, 0x00020000);
    const int voff = lane * 16;
    const int KB = G.KB;
    const int rta = (G.M + 15) / 16, rtb = (G.N + 15) / 16;
    const float inv = GROUP ? 1.f : 1.f / (plane_scale(G.amax_a) * plane_scale(G.amax_b));

    // this workgroup's work items: workgroup id b runs on XCD b % 8; every XCD owns one contiguous range of the item list - k range
    // by k range the band-major tile list (bands of G.band tile rows, column by column) -, of which its j-th workgroup takes every
    // (grid / 8)-th
    int TT = G.tiles_m * G.tiles_n;
    if constexpr (GROUP) TT = G.T.total_tiles;
    const int T = TT * G.splits;
    const int xcd = blockIdx.x & 7, j0 = blockIdx.x >> 3, per = gridDim.x >> 3;
    const int q = T / 8, r8 = T % 8;
    const int cnt = xcd < r8 ? q + 1 : q;
    const int first = xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q;
    if (j0 >= cnt) return;
    const int band_tiles = G.band * G.tiles_n;
    auto tile_rc = [&](int item, int& tm, int& tn, int& z) {
        z = item / TT;
        const int idx = item - z * TT;
        const int b = idx / band_tiles, rem = idx - b * band_tiles;
        const int h = min(G.band, G.tiles_m - b * G.band);
        tn = rem / h;
        tm = b * G.band + (rem - tn * h);
    };
    // grouped call: what an item's loads and stores need of its block (workgroup-uniform: scalar registers, looked up once per item)
    struct Blk {
        int a_rt0, a_rts, b_rts;            // A: first 16-row tile of the part and how many; B: 16-row tiles of the segment
        __amdgpu_buffer_rsrc_t rb;
        int rows, cols;
        long long slab;                     // slab 0 of the block
        long long slab_stride;
    };
    auto tile_rc_group = [&](int item, int& tm, int& tn, int& z, Blk& k) {
        if constexpr (GROUP) {
            z = item / TT;
            int idx = item - z * TT, blk = 0;
#pragma unroll
            for (int b = 1; b < GROUP_BLOCKS; ++b) blk += idx >= G.T.tile_start[b] ? 1 : 0;
            idx -= G.T.tile_start[blk];
            const int tiles_m = G.T.tiles_m[blk], tiles_n = G.T.tiles_n[blk];
            const int bt = G.band * tiles_n;
            const int b = idx / bt, rem = idx - b * bt;
            const int h = min(G.band, tiles_m - b * G.band);
            tn = rem / h;
            tm = b * G.band + (rem - tn * h);
            const int p = G.T.part[blk], s = G.T.seg[blk];
            k.a_rt0 = G.T.part_rt0[p];
            k.a_rts = G.T.part_rts[p];
            k.b_rts = G.T.rtb[s];
            k.rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(G.T.B[s]), 0, G.T.b_bytes[s], 0x00020000);
            k.rows = G.T.rows[blk];
            k.cols = G.T.cols[blk];
            k.slab = G.T.slab_off[blk];
            k.slab_stride = G.T.slab_stride[blk];
        }
    };
    const int KBS = (GROUP || G.splits > 1) ? G.kb_per_split : KB;        // k blocks per work item (the last range may be shorter)
    auto issue = [&](int i, int tm, int tn, int kb, int st) {            // piece i of this wavefront for (tile, k step) into stage st
        if (i < PA) {
            const int f = wave * PA + i;
            const int rt = min(tm * RA + (f >> 1), rta - 1);
            if (!ONE || !(f & 1))           // (ONE: the lo planes stay where they are)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, &lds[(st * PIECES + f) * FR], 16, voff, ((rt * KB + kb) * 2 + (f & 1)) * 1024, 0, 0);
        } else {
            const int f = wave * PB + (i - PA);
            const int rt = min(tn * RB + (f >> 1), rtb - 1);
            if (!ONE || !(f & 1))
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, &lds[(st * PIECES + 2 * RA + f) * FR], 16, voff, ((rt * KB + kb) * 2 + (f & 1)) * 1024, 0, 0);
        }
    };
    // the same for an item of a grouped call: row tiles counted within the part / segment (a tile never reaches into the next part)
    auto issue_group = [&](int i, int tm, int tn, int kb, int st, int a_rt0, int a_rts, int b_rts, __amdgpu_buffer_rsrc_t rbk) {
        if (i < PA) {
            const int f = wave * PA + i;
            const int rt = a_rt0 + min(tm * RA + (f >> 1), a_rts - 1);
            if (!ONE || !(f & 1))
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, &lds[(st * PIECES + f) * FR], 16, voff, ((rt * KB + kb) * 2 + (f & 1)) * 1024, 0, 0);
        } else {
            const int f = wave * PB + (i - PA);
            const int rt = min(tn * RB + (f >> 1), b_rts - 1);
            if (!ONE || !(f & 1))
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rbk, &lds[(st * PIECES + 2 * RA + f) * FR], 16, voff, ((rt * KB + kb) * 2 + (f & 1)) * 1024, 0, 0);
        }
    };

    f4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    int idx = j0, tm, tn, tz;
    Blk bk{}, nbk{};
    if constexpr (GROUP) {
        tile_rc_group(first + idx, tm, tn, tz, bk);
#pragma unroll
        for (int i = 0; i < PW; ++i) issue_group(i, tm, tn, tz * KBS, 0, bk.a_rt0, bk.a_rts, bk.b_rts, bk.rb);
    } else {
        tile_rc(first + idx, tm, tn, tz);
#pragma unroll
        for (int i = 0; i < PW; ++i) issue(i, tm, tn, tz * KBS, 0);
    }
    int st = 0;
    constexpr int PPI = (PW + MT - 1) / MT;             // pieces issued per row-tile iteration
    unsigned relu_max = 0u;                             // (G.relu: the largest output of all this workgroup's tiles, one atomic at the end)
    while (true) {
        const int nidx = idx + per;
        const bool has_next_tile = nidx < cnt;
        int ntm = tm, ntn = tn, ntz = tz;
        if constexpr (GROUP) {
            nbk = bk;
            if (has_next_tile) tile_rc_group(first + nidx, ntm, ntn, ntz, nbk);
        } else {
            if (has_next_tile) tile_rc(first + nidx, ntm, ntn, ntz);
        }
        const int kb_lo = tz * KBS, kb_hi = min(KB, kb_lo + KBS);
        for (int kb = kb_lo; kb < kb_hi; ++kb) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wavefront's pieces of stage `st` have landed
            __builtin_amdgcn_s_barrier();                             // everybody's have; everybody is done reading stage st ^ 1
            // the stage requested during this step: the next k step of this tile, or the first one of the next tile (behind the
            // very last step: this tile's first stage once more - never read, keeps the loop free of branches)
            const bool last = kb + 1 == kb_hi;
            const int ptm = last ? ntm : tm, ptn = last ? ntn : tn, pkb = last ? ntz * KBS : kb + 1;
            const int pa0 = last ? nbk.a_rt0 : bk.a_rt0, pas = last ? nbk.a_rts : bk.a_rts, pbs = last ? nbk.b_rts : bk.b_rts;
            const __amdgpu_buffer_rsrc_t prb = last ? nbk.rb : bk.rb;
            const uint4* sa = &lds[(st * PIECES + wm * MT * 2) * FR + lane];
            const uint4* sb = &lds[(st * PIECES + 2 * RA + wn * NT * 2) * FR + lane];
            h8 bh[NT], bl[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bh[j] = __builtin_bit_cast(h8, sb[(j * 2 + 0) * FR]);
                bl[j] = ONE ? bh[j] : __builtin_bit_cast(h8, sb[(j * 2 + 1) * FR]);
            }
            h8 ah = __builtin_bit_cast(h8, sa[0]), al = ONE ? ah : __builtin_bit_cast(h8, sa[FR]);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                h8 nh = ah, nl = al;
                if (i + 1 < MT) {
                    nh = __builtin_bit_cast(h8, sa[((i + 1) * 2 + 0) * FR]);
                    nl = ONE ? nh : __builtin_bit_cast(h8, sa[((i + 1) * 2 + 1) * FR]);
                }
#pragma unroll
                for (int pc = i * PPI; pc < (i + 1) * PPI; ++pc) {
                    if constexpr (GROUP) {
                        if (pc < PW) issue_group(pc, ptm, ptn, pkb, st ^ 1, pa0, pas, pbs, prb);
                    } else {
                        if (pc < PW) issue(pc, ptm, ptn, pkb, st ^ 1);
                    }
                }
                // D[n = 4 (lane >> 4) + e][m = lane & 15]: the MFMA's "a" operand is the B fragment, so a lane holds four consecutive
                // columns of C; product kind outermost: NT independent MFMAs between two on one accumulator
#pragma unroll
                for (int p = ONE ? 2 : 0; p < 3; ++p)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[i][j] = BF16 ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, p == 0 ? bl[j] : bh[j]),
                                                                                   __builtin_bit_cast(b8, p == 1 ? al : ah), acc[i][j], 0, 0, 0)
                                         : __builtin_amdgcn_mfma_f32_16x16x32_f16(p == 0 ? bl[j] : bh[j], p == 1 ? al : ah, acc[i][j], 0, 0, 0);
                ah = nh;
                al = nl;
            }
            st ^= 1;
        }
        // epilogue of tile (tm, tn); the next tile's first stage is in flight meanwhile
        {
            const int r = lane & 15, g = lane >> 4;
            const int n0 = (tn * WN + wn) * NT * 16 + g * 4;
            const bool vec = (G.ldc & 3) == 0 && ((reinterpret_cast<unsigned long long>(G.C) | reinterpret_cast<unsigned long long>(G.C2)) & 15) == 0;
            const bool full = vec && (tn * WN + wn + 1) * NT * 16 <= G.N;           // wave-uniform: every column of this wave's tile exists
            f4 bv[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bv[j] = f4{0.f, 0.f, 0.f, 0.f};
                if (G.bias) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) bv[j][e] = G.bias[min(n0 + j * 16 + e, G.N - 1)];
                }
            }
            const int mrow = (tm * WM + wm) * MT * 16 + r;
            if (GROUP || G.splits > 1) {         // the partial product of this k range: slab tz, row stride N (planes_reduce_kernel adds bias / C)
                // (grouped call: slab tz of the item's block, that block's rows and columns)
                const int sM = GROUP ? bk.rows : G.M, sN = GROUP ? bk.cols : G.N;
                float* const srow = GROUP ? G.slabs + bk.slab + tz * bk.slab_stride + (long long)mrow * sN + n0
                                          : G.slabs + ((long long)tz * G.M + mrow) * G.N + n0;
                const bool svec = (sN & 3) == 0 && (reinterpret_cast<unsigned long long>(G.slabs) & 15) == 0;
                const bool sfull = svec && (tn * WN + wn + 1) * NT * 16 <= sN;
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const bool ok = mrow + i * 16 < sM;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const f4 v = acc[i][j] * inv;
                        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
                        float* o = srow + (long long)i * 16 * sN + j * 16;
                        if (sfull) {
                            if (ok) *reinterpret_cast<f4*>(o) = v;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (ok && n0 + j * 16 + e < sN) o[e] = v[e];
                        }
                    }
                }
                if (!has_next_tile) break;
                idx = nidx;
                tm = ntm;
                tn = ntn;
                tz = ntz;
                if constexpr (GROUP) bk = nbk;
                continue;
            }
            // row of subtile i (two-part output: rows from m_split on live in C2)
            auto rowp = [&](int i) {
                const int m = mrow + i * 16;
                return (G.C2 != nullptr && m >= G.m_split ? G.C2 + (long long)(m - G.m_split) * G.ldc : G.C + (long long)m * G.ldc) + n0;
            };
            if (RELU) {             // dense layer + ReLU (no accumulation): the activation and the next operand's scale, here
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const bool ok = mrow + i * 16 < G.M;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        f4 v = acc[i][j] * inv + bv[j];
                        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = v[e] < 0.f ? 0.f : v[e];           // (a NaN stays a NaN, like torch.relu)
                            if (ok && n0 + j * 16 + e < G.N) relu_max = max(relu_max, __float_as_uint(v[e]));
                        }
                        float* o = rowp(i) + j * 16;
                        if (full) {
                            if (ok) *reinterpret_cast<f4*>(o) = v;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (ok && n0 + j * 16 + e < G.N) o[e] = v[e];
                        }
                    }
                }
            } else if (full && !G.accumulate) {
#pragma unroll
                for (int i = 0; i < MT; ++i) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const f4 v = acc[i][j] * inv + bv[j];
                        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
                        if (mrow + i * 16 < G.M) *reinterpret_cast<f4*>(rowp(i) + j * 16) = v;
                    }
                }
            } else if (full) {
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const bool ok = mrow + i * 16 < G.M;
                    f4 old[NT];                         // all of a row tile's loads in flight before the first add
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        old[j] = ok ? *reinterpret_cast<const f4*>(rowp(i) + j * 16) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const f4 v = acc[i][j] * inv + bv[j] + old[j];
                        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
                        if (ok) *reinterpret_cast<f4*>(rowp(i) + j * 16) = v;
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const bool ok = mrow + i * 16 < G.M;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const f4 v = acc[i][j] * inv + bv[j];
                        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
                        float* o = rowp(i) + j * 16;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (ok && n0 + j * 16 + e < G.N) o[e] = G.accumulate ? o[e] + v[e] : v[e];
                    }
                }
            }
        }
        if (!has_next_tile) break;          // (the stage requested during the last step is never read; the wait below retires it)
        idx = nidx;
        tm = ntm;
        tn = ntn;
        tz = ntz;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (RELU) {
        if (G.amax_out && G.splits == 1) {
            __shared__ unsigned red[8];
            block_amax(G.amax_out, relu_max, red);
        }
    }
#endif
}

// max |x| as float bits (non-negative floats order like unsigned integers): one atomicMax per workgroup
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long long rows, long long cols, long long ld,
                                                     unsigned* __restrict__ out) {
    __shared__ unsigned red[4];
    const long long n = rows * cols;
    unsigned m = 0u;
    if (ld == cols && (cols & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        // four independent 16-byte loads per lane and iteration (few workgroups - see ptmi_absmax - so each has to keep
        // enough bytes in flight itself)
        const long long n4 = n >> 2, stride = (long long)gridDim.x * 256;
        const f4* x4 = reinterpret_cast<const f4*>(x);
        long long i = blockIdx.x * 256ll + threadIdx.x;
        for (; i + 3 * stride < n4; i += 4 * stride) {
            const f4 v0 = x4[i], v1 = x4[i + stride], v2 = x4[i + 2 * stride], v3 = x4[i + 3 * stride];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                m = max(max(m, __float_as_uint(v0[q]) & 0x7fffffffu),
                        max(max(__float_as_uint(v1[q]) & 0x7fffffffu, __float_as_uint(v2[q]) & 0x7fffffffu), __float_as_uint(v3[q]) & 0x7fffffffu));
        }
        for (; i < n4; i += stride) {
            const f4 v = x4[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) m = max(m, __float_as_uint(v[q]) & 0x7fffffffu);
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
            const long long r = i / cols, c = i - r * cols;
            m = max(m, __float_as_uint(x[r * ld + c]) & 0x7fffffffu);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        if (m >= 0x7f800000u) m = 0x7f7fffffu;          // inf / nan: the GEMM result will be non-finite anyway
        atomicMax(out, m);
    }
}

// 8 values -> their 16-bit (hi, lo) halves as one 16-byte chunk per plane (round to nearest; v - hi is exact in fp32)
template <bool BF16>
__device__ __forceinline__ void split_chunk(const float (&v)[8], uint4* hi_out, uint4* lo_out) {
    if (BF16) {
        b8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (__bf16)v[e];
            lo[e] = (__bf16)(v[e] - (float)hi[e]);
        }
        *hi_out = __builtin_bit_cast(uint4, hi);
        *lo_out = __builtin_bit_cast(uint4, lo);
    } else {
        h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (_Float16)v[e];
            lo[e] = (_Float16)(v[e] - (float)hi[e]);
        }
        *hi_out = __builtin_bit_cast(uint4, hi);
        *lo_out = __builtin_bit_cast(uint4, lo);
    }
}

// split K, second pass: C (+)= sum over the slabs in slab order (fixed order: bitwise reproducible)
__global__ __launch_bounds__(256) void planes_reduce_kernel(const float* __restrict__ ws, int splits, float* __restrict__ C, long long ldc,
                                                            const float* __restrict__ bias, int M, int N, int accumulate,
                                                            float* __restrict__ C2 = nullptr, int m_split = 0, int relu = 0,
                                                            unsigned* __restrict__ amax_out = nullptr) {
    const long long total = (long long)M * N;
    unsigned mx = 0u;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / N), c = (int)(i - (long long)r * N);
        float sum = 0.f;
        for (int z = 0; z < splits; ++z) sum += ws[(long long)z * total + i];
        if (bias) sum += bias[c];
        if (relu) {
            sum = sum < 0.f ? 0.f : sum;           // (a NaN stays a NaN, like torch.relu)
            mx = max(mx, __float_as_uint(sum));
        }
        float* o = (C2 != nullptr && r >= m_split) ? C2 + (long long)(r - m_split) * ldc + c : C + (long long)r * ldc + c;
        *o = accumulate ? *o + sum : sum;
    }
    if (relu && amax_out) {
        __shared__ unsigned red[4];
        block_amax(amax_out, mx, red);
    }
}

// The same pass behind a grouped call: every block's slabs summed in slab order into that block's output (row stride of its own:
// views into wider .grad buffers), ONE launch over the elements of all blocks
struct ReduceGroupArgs {
    const float* ws;
    int splits, nblocks, accumulate;
    long long start[GROUP_BLOCKS + 1];          // first UNIT of block b in the launch's flat index (past the last block: the total)
    long long slab_off[GROUP_BLOCKS], slab_stride[GROUP_BLOCKS];
    float* C[GROUP_BLOCKS];
    long long ldc[GROUP_BLOCKS];
    int cols[GROUP_BLOCKS];
    int vec[GROUP_BLOCKS];                      // unit = 4 consecutive elements of a row (cols, ldc multiples of 4, C 16-byte aligned), else 1
};

__global__ __launch_bounds__(256) void planes_reduce_kernel(const ReduceGroupArgs R) {
    const long long total = R.start[R.nblocks];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        int b = 0;
#pragma unroll
        for (int q = 1; q < GROUP_BLOCKS; ++q) b += (q < R.nblocks && i >= R.start[q]) ? 1 : 0;
        const int N = R.cols[b];
        const long long stride = R.slab_stride[b];
        if (R.vec[b]) {
            const long long j = (i - R.start[b]) * 4;
            const int r = (int)(j / N), c = (int)(j - (long long)r * N);
            const float* w = R.ws + R.slab_off[b] + j;
            f4 sum = {0.f, 0.f, 0.f, 0.f};
            for (int z = 0; z < R.splits; ++z) sum += *reinterpret_cast<const f4*>(w + (long long)z * stride);
            f4* o = reinterpret_cast<f4*>(R.C[b] + (long long)r * R.ldc[b] + c);
            *o = R.accumulate ? *o + sum : sum;
        } else {
            const long long j = i - R.start[b];
            const int r = (int)(j / N), c = (int)(j - (long long)r * N);
            const float* w = R.ws + R.slab_off[b] + j;
            float sum = 0.f;
            for (int z = 0; z < R.splits; ++z) sum += w[(long long)z * stride];
            float* o = R.C[b] + (long long)r * R.ldc[b] + c;
            *o = R.accumulate ? *o + sum : sum;
        }
    }
}

// dx of a ReLU and the operand scale of what multiplies it next, one pass: out = 0 where y <= 0 (y: the ReLU's OUTPUT), else g - torch's
// threshold_backward, which lets the gradient through where y is NaN; float bits
// of max |out| into *amax_out (zeroed by the host call)
__global__ __launch_bounds__(256) void relu_backward_absmax_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ out,
                                                                   long long rows, long long cols, long long ld_g, long long ld_y, long long ld_o,
                                                                   unsigned* __restrict__ amax_out) {
    unsigned mx = 0u;
    const long long n = rows * cols;
    if (ld_g == cols && ld_y == cols && ld_o == cols && (cols & 3) == 0 &&
        ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
        const long long n4 = n >> 2, stride = (long long)gridDim.x * 256;
        const f4* g4 = reinterpret_cast<const f4*>(g);
        const f4* y4 = reinterpret_cast<const f4*>(y);
        f4* o4 = reinterpret_cast<f4*>(out);
        long long i = blockIdx.x * 256ll + threadIdx.x;
        for (; i + stride < n4; i += 2 * stride) {          // two independent 16-byte pairs per lane and iteration
            const f4 ga = g4[i], ya = y4[i], gb = g4[i + stride], yb = y4[i + stride];
            f4 va, vb;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                va[q] = ya[q] <= 0.f ? 0.f : ga[q];
                vb[q] = yb[q] <= 0.f ? 0.f : gb[q];
                mx = max(mx, max(__float_as_uint(va[q]) & 0x7fffffffu, __float_as_uint(vb[q]) & 0x7fffffffu));
            }
            o4[i] = va;
            o4[i + stride] = vb;
        }
        for (; i < n4; i += stride) {
            const f4 ga = g4[i], ya = y4[i];
            f4 va;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                va[q] = ya[q] <= 0.f ? 0.f : ga[q];
                mx = max(mx, __float_as_uint(va[q]) & 0x7fffffffu);
            }
            o4[i] = va;
        }
    } else {
        for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
            const long long r = i / cols, c = i - r * cols;
            const float v = y[r * ld_y + c] <= 0.f ? 0.f : g[r * ld_g + c];
            out[r * ld_o + c] = v;
            mx = max(mx, __float_as_uint(v) & 0x7fffffffu);
        }
    }
    __shared__ unsigned red[4];
    block_amax(amax_out, mx, red);
}

// Source x[k][c] (row stride ld; the operand's ROWS are the columns c, its reduction axis the rows k) -> planes.
// Workgroup: 32 k x 64 c; loads coalesced along c, a transpose through LDS, one 16 B chunk per thread and plane.
template <bool BF16>
__global__ __launch_bounds__(256) void pack_planes_t_kernel(const float* __restrict__ x, long long krows, long long cols, long long ld,
                                                            const unsigned* __restrict__ amax, uint4* __restrict__ out, long long KBS,
                                                            long long KBO) {
    __shared__ float tile[32][65];
    const int tid = threadIdx.x;
    const long long kb = blockIdx.x, c0 = (long long)blockIdx.y * 64;
    const float s = plane_scale(amax);
    {
        const int cx = tid & 63, ky = tid >> 6;             // 64 columns x 4 rows per pass
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const long long k = kb * 32 + ky + p * 4, c = c0 + cx;
            tile[ky + p * 4][cx] = (k < krows && c < cols) ? x[k * ld + c] * s : 0.f;
        }
    }
    __syncthreads();
    // chunk of this thread: row tile rl = tid / 64 of the 4 in this block, k group g, row r
    const int rl = tid >> 6, g = (tid >> 4) & 3, r = tid & 15;
    const long long rt = blockIdx.y * 4 + rl;
    if (rt * 16 >= ((cols + 15) / 16) * 16) return;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[g * 8 + e][rl * 16 + r];
    uint4* o = out + ((rt * KBS + KBO + kb) * 2) * FR + g * 16 + r;
    split_chunk<BF16>(v, o, o + FR);
}

// The same pass for sources whose rows are 16-byte aligned (x and ld: every operand of the training step but the 257-column
// input): float4 loads (16 lanes per row, 16 rows per pass), column blocks fastest in the grid so that workgroups running together
// read whole rows.  scripts/mb/pack_t.hip: 32192 x 2400 of 4800 columns 153 -> 117 us, 32192 x 1200 82 -> 52 us (a copy of the same
// bytes: 121 / 52 us); wider tiles or strips with the next tile's loads in flight are no faster.
template <bool BF16>
__device__ __forceinline__ void pack_planes_t4_block(const float* __restrict__ x, long long krows, long long cols, long long ld, float s,
                                                     uint4* __restrict__ out, long long KBS, long long KBO, long long kb, long long cblock,
                                                     bool aligned) {
    constexpr int P = 68;                                   // row pitch: float4 stores stay aligned
    __shared__ float tile[32 * P];
    const int tid = threadIdx.x;
    const long long c0 = cblock * 64;
    const int lx = tid & 15, ly = tid >> 4;
    f4 regs[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const long long k = kb * 32 + ly + p * 16, c = c0 + lx * 4;
        f4 z = {0.f, 0.f, 0.f, 0.f};
        if (k < krows) {
            if (aligned && c + 4 <= cols) {
                z = *reinterpret_cast<const f4*>(x + k * ld + c);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < cols) z[e] = x[k * ld + c + e];
            }
        }
        regs[p] = z;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) *reinterpret_cast<f4*>(&tile[(ly + p * 16) * P + lx * 4]) = regs[p] * s;
    __syncthreads();
    const int rl = tid >> 6, g = (tid >> 4) & 3, r = tid & 15;
    const long long rt = cblock * 4 + rl;
    if (rt * 16 >= ((cols + 15) / 16) * 16) return;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = tile[(g * 8 + e) * P + rl * 16 + r];
    uint4* o = out + ((rt * KBS + KBO + kb) * 2) * FR + g * 16 + r;
    split_chunk<BF16>(v, o, o + FR);
}

template <bool BF16>
__global__ __launch_bounds__(256) void pack_planes_t4_kernel(const float* __restrict__ x, long long krows, long long cols, long long ld,
                                                             const unsigned* __restrict__ amax, uint4* __restrict__ out, long long KBS,
                                                             long long KBO) {
    pack_planes_t4_block<BF16>(x, krows, cols, ld, plane_scale(amax), out, KBS, KBO, blockIdx.y, blockIdx.x, true);
}

// Up to three sources with one k extent in ONE launch (a BLSTM layer's x, h_prev forward, h_prev reverse: the B segments of
// ptmi_gemm_planes_bf16_group), every source into planes of its own: the column blocks of the sources lie behind each other in
// grid.x.  A source whose rows are not 16-byte aligned (the 257-column input) is read with scalar loads - the same values, so
// either way the planes are those of a launch of its own.
constexpr int PACK_SRCS = 3;
struct PackListArgs {
    const float* x[PACK_SRCS];
    uint4* out[PACK_SRCS];
    long long cols[PACK_SRCS], ld[PACK_SRCS];
    int cb_start[PACK_SRCS + 1];            // first column block of source i in grid.x (unused sources: the total)
    int aligned[PACK_SRCS];
    long long krows, KB;
};

template <bool BF16>
__global__ __launch_bounds__(256) void pack_planes_t4_kernel(const PackListArgs L) {
    const int cb = blockIdx.x;
    const int i = (cb >= L.cb_start[1] ? 1 : 0) + (cb >= L.cb_start[2] ? 1 : 0);
    pack_planes_t4_block<BF16>(L.x[i], L.krows, L.cols[i], L.ld[i], 1.f, L.out[i], L.KB, 0, blockIdx.y, cb - L.cb_start[i], L.aligned[i] != 0);
}

// Source x[r][k] (row stride ld, the reduction axis k contiguous) -> planes of the operand with rows r.  Workgroup: one
// 16-row tile x 4 k blocks; a thread makes one chunk (8 consecutive k of one row: 32 B read, 2 x 16 B written).
template <bool BF16>
__global__ __launch_bounds__(256) void pack_planes_n_kernel(const float* __restrict__ x, long long rows, long long K, long long ld,
                                                            const unsigned* __restrict__ amax, uint4* __restrict__ out, long long KB,
                                                            long long KBS, long long KBO) {
    const int tid = threadIdx.x;
    const int r = tid >> 4, c = tid & 15;
    const long long rt = blockIdx.y, kb = (long long)blockIdx.x * 4 + (c >> 2);
    const int g = c & 3;
    if (kb >= KB) return;
    const float s = plane_scale(amax);
    const long long row = rt * 16 + r, k0 = kb * 32 + g * 8;
    float v[8];
    const float* src = x + row * ld + k0;
    if (row < rows && k0 + 8 <= K && ((reinterpret_cast<unsigned long long>(src) & 15) == 0)) {
        const f4 a = *reinterpret_cast<const f4*>(src), b = *reinterpret_cast<const f4*>(src + 4);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
        v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (row < rows && k0 + e < K) ? src[e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= s;
    uint4* o = out + ((rt * KBS + KBO + kb) * 2) * FR + g * 16 + r;
    split_chunk<BF16>(v, o, o + FR);
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int ptmi_absmax(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* out_bits, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !out_bits || rows < 0 || cols < 0 || ld < cols, PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = zero_words_async(out_bits, 1, st);
    if (e != hipSuccess) return (int)e;
    if (rows * cols == 0) return PTMI_OK;
    // every workgroup ends with one atomicMax on the same word: ~12 ns each at the L2 (2048 workgroups spent 25 us there,
    // whatever the size of the matrix), so at most 512 of them
    const long long work = (rows * cols + 4095) / 4096;
    const unsigned grid = (unsigned)std::min<long long>(std::max<long long>(work, 1), 512);
    hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, st, x, (long long)rows, (long long)cols, (long long)ld, out_bits);
    return launch_status();
}

int ptmi_absmax_accumulate(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* inout_bits, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !inout_bits || rows < 0 || cols < 0 || ld < cols, PTMI_E_INVALID);
    if (rows * cols == 0) return PTMI_OK;
    const long long work = (rows * cols + 4095) / 4096;
    const unsigned grid = (unsigned)std::min<long long>(std::max<long long>(work, 1), 512);
    hipLaunchKernelGGL(absmax_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), x, (long long)rows, (long long)cols, (long long)ld,
                       inout_bits);
    return launch_status();
}

int64_t ptmi_planes_elems(int64_t rows, int64_t k) {
    return ((rows + 15) / 16) * ((k + 31) / 32) * 2 * 512;          // fp16 values
}

// kbs / kbo / kbn: the operand's k blocks per row tile, the first k block this pass writes and how many (>= the source's own
// ceil(k / 32); the surplus is zero): 0 / 0 / 0 = an operand of its own
static int pack_t_impl(bool bf16, const float* x, int64_t k_rows, int64_t cols, int64_t ld, const uint32_t* amax, uint16_t* out,
                       ptmi_stream_t stream, int64_t kbs = 0, int64_t kbo = 0, int64_t kbn = 0) {
    PTMI_RETURN_IF(!x || !out || k_rows < 1 || cols < 1 || ld < cols, PTMI_E_INVALID);
    PTMI_RETURN_IF((reinterpret_cast<uintptr_t>(out) & 15) != 0, PTMI_E_INVALID);
    const long long own = (k_rows + 31) / 32, KB = kbn ? kbn : own, KBS = kbs ? kbs : KB, cb = (cols + 63) / 64;
    PTMI_RETURN_IF(KB < own || kbo < 0 || kbo + KB > KBS, PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ld % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && KB <= 65535) {
        const dim3 grid4((unsigned)cb, (unsigned)KB);
        if (bf16)
            hipLaunchKernelGGL(pack_planes_t4_kernel<true>, grid4, dim3(256), 0, st, x, (long long)k_rows, (long long)cols, (long long)ld, amax,
                               reinterpret_cast<uint4*>(out), KBS, (long long)kbo);
        else
            hipLaunchKernelGGL(pack_planes_t4_kernel<false>, grid4, dim3(256), 0, st, x, (long long)k_rows, (long long)cols, (long long)ld, amax,
                               reinterpret_cast<uint4*>(out), KBS, (long long)kbo);
        return launch_status();
    }
    PTMI_RETURN_IF(cb > 65535, PTMI_E_UNSUPPORTED);
    const dim3 grid((unsigned)KB, (unsigned)cb);
    if (bf16)
        hipLaunchKernelGGL(pack_planes_t_kernel<true>, grid, dim3(256), 0, st, x, (long long)k_rows, (long long)cols, (long long)ld, amax,
                           reinterpret_cast<uint4*>(out), KBS, (long long)kbo);
    else
        hipLaunchKernelGGL(pack_planes_t_kernel<false>, grid, dim3(256), 0, st, x, (long long)k_rows, (long long)cols, (long long)ld, amax,
                           reinterpret_cast<uint4*>(out), KBS, (long long)kbo);
    return launch_status();
}

static int pack_n_impl(bool bf16, const float* x, int64_t rows, int64_t k, int64_t ld, const uint32_t* amax, uint16_t* out,
                       ptmi_stream_t stream, int64_t kbs = 0, int64_t kbo = 0, int64_t kbn = 0) {
    PTMI_RETURN_IF(!x || !out || rows < 1 || k < 1 || ld < k, PTMI_E_INVALID);
    PTMI_RETURN_IF((reinterpret_cast<uintptr_t>(out) & 15) != 0, PTMI_E_INVALID);
    const long long own = (k + 31) / 32, KB = kbn ? kbn : own, KBS = kbs ? kbs : KB, rt = (rows + 15) / 16;
    PTMI_RETURN_IF(KB < own || kbo < 0 || kbo + KB > KBS, PTMI_E_INVALID);
    PTMI_RETURN_IF(rt > 65535, PTMI_E_UNSUPPORTED);
    const dim3 grid((unsigned)((KB + 3) / 4), (unsigned)rt);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bf16)
        hipLaunchKernelGGL(pack_planes_n_kernel<true>, grid, dim3(256), 0, st, x, (long long)rows, (long long)k, (long long)ld, amax,
                           reinterpret_cast<uint4*>(out), KB, KBS, (long long)kbo);
    else
        hipLaunchKernelGGL(pack_planes_n_kernel<false>, grid, dim3(256), 0, st, x, (long long)rows, (long long)k, (long long)ld, amax,
                           reinterpret_cast<uint4*>(out), KB, KBS, (long long)kbo);
    return launch_status();
}

int ptmi_pack_planes_t(const float* x, int64_t k_rows, int64_t cols, int64_t ld, const uint32_t* amax, uint16_t* out,
                       ptmi_stream_t stream) {
    return pack_t_impl(false, x, k_rows, cols, ld, amax, out, stream);
}

int ptmi_pack_planes_n(const float* x, int64_t rows, int64_t k, int64_t ld, const uint32_t* amax, uint16_t* out,
                       ptmi_stream_t stream) {
    return pack_n_impl(false, x, rows, k, ld, amax, out, stream);
}

int ptmi_pack_planes_t_bf16(const float* x, int64_t k_rows, int64_t cols, int64_t ld, uint16_t* out, ptmi_stream_t stream) {
    return pack_t_impl(true, x, k_rows, cols, ld, nullptr, out, stream);
}

int ptmi_pack_planes_n_bf16(const float* x, int64_t rows, int64_t k, int64_t ld, uint16_t* out, ptmi_stream_t stream) {
    return pack_n_impl(true, x, rows, k, ld, nullptr, out, stream);
}

int ptmi_pack_planes_into(const float* x, int64_t rows_or_k, int64_t cols, int64_t ld, int32_t transposed, int32_t bf16, const uint32_t* amax,
                          uint16_t* out, int64_t kb_total, int64_t kb_offset, int64_t kb_count, ptmi_stream_t stream) {
    PTMI_RETURN_IF(kb_total < 1 || kb_count < 1, PTMI_E_INVALID);
    return transposed ? pack_t_impl(bf16 != 0, x, rows_or_k, cols, ld, amax, out, stream, kb_total, kb_offset, kb_count)
                      : pack_n_impl(bf16 != 0, x, rows_or_k, cols, ld, amax, out, stream, kb_total, kb_offset, kb_count);
}

int64_t ptmi_gemm_planes_workspace_elems(int32_t m, int32_t n, int32_t k, int32_t split_k) {
    const int KB = (k + 31) / 32;
    if (split_k < 0) split_k = -split_k;
    const int splits = std::max(1, std::min<int>(split_k, KB));
    return splits > 1 ? (int64_t)splits * m * n : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- planner and launch path
#include <type_traits>
// PTMI_GEMM_TILE=0..5 pins the workgroup tile of every call (5 = the 128 x 128 kernel) for the sweeps of scripts/ and the tile tests; read at
// every call (the tests change it between calls), unset / -1: the cost model.  Not an entry point of the library.
static int tile_override() {
    const char* v = getenv("PTMI_GEMM_TILE");
    if (!v || !*v) return -1;
    const int t = atoi(v);
    return (t >= 0 && t <= 5) ? t : -1;
}

static int cu_count() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
            cus = v;
        else
            cus = 256;
    }
    return cus;
}

// The instantiations of gemm_planes_big_kernel by tile index: workgroup tile (32 mt) x (64 nt), eff: the efficiency of the tile shape in
// pick_big's cost model.  Index -1 (5 in a plan answer and in PTMI_GEMM_TILE): the 128 x 128 kernel.
struct Tile { int mt, nt; double eff; };
constexpr Tile TILES[] = {{8, 5, 1.0}, {8, 4, 1.0}, {8, 3, 0.92}, {4, 5, 0.86}, {4, 4, 0.85}};
constexpr int NTILES = 5;

// f(std::integral_constant<int, tile>) for the tile index 0..4 of a plan: f reads its (MT, NT) from TILES as constants
template <int I = NTILES - 1, class F>
static void with_tile(int tile, F&& f) {
    if constexpr (I > 0)
        if (tile != I) return with_tile<I - 1>(tile, f);
    f(std::integral_constant<int, I>{});
}

// f(BF16, ONE, RELU) as std::bool_constants: the five variants either single-product kernel exists in (RELU: fp16, three products)
template <class F>
static void with_variant(bool bf16, bool one, bool relu, F&& f) {
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (relu) return f(no, no, yes);
    if (bf16) return one ? f(yes, yes, no) : f(yes, no, no);
    return one ? f(no, yes, no) : f(no, no, no);
}

// bytes of the planes of an operand with `rows` rows; the big-tile kernel forms piece offsets in 32-bit signed arithmetic, so planes
// of PLANES_LIMIT bytes and more go to the 128 x 128 kernel (a grouped call with such planes is refused)
constexpr long long PLANES_LIMIT = 1ll << 31;
static long long planes_bytes(int rows, int KB) { return (long long)((rows + 15) / 16) * KB * 2048; }

// the k-range count a split_k >= 1 stands for: at most KB, and one that exists (ranges are whole k blocks)
static int whole_ranges(int split_k, int KB) {
    const int splits = std::max(1, std::min(split_k, KB));
    const int per = (KB + splits - 1) / splits;
    return (KB + per - 1) / per;
}

// Picks the tile - and, for calls that allow split K, the number of k ranges - by a cost model fitted to scripts/mb/gemm_big.hip's
// and scripts/exp_wgrad_big.py's measurements (profiles/r3_mb_gemm_big.txt, profiles/r4_wgrad_big_split.txt):
//   time ~ rounds of the CUs x (k blocks per item x tile area / efficiency of the tile shape + an epilogue worth ~10 k blocks)
//          + the slab traffic of the reduction pass ((S + 2) M N floats at ~4 TB/s) + its launch
// with the 128 x 128 kernel (two workgroups per CU at half speed each) as one of the candidates.  Weight-gradient shapes land on
// 128 x 320 / 256 x 320 tiles with as many k ranges as fill ONE round of the CUs (2400 x 1200 x 8096: 76 tiles x 3 ranges, 127 us
// against 148 for the 128 x 128 slabs; x 32192: 40 tiles x 6, 448 against 531 = 0.50 of the 16-bit peak / 3).
struct BigPick { int tile; int splits; };       // tile -1: the 128 x 128 kernel

// (`rows` / `cols`: the products of the call - one, or the blocks of a grouped call, whose tiles and slab traffic add up;
//  always_slabs: every k-range count leaves slabs and runs the reduction pass, S = 1 included - the grouped call;
//  pinned: tile_override() - only that tile is a candidate)
static BigPick pick_big(const int* rows, const int* cols, int nblocks, int KB, int max_splits, bool always_slabs, int pinned) {
    const int cus = cu_count();
    const double unit = 3.1e-5;                  // us per (k block x output element) of a 256-row tile on one CU
    BigPick best{-1, 1};
    double best_cost = 1e300;
    const int smax = std::max(1, std::min(max_splits, KB / 4));
    double elems = 0.0;
    for (int b = 0; b < nblocks; ++b) elems += (double)rows[b] * cols[b];
    for (int i = -1; i < NTILES; ++i) {
        if (pinned >= 0 && pinned != (i < 0 ? 5 : i)) continue;
        const int tr = i < 0 ? 128 : 32 * TILES[i].mt, tc = i < 0 ? 128 : 64 * TILES[i].nt;
        const double area = (double)tr * tc;
        const double eff = i < 0 ? 0.79 : TILES[i].eff;
        long long tiles = 0;
        for (int b = 0; b < nblocks; ++b) tiles += (long long)((rows[b] + tr - 1) / tr) * ((cols[b] + tc - 1) / tc);
        const int slots = i < 0 ? 2 * cus : cus;                 // 128 x 128: two workgroups per CU, each at half the rate
        const double rate = i < 0 ? 2.0 : 1.0;
        for (int S = 1; S <= smax; ++S) {
            const int per = (KB + S - 1) / S;
            if ((KB + per - 1) / per != S) continue;             // this S does not exist (ranges are whole k blocks)
            const long long rounds = (tiles * S + slots - 1) / slots;
            // (calls without split K keep round 3's model - rounds x area / efficiency -, which its measurements were fitted with)
            double cost = (max_splits <= 1 && !always_slabs) ? (double)rounds * rate * area / eff * KB * unit
                                                             : (double)rounds * rate * (per * area * unit / eff + 10.0 * area * unit);
            if (S > 1 || always_slabs) cost += (double)(S + 2) * elems * 4.0 / 4.0e6 + 8.0;
            if (cost < best_cost) {
                best_cost = cost;
                best = BigPick{i, S};
            }
        }
    }
    return best;
}

// What a single-product call runs - gemm_planes_impl launches it, ptmi_gemm_planes_plan encodes it: tile (0..4: TILES, -1: 128 x 128) and
// `splits` k ranges of `kb_per_split` of the KB k blocks, a function of the shape alone, so a call is reproducible bit for bit.
//   split_k > 0: the MOST k ranges the caller's workspace holds; how many are used, and on which tile, is the cost model's choice.
//   split_k < 0: exactly -split_k ranges on the 128 x 128 kernel, whose workgroups (4 wavefronts, 64 KB of LDS) fit on a CU next to a
//                persistent recurrence workgroup, where a big tile needs a whole CU.  A pinned tile takes |split_k| as it is.
struct Plan { int tile, splits, kb_per_split, KB; };

static Plan plan_call(int m, int n, int k, int split_k) {
    const int KB = (k + 31) / 32;
    const bool co_resident = split_k < 0;
    const int splits = whole_ranges(co_resident ? -split_k : split_k, KB), pinned = tile_override();
    BigPick pk = pick_big(&m, &n, 1, KB, (co_resident && pinned < 0) ? 1 : splits, false, pinned);
    if (pinned >= 0) pk.splits = splits;
    else if (co_resident) pk = BigPick{-1, splits};
    if (planes_bytes(m, KB) >= PLANES_LIMIT || planes_bytes(n, KB) >= PLANES_LIMIT) pk.tile = -1;
    return Plan{pk.tile, pk.splits, (KB + pk.splits - 1) / pk.splits, KB};
}

static int32_t plan_code(int tile, int splits) { return (tile < 0 ? 5 : tile) * 100 + splits; }

// A single-product call as its entry point states it: C (+)= A B^T (+ bias), rows from m_split on into c2 where c2 is set.  The entry
// points fill it by field name (designated initializers: in declaration order).
struct PlanesCall {
    const uint16_t *a = nullptr, *b = nullptr;                  // planes: fp16 with the operand scales amax_a / amax_b, or bf16 (no scales)
    const uint32_t *amax_a = nullptr, *amax_b = nullptr;
    const float* bias = nullptr;
    float *c = nullptr, *c2 = nullptr;
    int32_t m_split = 0;
    int64_t ldc = 0;
    int32_t m = 0, n = 0, k = 0, accumulate = 0, split_k = 1;
    int relu = 0;                                               // the fused epilogue of PlanesArgs, with amax_out
    uint32_t* amax_out = nullptr;
    float* workspace = nullptr;                                 // slabs: ptmi_gemm_planes_workspace_elems floats
    bool bf16 = false, one = false;                             // one: only the hi planes are multiplied
    ptmi_stream_t stream = nullptr;
};

// (a launch with slabs leaves bare partial products: bias, accumulate and relu are reduce_slabs' business then; tiles_m / tiles_n: by tile)
static BigArgs big_args(const PlanesCall& q, const Plan& p) {
    const bool slabs = p.splits > 1;
    return {.A = reinterpret_cast<const uint4*>(q.a), .B = reinterpret_cast<const uint4*>(q.b), .C = q.c, .amax_a = q.amax_a, .amax_b = q.amax_b,
            .bias = slabs ? nullptr : q.bias, .M = q.m, .N = q.n, .KB = p.KB, .ldc = q.ldc, .accumulate = (q.accumulate && !slabs) ? 1 : 0,
            .band = 4, .a_bytes = (unsigned)planes_bytes(q.m, p.KB), .b_bytes = (unsigned)planes_bytes(q.n, p.KB), .splits = p.splits,
            .kb_per_split = p.kb_per_split, .slabs = q.workspace, .C2 = q.c2, .m_split = q.m_split, .relu = slabs ? 0 : q.relu,
            .amax_out = q.amax_out};
}

static PlanesArgs planes_args(const PlanesCall& q, const Plan& p) {
    return {.A = reinterpret_cast<const uint4*>(q.a), .B = reinterpret_cast<const uint4*>(q.b), .C = q.c, .workspace = q.workspace,
            .amax_a = q.amax_a, .amax_b = q.amax_b, .bias = q.bias, .M = q.m, .N = q.n, .KB = p.KB, .ldc = q.ldc,
            .accumulate = q.accumulate ? 1 : 0, .kb_per_split = p.kb_per_split, .tiles_m = (q.m + PBM - 1) / PBM, .tiles_n = (q.n + PBN - 1) / PBN,
            .C2 = q.c2, .m_split = q.m_split, .relu = p.splits > 1 ? 0 : q.relu, .amax_out = q.amax_out};
}

// the slabs of a single-product call, summed in slab order into its outputs (with bias, accumulate and the ReLU epilogue)
static int reduce_slabs(const PlanesCall& q, int splits, hipStream_t st) {
    const long long total = (long long)q.m * q.n;
    const unsigned rgrid = (unsigned)std::min<long long>((total + 255) / 256, q.relu ? 1024 : 4096);      // (relu: one atomic per workgroup)
    hipLaunchKernelGGL(planes_reduce_kernel, dim3(rgrid), dim3(256), 0, st, q.workspace, splits, q.c, (long long)q.ldc, q.bias, q.m, q.n,
                       q.accumulate ? 1 : 0, q.c2, q.m_split, q.relu, q.amax_out);
    return launch_status();
}

static int gemm_planes_impl(const PlanesCall& q) {
    PTMI_RETURN_IF(!q.a || !q.b || !q.c || q.m < 1 || q.n < 1 || q.k < 1 || q.ldc < q.n, PTMI_E_INVALID);
    PTMI_RETURN_IF(q.relu && (q.accumulate || q.c2 || q.bf16 || q.one), PTMI_E_INVALID);
    PTMI_RETURN_IF(q.c2 && (q.m_split < 16 || q.m_split >= q.m || q.m_split % 16 != 0), PTMI_E_INVALID);
    PTMI_RETURN_IF(((reinterpret_cast<uintptr_t>(q.a) | reinterpret_cast<uintptr_t>(q.b)) & 15) != 0, PTMI_E_INVALID);
    // (a split_k whose workspace query is not zero needs the workspace, whatever the plan makes of it)
    PTMI_RETURN_IF(!q.workspace && ptmi_gemm_planes_workspace_elems(q.m, q.n, q.k, q.split_k) > 0, PTMI_E_INVALID);
    const Plan p = plan_call(q.m, q.n, q.k, q.split_k);
    const bool relu = q.relu && p.splits == 1;
    hipStream_t st = static_cast<hipStream_t>(q.stream);
    if (p.tile >= 0) {
        BigArgs G = big_args(q, p);
        with_tile(p.tile, [&](auto t) {
            constexpr int MT = TILES[decltype(t)::value].mt, NT = TILES[decltype(t)::value].nt;
            G.tiles_m = (q.m + 32 * MT - 1) / (32 * MT);
            G.tiles_n = (q.n + 64 * NT - 1) / (64 * NT);
            const dim3 grid((unsigned)std::min((G.tiles_m * G.tiles_n * p.splits + 7) / 8 * 8, cu_count() / 8 * 8));
            with_variant(q.bf16, q.one, relu, [&](auto bf16, auto one, auto rl) {
                hipLaunchKernelGGL((gemm_planes_big_kernel<decltype(bf16)::value, MT, NT, decltype(one)::value, decltype(rl)::value>), grid,
                                   dim3(512), 0, st, G);
            });
        });
    } else {
        const PlanesArgs G = planes_args(q, p);
        const dim3 grid((unsigned)((G.tiles_m * G.tiles_n + 7) / 8 * 8), 1u, (unsigned)p.splits);
        with_variant(q.bf16, q.one, relu, [&](auto bf16, auto one, auto rl) {
            hipLaunchKernelGGL((gemm_planes_kernel<decltype(bf16)::value, decltype(one)::value, decltype(rl)::value>), grid, dim3(256), 0, st, G);
        });
    }
    const int rc = launch_status();
    return (rc != PTMI_OK || p.splits == 1) ? rc : reduce_slabs(q, p.splits, st);
}

extern "C" {

int ptmi_gemm_planes_relu(const uint16_t* a, const uint32_t* amax_a, const uint16_t* b, const uint32_t* amax_b, const float* bias, float* c,
                          int64_t ldc, int32_t m, int32_t n, int32_t k, int32_t split_k, int32_t products, float* workspace,
                          uint32_t* amax_out, int32_t amax_zeroed, ptmi_stream_t stream) {
    PTMI_RETURN_IF(products != 3 && products != 1, PTMI_E_INVALID);
    if (amax_out && !amax_zeroed) {
        hipError_t e = zero_words_async(amax_out, 1, static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return (int)e;
    }
    return gemm_planes_impl({.a = a, .b = b, .amax_a = amax_a, .amax_b = amax_b, .bias = bias, .c = c, .ldc = ldc, .m = m, .n = n, .k = k,
                             .split_k = split_k, .relu = 1, .amax_out = amax_out, .workspace = workspace, .one = products == 1, .stream = stream});
}

int ptmi_relu_backward_absmax(const float* g, const float* y, float* out, int64_t rows, int64_t cols, int64_t ld_g, int64_t ld_y,
                              int64_t ld_out, uint32_t* amax_out, int32_t amax_zeroed, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!g || !y || !out || !amax_out || rows < 0 || cols < 0 || ld_g < cols || ld_y < cols || ld_out < cols, PTMI_E_INVALID);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!amax_zeroed) {
        hipError_t e = zero_words_async(amax_out, 1, st);
        if (e != hipSuccess) return (int)e;
    }
    if (rows * cols == 0) return PTMI_OK;
    const long long work = (rows * cols + 4095) / 4096;
    const unsigned grid = (unsigned)std::min<long long>(std::max<long long>(work, 1), 1024);          // (one atomic per workgroup)
    hipLaunchKernelGGL(relu_backward_absmax_kernel, dim3(grid), dim3(256), 0, st, g, y, out, (long long)rows, (long long)cols, (long long)ld_g,
                       (long long)ld_y, (long long)ld_out, amax_out);
    return launch_status();
}

int ptmi_gemm_planes(const uint16_t* a, const uint32_t* amax_a, const uint16_t* b, const uint32_t* amax_b, const float* bias, float* c,
                     int64_t ldc, int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t split_k, int32_t products,
                     float* workspace, ptmi_stream_t stream) {
    PTMI_RETURN_IF(products != 3 && products != 1, PTMI_E_INVALID);
    return gemm_planes_impl({.a = a, .b = b, .amax_a = amax_a, .amax_b = amax_b, .bias = bias, .c = c, .ldc = ldc, .m = m, .n = n, .k = k,
                             .accumulate = accumulate, .split_k = split_k, .workspace = workspace, .one = products == 1, .stream = stream});
}

int32_t ptmi_gemm_planes_plan(int32_t m, int32_t n, int32_t k, int32_t split_k) {
    // what gemm_planes_impl runs for this call: 100 * tile + k ranges (tile 0..4: the big-tile instantiations, 5: 128 x 128)
    if (m < 1 || n < 1 || k < 1) return -1;
    const Plan p = plan_call(m, n, k, split_k);
    return plan_code(p.tile, p.splits);
}

int ptmi_gemm_planes_bf16(const uint16_t* a, const uint16_t* b, const float* bias, float* c, int64_t ldc, int32_t m, int32_t n,
                          int32_t k, int32_t accumulate, int32_t split_k, int32_t products, float* workspace, ptmi_stream_t stream) {
    PTMI_RETURN_IF(products != 3 && products != 1, PTMI_E_INVALID);
    return gemm_planes_impl({.a = a, .b = b, .bias = bias, .c = c, .ldc = ldc, .m = m, .n = n, .k = k, .accumulate = accumulate,
                             .split_k = split_k, .workspace = workspace, .bf16 = true, .one = products == 1, .stream = stream});
}

int ptmi_gemm_planes_bf16_two(const uint16_t* a, const uint16_t* b, float* c, float* c2, int32_t m_split, int64_t ldc, int32_t m,
                              int32_t n, int32_t k, int32_t accumulate, int32_t split_k, int32_t products, float* workspace,
                              ptmi_stream_t stream) {
    PTMI_RETURN_IF((products != 3 && products != 1) || !c2, PTMI_E_INVALID);
    PTMI_RETURN_IF((reinterpret_cast<uintptr_t>(c) ^ reinterpret_cast<uintptr_t>(c2)) & 15, PTMI_E_INVALID);       // one alignment class
    return gemm_planes_impl({.a = a, .b = b, .c = c, .c2 = c2, .m_split = m_split, .ldc = ldc, .m = m, .n = n, .k = k, .accumulate = accumulate,
                             .split_k = split_k, .workspace = workspace, .bf16 = true, .one = products == 1, .stream = stream});
}

// ---------------------------------------------------------------------------------------------------------------- grouped call
int ptmi_pack_planes_t_bf16_list(const float* const* x, const int64_t* cols, const int64_t* ld, uint16_t* const* out, int32_t sources,
                                 int64_t k_rows, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!x || !cols || !ld || !out || sources < 1 || sources > PACK_SRCS || k_rows < 1, PTMI_E_INVALID);
    PackListArgs L{};
    L.krows = k_rows;
    L.KB = (k_rows + 31) / 32;
    PTMI_RETURN_IF(L.KB > 65535, PTMI_E_UNSUPPORTED);
    long long cb = 0;
    for (int i = 0; i < PACK_SRCS; ++i) {
        L.cb_start[i] = (int)cb;
        if (i >= sources) continue;
        PTMI_RETURN_IF(!x[i] || !out[i] || cols[i] < 1 || ld[i] < cols[i], PTMI_E_INVALID);
        PTMI_RETURN_IF((reinterpret_cast<uintptr_t>(out[i]) & 15) != 0, PTMI_E_INVALID);
        L.x[i] = x[i];
        L.out[i] = reinterpret_cast<uint4*>(out[i]);
        L.cols[i] = cols[i];
        L.ld[i] = ld[i];
        L.aligned[i] = (ld[i] % 4 == 0 && (reinterpret_cast<uintptr_t>(x[i]) & 15) == 0) ? 1 : 0;
        cb += (cols[i] + 63) / 64;
        PTMI_RETURN_IF(cb > (1 << 30), PTMI_E_UNSUPPORTED);
    }
    L.cb_start[PACK_SRCS] = (int)cb;
    hipLaunchKernelGGL(pack_planes_t4_kernel<true>, dim3((unsigned)cb, (unsigned)L.KB), dim3(256), 0, static_cast<hipStream_t>(stream), L);
    return launch_status();
}

}  // extern "C"

// the blocks of a grouped call that are not skipped, part-major, and their slab layout for `splits` k ranges
namespace {
struct GroupPlan {
    int nblocks = 0;
    int part[GROUP_BLOCKS], seg[GROUP_BLOCKS], rows[GROUP_BLOCKS], cols[GROUP_BLOCKS];
    long long slab_elems = 0;       // one slab of every block (each rounded up to 4 floats)
};

bool group_plan(GroupPlan& P, int32_t m, int32_t m_split, const int32_t* n, int32_t segments, float* const* c) {
    if (!n || !c || segments < 1 || segments > GROUP_SEGS || m < 2 || m_split < 1 || m_split >= m) return false;
    for (int p = 0; p < 2; ++p)
        for (int s = 0; s < segments; ++s) {
            if (n[s] < 1) return false;
            if (!c[p * segments + s]) continue;
            const int b = P.nblocks++;
            P.part[b] = p;
            P.seg[b] = s;
            P.rows[b] = p ? m - m_split : m_split;
            P.cols[b] = n[s];
            P.slab_elems += ((long long)P.rows[b] * n[s] + 3) / 4 * 4;
        }
    return P.nblocks > 0;
}

// tile (0..4, or -1: the big-tile path is not possible) and k ranges of a grouped call: a function of the shapes alone
BigPick group_choice(const GroupPlan& P, int32_t m, int32_t m_split, const int32_t* n, int32_t segments, int KB, int32_t split_k) {
    const int splits = whole_ranges(split_k, KB), pinned = tile_override();
    BigPick pk = pick_big(P.rows, P.cols, P.nblocks, KB, splits, true, pinned);  // the plain calls' model over the items of ALL blocks
    if (pinned >= 0) pk.splits = splits;                    // a pinned tile takes split_k as it is
    if (m_split % 16 != 0 || planes_bytes(m, KB) >= PLANES_LIMIT) pk.tile = -1;
    for (int s = 0; s < segments; ++s)
        if (planes_bytes(n[s], KB) >= PLANES_LIMIT) pk.tile = -1;
    return pk;
}

template <int MT, int NT>
void launch_group_inst(GroupBigArgs& G, const GroupPlan& P, bool one, hipStream_t st) {
    int t = 0;
    for (int b = 0; b < GROUP_BLOCKS; ++b) {
        G.T.tile_start[b] = b < P.nblocks ? t : 0x7fffffff;
        if (b >= P.nblocks) continue;
        G.T.tiles_m[b] = (P.rows[b] + 32 * MT - 1) / (32 * MT);
        G.T.tiles_n[b] = (P.cols[b] + 64 * NT - 1) / (64 * NT);
        t += G.T.tiles_m[b] * G.T.tiles_n[b];
    }
    G.T.tile_start[GROUP_BLOCKS] = 0x7fffffff;
    G.T.total_tiles = t;
    const int T = t * G.splits;
    const int grid = std::min((T + 7) / 8 * 8, cu_count() / 8 * 8);
    if (one)
        hipLaunchKernelGGL((gemm_planes_big_kernel<true, MT, NT, true, false, GroupBigArgs>), dim3((unsigned)grid), dim3(512), 0, st, G);
    else
        hipLaunchKernelGGL((gemm_planes_big_kernel<true, MT, NT, false, false, GroupBigArgs>), dim3((unsigned)grid), dim3(512), 0, st, G);
}
}  // namespace

extern "C" {

int64_t ptmi_gemm_planes_group_workspace_elems(int32_t m, int32_t m_split, const int32_t* n, int32_t segments, float* const* c, int32_t k,
                                               int32_t split_k) {
    GroupPlan P;
    if (k < 1 || !group_plan(P, m, m_split, n, segments, c)) return 0;
    const int KB = (k + 31) / 32;
    return (int64_t)std::max(1, std::min<int>(split_k, KB)) * P.slab_elems;
}

int32_t ptmi_gemm_planes_group_plan(int32_t m, int32_t m_split, const int32_t* n, int32_t segments, float* const* c, int32_t k,
                                    int32_t split_k) {
    GroupPlan P;
    if (k < 1 || !group_plan(P, m, m_split, n, segments, c)) return -1;
    const BigPick pk = group_choice(P, m, m_split, n, segments, (k + 31) / 32, split_k);
    return plan_code(pk.tile, pk.splits);
}

int ptmi_gemm_planes_bf16_group(const uint16_t* a, int32_t m, int32_t m_split, const uint16_t* const* b, const int32_t* n, int32_t segments,
                                float* const* c, const int64_t* ldc, int32_t k, int32_t accumulate, int32_t split_k, int32_t products,
                                float* workspace, ptmi_stream_t stream) {
    PTMI_RETURN_IF((products != 3 && products != 1) || !a || !b || !ldc || !workspace || k < 1 || split_k < 1, PTMI_E_INVALID);
    GroupPlan P;
    PTMI_RETURN_IF(!group_plan(P, m, m_split, n, segments, c), PTMI_E_INVALID);
    PTMI_RETURN_IF((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(workspace)) & 15, PTMI_E_INVALID);
    for (int q = 0; q < P.nblocks; ++q) {
        const int s = P.seg[q];
        PTMI_RETURN_IF(!b[s] || (reinterpret_cast<uintptr_t>(b[s]) & 15) != 0 || ldc[P.part[q] * segments + s] < n[s], PTMI_E_INVALID);
    }
    const int KB = (k + 31) / 32;
    const BigPick pk = group_choice(P, m, m_split, n, segments, KB, split_k);
    if (pk.tile < 0) return PTMI_E_UNSUPPORTED;         // the caller falls back to separate calls (no other route is taken here)
    hipStream_t st = static_cast<hipStream_t>(stream);
    GroupBigArgs G{};
    G.A = reinterpret_cast<const uint4*>(a);
    G.M = m;
    G.KB = KB;
    G.band = 4;
    G.a_bytes = (unsigned)planes_bytes(m, KB);
    G.splits = pk.splits;
    G.kb_per_split = (KB + pk.splits - 1) / pk.splits;
    G.slabs = workspace;
    G.T.part_rt0[0] = 0;
    G.T.part_rts[0] = m_split / 16;
    G.T.part_rt0[1] = m_split / 16;
    G.T.part_rts[1] = (m - m_split + 15) / 16;
    for (int s = 0; s < segments; ++s) {
        G.T.B[s] = reinterpret_cast<const uint4*>(b[s]);
        G.T.rtb[s] = (n[s] + 15) / 16;
        G.T.b_bytes[s] = (unsigned)planes_bytes(n[s], KB);
    }
    ReduceGroupArgs R{};
    R.ws = workspace;
    R.splits = pk.splits;
    R.nblocks = P.nblocks;
    R.accumulate = accumulate ? 1 : 0;
    long long off = 0, start = 0;
    for (int q = 0; q < P.nblocks; ++q) {
        const long long e = (long long)P.rows[q] * P.cols[q], stride = (e + 3) / 4 * 4;
        G.T.part[q] = P.part[q];
        G.T.seg[q] = P.seg[q];
        G.T.rows[q] = P.rows[q];
        G.T.cols[q] = P.cols[q];
        G.T.slab_off[q] = R.slab_off[q] = off;
        G.T.slab_stride[q] = R.slab_stride[q] = stride;
        R.start[q] = start;
        R.C[q] = c[P.part[q] * segments + P.seg[q]];
        R.ldc[q] = ldc[P.part[q] * segments + P.seg[q]];
        R.cols[q] = P.cols[q];
        R.vec[q] = (P.cols[q] % 4 == 0 && R.ldc[q] % 4 == 0 && (reinterpret_cast<uintptr_t>(R.C[q]) & 15) == 0) ? 1 : 0;
        off += stride * pk.splits;
        start += R.vec[q] ? e / 4 : e;
    }
    for (int q = P.nblocks; q <= GROUP_BLOCKS; ++q) R.start[q] = start;
    with_tile(pk.tile, [&](auto t) {
        constexpr Tile tl = TILES[decltype(t)::value];
        launch_group_inst<tl.mt, tl.nt>(G, P, products == 1, st);
    });
    int rc = launch_status();
    if (rc != PTMI_OK) return rc;
    const unsigned rgrid = (unsigned)std::min<long long>((start + 255) / 256, 4096);
    hipLaunchKernelGGL(planes_reduce_kernel, dim3(rgrid), dim3(256), 0, st, R);
    return launch_status();
}

}  // extern "C"
