// The 2-D convolution blocks of padertorch/contrib/je/modules/conv.py (Conv2d, CNN2d) and Pool2d of conv_utils.py on channels-last rows
// [B, F, T, C] (row (b F + f) T + t): a DIRECT (implicit-GEMM) convolution on v_mfma_f32_16x16x32_f16.  No plane of per-tap products and
// no padded copy exists; an input element is read from HBM about once per layer (the halo overlap of neighbouring tiles aside).
//
//   forward   z[b, fo, to, co] = bias[co] + sum_{kf, kt, ci} a[b, fo s_f + kf d_f - front_f, to s_t + kt d_t - front_t, ci] W[co, ci, kf, kt]
//             (positions outside the plane are zero), the gate convolution's g in the same launch from the same staged input, and, with
//             no normalisation behind, out = act(z) sigmoid(g) + residual in the epilogue.
//   dx        the SAME kernel: sources dz (and dg), taps flipped, weight planes with k order (kf, kt, co), front' = (K - 1) d - front; for
//             a stride s the staging pass writes the zero-inserted dz into LDS (position u holds dz[u / s] where the division is exact),
//             so the zeros never exist in HBM and a position no window reaches comes out as zero.
//   wgrad     dW[q, co, ci, kf, kt] = sum_{b, fo, to} dz_q[b, fo, to, co] a[b, fo s_f + kf d_f - front_f, ...]: a GEMM whose reduction
//             axis is the pixels; both operands are transposed through LDS, the accumulators stay in registers over a contiguous range of
//             pixel tiles, every workgroup writes ONE fp32 slab and colreduce_kernel adds the slabs in order (reduce.h).
//   pool      max (int64 indices f T_padded + t on the padded and trimmed plane) and average pooling with their backward gathers.
//
// Arithmetic (csrc/gemm.hip): operands scaled by the power of two of their absmax word and split into fp16 hi / lo on the way into LDS
// (the weights: once per weight version, je_conv2d_pack_kernel); a b = hi hi + hi lo + lo hi in one fp32 accumulator.
//
// The convolution kernel.  A workgroup (4 wavefronts) owns 8 x 16 output pixels (fo, to) of one example times 64 output channels
// (gated: 32 of z and the same 32 of g).  Per chunk of CC reduction channels (8, 16 or 32; channels are padded with zeros to a multiple of
// 8 in LDS only) it stages the halo, ((8 - 1) s_f + (KF - 1) d_f + 1) x ((16 - 1) s_t + (KT - 1) d_t + 1) positions, as
// [position][hi: CC halves | lo: CC halves | 16 bytes of padding].  An MFMA row tile is 16 neighbouring `to` of one `fo`; the reduction
// index runs over k groups (tap, 8 channels), four groups to a 32-wide k step, so a lane's operand is ONE 16-byte LDS read at the pixel
// (f s_f + kf d_f, t s_t + kt d_t), an address that is arithmetic on the tap.  The pitch: the LDS has 64 banks of 4 bytes, a 16-byte read
// covers 4, so a bank row holds 16 units of 16 bytes; with a pitch of an ODD number of units (4 CC + 16 bytes = 3, 5, 9) the 16 lanes of a
// row tile (neighbouring t, stride 1) read 16 distinct units modulo 16: no conflict.  With s_t = 2 the distance is even, the lanes pair up
// and the reads should take two passes (not measured).  Weight fragments come straight from the packed planes in global memory (16 bytes per lane, contiguous
// per k step, the same for every workgroup of a layer: they live in L2).
#include "je_conv_act.h"

namespace ptmi {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kC2TileF = 8, kC2TileT = 16;      // output pixels of a workgroup
constexpr int kC2LdsLimit = 64 * 1024;          // dynamic LDS a launch may ask for without an attribute
constexpr int kC2WgradLdsLimit = 96 * 1024;     // the weight gradient's, raised by attribute (a compute unit has 160 KB)
constexpr int kC2DzPitch = 136;                 // wgrad: halves per row of the transposed dz tile (128 pixels + 8: 17 16-byte units)

// s = 2^(13 - e) for max|v| = m 2^e (csrc/gemm.hip::operand_scale; a zero or non-finite maximum: 1)
__device__ __forceinline__ float c2_scale(const unsigned* amax_bits) {
    const unsigned e = (*amax_bits >> 23) & 0xffu;
    if (e == 0u || e == 0xffu) return 1.f;
    return __uint_as_float((unsigned)(127 + 13 + 127 - (int)e) << 23);
}

// The geometry of one convolution launch, forward or input gradient.
struct C2Geom {
    long long B, lds, ldr;              // examples; row stride of the sources and of the residual
    int SF, ST, Cs, NS;                 // source plane, channels per source, sources (dx of a gated block: dz and dg)
    int us_f, us_t, VF, VT;             // zero insertion and the virtual plane (S - 1) us + 1 the windows move on
    int OF, OT, Co, NQ;                 // output plane, channels per output, outputs (z and g)
    int KF, KT, sf, st, df, dt, ff, ft; // taps, output stride, dilation, front padding
    int Cp, CC, NCH, KS;                // channels per source padded to 8; chunk; chunks; k steps per chunk
    int HF, HT, pitch;                  // halo, LDS bytes per position
    int tiles_f, tiles_t, tiles_n;
};

struct C2Args {
    const float* src[2];
    const uint4* W;                     // packed planes [tile_n][chunk][k step][slot 4][hi | lo][64 lanes]
    const unsigned *amax_x, *amax_w;
    const float* bias[2];
    const float* residual;
    const float* slope;
    float* z[2];
    float* out;
    int act, vec_in, vec_out;
    float act_p;
};

// fills the derived fields; false: a shape the kernel does not take
static bool c2_plan(C2Geom& G) {
    G.VF = (G.SF - 1) * G.us_f + 1, G.VT = (G.ST - 1) * G.us_t + 1;
    G.Cp = (G.Cs + 7) / 8 * 8;
    const long long hf = (long long)(kC2TileF - 1) * G.sf + (long long)(G.KF - 1) * G.df + 1;
    const long long ht = (long long)(kC2TileT - 1) * G.st + (long long)(G.KT - 1) * G.dt + 1;
    if (hf * ht > 8192) return false;
    G.HF = (int)hf, G.HT = (int)ht;
    const int cv = G.NS * G.Cp;
    G.CC = cv >= 32 ? 32 : (cv >= 16 ? 16 : 8);
    while (G.CC > 8 && hf * ht * (4 * G.CC + 16) > kC2LdsLimit) G.CC /= 2;
    G.pitch = 4 * G.CC + 16;
    if (hf * ht * G.pitch > kC2LdsLimit) return false;
    G.NCH = (cv + G.CC - 1) / G.CC;
    G.KS = (G.KF * G.KT * (G.CC / 8) + 3) / 4;
    G.tiles_f = (G.OF + kC2TileF - 1) / kC2TileF, G.tiles_t = (G.OT + kC2TileT - 1) / kC2TileT;
    G.tiles_n = (G.Co + 64 / G.NQ - 1) / (64 / G.NQ);
    return true;
}

template <int NQ>
__global__ __launch_bounds__(256) void je_conv2d_kernel(const C2Geom G, const C2Args A) {
    extern __shared__ uint4 c2_lds[];
    unsigned char* lds = reinterpret_cast<unsigned char*>(c2_lds);
    constexpr int SLOTS = 4 / NQ;                       // 16-channel tiles per output
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long tile = blockIdx.x;
    const int tt = (int)(tile % G.tiles_t);
    tile /= G.tiles_t;
    const int tf = (int)(tile % G.tiles_f);
    const long long b = tile / G.tiles_f;
    const int tile_n = blockIdx.y, co0 = tile_n * SLOTS * 16;
    const int f0 = tf * kC2TileF, t0 = tt * kC2TileT;
    const int vf0 = f0 * G.sf - G.ff, vt0 = t0 * G.st - G.ft;
    const float sx = c2_scale(A.amax_x), inv = 1.f / (sx * c2_scale(A.amax_w));
    const int taps = G.KF * G.KT, cgc = G.CC / 8, quads = G.CC / 4;
    bool live[SLOTS];                                   // the 16-channel tiles that hold a channel
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) live[j] = co0 + j * 16 < G.Co;
    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[i][s] = f4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < G.NCH; ++ch) {
        __syncthreads();                                // everybody has read the chunk before
        for (int it = tid; it < G.HF * G.HT * quads; it += 256) {
            const int cq = it % quads, pos = it / quads, hf = pos / G.HT, ht = pos - hf * G.HT;
            const int vc = ch * G.CC + cq * 4, s = vc / G.Cp, c = vc - s * G.Cp;
            const int vf = vf0 + hf, vt = vt0 + ht;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (s < G.NS && c < G.Cs && vf >= 0 && vf < G.VF && vt >= 0 && vt < G.VT && vf % G.us_f == 0 && vt % G.us_t == 0) {
                const float* p = A.src[s] + ((b * G.SF + vf / G.us_f) * G.ST + vt / G.us_t) * G.lds + c;
                if (A.vec_in) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < G.Cs) v[e] = p[e];
                }
            }
            h4 hi, lo;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w = v[e] * sx;
                hi[e] = (_Float16)w;
                lo[e] = (_Float16)(w - (float)hi[e]);
            }
            unsigned char* dst = lds + (long long)pos * G.pitch + cq * 8;
            *reinterpret_cast<h4*>(dst) = hi;
            *reinterpret_cast<h4*>(dst + G.CC * 2) = lo;
        }
        __syncthreads();
        const uint4* wp = A.W + (((long long)tile_n * G.NCH + ch) * G.KS) * 8 * 64 + lane;
        for (int ks = 0; ks < G.KS; ++ks, wp += 8 * 64) {
            const int kg = ks * 4 + (lane >> 4);
            int tap = kg / cgc;
            const int cg = kg - tap * cgc;
            if (tap >= taps) tap = taps - 1;            // a k group past the taps: its weights are zero, the read stays inside the halo
            const int kf = tap / G.KT, kt = tap - kf * G.KT;
            h8 wh[4], wl[4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (live[s % SLOTS]) {
                    wh[s] = __builtin_bit_cast(h8, wp[(s * 2) * 64]);
                    wl[s] = __builtin_bit_cast(h8, wp[(s * 2 + 1) * 64]);
                }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int pos = ((wave * 2 + i) * G.sf + kf * G.df) * G.HT + (lane & 15) * G.st + kt * G.dt;
                const unsigned char* xp = lds + (long long)pos * G.pitch + cg * 16;
                const h8 xh = *reinterpret_cast<const h8*>(xp), xl = *reinterpret_cast<const h8*>(xp + G.CC * 2);
                // D[co = 4 (lane >> 4) + e][pixel = lane & 15]: a lane holds four neighbouring channels of one pixel
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (live[s % SLOTS]) {
                        acc[i][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], xh, acc[i][s], 0, 0, 0);
                        acc[i][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[s], xl, acc[i][s], 0, 0, 0);
                        acc[i][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[s], xh, acc[i][s], 0, 0, 0);
                    }
            }
        }
    }

    const float p = (A.act == kActPrelu && A.slope) ? A.slope[0] : A.act_p;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int fo = f0 + wave * 2 + i, to = t0 + (lane & 15);
        if (fo >= G.OF || to >= G.OT) continue;
        const long long row = (b * G.OF + fo) * G.OT + to;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int co = co0 + j * 16 + (lane >> 4) * 4;
            if (co >= G.Co) continue;
            const bool full = A.vec_out && co + 3 < G.Co;
            float v[NQ][4], o[4];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = co + e < G.Co ? co + e : G.Co - 1;
                    v[q][e] = acc[i][q * SLOTS + j][e] * inv + (A.bias[q] ? A.bias[q][c] : 0.f);
                }
                float* zp = A.z[q] + row * G.Co + co;
                if (full) {
                    *reinterpret_cast<float4*>(zp) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < G.Co) zp[e] = v[q][e];
                }
            }
            if (!A.out) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = jc_act(v[0][e], A.act, p);
                if (NQ == 2) a *= jc_sigmoid(v[NQ - 1][e]);
                if (A.residual && co + e < G.Co) a += A.residual[row * G.ldr + co + e];
                o[e] = a;
            }
            float* op = A.out + row * G.Co + co;
            if (full) {
                *reinterpret_cast<float4*>(op) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (co + e < G.Co) op[e] = o[e];
            }
        }
    }
}

// The weight planes of a layer in fragment order.  mode 0 (forward): row n = channel co of output q, value W_q[co, c, kf, kt];
// mode 1 (dx): row n = input channel, source s = convolution q, value W_s[c, n, KF - 1 - kf, KT - 1 - kt].  One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void je_conv2d_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                                             const unsigned* __restrict__ amax, uint4* __restrict__ out, const C2Geom G,
                                                             const int mode, const long long chunks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const int lane = (int)(i & 63), plane = (int)((i >> 6) & 1), slot = (int)((i >> 7) & 3);
    long long rest = i >> 9;
    const int ks = (int)(rest % G.KS);
    rest /= G.KS;
    const int ch = (int)(rest % G.NCH), tile_n = (int)(rest / G.NCH);
    const int slots = 4 / G.NQ, q = slot / slots, n = (tile_n * slots + slot % slots) * 16 + (lane & 15);
    const int cgc = G.CC / 8, kg = ks * 4 + (lane >> 4), tap = kg / cgc, cg = kg - tap * cgc;
    const int kf = tap / G.KT, kt = tap - kf * G.KT;
    const float s = c2_scale(amax);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int vc = ch * G.CC + cg * 8 + e, src = vc / G.Cp, c = vc - src * G.Cp;
        float v = 0.f;
        if (tap < G.KF * G.KT && n < G.Co && src < G.NS && c < G.Cs) {
            if (mode == 0)
                v = (q ? w1 : w0)[(((long long)n * G.Cs + c) * G.KF + kf) * G.KT + kt];
            else
                v = (src ? w1 : w0)[(((long long)c * G.Co + n) * G.KF + (G.KF - 1 - kf)) * G.KT + (G.KT - 1 - kt)];
        }
        v *= s;
        const _Float16 hi = (_Float16)v;
        o[e] = plane ? (_Float16)(v - (float)hi) : hi;
    }
    out[i] = __builtin_bit_cast(uint4, o);
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
struct C2Wgrad {
    const float* dz[2];
    const float* x;
    float* ws;                          // [slabs][G Co][Ci taps]
    const unsigned *amax_dz, *amax_x;
    long long B, ldx, tiles, tiles_per_slab;
    int IF, IT, Ci, OF, OT, Co, NQ, KF, KT, sf, st, df, dt, ff, ft, HF, HT, HP, tiles_f, tiles_t, vec_dz;
};

// A workgroup owns 64 rows m = q Co + co and 64 columns n = ci taps + tap of dW (wavefront w: the 16 columns n0 + 16 w, all four row
// tiles) and a range of pixel tiles.  Per tile it stages dz transposed, [hi | lo][row][128 pixels], and the halo of the input channels its
// columns touch, [hi | lo][channel][position]: the dz operand is one 16-byte read (8 neighbouring `to`), the input operand eight 2-byte
// reads (8 neighbouring `to` of the tap's shifted row; their start is not 16-byte aligned and, with s_t > 1, they are not neighbours).
__global__ __launch_bounds__(256) void je_conv2d_wgrad_kernel(const C2Wgrad A) {
    extern __shared__ uint4 c2_lds[];
    _Float16* dzt = reinterpret_cast<_Float16*>(c2_lds);                // [2][64][kC2DzPitch]
    _Float16* halo = dzt + 2 * 64 * kC2DzPitch;                         // [2][nci][HP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int taps = A.KF * A.KT, M = A.NQ * A.Co, N = A.Ci * taps;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int n_last = n0 + 63 < N ? n0 + 63 : N - 1;
    const int ci_lo = n0 / taps, nci = n_last / taps - ci_lo + 1;
    const int n_mine = n0 + wave * 16 + (lane & 15);
    const bool n_ok = n_mine < N;
    const int cl = n_ok ? n_mine / taps - ci_lo : 0, tap = n_ok ? n_mine % taps : 0, kf = tap / A.KT, kt = tap - kf * A.KT;
    const float sd = c2_scale(A.amax_dz), sx = c2_scale(A.amax_x), inv = 1.f / (sd * sx);
    const long long halo_plane = (long long)nci * A.HP;
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    bool live[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) live[i] = m0 + i * 16 < M;

    const long long first = blockIdx.z * A.tiles_per_slab, last = first + A.tiles_per_slab < A.tiles ? first + A.tiles_per_slab : A.tiles;
    for (long long tile = first; tile < last; ++tile) {
        const int tt = (int)(tile % A.tiles_t), tf = (int)((tile / A.tiles_t) % A.tiles_f);
        const long long b = tile / ((long long)A.tiles_t * A.tiles_f);
        const int f0 = tf * kC2TileF, t0 = tt * kC2TileT;
        __syncthreads();
        for (int it = tid; it < 128 * 16; it += 256) {
            const int rq = it & 15, px = it >> 4, fo = f0 + (px >> 4), to = t0 + (px & 15);
            const bool inside = fo < A.OF && to < A.OT;
            const long long row = (b * A.OF + fo) * A.OT + to;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            const int m = m0 + rq * 4;
            if (inside && A.vec_dz && m < M) {
                const float4 q = *reinterpret_cast<const float4*>(A.dz[m / A.Co] + row * A.Co + m % A.Co);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else if (inside) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (m + e < M) v[e] = A.dz[(m + e) / A.Co][row * A.Co + (m + e) % A.Co];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w = v[e] * sd;
                const _Float16 hi = (_Float16)w;
                dzt[(rq * 4 + e) * kC2DzPitch + px] = hi;
                dzt[(64 + rq * 4 + e) * kC2DzPitch + px] = (_Float16)(w - (float)hi);
            }
        }
        for (int it = tid; it < A.HP * nci; it += 256) {
            const int c = it % nci, pos = it / nci, hf = pos / A.HT, ht = pos - hf * A.HT;
            const int vf = f0 * A.sf - A.ff + hf, vt = t0 * A.st - A.ft + ht;
            float v = 0.f;
            if (vf >= 0 && vf < A.IF && vt >= 0 && vt < A.IT) v = A.x[((b * A.IF + vf) * A.IT + vt) * A.ldx + ci_lo + c] * sx;
            const _Float16 hi = (_Float16)v;
            halo[(long long)c * A.HP + pos] = hi;
            halo[halo_plane + (long long)c * A.HP + pos] = (_Float16)(v - (float)hi);
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int p0 = ks * 32 + (lane >> 4) * 8;                  // this lane's 8 pixels: row p0 / 16 of the tile, from t = p0 % 16
            const long long base = (long long)cl * A.HP + ((p0 >> 4) * A.sf + kf * A.df) * A.HT + (p0 & 15) * A.st + kt * A.dt;
            h8 bh, bl;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bh[j] = halo[base + j * A.st];
                bl[j] = halo[halo_plane + base + j * A.st];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (live[i]) {
                    const _Float16* ap = dzt + (i * 16 + (lane & 15)) * kC2DzPitch + p0;
                    const h8 ah = *reinterpret_cast<const h8*>(ap), al = *reinterpret_cast<const h8*>(ap + 64 * kC2DzPitch);
                    // D[n = 4 (lane >> 4) + e][m = lane & 15]
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, ah, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh, al, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl, ah, acc[i], 0, 0, 0);
                }
        }
    }
    float* slab = A.ws + (long long)blockIdx.z * M * N;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + i * 16 + (lane & 15), n = n0 + wave * 16 + (lane >> 4) * 4;
        if (m >= M) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (n + e < N) slab[(long long)m * N + n + e] = acc[i][e] * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------- pools
struct C2Pool {
    long long B, ldx;
    int IF, IT, OF, OT, C, kf, kt, sf, st, ff, ft, TP;         // TP: the width of the padded and trimmed plane the indices count on
};

static bool c2_pool(const int64_t* g, C2Pool& P) {
    if (!g) return false;
    for (int i = 0; i < 13; ++i)
        if (g[i] < (i >= 11 ? 0 : 1) || g[i] > 0x3fffffff) return false;
    P.B = g[0], P.IF = (int)g[1], P.IT = (int)g[2], P.OF = (int)g[3], P.OT = (int)g[4], P.C = (int)g[5], P.kf = (int)g[6], P.kt = (int)g[7];
    P.sf = (int)g[8], P.st = (int)g[9], P.ff = (int)g[11], P.ft = (int)g[12], P.ldx = g[10];
    P.TP = (P.OT - 1) * P.st + P.kt;
    // the first position of the last window is a row of the input or of its end padding
    return P.ldx >= P.C && (long long)(P.OF - 1) * P.sf - P.ff < P.IF && (long long)(P.OT - 1) * P.st - P.ft < P.IT;
}

// the padded plane holds zeros around the IF x IT values, and they take part in the maximum
template <int V, bool MAX>
__global__ __launch_bounds__(256) void je_pool2d_forward_kernel(const float* __restrict__ x, const C2Pool P, float* __restrict__ y,
                                                                long long* __restrict__ index) {
    const int CG = P.C / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.B * P.OF * P.OT * CG) return;
    const int c = (int)(i % CG) * V;
    const long long r = i / CG;
    const int to = (int)(r % P.OT), fo = (int)((r / P.OT) % P.OF);
    const long long b = r / ((long long)P.OT * P.OF);
    float best[V], sum[V];
    long long at[V];
#pragma unroll
    for (int v = 0; v < V; ++v) best[v] = -INFINITY, sum[v] = 0.f, at[v] = (long long)fo * P.sf * P.TP + (long long)to * P.st;
    for (int a = 0; a < P.kf; ++a)
        for (int w = 0; w < P.kt; ++w) {
            const int pf = fo * P.sf + a, pt = to * P.st + w, f = pf - P.ff, t = pt - P.ft;
            float val[V];
#pragma unroll
            for (int v = 0; v < V; ++v) val[v] = 0.f;
            if (f >= 0 && f < P.IF && t >= 0 && t < P.IT) load_vec<V>(x + ((b * P.IF + f) * P.IT + t) * P.ldx + c, val);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if constexpr (MAX) {
                    // the first of equal values in row-major window order; a NaN beats every number (nn.MaxPool2d)
                    if (val[v] > best[v] || val[v] != val[v]) best[v] = val[v], at[v] = (long long)pf * P.TP + pt;
                } else {
                    sum[v] += val[v];
                }
            }
        }
    if constexpr (MAX) {
        store_vec<V>(y + r * P.C + c, best);
#pragma unroll
        for (int v = 0; v < V; ++v) index[r * P.C + c + v] = at[v];
    } else {
        const float n = (float)(P.kf * P.kt);
#pragma unroll
        for (int v = 0; v < V; ++v) sum[v] /= n;
        store_vec<V>(y + r * P.C + c, sum);
    }
}

// dx [B, IF, IT, C] contiguous, every element written: the windows that hold the position, ascending (fo, then to)
template <int V, bool MAX>
__global__ __launch_bounds__(256) void je_pool2d_backward_kernel(const float* __restrict__ dy, const long long* __restrict__ index,
                                                                 const C2Pool P, float* __restrict__ dx) {
    const int CG = P.C / V;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.B * P.IF * P.IT * CG) return;
    const int c = (int)(i % CG) * V;
    const long long r = i / CG;
    const int t = (int)(r % P.IT), f = (int)((r / P.IT) % P.IF);
    const long long b = r / ((long long)P.IT * P.IF);
    const int pf = f + P.ff, pt = t + P.ft;
    const int flo = pf - P.kf + 1 <= 0 ? 0 : (pf - P.kf + P.sf) / P.sf, fhi = pf / P.sf < P.OF - 1 ? pf / P.sf : P.OF - 1;
    const int tlo = pt - P.kt + 1 <= 0 ? 0 : (pt - P.kt + P.st) / P.st, thi = pt / P.st < P.OT - 1 ? pt / P.st : P.OT - 1;
    const long long me = (long long)pf * P.TP + pt;
    const float n = (float)(P.kf * P.kt);
    float s[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = 0.f;
    for (int fo = flo; fo <= fhi; ++fo)
        for (int to = tlo; to <= thi; ++to) {
            const long long o = ((b * P.OF + fo) * P.OT + to) * P.C + c;
            float g[V];
            load_vec<V>(dy + o, g);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if constexpr (MAX) {
                    if (index[o + v] == me) s[v] += g[v];
                } else {
                    s[v] += g[v] / n;
                }
            }
        }
    store_vec<V>(dx + r * P.C + c, s);
}

static bool c2_geom(const int64_t* g, C2Geom& G) {
    if (!g) return false;
    for (int i = 0; i < 21; ++i)
        if (g[i] < (i >= 17 && i < 19 ? 0 : 1) || g[i] > 0x3fffffff) return false;
    G.B = g[0], G.SF = (int)g[1], G.ST = (int)g[2], G.Cs = (int)g[3], G.NS = (int)g[4], G.us_f = (int)g[5], G.us_t = (int)g[6];
    G.OF = (int)g[7], G.OT = (int)g[8], G.Co = (int)g[9], G.NQ = (int)g[10], G.KF = (int)g[11], G.KT = (int)g[12], G.sf = (int)g[13];
    G.st = (int)g[14], G.df = (int)g[15], G.dt = (int)g[16], G.ff = (int)g[17], G.ft = (int)g[18], G.lds = g[19], G.ldr = g[20];
    if (G.NS > 2 || G.NQ > 2 || G.KF > 64 || G.KT > 64 || G.lds < G.Cs || G.ldr < G.Co) return false;
    return c2_plan(G) && G.B * G.tiles_f * G.tiles_t <= 0x7fffffffLL && G.tiles_n <= 65535;
}

static long long c2_pack_chunks(const C2Geom& G) { return (long long)G.tiles_n * G.NCH * G.KS * 8 * 64; }

// The geometry of a weight-gradient launch from geom [17] (ptmi.h): the launch's dynamic LDS in bytes; 0: a shape the kernel does not
// take (the transposed dz tile and the halo of the input channels of 64 columns beyond kC2WgradLdsLimit); -1: not a geometry.
static long long c2_wgrad_plan(const int64_t* geom, C2Wgrad& A) {
    if (!geom) return -1;
    for (int i = 0; i < 17; ++i)
        if (geom[i] < (i == 14 || i == 15 ? 0 : 1) || geom[i] > 0x3fffffff) return -1;
    A.B = geom[0], A.IF = (int)geom[1], A.IT = (int)geom[2], A.Ci = (int)geom[3], A.OF = (int)geom[4], A.OT = (int)geom[5];
    A.Co = (int)geom[6], A.NQ = (int)geom[7], A.KF = (int)geom[8], A.KT = (int)geom[9], A.sf = (int)geom[10], A.st = (int)geom[11];
    A.df = (int)geom[12], A.dt = (int)geom[13], A.ff = (int)geom[14], A.ft = (int)geom[15], A.ldx = geom[16];
    if (A.NQ > 2 || A.KF > 64 || A.KT > 64 || A.ldx < A.Ci) return -1;
    const long long hf = (long long)(kC2TileF - 1) * A.sf + (long long)(A.KF - 1) * A.df + 1;
    const long long ht = (long long)(kC2TileT - 1) * A.st + (long long)(A.KT - 1) * A.dt + 1;
    const long long taps = (long long)A.KF * A.KT, M = (long long)A.NQ * A.Co, N = A.Ci * taps;
    long long nci = (62 + taps) / taps + 1;             // the input channels 64 neighbouring columns ci taps + tap can touch
    if (nci > A.Ci) nci = A.Ci;
    const long long lds = 2 * 64 * kC2DzPitch * 2 + 2 * nci * hf * ht * 2;
    if (hf * ht > 8192 || lds > kC2WgradLdsLimit || M * N > 0x7fffffffLL || (N + 63) / 64 > 65535) return 0;
    A.HF = (int)hf, A.HT = (int)ht, A.HP = (int)(hf * ht);
    A.tiles_f = (A.OF + kC2TileF - 1) / kC2TileF, A.tiles_t = (A.OT + kC2TileT - 1) / kC2TileT;
    A.tiles = A.B * A.tiles_f * A.tiles_t;
    return lds;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_je_conv2d_pack_elems(const int64_t* geom) {
    C2Geom G;
    return c2_geom(geom, G) ? c2_pack_chunks(G) * 8 : 0;
}

int64_t ptmi_je_conv2d_wgrad_lds(const int64_t* geom) {
    C2Wgrad A;
    const long long lds = c2_wgrad_plan(geom, A);
    return lds > 0 ? lds : 0;
}

int ptmi_je_conv2d_pack(const float* w0, const float* w1, const uint32_t* amax, uint16_t* planes, const int64_t* geom, int32_t input_grad,
                        ptmi_stream_t stream) {
    C2Geom G;
    PTMI_RETURN_IF(!w0 || !amax || !planes || !c2_geom(geom, G), PTMI_E_INVALID);
    PTMI_RETURN_IF(!w1 && (input_grad ? G.NS : G.NQ) == 2, PTMI_E_INVALID);
    const long long chunks = c2_pack_chunks(G);
    PTMI_RETURN_IF((chunks + 255) / 256 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(je_conv2d_pack_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w0, w1,
                       amax, reinterpret_cast<uint4*>(planes), G, input_grad, chunks);
    return launch_status();
}

int ptmi_je_conv2d_forward(const float* x0, const float* x1, const uint16_t* planes, const uint32_t* amax_x, const uint32_t* amax_w,
                           const float* bias, const float* gate_bias, const float* residual, const float* slope, float* z, float* gz,
                           float* out, const int64_t* geom, int32_t act, float act_p, ptmi_stream_t stream) {
    C2Geom G;
    PTMI_RETURN_IF(!x0 || !planes || !amax_x || !amax_w || !z || !geom, PTMI_E_INVALID);
    PTMI_RETURN_IF(!c2_geom(geom, G), PTMI_E_UNSUPPORTED);
    PTMI_RETURN_IF((G.NS == 2 && !x1) || (G.NQ == 2 && !gz) || act < kActIdentity || act > kActPrelu, PTMI_E_INVALID);
    PTMI_RETURN_IF(act == kActPrelu && out && !slope, PTMI_E_INVALID);
    C2Args A;
    A.src[0] = x0, A.src[1] = x1, A.W = reinterpret_cast<const uint4*>(planes), A.amax_x = amax_x, A.amax_w = amax_w;
    A.bias[0] = bias, A.bias[1] = gate_bias, A.residual = residual, A.slope = slope, A.z[0] = z, A.z[1] = gz, A.out = out;
    A.act = act, A.act_p = act_p;
    A.vec_in = G.Cs % 4 == 0 && G.lds % 4 == 0 && aligned16({x0, x1});
    A.vec_out = G.Co % 4 == 0 && aligned16({z, gz, out});
    const dim3 grid((unsigned)(G.B * G.tiles_f * G.tiles_t), (unsigned)G.tiles_n);
    const size_t lds = (size_t)G.HF * G.HT * G.pitch;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (G.NQ == 2)
        hipLaunchKernelGGL((je_conv2d_kernel<2>), grid, dim3(256), lds, st, G, A);
    else
        hipLaunchKernelGGL((je_conv2d_kernel<1>), grid, dim3(256), lds, st, G, A);
    return launch_status();
}

// geom: B, IF, IT, Ci, OF, OT, Co, G, KF, KT, s_f, s_t, d_f, d_t, front_f, front_t, ldx
int ptmi_je_conv2d_wgrad(const float* dz, const float* dgz, const float* x, const uint32_t* amax_dz, const uint32_t* amax_x,
                         float* workspace, int64_t slabs, float* dw, const int64_t* geom, ptmi_stream_t stream) {
    PTMI_RETURN_IF(!dz || !x || !amax_dz || !amax_x || !workspace || !dw || !geom || slabs < 1 || slabs > 65535, PTMI_E_INVALID);
    C2Wgrad A;
    const long long lds = c2_wgrad_plan(geom, A);
    PTMI_RETURN_IF(lds < 0 || (A.NQ == 2 && !dgz), PTMI_E_INVALID);
    PTMI_RETURN_IF(lds == 0, PTMI_E_UNSUPPORTED);
    A.dz[0] = dz, A.dz[1] = dgz, A.x = x, A.ws = workspace, A.amax_dz = amax_dz, A.amax_x = amax_x;
    // a 1 x 1 layer with 64 or more input channels needs 66 KB (34 KB of dz, 32 KB of input): beyond what a launch gets unasked
    static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(je_conv2d_wgrad_kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, kC2WgradLdsLimit);
    PTMI_RETURN_IF(lds > kC2LdsLimit && raised != hipSuccess, PTMI_E_UNSUPPORTED);
    A.tiles_per_slab = (A.tiles + slabs - 1) / slabs;
    A.vec_dz = A.Co % 4 == 0 && aligned16({dz, dgz});
    const long long M = (long long)A.NQ * A.Co, N = (long long)A.Ci * A.KF * A.KT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(je_conv2d_wgrad_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((N + 63) / 64), (unsigned)slabs), dim3(256),
                       (size_t)lds, st, A);
    int rc = launch_status();
    if (rc) return rc;
    return colreduce(workspace, slabs, M * N, StorePlain{dw}, st);
}

int ptmi_je_pool2d_forward(const float* x, float* y, int64_t* index, const int64_t* geom, int32_t max_pool, ptmi_stream_t stream) {
    C2Pool P;
    PTMI_RETURN_IF(!x || !y || !c2_pool(geom, P) || (max_pool && !index), PTMI_E_INVALID);
    const bool vec = P.C % 4 == 0 && P.ldx % 4 == 0 && aligned16({x, y});
    const long long blocks = (P.B * P.OF * P.OT * (P.C / (vec ? 4 : 1)) + 255) / 256;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* ip = reinterpret_cast<long long*>(index);
    if (max_pool && vec)
        hipLaunchKernelGGL((je_pool2d_forward_kernel<4, true>), dim3((unsigned)blocks), dim3(256), 0, st, x, P, y, ip);
    else if (max_pool)
        hipLaunchKernelGGL((je_pool2d_forward_kernel<1, true>), dim3((unsigned)blocks), dim3(256), 0, st, x, P, y, ip);
    else if (vec)
        hipLaunchKernelGGL((je_pool2d_forward_kernel<4, false>), dim3((unsigned)blocks), dim3(256), 0, st, x, P, y, ip);
    else
        hipLaunchKernelGGL((je_pool2d_forward_kernel<1, false>), dim3((unsigned)blocks), dim3(256), 0, st, x, P, y, ip);
    return launch_status();
}

int ptmi_je_pool2d_backward(const float* dy, const int64_t* index, float* dx, const int64_t* geom, int32_t max_pool, ptmi_stream_t stream) {
    C2Pool P;
    PTMI_RETURN_IF(!dy || !dx || !c2_pool(geom, P) || (max_pool && !index), PTMI_E_INVALID);
    const bool vec = P.C % 4 == 0 && aligned16({dy, dx});
    const long long blocks = (P.B * P.IF * P.IT * (P.C / (vec ? 4 : 1)) + 255) / 256;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* ip = reinterpret_cast<const long long*>(index);
    if (max_pool && vec)
        hipLaunchKernelGGL((je_pool2d_backward_kernel<4, true>), dim3((unsigned)blocks), dim3(256), 0, st, dy, ip, P, dx);
    else if (max_pool)
        hipLaunchKernelGGL((je_pool2d_backward_kernel<1, true>), dim3((unsigned)blocks), dim3(256), 0, st, dy, ip, P, dx);
    else if (vec)
        hipLaunchKernelGGL((je_pool2d_backward_kernel<4, false>), dim3((unsigned)blocks), dim3(256), 0, st, dy, ip, P, dx);
    else
        hipLaunchKernelGGL((je_pool2d_backward_kernel<1, false>), dim3((unsigned)blocks), dim3(256), 0, st, dy, ip, P, dx);
    return launch_status();
}

}  // extern "C"
