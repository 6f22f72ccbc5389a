// The transposed convolution blocks of padertorch/contrib/je/modules/conv.py (ConvTranspose1d / 2d, CNNTranspose1d / 2d) and Unpool1d /
// Unpool2d of conv_utils.py on channels-last rows [B, F, T, C] (row (b F + f) T + t; the 1-D classes: F = 1): a SUB-PIXEL (phase-split)
// direct convolution on v_mfma_f32_16x16x32_f16 that never stages or multiplies an inserted zero.
//
//   y[b, o_f, o_t, co] = bias[co] + sum over (ci, k_f, k_t) with u - k d divisible by s (u = o + front, per axis) and i = (u - k d) / s
//                        inside the input plane of x[b, i_f, i_t, ci] W[ci, co, k_f, k_t]          (torch.nn.ConvTranspose2d's layout)
//
// Per axis an output position belongs to phase r = u mod s; only the taps with k d = r (mod s) reach it, and with u = r + s q they read
// i = q - (k d - r) / s: an offset that does not depend on q.  The pixels of one phase, indexed by q, are a dense grid on which the layer
// is a stride-1 convolution over the phase's taps.  `front` (the reference's trim) only shifts u: trimmed positions are masked at the
// store and never exist; every phase shares the grid q in [front / s, (O - 1 + front) / s].
//
// A workgroup (4 wavefronts) owns ONE phase (r_f, r_t): 8 x 16 neighbouring pixels of its grid (1 x 128 when the grid has one row) times
// 64 output channels (gated: 32 of z and the same 32 of g).  Per chunk of CC input channels (8 / 16 / 32, padded with zeros to 8 in LDS
// only) it stages the DENSE input halo, (8 + max offset_f) x (16 + max offset_t) positions with max offset = (K - 1) d / s, as
// [position][hi: CC halves | lo: CC halves | 16 bytes] (csrc/je_conv2d.hip's form, scale and split).  The reduction runs over k groups
// (tap of this phase, 8 channels), four to a k step; a row tile is 16 neighbouring q_t, so its 16 lanes read neighbouring positions of an
// odd pitch in 16-byte units: conflict-free at every stride.  A phase without a tap (stride beyond the kernel extent, or stride and
// dilation sharing a factor) has no k step: it stages nothing and writes the bias through the epilogue.  The weight planes are packed once
// per weight version by je_conv_transpose_pack_kernel: [channel tile][chunk][phase][k step][slot 4][hi | lo][64 lanes], k order (tap within
// the phase, channel).  The phase table (per axis: the taps in phase order) comes from the host, which also hands it to the tests.
//
// Backward: NO new arithmetic kernel.  dx of a transposed convolution is the plain strided convolution of dy with the same, unflipped
// weights (W[C_in, C_out, K_f, K_t] read as a Conv2d weight has C_in outputs and C_out inputs): ptmi_je_conv2d_forward in mode 0; dW is
// ptmi_je_conv2d_wgrad with the roles exchanged (x on the pixel grid, dy under the taps), whose columns are this weight layout.
//
// Unpooling (gather form, no atomics): with indices, MaxUnpool on the padded and trimmed plane followed by the reference's trim - output
// position p takes x[w] of the LAST window w (row-major) that holds p and whose stored index is p, else zero; without, nearest
// upsampling by the stride.  The backward is the matching gather / block sum.
#include "je_conv_act.h"

namespace ptmi {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kCtLdsLimit = 64 * 1024;          // dynamic LDS a launch may ask for without an attribute
constexpr int kCtMaxK = 16, kCtMaxS = 16, kCtMaxPhases = 64;
constexpr int kCtTapTable = kCtMaxK * kCtMaxK * 4;      // bytes in front of the halo: the LDS offset of every tap of the phase

// s = 2^(13 - e) for max|v| = m 2^e (csrc/gemm.hip::operand_scale; a zero or non-finite maximum: 1)
__device__ __forceinline__ float ct_scale(const unsigned* amax_bits) {
    const unsigned e = (*amax_bits >> 23) & 0xffu;
    if (e == 0u || e == 0xffu) return 1.f;
    return __uint_as_float((unsigned)(127 + 13 + 127 - (int)e) << 23);
}

struct CtGeom {
    long long B, ldx, ldr;
    int IF, IT, Ci, OF, OT, Co, NQ;             // input plane, output window, outputs (z and g)
    int KF, KT, sf, st, df, dt, ff, ft;
    int Cp, CC, NCH, KStot;                     // channels padded to 8; chunk; chunks; k steps of all phases per (channel tile, chunk)
    int TF, TT, mf, mt, HF, HT, pitch;          // pixel tile, largest tap offsets, halo, LDS bytes per position
    int QF0, QT0, tiles_f, tiles_t, tiles_n, phases;
    unsigned char tap_f[kCtMaxK], tap_t[kCtMaxK];               // the taps in phase order
    unsigned char start_f[kCtMaxS + 1], start_t[kCtMaxS + 1];   // phase r: entries start[r] .. start[r + 1]
    unsigned short ks_base[kCtMaxPhases + 1];                   // phase r_f s_t + r_t: k steps ks_base[p] .. ks_base[p + 1]
};

struct CtArgs {
    const float* x;
    const uint4* W;
    const unsigned *amax_x, *amax_w;
    const float* bias[2];
    const float* residual;
    const float* slope;
    float* z[2];
    float* out;
    int act, vec_in, vec_out;
    float act_p;
};

// one axis of the phase table from the host's tap order; false: not the taps of this axis in phase order
static bool ct_axis(const int64_t* order, int K, int s, int d, unsigned char* tap, unsigned char* start) {
    bool seen[kCtMaxK] = {};
    int r = 0;
    start[0] = 0;
    for (int j = 0; j < K; ++j) {
        const int64_t k = order[j];
        if (k < 0 || k >= K || seen[k]) return false;
        seen[k] = true;
        const int p = (int)(k * d % s);
        if (p < r) return false;
        while (r < p) start[++r] = (unsigned char)j;
        tap[j] = (unsigned char)k;
    }
    while (r < s) start[++r] = (unsigned char)K;
    return true;
}

// geom [18 + K_f + K_t] (ptmi.h); false: not a geometry, or one the kernel does not take (`invalid` tells which)
static bool ct_geom(const int64_t* g, CtGeom& G, bool& invalid) {
    invalid = true;
    if (!g) return false;
    for (int i = 0; i < 18; ++i)
        if (g[i] < (i == 14 || i == 15 ? 0 : 1) || g[i] > 0x3fffffff) return false;
    G.B = g[0], G.IF = (int)g[1], G.IT = (int)g[2], G.Ci = (int)g[3], G.OF = (int)g[4], G.OT = (int)g[5], G.Co = (int)g[6], G.NQ = (int)g[7];
    G.KF = (int)g[8], G.KT = (int)g[9], G.sf = (int)g[10], G.st = (int)g[11], G.df = (int)g[12], G.dt = (int)g[13], G.ff = (int)g[14];
    G.ft = (int)g[15], G.ldx = g[16], G.ldr = g[17];
    if (G.NQ > 2 || G.ldx < G.Ci || G.ldr < G.Co) return false;
    // the window lies inside the full output (I - 1) s + (K - 1) d + 1
    if ((long long)G.OF + G.ff > (long long)(G.IF - 1) * G.sf + (long long)(G.KF - 1) * G.df + 1) return false;
    if ((long long)G.OT + G.ft > (long long)(G.IT - 1) * G.st + (long long)(G.KT - 1) * G.dt + 1) return false;
    invalid = false;
    if (G.KF > kCtMaxK || G.KT > kCtMaxK || G.sf > kCtMaxS || G.st > kCtMaxS || G.sf * G.st > kCtMaxPhases) return false;
    if (!ct_axis(g + 18, G.KF, G.sf, G.df, G.tap_f, G.start_f) || !ct_axis(g + 18 + G.KF, G.KT, G.st, G.dt, G.tap_t, G.start_t)) {
        invalid = true;
        return false;
    }
    G.phases = G.sf * G.st;
    G.QF0 = G.ff / G.sf, G.QT0 = G.ft / G.st;
    const int nqf = (G.OF - 1 + G.ff) / G.sf - G.QF0 + 1, nqt = (G.OT - 1 + G.ft) / G.st - G.QT0 + 1;
    G.TF = nqf == 1 ? 1 : 8, G.TT = nqf == 1 ? 128 : 16;
    const long long mf = (long long)(G.KF - 1) * G.df / G.sf, mt = (long long)(G.KT - 1) * G.dt / G.st;
    const long long hf = G.TF + mf, ht = G.TT + mt;
    if (hf * ht > 8192) return false;
    G.mf = (int)mf, G.mt = (int)mt, G.HF = (int)hf, G.HT = (int)ht;
    G.Cp = (G.Ci + 7) / 8 * 8;
    G.CC = G.Cp >= 32 ? 32 : (G.Cp >= 16 ? 16 : 8);
    while (G.CC > 8 && hf * ht * (4 * G.CC + 16) + kCtTapTable > kCtLdsLimit) G.CC /= 2;
    G.pitch = 4 * G.CC + 16;
    if (hf * ht * G.pitch + kCtTapTable > kCtLdsLimit) return false;
    G.NCH = (G.Cp + G.CC - 1) / G.CC;
    int base = 0;
    for (int rf = 0; rf < G.sf; ++rf)
        for (int rt = 0; rt < G.st; ++rt) {
            G.ks_base[rf * G.st + rt] = (unsigned short)base;
            const int taps = (G.start_f[rf + 1] - G.start_f[rf]) * (G.start_t[rt + 1] - G.start_t[rt]);
            base += (taps * (G.CC / 8) + 3) / 4;
        }
    G.ks_base[G.phases] = (unsigned short)base;
    G.KStot = base;
    G.tiles_f = (nqf + G.TF - 1) / G.TF, G.tiles_t = (nqt + G.TT - 1) / G.TT;
    G.tiles_n = (G.Co + 64 / G.NQ - 1) / (64 / G.NQ);
    return G.B * G.tiles_f * G.tiles_t * G.phases <= 0x7fffffffLL && G.tiles_n <= 65535;
}

template <int NQ>
__global__ __launch_bounds__(256) void je_conv_transpose_kernel(const CtGeom G, const CtArgs A) {
    extern __shared__ uint4 ct_lds[];
    int* tap_pos = reinterpret_cast<int*>(ct_lds);                      // [taps of the phase]: halo position of pixel (0, 0) under the tap
    unsigned char* lds = reinterpret_cast<unsigned char*>(ct_lds) + kCtTapTable;
    constexpr int SLOTS = 4 / NQ;                       // 16-channel tiles per output
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long tile = blockIdx.x;
    const int ph = (int)(tile % G.phases);              // the phases of one tile are neighbours: they share the halo in L2
    tile /= G.phases;
    const int tt = (int)(tile % G.tiles_t);
    tile /= G.tiles_t;
    const int tf = (int)(tile % G.tiles_f);
    const long long b = tile / G.tiles_f;
    const int rf = ph / G.st, rt = ph - rf * G.st;
    const int ef = G.start_f[rf], et = G.start_t[rt], nt = G.start_t[rt + 1] - et, taps = (G.start_f[rf + 1] - ef) * nt;
    const int KS = G.ks_base[ph + 1] - G.ks_base[ph];
    const int tile_n = blockIdx.y, co0 = tile_n * SLOTS * 16;
    const int qf0 = G.QF0 + tf * G.TF, qt0 = G.QT0 + tt * G.TT;
    const int if0 = qf0 - G.mf, it0 = qt0 - G.mt;
    const float sx = ct_scale(A.amax_x), inv = 1.f / (sx * ct_scale(A.amax_w));
    const int cgc = G.CC / 8, quads = G.CC / 4;
    bool live[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) live[j] = co0 + j * 16 < G.Co;
    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[i][s] = f4{0.f, 0.f, 0.f, 0.f};
    // this lane's two pixels on the tile: row tile wave * 2 + i is a row of 8 x 16, or 16 neighbours of 1 x 128
    int pix[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) pix[i] = G.TF == 1 ? (wave * 2 + i) * 16 + (lane & 15) : (wave * 2 + i) * G.HT + (lane & 15);

    for (int j = tid; j < taps; j += 256) {
        const int jf = j / nt, kf = G.tap_f[ef + jf], kt = G.tap_t[et + j - jf * nt];
        tap_pos[j] = (G.mf - (kf * G.df - rf) / G.sf) * G.HT + G.mt - (kt * G.dt - rt) / G.st;
    }
    for (int ch = 0; ch < G.NCH && KS > 0; ++ch) {
        __syncthreads();                                // everybody has read the chunk before
        for (int it = tid; it < G.HF * G.HT * quads; it += 256) {
            const int cq = it % quads, pos = it / quads, hf = pos / G.HT, ht = pos - hf * G.HT;
            const int c = ch * G.CC + cq * 4, f = if0 + hf, t = it0 + ht;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (c < G.Ci && f >= 0 && f < G.IF && t >= 0 && t < G.IT) {
                const float* p = A.x + ((b * G.IF + f) * G.IT + t) * G.ldx + c;
                if (A.vec_in) {
                    const float4 q = *reinterpret_cast<const float4*>(p);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < G.Ci) v[e] = p[e];
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
        const uint4* wp = A.W + (((long long)tile_n * G.NCH + ch) * G.KStot + G.ks_base[ph]) * 8 * 64 + lane;
        for (int ks = 0; ks < KS; ++ks, wp += 8 * 64) {
            const int kg = ks * 4 + (lane >> 4);
            int j = kg / cgc;
            const int cg = kg - j * cgc;
            if (j >= taps) j = taps - 1;                // a k group past the taps: its weights are zero, the read stays inside the halo
            const int at = tap_pos[j];
            h8 wh[4], wl[4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (live[s % SLOTS]) {
                    wh[s] = __builtin_bit_cast(h8, wp[(s * 2) * 64]);
                    wl[s] = __builtin_bit_cast(h8, wp[(s * 2 + 1) * 64]);
                }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned char* xp = lds + (long long)(at + pix[i]) * G.pitch + cg * 16;
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
        const int qf = qf0 + (G.TF == 1 ? 0 : wave * 2 + i), qt = qt0 + (G.TF == 1 ? (wave * 2 + i) * 16 : 0) + (lane & 15);
        const long long fo = (long long)qf * G.sf + rf - G.ff, to = (long long)qt * G.st + rt - G.ft;
        if (fo < 0 || fo >= G.OF || to < 0 || to >= G.OT) continue;    // trimmed away, or past the plane
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

// The weight planes in fragment order: row n = channel co of output q, value W_q[c, co, k_f, k_t].  One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void je_conv_transpose_pack_kernel(const float* __restrict__ w0, const float* __restrict__ w1,
                                                                     const unsigned* __restrict__ amax, uint4* __restrict__ out,
                                                                     const CtGeom G, const long long chunks) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const int lane = (int)(i & 63), plane = (int)((i >> 6) & 1), slot = (int)((i >> 7) & 3);
    long long rest = i >> 9;
    const int ksg = (int)(rest % G.KStot);
    rest /= G.KStot;
    const int ch = (int)(rest % G.NCH), tile_n = (int)(rest / G.NCH);
    int ph = 0;
    while (G.ks_base[ph + 1] <= ksg) ++ph;              // (ks_base[phases] = KStot > ksg ends it)
    const int rf = ph / G.st, rt = ph - rf * G.st, ef = G.start_f[rf], et = G.start_t[rt];
    const int nt = G.start_t[rt + 1] - et, taps = (G.start_f[rf + 1] - ef) * nt;
    const int slots = 4 / G.NQ, q = slot / slots, n = (tile_n * slots + slot % slots) * 16 + (lane & 15);
    const int cgc = G.CC / 8, kg = (ksg - G.ks_base[ph]) * 4 + (lane >> 4), j = kg / cgc, cg = kg - j * cgc;
    const float s = ct_scale(amax);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * G.CC + cg * 8 + e;
        float v = 0.f;
        if (j < taps && n < G.Co && c < G.Ci) {
            const int jf = j / nt, kf = G.tap_f[ef + jf], kt = G.tap_t[et + j - jf * nt];
            v = (q ? w1 : w0)[(((long long)c * G.Co + n) * G.KF + kf) * G.KT + kt];
        }
        v *= s;
        const _Float16 hi = (_Float16)v;
        o[e] = plane ? (_Float16)(v - (float)hi) : hi;
    }
    out[i] = __builtin_bit_cast(uint4, o);
}

static long long ct_pack_chunks(const CtGeom& G) { return (long long)G.tiles_n * G.NCH * G.KStot * 8 * 64; }

// ---------------------------------------------------------------------------------------------------------------- unpooling
struct CtPool {
    long long B, ldx;
    int IF, IT, OF, OT, C, kf, kt, sf, st, ff, ft, PF, TP;     // PF x TP: the plane MaxUnpool writes, on which the indices count
};

static bool ct_pool(const int64_t* g, int with_index, CtPool& P) {
    if (!g) return false;
    for (int i = 0; i < 13; ++i)
        if (g[i] < (i >= 11 ? 0 : 1) || g[i] > 0x3fffffff) return false;
    P.B = g[0], P.IF = (int)g[1], P.IT = (int)g[2], P.OF = (int)g[3], P.OT = (int)g[4], P.C = (int)g[5], P.kf = (int)g[6], P.kt = (int)g[7];
    P.sf = (int)g[8], P.st = (int)g[9], P.ldx = g[10], P.ff = (int)g[11], P.ft = (int)g[12];
    const long long pf = (long long)(P.IF - 1) * P.sf + P.kf, tp = (long long)(P.IT - 1) * P.st + P.kt;
    if (P.ldx < P.C || pf > 0x3fffffff || tp > 0x3fffffff) return false;
    P.PF = (int)pf, P.TP = (int)tp;
    if (with_index) return (long long)P.OF + P.ff <= pf && (long long)P.OT + P.ft <= tp;
    return (long long)P.IF * P.sf == P.OF && (long long)P.IT * P.st == P.OT;
}

// the windows wf lo .. hi that hold the padded position p
__device__ __forceinline__ void ct_windows(int p, int k, int s, int n, int& lo, int& hi) {
    lo = p - k + 1 <= 0 ? 0 : (p - k + s) / s;
    hi = p / s < n - 1 ? p / s : n - 1;
}

// one thread per output element y[b, fo, to, c]
template <bool INDEX>
__global__ __launch_bounds__(256) void je_unpool_forward_kernel(const float* __restrict__ x, const long long* __restrict__ index,
                                                                const CtPool P, float* __restrict__ y) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.B * P.OF * P.OT * P.C) return;
    const int c = (int)(i % P.C);
    const long long r = i / P.C;
    const int to = (int)(r % P.OT), fo = (int)((r / P.OT) % P.OF);
    const long long b = r / ((long long)P.OT * P.OF);
    float v = 0.f;
    if constexpr (INDEX) {
        const int pf = fo + P.ff, pt = to + P.ft;
        const long long me = (long long)pf * P.TP + pt;
        int flo, fhi, tlo, thi;
        ct_windows(pf, P.kf, P.sf, P.IF, flo, fhi);
        ct_windows(pt, P.kt, P.st, P.IT, tlo, thi);
        for (int wf = flo; wf <= fhi; ++wf)
            for (int wt = tlo; wt <= thi; ++wt) {
                const long long w = (b * P.IF + wf) * P.IT + wt;
                if (index[w * P.C + c] == me) v = x[w * P.ldx + c];     // the later window wins (torch's CPU loop)
            }
    } else {
        v = x[((b * P.IF + fo / P.sf) * P.IT + to / P.st) * P.ldx + c];
    }
    y[i] = v;
}

// one thread per input element dx[b, wf, wt, c], every element written
template <bool INDEX>
__global__ __launch_bounds__(256) void je_unpool_backward_kernel(const float* __restrict__ dy, const long long* __restrict__ index,
                                                                 const CtPool P, float* __restrict__ dx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.B * P.IF * P.IT * P.C) return;
    const int c = (int)(i % P.C);
    const long long r = i / P.C;
    const int wt = (int)(r % P.IT), wf = (int)((r / P.IT) % P.IF);
    const long long b = r / ((long long)P.IT * P.IF);
    float v = 0.f;
    if constexpr (INDEX) {
        const long long me = index[i];
        const long long pf = me / P.TP, pt = me - pf * P.TP, fo = pf - P.ff, to = pt - P.ft;
        // the position lies in this window (what the forward gather looks at) and inside the trimmed output
        bool mine = me >= 0 && pf >= (long long)wf * P.sf && pf < (long long)wf * P.sf + P.kf && pt >= (long long)wt * P.st &&
                    pt < (long long)wt * P.st + P.kt && fo >= 0 && fo < P.OF && to >= 0 && to < P.OT;
        if (mine) {
            int flo, fhi, tlo, thi;
            ct_windows((int)pf, P.kf, P.sf, P.IF, flo, fhi);
            ct_windows((int)pt, P.kt, P.st, P.IT, tlo, thi);
            for (int f2 = wf; f2 <= fhi; ++f2)          // a later window with the same index took the position
                for (int t2 = tlo; t2 <= thi; ++t2)
                    if ((f2 > wf || t2 > wt) && index[((b * P.IF + f2) * P.IT + t2) * P.C + c] == me) mine = false;
        }
        if (mine) v = dy[((b * P.OF + fo) * P.OT + to) * P.C + c];
    } else {
        for (int a = 0; a < P.sf; ++a)
            for (int w = 0; w < P.st; ++w) v += dy[((b * P.OF + wf * P.sf + a) * P.OT + wt * P.st + w) * P.C + c];
    }
    dx[i] = v;
}

}  // namespace ptmi

using namespace ptmi;

extern "C" {

int64_t ptmi_je_conv_transpose_pack_elems(const int64_t* geom) {
    CtGeom G;
    bool invalid;
    return ct_geom(geom, G, invalid) ? ct_pack_chunks(G) * 8 : (invalid ? -1 : -2);
}

int64_t ptmi_je_conv_transpose_ksteps(const int64_t* geom) {
    CtGeom G;
    bool invalid;
    return ct_geom(geom, G, invalid) ? (int64_t)G.KStot * G.NCH : (invalid ? -1 : -2);
}

int ptmi_je_conv_transpose_pack(const float* w0, const float* w1, const uint32_t* amax, uint16_t* planes, const int64_t* geom,
                                ptmi_stream_t stream) {
    CtGeom G;
    bool invalid;
    PTMI_RETURN_IF(!w0 || !amax || !planes, PTMI_E_INVALID);
    if (!ct_geom(geom, G, invalid)) return invalid ? PTMI_E_INVALID : PTMI_E_UNSUPPORTED;
    PTMI_RETURN_IF(!w1 && G.NQ == 2, PTMI_E_INVALID);
    const long long chunks = ct_pack_chunks(G);
    if (chunks == 0) return PTMI_OK;                    // no phase has a tap: the planes are empty
    PTMI_RETURN_IF((chunks + 255) / 256 > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipLaunchKernelGGL(je_conv_transpose_pack_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       w0, w1, amax, reinterpret_cast<uint4*>(planes), G, chunks);
    return launch_status();
}

int ptmi_je_conv_transpose_forward(const float* x, const uint16_t* planes, const uint32_t* amax_x, const uint32_t* amax_w, const float* bias,
                                   const float* gate_bias, const float* residual, const float* slope, float* z, float* gz, float* out,
                                   const int64_t* geom, int32_t act, float act_p, ptmi_stream_t stream) {
    CtGeom G;
    bool invalid;
    PTMI_RETURN_IF(!x || !amax_x || !amax_w || !z || !geom, PTMI_E_INVALID);
    if (!ct_geom(geom, G, invalid)) return invalid ? PTMI_E_INVALID : PTMI_E_UNSUPPORTED;
    PTMI_RETURN_IF((!planes && G.KStot > 0) || (G.NQ == 2 && !gz) || act < kActIdentity || act > kActPrelu, PTMI_E_INVALID);
    PTMI_RETURN_IF(act == kActPrelu && out && !slope, PTMI_E_INVALID);
    CtArgs A;
    A.x = x, A.W = reinterpret_cast<const uint4*>(planes), A.amax_x = amax_x, A.amax_w = amax_w;
    A.bias[0] = bias, A.bias[1] = gate_bias, A.residual = residual, A.slope = slope, A.z[0] = z, A.z[1] = gz, A.out = out;
    A.act = act, A.act_p = act_p;
    A.vec_in = G.Ci % 4 == 0 && G.ldx % 4 == 0 && aligned16({x});
    A.vec_out = G.Co % 4 == 0 && aligned16({z, gz, out});
    const dim3 grid((unsigned)(G.B * G.tiles_f * G.tiles_t * G.phases), (unsigned)G.tiles_n);
    const size_t lds = (size_t)G.HF * G.HT * G.pitch + kCtTapTable;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (G.NQ == 2)
        hipLaunchKernelGGL((je_conv_transpose_kernel<2>), grid, dim3(256), lds, st, G, A);
    else
        hipLaunchKernelGGL((je_conv_transpose_kernel<1>), grid, dim3(256), lds, st, G, A);
    return launch_status();
}

int ptmi_je_unpool_forward(const float* x, const int64_t* index, float* y, const int64_t* geom, ptmi_stream_t stream) {
    CtPool P;
    PTMI_RETURN_IF(!x || !y || !ct_pool(geom, index != nullptr, P), PTMI_E_INVALID);
    const long long blocks = (P.B * P.OF * P.OT * P.C + 255) / 256;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* ip = reinterpret_cast<const long long*>(index);
    if (index)
        hipLaunchKernelGGL((je_unpool_forward_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, x, ip, P, y);
    else
        hipLaunchKernelGGL((je_unpool_forward_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, x, ip, P, y);
    return launch_status();
}

int ptmi_je_unpool_backward(const float* dy, const int64_t* index, float* dx, const int64_t* geom, ptmi_stream_t stream) {
    CtPool P;
    PTMI_RETURN_IF(!dy || !dx || !ct_pool(geom, index != nullptr, P), PTMI_E_INVALID);
    const long long blocks = (P.B * P.IF * P.IT * P.C + 255) / 256;
    PTMI_RETURN_IF(blocks > 0x7fffffffLL, PTMI_E_UNSUPPORTED);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long* ip = reinterpret_cast<const long long*>(index);
    if (index)
        hipLaunchKernelGGL((je_unpool_backward_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, dy, ip, P, dx);
    else
        hipLaunchKernelGGL((je_unpool_backward_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, dy, ip, P, dx);
    return launch_status();
}

}  // extern "C"
