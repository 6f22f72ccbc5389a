/*
 * ptmi.h - C ABI of libptmi.so: the MI355X (gfx950) kernels behind the padertorch PIT hot path.
 *
 * Plain pointers and sizes only (no torch types).  Every pointer marked "device" is a HIP device
 * pointer owned by the caller; kernels are enqueued on `stream` (a hipStream_t passed as void*)
 * and borrow the buffers until that work has run.  Every entry point returns 0 on success, a
 * negative PTMI_E_* code for argument errors, or a positive hipError_t from the launch.
 *
 * Each function cites the reference interface (file:line below /root/reference) it replaces.
 */
#ifndef PTMI_H_
#define PTMI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_OK 0
#define PTMI_E_INVALID (-1)     /* bad argument (null pointer, odd size, ...)            */
#define PTMI_E_UNSUPPORTED (-2) /* configuration the kernels do not cover                 */

typedef void* ptmi_stream_t; /* hipStream_t */

const char* ptmi_version(void);
const char* ptmi_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * STFT geometry: the framing of padertorch/ops/_stft.py:131-158 (STFT.__call__).
 *   pad_left / pad_right : fading zeros (L-shift each for 'full'; (L-shift)//2, ceil((L-shift)/2)
 *                          for 'half'; 0 for None/False)                       (_stft.py:137-146)
 *   pad                  : 1 = right-pad to a whole frame (ceil), 0 = cut (floor) (_stft.py:148-154)
 * ------------------------------------------------------------------------------------------- */
typedef struct ptmi_stft_geom {
    int32_t size;          /* FFT size (even)                                   */
    int32_t shift;         /* hop                                               */
    int32_t window_length; /* L <= size                                         */
    int32_t pad_left;
    int32_t pad_right;
    int32_t pad;
} ptmi_stft_geom;

/* Frame / sample bookkeeping (integer, bit-exact).
 * Replaces STFT.samples_to_frames / frames_to_samples (_stft.py:265-307 -> paderbox
 * _samples_to_stft_frames / _stft_frames_to_samples) and the conv1d output length of _stft.py:158. */
int64_t ptmi_stft_num_frames(const ptmi_stft_geom* g, int64_t num_samples);
int64_t ptmi_istft_num_samples(const ptmi_stft_geom* g, int64_t num_frames);

/* Output layouts of ptmi_stft_forward / input layouts of ptmi_istft_forward (_stft.py:162-174). */
#define PTMI_LAYOUT_INTERLEAVED 0 /* [..., frames, F, 2] == complex64 == 'stacked' */
#define PTMI_LAYOUT_CONCAT 1      /* [..., frames, 2F]  (re | im)                  */

/* Forward STFT: framing + window + real FFT in one kernel.
 * Replaces STFT.__call__ (_stft.py:103-174: F.pad, F.pad, kernel.to(x), F.conv1d, rearrange, chunk).
 *   x            device [batch, x_row_stride] float32, row b valid for row_samples[b] (or num_samples)
 *   row_samples  device int32[batch] or NULL (all rows num_samples long)
 *   window       device float32[window_length]
 *   twiddle      device float32[(size/2+1)*2]: (cos, -sin)(2*pi*j/size), j = 0..size/2
 *   out          device float32 [batch, out_frames, F, 2] or [batch, out_frames, 2F]; rows past a
 *                row's own frame count are zero-filled
 *   edge_scale   1.0 for the plain transform; 0.5 when used as the adjoint of ptmi_istft_forward
 *                (scales the DC/Nyquist bins and zeroes their imaginary part)
 */
int ptmi_stft_forward(const float* x, int64_t batch, int64_t x_row_stride, int64_t num_samples,
                      const int32_t* row_samples, const float* window, const float* twiddle,
                      const ptmi_stft_geom* g, int64_t out_frames, int32_t layout, float edge_scale,
                      float* out, ptmi_stream_t stream);

/* Inverse STFT: hermitian inverse real FFT + synthesis window + overlap-add + fading cut.
 * Replaces STFT.inverse (_stft.py:176-263: two conv_transpose1d over the hermitian-extended
 * spectrum, sum, cut).
 *   spec         device float32, layout as above, [batch, num_frames, ...]
 *   row_frames   device int32[batch] or NULL (all rows num_frames)
 *   syn_window   device float32[window_length]: biorthogonal window / size   (_stft.py:27-28)
 *   out          device float32 [batch, out_row_stride]; out_samples per row are written
 *   cut_left     samples dropped in front (int(pad_width), _stft.py:257-262)
 *   edge_scale   1.0 for the plain inverse; 2.0 when used as the adjoint of ptmi_stft_forward
 */
int ptmi_istft_forward(const float* spec, int64_t batch, int64_t num_frames, const int32_t* row_frames,
                       const float* syn_window, const float* twiddle, const ptmi_stft_geom* g,
                       int32_t layout, float edge_scale, int64_t cut_left, int64_t out_samples,
                       int64_t out_row_stride, float* out, ptmi_stream_t stream);

/* Fused PIT feature front-end: STFT of the mixture and of K sources + |.| + cos(phase difference).
 * Replaces pre_batch_transform (padertorch/contrib/examples/source_separation/pit/data.py:49-77).
 *   y            device [batch, row_stride]           mixture waveforms
 *   s            device [batch, K, row_stride]        source waveforms (may be NULL: only Y_abs)
 *   row_samples  device int32[batch] or NULL
 *   Y_abs        device [batch, out_frames, F]
 *   X_abs, cos_pd device [batch, out_frames, K, F]    (NULL when s is NULL)
 * Any even g->size (paderbox.stft takes any): powers of two in 64..2048 run the FFT kernels, every other size the direct-DFT kernel.
 */
int ptmi_pit_features(const float* y, const float* s, int64_t batch, int32_t K, int64_t row_stride,
                      int64_t num_samples, const int32_t* row_samples, const float* window,
                      const float* twiddle, const ptmi_stft_geom* g, int64_t out_frames, float* Y_abs,
                      float* X_abs, float* cos_pd, ptmi_stream_t stream);
/* The same launch, also writing the model's first-layer input (pit/model.py:91-94: pack_sequence(Y_abs) -> log1p):
 *   log1p_packed    device [rows, F] fp32, rows = sum of the examples' frame counts: log1p(Y_abs) as PackedSequence data, the row
 *                   of frame t of example b = packed_offsets[t] + b (examples sorted by descending length), or t * batch + b
 *                   when packed_offsets is NULL (all examples have out_frames frames)
 *   log1p_planes    NULL, or the same matrix as fp16 (hi, lo) planes of 2^9 log1p(Y_abs) in the layout of ptmi_pack_planes_n
 *                   (ptmi_planes_elems(rows, F) values, 16-byte aligned, ZEROED by the caller: padding is not written): operand A
 *                   of the first input projection on ptmi_gemm_planes with an operand-scale word of 16.0f (scale 2^13 / 16).
 *                   The fixed scale holds for every finite input: log1p(FLT_MAX) 2^9 < 65504. */
int ptmi_pit_features_packed(const float* y, const float* s, int64_t batch, int32_t K, int64_t row_stride,
                             int64_t num_samples, const int32_t* row_samples, const float* window,
                             const float* twiddle, const ptmi_stft_geom* g, int64_t out_frames, float* Y_abs,
                             float* X_abs, float* cos_pd, float* log1p_packed, uint16_t* log1p_planes,
                             const int64_t* packed_offsets, ptmi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Permutation-invariant training loss.
 * Replaces pit_loss (padertorch/ops/losses/source_separation.py:34-124) with loss_fn = mse_loss
 * and the review loop of pit/model.py:117-140.
 * ------------------------------------------------------------------------------------------- */

/* Pairwise sums of squared errors for `batch` ragged examples stored in padded buffers.
 *   est      device, element (b, t, i, f) at b*strides[0] + t*strides[1] + i*F + f: estimates
 *            (or masks when obs != NULL: est = mask * obs); batch- or time-major padded storage
 *   obs      device or NULL, element (b, t, f) at b*strides[2] + t*strides[3] + f
 *   tgt      device, element (b, t, j, f) at b*strides[4] + t*strides[5] + j*F + f
 *   tgt_scale device like tgt or NULL; second target = tgt * tgt_scale (cos phase difference)
 *   strides  HOST int64[6] (element strides, see above)
 *   row_frames device int32[batch] or NULL (all t_len)
 *   sse      device float64 [batch, nvar, K, K]: sse[b, v, i, j] = sum_{t,f} (est_i - tgt^v_j)^2
 *            nvar = 1 (tgt) or 2 (tgt, tgt*tgt_scale)
 *   workspace device float64 [ptmi_pit_workspace_elems(...)]
 */
int64_t ptmi_pit_workspace_elems(int64_t batch, int64_t t_len, int32_t K, int32_t F);
int ptmi_pit_pairwise_sse(const float* est, const float* obs, const float* tgt, const float* tgt_scale,
                          int64_t batch, int64_t t_len, const int64_t* strides, int32_t K, int32_t F,
                          const int32_t* row_frames, double* workspace, double* sse,
                          ptmi_stream_t stream);

/* Permutation search on the pairwise matrix + batch mean (first minimum wins, torch.min).
 *   loss     device float32 [nvar]         mean_b min_perm (1/(T_b K F)) sum_j sse[b,v,perm[j],j]
 *   perm     device int32 [batch, nvar, K] estimate index per target (pit_loss's convention)
 *   ex_loss  device float32 [batch, nvar]  per-example losses (may be NULL)
 */
int ptmi_pit_assign(const double* sse, int64_t batch, int32_t nvar, int32_t K, int32_t F,
                    int64_t t_len, const int32_t* row_frames, float* loss, int32_t* perm,
                    float* ex_loss, ptmi_stream_t stream);

/* Gradient wrt est (or wrt the mask when obs != NULL):
 *   grad[b,t,i,f] = sum_v gscale[v] * 2/(B T_b K F) * (est_i - tgt^v_{j: perm[b,v,j]=i}) [* obs]
 *   gscale   device float32 [nvar] (upstream gradients of the two batch-mean losses)
 *   grad     device, same addressing as est (strides[0], strides[1]); frames t >= T_b get 0
 */
int ptmi_pit_backward(const float* est, const float* obs, const float* tgt, const float* tgt_scale,
                      const int32_t* perm, const float* gscale, int64_t batch, int64_t t_len,
                      const int64_t* strides, int32_t K, int32_t F, int32_t nvar, const int32_t* row_frames,
                      float* grad, ptmi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Deep-clustering loss.  Replaces deep_clustering_loss (padertorch/ops/losses/source_separation.py:
 * 13-31) and the per-example review loop + re-layout of contrib/tcl/dc.py:73-84.
 *   x  embeddings, element (b, t, e, f) at b*strides[0] + t*strides[1] + e*strides[2] + f*strides[3]
 *   t  targets,    element (b, t, k, f) at b*strides[4] + t*strides[5] + k*strides[6] + f*strides[7]
 *      rows of example b: n = (t, f), t < T_b (row_frames[b] or T), f < F;  N_b = T_b * F
 *      (plain (N, E) / (N, K) matrices: T = N, F = 1, strides = {0, E, 1, 0, 0, K, 1, 0})
 *   strides HOST int64[8];  E + K <= 32
 *   gram    device float64 [batch, 32, 32]: V'V with V = [x | t] (zero padded)
 *   ex_loss device float32 [batch]: (|X'X|^2 - 2|X'T|^2 + |T'T|^2) / N_b^2;  loss [1]: batch mean
 *   workspace device float32 [ptmi_dc_workspace_elems(batch, T, F)]
 * ------------------------------------------------------------------------------------------- */
int64_t ptmi_dc_workspace_elems(int64_t batch, int64_t T, int32_t F);
int ptmi_dc_loss_forward(const float* x, const float* t, int64_t batch, int64_t T, const int64_t* strides,
                         int32_t E, int32_t K, int32_t F, const int32_t* row_frames, float* workspace,
                         double* gram, float* ex_loss, float* loss, ptmi_stream_t stream);
/* dx = gscale[0] / batch * 4 / N_b^2 * (x (X'X) - t (T'X)), same addressing as x. */
int ptmi_dc_loss_backward(const float* x, const float* t, const double* gram, const float* gscale,
                          int64_t batch, int64_t T, const int64_t* strides, int32_t E, int32_t K, int32_t F,
                          const int32_t* row_frames, float* dx, ptmi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Packed-sequence (B)LSTM recurrence (time loop of torch.nn.LSTM on a PackedSequence:
 * pit/model.py:60-66,97, contrib/tcl/dc.py:32-34,61; gate order i,f,g,o; zero initial state).
 * rows = packed time-major rows, row(t, b) = offsets[t] + b, b < batch_sizes[t] (descending).
 * One launch per timestep covers both directions (direction 1 walks time backwards).
 * ------------------------------------------------------------------------------------------- */

/* Forward through time.
 *   gates      device [rows, ndir, 4, H]  in: x W_ih^T + b_ih + b_hh; out: activated i,f,g,o (in place)
 *   hy, c      device [rows, ndir, H]     out: hidden / cell state of every step
 *   c0         device [ndir, max_batch, H] initial cell state of every sequence, or NULL (zero).  The
 *              initial HIDDEN state enters through `gates`: the caller adds h0 W_hh^T to the rows of
 *              each sequence's first processed step (torch.nn.LSTM(x, (h0, c0)) semantics).
 *   w_hh_pad   device [ndir, 4H, KP]      recurrent weights, K zero-padded to KP = roundup(H, 16)
 *   batch_sizes HOST int32 [T], offsets HOST int64 [T] (PackedSequence bookkeeping; per-step row
 *              ranges travel as kernel arguments)
 *   H % 4 == 0 is required (16-byte aligned operand rows), else PTMI_E_UNSUPPORTED.
 */
int ptmi_lstm_forward(float* gates, float* hy, float* c, const float* c0, const float* w_hh_pad, const int32_t* batch_sizes,
                      const int64_t* offsets, int32_t T, int32_t max_batch, int32_t H, int32_t KP,
                      int32_t ndir, ptmi_stream_t stream);

/* Backward through time.
 *   gates, c   saved by ptmi_lstm_forward;  dhy device [rows, ndir, H] gradient wrt hy
 *   w_hh_t     device [ndir, H, 4H]  (transposed recurrent weights)
 *   dgates     device [rows, ndir, 4, H]  out: gradient wrt the gate pre-activations
 *   dc_state   device [max_batch, ndir, H] scratch (need not be initialised)
 * dW_ih, dW_hh, db and dx follow from dgates by dense GEMMs on the caller's side.
 */
int ptmi_lstm_backward(const float* gates, const float* c, const float* c0, const float* dhy, const float* w_hh_t, float* dgates,
                       float* dc_state, const int32_t* batch_sizes, const int64_t* offsets, int32_t T,
                       int32_t max_batch, int32_t H, int32_t ndir, ptmi_stream_t stream);

/* ---- Persistent recurrence: ONE launch per layer and pass (host side csrc/lstm.hip, kernels csrc/lstm_split.hip) ----
 * A workgroup's slice of W_hh stays in registers for all T steps.  The per-step product is evaluated as three 16-bit MFMA
 * products of (hi, lo) operand halves with fp32 accumulation (fp32-equivalent result): forward fp16 halves of 2^10 h and of the
 * scaled weights (w_hh_amax = device word from ptmi_absmax over w_hh_pad; NULL: |W_hh| within fp16's range as it is), backward
 * bf16 halves (no scale).  The steps are chained through 16-bit hand-off planes at the START of the scratch, synchronised by
 * their data (data-as-flag): every 16-bit value of the planes starts out as 0xFFFF - a pattern no conversion to fp16 / bf16
 * produces -, producers only store, consumers re-request an operand tile until none of the values they are going to use is the
 * pattern.  Every poll is bounded.  Same results as ptmi_lstm_forward / ptmi_lstm_backward.  With PTMI_LSTM_F32 in the
 * environment (ptmi_lstm_split_enabled() == 0) the persistent entries refuse every configuration, and the callers run the
 * exact-fp32 step-per-launch kernels above.
 *
 * batch_sizes_dev / offsets_dev are DEVICE copies here.  `flags` is the launch's device scratch of
 * ptmi_lstm_scratch_elems(T, ndir, max_batch, H, backward) uint32:
 *   forward    [ hand-off planes of hy | ptmi_lstm_flags_elems(T, ndir, max_batch) words ]
 *   backward   [ hand-off planes of dgates | BIAS GRADIENT [ndir][4H] floats (sum of dgates over all rows, out) | 8 words, word 0:
 *                float bits of max |dgates| (out) | ptmi_lstm_flags_elems(T, ndir, max_batch) words ]
 * The LAST 8 words are the error words in both (non-zero after the call = a bounded poll ran out; ptmi_lstm_set_error_sink
 * counts such launches per device).  The words in front of them are reserved and zeroed (the slots of the former flag protocol). */
int64_t ptmi_lstm_flags_elems(int32_t T, int32_t ndir, int32_t max_batch);
int64_t ptmi_lstm_scratch_elems(int32_t T, int32_t ndir, int32_t max_batch, int32_t H, int32_t backward);
/* ptmi_lstm_weight_prep (csrc/lstm_prep.hip): the operand forms of ONE (bi)directional LSTM layer's parameters
 * (torch.nn.LSTM layout, padertorch/contrib/examples/source_separation/pit/model.py:60-66) in one launch:
 *   w_ih / w_hh / b_ih / b_hh  HOST arrays of ndir device pointers: [4H, I], [4H, H], [4H], [4H] per direction
 *   w_ih_cat [ndir * 4H, Ipad]  stacked input weights, columns I .. Ipad-1 zero (Ipad >= I, e.g. I rounded up to 4)
 *   bias     [ndir * 4H]        b_ih + b_hh
 *   w_pad    [ndir, 4H, KP]     recurrent weights, columns H .. KP-1 zero (what ptmi_lstm_forward* take as w_hh_pad)
 *   w_t      [ndir, H, 4H]      transposed recurrent weights (what ptmi_lstm_backward* take)
 *   amax     [2] uint32         float bits of max |w_ih|, max |w_hh| over both directions (the words ptmi_gemm_split /
 *                               ptmi_lstm_forward_persistent take as operand scales) */
int ptmi_lstm_weight_prep(const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                          const float* const* b_hh, int32_t ndir, int32_t H, int32_t I, float* w_ih_cat, int32_t Ipad,
                          float* bias, float* w_pad, int32_t KP, float* w_t, uint32_t* amax, ptmi_stream_t stream);
/* ptmi_lstm_set_error_sink: `word` (device uint32, zeroed by the caller, alive as long as launches may run; NULL to
 * unset) of the CURRENT device is incremented by every persistent launch whose bounded spin runs out (next to that
 * launch's own error word in its scratch): ONE word for the host to watch instead of one per call. */
int ptmi_lstm_set_error_sink(uint32_t* word);
int ptmi_lstm_split_enabled(void);
/* Queries: what the persistent launches of a configuration do (CU count of the current device).
 * ptmi_lstm_handoff_cols: columns per direction (H resp. 4H rounded up to 32) of the hand-off planes - forward (backward = 0):
 *   fp16 (hi, lo) halves of 2^10 h, backward: bf16 halves of dgates -, laid out as [T][16-row tile][direction][cols / 32][hi | lo]
 *   [64 chunks of 8 values] in the fragment order of ptmi_gemm_planes: for a batch of equal-length sequences whose size is a multiple of
 *   16 this IS the A operand (rows = packed rows, k = direction-major columns) of the dense GEMM that follows.  0: no persistent
 *   kernel for this H (PTMI_LSTM_F32, or a layer too wide for the kernels' register budget).
 * ptmi_lstm_backward_planes_ok: != 0 when the backward launch can emit dgates^T planes (dgates_t below): a configuration it runs
 *   at all, equal-length sequences (rows == T * max_batch), max_batch a multiple of 16.
 * ptmi_lstm_forward_fills: the value to pass as `prefilled` to the backward call of a layer whose forward call got that backward
 *   call's scratch as `backward_scratch` - 2: the forward launch writes the pattern into the backward planes and zeros into the
 *   words behind them (an otherwise idle wavefront of every workgroup, a slice per time step, i.e. for free), the backward call
 *   enqueues nothing in front of its recurrence kernel; 0: it does not, `backward_scratch` is ignored. */
int32_t ptmi_lstm_handoff_cols(int32_t H, int32_t backward);
int32_t ptmi_lstm_backward_planes_ok(int32_t T, int32_t ndir, int32_t max_batch, int64_t rows, int32_t H);
int ptmi_lstm_forward_fills(int32_t T, int32_t ndir, int32_t max_batch, int32_t H);

/* Persistent forward recurrence.  Arguments as ptmi_lstm_forward, and
 *   step_masks        NULL, or a ROW-SLOT batch: several sequences lie END TO END in one row slot, so that every one of the (at most
 *                     64) slots works in (nearly) every time step - a recurrence costs its number of steps, whatever the number of rows
 *                     up to 32 (64) per step, so a ragged batch packed this way takes total frames / slots steps instead of the longest
 *                     sequence's.  Layout: uniform, row(t, slot) = t * max_batch + slot, every such row exists in all buffers;
 *                     step_masks [T][3] uint64 (device): rows alive at time index t, rows whose sequence STARTS at t, rows whose
 *                     sequence ENDS at t (bit b = slot b).  A sequence start resets (h, c) to zero in the forward direction, a
 *                     sequence end in the reverse direction; idle rows are neither computed nor handed on (hy / c of idle rows are
 *                     not written: hand in zeroed buffers; their gate gradients come out as zeros, and their rows of the hand-off
 *                     planes as zeros too, so that for max_batch % 16 == 0 the planes are the GEMM operands they are for
 *                     equal-length batches).  Same results per sequence as one sequence per row (torch.nn.LSTM on a
 *                     PackedSequence, pit/model.py:60-66,97).
 *   prefilled         != 0: the caller has filled the planes with the pattern (32-bit words 0xFFFFFFFF) on a stream ordered before
 *                     this one; the call then only zeroes the words behind them
 *   backward_scratch  NULL, or the scratch of this layer's backward call (ptmi_lstm_forward_fills)
 * Refused, with NOTHING enqueued:
 *   PTMI_E_INVALID      gates, hy, c, w_hh_pad, batch_sizes_dev, offsets_dev or flags NULL; T, max_batch, H or rows < 1; ndir not 1 or 2
 *   PTMI_E_UNSUPPORTED  step_masks with c0, with rows != T * max_batch or with max_batch > 64; H % 4 != 0; KP != H rounded up to 16;
 *                       a configuration the kernels cannot keep resident (the caller falls back to ptmi_lstm_forward);
 *                       rows * ndir * H * 4 bytes >= 2^31 */
int ptmi_lstm_forward_persistent(float* gates, float* hy, float* c, const float* c0, const float* w_hh_pad,
                                 const uint32_t* w_hh_amax, const int32_t* batch_sizes_dev, const int64_t* offsets_dev,
                                 const uint64_t* step_masks, uint32_t* flags, int32_t T, int32_t max_batch, int64_t rows,
                                 int32_t H, int32_t KP, int32_t ndir, int32_t prefilled, uint32_t* backward_scratch,
                                 ptmi_stream_t stream);

/* Persistent backward-through-time.  Arguments as ptmi_lstm_backward (no dc_state scratch: the cell-state gradient stays in
 * registers), step_masks as above, and
 *   s_begin, s_end    the launch processes the steps [s_begin, s_end) of the T processing steps (step s handles time index T-1-s in
 *                     direction 0, s in direction 1); [0, T) is the whole recurrence.  Ranges must be launched in order on one stream
 *                     with the same scratch; the first (s_begin == 0) sets the scratch up.  After the range [0, s) the gate gradients
 *                     of direction 0 are complete for time indices >= T - s and of direction 1 for time indices < s: their
 *                     weight-gradient GEMMs can run under the next range.
 *   dc_carry          NULL, or device fp32 [ndir, max_batch, H]: takes the cell-state gradient across a cut between ranges; after
 *                     the last range it is the gradient w.r.t. the initial cell state c0
 *   dc_n              NULL, or device fp32 [ndir, max_batch, H]: gradient w.r.t. the FINAL cell state, added to the cell-state
 *                     gradient at every sequence's last step (torch.nn.LSTM returns (h_n, c_n) with their graph,
 *                     padertorch/modules/recurrent.py:42 carries them; the final / initial HIDDEN states' gradients travel through
 *                     dhy resp. dgates W_hh on the caller's side)
 *   dgates_t          NULL, or ndir * ptmi_planes_elems(4H, range_rows) uint16, range_rows = (s_end - s_begin) * max_batch: the gate
 *                     gradients of THIS launch's step range - for the forward direction the time indices T - s_end .. T - s_begin - 1,
 *                     for the reverse direction s_begin .. s_end - 1 - as the operand of the weight-gradient GEMMs dW_ih = dgates^T x,
 *                     dW_hh = dgates^T h_prev (torch.nn.LSTM backward inside pit/model.py:60-66,97): bf16 (hi, lo) planes of dgates^T
 *                     per direction, [ndir][4H / 16 column tiles][ceil(range_rows / 32) k blocks][hi | lo][64 chunks of 8 values] =
 *                     exactly what ptmi_pack_planes_t_bf16 makes of one direction's [rows, 4H] block, i.e. operand A of
 *                     ptmi_gemm_planes_bf16(m = 4H, k = rows) at byte offset direction * ptmi_planes_elems(4H, rows) * 2.  The call
 *                     writes every value.  No transposing pack pass.
 *   dgates            may be NULL when dgates_t is given (the hand-off copy in `flags` still serves dx = dgates W_ih): no row-major
 *                     fp32 store then
 *   prefilled         0: the call sets its scratch up itself (one launch in front of the recurrence); 1: the caller has filled the
 *                     planes with the pattern, the call zeroes the words behind them; 2: those are zero as well
 *                     (ptmi_lstm_forward_fills), the call enqueues its recurrence only.  Read by the first range.
 * Refused, with NOTHING enqueued (a "partial range" is any [s_begin, s_end) other than [0, T)):
 *   PTMI_E_INVALID      gates, c, dhy, w_hh_t, batch_sizes_dev, offsets_dev or flags NULL; T, max_batch, H or rows < 1; ndir not 1 or 2
 *   PTMI_E_INVALID      dgates and dgates_t both NULL
 *   PTMI_E_INVALID      dgates_t not 16-byte aligned
 *   PTMI_E_INVALID      s_begin < 0, s_end > T or s_begin >= s_end
 *   PTMI_E_INVALID      a partial range without dc_carry
 *   PTMI_E_INVALID      dc_n with a partial range
 *   PTMI_E_UNSUPPORTED  dc_n with step_masks
 *   PTMI_E_UNSUPPORTED  step_masks with c0, with rows != T * max_batch, with max_batch > 64 or with a partial range
 *   PTMI_E_UNSUPPORTED  dgates_t where ptmi_lstm_backward_planes_ok(...) == 0
 *   PTMI_E_UNSUPPORTED  H % 4 != 0; a configuration the kernels cannot keep resident (the caller falls back to
 *                       ptmi_lstm_backward); rows * ndir * 4H * 4 bytes >= 2^31 */
int ptmi_lstm_backward_persistent(const float* gates, const float* c, const float* c0, const float* dhy, const float* dc_n,
                                  const float* w_hh_t, float* dgates, uint16_t* dgates_t, const int32_t* batch_sizes_dev,
                                  const int64_t* offsets_dev, const uint64_t* step_masks, uint32_t* flags, float* dc_carry,
                                  int32_t T, int32_t max_batch, int64_t rows, int32_t H, int32_t ndir, int32_t s_begin,
                                  int32_t s_end, int32_t prefilled, ptmi_stream_t stream);

/* ---- (log-)mel features ----------------------------------------------------------------------------
 * Replaces MelTransform.forward (padertorch/contrib/je/modules/features.py:297-330: spectrogram @
 * fbanks, log(x + eps)) and, fused with the STFT, the extractor front-end features.py:171-176
 * (power of the stacked STFT -> MelTransform) without materialising the spectrum.
 * The [F, M] filterbank is passed band-compressed in 16-byte aligned groups of 8 bins: filter m covers
 * bins 4 mel_lo[m] .. 4 mel_lo[m] + 8 mel_cnt[m] - 1 with the (zero-padded) weights
 * mel_w[4 mel_off[m] ...] (device arrays; mel_nnz = number of floats in mel_w, a multiple of 8).
 * ptmi_stft_logmel: x [batch, num_samples] -> out [batch, out_frames, mel_M] = f(|STFT|^power),
 * power in {1, 2}; sizes 64..2048 (powers of two).  ptmi_mel_apply: spec [N, F] -> out [N, mel_M]. */
int ptmi_stft_logmel(const float* x, int64_t batch, int64_t x_row_stride, int64_t num_samples,
                     const int32_t* row_samples, const float* window, const float* twiddle,
                     const ptmi_stft_geom* g, int64_t out_frames, const int32_t* mel_lo, const int32_t* mel_cnt,
                     const int32_t* mel_off, const float* mel_w, int32_t mel_M, int32_t mel_nnz, int32_t power,
                     int32_t log_, float eps, float* out, ptmi_stream_t stream);
int ptmi_mel_apply(const float* spec, int64_t N, int32_t F, const int32_t* mel_lo, const int32_t* mel_cnt,
                   const int32_t* mel_off, const float* mel_w, int32_t mel_M, int32_t mel_nnz, int32_t log_,
                   float eps, float* out, ptmi_stream_t stream);

/* ---- Masked normalisation --------------------------------------------------------------------------
 * Replaces padertorch/modules/normalization.py: normalize / _Normalize.forward (:345-372, statistics by
 * mask_and_compute_stats :497-512), the hand-written backward (:374-411) and the running-statistics
 * path Normalization._running_norm (:233-246).
 * The tensor is contiguous, rank <= 5; per axis: its size, its stride in the statistics-group index
 * (0 for an axis the statistics run over) and in the gamma / beta index (0 where those broadcast);
 * batch_dim / seq_dim (or -1) locate the mask t < lengths[b].
 *   ptmi_norm_reduce      mode 0: (sum m x, sum m x^2, sum m) per statistics group;
 *                         mode 1: (sum ghat, sum ghat xc, sum xc), ghat = gy gamma, xc = x - mean (shift);
 *                         mode 2: (sum gy xhat, sum gy, 0) per gamma / beta element (their gradients).
 *                         out [groups, 3] float64; workspace: ptmi_norm_workspace_elems(geom, mode == 2).
 *   ptmi_norm_elementwise backward = 0: y = m ((x - mean) rstd gamma + beta);
 *                         backward = 1: dx = m (gy gamma rstd + c1[g] (x - mean) + c0[g]).
 * mean / rstd / c0 / c1 are float32 per statistics group, gamma / beta float32 per independent index
 * (NULL = absent). */
typedef struct ptmi_norm_geom {
    int32_t rank;
    int64_t size[5];
    int64_t stat_group_stride[5];
    int64_t indep_stride[5];
    int32_t batch_dim, seq_dim;
} ptmi_norm_geom;
int64_t ptmi_norm_workspace_elems(const ptmi_norm_geom* geom, int32_t which);
int ptmi_norm_reduce(int32_t mode, const float* x, const float* gy, const int32_t* lengths, const float* mean,
                     const float* rstd, const float* gamma, const ptmi_norm_geom* geom, int32_t shift,
                     double* workspace, double* out, ptmi_stream_t stream);
int ptmi_norm_elementwise(int32_t backward, const float* x, const float* gy, const int32_t* lengths,
                          const float* mean, const float* rstd, const float* gamma, const float* beta,
                          const float* c0, const float* c1, const ptmi_norm_geom* geom, int32_t shift,
                          int32_t scale, float* out, ptmi_stream_t stream);

/* ---- Unit-norm embeddings ------------------------------------------------------------------------
 * Replaces torch.nn.functional.normalize(h, dim=-2) of padertorch/contrib/tcl/dc.py:70 (and its autograd
 * backward) on the [N, E, F] embedding (F contiguous; E <= 32: register-tiled, one HBM pass; wider: the E values read twice):
 *   forward : y = x / max(||x[n, :, f]||_2, eps);  inv_norm [N, F] = 1 / max(norm, eps) is kept for
 *   backward: dx = inv_norm (gy - y <gy, y>_E)   (inv_norm gy where the norm was clamped to eps).
 * One HBM pass each. */
int ptmi_unit_norm_forward(const float* x, float* y, float* inv_norm, int64_t N, int32_t E, int32_t F, float eps,
                           ptmi_stream_t stream);
int ptmi_unit_norm_backward(const float* gy, const float* y, const float* inv_norm, float* dx, int64_t N, int32_t E,
                            int32_t F, float eps, ptmi_stream_t stream);

/* ---- Time-domain regression losses under PIT ------------------------------------------------------
 * Replaces padertorch/ops/losses/regression.py:47-378 (mse_loss, log_mse_loss, sdr_loss, si_sdr_loss,
 * log1p_mse_loss, source_aggregated_sdr_loss) evaluated per permutation by pit_loss
 * (ops/losses/source_separation.py:110-119) and the TasNet loss loop
 * (contrib/examples/source_separation/tasnet/model.py:154-176).
 *
 * ptmi_td_pair_stats: one streaming pass over est / tgt [batch, K, T] (time contiguous; strides[4] =
 * {est_b, est_k, tgt_b, tgt_k} in elements, HOST array; lengths[b] <= T valid samples or NULL) ->
 * stats [batch, K*K + 4K] float64 per example:  Set[i][j] = sum e_i t_j | See[i] | Stt[j] | Se[i] | St[j].
 * workspace: ptmi_td_workspace_elems(batch, K, T) float64.  K <= 8, batch <= 65535.
 *
 * ptmi_td_lincomb: out[b,i,t] = a[b,i] x[b,i,t] + sum_j bmat[b,i,j] y[b,j,t] + c[b,i] for t < lengths[b],
 * 0 beyond (the backward pass: d loss / d estimate with x = est, y = tgt; d / d target with the roles
 * swapped).  strides[6] = {x_b, x_k, y_b, y_k, out_b, out_k}; coefficients are device float32. */
int64_t ptmi_td_stats_elems(int32_t K);
int64_t ptmi_td_workspace_elems(int64_t batch, int32_t K, int64_t T);
int ptmi_td_pair_stats(const float* est, const float* tgt, const int32_t* lengths, int64_t batch, int32_t K,
                       int64_t T, const int64_t* strides, double* workspace, double* stats,
                       ptmi_stream_t stream);
int ptmi_td_lincomb(const float* x, const float* y, const int32_t* lengths, const float* coef_a,
                    const float* coef_b, const float* coef_c, int64_t batch, int32_t K, int64_t T,
                    const int64_t* strides, float* out, ptmi_stream_t stream);

/* ---- TasNet learned-basis encoder / decoder ---------------------------------------------------------
 * Replaces torch.nn.Conv1d(1, N, L, stride) + relu of TasEncoder and torch.nn.ConvTranspose1d(N, 1, L, stride)
 * of TasDecoder (padertorch/contrib/examples/source_separation/tasnet/tas_coders.py:9-135), the
 * "mask x encoded -> decode" tail of TasNet.forward (tasnet/model.py:119-129), and their autograd backwards.
 * All tensors fp32 and contiguous: signals [B, T], features [B, N, E], masks [K, B, N, E], weight [N, L]
 * (either module's [N, 1, L] parameter).  No atomics; every sum has a fixed order (bit-reproducible); no
 * allocation and no synchronisation (capturable).  B <= 65535.
 *
 * ptmi_tas_analysis : out[b,n,tau] = act(sum_l weight[n,l] x[b, tau stride + l] + bias[n]), tau < E; samples at or
 *   beyond T read as zero (the zero padding of tas_coders.py:73-76 without the copy); bias [N] or NULL;
 *   relu != 0: act = relu (tas_coders.py:87), else identity (the decoder's gradient w.r.t. its input).
 * ptmi_tas_synthesis: y[k,b,t] = sum_n sum_{tau stride + l = t} p[b,n,tau] weight[n,l] + bias[0], t < T_out: the decoder's
 *   T_out is (E - 1) stride + L (tas_coders.py:135); a sample no window reaches (stride > L, or t beyond that) gets the
 *   bias alone; bias [1] or NULL.  mask [K, B, N, E]: p counts as mask[k] p, formed
 *   on the fly (model.py:119-129); else K = 1.  gate [B, N, E] (without mask): p counts where gate > 0 (the
 *   encoder's gradient w.r.t. its input: p = grad, gate = the encoder's output, T_out = T).
 * ptmi_tas_masked_decode_backward: with A_k = analysis(gy[k]) (identity, no bias; never stored):
 *   dmask[k,b,n,tau] = encoded[b,n,tau] A_k[b,n,tau], dencoded[b,n,tau] = sum_k mask[k,b,n,tau] A_k[b,n,tau];
 *   gy [K, B, T].
 * ptmi_tas_wgrad    : out[0 : N L]       = dW[n,l] = sum_{k,b,tau} g[b,n,tau] x[k,b, tau stride + l]
 *                     out[N L : N L + N] = sum_{b,tau} g[b,n,tau]     (the encoder's bias gradient)
 *                     out[N L + N]       = sum_{k,b,t} x[k,b,t]       (the decoder's bias gradient)
 *   x [K, B, T] reads as zero beyond T.  mask / gate as in ptmi_tas_synthesis (g counts as mask[k] g, or where
 *   gate > 0).  workspace: ptmi_tas_wgrad_workspace_elems(B, N, L, stride, E) floats of per-workgroup partial
 *   sums, added in a fixed order by a second kernel. */
int ptmi_tas_analysis(const float* x, const float* weight, const float* bias, float* out, int64_t B, int64_t T, int32_t N,
                      int32_t L, int32_t stride, int64_t E, int32_t relu, ptmi_stream_t stream);
int ptmi_tas_synthesis(const float* p, const float* mask, const float* gate, const float* weight, const float* bias, float* y,
                       int32_t K, int64_t B, int32_t N, int32_t L, int32_t stride, int64_t E, int64_t T_out,
                       ptmi_stream_t stream);
int ptmi_tas_masked_decode_backward(const float* gy, const float* mask, const float* encoded, const float* weight, float* dmask,
                                    float* dencoded, int32_t K, int64_t B, int64_t T, int32_t N, int32_t L, int32_t stride,
                                    int64_t E, ptmi_stream_t stream);
int64_t ptmi_tas_wgrad_workspace_elems(int64_t B, int32_t N, int32_t L, int32_t stride, int64_t E);
int ptmi_tas_wgrad(const float* g, const float* mask, const float* gate, const float* x, int32_t K, int64_t B, int64_t T,
                   int32_t N, int32_t L, int32_t stride, int64_t E, float* workspace, float* out, ptmi_stream_t stream);

/* ---- Conv-TasNet separator: the non-GEMM part of a temporal convolution block -------------------------
 * Replaces, inside _Conv1DBlock (padertorch/modules/convnet.py:114-161), the chain PReLU -> pad -> depthwise dilated
 * Conv1d -> PReLU and the norms gLN / cLN of padertorch/contrib/jensheit/norm.py:10-70, forward and backward.
 * All activations fp32 [B, T, C] contiguous, CHANNELS INNERMOST (the reference's [B, C, T] transposed).  No atomics;
 * partial sums are fp64 and added in a fixed order (bit-reproducible); no allocation, no synchronisation
 * (capturable).  Workspaces are caller-owned arrays of DOUBLES.  B <= 65535.
 *
 * ptmi_tcn_depthwise_forward : v[b,t,h] = prelu(slope_out, bias[h] + sum_k weight[h,k] p[b, t + k dilation - front, h])
 *   with p = prelu(slope_in, u), p = 0 outside [0, T) (the reference pads behind the first PReLU), front =
 *   (dilation (K - 1)) / 2 (compute_pad_size(K, dilation, 1, 'both'): an even K pads the end more); weight [H, K] (the
 *   [H, 1, K] parameter), bias [H] or NULL, slopes [1] in device memory; prelu'(0) = slope.
 *   stats [B, 2] = (mean, 1 / sqrt(var + eps)) of v per example (biased variance): the gLN statistics, from the same launch's
 *   partial sums.
 * ptmi_tcn_depthwise_backward: gz [B, T, H] (scratch: the gradient at the second pre-activation, recomputed from u), gu,
 *   dparams [H K + H + 2] = d weight [H, K] | d bias [H] | d slope_in | d slope_out.
 * ptmi_tcn_norm_stats  : stats [G, 2] = (mean, rstd) of x per group: rows == 0 a group is an example (over T C, gLN; needs the
 *   workspace), else a row (over C, cLN; workspace unused, may be NULL).
 * ptmi_tcn_norm_apply  : y = gamma[c] (x - mean_g) rstd_g + beta[c].
 * ptmi_tcn_norm_backward: dx, dparams [2 C] = d gamma | d beta; gsum [G, 2] scratch (the two group means of the gradient). */
int64_t ptmi_tcn_depthwise_workspace_elems(int64_t B, int64_t T, int32_t H, int32_t K);
int ptmi_tcn_depthwise_forward(const float* u, const float* slope_in, const float* weight, const float* bias, const float* slope_out,
                               float* v, float* stats, double* workspace, int64_t B, int64_t T, int32_t H, int32_t K,
                               int32_t dilation, float eps, ptmi_stream_t stream);
int ptmi_tcn_depthwise_backward(const float* gv, const float* u, const float* slope_in, const float* weight, const float* bias,
                                const float* slope_out, float* gz, float* gu, float* dparams, double* workspace, int64_t B,
                                int64_t T, int32_t H, int32_t K, int32_t dilation, ptmi_stream_t stream);
int64_t ptmi_tcn_norm_workspace_elems(int64_t B, int64_t T, int32_t C);
int ptmi_tcn_norm_stats(const float* x, float* stats, double* workspace, int64_t B, int64_t T, int32_t C, int32_t rows, float eps,
                        ptmi_stream_t stream);
int ptmi_tcn_norm_apply(const float* x, const float* stats, const float* gamma, const float* beta, float* y, int64_t B, int64_t T,
                        int32_t C, int32_t rows, ptmi_stream_t stream);
int ptmi_tcn_norm_backward(const float* gy, const float* x, const float* stats, const float* gamma, float* dx, float* dparams,
                           float* gsum, double* workspace, int64_t B, int64_t T, int32_t C, int32_t rows, ptmi_stream_t stream);

/* ---- TasNet model: the glue between encoder, separator, output projection and decoder -----------------
 * Replaces, in TasNet.forward (padertorch/contrib/examples/source_separation/tasnet/model.py:69-152), the examplewise LayerNorm
 * with its rearranges, the output PReLU, chunk / stack / nonlinearity behind the output projection and the mean subtraction,
 * forward and backward.  The coders' side is [B, N, E] (channels first, E frames innermost), the separator's [B, E, C]
 * (channels last); fp32, contiguous.  No atomics; sums are fp64, their per-workgroup partials go to the caller's workspace
 * (DOUBLES) and are added in ascending order by a second kernel (bit-reproducible); no allocation, no synchronisation
 * (capturable).  B <= 65535.
 *
 * ptmi_tasnet_entry_norm_forward : y[b,e,:] = gamma (w[b,:,e] - mean) rstd + beta over the N channels of frame e (biased variance,
 *   rstd = 1 / sqrt(var + eps)) for e < lengths[b], 0 (not beta) from there on; lengths [B] in DEVICE memory, int32 or
 *   (lengths_int64 != 0) int64, clipped to [0, E], NULL: every frame is live.  stats [B E, 2] = (mean, rstd), (0, 0) on dead rows.
 * ptmi_tasnet_entry_norm_backward: dw [B, N, E] = rstd (gy gamma - mean_n(gy gamma) - xhat mean_n(gy gamma xhat)) on live rows, 0 on
 *   dead ones; dparams [2 N] = d gamma | d beta over the live rows.
 * ptmi_tasnet_prelu_forward / _backward: y = x > 0 ? x : a x on n elements, a = slope[0] in device memory; gx = x > 0 ? g : a g,
 *   dslope [1] = sum over x <= 0 of g x.
 * ptmi_tasnet_mask_head_forward  : z [B, E, A + K N] -> m [K, B, N, E] = act(z[b, e, A + k N + n]) and, A > 0,
 *   additional [B, A, E] = z[b, e, :A] (no activation).  activation: 0 sigmoid, 1 relu, 2 leaky_relu (0.01), 3 elu (alpha 1),
 *   4 tanh, 5 identity.
 * ptmi_tasnet_mask_head_backward : gz [B, E, A + K N] from gm, the saved OUTPUT m and g_additional (NULL: zeros).
 * ptmi_tasnet_center : backward == 0: in [K, B, T_in] -> out [B, K, T_out] = in[k, b, t] - mean_{t < T_out} in[k, b, t] (T_out <= T_in);
 *   backward != 0, its adjoint: in [B, K, T_out] -> out [K, B, T_in] = in - mean(in), zeros from T_out on.  K B <= 65535. */
int64_t ptmi_tasnet_entry_norm_workspace_elems(int64_t B, int32_t N, int64_t E);
int ptmi_tasnet_entry_norm_forward(const float* w, const float* gamma, const float* beta, const void* lengths, int32_t lengths_int64,
                                   float* y, float* stats, int64_t B, int32_t N, int64_t E, float eps, ptmi_stream_t stream);
int ptmi_tasnet_entry_norm_backward(const float* gy, const float* w, const float* stats, const float* gamma, const void* lengths,
                                    int32_t lengths_int64, float* dw, float* dparams, double* workspace, int64_t B, int32_t N,
                                    int64_t E, ptmi_stream_t stream);
int64_t ptmi_tasnet_prelu_workspace_elems(int64_t n);
int ptmi_tasnet_prelu_forward(const float* x, const float* slope, float* y, int64_t n, ptmi_stream_t stream);
int ptmi_tasnet_prelu_backward(const float* g, const float* x, const float* slope, float* gx, float* dslope, double* workspace,
                               int64_t n, ptmi_stream_t stream);
int ptmi_tasnet_mask_head_forward(const float* z, float* m, float* additional, int64_t B, int64_t E, int32_t N, int32_t K, int32_t A,
                                  int32_t activation, ptmi_stream_t stream);
int ptmi_tasnet_mask_head_backward(const float* gm, const float* m, const float* g_additional, float* gz, int64_t B, int64_t E,
                                   int32_t N, int32_t K, int32_t A, int32_t activation, ptmi_stream_t stream);
int64_t ptmi_tasnet_center_workspace_elems(int64_t K, int64_t B, int64_t T_in, int64_t T_out);
int ptmi_tasnet_center(const float* in, float* out, double* workspace, int64_t K, int64_t B, int64_t T_in, int64_t T_out,
                       int32_t backward, ptmi_stream_t stream);

/* ---- Dual-path RNN separator ------------------------------------------------------------------------
 * padertorch/modules/dual_path_rnn.py between its GEMMs.  The chunked activation is [B, S, K, N] (channels last, chunk-major); a
 * "position" is a row (b, s, k) of it; fp32, contiguous unless strides are taken.  A sequence is (base row, step stride, step
 * count): an int32 table [nseq][3] in DEVICE memory.  No atomics; sums over rows are fp64, per-slab partials in the caller's
 * workspace (DOUBLES) added in ascending order by a second kernel (bit-reproducible); no allocation, no synchronisation (capturable).
 *
 * ptmi_dprnn_num_chunks : S of a signal of L frames: the K - P zero frames in front and behind, window K, hop P, end='pad'.
 * ptmi_dprnn_tables     : chunks [B] = S_b = (len_b + (K - P) - 1) // P + 1 clipped to [0, S] (lengths [B] in DEVICE memory, int32 or
 *   (lengths_int64 != 0) int64; NULL: S); intra [B S][3] = (row (b, s, 0), 1, s < S_b ? K : 0); inter [B K][3] = (row (b, 0, k), K, S_b).
 *   B S K < 2^31.
 * ptmi_chunk_lstm_forward : the time loop of one torch.nn.LSTM layer, ndir = 1 or 2 directions, over the table's sequences.  gates
 *   [rows, ndir 4H] holds x W_ih^T + b_ih (direction-major, then i | f | g | o) and is OVERWRITTEN by the activated gates; h, c
 *   [rows, ndir H] are written on the rows of the steps; h is 0 on rows base + t stride, count <= t < cap (cap: the steps a sequence
 *   has room for); rows of no sequence are not touched.  A reverse direction starts at the sequence's own last step.  One workgroup
 *   owns ptmi_chunk_lstm_tile() sequences of one direction; W_hh stays in registers for H <= ptmi_chunk_lstm_max_resident_hidden()
 *   (128) and is streamed from the L2 every step above that, up to H = ptmi_chunk_lstm_max_hidden() (1536: the backward kernel
 *   keeps d gates, dh and dc of its sequences in LDS, 96 H bytes of the 160 KB of a CU).
 * ptmi_chunk_lstm_backward: gates holds the forward's output and is OVERWRITTEN by d gates (pre-activation), 0 on the rows between
 *   count and cap; hprev [rows, ndir H] = h of the step before (0 at a first step and between count and cap): the operand of dW_hh.
 * ptmi_dprnn_colsum     : out [C] = sum over rows of x [rows, C] (row stride ld); out2 (or NULL) receives the same sums.
 * ptmi_dprnn_norm_residual_forward : y = (s < chunks[b] ? gamma (z - mean) rstd + beta : 0) + residual per row of z [rows, N],
 *   rows = B S K, statistics over N (biased variance); chunks NULL: every row is valid.  stats [rows, 2] = (mean, rstd), (0, 0) on
 *   invalid rows.
 * ptmi_dprnn_norm_residual_backward: dz (0 on invalid rows), dresidual = gy, dparams [2 N] = d gamma | d beta.
 * ptmi_dprnn_segment    : x [B, L, N] (strides {b, l, n} in elements, HOST array) -> seg [B, S, K, N],
 *   seg[b, s, k] = x[b, s P + k - (K - P)] inside [0, L), 0 outside.
 * ptmi_dprnn_overlap_add: seg [B, S, K, N] (strides {b, s, k, n}, HOST array) -> out [B, L_out, N]: the sum, chunks ascending, of the
 *   elements of the padded signal's frame l + front (front = K - P: the frames of x, what segment maps frame l to - its adjoint,
 *   and segment is the adjoint of this; front = 0: the padded signal, L_out up to (S - 1) P + K). */
int64_t ptmi_dprnn_num_chunks(int64_t L, int32_t K, int32_t P);
int ptmi_dprnn_tables(const void* lengths, int32_t lengths_int64, int32_t B, int32_t S, int32_t K, int32_t P, int32_t* chunks,
                      int32_t* intra, int32_t* inter, ptmi_stream_t stream);
int32_t ptmi_chunk_lstm_max_hidden(void);
int32_t ptmi_chunk_lstm_max_resident_hidden(void);
int32_t ptmi_chunk_lstm_tile(void);
int ptmi_chunk_lstm_forward(float* gates, const float* w_hh, const float* w_hh_reverse, const float* b_hh, const float* b_hh_reverse,
                            float* h, float* c, const int32_t* table, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                            ptmi_stream_t stream);
int ptmi_chunk_lstm_backward(float* gates, const float* dh, const float* w_hh, const float* w_hh_reverse, const float* h, const float* c,
                             float* hprev, const int32_t* table, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                             ptmi_stream_t stream);
int64_t ptmi_dprnn_colsum_workspace_elems(int64_t rows, int32_t C);
int ptmi_dprnn_colsum(const float* x, int64_t ld, float* out, float* out2, double* workspace, int64_t rows, int32_t C,
                      ptmi_stream_t stream);
int ptmi_dprnn_norm_residual_forward(const float* z, const float* residual, const float* gamma, const float* beta,
                                     const int32_t* chunks, float* y, float* stats, int64_t rows, int32_t N, int32_t S, int32_t K,
                                     float eps, ptmi_stream_t stream);
int ptmi_dprnn_norm_residual_backward(const float* gy, const float* z, const float* stats, const float* gamma, const int32_t* chunks,
                                      float* dz, float* dresidual, float* dparams, double* workspace, int64_t rows, int32_t N,
                                      int32_t S, int32_t K, ptmi_stream_t stream);
int ptmi_dprnn_segment(const float* x, const int64_t* x_strides, float* seg, int64_t B, int64_t L, int32_t N, int32_t S, int32_t K,
                       int32_t P, ptmi_stream_t stream);
int ptmi_dprnn_overlap_add(const float* seg, const int64_t* seg_strides, float* out, int64_t B, int64_t L_out, int32_t N, int32_t S,
                           int32_t K, int32_t P, int32_t front, ptmi_stream_t stream);

/* ---- One-and-Rest PIT: loss and flag head ------------------------------------------------------------
 * Replaces, in padertorch/contrib/examples/source_separation/or_pit/model.py, the loss loop of review (:319-350: B x iterations x K
 * calls of log_mse_loss on slices through one_and_rest_permutation_invariant_loss, :58-98, with fill_missing_with_zeros=True) and
 * the flag head (:187-218: rearrange, Linear, (weighted) mean, sigmoid), forward and backward.  fp32 data, fp64 sums of exact
 * products; no atomics, per-workgroup partials in the caller's workspace (DOUBLES) added in ascending order by a second kernel
 * (bit-reproducible); no allocation, no synchronisation (capturable).  batch <= 65535.
 *
 * ptmi_td_rect_stats  : est [batch, M, T], tgt [batch, K, T] (time contiguous; strides[4] = {est_b, est_m, tgt_b, tgt_k} in
 *   elements, HOST array) -> stats [batch, M K + M] float64 = C[m][j] = sum e_m t_j | See[m] = sum e_m^2 and, gram != NULL,
 *   gram [batch, K, K] = sum t_j t_l (it does not depend on est: once per step).  0 <= K <= 8 (tgt may be NULL for K == 0),
 *   1 <= M <= 8.  workspace: ptmi_td_rect_workspace_elems(batch, M, K, T) float64.
 * ptmi_orpit_select   : one iteration's loss per example from stats (M = 2) and gram, n = T samples.  alive_in [batch, K] int32
 *   marks the targets not yet chosen, R their number.  R >= 2: the candidates i (alive) are
 *   log10(mse(e_0, t_i)) + 1 / (R - 1) log10(mse(e_1, sum_{j alive, j != i} t_j)), mse = (See - 2 Set + Stt) / n; the first minimum
 *   in ascending i wins (a NaN candidate wins over numbers, as torch.min).  R == 1: log10(mse(e_0, t_alive)) + log10(See_1 / n).
 *   R == 0: log10(See_0 / n) + log10(See_1 / n).  Outputs: loss [batch] fp32, choice [batch] int32 (-1: none), alive_out (may be
 *   alive_in) and the coefficients of d loss / d e_m = a[m] e_m + sum_j bmat[m][j] t_j: coef_a [batch, 2], coef_b [batch, 2, K]
 *   (a_m = 2 w_m / (ln 10 SSE_m), w_0 = 1, w_1 = 1 / (R - 1) or 1; bmat[m][j] = -a_m on row m's target set, else 0).
 * ptmi_td_rect_lincomb: out[b,m,t] = g[b] (coef_a[b,m] est[b,m,t] + sum_j coef_b[b,m,j] tgt[b,j,t]); g [batch] or NULL (= 1);
 *   strides[6] = {est_b, est_m, tgt_b, tgt_k, out_b, out_m}.
 * ptmi_orpit_flag_forward : additional [B, A, E], weight [A], bias [1] -> pre[b,e] = bias + sum_a weight[a] additional[b,a,e] and
 *   flag[b] = sigmoid(sum_e pre w / sum_e w).  weighted == 0: w = 1 (the mean; mask, encoded, w unused).  weighted != 0:
 *   w[b,e] = mean_n (mask[k,b,n,e] encoded[b,n,e])^2 with mask [K, B, N, E], encoded [B, N, E] or NULL (the mask IS the
 *   estimate); w [B, E] is stored for the backward pass.  No epsilon: a silent stream gives 0 / 0.
 *   stat [B, 2] float64 = (sum pre w / sum w, sum w).  workspace: ptmi_orpit_flag_workspace_elems(B, A, E) float64.
 * ptmi_orpit_flag_backward: from gflag [B] and gpre [B, E] (or NULL): dadditional [B, A, E], dparams [A + 1] = d weight | d bias
 *   and, weighted, dmask [K, B, N, E] (zeros on the slices other than k) and dencoded [B, N, E] (encoded given). */
int64_t ptmi_td_rect_workspace_elems(int64_t batch, int32_t M, int32_t K, int64_t T);
int ptmi_td_rect_stats(const float* est, const float* tgt, int64_t batch, int32_t M, int32_t K, int64_t T, const int64_t* strides,
                       double* workspace, double* stats, double* gram, ptmi_stream_t stream);
int ptmi_orpit_select(const double* stats, const double* gram, const int32_t* alive_in, int32_t* alive_out, float* loss,
                      int32_t* choice, float* coef_a, float* coef_b, int64_t batch, int32_t K, int64_t n, ptmi_stream_t stream);
int ptmi_td_rect_lincomb(const float* est, const float* tgt, const float* g, const float* coef_a, const float* coef_b, int64_t batch,
                         int32_t M, int32_t K, int64_t T, const int64_t* strides, float* out, ptmi_stream_t stream);
int64_t ptmi_orpit_flag_workspace_elems(int64_t B, int32_t A, int64_t E);
int ptmi_orpit_flag_forward(const float* additional, const float* weight, const float* bias, const float* mask, const float* encoded,
                            float* pre, float* w, float* flag, double* stat, double* workspace, int64_t B, int32_t A, int64_t E,
                            int32_t N, int32_t K, int32_t k, int32_t weighted, ptmi_stream_t stream);
int ptmi_orpit_flag_backward(const float* gflag, const float* gpre, const float* flag, const double* stat, const float* pre, const float* w,
                             const float* additional, const float* weight, const float* mask, const float* encoded, float* dadditional,
                             float* dparams, float* dmask, float* dencoded, double* workspace, int64_t B, int32_t A, int64_t E, int32_t N,
                             int32_t K, int32_t k, int32_t weighted, ptmi_stream_t stream);

/* ---- Mask estimator loss: pooled and power-weighted BCE on logits -------------------------------------
 * Replaces, in padertorch/contrib/jensheit/mask_estimator_example/model.py, the per-example loop of add_losses (:128-237:
 * binary_cross_entropy_with_logits(reduction='none'), TORCH_POOLING_FN_MAP[reduction], weight_loss) for one mask of the whole
 * padded batch, forward and backward.  fp32 data, fp64 sums in one fixed order through per-workgroup partials in the caller's
 * workspace (no floating-point atomics; the histograms of the selection count with integer atomics); bit-reproducible; no
 * allocation, no synchronisation (capturable).  B <= 65535, C T F < 2^31.
 *
 * logits, target: logical [B, C, T, F], unit stride on F; strides[9] = {logits b, c, t, target b, c, t, power b, c, t} in elements
 *   (HOST array; a complex power counts complex elements).  num_frames: device int32 [B] or NULL (all T frames); only frames
 *   t < num_frames[b] (clamped to [0, T]) are read.  power_kind: 0 none, 1 real weights float32 [B, C, T, F], 2 complex64
 *   [B, C, T, F] (the weight is re^2 + im^2).  reduction: 0 mean, 1 median (torch's lower median: rank (n - 1) / 2), 2 min, 3 max.
 * Element loss l = max(x, 0) - x t + log1p(exp(-|x|)).
 * ptmi_mask_loss_forward : pooled [B] (a NaN element makes it NaN), weighted [B] = sum l w / sum w (power given; else may be NULL),
 *   and for the backward pass stat [B, 4] float64 = (sum l, sum l w, sum w, n) and sel [B, 2] int32 = (order-preserving key of the
 *   pooled element, number m of elements with that key; zeros for the mean).
 *   workspace: ptmi_mask_loss_workspace_elems(B, C, T, F) float64.
 * ptmi_mask_loss_backward: dlogits [B, C, T, F] dense = (g_pooled[b] / n (mean) or g_pooled[b] / m on the elements whose loss has
 *   the pooled key (median, min, max), + g_weighted[b] w / sum w) (sigmoid(x) - t); exact zeros behind num_frames[b].  g_pooled and
 *   g_weighted [B] may each be NULL (= 0). */
int64_t ptmi_mask_loss_workspace_elems(int64_t B, int32_t C, int32_t T, int32_t F);
int ptmi_mask_loss_forward(const float* logits, const float* target, const void* power, int32_t power_kind, const int32_t* num_frames,
                           const int64_t* strides, int64_t B, int32_t C, int32_t T, int32_t F, int32_t reduction, double* workspace,
                           float* pooled, float* weighted, double* stat, int32_t* sel, ptmi_stream_t stream);
int ptmi_mask_loss_backward(const float* logits, const float* target, const void* power, int32_t power_kind, const int32_t* num_frames,
                            const int64_t* strides, const float* g_pooled, const float* g_weighted, const double* stat,
                            const int32_t* sel, int64_t B, int32_t C, int32_t T, int32_t F, int32_t reduction, float* dlogits,
                            ptmi_stream_t stream);

/* ---- Mask-based MVDR beamforming --------------------------------------------------------------------
 * What the mask estimators are trained for (padertorch/contrib/examples/speech_enhancement/mask_estimator/evaluate.py:110-137,
 * contrib/jensheit/evaluation.py:14-45; there through pb_bss / paderbox on the host).  Y and X [B, C, T, F] complex64 as interleaved
 * floats (F contiguous), 1 <= C <= 8, B <= 65535; frames [B] int32 or NULL: frames t >= frames[b] are never read, contribute nothing
 * and come out as zero.  fp32 data and products, every sum fp64, no atomics, workspace partials added in a fixed order
 * (bit-reproducible); no allocation, no synchronisation (capturable).
 *
 * ptmi_bf_psd   : psd [M, B, F, C, C] complex128 (interleaved doubles) for the M (1 or 2) masks from ONE pass over Y:
 *   psd[k][b,f,d,e] = sum_t m_k[b,t,f] Y[b,d,t,f] conj(Y[b,e,t,f]) / max(sum_t m_k[b,t,f], 1e-10) (normalize == 0: no division);
 *   both triangles are written from the one sum of the upper one (exactly Hermitian, real diagonal).
 *   mask_mode 2: mask_k [B, C, T, F] fp32 and m_k is its median over the channels (even C: the mean of the two middle values);
 *   mask_mode 1: mask_k [B, T, F] is m_k; mask_mode 0: no mask, m = 1 (M must be 1, the masks NULL): the covariance over the valid
 *   frames.  workspace: ptmi_bf_psd_workspace_elems(B, C, T, F, M) float64.
 * ptmi_bf_souden: psd_target, psd_noise [B, F, C, C] complex128 -> X = psd_noise^-1 psd_target by Gaussian elimination with partial
 *   pivoting (a pivot that is exactly zero leaves the unknowns of its column zero: an all-zero psd_noise gives w = 0),
 *   w_all [B, F, C, C] complex64 = X / max(Re trace X, DBL_MIN) and w [B, F, C] = w_all[:, :, :, ref].  ref_channel >= 0: that column
 *   for every example; ref_channel < 0: per example argmax_r sum_f Re(w_r^H psd_target w_r) / max(sum_f Re(w_r^H psd_noise w_r), DBL_MIN)
 *   with w_r = w_all[:, :, :, r] before rounding, the first maximum; numden [B, F, C, 2] float64 holds the summands (may be NULL for
 *   ref_channel >= 0).  ref_out [B] int32: the column taken.  Rank-deficient, non-zero psd_noise is not guarded.
 * ptmi_bf_apply : Z[b,t,f] = sum_c conj(w[b,f,c]) X[b,c,t,f], Z [B, T, F] complex64; T <= 32 * 65535.
 * ptmi_bf_eig   : the GEV (mode 0) or PCA (mode 1) vector per bin, fp64, one lane a bin: w [B, F, C] complex64, lambda [B, F] float64
 *   (the eigenvalue), sweeps [B, F] int32 or NULL (the Jacobi sweeps a bin took).
 *   mode 0: Cholesky psd_noise = L L^H (lower triangle read), A = L^-1 psd_target L^-H by two triangular solves, made exactly
 *   Hermitian ((A + A^H) / 2); cyclic complex Jacobi (pairs p < q in row order) while off(A)^2 > (2^-52)^2 ||A||_F^2, at most 16
 *   sweeps; v the eigenvector of the largest eigenvalue (first maximum), w = L^-H v, so w^H psd_noise w = 1.
 *   mode 1: the same Jacobi on (psd_target + psd_target^H) / 2, |w|_2 = 1; psd_noise may be NULL unless ban.
 *   Gauge: w is rotated so that its component of largest squared magnitude (first maximum) is real and positive.
 *   A Cholesky pivot that is not > 0 (zero or indefinite psd_noise, NaN) or an all-zero A gives w = 0 and lambda = 0.
 *   ban != 0: the rounded (complex64) w goes through ptmi_bf_ban's arithmetic before it is stored: the same bits as the two calls.
 * ptmi_bf_ban   : blind analytic normalisation, out = w sqrt(|w^H N N w|) / max(|w^H N w|, DBL_MIN) with N = psd_noise, in fp64 on the
 *   complex64 w; a zero vector stays zero.  out may be w.
 * ptmi_bf_phase : per example, for f = 1 .. F-1 in order out_f = w_f exp(-i arg(sum_c w_f,c conj(out_{f-1},c))), out_0 = w_0; a sum that
 *   is exactly zero rotates by nothing.  Computed as out_f = c_f w_f, c_f = c_{f-1} conj(d_f / |d_f|) with d_f = sum_c w_f,c conj(w_{f-1},c)
 *   (c_f = 1 where d_f = 0): a segmented inclusive scan of fp64 unit phasors by one workgroup per example in one fixed order for any
 *   F (bit-reproducible).  out must not be w. */
int64_t ptmi_bf_psd_workspace_elems(int64_t B, int32_t C, int64_t T, int64_t F, int32_t M);
int ptmi_bf_psd(const float* Y, const float* mask0, const float* mask1, const int32_t* frames, int64_t B, int32_t C, int64_t T, int64_t F,
                int32_t M, int32_t mask_mode, int32_t normalize, double* workspace, double* psd, ptmi_stream_t stream);
int ptmi_bf_souden(const double* psd_target, const double* psd_noise, int64_t B, int64_t F, int32_t C, int32_t ref_channel, float* w_all,
                   double* numden, float* w, int32_t* ref_out, ptmi_stream_t stream);
int ptmi_bf_apply(const float* w, const float* X, const int32_t* frames, int64_t B, int32_t C, int64_t T, int64_t F, float* Z,
                  ptmi_stream_t stream);
int ptmi_bf_eig(const double* psd_target, const double* psd_noise, int64_t B, int64_t F, int32_t C, int32_t mode, int32_t ban, float* w,
                double* lambda, int32_t* sweeps, ptmi_stream_t stream);
int ptmi_bf_ban(const float* w, const double* psd_noise, int64_t B, int64_t F, int32_t C, float* out, ptmi_stream_t stream);
int ptmi_bf_phase(const float* w, int64_t B, int64_t F, int32_t C, float* out, ptmi_stream_t stream);

/* ---- Dense layers: fp32 GEMM on the 16-bit matrix cores (split operands) --------------------------
 * Replaces the library GEMMs behind torch.nn.LSTM's input projections and torch.nn.Linear in
 * padertorch/contrib/examples/source_separation/pit/model.py:60-66,97-104 and contrib/tcl/dc.py:32-40,61-66
 * (forward, input gradients, weight gradients): every fp32 operand value v is used as v s = hi + lo (16-bit halves, s a power
 * of two per operand tensor) and every product as hi hi + hi lo + lo hi with fp32 accumulation - as close to the exact result as
 * an fp32 MFMA chain at several times its rate (fp32 MFMA runs at 1/16 of the 16-bit rate on gfx950).
 *
 * ptmi_absmax: out_bits[0] = float bits of max |x[r, c]| over a [rows, cols] fp32 matrix with row stride ld
 * (device; zeroed and written on `stream`).  The pack passes derive the operand scale 2^(13 - exponent) from it. */
int ptmi_absmax(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* out_bits, ptmi_stream_t stream);
/* The same reduction INTO a word that already holds float bits of a non-negative value (0: a pre-zeroed word): the word ends as the
 * maximum of both - a running maximum over several matrices, or ptmi_absmax without its zeroing launch when the caller hands out words
 * of a buffer it has zeroed once. */
int ptmi_absmax_accumulate(const float* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* inout_bits, ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The GEMM itself runs on operands already split into fp16 (hi, lo) planes in MFMA-fragment order (csrc/gemm_planes.hip); a
 * streaming pass per operand makes them from either storage order (weights: once per optimizer step; activations that a
 * recurrence or the feature kernel has already left as planes: not at all).
 *
 * ptmi_pack_planes_t: source x[k][c] fp32, k_rows x cols, row stride ld  ->  planes of the operand whose rows are the
 *   columns c and whose reduction axis is k: [ceil(cols / 16)][ceil(k_rows / 32)][hi | lo][64 chunks of 8 fp16]
 *   (ptmi_planes_elems(cols, k_rows) fp16 values, 16-byte aligned), every value scaled by 2^(13 - exponent(*amax))
 *   (amax: device word from ptmi_absmax or the backward recurrence; NULL: scale 1), zero past the matrix.
 * ptmi_pack_planes_n: the same planes from a source x[r][k] whose reduction axis is contiguous (rows x k, row stride ld):
 *   activations and weights of the forward form x W^T.
 * ptmi_gemm_planes:  C[m, n] (+)= sum_k A[m, k] B[n, k] / (scale_a scale_b) + bias[n]  with A, B as planes of m x k and n x k
 *   operands (same amax words as at packing), fp32 accumulation; products = 3: hi hi + hi lo + lo hi (fp32-equivalent), 1: the
 *   hi planes only (plain 16-bit operands: the reduced-precision mode of BASELINE configs[1]);
 *   split_k > 1: AT MOST that many k ranges (what the workspace of ptmi_gemm_planes_workspace_elems floats holds); how many are used,
 *   and on which workgroup tile (persistent big-tile kernel: work item = (k range, tile)), is a cost model's choice that depends on
 *   the shape alone; the ranges' partial products are summed in range order by a second kernel (reproducible, no atomics).
 *   split_k < 0: exactly -split_k ranges (-1: no split) on the 128 x 128 kernel, whose workgroups fit on a CU next to a workgroup of the
 *   persistent recurrence kernels (callers whose GEMM runs beside a recurrence). */
int64_t ptmi_planes_elems(int64_t rows, int64_t k);
int ptmi_pack_planes_t(const float* x, int64_t k_rows, int64_t cols, int64_t ld, const uint32_t* amax, uint16_t* out,
                       ptmi_stream_t stream);
int ptmi_pack_planes_n(const float* x, int64_t rows, int64_t k, int64_t ld, const uint32_t* amax, uint16_t* out,
                       ptmi_stream_t stream);
int64_t ptmi_gemm_planes_workspace_elems(int32_t m, int32_t n, int32_t k, int32_t split_k);
int ptmi_gemm_planes(const uint16_t* a, const uint32_t* amax_a, const uint16_t* b, const uint32_t* amax_b, const float* bias, float* c,
                     int64_t ldc, int32_t m, int32_t n, int32_t k, int32_t accumulate, int32_t split_k, int32_t products,
                     float* workspace, ptmi_stream_t stream);
/* A dense layer with the ReLU behind it in one call (torch.nn.Linear + torch.nn.ReLU, pit/model.py:98-104, tcl/dc.py:38-40):
 * c = max(a b^T + bias, 0) as ptmi_gemm_planes computes the product (no accumulation), and the float bits of max c into *amax_out (may be
 * NULL; zeroed by the call unless amax_zeroed says the caller has done that) - the operand scale ptmi_pack_planes_n takes when c is the next layer's input, so that neither the activation
 * nor ptmi_absmax is a pass of its own.  ptmi_relu_backward_absmax is the matching backward step: out = g where y > 0 (y = the ReLU's
 * output c), else 0, and the float bits of max |out| into *amax_out - what torch's threshold_backward and ptmi_absmax did in two passes. */
int ptmi_gemm_planes_relu(const uint16_t* a, const uint32_t* amax_a, const uint16_t* b, const uint32_t* amax_b, const float* bias, float* c,
                          int64_t ldc, int32_t m, int32_t n, int32_t k, int32_t split_k, int32_t products, float* workspace,
                          uint32_t* amax_out, int32_t amax_zeroed, ptmi_stream_t stream);
int ptmi_relu_backward_absmax(const float* g, const float* y, float* out, int64_t rows, int64_t cols, int64_t ld_g, int64_t ld_y,
                              int64_t ld_out, uint32_t* amax_out, int32_t amax_zeroed, ptmi_stream_t stream);
/* The bf16 flavour of the three calls above: the planes hold bf16 (hi, lo) halves, no operand scale (fp32's exponent range).
 * It exists for the LSTM input gradient dx = dgates W_ih (torch.nn.LSTM backward inside pit/model.py:60-66): the persistent
 * backward recurrence hands its gate gradients on as exactly such planes (its scratch, ptmi_lstm_handoff_cols), so the
 * GEMM takes them as operand A as they lie and only W_ih is packed (once per optimizer step). */
int ptmi_pack_planes_t_bf16(const float* x, int64_t k_rows, int64_t cols, int64_t ld, uint16_t* out, ptmi_stream_t stream);
int ptmi_pack_planes_n_bf16(const float* x, int64_t rows, int64_t k, int64_t ld, uint16_t* out, ptmi_stream_t stream);
/* Any of the four pack passes writing INTO a wider operand: `out` are planes with kb_total k blocks (of 32) per row tile; the
 * source's k blocks land at k block kb_offset, kb_count of them (>= ceil(k / 32); the surplus is zero).  x is [rows_or_k][cols]:
 * transposed = 0: rows x k (ptmi_pack_planes_n), 1: k x operand rows (ptmi_pack_planes_t); bf16 = 1: the bf16 flavour (amax NULL).
 * The stacked input weights of a BLSTM layer as the operand of the previous layer's hand-off planes (k = H columns per direction,
 * padded to ptmi_lstm_handoff_cols) are packed direction by direction this way - no padded fp32 copy. */
int ptmi_pack_planes_into(const float* x, int64_t rows_or_k, int64_t cols, int64_t ld, int32_t transposed, int32_t bf16, const uint32_t* amax,
                          uint16_t* out, int64_t kb_total, int64_t kb_offset, int64_t kb_count, ptmi_stream_t stream);
int ptmi_gemm_planes_bf16(const uint16_t* a, const uint16_t* b, const float* bias, float* c, int64_t ldc, int32_t m, int32_t n,
                          int32_t k, int32_t accumulate, int32_t split_k, int32_t products, float* workspace, ptmi_stream_t stream);
/* ptmi_gemm_planes_bf16 with a TWO-PART output: rows m < m_split of the product go to c, rows m >= m_split to c2 (row m - m_split;
 * same row stride ldc; m_split a multiple of 16; c and c2 equally aligned).  Both directions' dW_ih = [dgates_f | dgates_r]^T x of a
 * BLSTM layer (torch.nn.LSTM backward, pit/model.py:60-66: weight_ih_l<k> and weight_ih_l<k>_reverse are separate parameters) as
 * ONE launch over the operand the backward recurrence hands on (both directions' dgates^T planes lie behind each other). */
int ptmi_gemm_planes_bf16_two(const uint16_t* a, const uint16_t* b, float* c, float* c2, int32_t m_split, int64_t ldc, int32_t m,
                              int32_t n, int32_t k, int32_t accumulate, int32_t split_k, int32_t products, float* workspace,
                              ptmi_stream_t stream);
/* A GROUP of products over one reduction axis as ONE launch of the big-tile kernel and ONE slab reduction: a BLSTM layer's four weight
 * gradients dW_ih_f = dG_f^T X, dW_ih_b = dG_b^T X, dW_hh_f = dG_f^T H_f,prev, dW_hh_b = dG_b^T H_b,prev (torch.nn.LSTM backward inside
 * pit/model.py:60-66,97), whose operands reduce over the same packed rows.
 *   a, m, m_split   bf16 planes of the m x k operand A; rows below m_split are part 0, the rest part 1 (as in ptmi_gemm_planes_bf16_two)
 *   b, n, segments  1..3 B segments: host arrays of the segments' plane buffers (n[s] x k, each packed on its own, 16-byte aligned)
 *                   and column counts
 *   c, ldc          host arrays [2 * segments], entry part * segments + s: where the block (part, segment) goes (rows of the part x
 *                   n[s], row stride ldc >= n[s]), or NULL: the block is skipped (no work item, no store)
 *   split_k         the most k ranges the workspace holds (>= 1); tile and k ranges are picked by the cost model of the plain calls
 *                   over the work items (k range, block, tile) of ALL blocks - a function of the shapes alone (PTMI_GEMM_TILE pins
 *                   the tile and takes split_k as it is)
 *   workspace       ptmi_gemm_planes_group_workspace_elems floats, 16-byte aligned: per block its slabs [k ranges][rows][n[s]]; the
 *                   reduction sums them in slab order and honours accumulate and every block's ldc.  No atomics, no workgroup waits
 *                   for another (safe beside a persistent recurrence); two identical calls give identical bits.
 * Returns PTMI_E_UNSUPPORTED - and launches nothing - where the big-tile path is not possible: the cost model picks the 128 x 128
 * kernel, m_split % 16 != 0, or an operand's planes reach 2 GB; the caller then issues separate calls.
 * ptmi_gemm_planes_group_plan: 100 * tile + k ranges of such a call (tile 5: it would be refused), -1: invalid arguments. */
int ptmi_gemm_planes_bf16_group(const uint16_t* a, int32_t m, int32_t m_split, const uint16_t* const* b, const int32_t* n, int32_t segments,
                                float* const* c, const int64_t* ldc, int32_t k, int32_t accumulate, int32_t split_k, int32_t products,
                                float* workspace, ptmi_stream_t stream);
int64_t ptmi_gemm_planes_group_workspace_elems(int32_t m, int32_t m_split, const int32_t* n, int32_t segments, float* const* c, int32_t k,
                                               int32_t split_k);
int32_t ptmi_gemm_planes_group_plan(int32_t m, int32_t m_split, const int32_t* n, int32_t segments, float* const* c, int32_t k,
                                    int32_t split_k);
/* ptmi_pack_planes_t_bf16 for 1..3 sources x[i] ([k_rows][cols[i]], row stride ld[i]) with one k_rows in ONE launch, each into planes
 * out[i] of its own (ptmi_planes_elems(cols[i], k_rows) values) - the B segments of the call above.  Host arrays.  The planes are
 * bit for bit those of separate ptmi_pack_planes_t_bf16 calls (sources whose rows are not 16-byte aligned are read with scalar loads). */
int ptmi_pack_planes_t_bf16_list(const float* const* x, const int64_t* cols, const int64_t* ld, uint16_t* const* out, int32_t sources,
                                 int64_t k_rows, ptmi_stream_t stream);
/* Calls without split K run on a persistent big-tile kernel (8 wavefronts, workgroup tile picked per problem by a cost model:
 * 0 = 256 x 320, 1 = 256 x 256, 2 = 256 x 192, 3 = 128 x 320, 4 = 128 x 256) or on the 128 x 128 kernel (5) that also carries
 * every co-resident split-K call; ptmi_gemm_planes_plan reports the choice.  (Tests and sweeps pin a tile through the environment
 * variable PTMI_GEMM_TILE, read at every call; there is no entry point for it.) */
/* What a ptmi_gemm_planes[_bf16] call of this shape runs as: 100 * tile + k ranges (tile as above; measurement / labelling only). */
int32_t ptmi_gemm_planes_plan(int32_t m, int32_t n, int32_t k, int32_t split_k);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer step on the Trainer's flat gradient bucket (csrc/optim.hip): replaces, on the step path of
 * padertorch/train/trainer.py:512-532, torch.nn.utils.clip_grad_norm_ (padertorch/train/optimizer.py:35-42),
 * torch.optim.Adam.step (padertorch/train/optimizer.py:79-90 -> :31-33) and zero_grad (:27-29).
 *
 * ptmi_grad_norm: norm_out[0] = 2-norm of flat[0:n] (device fp32; 16-byte aligned).  Reproducible: fixed
 *   per-workgroup slices summed in double, folded in a fixed order.  workspace = device buffer of
 *   ptmi_grad_norm_workspace_elems() doubles.
 *
 * ptmi_adam_flat: for every element i of the bucket (segment s = the parameter tensor it belongs to):
 *     g = flat_grad[i] * min(1, max_norm / (norm[0] + 1e-6))          (norm == NULL: no clipping)
 *     g += weight_decay * p;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g
 *     p -= (lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)),   t = step[0] + 1
 *   i.e. torch.optim.Adam's arithmetic (amsgrad / maximize not supported); flat_grad[i] = 0 afterwards when
 *   zero_grad != 0.  The update is SKIPPED (gradients are still zeroed) when found_inf (device fp32 scalar or NULL)
 *   is non-zero - the semantics of torch's fused Adam -, when `finite` (device fp32 scalar or NULL, e.g. the sum of the
 *   step's losses) or norm[0] is not finite; applied (device fp32 scalar or NULL) receives 1 / 0 = applied / skipped.  segments = device int64 [nseg][3]: parameter pointer, first flat
 *   index, element count, ascending and dense over [0, n).  exp_avg / exp_avg_sq: flat fp32 [n].  The caller
 *   advances `step` (a device fp32 scalar) afterwards.
 *   hyper (device doubles [6] = lr, beta1, beta2, eps, weight_decay, max_norm; 8-byte aligned; or NULL): when given, the kernel reads
 *   the hyper-parameters from these words INSTEAD of the by-value arguments - a step replayed from a hipGraph has its kernel
 *   arguments frozen, and padertorch's hooks rewrite param_group['lr'] between iterations (padertorch/train/hooks.py:736,1029). */
/* ptmi_lstm_bias_grad_add: bias_ih_grad[d][i] += db[d][i] and bias_hh_grad[d][i] += db[d][i] for every direction d (HOST arrays of
 * ndir device pointers; db [ndir][n] = the bias gradient the persistent backward recurrence leaves in its scratch): torch.nn.LSTM
 * keeps two bias vectors per direction (pit/model.py:60-66) that receive the same gradient - one launch instead of 2 ndir. */
int ptmi_lstm_bias_grad_add(const float* db, int32_t ndir, int32_t n, float* const* bias_ih_grad, float* const* bias_hh_grad,
                            ptmi_stream_t stream);
int64_t ptmi_grad_norm_workspace_elems(void);
int ptmi_grad_norm(const float* flat, int64_t n, double* workspace, float* norm_out, ptmi_stream_t stream);
int ptmi_adam_flat(float* flat_grad, float* exp_avg, float* exp_avg_sq, const int64_t* segments, int32_t nseg, int64_t n,
                   const float* norm, float max_norm, const float* found_inf, const float* finite, float* applied,
                   const float* step, double lr, double beta1, double beta2, double eps, double weight_decay, const double* hyper,
                   int32_t zero_grad, ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fast Griffin-Lim phase retrieval (csrc/griffin_lim.hip, the fused update in csrc/stft.hip): replaces
 * padertorch/contrib/mk/synthesis/parametric/griffin_lim.py:32-74 (griffin_lim_step) and :132-155 (the loop of fast_griffin_lim).
 * Spectra are interleaved (re, im) fp32 of n bins; a [n] fp32 magnitudes.  angle(0) := 0 (np.angle): y == 0 projects to (a, 0); a bin
 * whose |y|^2 lies below fp32's normal range projects to the correct unit phasor.
 *
 * Device state of one retrieval: state int32 [4] = done, num_iterations, nparts, reserved (zeroed by the caller before the first
 * iteration); partials = ptmi_gl_partials_elems() doubles; rmse fp32 [iterations] (filled with NaN by the caller).
 *
 * ptmi_gl_project          : P = a y / |y|                                   (griffin_lim.py:55-56, :151-152)
 * ptmi_gl_project_backward : da = Re(conj(y / |y|) g)                        (its adjoint in a; the phase is a constant)
 * ptmi_gl_update           : y = xnew + alpha (xnew - x); x <- xnew; P <- a y / |y|; per-workgroup fp64 partials of (|xnew| - a)^2
 *                            (griffin_lim.py:137-142 on a computed xnew = STFT(iSTFT(P)), :136).  y is never stored.
 * ptmi_gl_stft_update      : the same with xnew = STFT(audio) computed by the launch itself and never stored (the forward STFT's third
 *                            epilogue; x is updated in place); audio [batch, num_samples] whose STFT has exactly `frames` frames
 *                            (PTMI_E_INVALID otherwise).  PTMI_E_UNSUPPORTED for sizes outside the powers of two 64..2048: use
 *                            ptmi_stft_forward + ptmi_gl_update.
 * ptmi_gl_finish           : rmse[iteration] = sqrt(sum of the partials / count) (fixed order, fp64), num_iterations = iteration + 1,
 *                            done = 1 if rmse < atol (griffin_lim.py:139-142, :149; a NaN never stops).
 * Once done is set, ptmi_gl_update / ptmi_gl_stft_update / ptmi_gl_finish return without writing: the loop needs no host read.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t ptmi_gl_partials_elems(void);
int ptmi_gl_project(const float* a, const float* y, int64_t n, float* P, ptmi_stream_t stream);
int ptmi_gl_project_backward(const float* g, const float* y, int64_t n, float* da, ptmi_stream_t stream);
int ptmi_gl_update(const float* xnew, float* x, const float* a, int64_t n, float alpha, float* P, double* partials, int32_t* state,
                   ptmi_stream_t stream);
int ptmi_gl_stft_update(const float* audio, int64_t batch, int64_t row_stride, int64_t num_samples, const float* window,
                        const float* twiddle, const ptmi_stft_geom* g, int64_t frames, float alpha, float* x, const float* a, float* P,
                        double* partials, int32_t* state, ptmi_stream_t stream);
int ptmi_gl_finish(const double* partials, int64_t count, double atol, int32_t iteration, float* rmse, int32_t* state,
                   ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * BigVGAN's anti-aliased periodic activation (csrc/anti_alias.hip): replaces Activation1d, UpSample1d, DownSample1d, LowPassFilter1d of
 * padertorch/contrib/mk/synthesis/vocoder/nvidia_bigvgan/alias_free_activation/torch/ and Snake / SnakeBeta of .../activations.py.
 * x [B, C, T] fp32 contiguous -> y [B, C, M]; one pass: the up-sampled signal stays on chip.
 *
 *   up   (up_filter [up_taps] != NULL)    u[n] = r sum_j x[clamp(j - p)] f[n + pl - j r], n < r T; p = k / r - 1, pl = p r + (k - r) / 2
 *   act  (act = 1; alpha, beta [C])       a = u + sin^2(alpha' u) / (beta' + 1e-9); alpha' = exp(alpha) if logscale
 *   down (down_filter [down_taps] != NULL) y[m] = sum_i g[i] a[clamp(m d + i - left)]; padding: left = k / 2 - (k even), M = ceil(U / d);
 *                                         padding = 0: left = 0, no clamp, M = (U - k) / d + 1
 * A NULL filter switches its stage off (its ratio and taps are ignored); act = 0 makes a = u.  Snake passes beta = alpha.
 * Limits: ratios 1 .. 8, 1 .. 64 taps, up_taps >= up_ratio, r T < 2^30 (PTMI_E_UNSUPPORTED beyond).
 *
 * ptmi_anti_alias_tile            : outputs (forward) / input samples (backward) one workgroup owns: the default geometry (2, 12, 2, 12,
 *                                   padded) is a compile-time specialisation with a tile of its own
 * ptmi_anti_alias_out_len         : M (-1: unsupported geometry)
 * ptmi_anti_alias_workspace_elems : doubles of `workspace` (per-workgroup partials of the parameter gradients)
 * ptmi_anti_alias_backward        : dx [B, C, T] (gather form, u recomputed from x); dalpha / dbeta [C] fp32 when dalpha != NULL: summed in
 *                                   fp64 in one fixed order, no atomics; dbeta == NULL adds both sums into dalpha (Snake).  dalpha == NULL
 *                                   skips the parameter gradients and the workspace.
 * The launches neither allocate nor synchronise.
 * ---------------------------------------------------------------------------------------------------------- */
int32_t ptmi_anti_alias_tile(int32_t default_geometry);
int64_t ptmi_anti_alias_out_len(int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio, int32_t down_taps, int32_t padding);
int64_t ptmi_anti_alias_workspace_elems(int64_t B, int32_t C, int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio,
                                        int32_t down_taps, int32_t padding);
int ptmi_anti_alias_forward(const float* x, const float* up_filter, const float* down_filter, const float* alpha, const float* beta,
                            int64_t B, int32_t C, int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio, int32_t down_taps,
                            int32_t padding, int32_t act, int32_t logscale, float* y, ptmi_stream_t stream);
int ptmi_anti_alias_backward(const float* dy, const float* x, const float* up_filter, const float* down_filter, const float* alpha,
                             const float* beta, int64_t B, int32_t C, int64_t T, int32_t up_ratio, int32_t up_taps, int32_t down_ratio,
                             int32_t down_taps, int32_t padding, int32_t act, int32_t logscale, float* dx, float* dalpha, float* dbeta,
                             double* workspace, ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * WaveNet vocoder (csrc/wavenet.hip): padertorch/ops/mu_law.py, padertorch/modules/wavenet/wavenet.py and the sampling loop of
 * nv-wavenet behind WaveNet.infer.  fp32, activations [B, T, C] with channels innermost; the 1x1 convolutions are ptmi_gemm_planes calls.
 *
 * ptmi_mu_law_encode / _decode : the companding per element in fp64; codes (int64) clamped to [0, Q - 1].  codes_are_float: the decode
 *                                reads float codes.
 * ptmi_wavenet_embed_forward   : codes[i] = mu_law(audio[i]) with Q = A and x0[i, :] = embed[codes[i], :], n = B T rows, one launch
 * ptmi_wavenet_embed_backward  : dembed [A, R] = sum of the rows of dx0 per code, fp64, one fixed order, no atomics
 *                                (workspace: ptmi_wavenet_embed_workspace_elems doubles)
 * ptmi_wavenet_colsum          : out[j] = sum_r x[r ld + j], j < width, fp64, one fixed order (workspace: ..._colsum_workspace_elems)
 * ptmi_wavenet_ola_forward     : the overlap-add of ConvTranspose1d(C, C, window, stride) behind its GEMM G [B Tf, C window] (column
 *                                co window + k): out[b, t', co] = bias[co] + sum_f G[b, f, co, t' + front - f stride], t' < Tout
 *                                (front: what the fading crops in front; front + Tout <= (Tf - 1) stride + window)
 * ptmi_wavenet_ola_backward    : dG[b, f, co, k] = dout[b, f stride + k - front, co] (0 outside [0, Tout))
 * ptmi_wavenet_gate_forward    : P [B T, 4R] = x W^T (rows 0 .. 2R - 1 of W: the tap on x[t - d]); z[b,t,j] = P[b,t-d,j] (0 for t < d)
 *                                + P[b,t,2R+j] + bias[j] + cond[(b T + t) ldc + j]; acts[(b T + t) lda + r] = tanh(z[r]) sigmoid(z[R+r])
 * ptmi_wavenet_gate_backward   : z recomputed; dz [.., 2R] with row stride ldd; dP [B T, 4R] (NULL: skipped): dP[b,t,j] = dz[b,t+d,j],
 *                                dP[b,t,2R+j] = dz[b,t,j]; dbias [2R] (NULL: skipped) the column sum of dz (workspace as _colsum, 2R wide)
 * ptmi_wavenet_generate        : nsteps time steps from t0 for nseq sequences, ptmi_wavenet_generate_ex() of them per workgroup, which
 *                                synchronise with the workgroup barrier alone.  packed: per layer Wg [2R][2R] (k: x[t-d] | x[t]), bg [2R],
 *                                Wrs [R][S + R] (skip | residual), brs [S + R]; then Wo [S][A], We [A][A].  cond [., Tc, L 2R], u [., Tc];
 *                                layer_meta [L][2] = (dilation, first ring row), seq_meta [nseq][3] = (row of cond / u, onset, length).
 *                                ring [groups][ring_rows][ex][R] (zero before t0 = 0) and last_code [groups ex] persist between launches;
 *                                y [nseq, Tmax] int64, logits [nseq, Tmax, A] or NULL.  R <= 256, S <= 1024, A <= 1024.
 * The launches neither allocate nor synchronise.
 * ---------------------------------------------------------------------------------------------------------- */
int ptmi_mu_law_encode(const float* x, int64_t n, int32_t mu_quantization, int64_t* codes, ptmi_stream_t stream);
int ptmi_mu_law_decode(const void* codes, int32_t codes_are_float, int64_t n, int32_t mu_quantization, float* out, ptmi_stream_t stream);
int ptmi_wavenet_embed_forward(const float* audio, const float* embed, int64_t n, int32_t A, int32_t R, int64_t* codes, float* x0,
                               ptmi_stream_t stream);
int64_t ptmi_wavenet_embed_workspace_elems(int64_t n, int32_t A, int32_t R);
int ptmi_wavenet_embed_backward(const float* dx0, const int64_t* codes, int64_t n, int32_t A, int32_t R, float* dembed, double* workspace,
                                ptmi_stream_t stream);
int64_t ptmi_wavenet_colsum_workspace_elems(int64_t rows, int32_t width);
int ptmi_wavenet_colsum(const float* x, int64_t rows, int32_t width, int64_t ld, float* out, double* workspace, ptmi_stream_t stream);
int ptmi_wavenet_ola_forward(const float* G, const float* bias, int64_t B, int32_t C, int64_t Tf, int32_t window, int32_t stride,
                             int64_t front, int64_t Tout, float* out, ptmi_stream_t stream);
int ptmi_wavenet_ola_backward(const float* dout, int64_t B, int32_t C, int64_t Tf, int32_t window, int32_t stride, int64_t front,
                              int64_t Tout, float* dG, ptmi_stream_t stream);
int ptmi_wavenet_gate_forward(const float* P, const float* bias, const float* cond, int64_t ldc, int64_t B, int64_t T, int32_t R,
                              int32_t dilation, float* acts, int64_t lda, ptmi_stream_t stream);
int ptmi_wavenet_gate_backward(const float* dacts, int64_t lda, const float* P, const float* bias, const float* cond, int64_t ldc, int64_t B,
                               int64_t T, int32_t R, int32_t dilation, float* dz, int64_t ldd, float* dP, float* dbias, double* workspace,
                               ptmi_stream_t stream);
int32_t ptmi_wavenet_generate_ex(void);
int32_t ptmi_wavenet_generate_ring_in_lds(int32_t R, int32_t S, int32_t A, int64_t ring_rows);
int ptmi_wavenet_generate(const float* packed, const float* embed, const float* cond, const float* u, const int32_t* layer_meta,
                          const int32_t* seq_meta, int32_t nseq, int64_t Tc, int32_t L, int32_t R, int32_t S, int32_t A, int32_t ring_rows,
                          int64_t t0, int32_t nsteps, int64_t Tmax, float* ring, int32_t* last_code, int64_t* y, float* logits,
                          ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The BigVGAN generator's convolutions, inference only (csrc/bigvgan.hip): conv_pre, the up-sampling ConvTranspose1d, the dilated Conv1d
 * of AMPBlock1 / AMPBlock2 and conv_post of padertorch/contrib/mk/synthesis/vocoder/nvidia_bigvgan/bigvgan.py.  fp32, activations
 * [B, C, T] contiguous (the layout of ptmi_anti_alias_forward), zero padding, every sum in one fixed order, no atomics, no host reads.
 *
 * A dilated Conv1d(C_in, C_out, K odd, dilation d, padding (K - 1) d / 2), weight [C_out, C_in, K], has two forms with one epilogue,
 *   v = scale (conv + bias + residual);  out = v,  or  out += v  when accumulate     (bias [C_out], residual [B, C_out, T]: NULL = absent)
 * ptmi_bigvgan_taps        : the GEMM path behind P [B, K C_out, T] = Wtaps x_b per batch entry (row k C_out + co = tap k of channel co, a
 *                            ptmi_gemm_planes call): conv[b,co,t] = sum_k P[b, k C_out + co, t + (k - (K-1)/2) d], zero outside [0, T).  K <= 63.
 * ptmi_bigvgan_conv_direct : the same convolution from x [B, C_in, T] in plain fp32 FMAs (ci ascending, then k), no P; for the layers
 *                            ptmi_bigvgan_direct_ok admits: C_in <= ptmi_bigvgan_direct_max_channels(), K <= 11, (K - 1) d / 2 <= 64.
 * ptmi_bigvgan_tile        : samples of a row per workgroup, of the taps kernel (0) / the direct kernel (1): what the tests put T around
 * ptmi_bigvgan_ola         : ConvTranspose1d(C_in, C_out, k, u, padding p = (k - u) / 2) behind G [B, C_out k, T] = W^T x_b (row co k + kk):
 *                            out[b,co,t'] = bias[co] + sum_f G[b, co k + kk, f] over f u + kk - p = t' (f ascending, gather form),
 *                            t' < ptmi_bigvgan_ola_out_len = (T - 1) u - 2 p + k.  1 <= u <= 8, k >= u, either parity of k - u.
 * ptmi_bigvgan_post        : conv_post, C -> 1 channel: out[b,t] = act(bias[0] + sum_c sum_k w[c,k] x[b,c,t + k - (K-1)/2]), act = tanhf or the
 *                            clamp to [-1, 1] (NaN stays NaN under both).  K odd, K <= 11.
 * Geometry outside these limits (even K, u > 8, ...) is PTMI_E_INVALID and nothing is launched.  The launches neither allocate nor
 * synchronise.
 * ---------------------------------------------------------------------------------------------------------- */
int32_t ptmi_bigvgan_direct_max_channels(void);
int32_t ptmi_bigvgan_direct_ok(int32_t C_in, int32_t K, int32_t dilation);
int32_t ptmi_bigvgan_tile(int32_t direct);
int64_t ptmi_bigvgan_ola_out_len(int64_t T, int32_t k, int32_t u);
int ptmi_bigvgan_taps(const float* P, const float* bias, const float* residual, int64_t B, int32_t C_out, int64_t T, int32_t K,
                      int32_t dilation, float scale, int32_t accumulate, float* out, ptmi_stream_t stream);
int ptmi_bigvgan_conv_direct(const float* x, const float* weight, const float* bias, const float* residual, int64_t B, int32_t C_in,
                             int32_t C_out, int64_t T, int32_t K, int32_t dilation, float scale, int32_t accumulate, float* out,
                             ptmi_stream_t stream);
int ptmi_bigvgan_ola(const float* G, const float* bias, int64_t B, int32_t C_out, int64_t T, int32_t k, int32_t u, float* out,
                     ptmi_stream_t stream);
int ptmi_bigvgan_post(const float* x, const float* weight, const float* bias, int64_t B, int32_t C, int64_t T, int32_t K, int32_t use_tanh,
                      float* out, ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused attention and the transformer layer's glue (csrc/attention.hip): padertorch/contrib/je/modules/transformer.py.  fp32, every
 * product on the matrix cores in exact fp32 (v_mfma_f32_16x16x4_f32), softmax and all reductions in one fixed order, no atomics, no
 * host reads; the [B, H, Tq, Tk] score tensor is never written unless ptmi_attn_weights is called.
 *
 * Operands are addressed as x[b, h, t, c] = base[b s0 + h s1 + t s2 + c]: `strides` is a HOST array of (s0, s1, s2) per tensor, in the
 * order the prototype lists them (forward: q k v out; weights: q k; backward: q k v out dout dq dk dv).  lse, delta [B, H, Tq] and
 * weights [B, H, Tq, Tk] are contiguous.  1 <= dh, dv <= ptmi_attn_max_head() (= 128; PTMI_E_UNSUPPORTED beyond).
 * Masks (transformer.py:29-36, y + log(mask > 0)): (i, j) is visible iff j < min(Tk, lengths[b]) (lengths: int32 or int64 DEVICE
 * vector, NULL: absent), j <= i + Tk - Tq when causal (get_causal_mask, :259-260) and mask[b m0 + h m1 + i m2 + j m3] != 0 (bytes,
 * `mask_strides` a HOST array of 4, NULL mask: absent).  A row without a visible key is NaN in out, lse and weights.
 *
 * ptmi_attn_tile / _key_tile : rows a workgroup owns (64) / rows of a streamed tile (32): what the tests put Tq and Tk around
 * ptmi_attn_forward   : out = softmax(scale q k^T + masks) v and lse = log sum exp per row (transformer.py:28-38)
 * ptmi_attn_weights   : weights = exp(scale q k^T - lse), renormalised per row, 0 where masked (the second return value of :38)
 * ptmi_attn_backward  : delta = rowsum(dout out) (one small launch), then (dk, dv) by key tile and dq by query tile, probabilities
 *                       recomputed from lse: the adjoint of :28-38 in out
 * ptmi_transformer_posenc : out[b,t,2i] = x + cos(t / freq[i]), out[b,t,2i+1] = x + sin(same) (:234-243; out may be x), d even; freq
 *                       [d / 2] = 10000^(2i/d) is a DEVICE table in float32, as the reference's float32 tensors hold it; the
 *                       angle is one correctly rounded fp32 division, cos / sin the accurate cosf / sinf
 * ptmi_transformer_norm_residual_forward  : rows (b, t) of N channels; norm_first: y = LN(z) + res, else u = z + res, y = LN(u)
 *                       (:151-155, :162-166, :170-174 with norm='layer': Normalization(data_format='btc', statistics_axis='c')); LN is
 *                       zero for t >= lengths[b]; stats [B T, 2] = (mean, rstd)
 * ptmi_transformer_norm_residual_backward : dv = the gradient of LN's input v (z or u) from gy, zero behind the length; dparams [2 N]
 *                       = d gamma | d beta as ordered fp64 column sums (NULL: skipped; workspace: ..._norm_workspace_elems doubles)
 * ---------------------------------------------------------------------------------------------------------- */
int32_t ptmi_attn_tile(void);
int32_t ptmi_attn_key_tile(void);
int32_t ptmi_attn_max_head(void);
int ptmi_attn_forward(const float* q, const float* k, const float* v, const int64_t* strides, int32_t B, int32_t H, int64_t Tq, int64_t Tk,
                      int32_t dh, int32_t dv, float scale, const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask,
                      const int64_t* mask_strides, float* out, float* lse, ptmi_stream_t stream);
int ptmi_attn_weights(const float* q, const float* k, const float* lse, const int64_t* strides, int32_t B, int32_t H, int64_t Tq, int64_t Tk,
                      int32_t dh, float scale, const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask,
                      const int64_t* mask_strides, float* weights, ptmi_stream_t stream);
int ptmi_attn_backward(const float* q, const float* k, const float* v, const float* out, const float* dout, const float* lse,
                       const int64_t* strides, int32_t B, int32_t H, int64_t Tq, int64_t Tk, int32_t dh, int32_t dv, float scale,
                       const void* lengths, int32_t lengths_int64, int32_t causal, const uint8_t* mask, const int64_t* mask_strides,
                       float* delta, float* dq, float* dk, float* dv_out, ptmi_stream_t stream);
int ptmi_transformer_posenc(const float* x, float* out, const float* freq, int64_t B, int64_t T, int32_t d, ptmi_stream_t stream);
int64_t ptmi_transformer_norm_workspace_elems(int64_t rows, int32_t N);
int ptmi_transformer_norm_residual_forward(const float* z, const float* res, const float* gamma, const float* beta, const void* lengths,
                                           int32_t lengths_int64, int64_t B, int64_t T, int32_t N, float eps, int32_t norm_first, float* y,
                                           float* u, float* stats, ptmi_stream_t stream);
int ptmi_transformer_norm_residual_backward(const float* gy, const float* v, const float* stats, const float* gamma, const void* lengths,
                                            int32_t lengths_int64, int64_t B, int64_t T, int32_t N, float* dv, float* dparams,
                                            double* workspace, ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The GRU recurrence (csrc/gru.hip) and the sequence glue (csrc/seq_pool.hip) of padertorch/contrib/je/modules/rnn.py and reduce.py.
 * fp32, every launcher capturable, lengths and tables are device data, sums fp64 in a fixed order, no atomics.
 *
 * ptmi_chunk_gru_forward  : the time loop of one torch.nn.GRU layer (gate order r, z, n), ndir = 1 or 2 directions, over the sequences
 *   of table [nseq][3] = (base row, step stride, step count <= cap), the contract of ptmi_chunk_lstm_forward.  gates [rows, ndir 3H]
 *   holds x W_ih^T + b_ih and becomes the activated gates; q [rows, ndir H] receives h W_hn^T + b_hn, h [rows, ndir H] the output (zero
 *   on a sequence's rows count .. cap).  b_hh may be NULL (bias=False).  flip != 0 runs direction d in the opposite sense of time.  A
 *   sequence whose rows do not all lie inside [0, rows) is skipped.  A workgroup owns ptmi_chunk_gru_tile() sequences of one
 *   direction; W_hh stays in registers for H <= ptmi_chunk_gru_max_resident_hidden() (128) and is streamed from the L2 above that, up
 *   to H = ptmi_chunk_gru_max_hidden() (1792: the streamed backward kernel keeps 5 tile H words in LDS); beyond: PTMI_E_UNSUPPORTED.
 * ptmi_chunk_gru_backward : gates is OVERWRITTEN by (dr_pre, dz_pre, dn_pre) - the operand of dW_ih, db_ih and dx - and q by dn_pre r,
 *   the n block of the operand of dW_hh and db_hh (its r and z blocks are those of gates); hprev [rows, ndir H] receives h of every
 *   row's step before.  Zeros in all three on the rows of no step.
 * ptmi_seq_table   : table [B][3] = (b T, 1, clip(lengths[b], 0, T)); lengths NULL: T.
 * ptmi_seq_gather  : out [B, T, F] contiguous from x through x_strides [3].  mode 0: a copy; 1: reverse_sequence (rnn.py:130-154:
 *   out[b, t] = x[b, len - 1 - t] below the length, x[b, (len - 1 - t) mod T] * 0 behind it); 2: its adjoint (plain zeros behind).
 * ptmi_seq_pool_forward  : x read as [B, M, T, I] = dims [4] through strides [4]; y [B, M, I].  mode 0 sum, 1 mean (with lengths: sum /
 *   (float(len) + 1e-6f), without: / T), 2 max (index [B, M, I] int64 = first position of the maximum, a NaN wins; no step: -inf, 0), 3
 *   last (x[len - 1]; len 0: x[T - 1]), 4 autopool (sum_t softmax_t(alpha x) x over t < len; alpha [M] (then I = 1) or NULL: alpha0).
 *   wave_per_row != 0: a wavefront per (b, m, i), else a thread.
 * ptmi_seq_pool_backward : dx [B, M, T, I] contiguous, written whole.  autopool recomputes the softmax from x and y; dalpha [M] (with
 *   workspace [B M] doubles) = sum over b of g (sum_t w x^2 - y^2), or both NULL.
 * ---------------------------------------------------------------------------------------------------------- */
int32_t ptmi_chunk_gru_max_hidden(void);
int32_t ptmi_chunk_gru_max_resident_hidden(void);
int32_t ptmi_chunk_gru_tile(void);
int ptmi_chunk_gru_forward(float* gates, const float* w_hh, const float* w_hh_reverse, const float* b_hh, const float* b_hh_reverse,
                           float* q, float* h, const int32_t* table, int64_t rows, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                           int32_t flip, ptmi_stream_t stream);
int ptmi_chunk_gru_backward(float* gates, float* q, const float* dh, const float* w_hh, const float* w_hh_reverse, const float* h,
                            float* hprev, const int32_t* table, int64_t rows, int32_t nseq, int32_t cap, int32_t H, int32_t ndir,
                            int32_t flip, ptmi_stream_t stream);
int ptmi_seq_table(const void* lengths, int32_t lengths_int64, int32_t B, int32_t T, int32_t* table, ptmi_stream_t stream);
int ptmi_seq_gather(const float* x, const int64_t* x_strides, const void* lengths, int32_t lengths_int64, float* out, int64_t B, int64_t T,
                    int64_t F, int32_t mode, ptmi_stream_t stream);
int ptmi_seq_pool_forward(const float* x, const int64_t* dims, const int64_t* strides, const void* lengths, int32_t lengths_int64,
                          int32_t mode, const float* alpha, float alpha0, float* y, int64_t* index, int32_t wave_per_row,
                          ptmi_stream_t stream);
int ptmi_seq_pool_backward(const float* x, const int64_t* dims, const int64_t* strides, const void* lengths, int32_t lengths_int64,
                           int32_t mode, const float* alpha, float alpha0, const float* g, const float* y, const int64_t* index,
                           float* dx, double* workspace, float* dalpha, int32_t wave_per_row, ptmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The convolution blocks and pools of padertorch/contrib/je/modules/conv.py and conv_utils.py (csrc/je_conv.hip) on channels-last rows:
 * an activation [B, C, T] is held as [B T, C] (row b T + t).  fp32, every launcher capturable, lengths are device data (int32 or int64,
 * clipped to [0, T]; NULL: T), sums fp64 in a fixed order, no atomics.  act: 0 identity, 1 relu, 2 leaky_relu (act_p: negative slope),
 * 3 elu (act_p: alpha), 4 tanh, 5 sigmoid, 6 prelu (slope: its one parameter on the device).
 *
 * geom [11] of taps / dtaps = (B, T_in, T_out, C_out, K, stride, dilation, front pad, G, ld of P, ld of residual); G = 1, or 2 with gate rows.
 * ptmi_je_conv_taps  : z[b, t, co] = bias[co] + sum_k P[b, t stride + k dilation - front, k C_out + co] (k ascending; rows outside
 *   [0, T_in) are zero: no padded copy), P [B T_in, G K C_out]; gz likewise from the columns K C_out.. and gate_bias.  out != NULL:
 *   out = act(z) sigmoid(gz) + residual in the same launch (gz / residual where given).  z, gz, out [B T_out, C_out] contiguous.
 * ptmi_je_conv_dtaps : dP[b, u, (q K + k) C_out + co] = (q ? dgz : dz)[b, (u + front - k dilation) / stride, co] where the division is
 *   exact and the row exists, else 0; every element of dP [B T_in, G K C_out] is written.
 * ptmi_je_conv_stats : sums [3][groups][C] (doubles; sum, sum of squares, 0) of x [B T, C] (row stride ldx) over t < lengths[b], and
 *   stats [groups][4][C] = mean, rstd = 1 / sqrt(max(power - mean^2, 0) + eps), power, count; groups = 1 (per_example 0: over b and t)
 *   or B.  workspace: ptmi_je_conv_workspace_elems(B, T, C) doubles.
 * ptmi_je_conv_apply : out = act(n) sigmoid(g) + residual with n = gamma (z - mean) rstd + beta and n = 0 for t >= lengths[b]; stats
 *   NULL: n = z and gamma, beta, lengths are not read.  g, residual, gamma, beta may be NULL.
 * ptmi_je_conv_apply_backward : dz (the gradient of z: through the statistics unless fixed_stats) and dgz from dout [B T, C]; dparams
 *   [2 C + 1] = d gamma | d beta | d slope or NULL.  workspace as above and sums [3][groups][C] doubles are needed with stats (not
 *   fixed) or dparams.
 * geom [8] of the pools = (B, T_in, T_out, C, size, stride, front pad, ld of x): the padded axis holds zeros around the T_in values.
 * ptmi_je_pool_forward  : max (index [B T_out, C]: position on the padded axis; the first of equal values, a NaN beats numbers) or mean.
 * ptmi_je_pool_backward : dx [B T_in, C] contiguous, every element written: a gather over the windows that hold the position.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t ptmi_je_conv_workspace_elems(int64_t B, int64_t T, int64_t C);
int ptmi_je_conv_taps(const float* P, const float* bias, const float* gate_bias, const float* residual, const float* slope, float* z,
                      float* gz, float* out, const int64_t* geom, int32_t act, float act_p, ptmi_stream_t stream);
int ptmi_je_conv_dtaps(const float* dz, const float* dgz, float* dP, const int64_t* geom, ptmi_stream_t stream);
int ptmi_je_conv_stats(const float* x, int64_t ldx, const void* lengths, int32_t lengths_int64, int64_t B, int64_t T, int64_t C,
                       int32_t per_example, float eps, double* workspace, double* sums, float* stats, ptmi_stream_t stream);
int ptmi_je_conv_apply(const float* z, int64_t ldz, const float* g, const float* residual, int64_t ldr, const float* stats,
                       const float* gamma, const float* beta, const void* lengths, int32_t lengths_int64, const float* slope, float* out,
                       int64_t B, int64_t T, int64_t C, int32_t per_example, int32_t act, float act_p, ptmi_stream_t stream);
int ptmi_je_conv_apply_backward(const float* dout, const float* z, int64_t ldz, const float* g, const float* stats, const float* gamma,
                                const float* beta, const void* lengths, int32_t lengths_int64, const float* slope, float* dz, float* dgz,
                                float* dparams, double* workspace, double* sums, int64_t B, int64_t T, int64_t C, int32_t per_example,
                                int32_t fixed_stats, int32_t act, float act_p, ptmi_stream_t stream);
int ptmi_je_pool_forward(const float* x, float* y, int64_t* index, const int64_t* geom, int32_t max_pool, ptmi_stream_t stream);
int ptmi_je_pool_backward(const float* dy, const int64_t* index, float* dx, const int64_t* geom, int32_t max_pool, ptmi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Data parallelism: the gradient exchange of padertorch/train/trainer.py:396-442 (parallel_apply over the devices of ONE
 * process, gradients of the replicas summed at :426-428 - accumulated, NOT averaged) as one process per GPU and one RCCL
 * all_reduce(SUM) over xGMI on the flat fp32 gradient bucket.  librccl is opened on first use (dlopen).
 *
 * ptmi_comm_unique_id : rank 0 draws the 128-byte rendezvous id and hands it to the other ranks (file, socket, MPI, env).
 * ptmi_comm_create    : collective over all ranks; binds the device that is CURRENT in the calling thread.
 * ptmi_allreduce_sum  : buffer[0:n] (device fp32) <- sum over ranks, in place, enqueued on `stream`; no division by the
 *                       world size.  Call it for the same n in the same order on every rank.
 * Errors: PTMI_E_UNSUPPORTED when librccl cannot be opened; RCCL's own result r is returned as -100 - r.
 * ------------------------------------------------------------------------------------------- */
#define PTMI_COMM_ID_BYTES 128
typedef struct ptmi_comm ptmi_comm;
int32_t ptmi_comm_rccl_version(void);                  /* e.g. 22105 for 2.21.5; 0: librccl not available */
int ptmi_comm_unique_id(uint8_t* id_out /* [PTMI_COMM_ID_BYTES] */);
int ptmi_comm_create(ptmi_comm** comm, int32_t world_size, int32_t rank, const uint8_t* id);
int ptmi_allreduce_sum(ptmi_comm* comm, float* buffer, int64_t n, ptmi_stream_t stream);
int ptmi_comm_destroy(ptmi_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H_ */
