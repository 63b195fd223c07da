/*
 * s2vt_hip.h — C ABI of libs2vt_hip.so: the MI355X (gfx950) implementation of the S2VT hot path.
 *
 * The reference (Kamino666/S2VT-video-caption) has no native boundary: the path sits behind the
 * Python class `S2VT(nn.Module)` (S2VTModel.py:10-110) and `MaskCriterion` (utils.py:6-26) and all
 * arithmetic is delegated to torch ops.  Each entry point below therefore names the reference call
 * site(s) whose torch op(s) it replaces; `S2VTModel.py` / `utils.py` at the root of this repository
 * are the reference-side bindings (ctypes) a maintainer would drop in — see INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, a positive hipError_t or -1 (bad argument) on failure;
 *    `s2vt_last_error()` gives the message (thread-local).  No C++ exception crosses the ABI.
 *  - all pointers are DEVICE pointers into memory owned by the caller (torch); fp32 unless noted;
 *    parameter tensors use the reference's state_dict layout.
 *  - every call is asynchronous and ordered on `stream` (a hipStream_t passed as void*); nothing is
 *    allocated: scratch comes from the caller-provided workspace (size from *_workspace_bytes).
 *  - one process drives one GPU (one process per GPU for data parallelism).  The library keeps
 *    process-wide state - GEMM arithmetic mode, pipeline block size, its internal side stream, the gradient-ready
 *    events of the last backward - so entry points may be called from any host thread (torch runs the backward
 *    on its autograd thread) but not from several threads at the same time.
 *  - dims: B batch, L = `length` frames (= padded caption length), F feat_dim, H dim_hid,
 *    E dim_embed, V vocab_size; T = 2L-1 LSTM steps.  Internal activations are time-major
 *    [t][b][:]; the external tensors keep the reference's batch-major layout.
 */
#ifndef S2VT_HIP_H
#define S2VT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2VT_ABI_VERSION 9

/* negative return codes (positive ones are hipError_t values) */
#define S2VT_ERR_ARG (-1)      /* bad argument */
#define S2VT_ERR_INDEX (-2)    /* a target id outside [0, vocab_size): the reference raises IndexError (S2VTModel.py:71) */
#define S2VT_ERR_TIMEOUT (-3)  /* a hand-off wait of a persistent recurrence kernel timed out */

typedef struct s2vt_dims {
    int32_t B, L, F, H, E, V;
} s2vt_dims;

/* The 13 parameter tensors of S2VT.__init__ (S2VTModel.py:19-28), reference names in comments. */
typedef struct s2vt_params {
    const float* vid_w_ih;  /* vid_rnn.weight_ih_l0  [4H, H]   */
    const float* vid_w_hh;  /* vid_rnn.weight_hh_l0  [4H, H]   */
    const float* vid_b_ih;  /* vid_rnn.bias_ih_l0    [4H]      */
    const float* vid_b_hh;  /* vid_rnn.bias_hh_l0    [4H]      */
    const float* word_w_ih; /* word_rnn.weight_ih_l0 [4H, E+H] columns = [embed | vid_out] (S2VTModel.py:75) */
    const float* word_w_hh; /* word_rnn.weight_hh_l0 [4H, H]   */
    const float* word_b_ih; /* word_rnn.bias_ih_l0   [4H]      */
    const float* word_b_hh; /* word_rnn.bias_hh_l0   [4H]      */
    const float* feat_w;    /* feat_linear.weight    [H, F]    */
    const float* feat_b;    /* feat_linear.bias      [H]       */
    const float* out_w;     /* out_linear.weight     [V, H]    */
    const float* out_b;     /* out_linear.bias       [V]       */
    const float* emb_w;     /* embedding.weight      [V, E]    */
} s2vt_params;

/* Gradient outputs, same order and shapes; every tensor is OVERWRITTEN (not accumulated). */
typedef struct s2vt_grads {
    float* vid_w_ih; float* vid_w_hh; float* vid_b_ih; float* vid_b_hh;
    float* word_w_ih; float* word_w_hh; float* word_b_ih; float* word_b_hh;
    float* feat_w; float* feat_b; float* out_w; float* out_b; float* emb_w;
} s2vt_grads;

int s2vt_abi_version(void);
const char* s2vt_last_error(void);

/* ---------------------------------------------------------------- whole-path entry points */

/* The batch size the whole-path drivers RUN at for a caller's batch B in the current arithmetic mode: in the plane modes (gemm mode
 * 3 / 1) a batch that is not a multiple of 64 and has at least `pad_min_batch` rows (option, default 33) is padded to the next
 * multiple inside the workspace (zero features, token 0; the pad rows' logits / ids are never handed out and their gradient
 * contributions are exact zeros), so that it takes the plane GEMMs, the persistent recurrence kernels and the decode cache.
 * Smaller batches - the reference's own defaults are 16 (train.py:27) and 10 (eval.py:27) - and gemm mode 0 run as they are on
 * the launch-per-timestep path (exact-fp32 MFMA tiles, gate GEMVs up to B = 4), which is FASTER at those sizes than 64 padded
 * rows (measured: profiles/round5_ragged_batches.txt). */
int32_t s2vt_padded_batch(int32_t B);

/* Bytes of workspace s2vt_train_forward/backward need (saved activations + scratch). */
size_t s2vt_train_workspace_bytes(const s2vt_dims* d);

/* S2VT.forward(feats, targets, mode='train')  (S2VTModel.py:48-54, 63-81; called at train.py:120,142).
 *   feats   [B, L, F]; targets int64 [B, L-1] with row stride targets_ld (= caption[:, :-1]);
 *   logits  [B, L-1, V] out.  The workspace then holds what s2vt_train_backward needs. */
int s2vt_train_forward(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets,
                       int64_t targets_ld, float* logits, void* workspace, size_t workspace_bytes, void* stream);

/* The same with out_dropout > 0 (S2VTModel.py:25,79: `res = self.out_drop(res)` between word_rnn and out_linear in
 * training mode).  out_mask: [(L-1)*B, H] TIME-MAJOR (row j*B + b = caption step j of sample b), entries 0 or 1/(1-p),
 * drawn by the caller (torch's dropout on a ones tensor: the reference's RNG stream); the backward must get the same mask. */
int s2vt_train_forward_dropout(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets,
                               int64_t targets_ld, const float* out_mask, float* logits, void* workspace,
                               size_t workspace_bytes, void* stream);

/* mode='train' on K captions per clip with ONE encode per clip (not in the reference; additive, ABI 9).
 *   feats [B, L, F]; targets int64 [B, K, L-1] at b * stride_b + k * stride_k + j (either stride may be 0: an expanded view);
 *   logits [B, K, L-1, V] out = those of s2vt_train_forward on the clips repeated K times, row r = b * K + k.
 *   out_mask: NULL, or the out_drop mask [(L-1)*B*K, H] TIME-MAJOR (row j*B*K + r), entries 0 or 1/(1-p); the backward gets the same.
 * The backward writes the 13 parameter gradients of that repeated call and, if dfeats != NULL, dfeats [B, L, F] = the repeated
 * call's dfeats summed over each clip's K rows; K is the forward's.  The feature projection, vid_rnn and word_rnn's L encode steps
 * run once per clip in both directions; the gradients arriving at them are summed over a clip's K rows in a fixed order
 * (s2vt_group_sum_rows), so a step is bitwise reproducible.  Launches per timestep on the fp32-input MFMA in every gemm mode.
 * Workspace, errors and gradient-group events (s2vt_backward_wait_grads) as for s2vt_train_forward / s2vt_train_backward: a target id
 * outside [0, V) is clamped and reported as S2VT_ERR_INDEX by s2vt_check_async_error / the next call; a backward on a workspace no
 * grouped forward filled, or a second backward on one forward, is refused.  Shapes whose row or element counts overflow what the
 * GEMMs index are refused on the host (S2VT_ERR_ARG; the size query returns 0 for them, for invalid dims and for K < 1). */
size_t s2vt_train_group_workspace_bytes(const s2vt_dims* d, int32_t K);
int s2vt_train_group_forward(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t stride_b,
                             int64_t stride_k, int32_t K, const float* out_mask, float* logits, void* workspace, size_t workspace_bytes,
                             void* stream);
int s2vt_train_group_backward(const s2vt_dims* d, const s2vt_params* p, const float* feats, const float* dlogits, const float* out_mask,
                              const s2vt_grads* g, float* dfeats, void* workspace, size_t workspace_bytes, void* stream);

/* Device-side errors are asynchronous: a target id outside [0, V) (the reference's nn.Embedding raises IndexError,
 * S2VTModel.py:71) or a timed-out hand-off of the persistent recurrence raise a flag that every s2vt_train_forward
 * copies to the host at its end.  The NEXT s2vt_train_forward / s2vt_train_backward that finds the copy complete returns
 * S2VT_ERR_INDEX / S2VT_ERR_TIMEOUT for it; a caller that has just synchronised the stream (loss.item()) calls this with
 * wait = 1 and gets the error of the forward it has just run.  0 = no error (or, with wait = 0, not known yet). */
int s2vt_check_async_error(int32_t wait);

/* One depth of the batched beam search (beam.py; S2VTModel.py:205-223 for every expandable node of every sample at once):
 *   1. one zero-input vid_rnn step for the whole batch: (vid_h_in, vid_c_in) [B,H] -> (vid_h_out, vid_c_out);
 *   2. for the R expandable rows r (sample row_b[r], parent state row row_state[r] of the previous depth's table,
 *      last token tok[r]): word_rnn step on [Emb[tok] | vid_h_out[row_b]] from (word_h_in, word_c_in)[row_state] ->
 *      the new state table (word_h_out, word_c_out) [R,H];
 *   3. out_linear, log_softmax and the 20 most probable tokens of every row in ASCENDING token order (the order the
 *      reference pushes them): top_ix [R,20] int32, top_lp [R,20] fp32 log-probs.
 * d->B = batch size; R may be 0 (only the vid step runs).  Workspace: s2vt_beam_workspace_bytes(d, max R). */
size_t s2vt_beam_workspace_bytes(const s2vt_dims* d, int32_t max_rows);
int s2vt_beam_step(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                   const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                   const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out, int32_t* top_ix,
                   float* top_lp, void* workspace, size_t workspace_bytes, void* stream);
/* The same depth with the weight-derived images of a greedy decode of the SAME weights (`cache` as filled by
 * s2vt_greedy_decode_cached: plane images of W_v / W_o, the per-token gate table): vid_out's half of the gate input once per sample,
 * the embedded word from the table, out_linear in split precision on the bf16 matrix cores.  Results as s2vt_beam_step to fp32
 * rounding (the fixtures' beam ids are unchanged). */
int s2vt_beam_step_cached(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out, int32_t* top_ix,
                          float* top_lp, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, void* stream);

/* The reference's per-sample priority queues of the beam search (S2VTModel.py:186-238) ON THE DEVICE, all samples of the batch in one
 * launch per depth: heapq's own sift-down / sift-up replayed per sample (one lane each, heap in LDS), so that the pop order - also
 * among EQUAL scores, where it depends on the binary heap's layout - is the reference's.  `state`: s2vt_beam_queue_bytes() of
 * caller-owned device memory that lives for one search.  Rows of the batched step are fixed: r = b * beam_width + slot.
 *   depth = 1          : initialise, pop the roots; writes row_b / row_state / row_tok for the first s2vt_beam_step
 *   depth = 2..max     : push the children of the depth just stepped (top_ix / top_lp [B*beam_width][20] of s2vt_beam_step), record
 *                        each sample's best entry, freeze samples whose queue holds <= beam_width entries (:227-228), pop the next
 *                        beam (queue cleared, finished entries re-inserted: :190-202) and write the rows of the next step
 *   depth = 0          : the final push (nothing is popped any more)
 * A frozen sample's slots carry token 0 / state row 0 (their step results are ignored).  The int32 at byte 0 of `state` counts the
 * frozen samples (== B: the reference's loop would stop; further calls change nothing).
 * s2vt_beam_queue_result: back-trace of every sample's best entry (:231-236) -> out_tokens[b][0..out_len[b]) = <sos> .. last word. */
size_t s2vt_beam_queue_bytes(int32_t B, int32_t beam_width, int32_t max_depth);
int s2vt_beam_queue_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, int32_t depth, void* state,
                         size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b, int32_t* row_state,
                         int32_t* row_tok, void* stream);
int s2vt_beam_queue_result(int32_t B, int32_t beam_width, int32_t max_depth, void* state, size_t state_bytes, int32_t* out_tokens,
                           int32_t out_cap, int32_t* out_len, void* stream);

/* Cumulative-score beam search (S2VT.forward(mode='beam'); not in the reference): the search policy ON THE DEVICE on the same fixed
 * rows r = b * beam_width + slot, one wave per sample and depth.  A hypothesis scores S = the fp32 sum of its tokens' log-probs (each
 * clamped to <= 0); per depth t the min(beam_width, count) best of the candidates S_j + top_lp[j][f] by (S descending, slot ascending,
 * token ascending) are kept: one ending in <eos> enters the sample's pool with score S / t**length_alpha, the others are the next
 * live slots in that order; at t = max_depth the live ones enter the pool with S / max_depth**length_alpha and no <eos>.  The pool
 * keeps its best beam_width entries by (score descending, insertion ascending).  t**alpha is fp32(double pow), as len**0.7 above.
 * 1 <= beam_width <= 8 (the fan-out of 20 is then exact), length_alpha finite and >= 0.  `state`: s2vt_beam_cum_bytes() of
 * caller-owned device memory that lives for one search.
 *   depth = 1          : initialise; writes row_b / row_state / row_tok for the first s2vt_beam_step
 *   depth = 2..max     : consume top_ix / top_lp [B*beam_width][20] of step depth-1 and write the rows of the next step
 *   depth = 0          : consume the last step, max_depth (a search that stops early may call it as well: frozen samples ignore it)
 * A sample is frozen when no live slot is left, at max_depth, or as soon as its pool is full and pool[beam_width-1].score >=
 * live[0].S / max_depth**alpha (no later hypothesis can enter: scores only fall and ties lose by insertion order).  A frozen sample's
 * slots carry token 0 / state row 0.  The int32 at byte 0 of `state` counts the frozen samples.
 * s2vt_beam_cum_result: the pool's first n_best entries (1 <= n_best <= beam_width) -> out_tokens [B][n_best][max_depth] int32 (words
 * after <sos>, padded with eos_ix), out_len [B][n_best] (tokens, <eos> included where present), out_score [B][n_best], best first. */
size_t s2vt_beam_cum_bytes(int32_t B, int32_t beam_width, int32_t max_depth);
int s2vt_beam_cum_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, double length_alpha, int32_t depth,
                       void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b, int32_t* row_state,
                       int32_t* row_tok, void* stream);
int s2vt_beam_cum_result(int32_t B, int32_t beam_width, int32_t max_depth, int32_t eos_ix, int32_t n_best, void* state, size_t state_bytes,
                         int32_t* out_tokens, int32_t* out_len, float* out_score, void* stream);

/* Caption scoring (S2VT.forward(mode='score'); not in the reference): the log-likelihood of GIVEN captions, K candidates per clip, in
 * the arithmetic of mode='train' without dropout.  A caption c[0..T-1] (2 <= T <= L) is <sos>, words, <eos>, padding, as the data
 * loader lays it out (dataloader.py); candidate k of clip b starts at captions + b * stride_b + k * stride_k (unit token stride;
 * either stride may be 0 - a broadcast view - nothing is copied).  Row r = b * K + k:
 *   n        = 1 + the position of the first eos_ix in c[1:], T-1 where there is none (the <eos> counts, as in s2vt_beam_cum_result)
 *   lp[j]    = min(log_softmax(z_j)[c[j+1]], 0) for j < n, 0 behind; z_j = row j of the logits s2vt_train_forward gives for c[:-1]
 *              (S2VTModel.py:63-81; the log_softmax of :214, clamped as s2vt_beam_cum_step clamps it)     -> token_lp [B*K][T-1]
 *   score    = (fp32 sum of lp[0..n-1], j ascending) / fp32(pow((double)n, length_alpha)), s2vt_beam_cum_step's power rule
 *   length   = n (int64)
 * The K candidates of a clip share ONE encode of it (feature projection, both layers over the L frames, vid_rnn's input-free decode
 * steps: S2VTModel.py:54, 64-67); then T-1 word steps over the B*K rows (the step of s2vt_beam_step), out_linear (:80) over all
 * steps' hidden states in chunks of S2VT_SCORE_HEAD_ROWS rows - the workspace never holds more logits than that - and one finisher
 * launch.  Every id of `captions`, also behind the first <eos>, must lie in [0, V): another one is reported as S2VT_ERR_INDEX through
 * s2vt_check_async_error, as nn.Embedding's IndexError (:71), and is clamped before it indexes anything.
 * cache == NULL: the fp32-input MFMA path, launches per timestep.  Otherwise the plane path on the weight images of
 * s2vt_greedy_decode_cached (same cache, same cache_valid protocol: 0 = the images are built by this call) with the encode phase of
 * s2vt_decode_encode_cached, which refuses (S2VT_ERR_ARG, nothing enqueued) shapes and modes without the persistent recurrence -
 * s2vt_decode_plan(d, 1, ...) tells.  Stream-ordered on `stream`, no host round trip.
 * The workspace holds what the word steps, the head and the finisher work on.  The encode phase's own scratch (a decode workspace,
 * s2vt_decode_workspace_bytes, dead once the states are handed out and several times larger than all the rest) is not in it: the
 * library keeps one such buffer per (device, stream) and grows it on demand - the only calls that allocate, and that wait for the
 * device, are the ones that grow it.
 * s2vt_score_workspace_bytes: 0 where the shape cannot be served (K < 1, T outside [2, L], 2^31 or more token rows). */
#define S2VT_SCORE_HEAD_ROWS 1024
size_t s2vt_score_workspace_bytes(const s2vt_dims* d, int32_t K, int32_t T);
int s2vt_score_captions(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* captions, int64_t stride_b,
                        int64_t stride_k, int32_t K, int32_t T, int32_t eos_ix, double length_alpha, float* token_lp, float* score,
                        int64_t* length, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                        void* stream);
/* The head kernel of the above alone: lp_out[r] = min(x[target[r]] - max(x) - logf(sum_i expf(x[i] - max(x))), 0) for the rows
 * x = logits + r * ld (ld >= V), i.e. log_softmax (S2VTModel.py:214) read at one token.  One workgroup per row, any V.  A target
 * outside [0, V) sets *err_flag (device int32, may be NULL) to non-zero and reads the nearest valid column. */
int s2vt_pick_logprob(const float* logits, int64_t ld, int64_t rows, int32_t V, const int32_t* target, float* lp_out, int32_t* err_flag,
                      void* stream);

/* Data-parallel overlap (no reference counterpart: the reference is single-device).  After s2vt_train_backward has
 * RETURNED (all of its work is enqueued), make `stream` wait until a group of that call's parameter gradients is
 * final, so that their all-reduce can run under the rest of the backward:
 *   group 0 = out_linear.weight, out_linear.bias: final ~1 ms into the backward (behind the last persistent BPTT launch
 *             where the schedule has one);
 *   group 1 = word_rnn.weight_ih, weight_hh, bias_ih, bias_hh + embedding.weight: final before the vid_rnn / feat_linear
 *             weight-gradient GEMMs.
 * The promise: every write to a group's tensors that the backward enqueues, on the caller's stream and on the side lane
 * alike, is ordered before the group's event - the values `stream` sees once the wait completes are the final gradients bit
 * for bit, under every schedule and option (tests/test_gpu_grad_release.py).  The remaining gradients (vid_rnn, feat_linear)
 * are final when the backward's own stream is. */
int s2vt_backward_wait_grads(int32_t group, void* stream);
/* Order check of that overlap for the last s2vt_train_backward of the plane drivers: how many persistent BPTT launches it
 * enqueued, and how many of them were already enqueued when gradient group 0's event was recorded for the last time.  The two
 * must be equal: a persistent launch needs all of its workgroups resident, so no collective may be released beside one (the
 * out_linear all-reduce then overlaps the weight-gradient GEMMs behind the recurrence instead). */
int s2vt_backward_order(int32_t* persistent_bptt_launches, int32_t* group0_recorded_after);

/* Autograd of the above (loss.backward(), train.py:124) given dlogits [B, L-1, V] (contiguous).
 * dfeats [B, L, F] may be NULL (nothing reads it in the reference: SURVEY.md §3.1 note). */
int s2vt_train_backward(const s2vt_dims* d, const s2vt_params* p, const float* feats, const float* dlogits,
                        const s2vt_grads* g, float* dfeats, void* workspace, size_t workspace_bytes, void* stream);
int s2vt_train_backward_dropout(const s2vt_dims* d, const s2vt_params* p, const float* feats, const float* dlogits,
                                const float* out_mask, const s2vt_grads* g, float* dfeats, void* workspace,
                                size_t workspace_bytes, void* stream);

size_t s2vt_decode_workspace_bytes(const s2vt_dims* d);

/* S2VT.forward(feats, mode='test')  (S2VTModel.py:82-110; called at eval.py:52): greedy decode,
 * ids int64 [B, L-1] out, never stops at <eos>, lowest index wins argmax ties. */
int s2vt_greedy_decode(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, int64_t* ids,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The same decode with the WEIGHT-derived images kept across calls (eval.py:48-52 calls model(feats, mode='test') once per batch
 * with fixed weights): plane images of W_f / W_ih1 / W_v / W_o and the per-token gate-input table Emb·W_e^T live in `cache`
 * (s2vt_decode_cache_bytes; caller-owned device memory that outlives the call).  cache_valid == 0: this call fills the cache;
 * != 0: the caller vouches that the parameters, dims and library modes are those of the call that filled it (the Python binding
 * keys on every parameter's data pointer and version counter) and the call reuses it - 0.65 ms less of a 9.2-ms decode at
 * B = 128.  Calls that share a cache must be ordered by the stream.  The per-call workspace is s2vt_decode_workspace_bytes as
 * for s2vt_greedy_decode (whose weight images live behind the per-call part of that workspace and are rebuilt every call). */
size_t s2vt_decode_cache_bytes(const s2vt_dims* d);
/* 1 if s2vt_greedy_decode_cached reads (and, with cache_valid == 0, fills) the cache for this batch size in the current mode;
 * 0 for the batches that decode on the launch-per-timestep path (gemm mode 0, or fewer than 24 clips: measured faster there than
 * 64 padded rows on the plane path) - the caller must then not mark its cache as filled. */
int32_t s2vt_decode_uses_cache(const s2vt_dims* d);
int s2vt_greedy_decode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, int64_t* ids,
                              void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                              void* stream);

/* optimizer.step() of the reference's loop (train.py:89-93,126: torch.optim.Adam, default betas / eps, no weight decay, no
 * amsgrad) as ONE launch over flat fp32 buffers of n elements - every parameter, its gradient and its two moments at the same
 * offsets (s2vt-video-caption_amd/optim.py lays a model's parameters out that way).  torch's arithmetic operation for operation:
 * m += (g - m)(1 - beta1); v = beta2 v + (1 - beta2) g g; p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).
 * step counts from 1; the hyper-parameters are doubles because torch forms 1 - beta and the bias corrections from the Python doubles
 * before rounding to fp32 once. */
int s2vt_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                   double eps, int64_t step, void* stream);

/* ---------------------------------------------------------------- clipped step: global-norm clipping, weight decay, non-finite skip
 * (optim.FlatAdam(max_grad_norm=, weight_decay=, decoupled=, no_decay=, skip_nonfinite=); csrc/optim.hip; restated in numpy by
 * tests/optim_ref.step_ref).  s2vt_adam_step above is unchanged and is what FlatAdam launches at its defaults; these two entry
 * points stand beside it.  For flat buffers of n elements (the layout of s2vt_adam_step), gradients g, max_norm = c:
 *   1. norm     S = sum of (double)g_i * (double)g_i in fp64 (an fp32 square is exact there); grad_norm = fp32(sqrt(S)).  The order is
 *               fixed: the chunk [w C, min((w+1) C, n)) with C = S2VT_GRAD_NORM_CHUNK gives one fp64 partial (per thread in ascending
 *               element order, wave butterfly, (w0 + w1) + (w2 + w3)), written to the workspace by a plain store; a second launch of
 *               ONE workgroup sums the partials in the same manner.  The number of partials depends on n alone.  No floating-point
 *               atomics, no ticket, no cooperative launch, no wait across workgroups: the launch boundary is the synchronisation, and
 *               the same gradients give the same record bits on every call.  A 4-byte-aligned `grads` that is not 16-byte aligned is
 *               loaded element by element and gives the same bits.
 *   2. record   scale = 1 if c <= 0 (no clipping), else coef = fp32(c) / (grad_norm + 1e-6f) and scale = coef >= 1 ? 1 : coef, all
 *               in fp32 - the rule of torch.nn.utils.clip_grad_norm_ (a NaN coef stays NaN, as torch.clamp leaves it).
 *               nonfinite = !isfinite(grad_norm): an inf or NaN gradient, or a norm above fp32's range.
 *               skipped_total += nonfinite if skip_nonfinite (the caller zeroes the record ONCE; the library only ever adds).
 *   3. step     if skip_nonfinite and record.nonfinite: nothing is written, params / exp_avg / exp_avg_sq keep their bits.  Otherwise
 *               per element, every product and sum rounded to fp32 on its own:
 *                 g' = g * scale
 *                 coupled decay   (decoupled == 0, torch.optim.Adam(weight_decay=)):  g' = g' + fp32(wd) * p   where the element's
 *                                 segment is decayed
 *                 decoupled decay (decoupled != 0, torch.optim.AdamW):  p = p * f, f = fp32(1.0 - lr * wd) formed in double on the
 *                                 host, where the element's segment is decayed
 *                 then the update of s2vt_adam_step on (p, g', m, v) - the two kernels compile one expression, so a step at scale 1
 *                 without decay is s2vt_adam_step bit for bit.
 *               Segments: seg_end[0 .. n_seg) ascending with seg_end[n_seg - 1] == n, segment k = [seg_end[k-1], seg_end[k]), decayed iff
 *               seg_decay[k] != 0; n_seg == 0: one segment, decayed.  Ends need not be multiples of 4: every element takes its own
 *               segment's flag.  One wd and one f for all decayed segments; wd == 0 decays nothing.  seg_end / seg_decay are HOST
 *               arrays, copied into the launch arguments (at most S2VT_ADAM_MAX_SEGMENTS).
 * THE CLIPPED GRADIENT IS NOT WRITTEN BACK: `grads` keeps the unclipped gradient (4 bytes per parameter per step saved; the norm and
 * the scale are on the record).  A SKIPPED STEP STILL COUNTS AS A STEP: the bias corrections are formed on the host from `step`, as in
 * s2vt_adam_step, and the host does not learn of a skip without reading the record - so the caller advances `step` regardless.
 * `record`: an s2vt_clip_record in device memory, 16-byte aligned.  s2vt_adam_step_clipped reads scale and nonfinite from it ON
 * THE DEVICE (no host round trip: norm + step are three launches); record == NULL there means scale 1 and needs skip_nonfinite == 0
 * (weight decay alone needs no norm).  `workspace`: s2vt_grad_norm_workspace_bytes(n) bytes of device memory, 8-byte aligned
 * (0 for n <= 0).
 * Checked on the host before anything is enqueued (S2VT_ERR_ARG; s2vt_last_error names the rule): n > 0; null buffers; params /
 * grads / moments not 16-byte aligned (s2vt_grad_norm: grads not 4-byte aligned); record null or not 16-byte aligned; step < 1;
 * weight_decay negative or not finite; n_seg outside [0, 16]; segment ends not ascending or not ending at n; max_norm NaN or -inf
 * (any max_norm <= 0 otherwise means no clipping); a workspace that is null or too small. */
#define S2VT_GRAD_NORM_CHUNK 16384
#define S2VT_ADAM_MAX_SEGMENTS 16
typedef struct s2vt_clip_record {
    float grad_norm;       /* fp32(sqrt(sum of squares in fp64)) of the last s2vt_grad_norm */
    float scale;           /* what s2vt_adam_step_clipped multiplies every gradient with */
    int32_t nonfinite;     /* 1: grad_norm is inf or NaN */
    int32_t pad;
    int64_t skipped_total; /* calls with skip_nonfinite != 0 that found nonfinite == 1 */
} s2vt_clip_record;
size_t s2vt_grad_norm_workspace_bytes(int64_t n);
int s2vt_grad_norm(const float* grads, int64_t n, double max_norm, int32_t skip_nonfinite, void* workspace, size_t workspace_bytes,
                   void* record, void* stream);
int s2vt_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                           double beta2, double eps, int64_t step, double weight_decay, int32_t decoupled, const int64_t* seg_end,
                           const int32_t* seg_decay, int32_t n_seg, int32_t skip_nonfinite, const void* record, void* stream);

/* MaskCriterion's inner nn.CrossEntropyLoss() (utils.py:11,22): mean CE of logits [B, L-1, V] against
 * target[:, 1:] (target int64 [B, L], row stride target_ld).  lse [B*(L-1)] and rowloss [B*(L-1)] are
 * caller-provided scratch (lse is consumed by the backward); loss_out is one device float.
 * A target id outside [0, V) (nn.CrossEntropyLoss raises IndexError; ignore_index is not used by the reference) is
 * detected on the device and reported as S2VT_ERR_INDEX by s2vt_check_async_error / the next call, like the
 * embedding's check in s2vt_train_forward; the row's loss is then computed against the clamped id. */
int s2vt_mean_ce_forward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target,
                         int64_t target_ld, float* lse, float* rowloss, float* loss_out, void* stream);
/* dlogits = (softmax(logits) - onehot(target)) * gout[0] / (B*(L-1)); gout is a device scalar. */
int s2vt_mean_ce_backward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target,
                          int64_t target_ld, const float* lse, const float* gout, float* dlogits, void* stream);

/* MaskCriterion.forward as a whole (utils.py:13-26; called at train.py:122,143): the mean CE above, then
 * `loss = sum(mean_ce * w) / sum(w)` with w = mask[:, 1:] (mask fp32 [B, L], row stride mask_ld), product by product as the
 * reference evaluates it (NaN for an all-zero mask).  out3 = {loss, mean_ce, sum(w)} (three device floats). */
int s2vt_mask_criterion_forward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target, int64_t target_ld,
                                const float* mask, int64_t mask_ld, float* lse, float* rowloss, float* out3, void* stream);
/* autograd of those lines: g_ce[0] = sum_i (gout[0] / out3[2]) * w_i, the `gout` of s2vt_mean_ce_backward / _fused. */
int s2vt_mask_criterion_backward(int32_t B, int32_t Lm1, const float* mask, int64_t mask_ld, const float* out3, const float* gout,
                                 float* g_ce, void* stream);

/* Reward-weighted CE (utils.RewardCriterion; sequence-level training on sampled captions):
 *     loss = sum_i w_i * (lse_i - logit_i[target_i]) / norm,     norm = max(number of i with w_i != 0, 1)
 * over the B*(L-1) rows, w = weight[:, 1:] (fp32 [B, L], row stride weight_ld, read like the mask above; any sign).  The
 * normaliser is the number of tokens that carry a weight - with a 0/1 mask the masked mean, with self-critical advantages the mean
 * over the sampled tokens up to <eos> - and an all-zero weight gives 0, not NaN.  out2 = {loss, norm} (two device floats); lse and
 * rowloss as for s2vt_mean_ce_forward; target ids outside [0, V) are reported as S2VT_ERR_INDEX the same way.  Fixed summation
 * order.  No gradient flows to the weight. */
int s2vt_weighted_ce_forward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target, int64_t target_ld,
                             const float* weight, int64_t weight_ld, float* lse, float* rowloss, float* out2, void* stream);
/* dlogits_i = w_i * (softmax(logits_i) - onehot(target_i)) * gout[0] / out2[1]  (rows with w_i == 0: zeros). */
int s2vt_weighted_ce_backward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target, int64_t target_ld,
                              const float* weight, int64_t weight_ld, const float* lse, const float* out2, const float* gout,
                              float* dlogits, void* stream);

/* ---------------------------------------------------------------- self-critical rewards on the device (train.py --sc-reward device)
 * The reference side of CIDEr (caption_metrics.cider_vector / cider_of_vectors over token ids) as flat device arrays, built once
 * per run by self_critical.DeviceCiderRewarder.  An n-gram KEY is exact: up to four tokens of 16 bits each in a uint64, the first
 * token in bits 63..48, an absent position 0 (a real token is never 0: the pad id is stripped), so the number of non-zero fields
 * is the order.  Every fp64 factor that needs log / exp is precomputed by the host with caption_metrics' own expressions; the
 * device only adds, multiplies, divides, takes sqrt and min.
 *   idf_keys / idf_vals [n_idf]  every n-gram of the training references, keys ascending, value log_n - log(max(1, df)); a key
 *                                that is absent has idf = log_n
 *   clip_ref_off [n_clips + 1]   CSR: the references of clip c are clip_ref_off[c] .. clip_ref_off[c+1] - 1 (at least one each)
 *   ent_off [4*n_refs + 1]       CSR: the (key, tf*idf) entries of reference r, order k = 1..4, are ent_off[4r + k-1] ..
 *                                ent_off[4r + k] - 1 of ent_keys / ent_w, keys strictly ascending inside one (r, k)
 *   ref_norm [4*n_refs]          cider_vector's norm of reference r, order k at [4r + k-1];  ref_len [n_refs] its length (bigrams)
 *   pen [n_pen]                  pen[d] = e ** (-(d*d) / (2 sigma**2)), d = |candidate length - reference length|; n_pen covers
 *                                every reference length and S2VT_CIDER_MAX_T */
#define S2VT_CIDER_MAX_T 512       /* longest id row s2vt_cider_rewards takes (its n-gram list lives in LDS) */
typedef struct s2vt_cider_table {
    const uint64_t* idf_keys; const double* idf_vals;
    const int32_t* clip_ref_off; const int32_t* ent_off;
    const uint64_t* ent_keys; const double* ent_w;
    const double* ref_norm; const int32_t* ref_len;
    const double* pen;
    double log_n;
    int64_t n_idf;
    int32_t n_clips, n_refs, n_pen;
} s2vt_cider_table;
/* out[b] (fp64) = CiderRewarder.score(clip clip_rows[b], ids[b]) for the B rows of ids (int64 [B, T], row stride ld): the row is
 * stripped like self_critical.strip_caption (a leading sos dropped, pads dropped, cut at the first eos), its 1..4-grams are sorted
 * and counted in LDS, weighted with their idf, and compared with every reference of the clip (clipped product min(w_h, w_r) * w_r
 * per order, divided by the norms where both are non-zero, length penalty, mean over orders and references, x10).  One workgroup
 * per row, every sum in a fixed order, no floating-point atomics: a row's value does not depend on the rest of the batch.
 * `table` is a HOST struct of device pointers; clip_rows int32 [B] on the device.  T > S2VT_CIDER_MAX_T is refused (S2VT_ERR_ARG).
 * A token outside [0, 65535] among those the scorer reads (before the first eos) or a clip row outside [0, n_clips) is never
 * used as an index: the row scores without it (0 for a bad clip row) and the call is reported as S2VT_ERR_INDEX by
 * s2vt_check_async_error / a later call. */
int s2vt_cider_rewards(const s2vt_cider_table* table, const int32_t* clip_rows, const int64_t* ids, int32_t B, int32_t T, int64_t ld,
                       int32_t sos, int32_t eos, double* out, void* stream);
/* Consensus (minimum-Bayes-risk) selection among the K candidate captions of each of B clips: ids int64 [B*K, T], rows r = b*K + k
 * with row stride ld >= T; valid uint8 [B*K] or NULL (every candidate valid).  With words_k = strip_caption(row k) and vec_k =
 * cider_vector(ngrams(words_k, 4), df, log_n) - df / log_n of the table's training split; the clips themselves need not be in it -
 * and Vb the valid candidates of clip b:
 *   utility[b*K + i] = cider_of_vectors(vec_i, [vec_j for j ascending, j in Vb, j != i], 4, sigma)   for i in Vb (0.0 when i is alone)
 *                    = -inf                                                                           for i not in Vb
 *   best[b]          = the smallest i in Vb whose utility is the maximum, 0 when Vb is empty
 * i.e. CIDEr-D of candidate i with the other candidates as its references: the clipped product min(w_i, w_j) * w_j per order, divided
 * by both norms where both are non-zero, times the length penalty pen[|bigrams_i - bigrams_j|], the pairs' terms added in ascending j
 * from 0.0 per order, mean over the orders and the others, x10.  A candidate without words has all norms zero and utility 0.0.
 * fp64 in a fixed order, no floating-point atomics: a clip's result does not depend on the rest of the batch, and the same inputs
 * give the same bits on every call.  Of the table only idf_keys, idf_vals, n_idf, log_n, pen and n_pen are read.
 * 1 <= K <= S2VT_CONSENSUS_MAX_K, 1 <= T <= S2VT_CIDER_MAX_T; null pointers, bad dims, a workspace below
 * s2vt_cider_consensus_workspace_bytes(B, K, T) (0 for bad dims) or an incomplete table: S2VT_ERR_ARG before any launch.  A row that
 * is not valid is not read.  A token outside [0, 65535] before the first eos of a valid row is never used as an index: the row is
 * scored without it and the call is reported as S2VT_ERR_INDEX by s2vt_check_async_error / a later call, as for s2vt_cider_rewards;
 * other clips are untouched.  Three launches: the candidate phase of s2vt_cider_rewards per row into the workspace's slots, one
 * workgroup per (clip, candidate) over the pairs, one wavefront per clip for the arg-max. */
#define S2VT_CONSENSUS_MAX_K 64
size_t s2vt_cider_consensus_workspace_bytes(int32_t B, int32_t K, int32_t T);
int s2vt_cider_consensus(const s2vt_cider_table* table, const int64_t* ids, int32_t B, int32_t K, int32_t T, int64_t ld,
                         int32_t sos, int32_t eos, const uint8_t* valid, double* utility, int32_t* best,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Sentence BLEU-4 beside CIDEr (train.py --sc-bleu-weight, eval.py --consensus-bleu-weight): the per-sentence BLEU_4 of
 * caption_metrics.bleu over token ids, with sqrt(sqrt(prod)) for prod ** 0.25 (sqrt is correctly rounded on host and device, pow is
 * not).  In fp64, with c = the number of words of the stripped row (strip_caption) and the clip's references:
 *   tf(g) = count of n-gram g in the row, rmax(g) = max over the references of g's count there,
 *   match_k = sum over the distinct g of order k of min(tf(g), rmax(g)), k = 1..4 (integers, exact in any order),
 *   guess_k = max(0, c - (k-1)),   rl = the reference length in WORDS closest to c, ties to the shorter,
 *   f_k = (match_k + 1e-15) / (guess_k + 1e-9),   prod = (((1.0 * f_1) * f_2) * f_3) * f_4,
 *   bleu4 = sqrt(sqrt(prod)) * bp[c][rl],   bp[c][rl] = exp(1 - 1/ratio) if ratio < 1 else 1.0, ratio = (c + 1e-15) / (rl + 1e-9).
 * bp needs exp and comes from the host (math.exp), row-major [S2VT_CIDER_MAX_T + 1][n_rl] with n_rl > max(S2VT_CIDER_MAX_T, longest
 * reference); an empty row scores exactly 0.0 (bp[0][*] = 0).  The mixed reward is w_cider * cider + w_bleu * bleu4: two products and
 * one add, not contracted.  The table, built once by self_critical.DeviceMixedRewarder beside the CIDEr table of the same clips:
 *   clip_key_off [n_clips + 1]   CSR: the (key, max count) entries of clip c - the union of its references' 1..4-grams, the keys of
 *                                s2vt_cider_table (a key names its own order), strictly ascending inside a clip; max_count >= 1
 *   clip_ref_off [n_clips + 1]   CSR: ref_words [n_refs], the references' lengths in words (s2vt_cider_table.ref_len counts bigrams) */
typedef struct s2vt_bleu_table {
    const int32_t* clip_key_off; const uint64_t* keys; const int32_t* max_count;
    const int32_t* clip_ref_off; const int32_t* ref_words;
    const double* bp;
    int64_t n_keys;
    int32_t n_clips, n_refs, n_rl;
} s2vt_bleu_table;
/* s2vt_cider_rewards with the BLEU-4 of the same rows: out[b] = w_cider * cider + w_bleu * bleu4, and where they are not NULL
 * out_cider[b] / out_bleu[b] the two parts.  One workgroup per row and ONE candidate phase for both scores (the row is stripped and
 * sorted once); the reference phase is s2vt_cider_rewards' own code, so out_cider has its bits.  BLEU works on the sorted keys in
 * LDS: an entry that differs from its predecessor heads a run, the run's length is tf, a binary search in the clip's key range gives
 * rmax; integer sums through wave shuffles, the closest length as a keyed minimum, the fp64 chain on one thread.  No floating-point
 * atomics; a row's value does not depend on the rest of the batch.  Errors as s2vt_cider_rewards: T > S2VT_CIDER_MAX_T, null
 * pointers, an incomplete table, tables of different n_clips or a weight that is not finite: S2VT_ERR_ARG before any launch; a token
 * outside [0, 65535] or a clip row out of range (all three outputs 0.0) is never used as an index and reported as S2VT_ERR_INDEX by
 * s2vt_check_async_error / a later call. */
int s2vt_mixed_rewards(const s2vt_cider_table* table, const s2vt_bleu_table* bleu, const int32_t* clip_rows, const int64_t* ids,
                       int32_t B, int32_t T, int64_t ld, int32_t sos, int32_t eos, double w_cider, double w_bleu, double* out,
                       double* out_cider, double* out_bleu, void* stream);
/* s2vt_cider_consensus with the mixed utility: for i in Vb with at least one other valid candidate
 *   utility[b*K + i] = w_cider * (s2vt_cider_consensus' utility, the same bits) + w_bleu * bleu4(words_i; references = words_j for j
 *                      ascending, j in Vb, j != i),
 * 0.0 when i is alone, -inf for i not in Vb; best as there.  The candidate launch is s2vt_cider_consensus'; the pair launch finds,
 * for every run head of candidate i, the largest run length at the key's lower bound in the slots of the other valid j, and rl among
 * the others' word counts.  Of the BLEU table only bp and n_rl are read.  Same dims, workspace size, errors and launches as
 * s2vt_cider_consensus; a weight that is not finite: S2VT_ERR_ARG. */
size_t s2vt_mixed_consensus_workspace_bytes(int32_t B, int32_t K, int32_t T);
int s2vt_mixed_consensus(const s2vt_cider_table* table, const s2vt_bleu_table* bleu, const int64_t* ids, int32_t B, int32_t K, int32_t T,
                         int64_t ld, int32_t sos, int32_t eos, const uint8_t* valid, double w_cider, double w_bleu, double* utility,
                         int32_t* best, void* workspace, size_t workspace_bytes, void* stream);
/* What the self-critical step feeds the train step (self_critical.advantage_weights and the <sos> column, on the device):
 * caps int64 [B, T+1] = sos || sampled (int64 [B, T], contiguous); weight fp32 [B, T+1] = fp32(r_sample[b] - r_greedy[b]) - the
 * fp64 difference rounded once - on positions 1 .. the first eos of the row inclusive (all T without one), zero elsewhere. */
int s2vt_sc_weights(const int64_t* sampled, const double* r_sample, const double* r_greedy, int32_t B, int32_t T, int32_t sos,
                    int32_t eos, int64_t* caps, float* weight, void* stream);
/* The same for K sampled captions per clip, rows r = b*K + k (sampled int64 [B*K, T], r_sample fp64 [B*K]); one wavefront per clip.
 *   r_greedy == NULL: baseline[b*K + k] = ((sum over j = 0 .. K-1, ascending, from 0.0, of r_sample[b*K + j]) - r_sample[b*K + k])
 *                     / (K - 1) in fp64 - the mean reward of the clip's OTHER samples (Luo 2020).  Needs K >= 2 (S2VT_ERR_ARG).
 *   r_greedy != NULL: baseline[b*K + k] = r_greedy[b] (fp64 [B]); K = 1 is then s2vt_sc_weights.
 * caps int64 [B*K, T+1] = sos || sampled; weight fp32 [B*K, T+1] = fp32(r_sample[r] - baseline[r]), the fp64 difference rounded
 * once, on positions 1 .. the first eos inclusive (all T without one), zero elsewhere; baseline fp64 [B*K] or NULL.  Adds, one
 * subtract, one divide in the stated order: self_critical.group_advantages restates it in numpy bit for bit.  A clip whose K
 * rewards are all equal (r_greedy == NULL) gets weight 0 on every row: its baseline is that reward itself, by comparison - the
 * rounded K-term sum alone would leave a difference of rounding size (at K = 3 for about half of all values), a weight that is
 * not zero.  s2vt_weighted_ce_forward's normaliser counts the tokens that carry a weight, so that clip's tokens are not counted. */
int s2vt_sc_weights_group(const int64_t* sampled, const double* r_sample, const double* r_greedy, int32_t B, int32_t K, int32_t T,
                          int32_t sos, int32_t eos, int64_t* caps, float* weight, double* baseline, void* stream);
/* ---- without-replacement weights
 * The same for the K pairwise distinct captions per clip of one stochastic beam search (S2VT.sample_distinct: sampled int64
 * [B*K, T], logprob fp32 [B*K], kappa fp32 [B]), 2 <= K <= S2VT_SWOR_MAX_K: the normalised importance-weighted REINFORCE estimator
 * with a built-in baseline of Kool, van Hoof, Welling, "Buy 4 REINFORCE Samples, Get a Baseline for Free!" (2019).  A caption with
 * log-prob phi is among the K when its Gumbel(phi) score exceeds kappa: inclusion probability q = 1 - exp(-exp(phi - kappa)).
 * Per clip b, rows i = 0 .. K-1 at r = b*K + i, phi_i = (double)logprob[r], kap = (double)kappa[b], r_i = r_sample[r]; everything in
 * fp64, every sum over ascending i from 0.0, products and sums rounded apart, no atomics:
 *   1. a_i = phi_i - kap (+inf when kap = -inf), e_i = exp(a_i)
 *   2. lq_i = log(-expm1(-e_i)), or a_i - 0.5 * e_i when a_i < -30: log q_i, finite where e_i underflows (at the switch the two
 *      forms differ by about e^2 / 24 < 1e-27); kap = -inf gives lq_i = 0
 *   3. lw_i = phi_i - lq_i, m = max_i lw_i, om_i = exp(lw_i - m), pi_i = exp(phi_i - m): both exponents <= 0, and nothing changes
 *      when phi and kap are shifted together - 79-word captions with phi ~ -700 do not underflow
 *   4. W = sum om_j, N = sum om_j * r_j
 *   5. base = r_greedy[b] (fp64 [B]) when given, else N / W: the importance-weighted estimate of the model's expected reward
 *   6. W_i = (W - om_i) + pi_i, c_i = om_i / W_i, adv_i = c_i * (r_i - base)
 *   7. caps int64 [B*K, T+1] = sos || sampled; weight fp32 [B*K, T+1] = fp32(adv_i), rounded once, on positions 1 .. the first eos
 *      of the row inclusive (all T without one), zero elsewhere: s2vt_sc_weights_group's layout
 * r_greedy == NULL and the K rewards compare equal: every adv_i is exactly 0 and base = r_0 (N / W alone would leave a difference
 * of rounding size; the reason given for s2vt_sc_weights_group).  A clip is BAD when a phi is not finite or positive, kap is NaN or
 * +inf, a reward (r_greedy[b] included) is not finite, or an fp32(adv_i) comes out not finite (rewards beyond fp32's range):
 * weight 0 on all its rows, coef 0, base NaN - no NaN reaches a gradient, and other clips are untouched.
 * coef fp64 [B*K] = c_i or NULL; baseline fp64 [B] = base or NULL.  self_critical.swor_advantages restates it in numpy step for step
 * (libm's exp / expm1 / log against the device's: rtol 1e-10).  One wavefront per clip, every lane walking the same K numbers.  Null
 * pointers, B < 1, T < 1 or K outside [2, S2VT_SWOR_MAX_K]: S2VT_ERR_ARG before any launch. */
#define S2VT_SWOR_MAX_K 8
int s2vt_sc_weights_swor(const int64_t* sampled, const float* logprob, const float* kappa, const double* r_sample,
                         const double* r_greedy, int32_t B, int32_t K, int32_t T, int32_t sos, int32_t eos, int64_t* caps,
                         float* weight, double* coef, double* baseline, void* stream);

/* The same gradient handed to s2vt_train_backward WITHOUT an fp32 dlogits tensor (utils.py:22 under loss.backward(), train.py:124):
 * evaluates (softmax(logits) - onehot(target)) * gout[0] / (B*(L-1)) inside the plane-split pass of the TRAIN workspace the
 * logits came from - the operand planes and bias-gradient partial sums the backward's first kernel would otherwise produce from
 * dlogits, bit for bit - and marks the workspace so that the following s2vt_train_backward may be called with dlogits == NULL.
 * Plane-driver workspaces only (B % 64 == 0, gemm mode 1 or 3); lse from s2vt_mean_ce_forward. */
int s2vt_mean_ce_backward_fused(const s2vt_dims* d, const float* logits, const int64_t* target, int64_t target_ld, const float* lse,
                                const float* gout, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- per-op entry points
 * (the pieces the whole-path drivers are built from; exported for tests, profiling and reuse) */

/* C[M,N] (+)= op(A)·op(B) (+ bias[N]) in fp32 on the matrix cores.
 *   a_kmajor: A stored [M][K] (else [K][M]);  b_kmajor: B stored [N][K] (else [K][N]).
 * Stands for torch's addmm/mm under nn.Linear / nn.LSTM input projections (S2VTModel.py:54,67,77,80). */
int s2vt_gemm_f32(int32_t a_kmajor, int32_t b_kmajor, int32_t M, int32_t N, int32_t K, const float* A, int64_t lda,
                  const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int32_t accumulate,
                  void* stream);

/* Same contraction with caller-provided scratch (`ws`, ws_floats floats) that lets small grids split K into
 * slices combined in a fixed order (deterministic); this is the form the whole-path drivers use. */
int s2vt_gemm_f32_splitk(int32_t a_kmajor, int32_t b_kmajor, int32_t M, int32_t N, int32_t K, const float* A,
                         int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                         int32_t accumulate, float* ws, size_t ws_floats, void* stream);

/* Split-precision path (split.hip, gemm_x3.hip, gemm_bf16.hip).  An fp32 matrix [rows][cols] is rewritten as `nplanes`
 * (1 or 3) bf16 planes p0+p1+p2 = x (24 mantissa bits) of a k-major GEMM operand, zero-filled in k beyond the data
 * (kpad % 64 == 0, ldo >= nplanes*kpad):
 *   nplanes = 1: plain rows, element (r, k) at r*ldo + k;
 *   nplanes = 3: BLOCKED layout of gemm_x3.hip - per 64-row block and 16-wide k chunk one 6-KB record of six 1-KB
 *     pieces (plane, k half) of 64 rows x 8 k:  (r/64)*(64*ldo) + (k/16)*3072 + (pl*2 + (k%16)/8)*512 + (r%64)*8 + k%8
 *     (bf16 units); the buffer must hold whole 64-row blocks: ceil(operand rows / 64) * 64 * ldo elements.
 * transpose = 0: operand rows = input rows, k = input columns; transpose = 1: operand rows = input columns
 * (out_rows_pad >= cols), k = input rows (kpad >= rows). */
int s2vt_split_planes(int32_t nplanes, int32_t transpose, const float* in, int64_t ld, int32_t rows, int32_t cols,
                      uint16_t* out, int64_t ldo, int32_t kpad, int32_t out_rows_pad, void* stream);
/* C[M,N] (+)= A[M,K]·B[N,K]^T (+bias) from bf16 planes (layouts above) on the bf16 matrix cores, fp32 accumulate;
 * K = kpad.  nplanes = 3 sums the six leading plane products (fp32-equivalent, ~2^-23 relative; LDS-DMA kernel,
 * 256x256 tiles); nplanes = 1 is a plain bf16 GEMM.  ws/ws_floats: optional scratch for deterministic split-K. */
int s2vt_gemm_bf16_nt(int32_t nplanes, int32_t M, int32_t N, int32_t K, const uint16_t* A, int64_t lda, const uint16_t* B,
                      int64_t ldb, float* C, int64_t ldc, const float* bias, int32_t accumulate, float* ws,
                      size_t ws_floats, void* stream);
/* The weight-gradient form, C[M,N] (+)= X_A^T · X_B, from the ROW images of its operands: A = blocked 3-plane image (transpose = 0
 * above) of X_A [K rows][M columns], B = that of X_B [K rows][N columns], both starting at a 64-row block; K (a multiple of 64)
 * image rows are contracted.  The kernel reads its fragments transposed (ds_read_b64_tr_b16), so dG / dlogits / h are split ONCE,
 * as rows, and serve both the data-gradient GEMMs (as A[M,K]) and the weight-gradient GEMMs (autograd of S2VTModel.py:54,67,77,80).
 * nplanes = 1: the same from plain bf16 row images (rows of at least M / N columns). */
int s2vt_gemm_bf16_tt(int32_t nplanes, int32_t M, int32_t N, int32_t K, const uint16_t* A, int64_t lda, const uint16_t* B,
                      int64_t ldb, float* C, int64_t ldc, const float* bias, int32_t accumulate, float* ws, size_t ws_floats,
                      void* stream);

/* Test / calibration hook of s2vt_gemm_bf16_nt: force the workgroup tile height (nplanes = 1: 128, 192, 256 or 320 rows; nplanes = 3:
 * 128, 192 or 256; 0 = the launcher's time model picks the height whose tile count fills whole rounds of the compute units) and
 * the split-K factor (0 = model).  Results do not depend on the tile height beyond the order of the fp32 sums along k, which it does not change
 * either (split-K does). */
int s2vt_gemm_tune(int32_t nplanes, int32_t tile_rows, int32_t nsplit);

/* feat_linear (S2VTModel.py:54): x1[l*B+b, :] = feats[b, l, :]·W^T + bias  (time-major output [L*B, H]). */
int s2vt_feat_proj_fwd(const s2vt_dims* d, const float* feats, const float* w, const float* bias, float* x1,
                       void* stream);
/* its weight/bias gradients from dx1 [L*B, H] (time-major); dfeats optional. colsum_ws: >= s2vt_colsum_ws_floats(L*B, H) floats. */
int s2vt_feat_proj_bwd(const s2vt_dims* d, const float* feats, const float* w, const float* dx1, float* dw,
                       float* dbias, float* dfeats, float* colsum_ws, void* stream);
size_t s2vt_colsum_ws_floats(int64_t rows, int32_t cols);

/* ---- per-op entry points, TEST SUPPORT (tests/test_gpu_backward_aux.py): the gather / scatter / reorder pieces of the train
 * backward one at a time, as the whole-path drivers call them.  No kernel of their own.  Each checks its arguments on the host
 * (null pointers, scratch below the *_ws_* size, geometry) and returns S2VT_ERR_ARG with a message before any launch.
 *
 * A row map (idx, inner, outer) names the STORED row of logical row r: idx[r] if idx != NULL (a gather), else
 * (r % inner) * outer + r / inner if inner != 0 (batch-major <-> time-major; inner * outer = the number of mapped rows), else r. */

/* s2vt_gemm_f32_splitk with a row map on the stored rows of A, B and C (the embedding lookup and every batch-major <->
 * time-major reorder of gemm mode 0).  The stored rows of A are m if a_kmajor, else k; those of B are n if b_kmajor, else k; a
 * gather is taken on m / n rows only.  splitk_cap > 0: K is split into at most that many slices (the launcher plans with
 * min(ws_floats, splitk_cap * M * N) floats of scratch); 0: no cap.  Slice s of a split writes ws[s*M*N .. (s+1)*M*N). */
int s2vt_gemm_f32_mapped(int32_t a_kmajor, int32_t b_kmajor, int32_t M, int32_t N, int32_t K, const float* A, int64_t lda,
                         const int32_t* a_idx, int32_t a_inner, int32_t a_outer, const float* B, int64_t ldb, const int32_t* b_idx,
                         int32_t b_inner, int32_t b_outer, float* C, int64_t ldc, const int32_t* c_idx, int32_t c_inner,
                         int32_t c_outer, const float* bias, int32_t accumulate, float* ws, size_t ws_floats, int32_t splitk_cap,
                         void* stream);
/* Embedding gradient (autograd of S2VTModel.py:71): d_emb[v, :] = sum of d_rows[r, :] over the rows with tok[r] == v, in a fixed
 * order; EVERY row of d_emb [V, E] is written (zeros for unused ids).  d_rows [rows, E], tok int32 [rows] with ids in [0, V);
 * ws: >= s2vt_embedding_grad_ws_ints(rows, V) ints, contents irrelevant on entry; on return it holds, for H = rows / 64 + 2,
 * ws[0 .. n) = the ids with more than 64 matches (summed by the many-row kernel; any order), ws[H] = their number n, and
 * ws[H + 1 + v] = the number of rows with tok[r] == v. */
size_t s2vt_embedding_grad_ws_ints(int64_t rows, int32_t V);
int s2vt_embedding_grad(const float* d_rows, int64_t rows, int32_t E, const int32_t* tok, int32_t V, float* d_emb, int32_t* ws,
                        size_t ws_ints, void* stream);
/* out[r, 0:cols] = src[idx[r], 0:cols] (src rows of stride ld, out contiguous); rows <= 65535. */
int s2vt_gather_rows(const float* src, int64_t ld, const int32_t* idx, int64_t rows, int32_t cols, float* out, void* stream);
/* out[g*ld_out + c] = in[(g*K + 0)*ld_in + c] + in[(g*K + 1)*ld_in + c] + ... + in[(g*K + K-1)*ld_in + c] for g < groups, c < cols:
 * fp32 adds in exactly that order, no atomics (bit-reproducible); 16-byte accesses where both row images are 16-byte aligned, any
 * cols >= 1; nothing outside [groups, cols] of out is written; out must not overlap in.  The grouped train backward's sum of a
 * clip's K caption rows (s2vt_train_group_backward: the decode steps' gate gradients, the carried cell gradient). */
int s2vt_group_sum_rows(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t groups, int32_t K, int32_t cols, void* stream);
/* out[cols][rows] = in[rows][cols]^T, both contiguous. */
int s2vt_transpose_f32(const float* in, int32_t rows, int32_t cols, float* out, void* stream);
/* out[c] (+)= sum_r x[r*ld + c] in a fixed order: partial sums over 64-row chunks into ws[chunk*cols + c]
 * (>= s2vt_colsum_ws_floats(rows, cols) floats), then s2vt_colsum_finish over the ceil(rows / 64) chunks. */
int s2vt_colsum(const float* x, int64_t rows, int32_t cols, int64_t ld, float* ws, size_t ws_floats, float* out, int32_t accumulate,
                void* stream);
int s2vt_colsum_finish(const float* partial, int32_t nchunks, int32_t cols, float* out, int32_t accumulate, void* stream);
/* One pass over in [rows][cols] (row stride ld, rows through the row map) that writes any of: out_r, the planes of
 * s2vt_split_planes(transpose = 0) (rows [0, rows) of the image; kpad_r = cols rounded up to 64); out_t, those of transpose = 1
 * (kpad_t = rows rounded up to 64); colpart [ceil(rows / 64)][cols], the column sums of each 64-row chunk (s2vt_colsum's partial
 * sums).  Images as for s2vt_split_planes: 16-byte aligned, whole 64-row blocks, ldo % 8 == 0, ldo >= nplanes * kpad.
 * With lse (then target, gout too; no row map): `in` holds the logits [B*Lm1][cols] and what is split and summed is the mean-CE
 * gradient (exp(in[r][c] - lse[r]) - [c == target[b*target_ld + j + 1]]) * gout[0] / rows of row r = b*Lm1 + j, bit for bit
 * s2vt_mean_ce_backward's.  alpha_out (optional, with lse): only the power of two s2 of the scale gout[0] / rows = alpha * s2,
 * alpha in [1, 2), goes into the planes; alpha is written to alpha_out[0] and colpart holds alpha * (the sums of the planes' values). */
int s2vt_split_planes_dual(int32_t nplanes, const float* in, int64_t ld, const int32_t* idx, int32_t inner, int32_t outer, int32_t rows,
                           int32_t cols, uint16_t* out_r, int64_t ldo_r, int32_t kpad_r, uint16_t* out_t, int64_t ldo_t, int32_t kpad_t,
                           float* colpart, const float* lse, const int64_t* target, int64_t target_ld, int32_t Lm1, const float* gout,
                           float* alpha_out, void* stream);

/* One LSTM timestep, gates i,f,g,o (what nn.LSTM runs per step: S2VTModel.py:67,77,86,93,103):
 *   G = gx (or bias if gx == NULL) + h_prev·W_hh^T ; cell update; writes h_out, c_out and, if stash != NULL,
 *   the activated gates [B,4H] for the backward.  h_prev/c_prev NULL = zero state.  Row stride of every
 *   [B, *] operand = its natural width. */
int s2vt_lstm_step_fwd(int32_t B, int32_t H, const float* gx, const float* bias, const float* w_hh,
                       const float* h_prev, const float* c_prev, float* h_out, float* c_out, float* stash,
                       void* stream);
/* One DECODE step of word_rnn (S2VTModel.py:100-103: embedding of the previous word, concatenated in front of vid_rnn's output,
 * one nn.LSTM step): G = gx + h_prev·W_hh^T + Emb[token(b)]·W_e^T with gx [B,4H] = the vid_out half of the gate input + both
 * biases, emb [V,E], w_e = the first E columns of word_rnn.weight_ih (row stride ldw_e).  token(b) = tok[b] (int32), else the
 * packed argmax word of the previous step (s2vt_decode_step_argmax: 0xFFFFFFFF - low 32 bits), else tok_const for every row.
 * A token id outside [0, V) - nn.Embedding raises IndexError there - is read as token 0 and reported as S2VT_ERR_INDEX by
 * s2vt_check_async_error / the next call: it never addresses memory outside the table. */
int s2vt_lstm_step_fwd_token(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* h_prev,
                             const float* c_prev, const float* emb, const float* w_e, int64_t ldw_e, const int32_t* tok,
                             const unsigned long long* tok_packed, int32_t tok_const, float* h_out, float* c_out, void* stream);

/* ---- the decode step's kernel forms, TEST SUPPORT (tests/test_gpu_decode_forms.py): the forms of the step and arg-max kernels
 * that the greedy / sampled decode drivers and the beam plane-path step run, one launch at a time.  No kernel of their own; each
 * checks its arguments on the host and returns S2VT_ERR_ARG with a message before any launch.  Row strides are the natural widths
 * (gx, stash: 4H; w_hh, h_prev, c_prev, h_out, c_out: H) unless an ld argument says otherwise.
 *
 * s2vt_lstm_step_fwd_table: one word_rnn step in the plane-path form,
 *   G[b] = gx[gx_idx ? gx_idx[b] : b] (or bias if gx == NULL) + gtab[token(b)] + h_prev[b]·W_hh^T ; cell update.
 * gx_idx (optional, only with gx): beam slots that share their sample's gate-input row.  gtab [V][ldtab] (optional, ldtab >= 4H):
 * the per-token gate table Emb·W_e^T; token sources and the out-of-range rule (token 0, S2VT_ERR_INDEX posted) as
 * s2vt_lstm_step_fwd_token.  h_prev / c_prev NULL = zero state.  stash (optional): the activated gates.  h_planes (optional): h_t
 * also as three bf16 planes in the blocked image of s2vt_split_planes(3 planes): hp_rows >= B rounded up to 64 rows of ldhp
 * elements, ldhp >= 3 * (H rounded up to 64), ldhp % 8 == 0, 16-byte aligned; only the elements of (b < B, unit < H) are written.
 * contract_only = 1: the contraction alone, z_out[b][g*H + u] = sum_k h_prev[b][k] W_hh[g*H + u][k] (rows of ldz >= 4H floats);
 * h_prev, w_hh and z_out are required, every other pointer is ignored and nothing else is written.  contract_only = 0: z_out
 * must be NULL. */
int s2vt_lstm_step_fwd_table(int32_t B, int32_t H, int32_t V, const float* gx, const int32_t* gx_idx, const float* bias, const float* gtab,
                             int64_t ldtab, const int32_t* tok, const unsigned long long* tok_packed, int32_t tok_const, const float* w_hh,
                             const float* h_prev, const float* c_prev, float* h_out, float* c_out, float* stash, uint16_t* h_planes,
                             int64_t ldhp, int32_t hp_rows, float* z_out, int64_t ldz, int32_t contract_only, void* stream);
/* The cell update of a step whose contraction ran as its own launch: the step above with z [B][ldz] (ldz >= 4H) in place of
 * h_prev·W_hh^T - the same additions in the same order, so every output has the fused step's bits. */
int s2vt_lstm_cell_pointwise(int32_t B, int32_t H, int32_t V, const float* gx, const int32_t* gx_idx, const float* bias, const float* gtab,
                             int64_t ldtab, const int32_t* tok, const unsigned long long* tok_packed, int32_t tok_const, const float* z,
                             int64_t ldz, const float* c_prev, float* h_out, float* c_out, float* stash, uint16_t* h_planes, int64_t ldhp,
                             int32_t hp_rows, void* stream);
/* The plane-path arg-max launch (csrc/argmax_x3.hip) on caller-made blocked 3-plane images (s2vt_split_planes) of one padded k = K:
 * W [w_rows >= V rounded up to 64][ldw], Hp = h_t [hp_rows >= B rounded up to 64][ldh], packed as for s2vt_decode_step_argmax.
 * M2 > 0: the same launch also writes z[b][m] = h_t[b]·W2[m] for m < M2 (W2 [w2_rows >= M2 rounded up to 64][ldw2], z rows of
 * ldz >= M2 floats, ldz % 4 == 0, 16-byte aligned): nothing of z past column M2 or row B is written.  with_logits = 0: the z role
 * alone (M2 > 0; packed is left as it is).  sample != 0 (with the logits only): the draw of s2vt_decode_step_sample_x3 with the
 * same temperature / seed / step / row0. */
int s2vt_argmax_x3_planes(int32_t B, int32_t V, int32_t K, const uint16_t* W, int64_t ldw, int32_t w_rows, const uint16_t* Hp, int64_t ldh,
                          int32_t kpad_h, int32_t hp_rows, const float* bias, unsigned long long* packed, const uint16_t* W2, int64_t ldw2,
                          int32_t kpad_w2, int32_t w2_rows, int32_t M2, float* z, int64_t ldz, int32_t with_logits, int32_t sample,
                          float temperature, uint64_t seed, int32_t step, int32_t row0, void* stream);

/* BPTT of one step: dh = dh_out + dg_next·W_hh (w_hh_t = W_hh^T [H,4H]); dc (in/out, [B,H]) carries dL/dc;
 * dg [B,4H] out (may alias stash). dg_next NULL at the last step; dc_is_zero = 1 there. */
int s2vt_lstm_step_bwd(int32_t B, int32_t H, const float* dg_next, const float* w_hh_t, const float* dh_out,
                       const float* stash, const float* c, const float* c_prev, float* dc, int32_t dc_is_zero,
                       float* dg, void* stream);

/* A whole layer: T steps from zero state. gx [n_gx*B, 4H] time-major covers steps 0..n_gx-1 (x-part + both
 * biases); later steps see `bias` only (the zero-padded input of S2VTModel.py:64-65).
 * Outputs time-major h_all/c_all [T*B, H], stash [T*B, 4H] (may alias gx). */
int s2vt_lstm_seq_fwd(int32_t T, int32_t B, int32_t H, const float* gx, int32_t n_gx, const float* bias,
                      const float* w_hh, float* h_all, float* c_all, float* stash, void* stream);
/* BPTT over the layer: dh_out [T*B, H] time-major with dh_out rows for steps < dh_first absent (treated as 0);
 * stash is overwritten by dG [T*B,4H]; w_hh_t and dc [B,H] are scratch provided by the caller. */
int s2vt_lstm_seq_bwd(int32_t T, int32_t B, int32_t H, const float* w_hh, const float* dh_out, int32_t dh_first,
                      const float* c_all, float* stash_dg, float* w_hh_t, float* dc, void* stream);

/* ---------------------------------------------------------------- GRU cell (rnn_type='gru')
 * What nn.GRU computes for S2VT(rnn_type='gru') (S2VTModel.py:11-22; torch's gate order r, z, n):
 *   r = sigmoid(gx_r + h W_hr^T + b_hr), z = sigmoid(gx_z + h W_hz^T + b_hz), n = tanh(gx_n + r * (h W_hn^T + b_hn)),
 *   h' = n + z * (h - n), with gx = x W_ih^T + b_ih.  weight_hh [3H,H] and b_hh [3H] are passed as they are; b_hh is added
 * inside the kernels (b_hn belongs inside the r product).  The fp32 fused timestep kernels of csrc/gru.hip (no whole-path
 * driver: the model-level composition is gru_functional.py's).  Row strides are the natural widths. */
/* One step (nn.GRU over one timestep: S2VTModel.py:67 / :77 per step): gx [B,3H] or, if NULL, b_ih alone (a zero input);
 * h_prev NULL = zero state.  stash (optional, [B,4H]) receives r, z, n and ghn = h_prev W_hn^T + b_hn for the backward. */
int s2vt_gru_step_fwd(int32_t B, int32_t H, const float* gx, const float* b_ih, const float* w_hh, const float* b_hh,
                      const float* h_prev, float* h_out, float* stash, void* stream);
/* One DECODE step of word_rnn (S2VTModel.py:100-103 with nn.GRU): gate input gx [B,3H] (vid_out half + b_ih) plus
 * Emb[token(b)]·W_e^T computed in the kernel; token sources and w_e / ldw_e as s2vt_lstm_step_fwd_token.  A bad id never
 * addresses memory outside the table (it is read as token 0).  tok_const outside [0, V) is refused at once (S2VT_ERR_INDEX); an
 * id of `tok` outside [0, V) is reported as S2VT_ERR_INDEX by s2vt_check_async_error / a later call; a packed argmax word is in
 * range by construction and posts nothing - a greedy loop of these steps makes no device-to-host copy and never waits. */
int s2vt_gru_step_fwd_token(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* b_hh,
                            const float* h_prev, const float* emb, const float* w_e, int64_t ldw_e, const int32_t* tok,
                            const unsigned long long* tok_packed, int32_t tok_const, float* h_out, void* stream);
/* The same step inside a scheduled-sampling pass (s2vt_scheduled_decode below states the rule): token(b) = the packed word of
 * tok_packed where coin(row0 + b, step) < ss_prob, targets[b * targets_ld + step] otherwise (always at step 0, where tok_packed
 * may be NULL).  A ground-truth id outside [0, V) is read as token 0 and reported like a bad id of `tok`. */
int s2vt_gru_step_fwd_token_ss(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* b_hh,
                               const float* h_prev, const float* emb, const float* w_e, int64_t ldw_e,
                               const unsigned long long* tok_packed, const int64_t* targets, int64_t targets_ld, float ss_prob,
                               uint64_t seed, int32_t step, int32_t row0, float* h_out, void* stream);
/* BPTT of one step (autograd of the same, train.py:124): dh_t = dh_out + dh_{t+1} * z_{t+1} + dgh_next·W_hh (w_hh_t = W_hh^T
 * [H,3H], stash_next = the stash of step t+1); dh [B,H] in: dh_{t+1}, out: dh_t.  dgh_next, stash_next and w_hh_t are all
 * NULL at the last step (dh is then not read).  Writes dgx [B,3H] = d(gate input) and dgh [B,3H] = d(h W_hh^T + b_hh). */
int s2vt_gru_step_bwd(int32_t B, int32_t H, const float* dgh_next, const float* w_hh_t, const float* stash_next, const float* dh_out,
                      const float* stash, const float* h_prev, float* dh, float* dgx, float* dgh, void* stream);
/* A whole layer from the zero state (vid_rnn / word_rnn at S2VTModel.py:67 / :77): gx [n_gx*B, 3H] time-major covers steps
 * 0..n_gx-1, later steps see b_ih only (the zero-padded frames of S2VTModel.py:64-65).  h_all [T*B,H] out; stash [T*B,4H]
 * optional (NULL: inference). */
int s2vt_gru_seq_fwd(int32_t T, int32_t B, int32_t H, const float* gx, int32_t n_gx, const float* b_ih, const float* w_hh,
                     const float* b_hh, float* h_all, float* stash, void* stream);
/* BPTT over the layer: dh_out rows for steps >= dh_first ([(T-dh_first)*B, H]; NULL: none); h_all and stash of the forward
 * (left untouched).  dgx, dgh [T*B,3H] out: dW_ih = dgx^T x, db_ih = colsum(dgx), dW_hh = dgh[B:]^T h_all[:-B],
 * db_hh = colsum(dgh).  w_hh_t [H*3H] and dh [B*H] are scratch provided by the caller. */
int s2vt_gru_seq_bwd(int32_t T, int32_t B, int32_t H, const float* w_hh, const float* dh_out, int32_t dh_first, const float* h_all,
                     const float* stash, float* w_hh_t, float* dh, float* dgx, float* dgh, void* stream);
/* tok[t*B + b] = targets[b*targets_ld + t] (int64 batch-major -> int32 time-major, t < Lm1): the word ids nn.Embedding gathers
 * at S2VTModel.py:71.  An id outside [0, V) is clamped and reported as S2VT_ERR_INDEX by s2vt_check_async_error / the next call. */
int s2vt_tokens_time_major(int32_t B, int32_t Lm1, int32_t V, const int64_t* targets, int64_t targets_ld, int32_t* tok, void* stream);

/* ---------------------------------------------------------------- stacked LSTM chain (num_layers > 1)
 * S2VT with num_layers = N (S2VTModel.py:11-22: nn.LSTM(num_layers=N) for vid_rnn and word_rnn) is one chain of 2N LSTM layers
 * over T = 2L-1 steps: vid_l0 .. vid_l(N-1), word_l0 (input [Emb | vid top]), word_l1 .. word_l(N-1).  Layer j > 0 of a chain
 * reads the output of layer j-1 at the same step (its masked copy hm when layer j-1 has a dropout mask).  The entry points run
 * the chain as a layer wavefront (csrc/lstm_stack.hip): launch d advances every layer-step (j, t = d - j), so the chain takes
 * T + n - 1 launches (more where a diagonal holds more layer-steps than one launch).  fp32 throughout; row strides are the
 * natural widths (H, 4H) unless given; all step-indexed buffers are time-major (row t*B + b). */
typedef struct s2vt_lstm_layer {
    const float* w_hh;               /* [4H,H] weight_hh_l{k} */
    const float* w_in;               /* [4H, ldw_in] with the H input columns first: weight_ih_l{k} of the layer (k > 0), or the
                                        last H columns of word_rnn.weight_ih_l0 (the vid half).  NULL: no dense input */
    int64_t ldw_in;
    const float* x_in;               /* layer 0 only: its dense input [T*B,H] (e.g. vid top for the word chain); NULL: none */
    const float* gx;                 /* gate input rows x W_ih^T + b_ih + b_hh for steps [gx_t0, gx_t0 + n_gx): [n_gx*B, 4H] */
    int32_t gx_t0, n_gx;
    const float* bias;               /* [4H] b_ih + b_hh: the gate input of every other step */
    const float* h0; const float* c0;  /* [B,H] initial state (NULL: zero) */
    const float* mask;               /* [T*B,H] dropout mask (0 or 1/(1-p)) of this output as the next layer's input, or NULL */
    /* token segment (greedy decode, T = 1): Emb[tok] . W_e^T with tok = the packed argmax word (tok_packed, from
     * s2vt_decode_step_argmax) or tok_const; emb [V,E], w_e [4H, ldw_e] with the E embedding columns first */
    const float* emb; const float* w_e; int64_t ldw_e; int32_t E, V;
    const unsigned long long* tok_packed; int32_t tok_const;
    float* h; float* c;              /* [T*B,H] out */
    float* stash;                    /* [T*B,4H] activated gates i,f,g,o (train; NULL: not kept) */
    float* hm;                       /* [T*B,H] m . h (required with mask) */
    /* backward only */
    const float* dh_ext; int32_t dh_t0;  /* gradient from outside for steps >= dh_t0: [(T-dh_t0)*B, H]; NULL: none */
    float* dg;                       /* [T*B,4H] out: gradient of the gate pre-activations (may alias stash) */
    /* scheduled sampling of the token segment (forward only; NULL: none): the coin of (ss_row0 + b, ss_step) picks tok_packed's
     * word or ss_targets[b * ss_ld + ss_step], as s2vt_scheduled_decode defines it; a ground-truth id outside [0, V) is read as
     * token 0 and reported as S2VT_ERR_INDEX by s2vt_check_async_error / a later call */
    const int64_t* ss_targets; int64_t ss_ld; uint64_t ss_seed; float ss_prob; int32_t ss_step, ss_row0;
} s2vt_lstm_layer;
/* Forward of the chain (S2VTModel.py:67 and :77 for N layers each; greedy decode :86-:106 with T = 1, h0/c0 and the token
 * segment on word_l0).  Arguments are checked before any launch. */
int s2vt_lstm_chain_fwd(int32_t T, int32_t B, int32_t H, int32_t n, const s2vt_lstm_layer* layers, void* stream);
/* BPTT of the same chain (autograd at train.py:124): reads w_hh, w_in, mask, c0, c, stash, dh_ext of each layer, writes dg; the
 * initial states are constants (no gradient).  dh of layer j at step t = dh_ext + dG^j_{t+1} W_hh^j + m^j_t . (dG^{j+1}_t W_in^{j+1}).
 * The caller forms the weight gradients: dW_hh = dg[B:]^T h[:-B] (+ dg[:B]^T h0), dW_in = dg^T x, biases = column sums of dg.
 * workspace: s2vt_lstm_chain_bwd_workspace_bytes (transposed weights and the dc rows). */
size_t s2vt_lstm_chain_bwd_workspace_bytes(int32_t B, int32_t H, int32_t n);
int s2vt_lstm_chain_bwd(int32_t T, int32_t B, int32_t H, int32_t n, const s2vt_lstm_layer* layers, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Config-3 arithmetic of one LSTM layer forward (nn.LSTM at S2VTModel.py:67/:77 with bf16 operands, fp32 accumulate,
 * fp32 cell state): gx_stash [T*B,4H] gate input in (steps < n_gx; bias for the rest), activated gates out; h_all,
 * c_all [T*B,H] out.  persistent = 0: one launch per timestep; 1: one persistent launch per `block` timesteps
 * (0 = all T) with the W_hh slice of each compute unit resident in registers.  workspace[0] (int32) is set to 1 if a
 * hand-off wait of the persistent kernel timed out. */
size_t s2vt_lstm_seq_bf16_workspace_bytes(int32_t T, int32_t B, int32_t H);
int s2vt_lstm_seq_fwd_bf16(int32_t T, int32_t B, int32_t H, float* gx_stash, int32_t n_gx, const float* bias,
                           const float* w_hh, float* h_all, float* c_all, void* workspace, size_t workspace_bytes,
                           int32_t persistent, int32_t block, void* stream);
/* Two independent layers of one shape with every block of timesteps of BOTH in one persistent launch (the schedule
 * of the whole-path driver: vid_rnn block k+1 next to word_rnn block k); workspace = 2 x the single-layer size. */
int s2vt_lstm_seq_fwd_bf16_pair(int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                                const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1,
                                float* h_all0, float* h_all1, float* c_all0, float* c_all1, void* workspace,
                                size_t workspace_bytes, int32_t block, void* stream);
/* Config-3 arithmetic of one layer's BPTT (autograd of nn.LSTM, train.py:124, with bf16 operands dG / W_hh^T and fp32
 * accumulation, cell-state gradient and outputs): stash_dg [T*B,4H] activated gates in, fp32 dG out (in place); dh_out =
 * gradient arriving from above for steps >= dh_first ([(T-dh_first)*B, H], nullable); c_all [T*B,H] from the forward.
 * persistent / block as in s2vt_lstm_seq_fwd_bf16; the _pair form runs two layers side by side in one launch. */
size_t s2vt_lstm_seq_bwd_bf16_workspace_bytes(int32_t T, int32_t B, int32_t H);
int s2vt_lstm_seq_bwd_bf16(int32_t T, int32_t B, int32_t H, const float* w_hh, const float* dh_out, int32_t dh_first,
                           const float* c_all, float* stash_dg, void* workspace, size_t workspace_bytes,
                           int32_t persistent, int32_t block, void* stream);
int s2vt_lstm_seq_bwd_bf16_pair(int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                                const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1,
                                float* stash_dg0, float* stash_dg1, void* workspace, size_t workspace_bytes, int32_t block,
                                void* stream);
/* Test support: where the bf16 images lie inside the workspace of s2vt_lstm_seq_fwd_bf16 (backward = 0: the W_hh rows, then
 * the h rows [T*B]) or of s2vt_lstm_seq_bwd_bf16 (backward = 1: the W_hh^T rows, then the dG rows [T*B]).  out[0..2] = byte
 * offset, row stride in bf16 elements and padded k extent of the weight image, out[3..5] the same of the row image.  A _pair
 * workspace holds two such workspaces back to back, the second at + the single-layer workspace size.  No GPU call. */
int s2vt_lstm_seq_bf16_layout(int32_t T, int32_t B, int32_t H, int32_t backward, int64_t* out);
/* Recurrence schedule inside the whole-path train drivers (option "persist"): 0 = one launch per timestep everywhere (a card
 * shared with another process); 1 (default) = persistent kernels where the shape allows: forward and BPTT of the bf16
 * configuration (gemm mode 1, lstm_persist.hip), forward of the fp32-equivalent configuration (gemm mode 3, the split-precision
 * kernel of lstm_persist_x3.hip; option "persist_x3_fwd") and, with option "persist_x3_bwd", its BPTT.  Negative: query.
 * Returns the previous mode. */
int s2vt_set_recurrence_mode(int32_t mode);
/* Which recurrence kernels s2vt_train_forward / s2vt_train_backward would run for (B, H) in the current modes:
 * *fwd, *bwd = 0 one launch per timestep, 1 persistent bf16, 3 persistent split precision. */
int s2vt_recurrence_plan(int32_t B, int32_t H, int32_t* fwd, int32_t* bwd);
/* Which path a decode of *d would take in the current modes (encode_only != 0: s2vt_decode_encode_cached): *padded_B = the batch the
 * library runs (d->B, or the next multiple of 64 where it pads), *persist_encode = 1 where the encode phase runs as persistent
 * split-precision launches, *schedule of the token-dependent steps = 0 launches per timestep on two lanes, 1 a step and an argmax
 * launch per step (two chains over the batch halves at B % 128 == 0), 2 fused (option "decode_fused"). */
int s2vt_decode_plan(const s2vt_dims* d, int32_t encode_only, int32_t* padded_B, int32_t* persist_encode, int32_t* schedule);

/* Persistent forward recurrence in split precision (lstm_persist_x3.hip): the same computation as s2vt_lstm_seq_fwd with ONE launch
 * per `block` timesteps (0 = all T) and each compute unit's slice of W_hh resident in registers: both operands of
 * h_{t-1} . W_hh^T as three bf16 planes, six plane products on the bf16 matrix cores, fp32 accumulate - fp32-equivalent like gemm
 * mode 3; one workgroup per compute unit keeps its W_hh planes in 384 registers per lane.  H <= 1024, B % 32 == 0.  Layer 1
 * pointers may all be null (one layer); otherwise both layers share every launch.  gx_stash: gate input in, activated gates
 * out (in place).  workspace from s2vt_lstm_seq_x3_workspace_bytes (0 = shape not supported on this device; word 0 of the
 * workspace: hand-off time-out flag).  Whole-path use: the forward recurrences of s2vt_train_forward in gemm mode 3
 * (S2VTModel.py:67,77; option "persist_x3_fwd"). */
size_t s2vt_lstm_seq_x3_workspace_bytes(int32_t T, int32_t B, int32_t H);
int s2vt_lstm_seq_fwd_x3_persist(int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                              const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1, float* h_all0,
                              float* h_all1, float* c_all0, float* c_all1, int32_t block, void* workspace,
                              size_t workspace_bytes, void* stream);
/* BPTT in split precision (lstm_persist_x3.hip), the counterpart of s2vt_lstm_seq_fwd_x3_persist: the contraction
 * dG_{t+1} . W_hh is split over the gate columns - every workgroup multiplies the dG tile it has just computed with its 64 rows
 * of W_hh (planes resident in registers) for all H outputs, scatters the fp32 partial sums per consumer and gathers the ones
 * addressed to it (fixed summation order).  Same arithmetic contract as s2vt_lstm_seq_bwd (fp32-equivalent); stash_dg: activated
 * gates in, dG out (in place).  Layer 1 pointers may all be null.  block: timesteps per launch (0 = all T).
 * Whole-path use: option "persist_x3_bwd" routes the BPTT of s2vt_train_backward (gemm mode 3) through it (one stream, both
 * layers per launch). */
size_t s2vt_lstm_seq_bwd_x3_workspace_bytes(int32_t T, int32_t B, int32_t H, int32_t block);
int s2vt_lstm_seq_bwd_x3_persist(int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                                 const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1, float* stash_dg0,
                                 float* stash_dg1, int32_t block, void* workspace, size_t workspace_bytes, void* stream);
/* ---- the persistent split-precision kernels' fused outputs, TEST SUPPORT (tests/test_gpu_persist_emit.py): the two entry points
 * above with the fields that otherwise only the train / decode drivers fill in.  No kernel of their own; the extra arguments are
 * checked on the host and refused with S2VT_ERR_ARG and a message before any device call.
 *
 * s2vt_lstm_seq_fwd_x3_persist_emit: hblk (per layer, nullable) - h_t also as the blocked 3-plane row image of
 * s2vt_split_planes(3 planes) that the batched GEMMs read: rows t * B + b of ldhblk elements, k = unit; needs B % 64 == 0,
 * ldhblk >= 3 * (H rounded up to 64), ldhblk % 8 == 0, 16-byte aligned, (T * B) rows.  The kernel writes whole 16-unit k records:
 * units [H, 16 * ceil(H / 16)) of a written row receive zeros, nothing past them is touched (the caller keeps those at zero).
 * no_stash = 1: the activated gates are not written back to gx_stash.
 *
 * s2vt_lstm_seq_bwd_x3_persist_emit: dgp (per layer, nullable) - dG_t also as such a row image with k = g * H + u: needs
 * H % 8 == 0, B % 64 == 0, lddgp >= 3 * (4H rounded up to 64), lddgp % 8 == 0, 16-byte aligned; exactly the elements of rows
 * < T * B, k < 4H are written (the k padding is the caller's to zero).  colpart (per layer, nullable) [T * B / 32][4H]: the column
 * sums of dG over each 32-row chain, row t * (B / 32) + chain (s2vt_colsum_finish over them is the bias gradient).  skip_dg = 1
 * (needs dgp for every layer): the fp32 dG is not stored and stash_dg keeps the activated gates. */
int s2vt_lstm_seq_fwd_x3_persist_emit(int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                                      const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1, float* h_all0,
                                      float* h_all1, float* c_all0, float* c_all1, uint16_t* hblk0, int64_t ldhblk0, uint16_t* hblk1,
                                      int64_t ldhblk1, int32_t no_stash, int32_t block, void* workspace, size_t workspace_bytes,
                                      void* stream);
int s2vt_lstm_seq_bwd_x3_persist_emit(int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                                      const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1, float* stash_dg0,
                                      float* stash_dg1, uint16_t* dgp0, int64_t lddgp0, uint16_t* dgp1, int64_t lddgp1, float* colpart0,
                                      float* colpart1, int32_t skip_dg, int32_t block, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* One greedy decode step's out_linear + argmax (S2VTModel.py:95-96,105-106): packed[b] (zeroed by the caller)
 * receives max over v of (ordered(logit) << 32 | (0xFFFFFFFF - v)); token = 0xFFFFFFFF - low 32 bits. */
int s2vt_decode_step_argmax(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out,
                            unsigned long long* packed, void* stream);

/* The same decode step on the bf16 matrix cores with fp32-equivalent arithmetic (three bf16 planes per operand, six plane
 * products: csrc/argmax_x3.hip) - what s2vt_greedy_decode runs per step when the batch is a multiple of 64.  h and w_out are
 * split into plane images in `workspace` (s2vt_decode_step_argmax_x3_workspace_bytes) by this call. */
size_t s2vt_decode_step_argmax_x3_workspace_bytes(int32_t B, int32_t H, int32_t V);
int s2vt_decode_step_argmax_x3(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out,
                               unsigned long long* packed, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- sampled decoding (S2VT.forward(mode='sample'))
 * A draw from softmax(logit / temperature) per decode step instead of the arg-max, by Gumbel-max: the arg-max kernels above with
 * score = logit * (1 / temperature) + g ahead of their packed max (lowest index wins ties; the packed word's high half is the
 * ordered SCORE).  g is counter-based noise, defined once (csrc/philox.h; s2vt-video-caption_amd/sampling.py restates it in numpy):
 *     x = word (v % 4) of Philox4x32-10(counter = (v / 4, batch row, decode step, 0x47554D42), key = (seed low, seed high 32 bits))
 *     u = ((x >> 9) + 0.5) * 2^-23        g = -log(-log(u))
 * for vocabulary index v.  The noise of an element depends on (seed, decode step, batch row, v) and on nothing else: not on the
 * batch padding, the tile shape, the schedule (option "decode_fused"), the gemm mode or which kernel ran - row b of a batch of 10
 * and row b of the same clips padded to 64 rows get the same noise.  (The LOGITS of the kernels differ by rounding, so two paths
 * may draw differently where two scores are closer than that.)  temperature must be > 0 and finite with a finite reciprocal (the kernels multiply by
 * 1 / temperature: fp32 subnormals are refused); every argument is checked on the host before any device call.
 * s2vt_decode_step_sample[_x3]: one step; `step` = the decode step, row0 = the batch row of h's row 0.  packed as for the arg-max. */
int s2vt_decode_step_sample(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out, float temperature,
                            uint64_t seed, int32_t step, int32_t row0, unsigned long long* packed, void* stream);
size_t s2vt_decode_step_sample_x3_workspace_bytes(int32_t B, int32_t H, int32_t V);
int s2vt_decode_step_sample_x3(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out, float temperature,
                               uint64_t seed, int32_t step, int32_t row0, unsigned long long* packed, void* workspace,
                               size_t workspace_bytes, void* stream);
/* The whole decode: s2vt_greedy_decode[_cached] with a draw at every step (ids int64 [B, L-1], never stops at <eos>).  Same
 * workspace (s2vt_decode_workspace_bytes), same weight-image cache: a cache filled by a greedy call serves a sampling call and the
 * reverse. */
int s2vt_sample_decode(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, float temperature, uint64_t seed,
                       int64_t* ids, void* workspace, size_t workspace_bytes, void* stream);
int s2vt_sample_decode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, float temperature,
                              uint64_t seed, int64_t* ids, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                              int32_t cache_valid, void* stream);
/* K draws per clip on ONE encode (S2VT.sample; csrc/api_sample_rows.hip): ids int64 [B*K, L-1], row r = b*K + k.
 * THE NOISE CONTRACT: row b*K + k draws with the noise of (seed, decode step, batch row = b*K + k, v) above - same stream tag, same
 * mapping as s2vt_sample_decode.  The call therefore makes the draw that s2vt_sample_decode makes on the clips repeated K times
 * (clip b at rows b*K .. b*K + K-1), up to the paths' logit rounding where two scores are that close; K = 1 is s2vt_sample_decode.
 * Feature projection and both layers over the L frames run once per clip; the L-1 word steps run over the B*K rows, each reading
 * its clip's gate input and the word it drew at the step before on the device.  cache == NULL: fp32-input MFMA path throughout.
 * cache != NULL (s2vt_decode_cache_bytes; the protocol of s2vt_greedy_decode_cached): the persistent split-precision encode of
 * s2vt_decode_encode_cached and the plane-path step and head; shapes that encode does not take are refused (S2VT_ERR_ARG) before
 * anything is enqueued.  The encode's scratch is kept by the library per (device, stream), as for s2vt_score_captions.  One chain on
 * the caller's stream, no host round trip.  temperature as above, K >= 1, sos_ix in [0, V), workspace_bytes >=
 * s2vt_sample_rows_workspace_bytes: checked on the host before anything is enqueued (S2VT_ERR_ARG).
 * s2vt_sample_rows_workspace_bytes: 0 where the shape cannot be served (K < 1, or (L-1) * rows64(B*K) >= 2^31 packed words). */
size_t s2vt_sample_rows_workspace_bytes(const s2vt_dims* d, int32_t K);
int s2vt_sample_decode_rows(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t K, int32_t sos_ix, float temperature,
                            uint64_t seed, int64_t* ids, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                            int32_t cache_valid, void* stream);

/* ---------------------------------------------------------------- truncated draw: top-k / nucleus (top-p) ahead of the sampled draw
 * (S2VT.sample_truncated(..., top_k=, top_p=); csrc/truncate.hip; restated in numpy by
 * sampling.truncation_mask).  The fused heads above never hold a logits row; this draw works on one: for a row x[0..V),
 * inv_t = 1 / temperature, top_k = k, top_p = p
 *   1. scores   s_v = x_v * inv_t in fp32 (the heads' expression).
 *   2. top-k    (k = 0 or k >= V: off)  tau = the k-th largest s, counted with multiplicity; survivors {v : s_v >= tau}.  Equal
 *               values at the k-th place all stay: at least k elements survive.
 *   3. nucleus  (p >= 1: off, not evaluated) over the survivors of 2:  m = max s, e_v = expf(s_v - m), Z = sum e_v;  v stays iff
 *               A(s_v) < p * Z with A(y) = sum of e_u over {u : s_u > y} - the shortest descending prefix whose mass reaches p,
 *               renormalised over the top-k set ("top-k, then top-p").  Equal values stay or go together; the maximum always stays
 *               (A = 0).
 *   4. draw     token = argmax over the kept v of (s_v + g_v), the lowest index wins a tie; g is EXACTLY the noise above: Philox
 *               counter (v / 4, batch row = row0 + r, decode step, 0x47554D42), key = seed halves.  With nothing truncated the draw
 *               is the heads' draw up to the logit rounding between GEMM paths.
 *   5. output   packed[r] = ordered(score) << 32 | (0xFFFFFFFF - v), the heads' word (a plain store: the row's workgroup owns it,
 *               packed need not be zeroed), read unchanged by the next token step; kept[r] (nullable) = the number of survivors.
 * Every sum is a fixed-order fp32 reduction (per thread in ascending element order, wave butterfly, (w0 + w1) + (w2 + w3)): no
 * floating-point atomics, the same inputs give the same bits.  The index written is always in [0, V).
 * s2vt_truncated_draw: logits fp32 [rows, V] with row stride ld >= V; V * 4 <= 150 KiB.  Checked on the host before anything is
 * enqueued (S2VT_ERR_ARG): top_k in [0, V], top_p in (0, 1] (NaN refused), the temperature rule of the sampled decode.
 * s2vt_sample_decode_rows_trunc: s2vt_sample_decode_rows with, per step, the head replaced by the logits GEMM ([rows64(B*K), V]
 * fp32 in the workspace: the plane GEMM on the cache's W_o image, or the fp32-input GEMM on out_w) and the draw above, batch row =
 * r.  top_k == 0 and top_p >= 1 run the fused head - the launches of s2vt_sample_decode_rows.  Workspace from
 * s2vt_sample_rows_trunc_workspace_bytes (0 where s2vt_sample_rows_workspace_bytes is 0 or V * 4 > 150 KiB). */
int s2vt_truncated_draw(const float* logits, int64_t ld, int64_t rows, int32_t V, float temperature, int32_t top_k, float top_p,
                        uint64_t seed, int32_t step, int32_t row0, unsigned long long* packed, int32_t* kept, void* stream);
/* The beam searches' fan-out kernel on its own (csrc/ce.hip, what s2vt_beam_step runs behind out_linear): per logits row the 20 most
 * probable tokens in ascending token order, top_ix int32 [rows, 20], and their log-probs, top_lp fp32 [rows, 20].  20 <= V, V * 4 <=
 * 150 KiB.  The existing row kernel of the truncated draw's frame: tools/bench_sample_trunc.py times the two on one logits buffer. */
int s2vt_top20_logprob(const float* logits, int64_t ld, int64_t rows, int32_t V, int32_t* top_ix, float* top_lp, void* stream);
size_t s2vt_sample_rows_trunc_workspace_bytes(const s2vt_dims* d, int32_t K);
int s2vt_sample_decode_rows_trunc(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t K, int32_t sos_ix,
                                  float temperature, uint64_t seed, int32_t top_k, float top_p, int64_t* ids, void* workspace,
                                  size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid, void* stream);

/* ---------------------------------------------------------------- constrained draw: what a decode must not generate
 * (S2VT.decode_constrained(..., no_repeat_ngram_size=, repetition_penalty=, min_length=, banned_ids=); csrc/truncate.hip; restated in
 * numpy by sampling.constrain_logits).  For one row at decode step t - t = the number of words already generated after <sos>, the
 * history h[0..t), the logits x[0..V) in fp32 - the rules apply in this order to the RAW logits, before the temperature:
 *   1. repetition penalty  theta >= 1 (1: off; the rule of CTRL, Keskar et al. 2019): once for every DISTINCT v of h, not once per
 *               occurrence, x_v <- x_v * r if x_v > 0, else x_v * theta, with r = fp32(1.0 / (double)theta) computed on the host - a
 *               multiplication, so the numpy restatement is bitwise.
 *   2. no-repeat n-gram    n >= 0 (0: off; n = 1 bans every word of h): if t >= n - 1, for every i in [0, t - n] with
 *               h[i .. i+n-2] == h[t-n+1 .. t-1]:  x[h[i+n-1]] <- -inf.
 *   3. banned ids          (at most 32, each in [0, V)):  x_v <- -inf.
 *   4. minimum length      m >= 0: if t < m, x[eos_ix] <- -inf.
 * A ban wins over a penalty on the same v.  Then the pick:
 *   greedy = 1  the arg-max of x, the lowest index wins a tie (-0 counts as +0); packed = ordered(x_v) << 32 | (0xFFFFFFFF - v); no
 *               noise; temperature, top_k, top_p must be 1, 0, 1.
 *   greedy = 0  steps 1-5 of the truncated draw above on the constrained row; the noise contract is unchanged.
 * The index written is always in [0, V); if nothing survives, the truncated draw's fallback holds (the row maximum by key).  A row
 * that has emitted <eos> is processed like any other: the decoders never stop at <eos>, callers cut behind it.
 * THE CALL MODIFIES `logits`: the edits are made in place in the rows (one workgroup owns a row, exactly one thread writes an edited
 * element), inside the row kernel's launch and in front of its load; afterwards the buffer holds the constrained rows.
 * hist: the drivers' packed words, unsigned long long [t][hist_ld]; the token of row r at step i is 0xFFFFFFFF - the low half of
 * hist[i * hist_ld + r].  May be null iff t == 0.  `banned` of s2vt_constraints is a HOST pointer: the ids are copied into the launch
 * arguments, no device allocation is made.
 * Checked on the host before anything is enqueued (S2VT_ERR_ARG; s2vt_last_error names the rule): repetition_penalty finite and
 * >= 1; no_repeat_ngram >= 0; min_length >= 0; n_banned in [0, 32]; every banned id and eos_ix in [0, V); t in [0, 1023]; hist_ld
 * >= rows where t > 0; the truncated draw's rules; greedy in {0, 1} and the greedy rule above. */
typedef struct s2vt_constraints {
    int32_t no_repeat_ngram;
    float repetition_penalty;
    int32_t min_length;
    int32_t eos_ix;
    int32_t n_banned;
    const int32_t* banned; /* host memory, n_banned ids; may be null when n_banned == 0 */
} s2vt_constraints;
int s2vt_constrained_draw(float* logits, int64_t ld, int64_t rows, int32_t V, const unsigned long long* hist, int64_t hist_ld, int32_t t,
                          const s2vt_constraints* c, int32_t greedy, float temperature, int32_t top_k, float top_p, uint64_t seed,
                          int32_t step, int32_t row0, unsigned long long* packed, int32_t* kept, void* stream);
/* s2vt_sample_decode_rows_trunc with a greedy flag and the constraints: at step j the head is the logits GEMM (plane path or
 * fp32-input path, as there) and the constrained draw over the driver's own packed words (hist_ld = rows64(B*K), t = j).  K >= 1;
 * greedy needs temperature 1, top_k 0, top_p 1.  With every constraint off (n = 0, theta = 1, m = 0, no banned id) the call runs
 * today's launches: greedy the fused arg-max head, sampled exactly what s2vt_sample_decode_rows_trunc runs.  A shape that could ban a
 * whole row is refused: V > (L - 1) + n_banned + 1 is required, and L - 1 <= 1024 (t <= 1023).  The workspace is the truncated one. */
size_t s2vt_decode_rows_constrained_workspace_bytes(const s2vt_dims* d, int32_t K);
int s2vt_decode_rows_constrained(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t K, int32_t sos_ix, int32_t greedy,
                                 float temperature, uint64_t seed, int32_t top_k, float top_p, const s2vt_constraints* c, int64_t* ids,
                                 void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                                 void* stream);

/* ---------------------------------------------------------------- constrained beam: the constraints inside the cumulative-score search
 * (S2VT.beam_constrained(..., no_repeat_ngram_size=, repetition_penalty=, min_length=, banned_ids=); csrc/beam_policy.hip, csrc/ce.hip;
 * restated in fp64 by tests/beam_constrained_ref.py).  The search is EXACTLY the cumulative-score beam search above
 * (s2vt_beam_cum_step) with one change.  At depth t, live slot j holds the words h = (w_1 .. w_{t-1}) (without <sos>).  Its fp32
 * logits row is first edited by rules 1-4 of the constrained draw with history h and step t-1 - sampling.constrain_logits(x, h, t-1,
 * spec), bit for bit in fp32: the penalty on every distinct word of h, -inf on a word that would complete an n-gram h already holds,
 * -inf on the banned ids, -inf on <eos> while t-1 < min_length.  lp_j is then log_softmax of the EDITED row: the mass is renormalised
 * over the surviving words (the stance of the constrained and the truncated draw: the rules act on the raw logits).  Scores, tie
 * rules, the pool and S / t**alpha, hypotheses unfinished at max_depth entering the pool without <eos>, and n_best are unchanged.
 *   defaults   with every constraint off the result is mode='beam''s bit for bit: the callers run the existing launches
 *              (s2vt_beam_cum_step and the unconstrained fan-out), not a neutral form of the new ones.
 *   width 1    beam_width = 1, length_alpha = 0, n_best = 1: the words up to and including the first <eos> are those of greedy
 *              s2vt_decode_rows_constrained with the same constraints, wherever the step margins are clear.
 *   fan-out    20 per row stays exact for beam_width <= 8: the top 20 are taken from the edited row.  A -inf candidate must never be
 *              selected, so a shape that could leave a row fewer than 20 finite words is refused:  V >= 20 + max_depth + n_banned + 1
 *              (per call of the head: V >= 20 + t + n_banned + 1), and max_depth <= 1023, the constraint phase's history bound.
 *   early stop unchanged: its proof needs lp <= 0 only, which the log_softmax of any edited row still gives.
 * s2vt_beam_cum_hist_bytes / s2vt_beam_cum_hist_step: s2vt_beam_cum_bytes / s2vt_beam_cum_step whose state also keeps every live
 * slot's words, hist[2][B][beam_width][max_depth] int32 behind the plain state (s2vt_beam_cum_result serves both forms), ping-ponged
 * by depth parity.  Same policy, same rows, same results as s2vt_beam_cum_step on the same inputs.  After the call with `depth`,
 * *hist_out is the device pointer and *hist_ld_out (= max_depth) the row stride of the buffer that the NEXT depth step must read:
 * row r = b * beam_width + slot holds that slot's depth - 1 words at (*hist_out)[r * ld + i], i < depth - 1.  Rows of unused slots and of
 * frozen samples hold defined words (zeros, or words written earlier); their fan-out is never consumed.
 * s2vt_top20_logprob_constrained: the fan-out head on its own - s2vt_top20_logprob with the constraint phase in front of the row's
 * load, in the same launch.  THE CALL MODIFIES `logits` (afterwards the constrained rows).  hist_i32: int32 [rows][hist_ld], row r's t
 * words at hist_i32[r * hist_ld + i]; null iff t == 0.  The host-side checks of s2vt_constrained_draw (S2VT_ERR_ARG), with hist_ld >= t,
 * plus V >= 20 and V >= 20 + t + n_banned + 1.  With every constraint off it runs s2vt_top20_logprob's launch.
 * s2vt_beam_step_constrained: the depth step with that head, for all three forms - gx_vid != NULL: s2vt_beam_step_gx (needs cache; the
 * vid_* arguments are not read); else cache != NULL: s2vt_beam_step_cached; else s2vt_beam_step.  hist / hist_ld: what
 * s2vt_beam_cum_hist_step returned for this depth; t = depth - 1. */
size_t s2vt_beam_cum_hist_bytes(int32_t B, int32_t beam_width, int32_t max_depth);
int s2vt_beam_cum_hist_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, double length_alpha,
                            int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b,
                            int32_t* row_state, int32_t* row_tok, const int32_t** hist_out, int64_t* hist_ld_out, void* stream);
int s2vt_top20_logprob_constrained(float* logits, int64_t ld, int64_t rows, int32_t V, const int32_t* hist_i32, int64_t hist_ld, int32_t t,
                                   const s2vt_constraints* c, int32_t* top_ix, float* top_lp, void* stream);
int s2vt_beam_step_constrained(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                               const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                               const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out,
                               int32_t* top_ix, float* top_lp, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                               const s2vt_constraints* c, const int32_t* hist, int64_t hist_ld, int32_t t, void* stream);

/* ---------------------------------------------------------------- diverse beam: diverse (group) beam search on the device
 * (S2VT.beam_diverse(..., beam_width=, num_groups=, diversity_lambda=); Vijayakumar et al., 2016; not in the reference;
 * csrc/beam_policy.hip; restated in fp64 and fp32 by tests/beam_div_ref.py).  Per sample: W = beam_width slots, G = num_groups,
 * Wg = W / G, lambda = diversity_lambda >= 0, D = max_depth; W % G == 0 and 1 <= G <= W <= 8.  Group g owns slots g*Wg .. (g+1)*Wg-1,
 * a live list and a pool of at most Wg entries.  Every live list starts as one empty hypothesis: S = 0, last word <sos>, the encoder
 * state of mode='beam'.  For t = 1..D:
 *   cnt[v] = 0 for every word; the groups run in order g = 0..G-1; a group whose live list is empty is closed, is skipped and
 *   contributes nothing to cnt.
 *   Candidate (j, v) of live slot j (in slot order) has the score s = S_j + lp_j[v] and the selection key a = s - lambda * cnt[v].
 *   The min(Wg, count) best candidates by (a descending, j ascending, v ascending) are walked in that order.  Every selected
 *   candidate does cnt[v] += 1, <eos> included.  v == <eos> enters the group's pool with s / t**alpha - the unpenalised sum: the
 *   penalty steers the selection only and is never accumulated; anything else becomes the group's next live slot with S = s.
 *   At t == D every live hypothesis enters its group's pool with S / D**alpha, with no <eos> appended.
 * A pool is ordered by (score descending, insertion ascending); the answer is each group's first n_best entries (n_best <= Wg).
 * lp is log_softmax of the slot's logits row; with constraints, of the row edited with the slot's own words as history, exactly as in
 * the constrained beam above.
 *   fp32 form  s = S_j + fminf(lp, 0), -0 folded to +0; a = s when cnt == 0, otherwise a = s - (fp32(lambda) * fp32(cnt)), the product
 *              and the difference each rounded to fp32 (never one FMA); pool scores divide by fp32(double pow), as above.
 *   groups     group 0 is never penalised: it is the cumulative-score search at width Wg.  lambda = 0: every group is.  G = 1 is that
 *              search itself; the callers then run s2vt_beam_cum_step, not this policy.
 *   fan-out    20 per row stays exact for W <= 8: in group g at most g * Wg <= W - Wg distinct words are penalised; a candidate outside
 *              its parent's unpenalised top W has W candidates of the same parent in front of it, at least Wg of them unpenalised,
 *              whose keys are >= its key and which win every tie.  With constraints the argument runs on the edited row, under the
 *              rule V >= 20 + max_depth + n_banned + 1.
 *   early stop a group is settled when it is closed, or when its pool holds Wg entries and pool[Wg-1].score >= max_j(live S_j) /
 *              D**alpha (the maximum: live slots are ordered by a, not by S); its pool can then never change (lp <= 0, the proof of
 *              the cumulative search per group), and "settled" is monotone.  A sample is frozen only when ALL its groups are settled:
 *              until then settled groups keep stepping and keep counting in cnt, because later groups depend on their choices.  A
 *              frozen sample's slots carry token 0 / state row 0; the int32 at byte 0 of `state` counts the frozen samples.
 * Row protocol and `depth` as for s2vt_beam_cum_step: row b * W + slot; depth = 1 gives the first slot of every group row_state = b,
 * row_tok = <sos> (unused slots: state 0 / token 0); depth = 2..max consume the step before; depth = 0 consumes step max_depth.
 * s2vt_beam_div_bytes: the state's size, 0 for dimensions that are refused; hist != 0: the form that also keeps every live slot's
 * words, hist[2][B][W][max_depth] int32 behind the plain state, as s2vt_beam_cum_hist_step keeps them.
 * s2vt_beam_div_step: hist_out and hist_ld_out both null: the plain form.  Both non-null: the form with the words; after the call
 * *hist_out / *hist_ld_out are what s2vt_beam_step_constrained must read at the next depth step (see s2vt_beam_cum_hist_step).
 * s2vt_beam_div_result: every group's first n_best pool entries (1 <= n_best <= Wg) -> out_tokens [B][G][n_best][max_depth] int32
 * (words after <sos>, padded with eos_ix), out_len [B][G][n_best], out_score [B][G][n_best], each group best first; serves both forms.
 * One policy, one state (csrc/beam_policy.hip): the s2vt_beam_cum_* entries are these at num_groups = 1, diversity_lambda = 0 (inert at one
 * group) - s2vt_beam_cum_bytes(B, W, D) == s2vt_beam_div_bytes(B, W, 1, D, 0), s2vt_beam_cum_hist_bytes(B, W, D) ==
 * s2vt_beam_div_bytes(B, W, 1, D, 1), and a state stepped through one family is read by the other's result entry. */
size_t s2vt_beam_div_bytes(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t hist);
int s2vt_beam_div_step(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t sos_ix, int32_t eos_ix,
                       double length_alpha, double diversity_lambda, int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix,
                       const float* top_lp, int32_t* row_b, int32_t* row_state, int32_t* row_tok, const int32_t** hist_out,
                       int64_t* hist_ld_out, void* stream);
int s2vt_beam_div_result(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t eos_ix, int32_t n_best, void* state,
                         size_t state_bytes, int32_t* out_tokens, int32_t* out_len, float* out_score, void* stream);

/* ---------------------------------------------------------------- ensemble beam: several models, one cumulative-score search
 * (S2VT.Ensemble(models, weights=None).beam(...); csrc/ensemble.hip; restated in numpy fp32 and fp64 by tests/ensemble_ref.py).
 * The search is EXACTLY the cumulative-score beam search above (s2vt_beam_cum_step; constrained: s2vt_beam_cum_hist_step) with one
 * change: lp_j, the log-probs of live slot j, is the log of the weighted arithmetic mean of the members' word distributions.  Each
 * member keeps its own encoder states, decode cache and depth step; the policy, the early-exit poll and the result are shared.
 * Members m = 0..M-1, 1 <= M <= 8; weights w_m > 0 and finite, normalised by the host to sum 1 in fp64; lw_m = fp32(log(w_m)), the
 * log taken in fp64; default: uniform.  For one row (a beam slot) with the members' raw logits rows x_m[0..V):
 *   lse_m    the log-sum-exp of x_m by exactly s2vt_top20_logprob's arithmetic: the block maximum; expf(x - max) summed per thread
 *            (thread tid owns the elements tid + 256 j) in ascending index; wave butterflies; (w0 + w1) + (w2 + w3); max + logf(sum)
 *   a_m[v]   = (x_m[v] - lse_m) + lw_m
 *   amax[v]  = max_m a_m[v]
 *   c[v]     = amax[v] + logf(sum over m ascending of expf(a_m[v] - amax[v])); -inf (never NaN) where every a_m[v] is -inf, a
 *            word the constraints removed in every member
 *   result   the 20 largest c[v], ties -> the lower id, in ASCENDING token order as s2vt_top20_logprob returns them; top_lp = c:
 *            the mean of normalised distributions is normalised, so there is no second normalisation
 *   M = 1    with w = 1: c = a_0 exactly (logf(expf(0)) = 0) and the head is s2vt_top20_logprob bit for bit; that kernel runs.
 *   constrained  every member's row of the slot is first edited IN PLACE by rules 1-4 of the constrained draw with the slot's own
 *            words as history (the same spec for every member), in the same launch; lse_m is then that of the edited row.
 * One 256-thread workgroup per row, fixed-order reductions, no atomics: the same inputs give the same bits.
 * s2vt_ensemble_top20: member m's row r starts at logits + m * member_stride + r * ld.  log_w: M HOST floats, passed by value into
 * the launch.  Requires 1 <= M <= 8, 20 <= V <= 38400, ld >= V, member_stride >= rows * ld, every log_w finite and <= 0;
 * everything else is S2VT_ERR_ARG with a message naming the entry.
 * s2vt_ensemble_top20_constrained: the same behind the checks of s2vt_top20_logprob_constrained (V >= 20 + t + n_banned + 1); THE
 * CALL MODIFIES `logits`.  With every constraint off it runs s2vt_ensemble_top20's launch and leaves the buffers untouched.
 * s2vt_beam_step_logits: the depth step of ONE member, stopped one launch early - the form is chosen as s2vt_beam_step_constrained
 * chooses it (gx_vid, else cache, else neither), the launches are the same up to and including out_linear, which writes the R rows'
 * logits to logits_out (row stride ld_out >= V); no fan-out, no top_ix / top_lp. */
int s2vt_ensemble_top20(const float* logits, int64_t member_stride, int64_t ld, int32_t M, int64_t rows, int32_t V, const float* log_w,
                        int32_t* top_ix, float* top_lp, void* stream);
int s2vt_ensemble_top20_constrained(float* logits, int64_t member_stride, int64_t ld, int32_t M, int64_t rows, int32_t V, const float* log_w,
                                    const int32_t* hist_i32, int64_t hist_ld, int32_t t, const s2vt_constraints* c, int32_t* top_ix,
                                    float* top_lp, void* stream);
int s2vt_beam_step_logits(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out,
                          float* logits_out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                          void* stream);

/* ---------------------------------------------------------------- stochastic beam: K distinct sampled captions per clip
 * (S2VT.sample_distinct(feats, n_samples=, temperature=, seed=, max_depth=); Kool, van Hoof, Welling, "Stochastic Beams and Where to
 * Find Them", ICML 2019; not in the reference; csrc/gumbel_top.hip, csrc/sbs_policy.hip; restated in numpy by tests/sbs_ref.py).
 * Sampling WITHOUT replacement from the model's distribution over whole sentences: W pairwise distinct captions of a clip, in the exact
 * order a sequential without-replacement sampler would draw them, with their log-probabilities, their perturbed scores and the
 * threshold that inclusion probabilities need - in one beam-shaped pass.
 * Per clip b: W = n_samples slots, 1 <= W <= 8; D = max_depth; inv_t = fp32(1 / temperature); a 64-bit seed.  A slot is empty, live or
 * finished and carries phi (fp32: the sum of its words' log-probs), G (fp64: its perturbed score), a back-trace node and a length.
 *   start      slot 0 is live with phi = 0, G = 0, last word <sos> and the encoder state of mode='beam'; the others are empty;
 *              kappa = -inf.
 *   depth t = 1..D: the depth step runs over the fixed rows r = b * W + slot, as in mode='beam'.  After it, for every live slot j:
 *   head       per logits row x of row r, in fp32: s_v = x_v * inv_t; lse = max + logf(sum expf(s - max)) in s2vt_top20_logprob's
 *              fixed order; lp_v = fminf(s_v - lse, 0); g_v = lp_v + gumbel(seed, step = t - 1, row = r, v) - the draw of the
 *              sampled decode above (Philox4x32-10, counter (v / 4, row, step, 0x47554D42), word v % 4; same stream tag).  The
 *              head returns the 20 largest g_v by (g descending, v ascending), IN THAT ORDER: top_ix, top_lp (unperturbed), top_g.
 *   children   child f of slot j: phi' = phi_j + top_lp[f], one fp32 add with -0 folded to +0.
 *   scores     Z = top_g[0], g = top_g[f], both widened exactly to fp64; in fp64: d = g - Z; l = log(-expm1(d)) if d > -ln 2, else
 *              log1p(-exp(d)); u = (G_j - g) + l; G~ = (G_j - max(u, 0)) - log1p(exp(-|u|)) - the numerically stable form of
 *              -log(exp(-G_j) - exp(-Z) + exp(-g)).  At f = 0: d = 0, l = u = -inf and G~ = G_j exactly.  Every G~ <= G_j.
 *   finished   a finished slot is one candidate, itself, with its own G.
 *   candidate  index c = j * 20 + f, f = 0 for a finished slot.
 *   selection  the min(W, count) best by (G~ descending, c ascending) become slots 0, 1, ... in that order.  A finished candidate
 *              stays as it is.  A child appends a back-trace node; v == <eos> makes it finished with length t, otherwise it is
 *              live with row_state its parent's row and row_tok = v.
 *   threshold  kappa = max(kappa, best unselected G~).
 *   stop       a clip with no live slot after the walk is frozen: nothing of it can change any more.  The int32 at byte 0 of
 *              `state` counts the frozen clips.
 *   end        after depth D the live slots remain as unfinished samples of length D, no <eos> appended.  The answer is the W slots
 *              in order, which is non-increasing G: the order in which sampling without replacement draws them.
 *   fan-out    20 per row is exact: G~ is increasing in g for one parent, so a parent's selected children are a prefix of its
 *              g-order; at most W <= 8 are selected and its best unselected child is at most its 9th.
 *   W = 1      ancestral Gumbel-max sampling with the noise of the sampled decode (row b, step t - 1): the words of
 *              s2vt_sample_decode_rows at K = 1 up to the first <eos>, wherever the draw is decided.
 * s2vt_top20_gumbel: the head on its own.  One 256-thread workgroup per row on s2vt_top20_logprob's register / LDS forms, every
 * element runs its own Philox block, fixed-order reductions, no atomics: the same inputs give the same bits.  Row i of the launch
 * draws with batch row row0 + i.  top_lp is recomputed from the logits row, not by subtracting the noise from g.  Requires
 * 20 <= V <= 38400, ld >= V, inv_temperature finite and > 0, step >= 0, row0 >= 0.
 * s2vt_beam_step_gumbel: the depth step with that head, the form chosen as s2vt_beam_step_constrained chooses it (gx_vid, else cache,
 * else neither); the launches in front of the head are those of the other forms; adds the output top_g [R, 20]; row0 = 0.
 * s2vt_sbs_bytes / s2vt_sbs_step / s2vt_sbs_result: the policy, one wave per clip, on the row protocol and `depth` convention of
 * s2vt_beam_cum_step (depth = 1 initialises; 2..max_depth consume the step before; 0 consumes step max_depth).  Rows of slots that
 * are not live carry token 0 / state row 0.  s2vt_sbs_bytes is 0 for dimensions that are refused.  s2vt_sbs_result back-traces:
 * out_tokens [B][W][max_depth] int32 (words after <sos>, padded with eos_ix), out_len [B][W], out_logprob [B][W] fp32 (phi),
 * out_perturbed [B][W] fp32 (G rounded), out_kappa [B] fp32. */
int s2vt_top20_gumbel(const float* logits, int64_t ld, int64_t rows, int32_t V, float inv_temperature, uint64_t seed, int32_t step,
                      int32_t row0, int32_t* top_ix, float* top_lp, float* top_g, void* stream);
int s2vt_beam_step_gumbel(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out,
                          int32_t* top_ix, float* top_lp, float* top_g, void* workspace, size_t workspace_bytes, void* cache,
                          size_t cache_bytes, float inv_temperature, uint64_t seed, int32_t step, void* stream);
size_t s2vt_sbs_bytes(int32_t B, int32_t n_samples, int32_t max_depth);
int s2vt_sbs_step(int32_t B, int32_t n_samples, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, int32_t depth, void* state,
                  size_t state_bytes, const int32_t* top_ix, const float* top_lp, const float* top_g, int32_t* row_b, int32_t* row_state,
                  int32_t* row_tok, void* stream);
int s2vt_sbs_result(int32_t B, int32_t n_samples, int32_t max_depth, int32_t eos_ix, void* state, size_t state_bytes, int32_t* out_tokens,
                    int32_t* out_len, float* out_logprob, float* out_perturbed, float* out_kappa, void* stream);

/* ---------------------------------------------------------------- scheduled sampling (S2VT.forward(mode='train', ss_prob > 0))
 * Bengio et al., NeurIPS 2015: during training each decode-step input is the ground-truth word with probability 1 - p and the
 * word the model itself chose at the previous step with probability p.  Two passes: the decode drivers above run once more with
 * a coin per (batch row, step) in front of every token step and hand out the words that were fed; the unchanged teacher-forced
 * train step then runs on those words.  Nothing differentiates through the choice or the coin.
 *   targets [B, T] int64, T = L - 1: the input words of mode='train' (caps[:, :-1], <sos> first), row stride targets_ld.
 *   used[b, 0]  = targets[b, 0]
 *   draws[b, j] = the model's choice at decode step j, the word layer having been fed used[b, 0..j]: the arg-max of the logits
 *                 (draw_mode 0) or the Gumbel-max draw of the sampled decode (draw_mode 1: the noise of (seed, decode step j,
 *                 batch row b, v) exactly as above - same stream tag, same mapping)
 *   used[b, j]  = draws[b, j-1] if coin(b, j) < p, else targets[b, j]                                  (j = 1 .. T-1)
 *   coin(b, j)  = ((x >> 9) + 0.5) * 2^-23, x = word 0 of Philox4x32-10(counter = (0, b, j, 0x53534D58), key = (seed low, seed
 *                 high 32 bits)): exact in fp32, strictly inside (0, 1); compared in fp32 with p, so p = 0 never and p = 1
 *                 always takes the model's word.  b is the row of the caller's batch: batch padding, the two-chain schedule
 *                 and tile shapes never enter (the noise contract of the sampled decode).
 * Inference arithmetic (no dropout, weights as they stand).  A ground-truth id outside [0, V) that is fed is read as token 0 and
 * reported as S2VT_ERR_INDEX by s2vt_check_async_error / the next call (used still records the id as given).
 * s2vt_scheduled_decode[_cached]: s2vt_sample_decode[_cached] with the coin - same workspace (s2vt_decode_workspace_bytes), same
 * weight-image cache, same schedules and padding.  used [B, L-1] and draws [B, L-1] (nullable) int64, contiguous.  0 <= ss_prob
 * <= 1 (NaN refused), draw_mode 0 or 1, the temperature rule of the sampled decode when draw_mode = 1 (ignored otherwise): all
 * checked on the host before anything is enqueued. */
int s2vt_scheduled_decode(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t targets_ld,
                          float ss_prob, int32_t draw_mode, float temperature, uint64_t seed, int64_t* used, int64_t* draws,
                          void* workspace, size_t workspace_bytes, void* stream);
int s2vt_scheduled_decode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t targets_ld,
                                 float ss_prob, int32_t draw_mode, float temperature, uint64_t seed, int64_t* used, int64_t* draws,
                                 void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                                 void* stream);
/* One step of the rule on token ids: out[b] = draw_tokens[b] if step > 0 and coin(row0 + b, step) < ss_prob, else
 * targets[b * targets_ld + step] (b < B; all int64). */
int s2vt_ss_mix(const int64_t* draw_tokens, const int64_t* targets, int64_t targets_ld, int32_t B, float ss_prob, uint64_t seed,
                int32_t step, int32_t row0, int64_t* out, void* stream);
/* used / draws (nullable) [B, steps] from the packed arg-max words packed[steps][B] of a loop of scheduled steps
 * (s2vt_gru_step_fwd_token_ss, s2vt_lstm_chain_fwd with ss_targets), by the same rule. */
int s2vt_ss_unpack(const unsigned long long* packed, int32_t steps, int32_t B, const int64_t* targets, int64_t targets_ld, float ss_prob,
                   uint64_t seed, int64_t* used, int64_t* draws, void* stream);

/* ---------------------------------------------------------------- run-time options
 * ONE table holds every switch of the library (csrc/options.hip).  The first read of an option takes S2VT_<NAME> (upper case)
 * from the environment when it is set; s2vt_set_option changes it afterwards and returns the previous value (a negative value
 * only queries; INT32_MIN: unknown name).  The typed setters below are views of the same table.
 *   gemm_mode       3 | 1 | 0   arithmetic of the batched GEMMs (s2vt_set_gemm_mode)
 *   persist         1 | 0       persistent recurrence kernels (s2vt_set_recurrence_mode)
 *   persist_x3_fwd  1 | 0       split-precision persistent forward of gemm mode 3
 *   persist_x3_bwd  2 | 1 | 0   split-precision persistent BPTT of gemm mode 3 (layers per launch: option bptt_solo): 1 wherever the
 *                               shape is supported, 2 only where a workgroup carries one 32-row chain (B = 64 at H = 1000), 0 never
 *   pipe_block      32          timesteps per pipeline block (s2vt_set_pipeline_block)
 *   graph           0 | 1       hipGraph replay of the train launch sequences (s2vt_set_graph_mode)
 *   decode_fused    1 | 0       schedule of the greedy decode's token steps (s2vt_set_decode_schedule)
 *   cu_reserve      0..128      the persistent GEMMs of s2vt_train_backward plan their grids for this many compute units fewer FROM
 *                               THE RELEASE OF GRADIENT GROUP 0 (s2vt_backward_wait_grads) to the end of the backward - the span in
 *                               which the communication kernels of a data-parallel run hold compute units; everything before
 *                               it (forward, BPTT and the GEMMs beside it) plans for the whole device
 *   bptt_units      0 | 16 | 32 hidden units per workgroup of the persistent bf16 BPTT (0: 32 where two layers fit the device)
 *   corun           3 (0..5)    persistent split-precision schedule (B = 64): this many TENTHS of a GEMM that nothing waits for (dW_o's
 *                               k range) run beside EACH one-layer first / last stage of the BPTT, planned for the compute units
 *                               that stage leaves idle (0: every GEMM alone on the device)
 *   bptt_solo       1 | 0       (with corun > 0, B = 64) every persistent BPTT launch carries ONE layer - word_rnn's blocks, then vid_rnn's -
 *                               on half of the compute units, with dW_o, the dh1 GEMMs and word_rnn's weight gradients on the other half;
 *                               0: two layers per launch, GEMM parts only beside the first / last (one-layer) launch
 *   pad_min_batch   33 (1..64)  ragged batches (B % 64 != 0) of at least this many rows - a greedy decode: three quarters of it - are
 *                               padded to a multiple of 64 inside the workspace (s2vt_padded_batch); smaller ones run as they
 *                               are, launches per timestep (faster there: profiles/round5_ragged_batches.txt)
 *   gemv            1 | 2 | 0   the launch-per-timestep forward step (s2vt_lstm_step_fwd and the drivers built on it) as gate
 *                               GEMVs - h staged in LDS, weight rows streamed to registers, wavefront shuffle reductions
 *                               (csrc/lstm_gemv.hip) - instead of the 16-row fp32-MFMA tile kernel: 1 = at B <= 4 (where it
 *                               measured faster), 2 = at every B <= 8, 0 = never
 * Do not change gemm_mode / persist / pipe_block between a forward and its backward (the backward refuses). */
int32_t s2vt_set_option(const char* name, int32_t value);
int32_t s2vt_option_count(void);
const char* s2vt_option_name(int32_t index);

/* Arithmetic of the batched GEMMs inside the whole-path train drivers: 0 = fp32-input MFMA (exact fp32 products),
 * 3 = split precision (3 bf16 planes per operand, six plane products on the bf16 matrix cores: fp32-equivalent to
 * ~2^-23 relative; default when B % 64 == 0, env S2VT_GEMM_MODE).  Returns the previous mode; a negative argument only queries.  Call it between a
 * forward and its backward only if you also re-query the workspace size. */
int s2vt_set_gemm_mode(int32_t mode);

/* Layer pipelining of the whole-path drivers: the two LSTM layers run as a software pipeline on two streams in
 * blocks of `steps` timesteps (default 32, or env S2VT_PIPE_BLOCK; the persistent bf16 schedule evens the default out over
 * the L frames - 27 at L = 80 - because its launches pair a block of one layer with a block of the other); 0 runs everything
 * on the caller's stream (kernels then never overlap: used to time kernels in isolation).  Returns the previous value. */
int s2vt_set_pipeline_block(int32_t steps);
/* Schedule of the token-dependent decode steps of s2vt_greedy_decode[_cached] on the plane path (the loop of
 * /root/reference/S2VTModel.py:98-107): 1 (default; env S2VT_DECODE_FUSED) = per step ONE launch that computes out_linear +
 * argmax of step t and, as extra row blocks, h_t W_hh^T of step t+1 (which does not depend on the token), then a one-thread-
 * per-cell launch that adds the token's gate-table row and updates the cell; 0 = a step kernel and an argmax kernel per step,
 * the two batch halves as independent chains on two streams.  Same ids either way.  Returns the previous value; any other
 * argument only queries. */
int s2vt_set_decode_schedule(int32_t schedule);
/* The encode phase of a decode alone - /root/reference/S2VTModel.py:56-60 (mode='beam_search': vid_rnn over the L frames, word_rnn
 * over the padded vid_out) - on the plane path, with the weight-derived images in the caller's cache as in
 * s2vt_greedy_decode_cached (cache_valid == 0: filled here, every image a decode or a beam search of these weights reads).
 * workspace: s2vt_decode_workspace_bytes(d).  Out: vid_h, vid_c, word_h, word_c [B, H], the states after frame L-1 that
 * S2VT.beam_search (:149) starts from.  Shapes the persistent split-precision recurrence does not take (B % 64, H > 1024,
 * fp32-MFMA mode) return S2VT_ERR_ARG. */
int s2vt_decode_encode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, void* workspace, size_t workspace_bytes,
                              void* cache, size_t cache_bytes, int32_t cache_valid, float* vid_h, float* vid_c, float* word_h,
                              float* word_c, float* gx_dec, int32_t depth, void* stream);
/* gx_dec (nullable) [depth][B][4H], depth <= L-1: vid_rnn's decode-phase steps take no input and see no token
 * (/root/reference/S2VTModel.py:208-210 runs one per depth inside the search loop), so the first `depth` of them run here in one
 * persistent launch and their half of word_rnn's gate input (h1_t W_v^T + both biases) comes out of one GEMM.
 * s2vt_beam_step_gx is s2vt_beam_step_cached for a depth whose slice gx_dec[depth - 1] replaces the vid_rnn state arguments. */
int s2vt_beam_step_gx(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                      const int32_t* tok, const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out,
                      float* word_c_out, int32_t* top_ix, float* top_lp, void* workspace, size_t workspace_bytes, void* cache,
                      size_t cache_bytes, void* stream);
/* 1 if the internal side stream was verified to execute concurrently with the caller's stream (it is chosen by a
 * one-time calibration at the first pipelined call: HIP may map two streams onto one hardware queue), 0 if no
 * candidate overlapped (the drivers still run, serially), -1 before the first pipelined call. */
int s2vt_pipeline_overlaps(void);

/* Launch-sequence capture: with on = 1 (or env S2VT_GRAPH=1) the ~350 launches of an s2vt_train_forward / s2vt_train_backward
 * call of the plane drivers (B % 64 == 0) are captured into a hipGraph the second time the same argument set - every pointer,
 * dims, modes, stream - is seen, and replayed with one hipGraphLaunch from then on (at most 8 executables are cached).  Results
 * are those of the eager sequence bit for bit; s2vt_backward_wait_grads(0 / 1) then completes with the whole backward (the
 * gradient all-reduce follows it instead of overlapping it).  Off by default; not active while s2vt_prof_enable(1).  Returns the previous
 * setting; a negative argument only queries.  s2vt_graph_stats: graphs captured / launches replayed so far. */
int s2vt_set_graph_mode(int32_t on);
int s2vt_graph_stats(int64_t* captures, int64_t* replays);

/* Test support (tests/test_gpu_kernels.py: co-residency of the persistent recurrence): launches `workgroups` one-wave
 * workgroups that each hold `lds_bytes` (<= 160 KB) of LDS and spin for `microseconds` (<= 5 s) - a stand-in for a foreign
 * kernel (an RCCL all-reduce on a communication stream, another tenant of the GPU) sitting on the compute units. */
int s2vt_test_occupy_cus(int32_t workgroups, int32_t lds_bytes, int64_t microseconds, void* stream);
/* Test support: while microseconds > 0, every launch the train backward driver issues through the Lane helpers
 * (psplit, pdual, pgemm, pgemm_tt, colsum_finish) on the selected lanes (bit 0: the caller's stream, bit 1: the side
 * lane) is preceded on the same stream by one occupy_kernel workgroup (no LDS) that spins for `microseconds`.  It makes a
 * late producer deterministically late (tests/test_gpu_grad_release.py: a gradient group released before its last write is
 * then caught on every run).  lanes 0..3, microseconds 0..5e6, else an error; 0 (the default) turns it off and costs nothing. */
int s2vt_test_lane_delay(int32_t lanes, int64_t microseconds);

/* ---------------------------------------------------------------- live kernel timing (bench.py)
 * When enabled, launch sites bracket kernels of one kind with hipEvents on the launch stream.
 * kinds: 0 gemm, 1 lstm_step_fwd (whole sequence loop), 2 lstm_step_bwd (whole sequence loop),
 *        3 ce, 4 logits_argmax, 5 gemm launches planned for PART of the compute units (option corun: beside a one-layer
 *        persistent launch; kind 0 counts only the GEMMs that have the device to themselves). */
int s2vt_prof_enable(int32_t on);
/* Synchronises the recorded events; returns summed milliseconds and launch count for `kind`. */
int s2vt_prof_read(int32_t kind, double* total_ms, int64_t* launches);
/* Milliseconds during which at least one bracket of `kind` was open (union of the intervals over both lanes): brackets of
 * one kind overlap where the two lanes run the same kind of kernel side by side, and the sum above counts that time twice. */
int s2vt_prof_read_busy(int32_t kind, double* busy_ms);
int s2vt_prof_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* S2VT_HIP_H */
