// Per-op entry points of include/s2vt_hip.h: the pieces the whole-path drivers are built from (criterion, GEMMs, plane split,
// feature projection, timestep and sequence kernels), exported for tests, profiling and reuse (Att_Baseline).
#include "api_internal.h"

using namespace s2vt;

extern "C" {

// ------------------------------------------------------------------ loss
// torch.optim.Adam.step() of train.py:126 over flat buffers (see adam_flat in misc.hip)
int s2vt_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                   double eps, int64_t step, void* stream) {
    return adam_flat((hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step);
}

// what stands around it: the fp64 gradient norm with its clip record, and the step that clips, decays and skips by that record (optim.hip)
size_t s2vt_grad_norm_workspace_bytes(int64_t n) { return grad_norm_workspace_bytes(n); }
int s2vt_grad_norm(const float* grads, int64_t n, double max_norm, int32_t skip_nonfinite, void* workspace, size_t workspace_bytes,
                   void* record, void* stream) {
    static_assert(sizeof(ClipRecord) == sizeof(s2vt_clip_record) && GN_CHUNK == S2VT_GRAD_NORM_CHUNK && ADAM_MAX_SEGS == S2VT_ADAM_MAX_SEGMENTS,
                  "kernels.h and s2vt_hip.h state the same record and constants");
    return grad_norm((hipStream_t)stream, grads, n, max_norm, skip_nonfinite, workspace, workspace_bytes, static_cast<ClipRecord*>(record));
}
int s2vt_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                           double beta2, double eps, int64_t step, double weight_decay, int32_t decoupled, const int64_t* seg_end,
                           const int32_t* seg_decay, int32_t n_seg, int32_t skip_nonfinite, const void* record, void* stream) {
    return adam_flat_clipped((hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, weight_decay, decoupled,
                             seg_end, seg_decay, n_seg, skip_nonfinite, static_cast<const ClipRecord*>(record));
}

int s2vt_mean_ce_forward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target,
                         int64_t target_ld, float* lse, float* rowloss, float* loss_out, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && V > 0, "s2vt_mean_ce_forward: bad dims");
    hipStream_t st = (hipStream_t)stream;
    // target ids outside [0, V): flagged on the device, reported like the embedding's (s2vt_check_async_error)
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    {
        ProfScope ps(st, K_CE, 1);
        if ((rc = mean_ce_fwd(st, logits, (int64_t)B * Lm1, V, target, Lm1, target_ld, lse, rowloss, loss_out, flags.p)))
            return rc;
    }
    return flags.close(st, 2);
}
int s2vt_mean_ce_backward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target,
                          int64_t target_ld, const float* lse, const float* gout, float* dlogits, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && V > 0, "s2vt_mean_ce_backward: bad dims");
    ProfScope ps((hipStream_t)stream, K_CE, 1);
    return mean_ce_bwd((hipStream_t)stream, logits, (int64_t)B * Lm1, V, target, Lm1, target_ld, lse, gout, dlogits);
}

// MaskCriterion.forward as ONE call (utils.py:13-26): the per-row CE kernel, then a single workgroup that forms the mean, weights it
// with mask[:, 1:] product by product and divides by the mask's sum - the reference's arithmetic (NaN for an all-zero mask) without
// the dozen elementwise / reduction launches the host framework spends on those three lines.  out3 = {loss, mean_ce, sum(mask[:, 1:])}.
int s2vt_mask_criterion_forward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target, int64_t target_ld,
                                const float* mask, int64_t mask_ld, float* lse, float* rowloss, float* out3, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && V > 0 && mask_ld >= Lm1 + 1, "s2vt_mask_criterion_forward: bad dims");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    {
        ProfScope ps(st, K_CE, 1);
        if ((rc = mask_criterion_fwd(st, logits, (int64_t)B * Lm1, V, target, Lm1, target_ld, mask, mask_ld, lse, rowloss, out3, flags.p)))
            return rc;
    }
    return flags.close(st, 2);
}
// Its autograd down to the mean CE: g_ce[0] = sum_i (gout[0] / sum(w)) * w_i - the `gout` of s2vt_mean_ce_backward[_fused].
int s2vt_mask_criterion_backward(int32_t B, int32_t Lm1, const float* mask, int64_t mask_ld, const float* out3, const float* gout,
                                 float* g_ce, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && mask_ld >= Lm1 + 1, "s2vt_mask_criterion_backward: bad dims");
    return mask_criterion_bwd((hipStream_t)stream, mask, mask_ld, (int64_t)B * Lm1, Lm1, out3, gout, g_ce);
}

// RewardCriterion.forward (utils.py of this repository; the reference has no such loss): the per-row CE kernel, then one workgroup
// that weights the rows with weight[:, 1:] and divides by the number of non-zero weights.  out2 = {loss, norm}.
int s2vt_weighted_ce_forward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target, int64_t target_ld,
                             const float* weight, int64_t weight_ld, float* lse, float* rowloss, float* out2, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && V > 0 && target_ld >= Lm1 + 1 && weight_ld >= Lm1 + 1, "s2vt_weighted_ce_forward: bad dims");
    S2VT_REQUIRE(logits && target && weight && lse && rowloss && out2, "s2vt_weighted_ce_forward: null argument");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    {
        ProfScope ps(st, K_CE, 1);
        if ((rc = weighted_ce_fwd(st, logits, (int64_t)B * Lm1, V, target, Lm1, target_ld, weight, weight_ld, lse, rowloss, out2, flags.p)))
            return rc;
    }
    return flags.close(st, 2);
}
int s2vt_weighted_ce_backward(int32_t B, int32_t Lm1, int32_t V, const float* logits, const int64_t* target, int64_t target_ld,
                              const float* weight, int64_t weight_ld, const float* lse, const float* out2, const float* gout,
                              float* dlogits, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && V > 0 && target_ld >= Lm1 + 1 && weight_ld >= Lm1 + 1, "s2vt_weighted_ce_backward: bad dims");
    S2VT_REQUIRE(logits && target && weight && lse && out2 && gout && dlogits, "s2vt_weighted_ce_backward: null argument");
    ProfScope ps((hipStream_t)stream, K_CE, 1);
    return weighted_ce_bwd((hipStream_t)stream, logits, (int64_t)B * Lm1, V, target, Lm1, target_ld, weight, weight_ld, lse, out2, gout,
                           dlogits);
}

// ------------------------------------------------------------------ per-op entry points
int s2vt_gemm_f32(int32_t a_kmajor, int32_t b_kmajor, int32_t M, int32_t N, int32_t K, const float* A, int64_t lda,
                  const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int32_t accumulate,
                  void* stream) {
    return gemm((hipStream_t)stream, a_kmajor != 0, b_kmajor != 0, M, N, K, A, lda, ID, B, ldb, ID, C, ldc, ID, bias,
                accumulate != 0);
}

int s2vt_gemm_f32_splitk(int32_t a_kmajor, int32_t b_kmajor, int32_t M, int32_t N, int32_t K, const float* A,
                         int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                         int32_t accumulate, float* ws, size_t ws_floats, void* stream) {
    GemmWsScope gscope(ws, ws_floats);
    return gemm((hipStream_t)stream, a_kmajor != 0, b_kmajor != 0, M, N, K, A, lda, ID, B, ldb, ID, C, ldc, ID, bias,
                accumulate != 0);
}

int s2vt_split_planes(int32_t nplanes, int32_t transpose, const float* in, int64_t ld, int32_t rows, int32_t cols,
                      uint16_t* out, int64_t ldo, int32_t kpad, int32_t out_rows_pad, void* stream) {
    return split_planes((hipStream_t)stream, nplanes, transpose != 0, in, ld, ID, rows, cols, out, ldo, kpad, out_rows_pad);
}

int s2vt_gemm_bf16_nt(int32_t nplanes, int32_t M, int32_t N, int32_t K, const uint16_t* A, int64_t lda, const uint16_t* B,
                      int64_t ldb, float* C, int64_t ldc, const float* bias, int32_t accumulate, float* ws,
                      size_t ws_floats, void* stream) {
    ProfScope ps((hipStream_t)stream, K_GEMM, 1);
    return gemm_bf16_nt((hipStream_t)stream, nplanes, M, N, K, A, lda, B, ldb, C, ldc, ID, bias, accumulate != 0, ws,
                        ws_floats);
}

int s2vt_gemm_bf16_tt(int32_t nplanes, int32_t M, int32_t N, int32_t K, const uint16_t* A, int64_t lda, const uint16_t* B,
                      int64_t ldb, float* C, int64_t ldc, const float* bias, int32_t accumulate, float* ws, size_t ws_floats,
                      void* stream) {
    S2VT_REQUIRE(nplanes == 3 || nplanes == 1, "s2vt_gemm_bf16_tt: planes must be 1 or 3");
    ProfScope ps((hipStream_t)stream, K_GEMM, 1);
    if (nplanes == 1) return gemm_b1_tt((hipStream_t)stream, M, N, K, A, lda, B, ldb, C, ldc, ID, bias, accumulate != 0, ws, ws_floats);
    return gemm_x3_tt((hipStream_t)stream, M, N, K, A, lda, B, ldb, C, ldc, ID, bias, accumulate != 0, ws, ws_floats);
}

int s2vt_feat_proj_fwd(const s2vt_dims* d, const float* feats, const float* w, const float* bias, float* x1,
                       void* stream) {
    S2VT_REQUIRE(dims_ok(d) && feats && w && x1, "s2vt_feat_proj_fwd: null/invalid argument");
    return gemm((hipStream_t)stream, true, true, d->B * d->L, d->H, d->F, feats, d->F, ID, w, d->F, ID, x1, d->H,
                perm(d->L, d->B), bias, false);
}

size_t s2vt_colsum_ws_floats(int64_t rows, int32_t cols) { return colsum_partial_floats(rows, cols); }

// ------------------------------------------------------------------ per-op entry points, test support
// The backward's gather / scatter / reorder pieces one at a time (tests/test_gpu_backward_aux.py): each forwards to the launch
// function the whole-path drivers call (kernels.h) after checking on the host what a launch would otherwise take on trust.
static bool rowmap_ok(const int32_t* idx, int32_t inner, int32_t outer, int64_t mapped_rows) {
    if (inner < 0 || outer < 0) return false;
    if (inner == 0) return outer == 0;
    return idx == nullptr && (int64_t)inner * outer == mapped_rows;       // a permutation of exactly the rows it maps
}
static RowMap rowmap(const int32_t* idx, int32_t inner, int32_t outer) { return RowMap{idx, inner, outer}; }

int s2vt_gemm_f32_mapped(int32_t a_kmajor, int32_t b_kmajor, int32_t M, int32_t N, int32_t K, const float* A, int64_t lda,
                         const int32_t* a_idx, int32_t a_inner, int32_t a_outer, const float* B, int64_t ldb, const int32_t* b_idx,
                         int32_t b_inner, int32_t b_outer, float* C, int64_t ldc, const int32_t* c_idx, int32_t c_inner,
                         int32_t c_outer, const float* bias, int32_t accumulate, float* ws, size_t ws_floats, int32_t splitk_cap,
                         void* stream) {
    S2VT_REQUIRE(M > 0 && N > 0 && K > 0 && A && B && C, "s2vt_gemm_f32_mapped: null operand or non-positive size (M=%d N=%d K=%d)", M, N, K);
    S2VT_REQUIRE(lda >= (a_kmajor ? K : M) && ldb >= (b_kmajor ? K : N) && ldc >= N,
                 "s2vt_gemm_f32_mapped: a row stride is shorter than the row it strides over");
    S2VT_REQUIRE(rowmap_ok(a_idx, a_inner, a_outer, a_kmajor ? M : K) && rowmap_ok(b_idx, b_inner, b_outer, b_kmajor ? N : K) &&
                     rowmap_ok(c_idx, c_inner, c_outer, M),
                 "s2vt_gemm_f32_mapped: bad row map (an index and a permutation together, or inner * outer != the mapped rows)");
    S2VT_REQUIRE(splitk_cap >= 0 && (ws != nullptr || ws_floats == 0), "s2vt_gemm_f32_mapped: bad split-K scratch or cap");
    // the cap reaches the launcher as the scratch size it may plan with: its own rule n * M * N > scratch ends the search
    size_t planned = ws ? ws_floats : 0;
    if (splitk_cap > 0 && (size_t)splitk_cap * M * N < planned) planned = (size_t)splitk_cap * M * N;
    ProfScope ps((hipStream_t)stream, K_GEMM, 1);
    return gemm_f32((hipStream_t)stream, a_kmajor != 0, b_kmajor != 0, M, N, K, A, lda, rowmap(a_idx, a_inner, a_outer), B, ldb,
                    rowmap(b_idx, b_inner, b_outer), C, ldc, rowmap(c_idx, c_inner, c_outer), bias, accumulate != 0, ws, planned);
}

size_t s2vt_embedding_grad_ws_ints(int64_t rows, int32_t V) {
    if (rows < 0 || V <= 0) return 0;
    return embedding_grad_ws_ints(rows, V);
}
int s2vt_embedding_grad(const float* d_rows, int64_t rows, int32_t E, const int32_t* tok, int32_t V, float* d_emb, int32_t* ws,
                        size_t ws_ints, void* stream) {
    S2VT_REQUIRE(rows >= 0 && rows <= 0x7fffffff && E > 0 && V > 0 && d_emb && ws && (rows == 0 || (d_rows && tok)),
                 "s2vt_embedding_grad: null argument or bad size (rows=%lld E=%d V=%d)", (long long)rows, E, V);
    S2VT_REQUIRE(ws_ints >= embedding_grad_ws_ints(rows, V), "s2vt_embedding_grad: scratch %zu < %zu ints", ws_ints,
                 embedding_grad_ws_ints(rows, V));
    return embedding_grad((hipStream_t)stream, d_rows, rows, E, tok, V, d_emb, ws);
}

int s2vt_gather_rows(const float* src, int64_t ld, const int32_t* idx, int64_t rows, int32_t cols, float* out, void* stream) {
    S2VT_REQUIRE(src && idx && out && rows > 0 && rows <= 65535 && cols > 0 && ld >= cols,
                 "s2vt_gather_rows: null argument or bad geometry (rows=%lld cols=%d ld=%lld)", (long long)rows, cols, (long long)ld);
    return gather_rows_f32((hipStream_t)stream, src, ld, idx, rows, cols, out);
}

int s2vt_transpose_f32(const float* in, int32_t rows, int32_t cols, float* out, void* stream) {
    S2VT_REQUIRE(in && out && in != out && rows > 0 && cols > 0 && (rows + 63) / 64 <= 65535,
                 "s2vt_transpose_f32: null argument or bad geometry (rows=%d cols=%d)", rows, cols);
    return transpose_f32((hipStream_t)stream, in, rows, cols, out);
}

int s2vt_colsum(const float* x, int64_t rows, int32_t cols, int64_t ld, float* ws, size_t ws_floats, float* out, int32_t accumulate,
                void* stream) {
    S2VT_REQUIRE(x && ws && out && rows > 0 && rows <= 64 * (int64_t)65535 && cols > 0 && ld >= cols,
                 "s2vt_colsum: null argument or bad geometry (rows=%lld cols=%d ld=%lld)", (long long)rows, cols, (long long)ld);
    S2VT_REQUIRE(ws_floats >= colsum_partial_floats(rows, cols), "s2vt_colsum: scratch %zu < %zu floats", ws_floats,
                 colsum_partial_floats(rows, cols));
    return colsum_f32((hipStream_t)stream, x, rows, cols, ld, ws, out, accumulate != 0);
}
int s2vt_colsum_finish(const float* partial, int32_t nchunks, int32_t cols, float* out, int32_t accumulate, void* stream) {
    S2VT_REQUIRE(partial && out && nchunks > 0 && cols > 0, "s2vt_colsum_finish: null argument or bad geometry (nchunks=%d cols=%d)",
                 nchunks, cols);
    return colsum_finish((hipStream_t)stream, partial, nchunks, cols, out, accumulate != 0);
}

int s2vt_split_planes_dual(int32_t nplanes, const float* in, int64_t ld, const int32_t* idx, int32_t inner, int32_t outer, int32_t rows,
                           int32_t cols, uint16_t* out_r, int64_t ldo_r, int32_t kpad_r, uint16_t* out_t, int64_t ldo_t, int32_t kpad_t,
                           float* colpart, const float* lse, const int64_t* target, int64_t target_ld, int32_t Lm1, const float* gout,
                           float* alpha_out, void* stream) {
    S2VT_REQUIRE((nplanes == 1 || nplanes == 3) && in && rows > 0 && cols > 0 && ld >= cols && (out_r || out_t || colpart),
                 "s2vt_split_planes_dual: null input, no output, or bad size (planes=%d rows=%d cols=%d)", nplanes, rows, cols);
    S2VT_REQUIRE(rowmap_ok(idx, inner, outer, rows), "s2vt_split_planes_dual: bad row map");
    auto image_ok = [&](const uint16_t* p, int64_t ldo, int kpad, int k) {
        return !p || (kpad % 64 == 0 && kpad >= k && kpad <= 64 * cdiv(k, 64) && ldo % 8 == 0 && ldo >= (int64_t)nplanes * kpad &&
                      (reinterpret_cast<uintptr_t>(p) & 15) == 0);
    };
    S2VT_REQUIRE(image_ok(out_r, ldo_r, kpad_r, cols) && image_ok(out_t, ldo_t, kpad_t, rows),
                 "s2vt_split_planes_dual: bad plane geometry (kpad = the k extent rounded up to 64, ldo >= planes * kpad, 16-byte aligned)");
    const bool with_ce = lse || target || gout || alpha_out;
    if (!with_ce) return split_planes_dual((hipStream_t)stream, nplanes, in, ld, rowmap(idx, inner, outer), rows, cols, out_r, ldo_r,
                                            kpad_r, out_t, ldo_t, kpad_t, colpart, nullptr);
    S2VT_REQUIRE(lse && target && gout && Lm1 > 0 && rows % Lm1 == 0 && target_ld >= Lm1 + 1 && !idx && inner == 0,
                 "s2vt_split_planes_dual: bad CE-gradient arguments (lse, target and gout together, rows = B * Lm1, no row map)");
    const CeGradArgs ce = {lse, target, gout, Lm1, target_ld, alpha_out};
    return split_planes_dual((hipStream_t)stream, nplanes, in, ld, ID, rows, cols, out_r, ldo_r, kpad_r, out_t, ldo_t, kpad_t, colpart, &ce);
}

int s2vt_feat_proj_bwd(const s2vt_dims* d, const float* feats, const float* w, const float* dx1, float* dw,
                       float* dbias, float* dfeats, float* colsum_ws, void* stream) {
    S2VT_REQUIRE(dims_ok(d) && feats && w && dx1 && dw && dbias && colsum_ws, "s2vt_feat_proj_bwd: null/invalid argument");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = gemm(st, false, false, d->H, d->F, d->L * d->B, dx1, d->H, ID, feats, d->F, perm(d->B, d->L), dw, d->F, ID,
                   nullptr, false)))
        return rc;
    if ((rc = colsum_f32(st, dx1, (int64_t)d->L * d->B, d->H, d->H, colsum_ws, dbias, false))) return rc;
    if (dfeats)
        return gemm(st, true, false, d->L * d->B, d->F, d->H, dx1, d->H, ID, w, d->F, ID, dfeats, d->F, perm(d->B, d->L),
                    nullptr, false);
    return 0;
}

int s2vt_lstm_step_fwd(int32_t B, int32_t H, const float* gx, const float* bias, const float* w_hh,
                       const float* h_prev, const float* c_prev, float* h_out, float* c_out, float* stash,
                       void* stream) {
    StepFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    a.h_prev = h_prev; a.ldh = H; a.w_hh = w_hh; a.ldw = H;
    a.gx = gx; a.ldgx = 4 * (int64_t)H; a.bias = bias;
    a.c_prev = c_prev; a.ldc = H;
    a.h_out = h_out; a.ldho = H; a.c_out = c_out; a.ldco = H;
    a.stash = stash; a.ldst = 4 * (int64_t)H;
    ProfScope ps((hipStream_t)stream, K_STEP_FWD, 1);
    return lstm_step_fwd((hipStream_t)stream, a);
}

int s2vt_lstm_step_fwd_token(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* h_prev,
                             const float* c_prev, const float* emb, const float* w_e, int64_t ldw_e, const int32_t* tok,
                             const unsigned long long* tok_packed, int32_t tok_const, float* h_out, float* c_out, void* stream) {
    S2VT_REQUIRE(B > 0 && H > 0 && E > 0 && V > 0 && gx && w_hh && emb && w_e && h_out && c_out && ldw_e >= E,
                 "s2vt_lstm_step_fwd_token: null/invalid argument");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    StepFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    a.h_prev = h_prev; a.ldh = H; a.w_hh = w_hh; a.ldw = H;
    a.x2 = emb; a.ldx2 = E; a.K2 = E; a.w2 = w_e; a.ldw2 = ldw_e;
    a.tok = TokenSrc{tok, tok_packed, tok_const, V, flags.p, {}};
    a.gx = gx; a.ldgx = 4 * (int64_t)H;
    a.c_prev = c_prev; a.ldc = H;
    a.h_out = h_out; a.ldho = H; a.c_out = c_out; a.ldco = H;
    {
        ProfScope ps(st, K_STEP_FWD, 1);
        if ((rc = lstm_step_fwd(st, a))) return rc;
    }
    return flags.close(st, 2);
}

// ------------------------------------------------------------------ the decode step's kernel forms, test support
// The forms of lstm_step_fwd / lstm_cell_pointwise / logits_argmax_x3 that only the decode drivers and the beam plane path fill in
// (api_decode.hip: decode_fused, decode_two_chains; api_beam.hip), one launch at a time (tests/test_gpu_decode_forms.py).  No kernel
// of their own: host checks, one args struct, one existing launch function.
static bool h_planes_ok(const uint16_t* p, int64_t ldhp, int32_t rows, int B, int H) {
    return !p || (ldhp >= 3 * (int64_t)pad64(H) && ldhp % 8 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0 &&
                  rows >= (int64_t)rows64((size_t)B));
}
// the arguments the fused table step and the stand-alone cell update share (everything but the recurrent segment and z)
static StepFwdArgs table_step_args(int32_t B, int32_t H, int32_t V, const float* gx, const int32_t* gx_idx, const float* bias,
                                   const float* gtab, int64_t ldtab, const int32_t* tok, const unsigned long long* tok_packed,
                                   int32_t tok_const, int* tok_err, const float* c_prev, float* h_out, float* c_out, float* stash,
                                   uint16_t* h_planes, int64_t ldhp) {
    StepFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    if (gtab) a.tok = TokenSrc{tok, tok_packed, tok_const, V, tok_err, {}};
    a.gx = gx; a.ldgx = 4 * (int64_t)H; a.gx_idx = gx_idx; a.bias = bias;
    a.gx_tab = gtab; a.ldtab = ldtab;
    a.c_prev = c_prev; a.ldc = H;
    a.h_out = h_out; a.ldho = H; a.c_out = c_out; a.ldco = H;
    a.stash = stash; a.ldst = 4 * (int64_t)H;
    a.h_planes = h_planes; a.ldhp = ldhp;
    return a;
}
// ... and the host checks on them (who: the entry's name)
static int table_step_check(const char* who, int32_t B, int32_t H, int32_t V, const float* gx, const int32_t* gx_idx, const float* bias,
                            const float* gtab, int64_t ldtab, const float* h_out, const float* c_out, const uint16_t* h_planes, int64_t ldhp,
                            int32_t hp_rows) {
    S2VT_REQUIRE(B > 0 && H > 0 && h_out && c_out && (gx || bias), "%s: null output, neither gx nor bias, or bad size (B=%d H=%d)", who, B, H);
    S2VT_REQUIRE(!gx_idx || gx, "%s: gx_idx names rows of gx, which is null", who);
    S2VT_REQUIRE(!gtab || (V > 0 && ldtab >= 4 * (int64_t)H), "%s: a gate table needs V > 0 rows of at least 4H floats (V=%d ldtab=%lld)", who, V,
                 (long long)ldtab);
    S2VT_REQUIRE(h_planes_ok(h_planes, ldhp, hp_rows, B, H),
                 "%s: bad h-plane image (ldhp >= 3 * pad64(H), ldhp %% 8 == 0, 16-byte aligned, whole 64-row blocks for B rows)", who);
    return 0;
}

int s2vt_lstm_step_fwd_table(int32_t B, int32_t H, int32_t V, const float* gx, const int32_t* gx_idx, const float* bias, const float* gtab,
                             int64_t ldtab, const int32_t* tok, const unsigned long long* tok_packed, int32_t tok_const, const float* w_hh,
                             const float* h_prev, const float* c_prev, float* h_out, float* c_out, float* stash, uint16_t* h_planes,
                             int64_t ldhp, int32_t hp_rows, float* z_out, int64_t ldz, int32_t contract_only, void* stream) {
    if (contract_only) {
        S2VT_REQUIRE(B > 0 && H > 0 && w_hh && h_prev && z_out && ldz >= 4 * (int64_t)H,
                     "s2vt_lstm_step_fwd_table: a contraction-only step needs w_hh, h_prev and z_out rows of at least 4H floats (ldz=%lld)",
                     (long long)ldz);
        StepFwdArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.H = H;
        a.h_prev = h_prev; a.ldh = H; a.w_hh = w_hh; a.ldw = H;
        a.z_out = z_out; a.ldz = ldz;
        ProfScope ps((hipStream_t)stream, K_STEP_FWD, 1);
        return lstm_step_fwd((hipStream_t)stream, a);
    }
    int rc;
    if ((rc = table_step_check("s2vt_lstm_step_fwd_table", B, H, V, gx, gx_idx, bias, gtab, ldtab, h_out, c_out, h_planes, ldhp, hp_rows))) return rc;
    S2VT_REQUIRE(!z_out, "s2vt_lstm_step_fwd_table: z_out is the output of contract_only = 1");
    S2VT_REQUIRE(!h_prev || w_hh, "s2vt_lstm_step_fwd_table: h_prev without w_hh");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    if ((rc = flags.open(st))) return rc;
    StepFwdArgs a = table_step_args(B, H, V, gx, gx_idx, bias, gtab, ldtab, tok, tok_packed, tok_const, flags.p, c_prev, h_out, c_out,
                                    stash, h_planes, ldhp);
    a.h_prev = h_prev; a.ldh = H; a.w_hh = w_hh; a.ldw = H;
    {
        ProfScope ps(st, K_STEP_FWD, 1);
        if ((rc = lstm_step_fwd(st, a))) return rc;
    }
    return flags.close(st, 2);
}

int s2vt_lstm_cell_pointwise(int32_t B, int32_t H, int32_t V, const float* gx, const int32_t* gx_idx, const float* bias, const float* gtab,
                             int64_t ldtab, const int32_t* tok, const unsigned long long* tok_packed, int32_t tok_const, const float* z,
                             int64_t ldz, const float* c_prev, float* h_out, float* c_out, float* stash, uint16_t* h_planes, int64_t ldhp,
                             int32_t hp_rows, void* stream) {
    int rc;
    if ((rc = table_step_check("s2vt_lstm_cell_pointwise", B, H, V, gx, gx_idx, bias, gtab, ldtab, h_out, c_out, h_planes, ldhp, hp_rows))) return rc;
    S2VT_REQUIRE(z && ldz >= 4 * (int64_t)H, "s2vt_lstm_cell_pointwise: z is null or its rows are shorter than 4H floats (ldz=%lld)", (long long)ldz);
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    if ((rc = flags.open(st))) return rc;
    StepFwdArgs a = table_step_args(B, H, V, gx, gx_idx, bias, gtab, ldtab, tok, tok_packed, tok_const, flags.p, c_prev, h_out, c_out,
                                    stash, h_planes, ldhp);
    a.z_out = const_cast<float*>(z); a.ldz = ldz;            // (the cell update reads it)
    {
        ProfScope ps(st, K_STEP_FWD, 1);
        if ((rc = lstm_cell_pointwise(st, a))) return rc;
    }
    return flags.close(st, 2);
}

int s2vt_argmax_x3_planes(int32_t B, int32_t V, int32_t K, const uint16_t* W, int64_t ldw, int32_t w_rows, const uint16_t* Hp, int64_t ldh,
                          int32_t kpad_h, int32_t hp_rows, const float* bias, unsigned long long* packed, const uint16_t* W2, int64_t ldw2,
                          int32_t kpad_w2, int32_t w2_rows, int32_t M2, float* z, int64_t ldz, int32_t with_logits, int32_t sample,
                          float temperature, uint64_t seed, int32_t step, int32_t row0, void* stream) {
    S2VT_REQUIRE(B > 0 && V > 0 && K > 0 && K % 64 == 0 && W && Hp && packed && M2 >= 0,
                 "s2vt_argmax_x3_planes: null argument or bad size (B=%d V=%d K=%d M2=%d)", B, V, K, M2);
    S2VT_REQUIRE(kpad_h == K && (M2 == 0 || kpad_w2 == K), "s2vt_argmax_x3_planes: the images must share one padded k (K=%d, h %d, W2 %d)", K,
                 kpad_h, kpad_w2);
    S2VT_REQUIRE(w_rows >= (int64_t)rows64((size_t)V) && hp_rows >= (int64_t)rows64((size_t)B) && (M2 == 0 || w2_rows >= (int64_t)rows64((size_t)M2)),
                 "s2vt_argmax_x3_planes: an image has fewer rows than the 64-row blocks the launch reads (W %d, h %d, W2 %d)", w_rows, hp_rows,
                 w2_rows);
    S2VT_REQUIRE(with_logits || M2 > 0, "s2vt_argmax_x3_planes: with_logits = 0 needs a second image (M2 > 0)");
    S2VT_REQUIRE(!sample || (with_logits && step >= 0 && row0 >= 0), "s2vt_argmax_x3_planes: a draw needs the logits, step >= 0 and row0 >= 0");
    S2VT_REQUIRE(!sample || temperature_ok(temperature), "s2vt_argmax_x3_planes: temperature and 1 / temperature must be finite and > 0 (got %g)",
                 (double)temperature);
    ArgmaxX3Args ax;
    memset(&ax, 0, sizeof(ax));
    ax.B = B; ax.V = V; ax.K = K;
    ax.W = W; ax.ldw = ldw; ax.Hp = Hp; ax.ldh = ldh;
    ax.bias = bias; ax.packed = packed;
    if (M2 > 0) { ax.W2 = W2; ax.ldw2 = ldw2; ax.M2 = M2; ax.z = z; ax.ldz = ldz; }
    ax.v_off = with_logits ? 0 : cdiv(V, 64);
    GumbelArgs g{};
    if (sample) g = gumbel_args(temperature, seed, (uint32_t)step, (uint32_t)row0, (uint32_t)row0 + (uint32_t)B);
    ProfScope ps((hipStream_t)stream, K_ARGMAX, 1);
    return logits_argmax_x3((hipStream_t)stream, ax, sample ? &g : nullptr);       // (geometry of ld / alignment / ldz: the launcher's own checks)
}

int s2vt_lstm_step_bwd(int32_t B, int32_t H, const float* dg_next, const float* w_hh_t, const float* dh_out,
                       const float* stash, const float* c, const float* c_prev, float* dc, int32_t dc_is_zero,
                       float* dg, void* stream) {
    StepBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    a.dg_next = dg_next; a.lddg = 4 * (int64_t)H; a.w_hh_t = w_hh_t; a.ldwt = 4 * (int64_t)H;
    a.dh_out = dh_out; a.lddho = H;
    a.stash = stash; a.ldst = 4 * (int64_t)H;
    a.c = c; a.ldc = H; a.c_prev = c_prev; a.ldcp = H;
    a.dc = dc; a.lddc = H; a.dc_is_zero = dc_is_zero;
    a.dg = dg; a.lddg_out = 4 * (int64_t)H;
    ProfScope ps((hipStream_t)stream, K_STEP_BWD, 1);
    return lstm_step_bwd((hipStream_t)stream, a);
}

int s2vt_lstm_seq_fwd(int32_t T, int32_t B, int32_t H, const float* gx, int32_t n_gx, const float* bias,
                      const float* w_hh, float* h_all, float* c_all, float* stash, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && w_hh && h_all && c_all && n_gx >= 0 && n_gx <= T,
                 "s2vt_lstm_seq_fwd: bad arguments");
    S2VT_REQUIRE(n_gx == 0 || gx, "s2vt_lstm_seq_fwd: gx missing");
    S2VT_REQUIRE(n_gx == T || bias, "s2vt_lstm_seq_fwd: bias needed for steps without gx");
    S2VT_REQUIRE(stash == nullptr || stash == gx || n_gx == 0,
                 "s2vt_lstm_seq_fwd: stash must alias gx (in-place) or gx must be absent");
    hipStream_t st = (hipStream_t)stream;
    if (stash) return seq_fwd(st, 0, T, B, H, stash, n_gx, bias, w_hh, h_all, c_all, true);
    return seq_fwd(st, 0, T, B, H, const_cast<float*>(gx), n_gx, bias, w_hh, h_all, c_all, false);
}

int s2vt_lstm_seq_bwd(int32_t T, int32_t B, int32_t H, const float* w_hh, const float* dh_out, int32_t dh_first,
                      const float* c_all, float* stash_dg, float* w_hh_t, float* dc, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && w_hh && c_all && stash_dg && w_hh_t && dc, "s2vt_lstm_seq_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = transpose_f32(st, w_hh, 4 * H, H, w_hh_t))) return rc;
    return seq_bwd(st, T, 0, T, B, H, w_hh_t, dh_out, dh_first, c_all, stash_dg, dc);
}

// bf16-operand layer forward (config 3 arithmetic) as its own entry point: kernel-level parity tests and benchmarks.
// workspace: [err int x64][sync][W_hh bf16 rows][h bf16 rows]
struct SeqBf16WS { int* err; unsigned int* sync; PB wb, hb; size_t bytes; };
static SeqBf16WS carve_seq_bf16(int T, int B, int H, void* base) {
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    SeqBf16WS w;
    w.err = c.take<int>(64);
    w.sync = c.take<unsigned int>(lstm_persist_sync_bytes() / sizeof(unsigned int));
    w.wb = take_planes(c, (size_t)4 * H, H, 1);
    w.hb = take_planes(c, (size_t)T * B, H, 1);
    w.bytes = align_up(c.off, 256);
    return w;
}
size_t s2vt_lstm_seq_bf16_workspace_bytes(int32_t T, int32_t B, int32_t H) {
    if (T <= 0 || B <= 0 || H <= 0) return 0;
    return carve_seq_bf16(T, B, H, nullptr).bytes;
}
static int seq_bf16_prepare(hipStream_t st, const SeqBf16WS& w, int T, int B, int H, const float* w_hh) {
    int rc;
    if ((rc = fill_zero(st, w.err, 64 * sizeof(int)))) return rc;
    if ((rc = split_planes(st, 1, false, w_hh, H, ID, 4 * H, H, w.wb.p, w.wb.ld, w.wb.kpad, (int)rows64((size_t)4 * H)))) return rc;
    return zero_pad_cols_u16(st, w.hb.p, (int64_t)T * B, w.hb.ld, H, w.hb.kpad);
}
static SeqFwdBf16Args seq_bf16_args(const SeqBf16WS& w, int B, int H, int t0, int t1, float* gx_stash, int n_gx,
                                    const float* bias, float* h_all, float* c_all) {
    SeqFwdBf16Args a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H; a.Kp = w.hb.kpad;
    a.t0 = t0; a.t1 = t1; a.n_gx = n_gx;
    a.wb = w.wb.p; a.ldwb = w.wb.ld;
    a.hb = w.hb.p; a.ldhb = w.hb.ld;
    a.gx_stash = gx_stash; a.bias = bias;
    a.h_all = h_all; a.c_all = c_all;
    a.sync = w.sync; a.err = w.err;
#ifdef S2VT_EXPERIMENT_STAMPS
    a.stamps = g_xstamps; a.stamp_block = g_xstamp_block;
#endif
    return a;
}

int s2vt_lstm_seq_fwd_bf16(int32_t T, int32_t B, int32_t H, float* gx_stash, int32_t n_gx, const float* bias,
                           const float* w_hh, float* h_all, float* c_all, void* workspace, size_t workspace_bytes,
                           int32_t persistent, int32_t block, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && gx_stash && w_hh && h_all && c_all && workspace && n_gx >= 0 && n_gx <= T,
                 "s2vt_lstm_seq_fwd_bf16: bad arguments");
    S2VT_REQUIRE(n_gx == T || bias, "s2vt_lstm_seq_fwd_bf16: bias needed for steps without gx");
    const SeqBf16WS w = carve_seq_bf16(T, B, H, workspace);
    S2VT_REQUIRE(workspace_bytes >= w.bytes, "s2vt_lstm_seq_fwd_bf16: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    // (refused before prepare: a shape the persistent kernel does not run launches nothing at all)
    S2VT_REQUIRE(!persistent || lstm_seq_fwd_bf16_persist_supported(B, H, w.hb.kpad),
                 "s2vt_lstm_seq_fwd_bf16: shape B=%d H=%d (Kp=%d) not supported by the persistent kernel (B %% 32, Kp <= 1024)", B, H, w.hb.kpad);
    if ((rc = seq_bf16_prepare(st, w, T, B, H, w_hh))) return rc;
    if (!persistent) return seq_fwd_bf16(st, 0, T, B, H, gx_stash, n_gx, bias, w.wb, w.hb, h_all, c_all);
    const int blk = block > 0 ? block : T;
    for (int t0 = 0; t0 < T; t0 += blk) {
        const int t1 = (t0 + blk < T) ? t0 + blk : T;
        ProfScope ps(st, K_STEP_FWD, t1 - t0);
        if ((rc = lstm_seq_fwd_bf16_persist(st, seq_bf16_args(w, B, H, t0, t1, gx_stash, n_gx, bias, h_all, c_all)))) return rc;
    }
    return 0;
}

// Two independent layers of the same shape, every block of timesteps of both in ONE persistent launch (the schedule the
// whole-path driver uses for vid_rnn block k+1 next to word_rnn block k); workspace = 2 x the single-layer size.
int s2vt_lstm_seq_fwd_bf16_pair(int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                                const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1,
                                float* h_all0, float* h_all1, float* c_all0, float* c_all1, void* workspace,
                                size_t workspace_bytes, int32_t block, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && gx_stash0 && gx_stash1 && w_hh0 && w_hh1 && h_all0 && h_all1 && c_all0 && c_all1 &&
                     workspace && n_gx >= 0 && n_gx <= T && (n_gx == T || (bias0 && bias1)),
                 "s2vt_lstm_seq_fwd_bf16_pair: bad arguments");
    const size_t one = carve_seq_bf16(T, B, H, nullptr).bytes;
    S2VT_REQUIRE(workspace_bytes >= 2 * one, "s2vt_lstm_seq_fwd_bf16_pair: workspace %zu < %zu bytes", workspace_bytes, 2 * one);
    const SeqBf16WS w0 = carve_seq_bf16(T, B, H, workspace);
    const SeqBf16WS w1 = carve_seq_bf16(T, B, H, reinterpret_cast<char*>(workspace) + one);
    S2VT_REQUIRE(lstm_seq_fwd_bf16_persist_supported(B, H, w0.hb.kpad),
                 "s2vt_lstm_seq_fwd_bf16_pair: shape B=%d H=%d (Kp=%d) not supported by the persistent kernel (B %% 32, Kp <= 1024)", B, H, w0.hb.kpad);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = seq_bf16_prepare(st, w0, T, B, H, w_hh0))) return rc;
    if ((rc = seq_bf16_prepare(st, w1, T, B, H, w_hh1))) return rc;
    const int blk = block > 0 ? block : T;
    for (int t0 = 0; t0 < T; t0 += blk) {
        const int t1 = (t0 + blk < T) ? t0 + blk : T;
        ProfScope ps(st, K_STEP_FWD, 2 * (t1 - t0));
        SeqFwdBf16Args a1 = seq_bf16_args(w1, B, H, t0, t1, gx_stash1, n_gx, bias1, h_all1, c_all1);
        a1.err = w0.err;
        if ((rc = lstm_seq_fwd_bf16_persist2(st, seq_bf16_args(w0, B, H, t0, t1, gx_stash0, n_gx, bias0, h_all0, c_all0), &a1)))
            return rc;
    }
    return 0;
}

// bf16-operand BPTT of one layer as its own entry point (kernel-level parity tests and benchmarks).
// workspace: [err int x64][sync][W_hh^T bf16 rows][dG bf16 rows][dc]
struct SeqBwdBf16WS { int* err; unsigned int* sync; PB wt, dgb; float* dc; size_t bytes; };
static SeqBwdBf16WS carve_seq_bwd_bf16(int T, int B, int H, void* base) {
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    SeqBwdBf16WS w;
    w.err = c.take<int>(64);
    w.sync = c.take<unsigned int>(lstm_persist_sync_bytes() / sizeof(unsigned int));
    w.wt = take_planes(c, (size_t)H, (size_t)4 * H, 1);
    w.dgb = take_planes(c, (size_t)T * B, (size_t)4 * H, 1);
    w.dc = c.take<float>((size_t)B * H);
    w.bytes = align_up(c.off, 256);
    return w;
}
size_t s2vt_lstm_seq_bwd_bf16_workspace_bytes(int32_t T, int32_t B, int32_t H) {
    if (T <= 0 || B <= 0 || H <= 0) return 0;
    return carve_seq_bwd_bf16(T, B, H, nullptr).bytes;
}
static int seq_bwd_bf16_prepare(hipStream_t st, const SeqBwdBf16WS& w, int T, int B, int H, const float* w_hh) {
    int rc;
    if ((rc = fill_zero(st, w.err, 64 * sizeof(int)))) return rc;
    if ((rc = split_planes(st, 1, true, w_hh, H, ID, 4 * H, H, w.wt.p, w.wt.ld, w.wt.kpad, (int)rows64((size_t)H)))) return rc;
    return zero_pad_cols_u16(st, w.dgb.p, (int64_t)T * B, w.dgb.ld, 4 * H, w.dgb.kpad);
}
// persistent: 0 = one launch per timestep, 1 = one persistent launch per `block` steps (0 = all T).
// stash_dg [T*B,4H]: activated gates in, fp32 dG out; dh_out rows for steps >= dh_first (nullable).
int s2vt_lstm_seq_bwd_bf16(int32_t T, int32_t B, int32_t H, const float* w_hh, const float* dh_out, int32_t dh_first,
                           const float* c_all, float* stash_dg, void* workspace, size_t workspace_bytes,
                           int32_t persistent, int32_t block, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && w_hh && c_all && stash_dg && workspace && dh_first >= 0, "s2vt_lstm_seq_bwd_bf16: bad arguments");
    const SeqBwdBf16WS w = carve_seq_bwd_bf16(T, B, H, workspace);
    S2VT_REQUIRE(workspace_bytes >= w.bytes, "s2vt_lstm_seq_bwd_bf16: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    S2VT_REQUIRE(!persistent || lstm_seq_bwd_bf16_persist_supported(B, H, w.dgb.kpad),
                 "s2vt_lstm_seq_bwd_bf16: shape B=%d H=%d (Kp=%d) not supported by the persistent kernel (B %% 32, H %% 8, 4H <= 4096)", B, H,
                 w.dgb.kpad);
    if ((rc = seq_bwd_bf16_prepare(st, w, T, B, H, w_hh))) return rc;
    if (!persistent) return seq_bwd_bf16(st, T, 0, T, B, H, w.wt, dh_out, dh_first, c_all, stash_dg, w.dgb, w.dc);
    const int blk = block > 0 ? block : T;
    for (int t1 = T; t1 > 0; t1 -= blk) {
        const int t0 = (t1 - blk > 0) ? t1 - blk : 0;
        ProfScope ps(st, K_STEP_BWD, t1 - t0);
        if ((rc = lstm_seq_bwd_bf16_persist2(st, seq_bwd_bf16_args(T, t0, t1, B, H, w.wt, w.dgb, dh_out, dh_first, c_all, stash_dg,
                                                                  w.dc, w.sync, w.err), nullptr)))
            return rc;
    }
    return 0;
}
// two independent layers of one shape, every block of both in ONE persistent launch; workspace = 2 x the single-layer size
int s2vt_lstm_seq_bwd_bf16_pair(int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                                const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1,
                                float* stash_dg0, float* stash_dg1, void* workspace, size_t workspace_bytes, int32_t block,
                                void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && w_hh0 && w_hh1 && c_all0 && c_all1 && stash_dg0 && stash_dg1 && workspace && dh_first >= 0,
                 "s2vt_lstm_seq_bwd_bf16_pair: bad arguments");
    const size_t one = carve_seq_bwd_bf16(T, B, H, nullptr).bytes;
    S2VT_REQUIRE(workspace_bytes >= 2 * one, "s2vt_lstm_seq_bwd_bf16_pair: workspace %zu < %zu bytes", workspace_bytes, 2 * one);
    const SeqBwdBf16WS w0 = carve_seq_bwd_bf16(T, B, H, workspace);
    const SeqBwdBf16WS w1 = carve_seq_bwd_bf16(T, B, H, reinterpret_cast<char*>(workspace) + one);
    S2VT_REQUIRE(lstm_seq_bwd_bf16_persist_supported(B, H, w0.dgb.kpad),
                 "s2vt_lstm_seq_bwd_bf16_pair: shape B=%d H=%d (Kp=%d) not supported by the persistent kernel (B %% 32, H %% 8, 4H <= 4096)", B, H,
                 w0.dgb.kpad);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = seq_bwd_bf16_prepare(st, w0, T, B, H, w_hh0))) return rc;
    if ((rc = seq_bwd_bf16_prepare(st, w1, T, B, H, w_hh1))) return rc;
    const int blk = block > 0 ? block : T;
    for (int t1 = T; t1 > 0; t1 -= blk) {
        const int t0 = (t1 - blk > 0) ? t1 - blk : 0;
        ProfScope ps(st, K_STEP_BWD, 2 * (t1 - t0));
        const SeqBwdBf16Args a1 = seq_bwd_bf16_args(T, t0, t1, B, H, w1.wt, w1.dgb, dh_out1, dh_first, c_all1, stash_dg1, w1.dc, w1.sync, w0.err);
        if ((rc = lstm_seq_bwd_bf16_persist2(st, seq_bwd_bf16_args(T, t0, t1, B, H, w0.wt, w0.dgb, dh_out0, dh_first, c_all0, stash_dg0,
                                                                  w0.dc, w0.sync, w0.err), &a1)))
            return rc;
    }
    return 0;
}

// Test support: where the bf16 images lie inside the two workspaces above, straight from their carvers.
int s2vt_lstm_seq_bf16_layout(int32_t T, int32_t B, int32_t H, int32_t backward, int64_t* out) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && out, "s2vt_lstm_seq_bf16_layout: bad arguments");
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);      // (never dereferenced: the carvers only add offsets)
    PB w, r;
    if (backward) {
        const SeqBwdBf16WS ws = carve_seq_bwd_bf16(T, B, H, base);
        w = ws.wt; r = ws.dgb;
    } else {
        const SeqBf16WS ws = carve_seq_bf16(T, B, H, base);
        w = ws.wb; r = ws.hb;
    }
    out[0] = reinterpret_cast<char*>(w.p) - base; out[1] = w.ld; out[2] = w.kpad;
    out[3] = reinterpret_cast<char*>(r.p) - base; out[4] = r.ld; out[5] = r.kpad;
    return 0;
}

#ifdef S2VT_EXPERIMENT_STAMPS
extern "C" int s2vt_experiment_set_stamps(unsigned long long* buf, int block) { g_xstamps = buf; g_xstamp_block = block; return 0; }
#endif

// Which recurrence kernels the whole-path train drivers would run for (B, H) in the current modes:
// 0 = one launch per timestep, 1 = persistent bf16, 2 = persistent exact-fp32 MFMA, 3 = persistent split precision.
int s2vt_recurrence_plan(int32_t B, int32_t H, int32_t* fwd, int32_t* bwd) {
    S2VT_REQUIRE(B > 0 && H > 0 && fwd && bwd, "s2vt_recurrence_plan: bad arguments");
    const RecurrencePlan pl = train_recurrence_plan(B, H);
    *fwd = pl.fwd;
    *bwd = pl.bwd;
    return 0;
}

int s2vt_set_recurrence_mode(int32_t mode) {
    return option_set(O_PERSIST, mode < 0 ? -1 : (mode ? 1 : 0));
}

// split-precision persistent forward (lstm_persist_x3.hip) as its own entry point.
// workspace: [err int x64][sync A][sync B][W planes 0][W planes 1][h planes 0][h planes 1]
size_t s2vt_lstm_seq_x3_workspace_bytes(int32_t T, int32_t B, int32_t H) {
    if (T <= 0 || B <= 0 || H <= 0 || H > 1024 || !lstm_seq_fwd_x3_persist_supported(B, H)) return 0;      // 0: shape not supported
    const size_t Kp = (size_t)(H + 63) / 64 * 64;
    return 256 + 2 * lstm_persist_sync_bytes() + 2 * align_up(3 * 4 * (size_t)H * Kp * 2, 256) + 2 * align_up(3 * (size_t)T * B * Kp * 2, 256);
}
// One body for the entry point and its test-support form (s2vt_lstm_seq_fwd_x3_persist_emit): the latter also fills in the fields
// that otherwise only the train / decode drivers set - SeqFwdX3Args::hblk / ldhblk (h_t as the batched GEMMs' row image) and
// no_stash.  The image's requirements repeat prep_x so that they are refused here, before any device call.
struct X3Image { unsigned short* p; int64_t ld; };
static bool x3_image_ok(const X3Image& im, int B, int64_t k) {
    return !im.p || (B % 64 == 0 && im.ld >= 3 * ((k + 63) / 64 * 64) && im.ld % 8 == 0 && (reinterpret_cast<uintptr_t>(im.p) & 15) == 0);
}
static int seq_fwd_x3_entry(const char* who, int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                            const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1, float* h_all0,
                            float* h_all1, float* c_all0, float* c_all1, X3Image hblk0, X3Image hblk1, int32_t no_stash,
                            int32_t block, void* workspace, size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && gx_stash0 && w_hh0 && h_all0 && c_all0 && workspace && n_gx >= 0 && n_gx <= T &&
                     (n_gx == T || bias0) && (no_stash == 0 || no_stash == 1), "%s: bad arguments", who);
    const bool two = gx_stash1 != nullptr;
    S2VT_REQUIRE(two || !hblk1.p, "%s: an h row image for a second layer that is not there", who);
    S2VT_REQUIRE(x3_image_ok(hblk0, B, H) && x3_image_ok(hblk1, B, H),
                 "%s: the h row image needs B %% 64 == 0 and 16-byte aligned rows of ldhblk >= 3 * pad64(H) elements, ldhblk %% 8 == 0", who);
    S2VT_REQUIRE(H <= 1024 && lstm_seq_fwd_x3_persist_supported(B, H), "%s: shape not supported", who);
    S2VT_REQUIRE(workspace_bytes >= s2vt_lstm_seq_x3_workspace_bytes(T, B, H), "%s: workspace too small", who);
    S2VT_REQUIRE(!two || (w_hh1 && h_all1 && c_all1 && (n_gx == T || bias1)), "%s: second layer incomplete", who);
    const int64_t Kp = (H + 63) / 64 * 64;
    const size_t wbytes = align_up(3 * 4 * (size_t)H * Kp * 2, 256), hbytes = align_up(3 * (size_t)T * B * Kp * 2, 256);
    char* base = reinterpret_cast<char*>(workspace);
    int* err = reinterpret_cast<int*>(base);
    unsigned int* sa = reinterpret_cast<unsigned int*>(base + 256);
    unsigned int* sb = reinterpret_cast<unsigned int*>(base + 256 + lstm_persist_sync_bytes());
    char* q = base + 256 + 2 * lstm_persist_sync_bytes();
    unsigned short* wp[2] = {reinterpret_cast<unsigned short*>(q), reinterpret_cast<unsigned short*>(q + wbytes)};
    unsigned short* hp[2] = {reinterpret_cast<unsigned short*>(q + 2 * wbytes), reinterpret_cast<unsigned short*>(q + 2 * wbytes + hbytes)};
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = fill_zero(st, err, 256))) return rc;
    if ((rc = split3_rows(st, w_hh0, H, 4 * H, H, (int)Kp, wp[0], 4 * (int64_t)H * Kp))) return rc;
    if (two && (rc = split3_rows(st, w_hh1, H, 4 * H, H, (int)Kp, wp[1], 4 * (int64_t)H * Kp))) return rc;
    const int blk = block > 0 ? block : T;
    for (int t0 = 0; t0 < T; t0 += blk) {
        const int t1 = (t0 + blk < T) ? t0 + blk : T;
        ProfScope ps(st, K_STEP_FWD, (two ? 2 : 1) * (t1 - t0));
        SeqFwdX3Args a0 = persist_fwd_x3_args(t0, t1, B, H, T, Kp, gx_stash0, n_gx, bias0, wp[0], hp[0], h_all0, c_all0, sa, err);
        a0.hblk = hblk0.p; a0.ldhblk = hblk0.ld; a0.no_stash = no_stash;
        SeqFwdX3Args a1;
        if (two) {
            a1 = persist_fwd_x3_args(t0, t1, B, H, T, Kp, gx_stash1, n_gx, bias1, wp[1], hp[1], h_all1, c_all1, sb, err);
            a1.hblk = hblk1.p; a1.ldhblk = hblk1.ld; a1.no_stash = no_stash;
        }
        if ((rc = lstm_seq_fwd_x3_persist2(st, a0, two ? &a1 : nullptr))) return rc;
    }
    return 0;
}
int s2vt_lstm_seq_fwd_x3_persist(int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                                 const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1, float* h_all0,
                                 float* h_all1, float* c_all0, float* c_all1, int32_t block, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return seq_fwd_x3_entry("s2vt_lstm_seq_fwd_x3_persist", T, B, H, gx_stash0, gx_stash1, n_gx, bias0, bias1, w_hh0, w_hh1, h_all0, h_all1,
                            c_all0, c_all1, X3Image{nullptr, 0}, X3Image{nullptr, 0}, 0, block, workspace, workspace_bytes, stream);
}
int s2vt_lstm_seq_fwd_x3_persist_emit(int32_t T, int32_t B, int32_t H, float* gx_stash0, float* gx_stash1, int32_t n_gx,
                                      const float* bias0, const float* bias1, const float* w_hh0, const float* w_hh1, float* h_all0,
                                      float* h_all1, float* c_all0, float* c_all1, uint16_t* hblk0, int64_t ldhblk0, uint16_t* hblk1,
                                      int64_t ldhblk1, int32_t no_stash, int32_t block, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return seq_fwd_x3_entry("s2vt_lstm_seq_fwd_x3_persist_emit", T, B, H, gx_stash0, gx_stash1, n_gx, bias0, bias1, w_hh0, w_hh1, h_all0,
                            h_all1, c_all0, c_all1, X3Image{hblk0, ldhblk0}, X3Image{hblk1, ldhblk1}, no_stash, block, workspace,
                            workspace_bytes, stream);
}
// split-precision persistent BPTT as its own entry point.
// workspace: [err int x64][sync A][sync B] then per layer [W_hh^T fp32][W_hh^T planes][dc][partial-sum ring]
static size_t bwd_x3_ws_layer_bytes(int T, int B, int H, int nslots) {
    const size_t Kp = (size_t)(H + 63) / 64 * 64, Hp = (size_t)(H + 15) / 16 * 16;
    return align_up((size_t)H * 4 * H * 4, 256) + align_up(3 * Kp * 4 * Hp * 2, 256) + align_up((size_t)B * H * 4, 256) +
           align_up((size_t)nslots * lstm_seq_bwd_x3_part_slot_floats(B, H) * 4, 256);
}
size_t s2vt_lstm_seq_bwd_x3_workspace_bytes(int32_t T, int32_t B, int32_t H, int32_t block) {
    if (T <= 0 || B <= 0 || H <= 0 || H > 1024 || B % 32) return 0;
    const int blk = (block > 0 && block < T) ? block : T;
    return 256 + 2 * lstm_persist_sync_bytes() + 2 * bwd_x3_ws_layer_bytes(T, B, H, blk + 1);
}
// ... and for the BPTT (s2vt_lstm_seq_bwd_x3_persist_emit): SeqBwdX3Args::dgp / lddgp, colpart and skip_dg, refused as prep_y does.
static int seq_bwd_x3_entry(const char* who, int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                            const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1, float* stash_dg0,
                            float* stash_dg1, X3Image dgp0, X3Image dgp1, float* colpart0, float* colpart1, int32_t skip_dg, int32_t block,
                            void* workspace, size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && w_hh0 && c_all0 && stash_dg0 && workspace && dh_first >= 0 && (skip_dg == 0 || skip_dg == 1),
                 "%s: bad arguments", who);
    const bool two = stash_dg1 != nullptr;
    S2VT_REQUIRE(two || (!dgp1.p && !colpart1), "%s: a dG row image or column sums for a second layer that is not there", who);
    S2VT_REQUIRE((!dgp0.p && !dgp1.p) || H % 8 == 0, "%s: the dG row image needs H %% 8 == 0", who);
    S2VT_REQUIRE(x3_image_ok(dgp0, B, 4 * (int64_t)H) && x3_image_ok(dgp1, B, 4 * (int64_t)H),
                 "%s: the dG row image needs B %% 64 == 0 and 16-byte aligned rows of lddgp >= 3 * pad64(4H) elements, lddgp %% 8 == 0", who);
    S2VT_REQUIRE(!skip_dg || (dgp0.p && (!two || dgp1.p)), "%s: skip_dg without a dG row image", who);
    S2VT_REQUIRE(H <= 1024 && lstm_seq_bwd_x3_persist_supported(B, H), "%s: shape not supported", who);
    S2VT_REQUIRE(workspace_bytes >= s2vt_lstm_seq_bwd_x3_workspace_bytes(T, B, H, block), "%s: workspace too small", who);
    S2VT_REQUIRE(!two || (w_hh1 && c_all1), "%s: second layer incomplete", who);
    const int blk = (block > 0 && block < T) ? block : T;
    const int64_t Kp = (H + 63) / 64 * 64, Hp = (H + 15) / 16 * 16;
    const int64_t pslot = (int64_t)lstm_seq_bwd_x3_part_slot_floats(B, H);
    char* base = reinterpret_cast<char*>(workspace);
    int* err = reinterpret_cast<int*>(base);
    unsigned int* sy[2] = {reinterpret_cast<unsigned int*>(base + 256), reinterpret_cast<unsigned int*>(base + 256 + lstm_persist_sync_bytes())};
    char* q = base + 256 + 2 * lstm_persist_sync_bytes();
    float* wt[2]; unsigned short* wtp[2]; float* dc[2]; float* part[2];
    for (int l = 0; l < 2; ++l) {
        wt[l] = reinterpret_cast<float*>(q); q += align_up((size_t)H * 4 * H * 4, 256);
        wtp[l] = reinterpret_cast<unsigned short*>(q); q += align_up(3 * (size_t)Kp * 4 * Hp * 2, 256);
        dc[l] = reinterpret_cast<float*>(q); q += align_up((size_t)B * H * 4, 256);
        part[l] = reinterpret_cast<float*>(q); q += align_up((size_t)(blk + 1) * pslot * 4, 256);
    }
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = fill_zero(st, err, 256))) return rc;
    const float* whh[2] = {w_hh0, w_hh1};
    for (int l = 0; l < (two ? 2 : 1); ++l) {
        if ((rc = transpose_f32(st, whh[l], 4 * H, H, wt[l]))) return rc;
        if ((rc = split3_wt(st, wt[l], H, (int)Kp, (int)Hp, wtp[l], Kp * 4 * Hp))) return rc;
    }
    for (int t1 = T; t1 > 0; t1 -= blk) {
        const int t0 = (t1 - blk > 0) ? t1 - blk : 0;
        ProfScope ps(st, K_STEP_BWD, (two ? 2 : 1) * (t1 - t0));
        SeqBwdX3Args a0 = persist_bwd_x3_args(T, t0, t1, B, H, Kp, Hp, wtp[0], dh_out0, dh_first, c_all0, stash_dg0, dc[0],
                                              part[0], pslot, blk + 1, sy[0], err);
        a0.dgp = dgp0.p; a0.lddgp = dgp0.ld; a0.colpart = colpart0; a0.skip_dg = skip_dg;
        SeqBwdX3Args a1;
        if (two) {
            a1 = persist_bwd_x3_args(T, t0, t1, B, H, Kp, Hp, wtp[1], dh_out1, dh_first, c_all1, stash_dg1, dc[1],
                                     part[1], pslot, blk + 1, sy[1], err);
            a1.dgp = dgp1.p; a1.lddgp = dgp1.ld; a1.colpart = colpart1; a1.skip_dg = skip_dg;
        }
        if ((rc = lstm_seq_bwd_x3_persist2(st, a0, two ? &a1 : nullptr))) return rc;
    }
    return 0;
}
int s2vt_lstm_seq_bwd_x3_persist(int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                                 const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1, float* stash_dg0,
                                 float* stash_dg1, int32_t block, void* workspace, size_t workspace_bytes, void* stream) {
    return seq_bwd_x3_entry("s2vt_lstm_seq_bwd_x3_persist", T, B, H, w_hh0, w_hh1, dh_out0, dh_out1, dh_first, c_all0, c_all1, stash_dg0,
                            stash_dg1, X3Image{nullptr, 0}, X3Image{nullptr, 0}, nullptr, nullptr, 0, block, workspace, workspace_bytes, stream);
}
int s2vt_lstm_seq_bwd_x3_persist_emit(int32_t T, int32_t B, int32_t H, const float* w_hh0, const float* w_hh1, const float* dh_out0,
                                      const float* dh_out1, int32_t dh_first, const float* c_all0, const float* c_all1, float* stash_dg0,
                                      float* stash_dg1, uint16_t* dgp0, int64_t lddgp0, uint16_t* dgp1, int64_t lddgp1, float* colpart0,
                                      float* colpart1, int32_t skip_dg, int32_t block, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return seq_bwd_x3_entry("s2vt_lstm_seq_bwd_x3_persist_emit", T, B, H, w_hh0, w_hh1, dh_out0, dh_out1, dh_first, c_all0, c_all1,
                            stash_dg0, stash_dg1, X3Image{dgp0, lddgp0}, X3Image{dgp1, lddgp1}, colpart0, colpart1, skip_dg, block,
                            workspace, workspace_bytes, stream);
}

}
