// Per-op entry points of the GRU cell (S2VTModel.py:11-22 with rnn_type='gru': nn.GRU in place of nn.LSTM): the timestep
// kernels of gru.hip, whole layers looping them, and the target-id conversion of the train path.  The model-level composition
// (projections, autograd, greedy loop) is gru_functional.py's; there is no GRU whole-path driver.
#include "api_internal.h"

using namespace s2vt;

static bool gru_rows_ok(int32_t T, int32_t B, int32_t H) {
    return T > 0 && B > 0 && H > 0 && (int64_t)T * B * 4 * H < ((int64_t)1 << 40);
}

extern "C" {

int s2vt_gru_step_fwd(int32_t B, int32_t H, const float* gx, const float* b_ih, const float* w_hh, const float* b_hh,
                      const float* h_prev, float* h_out, float* stash, void* stream) {
    S2VT_REQUIRE(gru_rows_ok(1, B, H) && (gx || b_ih) && w_hh && b_hh && h_out, "s2vt_gru_step_fwd: null/invalid argument");
    GruFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    a.h_prev = h_prev; a.ldh = H; a.w_hh = w_hh; a.ldw = H; a.b_hh = b_hh;
    a.gx = gx; a.ldgx = 3 * (int64_t)H; a.b_ih = b_ih;
    a.h_out = h_out; a.ldho = H;
    a.stash = stash; a.ldst = 4 * (int64_t)H;
    ProfScope ps((hipStream_t)stream, K_STEP_FWD, 1);
    return gru_step_fwd((hipStream_t)stream, a);
}

}  // (C linkage ends)
static int gru_step_fwd_token_impl(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* b_hh,
                                   const float* h_prev, const float* emb, const float* w_e, int64_t ldw_e, const int32_t* tok,
                                   const unsigned long long* tok_packed, int32_t tok_const, const SsArgs* ss, float* h_out, void* stream);
extern "C" {
int s2vt_gru_step_fwd_token(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* b_hh,
                            const float* h_prev, const float* emb, const float* w_e, int64_t ldw_e, const int32_t* tok,
                            const unsigned long long* tok_packed, int32_t tok_const, float* h_out, void* stream) {
    return gru_step_fwd_token_impl(B, H, E, V, gx, w_hh, b_hh, h_prev, emb, w_e, ldw_e, tok, tok_packed, tok_const, nullptr, h_out, stream);
}
// the same step of a scheduled-sampling pass: the coin of (row0 + b, step) picks tok_packed's word or targets[b][step]; a bad
// ground-truth id is posted like a bad `tok`
int s2vt_gru_step_fwd_token_ss(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* b_hh,
                               const float* h_prev, const float* emb, const float* w_e, int64_t ldw_e,
                               const unsigned long long* tok_packed, const int64_t* targets, int64_t targets_ld, float ss_prob,
                               uint64_t seed, int32_t step, int32_t row0, float* h_out, void* stream) {
    S2VT_REQUIRE(targets && step >= 0 && row0 >= 0 && targets_ld > step && (tok_packed || step == 0),
                 "s2vt_gru_step_fwd_token_ss: null/invalid argument");
    S2VT_REQUIRE(ss_prob >= 0.f && ss_prob <= 1.f, "s2vt_gru_step_fwd_token_ss: ss_prob must be in [0, 1] (got %g)", (double)ss_prob);
    const SsArgs ss{targets, targets_ld, ss_prob, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), (uint32_t)step,
                    (uint32_t)row0, (uint32_t)row0 + (uint32_t)B};
    return gru_step_fwd_token_impl(B, H, E, V, gx, w_hh, b_hh, h_prev, emb, w_e, ldw_e, nullptr, tok_packed, 0, &ss, h_out, stream);
}
}  // extern "C"
static int gru_step_fwd_token_impl(int32_t B, int32_t H, int32_t E, int32_t V, const float* gx, const float* w_hh, const float* b_hh,
                                   const float* h_prev, const float* emb, const float* w_e, int64_t ldw_e, const int32_t* tok,
                                   const unsigned long long* tok_packed, int32_t tok_const, const SsArgs* ss, float* h_out, void* stream) {
    S2VT_REQUIRE(gru_rows_ok(1, B, H) && E > 0 && V > 0 && gx && w_hh && b_hh && emb && w_e && h_out && ldw_e >= E,
                 "s2vt_gru_step_fwd_token: null/invalid argument");
    hipStream_t st = (hipStream_t)stream;
    // Where the token comes from decides how a bad id is reported.  tok_const is known here: it is checked on the host and
    // refused at once.  tok_packed is the word s2vt_decode_step_argmax left, whose index is in [0, V) by construction: nothing
    // to report (the kernel still reads an impossible id as token 0).  Only a caller's int32 array (tok) needs the device flag,
    // posted on the ring record of the asynchronous-error table, so that one call per step never waits for an earlier step.
    // The greedy loop (first step tok_const, then tok_packed) therefore makes no device-to-host copy and never synchronises.
    if (!tok && !tok_packed && !ss && (tok_const < 0 || tok_const >= V)) {
        set_error("s2vt_gru_step_fwd_token: token id %d outside [0, %d)", (int)tok_const, (int)V);
        return S2VT_ERR_INDEX;
    }
    PostedFlags flags;
    int rc;
    const bool posts = tok || ss;      // (ids of the caller: a caller's int32 array, or the ground-truth words of a scheduled pass)
    if (posts && (rc = flags.open(st))) return rc;
    GruFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    a.h_prev = h_prev; a.ldh = H; a.w_hh = w_hh; a.ldw = H; a.b_hh = b_hh;
    a.gx = gx; a.ldgx = 3 * (int64_t)H;
    a.x2 = emb; a.ldx2 = E; a.K2 = E; a.w2 = w_e; a.ldw2 = ldw_e;
    a.tok = TokenSrc{tok, tok_packed, tok_const, V, flags.p, ss ? *ss : SsArgs{}};
    a.h_out = h_out; a.ldho = H;
    {
        ProfScope ps(st, K_STEP_FWD, 1);
        if ((rc = gru_step_fwd(st, a))) return rc;
    }
    return flags.close(st, 3);
}
extern "C" {

int s2vt_gru_step_bwd(int32_t B, int32_t H, const float* dgh_next, const float* w_hh_t, const float* stash_next, const float* dh_out,
                      const float* stash, const float* h_prev, float* dh, float* dgx, float* dgh, void* stream) {
    S2VT_REQUIRE(gru_rows_ok(1, B, H) && stash && dh && dgx && dgh, "s2vt_gru_step_bwd: null/invalid argument");
    S2VT_REQUIRE((dgh_next == nullptr) == (stash_next == nullptr) && (!dgh_next || w_hh_t),
                 "s2vt_gru_step_bwd: dgh_next, stash_next and w_hh_t go together (all NULL at the last step only)");
    GruBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = H;
    a.dgh_next = dgh_next; a.lddgh = 3 * (int64_t)H; a.w_hh_t = w_hh_t; a.ldwt = 3 * (int64_t)H;
    a.stash_next = stash_next; a.ldstn = 4 * (int64_t)H;
    a.dh_out = dh_out; a.lddho = H;
    a.stash = stash; a.ldst = 4 * (int64_t)H;
    a.h_prev = h_prev; a.ldhp = H;
    a.dh = dh; a.lddh = H;
    a.dgx = dgx; a.lddgx = 3 * (int64_t)H;
    a.dgh = dgh; a.lddgh_out = 3 * (int64_t)H;
    ProfScope ps((hipStream_t)stream, K_STEP_BWD, 1);
    return gru_step_bwd((hipStream_t)stream, a);
}

int s2vt_gru_seq_fwd(int32_t T, int32_t B, int32_t H, const float* gx, int32_t n_gx, const float* b_ih, const float* w_hh,
                     const float* b_hh, float* h_all, float* stash, void* stream) {
    S2VT_REQUIRE(gru_rows_ok(T, B, H) && w_hh && b_hh && h_all && n_gx >= 0 && n_gx <= T, "s2vt_gru_seq_fwd: null/invalid argument");
    S2VT_REQUIRE(n_gx == 0 || gx, "s2vt_gru_seq_fwd: gx missing");
    S2VT_REQUIRE(n_gx == T || b_ih, "s2vt_gru_seq_fwd: b_ih needed for steps without gx");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, K_STEP_FWD, T);
    const int64_t BH = (int64_t)B * H, B3H = 3 * BH, B4H = 4 * BH;
    for (int t = 0; t < T; ++t) {
        GruFwdArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.H = H;
        a.h_prev = t ? h_all + (t - 1) * BH : nullptr; a.ldh = H;
        a.w_hh = w_hh; a.ldw = H; a.b_hh = b_hh;
        a.gx = (t < n_gx) ? gx + t * B3H : nullptr; a.ldgx = 3 * (int64_t)H; a.b_ih = b_ih;
        a.h_out = h_all + t * BH; a.ldho = H;
        a.stash = stash ? stash + t * B4H : nullptr; a.ldst = 4 * (int64_t)H;
        int rc = gru_step_fwd(st, a);
        if (rc) return rc;
    }
    return 0;
}

int s2vt_gru_seq_bwd(int32_t T, int32_t B, int32_t H, const float* w_hh, const float* dh_out, int32_t dh_first, const float* h_all,
                     const float* stash, float* w_hh_t, float* dh, float* dgx, float* dgh, void* stream) {
    S2VT_REQUIRE(gru_rows_ok(T, B, H) && w_hh && h_all && stash && w_hh_t && dh && dgx && dgh && dh_first >= 0,
                 "s2vt_gru_seq_bwd: null/invalid argument");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = transpose_f32(st, w_hh, 3 * H, H, w_hh_t))) return rc;
    ProfScope ps(st, K_STEP_BWD, T);
    const int64_t BH = (int64_t)B * H, B3H = 3 * BH, B4H = 4 * BH;
    for (int t = T - 1; t >= 0; --t) {
        GruBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.H = H;
        const bool next = t < T - 1;
        a.dgh_next = next ? dgh + (t + 1) * B3H : nullptr; a.lddgh = 3 * (int64_t)H;
        a.w_hh_t = w_hh_t; a.ldwt = 3 * (int64_t)H;
        a.stash_next = next ? stash + (t + 1) * B4H : nullptr; a.ldstn = 4 * (int64_t)H;
        a.dh_out = (dh_out && t >= dh_first) ? dh_out + (int64_t)(t - dh_first) * BH : nullptr; a.lddho = H;
        a.stash = stash + t * B4H; a.ldst = 4 * (int64_t)H;
        a.h_prev = t ? h_all + (t - 1) * BH : nullptr; a.ldhp = H;
        a.dh = dh; a.lddh = H;
        a.dgx = dgx + t * B3H; a.lddgx = 3 * (int64_t)H;
        a.dgh = dgh + t * B3H; a.lddgh_out = 3 * (int64_t)H;
        if ((rc = gru_step_bwd(st, a))) return rc;
    }
    return 0;
}

int s2vt_tokens_time_major(int32_t B, int32_t Lm1, int32_t V, const int64_t* targets, int64_t targets_ld, int32_t* tok, void* stream) {
    S2VT_REQUIRE(B > 0 && Lm1 > 0 && V > 0 && targets && tok && targets_ld >= Lm1, "s2vt_tokens_time_major: null/invalid argument");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    if ((rc = targets_to_time_major(st, targets, B, Lm1, targets_ld, V, tok, flags.p))) return rc;
    return flags.close(st, 0);
}

}  // extern "C"
