// The batched beam-search depth step (S2VTModel.py:186-228 for all (sample, beam slot) rows of a depth at once).
#include "api_internal.h"

using namespace s2vt;

namespace s2vt {
// One word_rnn step over R fixed rows whose tokens are known (S2VTModel.py:211-212; the beam searches' depth step and the scoring
// driver's word steps, api_score.hip): h_prev · W_hh^T + the rows' gate input + the embedded token's segment - the per-token gate
// table of the decode cache (kc) on the plane path, the embedding rows against W_e inside the kernel's second K segment otherwise.
int rows_word_step(hipStream_t st, const s2vt_dims& d, const s2vt_params* p, const DecodeConst* kc, const RowsStep& r) {
    const int H = d.H, E = d.E;
    StepFwdArgs a = {};
    a.B = r.R; a.H = H;
    a.h_prev = r.h_prev; a.ldh = H; a.w_hh = p->word_w_hh; a.ldw = H;
    a.tok.tok_idx = r.tok; a.tok.tok_packed = r.tok_packed; a.tok.tok_const = r.tok_const;
    a.tok.tok_limit = d.V; a.tok.tok_err = r.err;
    a.gx = r.gx; a.ldgx = 4 * (int64_t)H; a.gx_idx = r.gx_idx;
    a.c_prev = r.c_prev; a.ldc = H;
    a.h_out = r.h_out; a.ldho = H; a.c_out = r.c_out; a.ldco = H;
    a.h_planes = r.h_planes; a.ldhp = r.ldhp;
    if (kc) { a.gx_tab = kc->gtab; a.ldtab = 4 * (int64_t)H; }
    else { a.x2 = p->emb_w; a.ldx2 = E; a.K2 = E; a.w2 = p->word_w_ih; a.ldw2 = E + H; }
    return lstm_step_fwd(st, a);
}
}  // namespace s2vt

extern "C" {

// ---------------------------------------------------------------------------------- batched beam-search depth
struct BeamWS {
    float *bsum1, *bsum2, *ph, *pc, *gx, *logits, *gws;
    int* err;                // [0]: a token id outside [0, V) reached the word step (reported as S2VT_ERR_INDEX)
    PB pvid, pword;          // plane path (s2vt_beam_step_cached): planes of vid_rnn's h [B rows] and of the word step's h_t [R rows]
    size_t gws_floats, bytes;
};
static BeamWS carve_beam(const s2vt_dims& d, int max_rows, void* base) {
    const size_t H = d.H, V = d.V, R = (size_t)max_rows;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    BeamWS w;
    w.bsum1 = c.take<float>(4 * H);
    w.bsum2 = c.take<float>(4 * H);
    w.ph = c.take<float>(R * H);
    w.pc = c.take<float>(R * H);
    w.gx = c.take<float>(R * 4 * H);
    w.logits = c.take<float>(R * V);
    w.gws_floats = 4 * R * (V > 4 * H ? V : 4 * H);
    w.gws = c.take<float>(w.gws_floats);
    w.err = c.take<int>(4);
    w.pvid = take_planes(c, d.B, H, DECODE_PLANES); w.pword = take_planes(c, R, H, DECODE_PLANES);
    w.bytes = align_up(c.off, 256);
    return w;
}

size_t s2vt_beam_workspace_bytes(const s2vt_dims* d, int32_t max_rows) {
    if (!d || max_rows <= 0) return 0;
    return carve_beam(*d, max_rows, nullptr).bytes;
}

// con (nullable): the constrained search's depth step - the fan-out head is the constrained one (ce.hip: the rules of the constrained
// draw on each row with beam slot r's own words hist[r * hist_ld + i], i < t, then log_softmax and the top 20 of the edited row)
struct BeamCon { const char* fn; const s2vt_constraints* c; const int32_t* hist; int64_t hist_ld; int t; };
// gum (nullable): the stochastic beam's depth step - the fan-out head is the perturbed one (gumbel_top.hip: every row's 20 best words by
// log-prob + Gumbel noise of (seed, step, row r, v), best first, with the extra output top_g [R, 20])
struct BeamGum { GumbelArgs ga; float* top_g; };
static int beam_fan_out(hipStream_t st, float* logits, int R, int V, const BeamCon* con, int32_t* top_ix, float* top_lp,
                        const BeamGum* gum) {
    if (gum) return top20_gumbel(st, logits, V, R, V, gum->ga, top_ix, top_lp, gum->top_g);
    if (!con) return top20_logprob(st, logits, V, R, V, top_ix, top_lp);
    return top20_constrained_checked(con->fn, st, logits, V, R, V, con->hist, con->hist_ld, con->t, con->c, top_ix, top_lp);
}
static int beam_step_impl(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out, int32_t* top_ix,
                          float* top_lp, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, void* stream,
                          const float* gx_vid, const BeamCon* con = nullptr, float* logits_out = nullptr, int64_t ld_out = 0,
                          const BeamGum* gum = nullptr) {
    S2VT_REQUIRE(d && p && workspace && (gx_vid || (vid_h_in && vid_c_in && vid_h_out && vid_c_out)), "s2vt_beam_step: null argument");
    S2VT_REQUIRE(R >= 0 && (R == 0 || (row_b && row_state && tok && word_h_in && word_c_in && word_h_out && word_c_out &&
                                        (logits_out || (top_ix && top_lp)))),
                 "s2vt_beam_step: null row argument");
    const int B = d->B, H = d->H, E = d->E, V = d->V;
    S2VT_REQUIRE(workspace_bytes >= carve_beam(*d, R > 0 ? R : 1, nullptr).bytes, "s2vt_beam_step: workspace too small");
    const BeamWS w = carve_beam(*d, R > 0 ? R : 1, workspace);
    hipStream_t st = (hipStream_t)stream;
    // logits_out (s2vt_beam_step_logits): out_linear writes the caller's rows and the step ends there - no fan-out
    float* const lg = logits_out ? logits_out : w.logits;
    const int64_t ldl = logits_out ? ld_out : V;
    int rc;
    if (!gx_vid && (rc = bias_sums(st, p, H, w.bsum1, w.bsum2))) return rc;
    if (!gx_vid) {   // one zero-input vid_rnn step for the whole batch (S2VTModel.py:208-210)
        StepFwdArgs a = {};
        a.B = B; a.H = H;
        a.h_prev = vid_h_in; a.ldh = H; a.w_hh = p->vid_w_hh; a.ldw = H;
        a.bias = w.bsum1;
        a.c_prev = vid_c_in; a.ldc = H;
        a.h_out = vid_h_out; a.ldho = H; a.c_out = vid_c_out; a.ldco = H;
        if ((rc = lstm_step_fwd(st, a))) return rc;
    }
    if (R == 0) return 0;
    const Lane ln{st, w.gws, w.gws_floats, nullptr};
    // parents' word_rnn states, the vid_out half of the gate input (A rows gathered by sample), then the word step
    // with the embedding rows gathered inside the kernel's second K segment (:211-212)
    if ((rc = gather_rows_f32(st, word_h_in, H, row_state, R, H, w.ph))) return rc;
    if ((rc = gather_rows_f32(st, word_c_in, H, row_state, R, H, w.pc))) return rc;
    // the word step of the R rows (rows_word_step above): parents' states, the token checked against V; each path below names its
    // gate input - per sample + the gate table on the plane path, per row + the embedding K segment otherwise
    RowsStep a = {};
    a.R = R; a.tok = tok; a.err = w.err;
    a.gx = w.gx;
    a.h_prev = w.ph; a.c_prev = w.pc; a.h_out = word_h_out; a.c_out = word_c_out;
    if (cache && decode_plan(*d, true, false).planes && H <= 1024) {     // (any batch: the row counts of its GEMMs are free, the images are the cache's)
        // PLANE PATH (the weight-derived images of a greedy decode of the same weights, s2vt_greedy_decode_cached: W_v and W_o
        // as blocked 3-plane operands, the per-token gate table): the vid_out half of the gate input once per SAMPLE (every beam
        // slot reads its sample's row), the embedded word from the table, out_linear on the bf16 matrix cores in split
        // precision (fp32-equivalent) from the h_t planes the step kernel writes itself
        S2VT_REQUIRE(cache_bytes >= carve_decode_const(*d, nullptr).bytes, "s2vt_beam_step_cached: cache too small");
        const DecodeConst kc = carve_decode_const(*d, cache);
        if (!gx_vid) {
            if ((rc = psplit(ln, w.pvid, 0, vid_h_out, H, ID, B, H))) return rc;
            if ((rc = pgemm(ln, B, 4 * H, H, w.pvid, 0, 0, kc.wv, 0, 0, w.gx, 4 * H, ID, w.bsum2, false))) return rc;
        }
        if ((rc = fill_zero(st, w.pword.p, rows64((size_t)R) * (size_t)w.pword.ld * sizeof(unsigned short)))) return rc;
        if (gx_vid) a.gx = gx_vid;
        a.gx_idx = row_b;
        a.h_planes = w.pword.p; a.ldhp = w.pword.ld;
        if ((rc = fill_zero(st, w.err, 4 * sizeof(int)))) return rc;
        if ((rc = rows_word_step(st, *d, p, &kc, a))) return rc;
        if ((rc = pgemm(ln, R, V, H, w.pword, 0, 0, kc.wo, 0, 0, lg, ldl, ID, p->out_b, false))) return rc;
        if (!logits_out && (rc = beam_fan_out(st, w.logits, R, V, con, top_ix, top_lp, gum))) return rc;
        return post_async_error(st, w.err, 3);       // (ring slot: no wait for the previous depth step)
    }
    S2VT_REQUIRE(!gx_vid, "s2vt_beam_step_gx: the precomputed vid_rnn half needs the plane path (gemm mode 1 / 3, H <= 1024)");
    if ((rc = lgemm(ln, true, true, R, 4 * H, H, vid_h_out, H, gather(row_b), p->word_w_ih + E, E + H, ID, w.gx, 4 * H, ID,
                    w.bsum2, false)))
        return rc;
    if ((rc = fill_zero(st, w.err, 4 * sizeof(int)))) return rc;
    if ((rc = rows_word_step(st, *d, p, nullptr, a))) return rc;
    if ((rc = lgemm(ln, true, true, R, V, H, word_h_out, H, ID, p->out_w, H, ID, lg, ldl, ID, p->out_b, false))) return rc;       // (:213)
    if (!logits_out && (rc = beam_fan_out(st, w.logits, R, V, con, top_ix, top_lp, gum))) return rc;                                   // (:214-219)
    return post_async_error(st, w.err, 3);       // (ring slot: no wait for the previous depth step)
}
// the depth step with vid_rnn's part precomputed (s2vt_decode_encode_cached, gx_dec[depth - 1]): word step, out_linear, fan-out
int s2vt_beam_step_gx(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                      const int32_t* tok, const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out,
                      float* word_c_out, int32_t* top_ix, float* top_lp, void* workspace, size_t workspace_bytes, void* cache,
                      size_t cache_bytes, void* stream) {
    S2VT_REQUIRE(cache && gx_vid, "s2vt_beam_step_gx: null cache / gx_vid");
    return beam_step_impl(d, p, R, row_b, row_state, tok, nullptr, nullptr, nullptr, nullptr, word_h_in, word_c_in, word_h_out,
                          word_c_out, top_ix, top_lp, workspace, workspace_bytes, cache, cache_bytes, stream, gx_vid);
}
// the depth step of the constrained search, all three forms: gx_vid != null - s2vt_beam_step_gx's (needs the cache); else cache !=
// null - s2vt_beam_step_cached's; else s2vt_beam_step's
int s2vt_beam_step_constrained(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                               const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                               const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out,
                               int32_t* top_ix, float* top_lp, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                               const s2vt_constraints* c, const int32_t* hist, int64_t hist_ld, int32_t t, void* stream) {
    S2VT_REQUIRE(c, "s2vt_beam_step_constrained: null constraints");
    S2VT_REQUIRE(!gx_vid || cache, "s2vt_beam_step_constrained: gx_vid needs the cache");
    S2VT_REQUIRE(t >= 0 && t <= 1023 && (t == 0 || (hist && hist_ld >= t)), "s2vt_beam_step_constrained: t %d outside [0, 1023], or no history",
                 (int)t);
    const BeamCon con{"s2vt_beam_step_constrained", c, hist, hist_ld, t};
    if (gx_vid) {                  // (beam_step_impl takes vid_rnn's step from gx_vid; s2vt_beam_step_gx passes no states either)
        vid_h_in = vid_c_in = nullptr;
        vid_h_out = vid_c_out = nullptr;
    }
    return beam_step_impl(d, p, R, row_b, row_state, tok, vid_h_in, vid_c_in, vid_h_out, vid_c_out, word_h_in, word_c_in, word_h_out,
                          word_c_out, top_ix, top_lp, workspace, workspace_bytes, cache, cache ? cache_bytes : 0, stream, gx_vid, &con);
}
// the depth step of an ensemble member, all three forms chosen as s2vt_beam_step_constrained chooses them: the same launches up to
// and including out_linear, which writes the rows' logits to logits_out (row stride ld_out >= V); no fan-out
int s2vt_beam_step_logits(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out,
                          float* logits_out, int64_t ld_out, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                          void* stream) {
    S2VT_REQUIRE(d && logits_out && ld_out >= d->V, "s2vt_beam_step_logits: null logits_out, or ld_out < V");
    S2VT_REQUIRE(!gx_vid || cache, "s2vt_beam_step_logits: gx_vid needs the cache");
    if (gx_vid) {
        vid_h_in = vid_c_in = nullptr;
        vid_h_out = vid_c_out = nullptr;
    }
    return beam_step_impl(d, p, R, row_b, row_state, tok, vid_h_in, vid_c_in, vid_h_out, vid_c_out, word_h_in, word_c_in, word_h_out,
                          word_c_out, nullptr, nullptr, workspace, workspace_bytes, cache, cache ? cache_bytes : 0, stream, gx_vid, nullptr,
                          logits_out, ld_out);
}
// the depth step of the stochastic beam (S2VT.sample_distinct), all three forms chosen as s2vt_beam_step_constrained chooses them: the
// same launches up to and including out_linear, then the perturbed fan-out head with the noise of (seed, step, row r, v)
int s2vt_beam_step_gumbel(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* gx_vid, const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out,
                          int32_t* top_ix, float* top_lp, float* top_g, void* workspace, size_t workspace_bytes, void* cache,
                          size_t cache_bytes, float inv_temperature, uint64_t seed, int32_t step, void* stream) {
    S2VT_REQUIRE(top_g || R == 0, "s2vt_beam_step_gumbel: null top_g");
    S2VT_REQUIRE(!gx_vid || cache, "s2vt_beam_step_gumbel: gx_vid needs the cache");
    S2VT_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.4028234e38f && step >= 0,
                 "s2vt_beam_step_gumbel: inv_temperature must be finite and > 0 (got %g), step >= 0", (double)inv_temperature);
    const BeamGum gum{GumbelArgs{inv_temperature, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), (uint32_t)step, 0u,
                                 (uint32_t)(R > 0 ? R : 0)}, top_g};
    if (gx_vid) {
        vid_h_in = vid_c_in = nullptr;
        vid_h_out = vid_c_out = nullptr;
    }
    return beam_step_impl(d, p, R, row_b, row_state, tok, vid_h_in, vid_c_in, vid_h_out, vid_c_out, word_h_in, word_c_in, word_h_out,
                          word_c_out, top_ix, top_lp, workspace, workspace_bytes, cache, cache ? cache_bytes : 0, stream, gx_vid, nullptr,
                          nullptr, 0, &gum);
}
int s2vt_beam_step(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                   const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                   const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out, int32_t* top_ix,
                   float* top_lp, void* workspace, size_t workspace_bytes, void* stream) {
    return beam_step_impl(d, p, R, row_b, row_state, tok, vid_h_in, vid_c_in, vid_h_out, vid_c_out, word_h_in, word_c_in, word_h_out,
                          word_c_out, top_ix, top_lp, workspace, workspace_bytes, nullptr, 0, stream, nullptr);
}
int s2vt_beam_step_cached(const s2vt_dims* d, const s2vt_params* p, int32_t R, const int32_t* row_b, const int32_t* row_state,
                          const int32_t* tok, const float* vid_h_in, const float* vid_c_in, float* vid_h_out, float* vid_c_out,
                          const float* word_h_in, const float* word_c_in, float* word_h_out, float* word_c_out, int32_t* top_ix,
                          float* top_lp, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, void* stream) {
    S2VT_REQUIRE(cache, "s2vt_beam_step_cached: null cache");
    return beam_step_impl(d, p, R, row_b, row_state, tok, vid_h_in, vid_c_in, vid_h_out, vid_c_out, word_h_in, word_c_in, word_h_out,
                          word_c_out, top_ix, top_lp, workspace, workspace_bytes, cache, cache_bytes, stream, nullptr);
}
}
