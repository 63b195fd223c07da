// K sampled captions per clip on one encode (S2VT.sample; not in the reference): the draws of mode='sample' for the R = B * K rows
// r = b * K + k, for sequence-level training with K samples per clip.  One encode per clip (the scoring driver's two encode phases),
// word_rnn's start state gathered to the rows, then L-1 word steps over the fixed rows (the beam searches' step, rows_word_step):
// row r reads its clip's gate input through gx_idx and the packed word it drew at the step before, and the sampling head - the
// decode drivers' arg-max launches with their Gumbel arguments - draws for all R rows with row0 = 0, rows = R.  One chain on the
// caller's stream: no schedule splits the rows, so batch row = r at every launch.  A final launch turns the packed words into ids.
// s2vt_sample_decode_rows_trunc: the same driver with top-k / nucleus truncation - per step the head is replaced by out_linear as
// the beam step runs it (the plane GEMM on the cache's W_o image, or the fp32-input GEMM) into a [Rp, V] buffer of the workspace and
// the truncated draw of truncate.hip over its rows; with nothing to truncate it runs the fused head, launch for launch.
// s2vt_decode_rows_constrained: the same driver again with a greedy flag and the constraints of the constrained draw (S2VT.
// decode_constrained) - the head is the logits GEMM and truncate.hip's constrained row kernel, which reads the rows' history from
// this driver's own packed words (w.packed, stride Rp, t = the step); with every constraint off, the fused heads.
#include "api_internal.h"

using namespace s2vt;

extern "C" {

struct SampleRowsWS {
    int32_t* row_b;                  // [Rp] clip of each row
    int* err;
    float *states, *gx_dec;          // vid_h, vid_c, word_h, word_c [B][H] after the L frames; [L-1][B][4H] vid_rnn's half of the gate input
    float *ph, *pc;                  // [2][R][H] h_t ping-pong, [R][H] c_t
    unsigned long long* packed;      // [L-1][Rp] the steps' packed draws
    float* gws; size_t gws_floats;
    PB himg;                         // plane path: the step's h_t as blocked planes [Rp rows]
    float* logits;                   // truncated draws only: [Rp][V] the step's logits
    size_t bytes;
};
static bool sample_rows_shape_ok(const s2vt_dims* d, int K) {
    return dims_ok(d) && K >= 1 && (int64_t)(d->L - 1) * (int64_t)rows64((size_t)d->B * K) < (1ll << 31);
}
static SampleRowsWS carve_sample_rows(const s2vt_dims& d, int K, void* base, bool trunc = false) {
    const size_t B = d.B, H = d.H, R = B * K, Rp = rows64(R), S = d.L - 1;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    SampleRowsWS w;
    w.row_b = c.take<int32_t>(Rp);
    w.err = c.take<int>(4);
    w.states = c.take<float>(4 * B * H); w.gx_dec = c.take<float>(S * B * 4 * H);
    w.ph = c.take<float>(2 * R * H); w.pc = c.take<float>(R * H);
    w.packed = c.take<unsigned long long>(S * Rp);
    w.gws_floats = (size_t)4 << 20;
    w.gws = c.take<float>(w.gws_floats);
    // (sized for either path: which one a call takes depends on its cache argument)
    if (gemm_mode() != 0) w.himg = take_planes(c, R, H, DECODE_PLANES);
    w.logits = trunc ? c.take<float>(Rp * (size_t)d.V) : nullptr;
    w.bytes = align_up(c.off, 256);
    return w;
}
size_t s2vt_sample_rows_workspace_bytes(const s2vt_dims* d, int32_t K) {
    return sample_rows_shape_ok(d, K) ? carve_sample_rows(*d, K, nullptr).bytes : 0;
}

// the vocabulary bound of the truncated draw's row kernel (truncate.hip: the row in registers or LDS)
static bool trunc_vocab_ok(const s2vt_dims* d) { return (size_t)d->V * sizeof(float) <= 150 * 1024; }
size_t s2vt_sample_rows_trunc_workspace_bytes(const s2vt_dims* d, int32_t K) {
    return sample_rows_shape_ok(d, K) && trunc_vocab_ok(d) ? carve_sample_rows(*d, K, nullptr, true).bytes : 0;
}
}  // extern "C"

// The constraints of the constrained draw (include/s2vt_hip.h "constrained draw"), checked on the host: 0 and `out` filled in for
// step t (the caller sets hist / hist_ld / t / eos per step: constrain_at), or S2VT_ERR_ARG with the refusing rule in the message.
static int check_constraints(const char* fn, const s2vt_constraints* c, int V, int32_t greedy, float temperature, int32_t top_k, float top_p,
                             ConstrainArgs* out) {
    S2VT_REQUIRE(c, "%s: null constraints", fn);
    S2VT_REQUIRE(c->repetition_penalty >= 1.f && c->repetition_penalty <= 3.4028234e38f,
                 "%s: repetition_penalty must be finite and >= 1 (got %g)", fn, (double)c->repetition_penalty);
    S2VT_REQUIRE(c->no_repeat_ngram >= 0, "%s: no_repeat_ngram %d < 0", fn, (int)c->no_repeat_ngram);
    S2VT_REQUIRE(c->min_length >= 0, "%s: min_length %d < 0", fn, (int)c->min_length);
    S2VT_REQUIRE(c->n_banned >= 0 && c->n_banned <= 32 && (c->n_banned == 0 || c->banned), "%s: n_banned %d outside [0, 32] (or null banned)",
                 fn, (int)c->n_banned);
    for (int i = 0; i < c->n_banned; ++i)
        S2VT_REQUIRE(c->banned[i] >= 0 && c->banned[i] < V, "%s: banned id %d outside [0, V = %d)", fn, (int)c->banned[i], V);
    S2VT_REQUIRE(c->eos_ix >= 0 && c->eos_ix < V, "%s: eos_ix %d outside [0, V = %d)", fn, (int)c->eos_ix, V);
    S2VT_REQUIRE(greedy == 0 || greedy == 1, "%s: greedy must be 0 or 1 (got %d)", fn, (int)greedy);
    S2VT_REQUIRE(!greedy || (temperature == 1.f && top_k == 0 && top_p == 1.f),
                 "%s: greedy needs temperature 1, top_k 0 and top_p 1 (got %g, %d, %g)", fn, (double)temperature, (int)top_k, (double)top_p);
    memset(out, 0, sizeof(*out));
    out->ngram = c->no_repeat_ngram;
    out->theta = c->repetition_penalty;
    out->inv_theta = (float)(1.0 / (double)c->repetition_penalty);
    out->eos = -1;
    out->n_banned = c->n_banned;
    for (int i = 0; i < c->n_banned; ++i) out->banned[i] = c->banned[i];
    return 0;
}
static bool constraints_off(const s2vt_constraints* c) {
    return c->no_repeat_ngram == 0 && c->repetition_penalty == 1.f && c->min_length == 0 && c->n_banned == 0;
}
static ConstrainArgs constrain_at(ConstrainArgs a, const s2vt_constraints* c, const unsigned long long* hist, int64_t hist_ld, int t) {
    a.hist = t > 0 ? hist : nullptr; a.hist_ld = hist_ld; a.t = t;
    a.eos = t < c->min_length ? c->eos_ix : -1;
    return a;
}

// The constrained beam's fan-out head behind the host-side checks of the constrained draw (api_internal.h): the per-op entry and
// the constrained depth step (api_beam.hip) run it.  With every constraint off: top20_logprob, today's launch.
namespace s2vt {
int top20_constrained_checked(const char* fn, hipStream_t st, float* logits, int64_t ld, int64_t rows, int V, const int32_t* hist,
                              int64_t hist_ld, int t, const s2vt_constraints* c, int32_t* top_ix, float* top_lp) {
    S2VT_REQUIRE(logits && top_ix && top_lp && rows > 0 && rows < (1ll << 31) && V > 0 && ld >= V, "%s: null/invalid argument", fn);
    S2VT_REQUIRE(V >= 20 && (size_t)V * sizeof(float) <= 150 * 1024, "%s: vocab_size %d outside [20, 38400]", fn, (int)V);
    ConstrainArgs ca;
    int rc;
    if ((rc = check_constraints(fn, c, V, 0, 1.f, 0, 1.f, &ca))) return rc;
    S2VT_REQUIRE(t >= 0 && t <= 1023, "%s: t %d outside [0, 1023]", fn, (int)t);
    S2VT_REQUIRE(t == 0 || hist, "%s: null history at t = %d", fn, (int)t);
    S2VT_REQUIRE(t == 0 || hist_ld >= t, "%s: hist_ld %lld < t %d", fn, (long long)hist_ld, (int)t);
    if (constraints_off(c)) return top20_logprob(st, logits, ld, rows, V, top_ix, top_lp);
    S2VT_REQUIRE(V >= 20 + t + c->n_banned + 1, "%s: vocab_size %d < 20 + t + n_banned + 1 = %d: a row could keep fewer than 20 words", fn,
                 (int)V, 20 + t + (int)c->n_banned + 1);
    return top20_logprob_constrained(st, logits, ld, rows, V, constrain_at(ca, c, nullptr, 0, t), hist, hist_ld, top_ix, top_lp);
}
}  // namespace s2vt

// All three entry points (fn names the one that was called).  trunc: the workspace has the logits buffer and a step's head is the logits
// GEMM + the truncated draw - unless top_k / top_p truncate nothing, which runs the fused head like the plain entry point.
// con: s2vt_decode_rows_constrained - a greedy flag and the constraints on top of trunc; with every constraint off it runs the
// fused heads (greedy: the arg-max, no noise) or what trunc runs.
static int sample_rows_run(const char* fn, bool trunc, int32_t top_k, float top_p, const s2vt_constraints* con, int32_t greedy,
                           const s2vt_dims* d, const s2vt_params* p,
                           const float* feats, int32_t K, int32_t sos_ix, float temperature, uint64_t seed, int64_t* ids, void* workspace,
                           size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid, void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && ids && workspace, "%s: null/invalid argument", fn);
    S2VT_REQUIRE(sample_rows_shape_ok(d, K), "%s: K = %d samples per clip: need K >= 1 and fewer than 2^31 packed words", fn, (int)K);
    S2VT_REQUIRE(temperature_ok(temperature), "%s: temperature and 1 / temperature must be finite and > 0 (got %g)", fn,
                 (double)temperature);
    S2VT_REQUIRE(sos_ix >= 0 && sos_ix < d->V, "%s: sos_ix %d outside [0, V = %d)", fn, (int)sos_ix, d->V);
    if (trunc) {
        S2VT_REQUIRE(top_k >= 0 && top_k <= d->V, "%s: top_k %d outside [0, V = %d]", fn, (int)top_k, d->V);
        S2VT_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p must be in (0, 1] (got %g)", fn, (double)top_p);
        S2VT_REQUIRE(trunc_vocab_ok(d), "%s: vocab_size %d > 38400", fn, d->V);
    }
    ConstrainArgs ca = {};
    if (con || greedy) {
        int rc0;
        if ((rc0 = check_constraints(fn, con, d->V, greedy, temperature, top_k, top_p, &ca))) return rc0;
        S2VT_REQUIRE(d->L - 1 <= 1024, "%s: length %d: the history of a step holds at most 1023 words", fn, d->L);
        S2VT_REQUIRE((int64_t)d->V > (int64_t)(d->L - 1) + con->n_banned + 1,
                     "%s: vocab_size %d <= (L - 1) + n_banned + 1 = %d: the constraints could ban a whole row", fn, d->V,
                     (int)(d->L - 1 + con->n_banned + 1));
    }
    const bool constrained = con && !constraints_off(con);
    const bool cut = trunc && ((top_k > 0 && top_k < d->V) || top_p < 1.f);
    const SampleRowsWS w = carve_sample_rows(*d, K, workspace, trunc);
    S2VT_REQUIRE(workspace_bytes >= w.bytes, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, w.bytes);
    const int B = d->B, H = d->H, V = d->V, S = d->L - 1, R = B * K, Rp = (int)rows64((size_t)R);
    const int64_t BH = (int64_t)B * H, RH = (int64_t)R * H;
    const bool planes = cache != nullptr;
    S2VT_REQUIRE(!planes || w.himg.p, "%s: a cache needs a plane mode (gemm mode 1 / 3)", fn);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    // ---- 1. encode, once per clip.  With a cache: the decode drivers' encode phase on the plane path (persistent split-precision
    // recurrence; it fills the cache when cache_valid == 0 and refuses, before anything is enqueued, a shape or mode it does not take)
    if (planes) {
        void* scratch = nullptr;
        const size_t sbytes = s2vt_decode_workspace_bytes(d);
        if ((rc = encode_scratch(st, sbytes, &scratch))) return rc;
        if ((rc = s2vt_decode_encode_cached(d, p, feats, scratch, sbytes, cache, cache_bytes, cache_valid, w.states, w.states + BH,
                                            w.states + 2 * BH, w.states + 3 * BH, w.gx_dec, S, stream)))
            return rc;
    } else if ((rc = score_encode_per_step(*d, p, feats, S, w.states, w.gx_dec, Lane{st, w.gws, w.gws_floats, nullptr}))) {
        return rc;
    }
    if ((rc = fill_zero(st, w.err, 4 * sizeof(int)))) return rc;
    if ((rc = rows_clip(st, R, K, Rp, w.row_b))) return rc;
    // every step's packed words start from zero (the heads take an atomic max); rows R .. Rp - 1 stay zero and are never read
    if ((rc = fill_zero(st, w.packed, (size_t)S * Rp * sizeof(unsigned long long)))) return rc;
    // ---- 2. start states of the rows: their clip's word_rnn (h, c)
    const DecodeConst kc = planes ? carve_decode_const(*d, cache) : DecodeConst{};
    // (the whole image once: the steps write the H valid columns of the R rows, the k padding and the pad rows stay zero)
    if (planes && (rc = fill_zero(st, w.himg.p, (size_t)Rp * (size_t)w.himg.ld * sizeof(unsigned short)))) return rc;
    if ((rc = gather_rows_f32(st, w.states + 2 * BH, H, w.row_b, R, H, w.ph))) return rc;
    if ((rc = gather_rows_f32(st, w.states + 3 * BH, H, w.row_b, R, H, w.pc))) return rc;
    // ---- 3. L-1 steps: the word step over the rows, fed <sos> (step 0) or the previous step's packed draw, then the sampling head
    // over the same rows - noise of (seed, step j, batch row r, v)
    const float* hprev = w.ph;
    for (int j = 0; j < S; ++j) {
        unsigned long long* packed = w.packed + (int64_t)j * Rp;
        RowsStep a = {};
        a.R = R; a.err = w.err;
        a.tok_packed = j > 0 ? packed - Rp : nullptr; a.tok_const = sos_ix;
        a.gx = w.gx_dec + (int64_t)j * 4 * BH; a.gx_idx = w.row_b;
        a.h_prev = hprev; a.c_prev = w.pc; a.c_out = w.pc;
        a.h_out = w.ph + ((j + 1) & 1) * RH;
        if (planes) { a.h_planes = w.himg.p; a.ldhp = w.himg.ld; }
        {
            ProfScope ps(st, K_STEP_FWD, 1);
            if ((rc = rows_word_step(st, *d, p, planes ? &kc : nullptr, a))) return rc;
        }
        hprev = a.h_out;
        const GumbelArgs g = gumbel_args(temperature, seed, (uint32_t)j, 0u, (uint32_t)R);
        if (cut || constrained) {
            // out_linear as the beam step runs it (api_beam.hip), then the row kernel: it STORES the rows' packed words
            const Lane ln{st, w.gws, w.gws_floats, nullptr};
            {
                ProfScope pg(st, K_GEMM, 1);
                rc = planes ? pgemm(ln, R, V, H, w.himg, 0, 0, kc.wo, 0, 0, w.logits, V, ID, p->out_b, false)
                            : lgemm(ln, true, true, R, V, H, a.h_out, H, ID, p->out_w, H, ID, w.logits, V, ID, p->out_b, false);
            }
            if (rc) return rc;
            ProfScope ps(st, K_ARGMAX, 1);
            // (constrained: the rows' history is the driver's own packed words of the steps before, [j][Rp])
            rc = constrained ? constrained_draw(st, w.logits, V, R, V, constrain_at(ca, con, w.packed, Rp, j), greedy != 0, top_k, top_p, g,
                                                packed, nullptr)
                             : truncated_draw(st, w.logits, V, R, V, top_k, top_p, g, packed, nullptr);
            if (rc) return rc;
            continue;
        }
        ProfScope ps(st, K_ARGMAX, 1);
        if (planes) {
            ArgmaxX3Args ax;
            memset(&ax, 0, sizeof(ax));
            ax.B = R; ax.V = V; ax.K = kc.wo.kpad;
            ax.W = kc.wo.p; ax.ldw = kc.wo.ld;
            ax.Hp = w.himg.p; ax.ldh = w.himg.ld;
            ax.bias = p->out_b;
            ax.packed = packed;
            rc = logits_argmax_x3(st, ax, greedy ? nullptr : &g);
        } else {
            LogitsArgmaxArgs la;
            la.B = R; la.H = H; la.V = V; la.h = a.h_out; la.ldh = H; la.w_out = p->out_w; la.ldw = H; la.b_out = p->out_b;
            la.packed = packed;
            la.stamps = nullptr;
            rc = logits_argmax(st, la, greedy ? nullptr : &g);
        }
        if (rc) return rc;
    }
    // ---- 4. ids[r][j] of the R rows
    if ((rc = unpack_rows(st, w.packed, S, Rp, R, ids))) return rc;
    return post_async_error(st, w.err, 3);       // (a ring slot: no wait for an earlier call's record)
}

extern "C" {
int s2vt_sample_decode_rows(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t K, int32_t sos_ix, float temperature,
                            uint64_t seed, int64_t* ids, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                            int32_t cache_valid, void* stream) {
    return sample_rows_run("s2vt_sample_decode_rows", false, 0, 1.f, nullptr, 0, d, p, feats, K, sos_ix, temperature, seed, ids, workspace,
                           workspace_bytes, cache, cache_bytes, cache_valid, stream);
}
int s2vt_sample_decode_rows_trunc(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t K, int32_t sos_ix,
                                  float temperature, uint64_t seed, int32_t top_k, float top_p, int64_t* ids, void* workspace,
                                  size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid, void* stream) {
    return sample_rows_run("s2vt_sample_decode_rows_trunc", true, top_k, top_p, nullptr, 0, d, p, feats, K, sos_ix, temperature, seed, ids,
                           workspace, workspace_bytes, cache, cache_bytes, cache_valid, stream);
}
size_t s2vt_decode_rows_constrained_workspace_bytes(const s2vt_dims* d, int32_t K) { return s2vt_sample_rows_trunc_workspace_bytes(d, K); }
int s2vt_decode_rows_constrained(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t K, int32_t sos_ix, int32_t greedy,
                                 float temperature, uint64_t seed, int32_t top_k, float top_p, const s2vt_constraints* c, int64_t* ids,
                                 void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                                 void* stream) {
    S2VT_REQUIRE(c, "s2vt_decode_rows_constrained: null constraints");
    return sample_rows_run("s2vt_decode_rows_constrained", true, top_k, top_p, c, greedy, d, p, feats, K, sos_ix, temperature, seed, ids,
                           workspace, workspace_bytes, cache, cache_bytes, cache_valid, stream);
}
int s2vt_constrained_draw(float* logits, int64_t ld, int64_t rows, int32_t V, const unsigned long long* hist, int64_t hist_ld, int32_t t,
                          const s2vt_constraints* c, int32_t greedy, float temperature, int32_t top_k, float top_p, uint64_t seed,
                          int32_t step, int32_t row0, unsigned long long* packed, int32_t* kept, void* stream) {
    const char* fn = "s2vt_constrained_draw";
    S2VT_REQUIRE(logits && packed && rows > 0 && rows < (1ll << 31) && V > 0 && ld >= V && step >= 0 && row0 >= 0,
                 "%s: null/invalid argument", fn);
    S2VT_REQUIRE((size_t)V * sizeof(float) <= 150 * 1024, "%s: vocab_size %d > 38400", fn, (int)V);
    S2VT_REQUIRE(temperature_ok(temperature), "%s: temperature and 1 / temperature must be finite and > 0 (got %g)", fn, (double)temperature);
    S2VT_REQUIRE(top_k >= 0 && top_k <= V, "%s: top_k %d outside [0, V = %d]", fn, (int)top_k, (int)V);
    S2VT_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p must be in (0, 1] (got %g)", fn, (double)top_p);
    ConstrainArgs ca;
    int rc;
    if ((rc = check_constraints(fn, c, V, greedy, temperature, top_k, top_p, &ca))) return rc;
    S2VT_REQUIRE(t >= 0 && t <= 1023, "%s: t %d outside [0, 1023]", fn, (int)t);
    S2VT_REQUIRE(t == 0 || hist, "%s: null history at t = %d", fn, (int)t);
    S2VT_REQUIRE(t == 0 || hist_ld >= rows, "%s: hist_ld %lld < rows %lld", fn, (long long)hist_ld, (long long)rows);
    ProfScope ps((hipStream_t)stream, K_ARGMAX, 1);
    return constrained_draw((hipStream_t)stream, logits, ld, rows, V, constrain_at(ca, c, hist, hist_ld, t), greedy != 0, top_k, top_p,
                            gumbel_args(temperature, seed, (uint32_t)step, (uint32_t)row0, (uint32_t)row0 + (uint32_t)rows), packed, kept);
}
int s2vt_top20_logprob(const float* logits, int64_t ld, int64_t rows, int32_t V, int32_t* top_ix, float* top_lp, void* stream) {
    S2VT_REQUIRE(logits && top_ix && top_lp && rows > 0 && rows < (1ll << 31) && V > 0 && ld >= V, "s2vt_top20_logprob: null/invalid argument");
    return top20_logprob((hipStream_t)stream, logits, ld, rows, V, top_ix, top_lp);
}
int s2vt_top20_logprob_constrained(float* logits, int64_t ld, int64_t rows, int32_t V, const int32_t* hist, int64_t hist_ld, int32_t t,
                                   const s2vt_constraints* c, int32_t* top_ix, float* top_lp, void* stream) {
    return top20_constrained_checked("s2vt_top20_logprob_constrained", (hipStream_t)stream, logits, ld, rows, V, hist, hist_ld, t, c, top_ix,
                                     top_lp);
}
// the ensemble beam's fan-out head (ensemble.hip); the constrained form behind top20_constrained_checked's checks, and with every
// constraint off the unconstrained launch (the buffers stay untouched)
int s2vt_ensemble_top20(const float* logits, int64_t member_stride, int64_t ld, int32_t M, int64_t rows, int32_t V, const float* log_w,
                        int32_t* top_ix, float* top_lp, void* stream) {
    return ensemble_top20("s2vt_ensemble_top20", (hipStream_t)stream, logits, member_stride, ld, M, rows, V, log_w, top_ix, top_lp);
}
int s2vt_ensemble_top20_constrained(float* logits, int64_t member_stride, int64_t ld, int32_t M, int64_t rows, int32_t V, const float* log_w,
                                    const int32_t* hist, int64_t hist_ld, int32_t t, const s2vt_constraints* c, int32_t* top_ix,
                                    float* top_lp, void* stream) {
    const char* fn = "s2vt_ensemble_top20_constrained";
    S2VT_REQUIRE(V >= 20 && (size_t)V * sizeof(float) <= 150 * 1024, "%s: vocab_size %d outside [20, 38400]", fn, (int)V);
    ConstrainArgs ca;
    int rc;
    if ((rc = check_constraints(fn, c, V, 0, 1.f, 0, 1.f, &ca))) return rc;
    S2VT_REQUIRE(t >= 0 && t <= 1023, "%s: t %d outside [0, 1023]", fn, (int)t);
    S2VT_REQUIRE(t == 0 || hist, "%s: null history at t = %d", fn, (int)t);
    S2VT_REQUIRE(t == 0 || hist_ld >= t, "%s: hist_ld %lld < t %d", fn, (long long)hist_ld, (int)t);
    if (constraints_off(c)) return ensemble_top20(fn, (hipStream_t)stream, logits, member_stride, ld, M, rows, V, log_w, top_ix, top_lp);
    return ensemble_top20_constrained(fn, (hipStream_t)stream, logits, member_stride, ld, M, rows, V, log_w, constrain_at(ca, c, nullptr, 0, t),
                                      hist, hist_ld, top_ix, top_lp);
}
int s2vt_truncated_draw(const float* logits, int64_t ld, int64_t rows, int32_t V, float temperature, int32_t top_k, float top_p,
                        uint64_t seed, int32_t step, int32_t row0, unsigned long long* packed, int32_t* kept, void* stream) {
    S2VT_REQUIRE(logits && packed && rows > 0 && rows < (1ll << 31) && V > 0 && ld >= V && step >= 0 && row0 >= 0,
                 "s2vt_truncated_draw: null/invalid argument");
    S2VT_REQUIRE((size_t)V * sizeof(float) <= 150 * 1024, "s2vt_truncated_draw: vocab_size %d > 38400", (int)V);
    S2VT_REQUIRE(temperature_ok(temperature), "s2vt_truncated_draw: temperature and 1 / temperature must be finite and > 0 (got %g)",
                 (double)temperature);
    S2VT_REQUIRE(top_k >= 0 && top_k <= V, "s2vt_truncated_draw: top_k %d outside [0, V = %d]", (int)top_k, (int)V);
    S2VT_REQUIRE(top_p > 0.f && top_p <= 1.f, "s2vt_truncated_draw: top_p must be in (0, 1] (got %g)", (double)top_p);
    ProfScope ps((hipStream_t)stream, K_ARGMAX, 1);
    return truncated_draw((hipStream_t)stream, logits, ld, rows, V, top_k, top_p,
                          gumbel_args(temperature, seed, (uint32_t)step, (uint32_t)row0, (uint32_t)row0 + (uint32_t)rows), packed, kept);
}
}
