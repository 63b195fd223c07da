// Teacher-forced caption scoring (S2VT.forward(mode='score'); not in the reference): the log-likelihood of given captions, K per
// clip, in the arithmetic of mode='train' without dropout (S2VTModel.py:63-81 for the logits, :214 for the log_softmax).  One encode
// per clip (the decode drivers' encode phase), T-1 word steps over the fixed rows r = b * K + k (the beam searches' step,
// rows_word_step), then out_linear over ALL steps' hidden states in chunks of S2VT_SCORE_HEAD_ROWS rows, each followed by the
// one-token log_softmax kernel (ce.hip), and one finisher launch.  Everything on the caller's stream, no host round trip.
#include "api_internal.h"

using namespace s2vt;

extern "C" {

// The caller's workspace: what the word steps, the head and the finisher work on - tokens, per-token log-probs, the encode phase's
// results, the h_t row image of all steps and ONE chunk of logits.
struct ScoreWS {
    int32_t *tok, *row_b;            // [T][Rp] time-major tokens (clamped), [Rp] clip of each row
    int* err;
    float *lp, *powa;                // [T-1][Rp] per-token log-probs by image row, fp32(n ** alpha) for n = 0..T-1
    float *states, *gx_dec;          // vid_h, vid_c, word_h, word_c [B][H] after the L frames; [T-1][B][4H] vid_rnn's half of the gate input
    float *ph, *pc;                  // [2][R][H] h_t ping-pong (plane path), [R][H] c_t
    float* gws; size_t gws_floats;
    char* head;                      // carve_score_head
    size_t bytes;
};
struct ScoreHead { PB himg; float *hrows, *logits; size_t bytes; };      // himg: plane path, hrows: fp32 [(T-1) * Rp][H]
struct ScoreEnc { float *bsum1, *bsum2, *x1, *gxb, *h1, *c1, *h2, *c2; size_t bytes; };
static ScoreHead carve_score_head(const s2vt_dims& d, size_t rows, bool planes, void* base) {
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    ScoreHead h;
    h.hrows = nullptr;
    if (planes) h.himg = take_planes(c, rows, d.H, DECODE_PLANES);
    else h.hrows = c.take<float>(rows * (size_t)d.H);
    h.logits = c.take<float>((size_t)S2VT_SCORE_HEAD_ROWS * d.V);
    h.bytes = align_up(c.off, 256);
    return h;
}
static ScoreEnc carve_score_enc(const s2vt_dims& d, int S, void* base) {
    const size_t B = d.B, L = d.L, H = d.H, Tv = L + S;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    ScoreEnc e;
    e.bsum1 = c.take<float>(4 * H); e.bsum2 = c.take<float>(4 * H);
    e.x1 = c.take<float>(L * B * H);
    e.gxb = c.take<float>(Tv * B * 4 * H);       // vid_rnn's gate input [L], then word_rnn's vid_out half [L + S]
    e.h1 = c.take<float>(Tv * B * H); e.c1 = c.take<float>(Tv * B * H);
    e.h2 = c.take<float>(L * B * H); e.c2 = c.take<float>(L * B * H);
    e.bytes = align_up(c.off, 256);
    return e;
}
static bool score_shape_ok(const s2vt_dims* d, int K, int T) {
    return dims_ok(d) && K >= 1 && T >= 2 && T <= d->L && (int64_t)T * (int64_t)rows64((size_t)d->B * K) < (1ll << 31);
}
static ScoreWS carve_score(const s2vt_dims& d, int K, int T, void* base) {
    const size_t B = d.B, H = d.H, R = B * K, Rp = rows64(R), S = T - 1;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    ScoreWS w;
    w.tok = c.take<int32_t>((size_t)T * Rp); w.row_b = c.take<int32_t>(Rp);
    w.err = c.take<int>(4);
    w.lp = c.take<float>(S * Rp); w.powa = c.take<float>(T);
    w.states = c.take<float>(4 * B * H); w.gx_dec = c.take<float>(S * B * 4 * H);
    w.ph = c.take<float>(2 * R * H); w.pc = c.take<float>(R * H);
    w.gws_floats = (size_t)4 << 20;
    w.gws = c.take<float>(w.gws_floats);
    // (sized for either path: which one a call takes depends on its cache argument)
    size_t s = carve_score_head(d, S * Rp, false, nullptr).bytes;
    if (gemm_mode() != 0) s = std::max(s, carve_score_head(d, S * Rp, true, nullptr).bytes);
    w.head = c.take<char>(align_up(s, 256));
    w.bytes = align_up(c.off, 256);
    return w;
}
size_t s2vt_score_workspace_bytes(const s2vt_dims* d, int32_t K, int32_t T) {
    return score_shape_ok(d, K, T) ? carve_score(*d, K, T, nullptr).bytes : 0;
}

// The encode phase's scratch is NOT part of the caller's workspace: the decode drivers' encode phase works in a decode workspace
// (s2vt_decode_workspace_bytes: 2.6 GB at B = 128, L = 80, H = 1000, several times everything a scoring call keeps), all of it dead
// once the states and vid_rnn's gate-input rows are handed out.  The library keeps one such buffer per (device, stream) and grows
// it on demand - hipMalloc / hipFree, so a call that grows it synchronises the device once; every other call allocates nothing.
// Calls on one stream are stream-ordered, so they can share it; calls on different streams get different buffers.
}  // (C linkage ends: the encode phase is shared with api_sample_rows.hip, see api_internal.h)
namespace s2vt {
int encode_scratch(hipStream_t st, size_t bytes, void** out) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, std::pair<void*, size_t>> bufs;
    int dev = 0;
    S2VT_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto& e = bufs[std::make_pair(dev, st)];
    if (e.second < bytes) {
        if (e.first) S2VT_HIP(hipFree(e.first));         // (waits for the device: nothing reads the old buffer any more)
        e = std::make_pair((void*)nullptr, (size_t)0);
        void* p = nullptr;
        S2VT_HIP(hipMalloc(&p, bytes));
        e = std::make_pair(p, bytes);
    }
    *out = e.first;
    return 0;
}

// The encode phase as launches per timestep on the fp32-input MFMA (S2VTModel.py:54, 64-67 of mode='train' without its dropout):
// feature projection, vid_rnn over the L frames and its S input-free decode steps, their half of word_rnn's gate input, word_rnn
// over the L frames with a zero embedding.  Leaves what the word steps start from in states / gx_dec.
int score_encode_per_step(const s2vt_dims& d, const s2vt_params* p, const float* feats, int S, float* states, float* gx_dec, const Lane& ln) {
    const int B = d.B, L = d.L, H = d.H, E = d.E, Tv = L + S;
    const int64_t BH = (int64_t)B * H;
    hipStream_t st = ln.s;
    void* scratch = nullptr;
    if (int r = encode_scratch(st, carve_score_enc(d, S, nullptr).bytes, &scratch)) return r;
    const ScoreEnc e = carve_score_enc(d, S, scratch);
    int rc;
    if ((rc = bias_sums(st, p, H, e.bsum1, e.bsum2))) return rc;
    if ((rc = project_features_f32(ln, d, p, feats, e.x1, e.gxb, e.bsum1))) return rc;
    if ((rc = seq_fwd(st, 0, Tv, B, H, e.gxb, L, e.bsum1, p->vid_w_hh, e.h1, e.c1, false))) return rc;
    if ((rc = lgemm(ln, true, true, Tv * B, 4 * H, H, e.h1, H, ID, p->word_w_ih + E, E + H, ID, e.gxb, 4 * H, ID, e.bsum2, false))) return rc;
    if ((rc = seq_fwd(st, 0, L, B, H, e.gxb, L, e.bsum2, p->word_w_hh, e.h2, e.c2, false))) return rc;
    const float* last[4] = {e.h1 + (L - 1) * BH, e.c1 + (L - 1) * BH, e.h2 + (L - 1) * BH, e.c2 + (L - 1) * BH};
    for (int k = 0; k < 4; ++k)
        S2VT_HIP(hipMemcpyAsync(states + k * BH, last[k], (size_t)BH * sizeof(float), hipMemcpyDeviceToDevice, st));
    S2VT_HIP(hipMemcpyAsync(gx_dec, e.gxb + (int64_t)L * 4 * BH, (size_t)S * 4 * BH * sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
}
}  // namespace s2vt
extern "C" {

int s2vt_score_captions(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* captions, int64_t stride_b,
                        int64_t stride_k, int32_t K, int32_t T, int32_t eos_ix, double length_alpha, float* token_lp, float* score,
                        int64_t* length, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                        void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && captions && token_lp && score && length && workspace, "s2vt_score_captions: null/invalid argument");
    S2VT_REQUIRE(score_shape_ok(d, K, T), "s2vt_score_captions: K = %d candidates of T = %d tokens: need K >= 1, 2 <= T <= L = %d", (int)K,
                 (int)T, d->L);
    S2VT_REQUIRE(stride_b >= 0 && stride_k >= 0, "s2vt_score_captions: negative caption stride");
    S2VT_REQUIRE(length_alpha >= 0 && length_alpha <= 1.7e308, "s2vt_score_captions: length_alpha must be finite and >= 0 (got %g)", length_alpha);
    const ScoreWS w = carve_score(*d, K, T, workspace);
    S2VT_REQUIRE(workspace_bytes >= w.bytes, "s2vt_score_captions: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    const int B = d->B, H = d->H, V = d->V, S = T - 1, R = B * K, Rp = (int)rows64((size_t)R);
    const int64_t BH = (int64_t)B * H, RH = (int64_t)R * H;
    const bool planes = cache != nullptr;
    hipStream_t st = (hipStream_t)stream;
    const float* powtab = length_pow_table(length_alpha, T - 1);
    S2VT_REQUIRE(powtab, "s2vt_score_captions: no pinned memory for the length table");
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
    if ((rc = score_prep(st, captions, stride_b, stride_k, R, K, T, Rp, V, w.tok, w.row_b, w.err))) return rc;
    S2VT_HIP(hipMemcpyAsync(w.powa, powtab, (size_t)T * sizeof(float), hipMemcpyHostToDevice, st));
    // ---- 2. T-1 word steps over the fixed rows: every row keeps its own state, reads its clip's gate input (row_b) and token c[j];
    // h_t of step j goes to rows [j * Rp, j * Rp + R) of the head's row image
    const ScoreHead hd = carve_score_head(*d, (size_t)S * Rp, planes, w.head);
    const DecodeConst kc = planes ? carve_decode_const(*d, cache) : DecodeConst{};
    if (planes) rc = fill_zero(st, hd.himg.p, (size_t)S * Rp * (size_t)hd.himg.ld * sizeof(unsigned short));
    else rc = fill_zero(st, hd.hrows, (size_t)S * Rp * H * sizeof(float));
    if (rc) return rc;
    if ((rc = gather_rows_f32(st, w.states + 2 * BH, H, w.row_b, R, H, w.ph))) return rc;
    if ((rc = gather_rows_f32(st, w.states + 3 * BH, H, w.row_b, R, H, w.pc))) return rc;
    const float* hprev = w.ph;
    {
        ProfScope ps(st, K_STEP_FWD, S);
        for (int j = 0; j < S; ++j) {
            RowsStep a = {};
            a.R = R; a.tok = w.tok + (int64_t)j * Rp; a.err = w.err;
            a.gx = w.gx_dec + (int64_t)j * 4 * BH; a.gx_idx = w.row_b;
            a.h_prev = hprev; a.c_prev = w.pc; a.c_out = w.pc;
            if (planes) {
                a.h_out = w.ph + ((j + 1) & 1) * RH;
                a.h_planes = hd.himg.p + (int64_t)j * Rp * hd.himg.ld; a.ldhp = hd.himg.ld;
            } else {
                a.h_out = hd.hrows + (int64_t)j * Rp * H;
            }
            if ((rc = rows_word_step(st, *d, p, planes ? &kc : nullptr, a))) return rc;
            hprev = a.h_out;
        }
    }
    // ---- 3. head: out_linear (S2VTModel.py:80) over the image in chunks of S2VT_SCORE_HEAD_ROWS rows into ONE logits buffer, the
    // log-prob of each row's next token c[j + 1] behind every chunk
    const Lane ln{st, w.gws, w.gws_floats, nullptr};
    const int64_t NR = (int64_t)S * Rp;
    for (int64_t q = 0; q < NR; q += S2VT_SCORE_HEAD_ROWS) {
        const int m = (int)std::min<int64_t>(S2VT_SCORE_HEAD_ROWS, NR - q);
        if (planes) rc = pgemm(ln, m, V, H, hd.himg, (int)q, 0, kc.wo, 0, 0, hd.logits, V, ID, p->out_b, false);
        else rc = lgemm(ln, true, true, m, V, H, hd.hrows + q * H, H, ID, p->out_w, H, ID, hd.logits, V, ID, p->out_b, false);
        if (rc) return rc;
        ProfScope ps(st, K_CE, 1);
        if ((rc = pick_logprob(st, hd.logits, V, m, V, w.tok + Rp + q, w.lp + q, w.err))) return rc;
    }
    // ---- 4. lengths, masked sums, scores
    if ((rc = score_finish(st, w.lp, w.tok, R, Rp, T, eos_ix, w.powa, token_lp, score, length))) return rc;
    return post_async_error(st, w.err, 3);       // (a ring slot: no wait for an earlier call's record)
}

int s2vt_pick_logprob(const float* logits, int64_t ld, int64_t rows, int32_t V, const int32_t* target, float* lp_out, int32_t* err_flag,
                      void* stream) {
    S2VT_REQUIRE(logits && target && lp_out && rows >= 0 && rows < (1ll << 31) && V > 0 && ld >= V, "s2vt_pick_logprob: bad arguments");
    ProfScope ps((hipStream_t)stream, K_CE, 1);
    return pick_logprob((hipStream_t)stream, logits, ld, rows, V, target, lp_out, err_flag);
}
}
