// Greedy decode (S2VTModel.py:82-110, mode='test') with its sampled and scheduled variants, its encode phase handed out for the beam
// search, the decode step's out_linear + argmax entry points.  One DecodeDriver per call; decode_plan (api_internal.h) picks the schedule.
#include "api_internal.h"

using namespace s2vt;

extern "C" {

// ------------------------------------------------------------------ greedy decode
struct DecodeWS {
    float *bsum1, *bsum2, *x1, *gx1, *h1, *c1, *gx2, *h2, *c2, *gws_a, *gws_b;
    float* zbuf;                           // [B][4H]: h_t·W_hh^T, the recurrent half of the next decode step's gates
    size_t gws_floats;
    unsigned long long* packed;
    PB feats, px1, ph1;                    // packed planes of per-call activations (split-precision mode only)
    PB ph2;                                // the decode step's h_t planes
    PB embp, wep;                          // planes of the embedding table and of W_e (scratch of the per-token table's GEMM)
    // persistent split-precision recurrence of the ENCODE phase (lstm_persist_x3.hip): per-step cell states, word_rnn's encode
    // outputs, the h_t plane images of both layers, hand-off counters, error flags (xkp == 0: not provided)
    int64_t xkp;
    float *c1_all, *c2_all, *h2_all;
    unsigned short *xh1, *xh2;
    unsigned int *psync_a, *psync_b;
    int* err;
    size_t bytes;
};
static DecodeWS carve_decode(const s2vt_dims& d, void* base) {
    const size_t B = d.B, L = d.L, F = d.F, H = d.H, T = 2 * L - 1;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    DecodeWS w;
    w.bsum1 = c.take<float>(4 * H); w.bsum2 = c.take<float>(4 * H);
    w.x1 = c.take<float>(L * B * H);
    w.gx1 = c.take<float>(L * B * 4 * H);
    w.h1 = c.take<float>(T * B * H);
    w.c1 = c.take<float>(B * H);
    w.gx2 = c.take<float>(T * B * 4 * H);
    w.h2 = c.take<float>(2 * B * H);
    w.c2 = c.take<float>(B * H);
    w.zbuf = c.take<float>(B * 4 * H);
    w.packed = c.take<unsigned long long>((L - 1) * B);
    w.gws_floats = gemm_ws_floats(d);
    w.gws_a = c.take<float>(w.gws_floats); w.gws_b = c.take<float>(w.gws_floats);
    if (planes_ok(d)) {
        w.feats = take_planes(c, B * L, F, DECODE_PLANES); w.px1 = take_planes(c, L * B, H, DECODE_PLANES);
        w.ph1 = take_planes(c, T * B, H, DECODE_PLANES);   w.ph2 = take_planes(c, B, H, DECODE_PLANES);
        w.embp = take_planes(c, d.V, d.E, DECODE_PLANES);  w.wep = take_planes(c, 4 * H, d.E, DECODE_PLANES);
    }
    // (0: the persistent encode phase is not selectable.  The plan WITHOUT its device query - a size function works without a GPU -
    // so the carve is broader than the plan: wherever decode_plan selects the persistent encode, the workspace provides for it)
    w.xkp = decode_plan(d, false, false).persist_encode ? (int64_t)pad64((int)H) : 0;
    w.c1_all = c.take<float>(w.xkp ? T * B * H : 0);
    w.c2_all = c.take<float>(w.xkp ? L * B * H : 0); w.h2_all = c.take<float>(w.xkp ? L * B * H : 0);
    w.xh1 = c.take<unsigned short>(w.xkp ? 3 * T * B * (size_t)w.xkp : 0); w.xh2 = c.take<unsigned short>(w.xkp ? 3 * L * B * (size_t)w.xkp : 0);
    w.psync_a = c.take<unsigned int>(lstm_persist_sync_bytes() / sizeof(unsigned int));
    w.psync_b = c.take<unsigned int>(lstm_persist_sync_bytes() / sizeof(unsigned int));
    w.err = c.take<int>(4);
    w.bytes = align_up(c.off, 256);
    return w;
}
}  // (C linkage ends: carve_decode_const is shared with api_beam.hip, see api_internal.h)
namespace s2vt {
DecodeConst carve_decode_const(const s2vt_dims& d, void* base) {
    const size_t F = d.F, H = d.H;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    DecodeConst k;
    k.gtab = nullptr; k.xw1 = k.xw2 = nullptr;      // (the images: PB{})
    if (gemm_mode() != 0) {     // (the images depend on the weights' dims only: one cache serves every batch size)
        k.wf = take_planes(c, H, F, DECODE_PLANES);     k.wih1 = take_planes(c, 4 * H, H, DECODE_PLANES);
        k.wv = take_planes(c, 4 * H, H, DECODE_PLANES); k.wo = take_planes(c, d.V, H, DECODE_PLANES);
        k.gtab = c.take<float>((size_t)d.V * 4 * H);
        const size_t xkp = (H <= 1024) ? (size_t)pad64((int)H) : 0;
        k.xw1 = c.take<unsigned short>(3 * 4 * H * xkp); k.xw2 = c.take<unsigned short>(3 * 4 * H * xkp);
        k.whh = take_planes(c, 4 * H, H, DECODE_PLANES);       // (last: the images in front keep their offsets)
    }
    k.bytes = align_up(c.off, 256);
    return k;
}
}  // namespace s2vt
extern "C" {

// Batches that are not multiples of 64 are padded inside the workspace, like the train drivers' (api_train.hip): zero features for
// the pad samples, whose ids / states are never handed out.  A plain greedy decode of fewer than 24 clips (eval.py:27 decodes 10 at
// a time) is the exception (batch_pads): there the launch-per-timestep path - 16-row fp32-MFMA tiles, gate GEMVs up to B = 4 - is
// faster than 64 padded rows on the plane path; the encode phase for the beam search always takes the plane path (decode_plan).
struct DecodePad { float* feats; int64_t* ids; float* states; float* gx_dec; size_t bytes; };
static DecodePad carve_decode_pad(const s2vt_dims& d, const s2vt_dims& dp, void* base) {
    const size_t Bp = dp.B, L = d.L, F = d.F, H = d.H;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    DecodePad w;
    w.feats = c.take<float>(Bp * L * F);
    w.ids = c.take<int64_t>(Bp * (L - 1));
    w.states = c.take<float>(4 * Bp * H);                  // vid_h, vid_c, word_h, word_c of s2vt_decode_encode_cached
    w.gx_dec = c.take<float>((L - 1) * Bp * 4 * H);
    w.bytes = align_up(c.off, 256);
    return w;
}
static size_t decode_core_bytes(const s2vt_dims& d) { return align_up(carve_decode(d, nullptr).bytes + carve_decode_const(d, nullptr).bytes, 256); }
size_t s2vt_decode_workspace_bytes(const s2vt_dims* d) {
    if (!dims_ok(d)) return 0;
    if (decode_plan(*d, true, false).padded) {       // (sized for either use of the workspace: s2vt_decode_encode_cached pads every ragged batch)
        const s2vt_dims dp = padded_dims(*d);
        return decode_core_bytes(dp) + carve_decode_pad(*d, dp, nullptr).bytes;
    }
    return carve_decode(*d, nullptr).bytes + carve_decode_const(*d, nullptr).bytes;
}
size_t s2vt_decode_cache_bytes(const s2vt_dims* d) { return dims_ok(d) ? carve_decode_const(*d, nullptr).bytes : 0; }
int32_t s2vt_decode_uses_cache(const s2vt_dims* d) { return (dims_ok(d) && decode_plan(*d, false, false).planes) ? 1 : 0; }
int s2vt_decode_plan(const s2vt_dims* d, int32_t encode_only, int32_t* padded_B, int32_t* persist_encode, int32_t* schedule) {
    S2VT_REQUIRE(dims_ok(d) && padded_B && persist_encode && schedule, "s2vt_decode_plan: null/invalid argument");
    const DecodePlan pl = decode_plan(*d, encode_only != 0);
    *padded_B = pl.B; *persist_encode = pl.persist_encode ? 1 : 0; *schedule = pl.schedule;
    return 0;
}
int s2vt_set_decode_schedule(int32_t schedule) { return option_set(O_DECODE_FUSED, (schedule == 0 || schedule == 1) ? schedule : -1); }

// The three modes of a decode call, each a value with an "on" flag.  enc: the encode phase alone - the states [B, H] after the L
// encode steps; optional: word_rnn's vid_out gate input (+ biases) of the first `depth` decode steps [depth][B][4H].  smp:
// mode='sample'.  ss: scheduled sampling (s2vt_scheduled_decode) - the ground-truth words, the coin's probability and seed, and where
// the words that were fed (used) and every step's own choice (draws, optional) go: both [rows][L-1] for the rows of the caller's batch
struct EncodeOut { float *vid_h, *vid_c, *word_h, *word_c; float* gx_dec; int depth; bool on; };
struct Draw { GumbelArgs g; bool on; const GumbelArgs* ptr() const { return on ? &g : nullptr; } };
struct SchedArgs { const int64_t* targets; int64_t ldt; float p; uint32_t seed_lo, seed_hi; uint32_t rows; int64_t* used; int64_t* draws; bool on; };
struct DecodeModes { EncodeOut enc; Draw smp; SchedArgs ss; };
// out_linear + argmax of nb rows on the fp32-input MFMA (lstm.hip) ...
static LogitsArgmaxArgs logits_argmax_args(int nb, int H, int V, const float* h, const float* w_out, const float* b_out, unsigned long long* packed) {
    LogitsArgmaxArgs la;
    la.B = nb; la.H = H; la.V = V; la.h = h; la.ldh = H; la.w_out = w_out; la.ldw = H; la.b_out = b_out;
    la.packed = packed;
    la.stamps = nullptr;
    return la;
}
// ... and on the plane path (argmax_x3.hip): W_o and the rows' h_t as blocked 3-plane images
static ArgmaxX3Args argmax_x3_args(int nb, int V, const PB& wo, const unsigned short* hp, int64_t ldh, const float* bias,
                                   unsigned long long* packed) {
    ArgmaxX3Args ax;
    memset(&ax, 0, sizeof(ax));
    ax.B = nb; ax.V = V; ax.K = wo.kpad;
    ax.W = wo.p; ax.ldw = wo.ld;
    ax.Hp = hp; ax.ldh = ldh;
    ax.bias = bias;
    ax.packed = packed;
    return ax;
}
// What every schedule of a decode works with - dims, parameters, the workspace and weight-image views, the modes, the plan, the lane
// frame (Lanes; la: vid_rnn's lane on the caller's stream, lb: word_rnn's - encode, then the 79 decode steps) - and the call shapes
// the schedules share.  Lives on the stack of one greedy_decode_core call.
struct DecodeDriver : Lanes {
    const s2vt_params* p; const float* feats; int64_t* ids;
    const DecodeWS& w; const DecodeConst& kc; const DecodeModes& m; const DecodePlan pl;
    const int B, L, F, H, E, V, T, sos_ix;
    const int64_t BH, B4H;
    const bool fill, fill_all;        // see fill_weight_images
    const bool px;                    // the plan's persistent encode, and the workspace provides for it
    DecodeDriver(const s2vt_dims* d, const s2vt_params* p_, const float* feats_, int32_t sos_ix_, int64_t* ids_, const DecodeWS& w_,
                 const DecodeConst& kc_, const DecodeModes& m_, const DecodePlan& pl_, bool cached, bool cache_valid)
        : p(p_), feats(feats_), ids(ids_), w(w_), kc(kc_), m(m_), pl(pl_), B(d->B), L(d->L), F(d->F), H(d->H), E(d->E), V(d->V),
          T(2 * d->L - 1), sos_ix(sos_ix_), BH((int64_t)d->B * d->H), B4H(4 * (int64_t)d->B * d->H), fill(!(cached && cache_valid)),
          fill_all(fill && cached), px(pl_.persist_encode && w_.xkp > 0) {}
    int open_lanes(hipStream_t caller) { return open(caller, w.gws_a, w.gws_b, w.gws_floats, nullptr, nullptr); }
    // the plan's token schedule, ANDed with what only the driver knows (the fused launch needs W_hh's image with W_o's k padding)
    DecSchedule schedule() const {
        if (!px) return DEC_PER_STEP;
        return (pl.schedule == DEC_FUSED && !(kc.whh.p && kc.whh.kpad == kc.wo.kpad)) ? DEC_TWO_CHAINS : pl.schedule;
    }
    // Lane B's weight-derived images (lane A's two, W_f and W_ih1: project_features), built when the call has no valid cache (fill).
    // A caller-kept cache outlives this call's choices (batch size, recurrence mode, pipeline block, experiment switches): a call that
    // fills it builds EVERY weight-derived image it holds, not only the ones this call reads (fill_all: the W_hh planes of the
    // persistent encode) - a later call on the same weights with another batch or mode then finds its images whatever it selects
    // (cache_valid says "the weights stand", nothing about who filled it).
    int fill_weight_images() {
        int rc;
        if (!pl.planes) return 0;
        if (fill && H <= 1024 && (px || fill_all)) {       // W_hh planes, rows of pad64(H) (carve_decode_const)
            const int ckp = pad64(H);
            if ((rc = split3_rows(sx, p->vid_w_hh, H, 4 * H, H, ckp, kc.xw1, 4 * (int64_t)H * ckp))) return rc;
            if ((rc = split3_rows(sx, p->word_w_hh, H, 4 * H, H, ckp, kc.xw2, 4 * (int64_t)H * ckp))) return rc;
        }
        // W_o planes: constant over the decode steps; h_t planes: written by the decode steps themselves, k padding zeroed here
        if (fill && (rc = psplit(lb, kc.wo, 0, p->out_w, H, ID, V, H))) return rc;
        if ((rc = fill_zero(sx, w.ph2.p, rows64((size_t)B) * (size_t)w.ph2.ld * sizeof(unsigned short)))) return rc;
        if (!fill) return 0;
        // per-token gate-input table instead of the embedding K segment of the 79 decode steps: gtab[v] = Emb[v]·W_e^T for every token
        // (S2VTModel.py:90-93,100-103: embedding + the embed columns of word_rnn's W_ih) - one V x 4H x E GEMM (0.5 ms at V = 12000)
        // against B x 4H x E of MFMA work and E/(E+H) of the operand traffic in EVERY decode step: pays from B ~ 64
        if ((rc = psplit(lb, w.embp, 0, p->emb_w, E, ID, V, E))) return rc;
        if ((rc = psplit(lb, w.wep, 0, p->word_w_ih, E + H, ID, 4 * H, E))) return rc;
        if ((rc = pgemm(lb, V, 4 * H, E, w.embp, 0, 0, w.wep, 0, 0, kc.gtab, 4 * H, ID, nullptr, false))) return rc;
        if ((rc = psplit(lb, kc.wv, 0, p->word_w_ih + E, E + H, ID, 4 * H, H))) return rc;
        return psplit(lb, kc.whh, 0, p->word_w_hh, H, ID, 4 * H, H);
    }
    // feature projection + vid_rnn input GEMM on lane A                                  S2VTModel.py:54, 64-67
    int project_features() {
        int rc;
        if (!pl.planes) return project_features_f32(la, s2vt_dims{B, L, F, H, E, V}, p, feats, w.x1, w.gx1, w.bsum1);
        if ((rc = psplit(la, w.feats, 0, feats, F, ID, B * L, F))) return rc;
        if (fill && (rc = psplit(la, kc.wf, 0, p->feat_w, F, ID, H, F))) return rc;
        if (fill && (rc = psplit(la, kc.wih1, 0, p->vid_w_ih, H, ID, 4 * H, H))) return rc;
        if ((rc = pgemm(la, B * L, H, F, w.feats, 0, 0, kc.wf, 0, 0, w.x1, H, perm(L, B), p->feat_b, false))) return rc;
        if ((rc = psplit(la, w.px1, 0, w.x1, H, ID, L * B, H))) return rc;
        return pgemm(la, L * B, 4 * H, H, w.px1, 0, 0, kc.wih1, 0, 0, w.gx1, 4 * H, ID, w.bsum1, false);
    }
    // one word_rnn step (+ out_linear / argmax for a decode step): encode steps see a zero embedding (:84-86), decode steps
    // Emb[prev token] (:89-103)
    // (b0, nb): the batch rows [b0, b0 + nb) of the step - the whole batch, or one half of it when the decode runs as two
    // independent chains on two streams (b0 a multiple of 64: the plane images are blocked by 64 rows)
    StepFwdArgs word_step_args(int t, const float* hprev, const float* cprev, int b0, int nb) const {
        const int64_t o1 = (int64_t)b0 * H, o4 = 4 * o1;
        StepFwdArgs a;
        memset(&a, 0, sizeof(a));
        a.B = nb; a.H = H;
        a.h_prev = hprev ? hprev + o1 : nullptr; a.ldh = H;
        a.w_hh = p->word_w_hh; a.ldw = H;
        if (t >= L) {
            if (pl.planes) {
                a.gx_tab = kc.gtab; a.ldtab = 4 * (int64_t)H;
            } else {
                a.x2 = p->emb_w; a.ldx2 = E; a.K2 = E;
                a.w2 = p->word_w_ih; a.ldw2 = E + H;
            }
            a.tok.tok_packed = (t > L) ? w.packed + (int64_t)(t - L - 1) * B + b0 : nullptr;
            a.tok.tok_const = sos_ix;
            // the packed word is the previous step's argmax: a producer that left it unwritten would decode as token
            // 0xFFFFFFFF - clamped and flagged (w.err[0], S2VT_ERR_INDEX) instead of read from beyond the table
            a.tok.tok_limit = V; a.tok.tok_err = w.err;
            if (m.ss.on) {      // scheduled sampling: the coin of (batch row, decode step) picks the packed word or the ground truth
                a.tok.ss = SsArgs{m.ss.targets + (int64_t)b0 * m.ss.ldt, m.ss.ldt, m.ss.p, m.ss.seed_lo, m.ss.seed_hi, (uint32_t)(t - L),
                                  (uint32_t)b0, m.ss.rows};
            }
        }
        a.gx = w.gx2 + t * B4H + o4; a.ldgx = 4 * (int64_t)H;
        a.c_prev = cprev ? cprev + o1 : nullptr; a.ldc = H;
        a.h_out = w.h2 + (t & 1) * BH + o1; a.ldho = H;
        a.c_out = w.c2 + o1; a.ldco = H;
        if (t >= L && pl.planes) { a.h_planes = w.ph2.p + (int64_t)b0 * w.ph2.ld; a.ldhp = w.ph2.ld; }
        return a;
    }
    ArgmaxX3Args argmax_x3_args(int b0, int nb, unsigned long long* packed) const {
        return ::argmax_x3_args(nb, V, kc.wo, w.ph2.p + (int64_t)b0 * w.ph2.ld, w.ph2.ld, p->out_b, packed);
    }
    // mode='sample': the launch of decode step t - L over the batch rows from b0 draws instead of taking the arg-max
    Draw gumbel_at(int t, int b0) const {
        Draw g = m.smp;
        g.g.step = (uint32_t)(t - L); g.g.row0 = (uint32_t)b0;
        return g;
    }
    int word_step(hipStream_t s, int t, const float* hprev, const float* cprev, int b0, int nb) {
        {
            ProfScope ps(s, K_STEP_FWD, 1);
            if (const int r = lstm_step_fwd(s, word_step_args(t, hprev, cprev, b0, nb))) return r;
        }
        if (t < L) return 0;
        ProfScope ps(s, K_ARGMAX, 1);
        const Draw g = gumbel_at(t, b0);
        unsigned long long* packed = w.packed + (int64_t)(t - L) * B + b0;
        // out_linear + argmax (:95-96, :105-106) on the bf16 matrix cores: the step kernel above wrote h_t as planes (StepFwdArgs::h_planes)
        if (pl.planes) return logits_argmax_x3(s, argmax_x3_args(b0, nb, packed), g.ptr());
        // the same on the fp32-input MFMA, for batches the plane path does not take
        return logits_argmax(s, logits_argmax_args(nb, H, V, w.h2 + (t & 1) * BH + (int64_t)b0 * H, p->out_w, p->out_b, packed), g.ptr());
    }
    // the packed words of the L - 1 steps as ids - or, scheduled, as the words that were fed and the draws (caller's rows only) - and
    // the call's device-side error flags (a timed-out hand-off surfaces like the train path's)
    int finish() {
        int rc = 0;
        if (m.ss.on) {
            SsArgs sa;
            memset(&sa, 0, sizeof(sa));
            sa.forced = m.ss.targets; sa.ld = m.ss.ldt; sa.p = m.ss.p; sa.seed_lo = m.ss.seed_lo; sa.seed_hi = m.ss.seed_hi; sa.rows = m.ss.rows;
            rc = unpack_scheduled(st, w.packed, L - 1, B, std::min(B, (int)m.ss.rows), sa, m.ss.used, m.ss.draws);
        } else if (!m.enc.on) {
            rc = unpack_tokens(st, w.packed, L - 1, B, ids);
        }
        return rc ? rc : post_async_error(st, w.err);
    }
    // ---- the persistent split-precision encode: both layers over the L encode steps and vid_rnn's input-free decode steps; only the
    // 79 token-dependent word_rnn steps stay launches per step
    // vid_rnn's steps [t0, t1) as one persistent launch - beside `partner` (a word_rnn block) or alone on the whole device - and the
    // vid_out half of word_rnn's gate input for them (+ biases); the kernel writes h_t into the GEMM's row image w.ph1 itself (hblk)
    int vid_block(int t0, int t1, const SeqFwdX3Args* partner) {
        int rc;
        SeqFwdX3Args av = persist_fwd_x3_args(t0, t1, B, H, T, w.xkp, w.gx1, L, w.bsum1, kc.xw1, w.xh1, w.h1, w.c1_all, w.psync_a, w.err + 1);
        av.no_stash = 1;
        av.hblk = w.ph1.p; av.ldhblk = w.ph1.ld;
        {
            ProfScope ps(st, K_STEP_FWD, (t1 - t0) + (partner ? partner->t1 - partner->t0 : 0));
            if ((rc = lstm_seq_fwd_x3_persist2(st, av, partner))) return rc;
        }
        return pgemm(la, (t1 - t0) * B, 4 * H, H, w.ph1, t0 * B, 0, kc.wv, 0, 0, w.gx2 + t0 * B4H, 4 * H, ID, w.bsum2, false);
    }
    // The staged encode on the caller's stream; *tv = vid_rnn steps done when it returns (>= L, <= Tend)
    int encode_x3_persistent(int Tend, int* tv) {
        int rc;
        if ((rc = hand(sx, st))) return rc;                     // lane B's weight images before their first use on this stream
        if ((rc = zero_k16_tail(st, w.ph1, H, (size_t)T * B))) return rc;     // (the k16 records of w.ph1 past the last column slice)
        const std::vector<int> be = pipe_bounds(L, L, balanced_block(L, pipe_block()));     // blocks over the L encode steps
        const int nb = (int)be.size() - 1;
        // vid_rnn's blocks: the encode blocks and ONE block of its decode-phase steps (no input, no token) - the partner of word_rnn's
        // last encode block, which used to run alone on half of the device
        std::vector<int> bv(be);
        if (Tend > L) bv.push_back(L + (be[nb] - be[nb - 1]) < Tend ? L + (be[nb] - be[nb - 1]) : Tend);
        const int nbv = (int)bv.size() - 1;
        for (int k = 0; k <= nb; ++k) {          // stage k: vid_rnn block k next to word_rnn block k-1 (as in s2vt_train_forward)
            SeqFwdX3Args aw;
            if (k >= 1) {
                aw = persist_fwd_x3_args(be[k - 1], be[k], B, H, L, w.xkp, w.gx2, L, w.bsum2, kc.xw2, w.xh2, w.h2_all, w.c2_all, w.psync_b, w.err + 1);
                aw.no_stash = 1;
            }
            if (k < nbv) {
                if ((rc = vid_block(bv[k], bv[k + 1], k >= 1 ? &aw : nullptr))) return rc;
            } else {
                ProfScope ps(st, K_STEP_FWD, be[k] - be[k - 1]);
                if ((rc = lstm_seq_fwd_x3_persist2(st, aw, nullptr))) return rc;
            }
        }
        *tv = bv.back();
        return 0;
    }
    // the encode phase was what was asked for: the states after step L - 1
    int hand_out_encode(int tv) {
        int rc;
        const EncodeOut& enc = m.enc;
        const size_t nb_ = (size_t)BH * sizeof(float);
        S2VT_HIP(hipMemcpyAsync(enc.vid_h, w.h1 + (int64_t)(L - 1) * BH, nb_, hipMemcpyDeviceToDevice, st));
        S2VT_HIP(hipMemcpyAsync(enc.vid_c, w.c1_all + (int64_t)(L - 1) * BH, nb_, hipMemcpyDeviceToDevice, st));
        S2VT_HIP(hipMemcpyAsync(enc.word_h, w.h2_all + (int64_t)(L - 1) * BH, nb_, hipMemcpyDeviceToDevice, st));
        S2VT_HIP(hipMemcpyAsync(enc.word_c, w.c2_all + (int64_t)(L - 1) * BH, nb_, hipMemcpyDeviceToDevice, st));
        if (enc.depth > 0) {
            // vid_rnn's decode-phase steps take no input and see no token (S2VTModel.py:208-210 inside the depth loop): the
            // first `depth` of them in one launch, their half of word_rnn's gate input in one GEMM
            if (tv < L + enc.depth && (rc = vid_block(tv, L + enc.depth, nullptr))) return rc;
            S2VT_HIP(hipMemcpyAsync(enc.gx_dec, w.gx2 + (int64_t)L * B4H, (size_t)enc.depth * B4H * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
        return finish();
    }
    // ---- The 79 token-dependent steps behind the persistent encode.
    // Fused schedule (s2vt_set_decode_schedule(1), the default; option "decode_fused" = 0 selects the two-chain schedule below):
    // h_t·W_hh^T of step t+1 does not depend on step t's token - only the per-token rows of the gate table do - so it is computed
    // BESIDE step t's out_linear + argmax, by the same launch: W_hh's 4H rows are 63 more row blocks of the plane-path argmax kernel
    // (188 + 63 workgroups: one wave of the 256 compute units), which write their products to w.zbuf instead of reducing them.  A
    // one-thread-per-cell launch then finishes step t+1 (gates = z + gx + table row of the token, in the fused step's order).  Two
    // launches per step on ONE stream, and the chain is argmax + cell update instead of argmax + recurrent GEMM + cell update.
    int argmax_pair(int t, bool with_logits, bool with_z) {       // logits + argmax of step t (h_t planes) | z of step t+1
        ProfScope ps(st, K_ARGMAX, 1);
        ArgmaxX3Args ax = argmax_x3_args(0, B, w.packed + (int64_t)(with_logits ? t - L : 0) * B);
        if (with_z) { ax.W2 = kc.whh.p; ax.ldw2 = kc.whh.ld; ax.M2 = 4 * H; ax.z = w.zbuf; ax.ldz = 4 * (int64_t)H; }
        ax.v_off = with_logits ? 0 : cdiv(V, 64);
        return logits_argmax_x3(st, ax, with_logits ? gumbel_at(t, 0).ptr() : nullptr);
    }
    int decode_fused() {
        int rc;
        // h_{L-1} of the encode phase as blocked planes, then z(L) alone
        if ((rc = hand(sx, st))) return rc;
        if ((rc = psplit(la, w.ph2, 0, w.h2_all + (int64_t)(L - 1) * BH, H, ID, B, H))) return rc;
        if ((rc = argmax_pair(L, false, true))) return rc;
        for (int t = L; t < T; ++t) {
            StepFwdArgs a = word_step_args(t, nullptr, t == L ? w.c2_all + (int64_t)(L - 1) * BH : w.c2, 0, B);
            a.z_out = w.zbuf; a.ldz = 4 * (int64_t)H;
            {
                ProfScope ps(st, K_STEP_FWD, 1);
                if ((rc = lstm_cell_pointwise(st, a))) return rc;
            }
            if ((rc = argmax_pair(t, true, t + 1 < T))) return rc;
        }
        return finish();
    }
    // Two-chain schedule.  A decode step is two dependent launches (word_rnn step, out_linear + argmax) that each leave part of the
    // chip idle (188 of 256 compute units in the argmax; launch gaps and tails between the two) and batch rows never interact: at
    // B % 128 == 0 the two halves of the batch run as two INDEPENDENT chains on the two streams, so one half's step kernel fills the
    // other half's gaps
    int decode_two_chains() {
        int rc;
        const int nh = (pl.nh == 2 && sx != st) ? 2 : 1;
        if (nh == 2 && (rc = hand(st, sx))) return rc;
        for (int t = L; t < T; ++t)
            for (int hf = 0; hf < nh; ++hf)
                if ((rc = word_step(hf ? sx : st, t, t == L ? w.h2_all + (int64_t)(L - 1) * BH : w.h2 + ((t - 1) & 1) * BH,
                                    t == L ? w.c2_all + (int64_t)(L - 1) * BH : w.c2, hf * (B / nh), B / nh)))
                    return rc;
        if (nh == 2 && (rc = hand(sx, st))) return rc;
        return finish();
    }
    // ---- DEC_PER_STEP: launches per timestep on two lanes, all T steps of both layers in pipeline blocks
    int decode_two_lanes() {
        int rc;
        const std::vector<int> bd = pipe_bounds(T, L, pipe_block());
        for (size_t k = 0; k + 1 < bd.size(); ++k) {
            const int t0 = bd[k], t1 = bd[k + 1];
            {   // lane A: vid_rnn over all T steps (S2VTModel.py:64-67); c updated in place, h kept for the word layer
                ProfScope ps(st, K_STEP_FWD, t1 - t0);
                for (int t = t0; t < t1; ++t) {
                    StepFwdArgs a;
                    memset(&a, 0, sizeof(a));
                    a.B = B; a.H = H;
                    a.h_prev = t ? w.h1 + (t - 1) * BH : nullptr; a.ldh = H;
                    a.w_hh = p->vid_w_hh; a.ldw = H;
                    a.gx = (t < L) ? w.gx1 + t * B4H : nullptr; a.ldgx = 4 * (int64_t)H;
                    a.bias = w.bsum1;
                    a.c_prev = t ? w.c1 : nullptr; a.ldc = H;
                    a.h_out = w.h1 + t * BH; a.ldho = H;
                    a.c_out = w.c1; a.ldco = H;
                    if ((rc = lstm_step_fwd(st, a))) return rc;
                }
            }
            if ((rc = hand(st, sx))) return rc;
            // lane B: vid_out half of the word_rnn gate input for this block (+ biases)
            if (pl.planes) {
                if ((rc = psplit(lb, w.ph1, t0 * B, w.h1 + t0 * BH, H, ID, (t1 - t0) * B, H))) return rc;
                if ((rc = pgemm(lb, (t1 - t0) * B, 4 * H, H, w.ph1, t0 * B, 0, kc.wv, 0, 0, w.gx2 + t0 * B4H, 4 * H, ID, w.bsum2, false))) return rc;
            } else {
                if ((rc = lgemm(lb, true, true, (t1 - t0) * B, 4 * H, H, w.h1 + t0 * BH, H, ID, p->word_w_ih + E, E + H, ID,
                                w.gx2 + t0 * B4H, 4 * H, ID, w.bsum2, false)))
                    return rc;
            }
            for (int t = t0; t < t1; ++t)
                if ((rc = word_step(sx, t, t ? w.h2 + ((t - 1) & 1) * BH : nullptr, t ? w.c2 : nullptr, 0, B))) return rc;
        }
        if ((rc = hand(sx, st))) return rc;
        return finish();
    }
};
static int greedy_decode_core(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, int64_t* ids,
                              void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, bool cache_valid,
                              void* stream, const DecodeModes& m) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && (ids || m.enc.on) && workspace, "s2vt_greedy_decode: null/invalid argument");
    S2VT_REQUIRE(sos_ix >= 0 && sos_ix < d->V, "s2vt_greedy_decode: sos_ix %d outside vocabulary %d", sos_ix, d->V);
    const DecodeWS w = carve_decode(*d, workspace);
    const size_t kbytes = carve_decode_const(*d, nullptr).bytes;
    S2VT_REQUIRE(workspace_bytes >= w.bytes + (cache ? 0 : kbytes), "s2vt_greedy_decode: workspace %zu < %zu bytes", workspace_bytes,
                 w.bytes + (cache ? 0 : kbytes));
    S2VT_REQUIRE(!cache || cache_bytes >= kbytes, "s2vt_greedy_decode_cached: cache %zu < %zu bytes", cache_bytes, kbytes);
    // weight-derived images: in the caller's cache (filled by a call with cache_valid == 0, reused while the weights stand) or
    // behind the per-call part of the workspace (rebuilt by every call)
    const DecodeConst kc = carve_decode_const(*d, cache ? cache : reinterpret_cast<char*>(workspace) + w.bytes);
    const DecodePlan pl = decode_plan(*d, m.enc.on);
    DecodeDriver dr(d, p, feats, sos_ix, ids, w, kc, m, pl, cache != nullptr, cache_valid);
    // (refused BEFORE anything is enqueued: the caller frees the workspace on this error)
    S2VT_REQUIRE(!m.enc.on || dr.px, "s2vt_decode_encode_cached: this shape / mode does not take the persistent split-precision encode phase");
    int rc;
    if ((rc = dr.open_lanes((hipStream_t)stream))) return rc;
    hipStream_t st = dr.st;
    if ((rc = bias_sums(st, p, dr.H, w.bsum1, w.bsum2))) return rc;
    if ((rc = fill_zero(st, w.packed, sizeof(unsigned long long) * (size_t)(dr.L - 1) * dr.B))) return rc;
    if ((rc = fill_zero(st, w.err, 4 * sizeof(int)))) return rc;
    if ((rc = dr.hand(st, dr.sx))) return rc;
    if ((rc = dr.fill_weight_images())) return rc;
    if ((rc = dr.project_features())) return rc;
    if (dr.px) {
        int tv;
        if ((rc = dr.encode_x3_persistent(m.enc.on ? dr.L + m.enc.depth : dr.T, &tv))) return rc;
        if (m.enc.on) return dr.hand_out_encode(tv);
        // the rest of vid_rnn's decode steps (no input: bias only): one launch that may use the whole device
        if (tv < dr.T && (rc = dr.vid_block(tv, dr.T, nullptr))) return rc;
    }
    switch (dr.schedule()) {
        case DEC_FUSED: return dr.decode_fused();
        case DEC_TWO_CHAINS: return dr.decode_two_chains();
        default: return dr.decode_two_lanes();
    }
}
static int greedy_decode_impl(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, int64_t* ids,
                              void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, bool cache_valid,
                              void* stream, const DecodeModes& m) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && (ids || m.enc.on) && workspace, "s2vt_greedy_decode: null/invalid argument");
    if (!decode_plan(*d, m.enc.on, false).padded)
        return greedy_decode_core(d, p, feats, sos_ix, ids, workspace, workspace_bytes, cache, cache_bytes, cache_valid, stream, m);
    const s2vt_dims dp = padded_dims(*d);
    const size_t core = decode_core_bytes(dp);
    const DecodePad s = carve_decode_pad(*d, dp, reinterpret_cast<char*>(workspace) + core);
    S2VT_REQUIRE(workspace_bytes >= core + s.bytes, "s2vt_greedy_decode: workspace %zu < %zu bytes", workspace_bytes, core + s.bytes);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = d->B, Bp = dp.B, L = d->L, F = d->F, H = d->H;
    int rc;
    S2VT_HIP(hipMemcpyAsync(s.feats, feats, B * L * F * sizeof(float), hipMemcpyDeviceToDevice, st));
    if ((rc = fill_zero(st, s.feats + B * L * F, (Bp - B) * L * F * sizeof(float)))) return rc;
    DecodeModes mp = m;
    if (!m.enc.on) {
        if ((rc = greedy_decode_core(&dp, p, s.feats, sos_ix, s.ids, workspace, core, cache, cache_bytes, cache_valid, stream, mp))) return rc;
        if (m.ss.on) return 0;    // (used / draws were written for the caller's rows by the core itself)
        S2VT_HIP(hipMemcpyAsync(ids, s.ids, B * (L - 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    mp.enc = EncodeOut{s.states, s.states + Bp * H, s.states + 2 * Bp * H, s.states + 3 * Bp * H, m.enc.depth > 0 ? s.gx_dec : nullptr, m.enc.depth, true};
    if ((rc = greedy_decode_core(&dp, p, s.feats, sos_ix, nullptr, workspace, core, cache, cache_bytes, cache_valid, stream, mp))) return rc;
    float* outs[4] = {m.enc.vid_h, m.enc.vid_c, m.enc.word_h, m.enc.word_c};
    for (int k = 0; k < 4; ++k)
        S2VT_HIP(hipMemcpyAsync(outs[k], s.states + (size_t)k * Bp * H, B * H * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (m.enc.depth > 0)      // [depth][Bp][4H] -> [depth][B][4H]
        S2VT_HIP(hipMemcpy2DAsync(m.enc.gx_dec, B * 4 * H * sizeof(float), s.gx_dec, Bp * 4 * H * sizeof(float), B * 4 * H * sizeof(float),
                                  (size_t)m.enc.depth, hipMemcpyDeviceToDevice, st));
    return 0;
}
int s2vt_greedy_decode(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, int64_t* ids,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return greedy_decode_impl(d, p, feats, sos_ix, ids, workspace, workspace_bytes, nullptr, 0, false, stream, DecodeModes{});
}
int s2vt_greedy_decode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, int64_t* ids,
                              void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                              void* stream) {
    S2VT_REQUIRE(cache, "s2vt_greedy_decode_cached: null cache");
    return greedy_decode_impl(d, p, feats, sos_ix, ids, workspace, workspace_bytes, cache, cache_bytes, cache_valid != 0, stream, DecodeModes{});
}
// The ENCODE phase of the decode alone (S2VTModel.py:56-60 for mode='beam_search', the same computation as :64-86 of mode='test'):
// feature projection, both layers over the L frames on the plane path, the weight images in the caller's cache (filled here when
// cache_valid == 0 - every image a decode or a beam search of these weights reads).  Out: the four [B, H] states a beam search
// starts from.  Shapes the persistent split-precision recurrence does not take return S2VT_ERR_ARG (the caller keeps its own encoder).
int s2vt_decode_encode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, void* workspace, size_t workspace_bytes,
                              void* cache, size_t cache_bytes, int32_t cache_valid, float* vid_h, float* vid_c, float* word_h,
                              float* word_c, float* gx_dec, int32_t depth, void* stream) {
    S2VT_REQUIRE(cache && vid_h && vid_c && word_h && word_c, "s2vt_decode_encode_cached: null argument");
    S2VT_REQUIRE(!gx_dec || (d && depth > 0 && depth <= d->L - 1), "s2vt_decode_encode_cached: depth must be in [1, L-1]");
    DecodeModes m{};
    m.enc = EncodeOut{vid_h, vid_c, word_h, word_c, gx_dec, gx_dec ? depth : 0, true};
    return greedy_decode_impl(d, p, feats, 0, nullptr, workspace, workspace_bytes, cache, cache_bytes, cache_valid != 0, stream, m);
}
// ------------------------------------------------------------------ sampled decode (mode='sample')
// The greedy drivers with the sampling variants of their arg-max launches: same workspace, same weight-image cache.
// (temperature_ok / gumbel_args: api_internal.h)
static DecodeModes draw_mode_of(float temperature, uint64_t seed, int B, bool on = true) {      // every step of a B-row decode draws
    DecodeModes m{};
    m.smp = Draw{gumbel_args(temperature, seed, 0, 0, (uint32_t)B), on};
    return m;
}
int s2vt_sample_decode(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, float temperature, uint64_t seed,
                       int64_t* ids, void* workspace, size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && ids && workspace, "s2vt_sample_decode: null/invalid argument");
    S2VT_REQUIRE(temperature_ok(temperature), "s2vt_sample_decode: temperature and 1 / temperature must be finite and > 0 (got %g)", (double)temperature);
    return greedy_decode_impl(d, p, feats, sos_ix, ids, workspace, workspace_bytes, nullptr, 0, false, stream, draw_mode_of(temperature, seed, d->B));
}
int s2vt_sample_decode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, int32_t sos_ix, float temperature,
                              uint64_t seed, int64_t* ids, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                              int32_t cache_valid, void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && ids && workspace && cache, "s2vt_sample_decode_cached: null/invalid argument");
    S2VT_REQUIRE(temperature_ok(temperature), "s2vt_sample_decode_cached: temperature and 1 / temperature must be finite and > 0 (got %g)", (double)temperature);
    return greedy_decode_impl(d, p, feats, sos_ix, ids, workspace, workspace_bytes, cache, cache_bytes, cache_valid != 0, stream,
                              draw_mode_of(temperature, seed, d->B));
}

// ------------------------------------------------------------------ scheduled sampling (mode='train', ss_prob > 0)
// The decode drivers once more, each token step fed by the coin: the ground-truth word, or the model's own previous choice.
static int scheduled_decode_impl(const char* who, const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets,
                                 int64_t targets_ld, float ss_prob, int32_t draw_mode, float temperature, uint64_t seed, int64_t* used,
                                 int64_t* draws, void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes,
                                 bool cache_valid, void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && targets && used && workspace, "%s: null/invalid argument", who);
    S2VT_REQUIRE(targets_ld >= d->L - 1, "%s: targets row stride %lld < L - 1 = %d", who, (long long)targets_ld, d->L - 1);
    S2VT_REQUIRE(ss_prob >= 0.f && ss_prob <= 1.f, "%s: ss_prob must be in [0, 1] (got %g)", who, (double)ss_prob);     // (NaN fails both)
    S2VT_REQUIRE(draw_mode == 0 || draw_mode == 1, "%s: draw_mode must be 0 (arg-max) or 1 (sample), got %d", who, (int)draw_mode);
    S2VT_REQUIRE(draw_mode == 0 || temperature_ok(temperature), "%s: temperature and 1 / temperature must be finite and > 0 (got %g)", who,
                 (double)temperature);
    DecodeModes m = draw_mode_of(draw_mode ? temperature : 1.0f, seed, d->B, draw_mode != 0);
    m.ss = SchedArgs{targets, targets_ld, ss_prob, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), (uint32_t)d->B, used, draws, true};
    return greedy_decode_impl(d, p, feats, 0, used, workspace, workspace_bytes, cache, cache_bytes, cache_valid, stream, m);
}
int s2vt_scheduled_decode(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t targets_ld,
                          float ss_prob, int32_t draw_mode, float temperature, uint64_t seed, int64_t* used, int64_t* draws,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return scheduled_decode_impl("s2vt_scheduled_decode", d, p, feats, targets, targets_ld, ss_prob, draw_mode, temperature, seed, used,
                                 draws, workspace, workspace_bytes, nullptr, 0, false, stream);
}
int s2vt_scheduled_decode_cached(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t targets_ld,
                                 float ss_prob, int32_t draw_mode, float temperature, uint64_t seed, int64_t* used, int64_t* draws,
                                 void* workspace, size_t workspace_bytes, void* cache, size_t cache_bytes, int32_t cache_valid,
                                 void* stream) {
    S2VT_REQUIRE(cache, "s2vt_scheduled_decode_cached: null cache");
    return scheduled_decode_impl("s2vt_scheduled_decode_cached", d, p, feats, targets, targets_ld, ss_prob, draw_mode, temperature, seed,
                                 used, draws, workspace, workspace_bytes, cache, cache_bytes, cache_valid != 0, stream);
}
static bool ss_prob_ok(float p) { return p >= 0.f && p <= 1.f; }
static SsArgs ss_args(const int64_t* targets, int64_t ld, float p, uint64_t seed, int32_t step, int32_t row0, int32_t B) {
    return SsArgs{targets, ld, p, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)row0,
                  (uint32_t)row0 + (uint32_t)B};
}
int s2vt_ss_mix(const int64_t* draw_tokens, const int64_t* targets, int64_t targets_ld, int32_t B, float ss_prob, uint64_t seed,
                int32_t step, int32_t row0, int64_t* out, void* stream) {
    S2VT_REQUIRE(draw_tokens && targets && out && B > 0 && step >= 0 && row0 >= 0 && targets_ld > step, "s2vt_ss_mix: null/invalid argument");
    S2VT_REQUIRE(ss_prob_ok(ss_prob), "s2vt_ss_mix: ss_prob must be in [0, 1] (got %g)", (double)ss_prob);
    return ss_mix((hipStream_t)stream, draw_tokens, B, ss_args(targets, targets_ld, ss_prob, seed, step, row0, B), out);
}
int s2vt_ss_unpack(const unsigned long long* packed, int32_t steps, int32_t B, const int64_t* targets, int64_t targets_ld, float ss_prob,
                   uint64_t seed, int64_t* used, int64_t* draws, void* stream) {
    S2VT_REQUIRE(packed && targets && used && steps > 0 && B > 0 && targets_ld >= steps, "s2vt_ss_unpack: null/invalid argument");
    S2VT_REQUIRE(ss_prob_ok(ss_prob), "s2vt_ss_unpack: ss_prob must be in [0, 1] (got %g)", (double)ss_prob);
    return unpack_scheduled((hipStream_t)stream, packed, steps, B, B, ss_args(targets, targets_ld, ss_prob, seed, 0, 0, B), used, draws);
}

static int decode_step_argmax_impl(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out,
                                   unsigned long long* packed, void* stream, const GumbelArgs* smp) {
    LogitsArgmaxArgs la = logits_argmax_args(B, H, V, h, w_out, b_out, packed);
#ifdef S2VT_EXPERIMENT_STAMPS
    la.stamps = g_xstamps;
#endif
    ProfScope ps((hipStream_t)stream, K_ARGMAX, 1);
    return logits_argmax((hipStream_t)stream, la, smp);
}
int s2vt_decode_step_sample(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out, float temperature,
                            uint64_t seed, int32_t step, int32_t row0, unsigned long long* packed, void* stream) {
    S2VT_REQUIRE(B > 0 && H > 0 && V > 0 && h && w_out && packed && step >= 0 && row0 >= 0, "s2vt_decode_step_sample: bad arguments");
    S2VT_REQUIRE(temperature_ok(temperature), "s2vt_decode_step_sample: temperature and 1 / temperature must be finite and > 0 (got %g)", (double)temperature);
    const GumbelArgs g = gumbel_args(temperature, seed, (uint32_t)step, (uint32_t)row0, (uint32_t)row0 + (uint32_t)B);
    return decode_step_argmax_impl(B, H, V, h, w_out, b_out, packed, stream, &g);
}
int s2vt_decode_step_argmax(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out,
                            unsigned long long* packed, void* stream) {
    return decode_step_argmax_impl(B, H, V, h, w_out, b_out, packed, stream, nullptr);
}

// The same decode step on the bf16 matrix cores (argmax_x3.hip): both operands are split into blocked 3-plane images in the
// caller's workspace first (inside s2vt_greedy_decode W_o is split once per call, h_t once per step).
static size_t argmax_x3_ws_bytes(int B, int H, int V) {
    const size_t kp = (size_t)pad64(H);
    return (rows64((size_t)V) + rows64((size_t)B)) * 3 * kp * sizeof(unsigned short) + 512;
}
size_t s2vt_decode_step_argmax_x3_workspace_bytes(int32_t B, int32_t H, int32_t V) {
    return (B > 0 && H > 0 && V > 0) ? argmax_x3_ws_bytes(B, H, V) : 0;
}
static int decode_step_argmax_x3_impl(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out,
                                      unsigned long long* packed, void* workspace, size_t workspace_bytes, void* stream,
                                      const GumbelArgs* smp) {
    hipStream_t st = (hipStream_t)stream;
    Carver c{reinterpret_cast<char*>(workspace), 0, 0};
    const PB wp = take_planes(c, V, H, 3), hp = take_planes(c, B, H, 3);
    int rc;
    if ((rc = split_planes(st, 3, false, w_out, H, ID, V, H, wp.p, wp.ld, wp.kpad, (int)rows64((size_t)V)))) return rc;
    if ((rc = split_planes(st, 3, false, h, H, ID, B, H, hp.p, hp.ld, hp.kpad, (int)rows64((size_t)B)))) return rc;
    ArgmaxX3Args ax = argmax_x3_args(B, V, wp, hp.p, hp.ld, b_out, packed);
#ifdef S2VT_EXPERIMENT_STAMPS
    ax.stamps = g_xstamps;
#endif
    ProfScope ps(st, K_ARGMAX, 1);
    return logits_argmax_x3(st, ax, smp);
}
int s2vt_decode_step_argmax_x3(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out,
                               unsigned long long* packed, void* workspace, size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(B > 0 && H > 0 && V > 0 && h && w_out && packed && workspace, "s2vt_decode_step_argmax_x3: bad arguments");
    S2VT_REQUIRE(workspace_bytes >= argmax_x3_ws_bytes(B, H, V), "s2vt_decode_step_argmax_x3: workspace too small");
    return decode_step_argmax_x3_impl(B, H, V, h, w_out, b_out, packed, workspace, workspace_bytes, stream, nullptr);
}
size_t s2vt_decode_step_sample_x3_workspace_bytes(int32_t B, int32_t H, int32_t V) {
    return s2vt_decode_step_argmax_x3_workspace_bytes(B, H, V);
}
int s2vt_decode_step_sample_x3(int32_t B, int32_t H, int32_t V, const float* h, const float* w_out, const float* b_out, float temperature,
                               uint64_t seed, int32_t step, int32_t row0, unsigned long long* packed, void* workspace,
                               size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(B > 0 && H > 0 && V > 0 && h && w_out && packed && workspace && step >= 0 && row0 >= 0,
                 "s2vt_decode_step_sample_x3: bad arguments");
    S2VT_REQUIRE(temperature_ok(temperature), "s2vt_decode_step_sample_x3: temperature and 1 / temperature must be finite and > 0 (got %g)", (double)temperature);
    S2VT_REQUIRE(workspace_bytes >= argmax_x3_ws_bytes(B, H, V), "s2vt_decode_step_sample_x3: workspace too small");
    const GumbelArgs g = gumbel_args(temperature, seed, (uint32_t)step, (uint32_t)row0, (uint32_t)row0 + (uint32_t)B);
    return decode_step_argmax_x3_impl(B, H, V, h, w_out, b_out, packed, workspace, workspace_bytes, stream, &g);
}
}
