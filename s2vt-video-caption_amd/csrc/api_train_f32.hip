// The fp32-MFMA train driver: launches per timestep, fp32 operands read in place, two lanes.  ONE driver (TrainF32) for
//   plain    s2vt_train_forward / s2vt_train_backward in gemm mode 0 and at batches the plane drivers do not take (api_train.hip
//            carves the workspace and calls train_forward_f32 / train_backward_f32), and
//   grouped  s2vt_train_group_forward / s2vt_train_group_backward: mode='train' on K captions per clip with ONE encode per clip.
// The grouped logits and gradients are those of the plain driver on the clips repeated K times (row r = b * K + k), computed
// without the repeats: the feature projection, all 2L-1 steps of vid_rnn and the first L steps of word_rnn do not depend on the
// caption and run on B rows in both directions; only word_rnn's L-1 decode steps, out_linear and the embedding run on R = B * K
// rows.  The gradients that arrive at the shared part - the decode steps' dG2 and the cell gradient carried across the encode /
// decode boundary - are summed over a clip's K rows in a fixed order (group.hip); every consumer behind them is linear in them.
// The two paths differ in ONE place, where word_rnn's decode steps live (DecodeSteps), and in which half of the decode steps'
// gate input brings the biases; every grouped-only step is an `if (K)` at that seam.
#include "api_internal.h"

namespace s2vt {

// The grouped workspace.  Time-major images; the B-row ones as TrainWS's, except that word_rnn's own end after the L frames:
//   s2  [T*B][4H]  word_rnn's gates of the L frames; rows >= L*B: vid_rnn's half of the decode steps' gate input (+ biases) in the
//                  forward, the group-summed dG2 in the backward
//   h2, c2  [L*B][H]
// The decode images have L row blocks of R rows: block 0 of h2d / c2d is word_rnn's state after the L frames handed to the clip's
// K rows, block j >= 1 is decode step j-1 (timestep L-1+j), so that seq_fwd / seq_bwd run over them as over a layer of L steps
// whose step 0 is given (block 0 of s2d is not used).
struct GroupWS : TrainBufs {
    float *s2d, *h2d, *c2d;                      // [L*R][4H], [L*R][H], [L*R][H]
    float* hm;                                   // [(L-1)*R][H] out_drop mask (.) h2d (dropout only; kept for the backward)
    float* dcr;                                  // [R][H] cell gradient carried through the decode steps
    size_t bytes;
};

// what the GEMM wrappers, the column sums (64-row chunks on grid.y) and the int row indices of the kernels can address
static bool group_shape_ok(const s2vt_dims* d, int K) {
    if (!dims_ok(d) || K < 1) return false;
    const int64_t R = (int64_t)d->B * K, rows_d = (int64_t)d->L * R, rows_e = (2 * (int64_t)d->L - 1) * d->B;
    const int64_t wide = std::max<int64_t>(std::max<int64_t>(4 * (int64_t)d->H, d->V), std::max<int64_t>(d->F, d->E));
    const int64_t max_rows = 64 * (int64_t)65535;
    return R < (1ll << 24) && rows_d <= max_rows && rows_e <= max_rows && 4 * (int64_t)d->H < (1ll << 31) &&
           rows_d * wide < (1ll << 40) && rows_e * wide < (1ll << 40);
}

static GroupWS carve_group(const s2vt_dims& d, int K, void* base) {
    const size_t B = d.B, L = d.L, H = d.H, E = d.E, V = d.V, T = 2 * L - 1, R = B * (size_t)K, S = L - 1;
    Carver c{reinterpret_cast<char*>(base), 0, 0};
    GroupWS w;
    w.bsum1 = c.take<float>(4 * H);
    w.bsum2 = c.take<float>(4 * H);
    w.x1 = c.take<float>(L * B * H);
    w.s1 = c.take<float>(T * B * 4 * H);
    w.h1 = c.take<float>(T * B * H);
    w.c1 = c.take<float>(T * B * H);
    w.s2 = c.take<float>(T * B * 4 * H);
    w.h2 = c.take<float>(L * B * H);
    w.c2 = c.take<float>(L * B * H);
    w.s2d = c.take<float>(L * R * 4 * H);
    w.h2d = c.take<float>(L * R * H);
    w.c2d = c.take<float>(L * R * H);
    w.hm = c.take<float>(S * R * H);
    w.tok = c.take<int32_t>(S * R);
    w.embws = c.take<int>(embedding_grad_ws_ints((int64_t)(S * R), (int)d.V));
    w.err = c.take<int>(4);
    // backward-only scratch
    w.wt1 = c.take<float>(H * 4 * H);
    w.wt2 = c.take<float>(H * 4 * H);
    w.dh1 = c.take<float>(T * B * H);
    w.dh2dec = c.take<float>(S * R * H);
    w.dx1 = c.take<float>(L * B * H);
    w.de = c.take<float>(S * R * E);
    w.dc1 = c.take<float>(B * H);
    w.dc2 = c.take<float>(B * H);
    w.dcr = c.take<float>(R * H);
    const size_t cs = std::max(std::max(colsum_partial_floats((int64_t)(T * B), (int)(4 * H)), colsum_partial_floats((int64_t)(S * R), (int)V)),
                               colsum_partial_floats((int64_t)(L * B), (int)H));
    w.colsum_a = c.take<float>(cs);
    w.colsum_b = c.take<float>(cs);
    s2vt_dims dr = d;                            // split-K slabs sized for the R-row GEMMs
    dr.B = (int32_t)std::min<size_t>(R, (size_t)1 << 20);
    w.gws_floats = gemm_ws_floats(dr);
    w.gws_a = c.take<float>(w.gws_floats);
    w.gws_b = c.take<float>(w.gws_floats);
    w.bytes = align_up(c.off, 256);
    return w;
}

// Where word_rnn's decode steps (timesteps >= L) live: timestep L + j is row block at_L + j of images of n blocks of R rows
// (n: what seq_fwd takes as n_gx and seq_bwd as T).  Plain: the layer's own B-row images.  Grouped: the R-row decode images.
struct DecodeSteps {
    int R;
    float *s, *h, *c;
    int n, at_L;
    float* dc;               // cell gradient carried through the decode steps' BPTT
    float* hm;               // the forward's masked decode-step hidden states (dropout only)
};
static DecodeSteps plain_steps(const s2vt_dims& d, const TrainBufs& w) {
    return DecodeSteps{d.B, w.s2, w.h2, w.c2, 2 * d.L - 1, d.L, w.dc2, w.dh2dec};      // (dh2dec: free in the forward)
}
static DecodeSteps group_steps(const s2vt_dims& d, int K, const GroupWS& w) {
    return DecodeSteps{d.B * K, w.s2d, w.h2d, w.c2d, d.L, 1, w.dcr, w.hm};
}

// Lives on the stack of one forward or backward call.  K == 0: plain; K >= 1: grouped, K caption rows per clip.
struct TrainF32 : Lanes {
    const s2vt_dims& d; const s2vt_params* p; const s2vt_grads* g; const TrainBufs& w; const DecodeSteps v;
    const int K; const float* out_mask;
    const int B, L, F, H, E, V, T, S, R;      // S decode steps of R rows
    const int64_t BH, B4H, RH, R4H, SR;
    float *const dec_s, *const dec_h;         // the decode steps' gate image and hidden states from timestep L on: [S*R][4H], [S*R][H]
    const std::vector<int> bd;
    TrainF32(const s2vt_dims& d_, int K_, const s2vt_params* p_, const s2vt_grads* g_, const TrainBufs& w_, const DecodeSteps& v_,
             const float* out_mask_)
        : d(d_), p(p_), g(g_), w(w_), v(v_), K(K_), out_mask(out_mask_), B(d_.B), L(d_.L), F(d_.F), H(d_.H), E(d_.E), V(d_.V),
          T(2 * d_.L - 1), S(d_.L - 1), R(v_.R), BH((int64_t)B * H), B4H(4 * BH), RH((int64_t)R * H), R4H(4 * RH), SR((int64_t)S * R),
          dec_s(v_.s + v_.at_L * R4H), dec_h(v_.h + v_.at_L * RH), bd(pipe_bounds(T, L, pipe_block())) {}

    // targets: plain [B][L-1] with row stride stride_b; grouped [B][K][L-1] with strides stride_b, stride_k
    int forward(hipStream_t caller, const float* feats, const int64_t* targets, int64_t stride_b, int64_t stride_k, float* logits) {
        int rc;
        if ((rc = open(caller, w.gws_a, w.gws_b, w.gws_floats, w.colsum_a, w.colsum_b))) return rc;
        // la: vid_rnn lane (caller's stream), lb: word_rnn lane
        if ((rc = bias_sums(st, p, H, w.bsum1, w.bsum2))) return rc;
        if ((rc = fill_zero(st, w.err, 4 * sizeof(int)))) return rc;
        if ((rc = K ? group_tokens(st, targets, stride_b, stride_k, B, K, S, V, w.tok, w.err)
                    : targets_to_time_major(st, targets, B, S, stride_b, V, w.tok, w.err)))
            return rc;
        if ((rc = hand(st, sx))) return rc;
        // lane B, independent of vid_rnn: embedded-word half of the decode steps' gate input, R rows per step.  Plain: with both
        // biases; grouped: the biases come with the clip's half below                  S2VTModel.py:71-75
        if ((rc = lgemm(lb, true, true, S * R, 4 * H, E, p->emb_w, E, gather(w.tok), p->word_w_ih, E + H, ID, dec_s, 4 * H, ID,
                        K ? nullptr : w.bsum2, false)))
            return rc;
        if ((rc = project_features_f32(la, d, p, feats, w.x1, w.s1, w.bsum1))) return rc;
        for (size_t k = 0; k + 1 < bd.size(); ++k) {
            const int t0 = bd[k], t1 = bd[k + 1];
            if ((rc = seq_fwd(st, t0, t1, B, H, w.s1, L, w.bsum1, p->vid_w_hh, w.h1, w.c1, true))) return rc;
            if ((rc = hand(st, sx))) return rc;
            // vid_out half of word_rnn's gate input for this block (+ both biases), B rows.  Plain: rows >= L accumulate onto the
            // embedded-word half, which has the biases                                 S2VTModel.py:75-77
            const bool onto = !K && t0 >= L;
            if ((rc = lgemm(lb, true, true, (t1 - t0) * B, 4 * H, H, w.h1 + t0 * BH, H, ID, p->word_w_ih + E, E + H, ID, w.s2 + t0 * B4H, 4 * H,
                            ID, onto ? nullptr : w.bsum2, onto)))
                return rc;
            if (t1 <= L) {
                if ((rc = seq_fwd(sx, t0, t1, B, H, w.s2, T, w.bsum2, p->word_w_hh, w.h2, w.c2, true))) return rc;
                continue;
            }
            // decode steps [t0, t1) = row blocks [j0, j1) - beside vid_rnn's next block.  Grouped: first the clip's state after the L
            // frames (once) and its half of the gate input handed to its K caption rows
            const int j0 = t0 - L + v.at_L, j1 = t1 - L + v.at_L;
            if (K) {
                if (t0 == L) {
                    if ((rc = group_expand_rows(sx, w.h2 + (L - 1) * BH, H, v.h, H, B, K, H, false))) return rc;
                    if ((rc = group_expand_rows(sx, w.c2 + (L - 1) * BH, H, v.c, H, B, K, H, false))) return rc;
                }
                if ((rc = group_expand_rows(sx, w.s2 + t0 * B4H, 4 * H, v.s + j0 * R4H, 4 * H, (int64_t)(t1 - t0) * B, K, 4 * H, true))) return rc;
            }
            if ((rc = seq_fwd(sx, j0, j1, R, H, v.s, v.n, w.bsum2, p->word_w_hh, v.h, v.c, true))) return rc;
        }
        // logits[r, j, :] = (out_drop mask (.)) h2[L + j][r]·W_o^T + b_o                S2VTModel.py:78-80
        const float* hdec = dec_h;
        if (out_mask) {
            if ((rc = mul_vectors(sx, hdec, out_mask, v.hm, SR * H))) return rc;
            hdec = v.hm;
        }
        if ((rc = lgemm(lb, true, true, S * R, V, H, hdec, H, ID, p->out_w, H, ID, logits, V, perm(R, S), p->out_b, false))) return rc;
        return hand(sx, st);
    }

    int backward(hipStream_t caller, const float* feats, const float* dlogits, float* dfeats) {
        int rc;
        if ((rc = open(caller, w.gws_a, w.gws_b, w.gws_floats, w.colsum_a, w.colsum_b))) return rc;
        // la: word_rnn lane (caller's stream), lb: vid_rnn lane
        LaneDelayScope delay(st);
        if ((rc = hand(st, sx))) return rc;
        // lane A: gradient into the decode-step hidden states                          (autograd of S2VTModel.py:80, :79)
        if ((rc = lgemm(la, true, false, S * R, H, V, dlogits, V, ID, p->out_w, H, ID, w.dh2dec, H, perm(S, R), nullptr, false))) return rc;
        if (out_mask && (rc = mul_vectors(st, w.dh2dec, out_mask, w.dh2dec, SR * H))) return rc;
        if ((rc = transpose_f32(st, p->word_w_hh, 4 * H, H, w.wt2))) return rc;
        // lane B meanwhile: out_linear weight/bias gradients (need only dlogits and the (masked) decode-step hidden states) and
        // W_hh1^T.  The masked states: grouped kept the forward's; plain makes them again (dx1: free until the vid_rnn input gradient)
        const float* hdec = dec_h;
        if (out_mask) {
            if (!K && (rc = mul_vectors(sx, hdec, out_mask, w.dx1, SR * H))) return rc;
            hdec = K ? v.hm : w.dx1;
        }
        if ((rc = lgemm(lb, false, false, V, H, S * R, dlogits, V, ID, hdec, H, perm(S, R), g->out_w, H, ID, nullptr, false))) return rc;
        if ((rc = colsum_f32(sx, dlogits, SR, V, V, lb.colsum, g->out_b, false))) return rc;
        if ((rc = grads_ready(0, sx))) return rc;
        if ((rc = transpose_f32(sx, p->vid_w_hh, 4 * H, H, w.wt1))) return rc;
        // word_rnn's BPTT beside vid_rnn's of the block before.  Grouped: the decode steps run on the R rows, then what arrives at the
        // shared part is summed over each clip's K rows - the block's dG2 into the B-row image (rows [L*B, T*B) of s2) and, behind
        // the first decode step, the carried cell gradient into dc2.  Everything behind the sums is linear in them and runs on B
        // rows: the recurrent term of step L-1 (dg_next = row block L of s2), dh1, vid_rnn's BPTT, dW_v, the bias sums.
        for (size_t k = bd.size() - 1; k >= 1; --k) {
            const int t0 = bd[k - 1], t1 = bd[k];
            if (t0 >= L) {
                const int j0 = t0 - L + v.at_L, j1 = t1 - L + v.at_L;
                if ((rc = seq_bwd(st, v.n, j0, j1, R, H, w.wt2, w.dh2dec, v.at_L, v.c, v.s, v.dc))) return rc;
                if (K) {
                    if ((rc = group_sum_rows(st, v.s + j0 * R4H, 4 * H, w.s2 + t0 * B4H, 4 * H, (int64_t)(t1 - t0) * B, K, 4 * H))) return rc;
                    if (t0 == L && (rc = group_sum_rows(st, v.dc, H, w.dc2, H, B, K, H))) return rc;
                }
            } else if ((rc = seq_bwd(st, T, t0, t1, B, H, w.wt2, nullptr, 0, w.c2, w.s2, w.dc2))) {
                return rc;
            }
            // gradient into vid_out for this block: dh1 = dG2·W_v                      (autograd of :75)
            if ((rc = lgemm(la, true, false, (t1 - t0) * B, H, 4 * H, w.s2 + t0 * B4H, 4 * H, ID, p->word_w_ih + E, E + H, ID, w.dh1 + t0 * BH, H,
                            ID, nullptr, false)))
                return rc;
            if ((rc = hand(st, sx))) return rc;
            if ((rc = seq_bwd(sx, T, t0, t1, B, H, w.wt1, w.dh1, 0, w.c1, w.s1, w.dc1))) return rc;   // (autograd of :67)
        }
        // lane A: word_rnn parameter gradients + embedding gradient (run while lane B finishes the vid_rnn BPTT).
        // dW_hh2 = dG2[t]^T·h2[t-1].  Plain: t = 1..T-1 in the layer's images.  Grouped: t = 1..L on the B rows (row block L is the
        // summed dG2 of the first decode step against h2[L-1]), t > L on the R rows
        if ((rc = lgemm(la, false, false, 4 * H, H, (K ? L : T - 1) * B, w.s2 + B4H, 4 * H, ID, w.h2, H, ID, g->word_w_hh, H, ID, nullptr, false)))
            return rc;
        if (K && S >= 2 && (rc = lgemm(la, false, false, 4 * H, H, (S - 1) * R, dec_s + R4H, 4 * H, ID, dec_h, H, ID, g->word_w_hh, H, ID, nullptr,
                                       true)))
            return rc;
        if ((rc = lgemm(la, false, false, 4 * H, H, T * B, w.s2, 4 * H, ID, w.h1, H, ID, g->word_w_ih + E, E + H, ID, nullptr, false))) return rc;
        // dW_ih2[:, :E] = dG2dec^T · Emb[tok]: the embedded rows gathered (time-major) into w.de, which is free until the d(embedded
        // words) GEMM below overwrites it                                              (gather_rows_f32: at most 65535 rows per launch)
        for (int64_t r0 = 0; r0 < SR; r0 += 65535)
            if ((rc = gather_rows_f32(st, p->emb_w, E, w.tok + r0, std::min<int64_t>(65535, SR - r0), E, w.de + r0 * E))) return rc;
        if ((rc = lgemm(la, false, false, 4 * H, E, S * R, dec_s, 4 * H, ID, w.de, E, ID, g->word_w_ih, E + H, ID, nullptr, false))) return rc;
        if ((rc = colsum_f32(st, w.s2, (int64_t)T * B, 4 * H, 4 * H, la.colsum, g->word_b_ih, false))) return rc;
        S2VT_HIP(hipMemcpyAsync(g->word_b_hh, g->word_b_ih, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, st));
        if ((rc = lgemm(la, true, false, S * R, E, 4 * H, dec_s, 4 * H, ID, p->word_w_ih, E + H, ID, w.de, E, ID, nullptr, false))) return rc;
        if ((rc = embedding_grad(st, w.de, SR, E, w.tok, V, g->emb_w, w.embws))) return rc;
        if ((rc = grads_ready(1, st))) return rc;
        // lane B: vid_rnn and feat_linear parameter gradients, B rows                  (autograd of :67, :54)
        if ((rc = lgemm(lb, false, false, 4 * H, H, (T - 1) * B, w.s1 + B4H, 4 * H, ID, w.h1, H, ID, g->vid_w_hh, H, ID, nullptr, false))) return rc;
        if ((rc = lgemm(lb, false, false, 4 * H, H, L * B, w.s1, 4 * H, ID, w.x1, H, ID, g->vid_w_ih, H, ID, nullptr, false))) return rc;
        if ((rc = colsum_f32(sx, w.s1, (int64_t)T * B, 4 * H, 4 * H, lb.colsum, g->vid_b_ih, false))) return rc;
        S2VT_HIP(hipMemcpyAsync(g->vid_b_hh, g->vid_b_ih, sizeof(float) * 4 * H, hipMemcpyDeviceToDevice, sx));
        if ((rc = lgemm(lb, true, false, L * B, H, 4 * H, w.s1, 4 * H, ID, p->vid_w_ih, H, ID, w.dx1, H, ID, nullptr, false))) return rc;
        if ((rc = lgemm(lb, false, false, H, F, L * B, w.dx1, H, ID, feats, F, perm(B, L), g->feat_w, F, ID, nullptr, false))) return rc;
        if ((rc = colsum_f32(sx, w.dx1, (int64_t)L * B, H, H, lb.colsum, g->feat_b, false))) return rc;
        // dfeats [B, L, F] (grouped: the gradient of the clip's one row = the sum over its K repeats)
        if (dfeats && (rc = lgemm(lb, true, false, L * B, F, H, w.dx1, H, ID, p->feat_w, F, ID, dfeats, F, perm(B, L), nullptr, false))) return rc;
        return hand(sx, st);
    }
};

int train_forward_f32(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t targets_ld,
                      float* logits, const TrainBufs& w, hipStream_t st, const float* out_mask) {
    return TrainF32(*d, 0, p, nullptr, w, plain_steps(*d, w), out_mask).forward(st, feats, targets, targets_ld, 0, logits);
}
int train_backward_f32(const s2vt_dims* d, const s2vt_params* p, const float* feats, const float* dlogits, const s2vt_grads* g,
                       float* dfeats, const TrainBufs& w, hipStream_t st, const float* out_mask) {
    return TrainF32(*d, 0, p, g, w, plain_steps(*d, w), out_mask).backward(st, feats, dlogits, dfeats);
}

// What a grouped forward left in its workspace: the backward takes K from here and refuses a workspace no forward filled, other
// dims, or a second run on one forward (the activations are consumed in place).
struct GroupRecord { s2vt_dims d; int K; bool masked; };
static RecordTable<GroupRecord> g_group_records;
static int take_group_record(const void* ws, const s2vt_dims& d, bool masked, int* K) {
    GroupRecord r;
    S2VT_REQUIRE(g_group_records.take(ws, &r), "s2vt_train_group_backward: no s2vt_train_group_forward has run on this workspace (or its "
                                               "backward has run already: the saved activations are consumed in place)");
    S2VT_REQUIRE(memcmp(&r.d, &d, sizeof(d)) == 0, "s2vt_train_group_backward: dims differ from the forward that filled this workspace");
    S2VT_REQUIRE(r.masked == masked, "s2vt_train_group_backward: the forward ran %s an out_drop mask, the backward is called %s one",
                 r.masked ? "with" : "without", masked ? "with" : "without");
    *K = r.K;
    return 0;
}

}  // namespace s2vt

using namespace s2vt;

extern "C" {

size_t s2vt_train_group_workspace_bytes(const s2vt_dims* d, int32_t K) {
    return group_shape_ok(d, K) ? carve_group(*d, K, nullptr).bytes : 0;
}

int s2vt_train_group_forward(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t stride_b,
                             int64_t stride_k, int32_t K, const float* out_mask, float* logits, void* workspace, size_t workspace_bytes,
                             void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && targets && logits && workspace, "s2vt_train_group_forward: null/invalid argument");
    S2VT_REQUIRE(K >= 1, "s2vt_train_group_forward: K = %d captions per clip (need K >= 1)", (int)K);
    S2VT_REQUIRE(group_shape_ok(d, K), "s2vt_train_group_forward: B = %d, K = %d, L = %d, H = %d, V = %d: the row or element counts of "
                                       "the (L-1)*B*K-row images overflow what the GEMMs and column sums index",
                 d->B, (int)K, d->L, d->H, d->V);
    S2VT_REQUIRE(stride_b >= 0 && stride_k >= 0, "s2vt_train_group_forward: negative target stride");
    const GroupWS w = carve_group(*d, K, workspace);
    S2VT_REQUIRE(workspace_bytes >= w.bytes, "s2vt_train_group_forward: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    int rc = poll_async_error(false);        // a device-side error of the previous forward, if its flags have arrived
    if (rc) return rc;
    g_group_records.put(workspace, GroupRecord{*d, K, out_mask != nullptr});
    rc = TrainF32(*d, K, p, nullptr, w, group_steps(*d, K, w), out_mask).forward(st, feats, targets, stride_b, stride_k, logits);
    return rc ? rc : post_async_error(st, w.err);
}

int s2vt_train_group_backward(const s2vt_dims* d, const s2vt_params* p, const float* feats, const float* dlogits, const float* out_mask,
                              const s2vt_grads* g, float* dfeats, void* workspace, size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(dims_ok(d) && p && feats && dlogits && g && workspace, "s2vt_train_group_backward: null/invalid argument");
    BackwardScope scope;
    int rc = poll_async_error(false);        // flags of the forward, if they have arrived already
    int K = 0;
    if (rc || (rc = take_group_record(workspace, *d, out_mask != nullptr, &K))) return rc;
    const GroupWS w = carve_group(*d, K, workspace);
    S2VT_REQUIRE(workspace_bytes >= w.bytes, "s2vt_train_group_backward: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    return TrainF32(*d, K, p, g, w, group_steps(*d, K, w), out_mask).backward((hipStream_t)stream, feats, dlogits, dfeats);
}

int s2vt_group_sum_rows(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t groups, int32_t K, int32_t cols, void* stream) {
    S2VT_REQUIRE(in && out && groups > 0 && K >= 1 && cols > 0 && ld_in >= cols && ld_out >= cols && groups <= (1ll << 40) / K / cols,
                 "s2vt_group_sum_rows: null argument or bad geometry (groups=%lld K=%d cols=%d ld_in=%lld ld_out=%lld)", (long long)groups,
                 (int)K, (int)cols, (long long)ld_in, (long long)ld_out);
    // the output must not overlap the input (a thread reads K rows and writes another thread's inputs otherwise)
    const float *in_end = in + (groups * K - 1) * ld_in + cols, *out_end = out + (groups - 1) * ld_out + cols;
    S2VT_REQUIRE(out_end <= in || in_end <= out, "s2vt_group_sum_rows: the output overlaps the input");
    return group_sum_rows((hipStream_t)stream, in, ld_in, out, ld_out, groups, K, cols);
}

}
