// Chain entry points of a stacked LSTM (S2VT with num_layers > 1): the layer wavefront of lstm_stack.hip driven diagonal by
// diagonal from the host, the way s2vt_lstm_seq_fwd / _bwd loop their timesteps.  The model-level composition (projections,
// autograd, greedy loop, dropout masks) is stack_functional.py's.
#include "api_internal.h"

using namespace s2vt;

static int check_chain(const char* who, int32_t T, int32_t B, int32_t H, int32_t n, const s2vt_lstm_layer* L, bool bwd) {
    S2VT_REQUIRE(T > 0 && B > 0 && H > 0 && n > 0 && L && (int64_t)T * B * 4 * H < ((int64_t)1 << 40), "%s: null/invalid argument", who);
    for (int j = 0; j < n; ++j) {
        const s2vt_lstm_layer& l = L[j];
        S2VT_REQUIRE(l.w_hh && l.bias && l.h && l.c, "%s: layer %d needs w_hh, bias, h and c", who, j);
        S2VT_REQUIRE(l.n_gx >= 0 && l.gx_t0 >= 0 && (int64_t)l.gx_t0 + l.n_gx <= T && (l.n_gx == 0 || l.gx),
                     "%s: layer %d: gate-input range [%d, %d) outside [0, %d) or gx missing", who, j, (int)l.gx_t0,
                     (int)(l.gx_t0 + l.n_gx), (int)T);
        S2VT_REQUIRE(j == 0 || !l.x_in, "%s: layer %d: only layer 0 takes an external input (x_in)", who, j);
        const bool dense = j > 0 || l.x_in;
        S2VT_REQUIRE(!dense || (l.w_in && l.ldw_in >= H), "%s: layer %d: its input needs w_in with ldw_in >= H", who, j);
        S2VT_REQUIRE(dense || !l.w_in, "%s: layer 0 has w_in but no x_in", who);
        S2VT_REQUIRE(!l.mask || l.hm, "%s: layer %d: a mask needs the hm output", who, j);
        S2VT_REQUIRE(!l.emb || (T == 1 && l.w_e && l.E > 0 && l.V > 0 && l.ldw_e >= l.E),
                     "%s: layer %d: the token segment needs T = 1, w_e, E, V and ldw_e >= E", who, j);
        S2VT_REQUIRE(!l.ss_targets || (l.emb && l.ss_prob >= 0.f && l.ss_prob <= 1.f && l.ss_step >= 0 && l.ss_row0 >= 0 &&
                                       l.ss_ld > l.ss_step && (l.tok_packed || l.ss_step == 0)),
                     "%s: layer %d: scheduled sampling needs the token segment, ss_prob in [0, 1], a step inside the targets' rows and "
                     "tok_packed after step 0", who, j);
        S2VT_REQUIRE(!l.emb || l.tok_packed || l.ss_targets || (l.tok_const >= 0 && l.tok_const < l.V),
                     "%s: layer %d: token id %d outside [0, %d)", who, j, (int)l.tok_const, (int)l.V);
        if (bwd) {
            S2VT_REQUIRE(l.stash && l.dg, "%s: layer %d needs stash and dg", who, j);
            S2VT_REQUIRE(l.dh_t0 >= 0 && l.dh_t0 <= T, "%s: layer %d: dh_t0 %d outside [0, %d]", who, j, (int)l.dh_t0, (int)T);
            S2VT_REQUIRE(!l.emb && !l.x_in, "%s: layer %d: no backward through the token segment or an external input", who, j);
        }
    }
    return 0;
}

extern "C" {

int s2vt_lstm_chain_fwd(int32_t T, int32_t B, int32_t H, int32_t n, const s2vt_lstm_layer* layers, void* stream) {
    int rc;
    if ((rc = check_chain("s2vt_lstm_chain_fwd", T, B, H, n, layers, false))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t BH = (int64_t)B * H, B4H = 4 * BH;
    // a scheduled-sampling token segment reads the caller's ground-truth ids: a bad one is posted on the ring of the
    // asynchronous-error table (as s2vt_gru_step_fwd_token does for a caller's int32 ids), so a loop of steps never waits
    PostedFlags flags;
    bool posts = false;
    for (int j = 0; j < n; ++j) posts = posts || (layers[j].emb && layers[j].ss_targets);
    if (posts && (rc = flags.open(st))) return rc;
    for (int d = 0; d < T + n - 1; ++d) {
        ChainFwdLaunch a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.H = H;
        for (int j = std::max(0, d - T + 1); j <= std::min(d, n - 1); ++j) {
            const int t = d - j;
            const s2vt_lstm_layer& l = layers[j];
            ChainFwdStep& s = a.s[a.n++];
            s.gx = (t >= l.gx_t0 && t < l.gx_t0 + l.n_gx) ? l.gx + (t - l.gx_t0) * B4H : nullptr;
            s.bias = l.bias;
            s.h_prev = t ? l.h + (t - 1) * BH : l.h0;
            s.c_prev = t ? l.c + (t - 1) * BH : l.c0;
            s.w_hh = l.w_hh;
            if (j > 0) {
                const s2vt_lstm_layer& below = layers[j - 1];
                s.x = (below.mask ? below.hm : below.h) + t * BH;
            } else if (l.x_in) {
                s.x = l.x_in + t * BH;
            }
            s.w_in = s.x ? l.w_in : nullptr; s.ldw_in = l.ldw_in;
            if (l.emb) {
                s.emb = l.emb; s.E = l.E; s.w_e = l.w_e; s.ldw_e = l.ldw_e;
                s.tok.tok_packed = l.tok_packed; s.tok.tok_const = l.tok_const; s.tok.tok_limit = l.V;
                if (l.ss_targets) {
                    s.tok.ss = SsArgs{l.ss_targets, l.ss_ld, l.ss_prob, (uint32_t)(l.ss_seed & 0xFFFFFFFFull), (uint32_t)(l.ss_seed >> 32),
                                      (uint32_t)l.ss_step, (uint32_t)l.ss_row0, (uint32_t)l.ss_row0 + (uint32_t)B};
                    s.tok.tok_err = flags.p;
                }
            }
            s.mask = l.mask ? l.mask + t * BH : nullptr;
            s.h_out = l.h + t * BH; s.c_out = l.c + t * BH;
            s.stash = l.stash ? l.stash + t * B4H : nullptr;
            s.hm_out = l.mask ? l.hm + t * BH : nullptr;
            if (a.n == CHAIN_MAX) {          // a diagonal longer than one launch: its layer-steps are independent
                if ((rc = lstm_chain_fwd_launch(st, a))) return rc;
                a.n = 0;
            }
        }
        if (a.n && (rc = lstm_chain_fwd_launch(st, a))) return rc;
    }
    return flags.close(st, 3);
}

size_t s2vt_lstm_chain_bwd_workspace_bytes(int32_t B, int32_t H, int32_t n) {
    if (B <= 0 || H <= 0 || n <= 0) return 0;
    // W_hh^T [H,4H] and dc [B,H] per layer, W_in^T [H,4H] per layer above the first; 256-byte aligned pieces
    return (size_t)(2 * n - 1) * align_up((size_t)4 * H * H * sizeof(float), 256) + (size_t)n * align_up((size_t)B * H * sizeof(float), 256);
}

int s2vt_lstm_chain_bwd(int32_t T, int32_t B, int32_t H, int32_t n, const s2vt_lstm_layer* layers, void* workspace,
                        size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = check_chain("s2vt_lstm_chain_bwd", T, B, H, n, layers, true))) return rc;
    S2VT_REQUIRE(workspace && workspace_bytes >= s2vt_lstm_chain_bwd_workspace_bytes(B, H, n),
                 "s2vt_lstm_chain_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, s2vt_lstm_chain_bwd_workspace_bytes(B, H, n));
    hipStream_t st = (hipStream_t)stream;
    const int64_t BH = (int64_t)B * H, B4H = 4 * BH;
    const size_t wbytes = align_up((size_t)4 * H * H * sizeof(float), 256), dbytes = align_up((size_t)B * H * sizeof(float), 256);
    std::vector<float*> whh_t(n), win_t(n), dc(n);
    char* w = (char*)workspace;
    for (int j = 0; j < n; ++j) {
        whh_t[j] = (float*)w; w += wbytes;
        if (j > 0) { win_t[j] = (float*)w; w += wbytes; }
        dc[j] = (float*)w; w += dbytes;
        if (j > 0) {
            const float* src = layers[j].w_in;
            if (layers[j].ldw_in != H) {     // a column block of a wider weight: packed first, in W_hh^T's slot (still free)
                S2VT_HIP(hipMemcpy2DAsync(whh_t[j], H * sizeof(float), src, layers[j].ldw_in * sizeof(float), H * sizeof(float),
                                          4 * H, hipMemcpyDeviceToDevice, st));
                src = whh_t[j];
            }
            if ((rc = transpose_f32(st, src, 4 * H, H, win_t[j]))) return rc;
        }
        if ((rc = transpose_f32(st, layers[j].w_hh, 4 * H, H, whh_t[j]))) return rc;
        if ((rc = fill_zero(st, dc[j], BH * sizeof(float)))) return rc;
    }
    // reverse wavefront: launch d runs layer j at step t = T - 1 - d + (n - 1 - j)
    for (int d = 0; d < T + n - 1; ++d) {
        ChainBwdLaunch a;
        memset(&a, 0, sizeof(a));
        a.B = B; a.H = H;
        for (int j = n - 1; j >= 0; --j) {
            const int t = T - 1 - d + (n - 1 - j);
            if (t < 0 || t >= T) continue;
            const s2vt_lstm_layer& l = layers[j];
            ChainBwdStep& s = a.s[a.n++];
            s.dg_next = t < T - 1 ? l.dg + (t + 1) * B4H : nullptr;
            s.w_hh_t = whh_t[j];
            if (j < n - 1) {
                s.dg_up = layers[j + 1].dg + t * B4H;
                s.w_in_t = win_t[j + 1];
                s.mask = l.mask ? l.mask + t * BH : nullptr;
            }
            s.dh_ext = (l.dh_ext && t >= l.dh_t0) ? l.dh_ext + (t - l.dh_t0) * BH : nullptr;
            s.stash = l.stash + t * B4H;
            s.c = l.c + t * BH;
            s.c_prev = t ? l.c + (t - 1) * BH : l.c0;
            s.dc = dc[j];
            s.dg = l.dg + t * B4H;
            if (a.n == CHAIN_MAX) {
                if ((rc = lstm_chain_bwd_launch(st, a))) return rc;
                a.n = 0;
            }
        }
        if (a.n && (rc = lstm_chain_bwd_launch(st, a))) return rc;
    }
    return 0;
}

}  // extern "C"
