"""Thin tensor-level wrappers over the per-op C-ABI entry points (include/s2vt_hip.h).

Used by the beam-search driver and by the GPU parity tests; no autograd here.  All tensors must be
contiguous float32 HIP tensors unless noted; outputs are allocated by torch.
"""
import ctypes
import math

import torch

from . import capi
from .functional import _ptr, _stream, _f32c, require_hip


def gemm(a, b, bias=None, a_kmajor=True, b_kmajor=True, out=None, accumulate=False):
    """out[M,N] (+)= op(a)·op(b) (+bias).  a: [M,K] if a_kmajor else [K,M]; b: [N,K] if b_kmajor else [K,N]."""
    lib = capi.load()
    a, b = _f32c(a, "a"), _f32c(b, "b")
    M, K = (a.shape if a_kmajor else (a.shape[1], a.shape[0]))
    N = b.shape[0] if b_kmajor else b.shape[1]
    Kb = b.shape[1] if b_kmajor else b.shape[0]
    if K != Kb:
        raise ValueError("gemm: inner dims differ (%d vs %d)" % (K, Kb))
    dev = a.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(M, N, dtype=torch.float32, device=dev)
            if accumulate:
                out.zero_()
        capi.check(lib.s2vt_gemm_f32(int(a_kmajor), int(b_kmajor), M, N, K, _ptr(a), a.stride(0), _ptr(b),
                                     b.stride(0), _ptr(out), out.stride(0), _ptr(bias), int(accumulate),
                                     _stream(dev)), "s2vt_gemm_f32")
    return out


def split_planes(x, nplanes=3, transpose=False):
    """fp32 [rows, cols] -> bf16 planes of a k-major GEMM operand (include/s2vt_hip.h: blocked layout for 3 planes, plain
    rows for 1).  Returns (planes int16 [ceil64(operand rows), nplanes*kpad], ldo, kpad)."""
    lib = capi.load()
    x = _f32c(x, "x")
    rows, cols = x.shape
    orows, k = (cols, rows) if transpose else (rows, cols)
    kpad = (k + 63) // 64 * 64
    ldo = nplanes * kpad
    dev = x.device
    with torch.cuda.device(dev):
        out = torch.zeros((orows + 63) // 64 * 64, ldo, dtype=torch.int16, device=dev)
        capi.check(lib.s2vt_split_planes(nplanes, int(transpose), _ptr(x), x.stride(0), rows, cols, _ptr(out), ldo, kpad,
                                         orows, _stream(dev)), "s2vt_split_planes")
    return out, ldo, kpad


def gemm_planes_tt(pa, pb, M, N, K, bias=None, out=None, accumulate=False, splitk_ws=None, nplanes=3):
    """out[M,N] (+)= X_A^T X_B from the ROW plane images (split_planes(x, nplanes)) of X_A [K, M] and X_B [K, N]; K % 64 == 0."""
    lib = capi.load()
    (a, lda, _), (b, ldb, _) = pa, pb
    dev = a.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.zeros(M, N, dtype=torch.float32, device=dev) if accumulate else \
                torch.empty(M, N, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_gemm_bf16_tt(nplanes, M, N, K, _ptr(a), lda, _ptr(b), ldb, _ptr(out), out.stride(0), _ptr(bias),
                                         int(accumulate), _ptr(splitk_ws),
                                         ctypes.c_size_t(splitk_ws.numel() if splitk_ws is not None else 0), _stream(dev)),
                   "s2vt_gemm_bf16_tt")
    return out


def gemm_planes(pa, pb, M, N, nplanes=3, bias=None, out=None, accumulate=False, splitk_ws=None):
    """out[M,N] (+)= A·B^T (+bias) from operands written by split_planes (same nplanes, same kpad)."""
    lib = capi.load()
    (a, lda, ka), (b, ldb, kb) = pa, pb
    if ka != kb:
        raise ValueError("gemm_planes: operands have different padded k (%d vs %d)" % (ka, kb))
    dev = a.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.zeros(M, N, dtype=torch.float32, device=dev) if accumulate else \
                torch.empty(M, N, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_gemm_bf16_nt(nplanes, M, N, ka, _ptr(a), lda, _ptr(b), ldb, _ptr(out), out.stride(0), _ptr(bias),
                                         int(accumulate), _ptr(splitk_ws),
                                         ctypes.c_size_t(splitk_ws.numel() if splitk_ws is not None else 0), _stream(dev)),
                   "s2vt_gemm_bf16_nt")
    return out


def feat_proj_fwd(feats, w, bias):
    """x1 time-major [L*B, H] = feats[B,L,F]·w^T + bias."""
    lib = capi.load()
    feats, w = _f32c(feats, "feats"), _f32c(w, "w")
    B, L, F = feats.shape
    H = w.shape[0]
    d = capi.Dims(B, L, F, H, 1, 1)
    dev = feats.device
    with torch.cuda.device(dev):
        x1 = torch.empty(L * B, H, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_feat_proj_fwd(ctypes.byref(d), _ptr(feats), _ptr(w), _ptr(bias), _ptr(x1), _stream(dev)),
                   "s2vt_feat_proj_fwd")
    return x1


def feat_proj_bwd(feats, w, dx1, need_dfeats=False):
    lib = capi.load()
    feats, w, dx1 = _f32c(feats, "feats"), _f32c(w, "w"), _f32c(dx1, "dx1")
    B, L, F = feats.shape
    H = w.shape[0]
    d = capi.Dims(B, L, F, H, 1, 1)
    dev = feats.device
    with torch.cuda.device(dev):
        dw = torch.empty_like(w)
        db = torch.empty(H, dtype=torch.float32, device=dev)
        dfe = torch.empty_like(feats) if need_dfeats else None
        ws = torch.empty(max(1, lib.s2vt_colsum_ws_floats(L * B, H)), dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_feat_proj_bwd(ctypes.byref(d), _ptr(feats), _ptr(w), _ptr(dx1), _ptr(dw), _ptr(db),
                                          _ptr(dfe), _ptr(ws), _stream(dev)), "s2vt_feat_proj_bwd")
    return dw, db, dfe


def lstm_step_fwd(gx, bias, w_hh, h_prev, c_prev, want_stash=False):
    """One LSTM step; gx [B,4H] or None (then bias [4H]); h_prev/c_prev [B,H] or None."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    B = gx.shape[0] if gx is not None else h_prev.shape[0]
    dev = w_hh.device
    with torch.cuda.device(dev):
        h = torch.empty(B, H, dtype=torch.float32, device=dev)
        c = torch.empty(B, H, dtype=torch.float32, device=dev)
        stash = torch.empty(B, 4 * H, dtype=torch.float32, device=dev) if want_stash else None
        capi.check(lib.s2vt_lstm_step_fwd(B, H, _ptr(gx), _ptr(bias), _ptr(w_hh), _ptr(h_prev), _ptr(c_prev), _ptr(h),
                                          _ptr(c), _ptr(stash), _stream(dev)), "s2vt_lstm_step_fwd")
    return (h, c, stash) if want_stash else (h, c)


def lstm_step_fwd_token(gx, w_hh, h_prev, c_prev, emb, w_ih, tok=None, tok_packed=None, tok_const=0):
    """One decode step of word_rnn (S2VTModel.py:100-103): gx [B,4H] (vid_out half of the gate input + biases), emb [V,E],
    w_ih [4H, E+H] (its first E columns multiply the embedded word).  Token per row: `tok` int32 [B], else `tok_packed` (the
    packed argmax words of decode_step_argmax), else `tok_const`.  Ids outside [0, V) raise IndexError at the next
    capi.check_async_error()."""
    lib = capi.load()
    gx, w_hh, emb, w_ih = _f32c(gx, "gx"), _f32c(w_hh, "w_hh"), _f32c(emb, "emb"), _f32c(w_ih, "w_ih")
    B, H = gx.shape[0], w_hh.shape[1]
    V, E = emb.shape
    dev = gx.device
    with torch.cuda.device(dev):
        h = torch.empty(B, H, dtype=torch.float32, device=dev)
        c = torch.empty(B, H, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_lstm_step_fwd_token(B, H, E, V, _ptr(gx), _ptr(w_hh), _ptr(h_prev), _ptr(c_prev), _ptr(emb), _ptr(w_ih),
                                                w_ih.stride(0), _ptr(tok), _ptr(tok_packed), int(tok_const), _ptr(h), _ptr(c),
                                                _stream(dev)), "s2vt_lstm_step_fwd_token")
    return h, c


def lstm_step_bwd(dg_next, w_hh_t, dh_out, stash, c, c_prev, dc, dc_is_zero):
    lib = capi.load()
    B, H4 = stash.shape
    H = H4 // 4
    dev = stash.device
    with torch.cuda.device(dev):
        dg = torch.empty_like(stash)
        capi.check(lib.s2vt_lstm_step_bwd(B, H, _ptr(dg_next), _ptr(w_hh_t), _ptr(dh_out), _ptr(stash), _ptr(c),
                                          _ptr(c_prev), _ptr(dc), int(dc_is_zero), _ptr(dg), _stream(dev)),
                   "s2vt_lstm_step_bwd")
    return dg


def lstm_seq_fwd(T, B, gx, n_gx, bias, w_hh, want_stash=False):
    """Whole layer from zero state; gx [n_gx*B, 4H] time-major (overwritten by the stash if want_stash)."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        h_all = torch.empty(T * B, H, dtype=torch.float32, device=dev)
        c_all = torch.empty(T * B, H, dtype=torch.float32, device=dev)
        stash = None
        if want_stash:
            stash = torch.empty(T * B, 4 * H, dtype=torch.float32, device=dev)
            if n_gx:
                stash[:n_gx * B].copy_(gx)
            gx = stash
        capi.check(lib.s2vt_lstm_seq_fwd(T, B, H, _ptr(gx), n_gx, _ptr(bias), _ptr(w_hh), _ptr(h_all), _ptr(c_all),
                                         _ptr(stash), _stream(dev)), "s2vt_lstm_seq_fwd")
    return h_all, c_all, stash


def lstm_seq_bwd(T, B, w_hh, dh_out, dh_first, c_all, stash):
    """BPTT over a layer; returns dG [T*B,4H] (stash is consumed in place)."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        wt = torch.empty(H, 4 * H, dtype=torch.float32, device=dev)
        dc = torch.empty(B, H, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_lstm_seq_bwd(T, B, H, _ptr(w_hh), _ptr(dh_out), dh_first, _ptr(c_all), _ptr(stash),
                                         _ptr(wt), _ptr(dc), _stream(dev)), "s2vt_lstm_seq_bwd")
    return stash


def decode_step_argmax(h, w_out, b_out, planes=False):
    """token ids int64 [B] = argmax_v (h·w_out^T + b_out), lowest index on ties.  planes: the bf16-matrix-core kernel on
    3-plane operands (s2vt_decode_step_argmax_x3) instead of the fp32-input MFMA one."""
    lib = capi.load()
    h, w_out = _f32c(h, "h"), _f32c(w_out, "w_out")
    B, H = h.shape
    V = w_out.shape[0]
    dev = h.device
    with torch.cuda.device(dev):
        packed = torch.zeros(B, dtype=torch.int64, device=dev)
        if planes:
            nbytes = lib.s2vt_decode_step_argmax_x3_workspace_bytes(B, H, V)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            capi.check(lib.s2vt_decode_step_argmax_x3(B, H, V, _ptr(h), _ptr(w_out), _ptr(b_out), _ptr(packed), _ptr(ws), nbytes,
                                                      _stream(dev)), "s2vt_decode_step_argmax_x3")
            return 0xFFFFFFFF - (packed & 0xFFFFFFFF)
        capi.check(lib.s2vt_decode_step_argmax(B, H, V, _ptr(h), _ptr(w_out), _ptr(b_out), _ptr(packed), _stream(dev)),
                   "s2vt_decode_step_argmax")
        return 0xFFFFFFFF - (packed & 0xFFFFFFFF)


def decode_step_sample(h, w_out, b_out, temperature=1.0, seed=0, step=0, row0=0, planes=False, return_packed=False):
    """token ids int64 [B]: one draw per row from softmax((h·w_out^T + b_out) / temperature) by Gumbel-max - the arg-max kernels of
    decode_step_argmax with the noise of sampling.gumbel_noise(seed, step, row0 + b, V) added to logit / temperature.
    return_packed: (ids, packed) with the raw packed words (high half = the ordered bits of the winning score)."""
    lib = capi.load()
    h, w_out = _f32c(h, "h"), _f32c(w_out, "w_out")
    B, H = h.shape
    V = w_out.shape[0]
    temperature = float(temperature)
    if not (0.0 < temperature < float("inf")):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    dev = h.device
    with torch.cuda.device(dev):
        packed = torch.zeros(B, dtype=torch.int64, device=dev)
        if planes:
            nbytes = lib.s2vt_decode_step_sample_x3_workspace_bytes(B, H, V)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            capi.check(lib.s2vt_decode_step_sample_x3(B, H, V, _ptr(h), _ptr(w_out), _ptr(b_out), temperature, int(seed), int(step),
                                                      int(row0), _ptr(packed), _ptr(ws), nbytes, _stream(dev)),
                       "s2vt_decode_step_sample_x3")
        else:
            capi.check(lib.s2vt_decode_step_sample(B, H, V, _ptr(h), _ptr(w_out), _ptr(b_out), temperature, int(seed), int(step),
                                                   int(row0), _ptr(packed), _stream(dev)), "s2vt_decode_step_sample")
        ids = 0xFFFFFFFF - (packed & 0xFFFFFFFF)
    return (ids, packed) if return_packed else ids


def _trunc_of(sample, V):
    """(top_k, top_p) of a sample tuple (temperature, seed[, top_k, top_p]) where they cut anything off a row of V scores, else None"""
    from .sampling import truncates
    return tuple(sample[2:4]) if sample is not None and len(sample) == 4 and truncates(sample[2], sample[3], V) else None


def truncated_draw(logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, row0=0, return_kept=False, return_packed=False, packed=None):
    """token ids int64 [rows]: one draw per logits row from softmax(logits / temperature) cut to the top_k largest scores and then to
    the nucleus of mass top_p (s2vt_truncated_draw; the definition: sampling.py, include/s2vt_hip.h), with the noise of
    sampling.gumbel_noise(seed, step, row0 + r, V).  logits: fp32 [rows, V], unit column stride (a row stride > V is fine).
    return_kept / return_packed add the survivors per row (int32) / the raw packed words (high half = ordered bits of the winning
    score), in that order.  packed: the caller's int64 [rows] to write the words to (no allocation)."""
    from .sampling import check_truncation
    lib = capi.load()
    require_hip(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    temperature = float(temperature)
    if not (0.0 < temperature < float("inf")):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    top_k, top_p = check_truncation(top_k, top_p, V)
    dev = logits.device
    with torch.cuda.device(dev):
        if packed is None:
            packed = torch.empty(rows, dtype=torch.int64, device=dev)
        kept = torch.empty(rows, dtype=torch.int32, device=dev) if return_kept else None
        capi.check(lib.s2vt_truncated_draw(_ptr(logits), logits.stride(0), rows, V, temperature, top_k, top_p, int(seed), int(step),
                                           int(row0), _ptr(packed), _ptr(kept), _stream(dev)), "s2vt_truncated_draw")
        ids = 0xFFFFFFFF - (packed & 0xFFFFFFFF)
    out = (ids,) + ((kept,) if return_kept else ()) + ((packed,) if return_packed else ())
    return out if len(out) > 1 else ids


def constrained_draw(logits, hist, t, spec, greedy=False, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, row0=0, return_kept=False,
                     return_packed=False, packed=None):
    """token ids int64 [rows]: the constrained draw of decode step t (s2vt_constrained_draw; the definition: sampling.py,
    include/s2vt_hip.h "constrained draw") - repetition penalty, no-repeat n-gram, banned ids and minimum length of `spec` (a
    sampling.ConstraintSpec) applied to the raw logits, then the arg-max (greedy) or truncated_draw's draw on the constrained row.
    THE CALL MODIFIES `logits` (fp32 [rows, V], unit column stride): afterwards it holds the constrained rows.  hist: the decoders'
    packed words, int64 [>= t, hist_ld >= rows] with unit column stride (row r's word of step i at hist[i, r]; the token is
    0xFFFFFFFF - the low half); None where t == 0.  return_kept / return_packed / packed as for truncated_draw."""
    from .sampling import check_truncation, constraints_struct
    lib = capi.load()
    require_hip(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    t = int(t)
    temperature = float(temperature)
    if not (0.0 < temperature < float("inf")):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    top_k, top_p = check_truncation(top_k, top_p, V)
    hist_ld = 0
    if t > 0:
        require_hip(hist, "hist")
        if hist.dim() != 2 or hist.dtype != torch.int64 or hist.stride(1) != 1 or hist.shape[0] < t or hist.shape[1] < rows:
            raise ValueError("hist must be int64 [>= t = %d, >= rows = %d] with unit column stride" % (t, rows))
        hist_ld = hist.stride(0)
    dev = logits.device
    with torch.cuda.device(dev):
        if packed is None:
            packed = torch.empty(rows, dtype=torch.int64, device=dev)
        kept = torch.empty(rows, dtype=torch.int32, device=dev) if return_kept else None
        cs, keep = constraints_struct(spec)
        capi.check(lib.s2vt_constrained_draw(_ptr(logits), logits.stride(0), rows, V, _ptr(hist) if t > 0 else None, hist_ld, t,
                                             ctypes.byref(cs), 1 if greedy else 0, temperature, top_k, top_p, int(seed), int(step),
                                             int(row0), _ptr(packed), _ptr(kept), _stream(dev)), "s2vt_constrained_draw")
        ids = 0xFFFFFFFF - (packed & 0xFFFFFFFF)
    out = (ids,) + ((kept,) if return_kept else ()) + ((packed,) if return_packed else ())
    return out if len(out) > 1 else ids


def top20_logprob(logits):
    """(top_ix int32 [rows, 20], top_lp fp32 [rows, 20]): the 20 most probable tokens of every logits row in ascending token order
    and their log-probs - the beam searches' fan-out kernel on its own (s2vt_top20_logprob).  logits: fp32 [rows, V >= 20]."""
    lib = capi.load()
    require_hip(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    dev = logits.device
    with torch.cuda.device(dev):
        ix = torch.empty(rows, 20, dtype=torch.int32, device=dev)
        lp = torch.empty(rows, 20, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_top20_logprob(_ptr(logits), logits.stride(0), rows, V, _ptr(ix), _ptr(lp), _stream(dev)), "s2vt_top20_logprob")
    return ix, lp


def top20_gumbel(logits, inv_temperature=1.0, seed=0, step=0, row0=0):
    """(top_ix int32 [rows, 20], top_lp fp32 [rows, 20], top_g fp32 [rows, 20]): the fan-out head of S2VT.sample_distinct on its own
    (s2vt_top20_gumbel; include/s2vt_hip.h "stochastic beam") - per row the 20 words with the largest g_v = lp_v + noise, lp =
    log_softmax(logits * inv_temperature) and the noise sampling.gumbel_noise(seed, step, row0 + r, V), in the order (g descending,
    v ascending), with their unperturbed log-probs and their g.  logits: fp32 [rows, 20 <= V <= 38400], unit column stride (a row
    stride > V is fine); inv_temperature: the fp32 factor itself."""
    lib = capi.load()
    require_hip(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    dev = logits.device
    with torch.cuda.device(dev):
        ix = torch.empty(rows, 20, dtype=torch.int32, device=dev)
        lp = torch.empty(rows, 20, dtype=torch.float32, device=dev)
        g = torch.empty(rows, 20, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_top20_gumbel(_ptr(logits), logits.stride(0), rows, V, float(inv_temperature), int(seed), int(step), int(row0),
                                         _ptr(ix), _ptr(lp), _ptr(g), _stream(dev)), "s2vt_top20_gumbel")
    return ix, lp, g


def sbs_state(B, n_samples, max_depth, dev):
    """the policy state of a stochastic beam search (uint8, s2vt_sbs_bytes) and its rows int32 [3, B * n_samples] (sample, state row,
    token), for sbs_step / sbs_result"""
    nbytes = capi.load().s2vt_sbs_bytes(B, n_samples, max_depth)
    if nbytes == 0:
        raise ValueError("sbs: %d clips x %d samples x depth %d is not a shape the policy serves" % (B, n_samples, max_depth))
    with torch.cuda.device(dev):
        return torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.zeros(3, B * n_samples, dtype=torch.int32, device=dev)


def sbs_step(state, rows, B, n_samples, max_depth, sos_ix, eos_ix, depth, top_ix=None, top_lp=None, top_g=None):
    """One call of the stochastic beam's policy (s2vt_sbs_step; csrc/sbs_policy.hip) on a state of sbs_state: depth = 1 initialises,
    depth = 2..max_depth consumes the [B * n_samples, 20] arrays (int32, fp32, fp32; a head's output, best g first) of step depth - 1,
    depth = 0 those of step max_depth.  Writes `rows` for the next depth step; the int32 at byte 0 of `state` counts frozen clips."""
    lib = capi.load()
    dev = state.device
    R = B * n_samples
    if depth != 1:
        for t, dt, name in ((top_ix, torch.int32, "top_ix"), (top_lp, torch.float32, "top_lp"), (top_g, torch.float32, "top_g")):
            require_hip(t, name)
            if t.dtype != dt or tuple(t.shape) != (R, 20) or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s [%d, 20]" % (name, dt, R))
    if rows.dtype != torch.int32 or tuple(rows.shape) != (3, R) or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous int32 [3, %d]" % R)
    with torch.cuda.device(dev):
        capi.check(lib.s2vt_sbs_step(B, n_samples, max_depth, int(sos_ix), int(eos_ix), int(depth), _ptr(state), state.numel(),
                                     _ptr(top_ix), _ptr(top_lp), _ptr(top_g), _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), _stream(dev)),
                   "s2vt_sbs_step")


def sbs_result(state, B, n_samples, max_depth, eos_ix):
    """(ids int32 [B, W, D] padded with eos_ix, lengths int32 [B, W], logprob fp32 [B, W], perturbed fp32 [B, W], kappa fp32 [B]) of a
    stepped state (s2vt_sbs_result)"""
    lib = capi.load()
    dev = state.device
    with torch.cuda.device(dev):
        ids = torch.empty(B, n_samples, max_depth, dtype=torch.int32, device=dev)
        lens = torch.empty(B, n_samples, dtype=torch.int32, device=dev)
        lp = torch.empty(B, n_samples, dtype=torch.float32, device=dev)
        g = torch.empty(B, n_samples, dtype=torch.float32, device=dev)
        kappa = torch.empty(B, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_sbs_result(B, n_samples, max_depth, int(eos_ix), _ptr(state), state.numel(), _ptr(ids), _ptr(lens), _ptr(lp),
                                       _ptr(g), _ptr(kappa), _stream(dev)), "s2vt_sbs_result")
    return ids, lens, lp, g, kappa


def top20_logprob_constrained(logits, hist, t, spec):
    """(top_ix int32 [rows, 20], top_lp fp32 [rows, 20]): top20_logprob of the rows CONSTRAINED by `spec` (a sampling.ConstraintSpec)
    at step t - the fan-out head of S2VT.beam_constrained on its own (s2vt_top20_logprob_constrained; include/s2vt_hip.h "constrained
    beam").  THE CALL MODIFIES `logits` (fp32 [rows, V], unit column stride): afterwards it holds sampling.constrain_logits of the
    rows, and the log-probs are log_softmax of those.  hist: int32 [rows, >= t] with unit column stride, row r's words hist[r, :t]
    (the beam slots' layout); None where t == 0.  V >= 20 + t + banned ids + 1."""
    from .sampling import constraints_struct
    lib = capi.load()
    require_hip(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("logits must be fp32 [rows, V] with unit column stride")
    rows, V = logits.shape
    t = int(t)
    hist_ld = 0
    if t > 0:
        require_hip(hist, "hist")
        if hist.dim() != 2 or hist.dtype != torch.int32 or hist.stride(1) != 1 or hist.shape[0] < rows or hist.shape[1] < t:
            raise ValueError("hist must be int32 [>= rows = %d, >= t = %d] with unit column stride" % (rows, t))
        hist_ld = hist.stride(0)
    dev = logits.device
    with torch.cuda.device(dev):
        ix = torch.empty(rows, 20, dtype=torch.int32, device=dev)
        lp = torch.empty(rows, 20, dtype=torch.float32, device=dev)
        cs, keep = constraints_struct(spec)
        capi.check(lib.s2vt_top20_logprob_constrained(_ptr(logits), logits.stride(0), rows, V, _ptr(hist) if t > 0 else None, hist_ld, t,
                                                      ctypes.byref(cs), _ptr(ix), _ptr(lp), _stream(dev)), "s2vt_top20_logprob_constrained")
    return ix, lp


def ensemble_log_weights(weights, M):
    """fp32 log weights of an ensemble's M members (include/s2vt_hip.h "ensemble beam") as a ctypes float array: the weights
    normalised to sum 1 in fp64, the log in fp64, then fp32.  None: uniform.  ValueError ("Ensemble:") unless there are M of them,
    each finite and > 0."""
    import math
    if weights is None:
        weights = [1.0] * M
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError("Ensemble: weights must be %d numbers, got %r" % (M, weights))
    if len(w) != M:
        raise ValueError("Ensemble: %d weights for %d members" % (len(w), M))
    if not all(math.isfinite(x) and x > 0 for x in w):
        raise ValueError("Ensemble: weights must be finite and > 0, got %r" % (w,))
    tot = math.fsum(w)
    return (ctypes.c_float * M)(*[min(math.log(x / tot), 0.0) for x in w])      # (c_float rounds the fp64 log to fp32)


def _ensemble_logits(logits):
    require_hip(logits, "logits")
    if logits.dim() != 3 or logits.dtype != torch.float32 or logits.stride(2) != 1:
        raise ValueError("logits must be fp32 [M, rows, V] with unit column stride")
    return logits.shape


def ensemble_top20(logits, weights=None):
    """(top_ix int32 [rows, 20], top_lp fp32 [rows, 20]): the fan-out head of S2VT.Ensemble on its own (s2vt_ensemble_top20;
    include/s2vt_hip.h "ensemble beam") - per row the 20 best words, in ascending token order, of the log of the weighted mean of
    the M members' softmax distributions, and those log-probs.  logits: fp32 [M, rows, V >= 20], 1 <= M <= 8; weights: M positive
    numbers (normalised here), None: uniform.  M = 1 is top20_logprob."""
    lib = capi.load()
    M, rows, V = _ensemble_logits(logits)
    if not 1 <= M <= 8:
        raise ValueError("Ensemble: 1 to 8 members, got %d" % M)
    lw = ensemble_log_weights(weights, M)
    dev = logits.device
    with torch.cuda.device(dev):
        ix = torch.empty(rows, 20, dtype=torch.int32, device=dev)
        lp = torch.empty(rows, 20, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_ensemble_top20(_ptr(logits), logits.stride(0), logits.stride(1), M, rows, V, lw, _ptr(ix), _ptr(lp),
                                           _stream(dev)), "s2vt_ensemble_top20")
    return ix, lp


def ensemble_top20_constrained(logits, hist, t, spec, weights=None):
    """ensemble_top20 of the rows CONSTRAINED by `spec` at step t (s2vt_ensemble_top20_constrained): every member's row r is first
    edited with row r's words hist[r, :t] as top20_logprob_constrained edits it - THE CALL MODIFIES `logits` - and the members'
    distributions are those of the edited rows.  hist: int32 [rows, >= t], None where t == 0.  V >= 20 + t + banned ids + 1.  A spec
    that constrains nothing runs ensemble_top20's launch and leaves `logits` untouched."""
    from .sampling import constraints_struct
    lib = capi.load()
    M, rows, V = _ensemble_logits(logits)
    if not 1 <= M <= 8:
        raise ValueError("Ensemble: 1 to 8 members, got %d" % M)
    lw = ensemble_log_weights(weights, M)
    t = int(t)
    hist_ld = 0
    if t > 0:
        require_hip(hist, "hist")
        if hist.dim() != 2 or hist.dtype != torch.int32 or hist.stride(1) != 1 or hist.shape[0] < rows or hist.shape[1] < t:
            raise ValueError("hist must be int32 [>= rows = %d, >= t = %d] with unit column stride" % (rows, t))
        hist_ld = hist.stride(0)
    dev = logits.device
    with torch.cuda.device(dev):
        ix = torch.empty(rows, 20, dtype=torch.int32, device=dev)
        lp = torch.empty(rows, 20, dtype=torch.float32, device=dev)
        cs, keep = constraints_struct(spec)
        capi.check(lib.s2vt_ensemble_top20_constrained(_ptr(logits), logits.stride(0), logits.stride(1), M, rows, V, lw,
                                                       _ptr(hist) if t > 0 else None, hist_ld, t, ctypes.byref(cs), _ptr(ix), _ptr(lp),
                                                       _stream(dev)), "s2vt_ensemble_top20_constrained")
    return ix, lp


def decode_step_token_into(h, w_out, b_out, packed_i, sample=None, step=0, constraints=None):
    """out_linear + arg-max of one decode step into the caller's packed word row `packed_i` (int64 [B], zeroed) - what the greedy
    loops of the GRU and stacked models run per step; sample = (temperature, seed): the draw of mode='sample' for decode step
    `step` instead (s2vt_decode_step_sample); sample = (temperature, seed, top_k, top_p) that truncate: the logits GEMM and
    s2vt_truncated_draw.  constraints = (spec, packed_history, t): the logits GEMM and s2vt_constrained_draw on the loop's own
    packed words (int64 [steps, B]; the words of the t steps before) - the arg-max of the constrained row where sample is None,
    else the (truncated) draw on it.  No synchronisation; no allocation but the truncated and constrained forms' logits."""
    lib = capi.load()
    B, H = h.shape
    V = w_out.shape[0]
    dev = h.device
    trunc = _trunc_of(sample, V)
    if constraints is not None:
        spec, hist, t = constraints
        k, p = trunc if trunc is not None else (0, 1.0)
        constrained_draw(gemm(h, w_out, b_out), hist, t, spec, greedy=sample is None, temperature=1.0 if sample is None else sample[0],
                         top_k=k, top_p=p, seed=0 if sample is None else sample[1], step=step, packed=packed_i)
    elif trunc is not None:
        truncated_draw(gemm(h, w_out, b_out), sample[0], trunc[0], trunc[1], sample[1], step, packed=packed_i)
    elif sample is None:
        capi.check(lib.s2vt_decode_step_argmax(B, H, V, _ptr(h), _ptr(w_out), _ptr(b_out), _ptr(packed_i), _stream(dev)),
                   "s2vt_decode_step_argmax")
    else:
        capi.check(lib.s2vt_decode_step_sample(B, H, V, _ptr(h), _ptr(w_out), _ptr(b_out), sample[0], sample[1], int(step), 0,
                                               _ptr(packed_i), _stream(dev)), "s2vt_decode_step_sample")


def packed_score(packed):
    """fp32 scores from the high halves of packed arg-max words (the inverse of the kernels' order-preserving bit map)"""
    hi = (packed >> 32) & 0xFFFFFFFF
    u = torch.where(hi >= 0x80000000, hi - 0x80000000, 0xFFFFFFFF - hi)            # the float's own bits, as a non-negative int64
    return torch.where(u >= 0x80000000, u - 0x100000000, u).to(torch.int32).view(torch.float32)


def beam_step(params, dims, row_b, row_state, tok, vid_h, vid_c, word_h, word_c):
    """One s2vt_beam_step call (include/s2vt_hip.h).  params: 13 tensors in capi.PARAM_KEYS order; dims = (B,L,F,H,E,V);
    row_b / row_state / tok: int32 [R].  Returns (vid_h', vid_c', word_h' [R,H], word_c' [R,H], top_ix [R,20] int32,
    top_lp [R,20] fp32)."""
    from .functional import _params_struct
    lib = capi.load()
    d = capi.Dims(*dims)
    B, H = dims[0], dims[3]
    R = int(row_b.numel())
    dev = vid_h.device
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(d), max(R, 1))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        vh, vc = torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
        wh, wc = torch.empty(max(R, 1), H, device=dev), torch.empty(max(R, 1), H, device=dev)
        tix = torch.empty(max(R, 1), 20, dtype=torch.int32, device=dev)
        tlp = torch.empty(max(R, 1), 20, dtype=torch.float32, device=dev)
        ps = _params_struct(capi.Params, tuple(_f32c(p, "parameter") for p in params))
        capi.check(lib.s2vt_beam_step(ctypes.byref(d), ctypes.byref(ps), R, _ptr(row_b), _ptr(row_state), _ptr(tok),
                                      _ptr(_f32c(vid_h, "vid_h")), _ptr(_f32c(vid_c, "vid_c")), _ptr(vh), _ptr(vc),
                                      _ptr(_f32c(word_h, "word_h")), _ptr(_f32c(word_c, "word_c")), _ptr(wh), _ptr(wc),
                                      _ptr(tix), _ptr(tlp), _ptr(ws), nbytes, _stream(dev)), "s2vt_beam_step")
    return vh, vc, wh[:R], wc[:R], tix[:R], tlp[:R]


def _bf16_workspace(nbytes, dev, poison):
    """the workspace of the bf16 recurrence entry points: zeros, or (poison) 0xFF bytes - bf16 NaN patterns, counters and error
    flag at their maximum: the entry points themselves must establish whatever part of it the kernels rely on"""
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev) if poison else torch.zeros(nbytes, dtype=torch.uint8, device=dev)


def seq_bf16_layout(T, B, H, backward=False):
    """{"w": (byte offset, row stride, kpad), "rows": (...)} of the bf16 weight image and the bf16 row image (h rows of the forward,
    dG rows of the backward) inside the workspace `return_workspace=True` hands back; a _pair workspace holds two, the second at
    + the single-layer workspace size.  From the library's own carver (s2vt_lstm_seq_bf16_layout)."""
    lib = capi.load()
    out = (ctypes.c_int64 * 6)()
    capi.check(lib.s2vt_lstm_seq_bf16_layout(T, B, H, int(bool(backward)), out), "s2vt_lstm_seq_bf16_layout")
    return {"w": tuple(out[0:3]), "rows": tuple(out[3:6])}


def lstm_seq_fwd_bf16(gx, n_gx, bias, w_hh, T, B, H, persistent=False, block=0, poison=False, return_workspace=False):
    """Config-3 arithmetic of one LSTM layer (bf16 operands, fp32 accumulate / cell state): returns (h_all, c_all, gates)
    [T*B,H], [T*B,H], [T*B,4H].  `gx` [T*B,4H] is left untouched (the kernels work on a copy: the gate stash is written
    in place of the gate input).  persistent: one launch per `block` steps (0 = all).  poison: the workspace is handed over full
    of 0xFF bytes instead of zeros; return_workspace: the workspace is appended to the result (seq_bf16_layout)."""
    lib = capi.load()
    dev = w_hh.device
    stash = _f32c(gx, "gx").clone()
    w_hh = _f32c(w_hh, "w_hh")
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_lstm_seq_bf16_workspace_bytes(T, B, H)
        ws = _bf16_workspace(nbytes, dev, poison)
        # (NaN: an element the kernels leave unwritten shows)
        h_all = torch.full((T * B, H), float("nan"), dtype=torch.float32, device=dev)
        c_all = torch.full((T * B, H), float("nan"), dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_lstm_seq_fwd_bf16(T, B, H, _ptr(stash), int(n_gx), _ptr(bias), _ptr(w_hh), _ptr(h_all),
                                              _ptr(c_all), _ptr(ws), nbytes, int(persistent), int(block), _stream(dev)),
                   "s2vt_lstm_seq_fwd_bf16")
        if int(ws[:4].view(torch.int32)[0].item()) != 0:
            raise capi.S2VTHipError("persistent recurrence: a hand-off wait timed out (workgroups not co-resident?)")
    return (h_all, c_all, stash, ws) if return_workspace else (h_all, c_all, stash)


def lstm_seq_fwd_bf16_pair(gx0, gx1, n_gx, bias0, bias1, w0, w1, T, B, H, block=0, poison=False, return_workspace=False):
    """Two independent layers, every block of timesteps of both in ONE persistent launch.  Returns two (h_all, c_all, gates)
    (and, return_workspace, the workspace of both as a third element); poison as in lstm_seq_fwd_bf16."""
    lib = capi.load()
    dev = w0.device
    st0, st1 = _f32c(gx0, "gx0").clone(), _f32c(gx1, "gx1").clone()
    w0, w1 = _f32c(w0, "w0"), _f32c(w1, "w1")
    with torch.cuda.device(dev):
        nbytes = 2 * lib.s2vt_lstm_seq_bf16_workspace_bytes(T, B, H)
        ws = _bf16_workspace(nbytes, dev, poison)
        outs = [torch.full((T * B, H), float("nan"), dtype=torch.float32, device=dev) for _ in range(4)]
        capi.check(lib.s2vt_lstm_seq_fwd_bf16_pair(T, B, H, _ptr(st0), _ptr(st1), int(n_gx), _ptr(bias0), _ptr(bias1), _ptr(w0),
                                                   _ptr(w1), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(ws),
                                                   nbytes, int(block), _stream(dev)), "s2vt_lstm_seq_fwd_bf16_pair")
        if int(ws[:4].view(torch.int32)[0].item()) != 0:
            raise capi.S2VTHipError("persistent recurrence: a hand-off wait timed out (workgroups not co-resident?)")
    res = (outs[0], outs[2], st0), (outs[1], outs[3], st1)
    return res + (ws,) if return_workspace else res


def _check_persist_err(ws):
    if int(ws[:4].view(torch.int32)[0].item()) != 0:
        raise capi.S2VTHipError("persistent recurrence: a hand-off wait timed out (workgroups not co-resident?)")


def lstm_seq_bwd_bf16(w_hh, dh_out, dh_first, c_all, gates, T, B, H, persistent=False, block=0, poison=False, return_workspace=False):
    """Config-3 arithmetic of one layer's BPTT: returns fp32 dG [T*B,4H] (`gates` is left untouched).  poison / return_workspace
    as in lstm_seq_fwd_bf16 (then (dG, workspace) is returned)."""
    lib = capi.load()
    dev = w_hh.device
    dg = _f32c(gates, "gates").clone()
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_lstm_seq_bwd_bf16_workspace_bytes(T, B, H)
        ws = _bf16_workspace(nbytes, dev, poison)
        capi.check(lib.s2vt_lstm_seq_bwd_bf16(T, B, H, _ptr(_f32c(w_hh, "w_hh")), _ptr(dh_out), int(dh_first), _ptr(_f32c(c_all, "c_all")),
                                              _ptr(dg), _ptr(ws), nbytes, int(persistent), int(block), _stream(dev)),
                   "s2vt_lstm_seq_bwd_bf16")
        _check_persist_err(ws)
    return (dg, ws) if return_workspace else dg


def lstm_seq_bwd_bf16_pair(w0, w1, dh0, dh1, dh_first, c0, c1, gates0, gates1, T, B, H, block=0, poison=False, return_workspace=False):
    """Two layers' BPTT, every block of both in ONE persistent launch: returns (dG0, dG1) (and, return_workspace, the workspace)."""
    lib = capi.load()
    dev = w0.device
    dg0, dg1 = _f32c(gates0, "gates0").clone(), _f32c(gates1, "gates1").clone()
    with torch.cuda.device(dev):
        nbytes = 2 * lib.s2vt_lstm_seq_bwd_bf16_workspace_bytes(T, B, H)
        ws = _bf16_workspace(nbytes, dev, poison)
        capi.check(lib.s2vt_lstm_seq_bwd_bf16_pair(T, B, H, _ptr(_f32c(w0, "w0")), _ptr(_f32c(w1, "w1")), _ptr(dh0), _ptr(dh1),
                                                   int(dh_first), _ptr(_f32c(c0, "c0")), _ptr(_f32c(c1, "c1")), _ptr(dg0), _ptr(dg1),
                                                   _ptr(ws), nbytes, int(block), _stream(dev)), "s2vt_lstm_seq_bwd_bf16_pair")
        _check_persist_err(ws)
    return (dg0, dg1, ws) if return_workspace else (dg0, dg1)


def lstm_seq_fwd_persist(T, B, gx, n_gx, bias, w_hh, block=0, second=None, poison=True):
    """fp32-equivalent layer forward with the persistent split-precision kernel (three bf16 planes per operand,
    lstm_persist_x3.hip): returns (h_all, c_all, gates).  `second` = (gx, bias, w_hh) of another layer of the same shape that
    shares every launch: then a pair of result tuples is returned."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        # (0xFF bytes: bf16 NaN patterns - the kernel must never read a plane element it has not written)
        n = lib.s2vt_lstm_seq_x3_workspace_bytes(T, B, H)
        if n == 0:
            raise capi.S2VTHipError("lstm_seq_fwd_persist: shape B=%d H=%d is not supported on this device" % (B, H))
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev) if poison else torch.empty(n, dtype=torch.uint8, device=dev)
        sets = []
        for g, b, w in [(gx, bias, w_hh)] + ([second] if second is not None else []):
            stash = torch.empty(T * B, 4 * H, dtype=torch.float32, device=dev)
            if n_gx:
                stash[:n_gx * B].copy_(g)
            sets.append((stash, b, _f32c(w, "w_hh"), torch.empty(T * B, H, dtype=torch.float32, device=dev),
                         torch.empty(T * B, H, dtype=torch.float32, device=dev)))
        a, b2 = sets[0], (sets[1] if len(sets) > 1 else (None,) * 5)
        capi.check(lib.s2vt_lstm_seq_fwd_x3_persist(T, B, H, _ptr(a[0]), _ptr(b2[0]), int(n_gx), _ptr(a[1]), _ptr(b2[1]), _ptr(a[2]),
                                                    _ptr(b2[2]), _ptr(a[3]), _ptr(b2[3]), _ptr(a[4]), _ptr(b2[4]), int(block),
                                                    _ptr(ws), n, _stream(dev)), "s2vt_lstm_seq_fwd_x3_persist")
        _check_persist_err(ws)
    outs = [(x[3], x[4], x[0]) for x in sets]
    return outs[0] if second is None else tuple(outs)


def lstm_seq_bwd_persist(T, B, w_hh, dh_out, dh_first, c_all, gates, block=0, second=None):
    """fp32-equivalent BPTT with the persistent split-precision reduce-scatter kernel (lstm_persist_x3.hip): returns dG (`gates`
    untouched).  `second` = (w_hh, dh_out, c_all, gates)."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        n = lib.s2vt_lstm_seq_bwd_x3_workspace_bytes(T, B, H, int(block))
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)     # (NaN patterns: nothing may be read before it is written)
        sets = [(_f32c(w, "w_hh"), dh, _f32c(c, "c_all"), _f32c(g, "gates").clone())
                for w, dh, c, g in [(w_hh, dh_out, c_all, gates)] + ([second] if second is not None else [])]
        a, b2 = sets[0], (sets[1] if len(sets) > 1 else (None,) * 4)
        capi.check(lib.s2vt_lstm_seq_bwd_x3_persist(T, B, H, _ptr(a[0]), _ptr(b2[0]), _ptr(a[1]), _ptr(b2[1]), int(dh_first),
                                                    _ptr(a[2]), _ptr(b2[2]), _ptr(a[3]), _ptr(b2[3]), int(block), _ptr(ws), n,
                                                    _stream(dev)), "s2vt_lstm_seq_bwd_x3_persist")
        _check_persist_err(ws)
    return sets[0][3] if second is None else (sets[0][3], sets[1][3])


def row_plane_image(rows, k, dev, fill=0, extra_ld=0, extra_rows=0):
    """(image, ld): an int16 blocked 3-plane ROW image for `rows` rows of k elements as split_planes lays it out (row stride
    3 * pad64(k) + extra_ld, extra_rows further rows), every element = fill"""
    ld = 3 * ((k + 63) // 64 * 64) + extra_ld
    return torch.full(((rows + 63) // 64 * 64 + extra_rows, ld), fill, dtype=torch.int16, device=dev), ld


def _f32_inout(t, name):
    """a buffer the call writes into: float32 and contiguous as it stands (a copy would take the results with it)"""
    if _f32c(t, name) is not t:
        raise capi.S2VTHipError("%s is written in place and must be contiguous" % name)
    return t


def _x3_image(img, name):
    if img is None:
        return None, 0
    t, ld = img
    require_hip(t, name)
    if t.dtype != torch.int16 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != ld:
        raise capi.S2VTHipError("%s must be (int16 rows with unit column stride, their row stride)" % name)
    return t, int(ld)


def lstm_seq_fwd_persist_emit(T, B, stash, n_gx, bias, w_hh, hblk=None, no_stash=False, block=0, second=None):
    """lstm_seq_fwd_persist with the fields the train / decode drivers fill in (s2vt_lstm_seq_fwd_x3_persist_emit).  stash
    [T*B, 4H]: the caller's buffer, its first n_gx * B rows the gate input; the activated gates are written into it unless
    no_stash.  hblk = (int16 image, row stride) or None: h_t as the batched GEMMs' row image, written into the caller's tensor
    (row_plane_image).  Returns (h_all, c_all); `second` = (stash, bias, w_hh, hblk) of a layer that shares every launch: then
    a pair of them."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        n = lib.s2vt_lstm_seq_x3_workspace_bytes(T, B, H)
        if n == 0:
            raise capi.S2VTHipError("lstm_seq_fwd_persist_emit: shape B=%d H=%d is not supported on this device" % (B, H))
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)      # (bf16 NaN patterns, as lstm_seq_fwd_persist)
        sets = []
        for s, b, w, im in [(stash, bias, w_hh, hblk)] + ([second] if second is not None else []):
            s = _f32_inout(s, "stash")
            if tuple(s.shape) != (T * B, 4 * H):
                raise capi.S2VTHipError("lstm_seq_fwd_persist_emit: stash must be [T*B, 4H]")
            sets.append((s, b, _f32c(w, "w_hh"), torch.empty(T * B, H, dtype=torch.float32, device=dev),
                         torch.empty(T * B, H, dtype=torch.float32, device=dev)) + _x3_image(im, "hblk"))
        a, b2 = sets[0], (sets[1] if len(sets) > 1 else (None,) * 6 + (0,))
        capi.check(lib.s2vt_lstm_seq_fwd_x3_persist_emit(T, B, H, _ptr(a[0]), _ptr(b2[0]), int(n_gx), _ptr(a[1]), _ptr(b2[1]), _ptr(a[2]),
                                                         _ptr(b2[2]), _ptr(a[3]), _ptr(b2[3]), _ptr(a[4]), _ptr(b2[4]), _ptr(a[5]), a[6],
                                                         _ptr(b2[5]), b2[6], int(bool(no_stash)), int(block), _ptr(ws), n, _stream(dev)),
                   "s2vt_lstm_seq_fwd_x3_persist_emit")
        _check_persist_err(ws)
    outs = [(x[3], x[4]) for x in sets]
    return outs[0] if second is None else tuple(outs)


def lstm_seq_bwd_persist_emit(T, B, w_hh, dh_out, dh_first, c_all, stash_dg, dgp=None, colpart=None, skip_dg=False, block=0, second=None):
    """lstm_seq_bwd_persist with the fields the train driver fills in (s2vt_lstm_seq_bwd_x3_persist_emit), everything written
    into the caller's tensors: stash_dg [T*B, 4H] (activated gates in; fp32 dG out unless skip_dg), dgp = (int16 image, row
    stride) or None: dG_t as the batched GEMMs' row image, colpart [>= T*B/32, 4H] or None: its 32-row column sums.
    `second` = (w_hh, dh_out, c_all, stash_dg, dgp, colpart)."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        n = lib.s2vt_lstm_seq_bwd_x3_workspace_bytes(T, B, H, int(block))
        ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)     # (NaN patterns, as lstm_seq_bwd_persist)
        sets = []
        for w, dh, c, s, im, cp in [(w_hh, dh_out, c_all, stash_dg, dgp, colpart)] + ([second] if second is not None else []):
            s = _f32_inout(s, "stash_dg")
            if tuple(s.shape) != (T * B, 4 * H):
                raise capi.S2VTHipError("lstm_seq_bwd_persist_emit: stash_dg must be [T*B, 4H]")
            if cp is not None:
                cp = _f32_inout(cp, "colpart")
                if cp.dim() != 2 or cp.shape[0] < T * (B // 32) or cp.shape[1] != 4 * H:
                    raise capi.S2VTHipError("lstm_seq_bwd_persist_emit: colpart must be [>= T*B/32, 4H]")
            sets.append((_f32c(w, "w_hh"), dh, _f32c(c, "c_all"), s) + _x3_image(im, "dgp") + (cp,))
        a, b2 = sets[0], (sets[1] if len(sets) > 1 else (None,) * 5 + (0, None))
        capi.check(lib.s2vt_lstm_seq_bwd_x3_persist_emit(T, B, H, _ptr(a[0]), _ptr(b2[0]), _ptr(a[1]), _ptr(b2[1]), int(dh_first),
                                                         _ptr(a[2]), _ptr(b2[2]), _ptr(a[3]), _ptr(b2[3]), _ptr(a[4]), a[5], _ptr(b2[4]),
                                                         b2[5], _ptr(a[6]), _ptr(b2[6]), int(bool(skip_dg)), int(block), _ptr(ws), n,
                                                         _stream(dev)), "s2vt_lstm_seq_bwd_x3_persist_emit")
        _check_persist_err(ws)


# ---------------------------------------------------------------- GRU cell (include/s2vt_hip.h: s2vt_gru_*)
def gru_step_fwd(gx, b_ih, w_hh, b_hh, h_prev, want_stash=False, B=None):
    """One nn.GRU step: gx [B,3H] (x W_ih^T + b_ih) or None (then b_ih alone: a zero input); h_prev [B,H] or None (zero state;
    with neither, `B` gives the batch).  Returns h [B,H] (and the stash [B,4H] = r, z, n, ghn)."""
    lib = capi.load()
    w_hh, b_hh = _f32c(w_hh, "w_hh"), _f32c(b_hh, "b_hh")
    H = w_hh.shape[1]
    B = gx.shape[0] if gx is not None else (h_prev.shape[0] if h_prev is not None else int(B))
    dev = w_hh.device
    with torch.cuda.device(dev):
        h = torch.empty(B, H, dtype=torch.float32, device=dev)
        stash = torch.empty(B, 4 * H, dtype=torch.float32, device=dev) if want_stash else None
        capi.check(lib.s2vt_gru_step_fwd(B, H, _ptr(gx), _ptr(b_ih), _ptr(w_hh), _ptr(b_hh), _ptr(h_prev), _ptr(h), _ptr(stash),
                                         _stream(dev)), "s2vt_gru_step_fwd")
    return (h, stash) if want_stash else h


def gru_step_fwd_token(gx, w_hh, b_hh, h_prev, emb, w_ih, tok=None, tok_packed=None, tok_const=0, out=None, ss=None):
    """One greedy decode step of a GRU word_rnn: gx [B,3H] (vid half of the gate input + b_ih), emb [V,E], w_ih [3H, E+H] (its
    first E columns multiply the embedded word).  Token per row: `tok` int32 [B], else `tok_packed` (the packed argmax words of
    s2vt_decode_step_argmax), else `tok_const`.  Ids outside [0, V) raise IndexError at the next capi.check_async_error().
    `ss` = (targets int64 [B, T], ss_prob, seed, step): a scheduled-sampling step (s2vt_gru_step_fwd_token_ss) - the coin of
    (row, step) picks tok_packed's word or targets[:, step]."""
    lib = capi.load()
    gx, w_hh, b_hh, emb, w_ih = (_f32c(gx, "gx"), _f32c(w_hh, "w_hh"), _f32c(b_hh, "b_hh"), _f32c(emb, "emb"), _f32c(w_ih, "w_ih"))
    B, H = gx.shape[0], w_hh.shape[1]
    V, E = emb.shape
    dev = gx.device
    with torch.cuda.device(dev):
        h = out if out is not None else torch.empty(B, H, dtype=torch.float32, device=dev)
        if ss is not None:
            targets, ss_prob, seed, step = ss
            capi.check(lib.s2vt_gru_step_fwd_token_ss(B, H, E, V, _ptr(gx), _ptr(w_hh), _ptr(b_hh), _ptr(h_prev), _ptr(emb), _ptr(w_ih),
                                                      w_ih.stride(0), _ptr(tok_packed), _ptr(targets), targets.stride(0), float(ss_prob),
                                                      int(seed), int(step), 0, _ptr(h), _stream(dev)), "s2vt_gru_step_fwd_token_ss")
            return h
        capi.check(lib.s2vt_gru_step_fwd_token(B, H, E, V, _ptr(gx), _ptr(w_hh), _ptr(b_hh), _ptr(h_prev), _ptr(emb), _ptr(w_ih),
                                               w_ih.stride(0), _ptr(tok), _ptr(tok_packed), int(tok_const), _ptr(h), _stream(dev)),
                   "s2vt_gru_step_fwd_token")
    return h


def gru_step_bwd(dgh_next, w_hh_t, stash_next, dh_out, stash, h_prev, dh):
    """BPTT of one GRU step; `dh` [B,H] holds dh_{t+1} on entry (ignored at the last step: dgh_next None) and dh_t on exit.
    Returns (dgx, dgh) [B,3H]."""
    lib = capi.load()
    B, H4 = stash.shape
    H = H4 // 4
    dev = stash.device
    with torch.cuda.device(dev):
        dgx = torch.empty(B, 3 * H, dtype=torch.float32, device=dev)
        dgh = torch.empty(B, 3 * H, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_gru_step_bwd(B, H, _ptr(dgh_next), _ptr(w_hh_t), _ptr(stash_next), _ptr(dh_out), _ptr(stash),
                                         _ptr(h_prev), _ptr(dh), _ptr(dgx), _ptr(dgh), _stream(dev)), "s2vt_gru_step_bwd")
    return dgx, dgh


def gru_seq_fwd(T, B, gx, n_gx, b_ih, w_hh, b_hh, want_stash=False):
    """A GRU layer from the zero state; gx [n_gx*B, 3H] time-major, b_ih alone for the later steps.  Returns (h_all [T*B,H],
    stash [T*B,4H] or None)."""
    lib = capi.load()
    w_hh, b_hh = _f32c(w_hh, "w_hh"), _f32c(b_hh, "b_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    if n_gx:
        gx = _f32c(gx, "gx")
    with torch.cuda.device(dev):
        h_all = torch.empty(T * B, H, dtype=torch.float32, device=dev)
        stash = torch.empty(T * B, 4 * H, dtype=torch.float32, device=dev) if want_stash else None
        capi.check(lib.s2vt_gru_seq_fwd(T, B, H, _ptr(gx if n_gx else None), int(n_gx), _ptr(b_ih), _ptr(w_hh), _ptr(b_hh),
                                        _ptr(h_all), _ptr(stash), _stream(dev)), "s2vt_gru_seq_fwd")
    return h_all, stash


def gru_seq_bwd(T, B, w_hh, dh_out, dh_first, h_all, stash):
    """BPTT over a GRU layer (h_all, stash of gru_seq_fwd, left untouched).  Returns (dgx, dgh) [T*B,3H]."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    dev = w_hh.device
    with torch.cuda.device(dev):
        wt = torch.empty(H, 3 * H, dtype=torch.float32, device=dev)
        dh = torch.empty(B, H, dtype=torch.float32, device=dev)
        dgx = torch.empty(T * B, 3 * H, dtype=torch.float32, device=dev)
        dgh = torch.empty(T * B, 3 * H, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_gru_seq_bwd(T, B, H, _ptr(w_hh), _ptr(dh_out), int(dh_first), _ptr(_f32c(h_all, "h_all")),
                                        _ptr(_f32c(stash, "stash")), _ptr(wt), _ptr(dh), _ptr(dgx), _ptr(dgh), _stream(dev)),
                   "s2vt_gru_seq_bwd")
    return dgx, dgh


def tokens_time_major(targets, Lm1, V):
    """int32 [Lm1*B] time-major word ids of targets [B, >=Lm1] (int64); ids outside [0, V) are clamped and raise IndexError at
    the next capi.check_async_error()."""
    lib = capi.load()
    require_hip(targets, "targets")
    if targets.dtype != torch.int64 or targets.stride(1) != 1:
        targets = targets.long().contiguous()
    B = targets.shape[0]
    dev = targets.device
    with torch.cuda.device(dev):
        tok = torch.empty(Lm1 * B, dtype=torch.int32, device=dev)
        capi.check(lib.s2vt_tokens_time_major(B, Lm1, V, _ptr(targets), targets.stride(0), _ptr(tok), _stream(dev)),
                   "s2vt_tokens_time_major")
    return tok


_LAYER_TENSORS = ("w_hh", "w_in", "x_in", "gx", "bias", "h0", "c0", "mask", "emb", "w_e", "h", "c", "stash", "hm", "dh_ext", "dg")


def _chain_struct(layers):
    """capi.LstmLayer array of a chain: each layer a dict of s2vt_lstm_layer fields (tensors for the pointers, contiguous except
    w_in / w_e, whose row stride is taken from the tensor; tok_packed an int64 tensor)"""
    arr = (capi.LstmLayer * len(layers))()
    for s, lay in zip(arr, layers):
        for k in _LAYER_TENSORS:
            t = lay.get(k)
            if t is None:
                continue
            if t.dtype != torch.float32 or t.stride(-1) != 1 or (k not in ("w_in", "w_e") and not t.is_contiguous()):
                raise capi.S2VTHipError("chain layer field %s: float32 rows with unit column stride expected" % k)
            setattr(s, k, t.data_ptr())
        if lay.get("w_in") is not None:
            s.ldw_in = lay["w_in"].stride(0)
        if lay.get("w_e") is not None:
            s.ldw_e = lay["w_e"].stride(0)
        if lay.get("tok_packed") is not None:
            s.tok_packed = lay["tok_packed"].data_ptr()
        for k in ("gx_t0", "n_gx", "E", "V", "tok_const", "dh_t0"):
            setattr(s, k, int(lay.get(k, 0)))
        if lay.get("ss") is not None:        # (targets int64 [B, T], ss_prob, seed, step): a scheduled-sampling token segment
            targets, ss_prob, seed, step = lay["ss"]
            s.ss_targets, s.ss_ld, s.ss_prob, s.ss_seed, s.ss_step, s.ss_row0 = (targets.data_ptr(), targets.stride(0), float(ss_prob),
                                                                                 int(seed), int(step), 0)
    return arr


def lstm_chain_fwd(T, B, H, layers):
    """s2vt_lstm_chain_fwd over `layers` (dicts, see _chain_struct); the output tensors h, c (stash, hm) are the caller's."""
    lib = capi.load()
    dev = layers[0]["w_hh"].device
    arr = _chain_struct(layers)
    with torch.cuda.device(dev):
        capi.check(lib.s2vt_lstm_chain_fwd(T, B, H, len(layers), arr, _stream(dev)), "s2vt_lstm_chain_fwd")


def lstm_chain_bwd(T, B, H, layers):
    """s2vt_lstm_chain_bwd: writes each layer's dg (which may be its stash) from the forward's c / stash and dh_ext."""
    lib = capi.load()
    dev = layers[0]["w_hh"].device
    arr = _chain_struct(layers)
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_lstm_chain_bwd_workspace_bytes(B, H, len(layers))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        capi.check(lib.s2vt_lstm_chain_bwd(T, B, H, len(layers), arr, _ptr(ws), nbytes, _stream(dev)), "s2vt_lstm_chain_bwd")


def _ss_targets(targets):
    require_hip(targets, "targets")
    if targets.dim() != 2:
        raise ValueError("targets must be [B, T], got %s" % (tuple(targets.shape),))
    if targets.dtype != torch.int64 or targets.stride(1) != 1:
        targets = targets.long().contiguous()
    return targets


def ss_mix(draw_tokens, targets, ss_prob, seed, step, row0=0):
    """int64 [B]: one step of the scheduled-sampling rule (s2vt_ss_mix) - draw_tokens[b] where step > 0 and
    coin(row0 + b, step) < ss_prob, targets[b, step] otherwise.  draw_tokens int64 [B], targets int64 [B, T]."""
    lib = capi.load()
    targets = _ss_targets(targets)
    require_hip(draw_tokens, "draw_tokens")
    if draw_tokens.dtype != torch.int64 or tuple(draw_tokens.shape) != (targets.shape[0],):
        raise capi.S2VTHipError("ss_mix: draw_tokens must be int64 [B]")
    draw_tokens = draw_tokens.contiguous()
    B = targets.shape[0]
    if not 0 <= int(step) < targets.shape[1]:
        raise ValueError("ss_mix: step %d outside the %d columns of targets" % (step, targets.shape[1]))
    dev = targets.device
    with torch.cuda.device(dev):
        out = torch.empty(B, dtype=torch.int64, device=dev)
        capi.check(lib.s2vt_ss_mix(_ptr(draw_tokens), _ptr(targets), targets.stride(0), B, float(ss_prob), int(seed), int(step), int(row0),
                                   _ptr(out), _stream(dev)), "s2vt_ss_mix")
    return out


def ss_unpack(packed, targets, ss_prob, seed, want_draws=True):
    """(used, draws or None) int64 [B, T] from the packed arg-max words [T, B] (int64) of a loop of scheduled steps - s2vt_ss_unpack."""
    lib = capi.load()
    targets = _ss_targets(targets)
    T, B = packed.shape
    dev = targets.device
    with torch.cuda.device(dev):
        used = torch.empty(B, T, dtype=torch.int64, device=dev)
        draws = torch.empty(B, T, dtype=torch.int64, device=dev) if want_draws else None
        capi.check(lib.s2vt_ss_unpack(_ptr(packed), T, B, _ptr(targets), targets.stride(0), float(ss_prob), int(seed), _ptr(used),
                                      _ptr(draws), _stream(dev)), "s2vt_ss_unpack")
    return used, draws


def cider_rewards(table, clip_rows, ids, sos_ix, eos_ix):
    """fp64 [B]: CIDEr of the id rows `ids` (int64 [B, T], unit column stride) against the references of the clips `clip_rows`
    (int32 [B], rows of the table) - s2vt_cider_rewards.  `table` is a capi.CiderTable of device pointers that the caller keeps
    alive (self_critical.DeviceCiderRewarder).  A token outside [0, 65535] raises IndexError at the next capi.check_async_error()."""
    lib = capi.load()
    require_hip(ids, "ids")
    require_hip(clip_rows, "clip_rows")
    if ids.dim() != 2 or clip_rows.dtype != torch.int32 or clip_rows.numel() != ids.shape[0]:
        raise capi.S2VTHipError("cider_rewards: ids [B, T] and clip_rows int32 [B] expected")
    if ids.dtype != torch.int64 or ids.stride(1) != 1:
        ids = ids.long().contiguous()
    B, T = ids.shape
    if T > capi.CIDER_MAX_T:
        raise ValueError("cider_rewards: rows of %d ids; the kernel's n-gram list in LDS holds rows of up to %d" % (T, capi.CIDER_MAX_T))
    dev = ids.device
    with torch.cuda.device(dev):
        out = torch.empty(B, dtype=torch.float64, device=dev)
        capi.check(lib.s2vt_cider_rewards(ctypes.byref(table), _ptr(clip_rows.contiguous()), _ptr(ids), B, T, ids.stride(0), int(sos_ix),
                                          int(eos_ix), _ptr(out), _stream(dev)), "s2vt_cider_rewards")
    return out


def cider_consensus(table, ids, sos_ix, eos_ix, valid=None):
    """(best int64 [B], utility fp64 [B, K]) on the device, no synchronisation: consensus (MBR) selection among the K candidate rows of
    each clip under CIDEr-D with the table's idf - s2vt_cider_consensus (the definition is in include/s2vt_hip.h).  ids HIP int64
    [B, K, T]: a last stride other than 1 means a contiguous copy, a row-strided view (one stride from row b*K + k to the next) is
    taken as it is.  valid: bool / uint8 [B, K] on the device or None (all valid); a candidate that is not valid gets -inf and is
    nobody's reference.  A token outside [0, 65535] raises IndexError at the next capi.check_async_error()."""
    lib = capi.load()
    require_hip(ids, "ids")
    if ids.dim() != 3 or ids.shape[0] < 1:
        raise capi.S2VTHipError("cider_consensus: ids [B, K, T] expected, got %s" % (tuple(ids.shape),))
    B, K, T = ids.shape
    if not 1 <= K <= capi.CONSENSUS_MAX_K:
        raise ValueError("cider_consensus: %d candidates per clip; 1..%d are supported" % (K, capi.CONSENSUS_MAX_K))
    if not 1 <= T <= capi.CIDER_MAX_T:
        raise ValueError("cider_consensus: rows of %d ids; the kernel's n-gram list in LDS holds rows of 1..%d" % (T, capi.CIDER_MAX_T))
    if ids.dtype != torch.int64 or ids.stride(2) != 1 or ids.stride(1) < T or ids.stride(0) != K * ids.stride(1):
        ids = ids.long().contiguous()
    dev = ids.device
    if valid is not None:
        require_hip(valid, "valid")
        if tuple(valid.shape) != (B, K) or valid.dtype not in (torch.bool, torch.uint8):
            raise capi.S2VTHipError("cider_consensus: valid must be bool / uint8 [B, K] = [%d, %d]" % (B, K))
        valid = valid.to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_cider_consensus_workspace_bytes(B, K, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        utility = torch.empty(B, K, dtype=torch.float64, device=dev)
        best = torch.empty(B, dtype=torch.int32, device=dev)
        capi.check(lib.s2vt_cider_consensus(ctypes.byref(table), _ptr(ids), B, K, T, ids.stride(1), int(sos_ix), int(eos_ix), _ptr(valid),
                                            _ptr(utility), _ptr(best), _ptr(ws), nbytes, _stream(dev)), "s2vt_cider_consensus")
    return best.long(), utility


def _finite_weights(what, w_cider, w_bleu):
    w_cider, w_bleu = float(w_cider), float(w_bleu)
    if not (math.isfinite(w_cider) and math.isfinite(w_bleu)):
        raise ValueError("%s: the weights must be finite, got %r and %r" % (what, w_cider, w_bleu))
    return w_cider, w_bleu


def mixed_rewards(table, bleu_table, clip_rows, ids, sos_ix, eos_ix, w_cider, w_bleu, return_parts=False):
    """fp64 [B]: w_cider * CIDEr + w_bleu * sentence BLEU-4 of the id rows `ids` against the references of the clips `clip_rows` -
    s2vt_mixed_rewards, arguments as cider_rewards plus the capi.BleuTable of the same clips (self_critical.DeviceMixedRewarder
    keeps both alive).  return_parts: (mix, cider, bleu), the CIDEr part with cider_rewards' bits.  Weights that are not finite:
    ValueError before the library is called."""
    lib = capi.load()
    w_cider, w_bleu = _finite_weights("mixed_rewards", w_cider, w_bleu)
    require_hip(ids, "ids")
    require_hip(clip_rows, "clip_rows")
    if ids.dim() != 2 or clip_rows.dtype != torch.int32 or clip_rows.numel() != ids.shape[0]:
        raise capi.S2VTHipError("mixed_rewards: ids [B, T] and clip_rows int32 [B] expected")
    if ids.dtype != torch.int64 or ids.stride(1) != 1:
        ids = ids.long().contiguous()
    B, T = ids.shape
    if T > capi.CIDER_MAX_T:
        raise ValueError("mixed_rewards: rows of %d ids; the kernel's n-gram list in LDS holds rows of up to %d" % (T, capi.CIDER_MAX_T))
    dev = ids.device
    with torch.cuda.device(dev):
        out = torch.empty(B, dtype=torch.float64, device=dev)
        cider = torch.empty(B, dtype=torch.float64, device=dev) if return_parts else None
        bleu = torch.empty(B, dtype=torch.float64, device=dev) if return_parts else None
        capi.check(lib.s2vt_mixed_rewards(ctypes.byref(table), ctypes.byref(bleu_table), _ptr(clip_rows.contiguous()), _ptr(ids), B, T,
                                          ids.stride(0), int(sos_ix), int(eos_ix), w_cider, w_bleu, _ptr(out), _ptr(cider), _ptr(bleu),
                                          _stream(dev)), "s2vt_mixed_rewards")
    return (out, cider, bleu) if return_parts else out


def mixed_consensus(table, bleu_table, ids, sos_ix, eos_ix, w_cider, w_bleu, valid=None):
    """cider_consensus under the utility w_cider * CIDEr-D + w_bleu * sentence BLEU-4 (each against the clip's other valid candidates) -
    s2vt_mixed_consensus; same arguments, shapes and results, plus the capi.BleuTable (its bp alone is read) and the two weights
    (not finite: ValueError before the library is called)."""
    lib = capi.load()
    w_cider, w_bleu = _finite_weights("mixed_consensus", w_cider, w_bleu)
    require_hip(ids, "ids")
    if ids.dim() != 3 or ids.shape[0] < 1:
        raise capi.S2VTHipError("mixed_consensus: ids [B, K, T] expected, got %s" % (tuple(ids.shape),))
    B, K, T = ids.shape
    if not 1 <= K <= capi.CONSENSUS_MAX_K:
        raise ValueError("mixed_consensus: %d candidates per clip; 1..%d are supported" % (K, capi.CONSENSUS_MAX_K))
    if not 1 <= T <= capi.CIDER_MAX_T:
        raise ValueError("mixed_consensus: rows of %d ids; the kernel's n-gram list in LDS holds rows of 1..%d" % (T, capi.CIDER_MAX_T))
    if ids.dtype != torch.int64 or ids.stride(2) != 1 or ids.stride(1) < T or ids.stride(0) != K * ids.stride(1):
        ids = ids.long().contiguous()
    dev = ids.device
    if valid is not None:
        require_hip(valid, "valid")
        if tuple(valid.shape) != (B, K) or valid.dtype not in (torch.bool, torch.uint8):
            raise capi.S2VTHipError("mixed_consensus: valid must be bool / uint8 [B, K] = [%d, %d]" % (B, K))
        valid = valid.to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_mixed_consensus_workspace_bytes(B, K, T)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        utility = torch.empty(B, K, dtype=torch.float64, device=dev)
        best = torch.empty(B, dtype=torch.int32, device=dev)
        capi.check(lib.s2vt_mixed_consensus(ctypes.byref(table), ctypes.byref(bleu_table), _ptr(ids), B, K, T, ids.stride(1), int(sos_ix),
                                            int(eos_ix), _ptr(valid), w_cider, w_bleu, _ptr(utility), _ptr(best), _ptr(ws), nbytes,
                                            _stream(dev)), "s2vt_mixed_consensus")
    return best.long(), utility


def sc_weights(sampled, r_sample, r_greedy, sos_ix, eos_ix):
    """(caps int64 [B, T+1] = <sos> || sampled, weight fp32 [B, T+1] = self_critical.advantage_weights(sampled, r_sample - r_greedy,
    eos_ix)) from sampled ids int64 [B, T] and the two fp64 reward vectors [B], all on the device - s2vt_sc_weights."""
    lib = capi.load()
    require_hip(sampled, "sampled")
    if sampled.dim() != 2 or sampled.dtype != torch.int64:
        raise capi.S2VTHipError("sc_weights: sampled must be int64 [B, T]")
    sampled = sampled.contiguous()
    B, T = sampled.shape
    for name, r in (("r_sample", r_sample), ("r_greedy", r_greedy)):
        require_hip(r, name)
        if r.dtype != torch.float64 or tuple(r.shape) != (B,) or not r.is_contiguous():
            raise capi.S2VTHipError("sc_weights: %s must be a contiguous float64 [B]" % name)
    dev = sampled.device
    with torch.cuda.device(dev):
        caps = torch.empty(B, T + 1, dtype=torch.int64, device=dev)
        weight = torch.empty(B, T + 1, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_sc_weights(_ptr(sampled), _ptr(r_sample), _ptr(r_greedy), B, T, int(sos_ix), int(eos_ix), _ptr(caps),
                                       _ptr(weight), _stream(dev)), "s2vt_sc_weights")
    return caps, weight


def sc_weights_group(sampled, r_sample, r_greedy, K, sos_ix, eos_ix, return_baseline=False):
    """(caps int64 [B*K, T+1], weight fp32 [B*K, T+1][, baseline fp64 [B*K]]) for K sampled captions per clip, rows r = b*K + k -
    s2vt_sc_weights_group.  sampled int64 [B*K, T], r_sample fp64 [B*K].  r_greedy None: each row is baselined with the mean reward
    of its clip's other K - 1 rows (self_critical.group_advantages; K >= 2); r_greedy fp64 [B]: with its clip's greedy reward."""
    lib = capi.load()
    K = int(K)
    if K < 1 or (r_greedy is None and K < 2):
        raise ValueError("sc_weights_group: the mean of the other K - 1 rewards needs K >= 2 (K >= 1 with r_greedy), got K = %d" % K)
    require_hip(sampled, "sampled")
    if sampled.dim() != 2 or sampled.dtype != torch.int64 or sampled.shape[0] % K != 0 or sampled.shape[0] == 0:
        raise capi.S2VTHipError("sc_weights_group: sampled must be int64 [B*K, T]")
    sampled = sampled.contiguous()
    R, T = sampled.shape
    B = R // K
    for name, r, n in (("r_sample", r_sample, R), ("r_greedy", r_greedy, B)):
        if r is None:
            continue
        require_hip(r, name)
        if r.dtype != torch.float64 or tuple(r.shape) != (n,) or not r.is_contiguous():
            raise capi.S2VTHipError("sc_weights_group: %s must be a contiguous float64 [%d]" % (name, n))
    dev = sampled.device
    with torch.cuda.device(dev):
        caps = torch.empty(R, T + 1, dtype=torch.int64, device=dev)
        weight = torch.empty(R, T + 1, dtype=torch.float32, device=dev)
        baseline = torch.empty(R, dtype=torch.float64, device=dev) if return_baseline else None
        capi.check(lib.s2vt_sc_weights_group(_ptr(sampled), _ptr(r_sample), _ptr(r_greedy), B, K, T, int(sos_ix), int(eos_ix), _ptr(caps),
                                             _ptr(weight), _ptr(baseline), _stream(dev)), "s2vt_sc_weights_group")
    return (caps, weight, baseline) if return_baseline else (caps, weight)


def sc_weights_swor(sampled, logprob, kappa, r_sample, r_greedy, K, sos_ix, eos_ix, return_extras=False):
    """(caps int64 [B*K, T+1], weight fp32 [B*K, T+1][, coef fp64 [B*K], baseline fp64 [B]]) for the K pairwise distinct captions per
    clip of S2VT.sample_distinct, rows r = b*K + k - s2vt_sc_weights_swor (include/s2vt_hip.h "without-replacement weights";
    self_critical.swor_advantages).  sampled int64 [B*K, T], logprob fp32 [B*K] and kappa fp32 [B] as the search returns them,
    r_sample fp64 [B*K].  r_greedy None: the estimator's own baseline N / W; r_greedy fp64 [B]: the clip's greedy reward.
    2 <= K <= 8."""
    lib = capi.load()
    K = int(K)
    if not 2 <= K <= capi.SWOR_MAX_K:
        raise ValueError("sc_weights_swor: K distinct captions per clip with K in [2, %d], got K = %d" % (capi.SWOR_MAX_K, K))
    require_hip(sampled, "sampled")
    if sampled.dim() != 2 or sampled.dtype != torch.int64 or sampled.shape[0] % K != 0 or sampled.shape[0] == 0 or sampled.shape[1] == 0:
        raise capi.S2VTHipError("sc_weights_swor: sampled must be int64 [B*K, T]")
    sampled = sampled.contiguous()
    R, T = sampled.shape
    B = R // K
    for name, r, n, dt in (("logprob", logprob, R, torch.float32), ("kappa", kappa, B, torch.float32),
                           ("r_sample", r_sample, R, torch.float64), ("r_greedy", r_greedy, B, torch.float64)):
        if r is None and name == "r_greedy":
            continue
        require_hip(r, name)
        if r.dtype != dt or tuple(r.shape) != (n,) or not r.is_contiguous():
            raise capi.S2VTHipError("sc_weights_swor: %s must be a contiguous %s [%d]" % (name, str(dt).replace("torch.", ""), n))
    dev = sampled.device
    with torch.cuda.device(dev):
        caps = torch.empty(R, T + 1, dtype=torch.int64, device=dev)
        weight = torch.empty(R, T + 1, dtype=torch.float32, device=dev)
        coef = torch.empty(R, dtype=torch.float64, device=dev) if return_extras else None
        baseline = torch.empty(B, dtype=torch.float64, device=dev) if return_extras else None
        capi.check(lib.s2vt_sc_weights_swor(_ptr(sampled), _ptr(logprob), _ptr(kappa), _ptr(r_sample), _ptr(r_greedy), B, K, T,
                                            int(sos_ix), int(eos_ix), _ptr(caps), _ptr(weight), _ptr(coef), _ptr(baseline), _stream(dev)),
                   "s2vt_sc_weights_swor")
    return (caps, weight, coef, baseline) if return_extras else (caps, weight)


# ---------------------------------------------------------------- per-op test support (include/s2vt_hip.h: the backward's
# gather / scatter / reorder pieces).  Matrices here are float32 ROWS: unit column stride, the row stride is the tensor's own
# (a column block of a wider tensor is passed as the view it is).
def _f32rows(t, name):
    require_hip(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
        raise capi.S2VTHipError("%s must be float32 rows with unit column stride, got %s %s" % (name, t.dtype, tuple(t.stride())))
    return t


def _rowmap(m, name):
    """(idx pointer, inner, outer) of a row map: None (identity), an int32 tensor (gather) or a pair (inner, outer)"""
    if m is None:
        return ctypes.c_void_p(0), 0, 0
    if isinstance(m, torch.Tensor):
        require_hip(m, name)
        if m.dtype != torch.int32 or m.dim() != 1 or not m.is_contiguous():
            raise capi.S2VTHipError("%s: a gather index must be a contiguous int32 vector" % name)
        return _ptr(m), 0, 0
    inner, outer = m
    return ctypes.c_void_p(0), int(inner), int(outer)


def gemm_mapped(a, b, out, a_kmajor=True, b_kmajor=True, amap=None, bmap=None, cmap=None, bias=None, accumulate=False,
                splitk_ws=None, splitk_cap=0):
    """out (+)= op(a)·op(b) (+bias) through row maps on the stored rows of a, b and out (s2vt_gemm_f32_mapped).  A map is None,
    an int32 index tensor (gather; rows m / n only) or (inner, outer).  splitk_ws: fp32 scratch that allows split-K, in at most
    splitk_cap slices (0: the launcher's own choice)."""
    lib = capi.load()
    a, b, out = _f32rows(a, "a"), _f32rows(b, "b"), _f32rows(out, "out")
    K = a.shape[1] if a_kmajor else a.shape[0]
    # (a gather stands on m / n rows: the index then counts them; on k rows the library refuses it)
    M = amap.numel() if isinstance(amap, torch.Tensor) and a_kmajor else (a.shape[0] if a_kmajor else a.shape[1])
    N = bmap.numel() if isinstance(bmap, torch.Tensor) and b_kmajor else (b.shape[0] if b_kmajor else b.shape[1])
    if (b.shape[1] if b_kmajor else b.shape[0]) != K:
        raise ValueError("gemm_mapped: inner dims differ")
    if out.shape[1] != N or (not isinstance(cmap, torch.Tensor) and out.shape[0] != M):
        raise ValueError("gemm_mapped: out is %s for M=%d N=%d" % (tuple(out.shape), M, N))
    (ai, ain, aout), (bi, bin_, bout), (ci, cin, cout) = _rowmap(amap, "amap"), _rowmap(bmap, "bmap"), _rowmap(cmap, "cmap")
    dev = a.device
    with torch.cuda.device(dev):
        capi.check(lib.s2vt_gemm_f32_mapped(int(a_kmajor), int(b_kmajor), M, N, K, _ptr(a), a.stride(0), ai, ain, aout, _ptr(b),
                                            b.stride(0), bi, bin_, bout, _ptr(out), out.stride(0), ci, cin, cout, _ptr(bias),
                                            int(accumulate), _ptr(splitk_ws), splitk_ws.numel() if splitk_ws is not None else 0,
                                            int(splitk_cap), _stream(dev)), "s2vt_gemm_f32_mapped")
    return out


def embedding_grad(d_rows, tok, V, out=None, ws=None):
    """d_emb [V, E] = index_add of d_rows [rows, E] by tok (int32 [rows]) in a fixed order (s2vt_embedding_grad).  `out` / `ws`
    (int32 scratch of at least s2vt_embedding_grad_ws_ints) may be handed in pre-filled: every row of out is written."""
    lib = capi.load()
    d_rows = _f32c(d_rows, "d_rows")
    rows, E = d_rows.shape
    require_hip(tok, "tok")
    if tok.dtype != torch.int32 or tuple(tok.shape) != (rows,) or not tok.is_contiguous():
        raise capi.S2VTHipError("embedding_grad: tok must be a contiguous int32 [rows]")
    dev = d_rows.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(V, E, dtype=torch.float32, device=dev)
        if ws is None:
            ws = torch.empty(lib.s2vt_embedding_grad_ws_ints(rows, V), dtype=torch.int32, device=dev)
        capi.check(lib.s2vt_embedding_grad(_ptr(d_rows) if rows else None, rows, E, _ptr(tok) if rows else None, V, _ptr(out),
                                           _ptr(ws), ws.numel(), _stream(dev)), "s2vt_embedding_grad")
    return out


def gather_rows(src, idx):
    """out [rows, cols] = src[idx] (s2vt_gather_rows); src float32 rows, idx int32 [rows]."""
    lib = capi.load()
    src = _f32rows(src, "src")
    iptr, _, _ = _rowmap(idx, "idx")
    dev = src.device
    with torch.cuda.device(dev):
        out = torch.empty(idx.numel(), src.shape[1], dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_gather_rows(_ptr(src), src.stride(0), iptr, idx.numel(), src.shape[1], _ptr(out), _stream(dev)),
                   "s2vt_gather_rows")
    return out


def pick_logprob(logits, target):
    """(lp [rows], flag int32 [1]): lp[r] = min(log_softmax(logits[r])[target[r]], 0) (s2vt_pick_logprob, the head kernel of
    mode='score').  logits float32 [rows, V] with a unit column stride (any row stride >= V), target int32 [rows]; a target outside
    [0, V) sets flag and reads the nearest valid column."""
    lib = capi.load()
    logits = _f32rows(logits, "logits")
    require_hip(target, "target")
    rows, V = logits.shape
    if target.dtype != torch.int32 or target.numel() != rows or not target.is_contiguous():
        raise ValueError("target must be a contiguous int32 tensor of %d ids" % rows)
    dev = logits.device
    with torch.cuda.device(dev):
        lp = torch.empty(rows, dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        capi.check(lib.s2vt_pick_logprob(_ptr(logits), logits.stride(0), rows, V, _ptr(target), _ptr(lp), _ptr(flag), _stream(dev)),
                   "s2vt_pick_logprob")
    return lp, flag


def transpose(x):
    """x^T as a new contiguous tensor (s2vt_transpose_f32)."""
    lib = capi.load()
    x = _f32c(x, "x")
    rows, cols = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        out = torch.empty(cols, rows, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_transpose_f32(_ptr(x), rows, cols, _ptr(out), _stream(dev)), "s2vt_transpose_f32")
    return out


def colsum(x, out=None, accumulate=False):
    """(out [cols] (+)= x.sum(0), partial [ceil(rows / 64), cols]): the fixed-order column sum (s2vt_colsum) and its per-chunk
    partial sums."""
    lib = capi.load()
    x = _f32rows(x, "x")
    rows, cols = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        ws = torch.empty(lib.s2vt_colsum_ws_floats(rows, cols), dtype=torch.float32, device=dev)
        if out is None:
            out = torch.zeros(cols, dtype=torch.float32, device=dev) if accumulate else torch.empty(cols, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_colsum(_ptr(x), rows, cols, x.stride(0), _ptr(ws), ws.numel(), _ptr(out), int(accumulate), _stream(dev)),
                   "s2vt_colsum")
    return out, ws.view(-1, cols)


def colsum_finish(partial, out=None, accumulate=False):
    """out [cols] (+)= the fixed-order sum of the rows of partial [nchunks, cols] (s2vt_colsum_finish)."""
    lib = capi.load()
    partial = _f32c(partial, "partial")
    nchunks, cols = partial.shape
    dev = partial.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(cols, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_colsum_finish(_ptr(partial), nchunks, cols, _ptr(out), int(accumulate), _stream(dev)), "s2vt_colsum_finish")
    return out


def split_planes_dual(x, nplanes=3, rowmap=None, want_r=True, want_t=False, want_colpart=False, ce=None):
    """s2vt_split_planes_dual on x (float32 rows): a dict with any of 'r' / 't' (images as split_planes(.) / split_planes(.,
    transpose=True) return them: zero-filled int16 [ceil64(operand rows), nplanes * kpad]) and 'colpart' [ceil(rows / 64), cols].
    rowmap: None, an int32 index (then rows = its length) or (inner, outer).  ce = dict(lse, target, Lm1, gout[, alpha]): x holds
    logits and the mean-CE gradient is what is split (alpha=True: the power-of-two form; 'alpha' is returned as a 1-element tensor)."""
    lib = capi.load()
    x = _f32rows(x, "x")
    cols = x.shape[1]
    rows = rowmap.numel() if isinstance(rowmap, torch.Tensor) else x.shape[0]
    idx, inner, outer = _rowmap(rowmap, "rowmap")
    pad = lambda n: (n + 63) // 64 * 64
    dev = x.device
    res = {}
    with torch.cuda.device(dev):
        kr, kt = pad(cols), pad(rows)
        if want_r:
            res["r"] = torch.zeros(pad(rows), nplanes * kr, dtype=torch.int16, device=dev)
        if want_t:
            res["t"] = torch.zeros(pad(cols), nplanes * kt, dtype=torch.int16, device=dev)
        if want_colpart:
            res["colpart"] = torch.empty((rows + 63) // 64, cols, dtype=torch.float32, device=dev)
        lse = target = gout = None
        ldt = Lm1 = 0
        if ce is not None:
            lse, target, gout, Lm1 = ce["lse"], ce["target"], ce["gout"], int(ce["Lm1"])
            ldt = target.stride(0)
            if ce.get("alpha"):
                res["alpha"] = torch.empty(1, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_split_planes_dual(nplanes, _ptr(x), x.stride(0), idx, inner, outer, rows, cols, _ptr(res.get("r")),
                                              nplanes * kr, kr, _ptr(res.get("t")), nplanes * kt, kt, _ptr(res.get("colpart")),
                                              _ptr(lse), _ptr(target), ldt, Lm1, _ptr(gout), _ptr(res.get("alpha")), _stream(dev)),
                   "s2vt_split_planes_dual")
    return res


# ---------------------------------------------------------------- per-op test support (include/s2vt_hip.h: the decode step's
# kernel forms).  Outputs may be handed in (pre-filled: the tests look at what a launch leaves alone); every tensor is passed as
# the view it is - c_prev may start anywhere in its storage.
def _i32vec(t, n, name):
    if t is None:
        return None
    require_hip(t, name)
    if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise capi.S2VTHipError("%s must be a contiguous int32 [%d]" % (name, n))
    return t


def _rows_of(t, cols, name):
    """float32 [rows, >= cols] with unit column stride and contiguous rows (row stride = cols): the natural width"""
    if t is None:
        return None
    require_hip(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != cols or t.stride(1) != 1 or t.stride(0) != cols:
        raise capi.S2VTHipError("%s must be float32 [rows, %d] with row stride %d, got %s %s" % (name, cols, cols, tuple(t.shape),
                                                                                                  tuple(t.stride())))
    return t


def h_plane_image(B, H, dev, fill=0, extra_ld=0):
    """(image, ld, kpad): an int16 blocked 3-plane image for B rows of H units as split_planes lays it out, every element = fill"""
    kpad = (H + 63) // 64 * 64
    ld = 3 * kpad + extra_ld
    return torch.full(((B + 63) // 64 * 64, ld), fill, dtype=torch.int16, device=dev), ld, kpad


def _table_step_common(B, H, gx, gx_idx, gtab, tok, c_prev, h_out, c_out, stash, want_stash, h_planes, dev):
    gx, c_prev = _rows_of(gx, 4 * H, "gx"), _rows_of(c_prev, H, "c_prev")
    gx_idx, tok = _i32vec(gx_idx, B, "gx_idx"), _i32vec(tok, B, "tok")
    V, ldtab = 0, 0
    if gtab is not None:
        require_hip(gtab, "gtab")
        if gtab.dtype != torch.float32 or gtab.dim() != 2 or gtab.stride(1) != 1:
            raise capi.S2VTHipError("gtab must be float32 rows with unit column stride")
        V, ldtab = gtab.shape[0], gtab.stride(0)
    h_out = h_out if h_out is not None else torch.empty(B, H, dtype=torch.float32, device=dev)
    c_out = c_out if c_out is not None else torch.empty(B, H, dtype=torch.float32, device=dev)
    if stash is None and want_stash:
        stash = torch.empty(B, 4 * H, dtype=torch.float32, device=dev)
    img, ldhp, hp_rows = (h_planes[0], h_planes[1], h_planes[0].shape[0]) if h_planes is not None else (None, 0, 0)
    return gx, gx_idx, gtab, V, ldtab, tok, c_prev, _rows_of(h_out, H, "h_out"), _rows_of(c_out, H, "c_out"), \
        _rows_of(stash, 4 * H, "stash"), img, ldhp, hp_rows


def lstm_step_fwd_table(w_hh, h_prev, c_prev, gx=None, gx_idx=None, bias=None, gtab=None, tok=None, tok_packed=None, tok_const=0,
                        h_out=None, c_out=None, stash=None, want_stash=False, h_planes=None):
    """One word_rnn step in the plane-path form (s2vt_lstm_step_fwd_table): gates = gx[gx_idx] (or bias) + gtab[token] +
    h_prev·w_hh^T.  h_planes = (image, ld, kpad) as split_planes / h_plane_image return it: h_t is also written there as three
    bf16 planes.  Returns (h, c, stash or None)."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    B = gx_idx.numel() if gx_idx is not None else (gx.shape[0] if gx is not None else h_prev.shape[0])
    dev = w_hh.device
    with torch.cuda.device(dev):
        gx, gx_idx, gtab, V, ldtab, tok, c_prev, h_out, c_out, stash, img, ldhp, hp_rows = _table_step_common(
            B, H, gx, gx_idx, gtab, tok, c_prev, h_out, c_out, stash, want_stash, h_planes, dev)
        capi.check(lib.s2vt_lstm_step_fwd_table(B, H, V, _ptr(gx), _ptr(gx_idx), _ptr(bias), _ptr(gtab), ldtab, _ptr(tok), _ptr(tok_packed),
                                                int(tok_const), _ptr(w_hh), _ptr(_rows_of(h_prev, H, "h_prev")), _ptr(c_prev), _ptr(h_out),
                                                _ptr(c_out), _ptr(stash), _ptr(img), ldhp, hp_rows, None, 0, 0, _stream(dev)),
                   "s2vt_lstm_step_fwd_table")
    return h_out, c_out, stash


def lstm_step_contract(w_hh, h_prev, z=None):
    """z [B, >= 4H] = h_prev·w_hh^T, the contraction-only form of the step kernel (s2vt_lstm_step_fwd_table, contract_only = 1);
    `z` may be handed in (any row stride >= 4H): only its first 4H columns of the B rows are written."""
    lib = capi.load()
    w_hh = _f32c(w_hh, "w_hh")
    H = w_hh.shape[1]
    h_prev = _rows_of(h_prev, H, "h_prev")
    B = h_prev.shape[0]
    dev = w_hh.device
    with torch.cuda.device(dev):
        if z is None:
            z = torch.empty(B, 4 * H, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_lstm_step_fwd_table(B, H, 0, None, None, None, None, 0, None, None, 0, _ptr(w_hh), _ptr(h_prev), None, None,
                                                None, None, None, 0, 0, _ptr(z), z.stride(0), 1, _stream(dev)),
                   "s2vt_lstm_step_fwd_table")
    return z


def lstm_cell_pointwise(z, H, c_prev, gx=None, gx_idx=None, bias=None, gtab=None, tok=None, tok_packed=None, tok_const=0, h_out=None,
                        c_out=None, stash=None, want_stash=False, h_planes=None, B=None):
    """The cell update of a step whose contraction z [>= B, >= 4H] ran as its own launch (s2vt_lstm_cell_pointwise); the other
    arguments as lstm_step_fwd_table.  Returns (h, c, stash or None)."""
    lib = capi.load()
    require_hip(z, "z")
    if z.dtype != torch.float32 or z.dim() != 2 or z.stride(1) != 1:
        raise capi.S2VTHipError("z must be float32 rows with unit column stride")
    if B is None:
        B = gx_idx.numel() if gx_idx is not None else (gx.shape[0] if gx is not None else z.shape[0])
    dev = z.device
    with torch.cuda.device(dev):
        gx, gx_idx, gtab, V, ldtab, tok, c_prev, h_out, c_out, stash, img, ldhp, hp_rows = _table_step_common(
            B, H, gx, gx_idx, gtab, tok, c_prev, h_out, c_out, stash, want_stash, h_planes, dev)
        capi.check(lib.s2vt_lstm_cell_pointwise(B, H, V, _ptr(gx), _ptr(gx_idx), _ptr(bias), _ptr(gtab), ldtab, _ptr(tok), _ptr(tok_packed),
                                                int(tok_const), _ptr(z), z.stride(0), _ptr(c_prev), _ptr(h_out), _ptr(c_out), _ptr(stash),
                                                _ptr(img), ldhp, hp_rows, _stream(dev)), "s2vt_lstm_cell_pointwise")
    return h_out, c_out, stash


def argmax_x3_planes(pw, ph, B, V, bias=None, packed=None, pw2=None, M2=0, z=None, with_logits=True, sample=None):
    """The plane-path arg-max launch on caller-made images (s2vt_argmax_x3_planes).  pw / ph / pw2 = (image, ld, kpad) of
    out_linear.weight [V, H], h_t [B, H] and the second weight [M2, H] as split_planes returns them.  packed: int64 [B] (zeroed
    if not given).  z: float32 [rows, ldz] to receive h_t·W2^T in its first M2 columns of the first B rows.  with_logits = False:
    the z role alone.  sample = (temperature, seed, step, row0): a draw instead of the arg-max.  Returns (packed, z)."""
    lib = capi.load()
    (w, ldw, kw), (hp, ldh, kh) = pw, ph
    w2, ldw2, kw2 = pw2 if pw2 is not None else (None, 0, 0)
    dev = w.device
    temperature, seed, step, row0 = sample if sample is not None else (1.0, 0, 0, 0)
    with torch.cuda.device(dev):
        if packed is None:
            packed = torch.zeros(B, dtype=torch.int64, device=dev)
        if z is None and M2 > 0:
            z = torch.empty(B, (M2 + 3) // 4 * 4, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_argmax_x3_planes(B, V, kw, _ptr(w), ldw, w.shape[0], _ptr(hp), ldh, kh, hp.shape[0], _ptr(bias), _ptr(packed),
                                             _ptr(w2), ldw2, kw2, w2.shape[0] if w2 is not None else 0, int(M2), _ptr(z),
                                             z.stride(0) if z is not None else 0, int(bool(with_logits)), int(sample is not None),
                                             float(temperature), int(seed), int(step), int(row0), _stream(dev)), "s2vt_argmax_x3_planes")
    return packed, z
