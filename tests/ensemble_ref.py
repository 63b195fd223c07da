"""Restatement of the ensemble beam search for the tests (a helper, not a conftest): include/s2vt_hip.h "ensemble beam" - the
log of the weighted arithmetic mean of M members' word distributions, and mode='beam''s search over it.

  combine64     c[rows, V] in numpy fp64: logsumexp_m(log_softmax(x_m) + log w_m)
  combine_f32   the definition in numpy float32, operation by operation as csrc/ensemble.hip runs it: lse_m in the order of the
                256-thread row kernels (thread strips in ascending index, wave butterflies, (w0 + w1) + (w2 + w3)), a_m = (x_m -
                lse_m) + lw_m, amax, amax + log(sum_m exp(a_m - amax)) with m ascending; -inf where every member is -inf
  search_fp64   beam_cum_ref.search_fp64 with every member's encoder and word step and combine64's rule as the step's log-probs;
                the same two decision gaps
  head_case / head_want   the fixtures of the head tests and what the head must return on them
"""
import numpy as np
import torch

import beam_cum_ref as cum
from oracle import s2vt_oracle as oracle

F32 = np.float32
HEAD_GAP = 1e-4          # a row is checked by id where the adjacent fp64 gaps among its best 21 values are all at least this
HEAD_TOL = 3.2e-5        # top_lp against fp64: twice what the project allows top20_logprob
WEIGHTS = {1: [1.0], 2: None, 3: [0.5, 0.3, 0.2], 4: None, 8: None}       # (None: uniform)


def norm_weights(w, M):
    w = np.ones(M) if w is None else np.asarray(w, dtype=np.float64)
    assert w.shape == (M,) and (w > 0).all() and np.isfinite(w).all()
    return w / w.sum()


def combine64(x, w=None):
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[0]
    lw = np.log(norm_weights(w, M))
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = x.max(axis=2, keepdims=True)
        a = x - (mx + np.log(np.exp(x - mx).sum(axis=2, keepdims=True))) + lw[:, None, None]
        am = a.max(axis=0)
        c = am + np.log(np.exp(a - am).sum(axis=0))
    return np.where(np.isneginf(am), -np.inf, c)


def lse_f32(x):
    """log-sum-exp of the rows x[rows, V] (float32) in the order of top20_logprob_row"""
    x = np.asarray(x, dtype=F32)
    rows, V = x.shape
    mx = x.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp((x - mx).astype(F32)).astype(F32)
    n = (V + 255) // 256
    e = np.concatenate([e, np.zeros((rows, n * 256 - V), dtype=F32)], axis=1).reshape(rows, n, 256)
    # thread tid sums its elements tid + 256 j in ascending j; a pad adds nothing (the kernel skips it: the same sum)
    s = np.zeros((rows, 256), dtype=F32)
    for j in range(n):
        s = (s + e[:, j]).astype(F32)
    s = s.reshape(rows, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, :, lane ^ off]).astype(F32)
    tot = ((s[:, 0, 0] + s[:, 1, 0]).astype(F32) + (s[:, 2, 0] + s[:, 3, 0]).astype(F32)).astype(F32)
    return (mx[:, 0] + np.log(tot).astype(F32)).astype(F32)


def combine_f32(x, w=None):
    x = np.asarray(x, dtype=F32)
    M = x.shape[0]
    lw = np.log(norm_weights(w, M)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.stack([((x[m] - lse_f32(x[m])[:, None]).astype(F32) + lw[m]).astype(F32) for m in range(M)])
        am = a.max(axis=0)
        s = np.zeros_like(am)
        for m in range(M):
            s = (s + np.exp((a[m] - am).astype(F32)).astype(F32)).astype(F32)
        c = (am + np.log(s).astype(F32)).astype(F32)
    return np.where(np.isneginf(am), F32(-np.inf), c).astype(F32)


def head_case(V, rows, M, shift=0):
    """(x float32 [M, rows, V], weights) of the head tests"""
    x = (3.0 * np.random.RandomState(3000 + V + rows + M + shift).randn(M, rows, V)).astype(F32)
    return x, WEIGHTS[M]


def top20_of(c):
    """of c[rows, V] (fp64): (ids [rows, 20] ascending, their values, bool [rows]: the adjacent gaps among the best 21 are all >=
    HEAD_GAP) - ties -> the lower id"""
    c = np.asarray(c, dtype=np.float64)
    order = np.argsort(-c, axis=1, kind="stable")[:, :21]
    best = np.take_along_axis(c, order, axis=1)
    with np.errstate(invalid="ignore"):
        ok = (best[:, :-1] - best[:, 1:] >= HEAD_GAP).all(axis=1)
    ids = np.sort(order[:, :20], axis=1)
    return ids, np.take_along_axis(c, ids, axis=1), ok


def head_want(x, w=None):
    return top20_of(combine64(x, w))


# ---------------------------------------------------------------------------------------------------------------- the whole path
# name: (beam_cum_ref case, M, weights); members: the case's recipe with seed + 100 * m
ENS_CASES = {
    "tiny": ("tiny", 2, None),
    "tiny5": ("tiny5", 3, [0.5, 0.3, 0.2]),
    "mid64": ("mid64", 3, None),
}
MIXED_H = (32, 48)          # the further case: two members of different dim_hid on the tiny dims
MIXED_SEED = 31


def member_dicts(name):
    """the members' state dicts, the features, weights, W, D of a whole-path case ("mixed": the members of different dim_hid)"""
    from s2vt_video_caption_amd import synth
    if name == "mixed":
        (B, L, F, _, E, V), out_scale, _, W, D = cum.CASES["tiny"]
        sds = [synth.make_state_dict(V, F, H, E, seed=MIXED_SEED + 100 * m, out_scale=out_scale) for m, H in enumerate(MIXED_H)]
        feats = synth.make_batch(B, L, F, V, seed=1234 + MIXED_SEED)[0]
        w = None
    else:
        base, M, w = ENS_CASES[name]
        (B, L, F, H, E, V), out_scale, seed, W, D = cum.CASES[base]
        sds = [synth.make_state_dict(V, F, H, E, seed=seed + 100 * m, out_scale=out_scale) for m in range(M)]
        feats = cum.case_inputs(base)[1]
    for sd in sds:
        sd["out_linear.bias"][cum.EOS] += 0.5
    return sds, feats, w, W, D


def member_dims(name):
    """[(B, L, F, H, E, V) per member]"""
    if name == "mixed":
        B, L, F, _, E, V = cum.CASES["tiny"][0]
        return [(B, L, F, H, E, V) for H in MIXED_H]
    base, M, _ = ENS_CASES[name]
    return [cum.CASES[base][0]] * M


_SEARCHES = {}


def case_search(name):
    """search_fp64 of a case - computed once per process, shared by the tests, never modified"""
    if name not in _SEARCHES:
        sds, feats, w, W, D = member_dicts(name)
        _SEARCHES[name] = search_fp64(sds, w, feats, W, D)
    return _SEARCHES[name]


def _encode(p, feats, D):
    """a member's start states and its vid_rnn outputs of the D zero-input decode steps (beam_cum_ref.search_fp64's front)"""
    B, L, _ = feats.shape
    x1 = feats @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    vid = []
    for t in range(D):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        vid.append(h1)
    return h2, c2, vid


def search_fp64(param_dicts, w, feats, W, D, alpha=cum.ALPHA, sos=cum.SOS, eos=cum.EOS):
    """beam_cum_ref.search_fp64 over the ensemble: the same walk, the same outputs (ids, scores, cand_gap, pool_gap per sample);
    the step's log-probs are logsumexp_m(log_softmax_m + log w_m)"""
    ps = [{k: v.double() for k, v in sd.items()} for sd in param_dicts]
    M = len(ps)
    lw = torch.from_numpy(np.log(norm_weights(w, M)))
    feats = feats.double()
    B = feats.shape[0]
    enc = [_encode(p, feats, D) for p in ps]
    V = ps[0]["out_linear.weight"].shape[0]
    out = []
    for b in range(B):
        toks, S, last = [[]], torch.zeros(1, dtype=torch.float64), torch.tensor([sos])
        wh = [e[0][b:b + 1] for e in enc]
        wc = [e[1][b:b + 1] for e in enc]
        pool, cand_gap = [], float("inf")
        for t in range(1, D + 1):
            nl = len(toks)
            lps = []
            for m, p in enumerate(ps):
                wh[m], wc[m] = oracle._word_step(p, p["embedding.weight"][last], enc[m][2][t - 1][b:b + 1].expand(nl, -1), wh[m], wc[m])
                lps.append(torch.log_softmax(wh[m] @ p["out_linear.weight"].t() + p["out_linear.bias"], dim=1) + lw[m])
            lp = torch.logsumexp(torch.stack(lps), dim=0)
            cand = (S[:, None] + lp).reshape(-1)
            order = cum._stable_desc(cand)
            m_keep = min(W, cand.numel())
            if cand.numel() > m_keep:
                cand_gap = min(cand_gap, float(cand[order[m_keep - 1]] - cand[order[m_keep]]))
            keep_j, keep_v, ntoks, nS = [], [], [], []
            for c in order[:m_keep].tolist():
                j, v = divmod(c, V)
                if v == eos:
                    pool.append((float(cand[c]) / float(t) ** alpha, toks[j] + [eos]))
                else:
                    keep_j.append(j); keep_v.append(v); ntoks.append(toks[j] + [v]); nS.append(float(cand[c]))
            if not ntoks:
                break
            if t == D:
                pool.extend((s / float(D) ** alpha, tk) for s, tk in zip(nS, ntoks))
                break
            toks, S, last = ntoks, torch.tensor(nS, dtype=torch.float64), torch.tensor(keep_v)
            wh = [h[keep_j] for h in wh]
            wc = [c_[keep_j] for c_ in wc]
        rank = sorted(range(len(pool)), key=lambda i: -pool[i][0])
        sc = [pool[i][0] for i in rank]
        assert len(sc) >= W
        pool_gap = min([sc[i] - sc[i + 1] for i in range(min(W, len(sc) - 1))], default=float("inf"))
        out.append(dict(ids=[pool[i][1] for i in rank[:W]], scores=sc[:W], cand_gap=cand_gap, pool_gap=pool_gap))
    return out
