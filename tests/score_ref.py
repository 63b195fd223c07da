"""Restatement of S2VT.forward(mode='score') for the tests (a helper, not a conftest), in torch fp64 on the CPU.

A caption row c[0..T-1] is <sos>, words, <eos>, padding.  n = 1 + the position of the first <eos> in c[1:] (T-1 where there is
none); lp[j] = min(log_softmax(z_j)[c[j+1]], 0) for j < n and 0 behind, z_j = row j of the mode='train' logits for the inputs
c[:-1] (no dropout); score = sum(lp[:n]) / n**alpha.

  scores_fp64       the definition on oracle.forward_train + log_softmax + gather
  scores_stepwise   a second formulation: encode once, then a step-by-step decode with oracle.lstm_cell / _word_step
  make_captions     the captions the tests score: random words, <eos> at mixed positions, one row without <eos>
"""
import torch

from oracle import s2vt_oracle as oracle

SOS, EOS = 3, 4


def _as3(captions):
    return captions[:, None, :] if captions.dim() == 2 else captions


def lengths_of(captions, eos=EOS):
    """n int64 [B, K]: tokens scored per caption, the first <eos> included"""
    c = _as3(captions)
    T = c.shape[-1]
    hit = c[..., 1:] == eos
    first = torch.where(hit.any(-1), hit.float().argmax(-1) + 1, torch.full(hit.shape[:-1], T - 1, dtype=torch.long))
    return first.long()


def scores_fp64(params, feats, captions, eos=EOS, alpha=0.0):
    """-> dict(scores [B, K], sums [B, K], lengths int64 [B, K], token_lp [B, K, T-1]) in fp64; [B, T] captions count as K = 1"""
    c = _as3(captions).long()
    B, K, T = c.shape
    L = feats.shape[1]
    n = lengths_of(c, eos)
    lps = []
    for k in range(K):
        inp = torch.full((B, L - 1), eos, dtype=torch.long)          # (causal: what is fed behind T-2 changes nothing in front)
        inp[:, :T - 1] = c[:, k, :-1]
        logits = oracle.forward_train(params, feats, inp, dtype=torch.float64)[:, :T - 1]
        lp = torch.log_softmax(logits, dim=-1).gather(2, c[:, k, 1:, None])[..., 0]
        lps.append(lp.clamp(max=0.0))
    lp = torch.stack(lps, dim=1)                                       # [B, K, T-1]
    keep = torch.arange(T - 1)[None, None, :] < n[..., None]
    lp = torch.where(keep, lp, torch.zeros_like(lp))
    sums = lp.sum(-1)
    return dict(scores=sums / n.double() ** alpha, sums=sums, lengths=n, token_lp=lp)


def scores_stepwise(params, feats, captions, eos=EOS, alpha=0.0):
    """the same numbers by another road: the encoder of the beam searches (vid_rnn over the L frames, word_rnn with a zero
    embedding), vid_rnn stepped on with no input, one word step per caption token, log_softmax of that step alone"""
    p = {k: v.double() for k, v in params.items()}
    feats = feats.double()
    c = _as3(captions).long()
    B, K, T = c.shape
    L = feats.shape[1]
    x1 = feats @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    n = lengths_of(c, eos)
    lp = torch.zeros(B, K, T - 1, dtype=torch.float64)
    wh = [h2.clone() for _ in range(K)]
    wc = [c2.clone() for _ in range(K)]
    for j in range(T - 1):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        for k in range(K):
            wh[k], wc[k] = oracle._word_step(p, p["embedding.weight"][c[:, k, j]], h1, wh[k], wc[k])
            row = torch.log_softmax(wh[k] @ p["out_linear.weight"].t() + p["out_linear.bias"], dim=1)
            lp[:, k, j] = row[torch.arange(B), c[:, k, j + 1]].clamp(max=0.0)
    for b in range(B):
        for k in range(K):
            lp[b, k, int(n[b, k]):] = 0.0
    sums = lp.sum(-1)
    return dict(scores=sums / n.double() ** alpha, sums=sums, lengths=n, token_lp=lp)


def make_captions(B, K, T, V, seed, min_scored=5, max_scored=12, sos=SOS, eos=EOS):
    """int64 [B, K, T]: <sos>, n-1 random words (ids >= 5), <eos>, then random valid ids as padding (they must not matter),
    n drawn from [min_scored, min(max_scored, T-1)]; caption (0, 0) has no <eos> at all (n = T-1)."""
    g = torch.Generator().manual_seed(seed)
    hi = min(max_scored, T - 1)
    lo = min(min_scored, hi)
    caps = torch.randint(5, V, (B, K, T), generator=g)
    caps[..., 0] = sos
    n = torch.randint(lo, hi + 1, (B, K), generator=g)
    for b in range(B):
        for k in range(K):
            caps[b, k, int(n[b, k])] = eos
    caps[0, 0, 1:] = torch.randint(5, V, (T - 1,), generator=g)
    return caps


_REFS = {}
KMAX = 5


def case_reference(name, K, T, caption_seed):
    """(captions [B, K, T], scores_fp64 at alpha = 0) of a beam_cum_ref case: the first K of KMAX candidates per clip, computed once
    per process for all KMAX, shared by the tests, never modified"""
    import beam_cum_ref as ref
    assert 1 <= K <= KMAX
    key = (name, T, caption_seed)
    if key not in _REFS:
        sd, feats, _, _ = ref.case_inputs(name)
        caps = make_captions(feats.shape[0], KMAX, T, ref.CASES[name][0][5], caption_seed)
        _REFS[key] = (caps, scores_fp64(sd, feats, caps, ref.EOS, 0.0))
    caps, r = _REFS[key]
    return caps[:, :K], {k: v[:, :K] for k, v in r.items()}
