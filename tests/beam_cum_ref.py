"""Restatement of S2VT.forward(mode='beam') for the tests (a helper, not a conftest): the cumulative-score beam search written
from its definition, with NO early stop, so a stopping rule that changed an output would show.

Per sample, W = beam_width, D = max_depth: live starts as one empty hypothesis (S = 0, last word <sos>, the encoder state of
mode='beam_search'), pool empty.  For t = 1..D: candidates (j, v) of every live slot j (in slot order) and token v score
S_j + lp_j[v]; the min(W, count) best by (S descending, j ascending, v ascending) are walked in that order - v == <eos> enters the
pool with score S / t**alpha, anything else is the next live slot; live empty: done; t == D: every live hypothesis enters the pool,
in order, with S / D**alpha and no <eos>.  The pool is ordered by (score descending, insertion ascending); the answer is its
first n_best entries.

  search_fp64   the whole path in torch fp64 on the CPU (model arithmetic from oracle/s2vt_oracle.py), with the two decision gaps
  PolicyF32     the policy alone over given per-depth top-20 arrays, in numpy float32 with the device's adds, power table and
                division - what csrc/beam_policy.hip must reproduce exactly
"""
import numpy as np
import torch

from oracle import s2vt_oracle as oracle

ROBUST_GAP = 2e-4      # the greedy fixtures' per-step margin 1e-5 x the at most 15 terms a cumulative score sums here, rounded up

# name: (B, L, F, H, E, V), out_scale, seed, W, D   (out_linear.bias[eos] += 0.5: hypotheses finish at mixed depths)
CASES = {
    "tiny": ((8, 8, 64, 32, 24, 50), 4.0, 31, 3, 10),
    "tiny5": ((8, 8, 64, 32, 24, 50), 4.0, 32, 5, 12),
    "mid64": ((64, 24, 512, 256, 256, 1000), 8.0, 42, 5, 12),
}
SOS, EOS, ALPHA = 3, 4, 0.7


def case_inputs(name):
    """(state_dict, feats, W, D) of a case - the recipe of the issue, from the package's synth module"""
    from s2vt_video_caption_amd import synth
    (B, L, F, H, E, V), out_scale, seed, W, D = CASES[name]
    sd = synth.make_state_dict(V, F, H, E, seed=seed, out_scale=out_scale)
    sd["out_linear.bias"][EOS] += 0.5
    feats = synth.make_batch(B, L, F, V, seed=1234 + seed)[0]
    return sd, feats, W, D


_SEARCHES = {}


def case_search(name):
    """search_fp64 of a case with its own W, D and ALPHA - computed once per process, shared by the tests, never modified"""
    if name not in _SEARCHES:
        sd, feats, W, D = case_inputs(name)
        _SEARCHES[name] = search_fp64(sd, feats, W, D)
    return _SEARCHES[name]


def _stable_desc(x):
    """indices of x by (value descending, index ascending)"""
    return torch.sort(x, descending=True, stable=True).indices


def search_fp64(params, feats, W, D, alpha=ALPHA, sos=SOS, eos=EOS):
    """-> list over samples of dict(ids=[token lists, best first, W of them], scores=[...], cand_gap, pool_gap):
    cand_gap = the smallest gap between the W-th and (W+1)-th of all live*V candidates over the depths,
    pool_gap = the smallest gap between adjacent scores among the best W+1 pool entries."""
    p = {k: v.double() for k, v in params.items()}
    feats = feats.double()
    B, L, _ = feats.shape
    x1 = feats @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)                       # vid_rnn over the L real frames only
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    vid = []                                                           # vid_rnn stepped with zero input, shared by a sample's slots
    for t in range(D):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        vid.append(h1)
    V = p["out_linear.weight"].shape[0]
    out = []
    for b in range(B):
        toks, S, last = [[]], torch.zeros(1, dtype=torch.float64), torch.tensor([sos])
        wh, wc = h2[b:b + 1], c2[b:b + 1]
        pool, cand_gap = [], float("inf")                              # pool entries: (score, tokens), in insertion order
        for t in range(1, D + 1):
            nl = len(toks)
            wh, wc = oracle._word_step(p, p["embedding.weight"][last], vid[t - 1][b:b + 1].expand(nl, -1), wh, wc)
            lp = torch.log_softmax(wh @ p["out_linear.weight"].t() + p["out_linear.bias"], dim=1)
            cand = (S[:, None] + lp).reshape(-1)                       # index j * V + v: (j ascending, v ascending)
            order = _stable_desc(cand)
            m = min(W, cand.numel())
            if cand.numel() > m:
                cand_gap = min(cand_gap, float(cand[order[m - 1]] - cand[order[m]]))
            keep_j, keep_v, ntoks, nS = [], [], [], []
            for c in order[:m].tolist():
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
            wh, wc = wh[keep_j], wc[keep_j]
        rank = sorted(range(len(pool)), key=lambda i: -pool[i][0])     # (stable: insertion order among equal scores)
        sc = [pool[i][0] for i in rank]
        assert len(sc) >= W
        pool_gap = min([sc[i] - sc[i + 1] for i in range(min(W, len(sc) - 1))], default=float("inf"))
        out.append(dict(ids=[pool[i][1] for i in rank[:W]], scores=sc[:W], cand_gap=cand_gap, pool_gap=pool_gap))
    return out


def robust(res):
    """bool per sample: both gaps >= ROBUST_GAP"""
    return np.array([r["cand_gap"] >= ROBUST_GAP and r["pool_gap"] >= ROBUST_GAP for r in res])


def greedy_fp64(params, feats, D, sos=SOS, eos=EOS):
    """the first D greedy words per sample (fp64), cut behind the first <eos>; and each step's top-2 margin [B, L-1]"""
    ids, margins = oracle.greedy_decode(params, feats, sos_ix=sos, dtype=torch.float64, return_margins=True)
    rows = []
    for r in ids[:, :D].tolist():
        rows.append(r[:r.index(eos) + 1] if eos in r else r)
    return rows, margins.numpy()


def pow_table(D, alpha):
    """fp32(len ** alpha) as the device evaluates it: double pow, then fp32"""
    return np.array([np.float32(pow(float(l), alpha)) if l > 0 else np.float32(1) for l in range(D + 1)], dtype=np.float32)


class PolicyF32(object):
    """The policy alone on the row protocol of the library, one call per depth as the device runs it.  rows() = int array [2][B*W]
    (row_state, row_tok as the device writes them: slot j of sample b in row b*W+j, 0 in unused slots and for finished samples);
    step(top_ix, top_lp) consumes the [B*W][20] arrays of the next depth; done = bool [B]; result() = the n-best as (ids [B][W][D]
    padded with eos, lens [B][W], scores fp32 [B][W])."""

    def __init__(self, B, W, D, alpha, sos=SOS, eos=EOS):
        self.B, self.W, self.D, self.eos, self.t = B, W, D, eos, 0
        self.pw = pow_table(D, alpha)
        self.live = [[(np.float32(0), [], b, sos)] for b in range(B)]       # (S, tokens, state row, last word)
        self.pool = [[] for _ in range(B)]
        self.done = np.zeros(B, dtype=bool)

    def rows(self):
        out = np.zeros((2, self.B * self.W), dtype=np.int32)
        for b in range(self.B):
            for j, (_, _, row, tok) in enumerate(self.live[b]):
                out[0, b * self.W + j], out[1, b * self.W + j] = row, tok
        return out

    def step(self, top_ix, top_lp):
        self.t += 1
        t, W, D, pw = self.t, self.W, self.D, self.pw
        ix, lp = np.asarray(top_ix), np.minimum(np.asarray(top_lp, dtype=np.float32), np.float32(0))
        for b in range(self.B):
            if self.done[b]:
                continue
            S = np.concatenate([np.float32(s) + lp[b * W + j] for j, (s, _, _, _) in enumerate(self.live[b])]).astype(np.float32)
            order = np.argsort(-S, kind="stable")[:min(W, S.size)]      # (S descending, c = j*20+f ascending; -0 == +0)
            nxt = []
            for c in order.tolist():
                j, f = divmod(c, 20)
                v = int(ix[b * W + j, f])
                tk = self.live[b][j][1] + [v]
                if v == self.eos:
                    self.pool[b].append((np.float32(S[c]) / pw[t], tk))
                else:
                    nxt.append((np.float32(S[c]), tk, b * W + j, v))
            if t == D:
                self.pool[b].extend((s / pw[D], tk) for s, tk, _, _ in nxt)
                nxt = []
            self.live[b] = nxt
            self.done[b] = not nxt

    def may_stop(self):
        """bool [B]: the samples the device MAY freeze now although they are not done - pool full and pool[W-1].score >=
        live[0].S / D**alpha.  Reported, never applied: the restatement runs every sample to its end."""
        out = np.zeros(self.B, dtype=bool)
        for b in range(self.B):
            sc = sorted((float(s) for s, _ in self.pool[b]), reverse=True)
            if not self.done[b] and len(sc) >= self.W:
                out[b] = np.float32(sc[self.W - 1]) >= self.live[b][0][0] / self.pw[self.D]
        return out

    def result(self):
        B, W, D = self.B, self.W, self.D
        assert self.done.all()
        ids = np.full((B, W, D), self.eos, dtype=np.int64)
        lens = np.zeros((B, W), dtype=np.int64)
        scores = np.zeros((B, W), dtype=np.float32)
        for b in range(B):
            rank = sorted(range(len(self.pool[b])), key=lambda i: -float(self.pool[b][i][0]))[:W]      # (stable: insertion order)
            assert len(rank) == W
            for k, i in enumerate(rank):
                s, tk = self.pool[b][i]
                ids[b, k, :len(tk)] = tk
                lens[b, k] = len(tk)
                scores[b, k] = s
        return ids, lens, scores
