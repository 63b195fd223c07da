"""Restatement of S2VT.beam_diverse for the tests (a helper, not a conftest): diverse (group) beam search written from its definition
(include/s2vt_hip.h "diverse beam"), with NO early stop, so a stopping rule that changed an output would show.

Per sample, W = beam_width slots, G groups of Wg = W / G slots, lambda >= 0, D = max_depth: every group has a live list that starts
as one empty hypothesis (S = 0, last word <sos>, the encoder state of mode='beam') and a pool.  For t = 1..D: cnt[v] = 0 for every
word; the groups run in order; a group whose live list is empty is closed, skipped, and adds nothing to cnt.  Candidate (j, v) of
live slot j has the score s = S_j + lp_j[v] and the selection key a = s - lambda * cnt[v], cnt as the earlier groups left it.  The
min(Wg, count) best by (a descending, j ascending, v ascending) are walked in that order: every one does cnt[v] += 1; v == <eos>
enters the group's pool with s / t**alpha (the unpenalised sum), anything else is the group's next live slot with S = s.  At t == D
every live hypothesis enters its group's pool with S / D**alpha, no <eos> appended.  A pool is ordered by (score descending,
insertion ascending); the answer is each group's first n_best entries.  With a constraint spec lp_j is log_softmax of the row edited
by sampling.constrain_logits with slot j's own words as history, as in tests/beam_constrained_ref.py.

  search_fp64    the whole path in torch fp64 on the CPU (model arithmetic from oracle/s2vt_oracle.py), with the two decision gaps
  PolicyDivF32   the policy alone over given per-depth top-20 arrays, in numpy float32 with the device's operations - what
                 csrc/beam_policy.hip must reproduce exactly
"""
import numpy as np
import torch

import beam_cum_ref as ref
from oracle import s2vt_oracle as oracle

SOS, EOS, ALPHA, ROBUST_GAP = ref.SOS, ref.EOS, ref.ALPHA, ref.ROBUST_GAP


def search_fp64(params, feats, W, G, lam, D, spec=None, alpha=ALPHA, sos=SOS, eos=EOS):
    """-> list over samples of dict(ids=[per group its Wg token lists, best first], scores=[per group ...], cand_gap, pool_gap,
    changed): cand_gap = the smallest gap in a at any group's selection boundary (the Wg-th against the (Wg+1)-th of the group's
    live*V candidates), pool_gap = the smallest gap between adjacent scores among the best Wg+1 entries of any group's pool,
    changed = whether the penalty changed some group's selection at some depth (against the selection by s alone).
    spec: a sampling.ConstraintSpec or None."""
    from s2vt_video_caption_amd import sampling
    assert W % G == 0 and 1 <= G <= W
    Wg = W // G
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
        # per group: token lists, sums, last words, word_rnn state rows; pool entries (score, tokens) in insertion order
        grp = [dict(toks=[[]], S=[0.0], last=[sos], wh=h2[b:b + 1], wc=c2[b:b + 1], pool=[]) for _ in range(G)]
        cand_gap, changed = float("inf"), False
        for t in range(1, D + 1):
            open_g = [g for g in grp if g["toks"]]
            if not open_g:
                break
            # one word step and one projection for the live slots of all open groups (every slot holds t-1 words)
            n_all = sum(len(g["toks"]) for g in open_g)
            last = torch.tensor([v for g in open_g for v in g["last"]])
            wh, wc = oracle._word_step(p, p["embedding.weight"][last], vid[t - 1][b:b + 1].expand(n_all, -1),
                                       torch.cat([g["wh"] for g in open_g]), torch.cat([g["wc"] for g in open_g]))
            x = wh @ p["out_linear.weight"].t() + p["out_linear.bias"]
            if spec is not None:
                hist = np.asarray([tk for g in open_g for tk in g["toks"]], dtype=np.int64).reshape(n_all, t - 1)
                x = torch.from_numpy(sampling.constrain_logits(x.numpy(), hist, t - 1, spec))
            lp_all = torch.log_softmax(x, dim=1)
            cnt = torch.zeros(V, dtype=torch.float64)
            o = 0
            for g in open_g:
                nl = len(g["toks"])
                lp, gwh, gwc = lp_all[o:o + nl], wh[o:o + nl], wc[o:o + nl]
                o += nl
                s = (torch.tensor(g["S"], dtype=torch.float64)[:, None] + lp).reshape(-1)      # index j * V + v
                a = (s.view(nl, V) - lam * cnt[None, :]).reshape(-1)
                order = ref._stable_desc(a)
                m = min(Wg, a.numel())
                assert bool(torch.isfinite(a[order[m]]))               # (a banned candidate is never at the decision boundary)
                cand_gap = min(cand_gap, float(a[order[m - 1]] - a[order[m]]))
                changed = changed or order[:m].tolist() != ref._stable_desc(s)[:m].tolist()
                keep_j, ntoks, nS, nlast = [], [], [], []
                for c in order[:m].tolist():
                    j, v = divmod(c, V)
                    cnt[v] += 1
                    if v == eos:
                        g["pool"].append((float(s[c]) / float(t) ** alpha, g["toks"][j] + [eos]))
                    else:
                        keep_j.append(j); ntoks.append(g["toks"][j] + [v]); nS.append(float(s[c])); nlast.append(v)
                if t == D:
                    g["pool"].extend((sc / float(D) ** alpha, tk) for sc, tk in zip(nS, ntoks))
                    keep_j, ntoks, nS, nlast = [], [], [], []
                g["toks"], g["S"], g["last"], g["wh"], g["wc"] = ntoks, nS, nlast, gwh[keep_j], gwc[keep_j]
        ids, scores, pool_gap = [], [], float("inf")
        for g in grp:
            pool = g["pool"]
            rank = sorted(range(len(pool)), key=lambda i: -pool[i][0])     # (stable: insertion order among equal scores)
            sc = [pool[i][0] for i in rank]
            assert len(sc) >= Wg
            pool_gap = min([pool_gap] + [sc[i] - sc[i + 1] for i in range(min(Wg, len(sc) - 1))])
            ids.append([pool[i][1] for i in rank[:Wg]])
            scores.append(sc[:Wg])
        out.append(dict(ids=ids, scores=scores, cand_gap=cand_gap, pool_gap=pool_gap, changed=changed))
    return out


_SEARCHES = {}


def case_search(name, D, G, Wg, lam, spec_args=None):
    """search_fp64 on the inputs of a beam_cum_ref case (the case's own W and D are not used) - computed once per process, shared by
    the tests, never modified.  spec_args: a beam_constrained_ref spec tuple or None."""
    key = (name, D, G, Wg, lam, spec_args)
    if key not in _SEARCHES:
        sd, feats, _, _ = ref.case_inputs(name)
        spec = None
        if spec_args is not None:
            import beam_constrained_ref as cref
            spec = cref.spec_of(spec_args, ref.CASES[name][0][5])
        _SEARCHES[key] = search_fp64(sd, feats, G * Wg, G, lam, D, spec)
    return _SEARCHES[key]


robust = ref.robust


class PolicyDivF32(object):
    """The policy alone on the row protocol of the library, one call per depth as the device runs it, in the device's fp32
    operations: s = S + min(lp, 0) with -0 folded to +0; a = s where cnt == 0, else s - (fp32(lambda) * fp32(cnt)), the product and
    the difference each rounded to fp32; pool scores s / fp32(t ** alpha).  rows() = int array [2][B*W] (row_state, row_tok: slot
    g*Wg + i of sample b in row b*W + g*Wg + i, 0 in unused slots); step(top_ix, top_lp) consumes the [B*W][20] arrays of the next
    depth; settled() = bool [B][G]; histories() = the live slots' words; result() = every group's pool, best first, as (ids
    [B][G][Wg][D] padded with eos, lens [B][G][Wg], scores fp32 [B][G][Wg]).  No early stop: every sample runs to its end."""

    def __init__(self, B, W, G, D, alpha, lam, sos=SOS, eos=EOS):
        assert W % G == 0
        self.B, self.W, self.G, self.Wg, self.D, self.eos, self.t = B, W, G, W // G, D, eos, 0
        self.lam = np.float32(lam)
        self.pw = ref.pow_table(D, alpha)
        self.live = [[[(np.float32(0), [], b, sos)] for _ in range(G)] for b in range(B)]     # (S, tokens, state row, last word)
        self.pool = [[[] for _ in range(G)] for _ in range(B)]

    def rows(self):
        out = np.zeros((2, self.B * self.W), dtype=np.int32)
        for b in range(self.B):
            for g in range(self.G):
                for i, (_, _, row, tok) in enumerate(self.live[b][g]):
                    r = b * self.W + g * self.Wg + i
                    out[0, r], out[1, r] = row, tok
        return out

    def histories(self):
        """int array [B*W][D] and bool [B*W]: every live slot's words after the depths stepped so far, and which rows are live"""
        h = np.zeros((self.B * self.W, self.D), dtype=np.int32)
        live = np.zeros(self.B * self.W, dtype=bool)
        for b in range(self.B):
            for g in range(self.G):
                for i, (_, tk, _, _) in enumerate(self.live[b][g]):
                    r = b * self.W + g * self.Wg + i
                    h[r, :len(tk)] = tk
                    live[r] = True
        return h, live

    def step(self, top_ix, top_lp):
        self.t += 1
        t, W, Wg, D, pw = self.t, self.W, self.Wg, self.D, self.pw
        ix, lp = np.asarray(top_ix), np.minimum(np.asarray(top_lp, dtype=np.float32), np.float32(0))
        for b in range(self.B):
            cnt = {}
            for g in range(self.G):
                live = self.live[b][g]
                if not live:
                    continue                                            # closed: skipped, nothing added to cnt
                base = b * W + g * Wg
                S = np.concatenate([np.float32(s) + lp[base + j] for j, (s, _, _, _) in enumerate(live)]).astype(np.float32)
                S = np.where(S == 0, np.float32(0), S).astype(np.float32)
                n = np.array([cnt.get(int(v), 0) for j in range(len(live)) for v in ix[base + j]], dtype=np.float32)
                with np.errstate(invalid="ignore", over="ignore"):
                    pen = (self.lam * n).astype(np.float32)
                    a = np.where(n == 0, S, (S - pen).astype(np.float32)).astype(np.float32)
                order = np.argsort(-a, kind="stable")[:min(Wg, a.size)]        # (a descending, c = j*20+f ascending; -0 == +0)
                nxt = []
                for c in order.tolist():
                    j, f = divmod(c, 20)
                    v = int(ix[base + j, f])
                    cnt[v] = cnt.get(v, 0) + 1
                    tk = live[j][1] + [v]
                    if v == self.eos:
                        self.pool[b][g].append((np.float32(S[c]) / pw[t], tk))
                    else:
                        nxt.append((np.float32(S[c]), tk, base + j, v))
                if t == D:
                    self.pool[b][g].extend((s / pw[D], tk) for s, tk, _, _ in nxt)
                    nxt = []
                self.live[b][g] = nxt

    def settled(self):
        """bool [B][G]: the group is closed, or its pool holds Wg entries and pool[Wg-1].score >= max_j(live S_j) / D**alpha - its
        pool cannot change any more.  The device freezes a sample once all of its groups are settled."""
        out = np.zeros((self.B, self.G), dtype=bool)
        for b in range(self.B):
            for g in range(self.G):
                live = self.live[b][g]
                if not live:
                    out[b, g] = True
                    continue
                sc = sorted((float(s) for s, _ in self.pool[b][g]), reverse=True)
                if len(sc) >= self.Wg:
                    top = np.float32(max(float(s) for s, _, _, _ in live))
                    out[b, g] = np.float32(sc[self.Wg - 1]) >= top / self.pw[self.D]
        return out

    def result(self):
        B, G, Wg, D = self.B, self.G, self.Wg, self.D
        assert all(not l for per in self.live for l in per)
        ids = np.full((B, G, Wg, D), self.eos, dtype=np.int64)
        lens = np.zeros((B, G, Wg), dtype=np.int64)
        scores = np.zeros((B, G, Wg), dtype=np.float32)
        for b in range(B):
            for g in range(G):
                pool = self.pool[b][g]
                rank = sorted(range(len(pool)), key=lambda i: -float(pool[i][0]))[:Wg]      # (stable: insertion order)
                assert len(rank) == Wg
                for k, i in enumerate(rank):
                    s, tk = pool[i]
                    ids[b, g, k, :len(tk)] = tk
                    lens[b, g, k] = len(tk)
                    scores[b, g, k] = s
        return ids, lens, scores
