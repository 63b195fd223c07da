"""Restatement of S2VT.sample_distinct for the tests (a helper, not a conftest): stochastic beam search (Kool, van Hoof, Welling,
ICML 2019) written from its definition (include/s2vt_hip.h "stochastic beam") in numpy.

Per clip b, W = n_samples slots (empty / live / finished) carrying phi (the sum of the words' log-probs), G (the perturbed score), the
words and a length.  Start: slot 0 live with phi = 0, G = 0, <sos>; kappa = -inf.  For t = 1..D every live slot j gets its row's
lp = log_softmax(logits * inv_t) and g = lp + gumbel_noise(seed, t - 1, row b * W + j); its children in (g descending, v ascending)
order are f = 0, 1, ...; child f has phi' = phi_j + lp and G~ = cond_gumbel(G_j, g[0], g[f]); a finished slot is one candidate with
its own G; candidate index c = j * 20 + f; the min(W, count) best by (G~ descending, c ascending) become the slots in that order;
kappa = max(kappa, best unselected G~).  After depth D the live slots stay as unfinished samples of length D.

  cond_gumbel   the child-score transform, float64
  head_ref      the fan-out head of one depth in float64: per row the 20 best words by g, in order, with lp and g
  PolicyF64     the policy alone over given per-depth top_ix / top_lp / top_g: phi summed in float32 with the device's add, everything
                else float64 - what csrc/sbs_policy.hip must reproduce; NO early stop (a clip without live slots keeps stepping:
                its candidates are its finished slots, which is what "frozen" claims)
  search_fp64   the whole path: model arithmetic of oracle/s2vt_oracle.py in float64, sampling.gumbel_noise, every one of the V
                children of a live slot a candidate (no fan-out limit), no early stop; returns per clip the smallest decision gap
"""
import numpy as np
import torch

from oracle import s2vt_oracle as oracle
from s2vt_video_caption_amd import sampling

FAN = 20
SOS, EOS = 3, 4
LN2 = 0.6931471805599453


def cond_gumbel(G_parent, Z, g):
    """G~ = -log(exp(-G_parent) - exp(-Z) + exp(-g)) in its stable form, float64 (scalars or arrays): the children's perturbed
    scores g (maximum Z) conditioned on their maximum being G_parent.  g == Z gives G_parent exactly."""
    G_parent, Z, g = np.float64(G_parent), np.float64(Z), np.asarray(g, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = g - Z
        l = np.where(d > -LN2, np.log(-np.expm1(d)), np.log1p(-np.exp(d)))
        u = (G_parent - g) + l
        return (G_parent - np.maximum(u, 0.0)) - np.log1p(np.exp(-np.abs(u)))


def inv_temperature(temperature):
    """fp32(1 / temperature) as the library forms it: the fp32 quotient of fp32 operands"""
    return float(np.float32(1.0) / np.float32(temperature))


def head_ref(logits, inv_t, seed, step, rows):
    """float64 head over logits [R, V] (row i draws with batch row rows[i]): (top_ix [R, 20], top_lp [R, 20], top_g [R, 20]) in
    (g descending, v ascending) order, and the whole (lp, g) [R, V]"""
    x = np.asarray(logits, dtype=np.float64) * np.float64(inv_t)
    m = x.max(axis=1, keepdims=True)
    lp = np.minimum(x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))), 0.0)
    g = lp + sampling.gumbel_noise(seed, step, np.asarray(rows), x.shape[1])
    order = np.argsort(-g, axis=1, kind="stable")[:, :FAN]
    return order.astype(np.int64), np.take_along_axis(lp, order, 1), np.take_along_axis(g, order, 1), lp, g


class PolicyF64(object):
    """The policy alone on the row protocol of the library, one call per depth as the device runs it.  rows() = int array [2][B*W]
    (row_state, row_tok as the device writes them: slot j of clip b in row b*W+j, 0 where the slot is not live); step(top_ix, top_lp,
    top_g) consumes the [B*W][20] arrays of the next depth; frozen() = clips without a live slot; gap[b] = the smallest decision gap
    so far (W-th against (W+1)-th candidate, adjacent selected candidates); result() = (ids [B][W][D] padded with eos, lens [B][W],
    logprob fp32 [B][W], perturbed fp64 [B][W], kappa fp64 [B])."""

    def __init__(self, B, W, D, sos=SOS, eos=EOS):
        self.B, self.W, self.D, self.eos, self.t = B, W, D, eos, 0
        # a slot: (kind, phi fp32, G fp64, tokens, state row, last word); kind 1 live, 2 finished
        self.slots = [[(1, np.float32(0), np.float64(0), [], b, sos)] for b in range(B)]
        self.kappa = np.full(B, -np.inf)
        self.gap = np.full(B, np.inf)

    def rows(self):
        out = np.zeros((2, self.B * self.W), dtype=np.int32)
        for b in range(self.B):
            for j, (kind, _, _, _, row, tok) in enumerate(self.slots[b]):
                if kind == 1:
                    out[0, b * self.W + j], out[1, b * self.W + j] = row, tok
        return out

    def frozen(self):
        return np.array([all(s[0] != 1 for s in self.slots[b]) for b in range(self.B)])

    def step(self, top_ix, top_lp, top_g):
        self.t += 1
        t, W = self.t, self.W
        ix, lp, tg = np.asarray(top_ix), np.asarray(top_lp, dtype=np.float32), np.asarray(top_g, dtype=np.float32).astype(np.float64)
        for b in range(self.B):
            cands = []                                     # (G~, c)
            for j, (kind, phi, G, toks, _, _) in enumerate(self.slots[b]):
                r = b * W + j
                if kind == 1:
                    gt = cond_gumbel(G, tg[r, 0], tg[r])
                    cands.extend((float(gt[f]), j * FAN + f) for f in range(FAN))
                else:
                    cands.append((float(G), j * FAN))
            cands.sort(key=lambda e: (-e[0], e[1]))
            m = min(W, len(cands))
            nxt = []
            for gt, c in cands[:m]:
                j, f = divmod(c, FAN)
                kind, phi, G, toks, _, _ = self.slots[b][j]
                if kind == 2:
                    nxt.append(self.slots[b][j])
                    continue
                r = b * W + j
                v = int(ix[r, f])
                s = np.float32(phi) + lp[r, f]
                s = np.float32(0) if s == 0 else np.float32(s)
                nxt.append((2 if v == self.eos else 1, s, np.float64(gt), toks + [v], r, v))
            ref = [e[0] for e in cands[:m + 1]]
            if len(ref) > 1:
                self.gap[b] = min(self.gap[b], min(ref[i] - ref[i + 1] for i in range(len(ref) - 1)))
            if len(cands) > m:
                self.kappa[b] = max(self.kappa[b], cands[m][0])
            self.slots[b] = nxt

    def result(self):
        B, W, D = self.B, self.W, self.D
        ids = np.full((B, W, D), self.eos, dtype=np.int64)
        lens = np.zeros((B, W), dtype=np.int64)
        lp = np.full((B, W), -np.inf, dtype=np.float32)
        G = np.full((B, W), -np.inf, dtype=np.float64)
        for b in range(B):
            for k, (_, phi, g, toks, _, _) in enumerate(self.slots[b]):
                ids[b, k, :len(toks)] = toks
                lens[b, k], lp[b, k], G[b, k] = len(toks), phi, g
        return ids, lens, lp, G, self.kappa.copy()


def search_fp64(params, feats, W, D, temperature=1.0, seed=0, sos=SOS, eos=EOS):
    """-> list over clips of dict(ids=[W token lists in order], logprob=[...], G=[...], kappa, gap, stopped): the whole search in
    float64 with NO early stop and no fan-out limit.  gap = the smallest, over the depths, of: the W-th against the (W+1)-th
    candidate's G~, adjacent selected candidates' G~, and each live parent's W-th against (W+1)-th child by g.  stopped = the first
    depth after which the clip had no live slot (None: it ran to D)."""
    p = {k: v.double() for k, v in params.items()}
    feats = feats.double()
    inv_t = inv_temperature(temperature)
    B, L, _ = feats.shape
    x1 = feats @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)                       # vid_rnn over the L real frames only
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    vid = []                                                           # vid_rnn stepped with zero input, shared by a clip's slots
    for t in range(D):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        vid.append(h1)
    out = []
    for b in range(B):
        # a slot: dict(kind, phi, G, toks) ; live slots also carry their word_rnn state
        slots = [dict(kind=1, phi=0.0, G=0.0, toks=[], h=h2[b], c=c2[b], last=sos)]
        kappa, gap, stopped = -np.inf, np.inf, None
        for t in range(1, D + 1):
            live = [j for j, s in enumerate(slots) if s["kind"] == 1]
            cands = []                                                 # (G~, j, v, lp, g-rank)
            nh = nc = None
            if live:
                wh = torch.stack([slots[j]["h"] for j in live])
                wc = torch.stack([slots[j]["c"] for j in live])
                last = torch.tensor([slots[j]["last"] for j in live])
                nh, nc = oracle._word_step(p, p["embedding.weight"][last], vid[t - 1][b:b + 1].expand(len(live), -1), wh, wc)
                logits = (nh @ p["out_linear.weight"].t() + p["out_linear.bias"]).numpy()
                V = logits.shape[1]
                _, _, _, lp, g = head_ref(logits, inv_t, seed, t - 1, [b * W + j for j in live])
                for i, j in enumerate(live):
                    order = np.argsort(-g[i], kind="stable")
                    gs = g[i][order]
                    if V > W:
                        gap = min(gap, float(gs[W - 1] - gs[W]))
                    gt = cond_gumbel(slots[j]["G"], gs[0], gs)
                    cands.extend((float(gt[f]), j, int(order[f]), float(lp[i][order[f]]), i) for f in range(V))
            cands.extend((float(s["G"]), j, -1, 0.0, -1) for j, s in enumerate(slots) if s["kind"] == 2)
            cands.sort(key=lambda e: (-e[0], e[1], e[2]))
            m = min(W, len(cands))
            ref = [e[0] for e in cands[:m + 1]]
            if len(ref) > 1:
                gap = min(gap, min(ref[i] - ref[i + 1] for i in range(len(ref) - 1)))
            if len(cands) > m:
                kappa = max(kappa, cands[m][0])
            nxt = []
            for gt, j, v, lpv, i in cands[:m]:
                if v < 0:
                    nxt.append(slots[j])
                elif v == eos:
                    nxt.append(dict(kind=2, phi=slots[j]["phi"] + lpv, G=gt, toks=slots[j]["toks"] + [v]))
                else:
                    nxt.append(dict(kind=1, phi=slots[j]["phi"] + lpv, G=gt, toks=slots[j]["toks"] + [v], h=nh[i], c=nc[i], last=v))
            slots = nxt
            if stopped is None and t < D and all(s["kind"] == 2 for s in slots):
                stopped = t
        out.append(dict(ids=[s["toks"] for s in slots], logprob=[s["phi"] for s in slots], G=[s["G"] for s in slots], kappa=kappa,
                        gap=gap, stopped=stopped))
    return out


def ancestral_fp64(params, feats, D, temperature=1.0, seed=0, sos=SOS, eos=EOS):
    """Gumbel-max ancestral sampling in float64 with the noise of mode='sample' (row b, step t): per clip the words up to and
    including the first <eos>, at most D; written without any of the search's machinery"""
    p = {k: v.double() for k, v in params.items()}
    feats = feats.double()
    inv_t = np.float64(inv_temperature(temperature))
    B, L, _ = feats.shape
    x1 = feats @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, L)
    h2 = x1.new_zeros(B, x1.shape[2])
    c2 = x1.new_zeros(B, x1.shape[2])
    for t in range(L):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    last = torch.full((B,), sos, dtype=torch.long)
    words = []
    for t in range(D):
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        h2, c2 = oracle._word_step(p, p["embedding.weight"][last], h1, h2, c2)
        logits = (h2 @ p["out_linear.weight"].t() + p["out_linear.bias"]).numpy()
        sc = logits * inv_t + sampling.gumbel_noise(seed, t, B, logits.shape[1])
        last = torch.from_numpy(sc.argmax(1))
        words.append(last.numpy())
    rows = []
    for r in np.stack(words, 1).tolist():
        rows.append(r[:r.index(eos) + 1] if eos in r else r)
    return rows
