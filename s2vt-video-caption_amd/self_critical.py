"""Host side of self-critical sequence training (train.py --self-critical): CIDEr rewards of sampled and greedy captions against a
clip's references, and the per-token weights utils.RewardCriterion takes.

The score is caption_metrics.cider's own arithmetic (its cider_vector / cider_of_vectors) over token IDS, with the document
frequencies of the TRAINING split computed once - a batch is too small a corpus to take them from.  MixedRewarder /
DeviceMixedRewarder add the sentence BLEU-4 of the same rows: the reward cider_weight * CIDEr + bleu_weight * BLEU-4."""
import math
from collections import Counter

import numpy as np
import torch

from caption_metrics import cider_document_frequencies, cider_of_vectors, cider_vector, ngrams


def strip_caption(tokens, sos_ix, eos_ix, pad_ix=0):
    """the words of an id sequence: from after a leading <sos> up to the first <eos> (pads dropped)"""
    out = []
    for i, t in enumerate(tokens):
        t = int(t)
        if t == eos_ix:
            break
        if (i == 0 and t == sos_ix) or t == pad_ix:
            continue
        out.append(t)
    return out


class CiderRewarder(object):
    def __init__(self, captions, video_ids, sos_ix, eos_ix, n=4, sigma=6.0):
        """captions: {video id: [token id lists]} (dataloader.VideoDataset.captions); video_ids: the training split"""
        self.n, self.sigma, self.sos_ix, self.eos_ix = n, sigma, sos_ix, eos_ix
        self.refs = {v: [ngrams(strip_caption(c, sos_ix, eos_ix), n) for c in captions[v]] for v in video_ids}
        self.df, self.log_n = cider_document_frequencies(self.refs)
        self._ref_vecs = {}

    def score(self, video_id, tokens):
        """CIDEr of one candidate id sequence (cut at its first <eos>) against the references of video_id"""
        if video_id not in self._ref_vecs:
            self._ref_vecs[video_id] = [cider_vector(c, self.df, self.log_n, self.n) for c in self.refs[video_id]]
        hyp = cider_vector(ngrams(strip_caption(tokens, self.sos_ix, self.eos_ix), self.n), self.df, self.log_n, self.n)
        return float(cider_of_vectors(hyp, self._ref_vecs[video_id], self.n, self.sigma))

    def rewards(self, video_ids, ids):
        rows = ids.tolist() if isinstance(ids, torch.Tensor) else ids
        return np.array([self.score(v, r) for v, r in zip(video_ids, rows)])

    def consensus(self, ids, valid=None):
        """Consensus (minimum-Bayes-risk) selection among the K candidate id rows of each clip, ids [B, K, T] (host tensor, array or
        nested lists), valid bool [B, K] or None (all valid): numpy (best int64 [B], utility float64 [B, K]).  utility[b, i] is the
        CIDEr of candidate i against the clip's OTHER valid candidates, in ascending order, as its references - cider_of_vectors
        with the document frequencies of this rewarder's split; 0.0 when it has no other, -inf where i is not valid.  best[b] is the
        smallest valid i whose utility is the maximum, 0 without a valid candidate.  The clips need not be of the split."""
        rows, valid = _consensus_args(ids, valid)
        B, K = valid.shape
        best, utility = np.zeros(B, dtype=np.int64), np.full((B, K), -np.inf, dtype=np.float64)
        for b in range(B):
            vecs = [cider_vector(ngrams(strip_caption(rows[b][k], self.sos_ix, self.eos_ix), self.n), self.df, self.log_n, self.n)
                    if valid[b, k] else None for k in range(K)]
            for i in range(K):
                if valid[b, i]:
                    others = [vecs[j] for j in range(K) if valid[b, j] and j != i]
                    utility[b, i] = float(cider_of_vectors(vecs[i], others, self.n, self.sigma)) if others else 0.0
            best[b] = _first_best(utility[b], valid[b])
        return best, utility


# ------------------------------------------------------------------ sentence BLEU-4 beside CIDEr (train.py --sc-bleu-weight)
BLEU_TINY, BLEU_SMALL = 1e-15, 1e-9      # the reference scorer's epsilons on matches and on totals (caption_metrics.bleu)


def bleu_bp(c, rl):
    """brevity penalty of a row of c words against the reference length rl, with the scorer's epsilons"""
    ratio = (c + BLEU_TINY) / (rl + BLEU_SMALL)
    return math.exp(1.0 - 1.0 / ratio) if ratio < 1.0 else 1.0


def closest_length(c, ref_lens):
    """the reference length closest to c, ties to the shorter"""
    return min((abs(l - c), l) for l in ref_lens)[1]


def bleu_chain(c, match, bp):
    """BLEU-4 from the row's length, its four clipped match counts and the brevity penalty: caption_metrics.bleu's per-sentence
    product with sqrt(sqrt(.)) as the fourth root (correctly rounded on host and device; pow is not)"""
    prod = 1.0
    for k in range(4):
        prod *= (match[k] + BLEU_TINY) / (max(0, c - k) + BLEU_SMALL)
    return math.sqrt(math.sqrt(prod)) * bp


def sentence_bleu4(words, refs):
    """per-sentence BLEU_4 of a word (id) list against a list of reference word lists: caption_metrics.bleu(gts, res)[1][3] of that one
    id, the fourth root as in bleu_chain.  An empty `words` scores exactly 0.0."""
    c = len(words)
    ref_max = Counter()
    for r in refs:
        for g, n in ngrams(r, 4).items():
            if n > ref_max[g]:
                ref_max[g] = n
    match = [0] * 4
    for g, n in ngrams(words, 4).items():
        match[len(g) - 1] += min(n, ref_max.get(g, 0))
    return bleu_chain(c, match, bleu_bp(c, closest_length(c, [len(r) for r in refs])))


def _mix_weights(cider_weight, bleu_weight):
    try:
        w = (float(cider_weight), float(bleu_weight))
    except (TypeError, ValueError):
        raise ValueError("the reward weights must be finite floats, got %r and %r" % (cider_weight, bleu_weight))
    if not all(math.isfinite(x) for x in w):
        raise ValueError("the reward weights must be finite floats, got %r and %r" % (cider_weight, bleu_weight))
    return w


class MixedRewarder(CiderRewarder):
    """CiderRewarder with the reward cider_weight * CIDEr-D + bleu_weight * sentence BLEU-4 (the mix of Luo's self-critical.pytorch:
    cider_reward_weight / bleu_reward_weight), two products and one add in float64.  The host oracle of DeviceMixedRewarder."""

    def __init__(self, captions, video_ids, sos_ix, eos_ix, cider_weight=1.0, bleu_weight=0.0, n=4, sigma=6.0):
        self.cider_weight, self.bleu_weight = _mix_weights(cider_weight, bleu_weight)
        if n != 4:
            raise ValueError("the BLEU reward is BLEU-4 beside CIDEr over 1..4-grams, got n = %d" % n)
        CiderRewarder.__init__(self, captions, video_ids, sos_ix, eos_ix, n, sigma)
        self.ref_words = {v: [strip_caption(c, sos_ix, eos_ix) for c in captions[v]] for v in video_ids}
        self.last_parts = None      # (cider, bleu) of the latest rewards() call

    def bleu(self, video_id, tokens):
        """sentence BLEU-4 of one candidate id sequence against the references of video_id"""
        return sentence_bleu4(strip_caption(tokens, self.sos_ix, self.eos_ix), self.ref_words[video_id])

    def score(self, video_id, tokens):
        return self.cider_weight * CiderRewarder.score(self, video_id, tokens) + self.bleu_weight * self.bleu(video_id, tokens)

    def parts(self, video_ids, ids):
        """(cider, bleu) float64 [B] of the rows"""
        rows = ids.tolist() if isinstance(ids, torch.Tensor) else ids
        return (np.array([CiderRewarder.score(self, v, r) for v, r in zip(video_ids, rows)], dtype=np.float64),
                np.array([self.bleu(v, r) for v, r in zip(video_ids, rows)], dtype=np.float64))

    def rewards(self, video_ids, ids):
        self.last_parts = cider, bleu = self.parts(video_ids, ids)
        return self.cider_weight * cider + self.bleu_weight * bleu

    def consensus(self, ids, valid=None):
        """CiderRewarder.consensus under the mixed utility: utility[b, i] = cider_weight * (CiderRewarder.consensus' utility) +
        bleu_weight * BLEU-4 of candidate i with the clip's other valid candidates, ascending, as its references; 0.0 when i is the
        only valid candidate, -inf where i is not valid.  best[b] is the first maximum."""
        _, cider = CiderRewarder.consensus(self, ids, valid)
        rows, valid = _consensus_args(ids, valid)
        B, K = valid.shape
        best, utility = np.zeros(B, dtype=np.int64), np.full((B, K), -np.inf, dtype=np.float64)
        for b in range(B):
            words = [strip_caption(rows[b][k], self.sos_ix, self.eos_ix) if valid[b, k] else None for k in range(K)]
            for i in range(K):
                if valid[b, i]:
                    others = [words[j] for j in range(K) if valid[b, j] and j != i]
                    utility[b, i] = self.cider_weight * cider[b, i] + self.bleu_weight * sentence_bleu4(words[i], others) if others else 0.0
            best[b] = _first_best(utility[b], valid[b])
        return best, utility


def _consensus_args(ids, valid):
    """(rows as nested lists [B][K][T], valid bool [B, K]) of the arguments of a consensus call"""
    rows = ids.tolist() if isinstance(ids, (torch.Tensor, np.ndarray)) else ids
    B, K = len(rows), len(rows[0]) if len(rows) else 0
    if B < 1 or K < 1 or any(len(r) != K for r in rows):
        raise ValueError("consensus: ids must be [B, K, T] with B, K >= 1")
    valid = np.ones((B, K), dtype=bool) if valid is None else np.asarray(valid.cpu() if isinstance(valid, torch.Tensor) else valid).astype(bool)
    if valid.shape != (B, K):
        raise ValueError("consensus: valid must be [B, K] = [%d, %d], got %s" % (B, K, valid.shape))
    return rows, valid


def _first_best(utility, valid):
    """the smallest valid index whose utility is the maximum over the valid ones; 0 where none is valid"""
    ix = np.nonzero(valid)[0]
    return int(ix[np.argmax(utility[ix])]) if len(ix) else 0


def advantage_weights(sampled, advantage, eos_ix):
    """weight fp32 [B, L] for RewardCriterion from sampled ids [B, L-1] (host tensor) and one advantage per row: the advantage on
    positions 1 .. len_b (the sampled tokens up to and including the first <eos>), zero after it and at position 0 (<sos>)"""
    B, Lm1 = sampled.shape
    is_eos = sampled == eos_ix
    first = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((B,), Lm1))
    w = torch.zeros(B, Lm1 + 1, dtype=torch.float32)
    pos = torch.arange(1, Lm1 + 1)[None, :]
    w[:, 1:] = (pos <= first[:, None]).float() * torch.as_tensor(advantage, dtype=torch.float32)[:, None]
    return w


def group_advantages(rewards, greedy=None):
    """(advantage, baseline) float64 [B, K] for K sampled captions per clip with rewards [B, K].  greedy None: row k is baselined
    with the mean reward of the clip's OTHER K - 1 rows (Luo 2020), K >= 2 -
        baseline[b, k] = ((r[b, 0] + r[b, 1] + ... + r[b, K-1], added in that order from 0.0) - r[b, k]) / (K - 1);
    greedy float64 [B]: baseline[b, k] = greedy[b].  advantage = r - baseline.  s2vt_sc_weights_group's arithmetic operation for
    operation (np.sum would add pairwise), so the device reproduces it bit for bit.  A clip whose K rewards compare equal takes
    that reward as every row's baseline: its advantages are exactly zero."""
    r = np.asarray(rewards, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] < 1:
        raise ValueError("group_advantages: rewards must be [B, K], got %s" % (r.shape,))
    B, K = r.shape
    if greedy is None:
        if K < 2:
            raise ValueError("group_advantages: the mean of the other K - 1 rewards needs K >= 2, got K = %d" % K)
        total = np.zeros(B, dtype=np.float64)
        for j in range(K):
            total = total + r[:, j]
        baseline = (total[:, None] - r) / np.float64(K - 1)
        same = (r == r[:, :1]).all(1)          # K equal rewards: the baseline is that reward, exactly (the rounded sum would
        baseline[same] = r[same]               # leave a difference of rounding size, and with it a weight that is not zero)
    else:
        g = np.asarray(greedy, dtype=np.float64)
        if g.shape != (B,):
            raise ValueError("group_advantages: greedy must be [B] = [%d], got %s" % (B, g.shape))
        baseline = np.broadcast_to(g[:, None], r.shape).copy()
    return r - baseline, baseline


def inclusion_log_q(logprob, kappa):
    """log of the probability that a caption with log-prob phi is among the K of a stochastic beam search whose threshold is kappa
    (S2VT.sample_distinct): it is kept when its Gumbel(phi) score exceeds kappa, q = 1 - exp(-exp(phi - kappa)).  logprob [..., K],
    kappa [...]; float64 [..., K].  Steps 1-2 of include/s2vt_hip.h "without-replacement weights":
        a = phi - kappa, e = exp(a), log q = log(-expm1(-e)), or a - 0.5 * e where a < -30 (finite where e underflows);
    kappa = -inf (nothing was left out) gives log q = 0."""
    phi = np.asarray(logprob, dtype=np.float64)
    kap = np.asarray(kappa, dtype=np.float64)
    if phi.ndim != kap.ndim + 1 or phi.shape[:-1] != kap.shape:
        raise ValueError("inclusion_log_q: logprob [..., K] with kappa [...], got %s and %s" % (phi.shape, kap.shape))
    with np.errstate(all="ignore"):
        a = phi - kap[..., None]
        e = np.exp(a)
        return np.where(a < -30.0, a - 0.5 * e, np.log(-np.expm1(-e)))


def swor_advantages(logprob, kappa, rewards, greedy=None):
    """(advantage float64 [B, K], coef float64 [B, K], baseline float64 [B]) for the K pairwise distinct captions per clip of
    S2VT.sample_distinct with log-probs logprob [B, K], threshold kappa [B] and rewards [B, K], 2 <= K <= 8: the normalised
    importance-weighted estimator with a built-in baseline (Kool, van Hoof, Welling 2019, "Buy 4 REINFORCE Samples, Get a Baseline
    for Free!") - s2vt_sc_weights_swor's arithmetic step for step (include/s2vt_hip.h "without-replacement weights"), in float64,
    every sum in ascending k from 0.0:
        lw = phi - log q, m = max lw, om = exp(lw - m), pi = exp(phi - m); W = sum om, N = sum om * r;
        baseline = greedy[b] where given, else N / W; W_i = (W - om_i) + pi_i, coef = om_i / W_i, advantage = coef * (r - baseline).
    greedy None and K equal rewards: advantages exactly zero, baseline that reward.  A bad clip (a log-prob that is not finite or
    positive, kappa NaN or +inf, a reward - greedy's included - that is not finite, an fp32 advantage that is not finite):
    advantage 0, coef 0, baseline NaN."""
    phi = np.asarray(logprob, dtype=np.float64)
    kap = np.asarray(kappa, dtype=np.float64)
    r = np.asarray(rewards, dtype=np.float64)
    if r.ndim != 2 or not 2 <= r.shape[1] <= 8 or phi.shape != r.shape or kap.shape != r.shape[:1]:
        raise ValueError("swor_advantages: logprob and rewards [B, K] with 2 <= K <= 8 and kappa [B], got %s, %s, %s" % (
            phi.shape, r.shape, kap.shape))
    B, K = r.shape
    bad = ~np.isfinite(phi).all(1) | (phi > 0).any(1) | np.isnan(kap) | (kap == np.inf) | ~np.isfinite(r).all(1)
    g = None
    if greedy is not None:
        g = np.asarray(greedy, dtype=np.float64)
        if g.shape != (B,):
            raise ValueError("swor_advantages: greedy must be [B] = [%d], got %s" % (B, g.shape))
        bad = bad | ~np.isfinite(g)
    with np.errstate(all="ignore"):
        lw = phi - inclusion_log_q(phi, kap)
        m = lw.max(1, keepdims=True)
        om, pi = np.exp(lw - m), np.exp(phi - m)
        W, N = np.zeros(B, dtype=np.float64), np.zeros(B, dtype=np.float64)
        for j in range(K):
            W = W + om[:, j]
            N = N + om[:, j] * r[:, j]
        same = (r == r[:, :1]).all(1) if g is None else np.zeros(B, dtype=bool)
        base = g.copy() if g is not None else np.where(same, r[:, 0], N / W)
        coef = om / ((W[:, None] - om) + pi)
        adv = coef * (r - base[:, None])
        adv[same] = 0.0
        bad = bad | ~np.isfinite(adv.astype(np.float32)).all(1)
    adv[bad], coef[bad], base[bad] = 0.0, 0.0, np.nan
    return adv, coef, base


# ------------------------------------------------------------------ the same score on the device (train.py --sc-reward device)
KEY_TOKENS, KEY_BITS = 4, 16         # an n-gram key: up to four tokens of 16 bits in a uint64, first token on top, absent positions 0


def pack_key(gram):
    """exact uint64 key of an n-gram (tuple of 1..4 token ids in [1, 65535]); the number of non-zero fields is its order"""
    if not 1 <= len(gram) <= KEY_TOKENS:
        raise ValueError("n-grams of 1..%d tokens have a key, got %d" % (KEY_TOKENS, len(gram)))
    key = 0
    for j, t in enumerate(gram):
        t = int(t)
        if not 0 < t < (1 << KEY_BITS):
            raise ValueError("token id %d does not fit the %d-bit fields of an n-gram key (ids 1..%d)" % (t, KEY_BITS, (1 << KEY_BITS) - 1))
        key |= t << (KEY_BITS * (KEY_TOKENS - 1 - j))
    return key


def unpack_key(key):
    """the n-gram (tuple of token ids) of a key"""
    key = int(key)
    toks = [(key >> (KEY_BITS * (KEY_TOKENS - 1 - j))) & ((1 << KEY_BITS) - 1) for j in range(KEY_TOKENS)]
    while toks and toks[-1] == 0:
        toks.pop()
    return tuple(toks)


class DeviceCiderRewarder(object):
    """CiderRewarder's score as a HIP kernel (s2vt_cider_rewards) over a reference table that is built here once and lives on
    the card.  Every factor that needs log / exp (idf, the references' tf-idf weights and norms, the length penalties) is
    computed on the host with caption_metrics' own expressions and stored as float64; the table is plain arrays:

      idf_keys, idf_vals [n_idf]   every n-gram of the training references, keys ascending; an absent key has idf log_n
      clip_ref_off [n_clips + 1]   CSR: the references of clip c (row number of video_ids[c])
      ent_off [4 * n_refs + 1]     CSR: the (ent_keys, ent_w = tf * idf) entries of reference r and order k at 4r + k-1, keys ascending
      ref_norm [4 * n_refs], ref_len [n_refs], pen [n_pen]

    `host` keeps the numpy copies (table_walk scores from them without a GPU); `device` uploads them at construction,
    otherwise the first rewards() / consensus() call uploads to the device of its ids.  consensus() (s2vt_cider_consensus) scores the
    K candidates of a clip against each other instead of the references and reads only idf_keys, idf_vals and pen of the table."""

    def __init__(self, captions, video_ids, sos_ix, eos_ix, n=4, sigma=6.0, device=None, vocab_size=None):
        if n != KEY_TOKENS:
            raise ValueError("the n-gram keys and the kernel are laid out for n = %d, got %d" % (KEY_TOKENS, n))
        if vocab_size is not None and vocab_size > (1 << KEY_BITS):
            raise ValueError("vocab_size %d: n-gram keys hold token ids below %d" % (vocab_size, 1 << KEY_BITS))
        from . import capi
        self.n, self.sigma, self.sos_ix, self.eos_ix = n, sigma, sos_ix, eos_ix
        base = CiderRewarder(captions, video_ids, sos_ix, eos_ix, n, sigma)
        df, log_n = base.df, base.log_n
        self.video_ids = list(video_ids)
        self.row_of = {v: i for i, v in enumerate(self.video_ids)}
        idf = sorted((pack_key(g), log_n - np.log(max(1.0, df.get(g, 0.0)))) for g in df)
        clip_ref_off, ent_off, ent_keys, ent_w, ref_norm, ref_len = [0], [0], [], [], [], []
        for v in self.video_ids:
            if not base.refs[v]:
                raise ValueError("clip %r has no reference caption" % (v,))
            for counts in base.refs[v]:
                vec, norm, length = cider_vector(counts, df, log_n, n)
                for k in range(n):
                    ent = sorted((pack_key(g), w) for g, w in vec[k].items())
                    ent_keys += [e[0] for e in ent]
                    ent_w += [e[1] for e in ent]
                    ent_off.append(len(ent_keys))
                ref_norm += [float(x) for x in norm]
                ref_len.append(int(length))
            clip_ref_off.append(len(ref_len))
        n_pen = max(max(ref_len), capi.CIDER_MAX_T) + 1          # every |candidate length - reference length| that can occur
        pen = [np.e ** (-(float(d) ** 2) / (2 * sigma ** 2)) for d in range(n_pen)]
        self.host = {
            "idf_keys": np.array([e[0] for e in idf], dtype=np.uint64), "idf_vals": np.array([e[1] for e in idf], dtype=np.float64),
            "clip_ref_off": np.array(clip_ref_off, dtype=np.int32), "ent_off": np.array(ent_off, dtype=np.int32),
            "ent_keys": np.array(ent_keys, dtype=np.uint64), "ent_w": np.array(ent_w, dtype=np.float64),
            "ref_norm": np.array(ref_norm, dtype=np.float64), "ref_len": np.array(ref_len, dtype=np.int32),
            "pen": np.array(pen, dtype=np.float64)}
        self.log_n = float(log_n)
        self._dev = None            # (device, tensors, capi.CiderTable)
        if device is not None:
            self._upload(torch.device(device))

    def _upload(self, device):
        from . import capi
        if device.type != "cuda":
            raise capi.S2VTHipError("DeviceCiderRewarder scores on a HIP device, got %s (CiderRewarder is the host scorer)" % (device,))
        # torch has no arithmetic on uint64: the keys travel as the same bits in int64
        tens = {k: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(device) for k, a in self.host.items()}
        tb = capi.CiderTable()
        for k, t in tens.items():
            setattr(tb, k, t.data_ptr())
        tb.log_n, tb.n_idf = self.log_n, len(self.host["idf_keys"])
        tb.n_clips, tb.n_refs, tb.n_pen = len(self.video_ids), len(self.host["ref_len"]), len(self.host["pen"])
        self._dev = (tens["pen"].device, tens, tb)         # the tensors keep the pointers of tb alive

    def rewards(self, video_ids, ids):
        """fp64 HIP tensor [B]: the score of each row of `ids` (HIP int64 [B, T], contiguous or row-strided) against the references
        of its clip.  Host work: B dictionary look-ups (KeyError for an unknown clip) and one small copy of the row numbers."""
        from . import ops
        from .functional import require_hip
        require_hip(ids, "ids")
        rows = [self.row_of[v] for v in video_ids]
        if self._dev is None or self._dev[0] != ids.device:
            self._upload(ids.device)
        clip_rows = torch.tensor(rows, dtype=torch.int32).to(ids.device, non_blocking=True)
        return ops.cider_rewards(self._dev[2], clip_rows, ids, self.sos_ix, self.eos_ix)

    def consensus(self, ids, valid=None):
        """(best int64 [B], utility fp64 [B, K]) HIP tensors: CiderRewarder.consensus on the device (ops.cider_consensus) for ids HIP
        int64 [B, K, T] and valid bool [B, K] on the device or None.  No host work beyond the first call's upload of the table."""
        from . import ops
        from .functional import require_hip
        require_hip(ids, "ids")
        if self._dev is None or self._dev[0] != ids.device:
            self._upload(ids.device)
        return ops.cider_consensus(self._dev[2], ids, self.sos_ix, self.eos_ix, valid)

    def _row_walk(self, tokens):
        """the candidate phase of the kernels in numpy: (unique keys ascending, tf * idf, order of each key, norm per order, bigrams)"""
        h = self.host
        words = strip_caption(tokens, self.sos_ix, self.eos_ix)
        keys = np.array([pack_key(words[i:i + k]) for k in range(1, self.n + 1) for i in range(len(words) - k + 1)], dtype=np.uint64)
        uniq, tf = np.unique(keys, return_counts=True)
        order = np.array([len(unpack_key(u)) for u in uniq], dtype=np.int64)
        at = np.searchsorted(h["idf_keys"], uniq)
        w = np.empty(len(uniq), dtype=np.float64)
        for i in range(len(uniq)):
            hit = at[i] < len(h["idf_keys"]) and h["idf_keys"][at[i]] == uniq[i]
            w[i] = float(tf[i]) * (h["idf_vals"][at[i]] if hit else self.log_n)
        hn = [np.sqrt(sum(x * x for x in w[order == k + 1])) for k in range(self.n)]
        return uniq, w, order, hn, max(len(words) - 1, 0)

    def consensus_walk(self, rows, valid=None):
        """s2vt_cider_consensus' walk for ONE clip in numpy (float64), on the host copy of the table: rows = its K id rows, valid =
        K flags or None -> (best, utility float64 [K]).  Every candidate is a sorted key list with weights; a pair (i, j) looks i's
        keys up in j's list; the pairs' terms are added per order in ascending j."""
        h = self.host
        K = len(rows)
        valid = np.ones(K, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
        cand = [self._row_walk(r) if valid[k] else None for k, r in enumerate(rows)]
        utility = np.full(K, -np.inf, dtype=np.float64)
        for i in range(K):
            if not valid[i]:
                continue
            uniq, w, order, hn, hl = cand[i]
            total, others = np.zeros(self.n), 0
            for j in range(K):
                if j == i or not valid[j]:
                    continue
                jk, jw, _, jn, jl = cand[j]
                pen = h["pen"][abs(hl - jl)]
                dot = np.zeros(self.n)
                for e in np.nonzero(w != 0.0)[0]:
                    at = int(np.searchsorted(jk, uniq[e]))
                    if at < len(jk) and jk[at] == uniq[e]:
                        dot[order[e] - 1] += min(w[e], jw[at]) * jw[at]
                for k in range(self.n):
                    if hn[k] != 0 and jn[k] != 0:
                        dot[k] /= hn[k] * jn[k]
                    total[k] += dot[k] * pen
                others += 1
            utility[i] = float((((total[0] + total[1]) + total[2]) + total[3]) / 4.0 / others * 10.0) if others else 0.0
        return _first_best(utility, valid), utility

    def table_walk(self, video_id, tokens):
        """the kernel's walk over the flat arrays in numpy (float64), on the host copy: what s2vt_cider_rewards computes for one row"""
        h = self.host
        uniq, w, order, hn, hl = self._row_walk(tokens)
        c = self.row_of[video_id]
        r0, r1 = int(h["clip_ref_off"][c]), int(h["clip_ref_off"][c + 1])
        total = np.zeros(self.n)
        for r in range(r0, r1):
            pen = h["pen"][abs(hl - int(h["ref_len"][r]))]
            for k in range(self.n):
                lo, hi = int(h["ent_off"][4 * r + k]), int(h["ent_off"][4 * r + k + 1])
                rk, rw = h["ent_keys"][lo:hi], h["ent_w"][lo:hi]
                dot = 0.0
                for i in np.nonzero(order == k + 1)[0]:
                    j = int(np.searchsorted(rk, uniq[i]))
                    if j < len(rk) and rk[j] == uniq[i]:
                        dot += min(w[i], rw[j]) * rw[j]
                rn = h["ref_norm"][4 * r + k]
                if hn[k] != 0 and rn != 0:
                    dot /= hn[k] * rn
                total[k] += dot * pen
        return float(np.mean(total) / (r1 - r0) * 10.0)


class DeviceMixedRewarder(DeviceCiderRewarder):
    """MixedRewarder's reward and consensus utility on the device (s2vt_mixed_rewards / s2vt_mixed_consensus): DeviceCiderRewarder with
    the BLEU table (s2vt_bleu_table of include/s2vt_hip.h) built beside the CIDEr one, as plain arrays in `host`:

      bleu_key_off [n_clips + 1]     CSR: the (bleu_keys ascending, bleu_max int32) entries of clip c - the union of its references'
                                     1..4-grams under the keys above with the largest count among the references
      bleu_ref_words [n_refs]        the references' lengths in WORDS, under clip_ref_off (ref_len counts bigrams)
      bp [CIDER_MAX_T + 1, n_rl]     bleu_bp(c, rl) by math.exp for every row length and every rl up to the longest reference

    A subclass of DeviceCiderRewarder, so consensus.select routes it to the device.  bleu_walk / bleu_consensus_walk restate the
    kernels' BLEU phase in numpy over the flat arrays."""

    def __init__(self, captions, video_ids, sos_ix, eos_ix, cider_weight=1.0, bleu_weight=0.0, n=4, sigma=6.0, device=None, vocab_size=None):
        from . import capi
        self.cider_weight, self.bleu_weight = _mix_weights(cider_weight, bleu_weight)
        DeviceCiderRewarder.__init__(self, captions, video_ids, sos_ix, eos_ix, n, sigma, None, vocab_size)
        key_off, keys, counts, ref_words = [0], [], [], []
        for v in self.video_ids:
            union = {}
            for c in captions[v]:
                words = strip_caption(c, sos_ix, eos_ix)
                ref_words.append(len(words))
                for g, tf in ngrams(words, n).items():
                    k = pack_key(g)
                    union[k] = max(union.get(k, 0), tf)
            ent = sorted(union.items())
            keys += [e[0] for e in ent]
            counts += [e[1] for e in ent]
            key_off.append(len(keys))
        n_rl = max(max(ref_words), capi.CIDER_MAX_T) + 1
        self.host.update({
            "bleu_key_off": np.array(key_off, dtype=np.int32), "bleu_keys": np.array(keys, dtype=np.uint64),
            "bleu_max": np.array(counts, dtype=np.int32), "bleu_ref_words": np.array(ref_words, dtype=np.int32),
            "bp": np.array([[bleu_bp(c, rl) for rl in range(n_rl)] for c in range(capi.CIDER_MAX_T + 1)], dtype=np.float64)})
        self.last_parts = None      # (cider, bleu) of the latest rewards() call, HIP tensors
        if device is not None:
            self._upload(torch.device(device))

    def _upload(self, device):
        from . import capi
        h = self.host
        DeviceCiderRewarder._upload(self, device)           # (host entries that are no field of the CIDEr table do not reach it)
        tens = self._dev[1]
        bt = capi.BleuTable()
        for field, name in (("clip_key_off", "bleu_key_off"), ("keys", "bleu_keys"), ("max_count", "bleu_max"),
                            ("clip_ref_off", "clip_ref_off"), ("ref_words", "bleu_ref_words"), ("bp", "bp")):
            setattr(bt, field, tens[name].data_ptr())
        bt.n_keys, bt.n_clips, bt.n_refs, bt.n_rl = len(h["bleu_keys"]), len(self.video_ids), len(h["bleu_ref_words"]), h["bp"].shape[1]
        self._bleu = bt

    def _tables(self, ids):
        from .functional import require_hip
        require_hip(ids, "ids")
        if self._dev is None or self._dev[0] != ids.device:
            self._upload(ids.device)
        return self._dev[2], self._bleu

    def _scores(self, video_ids, ids):
        """(mix, cider, bleu) fp64 HIP tensors [B] of one s2vt_mixed_rewards call"""
        from . import ops
        tb, bt = self._tables(ids)
        clip_rows = torch.tensor([self.row_of[v] for v in video_ids], dtype=torch.int32).to(ids.device, non_blocking=True)
        return ops.mixed_rewards(tb, bt, clip_rows, ids, self.sos_ix, self.eos_ix, self.cider_weight, self.bleu_weight, return_parts=True)

    def rewards(self, video_ids, ids):
        """fp64 HIP tensor [B]: cider_weight * CIDEr + bleu_weight * BLEU-4 of each row (DeviceCiderRewarder.rewards' arguments)"""
        mix, cider, bleu = self._scores(video_ids, ids)
        self.last_parts = (cider, bleu)
        return mix

    def parts(self, video_ids, ids):
        """(cider, bleu) fp64 HIP tensors [B] of the rows, the CIDEr part with DeviceCiderRewarder.rewards' bits"""
        return self._scores(video_ids, ids)[1:]

    def consensus(self, ids, valid=None):
        """(best int64 [B], utility fp64 [B, K]) HIP tensors: MixedRewarder.consensus on the device (ops.mixed_consensus)"""
        from . import ops
        tb, bt = self._tables(ids)
        return ops.mixed_consensus(tb, bt, ids, self.sos_ix, self.eos_ix, self.cider_weight, self.bleu_weight, valid)

    def _sorted_keys(self, tokens):
        """(number of words, the row's 1..4-gram keys ascending with repeats) - what the candidate phase leaves in LDS"""
        words = strip_caption(tokens, self.sos_ix, self.eos_ix)
        keys = np.array([pack_key(words[i:i + k]) for k in range(1, self.n + 1) for i in range(len(words) - k + 1)], dtype=np.uint64)
        return len(words), np.sort(keys)

    @staticmethod
    def _run(keys, at):
        """number of entries equal to keys[at] from `at` on"""
        tf = 1
        while at + tf < len(keys) and keys[at + tf] == keys[at]:
            tf += 1
        return tf

    def bleu_walk(self, video_id, tokens):
        """the BLEU phase of s2vt_mixed_rewards for one row in numpy, on the host copy of the table: run heads of the sorted keys, the
        run length as tf, a binary search in the clip's key range for the largest reference count, the closest length as a keyed
        minimum, bleu_chain with bp from the table"""
        h = self.host
        c, keys = self._sorted_keys(tokens)
        row = self.row_of[video_id]
        k0, k1 = int(h["bleu_key_off"][row]), int(h["bleu_key_off"][row + 1])
        ck, cm = h["bleu_keys"][k0:k1], h["bleu_max"][k0:k1]
        match = [0] * 4
        for i in range(len(keys)):
            if i > 0 and keys[i - 1] == keys[i]:
                continue
            at = int(np.searchsorted(ck, keys[i]))
            if at < len(ck) and ck[at] == keys[i]:
                match[len(unpack_key(keys[i])) - 1] += min(self._run(keys, i), int(cm[at]))
        r0, r1 = int(h["clip_ref_off"][row]), int(h["clip_ref_off"][row + 1])
        near = min((abs(int(l) - c) << 32) | int(l) for l in h["bleu_ref_words"][r0:r1])
        return bleu_chain(c, match, float(h["bp"][c, min(near & 0xFFFFFFFF, h["bp"].shape[1] - 1)]))

    def bleu_consensus_walk(self, rows, valid=None):
        """the BLEU phase of s2vt_mixed_consensus for ONE clip in numpy: rows = its K id rows, valid = K flags or None -> float64 [K],
        the BLEU-4 of every valid candidate against the other valid ones (for every run head the largest run length at the key's
        lower bound in the others' sorted lists; rl among the others' word counts), 0.0 without another, -inf where not valid"""
        h = self.host
        K = len(rows)
        valid = np.ones(K, dtype=bool) if valid is None else np.asarray(valid).astype(bool)
        cand = [self._sorted_keys(r) if valid[k] else None for k, r in enumerate(rows)]
        out = np.full(K, -np.inf, dtype=np.float64)
        for i in range(K):
            if not valid[i]:
                continue
            others = [cand[j] for j in range(K) if j != i and valid[j]]
            if not others:
                out[i] = 0.0
                continue
            c, keys = cand[i]
            match = [0] * 4
            for e in range(len(keys)):
                if e > 0 and keys[e - 1] == keys[e]:
                    continue
                rmax = 0
                for _, jk in others:
                    at = int(np.searchsorted(jk, keys[e]))
                    if at < len(jk) and jk[at] == keys[e]:
                        rmax = max(rmax, self._run(jk, at))
                match[len(unpack_key(keys[e])) - 1] += min(self._run(keys, e), rmax)
            near = min((abs(jc - c) << 32) | jc for jc, _ in others)
            out[i] = bleu_chain(c, match, float(h["bp"][c, min(near & 0xFFFFFFFF, h["bp"].shape[1] - 1)]))
        return out
