"""Host side of self-critical sequence training (train.py --self-critical): CIDEr rewards of sampled and greedy captions against a
clip's references, and the per-token weights utils.RewardCriterion takes.

The score is caption_metrics.cider's own arithmetic (its cider_vector / cider_of_vectors) over token IDS, with the document
frequencies of the TRAINING split computed once - a batch is too small a corpus to take them from."""
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
