"""Consensus (minimum-Bayes-risk) selection among the candidate captions of a clip: keep the candidate that agrees most with the
others under CIDEr-D (Devlin et al. 2015's consensus re-ranking).  The candidates are what the model already produces - the K rows of
S2VT.sample / sample_truncated, the n_best list of mode='beam' / beam_constrained / Ensemble.beam, the groups of beam_diverse - as
token ids, so every model variant is served; the utility and the choice are self_critical.CiderRewarder.consensus' (the host oracle)
and, for a DeviceCiderRewarder, s2vt_cider_consensus' on the card.  A MixedRewarder / DeviceMixedRewarder chooses under its own utility,
cider_weight * CIDEr-D + bleu_weight * sentence BLEU-4 (s2vt_mixed_consensus on the card)."""
import torch

from .self_critical import DeviceCiderRewarder


def flatten_candidates(ids, scores=None):
    """(ids [B, K, T], valid bool [B, K] or None) of candidates [B, K, T] or [B, G, n, T] (the leading candidate axes are flattened,
    group-major) and their scores [B, K] / [B, G, n]: a candidate whose score is not finite - a beam slot that was never filled - is
    not valid.  ValueError for any other shape."""
    if not isinstance(ids, torch.Tensor) or ids.dim() not in (3, 4) or min(ids.shape) < 1:
        raise ValueError("consensus.select: ids must be a tensor [B, K, T] or [B, G, n, T], got %s" % (
            tuple(ids.shape) if isinstance(ids, torch.Tensor) else type(ids).__name__,))
    lead = tuple(ids.shape[:-1])
    flat = ids.reshape(ids.shape[0], -1, ids.shape[-1])
    if scores is None:
        return flat, None
    if not isinstance(scores, torch.Tensor) or tuple(scores.shape) != lead:
        raise ValueError("consensus.select: scores must be a tensor %s (one per candidate), got %s" % (
            lead, tuple(scores.shape) if isinstance(scores, torch.Tensor) else type(scores).__name__))
    return flat, torch.isfinite(scores).reshape(ids.shape[0], -1)


def select(rewarder, ids, scores=None):
    """(chosen_ids [B, T], best int64 [B], utility fp64 [B, K]) on the device of `ids`: per clip the candidate with the highest
    consensus utility (the first of equals; candidate 0 where none is valid).  rewarder: a DeviceCiderRewarder - kernel, gather on
    the device, no host read - or a host CiderRewarder, whose path copies the ids to the host and the results back (the two can
    be compared).  The utility is the rewarder's consensus(): CIDEr-D, or the CIDEr-D / BLEU-4 mix of a (Device)MixedRewarder - a
    DeviceMixedRewarder is a DeviceCiderRewarder and takes the device path.  scores: see flatten_candidates."""
    flat, valid = flatten_candidates(ids, scores)
    if isinstance(rewarder, DeviceCiderRewarder):
        best, utility = rewarder.consensus(flat, valid)
    else:
        b, u = rewarder.consensus(flat.cpu(), None if valid is None else valid.cpu())
        best, utility = torch.from_numpy(b).to(flat.device), torch.from_numpy(u).to(flat.device)
    chosen = flat.gather(1, best.view(-1, 1, 1).expand(-1, 1, flat.shape[2])).squeeze(1)
    return chosen, best, utility
