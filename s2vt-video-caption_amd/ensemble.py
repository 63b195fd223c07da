"""Ensemble beam search: several S2VT models, ONE cumulative-score search, on the device (`S2VTModel.Ensemble`; not in the
reference; include/s2vt_hip.h "ensemble beam").

At every depth the members' word distributions are averaged (the log of the weighted arithmetic mean of their probabilities) and
mode='beam''s policy runs over the average.  What belongs to one model stays per member - beam._DepthStep: encoder states, decode
cache, workspace, state tables and the depth step, stopped one launch early so that the member leaves its logits on the card
(s2vt_beam_step_logits) - and what does not is mode='beam''s own: the search driver with its policy kernel (csrc/beam_policy.hip at
one group), the depth loop with its polled early exit and the result kernel (beam._group_search).  This module adds the depth step
of an ensemble: the members' steps into one [M, R, V] logits buffer, then ONE fan-out head over it (csrc/ensemble.hip).  Nothing
crosses PCIe per depth.
"""
import ctypes

import torch

from . import beam, capi, ops, sampling

MAX_MEMBERS = 8
_AGREE = ("vocab_size", "length", "feat_dim", "sos_ix", "eos_ix")


def _member(lib, model, feats, D, R):
    """what one member owns in a search (beam._DepthStep), on its own encoder states"""
    feats = model.feat_drop(feats)
    params = model._hip_params()
    return beam._DepthStep(lib, model, feats, params, R, *beam._encoder_states(model, feats, params, D, beam.PLANE_STEP and beam.PLANE_ENCODER))


class Ensemble(object):
    """Ensemble([m0, m1, ...], weights=None): up to 8 one-layer LSTM S2VT models decoded as one.  weights: one positive number per
    member (normalised to sum 1), None: uniform.  The members must agree on vocab_size, length, feat_dim, sos_ix and eos_ix; they
    may differ in dim_hid and dim_embed."""

    def __init__(self, models, weights=None):
        models = list(models)
        if not 1 <= len(models) <= MAX_MEMBERS:
            raise ValueError("Ensemble: 1 to %d members, got %d" % (MAX_MEMBERS, len(models)))
        self.log_w = ops.ensemble_log_weights(weights, len(models))
        for a in _AGREE:
            vals = [getattr(m, a) for m in models]
            if any(v != vals[0] for v in vals):
                raise ValueError("Ensemble: the members disagree on %s: %r" % (a, vals))
        self.models = models

    @torch.no_grad()
    def beam(self, feats, beam_width=5, max_beam_depth=30, length_alpha=0.7, n_best=1, no_repeat_ngram_size=0, repetition_penalty=1.0,
             min_length=0, banned_ids=None):
        """mode='beam' (with the constraint arguments: `beam_constrained`) over the weighted mean of the members' word
        distributions: (ids int64 [B, n_best, max_beam_depth] padded with eos_ix, lengths int64 [B, n_best], scores fp32
        [B, n_best]) on the device, best first; no host synchronisation.  Per depth: ONE policy launch, one depth step per member
        (each with its own states, workspace, decode cache and precomputed vid_rnn steps) into a shared [M, R, V] logits buffer, ONE
        ensemble head launch.  One member IS mode='beam' / beam_constrained: the same launches, the same bits."""
        import S2VTModel
        from . import functional, gru_functional, stack_functional
        from .functional import _ptr
        m0 = self.models[0]
        V = m0.vocab_size
        W, D, alpha, n_best = beam.check_beam_args(beam_width, max_beam_depth, length_alpha, n_best, V)
        spec = sampling.check_constraints(no_repeat_ngram_size, repetition_penalty, min_length, banned_ids, V, m0.eos_ix)
        constrained = sampling.constrains(spec)
        if constrained:
            beam.check_beam_constraints(spec, D, V)
        for m in self.models:
            if gru_functional.is_gru_model(m):
                raise ValueError(S2VTModel._BEAM_GRU)
            if stack_functional.is_stacked_lstm_model(m):
                raise ValueError(S2VTModel._BEAM_STACKED)
        functional.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != m0.length or feats.shape[2] != m0.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (m0.length, m0.feat_dim, tuple(feats.shape)))
        dev = feats.device
        for m in self.models:
            if any(p.device != dev for p in m.parameters()):
                raise ValueError("Ensemble: every member and feats must be on one device (feats on %s)" % (dev,))
        if len(self.models) == 1:
            if not constrained:
                return m0(feats, mode='beam', beam_width=W, max_beam_depth=D, length_alpha=alpha, n_best=n_best)
            return m0.beam_constrained(feats, beam_width=W, max_beam_depth=D, length_alpha=alpha, n_best=n_best,
                                       no_repeat_ngram_size=no_repeat_ngram_size, repetition_penalty=repetition_penalty,
                                       min_length=min_length, banned_ids=banned_ids)
        M, B = len(self.models), feats.shape[0]

        def make_depth_step(lib, R, con, policy_name):
            with torch.cuda.device(dev):
                members = [_member(lib, m, feats, D, R) for m in self.models]
                logits = torch.empty(M, R, V, dtype=torch.float32, device=dev)
            beam.LAST_PATH = "ensemble cumulative beam (%d members%s): %s" % (
                M, ", constrained" if constrained else "",
                ", ".join("plane-path depth step" + (" (vid_rnn steps precomputed)" if mb.gx_dec is not None else "")
                          if mb.cache is not None else "fp32-MFMA depth step" for mb in members))

            def depth_step(depth, rows, top_ix, top_lp, words, st):
                for mb, logits_m in zip(members, logits):
                    mb(depth, rows, st, logits=logits_m)
                if constrained:
                    capi.check(lib.s2vt_ensemble_top20_constrained(_ptr(logits), logits.stride(0), logits.stride(1), M, R, V, self.log_w,
                                                                   words[0], words[1], depth - 1, ctypes.byref(con), _ptr(top_ix),
                                                                   _ptr(top_lp), st), "s2vt_ensemble_top20_constrained")
                else:
                    capi.check(lib.s2vt_ensemble_top20(_ptr(logits), logits.stride(0), logits.stride(1), M, R, V, self.log_w, _ptr(top_ix),
                                                       _ptr(top_lp), st), "s2vt_ensemble_top20")
            return depth_step
        return beam._group_search("Ensemble", dev, B, W, 1, D, int(m0.sos_ix), int(m0.eos_ix), alpha, 0.0, n_best,
                                  spec if constrained else None, make_depth_step)
