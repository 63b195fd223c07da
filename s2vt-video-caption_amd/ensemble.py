"""Ensemble beam search: several S2VT models, ONE cumulative-score search, on the device (`S2VTModel.Ensemble`; not in the
reference; include/s2vt_hip.h "ensemble beam").

At every depth the members' word distributions are averaged (the log of the weighted arithmetic mean of their probabilities) and
mode='beam''s policy runs over the average.  What belongs to one model stays per member - encoder states, decode cache, workspace,
state tables and the depth step, stopped one launch early so that the member leaves its logits on the card (s2vt_beam_step_logits) -
and what does not is shared: the policy kernel (csrc/beam_cum.hip), the polled early exit, the result kernel, and ONE fan-out head
per depth over the [M, R, V] logits (csrc/ensemble.hip).  Nothing crosses PCIe per depth.
"""
import ctypes

import torch

from . import beam, capi, ops, sampling

MAX_MEMBERS = 8
_AGREE = ("vocab_size", "length", "feat_dim", "sos_ix", "eos_ix")


class _Member(object):
    """what one member owns in a search: its parameters, dims, decode cache, workspace, vid_rnn states and word_rnn state tables"""

    def __init__(self, lib, model, feats, D, R):
        from . import functional
        from .functional import _dims, _params_struct
        dev = feats.device
        B, H = feats.shape[0], model.dim_hid
        feats = model.feat_drop(feats)
        params = model._hip_params()
        vid_h, vid_c, word_h, word_c, gx_dec = beam._encoder_states(model, feats, params, D, beam.PLANE_STEP and beam.PLANE_ENCODER)
        self.pcs = tuple(p.detach().contiguous() for p in params)
        self.d = _dims(feats, self.pcs)
        self.ps = _params_struct(capi.Params, self.pcs)
        # the decode cache of the member's weights, filled by one greedy decode where it is not there yet (beam._device_depth_loop)
        cache = None
        if beam.PLANE_STEP:
            cache, valid = functional.decode_cache_entry(model, params, self.d, dev, lib)
            if cache is not None and not valid:
                functional.greedy_decode(feats, params, int(model.sos_ix), owner=model)
                cache, valid = functional.decode_cache_entry(model, params, self.d, dev, lib)
                if not valid:
                    cache = None
        self.cache = cache
        self.gx_dec = gx_dec if cache is not None else None
        self.nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(self.d), R)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.vid = [(vid_h.contiguous(), vid_c.contiguous()), (torch.empty(B, H, device=dev), torch.empty(B, H, device=dev))]
        self.tab = [(torch.zeros(R, H, device=dev), torch.zeros(R, H, device=dev)) for _ in range(2)]
        self.tab[0][0][:B].copy_(word_h)
        self.tab[0][1][:B].copy_(word_c)

    def step(self, lib, depth, R, rows, logits_m, st):
        """the member's depth step up to its logits: [R, V] into logits_m"""
        from .functional import _ptr
        (vh_in, vc_in), (vh_out, vc_out) = self.vid[(depth - 1) & 1], self.vid[depth & 1]
        (wh_in, wc_in), (wh_out, wc_out) = self.tab[(depth - 1) & 1], self.tab[depth & 1]
        gx = self.gx_dec[depth - 1] if self.gx_dec is not None else None
        capi.check(lib.s2vt_beam_step_logits(ctypes.byref(self.d), ctypes.byref(self.ps), R, _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]),
                                             _ptr(vh_in), _ptr(vc_in), _ptr(vh_out), _ptr(vc_out), _ptr(gx), _ptr(wh_in), _ptr(wc_in),
                                             _ptr(wh_out), _ptr(wc_out), _ptr(logits_m), logits_m.stride(0), _ptr(self.ws), self.nbytes,
                                             _ptr(self.cache), self.cache.numel() if self.cache is not None else 0, st),
                   "s2vt_beam_step_logits")


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
        from .functional import _ptr, _stream
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
        M, B, R = len(self.models), feats.shape[0], feats.shape[0] * W
        sos, eos = int(m0.sos_ix), int(m0.eos_ix)
        lib = capi.load()
        qbytes = (lib.s2vt_beam_cum_hist_bytes if constrained else lib.s2vt_beam_cum_bytes)(B, W, D)
        if qbytes == 0:
            raise ValueError("Ensemble: batch %d x beam_width %d x max_beam_depth %d is more than the search state holds" % (B, W, D))
        with torch.cuda.device(dev):
            members = [_Member(lib, m, feats, D, R) for m in self.models]
            beam.LAST_PATH = "ensemble cumulative beam (%d members%s): %s" % (
                M, ", constrained" if constrained else "",
                ", ".join("plane-path depth step" + (" (vid_rnn steps precomputed)" if mb.gx_dec is not None else "")
                          if mb.cache is not None else "fp32-MFMA depth step" for mb in members))
            con = keep = None
            if constrained:
                con, keep = sampling.constraints_struct(spec)     # (keep: the banned ids' host array lives as long as con is used)
            words, words_ld = ctypes.c_void_p(), ctypes.c_int64()
            qs = torch.empty(qbytes, dtype=torch.uint8, device=dev)
            rows = torch.zeros(3, R, dtype=torch.int32, device=dev)
            top_ix = torch.zeros(R, beam.FANOUT, dtype=torch.int32, device=dev)
            top_lp = torch.zeros(R, beam.FANOUT, dtype=torch.float32, device=dev)
            logits = torch.empty(M, R, V, dtype=torch.float32, device=dev)
            st = _stream(dev)

            def policy(depth):
                if constrained:
                    capi.check(lib.s2vt_beam_cum_hist_step(B, W, D, sos, eos, alpha, depth, _ptr(qs), qbytes, _ptr(top_ix), _ptr(top_lp),
                                                           _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), ctypes.byref(words),
                                                           ctypes.byref(words_ld), st), "s2vt_beam_cum_hist_step")
                else:
                    capi.check(lib.s2vt_beam_cum_step(B, W, D, sos, eos, alpha, depth, _ptr(qs), qbytes, _ptr(top_ix), _ptr(top_lp),
                                                      _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), st), "s2vt_beam_cum_step")

            # the depth loop of beam._device_depth_loop (the early exit polled one depth late through pinned memory), with M depth
            # steps and the ensemble head where that loop has one depth step
            frozen = torch.zeros(D + 2, dtype=torch.int32).pin_memory()
            frozen_dev = qs[:4].view(torch.int32)
            events = []
            depth = 0
            while depth < D:
                if depth >= 2 and events[depth - 2].query() and int(frozen[depth - 1]) == B:
                    break
                depth += 1
                policy(depth)
                if depth > 1:
                    frozen[depth].copy_(frozen_dev[0], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                events.append(ev)
                for i, mb in enumerate(members):
                    mb.step(lib, depth, R, rows, logits[i], st)
                if constrained:
                    capi.check(lib.s2vt_ensemble_top20_constrained(_ptr(logits), logits.stride(0), logits.stride(1), M, R, V, self.log_w,
                                                                   ctypes.c_void_p(words.value), words_ld.value, depth - 1,
                                                                   ctypes.byref(con), _ptr(top_ix), _ptr(top_lp), st),
                               "s2vt_ensemble_top20_constrained")
                else:
                    capi.check(lib.s2vt_ensemble_top20(_ptr(logits), logits.stride(0), logits.stride(1), M, R, V, self.log_w, _ptr(top_ix),
                                                       _ptr(top_lp), st), "s2vt_ensemble_top20")
            policy(0)                                             # the last depth's results
            beam.LAST_DEPTHS = depth
            ids = torch.empty(B, n_best, D, dtype=torch.int32, device=dev)
            lens = torch.empty(B, n_best, dtype=torch.int32, device=dev)
            scores = torch.empty(B, n_best, dtype=torch.float32, device=dev)
            capi.check(lib.s2vt_beam_cum_result(B, W, D, eos, n_best, _ptr(qs), qbytes, _ptr(ids), _ptr(lens), _ptr(scores), st),
                       "s2vt_beam_cum_result")
            return ids.long(), lens.long(), scores
