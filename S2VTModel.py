"""Drop-in `S2VTModel` module for Kamino666/S2VT-video-caption, MI355X-native.

Same module name, class name, constructor and `forward` signature, sub-module names/types and
attributes as the reference (S2VTModel.py:10-37), so `torch.load` of reference full-module pickles,
`load_state_dict`, optimisers and the reference's train/eval scripts work unchanged.  The arithmetic
of `forward` does not go through `nn.LSTM`/`nn.Linear`: it is executed by hand-written HIP kernels
behind the C ABI in `include/s2vt_hip.h`.  The `nn.*` sub-modules are parameter
containers only.  HIP tensors only — there is no CPU fallback.
"""
import torch
from torch import nn

import s2vt_video_caption_amd  # noqa: F401  (registers the package alias)
from s2vt_video_caption_amd import capi as _capi
from s2vt_video_caption_amd import functional as _F
from s2vt_video_caption_amd import beam as _beam
from s2vt_video_caption_amd import gru_functional as _G
from s2vt_video_caption_amd import stack_functional as _S
from s2vt_video_caption_amd import sampling as _sampling
from s2vt_video_caption_amd import score as _score


# what mode='beam' and beam_constrained say to the models the batched depth step does not serve
_BEAM_GRU = "mode='beam' of a GRU model: the batched depth step is the LSTM's; use mode='test'"
_BEAM_STACKED = "mode='beam' of a stacked model (num_layers > 1): the batched depth step is the one-layer LSTM's; use mode='test'"


class S2VT(nn.Module):
    def __init__(self, vocab_size, feat_dim, length, dim_hid=500, dim_embed=500, feat_dropout=0, rnn_dropout=0,
                 out_dropout=0, num_layers=1, bidirectional=False, rnn_type='lstm', sos_ix=3, eos_ix=4):
        super(S2VT, self).__init__()
        # construction order = the reference's (S2VTModel.py:19-28) so seeded default init matches
        rnn_cell = nn.LSTM if rnn_type.lower() == 'lstm' else nn.GRU
        self.vid_rnn = rnn_cell(dim_hid, dim_hid, batch_first=True, num_layers=num_layers,
                                bidirectional=bidirectional, dropout=rnn_dropout)
        self.word_rnn = rnn_cell(dim_hid + dim_embed, dim_hid, batch_first=True, num_layers=num_layers,
                                 bidirectional=bidirectional, dropout=rnn_dropout)
        self.feat_drop = nn.Dropout(p=feat_dropout)
        self.out_drop = nn.Dropout(p=out_dropout)
        self.feat_linear = nn.Linear(feat_dim, dim_hid)
        self.out_linear = nn.Linear(dim_hid, vocab_size)
        self.embedding = nn.Embedding(vocab_size, dim_embed)
        self.feat_dim = feat_dim
        self.length = length
        self.dim_hid = dim_hid
        self.dim_embed = dim_embed
        self.sos_ix = sos_ix
        self.eos_ix = eos_ix
        self.vocab_size = vocab_size
        self.rnn_type = rnn_type

    # -- the 13 tensors in include/s2vt_hip.h order
    def _hip_params(self):
        self._check_supported()
        return (self.vid_rnn.weight_ih_l0, self.vid_rnn.weight_hh_l0, self.vid_rnn.bias_ih_l0,
                self.vid_rnn.bias_hh_l0, self.word_rnn.weight_ih_l0, self.word_rnn.weight_hh_l0,
                self.word_rnn.bias_ih_l0, self.word_rnn.bias_hh_l0, self.feat_linear.weight,
                self.feat_linear.bias, self.out_linear.weight, self.out_linear.bias, self.embedding.weight)

    def _check_supported(self):
        for rnn in (self.vid_rnn, self.word_rnn):
            if not isinstance(rnn, nn.LSTM) or rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias:
                raise NotImplementedError(
                    "the HIP S2VT whole-path drivers implement the reference configuration (1-layer unidirectional LSTM); "
                    "a 1-layer GRU model runs through forward() on the GRU timestep kernels (gru_functional.py), a stacked "
                    "LSTM (num_layers>1) on the layer-wavefront kernels (stack_functional.py); stacked GRU and bidirectional "
                    "models are not implemented (the reference's forward fails on a bidirectional model: word_rnn expects "
                    "dim_embed + dim_hid inputs and gets dim_embed + 2*dim_hid)")

    def forward(self, feats, targets=None, mode='train', beam_width=3, max_beam_depth=30, ss_prob=0.0, ss_temperature=None,
                length_alpha=0.7, n_best=1, temperature=1.0, seed=None):
        """
        :param feats: [B, L, feat_dim]
        :param targets: [B, L-1] word ids (train mode); or [B, K, L-1] (any strides, an expanded view is read as it is): K captions
                     per clip (not in the reference) -> logits [B, K, L-1, V], those of the call on feats.repeat_interleave(K, 0)
                     with targets.reshape(B*K, L-1), and its gradients (feats.grad summed over a clip's K rows).  The one-layer
                     LSTM encodes every clip once (functional.train_forward_group); a GRU or stacked model runs the repeated
                     clips.  feat_drop is drawn once per clip, out_drop on [B*K, L-1, H]; ss_prob > 0 is refused
        :param mode: 'train' -> logits [B, L-1, V]; 'test' -> greedy ids [B, L-1] (int64);
                     'beam_search' -> list of id sequences (each starting with <sos>): the reference's search, score = the LAST
                     token's log-prob / len**0.7;
                     'beam' -> (ids int64 [B, n_best, max_beam_depth], lengths int64 [B, n_best], scores fp32 [B, n_best]) on the
                     device, best first: hypotheses ranked by the SUM of their tokens' log-probs, divided by
                     length**length_alpha when they end (<eos>, or max_beam_depth words); ids are the words after <sos>, padded
                     with eos_ix; lengths count the <eos> where there is one (not in the reference; beam.beam_cumulative);
                     'sample' -> ids [B, L-1] (int64) drawn step by step from softmax(logit / temperature), never stopping at
                     <eos> (not in the reference; for sequence-level training, utils.RewardCriterion);
                     'score' -> (scores fp32 [B(, K)], lengths int64 [B(, K)], token_logprobs fp32 [B(, K), T-1]) on the device:
                     the log-likelihood of the GIVEN captions `targets`, int64 [B, T] or [B, K, T] (K candidates per clip, which
                     share one encode; an expanded view is fine), each <sos>, words, <eos>, padding with 2 <= T <= length.
                     token_logprobs[j] = log_softmax(logits of mode='train' without dropout)[targets[j + 1]] up to and including
                     the first <eos> (0 behind), lengths counts those tokens, scores = their sum / length**length_alpha - the
                     rule of mode='beam', whose scores are directly comparable at the same length_alpha (the signature's default
                     is 0.7; pass length_alpha=0.0 for the plain log-likelihood).  No gradient (not in the reference;
                     score.score_captions)
        :param beam_width: 'beam_search': any; 'beam': 1..8
        :param length_alpha: mode='beam' and mode='score' only: finite and >= 0 (0: the plain sum)
        :param n_best: mode='beam' only: hypotheses returned per clip, 1..beam_width
        :param temperature: mode='sample' only: finite and > 0
        :param seed: mode='sample' and scheduled sampling: None draws a 63-bit seed from torch's default generator
                     (torch.manual_seed makes the run reproducible); an int is used as is.  Same seed, same weights, same clips ->
                     same ids.
        :param ss_prob: mode='train' only - scheduled sampling (Bengio et al., 2015; not in the reference): each decode-step input
                     is, with this probability, the word the model itself chose at the previous step instead of targets' (the
                     first, <sos>, is always targets').  The words are fixed by one decode pass without gradient, dropout or host
                     round trip (functional.scheduled_inputs), then the usual train forward runs on them.  0 (default): plain
                     teacher forcing, nothing else is run.  Must be in [0, 1].
        :param ss_temperature: the model's choice in that pass: None = the arg-max, a number = a draw from
                     softmax(logit / ss_temperature)
        """
        ss_prob = _F.check_ss_prob(ss_prob) if mode == 'train' else 0.0      # (ignored elsewhere, as temperature is outside 'sample')
        if mode == 'beam':
            _beam.check_beam_args(beam_width, max_beam_depth, length_alpha, n_best, self.vocab_size)
        if mode == 'score':                                # (shape checks again, with the dims, in score.score_captions)
            _score.check_score_args(targets, feats.shape[0] if isinstance(feats, torch.Tensor) and feats.dim() else -1, self.length,
                                    None, length_alpha)
        # K captions per clip (not in the reference): 3-D targets [B, K, L-1] -> logits [B, K, L-1, V] on one encode per clip
        grouped = mode == 'train' and isinstance(targets, torch.Tensor) and targets.dim() == 3
        if grouped:
            if ss_prob > 0:
                raise ValueError("scheduled sampling (ss_prob > 0) is not implemented for K captions per clip (3-D targets)")
            nb = feats.shape[0] if isinstance(feats, torch.Tensor) and feats.dim() == 3 else -1
            if targets.shape[0] != nb or targets.shape[1] < 1 or targets.shape[2] != self.length - 1:
                raise ValueError("targets must be [B, K, L-1] = [%d, K >= 1, %d], got %s" % (nb, self.length - 1, tuple(targets.shape)))
        _F.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != self.length or feats.shape[2] != self.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (self.length, self.feat_dim, tuple(feats.shape)))
        sample = _sampling.check_sample_args(temperature, seed) if mode == 'sample' else None
        if grouped and (_G.is_gru_model(self) or _S.is_stacked_lstm_model(self)):
            # no shared encode on these paths: the repeated clips (as S2VT.sample runs them), feat_drop drawn once per clip
            _F.require_hip(targets, "targets")
            B, K = targets.shape[0], targets.shape[1]
            run = self._forward_gru if _G.is_gru_model(self) else self._forward_stacked
            out = run(self.feat_drop(feats).repeat_interleave(K, 0), targets.reshape(B * K, -1), mode, None, (0.0, None, None),
                      drop_feats=False)
            return out.view(B, K, self.length - 1, -1)
        if _G.is_gru_model(self):
            return self._forward_gru(feats, targets, mode, sample, (ss_prob, ss_temperature, seed))
        if _S.is_stacked_lstm_model(self):
            return self._forward_stacked(feats, targets, mode, sample, (ss_prob, ss_temperature, seed))
        params = self._hip_params()
        if mode == 'score':                                # (inference arithmetic whatever self.training says: no feat_drop draw)
            return _score.score_captions(self, feats, targets, params, length_alpha=length_alpha)
        clean = feats                                      # (the scheduled pass runs without dropout)
        feats = self.feat_drop(feats)                      # identity at the reference's p=0 (S2VTModel.py:52)
        if mode == 'beam_search':
            return _beam.beam_search(self, feats, params, beam_width=beam_width, max_depth=max_beam_depth)
        if mode == 'beam':
            return _beam.beam_cumulative(self, feats, params, beam_width=beam_width, max_depth=max_beam_depth,
                                         length_alpha=length_alpha, n_best=n_best)
        if mode == 'train':
            if targets is None:
                raise ValueError("mode='train' needs targets")
            if ss_prob > 0:
                targets = _F.scheduled_inputs(clean, targets, params, ss_prob, temperature=ss_temperature, seed=seed, owner=self)
            if grouped:
                # every clip encoded once (feat_drop drawn once per clip, above); the out_drop mask is the draw the call on the
                # repeated clips would make: nn.Dropout on a [B*K, L-1, H] ones tensor, time-major for the kernels
                out_mask = None
                if self.training and self.out_drop.p > 0:
                    R, H = feats.shape[0] * targets.shape[1], self.dim_hid
                    keep = self.out_drop(torch.ones(R, self.length - 1, H, dtype=torch.float32, device=feats.device))
                    out_mask = keep.transpose(0, 1).reshape((self.length - 1) * R, H).contiguous()
                return _F.train_forward_group(feats, targets, params, grad_sink=_F.grad_sink_for(self), out_mask=out_mask)
            out_mask = None
            if self.training and self.out_drop.p > 0:
                # S2VTModel.py:79 applies nn.Dropout to the [B, L-1, H] decode-step hidden states: the same call on a ones
                # tensor of that shape draws the same mask from torch's generator; the kernels want it time-major
                B, H = feats.shape[0], self.dim_hid
                keep = self.out_drop(torch.ones(B, self.length - 1, H, dtype=torch.float32, device=feats.device))
                out_mask = keep.transpose(0, 1).reshape((self.length - 1) * B, H).contiguous()
            return _F.train_forward(feats, targets, params, grad_sink=_F.grad_sink_for(self), out_mask=out_mask)
        elif mode == 'test':
            return _F.greedy_decode(feats, params, self.sos_ix, owner=self)
        elif mode == 'sample':
            return _F.greedy_decode(feats, params, self.sos_ix, owner=self, sample=sample)
        return None                                        # the reference falls through for unknown modes

    @torch.no_grad()
    def sample(self, feats, n_samples=1, temperature=1.0, seed=None):
        """ids int64 [B, n_samples, L-1] on the device: K = n_samples captions per clip drawn as mode='sample' draws them (never
        stopping at <eos>), for sequence-level training with K samples per clip (not in the reference).  Row b*K + k draws with
        the noise of (seed, decode step, batch row b*K + k, v), so `sample(feats, K, t, s).view(B*K, -1)` is the draw of
        `forward(feats.repeat_interleave(K, 0), mode='sample', temperature=t, seed=s)` - the two can differ only where two scores
        are closer than the paths' logit rounding - and K = 1 is mode='sample' with a middle axis of 1.  The one-layer LSTM
        encodes every clip ONCE and runs only the word steps over the B*K rows (sampling.sample_rows); a GRU or stacked model
        gives the same ids by decoding the repeated clips, without the shared encode.  feat_drop is applied once per clip, as
        forward applies it; temperature / seed as for mode='sample'.  No gradient.
        :param feats: [B, L, feat_dim]
        :param n_samples: an integer >= 1
        """
        return self._sample(feats, n_samples, temperature, seed, 0, 1.0)

    @torch.no_grad()
    def sample_truncated(self, feats, n_samples=1, temperature=1.0, seed=None, top_k=0, top_p=1.0):
        """`sample` with top-k / nucleus (top-p) truncation: ids int64 [B, n_samples, L-1], every word drawn from its step's
        softmax(logit / temperature) cut to the top_k largest scores (equal values at the k-th place all stay) and then to the
        nucleus - the shortest descending prefix whose mass, renormalised over the top-k set, reaches top_p (the rule: sampling.py,
        include/s2vt_hip.h "truncated draw").  Same rows, same noise as `sample`: row b*K + k draws with the noise of (seed, decode
        step, batch row b*K + k, v), so n_samples = 1 (and [:, 0]) is mode='sample' with truncation.  The fused sampling heads
        cannot truncate; per step the one-layer LSTM runs the logits GEMM and the row kernel of csrc/truncate.hip in `sample`'s
        driver (s2vt_sample_decode_rows_trunc), a GRU or stacked model the same pair in its step loop on the repeated clips.
        top_k=0, top_p=1.0 (the defaults) truncate nothing and run exactly what `sample` runs.  A method of its own: the parameter
        lists of forward and sample are fixed.  No gradient.
        :param top_k: an int in [0, vocab_size]; 0 (or vocab_size): off
        :param top_p: in (0, 1]; 1.0: off
        """
        k, p = _sampling.check_truncation(top_k, top_p, self.vocab_size)
        return self._sample(feats, n_samples, temperature, seed, k, p)

    @torch.no_grad()
    def decode_constrained(self, feats, n_samples=1, temperature=None, seed=None, top_k=0, top_p=1.0, no_repeat_ngram_size=0,
                           repetition_penalty=1.0, min_length=0, banned_ids=None):
        """Greedy or sampled decoding under constraints (not in the reference): ids int64 [B, n_samples, L-1] on the device, never
        stopping at <eos> (callers cut behind it).  Per step, on the raw logits of a row and in this order (the rule: sampling.py,
        include/s2vt_hip.h "constrained draw"): the repetition penalty (every distinct word generated so far: a positive logit is
        divided by repetition_penalty, any other multiplied), no-repeat n-gram blocking (a word that would complete an n-gram the
        row already holds gets -inf), the banned ids (-inf), and <eos> at -inf during the first min_length words.  Then the arg-max
        (temperature=None: greedy, which needs n_samples == 1, top_k == 0, top_p == 1.0) or `sample_truncated`'s draw with the same
        rows and noise.  The constraints run inside the row kernel of csrc/truncate.hip behind the logits GEMM: the one-layer LSTM
        in `sample`'s driver (s2vt_decode_rows_constrained), a GRU or stacked model in its step loop on the repeated clips.  With
        the constraints at their defaults nothing is constrained: greedy returns mode='test' (with a middle axis of 1), sampled
        what `sample_truncated` returns.  Not covered: mode='beam' (that is `beam_constrained`), Att_Baseline, scheduled sampling, dp.py.  No gradient.
        :param no_repeat_ngram_size: an int >= 0; 0: off, 1: no word twice
        :param repetition_penalty: finite and >= 1; 1.0: off
        :param min_length: an int >= 0: no <eos> among the first min_length words
        :param banned_ids: up to 32 word ids that are never generated
        """
        greedy = temperature is None
        K = _sampling.check_n_samples(n_samples)
        k, p = _sampling.check_truncation(top_k, top_p, self.vocab_size)
        if greedy and (K != 1 or k != 0 or p != 1.0):
            raise ValueError("greedy decoding (temperature=None) needs n_samples == 1, top_k == 0 and top_p == 1.0")
        spec = _sampling.check_constraints(no_repeat_ngram_size, repetition_penalty, min_length, banned_ids, self.vocab_size, self.eos_ix,
                                           length=self.length)
        t, s = (1.0, 0) if greedy else _sampling.check_sample_args(temperature, seed)
        _F.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != self.length or feats.shape[2] != self.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (self.length, self.feat_dim, tuple(feats.shape)))
        if not _sampling.constrains(spec):                 # nothing to constrain: today's calls
            return self(feats, mode='test').unsqueeze(1) if greedy else self._sample(feats, K, t, s, k, p)
        B = feats.shape[0]
        if _G.is_gru_model(self) or _S.is_stacked_lstm_model(self):
            decode = _G.greedy_decode if _G.is_gru_model(self) else _S.greedy_decode
            rows = self.feat_drop(feats).repeat_interleave(K, 0)
            smp = None if greedy else ((t, s, k, p) if _sampling.truncates(k, p, self.vocab_size) else (t, s))
            return decode(self, rows, self.sos_ix, sample=smp, constraints=spec).view(B, K, -1)
        return _sampling.sample_rows(self, self.feat_drop(feats), self._hip_params(), K, t, s, k, p, constraints=(spec, greedy))

    @torch.no_grad()
    def beam_constrained(self, feats, beam_width=3, max_beam_depth=30, length_alpha=0.7, n_best=1, no_repeat_ngram_size=0,
                         repetition_penalty=1.0, min_length=0, banned_ids=None):
        """mode='beam' under the constraints of `decode_constrained` (not in the reference): (ids int64 [B, n_best, max_beam_depth]
        padded with eos_ix, lengths int64 [B, n_best], scores fp32 [B, n_best]) on the device, best first, as mode='beam' returns
        them.  The search is mode='beam''s with one change (include/s2vt_hip.h "constrained beam"): at every
        depth each live hypothesis's raw logits row is first edited with the hypothesis's OWN words as history - the repetition
        penalty on every distinct word, -inf on a word that would complete an n-gram it already holds, -inf on the banned ids, -inf
        on <eos> during its first min_length words (sampling.constrain_logits, bit for bit) - and its log-probs are log_softmax of
        the edited row, renormalised over the surviving words.  Scores, tie rules, the pool, length_alpha and n_best are
        mode='beam''s.  The policy kernel keeps every beam slot's words on the device (csrc/beam_policy.hip), the depth step's fan-out
        kernel applies the rules in front of its top 20 (csrc/ce.hip): no host round trip per depth.  With the constraints at
        their defaults the call IS mode='beam' (the same launches, the same bits).  beam_width = 1, length_alpha = 0 gives greedy
        `decode_constrained` up to the first <eos>.  One-layer LSTM models only (a GRU or stacked model: ValueError with mode='beam''s
        message).  A method of its own: forward's parameter list is fixed.  Not covered: mode='beam_search', GRU and stacked
        models, Att_Baseline, dp.py.  No gradient.
        :param beam_width, max_beam_depth, length_alpha, n_best: as for mode='beam'; max_beam_depth <= 1023 and
                     vocab_size >= 20 + max_beam_depth + len(banned_ids) + 1 (every edited row keeps 20 words for the fan-out)
        :param no_repeat_ngram_size, repetition_penalty, min_length, banned_ids: as for decode_constrained
        """
        _beam.check_beam_args(beam_width, max_beam_depth, length_alpha, n_best, self.vocab_size)
        spec = _sampling.check_constraints(no_repeat_ngram_size, repetition_penalty, min_length, banned_ids, self.vocab_size, self.eos_ix)
        _beam.check_beam_constraints(spec, max_beam_depth, self.vocab_size)
        if _G.is_gru_model(self):
            raise ValueError(_BEAM_GRU)
        if _S.is_stacked_lstm_model(self):
            raise ValueError(_BEAM_STACKED)
        if not _sampling.constrains(spec):                 # nothing to constrain: today's call
            return self(feats, mode='beam', beam_width=beam_width, max_beam_depth=max_beam_depth, length_alpha=length_alpha, n_best=n_best)
        _F.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != self.length or feats.shape[2] != self.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (self.length, self.feat_dim, tuple(feats.shape)))
        return _beam.beam_cumulative(self, self.feat_drop(feats), self._hip_params(), beam_width=beam_width, max_depth=max_beam_depth,
                                     length_alpha=length_alpha, n_best=n_best, constraints=spec)

    @torch.no_grad()
    def beam_diverse(self, feats, beam_width=6, num_groups=3, diversity_lambda=0.5, max_beam_depth=30, length_alpha=0.7, n_best=1,
                     no_repeat_ngram_size=0, repetition_penalty=1.0, min_length=0, banned_ids=None):
        """Diverse (group) beam search (Vijayakumar et al., 2016; not in the reference): captions that differ on purpose.  Returns
        (ids int64 [B, num_groups, n_best, max_beam_depth] padded with eos_ix, lengths int64 [B, num_groups, n_best], scores fp32
        [B, num_groups, n_best]) on the device, every group best first; no host synchronisation.  The beam_width slots are split
        into num_groups groups of Wg = beam_width / num_groups.  At every depth the groups select one after the other, each the Wg
        best candidates of its OWN live hypotheses by (sum of log-probs) - diversity_lambda * (how many candidates chosen by the
        earlier groups at this depth carry the same word: Hamming diversity on the current word; <eos> counts like any word), ties
        by (slot, token) as in mode='beam'.  The penalty steers the selection only: a hypothesis carries, and is pooled with, its
        unpenalised sum, so scores are mode='beam''s (sum / length**length_alpha) and comparable with mode='score'.  Every group
        has a pool of its own; group 0 is never penalised and is exactly mode='beam' at width Wg, and diversity_lambda = 0 makes
        every group that search.  num_groups = 1 IS mode='beam' (or `beam_constrained`) with an axis of 1 inserted: the same
        launches, the same bits.  The constraint arguments are `beam_constrained`'s: every live hypothesis's logits row is edited
        with its own words in front of its log_softmax.  The policy runs on the device (csrc/beam_policy.hip; include/s2vt_hip.h
        "diverse beam"), one launch per depth beside mode='beam''s depth step.  One-layer LSTM models only (a GRU
        or stacked model: ValueError with mode='beam''s message).  A method of its own: forward's parameter list is fixed.  Not
        covered: mode='beam_search', GRU and stacked models, Att_Baseline, dp.py, the groups as samples of --self-critical,
        dissimilarity measures other than Hamming on the current word, widths above 8.  No gradient.
        :param beam_width: 1..8, a multiple of num_groups
        :param num_groups: 1..beam_width
        :param diversity_lambda: finite and >= 0
        :param n_best: hypotheses returned per group, 1..beam_width / num_groups
        :param max_beam_depth, length_alpha: as for mode='beam'; with constraints the shape rules of `beam_constrained`
        :param no_repeat_ngram_size, repetition_penalty, min_length, banned_ids: as for decode_constrained
        """
        _beam.check_beam_args(beam_width, max_beam_depth, length_alpha, 1, self.vocab_size)
        _beam.check_diverse_args(beam_width, num_groups, diversity_lambda, n_best)
        spec = _sampling.check_constraints(no_repeat_ngram_size, repetition_penalty, min_length, banned_ids, self.vocab_size, self.eos_ix)
        if _sampling.constrains(spec):
            _beam.check_beam_constraints(spec, max_beam_depth, self.vocab_size)
        if _G.is_gru_model(self):
            raise ValueError(_BEAM_GRU)
        if _S.is_stacked_lstm_model(self):
            raise ValueError(_BEAM_STACKED)
        _F.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != self.length or feats.shape[2] != self.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (self.length, self.feat_dim, tuple(feats.shape)))
        return _beam.beam_diverse(self, self.feat_drop(feats), self._hip_params(), beam_width=beam_width, num_groups=num_groups,
                                  diversity_lambda=diversity_lambda, max_depth=max_beam_depth, length_alpha=length_alpha, n_best=n_best,
                                  constraints=spec)

    @torch.no_grad()
    def sample_distinct(self, feats, n_samples=5, temperature=1.0, seed=None, max_depth=30):
        """Stochastic beam search (Kool, van Hoof, Welling, ICML 2019; not in the reference): n_samples captions per clip that are
        guaranteed PAIRWISE DISTINCT - sampled WITHOUT replacement from the model's distribution over whole sentences at
        `temperature`, in the exact order a sequential without-replacement sampler would draw them.  `sample` draws its K rows
        independently, and a peaked model returns mostly copies; this returns K different sentences on one encode.  Returns
        (ids int64 [B, n_samples, max_depth] - the words after <sos>, padded with eos_ix, lengths int64 [B, n_samples] - counting the
        <eos> where there is one; a sample still unfinished at max_depth has length max_depth and no <eos>, logprobs fp32
        [B, n_samples] - the sum of the words' log-probs under softmax(logit / temperature), mode='score' with length_alpha=0.0 at
        temperature 1, perturbed fp32 [B, n_samples] - the samples' perturbed scores G, non-increasing along a clip's row and <= 0,
        kappa fp32 [B] - the largest perturbed score that was NOT kept, <= perturbed[:, -1]: the threshold of the inclusion
        probabilities q = 1 - exp(-exp(logprob - kappa)) of importance-weighted estimators: a caption is kept when its Gumbel(logprob)
        score exceeds kappa; self_critical.inclusion_log_q) on the device; no host synchronisation.
        The search (include/s2vt_hip.h "stochastic beam") is beam-shaped: mode='beam''s encoder states, decode
        cache and depth step over the rows b * n_samples + slot; the fan-out head ranks a row's words by log-prob + Gumbel noise
        (csrc/gumbel_top.hip; the counter-based noise of mode='sample', keyed by seed, depth, row and word), the policy keeps the
        n_samples best children by the perturbed score conditioned on their parent's (csrc/sbs_policy.hip, fp64), one launch each per
        depth.  n_samples = 1 is ancestral sampling: ids[:, 0] are the words of `sample(feats, 1, temperature, seed)` up to the first
        <eos>, wherever a draw is decided.  Same seed, same weights, same clips -> the same bits.  One-layer LSTM models only (a GRU or
        stacked model: ValueError naming `sample`).  A method of its own: the parameter lists of forward and sample are fixed.  Not
        covered: top-k / nucleus truncation and the constraint rules inside this search, GRU, stacked and Att_Baseline models,
        Ensemble, widths above 8, dp.py (kappa in training: train.py --sc-distinct, ops.sc_weights_swor).  No gradient.
        :param n_samples: an integer in [1, 8]
        :param temperature: finite and > 0
        :param seed: None draws a 63-bit seed from torch's default generator, as `sample` does; an int is used as is
        :param max_depth: an integer >= 1: the most words a sample gets
        """
        W, t, s, D = _beam.check_stochastic_args(n_samples, temperature, seed, max_depth, self.vocab_size)
        if _G.is_gru_model(self):
            raise ValueError("sample_distinct of a GRU model: the batched depth step is the LSTM's; use sample")
        if _S.is_stacked_lstm_model(self):
            raise ValueError("sample_distinct of a stacked model (num_layers > 1): the batched depth step is the one-layer LSTM's; use sample")
        _F.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != self.length or feats.shape[2] != self.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (self.length, self.feat_dim, tuple(feats.shape)))
        return _beam.stochastic(self, self.feat_drop(feats), self._hip_params(), n_samples=W, temperature=t, seed=s, max_depth=D)

    def _sample(self, feats, n_samples, temperature, seed, k, p):
        K = _sampling.check_n_samples(n_samples)
        t, s = _sampling.check_sample_args(temperature, seed)
        _F.require_hip(feats, "feats")
        if feats.dim() != 3 or feats.shape[1] != self.length or feats.shape[2] != self.feat_dim:
            raise ValueError("feats must be [B, %d, %d], got %s" % (self.length, self.feat_dim, tuple(feats.shape)))
        B = feats.shape[0]
        if _G.is_gru_model(self) or _S.is_stacked_lstm_model(self):
            decode = _G.greedy_decode if _G.is_gru_model(self) else _S.greedy_decode
            rows = self.feat_drop(feats).repeat_interleave(K, 0)
            smp = (t, s, k, p) if _sampling.truncates(k, p, self.vocab_size) else (t, s)
            return decode(self, rows, self.sos_ix, sample=smp).view(B, K, -1)
        params = self._hip_params()
        return _sampling.sample_rows(self, self.feat_drop(feats), params, K, t, s, k, p)

    def _forward_gru(self, feats, targets, mode, sample=None, ss=(0.0, None, None), drop_feats=True):
        """rnn_type='gru' with one unidirectional layer: the GRU timestep kernels under autograd glue (gru_functional.py)"""
        if mode == 'beam_search':
            raise NotImplementedError("beam search of a GRU model: the reference's beam search does not support GRU either "
                                      "(S2VTModel.py:153, 'DO NOT SUPPORT GRU'); use mode='test'")
        if mode == 'beam':
            raise NotImplementedError(_BEAM_GRU)
        if mode == 'score':
            raise NotImplementedError("mode='score' of a GRU model: the scoring driver's word step is the LSTM's; take the logits "
                                      "of mode='train' and log_softmax(...).gather(...) them")
        clean = feats                                      # (the scheduled pass runs without dropout)
        feats = self.feat_drop(feats) if drop_feats else feats      # S2VTModel.py:52 (drop_feats False: the caller drew it)
        if mode == 'train':
            if targets is None:
                raise ValueError("mode='train' needs targets")
            _F.require_hip(targets, "targets")
            if ss[0] > 0:
                targets = _G.scheduled_inputs(self, clean, targets.reshape(targets.shape[0], -1), ss[0], temperature=ss[1], seed=ss[2])
            out_mask = None
            if self.training and self.out_drop.p > 0:
                # the LSTM path's draw (S2VTModel.py:79): nn.Dropout on a [B, L-1, H] ones tensor, batch-major as the GRU path uses it
                out_mask = self.out_drop(torch.ones(feats.shape[0], self.length - 1, self.dim_hid, dtype=torch.float32,
                                                    device=feats.device))
            return _G.train_forward(self, feats, targets.reshape(targets.shape[0], -1), out_mask=out_mask)
        elif mode == 'test':
            return _G.greedy_decode(self, feats, self.sos_ix)
        elif mode == 'sample':
            return _G.greedy_decode(self, feats, self.sos_ix, sample=sample)
        return None

    def _forward_stacked(self, feats, targets, mode, sample=None, ss=(0.0, None, None), drop_feats=True):
        """nn.LSTM with num_layers > 1: the layer-wavefront chain kernels under autograd glue (stack_functional.py)"""
        if mode == 'beam_search':
            raise NotImplementedError("beam search of a stacked model (num_layers > 1): the reference's BeamSearchNode views the "
                                      "per-sample [num_layers, H] state as [1, 1, -1] (S2VTModel.py:253-254) and raises for "
                                      "num_layers > 1; use mode='test'")
        if mode == 'beam':
            raise NotImplementedError(_BEAM_STACKED)
        if mode == 'score':
            raise NotImplementedError("mode='score' of a stacked model (num_layers > 1): the scoring driver's word step is the "
                                      "one-layer LSTM's; take the logits of mode='train' and log_softmax(...).gather(...) them")
        clean = feats                                      # (the scheduled pass runs without dropout)
        feats = self.feat_drop(feats) if drop_feats else feats      # S2VTModel.py:52 (drop_feats False: the caller drew it)
        if mode == 'train':
            if targets is None:
                raise ValueError("mode='train' needs targets")
            _F.require_hip(targets, "targets")
            if ss[0] > 0:
                targets = _S.scheduled_inputs(self, clean, targets.reshape(targets.shape[0], -1), ss[0], temperature=ss[1], seed=ss[2])
            B, T = feats.shape[0], 2 * self.length - 1
            # draw order: the inter-layer masks of vid_rnn, then of word_rnn (nn.LSTM's dropout, S2VTModel.py:17-20), then out_drop
            rnn_masks = _S.draw_rnn_masks(self, T, B, feats.device)
            out_mask = None
            if self.training and self.out_drop.p > 0:
                out_mask = self.out_drop(torch.ones(B, self.length - 1, self.dim_hid, dtype=torch.float32, device=feats.device))
            return _S.train_forward(self, feats, targets.reshape(targets.shape[0], -1), out_mask=out_mask, rnn_masks=rnn_masks)
        elif mode == 'test':
            return _S.greedy_decode(self, feats, self.sos_ix)
        elif mode == 'sample':
            return _S.greedy_decode(self, feats, self.sos_ix, sample=sample)
        return None

    @staticmethod
    def _get_word2embed_from_glove(glove_path, ix2word):
        """{word: [floats]} for the vocabulary words found in a GloVe text file (one 'word v1 v2 ...' line per word)."""
        wanted = set(ix2word.values())
        table = {}
        with open(glove_path, encoding='utf-8') as f:
            for line in f:
                word, _, rest = line.rstrip('\n').partition(' ')
                if word in wanted:
                    table[word] = [float(x) for x in rest.split(' ') if x]
        return table

    def load_glove_weights(self, glove_path, glove_dim, ix2word, word2embed='./data/word2embed.json'):
        """Initialise the embedding from GloVe vectors (S2VTModel.py:112-147; train.py:88 has the call commented out).
        `word2embed` None: parse `glove_path` and cache the {word: vector} table as ./data/word2embed.json; otherwise the
        path of such a cache.  Words without a vector keep a Xavier-normal row; the embedding stays trainable.  Host-side
        torch glue: the new `nn.Embedding` is an ordinary parameter of the HIP path."""
        import json
        import os
        assert glove_dim == self.dim_embed
        if word2embed is None:
            table = self._get_word2embed_from_glove(glove_path, ix2word)
            os.makedirs('./data', exist_ok=True)
            with open('./data/word2embed.json', 'w+', encoding='utf-8') as fp:
                json.dump(table, fp)
        else:
            with open(word2embed, encoding='utf-8') as fp:
                table = json.load(fp)
        print('get {} word2embed'.format(len(table)))
        dev = self.embedding.weight.device
        weights = torch.zeros([self.vocab_size, glove_dim], dtype=torch.float, device=dev)
        torch.nn.init.xavier_normal_(weights)
        for ix, word in ix2word.items():
            if word in table:
                weights[int(ix)] = torch.tensor(table[word], dtype=torch.float, device=dev)
        self.embedding = nn.Embedding.from_pretrained(weights, freeze=False)


BeamSearchNode = _beam.BeamSearchNode
# Ensemble([m0, m1, ...], weights=None).beam(feats, ...): mode='beam' / beam_constrained over the weighted mean of several models'
# word distributions, on the device (not in the reference; s2vt_video_caption_amd/ensemble.py)
from s2vt_video_caption_amd.ensemble import Ensemble  # noqa: E402
