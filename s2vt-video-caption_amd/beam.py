"""Beam search of the S2VT decoder (`S2VT.forward(mode='beam_search')` + `S2VT.beam_search`,
S2VTModel.py:56-61, 149-240), batched on the GPU.

The reference walks every sample and every node in Python and launches three tiny torch ops per node.
Here the priority-queue bookkeeping stays on the host (it is what defines the result, including its
quirks), but all samples advance one depth at a time and every LSTM step / vocabulary projection of
that depth runs as ONE batched call into the HIP library:
  * all expandable nodes of a sample at one depth share the vid_rnn state (zero-input recurrence from
    the encoder state), so the vid step runs once per depth for the whole batch;
  * the word step and the out_linear run over all (sample, beam slot) rows at once.
Semantics kept exactly: score = log-prob of the LAST token / len**0.7 (not
cumulative), queue cleared after popping `beam_width` entries, finished (<eos>) entries re-inserted
unchanged, fan-out = top-20 tokens pushed in ascending token order, stop when the queue holds
<= beam_width entries, answer = best queue entry back-traced, first element the [[<sos>]] tensor.

`S2VT.forward(mode='beam')` (beam_cumulative below) is the search the reference does not have: hypotheses ranked by their
cumulative log-probability, length-normalised when they end, n-best out.  It is the one-group case of the ONE device policy
(csrc/beam_policy.hip: group / diverse beam search), which also serves beam_constrained, beam_diverse and Ensemble.beam through one
driver (_group_search).  Every search whose policy lives on the device - the reference's included - runs the one depth loop
(_device_depth_loop) over a depth-step callable, and a model's depth step is spelled out once (_DepthStep).
"""
import heapq

import numpy as np
import torch

from . import capi, ops

FANOUT = 20  # hard-coded topk(20) of the reference (S2VTModel.py:216)


class BeamSearchNode(object):
    """API-compatible with the reference's BeamSearchNode (S2VTModel.py:243-274)."""

    def __init__(self, vid_hid, word_hid, previousNode, wordId, logProb, length):
        self.vid_hid = vid_hid
        self.word_hid = word_hid
        self.prevNode = previousNode
        self.wordid = wordId
        self.logp = logProb
        self.leng = length
        self.score = None

    def eval(self, alpha=0.7):
        if self.score is None:
            self.score = self.logp / pow(float(self.leng), alpha)
        return self.score

    def __gt__(self, other):
        return bool(other.eval() > self.eval())

    def __lt__(self, other):
        # the reference defines only __gt__; `a < b` therefore resolves to b.__gt__(a)
        return bool(self.eval() > other.eval())


PERSISTENT_ENCODER = True        # A/B switch: encoder recurrences on the persistent split-precision kernels
PLANE_ENCODER = True             # A/B switch: the whole encode phase by the library (s2vt_decode_encode_cached), GEMMs on the plane path
VID_PRECOMPUTE = True            # A/B switch: vid_rnn's token-independent decode steps and their gate-input GEMM once, in front of the depth loop


def _encoder_states(model, feats, params, max_depth, library_encode):
    """(vid_h, vid_c, word_h, word_c, gx_dec): the states [B, H] a search starts from - vid_rnn over the L real frames only, word_rnn
    with a zero embedding (S2VTModel.py:57-60) - and, from the library's encode phase only, vid_rnn's token-independent decode steps
    (functional.decode_encode; None otherwise)."""
    (w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, w_f, b_f, w_o, b_o, emb) = [p.detach() for p in params]
    B, L, _ = feats.shape
    H, E = model.dim_hid, model.dim_embed
    if library_encode:
        # the library's own encode phase (what mode='test' runs: plane-path GEMMs, paired persistent recurrence launches); it
        # fills the weight-image cache the plane-path depth step reads
        from . import functional
        enc = functional.decode_encode(feats, params, model, depth=max_depth if VID_PRECOMPUTE else 0)
        if enc is not None:
            return enc
    bsum1 = (b_ih1 + b_hh1).contiguous()
    bsum2 = (b_ih2 + b_hh2).contiguous()
    w_v = w_ih2[:, E:]          # [4H, H] view, row stride E+H
    x1 = ops.feat_proj_fwd(feats.contiguous(), w_f, b_f)                       # [L*B, H] time-major
    gx1 = _gemm_strided(x1, w_ih1, bsum1)
    # (the persistent split-precision recurrence, lstm_persist_x3.hip, where the shape is supported; else launches per timestep)
    px = capi.load().s2vt_lstm_seq_x3_workspace_bytes(L, B, H) > 0 and PERSISTENT_ENCODER

    def layer(gx, w_hh):
        if px:
            return ops.lstm_seq_fwd_persist(L, B, gx, L, None, w_hh, poison=False)
        return ops.lstm_seq_fwd(L, B, gx, L, None, w_hh)
    h1_all, c1_all, _ = layer(gx1, w_hh1)
    gx2 = _gemm_strided(h1_all, w_v, bsum2)
    h2_all, c2_all, _ = layer(gx2, w_hh2)
    return (h1_all[(L - 1) * B:], c1_all[(L - 1) * B:], h2_all[(L - 1) * B:].clone(), c2_all[(L - 1) * B:].clone(), None)


@torch.no_grad()
def beam_search(model, feats, params, beam_width=3, max_depth=30):
    (w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, w_f, b_f, w_o, b_o, emb) = [p.detach() for p in params]
    dev = feats.device
    B, L, _ = feats.shape
    H, E, V = model.dim_hid, model.dim_embed, model.vocab_size
    if V < FANOUT:
        raise RuntimeError("beam search needs vocab_size >= %d (topk(20), S2VTModel.py:216)" % FANOUT)
    sos, eos = int(model.sos_ix), int(model.eos_ix)
    lib = capi.load()
    device_queues = DEVICE_QUEUES and lib.s2vt_beam_queue_bytes(B, beam_width, max_depth) > 0
    states = _encoder_states(model, feats, params, max_depth, device_queues and PLANE_STEP and PLANE_ENCODER)
    if device_queues:
        return _beam_search_device_queues(lib, model, feats, params, B, H, beam_width, max_depth, sos, eos, *states)
    vid_h, vid_c, word_h, word_c, _ = states

    # ---- per-sample queues (host, BeamQueues) + one library call per depth (s2vt_beam_step): vid step for the batch,
    # word step / out_linear / log_softmax / top-20 for all expandable (sample, beam slot) rows
    import ctypes
    from .functional import _ptr, _stream, _dims, _params_struct
    max_rows = max(B * beam_width, B)
    global LAST_PATH
    LAST_PATH = "host queues"
    queues = (BeamQueues if FAST_QUEUES else HeapQueues)(B, beam_width, sos, eos)
    pcs = tuple(p.contiguous() for p in (w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, w_f, b_f, w_o, b_o, emb))
    d = _dims(feats, pcs)
    ps = _params_struct(capi.Params, pcs)
    with torch.cuda.device(dev):
        nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(d), max_rows)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        vid = [(vid_h.contiguous(), vid_c.contiguous()), (torch.empty(B, H, device=dev), torch.empty(B, H, device=dev))]
        tab = [(torch.empty(max_rows, H, device=dev), torch.empty(max_rows, H, device=dev)) for _ in range(2)]
        tab[0][0][:B].copy_(word_h)
        tab[0][1][:B].copy_(word_c)
        rows_dev = torch.empty(3, max_rows, dtype=torch.int32, device=dev)
        top_dev = torch.empty(2, max_rows, FANOUT, dtype=torch.int32, device=dev)      # [0] ids, [1] fp32 log-prob bits
        depth = 0
        while depth < max_depth and not queues.all_done():
            depth += 1
            rows_b, rows_state, rows_tok = queues.pop()
            R = len(rows_b)
            if R:
                rows_dev[:, :R].copy_(torch.from_numpy(np.stack([np.asarray(rows_b), np.asarray(rows_state),
                                                                  np.asarray(rows_tok)]).astype(np.int32)))
            (vh_in, vc_in), (vh_out, vc_out) = vid[(depth - 1) & 1], vid[depth & 1]
            (wh_in, wc_in), (wh_out, wc_out) = tab[(depth - 1) & 1], tab[depth & 1]
            capi.check(lib.s2vt_beam_step(ctypes.byref(d), ctypes.byref(ps), R, _ptr(rows_dev[0]), _ptr(rows_dev[1]),
                                          _ptr(rows_dev[2]), _ptr(vh_in), _ptr(vc_in), _ptr(vh_out), _ptr(vc_out),
                                          _ptr(wh_in), _ptr(wc_in), _ptr(wh_out), _ptr(wc_out), _ptr(top_dev[0]),
                                          _ptr(top_dev[1]), _ptr(ws), nbytes, _stream(dev)), "s2vt_beam_step")
            top_ix = top_lp = None
            if R:
                both = top_dev[:, :R].cpu().numpy()                                     # one D2H copy per depth
                top_ix = both[0].astype(np.int64)
                top_lp = both[1].view(np.float32)
            queues.push(top_ix, top_lp)
    # list[list[Tensor]] like the reference (first element the [[<sos>]] tensor, then 0-dim ids): one H2D copy for all
    # sequences, the elements are views of it
    seqs = queues.finish()
    flat = torch.as_tensor(np.concatenate([np.asarray(q, dtype=np.int64) for q in seqs]), device=dev)
    sentences, o = [], 0
    for q in seqs:
        t = flat[o:o + len(q)]
        o += len(q)
        sentences.append([t[:1].view(1, 1)] + list(t[1:].unbind(0)))
    return sentences


FAST_QUEUES = True
DEVICE_QUEUES = True         # the queues on the device (csrc/beam_queue.hip): no host work and no transfer per depth


PLANE_STEP = True            # s2vt_beam_step_cached: the depth's GEMMs on the plane path, from the decode cache of the same weights
LAST_PATH = None             # which path the last beam_search call took (bench.py reports it beside the rate)


def _decode_cache(lib, model, feats, params, d):
    """The decode cache of this model's weights - the weight-derived images of mode='test' (plane images of W_v / W_o, the per-token
    gate table), which serve the beam's depth step as well - or None where there is none (PLANE_STEP off, fp32-MFMA mode).  A model
    that has not decoded with these weights yet runs ONE greedy decode of this batch to fill it (7 ms, once per weight version -
    eval.py decodes the whole validation set with one set of weights)."""
    from . import functional
    if not PLANE_STEP:
        return None
    cache, valid = functional.decode_cache_entry(model, params, d, feats.device, lib)
    if cache is not None and not valid:
        functional.greedy_decode(feats, params, int(model.sos_ix), owner=model)
        cache, valid = functional.decode_cache_entry(model, params, d, feats.device, lib)
    return cache if valid else None


class _DepthStep(object):
    """One model's depth step over the fixed rows r = b * beam_width + slot: what the model owns in a search - parameters, dims, decode
    cache, precomputed vid_rnn steps, workspace, vid_rnn states and word_rnn state tables (both ping-ponged by depth parity) - and the
    ONE place that spells out the s2vt_beam_step* call."""

    def __init__(self, lib, model, feats, params, R, vid_h, vid_c, word_h, word_c, gx_dec):
        import ctypes
        from .functional import _dims, _params_struct
        dev = feats.device
        B, H = feats.shape[0], model.dim_hid
        self.lib = lib
        self.pcs = tuple(p.detach().contiguous() for p in params)
        self.d = _dims(feats, self.pcs)
        self.ps = _params_struct(capi.Params, self.pcs)
        self.cache = _decode_cache(lib, model, feats, params, self.d)
        self.gx_dec = gx_dec if self.cache is not None else None
        with torch.cuda.device(dev):
            self.nbytes = lib.s2vt_beam_workspace_bytes(ctypes.byref(self.d), R)
            self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
            self.vid = [(vid_h.contiguous(), vid_c.contiguous()), (torch.empty(B, H, device=dev), torch.empty(B, H, device=dev))]
            self.tab = [(torch.zeros(R, H, device=dev), torch.zeros(R, H, device=dev)) for _ in range(2)]
            self.tab[0][0][:B].copy_(word_h)
            self.tab[0][1][:B].copy_(word_c)

    def __call__(self, depth, rows, st, top_ix=None, top_lp=None, con=None, words=None, logits=None, top_g=None, gumbel=None):
        """the step of `depth` for rows [3, R] (sample, state row, token): every row's top 20 into (top_ix, top_lp) - behind the
        constrained fan-out head with con (a capi.Constraints) and words = (pointer, row stride) of the slots' histories - or, with
        logits [R, V], stopped one launch early so that the logits stay on the card - or, with top_g [R, 20] and gumbel = (fp32
        inv_temperature, seed), behind the perturbed head of the stochastic beam (best g first; the noise of step depth - 1)"""
        import ctypes
        from .functional import _ptr
        vid = tuple(_ptr(x) for x in self.vid[(depth - 1) & 1] + self.vid[depth & 1])           # h, c in; h, c out
        word = tuple(_ptr(x) for x in self.tab[(depth - 1) & 1] + self.tab[depth & 1])
        gx = self.gx_dec[depth - 1] if self.gx_dec is not None else None
        head = (ctypes.byref(self.d), ctypes.byref(self.ps), rows.shape[1], _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]))
        out = (_ptr(top_ix), _ptr(top_lp), _ptr(self.ws), self.nbytes)
        cache = (_ptr(self.cache), self.cache.numel() if self.cache is not None else 0)
        if logits is not None:
            name, args = "s2vt_beam_step_logits", head + vid + (_ptr(gx),) + word + (_ptr(logits), logits.stride(0)) + out[2:] + cache
        elif top_g is not None:
            name = "s2vt_beam_step_gumbel"
            args = head + vid + (_ptr(gx),) + word + out[:2] + (_ptr(top_g),) + out[2:] + cache + (gumbel[0], gumbel[1], depth - 1)
        elif con is not None:
            hist = (ctypes.byref(con), words[0], words[1], depth - 1)
            name, args = "s2vt_beam_step_constrained", head + vid + (_ptr(gx),) + word + out + cache + hist
        elif gx is not None:
            name, args = "s2vt_beam_step_gx", head + (_ptr(gx),) + word + out + cache
        elif self.cache is not None:
            name, args = "s2vt_beam_step_cached", head + vid + word + out + cache
        else:
            name, args = "s2vt_beam_step", head + vid + word + out
        capi.check(getattr(self.lib, name)(*args, st), name)


def _model_depth_step(lib, model, feats, params, R, states, policy_name, con=None):
    """the depth step of a one-model search for _device_depth_loop; names the path in LAST_PATH"""
    step = _DepthStep(lib, model, feats, params, R, *states)
    global LAST_PATH
    LAST_PATH = (policy_name + " + plane-path depth step (decode cache)" + (", vid_rnn steps precomputed" if step.gx_dec is not None else "")) \
        if step.cache is not None else policy_name + " + fp32-MFMA depth step"
    return lambda depth, rows, top_ix, top_lp, words, st: step(depth, rows, st, top_ix, top_lp, con, words)


def _device_depth_loop(dev, B, R, max_depth, qbytes, policy_step, depth_step, with_top_g=False):
    """The depth loop of a search whose policy lives on the device: per depth ONE words = policy_step(depth, qs, top_ix, top_lp, rows,
    st) (consume the top-20 of the depth before, freeze finished samples, write the rows of the step; the constrained forms return
    (pointer, row stride) of the live slots' words for the step they have just prepared) and ONE depth_step(depth, rows, top_ix,
    top_lp, words, st) over the fixed rows r = b * beam_width + slot (R of them) that fills top_ix / top_lp: one model's
    (_model_depth_step) or an ensemble's; nothing crosses PCIe.  The early exit (all samples frozen) is polled without blocking: the
    frozen-sample counter (the int32 at byte 0 of the policy's state) is copied to pinned memory after every depth and read one
    depth late - extra depths change nothing.  Ends with policy_step(0, ...), the last depth's results.  Returns the policy's state
    tensor (qbytes) and the stream.  with_top_g (the stochastic beam): a third buffer top_g fp32 [R, 20], the perturbed scores, is
    allocated beside top_ix / top_lp and handed to both callables as their last argument."""
    from .functional import _stream
    with torch.cuda.device(dev):
        qs = torch.empty(qbytes, dtype=torch.uint8, device=dev)
        rows = torch.zeros(3, R, dtype=torch.int32, device=dev)
        top_ix = torch.zeros(R, FANOUT, dtype=torch.int32, device=dev)
        top_lp = torch.zeros(R, FANOUT, dtype=torch.float32, device=dev)
        extra = (torch.zeros(R, FANOUT, dtype=torch.float32, device=dev),) if with_top_g else ()
        frozen = torch.zeros(max_depth + 2, dtype=torch.int32).pin_memory()
        frozen_dev = qs[:4].view(torch.int32)
        events = []
        st = _stream(dev)
        depth = 0
        while depth < max_depth:
            if depth >= 2 and events[depth - 2].query() and int(frozen[depth - 1]) == B:
                break                                   # every sample had stopped two depths ago: the reference's loop ended there
            depth += 1
            words = policy_step(depth, qs, top_ix, top_lp, rows, st, *extra)
            if depth > 1:
                frozen[depth].copy_(frozen_dev[0], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            events.append(ev)
            depth_step(depth, rows, top_ix, top_lp, words, st, *extra)
        policy_step(0, qs, top_ix, top_lp, rows, st, *extra)    # the last depth's results
        global LAST_DEPTHS
        LAST_DEPTHS = depth
    return qs, st


LAST_DEPTHS = 0              # depth steps the last device-policy search ran (tools/bench_beam_cum.py: time per depth)


def _beam_search_device_queues(lib, model, feats, params, B, H, beam_width, max_depth, sos, eos, vid_h, vid_c, word_h, word_c,
                               gx_dec=None):
    """mode='beam_search' with the reference's queue bookkeeping on the device (s2vt_beam_queue_step: push the children of the depth
    before, freeze finished samples, pop the next beam with heapq's own sift order); only the back-traced sequences cross PCIe, at
    the end."""
    from .functional import _ptr
    dev = feats.device
    qbytes = lib.s2vt_beam_queue_bytes(B, beam_width, max_depth)

    def qstep(depth, qs, top_ix, top_lp, rows, st):
        capi.check(lib.s2vt_beam_queue_step(B, beam_width, max_depth, sos, eos, depth, _ptr(qs), qbytes, _ptr(top_ix), _ptr(top_lp),
                                            _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), st), "s2vt_beam_queue_step")
    R = B * beam_width
    qs, st = _device_depth_loop(dev, B, R, max_depth, qbytes, qstep,
                                _model_depth_step(lib, model, feats, params, R, (vid_h, vid_c, word_h, word_c, gx_dec), "device queues"))
    with torch.cuda.device(dev):
        cap = max_depth + 2
        out = torch.empty(B, cap, dtype=torch.int32, device=dev)
        out_len = torch.empty(B, dtype=torch.int32, device=dev)
        capi.check(lib.s2vt_beam_queue_result(B, beam_width, max_depth, _ptr(qs), qbytes, _ptr(out), cap, _ptr(out_len), st),
                   "s2vt_beam_queue_result")
        host = torch.cat([out, out_len[:, None]], dim=1).cpu().numpy()        # (the one synchronisation of the search)
        lens = host[:, cap].tolist()
        flat = torch.as_tensor(np.concatenate([host[b, :lens[b]] for b in range(B)]).astype(np.int64), device=dev)
    sentences, o = [], 0
    for b in range(B):
        t = flat[o:o + lens[b]]
        o += lens[b]
        sentences.append([t[:1].view(1, 1)] + list(t[1:].unbind(0)))
    return sentences


MAX_BEAM_WIDTH = 8           # widths for which the step kernels' fan-out of 20 is exact (and the policy kernel's limit)


def check_beam_args(beam_width, max_depth, length_alpha, n_best, vocab_size):
    """(beam_width, max_depth, length_alpha, n_best) of mode='beam' as ints / a float, or ValueError - before anything reaches the
    library"""
    import math
    W, D, nb, alpha = int(beam_width), int(max_depth), int(n_best), float(length_alpha)
    if W != beam_width or not 1 <= W <= MAX_BEAM_WIDTH:
        raise ValueError("mode='beam': beam_width must be an integer in [1, %d], got %r" % (MAX_BEAM_WIDTH, beam_width))
    if nb != n_best or not 1 <= nb <= W:
        raise ValueError("mode='beam': n_best must be an integer in [1, beam_width = %d], got %r" % (W, n_best))
    if D != max_depth or D < 1:
        raise ValueError("mode='beam': max_beam_depth must be an integer >= 1, got %r" % (max_depth,))
    if not math.isfinite(alpha) or alpha < 0:
        raise ValueError("mode='beam': length_alpha must be finite and >= 0, got %r" % (length_alpha,))
    if int(vocab_size) < FANOUT:
        raise ValueError("mode='beam': vocab_size must be >= %d (the depth step returns each row's %d best tokens), got %r"
                         % (FANOUT, FANOUT, vocab_size))
    return W, D, alpha, nb


@torch.no_grad()
def check_beam_constraints(spec, max_depth, vocab_size):
    """the two shape rules of the constrained search, or ValueError - before anything reaches the library: the fan-out must find 20
    finite words in every edited row, and the constraint phase stages at most 1023 words of history"""
    from . import sampling
    D, V = int(max_depth), int(vocab_size)
    if D > sampling.MAX_HISTORY:
        raise ValueError("beam_constrained: max_beam_depth %d > %d, the history a constrained row kernel stages" % (D, sampling.MAX_HISTORY))
    need = FANOUT + D + len(spec.banned) + 1
    if V < need:
        raise ValueError("beam_constrained: vocab_size %d < %d + max_beam_depth + banned ids + 1 = %d: a row could keep fewer than %d "
                         "words" % (V, FANOUT, need, FANOUT))


def _checked_constraints(constraints, max_depth, vocab_size):
    """the ConstraintSpec of a constrained search after check_beam_constraints; None for None or a spec that constrains nothing"""
    from . import sampling
    if constraints is None or not sampling.constrains(constraints):
        return None
    check_beam_constraints(constraints, max_depth, vocab_size)
    return constraints


@torch.no_grad()
def _group_search(what, dev, B, W, G, D, sos, eos, alpha, lam, n_best, constraints, make_depth_step):
    """The one driver of the device policy (csrc/beam_policy.hip) behind mode='beam', beam_constrained, beam_diverse and Ensemble.beam:
    G groups of W / G slots, the cumulative search being G = 1 (where lam is inert).  constraints: a checked ConstraintSpec or None -
    with one the policy keeps every live slot's words and hands them to the depth step.  make_depth_step(lib, R, con, policy_name)
    returns the depth step of _device_depth_loop (con: the capi.Constraints or None) and names the path in LAST_PATH.  Returns
    (ids int64 [B, G, n_best, D] padded with <eos>, lengths int64 [B, G, n_best], scores fp32 [B, G, n_best]) on the device, every
    group best first, without the G axis at G = 1; no host synchronisation.  `what` names the caller in the error of a state too
    large.  One group runs through the s2vt_beam_div_* entries as well: s2vt_beam_cum_* are the same launches."""
    import ctypes
    from . import sampling
    from .functional import _ptr
    lib = capi.load()
    hist = constraints is not None
    qbytes = lib.s2vt_beam_div_bytes(B, W, G, D, int(hist))
    if qbytes == 0:
        raise ValueError("%s: batch %d x beam_width %d x max_beam_depth %d is more than the search state holds" % (what, B, W, D))
    con = keep = None
    words, words_ld = ctypes.c_void_p(), ctypes.c_int64()
    if hist:
        con, keep = sampling.constraints_struct(constraints)     # (keep: the banned ids' host array lives as long as con is used)

    def policy_step(depth, qs, top_ix, top_lp, rows, st):
        capi.check(lib.s2vt_beam_div_step(B, W, G, D, sos, eos, alpha, lam, depth, _ptr(qs), qbytes, _ptr(top_ix), _ptr(top_lp),
                                          _ptr(rows[0]), _ptr(rows[1]), _ptr(rows[2]), ctypes.byref(words) if hist else None,
                                          ctypes.byref(words_ld) if hist else None, st), "s2vt_beam_div_step")
        return (ctypes.c_void_p(words.value), words_ld.value) if hist else None
    name = ("constrained " if hist else "") + ("cumulative beam" if G == 1 else "diverse beam")
    qs, st = _device_depth_loop(dev, B, B * W, D, qbytes, policy_step, make_depth_step(lib, B * W, con, name))
    with torch.cuda.device(dev):
        lead = (B, n_best) if G == 1 else (B, G, n_best)
        ids = torch.empty(lead + (D,), dtype=torch.int32, device=dev)
        lens = torch.empty(lead, dtype=torch.int32, device=dev)
        scores = torch.empty(lead, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_beam_div_result(B, W, G, D, eos, n_best, _ptr(qs), qbytes, _ptr(ids), _ptr(lens), _ptr(scores), st),
                   "s2vt_beam_div_result")
        return ids.long(), lens.long(), scores


def _model_group_search(what, model, feats, params, W, G, D, alpha, lam, n_best, constraints):
    """_group_search of one model: its encoder states, decode cache and depth step"""
    def make_depth_step(lib, R, con, policy_name):
        states = _encoder_states(model, feats, params, D, PLANE_STEP and PLANE_ENCODER)
        return _model_depth_step(lib, model, feats, params, R, states, policy_name, con)
    return _group_search(what, feats.device, feats.shape[0], W, G, D, int(model.sos_ix), int(model.eos_ix), alpha, lam, n_best,
                         _checked_constraints(constraints, D, model.vocab_size), make_depth_step)


def beam_cumulative(model, feats, params, beam_width=3, max_depth=30, length_alpha=0.7, n_best=1, constraints=None):
    """mode='beam' (not in the reference): hypotheses ranked by the fp32 sum of their tokens' log-probs, the
    beam_width best of all live slots' candidates kept per depth by (sum descending, slot ascending, token ascending), a hypothesis
    that ends in <eos> at depth t pooled with score sum / t**length_alpha, the ones still live at max_depth with sum /
    max_depth**length_alpha.  Same encoder, decode cache, depth step and polled early exit as mode='beam_search'; the policy is
    csrc/beam_policy.hip at one group.  Returns (ids int64 [B, n_best, max_depth] padded with <eos>, lengths int64 [B, n_best],
    scores fp32 [B, n_best]) on the device, best first; no host synchronisation.
    constraints (a sampling.ConstraintSpec; S2VT.beam_constrained, include/s2vt_hip.h "constrained beam"): every live slot's logits
    row is edited by the rules of the constrained draw with the slot's own words as history before its log_softmax and top 20 - the
    policy keeps those words on the device, the depth step runs the constrained fan-out head (s2vt_beam_step_constrained).  None, or
    a spec that constrains nothing: the plain path, launch for launch."""
    W, D, alpha, n_best = check_beam_args(beam_width, max_depth, length_alpha, n_best, model.vocab_size)
    return _model_group_search("mode='beam'", model, feats, params, W, 1, D, alpha, 0.0, n_best, constraints)


def check_diverse_args(beam_width, num_groups, diversity_lambda, n_best):
    """(num_groups, diversity_lambda, n_best) of beam_diverse as ints / a float, or ValueError - before anything reaches the
    library; beam_width is an int that check_beam_args has passed"""
    import math
    W, G, nb = int(beam_width), int(num_groups), int(n_best)
    if G != num_groups or not 1 <= G <= W or W % G:
        raise ValueError("beam_diverse: num_groups must be an integer in [1, beam_width = %d] that divides beam_width, got %r"
                         % (W, num_groups))
    if nb != n_best or not 1 <= nb <= W // G:
        raise ValueError("beam_diverse: n_best must be an integer in [1, beam_width / num_groups = %d], got %r" % (W // G, n_best))
    try:
        lam = float(diversity_lambda)
        with np.errstate(over="ignore"):
            lam32 = float(np.float32(lam))
    except (TypeError, ValueError, OverflowError):
        lam = lam32 = float("nan")
    if not math.isfinite(lam) or not math.isfinite(lam32) or lam < 0:
        raise ValueError("beam_diverse: diversity_lambda must be finite (in fp32) and >= 0, got %r" % (diversity_lambda,))
    return G, lam, nb


def beam_diverse(model, feats, params, beam_width=6, num_groups=3, diversity_lambda=0.5, max_depth=30, length_alpha=0.7, n_best=1,
                 constraints=None):
    """S2VT.beam_diverse (not in the reference; include/s2vt_hip.h "diverse beam"): diverse (group) beam search
    (Vijayakumar et al., 2016).  The beam_width slots are num_groups groups of Wg = beam_width / num_groups; per depth the groups
    select in order, each the Wg best of its own slots' candidates by a = (sum of log-probs) - diversity_lambda * (how often the
    earlier groups chose the candidate's word at this depth), ties by (slot, token); hypotheses carry and are pooled with the
    unpenalised sum, per group, by mode='beam''s rules.  Same encoder, decode cache, depth step and polled early exit as mode='beam';
    the policy is csrc/beam_policy.hip, one launch per depth, nothing crosses PCIe.  Returns (ids int64 [B, num_groups, n_best,
    max_depth] padded with <eos>, lengths int64 [B, num_groups, n_best], scores fp32 [B, num_groups, n_best]) on the device, every
    group best first; no host synchronisation.
    constraints (a sampling.ConstraintSpec): as in beam_cumulative - every live slot's row is edited with the slot's own words in
    front of its log_softmax and top 20; the policy keeps those words.
    num_groups == 1 IS beam_cumulative with an axis of 1 inserted: the same launch of the same kernel, in which diversity_lambda is
    inert; the same bits."""
    W, D, alpha, _ = check_beam_args(beam_width, max_depth, length_alpha, 1, model.vocab_size)
    G, lam, n_best = check_diverse_args(W, num_groups, diversity_lambda, n_best)
    out = _model_group_search("beam_diverse" if G > 1 else "mode='beam'", model, feats, params, W, G, D, alpha, lam, n_best, constraints)
    return out if G > 1 else tuple(x.unsqueeze(1) for x in out)


def check_stochastic_args(n_samples, temperature, seed, max_depth, vocab_size):
    """(n_samples, temperature, seed, max_depth) of sample_distinct as ints / a float, or ValueError - before anything reaches the
    library; seed None draws one as `sample` does"""
    from . import sampling
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or not 1 <= int(n_samples) <= MAX_BEAM_WIDTH:
        raise ValueError("sample_distinct: n_samples must be an integer in [1, %d], got %r" % (MAX_BEAM_WIDTH, n_samples))
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or int(max_depth) < 1:
        raise ValueError("sample_distinct: max_depth must be an integer >= 1, got %r" % (max_depth,))
    if int(vocab_size) < FANOUT:
        raise ValueError("sample_distinct: vocab_size must be >= %d (the depth step returns each row's %d best words), got %r"
                         % (FANOUT, FANOUT, vocab_size))
    if isinstance(temperature, (bool, str)) or not isinstance(temperature, (int, float, np.integer, np.floating)):
        raise ValueError("sample_distinct: temperature must be finite and > 0, got %r" % (temperature,))
    t, seed = sampling.check_sample_args(temperature, seed)
    return int(n_samples), t, seed, int(max_depth)


def inv_temperature(temperature):
    """fp32(1 / temperature) as the library's sampled decodes form it: the fp32 quotient of fp32 operands"""
    return float(np.float32(1.0) / np.float32(temperature))


@torch.no_grad()
def stochastic(model, feats, params, n_samples=5, temperature=1.0, seed=0, max_depth=30):
    """S2VT.sample_distinct (not in the reference; include/s2vt_hip.h "stochastic beam"): stochastic beam search
    (Kool, van Hoof, Welling, 2019) - n_samples pairwise distinct captions per clip, sampled without replacement from the model's
    distribution over sentences at `temperature`, in the order a sequential without-replacement sampler draws them.  Same encoder
    states, decode cache, precomputed vid_rnn steps, depth loop and polled early exit as mode='beam'; the depth step ends in the
    perturbed fan-out head (csrc/gumbel_top.hip), the policy is csrc/sbs_policy.hip, one launch per depth; nothing crosses PCIe.
    Arguments as check_stochastic_args returns them.  Returns (ids int64 [B, W, D] padded with <eos>, lengths int64 [B, W], logprobs
    fp32 [B, W], perturbed fp32 [B, W], kappa fp32 [B]) on the device; no host synchronisation."""
    from .functional import _ptr
    lib = capi.load()
    dev = feats.device
    B, W, D = feats.shape[0], n_samples, max_depth
    sos, eos = int(model.sos_ix), int(model.eos_ix)
    qbytes = lib.s2vt_sbs_bytes(B, W, D)
    if qbytes == 0:
        raise ValueError("sample_distinct: batch %d x n_samples %d x max_depth %d is more than the search state holds" % (B, W, D))
    gum = (inv_temperature(temperature), int(seed))
    step = _DepthStep(lib, model, feats, params, B * W, *_encoder_states(model, feats, params, D, PLANE_STEP and PLANE_ENCODER))
    global LAST_PATH
    LAST_PATH = "stochastic beam + " + (("plane-path depth step (decode cache)" + (", vid_rnn steps precomputed" if step.gx_dec is not None
                                                                                   else "")) if step.cache is not None
                                        else "fp32-MFMA depth step")

    def policy_step(depth, qs, top_ix, top_lp, rows, st, top_g):
        capi.check(lib.s2vt_sbs_step(B, W, D, sos, eos, depth, _ptr(qs), qbytes, _ptr(top_ix), _ptr(top_lp), _ptr(top_g), _ptr(rows[0]),
                                     _ptr(rows[1]), _ptr(rows[2]), st), "s2vt_sbs_step")

    def depth_step(depth, rows, top_ix, top_lp, words, st, top_g):
        step(depth, rows, st, top_ix, top_lp, top_g=top_g, gumbel=gum)
    qs, st = _device_depth_loop(dev, B, B * W, D, qbytes, policy_step, depth_step, with_top_g=True)
    with torch.cuda.device(dev):
        ids = torch.empty(B, W, D, dtype=torch.int32, device=dev)
        lens = torch.empty(B, W, dtype=torch.int32, device=dev)
        lp = torch.empty(B, W, dtype=torch.float32, device=dev)
        g = torch.empty(B, W, dtype=torch.float32, device=dev)
        kappa = torch.empty(B, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_sbs_result(B, W, D, eos, _ptr(qs), qbytes, _ptr(ids), _ptr(lens), _ptr(lp), _ptr(g), _ptr(kappa), st),
                   "s2vt_sbs_result")
        return ids.long(), lens.long(), lp, g, kappa


class HeapQueues(object):
    """The reference's queue bookkeeping, literally: one Python heap of (key, node) tuples per sample
    (S2VTModel.py:186-236).  Kept as the definition the vectorised BeamQueues is tested against and as the
    tie fallback's model; ~30 ms per depth at B=128, beam 5."""

    def __init__(self, B, beam_width, sos, eos):
        self.B, self.bw, self.eos = B, beam_width, eos
        self.heaps = []
        for b in range(B):
            root = BeamSearchNode(None, b, None, sos, 0, 1)
            self.heaps.append([(-root.eval(), root)])
        self.done = [False] * B
        self.beams = [None] * B

    def all_done(self):
        return all(self.done)

    def pop(self):
        rows_b, rows_state, rows_tok = [], [], []
        self.beams = [None] * self.B
        for b in range(self.B):
            if self.done[b]:
                continue
            heap = self.heaps[b]
            beam = [heapq.heappop(heap) for _ in range(min(self.bw, len(heap)))]
            self.heaps[b] = []                                                 # queue cleared (:194)
            self.beams[b] = beam
            for key, n in beam:
                if n.wordid == self.eos and n.prevNode is not None:
                    continue
                rows_b.append(b)
                rows_state.append(n.word_hid)
                rows_tok.append(n.wordid)
        return rows_b, rows_state, rows_tok

    def push(self, top_ix, top_lp):
        r = 0
        for b in range(self.B):
            if self.beams[b] is None:
                continue
            heap = self.heaps[b]
            for key, n in self.beams[b]:
                if n.wordid == self.eos and n.prevNode is not None:
                    heapq.heappush(heap, (key, n))                             # (:200-202)
                    continue
                leng = n.leng + 1
                for j in range(FANOUT):
                    child = BeamSearchNode(None, r, n, int(top_ix[r, j]), top_lp[r, j], leng)
                    heapq.heappush(heap, (-child.eval(), child))               # (:220-223)
                r += 1
            if len(heap) <= self.bw:                                           # (:227-228)
                self.done[b] = True

    def finish(self):
        out = []
        for b in range(self.B):
            _, node = heapq.heappop(self.heaps[b])                             # (:231)
            seq = [node.wordid]
            while node.prevNode is not None:                                   # (:234-236)
                node = node.prevNode
                seq.append(node.wordid)
            out.append(seq[::-1])
        return out


class _Slot(object):
    """heap payload whose comparison answers what BeamSearchNode's does for EQUAL scores: never less."""
    __slots__ = ("i",)

    def __init__(self, i):
        self.i = i

    def __lt__(self, other):
        return False


def _heap_order(keys, m):
    """Indices the reference's heap would pop first, m of them: push in order, pop m times (ties included)."""
    heap = []
    for i, k in enumerate(keys):
        heapq.heappush(heap, (k, _Slot(i)))
    return [heapq.heappop(heap)[1].i for _ in range(m)]


class BeamQueues(object):
    """Same bookkeeping as HeapQueues, vectorised over samples AND candidates (numpy).

    Because the queue is emptied after every pop phase (:194), a sample's heap at depth d is just "the candidates
    pushed at depth d-1, in push order"; popping beam_width entries is a partial sort by key.  Distinct keys sort the
    same way in any heap, so the fast path is one stable argsort over a [B, beam_width*20] key matrix; when two of a
    sample's beam_width+1 smallest keys are EQUAL the pop order depends on the heap's internal layout, and that sample
    falls back to replaying its pushes into a real heap (_heap_order).  Nodes are materialised only when popped
    (<= beam_width per sample and depth instead of 20 x beam_width).
    """

    def __init__(self, B, beam_width, sos, eos):
        self.B, self.bw, self.eos = B, beam_width, eos
        self.NC = max(beam_width * FANOUT, 1)
        # node table (back-trace): token and parent of every popped node; the B roots come first
        self.tok_tab = [np.full(B, sos, dtype=np.int64)]
        self.prev_tab = [np.full(B, -1, dtype=np.int64)]
        self.n_nodes = B
        NC = self.NC
        # candidates of every sample in push order, padded to NC: key (+inf pad), token, parent node, length, state row,
        # node id (-1: not materialised yet)
        self.key = np.full((B, NC), np.inf)
        self.tok = np.zeros((B, NC), dtype=np.int64)
        self.par = np.full((B, NC), -1, dtype=np.int64)
        self.len = np.ones((B, NC), dtype=np.int64)
        self.row = np.zeros((B, NC), dtype=np.int64)
        self.nid = np.full((B, NC), -1, dtype=np.int64)
        self.n = np.ones(B, dtype=np.int64)
        self.key[:, 0] = -0.0
        self.tok[:, 0] = sos
        self.row[:, 0] = np.arange(B)
        self.nid[:, 0] = np.arange(B)
        self.done = np.zeros(B, dtype=bool)
        self.tie_fallbacks = 0
        # score divisor len**0.7 exactly as the reference evaluates it: Python float pow, then fp32 (S2VTModel.py:262-266)
        self.pow07 = np.array([np.float32(pow(float(l), 0.7)) if l > 0 else np.float32(1) for l in range(4096)],
                              dtype=np.float32)

    def all_done(self):
        return bool(self.done.all())

    def _tab(self):
        if len(self.tok_tab) > 1:
            self.tok_tab = [np.concatenate(self.tok_tab)]
            self.prev_tab = [np.concatenate(self.prev_tab)]
        return self.tok_tab[0], self.prev_tab[0]

    def _pop_order(self, m_want):
        """[B, m_want] candidate indices in pop order (entries j >= min(m_want, n_b) are meaningless)."""
        B = self.B
        k = min(m_want + 1, self.NC)
        order = np.argsort(self.key, axis=1, kind="stable")[:, :k]
        ks = np.take_along_axis(self.key, order, axis=1)
        # a tie matters only among the first min(m_want, n) + 1 VALID candidates
        pos = np.arange(1, k)[None, :]
        tie = ((ks[:, 1:] == ks[:, :-1]) & (pos < self.n[:, None]) & (pos <= m_want)).any(axis=1) & ~self.done
        order = order[:, :m_want] if order.shape[1] >= m_want else np.pad(order, ((0, 0), (0, m_want - order.shape[1])))
        for b in np.nonzero(tie)[0]:
            self.tie_fallbacks += 1
            nb = int(self.n[b])
            o = _heap_order(self.key[b, :nb].tolist(), min(m_want, nb))
            order[b, :len(o)] = o
        return order

    def pop(self):
        B, bw = self.B, self.bw
        act = ~self.done
        order = self._pop_order(bw)                                         # [B, bw]
        valid = (np.arange(bw)[None, :] < np.minimum(self.n, bw)[:, None]) & act[:, None]
        g = lambda arr: np.take_along_axis(arr, order, axis=1)
        key, tok, par, ln, row, nid = g(self.key), g(self.tok), g(self.par), g(self.len), g(self.row), g(self.nid)
        # materialise the popped candidates that are not nodes yet, in (sample, beam slot) order
        new = valid & (nid < 0)
        nnew = int(new.sum())
        if nnew:
            nid = nid.copy()
            nid[new] = self.n_nodes + np.arange(nnew)
            self.tok_tab.append(tok[new])
            self.prev_tab.append(par[new])
            self.n_nodes += nnew
        tok_tab, prev_tab = self._tab()
        prev = np.where(valid, prev_tab[np.where(valid, nid, 0)], -1)
        fin = valid & (tok == self.eos) & (prev >= 0)
        exp = valid & ~fin
        self.beam = (key, nid, ln, fin, exp, valid)
        bidx = np.broadcast_to(np.arange(B)[:, None], (B, bw))
        return bidx[exp], row[exp], tok[exp]

    def push(self, top_ix, top_lp):
        B, bw, NC, F = self.B, self.bw, self.NC, FANOUT
        key, nid, ln, fin, exp, valid = self.beam
        _, prev_tab = self._tab()
        size = np.where(exp, F, 0) + fin.astype(np.int64)                   # candidates each beam entry pushes
        off = np.cumsum(size, axis=1) - size                                # their first slot, in beam order
        n_new = size.sum(axis=1)
        act = valid.any(axis=1)
        nk = np.full((B, NC), np.inf)
        nt = np.zeros((B, NC), dtype=np.int64)
        npar = np.full((B, NC), -1, dtype=np.int64)
        nl = np.ones((B, NC), dtype=np.int64)
        nrow = np.zeros((B, NC), dtype=np.int64)
        nnid = np.full((B, NC), -1, dtype=np.int64)
        bidx = np.broadcast_to(np.arange(B)[:, None], (B, bw))
        if fin.any():                                                       # finished entries re-inserted unchanged (:200-202)
            fb, fo = bidx[fin], off[fin]
            nk[fb, fo] = key[fin]
            nt[fb, fo] = self.eos
            npar[fb, fo] = prev_tab[nid[fin]]
            nl[fb, fo] = ln[fin]
            nrow[fb, fo] = -1
            nnid[fb, fo] = nid[fin]
        if exp.any():                                                       # 20 children per expanded entry (:216-223)
            eb, eo, el, en = bidx[exp], off[exp], ln[exp] + 1, nid[exp]
            R = len(eb)
            cols = eo[:, None] + np.arange(F)[None, :]
            rows = eb[:, None]
            # score = fp32 log-prob / fp32(len**0.7); key = -score
            sc = np.asarray(top_lp, dtype=np.float32)[:R] / self.pow07[el][:, None]
            nk[rows, cols] = -sc.astype(np.float64)
            nt[rows, cols] = np.asarray(top_ix)[:R]
            npar[rows, cols] = en[:, None]
            nl[rows, cols] = el[:, None]
            nrow[rows, cols] = np.arange(R)[:, None]
        for dst, src in ((self.key, nk), (self.tok, nt), (self.par, npar), (self.len, nl), (self.row, nrow), (self.nid, nnid)):
            dst[act] = src[act]
        self.n[act] = n_new[act]
        self.done |= act & (n_new <= bw)                                    # (:227-228)

    def finish(self):
        tok_tab, prev_tab = self._tab()
        first = self._pop_order_final()
        out = []
        for b in range(self.B):
            i = int(first[b])                                               # (:231)
            seq = [int(self.tok[b, i])]
            node = int(self.nid[b, i])
            node = int(self.par[b, i]) if node < 0 else int(prev_tab[node])
            while node >= 0:                                                # (:234-236)
                seq.append(int(tok_tab[node]))
                node = int(prev_tab[node])
            out.append(seq[::-1])
        return out

    def _pop_order_final(self):
        saved, self.done = self.done, np.zeros(self.B, dtype=bool)          # frozen samples still pop their best entry
        try:
            return self._pop_order(1)[:, 0]
        finally:
            self.done = saved


def _gemm_strided(a, w, bias, out=None, accumulate=False):
    """a[M,K]·w[N,K]^T where w may be a column slice (row stride > K) of a larger matrix."""
    import ctypes
    from . import capi
    from .functional import _ptr, _stream
    lib = capi.load()
    M, K = a.shape
    N = w.shape[0]
    dev = a.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(M, N, dtype=torch.float32, device=dev)
        capi.check(lib.s2vt_gemm_f32(1, 1, M, N, K, _ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(out),
                                     out.stride(0), _ptr(bias), int(accumulate), _stream(dev)), "s2vt_gemm_f32")
    return out
