"""Autograd glue for S2VT built with num_layers > 1 (S2VTModel.py:11-22: nn.LSTM(num_layers=N) for vid_rnn and word_rnn) over the
chain entry points of libs2vt_hip.so: both recurrences are one chain of 2N layers run as a layer wavefront (s2vt_lstm_chain_fwd /
s2vt_lstm_chain_bwd, csrc/lstm_stack.hip); the projections and the weight gradients are att_functional.affine / ops.gemm, so
they follow the library's GEMM mode.  PyTorch holds the tensors and wires the autograd graph.

Chain order: vid_l0 .. vid_l(N-1), word_l0 (input [Emb | vid top]: the embedding half is a precomputed gate input for the steps
>= L, the vid half a dense input segment of the kernel), word_l1 .. word_l(N-1).  nn.LSTM's inter-layer dropout
(S2VTModel.py:17-20, `rnn_dropout`) is a mask on the output of every layer of an nn.LSTM but its last, applied while the model
is training; there is none between vid_rnn and word_rnn.
"""
import torch
import torch.nn.functional as F

from . import capi, ops
from .att_functional import affine, lstm_layer
from .functional import _ptr, _stream, _f32c


def is_stacked_lstm_model(model):
    """Both recurrences are unidirectional nn.LSTM with biases and num_layers >= 2: the configuration this module implements."""
    return all(isinstance(r, torch.nn.LSTM) and r.num_layers >= 2 and not r.bidirectional and r.bias
               for r in (model.vid_rnn, model.word_rnn))


def _layer(rnn, k):
    return (getattr(rnn, "weight_ih_l%d" % k), getattr(rnn, "weight_hh_l%d" % k), getattr(rnn, "bias_ih_l%d" % k),
            getattr(rnn, "bias_hh_l%d" % k))


def draw_rnn_masks(model, T, B, device):
    """The inter-layer dropout masks of S2VT.forward in training: time-major [T*B, H], entries 0 or 1/(1-p), for the N-1
    boundaries of vid_rnn, then the N-1 of word_rnn (F.dropout on a ones tensor on the device).  torch's CPU generator, which
    nn.LSTM's dropout draws from in the reference, cannot be reproduced on the device: the masks have its distribution, not its
    values.  None when no dropout applies."""
    p = float(model.vid_rnn.dropout)
    N = model.vid_rnn.num_layers
    if not model.training or p <= 0 or N < 2:
        return None
    ones = torch.ones(T * B, model.dim_hid, dtype=torch.float32, device=device)
    return [F.dropout(ones, p=p, training=True) for _ in range(2 * (N - 1))]


class _Chain(torch.autograd.Function):
    """Decode-step outputs [(L-1)*B, H] of the top word layer, time-major.  Inputs: gx_v (vid_l0's gate input for the L frames,
    biases included), gx_w (word_l0's embedding half for steps >= L, biases included), then per layer j of the chain its summed
    bias b_ih + b_hh, weight_hh and input-weight block (None for j = 0).  `masks`: per layer, its output mask or None."""

    @staticmethod
    def forward(ctx, T, B, L, N, masks, gx_v, gx_w, *lp):
        n = 2 * N
        H = lp[1].shape[1]
        dev = gx_v.device
        bias = [lp[3 * j].detach().contiguous() for j in range(n)]
        w_hh = [_f32c(lp[3 * j + 1].detach(), "weight_hh") for j in range(n)]
        # word_l0's block is the strided view weight_ih_l0[:, E:] (row stride E + H), handed over as it is
        w_in = [None] + [_rows(lp[3 * j + 2].detach(), "weight_ih") for j in range(1, n)]
        with torch.cuda.device(dev):
            layers = []
            for j in range(n):
                lay = dict(w_hh=w_hh[j], w_in=w_in[j], bias=bias[j], mask=masks[j],
                           h=torch.empty(T * B, H, dtype=torch.float32, device=dev),
                           c=torch.empty(T * B, H, dtype=torch.float32, device=dev),
                           stash=torch.empty(T * B, 4 * H, dtype=torch.float32, device=dev),
                           hm=torch.empty(T * B, H, dtype=torch.float32, device=dev) if masks[j] is not None else None)
                if j == 0:
                    lay.update(gx=gx_v.contiguous(), gx_t0=0, n_gx=L)
                elif j == N:
                    lay.update(gx=gx_w.contiguous(), gx_t0=L, n_gx=L - 1)
                layers.append(lay)
            ops.lstm_chain_fwd(T, B, H, layers)
        ctx.layers, ctx.T, ctx.B, ctx.L, ctx.N, ctx.used = layers, T, B, L, N, False
        return layers[-1]["h"][L * B:]

    @staticmethod
    def backward(ctx, dh):
        if ctx.used:
            raise RuntimeError("the saved gate stashes of this LSTM chain were consumed by an earlier backward (retain_graph is not supported)")
        ctx.used = True
        layers, T, B, L, N = ctx.layers, ctx.T, ctx.B, ctx.L, ctx.N
        n = 2 * N
        layers[-1].update(dh_ext=dh.contiguous(), dh_t0=L)
        for lay in layers:
            lay["dg"] = lay["stash"]                     # dG over the stash, in place
        H = layers[0]["h"].shape[1]
        ops.lstm_chain_bwd(T, B, H, layers)
        grads = [None] * (3 * n)
        for j, lay in enumerate(layers):
            dg = lay["dg"]
            if j == 0:
                db = dg[L * B:].sum(0)
            elif j == N:
                db = dg[:L * B].sum(0)
            else:
                db = dg.sum(0)
            grads[3 * j] = db
            grads[3 * j + 1] = ops.gemm(dg[B:], lay["h"][:-B], a_kmajor=False, b_kmajor=False)      # [4H,(T-1)B]·[(T-1)B,H]
            if j > 0:
                below = layers[j - 1]
                x = below["hm"] if below["hm"] is not None else below["h"]
                grads[3 * j + 2] = ops.gemm(dg, x, a_kmajor=False, b_kmajor=False)                  # [4H,TB]·[TB,H]
        dgx_v = layers[0]["dg"][:L * B]
        dgx_w = layers[N]["dg"][L * B:]
        ctx.layers = None
        return (None, None, None, None, None, dgx_v, dgx_w) + tuple(grads)


def _rows(t, name):
    """float32 HIP rows with a unit column stride (a column block of a wider weight stays a view)"""
    _f32c(t[:1, :1], name)
    return t if t.stride(1) == 1 else t.contiguous()


def _chain_inputs(model, feats, targets):
    """gx of vid_l0 and word_l0's embedding half (autograd-tracked projections), and the flat per-layer parameter list."""
    B, L, Fd = feats.shape
    H, E, V = model.dim_hid, model.dim_embed, model.vocab_size
    N = model.vid_rnn.num_layers
    x1 = affine(feats.reshape(B * L, Fd), model.feat_linear.weight, model.feat_linear.bias)        # feat_linear (:52-53)
    x_tm = x1.view(B, L, H).transpose(0, 1).reshape(L * B, H)
    lp = []
    for rnn in (model.vid_rnn, model.word_rnn):
        for k in range(N):
            w_ih, w_hh, b_ih, b_hh = _layer(rnn, k)
            b = b_ih + b_hh
            if k == 0 and rnn is model.vid_rnn:
                gx_v = affine(x_tm, w_ih, b)
                w_in = None
            elif k == 0:
                # the word ids of S2VTModel.py:71 through the library's guard: an id outside the vocabulary raises IndexError at
                # the next capi.check_async_error(); the gather itself only sees valid rows
                tok = ops.tokens_time_major(targets, L - 1, V).long()
                gx_w = affine(F.embedding(tok, model.embedding.weight), w_ih[:, :E], b)              # [(L-1)*B, 4H]
                w_in = w_ih[:, E:]
            else:
                w_in = w_ih
            lp += [b, w_hh, w_in]
    return gx_v, gx_w, lp


def train_forward(model, feats, targets, out_mask=None, rnn_masks=None):
    """mode='train' (S2VTModel.py:63-81) of a stacked model: logits [B, L-1, V].  `out_mask`: the out_drop mask [B, L-1, H] or
    None.  `rnn_masks`: None, or the 2(N-1) inter-layer masks of draw_rnn_masks (vid boundaries, then word boundaries)."""
    B, L, _ = feats.shape
    H, V = model.dim_hid, model.vocab_size
    N = model.vid_rnn.num_layers
    T = 2 * L - 1
    if targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] != L - 1:
        raise ValueError("targets must be [B, L-1] = [%d, %d], got %s" % (B, L - 1, tuple(targets.shape)))
    masks = _layer_masks(N, rnn_masks, T * B, H)
    gx_v, gx_w, lp = _chain_inputs(model, feats, targets)
    top = _Chain.apply(T, B, L, N, masks, gx_v, gx_w, *lp)                                         # [(L-1)*B, H]
    res = top.view(L - 1, B, H).transpose(0, 1).reshape(B * (L - 1), H)
    if out_mask is not None:
        res = res * out_mask.reshape(B * (L - 1), H)
    logits = affine(res, model.out_linear.weight, model.out_linear.bias)
    return logits.view(B, L - 1, V)


def _layer_masks(N, rnn_masks, rows, H):
    """per chain layer: its output mask or None (vid top and word top have none)"""
    masks = [None] * (2 * N)
    if rnn_masks is None:
        return masks
    if len(rnn_masks) != 2 * (N - 1):
        raise ValueError("rnn_masks: %d masks for %d layers, expected %d" % (len(rnn_masks), N, 2 * (N - 1)))
    for i, m in enumerate(rnn_masks):
        if tuple(m.shape) != (rows, H):
            raise ValueError("rnn_masks[%d] must be [%d, %d], got %s" % (i, rows, H, tuple(m.shape)))
        masks[i if i < N - 1 else i + 1] = _f32c(m, "rnn_masks[%d]" % i)
    return masks


@torch.no_grad()
def greedy_decode(model, feats, sos_ix, sample=None, ss=None, constraints=None):
    """mode='test' (S2VTModel.py:82-110) of a stacked model: ids int64 [B, L-1]; sample = (temperature, seed): mode='sample', the
    same loop with s2vt_decode_step_sample in place of the arg-max ((temperature, seed, top_k, top_p): the logits GEMM and the
    truncated draw, ops.decode_step_token_into).  constraints = a sampling.ConstraintSpec: every step's head is the logits
    GEMM and the constrained draw on the loop's packed words (S2VT.decode_constrained).
    ss = (targets, ss_prob, seed): the scheduled-sampling pass -
    the token layer of every step takes the coin's word, no dropout masks are drawn, and (used, draws) are returned.  The vid chain over T steps, the word chain's
    encode over the first L steps, then L-1 decode steps of one word-chain call each (T = 1, the previous step's state, the packed
    argmax word read on the device) followed by s2vt_decode_step_argmax.  No host synchronisation inside the loop.  In training
    mode with rnn_dropout > 0, masks are drawn as nn.LSTM would apply them."""
    B, L, Fd = feats.shape
    H, E, V = model.dim_hid, model.dim_embed, model.vocab_size
    N = model.vid_rnn.num_layers
    T = 2 * L - 1
    dev = feats.device
    p = float(model.vid_rnn.dropout) if (model.training and ss is None) else 0.0

    def mask(rows):
        return F.dropout(torch.ones(rows, H, dtype=torch.float32, device=dev), p=p, training=True) if p > 0 else None

    def f32(t, name):
        return _f32c(t.detach(), name)

    def stack(rnn, rows, first):
        out = []
        for k in range(N):
            w_ih, w_hh, b_ih, b_hh = _layer(rnn, k)
            lay = dict(w_hh=f32(w_hh, "weight_hh"), bias=(b_ih.detach() + b_hh.detach()).contiguous(),
                       w_in=None if k == 0 else f32(w_ih, "weight_ih"), mask=mask(rows) if k < N - 1 else None)
            out.append(lay)
        out[0].update(first)
        return out

    with torch.cuda.device(dev):
        x1 = ops.gemm(feats.reshape(B * L, Fd), f32(model.feat_linear.weight, "feat_linear.weight"),
                      bias=f32(model.feat_linear.bias, "feat_linear.bias"))
        x_tm = x1.view(B, L, H).transpose(0, 1).reshape(L * B, H)
        v0 = _layer(model.vid_rnn, 0)
        gx_v = ops.gemm(x_tm, f32(v0[0], "vid_rnn.weight_ih_l0"), bias=(v0[2].detach() + v0[3].detach()).contiguous())
        vid = stack(model.vid_rnn, T * B, dict(gx=gx_v, gx_t0=0, n_gx=L))
        ops.lstm_chain_fwd(T, B, H, _with_outputs(vid, T * B, H, dev))
        vtop = vid[-1]["h"]
        w0 = f32(_layer(model.word_rnn, 0)[0], "word_rnn.weight_ih_l0")
        w_v = w0[:, E:]
        word = stack(model.word_rnn, L * B, dict(x_in=vtop[:L * B], w_in=w_v))                      # encode (:86-87)
        ops.lstm_chain_fwd(L, B, H, _with_outputs(word, L * B, H, dev))
        state = [(lay["h"][(L - 1) * B:], lay["c"][(L - 1) * B:]) for lay in word]
        emb = f32(model.embedding.weight, "embedding.weight")
        wo, bo = f32(model.out_linear.weight, "out_linear.weight"), f32(model.out_linear.bias, "out_linear.bias")
        bufs = [[_with_outputs([dict()], B, H, dev, hm=p > 0)[0] for _ in range(N)] for _ in range(2)]
        packed = torch.zeros(L - 1, B, dtype=torch.int64, device=dev)
        for i in range(L - 1):
            step = stack(model.word_rnn, B, dict(x_in=vtop[(L + i) * B:(L + i + 1) * B], w_in=w_v, emb=emb, w_e=w0, E=E, V=V,
                                                 tok_packed=packed[i - 1] if i else None, tok_const=int(sos_ix),
                                                 ss=None if ss is None else ss + (i,)))
            for k, lay in enumerate(step):
                lay.update(h0=state[k][0], c0=state[k][1], h=bufs[i % 2][k]["h"], c=bufs[i % 2][k]["c"])
                if lay["mask"] is not None:
                    lay["hm"] = bufs[i % 2][k]["hm"]
            ops.lstm_chain_fwd(1, B, H, step)
            state = [(lay["h"], lay["c"]) for lay in step]
            ops.decode_step_token_into(state[-1][0], wo, bo, packed[i], sample=sample, step=i,
                                       constraints=None if constraints is None else (constraints, packed, i))
    capi.check_async_error(wait=False)
    if ss is not None:
        return ops.ss_unpack(packed, *ss)
    return (0xFFFFFFFF - (packed & 0xFFFFFFFF)).t().contiguous()


def scheduled_inputs(model, feats, targets, ss_prob, temperature=None, seed=None, return_draws=False):
    """functional.scheduled_inputs for a stacked model: the decode loop above with the coin in front of every token step
    (inference arithmetic: no dropout masks, no gradient)."""
    from .functional import check_scheduled_args
    B, L, _ = feats.shape
    targets, ss_prob, temperature, seed = check_scheduled_args(targets, B, L - 1, ss_prob, temperature, seed)
    used, draws = greedy_decode(model, feats, 0, sample=None if temperature is None else (temperature, seed),
                                ss=(targets, ss_prob, seed))
    return (used, draws) if return_draws else used


def _with_outputs(layers, rows, H, dev, hm=False):
    for lay in layers:
        lay["h"] = torch.empty(rows, H, dtype=torch.float32, device=dev)
        lay["c"] = torch.empty(rows, H, dtype=torch.float32, device=dev)
        if hm or lay.get("mask") is not None:
            lay["hm"] = torch.empty(rows, H, dtype=torch.float32, device=dev)
    return layers


def reference_layerwise(model, feats, targets, out_mask=None, rnn_masks=None):
    """The same train forward as train_forward, run layer by layer on the one-layer entry points (s2vt_lstm_seq_fwd / _bwd
    through att_functional.lstm_layer, the input projections as batched GEMMs).  A device-side reference for the tests and the
    A/B leg of tools/bench_stack.py; not a run-time option of the package."""
    B, L, Fd = feats.shape
    H, E, V = model.dim_hid, model.dim_embed, model.vocab_size
    N = model.vid_rnn.num_layers
    T = 2 * L - 1
    masks = _layer_masks(N, rnn_masks, T * B, H)
    x1 = affine(feats.reshape(B * L, Fd), model.feat_linear.weight, model.feat_linear.bias)
    x = x1.view(B, L, H).transpose(0, 1).reshape(L * B, H)
    j = 0
    for k in range(N):                                                    # vid_rnn
        w_ih, w_hh, b_ih, b_hh = _layer(model.vid_rnn, k)
        b = b_ih + b_hh
        if k == 0:
            gx = torch.cat([affine(x, w_ih, b), b.expand((T - L) * B, 4 * H)])
        else:
            gx = affine(x, w_ih, b)
        h = lstm_layer(gx, w_hh, T, B)
        x = h * masks[j] if masks[j] is not None else h
        j += 1
    tok = ops.tokens_time_major(targets, L - 1, V).long()
    for k in range(N):                                                    # word_rnn
        w_ih, w_hh, b_ih, b_hh = _layer(model.word_rnn, k)
        b = b_ih + b_hh
        if k == 0:
            gx = affine(x, w_ih[:, E:], b)
            gx_e = affine(F.embedding(tok, model.embedding.weight), w_ih[:, :E], None)
            gx = torch.cat([gx[:L * B], gx[L * B:] + gx_e])
        else:
            gx = affine(x, w_ih, b)
        h = lstm_layer(gx, w_hh, T, B)
        x = h * masks[j] if masks[j] is not None else h
        j += 1
    res = h[L * B:].view(L - 1, B, H).transpose(0, 1).reshape(B * (L - 1), H)
    if out_mask is not None:
        res = res * out_mask.reshape(B * (L - 1), H)
    return affine(res, model.out_linear.weight, model.out_linear.bias).view(B, L - 1, V)
