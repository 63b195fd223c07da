"""Autograd glue for S2VT built with rnn_type='gru' (S2VTModel.py:11-22: nn.GRU in place of nn.LSTM, the rest of the network
unchanged) over the per-op C-ABI entry points of libs2vt_hip.so: the projections and their gradients are att_functional.affine
(split-precision plane GEMMs in gemm mode 3, s2vt_gemm_f32 otherwise), both recurrences s2vt_gru_seq_fwd / s2vt_gru_seq_bwd
(the fused GRU timestep kernels of csrc/gru.hip), the greedy loop s2vt_gru_step_fwd_token + s2vt_decode_step_argmax.  PyTorch
holds the tensors and wires the autograd graph.

The structure is the LSTM model's (S2VTModel.py:48-110): feat_linear; vid_rnn over the L frames and L-1 zero steps; word_rnn over
[Emb | vid_rnn's output] with zero embeddings for the first L steps; out_linear on word_rnn's last L-1 outputs.  torch's gate order
r, z, n; b_ih joins the gate input, b_hh is added inside the kernels (b_hn sits inside the r product).
"""
import ctypes

import torch
import torch.nn.functional as F

from . import capi, ops
from .att_functional import affine
from .functional import _ptr, _stream, _f32c


class _GruLayer(torch.autograd.Function):
    """h_all [T*B, H] = one GRU layer from the zero state over time-major gate inputs gx [n_gx*B, 3H] (= x W_ih^T + b_ih; the
    steps >= n_gx see b_ih alone).  BPTT: d gx = dGx of the first n_gx steps, d b_ih = the column sums of the rest,
    dW_hh = sum_t dGh_t^T h_{t-1}, db_hh = sum_t dGh_t."""

    @staticmethod
    def forward(ctx, gx, b_ih, w_hh, b_hh, T, B, n_gx):
        w_hh, b_hh = w_hh.contiguous(), b_hh.contiguous()
        h, stash = ops.gru_seq_fwd(T, B, gx.contiguous() if n_gx else None, n_gx, b_ih.contiguous() if b_ih is not None else None,
                                   w_hh, b_hh, want_stash=True)
        ctx.save_for_backward(w_hh, h, stash)
        ctx.T, ctx.B, ctx.n_gx, ctx.has_b_ih = T, B, n_gx, b_ih is not None
        return h

    @staticmethod
    def backward(ctx, dh):
        w_hh, h, stash = ctx.saved_tensors
        T, B, n_gx = ctx.T, ctx.B, ctx.n_gx
        dgx, dgh = ops.gru_seq_bwd(T, B, w_hh, dh.contiguous(), 0, h, stash)
        dgx_in = dgx[:n_gx * B] if n_gx else None
        db_ih = dgx[n_gx * B:].sum(0) if (ctx.has_b_ih and n_gx < T) else None
        if T > 1:
            dw = ops.gemm(dgh[B:], h[:-B], a_kmajor=False, b_kmajor=False)          # [3H, (T-1)B]·[(T-1)B, H]
        else:
            dw = torch.zeros_like(w_hh)
        return dgx_in, db_ih, dw, dgh.sum(0), None, None, None


def gru_layer(gx, b_ih, w_hh, b_hh, T, B, n_gx):
    return _GruLayer.apply(gx, b_ih, w_hh, b_hh, T, B, n_gx)


def is_gru_model(model):
    """The model's recurrences are one-layer unidirectional nn.GRU with biases: the configuration this module implements."""
    return all(isinstance(r, torch.nn.GRU) and r.num_layers == 1 and not r.bidirectional and r.bias
               for r in (model.vid_rnn, model.word_rnn))


def _rnn(rnn):
    return rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0


def _encode_frames(model, feats):
    """feat_linear (S2VTModel.py:52-53) -> time-major rows [L*B, H], then vid_rnn's gate input for the L frames."""
    B, L, Fd = feats.shape
    H = model.dim_hid
    x1 = affine(feats.reshape(B * L, Fd), model.feat_linear.weight, model.feat_linear.bias)       # batch-major rows
    x_tm = x1.view(B, L, H).transpose(0, 1).reshape(L * B, H)
    w_ih, _, b_ih, _ = _rnn(model.vid_rnn)
    return affine(x_tm, w_ih, b_ih)


def train_forward(model, feats, targets, out_mask=None):
    """mode='train' (S2VTModel.py:63-81): logits [B, L-1, V].  `out_mask`: the out_drop mask [B, L-1, H] (entries 0 or 1/(1-p))
    or None."""
    B, L, _ = feats.shape
    H, E, V = model.dim_hid, model.dim_embed, model.vocab_size
    T = 2 * L - 1
    if targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] != L - 1:
        raise ValueError("targets must be [B, L-1] = [%d, %d], got %s" % (B, L - 1, tuple(targets.shape)))
    _, v_whh, v_bih, v_bhh = _rnn(model.vid_rnn)
    h1 = gru_layer(_encode_frames(model, feats), v_bih, v_whh, v_bhh, T, B, L)                    # [T*B, H]
    w_ih, w_hh, b_ih, b_hh = _rnn(model.word_rnn)
    gx = affine(h1, w_ih[:, E:], b_ih)                                                              # vid half, every step
    # the word ids of S2VTModel.py:71 through the library's guard: an id outside the vocabulary raises IndexError at the next
    # capi.check_async_error() (dp.train_step checks before the optimiser step), the gather itself only sees valid rows
    tok = ops.tokens_time_major(targets, L - 1, V).long()
    gx_e = affine(F.embedding(tok, model.embedding.weight), w_ih[:, :E], None)                      # [(L-1)*B, 3H]
    gx = torch.cat([gx[:L * B], gx[L * B:] + gx_e])
    h2 = gru_layer(gx, None, w_hh, b_hh, T, B, T)
    res = h2[L * B:].view(L - 1, B, H).transpose(0, 1).reshape(B * (L - 1), H)                      # batch-major decode outputs
    if out_mask is not None:
        res = res * out_mask.reshape(B * (L - 1), H)
    logits = affine(res, model.out_linear.weight, model.out_linear.bias)
    return logits.view(B, L - 1, V)


@torch.no_grad()
def greedy_decode(model, feats, sos_ix, sample=None, ss=None, constraints=None):
    """mode='test' (S2VTModel.py:82-110): ids int64 [B, L-1]; sample = (temperature, seed): mode='sample', the same loop with
    s2vt_decode_step_sample in place of the arg-max ((temperature, seed, top_k, top_p): the logits GEMM and the truncated draw,
    ops.decode_step_token_into).  constraints = a sampling.ConstraintSpec: every step's head is the logits
    GEMM and the constrained draw on the loop's packed words (S2VT.decode_constrained).
    ss = (targets, ss_prob, seed): the scheduled-sampling pass - every token
    step is s2vt_gru_step_fwd_token_ss, and (used, draws) are returned instead of the ids.  vid_rnn without a stash, word_rnn's encode over the first L steps,
    then L-1 decode steps of s2vt_gru_step_fwd_token (the previous step's packed argmax word is read on the device) and
    s2vt_decode_step_argmax.  No host synchronisation inside the loop: <sos> is checked on the host by the first step, and the
    packed words are in range by construction, so no step posts a device error flag."""
    B, L, _ = feats.shape
    H, E, V = model.dim_hid, model.dim_embed, model.vocab_size
    T = 2 * L - 1
    _, v_whh, v_bih, v_bhh = _rnn(model.vid_rnn)
    h1, _ = ops.gru_seq_fwd(T, B, _encode_frames(model, feats), L, v_bih.detach(), v_whh.detach(), v_bhh.detach())
    w_ih, w_hh, b_ih, b_hh = (p.detach() for p in _rnn(model.word_rnn))
    w_ih, w_hh, b_hh = _f32c(w_ih, "word_rnn.weight_ih_l0"), _f32c(w_hh, "word_rnn.weight_hh_l0"), _f32c(b_hh, "word_rnn.bias_hh_l0")
    w_v = w_ih[:, E:].contiguous()
    h_enc, _ = ops.gru_seq_fwd(L, B, ops.gemm(h1[:L * B], w_v, bias=b_ih.contiguous()), L, None, w_hh, b_hh)   # encode (:86-87)
    gx_dec = ops.gemm(h1[L * B:], w_v, bias=b_ih.contiguous())                                     # vid half of the L-1 steps
    emb = _f32c(model.embedding.weight.detach(), "embedding.weight")
    wo, bo = _f32c(model.out_linear.weight.detach(), "out_linear.weight"), _f32c(model.out_linear.bias.detach(), "out_linear.bias")
    dev = feats.device
    h = h_enc[(L - 1) * B:]
    with torch.cuda.device(dev):
        packed = torch.zeros(L - 1, B, dtype=torch.int64, device=dev)
        hs = torch.empty(2, B, H, dtype=torch.float32, device=dev)
        for i in range(L - 1):
            h = ops.gru_step_fwd_token(gx_dec[i * B:(i + 1) * B], w_hh, b_hh, h, emb, w_ih, tok_packed=packed[i - 1] if i else None,
                                       tok_const=int(sos_ix), out=hs[i % 2], ss=None if ss is None else ss + (i,))
            ops.decode_step_token_into(h, wo, bo, packed[i], sample=sample, step=i,
                                       constraints=None if constraints is None else (constraints, packed, i))
    capi.check_async_error(wait=False)
    if ss is not None:
        return ops.ss_unpack(packed, *ss)
    return (0xFFFFFFFF - (packed & 0xFFFFFFFF)).t().contiguous()


def scheduled_inputs(model, feats, targets, ss_prob, temperature=None, seed=None, return_draws=False):
    """functional.scheduled_inputs for a GRU model: the greedy / sampled decode loop above with the coin in front of every
    token step (inference arithmetic, no gradient)."""
    from .functional import check_scheduled_args
    B, L, _ = feats.shape
    targets, ss_prob, temperature, seed = check_scheduled_args(targets, B, L - 1, ss_prob, temperature, seed)
    used, draws = greedy_decode(model, feats, 0, sample=None if temperature is None else (temperature, seed),
                                ss=(targets, ss_prob, seed))
    return (used, draws) if return_draws else used
