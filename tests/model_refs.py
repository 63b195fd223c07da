"""Plain fp64 restatements on the CPU of what the per-op autograd glue computes (att_functional._Affine / _LstmLayer,
gru_functional._GruLayer, and the three model variants built on them): an affine map, one GRU layer forward and its
hand-written BPTT, the whole S2VT(rnn_type='gru') train forward, the whole Att_Baseline train forward and the reference's
MaskCriterion arithmetic.  tests/test_model_refs_host.py holds them to what the reference itself recorded
(tests/golden/gru_tiny.npz, att_tiny.npz) and to torch's fp64 autograd; tests/test_gpu_model_variants.py compares the HIP
paths with them."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def d64(t):
    return t.detach().double().cpu()


def affine64(x, w, b=None):
    """y = x W^T (+ b), x [M, K], W [N, K]"""
    y = x.double() @ w.double().t()
    return y if b is None else y + b.double()


# ------------------------------------------------------------------------------------------------------------ GRU layer
def gru_cell64(gi, h, w_hh, b_hh):
    """One nn.GRU step from the gate input gi [B, 3H] (= x W_ih^T + b_ih): gate order r, z, n, b_hn inside the r product.
    Returns (h', r, z, n, ghn)."""
    H = w_hh.shape[1]
    gh = h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return n + z * (h - n), r, z, n, gh[:, 2 * H:]


def gru_layer64(gx, n_gx, b_ih, w_hh, b_hh, T, B):
    """A GRU layer from the zero state over time-major gate inputs gx [n_gx*B, 3H]; the steps >= n_gx see b_ih alone.
    Returns (h_all [T*B, H], stash [T*B, 4H] = r, z, n, ghn)."""
    H = w_hh.shape[1]
    h = torch.zeros(B, H, dtype=F64)
    hs, st = [], []
    for t in range(T):
        gi = gx[t * B:(t + 1) * B] if t < n_gx else b_ih.expand(B, -1)
        h, r, z, n, ghn = gru_cell64(gi, h, w_hh, b_hh)
        hs.append(h)
        st.append(torch.cat([r, z, n, ghn], 1))
    return torch.cat(hs), torch.cat(st)


def gru_bptt64(w_hh, dh_out, dh_first, h_all, stash, T, B):
    """BPTT of a GRU layer from a GIVEN h_all [T*B, H] and stash [T*B, 4H]; dh_out [(T-dh_first)*B, H] (or None) is the upstream
    gradient of the outputs of the steps >= dh_first.  Returns (dgx, dgh) [T*B, 3H]: dgx = the gradient of the gate input,
    dgh = the gradient of h W_hh^T + b_hh (its n block is dn * r)."""
    H = w_hh.shape[1]
    dh = torch.zeros(B, H, dtype=F64)
    dgx = torch.zeros(T * B, 3 * H, dtype=F64)
    dgh = torch.zeros(T * B, 3 * H, dtype=F64)
    for t in range(T - 1, -1, -1):
        if dh_out is not None and t >= dh_first:
            dh = dh + dh_out[(t - dh_first) * B:(t - dh_first + 1) * B]
        s = stash[t * B:(t + 1) * B]
        r, z, n, ghn = s[:, :H], s[:, H:2 * H], s[:, 2 * H:3 * H], s[:, 3 * H:]
        hp = h_all[(t - 1) * B:t * B] if t else torch.zeros(B, H, dtype=F64)
        dn = dh * (1 - z) * (1 - n * n)
        dz = dh * (hp - n) * z * (1 - z)
        dr = dn * ghn * r * (1 - r)
        dgx[t * B:(t + 1) * B] = torch.cat([dr, dz, dn], 1)
        dgh[t * B:(t + 1) * B] = torch.cat([dr, dz, dn * r], 1)
        dh = dh * z + dgh[t * B:(t + 1) * B] @ w_hh
    return dgx, dgh


# ----------------------------------------------------------------------------------------------------------- whole models
def leaves64(named_parameters):
    """{name: fp64 CPU leaf} of a model's (or a state_dict's) tensors"""
    return {k: d64(v).requires_grad_() for k, v in named_parameters}


def _rnn64(cls, P, prefix, x, suffix=""):
    """one single-layer unidirectional fp64 nn.LSTM / nn.GRU (batch_first) with the weights `prefix.*_l0<suffix>` of P"""
    cell = cls(x.shape[2], P[prefix + ".weight_hh_l0" + suffix].shape[1], batch_first=True).double()
    out, _ = torch.func.functional_call(cell, {k + "_l0": P["%s.%s_l0%s" % (prefix, k, suffix)]
                                               for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}, (x,))
    return out


def gru_model64(P, feats, caps_in, out_mask=None):
    """S2VT(rnn_type='gru').forward(mode='train'): feat_linear; vid_rnn over the L frames and L-1 zero steps; word_rnn over
    [Emb | vid_rnn's output] with zero embeddings for the first L steps; out_linear on the (masked) last L-1 outputs.
    P: fp64 leaves; caps_in [B, L-1]; out_mask [B, L-1, H] or None.  Returns logits [B, L-1, V]."""
    feats = d64(feats)
    B, L, _ = feats.shape
    H, E = P["feat_linear.weight"].shape[0], P["embedding.weight"].shape[1]
    x = feats @ P["feat_linear.weight"].t() + P["feat_linear.bias"]
    v = _rnn64(torch.nn.GRU, P, "vid_rnn", torch.cat([x, torch.zeros(B, L - 1, H, dtype=F64)], 1))
    emb = P["embedding.weight"][caps_in.cpu()]
    w = _rnn64(torch.nn.GRU, P, "word_rnn", torch.cat([torch.cat([torch.zeros(B, L, E, dtype=F64), emb], 1), v], 2))
    res = w[:, L:]
    if out_mask is not None:
        res = res * d64(out_mask)
    return res @ P["out_linear.weight"].t() + P["out_linear.bias"]


def att_model64(P, feats, targets, feat_mask=None, out_mask=None):
    """Att_Baseline.forward(mode='train') as the reference computes it: feat_linear on the (masked) frames, a bidirectional LSTM
    encoder, context = the SUM of the encoder outputs over the frames (its attention weights are a softmax over a dimension of
    size one: all 1, the same context at every step), an LSTM decoder over [Emb | context], out_linear on the (masked)
    outputs.  The three attention layers join with an exactly-zero contribution, so their gradients are zeros, not None.
    feat_mask [B, L, F]; out_mask [B, L-1, H] batch-major.  Returns logits [B, L-1, V]."""
    feats = d64(feats)
    B, L, _ = feats.shape
    T = L - 1
    if feat_mask is not None:
        feats = feats * d64(feat_mask)
    x = feats @ P["feat_linear.weight"].t() + P["feat_linear.bias"]
    fwd = _rnn64(torch.nn.LSTM, P, "encoder", x)
    rev = _rnn64(torch.nn.LSTM, P, "encoder", x.flip(1), "_reverse").flip(1)
    ctx = torch.cat([fwd, rev], 2).sum(1, keepdim=True)
    ctx = ctx + sum(P[k].sum() for k in ("att_enc.weight", "att_enc.bias", "att_prev_hid.weight", "att_prev_hid.bias",
                                         "att_apply.weight")) * 0.0
    emb = F.embedding(targets[:, :T].cpu(), P["embedding.weight"], padding_idx=0)
    dec = _rnn64(torch.nn.LSTM, P, "decoder", torch.cat([emb, ctx.expand(B, T, -1)], 2))
    if out_mask is not None:
        dec = dec * d64(out_mask)
    return dec @ P["out_linear.weight"].t() + P["out_linear.bias"]


def reference_criterion64(logits, caps, mask):
    """The reference's MaskCriterion (utils.py:22-25): the inner loss is already the UNMASKED mean cross-entropy over all
    B*(L-1) positions; weighting it by the mask and dividing by the mask's sum returns that mean."""
    V = logits.shape[-1]
    ce = F.cross_entropy(logits.reshape(-1, V), caps[:, 1:].reshape(-1).cpu(), reduction="mean")
    w = d64(mask)[:, 1:].reshape(-1)
    return (ce * w).sum() / w.sum()
