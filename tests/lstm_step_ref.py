"""Plain fp64 restatements on the CPU of the fp32 launch-per-timestep LSTM kernels (csrc/lstm.hip: lstm_step_fwd / lstm_step_bwd;
csrc/api_shared.hip: seq_fwd / seq_bwd) with every optional input nullable, and the inputs the tests feed them.

  step_bwd      one BPTT step from the activated gates: dh = dh_out? + dg_next? . W_hh, dc = dh.o.(1 - tanh^2 c) + dc_in?, the four
                pre-activation gradients, dc_prev = dc.f.  None for dg_next / dh_out / dc_in / c_prev is the zero the kernel takes
                for a null pointer (dc_in None = dc_is_zero).
  cell_fwd      one forward step from the gate input (gx [B, 4H] or a bias [4H]) and the state (None = zero).
  layer_fwd / layer_bwd   a layer from the zero state and its BPTT, with the arguments of ops.lstm_seq_fwd / ops.lstm_seq_bwd.
  dw_from_dg    dW_hh = sum_t dG_t^T h_{t-1}.

`dtype` is the precision the formulas are evaluated in: float64 (the reference) or float32 (how far plain fp32 arithmetic on the
host lands from it: the room the GPU bounds leave).  tests/test_lstm_step_ref_host.py holds all of this to torch's fp64 autograd;
tests/test_gpu_lstm_step_edges.py compares the kernels with it.

The step inputs are those of test_gpu_kernels.py::test_lstm_step_bwd_matches_autograd (w_hh U(+-1/sqrt(H)) seed 1, gx seed 2, c_prev
seed 4, dh_out seed 5, dc seed 6, dg_next seed 7 scaled 0.1; the activated gates and c derived from gx and c_prev), the bounds
those of that test, of test_lstm_step_fwd_matches_cell and of test_lstm_seq_fwd_bwd_vs_autograd."""
import functools

import torch

F64 = torch.float64

# absolute bounds on the device results (fp32 kernels against the fp64 reference)
TOL_DG = 5e-6          # dG and dc_prev of a backward step / of a layer's BPTT
TOL_H = 2e-6           # h and the activated gates of a forward step / layer
TOL_C = 4e-6           # c
TOL_DW = 2e-5          # dW_hh formed from a layer's dG

# backward step, shapes (B, H): the grid of batch x hidden sizes, and the 32-row tile at its edges
GRID_SHAPES = [(B, H) for B in (1, 4, 10, 16, 17, 33, 64) for H in (30, 32, 36, 512, 1000)]
WIDE_SHAPES = [(250, 480), (256, 472), (250, 472)]      # cdiv(H, 16) * cdiv(B, 32) >= 240: the 32-row tile
NARROW_SHAPES = [(224, 472)]                            # < 240: the 16-row tile
FORM_SHAPES = [(17, 36), (33, 30), (64, 512), (250, 480)]
FORMS = ["last_step", "step0", "below_dh_first", "nothing_flows"]
FWD_SHAPES = [(17, 36), (33, 30), (5, 1000)]
# layer loops (T, B, H, n_gx, dh_first); dh_first None: no gradient arrives at all
LAYER_CASES = [(1, 3, 32, 1, 0), (1, 3, 30, 0, 0), (5, 17, 36, 5, 0), (5, 17, 36, 0, 4), (4, 33, 30, 2, 1), (3, 64, 512, 3, 0),
               (5, 17, 36, 2, None)]
# more than 65535 rows through the fp32 train driver: (B, K, L, F, H, E, V), (L-1) * B * K = 72000
DRIVER_PLAIN = (9000, 1, 9, 8, 8, 8, 24)
DRIVER_GROUP = (1800, 5, 9, 8, 8, 8, 24)
LOSS_SCALE = 4096.0    # a power of two (exact): lifts dfeats of the mean over 72000 rows above the 1e-6 floor of its bound


def cdiv(a, b):
    return (a + b - 1) // b


def wide_tiles(B, H):
    """the count lstm_step_bwd2 compares with 240 to choose the 32-row tile"""
    return cdiv(H, 16) * cdiv(B, 32)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _uniform(*shape, seed, k):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * k


def _to(t, dtype):
    return None if t is None else t.detach().to(device="cpu", dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------- the formulas
def activate(pre, c_prev=None):
    """(activated gates [B, 4H] = sigmoid i, sigmoid f, tanh g, sigmoid o; c [B, H]; h [B, H]) from the pre-activations, in their dtype"""
    i, f, g, o = pre.chunk(4, 1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = i * g if c_prev is None else f * c_prev + i * g
    return torch.cat([i, f, g, o], 1), c, o * torch.tanh(c)


def cell_fwd(gx, w_hh, h_prev, c_prev, dtype=F64):
    """One forward step: gx [B, 4H] or [4H] (a bias, every row), h_prev / c_prev [B, H] or None.  Returns (h, c, stash)."""
    gx, w_hh, h_prev, c_prev = _to(gx, dtype), _to(w_hh, dtype), _to(h_prev, dtype), _to(c_prev, dtype)
    pre = gx if h_prev is None else gx + h_prev @ w_hh.t()
    stash, c, h = activate(pre, c_prev)
    return h, c, stash


def step_bwd(dg_next, w_hh, dh_out, stash, c, c_prev, dc_in, dtype=F64):
    """One BPTT step.  dg_next [B, 4H] (dG of step t + 1), w_hh [4H, H], dh_out [B, H], stash [B, 4H] (activated gates), c, c_prev,
    dc_in [B, H]; dg_next, dh_out, c_prev, dc_in may be None.  Returns (dg [B, 4H], dc_prev [B, H])."""
    dg_next, w_hh, dh_out, stash = _to(dg_next, dtype), _to(w_hh, dtype), _to(dh_out, dtype), _to(stash, dtype)
    c, c_prev, dc_in = _to(c, dtype), _to(c_prev, dtype), _to(dc_in, dtype)
    dh = torch.zeros_like(c)
    if dg_next is not None:
        dh = dh + dg_next @ w_hh
    if dh_out is not None:
        dh = dh + dh_out
    i, f, g, o = stash.chunk(4, 1)
    tc = torch.tanh(c)
    dc = dh * o * (1.0 - tc * tc)
    if dc_in is not None:
        dc = dc + dc_in
    cp = torch.zeros_like(c) if c_prev is None else c_prev
    dg = torch.cat([dc * g * i * (1.0 - i), dc * cp * f * (1.0 - f), dc * i * (1.0 - g * g), dh * tc * o * (1.0 - o)], 1)
    return dg, dc * f


def layer_fwd(T, B, gx, n_gx, bias, w_hh, dtype=F64):
    """ops.lstm_seq_fwd: a layer from the zero state, gx [n_gx*B, 4H] time-major, the bias alone from step n_gx on.
    Returns (h_all [T*B, H], c_all [T*B, H], stash [T*B, 4H])."""
    gx, bias, w_hh = _to(gx, dtype), _to(bias, dtype), _to(w_hh, dtype)
    h = c = None
    hs, cs, ss = [], [], []
    for t in range(T):
        g = gx[t * B:(t + 1) * B] if t < n_gx else bias.expand(B, -1)
        h, c, s = cell_fwd(g, w_hh, h, c, dtype)
        hs.append(h), cs.append(c), ss.append(s)
    return torch.cat(hs), torch.cat(cs), torch.cat(ss)


def layer_bwd(T, B, w_hh, dh_out, dh_first, c_all, stash, dtype=F64):
    """ops.lstm_seq_bwd: BPTT over the layer; dh_out [(T - dh_first)*B, H] is the gradient into h_t for t >= dh_first, or None.
    Returns dG [T*B, 4H]."""
    dgs = [None] * T
    dc = None
    for t in range(T - 1, -1, -1):
        rows = slice(t * B, (t + 1) * B)
        dho = dh_out[(t - dh_first) * B:(t - dh_first + 1) * B] if dh_out is not None and t >= dh_first else None
        dgs[t], dc = step_bwd(dgs[t + 1] if t < T - 1 else None, w_hh, dho, stash[rows], c_all[rows],
                              c_all[(t - 1) * B:t * B] if t else None, dc, dtype)
    return torch.cat(dgs)


def dw_from_dg(T, B, dg, h_all):
    """dW_hh [4H, H] = sum over t >= 1 of dG_t^T h_{t-1}, in fp64"""
    dg, h_all = _to(dg, F64), _to(h_all, F64)
    return dg[B:].t() @ h_all[:(T - 1) * B]


# ----------------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def step_inputs(B, H, zero_state=False, seed_shift=0):
    """fp32 inputs of one backward step (never modified): w_hh, gx, c_prev, dh_out, dc, dg_next and the forward's stash and c.
    zero_state: the step is step 0 of a layer (c = i . g, c_prev None)."""
    s = seed_shift
    d = dict(w_hh=_uniform(4 * H, H, seed=1 + s, k=1.0 / H ** 0.5), gx=_randn(B, 4 * H, seed=2 + s),
             c_prev=None if zero_state else _randn(B, H, seed=4 + s), dh_out=_randn(B, H, seed=5 + s), dc=_randn(B, H, seed=6 + s),
             dg_next=_randn(B, 4 * H, seed=7 + s, scale=0.1))
    d["stash"], d["c"], _ = activate(d["gx"], d["c_prev"])
    return d


def form_args(B, H, form):
    """(dg_next, w_hh, dh_out, stash, c, c_prev, dc_in) of step_bwd for one of the forms the BPTT loop issues (None = null pointer):
      all             every input present
      last_step       step T - 1: no dg_next, dc_is_zero
      step0           step 0: no c_prev (c = i . g)
      below_dh_first  a step under dh_first: no dh_out
      nothing_flows   no dg_next, no dh_out, dc all zeros (dc_is_zero off)"""
    d = step_inputs(B, H, zero_state=(form == "step0"))
    a = dict(dg_next=d["dg_next"], w_hh=d["w_hh"], dh_out=d["dh_out"], stash=d["stash"], c=d["c"], c_prev=d["c_prev"], dc_in=d["dc"])
    if form == "last_step":
        a.update(dg_next=None, dc_in=None)
    elif form == "below_dh_first":
        a.update(dh_out=None)
    elif form == "nothing_flows":
        a.update(dg_next=None, dh_out=None, dc_in=torch.zeros(B, H))
    elif form not in ("all", "step0"):
        raise ValueError(form)
    return a


@functools.lru_cache(maxsize=None)
def fwd_inputs(B, H):
    """fp32 inputs of a forward step without gx, as the decode half of a layer runs it: bias, w_hh, h_prev, c_prev"""
    k = 1.0 / H ** 0.5
    return dict(bias=_uniform(4 * H, seed=21, k=k), w_hh=_uniform(4 * H, H, seed=1, k=k), h_prev=_randn(B, H, seed=3, scale=0.5),
                c_prev=_randn(B, H, seed=4))


@functools.lru_cache(maxsize=None)
def layer_inputs(T, B, H, n_gx, dh_first):
    """fp32 inputs of a layer and its BPTT (the scales of test_lstm_seq_fwd_bwd_vs_autograd): w_hh, bias, gx, dh_out"""
    k = 1.0 / H ** 0.5
    return dict(w_hh=_uniform(4 * H, H, seed=31, k=k), bias=_uniform(4 * H, seed=32, k=k),
                gx=_randn(n_gx * B, 4 * H, seed=33) if n_gx else None,
                dh_out=None if dh_first is None else _randn((T - dh_first) * B, H, seed=34))


@functools.lru_cache(maxsize=None)
def layer_ref(T, B, H, n_gx, dh_first):
    """the fp64 layer of layer_inputs: dict of h_all, c_all, stash, dg, dw"""
    d = layer_inputs(T, B, H, n_gx, dh_first)
    h_all, c_all, stash = layer_fwd(T, B, d["gx"], n_gx, d["bias"], d["w_hh"])
    dg = layer_bwd(T, B, d["w_hh"], d["dh_out"], dh_first or 0, c_all, stash)
    return dict(h_all=h_all, c_all=c_all, stash=stash, dg=dg, dw=dw_from_dg(T, B, dg, h_all))


# ------------------------------------------------------------------------------------------- the train driver above 65535 rows
@functools.lru_cache(maxsize=None)
def driver_data(shape):
    """(state dict, feats [B, L, F], caps [B, K, L], mask [B, K, L]) on the host, never modified.  B * K = 9000 for both shapes:
    the same captions, the grouped shape's clips are the first 1800 feature rows."""
    from s2vt_video_caption_amd import synth
    B, K, L, Fd, H, E, V = shape
    sd = synth.make_state_dict(V, Fd, H, E, seed=97)
    feats, caps, mask = synth.make_batch(B * K, L, Fd, V, seed=97, min_words=1)
    return sd, feats[:B].contiguous(), caps.view(B, K, L), mask.view(B, K, L)


def driver_oracle(shape, dtype=F64):
    """The oracle in `dtype` on the clips repeated K times, backward on loss * LOSS_SCALE: (logits [B*K, L-1, V], loss (unscaled),
    {name: grad}, dfeats summed over each clip's K rows [B, L, F])"""
    from oracle import s2vt_oracle as orc
    B, K, L, Fd, H, E, V = shape
    sd, feats, caps, mask = driver_data(shape)
    om = orc.OracleModel(sd, dtype=dtype)
    fo = feats.repeat_interleave(K, 0).to(dtype).requires_grad_()
    logits = om(fo, caps.reshape(B * K, L)[:, :-1])
    loss = orc.mask_criterion(logits, caps.reshape(B * K, L), mask.reshape(B * K, L))
    (loss * LOSS_SCALE).backward()
    grads = {k: q.grad.clone() for k, q in om.as_dict().items()}
    return logits.detach(), float(loss.detach()), grads, fo.grad.view(B, K, L, Fd).sum(1)


@functools.lru_cache(maxsize=None)
def driver_ref(shape):
    return driver_oracle(shape, F64)


def driver_errors(got, ref):
    """[(name, error, bound)] of a (logits, loss, grads, dfeats) tuple against a reference one, with the project's whole-path bounds
    (test_gpu_train_group._assert_close): logits < 2e-5, loss < 1e-5, every gradient and dfeats within 1e-6 + 1e-4 * max|ref|"""
    (gl, gloss, gg, gdf), (rl, rloss, rg, rdf) = got, ref
    rl = _to(rl, F64)
    out = [("logits", (_to(gl, F64).reshape(rl.shape) - rl).abs().max().item(), 2e-5), ("loss", abs(gloss - rloss), 1e-5)]
    assert sorted(gg) == sorted(rg) and len(rg) == 13
    for n, r in rg.items():
        r = _to(r, F64)
        out.append((n, (_to(gg[n], F64) - r).abs().max().item(), 1e-6 + 1e-4 * r.abs().max().item()))
    rdf = _to(rdf, F64)
    out.append(("dfeats", (_to(gdf, F64) - rdf).abs().max().item(), 1e-6 + 1e-4 * rdf.abs().max().item()))
    return out
