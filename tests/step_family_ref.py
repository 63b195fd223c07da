"""Plain fp64 restatements on the CPU of the two kernel families that share csrc/step_frame.h with the LSTM step kernels - the GRU
step kernels (csrc/gru.hip: gru_step_fwd / gru_step_bwd, GruFwdArgs / GruBwdArgs) and the layer-wavefront chain kernels
(csrc/lstm_stack.hip through s2vt_lstm_chain_fwd / _bwd of csrc/api_stack.hip, s2vt_lstm_layer) - with every optional input
nullable as it is there (None = the null pointer), the case lists of tests/test_gpu_step_family_edges.py and their seeded inputs.

  gru_cell_fwd   one nn.GRU step from the gate input (gx [B, 3H], or b_ih [3H] for every row), the state (None = zero) and an
                 optional token segment (the embedded rows [B, E] and W_e [3H, E]): (h, r, z, n, ghn).
  gru_step_bwd   one BPTT step from the stash (r, z, n, ghn): dh = dh_out? + (dh_in . z_next + dgh_next . W_hh)?, then
                 dgx = [dr, dz, dn], dgh = [dr, dz, dn . r].  dh_in is not read without dgh_next (the kernel's in/out dh buffer).
  chain_fwd      a chain of layers over T steps: per layer (h, c, stash, hm); gx on the steps [gx_t0, gx_t0 + n_gx), h0 / c0,
                 x_in on layer 0, masks, the token segment at T = 1.
  chain_bwd      its BPTT: per layer dG; dh_ext / dh_t0 on any layer, the mask on the gradient arriving from the layer above.

`dtype` is the precision the formulas are evaluated in: float64 (the reference) or float32 (the room the bounds leave).
tests/test_step_family_ref_host.py holds all of this to torch's fp64 cells and autograd.  The LSTM cell and its derivative are
those of tests/lstm_step_ref.py.

Bounds, relative to max|reference| as the project's tests state them: the GRU kernels 1e-5 (test_gpu_gru._close), the chain
forward 1e-5 and the chain dG 2e-5 (test_gpu_stack._close and its rel=2e-5 for dG)."""
import functools

import torch

import lstm_step_ref as L
from lstm_step_ref import F64, _randn, _to, _uniform, cdiv  # noqa: F401

REL_GRU = 1e-5         # test_gpu_gru._close
REL_CHAIN = 1e-5       # test_gpu_stack._close
REL_CHAIN_DG = 2e-5    # test_gpu_stack._close(..., rel=2e-5), dG of test_chain_kernels_against_fp64

# ------------------------------------------------------------------------------------------------------------------ the cases
# chain forward, then backward on its own outputs: T = 3, n = 3 (chain_case)
CHAIN_SHAPES = [(70, 40), (130, 72), (17, 8), (3, 4), (3, 5)]
CHAIN_MISALIGNED = (40, 40)                      # B > 16, H % 4 == 0: the 32-row tile unless an operand is misaligned
MISALIGNED_OPERANDS = ["w_hh", "w_in"]
CHAIN_TOKEN = [(40, 40, 36), (40, 40, 26), (70, 40, 36), (3, 4, 4)]          # (B, H, E): T = 1, n = 2
CHAIN_BWD_SHAPES = [(70, 40), (17, 8)]
CHAIN_BWD_FORMS = ["t1", "nothing_flows", "ext_layer0", "no_mask", "one_layer"]
GRU_SHAPES = [(3, 4), (3, 5), (17, 8), (70, 40), (130, 136)]
GRU_MISALIGNED = (70, 40)
GRU_BWD_SHAPES = [(17, 8), (70, 40)]
GRU_BWD_FORMS = ["last_nan_dh", "no_h_prev", "no_dh_out", "last_no_dh_out"]
GRU_TOKEN = [(70, 40, 36), (70, 40, 26)]                                      # (B, H, E)
GRU_TOKEN_ZERO_STATE = (17, 8, 4)
GEMV_LDS_CASE = (5, 2564, 2560)                  # (B, H, E): 8 * (2564 + 2560) * 4 = 163968 bytes of staged rows
TOL_GEMV = 4e-6                                  # test_small_batch_gemv_step_against_fp64_and_the_tile_kernel


# ---- the tile and instantiation arithmetic of the launchers, restated (the host test holds it to the sources' text)
def chain_vec(H, E=None, misaligned=False):
    """lstm_chain_fwd_launch: the 16-byte-load kernels need H % 4 == 0 (E % 4 == 0 with a token segment) and aligned operands"""
    return H % 4 == 0 and (E is None or E % 4 == 0) and not misaligned


def chain_fwd_rows(B, vec):
    """rows of a forward chain tile: `if (a.B <= 16 || !vec)` the 16-row tile, else the 32-row one"""
    return 16 if (B <= 16 or not vec) else 32


CHAIN_FWD_UNITS = 8    # hidden units (columns of every gate) of a forward chain tile
CHAIN_BWD_TILE = 16    # rows and columns of a backward chain tile
GRU_TILE = 16          # rows and hidden units of a GRU tile, forward and backward


def xcd_grid(nx, ny):
    return cdiv(nx, 8) * 8 * ny


def bound(ref, rel):
    return rel * max(ref.abs().max().item(), 1e-30)


def err(got, ref):
    return (got.detach().cpu().double() - ref.double()).abs().max().item()


def edge_moves(ref, B, H, rows, cols):
    """How far `ref` [T*B, G*H] (G gate blocks of H columns, T steps of B rows) moves when the last row block / the last column
    block of a rows x cols tiling is zeroed: (rows moved by, columns moved by)."""
    v = ref.double().reshape(-1, B, ref.shape[1] // H, H)
    r0, u0 = (B - 1) // rows * rows, (H - 1) // cols * cols
    cut_r, cut_c = v.clone(), v.clone()
    cut_r[:, r0:] = 0
    cut_c[..., u0:] = 0
    return (cut_r - v).abs().max().item(), (cut_c - v).abs().max().item()


# ------------------------------------------------------------------------------------------------------------- the GRU formulas
def gru_cell_fwd(gx, w_hh, b_hh, h_prev=None, tok_rows=None, B=None, dtype=F64):
    """gx [B, 3H] or [3H] (b_ih alone: a zero input, `B` rows unless the state gives them); h_prev [B, H] or None; tok_rows
    (x [B, E], W_e [3H, E]) or None.  Returns (h, r, z, n, ghn) with ghn = h_prev W_hn^T + b_hn."""
    gx, w_hh, b_hh, h_prev = _to(gx, dtype), _to(w_hh, dtype), _to(b_hh, dtype), _to(h_prev, dtype)
    H = w_hh.shape[1]
    if gx.dim() == 1:
        gx = gx.expand(h_prev.shape[0] if h_prev is not None else (tok_rows[0].shape[0] if tok_rows is not None else B), -1)
    if tok_rows is not None:
        gx = gx + _to(tok_rows[0], dtype) @ _to(tok_rows[1], dtype).t()
    gh = b_hh.expand(gx.shape[0], -1) if h_prev is None else h_prev @ w_hh.t() + b_hh
    r = torch.sigmoid(gx[:, :H] + gh[:, :H])
    z = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
    ghn = gh[:, 2 * H:]
    n = torch.tanh(gx[:, 2 * H:] + r * ghn)
    h = n + z * ((0.0 if h_prev is None else h_prev) - n)
    return h, r, z, n, ghn


def gru_step_bwd(dgh_next, w_hh, stash_next, dh_out, stash, h_prev, dh_in, dtype=F64):
    """dgh_next [B, 3H] (dgh of step t + 1), w_hh [3H, H], stash_next / stash [B, 4H] = (r, z, n, ghn), dh_out, h_prev, dh_in
    (dh of step t + 1) [B, H]; dgh_next (with stash_next and dh_in), dh_out and h_prev may be None.  Returns (dgx, dgh, dh)."""
    dgh_next, w_hh, stash_next, dh_out = _to(dgh_next, dtype), _to(w_hh, dtype), _to(stash_next, dtype), _to(dh_out, dtype)
    stash, h_prev, dh_in = _to(stash, dtype), _to(h_prev, dtype), _to(dh_in, dtype)
    r, z, n, ghn = stash.chunk(4, 1)
    dh = torch.zeros_like(r)
    if dgh_next is not None:
        dh = dh + dgh_next @ w_hh + dh_in * stash_next.chunk(4, 1)[1]
    if dh_out is not None:
        dh = dh + dh_out
    hp = torch.zeros_like(r) if h_prev is None else h_prev
    dn = dh * (1.0 - z)
    dz = dh * (hp - n)
    dnp = dn * (1.0 - n * n)
    drp = dnp * ghn * r * (1.0 - r)
    dzp = dz * z * (1.0 - z)
    return torch.cat([drp, dzp, dnp], 1), torch.cat([drp, dzp, dnp * r], 1), dh


# ----------------------------------------------------------------------------------------------------------- the chain formulas
def token_ids(B, tok_packed=None, tok_const=0):
    """token_of (csrc/philox.h): the low word of a packed argmax word holds 0xFFFFFFFF - id; else one constant token"""
    if tok_packed is not None:
        return 0xFFFFFFFF - (tok_packed.cpu().long() & 0xFFFFFFFF)
    return torch.full((B,), int(tok_const), dtype=torch.long)


def chain_fwd(T, B, H, layers, dtype=F64):
    """layers: dicts of w_hh [4H, H], bias [4H] and optionally gx [n_gx*B, 4H] with gx_t0 / n_gx, h0, c0 [B, H], w_in [4H, H]
    (layers above the first, and layer 0 with x_in [T*B, H]), mask [T*B, H], and at T = 1 emb [V, E], w_e [4H, E], tok_ids [B].
    Returns per layer (h [T*B, H], c [T*B, H], stash [T*B, 4H], hm = mask . h or None)."""
    outs = []
    for j, l in enumerate(layers):
        w_hh, bias, w_in = _to(l["w_hh"], dtype), _to(l["bias"], dtype), _to(l.get("w_in"), dtype)
        gx, t0, ng = _to(l.get("gx"), dtype), l.get("gx_t0", 0), l.get("n_gx", 0)
        mask = _to(l.get("mask"), dtype)
        if j > 0:
            x_all = outs[j - 1][3] if outs[j - 1][3] is not None else outs[j - 1][0]
        else:
            x_all = _to(l.get("x_in"), dtype)
        h, c = _to(l.get("h0"), dtype), _to(l.get("c0"), dtype)
        hs, cs, ss = [], [], []
        for t in range(T):
            pre = gx[(t - t0) * B:(t - t0 + 1) * B] if t0 <= t < t0 + ng else bias.expand(B, -1)
            if x_all is not None:
                pre = pre + x_all[t * B:(t + 1) * B] @ w_in.t()
            if l.get("emb") is not None:
                assert T == 1
                pre = pre + _to(l["emb"], dtype)[l["tok_ids"]] @ _to(l["w_e"], dtype).t()
            h, c, s = L.cell_fwd(pre, w_hh, h, c, dtype)
            hs.append(h), cs.append(c), ss.append(s)
        h_all = torch.cat(hs)
        outs.append((h_all, torch.cat(cs), torch.cat(ss), None if mask is None else mask * h_all))
    return outs


def chain_bwd(T, B, H, layers, fwd, dtype=F64):
    """BPTT of chain_fwd from its outputs `fwd`: layer j's dh at step t = dh_ext_j[t - dh_t0_j] (t >= dh_t0_j) + dG_j[t+1] . W_hh_j
    + mask_j[t] . (dG_{j+1}[t] . W_in_{j+1}).  Returns per layer dG [T*B, 4H]."""
    n = len(layers)
    dgs = [None] * n
    for j in range(n - 1, -1, -1):
        l = layers[j]
        _, c_all, stash, _ = fwd[j]
        ext, e0, mask = _to(l.get("dh_ext"), dtype), l.get("dh_t0", 0), _to(l.get("mask"), dtype)
        dg, dc = [None] * T, None
        for t in range(T - 1, -1, -1):
            rows = slice(t * B, (t + 1) * B)
            dh = ext[(t - e0) * B:(t - e0 + 1) * B] if ext is not None and t >= e0 else None
            if j < n - 1:
                up = dgs[j + 1][rows] @ _to(layers[j + 1]["w_in"], dtype)
                up = up if mask is None else up * mask[rows]
                dh = up if dh is None else dh + up
            dg[t], dc = L.step_bwd(dg[t + 1] if t < T - 1 else None, l["w_hh"], dh, stash[rows], c_all[rows],
                                   c_all[(t - 1) * B:t * B] if t else l.get("c0"), dc, dtype)
        dgs[j] = torch.cat(dg)
    return dgs


# ------------------------------------------------------------------------------------------------------------------- the inputs
def _keep_mask(rows, H, seed, p=0.3):
    return (torch.rand(rows, H, generator=torch.Generator().manual_seed(seed)) > p).float() / (1.0 - p)


@functools.lru_cache(maxsize=None)
def chain_case(B, H, form="main"):
    """fp32 inputs (never modified) of a chain and its backward: dict(T, layers).
      main           T = 3, n = 3: layer 0 with gx on step 1 alone, a state and x_in (forward only); layer 1 from the zero state under
                     a mask; layer 2 bias-only from a state; dh_ext into the top layer from step 1 on
      t1             the same at T = 1
      nothing_flows  dh_t0 == T on every layer (dh_ext NaN: never read)
      ext_layer0     dh_ext on layer 0 (every step) as well as on the top layer
      no_mask        no mask anywhere
      one_layer      n = 1"""
    T = 1 if form == "t1" else 3
    n = 1 if form == "one_layer" else 3
    k = H ** -0.5
    t0 = 1 if T > 1 else 0
    layers = []
    for j in range(n):
        s = 1000 * (j + 1)
        l = dict(w_hh=_uniform(4 * H, H, seed=s + 1, k=k), bias=_uniform(4 * H, seed=s + 2, k=k), w_in=_uniform(4 * H, H, seed=s + 3, k=k))
        if j != 1:
            l.update(h0=_randn(B, H, seed=s + 4, scale=0.5), c0=_randn(B, H, seed=s + 5))
        if j == 0:
            l.update(gx=_randn(B, 4 * H, seed=s + 6), gx_t0=t0, n_gx=1, x_in=_randn(T * B, H, seed=s + 7))
        if j == 1 and form != "no_mask":
            l["mask"] = _keep_mask(T * B, H, s + 8)
        layers.append(l)
    if form == "nothing_flows":
        for l in layers:
            l.update(dh_ext=torch.full((B, H), float("nan")), dh_t0=T)
    else:
        layers[-1].update(dh_ext=_randn((T - t0) * B, H, seed=77), dh_t0=t0)
        if form == "ext_layer0":
            layers[0].update(dh_ext=_randn(T * B, H, seed=78), dh_t0=0)
    return dict(T=T, layers=layers)


@functools.lru_cache(maxsize=None)
def chain_ref(B, H, form="main", dtype=F64):
    """(forward outputs, dG) per layer of chain_case in `dtype`"""
    c = chain_case(B, H, form)
    fwd = chain_fwd(c["T"], B, H, c["layers"], dtype)
    return fwd, chain_bwd(c["T"], B, H, c["layers"], fwd, dtype)


@functools.lru_cache(maxsize=None)
def token_case(B, H, E):
    """One decode step of a two-layer word chain (T = 1): x_in and the token segment as column blocks of one [4H, E + H] weight
    (w0: its first E columns multiply the embedded word), a constant token and packed argmax words."""
    V, k = 23, H ** -0.5
    g = torch.Generator().manual_seed(B * 100 + E)
    toks = torch.randint(0, V, (B,), generator=g)
    packed = (0xFFFFFFFF - toks) | (torch.randint(0, 2 ** 30, (B,), generator=g) << 32)
    layers = [dict(w_hh=_uniform(4 * H, H, seed=11, k=k), bias=_uniform(4 * H, seed=12, k=k), h0=_randn(B, H, seed=13, scale=0.5),
                   c0=_randn(B, H, seed=14), x_in=_randn(B, H, seed=15), w0=_uniform(4 * H, E + H, seed=16, k=k), emb=_randn(V, E, seed=17)),
              dict(w_hh=_uniform(4 * H, H, seed=21, k=k), bias=_uniform(4 * H, seed=22, k=k), h0=_randn(B, H, seed=23, scale=0.5),
                   c0=_randn(B, H, seed=24), w_in=_uniform(4 * H, H, seed=25, k=k))]
    return dict(V=V, E=E, tok_const=5, toks=toks, packed=packed, layers=layers)


def token_layers(B, H, E, source):
    """the layers of token_case for chain_fwd; source 'const' or 'packed'"""
    c = token_case(B, H, E)
    l0 = dict(c["layers"][0])
    w0 = l0.pop("w0")
    ids = token_ids(B, c["packed"]) if source == "packed" else token_ids(B, None, c["tok_const"])
    if source == "packed":
        assert torch.equal(ids, c["toks"])
    l0.update(w_in=w0[:, E:], w_e=w0[:, :E], tok_ids=ids)
    return [l0, c["layers"][1]]


@functools.lru_cache(maxsize=None)
def token_ref(B, H, E, source, dtype=F64):
    return chain_fwd(1, B, H, token_layers(B, H, E, source), dtype)


@functools.lru_cache(maxsize=None)
def gru_inputs(B, H, E=0):
    """fp32 inputs (never modified) of the GRU steps: the weights, gx / h_prev of step t, gx_next of step t + 1, dh_out, the dh and
    dgh arriving from step t + 1, the token segment, and the stashes the backward reads: the fp64 forward's, rounded to fp32
    (stash / h of step t from h_prev, stash_zero from the zero state, stash_next of step t + 1 from h)."""
    k = H ** -0.5
    d = dict(w_hh=_uniform(3 * H, H, seed=1, k=k), b_hh=_uniform(3 * H, seed=2, k=k), b_ih=_uniform(3 * H, seed=3, k=k),
             gx=_randn(B, 3 * H, seed=4), h_prev=_randn(B, H, seed=5).tanh(), gx_next=_randn(B, 3 * H, seed=6), dh_out=_randn(B, H, seed=7),
             dh_in=_randn(B, H, seed=8), dgh_next=_randn(B, 3 * H, seed=9, scale=0.1))
    if E:
        V = 29
        g = torch.Generator().manual_seed(B * 100 + E)
        tok = torch.randint(0, V, (B,), generator=g)
        d.update(V=V, w_ih=_uniform(3 * H, E + H, seed=10, k=k), emb=_randn(V, E, seed=11), tok=tok,
                 packed=(0xFFFFFFFF - tok) | (torch.randint(0, 2 ** 30, (B,), generator=g) << 32))
    out = gru_cell_fwd(d["gx"], d["w_hh"], d["b_hh"], d["h_prev"])
    d["h"], d["stash"] = out[0].float(), torch.cat(out[1:], 1).float()
    d["stash_zero"] = torch.cat(gru_cell_fwd(d["gx"], d["w_hh"], d["b_hh"], None)[1:], 1).float()
    d["stash_next"] = torch.cat(gru_cell_fwd(d["gx_next"], d["w_hh"], d["b_hh"], d["h"])[1:], 1).float()
    return d


def gru_bwd_args(B, H, form="all"):
    """the arguments of gru_step_bwd for a form the BPTT loop issues (None = null pointer):
      all             a step with a successor, every input present
      last_nan_dh     the last step: no dgh_next / stash_next, the dh buffer not read (the device test fills it with NaN)
      no_h_prev       step 0: the zero state
      no_dh_out       a step under dh_first
      last_no_dh_out  the last step under dh_first: nothing flows, every output exactly 0"""
    d = gru_inputs(B, H)
    a = dict(dgh_next=d["dgh_next"], w_hh=d["w_hh"], stash_next=d["stash_next"], dh_out=d["dh_out"], stash=d["stash"],
             h_prev=d["h_prev"], dh_in=d["dh_in"])
    if form in ("last_nan_dh", "last_no_dh_out"):
        a.update(dgh_next=None, stash_next=None, dh_in=None)
    if form in ("no_dh_out", "last_no_dh_out"):
        a.update(dh_out=None)
    if form == "no_h_prev":
        a.update(h_prev=None, stash=d["stash_zero"])
    if form not in ("all", "last_nan_dh", "no_h_prev", "no_dh_out", "last_no_dh_out"):
        raise ValueError(form)
    return a


@functools.lru_cache(maxsize=None)
def gru_bwd_ref(B, H, form="all", dtype=F64):
    a = gru_bwd_args(B, H, form)
    return gru_step_bwd(a["dgh_next"], a["w_hh"], a["stash_next"], a["dh_out"], a["stash"], a["h_prev"], a["dh_in"], dtype)


def gru_fwd_forms(B, H, E=0):
    """{name: arguments of gru_cell_fwd} of the forward forms: the zero state with b_ih alone, a step from a state, and with E the
    token segment from a state (the tokens of the int32 array = those of the packed words) and from the zero state"""
    d = gru_inputs(B, H, E)
    forms = dict(zero_state=dict(gx=d["b_ih"], w_hh=d["w_hh"], b_hh=d["b_hh"], h_prev=None, tok_rows=None, B=B),
                 state=dict(gx=d["gx"], w_hh=d["w_hh"], b_hh=d["b_hh"], h_prev=d["h_prev"], tok_rows=None))
    if E:
        rows = (d["emb"][d["tok"]], d["w_ih"][:, :E])
        forms = dict(token=dict(gx=d["gx"], w_hh=d["w_hh"], b_hh=d["b_hh"], h_prev=d["h_prev"], tok_rows=rows),
                     token_zero_state=dict(gx=d["gx"], w_hh=d["w_hh"], b_hh=d["b_hh"], h_prev=None, tok_rows=rows))
    return forms


@functools.lru_cache(maxsize=None)
def gru_fwd_ref(B, H, E, form, dtype=F64):
    """(h [B, H], stash [B, 4H]) of a forward form"""
    out = gru_cell_fwd(dtype=dtype, **gru_fwd_forms(B, H, E)[form])
    return out[0], torch.cat(out[1:], 1)


@functools.lru_cache(maxsize=None)
def gemv_lds_inputs():
    """fp32 inputs of the LSTM token step of GEMV_LDS_CASE and its fp64 (h, c)"""
    B, H, E = GEMV_LDS_CASE
    V = 11
    d = dict(gx=_randn(B, 4 * H, seed=1), w_hh=_randn(4 * H, H, seed=2, scale=H ** -0.5), h_prev=_randn(B, H, seed=5, scale=0.5),
             c_prev=_randn(B, H, seed=6, scale=0.5), emb=_randn(V, E, seed=4), w_ih=_randn(4 * H, E + H, seed=3, scale=(E + H) ** -0.5),
             tok=torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(7), dtype=torch.int32))
    pre = d["gx"].double() + d["emb"].double()[d["tok"].long()] @ d["w_ih"].double()[:, :E].t()
    h, c, _ = L.cell_fwd(pre, d["w_hh"], d["h_prev"], d["c_prev"])
    return d, h, c
