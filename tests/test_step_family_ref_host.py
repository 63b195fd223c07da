"""Host: the fp64 restatements of tests/step_family_ref.py against torch's fp64 nn.GRUCell / nn.LSTMCell and autograd, and for
every case of tests/test_gpu_step_family_edges.py the three things its bound needs besides a right reference:
  room    the same formulas in plain fp32 on the host stay under half the bound (the kernels sum in another order: another draw of
          the same size, see test_lstm_step_ref_host.py);
  sight   zeroing the last row block or the last column block of any output, at the tile size the kernel uses for the case, moves
          it by at least 10 bounds - the bounds are relative to max|reference| and must not hide a small-magnitude edge;
  place   the tile counts and the instantiation rule the case lists rely on, restated in step_family_ref and held to the text of
          csrc/lstm_stack.hip and csrc/gru.hip, so that a changed threshold fails here instead of moving what the GPU cases cover.
None of this needs a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_family_ref as R  # noqa: E402

F64 = torch.float64
F32 = torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda c: "-".join(str(x) for x in c)  # noqa: E731

CHAIN_CASES = [(B, H, "main") for B, H in R.CHAIN_SHAPES + [R.CHAIN_MISALIGNED]] + \
              [(B, H, f) for B, H in R.CHAIN_BWD_SHAPES for f in R.CHAIN_BWD_FORMS]
TOKEN_CASES = [(B, H, E, s) for B, H, E in R.CHAIN_TOKEN for s in ("const", "packed")]
GRU_FWD_CASES = [(B, H, 0, f) for B, H in R.GRU_SHAPES for f in ("zero_state", "state")] + \
                [(B, H, E, "token") for B, H, E in R.GRU_TOKEN] + [R.GRU_TOKEN_ZERO_STATE + ("token_zero_state",)]
GRU_BWD_CASES = [(B, H, "all") for B, H in R.GRU_SHAPES] + [(B, H, f) for B, H in R.GRU_BWD_SHAPES for f in R.GRU_BWD_FORMS]


def _d(t):
    return None if t is None else t.double()


def _torch_cell(cls, gi, w_hh, b_hh, state):
    """torch's fp64 nn.GRUCell / nn.LSTMCell on the gate input gi: input weight = identity, input bias = 0"""
    G, H = gi.shape[1], w_hh.shape[1]
    cell = cls(G, H).double()
    zero = torch.zeros(G, dtype=F64)
    return torch.func.functional_call(cell, {"weight_ih": torch.eye(G, dtype=F64), "weight_hh": w_hh, "bias_ih": zero,
                                             "bias_hh": zero if b_hh is None else b_hh}, (gi, state))


def _room(what, got32, ref, rel):
    e, b = R.err(got32, ref), R.bound(ref, rel)
    print(what, "fp32 error / bound %.3g" % (e / b))
    assert e < b / 2, (what, e, b)


def _sight(what, ref, B, H, rows, cols, rel):
    b = R.bound(ref, rel)
    mr, mc = R.edge_moves(ref, B, H, rows, cols)
    print(what, "last row block moves %.3g bounds, last column block %.3g" % (mr / b, mc / b))
    assert mr >= 10 * b and mc >= 10 * b, (what, mr, mc, b)


# ---------------------------------------------------------------------------------------------------------------------- place
def test_the_tiles_and_instantiations_the_case_lists_rely_on():
    cd, tile = R.cdiv, R.chain_fwd_rows
    # (70, 40): 32-row tile, third row block of 6 rows, five column tiles; backward 16 x 16, last column tile 8, last row block 6
    assert tile(70, R.chain_vec(40)) == 32 and cd(70, 32) == 3 and 70 - 64 == 6 and cd(40, R.CHAIN_FWD_UNITS) == 5
    assert cd(40, R.CHAIN_BWD_TILE) == 3 and 40 % 16 == 8 and cd(70, 16) == 5 and 70 % 16 == 6
    # (130, 72): nine column tiles - a second group of eight ids per row block, seven of them idle
    assert cd(72, R.CHAIN_FWD_UNITS) == 9 and R.xcd_grid(9, cd(130, 32)) == 16 * 5 and 16 - 9 == 7
    # a tile wider than the matrix, K below one 32-float chunk; the scalar kernels
    assert tile(17, R.chain_vec(8)) == 32 and tile(3, R.chain_vec(4)) == 16 and not R.chain_vec(5) and tile(3, False) == 16
    B, H = R.CHAIN_MISALIGNED
    assert B > 16 and H % 4 == 0 and tile(B, R.chain_vec(H)) == 32 and tile(B, R.chain_vec(H, misaligned=True)) == 16
    # the token segment: 32-row vector tile with a ragged second row block, ldw_e = 76; scalar; all three segments ragged
    assert [tile(B, R.chain_vec(H, E)) for B, H, E in R.CHAIN_TOKEN] == [32, 16, 32, 16]
    assert 40 % 32 == 8 and 36 + 40 == 76 and 76 % 4 == 0 and 36 * 4 % 16 == 0 and not R.chain_vec(40, 26)
    # GRU: (130, 136) nine column tiles of 16 units, the last 8 wide, the last row block 2 rows; H = 4 one partial K chunk
    assert R.cdiv(136, R.GRU_TILE) == 9 and 136 % 16 == 8 and 130 % 16 == 2 and 3 * 5 % 4 != 0
    B, H, E = R.GEMV_LDS_CASE
    assert B <= 8 and H % 4 == 0 and E % 4 == 0 and max(H, E) <= 4096 and 8 * (H + E) * 4 == 163968 > 160 * 1024


def test_the_restated_launch_rules_are_the_sources():
    src = lambda name: open(os.path.join(ROOT, "s2vt-video-caption_amd", "csrc", name)).read()  # noqa: E731
    stack, gru, tile = src("lstm_stack.hip"), src("gru.hip"), src("mfma_tile.h")
    for text in ("bool vec = a.H % 4 == 0;", "if (a.B <= 16 || !vec) {", "p.tiles = xcd_grid(cdiv(a.H, 8), cdiv(a.B, 16));",
                 "p.tiles = xcd_grid(cdiv(a.H, 8), cdiv(a.B, 32));", "p.tiles = xcd_grid(cdiv(a.H, 16), cdiv(a.B, 16));",
                 "(!s.emb || (s.E % 4 == 0 && vec_ok(s.emb, s.E) && vec_ok(s.w_e, s.ldw_e)))"):
        assert text in stack, text
    for text in ("constexpr int GRU_TM = 16;", "constexpr int GRU_UN = 16;", "xcd_grid(cdiv(a.H, GRU_UN), cdiv(a.B, GRU_TM))",
                 "xcd_grid(cdiv(a.H, 16), cdiv(a.B, GRU_TM))", "a.K2 % 4 == 0", "vec_ok(a.dgh_next, a.lddgh) && vec_ok(a.w_hh_t, a.ldwt)"):
        assert text in gru, text
    for text in ("#define S2VT_KC 32", "(ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(ptr) & 15) == 0)",
                 "static inline int xcd_grid(int NX, int NY) { return ((NX + 7) / 8) * 8 * NY; }"):
        assert text in tile, text


# ------------------------------------------------------------------------------------------------------------------------ GRU
@pytest.mark.parametrize("case", GRU_FWD_CASES, ids=_ids)
def test_gru_forward_reference_room_and_sight(case):
    B, H, E, form = case
    a = R.gru_fwd_forms(B, H, E)[form]
    h, stash = R.gru_fwd_ref(*case)
    gi = _d(a["gx"]).expand(B, -1)
    if a["tok_rows"] is not None:
        gi = gi + _d(a["tok_rows"][0]) @ _d(a["tok_rows"][1]).t()
    hp = torch.zeros(B, H, dtype=F64) if a["h_prev"] is None else _d(a["h_prev"])
    assert (h - _torch_cell(torch.nn.GRUCell, gi, _d(a["w_hh"]), _d(a["b_hh"]), hp)).abs().max().item() < 1e-12
    gh = hp @ _d(a["w_hh"]).t() + _d(a["b_hh"])
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    want = torch.cat([r, torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H]), torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:]), gh[:, 2 * H:]], 1)
    assert (stash - want).abs().max().item() < 1e-12
    h32, stash32 = R.gru_fwd_ref(B, H, E, form, F32)
    for name, ref, got in (("h", h, h32), ("stash", stash, stash32)):
        _room("gru fwd %s %s" % (case, name), got, ref, R.REL_GRU)
        _sight("gru fwd %s %s" % (case, name), ref, B, H, R.GRU_TILE, R.GRU_TILE, R.REL_GRU)


@pytest.mark.parametrize("B,H", R.GRU_SHAPES)
@pytest.mark.parametrize("zero_state,with_dh_out", [(False, True), (True, True), (False, False)])
def test_gru_backward_reference_is_fp64_autograd(B, H, zero_state, with_dh_out):
    """Two steps h0 -> h1 -> h2 of torch's cell under autograd (L = sum h2 . dh_out2 + sum h1 . dh_out1) against the reference's last
    step (no dgh_next) and the step before it, in every null form: h_prev None (zero state), dh_out None.  dgh is held through
    dW_hh = sum dgh^T h_prev and db_hh = the column sums of dgh, which only it determines."""
    d = R.gru_inputs(B, H)
    w = _d(d["w_hh"]).requires_grad_()
    bh = _d(d["b_hh"]).requires_grad_()
    h0 = torch.zeros(B, H, dtype=F64) if zero_state else _d(d["h_prev"])
    g1, g2 = _d(d["gx"]).requires_grad_(), _d(d["gx_next"]).requires_grad_()
    h1 = _torch_cell(torch.nn.GRUCell, g1, w, bh, h0)
    h1.retain_grad()
    h2 = _torch_cell(torch.nn.GRUCell, g2, w, bh, h1)
    loss = (h2 * _d(d["dh_out"])).sum()
    if with_dh_out:
        loss = loss + (h1 * _d(d["dh_in"])).sum()            # (dh_in plays dh_out of the earlier step here)
    loss.backward()
    hp = None if zero_state else d["h_prev"]
    st1 = torch.cat(R.gru_cell_fwd(g1.detach(), w.detach(), bh.detach(), hp)[1:], 1)
    st2 = torch.cat(R.gru_cell_fwd(g2.detach(), w.detach(), bh.detach(), h1.detach())[1:], 1)
    dgx2, dgh2, dh2 = R.gru_step_bwd(None, d["w_hh"], None, d["dh_out"], st2, h1.detach(), None)
    dgx1, dgh1, dh1 = R.gru_step_bwd(dgh2, d["w_hh"], st2, d["dh_in"] if with_dh_out else None, st1, hp, dh2)
    assert torch.equal(dh2, _d(d["dh_out"]))
    assert (dgx2 - g2.grad).abs().max().item() < 1e-12 and (dgx1 - g1.grad).abs().max().item() < 1e-12
    assert (dh1 - h1.grad).abs().max().item() < 1e-12
    assert (dgh2.t() @ h1.detach() + dgh1.t() @ h0 - w.grad).abs().max().item() < 1e-11
    assert (dgh2.sum(0) + dgh1.sum(0) - bh.grad).abs().max().item() < 1e-11
    # nothing arrives: the last step without dh_out
    for t in R.gru_step_bwd(None, d["w_hh"], None, None, st2, h1.detach(), None):
        assert float(t.abs().max()) == 0.0


@pytest.mark.parametrize("case", GRU_BWD_CASES, ids=_ids)
def test_gru_backward_cases_room_and_sight(case):
    B, H, form = case
    ref, got = R.gru_bwd_ref(B, H, form), R.gru_bwd_ref(B, H, form, F32)
    for name, r, g in zip(("dgx", "dgh", "dh"), ref, got):
        if form == "last_no_dh_out":
            assert float(r.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
            continue
        _room("gru bwd %s %s" % (case, name), g, r, R.REL_GRU)
        _sight("gru bwd %s %s" % (case, name), r, B, H, R.GRU_TILE, R.GRU_TILE, R.REL_GRU)


# ---------------------------------------------------------------------------------------------------------------------- chain
def _autograd_chain(T, B, H, layers):
    """the chain on torch's fp64 nn.LSTMCell under autograd: per layer (h [T*B, H], c, [gate inputs of every step]); the gate
    inputs keep their gradients = dG.  Backward of L = sum over layers and steps t >= dh_t0 of h_t . dh_ext."""
    outs, loss, x_all = [], 0.0, None
    zero = torch.zeros(B, H, dtype=F64)
    for j, l in enumerate(layers):
        w_hh, bias = _d(l["w_hh"]), _d(l["bias"])
        t0, ng = l.get("gx_t0", 0), l.get("n_gx", 0)
        if j == 0:
            x_all = _d(l.get("x_in"))
        h, c = (zero if l.get("h0") is None else _d(l["h0"])), (zero if l.get("c0") is None else _d(l["c0"]))
        hs, cs, gis = [], [], []
        for t in range(T):
            gi = _d(l["gx"])[(t - t0) * B:(t - t0 + 1) * B] if t0 <= t < t0 + ng else bias.expand(B, -1)
            gi = gi + torch.zeros(B, 4 * H, dtype=F64, requires_grad=True)
            if x_all is not None:
                gi = gi + x_all[t * B:(t + 1) * B] @ _d(l["w_in"]).t()
            if l.get("emb") is not None:
                gi = gi + _d(l["emb"])[l["tok_ids"]] @ _d(l["w_e"]).t()
            gi.retain_grad()
            h, c = _torch_cell(torch.nn.LSTMCell, gi, w_hh, None, (h, c))
            hs.append(h), cs.append(c), gis.append(gi)
        h_all = torch.cat(hs)
        outs.append((h_all, torch.cat(cs), gis))
        x_all = h_all if l.get("mask") is None else h_all * _d(l["mask"])
        e0 = l.get("dh_t0", 0)
        if l.get("dh_ext") is not None and e0 < T:
            loss = loss + (h_all[e0 * B:] * _d(l["dh_ext"])).sum()
    return outs, loss


def _check_forward_is_torch(T, B, H, layers, fwd, outs):
    for j, l in enumerate(layers):
        h, c, stash, hm = fwd[j]
        assert (h - outs[j][0].detach()).abs().max().item() < 1e-12 and (c - outs[j][1].detach()).abs().max().item() < 1e-12
        pre = torch.cat([g.detach() for g in outs[j][2]])
        h_before = torch.cat([torch.zeros(B, H, dtype=F64) if l.get("h0") is None else _d(l["h0"]), h[:(T - 1) * B]])
        i, f, g, o = (pre + h_before @ _d(l["w_hh"]).t()).chunk(4, 1)
        want = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)], 1)
        assert (stash - want).abs().max().item() < 1e-12
        assert (hm is None) == (l.get("mask") is None)
        if hm is not None:
            assert torch.equal(hm, h * _d(l["mask"]))


@pytest.mark.parametrize("case", CHAIN_CASES, ids=_ids)
def test_chain_reference_room_and_sight(case):
    B, H, form = case
    c = R.chain_case(B, H, form)
    T, layers = c["T"], c["layers"]
    fwd, dgs = R.chain_ref(B, H, form)
    outs, loss = _autograd_chain(T, B, H, layers)
    _check_forward_is_torch(T, B, H, layers, fwd, outs)
    if form == "nothing_flows":
        assert all(float(dg.abs().max()) == 0.0 for dg in dgs)
    else:
        loss.backward()
        for j in range(len(layers)):
            assert (dgs[j] - torch.cat([g.grad for g in outs[j][2]])).abs().max().item() < 1e-12, j
            assert float(dgs[j].abs().max()) > 1e-3
    fwd32, dgs32 = R.chain_ref(B, H, form, F32)
    rows = R.chain_fwd_rows(B, R.chain_vec(H))
    rows = (16, rows) if (B, H) == R.CHAIN_MISALIGNED else (rows,)      # the misaligned launches run the 16-row tile, the aligned one the 32-row
    for j in range(len(layers)):
        for name, ref, got in zip(("h", "c", "stash", "hm"), fwd[j], fwd32[j]):
            if ref is None:
                continue
            what = "chain %s layer %d %s" % (case, j, name)
            _room(what, got, ref, R.REL_CHAIN)
            for tm in rows:
                _sight(what, ref, B, H, tm, R.CHAIN_FWD_UNITS, R.REL_CHAIN)
        if form != "nothing_flows":
            what = "chain %s layer %d dG" % (case, j)
            _room(what, dgs32[j], dgs[j], R.REL_CHAIN_DG)
            _sight(what, dgs[j], B, H, R.CHAIN_BWD_TILE, R.CHAIN_BWD_TILE, R.REL_CHAIN_DG)


@pytest.mark.parametrize("case", TOKEN_CASES, ids=_ids)
def test_chain_token_reference_room_and_sight(case):
    B, H, E, source = case
    layers = R.token_layers(B, H, E, source)
    fwd = R.token_ref(*case)
    outs, _ = _autograd_chain(1, B, H, layers)
    _check_forward_is_torch(1, B, H, layers, fwd, outs)
    c = R.token_case(B, H, E)
    assert 0 <= c["tok_const"] < c["V"] and int(c["toks"].min()) >= 0 and int(c["toks"].max()) < c["V"]
    fwd32 = R.token_ref(B, H, E, source, F32)
    rows = R.chain_fwd_rows(B, R.chain_vec(H, E))
    for j in range(2):
        for name, ref, got in zip(("h", "c", "stash"), fwd[j], fwd32[j]):
            what = "token chain %s layer %d %s" % (case, j, name)
            _room(what, got, ref, R.REL_CHAIN)
            _sight(what, ref, B, H, rows, R.CHAIN_FWD_UNITS, R.REL_CHAIN)


def test_gemv_lds_case_in_fp32_is_inside_its_bound():
    d, h, c = R.gemv_lds_inputs()
    B, H, E = R.GEMV_LDS_CASE
    pre = d["gx"] + d["emb"][d["tok"].long()] @ d["w_ih"][:, :E].t()
    h32, c32, _ = R.L.cell_fwd(pre, d["w_hh"], d["h_prev"], d["c_prev"], F32)
    e = (R.err(h32, h), R.err(c32, c))
    print("gemv lds case fp32 h %.3g c %.3g (bound %.3g)" % (e[0], e[1], R.TOL_GEMV))
    assert max(e) < R.TOL_GEMV / 2
