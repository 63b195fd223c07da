"""mode='train' on K captions per clip with one encode per clip (3-D targets [B, K, L-1] -> logits [B, K, L-1, V];
functional.train_forward_group, s2vt_train_group_forward / _backward: the grouped path of csrc/api_train_f32.hip) and its group-sum kernel
(s2vt_group_sum_rows, csrc/group.hip).

The contract: the logits are those of mode='train' on feats.repeat_interleave(K, 0) with targets.reshape(B*K, L-1); the backward
gives that call's 13 parameter gradients and its dfeats summed over each clip's K rows.  Reference of the whole-path tests: the
oracle on the repeated clips, with the bounds of test_gpu_parity.py::test_against_oracle_on_fresh_seeds (logits 2e-5, loss 1e-5,
gradients 1e-6 + 1e-4 * max|ref|)."""
import ctypes
import functools

import pytest
import torch

from oracle import s2vt_oracle as orc
from s2vt_video_caption_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, K, L, F, H, E, V): K = 1; the smallest grouped case; ragged B and odd K; the fixtures' tiny dims at K = 5; R = B * K = 64, one
# full 64-row block of the column sums and GEMM tiles; R = 65, one row past it
SHAPES = [(1, 1, 4, 20, 12, 8, 23), (3, 2, 4, 20, 12, 8, 23), (19, 3, 6, 33, 36, 20, 57), (8, 5, 8, 64, 32, 24, 50),
          (16, 4, 5, 70, 44, 28, 61), (13, 5, 5, 70, 44, 28, 61)]
S85, S164 = SHAPES[3], SHAPES[4]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _model(shape, sd=None, **kw):
    import S2VTModel
    B, K, L, Fd, H, E, V = shape
    m = S2VTModel.S2VT(V, Fd, L, dim_hid=H, dim_embed=E, **kw)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _data(shape):
    """(state dict, feats [B, L, F], caps [B, K, L], mask [B, K, L]) on the host, seeded by the shape; never modified"""
    B, K, L, Fd, H, E, V = shape
    seed = 7 + B + 10 * K
    sd = synth.make_state_dict(V, Fd, H, E, seed=seed)
    feats, caps, mask = synth.make_batch(B * K, L, Fd, V, seed=seed, min_words=1)
    return sd, feats[:B].contiguous(), caps.view(B, K, L), mask.view(B, K, L)


def _assert_captions_differ(caps, mask):
    """within a clip the K captions differ in words (every pair, every clip) and - in at least one clip - in length"""
    B, K, L = caps.shape
    if K == 1:
        return
    for b in range(B):
        for i in range(K):
            for j in range(i + 1, K):
                assert not torch.equal(caps[b, i], caps[b, j]), (b, i, j)
    lens = mask.sum(2)
    assert bool((lens.max(1).values != lens.min(1).values).any())


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    """The oracle on the repeated clips: (logits [B*K, L-1, V], loss, {name: grad}, dfeats summed over K [B, L, F])"""
    B, K, L, Fd, H, E, V = shape
    sd, feats, caps, mask = _data(shape)
    om = orc.OracleModel(sd)
    fo = feats.repeat_interleave(K, 0).requires_grad_()
    ologits = om(fo, caps.reshape(B * K, L)[:, :-1])
    oloss = orc.mask_criterion(ologits, caps.reshape(B * K, L), mask.reshape(B * K, L))
    oloss.backward()
    grads = {k: q.grad.clone() for k, q in om.as_dict().items()}
    return ologits.detach(), float(oloss.detach()), grads, fo.grad.view(B, K, L, Fd).sum(1)


def _grouped(m, shape, targets=None, feats=None):
    """forward + MaskCriterion + backward of the grouped call: (logits [B, K, L-1, V], loss, {name: grad}, dfeats)"""
    import utils
    B, K, L, Fd, H, E, V = shape
    sd, f0, caps, mask = _data(shape)
    f = (f0 if feats is None else feats).to(DEV).requires_grad_()
    c = caps.to(DEV)
    m.zero_grad(set_to_none=True)
    logits = m(f, targets=c[:, :, :-1] if targets is None else targets, mode="train")
    assert tuple(logits.shape) == (B, K, L - 1, V)
    loss = utils.MaskCriterion()(logits.flatten(0, 1), c.view(B * K, L), mask.to(DEV).view(B * K, L))
    loss.backward()
    return logits.detach(), float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()}, f.grad.clone()


def _repeated(m, shape):
    """the same on the repeated clips through mode='train' (the definition): dfeats summed over each clip's K rows"""
    import utils
    B, K, L, Fd, H, E, V = shape
    sd, f0, caps, mask = _data(shape)
    f = f0.repeat_interleave(K, 0).to(DEV).requires_grad_()
    c = caps.reshape(B * K, L).to(DEV)
    m.zero_grad(set_to_none=True)
    logits = m(f, targets=c[:, :-1], mode="train")
    loss = utils.MaskCriterion()(logits, c, mask.reshape(B * K, L).to(DEV))
    loss.backward()
    return logits.detach(), float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()}, f.grad.view(B, K, L, Fd).sum(1)


def _assert_close(got, ref, what):
    """the project's bounds: logits < 2e-5, loss < 1e-5, every gradient within 1e-6 + 1e-4 * max|ref|"""
    (gl, gloss, gg, gdf), (rl, rloss, rg, rdf) = got, ref
    err = (gl.flatten(0, 1).cpu() - rl.reshape(gl.flatten(0, 1).shape).cpu()).abs().max().item()
    print(what, "logits", err, "loss", abs(gloss - rloss))
    assert err < 2e-5, what
    assert abs(gloss - rloss) < 1e-5, what
    assert list(gg) == list(rg)
    for n in gg:
        e, s = (gg[n].cpu() - rg[n].cpu()).abs().max().item(), rg[n].abs().max().item()
        print(what, n, e, s)
        assert e <= 1e-6 + 1e-4 * s, (what, n, e, s)
    e, s = (gdf.cpu() - rdf.cpu()).abs().max().item(), rdf.abs().max().item()
    print(what, "dfeats", e, s)
    assert e <= 1e-6 + 1e-4 * s, (what, "dfeats", e, s)


# ------------------------------------------------------------------ the group-sum kernel
@pytest.mark.parametrize("K", [1, 2, 5, 7])
def test_group_sum_rows_is_the_ordered_fp32_sum(lib, K):
    """out[g] = in[g*K] + in[g*K+1] + ... in that order, bitwise equal to the fp32 loop on the host, for column counts that are not
    multiples of 4, one group and many, row strides larger than cols (a multiple of 4 floats: the 16-byte path with its scalar
    tail; an odd stride: the scalar path); nothing outside [groups, cols] of the output is written (sentinel border)."""
    gen = torch.Generator().manual_seed(100 + K)
    for cols in (1, 48, 130, 4000):
        for groups in (1, 19, 1264):
            for pad in (4, 5):
                ld_in = (cols + 3) // 4 * 4 + pad
                ld_out = (cols + 3) // 4 * 4 + 2 * pad
                x = torch.randn(groups * K, ld_in, generator=gen) * torch.logspace(-3, 3, groups * K).unsqueeze(1)
                v = x.view(groups, K, ld_in)[:, :, :cols]
                acc = v[:, 0].clone()
                for k in range(1, K):
                    acc = acc + v[:, k]
                out = torch.full((groups + 2, ld_out), -7.5, device=DEV)
                xd = x.to(DEV)
                rc = lib.s2vt_group_sum_rows(_ptr(xd), ld_in, ctypes.c_void_p(out.data_ptr() + 4 * ld_out), ld_out, groups, K, cols, _stream())
                assert rc == 0, lib.s2vt_last_error()
                got = out.cpu()
                assert torch.equal(got[1:groups + 1, :cols], acc), (K, cols, groups, pad)
                assert bool((got[0] == -7.5).all()) and bool((got[groups + 1] == -7.5).all()), (K, cols, groups, pad)
                assert bool((got[:, cols:] == -7.5).all()), (K, cols, groups, pad)


def test_group_sum_rows_refuses_bad_arguments(lib):
    x = torch.zeros(8, 8, device=DEV)
    o = torch.zeros(8, 8, device=DEV)
    assert lib.s2vt_group_sum_rows(_ptr(x), 8, _ptr(o), 8, 4, 0, 8, _stream()) == -1          # K < 1
    assert lib.s2vt_group_sum_rows(_ptr(x), 4, _ptr(o), 8, 4, 2, 8, _stream()) == -1          # ld_in < cols
    assert lib.s2vt_group_sum_rows(_ptr(x), 8, _ptr(x), 8, 4, 2, 8, _stream()) == -1          # aliased
    assert lib.s2vt_group_sum_rows(None, 8, _ptr(o), 8, 4, 2, 8, _stream()) == -1


# ------------------------------------------------------------------ the whole path
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dK%dL%d" % s[:3])
def test_grouped_train_step_matches_the_oracle_on_repeated_clips(lib, shape):
    """logits, loss, the 13 parameter gradients and dfeats (the oracle's summed over K).  A missing dc or dG group sum leaves the
    encode-side gradients (vid_rnn, feat_linear, dfeats) far outside the bound."""
    sd, feats, caps, mask = _data(shape)
    _assert_captions_differ(caps, mask)
    got = _grouped(_model(shape, sd), shape)
    _assert_close(got, _oracle(shape), "oracle %s" % (shape,))
    from s2vt_video_caption_amd import capi
    torch.cuda.synchronize()
    capi.check_async_error()


@pytest.mark.parametrize("shape", [S85, S164], ids=["8x5", "16x4"])
@pytest.mark.parametrize("gemm_mode", [0, 3])
def test_grouped_equals_train_mode_on_repeated_clips_on_the_device(lib, shape, gemm_mode):
    """the definition itself, with the repeated call on the fp32-MFMA driver (mode 0) and on the split-precision plane drivers
    (mode 3: B * K = 40 runs padded to 64 rows, 64 as it is)"""
    sd = _data(shape)[0]
    prev = lib.s2vt_set_gemm_mode(gemm_mode)
    try:
        m = _model(shape, sd)
        ref = _repeated(m, shape)
        got = _grouped(m, shape)
    finally:
        lib.s2vt_set_gemm_mode(prev)
    _assert_close(got, ref, "device mode %d %s" % (gemm_mode, shape))


@pytest.mark.parametrize("pipe_block", [0, 2, 3])
def test_every_block_schedule_matches_the_oracle(lib, pipe_block):
    """the lanes' block pipeline: one stream (0), and blocks shorter than the caption (2, 3 timesteps at L = 8: several encode
    and several decode blocks, the last one ragged) - the default block of 32 timesteps covers the other tests' captions in one"""
    prev = lib.s2vt_set_option(b"pipe_block", pipe_block)
    try:
        got = _grouped(_model(S85, _data(S85)[0]), S85)
    finally:
        lib.s2vt_set_option(b"pipe_block", prev)
    _assert_close(got, _oracle(S85), "pipe_block %d" % pipe_block)


def test_k_equal_one_is_train_mode(lib):
    shape = (5, 1, 6, 33, 36, 20, 57)
    m = _model(shape, _data(shape)[0])
    _assert_close(_grouped(m, shape), _repeated(m, shape), "K=1")


def test_two_runs_are_bitwise_equal(lib):
    m = _model(S85, _data(S85)[0])
    a, b = _grouped(m, S85), _grouped(m, S85)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[3], b[3])
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def test_expanded_and_strided_target_views_are_read_as_they_are(lib):
    """one caption per clip expanded to K rows (stride 0 along K), and a non-contiguous [B, K, L-1] slice of a wider tensor, give
    the result of their contiguous copies"""
    B, K, L, Fd, H, E, V = S85
    sd, feats, caps, mask = _data(S85)
    m = _model(S85, sd)
    c = caps.to(DEV)
    one = c[:, 0, :-1]
    exp = one[:, None, :].expand(B, K, L - 1)
    assert exp.stride(1) == 0
    a, b = _grouped(m, S85, targets=exp), _grouped(m, S85, targets=exp.contiguous())
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and all(torch.equal(a[2][n], b[2][n]) for n in a[2])
    wide = torch.zeros(B, 2 * K, L + 3, dtype=torch.long, device=DEV)
    wide[:, ::2, 2:L + 1] = c[:, :, :-1]
    view = wide[:, ::2, 2:L + 1]
    assert not view.is_contiguous()
    a, b = _grouped(m, S85, targets=view), _grouped(m, S85)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and all(torch.equal(a[2][n], b[2][n]) for n in a[2])


def test_out_dropout_matches_the_oracle_with_the_same_mask(lib):
    """out_dropout = 0.5 in train mode: the mask is the draw nn.Dropout makes on a [B*K, L-1, H] ones tensor"""
    import utils
    B, K, L, Fd, H, E, V = S85
    sd, feats, caps, mask = _data(S85)
    m = _model(S85, sd, out_dropout=0.5)
    m.train()
    torch.manual_seed(11)
    keep = m.out_drop(torch.ones(B * K, L - 1, H, device=DEV)).cpu()
    assert 0.2 < float((keep == 0).float().mean()) < 0.8
    torch.manual_seed(11)
    got = _grouped(m, S85)
    om = orc.OracleModel(sd)
    fo = feats.repeat_interleave(K, 0).requires_grad_()
    ologits = om(fo, caps.reshape(B * K, L)[:, :-1], out_mask=keep)
    oloss = orc.mask_criterion(ologits, caps.reshape(B * K, L), mask.reshape(B * K, L))
    oloss.backward()
    ref = (ologits.detach(), float(oloss.detach()), {k: q.grad for k, q in om.as_dict().items()}, fo.grad.view(B, K, L, Fd).sum(1))
    _assert_close(got, ref, "dropout")


def test_grad_sink_receives_the_thirteen_gradients(lib):
    from s2vt_video_caption_amd import functional
    sd = _data(S85)[0]
    m = _model(S85, sd)
    ref = _grouped(m, S85)
    sink = [torch.full_like(p, float("nan")) for p in m._hip_params()]
    functional.set_grad_sink(m, sink)
    try:
        got = _grouped_nograd_read(m, S85)
    finally:
        functional.set_grad_sink(m, None)
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(got, ref[0])
    by_name = {id(p): n for n, p in m.named_parameters()}
    for p, g in zip(m._hip_params(), sink):
        assert torch.equal(g, ref[2][by_name[id(p)]]), by_name[id(p)]


def _grouped_nograd_read(m, shape):
    import utils
    B, K, L, Fd, H, E, V = shape
    sd, f0, caps, mask = _data(shape)
    c = caps.to(DEV)
    m.zero_grad(set_to_none=True)
    logits = m(f0.to(DEV).requires_grad_(), targets=c[:, :, :-1], mode="train")
    utils.MaskCriterion()(logits.flatten(0, 1), c.view(B * K, L), mask.to(DEV).view(B * K, L)).backward()
    return logits.detach()


def test_bad_id_raises_index_error_and_leaves_the_other_rows_alone(lib):
    from s2vt_video_caption_amd import capi
    B, K, L, Fd, H, E, V = S85
    sd, feats, caps, mask = _data(S85)
    m = _model(S85, sd)
    f = feats.to(DEV)
    good = caps[:, :, :-1].to(DEV)
    with torch.no_grad():
        ref = m(f, targets=good, mode="train")
        torch.cuda.synchronize()
        capi.check_async_error()
        bad = good.clone()
        bad[2, 3, 1] = V + 5
        out = m(f, targets=bad, mode="train")
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            capi.check_async_error()
    keep = torch.ones(B, K, dtype=torch.bool)
    keep[2, 3] = False
    assert torch.equal(out[keep.to(DEV)], ref[keep.to(DEV)])
    capi.check_async_error()          # reported once


def test_second_backward_on_one_forward_is_refused(lib):
    from s2vt_video_caption_amd import capi
    B, K, L, Fd, H, E, V = S85
    sd, feats, caps, mask = _data(S85)
    m = _model(S85, sd)
    logits = m(feats.to(DEV), targets=caps[:, :, :-1].to(DEV), mode="train")
    loss = logits.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(capi.S2VTHipError, match="backward ran twice"):
        loss.backward()


@pytest.mark.parametrize("kind", ["gru", "stacked"])
def test_gru_and_stacked_models_run_the_repeated_clips(lib, kind):
    import S2VTModel
    B, K, L, Fd, H, E, V = 3, 2, 4, 20, 12, 8, 23
    torch.manual_seed(5)
    kw = dict(rnn_type="gru") if kind == "gru" else dict(num_layers=2)
    m = S2VTModel.S2VT(V, Fd, L, dim_hid=H, dim_embed=E, **kw).to(DEV)
    feats, caps, mask = synth.make_batch(B * K, L, Fd, V, seed=3, min_words=1)
    f, c = feats[:B].to(DEV), caps.view(B, K, L).to(DEV)
    with torch.no_grad():
        got = m(f, targets=c[:, :, :-1], mode="train")
        ref = m(f.repeat_interleave(K, 0), targets=c.view(B * K, L)[:, :-1], mode="train")
    assert tuple(got.shape) == (B, K, L - 1, V)
    assert torch.equal(got.flatten(0, 1), ref)


def test_dp_train_step_with_group_equals_the_step_on_repeated_clips(lib):
    """dp.train_step(..., group=K) against the un-grouped step on the repeated clips: parameters after one Adam step within
    1e-6 + 1e-4 * max|ref|"""
    import utils
    from s2vt_video_caption_amd import dp
    B, K, L, Fd, H, E, V = S85
    sd, feats, caps, mask = _data(S85)
    c, k = caps.reshape(B * K, L).to(DEV), mask.reshape(B * K, L).to(DEV)
    crit = utils.MaskCriterion()
    ma, mb = _model(S85, sd), _model(S85, sd)
    oa, ob = torch.optim.Adam(ma.parameters(), lr=1e-4), torch.optim.Adam(mb.parameters(), lr=1e-4)
    la = dp.train_step(ma, crit, oa, feats.to(DEV), c, k, group=K)
    lb = dp.train_step(mb, crit, ob, feats.repeat_interleave(K, 0).to(DEV), c, k)
    assert abs(float(la) - float(lb)) < 1e-5
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        e, s = (p - q).abs().max().item(), q.abs().max().item()
        assert e <= 1e-6 + 1e-4 * s, (n, e, s)
        assert not torch.equal(q.detach().cpu(), sd[n]), n          # the step moved the parameter
