"""GPU: the clipped step (include/s2vt_hip.h, "clipped step"; csrc/optim.hip) through the C ABI against its numpy restatement
(tests/optim_ref.py, itself checked against torch in tests/test_optim_clip_host.py), and optim.FlatAdam's new arguments on a small model."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def _chunk():
    from s2vt_video_caption_amd import capi
    return capi.GRAD_NORM_CHUNK


def _grads(n, seed, steps=1):
    """the gradient recipe of test_flat_adam_step_is_torch_adam: randn * 10^k, k drawn from [-4, 1]"""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    return p0, [torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-4, 2, (1,), generator=g))) for _ in range(steps)]


class Norm:
    """s2vt_grad_norm on a device gradient: owns the record and the workspace"""

    def __init__(self, lib, n):
        self.lib, self.n = lib, n
        self.rec = torch.zeros(8, dtype=torch.int32, device=DEV)                 # the caller zeroes the record once
        self.ws = torch.empty(max(1, lib.s2vt_grad_norm_workspace_bytes(n) // 8), dtype=torch.float64, device=DEV)

    def __call__(self, g, max_norm=0.0, skip=0):
        assert self.lib.s2vt_grad_norm(ptr(g), self.n, max_norm, skip, ptr(self.ws), self.ws.numel() * 8, ptr(self.rec), None) == 0
        torch.cuda.synchronize()
        raw = self.rec.cpu().numpy()
        return {"bytes": raw.tobytes(), "grad_norm": raw.view(np.float32)[0], "scale": raw.view(np.float32)[1], "nonfinite": int(raw[2]),
                "skipped_total": int(raw.view(np.int64)[2])}


def _step(lib, p, g, m, v, step, wd=0.0, decoupled=0, ends=None, flags=None, skip=0, rec=None):
    n = p.numel()
    se = (ctypes.c_int64 * len(ends))(*ends) if ends else None
    sf = (ctypes.c_int32 * len(flags))(*flags) if ends else None
    rc = lib.s2vt_adam_step_clipped(ptr(p), ptr(g), ptr(m), ptr(v), n, LR, B1, B2, EPS, step, wd, decoupled, se, sf, len(ends) if ends else 0,
                                    skip, ptr(rec) if rec is not None else None, None)
    assert rc == 0, lib.s2vt_last_error()


def _norm_sizes():
    C = 16384       # asserted against the library's constant in the test
    return [1, 3, 5, 4096, C - 1, C, C + 1, 2 * C + 5, 1000003]


@pytest.mark.parametrize("n", _norm_sizes())
def test_grad_norm_at_the_edges(lib, n):
    """fp32(sqrt(sum of fp64 squares)) within one spacing of numpy's: an fp32 square is exact in fp64 and an fp64 sum of 2^20 terms is
    good to ~1e-10, so only the final rounding can differ.  Same record bytes on a second call; the same norm from a gradient pointer
    offset by 4 bytes (the scalar path); scale is the fp32 formula on the norm the record holds; max_norm above the norm gives 1.0f."""
    assert _chunk() == 16384
    _, (grad,) = _grads(n, seed=n)
    want = optim_ref.grad_norm_ref(grad.numpy())
    gd = grad.to(DEV)
    norm = Norm(lib, n)
    c = 0.5 * float(want)
    a = norm(gd, c)
    b = norm(gd, c)
    print("n", n, "got", a["grad_norm"], "want", want, "scale", a["scale"])
    assert abs(float(a["grad_norm"]) - float(want)) <= float(np.spacing(want))
    assert a["bytes"] == b["bytes"] and a["nonfinite"] == 0 and a["skipped_total"] == 0
    assert a["scale"] == f32(c) / (a["grad_norm"] + f32(1e-6)) and a["scale"] < 1
    buf = torch.zeros(n + 1, device=DEV)
    off = buf[1:]
    off.copy_(gd)
    assert off.data_ptr() % 16 == 4
    o = norm(off, c)
    assert o["bytes"] == a["bytes"]
    hi = norm(gd, 2.0 * float(want))
    assert hi["scale"] == f32(1.0) and hi["grad_norm"] == a["grad_norm"]
    assert norm(gd, 0.0)["scale"] == f32(1.0) and norm(gd, -3.0)["scale"] == f32(1.0) and norm(gd, float("inf"))["scale"] == f32(1.0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("where", ["first", "last", "chunk"])
def test_nonfinite_gradient_is_flagged_skipped_or_propagated(lib, bad, where):
    """One inf / NaN at index 0, n - 1 or a chunk boundary: nonfinite = 1.  With skip_nonfinite the step leaves p, m, v bit-identical
    and skipped_total advances by one per call; without it the step runs and the NaNs land where torch's clip_grad_norm_ + Adam put
    them (an inf norm gives coefficient 0 and 0 * inf = NaN in that element alone; a NaN norm a NaN coefficient and NaN everywhere)."""
    C = _chunk()
    n = 2 * C + 5
    ix = {"first": 0, "last": n - 1, "chunk": C}[where]
    p0, (grad,) = _grads(n, seed=7)
    grad[ix] = bad
    gd = grad.to(DEV)
    norm = Norm(lib, n)
    m0, v0 = torch.rand(n) * 0.1, torch.rand(n) * 0.01
    p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    for k in (1, 2):
        r = norm(gd, 1.0, skip=1)
        assert r["nonfinite"] == 1 and r["skipped_total"] == k and not np.isfinite(r["grad_norm"])
        _step(lib, p, gd, m, v, k, wd=0.01, skip=1, rec=norm.rec)
        torch.cuda.synchronize()
        assert torch.equal(p.cpu().view(torch.int32), p0.view(torch.int32))
        assert torch.equal(m.cpu().view(torch.int32), m0.view(torch.int32)) and torch.equal(v.cpu().view(torch.int32), v0.view(torch.int32))
    # without the guard: the counter stands still, the step runs
    r = norm(gd, 1.0, skip=0)
    assert r["nonfinite"] == 1 and r["skipped_total"] == 2
    _step(lib, p, gd, m, v, 1, skip=0, rec=norm.rec)
    torch.cuda.synchronize()
    ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=LR)
    opt.state[ref] = {"step": torch.tensor(0.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    ref.grad = grad.clone()
    torch.nn.utils.clip_grad_norm_([ref], 1.0)
    opt.step()
    st = opt.state[ref]
    for got, want in ((p, ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want))
    assert int(torch.isnan(ref.detach()).sum()) == (1 if bad == float("inf") else n)


def _segments(n):
    """three segments at odd offsets - [0, n//3) decayed, [n//3, n//3 + 1001) not, the rest decayed; below 1002 elements the middle one
    is dropped (and an empty first one with it)"""
    ends, flags = [], []
    if n // 3 > 0:
        ends.append(n // 3); flags.append(1)
    if n >= 1002:
        ends.append(n // 3 + 1001); flags.append(0)
    ends.append(n); flags.append(1)
    mask = np.ones(n, dtype=bool)
    if n >= 1002:
        mask[n // 3:n // 3 + 1001] = False
    return ends, flags, mask


CASES = {"clip": dict(c=0.5), "l2": dict(wd=0.01), "adamw": dict(wd=0.01, decoupled=1), "clip_l2_segments": dict(c=0.5, wd=0.01, seg=True)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [1, 5, 4096, 1000003])
def test_clipped_step_is_its_restatement(lib, n, case):
    """Five steps of s2vt_grad_norm + s2vt_adam_step_clipped against optim_ref.step_ref: m, v within 4e-7 of their largest element
    (the bound of test_flat_adam_step_is_torch_adam), p within 2 * step spacings of its largest element (one final rounding of p per
    step on either side, doubled); the norm within one spacing and the scale the fp32 formula on it.  At n = 4096 torch itself
    (clip_grad_norm_ + Adam(weight_decay) / AdamW) stands beside them at the same bounds."""
    kw = CASES[case]
    c, wd, dec = kw.get("c"), kw.get("wd", 0.0), kw.get("decoupled", 0)
    ends, flags, mask = _segments(n) if kw.get("seg") else (None, None, None)
    p0, grads = _grads(n, seed=n, steps=5)
    rp, rm, rv = p0.numpy().copy(), np.zeros(n, f32), np.zeros(n, f32)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    norm = Norm(lib, n)
    with_torch = n == 4096 and not kw.get("seg")
    if with_torch:
        tref = p0.clone().requires_grad_()
        topt = (torch.optim.AdamW if dec else torch.optim.Adam)([tref], lr=LR, weight_decay=wd)
    for step, grad in enumerate(grads, 1):
        rnorm, rscale, _ = optim_ref.step_ref(rp, grad.numpy(), rm, rv, step, LR, B1, B2, EPS, max_norm=c, wd=wd, decoupled=bool(dec), decay_mask=mask)
        gd = grad.to(DEV)
        rec = None
        if c is not None:
            r = norm(gd, c)
            rec = norm.rec
            assert abs(float(r["grad_norm"]) - float(rnorm)) <= float(np.spacing(rnorm))
            assert r["scale"] == optim_ref.scale_ref(r["grad_norm"], c)
        _step(lib, p, gd, m, v, step, wd=wd, decoupled=dec, ends=ends, flags=flags, rec=rec)
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), grad)                         # the clipped gradient is not written back
        legs = [("restatement", rp, rm, rv)]
        if with_torch:
            tref.grad = grad.clone()
            if c is not None:
                torch.nn.utils.clip_grad_norm_([tref], c)
            topt.step()
            st = topt.state[tref]
            legs.append(("torch", tref.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()))
        for name, wp, wm, wv in legs:
            em, ev, ep = np.abs(m.cpu().numpy() - wm).max(), np.abs(v.cpu().numpy() - wv).max(), np.abs(p.cpu().numpy() - wp).max()
            bm, bv, bp = 4e-7 * np.abs(wm).max(), 4e-7 * np.abs(wv).max(), 2 * step * float(np.spacing(f32(np.abs(wp).max())))
            print(case, n, step, name, "m %.3g/%.3g v %.3g/%.3g p %.3g/%.3g" % (em, bm, ev, bv, ep, bp))
            assert em <= bm and ev <= bv and ep <= bp, (name, step)


def test_scale_one_is_the_plain_step_bit_for_bit(lib):
    """s2vt_grad_norm(max_norm = 1e30) + s2vt_adam_step_clipped(wd = 0) against s2vt_adam_step on copies of the same buffers, three steps
    at n = 1 000 003: the two kernels compile one update expression"""
    n = 1000003
    p0, grads = _grads(n, seed=11, steps=3)
    a = [p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [t.clone() for t in a]
    norm = Norm(lib, n)
    for step, grad in enumerate(grads, 1):
        gd = grad.to(DEV)
        assert lib.s2vt_adam_step(ptr(a[0]), ptr(gd), ptr(a[1]), ptr(a[2]), n, LR, B1, B2, EPS, step, None) == 0
        assert norm(gd, 1e30)["scale"] == f32(1.0)
        _step(lib, b[0], gd, b[1], b[2], step, rec=norm.rec)
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), step
    # ... and so is weight decay at 0 over segments, and the step without a record
    c = [t.clone() for t in a]
    gd = grads[0].to(DEV)
    assert lib.s2vt_adam_step(ptr(a[0]), ptr(gd), ptr(a[1]), ptr(a[2]), n, LR, B1, B2, EPS, 4, None) == 0
    _step(lib, b[0], gd, b[1], b[2], 4, wd=0.0, decoupled=1, ends=[5, n], flags=[1, 0], rec=None)
    _step(lib, c[0], gd, c[1], c[2], 4, wd=0.0, rec=None)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))


# ---------------------------------------------------------------- optim.FlatAdam on the small model of test_flat_adam_trains_the_model_as_torch_adam_does
DIMS = dict(L=12, Fd=64, H=96, E=80, V=200, B=16)


@pytest.fixture(scope="module")
def tiny():
    import utils
    from s2vt_video_caption_amd import synth
    d = DIMS
    sd = synth.make_state_dict(d["V"], d["Fd"], d["H"], d["E"], seed=5)
    feats, caps, mask = (t.to(DEV) for t in synth.make_batch(d["B"], d["L"], d["Fd"], d["V"], seed=6))
    return sd, feats, caps, mask, utils.MaskCriterion()


def _model(sd):
    import S2VTModel
    d = DIMS
    m = S2VTModel.S2VT(d["V"], d["Fd"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(sd)
    return m.to(DEV)


def _state(m):
    return {k: t.detach().cpu().clone() for k, t in m.state_dict().items()}


def _same_bits(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


class _Spy:
    """stands in for the ctypes library of a FlatAdam: records the entry points that are called"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("s2vt_") or name == "s2vt_last_error":
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_flat_adam_defaults_are_the_plain_step(lib, tiny):
    """FlatAdam(m, lr) and FlatAdam(m, lr, max_grad_norm=None, weight_decay=0.0): bit-identical parameters after three train steps, and
    the only entry point either calls is s2vt_adam_step, once per step"""
    from s2vt_video_caption_amd import dp, optim
    sd, feats, caps, mask, crit = tiny
    out = []
    for kw in ({}, dict(max_grad_norm=None, weight_decay=0.0, decoupled=True, no_decay=("bias",), skip_nonfinite=False)):
        m = _model(sd)
        opt = optim.FlatAdam(m, lr=1e-3, **kw)
        opt._lib = spy = _Spy(opt._lib)
        for _ in range(3):
            dp.train_step(m, crit, opt, feats, caps, mask, None)
        assert spy.calls == ["s2vt_adam_step"] * 3
        out.append(_state(m))
    assert _same_bits(*out)
    # with an option set: the norm's entry, then the clipped step; weight decay alone needs no norm
    for kw, want in ((dict(max_grad_norm=1.0), ["s2vt_grad_norm", "s2vt_adam_step_clipped"]), (dict(weight_decay=1e-2), ["s2vt_adam_step_clipped"]),
                     (dict(skip_nonfinite=True), ["s2vt_grad_norm", "s2vt_adam_step_clipped"])):
        m = _model(sd)
        opt = optim.FlatAdam(m, lr=1e-3, **kw)
        opt._lib = spy = _Spy(opt._lib)
        dp.train_step(m, crit, opt, feats, caps, mask, None)
        assert spy.calls == want, kw
        assert opt.skipped_steps == 0


def _grad_norm64(m):
    return float(torch.sqrt(sum((p.grad.detach().double() ** 2).sum() for p in m.parameters())))


def test_flat_adam_clips_and_decays_as_torch_does(lib, tiny):
    """Four steps of FlatAdam(max_grad_norm=c, weight_decay=1e-2) against torch.optim.Adam(weight_decay=1e-2) on gradients multiplied by
    optim_ref's scale, both from one state dict; c = half the first step's norm (from the torch leg), so every step is clipped.
    Losses within 2e-5 (the bound of test_flat_adam_trains_the_model_as_torch_adam_does); optimizer.grad_norm within 1e-5 relative of
    the fp64 norm of the 13 p.grad, which keep the UNCLIPPED gradient."""
    from s2vt_video_caption_amd import dp, optim
    sd, feats, caps, mask, crit = tiny
    mt = _model(sd)
    topt = torch.optim.Adam(mt.parameters(), lr=1e-3, weight_decay=1e-2)
    c, tl = None, []
    for _ in range(4):
        topt.zero_grad()
        mt.train()
        loss = crit(mt(feats, targets=caps[:, :-1], mode='train'), caps, mask)
        loss.backward()
        n64 = _grad_norm64(mt)
        c = 0.5 * n64 if c is None else c
        scale = float(optim_ref.scale_ref(f32(n64), c))
        assert scale < 1
        for p in mt.parameters():
            p.grad.mul_(scale)
        topt.step()
        tl.append(float(loss.detach()))
    mf = _model(sd)
    opt = optim.FlatAdam(mf, lr=1e-3, max_grad_norm=c, weight_decay=1e-2)
    fl = []
    for _ in range(4):
        fl.append(float(dp.train_step(mf, crit, opt, feats, caps, mask, None)))
        n64 = _grad_norm64(mf)
        assert float(opt.clip_scale) < 1 and opt.clip_scale.dim() == 0 and opt.grad_norm.is_cuda
        assert abs(float(opt.grad_norm) - n64) <= 1e-5 * n64
        assert float(opt.clip_scale) == float(optim_ref.scale_ref(f32(float(opt.grad_norm)), c))
    print("losses torch", tl, "flat", fl)
    assert tl[0] > tl[-1] and max(abs(a - b) for a, b in zip(tl, fl)) < 2e-5
    st, sf = _state(mt), _state(mf)
    for k in st:
        assert (st[k] - sf[k]).abs().max().item() < 2e-5, k
    assert opt.skipped_steps == 0


def test_flat_adam_state_dict_carries_the_new_arguments(lib, tiny):
    """state_dict() -> a fresh FlatAdam built with OTHER keyword values -> load_state_dict: the next step is bit-identical to the
    original's.  A state dict without the five new keys (one saved before they existed) loads and steps as the plain step."""
    from s2vt_video_caption_amd import dp, optim
    sd, feats, caps, mask, crit = tiny
    kw = dict(max_grad_norm=0.05, weight_decay=1e-2, decoupled=True, no_decay=("bias",), skip_nonfinite=True)
    m = _model(sd)
    opt = optim.FlatAdam(m, lr=1e-3, **kw)
    for _ in range(2):
        dp.train_step(m, crit, opt, feats, caps, mask, None)
    state, weights = opt.state_dict(), copy.deepcopy(m.state_dict())
    assert all(state["param_groups"][0][k] == v for k, v in kw.items())
    m2 = _model(weights)
    opt2 = optim.FlatAdam(m2, lr=5e-2, max_grad_norm=7.0, weight_decay=0.3, decoupled=False, no_decay=(), skip_nonfinite=False)
    opt2.load_state_dict(state)
    la, lb = float(dp.train_step(m, crit, opt, feats, caps, mask, None)), float(dp.train_step(m2, crit, opt2, feats, caps, mask, None))
    assert la == lb and _same_bits(_state(m), _state(m2))
    assert float(opt.clip_scale) < 1 and float(opt.clip_scale) == float(opt2.clip_scale)
    # a state from before the clipped step existed
    old = copy.deepcopy(state)
    for k in kw:
        del old["param_groups"][0][k]
    m3, m4 = _model(weights), _model(weights)
    opt3 = optim.FlatAdam(m3, lr=5e-2, **kw)
    opt3.load_state_dict(old)
    opt4 = optim.FlatAdam(m4, lr=1e-3)
    opt4.load_state_dict(old)
    opt3._lib = spy = _Spy(opt3._lib)
    dp.train_step(m3, crit, opt3, feats, caps, mask, None)
    dp.train_step(m4, crit, opt4, feats, caps, mask, None)
    assert spy.calls == ["s2vt_adam_step"] and _same_bits(_state(m3), _state(m4))


def test_flat_adam_with_a_reducer_takes_the_reducers_slices(lib, tiny):
    """FlatAdam(reducer=FlatGradAllReducer(...).attach(model), max_grad_norm=c, weight_decay, no_decay) in one process against the same
    optimizer without the reducer: the reducer lays the parameters out in ITS order, and the decay segments must follow it.  The
    norm's fp64 partial sums then run in another order, so its last fp32 bit and with it the parameters may differ by roundings: p
    within 2 * steps spacings of its largest element (a decay flag on the wrong slice moves p by ~lr = 1e-3)."""
    from s2vt_video_caption_amd import dp, optim
    sd, feats, caps, mask, crit = tiny
    kw = dict(max_grad_norm=0.05, weight_decay=0.1, no_decay=("bias", "embedding.weight"))
    out = []
    for with_reducer in (False, True):
        m = _model(sd)
        red = dp.FlatGradAllReducer(m.parameters()).attach(m) if with_reducer else None
        opt = optim.FlatAdam(m, lr=1e-3, reducer=red, **kw)
        for _ in range(3):
            dp.train_step(m, crit, opt, feats, caps, mask, red)
        assert float(opt.clip_scale) < 1
        out.append((_state(m), float(opt.grad_norm)))
    (sa, na), (sb, nb) = out
    assert abs(na - nb) <= float(np.spacing(f32(na)))
    for k in sa:
        assert (sa[k] - sb[k]).abs().max().item() <= 2 * 3 * float(np.spacing(f32(sa[k].abs().max().item()))), k
