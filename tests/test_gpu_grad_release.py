"""The release promise of the data-parallel overlap, for every backward schedule: s2vt_backward_wait_grads(g, stream) makes
`stream` wait until gradient group g is FINAL (group 0 = out_linear weight + bias, group 1 = word_rnn's 4 tensors + embedding).
dp.FlatGradAllReducer._all_reduce_overlapped starts each group's all-reduce the moment that wait completes, under the rest of
the backward, so a group released before its last write would all-reduce half-accumulated gradients on every replica - with
no error and single-GPU results still correct (the backward's final hand-off repairs them there).

A late producer is made late deterministically (s2vt_test_lane_delay: a spinning one-wave workgroup in front of every
Lane-helper launch of the backward on the caller's stream or on the side lane), then a watcher stream waits for each group and
snapshots it: the snapshot must be the final gradient bit for bit.  The final gradients are checked against an fp64 restatement
of the model (oracle.s2vt_oracle), and every case asserts that it ran the schedule it names (recurrence plan, persistent
launch count and the order of group 0's release behind them, co-run GEMMs in a profiled run).  The second half pins the
hipGraph cache keys of the train drivers: a schedule option changed between steps under graph mode must capture anew, not
replay the old schedule."""
import contextlib
import ctypes

import pytest
import torch

from oracle import s2vt_oracle as orc
from s2vt_video_caption_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELAY_US = 1000      # per delayed launch: longer than a one-layer persistent BPTT stage at config 2 (~345 us), so a write that is
                     # not ordered before a group's event lands long after the event fires
GROUP_OF = lambda n: 0 if n.startswith("out_linear") else 1 if n.startswith(("word_rnn", "embedding")) else 2

# Relative Frobenius error bound of each gradient against the fp64 reference, per arithmetic mode.  Split precision (gemm mode 3,
# three bf16 planes per operand) and the fp32-MFMA driver are fp32-equivalent: what is left is fp32 rounding of the sums and of
# the 2L-1-step recurrences: measured at most 6e-7 at H = 256 and 3e-6 at config 2 (out_linear.weight, k = 5056 rows), bounded
# at 1e-5.  bf16 operands (gemm mode 1) round every GEMM and recurrent operand to 8 bits of mantissa: measured 4.5e-3
# (vid_rnn.weight_ih at B = 256, L = 24), bounded at 2e-2.  A missing dW_o piece (>= 1/11 of the k range) or a stale schedule
# would be off by ~0.1-0.3.
TOL = {"x3": 1e-5, "fp32": 1e-5, "bf16": 2e-2}

MID = dict(F=512, E=256)
C2 = dict(F=4096, E=1000)


@contextlib.contextmanager
def _options(lib, **kv):
    prev = {k: lib.s2vt_set_option(k.encode(), v) for k, v in kv.items()}
    assert all(v != -(2 ** 31) for v in prev.values()), "unknown option"
    try:
        yield
    finally:
        for k, v in prev.items():
            lib.s2vt_set_option(k.encode(), v)


# ---- the schedule arithmetic of csrc/api_train.hip (train_backward_x3), restated to name what each case must reach
def _balanced_block(L, blk):
    if blk != 32 or L <= 0:
        return blk
    n = (L + 31) // 32
    return (L + n - 1) // n


def _stages(L, blk):
    """word_rnn stages of the persistent BPTT = blocks of pipe_bounds(T, L, balanced_block(L, blk))"""
    T = 2 * L - 1
    b = list(range(0, L, blk)) + list(range(L, T, blk)) + [T]
    return len(b) - 1


def _wo_pieces(R, corun):
    """parts dW_o is cut into by the one-layer schedule's wo_part(): corun_k rows each, the last one absorbing a rest < 512"""
    ck = (R // 64 * corun // 10) * 64
    r, n = 0, 0
    while r < R:
        kk = min(ck, R - r)
        if R - r - kk < 512:
            kk = R - r
        r += kk
        n += 1
    return n


def _dims(B, L, H, V, F, E):
    return dict(B=B, L=L, F=F, H=H, E=E, V=V)


# id, dims, options, expectation: bwd = recurrence plan of the backward (0 launch per timestep / fp32 driver, 1 persistent bf16,
# 3 persistent split precision), sched = "solo" (one layer per launch, co-run GEMMs, group 0 on the caller's stream behind the
# last launch), "corun2" (two-layer stages, the rest of dW_o on the side lane), "two" (two-layer stages, no co-run), "bf16p"
# (persistent bf16), "lanes" (no persistent BPTT), "fp32" (the non-plane driver); trailing = more dW_o pieces than stages
CASES = [
    ("default_solo", _dims(64, 48, 256, 2000, **MID), {}, dict(bwd=3, sched="solo", trailing=False, mode="x3")),
    ("many_pieces", _dims(64, 48, 256, 2000, **MID), dict(corun=1), dict(bwd=3, sched="solo", trailing=True, mode="x3")),
    ("two_stages", _dims(64, 48, 256, 2000, **MID), dict(pipe_block=128), dict(bwd=3, sched="solo", trailing=True, mode="x3")),
    ("no_pipeline", _dims(64, 48, 256, 2000, **MID), dict(pipe_block=0), dict(bwd=0, sched="lanes", mode="x3")),
    ("corun_not_solo", _dims(64, 48, 256, 2000, **MID), dict(bptt_solo=0), dict(bwd=3, sched="corun2", mode="x3")),
    ("no_corun", _dims(64, 48, 256, 2000, **MID), dict(corun=0), dict(bwd=3, sched="two", mode="x3")),
    ("launch_per_timestep", _dims(64, 48, 256, 2000, **MID), dict(persist=0), dict(bwd=0, sched="lanes", mode="x3")),
    ("b128_x3_corun5", _dims(128, 48, 256, 2000, **MID), dict(persist_x3_bwd=1, corun=5),
     dict(bwd=3, sched="solo", trailing=False, mode="x3")),
    ("bf16_persistent", _dims(256, 24, 256, 2000, **MID), dict(gemm_mode=1, bptt_units=16), dict(bwd=1, sched="bf16p", mode="bf16")),
    ("exact_fp32_mfma", _dims(64, 24, 256, 2000, **MID), dict(gemm_mode=0), dict(bwd=0, sched="fp32", mode="fp32")),
    ("ragged_padded", _dims(100, 24, 256, 2000, **MID), {}, dict(bwd=3, sched="solo", trailing=True, mode="x3")),   # at B = 128
    ("fp32_driver", _dims(19, 8, 36, 57, F=40, E=28), {}, dict(bwd=0, sched="fp32", mode="fp32")),
    ("dropout_fused_ce", _dims(64, 48, 256, 2000, **MID), {}, dict(bwd=3, sched="solo", trailing=False, mode="x3", dropout=0.3)),
    ("c2_default", _dims(64, 80, 1000, 12000, **C2), {}, dict(bwd=3, sched="solo", trailing=False, mode="x3")),
    ("c2_corun1", _dims(64, 80, 1000, 12000, **C2), dict(corun=1), dict(bwd=3, sched="solo", trailing=True, mode="x3")),
    ("cu_reserve24", _dims(64, 48, 256, 2000, **MID), dict(cu_reserve=24), dict(bwd=3, sched="solo", trailing=False, mode="x3")),
]

_REFS = {}


def _inputs(d, seed):
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed)
    feats, caps, mask = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1000 + seed)
    return sd, feats.to(DEV), caps.to(DEV), mask.to(DEV)


def _reference(d, seed, out_mask=None):
    """fp64 gradients of the 13 tensors (oracle.s2vt_oracle restated on the device in float64), once per (dims, seed, mask): the
    options under test must not change the mathematics"""
    key = (tuple(sorted(d.items())), seed, None if out_mask is None else float(out_mask.sum()))
    if key not in _REFS:
        sd, feats, caps, mask = _inputs(d, seed)
        om = orc.OracleModel(sd, torch.float64).to(DEV)
        logits = om(feats, caps[:, :-1], out_mask=out_mask)
        orc.mask_criterion(logits, caps, mask).backward()
        _REFS[key] = {k: p.grad.detach().clone() for k, p in om.as_dict().items()}
        del om, logits
    return _REFS[key]


def _model(d, sd, dropout=0.0):
    import S2VTModel
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], out_dropout=dropout)
    m.load_state_dict(sd)
    return m.to(DEV)


def _order(lib):
    n_p, after = ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert lib.s2vt_backward_order(ctypes.byref(n_p), ctypes.byref(after)) == 0
    return n_p.value, after.value


def _step_and_snapshot(lib, m, red, feats, caps, mask, lanes, mask_seed):
    """forward, loss and backward() on the current stream with the lane delay on; then, WITHOUT synchronising, a watcher stream
    waits for gradient groups 0 and 1 and snapshots their slices of the flat buffer.  Returns {name: snapshot}."""
    import utils
    from s2vt_video_caption_amd import capi
    names = {id(p): n for n, p in m.named_parameters()}
    members = {0: [], 1: []}
    for p, (lo, hi) in zip(red.params, red.slices):
        g = GROUP_OF(names[id(p)])
        if g < 2:
            members[g].append((names[id(p)], lo, hi))
    # high priority: a hardware queue of its own.  A stream of normal priority may share one with the library's side lane, and then
    # its snapshot would run behind everything the side lane had enqueued - an early release would go unseen
    watcher = torch.cuda.Stream(device=DEV, priority=-1)
    snaps = {}
    capi.check(lib.s2vt_test_lane_delay(lanes, DELAY_US), "s2vt_test_lane_delay")
    try:
        m.train()
        torch.manual_seed(mask_seed)            # the out_drop mask of a dropout case: the same draw in every run
        logits = m(feats, targets=caps[:, :-1], mode="train")
        loss = utils.MaskCriterion()(logits, caps, mask)
        loss.backward()
        with torch.cuda.stream(watcher):
            for g in (0, 1):
                capi.check(lib.s2vt_backward_wait_grads(g, ctypes.c_void_p(watcher.cuda_stream)), "s2vt_backward_wait_grads")
                for n, lo, hi in members[g]:
                    snaps[n] = red.flat[lo:hi].clone()
    finally:
        lib.s2vt_test_lane_delay(0, 0)
    torch.cuda.synchronize()
    capi.check_async_error()
    return snaps


def _corun_gemms(lib, m, feats, caps, mask, mask_seed):
    """co-run GEMM launches (s2vt_prof_read kind 5: planned for part of the compute units) of one backward, in a profiled run"""
    import utils
    from s2vt_video_caption_amd import capi
    m.train()
    torch.manual_seed(mask_seed)
    logits = m(feats, targets=caps[:, :-1], mode="train")
    loss = utils.MaskCriterion()(logits, caps, mask)
    torch.cuda.synchronize()
    lib.s2vt_prof_reset()
    lib.s2vt_prof_enable(1)
    try:
        loss.backward()
        torch.cuda.synchronize()
        _, n = capi.prof_read(5)
    finally:
        lib.s2vt_prof_enable(0)
        lib.s2vt_prof_reset()
    capi.check_async_error()
    return n


def _check_against_reference(m, ref, mode):
    errs = {}
    for n, p in m.named_parameters():
        r = ref[n]
        errs[n] = float((p.grad.double() - r).norm() / r.norm().clamp_min(1e-30))
    print("max relative error %.3g (%s, bound %g)" % (max(errs.values()), max(errs, key=errs.get), TOL[mode]))
    bad = {n: e for n, e in errs.items() if not e <= TOL[mode]}
    assert not bad, ("relative Frobenius error above %g" % TOL[mode], bad)
    return errs


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gradient_groups_are_final_when_released(lib, case):
    from s2vt_video_caption_amd import capi, dp
    name, d, opts, exp = case
    seed = 5
    dropout = exp.get("dropout", 0.0)
    with _options(lib, **opts):
        sd, feats, caps, mask = _inputs(d, seed)
        m = _model(d, sd, dropout)
        red = dp.FlatGradAllReducer(m.parameters()).attach(m)
        # the schedule this case names
        Bp = int(lib.s2vt_padded_batch(d["B"]))
        assert capi.recurrence_plan(d["B"], d["H"])[1] == exp["bwd"], (name, capi.recurrence_plan(d["B"], d["H"]))
        if exp["sched"] == "fp32":
            assert Bp % 64 != 0 or lib.s2vt_set_gemm_mode(-1) == 0, "the case must take the non-plane driver"
        if exp["sched"] == "solo":
            R, stages = (d["L"] - 1) * Bp, _stages(d["L"], _balanced_block(d["L"], lib.s2vt_set_option(b"pipe_block", -1)))
            pieces = _wo_pieces(R, lib.s2vt_set_option(b"corun", -1))
            assert (pieces > stages) == exp["trailing"], (name, pieces, stages)
        finals = []
        for lanes in (2, 1):                    # side lane late, then the caller's stream late
            snaps = _step_and_snapshot(lib, m, red, feats, caps, mask, lanes, mask_seed=seed)
            for p, (lo, hi) in zip(red.params, red.slices):
                n = [k for k, q in m.named_parameters() if q is p][0]
                if n in snaps:
                    assert torch.equal(snaps[n], red.flat[lo:hi]), \
                        "%s (lane delay %d): gradient group %d released before %s was final" % (name, lanes, GROUP_OF(n), n)
            n_p, after = _order(lib)
            assert after == n_p, (name, n_p, after)
            assert (n_p > 0) == (exp["bwd"] != 0 and exp["sched"] != "lanes"), (name, n_p)
            finals.append(red.flat.clone())
        # determinism: the same step twice (under different delays) writes the same bits
        assert torch.equal(finals[0], finals[1]), name
        out_mask = None
        if dropout:
            torch.manual_seed(seed)
            out_mask = torch.nn.Dropout(dropout)(torch.ones(d["B"], d["L"] - 1, d["H"], device=DEV))
        ref = _reference(d, seed, out_mask)
        _check_against_reference(m, ref, exp["mode"])
        # co-run GEMMs beside one-layer persistent launches: present exactly in the co-run schedules
        nc = _corun_gemms(lib, m, feats, caps, mask, mask_seed=seed)
        if exp["sched"] == "solo":
            assert nc >= pieces + stages, (name, nc, pieces, stages)      # every dW_o piece + every block's dh1 GEMM
        elif exp["sched"] == "corun2":
            assert nc > 0, (name, nc)
        else:
            assert nc == 0, (name, nc)


def test_overlapped_all_reduce_sees_final_gradients(lib, monkeypatch):
    """dp.FlatGradAllReducer._all_reduce_overlapped itself, with dist.all_reduce replaced by a snapshot of its tensor on the
    communication stream: the exact stream / event sequence a data-parallel step uses must hand every collective final
    gradients, in the schedule with more dW_o pieces than BPTT stages (corun=1) and the side lane late."""
    from s2vt_video_caption_amd import capi, dp
    import utils
    d = _dims(64, 48, 256, 2000, **MID)
    seen = []

    def fake_all_reduce(t, op=None, group=None, async_op=False):
        seen.append((t.data_ptr(), t.numel(), t.clone()))        # on the current stream: the communication stream
    monkeypatch.setattr(dp.dist, "all_reduce", fake_all_reduce)
    with _options(lib, corun=1):
        sd, feats, caps, mask = _inputs(d, 5)
        m = _model(d, sd)
        red = dp.FlatGradAllReducer(m.parameters()).attach(m)
        red.comm_stream = torch.cuda.Stream(device=DEV, priority=-1)     # a hardware queue of its own (see _step_and_snapshot)
        assert red.world == 1
        capi.check(lib.s2vt_test_lane_delay(2, DELAY_US), "s2vt_test_lane_delay")
        try:
            m.train()
            logits = m(feats, targets=caps[:, :-1], mode="train")
            utils.MaskCriterion()(logits, caps, mask).backward()
            red._all_reduce_overlapped()
        finally:
            lib.s2vt_test_lane_delay(0, 0)
        torch.cuda.synchronize()
        capi.check_async_error()
        n_p, after = _order(lib)
        assert n_p > 0 and after == n_p, (n_p, after)
    base = red.flat.data_ptr()
    esz = red.flat.element_size()
    spans = sorted((lo, hi) for g in red.groups.values() for lo, hi in g)
    assert sorted(((p - base) // esz, (p - base) // esz + n) for p, n, _ in seen) == spans
    for p, n, snap in seen:
        lo = (p - base) // esz
        assert torch.equal(snap, red.flat[lo:lo + n]), "all-reduce of flat[%d:%d] read gradients that were not final" % (lo, lo + n)
    _check_against_reference(m, _reference(d, 5), "x3")


# ---- hipGraph cache keys: every option is in them
GRAPH_SWITCHES = [("corun", 3, 0), ("bptt_solo", 1, 0), ("pipe_block", 32, 128), ("persist_x3_bwd", 2, 0), ("cu_reserve", 0, 24)]


@pytest.mark.parametrize("opt,a,b", GRAPH_SWITCHES, ids=[s[0] for s in GRAPH_SWITCHES])
def test_graph_cache_follows_schedule_options(lib, opt, a, b):
    """Under s2vt_set_graph_mode(1), four Adam steps at option value a (captured, then replayed), then four at value b: the switch
    must capture anew (the cache key holds every option), and losses and parameters must be those of the eager run of the same
    sequence bit for bit - a replay of the schedule captured under a would differ (for corun and persist_x3_bwd the eager runs at
    a and b are checked to differ, so a stale replay is detectable)."""
    import utils
    from s2vt_video_caption_amd import capi, dp
    d = _dims(64, 48, 256, 2000, **MID)
    sd, feats, caps, mask = _inputs(d, 9)
    crit = utils.MaskCriterion()

    def run(graphs, values):
        lib.s2vt_set_graph_mode(1 if graphs else 0)
        m = _model(d, sd)
        opt_ = torch.optim.Adam(m.parameters(), lr=1e-3)
        losses, stats = [], []
        for v in values:
            with _options(lib, **{opt: v}):
                for _ in range(4):
                    losses.append(float(dp.train_step(m, crit, opt_, feats, caps, mask, None)))
                torch.cuda.synchronize()
                c, r = ctypes.c_int64(0), ctypes.c_int64(0)
                lib.s2vt_graph_stats(ctypes.byref(c), ctypes.byref(r))
                stats.append((c.value, r.value))
        capi.check_async_error()
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, stats

    try:
        c0, r0 = ctypes.c_int64(0), ctypes.c_int64(0)
        lib.s2vt_graph_stats(ctypes.byref(c0), ctypes.byref(r0))
        ref_losses, ref_sd, _ = run(False, (a, b))
        losses, got, stats = run(True, (a, b))
        # (under a the graphs may come from an earlier test with the same key and pointers: replayed, not captured)
        assert stats[0][1] > r0.value, "no graph replayed under value a"
        assert stats[1][0] > stats[0][0], "%s %d -> %d replayed the graph captured under the old value" % (opt, a, b)
        assert losses == ref_losses, (opt, losses, ref_losses)
        for k in ref_sd:
            assert torch.equal(got[k], ref_sd[k]), (opt, k)
        if opt in ("corun", "persist_x3_bwd"):
            only_a, only_a_sd, _ = run(False, (a, a))
            assert only_a != ref_losses or any(not torch.equal(only_a_sd[k], ref_sd[k]) for k in ref_sd), \
                "values a and b give the same bits: a stale replay would go unnoticed"
    finally:
        lib.s2vt_set_graph_mode(0)
