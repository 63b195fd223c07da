"""Time the row kernels of ce.hip - the three criteria forward + backward, the fused criterion backward (split_dual_kernel<3, true>)
and the top-20 fan-out behind s2vt_beam_step - at the workload's own shapes (128 x 79 rows, V = 12000; 640 beam rows) and at the
small shapes of the GPU tests that walk every path of them (tools, GPU box).  Seeded inputs; every line carries the first argument
as a tag, the median of 5 timed runs (HIP events) and the sha1 of every output tensor of every run: two library builds on one box
(S2VT_LIB, interleaved processes) compare for speed and for bit-equal results.
usage: [S2VT_LIB=<library>] python tools/bench_criterion.py [TAG]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2vt_video_caption_amd  # noqa
from s2vt_video_caption_amd import build, capi, ops, synth
from s2vt_video_caption_amd.functional import _ptr
from bench_sha import sha, show

TAG = sys.argv[1] if len(sys.argv) > 1 else "-"
if not os.environ.get("S2VT_LIB"):
    build.build()
lib = capi.load()
DEV = "cuda:0"


def timed(name, fn, inner=1, reps=5):
    """median over `reps` of the time of `inner` back-to-back calls (one warm-up); sha1 of every run's last result"""
    fn()
    torch.cuda.synchronize()
    ms, shas = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
        shas.append(sha(out))
    show(TAG, "%s: median %.4f ms (min %.4f, max %.4f; %d runs of %d)" % (name, statistics.median(ms), min(ms), max(ms), reps, inner), shas)


def r(g, *shape, k=1.0):
    return (torch.randn(*shape, generator=g) * k).to(DEV)


# ---- the criteria on the default stream: forward + materialised backward, then the fused backward's row-plane image
CRITERION_SHAPES = [(128, 79, 12000), (1, 2, 16388), (2, 3, 16384), (2, 3, 1028), (2, 3, 1027), (2, 3, 16388), (3, 4, 1027), (2, 3, 300)]
for B, Lm1, V in CRITERION_SHAPES:
    g = torch.Generator().manual_seed(B * 1000 + V)
    R = B * Lm1
    logits = r(g, R, V, k=3.0)
    target = torch.randint(0, V, (B, Lm1 + 1), generator=g).to(DEV)
    weight = torch.randn(B, Lm1 + 1, generator=g)
    weight[:, Lm1 // 2 + 2:] = 0.0
    weight = weight.to(DEV)
    mask = (weight != 0).float()
    gout = torch.tensor([1.7], dtype=torch.float32, device=DEV)
    lse, rowloss, out4 = torch.empty(R, device=DEV), torch.empty(R, device=DEV), torch.zeros(4, device=DEV)
    dlogits, g_ce = torch.empty_like(logits), torch.empty(1, device=DEV)
    inner = 50 if R > 1000 else 200                                      # (a timed run of 5 - 20 ms either way)
    what = "B=%d Lm1=%d V=%d" % (B, Lm1, V)

    def mean_ce():
        capi.check(lib.s2vt_mean_ce_forward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(lse), _ptr(rowloss), _ptr(out4), None), "fwd")
        capi.check(lib.s2vt_mean_ce_backward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(lse), _ptr(gout), _ptr(dlogits), None), "bwd")
        return [out4[:1], lse, dlogits]

    def mask_criterion():
        capi.check(lib.s2vt_mask_criterion_forward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(mask), mask.stride(0), _ptr(lse),
                                                   _ptr(rowloss), _ptr(out4), None), "fwd")
        capi.check(lib.s2vt_mask_criterion_backward(B, Lm1, _ptr(mask), mask.stride(0), _ptr(out4), _ptr(gout), _ptr(g_ce), None), "bwd")
        capi.check(lib.s2vt_mean_ce_backward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(lse), _ptr(g_ce), _ptr(dlogits), None), "bwd")
        return [out4[:3], g_ce, dlogits]

    def reward_criterion():
        capi.check(lib.s2vt_weighted_ce_forward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(weight), weight.stride(0), _ptr(lse),
                                                _ptr(rowloss), _ptr(out4), None), "fwd")
        capi.check(lib.s2vt_weighted_ce_backward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(weight), weight.stride(0), _ptr(lse),
                                                 _ptr(out4), _ptr(gout), _ptr(dlogits), None), "bwd")
        return [out4[:2], dlogits]

    def mean_ce_fwd():
        capi.check(lib.s2vt_mean_ce_forward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(lse), _ptr(rowloss), _ptr(out4), None), "fwd")
        return [out4[:1], lse]

    def mean_ce_bwd():
        capi.check(lib.s2vt_mean_ce_backward(B, Lm1, V, _ptr(logits), _ptr(target), target.stride(0), _ptr(lse), _ptr(gout), _ptr(dlogits), None), "bwd")
        return [dlogits]

    timed("%s mean CE fwd+bwd (loss, lse, dlogits)" % what, mean_ce, inner)
    if R > 1000:                                                        # (the workload's shape: the two halves on their own as well)
        timed("%s mean CE fwd alone (loss, lse)" % what, mean_ce_fwd, inner)
        timed("%s mean CE bwd alone (dlogits)" % what, mean_ce_bwd, inner)
    timed("%s MaskCriterion fwd+bwd (out3, g_ce, dlogits)" % what, mask_criterion, inner)
    timed("%s RewardCriterion fwd+bwd (out2, dlogits)" % what, reward_criterion, inner)
    mean_ce()                                                           # (lse and dlogits of the mean CE for the two routes below)
    ce = dict(lse=lse, target=target, Lm1=Lm1, gout=gout)
    timed("%s fused backward 'r' image" % what, lambda: ops.split_planes_dual(logits, 3, ce=ce)["r"], 10)
    timed("%s split of the materialised dlogits, 'r' image" % what, lambda: ops.split_planes_dual(dlogits, 3)["r"], 10)
capi.check_async_error()


# ---- top-20 behind s2vt_beam_step: the workload's step (R = 640, V = 12000), then every instantiation at the tests' small dims
def beam(B, L, F, H, E, V, R, S, seed, inner):
    g = torch.Generator().manual_seed(seed)
    sd = synth.make_state_dict(V, F, H, E, seed=13, out_scale=16.0)
    params = [sd[k].to(DEV) for k in capi.PARAM_KEYS]
    row_b = torch.randint(0, B, (R,), generator=g, dtype=torch.int32).to(DEV)
    row_state = torch.randint(0, S, (R,), generator=g, dtype=torch.int32).to(DEV)
    tok = torch.randint(0, V, (R,), generator=g, dtype=torch.int32).to(DEV)
    vid_h, vid_c, word_h, word_c = r(g, B, H, k=0.5), r(g, B, H, k=0.5), r(g, S, H, k=0.5), r(g, S, H, k=0.5)
    timed("R=%d V=%d H=%d beam_step (top_ix, top_lp)" % (R, V, H),
          lambda: list(ops.beam_step(params, (B, L, F, H, E, V), row_b, row_state, tok, vid_h, vid_c, word_h, word_c)[4:]), inner)


beam(128, 80, 4096, 1000, 1000, 12000, 640, 640, 7, 20)
for V in (20, 257, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385, 38400):
    beam(2, 4, 16, 16, 16, V, 5, 7, 8, 100)
capi.check_async_error()
