"""Time the launch-per-timestep cell kernels (lstm.hip, lstm_gemv.hip, gru.hip, lstm_stack.hip) and the decode / beam steps built
on them, at H = E = 1000, V = 12000, T = 159 (tools, GPU box).  Seeded inputs; every line carries the first argument as a tag, the
median of 5 timed runs (HIP events) and the sha1 of every output tensor of every run: two library builds on one box (S2VT_LIB,
interleaved processes) compare for speed and for bit-equal results.
usage: [S2VT_LIB=<library>] python tools/bench_step_kernels.py [TAG]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2vt_video_caption_amd  # noqa
from s2vt_video_caption_amd import build, capi, ops, synth
from bench_sha import sha, show

TAG = sys.argv[1] if len(sys.argv) > 1 else "-"
if not os.environ.get("S2VT_LIB"):
    build.build()
capi.load()
DEV = "cuda:0"
T, H, E, V = 159, 1000, 1000, 12000


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


# ---- whole layers: LSTM (B = 64, 128), GRU (B = 64), a chain of 2 (B = 64)
for B in (64, 128):
    g = torch.Generator().manual_seed(3)
    gx, bias, w = r(g, 80 * B, 4 * H), r(g, 4 * H, k=0.3), r(g, 4 * H, H, k=H ** -0.5)
    gates, c_all, dh = torch.sigmoid(r(g, T * B, 4 * H)), r(g, T * B, H, k=0.7), r(g, T * B, H, k=0.1)
    timed("B=%d lstm_seq_fwd" % B, lambda: ops.lstm_seq_fwd(T, B, gx.clone(), 80, bias, w, want_stash=True))
    timed("B=%d lstm_seq_bwd" % B, lambda: ops.lstm_seq_bwd(T, B, w, dh, 0, c_all, gates.clone()))
B = 64
g = torch.Generator().manual_seed(4)
gx3, b_ih, b_hh, w3 = r(g, 80 * B, 3 * H), r(g, 3 * H, k=0.3), r(g, 3 * H, k=0.3), r(g, 3 * H, H, k=H ** -0.5)
dh = r(g, T * B, H, k=0.1)
timed("B=64 gru_seq_fwd", lambda: ops.gru_seq_fwd(T, B, gx3, 80, b_ih, w3, b_hh, want_stash=True))
h_all, stash = ops.gru_seq_fwd(T, B, gx3, 80, b_ih, w3, b_hh, want_stash=True)
timed("B=64 gru_seq_bwd", lambda: ops.gru_seq_bwd(T, B, w3, dh, 0, h_all, stash))

g = torch.Generator().manual_seed(5)
x_in = r(g, T * B, H)
layers = [dict(w_hh=r(g, 4 * H, H, k=H ** -0.5), w_in=r(g, 4 * H, H, k=H ** -0.5), bias=r(g, 4 * H, k=0.3), x_in=x_in if j == 0 else None,
               h=torch.empty(T * B, H, device=DEV), c=torch.empty(T * B, H, device=DEV), stash=torch.empty(T * B, 4 * H, device=DEV))
          for j in range(2)]


def chain_fwd():
    ops.lstm_chain_fwd(T, B, H, layers)
    return [t for l in layers for t in (l["h"], l["c"], l["stash"])]


timed("B=64 lstm_chain_fwd N=2", chain_fwd)
blayers = [dict(l, dg=torch.empty(T * B, 4 * H, device=DEV)) for l in layers]
blayers[0].update(x_in=None, w_in=None)
blayers[-1].update(dh_ext=dh, dh_t0=0)


def chain_bwd():
    ops.lstm_chain_bwd(T, B, H, blayers)
    return [l["dg"] for l in blayers]


timed("B=64 lstm_chain_bwd N=2", chain_bwd)

# ---- the token step of each of the four kernels (packed argmax words)
g = torch.Generator().manual_seed(6)
emb, w_ih, w_hh = r(g, V, E), r(g, 4 * H, E + H, k=(E + H) ** -0.5), r(g, 4 * H, H, k=H ** -0.5)
for Bt, what in ((64, "tile"), (4, "gemv")):
    gxt, hp, cp = r(g, Bt, 4 * H), r(g, Bt, H, k=0.5), r(g, Bt, H, k=0.5)
    tok = torch.randint(0, V, (Bt,), generator=g)
    packed = ((torch.arange(Bt, dtype=torch.int64) + 1234) << 32 | (0xFFFFFFFF - tok)).to(DEV)
    timed("B=%d lstm token step (%s)" % (Bt, what), lambda: ops.lstm_step_fwd_token(gxt, w_hh, hp, cp, emb, w_ih, tok_packed=packed), inner=50)
    if Bt == 64:
        gxg, w3i = r(g, Bt, 3 * H), r(g, 3 * H, E + H, k=(E + H) ** -0.5)
        timed("B=64 gru token step", lambda: ops.gru_step_fwd_token(gxg, w3, b_hh, hp, emb, w3i, tok_packed=packed), inner=50)
        xv = r(g, Bt, H)
        lay = [dict(w_hh=w_hh, bias=bias, h0=hp, c0=cp, h=torch.empty(Bt, H, device=DEV), c=torch.empty(Bt, H, device=DEV), x_in=xv,
                    w_in=w_ih[:, E:], emb=emb, w_e=w_ih, E=E, V=V, tok_const=0, tok_packed=packed)]

        def chain_tok():
            ops.lstm_chain_fwd(1, Bt, H, lay)
            return [lay[0]["h"], lay[0]["c"]]
        timed("B=64 chain token step (one layer-step)", chain_tok, inner=50)
capi.check_async_error()

# ---- decode argmax step, beam step (the size of tests/test_gpu_kernels.py::test_beam_step_at_config5_size)
g = torch.Generator().manual_seed(7)
h, w_out, b_out = r(g, 64, H, k=0.5), r(g, V, H, k=H ** -0.5), r(g, V, k=0.3)
timed("B=64 decode_step_argmax", lambda: ops.decode_step_argmax(h, w_out, b_out), inner=50)
Bb, L, F, R = 128, 80, 4096, 640
sd = synth.make_state_dict(V, F, H, E, seed=13, out_scale=16.0)
params = [sd[k].to(DEV) for k in capi.PARAM_KEYS]
row_b = torch.arange(Bb, dtype=torch.int32).repeat_interleave(5).to(DEV)
row_state = torch.randperm(R, generator=g).to(torch.int32).to(DEV)
tokb = torch.randint(0, V, (R,), generator=g, dtype=torch.int32).to(DEV)
vid_h, vid_c, word_h, word_c = r(g, Bb, H, k=0.5), r(g, Bb, H, k=0.5), r(g, R, H, k=0.5), r(g, R, H, k=0.5)
timed("R=640 beam_step", lambda: ops.beam_step(params, (Bb, L, F, H, E, V), row_b, row_state, tokb, vid_h, vid_c, word_h, word_c), inner=5)
