"""Generate tests/golden/stack*.npz from the REFERENCE's own S2VT with num_layers > 1 (S2VTModel.py:11-22: nn.LSTM(num_layers=N)
for vid_rnn and word_rnn), on CPU, from the seeded recipe synth.make_state_dict(num_layers=N) / synth.make_batch.  TEST
INFRASTRUCTURE ONLY: it needs a checkout of the reference next to it (--reference DIR) and is run where that checkout is, never on a
GPU machine.

What is stored are seeds, dimensions and the reference's OUTPUTS (data), never its source: the loss, a logits slice (+ sums),
every parameter gradient by norm / sum / leading entries (all of it for the tiny sizes), greedy ids of mode='test' and per-step
top-2 logit margins from an fp64 replay of the greedy loop (`replay_fp64`, below, needs no reference: tests/test_stack_host.py
re-runs it against the stored outputs), the number of rows whose margin is >= 1e-5 at every step, and at BASELINE configs[1] the
loss after each of ten torch.optim.Adam steps (lr 1e-3) on one batch with the final parameter norms.

  python tools/make_stack_golden.py --reference ../S2VT-video-caption [names...]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import s2vt_video_caption_amd  # noqa: E402,F401
from s2vt_video_caption_amd import synth  # noqa: E402
from make_gru_golden import MARGIN, _reference  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")

CONFIGS = {
    "stack_tiny": dict(N=2, B=4, L=8, F=64, H=24, E=16, V=50, seed=21, full=True),
    "stack3_tiny": dict(N=3, B=4, L=8, F=64, H=24, E=16, V=50, seed=22, full=True),
    # the reference's defaults (train.py Opt: batch 16, 80 frames of 4096 features, dim_hidden = dim_embed = 512)
    "stack_ref": dict(N=2, B=16, L=80, F=4096, H=512, E=512, V=3000, seed=23, full=False),
    # BASELINE configs[1]
    "stack_c2": dict(N=2, B=64, L=80, F=4096, H=1000, E=1000, V=12000, seed=24, full=False, long_steps=10),
    # a ragged batch (no multiple of 16) for the greedy decode
    "stack_ragged": dict(N=2, B=10, L=80, F=4096, H=512, E=512, V=3000, seed=25, full=False, greedy_only=True),
}


def setup(name):
    """(dims, state_dict, feats, caps, mask) of a fixture, from its seed alone."""
    d = CONFIGS[name]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=d["seed"], num_layers=d["N"])
    feats, caps, mask = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + d["seed"])
    return d, sd, feats, caps, mask


def _lstm_stack_step(x, state, p, prefix, N):
    """one step of an N-layer nn.LSTM in fp64: x [B, K], state = [(h, c)] * N"""
    new = []
    for k in range(N):
        h, c = state[k]
        g = x @ p["%s.weight_ih_l%d" % (prefix, k)].t() + p["%s.bias_ih_l%d" % (prefix, k)] + \
            h @ p["%s.weight_hh_l%d" % (prefix, k)].t() + p["%s.bias_hh_l%d" % (prefix, k)]
        H = h.shape[1]
        i, f, gg, o = g[:, :H].sigmoid(), g[:, H:2 * H].sigmoid(), g[:, 2 * H:3 * H].tanh(), g[:, 3 * H:].sigmoid()
        c = f * c + i * gg
        h = o * c.tanh()
        new.append((h, c))
        x = h
    return x, new


def replay_fp64(d, sd, feats, ids):
    """fp64 replay of mode='test' (S2VTModel.py:82-110) that follows the given ids: (its own argmax ids [B, L-1], top-2 logit
    margins [B, L-1]).  Pure torch on CPU; no reference import."""
    p = {k: v.double() for k, v in sd.items()}
    B, L, N = feats.shape[0], d["L"], d["N"]
    H, E = d["H"], d["E"]
    x = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    z = torch.zeros(B, H, dtype=torch.float64)
    sv, sw = [(z, z)] * N, [(z, z)] * N
    for t in range(L):
        v, sv = _lstm_stack_step(x[:, t], sv, p, "vid_rnn", N)
        _, sw = _lstm_stack_step(torch.cat([torch.zeros(B, E, dtype=torch.float64), v], 1), sw, p, "word_rnn", N)
    own, marg = [], []
    tok = torch.full((B,), 3, dtype=torch.long)
    for i in range(L - 1):
        if i:
            tok = ids[:, i - 1]
        v, sv = _lstm_stack_step(z, sv, p, "vid_rnn", N)
        o, sw = _lstm_stack_step(torch.cat([p["embedding.weight"][tok], v], 1), sw, p, "word_rnn", N)
        logits = o @ p["out_linear.weight"].t() + p["out_linear.bias"]
        top = logits.topk(2, dim=1).values
        own.append(logits.argmax(1))
        marg.append(top[:, 0] - top[:, 1])
    return torch.stack(own, 1), torch.stack(marg, 1)


def _ref_model(S2VT, d, sd):
    m = S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], num_layers=d["N"])
    m.load_state_dict(sd)
    return m


def _train(S2VT, Crit, d, sd, feats, caps, mask, n_steps, lr):
    m = _ref_model(S2VT, d, sd)
    crit = Crit()
    opt = torch.optim.Adam(m.parameters(), lr=lr)                     # train.py:89-93
    losses, grads, logits0 = [], None, None
    for s in range(n_steps):                                          # train.py:116-127
        opt.zero_grad()
        m.train()
        probs = m(feats, targets=caps[:, :-1], mode="train")
        loss = crit(probs, caps, mask)
        loss.backward()
        if s == 0:
            logits0 = probs.detach().clone()
            grads = {k: q.grad.detach().clone() for k, q in m.named_parameters()}
        opt.step()
        losses.append(float(loss))
    return losses, grads, logits0, {k: q.detach().clone() for k, q in m.state_dict().items()}


def gen(name, S2VT, Crit):
    d, sd, feats, caps, mask = setup(name)
    out = dict(seed=d["seed"], num_layers=d["N"], n_steps=1, dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64))
    if not d.get("greedy_only"):
        t0 = time.time()
        losses, grads, logits0, _ = _train(S2VT, Crit, d, sd, feats, caps, mask, 1, 1e-4)
        print(f"[{name}] reference train: {time.time() - t0:.1f}s loss={losses[0]:.6f}", flush=True)
        out["loss"] = np.array(losses[0])
        out["logits_rows"] = logits0[:, ::13, :64].contiguous().numpy()
        out["logits_sum"] = np.array(logits0.double().sum().item())
        if d["full"]:
            out["logits"] = logits0.numpy()
        for k, g in grads.items():
            out["gradnorm/" + k] = np.array(g.double().norm().item())
            out["gradsum/" + k] = np.array(g.double().sum().item())
            out["gradhead/" + k] = g.reshape(-1)[:32].numpy()
            if d["full"]:
                out["grad/" + k] = g.numpy()
    t0 = time.time()
    m = _ref_model(S2VT, d, sd).eval()
    with torch.no_grad():
        ids = m(feats, mode="test")
    own, marg = replay_fp64(d, sd, feats, ids)
    robust = (marg >= MARGIN).all(1)
    assert (own[robust] == ids[robust]).all(), "fp64 replay disagrees with the reference on a row with a wide margin"
    print(f"[{name}] greedy: {time.time() - t0:.1f}s robust rows {int(robust.sum())}/{d['B']} min margin {marg.min().item():.2e}",
          flush=True)
    out["greedy_ids"] = ids.numpy()
    out["greedy_margin"] = marg.numpy()
    out["n_robust_rows"] = np.array(int(robust.sum()))
    if d.get("long_steps"):
        n = d["long_steps"]
        t0 = time.time()
        losses, _, _, final = _train(S2VT, Crit, d, sd, feats, caps, mask, n, 1e-3)
        print(f"[{name}] reference Adam x{n}: {time.time() - t0:.1f}s {losses[0]:.4f} -> {losses[-1]:.4f}", flush=True)
        out["long_lr"] = np.array(1e-3)
        out["long_losses"] = np.array(losses, dtype=np.float64)
        for k, g in final.items():
            out["finalnorm/" + k] = np.array(g.double().norm().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] wrote", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (S2VTModel.py, utils.py)")
    ap.add_argument("names", nargs="*", default=list(CONFIGS))
    a = ap.parse_args()
    torch.manual_seed(0)
    S2VT, Crit = _reference(a.reference)
    for name in a.names:
        gen(name, S2VT, Crit)


if __name__ == "__main__":
    main()
