"""Generate tests/golden/*.npz by running the REFERENCE itself (read-only import from
/root/reference) and pin the oracle against it.  TEST INFRASTRUCTURE ONLY.

Run in the build container only (the reference does not travel):
    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden.py [tiny c1 c2 c2beam]

What is stored are inputs' seeds and the reference's OUTPUTS (data), never its source.
Inputs/weights are re-created from `s2vt_video_caption_amd.synth` by seed.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from s2vt_video_caption_amd import synth          # noqa: E402
from oracle import s2vt_oracle as orc             # noqa: E402

REF = "/root/reference"
GOLD = os.path.join(ROOT, "tests", "golden")


def _reference():
    sys.path.insert(0, REF)
    # the repo root also holds drop-in modules called S2VTModel / utils: make sure the
    # REFERENCE's files win for this script.
    for name in ("S2VTModel", "utils"):
        sys.modules.pop(name, None)
    import importlib.util
    mods = {}
    for name in ("S2VTModel", "utils"):
        spec = importlib.util.spec_from_file_location("_ref_" + name, os.path.join(REF, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["S2VTModel"].S2VT, mods["utils"].MaskCriterion


def _ref_model(S2VT, d, sd):
    m = S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(sd)
    return m


def _ref_train(S2VT, Crit, d, sd, feats, caps, mask, n_steps, lr=1e-4):
    m = _ref_model(S2VT, d, sd)
    crit = Crit()
    opt = torch.optim.Adam(m.parameters(), lr=lr)              # train.py:89-93
    losses, grads, logits0 = [], None, None
    for s in range(n_steps):                                   # train.py:116-127
        opt.zero_grad()
        m.train()
        probs = m(feats, targets=caps[:, :-1], mode="train")
        loss = crit(probs, caps, mask)
        loss.backward()
        if s == 0:
            logits0 = probs.detach().clone()
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        opt.step()
        losses.append(float(loss))
    return losses, grads, logits0, {k: v.detach().clone() for k, v in m.state_dict().items()}


def _margins(S2VT, d, sd, feats):
    """greedy ids from the reference + top-2 logit margins (from the oracle's replay)."""
    m = _ref_model(S2VT, d, sd)
    m.eval()
    with torch.no_grad():
        ids = m(feats, mode="test")
    oids, marg = orc.greedy_decode(sd, feats, return_margins=True)
    return ids, oids, marg


def screen(cfg, seeds, target=1e-3, beam_b=None, beam_width=5, max_scale=64.0, fixed_scale=None, stop=None):
    """Fixture screening (SURVEY.md §7 "Bit-exact token ids").  For every candidate seed: the smallest top-2 logit margin
    of the greedy decode at out_scale = 1 (oracle), the smallest power-of-two `out_scale` that lifts it to >= `target`
    (greedy ids do not depend on out_scale: out_linear's weight and bias are scaled together), and - with `beam_b` - the
    smallest score gap any decision of the beam search rests on AT that out_scale.  The first seed whose margin and gap
    both reach `target` (`stop`, if given) with out_scale <= max_scale (or at `fixed_scale`) wins, otherwise the best one.
    Scaling out_linear scales logits, margins AND any implementation's rounding differences alike, so out_scale only
    restates the margin in absolute terms (and sharpens the otherwise near-uniform softmax the beam search ranks): what
    protects the token ids is the margin RELATIVE to the logits, which is what the seed is screened for.
    Returns (seed, out_scale)."""
    d = dict(synth.CONFIGS[cfg])
    if beam_b:
        d["B"] = beam_b
    best = None
    for seed in seeds:
        sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed)
        feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
        t0 = time.time()
        _, marg = orc.greedy_decode(sd, feats, return_margins=True)
        mm = marg.min().item()
        scale = fixed_scale or 1.0
        while fixed_scale is None and mm * scale < target and scale < max_scale:
            scale *= 2.0
        gap = float("inf")
        if beam_b and mm * scale >= target:
            sds = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=scale)
            _, gap = orc.beam_search(sds, feats, beam_width=beam_width, max_depth=30, return_gap=True)
        print(f"[screen {cfg}] seed={seed} min top-2 margin(out_scale 1)={mm:.3e} out_scale={scale:g} "
              f"min beam gap={gap:.3e} ({time.time()-t0:.1f}s)", flush=True)
        score = min(mm * scale, gap)
        if best is None or score > best[0]:
            best = (score, seed, scale)
        if score >= (stop or target):
            break
    print(f"[screen {cfg}] chose seed={best[1]} out_scale={best[2]:g} (weakest decision {best[0]:.3e})", flush=True)
    return best[1], best[2]


C5_CHOICE = (298, 32.0)     # screen("c5", range(200, 330), beam_b=4, beam_width=5, fixed_scale=32): weakest decision 1.2e-3


def gen(name, seed, n_steps, out_scale, do_beam, beam_b=None, beam_width=3, full=False, greedy=True):
    S2VT, Crit = _reference()
    d = synth.CONFIGS[name]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=out_scale)
    feats, caps, mask = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
    out = dict(seed=seed, out_scale=out_scale, n_steps=n_steps,
               dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64))
    t0 = time.time()
    losses, grads, logits0, final = _ref_train(S2VT, Crit, d, sd, feats, caps, mask, n_steps)
    print(f"[{name}] reference train x{n_steps}: {time.time()-t0:.1f}s losses={losses}")
    o_losses, o_grads, o_final = orc.train_steps(sd, feats, caps, mask, n_steps)
    o_logits = orc.forward_train(sd, feats, caps[:, :-1])
    print(f"[{name}] oracle    losses={o_losses}")
    err = (o_logits - logits0).abs().max().item()
    print(f"[{name}] oracle-vs-reference max|dlogits|={err:.3e}")
    assert err < 5e-5, err
    for k in grads:      # fp32 summation order differs (oneDNN vs explicit loops): bound relative to the gradient's norm
        ge = (o_grads[k] - grads[k]).double().norm().item()
        gs = grads[k].double().norm().item()
        assert ge <= 1e-4 * gs + 1e-9, (k, ge, gs)
    assert max(abs(a - b) for a, b in zip(losses, o_losses)) < 2e-5
    out["losses"] = np.array(losses, dtype=np.float64)
    if full:
        out["logits"] = logits0.numpy()
        for k, g in grads.items():
            out["grad/" + k] = g.numpy()
        for k, g in final.items():
            out["final/" + k] = g.numpy()
    else:
        out["logits_rows"] = logits0[:, ::13, :64].contiguous().numpy()     # a thin slice
        out["logits_sum"] = np.array(logits0.double().sum().item())
        out["logits_abs_sum"] = np.array(logits0.double().abs().sum().item())
        for k, g in grads.items():
            out["gradnorm/" + k] = np.array(g.double().norm().item())
            out["gradsum/" + k] = np.array(g.double().sum().item())
            out["gradhead/" + k] = g.reshape(-1)[:32].numpy()
        for k, g in final.items():
            out["finalnorm/" + k] = np.array(g.double().norm().item())
    if greedy:
        t0 = time.time()
        ids, oids, marg = _margins(S2VT, d, sd, feats)
        print(f"[{name}] greedy: {time.time()-t0:.1f}s  oracle==reference: {bool((ids == oids).all())} "
              f"min margin={marg.min().item():.3e} p1={marg.flatten().kthvalue(max(1, marg.numel()//100)).values.item():.3e}")
        assert (ids == oids).all()
        out["greedy_ids"] = ids.numpy()
        out["greedy_margin"] = marg.numpy()
    if do_beam:
        bb = beam_b or d["B"]
        m = _ref_model(S2VT, d, sd)
        m.eval()
        t0 = time.time()
        with torch.no_grad():
            ref_beam = m(feats[:bb], mode="beam_search", beam_width=beam_width, max_beam_depth=30)
        ref_beam = [[int(t.item()) for t in s] for s in ref_beam]
        print(f"[{name}] reference beam(bw={beam_width}, B={bb}): {time.time()-t0:.1f}s lens={[len(s) for s in ref_beam]}")
        o_beam = orc.beam_search(sd, feats[:bb], beam_width=beam_width, max_depth=30)
        assert o_beam == ref_beam, (o_beam, ref_beam)
        mx = max(len(s) for s in ref_beam)
        arr = -np.ones((bb, mx), dtype=np.int64)
        for i, s in enumerate(ref_beam):
            arr[i, :len(s)] = s
        out["beam_ids"] = arr
        out["beam_width"] = np.array(beam_width)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] wrote {os.path.join(GOLD, name + '.npz')}")
    return S2VT, d, sd


def gen_long(name="c1long", cfg="c1", seed=31, n_steps=40, lr=1e-3):
    """A LONG loss trajectory of the reference on one fixed batch (40 Adam steps at a ten times larger learning rate than
    train.py's, so that the weights really move: the loss falls by an order of magnitude): every later step runs on weights
    that carry the rounding history of all earlier ones."""
    S2VT, Crit = _reference()
    d = synth.CONFIGS[cfg]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed)
    feats, caps, mask = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
    t0 = time.time()
    losses, _, _, final = _ref_train(S2VT, Crit, d, sd, feats, caps, mask, n_steps, lr=lr)
    print(f"[{name}] reference train x{n_steps} (lr {lr}): {time.time()-t0:.1f}s first {losses[0]:.4f} last {losses[-1]:.4f}")
    out = dict(seed=seed, out_scale=1.0, n_steps=n_steps, lr=lr, dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64),
               losses=np.array(losses, dtype=np.float64))
    for k, g in final.items():
        out["finalnorm/" + k] = np.array(g.double().norm().item())
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] wrote {os.path.join(GOLD, name + '.npz')}")


ATT_CONFIGS = {"att_tiny": dict(B=5, L=8, F=48, H=32, E=24, V=60, seed=3, full=True),
               "att_mid": dict(B=16, L=20, F=256, H=128, E=96, V=300, seed=4, full=False),
               # the reference's OWN size (train.py:20-48 defaults as committed upstream: batch 16, 80 frames of 4096 features,
               # dim_hidden = dim_embed = 512; vocabulary of the order of MSVD's): round-3 verdict, weak #3
               "att_full": dict(B=16, L=80, F=4096, H=512, E=512, V=12000, seed=5, full=False)}


def gen_att(name):
    """The reference's SECOND network, Att_Baseline (attention_baseline.py:9-105; what its committed train.py instantiates):
    one train forward + MaskCriterion loss + backward and one greedy decode of the reference itself on seeded inputs.  Stored:
    the seeded default initialisation (arrays for the tiny case, the seed for the larger one - the drop-in creates its
    parameter containers in the reference's order, checked here), logits, loss, every parameter's gradient (full / norm +
    head), greedy ids and the top-2 margin of every decision."""
    import importlib.util
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("_ref_attention_baseline", os.path.join(REF, "attention_baseline.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    _, Crit = _reference()
    d = ATT_CONFIGS[name]
    torch.manual_seed(d["seed"])
    m = ref.Att_Baseline(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    feats, caps, mask = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=900 + d["seed"])
    m.train()
    logits = m(feats, targets=caps[:, :-1], mode="train")
    loss = Crit()(logits, caps, mask)
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    m.eval()
    with torch.no_grad():
        ids = m(feats, mode="test")
        # replay of the greedy loop on the reference's own sub-modules for the margins (attention_baseline.py:85-104)
        x = m.feat_linear(feats)
        enc, _ = m.encoder(x)
        ctxv = enc.sum(dim=1, keepdim=True)             # softmax over a size-one dimension: all weights 1
        tok = torch.full((d["B"],), m.sos_ix, dtype=torch.long)
        state, rid, marg = None, [], []
        for _ in range(d["L"]):
            out, state = m.decoder(torch.cat([m.embedding(tok).unsqueeze(1), ctxv], dim=2), state)
            pr = m.out_linear(out)[:, 0]
            top = pr.topk(2, dim=1).values
            marg.append(top[:, 0] - top[:, 1])
            tok = pr.argmax(dim=1)
            rid.append(tok)
        assert torch.equal(torch.stack(rid, 1), ids), "replay of the reference's greedy loop differs from the reference"
    # the drop-in's seeded default initialisation must equal the reference's (same containers in the same order)
    spec2 = importlib.util.spec_from_file_location("_mine_attention_baseline", os.path.join(ROOT, "attention_baseline.py"))
    mine = importlib.util.module_from_spec(spec2)        # the repo's drop-in, loaded by path (REF is in front on sys.path)
    spec2.loader.exec_module(mine)
    torch.manual_seed(d["seed"])
    mm = mine.Att_Baseline(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    for k, v in mm.state_dict().items():
        assert torch.equal(v, sd[k]), k
    out = dict(seed=d["seed"], dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64), loss=np.array(float(loss)),
               keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]),
               ids=ids.numpy(), margins=torch.stack(marg, 1).numpy())
    if d["full"]:
        out["logits"] = logits.detach().numpy()
        for k, v in sd.items():
            out["param/" + k] = v.numpy()
    else:
        out["logits_rows"] = logits.detach()[:, ::3, :64].contiguous().numpy()
        out["logits_abs_sum"] = np.array(logits.detach().double().abs().sum().item())
    for k, g in grads.items():
        assert g is not None, k                           # the attention layers get zeros, not None
        out["gradnorm/" + k] = np.array(g.double().norm().item())
        out["gradhead/" + k] = g.reshape(-1)[:32].numpy()
        if d["full"]:
            out["grad/" + k] = g.numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(f"[{name}] loss {float(loss):.6f}, weakest greedy top-2 margin {float(torch.stack(marg,1).min()):.3e}, "
          f"att grad norms {[float(grads[k].norm()) for k in grads if k.startswith('att_')]}; wrote {name}.npz")


def gen_beam_only(name, cfg, seed, beam_b, beam_width, out_scale=1.0):
    """BASELINE config 5 dims (H=E=1000, V=12000), a few samples: reference beam-search ids (beam 5, depth 30) and
    greedy ids; the reference needs ~16 s per caption on CPU, so only `beam_b` samples are generated."""
    S2VT, _ = _reference()
    d = dict(synth.CONFIGS[cfg]); d["B"] = beam_b
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=out_scale)
    feats, caps, mask = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
    m = _ref_model(S2VT, d, sd)
    m.eval()
    t0 = time.time()
    with torch.no_grad():
        ref_beam = m(feats, mode="beam_search", beam_width=beam_width, max_beam_depth=30)
        ids = m(feats, mode="test")
    ref_beam = [[int(t.item()) for t in s] for s in ref_beam]
    print(f"[{name}] reference beam(bw={beam_width}, B={beam_b}): {time.time()-t0:.1f}s")
    o_beam, gap = orc.beam_search(sd, feats, beam_width=beam_width, max_depth=30, return_gap=True)
    assert o_beam == ref_beam, (o_beam, ref_beam)
    oids, marg = orc.greedy_decode(sd, feats, return_margins=True)
    assert (ids == oids).all()
    print(f"[{name}] weakest greedy top-2 margin {marg.min().item():.3e}, weakest beam decision gap {gap:.3e}")
    mx = max(len(s) for s in ref_beam)
    arr = -np.ones((beam_b, mx), dtype=np.int64)
    for i, s in enumerate(ref_beam):
        arr[i, :len(s)] = s
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), seed=seed, out_scale=out_scale, beam_width=np.array(beam_width),
                        beam_min_gap=np.array(gap),
                        dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64), beam_ids=arr, greedy_ids=ids.numpy(),
                        greedy_margin=marg.numpy())
    print(f"[{name}] wrote {name}.npz; oracle beam == reference beam")


C5FULL_CHOICE = (460, 16.0)   # screen_c5full(range(400, 640)): seed 460 has the widest weakest greedy margin of 240 seeds (2.6e-4 at out_scale 1: no row below 1e-4);
                                # out_scale 16: 1 of 128 beam searches rests on a score gap below 1e-5 (oracle replay), 7 below 3e-5


def screen_c5full(seeds, scales=(1.0, 2.0, 4.0, 8.0)):
    """Screening for the B=128 fixture of BASELINE configs[4]: per seed the smallest greedy top-2 margin over all 128 x 79
    decisions at out_scale 1 (oracle) and the number of rows whose weakest margin is below 1e-4 / 3e-5."""
    d = dict(synth.CONFIGS["c5"])
    for seed in seeds:
        sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed)
        feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
        _, marg = orc.greedy_decode(sd, feats, return_margins=True)
        rm = marg.min(dim=1).values
        print(f"[screen c5full] seed={seed} min margin={marg.min().item():.3e} rows<1e-4: {int((rm < 1e-4).sum())} "
              f"rows<3e-5: {int((rm < 3e-5).sum())}", flush=True)


def _c5full_beam_worker(job):
    """One worker = the reference's beam_search (S2VTModel.py:149-240) on rows [lo, hi) of the B=128 batch.  The encoder part
    of forward(mode='beam_search') (:56-60) runs on the FULL batch in every worker (one thread: the same numbers everywhere);
    only the per-sample Python search - 16 s per caption - is divided, by handing the reference's own method a slice of the
    states it was called with."""
    seed, out_scale, lo, hi, beam_width = job
    torch.set_num_threads(1)
    S2VT, _ = _reference()
    d = synth.CONFIGS["c5"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=out_scale)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
    m = _ref_model(S2VT, d, sd)
    m.eval()
    search = m.beam_search

    def rows_only(state1, state2, **kw):
        return search(tuple(x[:, lo:hi].contiguous() for x in state1), tuple(x[:, lo:hi].contiguous() for x in state2), **kw)
    m.beam_search = rows_only
    with torch.no_grad():
        out = m(feats, mode="beam_search", beam_width=beam_width, max_beam_depth=30)
    return lo, [[int(t.item()) for t in s] for s in out]


def gen_c5full(seed, out_scale, beam_width=5, workers=6, name="c5full"):
    """BASELINE configs[4] at its own size: B=128, beam 5, depth 30 (S2VTModel.py:56-61,149-240; eval.py:81-96) and the greedy
    decode of the same batch (S2VTModel.py:82-110), both from the REFERENCE (one CPU thread), with the per-row weakest top-2
    margin of the greedy decode and the per-sample weakest decision gap of the beam search (oracle replay) stored beside the
    ids so that a test can tell a wrong id from a legitimately flipped near-tie."""
    import multiprocessing as mp
    torch.set_num_threads(1)
    S2VT, _ = _reference()
    d = synth.CONFIGS["c5"]
    B = d["B"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=out_scale)
    feats, _, _ = synth.make_batch(B, d["L"], d["F"], d["V"], seed=1234 + seed)
    t0 = time.time()
    m = _ref_model(S2VT, d, sd)
    m.eval()
    with torch.no_grad():
        ids = m(feats, mode="test")
    print(f"[{name}] reference greedy B={B}: {time.time()-t0:.1f}s", flush=True)
    step = (B + workers - 1) // workers
    jobs = [(seed, out_scale, lo, min(lo + step, B), beam_width) for lo in range(0, B, step)]
    t0 = time.time()
    with mp.get_context("spawn").Pool(len(jobs)) as pool:
        parts = dict(pool.map(_c5full_beam_worker, jobs))
    ref_beam = [s for lo in sorted(parts) for s in parts[lo]]
    assert len(ref_beam) == B
    print(f"[{name}] reference beam(bw={beam_width}, B={B}) in {len(jobs)} workers: {time.time()-t0:.1f}s", flush=True)
    torch.set_num_threads(8)
    oids, marg = orc.greedy_decode(sd, feats, return_margins=True)
    o_beam, gaps = orc.beam_search(sd, feats, beam_width=beam_width, max_depth=30, return_gap="per_sample")
    g_same = (ids == oids).all(dim=1).numpy()
    b_same = np.array([a == b for a, b in zip(o_beam, ref_beam)])
    rm = marg.min(dim=1).values.numpy()
    gaps = np.array(gaps, dtype=np.float64)
    print(f"[{name}] oracle == reference: greedy rows {int(g_same.sum())}/{B}, beam rows {int(b_same.sum())}/{B}")
    print(f"[{name}] weakest greedy margin {rm.min():.3e} (rows < 1e-4: {int((rm < 1e-4).sum())}); weakest beam gap "
          f"{gaps.min():.3e} (rows < 1e-4: {int((gaps < 1e-4).sum())}, < 3e-5: {int((gaps < 3e-5).sum())})")
    # the oracle may only differ from the reference where the recorded margin says a rounding difference can decide
    assert all(rm[i] < 1e-4 for i in np.nonzero(~g_same)[0]), rm[~g_same]
    assert all(gaps[i] < 1e-4 for i in np.nonzero(~b_same)[0]), gaps[~b_same]
    mx = max(len(s) for s in ref_beam)
    arr = -np.ones((B, mx), dtype=np.int64)
    for i, s in enumerate(ref_beam):
        arr[i, :len(s)] = s
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), seed=seed, out_scale=out_scale, beam_width=np.array(beam_width),
                        dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64), beam_ids=arr, beam_gap=gaps,
                        beam_oracle_equal=b_same, greedy_ids=ids.numpy(), greedy_margin=marg.numpy().astype(np.float32),
                        greedy_oracle_equal=g_same)
    print(f"[{name}] wrote {name}.npz")


def gen_c5raw(seed, name="c5raw"):
    """The UNSCALED companion of c5full (round-3 verdict, weak #2): the reference's greedy decode of the same B=128 batch with the
    recipe's weights as they are (out_scale 1: logit margins of the size random-init weights really give, weakest 2.6e-4 for this
    seed), ids + per-decision top-2 margins.  The GPU test compares every row whose weakest margin is >= 1e-4."""
    S2VT, _ = _reference()
    d = synth.CONFIGS["c5"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed, out_scale=1.0)
    feats, _, _ = synth.make_batch(d["B"], d["L"], d["F"], d["V"], seed=1234 + seed)
    m = _ref_model(S2VT, d, sd)
    m.eval()
    with torch.no_grad():
        ids = m(feats, mode="test")
    oids, marg = orc.greedy_decode(sd, feats, return_margins=True)
    rm = marg.min(dim=1).values.numpy()
    same = (ids == oids).all(dim=1).numpy()
    assert all(rm[i] < 1e-4 for i in np.nonzero(~same)[0]), rm[~same]
    print(f"[{name}] oracle == reference on {int(same.sum())}/{d['B']} rows; weakest margin {rm.min():.3e}, rows < 1e-4: {int((rm < 1e-4).sum())}")
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), seed=seed, out_scale=1.0, dims=np.array([d[k] for k in "BLFHEV"], dtype=np.int64),
                        greedy_ids=ids.numpy(), greedy_margin=marg.numpy().astype(np.float32), greedy_oracle_equal=same)
    print(f"[{name}] wrote {name}.npz")


def gen_tiny_seed17(name="tiny_seed17", seed=17, B=4):
    """tests/test_oracle_golden.py::test_oracle_against_live_reference: the reference's train forward (logits) and greedy ids
    on the tiny dims at seed 17, B = 4 - checked against the oracle here as the test checks them."""
    S2VT, _ = _reference()
    d = synth.CONFIGS["tiny"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=seed)
    feats, caps, _ = synth.make_batch(B, d["L"], d["F"], d["V"], seed=seed)
    m = _ref_model(S2VT, d, sd)
    with torch.no_grad():
        logits = m(feats, targets=caps[:, :-1], mode="train")
        ids = m(feats, mode="test")
    err = (logits - orc.forward_train(sd, feats, caps[:, :-1])).abs().max().item()
    assert err < 2e-6 and torch.equal(ids, orc.greedy_decode(sd, feats)), err
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), seed=seed, dims=np.array([B] + [d[k] for k in "LFHEV"]),
                        logits=logits.numpy(), greedy_ids=ids.numpy())
    print(f"[{name}] oracle-vs-reference max|dlogits|={err:.3e}")


def gen_pickle():
    """A full-module pickle WRITTEN BY THE REFERENCE class (train.py:167-168 style) at tiny
    dims, to test that the drop-in S2VTModel.S2VT loads reference checkpoints."""
    sys.path.insert(0, REF)
    for name in ("S2VTModel",):
        sys.modules.pop(name, None)
    import importlib
    sys.path.insert(0, REF)
    ref_mod = importlib.import_module("S2VTModel")
    assert ref_mod.__file__.startswith(REF), ref_mod.__file__
    d = synth.CONFIGS["tiny"]
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=7)
    m = ref_mod.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"])
    m.load_state_dict(sd)
    torch.save(m, os.path.join(GOLD, "tiny_reference_module.pth"))
    sys.modules.pop("S2VTModel", None)
    sys.path.remove(REF)
    print("wrote tiny_reference_module.pth")


def check_early_stopping():
    """Pin oracle/train_oracle.py::EarlyStoppingOracle against the reference's own class (utils.py:29-80; `np.Inf` of
    NumPy < 2 is aliased so that it imports) on random validation-loss sequences."""
    import importlib.util
    import tempfile
    np.Inf = np.inf
    spec = importlib.util.spec_from_file_location("_ref_utils", os.path.join(REF, "utils.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    from oracle.train_oracle import EarlyStoppingOracle
    rng = np.random.RandomState(0)
    for trial in range(50):
        pat = int(rng.randint(1, 6))
        seq = list(np.round(rng.rand(30) * 0.2 + np.linspace(1, 0.8, 30) * (rng.rand() > 0.3), 3))
        with tempfile.TemporaryDirectory() as d:
            ref = m.EarlyStopping(patience=pat, verbose=False, path=os.path.join(d, "x.pt"), trace_func=lambda *a: None)
            mine = EarlyStoppingOracle(patience=pat)
            for v in seq:
                ref(v, torch.nn.Linear(1, 1))
                mine(v)
                assert (ref.counter, ref.early_stop, ref.best_score) == (mine.counter, mine.early_stop, mine.best_score)
                if ref.early_stop:
                    break
    print("EarlyStoppingOracle == reference EarlyStopping on 50 random sequences")


if __name__ == "__main__":
    torch.manual_seed(0)
    which = sys.argv[1:] or ["tiny", "c1"]
    os.makedirs(GOLD, exist_ok=True)
    if "es" in which:
        check_early_stopping()
    if "tiny" in which:
        gen("tiny", seed=7, n_steps=3, out_scale=1.0, do_beam=True, beam_width=3, full=True)
        gen_pickle()
    if "tiny17" in which:
        gen_tiny_seed17()
    if "c1" in which:
        gen("c1", seed=11, n_steps=3, out_scale=1.0, do_beam=True, beam_b=2, beam_width=5)
    # c2 / c5beam: (seed, out_scale) chosen by screen() so that the weakest decision of the reference's greedy decode
    # (and beam search) is >= 1e-3: screen("c2", range(100, 440)) -> seed 160 (smallest top-2 margin 6.5e-4 at out_scale 1,
    # the widest of 340 seeds), out_scale 2; screen("c5", range(200, 330), beam_b=4, fixed_scale=32) -> see C5_CHOICE
    if "c2" in which:
        gen("c2", seed=160, n_steps=2, out_scale=2.0, do_beam=False)
    if "c3" in which:     # BASELINE configs[2] shape (B=256): ONE fp32 reference train step; the bf16 GPU run is compared
        gen("c3", seed=5, n_steps=1, out_scale=1.0, do_beam=False, greedy=False)      # with it at bf16 bounds
    if "c4" in which:     # BASELINE configs[3]: the B=128 shard one GPU of the 8-way data-parallel run takes; two fp32 train steps
        gen("c4", seed=7, n_steps=2, out_scale=1.0, do_beam=False, greedy=False)
    if "c1long" in which:
        gen_long()
    if "mid64long" in which:
        gen_long("mid64long", "mid64", seed=41)
    for att in ("att_tiny", "att_mid", "att_full"):
        if att in which:
            gen_att(att)
    if "c2long" in which:   # BASELINE configs[1] (the headline) at its own size: 10 fp32 reference Adam steps (lr 1e-3) on one B=64
        gen_long("c2long", "c2", seed=7, n_steps=10)       # batch; the fp32-equivalent GPU trajectory must stay within 1e-4 of it
    if "c3long" in which:   # BASELINE configs[2] at its own size: 10 fp32 reference Adam steps (lr 1e-3) on one B=256 batch;
        gen_long("c3long", "c3", seed=5, n_steps=10)       # the bf16 GPU trajectory is compared with it step by step
    if "c5full" in which:
        gen_c5full(*C5FULL_CHOICE)
    if "c5raw" in which:
        gen_c5raw(C5FULL_CHOICE[0])
    if "c5rawbeam" in which:     # the UNSCALED beam fixture: the reference's 128 beam searches with the recipe's weights as they are
        gen_c5full(C5FULL_CHOICE[0], 1.0, name="c5rawbeam")
    if "c5beam" in which:
        gen_beam_only("c5beam", "c5", seed=C5_CHOICE[0], beam_b=4, beam_width=5, out_scale=C5_CHOICE[1])
