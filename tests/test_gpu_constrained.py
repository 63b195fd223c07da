"""GPU tests of constrained decoding (csrc/truncate.hip "constrained draw": repetition penalty, no-repeat n-gram, banned ids and a
minimum length inside the row kernel) from the row kernel up to S2VT.decode_constrained, the GRU / stacked step loops and eval.py.

The row kernel edits its logits IN PLACE, so its first check is bitwise: the buffer afterwards equals sampling.constrain_logits (the
definition restated in numpy, fp32 multiplications).  Whole decodes are checked by exact invariants of their ids and by a float64
teacher-forced replay ALONG THE DEVICE'S OWN IDS whose logits go through constrain_logits with the device's own history."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, ops, sampling, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_refs as refs  # noqa: E402
import test_constrained_host as hc  # noqa: E402
import test_sampling_host as hs  # noqa: E402
import test_truncated_host as ht  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS = 4


def _key(x):
    """the order-preserving 32-bit key of fp32 values (the high half of a packed word)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. the row kernel by value
@pytest.mark.parametrize("V", hc.KERNEL_V)
def test_row_kernel_leaves_the_constrained_row_and_picks_from_it(lib, V):
    """per (t, spec, rows): the logits buffer afterwards IS constrain_logits (bitwise; rows beyond `rows` untouched), the greedy id is
    numpy's arg-max of that row with its ordered key in the packed word, and the sampled draws (top_k = 5; nothing truncated) come
    from truncation_mask on the constrained row with exact `kept` - the inputs are multiples of 1/8, and so are their products with
    theta = 1.5 and r = fp32(2/3) only up to fp32 rounding, which numpy reproduces bit for bit"""
    x, h = hc.kernel_case(V)
    R, extra = x.shape[0], 2
    seed, step = 7000 + V, 3
    noise = sampling.gumbel_noise(seed, step, R, V)
    master = torch.cat([x, torch.full((extra, V), 0.375)]).to(DEV)
    buf = torch.empty_like(master)
    worst, n_blocked = 0.0, 0
    for t in hc.KERNEL_T:
        for sp in hc.kernel_specs(V, t):
            want = sampling.constrain_logits(x.numpy(), h.numpy(), t, sp)
            n_blocked += int(np.isneginf(want).sum())
            want64 = want.astype(np.float64)
            want_ids = want.argmax(1)
            want_dev = torch.cat([torch.from_numpy(want), torch.full((extra, V), 0.375)]).to(DEV)
            masks = {5: sampling.truncation_mask(want64, 5, 1.0), 0: np.ones(want.shape, dtype=bool)}
            for rows in hc.KERNEL_ROWS:
                hist = hc.pack_history(h[:rows, :t], rows + 3).to(DEV)
                expect = torch.cat([want_dev[:rows], master[rows:]])
                buf.copy_(master)
                ids, kept, packed = ops.constrained_draw(buf[:rows], hist, t, sp, greedy=True, return_kept=True, return_packed=True)
                assert torch.equal(_bits(buf), _bits(expect)), (t, sp, rows)
                ids, packed = ids.cpu().numpy(), packed.cpu().numpy()
                assert np.array_equal(ids, want_ids[:rows]), (t, sp, rows)
                assert np.array_equal((packed >> 32) & 0xFFFFFFFF, _key(want[np.arange(rows), ids])), (t, sp, rows)
                assert (kept.cpu().numpy() == V).all()
                for k, mask in masks.items():
                    buf.copy_(master)
                    ids, kept = ops.constrained_draw(buf[:rows], hist, t, sp, top_k=k, top_p=1.0, seed=seed, step=step, return_kept=True)
                    assert torch.equal(_bits(buf), _bits(expect)), (t, sp, rows, k)
                    assert np.array_equal(kept.cpu().numpy(), mask[:rows].sum(1)), (t, sp, rows, k)
                    worst = max(worst, ht.check_draws(want64[:rows] + noise[:rows], ids.cpu().numpy(), mask[:rows], mask[:rows], hs.NOISE_TOL))
    print("V=%d: %d blocked elements over the cases; largest float64 gap of a draw %.3g (tol %.3g)" % (V, n_blocked, worst, hs.NOISE_TOL))
    assert n_blocked > 0
    capi.check_async_error()


# ------------------------------------------------------------------ 2. nothing constrained is today's result
@pytest.mark.parametrize("V", [301, 12289])
def test_nothing_constrained_is_the_truncated_draw(lib, V):
    x, h = hc.kernel_case(V, seed=1)
    off = sampling.check_constraints(0, 1.0, 0, None, V, EOS)
    xd = x.to(DEV)
    for t in (0, 40):
        hist = hc.pack_history(h[:, :t], 73).to(DEV)
        for kw in (dict(), dict(top_k=5), dict(top_p=0.7), dict(top_k=20, top_p=0.9), dict(temperature=0.5, top_k=5)):
            buf = xd.clone()
            _, kept, packed = ops.constrained_draw(buf, hist, t, off, seed=11, step=t, row0=2, return_kept=True, return_packed=True, **kw)
            _, kept0, packed0 = ops.truncated_draw(xd, seed=11, step=t, row0=2, return_kept=True, return_packed=True, **kw)
            assert torch.equal(packed, packed0) and torch.equal(kept, kept0), (t, kw)
            assert torch.equal(_bits(buf), _bits(xd))
    capi.check_async_error()


# ------------------------------------------------------------------ 3. the whole decode, one-layer LSTM
DIMS = dict(L=12, F=64, E=40, V=301)
M_LEN = 6


def _model(d, sd, **kw):
    import S2VTModel
    m = S2VTModel.S2VT(d["V"], d["F"], d["L"], dim_hid=d["H"], dim_embed=d["E"], **kw)
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _lstm_case(H, B):
    d = dict(DIMS, B=B, H=H)
    sd = synth.make_state_dict(d["V"], d["F"], d["H"], d["E"], seed=21)
    feats, _, _ = synth.make_batch(B, d["L"], d["F"], d["V"], seed=22)
    return d, sd, feats


def _check_invariants(ids, shape, V, n=0, m=0, banned=()):
    assert ids.dtype == torch.int64 and tuple(ids.shape) == shape, (ids.dtype, ids.shape)
    a = ids.cpu().numpy().reshape(-1, shape[-1])
    assert a.min() >= 0 and a.max() < V
    if n:
        assert all(hc.ngram_repeats(r.tolist(), n) == 0 for r in a), "a repeated %d-gram" % n
    if m:
        assert not (a[:, :m] == EOS).any(), "<eos> among the first %d words" % m
    for b in banned:
        assert not (a == b).any(), "banned id %d generated" % b
    return a


# The tolerance of the value checks.  The device's logits and the float64 replay's differ by at most MARGIN (test_sampling_host: what
# the greedy tests grant the kernels' logits).  The constraints leave an untouched logit as it is, set a banned one to -inf on both
# sides (the history is the device's own on both sides), and MULTIPLY a penalised one: x * r with r < 1 shrinks the error, x * theta
# (x <= 0) scales it by theta.  Around x = 0 the two branches meet (both products go to 0), so a logit whose sign differs between the
# two sides is off by at most theta * MARGIN as well.  Hence every constrained logit is within theta * MARGIN, and so is every bound
# derived from MARGIN: the greedy gap, the sampled eps (MARGIN / t + NOISE_TOL) and the bracket's margins (test_gpu_truncated).
def _tol(theta):
    return hs.MARGIN * theta


def _replay_check(logits64, ids, spec, sample=None, rows=None):
    """logits64 float64 [R, S, V] teacher-forced along ids int64 [R, S]: at every step the device's word is a survivor of the
    constrained float64 row and within tolerance of its best (greedy), or inside the bracket of the truncated draw on it (sample =
    (temperature, seed, top_k)).  Returns the largest gap."""
    R, S, V = logits64.shape
    rows = np.arange(R) if rows is None else rows
    theta = spec.repetition_penalty
    worst = 0.0
    for j in range(S):
        xc = sampling.constrain_logits(logits64[:, j], ids, j, spec)
        got = xc[np.arange(R), ids[:, j]]
        assert np.isfinite(got).all(), "step %d: a banned word was generated" % j
        if sample is None:
            gap = xc.max(1) - got
            assert (gap <= _tol(theta)).all(), "step %d: float64 gap %.3g > %.3g" % (j, gap.max(), _tol(theta))
            worst = max(worst, float(gap.max()))
        else:
            t, seed, k = sample
            noise = sampling.gumbel_noise(seed, j, rows, V)
            lo, hi = ht.bracket(xc / t, k, 1.0, ht.DELTA + 2 * _tol(theta) / t, _tol(theta) / t)
            worst = max(worst, ht.check_draws(xc / t + noise, ids[:, j], lo, hi, _tol(theta) / t + hs.NOISE_TOL))
    return worst


def _cpu_constrained_greedy(sd, feats, spec, sos_ix=3):
    """float64 constrained greedy decode on the CPU: (ids [B, L-1], top-2 margins of the constrained rows [B, L-1])"""
    from oracle import s2vt_oracle as orc
    B, L, _ = feats.shape
    prefix = torch.zeros(B, L - 1, dtype=torch.long)
    prefix[:, 0] = sos_ix
    ids = np.zeros((B, L - 1), dtype=np.int64)
    marg = np.zeros((B, L - 1))
    for j in range(L - 1):
        with torch.no_grad():
            x = orc.forward_train(sd, feats, prefix, dtype=torch.float64)[:, j].numpy()
        xc = sampling.constrain_logits(x, ids, j, spec)
        ids[:, j] = xc.argmax(1)
        top = np.sort(xc, axis=1)
        marg[:, j] = top[:, -1] - top[:, -2]
        if j + 1 < L - 1:
            prefix[:, j + 1] = torch.from_numpy(ids[:, j])
    return ids, marg


def _logits_along(sd, feats, ids):
    """float64 logits [R, S, V] teacher-forced along the device's ids: test_sampling_host.scores_along_ids_fp64 at temperature 1
    less the noise it adds (the constraints apply to the raw logits; the difference is exact to ~1e-15)"""
    R, S = ids.shape
    V = sd["out_linear.weight"].shape[0]
    noise = np.stack([sampling.gumbel_noise(0, j, R, V) for j in range(S)], 1)
    return hs.scores_along_ids_fp64(sd, feats, ids.cpu(), 0, 1.0) - noise


def test_no_repeat_bigram_breaks_a_stuck_greedy_caption(lib):
    """the case that fails without the feature: a model whose greedy caption is one word over and over"""
    d, sd, feats = _lstm_case(32, 4)
    sd = dict(sd)
    sd["out_linear.bias"] = sd["out_linear.bias"].clone()
    sd["out_linear.bias"][7] += 50.0
    m, x = _model(d, sd), feats.to(DEV)
    assert bool((m(x, mode="test") == 7).all())                          # (on the device: the unconstrained caption is 7 7 7 ...)
    ids = m.decode_constrained(x, no_repeat_ngram_size=2)
    a = _check_invariants(ids, (4, 1, d["L"] - 1), d["V"], n=2)
    assert (a[:, :2] == 7).all() and (a[:, 2] != 7).all()
    capi.check_async_error()


@pytest.mark.parametrize("B", [4, 40, 64])                               # the per-step path, a padded plane batch, 64 rows
@pytest.mark.parametrize("H", [32, 512])
def test_whole_decode_keeps_its_constraints(lib, B, H):
    d, sd, feats = _lstm_case(H, B)
    V, S = d["V"], d["L"] - 1
    theta = 1.5
    # ---- CPU first: the float64 constrained greedy decode decides at least 90 % of its row-steps by more than the tolerance
    main = sampling.check_constraints(2, theta, M_LEN, None, V, EOS, length=d["L"])
    cpu_ids, cpu_marg = _cpu_constrained_greedy(sd, feats, main)
    decided = cpu_marg > 2 * _tol(theta)
    assert decided.mean() >= 0.9, decided.mean()
    first = np.where(decided.all(1), S, (~decided).argmax(1))            # per row: the steps in front of its first undecided one
    m, x = _model(d, sd), feats.to(DEV)
    greedy = m(x, mode="test")
    # ---- defaults: nothing constrained is today's result
    assert torch.equal(m.decode_constrained(x)[:, 0], greedy)
    assert torch.equal(m.decode_constrained(x, temperature=0.8, seed=5, top_k=5), m.sample_truncated(x, 1, temperature=0.8, seed=5, top_k=5))
    assert torch.equal(m.decode_constrained(x, 2, temperature=1.0, seed=5), m.sample_truncated(x, 2, temperature=1.0, seed=5))
    # banned ids that would otherwise be generated: the most frequent words of the unconstrained caption (never <eos>)
    freq = np.bincount(greedy.cpu().numpy().reshape(-1), minlength=V)
    freq[EOS] = 0
    banned = [int(v) for v in np.argsort(-freq)[:3]]
    kw = dict(repetition_penalty=theta, min_length=M_LEN)
    # ---- greedy
    ids = m.decode_constrained(x, no_repeat_ngram_size=2, **kw)
    a = _check_invariants(ids, (B, 1, S), V, n=2, m=M_LEN)[:, :]
    for r in range(B):                                                   # the CPU's caption up to the row's first undecided step
        assert np.array_equal(a[r, :first[r]], cpu_ids[r, :first[r]]), r
    worst = _replay_check(_logits_along(sd, feats, ids[:, 0]), a, main)
    print("B=%d H=%d greedy: %.1f %% of the row-steps decided; largest float64 gap %.3g (tol %.3g)" % (B, H, 100 * decided.mean(), worst, _tol(theta)))
    for n in (1, 3):
        ids = m.decode_constrained(x, no_repeat_ngram_size=n, banned_ids=banned, **kw)
        a = _check_invariants(ids, (B, 1, S), V, n=n, m=M_LEN, banned=banned)
        _replay_check(_logits_along(sd, feats, ids[:, 0]), a, sampling.check_constraints(n, theta, M_LEN, banned, V, EOS))
    assert torch.equal(ids, m.decode_constrained(x, no_repeat_ngram_size=3, banned_ids=banned, **kw))
    # ---- sampled, top_k = 5 (K = 3 captions per clip at B = 4)
    K = 3 if B == 4 else 1
    t, seed = 1.0, 77
    rep = feats.repeat_interleave(K, 0)
    for n in (1, 2, 3):
        spec = sampling.check_constraints(n, theta, M_LEN, banned, V, EOS)
        skw = dict(temperature=t, top_k=5, no_repeat_ngram_size=n, banned_ids=banned, **kw)
        ids = m.decode_constrained(x, K, seed=seed, **skw)
        a = _check_invariants(ids, (B, K, S), V, n=n, m=M_LEN, banned=banned)
        assert torch.equal(ids, m.decode_constrained(x, K, seed=seed, **skw))
        assert not torch.equal(ids, m.decode_constrained(x, K, seed=seed + 1, **skw))
        _replay_check(_logits_along(sd, rep, ids.view(B * K, S)), a, spec, sample=(t, seed, 5))
    capi.check_async_error()


# ------------------------------------------------------------------ 4. GRU and stacked LSTM
def _stack_logits64(sd, feats, caps_in, N):
    """S2VT(num_layers=N).forward(mode='train') in float64: model_refs.gru_model64's composition on fp64 nn.LSTM stacks"""
    P = {k: refs.d64(v) for k, v in sd.items()}
    feats = refs.d64(feats)
    B, L, _ = feats.shape
    H, E = P["feat_linear.weight"].shape[0], P["embedding.weight"].shape[1]

    def rnn(prefix, inp):
        cell = torch.nn.LSTM(inp.shape[2], H, num_layers=N, batch_first=True).double()
        cell.load_state_dict({k[len(prefix) + 1:]: v for k, v in P.items() if k.startswith(prefix + ".")})
        return cell(inp)[0]
    with torch.no_grad():
        x = feats @ P["feat_linear.weight"].t() + P["feat_linear.bias"]
        v = rnn("vid_rnn", torch.cat([x, torch.zeros(B, L - 1, H, dtype=torch.float64)], 1))
        emb = P["embedding.weight"][caps_in]
        w = rnn("word_rnn", torch.cat([torch.cat([torch.zeros(B, L, E, dtype=torch.float64), emb], 1), v], 2))
        return (w[:, L:] @ P["out_linear.weight"].t() + P["out_linear.bias"]).numpy()


def _variant(m, feats, sos, logits_fn, V, S):
    B = feats.shape[0]
    x = feats.to(DEV)
    theta = 1.5
    greedy = m(x, mode="test")
    assert torch.equal(m.decode_constrained(x)[:, 0], greedy)
    assert torch.equal(m.decode_constrained(x, 2, temperature=1.0, seed=3, top_k=5), m.sample_truncated(x, 2, temperature=1.0, seed=3, top_k=5))
    freq = np.bincount(greedy.cpu().numpy().reshape(-1), minlength=V)
    freq[EOS] = 0
    banned = [int(v) for v in np.argsort(-freq)[:2]]
    kw = dict(repetition_penalty=theta, min_length=4, banned_ids=banned)

    def along(ids2d):
        caps_in = torch.cat([torch.full((ids2d.shape[0], 1), sos, dtype=torch.long), ids2d[:, :-1].cpu()], 1)
        return caps_in
    for n in (1, 2, 3):
        spec = sampling.check_constraints(n, theta, 4, banned, V, EOS)
        ids = m.decode_constrained(x, no_repeat_ngram_size=n, **kw)
        a = _check_invariants(ids, (B, 1, S), V, n=n, m=4, banned=banned)
        _replay_check(logits_fn(feats, along(ids[:, 0])), a, spec)
        ids = m.decode_constrained(x, 3, temperature=1.0, seed=9, top_k=5, no_repeat_ngram_size=n, **kw)
        a = _check_invariants(ids, (B, 3, S), V, n=n, m=4, banned=banned)
        _replay_check(logits_fn(feats.repeat_interleave(3, 0), along(ids.view(B * 3, S))), a, spec, sample=(1.0, 9, 5))
        # n_samples = 3 is the decode of the repeated clips
        assert torch.equal(ids.view(B * 3, S), m.decode_constrained(x.repeat_interleave(3, 0), 1, temperature=1.0, seed=9, top_k=5,
                                                                    no_repeat_ngram_size=n, **kw)[:, 0])
        assert not torch.equal(ids, m.decode_constrained(x, 3, temperature=1.0, seed=10, top_k=5, no_repeat_ngram_size=n, **kw))
    capi.check_async_error()


def test_gru_constrained(lib):
    import make_gru_golden as gru_gen
    d, sd, feats, _, _ = gru_gen.setup("gru_tiny")
    m = _model(d, sd, rnn_type="gru")
    P = {k: refs.d64(v) for k, v in sd.items()}

    def logits(f, caps_in):
        with torch.no_grad():
            return refs.gru_model64(P, f, caps_in).numpy()
    _variant(m, feats, 3, logits, d["V"], d["L"] - 1)


def test_stacked_constrained(lib):
    import make_stack_golden as stack_gen
    d, sd, feats, _, _ = stack_gen.setup("stack_tiny")
    m = _model(d, sd, num_layers=d["N"])
    _variant(m, feats, 3, lambda f, caps_in: _stack_logits64(sd, f, caps_in, d["N"]), d["V"], d["L"] - 1)


# ------------------------------------------------------------------ 5. eval.py
_CHILD = """
import sys
sys.path.insert(0, %r)
import eval as ev
common = ["--model-path", %r, "--caption-file", %r, "--feats-path", %r, "--batch-size", "3"]
ev.main(common + ["--out", %r])
ev.main(common + ["--out", %r, "--no-repeat-ngram", "2", "--ban-words", "<unk>", "--sample", "2", "--top-k", "5"])
"""


def test_eval_flags_in_a_child_process(lib, tmp_path):
    import S2VTModel
    import dataloader
    import eval as ev
    import test_train_eval_parity as toy
    data = toy.make_toy(str(tmp_path))
    V = len(data["word2ix"]) + 1                                         # (ids 0..29 with 2 unused)
    sd = synth.make_state_dict(V, toy.F, toy.H, toy.E, seed=23)
    sd["out_linear.bias"][1] += 50.0                                     # <unk> wins every step of the unconstrained caption
    sd["out_linear.bias"][2] -= 50.0                                     # (id 2 has no word in the toy vocabulary)
    m = S2VTModel.S2VT(V, toy.F, toy.L, dim_hid=toy.H, dim_embed=toy.E)
    m.load_state_dict(sd)
    ck = str(tmp_path / "model.pth")
    torch.save(m, ck)
    caps, fdir = str(tmp_path / "captions.json"), str(tmp_path / "feats")
    plain, con = str(tmp_path / "plain.json"), str(tmp_path / "con.json")
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, ck, caps, fdir, plain, con)], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    # without the flags: today's output, byte for byte - the captions of mode='test' written as main() writes them
    dataset = dataloader.VideoDataset(caps, fdir, mode="test")
    loader = torch.utils.data.DataLoader(dataset, batch_size=3, shuffle=False)
    md = m.to(DEV).eval()
    want = {}
    with torch.no_grad():
        for feats, targets, ids, masks in loader:
            for vid, seq in zip(ids, md(feats.to(DEV), mode="test").cpu()):
                want[vid] = ev.ids_to_caption(seq.tolist(), dataset.ix2word)
    with open(plain, "rb") as f:
        assert f.read() == json.dumps(want, ensure_ascii=False, indent=1).encode("utf-8")
    assert all(c.split() == ["<unk>"] * (toy.L - 1) for c in want.values())
    with open(con, encoding="utf-8") as f:
        preds = json.load(f)
    with open(con + ".samples.json", encoding="utf-8") as f:
        samples = json.load(f)
    assert set(preds) == set(want) == set(samples) and len(preds) == 4
    for cap in list(preds.values()) + [c for cs in samples.values() for c in cs]:
        words = cap.split()
        assert "<unk>" not in words and hc.ngram_repeats(words, 2) == 0, cap
    capi.check_async_error()
