"""CPU: constrained decoding (csrc/truncate.hip "constrained draw", S2VT.decode_constrained) - known answers of the numpy
restatement (sampling.constrain_logits), the C ABI's surface, the argument checks that come before any device call, and the
fixtures that the GPU tests of test_gpu_constrained.py share (with their CPU preconditions)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import capi, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("s2vt_constrained_draw", "s2vt_decode_rows_constrained", "s2vt_decode_rows_constrained_workspace_bytes")
INF = float("inf")


def spec(n=0, theta=1.0, m=0, banned=(), V=10, eos=4):
    return sampling.check_constraints(n, theta, m, list(banned), V, eos)


# ---- shared with test_gpu_constrained.py
KERNEL_V = (23, 4096, 4097, 12289, 16385)            # every RegRow width, one boundary, LdsRow above 48 KiB of dynamic LDS
KERNEL_ROWS = (1, 5, 70)
KERNEL_T = (0, 1, 2, 3, 40, 79)
HIST_WORDS = 6                                       # the histories draw from 6 distinct words: n-grams do repeat


def kernel_case(V, seed=0):
    """(logits fp32 [70, V] = randint(-40, 40) / 8, exact in fp32; history ids int64 [70, 79] over HIST_WORDS distinct words spread
    over [0, V))"""
    g = torch.Generator().manual_seed(1234 + V + seed)
    x = torch.randint(-40, 40, (max(KERNEL_ROWS), V), generator=g).float() / 8
    words = torch.tensor([0, 1, V // 3, V // 2, V - 2, V - 1], dtype=torch.int64)[:HIST_WORDS]
    h = words[torch.randint(0, HIST_WORDS, (max(KERNEL_ROWS), max(KERNEL_T)), generator=g)]
    return x, h


def pack_history(h, hist_ld, score_bits=0x12345678):
    """the drivers' packed words int64 [t, hist_ld] of history ids [rows, t]: (some ordered score) << 32 | (0xFFFFFFFF - id), the
    columns beyond the rows filled with a word whose token is far outside any vocabulary"""
    rows, t = h.shape
    out = torch.full((max(t, 1), hist_ld), (score_bits << 32) | 0x0000FFFF, dtype=torch.int64)      # token 0xFFFF0000
    out[:t, :rows] = ((score_bits << 32) | (0xFFFFFFFF - h.t())).to(torch.int64)
    return out


def kernel_specs(V, t):
    """the specs of the row-kernel test: n in (0, 1, 2, 3) x theta in (1, 1.5) x m in (0, t + 1) x banned in ([], [0, V - 1])"""
    return [sampling.check_constraints(n, theta, m, banned, V, 4)
            for n in (0, 1, 2, 3) for theta in (1.0, 1.5) for m in (0, t + 1) for banned in ([], [0, V - 1])]


def ngram_repeats(ids, n):
    """number of n-grams that occur more than once in a sequence of ids"""
    grams = [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]
    return len(grams) - len(set(grams))


# ---- the restatement: known answers
def test_repetition_penalty_once_per_distinct_word_by_sign():
    x = np.array([2.0, -2.0, 0.0, 3.0, 1.0, -1.0, 4.0, 8.0, 16.0, -4.0], dtype=np.float32)
    sp = spec(theta=2.0)
    # word 0 seen three times: penalised ONCE (2 / 2, not 2 / 8); positive -> * r, negative -> * theta, zero stays zero
    got = sampling.constrain_logits(x, [0, 0, 0, 1, 2], 5, sp)
    assert got.dtype == np.float32 and got.tolist() == [1.0, -4.0, 0.0, 3.0, 1.0, -1.0, 4.0, 8.0, 16.0, -4.0]
    assert sampling.constrain_logits(x, [0, 0, 0, 1, 2], 0, sp).tolist() == x.tolist()              # t = 0: no history yet
    assert sampling.constrain_logits(x, [0, 0, 0, 1, 2], 2, sp).tolist()[:2] == [1.0, -2.0]         # only h[0..2)
    # r = fp32(1 / theta), a multiplication: bitwise in fp32, the same factors in float64
    sp3 = spec(theta=1.5)
    r = np.float32(1.0 / float(np.float32(1.5)))
    assert sampling.constrain_logits(x, [7], 1, sp3)[7] == np.float32(8.0) * r
    assert sampling.constrain_logits(x.astype(np.float64), [7], 1, sp3)[7] == 8.0 * float(r)
    assert sampling.constrain_logits(x.astype(np.float64), [9], 1, sp3)[9] == -6.0
    assert x.tolist()[0] == 2.0                                                                     # the input is not modified
    # theta = 1: off
    assert sampling.constrain_logits(x, [0, 1, 2], 3, spec()).tolist() == x.tolist()


def test_no_repeat_ngram_at_the_first_steps():
    x = np.arange(10, dtype=np.float32)
    h = [5, 6, 5, 6, 7]

    def banned(n, t, hist=h):
        return np.nonzero(np.isneginf(sampling.constrain_logits(x, hist, t, spec(n=n))))[0].tolist()
    # n = 1: every word of the history (t = n - 2 = -1 does not exist; t = 0, 1)
    assert banned(1, 0) == [] and banned(1, 1) == [5] and banned(1, 4) == [5, 6]
    # n = 2 at t = 0 (n - 2), 1 (n - 1), 2 (n): the word after every earlier occurrence of h[t-1]
    assert banned(2, 0) == [] and banned(2, 1) == [] and banned(2, 2) == []                          # 6 was never followed
    assert banned(2, 3) == [6] and banned(2, 4) == [5] and banned(2, 5) == []
    # n = 3 at t = 1 (n - 2), 2 (n - 1), 3 (n), then the first repeat: suffix (5, 6) occurred at 0, followed by 5
    assert banned(3, 1) == [] and banned(3, 2) == [] and banned(3, 3) == [] and banned(3, 4) == [5]
    # overlapping matches: 5 5 5
    assert banned(2, 3, [5, 5, 5]) == [5] and banned(3, 3, [5, 5, 5]) == [5] and banned(3, 2, [5, 5, 5]) == []
    assert banned(2, 1, [5, 5, 5]) == [] and banned(2, 2, [5, 5, 5]) == [5] and banned(1, 3, [5, 5, 5]) == [5]
    # several continuations of one prefix are all banned
    assert banned(2, 5, [1, 2, 1, 3, 1]) == [2, 3]
    # rows are independent
    both = sampling.constrain_logits(np.stack([x, x]), [[5, 5, 5], [1, 2, 1]], 3, spec(n=2))
    assert np.nonzero(np.isneginf(both[0]))[0].tolist() == [5] and np.nonzero(np.isneginf(both[1]))[0].tolist() == [2]


def test_bans_min_length_and_a_ban_wins_over_a_penalty():
    x = np.array([2.0, -2.0, 0.0, 3.0, 1.0, -1.0, 4.0, 8.0, 16.0, -4.0], dtype=np.float32)
    got = sampling.constrain_logits(x, [0, 3], 2, spec(theta=2.0, banned=[3, 9]))
    assert got.tolist() == [1.0, -2.0, 0.0, -INF, 1.0, -1.0, 4.0, 8.0, 16.0, -INF]                  # 3: penalised AND banned -> -inf
    got = sampling.constrain_logits(x, [0, 0], 2, spec(theta=2.0, n=2))
    assert got[0] == -INF                                                                           # n-gram ban over the penalty
    for t, want in ((4, -INF), (5, 1.0), (6, 1.0)):                                                  # m = 5: t = m - 1 and t = m
        assert sampling.constrain_logits(x, [7] * 8, t, spec(m=5))[4] == want, t
    assert sampling.constrain_logits(x, [], 0, spec(m=1))[4] == -INF
    # <eos> in the history and under min_length: banned, not penalised
    assert sampling.constrain_logits(x, [4], 1, spec(m=3, theta=2.0))[4] == -INF


def test_check_constraints():
    sp = sampling.check_constraints(np.int64(2), np.float32(1.5), 3, (7, 7, 1), 30, 4)
    assert sp == sampling.ConstraintSpec(2, 1.5, 3, 4, (1, 7)) and sampling.constrains(sp)
    assert not sampling.constrains(sampling.check_constraints(0, 1, 0, None, 30, 4))
    for bad in (-1, 2.5, "2", True, None):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            sampling.check_constraints(bad, 1.0, 0, None, 30, 4)
    for bad in (0.99, 0, -2.0, float("nan"), float("inf"), 1e39, "1.5", None, True):
        with pytest.raises(ValueError, match="repetition_penalty"):
            sampling.check_constraints(0, bad, 0, None, 30, 4)
    for bad in (-1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="min_length"):
            sampling.check_constraints(0, 1.0, bad, None, 30, 4)
    for bad in ([30], [-1], [1.5], ["a"], [True], list(range(33))):
        with pytest.raises(ValueError, match="banned_ids"):
            sampling.check_constraints(0, 1.0, 0, bad, 40 if len(bad) > 1 else 30, 4)
    assert len(sampling.check_constraints(0, 1.0, 0, list(range(32)), 40, 4).banned) == 32
    with pytest.raises(ValueError, match="eos_ix"):
        sampling.check_constraints(0, 1.0, 0, None, 30, 30)
    # the drivers' rule: no step may ban a whole row
    sampling.check_constraints(2, 1.0, 0, [1, 2], 30, 4, length=27)                                 # 30 > 26 + 2 + 1
    with pytest.raises(ValueError, match="whole row"):
        sampling.check_constraints(2, 1.0, 0, [1, 2], 30, 4, length=28)
    with pytest.raises(ValueError, match="history"):
        sampling.check_constraints(2, 1.0, 0, None, 5000, 4, length=1026)
    sampling.check_constraints(2, 1.0, 0, None, 5000, 4, length=1025)


# ---- the C ABI
def test_new_symbols_declared_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "s2vt_hip.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in capi.SIGNATURES, name
    assert "constrained draw" in header and "struct s2vt_constraints" in header
    assert [f[0] for f in capi.Constraints._fields_] == ["no_repeat_ngram", "repetition_penalty", "min_length", "eos_ix", "n_banned", "banned"]
    assert lib.s2vt_abi_version() == capi.ABI_VERSION


def _cons(n=0, theta=1.0, m=0, eos=4, banned=(), n_banned=None, null=False):
    arr = (ctypes.c_int32 * max(1, len(banned)))(*banned)
    c = capi.Constraints(n, theta, m, eos, len(banned) if n_banned is None else n_banned,
                         None if null else ctypes.cast(arr, ctypes.POINTER(ctypes.c_int32)))
    return c, arr


def test_draw_refusals_come_before_the_device(lib):
    """made-up addresses stand for device memory: every rejection happens before anything is enqueued"""
    one = ctypes.c_void_p(256)

    def draw(logits=one, ld=30, rows=4, V=30, hist=one, hist_ld=4, t=2, con=None, greedy=0, temp=1.0, k=0, p=1.0, step=0, row0=0,
             packed=one, **ckw):
        c, keep = _cons(**ckw)
        return lib.s2vt_constrained_draw(logits, ld, rows, V, hist, hist_ld, t, None if con == "null" else ctypes.byref(c), greedy, temp,
                                         k, p, 5, step, row0, packed, None, None)
    cases = (
        (dict(theta=0.5), b"repetition_penalty"), (dict(theta=float("nan")), b"repetition_penalty"),
        (dict(theta=float("inf")), b"repetition_penalty"), (dict(theta=-1.0), b"repetition_penalty"),
        (dict(n=-1), b"no_repeat_ngram"), (dict(m=-1), b"min_length"),
        (dict(banned=(1,), n_banned=-1), b"n_banned"), (dict(banned=tuple(range(20)), n_banned=33), b"n_banned"),
        (dict(n_banned=2, null=True), b"n_banned"),
        (dict(banned=(30,)), b"banned id"), (dict(banned=(1, -1)), b"banned id"),
        (dict(eos=30), b"eos_ix"), (dict(eos=-1), b"eos_ix"),
        (dict(t=-1), b"outside [0, 1023]"), (dict(t=1024), b"outside [0, 1023]"),
        (dict(hist=None), b"history"), (dict(hist_ld=3), b"hist_ld"),
        (dict(con="null"), b"constraints"),
        (dict(k=-1), b"top_k"), (dict(k=31), b"top_k"), (dict(p=0.0), b"top_p"), (dict(p=1.5), b"top_p"), (dict(p=float("nan")), b"top_p"),
        (dict(temp=0.0), b"temperature"), (dict(temp=float("nan")), b"temperature"), (dict(temp=float("inf")), b"temperature"),
        (dict(greedy=1, temp=0.5), b"greedy"), (dict(greedy=1, k=5), b"greedy"), (dict(greedy=1, p=0.5), b"greedy"), (dict(greedy=2), b"greedy"),
        (dict(logits=None), b"null"), (dict(packed=None), b"null"), (dict(ld=29), b"invalid"), (dict(rows=0), b"invalid"), (dict(V=0), b"invalid"),
        (dict(V=38401, ld=38401), b"vocab_size"), (dict(step=-1), b"invalid"), (dict(row0=-1), b"invalid"),
    )
    for kw, word in cases:
        assert draw(**kw) == -1, kw
        err = lib.s2vt_last_error()
        assert b"s2vt_constrained_draw" in err and word in err, (kw, err)


def test_driver_refusals_come_before_the_device(lib):
    one = ctypes.c_void_p(256)
    prm = capi.Params()
    big = 1 << 40

    def rows(d=(4, 6, 16, 8, 8, 30), K=2, sos=3, greedy=0, temp=1.0, k=0, p=1.0, ws=big, feats=one, con=None, **ckw):
        dd = capi.Dims(*d)
        c, keep = _cons(**dict(dict(n=2), **ckw))
        return lib.s2vt_decode_rows_constrained(ctypes.byref(dd), ctypes.byref(prm), feats, K, sos, greedy, temp, 5, k, p,
                                                None if con == "null" else ctypes.byref(c), one, one, ws, None, 0, 0, None)
    cases = (
        (dict(theta=0.5), b"repetition_penalty"), (dict(theta=float("nan")), b"repetition_penalty"), (dict(n=-1), b"no_repeat_ngram"),
        (dict(m=-1), b"min_length"), (dict(banned=tuple(range(20)), n_banned=33), b"n_banned"), (dict(banned=(30,)), b"banned id"),
        (dict(eos=30), b"eos_ix"), (dict(con="null"), b"constraints"),
        (dict(greedy=1, temp=0.5), b"greedy"), (dict(greedy=1, k=5), b"greedy"), (dict(greedy=1, p=0.5), b"greedy"),
        (dict(k=-1), b"top_k"), (dict(k=31), b"top_k"), (dict(p=0.0), b"top_p"), (dict(p=float("nan")), b"top_p"),
        (dict(K=0), b"K"), (dict(sos=30), b"sos_ix"), (dict(temp=0.0), b"temperature"), (dict(ws=16), b"workspace"), (dict(feats=None), b"null"),
        # a shape that could ban a whole row: V = 30 <= (L - 1) + n_banned + 1
        (dict(d=(4, 30, 16, 8, 8, 30)), b"whole row"), (dict(d=(4, 28, 16, 8, 8, 30), banned=(1, 2)), b"whole row"),
        (dict(d=(4, 1026, 16, 8, 8, 3000)), b"history"),
    )
    for kw, word in cases:
        assert rows(**kw) == -1, kw
        err = lib.s2vt_last_error()
        assert b"s2vt_decode_rows_constrained" in err and word in err, (kw, err)
    d = capi.Dims(16, 80, 4096, 512, 512, 3000)
    for K in (1, 3):
        assert lib.s2vt_decode_rows_constrained_workspace_bytes(ctypes.byref(d), K) == lib.s2vt_sample_rows_trunc_workspace_bytes(ctypes.byref(d), K) > 0
    assert lib.s2vt_decode_rows_constrained_workspace_bytes(ctypes.byref(d), 0) == 0


def test_model_refusals_come_before_the_device():
    import S2VTModel
    x = torch.zeros(2, 5, 16)                            # a CPU tensor: a bad argument is refused before the tensor is looked at
    for kw in ({}, dict(rnn_type="gru"), dict(num_layers=2)):
        m = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8, **kw)
        for bad, word in ((dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
                          (dict(repetition_penalty=0.5), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                          (dict(min_length=-1), "min_length"), (dict(banned_ids=[30]), "banned_ids"), (dict(banned_ids=[-1]), "banned_ids"),
                          (dict(top_k=31, temperature=1.0), "top_k"), (dict(top_p=0.0, temperature=1.0), "top_p"),
                          (dict(temperature=0.0), "temperature"), (dict(temperature=1.0, seed=-1), "seed"),
                          (dict(n_samples=0), "n_samples"), (dict(n_samples=2.5), "n_samples"),
                          # greedy (temperature=None) takes one caption and no truncation
                          (dict(n_samples=2), "greedy"), (dict(top_k=5), "greedy"), (dict(top_p=0.9), "greedy"),
                          (dict(banned_ids=list(range(25))), "whole row")):
            with pytest.raises(ValueError, match=word):
                m.decode_constrained(x, **dict(dict(no_repeat_ngram_size=2), **bad))
        for good in (dict(no_repeat_ngram_size=2), dict(temperature=1.0, seed=1, n_samples=2, top_k=5, repetition_penalty=1.2),
                     dict(), dict(temperature=1.0, seed=1)):
            with pytest.raises(capi.S2VTHipError):       # good arguments: the CPU tensor fails loudly
                m.decode_constrained(x, **good)


def test_signatures():
    import S2VTModel
    S = S2VTModel.S2VT
    assert list(inspect.signature(S.forward).parameters) == ["self", "feats", "targets", "mode", "beam_width", "max_beam_depth", "ss_prob",
                                                             "ss_temperature", "length_alpha", "n_best", "temperature", "seed"]
    assert list(inspect.signature(S.sample).parameters) == ["self", "feats", "n_samples", "temperature", "seed"]
    assert list(inspect.signature(S.sample_truncated).parameters) == ["self", "feats", "n_samples", "temperature", "seed", "top_k", "top_p"]
    sig = inspect.signature(S.decode_constrained)
    assert list(sig.parameters) == ["self", "feats", "n_samples", "temperature", "seed", "top_k", "top_p", "no_repeat_ngram_size",
                                    "repetition_penalty", "min_length", "banned_ids"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [1, None, None, 0, 1.0, 0, 1.0, 0, None]


def test_eval_flags():
    sys.path.insert(0, ROOT)
    import eval as ev
    a = ev.build_parser().parse_args(["--model-path", "m.pth"])
    assert (a.no_repeat_ngram, a.repetition_penalty, a.min_length, a.ban_words) == (0, 1.0, 0, "") and ev.constraints_of(a) is None
    a = ev.build_parser().parse_args(["--model-path", "m.pth", "--no-repeat-ngram", "3", "--repetition-penalty", "1.2", "--min-length", "5",
                                      "--ban-words", "<unk>,<pad>"])
    assert ev.constraints_of(a) == dict(no_repeat_ngram_size=3, repetition_penalty=1.2, min_length=5, ban_words=["<unk>", "<pad>"])
    with pytest.raises(SystemExit):                      # refused together with --beam, before a model is loaded
        ev.main(["--model-path", "m.pth", "--beam", "3", "--no-repeat-ngram", "2"])

    class M:
        def decode_constrained(self):
            pass
    m = M()
    con = ev.constraint_kwargs(dict(no_repeat_ngram_size=2, repetition_penalty=1.0, min_length=0, ban_words=["<unk>"]), {"<unk>": 2, "<eos>": 9}, m)
    assert con == dict(no_repeat_ngram_size=2, repetition_penalty=1.0, min_length=0, banned_ids=[2]) and m.eos_ix == 9
    with pytest.raises(ValueError, match="not in the vocabulary: zebra"):
        ev.constraint_kwargs(dict(ban_words=["<unk>", "zebra"]), {"<unk>": 2}, m)
    assert ev.constraint_kwargs(None, {}, m) == {}


# ---- CPU preconditions of the GPU tests
@pytest.mark.parametrize("V", KERNEL_V)
def test_kernel_fixture_repeats_its_ngrams(V):
    """at least half of the rows with t >= 3 have one or more blocked words at n = 2, and the logits are exact multiples of 1/8"""
    x, h = kernel_case(V)
    assert torch.equal(x * 8, (x * 8).round()) and x.abs().max() <= 5
    sp = sampling.check_constraints(2, 1.0, 0, None, V, 4)
    hit = np.concatenate([np.isneginf(sampling.constrain_logits(x.numpy(), h.numpy(), t, sp)).sum(1) >= 1 for t in KERNEL_T if t >= 3])
    assert hit.size == 3 * 70 and hit.mean() >= 0.5, (V, hit.mean())                               # (pooled over t = 3, 40, 79)
    p = pack_history(h[:5, :3], 8)
    assert tuple(p.shape) == (3, 8) and torch.equal(0xFFFFFFFF - (p[:, :5] & 0xFFFFFFFF), h[:5, :3].t())
    assert int(0xFFFFFFFF - (p[0, 7] & 0xFFFFFFFF)) >= 38400
