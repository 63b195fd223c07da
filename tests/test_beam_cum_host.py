"""CPU: the cumulative-score beam search (S2VT.forward(mode='beam'), csrc/beam_policy.hip) - argument checks of the Python surface and
of the C ABI before anything is launched, and the fp64 restatement the GPU tests compare against (tests/beam_cum_ref.py): it
degenerates to greedy decoding at width 1, its float32 policy restatement takes the same decisions, and at most a quarter of each
case's samples rest on a near-tie (the cap on what tests/test_gpu_beam_cum.py may leave out)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import s2vt_video_caption_amd  # noqa: F401
from s2vt_video_caption_amd import beam, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_cum_ref as ref  # noqa: E402

# robust samples per case, measured with the fp64 restatement (both gaps >= 2e-4); the GPU test asserts the same counts
ROBUST = {"tiny": 8, "tiny5": 7, "mid64": 56}


@pytest.fixture(scope="module")
def searches():
    return {name: ref.case_search(name) for name in ref.CASES}


def test_forward_signature_and_argument_errors_before_the_library():
    import S2VTModel
    sig = inspect.signature(S2VTModel.S2VT.forward)
    names = list(sig.parameters)
    assert names[-4:] == ["length_alpha", "n_best", "temperature", "seed"]
    assert sig.parameters["length_alpha"].default == 0.7 and sig.parameters["n_best"].default == 1
    m = S2VTModel.S2VT(30, 16, 5, dim_hid=8, dim_embed=8)
    x = torch.zeros(2, 5, 16)                       # a CPU tensor: a bad argument is refused before the tensor is looked at
    for kw in (dict(beam_width=0), dict(beam_width=9), dict(beam_width=2.5), dict(n_best=0), dict(beam_width=3, n_best=4),
               dict(max_beam_depth=0), dict(length_alpha=-0.1), dict(length_alpha=float("nan")), dict(length_alpha=float("inf"))):
        with pytest.raises(ValueError, match="mode='beam'"):
            m(x, mode="beam", **kw)
    small = S2VTModel.S2VT(19, 16, 5, dim_hid=8, dim_embed=8)
    with pytest.raises(ValueError, match="vocab_size"):
        small(x, mode="beam")
    with pytest.raises(capi.S2VTHipError):          # good arguments: the CPU tensor fails loudly
        m(x, mode="beam", beam_width=8, n_best=8, length_alpha=0)
    assert beam.check_beam_args(8, 1, 0, 8, 20) == (8, 1, 0.0, 8)
    # the other modes ignore the new arguments, as they ignore temperature
    with pytest.raises(capi.S2VTHipError):
        m(x, mode="test", n_best=99, length_alpha=-1)


def test_c_abi_is_declared_bound_and_refuses_bad_arguments(lib):
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in ("s2vt_beam_cum_bytes", "s2vt_beam_cum_step", "s2vt_beam_cum_result"):
        assert re.search(r"\b%s\(" % name, header) and name in capi.SIGNATURES, name
    assert lib.s2vt_abi_version() == 9              # the API is additive
    nb = lib.s2vt_beam_cum_bytes(64, 5, 12)
    assert 0 < nb < 1 << 20
    assert lib.s2vt_beam_cum_bytes(64, 8, 30) > nb
    for bad in ((0, 5, 12), (64, 0, 12), (64, 9, 12), (64, 5, 0), (-1, 5, 12), (1 << 20, 8, 1 << 10)):
        assert lib.s2vt_beam_cum_bytes(*bad) == 0, bad
    p = ctypes.c_void_p(256)                        # never dereferenced: every call below is refused before a launch
    ok = dict(B=4, W=3, D=6, sos=3, eos=4, alpha=0.7, depth=1, state=p, nbytes=1 << 20)

    def step(**kw):
        a = dict(ok, **kw)
        return lib.s2vt_beam_cum_step(a["B"], a["W"], a["D"], a["sos"], a["eos"], a["alpha"], a["depth"], a["state"], a["nbytes"],
                                      a.get("ix", p), a.get("lp", p), a.get("rb", p), a.get("rs", p), a.get("rt", p), None)
    for kw in (dict(B=0), dict(W=0), dict(W=9), dict(D=0), dict(depth=-1), dict(depth=7), dict(state=None), dict(rb=None), dict(rs=None),
               dict(rt=None), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(depth=2, ix=None),
               dict(depth=0, lp=None), dict(nbytes=16)):
        rc = step(**kw)
        assert rc == -1 and b"s2vt_beam_cum_step" in lib.s2vt_last_error(), kw
    with pytest.raises(capi.S2VTHipError):
        capi.check(step(W=9), "s2vt_beam_cum_step")
    for args in ((0, 3, 6, 4, 1, p, 1 << 20, p, p, p), (4, 9, 6, 4, 1, p, 1 << 20, p, p, p), (4, 3, 6, 4, 0, p, 1 << 20, p, p, p),
                 (4, 3, 6, 4, 4, p, 1 << 20, p, p, p), (4, 3, 6, 4, 3, None, 1 << 20, p, p, p), (4, 3, 6, 4, 3, p, 16, p, p, p),
                 (4, 3, 6, 4, 3, p, 1 << 20, None, p, p), (4, 3, 6, 4, 3, p, 1 << 20, p, None, p), (4, 3, 6, 4, 3, p, 1 << 20, p, p, None)):
        rc = lib.s2vt_beam_cum_result(*args, None)
        assert rc == -1 and b"s2vt_beam_cum_result" in lib.s2vt_last_error(), args


def test_width_one_without_length_penalty_is_greedy_decoding():
    """W = 1, alpha = 0: the one live hypothesis takes the arg-max word of every step until <eos> or D words"""
    ended = 0
    for name in ("tiny", "mid64"):
        sd, feats, _, D = ref.case_inputs(name)
        D = min(D, feats.shape[1] - 1)
        res = ref.search_fp64(sd, feats, 1, D, alpha=0.0)
        greedy, _ = ref.greedy_fp64(sd, feats, D)
        assert [r["ids"][0] for r in res] == greedy
        ended += sum(g[-1] == ref.EOS and len(g) < D for g in greedy)
    assert ended >= 1                               # (the cut at <eos> is exercised)


def test_float32_policy_restatement_takes_the_fp64_decisions(searches):
    """PolicyF32 (what the kernel is compared with bit for bit) fed with the fp64 search's own top-20 log-probs, rounded to fp32,
    returns the fp64 n-best on every robust sample: the two restatements are one definition."""
    name = "tiny5"
    sd, feats, W, D = ref.case_inputs(name)
    p = {k: v.double() for k, v in sd.items()}
    B = feats.shape[0]
    # per depth, every row's top-20 (ascending ids) from the fp64 model, driven by the policy's own rows
    from oracle import s2vt_oracle as oracle
    x1 = feats.double() @ p["feat_linear.weight"].t() + p["feat_linear.bias"]
    out1, (h1, c1) = oracle._vid_layer(p, x1, feats.shape[1])
    h2 = torch.zeros(B, x1.shape[2], dtype=torch.float64)
    c2 = torch.zeros_like(h2)
    for t in range(feats.shape[1]):
        h2, c2 = oracle._word_step(p, None, out1[:, t], h2, c2)
    R = B * W
    tabs = [(torch.zeros(R, h2.shape[1], dtype=torch.float64), torch.zeros(R, h2.shape[1], dtype=torch.float64)) for _ in range(2)]
    tabs[0][0][:B], tabs[0][1][:B] = h2, c2
    pol = ref.PolicyF32(B, W, D, ref.ALPHA)
    for t in range(1, D + 1):
        rs, rt = [torch.as_tensor(r).long() for r in pol.rows()]
        h1, c1 = oracle.lstm_cell(None, h1, c1, p["vid_rnn.weight_ih_l0"], p["vid_rnn.weight_hh_l0"], p["vid_rnn.bias_ih_l0"],
                                  p["vid_rnn.bias_hh_l0"])
        wh_in, wc_in = tabs[(t - 1) & 1]
        wh, wc = oracle._word_step(p, p["embedding.weight"][rt], h1.repeat_interleave(W, dim=0), wh_in[rs], wc_in[rs])
        tabs[t & 1][0][:], tabs[t & 1][1][:] = wh, wc
        lp = torch.log_softmax(wh @ p["out_linear.weight"].t() + p["out_linear.bias"], dim=1)
        ix = lp.topk(20, dim=1).indices.sort(dim=1).values
        pol.step(ix.numpy().astype(np.int32), lp.gather(1, ix).numpy().astype(np.float32))
    ids, lens, scores = pol.result()
    rb = ref.robust(searches[name])
    for b in np.nonzero(rb)[0]:
        want = searches[name][b]
        assert [ids[b, k, :lens[b, k]].tolist() for k in range(W)] == want["ids"], b
        assert np.abs(scores[b] - np.array(want["scores"])).max() < 1e-5, b


def test_most_samples_of_every_case_are_robust(searches):
    """At least three quarters of each batch decide every selection and the n-best order by >= 2e-4: the GPU comparison covers them"""
    for name, res in searches.items():
        rb = ref.robust(res)
        B = len(res)
        lens = [len(r["ids"][0]) for r in res]
        print("%s: robust %d/%d, best lengths %d..%d" % (name, int(rb.sum()), B, min(lens), max(lens)))
        assert 4 * int(rb.sum()) >= 3 * B, (name, int(rb.sum()))
        assert int(rb.sum()) == ROBUST[name]
        assert all(len(r["ids"]) == ref.CASES[name][3] for r in res)
