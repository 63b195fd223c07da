"""CPU: the GRU cell's C-ABI entry points (include/s2vt_hip.h, s2vt_gru_*) are exported, bound and refuse bad arguments before any
device call; a GRU model keeps its host-side contract; the GRU fixtures (tests/golden/gru_*.npz, tools/make_gru_golden.py) agree
with the generator's fp64 replay of the greedy loop."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GRU_ENTRIES = ("s2vt_gru_step_fwd", "s2vt_gru_step_fwd_token", "s2vt_gru_step_bwd", "s2vt_gru_seq_fwd", "s2vt_gru_seq_bwd",
               "s2vt_tokens_time_major")


def test_gru_entry_points_exported_and_bound(lib):
    from s2vt_video_caption_amd import capi
    raw = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in GRU_ENTRIES:
        assert hasattr(raw, name), "libs2vt_hip.so does not export %s" % name
        assert name in capi.SIGNATURES, "capi.py does not bind %s" % name
        assert (name + "(") in header
    assert lib.s2vt_abi_version() == capi.ABI_VERSION == 9


def _rejects(lib, name, rc):
    assert rc == -1, (name, rc)
    assert name.encode() in lib.s2vt_last_error(), (name, lib.s2vt_last_error())


def test_gru_entry_points_reject_bad_arguments(lib):
    """Null operands / non-positive sizes return S2VT_ERR_ARG with a message naming the entry point (no device call is made)."""
    p = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced: the argument check runs first
    _rejects(lib, "s2vt_gru_step_fwd", lib.s2vt_gru_step_fwd(4, 32, None, None, p, p, None, p, None, None))       # no gx, no b_ih
    _rejects(lib, "s2vt_gru_step_fwd", lib.s2vt_gru_step_fwd(0, 32, p, None, p, p, None, p, None, None))
    _rejects(lib, "s2vt_gru_step_fwd", lib.s2vt_gru_step_fwd(4, 32, p, None, p, None, None, p, None, None))       # no b_hh
    _rejects(lib, "s2vt_gru_step_fwd_token",
             lib.s2vt_gru_step_fwd_token(4, 32, 24, 50, p, p, p, None, p, p, 10, None, None, 3, p, None))          # ldw_e < E
    _rejects(lib, "s2vt_gru_step_fwd_token",
             lib.s2vt_gru_step_fwd_token(4, 32, 24, 0, p, p, p, None, p, p, 56, None, None, 3, p, None))           # V = 0
    # a constant token outside the vocabulary is refused on the host with S2VT_ERR_INDEX (no device flag, nothing to synchronise on)
    for bad in (50, -1):
        rc = lib.s2vt_gru_step_fwd_token(4, 32, 24, 50, p, p, p, None, p, p, 56, None, None, bad, p, None)
        assert rc == -2 and b"s2vt_gru_step_fwd_token" in lib.s2vt_last_error(), (bad, rc)
    _rejects(lib, "s2vt_gru_step_bwd", lib.s2vt_gru_step_bwd(4, 32, None, None, None, None, None, None, p, p, p, None))  # no stash
    _rejects(lib, "s2vt_gru_step_bwd", lib.s2vt_gru_step_bwd(4, 32, p, p, None, None, p, None, p, p, p, None))     # no stash_next
    _rejects(lib, "s2vt_gru_step_bwd", lib.s2vt_gru_step_bwd(4, 32, p, None, p, None, p, None, p, p, p, None))     # no W_hh^T
    _rejects(lib, "s2vt_gru_seq_fwd", lib.s2vt_gru_seq_fwd(8, 4, 32, None, 3, p, p, p, p, None, None))           # n_gx without gx
    _rejects(lib, "s2vt_gru_seq_fwd", lib.s2vt_gru_seq_fwd(8, 4, 32, p, 3, None, p, p, p, None, None))           # no b_ih for step 3+
    _rejects(lib, "s2vt_gru_seq_fwd", lib.s2vt_gru_seq_fwd(8, 4, 32, p, 9, p, p, p, p, None, None))              # n_gx > T
    _rejects(lib, "s2vt_gru_seq_bwd", lib.s2vt_gru_seq_bwd(8, 4, 32, p, None, 0, p, p, None, p, p, p, None))     # no W_hh^T scratch
    _rejects(lib, "s2vt_gru_seq_bwd", lib.s2vt_gru_seq_bwd(0, 4, 32, p, None, 0, p, p, p, p, p, p, None))
    _rejects(lib, "s2vt_tokens_time_major", lib.s2vt_tokens_time_major(4, 7, 50, None, 8, p, None))
    _rejects(lib, "s2vt_tokens_time_major", lib.s2vt_tokens_time_major(4, 7, 50, p, 6, p, None))                # ld < L-1


def test_gru_model_host_contract():
    """A one-layer GRU model takes the GRU path (not the LSTM whole-path tuple, which keeps refusing it) and, like every HIP
    path here, refuses CPU tensors."""
    import S2VTModel
    from s2vt_video_caption_amd import capi, gru_functional, synth
    m = S2VTModel.S2VT(50, 64, 8, dim_hid=32, dim_embed=24, rnn_type="gru")
    assert gru_functional.is_gru_model(m)
    assert set(m.state_dict()) == set(synth.gru_param_shapes(50, 64, 32, 24))
    assert all(tuple(v.shape) == synth.gru_param_shapes(50, 64, 32, 24)[k] for k, v in m.state_dict().items())
    with pytest.raises(NotImplementedError):
        m._hip_params()
    feats = torch.randn(2, 8, 64)
    caps = torch.randint(5, 50, (2, 7))
    for mode in ("train", "test", "beam_search"):
        with pytest.raises(capi.S2VTHipError):
            m(feats, targets=caps, mode=mode)
    assert not gru_functional.is_gru_model(S2VTModel.S2VT(50, 64, 8, dim_hid=32, dim_embed=24, rnn_type="gru", num_layers=2))
    assert not gru_functional.is_gru_model(S2VTModel.S2VT(50, 64, 8, dim_hid=32, dim_embed=24))


def test_gru_weight_recipe_is_seeded():
    from s2vt_video_caption_amd import synth
    a = synth.make_gru_state_dict(50, 64, 32, 24, seed=3)
    b = synth.make_gru_state_dict(50, 64, 32, 24, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["vid_rnn.weight_hh_l0"].shape == (96, 32) and a["word_rnn.weight_ih_l0"].shape == (96, 56)
    # one recipe for both layouts: every GRU tensor is the LSTM recipe's tensor of the same key and seed (its first 3H rows for
    # the recurrent ones), so the two cannot drift apart
    lstm = synth.make_state_dict(50, 64, 32, 24, seed=3)
    assert set(a) == set(lstm)
    for k in a:
        assert torch.equal(a[k], lstm[k][:a[k].shape[0]]), k


def test_train_cli_accepts_rnn_type():
    sys.path.insert(0, ROOT)
    import train
    assert train.parse([]).rnn_type == "lstm"
    assert train.parse(["--rnn-type", "gru"]).rnn_type == "gru"


@pytest.mark.parametrize("name", ["gru_tiny", "gru_ragged"])
def test_gru_fixture_agrees_with_the_fp64_replay(name):
    """The generator's fp64 replay of the greedy loop, re-run from the fixture's seeds alone: same margins, its own argmax equals
    the stored reference ids on every row whose margin is >= 1e-5 at every step, and the fixture's count of such rows."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_gru_golden as gen
    g = np.load(os.path.join(GOLD, name + ".npz"))
    d, sd, feats, _, _ = gen.setup(name)
    assert list(g["dims"]) == [d[k] for k in "BLFHEV"] and int(g["seed"]) == d["seed"]
    ids = torch.from_numpy(g["greedy_ids"])
    own, marg = gen.replay_fp64(d, sd, feats, ids)
    assert np.allclose(marg.numpy(), g["greedy_margin"], rtol=0, atol=1e-9)
    robust = (marg >= gen.MARGIN).all(1)
    assert int(robust.sum()) == int(g["n_robust_rows"])
    assert torch.equal(own[robust], ids[robust])
