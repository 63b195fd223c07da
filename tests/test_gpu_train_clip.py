"""GPU: train.py --grad-clip / --weight-decay / --adamw / --no-decay-bias / --skip-nonfinite through the harness on the toy data set of
tests/test_train_eval_parity.py: the flags reach optim.FlatAdam (one-layer LSTM) or torch's clip_grad_norm_ + Adam / AdamW (GRU), the
history gains `grad_norm` / `skipped_steps` only when asked, and the loss still falls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_train_eval_parity import BS, E, F, H, L, LR, ROOT, SEED, make_toy  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(tmp_path, *flags, epochs=3):
    sys.path.insert(0, ROOT)
    import train
    make_toy(str(tmp_path))
    opt = train.parse(["--caption-file", str(tmp_path / "captions.json"), "--feats-path", str(tmp_path / "feats"),
                       "--train-length", str(L), "--dim-hidden", str(H), "--dim-embed", str(E), "--feat-dim", str(F),
                       "--batch-size", str(BS), "--epochs", str(epochs), "--lr", str(LR), "--save-freq", "100",
                       "--save-path", str(tmp_path / "ck"), "--no-shuffle", "--seed", str(SEED)] + list(flags))
    return train.run(opt)


def test_train_flags_reach_flat_adam(tmp_path, capsys):
    got = _run(tmp_path, "--grad-clip", "0.25", "--weight-decay", "5e-5", "--adamw", "--no-decay-bias", "--skip-nonfinite")
    tl, gn = got["train_loss"], got["grad_norm"]
    assert len(tl) == 3 and all(np.isfinite(tl)) and tl[-1] < tl[0], tl
    assert len(gn) == 3 and all(np.isfinite(gn)) and all(x > 0.25 for x in gn), gn      # a fresh model's gradient norm is O(1): the clip acts
    assert got["skipped_steps"] == [0, 0, 0]
    out = capsys.readouterr().out
    assert "grad norm: %s skipped steps: 0" % gn[0] in out


def test_train_flags_reach_torch_adam_for_the_gru(tmp_path):
    got = _run(tmp_path, "--rnn-type", "gru", "--grad-clip", "0.25", "--weight-decay", "5e-5", "--adamw", "--no-decay-bias")
    tl, gn = got["train_loss"], got["grad_norm"]
    assert len(tl) == 3 and all(np.isfinite(tl)) and tl[-1] < tl[0], tl
    assert len(gn) == 3 and all(np.isfinite(gn)) and all(x > 0.25 for x in gn), gn
    assert got["skipped_steps"] == [0, 0, 0]


def test_history_keys_appear_only_with_a_flag(tmp_path):
    got = _run(tmp_path, "--weight-decay", "5e-5", epochs=1)
    assert "grad_norm" not in got and "skipped_steps" not in got
    assert np.isfinite(got["train_loss"][0])
