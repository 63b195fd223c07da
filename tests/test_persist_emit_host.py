"""CPU: the test-support entry points of the persistent split-precision kernels' fused outputs (include/s2vt_hip.h:
s2vt_lstm_seq_fwd_x3_persist_emit, s2vt_lstm_seq_bwd_x3_persist_emit) are declared, exported and bound, and each refuses what the
kernel file's own prep_x / prep_y would refuse of an image - with a message and a non-zero return before any device call
(tests/test_gpu_persist_emit.py runs them on the GPU).  Every call here fails one of those checks: none reaches a launch."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMIT_ENTRIES = ("s2vt_lstm_seq_fwd_x3_persist_emit", "s2vt_lstm_seq_bwd_x3_persist_emit")
P = ctypes.c_void_p(64)          # a non-null, 16-byte aligned pointer that is never dereferenced: the argument checks run first
ODD = ctypes.c_void_p(72)        # ... and one that is only 8-byte aligned


def test_emit_entry_points_declared_exported_and_bound(lib):
    from s2vt_video_caption_amd import capi, ops
    raw = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in EMIT_ENTRIES:
        assert hasattr(raw, name), "libs2vt_hip.so does not export %s" % name
        assert name in capi.SIGNATURES, "capi.py does not bind %s" % name
        assert (name + "(") in header, "include/s2vt_hip.h does not declare %s" % name
    # the forms without emission stay as they were: three / four arguments fewer ... (+ 2 x (image, stride) + flag; + 2 colpart)
    assert len(capi.SIGNATURES["s2vt_lstm_seq_fwd_x3_persist_emit"][1]) == len(capi.SIGNATURES["s2vt_lstm_seq_fwd_x3_persist"][1]) + 5
    assert len(capi.SIGNATURES["s2vt_lstm_seq_bwd_x3_persist_emit"][1]) == len(capi.SIGNATURES["s2vt_lstm_seq_bwd_x3_persist"][1]) + 7
    for wrapper in ("lstm_seq_fwd_persist_emit", "lstm_seq_bwd_persist_emit", "row_plane_image", "lstm_seq_fwd_persist", "lstm_seq_bwd_persist"):
        assert callable(getattr(ops, wrapper))
    assert lib.s2vt_abi_version() == capi.ABI_VERSION


def _rejects(lib, name, rc, text=None):
    assert rc == -1, (name, rc)
    msg = lib.s2vt_last_error().decode()
    assert name in msg and (text or name) in msg, (name, msg)


# T = 3 steps of B = 64 rows, H = 37 units: pad64(H) = 64, so an h row image has rows of at least 192 elements
def _fwd(lib, T=3, B=64, H=37, gx0=P, gx1=None, n_gx=1, bias0=P, bias1=None, w0=P, w1=None, h0=P, h1=None, c0=P, c1=None, hblk0=P,
         ld0=192, hblk1=None, ld1=0, no_stash=0, block=0, ws=P, ws_bytes=1 << 40):
    return lib.s2vt_lstm_seq_fwd_x3_persist_emit(T, B, H, gx0, gx1, n_gx, bias0, bias1, w0, w1, h0, h1, c0, c1, hblk0, ld0, hblk1, ld1,
                                                 no_stash, block, ws, ws_bytes, None)


def test_fwd_emit_rejects_bad_arguments(lib):
    n = "s2vt_lstm_seq_fwd_x3_persist_emit"
    for bad in (dict(T=0), dict(B=0), dict(H=-1), dict(gx0=None), dict(w0=None), dict(h0=None), dict(c0=None), dict(ws=None), dict(n_gx=4),
                dict(n_gx=-1), dict(bias0=None), dict(no_stash=2), dict(no_stash=-1)):
        _rejects(lib, n, _fwd(lib, **bad), "bad arguments")
    img = "the h row image"
    _rejects(lib, n, _fwd(lib, B=96), img)                       # the kernel runs B = 96 (three chains); the image's 64-row blocks do not
    _rejects(lib, n, _fwd(lib, B=32), img)
    _rejects(lib, n, _fwd(lib, ld0=191), img)                    # ldhblk < 3 * pad64(H) (and odd)
    _rejects(lib, n, _fwd(lib, ld0=184), img)                    # ldhblk % 8 == 0 but < 3 * pad64(H)
    _rejects(lib, n, _fwd(lib, ld0=196), img)                    # ldhblk % 8 != 0
    _rejects(lib, n, _fwd(lib, ld0=0), img)
    _rejects(lib, n, _fwd(lib, hblk0=ODD), img)                  # not 16-byte aligned
    _rejects(lib, n, _fwd(lib, H=100, ld0=376), img)             # pad64(100) = 128: 384 elements per row
    _rejects(lib, n, _fwd(lib, H=1024, ld0=3064), img)
    _rejects(lib, n, _fwd(lib, hblk1=P, ld1=192), "second layer that is not there")
    two = dict(gx1=P, bias1=P, w1=P, h1=P, c1=P)
    _rejects(lib, n, _fwd(lib, hblk1=P, ld1=184, **two), img)    # the second layer's image is held to the same rules
    _rejects(lib, n, _fwd(lib, hblk1=ODD, ld1=192, **two), img)
    _rejects(lib, n, _fwd(lib, hblk0=None, ld0=0, hblk1=P, ld1=196, **two), img)
    _rejects(lib, n, _fwd(lib, B=96, hblk0=None, ld0=0, hblk1=P, ld1=192, **two), img)


# H = 72 units: 4H = 288, pad64 = 320, so a dG row image has rows of at least 960 elements
def _bwd(lib, T=3, B=64, H=72, w0=P, w1=None, dh0=P, dh1=None, dh_first=0, c0=P, c1=None, st0=P, st1=None, dgp0=P, ld0=960, dgp1=None,
         ld1=0, cp0=P, cp1=None, skip_dg=0, block=0, ws=P, ws_bytes=1 << 40):
    return lib.s2vt_lstm_seq_bwd_x3_persist_emit(T, B, H, w0, w1, dh0, dh1, dh_first, c0, c1, st0, st1, dgp0, ld0, dgp1, ld1, cp0, cp1,
                                                 skip_dg, block, ws, ws_bytes, None)


def test_bwd_emit_rejects_bad_arguments(lib):
    n = "s2vt_lstm_seq_bwd_x3_persist_emit"
    for bad in (dict(T=0), dict(B=-64), dict(H=0), dict(w0=None), dict(c0=None), dict(st0=None), dict(ws=None), dict(dh_first=-1),
                dict(skip_dg=2), dict(skip_dg=-1)):
        _rejects(lib, n, _bwd(lib, **bad), "bad arguments")
    img = "the dG row image needs B"
    _rejects(lib, n, _bwd(lib, H=44, ld0=576), "H % 8 == 0")     # the kernel runs H = 44; 16-byte pieces of the image need H % 8 == 0
    _rejects(lib, n, _bwd(lib, H=37, ld0=576), "H % 8 == 0")
    _rejects(lib, n, _bwd(lib, H=1001, ld0=12096), "H % 8 == 0")
    _rejects(lib, n, _bwd(lib, B=96), img)                       # the kernel runs B = 96; the image's 64-row blocks do not
    _rejects(lib, n, _bwd(lib, B=32), img)
    _rejects(lib, n, _bwd(lib, ld0=959), img)                    # lddgp < 3 * pad64(4H) (and odd)
    _rejects(lib, n, _bwd(lib, ld0=952), img)                    # lddgp % 8 == 0 but < 3 * pad64(4H)
    _rejects(lib, n, _bwd(lib, ld0=864), img)                    # 3 * 4H, without the k padding
    _rejects(lib, n, _bwd(lib, ld0=964), img)                    # lddgp % 8 != 0
    _rejects(lib, n, _bwd(lib, dgp0=ODD), img)                   # not 16-byte aligned
    _rejects(lib, n, _bwd(lib, dgp0=None, ld0=0, skip_dg=1), "skip_dg without")
    _rejects(lib, n, _bwd(lib, dgp0=None, ld0=0, cp0=None, skip_dg=1), "skip_dg without")
    _rejects(lib, n, _bwd(lib, dgp1=P, ld1=960), "second layer that is not there")
    _rejects(lib, n, _bwd(lib, cp1=P), "second layer that is not there")
    two = dict(w1=P, dh1=P, c1=P, st1=P)
    _rejects(lib, n, _bwd(lib, skip_dg=1, **two), "skip_dg without")                     # ... for EVERY layer of the launch
    _rejects(lib, n, _bwd(lib, dgp1=P, ld1=952, **two), img)
    _rejects(lib, n, _bwd(lib, dgp1=ODD, ld1=960, **two), img)
    _rejects(lib, n, _bwd(lib, H=44, dgp0=None, ld0=0, dgp1=P, ld1=576, **two), "H % 8 == 0")
    _rejects(lib, n, _bwd(lib, B=96, dgp0=None, ld0=0, dgp1=P, ld1=960, **two), img)


def test_entries_without_emission_keep_their_names_in_messages(lib):
    """s2vt_lstm_seq_{fwd,bwd}_x3_persist are the same bodies with the new fields null: their refusals still name them."""
    rc = lib.s2vt_lstm_seq_fwd_x3_persist(0, 64, 37, P, None, 1, P, None, P, None, P, None, P, None, 0, P, 1 << 40, None)
    assert rc == -1 and lib.s2vt_last_error().decode() == "s2vt_lstm_seq_fwd_x3_persist: bad arguments"
    rc = lib.s2vt_lstm_seq_bwd_x3_persist(3, 64, 72, None, None, P, None, 0, P, None, P, None, 0, P, 1 << 40, None)
    assert rc == -1 and lib.s2vt_last_error().decode() == "s2vt_lstm_seq_bwd_x3_persist: bad arguments"
