"""CPU: the test-support entry points of the decode step's kernel forms (include/s2vt_hip.h: s2vt_lstm_step_fwd_table,
s2vt_lstm_cell_pointwise, s2vt_argmax_x3_planes) are declared, exported and bound, and each refuses bad arguments with a message
and a non-zero return before any device call (tests/test_gpu_decode_forms.py runs them on the GPU)."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_ENTRIES = ("s2vt_lstm_step_fwd_table", "s2vt_lstm_cell_pointwise", "s2vt_argmax_x3_planes")
P = ctypes.c_void_p(64)          # a non-null, 16-byte aligned pointer that is never dereferenced: the argument checks run first
ODD = ctypes.c_void_p(72)        # ... and one that is only 8-byte aligned


def test_form_entry_points_declared_exported_and_bound(lib):
    from s2vt_video_caption_amd import capi, ops
    raw = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in FORM_ENTRIES:
        assert hasattr(raw, name), "libs2vt_hip.so does not export %s" % name
        assert name in capi.SIGNATURES, "capi.py does not bind %s" % name
        assert (name + "(") in header, "include/s2vt_hip.h does not declare %s" % name
    for wrapper in ("lstm_step_fwd_table", "lstm_step_contract", "lstm_cell_pointwise", "argmax_x3_planes", "h_plane_image"):
        assert callable(getattr(ops, wrapper))
    assert lib.s2vt_abi_version() == capi.ABI_VERSION


def _rejects(lib, name, rc, text=None):
    assert rc == -1, (name, rc)
    msg = lib.s2vt_last_error().decode()
    assert (text or name) in msg, (name, msg)


# B = 5 rows of H = 44 units: pad64(H) = 64, so an h-plane image has 64 rows of at least 192 elements
def _step(lib, B=5, H=44, V=50, gx=P, gx_idx=None, bias=None, gtab=P, ldtab=176, tok=P, w_hh=P, h_prev=P, c_prev=P, h_out=P, c_out=P,
          stash=None, hp=None, ldhp=0, hp_rows=0, z=None, ldz=0, contract=0):
    return lib.s2vt_lstm_step_fwd_table(B, H, V, gx, gx_idx, bias, gtab, ldtab, tok, None, 0, w_hh, h_prev, c_prev, h_out, c_out, stash,
                                        hp, ldhp, hp_rows, z, ldz, contract, None)


def test_step_fwd_table_rejects_bad_arguments(lib):
    n = "s2vt_lstm_step_fwd_table"
    _rejects(lib, n, _step(lib, B=0))
    _rejects(lib, n, _step(lib, H=-1))
    _rejects(lib, n, _step(lib, h_out=None))
    _rejects(lib, n, _step(lib, c_out=None))
    _rejects(lib, n, _step(lib, gx=None))                                                # neither gx nor bias
    _rejects(lib, n, _step(lib, gx=None, bias=P, gx_idx=P), "gx_idx")                    # an index into rows that are not there
    _rejects(lib, n, _step(lib, V=0), "gate table")
    _rejects(lib, n, _step(lib, ldtab=175), "gate table")                                # table rows shorter than 4H
    _rejects(lib, n, _step(lib, w_hh=None), "h_prev without w_hh")
    _rejects(lib, n, _step(lib, z=P, ldz=176), "contract_only")                          # z_out belongs to the other mode
    img = dict(hp=P, ldhp=192, hp_rows=64)
    _rejects(lib, n, _step(lib, **dict(img, ldhp=191)), "h-plane image")                 # ldhp < 3 * pad64(H) (and odd)
    _rejects(lib, n, _step(lib, **dict(img, ldhp=184)), "h-plane image")                 # ldhp % 8 == 0 but < 3 * pad64(H)
    _rejects(lib, n, _step(lib, **dict(img, ldhp=196)), "h-plane image")                 # ldhp % 8 != 0
    _rejects(lib, n, _step(lib, **dict(img, hp=ODD)), "h-plane image")                   # not 16-byte aligned
    _rejects(lib, n, _step(lib, B=65, **img), "h-plane image")                           # 65 rows need two 64-row blocks
    _rejects(lib, n, _step(lib, H=100, ldtab=400, **img), "h-plane image")               # pad64(100) = 128: 384 elements per row
    # contraction only: w_hh, h_prev, z_out and ldz >= 4H
    c = dict(contract=1, z=P, ldz=176)
    _rejects(lib, n, _step(lib, **dict(c, z=None)), "contraction-only")
    _rejects(lib, n, _step(lib, **dict(c, ldz=175)), "contraction-only")
    _rejects(lib, n, _step(lib, **dict(c, h_prev=None)), "contraction-only")
    _rejects(lib, n, _step(lib, **dict(c, w_hh=None)), "contraction-only")
    _rejects(lib, n, _step(lib, **dict(c, B=0)), "contraction-only")


def _cell(lib, B=5, H=44, V=50, gx=P, gx_idx=None, bias=None, gtab=P, ldtab=176, tok=P, z=P, ldz=176, c_prev=P, h_out=P, c_out=P, hp=None,
          ldhp=0, hp_rows=0):
    return lib.s2vt_lstm_cell_pointwise(B, H, V, gx, gx_idx, bias, gtab, ldtab, tok, None, 0, z, ldz, c_prev, h_out, c_out, None, hp, ldhp,
                                        hp_rows, None)


def test_cell_pointwise_rejects_bad_arguments(lib):
    n = "s2vt_lstm_cell_pointwise"
    _rejects(lib, n, _cell(lib, B=0))
    _rejects(lib, n, _cell(lib, h_out=None))
    _rejects(lib, n, _cell(lib, c_out=None))
    _rejects(lib, n, _cell(lib, gx=None))
    _rejects(lib, n, _cell(lib, gx=None, bias=P, gx_idx=P), "gx_idx")
    _rejects(lib, n, _cell(lib, V=0), "gate table")
    _rejects(lib, n, _cell(lib, ldtab=100), "gate table")
    _rejects(lib, n, _cell(lib, z=None), "z is null")
    _rejects(lib, n, _cell(lib, ldz=175), "z is null")
    _rejects(lib, n, _cell(lib, hp=P, ldhp=192, hp_rows=0), "h-plane image")
    _rejects(lib, n, _cell(lib, hp=P, ldhp=190, hp_rows=64), "h-plane image")
    _rejects(lib, n, _cell(lib, hp=P, ldhp=200, hp_rows=64, H=100, ldtab=400, ldz=400), "h-plane image")
    _rejects(lib, n, _cell(lib, hp=ODD, ldhp=192, hp_rows=64), "h-plane image")


# B = 37 rows, V = 130 vocabulary rows, K = 64, a second image of M2 = 61 rows
def _amax(lib, B=37, V=130, K=64, W=P, ldw=192, w_rows=192, Hp=P, ldh=192, kh=64, hp_rows=64, packed=P, W2=P, ldw2=192, kw2=64, w2_rows=64,
          M2=61, z=P, ldz=64, with_logits=1, sample=0, temperature=1.0, step=0, row0=0):
    return lib.s2vt_argmax_x3_planes(B, V, K, W, ldw, w_rows, Hp, ldh, kh, hp_rows, None, packed, W2, ldw2, kw2, w2_rows, M2, z, ldz,
                                     with_logits, sample, temperature, 7, step, row0, None)


def test_argmax_x3_planes_rejects_bad_arguments(lib):
    n = "s2vt_argmax_x3_planes"
    _rejects(lib, n, _amax(lib, B=0))
    _rejects(lib, n, _amax(lib, V=0))
    _rejects(lib, n, _amax(lib, K=96))                                                   # K % 64
    _rejects(lib, n, _amax(lib, W=None))
    _rejects(lib, n, _amax(lib, Hp=None))
    _rejects(lib, n, _amax(lib, packed=None))
    _rejects(lib, n, _amax(lib, M2=-1))
    _rejects(lib, n, _amax(lib, kh=128), "one padded k")
    _rejects(lib, n, _amax(lib, kw2=128), "one padded k")
    _rejects(lib, n, _amax(lib, w_rows=128), "fewer rows")                               # V = 130 reads three 64-row blocks
    _rejects(lib, n, _amax(lib, hp_rows=0), "fewer rows")
    _rejects(lib, n, _amax(lib, B=65, hp_rows=64), "fewer rows")
    _rejects(lib, n, _amax(lib, M2=65, ldz=68), "fewer rows")                            # W2 of 64 rows, M2 = 65 reads two blocks
    _rejects(lib, n, _amax(lib, with_logits=0, M2=0), "with_logits = 0")
    _rejects(lib, n, _amax(lib, with_logits=0, sample=1), "a draw needs the logits")
    _rejects(lib, n, _amax(lib, sample=1, step=-1), "a draw needs the logits")
    _rejects(lib, n, _amax(lib, sample=1, row0=-1), "a draw needs the logits")
    for t in (0.0, -1.0, float("inf"), float("nan"), 1e-45):
        _rejects(lib, n, _amax(lib, sample=1, temperature=t), "temperature")
    # what the launcher itself requires of the geometry, with its own messages
    _rejects(lib, n, _amax(lib, ldw=190), "logits_argmax_x3: operands must be blocked 3-plane images")
    _rejects(lib, n, _amax(lib, ldh=196), "logits_argmax_x3: operands must be blocked 3-plane images")
    _rejects(lib, n, _amax(lib, Hp=ODD), "logits_argmax_x3: operands must be blocked 3-plane images")
    _rejects(lib, n, _amax(lib, W2=None), "logits_argmax_x3: the second image")
    _rejects(lib, n, _amax(lib, z=None), "logits_argmax_x3: the second image")
    _rejects(lib, n, _amax(lib, ldz=60), "logits_argmax_x3: the second image")           # ldz < M2
    _rejects(lib, n, _amax(lib, ldz=62), "logits_argmax_x3: the second image")           # ldz % 4
    _rejects(lib, n, _amax(lib, z=ODD), "logits_argmax_x3: the second image")
    _rejects(lib, n, _amax(lib, ldw2=188), "logits_argmax_x3: the second image")
