"""CPU: the test-support entry points of the backward's gather / scatter / reorder kernels (include/s2vt_hip.h:
s2vt_gemm_f32_mapped, s2vt_embedding_grad, s2vt_gather_rows, s2vt_transpose_f32, s2vt_colsum, s2vt_colsum_finish,
s2vt_split_planes_dual) are declared, exported and bound, and each refuses bad arguments with a message and a non-zero return
before any device call (tests/test_gpu_backward_aux.py runs them on the GPU)."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUX_ENTRIES = ("s2vt_gemm_f32_mapped", "s2vt_embedding_grad", "s2vt_embedding_grad_ws_ints", "s2vt_gather_rows", "s2vt_transpose_f32",
               "s2vt_colsum", "s2vt_colsum_finish", "s2vt_split_planes_dual")
P = ctypes.c_void_p(64)          # a non-null, 16-byte aligned pointer that is never dereferenced: the argument checks run first


def test_aux_entry_points_declared_exported_and_bound(lib):
    from s2vt_video_caption_amd import capi, ops
    raw = ctypes.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    for name in AUX_ENTRIES:
        assert hasattr(raw, name), "libs2vt_hip.so does not export %s" % name
        assert name in capi.SIGNATURES, "capi.py does not bind %s" % name
        assert (name + "(") in header, "include/s2vt_hip.h does not declare %s" % name
    for wrapper in ("gemm_mapped", "embedding_grad", "gather_rows", "transpose", "colsum", "colsum_finish", "split_planes_dual"):
        assert callable(getattr(ops, wrapper))
    assert lib.s2vt_abi_version() == capi.ABI_VERSION


def test_scratch_size_queries(lib):
    # heavy-token list (rows / 64 + 2) + its counter + one count per token; one partial row per 64-row chunk
    assert lib.s2vt_embedding_grad_ws_ints(20037, 50) == 20037 // 64 + 2 + 1 + 50
    assert lib.s2vt_embedding_grad_ws_ints(0, 50) == 2 + 1 + 50
    assert lib.s2vt_embedding_grad_ws_ints(-1, 50) == 0 and lib.s2vt_embedding_grad_ws_ints(10, 0) == 0
    assert lib.s2vt_colsum_ws_floats(4097, 17) == 65 * 17


def _rejects(lib, name, rc, text=None):
    assert rc == -1, (name, rc)
    msg = lib.s2vt_last_error().decode()
    assert (text or name) in msg, (name, msg)


def _gemm(lib, ak=1, bk=1, M=8, N=8, K=8, A=P, lda=8, am=(None, 0, 0), B=P, ldb=8, bm=(None, 0, 0), C=P, ldc=8, cm=(None, 0, 0),
          ws=None, ws_floats=0, cap=0):
    return lib.s2vt_gemm_f32_mapped(ak, bk, M, N, K, A, lda, *am, B, ldb, *bm, C, ldc, *cm, None, 0, ws, ws_floats, cap, None)


def test_gemm_mapped_rejects_bad_arguments(lib):
    n = "s2vt_gemm_f32_mapped"
    _rejects(lib, n, _gemm(lib, A=None))
    _rejects(lib, n, _gemm(lib, C=None))
    _rejects(lib, n, _gemm(lib, M=0))
    _rejects(lib, n, _gemm(lib, K=-3))
    _rejects(lib, n, _gemm(lib, lda=7), "row stride")
    _rejects(lib, n, _gemm(lib, ldc=7), "row stride")
    _rejects(lib, n, _gemm(lib, ak=0, bk=0, M=12, lda=8), "row stride")                  # A^T stored: rows of M elements
    _rejects(lib, n, _gemm(lib, cm=(None, 3, 3)), "row map")                             # 3 * 3 != M
    _rejects(lib, n, _gemm(lib, am=(P, 2, 4)), "row map")                                # an index AND a permutation
    _rejects(lib, n, _gemm(lib, bm=(None, 0, 4)), "row map")                             # outer without inner
    _rejects(lib, n, _gemm(lib, ak=0, bk=0, am=(None, 2, 3)), "row map")                 # permutes the K = 8 stored rows of A^T
    _rejects(lib, n, _gemm(lib, ws=None, ws_floats=64), "scratch")
    _rejects(lib, n, _gemm(lib, ws=P, ws_floats=64, cap=-1), "scratch")
    # a gather on an operand whose stored rows are k: refused by the launcher itself, with its own message
    _rejects(lib, n, _gemm(lib, ak=0, bk=0, am=(P, 0, 0)), "gemm_f32: a gather index is only supported on operands whose stored rows are m / n")
    _rejects(lib, n, _gemm(lib, ak=1, bk=0, bm=(P, 0, 0)), "gemm_f32: a gather index is only supported on operands whose stored rows are m / n")
    _rejects(lib, n, _gemm(lib, ak=0, bk=1), "gemm_f32: A^T * B^T form")


def test_embedding_grad_rejects_bad_arguments(lib):
    n = "s2vt_embedding_grad"
    need = lib.s2vt_embedding_grad_ws_ints(100, 50)
    _rejects(lib, n, lib.s2vt_embedding_grad(None, 100, 24, P, 50, P, P, need, None))     # rows without d_rows
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 100, 24, None, 50, P, P, need, None))     # rows without tok
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 100, 24, P, 50, None, P, need, None))
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 100, 24, P, 50, P, None, need, None))
    _rejects(lib, n, lib.s2vt_embedding_grad(P, -1, 24, P, 50, P, P, need, None))
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 2 ** 31, 24, P, 50, P, P, 2 ** 30, None))
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 100, 0, P, 50, P, P, need, None))
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 100, 24, P, 0, P, P, need, None))
    _rejects(lib, n, lib.s2vt_embedding_grad(P, 100, 24, P, 50, P, P, need - 1, None), "scratch")


def test_row_kernels_reject_bad_arguments(lib):
    _rejects(lib, "s2vt_gather_rows", lib.s2vt_gather_rows(None, 8, P, 4, 8, P, None))
    _rejects(lib, "s2vt_gather_rows", lib.s2vt_gather_rows(P, 8, None, 4, 8, P, None))
    _rejects(lib, "s2vt_gather_rows", lib.s2vt_gather_rows(P, 8, P, 4, 8, None, None))
    _rejects(lib, "s2vt_gather_rows", lib.s2vt_gather_rows(P, 7, P, 4, 8, P, None))       # ld < cols
    _rejects(lib, "s2vt_gather_rows", lib.s2vt_gather_rows(P, 8, P, 0, 8, P, None))
    _rejects(lib, "s2vt_gather_rows", lib.s2vt_gather_rows(P, 8, P, 65536, 8, P, None))   # one grid row per output row
    _rejects(lib, "s2vt_transpose_f32", lib.s2vt_transpose_f32(None, 4, 4, P, None))
    _rejects(lib, "s2vt_transpose_f32", lib.s2vt_transpose_f32(P, 4, 4, None, None))
    _rejects(lib, "s2vt_transpose_f32", lib.s2vt_transpose_f32(P, 4, 4, P, None))         # in place
    _rejects(lib, "s2vt_transpose_f32", lib.s2vt_transpose_f32(P, 0, 4, ctypes.c_void_p(128), None))
    need = lib.s2vt_colsum_ws_floats(130, 70)
    _rejects(lib, "s2vt_colsum", lib.s2vt_colsum(None, 130, 70, 70, P, need, P, 0, None))
    _rejects(lib, "s2vt_colsum", lib.s2vt_colsum(P, 130, 70, 70, None, need, P, 0, None))
    _rejects(lib, "s2vt_colsum", lib.s2vt_colsum(P, 130, 70, 70, P, need, None, 0, None))
    _rejects(lib, "s2vt_colsum", lib.s2vt_colsum(P, 130, 70, 69, P, need, P, 0, None))    # ld < cols
    _rejects(lib, "s2vt_colsum", lib.s2vt_colsum(P, 0, 70, 70, P, need, P, 0, None))
    _rejects(lib, "s2vt_colsum", lib.s2vt_colsum(P, 130, 70, 70, P, need - 1, P, 0, None), "scratch")
    _rejects(lib, "s2vt_colsum_finish", lib.s2vt_colsum_finish(None, 3, 70, P, 0, None))
    _rejects(lib, "s2vt_colsum_finish", lib.s2vt_colsum_finish(P, 3, 70, None, 0, None))
    _rejects(lib, "s2vt_colsum_finish", lib.s2vt_colsum_finish(P, 0, 70, P, 0, None))
    _rejects(lib, "s2vt_colsum_finish", lib.s2vt_colsum_finish(P, 3, 0, P, 0, None))


def _dual(lib, nplanes=3, x=P, ld=70, rm=(None, 0, 0), rows=130, cols=70, out_r=P, ldo_r=384, kpad_r=128, out_t=None, ldo_t=0, kpad_t=0,
          colpart=None, lse=None, target=None, ldt=0, Lm1=0, gout=None, alpha=None):
    return lib.s2vt_split_planes_dual(nplanes, x, ld, *rm, rows, cols, out_r, ldo_r, kpad_r, out_t, ldo_t, kpad_t, colpart, lse, target,
                                      ldt, Lm1, gout, alpha, None)


def test_split_planes_dual_rejects_bad_arguments(lib):
    n = "s2vt_split_planes_dual"
    _rejects(lib, n, _dual(lib, nplanes=2))
    _rejects(lib, n, _dual(lib, x=None))
    _rejects(lib, n, _dual(lib, out_r=None))                                             # no output at all
    _rejects(lib, n, _dual(lib, ld=69))
    _rejects(lib, n, _dual(lib, rows=0))
    _rejects(lib, n, _dual(lib, rm=(None, 10, 12)), "row map")                           # 120 != 130 rows
    _rejects(lib, n, _dual(lib, rm=(P, 10, 13)), "row map")
    _rejects(lib, n, _dual(lib, kpad_r=64, ldo_r=192), "plane geometry")                 # kpad < cols
    _rejects(lib, n, _dual(lib, kpad_r=192, ldo_r=576), "plane geometry")                # kpad beyond the last column tile
    _rejects(lib, n, _dual(lib, kpad_r=128, ldo_r=380), "plane geometry")                # ldo < 3 * kpad
    _rejects(lib, n, _dual(lib, out_r=ctypes.c_void_p(72)), "plane geometry")            # not 16-byte aligned
    _rejects(lib, n, _dual(lib, out_t=P, kpad_t=128, ldo_t=384), "plane geometry")       # kpad_t < rows
    _rejects(lib, n, _dual(lib, nplanes=1, ldo_r=128, out_t=P, kpad_t=192, ldo_t=190), "plane geometry")
    ce = dict(rows=135, lse=P, target=P, ldt=28, Lm1=27, gout=P, kpad_r=128)
    _rejects(lib, n, _dual(lib, **dict(ce, lse=None)), "CE-gradient")
    _rejects(lib, n, _dual(lib, **dict(ce, target=None)), "CE-gradient")
    _rejects(lib, n, _dual(lib, **dict(ce, gout=None)), "CE-gradient")
    _rejects(lib, n, _dual(lib, **dict(ce, Lm1=0)), "CE-gradient")
    _rejects(lib, n, _dual(lib, **dict(ce, Lm1=26)), "CE-gradient")                      # rows is not B * Lm1
    _rejects(lib, n, _dual(lib, **dict(ce, ldt=27)), "CE-gradient")                      # target rows hold Lm1 + 1 ids
    _rejects(lib, n, _dual(lib, **dict(ce, rm=(None, 5, 27))), "CE-gradient")            # the CE rows are not mapped
    _rejects(lib, n, _dual(lib, alpha=P), "CE-gradient")                                 # alpha_out without the CE transform
