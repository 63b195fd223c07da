"""GPU: the fp32 -> bf16 plane split (csrc/split.hip) against the HOST split of tests/plane_ref.py, bit for bit, read back through the
header's layout formulas - the reference every "bit-equal to ops.split_planes" assertion of the suite rests on.

s2vt_split_planes is called directly: ops.split_planes makes its input contiguous and zero-allocates its output, which hides the
input's row stride and what the kernel writes.  The output image is pre-filled with PLANE_SENT (0x7FFF, a NaN pattern split3 makes
from no finite input), is 8 elements wider than needed (ldo = nplanes*kpad + 8) and has 64 rows more than ceil64(operand rows);
out_rows_pad = ceil64(operand rows).  The region each kernel writes, as read from split.hip:

  3 planes (split_dual_kernel<3, false>, either orientation): operand rows r < operand rows, k < kpad, all three planes - the k
      padding [K, kpad) of those rows as zero bits; the rows [operand rows, ceil64) of the last 64-row block are NOT written (their
      slots keep the sentinel), nor are the 8 spare elements per row of the wider stride (64 * 8 per 64-row block);
  1 plane, rows (split_rows_kernel<1>): r < out_rows_pad, k < kpad - zero bits outside (r < rows, k < K);
  1 plane, transposed (split_transpose_kernel<1>): r < out_rows_pad, k < kpad likewise.

Inputs: views with row stride cols, cols + 1 and cols + 2, and a contiguous matrix whose base is 4 bytes past a 16-byte boundary.
The kernels' 16-byte loads need ld % 4 == 0 and a 16-byte aligned base: they are on at (64, 64) with ld = 64 and at (130, 70) with
ld = 72 (a stride wider than the row), off for every other stride here and for the shifted base; both ways must give the same bits.
Values: randn * 2^U[-100, 100) with the edge list (ties to even both ways, the carry into the exponent, -0.0, bf16-exact values) at
the start, and one all-integer matrix."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (64, 64), (130, 70), (200, 129)]
INPUTS = ["ld+0", "ld+1", "ld+2", "base+4"]


def _values(rows, cols, kind):
    if kind == "range":
        return P.split_values(rows, cols, seed=rows * 1000 + cols)
    return np.random.default_rng(rows + cols).integers(-300, 301, (rows, cols)).astype(np.float32)


def _device_input(x, how):
    """x on the device as the view `how` names; returns (view, row stride)"""
    rows, cols = x.shape
    xt = torch.from_numpy(x)
    if how == "base+4":
        store = torch.full((rows * cols + 1,), 7.0, device=DEV)
        v = store[1:].view(rows, cols)
        assert v.data_ptr() % 16 == 4
    else:
        ld = cols + int(how[3:])
        store = torch.full((rows, ld), 7.0, device=DEV)
        v = store[:, :cols]
        assert v.data_ptr() % 16 == 0
    v.copy_(xt)
    assert v.stride(1) == 1
    return v, v.stride(0)


def _expected(x, nplanes, transpose, ldo, out_rows_pad):
    """the whole expected image (sentinel where nothing may be written)"""
    op = x.T if transpose else x
    if nplanes == 3:
        img = P.build_image(P.split3(op), ld=ldo, extra_rows=64, fill=P.PLANE_SENT).numpy().view(np.uint16).copy()
        flat = img.reshape(-1)
        orows, K = op.shape
        if orows < P.pad64(orows):        # rows of the last block beyond the operand: build_image zero-fills them, the kernel skips them
            flat[P.plane_index(P.pad64(orows), P.pad64(K), ldo)[orows:].reshape(-1)] = P.PLANE_SENT
        return img
    return P.build_row_image(P.bf16_rn_bits(op), ld=ldo, extra_rows=64, fill=P.PLANE_SENT, rows_pad=out_rows_pad).numpy().view(np.uint16)


@pytest.mark.parametrize("how", INPUTS)
@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("nplanes", [3, 1])
def test_split_planes_bits_padding_and_untouched_elements(lib, nplanes, transpose, rows, cols, how):
    """Every data element has the host split3 bits (bf16_rn_bits for one plane), the k padding of written rows is zero bits, and
    everything else - see the module docstring for each kernel's written region - still holds the sentinel: the whole image is
    compared with one built on the host."""
    from s2vt_video_caption_amd import capi
    from s2vt_video_caption_amd.functional import _ptr, _stream
    orows, K = (cols, rows) if transpose else (rows, cols)
    kpad, out_rows_pad = P.pad64(K), P.pad64(orows)
    ldo = nplanes * kpad + 8
    for kind in ("range", "integers"):
        x = _values(rows, cols, kind)
        v, ld = _device_input(x, how)
        out = torch.full((out_rows_pad + 64, ldo), P.PLANE_SENT, dtype=torch.int16, device=DEV)
        capi.check(lib.s2vt_split_planes(nplanes, transpose, _ptr(v), ld, rows, cols, _ptr(out), ldo, kpad, out_rows_pad,
                                         _stream(torch.device(DEV))), "s2vt_split_planes")
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        want = _expected(x, nplanes, transpose, ldo, out_rows_pad)
        assert got.shape == want.shape
        bad = got != want
        assert not bad.any(), "%s, %s: %d image elements differ, first (image row, column) = %s: got 0x%04x, want 0x%04x" % (
            how, kind, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])
        if nplanes == 3:                  # and once more through read_image: the data elements alone, by plane
            op = x.T if transpose else x
            for pl, (a, b) in enumerate(zip(P.read_image(got, orows, K, ld=ldo), P.split3(op))):
                assert np.array_equal(a, b), pl
    capi.check_async_error()


def _stored(rows, inner, outer):
    r = np.arange(rows)
    return (r % inner) * outer + r // inner


@pytest.mark.parametrize("nplanes", [3, 1])
@pytest.mark.parametrize("mapping", ["rowmap", "gather"])
def test_split_planes_dual_against_the_host_split_of_the_mapped_matrix(lib, nplanes, mapping):
    """s2vt_split_planes_dual through ops.split_planes_dual (zero-allocated images of the natural width), row planes and transposed
    planes of one call, with rowmap = (inner, outer) and with a gather index that repeats and skips rows: the images are those of
    the HOST split of the mapped matrix - test_gpu_backward_aux.py compares this entry with ops.split_planes, i.e. with itself."""
    from s2vt_video_caption_amd import ops
    rows, cols = 135, 70
    x = P.split_values(rows, cols, seed=77)
    if mapping == "rowmap":
        inner, outer = 27, 5
        rowmap, src = (inner, outer), _stored(rows, inner, outer)
    else:
        src = np.random.default_rng(8).integers(0, rows, 150)
        src[:3] = [rows - 1, 0, rows - 1]
        rowmap = torch.from_numpy(src.astype(np.int32)).to(DEV)
    mat = x[src]
    res = ops.split_planes_dual(torch.from_numpy(x).to(DEV), nplanes, rowmap=rowmap, want_r=True, want_t=True)
    for key, op in (("r", mat), ("t", np.ascontiguousarray(mat.T))):
        if nplanes == 3:
            want = P.build_image(P.split3(op))
        else:
            want = P.build_row_image(P.bf16_rn_bits(op))
        got = res[key].cpu()
        assert got.shape == want.shape, key
        assert torch.equal(got, want), "%s planes: %d elements differ from the host split" % (key, int((got != want).sum()))
