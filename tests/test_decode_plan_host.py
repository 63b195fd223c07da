"""CPU: the workspace / cache layouts of the decode, beam and train drivers against a table recorded from the build before the decode
driver was split into one function per schedule (tests/golden/workspace_layout.json), and the argument checks of s2vt_decode_plan.
No device is needed: the size functions make no device query.

Recording the table (with the library whose layout is the reference):
    S2VT_LIB=<library> python tests/test_decode_plan_host.py tests/golden/workspace_layout.json"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_layout.json")

OPTIONS = ("gemm_mode", "pipe_block", "persist", "pad_min_batch")
OPTION_VALUES = ((0, 1, 3), (0, 32), (0, 1), (1, 33))
BATCHES = (1, 10, 16, 24, 40, 64, 100, 128, 192)
HIDDEN = (44, 512, 1000, 1100)
LFEV = ((5, 70, 28, 61), (80, 4096, 500, 12000))       # (L, F, E, V): a test-sized set and the flagship's


def layout_table(lib, capi):
    """{"gemm_mode,pipe_block,persist,pad_min_batch": [[decode workspace, decode cache, beam workspace (5 rows per clip), train workspace]
    for every (L, F, E, V) x H x B in the order of the constants above]}; the options are put back afterwards"""
    before = [lib.s2vt_set_option(n.encode(), -1) for n in OPTIONS]
    table = {}
    try:
        for values in itertools.product(*OPTION_VALUES):
            for n, v in zip(OPTIONS, values):
                lib.s2vt_set_option(n.encode(), v)
            rows = []
            for (L, F, E, V), H, B in itertools.product(LFEV, HIDDEN, BATCHES):
                d = capi.Dims(B, L, F, H, E, V)
                rows.append([lib.s2vt_decode_workspace_bytes(d), lib.s2vt_decode_cache_bytes(d), lib.s2vt_beam_workspace_bytes(d, 5 * B),
                             lib.s2vt_train_workspace_bytes(d)])
            table[",".join(str(v) for v in values)] = rows
    finally:
        for n, v in zip(OPTIONS, before):
            lib.s2vt_set_option(n.encode(), v)
    return table


def test_workspace_and_cache_layouts_are_the_recorded_ones(lib):
    from s2vt_video_caption_amd import capi
    with open(GOLDEN) as f:
        want = json.load(f)
    got = layout_table(lib, capi)
    assert sorted(got) == sorted(want) and len(want) == 24
    shapes = list(itertools.product(LFEV, HIDDEN, BATCHES))
    for key in want:
        assert len(got[key]) == len(want[key]) == len(shapes)
        for shape, g, w in zip(shapes, got[key], want[key]):
            assert g == w and g[0] > 0 and g[2] > 0 and g[3] > 0, (key, shape, g, w)     # (the cache is empty in gemm mode 0)


def _last_error(lib):
    msg = lib.s2vt_last_error()
    return msg.decode() if msg else ""


def test_decode_plan_declared_bound_and_exported(lib):
    from s2vt_video_caption_amd import capi
    header = open(os.path.join(ROOT, "include", "s2vt_hip.h")).read()
    assert "s2vt_decode_plan(" in header and "s2vt_decode_plan" in capi.SIGNATURES
    assert lib.s2vt_decode_plan is not None


def test_decode_plan_arguments_rejected_on_the_host(lib):
    """checked before the plan is worked out: no device query is reached, no GPU needed"""
    from s2vt_video_caption_amd import capi
    d = capi.Dims(64, 5, 70, 44, 28, 61)
    b, pe, sc = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int32(-7)
    refs = [ctypes.byref(x) for x in (b, pe, sc)]
    for enc in (0, 1):
        assert lib.s2vt_decode_plan(None, enc, *refs) == -1 and "s2vt_decode_plan" in _last_error(lib)
        for k in range(3):
            args = list(refs)
            args[k] = None
            assert lib.s2vt_decode_plan(d, enc, *args) == -1 and "s2vt_decode_plan" in _last_error(lib)
        for bad in (capi.Dims(0, 5, 70, 44, 28, 61), capi.Dims(64, 1, 70, 44, 28, 61), capi.Dims(64, 5, 70, 0, 28, 61)):
            assert lib.s2vt_decode_plan(bad, enc, *refs) == -1
    assert (b.value, pe.value, sc.value) == (-7, -7, -7)          # (a refused call writes nothing)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import s2vt_video_caption_amd  # noqa: F401
    from s2vt_video_caption_amd import capi
    try:
        the_lib = capi.load()
    except AttributeError:          # (a library from before s2vt_decode_plan: the layout functions are all this needs)
        del capi.SIGNATURES["s2vt_decode_plan"]
        the_lib = capi.load()
    with open(sys.argv[1], "w") as out:
        json.dump(layout_table(the_lib, capi), out, separators=(",", ":"))
        out.write("\n")
    print("recorded", sys.argv[1], "from", capi.LIB_PATH)
