"""GPU check of the search kernel's task loop around the full-task body (me_search_kernel<1, SPLIT, 2>, me_kernels.hpp): the prologue of
its own that a full task's lane-iterations run (the x halves of the MV costs, the lane field and the window address are the task's), and
the packed running minima that a wave of a whole-picture launch carries across the full tasks of one part (keys of me_carry_index,
flushed before a task of another kind or part and when the counter runs dry).  8-bit, FEN 1, search range 64, at lambda 57.9 and at the
largest lambda of me_pk2_gate, bit-exact against the oracle's exhaustive search for all 593 slots of every CTU:
  * 192 x 192 (nine CTUs) as whole jobs: the centre CTU has the full 129 x 129 window -- 17 full tasks dealt to four waves, the folded
    iteration and the 33rd quad in the twin;
  * 136 x 72 as whole jobs: a picture size that is no multiple of 64, every window clipped;
  * 128 x 128 as segments (SPLIT 2), which flush per task;
  * the per-CTU call (SPLIT 1) on the centre and on a corner CTU of the 192 x 192 picture;
each with zero predictors and with seeded random ones (windows of many sizes, wx % 4 != 0 and even wy among them), on seeded noise, on a
constant pair (every SAD ties: the MV cost and raster order decide across iterations, tasks and waves) and on stripes of period 16
columns and 2 rows (equal costs in different lane-iterations of one wave, and in every 16-candidate group of a row).  The whole-job
launches run in a child process (the planner's knob HMME_TAIL_PARTS is read once per process); the child also runs one case on a fresh
context and again on the used one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LQ = 3794534            # lambda 57.9
GATE2_LQ = 14680063     # the largest lambda_q16 of me_pk2_gate (tests/test_tree_pkmin2.py pins it)
SR = 64
PICTURES = {"nine_ctus": (192, 192), "ragged": (136, 72), "segments": (128, 128)}
WHOLE = ("nine_ctus", "ragged")
KINDS = ("noise", "constant", "stripes")
PREDS = ("zero", "random")
LAMBDAS = (LQ, GATE2_LQ)
FRESH = ("nine_ctus", "stripes", "random", LQ)      # the case the child runs first on its fresh context and again at its place


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


_CONTENT = {}


def content(pic, kind, pred):
    """-> (cur, ref) padded int16 planes, predictors int16[n_ctu, 2] or None"""
    from hmme import synth
    w, h = PICTURES[pic]
    if (pic, kind) not in _CONTENT:
        if kind == "constant":
            cur = ref = np.full((h, w), 77)
        elif kind == "stripes":
            y, x = np.mgrid[0:h, 0:w]
            cur = ref = 40 + 9 * (x % 16) + 60 * (y % 2)
        else:
            rng = np.random.default_rng(2024 + w + h)
            ref = rng.integers(0, 256, size=(h, w))
            cur = np.clip(np.roll(ref, (3, -5), axis=(0, 1)) + rng.integers(-5, 6, size=(h, w)), 0, 255)
        _CONTENT[(pic, kind)] = (synth.pad_plane(cur.astype(np.uint8)), synth.pad_plane(ref.astype(np.uint8)))
    p = synth.random_predictors(n_ctus(w, h), seed=w + h, max_pel=40) if pred == "random" else None
    return _CONTENT[(pic, kind)] + (p,)


def key(pic, kind, pred, lq):
    return "%s_%s_%s_%d" % (pic, kind, pred, lq)


_HELPER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_task_carry as T
from hmme import api, synth
m, out = synth.MARGIN, {}
def run(e, pic, kind, pred, lq):
    w, h = T.PICTURES[pic]
    cur, ref, p = T.content(pic, kind, pred)
    e.set_lambda_q16(lq)
    with e.plane(w, h) as pc, e.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        return e.search_frame(pc, pr, T.SR, p, fen=1)
with api.Engine(0, 128) as e:
    out["fresh_mv"], out["fresh_sad"] = run(e, *T.FRESH)
    for pic in T.WHOLE:
        for kind in T.KINDS:
            for pred in T.PREDS:
                for lq in T.LAMBDAS:
                    out["mv_" + T.key(pic, kind, pred, lq)], out["sad_" + T.key(pic, kind, pred, lq)] = run(e, pic, kind, pred, lq)
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def whole_tables(tmp_path_factory):
    """the whole-job searches of every case: one child process with HMME_TAIL_PARTS=1"""
    path = str(tmp_path_factory.mktemp("task_carry") / "whole.npz")
    r = subprocess.run([sys.executable, "-c", _HELPER, os.path.join(ROOT, "hm-opencl_amd"), os.path.join(ROOT, "tests"), path],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, HMME_TAIL_PARTS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


_ORACLE = {}


def oracle(oracle_lib, pic, kind, pred, lq):
    """the exhaustive search of one case, computed once"""
    from hmme import synth
    if (pic, kind, pred, lq) not in _ORACLE:
        w, h = PICTURES[pic]
        cur, ref, p = content(pic, kind, pred)
        _ORACLE[(pic, kind, pred, lq)] = oracle_lib.search_frame(cur, ref, (synth.MARGIN, synth.MARGIN), w, h, SR, p, lq, 1, 8, n_threads=8)
    return _ORACLE[(pic, kind, pred, lq)]


def lib():
    from hmme import api
    L = api.load()
    L.hmme_test_pk_body.argtypes = [C.c_uint32, C.c_int]
    L.hmme_test_pk_task_full.argtypes = [C.c_int] * 5
    L.hmme_test_tail_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    return L


def test_the_cases_are_what_they_claim():
    from refine_tables import oracle_windows
    L = lib()
    assert L.hmme_test_pk_body(LQ, 1) == 2 and L.hmme_test_pk_body(GATE2_LQ, 1) == 2 and L.hmme_test_pk_body(GATE2_LQ + 1, 1) == 1
    out = (C.c_int * 4)()
    assert L.hmme_test_tail_plan(128, 128, SR, 1, 512, out) == 0 and (out[0], out[1], out[3]) == (4, 0, 1) and out[2] > 4, "segments"
    assert tuple(oracle_windows(192, 192, SR)[4]) == (-64, -64, 64, 64), "the centre CTU's window is 129 x 129"
    # its 32-quad part: lane-iterations 0..63 full in the guided task sizes, the folded 65th and the 33rd quad are not
    assert all(L.hmme_test_pk_task_full(129, 129, 5, it, n) for it, n in ((0, 4), (56, 4), (60, 2), (62, 2)))
    assert not L.hmme_test_pk_task_full(129, 129, 5, 64, 1) and not L.hmme_test_pk_task_full(129, 129, 0, 0, 4)
    # the random predictors give windows of many sizes: a cut last quad, an even number of rows, full tasks beside the twin's
    sizes = []
    for pic in WHOLE:
        w, h = PICTURES[pic]
        win = oracle_windows(w, h, SR, content(pic, "noise", "random")[2])
        sizes += [(int(x1 - x0 + 1), int(y1 - y0 + 1)) for x0, y0, x1, y1 in win]
    assert any(wx % 4 and wx < 129 for wx, wy in sizes) and any(wy % 2 == 0 for wx, wy in sizes) and len(set(sizes)) >= 10, sizes
    assert all(any(L.hmme_test_pk_task_full(wx, wy, k, 0, 1) for k in (2, 3, 4, 5)) for wx, wy in sizes)
    # stripes: a candidate two rows down or sixteen columns right has the same SAD in every slot
    cur, ref, _ = content("nine_ctus", "stripes", "zero")
    assert np.array_equal(ref[82:182, 96:196], ref[80:180, 80:180])


def check(mv, sad, want, what):
    ox, oy, osad = want
    bad = np.argwhere((mv[..., 0] != ox) | (mv[..., 1] != oy) | (sad != osad))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


@pytest.mark.parametrize("lq", LAMBDAS)
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pic", WHOLE)
def test_whole_job_launch_equals_the_exhaustive_search(oracle_lib, whole_tables, pic, kind, pred, lq):
    t = whole_tables
    check(t["mv_" + key(pic, kind, pred, lq)], t["sad_" + key(pic, kind, pred, lq)], oracle(oracle_lib, pic, kind, pred, lq), "whole")
    if kind == "constant":
        assert (t["sad_" + key(pic, kind, pred, lq)] == 0).all()


def test_used_context_gives_what_a_fresh_one_gives(whole_tables):
    t = whole_tables
    assert np.array_equal(t["fresh_mv"], t["mv_" + key(*FRESH)]) and np.array_equal(t["fresh_sad"], t["sad_" + key(*FRESH)])


@pytest.mark.parametrize("lq", LAMBDAS)
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind", KINDS)
def test_segment_launch_equals_the_exhaustive_search(engine, oracle_lib, kind, pred, lq):
    from hmme import synth
    w, h = PICTURES["segments"]
    cur, ref, p = content("segments", kind, pred)
    m = synth.MARGIN
    engine.set_lambda_q16(lq)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, SR, p, fen=1)
    check(mv, sad, oracle(oracle_lib, "segments", kind, pred, lq), "segments")


@pytest.mark.parametrize("lq", LAMBDAS)
@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("kind", KINDS)
def test_per_ctu_call_equals_the_exhaustive_search(engine, oracle_lib, kind, pred, lq):
    """SPLIT 1 on the centre CTU (the full window) and the bottom-right one (clipped on two sides) of the 192 x 192 picture"""
    from hmme import api, synth
    from refine_tables import oracle_windows
    cur, ref, p = content("nine_ctus", kind, pred)
    ox, oy, osad = oracle(oracle_lib, "nine_ctus", kind, pred, lq)
    win = oracle_windows(192, 192, SR, p)
    m = synth.MARGIN
    engine.set_lambda_q16(lq)
    for ctu in (4, 8):
        lt_x, lt_y, rb_x, rb_y = (int(v) for v in win[ctu])
        px, py = (int(p[ctu, 0]), int(p[ctu, 1])) if p is not None else (0, 0)
        x, y = m + 64 * (ctu % 3), m + 64 * (ctu // 3)
        mv, sad = engine.search_ctu(cur, (x, y), ref, (x, y), api.SearchParams(lt_x, lt_y, rb_x, rb_y, px, py, 1, 8))
        check(mv, sad, (ox[ctu], oy[ctu], osad[ctu]), ("ctu", ctu))
