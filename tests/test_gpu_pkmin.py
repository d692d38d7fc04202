"""GPU check of the packed-minimum twin of the 8-bit search kernel (me_search_kernel<FEN, SPLIT, 1>: ME_PKMIN and me_pk_recover in
me_kernels.hpp, the tree of tools/gen_me_tree.py Tree(fen, pk=True)), bit-exact against the oracle in every launch form:
whole jobs (SPLIT 0) and segments (SPLIT 2) -- every picture both ways, chosen with the planner's knob HMME_TAIL_PARTS, which is read once
per process, hence one child process per mode, each running every case -- the per-CTU call and the window tiles of search range 128
(SPLIT 1).  The cases: windows clipped on every side and full 17-wide rows (4 + 1 quads), the full
129 x 129 window with its folded last row, pictures where every cost ties and where the winner sits at each place of its quad, lambda at
and just beyond the host's gate (the twin and the 32-bit kernel), a segment that crosses a job boundary, 2 x 2 tiles, and FEN off."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LQ = 3794534            # lambda 57.9
GATE_LQ = 29132523      # the largest lambda_q16 the gate admits (tests/test_tree_pkmin.py pins it)
MODES = {"default": {}, "whole": {"HMME_TAIL_PARTS": "1"}, "parts3": {"HMME_TAIL_PARTS": "3"}}
# name -> (width, height, search range, FEN, lambda_q16, content)
CASES = {
    "clipped":   (128, 128, 8, 1, LQ, "noise_out"),          # predictors that push every CTU's window over the picture's corner
    "rows17":    (128, 128, 8, 1, LQ, "noise"),              # 17 x 17 candidates: 4 + 1 quads per row, the last one with one valid candidate
    "fen0":      (128, 128, 8, 0, LQ, "noise_out"),
    "centre129": (192, 192, 64, 1, LQ, "noise"),             # the centre CTU has the full 129 x 129 window (32 + 1 quads, folded last row)
    "flat":      (128, 128, 8, 1, 0, "flat"),                # every cost ties
    "column1":   (128, 128, 8, 1, 0, "column1"),
    "column2":   (128, 128, 8, 1, 0, "column2"),
    "column3":   (128, 128, 8, 1, 0, "column3"),
    "gate_in":   (128, 128, 8, 1, GATE_LQ, "noise"),         # the twin at the largest MV costs it meets
    "gate_out":  (128, 128, 8, 1, GATE_LQ + 1, "noise"),     # the 32-bit kernel
    "crossing":  (384, 384, 64, 1, LQ, "noise"),             # 36 jobs x 17 units on 512 segments
    "tiles":     (128, 128, 128, 1, LQ, "noise"),            # 8-bit search range 128: 2 x 2 window tiles
}


def content(name):
    """-> (cur, ref) padded int16 planes, predictors int16[n_ctu, 2] or None"""
    from hmme import synth
    w, h, sr, fen, lq, kind = CASES[name]
    if kind == "flat":
        return synth.pad_plane(np.full((h, w), 77, np.uint8)), synth.pad_plane(np.full((h, w), 77, np.uint8)), None
    if kind.startswith("column"):
        # a flat pair but for ONE reference column: a block that covers it costs more, so a slot's winner is the first candidate of the
        # first row whose block does not.  Column 55 + j lies in the blocks of candidates 0 .. j - 1 of the slots at the left edge of the
        # second CTU column (block of candidate k: picture columns 56 + k ..): their winner is candidate j of the row's first quad
        j = int(kind[-1])
        ref = np.full((h, w), 77, np.uint8)
        ref[:, 55 + j] = 200
        return synth.pad_plane(np.full((h, w), 77, np.uint8)), synth.pad_plane(ref), None
    rng = np.random.default_rng(4711 + w + sr)
    ref = rng.integers(0, 256, size=(h, w))
    cur = np.clip(np.roll(ref, (3, -5), axis=(0, 1)) + rng.integers(-5, 6, size=(h, w)), 0, 255)
    pred = None
    if kind == "noise_out":      # quarter pels beyond TComDataCU::clipMv's limits, outwards at each of the four CTUs
        pred = np.array([[-70 * 4, -69 * 4], [69 * 4, -70 * 4], [-69 * 4, 70 * 4], [70 * 4, 69 * 4]], np.int16)
    return synth.pad_plane(cur), synth.pad_plane(ref), pred


_HELPER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_pkmin as T
from hmme import api, synth
m, out = synth.MARGIN, {}
with api.Engine(0, 128) as e:
    for name, (w, h, sr, fen, lq, kind) in T.CASES.items():
        cur, ref, pred = T.content(name)
        e.set_lambda_q16(lq)
        with e.plane(w, h) as pc, e.plane(w, h) as pr:
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            mv, sad = e.search_frame(pc, pr, sr, pred, fen=fen)
        out["mv_" + name], out["sad_" + name] = mv, sad
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def frame_tables(tmp_path_factory):
    """mode -> npz of the picture search of every case, one child process per mode"""
    d = tmp_path_factory.mktemp("pkmin")
    tables = {}
    for mode, env in MODES.items():
        path = str(d / (mode + ".npz"))
        r = subprocess.run([sys.executable, "-c", _HELPER, os.path.join(ROOT, "hm-opencl_amd"), os.path.join(ROOT, "tests"), path],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, (mode, r.stderr[-2000:])
        tables[mode] = np.load(path)
    return tables


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


_ORACLE = {}


def oracle(oracle_lib, name):
    """(ox, oy, osad) of a case, computed once"""
    if name not in _ORACLE:
        from hmme import synth
        w, h, sr, fen, lq, kind = CASES[name]
        cur, ref, pred = content(name)
        _ORACLE[name] = oracle_lib.search_frame(cur, ref, (synth.MARGIN, synth.MARGIN), w, h, sr, pred, lq, fen, 8, n_threads=8)
    return _ORACLE[name]


def gate(lq):
    from hmme import api
    L = api.load()
    L.hmme_test_pk_gate.argtypes = [C.c_uint32]
    return L.hmme_test_pk_gate(lq)


def tail_plan(w, h, sr):
    from hmme import api
    L = api.load()
    L.hmme_test_tail_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    out = (C.c_int * 4)()
    assert L.hmme_test_tail_plan(w, h, sr, 1, 512, out) == 0
    return tuple(out)


def test_the_cases_are_what_they_claim(oracle_lib):
    from refine_tables import oracle_windows
    assert all(gate(CASES[n][4]) == (0 if n == "gate_out" else 1) for n in CASES)
    win = oracle_windows(128, 128, 8, content("clipped")[2])
    assert all(win[c][2] - win[c][0] < 16 and win[c][3] - win[c][1] < 16 for c in range(4)), win       # cut on two sides each, all four sides met
    assert win[0][0] > -8 - 70 and win[1][2] < 70 + 8 and win[2][3] < 70 + 8 and win[0][1] > -8 - 69
    assert all(tuple(w) == (-8, -8, 8, 8) for w in oracle_windows(128, 128, 8)), "rows of 17 candidates"
    assert tuple(oracle_windows(192, 192, 64)[4]) == (-64, -64, 64, 64), "the centre CTU's window is 129 x 129"
    # the planner runs the four one-unit jobs of the 128 x 128 cases whole (as segments only in mode `parts3`) and the pictures of search range
    # 64 as segments (whole only in mode `whole`); `crossing`: 36 jobs of 17 units on 512 segments, segment s owns units
    # [612 s / 512, 612 (s + 1) / 512) (me_prep_segments_kernel) -- some segment holds the last unit of one job and the first of the next
    assert tail_plan(128, 128, 8) == (4, 4, 0, 0) and tail_plan(192, 192, 64) == (9, 0, 153, 1)
    assert tail_plan(384, 384, 64) == (36, 0, 512, 1)
    assert all(tuple(w) == (-64, -64, 64, 64) for w in oracle_windows(384, 384, 64)), "no window of `crossing` is clipped: 17 units each"
    assert any(612 * s // 512 < 17 * n < 612 * (s + 1) // 512 for s in range(512) for n in range(1, 36))
    wt = oracle_windows(128, 128, 128)
    assert all(w[2] - w[0] + 1 > 129 and w[3] - w[1] + 1 > 129 for w in wt), "2 x 2 tiles per CTU"
    # ties: the raster-first candidate everywhere; one reference column: the winner of the second CTU column's left-edge slots at j
    ox, oy, osad = oracle(oracle_lib, "flat")
    assert (ox == -8).all() and (oy == -8).all() and (osad == 0).all()
    for j in (1, 2, 3):
        ox, oy, osad = oracle(oracle_lib, "column%d" % j)
        for s in (0, 8, 128, 384):        # 8x4 top and bottom, 4x8 left, 8x8 of the CU at the CTU's top-left corner
            assert (ox[1, s], oy[1, s], osad[1, s]) == (-8 + j, -8, 0), (j, s)


@pytest.mark.parametrize("name", list(CASES))
def test_picture_search_equals_the_oracle_whole_and_as_segments(oracle_lib, frame_tables, name):
    ox, oy, osad = oracle(oracle_lib, name)
    for mode, t in frame_tables.items():
        mv, sad = t["mv_" + name], t["sad_" + name]
        assert mv.shape == ox.shape + (2,)
        bad = np.argwhere((mv[:, :, 0] != ox) | (mv[:, :, 1] != oy) | (sad != osad))
        assert len(bad) == 0, (mode, len(bad), bad[:8].tolist())


@pytest.mark.parametrize("name", ["clipped", "fen0", "column2", "gate_in", "gate_out", "tiles"])
def test_per_ctu_call_equals_the_oracle(engine, oracle_lib, name):
    """SPLIT 1: the per-CTU call on each CTU's own window (search range 128: its window tiles)"""
    from hmme import api, synth
    from refine_tables import oracle_windows
    w, h, sr, fen, lq, kind = CASES[name]
    cur, ref, pred = content(name)
    ox, oy, osad = oracle(oracle_lib, name)
    win = oracle_windows(w, h, sr, pred)
    m = synth.MARGIN
    engine.set_lambda_q16(lq)
    for ctu in range(4):
        lt_x, lt_y, rb_x, rb_y = (int(v) for v in win[ctu])
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        p = api.SearchParams(lt_x, lt_y, rb_x, rb_y, px, py, fen, 8)
        x, y = m + 64 * (ctu % 2), m + 64 * (ctu // 2)
        mv, sad = engine.search_ctu(cur, (x, y), ref, (x, y), p)
        assert np.array_equal(mv[:, 0], ox[ctu]) and np.array_equal(mv[:, 1], oy[ctu]) and np.array_equal(sad, osad[ctu]), ctu
