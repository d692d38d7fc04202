"""GPU check of the 8-bit reduction tree's key subtractions and packed 32x8 strips (tools/gen_me_tree.py, class Tree) in all three
instantiations of me_search_kernel that include the generated tree: the per-CTU call (SPLIT 1), the picture search as whole jobs
(SPLIT 0) and as segments (SPLIT 2) -- the last two selected with the planner's knobs exactly as
test_gpu_parity.py::test_tail_launch_modes_give_the_same_tables_as_whole_jobs_and_the_oracle selects them (they are read once per
process, hence one child process per mode, each running every case).  A 128x64 picture = two CTUs, search ranges 8 and 64, FEN on
and off; all 593 MVs and SADs of both CTUs bit-exact against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = 128, 64
CASES = [(name, sr, fen) for name in ("max", "equal", "corner") for sr in (8, 64) for fen in (0, 1)]
MODES = {"default": {}, "one": {"HMME_TAIL_LAUNCHES": "1"}, "two": {"HMME_TAIL_LAUNCHES": "2"}, "parts3": {"HMME_TAIL_PARTS": "3"},
         "whole": {"HMME_TAIL_PARTS": "1"}}
LAMBDA = {"max": 57.9, "equal": 0.0, "corner": 57.9}    # 0.0: nothing but the raster order separates the candidates of 'equal'


def content(name):
    """-> (cur, ref) padded int16 planes, predictors int16[2, 2] or None"""
    from hmme import synth
    if name == "max":       # every packed sum at its maximum (16x16 and, without FEN, 32x8: 65 280), every candidate a tie
        return synth.pad_plane(np.zeros((H, W), np.uint8)), synth.pad_plane(np.full((H, W), 255, np.uint8)), None
    if name == "equal":     # every SAD 0: each key subtraction sees two equal keys
        return synth.pad_plane(np.full((H, W), 77, np.uint8)), synth.pad_plane(np.full((H, W), 77, np.uint8)), None
    rng = np.random.default_rng(4711)
    ref = rng.integers(0, 256, size=(H, W))
    cur = np.clip(np.roll(ref, (3, -5), axis=(0, 1)) + rng.integers(-5, 6, size=(H, W)), 0, 255)
    # predictors (quarter pel) at the limits of TComDataCU::clipMv: CTU 0's window lies in the picture's top left corner, CTU 1's in
    # the bottom right one, cut by the limit on two sides at search range 8 as well as 64
    pred = np.array([[-70 * 4, -69 * 4], [69 * 4, 70 * 4]], np.int16)
    return synth.pad_plane(cur), synth.pad_plane(ref), pred


_HELPER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_tree_linearity as T
from hmme import api, synth
m, out = synth.MARGIN, {}
with api.Engine(0, 64) as e:
    for name, sr, fen in T.CASES:
        cur, ref, pred = T.content(name)
        e.set_lambda(T.LAMBDA[name])
        with e.plane(T.W, T.H) as pc, e.plane(T.W, T.H) as pr:
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            mv, sad = e.search_frame(pc, pr, sr, pred, fen=fen)
        out["mv_%s_%d_%d" % (name, sr, fen)], out["sad_%s_%d_%d" % (name, sr, fen)] = mv, sad
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def frame_tables(tmp_path_factory):
    """mode -> npz of the picture search of every case, one child process per mode"""
    d = tmp_path_factory.mktemp("tree_linearity")
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
    e = api.Engine(0, 64)
    yield e
    e.close()


@pytest.mark.parametrize("name,sr,fen", CASES)
def test_every_launch_form_equals_the_oracle(engine, oracle_lib, frame_tables, name, sr, fen):
    from hmme import api, synth
    from refine_tables import oracle_windows
    cur, ref, pred = content(name)
    m = synth.MARGIN
    lq = oracle_lib.oracle().hmo_lambda_q16(LAMBDA[name])
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), W, H, sr, pred, lq, fen, 8, n_threads=2)
    assert ox.shape == (2, 593)
    win = oracle_windows(W, H, sr, pred)
    if name == "corner":      # clipped on two sides, both search ranges
        assert all(win[c][2] - win[c][0] < 2 * sr and win[c][3] - win[c][1] < 2 * sr for c in range(2)), win
    else:
        assert all(tuple(win[c]) == (-sr, -sr, sr, sr) for c in range(2)), win
        # every candidate has the same SAD: lambda 0 leaves the first one in raster order, any other lambda the cheapest MV, (0, 0)
        assert (ox == (-sr if name == "equal" else 0)).all() and (oy == (-sr if name == "equal" else 0)).all()
    if name == "max" and not fen:
        assert osad[0, 544] == 65280 and osad[1, 512] == 65280      # a 16x16 and a 32x8: the packed sums at their maximum
    # SPLIT 1: the per-CTU call on each CTU's own window
    engine.set_lambda(LAMBDA[name])
    assert engine.lambda_q16 == lq
    for ctu in range(2):
        lt_x, lt_y, rb_x, rb_y = (int(v) for v in win[ctu])
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        p = api.SearchParams(lt_x, lt_y, rb_x, rb_y, px, py, fen, 8)
        mv, sad = engine.search_ctu(cur, (m + 64 * ctu, m), ref, (m + 64 * ctu, m), p)
        assert np.array_equal(mv[:, 0], ox[ctu]) and np.array_equal(mv[:, 1], oy[ctu]) and np.array_equal(sad, osad[ctu]), ("per-CTU call", ctu)
    # SPLIT 0 and 2: the picture search, every launch mode
    for mode, t in frame_tables.items():
        mv, sad = t["mv_%s_%d_%d" % (name, sr, fen)], t["sad_%s_%d_%d" % (name, sr, fen)]
        assert mv.shape == (2, 593, 2)
        assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy) and np.array_equal(sad, osad), mode
