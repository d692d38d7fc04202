"""Search, refinement and the three decisions on the device where the MV cost wraps or peaks (tests/lambda_cases.py): every cost is
distortion + getCost(bits), getCost is HM's (lambda_q16 * bits) >> 16 with the product wrapping in 32 bits, and the kernels' key fields
(me_kernels.hpp kInvCost, kInvCost16) and the host guards in front of them are sized for an MV cost of at most 65 535 -- which holds only
through that wrap.  Every comparison is bit-exact against the CPU oracle or the Python models; tests/test_oracle_vs_ref.py holds the oracle
to the reference's own code at the same lambdas.  The picture search's launch forms are selected as tests/test_gpu_tree_linearity.py selects
them (the planner's knobs are read once per process: one child process per mode), the refinement's as
tests/test_gpu_parity.py::test_refinement_launch_modes_give_the_same_tables does."""
import contextlib
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import lambda_cases as lc
import range_content as rc
import select_dirs_model as sdm
import select_model as sm
import select_refs_model as srm
from conftest import ROOT
from frame_helpers import (bind_hmo, ctu_origin, mkplane, oracle_prediction, oracle_search_w, origin_picture, random_field, run_bi_search)
from refine_tables import clamp, oracle_windows

pytestmark = pytest.mark.gpu

DEFAULT_LAMBDA = 57.9
ERR_ARG = -1
TAIL_MODES = {"default": {}, "one": {"HMME_TAIL_LAUNCHES": "1"}, "two": {"HMME_TAIL_LAUNCHES": "2"}, "parts3": {"HMME_TAIL_PARTS": "3"},
              "whole": {"HMME_TAIL_PARTS": "1"}}
FRAC_MODES = {"grid 4": {"HMME_FRAC_GRID": "4"}, "grid -1": {"HMME_FRAC_GRID": "-1"}, "job table": {"HMME_FRAC_JOB_TABLE": "1"}}
CHILD_TIMEOUT = 180


# ---- the 8-bit search cases (a: the top of the cost field, b: non-monotonic costs) ----------------------------------------------------
# (content, width, height, search range, FEN, lambda_q16); SR 96 is the tiled form beyond 129 x 129 candidates
SEARCH_CASES = [("max", 128, 64, sr, fen, lq) for lq in lc.PEAKS for sr in (8, 64) for fen in (0, 1)]
SEARCH_CASES += [("max", 128, 64, 96, 0, lc.ALL_ONES)]
SEARCH_CASES += [("corner", 128, 64, sr, fen, lq) for lq in lc.ROUNDING for sr in (8, 64) for fen in (0, 1)]
SEARCH_CASES += [("lownoise", 192, 128, sr, fen, lq) for lq in lc.ROUNDING for sr, fen in ((8, 0), (64, 1))]
SEARCH_CASES += [("corner", 128, 64, 96, fen, lq) for lq in lc.ROUNDING for fen in (0, 1)]        # clipped to one tile: the other three run empty
SEARCH_CASES += [("lownoise far", 192, 128, 96, fen, lq) for lq in lc.ROUNDING for fen in (0, 1)]  # winners in all four tiles
TILE_STEP = 129     # me_kernels.hpp kTileStep: a window beyond 129 x 129 candidates is searched as up to 2 x 2 tiles of that step


def key(name, sr, fen, lq):
    return "%s_%d_%d_%d" % (name.replace(" ", "_"), sr, fen, lq)


@functools.lru_cache(maxsize=None)
def search_content(name):
    """-> (cur, ref) padded int16 planes, predictors int16[n_ctu, 2] or None.  'max' and 'corner' are test_gpu_tree_linearity.py's;
    'lownoise' is a 192 x 128 random texture moved by (3, -2) under noise of one level: at the moved position a block's SAD is next to
    nothing, everywhere else it is large, so the large PUs follow the motion whatever its bits cost and the small ones follow the MV cost.
    'lownoise far' is the same pair under predictors about 40 pels out (MV differences of 34 bits and more at the motion), their signs chosen
    per CTU so that at search range 96 the motion lies in tile (1,0) of the windows of CTUs 1, 2 and 5, (0,1) of CTU 3's and (1,1) of
    CTU 4's -- the picture's limits clip the windows of the outer CTUs, the tiles count from each window's own top-left; CTU 0 keeps a
    predictor next to the motion (tile (0,0), few bits)"""
    from hmme import synth
    if not name.startswith("lownoise"):
        import test_gpu_tree_linearity as tl
        return tl.content(name)
    rng = np.random.default_rng(90210)
    ref = rng.integers(0, 256, size=(128, 192))
    cur = np.clip(np.roll(ref, (-2, 3), axis=(0, 1)) + rng.integers(-1, 2, size=(128, 192)), 0, 255)
    pred = synth.random_predictors(6, seed=17, max_pel=20)
    if name == "lownoise far":
        pred = np.array([pred[2], [-163, 157], [-159, -162], [166, -161], [-157, -165], [-162, 163]], np.int16)
    return synth.pad_plane(cur), synth.pad_plane(ref), pred


_SEARCH_HELPER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_lambda_edges as T
from hmme import api, synth
m, out = synth.MARGIN, {}
for sr_max in (64, 128):
    with api.Engine(0, sr_max) as e:
        for name, w, h, sr, fen, lq in T.SEARCH_CASES:
            if (sr > 64) != (sr_max == 128):
                continue
            cur, ref, pred = T.search_content(name)
            e.set_lambda_q16(lq)
            with e.plane(w, h) as pc, e.plane(w, h) as pr:
                pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
                mv, sad = e.search_frame(pc, pr, sr, pred, fen=fen)
            out["mv_" + T.key(name, sr, fen, lq)], out["sad_" + T.key(name, sr, fen, lq)] = mv, sad
np.savez(sys.argv[3], **out)
"""


def run_children(helper, modes, tmp_dir, *more):
    """mode -> npz written by one child process per mode, each under its own time limit"""
    tables = {}
    base = {k: v for k, v in os.environ.items() if k not in ("HMME_TAIL_LAUNCHES", "HMME_TAIL_PARTS", "HMME_FRAC_GRID", "HMME_FRAC_JOB_TABLE")}
    for mode, env in modes.items():
        path = str(tmp_dir / (mode.replace(" ", "_") + ".npz"))
        r = subprocess.run([sys.executable, "-c", helper, os.path.join(ROOT, "hm-opencl_amd"), os.path.join(ROOT, "tests"), path, *more],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=dict(base, **env))
        assert r.returncode == 0, (mode, r.stderr[-2000:])
        tables[mode] = np.load(path)
    return tables


@pytest.fixture(scope="module")
def search_tables(tmp_path_factory):
    return run_children(_SEARCH_HELPER, TAIL_MODES, tmp_path_factory.mktemp("lambda_edges_search"))


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(DEFAULT_LAMBDA)
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine128():
    from hmme import api
    e = api.Engine(0, 128)
    e.set_lambda(DEFAULT_LAMBDA)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


@pytest.fixture(scope="module")
def mv_cost(oracle_lib):
    L = oracle_lib.oracle()
    return lambda lq, x, y, px, py, scale: L.hmo_mv_cost(lq, x, y, px, py, scale)


@contextlib.contextmanager
def at(engine, lq):
    """the shared engine at lambda_q16 = lq, its own lambda put back afterwards"""
    was = engine.lambda_q16
    engine.set_lambda_q16(lq)
    assert engine.lambda_q16 == lq
    try:
        yield
    finally:
        engine.set_lambda_q16(was)


def assert_the_wrap_is_met(lq, mv, win, pred, every_window=True):
    """at lambda_q16 = 178956971: every window (the 9 x 9 windows of the bi-prediction search around their own centres: some window) holds
    candidates on both sides of the first wrap -- the one nearest the predictor does not wrap, one of the corners does -- and among the
    winners int16[n_ctu, 593, 2] (integer pels) some have a wrapped product.  (22 bits cost 60 074 and 24 bits 0, so where the distortions
    do not differ by more the winners gather at 24 bits: whether some stay below is the content's affair, asserted where it holds)"""
    if lq != lc.WRAP24:
        return
    below, beyond = [], []
    for c in range(mv.shape[0]):
        near = [min(max((int(pred[c][i]) + 2) >> 2, int(win[c][i])), int(win[c][2 + i])) for i in (0, 1)]
        below.append(not lc.wraps(lq, lc.mv_bits(4 * near[0], 4 * near[1], *pred[c])))
        beyond.append(any(lc.wraps(lq, lc.mv_bits(4 * int(win[c][i]), 4 * int(win[c][j]), *pred[c])) for i in (0, 2) for j in (1, 3)))
    assert (all if every_window else any)(below) and (all if every_window else any)(beyond), (below, beyond, win, pred)
    assert any(lc.wraps(lq, lc.mv_bits(4 * int(mv[c, s, 0]), 4 * int(mv[c, s, 1]), *pred[c])) for c in range(mv.shape[0]) for s in range(593))


def diff(a, b):
    return [tuple(int(v) for v in i) for i in np.argwhere(np.asarray(a) != np.asarray(b))[:4]]


@pytest.mark.parametrize("name,w,h,sr,fen,lq", SEARCH_CASES)
def test_8bit_search_every_launch_form(engine, engine128, oracle_lib, search_tables, name, w, h, sr, fen, lq):
    from hmme import api, synth
    cur, ref, pred = search_content(name)
    m = synth.MARGIN
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, fen, 8, n_threads=8)
    win = oracle_windows(w, h, sr, pred)
    bits = np.array([[lc.mv_bits(4 * int(ox[c, s]), 4 * int(oy[c, s]), *((pred[c] if pred is not None else (0, 0)))) for s in range(593)] for c in range(n_ctu)])
    if name == "max":
        if sr <= 64:
            assert all(tuple(win[c]) == (-sr, -sr, sr, sr) for c in range(2)), win
        assert (osad[:, 592] == 1044480).all()                       # 4096 * 255: the largest 8-bit sum
        if lq == lc.ALL_ONES:   # every candidate ties at SAD + 65535: the first in raster order wins, and the 64x64 key carried 1 044 480 + 65 535
            assert (ox == win[:, None, 0]).all() and (oy == win[:, None, 1]).all()
            assert all(lc.get_cost(lq, int(b)) == lc.MAX_MV_COST for b in np.unique(bits))
        else:                   # 0x80000000: the first candidate with an even bit count, cost 0
            assert all(lc.get_cost(lq, int(b)) == 0 for b in np.unique(bits))
    elif lq == lc.WRAP24:
        # 'corner', whose windows up to search range 64 do not reach the motion, has every winner at 24 bits or beyond; in 'lownoise' the
        # PUs of a CTU whose predictor is near the motion stay below: winners on both sides of the wrap
        assert_the_wrap_is_met(lq, np.stack([ox, oy], axis=-1), win, pred)
        assert (bits < 24).any() or name == "corner", (bits.min(), bits.max())
    elif lq != lc.TINY:         # one per bit, rounded down or up: winners of several MV costs
        assert len({lc.get_cost(lq, int(b)) for b in np.unique(bits)}) >= 3, np.unique(bits)
    if name == "corner":
        assert all(win[c][2] - win[c][0] < 2 * sr and win[c][3] - win[c][1] < 2 * sr for c in range(2)), win
    if sr > 64 and name != "max":
        tiles = {(int(ox[c, s] - win[c][0]) // TILE_STEP, int(oy[c, s] - win[c][1]) // TILE_STEP) for c in range(n_ctu) for s in range(593)}
        if name == "corner":    # the clipped windows fit one tile
            assert tiles == {(0, 0)} and all(win[c][2] - win[c][0] < TILE_STEP and win[c][3] - win[c][1] < TILE_STEP for c in range(2)), (tiles, win)
        else:                   # winners decoded against the top-left from each of the four tiles, merged where their MV costs differ
            assert tiles == {(0, 0), (1, 0), (0, 1), (1, 1)}, tiles
            assert {(int(ox[c, 592] - win[c][0]) // TILE_STEP, int(oy[c, 592] - win[c][1]) // TILE_STEP) for c in range(n_ctu)} == tiles
    # the per-CTU call on each CTU's own window (beyond SR 64: its tiled form)
    e = engine128 if sr > 64 else engine
    with at(e, lq):
        for ctu in range(n_ctu):
            cx, cy = ctu_origin(ctu, w)
            if cx + 64 > w or cy + 64 > h:
                continue
            px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
            p = api.SearchParams(*(int(v) for v in win[ctu]), px, py, fen, 8)
            mv, sad = e.search_ctu(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p)
            assert np.array_equal(mv[:, 0], ox[ctu]) and np.array_equal(mv[:, 1], oy[ctu]), ("per-CTU call", ctu, diff(mv[:, 0], ox[ctu]), diff(mv[:, 1], oy[ctu]))
            assert np.array_equal(sad, osad[ctu]), ("per-CTU call", ctu, diff(sad, osad[ctu]))
    # the picture search: whole jobs, segmented tails, tiles
    for mode, t in search_tables.items():
        mv, sad = t["mv_" + key(name, sr, fen, lq)], t["sad_" + key(name, sr, fen, lq)]
        assert mv.shape == (n_ctu, 593, 2)
        assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy), (mode, diff(mv[:, :, 0], ox), diff(mv[:, :, 1], oy))
        assert np.array_equal(sad, osad), (mode, diff(sad, osad))


# ---- c: the 16-bit search at the accepted inputs nearest each refusal ----------------------------------------------------------------
# range_content.py's 136 x 72 pictures (3 x 2 CTUs; CTUs 3 and 5 saturated: flat 0 / maxv against the farthest value)
RW, RH, R_SR, R_SR_BI, R_CTUS = 136, 72, 8, 4, 6
IDENTITY = (64, 0, 6, 32)


@functools.lru_cache(maxsize=None)
def range_pair(bd, wp):
    cur, ref, _ = rc.extreme_pair(RW, RH, bd, wp, seed=1000 + bd)
    cur.setflags(write=False); ref.setflags(write=False)
    return cur, ref


def range_predictors(bd):
    from hmme import synth
    return synth.random_predictors(R_CTUS, seed=50 + bd, max_pel=4)


@pytest.mark.parametrize("lq", [lc.ALL_ONES, lc.WRAP24])
@pytest.mark.parametrize("bd", [10, 12])
def test_16bit_plain_search(engine, oracle_lib, bd, lq):
    """me_search16_kernel / me_finalize16_kernel (picture) and me_finalize1_kernel (per-CTU call): the saturated CTUs' 64x64 slot holds the
    largest sum of the bit depth, 4096 * maxv >> (bd - 8), under an MV cost of 65 535"""
    from hmme import api, synth
    m = synth.MARGIN
    cur, ref = range_pair(bd, IDENTITY)
    pred = range_predictors(bd)
    win = oracle_windows(RW, RH, R_SR, pred)
    pc, pr = mkplane(engine, cur, RW, RH, bd), mkplane(engine, ref, RW, RH, bd)
    try:
        with at(engine, lq):
            for fen in (0, 1):
                ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), RW, RH, R_SR, pred, lq, fen, bd, n_threads=6)
                assert int(osad.max()) == (4096 * ((1 << bd) - 1)) >> (bd - 8) == int(osad[3, 592]) == int(osad[5, 592])
                assert_the_wrap_is_met(lq, np.stack([ox, oy], axis=-1), win, pred)
                mv, sad = engine.search_frame(pc, pr, R_SR, pred, fen=fen)
                assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy), (fen, diff(mv[:, :, 0], ox), diff(mv[:, :, 1], oy))
                assert np.array_equal(sad, osad), (fen, diff(sad, osad))
                cx, cy = ctu_origin(3, RW)     # a whole CTU in the padded plane: the bottom row's first, saturated
                p = api.SearchParams(*(int(v) for v in win[3]), int(pred[3, 0]), int(pred[3, 1]), fen, bd)
                cmv, csad = engine.search_ctu(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p)
                assert np.array_equal(cmv[:, 0], ox[3]) and np.array_equal(cmv[:, 1], oy[3]) and np.array_equal(csad, osad[3]), ("per-CTU call", fen)
    finally:
        pc.close(); pr.close()


@pytest.mark.parametrize("lq", [lc.ALL_ONES, lc.WRAP24])
@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("bd", [8, 10])
def test_weighted_search_at_the_boundary_weights(engine, oracle_lib, bd, family, lq):
    """the accepted weight nearest the refusal of each family: the `+ 65535` of the host guards is what this MV cost needs"""
    from hmme import api, synth
    m = synth.MARGIN
    wp = rc.boundary_weight(bd, 0, family)
    cur, ref = range_pair(bd, wp)
    pred = range_predictors(bd)
    omv, osad = oracle_search_w(oracle_lib, cur, ref, RW, RH, R_SR, pred, lq, bd, wp, range(R_CTUS))
    assert int(osad.max()) == (4096 * rc.span_of(bd, wp)) >> (bd - 8)
    win = oracle_windows(RW, RH, R_SR, pred)
    assert_the_wrap_is_met(lq, omv, win, pred)
    if lq == lc.ALL_ONES:
        assert int(osad.max()) + lc.MAX_MV_COST < rc.INV_COST16
    pc, pr = mkplane(engine, cur, RW, RH, bd), mkplane(engine, ref, RW, RH, bd)
    try:
        with at(engine, lq):
            mv, sad = engine.search_frame_w(pc, pr, R_SR, wp, pred, fen=1)
            assert np.array_equal(mv, omv), (wp, diff(mv, omv))
            assert np.array_equal(sad, osad), (wp, diff(sad, osad))
            cx, cy = ctu_origin(3, RW)
            p = api.SearchParams(*(int(v) for v in win[3]), int(pred[3, 0]), int(pred[3, 1]), 1, bd)
            cmv, csad = engine.search_ctu_w(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p, wp)
            assert np.array_equal(cmv, omv[3]) and np.array_equal(csad, osad[3]), ("per-CTU call", wp)
    finally:
        pc.close(); pr.close()


@functools.lru_cache(maxsize=None)
def range_triple(bd):
    t = rc.extreme_triple(RW, RH, bd, seed=2000 + bd)
    for a in t:
        a.setflags(write=False)
    return t


@pytest.mark.parametrize("lq", [lc.ALL_ONES, lc.WRAP24])
@pytest.mark.parametrize("fen", [0, 1])
@pytest.mark.parametrize("bd", [8, 10])
def test_bi_search_on_extreme_origins(engine, oracle_lib, hmo, bd, fen, lq):
    maxv = (1 << bd) - 1
    with at(engine, lq):
        r = run_bi_search(engine, oracle_lib, hmo, RW, RH, bd, R_SR_BI, fen, 64 if fen else 1, seed=2100 + bd, planes3=range_triple(bd))
    assert r["org"].min() == -maxv and r["org"].max() == 2 * maxv
    assert_the_wrap_is_met(lq, r["mv"], oracle_windows(RW, RH, R_SR_BI, r["pred"], r["center"]), r["pred"], every_window=False)


@pytest.mark.parametrize("lq", [lc.ALL_ONES, lc.WRAP24])
@pytest.mark.parametrize("bd", [8, 10])
def test_bi_search_and_refinement_over_several_references(engine, hmo, bd, lq):
    """hmme_search / refine_frame_bi_refs, two references against two planes named block by block, window centres that differ from the
    predictors: every CTU and slot against the per-CTU calls on the origin at the same lambda"""
    from test_gpu_bipred_refs import SR_BI, check_against_the_per_ctu_calls, checkerboard, pictures, predictors, unrelated
    w, h, n = RW, RH, R_CTUS
    pics = pictures(w, h, bd, 2400 + bd, 3) + unrelated(w, h, bd, 2450 + bd, 2)
    field, ref_field = random_field(n, 64, 2410 + bd), checkerboard(n, 64, 2, w)
    seed = 2420 + bd
    pred, center = predictors(2, n, seed), predictors(2, n, seed + 50)          # what check_against_the_per_ctu_calls draws
    assert all(np.any(center[r] != pred[r], axis=1).all() for r in range(2))
    with at(engine, lq):
        for had in (True, False):
            mv, sad, qmv, cost = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, [1, 2], [3, 4], field, ref_field, seed, fen=int(bd == 8), had=had)
    for r in range(2):
        assert_the_wrap_is_met(lq, mv[r], oracle_windows(w, h, SR_BI, pred[r], center[r]), pred[r], every_window=False)


# ---- d: the refinement ----------------------------------------------------------------------------------------------------------------
FW, FH, F_CTUS, F_SR = 192, 128, 6, 32
REFINE_CASES = [(bd, had, lq) for bd in (8, 10) for had in (0, 1) for lq in lc.WRAPPING]
F_WP = (70, -9, 6, 32)


@functools.lru_cache(maxsize=None)
def refine_inputs(bd):
    """-> cur, ref, other (padded planes), integer MVs int16[6, 593, 2] (the oracle's search at the zero predictor, SR 8, an everyday lambda:
    a caller-chosen table), predictors int16[6, 2] placed 16 pels and 3 pels from each CTU's 64x64 winner: 4 * mv - pred = (+-64, +-12), so
    that the nine half-pel points around it have 13 or 15 bits in x and 9 in y -- 22 and 24, either side of the first wrap of
    lambda_q16 = 178956971.  The window of SR 32 around such a predictor holds every integer MV"""
    import oracle_py
    from hmme import synth
    m = synth.MARGIN
    cur, ref, _ = synth.make_pair(FW, FH, seed=300 + bd, bit_depth=bd, max_mv=5, region=64, noise_sigma=3.0)
    _, other, _ = synth.make_pair(FW, FH, seed=1300 + bd, bit_depth=bd, max_mv=5, region=64, noise_sigma=3.0)
    ox, oy, _ = oracle_py.search_frame(cur, ref, (m, m), FW, FH, 8, None, oracle_py.oracle().hmo_lambda_q16(DEFAULT_LAMBDA), 1, bd, n_threads=6)
    imv = np.stack([ox, oy], axis=-1).astype(np.int16)
    pred = np.zeros((F_CTUS, 2), np.int16)
    for k in range(F_CTUS):
        sx, sy = (1 if k % 2 == 0 else -1), (1 if k % 4 < 2 else -1)
        d = (64 * sx, 12 * sy) if k % 3 != 2 else (12 * sx, 64 * sy)
        pred[k] = (4 * int(imv[k, 592, 0]) - d[0], 4 * int(imv[k, 592, 1]) - d[1])
    win = oracle_windows(FW, FH, F_SR, pred)
    assert np.array_equal(clamp(imv, win), imv)
    for a in (cur, ref, other, imv, pred):
        a.setflags(write=False)
    return cur, ref, other, imv, pred


def nine_point_bits(mv, pred):
    """bit counts of the nine half-pel points around the integer MV"""
    return [lc.mv_bits(4 * int(mv[0]) + ox, 4 * int(mv[1]) + oy, int(pred[0]), int(pred[1])) for oy in (-2, 0, 2) for ox in (-2, 0, 2)]


def test_the_refinement_inputs_straddle_the_wrap():
    """the condition of the refinement cases, on the inputs alone"""
    for bd in (8, 10):
        _, _, _, imv, pred = refine_inputs(bd)
        for k in range(F_CTUS):
            b = nine_point_bits(imv[k, 592], pred[k])
            assert min(b) < 24 <= max(b), (bd, k, b)
            assert not lc.wraps(lc.WRAP24, min(b)) and lc.wraps(lc.WRAP24, max(b))


_REFINE_HELPER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_lambda_edges as T
from frame_helpers import mkplane
from hmme import api
out, inputs = {}, np.load(sys.argv[4])
with api.Engine(0, 64) as e:
    for bd, had, lq in T.REFINE_CASES:
        cur, ref, other, imv, pred = (inputs["%s_%d" % (k, bd)] for k in ("cur", "ref", "other", "imv", "pred"))
        e.set_lambda_q16(lq)
        pc, pr, po = (mkplane(e, a, T.FW, T.FH, bd) for a in (cur, ref, other))
        tabs = {"plain": e.refine_frame(pc, pr, T.F_SR, imv, pred, use_hadamard=bool(had)),
                "w": e.refine_frame_w(pc, pr, T.F_SR, T.F_WP, imv, pred, use_hadamard=bool(had)),
                "bi": e.refine_frame_bi(pc, pr, po, T.F_SR, T.bi_field(bd), imv, pred_q=pred, use_hadamard=bool(had))}
        pc.close(); pr.close(); po.close()
        for form, (q, c) in tabs.items():
            out["q_" + T.refine_key(form, bd, had, lq)], out["c_" + T.refine_key(form, bd, had, lq)] = q, c
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def refine_mode_tables(tmp_path_factory):
    """the children refine the parent's inputs, handed over in a file"""
    d = tmp_path_factory.mktemp("lambda_edges_refine")
    inputs = {}
    for bd in (8, 10):
        cur, ref, other, imv, pred = refine_inputs(bd)
        inputs.update({"cur_%d" % bd: cur, "ref_%d" % bd: ref, "other_%d" % bd: other, "imv_%d" % bd: imv, "pred_%d" % bd: pred})
    np.savez(str(d / "inputs.npz"), **inputs)
    return run_children(_REFINE_HELPER, FRAC_MODES, d, str(d / "inputs.npz"))


def refine_key(form, bd, had, lq):
    return "%s_%d_%d_%d" % (form, bd, had, lq)


def bi_field(bd):
    """the other direction's motion field, one MV per 8x8 block"""
    return random_field(F_CTUS, 64, seed=77 + bd)


def assert_every_launch_mode(tables, form, bd, had, lq, q, c):
    """the job-walking launches (4 workgroups; as many as the chip holds) and the job table give the tables q, c of the default launch"""
    assert set(tables) == set(FRAC_MODES)
    for mode, t in tables.items():
        tq, tc = t["q_" + refine_key(form, bd, had, lq)], t["c_" + refine_key(form, bd, had, lq)]
        assert np.array_equal(tq, q) and np.array_equal(tc, c), (form, mode, diff(tq, q), diff(tc, c))


@pytest.mark.parametrize("bd,had,lq", REFINE_CASES)
def test_refinement_plain(engine, oracle_lib, refine_mode_tables, bd, had, lq):
    """one workgroup per job (the default launch), the two job-walking launches and the job table, and the per-CTU call"""
    from hmme import api, synth
    m = synth.MARGIN
    cur, ref, _, imv, pred = refine_inputs(bd)
    oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), FW, FH, imv, pred, lq, had, bd, n_threads=6)
    pc, pr = mkplane(engine, cur, FW, FH, bd), mkplane(engine, ref, FW, FH, bd)
    try:
        with at(engine, lq):
            q, c = engine.refine_frame(pc, pr, F_SR, imv, pred, use_hadamard=bool(had))
            assert np.array_equal(q, oq), diff(q, oq)
            assert np.array_equal(c, oc), diff(c, oc)
            win = oracle_windows(FW, FH, F_SR, pred)
            for ctu in (0, 5):
                cx, cy = ctu_origin(ctu, FW)
                p = api.SearchParams(*(int(v) for v in win[ctu]), int(pred[ctu, 0]), int(pred[ctu, 1]), 1, bd)
                cq, cc = engine.refine_ctu(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p, imv[ctu], use_hadamard=bool(had))
                assert np.array_equal(cq, oq[ctu]) and np.array_equal(cc, oc[ctu]), ("refine_ctu", ctu, diff(cq, oq[ctu]), diff(cc, oc[ctu]))
    finally:
        pc.close(); pr.close()
    assert_every_launch_mode(refine_mode_tables, "plain", bd, had, lq, oq, oc)


@pytest.mark.parametrize("bd,had,lq", REFINE_CASES)
def test_refinement_weighted(engine, oracle_lib, refine_mode_tables, bd, had, lq):
    """the default launch against the oracle slot by slot in two CTUs; every other launch mode gives the default launch's tables"""
    from hmme import api, synth
    m = synth.MARGIN
    cur, ref, _, imv, pred = refine_inputs(bd)
    assert api.weight_check(bd, F_WP, True) == 0
    table = oracle_lib.slot_table()
    pc, pr = mkplane(engine, cur, FW, FH, bd), mkplane(engine, ref, FW, FH, bd)
    try:
        with at(engine, lq):
            q, c = engine.refine_frame_w(pc, pr, F_SR, F_WP, imv, pred, use_hadamard=bool(had))
    finally:
        pc.close(); pr.close()
    for ctu in (1, 4):
        cx, cy = ctu_origin(ctu, FW)
        pq = (int(pred[ctu, 0]), int(pred[ctu, 1]))
        for s in range(593):
            x, y, bw, bh = (int(v) for v in table[s])
            mv = (int(imv[ctu, s, 0]), int(imv[ctu, s, 1]))
            hx, hy, qx, qy, oc = oracle_lib.frac_refine_w(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, mv, pq, lq, had, bd, F_WP)
            assert (int(q[ctu, s, 0]), int(q[ctu, s, 1]), int(c[ctu, s])) == (4 * mv[0] + 2 * hx + qx, 4 * mv[1] + 2 * hy + qy, oc), (ctu, s)
    assert_every_launch_mode(refine_mode_tables, "w", bd, had, lq, q, c)


@pytest.mark.parametrize("bd,had,lq", REFINE_CASES)
def test_refinement_bi(engine, oracle_lib, hmo, refine_mode_tables, bd, had, lq):
    from hmme import synth
    m = synth.MARGIN
    cur, ref, other, imv, pred = refine_inputs(bd)
    field = bi_field(bd)
    org = origin_picture(cur, oracle_prediction(hmo, other, FW, FH, bd, field), FW, FH)
    oq, oc = oracle_lib.refine_frame(np.ascontiguousarray(np.pad(org, m)), ref, (m, m), FW, FH, imv, pred, lq, had, bd, n_threads=6)
    pc, pr, po = (mkplane(engine, a, FW, FH, bd) for a in (cur, ref, other))
    try:
        with at(engine, lq):
            q, c = engine.refine_frame_bi(pc, pr, po, F_SR, field, imv, pred_q=pred, use_hadamard=bool(had))
    finally:
        pc.close(); pr.close(); po.close()
    assert np.array_equal(q, oq), diff(q, oq)
    assert np.array_equal(c, oc), diff(c, oc)
    assert_every_launch_mode(refine_mode_tables, "bi", bd, had, lq, oq, oc)


# ---- e: the decisions -----------------------------------------------------------------------------------------------------------------
def far_predictors(shape, seed):
    """quarter-pel predictors out to +-2000, half of them within +-40: MV bit counts from a few to about 50"""
    rng = np.random.default_rng(seed)
    far = rng.integers(-2000, 2001, size=shape + (2,))
    near = rng.integers(-40, 41, size=shape + (2,))
    return np.where(rng.integers(0, 2, size=shape + (1,)) == 1, far, near).astype(np.int16)


@functools.lru_cache(maxsize=None)
def decision_tables(w, h):
    """8-bit tables of the oracle for a w x h picture: a search's (integer MVs, SADs) and a refinement's (quarter-pel MVs, costs)"""
    import oracle_py
    from hmme import synth
    m = synth.MARGIN
    cur, ref, _ = synth.make_pair(w, h, seed=500 + w, max_mv=5, region=32, noise_sigma=3.0)
    lq = oracle_py.oracle().hmo_lambda_q16(DEFAULT_LAMBDA)
    ox, oy, osad = oracle_py.search_frame(cur, ref, (m, m), w, h, 8, None, lq, 1, 8, n_threads=6)
    imv = np.stack([ox, oy], axis=-1).astype(np.int16)
    qmv, cost = oracle_py.refine_frame(cur, ref, (m, m), w, h, imv, None, lq, 1, 8, n_threads=6)
    return imv, osad, qmv, cost


@pytest.mark.parametrize("lq", lc.WRAPPING)
@pytest.mark.parametrize("unit", [1, 0])
@pytest.mark.parametrize("w,h", [(192, 128), (64, 64)])
def test_select_frame_prices_the_mv_with_the_wrap(engine, mv_cost, w, h, unit, lq):
    """price_mv at both mv_units: the integer tables of a search (unit 1), the quarter-pel tables of a refinement (unit 0)"""
    from hmme import api
    imv, sad, qmv, cost = decision_tables(w, h)
    mv, c = (imv, sad) if unit else (qmv, cost)
    n = mv.shape[0]
    pred = far_predictors((n,), seed=600 + w + unit)
    if n == 1:
        pred[0] = (-1012, 0)      # 4 * mv - pred.x crosses 1024, where a component goes from 21 to 23 bits: totals on both sides of 24
    sel = api.SelectParams(64, mv_unit=unit, price_mv=1, cu_cost=40, pu_cost=12)
    bits = [lc.mv_bits(int(mv[k, s, 0]) << (2 * unit), int(mv[k, s, 1]) << (2 * unit), *pred[k]) for k in range(n) for s in range(593)]
    assert any(lc.wraps(lq, b) for b in bits) and (lq != lc.WRAP24 or any(not lc.wraps(lq, b) for b in bits))
    mf, ms, mc, _ = sm.select_picture(mv, c, sel, w, h, 0, pred, lq, mv_cost)
    with at(engine, lq):
        f, s, cc = engine.select_frame(w, h, sel, mv, c, pred)
    assert np.array_equal(f, mf) and np.array_equal(s, ms) and np.array_equal(cc, mc), (diff(f, mf), diff(s, ms), diff(cc, mc))
    # the wrap decides: priced with the 64-bit product the model chooses differently
    wide = lambda q, x, y, px, py, scale: lc.get_cost_64(q, lc.mv_bits(x << scale, y << scale, px, py))
    _, _, wc, _ = sm.select_picture(mv, c, sel, w, h, 0, pred, lq, wide)
    assert not np.array_equal(wc, mc)


@pytest.mark.parametrize("lq", lc.WRAPPING)
@pytest.mark.parametrize("unit", [1, 0])
@pytest.mark.parametrize("w,h", [(192, 128), (64, 64)])
def test_select_refs_frame_prices_the_mv_with_the_wrap(engine, mv_cost, w, h, unit, lq):
    from hmme import api
    n = srm.n_ctus(w, h)
    mv, cost = srm.random_ref_tables(3, n, seed=700 + w, noise=64)
    pred = far_predictors((3, n), seed=710 + w + unit)
    assert len({tuple(pred[r, 0]) for r in range(3)}) == 3
    sel = api.SelectParams(64, mv_unit=unit, price_mv=1, cu_cost=40, pu_cost=12, min_depth=2 if n == 1 else 0)
    ref_cost = srm.hm_ref_cost(3)
    mf, mr, ms, mc, _ = srm.select_refs_picture(mv, cost, sel, w, h, ref_cost, 0, pred, lq, mv_cost)
    assert len(set(mr[ms != sm.NO_SLOT].tolist())) >= (2 if n > 1 else 1)
    # among the MVs of the chosen (reference, slot) pairs some are priced with a wrapped product (at 178956971 some of the priced are not:
    # 22 bits cost 60 074 there and 24 bits 0, so the chosen gather at 24 bits and beyond)
    chosen = [lc.mv_bits(int(mv[rr, k, ss, 0]) << (2 * unit), int(mv[rr, k, ss, 1]) << (2 * unit), *pred[rr, k])
              for k in range(n) for rr, ss in zip(mr[k].tolist(), ms[k].tolist()) if ss != sm.NO_SLOT]
    priced = [lc.mv_bits(int(mv[rr, k, ss, 0]) << (2 * unit), int(mv[rr, k, ss, 1]) << (2 * unit), *pred[rr, k]) for rr in range(3) for k in range(n) for ss in range(593)]
    assert any(lc.wraps(lq, b) for b in chosen) and (lq != lc.WRAP24 or any(not lc.wraps(lq, b) for b in priced)), (sorted(set(chosen)), min(priced))
    with at(engine, lq):
        f, r, s, cc = engine.select_refs_frame(w, h, sel, mv, cost, ref_cost, pred)
    assert np.array_equal(f, mf) and np.array_equal(r, mr) and np.array_equal(s, ms) and np.array_equal(cc, mc), (diff(r, mr), diff(s, ms), diff(cc, mc))
    # the wrap decides: priced with the 64-bit product the model chooses other references or reports other costs
    wide = lambda q, x, y, px, py, scale: lc.get_cost_64(q, lc.mv_bits(x << scale, y << scale, px, py))
    _, wr, _, wc, _ = srm.select_refs_picture(mv, cost, sel, w, h, ref_cost, 0, pred, lq, wide)
    assert not np.array_equal(wc, mc) and (n == 1 or not np.array_equal(wr, mr))


DIR_BITS = (sdm.HM_BITS, ((1000, 7, 4096), (4096, 33)))


def dir_tables(n, seed, pred):
    """select_dirs_model.random_dir_tables written at lambda_q16 = 1 (costs = distortions alone), a seeded half of the slots' distortions raised by
    60 000: below and above both 32 768 and 65 535, so that at every lambda of the set the floor of rule 1 is hit in some slots and not in others"""
    low = sdm.random_dir_tables(n, n, seed, pred=pred, lambda_q16=lc.TINY)
    high = sdm.random_dir_tables(n, n, seed, pred=pred, lambda_q16=lc.TINY, base=60000)
    assert all(np.array_equal(low[k], high[k]) for k in (0, 2, 4))
    odd = np.random.default_rng(seed + 1).integers(0, 2, size=593) == 1
    return low[0], np.where(odd, high[1], low[1]), low[2], np.where(odd, high[3], low[3]), low[4]


@pytest.mark.parametrize("lq", lc.WRAPPING)
@pytest.mark.parametrize("bits", DIR_BITS)
@pytest.mark.parametrize("w,h", [(192, 128), (64, 64)])
def test_select_dirs_frame_wraps_both_costs_and_hits_the_floor(engine, w, h, bits, lq):
    """tables whose costs are distortions alone (dir_tables): taking gc(mv bits) out again hits the floor of rule 1 wherever
    the MV cost exceeds the distortion; the bits put back wrap as well"""
    from hmme import api
    n = sdm.n_ctus(w, h)
    pred = far_predictors((2, n), seed=800 + w)
    tabs = dir_tables(n, 810 + w, pred)
    mv_uni, cost_uni = tabs[0], tabs[1]
    floor = clear = wrap_out = wrap_back = 0
    for l in range(2):
        for k in range(n):
            for s in range(0, 593, 3):
                bu = sdm.mvb(mv_uni[l, k, s], pred[l][k])
                g = sdm.gc(lq, bu)
                floor += int(cost_uni[l, k, s]) < g
                clear += int(cost_uni[l, k, s]) > g > 0 or g == 0
                wrap_out += lc.wraps(lq, bu)
                wrap_back += lc.wraps(lq, bits[0][l] + bits[1][l] + bu)
    # an MV's bit count is the sum of two odd exp-Golomb lengths: even, so at 0x80000000 gc(mv bits) is 0 and only the bits put back cost
    assert (floor or lq == lc.HALF) and clear and wrap_out and wrap_back, (floor, clear, wrap_out, wrap_back)
    sel = api.SelectParams(64, min_depth=2 if n == 1 else 0, cu_cost=40, pu_cost=12)
    mf, md, ms, mc = sdm.select_dirs_picture(*tabs, sel, w, h, bits, 0, pred, lq)
    assert len(set(md[ms != sm.NO_SLOT].tolist())) >= 2
    with at(engine, lq):
        f, d, s, cc = engine.select_dirs_frame(w, h, sel, api.DirParams(*bits), *tabs, pred)
    assert np.array_equal(f, mf) and np.array_equal(d, md) and np.array_equal(s, ms) and np.array_equal(cc, mc), (diff(d, md), diff(s, ms), diff(cc, mc))


@pytest.mark.parametrize("lq", [lc.HALF, lc.WRAP24])
@pytest.mark.parametrize("R", [2, 4])
def test_select_dirs_refs_frame_at_odd_and_even_bit_totals(engine, R, lq):
    """hmme_select_dirs_refs_device with far predictors and reference-index bits that make the totals dir_bits + ref_bits (+ an MV's even bit
    count) odd for one reference and even for the next in either list: at 0x80000000 a candidate is priced at 32768 or at 0 by that parity
    alone; at the first wrap some totals wrap and some do not"""
    import select_dirs_refs_model as drm
    from hmme import api
    from test_gpu_select_dirs_refs import compare
    w, h = 100, 70
    n = sdm.n_ctus(w, h)
    pred = far_predictors((2, R, n), seed=900 + R)
    tabs = tuple(a[None] for a in drm.random_tables(R, n, n, 901 + R, pred, 0, lc.TINY, bi_gain=0))   # costs = distortions alone; uni and bi alike
    bits = drm.Bits((3, 3, 5), (R, R), ([1, 2, 3, 6][:R], [2, 1, 4, 3][:R]), 0b10 if R == 2 else 0b0101)
    totals = [{bits.dir_bits[l] + bits.ref_bits[l][r] for r in range(R)} for l in range(2)]
    assert all({t & 1 for t in totals[l]} == {0, 1} for l in range(2))
    priced, wrapped = [set(), set()], set()
    for l in range(2):
        for r in range(R):
            for k in range(n):
                for s in range(0, 593, 7):
                    bu = sdm.mvb(tabs[0][0, l, r, k, s], pred[l, r, k])
                    assert bu % 2 == 0
                    priced[l].add(sdm.gc(lq, bits.dir_bits[l] + bits.ref_bits[l][r] + bu))
                    wrapped.add(lc.wraps(lq, bits.dir_bits[l] + bits.ref_bits[l][r] + bu))
    if lq == lc.HALF:
        assert priced == [{0, 32768}, {0, 32768}] and wrapped == {True}
    else:
        assert wrapped == {False, True}
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12)
    with at(engine, lq):
        _, mr, md, ms, _ = compare(engine, w, h, tabs, sel, [bits], pred[None], lambda_q16=lq)
    coded = ms != sm.NO_SLOT
    assert len(set(md[coded].tolist())) >= 2 and (md[0] == 1).any()
    if lq == lc.HALF:                                                           # 32768 is more than any distortion here: the parity alone rules a reference out
        assert all((bits.dir_bits[l] + bits.ref_bits[l][r]) % 2 == 0 for l in range(2) for r in set(mr[0, l][md[0] == l + 1].tolist()))


# ---- f: one chain end to end ------------------------------------------------------------------------------------------------------------
def test_chain_search_refine_select_predict_at_the_first_wrap(engine, oracle_lib, hmo):
    """out_sad = cost - getCost(winner) of the search feeds the refinement, whose costs feed the decision, whose field feeds the prediction"""
    from hmme import api, synth
    m, lq, bd = synth.MARGIN, lc.WRAP24, 8
    cur, ref, _ = search_content("lownoise")      # large PUs follow the motion (few bits), small ones the MV cost (24 bits: cost 0)
    pred = synth.random_predictors(F_CTUS, seed=4244, max_pel=6)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), FW, FH, 16, pred, lq, 1, bd, n_threads=6)
    omv = np.stack([ox, oy], axis=-1).astype(np.int16)
    oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), FW, FH, omv, pred, lq, 1, bd, n_threads=6)
    bits = [lc.mv_bits(int(oq[k, s, 0]), int(oq[k, s, 1]), *pred[k]) for k in range(F_CTUS) for s in range(593)]
    assert any(b >= 24 for b in bits) and any(b < 24 for b in bits)
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12)
    mf, ms, mc, _ = sm.select_picture(oq, oc, sel, FW, FH)
    want = oracle_prediction(hmo, ref, FW, FH, bd, mf)[:FH, :FW]
    pc, pr = mkplane(engine, cur, FW, FH, bd), mkplane(engine, ref, FW, FH, bd)
    try:
        with at(engine, lq):
            mv, sad = engine.search_frame(pc, pr, 16, pred, fen=1)
            assert np.array_equal(mv, omv) and np.array_equal(sad, osad), (diff(mv, omv), diff(sad, osad))
            q, c = engine.refine_frame(pc, pr, 16, mv, pred, use_hadamard=True)
            assert np.array_equal(q, oq) and np.array_equal(c, oc), (diff(q, oq), diff(c, oc))
            f, s, cc = engine.select_frame(FW, FH, sel, q, c)
            assert np.array_equal(f, mf) and np.array_equal(s, ms) and np.array_equal(cc, mc)
            got = engine.predict_frame(pr, f)
            assert np.array_equal(got.astype(np.int16), want)
    finally:
        pc.close(); pr.close()


# ---- the range of hmme_set_lambda ---------------------------------------------------------------------------------------------------------
def test_set_lambda_refuses_what_does_not_fit_32_bits(engine):
    L = engine.L
    was = L.hmme_set_error_printing(engine.h, 0)
    try:
        with at(engine, 12345):
            for lam in (4294967296.0, 4294967296.0 * 4, 1.0e300, math.inf, -math.inf, math.nan, -1.0):
                assert L.hmme_set_lambda(engine.h, lam) == ERR_ARG, lam
                assert engine.lambda_q16 == 12345, lam                     # the context's value is unchanged
            for lq in (lc.ALL_ONES, lc.HALF, lc.WRAP24, lc.BELOW_ONE, lc.ABOVE_ONE, lc.TINY):
                engine.set_lambda(lc.as_double(lq))
                assert engine.lambda_q16 == lq
            engine.set_lambda(0.0)
            assert engine.lambda_q16 == 0
            for q in (-1, 1 << 32, (1 << 32) + 5, 1 << 40):
                with pytest.raises(ValueError):
                    engine.set_lambda_q16(q)
                assert engine.lambda_q16 == 0
            engine.set_lambda_q16(lc.ALL_ONES)
            assert engine.lambda_q16 == lc.ALL_ONES
    finally:
        L.hmme_set_error_printing(engine.h, was)
    assert engine.lambda_q16 == int(math.floor(65536.0 * math.sqrt(DEFAULT_LAMBDA)))
