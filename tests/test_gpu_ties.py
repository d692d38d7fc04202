"""Partial ties on the device: where some candidates cost the same and the others do not, HM's answer is its loop order's alone -- the raster
order of the window in the search, the order of s_acMvRefineH / s_acMvRefineQ in the refinement -- and the kernels reach it through the tags
of their keys: (iteration, lane, j) in the 8-bit search, (lane, j) per task, two column-parity passes and strips in the 16-bit search, 2 x 2
tiles beyond 129 x 129 candidates, idxH / idxQ in the refinement.  The content is tests/tie_content.py's (skewed lattices of candidates with
SAD 0, a block planted twice, flat pictures and pictures constant along one axis); tests/test_ties_cpu.py asserts on the oracle and the models
alone that these inputs hold ties an order other than HM's decides differently, tests/test_oracle_vs_ref.py holds the oracle to the
reference's own code on them.  Everything here is bit for bit against the oracle, all 593 slots.  The picture search's launch forms are
selected as tests/test_gpu_tree_linearity.py selects them: one child process per planner mode, each running every case.

Seen to fail on builds with a wrong order (scratch builds, wrong results only), first failing case of each:
  refinement, the two point tables swapped        test_refinement_plain[8-flat], caller's table, Hadamard, lambda 1.0: CTU 0 slot 1, y (23 tests fail)
  refinement, `d <= best` in the winner loop      test_refinement_plain[8-flat], caller's table, Hadamard, lambda 0: CTU 0 slot 0, x (23 tests fail)
  16-bit search, key tag 63 - lane, decode to match   test_16bit_lattices[10-lat0-8], FEN 0, lambda 0, seed 1: CTU 0 slot 0 (57 tests fail)
  8-bit search, key tag 63 - lane, decode to match    test_8bit_lattices_every_launch_form[lat0-8], per-CTU call, CTU 0 (14 tests fail; of the
                                                   two_match cases only `one tile` at lambda 0: across tasks and tiles (cost, y, x) decides)"""
import functools

import numpy as np
import pytest

import tie_content as tc
from frame_helpers import bind_hmo, ctu_origin, mkplane, oracle_bi_search, oracle_prediction, oracle_search_w, origin_picture
from refine_tables import oracle_windows
from test_gpu_lambda_edges import TAIL_MODES, at, diff, run_children

pytestmark = pytest.mark.gpu

W, H, N_CTU = tc.SEARCH_W, tc.SEARCH_H, tc.SEARCH_CTUS
SEED = 11
# (lattice, search range, FEN, lambda_q16, predictor seed): search range 8 the full cross product; 64 once per lattice and lambda, FEN alternating
CASES_8 = [(lat, 8, fen, lq, seed) for lat in tc.LATTICES for fen in (0, 1) for lq in tc.SEARCH_LAMBDA_Q16 for seed in tc.PRED_SEEDS[8]]
CASES_64 = [(lat, 64, (i + j) & 1, lq, tc.PRED_SEEDS[64][0]) for i, lat in enumerate(tc.LATTICES) for j, lq in enumerate(tc.SEARCH_LAMBDA_Q16)]
SEARCH_CASES = CASES_8 + CASES_64


def key(lat, sr, fen, lq, seed):
    return "%d_%d_%d_%d_%d_%d_%d" % (lat + (sr, fen, lq, seed))


@functools.lru_cache(maxsize=None)
def lattice_pair(lat, bd, weight=None, shift=tc.LATTICE_SHIFT):
    cur, ref = tc.skewed_lattice(W, H, *lat, bd, seed=SEED, shift=shift, weight=weight)
    cur.setflags(write=False); ref.setflags(write=False)
    return cur, ref


_SEARCH_HELPER = """
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_ties as T
import tie_content as tc
from hmme import api, synth
m, out = synth.MARGIN, {}
with api.Engine(0, 64) as e:
    for lat, sr, fen, lq, seed in T.SEARCH_CASES:
        cur, ref = T.lattice_pair(lat, 8)
        e.set_lambda_q16(lq)
        with e.plane(T.W, T.H) as pc, e.plane(T.W, T.H) as pr:
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            mv, sad = e.search_frame(pc, pr, sr, tc.search_predictors(sr, seed), fen=fen)
        out["mv_" + T.key(lat, sr, fen, lq, seed)], out["sad_" + T.key(lat, sr, fen, lq, seed)] = mv, sad
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def search_tables(tmp_path_factory):
    return run_children(_SEARCH_HELPER, TAIL_MODES, tmp_path_factory.mktemp("ties_search"))


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(57.9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine128():
    from hmme import api
    e = api.Engine(0, 128)
    e.set_lambda(57.9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def same(got_mv, got_sad, omv, osad, what):
    assert np.array_equal(got_mv, omv), (what, diff(got_mv, omv))
    assert np.array_equal(got_sad, osad), (what, diff(got_sad, osad))


def oracle_search(oracle_lib, cur, ref, w, h, sr, pred, lq, fen, bd, first=0, count=-1):
    from hmme import synth
    m = synth.MARGIN
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, fen, bd, first, count, n_threads=8)
    return np.stack([ox, oy], axis=-1).astype(np.int16), osad


def assert_the_lattice_ties_are_met(omv, osad, lat, win, pred, lq, shift=tc.LATTICE_SHIFT):
    """CTU 4, whose whole window lies in the picture: the oracle's 64x64 winner has SAD 0 and is the analytic tie set's first member in
    raster order.  (That the tie sets hold several members whose first by rows is not the first by columns: tests/test_ties_cpu.py)"""
    ts = tc.tie_set(win[4], pred[4], lq, lat, shift, (W, H, 64, 64))
    assert ts is not None and int(osad[4, 592]) == 0 and (int(omv[4, 592, 0]), int(omv[4, 592, 1])) == ts["raster_first"], (lat, lq, ts)
    return len(ts["members"])


def per_ctu_calls(e, cur, ref, win, pred, fen, bd, omv, osad, ctus, wp=None):
    from hmme import api, synth
    m = synth.MARGIN
    for ctu in ctus:
        cx, cy = ctu_origin(ctu, W)
        p = api.SearchParams(*(int(v) for v in win[ctu]), int(pred[ctu, 0]), int(pred[ctu, 1]), fen, bd)
        if wp is None:
            mv, sad = e.search_ctu(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p)
        else:
            mv, sad = e.search_ctu_w(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p, wp)
        same(mv, sad, omv[ctu], osad[ctu], ("per-CTU call", ctu))


# ---- the 8-bit search ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [8, 64])
@pytest.mark.parametrize("lat", tc.LATTICES)
def test_8bit_lattices_every_launch_form(engine, oracle_lib, search_tables, lat, sr):
    """the per-CTU call on every CTU's own window (CTU 4: the whole window; the eight others at search range 64: windows the picture's limits
    clip, so quad counts other than 33 per row occur) and the picture search in the five planner modes"""
    cur, ref = lattice_pair(lat, 8)
    tied = 0
    for c_lat, c_sr, fen, lq, seed in SEARCH_CASES:
        if (c_lat, c_sr) != (lat, sr):
            continue
        pred = tc.search_predictors(sr, seed)
        win = oracle_windows(W, H, sr, pred)
        assert tuple(win[4][2:] - win[4][:2]) == (2 * sr, 2 * sr)
        if sr == 64:    # the picture's limits cut windows of the outer CTUs
            assert sum(tuple(win[c][2:] - win[c][:2]) != (2 * sr, 2 * sr) for c in range(N_CTU)) >= 4, win
        omv, osad = oracle_search(oracle_lib, cur, ref, W, H, sr, pred, lq, fen, 8)
        tied += assert_the_lattice_ties_are_met(omv, osad, lat, win, pred, lq) >= 2
        with at(engine, lq):
            per_ctu_calls(engine, cur, ref, win, pred, fen, 8, omv, osad, range(N_CTU))
        assert set(search_tables) == set(TAIL_MODES)
        for mode, t in search_tables.items():
            same(t["mv_" + key(lat, sr, fen, lq, seed)], t["sad_" + key(lat, sr, fen, lq, seed)], omv, osad, (mode, fen, lq, seed))
    assert tied >= (2 if sr == 8 else 1), tied


TWO_MATCH_LAMBDAS = (0, tc.Q16_57_9)


def two_match_case(oracle_lib, bd, sr, a, b, lq):
    """-> planes, picture size, centre CTU, predictors for the picture call, the centre CTU's window, the oracle's tables of that CTU (all 593
    slots: a, SAD 0).  The window is the whole 2 * sr + 1 candidates around the rounded predictor and holds a and b"""
    size = tc.two_match_size(sr)
    ctu, cu_x, cu_y = tc.centre_ctu(size)
    cur, ref = tc.two_match(bd, 31, a, b, size)
    pq = tc.tie_predictor(a, b, lq) if lq else (0, 0)
    pred = np.zeros(((size[0] // 64) * (size[1] // 64), 2), np.int16)
    pred[ctu] = pq
    omv, osad = oracle_search(oracle_lib, cur, ref, size[0], size[1], sr, pred, lq, 1, bd, ctu, 1)
    assert (omv[0, :, 0] == a[0]).all() and (omv[0, :, 1] == a[1]).all() and (osad == 0).all()
    win = tuple(int(v) for v in oracle_windows(size[0], size[1], sr, pred)[ctu])
    assert (win[2] - win[0], win[3] - win[1]) == (2 * sr, 2 * sr) and all(win[0] <= v[0] <= win[2] and win[1] <= v[1] <= win[3] for v in (a, b))
    return cur, ref, size, (ctu, cu_x, cu_y), pred, win, omv, osad


@pytest.mark.parametrize("lq", TWO_MATCH_LAMBDAS)
@pytest.mark.parametrize("name,sr,a,b", tc.TWO_MATCH_8)
def test_8bit_two_matches(engine, engine128, oracle_lib, name, sr, a, b, lq):
    """the CTU's block lies in the reference twice, a before b in raster order and to its right: in one tile, and in two tiles of the 2 x 2 a
    window of search range 128 is searched as -- the per-CTU call and the picture call on the centre CTU alone, whose window the picture's
    limits do not cut"""
    from hmme import api, synth
    m = synth.MARGIN
    e = engine128 if sr > 64 else engine
    cur, ref, size, (ctu, cu_x, cu_y), pred, win, omv, osad = two_match_case(oracle_lib, 8, sr, a, b, lq)
    tiles = [((v[0] - win[0]) // tc.TILE, (v[1] - win[1]) // tc.TILE) for v in (a, b)]     # counted from the window's top-left
    assert tiles == {"one tile": [(0, 0), (0, 0)], "one tile of four": [(0, 0), (0, 0)], "right tile then left tile one row lower": [(1, 0), (0, 0)],
                     "vertically adjacent tiles": [(1, 0), (1, 1)], "diagonal tiles": [(1, 0), (0, 1)]}[name], (name, win, tiles)
    with at(e, lq):
        p = api.SearchParams(*win, int(pred[ctu, 0]), int(pred[ctu, 1]), 1, 8)
        mv, sad = e.search_ctu(cur, (m + cu_x, m + cu_y), ref, (m + cu_x, m + cu_y), p)
        assert (int(mv[592, 0]), int(mv[592, 1])) == a, (name, "per-CTU call", mv[592])
        same(mv, sad, omv[0], osad[0], (name, "per-CTU call"))
        pc, pr = mkplane(e, cur, size[0], size[1], 8), mkplane(e, ref, size[0], size[1], 8)
        try:
            mv, sad = e.search_frame(pc, pr, sr, pred, fen=1, ctu_first=ctu, ctu_count=1)
        finally:
            pc.close(); pr.close()
        assert (int(mv[0, 592, 0]), int(mv[0, 592, 1])) == a, (name, "picture call", mv[0, 592])
        same(mv, sad, omv, osad, (name, "picture call"))


# ---- the 16-bit search -------------------------------------------------------------------------------------------------------------------------
def cases_16(lat, sr):
    if sr == 8:
        return [(fen, lq, seed) for fen in (0, 1) for lq in tc.SEARCH_LAMBDA_Q16 for seed in tc.PRED_SEEDS[8]]
    return [((tc.LATTICES.index(lat) + j) & 1, lq, tc.PRED_SEEDS[sr][0]) for j, lq in enumerate(tc.SEARCH_LAMBDA_Q16)]


@pytest.mark.parametrize("sr", [8, 64])
@pytest.mark.parametrize("lat", tc.LATTICES)
@pytest.mark.parametrize("bd", [10, 12])
def test_16bit_lattices(engine, oracle_lib, bd, lat, sr):
    """me_search16_kernel: the picture search, and the per-CTU call on CTU 4 (the whole window) and CTU 0 (a clipped one)"""
    cur, ref = lattice_pair(lat, bd)
    pc, pr = mkplane(engine, cur, W, H, bd), mkplane(engine, ref, W, H, bd)
    tied = 0
    try:
        for fen, lq, seed in cases_16(lat, sr):
            pred = tc.search_predictors(sr, seed)
            win = oracle_windows(W, H, sr, pred)
            omv, osad = oracle_search(oracle_lib, cur, ref, W, H, sr, pred, lq, fen, bd)
            tied += assert_the_lattice_ties_are_met(omv, osad, lat, win, pred, lq) >= 2
            with at(engine, lq):
                mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
                same(mv, sad, omv, osad, (fen, lq, seed))
                per_ctu_calls(engine, cur, ref, win, pred, fen, bd, omv, osad, (4, 0))
    finally:
        pc.close(); pr.close()
    assert tied >= (2 if sr == 8 else 1), tied


def test_16bit_lattice_through_strips(engine128, oracle_lib):
    """search range 128: the windows (CTU 4: 193 x 193 candidates inside the picture's limits) are cut into strips that merge through the
    global table; lambda_q16 1 << 13 and 0, FEN 0 and 1"""
    lat, bd, sr = tc.LATTICES[3], 10, 128
    cur, ref = lattice_pair(lat, bd)
    pred = tc.search_predictors(sr, tc.PRED_SEEDS[sr][0])
    win = oracle_windows(W, H, sr, pred)
    pc, pr = mkplane(engine128, cur, W, H, bd), mkplane(engine128, ref, W, H, bd)
    try:
        for fen, lq in ((0, 1 << 13), (1, 0)):
            omv, osad = oracle_search(oracle_lib, cur, ref, W, H, sr, pred, lq, fen, bd)
            assert int(osad[4, 592]) == 0
            with at(engine128, lq):
                mv, sad = engine128.search_frame(pc, pr, sr, pred, fen=fen)
            same(mv, sad, omv, osad, (fen, lq))
    finally:
        pc.close(); pr.close()


@pytest.mark.parametrize("lq", TWO_MATCH_LAMBDAS)
@pytest.mark.parametrize("name,sr,a,b", tc.TWO_MATCH_16)
def test_16bit_two_matches(engine128, oracle_lib, name, sr, a, b, lq):
    """10 bit, search range 128: a and b in the two column-parity passes, in one strip, and sixty rows apart with b to the left of a"""
    from hmme import api, synth
    m = synth.MARGIN
    cur, ref, size, (ctu, cu_x, cu_y), pred, win, omv, osad = two_match_case(oracle_lib, 10, sr, a, b, lq)
    assert ((a[0] - win[0]) & 1 != (b[0] - win[0]) & 1) == (name == "different column parity")
    with at(engine128, lq):
        p = api.SearchParams(*win, int(pred[ctu, 0]), int(pred[ctu, 1]), 1, 10)
        mv, sad = engine128.search_ctu(cur, (m + cu_x, m + cu_y), ref, (m + cu_x, m + cu_y), p)
        assert (int(mv[592, 0]), int(mv[592, 1])) == a, (name, "per-CTU call", mv[592])
        same(mv, sad, omv[0], osad[0], (name, "per-CTU call"))
        pc, pr = mkplane(engine128, cur, size[0], size[1], 10), mkplane(engine128, ref, size[0], size[1], 10)
        try:
            mv, sad = engine128.search_frame(pc, pr, sr, pred, fen=1, ctu_first=ctu, ctu_count=1)
        finally:
            pc.close(); pr.close()
        assert (int(mv[0, 592, 0]), int(mv[0, 592, 1])) == a, (name, "picture call", mv[0, 592])
        same(mv, sad, omv, osad, (name, "picture call"))


@pytest.mark.parametrize("sr", [8, 64])
@pytest.mark.parametrize("lat", tc.LATTICES)
@pytest.mark.parametrize("bd", [8, 10])
def test_weighted_lattices(engine, oracle_lib, bd, lat, sr):
    """search_frame_w / search_ctu_w: the current picture is the weighted reference, shifted, so the WEIGHTED distortion is 0 on the lattice"""
    from hmme import api
    assert api.weight_check(bd, tc.WP, False) == 0 and tc.WP != (64, 0, 6, 32)
    cur, ref = lattice_pair(lat, bd, weight=tc.WP)
    assert not np.array_equal(cur, lattice_pair(lat, bd)[0])
    pc, pr = mkplane(engine, cur, W, H, bd), mkplane(engine, ref, W, H, bd)
    tied = 0
    try:
        cases = [(lq, seed) for lq in tc.SEARCH_LAMBDA_Q16 for seed in tc.PRED_SEEDS[8]] if sr == 8 else \
                [(lq, tc.PRED_SEEDS[64][0]) for lq in (0, 1 << 13)]
        for lq, seed in cases:
            pred = tc.search_predictors(sr, seed)
            win = oracle_windows(W, H, sr, pred)
            omv, osad = oracle_search_w(oracle_lib, cur, ref, W, H, sr, pred, lq, bd, tc.WP, range(N_CTU))
            tied += assert_the_lattice_ties_are_met(omv, osad, lat, win, pred, lq) >= 2
            with at(engine, lq):
                mv, sad = engine.search_frame_w(pc, pr, sr, tc.WP, pred, fen=1)
                same(mv, sad, omv, osad, (lq, seed))
                per_ctu_calls(engine, cur, ref, win, pred, 1, bd, omv, osad, (4, 8), wp=tc.WP)
    finally:
        pc.close(); pr.close()
    assert tied >= 1, tied


OTHER_SHIFT = (2, 1)


@pytest.mark.parametrize("sr", [8, 64])
@pytest.mark.parametrize("lat", tc.LATTICES)
@pytest.mark.parametrize("bd", [8, 10])
def test_bi_lattices(engine, oracle_lib, hmo, bd, lat, sr):
    """search_frame_bi under a zero field: the prediction of the other plane is that plane, so the origin 2 * cur - other has the lattice's
    period as well.  8 bit: the other plane is the current one, the origin is the current picture and the distortion 0 on the lattice;
    10 bit: the other plane is the lattice function at another shift, so no candidate has distortion 0 and the candidates of each coset of
    the lattice tie among themselves"""
    cur, ref = lattice_pair(lat, bd)
    other = cur if bd == 8 else lattice_pair(lat, bd, shift=OTHER_SHIFT)[0]
    field = np.zeros((N_CTU, 1, 2), np.int16)
    from hmme import synth
    m = synth.MARGIN
    org = origin_picture(cur, oracle_prediction(hmo, other, W, H, bd, field), W, H)
    assert np.array_equal(org, cur[m:m + H, m:m + W]) == (bd == 8)
    pc, pr, po = (mkplane(engine, a, W, H, bd) for a in (cur, ref, other))
    try:
        cases = [(fen, lq, seed) for fen in (0, 1) for lq in tc.SEARCH_LAMBDA_Q16 for seed in tc.PRED_SEEDS[8][:2]] if sr == 8 else \
                [((bd == 10) ^ (tc.LATTICES.index(lat) & 1), tc.SEARCH_LAMBDA_Q16[(tc.LATTICES.index(lat) + 1) % 4], tc.PRED_SEEDS[64][0])]
        for fen, lq, seed in cases:
            pred = tc.search_predictors(sr, seed)
            omv, osad = oracle_bi_search(oracle_lib, org, ref, W, H, sr, None, pred, lq, int(fen), bd, range(N_CTU))
            if bd == 8:
                assert_the_lattice_ties_are_met(omv, osad, lat, oracle_windows(W, H, sr, pred), pred, lq)
            with at(engine, lq):
                mv, sad = engine.search_frame_bi(pc, pr, po, sr, field, pred_q=pred, fen=int(fen))
            same(mv, sad, omv, osad, (fen, lq, seed))
    finally:
        pc.close(); pr.close(); po.close()


# ---- the refinement --------------------------------------------------------------------------------------------------------------------------------
RW, RH, R_SR, R_CTUS = tc.RW, tc.RH, tc.R_SR, tc.R_CTUS
REFINE_CASES = [(had, lam) for had in (1, 0) for lam in tc.REFINE_LAMBDAS]


@functools.lru_cache(maxsize=None)
def refine_pair(kind, bd):
    cur, ref = tc.refine_content(kind, RW, RH, bd, seed=3)
    cur.setflags(write=False); ref.setflags(write=False)
    return cur, ref


def assert_flat_model(kind, q, pred, imv, lq):
    if kind == "flat":
        mq, _ = tc.flat_refine_tables(pred, imv, lq)
        assert np.array_equal(q, mq), ("flat model", diff(q, mq))


@pytest.mark.parametrize("kind", tc.REFINE_KINDS)
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_refinement_plain(engine, oracle_lib, bd, kind):
    """refine_frame at the table of tie_content.refine_inputs (every offset 4 * int_mv - pred of -9..10 in both components), and at the
    table the device's own search returns (every slot of a CTU the same MV: the most sharing of work between slots)"""
    from hmme import synth
    m = synth.MARGIN
    cur, ref = refine_pair(kind, bd)
    pred, imv = tc.refine_inputs()
    pc, pr = mkplane(engine, cur, RW, RH, bd), mkplane(engine, ref, RW, RH, bd)
    try:
        for had, lam in REFINE_CASES:
            lq = tc.lambda_q16_of(lam)
            oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), RW, RH, imv, pred, lq, had, bd, n_threads=8)
            assert lq == 0 or (oq != 4 * imv).any()
            assert_flat_model(kind, oq, pred, imv, lq)
            with at(engine, lq):
                q, c = engine.refine_frame(pc, pr, R_SR, imv, pred, use_hadamard=bool(had))
                same(q, c, oq, oc, ("caller's table", had, lam))
                smv, ssad = engine.search_frame(pc, pr, R_SR, pred, fen=had)
                omv, osad = oracle_search(oracle_lib, cur, ref, RW, RH, R_SR, pred, lq, had, bd)
                same(smv, ssad, omv, osad, ("search", had, lam))
                q, c = engine.refine_frame(pc, pr, R_SR, smv, pred, use_hadamard=bool(had))
            oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), RW, RH, omv, pred, lq, had, bd, n_threads=8)
            same(q, c, oq, oc, ("the search's table", had, lam))
            assert_flat_model(kind, q, pred, omv, lq)
    finally:
        pc.close(); pr.close()


@pytest.mark.parametrize("kind", tc.REFINE_KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_refinement_weighted(engine, oracle_lib, bd, kind):
    """refine_frame_w under a served non-identity weight, three CTUs slot by slot against hmo_frac_refine_w"""
    from hmme import api, synth
    m = synth.MARGIN
    assert api.weight_check(bd, tc.WP, True) == 0
    cur, ref = refine_pair(kind, bd)
    pred, imv = tc.refine_inputs()
    table = oracle_lib.slot_table()
    pc, pr = mkplane(engine, cur, RW, RH, bd), mkplane(engine, ref, RW, RH, bd)
    try:
        for had, lam in REFINE_CASES:
            lq = tc.lambda_q16_of(lam)
            with at(engine, lq):
                q, c = engine.refine_frame_w(pc, pr, R_SR, tc.WP, imv, pred, use_hadamard=bool(had))
            for ctu in (0, 6, 15):
                cx, cy = ctu_origin(ctu, RW)
                pq = (int(pred[ctu, 0]), int(pred[ctu, 1]))
                for s in range(593):
                    x, y, bw, bh = (int(v) for v in table[s])
                    mv = (int(imv[ctu, s, 0]), int(imv[ctu, s, 1]))
                    hx, hy, qx, qy, oc = oracle_lib.frac_refine_w(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, mv, pq, lq, had, bd, tc.WP)
                    assert (int(q[ctu, s, 0]), int(q[ctu, s, 1]), int(c[ctu, s])) == (4 * mv[0] + 2 * hx + qx, 4 * mv[1] + 2 * hy + qy, oc), (had, lam, ctu, s)
            assert_flat_model(kind, q, pred, imv, lq)
    finally:
        pc.close(); pr.close()


@pytest.mark.parametrize("kind", tc.REFINE_KINDS)
@pytest.mark.parametrize("bd", [8, 10])
def test_refinement_bi(engine, oracle_lib, hmo, bd, kind):
    """refine_frame_bi with a flat other plane at the top of the sample range and a zero field: the origin 2 * cur - maxv lies outside the
    sample range"""
    from hmme import api, synth
    m = synth.MARGIN
    maxv = (1 << bd) - 1
    assert api.bipred_check(bd, True) == 0
    cur, ref = refine_pair(kind, bd)
    other = synth.pad_plane(np.full((RH, RW), maxv, np.int64))
    pred, imv = tc.refine_inputs()
    field = np.zeros((R_CTUS, 1, 2), np.int16)
    org = origin_picture(cur, oracle_prediction(hmo, other, RW, RH, bd, field), RW, RH)
    assert org.min() < 0
    org_padded = np.ascontiguousarray(np.pad(org, m))
    pc, pr, po = (mkplane(engine, a, RW, RH, bd) for a in (cur, ref, other))
    try:
        for had, lam in REFINE_CASES:
            lq = tc.lambda_q16_of(lam)
            oq, oc = oracle_lib.refine_frame(org_padded, ref, (m, m), RW, RH, imv, pred, lq, had, bd, n_threads=8)
            with at(engine, lq):
                q, c = engine.refine_frame_bi(pc, pr, po, R_SR, field, imv, pred_q=pred, use_hadamard=bool(had))
            same(q, c, oq, oc, (had, lam))
            assert_flat_model(kind, q, pred, imv, lq)
    finally:
        pc.close(); pr.close(); po.close()


@pytest.mark.parametrize("kind", ["flat", "rows"])
def test_refinement_per_ctu_calls(engine, oracle_lib, kind):
    """refine_ctu, refine_ctu_w and search_refine_ctu on CTU 5 of the refinement picture, 8 bit"""
    from hmme import api, synth
    m, bd, ctu = synth.MARGIN, 8, 5
    cur, ref = refine_pair(kind, bd)
    pred, imv = tc.refine_inputs()
    win = oracle_windows(RW, RH, R_SR, pred)
    cx, cy = ctu_origin(ctu, RW)
    o = (m + cx, m + cy)
    pq = (int(pred[ctu, 0]), int(pred[ctu, 1]))
    table = oracle_lib.slot_table()

    def oracle_tables(mvs, lq, had, wp=None):
        q, c = np.zeros((593, 2), np.int16), np.zeros(593, np.uint32)
        for s in range(593):
            x, y, bw, bh = (int(v) for v in table[s])
            mv = (int(mvs[s, 0]), int(mvs[s, 1]))
            if wp is None:
                hx, hy, qx, qy, c[s] = oracle_lib.frac_refine(cur, (o[0] + x, o[1] + y), ref, (o[0] + x, o[1] + y), bw, bh, mv, pq, lq, had, bd)
            else:
                hx, hy, qx, qy, c[s] = oracle_lib.frac_refine_w(cur, (o[0] + x, o[1] + y), ref, (o[0] + x, o[1] + y), bw, bh, mv, pq, lq, had, bd, wp)
            q[s] = (4 * mv[0] + 2 * hx + qx, 4 * mv[1] + 2 * hy + qy)
        return q, c

    for had, lam in REFINE_CASES:
        lq = tc.lambda_q16_of(lam)
        p = api.SearchParams(*(int(v) for v in win[ctu]), pq[0], pq[1], had, bd)
        with at(engine, lq):
            q, c = engine.refine_ctu(cur, o, ref, o, p, imv[ctu], use_hadamard=bool(had))
            same(q, c, *oracle_tables(imv[ctu], lq, had), ("refine_ctu", had, lam))
            q, c = engine.refine_ctu_w(cur, o, ref, o, p, tc.WP, imv[ctu], use_hadamard=bool(had))
            same(q, c, *oracle_tables(imv[ctu], lq, had, tc.WP), ("refine_ctu_w", had, lam))
            mv, sad, q, c = engine.search_refine_ctu(cur, o, ref, o, p, use_hadamard=bool(had))
        op = oracle_lib.make_params((int(win[ctu][0]), int(win[ctu][1])), (int(win[ctu][2]), int(win[ctu][3])), pq, lq, had, bd)
        ox, oy, osad = oracle_lib.search_ctu(cur, o, ref, o, op)
        omv = np.stack([ox, oy], axis=-1).astype(np.int16)
        same(mv, sad, omv, osad, ("search_refine_ctu: search", had, lam))
        same(q, c, *oracle_tables(omv, lq, had), ("search_refine_ctu: refinement", had, lam))
