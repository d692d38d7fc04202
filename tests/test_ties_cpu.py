"""The inputs of tests/test_gpu_ties.py, held to the oracle and to the conditions that keep the GPU tests from passing emptily
(tests/tie_content.py): the analytic tie sets of the skewed lattices against the oracle's 64x64 winner, the flat refinement model against
the oracle on the whole offset grid -- and, on the oracle and the models alone, that the ties these inputs hold are of the kind an order other
than HM's would decide differently.  tests/test_oracle_vs_ref.py holds the oracle to the reference's own code on the same content."""
import numpy as np
import pytest

import lambda_cases as lc
import tie_content as tc
from refine_tables import oracle_windows

W, H = tc.SEARCH_W, tc.SEARCH_H


def tie_sets(lattice, sr, seed, lq):
    """-> per CTU: (window, predictor, tie_set or None)"""
    pred = tc.search_predictors(sr, seed)
    win = oracle_windows(W, H, sr, pred)
    out = []
    for ctu in range(9):
        cu = (64 * (ctu % 3), 64 * (ctu // 3))
        out.append((win[ctu], pred[ctu], tc.tie_set(win[ctu], pred[ctu], lq, lattice, tc.LATTICE_SHIFT, (W, H) + cu)))
    return out


@pytest.mark.parametrize("lattice,sr", [(lat, sr) for lat in tc.LATTICES for sr in (8, 64)] + [(tc.LATTICES[3], 128)])
def test_tie_sets_are_the_oracles_winners_and_need_the_raster_order(oracle_lib, lattice, sr):
    """every (lattice, search range) tests/test_gpu_ties.py runs, with its predictor sets: the model against the oracle's 64x64 slot, and the
    conditions on the tie sets, counted at lambda_q16 0 and 1 << 13"""
    from hmme import synth
    m = synth.MARGIN
    cur, ref = tc.skewed_lattice(W, H, *lattice, 8, seed=11)
    differs = quads = spread = zero = 0
    for lq in tc.SEARCH_LAMBDA_Q16:
        for seed in tc.PRED_SEEDS[sr]:
            for ctu, (win, pred, ts) in enumerate(tie_sets(lattice, sr, seed, lq)):
                cu = (64 * (ctu % 3), 64 * (ctu // 3))
                p = oracle_lib.make_params((int(win[0]), int(win[1])), (int(win[2]), int(win[3])), (int(pred[0]), int(pred[1])), lq, 0, 8)
                x, y, sad = oracle_lib.pattern_search(cur, (m + cu[0], m + cu[1]), ref, (m + cu[0], m + cu[1]), 64, 64, p)
                if sad == 0:
                    zero += 1
                    assert ts is not None and (x, y) == ts["raster_first"], (lq, seed, ctu, (x, y), ts)
                if ts is None or lq not in (0, 1 << 13):
                    continue
                # the conditions: counted at lambda_q16 0 and 1 << 13 only
                n = len(ts["members"])
                differs += n >= 3 and ts["raster_first"] != ts["column_first"] and ts["raster_first"] != ts["last"]
                quads += tc.ties_in_one_quad(ts["members"], int(win[0])) > 0
                rows = {}
                for mx, my in ts["members"].tolist():
                    rows.setdefault(my, set()).add((mx - int(win[0])) // 4)
                spread += any(len(g) >= 2 for g in rows.values())
    assert zero >= 9, zero
    assert differs >= 1, "no CTU whose first tied candidate by rows differs from the first by columns and from the last"
    if lattice[0] < 4:
        assert quads >= 1, "no CTU with two tied candidates inside one aligned group of four columns of a row"
    else:
        # two lattice points of one row lie px >= 5 columns apart: never inside one group of four columns.  What these lattices give
        # instead is ties between neighbouring groups of a row, and between rows
        assert quads == 0
    assert spread >= 1


def test_lattice_content_is_periodic_inside_the_picture_only():
    for lattice in tc.LATTICES:
        px, py, s = lattice
        for bd in (8, 10, 12):
            tile = tc.lattice_tile(px, py, bd, seed=11)
            ys, xs = np.mgrid[-9:40, -9:40]
            v = tc.lattice_value(tile, s, xs, ys)
            assert np.array_equal(v, tc.lattice_value(tile, s, xs + px, ys)) and np.array_equal(v, tc.lattice_value(tile, s, xs + s, ys + py))
            # no shorter period: all samples of the tile differ, and the lattice test names exactly the equal displacements
            for dy in range(-3, 4):
                for dx in range(-7, 8):
                    same = np.array_equal(v, tc.lattice_value(tile, s, xs + dx, ys + dy))
                    assert same == bool(tc.on_lattice(lattice, (0, 0), dx, dy)), (lattice, dx, dy)
        from hmme import synth
        m = synth.MARGIN
        cur, ref = tc.skewed_lattice(W, H, *lattice, 8, seed=11)
        sx, sy = tc.LATTICE_SHIFT
        assert np.array_equal(cur[m + 64:m + 128, m + 64:m + 128], ref[m + 64 + sy:m + 128 + sy, m + 64 + sx:m + 128 + sx])
        # the edge replication breaks the period: column -1 repeats column 0, the lattice function does not
        assert (ref[m:m + 64, m - 1] != tc.lattice_value(tc.lattice_tile(px, py, 8, 11), s, np.full(64, -1), np.arange(64))).all()
        wcur, _ = tc.skewed_lattice(W, H, *lattice, 8, seed=11, weight=tc.WP)
        assert not np.array_equal(wcur, cur)


def test_two_match_cases_tie_exactly(oracle_lib):
    for bd, cases in ((8, tc.TWO_MATCH_8), (10, tc.TWO_MATCH_16)):
        for name, sr, a, b in cases:
            assert tc.raster_before(a, b) and b[0] < a[0], name
            assert max(abs(v) for v in a + b) <= sr
            pred = tc.tie_predictor(a, b)
            bits_a, bits_b = lc.mv_bits(4 * a[0], 4 * a[1], *pred), lc.mv_bits(4 * b[0], 4 * b[1], *pred)
            assert lc.get_cost(tc.Q16_57_9, bits_a) == lc.get_cost(tc.Q16_57_9, bits_b) > 0, (name, pred, bits_a, bits_b)
            assert lc.get_cost(0, bits_a) == lc.get_cost(0, lc.mv_bits(4 * b[0], 4 * b[1], 0, 0)) == 0
    t = {name: (tc.tile_of(a, sr), tc.tile_of(b, sr)) for name, sr, a, b in tc.TWO_MATCH_8 if sr > 64}
    assert t["one tile of four"][0] == t["one tile of four"][1]
    assert t["right tile then left tile one row lower"] == ((1, 0), (0, 0))
    assert t["vertically adjacent tiles"] == ((1, 0), (1, 1)) and t["diagonal tiles"] == ((1, 0), (0, 1))
    p = {name: ((a[0] + sr) & 1, (b[0] + sr) & 1, b[1] - a[1]) for name, sr, a, b in tc.TWO_MATCH_16}
    assert p["different column parity"][0] != p["different column parity"][1]
    assert p["one strip"][0] == p["one strip"][1] and p["one strip"][2] == 1 and p["sixty rows apart"][2] >= 60
    # the small case on the oracle: both copies give SAD 0 in every slot, the first in raster order wins
    from hmme import synth
    m = synth.MARGIN
    name, sr, a, b = tc.TWO_MATCH_8[0]
    cur, ref = tc.two_match(8, 31, a, b, tc.two_match_size(sr))
    _, cu_x, cu_y = tc.centre_ctu(tc.two_match_size(sr))
    for lq, pred in ((0, (0, 0)), (tc.Q16_57_9, tc.tie_predictor(a, b))):
        p = oracle_lib.make_params((-sr, -sr), (sr, sr), pred, lq, 1, 8)
        ox, oy, osad = oracle_lib.search_ctu(cur, (m + cu_x, m + cu_y), ref, (m + cu_x, m + cu_y), p)
        assert (ox == a[0]).all() and (oy == a[1]).all() and (osad == 0).all()


def test_refinement_inputs_cover_the_offset_grid():
    pred, imv = tc.refine_inputs()
    offs = tc.refine_offsets(pred, imv)
    assert {(x, y) for x in range(-9, 11) for y in range(-9, 11)} <= offs
    assert {(int(p[0]) & 3, int(p[1]) & 3) for p in pred} == {(a, b) for a in range(4) for b in range(4)}
    win = oracle_windows(tc.RW, tc.RH, tc.R_SR, pred)
    assert (imv >= win[:, None, 0:2]).all() and (imv <= win[:, None, 2:4]).all()


@pytest.mark.parametrize("lam", tc.REFINE_LAMBDAS)
def test_flat_refine_model_equals_the_oracle_and_the_order_decides(oracle_lib, lam):
    """the model against the oracle on every offset of the inputs (Hadamard and SAD, a small and a large block); and on the model alone: with
    the two tables swapped, or with a 3 x 3 raster order, some answers change at each non-zero lambda -- at lambda 0 the centre, first in
    every order, wins both stages"""
    from hmme import synth
    m = synth.MARGIN
    lq = tc.lambda_q16_of(lam)
    assert lq == oracle_lib.oracle().hmo_lambda_q16(lam)
    pred, imv = tc.refine_inputs()
    cur, ref = tc.refine_content("flat", tc.RW, tc.RH, 8, seed=3)
    mq, mc = tc.flat_refine_tables(pred, imv, lq)
    seen = set()
    for c in range(tc.R_CTUS):
        for s in range(25):          # the 25 integer MVs of a CTU recur every 25 slots
            key = (int(4 * imv[c, s, 0] - pred[c, 0]), int(4 * imv[c, s, 1] - pred[c, 1]))
            seen.add(key)
            for had, (bw, bh) in ((1, (8, 4)), (0, (16, 16)), (1, (16, 16))):
                mv = (int(imv[c, s, 0]), int(imv[c, s, 1]))
                hx, hy, qx, qy, cost = oracle_lib.frac_refine(cur, (m + 64, m + 64), ref, (m + 64, m + 64), bw, bh, mv, (int(pred[c, 0]), int(pred[c, 1])), lq, had, 8)
                dist = oracle_lib.frac_refine(cur, (m + 64, m + 64), ref, (m + 64, m + 64), bw, bh, mv, (int(pred[c, 0]), int(pred[c, 1])), 0, had, 8)[4]
                assert (4 * mv[0] + 2 * hx + qx, 4 * mv[1] + 2 * hy + qy, cost - dist) == (int(mq[c, s, 0]), int(mq[c, s, 1]), int(mc[c, s])), (key, had, bw)
    assert len(seen) == 400
    swapped, _ = tc.flat_refine_tables(pred, imv, lq, (tc.REFINE_Q, tc.REFINE_H))
    raster, _ = tc.flat_refine_tables(pred, imv, lq, (tc.RASTER_3X3, tc.RASTER_3X3))
    n_swapped = int((swapped[:, :25] != mq[:, :25]).any(axis=2).sum())
    n_raster = int((raster[:, :25] != mq[:, :25]).any(axis=2).sum())
    if lq == 0:
        assert n_swapped == 0 and np.array_equal(mq, 4 * imv) and (mc == 0).all()
    else:
        assert n_swapped >= 1 and n_raster >= 1, (n_swapped, n_raster)


@pytest.mark.parametrize("kind", ["rows", "cols"])
def test_one_component_of_the_mv_does_not_change_the_distortion(oracle_lib, kind):
    """rows / cols: at lambda 0 the distortion alone decides, and it is the same along one axis -- the winner of each stage is the first of
    the tied points in the table's order, which for `cols` is not the first in raster order"""
    from hmme import synth
    m = synth.MARGIN
    for bd in (8, 10):
        cur, ref = tc.refine_content(kind, tc.RW, tc.RH, bd, seed=3)
        for had in (0, 1):
            for (bw, bh) in ((8, 4), (16, 16)):
                hx, hy, qx, qy, _ = oracle_lib.frac_refine(cur, (m + 64, m + 64), ref, (m + 64, m + 64), bw, bh, (0, 0), (0, 0), 0, had, bd)
                if kind == "rows":
                    assert hx == 0 and qx == 0, (bd, had, bw, (hx, hy, qx, qy))
                else:   # s_acMvRefineH has (-1, 0) and (1, 0) in front of the corners, s_acMvRefineQ has (-1, -1) and (1, -1) in front of them
                    assert hy == 0 and qy == (0 if qx == 0 else -1), (bd, had, bw, (hx, hy, qx, qy))
