"""The integer-MV tables of tests/refine_tables.py do what they are for; the oracle's window equals the library's for every CTU the GPU tests
refine; and the oracle's xPatternSearchFracDIF equals the reference's at window corners, clipMv extremes and far predictors -- live where the
compiled reference is present, and against its recorded answers (tests/golden/frac_edges.npz) everywhere.  No GPU."""
import os

import numpy as np
import pytest

import refine_tables as rt
from conftest import GOLDEN


@pytest.fixture(scope="module")
def built(oracle_lib):
    return oracle_lib


def _cases():
    return rt.gpu_window_cases()


def test_every_kind_does_what_it_is_for(built):
    seen_collapsed = 0
    for name, w, h, sr, mid in _cases():
        win = rt.oracle_windows(w, h, sr, mid)
        tabs = rt.tables(win, sr, seed=7)
        assert set(tabs) == set(rt.KINDS)
        for ctu, (ltx, lty, rbx, rby) in enumerate(win):
            tag = (name, w, h, sr, ctu)
            lo, hi = np.array([ltx, lty]), np.array([rbx, rby])
            n_cand = (rbx - ltx + 1) * (rby - lty + 1)
            # corners: all eight positions, nothing else
            want8 = {tuple(p) for p in rt.eight_positions(win[ctu])}
            assert {tuple(v) for v in tabs["corners"][ctu]} == want8, tag
            assert {(ltx, lty), (rbx, lty), (rbx, rby), (ltx, rby)} <= want8
            for k, p in zip(rt.ONE_CORNER, ((ltx, lty), (rbx, rby), (ltx, rby), (rbx, lty))):
                assert (tabs[k][ctu] == np.array(p)).all(), (tag, k)
            # distinct: in the window, 593 different MVs (or every candidate of a smaller window)
            d = tabs["distinct"][ctu].astype(np.int64)
            assert (d >= lo).all() and (d <= hi).all(), tag
            assert len({tuple(v) for v in d}) == min(593, n_cand), tag
            # outside: beyond each of the four sides, both int16 extremes, both components at once, and some entries inside
            o = tabs["outside"][ctu].astype(np.int64)
            assert (o[:, 0] < ltx).any() and (o[:, 0] > rbx).any() and (o[:, 1] < lty).any() and (o[:, 1] > rby).any(), tag
            assert (o == 32767).any() and (o == -32768).any(), tag
            out_c = (o < lo) | (o > hi)
            assert out_c.all(axis=1).any() and (~out_c).all(axis=1).any() and (out_c[:, 0] & ~out_c[:, 1]).any() and (~out_c[:, 0] & out_c[:, 1]).any(), tag
            assert (o[:, 0] == ltx - 1).any() or (o[:, 0] == rbx + 1).any(), tag
            assert (o[:, 0] == ltx - sr).any() or (o[:, 0] == rbx + sr).any(), tag
            # mixed: about a third outside, every corner position present, the rest distinct
            mx = tabs["mixed"][ctu].astype(np.int64)
            n_out = int(((mx < lo) | (mx > hi)).any(axis=1).sum())
            assert 100 <= n_out <= 198, (tag, n_out)
            assert want8 <= {tuple(v) for v in mx}, tag
            seen_collapsed += int(n_cand == (sr + 1) ** 2)
        # the clamped twin is np.clip against the oracle's window
        for k, t in tabs.items():
            c = rt.clamp(t, win)
            for ctu in range(len(win)):
                assert np.array_equal(c[ctu], np.clip(t[ctu].astype(np.int64), win[ctu, 0:2], win[ctu, 2:4])), (name, k, ctu)
            assert c.dtype == np.int16 and c.shape == t.shape
            if k not in ("outside", "mixed"):
                assert np.array_equal(c, t), (name, k)
    assert seen_collapsed >= 6 * 4 * len(rt.COLLAPSED_SR)


def test_windows_of_the_gpu_cases(built):
    """what the GPU tests assert about their windows holds for the oracle's windows, and the library's host-side hmme_set_search_range gives
    the same window for every CTU and centre they use"""
    from hmme import api
    n = 0
    for name, w, h, sr, mid in _cases():
        win = rt.oracle_windows(w, h, sr, mid)
        cx_n = (w + 63) // 64
        for ctu in range(len(win)):
            qx, qy = (int(mid[ctu, 0]), int(mid[ctu, 1])) if mid is not None else (0, 0)
            got = api.set_search_range(qx, qy, sr, (ctu % cx_n) * 64, (ctu // cx_n) * 64, w, h)
            assert tuple(int(v) for v in got) == tuple(int(v) for v in win[ctu]), (name, w, h, sr, ctu, (qx, qy))
            n += 1
        if name == "full":
            assert tuple(win[rt.FULL["ctu"]]) == (-128, -128, 128, 128)
        if name == "edges":
            for ctu, (sx, sy) in zip((0, 2, 3, 5), rt.DIAGONALS):
                lim = rt.clip_limits(ctu, w, h)
                assert win[ctu, 0 if sx < 0 else 2] == lim[0 if sx < 0 else 2] and win[ctu, 1 if sy < 0 else 3] == lim[1 if sy < 0 else 3], (sr, ctu)
        if name == "far":
            # xSetSearchRange clips the predictor first (TEncSearch.cpp:3817-3818), so a predictor beyond the clipMv limit leaves the window
            # with sr + 1 candidates per direction, pinned to the limit: the narrowest window a picture-level call can have
            sx, sy = np.sign(mid[0, 0]), np.sign(mid[0, 1])
            for ctu in range(len(win)):
                lim = rt.clip_limits(ctu, w, h)
                assert win[ctu, 2] - win[ctu, 0] == sr and win[ctu, 3] - win[ctu, 1] == sr
                assert win[ctu, 0 if sx < 0 else 2] == lim[0 if sx < 0 else 2] and win[ctu, 1 if sy < 0 else 3] == lim[1 if sy < 0 else 3]
    assert n > 60
    pred, center = rt.family_predictors()
    assert not np.array_equal(rt.oracle_windows(rt.EDGE_W, rt.EDGE_H, rt.FAMILY_SR, pred), rt.oracle_windows(rt.EDGE_W, rt.EDGE_H, rt.FAMILY_SR, center))


def _golden():
    return np.load(os.path.join(GOLDEN, "frac_edges.npz"))


def test_edge_cases_cover_what_they_name(built):
    rows = rt.frac_edge_cases()
    col = {k: i for i, k in enumerate(rt.EDGE_COLUMNS)}
    full = rows[rows[:, col["picture"]] == 0]
    assert {(int(r[col["int_x"]]), int(r[col["int_y"]])) for r in full} == {(-128, -128), (128, -128), (128, 128), (-128, 128)}
    edge = rows[rows[:, col["picture"]] == 1]
    assert {(int(r[col["ctu"]]), int(r[col["int_x"]]), int(r[col["int_y"]])) for r in edge} == {(0, -71, -71), (2, 15, -71), (3, -71, 15), (5, 15, 15)}
    far = edge[np.abs(edge[:, col["pred_x"]]) == rt.FAR]
    assert {int(v) for v in far[:, col["lambda_x10"]]} == {0, 579, 40000} and len(far) >= 96
    for c, vals in (("bit_depth", {8, 10}), ("had", {0, 1})):
        assert {int(v) for v in rows[:, col[c]]} == vals
    # the block of a picture-corner case lies 71 samples outside the picture, the filter support inside the 80-sample margin
    assert 71 + 3 + 4 <= 80


def test_oracle_refinement_matches_the_reference_at_the_edges(built):
    """frac_refine(..., use_ref=True) == frac_refine(...) on every case.  Where the compiled reference is present it answers live, and its
    answers must equal the recorded ones; elsewhere the recorded answers stand in for it (as in tests/test_oracle_vs_ref.py)"""
    live = built.ref_available()
    g = _golden()
    rows = rt.frac_edge_cases()
    assert np.array_equal(rows, g["rows"])
    planes, table = rt.edge_case_planes(), built.slot_table()
    for i, row in enumerate(rows):
        recorded = tuple(int(v) for v in g["out"][i])
        want = rt.run_edge_case(built, row, planes, table, use_ref=True) if live else recorded
        assert rt.run_edge_case(built, row, planes, table) == want, (i, row.tolist(), want)
        assert want == recorded, (i, row.tolist())
        if live:
            assert built.ref().ref_lambda_q16(int(row[-1]) / 10.0) == int(g["lambda_q16"][i])


def test_oracle_refinement_matches_the_recorded_reference_at_the_edges(built):
    g = _golden()
    rows = rt.frac_edge_cases()
    assert np.array_equal(rows, g["rows"]) and g["columns"].tolist() == rt.EDGE_COLUMNS and len(rows) >= 300
    planes, table = rt.edge_case_planes(), built.slot_table()
    for i, row in enumerate(rows):
        assert built.oracle().hmo_lambda_q16(int(row[-1]) / 10.0) == int(g["lambda_q16"][i])
        assert rt.run_edge_case(built, row, planes, table) == tuple(int(v) for v in g["out"][i]), (i, row.tolist())
