"""The fractional-pel refinement at integer MVs the search would not produce (tests/refine_tables.py): window corners at the last value the
9-bit fields hold, the clipMv extremes of the picture corners, windows pinned to them by far predictors, 593 different MVs per CTU and MVs
outside the window, which the library clamps.  Expected values: the CPU oracle at the table clamped to the ORACLE's window.  Every comparison is
bit for bit, quarter-pel MV and cost, over all 593 slots of every refined CTU."""
import numpy as np
import pytest

import bipred_wp_model as model
import range_content as rc
import refine_tables as rt
from frame_helpers import bind_hmo, device_tables, mkplane, oracle_prediction, origin_picture, random_field, three_planes

pytestmark = pytest.mark.gpu

LAMBDA = 57.9
W, H = rt.EDGE_W, rt.EDGE_H


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


@pytest.fixture(scope="module")
def slot_rects(oracle_lib):
    return oracle_lib.slot_table()


def set_lambda(engine, oracle_lib, lam=LAMBDA):
    engine.set_lambda(lam)
    assert engine.lambda_q16 == oracle_lib.oracle().hmo_lambda_q16(lam)
    return engine.lambda_q16


def same(tag, qmv, cost, oq, oc):
    assert qmv.shape == oq.shape and cost.shape == oc.shape
    bad = np.argwhere((qmv != oq).any(axis=-1) | (cost != oc))
    assert len(bad) == 0, (tag, len(bad), [(tuple(b), qmv[tuple(b)].tolist(), oq[tuple(b)].tolist(), int(cost[tuple(b)]), int(oc[tuple(b)])) for b in bad[:4]])


def host_window(ctu, w, h, sr, mid):
    from hmme import api
    cx_n = (w + 63) // 64
    qx, qy = (int(mid[ctu, 0]), int(mid[ctu, 1])) if mid is not None else (0, 0)
    return tuple(int(v) for v in api.set_search_range(qx, qy, sr, (ctu % cx_n) * 64, (ctu // cx_n) * 64, w, h))


def refine_plain(engine, oracle_lib, pics, w, h, bd, sr, pred, had, names, lq, seed, first=0, count=-1, tag=()):
    """refine_frame at each named table against oracle_lib.refine_frame at its clamped twin"""
    from hmme import synth
    m = synth.MARGIN
    cur, ref = pics
    win = rt.oracle_windows(w, h, sr, pred)
    tabs = rt.tables(win, sr, seed)
    n = len(win) - first if count < 0 else count
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        for name in names:
            t = tabs[name][first:first + n]
            qmv, cost = engine.refine_frame(pc, pr, sr, t, pred, use_hadamard=bool(had), ctu_first=first, ctu_count=n)
            oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), w, h, rt.clamp(tabs[name], win)[first:first + n], pred, lq, had, bd, first, n, n_threads=8)
            same(tag + (name, bd, sr, had), qmv, cost, oq, oc)
    return win


# ---- full window: the field value 256 is the last one 9 bits hold ------------------------------------------------------------------------------
@pytest.mark.parametrize("had", [1, 0])
@pytest.mark.parametrize("bd", [8, 10])
def test_full_window_nine_bit_fields(engine, oracle_lib, bd, had):
    w, h, sr, ctu = rt.FULL["w"], rt.FULL["h"], rt.FULL["sr"], rt.FULL["ctu"]
    assert host_window(ctu, w, h, sr, None) == (-128, -128, 128, 128)
    lq = set_lambda(engine, oracle_lib)
    win = refine_plain(engine, oracle_lib, rt.full_picture(bd), w, h, bd, sr, None, had, ("corners",) + rt.ONE_CORNER + ("distinct", "outside"), lq,
                       seed=11 + bd, first=ctu, count=1)
    assert tuple(win[ctu]) == (-128, -128, 128, 128)


# ---- picture corners: the block 71 samples outside the picture, the filter support 75-78 samples out, inside the 80-sample margin --------------
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("sr", [16, 64])
def test_picture_corners_and_margins(engine, oracle_lib, bd, sr):
    pred = rt.edge_predictors()
    for ctu, (sx, sy) in zip((0, 2, 3, 5), rt.DIAGONALS):
        lim, got = rt.clip_limits(ctu, W, H), host_window(ctu, W, H, sr, pred)
        ix, iy = (0 if sx < 0 else 2), (1 if sy < 0 else 3)
        assert got[ix] == lim[ix] and got[iy] == lim[iy], (ctu, got, lim)
    lq = set_lambda(engine, oracle_lib)
    for had in (1, 0):
        win = refine_plain(engine, oracle_lib, rt.edge_picture(bd), W, H, bd, sr, pred, had, ("corners", "outside", "mixed"), lq, seed=21 + bd + sr)
    assert all(tuple(win[c]) == host_window(c, W, H, sr, pred) for c in range(6))


# ---- far predictors: the window pinned to the clipMv extreme, the MV cost at its largest -------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("direction", rt.DIAGONALS)
def test_windows_collapsed_by_far_predictors(engine, oracle_lib, bd, direction):
    """predictors 8191 pels away in a diagonal direction.  xSetSearchRange clips the predictor before it spans the window (TEncSearch.cpp:
    3817-3818), so lt == rb cannot happen for a search range >= 1: the window keeps sr + 1 candidates per direction and lies against the
    clipMv limit.  Search range 1 gives the narrowest window a picture-level call can have (2 x 2); the single-candidate window is covered by
    the per-CTU calls below."""
    pred = rt.far_predictors(direction)
    pics = rt.edge_picture(bd, seed=1)
    for sr in rt.COLLAPSED_SR:
        for ctu in range(6):
            lim, got = rt.clip_limits(ctu, W, H), host_window(ctu, W, H, sr, pred)
            assert got[2] - got[0] == sr and got[3] - got[1] == sr
            assert got[0 if direction[0] < 0 else 2] == lim[0 if direction[0] < 0 else 2] and got[1 if direction[1] < 0 else 3] == lim[1 if direction[1] < 0 else 3]
        for lam in (LAMBDA, 0.0, 4000.0):
            lq = set_lambda(engine, oracle_lib, lam)
            for had in (1, 0):
                refine_plain(engine, oracle_lib, pics, W, H, bd, sr, pred, had, ("mixed", "outside"), lq, seed=31 + bd + sr, tag=(direction, lam))


# ---- slivers and tiny pictures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,sr", rt.SLIVERS)
def test_mixed_table_on_tiny_and_sliver_pictures(engine, oracle_lib, w, h, sr):
    from hmme import synth
    cur, ref, _ = synth.make_pair(w, h, seed=w + h, bit_depth=8, max_mv=min(4, sr))
    lq = set_lambda(engine, oracle_lib)
    for had in (1, 0):
        refine_plain(engine, oracle_lib, (cur, ref), w, h, 8, sr, rt.sliver_predictors(w, h), had, ("mixed",), lq, seed=41 + w)


# ---- per-CTU calls -----------------------------------------------------------------------------------------------------------------------------
HALO = 8     # the per-CTU refinement reads 4 samples (+ up to 3 for alignment) beyond the window on every side (include/hmme.h)


def ctu_windows(n=30, seed=1000):
    """the windows, blocks and parameters test_fuzz_search_ctu_vs_oracle builds (tests/test_gpu_parity.py: ragged, one candidate wide, up to
    257 x 257, every bit depth, plain and bi-prediction origins), with the reference plane HALO samples larger on every side"""
    rng = np.random.default_rng(seed)
    for it in range(n):
        bd = int(rng.choice([8, 8, 9, 10, 12]))
        maxv = (1 << bd) - 1
        sr = int(rng.choice([1, 4, 4, 9, 33, 64, 100, 128]))
        lt = (-int(rng.integers(0, sr + 1)), -int(rng.integers(0, sr + 1)))
        rb = (int(rng.integers(0, sr + 1)), int(rng.integers(0, sr + 1)))
        if it % 7 == 0:
            lt, rb = (-sr, -sr), (sr, sr)
        wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
        ref = rng.integers(0, maxv + 1, size=(wy + 63 + 2 * HALO, wx + 63 + 2 * HALO)).astype(np.int16)
        o = (HALO - lt[0], HALO - lt[1])
        dx, dy = int(rng.integers(lt[0], rb[0] + 1)), int(rng.integers(lt[1], rb[1] + 1))
        cur = ref[o[1] + dy:o[1] + dy + 64, o[0] + dx:o[0] + dx + 64].astype(np.int32)
        cur = cur + rng.integers(-3, 4, size=cur.shape)
        bi = it % 3 == 0
        if bi:   # bi-prediction origin: 2 * org - other prediction, unclipped
            other = rng.integers(0, maxv + 1, size=cur.shape)
            cur = np.clip(2 * np.clip(cur, 0, maxv) - other, -maxv, 2 * maxv)
        else:
            cur = np.clip(cur, 0, maxv)
        pred = (int(rng.integers(-500, 501)), int(rng.integers(-500, 501)))
        lam = float(rng.choice([0.0, 4.7, 57.9, 2000.0]))
        yield dict(it=it, bd=bd, sr=sr, lt=lt, rb=rb, ref=ref, o=o, cur=np.ascontiguousarray(cur.astype(np.int16)), pred=pred, lam=lam, bi=bi)


def ctu_tables(c, seed):
    win = np.array([[c["lt"][0], c["lt"][1], c["rb"][0], c["rb"][1]]], np.int64)
    tabs = rt.tables(win, c["sr"], seed)
    return {k: (tabs[k][0], rt.clamp(tabs[k], win)[0]) for k in ("outside", "corners")}


def oracle_ctu(oracle_lib, slot_rects, c, imv, lq, had, wp=None):
    """per-slot frac_refine (frac_refine_w) at the given integer MVs -> (qmv [593, 2], cost [593])"""
    qmv, cost = np.zeros((593, 2), np.int16), np.zeros(593, np.uint32)
    o = c["o"]
    for s in range(593):
        x, y, bw, bh = (int(v) for v in slot_rects[s])
        mv = (int(imv[s, 0]), int(imv[s, 1]))
        if wp is None:
            hx, hy, qx, qy, cst = oracle_lib.frac_refine(c["cur"], (x, y), c["ref"], (o[0] + x, o[1] + y), bw, bh, mv, c["pred"], lq, had, c["bd"])
        else:
            hx, hy, qx, qy, cst = oracle_lib.frac_refine_w(c["cur"], (x, y), c["ref"], (o[0] + x, o[1] + y), bw, bh, mv, c["pred"], lq, had, c["bd"], wp)
        qmv[s] = (4 * mv[0] + 2 * hx + qx, 4 * mv[1] + 2 * hy + qy)
        cost[s] = cst
    return qmv, cost


@pytest.mark.parametrize("part", range(5))
def test_refine_ctu_outside_and_corner_tables(engine, oracle_lib, slot_rects, part):
    """hmme_refine_ctu on the windows of test_fuzz_search_ctu_vs_oracle, six windows per case: `outside` with one metric, `corners` with the
    other"""
    from hmme import api
    cases = [c for c in ctu_windows() if c["it"] // 6 == part]
    assert len(cases) == 6
    for c in cases:
        lq = set_lambda(engine, oracle_lib, c["lam"])
        p = api.SearchParams(c["lt"][0], c["lt"][1], c["rb"][0], c["rb"][1], c["pred"][0], c["pred"][1], 1, c["bd"])
        for k, (name, (t, tc)) in enumerate(ctu_tables(c, 51 + c["it"]).items()):
            had = (c["it"] + k) % 2
            qmv, cost = engine.refine_ctu(c["cur"], (0, 0), c["ref"], c["o"], p, t, use_hadamard=bool(had))
            oq, oc = oracle_ctu(oracle_lib, slot_rects, c, tc, lq, had)
            same((name, had, c["it"], c["bd"], c["lt"], c["rb"], c["bi"]), qmv, cost, oq, oc)


def test_refine_ctu_single_candidate_window(engine, oracle_lib, slot_rects):
    """lt == rb: every entry of every table is clamped to the one candidate (a picture-level call cannot have such a window)"""
    from hmme import api
    for it, bd_had in ((5, 1), (19, 0)):
        c = next(c for c in ctu_windows() if c["it"] == it)
        c = dict(c, rb=c["lt"])
        lq = set_lambda(engine, oracle_lib, 57.9)
        p = api.SearchParams(c["lt"][0], c["lt"][1], c["rb"][0], c["rb"][1], c["pred"][0], c["pred"][1], 1, c["bd"])
        for name, (t, tc) in ctu_tables(c, 55 + it).items():
            assert (tc == np.array(c["lt"])).all() and (name == "corners" or (t != tc).any())
            qmv, cost = engine.refine_ctu(c["cur"], (0, 0), c["ref"], c["o"], p, t, use_hadamard=bool(bd_had))
            oq, oc = oracle_ctu(oracle_lib, slot_rects, c, tc, lq, bd_had)
            same((name, it, c["bd"], c["lt"]), qmv, cost, oq, oc)


def test_ctu_windows_are_what_the_per_ctu_cases_are_for():
    cs = list(ctu_windows())
    sizes = [(c["rb"][0] - c["lt"][0] + 1, c["rb"][1] - c["lt"][1] + 1) for c in cs]
    assert {c["bd"] for c in cs} == {8, 9, 10, 12} and {c["bi"] for c in cs} == {True, False}
    assert (257, 257) in sizes and any(1 in s for s in sizes) and any(a != b for a, b in sizes)


@pytest.mark.parametrize("bd,family,it", [(8, "negative_offset", 4), (10, "inverting", 11)])
def test_refine_ctu_w_outside_and_corner_tables(engine, oracle_lib, slot_rects, bd, family, it):
    """hmme_refine_ctu_w with a weight the library serves: the accepted weight nearest to a refusal (tests/range_content.py)"""
    from hmme import api
    wp = rc.boundary_weight(bd, True, family)
    assert api.weight_check(bd, wp, True) == 0
    c = next(c for c in ctu_windows() if c["it"] == it)
    assert not c["bi"]
    maxv = (1 << bd) - 1
    c = dict(c, bd=bd, ref=(c["ref"].astype(np.int32) * maxv // ((1 << c["bd"]) - 1)).astype(np.int16))
    # the current block: the weighted reference at the planted displacement (what the weighted refinement should find), in range
    c["cur"] = np.ascontiguousarray(np.clip(rc.weigh(c["ref"][c["o"][1]:c["o"][1] + 64, c["o"][0]:c["o"][0] + 64], wp), 0, maxv).astype(np.int16))
    lq = set_lambda(engine, oracle_lib)
    p = api.SearchParams(c["lt"][0], c["lt"][1], c["rb"][0], c["rb"][1], c["pred"][0], c["pred"][1], 1, bd)
    for k, (name, (t, tc)) in enumerate(ctu_tables(c, 61 + bd).items()):
        qmv, cost = engine.refine_ctu_w(c["cur"], (0, 0), c["ref"], c["o"], p, wp, t, use_hadamard=bool(k))
        oq, oc = oracle_ctu(oracle_lib, slot_rects, c, tc, lq, k, wp=wp)
        same((name, bd, wp, c["lt"], c["rb"]), qmv, cost, oq, oc)


# ---- the other families, one launch each, on 136 x 72 with `mixed` -----------------------------------------------------------------------------
def oracle_refine_w(oracle_lib, slot_rects, cur, cur_origin, ref, int_mv, pred, lq, had, bd, wp, ctus):
    """hmo_frac_refine_w per slot; cur_origin: where sample (0, 0) of the picture lies in `cur` (the margin for a padded plane, 0 for an
    origin picture); int_mv [len(ctus), 593, 2]"""
    from hmme import synth
    m = synth.MARGIN
    cx_n = (W + 63) // 64
    qmv, cost = np.zeros((len(ctus), 593, 2), np.int16), np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        cx, cy = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        pq = (int(pred[ctu, 0]), int(pred[ctu, 1]))
        for s in range(593):
            x, y, bw, bh = (int(v) for v in slot_rects[s])
            mv = (int(int_mv[k, s, 0]), int(int_mv[k, s, 1]))
            hx, hy, qx, qy, c = oracle_lib.frac_refine_w(cur, (cur_origin + cx + x, cur_origin + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, mv, pq,
                                                         lq, had, bd, wp)
            qmv[k, s] = (4 * mv[0] + 2 * hx + qx, 4 * mv[1] + 2 * hy + qy)
            cost[k, s] = c
    return qmv, cost


def fetch(d_q, d_c):
    return d_q.cpu().numpy(), d_c.cpu().numpy().astype(np.uint32)


@pytest.mark.parametrize("bd", [8, 10])
def test_weighted_pairs_launch_with_mixed_tables(engine, oracle_lib, slot_rects, bd):
    """refine_pairs_w_device, weights [A, A, B], CTUs 4 and 5 of every pair (the partial bottom row, the corner): six refined CTUs"""
    import torch
    from hmme import api, synth
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    sr, first, count, had = rt.FAMILY_SR, 4, 2, bd == 8
    a, b = (40, 12 << (bd - 8), 6, 32), (-30, 180 << (bd - 8), 5, 16)
    wps = [a, a, b]
    assert all(api.weight_check(bd, wp, True) == 0 for wp in wps)
    pics = []
    for i, wp in enumerate(wps):   # ref a texture, cur its moved copy seen through the weight (weighting commutes with the edge replication)
        cur, ref, _ = synth.make_pair(W, H, seed=7100 + i + bd, bit_depth=bd, max_mv=5, region=64)
        pics.append((np.ascontiguousarray(np.clip(rc.weigh(cur, wp), 0, (1 << bd) - 1).astype(np.int16)), ref))
    pred = np.stack([rt.family_predictors()[0], rt.family_predictors()[1], rt.edge_predictors()])
    wins = [rt.oracle_windows(W, H, sr, pred[i]) for i in range(3)]
    tabs = [rt.tables(wins[i], sr, 71 + i)["mixed"] for i in range(3)]
    lq = set_lambda(engine, oracle_lib)
    pl = [(mkplane(engine, c, W, H, bd), mkplane(engine, r, W, H, bd)) for c, r in pics]
    try:
        d_pred = torch.from_numpy(pred).to(dev)
        d_imv = torch.from_numpy(np.stack([t[first:first + count] for t in tabs])).to(dev)
        d_q, d_c = device_tables(3, count, dev)
        engine.refine_pairs_w_device([p[0] for p in pl], [p[1] for p in pl], api.FrameParams(sr, 0, bd, first, count), wps, d_pred.data_ptr(), d_imv.data_ptr(),
                                     int(had), d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        qmv, cost = fetch(d_q, d_c)
    finally:
        for p in pl:
            p[0].close(); p[1].close()
    for i in range(3):
        tc = rt.clamp(tabs[i], wins[i])[first:first + count]
        oq, oc = oracle_refine_w(oracle_lib, slot_rects, pics[i][0], m, pics[i][1], tc, pred[i], lq, int(had), bd, wps[i], range(first, first + count))
        same(("pair", i, bd), qmv[i], cost[i], oq, oc)


def bi_inputs(bd, seed):
    pred, center = rt.family_predictors()
    sr = rt.FAMILY_SR
    w_pred, w_center = rt.oracle_windows(W, H, sr, pred), rt.oracle_windows(W, H, sr, center)
    assert not np.array_equal(w_pred, w_center) and all(tuple(w_center[c]) == host_window(c, W, H, sr, center) for c in range(6))
    table = rt.tables(w_center, sr, seed)["mixed"]
    # the clamp is to the window around the CENTRE: clamped to the predictor's window the table would be another one
    assert not np.array_equal(rt.clamp(table, w_center), rt.clamp(table, w_pred))
    return pred, center, w_center, table, random_field(6, 64, seed + 1), three_planes(W, H, bd, seed + 2)


@pytest.mark.parametrize("bd", [8, 10])
def test_bi_pairs_launch_with_mixed_table_clamped_to_the_centre_window(engine, oracle_lib, hmo, bd):
    import torch
    from hmme import api, synth
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    had = int(bd == 10)
    pred, center, win, table, field, (cur, ref, other) = bi_inputs(bd, 8100 + bd)
    lq = set_lambda(engine, oracle_lib)
    pc, pr, po = (mkplane(engine, a, W, H, bd) for a in (cur, ref, other))
    try:
        d_f, d_pred, d_center, d_imv = (torch.from_numpy(np.ascontiguousarray(a[None])).to(dev) for a in (field, pred, center, table))
        d_q, d_c = device_tables(1, 6, dev)
        engine.refine_pairs_bi_device([pc], [pr], [po], api.FrameParams(rt.FAMILY_SR, 1, bd, 0, 6), d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(),
                                      d_imv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        qmv, cost = fetch(d_q, d_c)
    finally:
        pc.close(); pr.close(); po.close()
    org = origin_picture(cur, oracle_prediction(hmo, other, W, H, bd, field), W, H)
    org_padded = np.ascontiguousarray(np.pad(org, m))
    oq, oc = oracle_lib.refine_frame(org_padded, ref, (m, m), W, H, rt.clamp(table, win), pred, lq, had, bd, n_threads=8)
    same(("bi", bd), qmv[0], cost[0], oq, oc)


@pytest.mark.parametrize("bd", [8, 10])
def test_weighted_bi_pairs_launch_with_mixed_table(engine, oracle_lib, hmo, slot_rects, bd):
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    had = int(bd == 8)
    wp, owp = (40, -12 << (bd - 8), 5, 16), (-20, 200 << (bd - 8), 5, 16)
    assert api.bipred_weight_check(bd, wp, owp, 1) == 0
    pred, center, win, table, field, (cur, ref, other) = bi_inputs(bd, 9100 + bd)
    lq = set_lambda(engine, oracle_lib)
    pc, pr, po = (mkplane(engine, a, W, H, bd) for a in (cur, ref, other))
    try:
        d_f, d_pred, d_center, d_imv = (torch.from_numpy(np.ascontiguousarray(a[None])).to(dev) for a in (field, pred, center, table))
        d_q, d_c = device_tables(1, 6, dev)
        engine.refine_pairs_bi_w_device([pc], [pr], [po], api.FrameParams(rt.FAMILY_SR, 0, bd, 0, 6), [wp], [owp], d_f.data_ptr(), 64, d_center.data_ptr(),
                                        d_pred.data_ptr(), d_imv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        qmv, cost = fetch(d_q, d_c)
    finally:
        pc.close(); pr.close(); po.close()
    org = model.origin(cur, model.pred_picture(hmo, other, W, H, bd, field, owp), W, H)
    oq, oc = oracle_refine_w(oracle_lib, slot_rects, org, 0, ref, rt.clamp(table, win), pred, lq, had, bd, wp, range(6))
    same(("bi_w", bd), qmv[0], cost[0], oq, oc)


# ---- three pairs, a table kind each, a CTU sub-range --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_three_pairs_three_table_kinds_and_a_ctu_sub_range(engine, oracle_lib, bd):
    """refine_pairs_device, ctu_first = 2, ctu_count = 3 == the three single-pair calls == the oracle"""
    import torch
    from hmme import api, synth
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    sr, first, count, had = 16, 2, 3, 1
    kinds = ("corners", "distinct", "outside")
    pics = [rt.edge_picture(bd, seed=10 + i) for i in range(3)]
    pred = rt.multi_pair_predictors()
    wins = [rt.oracle_windows(W, H, sr, pred[i]) for i in range(3)]
    tabs = [rt.tables(wins[i], sr, 91 + i)[kinds[i]] for i in range(3)]
    lq = set_lambda(engine, oracle_lib)
    pl = [(mkplane(engine, c, W, H, bd), mkplane(engine, r, W, H, bd)) for c, r in pics]
    try:
        d_pred = torch.from_numpy(pred).to(dev)
        d_imv = torch.from_numpy(np.stack([t[first:first + count] for t in tabs])).to(dev)
        d_q, d_c = device_tables(3, count, dev)
        engine.refine_pairs_device([p[0] for p in pl], [p[1] for p in pl], api.FrameParams(sr, 1, bd, first, count), d_pred.data_ptr(), d_imv.data_ptr(), had,
                                   d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        qmv, cost = fetch(d_q, d_c)
        for i in range(3):
            sq, sc = engine.refine_frame(pl[i][0], pl[i][1], sr, tabs[i][first:first + count], pred[i], use_hadamard=True, ctu_first=first, ctu_count=count)
            same(("single", kinds[i], bd), qmv[i], cost[i], sq, sc)
    finally:
        for p in pl:
            p[0].close(); p[1].close()
    for i in range(3):
        oq, oc = oracle_lib.refine_frame(pics[i][0], pics[i][1], (m, m), W, H, rt.clamp(tabs[i], wins[i])[first:first + count], pred[i], lq, had, bd,
                                         first, count, n_threads=8)
        same(("oracle", kinds[i], bd), qmv[i], cost[i], oq, oc)
