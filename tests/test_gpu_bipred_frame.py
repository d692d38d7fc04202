"""Motion compensation and the bi-prediction pass on whole pictures and picture pairs (hmme_predict_*, hmme_search_pairs_bi_device,
hmme_refine_pairs_bi_device, hmme_search_frame_bi, hmme_refine_frame_bi) against the CPU oracle: hmo_pred_block_qpel for the prediction,
hmo_search_ctu on the origin 2 * cur - prediction built in numpy for the search (both legs live in tests/frame_helpers.py, shared with
test_gpu_range_edges.py), hmo_frac_refine per slot for the refinement.  Every comparison is bit-exact.
Pictures are sized so that no case needs more than about a minute of oracle time."""
import numpy as np
import pytest

from frame_helpers import (bind_hmo, check_strided_image, dims, mkplane, oracle_bi_search, oracle_prediction, origin_picture, random_field, run_bi_search,
                           three_planes)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    e.set_lambda(57.9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


# ---- 1: the prediction against hmo_pred_block_qpel -----------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("per", [1, 64])
def test_prediction_equals_the_oracle_at_every_phase(engine, hmo, bd, per):
    from hmme import synth
    w, h = 296, 200                     # 5 x 4 CTUs, partial on the right, at the bottom and in the corner
    cx_n, cy_n = dims(w, h)
    n_ctu = cx_n * cy_n
    _, ref, _ = synth.make_pair(w, h, seed=11 + bd, bit_depth=bd, max_mv=4, region=64)
    rng = np.random.default_rng(5 + bd + per)
    field = np.zeros((n_ctu, per, 2), np.int16)
    # MVs beyond what clipMv allows at the CTU: every direction, and values at the ends of int16
    beyond = {0: (-3000, -2999), 4: (3001, -1203), 12: (-32768, 32767), 19: (32767, 32766)}
    inside = [c for c in range(n_ctu) if c not in beyond]
    for k, ctu in enumerate(inside):
        for b in range(per):
            ph = (k if per == 1 else b + ctu) % 16             # all 16 fractional phases: full-pel, single-stage and two-stage cases
            field[ctu, b] = (4 * int(rng.integers(-9, 10)) + (ph & 3), 4 * int(rng.integers(-9, 10)) + (ph >> 2))
    for ctu, mv in beyond.items():
        field[ctu, :] = mv
    assert len({(int(x) & 3, int(y) & 3) for c in inside for x, y in field[c]}) == 16
    want = oracle_prediction(hmo, ref, w, h, bd, field)[:h, :w]
    pr = mkplane(engine, ref, w, h, bd)
    try:
        got = engine.predict_frame(pr, field if per == 64 else field[:, 0])
        assert got.dtype == (np.uint8 if bd == 8 else np.uint16)
        assert np.array_equal(got.astype(np.int16), want), np.argwhere(got.astype(np.int16) != want)[:4]
        # a CTU sub-range into an image full of a sentinel: its samples are written, nothing else is touched
        sentinel = 0xA5 if bd == 8 else 0xA5A5
        first, count = 3, 9
        img = np.full((h, w), sentinel, got.dtype)
        engine.predict_frame(pr, field, out=img, ctu_first=first, ctu_count=count)
        inside = np.zeros((h, w), bool)
        for ctu in range(first, first + count):
            x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
            inside[y:y + 64, x:x + 64] = True
        assert np.array_equal(img[inside].astype(np.int16), want[inside])
        assert np.all(img[~inside] == sentinel)
    finally:
        pr.close()
    # ... and into an image whose stride exceeds the width, on 3 x 2 CTUs
    import ctypes as C
    sw, sh = 136, 72
    _, sref, _ = synth.make_pair(sw, sh, seed=13 + bd, bit_depth=bd, max_mv=4, region=64)
    sfield = random_field(6, per, 9 + bd + per)
    ps = mkplane(engine, sref, sw, sh, bd)
    try:
        check_strided_image(sw, sh, bd, lambda out, first, count: engine.predict_frame(ps, sfield, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_frame(engine.h, ps.h, C.byref(fp), sfield.ctypes.data, per, out, stride))
    finally:
        ps.close()


# ---- 2: the bi search against the oracle, all 593 slots of every CTU -----------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("fen", [0, 1])
@pytest.mark.parametrize("w,h", [(296, 200), (168, 136)])
@pytest.mark.parametrize("sr", [4, 12])
def test_bi_search_equals_the_oracle(engine, oracle_lib, hmo, bd, fen, w, h, sr):
    per = 64 if (sr + fen + bd // 2) % 2 else 1
    run_bi_search(engine, oracle_lib, hmo, w, h, bd, sr, fen, per, seed=500 + 7 * sr + 3 * fen + bd + w)


@pytest.mark.parametrize("bd", [8, 10])
def test_bi_search_with_a_null_centre_is_centred_on_the_predictor(engine, oracle_lib, hmo, bd):
    run_bi_search(engine, oracle_lib, hmo, 168, 136, bd, 12, 1, 64, seed=700 + bd, with_center=False)


@pytest.mark.parametrize("bd", [8, 10])
def test_bi_search_on_an_origin_that_reaches_both_extremes(engine, oracle_lib, hmo, bd):
    """a black current CTU against a white other picture (origin -maxv) and the reverse (origin 2 * maxv)"""
    from hmme import synth
    w, h, m, maxv = 168, 136, synth.MARGIN, (1 << bd) - 1
    cur, ref, other = three_planes(w, h, bd, seed=820 + bd)
    cur, other = cur[m:m + h, m:m + w].copy(), other[m:m + h, m:m + w].copy()
    cur[0:64, 0:64], other[0:64, 0:64] = 0, maxv
    cur[0:64, 64:128], other[0:64, 64:128] = maxv, 0
    other[0:80, 0:150] = np.where(np.arange(150)[None, :] < 64, maxv, 0)   # flat around the two CTUs: the 8-tap filter sees one value
    cur, other = synth.pad_plane(cur), synth.pad_plane(other)
    r = run_bi_search(engine, oracle_lib, hmo, w, h, bd, 4, 1, 1, seed=830 + bd, planes3=(cur, ref, other))
    # (the random field moves the prediction by a few samples: the flat areas are wide enough for most of both CTUs)
    assert r["org"].min() == -maxv and r["org"].max() == 2 * maxv


# ---- 3: the bi refinement against hmo_frac_refine, per slot --------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("had", [1, 0])
def test_bi_refinement_equals_the_oracle(engine, oracle_lib, hmo, bd, had):
    from hmme import synth
    w, h, sr, m = 168, 136, 4, synth.MARGIN
    r = run_bi_search(engine, oracle_lib, hmo, w, h, bd, sr, 1, 64 if had else 1, seed=900 + bd + had)
    pc, pr, po = (mkplane(engine, r[k], w, h, bd) for k in ("cur", "ref", "other"))
    try:
        qmv, cost = engine.refine_frame_bi(pc, pr, po, sr, r["field"], r["mv"], center_q=r["center"], pred_q=r["pred"], use_hadamard=bool(had))
    finally:
        pc.close(); pr.close(); po.close()
    org_padded = np.ascontiguousarray(np.pad(r["org"], m))   # the oracle's frame refinement takes both planes at one origin
    oqmv, ocost = oracle_lib.refine_frame(org_padded, r["ref"], (m, m), w, h, r["mv"], r["pred"], engine.lambda_q16, had, bd, n_threads=8)
    assert np.array_equal(qmv, oqmv), (bd, had, np.argwhere(qmv != oqmv)[:4])
    assert np.array_equal(cost, ocost), (bd, had, np.argwhere(cost != ocost)[:4])


# ---- 4: launch shapes ------------------------------------------------------------------------------------------------------------
def _tables(n_pairs, count, dev):
    import torch
    return (torch.zeros((n_pairs, count, 593, 2), dtype=torch.int16, device=dev), torch.zeros((n_pairs, count, 593), dtype=torch.int32, device=dev))


@pytest.mark.parametrize("bd", [8, 10])
def test_three_pairs_in_one_launch_sub_ranges_and_two_streams(engine, bd):
    import torch
    from hmme import api, synth
    w, h, sr = 232, 170, 4
    n_ctu = 4 * 3
    dev = torch.device("cuda", 0)
    cur, r0, r1 = three_planes(w, h, bd, seed=1100 + bd)
    cur2, r2, o2 = three_planes(w, h, bd, seed=1200 + bd)
    planes = [mkplane(engine, a, w, h, bd) for a in (cur, r0, r1, cur2, r2, o2)]
    pc, p0, p1, pc2, p2, po2 = planes
    try:
        # pairs 0 and 1: the two directions of one B picture, one MV per CTU (written out 64 times for the common launch); pair 2: a
        # field that differs from 8x8 block to 8x8 block
        f1 = [random_field(n_ctu, 1, 1300 + i + bd) for i in range(2)]
        f64 = np.stack([np.repeat(f1[0], 64, axis=1), np.repeat(f1[1], 64, axis=1), random_field(n_ctu, 64, 1310 + bd)])
        pred = np.stack([synth.random_predictors(n_ctu, seed=1320 + i, max_pel=6) for i in range(3)])
        center = np.stack([synth.random_predictors(n_ctu, seed=1330 + i, max_pel=6) for i in range(3)])
        curs, refs, others = [pc, pc, pc2], [p0, p1, p2], [p1, p0, po2]
        d_f, d_pred, d_center = (torch.from_numpy(a).to(dev) for a in (f64, pred, center))
        full = {}
        for first, count in ((0, n_ctu), (5, 6)):
            fp = api.FrameParams(sr, 1, bd, first, count)
            d_mv, d_sad = _tables(3, count, dev)
            engine.search_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
            d_q, d_c = _tables(3, count, dev)
            engine.refine_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), 1,
                                          d_q.data_ptr(), d_c.data_ptr(), 0)
            torch.cuda.synchronize()
            mv, sad, qmv, cost = (t.cpu().numpy() for t in (d_mv, d_sad, d_q, d_c))
            if first == 0:
                full = dict(mv=mv, sad=sad, qmv=qmv, cost=cost)
            else:   # a CTU sub-range == the same rows of the full call
                for k, a in (("mv", mv), ("sad", sad), ("qmv", qmv), ("cost", cost)):
                    assert np.array_equal(a, full[k][:, first:first + count]), k
            for i in range(3):   # == the three single calls (pairs 0 and 1 with their one-MV-per-CTU fields)
                field = f1[i] if i < 2 else f64[2]
                smv, ssad = engine.search_frame_bi(curs[i], refs[i], others[i], sr, field, center_q=center[i], pred_q=pred[i], fen=1, ctu_first=first, ctu_count=count)
                assert np.array_equal(mv[i], smv) and np.array_equal(sad[i].astype(np.uint32), ssad), (first, i)
                sq, sc = engine.refine_frame_bi(curs[i], refs[i], others[i], sr, field, smv, center_q=center[i], pred_q=pred[i], ctu_first=first, ctu_count=count)
                assert np.array_equal(qmv[i], sq) and np.array_equal(cost[i].astype(np.uint32), sc), (first, i)
        # a search on one stream, a refinement on another, a second search on the first: no host synchronisation in between, the scratch
        # they share is ordered by the library
        fp = api.FrameParams(sr, 1, bd, 0, n_ctu)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        d_imv = torch.from_numpy(full["mv"]).to(dev)
        a_mv, a_sad = _tables(3, n_ctu, dev)
        b_q, b_c = _tables(3, n_ctu, dev)
        c_mv, c_sad = _tables(1, n_ctu, dev)
        torch.cuda.synchronize()
        engine.search_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), a_mv.data_ptr(), a_sad.data_ptr(), s1.cuda_stream)
        engine.refine_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_imv.data_ptr(), 1,
                                      b_q.data_ptr(), b_c.data_ptr(), s2.cuda_stream)
        engine.search_pairs_bi_device(curs[2:], refs[2:], others[2:], fp, d_f[2:].data_ptr(), 64, d_center[2:].data_ptr(), d_pred[2:].data_ptr(),
                                      c_mv.data_ptr(), c_sad.data_ptr(), s1.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(a_mv.cpu().numpy(), full["mv"]) and np.array_equal(a_sad.cpu().numpy(), full["sad"])
        assert np.array_equal(b_q.cpu().numpy(), full["qmv"]) and np.array_equal(b_c.cpu().numpy(), full["cost"])
        assert np.array_equal(c_mv.cpu().numpy()[0], full["mv"][2]) and np.array_equal(c_sad.cpu().numpy()[0], full["sad"][2])
        # two pictures predicted in one launch == one at a time
        dt, tdt = (np.uint8, torch.uint8) if bd == 8 else (np.uint16, torch.int16)
        imgs = [torch.zeros((h, w), dtype=tdt, device=dev) for _ in range(2)]
        engine.predict_pairs_device([p1, po2], fp, d_f[1:].data_ptr(), 64, [t.data_ptr() for t in imgs], w * (1 if bd == 8 else 2), 0)
        torch.cuda.synchronize()
        for t, pl, f in zip(imgs, (p1, po2), (f64[1], f64[2])):
            assert np.array_equal(t.cpu().numpy().view(dt), engine.predict_frame(pl, f))
    finally:
        for p in planes:
            p.close()


# ---- 5: a real launch size ---------------------------------------------------------------------------------------------------
def test_1080p_bi_search_against_the_oracle_and_the_per_ctu_call(engine, oracle_lib, hmo):
    from hmme import api, synth
    w, h, sr, bd, m = 1920, 1080, 4, 8, synth.MARGIN
    cx_n, cy_n = dims(w, h)           # 30 x 17, the bottom row partial
    n_ctu = cx_n * cy_n
    cur, ref, other = three_planes(w, h, bd, seed=1500, max_mv=6)
    field = random_field(n_ctu, 64, 1501)
    pred = synth.random_predictors(n_ctu, seed=1502, max_pel=8)
    center = synth.random_predictors(n_ctu, seed=1503, max_pel=8)
    org = origin_picture(cur, oracle_prediction(hmo, other, w, h, bd, field), w, h)
    pc, pr, po = (mkplane(engine, a, w, h, bd) for a in (cur, ref, other))
    try:
        mv, sad = engine.search_frame_bi(pc, pr, po, sr, field, center_q=center, pred_q=pred, fen=1)
    finally:
        pc.close(); pr.close(); po.close()
    last = n_ctu - cx_n
    ctus = [0, cx_n - 1, last, n_ctu - 1,                                    # the four corners
            7, 19, last + 5, last + 22,                                      # top and bottom edge
            3 * cx_n, 11 * cx_n, 5 * cx_n - 1, 14 * cx_n - 1,                # left and right edge
            cx_n + 1, 4 * cx_n + 9, 8 * cx_n + 15, 9 * cx_n + 3, 12 * cx_n + 27, 15 * cx_n + 28]
    omv, osad = oracle_bi_search(oracle_lib, org, ref, w, h, sr, center, pred, engine.lambda_q16, 1, bd, ctus)
    assert np.array_equal(mv[ctus], omv) and np.array_equal(sad[ctus], osad)
    # every CTU against the per-CTU call on the same origin (pinned to the reference by test_bipred_origins_outside_the_sample_range)
    for ctu in range(n_ctu):
        x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        lt_x, lt_y, rb_x, rb_y = api.set_search_range(int(center[ctu, 0]), int(center[ctu, 1]), sr, x, y, w, h)
        p = api.SearchParams(lt_x, lt_y, rb_x, rb_y, int(pred[ctu, 0]), int(pred[ctu, 1]), 1, bd)
        cmv, csad = engine.search_ctu(org, (x, y), ref, (m + x, m + y), p)
        assert np.array_equal(mv[ctu], cmv) and np.array_equal(sad[ctu], csad), ctu


# ---- 6: what it is for -----------------------------------------------------------------------------------------------------------
def test_bi_cost_is_below_both_uni_costs_on_an_averaged_picture(engine):
    """cur = the rounded average of two differently displaced textures: after the uni-directional searches and refinements on both lists and
    the bi pass in both directions, the 64x64 slot's bi cost is below both uni-directional costs in every interior CTU"""
    from hmme import synth
    w, h, bd, m = 320, 256, 8, synth.MARGIN
    cx_n, cy_n = dims(w, h)
    n_ctu = cx_n * cy_n
    _, ta, _ = synth.make_pair(w, h, seed=1601, max_mv=0)
    _, tb, _ = synth.make_pair(w, h, seed=1602, max_mv=0)
    (ax, ay), (bx, by) = (3, -2), (-4, 1)
    a = np.roll(ta, (-ay, -ax), axis=(0, 1)).astype(np.int32)      # a[y, x] = ta[y + ay, x + ax]
    b = np.roll(tb, (-by, -bx), axis=(0, 1)).astype(np.int32)
    cur = synth.pad_plane(((a + b + 1) >> 1)[m:m + h, m:m + w])
    pc, pa, pb = (mkplane(engine, p, w, h, bd) for p in (cur, ta, tb))
    try:
        uni = []
        for ref in (pa, pb):
            mv, _ = engine.search_frame(pc, ref, 8, None, fen=1)
            uni.append(engine.refine_frame(pc, ref, 8, mv))
        bi = []
        for ref, other, (q_ref, _), (q_other, _) in ((pa, pb, uni[0], uni[1]), (pb, pa, uni[1], uni[0])):
            field = q_other[:, 592]                                  # the other list's 64x64 MV
            centre = q_ref[:, 592]
            mv, _ = engine.search_frame_bi(pc, ref, other, 4, field, center_q=centre, fen=1)
            bi.append(engine.refine_frame_bi(pc, ref, other, 4, field, mv, center_q=centre))
    finally:
        pc.close(); pa.close(); pb.close()
    interior = [cy * cx_n + cx for cy in range(1, cy_n - 1) for cx in range(1, cx_n - 1)]
    assert len(interior) == 6
    for d in range(2):
        for ctu in interior:
            c = int(bi[d][1][ctu, 592])
            assert c < int(uni[0][1][ctu, 592]) and c < int(uni[1][1][ctu, 592]), (d, ctu, c, int(uni[0][1][ctu, 592]), int(uni[1][1][ctu, 592]))


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(engine):
    import torch
    from hmme import api, synth
    w, h, sr = 168, 136, 4
    n_ctu = 9
    dev = torch.device("cuda", 0)
    d_f = torch.zeros((16, n_ctu, 1, 2), dtype=torch.int16, device=dev)
    d_imv = torch.zeros((16, n_ctu, 593, 2), dtype=torch.int16, device=dev)

    def sentinels():
        return (torch.full((16, n_ctu, 593, 2), 0x5A5A, dtype=torch.int16, device=dev), torch.full((16, n_ctu, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev))

    def untouched(t_mv, t_c):
        torch.cuda.synchronize()
        return bool((t_mv == 0x5A5A).all()) and bool((t_c == 0x5A5A5A5A).all())

    # a pair that fails hmme_bipred_check: the refinement at 12 bits
    assert api.bipred_check(12, True) != 0 and api.bipred_check(12, False) == 0
    cur, ref, other = three_planes(w, h, 12, seed=1700)
    p12 = [mkplane(engine, a, w, h, 12) for a in (cur, ref, other)]
    cur8, ref8, other8 = three_planes(w, h, 8, seed=1701)
    p8 = [mkplane(engine, a, w, h, 8) for a in (cur8, ref8, other8)]
    small = mkplane(engine, three_planes(104, 72, 8, seed=1702)[2], 104, 72, 8)
    eng2 = api.Engine(0, 64)
    foreign = mkplane(eng2, other8, w, h, 8)
    try:
        t_q, t_c = sentinels()
        fp12 = api.FrameParams(sr, 1, 12, 0, n_ctu)
        with pytest.raises(api.HmmeError):
            engine.refine_pairs_bi_device([p12[0]], [p12[1]], [p12[2]], fp12, d_f.data_ptr(), 1, None, None, d_imv.data_ptr(), 1, t_q.data_ptr(), t_c.data_ptr(), 0)
        assert untouched(t_q, t_c)
        with pytest.raises(api.HmmeError):
            engine.refine_frame_bi(p12[0], p12[1], p12[2], sr, np.zeros((n_ctu, 2), np.int16), np.zeros((n_ctu, 593, 2), np.int16))
        fp = api.FrameParams(sr, 1, 8, 0, n_ctu)
        for others, n in (([foreign], 1),                # a plane of another context
                          ([small], 1),                  # an `others` plane of a different size
                          ([p8[2]] * 17, 17)):           # more than 16 pairs
            t_mv, t_sad = sentinels()
            with pytest.raises(api.HmmeError):
                engine.search_pairs_bi_device([p8[0]] * n, [p8[1]] * n, others, fp, d_f.data_ptr(), 1, None, None, t_mv.data_ptr(), t_sad.data_ptr(), 0)
            with pytest.raises(api.HmmeError):
                engine.refine_pairs_bi_device([p8[0]] * n, [p8[1]] * n, others, fp, d_f.data_ptr(), 1, None, None, d_imv.data_ptr(), 1, t_mv.data_ptr(), t_sad.data_ptr(), 0)
            assert untouched(t_mv, t_sad)
        # a field of neither 1 nor 64 MVs per CTU
        t_mv, t_sad = sentinels()
        with pytest.raises(api.HmmeError):
            engine.search_pairs_bi_device([p8[0]], [p8[1]], [p8[2]], fp, d_f.data_ptr(), 4, None, None, t_mv.data_ptr(), t_sad.data_ptr(), 0)
        assert untouched(t_mv, t_sad)
        # ... and the call that is served still is
        engine.search_pairs_bi_device([p8[0]], [p8[1]], [p8[2]], fp, d_f.data_ptr(), 1, None, None, t_mv.data_ptr(), t_sad.data_ptr(), 0)
        torch.cuda.synchronize()
        assert not bool((t_sad[0] == 0x5A5A5A5A).any())
    finally:
        for p in p12 + p8 + [small]:
            p.close()
        foreign.close(); eng2.close()
