"""GPU parity tests (run with -m gpu on the MI355X box): the HIP engine, called through the C ABI,
against (a) the golden vectors generated from the compiled reference and (b) the CPU oracle on the
same seeded inputs.  Bit-exact: MVs and SADs are integers."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


def _golden_cases(fname):
    d = np.load(os.path.join(GOLDEN, fname))
    for i in range(len(d["cur"])):
        m = dict(zip(d["meta_columns"].tolist(), (int(v) for v in d["meta"][i])))
        yield i, m, d["cur"][i], d["ref"][i], d["out"][i]


@pytest.mark.parametrize("fname", ["search_sr8.npz", "search_sr64.npz"])
def test_search_ctu_matches_reference_goldens(engine, fname):
    """hmme_search_ctu == TEncSearch::xPatternSearch on all 593 PU rectangles (goldens from the compiled reference)"""
    from hmme import api
    n = 0
    for i, m, cur, ref, want in _golden_cases(fname):
        engine.set_lambda_q16(m["lambda_q16"])   # 8-bit cases run the packed-byte kernel, 10-bit ones the 16-bit kernel
        p = api.SearchParams(m["lt_x"], m["lt_y"], m["rb_x"], m["rb_y"], m["pred_x"], m["pred_y"], m["fen"], m["bit_depth"])
        mv, sad = engine.search_ctu(cur, (0, 0), ref, (m["origin_x"], m["origin_y"]), p)
        assert np.array_equal(mv.astype(np.int64), want[:, :2]), f"{fname} case {i}: MV mismatch"
        assert np.array_equal(sad.astype(np.int64), want[:, 2]), f"{fname} case {i}: SAD mismatch"
        n += 1
    assert n >= 2


def test_search_ctu_random_windows_vs_oracle(engine, oracle_lib):
    """ragged / clipped windows, all parameter mixes, against the oracle"""
    from hmme import api
    rng = np.random.default_rng(77)
    for it in range(24):
        sr = int(rng.choice([1, 5, 8, 21, 40, 64]))
        side = 64 + 2 * sr + 8
        kind = it % 4
        if kind == 3:   # motion-like content: ref = shifted cur + noise
            base = rng.integers(0, 256, size=(side + 16, side + 16))
            ref = base[8:8 + side, 8:8 + side].astype(np.int16)
            dx, dy = int(rng.integers(-min(sr, 7), min(sr, 7) + 1)), int(rng.integers(-min(sr, 7), min(sr, 7) + 1))
            o = sr + 4
            cur = base[8 + o + dy:8 + o + dy + 64, 8 + o + dx:8 + o + dx + 64].astype(np.int16)
        else:
            cur = rng.integers(0, 256, size=(64, 64)).astype(np.int16)
            ref = rng.integers(0, 256, size=(side, side)).astype(np.int16)
        o = sr + 4
        lt = (-int(rng.integers(0, sr + 1)), -int(rng.integers(0, sr + 1)))
        rb = (int(rng.integers(0, sr + 1)), int(rng.integers(0, sr + 1)))
        if it % 5 == 0:
            lt, rb = (-sr, -sr), (sr, sr)
        pred = (int(rng.integers(-80, 81)), int(rng.integers(-80, 81)))
        fen = int(rng.integers(0, 2))
        lam = float(rng.choice([0.0, 4.7, 57.9, 2000.0, 6.0e6]))
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        engine.set_lambda(lam)
        assert engine.lambda_q16 == lq
        p = api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, 8)
        mv, sad = engine.search_ctu(cur, (0, 0), ref, (o, o), p)
        op = oracle_lib.make_params(lt, rb, pred, lq, fen, 8)
        ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), op)
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy), f"iter {it}: MV mismatch"
        assert np.array_equal(sad, osad), f"iter {it}: SAD mismatch"
        if kind == 3 and lt[0] <= dx <= rb[0] and lt[1] <= dy <= rb[1] and lam < 100:
            assert tuple(mv[592]) == (dx, dy) and sad[592] == 0


def test_weighted_prediction_search_matches_reference_goldens_and_oracle(engine, oracle_lib):
    """hmme_search_ctu_w == TEncSearch::xPatternSearch with m_cDistParam.bApplyWeight (explicit weighted prediction: every candidate priced
    by xGetSADw) on all 593 PU rectangles: goldens from the compiled reference (tests/golden/wp.npz: fades and the weights that undo them,
    a negative weight, a mismatched weight, shift 0, 10 bit, a clipped window), then random weights / windows / search ranges against the
    oracle, and what the engine must refuse (weighted samples beyond a Pel)."""
    from hmme import api
    d = np.load(os.path.join(GOLDEN, "wp.npz"))
    for i in range(len(d["cur"])):
        m = dict(zip(d["meta_columns"].tolist(), (int(v) for v in d["meta"][i])))
        engine.set_lambda_q16(m["lambda_q16"])
        p = api.SearchParams(m["lt_x"], m["lt_y"], m["rb_x"], m["rb_y"], m["pred_x"], m["pred_y"], m["fen"], m["bit_depth"])
        wp = (m["wp_w"], m["wp_offset"], m["wp_shift"], m["wp_round"])
        mv, sad = engine.search_ctu_w(np.ascontiguousarray(d["cur"][i]), (0, 0), np.ascontiguousarray(d["ref"][i]), (m["origin_x"], m["origin_y"]), p, wp)
        want = d["out"][i]
        assert np.array_equal(mv.astype(np.int64), want[:, :2]), f"wp case {i}: MV mismatch"
        assert np.array_equal(sad.astype(np.int64), want[:, 2]), f"wp case {i}: SAD mismatch"
    rng = np.random.default_rng(4242)
    refused = 0
    for it in range(30):
        bd = int(rng.choice([8, 8, 10, 12]))
        sr = int(rng.choice([2, 8, 17, 40, 64, 100]))
        side = 64 + 2 * sr + 8
        o = sr + 4
        maxv = (1 << bd) - 1
        ref = rng.integers(0, maxv + 1, size=(side, side)).astype(np.int16)
        shift = int(rng.integers(0, 8))
        denom = 1 << shift
        w0 = int(rng.integers(-denom, 2 * denom + 1)) if it % 3 else int(rng.integers(-128, 128))
        wp = (w0, int(rng.integers(-128, 128)) << (bd - 8), shift, denom >> 1)
        dx, dy = int(rng.integers(-min(sr, 9), min(sr, 9) + 1)), int(rng.integers(-min(sr, 9), min(sr, 9) + 1))
        blk = ref[o + dy:o + dy + 64, o + dx:o + dx + 64].astype(np.int64)
        if it % 2:   # the current block IS the weighted reference at (dx, dy), clipped like a real picture, + noise
            cur = np.clip(((wp[0] * blk + wp[3]) >> wp[2]) + wp[1] + rng.integers(-2, 3, size=(64, 64)), 0, maxv).astype(np.int16)
        else:
            cur = rng.integers(0, maxv + 1, size=(64, 64)).astype(np.int16)
        if it % 7 == 3:   # a bi-prediction origin under weighted prediction: samples in [-maxv, 2 maxv]
            cur = rng.integers(-maxv, 2 * maxv + 1, size=(64, 64)).astype(np.int16)
        lt = (-int(rng.integers(0, sr + 1)), -int(rng.integers(0, sr + 1)))
        rb = (int(rng.integers(0, sr + 1)), int(rng.integers(0, sr + 1)))
        if it % 4 == 0:
            lt, rb = (-sr, -sr), (sr, sr)
        pred = (int(rng.integers(-60, 61)), int(rng.integers(-60, 61)))
        lam = float(rng.choice([0.0, 57.9, 3000.0]))
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        engine.set_lambda(lam)
        fen = int(rng.integers(0, 2))
        p = api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, bd)
        wlo = min(((w0 * v + wp[3]) >> shift) + wp[1] for v in (0, maxv))
        whi = max(((w0 * v + wp[3]) >> shift) + wp[1] for v in (0, maxv))
        try:
            mv, sad = engine.search_ctu_w(cur, (0, 0), ref, (o, o), p, wp)
        except api.HmmeError as e:
            # refusals are allowed only where the engine says so: weighted samples beyond a Pel / 16 bits, or sums beyond the cost field
            assert ("beyond a Pel" in str(e) and (wlo < -32768 or whi > 32767)) or "cost field" in str(e) or "16 bits" in str(e), (it, wp, str(e))
            refused += 1
            continue
        op = oracle_lib.make_params(lt, rb, pred, lq, fen, bd)
        ox, oy, osad = oracle_lib.search_ctu_w(cur, (0, 0), ref, (o, o), op, wp)
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy), f"iter {it} {wp}: MV mismatch"
        assert np.array_equal(sad, osad), f"iter {it} {wp}: SAD mismatch"
    assert refused <= 12
    # beyond a Pel: refused, never wrapped
    ref = np.full((88, 88), 1023, np.int16)
    with pytest.raises(api.HmmeError, match="beyond a Pel"):
        engine.search_ctu_w(np.zeros((64, 64), np.int16), (0, 0), ref, (12, 12), api.SearchParams(-8, -8, 8, 8, 0, 0, 1, 10), (127, 0, 0, 0))
    # weight (1 << shift, 0): the unweighted search with every row counted
    cur = rng.integers(0, 256, size=(64, 64)).astype(np.int16)
    ref = rng.integers(0, 256, size=(88, 88)).astype(np.int16)
    engine.set_lambda(57.9)
    a = engine.search_ctu_w(cur, (0, 0), ref, (12, 12), api.SearchParams(-8, -8, 8, 8, 3, -5, 1, 8), (64, 0, 6, 32))
    b = engine.search_ctu(cur, (0, 0), ref, (12, 12), api.SearchParams(-8, -8, 8, 8, 3, -5, 0, 8))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_weighted_search_and_refinement_in_one_call_vs_oracle(engine, oracle_lib):
    """hmme_search_refine_ctu_w: the integer search priced by xGetSADw and, on its winners, xPatternSearchFracDIF priced by xGetHADsw /
    xGetSADw (the interpolated prediction weighted sample by sample) -- all 593 slots against the oracle, whose weighted refinement is
    pinned by 112 goldens from the compiled reference (tests/golden/frac_wp.npz); fades and mismatched weights, negative weights,
    shift 0, 8 / 10 bit, Hadamard and SAD, bi-prediction origins"""
    from hmme import api
    table = oracle_lib.slot_table()
    rng = np.random.default_rng(515)
    done = 0
    for it in range(14):
        bd = 10 if it % 4 == 3 else 8
        sr = int(rng.choice([4, 8, 16, 33]))
        side = 64 + 2 * sr + 16
        o = sr + 8
        maxv = (1 << bd) - 1
        base = rng.integers(0, maxv + 1, size=(side + 8, side + 8))
        k = np.ones(3) / 3.0   # a little smoothing: fractional positions then matter
        sm = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, base.astype(np.float64)))
        ref = np.clip(np.rint(sm[4:4 + side, 4:4 + side]), 0, maxv).astype(np.int16)
        shift = int(rng.choice([0, 5, 6, 7]))
        denom = 1 << shift
        w0 = int(rng.integers(denom // 2, 2 * denom + 1)) if it % 5 else -int(rng.integers(1, denom + 1))
        wp = (w0, int(rng.integers(-40, 41)) << (bd - 8), shift, denom >> 1)
        dx, dy = int(rng.integers(-min(sr, 5), min(sr, 5) + 1)), int(rng.integers(-min(sr, 5), min(sr, 5) + 1))
        blk = ref[o + dy:o + dy + 64, o + dx:o + dx + 64].astype(np.int64)
        cur = np.clip(((wp[0] * blk + wp[3]) >> wp[2]) + wp[1] + rng.integers(-3, 4, size=(64, 64)), 0, maxv).astype(np.int16)
        if it % 6 == 5:
            cur = np.clip(2 * cur.astype(np.int64) - rng.integers(0, maxv + 1, size=(64, 64)), -maxv, 2 * maxv).astype(np.int16)   # a bi-prediction origin
        pred = (int(rng.integers(-30, 31)), int(rng.integers(-30, 31)))
        lam = float(rng.choice([0.0, 57.9, 600.0]))
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        engine.set_lambda(lam)
        had = it % 3 != 2
        p = api.SearchParams(-sr, -sr, sr, sr, pred[0], pred[1], 1, bd)
        try:
            mv, sad, qmv, cost = engine.search_refine_ctu_w(cur, (0, 0), ref, (o, o), p, wp, use_hadamard=had)
        except api.HmmeError as e:
            assert "Pel" in str(e) or "cost field" in str(e) or "16 bits" in str(e) or "Hadamard sums" in str(e), str(e)
            continue
        op = oracle_lib.make_params((-sr, -sr), (sr, sr), pred, lq, 1, bd)
        ox, oy, osad = oracle_lib.search_ctu_w(cur, (0, 0), ref, (o, o), op, wp)
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad), (it, wp)
        for s_ in range(593):
            x, y, bw, bh = (int(v) for v in table[s_])
            imv = (int(mv[s_, 0]), int(mv[s_, 1]))
            hx, hy, qx, qy, c = oracle_lib.frac_refine_w(cur, (x, y), ref, (o + x, o + y), bw, bh, imv, pred, lq, int(had), bd, wp)
            assert (int(qmv[s_, 0]), int(qmv[s_, 1]), int(cost[s_])) == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (it, s_, wp, (bw, bh))
        done += 1
    assert done >= 10
    # the identity weight: the refinement of the unweighted call (its integer search runs with FEN off, as xGetSADw reads every row)
    cur = rng.integers(0, 256, size=(64, 64)).astype(np.int16)
    ref = rng.integers(0, 256, size=(96, 96)).astype(np.int16)
    engine.set_lambda(57.9)
    a = engine.search_refine_ctu_w(cur, (0, 0), ref, (16, 16), api.SearchParams(-8, -8, 8, 8, 2, 1, 1, 8), (64, 0, 6, 32))
    b = engine.search_refine_ctu(cur, (0, 0), ref, (16, 16), api.SearchParams(-8, -8, 8, 8, 2, 1, 0, 8))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_ocl_compat_mode_vs_oracle(engine, oracle_lib):
    """the reference GPU path's choices (pred (0,0), window LT..LT+2SR, all rows): cl/sad.cl:374-408"""
    from hmme import api
    rng = np.random.default_rng(5)
    sr = 8
    cur = rng.integers(0, 256, size=(64, 64)).astype(np.int16)
    ref = rng.integers(0, 256, size=(64 + 4 * sr + 8, 64 + 4 * sr + 8)).astype(np.int16)
    o = 2 * sr + 2
    lq = oracle_lib.oracle().hmo_lambda_q16(57.9)
    engine.set_lambda(57.9)
    p = api.ocl_compat_params(-sr - 3, -sr + 2, sr)
    mv, sad = engine.search_ctu(cur, (0, 0), ref, (o, o), p)
    import ctypes as C
    op = oracle_lib.Params()
    oracle_lib.oracle().hmo_ocl_compat_params(C.byref(op), -sr - 3, -sr + 2, sr, C.c_uint32(lq))
    ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), op)
    assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad)


@pytest.mark.parametrize("w,h,sr,fen,use_pred", [(64, 64, 8, 1, False),   # BASELINE config 1 shape: one CTU, SR 8
                                                 (200, 136, 16, 1, True), (320, 192, 64, 1, False), (192, 128, 8, 0, True)])
def test_search_frame_vs_oracle(engine, oracle_lib, w, h, sr, fen, use_pred):
    """whole-picture path incl. partial edge CTUs and clipped windows == oracle frame search"""
    from hmme import synth
    cur, ref, _ = synth.make_pair(w, h, seed=w + sr, max_mv=min(sr, 12), region=64)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    pred = synth.random_predictors(n_ctu, seed=3, max_pel=sr) if use_pred else None
    lq = oracle_lib.oracle().hmo_lambda_q16(57.9)
    engine.set_lambda(57.9)
    pc, pr = engine.plane(w, h), engine.plane(w, h)
    pc.upload_pel(cur, (synth.MARGIN, synth.MARGIN))
    pr.upload_pel(ref, (synth.MARGIN, synth.MARGIN))
    mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (synth.MARGIN, synth.MARGIN), w, h, sr, pred, lq, fen, 8, n_threads=8)
    pc.close(); pr.close()
    assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy)
    assert np.array_equal(sad, osad)


def test_frame_ctu_subrange_and_u8_upload(engine, oracle_lib):
    from hmme import synth
    w, h, sr = 256, 128, 8
    cur, ref, _ = synth.make_pair(w, h, seed=9, max_mv=6, region=64)
    m = synth.MARGIN
    pc, pr = engine.plane(w, h), engine.plane(w, h)
    pc.upload_u8(cur[m:m + h, m:m + w].astype(np.uint8))
    pr.upload_u8(ref[m:m + h, m:m + w].astype(np.uint8))
    engine.set_lambda(57.9)
    full_mv, full_sad = engine.search_frame(pc, pr, sr)
    part_mv, part_sad = engine.search_frame(pc, pr, sr, ctu_first=3, ctu_count=4)
    pc.close(); pr.close()
    assert np.array_equal(part_mv, full_mv[3:7]) and np.array_equal(part_sad, full_sad[3:7])
    lq = oracle_lib.oracle().hmo_lambda_q16(57.9)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, None, lq, 1, 8, n_threads=4)
    assert np.array_equal(full_mv[:, :, 0], ox) and np.array_equal(full_sad, osad)


def test_error_behaviour(engine):
    """errors come back as status codes with a message; nothing falls back to the CPU"""
    from hmme import api
    cur = np.zeros((64, 64), np.int16)
    ref = np.zeros((100, 100), np.int16)
    engine.set_lambda(1.0)
    bad = api.SearchParams(-129, -8, 129, 8, 0, 0, 1, 8)         # window wider than 2 * sr_max + 1
    with pytest.raises(api.HmmeError, match="window"):
        engine.search_ctu(cur, (0, 0), np.zeros((100, 400), np.int16), (140, 18), bad)
    with api.Engine(0, 32) as small:                             # an engine created for a smaller range enforces it
        with pytest.raises(api.HmmeError, match="window"):
            small.search_ctu(cur, (0, 0), np.zeros((100, 200), np.int16), (50, 18), api.SearchParams(-40, -8, 40, 8, 0, 0, 1, 8))
    p14 = api.SearchParams(-8, -8, 8, 8, 0, 0, 1, 14)
    with pytest.raises(api.HmmeError, match="bit depth"):
        engine.search_ctu(cur, (0, 0), ref, (18, 18), p14)
    wide8 = api.SearchParams(-130, -8, 130, 8, 0, 0, 1, 8)          # beyond HMME_MAX_SEARCH_RANGE
    with pytest.raises(api.HmmeError, match="window"):
        engine.search_ctu(cur, (0, 0), np.zeros((100, 400), np.int16), (148, 18), wide8)
    cur2 = cur.copy(); cur2[5, 5] = 999                             # beyond even a bi-pred origin (2*255)
    p = api.SearchParams(-8, -8, 8, 8, 0, 0, 1, 8)
    with pytest.raises(api.HmmeError, match="outside"):
        engine.search_ctu(cur2, (0, 0), ref, (18, 18), p)
    ref2 = ref.copy(); ref2[30, 30] = -1                            # reference samples must be real samples
    with pytest.raises(api.HmmeError, match="reference sample"):
        engine.search_ctu(cur, (0, 0), ref2, (18, 18), p)
    pl = engine.plane(64, 64)
    with pytest.raises(api.HmmeError, match="outside"):
        pl.upload_pel(np.full((64, 64), 700, np.int16), (0, 0))
    pl.close()
    with pytest.raises(api.HmmeError):
        api.Engine(0, 4096)


def test_1080p_planted_motion_and_oracle_spot_check(engine, oracle_lib):
    """BASELINE config 2 shape (1920x1080, SR 64, FEN 1): size-independent properties over the whole
    frame + bit-exact oracle comparison on a CTU sample"""
    from hmme import synth
    w, h, sr = 1920, 1080, 64
    cur, ref, true_mv = synth.make_pair(w, h, seed=1234, max_mv=12, region=128, noise_sigma=0.0)
    m = synth.MARGIN
    engine.set_lambda(57.9)
    pc, pr = engine.plane(w, h), engine.plane(w, h)
    pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
    mv, sad = engine.search_frame(pc, pr, sr)
    qmv, cost = engine.refine_frame(pc, pr, sr, mv)          # the step after the path, on the whole picture
    pc.close(); pr.close()
    ctus_x = 30
    assert mv.shape == (510, 593, 2)
    # (1) noise-free translated texture: interior CTUs that lie inside one 128x128 region find it exactly
    hits = 0
    for cy in range(0, 16, 2):
        for cx in range(0, 30, 2):
            # CTU (cx,cy) and its right/bottom neighbour share a region; take the region-aligned one
            ctu = cy * ctus_x + cx
            dx, dy = true_mv[cy // 2, cx // 2]
            if cx in (0, 28) or cy in (0, 14):
                continue
            assert tuple(mv[ctu, 592]) == (dx, dy) and sad[ctu, 592] == 0, (cx, cy)
            hits += 1
    assert hits > 50
    # (2) hierarchy consistency: a PU's best cost can never beat the sum of ... (SAD additivity at the
    # winning MV of the 64x64 PU): SAD(64x64 @ mv592) == sum of the four 32x32 SADs at that MV >= sum of
    # the 32x32 minima's SADs is NOT guaranteed with MV costs, so only check range sanity here
    assert sad.max() < 1044481
    # (3) the whole picture against the oracle: 510 CTUs x 593 slots
    lq = oracle_lib.oracle().hmo_lambda_q16(57.9)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, None, lq, 1, 8, n_threads=16)
    assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy) and np.array_equal(sad, osad)
    # (4) ... and xPatternSearchFracDIF (Hadamard) of all 510 x 593 winners against the oracle's
    oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), w, h, mv, None, lq, 1, 8, n_threads=16)
    assert np.array_equal(qmv, oq) and np.array_equal(cost, oc)


def test_cpp_host_module_tencopencl(oracle_lib):
    """the TEncOpenCL-shaped C++ class, driven like TEncTop / TEncSearch drive the reference's"""
    import subprocess
    from conftest import ROOT
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hm-opencl_amd", "host")], check=True)
    exe = os.path.join(ROOT, "tests", "cpp", "test_tencopencl")
    subprocess.run(["g++", "-O2", "-std=c++11", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_tencopencl.cpp"),
                    "-L" + os.path.join(ROOT, "hm-opencl_amd", "host"), "-lhmme_host",
                    "-L" + os.path.join(ROOT, "hm-opencl_amd", "csrc"), "-lhmme",
                    "-L" + os.path.join(ROOT, "oracle"), "-loracle",
                    "-Wl,-rpath," + os.path.join(ROOT, "hm-opencl_amd", "host"),
                    "-Wl,-rpath," + os.path.join(ROOT, "hm-opencl_amd", "csrc"),
                    "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


def test_cpp_host_module_for_an_encoder_built_with_amp_enc_speedup(oracle_lib):
    """the same class compiled with -DNUM_CTU_PARTS=425 (an HM built with AMP_ENC_SPEEDUP, TypeDef.h:260-261): its tables are the 425
    entries of that build's getIndexBlock (TComDataCU.cpp:3393-4675), filled from the engine's 593 results; against the oracle"""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "test_tencopencl_amp_off")
    subprocess.run(["g++", "-O2", "-std=c++11", "-DNUM_CTU_PARTS=425", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_tencopencl_amp_off.cpp"),
                    os.path.join(ROOT, "hm-opencl_amd", "host", "TEncOpenCL.cpp"),
                    "-L" + os.path.join(ROOT, "hm-opencl_amd", "csrc"), "-lhmme", "-L" + os.path.join(ROOT, "oracle"), "-loracle",
                    "-Wl,-rpath," + os.path.join(ROOT, "hm-opencl_amd", "csrc"), "-Wl,-rpath," + os.path.join(ROOT, "oracle")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout


def test_16bit_path_random_windows_vs_oracle(engine, oracle_lib):
    """bit depth 10 / 12 (v_sad_u16 kernel): ragged windows up to SR 128, FEN 0/1, strips"""
    from hmme import api
    rng = np.random.default_rng(1010)
    for it in range(14):
        bd = int(rng.choice([10, 10, 12, 9]))
        sr = int(rng.choice([2, 8, 33, 64, 100, 128]))
        side = 64 + 2 * sr + 8
        cur = rng.integers(0, 1 << bd, size=(64, 64)).astype(np.int16)
        ref = rng.integers(0, 1 << bd, size=(side, side)).astype(np.int16)
        o = sr + 4
        if it % 3 == 2:   # planted motion
            dx, dy = int(rng.integers(-min(sr, 9), min(sr, 9) + 1)), int(rng.integers(-min(sr, 9), min(sr, 9) + 1))
            cur = ref[o + dy:o + dy + 64, o + dx:o + dx + 64].copy()
        lt = (-int(rng.integers(0, sr + 1)), -int(rng.integers(0, sr + 1)))
        rb = (int(rng.integers(0, sr + 1)), int(rng.integers(0, sr + 1)))
        if it % 4 == 0:
            lt, rb = (-sr, -sr), (sr, sr)
        pred = (int(rng.integers(-80, 81)), int(rng.integers(-80, 81)))
        fen = int(rng.integers(0, 2))
        lam = float(rng.choice([0.0, 57.9, 900.0, 6.0e6]))
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        engine.set_lambda(lam)
        p = api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, bd)
        mv, sad = engine.search_ctu(cur, (0, 0), ref, (o, o), p)
        ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), oracle_lib.make_params(lt, rb, pred, lq, fen, bd))
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy), f"iter {it} (bd {bd}, sr {sr}): MV mismatch"
        assert np.array_equal(sad, osad), f"iter {it}: SAD mismatch"


@pytest.mark.parametrize("w,h,sr,fen", [(200, 136, 16, 1), (256, 192, 64, 1), (192, 128, 128, 0)])
def test_search_frame_10bit_vs_oracle(engine, oracle_lib, w, h, sr, fen):
    """BASELINE config 5 shape in small: 10-bit planes, SR up to 128 (window strips merged through global atomics)"""
    from hmme import synth
    cur, ref, _ = synth.make_pair(w, h, seed=w + sr, bit_depth=10, max_mv=min(sr, 12), region=64)
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    pred = synth.random_predictors(n_ctu, seed=4, max_pel=min(sr, 24))
    lq = oracle_lib.oracle().hmo_lambda_q16(238.5)
    engine.set_lambda(238.5)
    m = synth.MARGIN
    pc, pr = engine.plane(w, h, 10), engine.plane(w, h, 10)
    pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
    mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
    pc.close(); pr.close()
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, fen, 10, n_threads=8)
    assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy)
    assert np.array_equal(sad, osad)


def test_plane_bit_depth_mismatch_is_an_error(engine):
    from hmme import api
    p8, p10 = engine.plane(64, 64), engine.plane(64, 64, 10)
    p8.upload_u8(np.zeros((64, 64), np.uint8))
    p10.upload_pel(np.full((64, 64), 1000, np.int16), (0, 0))
    with pytest.raises(api.HmmeError, match="outside"):
        p10.upload_pel(np.full((64, 64), 1024, np.int16), (0, 0))
    with pytest.raises(api.HmmeError, match="bit"):
        engine.search_frame(p8, p10, 8)
    with pytest.raises(api.HmmeError, match="search range"):
        engine.search_frame(p8, p8, 129)          # beyond HMME_MAX_SEARCH_RANGE
    p8.close(); p10.close()


def test_bipred_origins_outside_the_sample_range(engine, oracle_lib):
    """bi-prediction refinement (reference TEncSearch.cpp:3702-3712, 3221): the current block is
    2*org - pred_other, unclipped (TComYuv.cpp:409-440), SearchRange = BipredSearchRange = 4.
    Such blocks run on the 16-bit kernel with biased samples and must stay bit-exact."""
    from hmme import api
    rng = np.random.default_rng(4242)
    for it in range(10):
        bd = 8 if it % 3 else 10
        maxv = (1 << bd) - 1
        sr = 4 if it % 2 == 0 else int(rng.choice([8, 20]))
        side = 64 + 2 * sr + 8
        org = rng.integers(0, maxv + 1, size=(64, 64))
        other = rng.integers(0, maxv + 1, size=(64, 64))
        cur = (2 * org - other).astype(np.int16)                       # in [-maxv, 2*maxv]
        if it == 0:
            cur[0, 0], cur[63, 63] = -maxv, 2 * maxv                   # the extremes
        ref = rng.integers(0, maxv + 1, size=(side, side)).astype(np.int16)
        o = sr + 4
        lt, rb = (-sr, -sr), (sr, sr)
        pred = (int(rng.integers(-20, 21)), int(rng.integers(-20, 21)))
        fen = int(rng.integers(0, 2))
        lam = float(rng.choice([4.7, 57.9, 5.0e6]))
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        engine.set_lambda(lam)
        mv, sad = engine.search_ctu(cur, (0, 0), ref, (o, o), api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, bd))
        ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), oracle_lib.make_params(lt, rb, pred, lq, fen, bd))
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy), f"iter {it}: MV mismatch"
        assert np.array_equal(sad, osad), f"iter {it}: SAD mismatch"


def test_2160p_whole_frame_properties_and_spot_checks(engine, oracle_lib):
    """BASELINE config 3 shape (3840x2160, SR 64, FEN 1): per-CTU random predictors (clipped windows at the
    picture edges), planted motion recovered everywhere it is recoverable, oracle equality on a CTU sample."""
    from hmme import synth
    w, h, sr = 3840, 2160, 64
    cur, ref, true_mv = synth.make_pair(w, h, seed=77, max_mv=20, region=256, noise_sigma=0.0)
    m = synth.MARGIN
    n_ctu = 60 * 34
    pred = synth.random_predictors(n_ctu, seed=77, max_pel=24)
    engine.set_lambda(57.9)
    lq = engine.lambda_q16
    pc, pr = engine.plane(w, h), engine.plane(w, h)
    pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
    mv, sad = engine.search_frame(pc, pr, sr, pred)
    mv2, sad2 = engine.search_frame(pc, pr, sr, pred)                    # idempotence: no state leaks between launches
    pc.close(); pr.close()
    assert mv.shape == (n_ctu, 593, 2) and np.array_equal(mv, mv2) and np.array_equal(sad, sad2)
    hits = 0
    for cy in range(1, 32):
        for cx in range(1, 59):
            if (cx % 4) in (0, 3) or (cy % 4) in (0, 3):                  # keep CTUs strictly inside one 256x256 region
                continue
            dx, dy = (int(v) for v in true_mv[cy // 4, cx // 4])
            ctu = cy * 60 + cx
            px, py = int(pred[ctu, 0]) >> 2, int(pred[ctu, 1]) >> 2
            if abs(dx - px) < sr - 1 and abs(dy - py) < sr - 1:           # planted MV lies inside this CTU's window
                assert sad[ctu, 592] == 0 and tuple(mv[ctu, 592]) == (dx, dy), (cx, cy)
                hits += 1
    assert hits > 300
    # the whole picture against the oracle: all 2 040 CTUs x 593 slots (16 host threads: a few seconds)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, 1, 8, n_threads=16)
    bad = np.flatnonzero((mv[:, :, 0] != ox).any(axis=1) | (mv[:, :, 1] != oy).any(axis=1) | (sad != osad).any(axis=1))
    assert bad.size == 0, f"CTUs that differ from the oracle: {bad[:20]}"


def test_engine_lifecycle_and_two_contexts(oracle_lib):
    from hmme import api, synth
    w, h, sr = 128, 128, 8
    cur, ref, _ = synth.make_pair(w, h, seed=3, max_mv=5, region=64)
    m = synth.MARGIN
    lq = oracle_lib.oracle().hmo_lambda_q16(57.9)
    want = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, None, lq, 1, 8)
    engines = []
    for i in range(4):                                                    # create/destroy cycles and two live contexts
        e = api.Engine(0, 16 + 16 * i)
        e.set_lambda(57.9)
        engines.append(e)
        if len(engines) > 2:
            engines.pop(0).close()
        for eng in engines:
            pc, pr = eng.plane(w, h), eng.plane(w, h)
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            mv, sad = eng.search_frame(pc, pr, sr)
            assert np.array_equal(mv[:, :, 0], want[0]) and np.array_equal(mv[:, :, 1], want[1]) and np.array_equal(sad, want[2])
            pc.close(); pr.close()
    for e in engines:
        e.close()


def test_planes_of_another_context_are_refused_and_error_printing_is_restorable(oracle_lib):
    """a launch ties the planes it reads to an event of the launching context (hmme.hip plane_read_mark): a plane created by context A
    launched through context B would be left pointing at B's events after B is destroyed -- every frame call refuses it (HMME_ERR_ARG),
    search and refinement, whichever of the two planes is the foreign one; A's own use of the plane is unaffected afterwards.
    hmme_set_error_printing returns the previous setting (a probing caller restores what ITS caller had chosen)"""
    from hmme import api, synth
    w, h, sr = 128, 64, 8
    cur, ref, _ = synth.make_pair(w, h, seed=5, max_mv=4, region=64)
    m = synth.MARGIN
    with api.Engine(0, 16) as a, api.Engine(0, 16) as b:
        a.set_lambda(57.9); b.set_lambda(57.9)
        assert a.L.hmme_set_error_printing(b.h, 0) == 1 and a.L.hmme_set_error_printing(b.h, 0) == 0      # quiet: the refusals below are expected
        assert a.L.hmme_set_error_printing(None, 0) == 1
        pa_c, pa_r, pb_c, pb_r = a.plane(w, h), a.plane(w, h), b.plane(w, h), b.plane(w, h)
        for pl in (pa_c, pb_c):
            pl.upload_pel(cur, (m, m))
        for pl in (pa_r, pb_r):
            pl.upload_pel(ref, (m, m))
        want = a.search_frame(pa_c, pa_r, sr)
        for pc, pr in ((pa_c, pb_r), (pb_c, pa_r), (pa_c, pa_r)):
            with pytest.raises(api.HmmeError, match="another context"):
                b.search_frame(pc, pr, sr)
            with pytest.raises(api.HmmeError, match="another context"):
                b.refine_frame(pc, pr, sr, want[0])
        got_b = b.search_frame(pb_c, pb_r, sr)
        assert a.L.hmme_set_error_printing(b.h, 1) == 0
        for pl in (pb_c, pb_r):
            pl.close()
    # b is gone; a's planes were never tied to it
    with api.Engine(0, 16) as a2:
        pass
    assert np.array_equal(want[0], got_b[0]) and np.array_equal(want[1], got_b[1])


def test_sequence_driver_single_gpu(tmp_path):
    """tools/me_sequence.py (BASELINE config 4 driver) on one GPU with a small synthetic sequence"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "me_sequence.py"), "--frames", "6", "--gop", "randomaccess",
                        "--size", "640x448", "--search-range", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["pairs"] == 9 and d["gpus"] == 1
    # frame t is the texture shifted by (3t, 2t): pair (4, 0) -> MV (-12, -8) for cur(x) = ref(x + mv) ... sign per synth.make_pair
    assert d["first_pairs"][0] == [4, 0] and [abs(v) for v in d["median_mv_64x64_of_first_pairs"][0]] == [12, 8]


@pytest.mark.parametrize("bd", [8, 10])
def test_multi_reference_launch_equals_per_reference_searches(engine, bd):
    """hmme_search_frame_multi: the low-delay P structure searches 4 references per picture (reference
    cfg/encoder_lowdelay_P_main.cfg:24-27); one launch must equal four single-reference searches.
    NOTE: this compares the HIP path with ITSELF (batched launch vs single launches); the oracle comparison of a multi-reference
    launch is in test_tail_plan_pictures_whose_searches_do_not_fill_whole_rounds (refs = 2) and, for launches of different
    picture PAIRS, in tests/test_gpu_sequence.py::test_pairs_per_launch_equals_single_launches_and_oracle."""
    from hmme import synth
    w, h, sr = 256, 192, 16
    m = synth.MARGIN
    engine.set_lambda(57.9)
    cur, _, _ = synth.make_pair(w, h, seed=1, bit_depth=bd, max_mv=0, shift=(0, 0), pad=40)
    pc = engine.plane(w, h, bd)
    pc.upload_pel(cur, (m, m))
    refs = []
    for t in range(1, 5):
        r, _, _ = synth.make_pair(w, h, seed=1, bit_depth=bd, max_mv=0, shift=(3 * t, -2 * t), pad=40)
        pl = engine.plane(w, h, bd)
        pl.upload_pel(r, (m, m))
        refs.append(pl)
    n_ctu = 4 * 3
    pred = np.stack([synth.random_predictors(n_ctu, seed=10 + t, max_pel=8) for t in range(4)])
    mv, sad = engine.search_frame_multi(pc, refs, sr, pred)
    for t in range(4):
        mv1, sad1 = engine.search_frame(pc, refs[t], sr, pred[t])
        assert np.array_equal(mv[t], mv1) and np.array_equal(sad[t], sad1), t
    assert len({tuple(mv[t, 5, 592]) for t in range(4)}) == 4      # the four references really differ
    for pl in refs:
        pl.close()
    pc.close()


def test_device_resident_producer_and_async_api(engine, oracle_lib):
    """planes filled from device memory (a torch tensor) and the asynchronous, all-device entry point that
    bench.py uses, with per-CTU predictors living on the device"""
    import torch
    from hmme import api, synth
    w, h, sr = 320, 192, 24
    cur, ref, _ = synth.make_pair(w, h, seed=21, max_mv=9, region=64)
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    t_cur = torch.from_numpy(cur[m:m + h, m:m + w].astype(np.uint8)).to(dev)
    t_ref = torch.from_numpy(np.ascontiguousarray(ref[m:m + h, m:m + w].astype(np.uint8))).to(dev)
    n_ctu = 5 * 3
    pred = synth.random_predictors(n_ctu, seed=2, max_pel=10)
    d_pred = torch.from_numpy(pred).to(dev)
    d_mv = torch.zeros((n_ctu, 593, 2), dtype=torch.int16, device=dev)
    d_sad = torch.zeros((n_ctu, 593), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    engine.set_lambda(57.9)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.set_device_u8(t_cur.data_ptr(), t_cur.stride(0), stream)
        pr.set_device_u8(t_ref.data_ptr(), t_ref.stride(0), stream)
        fp = api.FrameParams(sr, 1, 8, 0, n_ctu)
        engine.search_frame_device(pc, pr, fp, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), stream)
        torch.cuda.synchronize()
        ms = engine.time_search_kernel(pc, pr, fp, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), stream, reps=2)
    assert ms > 0
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, engine.lambda_q16, 1, 8, n_threads=4)
    assert np.array_equal(d_mv.cpu().numpy()[:, :, 0], ox) and np.array_equal(d_mv.cpu().numpy()[:, :, 1], oy)
    assert np.array_equal(d_sad.cpu().numpy().astype(np.uint32), osad)


@pytest.mark.parametrize("use_had,sr,use_pred,bd", [(1, 16, True, 8), (0, 16, True, 8), (1, 64, False, 8), (1, 16, True, 10),
                                                      (0, 64, False, 12), (1, 24, True, 9), (1, 17, True, -8), (0, 33, False, -10),
                                                      (1, 128, False, 10), (0, 96, True, 12), (1, 70, True, -10)])
def test_fractional_refinement_vs_oracle(engine, oracle_lib, use_had, sr, use_pred, bd):
    """the step after the path: xPatternSearchFracDIF for all 593 slots of every CTU (half + quarter-pel, HM's
    8-tap interpolation, Hadamard or SAD), fed with the engine's own integer MVs"""
    from hmme import synth
    w, h = 200, 136                                   # 4 x 3 CTUs, partial right column and bottom row
    unrelated = bd < 0   # negative depth: current and reference are unrelated noise -> nearly every slot has its own MV (no work sharing)
    bd = abs(bd)
    cur, ref, _ = synth.make_pair(w, h, seed=31 + sr, bit_depth=bd, max_mv=min(sr, 9), region=64, noise_sigma=2.5)
    if unrelated:
        rng0 = np.random.default_rng(77 + sr)
        cur = np.ascontiguousarray(np.pad(rng0.integers(0, 1 << bd, size=(h, w)), synth.MARGIN, mode="edge").astype(cur.dtype))
        ref = np.ascontiguousarray(np.pad(rng0.integers(0, 1 << bd, size=(h, w)), synth.MARGIN, mode="edge").astype(ref.dtype))
    m = synth.MARGIN
    n_ctu = 4 * 3
    pred = synth.random_predictors(n_ctu, seed=8, max_pel=6) if use_pred else None
    engine.set_lambda(57.9)
    lq = engine.lambda_q16
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred)
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred, use_hadamard=bool(use_had))
    table = oracle_lib.slot_table()
    rng = np.random.default_rng(5)
    checked = 0
    for ctu in range(n_ctu):
        cx, cy = (ctu % 4) * 64, (ctu // 4) * 64
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if use_pred else (0, 0)
        for s in list(rng.choice(593, size=90, replace=False)) + [592, 588, 576, 0, 128, 256, 300]:
            x, y, bw, bh = (int(v) for v in table[s])
            imv = (int(mv[ctu, s, 0]), int(mv[ctu, s, 1]))
            hx, hy, qx, qy, c = oracle_lib.frac_refine(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv,
                                                        (px, py), lq, use_had, bd)
            want = (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c)
            got = (int(qmv[ctu, s, 0]), int(qmv[ctu, s, 1]), int(cost[ctu, s]))
            assert got == want, (ctu, s, (bw, bh), imv, got, want)
            checked += 1
    assert checked > 1000


@pytest.mark.parametrize("bd,use_had", [(8, 1), (8, 0), (10, 1)])
def test_fractional_refinement_partial_sharing_every_slot_vs_oracle(engine, oracle_lib, bd, use_had):
    """content on which the slots of a CTU share SOME of their work (24-sample regions of their own motion under noise): 8x8 items, the
    4x4-kind slots that ride on them and 4x4 items of their own coexist in every CTU.  Every slot of every CTU (partial right column
    and bottom row included) against the oracle's xPatternSearchFracDIF."""
    from hmme import synth
    w, h, sr = 328, 200, 12
    cur, ref, _ = synth.make_pair(w, h, seed=91 + bd, bit_depth=bd, max_mv=8, region=24, noise_sigma=6.0)
    m = synth.MARGIN
    engine.set_lambda(57.9)
    lq = engine.lambda_q16
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, None)
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, None, use_hadamard=bool(use_had))
    oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), w, h, mv, None, lq, use_had, bd, n_threads=16)
    assert np.array_equal(qmv, oq), np.argwhere(qmv != oq)[:5]
    assert np.array_equal(cost, oc), np.argwhere(cost != oc)[:5]
    # the content does what the test is for: neither one MV per CTU nor one per slot
    distinct = [len({tuple(v) for v in mv[c]}) for c in range(mv.shape[0])]
    assert 3 < np.median(distinct) < 300, distinct


def test_refinement_multi_reference_and_errors(engine):
    """device entry point with two references in one launch == two single-reference calls; unsupported inputs fail loudly"""
    import torch
    from hmme import api, synth
    w, h, sr = 192, 128, 12
    m = synth.MARGIN
    engine.set_lambda(57.9)
    cur, _, _ = synth.make_pair(w, h, seed=2, max_mv=0, pad=30)
    planes = []
    for t in range(3):
        f, _, _ = synth.make_pair(w, h, seed=2, max_mv=0, shift=(2 * t, -t), pad=30, noise_sigma=1.0 + t)
        pl = engine.plane(w, h)
        pl.upload_pel(f, (m, m))
        planes.append(pl)
    pc, refs = planes[0], planes[1:]
    n = 3 * 2
    mv, _ = engine.search_frame_multi(pc, refs, sr)
    dev = torch.device("cuda", 0)
    d_mv = torch.from_numpy(mv).to(dev)
    d_q = torch.zeros((2, n, 593, 2), dtype=torch.int16, device=dev)
    d_c = torch.zeros((2, n, 593), dtype=torch.int32, device=dev)
    fp = api.FrameParams(sr, 1, 8, 0, n)
    engine.refine_frame_multi_device(pc, refs, fp, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for r in range(2):
        q1, c1 = engine.refine_frame(pc, refs[r], sr, mv[r])
        assert np.array_equal(d_q[r].cpu().numpy(), q1) and np.array_equal(d_c[r].cpu().numpy().astype(np.uint32), c1)
        assert np.abs(q1.astype(np.int32) - 4 * mv[r].astype(np.int32)).max() <= 3
    with pytest.raises(api.HmmeError, match="search range"):
        engine.refine_frame(pc, refs[0], 129, np.zeros((n, 593, 2), np.int16))
    for pl in planes:
        pl.close()


@pytest.mark.parametrize("w,h,sr,bd", [(40, 24, 16, 8), (8, 8, 8, 8), (72, 8, 32, 8), (8, 200, 64, 8), (40, 24, 16, 10), (136, 72, 128, 10)])
def test_tiny_and_sliver_pictures(engine, oracle_lib, w, h, sr, bd):
    """pictures smaller than a CTU and one-CU-wide slivers: the window is clipped on every side at once (clipMv,
    TComDataCU.cpp:2907-2920) and most of each CTU lies in the padded border"""
    from hmme import api, synth
    cur, ref, _ = synth.make_pair(w, h, seed=w + h, bit_depth=bd, max_mv=min(4, sr))
    m = synth.MARGIN
    n = api.load().hmme_num_ctus(w, h)
    pred = synth.random_predictors(n, seed=3, max_pel=5)
    engine.set_lambda(57.9)
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred)
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred)
        assert np.abs(qmv.astype(np.int32) - 4 * mv.astype(np.int32)).max() <= 3
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, engine.lambda_q16, 1, bd, n_threads=4)
    assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy) and np.array_equal(sad, osad)
    # the refinement of the winners: every slot of every CTU equals the oracle's xPatternSearchFracDIF
    oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), w, h, mv, pred, engine.lambda_q16, 1, bd, n_threads=4)
    assert np.array_equal(qmv, oq), np.argwhere(qmv != oq)[:5]
    assert np.array_equal(cost, oc), np.argwhere(cost != oc)[:5]


@pytest.mark.parametrize("sr,fen,use_pred", [(65, 1, True), (100, 1, False), (128, 0, True)])
def test_8bit_search_range_beyond_64_tiles(engine, oracle_lib, sr, fen, use_pred):
    """8-bit planes with a window beyond 129 x 129 candidates: four tile searches per CTU merged in raster order"""
    from hmme import api, synth
    w, h = 328, 200                                   # 6 x 4 CTUs, partial right column and bottom row; windows clipped at every border
    cur, ref, _ = synth.make_pair(w, h, seed=900 + sr, max_mv=40, region=64, noise_sigma=3.0)
    m = synth.MARGIN
    n = api.load().hmme_num_ctus(w, h)
    pred = synth.random_predictors(n, seed=sr, max_pel=30) if use_pred else None
    engine.set_lambda(57.9)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, engine.lambda_q16, fen, 8, n_threads=8)
    assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy) and np.array_equal(sad, osad)
    assert np.abs(qmv.astype(np.int32) - 4 * mv.astype(np.int32)).max() <= 3
    table = oracle_lib.slot_table()
    for ctu, s in [(0, 592), (7, 300), (n - 1, 0), (9, 566)]:
        cx, cy = (ctu % 6) * 64, (ctu // 6) * 64
        x, y, bw, bh = (int(v) for v in table[s])
        imv = (int(mv[ctu, s, 0]), int(mv[ctu, s, 1]))
        p = (int(pred[ctu, 0]), int(pred[ctu, 1])) if use_pred else (0, 0)
        hx, hy, qx, qy, c = oracle_lib.frac_refine(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, p,
                                                    engine.lambda_q16, 1, 8)
        assert (int(qmv[ctu, s, 0]), int(qmv[ctu, s, 1]), int(cost[ctu, s])) == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c)


def test_search_ctu_8bit_windows_beyond_129(engine, oracle_lib):
    """per-CTU call with an 8-bit window wider / taller than 129 candidates (2 x 1, 1 x 2 and 2 x 2 tiles)"""
    from hmme import api
    rng = np.random.default_rng(11)
    for (lt, rb) in [((-100, -20), (90, 30)), ((-10, -128), (12, 128)), ((-128, -128), (128, 128)), ((-64, -64), (65, 64))]:
        wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
        ref = rng.integers(0, 256, size=(wy + 63 + 8, wx + 63 + 8)).astype(np.int16)
        o = (4 - lt[0], 4 - lt[1])
        dx, dy = int(rng.integers(lt[0], rb[0] + 1)), int(rng.integers(lt[1], rb[1] + 1))
        cur = ref[o[1] + dy:o[1] + dy + 64, o[0] + dx:o[0] + dx + 64].copy()
        cur[::7, ::5] ^= 3
        pred = (int(rng.integers(-200, 201)), int(rng.integers(-200, 201)))
        fen = int(rng.integers(0, 2))
        engine.set_lambda(57.9)
        p = api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, 8)
        mv, sad = engine.search_ctu(cur, (0, 0), ref, o, p)
        op = oracle_lib.make_params(lt, rb, pred, engine.lambda_q16, fen, 8)
        ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, o, op)
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad), (lt, rb)
        assert tuple(mv[592]) == (dx, dy)


def _fuzz_case(engine, oracle_lib, seed):
    from hmme import api, synth
    rng = np.random.default_rng(seed)
    w, h = 8 * int(rng.integers(1, 26)), 8 * int(rng.integers(1, 18))
    bd = int(rng.choice([8, 8, 10, 12, 9]))
    sr = int(rng.choice([1, 2, 3, 7, 16, 31, 64, 65, 90, 128]))
    fen = int(rng.integers(0, 2))
    n = api.load().hmme_num_ctus(w, h)
    if n * (2 * sr + 1) ** 2 > 6 * 129 * 129:     # keep the oracle's share of the run in seconds
        sr = 16
    max_pel = int(rng.choice([0, 4, 40, 300]))    # far predictors: windows clipped to slivers at the picture border
    pred = synth.random_predictors(n, seed=seed, max_pel=max_pel) if max_pel else None
    cur, ref, _ = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=min(sr, 10), region=32, noise_sigma=float(rng.choice([0.0, 2.0])))
    lam = float(rng.choice([0.0, 3.3, 57.9, 4000.0]))
    engine.set_lambda(lam)
    m = synth.MARGIN
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
        use_had = int(rng.integers(0, 2))
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred, use_hadamard=bool(use_had))
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, engine.lambda_q16, fen, bd, n_threads=8)
    tag = dict(seed=seed, w=w, h=h, bd=bd, sr=sr, fen=fen, max_pel=max_pel, lam=lam)
    assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy) and np.array_equal(sad, osad), tag
    table = oracle_lib.slot_table()
    ctus_x = (w + 63) // 64
    for k in range(int(os.environ.get("HMME_FUZZ_SLOTS", "12"))):
        ctu, s = int(rng.integers(0, n)), int(rng.integers(0, 593))
        cx, cy = (ctu % ctus_x) * 64, (ctu // ctus_x) * 64
        x, y, bw, bh = (int(v) for v in table[s])
        imv = (int(mv[ctu, s, 0]), int(mv[ctu, s, 1]))
        p = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        hx, hy, qx, qy, c = oracle_lib.frac_refine(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, p,
                                                    engine.lambda_q16, use_had, bd)
        got = (int(qmv[ctu, s, 0]), int(qmv[ctu, s, 1]), int(cost[ctu, s]))
        assert got == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (tag, ctu, s, use_had)


def test_fuzz_frames_vs_oracle(engine, oracle_lib):
    """random picture sizes (multiples of the 8-sample minimum CU), bit depths, search ranges 1..128, FEN, lambdas and
    predictors up to 300 pel away: integer search of every CTU and spot-checked refinement against the oracle"""
    n = int(os.environ.get("HMME_FUZZ_CASES", "14"))
    base = int(os.environ.get("HMME_FUZZ_SEED", "1000"))
    for i in range(n):
        _fuzz_case(engine, oracle_lib, base + i)


def test_fuzz_search_ctu_vs_oracle(engine, oracle_lib):
    """per-CTU call: random windows up to 257 x 257 (ragged, clipped, one candidate wide), every bit depth, FEN, lambdas,
    predictors, plain and bi-prediction origins (2*org - pred, outside the sample range)"""
    from hmme import api
    n = int(os.environ.get("HMME_FUZZ_CTU", "30"))
    rng = np.random.default_rng(int(os.environ.get("HMME_FUZZ_SEED", "1000")))
    for it in range(n):
        bd = int(rng.choice([8, 8, 9, 10, 12]))
        maxv = (1 << bd) - 1
        sr = int(rng.choice([1, 4, 4, 9, 33, 64, 100, 128]))
        lt = (-int(rng.integers(0, sr + 1)), -int(rng.integers(0, sr + 1)))
        rb = (int(rng.integers(0, sr + 1)), int(rng.integers(0, sr + 1)))
        if it % 7 == 0:
            lt, rb = (-sr, -sr), (sr, sr)
        wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
        ref = rng.integers(0, maxv + 1, size=(wy + 63 + 6, wx + 63 + 6)).astype(np.int16)
        o = (3 - lt[0], 3 - lt[1])
        dx, dy = int(rng.integers(lt[0], rb[0] + 1)), int(rng.integers(lt[1], rb[1] + 1))
        cur = ref[o[1] + dy:o[1] + dy + 64, o[0] + dx:o[0] + dx + 64].astype(np.int32)
        cur = cur + rng.integers(-3, 4, size=cur.shape)
        if it % 3 == 0:   # bi-prediction origin: 2 * org - other prediction, unclipped
            other = rng.integers(0, maxv + 1, size=cur.shape)
            cur = np.clip(2 * np.clip(cur, 0, maxv) - other, -maxv, 2 * maxv)
        else:
            cur = np.clip(cur, 0, maxv)
        cur = cur.astype(np.int16)
        pred = (int(rng.integers(-500, 501)), int(rng.integers(-500, 501)))
        fen = int(rng.integers(0, 2))
        lam = float(rng.choice([0.0, 4.7, 57.9, 2000.0]))
        engine.set_lambda(lam)
        p = api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, bd)
        mv, sad = engine.search_ctu(cur, (0, 0), ref, o, p)
        op = oracle_lib.make_params(lt, rb, pred, engine.lambda_q16, fen, bd)
        ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, o, op)
        tag = dict(it=it, bd=bd, lt=lt, rb=rb, pred=pred, fen=fen, lam=lam)
        assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad), tag


def test_upload_from_registered_host_memory(engine):
    """hmme_host_register page-locks the caller's picture buffer; uploads from it give the same plane"""
    from hmme import synth
    w, h, sr = 192, 128, 8
    cur, ref, _ = synth.make_pair(w, h, seed=5, max_mv=4)
    m = synth.MARGIN
    engine.set_lambda(57.9)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        want = engine.search_frame(pc, pr, sr)
        engine.host_register(cur); engine.host_register(ref)
        try:
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            got = engine.search_frame(pc, pr, sr)
        finally:
            engine.host_unregister(cur); engine.host_unregister(ref)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_contexts_are_independent_and_do_not_leak(oracle_lib):
    """two contexts used alternately (one per host thread / per stream is the documented model) give the same tables as one,
    and 25 create / use / destroy cycles leave the device memory where it was"""
    import threading
    import torch
    from hmme import api, synth
    w, h, sr = 256, 128, 16
    cur, ref, _ = synth.make_pair(w, h, seed=3, max_mv=8, region=64)
    m = synth.MARGIN

    def run(eng, out, key):
        eng.set_lambda(57.9)
        with eng.plane(w, h) as pc, eng.plane(w, h) as pr:
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            for _ in range(4):
                mv, sad = eng.search_frame(pc, pr, sr)
                q, c = eng.refine_frame(pc, pr, sr, mv)
                one = eng.search_ctu(cur, (m, m), ref, (m, m), api.SearchParams(-sr, -sr, sr, sr, 0, 0, 1, 8))
            out[key] = (mv, sad, q, c, one)

    with api.Engine(0, 64) as a, api.Engine(0, 64) as b:
        res = {}
        ts = [threading.Thread(target=run, args=(e, res, k)) for e, k in ((a, "a"), (b, "b"))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    assert set(res) == {"a", "b"}
    for x, y in zip(res["a"][:4], res["b"][:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(res["a"][4][0], res["b"][4][0]) and np.array_equal(res["a"][4][1], res["b"][4][1])
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, None, oracle_lib.oracle().hmo_lambda_q16(57.9), 1, 8, n_threads=4)
    assert np.array_equal(res["a"][0][:, :, 0], ox) and np.array_equal(res["a"][1], osad)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(25):
        with api.Engine(0, 128) as e:
            tmp = {}
            run(e, tmp, "x")
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 64 << 20, (free0, free1)


def test_2160p_10bit_sr128_whole_frame_properties_and_spot_checks(engine, oracle_lib):
    """BASELINE config 5 at full size (3840x2160 10-bit, SearchRange 128, FEN 1: the 16-bit kernel, window strips merged through
    global atomics): planted motion of up to 100 samples recovered wherever it is recoverable, idempotence, oracle equality on a
    CTU sample incl. the corners and the partial bottom row -- the 16-bit twin of the 8-bit 2160p test above"""
    from hmme import api, synth
    w, h, sr, bd = 3840, 2160, 128, 10
    cur, ref, true_mv = synth.make_pair(w, h, seed=510, bit_depth=bd, max_mv=100, region=256, noise_sigma=0.0)
    m = synth.MARGIN
    n_ctu = 60 * 34
    pred = synth.random_predictors(n_ctu, seed=510, max_pel=20)
    engine.set_lambda(238.5)
    lq = engine.lambda_q16
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred)
        mv2, sad2 = engine.search_frame(pc, pr, sr, pred)
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred, use_hadamard=True)
    assert mv.shape == (n_ctu, 593, 2) and np.array_equal(mv, mv2) and np.array_equal(sad, sad2)
    hits = far = 0
    for cy in range(1, 32):
        for cx in range(1, 59):
            if (cx % 4) in (0, 3) or (cy % 4) in (0, 3):                  # CTUs strictly inside one 256x256 region
                continue
            dx, dy = (int(v) for v in true_mv[cy // 4, cx // 4])
            ctu = cy * 60 + cx
            px, py = int(pred[ctu, 0]) >> 2, int(pred[ctu, 1]) >> 2
            lt_rb = api.set_search_range(int(pred[ctu, 0]), int(pred[ctu, 1]), sr, cx * 64, cy * 64, w, h)
            if lt_rb[0] <= dx <= lt_rb[2] and lt_rb[1] <= dy <= lt_rb[3] and 0 <= cx * 64 + dx and cx * 64 + 64 + dx <= w \
                    and 0 <= cy * 64 + dy and cy * 64 + 64 + dy <= h:      # planted MV inside the window and the block inside the picture
                assert sad[ctu, 592] == 0 and tuple(mv[ctu, 592]) == (dx, dy), (cx, cy, dx, dy)
                hits += 1
                far += max(abs(dx - px), abs(dy - py)) > 64                # beyond what SearchRange 64 could reach
    assert hits > 250 and far > 30
    # oracle equality on the first, the last (partial) and eight more CTU rows spread over the picture: 600 CTUs x 593 slots
    for row in (0, 3, 7, 11, 16, 20, 24, 28, 31, 33):
        ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, 1, bd, ctu_first=row * 60, ctu_count=60, n_threads=16)
        sl = slice(row * 60, row * 60 + 60)
        assert np.array_equal(mv[sl, :, 0], ox) and np.array_equal(mv[sl, :, 1], oy) and np.array_equal(sad[sl], osad), row
        if row in (0, 16, 33):       # the refinement of those winners on u16 planes (first-pass shift 2, clip to 1023, distortion >> 2)
            oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), w, h, mv[sl], pred, lq, 1, bd, ctu_first=row * 60, ctu_count=60, n_threads=16)
            assert np.array_equal(qmv[sl], oq) and np.array_equal(cost[sl], oc), row


def test_shift_free_and_int16_argument_checks(engine, oracle_lib):
    """hmme_search_params::shift_free (what cl/sad.cl computes on Pel of any width: no >> (bitDepth-8)) against
    the oracle's compat arithmetic; limits of the mode; window / predictor components beyond int16 are arguments errors, not
    device faults"""
    from hmme import api
    rng = np.random.default_rng(99)
    for bd, bipred in ((10, False), (9, True), (9, False), (8, True)):
        maxv = (1 << bd) - 1
        sr = 6
        side = 64 + 2 * sr + 8
        ref = rng.integers(0, maxv + 1, size=(side, side)).astype(np.int16)
        cur = rng.integers(0, maxv + 1, size=(64, 64))
        if bipred:
            cur = 2 * cur - rng.integers(0, maxv + 1, size=(64, 64))
        cur = cur.astype(np.int16)
        o = sr + 4
        engine.set_lambda(57.9)
        for fen in (0, 1):
            p = api.SearchParams(-sr, -sr, sr, sr - 1, 7, -9, fen, bd, 1)
            mv, sad = engine.search_ctu(cur, (0, 0), ref, (o, o), p)
            op = oracle_lib.make_params((-sr, -sr), (sr, sr - 1), (7, -9), engine.lambda_q16, fen, 8)   # depth 8 = no shift in the oracle
            ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), op)
            assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad), (bd, bipred, fen)
        shifted = engine.search_ctu(cur, (0, 0), ref, (o, o), api.SearchParams(-sr, -sr, sr, sr - 1, 7, -9, 0, bd, 0))[1]
        if bd > 8:
            assert int(shifted[592]) < int(sad[592])
    # beyond those widths the limit is the sample span of the call's own blocks (a 64x64 sum cannot exceed 4096 * span): 10-bit
    # bi-prediction origins and 12-bit content of moderate contrast are searched, bit-exact; a span that could reach the marker is refused
    for bd, lo_c, hi_c, lo_r, hi_r in ((10, -700, 1200, 40, 1000), (12, 1200, 2900, 1000, 2900), (11, -100, 1800, 0, 1830)):
        sr = 5
        side = 64 + 2 * sr + 8
        ref = rng.integers(lo_r, hi_r + 1, size=(side, side)).astype(np.int16)
        cur = rng.integers(lo_c, hi_c + 1, size=(64, 64)).astype(np.int16)
        cur[:8, :8] = ref[sr + 4 + 2:sr + 4 + 10, sr + 4 - 3:sr + 4 + 5]    # a few slots with a clear winner
        o = sr + 4
        for fen in (0, 1):
            mv, sad = engine.search_ctu(cur, (0, 0), ref, (o, o), api.SearchParams(-sr, -sr, sr, sr, -3, 5, fen, bd, 1))
            op = oracle_lib.make_params((-sr, -sr), (sr, sr), (-3, 5), engine.lambda_q16, fen, 8)
            ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), op)
            assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad), (bd, fen)
            assert int(sad[592]) > (1 << 20)
    cur = np.zeros((64, 64), np.int16)
    ref = np.zeros((100, 100), np.int16)
    engine.search_ctu(cur, (0, 0), ref, (18, 18), api.SearchParams(-8, -8, 8, 8, 0, 0, 0, 12, 1))       # span 0: nothing to refuse
    ref[40, 40] = 1938
    with pytest.raises(api.HmmeError, match="shift-free"):
        engine.search_ctu(cur, (0, 0), ref, (18, 18), api.SearchParams(-8, -8, 8, 8, 0, 0, 0, 12, 1))
    ref[40, 40] = 1937
    engine.search_ctu(cur, (0, 0), ref, (18, 18), api.SearchParams(-8, -8, 8, 8, 0, 0, 0, 12, 1))
    cur2 = cur.copy(); cur2[0, 0] = -1023; ref[40, 40] = 1000
    with pytest.raises(api.HmmeError, match="shift-free"):
        engine.search_ctu(cur2, (0, 0), ref, (18, 18), api.SearchParams(-8, -8, 8, 8, 0, 0, 0, 10, 1))
    for bad in (api.SearchParams(-8, -8, 8, 8, 40000, 0, 1, 8), api.SearchParams(-8, -8, 8, 8, 0, -40000, 1, 8),
                api.SearchParams(-40000, -8, -39990, 8, 0, 0, 1, 8), api.SearchParams(-8, 70000, 8, 70010, 0, 0, 1, 8)):
        with pytest.raises(api.HmmeError, match="int16"):
            engine.search_ctu(cur, (0, 0), ref, (18, 18), bad)


def test_bench_collective_path_under_torchrun_one_rank(tmp_path):
    """bench.py's N > 1 code path (process group, PipelinedGather, all_gather_object / all_reduce / barrier on RCCL, max-over-ranks) rehearsed
    with ONE rank on this one-GPU box: `torchrun --nproc-per-node 1` + HMME_BENCH_FORCE_DIST=1 (launcher started before any GPU call)"""
    import json
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HMME_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size", "1080p", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 100 and d["roofline"]["kernel_ms"] > 0
    assert d["config"]["collective"] == "gather to rank 0: grouped send/recv (nccl), world 1"
    m = d["multi_gpu"]
    assert m["ranks_seen"] == 1 and m["backend"] == "nccl" and m["crc32_tables_match_per_rank"] == [True] and len(m["devices"]) == 1
    assert m["devices"][0]["pci_bus_id"] and m["per_rank_kernel_ms"][0] > 0


def test_bench_starts_its_own_ranks_two_rank_rehearsal_on_one_gpu(tmp_path):
    """`python bench.py --gpus 2` exactly as a driver without a launcher invokes it: bench.py starts the two ranks itself (a child
    torch.distributed.run, before anything touches the GPU) and relays rank 0's line.  On this one-GPU box both ranks share cuda:0 and
    the tables travel over gloo (--share-gpu --backend gloo): a rehearsal of the code path, not a measurement.  The line must carry
    the evidence of a two-rank run: both ranks' devices and process ids, per-rank times, the gather's bytes, the per-rank CRC
    comparison (tables each rank computed == block rank 0 received) and rank 1's tables checked against the CPU oracle."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--backend", "gloo", "--steps", "3",
                        "--warmup", "1", "--size", "512x320", "--search-range", "16", "--full"], capture_output=True, text=True, timeout=900, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                      # ONE line on stdout, whatever the ranks and the launcher print
    d = json.loads(lines[0])
    n_ctu = 8 * 5
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["frames_per_step"] == 2 and d["scaling"] == "weak"
    m = d["multi_gpu"]
    assert m["ranks_seen"] == 2 and m["self_launched"] is True and m["shared_gpu_rehearsal"] is True and m["distinct_devices"] == 1
    assert [e["rank"] for e in m["devices"]] == [0, 1] and m["devices"][0]["pid"] != m["devices"][1]["pid"]
    assert m["crc32_tables_match_per_rank"] == [True, True]
    assert len(m["per_rank_kernel_ms"]) == 2 and min(m["per_rank_kernel_ms"]) > 0 and m["step_ms_min_max"][0] <= m["step_ms_min_max"][1]
    assert m["gather"]["bytes_received_by_rank0_per_step"] == 2 * n_ctu * 593 * 4           # rank 1's block, nothing else
    assert m["gather"]["bytes_received_in_timed_steps"] == 3 * 2 * n_ctu * 593 * 4
    assert m["verified_rank"]["rank"] == 1 and m["verified_rank"]["slots"] >= 593
    # the exchange switched off: the same steps, per rank, and the difference to the steps with the gather
    co, xc = m["compute_only"], m["exchange_cost"]
    assert len(co["per_rank_step_ms"]) == 2 and min(co["per_rank_kernel_ms"]) > 0 and co["ms_per_step"] > 0 and co["gsad_per_s"] > 0
    assert len(xc["per_rank_step_ms_delta"]) == 2 and len(xc["per_rank_kernel_ms_delta"]) == 2
    assert abs(xc["job_ms_per_step_delta"] - (d["ms_per_step"] - co["ms_per_step"])) < 2e-3
    # BASELINE config 4 as a sharded job: 124 pairs dealt p mod 2, gathered in pair order, CRCs per rank, a pair of rank 1 against the oracle
    c4 = d["configs"]["config4_sharded"]
    assert c4["pairs"] == 124 and c4["pair_counts"] == [62, 62] and c4["crc32_tables_match_per_rank"] == [True, True] and c4["scaling"] == "strong"
    assert c4["pairs_per_s"] > 0 and c4["one_gpu_same_run"]["pairs_per_s"] > 0 and c4["speedup_vs_one_gpu"] > 0 and len(c4["seconds_passes"]) == 3
    assert [e["pairs"] for e in c4["per_rank"]] == [62, 62]
    assert c4["verified"]["searched_by_rank"] == 1 and c4["verified"]["pair_index"] == 1 and c4["verified"]["slots"] >= 593
    assert c4["gathered_bytes"] == 62 * n_ctu * 593 * 8
    # the whole-job value counts both ranks' pictures
    assert abs(d["ctus_per_s"] - 2 * n_ctu * 3 / (d["ms_per_step"] * 3e-3)) / d["ctus_per_s"] < 0.01
    # without --share-gpu two ranks on a one-GPU box must refuse, not silently share the device
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "0",
                         "--size", "256x192", "--search-range", "8", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env,
                        cwd=str(tmp_path))
    assert r2.returncode != 0 and not [ln for ln in r2.stdout.splitlines() if ln.startswith("{")]
    assert "no GPU of its own" in r2.stderr


def test_bench_four_rank_rehearsal_deals_config4_raggedly(tmp_path):
    """`python bench.py --gpus 4 --share-gpu --backend gloo`: four ranks of one job on this one GPU.  124 pairs on 4 ranks are 31 each; the
    line carries compute_only / exchange_cost for four ranks and config4_sharded with the pair of rank 3 checked against the oracle"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--share-gpu", "--backend", "gloo", "--steps", "2",
                        "--warmup", "1", "--size", "256x192", "--search-range", "16", "--full"], capture_output=True, text=True, timeout=900, env=env,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    m = d["multi_gpu"]
    assert d["n_gpus"] == 4 and m["ranks_seen"] == 4 and m["crc32_tables_match_per_rank"] == [True] * 4
    assert len({e["pid"] for e in m["devices"]}) == 4 and len(m["compute_only"]["per_rank_step_ms"]) == 4
    assert m["verified_rank"]["rank"] == 3
    c4 = d["configs"]["config4_sharded"]
    assert c4["pair_counts"] == [31, 31, 31, 31] and c4["crc32_tables_match_per_rank"] == [True] * 4
    assert c4["verified"]["searched_by_rank"] == 3 and c4["ideal_speedup_at_this_deal"] == 4.0


def test_profiling_tooling_produces_a_counter_summary(tmp_path):
    """tools/profile_bench.sh + tools/summarize_profile.py -- the only way the counters behind roofline.traffic / valu_roofline are
    (re)generated -- on a small picture: rocprofv3 kernel trace + two --pmc passes of bench.py (never combined with other trace
    domains), a per-kernel summary with the derived figures, tied to the loaded library's build id; profiles/latest_pmc_* stay as they are."""
    import json
    import shutil
    import subprocess
    from conftest import ROOT
    from hmme import api
    if not shutil.which("rocprofv3"):
        pytest.skip("rocprofv3 not on PATH")
    before = {f: os.path.getmtime(os.path.join(ROOT, "profiles", f)) for f in os.listdir(os.path.join(ROOT, "profiles")) if f.startswith("latest_pmc_")}
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "profile_bench.sh"), "selftest", "quick"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    path = os.path.join(ROOT, "profiles", "selftest_pmc_summary_quick_512x320_sr16.json")
    d = json.load(open(path))
    k = d["kernels"]["me_search_kernel"]
    assert d["library_build_id"] == api.build_id() and k["valu_wave_instructions_per_launch"] > 1e5 and 0.001 < k["valu_busy_frac"] <= 1.0
    assert 0.005 < k["avg_waves_per_simd"] <= 2.01 and "me_frac_kernel" in d["kernels"]
    stats = os.path.join(ROOT, "profiles", "selftest_kernel_stats_quick_512x320_sr16.csv")
    assert "me_search_kernel" in open(stats).read()
    for f, t in before.items():
        assert os.path.getmtime(os.path.join(ROOT, "profiles", f)) == t
    for f in os.listdir(os.path.join(ROOT, "profiles")):     # scratch of this test, not evidence
        if f.startswith("selftest_"):
            os.remove(os.path.join(ROOT, "profiles", f))


def test_job_table_cache_is_invisible():
    """launches without predictors keep their job table for the next launch of the same geometry (hmme.hip TableTag): a sequence that
    revisits geometries, slips launches WITH predictors in between (they overwrite the table) and changes the CTU range gives, call
    by call, what a fresh context gives for that call alone -- search tables (8-bit whole jobs with a tail plan, 10-bit strips) and
    whole-picture refinement launches (2160p: 2 040 jobs; their workgroups derive their jobs themselves since round 5, a table is
    read only by the job-walking modes and under HMME_FRAC_JOB_TABLE=1, which test_refinement_launch_modes_give_the_same_tables runs)"""
    from hmme import api, synth
    m = synth.MARGIN

    def planes(eng, w, h, bd, seed):
        cur, ref, _ = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=6, region=64)
        pc, pr = eng.plane(w, h, bd), eng.plane(w, h, bd)
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        return pc, pr

    def call(eng, pl, sr, pred, first, count, refine):
        eng.set_lambda(57.9)
        mv, sad = eng.search_frame(pl[0], pl[1], sr, pred, ctu_first=first, ctu_count=count)
        if not refine:
            return mv, sad
        q, c = eng.refine_frame(pl[0], pl[1], sr, mv, pred) if (first, count) == (0, -1) else (mv, sad)
        return mv, sad, q, c

    geoms = {"A": (320, 192, 8, 16), "B": (256, 136, 10, 24), "C": (704, 576, 8, 64)}   # C: 99 jobs on 512 places -> all tail (split kernel + first-strip table)
    seq = [("A", None, 0, -1), ("A", None, 0, -1), ("A", "p", 0, -1), ("A", None, 0, -1), ("B", None, 0, -1), ("A", None, 0, -1), ("A", None, 2, 5),
           ("A", None, 0, -1), ("C", None, 0, -1), ("C", None, 0, -1), ("B", "p", 0, -1), ("B", None, 0, -1), ("C", "p", 0, -1), ("C", None, 0, -1)]
    eng = api.Engine(0, 128)
    held = {k: planes(eng, *g[:3], seed=40 + i) for i, (k, g) in enumerate(geoms.items())}
    for step, (k, pk, first, count) in enumerate(seq):
        w, h, bd, sr = geoms[k]
        n = api.load().hmme_num_ctus(w, h)
        pred = synth.random_predictors(n, seed=step, max_pel=6) if pk else None
        got = call(eng, held[k], sr, pred, first, count, True)
        fresh = api.Engine(0, 128)
        want = call(fresh, planes(fresh, w, h, bd, seed=40 + list(geoms).index(k)), sr, pred, first, count, True)
        fresh.close()
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (step, k, pk, first, count)
    # whole-picture refinement at 2160p, without / with / without predictors
    w, h, sr = 3840, 2160, 16
    big = planes(eng, w, h, 8, seed=77)
    n = api.load().hmme_num_ctus(w, h)
    mv, _ = eng.search_frame(big[0], big[1], sr)
    for step, pk in enumerate((None, None, "p", None)):
        pred = synth.random_predictors(n, seed=90 + step, max_pel=6) if pk else None
        q, c = eng.refine_frame(big[0], big[1], sr, mv, pred)
        other = api.Engine(0, 128)
        other.set_lambda(57.9)
        ob = planes(other, w, h, 8, seed=77)
        q1, c1 = other.refine_frame(ob[0], ob[1], sr, mv, pred)
        other.close()
        assert np.array_equal(q, q1) and np.array_equal(c, c1), (step, pk)
    eng.close()


def test_bench_n_rank_run_fails_loudly_when_a_rank_never_reaches_the_first_barrier(tmp_path):
    """An N-rank run first happens unattended (the driver's 8-GPU node).  A rank that hangs in front of its first barrier -- here rank 1 is
    made to sleep (HMME_BENCH_TEST_STALL) -- must not leave the job sitting in a collective: a rank's watchdog ends it after
    --rank-timeout with a line that names the rank and the stage, torch.distributed.run takes the rest down, bench.py's parent says which
    ranks never passed the barrier, prints no result line and exits non-zero.  The diagnostics of every rank (device count, device, RCCL /
    backend, ranks seen through the store) are on stderr before the first collective."""
    import subprocess
    import sys
    import time
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HMME_BENCH_TEST_STALL"] = "1:120"
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--backend", "gloo", "--steps", "1", "--warmup", "0",
                        "--size", "256x192", "--search-range", "8", "--no-cpu-baseline", "--rank-timeout", "20"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode != 0, r.stdout[-500:]
    assert time.time() - t0 < 110, "the stalled job was not ended by the watchdog"
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    # (both ranks' watchdogs run out at about the same time -- the sleeping rank's as well as the one waiting for it in the barrier --
    # and the launcher ends the other as soon as one has given up: either rank may be the one that is named)
    import re
    assert re.search(r"rank [01] of 2 did not get past '[a-z_ ()A-Z]+' within 20 s", r.stderr), r.stderr[-3000:]
    assert "ranks that never passed their first barrier: [0, 1]" in r.stderr, r.stderr[-3000:]
    assert "hipGetDeviceCount" in r.stderr and "ranks_seen 2 of 2" in r.stderr, r.stderr[-3000:]


def test_refinement_launch_modes_give_the_same_tables():
    """HMME_FRAC_GRID: one workgroup per job (the default, whole-frame == oracle elsewhere in this file), n workgroups that take job
    after job from the launch's counter, and as many of those as the chip holds -- the same tables, whoever evaluates a job"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    crcs = {}
    for grid in ("0", "7", "-1"):
        env = dict(os.environ, HMME_FRAC_GRID=grid)
        for bd in ("8", "10"):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "refine_rate.py"), "832x480", bd, "mixed"], capture_output=True, text=True,
                               timeout=600, env=env)
            assert r.returncode == 0, r.stderr[-1500:]
            crcs[(grid, bd)] = json.loads(r.stdout.strip().splitlines()[-1])["tables_crc32"]
    for bd in ("8", "10"):
        assert crcs[("0", bd)] == crcs[("7", bd)] == crcs[("-1", bd)], crcs
    assert crcs[("0", "8")] != crcs[("0", "10")]
    # HMME_FRAC_JOB_TABLE: the jobs read from a table that a kernel in front of the launch wrote (what the job-walking modes above do anyway)
    # instead of derived inside each workgroup -- the same tables
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "refine_rate.py"), "832x480", "8", "mixed"], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, HMME_FRAC_JOB_TABLE="1"))
    assert r.returncode == 0, r.stderr[-1500:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["tables_crc32"] == crcs[("0", "8")]


def test_weighted_and_bi_refinement_launch_modes_give_the_same_tables(oracle_lib):
    """The weighted and the bi-prediction refinement go through the launcher of the plain one (hmme.hip launch_refine), so the launch modes
    of the test above hold for them too -- tools/refine_modes.py, one process per mode (the knobs are read once per process): three pairs
    in one launch on 3 x 3 CTUs (168x136, search range 12, Hadamard, 8 and 10 bit); weights [A, A, B] with non-zero predictors (a run of
    two pairs, then a run of one: each run's job table and counter in the same buffer); bi with a motion field per 8x8 block and window
    centres.  HMME_FRAC_GRID=4 is fewer workgroups than the 9 jobs of the short run: every run walks.  The default mode's tables, computed
    here, are the oracle's: every CTU and slot of every pair (hmo_frac_refine_w per slot; the oracle's frame refinement of the origin
    2 * cur - prediction built in numpy)."""
    import importlib.util
    import json
    import subprocess
    import sys
    from conftest import ROOT
    from frame_helpers import bind_hmo, ctu_origin, oracle_prediction, origin_picture
    from hmme import synth
    tool = os.path.join(ROOT, "tools", "refine_modes.py")
    modes = {"default": {}, "grid 4": {"HMME_FRAC_GRID": "4"}, "grid -1": {"HMME_FRAC_GRID": "-1"}, "job table": {"HMME_FRAC_JOB_TABLE": "1"}}
    base = {k: v for k, v in os.environ.items() if k not in ("HMME_FRAC_GRID", "HMME_FRAC_JOB_TABLE")}
    crcs = {}
    for name, env in modes.items():
        r = subprocess.run([sys.executable, tool, "8", "10"], capture_output=True, text=True, timeout=600, env=dict(base, **env))
        assert r.returncode == 0, (name, r.stderr[-1500:])
        crcs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    for bd in ("8", "10"):
        for kind in ("weighted_crc32", "bi_crc32"):
            assert len({crcs[name][bd][kind] for name in modes}) == 1, (bd, kind, crcs)
    assert crcs["default"]["8"] != crcs["default"]["10"]

    # the default mode against the oracle (this process reads the knobs itself: it must be in the default mode too)
    assert "HMME_FRAC_GRID" not in os.environ and "HMME_FRAC_JOB_TABLE" not in os.environ
    spec = importlib.util.spec_from_file_location("refine_modes", tool)
    rm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rm)
    hmo = bind_hmo(oracle_lib)
    table = oracle_lib.slot_table()
    m, w, h = synth.MARGIN, rm.W, rm.H
    eng = rm.engine()
    try:
        for bd in (8, 10):
            r = rm.weighted(eng, bd)
            assert rm.crc(r) == crcs["default"][str(bd)]["weighted_crc32"]
            assert len({r["wps"][0], r["wps"][1]}) == 1 and r["wps"][2] != r["wps"][0]
            for i in range(3):
                cur, ref = r["curs"][i], r["refs"][i]
                for ctu in range(rm.N_CTU):
                    cx, cy = ctu_origin(ctu, w)
                    pq = (int(r["pred"][i, ctu, 0]), int(r["pred"][i, ctu, 1]))
                    for s in range(593):
                        x, y, bw, bh = (int(v) for v in table[s])
                        imv = (int(r["mv"][i, ctu, s, 0]), int(r["mv"][i, ctu, s, 1]))
                        hx, hy, qx, qy, c = oracle_lib.frac_refine_w(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, pq,
                                                                     eng.lambda_q16, 1, bd, r["wps"][i])
                        got = (int(r["qmv"][i, ctu, s, 0]), int(r["qmv"][i, ctu, s, 1]), int(r["cost"][i, ctu, s]))
                        assert got == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (bd, i, ctu, s)
            r = rm.bi(eng, bd)
            assert rm.crc(r) == crcs["default"][str(bd)]["bi_crc32"]
            for i in range(3):
                org = origin_picture(r["curs"][i], oracle_prediction(hmo, r["others"][i], w, h, bd, r["field"][i]), w, h)
                oq, oc = oracle_lib.refine_frame(np.ascontiguousarray(np.pad(org, m)), r["refs"][i], (m, m), w, h, r["mv"][i], r["pred"][i], eng.lambda_q16, 1,
                                                 bd, n_threads=8)
                assert np.array_equal(r["qmv"][i], oq), (bd, i, np.argwhere(r["qmv"][i] != oq)[:4])
                assert np.array_equal(r["cost"][i], oc), (bd, i, np.argwhere(r["cost"][i] != oc)[:4])
    finally:
        eng.close()


def test_sequence_driver_reads_a_yuv_file(tmp_path):
    """tools/me_sequence.py --yuv: the frame feeder (planar 8-bit 4:2:0 reader, hmme/yuv.py) in front of the sharded sequence
    search; the file holds a texture panning by (2, 1) per picture, which the 64x64 PUs must find"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    from hmme import synth, yuv
    w, h, n = 320, 192, 5
    pics = [synth.make_pair(w, h, seed=42, max_mv=0, noise_sigma=0.0, shift=(2 * t, t), pad=20, margin=0)[0].astype(np.uint8) for t in range(n)]
    path = str(tmp_path / "pan.yuv")
    yuv.write_luma_420(path, pics)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "me_sequence.py"), "--frames", str(n), "--gop", "lowdelay_P",
                        "--size", f"{w}x{h}", "--search-range", "16", "--yuv", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["gpus"] == 1 and d["first_pairs"][0] == [1, 0] and d["first_pairs"][1] == [2, 1]
    # picture t = texture shifted by (2t, t): cur(x) = ref(x + mv) with mv = (2, 1) * (cur - ref)
    assert d["median_mv_64x64_of_first_pairs"][0] == [2, 1] and d["median_mv_64x64_of_first_pairs"][2] == [4, 2]


def test_refine_ctu_matches_reference_goldens(engine):
    """hmme_refine_ctu == the reference's own TEncSearch::xPatternSearchFracDIF (tests/golden/frac.npz: 160 PUs of all shapes, 8/10 bit,
    Hadamard / SAD, generated from the compiled reference): per-CTU refinement at the caller's integer MVs"""
    from hmme import api
    d = np.load(os.path.join(GOLDEN, "frac.npz"))
    planes = {8: (np.ascontiguousarray(d["cur8"]), np.ascontiguousarray(d["ref8"])),
              10: (np.ascontiguousarray(d["cur10"]), np.ascontiguousarray(d["ref10"]))}
    n = 0
    for row, want in zip(d["rows"], d["out"]):
        slot, x, y, w, h, ix, iy, px, py, had, bd, lq, o = (int(v) for v in row)
        cur, ref = planes[bd]
        engine.set_lambda_q16(lq)
        imv = np.zeros((593, 2), np.int16)
        imv[slot] = (ix, iy)
        p = api.SearchParams(-8, -8, 8, 8, px, py, 1, bd)
        qmv, cost = engine.refine_ctu(cur, (o, o), ref, (o, o), p, imv, use_hadamard=bool(had))
        hx, hy, qx, qy, c = (int(v) for v in want)
        assert (int(qmv[slot, 0]), int(qmv[slot, 1]), int(cost[slot])) == (4 * ix + 2 * hx + qx, 4 * iy + 2 * hy + qy, c), row
        n += 1
    assert n == 160


def test_weighted_refine_ctu_matches_reference_goldens(engine):
    """hmme_refine_ctu_w == the reference's own xPatternSearchFracDIF with m_cDistParam.bApplyWeight (xGetHADsw / xGetSADw on the weighted
    interpolated prediction): tests/golden/frac_wp.npz, 112 PUs of all shapes on faded pictures, 8/10 bit, Hadamard / SAD, weights incl.
    a negative one and shift 0 -- straight through the C ABI, no oracle in between"""
    from hmme import api
    d = np.load(os.path.join(GOLDEN, "frac_wp.npz"))
    cols = d["columns"].tolist()
    n = refused = 0
    for row, want in zip(d["rows"], d["out"]):
        m = dict(zip(cols, (int(v) for v in row)))
        cur = np.ascontiguousarray(d["cur"][m["cur_index"]])
        ref = np.ascontiguousarray(d["ref8"] if m["bit_depth"] == 8 else d["ref10"])
        engine.set_lambda_q16(m["lambda_q16"])
        imv = np.zeros((593, 2), np.int16)
        imv[m["slot"]] = (m["int_x"], m["int_y"])
        o = m["origin"]
        p = api.SearchParams(-8, -8, 8, 8, m["pred_x"], m["pred_y"], 1, m["bit_depth"])
        wp = (m["wp_w"], m["wp_offset"], m["wp_shift"], m["wp_round"])
        try:
            qmv, cost = engine.refine_ctu_w(cur, (o, o), ref, (o, o), p, wp, imv, use_hadamard=bool(m["had"]))
        except api.HmmeError as e:      # the engine may refuse what it cannot keep exact (here: the whole CTU's sample span, not the PU's)
            assert "Hadamard sums" in str(e) or "Pel" in str(e) or "cost field" in str(e), str(e)
            refused += 1
            continue
        hx, hy, qx, qy, c = (int(v) for v in want)
        s_ = m["slot"]
        assert (int(qmv[s_, 0]), int(qmv[s_, 1]), int(cost[s_])) == (4 * m["int_x"] + 2 * hx + qx, 4 * m["int_y"] + 2 * hy + qy, c), m
        n += 1
    assert n >= 90 and refused <= 22, (n, refused)


@pytest.mark.parametrize("bd,sr,had", [(8, 16, 1), (8, 64, 0), (10, 24, 1), (8, 100, 1), (12, 128, 0)])
def test_search_refine_ctu_vs_oracle(engine, oracle_lib, bd, sr, had):
    """hmme_search_refine_ctu: one call = hmme_search_ctu (identical integer tables) + xPatternSearchFracDIF of the winners for all 593
    slots, on the block and window staged once (8-bit windows beyond 129 x 129 run as tiles, 9..12 bit on the 16-bit kernels)"""
    from hmme import api, synth
    w = h = 64 + 2 * sr + 16
    cur_p, ref_p, _ = synth.make_pair(w, h, seed=bd * 1000 + sr, bit_depth=bd, max_mv=min(sr, 20), region=48, noise_sigma=2.0, margin=0)
    o = sr + 8                                             # CTU origin: window + 4-sample halo + alignment slack stay inside the plane
    engine.set_lambda(57.9)
    pred = (13, -22)
    p = api.SearchParams(-sr, -sr, sr, sr - 1, pred[0], pred[1], 1, bd)
    mv, sad, qmv, cost = engine.search_refine_ctu(cur_p, (o, o), ref_p, (o, o), p, use_hadamard=bool(had))
    mv0, sad0 = engine.search_ctu(cur_p, (o, o), ref_p, (o, o), p)
    assert np.array_equal(mv, mv0) and np.array_equal(sad, sad0)
    ox, oy, osad = oracle_lib.search_ctu(cur_p, (o, o), ref_p, (o, o), oracle_lib.make_params((-sr, -sr), (sr, sr - 1), pred, engine.lambda_q16, 1, bd))
    assert np.array_equal(mv[:, 0], ox) and np.array_equal(mv[:, 1], oy) and np.array_equal(sad, osad)
    table = oracle_lib.slot_table()
    rng = np.random.default_rng(sr)
    for s in list(rng.choice(593, size=60, replace=False)) + [592, 588, 576, 0, 128, 256, 300, 384]:
        x, y, bw, bh = (int(v) for v in table[s])
        imv = (int(mv[s, 0]), int(mv[s, 1]))
        hx, hy, qx, qy, c = oracle_lib.frac_refine(cur_p, (o + x, o + y), ref_p, (o + x, o + y), bw, bh, imv, pred, engine.lambda_q16, had, bd)
        assert (int(qmv[s, 0]), int(qmv[s, 1]), int(cost[s])) == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (s, imv)
    # a bi-prediction origin (2*org - pred_other, samples outside the range) is refined too: every slot against the oracle
    rng2 = np.random.default_rng(bd + sr)
    maxv = (1 << bd) - 1
    near = np.clip(cur_p.astype(np.int32) + rng2.integers(-40, 41, size=cur_p.shape) * (1 << (bd - 8)), 0, maxv)
    cur2 = (2 * cur_p.astype(np.int32) - near).astype(np.int16)
    cur2[o + 3, o + 3], cur2[o + 40, o + 17] = -maxv, 2 * maxv
    assert cur2[o:o + 64, o:o + 64].min() < 0 and cur2[o:o + 64, o:o + 64].max() > maxv
    mv2, sad2, qmv2, cost2 = engine.search_refine_ctu(cur2, (o, o), ref_p, (o, o), p, use_hadamard=bool(had))
    ox, oy, osad = oracle_lib.search_ctu(cur2, (o, o), ref_p, (o, o), oracle_lib.make_params((-sr, -sr), (sr, sr - 1), pred, engine.lambda_q16, 1, bd))
    assert np.array_equal(mv2[:, 0], ox) and np.array_equal(mv2[:, 1], oy) and np.array_equal(sad2, osad)
    for s in range(0, 593, 7):
        x, y, bw, bh = (int(v) for v in table[s])
        imv = (int(mv2[s, 0]), int(mv2[s, 1]))
        hx, hy, qx, qy, c = oracle_lib.frac_refine(cur2, (o + x, o + y), ref_p, (o + x, o + y), bw, bh, imv, pred, engine.lambda_q16, had, bd)
        assert (int(qmv2[s, 0]), int(qmv2[s, 1]), int(cost2[s])) == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), ("bi-prediction origin", s, imv)
    cur3 = cur2.copy()
    cur3[o + 1, o + 1] = 2 * maxv + 1                                  # beyond what 2*org - pred can produce
    with pytest.raises(api.HmmeError, match="outside"):
        engine.search_refine_ctu(cur3, (o, o), ref_p, (o, o), p)


def test_refine_ctu_matches_reference_goldens_of_biprediction_origins(engine):
    """hmme_refine_ctu on bi-prediction origins == the reference's own xPatternSearchFracDIF(..., biPred = true) on 2*org - pred_other
    (tests/golden/frac_bipred.npz: 96 PUs, 8/10 bit, Hadamard / SAD, origins over the whole [-maxv, 2*maxv], from the compiled reference)"""
    from hmme import api
    d = np.load(os.path.join(GOLDEN, "frac_bipred.npz"))
    planes = {(bd, k): np.ascontiguousarray(d[f"org{bd}_{k}"]) for bd in (8, 10) for k in (0, 1)}
    refs = {bd: np.ascontiguousarray(d[f"ref{bd}"]) for bd in (8, 10)}
    n = n_out = 0
    for row, want in zip(d["rows"], d["out"]):
        slot, x, y, w, h, ix, iy, px, py, had, bd, lq, o, which = (int(v) for v in row)
        cur = planes[(bd, which)]
        blk = cur[o:o + 64, o:o + 64]
        n_out += int(blk.min() < 0 or blk.max() > (1 << bd) - 1)
        engine.set_lambda_q16(lq)
        imv = np.zeros((593, 2), np.int16)
        imv[slot] = (ix, iy)
        p = api.SearchParams(-8, -8, 8, 8, px, py, 1, bd)
        qmv, cost = engine.refine_ctu(cur, (o, o), refs[bd], (o, o), p, imv, use_hadamard=bool(had))
        hx, hy, qx, qy, c = (int(v) for v in want)
        assert (int(qmv[slot, 0]), int(qmv[slot, 1]), int(cost[slot])) == (4 * ix + 2 * hx + qx, 4 * iy + 2 * hy + qy, c), row
        n += 1
    assert n == 96 and n_out == 48      # plane 0 (unrelated other prediction): origins over the whole [-maxv, 2*maxv]; plane 1 (close prediction): in range


def test_device_border_extension_matches_reference_goldens(engine, oracle_lib):
    """me_fill_plane_kernel (= TComPicYuv::extendPicBorder) against the reference's own padded buffers (tests/golden/border.npz): the
    device plane is not readable through the C ABI, so the check goes through a search whose windows reach the outermost margin --
    cur = the picture, ref = the same picture: every clipped window of every CTU must give the oracle's tables on the REFERENCE's
    padded buffer, and SAD 0 at MV (0,0) for the 64x64 PU only if both planes were padded identically"""
    d = np.load(os.path.join(GOLDEN, "border.npz"))
    m = int(d["margin"])
    for i in range(int(d["n"])):
        img, padded = d[f"img{i}"], np.ascontiguousarray(d[f"out{i}"])
        h, w = img.shape
        bd = 10 if int(img.max()) > 255 else 8
        engine.set_lambda(4.7)
        with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
            pc.upload_pel(np.ascontiguousarray(img), (0, 0))      # un-padded picture in: the device extends the borders
            pr.upload_pel(np.ascontiguousarray(img), (0, 0))
            mv, sad = engine.search_frame(pc, pr, 64)
        ox, oy, osad = oracle_lib.search_frame(padded, padded, (m, m), w, h, 64, None, engine.lambda_q16, 1, bd, n_threads=4)
        assert np.array_equal(mv[:, :, 0], ox) and np.array_equal(mv[:, :, 1], oy) and np.array_equal(sad, osad), i
        assert (mv[:, 592] == 0).all() and (sad[:, 592] == 0).all()


def test_calls_of_one_context_spread_over_streams(engine, oracle_lib):
    """hmme.h "Streams": plane fills, searches and refinements of ONE context issued on different streams without any caller-side
    synchronisation between them -- the library's own events order the shared scratch and the plane contents.  Repeated with
    alternating pictures so that a search overtaking a fill, or two launches sharing a job table, would show as wrong tables."""
    import torch
    from hmme import api, synth
    w, h, sr = 256, 192, 20
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    pics = [synth.make_pair(w, h, seed=70 + k, max_mv=9, region=64) for k in range(2)]
    t_cur = [torch.from_numpy(np.ascontiguousarray(p[0][m:m + h, m:m + w].astype(np.uint8))).to(dev) for p in pics]
    t_ref = [torch.from_numpy(np.ascontiguousarray(p[1][m:m + h, m:m + w].astype(np.uint8))).to(dev) for p in pics]
    n_ctu = 4 * 3
    engine.set_lambda(57.9)
    want = [oracle_lib.search_frame(p[0], p[1], (m, m), w, h, sr, None, engine.lambda_q16, 1, 8, n_threads=4) for p in pics]
    s_fill, s_search, s_refine = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    fp = api.FrameParams(sr, 1, 8, 0, n_ctu)
    d_mv = [torch.zeros((n_ctu, 593, 2), dtype=torch.int16, device=dev) for _ in range(2)]
    d_sad = [torch.zeros((n_ctu, 593), dtype=torch.int32, device=dev) for _ in range(2)]
    d_q = torch.zeros((n_ctu, 593, 2), dtype=torch.int16, device=dev)
    d_c = torch.zeros((n_ctu, 593), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        for it in range(12):
            k = it & 1
            pc.set_device_u8(t_cur[k].data_ptr(), t_cur[k].stride(0), s_fill.cuda_stream)
            pr.set_device_u8(t_ref[k].data_ptr(), t_ref[k].stride(0), s_fill.cuda_stream)
            engine.search_frame_device(pc, pr, fp, None, d_mv[k].data_ptr(), d_sad[k].data_ptr(), s_search.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(s_search)
            s_refine.wait_event(ev)          # the caller's own buffer (d_mv) crosses streams: the caller's event
            engine.refine_frame_multi_device(pc, [pr], fp, None, d_mv[k].data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), s_refine.cuda_stream)
            s_refine.synchronize()
            # the next iteration refills the planes on s_fill while nothing else is pending: the refinement just finished reading them
            got_mv, got_sad = d_mv[k].cpu().numpy(), d_sad[k].cpu().numpy().astype(np.uint32)
            assert np.array_equal(got_mv[:, :, 0], want[k][0]) and np.array_equal(got_mv[:, :, 1], want[k][1]) and np.array_equal(got_sad, want[k][2]), it
            assert np.abs(d_q.cpu().numpy().astype(np.int32) - 4 * got_mv.astype(np.int32)).max() <= 3


@pytest.mark.gpu
@pytest.mark.parametrize("bd,sr,refs", [(8, 64, 1), (8, 16, 2), (10, 32, 1), (10, 64, 1), (10, 128, 1), (10, 24, 2)])
def test_tail_plan_pictures_whose_searches_do_not_fill_whole_rounds(engine, oracle_lib, bd, sr, refs):
    """1920x1200 is 570 CTU searches: one full round of 512 workgroups and a tail of 58, which the frame plan (hmme.hip FramePlan)
    deals in finer pieces -- 8-bit: a second launch through the split kernel with its own job numbering and output offset; 16-bit:
    more strips for the tail jobs inside the same launch; two references: 1 140 jobs, the tail crosses the reference boundary.
    Head and tail tables against the oracle on the CTU rows either side of job 512, the first row and the last"""
    from hmme import api, synth
    w, h = 1920, 1200
    cur, ref, _ = synth.make_pair(w, h, seed=1200 + bd + sr, bit_depth=bd, max_mv=min(sr, 24), region=128, noise_sigma=1.0)
    m = synth.MARGIN
    ref2 = np.pad(np.roll(ref[m:m + h, m:m + w], (3, -5), axis=(0, 1)), m, mode="edge")   # a second reference, borders extended like the first
    ctus_x, ctus_y = 30, 19
    n_ctu = ctus_x * ctus_y
    pred = synth.random_predictors(n_ctu * refs, seed=77, max_pel=12).reshape(refs, n_ctu, 2)
    engine.set_lambda(91.3)
    lq = engine.lambda_q16
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr, engine.plane(w, h, bd) as pr2:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m)); pr2.upload_pel(ref2, (m, m))
        if refs == 1:
            mv, sad = engine.search_frame(pc, pr, sr, pred[0])
            mv, sad = mv[None], sad[None]
        else:
            mv, sad = engine.search_frame_multi(pc, [pr, pr2], sr, pred)
    assert mv.shape == (refs, n_ctu, 593, 2)
    planes = [ref, ref2]
    for r in range(refs):
        for row in (0, 16, 17, 18):
            ox, oy, osad = oracle_lib.search_frame(cur, planes[r], (m, m), w, h, sr, pred[r], lq, 1, bd, ctu_first=row * ctus_x, ctu_count=ctus_x,
                                                   n_threads=16)
            sl = slice(row * ctus_x, (row + 1) * ctus_x)
            assert np.array_equal(mv[r, sl, :, 0], ox) and np.array_equal(mv[r, sl, :, 1], oy) and np.array_equal(sad[r, sl], osad), (r, row)


_TAIL_KNOB_HELPER = """
import sys, zlib, numpy as np
sys.path.insert(0, sys.argv[1])
from hmme import api, synth
w, h, sr, refs, out = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
cur, ref, _ = synth.make_pair(w, h, seed=4321, max_mv=min(sr, 12), region=96, noise_sigma=1.5)
m = synth.MARGIN
ref2 = np.pad(np.roll(ref[m:m + h, m:m + w], (2, -3), axis=(0, 1)), m, mode="edge")
n = api.load().hmme_num_ctus(w, h)
pred = synth.random_predictors(n * refs, seed=5, max_pel=sr).reshape(refs, n, 2)
with api.Engine(0, 64) as e:
    e.set_lambda(33.0)
    with e.plane(w, h) as pc, e.plane(w, h) as pr, e.plane(w, h) as pr2:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m)); pr2.upload_pel(ref2, (m, m))
        for fen in (1, 0):
            mv, sad = e.search_frame_multi(pc, [pr, pr2][:refs], sr, pred, fen=fen)
            np.savez(out + str(fen) + ".npz", mv=mv, sad=sad)
"""


@pytest.mark.parametrize("w,h,sr,refs", [(2560, 1440, 12, 1), (1344, 832, 16, 2), (1280, 720, 20, 1)])
def test_tail_launch_modes_give_the_same_tables_as_whole_jobs_and_the_oracle(tmp_path, oracle_lib, w, h, sr, refs):
    """a launch that does not fill whole rounds of workgroups: its tail as equal segments in ONE launch with the head (HMME_TAIL_LAUNCHES=1), as a
    second launch behind the head's whole jobs (=2), with another number of segments (HMME_TAIL_PARTS=3), and no tail plan at all
    (HMME_TAIL_PARTS=1: every job whole) -- 920 jobs = 512 + 408; two references of 273 = 512 + 34 (the tail inside the second
    reference's jobs); 240 jobs = all tail.  FEN on and off.  All five give identical tables, and those equal the oracle on CTU rows of head and tail"""
    import subprocess
    import sys
    from conftest import ROOT
    from hmme import synth
    modes = {"default": {}, "one": {"HMME_TAIL_LAUNCHES": "1"}, "two": {"HMME_TAIL_LAUNCHES": "2"}, "parts3": {"HMME_TAIL_PARTS": "3"}, "whole": {"HMME_TAIL_PARTS": "1"}}
    for name, env in modes.items():
        r = subprocess.run([sys.executable, "-c", _TAIL_KNOB_HELPER, os.path.join(ROOT, "hm-opencl_amd"), str(w), str(h), str(sr), str(refs), str(tmp_path / name)],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert r.returncode == 0, (name, r.stderr[-2000:])
    cur, ref, _ = synth.make_pair(w, h, seed=4321, max_mv=min(sr, 12), region=96, noise_sigma=1.5)
    m = synth.MARGIN
    ref2 = np.pad(np.roll(ref[m:m + h, m:m + w], (2, -3), axis=(0, 1)), m, mode="edge")
    ctus_x, ctus_y = (w + 63) // 64, (h + 63) // 64
    n = ctus_x * ctus_y
    pred = synth.random_predictors(n * refs, seed=5, max_pel=sr).reshape(refs, n, 2)
    lq = oracle_lib.oracle().hmo_lambda_q16(33.0)
    for fen in (1, 0):
        base = np.load(str(tmp_path / "whole") + f"{fen}.npz")
        for name in modes:
            d = np.load(str(tmp_path / name) + f"{fen}.npz")
            assert np.array_equal(d["mv"], base["mv"]) and np.array_equal(d["sad"], base["sad"]), (name, fen)
        mv, sad = base["mv"].reshape(refs, n, 593, 2), base["sad"].reshape(refs, n, 593)
        for r_, plane in enumerate([ref, ref2][:refs]):
            for row in sorted({0, ctus_y // 2, ctus_y - 1}):
                ox, oy, osad = oracle_lib.search_frame(cur, plane, (m, m), w, h, sr, pred[r_], lq, fen, 8, ctu_first=row * ctus_x, ctu_count=ctus_x, n_threads=16)
                sl = slice(row * ctus_x, (row + 1) * ctus_x)
                assert np.array_equal(mv[r_, sl, :, 0], ox) and np.array_equal(mv[r_, sl, :, 1], oy) and np.array_equal(sad[r_, sl], osad), (fen, r_, row)


def test_fuzz_pictures_with_a_tail_vs_oracle(engine, oracle_lib):
    """random pictures of 300..1 300 CTUs (more than one round of 512 workgroups, or nearly one): head and tail of the frame plan,
    8- and 10/12-bit, one or two references, small search ranges so that the oracle checks EVERY CTU in seconds"""
    from hmme import api, synth
    n_cases = int(os.environ.get("HMME_FUZZ_BIG", "3"))
    base = int(os.environ.get("HMME_FUZZ_SEED", "1000"))
    for case in range(n_cases):
        rng = np.random.default_rng(base + 7919 * case)
        while True:
            w, h = 8 * int(rng.integers(100, 400)), 8 * int(rng.integers(60, 220))
            n = api.load().hmme_num_ctus(w, h)
            if 300 <= n <= 1300:
                break
        bd = int(rng.choice([8, 8, 10, 12]))
        sr = int(rng.choice([3, 8, 12, 16]))
        refs = int(rng.choice([1, 1, 2]))
        fen = int(rng.integers(0, 2))
        cur, ref, _ = synth.make_pair(w, h, seed=base + case, bit_depth=bd, max_mv=min(sr, 10), region=64, noise_sigma=1.0)
        m = synth.MARGIN
        ref2 = np.pad(np.roll(ref[m:m + h, m:m + w], (-2, 4), axis=(0, 1)), m, mode="edge")
        pred = synth.random_predictors(n * refs, seed=base + case, max_pel=int(rng.choice([0, 6, 60]))).reshape(refs, n, 2)
        engine.set_lambda(float(rng.choice([3.3, 57.9, 400.0])))
        with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr, engine.plane(w, h, bd) as pr2:
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m)); pr2.upload_pel(ref2, (m, m))
            if refs == 1:
                mv, sad = engine.search_frame(pc, pr, sr, pred[0], fen=fen)
                mv, sad = mv[None], sad[None]
            else:
                mv, sad = engine.search_frame_multi(pc, [pr, pr2], sr, pred, fen=fen)
        tag = dict(case=case, w=w, h=h, n=n, bd=bd, sr=sr, refs=refs, fen=fen)
        for r in range(refs):
            ox, oy, osad = oracle_lib.search_frame(cur, (ref, ref2)[r], (m, m), w, h, sr, pred[r], engine.lambda_q16, fen, bd, n_threads=16)
            assert np.array_equal(mv[r, :, :, 0], ox) and np.array_equal(mv[r, :, :, 1], oy) and np.array_equal(sad[r], osad), (tag, r)
