"""The inputs of tests/test_gpu_range_edges.py, checked without a GPU: the boundary weights of tests/range_content.py really sit next to a
refusal of hmme_weight_check, its pictures really reach the sample differences the rule admits, and the CPU oracle -- the reference of the
GPU tests -- agrees there with int64 numpy restatements of the weighted SAD and of the luma interpolation (its own int / Pel arithmetic
must not wrap at inputs it has never seen)."""
import ctypes as C

import numpy as np
import pytest

import range_content as rc
from frame_helpers import bind_hmo, oracle_prediction, origin_picture, random_field

W, H = 136, 72          # the picture of the GPU tests: 3 x 2 CTUs, partial on the right, at the bottom and in the corner
BDS = (8, 9, 10, 11, 12)


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.build()
    return api


def all_boundaries(bd):
    """the boundary weights of search and refinement, each weight once"""
    seen = {}
    for refine in (0, 1):
        for b in rc.boundary_weights(bd, refine):
            seen.setdefault(b["wp"], b)
    return list(seen.values())


def test_every_boundary_weight_is_the_last_one_accepted(api):
    for bd in BDS:
        for refine in (0, 1):
            bs = rc.boundary_weights(bd, refine)
            assert [b["family"] for b in bs] == list(rc.FAMILIES)
            for b in bs:
                assert api.weight_check(bd, b["wp"], refine) == 0 and rc.failing(bd, b["wp"], refine) == (), (bd, refine, b)
                assert api.weight_check(bd, b["next"], refine) == -5 and rc.failing(bd, b["next"], refine) != (), (bd, refine, b)
                if refine:   # what the refinement takes, the search takes
                    assert api.weight_check(bd, b["wp"], 0) == 0


def test_the_restated_rule_is_the_rule(api):
    """rc.failing names the condition a boundary sits next to: it must refuse exactly what hmme_weight_check refuses.  And the two conditions
    no boundary can be found for ("pel", "span16") never refuse a weight the cost field accepts"""
    rng = np.random.default_rng(2024)
    n_refused = 0
    for _ in range(20000):
        bd = int(rng.integers(8, 13))
        shift = int(rng.integers(0, 16))
        gain = float(rng.choice([0.01, 0.5, 1, 2, 8, 40])) * float(rng.uniform(0.5, 1.5)) * (-1 if rng.integers(0, 4) == 0 else 1)
        w0 = int(round(gain * (1 << shift)))
        offset = int(rng.integers(-40000, 40001)) if rng.integers(0, 2) else int(rng.integers(-300, 301)) << (bd - 8)
        wp = (w0, offset, shift, (1 << (shift - 1)) if shift else 0)
        for refine in (0, 1):
            why = rc.failing(bd, wp, refine)
            assert (api.weight_check(bd, wp, refine) == 0) == (why == ()), (bd, wp, refine, why)
            if "pel" in why or "span16" in why:
                assert "cost" in why, (bd, wp, why)
                n_refused += 1
    assert n_refused > 500   # the sweep did reach them


def test_no_condition_is_skipped_silently(api):
    produced = {(bd, b["condition"]) for bd in BDS for refine in (0, 1) for b in rc.boundary_weights(bd, refine)}
    wanted = {(bd, c) for bd in BDS for c in rc.SEARCH_CONDITIONS + rc.REFINE_CONDITIONS}
    assert produced | set(rc.CANNOT_BIND) == wanted and not produced & set(rc.CANNOT_BIND)
    assert set(rc.CANNOT_BIND) == {(bd, c) for bd in BDS for c in ("pel", "span16")} | {(8, "hadamard"), (9, "hadamard")}
    assert len(produced) == 5 * 3 + 5 * 2 - len(rc.CANNOT_BIND) == 13
    # the search boundaries are the cost field's at every depth, the refinement meets both of its own conditions wherever they can bind
    for bd in BDS:
        assert {b["condition"] for b in rc.boundary_weights(bd, 0)} == {"cost"}
        want = {"fp32", "hadamard"} if bd >= 10 else {"fp32", "cost"}
        assert {b["condition"] for b in rc.boundary_weights(bd, 1)} == want
    # at 12 bit the refinement admits only weights that keep the weighted sample inside [0, 4095], the inverting weight among them
    inv = rc.boundary_weight(12, 1, "inverting")
    assert inv == (-64, 4095, 6, 32) and rc.span_of(12, inv) == 4095
    assert all(rc.span_of(12, b["wp"]) == 4095 for b in rc.boundary_weights(12, 1))
    # the largest span the cost field admits at each depth, from the rule as include/hmme.h states it: the search boundaries reach exactly it
    for bd in BDS:
        top = max(s for s in range(1 << 16) if ((4096 * s) >> (bd - 8)) + 65535 < 8000000)
        assert top == rc.COST_SPAN[bd] and top < 32767 and 2 * top <= 65535
        assert max(rc.span_of(bd, b["wp"]) for b in rc.boundary_weights(bd, 0)) == top


def block(plane, ctu, x=0, y=0, w=64, h=64, d=(0, 0)):
    from hmme import synth
    cx, cy = (ctu % 3) * 64, (ctu // 3) * 64
    m = synth.MARGIN
    return plane[m + cy + y + d[1]:m + cy + y + d[1] + h, m + cx + x + d[0]:m + cx + x + d[0] + w]


@pytest.mark.parametrize("bd", BDS)
def test_oracle_weighted_sad_equals_the_int64_restatement(api, oracle_lib, bd):
    """hmo_search_ctu_w and hmo_pattern_search_w over a window of ONE candidate return that candidate's SAD: slots 592 (64x64), 0 (the first
    8x4) and 576 (an AMP part), three displacements, a saturated CTU and a textured one, every boundary weight"""
    from hmme import synth
    table = oracle_lib.slot_table()
    m = synth.MARGIN
    lo_ctu, hi_ctu = rc.saturated_ctus(W, H)
    assert tuple(table[592]) == (0, 0, 64, 64) and tuple(table[0][2:]) in ((8, 4), (4, 8)) and table[576][2] != table[576][3]
    n = 0
    for b in all_boundaries(bd):
        wp = b["wp"]
        cur, ref, _ = rc.extreme_pair(W, H, bd, wp, seed=bd)
        for ctu in (lo_ctu, hi_ctu, 1):
            cx, cy = (ctu % 3) * 64, (ctu // 3) * 64
            for d in ((0, 0), (-3, 2), (8, -8)):
                p = oracle_lib.make_params(d, d, (0, 0), 3794534, 1, bd)
                _, _, osad = oracle_lib.search_ctu_w(cur, (m + cx, m + cy), ref, (m + cx, m + cy), p, wp)
                for s in (592, 0, 576):
                    x, y, bw, bh = (int(v) for v in table[s])
                    want = rc.sad_w(block(cur, ctu, x, y, bw, bh), block(ref, ctu, x, y, bw, bh, d), bd, wp)
                    assert int(osad[s]) == want, (bd, wp, ctu, d, s)
                    got = oracle_lib.pattern_search_w(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, p, wp)
                    assert got == (d[0], d[1], want), (bd, wp, ctu, d, s)
                    n += 1
    assert n >= 6 * 3 * 3 * 3


@pytest.mark.parametrize("bd", BDS)
def test_the_saturated_ctus_reach_the_admitted_span(api, bd):
    """conditions of the generator, not measurements: for every boundary weight one of the two flat CTUs has the 64x64 weighted SAD
    (4096 * span) >> (bd - 8), span recomputed here from the nominal range"""
    maxv = (1 << bd) - 1
    lo_ctu, hi_ctu = rc.saturated_ctus(W, H)
    for b in all_boundaries(bd):
        w0, offset, shift, rnd = b["wp"]
        ends = [((w0 * v + rnd) >> shift) + offset for v in (0, maxv)]
        span = max(maxv - min(ends), max(ends))
        assert span == rc.span_of(bd, b["wp"])
        cur, ref, true_mv = rc.extreme_pair(W, H, bd, b["wp"], seed=bd)
        assert set(np.unique(ref)) == {0, maxv} and cur.min() >= 0 and cur.max() <= maxv
        sads = [rc.sad_w(block(cur, c), block(ref, c), bd, b["wp"]) for c in (lo_ctu, hi_ctu)]
        assert max(sads) == (4096 * span) >> (bd - 8), (bd, b, sads)
        assert max(sads) + 65535 < rc.INV_COST16
        for c in (lo_ctu, hi_ctu):   # flat against flat, window included: every candidate of the search ties
            assert len(np.unique(block(cur, c))) == 1 and len(np.unique(block(ref, c, -8, -8, 80, 80))) == 1
        # most of the picture is the binary pattern, and the textured CTUs carry their displacement
        assert np.count_nonzero(true_mv.any(axis=1)) >= 2
    refb = rc.extreme_pair(W, H, bd, (64, 0, 6, 32), seed=bd)[1]
    inner = block(refb, 0, 0, 0, W, H)
    assert 0.35 < np.mean(inner[:64 - rc.FLAT_REACH] == maxv) < 0.65


@pytest.mark.parametrize("bd", BDS)
def test_the_bi_prediction_origin_reaches_both_extremes(oracle_lib, bd):
    hmo = bind_hmo(oracle_lib)
    maxv = (1 << bd) - 1
    lo_ctu, hi_ctu = rc.saturated_ctus(W, H)
    cur, ref, other = rc.extreme_triple(W, H, bd, seed=40 + bd)
    for per in (1, 64):
        field = random_field(6, per, 41 + bd + per)       # the field run_bi_search draws: MVs of up to 6 pels
        org = origin_picture(cur, oracle_prediction(hmo, other, W, H, bd, field), W, H)
        assert org.min() == -maxv and org.max() == 2 * maxv
        for ctu, v in ((lo_ctu, -maxv), (hi_ctu, 2 * maxv)):   # ... over the whole CTU
            cx, cy = (ctu % 3) * 64, (ctu // 3) * 64
            assert np.all(org[cy:cy + 64, cx:cx + 64] == v), (bd, per, ctu)
    assert set(np.unique(ref)) == {0, maxv} and set(np.unique(other)) == {0, maxv}


@pytest.mark.parametrize("bd", BDS)
def test_the_origin_of_several_references_reaches_both_extremes(oracle_lib, bd):
    """rc.extreme_lists at the size of the GPU case (128 x 64): whichever plane of the other list a block's index names, the origin is -maxv
    over the first 32 columns and 2 * maxv over the last 32; between them the two planes differ, so the index matters"""
    from bipred_refs_bands import refs_prediction
    hmo = bind_hmo(oracle_lib)
    maxv = (1 << bd) - 1
    w, h = 128, 64
    cur, refs, others = rc.extreme_lists(w, h, bd, seed=60 + bd)
    assert len(refs) == 2 and len(others) == 2 and all(set(np.unique(a)) == {0, maxv} for a in refs + others)
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(others[0], others[1])
    for per in (1, 64):
        field = random_field(2, per, 61 + bd + per)
        b = np.arange(per)
        by_index = []
        for ref_field in (np.zeros((2, per), np.uint8), np.ones((2, per), np.uint8), (((b % 8) + (b // 8)) % 2).astype(np.uint8)[None].repeat(2, axis=0)):
            org = origin_picture(cur, refs_prediction(hmo, others, w, h, bd, field, ref_field), w, h)
            assert np.all(org[:, :32] == -maxv) and np.all(org[:, -32:] == 2 * maxv) and org.min() == -maxv and org.max() == 2 * maxv
            by_index.append(org)
        assert len({o.tobytes() for o in by_index}) == (3 if per == 64 else 2)


@pytest.mark.parametrize("bd", [9, 11, 12])
def test_oracle_prediction_equals_the_int64_interpolation(oracle_lib, bd):
    """hmo_pred_block_qpel at the filter shifts only 9, 11 and 12 bit take (headroom 5, 3, 2), all 16 phases, on the binary pattern: the
    filter overshoots and the clip runs in both directions"""
    from hmme import synth
    hmo = bind_hmo(oracle_lib)
    maxv = (1 << bd) - 1
    m = synth.MARGIN
    _, ref, _ = rc.extreme_pair(W, H, bd, (64, 0, 6, 32), seed=70 + bd)
    p16 = C.POINTER(C.c_int16)
    out = np.zeros((64, 64), np.int16)
    clipped = 0
    for ph in range(16):
        qx, qy = 4 * (ph - 7) + (ph & 3), 4 * (5 - ph) + (ph >> 2)
        src = C.cast(ref.ctypes.data + 2 * ((m + 3) * ref.shape[1] + m + 5), p16)
        hmo.hmo_pred_block_qpel(src, ref.shape[1], 64, 64, qx, qy, bd, out.ctypes.data_as(p16), 64)
        want = rc.pred_qpel(ref, m + 5, m + 3, 64, 64, qx, qy, bd)
        assert np.array_equal(out, want), (bd, ph, np.argwhere(out != want)[:4])
        raw = rc.pred_qpel(ref, m + 5, m + 3, 64, 64, qx, qy, bd, clip=False)
        if ph:
            assert raw.min() < 0 and raw.max() > maxv, (bd, ph)
            clipped += 1
        else:
            assert np.array_equal(raw, ref[m + 3 + (qy >> 2):m + 67 + (qy >> 2), m + 5 + (qx >> 2):m + 69 + (qx >> 2)])
    assert clipped == 15
