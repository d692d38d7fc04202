"""The refusal rules of hmme_weight_check / hmme_bipred_check as tested contracts: at every bit depth 8..12 the accepted inputs nearest to each
refusal (tests/range_content.py finds them through hmme_weight_check) run on pictures of samples in {0, maxv} that reach the sample differences
the rule admits, and the engine must be bit-exact against the CPU oracle there -- weighted search and refinement, the prediction at the filter
shifts of 9, 11 and 12 bit, the bi-prediction search and refinement, single-reference and over several references per list (128 x 64).  tests/test_range_edges_cpu.py holds the oracle to int64 numpy on the
same inputs.  Pictures are 136 x 72 (3 x 2 CTUs, partial on the right, at the bottom and in the corner) unless a test says why not."""
import ctypes as C
import functools

import numpy as np
import pytest

import range_content as rc
from frame_helpers import bind_hmo, ctu_origin, device_tables, dims, mkplane, oracle_prediction, oracle_search_w, run_bi_search

pytestmark = pytest.mark.gpu

W, H, SR_W, SR_BI = 136, 72, 8, 4
N_CTU = 6
BDS = [8, 9, 10, 11, 12]
ERR_UNSUPPORTED = -5


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


@functools.lru_cache(maxsize=None)
def pictures(bd, wp):
    """one pair per (bit depth, weight), shared by the tests that use it; never written to"""
    cur, ref, _ = rc.extreme_pair(W, H, bd, wp, seed=1000 + bd)
    cur.setflags(write=False); ref.setflags(write=False)
    return cur, ref


def predictors(bd):
    from hmme import synth
    return synth.random_predictors(N_CTU, seed=50 + bd, max_pel=4)


def device_search_w(engine, bd, wp, fen):
    cur, ref = pictures(bd, wp)
    pc, pr = mkplane(engine, cur, W, H, bd), mkplane(engine, ref, W, H, bd)
    try:
        return engine.search_frame_w(pc, pr, SR_W, wp, predictors(bd), fen=fen)
    finally:
        pc.close(); pr.close()


# ---- 1: the weighted search at the search boundaries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("bd", BDS)
def test_weighted_search_at_every_bit_depth_and_boundary(engine, oracle_lib, bd, family):
    wp = rc.boundary_weight(bd, 0, family)
    cur, ref = pictures(bd, wp)
    mv, sad = device_search_w(engine, bd, wp, fen=1)   # FEN in the frame parameters: not consulted
    omv, osad = oracle_search_w(oracle_lib, cur, ref, W, H, SR_W, predictors(bd), engine.lambda_q16, bd, wp, range(N_CTU))
    print(f"bd {bd} {family} {wp}: largest SAD {int(sad.max())} (oracle {int(osad.max())}), admitted {(4096 * rc.span_of(bd, wp)) >> (bd - 8)}")
    assert np.array_equal(mv, omv), (bd, wp, [(int(c), int(s)) for c, s, _ in np.argwhere(mv != omv)[:4]])
    assert np.array_equal(sad, osad), (bd, wp, [(int(c), int(s), int(sad[c, s]), int(osad[c, s])) for c, s in np.argwhere(sad != osad)[:4]])
    # the cost field really was filled: a saturated CTU's 64x64 slot holds the largest sum the rule admits for this weight
    assert int(sad.max()) == (4096 * rc.span_of(bd, wp)) >> (bd - 8)
    assert int(sad.max()) == max(int(sad[c, 592]) for c in rc.saturated_ctus(W, H))


# ---- 2: the weighted refinement at the refinement boundaries -----------------------------------------------------------------------
@pytest.mark.parametrize("family", rc.FAMILIES)
@pytest.mark.parametrize("had", [1, 0])
@pytest.mark.parametrize("bd", BDS)
def test_weighted_refinement_at_every_bit_depth_and_boundary(engine, oracle_lib, bd, had, family):
    from hmme import synth
    wp = rc.boundary_weight(bd, 1, family)
    if bd == 12 and family == "inverting":
        assert wp == (-64, 4095, 6, 32) and rc.span_of(bd, wp) == 4095
    cur, ref = pictures(bd, wp)
    pred = predictors(bd)
    mv, _ = device_search_w(engine, bd, wp, fen=0)
    pc, pr = mkplane(engine, cur, W, H, bd), mkplane(engine, ref, W, H, bd)
    try:
        qmv, cost = engine.refine_frame_w(pc, pr, SR_W, wp, mv, pred, use_hadamard=bool(had))
    finally:
        pc.close(); pr.close()
    table = oracle_lib.slot_table()
    m = synth.MARGIN
    lo_ctu, hi_ctu = rc.saturated_ctus(W, H)     # 3 and 5: 5 is the corner CTU as well; 1 is textured
    assert (lo_ctu, hi_ctu) == (3, 5)
    for ctu in (lo_ctu, hi_ctu, 1):
        cx, cy = ctu_origin(ctu, W)
        pq = (int(pred[ctu, 0]), int(pred[ctu, 1]))
        for s in range(593):
            x, y, bw, bh = (int(v) for v in table[s])
            imv = (int(mv[ctu, s, 0]), int(mv[ctu, s, 1]))
            hx, hy, qx, qy, c = oracle_lib.frac_refine_w(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, pq,
                                                         engine.lambda_q16, had, bd, wp)
            got = (int(qmv[ctu, s, 0]), int(qmv[ctu, s, 1]), int(cost[ctu, s]))
            assert got == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (bd, had, wp, ctu, s)


# ---- 3: the weighted plane, through the SAD of the 64x64 slot ------------------------------------------------------------------------
@pytest.mark.parametrize("bd", BDS)
def test_weight_plane_against_numpy(engine, bd):
    """a reference that holds every sample value 0..maxv: the SAD returned for the 64x64 slot must be the int64 numpy SAD at the returned MV,
    for every search boundary weight -- no oracle in between, so an error the oracle shared would show"""
    from hmme import synth
    m = synth.MARGIN
    cur, ref = rc.ramp_pair(W, H, bd, seed=300 + bd)
    assert np.array_equal(np.unique(ref), np.arange(1 << bd))
    pc, pr = mkplane(engine, cur, W, H, bd), mkplane(engine, ref, W, H, bd)
    try:
        for b in rc.boundary_weights(bd, 0):
            wp = b["wp"]
            mv, sad = engine.search_frame_w(pc, pr, SR_W, wp, None, fen=1)
            for ctu in range(N_CTU):
                cx, cy = ctu_origin(ctu, W)
                dx, dy = int(mv[ctu, 592, 0]), int(mv[ctu, 592, 1])
                org = cur[m + cy:m + cy + 64, m + cx:m + cx + 64]
                want = rc.sad_w(org, ref[m + cy + dy:m + cy + dy + 64, m + cx + dx:m + cx + dx + 64], bd, wp)
                assert int(sad[ctu, 592]) == want, (bd, wp, ctu, (dx, dy))
    finally:
        pc.close(); pr.close()


# ---- 4: the prediction at the filter shifts of 9, 11 and 12 bit --------------------------------------------------------------------
@pytest.mark.parametrize("bd", [9, 11, 12])
@pytest.mark.parametrize("per", [1, 64])
def test_prediction_at_9_11_12_bit(engine, hmo, bd, per):
    """296 x 200 as in test_gpu_bipred_frame.py: one MV per CTU needs 16 CTUs for the 16 phases and four more for the MVs beyond clipMv"""
    from hmme import synth
    w, h = 296, 200
    cx_n, cy_n = dims(w, h)
    n_ctu = cx_n * cy_n
    maxv = (1 << bd) - 1
    m = synth.MARGIN
    rng = np.random.default_rng(7 + bd + per)
    ref = synth.pad_plane(np.where(rng.integers(0, 2, size=(h, w)) == 1, maxv, 0))
    field = np.zeros((n_ctu, per, 2), np.int16)
    beyond = {0: (-3000, -2999), 4: (3001, -1203), 12: (-32768, 32767), 19: (32767, 32766)}   # left / up, right, left / down, right / down
    inside = [c for c in range(n_ctu) if c not in beyond]
    for k, ctu in enumerate(inside):
        for b in range(per):
            ph = (k if per == 1 else b + ctu) % 16
            field[ctu, b] = (4 * int(rng.integers(-9, 10)) + (ph & 3), 4 * int(rng.integers(-9, 10)) + (ph >> 2))
    for ctu, mv in beyond.items():
        field[ctu, :] = mv
    assert {(int(x) & 3, int(y) & 3) for c in inside for x, y in field[c]} == {(a, b) for a in range(4) for b in range(4)}
    want = oracle_prediction(hmo, ref, w, h, bd, field)[:h, :w]
    pr = mkplane(engine, ref, w, h, bd)
    try:
        got = engine.predict_frame(pr, field if per == 64 else field[:, 0])
        assert got.dtype == np.uint16
        assert np.array_equal(got.astype(np.int16), want), (bd, per, np.argwhere(got.astype(np.int16) != want)[:4])
        # the clip ran in both directions, and it mattered: the unclipped filter gives other samples
        assert got.min() == 0 and got.max() == maxv
        ctu = inside[5]                                    # an interior CTU whose first MV has both fractions set
        x0, y0 = ctu_origin(ctu, w)
        raw = np.zeros((64, 64), np.int64)
        for b in range(per):
            bx, by, n = ((b & 7) * 8, (b >> 3) * 8, 8) if per == 64 else (0, 0, 64)
            qx, qy = (int(v) for v in field[ctu, b])
            raw[by:by + n, bx:bx + n] = rc.pred_qpel(ref, m + x0 + bx, m + y0 + by, n, n, qx, qy, bd, clip=False)
        assert field[ctu, 0, 0] & 3 and field[ctu, 0, 1] & 3
        assert np.array_equal(np.clip(raw, 0, maxv), got[y0:y0 + 64, x0:x0 + 64])
        assert np.any(raw < 0) and np.any(raw > maxv)
        if bd == 11:   # a CTU sub-range into an image full of a sentinel: its samples are written, nothing else is touched
            first, count = 3, 9
            img = np.full((h, w), 0xA5A5, np.uint16)
            engine.predict_frame(pr, field, out=img, ctu_first=first, ctu_count=count)
            written = np.zeros((h, w), bool)
            for c in range(first, first + count):
                x, y = ctu_origin(c, w)
                written[y:y + 64, x:x + 64] = True
            assert np.array_equal(img[written].astype(np.int16), want[written])
            assert np.all(img[~written] == 0xA5A5)
    finally:
        pr.close()


# ---- 5: the bi-prediction search on origins of -maxv and 2 * maxv -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def triple(bd):
    t = rc.extreme_triple(W, H, bd, seed=2000 + bd)
    for a in t:
        a.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def bi_search(engine, oracle_lib, hmo):
    """search_frame_bi against the oracle, all CTUs and slots, once per (bit depth, fen) for the search and the refinement test: one MV per 8x8 block
    at odd depths, one per CTU at even.  -> a function (bd, fen) -> what run_bi_search used and found"""
    done = {}

    def get(bd, fen):
        if (bd, fen) not in done:
            done[bd, fen] = run_bi_search(engine, oracle_lib, hmo, W, H, bd, SR_BI, fen, 64 if bd & 1 else 1, seed=2100 + bd, planes3=triple(bd))
        return done[bd, fen]
    return get


@pytest.mark.parametrize("fen", [0, 1])
@pytest.mark.parametrize("bd", BDS)
def test_bi_search_at_every_bit_depth(bi_search, bd, fen):
    maxv = (1 << bd) - 1
    r = bi_search(bd, fen)
    assert r["org"].min() == -maxv and r["org"].max() == 2 * maxv


# ---- 6: the bi-prediction refinement where it is served, its refusal where it is not ---------------------------------------------
@pytest.mark.parametrize("had", [1, 0])
@pytest.mark.parametrize("bd", BDS)
def test_bi_refinement_at_every_served_bit_depth(engine, oracle_lib, bi_search, bd, had):
    import torch
    from hmme import api, synth
    m = synth.MARGIN
    maxv = (1 << bd) - 1
    r = bi_search(bd, 1)   # the search leg and its comparison with the oracle: the fixture's, made once
    assert r["org"].min() == -maxv and r["org"].max() == 2 * maxv
    pc, pr, po = (mkplane(engine, r[k], W, H, bd) for k in ("cur", "ref", "other"))
    try:
        if bd < 12:
            assert api.bipred_check(bd, True) == 0
            qmv, cost = engine.refine_frame_bi(pc, pr, po, SR_BI, r["field"], r["mv"], center_q=r["center"], pred_q=r["pred"], use_hadamard=bool(had))
            org_padded = np.ascontiguousarray(np.pad(r["org"], m))   # the oracle's frame refinement takes both planes at one origin
            oqmv, ocost = oracle_lib.refine_frame(org_padded, r["ref"], (m, m), W, H, r["mv"], r["pred"], engine.lambda_q16, had, bd, n_threads=8)
            assert np.array_equal(qmv, oqmv), (bd, had, np.argwhere(qmv != oqmv)[:4])
            assert np.array_equal(cost, ocost), (bd, had, np.argwhere(cost != ocost)[:4])
            return
        # 12 bit: 4096 * 2 * maxv >= 2^24 -- refused with HMME_ERR_UNSUPPORTED, nothing launched
        assert api.bipred_check(12, True) == ERR_UNSUPPORTED and api.bipred_check(12, False) == 0
        dev = torch.device("cuda", 0)
        d_f = torch.from_numpy(np.ascontiguousarray(r["field"])).to(dev)
        d_imv = torch.from_numpy(r["mv"]).to(dev)
        t_q = torch.full((1, N_CTU, 593, 2), 0x5A5A, dtype=torch.int16, device=dev)
        t_c = torch.full((1, N_CTU, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        fp = api.FrameParams(SR_BI, 1, 12, 0, N_CTU)
        one = lambda p: (C.c_void_p * 1)(p.h)
        L = engine.L
        was = L.hmme_set_error_printing(engine.h, 0)
        try:
            torch.cuda.synchronize()
            rc_ = L.hmme_refine_pairs_bi_device(engine.h, one(pc), one(pr), one(po), 1, C.byref(fp), d_f.data_ptr(), int(r["field"].shape[1]), None, None,
                                                d_imv.data_ptr(), had, t_q.data_ptr(), t_c.data_ptr(), None)
        finally:
            L.hmme_set_error_printing(engine.h, was)
        torch.cuda.synchronize()
        assert rc_ == ERR_UNSUPPORTED
        assert bool((t_q == 0x5A5A).all()) and bool((t_c == 0x5A5A5A5A).all())
        with pytest.raises(api.HmmeError):
            engine.refine_frame_bi(pc, pr, po, SR_BI, r["field"], r["mv"], use_hadamard=bool(had))
    finally:
        pc.close(); pr.close(); po.close()


# ---- 6b: the bi pass over several references: the origin built from a field and a reference-index field -------------------------------
W_REFS, H_REFS, SR_REFS = 128, 64, 8


@functools.lru_cache(maxsize=None)
def lists(bd):
    cur, refs, others = rc.extreme_lists(W_REFS, H_REFS, bd, seed=2200 + bd)
    for a in [cur] + refs + others:
        a.setflags(write=False)
    return cur, refs, others


@pytest.fixture(scope="module")
def bi_refs_search(engine, hmo):
    """search_frame_bi_refs on rc.extreme_lists -- two references, two planes in the other list named block by block -- against the per-CTU
    search on the origin built here, all CTUs and slots, once per bit depth for the search and the refinement test; one MV per 8x8 block at
    odd depths, one per CTU at even -> a function bd -> what was used and found"""
    from bipred_refs_bands import refs_prediction
    from frame_helpers import origin_picture, random_field
    from test_gpu_bipred_refs import checkerboard, per_ctu, predictors as ref_predictors
    done = {}

    def get(bd):
        if bd not in done:
            from hmme import api, synth
            assert api.bipred_check(bd, False) == 0                             # the search is served at every depth 8..12
            maxv = (1 << bd) - 1
            cur, refs, others = lists(bd)
            per, n = 64 if bd & 1 else 1, 2
            field, ref_field = random_field(n, per, 2210 + bd), checkerboard(n, per, 2, W_REFS)
            pred, center = ref_predictors(2, n, 2220 + bd), ref_predictors(2, n, 2230 + bd)
            p_full = refs_prediction(hmo, others, W_REFS, H_REFS, bd, field, ref_field)
            org = origin_picture(cur, p_full, W_REFS, H_REFS)
            assert org.min() == -maxv and org.max() == 2 * maxv and set(ref_field.reshape(-1).tolist()) == {0, 1}
            m = synth.MARGIN                                                    # the current picture 0 where the other list's prediction is maxv, and the reverse
            assert (cur[m:m + H_REFS, m:m + 32] == 0).all() and (p_full[:, :32] == maxv).all()
            assert (cur[m:m + H_REFS, m + W_REFS - 32:m + W_REFS] == maxv).all() and (p_full[:, -32:] == 0).all()
            planes = [mkplane(engine, a, W_REFS, H_REFS, bd) for a in [cur] + refs + others]
            try:
                fen = (bd >> 1) & 1
                mv, sad = engine.search_frame_bi_refs(planes[0], planes[1:3], planes[3:], SR_REFS, field, ref_field, center_q=center, pred_q=pred, fen=fen)
            finally:
                for p in planes:
                    p.close()
            for r in range(2):
                smv, ssad = per_ctu(engine, org, refs[r], W_REFS, H_REFS, bd, SR_REFS, center[r], pred[r], fen, range(n))
                assert np.array_equal(mv[r], smv), (bd, r, np.argwhere(mv[r] != smv)[:4])
                assert np.array_equal(sad[r], ssad), (bd, r, np.argwhere(sad[r] != ssad)[:4])
            assert not np.array_equal(mv[0], mv[1])
            done[bd] = dict(org=org, field=field, ref_field=ref_field, pred=pred, center=center, mv=mv, fen=fen)
        return done[bd]
    return get


@pytest.mark.parametrize("bd", BDS)
def test_bi_refs_search_at_every_bit_depth(bi_refs_search, bd):
    maxv = (1 << bd) - 1
    r = bi_refs_search(bd)
    assert r["org"].min() == -maxv and r["org"].max() == 2 * maxv


@pytest.mark.parametrize("had", [1, 0])
@pytest.mark.parametrize("bd", BDS)
def test_bi_refs_refinement_at_every_served_bit_depth(engine, bi_refs_search, bd, had):
    import torch
    from hmme import api
    from test_gpu_bipred_refs import per_ctu
    r = bi_refs_search(bd)
    cur, refs, others = lists(bd)
    n = 2
    planes = [mkplane(engine, a, W_REFS, H_REFS, bd) for a in [cur] + refs + others]
    try:
        if api.bipred_check(bd, True) == 0:
            assert bd < 12
            qmv, cost = engine.refine_frame_bi_refs(planes[0], planes[1:3], planes[3:], SR_REFS, r["field"], r["ref_field"], r["mv"], center_q=r["center"],
                                                    pred_q=r["pred"], use_hadamard=bool(had))
            for k in range(2):
                sq, sc = per_ctu(engine, r["org"], refs[k], W_REFS, H_REFS, bd, SR_REFS, r["center"][k], r["pred"][k], r["fen"], range(n), r["mv"][k], bool(had))
                assert np.array_equal(qmv[k], sq), (bd, had, k, np.argwhere(qmv[k] != sq)[:4])
                assert np.array_equal(cost[k], sc), (bd, had, k, np.argwhere(cost[k] != sc)[:4])
            return
        # what hmme_bipred_check refuses the _refs call refuses: HMME_ERR_UNSUPPORTED, nothing launched
        assert bd == 12 and api.bipred_check(12, True) == ERR_UNSUPPORTED
        dev = torch.device("cuda", 0)
        d_f = torch.from_numpy(np.ascontiguousarray(r["field"])).to(dev)
        d_r = torch.from_numpy(np.ascontiguousarray(r["ref_field"])).to(dev)
        d_imv = torch.from_numpy(np.ascontiguousarray(r["mv"])).to(dev)
        t_q = torch.full((2, n, 593, 2), 0x5A5A, dtype=torch.int16, device=dev)
        t_c = torch.full((2, n, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        fp = api.FrameParams(SR_REFS, 1, 12, 0, n)
        L = engine.L
        was = L.hmme_set_error_printing(engine.h, 0)
        try:
            torch.cuda.synchronize()
            rc_ = L.hmme_refine_frame_bi_refs_device(engine.h, planes[0].h, api._handles(planes[1:3]), 2, api._handles(planes[3:]), 2, C.byref(fp), d_f.data_ptr(),
                                                     d_r.data_ptr(), int(r["field"].shape[1]), None, None, d_imv.data_ptr(), had, t_q.data_ptr(), t_c.data_ptr(), None)
        finally:
            L.hmme_set_error_printing(engine.h, was)
        torch.cuda.synchronize()
        assert rc_ == ERR_UNSUPPORTED
        assert bool((t_q == 0x5A5A).all()) and bool((t_c == 0x5A5A5A5A).all())
        with pytest.raises(api.HmmeError):
            engine.refine_frame_bi_refs(planes[0], planes[1:3], planes[3:], SR_REFS, r["field"], r["ref_field"], r["mv"], use_hadamard=bool(had))
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [9, 11, 12])
@pytest.mark.parametrize("per", [1, 64])
def test_prediction_of_a_b_picture_with_several_references_at_9_11_12_bit(engine, hmo, bd, per):
    """hmme_predict_bi_refs_frame on planes of samples in {0, maxv}, two per list, against predict_bi_refs_model: the average of two clipped
    predictions at the filter shifts of 9, 11 and 12 bit reaches both ends of the range"""
    import predict_bi_refs_model as pbrm
    from hmme import synth
    from test_gpu_predict_bi_refs import inputs
    maxv = (1 << bd) - 1
    rng = np.random.default_rng(2300 + bd)
    pics = [synth.pad_plane(rc._binary(rng, H, W, maxv)) for _ in range(4)]
    field, dirs, refs = inputs(W, H, per, 2310 + bd + per, 2, 2)
    fill = 0xA5A5
    want = pbrm.pred_picture(hmo, pics[:2], pics[2:], W, H, bd, field, dirs, refs, np.full((H, W), fill, np.int64))
    assert (want == 0).any() and (want == maxv).any() and (want == fill).any() == (per == 64)
    assert {int(d) for d in dirs.reshape(-1)} >= {1, 2, 3} and ((want != 0) & (want != maxv) & (want != fill)).any()
    planes = [mkplane(engine, a, W, H, bd) for a in pics]
    try:
        got = engine.predict_bi_refs_frame(planes[:2], planes[2:], field, dirs, refs, out=np.full((H, W), fill, np.uint16))
        assert got.dtype == np.uint16 and np.array_equal(got, want), (bd, per, np.argwhere(got != want)[:4])
    finally:
        for p in planes:
            p.close()


# ---- 7: bias and offset are per pair ---------------------------------------------------------------------------------------------
def test_three_boundary_pairs_in_one_launch(engine):
    """12 bit, three pairs with three different boundary weights (one the identity) in one search launch and one refinement launch: the
    tables of the three single-pair calls.  The weighted plane's offset and the bias of the current blocks differ from pair to pair by
    tens of thousands here; taking either from another pair cannot go unnoticed"""
    import torch
    from hmme import api
    bd = 12
    dev = torch.device("cuda", 0)
    ident = (64, 0, 6, 32)
    search_wps = [ident, rc.boundary_weight(bd, 0, "negative_offset"), rc.boundary_weight(bd, 0, "inverting")]
    refine_wps = [ident, rc.boundary_weight(bd, 1, "inverting"), rc.boundary_weight(bd, 1, "large_gain")]
    assert len(set(search_wps)) == 3 and len(set(refine_wps)) == 3
    assert rc.weigh(0, search_wps[1]) < -20000 and rc.weigh(0, search_wps[2]) > 20000     # bias > 0 in pair 1 only
    pred = np.stack([predictors(bd)] * 3)
    d_pred = torch.from_numpy(pred).to(dev)
    fp = api.FrameParams(SR_W, 1, bd, 0, N_CTU)
    for wps, refine in ((search_wps, False), (refine_wps, True)):
        pl = [(mkplane(engine, c, W, H, bd), mkplane(engine, r, W, H, bd)) for c, r in (pictures(bd, wp) for wp in wps)]
        try:
            curs, refs = [p[0] for p in pl], [p[1] for p in pl]
            d_mv, d_sad = device_tables(3, N_CTU, dev)
            engine.search_pairs_w_device(curs, refs, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
            torch.cuda.synchronize()
            mv, sad = d_mv.cpu().numpy(), d_sad.cpu().numpy().astype(np.uint32)
            for i in range(3):
                smv, ssad = engine.search_frame_w(curs[i], refs[i], SR_W, wps[i], pred[i])
                assert np.array_equal(mv[i], smv) and np.array_equal(sad[i], ssad), (i, wps[i])
            assert not np.array_equal(sad[0], sad[1]) and not np.array_equal(sad[1], sad[2]) and not np.array_equal(sad[0], sad[2])
            if not refine:
                continue
            d_q, d_c = device_tables(3, N_CTU, dev)
            for had in (1, 0):
                engine.refine_pairs_w_device(curs, refs, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), 0)
                torch.cuda.synchronize()
                qmv, cost = d_q.cpu().numpy(), d_c.cpu().numpy().astype(np.uint32)
                for i in range(3):
                    sq, sc = engine.refine_frame_w(curs[i], refs[i], SR_W, wps[i], mv[i], pred[i], use_hadamard=bool(had))
                    assert np.array_equal(qmv[i], sq) and np.array_equal(cost[i], sc), (had, i, wps[i])
        finally:
            for a, b in pl:
                a.close(); b.close()
