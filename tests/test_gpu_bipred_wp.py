"""Bi-prediction with explicit weighted prediction on whole pictures and picture pairs (hmme_predict_*_w, hmme_search_pairs_bi_w_device,
hmme_refine_pairs_bi_w_device, hmme_search_frame_bi_w, hmme_refine_frame_bi_w).  The other list's prediction and the origin come from the
numpy model tests/bipred_wp_model.py (pinned to the oracle's interpolation by tests/test_bipred_wp_cpu.py); on that origin the search is
compared with hmo_search_ctu_w and the refinement with hmo_frac_refine_w, every CTU and all 593 slots.  Every comparison is bit-exact, and
every weight is first accepted by hmme_bipred_weight_check on the host."""
import numpy as np
import pytest

import bipred_wp_model as model
import range_content as rc
from frame_helpers import bind_hmo, check_strided_image, device_tables, dims, mkplane, random_field, three_planes
from frame_helpers import oracle_origin_refine_w as oracle_refine, oracle_origin_search_w as oracle_search

pytestmark = pytest.mark.gpu

IDENT = model.IDENT
W, H = 136, 72          # 3 x 2 CTUs, partial on the right, at the bottom and in the corner
MV_SENT, COST_SENT = 0x5A5A, 0x5A5A5A5A


def scaled(wp, bd):
    """a weight written for 8 bits at bit depth bd: the offset scales with the samples"""
    return (wp[0], wp[1] << (bd - 8), wp[2], wp[3])


FADE = (40, -12, 5, 16)            # 40 / 32, offset -12
NEGATIVE = (-20, 200, 5, 16)       # a negative w0
BOTH_ENDS = (128, -300, 5, 16)     # gain 4: clips at 0 below 75 and at maxv above 138
BELOW_ZERO = (64, -300, 6, 32)     # the searched list's weighted samples go down to -300 << (bd - 8): bias above maxv


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


def accepted(bd, wp, owp, refine):
    from hmme import api
    assert api.bipred_weight_check(bd, wp, owp, refine) == 0, (bd, wp, owp, refine)


def run_case(engine, oracle_lib, hmo, w, h, bd, sr, wp, owp, per, seed, with_center=True, fen=0, planes3=None, had=None, field=None):
    """search_frame_bi_w (and, had = 0 | 1 or a tuple of both, refine_frame_bi_w per metric) on three pictures against the oracle on the
    model's origin, all CTUs and slots -> what was used and found"""
    from hmme import synth
    accepted(bd, wp, owp, 0)
    cx_n, cy_n = dims(w, h)
    n_ctu = cx_n * cy_n
    cur, ref, other = planes3 if planes3 is not None else three_planes(w, h, bd, seed)
    field = random_field(n_ctu, per, seed + 1) if field is None else field
    pred = synth.random_predictors(n_ctu, seed=seed + 2, max_pel=8)
    center = synth.random_predictors(n_ctu, seed=seed + 3, max_pel=8) if with_center else None
    if center is not None:
        assert np.any(center != pred)
    raw = model.pred_picture(hmo, other, w, h, bd, field, owp, clip=False)
    org = model.origin(cur, np.clip(raw, 0, (1 << bd) - 1), w, h)
    out = dict(cur=cur, ref=ref, other=other, field=field, pred=pred, center=center, org=org, raw=raw)
    pc, pr, po = (mkplane(engine, a, w, h, bd) for a in (cur, ref, other))
    try:
        mv, sad = engine.search_frame_bi_w(pc, pr, po, sr, wp, owp, field, center_q=center, pred_q=pred, fen=fen)
        omv, osad = oracle_search(oracle_lib, org, ref, w, h, sr, center, pred, engine.lambda_q16, bd, wp, range(n_ctu))
        assert np.array_equal(mv, omv), (bd, sr, wp, owp, np.argwhere(mv != omv)[:4])
        assert np.array_equal(sad, osad), (bd, sr, wp, owp, np.argwhere(sad != osad)[:4])
        out.update(mv=mv, sad=sad)
        for had in (() if had is None else had if isinstance(had, tuple) else (had,)):
            accepted(bd, wp, owp, 1)
            qmv, cost = engine.refine_frame_bi_w(pc, pr, po, sr, wp, owp, field, mv, center_q=center, pred_q=pred, use_hadamard=bool(had))
            oqmv, ocost = oracle_refine(oracle_lib, org, ref, w, h, mv, pred, engine.lambda_q16, had, bd, wp, range(n_ctu))
            assert np.array_equal(qmv, oqmv), (bd, had, wp, owp, np.argwhere(qmv != oqmv)[:4])
            assert np.array_equal(cost, ocost), (bd, had, wp, owp, np.argwhere(cost != ocost)[:4])
            out.update(qmv=qmv, cost=cost)
    finally:
        pc.close(); pr.close(); po.close()
    return out


# ---- 1: the prediction against the model ---------------------------------------------------------------------------------------------------
def phase_fields(n_ctu, per, seed):
    """fields that together carry all 16 fractional phases and MVs beyond what clipMv allows, in every direction and at the ends of int16"""
    rng = np.random.default_rng(seed)
    fields = []
    for k in range(3 if per == 1 else 1):
        f = np.zeros((n_ctu, per, 2), np.int16)
        for ctu in range(n_ctu):
            for b in range(per):
                ph = (k * n_ctu + ctu if per == 1 else b + ctu) % 16
                f[ctu, b] = (4 * int(rng.integers(-9, 10)) + (ph & 3), 4 * int(rng.integers(-9, 10)) + (ph >> 2))
        fields.append(f)
    assert len({(int(x) & 3, int(y) & 3) for f in fields for c in range(n_ctu) for x, y in f[c]}) == 16
    beyond = np.zeros((n_ctu, per, 2), np.int16)
    for ctu, mv in enumerate(((-3000, -2999), (3001, -1203), (-32768, 32767), (32767, 32766), (-1203, 3001), (2999, 3000))):
        beyond[ctu, :] = mv
    return fields + [beyond]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("per", [1, 64])
def test_weighted_prediction_equals_the_model(engine, hmo, bd, per):
    from hmme import api, synth
    cx_n, cy_n = dims(W, H)
    n_ctu = cx_n * cy_n
    maxv = (1 << bd) - 1
    _, ref, _ = synth.make_pair(W, H, seed=21 + bd, bit_depth=bd, max_mv=4, region=64)
    fields = phase_fields(n_ctu, per, 7 + bd + per)
    # the last field's MVs really lie beyond the clip range of their CTUs
    from frame_helpers import clip_mv
    assert all(clip_mv(hmo, *fields[-1][c, 0], (c % cx_n) * 64, (c // cx_n) * 64, W, H) != tuple(int(v) for v in fields[-1][c, 0]) for c in range(n_ctu))
    weights = [IDENT, scaled(FADE, bd), scaled(NEGATIVE, bd), scaled(BOTH_ENDS, bd)]
    pr = mkplane(engine, ref, W, H, bd)
    try:
        for wp in weights:
            accepted(bd, IDENT, wp, 0)
            for f in fields:
                raw = model.pred_picture(hmo, ref, W, H, bd, f, wp, clip=False)[:H, :W]
                want = np.clip(raw, 0, maxv)
                got = engine.predict_frame_w(pr, wp, f if per == 64 else f[:, 0])
                assert got.dtype == (np.uint8 if bd == 8 else np.uint16)
                assert np.array_equal(got.astype(np.int64), want), (wp, np.argwhere(got.astype(np.int64) != want)[:4])
                if wp == IDENT:   # ... which is the unweighted prediction
                    assert np.array_equal(got, engine.predict_frame(pr, f))
                if wp == scaled(BOTH_ENDS, bd) and f is not fields[-1]:   # the clip runs at both ends (the last field reads the flat margins)
                    assert raw.min() < 0 and raw.max() > maxv
                if wp == scaled(NEGATIVE, bd):    # brighter reference, darker prediction
                    assert wp[0] < 0 and want.min() < want.max()
        # a CTU sub-range into an image full of a sentinel: its samples are written, nothing else is touched
        wp, f = scaled(FADE, bd), fields[0]
        want = np.clip(model.pred_picture(hmo, ref, W, H, bd, f, wp)[:H, :W], 0, maxv)
        sentinel = 0xA5 if bd == 8 else 0xA5A5
        first, count = 1, 3
        img = np.full((H, W), sentinel, np.uint8 if bd == 8 else np.uint16)
        engine.predict_frame_w(pr, wp, f, out=img, ctu_first=first, ctu_count=count)
        inside = np.zeros((H, W), bool)
        for ctu in range(first, first + count):
            x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
            inside[y:y + 64, x:x + 64] = True
        assert np.array_equal(img[inside].astype(np.int64), want[inside]) and np.all(img[~inside] == sentinel)
        # ... and into an image whose stride exceeds the width
        import ctypes as C
        cw = api.Weight(*wp)
        check_strided_image(W, H, bd, lambda out, first, count: engine.predict_frame_w(pr, wp, f, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_frame_w(engine.h, pr.h, C.byref(fp), C.byref(cw), f.ctypes.data, per, out, stride))
        # two pictures with two weights in one launch == one at a time
        import torch
        dev = torch.device("cuda", 0)
        f64 = np.stack([np.repeat(fields[0], 64 // per, axis=1), np.repeat(fields[1 if per == 1 else 0], 64 // per, axis=1)])
        d_f = torch.from_numpy(f64).to(dev)
        tdt = torch.uint8 if bd == 8 else torch.int16
        imgs = [torch.zeros((H, W), dtype=tdt, device=dev) for _ in range(2)]
        fp = api.FrameParams(1, 0, bd, 0, n_ctu)
        engine.predict_pairs_w_device([pr, pr], fp, [scaled(FADE, bd), scaled(BOTH_ENDS, bd)], d_f.data_ptr(), 64, [t.data_ptr() for t in imgs],
                                      W * (1 if bd == 8 else 2), 0)
        torch.cuda.synchronize()
        for t, wp, f in zip(imgs, (scaled(FADE, bd), scaled(BOTH_ENDS, bd)), f64):
            assert np.array_equal(t.cpu().numpy().view(np.uint8 if bd == 8 else np.uint16), engine.predict_frame_w(pr, wp, f))
    finally:
        pr.close()


# ---- 2, 3: search and refinement against the oracle, all 593 slots of every CTU ----------------------------------------------------------------
CASES = {   # name: (searched weight, other weight), both written for 8 bits
    "both": (FADE, (48, 9, 5, 16)),
    "searched_identity": (IDENT, BOTH_ENDS),
    "other_identity": ((-40, 230, 6, 32), (1, 0, 0, 0)),
    "below_zero": (BELOW_ZERO, FADE),
}


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("w,h,sr", [(W, H, 12), (64, 64, 4), (W, H, 4)])
@pytest.mark.parametrize("had", [1, 0])
def test_bi_search_and_refinement_equal_the_oracle(engine, oracle_lib, hmo, bd, case, w, h, sr, had):
    """every case on every shape, the refinement of the search's winners with Hadamard and with SAD"""
    wp, owp = (scaled(v, bd) for v in CASES[case])
    maxv = (1 << bd) - 1
    k = list(CASES).index(case)
    per = 64 if (k + sr // 4 + bd // 2) % 2 else 1
    with_center = not (case == "both" and sr == 4 and w == W)       # one shape of one case: a null centre
    r = run_case(engine, oracle_lib, hmo, w, h, bd, sr, wp, owp, per, seed=2000 + 7 * sr + 13 * k + bd + w, with_center=with_center, fen=1, had=had)
    # the input does what the case is about
    wlo, whi, bias, span, _, _ = model.searched_terms(bd, wp)
    if case == "below_zero":
        assert wlo < -maxv and bias == -wlo > maxv and rc.weigh(r["ref"], wp).min() < 0   # the weighted samples do go negative
    if case == "searched_identity":
        assert r["raw"].min() < 0 and r["raw"].max() > maxv          # the other list's prediction clips at both ends
    ref = r["ref"].astype(np.int64)
    wref = rc.weigh(ref, wp)
    unweighted = model.pred_picture(hmo, r["other"], w, h, bd, r["field"], IDENT)
    if case == "both":      # both weights change samples: the origin is not the unweighted one, the priced reference not the raw one
        assert np.any(np.clip(r["raw"], 0, maxv) != unweighted) and np.any(wref != ref)
        assert not np.array_equal(r["org"], model.origin(r["cur"], unweighted, w, h))
    if case == "searched_identity":
        assert np.array_equal(wref, ref)
    if case == "other_identity":   # the origin is the unweighted one; the searched weight inverts: the darkest sample weighs most
        assert np.array_equal(np.clip(r["raw"], 0, maxv), unweighted) and wp[0] < 0 and bias == maxv
        assert wref.max() == rc.weigh(ref.min(), wp) > rc.weigh(ref.max(), wp) == wref.min()


@pytest.mark.parametrize("bd", [8, 10])
def test_fen_is_not_consulted(engine, oracle_lib, hmo, bd):
    wp, owp = (scaled(v, bd) for v in CASES["both"])
    a = run_case(engine, oracle_lib, hmo, 64, 64, bd, 4, wp, owp, 1, seed=2300 + bd, fen=0)
    b = run_case(engine, oracle_lib, hmo, 64, 64, bd, 4, wp, owp, 1, seed=2300 + bd, fen=1)
    assert np.array_equal(a["mv"], b["mv"]) and np.array_equal(a["sad"], b["sad"])


# ---- 4: batching ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_three_pairs_three_weight_pairs_in_one_launch(engine, oracle_lib, hmo, bd):
    import torch
    from hmme import api, synth
    sr = 4
    cx_n, cy_n = dims(W, H)
    n_ctu = cx_n * cy_n
    dev = torch.device("cuda", 0)
    wps = [scaled(FADE, bd), IDENT, scaled(BELOW_ZERO, bd)]
    owps = [scaled(BOTH_ENDS, bd), (1, 0, 0, 0), IDENT]            # the second pair: every weight the identity
    for a, b in zip(wps, owps):
        accepted(bd, a, b, 1)
    cur, r0, r1 = three_planes(W, H, bd, seed=2400 + bd)
    cur2, r2, o2 = three_planes(W, H, bd, seed=2500 + bd)
    planes = [mkplane(engine, a, W, H, bd) for a in (cur, r0, r1, cur2, r2, o2)]
    pc, p0, p1, pc2, p2, po2 = planes
    host = [(cur, r0, r1), (cur, r1, r0), (cur2, r2, o2)]
    try:
        f64 = np.stack([random_field(n_ctu, 64, 2410 + i + bd) for i in range(3)])
        pred = np.stack([synth.random_predictors(n_ctu, seed=2420 + i, max_pel=6) for i in range(3)])
        center = np.stack([synth.random_predictors(n_ctu, seed=2430 + i, max_pel=6) for i in range(3)])
        curs, refs, others = [pc, pc, pc2], [p0, p1, p2], [p1, p0, po2]
        d_f, d_pred, d_center = (torch.from_numpy(a).to(dev) for a in (f64, pred, center))
        full = {}
        for first, count in ((0, n_ctu), (2, 3)):
            fp = api.FrameParams(sr, 1, bd, first, count)
            # tables one CTU longer than the launch writes: the tail keeps its sentinels
            d_mv = torch.full((3 * count + 1, 593, 2), MV_SENT, dtype=torch.int16, device=dev)
            d_sad = torch.full((3 * count + 1, 593), COST_SENT, dtype=torch.int32, device=dev)
            d_q, d_c = torch.full_like(d_mv, MV_SENT), torch.full_like(d_sad, COST_SENT)
            engine.search_pairs_bi_w_device(curs, refs, others, fp, wps, owps, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(),
                                            d_sad.data_ptr(), 0)
            engine.refine_pairs_bi_w_device(curs, refs, others, fp, wps, owps, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), 1,
                                            d_q.data_ptr(), d_c.data_ptr(), 0)
            torch.cuda.synchronize()
            for t, sent in ((d_mv, MV_SENT), (d_q, MV_SENT), (d_sad, COST_SENT), (d_c, COST_SENT)):
                assert bool((t[3 * count] == sent).all()) and not bool((t[:3 * count, 0] == sent).all())
            mv, qmv = (t[:3 * count].cpu().numpy().reshape(3, count, 593, 2) for t in (d_mv, d_q))
            sad, cost = (t[:3 * count].cpu().numpy().astype(np.uint32).reshape(3, count, 593) for t in (d_sad, d_c))
            if first == 0:
                full = dict(mv=mv, sad=sad, qmv=qmv, cost=cost)
                for i, (hc, hr, ho) in enumerate(host):   # the search of every pair against the oracle
                    org = model.origin(hc, model.pred_picture(hmo, ho, W, H, bd, f64[i], owps[i]), W, H)
                    omv, osad = oracle_search(oracle_lib, org, hr, W, H, sr, center[i], pred[i], engine.lambda_q16, bd, wps[i], range(n_ctu))
                    assert np.array_equal(mv[i], omv) and np.array_equal(sad[i], osad), i
            else:   # a CTU sub-range == the same rows of the full call
                for k, a in (("mv", mv), ("sad", sad), ("qmv", qmv), ("cost", cost)):
                    assert np.array_equal(a, full[k][:, first:first + count]), k
            for i in range(3):   # == the three single calls (refinement: pinned to the oracle by the single-pair tests)
                smv, ssad = engine.search_frame_bi_w(curs[i], refs[i], others[i], sr, wps[i], owps[i], f64[i], center_q=center[i], pred_q=pred[i],
                                                     ctu_first=first, ctu_count=count)
                assert np.array_equal(mv[i], smv) and np.array_equal(sad[i], ssad), (first, i)
                sq, sc = engine.refine_frame_bi_w(curs[i], refs[i], others[i], sr, wps[i], owps[i], f64[i], smv, center_q=center[i], pred_q=pred[i],
                                                  ctu_first=first, ctu_count=count)
                assert np.array_equal(qmv[i], sq) and np.array_equal(cost[i], sc), (first, i)
        # the all-identity pair inside the mixed launch == the unweighted call without FEN
        umv, usad = engine.search_frame_bi(curs[1], refs[1], others[1], sr, f64[1], center_q=center[1], pred_q=pred[1], fen=0)
        uq, uc = engine.refine_frame_bi(curs[1], refs[1], others[1], sr, f64[1], umv, center_q=center[1], pred_q=pred[1])
        assert np.array_equal(full["mv"][1], umv) and np.array_equal(full["sad"][1], usad)
        assert np.array_equal(full["qmv"][1], uq) and np.array_equal(full["cost"][1], uc)
    finally:
        for p in planes:
            p.close()


# ---- 5: a launch of identity weights only IS the unweighted launch with fen = 0 ------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_an_all_identity_launch_is_the_unweighted_launch_without_fen(engine, bd):
    import torch
    from hmme import api, synth
    sr = 4
    n_ctu = 6
    dev = torch.device("cuda", 0)
    a = three_planes(W, H, bd, seed=2600 + bd)
    b = three_planes(W, H, bd, seed=2700 + bd)
    planes = [mkplane(engine, p, W, H, bd) for p in a + b]
    try:
        curs, refs, others = [planes[0], planes[3]], [planes[1], planes[4]], [planes[2], planes[5]]
        f = np.stack([random_field(n_ctu, 64, 2610 + i) for i in range(2)])
        pred = np.stack([synth.random_predictors(n_ctu, seed=2620 + i, max_pel=6) for i in range(2)])
        center = np.stack([synth.random_predictors(n_ctu, seed=2630 + i, max_pel=6) for i in range(2)])
        d_f, d_pred, d_center = (torch.from_numpy(x).to(dev) for x in (f, pred, center))
        ref_t = {}
        for fen in (0, 1):
            fp = api.FrameParams(sr, fen, bd, 0, n_ctu)
            d_mv, d_sad = device_tables(2, n_ctu, dev)
            d_q, d_c = device_tables(2, n_ctu, dev)
            engine.search_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
            engine.refine_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), 1, d_q.data_ptr(),
                                          d_c.data_ptr(), 0)
            torch.cuda.synchronize()
            ref_t[fen] = (d_mv, d_sad, d_q, d_c)
        assert not torch.equal(ref_t[0][1], ref_t[1][1])   # FEN does change the unweighted bi search of these pictures
        for idents in ([IDENT, (1, 0, 0, 0)], [(1 << 15, 0, 15, 1 << 14), IDENT]):
            for fen in (0, 1):
                fp = api.FrameParams(sr, fen, bd, 0, n_ctu)
                d_mv, d_sad = device_tables(2, n_ctu, dev)
                d_q, d_c = device_tables(2, n_ctu, dev)
                engine.search_pairs_bi_w_device(curs, refs, others, fp, idents, idents[::-1], d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(),
                                                d_mv.data_ptr(), d_sad.data_ptr(), 0)
                engine.refine_pairs_bi_w_device(curs, refs, others, fp, idents, idents[::-1], d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(),
                                                d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
                torch.cuda.synchronize()
                for got, want in zip((d_mv, d_sad, d_q, d_c), ref_t[0]):
                    assert torch.equal(got, want), (idents, fen)
    finally:
        for p in planes:
            p.close()


# ---- 6: range edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 9, 10, 11, 12])
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_search_and_refinement_at_the_accepted_weight_nearest_to_each_refusal(engine, oracle_lib, hmo, bd, family):
    """pictures of samples in {0, maxv}, one CTU whose origin is -maxv throughout and one where it is 2 * maxv (range_content.extreme_triple);
    the searched weight: the last member of its family hmme_bipred_weight_check accepts -- for the search, and (another weight) for the refinement"""
    from hmme import api
    maxv = (1 << bd) - 1
    planes3 = rc.extreme_triple(W, H, bd, seed=2800 + bd)
    assert all(set(np.unique(p)) == {0, maxv} for p in planes3)
    todo = [(0, b) for b in model.boundary_weights(bd, 0) if b["family"] == family] + [(1, b) for b in model.boundary_weights(bd, 1) if b["family"] == family]
    assert len(todo) == (1 if bd == 12 else 2)
    for refine, b in todo:
        wp = b["wp"]
        assert api.bipred_weight_check(bd, wp, IDENT, refine) == 0 and api.bipred_weight_check(bd, b["next"], IDENT, refine) == -5
        per = 1 if refine else 64
        r = run_case(engine, oracle_lib, hmo, W, H, bd, 4, wp, IDENT, per, seed=2810 + bd, planes3=planes3, had=(bd % 2) if refine else None,
                     field=random_field(6, per, 2811 + bd + per))
        # the content reaches what the rule bounds: both extremes of the origin, and the span between origin and weighted reference
        assert r["org"].min() == -maxv and r["org"].max() == 2 * maxv
        wlo, whi, bias, span, _, _ = model.searched_terms(bd, wp)
        wref = rc.weigh(planes3[1], wp)
        assert wref.min() == wlo and wref.max() == whi
        assert max(2 * maxv - wlo, whi + maxv) == span


def test_the_12_bit_refinement_is_refused_and_a_refused_pair_stops_the_whole_launch(engine):
    import torch
    from hmme import api
    sr, n_ctu = 4, 6
    dev = torch.device("cuda", 0)
    d_f = torch.zeros((3, n_ctu, 1, 2), dtype=torch.int16, device=dev)
    d_imv = torch.zeros((3, n_ctu, 593, 2), dtype=torch.int16, device=dev)

    def sentinels():
        return (torch.full((3, n_ctu, 593, 2), MV_SENT, dtype=torch.int16, device=dev), torch.full((3, n_ctu, 593), COST_SENT, dtype=torch.int32, device=dev))

    def untouched(t_mv, t_c):
        torch.cuda.synchronize()
        return bool((t_mv == MV_SENT).all()) and bool((t_c == COST_SENT).all())

    p12 = [mkplane(engine, a, W, H, 12) for a in three_planes(W, H, 12, seed=2900)]
    p8 = [mkplane(engine, a, W, H, 8) for a in three_planes(W, H, 8, seed=2901)]
    try:
        # 12 bits: the refinement is refused for every weight, the search is served
        fp12 = api.FrameParams(sr, 0, 12, 0, n_ctu)
        for wp in (IDENT, scaled(FADE, 12)):
            assert api.bipred_weight_check(12, wp, IDENT, 1) == -5 and api.bipred_weight_check(12, wp, IDENT, 0) == 0
            t_q, t_c = sentinels()
            with pytest.raises(api.HmmeError):
                engine.refine_pairs_bi_w_device([p12[0]], [p12[1]], [p12[2]], fp12, [wp], [IDENT], d_f.data_ptr(), 1, None, None, d_imv.data_ptr(), 1,
                                                t_q.data_ptr(), t_c.data_ptr(), 0)
            assert untouched(t_q, t_c)
        # three pairs, the middle one refused (its searched weight; then its other weight; then a shift of 16): nothing is written, the
        # error names pair 1
        fp = api.FrameParams(sr, 0, 8, 0, n_ctu)
        good, refused = scaled(FADE, 8), (64, 3000, 6, 32)
        assert api.bipred_weight_check(8, good, good, 1) == 0 and api.bipred_weight_check(8, refused, IDENT, 0) == -5
        assert api.bipred_weight_check(8, IDENT, (1 << 20, 0, 3, 4), 0) == -5 and api.bipred_weight_check(8, IDENT, (1 << 16, 0, 16, 0), 0) == -1
        for wps, owps in (([good, refused, good], [good] * 3), ([good] * 3, [good, (1 << 20, 0, 3, 4), good]), ([good] * 3, [good, (1 << 16, 0, 16, 0), good])):
            t_mv, t_sad = sentinels()
            with pytest.raises(api.HmmeError, match="pair 1"):
                engine.search_pairs_bi_w_device([p8[0]] * 3, [p8[1]] * 3, [p8[2]] * 3, fp, wps, owps, d_f.data_ptr(), 1, None, None, t_mv.data_ptr(), t_sad.data_ptr(), 0)
            with pytest.raises(api.HmmeError, match="pair 1"):
                engine.refine_pairs_bi_w_device([p8[0]] * 3, [p8[1]] * 3, [p8[2]] * 3, fp, wps, owps, d_f.data_ptr(), 1, None, None, d_imv.data_ptr(), 1,
                                                t_mv.data_ptr(), t_sad.data_ptr(), 0)
            assert untouched(t_mv, t_sad)
        img = np.full((H, W), 0xA5, np.uint8)
        with pytest.raises(api.HmmeError):
            engine.predict_frame_w(p8[1], (1 << 20, 0, 3, 4), np.zeros((n_ctu, 2), np.int16), out=img)
        assert np.all(img == 0xA5)
        # ... and the launch that is served still is
        t_mv, t_sad = sentinels()
        engine.search_pairs_bi_w_device([p8[0]] * 3, [p8[1]] * 3, [p8[2]] * 3, fp, [good] * 3, [good] * 3, d_f.data_ptr(), 1, None, None, t_mv.data_ptr(),
                                        t_sad.data_ptr(), 0)
        torch.cuda.synchronize()
        assert not bool((t_sad == COST_SENT).any())
    finally:
        for p in p12 + p8:
            p.close()


# ---- 7: what it is for -------------------------------------------------------------------------------------------------------------------
def test_on_a_fade_the_weighted_bi_pass_costs_less_than_the_unweighted_one(engine):
    """cur = the faded average of two differently displaced textures, both lists unfaded; the weights are the engine's own estimate.  After the
    weighted uni-directional searches and refinements of both lists, the bi pass with the weights has a smaller summed SAD than without"""
    from hmme import api, synth
    w = h = 128
    bd, m = 8, synth.MARGIN
    _, ta, _ = synth.make_pair(w, h, seed=3001, max_mv=0)
    _, tb, _ = synth.make_pair(w, h, seed=3002, max_mv=0)
    (ax, ay), (bx, by) = (3, -2), (-4, 1)
    a = np.roll(ta, (-ay, -ax), axis=(0, 1)).astype(np.int32)
    b = np.roll(tb, (-by, -bx), axis=(0, 1)).astype(np.int32)
    avg = ((a + b + 1) >> 1)[m:m + h, m:m + w]
    cur = synth.pad_plane(np.clip(((40 * avg + 32) >> 6) + 12, 0, 255))
    pc, pa, pb = (mkplane(engine, p, w, h, bd) for p in (cur, ta, tb))
    try:
        weights, infos = engine.wp_estimate(pc, [pa, pb])
        assert all(i.present for i in infos) and all(wt[0] != 1 << wt[2] for wt in weights)   # the estimator saw the fade
        uni = []
        for ref, wt in ((pa, weights[0]), (pb, weights[1])):
            assert api.weight_check(bd, wt, 1) == 0
            mv, _ = engine.search_frame_w(pc, ref, 8, wt)
            uni.append(engine.refine_frame_w(pc, ref, 8, wt, mv))
        total = {}
        for ref, other, wt, owt, (q_ref, _), (q_other, _) in ((pa, pb, weights[0], weights[1], uni[0], uni[1]), (pb, pa, weights[1], weights[0], uni[1], uni[0])):
            assert api.bipred_weight_check(bd, wt, owt, 1) == 0
            field, centre = q_other[:, 592], q_ref[:, 592]
            _, sad_w = engine.search_frame_bi_w(pc, ref, other, 4, wt, owt, field, center_q=centre)
            _, sad_u = engine.search_frame_bi(pc, ref, other, 4, field, center_q=centre, fen=0)
            total.setdefault("w", []).append(int(sad_w.astype(np.int64).sum()))
            total.setdefault("u", []).append(int(sad_u.astype(np.int64).sum()))
    finally:
        pc.close(); pa.close(); pb.close()
    for d in range(2):
        assert total["w"][d] < total["u"][d], total
