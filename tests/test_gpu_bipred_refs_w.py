"""The bi pass of one list over all its references in a slice with explicit weighted prediction (hmme_search_frame_bi_refs_w_device,
hmme_refine_frame_bi_refs_w_device and their host-array forms): per reference and CTU the per-CTU calls Engine.search_ctu_w /
Engine.refine_ctu_w with that reference's weight on the origin 2 * cur - P built here as tests/test_gpu_bipred_refs.py builds it, P =
bipred_wp_model.pred_w block by block from the plane AND the weight the block's index names -- inside the picture what
Engine.predict_refs_w_frame writes.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
from frame_helpers import bind_hmo, clip_mv, dims, mkplane, origin_picture, random_field
from test_gpu_bipred_refs import SR_BI, checkerboard, pictures, predictors, select_refs_field, unrelated

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5
IDENT = (64, 0, 6, 32)
# weights written for 8 bits: (w0, offset, shift, round)
FADE = (40, -12, 5, 16)            # 40 / 32, offset -12
NEGATIVE = (-20, 200, 5, 16)       # a negative w0
GAIN = (90, 7, 6, 32)
BELOW_ZERO = (64, -300, 6, 32)     # weighted samples down to -300 << (bd - 8), below -maxv: this weight's bias exceeds maxv
OTHERS = (FADE, (80, 5, 6, 32), IDENT, NEGATIVE)     # others[0] is not the identity: it is what an index >= n_others takes


def scaled(wp, bd):
    return (wp[0], wp[1] << (bd - 8) if wp[1] >= 0 else -((-wp[1]) << (bd - 8)), wp[2], wp[3])


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(57.9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def refs_prediction_w(hmo, others, owps, w, h, bd, field, ref_field):
    """bipred_refs_bands.refs_prediction with addWeightUni as the tail: bipred_wp_model.pred_w for every CTU of the picture, whole blocks
    (partial edge CTUs too), from others[index] with owps[index] -- index 0 where it is >= len(others) -> int16 [ctus_y * 64, ctus_x * 64]"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    out = np.zeros((cy_n * 64, cx_n * 64), np.int16)
    per = field.shape[1]
    g = 64 if per == 1 else 8
    for ctu in range(cx_n * cy_n):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(per):
            bx, by = (b % 8) * g, (b // 8) * g
            idx = int(ref_field[ctu, b])
            idx = idx if idx < len(others) else 0
            qx, qy = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
            out[cu_y + by:cu_y + by + g, cu_x + bx:cu_x + bx + g] = bwm.pred_w(others[idx], m + cu_x + bx, m + cu_y + by, g, g, qx, qy, bd, owps[idx])
    return out


def per_ctu_w(engine, org, ref, w, h, bd, sr, center, pred, wp, ctus, int_mv=None, had=True):
    """Engine.search_ctu_w (int_mv None) or Engine.refine_ctu_w per CTU on the origin `org` (sample (0, 0) at [0, 0]) against the padded `ref`;
    FEN on in the parameters: the weighted calls must not consult it"""
    from hmme import api, synth
    m = synth.MARGIN
    cx_n, _ = dims(w, h)
    mv, cost = np.zeros((len(ctus), 593, 2), np.int16), np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        qx, qy = (int(center[ctu, 0]), int(center[ctu, 1])) if center is not None else (px, py)
        p = api.SearchParams(*api.set_search_range(qx, qy, sr, x, y, w, h), px, py, 1, bd)
        if int_mv is None:
            mv[k], cost[k] = engine.search_ctu_w(org, (x, y), ref, (m + x, m + y), p, wp)
        else:
            mv[k], cost[k] = engine.refine_ctu_w(org, (x, y), ref, (m + x, m + y), p, wp, int_mv[k], use_hadamard=had)
    return mv, cost


def check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, refs_i, others_i, wps, owps, field, ref_field, seed, had=True, ctus=None):
    """both calls over the references pics[refs_i] (weights wps) against pics[others_i] (weights owps) -> the four tables, checked on `ctus`"""
    from hmme import api
    n_ctu = dims(w, h)[0] * dims(w, h)[1]
    assert api.bipred_refs_weight_check(bd, wps, owps, True) == 0
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        refs, others = [planes[i] for i in refs_i], [planes[i] for i in others_i]
        pred, center = predictors(len(refs), n_ctu, seed), predictors(len(refs), n_ctu, seed + 50)
        mv, sad = engine.search_frame_bi_refs_w(planes[0], refs, others, SR_BI, wps, owps, field, ref_field, center_q=center, pred_q=pred)
        qmv, cost = engine.refine_frame_bi_refs_w(planes[0], refs, others, SR_BI, wps, owps, field, ref_field, mv, center_q=center, pred_q=pred, use_hadamard=had)
        f3 = field.reshape(n_ctu, -1, 2)
        rf = np.asarray(ref_field).reshape(n_ctu, -1)
        p_full = refs_prediction_w(hmo, [pics[i] for i in others_i], owps, w, h, bd, f3, rf)
        # inside the picture, where the index names a plane, P is hmme_predict_refs_w_device's prediction
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0xA5A5)
        pr = engine.predict_refs_w_frame(others, owps, f3 if f3.shape[1] == 64 else f3[:, 0], rf, out=np.full((h, w), fill, dt))
        if f3.shape[1] == 64:
            cx_n, cy_n = dims(w, h)
            blocks = rf.reshape(cy_n, cx_n, 8, 8).transpose(0, 2, 1, 3).reshape(cy_n * 8, cx_n * 8)
            named = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:h, :w] < len(others)
            assert named.any() and np.array_equal(pr[named].astype(np.int16), p_full[:h, :w][named]) and (pr[~named] == fill).all()
        org = origin_picture(pics[0], p_full, w, h)
        todo = list(range(n_ctu) if ctus is None else ctus)
        for r, i in enumerate(refs_i):
            smv, ssad = per_ctu_w(engine, org, pics[i], w, h, bd, SR_BI, center[r], pred[r], wps[r], todo)
            assert np.array_equal(mv[r][todo], smv) and np.array_equal(sad[r][todo], ssad), ("search", r)
            sq, sc = per_ctu_w(engine, org, pics[i], w, h, bd, SR_BI, center[r], pred[r], wps[r], todo, mv[r][todo], had)
            assert np.array_equal(qmv[r][todo], sq) and np.array_equal(cost[r][todo], sc), ("refine", r)
        return dict(mv=mv, sad=sad, qmv=qmv, cost=cost, pred=pred, center=center)
    finally:
        for p in planes:
            p.close()


# ---- 1: several planes of different content and weight in the other list: the per-CTU calls on the origin ------------------------------------
@pytest.mark.parametrize("n_others", [2, 4])
@pytest.mark.parametrize("w,h,bd,per", [(64, 64, 10, 64), (100, 70, 8, 64), (136, 72, 8, 1), (136, 72, 10, 64)])
def test_a_checkerboard_of_references_equals_the_per_ctu_calls(engine, hmo, w, h, bd, per, n_others):
    n_ctu = dims(w, h)[0] * dims(w, h)[1]
    pics = pictures(w, h, bd, 4100 + w + bd, 3) + unrelated(w, h, bd, 4150 + w, n_others)
    others_i = list(range(3, 3 + n_others))
    wps, owps = [scaled(FADE, bd), scaled(NEGATIVE, bd)], [scaled(o, bd) for o in OTHERS[:n_others]]
    field = random_field(n_ctu, per, 4110 + w + n_others)
    ref_field = checkerboard(n_ctu, per, n_others, w)
    assert set(ref_field.reshape(-1).tolist()) == set(range(n_others))
    got = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, [1, 2], others_i, wps, owps, field, ref_field, 4120 + n_others, had=bool(per == 64))
    # the other list's weights matter, and so does the index that picks them
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        args = (planes[0], planes[1:3], [planes[i] for i in others_i], SR_BI)
        kw = dict(center_q=got["center"], pred_q=got["pred"])
        plain, _ = engine.search_frame_bi_refs_w(*args, wps, [IDENT] * n_others, field, ref_field, **kw)
        turned, _ = engine.search_frame_bi_refs_w(*args, wps, owps[1:] + owps[:1], field, ref_field, **kw)
        assert not np.array_equal(plain, got["mv"]) and not np.array_equal(turned, got["mv"])
    finally:
        for p in planes:
            p.close()


def test_a_field_out_of_select_refs_frame_equals_the_per_ctu_calls(engine, hmo):
    """the other list's uni pass gives the field: its 0xFF (blocks of CUs that do not exist, outside the picture, MV (0,0)) reads reference 0
    and takes reference 0's weight, which is not the identity"""
    from hmme import synth
    w, h, bd = 100, 70, 8
    pics = pictures(w, h, bd, 4200 + w, 7)
    for k, noise in enumerate(unrelated(w, h, bd, 4250 + w, 4)):               # other k shows the scene in the k-th quarter of the width only
        x0, x1 = (0 if k == 0 else synth.MARGIN + k * w // 4), (noise.shape[1] if k == 3 else synth.MARGIN + (k + 1) * w // 4)
        noise[:, x0:x1] = pics[3 + k][:, x0:x1]
        pics[3 + k] = noise
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        field, ref_field = select_refs_field(engine, planes[0], planes[3:7], w, h)
    finally:
        for p in planes:
            p.close()
    assert 0xFF in ref_field and len(set(ref_field.reshape(-1).tolist()) - {0xFF}) >= 2 and (field[ref_field == 0xFF] == 0).all()
    wps, owps = [scaled(GAIN, bd), scaled(FADE, bd)], [scaled(o, bd) for o in OTHERS]
    got = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, [1, 2], [3, 4, 5, 6], wps, owps, field, ref_field, 4220)
    # ... which is what the same field gives with index 0 in their place, and not what it gives when reference 0 has another weight
    zeroed = np.where(ref_field == 0xFF, 0, ref_field).astype(np.uint8)
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        kw = dict(center_q=got["center"], pred_q=got["pred"])
        mv0, sad0 = engine.search_frame_bi_refs_w(planes[0], planes[1:3], planes[3:7], SR_BI, wps, owps, field, zeroed, **kw)
        assert np.array_equal(mv0, got["mv"]) and np.array_equal(sad0, got["sad"])
        _, sad1 = engine.search_frame_bi_refs_w(planes[0], planes[1:3], planes[3:7], SR_BI, wps, [IDENT] + owps[1:], field, ref_field, **kw)
        edge = [c for c in range(ref_field.shape[0]) if (ref_field[c] == 0xFF).any()]
        assert edge and not np.array_equal(sad1[:, edge], got["sad"][:, edge])
    finally:
        for p in planes:
            p.close()


# ---- 2: the searched weights: runs of equal weights, and ONE bias for all references ---------------------------------------------------------------
@pytest.mark.parametrize("bd,had", [(8, True), (10, False)])
def test_runs_of_equal_searched_weights_and_a_common_bias_above_maxv(engine, hmo, bd, had):
    """[a, a, b, a]: three refinement launches, the second and third at their own table offsets; b's weighted samples go below -maxv, so the
    ONE origin of all four references carries b's bias, beside a, whose own bias would be maxv"""
    w, h = 100, 70
    a, b = scaled(FADE, bd), scaled(BELOW_ZERO, bd)
    maxv = (1 << bd) - 1
    assert bwm.searched_terms(bd, b)[2] > maxv and bwm.searched_terms(bd, a)[2] == maxv
    pics = pictures(w, h, bd, 4300 + bd, 5) + unrelated(w, h, bd, 4350, 2)
    field = random_field(4, 64, 4310 + bd)
    got = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, [1, 2, 3, 4], [5, 6], [a, a, b, a], [scaled(o, bd) for o in OTHERS[:2]], field,
                                          checkerboard(4, 64, 2, w), 4320, had=had, ctus=[0, 3])
    assert not np.array_equal(got["cost"][2], got["cost"][3])


# ---- 3: identities ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_identities_and_the_single_reference_calls(engine, bd):
    w, h, n_ctu = 100, 70, 4
    pics = pictures(w, h, bd, 4400 + bd, 3) + unrelated(w, h, bd, 4450, 2)
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        cur, refs, others = planes[0], planes[1:3], planes[3:5]
        field, ref_field = random_field(n_ctu, 64, 4410), checkerboard(n_ctu, 64, 2, w)
        pred, center = predictors(2, n_ctu, 4420), predictors(2, n_ctu, 4430)
        kw = dict(center_q=center, pred_q=pred)
        wt = scaled(FADE, bd)
        umv, usad = engine.search_frame_bi_refs(cur, refs, others, SR_BI, field, ref_field, fen=0, **kw)
        uq, uc = engine.refine_frame_bi_refs(cur, refs, others, SR_BI, field, ref_field, umv, **kw)
        # every weight of both lists the identity: the unweighted call with fen = 0 (other weights: whatever round holds)
        ids = [IDENT, (8, 0, 3, 4)]
        mv, sad = engine.search_frame_bi_refs_w(cur, refs, others, SR_BI, ids, [(64, 0, 6, 5), (1, 0, 0, 0)], field, ref_field, **kw)
        q, c = engine.refine_frame_bi_refs_w(cur, refs, others, SR_BI, ids, [(64, 0, 6, 5), (1, 0, 0, 0)], field, ref_field, mv, **kw)
        assert np.array_equal(mv, umv) and np.array_equal(sad, usad) and np.array_equal(q, uq) and np.array_equal(c, uc)
        # [identity, w] with identity other weights: table 0 is the unweighted call's
        mv, sad = engine.search_frame_bi_refs_w(cur, refs, others, SR_BI, [IDENT, wt], [IDENT, IDENT], field, ref_field, **kw)
        q, c = engine.refine_frame_bi_refs_w(cur, refs, others, SR_BI, [IDENT, wt], [IDENT, IDENT], field, ref_field, mv, **kw)
        assert np.array_equal(mv[0], umv[0]) and np.array_equal(sad[0], usad[0]) and np.array_equal(q[0], uq[0]) and np.array_equal(c[0], uc[0])
        assert not np.array_equal(sad[1], usad[1]) and not np.array_equal(c[1], uc[1])
        # one reference per list: search_frame_bi_w / refine_frame_bi_w (whatever the index: one plane is read, with its weight)
        owp = scaled(NEGATIVE, bd)
        any_index = np.random.default_rng(4440).choice(np.array([0, 0xFF, 1, 7], np.uint8), size=(n_ctu, 64))
        for r in range(2):
            mv, sad = engine.search_frame_bi_refs_w(cur, refs[r:r + 1], others[:1], SR_BI, [wt], [owp], field, any_index, center_q=center[r:r + 1], pred_q=pred[r:r + 1])
            q, c = engine.refine_frame_bi_refs_w(cur, refs[r:r + 1], others[:1], SR_BI, [wt], [owp], field, any_index, mv, center_q=center[r:r + 1], pred_q=pred[r:r + 1])
            smv, ssad = engine.search_frame_bi_w(cur, refs[r], others[0], SR_BI, wt, owp, field, center_q=center[r], pred_q=pred[r])
            sq, sc = engine.refine_frame_bi_w(cur, refs[r], others[0], SR_BI, wt, owp, field, smv, center_q=center[r], pred_q=pred[r])
            assert np.array_equal(mv[0], smv) and np.array_equal(sad[0], ssad) and np.array_equal(q[0], sq) and np.array_equal(c[0], sc), r
    finally:
        for p in planes:
            p.close()


# ---- 4: launch shapes: 1 and 16 references, SAD and Hadamard, a CTU sub-range, the device entries, a used context -----------------------------------
def test_sixteen_references_a_sub_range_and_the_device_entries(engine, hmo):
    import torch
    from hmme import api
    w, h, bd, n_ctu = 136, 72, 8, 6
    dev = torch.device("cuda", 0)
    pics = pictures(w, h, bd, 4500, 5) + unrelated(w, h, bd, 4550, 3)
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        cur, others = planes[0], planes[5:8]
        sixteen = [planes[1 + k % 4] for k in range(16)]
        four = [FADE, GAIN, BELOW_ZERO, IDENT]
        wps = [four[k % 4] for k in range(16)]                                  # no two neighbours equal: sixteen refinement launches
        owps = list(OTHERS[:3])
        field, ref_field = random_field(n_ctu, 64, 4510), checkerboard(n_ctu, 64, 3, w)
        pred, center = predictors(16, n_ctu, 4520), predictors(16, n_ctu, 4540)
        for k in range(4, 16):                                                 # the same plane, weight, predictor and centre: the same table
            pred[k], center[k] = pred[k % 4], center[k % 4]
        mv, sad = engine.search_frame_bi_refs_w(cur, sixteen, others, SR_BI, wps, owps, field, ref_field, center_q=center, pred_q=pred)
        qmv, cost = engine.refine_frame_bi_refs_w(cur, sixteen, others, SR_BI, wps, owps, field, ref_field, mv, center_q=center, pred_q=pred)
        sadq, sadc = engine.refine_frame_bi_refs_w(cur, sixteen, others, SR_BI, wps, owps, field, ref_field, mv, center_q=center, pred_q=pred, use_hadamard=False)
        for k in range(4, 16):
            assert np.array_equal(mv[k], mv[k % 4]) and np.array_equal(sad[k], sad[k % 4]) and np.array_equal(qmv[k], qmv[k % 4]) and np.array_equal(cost[k], cost[k % 4])
            assert np.array_equal(sadq[k], sadq[k % 4]) and np.array_equal(sadc[k], sadc[k % 4])
        assert not np.array_equal(sadc, cost)
        # ... pinned to the per-CTU calls on two CTUs of the four, Hadamard and SAD
        org = origin_picture(pics[0], refs_prediction_w(hmo, pics[5:8], owps, w, h, bd, field, ref_field), w, h)
        for r in range(4):
            smv, ssad = per_ctu_w(engine, org, pics[1 + r], w, h, bd, SR_BI, center[r], pred[r], wps[r], [1, 5])
            assert np.array_equal(mv[r][[1, 5]], smv) and np.array_equal(sad[r][[1, 5]], ssad), r
            for had, (tq, tc) in ((True, (qmv, cost)), (False, (sadq, sadc))):
                sq, sc = per_ctu_w(engine, org, pics[1 + r], w, h, bd, SR_BI, center[r], pred[r], wps[r], [1, 5], mv[r][[1, 5]], had)
                assert np.array_equal(tq[r][[1, 5]], sq) and np.array_equal(tc[r][[1, 5]], sc), (r, had)
        # 1 reference: the first table of the 16 -- whatever bias the other fifteen asked for
        a, b = engine.search_frame_bi_refs_w(cur, sixteen[:1], others, SR_BI, wps[:1], owps, field, ref_field, center_q=center[:1], pred_q=pred[:1])
        q, c = engine.refine_frame_bi_refs_w(cur, sixteen[:1], others, SR_BI, wps[:1], owps, field, ref_field, a, center_q=center[:1], pred_q=pred[:1])
        assert np.array_equal(a, mv[:1]) and np.array_equal(b, sad[:1]) and np.array_equal(q, qmv[:1]) and np.array_equal(c, cost[:1])
        # a CTU sub-range == the same rows of the full call, host form and device form
        first, count = 1, 4
        a, b = engine.search_frame_bi_refs_w(cur, sixteen[:3], others, SR_BI, wps[:3], owps, field, ref_field, center_q=center[:3], pred_q=pred[:3], ctu_first=first,
                                             ctu_count=count)
        q, c = engine.refine_frame_bi_refs_w(cur, sixteen[:3], others, SR_BI, wps[:3], owps, field, ref_field, a, center_q=center[:3], pred_q=pred[:3], ctu_first=first,
                                             ctu_count=count)
        rows = slice(first, first + count)
        assert np.array_equal(a, mv[:3, rows]) and np.array_equal(b, sad[:3, rows]) and np.array_equal(q, qmv[:3, rows]) and np.array_equal(c, cost[:3, rows])
        d_f, d_r, d_p, d_c = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (field, ref_field, pred[:3], center[:3]))
        d_mv = torch.zeros((3, count, 593, 2), dtype=torch.int16, device=dev)
        d_sad = torch.zeros((3, count, 593), dtype=torch.int32, device=dev)
        d_q, d_cc = torch.zeros_like(d_mv), torch.zeros_like(d_sad)
        torch.cuda.synchronize()
        fp = api.FrameParams(SR_BI, 1, bd, first, count)                        # fen = 1: not consulted
        engine.search_frame_bi_refs_w_device(cur, sixteen[:3], others, fp, wps[:3], owps, d_f.data_ptr(), d_r.data_ptr(), 64, d_c.data_ptr(), d_p.data_ptr(),
                                             d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_frame_bi_refs_w_device(cur, sixteen[:3], others, fp, wps[:3], owps, d_f.data_ptr(), d_r.data_ptr(), 64, d_c.data_ptr(), d_p.data_ptr(),
                                             d_mv.data_ptr(), 1, d_q.data_ptr(), d_cc.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(d_mv.cpu().numpy(), a) and np.array_equal(d_sad.cpu().numpy().view(np.uint32), b)
        assert np.array_equal(d_q.cpu().numpy(), q) and np.array_equal(d_cc.cpu().numpy().view(np.uint32), c)
        # a used context gives what a fresh one gives
        fresh = api.Engine(0, 64)
        fresh.set_lambda_q16(engine.lambda_q16)
        fplanes = [mkplane(fresh, p, w, h, bd) for p in pics]
        try:
            fa, fb = fresh.search_frame_bi_refs_w(fplanes[0], fplanes[1:4], fplanes[5:8], SR_BI, wps[:3], owps, field, ref_field, center_q=center[:3], pred_q=pred[:3])
            fq, fc = fresh.refine_frame_bi_refs_w(fplanes[0], fplanes[1:4], fplanes[5:8], SR_BI, wps[:3], owps, field, ref_field, fa, center_q=center[:3], pred_q=pred[:3])
            assert np.array_equal(fa, mv[:3]) and np.array_equal(fb, sad[:3]) and np.array_equal(fq, qmv[:3]) and np.array_equal(fc, cost[:3])
        finally:
            for p in fplanes:
                p.close()
            fresh.close()
    finally:
        for p in planes:
            p.close()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_sentinels(engine):
    import torch
    from hmme import api
    w, h, n_ctu = 136, 72, 6
    dev = torch.device("cuda", 0)
    d_f = torch.zeros((n_ctu, 64, 2), dtype=torch.int16, device=dev)
    d_r = torch.zeros((n_ctu, 64), dtype=torch.uint8, device=dev)
    d_imv = torch.zeros((16, n_ctu, 593, 2), dtype=torch.int16, device=dev)
    t_mv = torch.full((16, n_ctu, 593, 2), 0x5A5A, dtype=torch.int16, device=dev)
    t_c = torch.full((16, n_ctu, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((t_mv == 0x5A5A).all()) and bool((t_c == 0x5A5A5A5A).all())

    a, b, c, small, deep = engine.plane(w, h), engine.plane(w, h), engine.plane(w, h), engine.plane(64, 64), engine.plane(w, h, 10)
    p12 = [engine.plane(w, h, 12) for _ in range(3)]
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        fp = api.FrameParams(SR_BI, 1, 8, 0, n_ctu)
        ok, far = FADE, (32767, 0, 0, 0)                                         # far: a weighted sample beyond a Pel
        wide = (60000, 0, 6, 32)                                                 # as an other weight: |w0| * 40 960 beyond int32

        def both(cur, refs, others, wps, owps, fp=fp, f=d_f.data_ptr(), r=d_r.data_ptr(), per=64, mv=t_mv.data_ptr(), cost=t_c.data_ptr(), n_refs=None, n_others=None):
            ra, oa = api._handles(refs), api._handles(others)
            nr, no = len(refs) if n_refs is None else n_refs, len(others) if n_others is None else n_others
            wa, wb = (None if x is None else engine._weights(x) for x in (wps, owps))
            s = L.hmme_search_frame_bi_refs_w_device(engine.h, cur.h, ra, nr, oa, no, C.byref(fp), wa, wb, f, r, per, None, None, mv, cost, None)
            q = L.hmme_refine_frame_bi_refs_w_device(engine.h, cur.h, ra, nr, oa, no, C.byref(fp), wa, wb, f, r, per, None, None, d_imv.data_ptr(), 1, mv, cost, None)
            return s, q

        assert both(c, [a, b], [b], None, [ok]) == (ERR_ARG, ERR_ARG) and both(c, [a, b], [b], [ok, ok], None) == (ERR_ARG, ERR_ARG)
        assert both(c, [a, b], [b], [ok, (40, 0, 16, 0)], [ok]) == (ERR_ARG, ERR_ARG) and both(c, [a, b], [b], [ok, ok], [(40, 0, -1, 0)]) == (ERR_ARG, ERR_ARG)
        assert both(c, [a, b], [b], [far, ok], [(40, 0, 16, 0)]) == (ERR_ARG, ERR_ARG)             # the other list's argument error answers first
        assert both(c, [a, b], [b], [ok, far], [ok]) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
        assert both(c, [a, b], [b, a], [ok, ok], [ok, wide]) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
        assert both(c, [a], [b], [ok], [ok], n_refs=0) == (ERR_ARG, ERR_ARG) and both(c, [a], [b], [ok], [ok], n_others=17) == (ERR_ARG, ERR_ARG)
        # a weight the search serves and the refinement does not: w0 * sample + round at 2^24
        rough = (70000, 0, 15, 1 << 14)
        assert api.bipred_refs_weight_check(8, [ok, rough], [ok]) == 0 and api.bipred_refs_weight_check(8, [ok, rough], [ok], True) == ERR_UNSUPPORTED
        s, q = both(c, [a, b], [b], [ok, rough], [ok], mv=None)                  # the search gets as far as its buffers; the refinement stops at the weight
        assert (s, q) == (ERR_ARG, ERR_UNSUPPORTED)
        # with good weights the checks are the unweighted call's
        assert both(c, [a], [b, small], [ok], [ok, ok]) == (ERR_ARG, ERR_ARG) and both(c, [a, deep], [b], [ok, ok], [ok]) == (ERR_ARG, ERR_ARG)
        assert both(c, [a], [b], [ok], [ok], r=None) == (ERR_ARG, ERR_ARG) and both(c, [a], [b], [ok], [ok], per=4) == (ERR_ARG, ERR_ARG)
        assert both(c, [a], [b], [ok], [ok], fp=api.FrameParams(SR_BI, 1, 8, 5, 2)) == (ERR_ARG, ERR_ARG)
        assert both(c, [a], [b], [ok], [ok], fp=api.FrameParams(SR_BI, 1, 7, 0, n_ctu)) == (ERR_ARG, ERR_ARG)
        # 12 bits are searched and not refined, whatever the weights
        fp12 = api.FrameParams(SR_BI, 1, 12, 0, n_ctu)
        ra, oa = api._handles(p12[1:2]), api._handles(p12[2:])
        for wt in (IDENT, ok):
            assert api.bipred_refs_weight_check(12, [wt], [IDENT], True) == ERR_UNSUPPORTED and api.bipred_refs_weight_check(12, [wt], [IDENT], False) == 0
            assert L.hmme_refine_frame_bi_refs_w_device(engine.h, p12[0].h, ra, 1, oa, 1, C.byref(fp12), engine._weights([wt]), engine._weights([IDENT]), d_f.data_ptr(),
                                                        d_r.data_ptr(), 64, None, None, d_imv.data_ptr(), 1, t_mv.data_ptr(), t_c.data_ptr(), None) == ERR_UNSUPPORTED
        with pytest.raises(api.HmmeError, match="hmme_refine_frame_bi_refs_w"):
            engine.refine_frame_bi_refs_w(p12[0], p12[1:2], p12[2:], SR_BI, [ok], [IDENT], np.zeros((n_ctu, 2), np.int16), np.zeros((n_ctu, 1), np.uint8),
                                          np.zeros((1, n_ctu, 593, 2), np.int16))
        with pytest.raises(api.HmmeError, match="hmme_search_frame_bi_refs_w: other reference 1"):
            engine.search_frame_bi_refs_w(c, [a], [b, a], SR_BI, [ok], [ok, wide], np.zeros((n_ctu, 2), np.int16), np.zeros((n_ctu, 1), np.uint8))
        assert untouched()
        assert both(c, [a, b], [b, a], [ok, GAIN], [ok, IDENT]) == (0, 0)         # the accepted neighbour does run
        torch.cuda.synchronize()
        assert not bool((t_c[:2] == 0x5A5A5A5A).any()) and bool((t_c[2:] == 0x5A5A5A5A).all())
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in [a, b, c, small, deep] + p12:
            p.close()
