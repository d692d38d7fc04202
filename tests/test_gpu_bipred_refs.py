"""The bi pass of one list over all its references against a reference per block in the other list (hmme_search_frame_bi_refs_device,
hmme_refine_frame_bi_refs_device and their host-array forms): with one plane in the other list bit for bit the single-reference calls
Engine.search_frame_bi / refine_frame_bi per reference; with several, the per-CTU calls Engine.search_ctu / refine_ctu on the origin
2 * cur - P built here, P = hmo_pred_block_qpel block by block from the plane the block's index names -- inside the picture what
Engine.predict_refs_frame writes.  This is the way tests/test_gpu_bipred_frame.py checks the single-reference call.  Every comparison is
bit-exact."""
import ctypes as C

import numpy as np
import pytest

import bipred_refs_bands as bands
import predict_bi_refs_model as pbrm
import select_dirs_refs_model as drm
import select_refs_model as srm
from bipred_refs_bands import refs_prediction
from frame_helpers import bind_hmo, dims, mkplane, origin_picture, random_field

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (100, 70), (136, 72))
SR_UNI, SR_BI = 8, 4


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


def pictures(w, h, bd, seed, n):
    """n padded pictures of one scene, each moved as a whole and region by region: picture 0 serves as the current one"""
    from hmme import synth
    return [synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=3, region=32, shift=((5 * k) % 7 - 3, (3 * k) % 5 - 2), pad=12)[0] for k in range(n)]


def unrelated(w, h, bd, seed, n):
    """n padded pictures of DIFFERENT content"""
    from hmme import synth
    return [synth.make_pair(w, h, seed=seed + 13 * k, bit_depth=bd, max_mv=2)[1] for k in range(n)]


def per_ctu(engine, org, ref, w, h, bd, sr, center, pred, fen, ctus, int_mv=None, had=True):
    """Engine.search_ctu (int_mv None) or Engine.refine_ctu per CTU on the origin `org` (sample (0, 0) at [0, 0]) against the padded `ref`"""
    from hmme import api, synth
    m = synth.MARGIN
    cx_n, _ = dims(w, h)
    mv, cost = np.zeros((len(ctus), 593, 2), np.int16), np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        qx, qy = (int(center[ctu, 0]), int(center[ctu, 1])) if center is not None else (px, py)
        p = api.SearchParams(*api.set_search_range(qx, qy, sr, x, y, w, h), px, py, fen, bd)
        if int_mv is None:
            mv[k], cost[k] = engine.search_ctu(org, (x, y), ref, (m + x, m + y), p)
        else:
            mv[k], cost[k] = engine.refine_ctu(org, (x, y), ref, (m + x, m + y), p, int_mv[k], use_hadamard=had)
    return mv, cost


def predictors(n_refs, n_ctu, seed):
    from hmme import synth
    return np.stack([synth.random_predictors(n_ctu, seed=seed + r, max_pel=6) for r in range(n_refs)])


def checkerboard(n_ctu, per, n_others, w):
    """reference indices that change from block to block, every plane named; one MV per CTU: from CTU to CTU"""
    b = np.arange(per)
    c = np.arange(n_ctu)[:, None]
    return (((b % 8) + (b // 8) + c) % n_others).astype(np.uint8) if per == 64 else (c % n_others).astype(np.uint8).reshape(n_ctu, 1)


def select_refs_field(engine, cur_plane, other_planes, w, h):
    """a field and its reference indices out of the uni pass of the other list: search, refinement, hmme_select_refs_frame"""
    from hmme import api
    mv, _ = engine.search_frame_multi(cur_plane, other_planes, SR_UNI)
    q = [engine.refine_frame(cur_plane, p, SR_UNI, mv[k]) for k, p in enumerate(other_planes)]
    field, ref, _, _ = engine.select_refs_frame(w, h, api.SelectParams(64), np.stack([a for a, _ in q]), np.stack([c for _, c in q]))
    return field, ref


def check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, refs_i, others_i, field, ref_field, seed, fen=1, had=True, ctus=None, sr=SR_BI):
    """both calls over the references pics[refs_i] against pics[others_i] with the given field -> the four tables, checked on `ctus`"""
    n_ctu = dims(w, h)[0] * dims(w, h)[1]
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        refs, others = [planes[i] for i in refs_i], [planes[i] for i in others_i]
        pred, center = predictors(len(refs), n_ctu, seed), predictors(len(refs), n_ctu, seed + 50)
        mv, sad = engine.search_frame_bi_refs(planes[0], refs, others, sr, field, ref_field, center_q=center, pred_q=pred, fen=fen)
        qmv, cost = engine.refine_frame_bi_refs(planes[0], refs, others, sr, field, ref_field, mv, center_q=center, pred_q=pred, use_hadamard=had)
        f3 = field.reshape(n_ctu, -1, 2)
        rf = np.asarray(ref_field).reshape(n_ctu, -1)
        p_full = refs_prediction(hmo, [pics[i] for i in others_i], w, h, bd, f3, rf)
        # inside the picture, where the index names a plane, P is hmme_predict_refs_device's prediction
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0xA5A5)
        pr = engine.predict_refs_frame(others, f3 if f3.shape[1] == 64 else f3[:, 0], rf, out=np.full((h, w), fill, dt))
        if f3.shape[1] == 64:
            cx_n, cy_n = dims(w, h)
            blocks = rf.reshape(cy_n, cx_n, 8, 8).transpose(0, 2, 1, 3).reshape(cy_n * 8, cx_n * 8)      # the index of every 8x8 block of the CTU grid
            named = np.repeat(np.repeat(blocks, 8, axis=0), 8, axis=1)[:h, :w] < len(others)
            assert named.any() and np.array_equal(pr[named].astype(np.int16), p_full[:h, :w][named]) and (pr[~named] == fill).all()
        org = origin_picture(pics[0], p_full, w, h)
        for r, i in enumerate(refs_i):
            todo = range(n_ctu) if ctus is None else ctus
            smv, ssad = per_ctu(engine, org, pics[i], w, h, bd, sr, center[r], pred[r], fen, todo)
            assert np.array_equal(mv[r][list(todo)], smv) and np.array_equal(sad[r][list(todo)], ssad), ("search", r)
            sq, sc = per_ctu(engine, org, pics[i], w, h, bd, sr, center[r], pred[r], fen, todo, mv[r][list(todo)], had)
            assert np.array_equal(qmv[r][list(todo)], sq) and np.array_equal(cost[r][list(todo)], sc), ("refine", r)
        return mv, sad, qmv, cost
    finally:
        for p in planes:
            p.close()


# ---- 1: one plane in the other list: the single-reference calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("bd", [8, 10])
def test_with_one_other_plane_it_is_the_single_reference_call(engine, bd, w, h):
    n_ctu = dims(w, h)[0] * dims(w, h)[1]
    per = 64 if (w + bd) % 4 else 1
    pics = pictures(w, h, bd, 2000 + w + bd, 5)
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        cur, refs, other = planes[0], planes[1:4], planes[4]
        field = random_field(n_ctu, per, 2010 + w)
        rng = np.random.default_rng(2011)
        ref_field = rng.choice(np.array([0, 0xFF, 1, 7], np.uint8), size=(n_ctu, per))   # one plane: whatever the index, it is read
        pred, center = predictors(3, n_ctu, 2020), predictors(3, n_ctu, 2030)
        mv, sad = engine.search_frame_bi_refs(cur, refs, [other], SR_BI, field, ref_field, center_q=center, pred_q=pred, fen=1)
        qmv, cost = engine.refine_frame_bi_refs(cur, refs, [other], SR_BI, field, ref_field, mv, center_q=center, pred_q=pred)
        for r in range(3):
            smv, ssad = engine.search_frame_bi(cur, refs[r], other, SR_BI, field, center_q=center[r], pred_q=pred[r], fen=1)
            assert np.array_equal(mv[r], smv) and np.array_equal(sad[r], ssad), r
            sq, sc = engine.refine_frame_bi(cur, refs[r], other, SR_BI, field, smv, center_q=center[r], pred_q=pred[r])
            assert np.array_equal(qmv[r], sq) and np.array_equal(cost[r], sc), r
        assert not np.array_equal(mv[0], mv[1]) and not np.array_equal(cost[1], cost[2])
        # NULL centres and predictors are the single-reference call's, too
        mv0, sad0 = engine.search_frame_bi_refs(cur, refs[:1], [other], SR_BI, field, ref_field, fen=0)
        smv, ssad = engine.search_frame_bi(cur, refs[0], other, SR_BI, field, fen=0)
        assert np.array_equal(mv0[0], smv) and np.array_equal(sad0[0], ssad)
    finally:
        for p in planes:
            p.close()


# ---- 2: several planes of different content in the other list: the per-CTU calls on the origin -------------------------------------------------
@pytest.mark.parametrize("n_others", [2, 4])
@pytest.mark.parametrize("w,h,bd,per", [(64, 64, 10, 64), (100, 70, 8, 64), (136, 72, 8, 1), (136, 72, 10, 64)])
def test_a_checkerboard_of_references_equals_the_per_ctu_calls(engine, hmo, w, h, bd, per, n_others):
    n_ctu = dims(w, h)[0] * dims(w, h)[1]
    pics = pictures(w, h, bd, 2100 + w + bd, 3) + unrelated(w, h, bd, 2150 + w, n_others)
    others_i = list(range(3, 3 + n_others))
    field = random_field(n_ctu, per, 2110 + w + n_others)
    ref_field = checkerboard(n_ctu, per, n_others, w)
    assert set(ref_field.reshape(-1).tolist()) == set(range(n_others))
    mv, sad, qmv, cost = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, [1, 2], others_i, field, ref_field, 2120 + n_others, fen=n_others // 4,
                                                         had=bool(per == 64))
    # the index matters: the same field read from plane 0 alone gives other tables
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        flat, _ = engine.search_frame_bi_refs(planes[0], planes[1:3], [planes[i] for i in others_i], SR_BI, field, np.zeros_like(ref_field), fen=n_others // 4)
        again, _ = engine.search_frame_bi_refs(planes[0], planes[1:3], [planes[i] for i in others_i], SR_BI, field, ref_field, fen=n_others // 4)
        assert not np.array_equal(flat, again)
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("w,h,bd", [(100, 70, 10), (136, 72, 8)])
def test_a_field_out_of_select_refs_frame_equals_the_per_ctu_calls(engine, hmo, w, h, bd):
    """the other list's uni pass gives the field: its 0xFF (blocks of CUs that do not exist, outside the picture, MV (0,0)) reads reference 0"""
    from hmme import synth
    pics = pictures(w, h, bd, 2200 + w, 7)
    for k, noise in enumerate(unrelated(w, h, bd, 2250 + w, 4)):               # other k shows the scene in the k-th quarter of the width only
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
    mv, sad, qmv, cost = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, [1, 2], [3, 4, 5, 6], field, ref_field, 2220)
    # ... which is what the same field gives with index 0 in their place
    zeroed = np.where(ref_field == 0xFF, 0, ref_field).astype(np.uint8)
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        mv0, sad0 = engine.search_frame_bi_refs(planes[0], planes[1:3], planes[3:7], SR_BI, field, zeroed, center_q=predictors(2, mv.shape[1], 2270),
                                                pred_q=predictors(2, mv.shape[1], 2220), fen=1)
        assert np.array_equal(mv0, mv) and np.array_equal(sad0, sad)
    finally:
        for p in planes:
            p.close()


# ---- 3: launch shapes: 1, 3 and 16 references, a CTU sub-range, the device entry, a used context ------------------------------------------------
def test_sixteen_references_a_sub_range_and_the_device_entry(engine, hmo):
    import torch
    from hmme import api
    w, h, bd, n_ctu = 136, 72, 8, 6
    dev = torch.device("cuda", 0)
    pics = pictures(w, h, bd, 2300, 5) + unrelated(w, h, bd, 2350, 3)
    planes = [mkplane(engine, p, w, h, bd) for p in pics]
    try:
        cur, others = planes[0], planes[5:8]
        sixteen = [planes[1 + k % 4] for k in range(16)]
        field, ref_field = random_field(n_ctu, 64, 2310), checkerboard(n_ctu, 64, 3, w)
        pred, center = predictors(16, n_ctu, 2320), predictors(16, n_ctu, 2340)
        for k in range(4, 16):                                                 # the same plane, predictor and centre: the same table
            pred[k], center[k] = pred[k % 4], center[k % 4]
        mv, sad = engine.search_frame_bi_refs(cur, sixteen, others, SR_BI, field, ref_field, center_q=center, pred_q=pred, fen=1)
        qmv, cost = engine.refine_frame_bi_refs(cur, sixteen, others, SR_BI, field, ref_field, mv, center_q=center, pred_q=pred)
        for k in range(4, 16):
            assert np.array_equal(mv[k], mv[k % 4]) and np.array_equal(sad[k], sad[k % 4]) and np.array_equal(qmv[k], qmv[k % 4]) and np.array_equal(cost[k], cost[k % 4])
        # 1 and 3 references: the first tables of the 16
        for n in (1, 3):
            a, b = engine.search_frame_bi_refs(cur, sixteen[:n], others, SR_BI, field, ref_field, center_q=center[:n], pred_q=pred[:n], fen=1)
            q, c = engine.refine_frame_bi_refs(cur, sixteen[:n], others, SR_BI, field, ref_field, a, center_q=center[:n], pred_q=pred[:n])
            assert np.array_equal(a, mv[:n]) and np.array_equal(b, sad[:n]) and np.array_equal(q, qmv[:n]) and np.array_equal(c, cost[:n])
        # ... pinned to the per-CTU calls on two CTUs of three references
        org = origin_picture(pics[0], refs_prediction(hmo, pics[5:8], w, h, bd, field, ref_field), w, h)
        for r in range(3):
            smv, ssad = per_ctu(engine, org, pics[1 + r], w, h, bd, SR_BI, center[r], pred[r], 1, [1, 5])
            assert np.array_equal(mv[r][[1, 5]], smv) and np.array_equal(sad[r][[1, 5]], ssad)
            sq, sc = per_ctu(engine, org, pics[1 + r], w, h, bd, SR_BI, center[r], pred[r], 1, [1, 5], mv[r][[1, 5]])
            assert np.array_equal(qmv[r][[1, 5]], sq) and np.array_equal(cost[r][[1, 5]], sc)
        # a CTU sub-range == the same rows of the full call, host form and device form
        first, count = 1, 4
        a, b = engine.search_frame_bi_refs(cur, sixteen[:3], others, SR_BI, field, ref_field, center_q=center[:3], pred_q=pred[:3], fen=1, ctu_first=first, ctu_count=count)
        q, c = engine.refine_frame_bi_refs(cur, sixteen[:3], others, SR_BI, field, ref_field, a, center_q=center[:3], pred_q=pred[:3], ctu_first=first, ctu_count=count)
        rows = slice(first, first + count)
        assert np.array_equal(a, mv[:3, rows]) and np.array_equal(b, sad[:3, rows]) and np.array_equal(q, qmv[:3, rows]) and np.array_equal(c, cost[:3, rows])
        d_f, d_r, d_p, d_c = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (field, ref_field, pred[:3], center[:3]))
        d_mv = torch.zeros((3, count, 593, 2), dtype=torch.int16, device=dev)
        d_sad = torch.zeros((3, count, 593), dtype=torch.int32, device=dev)
        d_q, d_cc = torch.zeros_like(d_mv), torch.zeros_like(d_sad)
        torch.cuda.synchronize()
        fp = api.FrameParams(SR_BI, 1, bd, first, count)
        engine.search_frame_bi_refs_device(cur, sixteen[:3], others, fp, d_f.data_ptr(), d_r.data_ptr(), 64, d_c.data_ptr(), d_p.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_frame_bi_refs_device(cur, sixteen[:3], others, fp, d_f.data_ptr(), d_r.data_ptr(), 64, d_c.data_ptr(), d_p.data_ptr(), d_mv.data_ptr(), 1,
                                           d_q.data_ptr(), d_cc.data_ptr(), 0)
        torch.cuda.synchronize()
        assert np.array_equal(d_mv.cpu().numpy(), a) and np.array_equal(d_sad.cpu().numpy().view(np.uint32), b)
        assert np.array_equal(d_q.cpu().numpy(), q) and np.array_equal(d_cc.cpu().numpy().view(np.uint32), c)
        # a used context gives what a fresh one gives
        fresh = api.Engine(0, 64)
        fresh.set_lambda_q16(engine.lambda_q16)
        fplanes = [mkplane(fresh, p, w, h, bd) for p in pics]
        try:
            fa, fb = fresh.search_frame_bi_refs(fplanes[0], fplanes[1:4], fplanes[5:8], SR_BI, field, ref_field, center_q=center[:3], pred_q=pred[:3], fen=1)
            fq, fc = fresh.refine_frame_bi_refs(fplanes[0], fplanes[1:4], fplanes[5:8], SR_BI, field, ref_field, fa, center_q=center[:3], pred_q=pred[:3])
            assert np.array_equal(fa, mv[:3]) and np.array_equal(fb, sad[:3]) and np.array_equal(fq, qmv[:3]) and np.array_equal(fc, cost[:3])
        finally:
            for p in fplanes:
                p.close()
            fresh.close()
    finally:
        for p in planes:
            p.close()


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------------------
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

    eng2 = api.Engine(0, 64)
    a, b, c, small, deep, foreign = engine.plane(w, h), engine.plane(w, h), engine.plane(w, h), engine.plane(64, 64), engine.plane(w, h, 10), eng2.plane(w, h)
    p12 = [engine.plane(w, h, 12) for _ in range(3)]
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        fp = api.FrameParams(SR_BI, 1, 8, 0, n_ctu)

        def both(cur, refs, others, fp=fp, f=d_f.data_ptr(), r=d_r.data_ptr(), per=64, mv=t_mv.data_ptr(), cost=t_c.data_ptr(), imv=d_imv.data_ptr(), n_refs=None, n_others=None):
            ra, oa = api._handles(refs), api._handles(others)
            nr, no = len(refs) if n_refs is None else n_refs, len(others) if n_others is None else n_others
            s = L.hmme_search_frame_bi_refs_device(engine.h, cur.h if cur else None, ra, nr, oa, no, C.byref(fp), f, r, per, None, None, mv, cost, None)
            q = L.hmme_refine_frame_bi_refs_device(engine.h, cur.h if cur else None, ra, nr, oa, no, C.byref(fp), f, r, per, None, None, imv, 1, mv, cost, None)
            return s, q

        # every plane of `others` -- not the first alone: one size, fp's bit depth, this context
        for refs, others in (([a], [b, small]), ([a], [small]), ([a], [b, deep]), ([a], [b, c, foreign]), ([a, small], [b]), ([a, deep], [b]), ([foreign], [b])):
            assert both(c, refs, others) == (-1, -1), (refs, others)
        assert both(None, [a], [b]) == (-1, -1)
        assert both(c, [a], [b], r=None) == (-1, -1) and both(c, [a], [b], f=None) == (-1, -1) and both(c, [a], [b], per=4) == (-1, -1)   # a NULL d_other_ref
        assert both(c, [a], [b], n_refs=0) == (-1, -1) and both(c, [a] * 16, [b], n_refs=17) == (-1, -1)
        assert both(c, [a], [b], n_others=0) == (-1, -1) and both(c, [a], [b] * 16, n_others=17) == (-1, -1)
        assert both(c, [a], [b], mv=None) == (-1, -1) and both(c, [a], [b], cost=None) == (-1, -1)
        assert L.hmme_refine_frame_bi_refs_device(engine.h, c.h, api._handles([a]), 1, api._handles([b]), 1, C.byref(fp), d_f.data_ptr(), d_r.data_ptr(), 64, None, None,
                                                  None, 1, t_mv.data_ptr(), t_c.data_ptr(), None) == -1      # no integer MVs
        assert both(c, [a], [b], fp=api.FrameParams(SR_BI, 1, 8, 5, 2)) == (-1, -1)   # a CTU range outside the picture
        assert both(c, [a], [b], fp=api.FrameParams(SR_BI, 1, 7, 0, n_ctu)) == (-1, -1)
        assert both(c, [a], [b], fp=api.FrameParams(65, 1, 8, 0, n_ctu)) == (-1, -1)  # beyond the context's range
        # hmme_bipred_check runs first, with refine = 1 in the refinement: 12 bits are searched and not refined
        assert api.bipred_check(12, True) == -5 and api.bipred_check(12, False) == 0
        fp12 = api.FrameParams(SR_BI, 1, 12, 0, n_ctu)
        assert L.hmme_refine_frame_bi_refs_device(engine.h, p12[0].h, api._handles(p12[1:2]), 1, api._handles(p12[2:]), 1, C.byref(fp12), d_f.data_ptr(), d_r.data_ptr(), 64,
                                                  None, None, d_imv.data_ptr(), 1, t_mv.data_ptr(), t_c.data_ptr(), None) == -5
        with pytest.raises(api.HmmeError):
            engine.refine_frame_bi_refs(p12[0], p12[1:2], p12[2:], SR_BI, np.zeros((n_ctu, 2), np.int16), np.zeros((n_ctu, 1), np.uint8), np.zeros((1, n_ctu, 593, 2), np.int16))
        with pytest.raises(api.HmmeError):
            engine.search_frame_bi_refs(c, [a], [b, small], SR_BI, np.zeros((n_ctu, 2), np.int16), np.zeros((n_ctu, 1), np.uint8))
        assert untouched()
        assert both(c, [a, b], [b, a]) == (0, 0)                                 # the accepted neighbour does run
        torch.cuda.synchronize()
        assert not bool((t_c[:2] == 0x5A5A5A5A).any()) and bool((t_c[2:] == 0x5A5A5A5A).all())
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in [a, b, c, small, deep, foreign] + p12:
            p.close()
        eng2.close()


# ---- 5: end to end ------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_planted_bands(engine, hmo):
    """tests/bipred_refs_bands.py through the six steps of include/hmme.h on device buffers: the outputs equal the models' on the downloaded
    tables, and every block well inside a band carries the planted direction and reference indices (tests/test_select_dirs_refs_cpu.py shows
    that the numpy route alone does that on this content)"""
    import torch
    from hmme import api
    W, H, n, R = bands.W, bands.H, bands.N, bands.R
    dev = torch.device("cuda", 0)
    cur_pic, lists_pic = bands.content()
    lq = drm.LAMBDA_Q16
    prev = engine.lambda_q16
    engine.set_lambda_q16(lq)
    cur = mkplane(engine, cur_pic, W, H, 8)
    lists = [[mkplane(engine, p, W, H, 8) for p in lists_pic[l]] for l in range(2)]
    try:
        fp, fp_bi, sel, bits = api.FrameParams(bands.SR_UNI, 1, 8, 0, n), api.FrameParams(bands.SR_BI, 1, 8, 0, n), api.SelectParams(64), bands.bits()
        tab = lambda: (torch.zeros((2, R, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((2, R, n, 593), dtype=torch.int32, device=dev))
        (d_mv, d_sad), (d_q, d_c), (d_bmv, d_bsad), (d_bq, d_bc) = tab(), tab(), tab(), tab()
        d_uni = torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev)
        d_uref = torch.zeros((2, n, 64), dtype=torch.uint8, device=dev)
        d_field = torch.full((1, 2, n, 64, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_ref = torch.full((1, 2, n, 64), 0x6B, dtype=torch.uint8, device=dev)
        d_dir = torch.full((1, n, 64), 0xA7, dtype=torch.uint8, device=dev)
        d_slot = torch.zeros((1, n, 64), dtype=torch.int16, device=dev)
        d_cc = torch.zeros((1, n), dtype=torch.int32, device=dev)
        d_img = torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev)
        d_res = torch.full((H, W), 0x7777, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        for l in range(2):                                                      # 1: the uni pass of each list over its references
            engine.search_frame_multi_device(cur, lists[l], fp, None, d_mv[l].data_ptr(), d_sad[l].data_ptr(), 0)
            engine.refine_frame_multi_device(cur, lists[l], fp, None, d_mv[l].data_ptr(), 1, d_q[l].data_ptr(), d_c[l].data_ptr(), 0)
        # 2: the reference per PU, the two lists as the call's two "pictures"
        engine.select_refs_device(W, H, 2, R, fp, sel, srm.hm_ref_cost(R, lq), d_q.data_ptr(), d_c.data_ptr(), None, d_uni.data_ptr(), d_uref.data_ptr(), None, None, 0)
        for l in range(2):                                                      # 3: the bi pass of list l against list 1-l's field and indices
            engine.search_frame_bi_refs_device(cur, lists[l], lists[1 - l], fp_bi, d_uni[1 - l].data_ptr(), d_uref[1 - l].data_ptr(), 64, None, None,
                                               d_bmv[l].data_ptr(), d_bsad[l].data_ptr(), 0)
            engine.refine_frame_bi_refs_device(cur, lists[l], lists[1 - l], fp_bi, d_uni[1 - l].data_ptr(), d_uref[1 - l].data_ptr(), 64, None, None,
                                               d_bmv[l].data_ptr(), 1, d_bq[l].data_ptr(), d_bc[l].data_ptr(), 0)
        # 4: direction and reference per PU; 5: the prediction; 6: the residual
        engine.select_dirs_refs_device(W, H, 1, R, fp, sel, [api.DirRefsParams(bits.dir_bits, bits.n_refs, bits.ref_bits, bits.l1_valid_mask)], d_q.data_ptr(), d_c.data_ptr(),
                                       d_bq.data_ptr(), d_bc.data_ptr(), d_uni.data_ptr(), d_uref.data_ptr(), None, d_field.data_ptr(), d_ref.data_ptr(), d_dir.data_ptr(),
                                       d_slot.data_ptr(), d_cc.data_ptr(), 0)
        engine.predict_bi_refs_device(lists[0], lists[1], fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), W, 0)
        engine.residual_pairs_device([cur], [d_img.data_ptr()], W, fp, d_slot.data_ptr(), 64, 1, [d_res.data_ptr()], 2 * W, None, None, None, 0)
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()
        mv_uni, cost_uni, mv_bi, cost_bi = host(d_q), host(d_c).view(np.uint32), host(d_bq), host(d_bc).view(np.uint32)
        uni_field, uni_ref = host(d_uni), host(d_uref)
        # the device's steps against the models on the downloaded tables
        for l in range(2):
            f, r, _, _, _ = srm.select_refs_picture(mv_uni[l], cost_uni[l], sel, W, H, srm.hm_ref_cost(R, lq), 0, None, lq, None)
            assert np.array_equal(uni_field[l], f) and np.array_equal(uni_ref[l], r), l
        mf, mr, md, ms, mc = drm.select_dirs_refs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, W, H, bits, 0, None, lq)
        assert np.array_equal(host(d_field)[0], mf) and np.array_equal(host(d_ref)[0], mr) and np.array_equal(host(d_dir)[0], md)
        assert np.array_equal(host(d_slot)[0].view(np.uint16), ms) and np.array_equal(host(d_cc)[0].view(np.uint32), mc)
        pred = host(d_img)
        assert np.array_equal(pred, pbrm.pred_picture(hmo, lists_pic[0], lists_pic[1], W, H, 8, mf, md, mr, np.full((H, W), 0xEE, np.int64)))
        m = (cur_pic.shape[0] - H) // 2
        assert np.array_equal(host(d_res), cur_pic[m:m + H, m:m + W].astype(np.int16) - pred.astype(np.int16))
        # the bi tables are the per-CTU calls' on the origin of the downloaded field (list 0 searched, both references, two CTUs)
        org = origin_picture(cur_pic, refs_prediction(hmo, lists_pic[1], W, H, 8, uni_field[1], uni_ref[1]), W, H)
        for r in range(R):
            smv, ssad = per_ctu(engine, org, lists_pic[0][r], W, H, 8, bands.SR_BI, None, None, 1, [1, 4])
            assert np.array_equal(host(d_bmv)[0, r][[1, 4]], smv) and np.array_equal(host(d_bsad).view(np.uint32)[0, r][[1, 4]], ssad)
            sq, sc = per_ctu(engine, org, lists_pic[0][r], W, H, 8, bands.SR_BI, None, None, 1, [1, 4], smv)
            assert np.array_equal(mv_bi[0, r][[1, 4]], sq) and np.array_equal(cost_bi[0, r][[1, 4]], sc)
        # the planted bands
        assert bands.bands_hold(md, mr) == [] and len(bands.planted_blocks()) >= 60
        sad = lambda p: int(np.abs(p.astype(np.int32) - cur_pic[m:m + H, m:m + W]).sum())
        assert sad(pred) < min(sad(engine.predict_refs_frame(lists[l], uni_field[l], uni_ref[l])) for l in range(2))
    finally:
        engine.set_lambda_q16(prev)
        for p in [cur] + lists[0] + lists[1]:
            p.close()
