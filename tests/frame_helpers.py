"""Oracle legs and plane plumbing shared by the whole-picture GPU tests (test_gpu_wp_frame.py, test_gpu_bipred_frame.py,
test_gpu_range_edges.py): hmo_search_ctu_w per CTU for the weighted search, hmo_pred_block_qpel for the prediction, hmo_search_ctu on the
origin 2 * cur - prediction built here in numpy for the bi search; hmo_search_ctu_w / hmo_frac_refine_w on an origin for the weighted bi
calls (test_gpu_bipred_wp.py, test_gpu_context_state.py)."""
import ctypes as C

import numpy as np


def bind_hmo(oracle_lib):
    """the oracle library with the two functions oracle_py leaves unbound"""
    L = oracle_lib.oracle()
    p16 = C.POINTER(C.c_int16)
    L.hmo_pred_block_qpel.restype = None
    L.hmo_pred_block_qpel.argtypes = [p16, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, p16, C.c_int]
    L.hmo_clip_mv.restype = None
    L.hmo_clip_mv.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)] + [C.c_int] * 5
    return L


def dims(w, h):
    return (w + 63) // 64, (h + 63) // 64


def ctu_origin(ctu, w):
    cx = (w + 63) // 64
    return (ctu % cx) * 64, (ctu // cx) * 64


def mkplane(engine, padded, w, h, bd):
    from hmme import synth
    m = synth.MARGIN
    p = engine.plane(w, h, bd)
    if bd == 8:
        p.upload_u8(padded[m:m + h, m:m + w].astype(np.uint8))
    else:
        p.upload_pel(padded, (m, m))
    return p


def device_tables(n_pairs, count, dev):
    import torch
    return (torch.zeros((n_pairs, count, 593, 2), dtype=torch.int16, device=dev), torch.zeros((n_pairs, count, 593), dtype=torch.int32, device=dev))


def oracle_search_w(oracle_lib, cur, ref, w, h, sr, pred, lq, bd, wp, ctus):
    """hmo_search_ctu_w per CTU: the CTU's 64x64 block of the padded current plane (partial CTUs completed by its edge replication), the padded
    reference, the window of hmme_set_search_range for the CTU's predictor"""
    from hmme import api, synth
    m = synth.MARGIN
    mv = np.zeros((len(ctus), 593, 2), np.int16)
    sad = np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        x, y = ctu_origin(ctu, w)
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        lt_x, lt_y, rb_x, rb_y = api.set_search_range(px, py, sr, x, y, w, h)
        p = oracle_lib.make_params((lt_x, lt_y), (rb_x, rb_y), (px, py), lq, 1, bd)   # FEN on: xGetSADw must not consult it
        ox, oy, osad = oracle_lib.search_ctu_w(cur, (m + x, m + y), ref, (m + x, m + y), p, wp)
        mv[k, :, 0], mv[k, :, 1], sad[k] = ox, oy, osad
    return mv, sad


def clip_mv(hmo, qx, qy, cu_x, cu_y, w, h):
    a, b = C.c_int(int(qx)), C.c_int(int(qy))
    hmo.hmo_clip_mv(C.byref(a), C.byref(b), cu_x, cu_y, w, h, 64)
    return a.value, b.value


def as_field(field, n_ctu):
    f = np.asarray(field, np.int16)
    return f.reshape(n_ctu, 1, 2) if f.ndim == 2 else f


def oracle_prediction(hmo, ref, w, h, bd, field):
    """hmo_pred_block_qpel for every CTU of the picture, whole 64x64 blocks (partial edge CTUs too: the padded plane serves them), at the
    MV hmo_clip_mv gives for the CTU.  field: [n_ctu, 1 | 64, 2].  -> int16 [ctus_y * 64, ctus_x * 64]"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    field = as_field(field, cx_n * cy_n)
    out = np.zeros((cy_n * 64, cx_n * 64), np.int16)
    rs, os_ = ref.shape[1], out.shape[1]
    p16 = C.POINTER(C.c_int16)
    for ctu in range(cx_n * cy_n):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        if field.shape[1] == 1:
            blocks = [(0, 0, 64, field[ctu, 0])]
        else:
            blocks = [((b & 7) * 8, (b >> 3) * 8, 8, field[ctu, b]) for b in range(64)]
        for bx, by, n, mv in blocks:
            qx, qy = clip_mv(hmo, mv[0], mv[1], cu_x, cu_y, w, h)
            src = C.cast(ref.ctypes.data + 2 * ((m + cu_y + by) * rs + m + cu_x + bx), p16)
            dst = C.cast(out.ctypes.data + 2 * ((cu_y + by) * os_ + cu_x + bx), p16)
            hmo.hmo_pred_block_qpel(src, rs, n, n, qx, qy, bd, dst, os_)
    return out


def origin_picture(cur, pred_full, w, h):
    """2 * B - P per CTU block, B = the CTU's 64x64 block of the padded current plane (its edge replication completes partial CTUs)"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    b = cur[m:m + cy_n * 64, m:m + cx_n * 64].astype(np.int32)
    return np.ascontiguousarray((2 * b - pred_full).astype(np.int16))


def oracle_bi_search(oracle_lib, org, ref, w, h, sr, center, pred, lq, fen, bd, ctus):
    from hmme import api, synth
    m = synth.MARGIN
    cx_n, _ = dims(w, h)
    mv = np.zeros((len(ctus), 593, 2), np.int16)
    sad = np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        qx, qy = (int(center[ctu, 0]), int(center[ctu, 1])) if center is not None else (px, py)
        lt_x, lt_y, rb_x, rb_y = api.set_search_range(qx, qy, sr, x, y, w, h)
        p = oracle_lib.make_params((lt_x, lt_y), (rb_x, rb_y), (px, py), lq, fen, bd)
        ox, oy, osad = oracle_lib.search_ctu(org, (x, y), ref, (m + x, m + y), p)
        mv[k, :, 0], mv[k, :, 1], sad[k] = ox, oy, osad
    return mv, sad


def oracle_origin_search_w(oracle_lib, org, ref, w, h, sr, center, pred, lq, bd, wp, ctus):
    """hmo_search_ctu_w per CTU on an origin `org` (sample (0, 0) at [0, 0]: a bi-prediction origin, or a picture's CTU blocks), window
    around the centre (None: the predictor), FEN on: xGetSADw must not consult it"""
    from hmme import api, synth
    m = synth.MARGIN
    cx_n, _ = dims(w, h)
    mv = np.zeros((len(ctus), 593, 2), np.int16)
    sad = np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        x, y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        px, py = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        qx, qy = (int(center[ctu, 0]), int(center[ctu, 1])) if center is not None else (px, py)
        lt_x, lt_y, rb_x, rb_y = api.set_search_range(qx, qy, sr, x, y, w, h)
        p = oracle_lib.make_params((lt_x, lt_y), (rb_x, rb_y), (px, py), lq, 1, bd)
        ox, oy, osad = oracle_lib.search_ctu_w(org, (x, y), ref, (m + x, m + y), p, wp)
        mv[k, :, 0], mv[k, :, 1], sad[k] = ox, oy, osad
    return mv, sad


def oracle_origin_refine_w(oracle_lib, org, ref, w, h, int_mv, pred, lq, had, bd, wp, ctus):
    """hmo_frac_refine_w per slot on the origin -> (qmv [len(ctus), 593, 2], cost [len(ctus), 593])"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, _ = dims(w, h)
    table = oracle_lib.slot_table()
    qmv = np.zeros((len(ctus), 593, 2), np.int16)
    cost = np.zeros((len(ctus), 593), np.uint32)
    for k, ctu in enumerate(ctus):
        cx, cy = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        pq = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        for s in range(593):
            x, y, bw, bh = (int(v) for v in table[s])
            imv = (int(int_mv[k, s, 0]), int(int_mv[k, s, 1]))
            hx, hy, qx, qy, c = oracle_lib.frac_refine_w(org, (cx + x, cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, pq, lq, had, bd, wp)
            qmv[k, s] = (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy)
            cost[k, s] = c
    return qmv, cost


def check_strided_image(w, h, bd, wrapper, entry, spare=24):
    """A host prediction call into an image whose stride exceeds the picture width (the Python wrappers always pass the width), once over the
    whole picture and once over CTU 1 alone.  wrapper(out, ctu_first, ctu_count) -> the Python method's result into the contiguous `out`;
    entry(fp, out_address, out_stride) -> the return code of the C entry.  The picture columns equal the contiguous result bit for bit; the
    spare columns, and the picture outside the CTU range, keep the sentinel."""
    from hmme import api
    dt, sentinel = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0xA5A5)
    for first, count in ((0, -1), (1, 1)):
        want = wrapper(np.full((h, w), sentinel, dt), first, count)
        img = np.full((h, w + spare), sentinel, dt)
        assert entry(api.FrameParams(1, 0, bd, first, count), img.ctypes.data, w + spare) == 0
        assert np.array_equal(img[:, :w], want) and (want != sentinel).any()
        assert (img[:, w:] == sentinel).all()
        if count > 0:
            inside = np.zeros((h, w), bool)
            for ctu in range(first, first + count):
                x, y = ctu_origin(ctu, w)
                inside[y:y + 64, x:x + 64] = True
            assert (img[:, :w][~inside] == sentinel).all()


def random_field(n_ctu, per, seed, max_pel=6):
    rng = np.random.default_rng(seed)
    return rng.integers(-4 * max_pel, 4 * max_pel + 1, size=(n_ctu, per, 2)).astype(np.int16)


def three_planes(w, h, bd, seed, max_mv=5):
    """cur, ref (a moved copy of cur's texture) and an `other` picture of the same scene moved differently"""
    from hmme import synth
    cur, ref, _ = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=max_mv, region=64)
    _, other, _ = synth.make_pair(w, h, seed=seed + 1000, bit_depth=bd, max_mv=max_mv, region=64)
    return cur, ref, other


def run_bi_search(engine, oracle_lib, hmo, w, h, bd, sr, fen, per, seed, with_center=True, planes3=None):
    """search_frame_bi on three pictures against the oracle on the origin built here, all CTUs and slots -> what was used and found"""
    from hmme import synth
    cx_n, cy_n = dims(w, h)
    n_ctu = cx_n * cy_n
    cur, ref, other = planes3 if planes3 is not None else three_planes(w, h, bd, seed)
    field = random_field(n_ctu, per, seed + 1)
    pred = synth.random_predictors(n_ctu, seed=seed + 2, max_pel=8)
    center = synth.random_predictors(n_ctu, seed=seed + 3, max_pel=8) if with_center else None
    if center is not None:
        assert np.any(center != pred)
    org = origin_picture(cur, oracle_prediction(hmo, other, w, h, bd, field), w, h)
    pc, pr, po = (mkplane(engine, a, w, h, bd) for a in (cur, ref, other))
    try:
        mv, sad = engine.search_frame_bi(pc, pr, po, sr, field, center_q=center, pred_q=pred, fen=fen)
    finally:
        pc.close(); pr.close(); po.close()
    omv, osad = oracle_bi_search(oracle_lib, org, ref, w, h, sr, center, pred, engine.lambda_q16, fen, bd, range(n_ctu))
    assert np.array_equal(mv, omv), (bd, sr, fen, np.argwhere(mv != omv)[:4])
    assert np.array_equal(sad, osad), (bd, sr, fen, np.argwhere(sad != osad)[:4])
    return dict(cur=cur, ref=ref, other=other, field=field, pred=pred, center=center, org=org, mv=mv)
