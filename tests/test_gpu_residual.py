"""Residual and per-PU / per-CU distortion of a prediction on the device (hmme_residual_pairs_device, hmme_residual_frame) against
tests/residual_model.py, the rule of include/hmme.h restated in numpy with the oracle's hmo_had / hmo_sad.  Every comparison is bit-exact.
Slot maps come from real decisions: search -> refinement -> select_frame on synthetic pairs, the predicted image from predict_frame.  Cases
assert on the MODEL's inputs that they exercise what they are about, so a degenerate decision cannot pass silently."""
import ctypes as C

import numpy as np
import pytest

import residual_model as rm

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (100, 70), (136, 72)]     # one CTU; both edges partial, a height that is no multiple of 4; 3 x 2 CTUs
BDS = [8, 10, 12]
R_FILL, U_FILL, P_FILL = 0x5A5A, 0x0BADBEEF, 0xA5     # sentinels: residual (|D| <= 4095 never reaches it), the uint32 outputs, spare image columns
ERR_ARG = -1


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(57.9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return oracle_lib.oracle()


@pytest.fixture(scope="module")
def scenes(engine):
    """(w, h, bd) -> the pair's planes and pictures, its refinement tables and the default 8x8 decision with its prediction; made once, never
    modified, the planes closed at the end of the module"""
    from hmme import api, synth
    made = {}

    def get(w, h, bd, seed=0):
        key = (w, h, bd, seed)
        if key not in made:
            m = synth.MARGIN
            cur, ref, _ = synth.make_pair(w, h, seed=300 + w + bd + seed, bit_depth=bd, max_mv=4, region=16)
            pc, pr = engine.plane(w, h, bd), engine.plane(w, h, bd)
            pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
            mv, _ = engine.search_frame(pc, pr, 8)
            qmv, cost = engine.refine_frame(pc, pr, 8, mv)
            field, slot, _ = engine.select_frame(w, h, api.SelectParams(64), qmv, cost)
            pred = engine.predict_frame(pr, field)
            s = dict(w=w, h=h, bd=bd, pc=pc, pr=pr, cur=cur[m:m + h, m:m + w].copy(), qmv=qmv, cost=cost, slot64=slot, pred=pred)
            for a in (s["cur"], qmv, cost, slot, pred):
                a.setflags(write=False)
            made[key] = s
        return made[key]

    yield get
    for s in made.values():
        s["pc"].close(); s["pr"].close()


def decide(engine, s, sel, cost=None):
    """the decision `sel` over the scene's tables (cost: an edited copy) -> (slot map [n_ctu, per], predicted image).  With one MV per 8x8 block
    the prediction is the decision's own; the 4x4 form (no predict call takes its field) is measured against the scene's default prediction --
    the rule takes any image"""
    field, slot, _ = engine.select_frame(s["w"], s["h"], sel, s["qmv"], s["cost"] if cost is None else cost)
    pred = engine.predict_frame(s["pr"], field) if sel.mv_per_ctu == 64 else s["pred"]
    return slot, pred


def device_residual(engine, planes, preds, bd, slot, per, had, first=0, count=-1, want=(True, True, True, True), pred_spare=0, resid_spare=0, skip_resid=()):
    """ONE hmme_residual_pairs_device launch over len(planes) pairs -> (resid int16 [n_pairs, h, w + spare], pu, cu uint32 [n_pairs, n_ctu, per],
    ctu uint32 [n_pairs, n_ctu, 2]) as numpy arrays preset with the sentinels; want: which of the four outputs are passed (else NULL);
    skip_resid: pairs whose entry of the residual list is NULL.  preds: [h, w] arrays; slot: [n_pairs, n_ctu, per] or None"""
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    n_pairs, p0 = len(planes), planes[0]
    w, h = p0.width, p0.height
    n = rm.n_ctus(w, h)
    dt, fill = (np.uint8, P_FILL) if bd == 8 else (np.uint16, P_FILL << 8 | P_FILL)
    d_preds = []
    for p in preds:
        img = np.full((h, w + pred_spare), fill, dt)
        img[:, :w] = p
        d_preds.append(torch.from_numpy(img if bd == 8 else img.view(np.int16)).to(dev))
    wr = (w + 3) // 4 * 4 + resid_spare
    d_res = [torch.full((h, wr), R_FILL, dtype=torch.int16, device=dev) for _ in range(n_pairs)]
    d_slot = torch.from_numpy(np.ascontiguousarray(slot, dtype=np.uint16).view(np.int16)).to(dev) if slot is not None else None
    d_pu = torch.full((n_pairs, n, per), U_FILL, dtype=torch.int32, device=dev)
    d_cu = torch.full((n_pairs, n, per), U_FILL, dtype=torch.int32, device=dev)
    d_ctu = torch.full((n_pairs, n, 2), U_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fp = api.FrameParams(1, 0, bd, first, count)
    resids = [None if i in skip_resid else d_res[i].data_ptr() for i in range(n_pairs)] if want[0] else None
    engine.residual_pairs_device(planes, [t.data_ptr() for t in d_preds], (w + pred_spare) * (1 if bd == 8 else 2), fp,
                                 d_slot.data_ptr() if d_slot is not None else None, per, had, resids, wr * 2,
                                 d_pu.data_ptr() if want[1] else None, d_cu.data_ptr() if want[2] else None, d_ctu.data_ptr() if want[3] else None, 0)
    torch.cuda.synchronize()
    for t, p in zip(d_preds, preds):                      # the inputs are read, never written
        back = t.cpu().numpy().view(dt)
        assert np.array_equal(back[:, :w], p) and (back[:, w:] == fill).all()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    return np.stack([t.cpu().numpy() for t in d_res]), u32(d_pu), u32(d_cu), u32(d_ctu)


def compare(engine, hmo, planes, curs, preds, bd, slot, per, had, first=0, count=-1, **kw):
    """one launch against the model, pair by pair: what was to be written equals the model, everything else -- samples outside the picture or the
    CTU range, spare columns, entries of other CTUs, outputs passed as NULL -- keeps its sentinel -> the model's (pu, cu, ctu) per pair"""
    want = kw.get("want", (True, True, True, True))
    skip = kw.get("skip_resid", ())
    res, pu, cu, ctu = device_residual(engine, planes, preds, bd, slot, per, had, first, count, **kw)
    w, h = planes[0].width, planes[0].height
    n = rm.n_ctus(w, h)
    cnt = n - first if count < 0 else count
    inside = rm.range_mask(w, h, first, cnt)
    outside_ctus = np.ones(n, bool)
    outside_ctus[first:first + cnt] = False
    models = []
    for i in range(len(planes)):
        md, mpu, mcu, mctu = rm.residual_picture(hmo, curs[i], preds[i], w, h, bd, None if slot is None else slot[i], per, had, first, cnt)
        if want[0] and i not in skip:
            assert np.array_equal(res[i][:, :w][inside], md[inside]), (i, per, had)
            assert (res[i][:, :w][~inside] == R_FILL).all() and (res[i][:, w:] == R_FILL).all()
        else:
            assert (res[i] == R_FILL).all()
        for k, (got, model) in enumerate(((pu[i], mpu), (cu[i], mcu), (ctu[i], mctu))):
            if want[k + 1]:
                assert np.array_equal(got[first:first + cnt], model), (i, per, had, k, np.argwhere(got[first:first + cnt] != model)[:4])
                assert (got[outside_ctus] == U_FILL).all()
            else:
                assert (got == U_FILL).all()
        models.append((mpu, mcu, mctu))
    return models


def keys_of(slot):
    """{(part size, depth)} of the slots a map holds"""
    from hmme import api
    return {api.slot_key(int(v))[:2] for v in np.unique(slot) if v != rm.NO_SLOT}


# ---- 1: the device form against the model, slot maps from real decisions; with and without a map; HAD and SAD ----------------------------------
@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", SIZES)
def test_real_decisions(engine, hmo, scenes, size, bd):
    from hmme import api
    w, h = size
    s = scenes(w, h, bd)
    for per in (64, 256):
        slot, pred = decide(engine, s, api.SelectParams(per))
        assert len(np.unique(slot)) > 1 and (pred != s["cur"]).any()                   # a real partition, a prediction that leaves a residual
        assert ((slot == rm.NO_SLOT).any()) == (h % 64 != 0 or w % 64 != 0)
        for had in (1, 0):
            (mpu, mcu, mctu), = compare(engine, hmo, [s["pc"]], [s["cur"]], [pred], bd, slot[None], per, had)
            assert mctu.all() and (mpu[slot == rm.NO_SLOT] == 0).all() and (mcu[slot == rm.NO_SLOT] == 0).all()
            compare(engine, hmo, [s["pc"]], [s["cur"]], [pred], bd, None, per, had)     # d_slot NULL: every block its own PU and CU


# ---- 2: every PartSize at every depth, forced: only 2Nx2N and the shape are allowed, and the tables' 2Nx2N costs at that depth are raised ----------
@pytest.mark.parametrize("per", [64, 256])
def test_every_part_size_at_every_depth(engine, hmo, scenes, per):
    from hmme import api
    w, h, bd = 136, 72, 10
    s = scenes(w, h, bd)
    seen = set()
    for depth in range(4):
        square = [api.slot_index(0, depth, 0, z) for z in range(256)]
        square = [v for v in square if v >= 0]
        assert len(square) == 4 ** depth
        for ps in (0, 1, 2, 4, 5, 6, 7):
            if ps and (depth == 3 and (ps > 2 or per == 64) or (depth == 2 and ps > 2 and per == 64)):
                continue                                                                 # not tabulated / not 8-aligned
            cost = None
            if ps:
                cost = s["cost"].copy()
                cost[:, square] = 1 << 24
            slot, pred = decide(engine, s, api.SelectParams(per, part_mask=1 | 1 << ps, min_depth=depth, max_depth=depth), cost)
            assert keys_of(slot) == {(ps, depth)}, (ps, depth, keys_of(slot))
            seen.add((ps, depth))
            compare(engine, hmo, [s["pc"]], [s["cur"]], [pred], bd, slot[None], per, 1)
            if ps in (0, 5):
                compare(engine, hmo, [s["pc"]], [s["cur"]], [pred], bd, slot[None], per, 0)
    assert len(seen) == (7 + 7 + 3 + 1 if per == 64 else 7 + 7 + 7 + 3)
    if per == 256:
        assert {(4, 2), (5, 2), (6, 2), (7, 2), (1, 3), (2, 3)} <= seen                  # AMP at 16x16 and the 8x4 / 4x8 PUs: 4x4 Hadamards


# ---- 3: CUs that straddle the picture edge ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_cus_straddle_the_edge_with_max_depth_1(engine, hmo, scenes, bd):
    from hmme import api
    w, h = 100, 70
    s = scenes(w, h, bd)
    for per in (64, 256):
        slot, pred = decide(engine, s, api.SelectParams(per, max_depth=1))
        straddle = 0
        g, nb = (8, 8) if per == 64 else (4, 16)
        for c in range(4):
            x0, y0 = (c % 2) * 64, (c // 2) * 64
            for v in np.unique(slot[c]):
                if v == rm.NO_SLOT:
                    continue
                (rx, ry, rw, rh), (qx, qy, qs) = rm.slot_geometry(int(v))
                assert qs >= 32
                straddle += (x0 + qx < w < x0 + qx + qs) or (y0 + qy < h < y0 + qy + qs)
        assert straddle >= 4 and (slot == rm.NO_SLOT).any()
        for had in (1, 0):
            (mpu, mcu, _), = compare(engine, hmo, [s["pc"]], [s["cur"]], [pred], bd, slot[None], per, had)
        # blocks of a straddling CU that lie outside the picture still carry the CU's totals
        b_out = nb - 1                                                                  # CTU 1, top row, last block: x >= 100
        assert slot[1, b_out] != rm.NO_SLOT and mcu[1, b_out] == mcu[1, (96 - 64) // g] != 0


# ---- 4: extremes at 12 bits ---------------------------------------------------------------------------------------------------------------------
def test_extremes_at_12_bits(engine, hmo):
    """0 against 4095 over whole CTUs: the sums reach what the header's bound speaks of and nothing wraps (the model computes in Python integers and
    in int64, and asserts that every CTU sum stays below 2^32)"""
    import frame_helpers as fh
    import range_content as rc
    from hmme import api, synth
    bd, maxv, m = 12, 4095, synth.MARGIN
    # (a) one CTU, one 64x64 PU: flat, and binary patterns whose Hadamard sums are far larger
    rng = np.random.default_rng(4)
    ys, xs = np.mgrid[0:64, 0:64]
    top = 0
    for k, pattern in enumerate((np.ones((64, 64), bool), ((xs >> 2) ^ (ys >> 2)) & 1 == 1, rng.integers(0, 2, size=(64, 64)) == 1)):
        cur = np.where(pattern, maxv, 0)
        pred = (maxv - cur).astype(np.uint16)
        pc = fh.mkplane(engine, synth.pad_plane(cur), 64, 64, bd)
        try:
            slot = np.full((1, 1, 64), 592, np.uint16)
            (mpu, mcu, mctu), = compare(engine, hmo, [pc], [cur], [pred], bd, slot, 64, 1)
            assert (mcu == 4096 * ((maxv * maxv) >> 8)).all() and mctu[0, 0] == mpu[0, 0]
            top = max(top, int(mpu[0, 0]) << 4)
            (mpu, _, _), = compare(engine, hmo, [pc], [cur], [pred], bd, slot, 64, 0)
            assert (mpu == (4096 * maxv) >> 4).all()
            for per in (64, 256):
                compare(engine, hmo, [pc], [cur], [pred], bd, None, per, 1)
        finally:
            pc.close()
    assert 64 * 65520 <= top <= 64 * ((64 * 64 * maxv + 2) >> 2)          # at least the flat picture's total, within the header's bound
    # (b) range_content's pictures: samples in {0, maxv}, two CTUs saturated against their reference; the reference is the prediction (MV 0)
    w, h = 136, 72
    cur, ref, _ = rc.extreme_pair(w, h, bd, (64, 0, 6, 32), seed=9)
    cur_img, pred = cur[m:m + h, m:m + w], ref[m:m + h, m:m + w].astype(np.uint16)
    lo_ctu, hi_ctu = rc.saturated_ctus(w, h)
    assert set(np.unique(pred)) == {0, maxv} and (np.abs(cur_img[64:, :64].astype(int) - pred[64:, :64]) == maxv).all()
    pc, pr = fh.mkplane(engine, cur, w, h, bd), fh.mkplane(engine, ref, w, h, bd)
    try:
        mv, _ = engine.search_frame(pc, pr, 8)
        qmv, cost = engine.refine_frame(pc, pr, 8, mv)
        for per in (64, 256):
            _, slot, _ = engine.select_frame(w, h, api.SelectParams(per, max_depth=2), qmv, cost)
            for had in (1, 0):
                (_, mcu, _), = compare(engine, hmo, [pc], [cur_img], [pred], bd, slot[None], per, had)
            assert mcu[lo_ctu].max() >= 16 * 8 * ((maxv * maxv) >> 8) and mcu[hi_ctu].max() > 0
    finally:
        pc.close(); pr.close()


# ---- 5: several pairs, CTU sub-ranges, strided images, NULL outputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_pairs_ranges_strides_and_null_outputs(engine, hmo, scenes, bd):
    from hmme import api
    w, h = 136, 72
    ss = [scenes(w, h, bd, seed) for seed in (0, 1, 2)]
    planes, curs = [s["pc"] for s in ss], [s["cur"] for s in ss]
    for per in (64, 256):
        dec = [decide(engine, s, api.SelectParams(per)) for s in ss]
        slot, preds = np.stack([d[0] for d in dec]), [d[1] for d in dec]
        assert not np.array_equal(preds[0], preds[1]) and not np.array_equal(preds[1], preds[2])     # a pair read in another's place would show
        whole = compare(engine, hmo, planes, curs, preds, bd, slot, per, 1)                         # three pairs, one launch
        for first, count in ((1, 4), (5, 1), (0, 2), (2, 0)):                                       # sub-ranges (sentinels outside: compare)
            part = compare(engine, hmo, planes, curs, preds, bd, slot, per, 1, first, count)
            for i in range(3):
                for a, b in zip(part[i], whole[i]):
                    assert np.array_equal(a, b[first:first + count])
        # strided images: an aligned spare, and a predicted pitch that is no multiple of 4 (served sample by sample)
        compare(engine, hmo, planes, curs, preds, bd, slot, per, 1, pred_spare=24, resid_spare=8)
        compare(engine, hmo, planes, curs, preds, bd, slot, per, 0, 1, 3, pred_spare=3 if bd == 8 else 1, resid_spare=4)
        compare(engine, hmo, planes, curs, preds, bd, None, per, 1, pred_spare=3 if bd == 8 else 1)
        # every output NULL in turn, and a NULL entry of the residual list: nothing of a NULL output is written, the others are complete
        for k in range(4):
            want = tuple(j != k for j in range(4))
            compare(engine, hmo, planes, curs, preds, bd, slot, per, 1, 1, 4, want=want)
        compare(engine, hmo, planes, curs, preds, bd, slot, per, 1, skip_resid=(1,))
        compare(engine, hmo, planes, curs, preds, bd, None, per, 0, want=(True, False, False, False))
    # sixteen pairs in one launch (the limit), the same plane sixteen times with sixteen different slot maps
    s = ss[0]
    maps = [decide(engine, s, api.SelectParams(64, min_depth=d % 4, max_depth=max(d % 4, (d // 4) % 4)))[0] for d in range(16)]
    compare(engine, hmo, [s["pc"]] * 16, [s["cur"]] * 16, [s["pred"]] * 16, bd, np.stack(maps), 64, 1, want=(False, True, True, True))


# ---- 6: the host-facing call ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 12])
def test_frame_form_equals_the_device_form(engine, hmo, scenes, bd):
    from hmme import api
    w, h = 100, 70
    s = scenes(w, h, bd)
    n = rm.n_ctus(w, h)
    for per in (64, 256):
        slot, pred = decide(engine, s, api.SelectParams(per))
        for had, use_map in ((1, True), (0, True), (1, False)):
            sm = slot if use_map else None
            res, pu, cu, ctu = device_residual(engine, [s["pc"]], [pred], bd, None if sm is None else sm[None], per, had)
            f_res, f_pu, f_cu, f_ctu = engine.residual_frame(s["pc"], pred, sm, per, bool(had))
            assert np.array_equal(f_res, res[0][:, :w]) and np.array_equal(f_pu, pu[0]) and np.array_equal(f_cu, cu[0]) and np.array_equal(f_ctu, ctu[0])
            assert f_res.any() and f_pu.any() and f_cu.any()
            # a sub-range into the caller's arrays: samples and entries outside keep their values
            first, cnt = 1, 2
            r0 = np.full((h, w), 0x1111, np.int16); p0 = np.full((n, per), 0x22222222, np.uint32); c0 = p0.copy(); t0 = np.full((n, 2), 0x33333333, np.uint32)
            engine.residual_frame(s["pc"], pred, sm, per, bool(had), first, cnt, resid=r0, pu=p0, cu=c0, ctu=t0)
            inside = rm.range_mask(w, h, first, cnt)
            assert np.array_equal(r0[inside], f_res[inside]) and (r0[~inside] == 0x1111).all()
            for got, full, fill in ((p0, f_pu, 0x22222222), (c0, f_cu, 0x22222222), (t0, f_ctu, 0x33333333)):
                assert np.array_equal(got[first:first + cnt], full[first:first + cnt]) and (got[:first] == fill).all() and (got[first + cnt:] == fill).all()
            r2, p2 = r0.copy(), p0.copy()
            engine.residual_frame(s["pc"], pred, sm, per, bool(had), 2, 0, resid=r2, pu=p2)      # an empty range: accepted, nothing changes
            assert np.array_equal(r2, r0) and np.array_equal(p2, p0)
    # strides beyond the width (the Python method always passes the width) and NULL outputs, through the C entry
    dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0xA5A5)
    slot, pred = decide(engine, s, api.SelectParams(64))
    f_res, f_pu, f_cu, f_ctu = engine.residual_frame(s["pc"], pred, slot, 64, True)
    wide = np.full((h, w + 7), fill, dt); wide[:, :w] = pred
    fp = api.FrameParams(1, 0, bd, 0, -1)
    r1 = np.full((h, w + 5), 0x1111, np.int16); p1 = np.full((n, 64), 7, np.uint32); c1 = p1.copy(); t1 = np.full((n, 2), 7, np.uint32)
    assert engine.L.hmme_residual_frame(engine.h, s["pc"].h, C.byref(fp), wide.ctypes.data, w + 7, slot.ctypes.data, 64, 1, r1.ctypes.data, w + 5,
                                        p1.ctypes.data, None, t1.ctypes.data) == 0
    assert np.array_equal(r1[:, :w], f_res) and (r1[:, w:] == 0x1111).all() and np.array_equal(p1, f_pu) and (c1 == 7).all() and np.array_equal(t1, f_ctu)
    assert engine.L.hmme_residual_frame(engine.h, s["pc"].h, C.byref(fp), wide.ctypes.data, w + 7, slot.ctypes.data, 64, 1, None, 0, None, c1.ctypes.data, None) == 0
    assert np.array_equal(c1, f_cu)


# ---- 7: a used context gives what a fresh one gives --------------------------------------------------------------------------------------------
def test_a_used_context_gives_what_a_fresh_one_gives(engine, scenes):
    """the module's context has run searches, refinements, selections and predictions (and grown its staging arena for them) before this call"""
    from hmme import api, synth
    w, h, bd = 136, 72, 10
    s = scenes(w, h, bd)
    slot, pred = decide(engine, s, api.SelectParams(256))
    engine.search_frame(s["pc"], s["pr"], 8)
    used = [engine.residual_frame(s["pc"], pred, sm, 256, had) for sm in (slot, None) for had in (True, False)]
    fresh_engine = api.Engine(0, 64)
    try:
        pc = fresh_engine.plane(w, h, bd)
        pc.upload_pel(synth.pad_plane(s["cur"]), (synth.MARGIN, synth.MARGIN))
        fresh = [fresh_engine.residual_frame(pc, pred, sm, 256, had) for sm in (slot, None) for had in (True, False)]
        pc.close()
    finally:
        fresh_engine.close()
    for a, b in zip(used, fresh):
        for x, y in zip(a, b):
            assert np.array_equal(x, y) and x.any()


# ---- 8: refusals: the code, nothing launched, the outputs keep their sentinel ---------------------------------------------------------------------
def test_refusals(engine, scenes):
    import torch
    from hmme import api
    L = api.load()
    dev = torch.device("cuda", 0)
    w, h, bd = 100, 70, 8
    s = scenes(w, h, bd)
    s10 = scenes(w, h, 10)
    s_other_size = scenes(64, 64, 8)
    n = rm.n_ctus(w, h)
    d_pred = torch.from_numpy(np.array(s["pred"])).to(dev)
    d_slot = torch.from_numpy(np.array(s["slot64"]).view(np.int16)).to(dev)
    d_res = torch.full((h, 104), R_FILL, dtype=torch.int16, device=dev)
    d_pu = torch.full((n, 64), U_FILL, dtype=torch.int32, device=dev); d_cu = d_pu.clone(); d_ctu = torch.full((n, 2), U_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    other = api.Engine(0, 64)
    foreign = other.plane(w, h, 8)
    vp = C.c_void_p

    def call(ctx=engine.h, planes=(s["pc"],), preds=(d_pred.data_ptr(),), pitch=w, n_pairs=1, fp=api.FrameParams(1, 0, 8, 0, -1), slot=d_slot.data_ptr(), per=64, had=1,
             resids=(d_res.data_ptr(),), rpitch=208, pu=d_pu.data_ptr(), cu=d_cu.data_ptr(), ctu=d_ctu.data_ptr()):
        pa = None if planes is None else (vp * 16)(*[None if p is None else p.h for p in planes])
        ia = None if preds is None else (vp * 16)(*preds)
        ra = None if resids is None else (vp * 16)(*resids)
        return L.hmme_residual_pairs_device(ctx, pa, ia, pitch, n_pairs, None if fp is None else C.byref(fp), slot, per, had, ra, rpitch, pu, cu, ctu, None)

    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        assert call() == 0                                               # the baseline every refusal below departs from in one argument
        torch.cuda.synchronize()
        assert (d_pu.cpu().numpy().view(np.uint32) != U_FILL).all()
        for t, v in ((d_res, R_FILL), (d_pu, U_FILL), (d_cu, U_FILL), (d_ctu, U_FILL)):
            t.fill_(v)
        torch.cuda.synchronize()
        refused = dict(
            null_context=dict(ctx=None), null_planes=dict(planes=None), null_plane=dict(planes=(None,)), null_images=dict(preds=None), null_image=dict(preds=(None,)),
            null_fp=dict(fp=None), no_output=dict(resids=None, pu=None, cu=None, ctu=None),
            zero_pairs=dict(n_pairs=0), seventeen_pairs=dict(n_pairs=17, planes=(s["pc"],) * 16, preds=(d_pred.data_ptr(),) * 16, resids=None),
            per_128=dict(per=128), per_1=dict(per=1), had_2=dict(had=2), had_minus_1=dict(had=-1),
            depth_mismatch=dict(fp=api.FrameParams(1, 0, 10, 0, -1)), plane_of_other_depth=dict(planes=(s10["pc"],)),
            foreign_plane=dict(planes=(foreign,)), sizes_differ=dict(n_pairs=2, planes=(s["pc"], s_other_size["pc"]), preds=(d_pred.data_ptr(),) * 2, resids=None),
            ctu_range=dict(fp=api.FrameParams(1, 0, 8, 3, 2)), pitch_short=dict(pitch=w - 1), resid_pitch_short=dict(rpitch=192), resid_pitch_odd=dict(rpitch=204),
            image_misaligned=dict(preds=(d_pred.data_ptr() + 2,)), slot_misaligned=dict(slot=d_slot.data_ptr() + 2), resid_misaligned=dict(resids=(d_res.data_ptr() + 4,)),
            pu_misaligned=dict(pu=d_pu.data_ptr() + 2), cu_misaligned=dict(cu=d_cu.data_ptr() + 1), ctu_misaligned=dict(ctu=d_ctu.data_ptr() + 2))
        for name, kw in refused.items():
            assert call(**kw) == ERR_ARG, name
            if name != "null_context":
                assert b"hmme_residual_pairs_device" in L.hmme_last_error(engine.h), name
        torch.cuda.synchronize()
        assert (d_res.cpu().numpy() == R_FILL).all()
        for t in (d_pu, d_cu, d_ctu):
            assert (t.cpu().numpy().view(np.uint32) == U_FILL).all()
        # the host-facing call refuses the same and launches nothing: the caller's arrays keep their values
        pred, slot = np.array(s["pred"]), np.array(s["slot64"])
        fp = api.FrameParams(1, 0, 8, 0, -1)
        r = np.full((h, w), 0x1111, np.int16); p = np.full((n, 64), 7, np.uint32)
        frame = lambda cur=s["pc"].h, fp=fp, pred=pred.ctypes.data, stride=w, per=64, had=1, res=r.ctypes.data, rstride=w, pu=p.ctypes.data: \
            L.hmme_residual_frame(engine.h, cur, C.byref(fp), pred, stride, slot.ctypes.data, per, had, res, rstride, pu, None, None)
        assert frame() == 0 and p.any() and (p != 7).any()
        r[:] = 0x1111; p[:] = 7
        for kw in (dict(cur=None), dict(pred=None), dict(stride=w - 1), dict(rstride=w - 1), dict(per=32), dict(had=3), dict(cur=foreign.h), dict(cur=s10["pc"].h),
                   dict(fp=api.FrameParams(1, 0, 8, 4, 1)), dict(res=None, pu=None)):
            assert frame(**kw) == ERR_ARG, kw
            assert b"hmme_residual_frame" in L.hmme_last_error(engine.h), kw
        assert (r == 0x1111).all() and (p == 7).all()
        assert L.hmme_residual_frame(None, s["pc"].h, C.byref(fp), pred.ctypes.data, w, None, 64, 1, r.ctypes.data, w, None, None, None) == ERR_ARG
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        foreign.close()
        other.close()
