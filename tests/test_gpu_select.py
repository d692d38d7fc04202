"""Partition decision and motion field from the 593-slot tables on the device (hmme_select_pairs_device, hmme_select_frame,
sequence.run_rank(select=...)) against tests/select_model.py, the rule of include/hmme.h restated one CU at a time in Python.  Every
comparison is bit-exact.  The kernel reads tables, not pictures: most cases feed synthetic tables (select_model.random_tables) and assert on
the MODEL's result that the input exercises what the case is about, so a degenerate input cannot pass silently."""
import numpy as np
import pytest

import select_model as sm

pytestmark = pytest.mark.gpu

LAMBDA = 57.9
ALL_SHAPES = {0, 1, 2, 4, 5, 6, 7}
F_FILL, S_FILL, C_FILL = 0x5A5A, 0x1234, 0x0BADBEEF   # sentinels the outputs are preset with


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(LAMBDA)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mv_cost(oracle_lib):
    L = oracle_lib.oracle()
    return lambda lq, x, y, px, py, scale: L.hmo_mv_cost(lq, x, y, px, py, scale)


@pytest.fixture(scope="module")
def tables40():
    """the recipe's 40 CTUs, drawn once and shared (never modified: the cases that edit tables copy them)"""
    mv, cost = sm.random_tables(40, seed=1)
    mv.setflags(write=False); cost.setflags(write=False)
    return mv, cost


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def device_select(engine, w, h, mv, cost, sel, pred=None, first=0, count=-1, want_slot=True, want_cost=True):
    """mv int16[n_pairs, count, 593, 2], cost uint32[n_pairs, count, 593] -> the three outputs of ONE hmme_select_pairs_device launch as numpy
    arrays over ALL CTUs of the picture, preset with the sentinels (None for an output that was passed as NULL)"""
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    n_pairs, n = mv.shape[0], n_ctus(w, h)
    cnt = n - first if count < 0 else count
    assert mv.shape == (n_pairs, cnt, 593, 2) and cost.shape == (n_pairs, cnt, 593)
    per = int(sel.mv_per_ctu)
    d_mv = torch.from_numpy(np.array(mv)).to(dev)                  # a copy: the shared tables are read-only
    d_cost = torch.from_numpy(np.array(cost).view(np.int32)).to(dev)
    d_pred = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.int16)).to(dev) if pred is not None else None
    d_field = torch.full((n_pairs, n, per, 2), F_FILL, dtype=torch.int16, device=dev)
    d_slot = torch.full((n_pairs, n, per), S_FILL, dtype=torch.int16, device=dev)
    d_cc = torch.full((n_pairs, n), C_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fp = api.FrameParams(1, 0, 8, first, cnt)
    engine.select_pairs_device(w, h, n_pairs, fp, sel, d_mv.data_ptr(), d_cost.data_ptr(), d_pred.data_ptr() if d_pred is not None else None,
                               d_field.data_ptr(), d_slot.data_ptr() if want_slot else None, d_cc.data_ptr() if want_cost else None, 0)
    torch.cuda.synchronize()
    return d_field.cpu().numpy(), d_slot.cpu().numpy().view(np.uint16), d_cc.cpu().numpy().view(np.uint32)


def model_select(engine, mv_cost, w, h, mv, cost, sel, pred=None, first=0):
    """the model over the same launch -> (field [n_pairs, count, per, 2], slot [n_pairs, count, per], cost [n_pairs, count], leaves)"""
    f, s, c, leaves = [], [], [], []
    for i in range(mv.shape[0]):
        fi, si, ci, lv = sm.select_picture(mv[i], cost[i], sel, w, h, first, None if pred is None else pred[i], engine.lambda_q16, mv_cost)
        f.append(fi); s.append(si); c.append(ci); leaves += lv
    return np.stack(f), np.stack(s), np.stack(c), leaves


def check_consistency(field, slot, mv, sel):
    """for every written block: out_slot's rectangle contains the block and the field is that slot's table MV, shifted as mv_unit says; blocks
    of CUs that do not exist carry 0xFFFF and (0,0).  field [count, per, 2], slot [count, per], mv [count, 593, 2]"""
    per = int(sel.mv_per_ctu)
    g, n = (8, 8) if per == 64 else (4, 16)
    for c in range(field.shape[0]):
        for b in range(per):
            s = int(slot[c, b])
            if s == sm.NO_SLOT:
                assert tuple(field[c, b]) == (0, 0)
                continue
            x, y, w, h = sm.rect(s)
            bx, by = (b % n) * g, (b // n) * g
            assert x <= bx and bx + g <= x + w and y <= by and by + g <= y + h, (c, b, s)
            want = (mv[c, s].astype(np.int32) << (2 if sel.mv_unit else 0)).astype(np.int16)
            assert tuple(field[c, b]) == tuple(want), (c, b, s)


def compare(engine, mv_cost, w, h, mv, cost, sel, pred=None, first=0, count=-1):
    """one launch against the model; also the sentinels outside the CTU range and the consistency of what was written -> the model's leaves"""
    field, slot, cc = device_select(engine, w, h, mv, cost, sel, pred, first, count)
    mf, ms, mc, leaves = model_select(engine, mv_cost, w, h, mv, cost, sel, pred, first)
    cnt = mv.shape[1]
    assert np.array_equal(field[:, first:first + cnt], mf)
    assert np.array_equal(slot[:, first:first + cnt], ms)
    assert np.array_equal(cc[:, first:first + cnt], mc)
    outside = np.ones(field.shape[1], bool)
    outside[first:first + cnt] = False
    assert (field[:, outside].view(np.uint16) == F_FILL).all() and (slot[:, outside] == S_FILL).all() and (cc[:, outside] == C_FILL).all()
    for i in range(mv.shape[0]):
        check_consistency(field[i, first:first + cnt], slot[i, first:first + cnt], mv[i], sel)
    return leaves, (mf, ms, mc)


def allowed_shapes(per):
    """(depth, PartSize) the 8-aligned restriction leaves with one MV per 8x8 block; everything the tables hold with four"""
    out = set()
    for d in range(4):
        for ps in ALL_SHAPES:
            if d == 3 and ps > 2:
                continue                                   # not tabulated
            if per == 64 and ((d == 3 and ps != 0) or (d == 2 and ps > 2)):
                continue
            out.add((d, ps))
    return out


# ---- 1: single CTU, 64x64 pictures: both field layouts, both MV units, with and without the MV cost ------------------------------------
@pytest.mark.parametrize("price", [0, 1])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("per", [64, 256])
def test_single_ctu_pictures(engine, mv_cost, tables40, per, unit, price):
    from hmme import api
    # the MV cost (about 300 per PU at lambda 57.9) outweighs the recipe's noise on small blocks -- with it the model never reached 8x8 CUs up to
    # 16 * w * h of noise: widened to 64 * w * h
    mv, cost = tables40 if not price else sm.random_tables(40, seed=2, noise=64)
    sel = api.SelectParams(per, mv_unit=unit, price_mv=price)
    rng = np.random.default_rng(100 + per + 2 * unit + price)
    leaves = []
    for k in range(0, 40, 16):                              # 64x64 pictures, up to 16 pairs per launch
        m, c = mv[k:k + 16, None], cost[k:k + 16, None]
        pred = rng.integers(-40, 41, size=(m.shape[0], 1, 2)).astype(np.int16)
        pred[pred == 0] = 7
        lv, _ = compare(engine, mv_cost, 64, 64, m, c, sel, pred if price else None)
        leaves += lv
    assert {d for d, _ in leaves} == {0, 1, 2, 3}
    if per == 256:
        assert {ps for _, ps in leaves} == ALL_SHAPES
    else:
        assert {ps for _, ps in leaves} == ALL_SHAPES and {(d, ps) for d, ps in leaves} <= allowed_shapes(64)
        assert {(2, 0), (2, 1), (2, 2), (3, 0)} <= set(leaves)


def test_the_mv_cost_changes_the_decision(engine, mv_cost, tables40):
    """price_mv is not a no-op on these tables: the model's fields with and without it differ (and the device followed both above)"""
    from hmme import api
    mv, cost = tables40
    pred = np.full((1, 40, 2), 9, np.int16)
    a = model_select(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(64, mv_unit=1, price_mv=0), pred)
    b = model_select(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(64, mv_unit=1, price_mv=1), pred)
    assert not np.array_equal(a[1], b[1]) and (b[2] > a[2]).all()
    lv, _ = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(64, mv_unit=1, price_mv=1), pred)
    assert lv == b[3]


# ---- 2: edge and off-grid pictures, three pairs per launch ------------------------------------------------------------------------------
EDGE_SIZES = [(136, 72), (100, 70), (200, 136)]    # 3x2, 2x2 and 4x3 CTUs: 3 * (6 + 4 + 12) = 66 CTUs over the three launches


@pytest.mark.parametrize("per", [64, 256])
@pytest.mark.parametrize("size", EDGE_SIZES)
def test_edge_and_off_grid_pictures(engine, mv_cost, size, per):
    from hmme import api
    w, h = size
    n = n_ctus(w, h)
    ctus_x = (w + 63) // 64
    mv, cost = sm.random_tables(3 * n, seed=10 + w)
    mv, cost = mv.reshape(3, n, 593, 2), cost.reshape(3, n, 593)
    sel = api.SelectParams(per)
    _, (mf, ms, mc) = compare(engine, mv_cost, w, h, mv, cost, sel)
    g, nb = (8, 8) if per == 64 else (4, 16)
    forced = absent = straddle = 0
    for c in range(n):
        x0, y0 = (c % ctus_x) * 64, (c // ctus_x) * 64
        if x0 + 64 <= w and y0 + 64 <= h:
            assert (ms[:, c] != sm.NO_SLOT).all()         # an interior CTU is covered completely
            continue
        for i in range(3):
            for b in range(per):
                bx, by = x0 + (b % nb) * g, y0 + (b // nb) * g
                s = int(ms[i, c, b])
                if s == sm.NO_SLOT:
                    absent += 1
                    assert tuple(mf[i, c, b]) == (0, 0)
                    # absent only where no bottom-level CU with its origin inside the picture covers the block
                    assert (bx // 8) * 8 >= w or (by // 8) * 8 >= h
                else:
                    rx, ry, rw, rh = sm.rect(s)
                    forced += 1                           # a CU of a partial CTU: the 64x64 CU was forced to split
                    assert max(rw, rh) < 64
                    if x0 + rx + rw > w or y0 + ry + rh > h:
                        straddle += 1                     # only bottom-level CUs may reach beyond the picture
                        assert max(rw, rh) <= 8
    assert forced > 0 and absent > 0                       # forced splits, absent CUs (0xFFFF slots with zero MVs) all occur
    if w % 8 or h % 8:
        assert straddle > 0                                # 100x70: bottom-level CUs straddle the edge
    else:
        assert straddle == 0


# ---- 3: ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [64, 256])
@pytest.mark.parametrize("kind", ["zero", "area"])
def test_ties_go_to_the_parent_and_the_lower_enum(engine, mv_cost, kind, per):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    rng = np.random.default_rng(3)
    mv = rng.integers(-200, 201, size=(1, n, 593, 2)).astype(np.int16)
    area = np.array([sm.rect(s)[2] * sm.rect(s)[3] for s in range(593)], np.uint32)
    cost = np.zeros((1, n, 593), np.uint32) if kind == "zero" else np.broadcast_to(area, (1, n, 593)).copy()
    _, (mf, ms, mc) = compare(engine, mv_cost, w, h, mv, cost, api.SelectParams(per))
    for c in (0, 1):                                        # the interior CTUs: one 64x64 2Nx2N leaf
        assert (ms[0, c] == 592).all() and (mf[0, c] == mv[0, c, 592]).all()
        assert mc[0, c] == (0 if kind == "zero" else 4096)
    assert (ms[0, 2] != 592).all() and (ms[0, 3:] != 592).all()   # the partial ones had to split


# ---- 4: restrictions and penalties ------------------------------------------------------------------------------------------------------
def test_part_mask_restrictions(engine, mv_cost, tables40):
    from hmme import api
    mv, cost = tables40
    for per in (64, 256):
        lv, _ = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(per, part_mask=0x01))
        assert {ps for _, ps in lv} == {0} and {d for d, _ in lv} == {0, 1, 2, 3}
        lv, _ = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(per, part_mask=0x07))
        assert {ps for _, ps in lv} == {0, 1, 2} and {d for d, _ in lv} == {0, 1, 2, 3}


def test_depth_restrictions(engine, mv_cost, tables40):
    from hmme import api
    mv, cost = tables40
    for per in (64, 256):
        lv, _ = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(per, min_depth=2, max_depth=2))
        assert {d for d, _ in lv} == {2} and len(lv) == 40 * 16
        assert {ps for _, ps in lv} == ({0, 1, 2} if per == 64 else ALL_SHAPES)
        lv, _ = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(per, min_depth=1, max_depth=2))
        assert {d for d, _ in lv} == {1, 2}
        lv, _ = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(per, min_depth=0, max_depth=0))
        assert {d for d, _ in lv} == {0} and len(lv) == 40
    # an edge picture whose deepest level is 16x16: CUs exist by their origin, whole 16x16 rectangles
    mv2, cost2 = sm.random_tables(3 * 4, seed=77)
    lv, (_, ms, _) = compare(engine, mv_cost, 100, 70, mv2.reshape(3, 4, 593, 2), cost2.reshape(3, 4, 593), api.SelectParams(64, min_depth=1, max_depth=2))
    assert (ms == sm.NO_SLOT).any() and {d for d, _ in lv} == {1, 2}


def test_penalties_of_2_to_the_20(engine, mv_cost, tables40):
    from hmme import api
    mv, cost = tables40
    plain = model_select(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(256))
    for cu, pu in ((1 << 20, 0), (0, 1 << 20), (1 << 20, 1 << 20)):
        lv, (_, ms, mc) = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(256, cu_cost=cu, pu_cost=pu))
        if cu:                                              # a CU penalty beyond any table cost: one CU per CTU; of the shapes the cheapest counts again
            assert {d for d, _ in lv} == {0} and len(lv) == 40
        if pu:
            assert {ps for _, ps in lv} == {0}             # a second PU never pays
        assert (mc > plain[2]).all() and mc.min() >= max(cu, pu)
    # forced to the bottom with both penalties: 64 CUs and 64 PUs per CTU, sums beyond 2^26 carried exactly
    lv, (_, _, mc) = compare(engine, mv_cost, 512, 320, mv[None], cost[None], api.SelectParams(64, min_depth=3, max_depth=3, cu_cost=1 << 20, pu_cost=1 << 20))
    assert (mc >= 128 << 20).all() and len(lv) == 40 * 64


def test_cost_saturates_at_uint32_max(engine, mv_cost, tables40):
    from hmme import api
    mv, cost = tables40[0][:6].copy(), tables40[1][:6].copy()
    cost[1] = 0xFFFFFFFF                                     # a whole CTU
    cost[4] = 0xFFFFFFFF
    for per in (64, 256):
        # without penalties the 64x64 2Nx2N leaf costs exactly UINT32_MAX, everything else at least twice that
        _, (_, ms, mc) = compare(engine, mv_cost, 192, 128, mv[None], cost[None], api.SelectParams(per))
        assert mc[0, 1] == 0xFFFFFFFF and mc[0, 4] == 0xFFFFFFFF and (ms[0, 1] == 592).all() and (mc[0, [0, 2, 3, 5]] < 1 << 20).all()
        # with penalties the sum passes 2^32: carried in 64 bits (the leaf stays the 64x64 CU), saturated on the way out
        _, (_, ms, mc) = compare(engine, mv_cost, 192, 128, mv[None], cost[None], api.SelectParams(per, cu_cost=5, pu_cost=3))
        assert mc[0, 1] == 0xFFFFFFFF and (ms[0, 1] == 592).all()
        # forced below the top: four CUs of UINT32_MAX each
        _, (_, ms, mc) = compare(engine, mv_cost, 192, 128, mv[None], cost[None], api.SelectParams(per, min_depth=1, max_depth=3))
        assert mc[0, 4] == 0xFFFFFFFF and set(ms[0, 4].tolist()) == {584, 585, 586, 587}
    # with the MV cost on top of UINT32_MAX entries
    pred = np.full((1, 6, 2), -13, np.int16)
    _, (_, _, mc) = compare(engine, mv_cost, 192, 128, mv[None], cost[None], api.SelectParams(64, mv_unit=1, price_mv=1), pred)
    assert mc[0, 1] == 0xFFFFFFFF


# ---- 5: CTU sub-range, NULL outputs, the host-facing call ----------------------------------------------------------------------------------
def test_ctu_sub_range_and_null_outputs(engine, mv_cost, tables40):
    from hmme import api
    mv, cost = tables40
    first, cnt = 7, 9
    m = np.stack([mv[first:first + cnt], mv[20:20 + cnt]])
    c = np.stack([cost[first:first + cnt], cost[20:20 + cnt]])
    for per in (64, 256):
        sel = api.SelectParams(per)
        _, (mf, ms, mc) = compare(engine, mv_cost, 512, 320, m, c, sel, None, first, cnt)    # sentinels outside the range: checked there
        field, slot, cc = device_select(engine, 512, 320, m, c, sel, None, first, cnt, want_slot=False, want_cost=False)
        assert np.array_equal(field[:, first:first + cnt], mf)
        assert (slot == S_FILL).all() and (cc == C_FILL).all()                               # NULL outputs: nothing written anywhere
        field, slot, cc = device_select(engine, 512, 320, m, c, sel, None, first, cnt, want_slot=True, want_cost=False)
        assert np.array_equal(slot[:, first:first + cnt], ms) and (cc == C_FILL).all()
    # the host-facing call with NULL for out_slot, out_cost and both (the Python method always passes every array), on a sub-range of 3 x 2 CTUs:
    # the field is the full call's, an array that was not passed is not written
    import ctypes as C
    w, h, n, first, cnt = 136, 72, 6, 1, 4
    fp = api.FrameParams(1, 0, 8, first, cnt)
    t_mv, t_cost = np.ascontiguousarray(mv[first:first + cnt]), np.ascontiguousarray(cost[first:first + cnt])
    for per in (64, 256):
        sel = api.SelectParams(per)
        f0 = np.full((n, per, 2), 0x1111, np.int16); s0 = np.full((n, per), 0x2222, np.uint16); c0 = np.full(n, 0x33333333, np.uint32)
        engine.select_frame(w, h, sel, t_mv, t_cost, None, ctu_first=first, ctu_count=cnt, field=f0, slot=s0, ctu_cost=c0)
        mf, ms, mc, _ = sm.select_picture(t_mv, t_cost, sel, w, h, first, None, engine.lambda_q16, mv_cost)
        assert np.array_equal(f0[first:first + cnt], mf) and np.array_equal(s0[first:first + cnt], ms) and np.array_equal(c0[first:first + cnt], mc)
        for want_slot, want_cost in ((False, True), (True, False), (False, False)):
            f1 = np.full((n, per, 2), 0x1111, np.int16); s1 = np.full((n, per), 0x2222, np.uint16); c1 = np.full(n, 0x33333333, np.uint32)
            assert engine.L.hmme_select_frame(engine.h, w, h, C.byref(fp), C.byref(sel), t_mv.ctypes.data, t_cost.ctypes.data, None, f1.ctypes.data,
                                              s1.ctypes.data if want_slot else None, c1.ctypes.data if want_cost else None) == 0
            assert np.array_equal(f1, f0)
            assert np.array_equal(s1, s0) if want_slot else (s1 == 0x2222).all()
            assert np.array_equal(c1, c0) if want_cost else (c1 == 0x33333333).all()


def test_select_frame_host_call(engine, mv_cost, tables40):
    from hmme import api
    mv, cost = tables40
    rng = np.random.default_rng(8)
    pred = rng.integers(-30, 31, size=(40, 2)).astype(np.int16)
    for per, unit, price in ((64, 0, 0), (256, 1, 1)):
        sel = api.SelectParams(per, mv_unit=unit, price_mv=price)
        field, slot, cc = engine.select_frame(512, 320, sel, mv, cost, pred if price else None)
        mf, ms, mc, _ = sm.select_picture(mv, cost, sel, 512, 320, 0, pred if price else None, engine.lambda_q16, mv_cost)
        assert np.array_equal(field, mf) and np.array_equal(slot, ms) and np.array_equal(cc, mc)
        # a sub-range into the caller's arrays: entries outside keep their values
        first, cnt = 33, 7
        f0 = np.full((40, per, 2), 0x1111, np.int16); s0 = np.full((40, per), 0x2222, np.uint16); c0 = np.full(40, 0x33333333, np.uint32)
        engine.select_frame(512, 320, sel, mv[first:], cost[first:], pred if price else None, ctu_first=first, ctu_count=cnt, field=f0, slot=s0, ctu_cost=c0)
        assert np.array_equal(f0[first:], mf[first:]) and np.array_equal(s0[first:], ms[first:]) and np.array_equal(c0[first:], mc[first:])
        assert (f0[:first] == 0x1111).all() and (s0[:first] == 0x2222).all() and (c0[:first] == 0x33333333).all()


def test_bad_arguments_are_refused(engine):
    import ctypes as C
    from hmme import api
    L = api.load()
    fp = api.FrameParams(1, 0, 8, 0, -1)
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        good = api.SelectParams(64)
        one = C.c_void_p(256)     # never dereferenced: every call below is refused before anything is launched
        assert L.hmme_select_pairs_device(engine.h, 64, 64, 1, C.byref(fp), C.byref(api.SelectParams(128)), one, one, None, one, None, None, None) == -1
        assert L.hmme_select_pairs_device(engine.h, 64, 64, 17, C.byref(fp), C.byref(good), one, one, None, one, None, None, None) == -1
        assert L.hmme_select_pairs_device(engine.h, 0, 64, 1, C.byref(fp), C.byref(good), one, one, None, one, None, None, None) == -1
        assert L.hmme_select_pairs_device(engine.h, 64, 64, 1, C.byref(fp), C.byref(good), None, one, None, one, None, None, None) == -1
        assert L.hmme_select_pairs_device(engine.h, 64, 64, 1, C.byref(api.FrameParams(1, 0, 8, 1, 1)), C.byref(good), one, one, None, one, None, None, None) == -1
    finally:
        L.hmme_set_error_printing(engine.h, prev)


# ---- 6: end to end: search + refinement on picture pairs, then the decision, then the calls that take the field ----------------------------
def test_end_to_end_on_two_picture_pairs(engine, mv_cost):
    import torch
    from hmme import api, synth
    w, h, sr, m = 128, 128, 8, synth.MARGIN
    dev = torch.device("cuda", 0)
    pics = [synth.make_pair(w, h, seed=40 + i, max_mv=5, region=32) for i in range(2)]
    curs, refs = [], []
    for cur, ref, _ in pics:
        for lst, a in ((curs, cur), (refs, ref)):
            p = engine.plane(w, h)
            p.upload_pel(a, (m, m))
            lst.append(p)
    try:
        n = n_ctus(w, h)
        fp = api.FrameParams(sr, 1, 8, 0, n)
        d_mv = torch.zeros((2, n, 593, 2), dtype=torch.int16, device=dev); d_sad = torch.zeros((2, n, 593), dtype=torch.int32, device=dev)
        d_q = torch.zeros_like(d_mv); d_c = torch.zeros_like(d_sad)
        sel = api.SelectParams(64)
        d_field = torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev)
        d_slot = torch.zeros((2, n, 64), dtype=torch.int16, device=dev); d_cc = torch.zeros((2, n), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        engine.search_pairs_device(curs, refs, fp, None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_pairs_device(curs, refs, fp, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
        engine.select_pairs_device(w, h, 2, fp, sel, d_q.data_ptr(), d_c.data_ptr(), None, d_field.data_ptr(), d_slot.data_ptr(), d_cc.data_ptr(), 0)
        torch.cuda.synchronize()
        qmv, cost = d_q.cpu().numpy(), d_c.cpu().numpy().view(np.uint32)
        field, slot, cc = d_field.cpu().numpy(), d_slot.cpu().numpy().view(np.uint16), d_cc.cpu().numpy().view(np.uint32)
        mf, ms, mc, leaves = model_select(engine, mv_cost, w, h, qmv, cost, sel)
        assert np.array_equal(field, mf) and np.array_equal(slot, ms) and np.array_equal(cc, mc)
        assert len(leaves) > 8 and (mf != 0).any()            # real content: more than one CU per CTU, moving blocks
        for i in range(2):
            check_consistency(field[i], slot[i], qmv[i], sel)
            # the calls that take a motion field, fed the device's and the model's: pair i's field describes refs[i], the other list of pair 1 - i
            j = 1 - i
            pa, pb = engine.predict_frame(refs[i], field[i]), engine.predict_frame(refs[i], mf[i])
            assert np.array_equal(pa, pb) and pa.any()
            ba = engine.search_frame_bi(curs[j], refs[j], refs[i], 4, field[i])
            bb = engine.search_frame_bi(curs[j], refs[j], refs[i], 4, mf[i])
            assert np.array_equal(ba[0], bb[0]) and np.array_equal(ba[1], bb[1]) and ba[1].any()
    finally:
        for p in curs + refs:
            p.close()


# ---- 7: the sequence pipeline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [True, False])
def test_run_rank_select(engine, refine):
    import torch
    from hmme import api, sequence, synth
    w, h, sr = 136, 72, 8
    pairs = [(1, 0), (2, 1), (3, 2)]
    source = synth.Sequence(w, h, 4, seed=5)
    sel = api.SelectParams(64, mv_unit=0 if refine else 1, price_mv=0 if refine else 1, cu_cost=40, pu_cost=12)
    res = sequence.run_rank(engine, source, pairs, w, h, 8, sr, pairs_per_launch=2, refine=refine, download=True, select=sel,
                            device=torch.device("cuda", 0))
    tabs = ("qmv", "cost") if refine else ("mv", "sad")
    n = n_ctus(w, h)
    assert res["field"].shape == (3, n, 64, 2) and res["slot"].shape == (3, n, 64) and res["ctu_cost"].shape == (3, n)
    assert "host_mv" not in res and "host_sad" not in res and "host_qmv" not in res   # the tables stay on the device
    assert "select_s" in res["stages"]
    for i in range(3):
        mv = res[tabs[0]][i].cpu().numpy()
        cost = res[tabs[1]][i].cpu().numpy().view(np.uint32)
        field, slot, cc = engine.select_frame(w, h, sel, mv, cost)
        assert cost.any() and (slot != sm.NO_SLOT).any() and (slot == sm.NO_SLOT).any()
        for key, want in (("field", field), ("slot", slot.view(np.int16)), ("ctu_cost", cc.view(np.int32))):
            assert np.array_equal(res[key][i].cpu().numpy(), want), key
            assert np.array_equal(res["host_" + key][i].numpy(), want), key
