"""The reference picture per PU on the device (hmme_select_refs_device / _frame) and the prediction from it (hmme_predict_refs_device /
_frame) against tests/select_refs_model.py -- the rule of include/hmme.h restated in Python integers -- and, for the prediction, against
Engine.predict_frame block by block (that call is pinned to the oracle elsewhere).  Every comparison is bit-exact.  The decision reads
tables, not pictures: most cases feed the recipes of select_refs_model, of which tests/test_select_refs_cpu.py shows on the model alone
that every reference wins blocks; the other cases assert on the MODEL's result that the input exercises what the case is about."""
import ctypes as C

import numpy as np
import pytest

import select_model as sm
import select_refs_model as srm

pytestmark = pytest.mark.gpu

F_FILL, R_FILL, S_FILL, C_FILL = 0x5A5A, 0xA7, 0x1234, 0x0BADBEEF   # sentinels the outputs are preset with
n_ctus = srm.n_ctus


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda_q16(srm.LAMBDA_Q16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mv_cost(oracle_lib):
    L = oracle_lib.oracle()
    return lambda lq, x, y, px, py, scale: L.hmo_mv_cost(lq, x, y, px, py, scale)


class Outputs:
    """the four outputs of one launch on the device, preset with the sentinels"""

    def __init__(self, n_pics, n, per):
        import torch
        dev = torch.device("cuda", 0)
        self.field = torch.full((n_pics, n, per, 2), F_FILL, dtype=torch.int16, device=dev)
        self.ref = torch.full((n_pics, n, per), R_FILL, dtype=torch.uint8, device=dev)
        self.slot = torch.full((n_pics, n, per), S_FILL, dtype=torch.int16, device=dev)
        self.cc = torch.full((n_pics, n), C_FILL, dtype=torch.int32, device=dev)

    def host(self):
        return self.field.cpu().numpy(), self.ref.cpu().numpy(), self.slot.cpu().numpy().view(np.uint16), self.cc.cpu().numpy().view(np.uint32)

    def untouched(self):
        f, r, s, c = self.host()
        return (f.view(np.uint16) == F_FILL).all() and (r == R_FILL).all() and (s == S_FILL).all() and (c == C_FILL).all()


def to_device(mv, cost, pred):
    import torch
    dev = torch.device("cuda", 0)
    d_mv = torch.from_numpy(np.array(mv)).to(dev)                  # copies: the shared tables are read-only
    d_cost = torch.from_numpy(np.array(cost).view(np.int32)).to(dev)
    d_pred = torch.from_numpy(np.array(pred, dtype=np.int16)).to(dev) if pred is not None else None
    return d_mv, d_cost, d_pred


def device_select_refs(engine, w, h, mv, cost, sel, ref_cost=None, pred=None, first=0, count=-1, want_slot=True, want_cost=True):
    """mv int16[n_pics, n_refs, count, 593, 2], cost uint32[n_pics, n_refs, count, 593], pred int16[n_pics, n_refs, n_ctu, 2] or None -> the four
    outputs of ONE hmme_select_refs_device launch as numpy arrays over ALL CTUs of the picture (sentinels where nothing was written)"""
    import torch
    from hmme import api
    n_pics, n_refs, n = mv.shape[0], mv.shape[1], n_ctus(w, h)
    cnt = n - first if count < 0 else count
    assert mv.shape == (n_pics, n_refs, cnt, 593, 2) and cost.shape == (n_pics, n_refs, cnt, 593)
    assert pred is None or pred.shape == (n_pics, n_refs, n, 2)
    d_mv, d_cost, d_pred = to_device(mv, cost, pred)
    out = Outputs(n_pics, n, int(sel.mv_per_ctu))
    torch.cuda.synchronize()
    fp = api.FrameParams(1, 0, 8, first, cnt)
    engine.select_refs_device(w, h, n_pics, n_refs, fp, sel, ref_cost, d_mv.data_ptr(), d_cost.data_ptr(), d_pred.data_ptr() if d_pred is not None else None,
                              out.field.data_ptr(), out.ref.data_ptr(), out.slot.data_ptr() if want_slot else None, out.cc.data_ptr() if want_cost else None, 0)
    torch.cuda.synchronize()
    return out.host()


def model_select_refs(mv_cost, w, h, mv, cost, sel, ref_cost=None, pred=None, first=0):
    """the model over the same launch -> (field [n_pics, count, per, 2], ref, slot [n_pics, count, per], cost [n_pics, count])"""
    res = [srm.select_refs_picture(mv[i], cost[i], sel, w, h, ref_cost, first, None if pred is None else pred[i], srm.LAMBDA_Q16, mv_cost)
           for i in range(mv.shape[0])]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


def compare(engine, mv_cost, w, h, mv, cost, sel, ref_cost=None, pred=None, first=0, count=-1):
    """one launch against the model, the sentinels outside the CTU range included -> the model's (field, ref, slot, cost)"""
    got = device_select_refs(engine, w, h, mv, cost, sel, ref_cost, pred, first, count)
    want = model_select_refs(mv_cost, w, h, mv, cost, sel, ref_cost, pred, first)
    cnt = mv.shape[2]
    for g, m, name in zip(got, want, ("field", "ref", "slot", "cost")):
        assert np.array_equal(g[:, first:first + cnt], m), name
    outside = np.ones(got[0].shape[1], bool)
    outside[first:first + cnt] = False
    assert (got[0][:, outside].view(np.uint16) == F_FILL).all() and (got[1][:, outside] == R_FILL).all()
    assert (got[2][:, outside] == S_FILL).all() and (got[3][:, outside] == C_FILL).all()
    mf, mr, ms, _ = want
    assert ((mr == srm.NO_REF) == (ms == sm.NO_SLOT)).all() and (mr[ms != sm.NO_SLOT] < mv.shape[1]).all()
    # the field is the table MV of the winning reference at the covering slot
    for i, c, b in zip(*np.nonzero(ms != sm.NO_SLOT)):
        v = mv[i, mr[i, c, b], c, ms[i, c, b]].astype(np.int32) << (2 if sel.mv_unit else 0)
        assert tuple(mf[i, c, b]) == tuple(v.astype(np.int16))
    return want


# ---- 1: every number of references, both field layouts, both MV units, with and without the MV cost --------------------------------------
@pytest.mark.parametrize("price", [0, 1])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("per", [64, 256])
@pytest.mark.parametrize("n_refs", [1, 2, 4, 16])
def test_references_layouts_units_and_pricing(engine, mv_cost, n_refs, per, unit, price):
    from hmme import api
    w, h, mv, cost, pred, ref_cost, min_depth = srm.case(n_refs, price)
    sel = api.SelectParams(per, mv_unit=unit, price_mv=price, min_depth=min_depth)
    _, mr, ms, _ = compare(engine, mv_cost, w, h, mv[None], cost[None], sel, ref_cost, pred[None])
    assert set(mr[ms != sm.NO_SLOT].tolist()) == set(range(n_refs))     # every reference wins blocks (shown on the CPU as well)


# ---- 2: one reference is the partition decision -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("per,unit,price", [(64, 0, 0), (256, 1, 1)])
def test_one_reference_at_no_price_is_select_frame(engine, per, unit, price):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    mv, cost = sm.random_tables(n, seed=21, noise=64 if price else 2)
    pred = srm.ref_predictors(1, n, seed=22)
    sel = api.SelectParams(per, mv_unit=unit, price_mv=price, cu_cost=40, pu_cost=12)
    f0, s0, c0 = engine.select_frame(w, h, sel, mv, cost, pred[0])
    for ref_cost in (None, [0]):
        f, r, s, c = engine.select_refs_frame(w, h, sel, mv[None], cost[None], ref_cost, pred)
        assert np.array_equal(f, f0) and np.array_equal(s, s0) and np.array_equal(c, c0)
        assert (r[s0 != sm.NO_SLOT] == 0).all() and (r[s0 == sm.NO_SLOT] == srm.NO_REF).all() and (s0 == sm.NO_SLOT).any()


# ---- 3: ties go to the lowest index -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [64, 256])
def test_ties_go_to_the_lowest_reference_index(engine, mv_cost, per):
    from hmme import api
    w, h = 100, 70
    n = n_ctus(w, h)
    mv1, cost1 = sm.random_tables(n, seed=31)
    mv, cost = np.stack([mv1] * 4)[None], np.stack([cost1] * 4)[None]
    mv[0, 1:, :, :, 0] += np.arange(1, 4, dtype=np.int16)[:, None, None]   # same costs, MVs that tell the references apart
    sel = api.SelectParams(per)
    mf, mr, ms, _ = compare(engine, mv_cost, w, h, mv, cost, sel, [0, 0, 0, 0])
    assert (mr[ms != sm.NO_SLOT] == 0).all() and (ms != sm.NO_SLOT).any()
    mf1, mr1, ms1, _ = compare(engine, mv_cost, w, h, mv, cost, sel, [1, 0, 0, 0])
    assert (mr1[ms1 != sm.NO_SLOT] == 1).all() and np.array_equal(ms1, ms) and not np.array_equal(mf1, mf)


# ---- 4: the price of a reference index changes the outcome -------------------------------------------------------------------------------
def test_ref_cost_changes_the_outcome(engine, mv_cost):
    from hmme import api
    w, h, mv, cost, pred, _, _ = srm.case(4, 0)
    sel = api.SelectParams(256)
    _, mr, ms, mc = compare(engine, mv_cost, w, h, mv[None], cost[None], sel, [0, 0, 0, 0])
    assert (mr[ms != sm.NO_SLOT] == 2).any()                                # reference 2 wins blocks for free ...
    _, mr2, ms2, mc2 = compare(engine, mv_cost, w, h, mv[None], cost[None], sel, [0, 0, 1 << 20, 0])
    assert not (mr2 == 2).any() and (mc2 >= mc).all() and (mc2 > mc).any()   # ... and none at 2^20, which no table cost of the recipe reaches


# ---- 5: every reference is priced against its own predictor ------------------------------------------------------------------------------
def test_the_mv_cost_uses_each_references_own_predictor(engine, mv_cost):
    from hmme import api
    w, h, mv, cost, pred, _, _ = srm.case(4, 1)
    cost = np.stack([cost[0]] * 4)                                          # the same costs in every reference: the MV cost alone decides
    sel = api.SelectParams(64, mv_unit=1, price_mv=1)
    own = compare(engine, mv_cost, w, h, mv[None], cost[None], sel, None, pred[None])
    shared = np.broadcast_to(pred[0], pred.shape)                           # every reference priced against reference 0's predictor
    other = model_select_refs(mv_cost, w, h, mv[None], cost[None], sel, None, shared[None])
    assert not np.array_equal(own[1], other[1])                             # the model chooses differently: the device followed `own`
    assert set(own[1][own[2] != sm.NO_SLOT].tolist()) == {0, 1, 2, 3}


# ---- 6: several pictures in one launch, CTU sub-ranges, NULL outputs --------------------------------------------------------------------
def test_two_pictures_of_three_references_in_one_launch(engine, mv_cost):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    mv, cost = srm.random_ref_tables(6, n, seed=61)
    mv, cost = mv.reshape(2, 3, n, 593, 2), cost.reshape(2, 3, n, 593)
    pred = srm.ref_predictors(6, n, seed=62).reshape(2, 3, n, 2)
    for per, unit, price in ((64, 0, 0), (256, 1, 1)):
        _, mr, ms, _ = compare(engine, mv_cost, w, h, mv, cost, api.SelectParams(per, mv_unit=unit, price_mv=price), [3, 0, 5], pred)
        for i in range(2):
            assert set(mr[i][ms[i] != sm.NO_SLOT].tolist()) == {0, 1, 2}
        assert not np.array_equal(mr[0], mr[1])


def test_ctu_sub_range_and_null_outputs(engine, mv_cost):
    from hmme import api
    w, h, first, cnt = 136, 72, 1, 4
    mv, cost = srm.random_ref_tables(4, cnt, seed=71)
    mv, cost = mv.reshape(2, 2, cnt, 593, 2), cost.reshape(2, 2, cnt, 593)
    for per in (64, 256):
        sel = api.SelectParams(per)
        mf, mr, ms, mc = compare(engine, mv_cost, w, h, mv, cost, sel, [0, 2], None, first, cnt)     # sentinels outside the range: checked there
        f, r, s, c = device_select_refs(engine, w, h, mv, cost, sel, [0, 2], None, first, cnt, want_slot=False, want_cost=False)
        assert np.array_equal(f[:, first:first + cnt], mf) and np.array_equal(r[:, first:first + cnt], mr)
        assert (s == S_FILL).all() and (c == C_FILL).all()                                            # NULL outputs: nothing written anywhere
        f, r, s, c = device_select_refs(engine, w, h, mv, cost, sel, [0, 2], None, first, cnt, want_slot=True, want_cost=False)
        assert np.array_equal(s[:, first:first + cnt], ms) and (c == C_FILL).all()
    # the host-facing call into the caller's arrays: entries outside the range keep their values
    sel = api.SelectParams(64)
    n = n_ctus(w, h)
    f0 = np.full((n, 64, 2), 0x1111, np.int16); r0 = np.full((n, 64), 0x22, np.uint8); s0 = np.full((n, 64), 0x3333, np.uint16); c0 = np.full(n, 0x44444444, np.uint32)
    engine.select_refs_frame(w, h, sel, mv[1], cost[1], [0, 2], None, ctu_first=first, ctu_count=cnt, field=f0, ref=r0, slot=s0, ctu_cost=c0)
    mf, mr, ms, mc = model_select_refs(mv_cost, w, h, mv[1:], cost[1:], sel, [0, 2], None, first)
    rng_ = slice(first, first + cnt)
    assert np.array_equal(f0[rng_], mf[0]) and np.array_equal(r0[rng_], mr[0]) and np.array_equal(s0[rng_], ms[0]) and np.array_equal(c0[rng_], mc[0])
    out = np.ones(n, bool); out[rng_] = False
    assert (f0[out] == 0x1111).all() and (r0[out] == 0x22).all() and (s0[out] == 0x3333).all() and (c0[out] == 0x44444444).all()
    # ... with NULL for out_slot, out_cost and both (the Python method always passes every array), in both layouts: the field and the references
    # are the full call's, an array that was not passed is not written
    fp, rcost = api.FrameParams(1, 0, 8, first, cnt), (C.c_uint32 * 2)(0, 2)
    t_mv, t_cost = np.ascontiguousarray(mv[1], dtype=np.int16), np.ascontiguousarray(cost[1], dtype=np.uint32)
    for per in (64, 256):
        sel = api.SelectParams(per)
        fill = lambda: (np.full((n, per, 2), 0x1111, np.int16), np.full((n, per), 0x22, np.uint8), np.full((n, per), 0x3333, np.uint16), np.full(n, 0x44444444, np.uint32))
        f0, r0, s0, c0 = fill()
        engine.select_refs_frame(w, h, sel, mv[1], cost[1], [0, 2], None, ctu_first=first, ctu_count=cnt, field=f0, ref=r0, slot=s0, ctu_cost=c0)
        mf, mr, ms, mc = model_select_refs(mv_cost, w, h, mv[1:], cost[1:], sel, [0, 2], None, first)
        assert np.array_equal(f0[rng_], mf[0]) and np.array_equal(r0[rng_], mr[0]) and np.array_equal(s0[rng_], ms[0]) and np.array_equal(c0[rng_], mc[0])
        for want_slot, want_cost in ((False, True), (True, False), (False, False)):
            f1, r1, s1, c1 = fill()
            assert engine.L.hmme_select_refs_frame(engine.h, w, h, 2, C.byref(fp), C.byref(sel), rcost, t_mv.ctypes.data, t_cost.ctypes.data, None, f1.ctypes.data,
                                                   r1.ctypes.data, s1.ctypes.data if want_slot else None, c1.ctypes.data if want_cost else None) == 0
            assert np.array_equal(f1, f0) and np.array_equal(r1, r0)
            assert np.array_equal(s1, s0) if want_slot else (s1 == 0x3333).all()
            assert np.array_equal(c1, c0) if want_cost else (c1 == 0x44444444).all()


# ---- 7: 64-bit merged costs -------------------------------------------------------------------------------------------------------------
def test_costs_near_uint32_max_in_every_reference(engine, mv_cost):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    mv, _ = srm.random_ref_tables(3, n, seed=81)
    rng = np.random.default_rng(82)
    cost = (0xFFFFFFFF - rng.integers(0, 4000, size=(3, n, 593))).astype(np.uint32)
    pred = srm.ref_predictors(3, n, seed=83)
    for per, unit, price, ref_cost in ((64, 0, 0, [0, 0, 0]), (256, 1, 1, [1 << 20, (1 << 20) - 900, (1 << 20) - 1800]), (64, 0, 1, [700, 0, 1400])):
        # every priced slot lies at or beyond 2^32 - 4000 (beyond 2^32 with the prices of the second case) and every CU beyond 2^32: compared
        # exactly in 64 bits
        sel = api.SelectParams(per, mv_unit=unit, price_mv=price, cu_cost=5000, pu_cost=3)
        _, mr, ms, mc = compare(engine, mv_cost, w, h, mv[None], cost[None], sel, ref_cost, pred[None])
        assert (mc == 0xFFFFFFFF).all()                                      # saturated on the way out
        assert set(mr[ms != sm.NO_SLOT].tolist()) == {0, 1, 2}               # a wrapped or saturated sum would not tell them apart


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):
    import torch
    from hmme import api
    L = api.load()
    w, h, n = 64, 64, 1
    mv, cost = srm.random_ref_tables(16, n, seed=91)
    d_mv, d_cost, _ = to_device(mv, cost, None)
    out = Outputs(16, n, 64)
    torch.cuda.synchronize()
    fp, sel = api.FrameParams(1, 0, 8, 0, n), api.SelectParams(64)
    u32 = lambda v: (C.c_uint32 * 17)(*v)

    def call(n_pics, n_refs, ref_cost, mv_p=d_mv.data_ptr(), cost_p=d_cost.data_ptr(), field_p=out.field.data_ptr(), ref_p=out.ref.data_ptr(),
             slot_p=out.slot.data_ptr(), cc_p=out.cc.data_ptr(), s=sel):
        return L.hmme_select_refs_device(engine.h, w, h, n_pics, n_refs, C.byref(fp), C.byref(s), ref_cost, mv_p, cost_p, None, field_p, ref_p, slot_p, cc_p, None)

    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        assert call(1, 17, None) == -1 and call(1, 0, None) == -1
        assert call(17, 1, None) == -1 and call(6, 3, None) == -1 and call(0, 1, None) == -1
        assert call(1, 4, u32([0, 0, 0, (1 << 20) + 1] + [0] * 13)) == -1
        assert call(1, 1, None, s=api.SelectParams(128)) == -1
        assert call(1, 1, None, ref_p=None) == -1                           # the reference indices are the point of the call
        assert call(1, 1, None, field_p=None) == -1 and call(1, 1, None, mv_p=None) == -1
        assert call(1, 1, None, mv_p=d_mv.data_ptr() + 2) == -1 and call(1, 1, None, cost_p=d_cost.data_ptr() + 2) == -1
        assert call(1, 1, None, field_p=out.field.data_ptr() + 4) == -1 and call(1, 1, None, ref_p=out.ref.data_ptr() + 1) == -1
        assert call(1, 1, None, slot_p=out.slot.data_ptr() + 2) == -1 and call(1, 1, None, cc_p=out.cc.data_ptr() + 2) == -1
        with pytest.raises(api.HmmeError):
            engine.select_refs_device(w, h, 1, 1, fp, sel, None, d_mv.data_ptr(), d_cost.data_ptr(), None, out.field.data_ptr(), None)
        torch.cuda.synchronize()
        assert out.untouched()
        assert call(16, 1, None) == 0 and call(1, 16, u32([1 << 20] * 17)) == 0   # the accepted neighbours do run
        torch.cuda.synchronize()
        assert not out.untouched()
    finally:
        L.hmme_set_error_printing(engine.h, prev)


# ---- 9: prediction with a reference per block --------------------------------------------------------------------------------------------
def three_planes(engine, w, h, bit_depth):
    from hmme import synth
    planes = []
    for k in range(3):
        _, ref, _ = synth.make_pair(w, h, seed=500 + 7 * k + bit_depth, bit_depth=bit_depth, max_mv=2)
        p = engine.plane(w, h, bit_depth)
        p.upload_pel(ref, (synth.MARGIN, synth.MARGIN))
        planes.append(p)
    return planes


def predict_inputs(n, per, seed):
    """(field int16[n, per, 2], ref_field uint8[n, per]) for three planes: quarter-pel MVs of all 16 phases (per = 1: six different ones) that
    also reach beyond TComDataCU::clipMv's range, reference indices 0..2 and, in some blocks, 3 (= n_refs) and 0xFF"""
    rng = np.random.default_rng(seed)
    field = rng.integers(-800, 801, size=(n, per, 2)).astype(np.int16)
    ref_field = rng.integers(0, 3, size=(n, per)).astype(np.uint8)
    if per == 1:
        field[:6, 0] = [(-700, 650), (5, -3), (-18, 7), (33, 2), (-1, -1), (14, 12)]
        ref_field[:6, 0] = [0, 1, 0xFF, 2, 3, 1]
    else:
        dead = rng.random((n, per)) < 0.15
        ref_field[dead] = np.where(rng.random(int(dead.sum())) < 0.5, 0xFF, 3).astype(np.uint8)
    assert len({(int(x) & 3, int(y) & 3) for x, y in field.reshape(-1, 2)}) == (16 if per == 64 else 6)
    assert (field[0, :, 0] < -4 * (64 + 8)).any() and (field[0, :, 1] > 4 * (72 + 8)).any()   # beyond the clip range at CTU 0, both axes
    assert {0, 1, 2, 3, 0xFF} <= set(ref_field.reshape(-1).tolist())
    return field, ref_field


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bit_depth", [8, 10])
def test_predict_refs_frame_is_predict_frame_block_by_block(engine, bit_depth, per):
    w, h = 136, 72
    n, ctus_x = n_ctus(w, h), 3
    planes = three_planes(engine, w, h, bit_depth)
    try:
        field, ref_field = predict_inputs(n, per, seed=600 + bit_depth + per)
        singles = [engine.predict_frame(p, field) for p in planes]
        assert not np.array_equal(singles[0], singles[1]) and not np.array_equal(singles[1], singles[2])
        dt = singles[0].dtype
        fill = 0xA5 if bit_depth == 8 else 0x2A5
        want = np.full((h, w), fill, dt)
        g = 64 if per == 1 else 8
        live = 0
        for c in range(n):
            for b in range(per):
                x0 = (c % ctus_x) * 64 + (b % 8) * g
                y0 = (c // ctus_x) * 64 + (b // 8) * g
                r = int(ref_field[c, b])
                if r < 3 and x0 < w and y0 < h:
                    want[y0:y0 + g, x0:x0 + g] = singles[r][y0:y0 + g, x0:x0 + g]
                    live += 1
        got = engine.predict_refs_frame(planes, field, ref_field, out=np.full((h, w), fill, dt))
        assert np.array_equal(got, want)
        assert live > 0 and (want == fill).any()
        # a CTU sub-range: the rest of the caller's image keeps its samples
        part = engine.predict_refs_frame(planes, field, ref_field, out=np.full((h, w), fill, dt), ctu_first=1, ctu_count=1)
        assert np.array_equal(part[:64, 64:128], want[:64, 64:128])
        part[:64, 64:128] = fill
        assert (part == fill).all()
        # ... and into an image whose stride exceeds the width
        from frame_helpers import check_strided_image
        ra = (C.c_void_p * 3)(*[p.h for p in planes])
        check_strided_image(w, h, bit_depth, lambda out, first, count: engine.predict_refs_frame(planes, field, ref_field, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_refs_frame(engine.h, ra, 3, C.byref(fp), field.ctypes.data, ref_field.ctypes.data, per, out, stride))
    finally:
        for p in planes:
            p.close()


def test_predict_refs_refuses_mixed_planes(engine):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    field, ref_field = np.zeros((n, 64, 2), np.int16), np.zeros((n, 64), np.uint8)
    other_engine = api.Engine(0, 64)
    a, b, small, deep, foreign = engine.plane(w, h), engine.plane(w, h), engine.plane(64, 64), engine.plane(w, h, 10), other_engine.plane(w, h)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        img = np.full((h, w), 0x5C, np.uint8)
        for refs in ([a, small], [a, b, deep], [a, foreign], [foreign, a]):
            with pytest.raises(api.HmmeError):
                engine.predict_refs_frame(refs, field, ref_field, out=img)
        for bad_field, bad_refs in ((field[:, :32], ref_field[:, :32]),):
            with pytest.raises(AssertionError):
                engine.predict_refs_frame([a, b], bad_field, bad_refs, out=img)
        fp = api.FrameParams(1, 0, 8, 0, -1)
        ra = (C.c_void_p * 17)(*([a.h] * 17))
        one = C.c_void_p(256)     # never dereferenced: refused before anything is launched
        assert L.hmme_predict_refs_device(engine.h, ra, 17, C.byref(fp), one, one, 64, one, w, None) == -1
        assert L.hmme_predict_refs_device(engine.h, ra, 0, C.byref(fp), one, one, 64, one, w, None) == -1
        assert L.hmme_predict_refs_device(engine.h, ra, 2, C.byref(fp), one, one, 256, one, w, None) == -1
        assert L.hmme_predict_refs_device(engine.h, ra, 2, C.byref(fp), one, None, 64, one, w, None) == -1
        assert L.hmme_predict_refs_device(engine.h, ra, 2, C.byref(fp), one, one, 64, one, w - 1, None) == -1
        assert (img == 0x5C).all()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (a, b, small, deep, foreign):
            p.close()
        other_engine.close()


# ---- 10: end to end: multi-reference search + refinement, the decision, the prediction ---------------------------------------------------
def test_end_to_end_two_references(engine, mv_cost):
    import torch
    from hmme import api, synth
    w, h, sr, m = 136, 72, 8, synth.MARGIN
    half = w // 2
    dev = torch.device("cuda", 0)
    cur_a, ref_a, _ = synth.make_pair(w, h, seed=701, max_mv=5, region=32)
    cur_b, ref_b, _ = synth.make_pair(w, h, seed=702, max_mv=5, region=32)
    cur_img = cur_a[m:m + h, m:m + w].copy()
    cur_img[:, half:] = cur_b[m:m + h, m + half:m + w]        # the left half moves out of reference 0, the right half out of reference 1
    planes = [engine.plane(w, h) for _ in range(3)]
    cur, refs = planes[0], planes[1:]
    try:
        cur.upload_pel(synth.pad_plane(cur_img), (m, m))
        refs[0].upload_pel(ref_a, (m, m))
        refs[1].upload_pel(ref_b, (m, m))
        n = n_ctus(w, h)
        fp = api.FrameParams(sr, 1, 8, 0, n)
        sel = api.SelectParams(64)
        ref_cost = srm.hm_ref_cost(2)
        d_mv = torch.zeros((2, n, 593, 2), dtype=torch.int16, device=dev); d_sad = torch.zeros((2, n, 593), dtype=torch.int32, device=dev)
        d_q = torch.zeros_like(d_mv); d_c = torch.zeros_like(d_sad)
        out = Outputs(1, n, 64)
        d_img = torch.full((h, w), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        engine.search_frame_multi_device(cur, refs, fp, None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_frame_multi_device(cur, refs, fp, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
        engine.select_refs_device(w, h, 1, 2, fp, sel, ref_cost, d_q.data_ptr(), d_c.data_ptr(), None, out.field.data_ptr(), out.ref.data_ptr(),
                                  out.slot.data_ptr(), out.cc.data_ptr(), 0)
        engine.predict_refs_device(refs, fp, out.field.data_ptr(), out.ref.data_ptr(), 64, d_img.data_ptr(), w, 0)
        torch.cuda.synchronize()
        qmv, cost = d_q.cpu().numpy(), d_c.cpu().numpy().view(np.uint32)
        field, ref, slot, cc = out.host()
        mf, mr, ms, mc = model_select_refs(mv_cost, w, h, qmv[None], cost[None], sel, ref_cost)
        assert np.array_equal(field, mf) and np.array_equal(ref, mr) and np.array_equal(slot, ms) and np.array_equal(cc, mc)
        # the chosen references follow the halves: counted on the model's field, block by block
        counts = {"left": [0, 0], "right": [0, 0]}
        for c in range(n):
            for b in range(64):
                x0 = (c % 3) * 64 + (b % 8) * 8
                if mr[0, c, b] == srm.NO_REF or x0 < half < x0 + 8:
                    continue                                   # no CU, or the block straddles the seam
                counts["left" if x0 < half else "right"][int(mr[0, c, b])] += 1
        assert np.array_equal(np.bincount(ref[ref != srm.NO_REF], minlength=2), np.bincount(mr[mr != srm.NO_REF], minlength=2))
        assert counts["left"][0] > counts["left"][1] and counts["right"][1] > counts["right"][0], counts
        assert (mr == srm.NO_REF).any() and (mr == 0).any() and (mr == 1).any()
        # the prediction: the model's field through the host call gives the same picture; blocks of no CU keep the sentinel
        pred = d_img.cpu().numpy()
        assert np.array_equal(pred, engine.predict_refs_frame(refs, mf[0], mr[0], out=np.full((h, w), 0xEE, np.uint8)))
        sad = lambda p: int(np.abs(p.astype(np.int32) - cur_img.astype(np.int32)).sum())
        for r in range(2):                                     # either reference alone: its own decision and prediction
            f1, _, _ = engine.select_frame(w, h, sel, qmv[r], cost[r])
            assert sad(pred) <= sad(engine.predict_frame(refs[r], f1))
    finally:
        for p in planes:
            p.close()
