"""L0, L1 or bi and the reference index per list, per PU, on the device (hmme_select_dirs_refs_device / _frame) against
tests/select_dirs_refs_model.py -- the rule of include/hmme.h restated in Python integers -- bit for bit.  The decision reads tables, not
pictures: the cases feed the recipes of select_dirs_refs_model, of which tests/test_select_dirs_refs_cpu.py shows on the model alone that
every direction, every reference and the mask occur; the other cases assert on the MODEL's result that the input exercises what the case is
about.  Random tables hold no exact tie: the ties of rules 1-4 come from the hand-made scenarios of select_dirs_refs_model.  Tables of the engine go through the decision in tests/test_gpu_bipred_refs.py (the end-to-end case)."""
import ctypes as C

import numpy as np
import pytest

import lambda_cases as lc
import select_dirs_model as sdm
import select_dirs_refs_model as drm
import select_model as sm

pytestmark = pytest.mark.gpu

F_FILL, R_FILL, D_FILL, S_FILL, C_FILL = 0x5A5A, 0x6B, 0xA7, 0x1234, 0x0BADBEEF   # sentinels the outputs are preset with
n_ctus = sdm.n_ctus


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda_q16(drm.LAMBDA_Q16)
    yield e
    e.close()


class Outputs:
    """the five outputs of one launch on the device, preset with the sentinels"""

    def __init__(self, n_pics, n):
        import torch
        dev = torch.device("cuda", 0)
        self.field = torch.full((n_pics, 2, n, 64, 2), F_FILL, dtype=torch.int16, device=dev)
        self.ref = torch.full((n_pics, 2, n, 64), R_FILL, dtype=torch.uint8, device=dev)
        self.dir = torch.full((n_pics, n, 64), D_FILL, dtype=torch.uint8, device=dev)
        self.slot = torch.full((n_pics, n, 64), S_FILL, dtype=torch.int16, device=dev)
        self.cc = torch.full((n_pics, n), C_FILL, dtype=torch.int32, device=dev)

    def host(self):
        return (self.field.cpu().numpy(), self.ref.cpu().numpy(), self.dir.cpu().numpy(), self.slot.cpu().numpy().view(np.uint16),
                self.cc.cpu().numpy().view(np.uint32))

    def untouched(self):
        f, r, d, s, c = self.host()
        return (f.view(np.uint16) == F_FILL).all() and (r == R_FILL).all() and (d == D_FILL).all() and (s == S_FILL).all() and (c == C_FILL).all()


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to(torch.device("cuda", 0))


def dir_params(b):
    from hmme import api
    return api.DirRefsParams(b.dir_bits, b.n_refs, b.ref_bits, b.l1_valid_mask)


def device_select(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1, want_slot=True, want_cost=True):
    """tabs = (mv_uni, cost_uni, mv_bi, cost_bi [n_pics, 2, R, count, 593, ...], uni_field [n_pics, 2, n_ctu, 64, 2], uni_ref [n_pics, 2, n_ctu,
    64]), bits = one select_dirs_refs_model.Bits per picture, pred int16[n_pics, 2, R, n_ctu, 2] or None -> the five outputs of ONE
    hmme_select_dirs_refs_device launch as numpy arrays over ALL CTUs of the picture (sentinels where nothing was written)"""
    import torch
    from hmme import api
    n_pics, R, n = tabs[0].shape[0], tabs[0].shape[2], n_ctus(w, h)
    cnt = n - first if count < 0 else count
    assert tabs[0].shape == tabs[2].shape == (n_pics, 2, R, cnt, 593, 2) and tabs[1].shape == tabs[3].shape == (n_pics, 2, R, cnt, 593)
    assert tabs[4].shape == (n_pics, 2, n, 64, 2) and tabs[5].shape == (n_pics, 2, n, 64) and (pred is None or pred.shape == (n_pics, 2, R, n, 2))
    d = [to_device(a) for a in tabs]
    d_pred = to_device(pred) if pred is not None else None
    out = Outputs(n_pics, n)
    torch.cuda.synchronize()
    fp = api.FrameParams(1, 0, 8, first, cnt)
    engine.select_dirs_refs_device(w, h, n_pics, R, fp, sel, [dir_params(b) for b in bits], *[t.data_ptr() for t in d], d_pred.data_ptr() if d_pred is not None else None,
                                   out.field.data_ptr(), out.ref.data_ptr(), out.dir.data_ptr(), out.slot.data_ptr() if want_slot else None,
                                   out.cc.data_ptr() if want_cost else None, 0)
    torch.cuda.synchronize()
    return out.host()


def model_select(w, h, tabs, sel, bits, pred=None, first=0, lambda_q16=drm.LAMBDA_Q16):
    """the model over the same launch -> (field [n_pics, 2, count, 64, 2], ref [n_pics, 2, count, 64], dir, slot [n_pics, count, 64], cost [n_pics, count])"""
    res = [drm.select_dirs_refs_picture(*[t[i] for t in tabs], sel, w, h, bits[i], first, None if pred is None else pred[i], lambda_q16) for i in range(tabs[0].shape[0])]
    return tuple(np.stack([r[k] for r in res]) for k in range(5))


def compare(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1, lambda_q16=drm.LAMBDA_Q16):
    """one launch against the model, the sentinels outside the CTU range included -> the model's (field, ref, dir, slot, cost)"""
    got = device_select(engine, w, h, tabs, sel, bits, pred, first, count)
    want = model_select(w, h, tabs, sel, bits, pred, first, lambda_q16)
    cnt = tabs[0].shape[3]
    assert np.array_equal(got[0][:, :, first:first + cnt], want[0]), "field"
    assert np.array_equal(got[1][:, :, first:first + cnt], want[1]), "ref"
    for g, m, name in zip(got[2:], want[2:], ("dir", "slot", "cost")):
        assert np.array_equal(g[:, first:first + cnt], m), name
    outside = np.ones(got[2].shape[1], bool)
    outside[first:first + cnt] = False
    assert (got[0][:, :, outside].view(np.uint16) == F_FILL).all() and (got[1][:, :, outside] == R_FILL).all() and (got[2][:, outside] == D_FILL).all()
    assert (got[3][:, outside] == S_FILL).all() and (got[4][:, outside] == C_FILL).all()
    mf, mr, md, ms, _ = want
    assert ((md == drm.NO_DIR) == (ms == sm.NO_SLOT)).all() and set(md[ms != sm.NO_SLOT].tolist()) <= {1, 2, 3}
    return want


def one_picture(R, w, h, seed, pred=None, first=0, count=-1, lambda_q16=drm.LAMBDA_Q16):
    n = n_ctus(w, h)
    cnt = n - first if count < 0 else count
    return tuple(a[None] for a in drm.random_tables(R, n, cnt, seed, pred, first, lambda_q16))


# ---- 1: random tables at every size and every (n0, n1), HM-like bits, distinct predictors per list and reference, a mask ----------------------
@pytest.mark.parametrize("n0,n1,mask", [(1, 1, None), (2, 2, 0b10), (4, 4, 0b0101), (3, 1, None)])
@pytest.mark.parametrize("w,h", sdm.SIZES)
def test_random_tables(engine, w, h, n0, n1, mask):
    from hmme import api
    n, R = n_ctus(w, h), max(n0, n1)
    pred = drm.predictors(R, n, seed=100 + w + R)
    tabs = one_picture(R, w, h, 101 + w + n0 + n1, pred)
    sel = api.SelectParams(64, min_depth=2, cu_cost=40, pu_cost=12)             # CUs of 16x16 at most, so that there are many
    mf, mr, md, ms, _ = compare(engine, w, h, tabs, sel, [drm.hm_bits(n0, n1, mask)], pred[None])
    assert set(md[ms != sm.NO_SLOT].tolist()) == {1, 2, 3}
    assert ((md == drm.NO_DIR).any()) == (w != 64)
    full = (1 << n1) - 1 if mask is None else mask
    assert set(mr[0, 1][md[0] == 2].tolist()) <= {r for r in range(n1) if (full >> r) & 1}
    if w == 136:                                                              # enough CUs for every allowed reference to win
        assert set(mr[0, 1][md[0] == 2].tolist()) == {r for r in range(n1) if (full >> r) & 1} and set(mr[0, 0][md[0] == 1].tolist()) == set(range(n0))
    # under a bi block one list carries the INPUT field's block and reference index, which no table holds
    bi = np.argwhere(md[0] == 3)
    assert len(bi) > 0
    for c, b in bi:
        assert any(tuple(mf[0, l, c, b]) == tuple(tabs[4][0, l, c, b]) and mr[0, l, c, b] == tabs[5][0, l, c, b] for l in range(2)), (c, b)


def test_pred_null_is_the_zero_predictor(engine):
    from hmme import api
    w, h, R = 100, 70, 2
    tabs = one_picture(R, w, h, 150)
    sel, bits = api.SelectParams(64), [drm.hm_bits(2, 2)]
    a = device_select(engine, w, h, tabs, sel, bits, None)
    b = device_select(engine, w, h, tabs, sel, bits, np.zeros((1, 2, R, n_ctus(w, h), 2), np.int16))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    compare(engine, w, h, tabs, sel, bits, None)


def test_an_empty_mask_and_a_masked_out_cheapest_reference(engine):
    """list 1 far cheaper than list 0 and bi: with the whole mask direction 2 everywhere; without reference 0 -- the cheapest -- direction 2
    from reference 1; with an empty mask none"""
    from hmme import api
    w, h, R = 136, 72, 2
    n = n_ctus(w, h)
    pred = drm.predictors(R, n, seed=160)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref = drm.random_tables(R, n, n, 161, pred, base=6000)
    cost_uni = cost_uni.copy()
    cost_uni[1, 0] -= 5500
    cost_uni[1, 1] -= 3000
    cost_bi = cost_bi + np.uint32(12000)                                        # the halved bi distortion stays above list 0's
    tabs = tuple(a[None] for a in (mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref))
    sel = api.SelectParams(64, min_depth=2)
    for mask, dirs, refs1 in ((0b11, {2}, {0}), (0b10, {2}, {1}), (0b00, {1}, {drm.NO_REF})):
        _, mr, md, ms, _ = compare(engine, w, h, tabs, sel, [drm.hm_bits(2, 2, mask)], pred[None])
        coded = ms != sm.NO_SLOT
        assert set(md[coded].tolist()) == dirs and set(mr[0, 1][coded[0]].tolist()) == refs1, mask


def test_every_tie_of_the_reference_and_direction_rules(engine):
    """the hand-made scenarios of select_dirs_refs_model.tie_scenarios (tests/test_select_dirs_refs_cpu.py shows what the model makes of each)
    through the device: three references per list, list 1's cheapest outside the mask, every scenario in 2Nx2N slots of CUs of different
    depths with every other slot priced out of reach -- four pictures in one launch: the mask and the empty mask, each with HM-like and with
    all-zero bit counts.  Beyond the comparison with the model, every site of the field carries the winner the scenario states"""
    from hmme import api
    bits = drm.tie_bits(drm.TIE_MASK) + drm.tie_bits(0)
    made = [drm.tie_tables(b, seed=i) for i, b in enumerate(bits)]
    tabs = tuple(np.stack([m[0][k] for m in made]) for k in range(6))
    engine.set_lambda_q16(drm.TIE_LAMBDA_Q16)
    try:
        mf, mr, md, ms, _ = compare(engine, 64, 64, tabs, api.SelectParams(64), bits, None, lambda_q16=drm.TIE_LAMBDA_Q16)
    finally:
        engine.set_lambda_q16(drm.LAMBDA_Q16)
    scenarios, seen = drm.tie_scenarios(), set()
    for i, (b, (t, placed)) in enumerate(zip(bits, made)):
        assert set(ms[i, 0].tolist()) == set(placed)                            # every site is coded, nothing else
        for s, name in placed.items():
            d, bl, mv, refs = drm.tie_want(b.l1_valid_mask, scenarios[name])
            blocks = np.flatnonzero(ms[i, 0] == s)
            l = bl if d == 3 else d - 1
            assert (md[i, 0, blocks] == d).all() and (mf[i, l, 0, blocks] == mv).all() and (mr[i, l, 0, blocks] == refs[l]).all(), (i, name, s)
            if d == 3:                                                          # the other list: the block's own entries of the input fields
                assert np.array_equal(mf[i, 1 - l, 0, blocks], t[4][1 - l, 0, blocks]) and np.array_equal(mr[i, 1 - l, 0, blocks], t[5][1 - l, 0, blocks])
            else:
                assert (mf[i, 1 - l, 0, blocks] == 0).all() and (mr[i, 1 - l, 0, blocks] == drm.NO_REF).all()
            seen.add((name, len(blocks)))
    assert {n for n, _ in seen} == set(scenarios) and {c for _, c in seen} == {1, 4, 16}   # 8x8, 16x16 and 32x32 CUs


# ---- 2: with one reference per list it is hmme_select_dirs_frame -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", sdm.SIZES)
def test_with_one_reference_per_list_it_is_select_dirs_frame(engine, w, h):
    from hmme import api
    n = n_ctus(w, h)
    pred = sdm.predictors(n, seed=200 + w)
    t = drm.random_tables(1, n, n, 201 + w, pred[:, None])
    (mv_uni, cost_uni, mv_bi, cost_bi), uni_field = (a[:, 0] for a in t[:4]), t[4]
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12, min_depth=2)
    field, dirs, slot, cc = engine.select_dirs_frame(w, h, sel, api.DirParams(*sdm.HM_BITS), mv_uni, cost_uni, mv_bi, cost_bi, uni_field, pred)
    dp = api.DirRefsParams(sdm.HM_BITS[0], (1, 1), ([sdm.HM_BITS[1][0]], [sdm.HM_BITS[1][1]]), 1)
    zero = np.zeros((2, n, 64), np.uint8)
    f2, r2, d2, s2, c2 = engine.select_dirs_refs_frame(w, h, sel, dp, mv_uni[:, None], cost_uni[:, None], mv_bi[:, None], cost_bi[:, None], uni_field, zero, pred[:, None])
    assert np.array_equal(f2, field) and np.array_equal(d2, dirs) and np.array_equal(s2, slot) and np.array_equal(c2, cc)
    # every reference index 0: in the list(s) the direction names, 0xFF in the other
    for l in range(2):
        assert np.array_equal(r2[l], np.where((dirs == l + 1) | (dirs == 3), 0, 0xFF).astype(np.uint8))
    assert {1, 2, 3} <= set(dirs.reshape(-1).tolist())                       # about the recipe (tests/test_select_dirs_refs_cpu.py)


# ---- 3: costs near UINT32_MAX, and a lambda at which getCost wraps ------------------------------------------------------------------------
def test_costs_near_uint32_max(engine):
    from hmme import api
    w, h, R = 136, 72, 2
    n = n_ctus(w, h)
    pred = drm.predictors(R, n, seed=400)
    mv_uni, _, mv_bi, _, uni_field, uni_ref = drm.random_tables(R, n, n, seed=401, pred=pred)
    rng = np.random.default_rng(402)
    near = lambda top: (top - rng.integers(0, 4000, size=(2, R, n, 593))).astype(np.uint32)
    # every table within 4000 of UINT32_MAX: the halved bi distortion (about 2^31) wins every slot; two PUs already pass 2^32
    tabs = tuple(a[None] for a in (mv_uni, near(0xFFFFFFFF), mv_bi, near(0xFFFFFFFF), uni_field, uni_ref))
    sel = api.SelectParams(64, min_depth=2, cu_cost=5000, pu_cost=3)
    top = drm.Bits((4096, 4096, 4096), (2, 2), ([4096, 4096], [4096, 4096]))
    _, mr, md, ms, mc = compare(engine, w, h, tabs, sel, [top], pred[None])
    assert (mc[0, :n - 1] == 0xFFFFFFFF).all() and 1 << 30 < mc[0, n - 1] < 0xFFFFFFFF and set(md[ms != sm.NO_SLOT].tolist()) == {3}
    # the uni tables at UINT32_MAX and no bi to speak of in list 0's way: sums beyond 2^32 are compared as they are
    cost_uni = near(0xFFFFFFFF)
    cost_uni[1] = near(0x80000000 + 2000)[1]
    tabs = tuple(a[None] for a in (mv_uni, cost_uni, mv_bi, near(0xFFFFFFFF), uni_field, uni_ref))
    _, mr, md, ms, mc = compare(engine, w, h, tabs, sel, [drm.hm_bits(2, 2)], pred[None])
    assert (mc[0, :n - 1] == 0xFFFFFFFF).all() and set(md[ms != sm.NO_SLOT].tolist()) == {2, 3}   # a wrapped or saturated sum would not tell them apart
    assert set(mr[0, 1][md[0] == 2].tolist()) == {0, 1}


@pytest.mark.parametrize("lq", [lc.WRAP24, lc.ALL_ONES])
def test_a_lambda_at_which_get_cost_wraps(engine, lq):
    """distortion-only tables (written at lambda_q16 = 1) priced at lq: both uses of gc wrap and the floor of rule 1 is hit"""
    from hmme import api
    w, h, R = 100, 70, 3
    n = n_ctus(w, h)
    rng = np.random.default_rng(93)
    pred = rng.integers(-2000, 2001, size=(2, R, n, 2)).astype(np.int16)
    tabs = one_picture(R, w, h, 94, pred, lambda_q16=lc.TINY)
    engine.set_lambda_q16(lq)
    try:
        compare(engine, w, h, tabs, api.SelectParams(64, cu_cost=40, pu_cost=12), [drm.hm_bits(3, 2, 0b01)], pred[None], lambda_q16=lq)
    finally:
        engine.set_lambda_q16(drm.LAMBDA_Q16)


def test_eight_table_sets_per_list_the_limit(engine):
    """n_refs_max = 8 (kMaxDirRefs): n_refs = (8, 8) with a mask of bits 1, 4 and 7, and n_refs = (8, 5), where bit 7 lies beyond list 1's
    count and is refused, with bits 1 and 4; reference 7 of list 0 is the strict winner in some slots; nine sets are refused with the
    outputs untouched"""
    import torch
    from hmme import api
    w, h, R, n = 64, 64, 8, 1
    pred = drm.predictors(R, n, seed=800)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref = drm.random_tables(R, n, n, 801, pred)
    cost_uni = cost_uni.copy()
    rng = np.random.default_rng(802)
    cheap = rng.random(593) < 0.3                                               # list 0's last reference far below every other candidate there
    cost_uni[0, 7, 0, cheap] = cost_uni[:, :, 0][:, :, cheap].min(axis=(0, 1)) // 4
    tabs = tuple(a[None] for a in (mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref))
    sel = api.SelectParams(64, min_depth=2, cu_cost=40, pu_cost=12)
    p = [[pred[l][r][0] for r in range(R)] for l in range(2)]
    # bit 7 needs eight references in list 1 (include/hmme.h: mask bits below n_refs[1] only); with five, bits 1 and 4 are the mask
    for n_refs, mask in (((8, 8), 0b10010010), ((8, 5), 0b00010010)):
        bits = drm.hm_bits(*n_refs, mask)
        mf, mr, md, ms, _ = compare(engine, w, h, tabs, sel, [bits], pred[None])
        strict = 0
        for s in (int(v) for v in np.unique(ms[0, 0]) if v != sm.NO_SLOT):      # on the model: reference 7 wins direction 1 strictly, not by a tie
            slot_tabs = (mv_uni[:, :, 0, s], cost_uni[:, :, 0, s], mv_bi[:, :, 0, s], cost_bi[:, :, 0, s])
            d, _, c, _, refs = drm.slot_decide(*slot_tabs, p, bits, drm.LAMBDA_Q16)
            if (d, refs[0]) == (1, 7):
                without = drm.Bits(bits.dir_bits, (7, n_refs[1]), bits.ref_bits, mask)
                strict += drm.slot_decide(*slot_tabs, p, without, drm.LAMBDA_Q16)[2] > c
        assert strict >= 3 and 7 in mr[0, 0][md[0] == 1], n_refs
        allowed = {r for r in range(n_refs[1]) if (mask >> r) & 1}
        assert set(mr[0, 1][md[0] == 2].tolist()) <= allowed and len(allowed) == (3 if n_refs[1] == 8 else 2) and (md[0] == 2).any()
    assert api.select_dirs_refs_check(sel, 1, 8, [dir_params(drm.Bits(bits.dir_bits, (8, 5), bits.ref_bits, 0b10010010))]) == -1   # bit 7: list 1 has five
    # nine table sets per list: refused, nothing written (the tables need not be that large: they are not read)
    d = [to_device(a) for a in tabs]
    out = Outputs(1, n)
    torch.cuda.synchronize()
    L = api.load()
    fp = api.FrameParams(1, 0, 8, 0, n)
    dp = (api.DirRefsParams * 1)(dir_params(bits))
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        call = lambda r: L.hmme_select_dirs_refs_device(engine.h, w, h, 1, r, C.byref(fp), C.byref(sel), dp, *[t.data_ptr() for t in d], None, out.field.data_ptr(),
                                                        out.ref.data_ptr(), out.dir.data_ptr(), out.slot.data_ptr(), out.cc.data_ptr(), None)
        assert call(9) == -1 and api.select_dirs_refs_check(sel, 1, 9, [dir_params(bits)]) == -1
        torch.cuda.synchronize()
        assert out.untouched()
        assert call(8) == 0                                                     # the accepted neighbour does run
        torch.cuda.synchronize()
        assert not out.untouched()
    finally:
        L.hmme_set_error_printing(engine.h, prev)


# ---- 4: several pictures, the partition limits, CTU sub-ranges, NULL outputs ---------------------------------------------------------------
def test_four_pictures_with_different_parameters_in_one_launch(engine):
    from hmme import api
    w, h, R = 136, 72, 4
    n = n_ctus(w, h)
    pred = np.stack([drm.predictors(R, n, seed=500 + i) for i in range(4)])
    one = drm.random_tables(R, n, n, seed=502, pred=pred[0])
    tabs = tuple(np.stack([a] * 4) for a in one)                                # the same tables four times: bits, counts, masks and predictors differ
    bits = [drm.hm_bits(4, 4), drm.hm_bits(2, 3, 0b100), drm.Bits((40, 0, 90), (1, 4), ([7], [300, 0, 5, 9]), 0b1010), drm.hm_bits(3, 1, 0)]
    _, mr, md, _, mc = compare(engine, w, h, tabs, api.SelectParams(64), bits, pred)
    assert len({md[i].tobytes() for i in range(4)}) == 4 and len({mc[i].tobytes() for i in range(4)}) == 4
    assert 2 not in md[3] and set(mr[1, 0][md[1] == 1].tolist()) == {0, 1} and set(mr[1, 1][md[1] == 2].tolist()) == {2}   # an empty mask; two references; a mask of one


@pytest.mark.parametrize("limits", [dict(part_mask=0x01), dict(part_mask=0x07), dict(min_depth=2, max_depth=2), dict(min_depth=1, max_depth=2),
                                    dict(min_depth=0, max_depth=0), dict(min_depth=3, max_depth=3, cu_cost=1 << 20, pu_cost=1 << 20), dict(min_depth=1, max_depth=3)],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_part_mask_and_depth_limits(engine, limits):
    """the limits of tests/test_gpu_select.py::test_part_mask_restrictions"""
    from hmme import api
    w, h, R = 100, 70, 2
    n = n_ctus(w, h)
    pred = drm.predictors(R, n, seed=550)
    tabs = one_picture(R, w, h, 551, pred)
    compare(engine, w, h, tabs, api.SelectParams(64, **limits), [drm.hm_bits(2, 2)], pred[None])


def test_ctu_sub_range_and_null_outputs(engine):
    from hmme import api
    w, h, first, cnt, R = 136, 72, 1, 4, 2
    n = n_ctus(w, h)
    pred = np.stack([drm.predictors(R, n, seed=600), drm.predictors(R, n, seed=601)])
    pics = [drm.random_tables(R, n, cnt, 602 + i, pred[i], first) for i in range(2)]
    tabs = tuple(np.stack([pics[0][k], pics[1][k]]) for k in range(6))
    sel, bits = api.SelectParams(64), [drm.hm_bits(2, 2), drm.hm_bits(1, 2, 0b10)]
    mf, mr, md, ms, mc = compare(engine, w, h, tabs, sel, bits, pred, first, cnt)   # sentinels outside the range: checked there
    f, r, d, s, c = device_select(engine, w, h, tabs, sel, bits, pred, first, cnt, want_slot=False, want_cost=False)
    rng_ = slice(first, first + cnt)
    assert np.array_equal(f[:, :, rng_], mf) and np.array_equal(r[:, :, rng_], mr) and np.array_equal(d[:, rng_], md)
    assert (s == S_FILL).all() and (c == C_FILL).all()                          # NULL outputs: nothing written anywhere
    f, r, d, s, c = device_select(engine, w, h, tabs, sel, bits, pred, first, cnt, want_slot=True, want_cost=False)
    assert np.array_equal(s[:, rng_], ms) and (c == C_FILL).all()
    f, r, d, s, c = device_select(engine, w, h, tabs, sel, bits, pred, first, cnt, want_slot=False, want_cost=True)
    assert np.array_equal(c[:, rng_], mc) and (s == S_FILL).all()
    # the host-facing call into the caller's arrays: entries outside the range keep their values
    f0 = np.full((2, n, 64, 2), 0x1111, np.int16); r0 = np.full((2, n, 64), 0x55, np.uint8); d0 = np.full((n, 64), 0x22, np.uint8)
    s0 = np.full((n, 64), 0x3333, np.uint16); c0 = np.full(n, 0x44444444, np.uint32)
    engine.select_dirs_refs_frame(w, h, sel, dir_params(bits[1]), *pics[1], pred[1], ctu_first=first, ctu_count=cnt, field=f0, ref=r0, dirs=d0, slot=s0, ctu_cost=c0)
    assert np.array_equal(f0[:, rng_], mf[1]) and np.array_equal(r0[:, rng_], mr[1]) and np.array_equal(d0[rng_], md[1]) and np.array_equal(s0[rng_], ms[1])
    assert np.array_equal(c0[rng_], mc[1])
    out = np.ones(n, bool); out[rng_] = False
    assert (f0[:, out] == 0x1111).all() and (r0[:, out] == 0x55).all() and (d0[out] == 0x22).all() and (s0[out] == 0x3333).all() and (c0[out] == 0x44444444).all()
    # ... with NULL for out_slot and out_cost
    fp, dp = api.FrameParams(1, 0, 8, first, cnt), dir_params(bits[1])
    host = [np.ascontiguousarray(a) for a in pics[1]]
    pq = np.ascontiguousarray(pred[1])
    f1 = np.full((2, n, 64, 2), 0x1111, np.int16); r1 = np.full((2, n, 64), 0x55, np.uint8); d1 = np.full((n, 64), 0x22, np.uint8)
    assert engine.L.hmme_select_dirs_refs_frame(engine.h, w, h, R, C.byref(fp), C.byref(sel), C.byref(dp), *[a.ctypes.data for a in host], pq.ctypes.data,
                                                f1.ctypes.data, r1.ctypes.data, d1.ctypes.data, None, None) == 0
    assert np.array_equal(f1, f0) and np.array_equal(r1, r0) and np.array_equal(d1, d0)


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):
    import torch
    from hmme import api
    L = api.load()
    w, h, n, R = 64, 64, 1, 2
    one = drm.random_tables(R, n, n, seed=700)
    d = [to_device(np.stack([a] * 5)) for a in one]                             # room for the refused launch of five pictures
    out = Outputs(5, n)
    torch.cuda.synchronize()
    fp, sel = api.FrameParams(1, 0, 8, 0, n), api.SelectParams(64)
    D = api.DirRefsParams
    dirs = lambda **kw: (D * 5)(*[D(**dict(dict(n_refs=(2, 2)), **kw))] * 5)
    ptr = dict(mv_uni=d[0].data_ptr(), cost_uni=d[1].data_ptr(), mv_bi=d[2].data_ptr(), cost_bi=d[3].data_ptr(), uni_field=d[4].data_ptr(), uni_ref=d[5].data_ptr(),
               pred=None, field=out.field.data_ptr(), ref=out.ref.data_ptr(), dir=out.dir.data_ptr(), slot=out.slot.data_ptr(), cc=out.cc.data_ptr())

    def call(n_pics=1, s=sel, dp=None, r=R, **over):
        p = dict(ptr, **over)
        return L.hmme_select_dirs_refs_device(engine.h, w, h, n_pics, r, C.byref(fp), C.byref(s), dirs() if dp is None else dp, p["mv_uni"], p["cost_uni"], p["mv_bi"],
                                              p["cost_bi"], p["uni_field"], p["uni_ref"], p["pred"], p["field"], p["ref"], p["dir"], p["slot"], p["cc"], None)

    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        assert call(5) == -1 and call(0) == -1 and call(r=0) == -1 and call(r=9) == -1 and call(r=1) == -1   # (r = 1: n_refs 2 above it)
        assert call(s=api.SelectParams(64, price_mv=1)) == -1 and call(s=api.SelectParams(64, mv_unit=1)) == -1 and call(s=api.SelectParams(256)) == -1
        assert call(dp=dirs(dir_bits=(0, 0, 4097))) == -1 and call(dp=dirs(ref_bits=([0, 4097], [0, 0]))) == -1 and call(dp=C.cast(None, C.POINTER(D))) == -1
        assert call(dp=dirs(n_refs=(0, 1))) == -1 and call(dp=dirs(n_refs=(2, 3))) == -1 and call(dp=dirs(l1_valid_mask=0b100)) == -1
        assert call(dir=None) == -1 and call(ref=None) == -1                    # directions and references are the point of the call
        for name in ("mv_uni", "cost_uni", "mv_bi", "cost_bi", "uni_field", "uni_ref", "field"):
            assert call(**{name: None}) == -1, name
        for name, off in (("mv_uni", 2), ("cost_uni", 2), ("mv_bi", 2), ("cost_bi", 2), ("uni_field", 2), ("field", 4), ("slot", 2), ("cc", 2)):
            assert call(**{name: ptr[name] + off}) == -1, name
        assert call(pred=d[4].data_ptr() + 1) == -1
        with pytest.raises(api.HmmeError):
            engine.select_dirs_refs_device(w, h, 1, R, fp, sel, [D(n_refs=(2, 2))], ptr["mv_uni"], ptr["cost_uni"], ptr["mv_bi"], ptr["cost_bi"], ptr["uni_field"],
                                           ptr["uni_ref"], None, ptr["field"], ptr["ref"], None)
        torch.cuda.synchronize()
        assert out.untouched()
        assert call(4, dp=dirs(dir_bits=(4096, 4096, 4096))) == 0               # the accepted neighbours do run
        torch.cuda.synchronize()
        f, rr, dd, s, c = out.host()
        assert (dd[:4] != D_FILL).all() and (dd[4] == D_FILL).all() and (c[:4] != C_FILL).all() and (c[4] == C_FILL).all()
        assert (rr[:4] != R_FILL).all() and (rr[4] == R_FILL).all()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
