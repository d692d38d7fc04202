"""L0, L1 or bi per PU on the device (hmme_select_dirs_device / _frame) against tests/select_dirs_model.py -- the rule of include/hmme.h
restated in Python integers -- bit for bit.  The decision reads tables, not pictures: the cases feed the recipes of select_dirs_model, of
which tests/test_select_dirs_cpu.py shows on the model alone that every direction and every tie occurs; the other cases assert on the
MODEL's result that the input exercises what the case is about.  The end-to-end chain on pictures is in tests/test_gpu_predict_bi.py."""
import ctypes as C

import numpy as np
import pytest

import select_dirs_model as sdm
import select_model as sm

pytestmark = pytest.mark.gpu

F_FILL, D_FILL, S_FILL, C_FILL = 0x5A5A, 0xA7, 0x1234, 0x0BADBEEF   # sentinels the outputs are preset with
ZERO_BITS = ((0, 0, 0), (0, 0))
n_ctus = sdm.n_ctus


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda_q16(sdm.LAMBDA_Q16)
    yield e
    e.close()


class Outputs:
    """the four outputs of one launch on the device, preset with the sentinels"""

    def __init__(self, n_pics, n):
        import torch
        dev = torch.device("cuda", 0)
        self.field = torch.full((n_pics, 2, n, 64, 2), F_FILL, dtype=torch.int16, device=dev)
        self.dir = torch.full((n_pics, n, 64), D_FILL, dtype=torch.uint8, device=dev)
        self.slot = torch.full((n_pics, n, 64), S_FILL, dtype=torch.int16, device=dev)
        self.cc = torch.full((n_pics, n), C_FILL, dtype=torch.int32, device=dev)

    def host(self):
        return self.field.cpu().numpy(), self.dir.cpu().numpy(), self.slot.cpu().numpy().view(np.uint16), self.cc.cpu().numpy().view(np.uint32)

    def untouched(self):
        f, d, s, c = self.host()
        return (f.view(np.uint16) == F_FILL).all() and (d == D_FILL).all() and (s == S_FILL).all() and (c == C_FILL).all()


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to(torch.device("cuda", 0))


def dir_params(bits):
    from hmme import api
    return api.DirParams(*bits)


def device_select_dirs(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1, want_slot=True, want_cost=True):
    """tabs = (mv_uni, cost_uni, mv_bi, cost_bi [n_pics, 2, count, 593, ...], uni_field [n_pics, 2, n_ctu, 64, 2]), bits = one
    (dir_bits, list_bits) per picture, pred int16[n_pics, 2, n_ctu, 2] or None -> the four outputs of ONE hmme_select_dirs_device launch as
    numpy arrays over ALL CTUs of the picture (sentinels where nothing was written)"""
    import torch
    from hmme import api
    n_pics, n = tabs[0].shape[0], n_ctus(w, h)
    cnt = n - first if count < 0 else count
    assert tabs[0].shape == tabs[2].shape == (n_pics, 2, cnt, 593, 2) and tabs[1].shape == tabs[3].shape == (n_pics, 2, cnt, 593)
    assert tabs[4].shape == (n_pics, 2, n, 64, 2) and (pred is None or pred.shape == (n_pics, 2, n, 2))
    d = [to_device(a) for a in tabs]
    d_pred = to_device(pred) if pred is not None else None
    out = Outputs(n_pics, n)
    torch.cuda.synchronize()
    fp = api.FrameParams(1, 0, 8, first, cnt)
    engine.select_dirs_device(w, h, n_pics, fp, sel, [dir_params(b) for b in bits], *[t.data_ptr() for t in d], d_pred.data_ptr() if d_pred is not None else None,
                              out.field.data_ptr(), out.dir.data_ptr(), out.slot.data_ptr() if want_slot else None, out.cc.data_ptr() if want_cost else None, 0)
    torch.cuda.synchronize()
    return out.host()


def model_select_dirs(w, h, tabs, sel, bits, pred=None, first=0, lambda_q16=sdm.LAMBDA_Q16):
    """the model over the same launch -> (field [n_pics, 2, count, 64, 2], dir, slot [n_pics, count, 64], cost [n_pics, count])"""
    res = [sdm.select_dirs_picture(*[t[i] for t in tabs], sel, w, h, bits[i], first, None if pred is None else pred[i], lambda_q16) for i in range(tabs[0].shape[0])]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


def compare(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1, lambda_q16=sdm.LAMBDA_Q16):
    """one launch against the model, the sentinels outside the CTU range included -> the model's (field, dir, slot, cost)"""
    got = device_select_dirs(engine, w, h, tabs, sel, bits, pred, first, count)
    want = model_select_dirs(w, h, tabs, sel, bits, pred, first, lambda_q16)
    cnt = tabs[0].shape[2]
    assert np.array_equal(got[0][:, :, first:first + cnt], want[0]), "field"
    for g, m, name in zip(got[1:], want[1:], ("dir", "slot", "cost")):
        assert np.array_equal(g[:, first:first + cnt], m), name
    outside = np.ones(got[1].shape[1], bool)
    outside[first:first + cnt] = False
    assert (got[0][:, :, outside].view(np.uint16) == F_FILL).all() and (got[1][:, outside] == D_FILL).all()
    assert (got[2][:, outside] == S_FILL).all() and (got[3][:, outside] == C_FILL).all()
    mf, md, ms, _ = want
    assert ((md == sdm.NO_DIR) == (ms == sm.NO_SLOT)).all() and set(md[ms != sm.NO_SLOT].tolist()) <= {1, 2, 3}
    return want


def one_picture(w, h, seed, pred=None, first=0, count=-1):
    n = n_ctus(w, h)
    cnt = n - first if count < 0 else count
    return tuple(a[None] for a in sdm.random_dir_tables(n, cnt, seed, pred, first))


# ---- 1: random tables at every size, HM-like and zero bits, distinct predictors per list -------------------------------------------------
@pytest.mark.parametrize("bits", [sdm.HM_BITS, ZERO_BITS])
@pytest.mark.parametrize("w,h", sdm.SIZES)
def test_random_tables(engine, w, h, bits):
    from hmme import api
    n = n_ctus(w, h)
    pred = sdm.predictors(n, seed=100 + w)
    assert (pred[0] != pred[1]).any()
    tabs = one_picture(w, h, 101 + w, pred)
    sel = api.SelectParams(64, min_depth=2 if n == 1 else 0, cu_cost=40, pu_cost=12)   # one CTU: CUs of 16x16 at most, so that there are several
    mf, md, ms, _ = compare(engine, w, h, tabs, sel, [bits], pred[None])
    assert set(md[ms != sm.NO_SLOT].tolist()) == {1, 2, 3}
    assert ((md == sdm.NO_DIR).any()) == (w != 64)
    # under a bi block the other list carries the INPUT field's block, which no table holds
    uni_field = tabs[4]
    bi = np.argwhere(md[0] == 3)
    assert len(bi) > 0
    hits = 0
    for c, b in bi:
        lists = [l for l in range(2) if tuple(mf[0, l, c, b]) == tuple(uni_field[0, l, c, b])]
        assert lists, (c, b)
        s = ms[0, c, b]
        hits += all(tuple(mf[0, l, c, b]) != tuple(tabs[0][0, l, c, s]) for l in lists)
    assert hits > 0


def test_pred_null_is_the_zero_predictor(engine):
    from hmme import api
    w, h = 100, 70
    tabs = one_picture(w, h, 150)
    sel = api.SelectParams(64)
    a = device_select_dirs(engine, w, h, tabs, sel, [sdm.HM_BITS], None)
    b = device_select_dirs(engine, w, h, tabs, sel, [sdm.HM_BITS], np.zeros((1, 2, n_ctus(w, h), 2), np.int16))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    compare(engine, w, h, tabs, sel, [sdm.HM_BITS], None)


# ---- 2: every tie of rules 3 and 4 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [sdm.HM_BITS, ZERO_BITS])
def test_every_tie_of_the_direction_rule(engine, bits):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    pred = sdm.predictors(n, seed=200)
    ties, pat = sdm.tie_tables(n, 201, bits, pred)
    assert set(pat.reshape(-1).tolist()) == set(range(27))
    engine.set_lambda_q16(1 << 16)                                             # the recipe's lambda: 1 per bit
    try:
        _, md, ms, _ = compare(engine, w, h, tuple(a[None] for a in ties), sdm.tie_sel(api), [bits], pred[None], lambda_q16=1 << 16)
    finally:
        engine.set_lambda_q16(sdm.LAMBDA_Q16)
    assert set(md[ms != sm.NO_SLOT].tolist()) == {1, 2, 3}
    coded = {sdm.TIE_PATTERNS[pat[c, s]] for c in range(n) for s in set(ms[0, c][ms[0, c] != sm.NO_SLOT].tolist())}
    assert (0, 0, 0) in coded and any(p[1] == p[2] for p in coded) and any(p[0] == 0 and min(p[1:]) > 0 for p in coded)   # ties that were coded


# ---- 3: the degenerate case is the reference choice --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", sdm.SIZES)
def test_without_bits_and_without_bi_it_is_select_refs_frame(engine, w, h):
    from hmme import api
    n = n_ctus(w, h)
    pred = sdm.predictors(n, seed=300)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = sdm.random_dir_tables(n, n, seed=301, pred=pred)
    cost_bi = np.full_like(cost_bi, 0xFFFFFFFF)
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12, min_depth=2)
    field, dirs, slot, cc = engine.select_dirs_frame(w, h, sel, api.DirParams(), mv_uni, cost_uni, mv_bi, cost_bi, uni_field, pred)
    rf, rr, rs, rc_ = engine.select_refs_frame(w, h, sel, mv_uni, cost_uni, None, pred)
    assert np.array_equal(slot, rs) and np.array_equal(cc, rc_)
    assert np.array_equal(dirs, np.where(rr == 0xFF, 0xFF, rr + 1).astype(np.uint8))
    for l in range(2):
        assert np.array_equal(field[l], np.where((rr == l)[..., None], rf, 0))
    assert {1, 2} <= set(dirs.reshape(-1).tolist()) and 3 not in dirs


# ---- 4: costs near UINT32_MAX ------------------------------------------------------------------------------------------------------------
def test_costs_near_uint32_max(engine):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    pred = sdm.predictors(n, seed=400)
    mv_uni, _, mv_bi, _, uni_field = sdm.random_dir_tables(n, n, seed=401, pred=pred)
    rng = np.random.default_rng(402)
    near = lambda top: (top - rng.integers(0, 4000, size=(2, n, 593))).astype(np.uint32)
    # every table within 4000 of UINT32_MAX: the halved bi distortion (about 2^31) wins every slot; two PUs already pass 2^32
    tabs = tuple(a[None] for a in (mv_uni, near(0xFFFFFFFF), mv_bi, near(0xFFFFFFFF), uni_field))
    sel = api.SelectParams(64, min_depth=2, cu_cost=5000, pu_cost=3)
    _, md, ms, mc = compare(engine, w, h, tabs, sel, [((4096, 4096, 4096), (4096, 4096))], pred[None])
    # saturated on the way out wherever the CTU holds two CUs of 2^31 and more; the corner CTU's single 8x8 CU leaves unsaturated
    assert (mc[0, :n - 1] == 0xFFFFFFFF).all() and 1 << 30 < mc[0, n - 1] < 0xFFFFFFFF and set(md[ms != sm.NO_SLOT].tolist()) == {3}
    # list 0 and bi at UINT32_MAX, list 1 around 2^31: list 1 and bi compete within a few thousand of each other
    cost_uni = np.stack([near(0xFFFFFFFF)[0], near(0x80000000 + 2000)[1]])
    tabs = tuple(a[None] for a in (mv_uni, cost_uni, mv_bi, near(0xFFFFFFFF), uni_field))
    _, md, ms, mc = compare(engine, w, h, tabs, sel, [sdm.HM_BITS], pred[None])
    assert (mc[0, :n - 1] == 0xFFFFFFFF).all() and set(md[ms != sm.NO_SLOT].tolist()) == {2, 3}   # a wrapped or saturated sum would not tell them apart


# ---- 5: several pictures, CTU sub-ranges, NULL outputs -----------------------------------------------------------------------------------
def test_two_pictures_with_different_bits_in_one_launch(engine):
    from hmme import api
    w, h = 136, 72
    n = n_ctus(w, h)
    pred = np.stack([sdm.predictors(n, seed=500), sdm.predictors(n, seed=501)])
    one = sdm.random_dir_tables(n, n, seed=502, pred=pred[0])
    tabs = tuple(np.stack([a, a]) for a in one)                                 # the same tables twice: the bits and predictors alone differ
    bits = [sdm.HM_BITS, ((40, 0, 90), (7, 300))]
    _, md, _, mc = compare(engine, w, h, tabs, api.SelectParams(64), bits, pred)
    assert not np.array_equal(md[0], md[1]) and not np.array_equal(mc[0], mc[1])
    four = tuple(np.stack([a] * 4) for a in one)                                # the largest launch
    compare(engine, w, h, four, api.SelectParams(64), [sdm.HM_BITS, ZERO_BITS, bits[1], sdm.HM_BITS], np.stack([pred[0], pred[1], pred[0], pred[1]]))


def test_ctu_sub_range_and_null_outputs(engine):
    from hmme import api
    w, h, first, cnt = 136, 72, 1, 4
    n = n_ctus(w, h)
    pred = np.stack([sdm.predictors(n, seed=600), sdm.predictors(n, seed=601)])
    pics = [sdm.random_dir_tables(n, cnt, 602 + i, pred[i], first) for i in range(2)]
    tabs = tuple(np.stack([pics[0][k], pics[1][k]]) for k in range(5))
    sel, bits = api.SelectParams(64), [sdm.HM_BITS, ZERO_BITS]
    mf, md, ms, mc = compare(engine, w, h, tabs, sel, bits, pred, first, cnt)   # sentinels outside the range: checked there
    f, d, s, c = device_select_dirs(engine, w, h, tabs, sel, bits, pred, first, cnt, want_slot=False, want_cost=False)
    assert np.array_equal(f[:, :, first:first + cnt], mf) and np.array_equal(d[:, first:first + cnt], md)
    assert (s == S_FILL).all() and (c == C_FILL).all()                          # NULL outputs: nothing written anywhere
    f, d, s, c = device_select_dirs(engine, w, h, tabs, sel, bits, pred, first, cnt, want_slot=True, want_cost=False)
    assert np.array_equal(s[:, first:first + cnt], ms) and (c == C_FILL).all()
    # the host-facing call into the caller's arrays: entries outside the range keep their values
    f0 = np.full((2, n, 64, 2), 0x1111, np.int16); d0 = np.full((n, 64), 0x22, np.uint8); s0 = np.full((n, 64), 0x3333, np.uint16); c0 = np.full(n, 0x44444444, np.uint32)
    engine.select_dirs_frame(w, h, sel, dir_params(bits[1]), *pics[1], pred[1], ctu_first=first, ctu_count=cnt, field=f0, dirs=d0, slot=s0, ctu_cost=c0)
    rng_ = slice(first, first + cnt)
    assert np.array_equal(f0[:, rng_], mf[1]) and np.array_equal(d0[rng_], md[1]) and np.array_equal(s0[rng_], ms[1]) and np.array_equal(c0[rng_], mc[1])
    out = np.ones(n, bool); out[rng_] = False
    assert (f0[:, out] == 0x1111).all() and (d0[out] == 0x22).all() and (s0[out] == 0x3333).all() and (c0[out] == 0x44444444).all()
    # ... with NULL for out_slot and out_cost
    fp, dp = api.FrameParams(1, 0, 8, first, cnt), dir_params(bits[1])
    host = [np.ascontiguousarray(a) for a in pics[1]]
    pq = np.ascontiguousarray(pred[1])
    f1 = np.full((2, n, 64, 2), 0x1111, np.int16); d1 = np.full((n, 64), 0x22, np.uint8)
    assert engine.L.hmme_select_dirs_frame(engine.h, w, h, C.byref(fp), C.byref(sel), C.byref(dp), *[a.ctypes.data for a in host], pq.ctypes.data, f1.ctypes.data,
                                           d1.ctypes.data, None, None) == 0
    assert np.array_equal(f1, f0) and np.array_equal(d1, d0)


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(engine):
    import torch
    from hmme import api
    L = api.load()
    w, h, n = 64, 64, 1
    one = sdm.random_dir_tables(n, n, seed=700)
    d = [to_device(np.stack([a] * 5)) for a in one]                             # room for the refused launch of five pictures
    out = Outputs(5, n)
    torch.cuda.synchronize()
    fp, sel = api.FrameParams(1, 0, 8, 0, n), api.SelectParams(64)
    dirs = lambda v=0: (api.DirParams * 5)(*[api.DirParams((0, 0, v), (0, 0))] * 5)
    ptr = dict(mv_uni=d[0].data_ptr(), cost_uni=d[1].data_ptr(), mv_bi=d[2].data_ptr(), cost_bi=d[3].data_ptr(), uni_field=d[4].data_ptr(), pred=None,
               field=out.field.data_ptr(), dir=out.dir.data_ptr(), slot=out.slot.data_ptr(), cc=out.cc.data_ptr())

    def call(n_pics=1, s=sel, dp=None, **over):
        p = dict(ptr, **over)
        return L.hmme_select_dirs_device(engine.h, w, h, n_pics, C.byref(fp), C.byref(s), dirs() if dp is None else dp, p["mv_uni"], p["cost_uni"], p["mv_bi"],
                                         p["cost_bi"], p["uni_field"], p["pred"], p["field"], p["dir"], p["slot"], p["cc"], None)

    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        assert call(5) == -1 and call(0) == -1
        assert call(s=api.SelectParams(64, price_mv=1)) == -1 and call(s=api.SelectParams(64, mv_unit=1)) == -1 and call(s=api.SelectParams(256)) == -1
        assert call(dp=dirs(4097)) == -1 and call(dp=C.cast(None, C.POINTER(api.DirParams))) == -1
        assert call(dir=None) == -1                                            # the directions are the point of the call
        for name in ("mv_uni", "cost_uni", "mv_bi", "cost_bi", "uni_field", "field"):
            assert call(**{name: None}) == -1, name
        for name, off in (("mv_uni", 2), ("cost_uni", 2), ("mv_bi", 2), ("cost_bi", 2), ("uni_field", 2), ("field", 4), ("dir", 1), ("slot", 2), ("cc", 2)):
            assert call(**{name: ptr[name] + off}) == -1, name
        assert call(pred=d[4].data_ptr() + 1) == -1
        with pytest.raises(api.HmmeError):
            engine.select_dirs_device(w, h, 1, fp, sel, [api.DirParams()], ptr["mv_uni"], ptr["cost_uni"], ptr["mv_bi"], ptr["cost_bi"], ptr["uni_field"], None,
                                      ptr["field"], None)
        torch.cuda.synchronize()
        assert out.untouched()
        assert call(4, dp=dirs(4096)) == 0                                      # the accepted neighbours do run
        torch.cuda.synchronize()
        f, dd, s, c = out.host()
        assert (dd[:4] != D_FILL).all() and (dd[4] == D_FILL).all() and (c[:4] != C_FILL).all() and (c[4] == C_FILL).all()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
