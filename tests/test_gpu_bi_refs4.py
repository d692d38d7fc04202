"""B pictures with several references per list from one MV per 4x4 block on the device (the "bi_refs4" family of include/hmme.h: the bi pass
against an origin built from a 4x4 field with a reference index per block, the L0 / L1 / bi decision with the reference per list over all
593 slots, the luma and 4:2:0 prediction from its output), bit for bit against two yardsticks: tests/bi_refs4_model.py (pinned to the models
of the 64 forms and of the bi4 family by tests/test_bi_refs4_cpu.py, which also examines the content used here) and the existing device calls
-- the bi_refs family on replicated fields and quadrant by quadrant, the bi4 family with one reference per list.  Every output is
sentinel-filled: what is not written keeps the sentinel.  Pictures are one to six CTUs."""
import ctypes as C

import numpy as np
import pytest

import bi4_model as b4
import bi_refs4_model as br4
import predict4_model as p4
import residual_model as rm
import select_dirs_model as sdm
import select_dirs_refs_model as drm
import select_model as sm
import select_refs_model as srm
from frame_helpers import bind_hmo, check_strided_image, dims, mkplane, oracle_bi_search, random_field, three_planes

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5
F_FILL, R_FILL, D_FILL, S_FILL, C_FILL = 0x5A5A, 0xC3, 0xA7, 0x1234, 0x0BADBEEF   # sentinels the decision's outputs are preset with


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda_q16(sdm.LAMBDA_Q16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def sentinel(bd):
    return (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)


def fill(w, h, bd, dtype=None):
    dt, v = sentinel(bd)
    return np.full((h, w), v, dtype or dt)


def fills(w, h, bd, dtype=None):
    return tuple(fill(w // 2, h // 2, bd, dtype) for _ in range(2))


def same(got, want, what):
    assert np.array_equal(got, want), (what, np.argwhere(np.asarray(got) != np.asarray(want))[:4])


def same2(got, want, what):
    for c in range(2):
        same(got[c], want[c], (what, "Cb" if c == 0 else "Cr"))


class Scene:
    """the references of both lists (n0, n1 of them) of a w x h B picture at one depth: luma and, for even sizes with at most 8 references in
    all, Cb and Cr -- padded arrays for the models, planes for the engine; all textures unrelated"""

    def __init__(self, engine, w, h, bd, n0, n1, seed, chroma=True):
        from hmme import synth
        self.w, self.h, self.bd, self.n = w, h, bd, (n0, n1)
        tex = lambda pw, ph, s: synth.make_pair(pw, ph, seed=s, bit_depth=bd, max_mv=2)[1]
        self.luma = [[tex(w, h, seed + 13 * (16 * l + r)) for r in range(self.n[l])] for l in range(2)]
        self.y = [[mkplane(engine, a, w, h, bd) for a in lst] for lst in self.luma]
        self.chroma = chroma and w % 2 == 0 and h % 2 == 0 and w >= 16 and h >= 16 and n0 + n1 <= 8
        self.c_arrays, self.c_planes = [], []
        if self.chroma:   # arrays [component][list][reference]; planes [list] = [cb0, cr0, cb1, cr1, ...]
            self.c_arrays = [[[tex(w // 2, h // 2, seed + 500 + 7 * (16 * l + r) + 3 * c) for r in range(self.n[l])] for l in range(2)] for c in range(2)]
            self.c_planes = [[mkplane(engine, self.c_arrays[c][l][r], w // 2, h // 2, bd) for r in range(self.n[l]) for c in range(2)] for l in range(2)]

    def close(self):
        for p in [p for lst in self.y for p in lst] + [p for lst in self.c_planes for p in lst]:
            p.close()


def check_rule(engine, hmo, sc, field, dirs, refs, ctus=None, first=0, count=-1):
    """one field through the luma call (and the chroma call) against both yardsticks -> the luma image"""
    w, h, bd = sc.w, sc.h, sc.bd
    kw = dict(ctu_first=first, ctu_count=count)
    got = engine.predict_bi_refs4_frame(sc.y[0], sc.y[1], field, dirs, refs, out=fill(w, h, bd), **kw)
    same(got, br4.luma_picture(hmo, sc.luma[0], sc.luma[1], w, h, bd, field, dirs, refs, fill(w, h, bd, np.int64), ctus), ("model", w, h, bd))
    quads = br4.quadrant_fields(field, dirs, refs)
    images = [engine.predict_bi_refs_frame(sc.y[0], sc.y[1], fq, dq, rq, out=fill(w, h, bd), **kw) for fq, dq, rq in quads]
    same(got, p4.compose(images, w, h), ("four calls of the 64 form", w, h, bd))
    if sc.chroma:
        got_c = engine.predict_chroma_bi_refs4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, refs, outs=fills(w, h, bd), **kw)
        same2(got_c, br4.chroma_picture(hmo, sc.c_arrays, w, h, bd, field, dirs, refs, fills(w, h, bd, np.int64), ctus), ("chroma model", w, h, bd))
        images = [engine.predict_chroma_bi_refs_frame(sc.c_planes[0], sc.c_planes[1], w, h, fq, dq, rq, outs=fills(w, h, bd), **kw) for fq, dq, rq in quads]
        same2(got_c, [p4.compose([im[c] for im in images], w, h, 2) for c in range(2)], ("four chroma calls of the 64 form", w, h, bd))
    return got


# ---- 1: the prediction on replicated fields ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,bd,n", [((64, 64), 8, (2, 2)), ((101, 71), 10, (4, 4)), ((65, 67), 12, (16, 1)), ((130, 66), 8, (4, 4)), ((16, 16), 10, (2, 2)),
                                       ((9, 9), 12, (4, 4)), ((130, 66), 12, (2, 2)), ((64, 64), 10, (16, 1))])
def test_replicated_fields_give_the_images_of_the_64_forms(engine, size, bd, n):
    """101 x 71: the last 4x4 column is one sample wide; 65 x 67 and 9 x 9: luma only; 130 x 66: odd chroma planes (65 x 33)"""
    w, h = size
    n0, n1 = n
    nc = dims(w, h)[0] * dims(w, h)[1]
    sc = Scene(engine, w, h, bd, n0, n1, seed=5000 + w + bd)
    try:
        rng = np.random.default_rng(5003 + w + bd)
        field64 = np.stack([random_field(nc, 64, 5001 + l + w, max_pel=20) for l in range(2)])
        dirs64 = rng.choice(np.array([1, 2, 3, 3, 0xFF, 0], np.uint8), size=(nc, 64))
        refs64 = np.stack([rng.choice(np.array(list(range(k)) * 3 + [0xFF, k], np.uint8), size=(nc, 64)) for k in n])
        field, dirs, refs = br4.replicate3(field64, dirs64, refs64)
        got = engine.predict_bi_refs4_frame(sc.y[0], sc.y[1], field, dirs, refs, out=fill(w, h, bd))
        same(got, engine.predict_bi_refs_frame(sc.y[0], sc.y[1], field64, dirs64, refs64, out=fill(w, h, bd)), ("luma", size, bd))
        assert (got != sentinel(bd)[1]).any()
        if sc.chroma:
            got_c = engine.predict_chroma_bi_refs4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, refs, outs=fills(w, h, bd))
            same2(got_c, engine.predict_chroma_bi_refs_frame(sc.c_planes[0], sc.c_planes[1], w, h, field64, dirs64, refs64, outs=fills(w, h, bd)), ("chroma", size, bd))
            assert not np.array_equal(got_c[0], got_c[1])
        else:
            assert w % 2 or n0 + n1 > 8
    finally:
        sc.close()


@pytest.mark.parametrize("size,bd", [((101, 71), 10), ((130, 66), 8), ((16, 16), 12)])
def test_one_reference_per_list_gives_the_images_of_the_bi4_forms(engine, size, bd):
    w, h = size
    nc = dims(w, h)[0] * dims(w, h)[1]
    sc = Scene(engine, w, h, bd, 1, 1, seed=5050 + w)
    try:
        field, dirs = b4.random_field_bi4(w, h, 5051 + w)
        refs = np.zeros((2, nc, 256), np.uint8)
        got = engine.predict_bi_refs4_frame(sc.y[0], sc.y[1], field, dirs, refs, out=fill(w, h, bd))
        same(got, engine.predict_bi4_frame(sc.y[0][0], sc.y[1][0], field, dirs, out=fill(w, h, bd)), ("luma", size, bd))
        assert (got != sentinel(bd)[1]).any()
        if sc.chroma:
            got_c = engine.predict_chroma_bi_refs4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, refs, outs=fills(w, h, bd))
            same2(got_c, engine.predict_chroma_bi4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, outs=fills(w, h, bd)), ("chroma", size, bd))
    finally:
        sc.close()


# ---- 2: the prediction on random 4x4 fields -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", br4.FIELD_CASES, ids=str)
def test_the_rule_on_random_4x4_fields(engine, hmo, case):
    """directions in thirds plus 0xFF and 0, every index of both lists plus 0xFF and n, MVs at +-32767 on bi blocks, the index changing
    block by block across the picture edge: against the model AND against four calls of the 64 forms composed quadrant by quadrant"""
    (w, h), bd, (n0, n1), seed = case
    sc = Scene(engine, w, h, bd, n0, n1, seed=seed + 50)
    try:
        field, dirs, refs = br4.random_field_bi_refs4(w, h, n0, n1, seed)
        got = check_rule(engine, hmo, sc, field, dirs, refs)
        sv = sentinel(bd)[1]
        assert (got != sv).any() and ((got == sv).any() or w < 64)                      # dead blocks keep the sentinel
    finally:
        sc.close()


def test_ctu_sub_range_and_strided_image(engine, hmo):
    w, h, bd = 136, 72, 8
    sc = Scene(engine, w, h, bd, 2, 3, seed=5300)
    try:
        field, dirs, refs = br4.random_field_bi_refs4(w, h, 2, 3, 5301)
        sv = sentinel(bd)[1]
        for first, count in ((1, 2), (4, 1), (2, 0)):
            got = check_rule(engine, hmo, sc, field, dirs, refs, ctus=range(first, first + count), first=first, count=count)
            assert ((got != sv).any()) == (count > 0)
        hs = lambda ps: (C.c_void_p * len(ps))(*[p.h for p in ps])
        check_strided_image(w, h, bd, lambda out, first, count: engine.predict_bi_refs4_frame(sc.y[0], sc.y[1], field, dirs, refs, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_bi_refs4_frame(engine.h, hs(sc.y[0]), 2, hs(sc.y[1]), 3, C.byref(fp), field.ctypes.data,
                                                                                        dirs.ctypes.data, refs.ctypes.data, out, stride))
    finally:
        sc.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_device_entries(engine, bd):
    """the device forms on device buffers with pitches wider than a row; the _frame forms are the yardstick"""
    import torch
    from hmme import api
    w, h = 100, 70
    dev = torch.device("cuda", 0)
    sc = Scene(engine, w, h, bd, 4, 4, seed=5400 + bd)
    try:
        dt, sv = sentinel(bd)
        bps = 1 if bd == 8 else 2
        to_dev = lambda a: torch.from_numpy(a if a.dtype != np.uint16 else a.view(np.int16)).to(dev)
        field, dirs, refs = br4.random_field_bi_refs4(w, h, 4, 4, 5401 + bd)
        d_field, d_dirs, d_refs = to_dev(field), to_dev(dirs), to_dev(refs)
        fp = api.FrameParams(1, 0, bd, 0, -1)
        d_y = to_dev(np.full((h, w + 12), sv, dt))
        d_c = [to_dev(np.full((h // 2, w // 2 + 12), sv, dt)) for _ in range(2)]
        torch.cuda.synchronize()
        engine.predict_bi_refs4_device(sc.y[0], sc.y[1], fp, d_field.data_ptr(), d_dirs.data_ptr(), d_refs.data_ptr(), d_y.data_ptr(), (w + 12) * bps)
        engine.predict_chroma_bi_refs4_device(sc.c_planes[0], sc.c_planes[1], w, h, fp, d_field.data_ptr(), d_dirs.data_ptr(), d_refs.data_ptr(), d_c[0].data_ptr(),
                                              d_c[1].data_ptr(), (w // 2 + 12) * bps)
        torch.cuda.synchronize()
        want = [engine.predict_bi_refs4_frame(sc.y[0], sc.y[1], field, dirs, refs, out=fill(w, h, bd))]
        want += list(engine.predict_chroma_bi_refs4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, refs, outs=fills(w, h, bd)))
        for k, (d_img, wanted) in enumerate(zip([d_y] + d_c, want)):
            back = d_img.cpu().numpy().view(dt)
            pw = wanted.shape[1]
            same(back[:, :pw], wanted, ("device", k))
            assert (back[:, pw:] == sv).all() and (wanted != sv).any()
    finally:
        sc.close()


def test_a_used_context_gives_what_a_fresh_one_gives(engine):
    """the module's engine has run every call of this file (and runs a 64-form call first); a context made here has run nothing"""
    from hmme import api
    w, h, bd = 100, 70, 10
    field, dirs, refs = br4.random_field_bi_refs4(w, h, 2, 2, 5501)
    results = []
    fresh = api.Engine(0, 64)
    try:
        for e in (engine, fresh):
            sc = Scene(e, w, h, bd, 2, 2, seed=5500)
            try:
                if e is engine:
                    fq, dq, rq = br4.quadrant_fields(field, dirs, refs)[0]
                    e.predict_bi_refs_frame(sc.y[0], sc.y[1], fq, dq, rq)
                results.append((e.predict_bi_refs4_frame(sc.y[0], sc.y[1], field, dirs, refs, out=fill(w, h, bd)),
                                *e.predict_chroma_bi_refs4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, refs, outs=fills(w, h, bd))))
            finally:
                sc.close()
    finally:
        fresh.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b) and (a != sentinel(bd)[1]).any()


# ---- 3: the decision -----------------------------------------------------------------------------------------------------------------------
def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to(torch.device("cuda", 0))


def dir_params(api, bits):
    return api.DirRefsParams(bits.dir_bits, bits.n_refs, bits.ref_bits, bits.l1_valid_mask)


def device_select(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1):
    """tabs = (mv_uni, cost_uni, mv_bi, cost_bi [n_pics, 2, R, count, 593, ...], uni_field [n_pics, 2, n_ctu, 256, 2], uni_ref [n_pics, 2, n_ctu,
    256]), bits = one select_dirs_refs_model.Bits per picture -> the five outputs of ONE hmme_select_dirs_refs4_device launch over ALL CTUs
    (sentinels where nothing was written)"""
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    n_pics, R, n = tabs[0].shape[0], tabs[0].shape[2], sdm.n_ctus(w, h)
    cnt = n - first if count < 0 else count
    assert tabs[0].shape == (n_pics, 2, R, cnt, 593, 2) and tabs[4].shape == (n_pics, 2, n, 256, 2) and tabs[5].shape == (n_pics, 2, n, 256)
    d = [to_device(a) for a in tabs]
    d_pred = to_device(pred) if pred is not None else None
    field = torch.full((n_pics, 2, n, 256, 2), F_FILL, dtype=torch.int16, device=dev)
    ref = torch.full((n_pics, 2, n, 256), R_FILL, dtype=torch.uint8, device=dev)
    dirs = torch.full((n_pics, n, 256), D_FILL, dtype=torch.uint8, device=dev)
    slot = torch.full((n_pics, n, 256), S_FILL, dtype=torch.int16, device=dev)
    cc = torch.full((n_pics, n), C_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.select_dirs_refs4_device(w, h, n_pics, R, api.FrameParams(1, 0, 8, first, cnt), sel, [dir_params(api, b) for b in bits], *[t.data_ptr() for t in d],
                                    d_pred.data_ptr() if d_pred is not None else None, field.data_ptr(), ref.data_ptr(), dirs.data_ptr(), slot.data_ptr(), cc.data_ptr(), 0)
    torch.cuda.synchronize()
    return field.cpu().numpy(), ref.cpu().numpy(), dirs.cpu().numpy(), slot.cpu().numpy().view(np.uint16), cc.cpu().numpy().view(np.uint32)


def compare_select(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1, lambda_q16=sdm.LAMBDA_Q16):
    """one device launch against the model, picture by picture; outside the CTU range the sentinels -> the model's results"""
    n = sdm.n_ctus(w, h)
    cnt = n - first if count < 0 else count
    f, rf, d, s, c = device_select(engine, w, h, tabs, sel, bits, pred, first, count)
    res = []
    for i in range(tabs[0].shape[0]):
        mf, mr, md, ms, mc = br4.select_dirs_refs4_picture(*[t[i] for t in tabs], sel, w, h, bits[i], first, None if pred is None else pred[i], lambda_q16)
        r = slice(first, first + cnt)
        same(f[i][:, r], mf, ("field", i)); same(rf[i][:, r], mr, ("ref", i)); same(d[i][r], md, ("dir", i)); same(s[i][r], ms, ("slot", i)); same(c[i][r], mc, ("cost", i))
        out = np.ones(n, bool); out[r] = False
        assert (f[i][:, out].view(np.uint16) == F_FILL).all() and (rf[i][:, out] == R_FILL).all() and (d[i][out] == D_FILL).all()
        assert (s[i][out] == S_FILL).all() and (c[i][out] == C_FILL).all()
        res.append((mf, mr, md, ms, mc))
    return res


@pytest.mark.parametrize("R,n_refs,mask", [(1, (1, 1), None), (2, (2, 1), 0b1), (4, (3, 4), 0b0110), (8, (8, 5), 0)])
@pytest.mark.parametrize("size", [(64, 64), (101, 71), (130, 66)])
def test_the_decision_equals_the_model(engine, size, R, n_refs, mask):
    """all 593 slots; R = 1, 2, 4, 8 with unequal counts per list; a full, a partial and an empty l1_valid_mask; with predictors (R = 2, 8)
    and without"""
    from hmme import api
    w, h = size
    n = sdm.n_ctus(w, h)
    pred = drm.predictors(R, n, 6001 + w + R)[None] if R in (2, 8) else None
    tabs = tuple(a[None] for a in br4.random_tables4(R, n, n, 6002 + w + R, None if pred is None else pred[0]))
    rng = np.random.default_rng(6003 + R)
    bits = drm.Bits((3, 3, 5), n_refs, (rng.integers(0, 6, size=R).tolist(), rng.integers(0, 6, size=R).tolist()), mask)
    seen_d, seen_r = set(), set()
    for sel in (api.SelectParams(256), api.SelectParams(256, min_depth=3, max_depth=3), api.SelectParams(256, cu_cost=40, pu_cost=15, min_depth=2, max_depth=2)):
        (mf, mr, md, ms, mc), = compare_select(engine, w, h, tabs, sel, [bits], pred)
        seen_d |= set(md.reshape(-1).tolist())
        seen_r |= set(mr.reshape(-1).tolist())
    assert {1, 3} <= seen_d and ((2 in seen_d) == (mask != 0)) and (w == 64 or 0xFF in seen_d), seen_d
    assert R == 1 or len(seen_r - {0xFF}) >= 2


def test_a_ctu_sub_range_and_four_pictures_with_their_own_bits(engine):
    from hmme import api
    w, h, R = 136, 72, 3
    n = sdm.n_ctus(w, h)
    pred = np.stack([drm.predictors(R, n, 6100 + i) for i in range(4)])
    bits = [drm.hm_bits(3, 3), drm.Bits((0, 0, 0), (1, 3), ([0] * 3, [0] * 3), 0b100), drm.Bits((40, 2, 3), (3, 2), ((1, 9, 2), (0, 7, 0)), 0b01),
            drm.Bits((1, 50, 0), (2, 2), ((7, 0, 0), (3, 3, 0)), 0)]
    sel = api.SelectParams(256, min_depth=2)
    for first, count in ((0, n), (1, 3), (5, 1)):
        per_pic = [br4.random_tables4(R, n, count, 6110 + i, pred[i], first) for i in range(4)]
        tabs = tuple(np.stack([p[k] for p in per_pic]) for k in range(6))
        res = compare_select(engine, w, h, tabs, sel, bits, pred, first, count)
        if count == n:   # one table recipe per picture, but also: the bits matter
            one = br4.select_dirs_refs4_picture(*[t[0] for t in tabs], sel, w, h, bits[2], 0, pred[0])
            assert not np.array_equal(one[2], res[0][2])


def test_replicated_input_gives_what_select_dirs_refs_frame_gives(engine):
    """a sel that admits only 8-aligned shapes and replicated uni fields: every 4x4 output is select_dirs_refs_frame's output of its 8x8 block"""
    from hmme import api
    w, h, R = 101, 71, 3
    n = sdm.n_ctus(w, h)
    pred = drm.predictors(R, n, 6200)
    tabs = drm.random_tables(R, n, n, 6201, pred)
    bits = drm.Bits((3, 3, 5), (3, 2), ((1, 2, 3), (2, 2, 0)), 0b10)
    dp = dir_params(api, bits)
    for kw in (dict(min_depth=2, max_depth=2, part_mask=0x07), dict(min_depth=1, max_depth=2, part_mask=0x03, cu_cost=9, pu_cost=4)):
        f64, r64, d64, s64, c64 = engine.select_dirs_refs_frame(w, h, api.SelectParams(64, **kw), dp, *tabs, pred_q=pred)
        f, r, d, s, c = engine.select_dirs_refs4_frame(w, h, api.SelectParams(256, **kw), dp, *tabs[:4], b4.replicate_lists(tabs[4]), b4.replicate_lists(tabs[5]), pred_q=pred)
        same(f, b4.replicate_lists(f64), "field"); same(r, b4.replicate_lists(r64), "ref"); same(d, p4.replicate(d64), "dir"); same(s, p4.replicate(s64), "slot")
        same(c, c64, "cost")
        assert {1, 2, 3, 0xFF} <= set(d.reshape(-1).tolist())


def test_one_table_set_per_list_gives_what_select_dirs4_frame_gives(engine):
    """R = 1 with the reference bits folded into the direction bits of hmme_select_dirs4_frame"""
    from hmme import api
    w, h = 101, 71
    n = sdm.n_ctus(w, h)
    pred = sdm.predictors(n, 6250)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = b4.random_dir_tables4(n, n, 6251, pred)
    rb = (2, 1)
    folded = api.DirParams((3 + rb[0], 3 + rb[1], 5 + rb[0] + rb[1]), (0, 0))
    dp = api.DirRefsParams((3, 3, 5), (1, 1), ((rb[0],), (rb[1],)))
    seen = set()
    for sel in (api.SelectParams(256), api.SelectParams(256, min_depth=3, max_depth=3)):
        f4, d4, s4, c4 = engine.select_dirs4_frame(w, h, sel, folded, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, pred_q=pred)
        f, r, d, s, c = engine.select_dirs_refs4_frame(w, h, sel, dp, mv_uni[:, None], cost_uni[:, None], mv_bi[:, None], cost_bi[:, None], uni_field,
                                                       np.zeros((2, n, 256), np.uint8), pred_q=pred[:, None])
        same(f, f4, "field"); same(d, d4, "dir"); same(s, s4, "slot"); same(c, c4, "cost")
        used = np.stack([(d & (1 << l)) != 0 for l in range(2)]) & (d != 0xFF)[None]
        assert (r[used] == 0).all() and (r[~used] == 0xFF).all()
        seen |= set(d.reshape(-1).tolist())
    assert {1, 2, 3, 0xFF} <= seen


def test_an_8x4_or_4x8_pu_is_never_bi_whatever_its_bi_tables_hold(engine):
    """the bi tables of slots 0..255 overwritten with costs of 0 and wild MVs, for every reference: no output byte changes"""
    from hmme import api
    w, h, R = 128, 64, 3
    lq = b4.TABLE_LAMBDA_Q16
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref = br4.random_tables4(R, 2, 2, 21, lambda_q16=lq)
    rs = sorted(b4.restricted_slots())
    cost_uni = cost_uni.copy()
    cost_uni[:, :, :, rs] //= 3                                                       # (the recipe favours bi: cheaper here, both kinds of slot are coded)
    bits = drm.Bits((0, 0, 0), (3, 3), ([0] * 3, [0] * 3))
    sel, dp = api.SelectParams(256, min_depth=3, max_depth=3), dir_params(api, bits)
    engine.set_lambda_q16(lq)
    try:
        first = engine.select_dirs_refs4_frame(w, h, sel, dp, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref)
        want = br4.select_dirs_refs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, w, h, bits, lambda_q16=lq)
        for got, model in zip(first, want):
            same(got, model, "model")
        under = np.isin(first[3], rs)
        assert under.any() and set(first[2][under].tolist()) <= {1, 2} and (first[2][~under] == 3).any()
        rng = np.random.default_rng(22)
        cost_bi, mv_bi = cost_bi.copy(), mv_bi.copy()
        cost_bi[:, :, :, rs] = 0
        mv_bi[:, :, :, rs] = rng.integers(-32768, 32768, size=mv_bi[:, :, :, rs].shape).astype(np.int16)
        second = engine.select_dirs_refs4_frame(w, h, sel, dp, mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref)
        for a, b in zip(first, second):
            same(a, b, "overwritten bi entries")
    finally:
        engine.set_lambda_q16(sdm.LAMBDA_Q16)


def test_every_tie_of_the_rule_through_the_4_form(engine):
    """every scenario of select_dirs_refs_model.tie_scenarios() on slots below and above 256"""
    from hmme import api
    w, h = 128, 64
    engine.set_lambda_q16(drm.TIE_LAMBDA_Q16)
    try:
        for bits in drm.tie_bits(drm.TIE_MASK) + drm.tie_bits(0):
            tabs, placed = br4.tie_tables4(bits)
            seen = set()
            for sel in (api.SelectParams(256), api.SelectParams(256, min_depth=3, max_depth=3)):
                (mf, mr, md, ms, mc), = compare_select(engine, w, h, tuple(a[None] for a in tabs), sel, [bits], lambda_q16=drm.TIE_LAMBDA_Q16)
                seen |= {(k, int(s)) for k in range(2) for s in ms[k].tolist()} & set(placed)
            assert seen == set(placed)                                                  # every site was coded, below and above 256
    finally:
        engine.set_lambda_q16(sdm.LAMBDA_Q16)


# ---- 4: the bi pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,bd", [((64, 64), 8), ((101, 71), 10), ((9, 9), 8)])
def test_the_bi_pass_equals_the_per_ctu_rule_and_its_siblings(engine, oracle_lib, hmo, size, bd):
    """search and refinement (SAD and Hadamard) of two searched references against the oracle's per-CTU search and refinement on the origin
    the model builds from three other references; replicated from 64 the tables are *_frame_bi_refs', with one other reference *_frame_bi4's"""
    from hmme import synth
    w, h = size
    sr, m = 4, synth.MARGIN
    n = sdm.n_ctus(w, h)
    cur, ref_a, other_a = three_planes(w, h, bd, seed=7000 + w + bd)
    _, ref_b, other_b = three_planes(w, h, bd, seed=7050 + w + bd)
    other_c = synth.make_pair(w, h, seed=7090 + w, bit_depth=bd, max_mv=2)[1]
    refs_np, others_np = [ref_a, ref_b], [other_a, other_b, other_c]
    field, rfield = p4.random_field4(w, h, 3, 7001 + w + bd)                              # indices 0..2, 0xFF and 3: the last two read reference 0
    assert w < 64 or {0, 1, 2, 3, 0xFF} <= set(rfield.reshape(-1).tolist())
    pred = np.stack([synth.random_predictors(n, seed=7002 + w + i, max_pel=8) for i in range(2)])
    center = np.stack([synth.random_predictors(n, seed=7003 + w + i, max_pel=8) for i in range(2)])
    org = br4.origin4(hmo, cur, others_np, w, h, bd, field, rfield)
    pc = mkplane(engine, cur, w, h, bd)
    prs, pos = [mkplane(engine, a, w, h, bd) for a in refs_np], [mkplane(engine, a, w, h, bd) for a in others_np]
    try:
        mv, sad = engine.search_frame_bi_refs4(pc, prs, pos, sr, field, rfield, center_q=center, pred_q=pred, fen=1)
        org_padded = np.ascontiguousarray(np.pad(org, m))
        for r in range(2):
            omv, osad = oracle_bi_search(oracle_lib, org, refs_np[r], w, h, sr, center[r], pred[r], engine.lambda_q16, 1, bd, range(n))
            same(mv[r], omv, ("search mv", size, bd, r)); same(sad[r], osad, ("search sad", size, bd, r))
        for had in (1, 0):
            qmv, cost = engine.refine_frame_bi_refs4(pc, prs, pos, sr, field, rfield, mv, center_q=center, pred_q=pred, use_hadamard=bool(had))
            for r in range(2):
                oq, oc = oracle_lib.refine_frame(org_padded, refs_np[r], (m, m), w, h, mv[r], pred[r], engine.lambda_q16, had, bd, n_threads=8)
                same(qmv[r], oq, ("refine mv", size, bd, had, r)); same(cost[r], oc, ("refine cost", size, bd, had, r))
        if n > 2:   # a CTU sub-range == the same rows
            smv, ssad = engine.search_frame_bi_refs4(pc, prs, pos, sr, field, rfield, center_q=center, pred_q=pred, fen=1, ctu_first=1, ctu_count=2)
            assert np.array_equal(smv, mv[:, 1:3]) and np.array_equal(ssad, sad[:, 1:3])
        # with a field and a reference field replicated from 64: bit for bit the 64 form
        f64 = random_field(n, 64, 7004 + w, max_pel=8)
        r64 = np.random.default_rng(7005 + w).choice(np.array([0, 1, 2, 3, 0xFF], np.uint8), size=(n, 64))
        a = engine.search_frame_bi_refs4(pc, prs, pos, sr, p4.replicate(f64), p4.replicate(r64), center_q=center, pred_q=pred, fen=1)
        b = engine.search_frame_bi_refs(pc, prs, pos, sr, f64, r64, center_q=center, pred_q=pred, fen=1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        a = engine.refine_frame_bi_refs4(pc, prs, pos, sr, p4.replicate(f64), p4.replicate(r64), b[0], center_q=center, pred_q=pred)
        b = engine.refine_frame_bi_refs(pc, prs, pos, sr, f64, r64, b[0], center_q=center, pred_q=pred)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # with one other reference: the bi4 form, whatever the indices say
        a = engine.search_frame_bi_refs4(pc, prs[:1], pos[:1], sr, field, rfield, center_q=center[:1], pred_q=pred[:1], fen=1)
        b = engine.search_frame_bi4(pc, prs[0], pos[0], sr, field, center_q=center[0], pred_q=pred[0], fen=1)
        assert np.array_equal(a[0][0], b[0]) and np.array_equal(a[1][0], b[1])
        a = engine.refine_frame_bi_refs4(pc, prs[:1], pos[:1], sr, field, rfield, b[0][None], center_q=center[:1], pred_q=pred[:1])
        b = engine.refine_frame_bi4(pc, prs[0], pos[0], sr, field, b[0], center_q=center[0], pred_q=pred[0])
        assert np.array_equal(a[0][0], b[0]) and np.array_equal(a[1][0], b[1])
    finally:
        for p in [pc] + prs + pos:
            p.close()


def test_the_refinement_at_12_bits_is_refused_and_the_search_served(engine):
    import torch
    from hmme import api
    w, h, sr, n = 100, 70, 4, 4
    dev = torch.device("cuda", 0)
    p12 = [mkplane(engine, a, w, h, 12) for a in three_planes(w, h, 12, seed=7101)]
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        field, rfield = p4.random_field4(w, h, 1, 7102)
        assert api.bipred_check(12, True) == ERR_UNSUPPORTED and api.bipred_check(12) == 0
        fp12 = api.FrameParams(sr, 1, 12, 0, n)
        d_f, d_r = torch.from_numpy(field).to(dev), torch.from_numpy(rfield).to(dev)
        d_imv = torch.zeros((1, n, 593, 2), dtype=torch.int16, device=dev)
        t_q, t_c = torch.full((1, n, 593, 2), 0x5A5A, dtype=torch.int16, device=dev), torch.full((1, n, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        hs = lambda p: (C.c_void_p * 1)(p.h)
        rc = L.hmme_refine_frame_bi_refs4_device(engine.h, p12[0].h, hs(p12[1]), 1, hs(p12[2]), 1, C.byref(fp12), d_f.data_ptr(), d_r.data_ptr(), None, None, d_imv.data_ptr(), 1,
                                                 t_q.data_ptr(), t_c.data_ptr(), None)
        assert rc == ERR_UNSUPPORTED and b"hmme_refine_frame_bi_refs4_device" in L.hmme_last_error(engine.h)
        q, c = np.full((1, n, 593, 2), 0x5A5A, np.int16), np.full((1, n, 593), 0x5A5A5A5A, np.uint32)
        rc = L.hmme_refine_frame_bi_refs4(engine.h, p12[0].h, hs(p12[1]), 1, hs(p12[2]), 1, C.byref(fp12), field.ctypes.data, rfield.ctypes.data, None, None,
                                          np.zeros((1, n, 593, 2), np.int16).ctypes.data, 1, q.ctypes.data, c.ctypes.data)
        assert rc == ERR_UNSUPPORTED and b"hmme_refine_frame_bi_refs4" in L.hmme_last_error(engine.h)
        torch.cuda.synchronize()
        assert bool((t_q == 0x5A5A).all()) and bool((t_c == 0x5A5A5A5A).all()) and (q == 0x5A5A).all() and (c == 0x5A5A5A5A).all()
        mv12, _ = engine.search_frame_bi_refs4(p12[0], [p12[1]], [p12[2]], sr, field, rfield)
        assert mv12.any()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in p12:
            p.close()


# ---- 5: one B picture with 2 + 2 references end to end ---------------------------------------------------------------------------------------
def test_a_b_picture_end_to_end(engine, oracle_lib, hmo):
    """refine_frame_multi per list -> select_refs at 256 with the lists as its pictures -> refine_frame_bi_refs4 per list -> select_dirs_refs4
    -> predict_bi_refs4 + predict_chroma_bi_refs4 -> residual at 256, every step on device buffers and against its model, at depth 3"""
    import torch
    from hmme import api, synth
    w, h = br4.E2E_SIZE
    bd, m, R = 8, synth.MARGIN, 2
    n = sdm.n_ctus(w, h)
    dev = torch.device("cuda", 0)
    lq = br4.E2E_LAMBDA_Q16
    bits = drm.hm_bits(R, R)
    cur, lists_np = br4.b_refs_scene(w, h, bd, br4.E2E_SEED)
    want = br4.chain(oracle_lib, hmo, api, cur, lists_np, w, h, bd, lq, bits)
    pus, mixed = br4.beyond_the_64_form(want["slot"], want["dirs"], want["ref"])
    assert pus >= 1 and mixed >= 1                                                      # on the model first
    sc = Scene(engine, w, h, bd, R, R, seed=8000)                                       # (its chroma planes; the luma references are the scene's)
    pc = mkplane(engine, cur, w, h, bd)
    lists = [[mkplane(engine, a, w, h, bd) for a in lst] for lst in lists_np]
    try:
        sel = br4.e2e_sel(api)
        fp = api.FrameParams(4, 1, bd, 0, n)
        zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        host = lambda t, dt=None: t.cpu().numpy() if dt is None else t.cpu().numpy().view(dt)
        d_imv = zeros((R, n, 593, 2), torch.int16)
        # 1. the uni-directional refinement of each list over its references
        d_mvu, d_cu = zeros((2, R, n, 593, 2), torch.int16), zeros((2, R, n, 593), torch.int32)
        for l in range(2):
            engine.refine_frame_multi_device(pc, lists[l], fp, None, d_imv.data_ptr(), 1, d_mvu[l].data_ptr(), d_cu[l].data_ptr(), 0)
        # 2. the reference per PU at 256, the two lists as the call's two pictures
        d_uf, d_ur = zeros((2, n, 256, 2), torch.int16), zeros((2, n, 256), torch.uint8)
        engine.select_refs_device(w, h, 2, R, fp, sel, srm.hm_ref_cost(R, lq), d_mvu.data_ptr(), d_cu.data_ptr(), None, d_uf.data_ptr(), d_ur.data_ptr(), None, None, 0)
        # 3. the bi pass of each list against the origin from the other list's field and indices
        d_mvb, d_cb = zeros((2, R, n, 593, 2), torch.int16), zeros((2, R, n, 593), torch.int32)
        for l in range(2):
            engine.refine_frame_bi_refs4_device(pc, lists[l], lists[1 - l], fp, d_uf[1 - l].data_ptr(), d_ur[1 - l].data_ptr(), None, None, d_imv.data_ptr(), 1,
                                                d_mvb[l].data_ptr(), d_cb[l].data_ptr(), 0)
        # 4. the decision
        d_field, d_ref, d_dir = zeros((1, 2, n, 256, 2), torch.int16), zeros((1, 2, n, 256), torch.uint8), zeros((1, n, 256), torch.uint8)
        d_slot, d_cc = zeros((1, n, 256), torch.int16), zeros((1, n), torch.int32)
        engine.select_dirs_refs4_device(w, h, 1, R, fp, sel, [dir_params(api, bits)], d_mvu.data_ptr(), d_cu.data_ptr(), d_mvb.data_ptr(), d_cb.data_ptr(), d_uf.data_ptr(),
                                        d_ur.data_ptr(), None, d_field.data_ptr(), d_ref.data_ptr(), d_dir.data_ptr(), d_slot.data_ptr(), d_cc.data_ptr(), 0)
        # 5. the prediction, luma and chroma
        d_y = zeros((h, w), torch.uint8)
        d_c = [zeros((h // 2, w // 2), torch.uint8) for _ in range(2)]
        engine.predict_bi_refs4_device(lists[0], lists[1], fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), d_y.data_ptr(), w)
        engine.predict_chroma_bi_refs4_device(sc.c_planes[0], sc.c_planes[1], w, h, fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), d_c[0].data_ptr(),
                                              d_c[1].data_ptr(), w // 2)
        # 6. the residual on Y
        d_res, d_pu = zeros((h, w), torch.int16), zeros((1, n, 256), torch.int32)
        d_cuo, d_ctu = zeros((1, n, 256), torch.int32), zeros((1, n, 2), torch.int32)
        engine.residual_pairs_device([pc], [d_y.data_ptr()], w, fp, d_slot.data_ptr(), 256, 1, [d_res.data_ptr()], 2 * w, d_pu.data_ptr(), d_cuo.data_ptr(), d_ctu.data_ptr(), 0)
        torch.cuda.synchronize()
        same(host(d_mvu), want["mv_uni"], "1 mv"); same(host(d_cu, np.uint32), want["cost_uni"], "1 cost")
        same(host(d_uf), want["uni_field"], "2 field"); same(host(d_ur), want["uni_ref"], "2 ref")
        same(host(d_mvb), want["mv_bi"], "3 mv"); same(host(d_cb, np.uint32), want["cost_bi"], "3 cost")
        same(host(d_field)[0], want["field"], "4 field"); same(host(d_ref)[0], want["ref"], "4 ref"); same(host(d_dir)[0], want["dirs"], "4 dir")
        same(host(d_slot, np.uint16)[0], want["slot"], "4 slot"); same(host(d_cc, np.uint32)[0], want["cost"], "4 cost")
        got = br4.beyond_the_64_form(host(d_slot, np.uint16)[0], host(d_dir)[0], host(d_ref)[0])
        assert got[0] >= 1 and got[1] >= 1                                              # ... then on the device
        pred = host(d_y)
        same(pred, br4.luma_picture(hmo, lists_np[0], lists_np[1], w, h, bd, want["field"], want["dirs"], want["ref"], np.zeros((h, w), np.int64)), "5 luma")
        same2([host(t) for t in d_c], br4.chroma_picture(hmo, sc.c_arrays, w, h, bd, want["field"], want["dirs"], want["ref"],
                                                        tuple(np.zeros((h // 2, w // 2), np.int64) for _ in range(2))), "5 chroma")
        md, mpu, mcu, mctu = rm.residual_picture(hmo, cur[m:m + h, m:m + w], pred, w, h, bd, want["slot"], 256, 1)
        same(host(d_res), md, "6 residual"); same(host(d_pu, np.uint32)[0], mpu, "6 pu"); same(host(d_cuo, np.uint32)[0], mcu, "6 cu"); same(host(d_ctu, np.uint32)[0], mctu, "6 ctu")
        assert md.any()
    finally:
        sc.close()
        for p in [pc] + [p for lst in lists for p in lst]:
            p.close()


# ---- 6: refusals: one case per layer -- the code, the entry's name, no output byte changed --------------------------------------------------
def test_refusals(engine):
    import torch
    from hmme import api
    L = api.load()
    w, h, n = 128, 64, 2
    dev = torch.device("cuda", 0)
    y = [engine.plane(w, h) for _ in range(5)]
    cc = [engine.plane(w // 2, h // 2) for _ in range(18)]
    small, c_small = engine.plane(64, 64), engine.plane(32, 32)
    odd = [engine.plane(50, 35) for _ in range(4)]                                     # the chroma of 100 x 70; asked for with 101 x 70
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        field, dirs, refs = np.zeros((2, n, 256, 2), np.int16), np.full((n, 256), 3, np.uint8), np.zeros((2, n, 256), np.uint8)
        img = np.full((h, w), 0x5C, np.uint8)
        cimg = [np.full((h // 2, w // 2), 0x5C, np.uint8) for _ in range(2)]
        couts = (C.c_void_p * 2)(cimg[0].ctypes.data, cimg[1].ctypes.data)
        hs = lambda ps: (C.c_void_p * len(ps))(*[p.h for p in ps])
        fp = api.FrameParams(4, 1, 8, 0, -1)
        fpr, F, D, R, I = C.byref(fp), field.ctypes.data, dirs.ctypes.data, refs.ctypes.data, img.ctypes.data
        bad_range = api.FrameParams(4, 1, 8, 1, 2)
        d_t = torch.full((2, 2, n, 593, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_c = torch.full((2, 2, n, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_f = torch.zeros((2, 2, n, 256, 2), dtype=torch.int16, device=dev)
        d_o = torch.full((4, n, 256, 2), 0x5A5A, dtype=torch.int16, device=dev)       # every output of the decision, one buffer (8-byte aligned)
        T, Cc, Fd, O = d_t.data_ptr(), d_c.data_ptr(), d_f.data_ptr(), d_o.data_ptr()
        t_mv, t_cost = np.full((1, n, 593, 2), 0x5A5A, np.int16), np.full((1, n, 593), 0x5A5A5A5A, np.uint32)
        sel, sel64 = api.SelectParams(256), api.SelectParams(64)
        D_ = api.DirRefsParams
        ok = D_((3, 3, 5), (2, 2), ((1, 2), (1, 2)))

        def sd(s=sel, R_=2, dirs_=ok, fpa=fpr, ref_out=O, lw=w):
            return "hmme_select_dirs_refs4_device", L.hmme_select_dirs_refs4_device(engine.h, lw, h, 1, R_, fpa, C.byref(s), C.byref(dirs_), T, Cc, T, Cc, Fd, Fd, None, O, ref_out,
                                                                                   O, O, O, None)

        def bs(o=None, fpa=fpr, rf=Fd, mv=T):
            return "hmme_search_frame_bi_refs4_device", L.hmme_search_frame_bi_refs4_device(engine.h, y[0].h, hs(y[1:3]), 2, hs(o or y[3:5]), 2, fpa, Fd, rf, None, None, mv, Cc,
                                                                                           None)

        def fs(o=None, fpa=fpr, rf=R):
            return "hmme_search_frame_bi_refs4", L.hmme_search_frame_bi_refs4(engine.h, y[0].h, hs(y[1:2]), 1, hs(o or y[3:5]), 2, fpa, F, rf, None, None, t_mv.ctypes.data,
                                                                             t_cost.ctypes.data)

        def lf(r1=None, fpa=fpr, rf=R):
            return "hmme_predict_bi_refs4_frame", L.hmme_predict_bi_refs4_frame(engine.h, hs(y[:2]), 2, hs(r1 or y[2:4]), 2, fpa, F, D, rf, I, w)

        def cf(r0=None, r1=None, n0=2, n1=2, lw=w, lh=h, fpa=fpr):
            return "hmme_predict_chroma_bi_refs4_frame", L.hmme_predict_chroma_bi_refs4_frame(engine.h, hs(r0 or cc[:4]), n0, hs(r1 or cc[4:8]), n1, lw, lh, fpa, F, D, R, couts,
                                                                                             w // 2)

        def cd(n0=2, n1=2):
            return "hmme_predict_chroma_bi_refs4_device", L.hmme_predict_chroma_bi_refs4_device(engine.h, hs(cc[:2 * n0]), n0, hs(cc[10:10 + 2 * n1]), n1, w, h, fpr, Fd, Fd, Fd, O, O,
                                                                                               w // 2, None)

        cases = [
            # hmme_select_dirs_refs4_check: R = 9, n_refs = 0, mask bits beyond n_refs[1], mv_per_ctu = 64; then a misaligned d_out_ref and the CTU range
            (sd, dict(R_=9), ERR_ARG), (sd, dict(dirs_=D_((3, 3, 5), (0, 2), ((), (1, 2)))), ERR_ARG), (sd, dict(dirs_=D_((3, 3, 5), (2, 2), ((1, 2), (1, 2)), 0b100)), ERR_ARG),
            (sd, dict(s=sel64), ERR_ARG), (sd, dict(ref_out=O + 1), ERR_ARG), (sd, dict(fpa=C.byref(bad_range)), ERR_ARG),
            # the bi pass: a NULL d_other_ref, a plane of another size, the CTU range
            (bs, dict(rf=None), ERR_ARG), (bs, dict(o=[y[3], small]), ERR_ARG), (bs, dict(fpa=C.byref(bad_range)), ERR_ARG), (bs, dict(mv=None), ERR_ARG),
            (fs, dict(rf=None), ERR_ARG), (fs, dict(o=[small, y[4]]), ERR_ARG), (fs, dict(fpa=C.byref(bad_range)), ERR_ARG),
            # the prediction: a NULL reference field, a plane of another size, the CTU range; chroma: an odd luma size, 5 + 4 references
            (lf, dict(rf=None), ERR_ARG), (lf, dict(r1=[y[2], small]), ERR_ARG), (lf, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (cf, dict(r1=cc[4:7] + [c_small]), ERR_ARG), (cf, dict(r0=odd[:2], r1=odd[2:], n0=1, n1=1, lw=101, lh=70), ERR_ARG), (cf, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (cf, dict(r0=cc[:10], n0=5, r1=cc[10:18], n1=4), ERR_ARG), (cd, dict(n0=5, n1=4), ERR_ARG),
        ]
        for call, kw, want in cases:
            name, rc = call(**kw)
            msg = L.hmme_last_error(engine.h)
            assert rc == want and name.encode() in msg, (name, sorted(kw), rc, want, msg)
        torch.cuda.synchronize()
        assert (img == 0x5C).all() and all((c == 0x5C).all() for c in cimg) and (t_mv == 0x5A5A).all() and (t_cost == 0x5A5A5A5A).all()
        assert bool((d_t == 0x5A5A).all()) and bool((d_c == 0x5A5A5A5A).all()) and bool((d_o == 0x5A5A).all())
        # the existing entries still refuse 256 MVs per CTU
        assert L.hmme_predict_bi_refs_frame(engine.h, hs(y[:2]), 2, hs(y[2:4]), 2, fpr, F, D, R, 256, I, w) == ERR_ARG
        assert api.select_dirs_refs_check(sel, 1, 2, [ok]) == ERR_ARG and (img == 0x5C).all()
        # ... and the calls that are served still are
        assert lf()[1] == 0 and cf()[1] == 0 and cd(4, 4)[1] == 0 and (img != 0x5C).any() and (cimg[0] != 0x5C).any()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in y + cc + odd + [small, c_small]:
            p.close()
