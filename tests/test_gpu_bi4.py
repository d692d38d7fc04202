"""B pictures from one MV per 4x4 block on the device (the "bi4" family of include/hmme.h: the bi pass against an origin built from a 4x4
field, the L0 / L1 / bi decision over all 593 slots, the luma and 4:2:0 prediction from its output), bit for bit against two yardsticks:
tests/bi4_model.py (pinned to the models of the 64 forms by tests/test_bi4_cpu.py) and the existing 64 forms themselves -- on replicated
fields the whole result, on 4x4 fields quadrant by quadrant.  Every output is sentinel-filled: what is not written keeps the sentinel.
Pictures are one to six CTUs."""
import ctypes as C

import numpy as np
import pytest

import bi4_model as b4
import predict4_model as p4
import residual_model as rm
import select_dirs_model as sdm
import select_model as sm
from frame_helpers import bind_hmo, check_strided_image, dims, mkplane, oracle_bi_search, random_field, three_planes

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5
F_FILL, D_FILL, S_FILL, C_FILL = 0x5A5A, 0xA7, 0x1234, 0x0BADBEEF   # sentinels the decision's outputs are preset with
ZERO_BITS = ((0, 0, 0), (0, 0))


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
    """the two references (list 0, list 1) of a w x h B picture at one depth: luma and, for even sizes, Cb and Cr -- padded arrays for the
    models, planes for the engine; all textures unrelated"""

    def __init__(self, engine, w, h, bd, seed, chroma=True):
        from hmme import synth
        self.w, self.h, self.bd = w, h, bd
        self.luma = [synth.make_pair(w, h, seed=seed + 13 * k, bit_depth=bd, max_mv=2)[1] for k in range(2)]
        self.y = [mkplane(engine, a, w, h, bd) for a in self.luma]
        self.chroma = chroma and w % 2 == 0 and h % 2 == 0 and w >= 16 and h >= 16
        self.c_arrays, self.c_planes = [], []
        if self.chroma:   # [list][component]
            self.c_arrays = [[synth.make_pair(w // 2, h // 2, seed=seed + 500 + 7 * k + 3 * c, bit_depth=bd, max_mv=2)[1] for c in range(2)] for k in range(2)]
            self.c_planes = [[mkplane(engine, a, w // 2, h // 2, bd) for a in pic] for pic in self.c_arrays]

    def comps(self):
        """model order: [component] = (list 0, list 1)"""
        return [(self.c_arrays[0][c], self.c_arrays[1][c]) for c in range(2)]

    def close(self):
        for p in self.y + [p for pic in self.c_planes for p in pic]:
            p.close()


def check_rule(engine, hmo, sc, field, dirs, ctus=None, first=0, count=-1):
    """one field through the luma call (and the chroma call) against both yardsticks -> the luma image"""
    w, h, bd = sc.w, sc.h, sc.bd
    kw = dict(ctu_first=first, ctu_count=count)
    got = engine.predict_bi4_frame(sc.y[0], sc.y[1], field, dirs, out=fill(w, h, bd), **kw)
    same(got, b4.luma_picture(hmo, sc.luma, w, h, bd, field, dirs, fill(w, h, bd, np.int64), ctus), ("model", w, h, bd))
    quads = b4.quadrant_fields(field, dirs)
    images = [engine.predict_bi_frame(sc.y[0], sc.y[1], fq, dq, out=fill(w, h, bd), **kw) for fq, dq in quads]
    same(got, p4.compose(images, w, h), ("four calls of the 64 form", w, h, bd))
    if sc.chroma:
        got_c = engine.predict_chroma_bi4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, outs=fills(w, h, bd), **kw)
        same2(got_c, b4.chroma_picture(hmo, sc.comps(), w, h, bd, field, dirs, fills(w, h, bd, np.int64), ctus), ("chroma model", w, h, bd))
        images = [engine.predict_chroma_bi_frame(sc.c_planes[0], sc.c_planes[1], w, h, fq, dq, outs=fills(w, h, bd), **kw) for fq, dq in quads]
        same2(got_c, [p4.compose([im[c] for im in images], w, h, 2) for c in range(2)], ("four chroma calls of the 64 form", w, h, bd))
    return got


# ---- 1: the prediction --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(64, 64), (101, 71), (130, 66), (16, 16)])
def test_replicated_fields_give_the_images_of_the_64_forms(engine, size, bd):
    w, h = size
    n = dims(w, h)[0] * dims(w, h)[1]
    sc = Scene(engine, w, h, bd, seed=5000 + w + bd)
    try:
        field64 = np.stack([random_field(n, 64, 5001 + l + w, max_pel=20) for l in range(2)])
        dirs64 = np.random.default_rng(5003 + w).choice(np.array([1, 2, 3, 3, 0xFF, 0], np.uint8), size=(n, 64))
        field, dirs = b4.replicate_lists(field64), p4.replicate(dirs64)
        got = engine.predict_bi4_frame(sc.y[0], sc.y[1], field, dirs, out=fill(w, h, bd))
        same(got, engine.predict_bi_frame(sc.y[0], sc.y[1], field64, dirs64, out=fill(w, h, bd)), ("luma", size, bd))
        assert (got != sentinel(bd)[1]).any()
        if sc.chroma:
            got_c = engine.predict_chroma_bi4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, outs=fills(w, h, bd))
            same2(got_c, engine.predict_chroma_bi_frame(sc.c_planes[0], sc.c_planes[1], w, h, field64, dirs64, outs=fills(w, h, bd)), ("chroma", size, bd))
            assert not np.array_equal(got_c[0], got_c[1])
    finally:
        sc.close()


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("size", [(100, 70), (9, 9), (130, 66), (64, 64), (16, 16)])
def test_the_rule_on_random_4x4_fields(engine, hmo, size, bd):
    """directions in thirds plus 0xFF and 0 entries, every phase pair in both lists, MVs at +-32767 on bi blocks: against the model AND
    against four calls of the 64 forms composed quadrant by quadrant; luma at every size, chroma at the even ones"""
    w, h = size
    if size in ((130, 66), (64, 64), (16, 16)) and bd == 12:
        bd = 9                                                                          # (the chroma sizes: a fourth depth instead of 12 twice more)
    sc = Scene(engine, w, h, bd, seed=5100 + w + bd)
    try:
        field, dirs = b4.random_field_bi4(w, h, 5101 + w + bd)
        if w >= 64:
            assert {1, 2, 3, 0, 0xFF} <= set(dirs.reshape(-1).tolist()) and int(np.abs(field.astype(np.int32)).max()) >= 32767
        if w >= 100:
            assert all(len(s) == 16 for s in b4.phase_pairs(w, h, field, dirs))
        got = check_rule(engine, hmo, sc, field, dirs)
        sv = sentinel(bd)[1]
        assert (got != sv).any() and ((got == sv).any() or w < 64)                      # dead blocks keep the sentinel
    finally:
        sc.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_quadrant_directions_in_every_rotation(engine, hmo, bd):
    """one CTU whose 8x8 blocks carry 1 / 2 / 3 / dead in their quadrants in every rotation: the four waves of an iteration see four
    different rotations, and every dead quadrant has live neighbours inside its own 8x8 block"""
    w, h = 64, 64
    sc = Scene(engine, w, h, bd, seed=5200 + bd)
    try:
        field, dirs = b4.rotation_ctu(5201 + bd)
        got = check_rule(engine, hmo, sc, field, dirs)
        dead = np.kron(~np.isin(dirs.reshape(16, 16), (1, 2, 3)), np.ones((4, 4), bool))
        assert dead.sum() == 64 * 16 and (got[dead] == sentinel(bd)[1]).all()
    finally:
        sc.close()


def test_ctu_sub_range_and_strided_image(engine, hmo):
    w, h, bd = 136, 72, 8
    sc = Scene(engine, w, h, bd, seed=5300)
    try:
        field, dirs = b4.random_field_bi4(w, h, 5301)
        sv = sentinel(bd)[1]
        for first, count in ((1, 2), (4, 1), (2, 0)):
            got = check_rule(engine, hmo, sc, field, dirs, ctus=range(first, first + count), first=first, count=count)
            assert ((got != sv).any()) == (count > 0)
        check_strided_image(w, h, bd, lambda out, first, count: engine.predict_bi4_frame(sc.y[0], sc.y[1], field, dirs, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_bi4_frame(engine.h, sc.y[0].h, sc.y[1].h, C.byref(fp), field.ctypes.data, dirs.ctypes.data, out,
                                                                                   stride))
    finally:
        sc.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_device_entries_with_eight_and_four_pictures(engine, bd):
    """the device forms on device buffers, pitches wider than a row, the most pictures a launch takes; the _frame forms are the yardstick"""
    import torch
    from hmme import api
    w, h = 100, 70
    dev = torch.device("cuda", 0)
    scenes = [Scene(engine, w, h, bd, seed=5400 + 31 * i + bd, chroma=i < 4) for i in range(8)]
    try:
        dt, sv = sentinel(bd)
        bps = 1 if bd == 8 else 2
        to_dev = lambda a: torch.from_numpy(a if a.dtype != np.uint16 else a.view(np.int16)).to(dev)
        fd = [b4.random_field_bi4(w, h, 5401 + i) for i in range(8)]
        fp = api.FrameParams(1, 0, bd, 0, -1)
        for n_pics, comps in ((8, 1), (4, 2)):
            d_field = to_dev(np.stack([f for f, _ in fd[:n_pics]]))
            d_dirs = to_dev(np.stack([d for _, d in fd[:n_pics]]))
            pw, ph = (w, h) if comps == 1 else (w // 2, h // 2)
            d_imgs = [to_dev(np.full((ph, pw + 12), sv, dt)) for _ in range(comps * n_pics)]
            torch.cuda.synchronize()
            if comps == 1:
                engine.predict_bi4_device([s.y[0] for s in scenes], [s.y[1] for s in scenes], fp, d_field.data_ptr(), d_dirs.data_ptr(), [t.data_ptr() for t in d_imgs],
                                          (pw + 12) * bps)
                want = [engine.predict_bi4_frame(s.y[0], s.y[1], f, d, out=fill(w, h, bd)) for s, (f, d) in zip(scenes, fd)]
            else:
                engine.predict_chroma_bi4_device([p for s in scenes[:4] for p in s.c_planes[0]], [p for s in scenes[:4] for p in s.c_planes[1]], w, h, fp, d_field.data_ptr(),
                                                 d_dirs.data_ptr(), [t.data_ptr() for t in d_imgs], (pw + 12) * bps)
                want = [im for s, (f, d) in zip(scenes[:4], fd) for im in engine.predict_chroma_bi4_frame(s.c_planes[0], s.c_planes[1], w, h, f, d, outs=fills(w, h, bd))]
            torch.cuda.synchronize()
            for k, (d_img, wanted) in enumerate(zip(d_imgs, want)):
                back = d_img.cpu().numpy().view(dt)
                same(back[:, :pw], wanted, ("device", n_pics, comps, k))
                assert (back[:, pw:] == sv).all() and (wanted != sv).any()
            assert not np.array_equal(want[0], want[1])
    finally:
        for s in scenes:
            s.close()


def test_a_used_context_gives_what_a_fresh_one_gives(engine):
    """the module's engine has run every call of this file (and runs a 64-form call first); a context made here has run nothing"""
    from hmme import api
    w, h, bd = 100, 70, 10
    field, dirs = b4.random_field_bi4(w, h, 5501)
    results = []
    fresh = api.Engine(0, 64)
    try:
        for e in (engine, fresh):
            sc = Scene(e, w, h, bd, seed=5500)
            try:
                if e is engine:
                    fq, dq = b4.quadrant_fields(field, dirs)[0]
                    e.predict_bi_frame(sc.y[0], sc.y[1], fq, dq)
                results.append((e.predict_bi4_frame(sc.y[0], sc.y[1], field, dirs, out=fill(w, h, bd)),
                                *e.predict_chroma_bi4_frame(sc.c_planes[0], sc.c_planes[1], w, h, field, dirs, outs=fills(w, h, bd))))
            finally:
                sc.close()
    finally:
        fresh.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b) and (a != sentinel(bd)[1]).any()


# ---- 2: the decision -----------------------------------------------------------------------------------------------------------------------
def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.copy()).to(torch.device("cuda", 0))


def device_select_dirs4(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1):
    """tabs = (mv_uni, cost_uni, mv_bi, cost_bi [n_pics, 2, count, 593, ...], uni_field [n_pics, 2, n_ctu, 256, 2]), bits = one
    (dir_bits, list_bits) per picture -> the four outputs of ONE hmme_select_dirs4_device launch over ALL CTUs (sentinels where nothing was
    written)"""
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    n_pics, n = tabs[0].shape[0], sdm.n_ctus(w, h)
    cnt = n - first if count < 0 else count
    assert tabs[0].shape == (n_pics, 2, cnt, 593, 2) and tabs[4].shape == (n_pics, 2, n, 256, 2)
    d = [to_device(a) for a in tabs]
    d_pred = to_device(pred) if pred is not None else None
    field = torch.full((n_pics, 2, n, 256, 2), F_FILL, dtype=torch.int16, device=dev)
    dirs = torch.full((n_pics, n, 256), D_FILL, dtype=torch.uint8, device=dev)
    slot = torch.full((n_pics, n, 256), S_FILL, dtype=torch.int16, device=dev)
    cc = torch.full((n_pics, n), C_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.select_dirs4_device(w, h, n_pics, api.FrameParams(1, 0, 8, first, cnt), sel, [api.DirParams(*b) for b in bits], *[t.data_ptr() for t in d],
                               d_pred.data_ptr() if d_pred is not None else None, field.data_ptr(), dirs.data_ptr(), slot.data_ptr(), cc.data_ptr(), 0)
    torch.cuda.synchronize()
    return field.cpu().numpy(), dirs.cpu().numpy(), slot.cpu().numpy().view(np.uint16), cc.cpu().numpy().view(np.uint32)


def compare_dirs4(engine, w, h, tabs, sel, bits, pred=None, first=0, count=-1, lambda_q16=sdm.LAMBDA_Q16):
    """one device launch against the model, picture by picture; outside the CTU range the sentinels -> the model's results"""
    n = sdm.n_ctus(w, h)
    cnt = n - first if count < 0 else count
    f, d, s, c = device_select_dirs4(engine, w, h, tabs, sel, bits, pred, first, count)
    res = []
    for i in range(tabs[0].shape[0]):
        mf, md, ms, mc, lv = b4.select_dirs4_picture(*[t[i] for t in tabs], sel, w, h, bits[i], first, None if pred is None else pred[i], lambda_q16)
        r = slice(first, first + cnt)
        same(f[i][:, r], mf, ("field", i)); same(d[i][r], md, ("dir", i)); same(s[i][r], ms, ("slot", i)); same(c[i][r], mc, ("cost", i))
        out = np.ones(n, bool); out[r] = False
        assert (f[i][:, out].view(np.uint16) == F_FILL).all() and (d[i][out] == D_FILL).all() and (s[i][out] == S_FILL).all() and (c[i][out] == C_FILL).all()
        res.append((mf, md, ms, mc, lv))
    return res


@pytest.mark.parametrize("with_pred", [False, True])
@pytest.mark.parametrize("size", [(64, 64), (101, 71), (65, 67)])
def test_the_decision_equals_the_model(engine, size, with_pred):
    """all 593 slots, default parameters and a priced decision; 65 x 67: a last CTU column one sample wide and a bottom row three samples
    high, where the splits are forced"""
    from hmme import api
    w, h = size
    n = sdm.n_ctus(w, h)
    pred = sdm.predictors(n, 6001 + w)[None] if with_pred else None
    tabs = tuple(a[None] for a in b4.random_dir_tables4(n, n, 6002 + w, None if pred is None else pred[0]))
    seen_d, seen_ps = set(), set()
    for sel, bits in ((api.SelectParams(256), sdm.HM_BITS), (api.SelectParams(256, cu_cost=40, pu_cost=15, min_depth=1), ZERO_BITS),
                      (api.SelectParams(256, min_depth=3, max_depth=3), ZERO_BITS), (api.SelectParams(256, min_depth=2, max_depth=2), ZERO_BITS)):
        (mf, md, ms, mc, lv), = compare_dirs4(engine, w, h, tabs, sel, [bits], pred)
        seen_d |= set(md.reshape(-1).tolist())
        seen_ps |= {ps for ctu in lv for _, ps in ctu}
    assert {1, 2, 3} <= seen_d and (w == 64 or 0xFF in seen_d)
    assert len(seen_ps) >= 4 and (w != 101 or seen_ps == {0, 1, 2, 4, 5, 6, 7}), seen_ps   # (101 x 71: every PartSize is coded somewhere)


def test_a_ctu_sub_range_and_four_pictures_with_their_own_bits(engine):
    from hmme import api
    w, h = 136, 72
    n = sdm.n_ctus(w, h)
    pred = np.stack([sdm.predictors(n, 6100 + i) for i in range(4)])
    bits = [sdm.HM_BITS, ZERO_BITS, ((40, 2, 3), (1, 9)), ((1, 50, 0), (7, 0))]
    sel = api.SelectParams(256, min_depth=2)
    for first, count in ((0, n), (1, 3), (5, 1)):
        per_pic = [b4.random_dir_tables4(n, count, 6110 + i, pred[i], first) for i in range(4)]
        tabs = tuple(np.stack([p[k] for p in per_pic]) for k in range(5))
        res = compare_dirs4(engine, w, h, tabs, sel, bits, pred, first, count)
        if count == n:   # one table recipe per picture, but also: the bits matter
            one = b4.select_dirs4_picture(*[t[0] for t in tabs], sel, w, h, bits[2], 0, pred[0])
            assert not np.array_equal(one[1], res[0][1])


def test_replicated_input_gives_what_select_dirs_frame_gives(engine):
    """a sel that admits only 8-aligned shapes and a replicated uni field: every 4x4 output is select_dirs_frame's output of its 8x8 block"""
    from hmme import api
    w, h = 101, 71
    n = sdm.n_ctus(w, h)
    pred = sdm.predictors(n, 6200)
    tabs = sdm.random_dir_tables(n, n, 6201, pred)
    dp = api.DirParams(*sdm.HM_BITS)
    for kw in (dict(min_depth=2, max_depth=2, part_mask=0x07), dict(min_depth=1, max_depth=2, part_mask=0x03, cu_cost=9, pu_cost=4)):
        f64, d64, s64, c64 = engine.select_dirs_frame(w, h, api.SelectParams(64, **kw), dp, *tabs, pred_q=pred)
        f, d, s, c = engine.select_dirs4_frame(w, h, api.SelectParams(256, **kw), dp, *tabs[:4], b4.replicate_lists(tabs[4]), pred_q=pred)
        same(f, b4.replicate_lists(f64), "field"); same(d, p4.replicate(d64), "dir"); same(s, p4.replicate(s64), "slot"); same(c, c64, "cost")
        assert {1, 2, 3, 0xFF} <= set(d.reshape(-1).tolist())


def test_an_8x4_or_4x8_pu_is_never_bi_whatever_its_bi_tables_hold(engine):
    from hmme import api
    w, h = 128, 64
    lq = b4.TABLE_LAMBDA_Q16
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = b4.random_dir_tables4(2, 2, 21, lambda_q16=lq)
    rs = sorted(b4.restricted_slots())
    cost_bi, mv_bi = cost_bi.copy(), mv_bi.copy()
    cost_bi[:, :, rs] = 0
    sel, dp = api.SelectParams(256, min_depth=3, max_depth=3), api.DirParams(*ZERO_BITS)
    engine.set_lambda_q16(lq)
    try:
        first = engine.select_dirs4_frame(w, h, sel, dp, mv_uni, cost_uni, mv_bi, cost_bi, uni_field)
        want = b4.select_dirs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, w, h, ZERO_BITS, lambda_q16=lq)
        for got, model in zip(first, want[:4]):
            same(got, model, "model")
        under = np.isin(first[2], rs)
        assert under.any() and set(first[1][under].tolist()) == {1, 2} and (first[1][~under] == 3).any()
        rng = np.random.default_rng(22)
        cost_bi[:, :, rs] = rng.integers(0, 1 << 32, size=cost_bi[:, :, rs].shape, dtype=np.uint64).astype(np.uint32)
        mv_bi[:, :, rs] = rng.integers(-32768, 32768, size=mv_bi[:, :, rs].shape).astype(np.int16)
        second = engine.select_dirs4_frame(w, h, sel, dp, mv_uni, cost_uni, mv_bi, cost_bi, uni_field)
        for a, b in zip(first, second):
            same(a, b, "refilled bi entries")
    finally:
        engine.set_lambda_q16(sdm.LAMBDA_Q16)


def test_every_tie_of_the_rule_through_the_4_form(engine):
    from hmme import api
    w, h = 192, 128
    n = sdm.n_ctus(w, h)
    bits = ((3, 1, 4), (1, 5))
    pred = sdm.predictors(n, 6400)
    ties, pat = sdm.tie_tables(n, 6401, bits, pred)
    tabs = tuple(a[None] for a in ties[:4]) + (np.random.default_rng(6402).integers(-300, 301, size=(1, 2, n, 256, 2)).astype(np.int16),)
    engine.set_lambda_q16(1 << 16)
    try:
        seen = set()
        for sel in (api.SelectParams(256, min_depth=2), api.SelectParams(256, min_depth=3, max_depth=3)):
            (mf, md, ms, mc, lv), = compare_dirs4(engine, w, h, tabs, sel, [bits], pred[None], lambda_q16=1 << 16)
            seen |= {int(pat[k, s]) for k in range(n) for s in set(ms[k].tolist()) if s != sm.NO_SLOT}
        assert len(seen) == len(sdm.TIE_PATTERNS), len(seen)                            # every pattern's slot was coded somewhere
    finally:
        engine.set_lambda_q16(sdm.LAMBDA_Q16)


# ---- 3: the bi pass ------------------------------------------------------------------------------------------------------------------------
def origin4(hmo, cur, other, w, h, bd, field):
    from hmme import synth
    m = synth.MARGIN
    p = b4.origin_prediction(hmo, other, w, h, bd, field)
    return np.ascontiguousarray((2 * cur[m:m + p.shape[0], m:m + p.shape[1]].astype(np.int64) - p).astype(np.int16))


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(64, 64), (100, 70)])
def test_the_bi_pass_equals_the_per_ctu_rule_on_the_origin(engine, oracle_lib, hmo, size, bd):
    """search and refinement (SAD and Hadamard) against the oracle's per-CTU search and refinement on the origin the model builds: every 4x4
    block of every CTU block, beyond the picture edge too, from the other list at its own clamped entry"""
    from hmme import synth
    w, h = size
    sr, m = 4, synth.MARGIN
    n = sdm.n_ctus(w, h)
    cur, ref, other = three_planes(w, h, bd, seed=7000 + w + bd)
    field = p4.random_field4(w, h, 1, 7001 + w + bd)[0]
    pred = synth.random_predictors(n, seed=7002 + w, max_pel=8)
    center = synth.random_predictors(n, seed=7003 + w, max_pel=8)
    org = origin4(hmo, cur, other, w, h, bd, field)
    pc, pr, po = (mkplane(engine, a, w, h, bd) for a in (cur, ref, other))
    try:
        mv, sad = engine.search_frame_bi4(pc, pr, po, sr, field, center_q=center, pred_q=pred, fen=1)
        omv, osad = oracle_bi_search(oracle_lib, org, ref, w, h, sr, center, pred, engine.lambda_q16, 1, bd, range(n))
        same(mv, omv, ("search mv", size, bd)); same(sad, osad, ("search sad", size, bd))
        org_padded = np.ascontiguousarray(np.pad(org, m))
        for had in (1, 0):
            qmv, cost = engine.refine_frame_bi4(pc, pr, po, sr, field, mv, center_q=center, pred_q=pred, use_hadamard=bool(had))
            oq, oc = oracle_lib.refine_frame(org_padded, ref, (m, m), w, h, mv, pred, engine.lambda_q16, had, bd, n_threads=8)
            same(qmv, oq, ("refine mv", size, bd, had)); same(cost, oc, ("refine cost", size, bd, had))
        # a CTU sub-range == the same rows
        if n > 1:
            smv, ssad = engine.search_frame_bi4(pc, pr, po, sr, field, center_q=center, pred_q=pred, fen=1, ctu_first=1, ctu_count=2)
            sq, sc = engine.refine_frame_bi4(pc, pr, po, sr, field, smv, center_q=center, pred_q=pred, ctu_first=1, ctu_count=2)
            q1, c1 = engine.refine_frame_bi4(pc, pr, po, sr, field, mv, center_q=center, pred_q=pred)
            assert np.array_equal(smv, mv[1:3]) and np.array_equal(ssad, sad[1:3]) and np.array_equal(sq, q1[1:3]) and np.array_equal(sc, c1[1:3])
        # with a replicated field: bit for bit the 64 form
        f64 = random_field(n, 64, 7004 + w, max_pel=8)
        a = engine.search_frame_bi4(pc, pr, po, sr, p4.replicate(f64), center_q=center, pred_q=pred, fen=1)
        b = engine.search_frame_bi(pc, pr, po, sr, f64, center_q=center, pred_q=pred, fen=1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        a = engine.refine_frame_bi4(pc, pr, po, sr, p4.replicate(f64), b[0], center_q=center, pred_q=pred)
        b = engine.refine_frame_bi(pc, pr, po, sr, f64, b[0], center_q=center, pred_q=pred)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not np.array_equal(a[0], qmv)                                            # (and the field matters)
    finally:
        pc.close(); pr.close(); po.close()


def test_the_bi_pass_device_entries_with_two_pairs_and_the_12_bit_refusal(engine):
    import torch
    from hmme import api, synth
    w, h, sr, bd = 100, 70, 4, 8
    n = sdm.n_ctus(w, h)
    dev = torch.device("cuda", 0)
    cur, r0, r1 = three_planes(w, h, bd, seed=7100)
    planes = [mkplane(engine, a, w, h, bd) for a in (cur, r0, r1)]
    pc, p0, p1 = planes
    cur12 = three_planes(w, h, 12, seed=7101)
    p12 = [mkplane(engine, a, w, h, 12) for a in cur12]
    try:
        fields = np.stack([p4.random_field4(w, h, 1, 7102 + i)[0] for i in range(2)])
        pred = np.stack([synth.random_predictors(n, seed=7110 + i, max_pel=6) for i in range(2)])
        center = np.stack([synth.random_predictors(n, seed=7120 + i, max_pel=6) for i in range(2)])
        curs, refs, others = [pc, pc], [p0, p1], [p1, p0]                               # the two directions of one B picture
        d_f, d_pred, d_center = (torch.from_numpy(a).to(dev) for a in (fields, pred, center))
        tables = lambda k, c: (torch.full((k, c, 593, 2), 0x5A5A, dtype=torch.int16, device=dev), torch.full((k, c, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev))
        for first, count in ((0, n), (1, 2)):
            fp = api.FrameParams(sr, 1, bd, first, count)
            d_mv, d_sad = tables(2, count)
            engine.search_pairs_bi4_device(curs, refs, others, fp, d_f.data_ptr(), d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
            d_q, d_c = tables(2, count)
            engine.refine_pairs_bi4_device(curs, refs, others, fp, d_f.data_ptr(), d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
            torch.cuda.synchronize()
            for i in range(2):
                smv, ssad = engine.search_frame_bi4(curs[i], refs[i], others[i], sr, fields[i], center_q=center[i], pred_q=pred[i], fen=1, ctu_first=first, ctu_count=count)
                sq, sc = engine.refine_frame_bi4(curs[i], refs[i], others[i], sr, fields[i], smv, center_q=center[i], pred_q=pred[i], ctu_first=first, ctu_count=count)
                assert np.array_equal(d_mv[i].cpu().numpy(), smv) and np.array_equal(d_sad[i].cpu().numpy().view(np.uint32), ssad), (first, i)
                assert np.array_equal(d_q[i].cpu().numpy(), sq) and np.array_equal(d_c[i].cpu().numpy().view(np.uint32), sc), (first, i)
        # the refinement at 12 bits fails hmme_bipred_check: refused, nothing written; the search at 12 bits is served
        assert api.bipred_check(12, True) == ERR_UNSUPPORTED and api.bipred_check(12) == 0
        t_q, t_c = tables(1, n)
        fp12 = api.FrameParams(sr, 1, 12, 0, n)
        L = api.load()
        prev = L.hmme_set_error_printing(engine.h, 0)
        try:
            hs = lambda p: (C.c_void_p * 1)(p.h)
            rc = L.hmme_refine_pairs_bi4_device(engine.h, hs(p12[0]), hs(p12[1]), hs(p12[2]), 1, C.byref(fp12), d_f.data_ptr(), None, None, d_mv.data_ptr(), 1,
                                                t_q.data_ptr(), t_c.data_ptr(), None)
            assert rc == ERR_UNSUPPORTED and b"hmme_refine_pairs_bi4_device" in L.hmme_last_error(engine.h)
            q, c = np.full((n, 593, 2), 0x5A5A, np.int16), np.full((n, 593), 0x5A5A5A5A, np.uint32)
            rc = L.hmme_refine_frame_bi4(engine.h, p12[0].h, p12[1].h, p12[2].h, C.byref(fp12), fields[0].ctypes.data, None, None, np.zeros((n, 593, 2), np.int16).ctypes.data, 1,
                                         q.ctypes.data, c.ctypes.data)
            assert rc == ERR_UNSUPPORTED and b"hmme_refine_frame_bi4" in L.hmme_last_error(engine.h)
            torch.cuda.synchronize()
            assert bool((t_q == 0x5A5A).all()) and bool((t_c == 0x5A5A5A5A).all()) and (q == 0x5A5A).all() and (c == 0x5A5A5A5A).all()
        finally:
            L.hmme_set_error_printing(engine.h, prev)
        mv12, _ = engine.search_frame_bi4(p12[0], p12[1], p12[2], sr, fields[0])
        assert mv12.any()
    finally:
        for p in planes + p12:
            p.close()


# ---- 4: one B picture end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 2])
def test_a_b_picture_end_to_end(engine, oracle_lib, hmo, depth):
    """refine of both lists -> select_pairs at 256 per list -> refine_pairs_bi4 per list -> select_dirs4 -> predict_bi4 + predict_chroma_bi4
    -> residual at 256, every step on device buffers and against its model.  Depth 3 forces 8x8 CUs (8x4 / 4x8 PUs, never bi), depth 2
    16x16 CUs with AMP (bi PUs of 16x4 / 16x12 / 4x16 / 12x16); tests/test_bi4_cpu.py shows that this picture chooses them"""
    import torch
    from hmme import api, synth
    w, h = b4.E2E_SIZE
    bd, m, n = 8, synth.MARGIN, 2
    dev = torch.device("cuda", 0)
    lq = sdm.LAMBDA_Q16
    cur, r0, r1 = b4.b_scene(w, h, bd, b4.E2E_SEED)
    want = b4.chain(oracle_lib, hmo, api, cur, (r0, r1), w, h, bd, depth, lq)
    cov = b4.coverage(depth, want["slot"], want["dirs"], want["field"], want["leaves"])
    if depth == 3:
        assert {1, 2} <= cov["sizes"] and all(set(cov["dirs_by_ps"][ps]) <= {1, 2} for ps in (1, 2))
    else:
        assert all(3 in cov["dirs_by_ps"].get(ps, []) for ps in (4, 5, 6, 7))
    assert cov["mixed"] >= 20
    sc = Scene(engine, w, h, bd, seed=8000)                                             # (its chroma planes; the luma references are the scene's)
    pc, p0, p1 = (mkplane(engine, a, w, h, bd) for a in (cur, r0, r1))
    try:
        sel = b4.e2e_sel(api, depth)
        fp = api.FrameParams(4, 1, bd, 0, n)
        zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        host = lambda t, dt=None: t.cpu().numpy() if dt is None else t.cpu().numpy().view(dt)
        d_imv = zeros((2, n, 593, 2), torch.int16)
        # 1. the uni-directional refinement of both lists, pairs ordered (picture, list)
        d_mvu, d_cu = zeros((2, n, 593, 2), torch.int16), zeros((2, n, 593), torch.int32)
        engine.refine_pairs_device([pc, pc], [p0, p1], fp, None, d_imv.data_ptr(), 1, d_mvu.data_ptr(), d_cu.data_ptr(), 0)
        # 2. each list's own decision at 256: the lists' fields
        d_uf, d_us = zeros((2, n, 256, 2), torch.int16), zeros((2, n, 256), torch.int16)
        engine.select_pairs_device(w, h, 2, fp, sel, d_mvu.data_ptr(), d_cu.data_ptr(), None, d_uf.data_ptr(), d_us.data_ptr(), None, 0)
        # 3. the bi pass of each list against the origin from the other list's field
        d_other = torch.stack([d_uf[1], d_uf[0]]).contiguous()
        d_mvb, d_cb = zeros((2, n, 593, 2), torch.int16), zeros((2, n, 593), torch.int32)
        engine.refine_pairs_bi4_device([pc, pc], [p0, p1], [p1, p0], fp, d_other.data_ptr(), None, None, d_imv.data_ptr(), 1, d_mvb.data_ptr(), d_cb.data_ptr(), 0)
        # 4. the decision
        d_field, d_dir = zeros((1, 2, n, 256, 2), torch.int16), zeros((1, n, 256), torch.uint8)
        d_slot, d_cc = zeros((1, n, 256), torch.int16), zeros((1, n), torch.int32)
        engine.select_dirs4_device(w, h, 1, fp, sel, [api.DirParams(*b4.E2E_BITS)], d_mvu.data_ptr(), d_cu.data_ptr(), d_mvb.data_ptr(), d_cb.data_ptr(), d_uf.data_ptr(),
                                   None, d_field.data_ptr(), d_dir.data_ptr(), d_slot.data_ptr(), d_cc.data_ptr(), 0)
        # 5. the prediction, luma and chroma
        d_y = zeros((h, w), torch.uint8)
        d_c = [zeros((h // 2, w // 2), torch.uint8) for _ in range(2)]
        engine.predict_bi4_device([p0], [p1], fp, d_field.data_ptr(), d_dir.data_ptr(), [d_y.data_ptr()], w)
        engine.predict_chroma_bi4_device(sc.c_planes[0], sc.c_planes[1], w, h, fp, d_field.data_ptr(), d_dir.data_ptr(), [t.data_ptr() for t in d_c], w // 2)
        # 6. the residual on Y
        d_res, d_pu = zeros((h, w), torch.int16), zeros((1, n, 256), torch.int32)
        d_cuo, d_ctu = zeros((1, n, 256), torch.int32), zeros((1, n, 2), torch.int32)
        engine.residual_pairs_device([pc], [d_y.data_ptr()], w, fp, d_slot.data_ptr(), 256, 1, [d_res.data_ptr()], 2 * w, d_pu.data_ptr(), d_cuo.data_ptr(), d_ctu.data_ptr(), 0)
        torch.cuda.synchronize()
        same(host(d_mvu), want["mv_uni"], "1 mv"); same(host(d_cu, np.uint32), want["cost_uni"], "1 cost")
        same(host(d_uf), want["uni_field"], "2 field"); same(host(d_us, np.uint16), np.stack(want["uni_slot"]), "2 slot")
        same(host(d_mvb), want["mv_bi"], "3 mv"); same(host(d_cb, np.uint32), want["cost_bi"], "3 cost")
        same(host(d_field)[0], want["field"], "4 field"); same(host(d_dir)[0], want["dirs"], "4 dir")
        same(host(d_slot, np.uint16)[0], want["slot"], "4 slot"); same(host(d_cc, np.uint32)[0], want["cost"], "4 cost")
        pred = host(d_y)
        same(pred, b4.luma_picture(hmo, (r0, r1), w, h, bd, want["field"], want["dirs"], np.zeros((h, w), np.int64)), "5 luma")
        same2([host(t) for t in d_c], b4.chroma_picture(hmo, sc.comps(), w, h, bd, want["field"], want["dirs"], tuple(np.zeros((h // 2, w // 2), np.int64) for _ in range(2))),
              "5 chroma")
        md, mpu, mcu, mctu = rm.residual_picture(hmo, cur[m:m + h, m:m + w], pred, w, h, bd, want["slot"], 256, 1)
        same(host(d_res), md, "6 residual"); same(host(d_pu, np.uint32)[0], mpu, "6 pu"); same(host(d_cuo, np.uint32)[0], mcu, "6 cu"); same(host(d_ctu, np.uint32)[0], mctu, "6 ctu")
        assert md.any()
    finally:
        sc.close()
        for p in (pc, p0, p1):
            p.close()


# ---- 5: refusals: one case per layer of each entry's checks -- the code, the entry's name, no output byte changed --------------------------
def test_refusals(engine):
    import torch
    from hmme import api
    L = api.load()
    w, h, n = 128, 64, 2
    dev = torch.device("cuda", 0)
    other = api.Engine(0, 64)
    y = [engine.plane(w, h) for _ in range(3)]
    cc = [engine.plane(w // 2, h // 2) for _ in range(4)]
    small, deep, foreign = engine.plane(64, 64), engine.plane(w, h, 10), other.plane(w, h)
    c_small, c_foreign = engine.plane(32, 32), other.plane(w // 2, h // 2)
    odd = [engine.plane(50, 35) for _ in range(4)]                                     # the chroma of 100 x 70; asked for with 101 x 70
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        field, dirs = np.zeros((2, n, 256, 2), np.int16), np.full((n, 256), 3, np.uint8)
        img = np.full((h, w), 0x5C, np.uint8)
        cimg = [np.full((h // 2, w // 2), 0x5C, np.uint8) for _ in range(2)]
        couts = (C.c_void_p * 2)(cimg[0].ctypes.data, cimg[1].ctypes.data)
        hs = lambda ps: (C.c_void_p * len(ps))(*[p.h for p in ps])
        fp = api.FrameParams(4, 1, 8, 0, -1)
        fpr, F, R, I = C.byref(fp), field.ctypes.data, dirs.ctypes.data, img.ctypes.data
        bad_range, deep_fp = api.FrameParams(4, 1, 8, 1, 2), api.FrameParams(4, 1, 13, 0, -1)
        d_t = torch.full((2, n, 593, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_c = torch.full((2, n, 593), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_f = torch.zeros((2, 2, n, 256, 2), dtype=torch.int16, device=dev)
        d_o = torch.full((4, n, 256, 2), 0x5A5A, dtype=torch.int16, device=dev)       # every output of the decision, one buffer (8-byte aligned)
        T, Cc, Fd, O = d_t.data_ptr(), d_c.data_ptr(), d_f.data_ptr(), d_o.data_ptr()
        imv = np.zeros((n, 593, 2), np.int16)
        t_mv, t_cost = np.full((n, 593, 2), 0x5A5A, np.int16), np.full((n, 593), 0x5A5A5A5A, np.uint32)
        sel, sel64, dp = api.SelectParams(256), api.SelectParams(64), api.DirParams(*sdm.HM_BITS)
        big = api.DirParams((4097, 0, 0), (0, 0))

        def lf(r0=None, r1=None, fpa=fpr, f=F, d=R, out=I, stride=w):
            return "hmme_predict_bi4_frame", L.hmme_predict_bi4_frame(engine.h, (r0 or y[0]).h, (r1 or y[1]).h, fpa, f, d, out, stride)

        def ld(r0=None, r1=None, n_pics=1, fpa=fpr, f=Fd, d=Fd, outs=None, pitch=w):
            return "hmme_predict_bi4_device", L.hmme_predict_bi4_device(engine.h, hs(r0 or [y[0]]), hs(r1 or [y[1]]), n_pics, fpa, f, d, outs or (C.c_void_p * 1)(O), pitch, None)

        def cf(r0=None, r1=None, lw=w, lh=h, fpa=fpr, f=F, d=R, outs=couts, stride=w // 2):
            return "hmme_predict_chroma_bi4_frame", L.hmme_predict_chroma_bi4_frame(engine.h, hs(r0 or cc[:2]), hs(r1 or cc[2:]), lw, lh, fpa, f, d, outs, stride)

        def cd(r0=None, r1=None, n_pics=1, lw=w, lh=h, fpa=fpr, f=Fd, d=Fd, outs=None, pitch=w // 2):
            return "hmme_predict_chroma_bi4_device", L.hmme_predict_chroma_bi4_device(engine.h, hs(r0 or cc[:2]), hs(r1 or cc[2:]), n_pics, lw, lh, fpa, f, d,
                                                                                      outs or (C.c_void_p * 2)(O, O), pitch, None)

        def sd(s=sel, n_pics=1, dirs_=dp, fpa=fpr, mv=T, field_out=O, dir_out=O, uni=Fd, lw=w):
            return "hmme_select_dirs4_device", L.hmme_select_dirs4_device(engine.h, lw, h, n_pics, fpa, C.byref(s), C.byref(dirs_) if dirs_ is not None else None, mv, Cc, T, Cc,
                                                                          uni, None, field_out, dir_out, O, O, None)

        def sf(s=sel, dirs_=dp, fpa=fpr, mv=None, field_out=None):
            a = np.zeros((2, n, 593, 2), np.int16), np.zeros((2, n, 593), np.uint32)
            return "hmme_select_dirs4_frame", L.hmme_select_dirs4_frame(engine.h, w, h, fpa, C.byref(s), C.byref(dirs_) if dirs_ is not None else None,
                                                                        a[0].ctypes.data if mv is None else mv, a[1].ctypes.data, a[0].ctypes.data, a[1].ctypes.data, F, None,
                                                                        t_mv.ctypes.data if field_out is None else field_out, t_cost.ctypes.data, None, None)

        def bs(curs=None, refs=None, others=None, k=1, fpa=fpr, f=Fd, mv=T, sad=Cc):
            return "hmme_search_pairs_bi4_device", L.hmme_search_pairs_bi4_device(engine.h, hs(curs or [y[0]]), hs(refs or [y[1]]), hs(others or [y[2]]), k, fpa, f, None, None,
                                                                                  mv, sad, None)

        def br(curs=None, refs=None, others=None, k=1, fpa=fpr, f=Fd, im=Fd, had=1, mv=T, cost=Cc):
            return "hmme_refine_pairs_bi4_device", L.hmme_refine_pairs_bi4_device(engine.h, hs(curs or [y[0]]), hs(refs or [y[1]]), hs(others or [y[2]]), k, fpa, f, None, None,
                                                                                  im, had, mv, cost, None)

        def fs(o=None, fpa=fpr, f=F, mv=None):
            return "hmme_search_frame_bi4", L.hmme_search_frame_bi4(engine.h, y[0].h, y[1].h, (o or y[2]).h, fpa, f, None, None, t_mv.ctypes.data if mv is None else mv,
                                                                    t_cost.ctypes.data)

        def fr(o=None, fpa=fpr, f=F, im=None):
            return "hmme_refine_frame_bi4", L.hmme_refine_frame_bi4(engine.h, y[0].h, y[1].h, (o or y[2]).h, fpa, f, None, None, imv.ctypes.data if im is None else im, 1,
                                                                    t_mv.ctypes.data, t_cost.ctypes.data)

        cases = [
            # prediction: a bit depth outside 8..12, a NULL field / direction field / image, a pitch below a row, a plane of another size, depth
            # or context, too many pictures, a CTU range outside the picture, an odd luma size
            (lf, dict(fpa=C.byref(deep_fp)), ERR_ARG), (lf, dict(f=None), ERR_ARG), (lf, dict(d=None), ERR_ARG), (lf, dict(out=None), ERR_ARG), (lf, dict(stride=w - 1), ERR_ARG),
            (lf, dict(r1=small), ERR_ARG), (lf, dict(r1=deep), ERR_ARG), (lf, dict(r0=foreign), ERR_ARG), (lf, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (ld, dict(f=None), ERR_ARG), (ld, dict(d=None), ERR_ARG), (ld, dict(pitch=w - 1), ERR_ARG), (ld, dict(n_pics=0), ERR_ARG), (ld, dict(n_pics=9), ERR_ARG),
            (ld, dict(r1=[small]), ERR_ARG), (ld, dict(r1=[foreign]), ERR_ARG), (ld, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (cf, dict(f=None), ERR_ARG), (cf, dict(outs=None), ERR_ARG), (cf, dict(stride=w // 2 - 1), ERR_ARG), (cf, dict(r1=[cc[2], c_small]), ERR_ARG),
            (cf, dict(r0=[c_foreign, cc[1]]), ERR_ARG), (cf, dict(r0=odd[:2], r1=odd[2:], lw=101, lh=70), ERR_ARG), (cf, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (cd, dict(d=None), ERR_ARG), (cd, dict(n_pics=5), ERR_ARG), (cd, dict(pitch=w // 2 - 1), ERR_ARG), (cd, dict(r1=[cc[2], c_small]), ERR_ARG),
            (cd, dict(r0=odd[:2], r1=odd[2:], lw=101, lh=70), ERR_ARG), (cd, dict(fpa=C.byref(bad_range)), ERR_ARG),
            # decision: the check function's refusals, a NULL or misaligned buffer, a CTU range outside the picture
            (sd, dict(s=sel64), ERR_ARG), (sd, dict(s=api.SelectParams(256, price_mv=1)), ERR_ARG), (sd, dict(n_pics=5), ERR_ARG), (sd, dict(dirs_=None), ERR_ARG),
            (sd, dict(dirs_=big), ERR_ARG), (sd, dict(mv=None), ERR_ARG), (sd, dict(uni=None), ERR_ARG), (sd, dict(dir_out=None), ERR_ARG), (sd, dict(field_out=O + 4), ERR_ARG),
            (sd, dict(dir_out=O + 1), ERR_ARG), (sd, dict(mv=T + 2), ERR_ARG), (sd, dict(fpa=C.byref(bad_range)), ERR_ARG), (sd, dict(lw=0), ERR_ARG),
            (sf, dict(s=sel64), ERR_ARG), (sf, dict(dirs_=big), ERR_ARG), (sf, dict(fpa=C.byref(bad_range)), ERR_ARG),
            # bi pass: hmme_bipred_check, pair counts, a NULL field, the other list's plane of another size / depth / context, NULL outputs
            (bs, dict(fpa=C.byref(deep_fp)), ERR_ARG), (bs, dict(k=0), ERR_ARG), (bs, dict(curs=[y[0]] * 17, refs=[y[1]] * 17, others=[y[2]] * 17, k=17), ERR_ARG),
            (bs, dict(f=None), ERR_ARG), (bs, dict(others=[small]), ERR_ARG), (bs, dict(others=[deep]), ERR_ARG), (bs, dict(others=[foreign]), ERR_ARG), (bs, dict(mv=None), ERR_ARG),
            (bs, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (br, dict(fpa=C.byref(api.FrameParams(4, 1, 12, 0, -1))), ERR_UNSUPPORTED), (br, dict(f=None), ERR_ARG), (br, dict(others=[small]), ERR_ARG), (br, dict(im=None), ERR_ARG),
            (br, dict(cost=None), ERR_ARG), (br, dict(others=[foreign]), ERR_ARG),
            (fs, dict(f=None), ERR_ARG), (fs, dict(o=small), ERR_ARG), (fs, dict(o=foreign), ERR_ARG), (fs, dict(fpa=C.byref(bad_range)), ERR_ARG),
            (fr, dict(f=None), ERR_ARG), (fr, dict(o=deep), ERR_ARG), (fr, dict(fpa=C.byref(api.FrameParams(4, 1, 12, 0, -1))), ERR_UNSUPPORTED),
        ]
        for call, kw, want in cases:
            name, rc = call(**kw)
            msg = L.hmme_last_error(engine.h)
            assert rc == want and name.encode() in msg, (name, sorted(kw), rc, want, msg)
        torch.cuda.synchronize()
        assert (img == 0x5C).all() and all((c == 0x5C).all() for c in cimg) and (t_mv == 0x5A5A).all() and (t_cost == 0x5A5A5A5A).all()
        assert bool((d_t == 0x5A5A).all()) and bool((d_c == 0x5A5A5A5A).all()) and bool((d_o == 0x5A5A).all())
        # the existing entries still refuse 256 MVs per CTU, and the new ones have no way to ask for 64
        assert L.hmme_predict_bi_frame(engine.h, y[0].h, y[1].h, fpr, F, R, 256, I, w) == ERR_ARG
        assert L.hmme_search_frame_bi(engine.h, y[0].h, y[1].h, y[2].h, fpr, F, 256, None, None, t_mv.ctypes.data, t_cost.ctypes.data) == ERR_ARG
        assert (img == 0x5C).all() and (t_mv == 0x5A5A).all()
        # ... and the calls that are served still are
        assert lf()[1] == 0 and cf()[1] == 0 and (img != 0x5C).any() and (cimg[0] != 0x5C).any()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in y + cc + odd + [small, deep, foreign, c_small, c_foreign]:
            p.close()
        other.close()
