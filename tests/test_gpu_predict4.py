"""Prediction from one MV per 4x4 block (hmme_predict_refs4_* / hmme_predict_chroma_refs4_*, device and _frame forms) against the rule in
include/hmme.h, with two independent yardsticks: tests/predict4_model.py (numpy, pinned to the models of the 64 forms by
tests/test_predict4_cpu.py) and the existing 64 forms themselves -- bit for bit on replicated fields, and quadrant by quadrant on 4x4 fields
(four calls on the fields F_q, quadrant q taken from image q).  Every image is sentinel-filled: what is not written keeps the sentinel.
Pictures are one to six CTUs."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
import predict4_model as p4
import predict_bi_w_model as pbw
import residual_model as rm
import select_refs_model as srm
from frame_helpers import bind_hmo, check_strided_image, clip_mv, dims, mkplane, random_field

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = pbw.ERR_ARG, pbw.ERR_UNSUPPORTED
IDENT = bwm.IDENT


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
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


class Scene:
    """n reference pictures of a w x h picture at one depth: luma, and (even sizes) Cb and Cr, as padded arrays for the models and as planes
    for the engine; all textures unrelated"""

    def __init__(self, engine, w, h, bd, seed, n, chroma=True):
        from hmme import synth
        self.w, self.h, self.bd, self.n = w, h, bd, n
        self.luma = [synth.make_pair(w, h, seed=seed + 13 * k, bit_depth=bd, max_mv=2)[1] for k in range(n)]
        self.y = [mkplane(engine, a, w, h, bd) for a in self.luma]
        self.chroma = chroma and w % 2 == 0 and h % 2 == 0
        self.c_arrays, self.c_planes = [], []
        if self.chroma:
            self.c_arrays = [[synth.make_pair(w // 2, h // 2, seed=seed + 500 + 7 * k + 3 * c, bit_depth=bd, max_mv=2)[1] for c in range(2)] for k in range(n)]
            self.c_planes = [[mkplane(engine, a, w // 2, h // 2, bd) for a in pic] for pic in self.c_arrays]

    def comps(self):
        """model order: [component][reference]"""
        return [[self.c_arrays[k][c] for k in range(self.n)] for c in range(2)]

    def flat(self):
        """engine order: [cb, cr] of each reference in turn"""
        return [p for pic in self.c_planes for p in pic]

    def close(self):
        for p in self.y + self.flat():
            p.close()


def flat_weights(wps):
    """model order [component][reference] -> engine order"""
    return [wps[c][r] for r in range(len(wps[0])) for c in range(2)]


def same(got, want, what):
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])


def same2(got, want, what):
    for c in range(2):
        same(got[c], want[c], (what, "Cb" if c == 0 else "Cr"))


def check_rule(engine, hmo, sc, field, ref, wps=None, cwps=None, chroma=True):
    """one field through the luma call (and the chroma call) against both yardsticks -> the luma image"""
    w, h, bd = sc.w, sc.h, sc.bd
    got = engine.predict_refs4_frame(sc.y, field, ref, out=fill(w, h, bd), weights=wps)
    same(got, p4.luma_picture(hmo, sc.luma, w, h, bd, field, ref, fill(w, h, bd, np.int64), wps), ("model", w, h, bd))
    quads = p4.quadrant_fields(field, ref)
    if wps is None:
        images = [engine.predict_refs_frame(sc.y, fq, rq, out=fill(w, h, bd)) for fq, rq in quads]
    else:
        images = [engine.predict_refs_w_frame(sc.y, wps, fq, rq, out=fill(w, h, bd)) for fq, rq in quads]
    same(got, p4.compose(images, w, h), ("four calls of the 64 form", w, h, bd))
    if chroma and sc.chroma:
        fw = None if cwps is None else flat_weights(cwps)
        got_c = engine.predict_chroma_refs4_frame(sc.flat(), w, h, field, ref, outs=fills(w, h, bd), weights=fw)
        same2(got_c, p4.chroma_picture(hmo, sc.comps(), w, h, bd, field, ref, fills(w, h, bd, np.int64), cwps), ("chroma model", w, h, bd))
        images = [engine.predict_chroma_refs_frame(sc.flat(), w, h, fq, rq, outs=fills(w, h, bd), weights=fw) for fq, rq in quads]
        same2(got_c, [p4.compose([im[c] for im in images], w, h, 2) for c in range(2)], ("four chroma calls of the 64 form", w, h, bd))
        assert not np.array_equal(got_c[0], got_c[1])
    return got


# ---- 1: on replicated fields the image is bit for bit that of the 64 form ------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", [(64, 64), (101, 71), (130, 66), (16, 16)])
def test_replicated_fields_give_the_image_of_the_64_form(engine, size, bd):
    w, h = size
    s = 1 << (bd - 8)
    sc = Scene(engine, w, h, bd, seed=3100 + w + bd, n=3)
    try:
        n = dims(w, h)[0] * dims(w, h)[1]
        f64 = random_field(n, 64, 3101 + w + bd, max_pel=30)
        r64 = np.random.default_rng(3102 + w).choice(np.array([0, 1, 2, 2, 3, 0xFF], np.uint8), size=(n, 64))
        r64[0, :3] = (0, 1, 2)                                                    # whatever the size: every reference is used inside the picture
        f4, r4 = p4.replicate(f64), p4.replicate(r64)
        assert p4.mixed_blocks(f4, r4) == 0
        wps = [(70, 9 * s, 6, 32), IDENT, (35, -14 * s, 5, 16)]
        dt, sv = sentinel(bd)
        # n_refs = 1 and no reference field: hmme_predict_frame
        one = engine.predict_refs4_frame(sc.y[:1], f4, None, out=fill(w, h, bd))
        same(one, engine.predict_frame(sc.y[0], f64, out=fill(w, h, bd)), "predict_frame")
        assert (one != sv).any()
        one_w = engine.predict_refs4_frame(sc.y[:1], f4, None, out=fill(w, h, bd), weights=wps[:1])
        same(one_w, engine.predict_frame_w(sc.y[0], wps[0], f64, out=fill(w, h, bd)), "predict_frame_w")
        assert not np.array_equal(one, one_w)
        got = engine.predict_refs4_frame(sc.y, f4, r4, out=fill(w, h, bd))
        same(got, engine.predict_refs_frame(sc.y, f64, r64, out=fill(w, h, bd)), "predict_refs_frame")
        got_w = engine.predict_refs4_frame(sc.y, f4, r4, out=fill(w, h, bd), weights=wps)
        same(got_w, engine.predict_refs_w_frame(sc.y, wps, f64, r64, out=fill(w, h, bd)), "predict_refs_w_frame")
        assert not np.array_equal(got, got_w) and (w < 64 or (got == sv).any())
        if sc.chroma:
            cw = [[(64 + 5 * r + 3 * c, (r - c) * s, 6, 32) for r in range(3)] for c in range(2)]
            for weights in (None, flat_weights(cw)):
                got_c = engine.predict_chroma_refs4_frame(sc.flat(), w, h, f4, r4, outs=fills(w, h, bd), weights=weights)
                same2(got_c, engine.predict_chroma_refs_frame(sc.flat(), w, h, f64, r64, outs=fills(w, h, bd), weights=weights), ("chroma", weights is not None))
                assert all((g != sv).any() for g in got_c)
    finally:
        sc.close()


# ---- 2: the rule on 4x4 fields -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("size", [(100, 70), (9, 9)])
def test_the_rule_on_random_4x4_fields(engine, hmo, size, bd):
    """100 x 70: 2 x 2 CTUs, the last row of 4x4 blocks cut in half (and one chroma row left of it), a partial CTU column; 9 x 9: a last
    block row and column of one sample"""
    w, h = size
    n_refs = 3
    sc = Scene(engine, w, h, bd, seed=3200 + w + bd, n=n_refs)
    try:
        field, ref = p4.random_field4(w, h, n_refs, 3201 + w)
        if w == 9:                                                                # nine blocks: all live, the phases dealt out, the corners as drawn
            ref[0, [0, 1, 2, 16, 17, 18, 32, 33, 34]] = (0, 1, 2, 1, 2, 0, 2, 0, 1)
            field[0, [1, 16, 17, 18, 33]] = ((-6, 9), (11, -8), (-3, 6), (4, 3), (-9, -2))
        px, py, pairs = p4.phases_seen(w, h, field, ref, n_refs)
        assert px == py == {0, 1, 2, 3} and (w == 9 or len(pairs) == 16)
        if w > 9:                                                                 # chroma reads the MV in eighths: all eight phases on each axis
            live = [(int(field[c, b, 0]) & 7, int(field[c, b, 1]) & 7) for c, b, *_ in p4.live_blocks(w, h, ref, n_refs)]
            assert {p[0] for p in live} == {p[1] for p in live} == set(range(8))
            assert {0, 1, 2, 3, 0xFF} <= set(ref.reshape(-1).tolist())
        # MVs at +-32767 and beyond the picture: the clamp acts on all four sides
        acts = set()
        for c, b, cu_x, cu_y, *_ in p4.live_blocks(w, h, ref, n_refs):
            mx, my = int(field[c, b, 0]), int(field[c, b, 1])
            qx, qy = clip_mv(hmo, mx, my, cu_x, cu_y, w, h)
            acts |= {("x", np.sign(qx - mx)), ("y", np.sign(qy - my))}
        assert {("x", 1), ("x", -1), ("y", 1), ("y", -1)} <= acts and (np.abs(field.astype(np.int32)) >= 32767).any()
        got = check_rule(engine, hmo, sc, field, ref)
        dt, sv = sentinel(bd)
        assert (got != sv).any() and (w == 9 or (got == sv).any())
    finally:
        sc.close()


# ---- 3: block patterns inside one CTU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_block_patterns_inside_one_ctu(engine, hmo, bd):
    """uniform, 8x4, 4x8, four MVs, four references, a dead quadrant and wholly dead 8x8 blocks side by side: the four waves of an iteration
    (four neighbouring 8x8 blocks) each see a different pattern, and every dead block has live neighbours"""
    w = h = 64
    sc = Scene(engine, w, h, bd, seed=3300 + bd, n=4)
    try:
        field, ref, names = p4.pattern_ctu(4, 3301 + bd)
        assert {n for row in names for n in row} == set(p4.PATTERNS)
        for by in range(8):
            for half in range(2):
                assert len({names[by][4 * half + k] for k in range(4)}) == 4       # one iteration: blocks 4 it .. 4 it + 3
            for bx in range(8):
                if names[by][bx] == "dead":
                    assert any(names[by][x] != "dead" for x in (bx - 1, bx + 1) if 0 <= x < 8)
        f, r = field.reshape(16, 16, 2), ref.reshape(16, 16)
        for by in range(8):
            for bx in range(8):
                mvs = {tuple(v) for v in f[2 * by:2 * by + 2, 2 * bx:2 * bx + 2].reshape(4, 2).tolist()}
                rs = r[2 * by:2 * by + 2, 2 * bx:2 * bx + 2].reshape(4).tolist()
                want = {"uniform": (1, 1), "top_bottom": (2, 1), "left_right": (2, 1), "four_mvs": (4, 1), "four_refs": (1, 4)}.get(names[by][bx])
                if want:
                    assert (len(mvs), len(set(rs))) == want and max(rs) < 4
                elif names[by][bx] == "dead":
                    assert min(rs) >= 4
                else:
                    assert sum(1 for v in rs if v >= 4) == 1
        got = check_rule(engine, hmo, sc, field, ref)
        dt, sv = sentinel(bd)
        dead = np.repeat(np.repeat(r >= 4, 4, axis=0), 4, axis=1)
        assert (got[dead] == sv).all() and dead.any() and (got[~dead] != sv).any()
    finally:
        sc.close()


# ---- 4: weights --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_one_weight_per_reference(engine, hmo, bd):
    from hmme import api
    w, h = 100, 70
    s = 1 << (bd - 8)
    sc = Scene(engine, w, h, bd, seed=3400 + bd, n=3)
    try:
        field, ref = p4.random_field4(w, h, 3, 3401 + bd)
        wps = [(70, 9 * s, 6, 32), IDENT, (35, -14 * s, 5, 16)]                   # an identity among them, a negative offset, a shift other than 6
        cwps = [[(64 + 9 * r, (3 - 5 * r) * s, 6, 32) for r in range(3)], [(29 + 4 * r, (11 * r - 6) * s, 5, 16) for r in range(3)]]   # Cb and Cr differ
        assert all(api.bipred_weight_check(bd, IDENT, wp, 0) == 0 for wp in wps + cwps[0] + cwps[1]) and cwps[0] != cwps[1]
        got_w = check_rule(engine, hmo, sc, field, ref, wps, cwps)
        plain = engine.predict_refs4_frame(sc.y, field, ref, out=fill(w, h, bd))
        assert not np.array_equal(got_w, plain)
        on_ident = np.repeat(np.repeat(ref.reshape(-1, 16, 16) == 1, 4, axis=1), 4, axis=2)
        # all identities: the unweighted image, luma and chroma
        same(engine.predict_refs4_frame(sc.y, field, ref, out=fill(w, h, bd), weights=[IDENT, (32, 0, 5, 16), (1, 0, 0, 0)]), plain, "identities")
        plain_c = engine.predict_chroma_refs4_frame(sc.flat(), w, h, field, ref, outs=fills(w, h, bd))
        same2(engine.predict_chroma_refs4_frame(sc.flat(), w, h, field, ref, outs=fills(w, h, bd), weights=[IDENT] * 6), plain_c, "chroma identities")
        assert on_ident.any()
    finally:
        sc.close()


# ---- 5: forms ----------------------------------------------------------------------------------------------------------------------------
def test_ctu_sub_range_and_strided_image(engine, hmo):
    w, h, bd = 136, 72, 8
    sc = Scene(engine, w, h, bd, seed=3500, n=2)
    try:
        field, ref = p4.random_field4(w, h, 2, 3501)
        dt, sv = sentinel(bd)
        for first, count in ((1, 2), (4, 1), (2, 0)):
            ctus = range(first, first + count)
            got = engine.predict_refs4_frame(sc.y, field, ref, out=fill(w, h, bd), ctu_first=first, ctu_count=count)
            same(got, p4.luma_picture(hmo, sc.luma, w, h, bd, field, ref, fill(w, h, bd, np.int64), ctus=ctus), ("range", first, count))
            got_c = engine.predict_chroma_refs4_frame(sc.flat(), w, h, field, ref, outs=fills(w, h, bd), ctu_first=first, ctu_count=count)
            same2(got_c, p4.chroma_picture(hmo, sc.comps(), w, h, bd, field, ref, fills(w, h, bd, np.int64), ctus=ctus), ("chroma range", first, count))
            assert ((got != sv).any()) == (count > 0)
        ra = (C.c_void_p * 2)(*[p.h for p in sc.y])
        check_strided_image(w, h, bd, lambda out, first, count: engine.predict_refs4_frame(sc.y, field, ref, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_refs4_frame(engine.h, ra, 2, C.byref(fp), None, field.ctypes.data, ref.ctypes.data, out, stride))
    finally:
        sc.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_device_entries_with_sixteen_and_eight_references(engine, bd):
    """the device forms on device buffers, pitches wider than a row, every reference in use; the _frame forms are the yardstick"""
    import torch
    from hmme import api
    w, h = 100, 70
    dev = torch.device("cuda", 0)
    sc = Scene(engine, w, h, bd, seed=3600 + bd, n=16, chroma=False)
    sc8 = Scene(engine, w, h, bd, seed=3650 + bd, n=8)
    try:
        dt, sv = sentinel(bd)
        bps = 1 if bd == 8 else 2
        s = 1 << (bd - 8)
        to_dev = lambda a: torch.from_numpy(a if a.dtype != np.uint16 else a.view(np.int16)).to(dev)
        for scene, n_refs, comps in ((sc, 16, 1), (sc8, 8, 2)):
            field, ref = p4.random_field4(w, h, n_refs, 3601 + n_refs)
            assert set(range(n_refs)) <= set(ref.reshape(-1).tolist())
            d_field, d_ref = to_dev(field), to_dev(ref)
            fp = api.FrameParams(1, 0, bd, 0, -1)
            pw, ph = (w, h) if comps == 1 else (w // 2, h // 2)
            for weighted in (False, True):
                wps = [(60 + r, (r - 5) * s, 6, 32) for r in range(comps * n_refs)] if weighted else None
                d_imgs = [to_dev(np.full((ph, pw + 12), sv, dt)) for _ in range(comps)]
                torch.cuda.synchronize()
                if comps == 1:
                    engine.predict_refs4_device(scene.y, fp, d_field.data_ptr(), d_ref.data_ptr(), d_imgs[0].data_ptr(), (pw + 12) * bps, weights=wps)
                    want = [engine.predict_refs4_frame(scene.y, field, ref, out=fill(w, h, bd), weights=wps)]
                else:
                    engine.predict_chroma_refs4_device(scene.flat(), w, h, fp, d_field.data_ptr(), d_ref.data_ptr(), d_imgs[0].data_ptr(), d_imgs[1].data_ptr(),
                                                       (pw + 12) * bps, weights=wps)
                    want = engine.predict_chroma_refs4_frame(scene.flat(), w, h, field, ref, outs=fills(w, h, bd), weights=wps)
                torch.cuda.synchronize()
                for d_img, wanted in zip(d_imgs, want):
                    back = d_img.cpu().numpy().view(dt)
                    same(back[:, :pw], wanted, ("device", n_refs, comps, weighted))
                    assert (back[:, pw:] == sv).all() and (wanted != sv).any()
            # no reference field: every block from reference 0
            d_img = to_dev(np.full((ph, pw), sv, dt))
            d_img2 = to_dev(np.full((ph, pw), sv, dt))
            torch.cuda.synchronize()
            if comps == 1:
                engine.predict_refs4_device(scene.y, fp, d_field.data_ptr(), None, d_img.data_ptr(), pw * bps)
                want0 = engine.predict_refs4_frame(scene.y, field, np.zeros_like(ref), out=fill(w, h, bd))
            else:
                engine.predict_chroma_refs4_device(scene.flat(), w, h, fp, d_field.data_ptr(), None, d_img.data_ptr(), d_img2.data_ptr(), pw * bps)
                want0 = engine.predict_chroma_refs4_frame(scene.flat(), w, h, field, np.zeros_like(ref), outs=fills(w, h, bd))[0]
            torch.cuda.synchronize()
            same(d_img.cpu().numpy().view(dt), want0, ("no reference field", comps))
            assert (want0 != sv).mean() > 0.9                                     # every block is live (a sample may hold the sentinel's value)
    finally:
        sc.close(); sc8.close()


def test_a_used_context_gives_what_a_fresh_one_gives(engine):
    """the module's engine has run every call of this file (and runs another 64-form call first); a context made here has run nothing"""
    from hmme import api
    w, h, bd = 100, 70, 10
    field, ref = p4.random_field4(w, h, 2, 3701)
    cw = [(70, 36, 6, 32), IDENT, (40, -20, 5, 16), (64, 4, 6, 32)]
    results = []
    fresh = api.Engine(0, 64)
    try:
        for e in (engine, fresh):
            sc = Scene(e, w, h, bd, seed=3700, n=2)
            try:
                if e is engine:
                    e.predict_refs_frame(sc.y, p4.quadrant_fields(field, ref)[0][0], p4.quadrant_fields(field, ref)[0][1])
                results.append((e.predict_refs4_frame(sc.y, field, ref, out=fill(w, h, bd), weights=cw[:2]),
                                *e.predict_chroma_refs4_frame(sc.flat(), w, h, field, ref, outs=fills(w, h, bd), weights=cw)))
            finally:
                sc.close()
    finally:
        fresh.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b) and (a != sentinel(bd)[1]).any()


# ---- 6: refusals: one case per layer, the code of the matching refs entry, the new entry's name, nothing written ----------------------------------
def test_refusals(engine):
    from hmme import api
    L = api.load()
    w, h = 128, 64
    n = 2
    other = api.Engine(0, 64)
    y = [engine.plane(w, h), engine.plane(w, h)]
    cc = [engine.plane(w // 2, h // 2) for _ in range(4)]
    small, deep, foreign = engine.plane(64, 64), engine.plane(w, h, 10), other.plane(w, h)
    c_small, c_deep, c_foreign = engine.plane(32, 32), engine.plane(w // 2, h // 2, 10), other.plane(w // 2, h // 2)
    odd_cb, odd_cr = engine.plane(50, 35), engine.plane(50, 35)                   # the chroma of 100 x 70; asked for with 101 x 70
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        field, ref = np.zeros((n, 256, 2), np.int16), np.zeros((n, 256), np.uint8)
        img = np.full((h, w), 0x5C, np.uint8)
        cimg = [np.full((h // 2, w // 2), 0x5C, np.uint8) for _ in range(2)]
        couts = (C.c_void_p * 2)(cimg[0].ctypes.data, cimg[1].ctypes.data)
        hs = lambda ps: (C.c_void_p * len(ps))(*[p.h for p in ps])
        wa = lambda ws: (api.Weight * len(ws))(*[api.Weight(*w) for w in ws])
        fp = api.FrameParams(1, 0, 8, 0, -1)
        fpr, F, R, I = C.byref(fp), field.ctypes.data, ref.ctypes.data, img.ctypes.data
        D = 256                                                                   # a device address that is never dereferenced
        good, huge = (70, 9, 6, 32), (1 << 20, 0, 6, 32)
        out_of_range = api.FrameParams(1, 0, 8, 1, 2)
        y17, c18 = hs([y[0]] * 17), hs(cc[:2] * 9)

        def luma_frame(refs=None, n_refs=2, fpa=fpr, wps=None, f=F, r=R, out=I, stride=w):
            return "hmme_predict_refs4_frame", L.hmme_predict_refs4_frame(engine.h, refs or hs(y), n_refs, fpa, wps, f, r, out, stride)

        def luma_dev(refs=None, n_refs=2, fpa=fpr, wps=None, f=D, r=D, out=D, pitch=w):
            return "hmme_predict_refs4_device", L.hmme_predict_refs4_device(engine.h, refs or hs(y), n_refs, fpa, wps, f, r, out, pitch, None)

        def chroma_frame(refs=None, n_refs=2, lw=w, lh=h, fpa=fpr, wps=None, f=F, r=R, outs=couts, stride=w // 2):
            return "hmme_predict_chroma_refs4_frame", L.hmme_predict_chroma_refs4_frame(engine.h, refs or hs(cc), n_refs, lw, lh, fpa, wps, f, r, outs, stride)

        def chroma_dev(refs=None, n_refs=2, lw=w, lh=h, fpa=fpr, wps=None, f=D, r=D, cb=D, cr=D, pitch=w // 2):
            return "hmme_predict_chroma_refs4_device", L.hmme_predict_chroma_refs4_device(engine.h, refs or hs(cc), n_refs, lw, lh, fpa, wps, f, r, cb, cr, pitch, None)

        cases = [
            # a NULL field or image
            (luma_frame(f=None), ERR_ARG), (luma_frame(out=None), ERR_ARG), (luma_dev(f=None), ERR_ARG), (luma_dev(out=None), ERR_ARG),
            (chroma_frame(f=None), ERR_ARG), (chroma_frame(outs=None), ERR_ARG), (chroma_dev(f=None), ERR_ARG), (chroma_dev(cr=None), ERR_ARG),
            # n_refs 0 and 17 (chroma 9)
            (luma_frame(n_refs=0), ERR_ARG), (luma_frame(refs=y17, n_refs=17), ERR_ARG), (luma_dev(n_refs=0), ERR_ARG), (luma_dev(refs=y17, n_refs=17), ERR_ARG),
            (chroma_frame(n_refs=0), ERR_ARG), (chroma_frame(refs=c18, n_refs=9), ERR_ARG), (chroma_dev(n_refs=0), ERR_ARG), (chroma_dev(refs=c18, n_refs=9), ERR_ARG),
            # a pitch below a row
            (luma_frame(stride=w - 1), ERR_ARG), (luma_dev(pitch=w - 1), ERR_ARG), (chroma_frame(stride=w // 2 - 1), ERR_ARG), (chroma_dev(pitch=w // 2 - 1), ERR_ARG),
            # a plane of another size, depth or context
            (luma_frame(refs=hs([y[0], small])), ERR_ARG), (luma_frame(refs=hs([y[0], deep])), ERR_ARG), (luma_frame(refs=hs([y[0], foreign])), ERR_ARG),
            (luma_frame(refs=hs([foreign, y[0]])), ERR_ARG), (luma_dev(refs=hs([y[0], small])), ERR_ARG), (luma_dev(refs=hs([y[0], deep])), ERR_ARG),
            (luma_dev(refs=hs([y[0], foreign])), ERR_ARG),
            (chroma_frame(refs=hs(cc[:3] + [c_small])), ERR_ARG), (chroma_frame(refs=hs(cc[:3] + [c_deep])), ERR_ARG), (chroma_frame(refs=hs(cc[:3] + [c_foreign])), ERR_ARG),
            (chroma_dev(refs=hs(cc[:3] + [c_small])), ERR_ARG), (chroma_dev(refs=hs(cc[:3] + [c_deep])), ERR_ARG), (chroma_dev(refs=hs(cc[:3] + [c_foreign])), ERR_ARG),
            # an odd luma size for chroma
            (chroma_frame(refs=hs([odd_cb, odd_cr]), n_refs=1, lw=101, lh=70), ERR_ARG), (chroma_dev(refs=hs([odd_cb, odd_cr]), n_refs=1, lw=101, lh=70), ERR_ARG),
            # a CTU range outside the picture
            (luma_frame(fpa=C.byref(out_of_range)), ERR_ARG), (luma_dev(fpa=C.byref(out_of_range)), ERR_ARG),
            (chroma_frame(fpa=C.byref(out_of_range)), ERR_ARG), (chroma_dev(fpa=C.byref(out_of_range)), ERR_ARG),
            # a weight the check refuses
            (luma_frame(wps=wa([good, huge])), ERR_UNSUPPORTED), (luma_dev(wps=wa([good, huge])), ERR_UNSUPPORTED),
            (chroma_frame(wps=wa([good, good, good, huge])), ERR_UNSUPPORTED), (chroma_dev(wps=wa([good, good, good, huge])), ERR_UNSUPPORTED),
            (luma_frame(wps=wa([good, (64, 0, 16, 0)])), ERR_ARG), (chroma_dev(wps=wa([good, good, good, (64, 0, -1, 0)])), ERR_ARG),
        ]
        # evaluated in order above: the message of each call is gone by now, so the calls are made again one by one for name and code
        assert all(rc == want for (_, rc), want in cases), [(name, rc, want) for (name, rc), want in cases if rc != want]
        assert (img == 0x5C).all() and all((c == 0x5C).all() for c in cimg)
        for call, kw, want in ((luma_frame, dict(f=None), ERR_ARG), (luma_dev, dict(pitch=w - 1), ERR_ARG), (chroma_frame, dict(stride=w // 2 - 1), ERR_ARG),
                               (chroma_dev, dict(n_refs=0), ERR_ARG), (luma_frame, dict(wps=wa([good, huge])), ERR_UNSUPPORTED),
                               (luma_dev, dict(refs=hs([y[0], small])), ERR_ARG), (luma_frame, dict(refs=hs([y[0], foreign])), ERR_ARG),
                               (chroma_frame, dict(refs=hs([odd_cb, odd_cr]), n_refs=1, lw=101, lh=70), ERR_ARG), (chroma_dev, dict(fpa=C.byref(out_of_range)), ERR_ARG),
                               (luma_dev, dict(fpa=C.byref(out_of_range)), ERR_ARG), (chroma_dev, dict(wps=wa([good, good, good, huge])), ERR_UNSUPPORTED)):
            name, rc = call(**kw)
            msg = L.hmme_last_error(engine.h)
            assert rc == want and name.encode() in msg, (name, kw, rc, msg)
        # the codes are those of the matching refs entries
        f64, r64 = np.zeros((n, 64, 2), np.int16), np.zeros((n, 64), np.uint8)
        assert L.hmme_predict_refs_frame(engine.h, hs(y), 2, fpr, f64.ctypes.data, r64.ctypes.data, 64, I, w - 1) == ERR_ARG
        assert L.hmme_predict_refs_w_frame(engine.h, hs(y), 2, fpr, wa([good, huge]), f64.ctypes.data, r64.ctypes.data, 64, I, w) == ERR_UNSUPPORTED
        assert L.hmme_predict_chroma_refs_device(engine.h, hs(cc[:3] + [c_small]), 2, w, h, fpr, None, D, D, 64, D, D, w // 2, None) == ERR_ARG
        assert L.hmme_predict_refs_device(engine.h, hs(y), 2, C.byref(out_of_range), D, D, 64, D, w, None) == ERR_ARG
        assert (img == 0x5C).all() and all((c == 0x5C).all() for c in cimg)
        # what is an argument here and an error there: no reference field
        assert luma_frame(r=None)[1] == 0 and chroma_frame(r=None)[1] == 0 and (img != 0x5C).any() and (cimg[0] != 0x5C).any()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in y + cc + [small, deep, foreign, c_small, c_deep, c_foreign, odd_cb, odd_cr]:
            p.close()
        other.close()


# ---- 7: a P picture end to end, all shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 2])
def test_a_p_picture_end_to_end(engine, hmo, depth):
    """decision at 256 -> prediction -> residual, every step against its model: depth 3 forces 8x8 CUs (8x4 / 4x8 PUs), depth 2 16x16 CUs
    with AMP (16x4, 16x12, 4x16, 12x16 PUs); tests/test_predict4_cpu.py shows the recipe chooses them"""
    from hmme import api, synth
    w, h, bd = 128, 64, 8
    m = synth.MARGIN
    sc = Scene(engine, w, h, bd, seed=3800, n=2)
    cur = synth.make_pair(w, h, seed=3801, bit_depth=bd, max_mv=2)[0]
    pc = mkplane(engine, cur, w, h, bd)
    try:
        mv, cost = srm.random_ref_tables(2, 2, seed=7)
        sel = api.SelectParams(256, min_depth=depth, max_depth=depth)
        field, ref, slot, _ = engine.select_refs_frame(w, h, sel, mv, cost)
        mf, mr, ms, _, leaves = srm.select_refs_picture(mv, cost, sel, w, h)
        assert np.array_equal(field, mf) and np.array_equal(ref, mr) and np.array_equal(slot, ms)
        sizes = {ps for d, ps in leaves}
        assert ({1, 2} <= sizes if depth == 3 else {4, 5, 6, 7} <= sizes) and p4.mixed_blocks(field, ref) >= 20
        assert {0, 1} == set(ref.reshape(-1).tolist())
        pred = engine.predict_refs4_frame(sc.y, field, ref, out=fill(w, h, bd))
        same(pred, p4.luma_picture(hmo, sc.luma, w, h, bd, field, ref, fill(w, h, bd, np.int64)), ("prediction", depth))
        got_c = engine.predict_chroma_refs4_frame(sc.flat(), w, h, field, ref, outs=fills(w, h, bd))
        same2(got_c, p4.chroma_picture(hmo, sc.comps(), w, h, bd, field, ref, fills(w, h, bd, np.int64)), ("chroma prediction", depth))
        cur_img = cur[m:m + h, m:m + w]
        for had in (True, False):
            res, pu, cu, ctu = engine.residual_frame(pc, pred, slot, 256, had)
            md, mpu, mcu, mctu = rm.residual_picture(hmo, cur_img, pred, w, h, bd, slot, 256, had)
            assert np.array_equal(res, md) and np.array_equal(pu, mpu) and np.array_equal(cu, mcu) and np.array_equal(ctu, mctu), (depth, had)
        assert res.any()
    finally:
        sc.close(); pc.close()
