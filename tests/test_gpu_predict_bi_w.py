"""The prediction of a picture whose blocks are L0, L1 or bi in a slice with explicit weighted prediction (hmme_predict_bi_w_device / _frame)
against tests/predict_bi_w_model.py -- TComWeightPrediction::addWeightBi / addWeightUni over the 14-bit intermediates, restated in numpy --,
for blocks of one list against Engine.predict_frame_w, for identity weights against Engine.predict_bi_frame; and the whole chain of a WP
slice on pictures: hmme_wp_estimate, weighted search and refinement, the partition per list, the weighted bi pass in both directions,
hmme_select_dirs_device, hmme_predict_bi_w_device.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
import predict_bi_w_model as pm
import range_content as rc
import select_dirs_model as sdm
from frame_helpers import bind_hmo, check_strided_image, dims, mkplane

pytestmark = pytest.mark.gpu

W, H = 136, 72                                                # 3 x 2 CTUs, the right column and the bottom row partial
SIZES = ((64, 64), (100, 70), (136, 72))                      # one CTU; 2 x 2 with both edges partial; 3 x 2
# (list 0, list 1) as (w0, offset in 8-bit units, shift): HM-like positive weights with offsets, a negative weight, a large shift
WEIGHT_SETS = {"hm_like": ((70, 9, 6), (55, -14, 6)), "negative": ((-37, 150, 5), (90, -3, 5)), "large_shift": ((30000, 2, 15), (15000, -1, 15))}


def wset(name, bd):
    """the weights of a set at a bit depth: offsets scale with the depth, round is what initWpScaling would give (and is not used)"""
    return tuple((w, o * (1 << (bd - 8)), d, 1 << (d - 1)) for w, o, d in WEIGHT_SETS[name])


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


def textures(w, h, bd, seed):
    """two unrelated padded pictures"""
    from hmme import synth
    return [synth.make_pair(w, h, seed=seed + 7 * k, bit_depth=bd, max_mv=2)[1] for k in range(2)]


def in_picture(w, h):
    cx_n, cy_n = dims(w, h)
    return [(c, b) for c in range(cx_n * cy_n) for b in range(64) if (c % cx_n) * 64 + (b % 8) * 8 < w and (c // cx_n) * 64 + (b // 8) * 8 < h]


def inputs(w, h, per, seed, rnd=0, n_bi=110):
    """(field int16[2, n, per, 2], dirs uint8[n, per]).  One MV per 8x8 block: n_bi of the blocks inside the picture are bi and take the
    pairs of quarter-pel phases of the two lists number rnd * n_bi onward (16 x 16 pairs), the rest are drawn from 1, 2, 3, 0xFF, 0 and 4; MVs reach beyond TComDataCU::clipMv's range on both axes in both lists.  One MV per CTU: directions 3, 1, 2, 0xFF, 3, 3
    as far as there are CTUs"""
    cx_n, cy_n = dims(w, h)
    n = cx_n * cy_n
    rng = np.random.default_rng(seed + 1000 * rnd)
    field = (4 * rng.integers(-200, 201, size=(2, n, per, 2))).astype(np.int16)
    if per == 1:
        field[:, :, 0] += rng.integers(0, 4, size=(2, n, 2)).astype(np.int16)
        field[0, 0, 0], field[1, 0, 0] = (-700, 650), (700, -650)
        dirs = np.array([3, 1, 2, 0xFF, 3, 3][:n], np.uint8).reshape(n, 1)
        return field, dirs
    dirs = rng.choice(np.array([1, 2, 3, 0xFF, 0, 4], np.uint8), size=(n, per))
    dirs[0, :2], dirs[0, 8:12] = (1, 2), (0xFF, 4, 0, 1)        # every kind inside the picture, whatever was drawn
    made = 0
    for j, (c, b) in enumerate(in_picture(w, h)):
        make_bi = j >= 2 and made < n_bi and not (c == 0 and 8 <= b < 12)
        k = rnd * n_bi + made if make_bi else j
        field[0, c, b] += (k & 3, (k >> 2) & 3)
        field[1, c, b] += ((k >> 4) & 3, (k >> 6) & 3)
        if make_bi:
            dirs[c, b], made = 3, made + 1
    for l in range(2):
        assert (field[l, 0, :, 0] < -4 * (64 + 8)).any() and (field[l, 0, :, 1] > 4 * (h + 8)).any()   # beyond the clip range at CTU 0
    return field, dirs


def phase_pairs(w, h, field, dirs):
    return {(int(field[0, c, b, 0]) & 3, int(field[0, c, b, 1]) & 3, int(field[1, c, b, 0]) & 3, int(field[1, c, b, 1]) & 3)
            for c, b in in_picture(w, h) if dirs[c, b] == 3}


def blocks_of(w, h, dirs, per, want):
    """boolean [h, w]: the samples of the blocks whose direction is in `want`"""
    cx_n, cy_n = dims(w, h)
    g = 64 if per == 1 else 8
    mask = np.zeros((cy_n * 64, cx_n * 64), bool)
    for c in range(cx_n * cy_n):
        for b in range(per):
            if int(dirs[c, b]) in want:
                x0, y0 = (c % cx_n) * 64 + (b % 8) * g, (c // cx_n) * 64 + (b // 8) * g
                mask[y0:y0 + g, x0:x0 + g] = True
    return mask[:h, :w]


def sentinel(bd):
    return (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)


def check_picture(engine, hmo, refs, planes, w, h, bd, field, dirs, wps):
    """one weighted picture against the model; its uni blocks against predict_frame_w, its dead blocks against the sentinel -> the picture"""
    dt, fill = sentinel(bd)
    per = dirs.shape[1]
    got = engine.predict_bi_w_frame(planes[0], planes[1], wps[0], wps[1], field, dirs, out=np.full((h, w), fill, dt))
    want = pm.pred_picture(hmo, refs, w, h, bd, field, dirs, wps, np.full((h, w), fill, np.int64))
    assert np.array_equal(got, want), (w, h, bd, per, wps, np.argwhere(got != want)[:4])
    for l in range(2):
        m = blocks_of(w, h, dirs, per, {l + 1})
        if m.any():
            assert np.array_equal(got[m], engine.predict_frame_w(planes[l], wps[l], field[l])[m])
    dead = blocks_of(w, h, dirs, per, {0, 4, 0xFF})
    assert (got[dead] == fill).all()
    return got


@pytest.mark.parametrize("name", list(WEIGHT_SETS))
@pytest.mark.parametrize("bd", [8, 10])
def test_all_phase_pairs_of_bi_blocks(engine, hmo, bd, name):
    from hmme import api
    wps = wset(name, bd)
    assert api.predict_bi_weight_check(bd, *wps) == 0
    refs = textures(W, H, bd, seed=1800 + bd)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        seen, kinds = set(), set()
        for rnd in range(3):                                                    # 3 x 110 bi blocks >= the 256 pairs of phases
            field, dirs = inputs(W, H, 64, 1810 + bd, rnd)
            seen |= phase_pairs(W, H, field, dirs)
            got = check_picture(engine, hmo, refs, planes, W, H, bd, field, dirs, wps)
            kinds |= {int(dirs[c, b]) for c, b in in_picture(W, H)}
            bi = blocks_of(W, H, dirs, 64, {3})
            assert not np.array_equal(got[bi], engine.predict_bi_frame(planes[0], planes[1], field, dirs)[bi])   # the weights act
        assert len(seen) == 256 and kinds >= {0, 1, 2, 3, 4, 0xFF}
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", SIZES)
def test_sizes_and_fields_of_either_granularity(engine, hmo, size, bd, per):
    w, h = size
    refs = textures(w, h, bd, seed=1820 + bd + w)
    planes = [mkplane(engine, r, w, h, bd) for r in refs]
    try:
        field, dirs = inputs(w, h, per, 1830 + bd + per + w, n_bi=40)
        got = check_picture(engine, hmo, refs, planes, w, h, bd, field, dirs, wset("hm_like", bd))
        n = dirs.shape[0]                                                       # one MV per CTU: as many kinds as there are CTUs
        assert blocks_of(w, h, dirs, per, {3}).any()
        assert (blocks_of(w, h, dirs, per, {1}).any() or (per == 1 and n < 2)) and (blocks_of(w, h, dirs, per, {2}).any() or (per == 1 and n < 3))
        assert blocks_of(w, h, dirs, per, {0, 4, 0xFF}).any() or (per == 1 and n < 4)
    finally:
        for p in planes:
            p.close()


def test_twelve_bits_where_the_head_room_clamps_at_two(engine, hmo):
    bd = 12
    refs = textures(W, H, bd, seed=1840)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        field, dirs = inputs(W, H, 64, 1841)
        for name in WEIGHT_SETS:
            check_picture(engine, hmo, refs, planes, W, H, bd, field, dirs, wset(name, bd))
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_identities(engine, hmo, bd):
    refs = textures(W, H, bd, seed=1850 + bd)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        field, dirs = inputs(W, H, 64, 1851 + bd)
        plain = engine.predict_bi_frame(planes[0], planes[1], field, dirs)
        # both the identity, whatever the denominator and whatever round holds: hmme_predict_bi_frame
        for d, rnd in ((0, 0), (6, 32), (6, 5), (7, 64), (14, 1 << 13)):
            got = engine.predict_bi_w_frame(planes[0], planes[1], (1 << d, 0, d, rnd), (1 << d, 0, d, rnd), field, dirs)
            assert np.array_equal(got, plain), d
        # one list the identity, the other not: the weighted kernel serves both, the identity's uni blocks equal the unweighted ones
        other = wset("hm_like", bd)[1]
        for wps in ((pm.ident(6), other), (other, pm.ident(6))):
            got = check_picture(engine, hmo, refs, planes, W, H, bd, field, dirs, wps)
            l = 0 if wps[0] == pm.ident(6) else 1
            m = blocks_of(W, H, dirs, 64, {l + 1})
            assert m.any() and np.array_equal(got[m], plain[m])
            m = blocks_of(W, H, dirs, 64, {3, 2 - l})
            assert not np.array_equal(got[m], plain[m])
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_last_accepted_weights_on_extreme_content(engine, hmo, bd):
    """the weights next to a refusal (tests/test_predict_bi_w_cpu.py finds them the same way) on pictures of samples in {0, maxv}: the int32
    numerator at its bound"""
    from hmme import api
    _, ref0, ref1 = rc.extreme_triple(W, H, bd, seed=1860 + bd)
    refs = [ref0, ref1]
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        field, dirs = inputs(W, H, 64, 1861 + bd)
        field = (field // 16).astype(np.int16)                                  # fractional MVs of a few pels: the patterns, not the flat border
        dirs[dirs > 3] = 3
        cases = []
        for name, member in rc.families(bd).items():
            other = pm.ident(member(0)[2])
            cases.append((bwm.last_accepted(member, lambda w: api.predict_bi_weight_check(bd, w, other))[1], other))
        pair = lambda k: (1 + k, 0, 0, 0)
        both = bwm.last_accepted(pair, lambda w: api.predict_bi_weight_check(bd, w, w))[1]
        cases += [(both, both), (cases[0][1], cases[0][0])]
        reach = 0
        for wps in cases:
            assert api.predict_bi_weight_check(bd, *wps) == 0
            reach = max(reach, pm.pair_reach(bd, *wps))
            check_picture(engine, hmo, refs, planes, W, H, bd, field, dirs, wps)
        assert reach > pm.INT32_MAX - 2 * pm.PEL_REACH                          # within one step of a weight of the bound
    finally:
        for p in planes:
            p.close()


def test_two_pictures_with_different_weights_in_one_launch(engine, hmo):
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    refs = textures(W, H, 8, seed=1870) + textures(W, H, 8, seed=1880)       # picture 0: lists (0, 1); picture 1: lists (2, 3)
    planes = [mkplane(engine, r, W, H, 8) for r in refs]
    try:
        f0, d0 = inputs(W, H, 64, seed=1871)
        f1, d1 = inputs(W, H, 64, seed=1872)
        w_a, w_b = wset("hm_like", 8), wset("negative", 8)
        d_field = torch.from_numpy(np.stack([f0, f1])).to(dev)
        d_dirs = torch.from_numpy(np.stack([d0, d1])).to(dev)
        imgs = [torch.full((H, W + 24), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        fp = api.FrameParams(1, 0, 8, 1, 4)                                     # CTUs 1..4 of both, into images whose pitch exceeds the width
        engine.predict_bi_w_device([planes[0], planes[2]], [planes[1], planes[3]], fp, [w_a[0], w_b[0]], [w_a[1], w_b[1]], d_field.data_ptr(), d_dirs.data_ptr(),
                                   64, [i.data_ptr() for i in imgs], W + 24, 0)
        torch.cuda.synchronize()
        for i, (f, d, wps) in enumerate(((f0, d0, w_a), (f1, d1, w_b))):
            want = pm.pred_picture(hmo, refs[2 * i:2 * i + 2], W, H, 8, f, d, wps, np.full((H, W), 0xA5, np.int64), ctus=range(1, 5))
            got = imgs[i].cpu().numpy()
            assert np.array_equal(got[:, :W], want) and (got[:, W:] == 0xA5).all()
            assert (want[:64, :64] == 0xA5).all() and (want[64:, 128:] == 0xA5).all() and (want != 0xA5).any()
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_ctu_sub_range_and_strided_image(engine, bd):
    refs = textures(W, H, bd, seed=1890 + bd)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        from hmme import api
        field, dirs = inputs(W, H, 64, 1891 + bd)
        wps = wset("hm_like", bd)
        dt, fill = sentinel(bd)
        whole = engine.predict_bi_w_frame(planes[0], planes[1], wps[0], wps[1], field, dirs, out=np.full((H, W), fill, dt))
        part = engine.predict_bi_w_frame(planes[0], planes[1], wps[0], wps[1], field, dirs, out=np.full((H, W), fill, dt), ctu_first=1, ctu_count=1)
        assert np.array_equal(part[:64, 64:128], whole[:64, 64:128])
        part[:64, 64:128] = fill
        assert (part == fill).all()
        f = np.ascontiguousarray(field)
        w0, w1 = (api.Weight(*w) for w in wps)
        check_strided_image(W, H, bd, lambda out, first, count: engine.predict_bi_w_frame(planes[0], planes[1], wps[0], wps[1], field, dirs, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_bi_w_frame(engine.h, planes[0].h, planes[1].h, C.byref(fp), C.byref(w0), C.byref(w1), f.ctypes.data,
                                                                                     dirs.ctypes.data, 64, out, stride))
    finally:
        for p in planes:
            p.close()


def test_refusals_launch_and_write_nothing(engine):
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    field, dirs = np.zeros((2, 6, 64, 2), np.int16), np.full((6, 64), 3, np.uint8)
    other_engine = api.Engine(0, 64)
    a, b, small, deep, foreign = engine.plane(W, H), engine.plane(W, H), engine.plane(64, 64), engine.plane(W, H, 10), other_engine.plane(W, H)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        img = np.full((H, W), 0x5C, np.uint8)
        fp8 = api.FrameParams(1, 0, 8, 0, -1)
        good, bad = api.Weight(70, 9, 6, 32), api.Weight(1 << 20, 0, 6, 32)
        frame = lambda r0, r1, w0=good, w1=good: L.hmme_predict_bi_w_frame(engine.h, r0.h, r1.h, C.byref(fp8), C.byref(w0), C.byref(w1), field.ctypes.data,
                                                                           dirs.ctypes.data, 64, img.ctypes.data, W)
        # a plane of another size, bit depth or context
        for r0, r1 in ((a, small), (small, a), (a, deep), (a, foreign), (foreign, a)):
            assert frame(r0, r1) == pm.ERR_ARG
        # unequal shifts; an unsupported weight in either list; a shift outside 0..15
        assert frame(a, b, good, api.Weight(35, 9, 5, 16)) == pm.ERR_ARG and b"shifts 6 and 5" in L.hmme_last_error(engine.h)
        assert frame(a, b, bad, good) == pm.ERR_UNSUPPORTED and frame(a, b, good, bad) == pm.ERR_UNSUPPORTED
        assert frame(a, b, api.Weight(1, 0, 16, 0), api.Weight(1, 0, 16, 0)) == pm.ERR_ARG
        with pytest.raises(api.HmmeError):
            engine.predict_bi_w_frame(a, b, (1 << 20, 0, 6, 32), (64, 0, 6, 32), field, dirs, out=img)
        assert (img == 0x5C).all()
        assert frame(a, b) == 0 and (img != 0x5C).any()                         # the accepted neighbour does run
        # the device call: the second picture's weights are refused, the message names it, the first picture's image is untouched
        d_field = torch.zeros((2, 2, 6, 64, 2), dtype=torch.int16, device=dev)
        d_dirs = torch.full((2, 6, 64), 3, dtype=torch.uint8, device=dev)
        imgs = [torch.full((H, W), 0x5C, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        g, bw = (70, 9, 6, 32), (1 << 20, 0, 6, 32)
        for w0s, w1s, code, text in (([g, bw], [g, g], pm.ERR_UNSUPPORTED, "picture 1"), ([g, g], [g, (3, 0, 7, 64)], pm.ERR_ARG, "picture 1"),
                                     ([bw, g], [g, g], pm.ERR_UNSUPPORTED, "picture 0")):
            with pytest.raises(api.HmmeError, match=f"hmme error {code}: .*{text}"):
                engine.predict_bi_w_device([a, a], [b, b], fp8, w0s, w1s, d_field.data_ptr(), d_dirs.data_ptr(), 64, [i.data_ptr() for i in imgs], W, 0)
        torch.cuda.synchronize()
        assert all((i.cpu().numpy() == 0x5C).all() for i in imgs)
        # the argument checks of the unweighted call, unchanged
        one = C.c_void_p(256)     # never dereferenced: refused before anything is launched
        ra = (C.c_void_p * 9)(*([a.h] * 9))
        outs = (C.c_void_p * 9)(*([256] * 9))
        ws = (api.Weight * 9)(*([good] * 9))
        call = lambda n, fp, f=one, d=one, per=64, o=outs, pitch=W, w0=ws, w1=ws: L.hmme_predict_bi_w_device(engine.h, ra, ra, n, C.byref(fp), w0, w1, f, d, per, o, pitch, None)
        ok = api.FrameParams(1, 0, 8, 0, -1)
        assert call(9, ok) == -1 and call(0, ok) == -1 and call(1, ok, per=256) == -1 and call(1, ok, f=None) == -1 and call(1, ok, d=None) == -1
        assert call(1, ok, o=None) == -1 and call(1, ok, pitch=W - 1) == -1 and call(1, ok, w0=None) == -1 and call(1, ok, w1=None) == -1
        assert call(1, api.FrameParams(1, 0, 7, 0, -1)) == -1 and call(1, api.FrameParams(1, 0, 13, 0, -1)) == -1
        assert call(1, api.FrameParams(1, 0, 10, 0, -1)) == -1                  # 8-bit planes, a 10-bit call
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (a, b, small, deep, foreign):
            p.close()
        other_engine.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_fading_three_bands(engine, hmo):
    """the fade of tests/test_predict_bi_w_cpu.py through the whole chain of a WP slice; the prediction is the model's at the device's own
    field, directions and estimated weights"""
    import torch
    from hmme import api, synth
    sr, n = 8, 6
    dev = torch.device("cuda", 0)
    cur_img, ref = pm.fade_pictures(W, H, 8, seed=900 + 8)
    planes = [mkplane(engine, synth.pad_plane(cur_img), W, H, 8)] + [mkplane(engine, r, W, H, 8) for r in ref]
    cur, refs = planes[0], planes[1:]
    try:
        wps, infos = engine.wp_estimate(cur, refs)                              # both lists' references in ONE call: one denominator
        assert wps[0][2] == wps[1][2] and all(i.present for i in infos) and api.predict_bi_weight_check(8, *wps) == 0
        assert all(api.bipred_weight_check(8, wps[l], wps[1 - l], True) == 0 for l in range(2))
        fp, sel, bits = api.FrameParams(sr, 0, 8, 0, n), api.SelectParams(64), sdm.HM_BITS
        tab = lambda: (torch.zeros((2, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((2, n, 593), dtype=torch.int32, device=dev))
        (d_mv, d_sad), (d_q, d_c), (d_bmv, d_bsad), (d_bq, d_bc) = tab(), tab(), tab(), tab()
        d_uni = torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev)
        d_field = torch.full((1, 2, n, 64, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_dir = torch.full((1, n, 64), 0xA7, dtype=torch.uint8, device=dev)
        d_img = torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        curs, others, other_wps = [cur, cur], [refs[1], refs[0]], [wps[1], wps[0]]
        engine.search_pairs_w_device(curs, refs, fp, wps, None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_pairs_w_device(curs, refs, fp, wps, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
        engine.select_pairs_device(W, H, 2, fp, sel, d_q.data_ptr(), d_c.data_ptr(), None, d_uni.data_ptr(), None, None, 0)   # each list on its own tables
        torch.cuda.synchronize()
        d_other = d_uni.flip(0).contiguous()                                    # list l is searched against the origin built from list 1-l's field
        torch.cuda.synchronize()
        engine.search_pairs_bi_w_device(curs, refs, others, fp, wps, other_wps, d_other.data_ptr(), 64, None, None, d_bmv.data_ptr(), d_bsad.data_ptr(), 0)
        engine.refine_pairs_bi_w_device(curs, refs, others, fp, wps, other_wps, d_other.data_ptr(), 64, None, None, d_bmv.data_ptr(), 1, d_bq.data_ptr(), d_bc.data_ptr(), 0)
        engine.select_dirs_device(W, H, 1, fp, sel, [api.DirParams(*bits)], d_q.data_ptr(), d_c.data_ptr(), d_bq.data_ptr(), d_bc.data_ptr(), d_uni.data_ptr(), None,
                                  d_field.data_ptr(), d_dir.data_ptr(), None, None, 0)
        engine.predict_bi_w_device([refs[0]], [refs[1]], fp, [wps[0]], [wps[1]], d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()], W, 0)
        torch.cuda.synchronize()
        field, dirs, pred = d_field.cpu().numpy()[0], d_dir.cpu().numpy()[0], d_img.cpu().numpy()
        counts = np.bincount(dirs.reshape(-1), minlength=256)
        assert counts[3] > 0, counts[:4]                                        # direction 3 occurs
        want = pm.pred_picture(hmo, ref, W, H, 8, field, dirs, wps, np.full((H, W), 0xEE, np.int64))
        assert np.array_equal(pred, want)
        assert np.array_equal(pred, engine.predict_bi_w_frame(refs[0], refs[1], wps[0], wps[1], field, dirs, out=np.full((H, W), 0xEE, np.uint8)))
        # and it is the better prediction: against the same decisions predicted without the weights
        sad = lambda p: int(np.abs(p.astype(np.int64) - cur_img).sum())
        assert sad(pred) < sad(engine.predict_bi_frame(refs[0], refs[1], field, dirs, out=np.full((H, W), 0xEE, np.uint8)))
    finally:
        for p in planes:
            p.close()
