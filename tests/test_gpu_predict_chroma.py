"""4:2:0 chroma motion compensation from the luma motion fields (hmme_predict_chroma_pairs / _refs / _bi, device and _frame forms) against
tests/predict_chroma_model.py -- TComPrediction::xPredInterBlk for a chroma component restated in numpy and pinned to the reference's compiled
filters by tests/test_predict_chroma_cpu.py.  Cb and Cr always hold different content, every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
import predict_bi_w_model as pbw
import predict_chroma_model as cm
import range_content as rc
import select_dirs_model as sdm
from frame_helpers import bind_hmo, dims, mkplane

pytestmark = pytest.mark.gpu

W, H = 136, 72                                                # 3 x 2 luma CTUs, the right column and the bottom row partial
SIZES = ((64, 64), (100, 70), (136, 72))                      # one CTU; 2 x 2 with both edges partial and a half-width last chroma block; 3 x 2
# per component (Cb, Cr), per list (0, 1): (w0, offset in 8-bit units, shift).  The two lists of a component share the shift, Cb and Cr do not
WEIGHT_SETS = {"hm_like": (((70, 9, 6), (55, -14, 6)), ((40, -5, 5), (29, 11, 5))),
               "negative": (((-37, 150, 5), (90, -3, 5)), ((61, 4, 6), (-20, 170, 6))),
               "shift_15": (((30000, 2, 15), (15000, -1, 15)), ((70, 9, 6), (55, -14, 6)))}
ERR_ARG, ERR_UNSUPPORTED = pbw.ERR_ARG, pbw.ERR_UNSUPPORTED
CORNERS = ((-704, -656), (704, -656), (-704, 656), (704, 656))   # quarter pels, whole chroma samples: beyond TComDataCU::clipMv's range at every corner


def wset(name, bd):
    """wps[component] = (weight of list 0, of list 1) at a bit depth: offsets scale with the depth, round is not used"""
    return tuple(tuple((w, o * (1 << (bd - 8)), d, 1 << (d - 1)) for w, o, d in comp) for comp in WEIGHT_SETS[name])


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


def fills(w, h, bd, dtype=None):
    dt, fill = sentinel(bd)
    return tuple(np.full((h // 2, w // 2), fill, dtype or dt) for _ in range(2))


class Chroma:
    """n pictures' Cb and Cr of a w x h LUMA picture: unrelated textures, as padded arrays (model) and as planes (engine)"""

    def __init__(self, engine, w, h, bd, seed, n=2, arrays=None):
        from hmme import synth
        self.w, self.h, self.bd = w, h, bd
        self.arrays = arrays or [[synth.make_pair(w // 2, h // 2, seed=seed + 7 * k + 3 * c, bit_depth=bd, max_mv=2)[1] for c in range(2)] for k in range(n)]
        self.planes = [[mkplane(engine, a, w // 2, h // 2, bd) for a in pic] for pic in self.arrays]

    def comps(self, pics):
        """model order: [component][picture]"""
        return [[self.arrays[k][c] for k in pics] for c in range(2)]

    def flat(self, pics):
        """engine order: [cb, cr] of each picture in turn"""
        return [p for k in pics for p in self.planes[k]]

    def close(self):
        for pic in self.planes:
            for p in pic:
                p.close()


def in_picture(w, h):
    cx_n, cy_n = dims(w, h)
    return [(c, b) for c in range(cx_n * cy_n) for b in range(64) if (c % cx_n) * 64 + (b % 8) * 8 < w and (c // cx_n) * 64 + (b // 8) * 8 < h]


def make_field(w, h, per, seed, rot=0):
    """int16[n, per, 2] quarter-pel luma MVs.  One per 8x8 block: block number j inside the picture takes the phase pair (j + rot) % 64 --
    neighbours of one wave differ in phase, all 64 occur --, whole displacements of up to 50 luma pels of either sign, and the four corners
    of the picture carry MVs beyond the clip range.  One per CTU: random, CTU 0 beyond the range"""
    cx_n, cy_n = dims(w, h)
    n = cx_n * cy_n
    rng = np.random.default_rng(seed)
    field = (8 * rng.integers(-25, 26, size=(n, per, 2))).astype(np.int16)
    if per == 1:
        field += rng.integers(0, 8, size=(n, 1, 2)).astype(np.int16)
        field[0, 0] = CORNERS[seed % 4]
        return field
    inside = in_picture(w, h)
    for j, (c, b) in enumerate(inside):
        p = (j + rot) % 64
        field[c, b] += (p & 7, p >> 3)
    xs = [(c % cx_n) * 64 + (b % 8) * 8 for c, b in inside]
    ys = [(c // cx_n) * 64 + (b // 8) * 8 for c, b in inside]
    for (mx, my), want_x, want_y in zip(CORNERS, (min(xs), max(xs), min(xs), max(xs)), (min(ys), min(ys), max(ys), max(ys))):
        c, b = next(cb for cb, x, y in zip(inside, xs, ys) if (x, y) == (want_x, want_y))
        field[c, b] = (mx + (int(field[c, b, 0]) & 7), my + (int(field[c, b, 1]) & 7))
    return field


def phases(w, h, field):
    return {(int(field[c, b, 0]) & 7, int(field[c, b, 1]) & 7) for c, b in in_picture(w, h)}


def make_dirs(w, h, per, seed):
    cx_n, cy_n = dims(w, h)
    n = cx_n * cy_n
    if per == 1:
        return np.array([3, 1, 2, 0xFF, 3, 3][:n], np.uint8).reshape(n, 1)
    rng = np.random.default_rng(seed)
    dirs = rng.choice(np.array([1, 2, 3, 3, 0xFF, 0, 4], np.uint8), size=(n, per))
    dirs[0, :2], dirs[0, 8:12] = (1, 2), (0xFF, 4, 0, 3)          # every kind inside the picture, whatever was drawn
    return dirs


def block_mask(w, h, values, per, want):
    """boolean [h / 2, w / 2]: the chroma samples of the blocks whose entry of `values` is in `want`"""
    cx_n, cy_n = dims(w, h)
    g = 32 if per == 1 else 4
    mask = np.zeros((cy_n * 32, cx_n * 32), bool)
    for c in range(cx_n * cy_n):
        for b in range(per):
            if int(values[c, b]) in want:
                x0, y0 = (c % cx_n) * 32 + (b % 8) * g, (c // cx_n) * 32 + (b // 8) * g
                mask[y0:y0 + g, x0:x0 + g] = True
    return mask[:h // 2, :w // 2]


def same(got, want, what):
    for c in range(2):
        assert np.array_equal(got[c], want[c]), (what, "Cb" if c == 0 else "Cr", np.argwhere(got[c] != want[c])[:4])


def check_bi(engine, hmo, ch, field, dirs, wps=None, pics=(0, 1)):
    """one picture of the bi form against the model; its uni blocks against the pairs form; its dead blocks against the sentinel"""
    w, h, bd, per = ch.w, ch.h, ch.bd, dirs.shape[1]
    w0, w1 = (None, None) if wps is None else ([wps[0][0], wps[1][0]], [wps[0][1], wps[1][1]])
    got = engine.predict_chroma_bi_frame(ch.planes[pics[0]], ch.planes[pics[1]], w, h, field, dirs, outs=fills(w, h, bd), weights0=w0, weights1=w1)
    want = cm.bi_picture(hmo, ch.comps(pics), w, h, bd, field, dirs, fills(w, h, bd, np.int64), wps)
    same(got, want, ("bi", w, h, bd, per, wps))
    for l, wl in ((0, w0), (1, w1)):
        m = block_mask(w, h, dirs, per, {l + 1})
        if m.any():
            uni = engine.predict_chroma_frame(ch.planes[pics[l]], w, h, field[l], weights=wl)
            assert all(np.array_equal(got[c][m], uni[c][m]) for c in range(2))
    dead = block_mask(w, h, dirs, per, {0, 4, 0xFF})
    assert all((got[c][dead] == sentinel(bd)[1]).all() for c in range(2))
    return got


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", SIZES)
def test_one_reference_every_phase_and_beyond_the_clip_range(engine, hmo, size, bd, per):
    w, h = size
    ch = Chroma(engine, w, h, bd, seed=2100 + bd + w, n=1)
    try:
        field = make_field(w, h, per, 2101 + bd + w)
        if per == 64:
            assert len(phases(w, h, field)) == 64 and (field < 0).any()
            assert sum(1 for c, b in in_picture(w, h) if abs(int(field[c, b, 0])) > 4 * (64 + 8) and abs(int(field[c, b, 1])) > 4 * (64 + 8)) >= (4 if w > 64 else 1)
        got = engine.predict_chroma_frame(ch.planes[0], w, h, field, outs=fills(w, h, bd))
        want = cm.pairs_picture(hmo, ch.arrays[0], w, h, bd, field, fills(w, h, bd, np.int64))
        same(got, want, ("pairs", w, h, bd, per))
        assert all((g != sentinel(bd)[1]).any() for g in got) and not np.array_equal(got[0], got[1])
        swapped = cm.pairs_picture(hmo, ch.arrays[0][::-1], w, h, bd, field, fills(w, h, bd, np.int64))
        assert not np.array_equal(got[0], swapped[0])                           # a swapped component would show
    finally:
        ch.close()


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", SIZES)
def test_directions_and_sentinels(engine, hmo, size, bd, per):
    w, h = size
    ch = Chroma(engine, w, h, bd, seed=2200 + bd + w)
    try:
        field = np.stack([make_field(w, h, per, 2201 + bd + w + 50 * l, rot=23 * l) for l in range(2)])
        dirs = make_dirs(w, h, per, 2203 + bd + w)
        check_bi(engine, hmo, ch, field, dirs)
        n = dirs.shape[0]
        assert block_mask(w, h, dirs, per, {3}).any() and (block_mask(w, h, dirs, per, {0, 4, 0xFF}).any() or (per == 1 and n < 4))
    finally:
        ch.close()


def test_direction_three_at_all_phase_pairs_of_both_lists(engine, hmo):
    """every block bi: 64 pictures, list 1's phase pairs rotated one step further against list 0's in each -- every one of the 64 x 64
    combinations of the two lists' phase pairs occurs"""
    ch = Chroma(engine, W, H, 8, seed=2300)
    try:
        seen = set()
        dirs = np.full((6, 64), 3, np.uint8)
        for rnd in range(64):
            field = np.stack([make_field(W, H, 64, 2301 + rnd, rot=0), make_field(W, H, 64, 2401 + rnd, rot=rnd)])
            seen |= {tuple(int(v) & 7 for v in (*field[0, c, b], *field[1, c, b])) for c, b in in_picture(W, H)}
            check_bi(engine, hmo, ch, field, dirs)
        assert len(seen) == 4096, len(seen)
    finally:
        ch.close()


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", [8, 10])
def test_four_references_block_by_block(engine, hmo, bd, per):
    ch = Chroma(engine, W, H, bd, seed=2400 + bd, n=4)
    try:
        pics = (0, 1, 2, 3)
        field = make_field(W, H, per, 2401 + bd + per)
        rng = np.random.default_rng(2402 + bd)
        ref_field = rng.choice(np.array([0, 1, 2, 3, 4, 9, 0xFF], np.uint8), size=field.shape[:2]) if per == 64 else np.array([3, 0, 0xFF, 1, 2, 4], np.uint8).reshape(6, 1)
        wps = [[(64 + 5 * r + 3 * c, (r - c) * (1 << (bd - 8)), 6, 32) for r in pics] for c in range(2)]
        flat_w = [wps[c][r] for r in pics for c in range(2)]
        for weights, model_w in ((None, None), (flat_w, wps)):
            got = engine.predict_chroma_refs_frame(ch.flat(pics), W, H, field, ref_field, outs=fills(W, H, bd), weights=weights)
            want = cm.refs_picture(hmo, ch.comps(pics), W, H, bd, field, ref_field, fills(W, H, bd, np.int64), model_w)
            same(got, want, ("refs", bd, per, weights is not None))
            for r in pics:                                                       # block by block the uni call of that reference
                m = block_mask(W, H, ref_field, per, {r})
                uni = engine.predict_chroma_frame(ch.planes[r], W, H, field, weights=None if weights is None else [wps[0][r], wps[1][r]])
                assert m.any() and all(np.array_equal(got[c][m], uni[c][m]) for c in range(2))
            dead = block_mask(W, H, ref_field, per, {4, 9, 0xFF})
            assert dead.any() and all((got[c][dead] == sentinel(bd)[1]).all() for c in range(2))
    finally:
        ch.close()


def test_twelve_bits_where_the_head_room_clamps_at_two(engine, hmo):
    bd = 12
    ch = Chroma(engine, W, H, bd, seed=2500)
    try:
        field = np.stack([make_field(W, H, 64, 2501 + l, rot=29 * l) for l in range(2)])
        dirs = make_dirs(W, H, 64, 2503)
        check_bi(engine, hmo, ch, field, dirs)
        check_bi(engine, hmo, ch, field, dirs, wset("hm_like", bd))
        ref_field = (dirs & 1).astype(np.uint8)
        got = engine.predict_chroma_refs_frame(ch.flat((0, 1)), W, H, field[0], ref_field, outs=fills(W, H, bd))
        same(got, cm.refs_picture(hmo, ch.comps((0, 1)), W, H, bd, field[0], ref_field, fills(W, H, bd, np.int64)), "refs at 12 bits")
    finally:
        ch.close()


@pytest.mark.parametrize("name", list(WEIGHT_SETS))
@pytest.mark.parametrize("bd", [8, 10])
def test_weights_per_component(engine, hmo, bd, name):
    from hmme import api
    wps = wset(name, bd)
    assert all(api.predict_bi_weight_check(bd, *wps[c]) == 0 for c in range(2)) and wps[0] != wps[1]
    ch = Chroma(engine, W, H, bd, seed=2600 + bd)
    try:
        field = np.stack([make_field(W, H, 64, 2601 + bd + l, rot=17 * l) for l in range(2)])
        dirs = make_dirs(W, H, 64, 2603 + bd)
        got = check_bi(engine, hmo, ch, field, dirs, wps)                       # uni blocks: the pairs form with that list's weights, inside
        plain = engine.predict_chroma_bi_frame(ch.planes[0], ch.planes[1], W, H, field, dirs, outs=fills(W, H, bd))
        live = block_mask(W, H, dirs, 64, {1, 2, 3})
        assert all(not np.array_equal(got[c][live], plain[c][live]) for c in range(2))   # the weights act on both components
        # the pairs form on its own against the model, Cb and Cr weighted differently
        w_l0 = [wps[0][0], wps[1][0]]
        uni = engine.predict_chroma_frame(ch.planes[0], W, H, field[0], outs=fills(W, H, bd), weights=w_l0)
        same(uni, cm.pairs_picture(hmo, ch.arrays[0], W, H, bd, field[0], fills(W, H, bd, np.int64), w_l0), ("pairs_w", bd, name))
        # one mv per CTU
        f1 = np.stack([make_field(W, H, 1, 2605 + bd + l) for l in range(2)])
        check_bi(engine, hmo, ch, f1, make_dirs(W, H, 1, 0), wps)
    finally:
        ch.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_identities_run_the_unweighted_call(engine, hmo, bd):
    ch = Chroma(engine, W, H, bd, seed=2700 + bd)
    try:
        field = np.stack([make_field(W, H, 64, 2701 + bd + l, rot=11 * l) for l in range(2)])
        dirs = make_dirs(W, H, 64, 2703 + bd)
        ref_field = (dirs & 1).astype(np.uint8)
        plain_bi = engine.predict_chroma_bi_frame(ch.planes[0], ch.planes[1], W, H, field, dirs, outs=fills(W, H, bd))
        plain_uni = engine.predict_chroma_frame(ch.planes[0], W, H, field[0])
        plain_refs = engine.predict_chroma_refs_frame(ch.flat((0, 1)), W, H, field[0], ref_field, outs=fills(W, H, bd))
        for (da, ra), (db, rb) in (((0, 0), (0, 0)), ((6, 32), (7, 64)), ((6, 5), (14, 1 << 13)), ((13, 0), (3, 1))):   # Cb's and Cr's shift and round
            ia, ib = (1 << da, 0, da, ra), (1 << db, 0, db, rb)
            same(engine.predict_chroma_bi_frame(ch.planes[0], ch.planes[1], W, H, field, dirs, outs=fills(W, H, bd), weights0=[ia, ib], weights1=[ia, ib]), plain_bi, (da, db))
            same(engine.predict_chroma_frame(ch.planes[0], W, H, field[0], weights=[ia, ib]), plain_uni, (da, db))
            same(engine.predict_chroma_refs_frame(ch.flat((0, 1)), W, H, field[0], ref_field, outs=fills(W, H, bd), weights=[ia, ib, ib, ia]), plain_refs, (da, db))
        # Cb the identity, Cr not: the weighted kernel serves both, Cb comes out as without weights
        wps = (((64, 0, 6, 32), (64, 0, 6, 32)), wset("hm_like", bd)[1])
        got = check_bi(engine, hmo, ch, field, dirs, wps)
        assert np.array_equal(got[0], plain_bi[0]) and not np.array_equal(got[1], plain_bi[1])
    finally:
        ch.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_last_accepted_weights_on_extreme_content(engine, hmo, bd):
    """the weights next to a refusal on chroma planes of samples in {0, maxv}: the int32 numerators at their bound"""
    from hmme import api
    w, h = 272, 72                                                              # range_content's layout needs chroma planes three CTUs wide
    trip = [rc.extreme_triple(w // 2, h // 2, bd, seed=2800 + bd + 5 * c) for c in range(2)]
    arrays = [[trip[c][1 + k] for c in range(2)] for k in range(2)]               # picture k: (Cb, Cr) = ref / other of the component's triple
    ch = Chroma(engine, w, h, bd, seed=0, arrays=arrays)
    try:
        field = np.stack([make_field(w, h, 64, 2801 + bd + l, rot=13 * l) for l in range(2)])
        field = (field // 16).astype(np.int16)                                  # fractional MVs of a few pels: the patterns, not the flat border
        dirs = make_dirs(w, h, 64, 2803 + bd)
        dirs[dirs > 3] = 3
        cases = []
        for name, member in rc.families(bd).items():
            other = pbw.ident(member(0)[2])
            cases.append((bwm.last_accepted(member, lambda w: api.predict_bi_weight_check(bd, w, other))[1], other))
        both = bwm.last_accepted(lambda k: (1 + k, 0, 0, 0), lambda w: api.predict_bi_weight_check(bd, w, w))[1]
        cases += [(both, both), (cases[0][1], cases[0][0])]
        reach = 0
        for k, pair in enumerate(cases):
            wps = (pair, cases[(k + 1) % len(cases)])                           # Cb and Cr at different bounds
            assert all(api.predict_bi_weight_check(bd, *p) == 0 for p in wps)
            reach = max(reach, pbw.pair_reach(bd, *pair))
            check_bi(engine, hmo, ch, field, dirs, wps)
        assert reach > pbw.INT32_MAX - 2 * pbw.PEL_REACH
    finally:
        ch.close()


def test_two_pictures_per_launch_into_strided_images_over_a_ctu_sub_range(engine, hmo):
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    ch = Chroma(engine, W, H, 8, seed=2900, n=4)                              # picture 0: lists (0, 1); picture 1: lists (2, 3)
    try:
        cw, chh, pitch = W // 2, H // 2, W // 2 + 24
        fields = [np.stack([make_field(W, H, 64, 2901 + 10 * i + l, rot=9 * l + i) for l in range(2)]) for i in range(2)]
        dirs = [make_dirs(W, H, 64, 2903 + i) for i in range(2)]
        wps = [wset("hm_like", 8), wset("negative", 8)]
        fp = api.FrameParams(1, 0, 8, 1, 4)                                     # luma CTUs 1..4 of both pictures
        new = lambda k: [torch.full((chh, pitch), 0xA5, dtype=torch.uint8, device=dev) for _ in range(k)]
        inside = np.zeros((chh, cw), bool)
        inside[:32, 32:] = True
        inside[32:, :64] = True

        def check(imgs, want, what):
            for got, exp in zip(imgs, want):
                got = got.cpu().numpy()
                assert np.array_equal(got[:, :cw], exp), what
                assert (got[:, cw:] == 0xA5).all() and (got[:, :cw][~inside] == 0xA5).all() and (got[:, :cw][inside] != 0xA5).any()

        # bi, weighted and not
        d_field = torch.from_numpy(np.stack(fields)).to(dev)
        d_dirs = torch.from_numpy(np.stack(dirs)).to(dev)
        for weighted in (False, True):
            imgs = new(4)
            torch.cuda.synchronize()
            w0 = [wps[i][c][0] for i in range(2) for c in range(2)] if weighted else None
            w1 = [wps[i][c][1] for i in range(2) for c in range(2)] if weighted else None
            engine.predict_chroma_bi_device(ch.flat((0, 2)), ch.flat((1, 3)), W, H, fp, d_field.data_ptr(), d_dirs.data_ptr(), 64, [i.data_ptr() for i in imgs],
                                            pitch, weights0=w0, weights1=w1)
            torch.cuda.synchronize()
            want = [o for i in range(2) for o in cm.bi_picture(hmo, ch.comps((2 * i, 2 * i + 1)), W, H, 8, fields[i], dirs[i], fills(W, H, 8, np.int64),
                                                                wps[i] if weighted else None, ctus=range(1, 5))]
            check(imgs, want, ("bi", weighted))
        # pairs: two pictures, each with its own field
        d_uni = torch.from_numpy(np.stack([fields[0][0], fields[1][0]])).to(dev)
        imgs = new(4)
        torch.cuda.synchronize()
        engine.predict_chroma_pairs_device(ch.flat((0, 2)), W, H, fp, d_uni.data_ptr(), 64, [i.data_ptr() for i in imgs], pitch)
        torch.cuda.synchronize()
        want = [o for i in range(2) for o in cm.pairs_picture(hmo, ch.arrays[2 * i], W, H, 8, fields[i][0], fills(W, H, 8, np.int64), ctus=range(1, 5))]
        check(imgs, want, "pairs")
        # refs: one picture from four references
        ref_field = (dirs[0] & 3).astype(np.uint8)
        d_ref = torch.from_numpy(ref_field).to(dev)
        imgs = new(2)
        torch.cuda.synchronize()
        engine.predict_chroma_refs_device(ch.flat((0, 1, 2, 3)), W, H, fp, d_uni.data_ptr(), d_ref.data_ptr(), 64, imgs[0].data_ptr(), imgs[1].data_ptr(), pitch)
        torch.cuda.synchronize()
        check(imgs, cm.refs_picture(hmo, ch.comps((0, 1, 2, 3)), W, H, 8, fields[0][0], ref_field, fills(W, H, 8, np.int64), ctus=range(1, 5)), "refs")
    finally:
        ch.close()


def test_refusals_launch_and_write_nothing(engine):
    from hmme import api
    L = api.load()
    other_engine = api.Engine(0, 64)
    cw, chh = W // 2, H // 2
    cb, cr, cb1, cr1 = (engine.plane(cw, chh) for _ in range(4))
    small, luma_sized, deep, foreign = engine.plane(32, 32), engine.plane(W, H), engine.plane(cw, chh, 10), other_engine.plane(cw, chh)
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        field, dirs = np.zeros((2, 6, 64, 2), np.int16), np.full((6, 64), 3, np.uint8)
        refs0 = np.zeros((6, 64), np.uint8)
        imgs = [np.full((chh, cw), 0x5C, np.uint8) for _ in range(2)]
        outs = (C.c_void_p * 2)(*[i.ctypes.data for i in imgs])
        fp8 = api.FrameParams(1, 0, 8, 0, -1)
        hs = lambda *planes: (C.c_void_p * len(planes))(*[p.h for p in planes])
        wa = lambda *ws: (api.Weight * len(ws))(*[api.Weight(*w) for w in ws])
        good, shift5, huge = (70, 9, 6, 32), (35, 9, 5, 16), (1 << 20, 0, 6, 32)

        def pairs(planes=(cb, cr), w=W, h=H, fp=fp8, wp=None, per=64):
            return L.hmme_predict_chroma_frame(engine.h, hs(*planes), w, h, C.byref(fp), wp, field.ctypes.data, per, outs, cw)

        def refs(planes=(cb, cr, cb1, cr1), w=W, h=H, fp=fp8, wp=None):
            return L.hmme_predict_chroma_refs_frame(engine.h, hs(*planes), len(planes) // 2, w, h, C.byref(fp), wp, field.ctypes.data, refs0.ctypes.data, 64, outs, cw)

        def bi(l0=(cb, cr), l1=(cb1, cr1), w=W, h=H, fp=fp8, w0=None, w1=None):
            return L.hmme_predict_chroma_bi_frame(engine.h, hs(*l0), hs(*l1), w, h, C.byref(fp), w0, w1, field.ctypes.data, dirs.ctypes.data, 64, outs, cw)

        def refused(rc, code, entry):
            assert rc == code and entry.encode() in L.hmme_last_error(engine.h), (rc, L.hmme_last_error(engine.h))

        # an odd luma width or height
        for call, entry in ((pairs, "hmme_predict_chroma_frame"), (refs, "hmme_predict_chroma_refs_frame"), (bi, "hmme_predict_chroma_bi_frame")):
            refused(call(w=W + 1), ERR_ARG, entry)
            refused(call(h=H - 1), ERR_ARG, entry)
            refused(call(w=W + 2), ERR_ARG, entry)                              # even, but the planes are not half of it
        # a plane whose size is not (W / 2, H / 2); Cb / Cr or lists of another bit depth; a plane of another context
        for bad in (small, luma_sized, deep, foreign):
            refused(pairs((cb, bad)), ERR_ARG, "hmme_predict_chroma_frame")
            refused(pairs((bad, cr)), ERR_ARG, "hmme_predict_chroma_frame")
            refused(refs((cb, cr, cb1, bad)), ERR_ARG, "hmme_predict_chroma_refs_frame")
            refused(bi(l1=(cb1, bad)), ERR_ARG, "hmme_predict_chroma_bi_frame")
            refused(bi(l0=(cb, bad)), ERR_ARG, "hmme_predict_chroma_bi_frame")
        refused(pairs(fp=api.FrameParams(1, 0, 10, 0, -1)), ERR_ARG, "hmme_predict_chroma_frame")     # 8-bit planes, a 10-bit call
        # the CTU range is the luma picture's; MVs per CTU
        refused(pairs(fp=api.FrameParams(1, 0, 8, 0, 7)), ERR_ARG, "hmme_predict_chroma_frame")
        refused(pairs(per=256), ERR_ARG, "hmme_predict_chroma_frame")
        # weights: unequal shifts of the two lists within a component; an unsupported weight; one list's weights missing
        refused(bi(w0=wa(good, good), w1=wa(good, shift5)), ERR_ARG, "hmme_predict_chroma_bi_frame")
        assert b"shifts 6 and 5" in L.hmme_last_error(engine.h)
        refused(bi(w0=wa(good, good), w1=None), ERR_ARG, "hmme_predict_chroma_bi_frame")
        refused(bi(w0=wa(huge, good), w1=wa(good, good)), ERR_UNSUPPORTED, "hmme_predict_chroma_bi_frame")
        refused(pairs(wp=wa(good, huge)), ERR_UNSUPPORTED, "hmme_predict_chroma_frame")
        refused(pairs(wp=wa(good, (1, 0, 16, 0))), ERR_ARG, "hmme_predict_chroma_frame")
        refused(refs(wp=wa(good, good, good, huge)), ERR_UNSUPPORTED, "hmme_predict_chroma_refs_frame")
        assert all((i == 0x5C).all() for i in imgs)
        # the accepted neighbours do run: Cb and Cr of different shift
        assert bi(w0=wa(good, shift5), w1=wa(good, shift5)) == 0 and all((i != 0x5C).any() for i in imgs)
        assert pairs() == 0 and refs() == 0 and bi() == 0
        # the device calls: more planes than a launch takes, null arguments, a pitch below a chroma row
        one = C.c_void_p(256)     # never dereferenced: refused before anything is launched
        many = (C.c_void_p * 20)(*([cb.h] * 20))
        o20 = (C.c_void_p * 20)(*([256] * 20))
        dp = lambda n, f=one, o=o20, pitch=cw: L.hmme_predict_chroma_pairs_device(engine.h, many, n, W, H, C.byref(fp8), None, f, 64, o, pitch, None)
        dr = lambda n, f=one, r=one, o=one, pitch=cw: L.hmme_predict_chroma_refs_device(engine.h, many, n, W, H, C.byref(fp8), None, f, r, 64, o, o, pitch, None)
        db = lambda n, f=one, d=one, o=o20, pitch=cw: L.hmme_predict_chroma_bi_device(engine.h, many, many, n, W, H, C.byref(fp8), None, None, f, d, 64, o, pitch, None)
        assert dp(9) == dp(0) == dp(1, f=None) == dp(1, o=None) == dp(1, pitch=cw - 1) == ERR_ARG
        assert dr(9) == dr(0) == dr(1, f=None) == dr(1, r=None) == dr(1, o=None) == dr(1, pitch=cw - 1) == ERR_ARG
        assert db(5) == db(0) == db(1, f=None) == db(1, d=None) == db(1, o=None) == db(1, pitch=cw - 1) == ERR_ARG
        assert b"hmme_predict_chroma_bi_device" in L.hmme_last_error(engine.h)
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (cb, cr, cb1, cr1, small, luma_sized, deep, foreign):
            p.close()
        other_engine.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_three_bands_with_chroma(engine, hmo):
    """the three-band picture of tests/test_gpu_predict_bi.py with chroma that moves with it: the whole chain on luma, then the chroma
    prediction from the device's own field and directions"""
    import torch
    from hmme import api, synth
    sr, m, n = 8, synth.MARGIN, 6
    dev = torch.device("cuda", 0)
    ref = [synth.make_pair(W, H, seed=900 + 7 * k, bit_depth=8, max_mv=2)[1] for k in range(2)]
    mvs = ((3, -2), (-2, 1))                                                    # full luma pels: list 0 and list 1
    moved = [r[m + dy:m + dy + H, m + dx:m + dx + W].astype(np.int32) for r, (dx, dy) in zip(ref, mvs)]
    cur_img = moved[0].copy()
    cur_img[:, 48:96] = (moved[0][:, 48:96] + moved[1][:, 48:96] + 1) >> 1
    cur_img[:, 96:] = moved[1][:, 96:]
    ch = Chroma(engine, W, H, 8, seed=2950)
    # the true chroma: every block predicted by the model at the true motion (a chroma displacement of (1.5, -1) and (-1, 0.5)) and direction
    true_field, true_dirs = pbw.fade_truth(W, H)
    assert pbw.FADE_MV == mvs and pbw.FADE_BANDS == (48, 96)
    true_c = cm.bi_picture(hmo, ch.comps((0, 1)), W, H, 8, true_field, true_dirs, fills(W, H, 8, np.int64))
    planes = [mkplane(engine, synth.pad_plane(cur_img), W, H, 8)] + [mkplane(engine, r, W, H, 8) for r in ref]
    cur, refs = planes[0], planes[1:]
    try:
        fp, sel, bits = api.FrameParams(sr, 1, 8, 0, n), api.SelectParams(64), sdm.HM_BITS
        tab = lambda: (torch.zeros((2, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((2, n, 593), dtype=torch.int32, device=dev))
        (d_mv, d_sad), (d_q, d_c), (d_bmv, d_bsad), (d_bq, d_bc) = tab(), tab(), tab(), tab()
        d_uni = torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev)
        d_field = torch.full((1, 2, n, 64, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_dir = torch.full((1, n, 64), 0xA7, dtype=torch.uint8, device=dev)
        d_img = torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev)
        d_c_imgs = [torch.full((H // 2, W // 2), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        curs, others = [cur, cur], [refs[1], refs[0]]
        engine.search_pairs_device(curs, refs, fp, None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_pairs_device(curs, refs, fp, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
        engine.select_pairs_device(W, H, 2, fp, sel, d_q.data_ptr(), d_c.data_ptr(), None, d_uni.data_ptr(), None, None, 0)
        torch.cuda.synchronize()
        d_other = d_uni.flip(0).contiguous()                                    # list l is searched against the origin built from list 1-l's field
        torch.cuda.synchronize()
        engine.search_pairs_bi_device(curs, refs, others, fp, d_other.data_ptr(), 64, None, None, d_bmv.data_ptr(), d_bsad.data_ptr(), 0)
        engine.refine_pairs_bi_device(curs, refs, others, fp, d_other.data_ptr(), 64, None, None, d_bmv.data_ptr(), 1, d_bq.data_ptr(), d_bc.data_ptr(), 0)
        engine.select_dirs_device(W, H, 1, fp, sel, [api.DirParams(*bits)], d_q.data_ptr(), d_c.data_ptr(), d_bq.data_ptr(), d_bc.data_ptr(), d_uni.data_ptr(), None,
                                  d_field.data_ptr(), d_dir.data_ptr(), None, None, 0)
        engine.predict_bi_device([refs[0]], [refs[1]], fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()], W, 0)
        engine.predict_chroma_bi_device(ch.planes[0], ch.planes[1], W, H, fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [i.data_ptr() for i in d_c_imgs], W // 2)
        torch.cuda.synchronize()
        field, dirs = d_field.cpu().numpy()[0], d_dir.cpu().numpy()[0]
        assert np.bincount(dirs.reshape(-1), minlength=4)[3] > 0                # direction 3 occurs
        got = [i.cpu().numpy() for i in d_c_imgs]
        want = cm.bi_picture(hmo, ch.comps((0, 1)), W, H, 8, field, dirs, tuple(np.full((H // 2, W // 2), 0xEE, np.int64) for _ in range(2)))
        same(got, want, "end to end")
        still = engine.predict_chroma_bi_frame(ch.planes[0], ch.planes[1], W, H, np.zeros_like(field), dirs)
        for c in range(2):
            sad = lambda p: int(np.abs(p.astype(np.int64) - true_c[c]).sum())
            assert sad(got[c]) < sad(still[c]), (c, sad(got[c]), sad(still[c]))
    finally:
        ch.close()
        for p in planes:
            p.close()
