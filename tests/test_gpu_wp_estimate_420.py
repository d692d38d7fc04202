"""hmme_wp_estimate_420 on the device against the numpy restatement of HM's joint estimator (tests/wp_estimate_420_model.py): every field of
every hmme_wp_info and every hmme_weight bit for bit.  Each case first asserts ON THE MODEL that its input does what the case is about."""
import ctypes as C
import math

import numpy as np
import pytest

import wp_estimate_420_model as model
import wp_estimate_model as luma_model
from test_gpu_wp_estimate import fade, make_plane, noise, smooth, upload

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(57.9)
    yield e
    e.close()


class Planes:
    """planes of the arrays of a case: the same array given twice is the same plane given twice"""

    def __init__(self, engine, bd):
        self.engine, self.bd, self.by_id = engine, bd, {}

    def __call__(self, img):
        if id(img) not in self.by_id:
            self.by_id[id(img)] = (make_plane(self.engine, img, self.bd), img)     # the array is kept: its id stays its own
        return self.by_id[id(img)][0]

    def triple(self, pic3):
        return [self(p) for p in pic3]

    def close(self):
        for p, _ in self.by_id.values():
            p.close()


def compare(got, want, bd):
    """(luma weights, chroma weights, infos) of the device against the model's entries"""
    from hmme import api
    wl, wc, infos = got
    assert len(wl) == len(want) and len(wc) == 2 * len(want) and len(infos) == 3 * len(want)
    for r, entries in enumerate(want):
        for c, e in enumerate(entries):
            info = infos[3 * r + c].as_dict()
            assert {k: info[k] for k in luma_model.INFO_FIELDS} == {k: e[k] for k in luma_model.INFO_FIELDS}, (r, c, info, e)
            w = wl[r] if c == 0 else wc[2 * r + c - 1]
            assert tuple(w) == e["wp"], (r, c, w, e["wp"])
            if c == 0:
                assert info["served_search"] == int(api.weight_check(bd, e["wp"], False) == 0)
                assert info["served_refine"] == int(api.weight_check(bd, e["wp"], True) == 0)
            else:
                # an estimated weight is at most 15 << 7 = 1920 at a shift of at most 7: 1920 * 40960 + 2^12 is far inside 32 bits, which is
                # all the chroma prediction calls ask of a component's weight (test_estimated_weights_serve_... hands them over)
                assert 0 <= e["wp"][0] <= 1920 and (info["served_search"], info["served_refine"]) == (1, 1)


def check(engine, cur3, refs3, bd, start=6):
    """one device call against the model, everything compared; -> the model's entries"""
    planes = Planes(engine, bd)
    try:
        got = engine.wp_estimate_420(planes.triple(cur3), [planes.triple(r) for r in refs3], start)
    finally:
        planes.close()
    want = model.estimate(cur3, refs3, bd, start)
    compare(got, want, bd)
    return want


def picture(w, h, bd, seed, kind=noise):
    return tuple(kind(ww, hh, bd, seed + 17 * c) for c, (ww, hh) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2))))


def faded(pic3, a, b, bd):
    return tuple(fade(p, a, b, bd) for p in pic3)


def mirrored(pic3):
    """the picture flipped left to right: every sum of hmme_plane_stats is that of the picture itself, so the estimate is weight 1 << d, offset 0,
    the two SADs are equal and the ratio is exactly 1 -- not present"""
    return tuple(np.ascontiguousarray(p[:, ::-1]) for p in pic3)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------

# luma sizes: 16 x 16 -- a chroma row is half a vector (u8); 32 x 16; 48 x 18 -- chroma 24 x 9, one and a half vectors, odd height; 130 x 66 -- chroma
# 65 x 33; 8200 x 16 -- more vectors per row than lanes in luma and, by one, in chroma (u8: 513 and 257), lpr differing between the planes
GEOMETRY = [(16, 16), (32, 16), (48, 18), (130, 66), (8200, 16)]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h", GEOMETRY)
def test_geometry(engine, w, h, bd):
    ref0 = picture(w, h, bd, seed=w + h + bd)
    cur = faded(ref0, 0.75, 12, bd)
    ref1 = mirrored(cur)
    es = check(engine, cur, [ref0, ref1], bd)
    assert all(e["cur_ac"] > 0 and e["ref_ac"] > 0 and e["sad_nowp"] > 0 for r in es for e in r)
    assert [es[0][0]["present"], es[1][0]["present"]] == [1, 0]                 # the fade is found, the mirrored picture is not
    assert all(e["weight"] != 1 << e["log2_denom"] for e in es[0])              # ... in all three components


# ---- joint behaviour -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [1, 2, 3])
def test_hand_checkable_cases_on_the_device(engine, case):
    cur, ref = model.pictures(case)
    (alone,) = luma_model.estimate(cur[0], [ref[0]], 8, 6)
    (e,) = check(engine, cur, [ref], 8)
    if case == 1:       # Cb lowers luma's denominator, and its offset goes through the chroma rule: raw 100 -> -1 where a plain clip keeps 100
        assert alone["wp"] == (64, 0, 6, 32) and e[0]["wp"] == (32, 0, 5, 16)
        assert e[1]["wp"] == (160, -1, 5, 16) and (sum(x["sad_wp"] for x in e), sum(x["sad_nowp"] for x in e)) == (3232, 5760)
    elif case == 2:     # the ratio flips luma's decision to present
        assert alone["present"] == 0 and e[0]["present"] == 1 and e[0]["weight"] == 66
    else:               # ... and to not present
        assert alone["present"] == 1 and alone["offset"] == 2 and [x["present"] for x in e] == [0, 0, 0]
        assert (sum(x["sad_wp"] for x in e), sum(x["sad_nowp"] for x in e)) == (12288, 864)


def steep(p, bd):
    """a picture whose AC is a quarter of p's: the weight 4 << d fits no denominator above 5"""
    return fade(p, 0.25, 40, bd)


@pytest.mark.parametrize("where", ["cb", "cr", "last_reference"])
def test_one_chroma_plane_lowers_the_denominator_of_all(engine, where):
    bd, w, h = 8, 48, 18
    cur = picture(w, h, bd, seed=31, kind=smooth)
    n = 4 if where == "last_reference" else 1
    refs = [faded(cur, 0.8 + 0.1 * i, 3 * i, bd) for i in range(n)]
    start = 7 if n > 3 else 6
    assert all(e["log2_denom"] == start for r in model.estimate(cur, refs, bd, start) for e in r)     # without the steep plane the start is kept
    c = {"cb": 1, "cr": 2, "last_reference": 2}[where]
    last = list(refs[-1])
    last[c] = steep(cur[c], bd)
    refs[-1] = tuple(last)
    es = check(engine, cur, refs, bd, start)
    assert all(e["log2_denom"] == 5 for r in es for e in r)
    assert es[-1][c]["weight"] > 3 << 5 and es[0][0]["weight"] != 32            # about 4: twice that weight is beyond 64 + 127


# ---- HM's corners ----------------------------------------------------------------------------------------------------------------------------------

def test_identical_pictures_stay_present(engine):
    cur = picture(48, 18, 8, seed=41)
    (e,) = check(engine, cur, [tuple(p.copy() for p in cur)], 8)
    assert math.isnan(e[0]["ratio"]) and all(x["present"] == 1 and x["wp"] == (64, 0, 6, 32) for x in e)


def test_identical_luma_with_differing_chroma(engine):
    cur = picture(48, 18, 8, seed=42, kind=smooth)
    ref = (cur[0].copy(), fade(cur[1], 0.8, 20, 8), noise(24, 9, 8, seed=43))
    (e,) = check(engine, cur, [ref], 8)
    assert (e[0]["sad_wp"], e[0]["sad_nowp"]) == (0, 0) and not math.isnan(e[0]["ratio"])
    assert e[1]["weight"] != 64 and e[2]["sad_nowp"] > 0


def test_flat_chroma_reference(engine):
    cur = picture(48, 18, 8, seed=44)
    ref = (fade(cur[0], 0.9, 4, 8), model.flat(24, 9, 77), model.flat(24, 9, 0))
    (e,) = check(engine, cur, [ref], 8)
    assert e[1]["ref_ac"] == 0 and e[2]["ref_ac"] == 0 and e[1]["log2_denom"] == 6
    ok, p = model.update_parameters([luma_model.plane_stats(x) for x in cur], [[luma_model.plane_stats(x) for x in ref]], [x.size for x in cur], 8, 6)
    assert ok and p[0][1][0] == 64 and p[0][2][0] == 64                         # dWeight 1.0


def test_twelve_bit_extremes_with_the_largest_weight(engine):
    # every component: current 4095 / 0 in alternating columns, reference 0 / 2057 -- weight 255 at a denominator of 7, a weighted term of about
    # 2^19 per sample; 512 x 128 luma / 256 x 64 chroma put every plane's sum beyond 32 bits
    def pair(w, h):
        cur, ref = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
        cur[:, 0::2] = 4095
        ref[:, 1::2] = 2057
        return cur, ref
    (cy, ry), (cb, rb), (cr, rr) = pair(512, 128), pair(256, 64), pair(256, 64)
    ok, p = model.update_parameters([luma_model.plane_stats(x) for x in (cy, cb, cr)], [[luma_model.plane_stats(x) for x in (ry, rb, rr)]],
                                    [cy.size, cb.size, cr.size], 12, 7)
    assert ok and [wgt for wgt, _ in p[0]] == [255, 255, 255]
    (e,) = check(engine, (cy, cb, cr), [(ry, rb, rr)], 12, start=7)
    assert all(x["log2_denom"] == 7 and x["sad_wp"] > 1 << 18 and x["sad_wp"] * n > 1 << 32 for x, n in zip(e, (cy.size, cb.size, cr.size)))
    # and plain 0 / 4095 checkerboards against their inverse: the largest unweighted difference
    cur = tuple(model.checkerboard(w, h, 0, 4095) for w, h in ((512, 128), (256, 64), (256, 64)))
    ref = tuple(4095 - p for p in cur)
    (e,) = check(engine, cur, [ref], 12, start=7)
    assert all(x["sad_nowp"] == 4095 << 7 for x in e)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------------------

def test_sixteen_references_in_one_call(engine):
    bd, w, h = 8, 32, 16
    cur = picture(w, h, bd, seed=51, kind=smooth)
    gains = [0.6, 0.8, 1.0, 1.3, 1.6, 0.9, 1.1, 0.7]
    refs = [faded(cur, gains[i % 8], (i * 7) % 40 - 20, bd) if i % 5 != 4 else mirrored(cur) for i in range(16)]
    es = check(engine, cur, refs, bd, 7)                                         # 51 planes, 48 pairs
    assert len({e["log2_denom"] for r in es for e in r}) == 1
    assert {r[0]["present"] for r in es} == {0, 1}


def test_the_same_picture_twice_and_the_current_picture_as_a_reference(engine):
    bd = 8
    cur = picture(48, 18, bd, seed=52, kind=smooth)
    ref = faded(cur, 0.75, 10, bd)
    other = picture(48, 18, bd, seed=53)
    es = check(engine, cur, [ref, other, ref, cur], bd)
    assert es[0] == es[2] and es[0][0]["present"] == 1 and es[0] != es[1]
    assert math.isnan(es[3][0]["ratio"]) and all(x["present"] == 1 and x["weight"] == 1 << x["log2_denom"] for x in es[3])


def test_start_seven_is_kept_when_every_weight_fits(engine):
    cur = picture(48, 18, 8, seed=54, kind=smooth)
    es = check(engine, cur, [faded(cur, 0.8, 5, 8), faded(cur, 1.2, -5, 8)], 8, 7)
    assert all(e["log2_denom"] == 7 for r in es for e in r) and any(e["present"] and e["weight"] != 128 for r in es for e in r)


def test_cached_statistics(engine):
    bd = 8
    cur = picture(48, 18, bd, seed=55, kind=smooth)
    ref = faded(cur, 0.75, 10, bd)
    new_cb = fade(cur[1], 0.5, 30, bd)
    assert luma_model.plane_stats(new_cb) != luma_model.plane_stats(ref[1])
    planes = Planes(engine, bd)
    try:
        pc, pr = planes.triple(cur), planes.triple(ref)
        luma_before = engine.wp_estimate(pc[0], [pr[0]])
        for p, img in zip(pr, ref):                                                 # planes that went through hmme_plane_stats before ...
            assert engine.plane_stats(p) == luma_model.plane_stats(img)
        first = engine.wp_estimate_420(pc, [pr])
        compare(first, model.estimate(cur, [ref], bd), bd)                          # ... give what fresh ones give
        again = engine.wp_estimate_420(pc, [pr])                                    # every sum cached
        assert [tuple(x) for x in again[0] + again[1]] == [tuple(x) for x in first[0] + first[1]]
        assert [i.as_dict() for i in again[2]] == [i.as_dict() for i in first[2]]
        upload(engine, pr[1], new_cb)                                               # a refill drops that plane's sums
        compare(engine.wp_estimate_420(pc, [pr]), model.estimate(cur, [(ref[0], new_cb, ref[2])], bd), bd)
        # the old call neither sees nor loses anything: its result on the luma planes is what it was
        luma_after = engine.wp_estimate(pc[0], [pr[0]])
        assert luma_after[0] == luma_before[0] and [i.as_dict() for i in luma_after[1]] == [i.as_dict() for i in luma_before[1]]
        assert luma_after[0] == [luma_model.estimate(cur[0], [ref[0]], bd)[0]["wp"]]
    finally:
        planes.close()


# ---- against the existing call ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10])
def test_flat_equal_chroma_leaves_the_luma_estimate(engine, bd):
    w, h = 130, 66
    cur_y = smooth(w, h, bd, seed=61)
    refs_y = [fade(cur_y, 0.75, 10, bd), np.ascontiguousarray(cur_y[:, ::-1]), fade(cur_y, 0.25, 40, bd)]   # a fade, the mirror image, a steep fade
    cb, cr = model.flat(w // 2, h // 2, 90 << (bd - 8)), model.flat(w // 2, h // 2, 200 << (bd - 8))
    planes = Planes(engine, bd)
    try:
        py, pcb, pcr = planes(cur_y), planes(cb), planes(cr)
        pry = [planes(r) for r in refs_y]
        wl, wc, infos = engine.wp_estimate_420([py, pcb, pcr], [[r, pcb, pcr] for r in pry])
        weights, luma_infos = engine.wp_estimate(py, pry)
    finally:
        planes.close()
    assert wl == weights and [infos[3 * r].as_dict() for r in range(3)] == [i.as_dict() for i in luma_infos]
    assert {i.present for i in luma_infos} == {0, 1} and luma_infos[0].log2_denom == 5


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing(engine):
    from hmme import api
    L = engine.L
    other_engine = api.Engine(0, 64)
    img = lambda w, h: noise(w, h, 8, seed=w + h)
    mk = lambda e, w, h, bd=8: make_plane(e, img(w, h), bd)
    P = {"y": mk(engine, 32, 16), "cb": mk(engine, 16, 8), "cr": mk(engine, 16, 8), "y_big": mk(engine, 48, 16), "c_big": mk(engine, 24, 8),
         "y_odd": mk(engine, 33, 16), "y_low": mk(engine, 32, 14), "y10": mk(engine, 32, 16, 10), "c10": mk(engine, 16, 8, 10),
         "foreign": mk(other_engine, 16, 8)}
    was = L.hmme_set_error_printing(engine.h, 0)
    sentinel = api.Weight(-1, -2, -3, -4)

    def call(cur, refs, start=6, n_refs=None, null=None):
        n = len(refs) // 3 if n_refs is None else n_refs
        ca = (C.c_void_p * 3)(*[p.h if p else None for p in cur])
        ra = (C.c_void_p * max(1, len(refs)))(*[p.h if p else None for p in refs])
        wl, wc, ia = (api.Weight * 17)(*[sentinel] * 17), (api.Weight * 34)(*[sentinel] * 34), (api.WpInfo * 51)()
        C.memset(ia, 0x5a, C.sizeof(ia))
        args = {"cur": ca, "refs": ra, "wl": wl, "wc": wc, "info": ia}
        if null:
            args[null] = None
        rc = L.hmme_wp_estimate_420(engine.h, args["cur"], args["refs"], n, start, args["wl"], args["wc"], args["info"])
        untouched = all((w.w0, w.offset, w.shift, w.round) == (-1, -2, -3, -4) for w in list(wl) + list(wc)) and bytes(ia) == b"\x5a" * C.sizeof(ia)
        return rc, untouched
    try:
        good = [P["y"], P["cb"], P["cr"]]
        cases = [("null cur", dict(cur=good, refs=good, null="cur")), ("null refs", dict(cur=good, refs=good, null="refs")),
                 ("null luma output", dict(cur=good, refs=good, null="wl")), ("null chroma output", dict(cur=good, refs=good, null="wc")),
                 ("null plane", dict(cur=good, refs=[P["y"], None, P["cr"]])), ("null current plane", dict(cur=[P["y"], P["cb"], None], refs=good)),
                 ("n_refs 0", dict(cur=good, refs=good, n_refs=0)), ("n_refs 17", dict(cur=good, refs=good * 17)),
                 ("start 2", dict(cur=good, refs=good, start=2)), ("start 8", dict(cur=good, refs=good, start=8)),
                 ("context", dict(cur=good, refs=[P["y"], P["foreign"], P["cr"]])),
                 ("odd luma", dict(cur=[P["y_odd"], P["cb"], P["cr"]], refs=[P["y_odd"], P["cb"], P["cr"]])),
                 ("low luma", dict(cur=[P["y_low"], P["cb"], P["cr"]], refs=[P["y_low"], P["cb"], P["cr"]])),
                 ("current chroma size", dict(cur=[P["y"], P["cb"], P["c_big"]], refs=good)),
                 ("reference chroma size", dict(cur=good, refs=good + [P["y"], P["c_big"], P["cr"]])),
                 ("reference depth", dict(cur=good, refs=[P["y"], P["cb"], P["c10"]])),
                 ("luma depth", dict(cur=good, refs=[P["y10"], P["cb"], P["cr"]])),
                 ("reference luma size", dict(cur=good, refs=good + [P["y_big"], P["c_big"], P["c_big"]]))]
        for name, kw in cases:
            assert call(**kw) == (ERR_ARG, True), name
        rc, untouched = call(good, good * 16, null="info")                        # the largest call that is served, without out_info
        assert rc == 0 and not untouched
    finally:
        L.hmme_set_error_printing(engine.h, was)
        for p in P.values():
            p.close()
        other_engine.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------

def test_estimated_weights_serve_the_search_and_the_chroma_prediction(engine):
    from hmme import synth
    w = h = 128
    m = synth.MARGIN
    area = lambda p: np.asarray(p)[m:-m, m:-m].astype(np.int64)
    cur_y, ref_y, true_mv = synth.make_pair(w, h, seed=71, max_mv=4, region=64)
    cur_c, ref_c = synth.make_chroma_pair(w, h, true_mv, seed=71, region=64)
    cur = faded((area(cur_y), area(cur_c[0]), area(cur_c[1])), 0.75, 10, 8)       # the fade on all three components
    ref = (area(ref_y), area(ref_c[0]), area(ref_c[1]))
    (e,) = model.estimate(cur, [ref], 8)
    assert all(x["present"] == 1 and abs(x["weight"] - 48) <= 1 and abs(x["offset"] - 10) <= 2 for x in e)
    planes = Planes(engine, 8)
    try:
        pc, pr = planes.triple(cur), planes.triple(ref)
        wl, wc, infos = engine.wp_estimate_420(pc, [pr])
        compare((wl, wc, infos), [e], 8)
        assert all(i.served_search == 1 and i.served_refine == 1 for i in infos)
        mv_w, sad_w = engine.search_frame_w(pc[0], pr[0], 8, wl[0])
        mv_u, sad_u = engine.search_frame(pc[0], pr[0], 8, fen=0)
        field = (4 * true_mv.reshape(-1, 2)).astype(np.int16)                    # one MV per CTU (region = CTU), quarter pels
        assert (mv_w[:, 592] == true_mv.reshape(-1, 2)).all()
        weighted = engine.predict_chroma_frame(pr[1:], w, h, field, weights=wc)    # the chroma weights are accepted as they come
        plain = engine.predict_chroma_frame(pr[1:], w, h, field)
    finally:
        planes.close()
    assert int(sad_w.astype(np.int64).sum()) < int(sad_u.astype(np.int64).sum())
    for c in range(2):
        sad = lambda p: int(np.abs(p.astype(np.int64) - cur[1 + c]).sum())
        assert sad(weighted[c]) < sad(plain[c]), (c, sad(weighted[c]), sad(plain[c]))
