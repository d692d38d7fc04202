"""hmme_plane_stats / hmme_wp_estimate on the device against the numpy restatement of HM's WeightPredAnalysis (tests/wp_estimate_model.py):
every sum, every intermediate and every weight bit for bit.  Each case first asserts ON THE MODEL that its input exercises what it is about."""
import ctypes as C
import math

import numpy as np
import pytest

import wp_estimate_model as model

pytestmark = pytest.mark.gpu

ERR_ARG = -1


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(57.9)
    yield e
    e.close()


def upload(engine, plane, img):
    bd = plane.bit_depth
    if bd == 8:
        plane.upload_u8(np.ascontiguousarray(img, dtype=np.uint8))
    else:
        a = np.ascontiguousarray(img, dtype=np.int16)
        engine._check(engine.L.hmme_plane_upload_pel(plane.h, a.ctypes.data, a.shape[1]))


def make_plane(engine, img, bd):
    img = np.asarray(img)
    pl = engine.plane(img.shape[1], img.shape[0], bd)
    upload(engine, pl, img)
    return pl


def noise(w, h, bd, seed):
    return np.random.default_rng(seed).integers(0, 1 << bd, (h, w)).astype(np.int64)


def smooth(w, h, bd, seed):
    """a texture with neighbouring samples alike (what a fade is estimated on), full range"""
    from hmme import synth
    base = synth._box5(np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.float64))
    return np.rint((base - base.min()) * (((1 << bd) - 1) / (base.max() - base.min()))).astype(np.int64)


def fade(ref, a, b, bd):
    """cur = clip(a * ref + b), b in 8-bit units"""
    return np.clip(np.rint(a * ref + b * (1 << (bd - 8))), 0, (1 << bd) - 1).astype(np.int64)


def check_estimate(engine, cur, refs, bd, start=6):
    """one device call against the model, everything compared; -> the model's entries"""
    from hmme import api
    planes = {}

    def plane_of(img):      # the same array given twice is the same plane given twice
        if id(img) not in planes:
            planes[id(img)] = make_plane(engine, img, bd)
        return planes[id(img)]
    try:
        weights, infos = engine.wp_estimate(plane_of(cur), [plane_of(r) for r in refs], start)
    finally:
        for p in planes.values():
            p.close()
    want = model.estimate(cur, refs, bd, start)
    assert len(weights) == len(infos) == len(want)
    for r, (w, info, e) in enumerate(zip(weights, infos, want)):
        got = info.as_dict()
        assert {k: got[k] for k in model.INFO_FIELDS} == {k: e[k] for k in model.INFO_FIELDS}, (r, got, e)
        assert tuple(w) == e["wp"], (r, w, e["wp"])
        assert got["served_search"] == int(api.weight_check(bd, e["wp"], False) == 0)
        assert got["served_refine"] == int(api.weight_check(bd, e["wp"], True) == 0)
    return want


# ---- plane_stats ---------------------------------------------------------------------------------------------------------------------------------

# widths that are 0, 6, 8 and 14 mod 16 (78 x 10 adds the last to the listed sizes), i.e. rows that end in a whole vector, in 6, 8 or 14 bytes of one
# (u8) or in 12 (u16); 64 and 70 are rows of fewer vectors than a wave has lanes, 1000 x 8 is wider than it is high
SIZES = [(64, 64), (70, 38), (136, 72), (200, 136), (1000, 8), (78, 10)]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("w,h", SIZES)
def test_plane_stats_random(engine, w, h, bd):
    img = noise(w, h, bd, seed=w * 31 + h + bd)
    want = model.plane_stats(img)
    assert want[1] > 0
    with make_plane(engine, img, bd) as pl:
        assert engine.plane_stats(pl) == want
        assert engine.plane_stats(pl) == want          # the cached sums


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_plane_stats_constant_pictures(engine, bd):
    maxv = (1 << bd) - 1
    for v in (0, maxv):
        img = np.full((38, 70), v, np.int64)
        assert model.plane_stats(img) == (v * 70 * 38, 0)
        with make_plane(engine, img, bd) as pl:
            assert engine.plane_stats(pl) == (v * 70 * 38, 0)


def test_plane_stats_sum_beyond_32_bits(engine):
    img = np.full((1080, 1920), 4095, np.int64)
    want = model.plane_stats(img)
    assert want[0] > 1 << 32 and want[1] == 0
    with make_plane(engine, img, 12) as pl:
        assert engine.plane_stats(pl) == want
    img = np.full((1080, 2048), 4095, np.int64)          # and an AC beyond 32 bits: |sample - 2048| = 2047 or 2048 on 2.2 M samples
    img[:, ::2] = 0
    want = model.plane_stats(img)
    assert want[1] > 1 << 32
    with make_plane(engine, img, 12) as pl:
        assert engine.plane_stats(pl) == want


@pytest.mark.parametrize("bd", [8, 10])
def test_plane_stats_do_not_count_the_margins(engine, bd):
    # the border rows and columns are replicated into 128 / 80 samples of margin on every side: a kernel that counted any of it would be far off
    maxv = (1 << bd) - 1
    img = np.zeros((38, 70), np.int64)
    img[0, :] = img[-1, :] = maxv
    img[:, 0] = img[:, -1] = maxv
    want = model.plane_stats(img)
    assert want[0] == maxv * (2 * 70 + 2 * 36)
    with make_plane(engine, img, bd) as pl:
        assert engine.plane_stats(pl) == want


def test_plane_stats_follow_a_second_upload(engine):
    a, b = noise(136, 72, 8, seed=1), noise(136, 72, 8, seed=2) // 3
    assert model.plane_stats(a) != model.plane_stats(b)
    with make_plane(engine, a, 8) as pl:
        assert engine.plane_stats(pl) == model.plane_stats(a)
        upload(engine, pl, b)
        assert engine.plane_stats(pl) == model.plane_stats(b)


# ---- wp_estimate, one reference --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", model.CASES)
def test_hand_checkable_cases_on_the_device(engine, case):
    cur, ref = model.pictures(case)
    (e,) = check_estimate(engine, cur, [ref], 8)
    if case == "checkerboard":
        assert (e["log2_denom"], e["sad_wp"], e["sad_nowp"], e["present"]) == (5, 6144, 400, 0)
    elif case == "identical":
        assert math.isnan(e["ratio"]) and e["present"] == 1 and e["wp"] == (64, 0, 6, 32)
    elif case == "flat_reference":
        assert e["ref_ac"] == 0
    elif case == "offset_fade":
        assert (e["weight"], e["offset"], e["present"]) == (64, 20, 1)
    else:
        assert e["ratio"] >= 0.99 and e["present"] == 0


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("b", [-20, 0, 30])
@pytest.mark.parametrize("a", [0.5, 0.75, 1.25, 3.5])
def test_fades(engine, a, b, bd):
    scale = 1 << (bd - 8)
    ref = (24 * scale + smooth(136, 72, bd, seed=77) * 36 // 255).astype(np.int64)      # a dark picture: 24 .. 60 in 8-bit units
    cur = fade(ref, a, b, bd)
    (e,) = check_estimate(engine, cur, [ref], bd)
    assert e["cur_ac"] > 0 and e["ref_ac"] > 0
    if (a * ref + b * scale).min() >= 0 and (a * ref + b * scale).max() <= (1 << bd) - 1:   # nothing clipped: the estimate is the fade itself
        if a == 3.5:
            assert e["log2_denom"] == 5 and abs(e["weight"] / 32 - a) < 0.1                # 3.5 * 64 = 224 does not fit the denominator HM starts with
        else:
            assert e["log2_denom"] == 6 and e["present"] == 1 and abs(e["weight"] / 64 - a) < 0.05
    else:
        assert a * 24 + b < 0                            # the only fades of this picture that clip are those that reach below zero


def test_twelve_bit_extremes(engine):
    w, h = 1920, 1080
    # the issue's picture: current all 4095, reference alternating 0 / 4095
    cur = np.full((h, w), 4095, np.int64)
    ref = np.zeros((h, w), np.int64)
    ref[:, 1::2] = 4095
    (e,) = check_estimate(engine, cur, [ref], 12)
    assert e["cur_ac"] == 0 and e["sad_nowp"] * w * h > 1 << 32
    # ... and the weighted term near the top of what a denominator of 7 admits (weight 255): about 2^19 for every one of 2 M samples
    cur = np.zeros((h, w), np.int64)
    cur[:, 0::2] = 4095
    ref = np.zeros((h, w), np.int64)
    ref[:, 1::2] = 2057
    (e,) = check_estimate(engine, cur, [ref], 12, start=7)
    (ok, ((weight, offset),)) = model.update_parameters(model.plane_stats(cur), [model.plane_stats(ref)], w * h, 12, 7)
    assert ok and weight == 255 and e["log2_denom"] == 7
    per_sample = min(abs((4095 << 7) - (offset << 11)), abs(2057 * weight + (offset << 11)))
    assert per_sample > 1 << 18 and e["sad_wp"] >= per_sample and per_sample * w * h > 1 << 38


# ---- wp_estimate, several references ---------------------------------------------------------------------------------------------------------------

def reference_set(cur, n, bd, steep):
    """n references of `cur`: fades of it by gains below 2 (they fit a denominator of 7), unrelated noise, and -- steep -- one whose AC is a
    quarter of the picture's, which no denominator above 5 holds"""
    h, w = cur.shape
    gains = [0.6, 0.8, 1.0, 1.3, 1.6, 0.9, 1.1, 0.7]
    refs = [fade(cur, gains[i % len(gains)], (i * 7) % 40 - 20, bd) if i % 5 != 4 else noise(w, h, bd, seed=900 + i) for i in range(n)]
    if steep:
        refs[n // 2] = fade(cur, 0.25, 40, bd)
    return refs


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n", [4, 16])
def test_several_references_share_a_denominator(engine, n, bd):
    cur = smooth(136, 72, bd, seed=5)
    start = 7 if n > 3 else 6                            # HM's own rule
    es = check_estimate(engine, cur, reference_set(cur, n, bd, steep=True), bd, start)
    assert all(e["log2_denom"] < start for e in es) and len({e["log2_denom"] for e in es}) == 1
    assert any(e["present"] and e["weight"] != 32 for e in es)


def test_start_seven_is_kept_when_every_weight_fits(engine):
    cur = smooth(200, 136, 8, seed=6)
    es = check_estimate(engine, cur, reference_set(cur, 4, 8, steep=False), 8, 7)
    assert all(e["log2_denom"] == 7 for e in es)
    assert any(e["present"] and e["weight"] != 128 for e in es)


def test_the_same_plane_twice_gives_equal_entries(engine):
    cur = smooth(136, 72, 8, seed=7)
    ref = fade(cur, 0.75, 10, 8)
    other = noise(136, 72, 8, seed=8)
    es = check_estimate(engine, cur, [ref, other, ref], 8)
    assert es[0] == es[2] and es[0]["present"] == 1 and es[0] != es[1]


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing(engine):
    from hmme import api
    L = engine.L
    img = noise(136, 72, 8, seed=9)
    other_engine = api.Engine(0, 64)
    planes = {"cur": make_plane(engine, img, 8), "ref": make_plane(engine, img, 8), "small": make_plane(engine, img[:64, :128], 8),
              "deep": make_plane(engine, img, 10), "foreign": make_plane(other_engine, img, 8)}
    was = L.hmme_set_error_printing(engine.h, 0)

    def call(cur, refs, start):
        ra = (C.c_void_p * max(1, len(refs)))(*[r.h for r in refs])
        wa = (api.Weight * 17)(*[api.Weight(-1, -2, -3, -4)] * 17)
        ia = (api.WpInfo * 17)()
        C.memset(ia, 0x5a, C.sizeof(ia))
        rc = L.hmme_wp_estimate(engine.h, cur.h, ra, len(refs), start, wa, ia)
        untouched = all((w.w0, w.offset, w.shift, w.round) == (-1, -2, -3, -4) for w in wa) and bytes(ia) == b"\x5a" * C.sizeof(ia)
        return rc, untouched
    try:
        cur, ref = planes["cur"], planes["ref"]
        for name, refs, start in (("size", [ref, planes["small"]], 6), ("depth", [planes["deep"]], 6), ("context", [ref, planes["foreign"]], 6),
                                  ("n_refs 0", [], 6), ("n_refs 17", [ref] * 17, 6), ("start 2", [ref], 2), ("start 8", [ref], 8)):
            assert call(cur, refs, start) == (ERR_ARG, True), name
        assert call(planes["foreign"], [ref], 6) == (ERR_ARG, True)
        rc, untouched = call(cur, [ref] * 16, 6)          # the largest call that is served
        assert rc == 0 and not untouched
    finally:
        L.hmme_set_error_printing(engine.h, was)
        for p in planes.values():
            p.close()
        other_engine.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------

def shifted_fade_pictures(n, size=128, gains=(1.0, 0.75, 0.5625, 0.45), offsets=(0, 10, 20, 28)):
    """picture t = the fade (gains[t], offsets[t]) of one texture displaced by t * (3, -2): for cur = t and ref = t - 1, cur[y, x] is the faded
    ref[y - 2, x + 3] -- the motion vector (3, -2)"""
    g = 16
    base = smooth(size + 2 * g, size + 2 * g, 8, seed=321)
    pics = []
    for t in range(n):
        part = base[g - 2 * t:g - 2 * t + size, g + 3 * t:g + 3 * t + size]
        pics.append(np.clip(np.rint(gains[t] * part + offsets[t]), 0, 255).astype(np.uint8))
    return pics


def test_estimated_weight_serves_the_weighted_search(engine):
    ref, cur = shifted_fade_pictures(2)
    (e,) = model.estimate(cur.astype(np.int64), [ref.astype(np.int64)], 8, 6)
    assert e["present"] == 1 and e["weight"] == 48 and abs(e["offset"] - 10) <= 2
    with make_plane(engine, cur, 8) as pc, make_plane(engine, ref, 8) as pr:
        (wp,), (info,) = engine.wp_estimate(pc, [pr])
        assert tuple(wp) == e["wp"] and info.served_search == 1
        mv_w, sad_w = engine.search_frame_w(pc, pr, 8, wp)
        mv_u, sad_u = engine.search_frame(pc, pr, 8, fen=0)
    assert (mv_w[:, 592] == (3, -2)).all(), mv_w[:, 592]          # slot 592: the 64x64 PU
    assert int(sad_w.astype(np.int64).sum()) < int(sad_u.astype(np.int64).sum())


class _Pictures:
    def __init__(self, pics):
        self.pics = pics

    def read_into(self, poc, out):
        np.copyto(out, self.pics[poc])


def test_run_rank_estimates_like_the_engine(engine):
    import torch
    from hmme import sequence
    pics = shifted_fade_pictures(4)
    pairs = [(1, 0), (2, 1), (3, 2)]
    want = [model.estimate(pics[c].astype(np.int64), [pics[r].astype(np.int64)], 8, 6)[0] for c, r in pairs]
    assert all(e["present"] == 1 and e["weight"] != 64 for e in want)
    weights = []
    for c, r in pairs:
        with make_plane(engine, pics[c], 8) as pc, make_plane(engine, pics[r], 8) as pr:
            (wp,), _ = engine.wp_estimate(pc, [pr])
            weights.append(tuple(wp))
    assert weights == [e["wp"] for e in want]
    src = _Pictures(pics)
    est = sequence.run_rank(engine, src, pairs, 128, 128, 8, 8, pairs_per_launch=2, refine=True, weights="estimate")
    lst = sequence.run_rank(engine, src, pairs, 128, 128, 8, 8, pairs_per_launch=2, refine=True, weights=weights)
    assert [tuple(w) for w in est["weights"]] == weights
    assert [d["present"] for d in est["wp_info"]] == [1, 1, 1]
    for k in ("mv", "sad", "qmv", "cost"):
        assert torch.equal(est[k], lst[k]), k
    assert (est["mv"][:, :, 592].cpu().numpy() == (3, -2)).all()
