"""The device against the reference's own recorded answers (tests/golden/ref_*.npz, read through tests/ref_tails.py): motion-compensated
luma and chroma blocks, TComYuv::addAvg, addWeightUni / addWeightBi, the weighted-prediction estimator and the residual's distortions.  No numpy
model stands between the recording and the device's output.  Every case is a one-CTU picture (64x64 luma, 32x32 chroma) with up to nine golden
blocks inside, each at the MV whose fraction is the case's phase; every comparison is bit-exact."""
import functools

import numpy as np
import pytest

import ref_tails as rt

pytestmark = pytest.mark.gpu

BDS = (8, 9, 10, 11, 12)
NO_SLOT = 0xFFFF


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda(57.9)
    yield e
    e.close()


class Planes:
    """planes made from picture-area images, closed together"""

    def __init__(self, engine, bd):
        self.engine, self.bd, self.made = engine, bd, []

    def __call__(self, img):
        img = np.asarray(img)
        p = self.engine.plane(img.shape[1], img.shape[0], self.bd)
        self.made.append(p)
        if self.bd == 8:
            p.upload_u8(np.ascontiguousarray(img, dtype=np.uint8))
        else:
            p.upload_pel(np.ascontiguousarray(img, dtype=np.int16), (0, 0))
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.made:
            p.close()


def chunks(items, n=rt.PER_PICTURE):
    return [items[i:i + n] for i in range(0, len(items), n)]


def dirs_field(n_blocks, direction):
    d = np.full((1, 64), 0xFF, np.uint8)
    for n in range(n_blocks):
        d[0, rt.block_index(n)] = direction if np.isscalar(direction) else direction[n]
    return d


def check_blocks(kind, image, wants, where):
    for n, want in enumerate(wants):
        got = rt.cut(kind, image, n)
        assert np.array_equal(got, np.asarray(want).astype(np.int64)), (where, n, got.tolist(), np.asarray(want).tolist())


# ---- luma ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", BDS)
def test_luma_prediction_of_every_recorded_block(engine, bd):
    """hmme_predict_frame, hmme_predict_refs_frame and the one-list blocks (directions 1 and 2) of hmme_predict_bi_frame on random, binary,
    all-maximum and tap-sign content at all 16 phases: the reference's clipped sample"""
    i = BDS.index(bd)
    fill = (1 << bd) >> 1
    zero = np.zeros((1, 64, 2), np.int16)
    for group in chunks(rt.all_block_cases("luma")):
        field = rt.field("luma", [ph for _, ph in group])
        wants = [rt.block("luma", i, c, ph, 0) for c, ph in group]
        with Planes(engine, bd) as mk:
            p = mk(rt.picture("luma", [rt.source("luma", i, c) for c, _ in group], fill))
            flat = mk(np.full((64, 64), fill))
            check_blocks("luma", engine.predict_frame(p, field), wants, ("predict_frame", bd, group))
            refs = np.zeros((1, 64), np.uint8)
            refs[0, [rt.block_index(n) for n in range(len(group))]] = 1
            check_blocks("luma", engine.predict_refs_frame([flat, p], field, refs), wants, ("predict_refs_frame", bd, group))
            check_blocks("luma", engine.predict_bi_frame(p, flat, (field, zero), dirs_field(len(group), 1)), wants, ("predict_bi_frame L0", bd, group))
            check_blocks("luma", engine.predict_bi_frame(flat, p, (zero, field), dirs_field(len(group), 2)), wants, ("predict_bi_frame L1", bd, group))


def tail_pictures(kind, i, fill):
    """-> (picture of list 0, picture of list 1, field of list 0, of list 1, directions): blocks 0..3 the four operand pairs (direction 3), blocks 4..7
    the four operands alone, in both pictures (direction 1)"""
    T = rt.load("ref_tails")
    ops = [rt.operand(kind, i, o) for o in range(4)]
    a = [ops[int(p[0])] for p in T["pairs"]] + ops
    b = [ops[int(p[1])] for p in T["pairs"]] + ops
    pic = lambda side: rt.picture(kind, [rt.source(kind, i, c) for c, _, _ in side], fill)
    fld = lambda side: rt.field(kind, [ph for _, ph, _ in side])
    return pic(a), pic(b), fld(a), fld(b), dirs_field(8, [3] * 4 + [1] * 4)


@pytest.mark.parametrize("bd", BDS)
def test_luma_tails(engine, bd):
    """direction 3 of hmme_predict_bi_frame (addAvg), hmme_predict_frame_w and hmme_predict_refs_w_frame (addWeightUni), hmme_predict_bi_w_frame
    (addWeightBi) on the largest and the smallest intermediate the interpolation can give and on random ones, over HM's whole weight syntax"""
    i = BDS.index(bd)
    T = rt.load("ref_tails")
    pa, pb, fa, fb, dirs = tail_pictures("luma", i, (1 << bd) >> 1)
    refs = np.zeros((1, 64), np.uint8)
    refs[0, [rt.block_index(n) for n in (5, 7)]] = 1
    with Planes(engine, bd) as mk:
        a, b = mk(pa), mk(pb)
        avg = engine.predict_bi_frame(a, b, (fa, fb), dirs)
        check_blocks("luma", avg, T["avg_luma"][i], ("addAvg", bd))
        for k in range(rt.N_WEIGHTS):
            wp = rt.hmme_weight(T["triples"][k], bd)
            k1 = (k + 1) % rt.N_WEIGHTS
            wp1 = rt.hmme_weight(T["triples"][k1], bd)
            firsts = [int(p[0]) for p in T["pairs"]]                 # blocks 0..3 of list 0's picture: the pairs' first operands
            uni = engine.predict_frame_w(a, wp, fa)
            check_blocks("luma", uni, [T["uni_luma"][i, o, k] for o in firsts + [0, 1, 2, 3]], ("addWeightUni", bd, wp))
            two = engine.predict_refs_w_frame([a, a], [wp, wp1], fa, refs)
            want = [T["uni_luma"][i, o, k] for o in firsts] + [T["uni_luma"][i, o, k1 if o in (1, 3) else k] for o in range(4)]
            check_blocks("luma", two, want, ("predict_refs_w_frame", bd, wp, wp1))
            w0, w1 = rt.bi_weights(T["bi_weights"][k], bd)
            bi = engine.predict_bi_w_frame(a, b, w0, w1, (fa, fb), dirs)
            check_blocks("luma", bi, T["bi_luma"][i, :, k], ("addWeightBi", bd, w0, w1))


# ---- chroma ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", BDS)
def test_chroma_prediction_of_every_recorded_block(engine, bd):
    """hmme_predict_chroma_frame, _refs_frame and the one-list blocks of _bi_frame at all 64 phases; Cb and Cr hold different content of the
    same phases (the field is the luma field, shared)"""
    i = BDS.index(bd)
    fill = (1 << bd) >> 1
    zero = np.zeros((1, 64, 2), np.int16)
    content = lambda c, ph: c if c < 3 else 3 + 2 * ph + (c - 3)           # 3, 4: the phase's tap-sign picture and its complement
    for cb_c, cr_c in ((0, 1), (2, 3), (4, 0), (1, 4), (3, 2)):
        for group in chunks(list(range(64))):
            field = rt.field("chroma", group)
            wants = [[rt.block("chroma", i, content(c, ph), ph, 0) for ph in group] for c in (cb_c, cr_c)]
            with Planes(engine, bd) as mk:
                cb, cr = (mk(rt.picture("chroma", [rt.source("chroma", i, content(c, ph)) for ph in group], fill)) for c in (cb_c, cr_c))
                flat = mk(np.full((32, 32), fill))
                where = (bd, cb_c, cr_c, group)
                for got, want in zip(engine.predict_chroma_frame((cb, cr), 64, 64, field), wants):
                    check_blocks("chroma", got, want, ("predict_chroma_frame",) + where)
                if cb_c in (0, 3):    # the other forms share the kernel's filter: the random and the tap-sign content go through them
                    refs = np.zeros((1, 64), np.uint8)
                    refs[0, [rt.block_index(n) for n in range(len(group))]] = 1
                    for got, want in zip(engine.predict_chroma_refs_frame([flat, flat, cb, cr], 64, 64, field, refs), wants):
                        check_blocks("chroma", got, want, ("predict_chroma_refs_frame",) + where)
                    for got, want in zip(engine.predict_chroma_bi_frame((cb, cr), (flat, flat), 64, 64, (field, zero), dirs_field(len(group), 1)), wants):
                        check_blocks("chroma", got, want, ("predict_chroma_bi_frame L0",) + where)
                    for got, want in zip(engine.predict_chroma_bi_frame((flat, flat), (cb, cr), 64, 64, (zero, field), dirs_field(len(group), 2)), wants):
                        check_blocks("chroma", got, want, ("predict_chroma_bi_frame L1",) + where)
                    rf = np.zeros((2, 1, 64), np.uint8)
                    rf[0] = refs
                    for got, want in zip(engine.predict_chroma_bi_refs_frame([flat, flat, cb, cr], [flat, flat], 64, 64, (field, zero), dirs_field(len(group), 1), rf),
                                         wants):
                        check_blocks("chroma", got, want, ("predict_chroma_bi_refs_frame L0",) + where)


@pytest.mark.parametrize("bd", BDS)
def test_chroma_tails(engine, bd):
    """addAvg, addWeightUni and addWeightBi of both chroma components, each component with its own weight"""
    i = BDS.index(bd)
    T = rt.load("ref_tails")
    pa, pb, fa, fb, dirs = tail_pictures("chroma", i, (1 << bd) >> 1)
    rf = np.zeros((2, 1, 64), np.uint8)
    with Planes(engine, bd) as mk:
        a, b = mk(pa), mk(pb)          # Cb and Cr read the same plane: the reference was given the same operands for both components
        for c, got in enumerate(engine.predict_chroma_bi_frame((a, a), (b, b), 64, 64, (fa, fb), dirs)):
            check_blocks("chroma", got, T["avg_chroma"][i, c], ("addAvg", bd, c))
        for c, got in enumerate(engine.predict_chroma_bi_refs_frame([a, a], [b, b], 64, 64, (fa, fb), dirs, rf)):
            check_blocks("chroma", got, T["avg_chroma"][i, c], ("addAvg refs", bd, c))
        for k in range(rt.N_WEIGHTS):
            ks = (k, rt.cr_index(k))
            wps = [rt.hmme_weight(T["triples"][kk], bd) for kk in ks]
            for c, got in enumerate(engine.predict_chroma_frame((a, a), 64, 64, fa, weights=wps)):
                want = [T["uni_chroma"][i, c, o, k] for o in [int(p[0]) for p in T["pairs"]] + [0, 1, 2, 3]]
                check_blocks("chroma", got, want, ("addWeightUni", bd, c, wps[c]))
            pairs = [rt.bi_weights(T["bi_weights"][kk], bd) for kk in ks]
            w0, w1 = [p[0] for p in pairs], [p[1] for p in pairs]
            for c, got in enumerate(engine.predict_chroma_bi_frame((a, a), (b, b), 64, 64, (fa, fb), dirs, weights0=w0, weights1=w1)):
                check_blocks("chroma", got, T["bi_chroma"][i, c, :, k], ("addWeightBi", bd, c, pairs[c]))
            if k % 6 == 0:
                for c, got in enumerate(engine.predict_chroma_bi_refs_frame([a, a], [b, b], 64, 64, (fa, fb), dirs, rf, weights0=w0, weights1=w1)):
                    check_blocks("chroma", got, T["bi_chroma"][i, c, :, k], ("addWeightBi refs", bd, c, pairs[c]))


# ---- the estimator -----------------------------------------------------------------------------------------------------------------------------
def check_entry(case, r, c, weight, info):
    present, w, o, d = (int(v) for v in case["table"][r, c])
    assert (info.present, info.weight, info.offset, info.log2_denom) == (present, w, o, d), (case["name"], r, c, info.as_dict(), case["table"][r, c])
    assert tuple(weight) == rt.hmme_weight((w, o, d), case["bd"]), (case["name"], r, c, weight)


def test_wp_estimate_of_every_recorded_case(engine):
    """hmme_wp_estimate (4:0:0) and hmme_wp_estimate_420: present flag, weight, offset and denominator of every reference and component as
    TComSlice::initWpScaling leaves them in the reference, and the slice's two flags (on exactly when some entry is present)"""
    seen = set()
    for case in rt.wp_cases():
        bd, n = case["bd"], case["n_l0"] + case["n_l1"]
        ncomp = 3 if case["fmt"] == 420 else 1
        with Planes(engine, bd) as mk:
            if case["fmt"] == 400:
                planes = [mk(p) for p in case["pics"]]
                weights, infos = engine.wp_estimate(planes[0], planes[1:], case["start"])
                for r in range(n):
                    check_entry(case, r, 0, weights[r], infos[r])
            else:
                planes = [[mk(c) for c in p] for p in case["pics"]]
                luma, chroma, infos = engine.wp_estimate_420(planes[0], planes[1:], case["start"])
                for r in range(n):
                    check_entry(case, r, 0, luma[r], infos[3 * r])
                    for c in (1, 2):
                        check_entry(case, r, c, chroma[2 * r + c - 1], infos[3 * r + c])
        on = any(info.present for info in infos)
        assert tuple(case["flags"]) == (int(on), int(on)), case["name"]
        seen.add((case["fmt"], case["n_l0"], case["n_l1"]))
    assert len(seen) == 8


# ---- the residual's distortions ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_slot_of(w, h):
    from hmme import api
    for s in range(593):
        x, y, sw, sh = api.slot_rect(s)
        if (sw, sh) == (w, h):
            return s, x, y
    return None


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_residual_distortions_of_every_pu_rectangle(engine, bd):
    """hmme_residual_frame with a slot map that makes the golden rectangle one PU inside its CU, Hadamard and SAD: the PU's error is the
    reference's DF_HADS / DF_SAD, the CU's SSE its DF_SSE (the rest of the CU predicts exactly), the residual image the difference"""
    fill = (1 << bd) >> 1
    dt = np.uint8 if bd == 8 else np.uint16
    n = 0
    for w, h, case_bd, content, org, pred, want in rt.dist_cases():
        if case_bd != bd or (w, h) == (4, 4):
            continue
        slot, x, y = first_slot_of(w, h)
        cur_img, pred_img = np.full((64, 64), fill, np.int64), np.full((64, 64), fill, np.int64)
        cur_img[y:y + h, x:x + w], pred_img[y:y + h, x:x + w] = org, pred
        smap = np.full((1, 256), NO_SLOT, np.uint16)
        inside = [(by // 4) * 16 + bx // 4 for by in range(y, y + h, 4) for bx in range(x, x + w, 4)]
        smap[0, inside] = slot
        with Planes(engine, bd) as mk:
            cur = mk(cur_img)
            for had in (1, 0):
                resid, pu, cu, ctu = engine.residual_frame(cur, pred_img.astype(dt), smap, 256, bool(had))
                where = (w, h, bd, rt.DIST_CONTENTS[content], had)
                assert (pu[0, inside] == want[rt.HADS if had else rt.SAD]).all(), (where, pu[0, inside[0]], want)
                assert (cu[0, inside] == want[rt.SSE]).all(), (where, cu[0, inside[0]], want)
                assert tuple(ctu[0]) == (want[rt.HADS if had else rt.SAD], want[rt.SSE]), where
                assert np.array_equal(resid, (cur_img - pred_img).astype(np.int16)), where
                outside = np.setdiff1d(np.arange(256), inside)
                assert not pu[0, outside].any() and not cu[0, outside].any(), where
        n += 1
    assert n == 24 * 4


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_residual_distortions_without_a_slot_map(engine, bd):
    """every block its own PU and CU: the recorded 8x8 blocks (one MV per 8x8) and 4x4 blocks (one per 4x4), the four contents in one picture"""
    fill = (1 << bd) >> 1
    dt = np.uint8 if bd == 8 else np.uint16
    for size, per in ((8, 64), (4, 256)):
        cases = [c for c in rt.dist_cases() if c[:3] == (size, size, bd)]
        assert len(cases) == 4
        cur_img, pred_img = np.full((64, 64), fill, np.int64), np.full((64, 64), fill, np.int64)
        at = [(16 * k + 8, 16 * k + 8) for k in range(4)]
        for (x, y), case in zip(at, cases):
            cur_img[y:y + size, x:x + size], pred_img[y:y + size, x:x + size] = case[4], case[5]
        with Planes(engine, bd) as mk:
            cur = mk(cur_img)
            for had in (1, 0):
                resid, pu, cu, ctu = engine.residual_frame(cur, pred_img.astype(dt), None, per, bool(had))
                g = 64 // size
                for (x, y), case in zip(at, cases):
                    b = (y // size) * g + x // size
                    want = case[6]
                    assert (int(pu[0, b]), int(cu[0, b])) == (want[rt.HADS if had else rt.SAD], want[rt.SSE]), (size, bd, had, rt.DIST_CONTENTS[case[3]])
                assert int(pu[0].astype(np.int64).sum()) == sum(c[6][rt.HADS if had else rt.SAD] for c in cases) == int(ctu[0, 0])
                assert int(cu[0].astype(np.int64).sum()) == sum(c[6][rt.SSE] for c in cases) == int(ctu[0, 1])
                assert np.array_equal(resid, (cur_img - pred_img).astype(np.int16))


# ---- refinement on the tap-sign content ------------------------------------------------------------------------------------------------------
SR = 8


def same_tables(q, c, want, where):
    """device (qmv [593, 2], cost [593]) == the reference's recorded (x, y, cost) per slot; the message names the first differing slots"""
    got = np.concatenate([np.asarray(q).astype(np.int64), np.asarray(c).astype(np.int64)[:, None]], axis=1)
    bad = np.argwhere((got != want).any(axis=1))[:3, 0]
    assert len(bad) == 0, (where, [(int(s), got[s].tolist(), np.asarray(want[s]).tolist()) for s in bad])


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_refinement_on_tap_sign_content(engine, bd):
    """hmme_refine_ctu and hmme_refine_frame at integer MV (0, 0) against references in the sign pattern of the half-pel and quarter-pel taps,
    where the interpolation's intermediates reach their bounds; current picture the complement or random; SAD and Hadamard; all 593 slots
    against ref_frac_refine's recorded answers"""
    from hmme import api, synth
    g = rt.load("ref_refine")
    i = list(g["bds"]).index(bd)
    m = synth.MARGIN
    imv = np.zeros((593, 2), np.int16)
    try:
        for r in range(4):
            with Planes(engine, bd) as mk:
                ref_p, pr = synth.pad_plane(g["ref"][i, r]), mk(g["ref"][i, r])
                for c in range(2):
                    cur_p, pc = synth.pad_plane(g["cur"][i, r, c]), mk(g["cur"][i, r, c])
                    for had in range(2):
                        lq, px, py = (int(v) for v in g["plain_meta"][i, r, c, had])
                        want = g["plain"][i, r, c, had]
                        engine.set_lambda_q16(lq)
                        q, cost = engine.refine_ctu(cur_p, (m, m), ref_p, (m, m), api.SearchParams(-SR, -SR, SR, SR, px, py, 1, bd), imv, use_hadamard=bool(had))
                        same_tables(q, cost, want, ("refine_ctu", bd, r, c, had))
                        q, cost = engine.refine_frame(pc, pr, SR, imv[None], np.array([[px, py]], np.int16), use_hadamard=bool(had))
                        same_tables(q[0], cost[0], want, ("refine_frame", bd, r, c, had))
    finally:
        engine.set_lambda(57.9)


@pytest.mark.parametrize("bd", (8, 10))
def test_bi_origin_refinement_on_tap_sign_content(engine, bd):
    """the bi-origin form: current block 2 * cur - other in {2 maxv, -maxv} (staged with the bias 2^bd), hmme_refine_ctu on the origin plane and
    hmme_refine_frame_bi, which builds the origin itself, against ref_frac_refine_bi's recorded answers"""
    from hmme import api, synth
    g = rt.load("ref_refine")
    i, j = list(g["bds"]).index(bd), list(g["bi_bds"]).index(bd)
    m = synth.MARGIN
    imv = np.zeros((593, 2), np.int16)
    org_p = (2 * synth.pad_plane(g["bi_cur"][j]).astype(np.int32) - synth.pad_plane(g["bi_other"][j])).astype(np.int16)
    try:
        with Planes(engine, bd) as mk:
            pc, po = mk(g["bi_cur"][j]), mk(g["bi_other"][j])
            for r in range(4):
                ref_p, pr = synth.pad_plane(g["ref"][i, r]), mk(g["ref"][i, r])
                for had in range(2):
                    lq, px, py = (int(v) for v in g["bi_meta"][j, r, had])
                    want = g["bi"][j, r, had]
                    engine.set_lambda_q16(lq)
                    q, cost = engine.refine_ctu(org_p, (m, m), ref_p, (m, m), api.SearchParams(-SR, -SR, SR, SR, px, py, 1, bd), imv, use_hadamard=bool(had))
                    same_tables(q, cost, want, ("refine_ctu on the origin", bd, r, had))
                    q, cost = engine.refine_frame_bi(pc, pr, po, SR, np.zeros((1, 2), np.int16), imv[None], pred_q=np.array([[px, py]], np.int16),
                                                     use_hadamard=bool(had))
                    same_tables(q[0], cost[0], want, ("refine_frame_bi", bd, r, had))
    finally:
        engine.set_lambda(57.9)


@pytest.mark.parametrize("bd", (8, 9, 10, 11))
def test_origin_form_of_the_prediction(engine, bd):
    """the origin 2 * cur - P that hmme_refine_frame_bi builds from the other list's motion field, P at every phase of the tap-sign content: the
    8x8 slot of each golden block against the reference's bBi refinement of the origin made from ITS recorded block (Hadamard: every sample
    of the origin counts)"""
    g = rt.load("ref_refine")
    j, i = list(g["origin_bds"]).index(bd), BDS.index(bd)
    slots = [int(s) for s in g["origin_slots"]]
    cases = [(3 + n, n >> 1) for n in range(32)]
    imv = np.zeros((1, 593, 2), np.int16)
    engine.set_lambda_q16(int(g["lambda_q16"]))
    try:
        with Planes(engine, bd) as mk:
            pc, pr = mk(g["origin_cur"][j]), mk(g["origin_ref"][j])
            for k, group in enumerate(chunks(cases)):
                other = mk(rt.picture("luma", [rt.source("luma", i, c) for c, _ in group], (1 << bd) >> 1))
                q, cost = engine.refine_frame_bi(pc, pr, other, SR, rt.field("luma", [ph for _, ph in group]), imv, use_hadamard=True)
                for n in range(len(group)):
                    want = g["origin"][j, k * rt.PER_PICTURE + n]
                    got = (int(q[0, slots[n], 0]), int(q[0, slots[n], 1]), int(cost[0, slots[n]]))
                    assert got == tuple(int(v) for v in want), (bd, group[n], got, want.tolist())
    finally:
        engine.set_lambda(57.9)


@pytest.mark.parametrize("bd", BDS)
def test_luma_tails_on_tap_sign_content_of_every_phase(engine, bd):
    """direction 3 of hmme_predict_bi_frame, hmme_predict_frame_w, hmme_predict_refs_w_frame and hmme_predict_bi_w_frame on the tap-sign picture of
    each of the 16 phases (list 0) and its complement (list 1), four weights of HM's range"""
    i = BDS.index(bd)
    T = rt.load("ref_tails")
    fill = (1 << bd) >> 1
    for k, group in enumerate(chunks(list(range(32)))):
        field = rt.field("luma", [n >> 1 for n in group])
        dirs = dirs_field(len(group), 3)
        refs = np.zeros((1, 64), np.uint8)
        refs[0, [rt.block_index(n) for n in range(len(group))]] = 1
        with Planes(engine, bd) as mk:
            a = mk(rt.picture("luma", [rt.source("luma", i, 3 + n) for n in group], fill))
            b = mk(rt.picture("luma", [rt.source("luma", i, 3 + (n ^ 1)) for n in group], fill))
            where = (bd, group)
            check_blocks("luma", engine.predict_bi_frame(a, b, (field, field), dirs), T["sign_avg_luma"][i, group], ("addAvg",) + where)
            for j, kw in enumerate(T["sign_weights"]):
                wp = rt.hmme_weight(T["triples"][kw], bd)
                check_blocks("luma", engine.predict_frame_w(a, wp, field), T["sign_uni_luma"][i, group, j], ("addWeightUni", wp) + where)
                two = engine.predict_refs_w_frame([b, a], [rt.hmme_weight((64, 0, 6), bd), wp], field, refs)
                check_blocks("luma", two, T["sign_uni_luma"][i, group, j], ("predict_refs_w_frame", wp) + where)
                w0, w1 = rt.bi_weights(T["bi_weights"][kw], bd)
                check_blocks("luma", engine.predict_bi_w_frame(a, b, w0, w1, (field, field), dirs), T["sign_bi_luma"][i, group, j], ("addWeightBi", w0, w1) + where)
