"""B pictures with several references per list (hmme_*_bi_refs*, hmme_select_dirs_refs_*, hmme_predict_bi_refs_*), the part that needs no
GPU: the new names declared, exported and bound; hmme_select_dirs_refs_check at every limit include/hmme.h states and at its accepted
neighbour; a NULL context; and the model tests/select_dirs_refs_model.py against its two degenerate cases (select_dirs_model with one
reference per list, select_refs_model with list 1 and bi priced out), at the mask and at every strict comparison of the rule (nothing here
touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bipred_refs_bands as bands
import select_dirs_model as sdm
import select_dirs_refs_model as drm
import select_refs_model as srm
from conftest import ROOT

OK, ERR_ARG = 0, -1
NAMES = ["hmme_search_frame_bi_refs_device", "hmme_refine_frame_bi_refs_device", "hmme_search_frame_bi_refs", "hmme_refine_frame_bi_refs",
         "hmme_select_dirs_refs_check", "hmme_select_dirs_refs_device", "hmme_select_dirs_refs_frame", "hmme_predict_bi_refs_device", "hmme_predict_bi_refs_frame"]


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.build()
    return api


def test_the_new_names_are_declared_exported_and_bound(api):
    L = api.load()
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    declared = set(re.findall(r"\b(hmme_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/hmme.h"
        assert hasattr(L, name), f"libhmme.so does not export {name}"
        assert name in api.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"api.py binds no argument types for {name}"
    for method in ("search_frame_bi_refs", "search_frame_bi_refs_device", "refine_frame_bi_refs", "refine_frame_bi_refs_device", "select_dirs_refs_device",
                   "select_dirs_refs_frame", "predict_bi_refs_device", "predict_bi_refs_frame"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.select_dirs_refs_check) and C.sizeof(api.DirRefsParams) == 4 * (3 + 2 + 16 + 1)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only
    section = header.split("B pictures with several references per list")[1].split("typedef struct hmme_dir_refs_params")[0]
    assert "THIS TEXT PLUS THE CITATIONS IS THE RULE" in section and "Out of scope" in section


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp, sel, dp = api.FrameParams(1, 0, 8, 0, -1), api.SelectParams(64), api.DirRefsParams()
    assert L.hmme_search_frame_bi_refs_device(None, None, None, 1, None, 1, C.byref(fp), None, None, 64, None, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_frame_bi_refs_device(None, None, None, 1, None, 1, C.byref(fp), None, None, 64, None, None, None, 1, None, None, None) == ERR_ARG
    assert L.hmme_search_frame_bi_refs(None, None, None, 1, None, 1, C.byref(fp), None, None, 64, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_frame_bi_refs(None, None, None, 1, None, 1, C.byref(fp), None, None, 64, None, None, None, 1, None, None) == ERR_ARG
    assert L.hmme_select_dirs_refs_device(None, 64, 64, 1, 1, C.byref(fp), C.byref(sel), C.byref(dp), *([None] * 13)) == ERR_ARG
    assert L.hmme_select_dirs_refs_frame(None, 64, 64, 1, C.byref(fp), C.byref(sel), C.byref(dp), *([None] * 12)) == ERR_ARG
    assert L.hmme_predict_bi_refs_device(None, None, 1, None, 1, C.byref(fp), None, None, None, 64, None, 64, None) == ERR_ARG
    assert L.hmme_predict_bi_refs_frame(None, None, 1, None, 1, C.byref(fp), None, None, None, 64, None, 64) == ERR_ARG


def test_select_dirs_refs_check_at_every_limit(api):
    sel, check, D = api.SelectParams(64), api.select_dirs_refs_check, api.DirRefsParams
    assert api.load().hmme_select_dirs_refs_check(None, 1, 1, C.byref(D())) == ERR_ARG
    assert check(sel, 1, 1, None) == ERR_ARG                                  # the bit counts are not optional
    # anything hmme_select_dirs_check refuses: the number of pictures, sel
    for n_pics, want in ((0, ERR_ARG), (1, OK), (4, OK), (5, ERR_ARG), (-1, ERR_ARG), (1 << 30, ERR_ARG)):
        assert check(sel, n_pics, 1, [D()] * 4) == want, n_pics
    for bad in (api.SelectParams(256), api.SelectParams(64, mv_unit=1), api.SelectParams(64, price_mv=1), api.SelectParams(128),
                api.SelectParams(64, part_mask=0x06), api.SelectParams(64, min_depth=2, max_depth=1), api.SelectParams(64, cu_cost=(1 << 20) + 1)):
        assert check(bad, 1, 1, [D()]) == ERR_ARG
        assert api.select_dirs_check(bad, 1, [api.DirParams()]) == ERR_ARG
    # R in 1..8
    for R, want in ((0, ERR_ARG), (1, OK), (8, OK), (9, ERR_ARG), (-1, ERR_ARG), (16, ERR_ARG)):
        assert check(sel, 1, R, [D()]) == want, R
    # n_refs[l] in 1..R, in every picture of the launch
    for R in (1, 3, 8):
        for l in range(2):
            for v, want in ((0, ERR_ARG), (1, OK), (R, OK), (R + 1, ERR_ARG), (-1, ERR_ARG)):
                n = [1, 1]
                n[l] = v
                for pic in range(4):
                    dirs = [D()] * 4
                    dirs[pic] = D(n_refs=n, l1_valid_mask=0)
                    assert check(sel, 4, R, dirs) == want, (R, l, v, pic)
    # any bit count above 4096
    for v, want in ((0, OK), (4096, OK), (4097, ERR_ARG), (0xFFFFFFFF, ERR_ARG)):
        for at in range(3):
            b = [0] * 3
            b[at] = v
            assert check(sel, 2, 8, [D(), D(dir_bits=b, n_refs=(8, 8))]) == want, (v, at)
        for l in range(2):
            for r in range(8):
                rb = [[0] * 8, [0] * 8]
                rb[l][r] = v
                assert check(sel, 2, 8, [D(), D(n_refs=(8, 8), ref_bits=rb)]) == want, (v, l, r)
    assert check(sel, 1, 1, [D(), D(dir_bits=(4097, 0, 0))]) == OK             # only n_pics entries are read
    # l1_valid_mask: bits below n_refs[1] only; empty is fine
    for n1 in (1, 2, 5, 8):
        for mask, want in ((0, OK), ((1 << n1) - 1, OK), (1 << (n1 - 1), OK), (1 << n1, ERR_ARG), ((1 << n1) | 1, ERR_ARG), (0x80000000, ERR_ARG)):
            assert check(sel, 1, 8, [D(n_refs=(3, n1), l1_valid_mask=mask)]) == want, (n1, mask)
    assert check(api.SelectParams(64, cu_cost=1 << 20, pu_cost=1 << 20), 4, 8, [D((4096,) * 3, (8, 8), ([4096] * 8, [4096] * 8), 0xFF)] * 4) == OK


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def as_refs(tabs, R=1):
    """select_dirs_model tables [2, count, ...] with a reference dimension of R behind the list, set 0 the given one, the others dearer copies"""
    out = []
    for k, a in enumerate(tabs[:4]):
        a = np.repeat(a[:, None], R, axis=1)
        out.append(a)
    return out


@pytest.mark.parametrize("w,h", sdm.SIZES)
@pytest.mark.parametrize("bits", [sdm.HM_BITS, ((0, 0, 0), (0, 0)), ((40, 0, 90), (7, 300))])
def test_with_one_reference_per_list_the_model_is_select_dirs_model(api, w, h, bits):
    n = sdm.n_ctus(w, h)
    pred = sdm.predictors(n, seed=31)
    tabs = sdm.random_dir_tables(n, n, seed=32, pred=pred)
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12, min_depth=2 if n == 1 else 0)
    want = sdm.select_dirs_picture(*tabs, sel, w, h, bits, 0, pred)
    rng = np.random.default_rng(33)
    uni_ref = rng.integers(0, 3, size=(2, n, 64)).astype(np.uint8)             # whatever the lists' fields name: carried through under bi blocks only
    b = drm.Bits(bits[0], (1, 1), ([bits[1][0]], [bits[1][1]]), 1)
    field, ref, dirs, slot, cost = drm.select_dirs_refs_picture(*as_refs(tabs), tabs[4], uni_ref, sel, w, h, b, 0, pred[:, None])
    assert np.array_equal(field, want[0]) and np.array_equal(dirs, want[1]) and np.array_equal(slot, want[2]) and np.array_equal(cost, want[3])
    assert bits != sdm.HM_BITS or set(dirs.reshape(-1).tolist()) >= {1, 2}
    # the reference fields: 0 in the winner's list, the input's entry in the other list of a bi block, 0xFF elsewhere
    bl = np.zeros(dirs.shape, int)                                             # the list the bi candidate of the covering slot searched
    for k in range(n):
        m_bl = sdm.merge_ctu(tabs[0][:, k], tabs[1][:, k], tabs[2][:, k], tabs[3][:, k], [pred[l][k] for l in range(2)], bits, sdm.LAMBDA_Q16)[3]
        for blk in range(64):
            if dirs[k, blk] == 3:
                bl[k, blk] = m_bl[slot[k, blk]]
    for l in range(2):
        want_ref = np.where(dirs == l + 1, 0, np.where(dirs == 3, np.where(bl == l, 0, uni_ref[l]), drm.NO_REF))
        assert np.array_equal(ref[l], want_ref.astype(np.uint8)), l


@pytest.mark.parametrize("n_refs", [2, 4])
def test_with_list_1_and_bi_priced_out_the_model_is_the_reference_choice_on_list_0(api, n_refs):
    """list 1's and the bi tables' costs at UINT32_MAX, direction bits 0: list 0's reference r at the price gc-free select_refs_model adds as
    ref_cost -- here through the MV cost: ref_bits enter INSIDE getCost with the MV bits, so the comparison is made at lambda 1 per bit, where
    gc(a + b) = gc(a) + gc(b)"""
    w, h = 136, 72
    n = sdm.n_ctus(w, h)
    lq = 1 << 16
    pred = drm.predictors(n_refs, n, seed=41)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref = drm.random_tables(n_refs, n, n, seed=42, pred=pred, lambda_q16=lq)
    cost_uni = cost_uni.copy()
    cost_uni[1] = 0xFFFFFFFF
    cost_bi = np.full_like(cost_bi, 0xFFFFFFFF)
    ref_bits = [srm.hm_ref_idx_bits(n_refs, r) + 2 for r in range(n_refs)]
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12, min_depth=2)
    b = drm.Bits((0, 0, 0), (n_refs, n_refs), (ref_bits, ref_bits))
    field, ref, dirs, slot, cost = drm.select_dirs_refs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, w, h, b, 0, pred, lq)
    rf, rr, rs, rc_, _ = srm.select_refs_picture(mv_uni[0], cost_uni[0], sel, w, h, ref_bits, 0, pred[0], lq, None)
    assert np.array_equal(slot, rs) and np.array_equal(cost, rc_) and np.array_equal(field[0], rf) and np.array_equal(ref[0], rr)
    assert (field[1] == 0).all() and (ref[1] == drm.NO_REF).all()
    assert np.array_equal(dirs, np.where(rr == srm.NO_REF, drm.NO_DIR, 1).astype(np.uint8))
    assert set(rr.reshape(-1).tolist()) >= set(range(n_refs))                  # every reference wins somewhere


slot, NO_BI, Z = drm.slot_of_lists, drm.NO_BI, drm.Z                           # the hand-made tables' builders: shared with tests/test_gpu_select_dirs_refs.py
dcr = lambda res: (res[0], res[2], res[4])                                     # direction, cost, the two reference indices


def test_the_mask():
    """direction 2 is taken over the references of the mask only; mot[1] and the bi pass still see the unrestricted list 1"""
    flat = lambda n0, n1, mask: drm.Bits((0, 0, 0), (n0, n1), ([0] * n0, [0] * n1), mask)
    # list 1's reference 0 is the cheapest of all: it wins direction 2 when allowed, reference 1 does when 0 is masked out, list 0 when none is
    args = ([[Z], [Z, Z]], [[500], [100, 300]], [[Z], [Z, Z]], [[NO_BI], [NO_BI, NO_BI]])
    assert dcr(slot(*args, flat(1, 2, 0b11))) == (2, 100, (drm.NO_REF, 0))
    assert dcr(slot(*args, flat(1, 2, 0b10))) == (2, 300, (drm.NO_REF, 1))
    assert dcr(slot(*args, flat(1, 2, 0b00))) == (1, 500, (0, drm.NO_REF))
    # an empty mask: direction 2 never wins, whatever list 1 costs -- and bi is compared with list 0 alone: a bi cost of 994 is a distortion
    # of (994 - 2) >> 1 = 496 plus gc(2 + mot[1] = 2): 500, the tie bi wins
    assert dcr(slot([[Z], [Z]], [[500], [0]], [[Z], [Z]], [[NO_BI], [NO_BI]], flat(1, 1, 0))) == (1, 500, (0, drm.NO_REF))
    assert dcr(slot([[Z], [Z]], [[500], [0]], [[Z], [Z]], [[994], [NO_BI]], flat(1, 1, 0))) == (3, 500, (0, drm.NO_REF))
    assert dcr(slot([[Z], [Z]], [[500], [0]], [[Z], [Z]], [[994], [NO_BI]], flat(1, 1, 1))) == (2, 2, (drm.NO_REF, 0))   # max(0, 0 - 2) + gc(2)
    # a masked-out cheaper reference still sets mot[1]: list 1's reference 0 (cost 100, an MV of 2 bits, ref_bits 0) against reference 1 (MV
    # (40, 0): 13 + 1 = 14 bits, ref_bits 9, C = 2000 - 14 + 9 + 14 = 2009).  The bi cost of list 0 carries mot[1] of the UNRESTRICTED winner,
    # reference 0: 0 + 2; with the masked winner's motion it were 1000 + 2 + 23
    bits = drm.Bits((0, 0, 0), (1, 2), ([0], [0, 9]), 0b10)
    far = (40, 0)
    assert sdm.mvb(far, Z) == 14
    d, bl, c, m, refs = slot([[Z], [Z, far]], [[5000], [100, 2000]], [[Z], [Z, Z]], [[2 * 1000 + 2], [NO_BI, NO_BI]], bits)
    assert (d, bl, c, refs) == (3, 0, 1000 + 2 + 2, (0, drm.NO_REF))
    d, _, c, m, refs = slot([[Z], [Z, far]], [[5000], [100, 2000]], [[Z], [Z, Z]], [[NO_BI], [NO_BI, NO_BI]], bits)
    assert (d, c, tuple(m), refs) == (2, 2009, far, (drm.NO_REF, 1))            # direction 2 itself is the masked-in reference 1


def test_every_strict_comparison():
    flat = lambda n0, n1, mask=None: drm.Bits((0, 0, 0), (n0, n1), ([0] * n0, [0] * n1), mask)
    a, b_ = (4, 0), (0, 4)                                                     # two MVs of equal bit count, told apart in the result
    bbits = sdm.mvb(a, Z)
    assert bbits == sdm.mvb(b_, Z) == 8
    # rule 1: the first of equal uni costs wins, a strictly cheaper later one does (:3086)
    for l in range(2):
        mu, cu = [[Z], [Z]], [[9000], [9000]]
        mu[l], cu[l] = [a, b_, a], [700, 700, 700]
        d, _, c, m, refs = slot(mu, cu, [[Z] * 3] * 2, [[NO_BI] * 3] * 2, flat(3 if l == 0 else 1, 3 if l == 1 else 1))
        assert (d, c, tuple(m), refs[l]) == (l + 1, 700, a, 0)
        cu[l] = [700, 699, 699]
        d, _, c, m, refs = slot(mu, cu, [[Z] * 3] * 2, [[NO_BI] * 3] * 2, flat(3 if l == 0 else 1, 3 if l == 1 else 1))
        assert (d, c, tuple(m), refs[l]) == (l + 1, 699, b_, 1)
    # rule 2: the same inside the mask
    d, _, c, m, refs = slot([[Z], [a, b_, a]], [[9000], [600, 700, 700]], [[Z] * 3] * 2, [[NO_BI] * 3] * 2, flat(1, 3, 0b110))
    assert (d, c, tuple(m), refs) == (2, 700, b_, (drm.NO_REF, 1))
    # rule 3: the first of equal bi costs per list (:3226); list 0's bi candidate unless list 1's is strictly cheaper.  A bi cost of
    # 2 v + bbits is a distortion of v; the candidate adds gc(bbits + mot[1-l]) with mot = 0 + mvb(Z) = 2
    uni = ([[Z, Z], [Z, Z]], [[9000, 9000], [9000, 9000]])
    bi = lambda c0, c1: [[2 * v + bbits for v in c0], [2 * v + bbits for v in c1]]
    tot = lambda v: v + bbits + 2
    d, bl, c, m, refs = slot(*uni, [[a, b_], [b_, a]], bi([500, 500], [500, 500]), flat(2, 2))
    assert (d, bl, c, tuple(m), refs) == (3, 0, tot(500), a, (0, drm.NO_REF))
    d, bl, c, m, refs = slot(*uni, [[a, b_], [b_, a]], bi([500, 499], [499, 499]), flat(2, 2))
    assert (d, bl, c, tuple(m), refs) == (3, 0, tot(499), b_, (1, drm.NO_REF))   # list 0's later reference strictly cheaper; list 1 ties: list 0 stays
    d, bl, c, m, refs = slot(*uni, [[a, b_], [b_, a]], bi([500, 500], [500, 499]), flat(2, 2))
    assert (d, bl, c, tuple(m), refs) == (3, 1, tot(499), a, (drm.NO_REF, 1))
    # rule 4: bi wins ties against both lists, list 0 wins ties against list 1 (:3291, :3314)
    t = tot(500)
    one = lambda c0, c1, mask=None: slot([[Z], [Z]], [[c0], [c1]], [[a], [a]], bi([500], [600]), flat(1, 1, mask))
    assert one(t, t)[0] == 3 and one(t - 1, t)[0] == 1 and one(t, t - 1)[0] == 2 and one(t - 1, t - 1)[0] == 1 and one(t - 1, t - 2)[0] == 2
    assert one(t, t - 1, 0)[0] == 3 and one(t - 1, 0, 0)[0] == 1               # ... and against list 0 alone with an empty mask


tie_bits = drm.tie_bits


def test_the_tie_scenarios_price_as_stated_and_decide_as_stated(api):
    """select_dirs_refs_model.tie_scenarios: under either set of bit counts the tables of tie_slot_tables price at exactly the stated costs,
    slot_decide makes of them what the scenario states, and the picture of tie_tables codes every site, so every scenario shows in the field"""
    scenarios = drm.tie_scenarios()
    assert len(scenarios) >= 16 and {v[0] for v in scenarios.values()} == {drm.TIE_MASK, 0}
    assert len({sdm.mvb(m, Z) for m in drm.TIE_MVS}) == 1 and len(set(drm.TIE_MVS)) == 4
    gc, mvb = sdm.gc, sdm.mvb
    for name, sc in scenarios.items():
        for bits in tie_bits(sc[0]):
            mu, cu, mb, cb = drm.tie_slot_tables(*sc[1:5], bits)
            lq = drm.TIE_LAMBDA_Q16
            priced = [[int(cu[l][r]) - gc(lq, mvb(mu[l][r], Z)) + gc(lq, bits.dir_bits[l] + bits.ref_bits[l][r] + mvb(mu[l][r], Z)) for r in range(3)] for l in range(2)]
            assert priced == [list(sc[1]), list(sc[2])], name
            d, bl, c, m, refs = drm.slot_decide(mu, cu, mb, cb, [[Z] * 3] * 2, bits, lq)
            wd, wbl, wm, wrefs = drm.tie_want(bits.l1_valid_mask, sc)
            assert (d, tuple(m), refs) == (wd, wm, wrefs) and (d != 3 or bl == wbl), (name, d, bl, m, refs)
            assert c == min(v for v in sc[1] + (sc[2][1:] if sc[0] else []) + sc[3] + sc[4]), name      # the winner's priced cost: the least of those allowed
    # in every masked scenario list 1's cheapest reference is the one outside the mask
    assert all(sc[2].index(min(sc[2])) == 0 and not drm.TIE_MASK & 1 for sc in scenarios.values() if sc[0])
    sel = api.SelectParams(64)
    for mask in (drm.TIE_MASK, 0):
        for bits in tie_bits(mask):
            tabs, placed = drm.tie_tables(bits)
            field, ref, dirs, slot_, cost = drm.select_dirs_refs_picture(*tabs, sel, 64, 64, bits, 0, None, drm.TIE_LAMBDA_Q16)
            assert set(slot_.reshape(-1).tolist()) == set(placed) and len(placed) == 25
            assert {placed[s] for s in placed} == {k for k, v in scenarios.items() if v[0] == mask}
            assert len({d for _, d in drm.tie_sites()}) == 3


def test_the_model_carries_its_sums_unwrapped_and_its_products_wrapped():
    # sums: list 0's reference 1 prices at 0xFFFFF000 - 2 + gc(4096 + 2) = 2^32 exactly, reference 0 at 2^32 - 1: reference 0 stays the
    # winner, which list 1's bi candidate shows through mot[0] = 0 + 2 (a wrapped sum would make it 4096 + 2)
    bits = drm.Bits((0, 0, 0), (2, 1), ([0, 4096], [0]))
    d, bl, c, _, refs = slot([[Z, Z], [Z]], [[0xFFFFFFFF, 0xFFFFF000], [0xFFFFFFFF]], [[Z, Z], [Z]], [[NO_BI, NO_BI], [2 * 1000 + 2]], bits)
    assert (d, bl, c, refs) == (3, 1, 1000 + 2 + 2, (drm.NO_REF, 0))
    # products: at lambda_q16 = 2^30 gc(2) = 32768 and gc(4) = 0 (HM's 32-bit product): a cost of 1000 under gc(2) leaves a distortion of 0,
    # and the bits put back cost nothing; a 64-bit product would price them at 65536
    bits = drm.Bits((0, 0, 0), (1, 1), ([2], [0]))
    assert sdm.gc(1 << 30, 2) == 32768 and sdm.gc(1 << 30, 4) == 0
    assert dcr(slot([[Z], [Z]], [[1000], [5000]], [[Z], [Z]], [[NO_BI], [NO_BI]], bits, 1 << 30)) == (1, 0, (0, drm.NO_REF))


def test_the_recipes_of_the_gpu_cases_exercise_directions_references_and_the_mask(api):
    w, h = 136, 72
    n = sdm.n_ctus(w, h)
    sel = api.SelectParams(64, min_depth=2)
    for n0, n1, mask in ((1, 1, None), (2, 2, 0b10), (4, 4, 0b0101), (3, 1, None)):
        R = max(n0, n1)
        pred = drm.predictors(R, n, seed=51 + R)
        tabs = drm.random_tables(R, n, n, seed=52 + n0 + n1, pred=pred)
        field, ref, dirs, slot_, cost = drm.select_dirs_refs_picture(*tabs, sel, w, h, drm.hm_bits(n0, n1, mask), 0, pred)
        assert set(dirs.reshape(-1).tolist()) == {1, 2, 3, drm.NO_DIR}, (n0, n1)
        full = (1 << n1) - 1 if mask is None else mask
        assert set(ref[1][dirs == 2].tolist()) == {r for r in range(n1) if (full >> r) & 1}, (n0, n1)
        assert set(ref[0][dirs == 1].tolist()) == set(range(n0)), (n0, n1)
        assert set(ref[0][dirs == 3].tolist()) <= set(range(R)) and set(ref[1][dirs == 3].tolist()) <= set(range(R))
        assert ((dirs == drm.NO_DIR) == (ref[0] == drm.NO_REF) & (ref[1] == drm.NO_REF) & (field == 0).all(axis=(0, 3))).all()


# ---- the end-to-end content of tests/test_gpu_bipred_refs.py ---------------------------------------------------------------------------------
def test_the_numpy_route_alone_finds_the_planted_bands(api, oracle_lib):
    """the oracle's searches and refinements and the models' decisions on tests/bipred_refs_bands.py: every 8x8 block at least 8 samples
    inside a band carries the planted direction and reference indices"""
    from frame_helpers import bind_hmo
    cur, lists = bands.content()
    got = bands.numpy_route(oracle_lib, bind_hmo(oracle_lib), cur, lists, sdm.LAMBDA_Q16, api.SelectParams(64))
    planted = bands.planted_blocks()
    assert {(d, refs) for _, _, d, refs in planted} == {(d, refs) for _, _, d, refs in bands.BANDS} and len(planted) >= 60
    assert bands.bands_hold(got["dirs"], got["ref"]) == []
    assert (got["dirs"] == drm.NO_DIR).sum() == 6 * 64 - 17 * 9                # the blocks outside the picture, and only they
