"""The bent pictures of tests/spectral_content.py are what they claim, and the oracle agrees with an int64 restatement on them (no GPU):
tests/test_gpu_refine_spectral.py then holds the device to the oracle on the same inputs.  One 64x64 CTU, integer MV 0, edge-replicated.

`complement` (reference = maxv - current, difference +-maxv in the H8 pattern): the integer-position Hadamard sum of every slot is
w * h * 2 * maxv >> (bd - 8), the bound the packed 21-bit sums of the 8-bit refinement kernel are sized for.  The oracle's figures, pinned below:

  bit depth   the nine half-pel sums of slot 592 (64x64) in HM's point order, after >> (bd - 8)                             least of the other 48
   8          2 088 960, 1 562 976 x4, 1 277 042, 1 568 716, 1 568 716, 1 233 592                                        973 906
  10          2 095 104, 1 567 608 x4, 1 280 712, 1 573 382, 1 573 382, 1 237 507                                        976 712
  12          2 096 640, 1 568 766 x4, 1 281 556, 1 574 398, 1 574 409, 1 238 419                                        977 484

  largest advantage over the integer point, block sums >> (bd - 8)      half-pel point: 8x8 / 4x4 block     quarter-pel ring: 8x8 / 4x4 block
   8                                                                     13 926 / 3 818                      5 940 / 1 686
  10                                                                     13 960 / 3 829                      5 966 / 1 693
  12                                                                     13 970 / 3 832                      5 972 / 1 694

At 8 bit these are the figures of the issue that asked for this file.  With the predictor on the integer MV a half-pel neighbour costs 4 bits
more than the centre and a quarter-pel neighbour 2; at lambda_q16 = 1 << 28 (4096 per bit; at most 10 bits here, the 32-bit product does not
wrap) that is 16 384 and 8 192, above the advantages of an 8x8 block and of the four 4x4 blocks of a 16x4 sliver (15 328 / 6 776 at 12 bit).  So
the integer point wins both stages in EVERY slot of at most 64 samples at every bit depth -- 384 slots: the 320 of the 8x8 CUs and the 64 AMP
slivers (16x4, 4x16) of the 16x16 CUs -- and no slot class is left out; the cost reported there is the bound plus the MV cost."""
import ctypes as C
import functools

import numpy as np
import pytest

import range_content as rc
import residual_model as rm
import spectral_content as sc
from frame_helpers import bind_hmo
from tie_content import REFINE_H

LQ_TOP = 1 << 28
LAMBDAS = (0, 3794534, LQ_TOP)
PREDS = ((0, 0), (0, -2))
HALF_PEL_592 = {
    8: (2088960, 1562976, 1562976, 1562976, 1562976, 1277042, 1568716, 1568716, 1233592),
    10: (2095104, 1567608, 1567608, 1567608, 1567608, 1280712, 1573382, 1573382, 1237507),
    12: (2096640, 1568766, 1568766, 1568766, 1568766, 1281556, 1574398, 1574409, 1238419),
}
LEAST_OTHER_592 = {8: 973906, 10: 976712, 12: 977484}
ADVANTAGE = {8: ((13926, 3818), (5940, 1686)), 10: ((13960, 3829), (5966, 1693)), 12: ((13970, 3832), (5972, 1694))}   # (half 8x8, 4x4), (quarter ring)


@functools.lru_cache(maxsize=None)
def pair(kind, bd):
    p = sc.bent_pair(kind, 64, 64, bd)
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def sums(kind, bd):
    return sc.position_sums(*pair(kind, bd), bd)


def oracle_refine(oracle_lib, org, ref, bd, lq, had, pred):
    from hmme import synth
    m = synth.MARGIN
    q, c = oracle_lib.refine_frame(org, ref, (m, m), 64, 64, np.zeros((1, 593, 2), np.int16), np.array([pred], np.int16), lq, had, bd)
    return q[0].astype(np.int64), c[0].astype(np.int64)


def test_the_pattern_is_bent_and_the_pictures_are_what_they_claim():
    h8 = sc.bent_sign(8, 8)
    assert np.array_equal(h8, rm._hadamard(8)) and (np.abs(h8 @ h8 @ h8.T) == 8).all()
    for bd in (8, 10, 12):
        maxv = (1 << bd) - 1
        cur = sc.bent_plane(64, 64, bd)
        d = cur - sc.complement(cur, bd)
        assert set(np.unique(cur)) == {0, maxv} and np.array_equal(d, maxv * sc.bent_sign(64, 64))
        blk = d[8:16, 24:32]
        assert rm.had_abs_sum(blk) == 512 * maxv == rm.had8_from_quadrants(blk) and rm.had_rule(blk, 8) == (512 * maxv + 2) >> 2 == 128 * maxv
        assert all(rm.had_rule(blk[y:y + 4, x:x + 4], 8) == (64 * maxv + 1) >> 1 == 32 * maxv for y in (0, 4) for x in (0, 4))
    assert len(sc.small_slots()) == 384 and sum(1 for _, _, w, h in sc.slot_rects() if max(w, h) <= 8) == 320
    assert sc.slot_bound(592, 8, 255) == 2088960 == (1 << 21) - 8192 and sc.slot_bound(592, 12, 4095) == (4096 * 2 * 4095) >> 4


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_complement_reaches_the_bound_and_the_oracle_reports_it(oracle_lib, bd):
    maxv = (1 << bd) - 1
    cur, ref = pair("complement", bd)
    s = sums("complement", bd)
    # every slot at the integer position: the bound, by the restatement
    assert all(int(s[0, 0][1][k]) >> (bd - 8) == sc.slot_bound(k, bd, maxv) for k in range(593))
    assert all(int(s[0, 0][0][k]) >> (bd - 8) == sc.slot_bound(k, bd, maxv) >> 1 for k in range(593))          # SAD: w * h * maxv
    # the figures of the docstring: from the oracle's interpolation and Hadamard, equal to the restatement's
    from hmme import synth
    hmo, m = bind_hmo(oracle_lib), synth.MARGIN
    p16 = C.POINTER(C.c_int16)
    at = lambda a: C.cast(a.ctypes.data + 2 * (m * a.shape[1] + m), p16)
    blk = np.zeros((64, 64), np.int16)
    nine = []
    for hx, hy in REFINE_H:
        hmo.hmo_pred_block_qpel(at(ref), ref.shape[1], 64, 64, 2 * hx, 2 * hy, bd, C.cast(blk.ctypes.data, p16), 64)
        nine.append(int(hmo.hmo_had(at(cur), cur.shape[1], C.cast(blk.ctypes.data, p16), 64, 64, 64, bd)))
    print(f"bd {bd}: half-pel sums of slot 592 {nine}")
    assert tuple(nine) == HALF_PEL_592[bd] == tuple(int(s[2 * hx, 2 * hy][1][592]) >> (bd - 8) for hx, hy in REFINE_H)
    assert min(nine) > 1 << 20 and nine[0] == sc.slot_bound(592, bd, maxv)
    assert min(int(v[1][592]) >> (bd - 8) for p, v in s.items() if p != (0, 0)) == LEAST_OTHER_592[bd]
    b0 = sc.block_maps(sc.ctu_difference(cur, ref, bd, 0, 0))
    rings = ([(2 * x, 2 * y) for x, y in REFINE_H[1:]], [(x, y) for x, y in REFINE_H[1:]])
    adv = tuple(tuple(max(int(((b0[k] >> (bd - 8)) - (sc.block_maps(sc.ctu_difference(cur, ref, bd, *p))[k] >> (bd - 8))).max()) for p in ring)
                      for k in (0, 1)) for ring in rings)
    print(f"bd {bd}: largest advantage over the integer point (8x8, 4x4 block): half-pel {adv[0]}, quarter-pel ring {adv[1]}")
    assert adv == ADVANTAGE[bd]
    assert adv[0][0] < 4 * 4096 and 4 * adv[0][1] < 4 * 4096 and adv[1][0] < 2 * 4096 and 4 * adv[1][1] < 2 * 4096
    # the oracle against the restatement, all 593 slots, both predictors
    for had in (1, 0):
        for lq in LAMBDAS:
            for pred in PREDS:
                q, c = oracle_refine(oracle_lib, cur, ref, bd, lq, had, pred)
                mq, mc = sc.refine_model(s, had, bd, lq, pred)
                assert np.array_equal(q, mq) and np.array_equal(c, mc), (bd, had, lq, pred, np.argwhere(c != mc)[:4])
    # lambda_q16 = 1 << 28, predictor = integer MV: the integer point wins in every slot of at most 64 samples; its cost is the bound + the MV cost
    assert max(sc.component_bits(v) for v in range(-3, 4)) * 2 * LQ_TOP < 1 << 32
    q, c = oracle_refine(oracle_lib, cur, ref, bd, LQ_TOP, 1, (0, 0))
    small = sc.small_slots()
    assert (q[small] == 0).all()
    assert all(int(c[k]) == sc.slot_bound(k, bd, maxv) + sc.mv_cost(LQ_TOP, 0, 0, (0, 0)) for k in small) and sc.mv_cost(LQ_TOP, 0, 0, (0, 0)) == 8192
    # the other predictor moves every one of them off the centre: the packed fields next to the one at its bound decide
    q, _ = oracle_refine(oracle_lib, cur, ref, bd, LQ_TOP, 1, PREDS[1])
    assert (np.abs(q[small]).sum(axis=1) > 0).all()


@pytest.mark.parametrize("kind", ["flat0", "flatmax"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_flat_references_tie_everywhere_and_the_integer_point_wins(oracle_lib, bd, kind):
    cur, ref = pair(kind, bd)
    s = sums(kind, bd)
    assert all(np.array_equal(v, s[0, 0]) for v in s.values()), "all 49 positions tie"
    for had in (1, 0):
        for lq in (0, LQ_TOP):
            q, c = oracle_refine(oracle_lib, cur, ref, bd, lq, had, (0, 0))
            assert (q == 0).all(), (bd, kind, had, lq)
            want = (s[0, 0][had] >> (bd - 8)) + sc.mv_cost(lq, 0, 0, (0, 0))
            assert np.array_equal(c, want), (bd, kind, had, lq)
    top = int(s[0, 0][1][592]) >> (bd - 8)
    assert top > 1 << 20
    if bd == 8:   # 64 blocks of 18 360 / 17 850
        assert top == {"flat0": 1175040, "flatmax": 1142400}[kind]


@pytest.mark.parametrize("bd", [8, 10, 11])
def test_bi_origin_doubles_the_difference(oracle_lib, bd):
    from hmme import api, synth
    m, maxv = synth.MARGIN, (1 << bd) - 1
    cur, ref, other = sc.bi_triple(64, 64, bd)
    org = 2 * cur[m:m + 64, m:m + 64].astype(np.int64) - other[m:m + 64, m:m + 64]          # the other list's prediction at MV 0: its samples
    assert org.max() == 2 * maxv and org.min() == -maxv
    org_padded = np.ascontiguousarray(np.pad(org, m).astype(np.int16))
    s = sc.position_sums(org_padded, ref, bd)
    assert np.array_equal(sc.ctu_difference(org_padded, ref, bd, 0, 0), 2 * maxv * sc.bent_sign(64, 64))
    assert all(int(s[0, 0][1][k]) >> (bd - 8) == sc.slot_bound(k, bd, 2 * maxv) for k in range(593))
    assert api.bipred_check(bd, True) == 0
    for had in (1, 0):
        for lq in (0, 3794534):
            q, c = oracle_refine(oracle_lib, org_padded, ref, bd, lq, had, (0, 0))
            mq, mc = sc.refine_model(s, had, bd, lq, (0, 0))
            assert np.array_equal(q, mq) and np.array_equal(c, mc), (bd, had, lq)
    # the advantages of the other points double with the difference: at 1 << 28 the 4 bits of a half-pel neighbour (16 384) still outweigh
    # those of two 4x4 blocks, so the integer point wins in the 8x4 and 4x8 slots and the oracle reports their bound
    q, c = oracle_refine(oracle_lib, org_padded, ref, bd, LQ_TOP, 1, (0, 0))
    small32 = [k for k, (_, _, w, h) in enumerate(sc.slot_rects()) if w * h == 32]
    assert 2 * 2 * ADVANTAGE[12][0][1] < 4 * 4096 and 2 * 2 * ADVANTAGE[12][1][1] < 2 * 4096
    assert len(small32) == 256 and (q[small32] == 0).all() and all(int(c[k]) == sc.slot_bound(k, bd, 2 * maxv) + 8192 for k in small32)


def test_bi_refinement_is_still_refused_at_12_bits():
    from hmme import api
    assert api.bipred_check(12, True) == -5 and api.bipred_check(12, False) == 0      # 4096 * 2 * 4095 >= 2^24
    assert 4096 * 2 * 4095 >= 1 << 24 > 4096 * 2 * 2047


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_inverting_weight_makes_the_picture_its_own_reference(bd):
    maxv = (1 << bd) - 1
    wp = (-64, maxv, 6, 32)
    cur, ref = sc.weighted_pair(64, 64, bd, wp)
    assert np.array_equal(cur, ref) and sc.weighted_differences(bd, wp) == (maxv, -maxv)
    d = sc.ctu_difference(cur, ref, bd, 0, 0, wp=wp)
    assert np.array_equal(d, maxv * sc.bent_sign(64, 64))
    for family, member in rc.families(bd).items():
        w = member(3)
        a, b = sc.weighted_differences(bd, w)
        d = sc.ctu_difference(*sc.weighted_pair(64, 64, bd, w), bd, 0, 0, wp=w)
        assert np.array_equal(d, np.where(sc.bent_sign(64, 64) > 0, a, b)) and max(abs(a), abs(b)) == rc.span_of(bd, w), (bd, family)


def test_packed_fields_hold_the_bound():
    """pk[k] of me_frac_compute in Python integers.  Up to sixteen lanes add to one slot, each the sum of ITS blocks: the contributions are
    disjoint parts of the slot, so per field they add up to at most the slot's bound -- never sixteen times it"""
    bound = 64 * 32640
    pack = lambda d0, d1, d2: ((d0 | d1 << 21) & 0xffffffff) | ((d1 >> 11 | d2 << 10) & 0xffffffff) << 32
    unpack = lambda v: (v & 0x1fffff, (v >> 21) & 0x1fffff, v >> 42)
    assert bound == 2088960 == (1 << 21) - 8192
    for trio in ((bound, bound, bound), (bound, 0, bound), (0, bound, 0)):
        assert unpack(pack(*trio)) == trio
        assert unpack(sum(pack(*(v // 16 for v in trio)) for _ in range(16)) & (1 << 64) - 1) == trio           # 4 blocks of 32 640 per lane
    assert unpack(pack(bound, 0, 0) + pack(8192, 0, 0)) == (0, 1, 0), "one more than the headroom carries into the neighbour"
