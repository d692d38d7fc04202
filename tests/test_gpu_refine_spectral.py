"""The refinement kernel (me_frac_kernel<HAD, BPS, WP>) and the residual's Hadamard sums AT their spectral maximum: tests/spectral_content.py's
pictures put a difference of +-span in the sign pattern of the Sylvester matrix H8 into every 8x8 block, so every 8x8 and every 4x4 Hadamard
block reaches Parseval's bound at once and the integer-position sum of every slot is w * h * 2 * span -- at 8 bit the 64x64 slot's 2 088 960,
8 192 below the 2^21 of a packed sum field, with the other eight fields of the slot above 2^20.  tests/test_spectral_cpu.py holds the oracle
to an int64 restatement on the same inputs; everything here is bit for bit against the oracle, MVs and costs, all 593 slots.  Where the
integer point wins (slots of at most 64 samples under lambda_q16 = 1 << 28, flat references everywhere) the cost read from the device IS the
bound plus the MV cost, and is asserted as such.  Pictures are one CTU (64 x 64) or 136 x 72 (3 x 2 CTUs, partial on the right, at the
bottom and in the corner); one refinement launch per case.

Seen to fail on builds with a wrong kernel (scratch builds, wrong results only), first failing case of each:
  20-bit fields in the packed sums (the shift and mask constants    test_plain_refinement_of_one_ctu[8-1-complement], lambda 0, predictor on the integer
  of pk[k] and of the winners' unpack alone: 20 / 12 / 8, 40)       MV: slot 578 (a 64x48) MV (-2, -1) for (3, 3); 9 tests fail, all 8 bit Hadamard
  no `+ 2` in the 8x8 rounding of the refinement's Hadamard         test_plain_refinement_of_one_ctu[8-1-complement], lambda 0: slot 384 (an 8x8) cost
                                                                    15 866 for 15 867; 15 tests fail (no flat case: 64 * 255 is a multiple of 4)
  the clip of a biased bi-prediction origin's prediction to         test_per_ctu_call[origin-8], lambda_q16 1 << 28: slot 256 (a 16x4) MV (0, 1) for
  [0, maxv] instead of [2^bd, 2^bd + maxv] (clip_lo = 0)            (0, 0); 3 tests fail, the three per-CTU origins -- the picture-level bi calls
                                                                    refine on the raw reference and take the bias off the origin (FracWp::org_sub)
"""
import functools

import numpy as np
import pytest

import range_content as rc
import residual_model as rm
import spectral_content as sc
from frame_helpers import bind_hmo, mkplane, oracle_origin_refine_w, oracle_prediction, origin_picture

pytestmark = pytest.mark.gpu

LQ_TOP = 1 << 28                       # 4096 per bit: the largest power of two whose product with the 10 bits of a refinement MV stays below 2^32
LAMBDAS = (0, 3794534, LQ_TOP)         # none, lambda 57.9, the top
PREDS = ((0, 0), (0, -2))              # on the integer MV; two quarter-pels above it: the half-pel point (0, -1) is then the cheapest
EW, EH, E_CTU = 136, 72, 6
SR = 8
M = 80                                 # margin of the hand-made planes of the per-CTU calls: a multiple of 8, the pattern runs through


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


@functools.lru_cache(maxsize=None)
def pair(kind, w, h, bd):
    p = sc.bent_pair(kind, w, h, bd)
    for a in p:
        a.setflags(write=False)
    return p


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def preds_of(pred, n):
    return np.tile(np.array(pred, np.int16), (n, 1))


def same(q, c, oq, oc, *what):
    """device tables == oracle tables; the message names the first differing (CTU, slot) with the device's and the oracle's value"""
    bad_q, bad_c = np.argwhere((q != oq).any(axis=-1))[:3], np.argwhere(c != oc)[:3]
    assert len(bad_q) == 0, f"{what}: MV of (CTU, slot) " + ", ".join(f"({a}, {b}) {q[a, b].tolist()} != {oq[a, b].tolist()}" for a, b in bad_q)
    assert len(bad_c) == 0, f"{what}: cost of (CTU, slot) " + ", ".join(f"({a}, {b}) {int(c[a, b])} != {int(oc[a, b])}" for a, b in bad_c)


def plain(engine, oracle_lib, kind, w, h, bd, had, lq, pred, imv=(0, 0), planes=None):
    """one refine_frame launch against the oracle's frame refinement -> (qmv, cost) of the device"""
    from hmme import synth
    m, n = synth.MARGIN, n_ctus(w, h)
    cur, ref = planes if planes is not None else pair(kind, w, h, bd)
    int_mv = np.tile(np.array(imv, np.int16), (n, 593, 1))
    pq = preds_of(pred, n)
    engine.set_lambda_q16(lq)
    pc, pr = mkplane(engine, cur, w, h, bd), mkplane(engine, ref, w, h, bd)
    try:
        q, c = engine.refine_frame(pc, pr, SR, int_mv, pq, use_hadamard=bool(had))
    finally:
        pc.close(); pr.close()
    oq, oc = oracle_lib.refine_frame(cur, ref, (m, m), w, h, int_mv, pq, lq, had, bd, n_threads=8)
    same(q, c, oq, oc, kind, (w, h), bd, had, lq, pred)
    return q, c


# ---- 1: plain refinement, <1,1,0> <0,1,0> <1,2,0> <0,2,0> ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("had", [1, 0])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_plain_refinement_of_one_ctu(engine, oracle_lib, bd, had, kind):
    maxv = (1 << bd) - 1
    small = sc.small_slots()
    for lq in LAMBDAS:
        for pred in PREDS:
            q, c = plain(engine, oracle_lib, kind, 64, 64, bd, had, lq, pred)
            if kind != "complement":
                # all 49 positions tie: with the predictor on the integer MV that point wins everywhere, and so it does without an MV cost
                if pred == (0, 0) or lq == 0:
                    assert (q == 0).all(), (bd, had, kind, lq, pred)
                if bd == 8 and had:
                    assert int(c[0, 592]) >> 20 & 1 and int(c[0, 592]) < 1 << 21, "the 64x64 sum of a flat reference: above 2^20 in all nine fields"
            elif lq == LQ_TOP and pred == (0, 0):
                # the integer point wins in every slot of at most 64 samples: the device reports the bound itself (SAD: half of it)
                assert (q[0, small] == 0).all()
                assert all(int(c[0, s]) == (sc.slot_bound(s, bd, maxv) >> (0 if had else 1)) + sc.mv_cost(lq, 0, 0, pred) for s in small), (bd, had)
            elif lq == LQ_TOP:
                assert (np.abs(q[0, small]).sum(axis=1) > 0).all(), "a predictor off the integer MV moves every small slot off it"


@pytest.mark.parametrize("kind,bd,had,lq,pred", [("complement", 8, 1, LQ_TOP, (0, 0)), ("complement", 8, 1, 0, (0, -2)), ("flat0", 8, 1, 3794534, (0, 0)),
                                                 ("complement", 10, 1, 3794534, (0, -2)), ("flatmax", 12, 0, LQ_TOP, (0, 0))])
def test_plain_refinement_of_six_ctus(engine, oracle_lib, kind, bd, had, lq, pred):
    """136 x 72: the edge CTUs complete their blocks by edge replication, which breaks the pattern there; CTU 0 is whole"""
    q, c = plain(engine, oracle_lib, kind, EW, EH, bd, had, lq, pred)
    if kind == "complement" and lq == LQ_TOP:
        small = sc.small_slots()
        assert (q[0, small] == 0).all() and all(int(c[0, s]) == sc.slot_bound(s, bd, (1 << bd) - 1) + 8192 for s in small)


# ---- 2: the per-CTU call: another staging path into the same kernel; a bi-prediction origin there runs on biased samples ---------------------
def ctu_planes(kind, bd):
    """-> (cur, ref) int16 planes of one CTU at (M, M), the pattern continued through the M samples around it.  kind `origin`: the current
    block is the bi-prediction origin 2 * cur - other with other = the complement = the reference: samples in {2 * maxv, -maxv}"""
    n, maxv = 64 + 2 * M, (1 << bd) - 1
    pos = sc.bent_sign(n, n) > 0
    cur = np.where(pos, maxv, 0)
    ref = {"complement": maxv - cur, "flat0": np.zeros_like(cur), "origin": maxv - cur}[kind]
    if kind == "origin":
        cur = 2 * cur - ref
    return np.ascontiguousarray(cur.astype(np.int16)), np.ascontiguousarray(ref.astype(np.int16))


@pytest.mark.parametrize("kind,bd", [("complement", 8), ("flat0", 8), ("origin", 8), ("origin", 10), ("origin", 11)])
def test_per_ctu_call(engine, oracle_lib, kind, bd):
    from hmme import api
    maxv = (1 << bd) - 1
    cur, ref = ctu_planes(kind, bd)
    if kind == "origin":
        assert cur.max() == 2 * maxv and cur.min() == -maxv
    table = oracle_lib.slot_table()
    imv = np.zeros((593, 2), np.int16)
    for lq, pred in ((LQ_TOP, (0, 0)), (0, (0, -2)), (3794534, (0, -2))):
        engine.set_lambda_q16(lq)
        q, c = engine.refine_ctu(cur, (M, M), ref, (M, M), api.SearchParams(-SR, -SR, SR, SR, pred[0], pred[1], 1, bd), imv, use_hadamard=True)
        oq, oc = np.zeros_like(q), np.zeros_like(c)
        for s in range(593):
            x, y, bw, bh = (int(v) for v in table[s])
            hx, hy, qx, qy, cost = oracle_lib.frac_refine(cur, (M + x, M + y), ref, (M + x, M + y), bw, bh, (0, 0), pred, lq, 1, bd)
            oq[s], oc[s] = (2 * hx + qx, 2 * hy + qy), cost
        same(q[None], c[None], oq[None], oc[None], kind, bd, lq, pred)
        if lq == LQ_TOP and kind != "flat0":
            # complement: every slot of at most 64 samples reports its bound.  origin: the difference doubles and so do the advantages of the
            # other points; 4 bits (16 384) still outweigh those of two 4x4 blocks (2 * 2 * 3 832), so the 8x4 and 4x8 slots report theirs
            span = maxv if kind == "complement" else 2 * maxv
            at_bound = [s for s in sc.small_slots() if kind == "complement" or table[s][2] * table[s][3] == 32]
            assert len(at_bound) == (384 if kind == "complement" else 256) and (q[at_bound] == 0).all()
            assert all(int(c[s]) == sc.slot_bound(s, bd, span) + 8192 for s in at_bound)


# ---- 3: caller-chosen integer MVs off the pattern's grid ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_integer_mv_off_the_grid(engine, oracle_lib, bd):
    """the complement displaced by (+3, -2) samples and the integer MV (3, -2) in every slot: the patch fetch starts 3 bytes (6 at 10 bit) into
    a dword and the pattern's blocks straddle the 4x4 grid of the fetch.  Blocks whose 8-tap support stays inside the picture see the
    periodic pattern: there the bound holds as in the aligned case"""
    maxv = (1 << bd) - 1
    cur = sc.bent_plane(64, 64, bd)
    ref = np.where(sc.bent_sign(64, 64, 3, -2) > 0, 0, maxv)
    planes = (sc.pad(cur), sc.pad(ref))
    for lq, pred in ((LQ_TOP, (12, -8)), (0, (12, -8)), (3794534, (12, -10))):
        q, c = plain(engine, oracle_lib, "shifted", 64, 64, bd, 1, lq, pred, imv=(3, -2), planes=planes)
        if lq == LQ_TOP:
            inner = [s for s, (x, y, w, h) in enumerate(sc.slot_rects()) if w * h <= 64 and min(x, y) >= 8 and max(x + w, y + h) <= 56]
            assert len(inner) > 100 and (q[0, inner] == (12, -8)).all()
            assert all(int(c[0, s]) == sc.slot_bound(s, bd, maxv) + 8192 for s in inner)


# ---- 4: weighted refinement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("had", [1, 0])
@pytest.mark.parametrize("bd", [8, 9, 10, 11, 12])
def test_weighted_refinement(engine, oracle_lib, bd, had):
    """the inverting weight on the picture itself (difference exactly +-maxv: the bound, through the weighted kernel) and every refinement
    boundary weight of range_content on the pattern instead of its random binary pictures"""
    from hmme import api, synth
    m, maxv = synth.MARGIN, (1 << bd) - 1
    inverting = (-64, maxv, 6, 32)
    weights = [("inverting, the picture its own reference", inverting)] + [(f, rc.boundary_weight(bd, 1, f)) for f in rc.FAMILIES]
    imv = np.zeros((1, 593, 2), np.int16)
    small = sc.small_slots()
    for k, (name, wp) in enumerate(weights):
        assert api.weight_check(bd, wp, True) == 0
        lq, pred = (LQ_TOP, (0, 0)) if k == 0 else ((0, 3794534)[k & 1], PREDS[(k >> 1) & 1])
        cur, ref = sc.weighted_pair(64, 64, bd, wp)
        engine.set_lambda_q16(lq)
        pc, pr = mkplane(engine, cur, 64, 64, bd), mkplane(engine, ref, 64, 64, bd)
        try:
            q, c = engine.refine_frame_w(pc, pr, SR, wp, imv, preds_of(pred, 1), use_hadamard=bool(had))
        finally:
            pc.close(); pr.close()
        org = np.ascontiguousarray(cur[m:m + 64, m:m + 64])
        oq, oc = oracle_origin_refine_w(oracle_lib, org, ref, 64, 64, imv, preds_of(pred, 1), lq, had, bd, wp, [0])
        same(q, c, oq, oc, name, wp, bd, had, lq, pred)
        if k == 0:
            assert np.array_equal(cur, ref) and (q[0, small] == 0).all()
            assert all(int(c[0, s]) == (sc.slot_bound(s, bd, maxv) >> (0 if had else 1)) + 8192 for s in small)


def test_weighted_refinement_of_six_ctus(engine, oracle_lib):
    from hmme import synth
    m, bd = synth.MARGIN, 8
    wp = (-64, 255, 6, 32)
    cur, ref = sc.weighted_pair(EW, EH, bd, wp)
    imv = np.zeros((E_CTU, 593, 2), np.int16)
    pq = preds_of((0, -2), E_CTU)
    engine.set_lambda_q16(3794534)
    pc, pr = mkplane(engine, cur, EW, EH, bd), mkplane(engine, ref, EW, EH, bd)
    try:
        q, c = engine.refine_frame_w(pc, pr, SR, wp, imv, pq, use_hadamard=True)
    finally:
        pc.close(); pr.close()
    org = np.ascontiguousarray(cur[m:m + 128, m:m + 192])
    oq, oc = oracle_origin_refine_w(oracle_lib, org, ref, EW, EH, imv, pq, 3794534, 1, bd, wp, range(E_CTU))
    same(q, c, oq, oc, "weighted", (EW, EH))


# ---- 5: bi-prediction refinement: an origin in {2 * maxv, -maxv}, a difference of +-2 * maxv ---------------------------------------------------
# one CTU at every served depth, Hadamard and SAD; the six-CTU form once per kernel, <1, 2, 1> and <0, 2, 1>
BI_CASES = [(bd, had, 64, 64) for bd in (8, 10, 11) for had in (1, 0)] + [(8, 1, EW, EH), (11, 0, EW, EH)]


@pytest.mark.parametrize("bd,had,w,h", BI_CASES)
def test_bi_refinement(engine, oracle_lib, hmo, bd, had, w, h):
    from hmme import api, synth
    m, maxv, n = synth.MARGIN, (1 << bd) - 1, n_ctus(w, h)
    assert api.bipred_check(bd, True) == 0
    cur, ref, other = sc.bi_triple(w, h, bd)
    field = np.zeros((n, 1, 2), np.int16)
    org = origin_picture(cur, oracle_prediction(hmo, other, w, h, bd, field), w, h)
    assert org[:64, :64].max() == 2 * maxv and org[:64, :64].min() == -maxv
    org_padded = np.ascontiguousarray(np.pad(org, m))
    imv = np.zeros((n, 593, 2), np.int16)
    small32 = [s for s in sc.small_slots() if sc.slot_rects()[s][2] * sc.slot_rects()[s][3] == 32]
    for lq, pred in ((0, (0, 0)), (3794534, (0, -2)), (LQ_TOP, (0, 0))):
        pq = preds_of(pred, n)
        engine.set_lambda_q16(lq)
        pc, pr, po = (mkplane(engine, a, w, h, bd) for a in (cur, ref, other))
        try:
            q, c = engine.refine_frame_bi(pc, pr, po, SR, field, imv, pred_q=pq, use_hadamard=bool(had))
        finally:
            pc.close(); pr.close(); po.close()
        oq, oc = oracle_lib.refine_frame(org_padded, ref, (m, m), w, h, imv, pq, lq, had, bd, n_threads=8)
        same(q, c, oq, oc, "bi", (w, h), bd, had, lq, pred)
        # the largest cost: the 64x64 bound less what the oracle's winner gains on the integer point (the device cost IS the oracle's, and
        # tests/test_spectral_cpu.py asserts the oracle's integer-position value to be the bound)
        bound = sc.slot_bound(592, bd, 2 * maxv) >> (0 if had else 1)
        gain = bound - (int(oc[0, 592]) - sc.mv_cost(lq, int(oq[0, 592, 0]), int(oq[0, 592, 1]), pred))
        assert gain >= 0 and int(c.max()) >= bound - gain
        if lq == LQ_TOP and had:   # 16 384 for 4 bits outweigh the doubled advantages of two 4x4 blocks: the 8x4 and 4x8 slots report their bound
            assert len(small32) == 256 and (q[0, small32] == 0).all()
            assert all(int(c[0, s]) == sc.slot_bound(s, bd, 2 * maxv) + 8192 for s in small32)


# ---- 6: the residual's per-PU Hadamard error ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 12])
def test_residual_hadamard_error_is_the_bound(engine, oracle_lib, bd):
    """cur = the pattern, pred = its complement: one 64x64 PU, then every 8x8 and every 4x4 block its own PU -- each error EXACTLY the bound"""
    maxv = (1 << bd) - 1
    cur = sc.bent_plane(64, 64, bd)
    pred = sc.complement(cur, bd).astype(np.uint8 if bd == 8 else np.uint16)
    L = oracle_lib.oracle()
    pc = mkplane(engine, sc.pad(cur), 64, 64, bd)
    try:
        for slot, per, want in ((np.full((1, 64), 592, np.uint16), 64, sc.slot_bound(592, bd, maxv)), (None, 64, (128 * maxv) >> (bd - 8)),
                                (None, 256, (32 * maxv) >> (bd - 8))):
            resid, pu, cu, ctu = engine.residual_frame(pc, pred, slot=slot, mv_per_ctu=per, use_hadamard=True)
            md, mpu, mcu, mctu = rm.residual_picture(L, cur, pred, 64, 64, bd, slot, per, 1)
            assert np.array_equal(resid, md) and np.array_equal(resid, maxv * sc.bent_sign(64, 64))
            assert np.array_equal(pu, mpu) and np.array_equal(cu, mcu) and np.array_equal(ctu, mctu), (bd, per)
            assert (pu == want).all(), (bd, per, int(pu.max()), want)
            assert int(ctu[0, 0]) == (want if slot is not None else per * want)
    finally:
        pc.close()
