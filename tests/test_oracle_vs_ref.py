"""Cross-check of the oracle against the reference's own compiled code (oracle/_ref/libhmref.so).
Where that library was built the reference answers live, and its answers must also equal the ones
recorded from it in tests/golden/oracle_vs_ref.npz; elsewhere the recorded answers stand in for it,
so the check runs on every machine."""
import ctypes as C
import os

import numpy as np
import pytest

import lambda_cases as lc
import oracle_py

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_ref.npz")


class ReferenceAnswers:
    """The reference's answers to one test's questions, asked in a fixed order.  `ask(question)` calls question() on the live library
    when it is there and returns the answer as a flat int64 array, or returns the recorded answer of the same place in the order.
    HMME_RECORD_REF_ANSWERS=1 with the live library rewrites this test's recording (tests/golden/gen_golden.py oracle_vs_ref)."""

    def __init__(self, name):
        self.name, self.i, self.out = name, 0, []
        self.live = oracle_py.ref_available()
        self.record = self.live and os.environ.get("HMME_RECORD_REF_ANSWERS") == "1"
        if not self.record:
            with np.load(GOLDEN) as g:
                self.flat, lens = g[name], g[name + ".lens"]
            self.offs = np.concatenate([[0], np.cumsum(lens)])

    def ask(self, question):
        i = self.i
        self.i += 1
        if not self.live:
            return self.flat[self.offs[i]:self.offs[i + 1]]
        got = np.ravel(np.asarray(question())).astype(np.int64)
        if self.record:
            self.out.append(got)
        else:
            assert np.array_equal(got, self.flat[self.offs[i]:self.offs[i + 1]]), f"{self.name}: live answer {i} differs from the recorded one"
        return got

    def done(self):
        """every recorded answer was asked for; in recording mode, store this test's answers"""
        if not self.record:
            assert self.i == len(self.offs) - 1, f"{self.name}: {self.i} answers asked, {len(self.offs) - 1} recorded"
            return
        d = dict(np.load(GOLDEN)) if os.path.exists(GOLDEN) else {}
        d[self.name] = np.concatenate(self.out)
        d[self.name + ".lens"] = np.array([len(v) for v in self.out], np.int64)
        np.savez_compressed(GOLDEN, **d)


@pytest.fixture
def reference(request):
    return ReferenceAnswers(request.node.name)


def test_random_pu_searches_match_reference(oracle_lib, reference):
    R = oracle_lib.ref() if reference.live else None
    rng = np.random.default_rng(2024)
    table = oracle_lib.slot_table()
    for it in range(40):
        bd = int(rng.choice([8, 10]))
        sr = int(rng.choice([3, 8, 12]))
        side = 64 + 2 * sr + 8
        cur = rng.integers(0, 1 << bd, size=(64, 64)).astype(np.int16)
        ref = rng.integers(0, 1 << bd, size=(side, side)).astype(np.int16)
        o = sr + 4
        lam = float(rng.choice([0.0, 3.3, 57.9, 900.0, 5.0e6]))
        pred = (int(rng.integers(-60, 61)), int(rng.integers(-60, 61)))
        lt = (-int(rng.integers(0, sr + 1)), -int(rng.integers(0, sr + 1)))
        rb = (int(rng.integers(0, sr + 1)), int(rng.integers(0, sr + 1)))
        fen = int(rng.integers(0, 2))
        lq = int(reference.ask(lambda: R.ref_lambda_q16(lam))[0])
        p = oracle_lib.make_params(lt, rb, pred, lq, fen, bd)
        ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), p)
        for s in rng.choice(593, size=25, replace=False):
            x, y, w, h = (int(v) for v in table[s])
            want = tuple(int(v) for v in reference.ask(lambda: oracle_lib.pattern_search(cur, (x, y), ref, (o + x, o + y), w, h, p, use_ref=True, lam=lam)))
            assert (int(ox[s]), int(oy[s]), int(osad[s])) == want, (it, s)
            assert tuple(oracle_lib.pattern_search(cur, (x, y), ref, (o + x, o + y), w, h, p)) == want
    reference.done()


def test_random_weighted_pu_searches_match_reference(oracle_lib, reference):
    """live: the reference's xPatternSearch with bApplyWeight (explicit weighted prediction) against the oracle's all-slot and
    per-PU weighted searches, random weights incl. negative ones and shift 0"""
    R = oracle_lib.ref() if reference.live else None
    if reference.live and not hasattr(R, "ref_pattern_search_w"):
        pytest.skip("libhmref.so predates the weighted-prediction harness")
    rng = np.random.default_rng(404)
    table = oracle_lib.slot_table()
    for it in range(24):
        bd = int(rng.choice([8, 10]))
        sr = int(rng.choice([3, 8]))
        side = 64 + 2 * sr + 8
        cur = rng.integers(0, 1 << bd, size=(64, 64)).astype(np.int16)
        ref = rng.integers(0, 1 << bd, size=(side, side)).astype(np.int16)
        o = sr + 4
        lam = float(rng.choice([0.0, 57.9, 900.0]))
        pred = (int(rng.integers(-40, 41)), int(rng.integers(-40, 41)))
        shift = int(rng.integers(0, 8))
        wp = (int(rng.integers(-40, 128)), int(rng.integers(-128, 128)) << (bd - 8), shift, (1 << (shift - 1)) if shift else 0)
        fen = int(rng.integers(0, 2))
        p = oracle_lib.make_params((-sr, -sr), (sr, sr), pred, int(reference.ask(lambda: R.ref_lambda_q16(lam))[0]), fen, bd)
        ox, oy, osad = oracle_lib.search_ctu_w(cur, (0, 0), ref, (o, o), p, wp)
        for s in rng.choice(593, size=16, replace=False):
            x, y, w, h = (int(v) for v in table[s])
            want = tuple(int(v) for v in reference.ask(lambda: oracle_lib.pattern_search_w(cur, (x, y), ref, (o + x, o + y), w, h, p, wp, use_ref=True, lam=lam)))
            assert (int(ox[s]), int(oy[s]), int(osad[s])) == want, (it, s, wp)
            assert tuple(oracle_lib.pattern_search_w(cur, (x, y), ref, (o + x, o + y), w, h, p, wp)) == want
    reference.done()


def test_cost_and_bits_match_reference(oracle_lib, reference):
    L, R = oracle_lib.oracle(), (oracle_lib.ref() if reference.live else None)
    rng = np.random.default_rng(5)
    for v in rng.integers(-40000, 40001, size=500):
        assert L.hmo_component_bits(int(v)) == reference.ask(lambda: R.ref_component_bits(int(v)))[0]
    for lam in (0.1, 33.0, 2.0e5, 9.9e6):
        lq = int(reference.ask(lambda: R.ref_lambda_q16(lam))[0])
        assert lq == L.hmo_lambda_q16(lam)
        for _ in range(100):
            x, y, px, py = (int(v) for v in rng.integers(-300, 301, size=4))
            assert L.hmo_mv_cost(lq, x, y, px, py, 2) == reference.ask(lambda: R.ref_mv_cost(lam, x, y, px, py))[0]
    reference.done()


def test_fractional_refinement_matches_reference(oracle_lib, reference):
    from hmme import synth
    rng = np.random.default_rng(99)
    table = oracle_lib.slot_table()
    for it in range(40):
        bd = 8 if it % 3 else 10
        cur, ref, _ = synth.make_pair(160, 160, seed=200 + it, bit_depth=bd, max_mv=3, region=64, margin=16, noise_sigma=3.0)
        x, y, w, h = (int(v) for v in table[int(rng.integers(0, 593))])
        mv = (int(rng.integers(-5, 6)), int(rng.integers(-5, 6)))
        pred = (int(rng.integers(-50, 51)), int(rng.integers(-50, 51)))
        lam = float(rng.choice([0.0, 12.0, 57.9, 3000.0]))
        had = int(rng.integers(0, 2))
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        o = 16 + 48
        a = oracle_lib.frac_refine(cur, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lq, had, bd)
        b = tuple(int(v) for v in reference.ask(lambda: oracle_lib.frac_refine(cur, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lam, had, bd,
                                                                             use_ref=True)))
        assert tuple(a) == b, (it, w, h, mv, pred, lam, had, bd)
        # the bBi call: origin 2*org - pred_other (unclipped, TComYuv.cpp:409-440), biPred = true
        other = np.roll(cur, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(0, 1)).astype(np.int32) + rng.integers(-30, 31, size=cur.shape)
        org = (2 * cur.astype(np.int32) - np.clip(other, 0, (1 << bd) - 1)).astype(np.int16)
        a = oracle_lib.frac_refine(org, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lq, had, bd)
        b = tuple(int(v) for v in reference.ask(lambda: oracle_lib.frac_refine(org, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lam, had, bd,
                                                                             use_ref=True, bi=True)))
        assert tuple(a) == b, ("bi", it, w, h, mv, pred, lam, had, bd)
    reference.done()


def test_tz_search_over_whole_ctus_matches_reference(oracle_lib, reference):
    """bench.py's CPU baseline legs: the reference's own xTZSearch over all 593 PU shapes of a CTU range (ref_tz_frame: 64x64 PU first,
    the others seeded with its integer MV, TEncSearch.cpp:3780-3789) == the oracle's threaded restatement (hmo_tz_frame), 8 and 10 bit"""
    from hmme import synth
    for bd, sr in ((8, 64), (10, 24)):
        w, h = 448, 320
        cur, ref, _ = synth.make_pair(w, h, seed=60 + bd, bit_depth=bd)
        m = synth.MARGIN
        lq = oracle_lib.oracle().hmo_lambda_q16(57.9)
        want = reference.ask(lambda: oracle_lib.ref_tz_frame(cur, ref, (m, m), w, h, sr, 57.9, 1, bd, 8, 9))   # (x, y, cost) tables, flat
        _, _, ox, oy, os_ = oracle_lib.tz_frame(cur, ref, (m, m), w, h, sr, None, lq, 1, bd, 8, 9, 4, True, True)
        assert ox.shape == (9, 593) and np.array_equal(want, np.concatenate([np.ravel(a) for a in (ox, oy, os_)]))
    reference.done()


def test_full_search_over_whole_ctus_matches_reference(oracle_lib, reference):
    """bench.py's `cpu_baseline.reference_full_search` leg: the reference's own xPatternSearch for each of the 593 PUs of a CTU range (one
    window per CTU, predictor (0,0)) == the oracle's whole-frame restatement, incl. a picture-edge CTU whose window clipMv cuts, 8 and 10 bit"""
    from hmme import synth
    for bd, sr, first in ((8, 12, 0), (10, 7, 8)):
        w, h = 448, 320
        cur, ref, _ = synth.make_pair(w, h, seed=70 + bd, bit_depth=bd)
        m = synth.MARGIN
        lq = oracle_lib.oracle().hmo_lambda_q16(57.9)

        def live():
            rx, ry, rs, dt = oracle_lib.ref_full_search_ctus(cur, ref, (m, m), w, h, sr, 57.9, 1, bd, first, min_ctus=2, max_ctus=2, budget_s=0.0)
            assert rx.shape == (2, 593) and dt > 0
            return rx, ry, rs

        want = reference.ask(live)   # (x, y, cost) tables, flat
        ox, oy, os_ = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, None, lq, 1, bd, first, 2, 2)
        assert ox.shape == (2, 593) and np.array_equal(want, np.concatenate([np.ravel(a) for a in (ox, oy, os_)]))
    reference.done()


# ---- where the MV cost wraps or peaks (tests/lambda_cases.py): getCost's product wraps in 32 bits in the reference, and so must the oracle's ----
def _edge_predictor(rng):
    """quarter pels: each component near (+-60) or far (out to +-2000, where one component alone takes 21 or 23 bits)"""
    return tuple(int(rng.integers(-s, s + 1)) for s in rng.choice([60, 2000], size=2))


def _edge_lambda(reference, R, lq):
    """the double the reference is asked with; its own conversion must give lambda_q16 back"""
    lam = lc.as_double(lq)
    assert int(reference.ask(lambda: R.ref_lambda_q16(lam))[0]) == lq
    return lam


def _moved_block(rng, bd, sr, noise=2):
    """a 64x64 block that lies in `ref` displaced by a motion inside the window, under a little noise: the large PUs find it whatever its
    bits cost, the small ones follow the MV cost"""
    side = 64 + 2 * sr + 8
    o = sr + 4
    ref = rng.integers(0, 1 << bd, size=(side, side)).astype(np.int16)
    tx, ty = (int(v) for v in rng.integers(-sr + 1, sr, size=2))
    cur = np.clip(ref[o + ty:o + ty + 64, o + tx:o + tx + 64].astype(np.int32) + rng.integers(-noise, noise + 1, size=(64, 64)), 0, (1 << bd) - 1)
    return np.ascontiguousarray(cur.astype(np.int16)), ref, o


def _check_winner_conditions(bits):
    """bits: lambda_q16 -> MV bit counts of the winners.  178956971: wrapped and unwrapped winners both occur.  0x80000000: an MV's bit count
    is the sum of two odd exp-Golomb lengths, hence even, so getCost of it is 0 for every candidate -- winners of odd parity cannot occur in
    a search or a refinement (they do in the direction decision, which adds the caller's bits: tests/test_select_dirs_cpu.py)"""
    assert any(lc.wraps(lc.WRAP24, b) for b in bits[lc.WRAP24]) and any(not lc.wraps(lc.WRAP24, b) for b in bits[lc.WRAP24])
    assert bits[lc.HALF] and all(b % 2 == 0 and lc.get_cost(lc.HALF, b) == 0 for b in bits[lc.HALF])
    assert all(lc.get_cost(lc.ALL_ONES, b) == lc.MAX_MV_COST for b in bits[lc.ALL_ONES])
    assert max(max(v) for v in bits.values()) >= 30


def test_pu_searches_at_wrapping_lambdas_match_reference(oracle_lib, reference):
    """per-PU integer search, 8 and 10 bit, FEN 0 and 1, at the six lambda_q16 of tests/lambda_cases.py, predictors out to +-2000 quarter pels"""
    R = oracle_lib.ref() if reference.live else None
    rng = np.random.default_rng(3101)
    table = oracle_lib.slot_table()
    bits = {lq: [] for lq in lc.LAMBDA_Q16}
    for lq in lc.LAMBDA_Q16:
        lam = _edge_lambda(reference, R, lq)
        for bd in (8, 10):
            for fen in (0, 1):
                sr = 8
                cur, ref, o = _moved_block(rng, bd, sr)
                pred = _edge_predictor(rng) if fen else tuple(int(v) for v in rng.integers(-30, 31, size=2))
                p = oracle_lib.make_params((-sr, -sr), (sr, sr), pred, lq, fen, bd)
                ox, oy, osad = oracle_lib.search_ctu(cur, (0, 0), ref, (o, o), p)
                for s in [592, 0] + [int(v) for v in rng.choice(np.arange(1, 592), size=8, replace=False)]:
                    x, y, w, h = (int(v) for v in table[s])
                    want = tuple(int(v) for v in reference.ask(lambda: oracle_lib.pattern_search(cur, (x, y), ref, (o + x, o + y), w, h, p, use_ref=True, lam=lam)))
                    assert (int(ox[s]), int(oy[s]), int(osad[s])) == want, (lq, bd, fen, s, pred)
                    assert tuple(oracle_lib.pattern_search(cur, (x, y), ref, (o + x, o + y), w, h, p)) == want
                    bits[lq].append(lc.mv_bits(4 * want[0], 4 * want[1], *pred))
    _check_winner_conditions(bits)
    reference.done()


def test_weighted_pu_searches_at_wrapping_lambdas_match_reference(oracle_lib, reference):
    R = oracle_lib.ref() if reference.live else None
    rng = np.random.default_rng(3102)
    table = oracle_lib.slot_table()
    bits = {lq: [] for lq in lc.LAMBDA_Q16}
    for lq in lc.LAMBDA_Q16:
        lam = _edge_lambda(reference, R, lq)
        for bd in (8, 10):
            sr = 8
            cur, ref, o = _moved_block(rng, bd, sr)
            shift = int(rng.integers(4, 8))
            wp = ((1 << shift) + int(rng.integers(-3, 4)), int(rng.integers(-6, 7)) << (bd - 8), shift, 1 << (shift - 1))   # near the identity: the motion stays findable
            pred = _edge_predictor(rng) if bd == 10 else tuple(int(v) for v in rng.integers(-30, 31, size=2))
            p = oracle_lib.make_params((-sr, -sr), (sr, sr), pred, lq, int(rng.integers(0, 2)), bd)
            ox, oy, osad = oracle_lib.search_ctu_w(cur, (0, 0), ref, (o, o), p, wp)
            for s in [592, 0] + [int(v) for v in rng.choice(np.arange(1, 592), size=6, replace=False)]:
                x, y, w, h = (int(v) for v in table[s])
                want = tuple(int(v) for v in reference.ask(lambda: oracle_lib.pattern_search_w(cur, (x, y), ref, (o + x, o + y), w, h, p, wp, use_ref=True, lam=lam)))
                assert (int(ox[s]), int(oy[s]), int(osad[s])) == want, (lq, bd, s, wp, pred)
                assert tuple(oracle_lib.pattern_search_w(cur, (x, y), ref, (o + x, o + y), w, h, p, wp)) == want
                bits[lq].append(lc.mv_bits(4 * want[0], 4 * want[1], *pred))
    _check_winner_conditions(bits)
    reference.done()


def test_fractional_refinement_at_wrapping_lambdas_matches_reference(oracle_lib, reference):
    """SAD and Hadamard, plain and the bi origin, 8 and 10 bit.  Every second case puts the predictor 16 and 3 pels from the integer MV
    (4 * mv - pred = (+-64, +-12): 13 or 15 bits in x, 9 in y), so that the nine half-pel points lie on both sides of 24 bits, the first
    wrap of lambda_q16 = 178956971; the others draw it out to +-2000 quarter pels"""
    from hmme import synth
    R = oracle_lib.ref() if reference.live else None
    rng = np.random.default_rng(3103)
    table = oracle_lib.slot_table()
    straddles, top = {lq: 0 for lq in lc.LAMBDA_Q16}, 0
    it = 0
    for lq in lc.LAMBDA_Q16:
        lam = _edge_lambda(reference, R, lq)
        for bd in (8, 10):
            for had in (0, 1):
                for near in (True, False):
                    it += 1
                    cur, ref, _ = synth.make_pair(160, 160, seed=700 + it, bit_depth=bd, max_mv=3, region=64, margin=16, noise_sigma=3.0)
                    x, y, w, h = (int(v) for v in table[int(rng.integers(0, 593))])
                    mv = (int(rng.integers(-5, 6)), int(rng.integers(-5, 6)))
                    sx, sy = (int(v) for v in rng.choice([-1, 1], size=2))
                    pred = (4 * mv[0] - 64 * sx, 4 * mv[1] - 12 * sy) if near else _edge_predictor(rng)
                    nine = [lc.mv_bits(4 * mv[0] + dx, 4 * mv[1] + dy, *pred) for dy in (-2, 0, 2) for dx in (-2, 0, 2)]
                    straddles[lq] += min(nine) < 24 <= max(nine)
                    top = max(top, max(nine))
                    o = 16 + 48
                    a = oracle_lib.frac_refine(cur, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lq, had, bd)
                    b = tuple(int(v) for v in reference.ask(lambda: oracle_lib.frac_refine(cur, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lam, had, bd,
                                                                                         use_ref=True)))
                    assert tuple(a) == b, (lq, w, h, mv, pred, had, bd)
                    other = np.roll(cur, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(0, 1)).astype(np.int32) + rng.integers(-30, 31, size=cur.shape)
                    org = (2 * cur.astype(np.int32) - np.clip(other, 0, (1 << bd) - 1)).astype(np.int16)
                    a = oracle_lib.frac_refine(org, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lq, had, bd)
                    b = tuple(int(v) for v in reference.ask(lambda: oracle_lib.frac_refine(org, (o + x, o + y), ref, (o + x, o + y), w, h, mv, pred, lam, had, bd,
                                                                                         use_ref=True, bi=True)))
                    assert tuple(a) == b, ("bi", lq, w, h, mv, pred, had, bd)
    assert all(n >= 4 for n in straddles.values()) and top >= 30, (straddles, top)
    assert not lc.wraps(lc.WRAP24, 22) and lc.wraps(lc.WRAP24, 24)
    reference.done()


# ---- partial ties (tests/tie_content.py): where candidates cost the same the reference's answer is its loop order's alone, and so must the oracle's be ----
def test_pu_searches_on_partial_ties_match_reference(oracle_lib, reference):
    """per-PU integer search on the four skewed lattices (every slot has SAD 0 on a lattice of candidates; the MV cost leaves several of them
    tied), search range 8, lambda_q16 0, 1 << 13, 1 << 16 and that of 57.9, 8 and 10 bit, FEN 0 and 1; and on two pictures that hold the
    CTU's block twice, at search ranges 64 and 128"""
    import tie_content as tc
    from hmme import synth
    from refine_tables import oracle_windows
    R = oracle_lib.ref() if reference.live else None
    rng = np.random.default_rng(3201)
    table = oracle_lib.slot_table()
    m, w, sr = synth.MARGIN, 192, 8
    o = m + 64                                        # CTU 4 of the 192 x 192 picture
    tied = 0
    for lattice in tc.LATTICES:
        for lq in tc.SEARCH_LAMBDA_Q16:
            lam = _edge_lambda(reference, R, lq)
            for bd in (8, 10):
                cur, ref = tc.skewed_lattice(w, w, *lattice, bd, seed=11)
                for fen in (0, 1):
                    pred = rng.integers(-32, 33, size=(9, 2)).astype(np.int16)
                    win = oracle_windows(w, w, sr, pred)[4]
                    pq = (int(pred[4, 0]), int(pred[4, 1]))
                    p = oracle_lib.make_params((int(win[0]), int(win[1])), (int(win[2]), int(win[3])), pq, lq, fen, bd)
                    ox, oy, osad = oracle_lib.search_ctu(cur, (o, o), ref, (o, o), p)
                    ts = tc.tie_set(win, pq, lq, lattice, tc.LATTICE_SHIFT, (w, w, 64, 64))
                    tied += len(ts["members"]) >= 2
                    for s in [592, 0] + [int(v) for v in rng.choice(np.arange(1, 592), size=23, replace=False)]:
                        x, y, bw, bh = (int(v) for v in table[s])
                        want = tuple(int(v) for v in reference.ask(lambda: oracle_lib.pattern_search(cur, (o + x, o + y), ref, (o + x, o + y), bw, bh, p, use_ref=True, lam=lam)))
                        assert (int(ox[s]), int(oy[s]), int(osad[s])) == want, (lattice, lq, bd, fen, s, pq)
                        assert tuple(oracle_lib.pattern_search(cur, (o + x, o + y), ref, (o + x, o + y), bw, bh, p)) == want
                    assert (int(ox[592]), int(oy[592]), int(osad[592])) == ts["raster_first"] + (0,), (lattice, lq, bd, fen, ts)
    assert tied >= 32, tied                           # in at least half of the 64 cases the 64x64 slot had several candidates tied for the win
    for (name, sr, a, b), bd, lq in ((tc.TWO_MATCH_8[0], 8, tc.Q16_57_9), (tc.TWO_MATCH_8[2], 10, 0)):
        lam = _edge_lambda(reference, R, lq)
        size = tc.two_match_size(sr)
        _, cu_x, cu_y = tc.centre_ctu(size)
        cur, ref = tc.two_match(bd, 31, a, b, size)
        pq = tc.tie_predictor(a, b) if lq else (0, 0)
        p = oracle_lib.make_params((-sr, -sr), (sr, sr), pq, lq, 1, bd)
        ox, oy, osad = oracle_lib.search_ctu(cur, (m + cu_x, m + cu_y), ref, (m + cu_x, m + cu_y), p)
        for s in [592, 0] + [int(v) for v in rng.choice(np.arange(1, 592), size=10, replace=False)]:
            x, y, bw, bh = (int(v) for v in table[s])
            want = tuple(int(v) for v in reference.ask(lambda: oracle_lib.pattern_search(cur, (m + cu_x + x, m + cu_y + y), ref, (m + cu_x + x, m + cu_y + y), bw, bh,
                                                                                       p, use_ref=True, lam=lam)))
            assert want == a + (0,) and (int(ox[s]), int(oy[s]), int(osad[s])) == want, (name, s, want)
    reference.done()


def test_fractional_refinement_on_partial_ties_matches_reference(oracle_lib, reference):
    """plain and weighted xPatternSearchFracDIF on flat content (the MV cost alone decides), on content constant along x and on content constant
    along y (the distortion ties along one axis), over the grid of predictor offsets -9..9 quarter pels in both components, lambda 0, 1.0 and
    57.9, Hadamard and SAD, 8 and 10 bit.  Block sizes 8x4, 16x16, 12x16 and 64x64: each combination runs the whole grid at one of them, in
    turn, and a seeded dozen of offsets at the three others"""
    import tie_content as tc
    from hmme import synth
    if reference.live and not hasattr(oracle_lib.ref(), "ref_frac_refine_w"):
        pytest.skip("libhmref.so predates the weighted-prediction harness")
    rng = np.random.default_rng(3202)
    sizes = ((8, 4), (16, 16), (12, 16), (64, 64))
    grid = [(dx, dy) for dy in range(-9, 10) for dx in range(-9, 10)]
    o = synth.MARGIN + 64
    combo = 0
    moved = {k: 0 for k in tc.REFINE_KINDS}
    for kind in tc.REFINE_KINDS:
        for bd in (8, 10):
            cur, ref = tc.refine_content(kind, 192, 192, bd, seed=3)
            for had in (0, 1):
                for lam in tc.REFINE_LAMBDAS:
                    lq = oracle_lib.oracle().hmo_lambda_q16(lam)
                    assert lq == tc.lambda_q16_of(lam)
                    for weighted in (False, True):
                        whole = sizes[combo % 4]
                        combo += 1
                        for bw, bh in sizes:
                            offs = grid if (bw, bh) == whole else [grid[i] for i in rng.choice(len(grid), size=12, replace=False)]
                            for dx, dy in offs:
                                mv = (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
                                pred = (4 * mv[0] - dx, 4 * mv[1] - dy)
                                if weighted:
                                    a = oracle_lib.frac_refine_w(cur, (o, o), ref, (o, o), bw, bh, mv, pred, lq, had, bd, tc.WP)
                                    b = reference.ask(lambda: oracle_lib.frac_refine_w(cur, (o, o), ref, (o, o), bw, bh, mv, pred, lam, had, bd, tc.WP, use_ref=True))
                                else:
                                    a = oracle_lib.frac_refine(cur, (o, o), ref, (o, o), bw, bh, mv, pred, lq, had, bd)
                                    b = reference.ask(lambda: oracle_lib.frac_refine(cur, (o, o), ref, (o, o), bw, bh, mv, pred, lam, had, bd, use_ref=True))
                                assert tuple(a) == tuple(int(v) for v in b), (kind, bd, had, lam, weighted, (bw, bh), mv, pred)
                                moved[kind] += a[:4] != (0, 0, 0, 0)
                                if kind == "flat" and not weighted:
                                    assert (4 * mv[0] + 2 * a[0] + a[2], 4 * mv[1] + 2 * a[1] + a[3]) == tc.flat_refine_model(mv, pred, lq)[:2]
    assert all(n > 1000 for n in moved.values()), moved
    reference.done()
