"""CPU check of the marker-free packed-minimum twin of the 8-bit reduction tree (tools/gen_me_tree.py, Tree(1, pk=2): beside the five
slots of every 8x8 CU, twelve of the thirteen slots of every 16x16 CU take their minimum on packed u16 costs, in tasks whose lanes are
all wholly valid or wholly invalid).  The generator's numpy interpreter runs the op lists of me_tree_pk2_fen1.inc and
me_tree_pk_fen1.inc inside a Python model of the kernel's task loop -- each task with the body the kernel's predicate gives it --
flush and j recovery, and must give what the same model gives with the 32-bit tree (which tests/test_tree_sim.py pins to the reference
goldens) for all 593 slots.  The operation counts are held against the stop rule (250 VALU instructions below the packed-minimum
tree), the gate at both sides of each threshold, the task predicate against a brute-force lane map."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_me_tree as G  # noqa: E402
import test_tree_pkmin as P  # noqa: E402
import test_tree_sim as T  # noqa: E402

INV, IDX = T.INV, T.IDX
MAX_BITS = P.MAX_BITS
GATE2_LQ = 14680063     # the largest lambda_q16 with (lambda_q16 * 74 >> 16) + 48 960 <= 65 535
mv_cost = P.mv_cost


def slot_rect2(s):
    """the rectangles of me_pk_slot (me_kernels.hpp) with WIDE: (x, y, w, h, row step), or None for a slot that keeps 32-bit keys"""
    r = P.slot_rect(s)
    if r:
        return r + (1,)
    if 256 <= s < 384:
        kk, x, y, w, h = (s - 256) >> 4, (s & 3) * 16, ((s >> 2) & 3) * 16, 16, 16
        if kk < 4:
            h = 4 if kk < 2 else 12
            y += (16 - h) if kk & 1 else 0
        else:
            w = 4 if kk < 6 else 12
            x += (16 - w) if kk & 1 else 0
        return x, y, w, h, 2 if h > 8 else 1
    if 448 <= s < 480:
        return (s & 3) * 16, ((s - 448) >> 3) * 16 + ((s >> 2) & 1) * 8, 16, 8, 1
    if 480 <= s < 512:
        return ((s >> 1) & 3) * 16 + (s & 1) * 8, ((s - 480) >> 3) * 16, 8, 16, 2
    return None


def parts(wx, wy):
    """-> [(k, x0, iterations)] of a window, as the kernel cuts it"""
    quads = (wx + 3) >> 2
    fold = bool(quads & 32) and bool(quads & 31) and bool(wy & 1)
    out, x0 = [], 0
    for k in range(5, -1, -1):
        if quads & (1 << k):
            ty = 64 >> k
            out.append((k, x0, ((wy if k == 5 or not fold else wy - 1) + ty - 1) // ty))
            x0 += 4 << k
    return out, fold


def lanes_of(wx, wy, fold, k, x0, it):
    lanes = np.arange(64)
    cx, cy = x0 + 4 * (lanes & ((1 << k) - 1)), it * (64 >> k) + (lanes >> k)
    if fold and k == 5:
        m_ = cy == wy
        cx, cy = np.where(m_, cx + 128, cx), np.where(m_, wy - 1, cy)
    return cx, cy


def marker_free_brute(wx, wy, k, x0, it0, n_it, fold):
    """no lane of the task's lane-iterations has both a valid and an invalid candidate"""
    for it in range(it0, it0 + n_it):
        cx, cy = lanes_of(wx, wy, fold, k, x0, it)
        n_valid = sum(((cy < wy) & (cx + j < wx)).astype(int) for j in range(4))
        if ((n_valid > 0) & (n_valid < 4)).any():
            return False
    return True


def marker_free(wx, wy, k, it0, n_it):
    """me_task_marker_free (me_kernels.hpp)"""
    if not wx & 3:
        return True
    quads = (wx + 3) >> 2
    if quads & -quads == 1 << k:
        return False
    fold = bool(quads & 32) and bool(quads & 31) and bool(wy & 1)
    return not (fold and k == 5 and 2 * (it0 + n_it) > wy)


_TREES = {}


def tree(pk):
    if pk not in _TREES:
        _TREES[pk] = G.Tree(1, pk).build()
    return _TREES[pk]


def model_search_pk2(cur, ref, origin, lt, rb, pred, lq, iters_per_task=2):
    """tests/test_tree_pkmin.py model_search_pk with the PK = 2 kernel's additions: the body per task, and the recovery of j for the
    slots of the 16x16 level (even rows x 2 where FEN halves the rows).  -> (table, lane-iterations run by each body)"""
    wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
    ox, oy = origin[0] + lt[0], origin[1] + lt[1]
    win = np.zeros((wy + 63, G.PDW * 4), np.uint8)
    w = ref[oy:oy + wy + 63, ox:ox + min(G.PDW * 4, ref.shape[1] - ox)]
    win[:w.shape[0], :w.shape[1]] = w
    slot_of = tree(2).slot_of_lane()
    best64 = np.full(593, (1 << 64) - 1, dtype=np.uint64)
    ran = {True: 0, False: 0}
    pp, fold = parts(wx, wy)
    for k, x0, iters in pp:
        ty = 64 >> k
        for it0 in range(0, iters, iters_per_task):
            best = np.full((G.N_GROUPS, 64), 0xFFFFFFFF, np.uint32)
            n_it = min(iters_per_task, iters - it0)
            mfree = marker_free(wx, wy, k, it0, n_it)
            ran[mfree] += n_it
            for it in range(n_it):
                cx, cy = lanes_of(wx, wy, fold, k, x0, it0 + it)
                c = np.zeros((4, 64), np.uint32)
                pkm = np.zeros((4, 64), np.uint32)
                ctag = np.zeros(64, np.uint32)
                for l in range(64):
                    for j in range(4):
                        cost = mv_cost(lq, lt[0] + int(cx[l]) + j, lt[1] + int(cy[l]), pred)
                        valid = cy[l] < wy and cx[l] + j < wx
                        c[j, l] = ((cost if valid else INV) << IDX) | (it << 8) | (l << 2) | j
                        pkm[j, l] = cost if valid else G.PK_MARKER
                    ctag[l] = ((0 if (cy[l] < wy and cx[l] < wx) else INV) << IDX) | (it << 8) | (l << 2)
                lane_off = (np.minimum(cy, wy - 1) * G.PDW + (np.minimum(cx, wx - 1) >> 2)) * 4
                G.simulate(tree(2 if mfree else True), win, cur, lane_off, c, best, pk=(pkm, ctag))
            for g in range(G.N_GROUPS):
                for l in range(64):
                    s, key = slot_of[g, l], int(best[g, l])
                    cost = key >> IDX
                    if s < 0 or cost >= INV:
                        continue
                    kit, kl, kj = (key >> 8) & 3, (key >> 2) & 63, key & 3
                    assert kj == 0 or not P.slot_rect(s) and not (mfree and slot_rect2(s))
                    bx = x0 + 4 * (kl & ((1 << k) - 1)) + kj
                    byy = (it0 + kit) * ty + (kl >> k)
                    if fold and k == 5 and byy == wy:
                        bx, byy = bx + 128, wy - 1
                    v = np.uint64((cost << 32) | (byy << 16) | bx)
                    if v < best64[s]:
                        best64[s] = v
    out = np.zeros((593, 3), np.int64)
    for s in range(593):
        v = int(best64[s])
        x, y, cost = v & 0xffff, (v >> 16) & 0xffff, v >> 32
        if slot_rect2(s):      # me_pk_recover<true>: the first valid candidate of the quad at x & ~3 whose cost is the minimum
            rx, ry, rw, rh, step = slot_rect2(s)
            xq = x & ~3
            blk = cur[ry:ry + rh:step, rx:rx + rw].astype(np.int64)
            hits = [j for j in range(4) if xq + j < wx and
                    step * int(np.abs(win[y + ry:y + ry + rh:step, xq + j + rx:xq + j + rx + rw].astype(np.int64) - blk).sum())
                    + mv_cost(lq, lt[0] + xq + j, lt[1] + y, pred) == cost]
            assert hits, ("no candidate of the winning quad has the minimum", s)
            assert x == xq or x == xq + hits[0], "a winner that came with its j is the first of its quad with that cost"
            x = xq + hits[0]
        mvx, mvy = lt[0] + x, lt[1] + y
        out[s] = (mvx, mvy, cost - mv_cost(lq, mvx, mvy, pred))
    return out, ran


def both(cur, ref, origin, lt, rb, pred, lq, want_bodies=(True, True)):
    old = T.model_search(G.Tree(1).build(), cur, ref, origin, lt, rb, pred, lq)
    new, ran = model_search_pk2(cur, ref, origin, lt, rb, pred, lq)
    assert np.array_equal(old, new), np.argwhere((old != new).any(axis=1)).ravel()[:20]
    assert (ran[True] > 0, ran[False] > 0) == want_bodies, ran      # (marker-free body ran, marker body ran)
    return old


def noise(seed, shape=(160, 264)):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


def test_operation_counts_meet_the_stop_rule():
    """the generator's count: at least 250 VALU instructions below the packed-minimum tree, class by class what PK2_CLASSES says"""
    pk, pk2 = G.valu_count(tree(True)), G.valu_count(tree(2))
    plain = G.valu_count(G.Tree(1).build())
    assert (plain[0], pk[0], pk2[0]) == (5708, 5260, 4956) and pk[0] - pk2[0] >= 250
    choice = G.pk2_choice()
    assert choice == {"16x8": True, "16x4": True, "8x16": True, "16x12": True, "4x16+12x16": True}
    for name, (n, mx, old, new, above) in G.PK2_CLASSES.items():
        assert name == "16x16" and mx > G.PK2_SLOT_MAX or (mx <= G.PK2_SLOT_MAX and new + above < old), name
    gain = sum(old - new - above for name, (n, mx, old, new, above) in G.PK2_CLASSES.items() if choice.get(name))
    assert 16 * gain == pk[0] - pk2[0] == 304
    assert sum(n for name, (n, mx, old, new, above) in G.PK2_CLASSES.items() if choice.get(name)) == 12
    # per slot: every packed slot is one PKMIN / PKMINE (4 instructions where keys + minimum are 6), every other one a MIN4 of keys
    kinds = dict(zip([s for s in tree(2).emitted if s is not None], [o[0] for o in tree(2).ops if o[0] in ("MIN4", "PKMIN", "PKMINE")]))
    for s in range(593):
        r = slot_rect2(s)
        assert kinds[s] == ("MIN4" if r is None else "PKMINE" if r[4] == 2 else "PKMIN"), s
        if r:
            assert r[2] * r[3] * 255 <= (G.PK_SLOT_MAX if max(r[2], r[3]) <= 8 else G.PK2_SLOT_MAX)
    assert sum(1 for s in range(593) if slot_rect2(s)) == 320 + 192
    assert G.PK2_SLOT_MAX == 48960 and G.PK2_COST_MAX == 16575 == (GATE2_LQ * MAX_BITS) >> 16
    assert np.array_equal(tree(2).slot_of_lane(), G.Tree(1).build().slot_of_lane())


def test_slot_rectangles_are_the_slot_table_s():
    from hmme import api
    for s in range(593):
        x, y, w, h = api.slot_rect(s)
        r = slot_rect2(s)
        assert (r[:4] if r else None) == ((x, y, w, h) if max(w, h) <= 16 and (w, h) != (16, 16) else None), s


@pytest.mark.parametrize("wx", [16, 17, 19, 22])
def test_random_content_in_both_bodies(wx):
    """16 candidates per row: every task marker-free; 17 / 19 / 22: the part of the last quad (1 / 3 / 2 valid candidates) runs the marker
    body, the parts before it the marker-free one"""
    ref = noise(wx)
    cur = np.clip(ref[40:104, 50:114].astype(np.int64) + np.random.default_rng(1).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    both(cur, ref, (48, 36), (-8, -6), (-8 + wx - 1, 4), (9, -14), 3794534, (True, wx != 16))     # lambda 57.9


@pytest.mark.parametrize("wx", [129, 132])
def test_folded_last_row(wx):
    """33 quads and five rows: the 32-quad part's third (last) iteration, a task of its own, holds row 4 and, folded into its idle lane row,
    the 33rd quad of row 4 -- partly valid at 129 (marker body), whole at 132 (everything marker-free); its first two run marker-free"""
    ref = noise(wx, (100, 264))
    cur = np.clip(ref[20:84, 70:134].astype(np.int64) + np.random.default_rng(2).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    both(cur, ref, (64, 18), (-64, -1), (-64 + wx - 1, 3), (-3, 5), 3794534, (True, wx == 129))


def test_every_cost_ties():
    """flat pictures, lambda 0: every candidate of every slot costs the same, the first one in raster order wins everywhere"""
    ref = np.full((160, 200), 77, np.uint8)
    out = both(np.full((64, 64), 77, np.uint8), ref, (48, 36), (-8, -6), (10, 4), (0, 0), 0)
    assert (out[:, 0] == -8).all() and (out[:, 1] == -6).all() and (out[:, 2] == 0).all()


@pytest.mark.parametrize("j", [1, 3])
def test_winner_inside_its_quad(j):
    """the current block is a copy of the reference at window column 8 + j, row 5: every slot's winner is candidate j of its quad"""
    ref = noise(100 + j)
    lt, origin = (-8, -6), (48, 36)
    x, y = origin[0] + lt[0] + 8 + j, origin[1] + lt[1] + 5
    cur = ref[y:y + 64, x:x + 64].copy()
    out = both(cur, ref, origin, lt, (10, 4), (0, 0), 0)
    assert (out[:, 0] == lt[0] + 8 + j).all() and (out[:, 1] == lt[1] + 5).all() and (out[:, 2] == 0).all()


@pytest.mark.parametrize("wx", [16, 17])
def test_sums_at_the_class_maxima_and_mv_cost_at_the_gate(wx):
    """|cur - ref| = 255 everywhere: 16x4 / 4x16 cost 16 320, 16x8 / 8x16 32 640, 16x12 / 12x16 48 960; the largest lambda the new gate
    admits at a window and a predictor at the ends of int16: the MV cost reaches 16 575 and the largest packed cost 65 535"""
    lt, pred = (32750, 32757), (-32768, -32768)
    assert mv_cost(GATE2_LQ, lt[0], lt[1], pred) == G.PK2_COST_MAX and T.cbits((lt[0] << 2) - pred[0]) == 37
    ref = np.full((160, 200), 255, np.uint8)
    out = both(np.zeros((64, 64), np.uint8), ref, (-lt[0], -lt[1]), lt, (lt[0] + wx - 1, lt[1] + 10), pred, GATE2_LQ, (True, wx == 17))
    assert (out[256, 2], out[448, 2], out[480, 2], out[288, 2], out[352, 2], out[320, 2]) == (16320, 32640, 32640, 48960, 48960, 16320)


def test_gate_is_pinned_at_both_thresholds():
    from hmme import api
    api.build()
    L = api.load()
    L.hmme_test_pk_body.argtypes = [C.c_uint32, C.c_int]
    L.hmme_test_pk_body.restype = C.c_int
    assert ((GATE2_LQ * MAX_BITS) >> 16) + 48960 == 65535 and (((GATE2_LQ + 1) * MAX_BITS) >> 16) + 48960 == 65536
    assert [L.hmme_test_pk_body(lq, 1) for lq in (0, 3794534, GATE2_LQ, GATE2_LQ + 1, P.GATE_LQ, P.GATE_LQ + 1)] == [2, 2, 2, 1, 1, 0]
    assert [L.hmme_test_pk_body(lq, 0) for lq in (0, 3794534, GATE2_LQ, GATE2_LQ + 1, P.GATE_LQ, P.GATE_LQ + 1)] == [1, 1, 1, 1, 1, 0]
    for lq in (1 << 25, (1 << 32) // MAX_BITS, (1 << 32) // MAX_BITS + 1, 0xFFFFFFFF):     # the product would wrap: never packed
        assert L.hmme_test_pk_body(lq, 1) == 0 and L.hmme_test_pk_body(lq, 0) == 0
    assert GATE2_LQ / 65536 > 223.9       # lambda 224


def test_task_predicate_equals_a_brute_force_lane_map():
    """wx 1..132, odd and even wy (with and without the fold, one and several iterations per part): a task runs the marker-free body
    exactly where none of its lanes is partly valid -- for single lane-iterations (split launches) and for the runs of 2 and 4 that a
    whole-job launch deals"""
    from hmme import api
    api.build()
    L = api.load()
    L.hmme_test_pk_task_marker_free.argtypes = [C.c_int] * 5
    L.hmme_test_pk_task_marker_free.restype = C.c_int
    n = {0: 0, 1: 0}
    for wx in range(1, 133):
        for wy in (1, 2, 8, 9, 128, 129):
            pp, fold = parts(wx, wy)
            for k, x0, iters in pp:
                if not iters:      # one folded row: the narrow parts have no row left
                    continue
                tasks = {(it, 1) for it in range(iters)} | {(it, min(2, iters - it)) for it in range(0, iters, 2)} | {(max(0, iters - 4), min(4, iters))}
                if iters > 6:      # the middle of a long part is all alike
                    tasks = {t for t in tasks if t[0] < 3 or t[0] + t[1] > iters - 3}
                for it0, n_it in tasks:
                    want = marker_free_brute(wx, wy, k, x0, it0, n_it, fold)
                    assert marker_free(wx, wy, k, it0, n_it) == want, (wx, wy, k, it0, n_it)
                    assert L.hmme_test_pk_task_marker_free(wx, wy, k, it0, n_it) == int(want), (wx, wy, k, it0, n_it)
                    n[int(want)] += 1
    assert n[0] > 1000 and n[1] > 1000
    # the benchmark's window: 64 of its 67 lane-iterations are marker-free
    pp, fold = parts(129, 129)
    assert sum(iters for k, x0, iters in pp) == 67
    assert sum(marker_free_brute(129, 129, k, x0, it, 1, fold) for k, x0, iters in pp for it in range(iters)) == 64
