"""CPU check of the full-task twin of the 8-bit reduction tree (tools/gen_me_tree.py, Tree(1, pk=3): the 512 packed slots of the
marker-free twin leave the lane as 16-bit minima, two to a register, and take the butterfly levels on lane bits 5 and 4 -- the two lowest
bits of the quad index in that body's lane layout -- on the packed minima; keys are formed afterwards, for a quarter as many values, and
name a 16-candidate group).  The generator's numpy interpreter runs the op lists of me_tree_pk3_fen1.inc and me_tree_pk_fen1.inc inside a
Python model of the kernel's task loop -- each task with the body and the lane layout the kernel's predicate gives it -- flush and
recovery of the candidate inside its group, and must give what the same model gives with the 32-bit tree (which tests/test_tree_sim.py
pins to the reference goldens) for all 593 slots.  The operation count is held against the stop rule (700 VALU instructions below the
marker-free tree), the slot map must be a permutation, the task predicate is held against a brute-force lane map, and the lane layout
against the LDS bank rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_me_tree as G  # noqa: E402
import test_tree_pkmin2 as P2  # noqa: E402
import test_tree_sim as T  # noqa: E402

INV, IDX = T.INV, T.IDX
mv_cost, slot_rect2, parts, lanes_of, tree, noise = P2.mv_cost, P2.slot_rect2, P2.parts, P2.lanes_of, P2.tree, P2.noise
LQ = 3794534      # lambda 57.9


def guided(iters):
    """me_guided (me_kernels.hpp): the task sizes of a whole-job launch -> [(it0, n_it)]"""
    n4 = (iters - 8 + 3) >> 2 if iters > 8 else 0
    rem = iters - 4 * n4
    n2 = (rem - 2 + 1) >> 1 if rem > 2 else 0
    out, it = [], 0
    for n, size in ((n4, 4), (n2, 2), (rem - 2 * n2, 1)):
        for _ in range(n):
            out.append((it, size))
            it += size
    assert it == iters
    return out


def model_search_pk3(cur, ref, origin, lt, rb, pred, lq, tasks_of=None):
    """tests/test_tree_pkmin2.py model_search_pk2 with the full-task twin: body, lane layout and slot map per task (me_task_full), and the
    recovery over the 16-candidate group for entries whose quad is the first of one.  -> (table, lane-iterations run by each body)"""
    wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
    ox, oy = origin[0] + lt[0], origin[1] + lt[1]
    win = np.zeros((wy + 63, G.PDW * 4), np.uint8)
    w = ref[oy:oy + wy + 63, ox:ox + min(G.PDW * 4, ref.shape[1] - ox)]
    win[:w.shape[0], :w.shape[1]] = w
    slot_of = {True: tree(3).slot_of_lane(), False: tree(True).slot_of_lane()}
    best64 = np.full(593, (1 << 64) - 1, dtype=np.uint64)
    ran = {True: 0, False: 0}
    pp, fold = parts(wx, wy)
    for k, x0, iters in pp:
        ty = 64 >> k
        for it0, n_it in (tasks_of(iters) if tasks_of else [(i, min(2, iters - i)) for i in range(0, iters, 2)]):
            best = np.full((G.N_GROUPS, 64), 0xFFFFFFFF, np.uint32)
            full = G.task_full(wx, wy, k, it0, n_it)
            ran[full] += n_it
            for it in range(n_it):
                if full:
                    lx, ly = G.full_layout(k)
                    cx, cy = x0 + 4 * lx, (it0 + it) * ty + ly
                    assert (cy < wy).all() and (cx + 3 < wx).all() and x0 % 16 == 0
                else:
                    cx, cy = lanes_of(wx, wy, fold, k, x0, it0 + it)
                    lx, ly = G.LANES & ((1 << k) - 1), G.LANES >> k
                vl = (ly << k) | lx                     # the key's lane field: raster order inside the lane-iteration
                c = np.zeros((4, 64), np.uint32)
                pkm = np.zeros((4, 64), np.uint32)
                ctag = np.zeros(64, np.uint32)
                for l in range(64):
                    for j in range(4):
                        cost = mv_cost(lq, lt[0] + int(cx[l]) + j, lt[1] + int(cy[l]), pred)
                        valid = cy[l] < wy and cx[l] + j < wx
                        c[j, l] = ((cost if valid else INV) << IDX) | (it << 8) | (int(vl[l]) << 2) | j
                        pkm[j, l] = cost if valid else G.PK_MARKER
                    ctag[l] = ((0 if (cy[l] < wy and cx[l] < wx) else INV) << IDX) | (it << 8) | (int(vl[l]) << 2)
                    if full:
                        ctag[l] = (it << 8) | ((int(vl[l]) & ~3) << 2)
                lane_off = (np.minimum(cy, wy - 1) * G.PDW + (np.minimum(cx, wx - 1) >> 2)) * 4
                G.simulate(tree(3 if full else True), win, cur, lane_off, c, best, pk=(pkm, ctag))
            for g in range(G.N_GROUPS):
                for l in range(64):
                    s, key = slot_of[full][g, l], int(best[g, l])
                    cost = key >> IDX
                    if s < 0 or cost >= INV:
                        continue
                    kit, kl, kj = (key >> 8) & 3, (key >> 2) & 63, key & 3
                    if full and slot_rect2(s):
                        assert kj == 0 and kl & 3 == 0, "a packed slot's key of a full task names the first quad of a group"
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
        if slot_rect2(s):      # me_pk_recover<true>: the group of 16 where the entry's quad is the first of one, its quad otherwise
            rx, ry, rw, rh, step = slot_rect2(s)
            xq = x & ~3
            blk = cur[ry:ry + rh:step, rx:rx + rw].astype(np.int64)
            hits = [xc for xc in range(xq, min(xq + (4 if xq & 12 else 16), wx)) if
                    step * int(np.abs(win[y + ry:y + ry + rh:step, xc + rx:xc + rx + rw].astype(np.int64) - blk).sum())
                    + mv_cost(lq, lt[0] + xc, lt[1] + y, pred) == cost]
            assert hits, ("no candidate of the winning group has the minimum", s)
            assert x == xq or x == hits[0], "a winner that came with its j is the first of its group with that cost"
            x = hits[0]
        mvx, mvy = lt[0] + x, lt[1] + y
        out[s] = (mvx, mvy, cost - mv_cost(lq, mvx, mvy, pred))
    return out, ran


def both(cur, ref, origin, lt, rb, pred, lq, want_bodies, tasks_of=None):
    old = T.model_search(G.Tree(1).build(), cur, ref, origin, lt, rb, pred, lq)
    new, ran = model_search_pk3(cur, ref, origin, lt, rb, pred, lq, tasks_of)
    assert np.array_equal(old, new), np.argwhere((old != new).any(axis=1)).ravel()[:20]
    assert (ran[True] > 0, ran[False] > 0) == want_bodies, ran      # (full-task body ran, twin body ran)
    return old, ran


def test_operation_count_meets_the_stop_rule():
    """at least 700 VALU instructions below the marker-free tree's 4 956, and as many with every merge at its price in the ISA"""
    pk2, pk3 = G.valu_count(tree(2)), G.valu_count(tree(3))
    assert pk2[0] == 4956 and pk2[0] - pk3[0] >= 700
    assert (pk3[0], G.valu_count(tree(2), isa=True)[0], G.valu_count(tree(3), isa=True)[0]) == (3996, 4730, 3962)
    # the packed slots are the marker-free twin's 512; two packed levels, then one key per half, then four levels on keys
    assert (pk3[1]["PKMIN16"], pk3[1]["PMERGE"], pk3[1]["KEY16"], pk3[1]["MIN4"]) == (512, 128 + 64, 128, 81)
    assert sorted(o[5] for o in tree(3).ops if o[0] == "PKMIN16") == [s for s in range(593) if slot_rect2(s)]
    assert pk3[2] == [64 + 41, 32 + 21, 11, 6, 16 + 3, 8 + 2]         # the 81 slots with 32-bit keys keep the six-level butterfly
    # the pieces of the issue's table: 512 -> 128 keys; swap levels 384 packed; 192 + 96 on keys
    assert 128 * 2 + 64 * 2 == 384 and 2 * (64 + 32) == 192
    # even-row sums are doubled by the same 64-bit add (PKMINE's slots), all-row sums are not
    for o in tree(3).ops:
        if o[0] == "PKMIN16":
            assert o[4] == (slot_rect2(o[5])[4] == 2), o


def test_slot_map_is_a_permutation_of_the_593_slots():
    t = tree(3).slot_of_lane()
    assert t.shape == (G.N_GROUPS, 64) and sorted(int(v) for v in t.ravel() if v >= 0) == list(range(593))
    # the traced map is the closed form wherever there is one
    for pk in (False, True, 2):
        tr = tree(pk) if pk else G.Tree(1).build()
        assert np.array_equal(tr.slot_of_lane(), tr.slot_of_lane_traced())
    # a running-minimum register holds packed slots or slots with keys of their own, never both: the flush treats a register alike
    kinds = [{bool(slot_rect2(int(s))) for s in t[g] if s >= 0} for g in range(G.N_GROUPS)]
    assert all(len(kk) == 1 for kk in kinds) and sum(kk == {True} for kk in kinds) == 8


@pytest.mark.parametrize("wx,k", [(16, 2), (32, 3), (64, 4), (128, 5)])
@pytest.mark.parametrize("extra", [0, 1])
def test_full_tasks_of_every_part_size(wx, k, extra):
    """one part of 2^k quads; wy a multiple of its 64 >> k rows (two full lane-iterations) and one row more (the third, partial
    lane-iteration runs the twin)"""
    wy = 2 * (64 >> k) + extra
    ref = noise(wx + extra, (wy + 70, 264))
    cur = np.clip(ref[3:67, 30:94].astype(np.int64) + np.random.default_rng(k).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    out, ran = both(cur, ref, (24, 2), (-8, -1), (-8 + wx - 1, wy - 2), (9, -14), LQ, (True, bool(extra)))
    assert ran[True] == 2


@pytest.mark.parametrize("wx", [20, 48, 15, 12])
def test_parts_beside_a_full_one(wx):
    """20: k = 2 full and the one-quad part in the twin; 48: two full parts (k = 3, k = 2); 15: the cut quad lies in the k = 2 part,
    nothing is full; 12: no part with k >= 2"""
    ref = noise(wx, (100, 264))
    cur = np.clip(ref[5:69, 40:104].astype(np.int64) + np.random.default_rng(3).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    both(cur, ref, (36, 4), (-8, -2), (-8 + wx - 1, 13), (-3, 5), LQ, (wx in (20, 48), wx != 48))


@pytest.mark.parametrize("wx", [129, 131])
def test_fold_and_cut_quad_beside_full_tasks(wx):
    """33 quads, nine rows, the task sizes of a whole-job launch: iterations 0..3 of the 32-quad part are full, the folded fifth and the
    33rd quad's part run the twin"""
    ref = noise(wx, (100, 264))
    cur = np.clip(ref[20:84, 70:134].astype(np.int64) + np.random.default_rng(2).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    out, ran = both(cur, ref, (64, 18), (-64, -1), (-64 + wx - 1, 7), (-3, 5), LQ, (True, True), guided)
    assert ran[True] == 4


@pytest.mark.parametrize("lq", [0, LQ])
@pytest.mark.parametrize("period", [0, 4, 16, 64])
def test_ties_inside_and_between_groups(period, lq):
    """a flat reference (every SAD equal: MV cost and raster order alone decide), then references periodic in x: equal costs in
    neighbouring quads of one group (4), in neighbouring groups (16), in candidates 64 apart -- the pair a key without lane bit 4
    would confuse in the twin's layout"""
    if period:
        line = np.random.default_rng(period).integers(0, 256, size=period).astype(np.uint8)
        ref = np.tile(line, (80, 264 // period + 1))[:, :264].copy()
    else:
        ref = np.full((80, 264), 77, np.uint8)
    cur = ref[10:74, 40:104].copy()
    both(cur, ref, (30, 8), (-6, -2), (-6 + 127, 1), (11, -3), lq, (True, False))


@pytest.mark.parametrize("lq", [0, LQ])
def test_tie_in_the_next_row_at_a_smaller_x(lq):
    """every row is the row above shifted left by three samples: candidate (x - 3, y + 1) sees what (x, y) sees.  The first in raster
    order is the one in the upper row although its x is larger: a key must order by ly before any bit of lx"""
    line = np.random.default_rng(9).integers(0, 256, size=700).astype(np.uint8)
    ref = np.stack([line[3 * r:3 * r + 264] for r in range(80)])
    cur = ref[4:68, 44:108].copy()                      # the block at window (20, 4); equal at (23, 3), (26, 2), (29, 1), (32, 0)
    out, ran = both(cur, ref, (30, 2), (-6, -2), (-6 + 63, 5), (0, 0), lq, (True, False))
    if lq == 0:
        assert (out[:, 0] == -6 + 32).all() and (out[:, 1] == -2).all() and (out[:, 2] == 0).all()


@pytest.mark.parametrize("hi", [0, 255])
def test_sums_at_their_maximum_at_the_gate(hi):
    """|cur - ref| = 255 everywhere: 16x12 and 12x16 reach 48 960, with the largest MV cost the gate admits 65 535 in a u16 half"""
    lt, pred = (32750, 32757), (-32768, -32768)
    assert mv_cost(P2.GATE2_LQ, lt[0], lt[1], pred) == G.PK2_COST_MAX
    ref = np.full((160, 200), 255 - hi, np.uint8)
    out, ran = both(np.full((64, 64), hi, np.uint8), ref, (-lt[0], -lt[1]), lt, (lt[0] + 15, lt[1] + 10), pred, P2.GATE2_LQ, (False, True),
                    lambda iters: [(0, iters)])
    out, ran = both(np.full((64, 64), hi, np.uint8), ref, (-lt[0], -lt[1]), lt, (lt[0] + 15, lt[1] + 15), pred, P2.GATE2_LQ, (True, False))
    assert (out[256, 2], out[448, 2], out[480, 2], out[288, 2], out[352, 2], out[320, 2]) == (16320, 32640, 32640, 48960, 48960, 16320)


def full_brute(wx, wy, k, x0, it0, n_it, fold):
    """k >= 2 and every lane of the task's lane-iterations has four candidates inside the window, in a row of the part (none folded)"""
    rows = wy if k == 5 or not fold else wy - 1
    for it in range(it0, it0 + n_it):
        lanes = np.arange(64)
        cx, cy = x0 + 4 * (lanes & ((1 << k) - 1)), it * (64 >> k) + (lanes >> k)
        if k < 2 or (cy >= rows).any() or (cx + 3 >= wx).any():
            return False
    return True


def test_task_predicate_equals_a_brute_force_lane_map():
    from hmme import api
    api.build()
    L = api.load()
    L.hmme_test_pk_task_full.argtypes = [C.c_int] * 5
    L.hmme_test_pk_task_full.restype = C.c_int
    n = {0: 0, 1: 0}
    for wx in range(1, 133):
        for wy in range(1, 131):
            pp, fold = parts(wx, wy)
            for k, x0, iters in pp:
                if not iters:
                    continue
                tasks = {(it, 1) for it in range(iters)} | set(guided(iters)) | {(it, min(2, iters - it)) for it in range(0, iters, 2)}
                if iters > 6:
                    tasks = {t for t in tasks if t[0] < 2 or t[0] + t[1] > iters - 2}
                for it0, n_it in tasks:
                    want = full_brute(wx, wy, k, x0, it0, n_it, fold)
                    assert G.task_full(wx, wy, k, it0, n_it) == want, (wx, wy, k, it0, n_it)
                    assert L.hmme_test_pk_task_full(wx, wy, k, it0, n_it) == int(want), (wx, wy, k, it0, n_it)
                    if want:   # a full task is marker-free, and starts on a group
                        assert P2.marker_free(wx, wy, k, it0, n_it) and x0 % 16 == 0
                    n[int(want)] += 1
    assert n[0] > 10000 and n[1] > 10000
    # the benchmark's window under the guided sizes: exactly the tasks holding iterations 0..63 of the 32-quad part are full
    pp, fold = parts(129, 129)
    full_its = [(k, it) for k, x0, iters in pp for it0, n_it in guided(iters) if G.task_full(129, 129, k, it0, n_it) for it in range(it0, it0 + n_it)]
    assert full_its == [(5, it) for it in range(64)] and sum(iters for k, x0, iters in pp) == 67


def test_lane_layout_meets_the_lds_bank_rule():
    """ds_read2_b32 goes out as lanes 0..31 and 32..63, each dword of the pair on its own, bank = dword mod 32.  The 32-quad part's
    layout (the benchmark's) is conflict-free.  Lane bits 5 and 4 are the quad's two lowest bits in every part, so each half-wave holds
    every other quad of 16 >> (6 - k) groups in 64 >> k rows of 49 dwords; for k = 2..4 no assignment of lane bits 0..3 to the other
    quad bits and the rows changes WHICH dwords a half-wave reads, only which lane reads them: the layout with ly above lx (raster order
    in the key without a remap) is as good as any"""
    import itertools
    lx, ly = G.full_layout(5)
    assert G.lds_conflicts(lx, ly) == 1
    twin = {k: G.lds_conflicts(G.LANES & ((1 << k) - 1), G.LANES >> k) for k in (2, 3, 4, 5)}
    for k in (2, 3, 4):
        lx, ly = G.full_layout(k)
        # the four adjacent quads of a group sit in lanes l, l ^ 16, l ^ 32, l ^ 48
        assert all(len({int(ly[l ^ m]) for m in (0, 16, 32, 48)}) == 1 and sorted(int(lx[l ^ m]) & 3 for m in (0, 16, 32, 48)) == [0, 1, 2, 3]
                   and len({int(lx[l ^ m]) >> 2 for m in (0, 16, 32, 48)}) == 1 for l in range(16))
        chosen = G.lds_conflicts(lx, ly)
        best = chosen
        for perm in itertools.permutations(range(4)):      # lane bit b carries bit perm[b] of (ly << (k - 2) | lx >> 2)
            v = sum(((G.LANES >> b) & 1) << perm[b] for b in range(4))
            plx = ((G.LANES >> 5) & 1) | (((G.LANES >> 4) & 1) << 1) | ((v & ((1 << (k - 2)) - 1)) << 2)
            best = min(best, G.lds_conflicts(plx, v >> (k - 2)))
        assert chosen == best, (k, chosen, best)
    assert twin[5] == 1
