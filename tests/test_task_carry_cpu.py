"""CPU checks of the packed running minima that a wave of a whole-picture launch carries across the full tasks of one part
(me_search_kernel<1, 0, 2>, me_kernels.hpp: me_task_carry_fits, me_carry_index, me_carry_position):
  * the six iteration bits hold every lane-iteration of every full task, for every window up to 129 x 129 and every task the guided
    sizes and the split sizes (single lane-iterations, and the runs of up to four that a segment's wave draws) can make;
  * the ten-bit index is a bijection between what a part's full tasks can reach and (row, group), and its integer order is raster order;
  * the task-loop model of tests/test_tree_pkswap.py with waves that keep registers 0..7 across full tasks of one part -- keys with the
    absolute iteration, flushed before a task of another kind or part and at the end -- gives the table of the per-task flush, with the
    tasks dealt to several waves in turn and in a seeded random order."""
import ctypes as C

import numpy as np
import pytest

import test_tree_pkswap as S

G, P2 = S.G, S.P2
INV, IDX = S.INV, S.IDX


@pytest.fixture(scope="module")
def L():
    from hmme import api
    lib = api.load()
    lib.hmme_test_task_carry_fits.argtypes = [C.c_int] * 5
    lib.hmme_test_pk_task_full.argtypes = [C.c_int] * 5
    lib.hmme_test_carry_index.argtypes = [C.c_int] * 3
    lib.hmme_test_carry_position.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


def test_six_bits_hold_every_iteration_of_a_full_task(L):
    """me_task_full is monotone in it0 + n_it: the last full lane-iteration of a part bounds every task.  Every window; the library is
    asked about the guided tasks and the single lane-iterations at the end of every part, and about every task of a sample of windows"""
    n_full = 0
    for wx in range(1, 130):
        for wy in range(1, 130):
            pp, fold = P2.parts(wx, wy)
            for k, x0, iters in pp:
                if k < 2:
                    assert not G.task_full(wx, wy, k, 0, 1)
                    continue
                full_its = [it for it in range(iters) if G.task_full(wx, wy, k, it, 1)]
                last = len(full_its) - 1
                assert full_its == list(range(last + 1)) and last + 1 <= 64, (wx, wy, k, full_its)
                tasks = S.guided(iters)[-3:] + [(max(last, 0), 1), (min(last + 1, iters - 1), 1)]
                if (wx * 131 + wy) % 97 == 0:      # every task of any size a split launch can draw
                    tasks = S.guided(iters) + [(it0, n) for it0 in range(iters) for n in (1, 2, 3, 4) if it0 + n <= iters]
                for it0, n_it in tasks:
                    full = G.task_full(wx, wy, k, it0, n_it)
                    assert L.hmme_test_pk_task_full(wx, wy, k, it0, n_it) == int(full)
                    assert L.hmme_test_task_carry_fits(wx, wy, k, it0, n_it) == 1 and (not full or it0 + n_it <= 64)
                    n_full += full
    assert n_full > 20000
    # the bound is met: the 32-quad part of the full window, lane-iteration 63; a 65th full one would not fit
    assert G.task_full(129, 129, 5, 63, 1) and G.task_full(128, 129, 5, 60, 4) and not G.task_full(128, 129, 5, 64, 1)
    assert L.hmme_test_task_carry_fits(128, 130, 5, 64, 1) == 0 and L.hmme_test_pk_task_full(128, 130, 5, 64, 1) == 1, "a taller window would not fit"


@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_index_is_a_bijection_in_raster_order(L, k):
    ty, groups = 64 >> k, 1 << (k - 2)
    rows = 64 * ty                                   # 64 lane-iterations of ty rows
    out = (C.c_int * 2)()
    seen = {}
    for row in range(rows):
        for g in range(groups):
            idx = L.hmme_test_carry_index(k, row, g)
            assert 0 <= idx < 1024 and idx not in seen
            seen[idx] = (row, g)
            assert L.hmme_test_carry_position(k, idx, out) == 0 and (out[0], out[1]) == (row, g)
            # the kernel's form: absolute iteration above the lane field's upper four bits (ly << k | lx, lx = 4 * group + quad)
            assert idx == (row // ty) << 4 | (((row % ty) << k | 4 * g) >> 2)
    assert sorted(seen) == list(range(1024)), "onto: every ten-bit value is a place of the part"
    order = [seen[i] for i in range(1024)]
    assert order == sorted(order), "integer order is raster order"
    assert L.hmme_test_carry_index(k, 0, groups) == -1 and L.hmme_test_carry_index(1, 0, 0) == -1 and L.hmme_test_carry_position(k, 1024, out) == -1


def model_search_carried(L, cur, ref, origin, lt, rb, pred, lq, n_waves, seed=None):
    """tests/test_tree_pkswap.py model_search_pk3 with the whole-job kernel's task loop: the guided tasks of all parts are dealt to
    n_waves waves (in turn, or by a seeded draw); a wave keeps registers 0..7 across its full tasks of one part.
    -> (table, flushes of carried registers, full tasks)"""
    wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
    ox, oy = origin[0] + lt[0], origin[1] + lt[1]
    win = np.zeros((wy + 63, G.PDW * 4), np.uint8)
    w = ref[oy:oy + wy + 63, ox:ox + min(G.PDW * 4, ref.shape[1] - ox)]
    win[:w.shape[0], :w.shape[1]] = w
    slot_of = {True: S.tree(4).slot_of_lane(), False: S.tree(True).slot_of_lane()}
    best64 = np.full(593, (1 << 64) - 1, dtype=np.uint64)
    pp, fold = P2.parts(wx, wy)
    tasks = [(k, x0, it0, n_it) for k, x0, iters in pp for it0, n_it in S.guided(iters)]
    rng = np.random.default_rng(seed) if seed is not None else None
    owner = [int(rng.integers(n_waves)) if rng is not None else i % n_waves for i in range(len(tasks))]
    carried = [None] * n_waves                      # per wave: None or (k, x0, registers 0..7)
    out2 = (C.c_int * 2)()
    stats = {"flushes": 0, "full": 0}

    def merge(s, cost, y, x):
        v = np.uint64((cost << 32) | (y << 16) | x)
        if v < best64[s]:
            best64[s] = v

    def flush_carried(wv):
        k, x0, regs = carried[wv]
        carried[wv] = None
        stats["flushes"] += 1
        for g in range(8):
            for l in range(64):
                s, key = slot_of[True][g, l], int(regs[g, l])
                assert s >= 0 and P2.slot_rect2(s) and key >> IDX < INV, "registers 0..7 of a full task: packed slots, every lane valid"
                assert L.hmme_test_carry_position(k, key & 1023, out2) == 0
                merge(s, key >> IDX, out2[0], x0 + 16 * out2[1])

    for (k, x0, it0, n_it), wv in zip(tasks, owner):
        ty = 64 >> k
        full = G.task_full(wx, wy, k, it0, n_it)
        if carried[wv] is not None and not (full and carried[wv][:2] == (k, x0)):
            flush_carried(wv)
        best = np.full((G.N_GROUPS, 64), 0xFFFFFFFF, np.uint32)
        if full and carried[wv] is not None:
            best[:8] = carried[wv][2]
        stats["full"] += full
        for it in range(n_it):
            if full:
                lx, ly = G.full_layout(k)
                cx, cy = x0 + 4 * lx, (it0 + it) * ty + ly
            else:
                cx, cy = P2.lanes_of(wx, wy, fold, k, x0, it0 + it)
                lx, ly = G.LANES & ((1 << k) - 1), G.LANES >> k
            vl = (ly << k) | lx
            c = np.zeros((4, 64), np.uint32)
            pkm = np.zeros((4, 64), np.uint32)
            ctag = np.zeros(64, np.uint32)
            for l in range(64):
                for j in range(4):
                    cost = S.mv_cost(lq, lt[0] + int(cx[l]) + j, lt[1] + int(cy[l]), pred)
                    valid = cy[l] < wy and cx[l] + j < wx
                    c[j, l] = ((cost if valid else INV) << IDX) | (it << 8) | (int(vl[l]) << 2) | j
                    pkm[j, l] = cost if valid else G.PK_MARKER
                ctag[l] = ((0 if (cy[l] < wy and cx[l] < wx) else INV) << IDX) | (it << 8) | (int(vl[l]) << 2)
                if full:       # the absolute iteration above the group: me_carry_index
                    assert it0 + it < 64
                    ctag[l] = ((it0 + it) << 4) | (int(vl[l]) >> 2)
                    assert ctag[l] == L.hmme_test_carry_index(k, int(cy[l]), (int(cx[l]) - x0) >> 4)
            lane_off = (np.minimum(cy, wy - 1) * G.PDW + (np.minimum(cx, wx - 1) >> 2)) * 4
            G.simulate(S.tree(4 if full else True), win, cur, lane_off, c, best, pk=(pkm, ctag))
        for g in range(8 if full else 0, G.N_GROUPS):      # per task: everything of the twin's, registers 8 and 9 of a full task
            for l in range(64):
                s, key = slot_of[full][g, l], int(best[g, l])
                cost = key >> IDX
                if s < 0 or cost >= INV:
                    continue
                assert not (full and P2.slot_rect2(s))
                kit, kl, kj = (key >> 8) & 3, (key >> 2) & 63, key & 3
                bx, byy = x0 + 4 * (kl & ((1 << k) - 1)) + kj, (it0 + kit) * ty + (kl >> k)
                if fold and k == 5 and byy == wy:
                    bx, byy = bx + 128, wy - 1
                merge(s, cost, byy, bx)
        if full:
            carried[wv] = (k, x0, best[:8].copy())
    for wv in range(n_waves):      # the counter has run dry
        if carried[wv] is not None:
            flush_carried(wv)
    out = np.zeros((593, 3), np.int64)
    for s in range(593):
        v = int(best64[s])
        x, y, cost = v & 0xffff, (v >> 16) & 0xffff, v >> 32
        if P2.slot_rect2(s):      # me_pk_recover<true>
            rx, ry, rw, rh, step = P2.slot_rect2(s)
            xq = x & ~3
            blk = cur[ry:ry + rh:step, rx:rx + rw].astype(np.int64)
            hits = [xc for xc in range(xq, min(xq + (4 if xq & 12 else 16), wx)) if
                    step * int(np.abs(win[y + ry:y + ry + rh:step, xc + rx:xc + rx + rw].astype(np.int64) - blk).sum())
                    + S.mv_cost(lq, lt[0] + xc, lt[1] + y, pred) == cost]
            assert hits, ("no candidate of the winning group has the minimum", s)
            x = hits[0]
        mvx, mvy = lt[0] + x, lt[1] + y
        out[s] = (mvx, mvy, cost - S.mv_cost(lq, mvx, mvy, pred))
    return out, stats["flushes"], stats["full"]


def pictures(kind, seed):
    ref = P2.noise(seed, (170, 264))
    if kind == "flat":      # every SAD ties: MV cost and raster order decide, across iterations, tasks and waves
        return np.full((64, 64), 90, np.uint8), np.full((170, 264), 90, np.uint8)
    if kind == "stripes":   # period 16 columns, 2 rows: equal costs in different lane-iterations and groups
        y, x = np.mgrid[0:170, 0:264]
        ref = (40 + 9 * (x % 16) + 60 * (y % 2)).astype(np.uint8)
        return ref[4:68, 32:96].copy(), ref
    cur = np.clip(ref[6:70, 44:108].astype(np.int64) + np.random.default_rng(seed).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    return cur, ref


@pytest.fixture(scope="module")
def carry_tree():
    """the model of test_tree_pkswap runs the tree the kernel runs (Tree(1, 4)) where it names Tree(1, 3)"""
    real = S.tree
    S.tree = lambda pk: P2.tree(4 if pk == 3 else pk)
    yield
    S.tree = real


@pytest.mark.parametrize("kind,wx,wy,pred,waves,seed", [
    ("noise", 80, 40, (11, -3), 2, None),        # k = 4: five full tasks, k = 2: one full task and the partial third iteration in the twin
    ("flat", 80, 40, (-150, 37), 3, 5),          # ties everywhere, the waves draw at random
    ("stripes", 128, 20, (2, 6), 2, None),       # the 32-quad part alone: ten lane-iterations, 4 + 2 + 2 + 1 + 1
    ("stripes", 81, 33, (0, 0), 1, None),        # a cut quad (its part never full), one wave carries through every full task of a part
])
def test_carried_minima_give_the_table_of_the_per_task_flush(L, carry_tree, kind, wx, wy, pred, waves, seed):
    cur, ref = pictures(kind, wx + wy)
    lt = (-(wx // 2), -(wy // 2))
    rb = (lt[0] + wx - 1, lt[1] + wy - 1)
    origin = (100, 50)
    per_task, ran = S.model_search_pk3(cur, ref, origin, lt, rb, pred, S.LQ, S.guided)
    got, flushes, full = model_search_carried(L, cur, ref, origin, lt, rb, pred, S.LQ, waves, seed)
    assert np.array_equal(got, per_task), np.argwhere((got != per_task).any(axis=1)).ravel()[:20]
    assert ran[True] > 0 and full >= 3 and 0 < flushes < full, (flushes, full)       # fewer flushes of registers 0..7 than full tasks
