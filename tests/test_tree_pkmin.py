"""CPU check of the packed-minimum twin of the 8-bit reduction tree (tools/gen_me_tree.py, Tree(fen, pk=True): the five slots of every
8x8 CU take their minimum on packed u16 costs, the key says which quad won, the candidate inside the quad is recovered afterwards).
The generator's numpy interpreter runs the op list that is emitted as me_tree_pk_fen*.inc inside a Python model of the kernel's task
loop, flush and j recovery (me_pk_recover), and must give what the same model gives with the 32-bit tree -- which tests/test_tree_sim.py
pins to the reference goldens -- on random content, on ties, with the winner at each position of its quad, with quads of 1, 2 and 3
valid candidates, and with the sums and the MV cost at the bounds the host's gate (me_pk_gate) admits.  The gate itself is pinned at
and just beyond its boundary."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_me_tree as G  # noqa: E402
import test_tree_sim as T  # noqa: E402

INV, IDX = T.INV, T.IDX
GATE_LQ = 29132523      # the largest lambda_q16 with (lambda_q16 * 74 >> 16) + 16 320 < 49 215
MAX_BITS = 74           # two components of at most 2 * 18 + 1 bits: int16 windows (integer pels) against int16 predictors (quarter pels)


def mv_cost(lq, x, y, pred):
    return ((lq * (T.cbits((x << 2) - pred[0]) + T.cbits((y << 2) - pred[1]))) & 0xFFFFFFFF) >> 16


def slot_rect(s):
    """the rectangles of me_pk_slot (me_kernels.hpp), or None for a slot of the 32-bit tree"""
    if s < 128:
        return (s & 7) * 8, (s >> 4) * 8 + ((s >> 3) & 1) * 4, 8, 4
    if s < 256:
        return ((s >> 1) & 7) * 8 + (s & 1) * 4, ((s - 128) >> 4) * 8, 4, 8
    if 384 <= s < 448:
        return (s & 7) * 8, ((s - 384) >> 3) * 8, 8, 8
    return None


def test_packed_slots_are_the_five_of_every_8x8_cu():
    from hmme import api
    for fen in (0, 1):
        tree = G.Tree(fen, pk=True).build()
        packed = sorted(s for s, op in zip([s for s in tree.emitted if s is not None],
                                           [o for o in tree.ops if o[0] in ("MIN4", "PKMIN")]) if op[0] == "PKMIN")
        assert packed == [s for s in range(593) if slot_rect(s)] and len(packed) == 320
        assert np.array_equal(tree.slot_of_lane(), G.Tree(fen).build().slot_of_lane())
    for s in range(593):
        x, y, w, h = api.slot_rect(s)
        assert slot_rect(s) == ((x, y, w, h) if max(w, h) <= 8 else None)
    assert G.PK_MARKER == 49215 and G.PK_SLOT_MAX == 16320 and G.PK_MARKER + G.PK_SLOT_MAX == 0xFFFF
    assert G.PK_COST_MAX == (GATE_LQ * MAX_BITS) >> 16 == 32894


def model_search_pk(tree, cur, ref, origin, lt, rb, pred, lq, iters_per_task=2):
    """tests/test_tree_sim.py model_search with the kernel's PK additions: packed MV costs and the j-less key constant per lane, and the
    recovery of j from the window for the packed slots"""
    wx, wy = rb[0] - lt[0] + 1, rb[1] - lt[1] + 1
    ox, oy = origin[0] + lt[0], origin[1] + lt[1]
    win = np.zeros((wy + 63, G.PDW * 4), np.uint8)
    w = ref[oy:oy + wy + 63, ox:ox + min(G.PDW * 4, ref.shape[1] - ox)]
    win[:w.shape[0], :w.shape[1]] = w
    slot_of = tree.slot_of_lane()
    best64 = np.full(593, (1 << 64) - 1, dtype=np.uint64)
    lanes = np.arange(64)
    quads = (wx + 3) >> 2
    fold = bool(quads & 32) and bool(quads & 31) and bool(wy & 1)
    x0 = 0
    for k in range(5, -1, -1):
        if not quads & (1 << k):
            continue
        ty = 64 >> k
        iters = ((wy if k == 5 or not fold else wy - 1) + ty - 1) // ty
        for it0 in range(0, iters, iters_per_task):
            best = np.full((G.N_GROUPS, 64), 0xFFFFFFFF, np.uint32)
            n_it = min(iters_per_task, iters - it0)
            lx, ly = lanes & ((1 << k) - 1), lanes >> k
            for it in range(n_it):
                cx = x0 + 4 * lx
                cy = (it0 + it) * ty + ly
                if fold and k == 5:
                    m_ = cy == wy
                    cx = np.where(m_, cx + 128, cx)
                    cy = np.where(m_, wy - 1, cy)
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
                G.simulate(tree, win, cur, lane_off, c, best, pk=(pkm, ctag))
            for g in range(G.N_GROUPS):
                for l in range(64):
                    s, key = slot_of[g, l], int(best[g, l])
                    cost = key >> IDX
                    if s < 0 or cost >= INV:
                        continue
                    kit, kl, kj = (key >> 8) & 3, (key >> 2) & 63, key & 3
                    assert kj == 0 or slot_rect(s) is None
                    bx = x0 + 4 * (kl & ((1 << k) - 1)) + kj
                    byy = (it0 + kit) * ty + (kl >> k)
                    if fold and k == 5 and byy == wy:
                        bx, byy = bx + 128, wy - 1
                    v = np.uint64((cost << 32) | (byy << 16) | bx)
                    if v < best64[s]:
                        best64[s] = v
        x0 += 4 << k
    out = np.zeros((593, 3), np.int64)
    for s in range(593):
        v = int(best64[s])
        xq, y, cost = v & 0xffff, (v >> 16) & 0xffff, v >> 32
        if slot_rect(s):       # me_pk_recover: the first valid candidate of the quad whose SAD + MV cost is the minimum
            rx, ry, rw, rh = slot_rect(s)
            blk = cur[ry:ry + rh, rx:rx + rw].astype(np.int64)
            hits = [j for j in range(4) if xq + j < wx and
                    int(np.abs(win[y + ry:y + ry + rh, xq + j + rx:xq + j + rx + rw].astype(np.int64) - blk).sum())
                    + mv_cost(lq, lt[0] + xq + j, lt[1] + y, pred) == cost]
            assert hits, ("no candidate of the winning quad has the minimum", s)
            xq += hits[0]
        mvx, mvy = lt[0] + xq, lt[1] + y
        out[s] = (mvx, mvy, cost - mv_cost(lq, mvx, mvy, pred))
    return out


def both(fen, cur, ref, origin, lt, rb, pred, lq):
    old = T.model_search(G.Tree(fen).build(), cur, ref, origin, lt, rb, pred, lq)
    new = model_search_pk(G.Tree(fen, pk=True).build(), cur, ref, origin, lt, rb, pred, lq)
    assert np.array_equal(old, new), np.argwhere((old != new).any(axis=1)).ravel()[:20]
    return old


def noise(seed, shape=(160, 200)):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.uint8)


@pytest.mark.parametrize("fen", [0, 1])
@pytest.mark.parametrize("wx", [17, 18, 19, 20])
def test_random_content_and_partly_valid_quads(fen, wx):
    """17 / 18 / 19 candidates per row: the last quad of a row has 1 / 2 / 3 valid candidates (20: four)"""
    ref = noise(wx)
    cur = np.clip(ref[40:104, 50:114].astype(np.int64) + np.random.default_rng(1).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    both(fen, cur, ref, (48, 36), (-8, -6), (-8 + wx - 1, 4), (9, -14), 3794534)     # lambda 57.9


def test_every_cost_ties():
    """flat pictures, lambda 0: every candidate of every slot costs the same, the first one in raster order wins everywhere"""
    ref = np.full((160, 200), 77, np.uint8)
    out = both(1, np.full((64, 64), 77, np.uint8), ref, (48, 36), (-8, -6), (10, 4), (0, 0), 0)
    assert (out[:, 0] == -8).all() and (out[:, 1] == -6).all() and (out[:, 2] == 0).all()


@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_winner_at_each_place_of_its_quad(j):
    """the current block is a copy of the reference at window column 8 + j, row 5: every slot's winner is candidate j of its quad"""
    ref = noise(100 + j)
    lt, origin = (-8, -6), (48, 36)
    x, y = origin[0] + lt[0] + 8 + j, origin[1] + lt[1] + 5
    cur = ref[y:y + 64, x:x + 64].copy()
    out = both(1, cur, ref, origin, lt, (10, 4), (0, 0), 0)
    assert (out[:, 0] == lt[0] + 8 + j).all() and (out[:, 1] == lt[1] + 5).all() and (out[:, 2] == 0).all()


@pytest.mark.parametrize("fen", [0, 1])
def test_sums_and_mv_cost_at_the_bounds_of_the_gate(fen):
    """|cur - ref| = 255 everywhere (the 8x8 sums are 16 320) and the largest lambda the gate admits, at a window and a predictor at the
    ends of int16: a component costs 37 bits, the MV cost reaches PK_COST_MAX, cost + sum the last value below the marker -- also in
    rows whose last quad has one valid candidate beside three markers"""
    lt, pred = (32750, 32757), (-32768, -32768)
    assert mv_cost(GATE_LQ, lt[0], lt[1], pred) == G.PK_COST_MAX and T.cbits((lt[0] << 2) - pred[0]) == 37
    ref = np.full((160, 200), 255, np.uint8)
    out = both(fen, np.zeros((64, 64), np.uint8), ref, (-lt[0], -lt[1]), lt, (lt[0] + 16, lt[1] + 10), pred, GATE_LQ)
    assert out[384, 2] == 16320 and out[0, 2] == 8160


def test_gate_is_pinned_at_its_boundary():
    from hmme import api
    api.build()
    L = api.load()
    L.hmme_test_pk_gate.argtypes = [C.c_uint32]
    L.hmme_test_pk_gate.restype = C.c_int
    assert L.hmme_test_pk_gate(GATE_LQ) == 1 and L.hmme_test_pk_gate(GATE_LQ + 1) == 0
    assert ((GATE_LQ * MAX_BITS) >> 16) + G.PK_SLOT_MAX == G.PK_MARKER - 1 and (((GATE_LQ + 1) * MAX_BITS) >> 16) + G.PK_SLOT_MAX == G.PK_MARKER
    assert L.hmme_test_pk_gate(0) == 1 and L.hmme_test_pk_gate(3794534) == 1            # lambda 0 and the benchmark's 57.9
    for lq in (1 << 25, 1 << 26, (1 << 32) // MAX_BITS, (1 << 32) // MAX_BITS + 1, 0xFFFFFFFF, 6000000 << 16 & 0xFFFFFFFF):
        want = lq * MAX_BITS < (1 << 32) and ((lq * MAX_BITS) >> 16) + G.PK_SLOT_MAX < G.PK_MARKER
        assert L.hmme_test_pk_gate(lq) == int(want), lq
    assert L.hmme_test_pk_gate(1 << 25) == 0     # lambda 512: beyond the packed costs, the 32-bit tree runs
