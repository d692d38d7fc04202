"""Integer-MV tables the search would not produce, for the refinement at caller-chosen MVs (tests/test_refine_tables_cpu.py,
tests/test_gpu_refine_tables.py).  Plain numpy; the windows come from the ORACLE's hmo_set_search_range, so the expected side of a test never
takes its window from the code under test.

  oracle_windows(w, h, sr, pred_q, center_q)   int[n_ctu, 4]: lt_x, lt_y, rb_x, rb_y of every CTU, around the centre (None: the predictor)
  clamp(table, win)                            the table with every entry clamped to its CTU's window: what the oracle is given
  tables(win, sr, seed)                        name -> int16[n_ctu, 593, 2] for every kind below

  corners          slots dealt round-robin over the four corners and the four edge midpoints of the window (maximal sharing, furthest out)
  lt, rb, lb, rt   every slot on one corner: LT, RB, (LT.x, RB.y), (RB.x, LT.y)
  distinct         593 different in-window MVs per CTU (as many as the window holds where it holds fewer): no two slots share an item
  outside          per entry a seeded choice of which components leave the window (none, x, y, both) and how: 1 pel or SR pels beyond either
                   side, +32767, -32768
  mixed            distinct with a seeded third of the entries from `outside` and a third from `corners`

  frac_edge_cases()   the per-PU cases of tests/golden/frac_edges.npz (window corners, clipMv extremes, far predictors)
"""
import ctypes as C

import numpy as np

NUM_PARTS = 593
ONE_CORNER = ("lt", "rb", "lb", "rt")
KINDS = ("corners",) + ONE_CORNER + ("distinct", "outside", "mixed")


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def clip_limits(ctu, w, h):
    """TComDataCU::clipMv for the CTU in whole pels: (hor_min, ver_min, hor_max, ver_max)"""
    cx_n = (w + 63) // 64
    cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
    return -64 - 8 - cu_x + 1, -64 - 8 - cu_y + 1, w + 8 - cu_x - 1, h + 8 - cu_y - 1


def oracle_windows(w, h, sr, pred_q=None, center_q=None):
    import oracle_py
    L = oracle_py.oracle()
    cx_n = (w + 63) // 64
    n = n_ctus(w, h)
    mid = center_q if center_q is not None else pred_q
    win = np.zeros((n, 4), np.int64)
    v = [C.c_int() for _ in range(4)]
    for ctu in range(n):
        qx, qy = (int(mid[ctu][0]), int(mid[ctu][1])) if mid is not None else (0, 0)
        L.hmo_set_search_range(qx, qy, sr, (ctu % cx_n) * 64, (ctu // cx_n) * 64, w, h, 64, *[C.byref(a) for a in v])
        win[ctu] = [a.value for a in v]
    return win


def clamp(table, win):
    t = np.asarray(table).astype(np.int64)
    lo, hi = win[:, None, 0:2], win[:, None, 2:4]
    return np.minimum(np.maximum(t, lo), hi).astype(np.int16)


def eight_positions(wn):
    """the four corners, then the four edge midpoints"""
    ltx, lty, rbx, rby = (int(v) for v in wn)
    mx, my = (ltx + rbx) // 2, (lty + rby) // 2
    return np.array([(ltx, lty), (rbx, lty), (rbx, rby), (ltx, rby), (mx, lty), (rbx, my), (mx, rby), (ltx, my)], np.int64)


def _corners(wn):
    return eight_positions(wn)[np.arange(NUM_PARTS) % 8]


def _distinct(wn, rng):
    ltx, lty, rbx, rby = (int(v) for v in wn)
    wx, wy = rbx - ltx + 1, rby - lty + 1
    n = wx * wy
    pick = rng.choice(n, size=NUM_PARTS, replace=False) if n >= NUM_PARTS else rng.permutation(n)[np.arange(NUM_PARTS) % n]
    return np.stack([ltx + pick % wx, lty + pick // wx], axis=1)


def _outside(wn, sr, rng):
    ltx, lty, rbx, rby = (int(v) for v in wn)
    out = np.zeros((NUM_PARTS, 2), np.int64)
    which = rng.integers(0, 4, size=NUM_PARTS)              # 0: both inside, 1: x leaves, 2: y leaves, 3: both leave
    how = rng.integers(0, 4, size=(NUM_PARTS, 2))           # 0: 1 pel beyond, 1: SR pels beyond, 2: +32767, 3: -32768
    side = rng.integers(0, 2, size=(NUM_PARTS, 2))          # for 0 and 1: below lt or above rb
    for c, (lo, hi) in enumerate(((ltx, rbx), (lty, rby))):
        inside = rng.integers(lo, hi + 1, size=NUM_PARTS)
        step = np.where(how[:, c] == 0, 1, sr)
        beyond = np.where(side[:, c] == 0, lo - step, hi + step)
        beyond = np.where(how[:, c] == 2, 32767, np.where(how[:, c] == 3, -32768, beyond))
        out[:, c] = np.where((which >> c) & 1 == 1, beyond, inside)
    return out


def tables(win, sr, seed):
    """-> dict name -> int16[n_ctu, 593, 2]"""
    n = len(win)
    out = {k: np.zeros((n, NUM_PARTS, 2), np.int64) for k in KINDS}
    for ctu in range(n):
        rng = np.random.default_rng([seed, ctu])
        wn = win[ctu]
        pos = eight_positions(wn)
        out["corners"][ctu] = _corners(wn)
        out["lt"][ctu], out["rt"][ctu], out["rb"][ctu], out["lb"][ctu] = pos[0], pos[1], pos[2], pos[3]
        out["distinct"][ctu] = _distinct(wn, rng)
        out["outside"][ctu] = _outside(wn, sr, rng)
        order = rng.permutation(NUM_PARTS)
        third = NUM_PARTS // 3
        mixed = out["distinct"][ctu].copy()
        mixed[order[:third]] = out["outside"][ctu][order[:third]]
        mixed[order[third:2 * third]] = out["corners"][ctu][order[third:2 * third]]
        out["mixed"][ctu] = mixed
    for k, t in out.items():
        assert t.min() >= -32768 and t.max() <= 32767, k
    return {k: t.astype(np.int16) for k, t in out.items()}


# ---- the pictures and predictors the GPU tests use ---------------------------------------------------------------------------------------
FULL = dict(w=200, h=200, sr=128, ctu=5)          # the one interior CTU at (64, 64): window -128..128 in both directions
EDGE_W, EDGE_H = 136, 72                          # 3 x 2 CTUs, partial on the right, at the bottom and in the corner
FAR = 32764                                       # 8191 pels in quarter pels


def edge_predictors():
    """quarter-pel predictors for the 3 x 2 CTUs of the 136 x 72 picture: at SR 16 and beyond, every window reaches the clipMv limit(s) of the
    picture edge(s) its CTU lies on (-71 - cu on the left / at the top, picture + 7 - cu on the right / at the bottom)"""
    lo, hi = -60 * 4 + 1, 10 * 4 + 2                # fractional predictors: the MV cost is taken against the unrounded value
    return np.array([(lo, lo), (3, lo), (hi, lo), (lo, hi), (-2, hi), (hi, hi)], np.int16)


def far_predictors(direction):
    """all six CTUs' predictors 8191 pels away in one diagonal direction (sx, sy)"""
    return np.tile(np.array([direction[0] * FAR, direction[1] * FAR], np.int16), (6, 1))


DIAGONALS = ((-1, -1), (1, -1), (-1, 1), (1, 1))


def edge_picture(bd, seed=0):
    from hmme import synth
    cur, ref, _ = synth.make_pair(EDGE_W, EDGE_H, seed=4100 + bd + seed, bit_depth=bd, max_mv=5, region=32, noise_sigma=3.0)
    return cur, ref


def full_picture(bd):
    from hmme import synth
    cur, ref, _ = synth.make_pair(FULL["w"], FULL["h"], seed=4200 + bd, bit_depth=bd, max_mv=7, region=32, noise_sigma=3.0)
    return cur, ref


# ---- per-PU cases at the edges: what tests/golden/frac_edges.npz records from the reference --------------------------------------------------
EDGE_COLUMNS = "picture bit_depth ctu slot int_x int_y pred_x pred_y had lambda_x10".split()   # picture: 0 = full_picture, 1 = edge_picture


def frac_edge_cases():
    """-> int64 [n, len(EDGE_COLUMNS)]: a seeded sample of slots (64x64 and slot 0 always among them)
      - on the four corners of the full 257 x 257 window at SR 128,
      - on the clipMv extreme of each of the four picture corners of the 136 x 72 picture (the block 71 samples outside the picture),
      - on the same extremes with a predictor 8191 pels away beyond them (the window of such a predictor is pinned to the extreme; the MV
        cost is at its largest), lambda 0, 57.9 and 4000,
    at 8 and 10 bit, with Hadamard and with SAD"""
    rng = np.random.default_rng(20261)
    rows = []
    epred = edge_predictors()
    corner_ctus = (0, 2, 3, 5)
    for bd in (8, 10):
        for had in (1, 0):
            for (x, y) in ((-128, -128), (128, -128), (128, 128), (-128, 128)):
                for s in [592, 0] + [int(v) for v in rng.choice(np.arange(1, 592), size=5, replace=False)]:
                    rows.append((0, bd, FULL["ctu"], s, x, y, 0, 0, had, 579))
            for ctu, (sx, sy) in zip(corner_ctus, DIAGONALS):
                lim = clip_limits(ctu, EDGE_W, EDGE_H)
                x, y = lim[0] if sx < 0 else lim[2], lim[1] if sy < 0 else lim[3]
                for s in [592, 0] + [int(v) for v in rng.choice(np.arange(1, 592), size=5, replace=False)]:
                    rows.append((1, bd, ctu, s, x, y, int(epred[ctu, 0]), int(epred[ctu, 1]), had, 579))
                for lam10 in (0, 579, 40000):
                    for s in [592] + [int(v) for v in rng.choice(592, size=3, replace=False)]:
                        rows.append((1, bd, ctu, s, x, y, sx * FAR, sy * FAR, had, lam10))
    return np.array(rows, np.int64)


def run_edge_case(oracle_lib, row, planes, table, use_ref=False):
    """one row of frac_edge_cases on the oracle (or, use_ref, the compiled reference) -> (half_x, half_y, qter_x, qter_y, cost)"""
    from hmme import synth
    pic, bd, ctu, s, ix, iy, px, py, had, lam10 = (int(v) for v in row)
    cur, ref = planes[(pic, bd)]
    w = FULL["w"] if pic == 0 else EDGE_W
    cx_n = (w + 63) // 64
    x, y, bw, bh = (int(v) for v in table[s])
    ox, oy = synth.MARGIN + (ctu % cx_n) * 64 + x, synth.MARGIN + (ctu // cx_n) * 64 + y
    lam = lam10 / 10.0
    lam_arg = lam if use_ref else oracle_lib.oracle().hmo_lambda_q16(lam)
    return tuple(int(v) for v in oracle_lib.frac_refine(cur, (ox, oy), ref, (ox, oy), bw, bh, (ix, iy), (px, py), lam_arg, had, bd, use_ref=use_ref))


def edge_case_planes():
    return {(pic, bd): (full_picture(bd) if pic == 0 else edge_picture(bd)) for pic in (0, 1) for bd in (8, 10)}


# ---- every (picture, search range, window centres) the GPU tests refine at -------------------------------------------------------------------
FAMILY_SR = 12
COLLAPSED_SR = (1, 16)
SLIVERS = ((8, 8, 8), (72, 8, 32))                # w, h, sr: two of the pictures of test_tiny_and_sliver_pictures


def sliver_predictors(w, h):
    from hmme import synth
    return synth.random_predictors(n_ctus(w, h), seed=3, max_pel=5)


def family_predictors():
    """predictors and (different) window centres for the weighted and bi-prediction launches on the 136 x 72 picture; two centres lie far
    enough out for clipMv to cut their windows"""
    from hmme import synth
    pred = synth.random_predictors(6, seed=51, max_pel=8)
    center = synth.random_predictors(6, seed=52, max_pel=8)
    center[0] = (-70 * 4 + 1, -66 * 4)
    center[5] = (12 * 4 + 3, 9 * 4)
    return pred, center


def multi_pair_predictors():
    from hmme import synth
    return np.stack([synth.random_predictors(6, seed=61 + i, max_pel=20) for i in range(3)])


def gpu_window_cases():
    """-> list of (name, w, h, sr, centres int16[n_ctu, 2] | None)"""
    out = [("full", FULL["w"], FULL["h"], FULL["sr"], None)]
    out += [("edges", EDGE_W, EDGE_H, sr, edge_predictors()) for sr in (16, 64)]
    out += [("far", EDGE_W, EDGE_H, sr, far_predictors(d)) for d in DIAGONALS for sr in COLLAPSED_SR]
    out += [("sliver", w, h, sr, sliver_predictors(w, h)) for w, h, sr in SLIVERS]
    pred, center = family_predictors()
    out += [("family", EDGE_W, EDGE_H, FAMILY_SR, pred), ("family centre", EDGE_W, EDGE_H, FAMILY_SR, center)]
    out += [("multi", EDGE_W, EDGE_H, 16, p) for p in multi_pair_predictors()]
    return out
