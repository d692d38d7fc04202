"""Content on which candidates tie IN PART, and the analytic answers to it, for tests/test_ties_cpu.py, tests/test_gpu_ties.py and the tie
cases of tests/test_oracle_vs_ref.py.  Plain numpy, no GPU.  Where two candidates cost the same HM's answer is its loop order's alone:
xPatternSearch scans the window row by row with a strict `<` (the first in raster order wins), xPatternRefinement walks s_acMvRefineH, then
s_acMvRefineQ with a strict `<` (the first in table order wins; the tables differ in entries 3..6).  An all-candidate tie only pins the
first candidate; here some candidates tie and the others do not, so the order among them decides.

  skewed_lattice(w, h, px, py, s, bd, seed, shift)   (cur, ref): content periodic under (px, 0) and (s, py); every slot has SAD 0 on a skewed
                                                     lattice of candidates -- whose first point by rows is not its first point by columns
  tie_set(window, pred, lambda_q16, lattice, shift, picture)   the lattice candidates of smallest MV cost, and which of them is first
  two_match(bd, seed, a, b, size)                    a random pair with the centre CTU's block planted at the displacements a and b
  tie_predictor(a, b, lambda_q16)                    a predictor at which a and b cost the same
  refine_content(kind, w, h, bd, seed)               'flat', 'rows', 'cols': distortions that do not depend on one or both MV components
  refine_inputs(seed)                                the predictors and integer MVs of the refinement runs (256 x 256, 16 CTUs)
  flat_refine_model(int_mv, pred, lambda_q16)        HM's two refinement stages where the cost is the MV cost alone
"""
import math

import numpy as np

import lambda_cases as lc

LATTICES = ((2, 1, 1), (3, 1, 1), (5, 3, 2), (7, 2, 3))               # (px, py, s)
Q16_57_9 = int(math.floor(65536.0 * math.sqrt(57.9)))
SEARCH_LAMBDA_Q16 = (0, 1 << 13, 1 << 16, Q16_57_9)                  # 1 << 13: an eighth per bit, so MVs of several bit counts cost the same
REFINE_LAMBDAS = (0.0, 1.0, 57.9)
WP = (70, -9, 6, 32)                                                 # a non-identity weight hmme_weight_check accepts for search and refinement
LATTICE_SHIFT = (1, -1)                                              # cur(x, y) = ref(x + 1, y - 1): the lattice passes through the MV (1, -1)

# xPatternRefinement's point orders (TEncSearch.cpp s_acMvRefineH, s_acMvRefineQ) written out, and a plain 3 x 3 raster for comparison
REFINE_H = ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))
REFINE_Q = ((0, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1))
RASTER_3X3 = tuple((x, y) for y in (-1, 0, 1) for x in (-1, 0, 1))


def lambda_q16_of(lam):
    return int(math.floor(65536.0 * math.sqrt(lam)))


# the pictures of the lattice searches: 3 x 3 CTUs, CTU 4 with its whole window, the windows of the eight others clipped by the picture's limits
SEARCH_W = SEARCH_H = 192
SEARCH_CTUS = 9
PRED_SEEDS = {8: (1, 2, 3, 4), 64: (1,), 128: (1,)}                  # search range -> seeds of the predictor sets run at it


def search_predictors(sr, seed):
    from hmme import synth
    return synth.random_predictors(SEARCH_CTUS, seed=seed, max_pel=min(sr, 30))


# ---- the search: skewed periodic content ------------------------------------------------------------------------------------------------
def lattice_tile(px, py, bd, seed):
    """py x px samples, all different and at least a 32nd of the range apart, inside [maxv / 8, 3 * maxv / 4] (WP maps that into the sample range:
    the weighted form of the content needs no clip)"""
    maxv = (1 << bd) - 1
    rng = np.random.default_rng([seed, px, py, bd])
    n = px * py
    lo, hi = maxv // 8, (3 * maxv) // 4
    step = (hi - lo) // n
    assert step >= maxv // 32
    vals = lo + step * rng.permutation(n) + rng.integers(0, step // 2, size=n)
    assert len(set(vals.tolist())) == n
    return vals.reshape(py, px).astype(np.int64)


def lattice_value(tile, s, x, y):
    """T[y % py, (x - s * (y // py)) % px] at any integer coordinates: unchanged under (px, 0) and under (s, py)"""
    py, px = tile.shape
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return tile[y % py, (x - s * (y // py)) % px]


def skewed_lattice(w, h, px, py, s, bd, seed, shift=LATTICE_SHIFT, weight=None):
    """-> (cur, ref) padded int16 planes.  ref is the lattice function inside the picture, cur the same function at (x + shift_x, y + shift_y)
    (weight: the weighted reference, so that the WEIGHTED distortion is 0 on the lattice).  The margins are edge-replicated and break the
    period: a candidate whose block leaves the picture is off the lattice"""
    from hmme import synth
    tile = lattice_tile(px, py, bd, seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ref = lattice_value(tile, s, xx, yy)
    cur = lattice_value(tile, s, xx + shift[0], yy + shift[1])
    if weight is not None:
        weighted = ((int(weight[0]) * cur + int(weight[3])) >> int(weight[2])) + int(weight[1])
        assert weighted.min() >= 0 and weighted.max() <= (1 << bd) - 1
        cur = weighted
    return synth.pad_plane(cur), synth.pad_plane(ref)


def on_lattice(lattice, shift, x, y):
    px, py, s = lattice
    ex, ey = np.asarray(x, np.int64) - shift[0], np.asarray(y, np.int64) - shift[1]
    return (ey % py == 0) & ((ex - s * (ey // py)) % px == 0)


def window_costs(window, pred, lambda_q16):
    """getCost(getBits) of every integer candidate of the window -> int64 [rows, columns]"""
    ltx, lty, rbx, rby = (int(v) for v in window)
    bx = np.array([lc.component_bits(4 * x - int(pred[0])) for x in range(ltx, rbx + 1)], np.int64)
    by = np.array([lc.component_bits(4 * y - int(pred[1])) for y in range(lty, rby + 1)], np.int64)
    return ((int(lambda_q16) * (by[:, None] + bx[None, :])) & 0xFFFFFFFF) >> 16


def tie_set(window, pred, lambda_q16, lattice, shift, picture):
    """The analytic model of the 64x64 slot on skewed_lattice content.  window: (lt_x, lt_y, rb_x, rb_y); picture: (w, h, cu_x, cu_y).
    -> None where no lattice candidate has its block inside the picture, else a dict:
      members        int [n, 2], raster order: the candidates whose 64 x 64 block lies inside the picture, that are on the lattice (SAD 0) and
                     have the smallest MV cost among those -- the candidates that tie for the win
      raster_first   HM's answer; column_first: the first by columns (smallest x, then smallest y); last: the last in raster order"""
    ltx, lty, rbx, rby = (int(v) for v in window)
    w, h, cu_x, cu_y = picture
    ys, xs = np.mgrid[lty:rby + 1, ltx:rbx + 1]
    ok = on_lattice(lattice, shift, xs, ys) & (cu_x + xs >= 0) & (cu_x + xs + 64 <= w) & (cu_y + ys >= 0) & (cu_y + ys + 64 <= h)
    if not ok.any():
        return None
    cost = window_costs(window, pred, lambda_q16)
    ok &= cost == cost[ok].min()
    members = np.stack([xs[ok], ys[ok]], axis=1)     # boolean indexing walks row by row: raster order
    by_column = members[np.lexsort((members[:, 1], members[:, 0]))]
    return dict(members=members, raster_first=tuple(members[0]), column_first=tuple(by_column[0]), last=tuple(members[-1]), cost=int(cost[ok].min()))


def ties_in_one_quad(members, lt_x):
    """how many aligned groups of four window columns of one row hold two or more of the tied candidates"""
    groups = {}
    for x, y in members.tolist():
        groups[(y, (x - lt_x) // 4)] = groups.get((y, (x - lt_x) // 4), 0) + 1
    return sum(1 for n in groups.values() if n >= 2)


# ---- the search: one block planted twice ---------------------------------------------------------------------------------------------------
def centre_ctu(size):
    """-> (ctu number, cu_x, cu_y) of the CTU in the middle of a picture of whole CTUs"""
    w, h = size
    assert w % 64 == 0 and h % 64 == 0
    cx, cy = (w // 64) // 2, (h // 64) // 2
    return cy * (w // 64) + cx, 64 * cx, 64 * cy


def two_match(bd, seed, a, b, size):
    """-> (cur, ref) padded int16 planes of random samples; the reference holds the block of the picture's centre CTU at the displacements a
    and b.  The two copies do not overlap, so each of the 593 slots has SAD 0 at a and at b and a large SAD everywhere else"""
    from hmme import synth
    w, h = size
    _, cu_x, cu_y = centre_ctu(size)
    assert abs(a[0] - b[0]) >= 64 or abs(a[1] - b[1]) >= 64
    rng = np.random.default_rng([seed, bd])
    cur = rng.integers(0, 1 << bd, size=(h, w))
    ref = rng.integers(0, 1 << bd, size=(h, w))
    for dx, dy in (a, b):
        assert 0 <= cu_x + dx and cu_x + dx + 64 <= w and 0 <= cu_y + dy and cu_y + dy + 64 <= h
        ref[cu_y + dy:cu_y + dy + 64, cu_x + dx:cu_x + dx + 64] = cur[cu_y:cu_y + 64, cu_x:cu_x + 64]
    return synth.pad_plane(cur), synth.pad_plane(ref)


def raster_before(a, b):
    return (a[1], a[0]) < (b[1], b[0])


def tie_predictor(a, b, lambda_q16=Q16_57_9, reach=24):
    """a quarter-pel predictor with both fractions set at which the MVs a and b (integer pels) have the same bit count: the one nearest (0, 0)"""
    best = None
    for py in range(-reach, reach + 1):
        for px in range(-reach, reach + 1):
            if px % 4 == 0 or py % 4 == 0:
                continue
            if lc.mv_bits(4 * a[0], 4 * a[1], px, py) == lc.mv_bits(4 * b[0], 4 * b[1], px, py):
                if best is None or abs(px) + abs(py) < abs(best[0]) + abs(best[1]):
                    best = (px, py)
    assert best is not None, (a, b)
    assert lc.get_cost(lambda_q16, lc.mv_bits(4 * a[0], 4 * a[1], *best)) == lc.get_cost(lambda_q16, lc.mv_bits(4 * b[0], 4 * b[1], *best))
    return best


# (name, search range, a, b): a before b in raster order, b.x < a.x.  TILE = 129 (me_kernels.hpp kTileStep): a window beyond 129 x 129
# candidates is searched as 2 x 2 tiles counted from its top-left; at search range 128 tile 0 holds -128..0 and tile 1 holds 1..128
TWO_MATCH_8 = (
    ("one tile", 64, (40, -30), (-50, -29)),
    ("one tile of four", 128, (-30, -100), (-120, -20)),
    ("right tile then left tile one row lower", 128, (100, -50), (-100, -49)),
    ("vertically adjacent tiles", 128, (90, -70), (70, 80)),
    ("diagonal tiles", 128, (100, -80), (-90, 70)),
)
# the 16-bit kernel at search range 128: two column-parity passes over horizontal strips of the window
TWO_MATCH_16 = (
    ("different column parity", 128, (51, -20), (-40, -19)),
    ("one strip", 128, (90, -100), (-70, -99)),
    ("sixty rows apart", 128, (30, -100), (-100, -30)),
)
TILE = 129


def two_match_size(sr):
    return (192, 192) if sr <= 64 else (320, 320)


def tile_of(mv, sr):
    return ((mv[0] + sr) // TILE, (mv[1] + sr) // TILE)


# ---- the refinement ------------------------------------------------------------------------------------------------------------------------
RW = RH = 256
R_CTUS = 16
R_SR = 8
REFINE_KINDS = ("flat", "rows", "cols")


def refine_content(kind, w, h, bd, seed):
    """-> (cur, ref) padded int16 planes.
    flat: cur one constant, ref another -- every fractional position has the same distortion, the cost is the MV cost alone.
    rows: every row constant, a seeded profile down the picture (cur: the same profile one row further on, under a little per-row noise).  The
          interpolation filters reproduce a constant exactly, so the distortion does not depend on the horizontal component: the three
          horizontal offsets of every row of the 3 x 3 pattern tie in distortion.
    cols: its transpose"""
    from hmme import synth
    maxv = (1 << bd) - 1
    rng = np.random.default_rng([seed, bd])
    if kind == "flat":
        return synth.pad_plane(np.full((h, w), maxv // 3, np.int64)), synth.pad_plane(np.full((h, w), maxv // 2 + 3, np.int64))
    n = h if kind == "rows" else w
    walk = np.cumsum(rng.integers(-(maxv // 24), maxv // 24 + 1, size=n + 1))
    profile = np.clip(maxv // 2 + walk - walk[n // 2], maxv // 8, (3 * maxv) // 4)
    ref_p = profile[:n]
    cur_p = np.clip(profile[1:] + rng.integers(-2, 3, size=n), 0, maxv)
    if kind == "rows":
        cur, ref = np.repeat(cur_p[:, None], w, axis=1), np.repeat(ref_p[:, None], w, axis=1)
    else:
        cur, ref = np.repeat(cur_p[None, :], h, axis=0), np.repeat(ref_p[None, :], h, axis=0)
    return synth.pad_plane(cur), synth.pad_plane(ref)


def refine_inputs(seed=5):
    """-> (pred int16[16, 2], int_mv int16[16, 593, 2]) for a 256 x 256 picture.  CTU c has the predictor phase (c % 4, c // 4) in quarter pels
    on a seeded integer part of up to 2 pels; slot s has the integer MV round(pred) + ((s % 5) - 2, ((s // 5) % 5) - 2).  Phase p puts the
    offsets 4 * int_mv - pred on 4 * k - p (p < 2) or 4 * (k + 1) - p, k = -2..2: every offset from -9 to 10 occurs in both components, in
    every combination, and the 3 x 3 patterns around them reach -12 to 13.  Every integer MV lies in the window of search range 8"""
    rng = np.random.default_rng(seed)
    pred = np.zeros((R_CTUS, 2), np.int16)
    imv = np.zeros((R_CTUS, 593, 2), np.int16)
    s = np.arange(593)
    for c in range(R_CTUS):
        pred[c] = 4 * rng.integers(-2, 3, size=2) + (c % 4, c // 4)
        rx, ry = (int(pred[c, 0]) + 2) >> 2, (int(pred[c, 1]) + 2) >> 2
        imv[c, :, 0], imv[c, :, 1] = rx + (s % 5) - 2, ry + ((s // 5) % 5) - 2
    return pred, imv


def refine_offsets(pred, imv):
    """the set of (4 * int_mv - pred) pairs the inputs hold"""
    d = 4 * imv.astype(np.int64) - pred[:, None, :].astype(np.int64)
    return {(int(x), int(y)) for x, y in d.reshape(-1, 2)}


def flat_refine_model(int_mv, pred, lambda_q16, tables=(REFINE_H, REFINE_Q)):
    """xPatternSearchFracDIF where the distortion is the same at every position: the cost is the MV cost alone.  Half-pel stage over the first
    table (MV cost of the half-pel MV, TComRdCost cost scale 1), quarter-pel stage over the second around the half-pel winner (scale 0), both
    with a strict `<`.  -> (quarter-pel MV x, y, MV cost of the winner)"""
    best, half = None, (0, 0)
    for hx, hy in tables[0]:
        c = lc.get_cost(lambda_q16, lc.mv_bits(4 * int_mv[0] + 2 * hx, 4 * int_mv[1] + 2 * hy, int(pred[0]), int(pred[1])))
        if best is None or c < best:
            best, half = c, (hx, hy)
    bx, by = 4 * int(int_mv[0]) + 2 * half[0], 4 * int(int_mv[1]) + 2 * half[1]
    best, qter = None, (0, 0)
    for qx, qy in tables[1]:
        c = lc.get_cost(lambda_q16, lc.mv_bits(bx + qx, by + qy, int(pred[0]), int(pred[1])))
        if best is None or c < best:
            best, qter = c, (qx, qy)
    return bx + qter[0], by + qter[1], best


def flat_refine_tables(pred, imv, lambda_q16, tables=(REFINE_H, REFINE_Q)):
    """flat_refine_model over the tables of refine_inputs -> (qmv int16 [n, 593, 2], MV cost int64 [n, 593]); one evaluation per distinct offset"""
    q = np.zeros(imv.shape, np.int16)
    c = np.zeros(imv.shape[:2], np.int64)
    memo = {}
    for k in range(imv.shape[0]):
        p = (int(pred[k, 0]), int(pred[k, 1]))
        for s in range(imv.shape[1]):
            m = (int(imv[k, s, 0]), int(imv[k, s, 1]))
            if (m, p) not in memo:
                memo[m, p] = flat_refine_model(m, p, lambda_q16, tables)
            q[k, s, 0], q[k, s, 1], c[k, s] = memo[m, p]
    return q, c
