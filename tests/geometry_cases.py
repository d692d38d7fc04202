"""Picture sizes that are no multiple of 8, and what each reaches -- shared by tests/test_geometry_cpu.py (the models and the host arithmetic at
these sizes, no device) and tests/test_gpu_geometry.py (every call family on the device).  include/hmme.h states what happens at the picture
edge -- partial CTUs completed by edge replication, a CU at max_depth exists iff its origin is inside the picture, the difference is 0 outside,
stores go only to samples inside -- and none of it assumes a multiple of anything.  Each size is the smallest that can still fail:

    101 x 71      both odd, w mod 4 = 1, h mod 4 = 3; 2 x 2 CTUs, the last column 37 wide, the last row 7 tall; at SR 64 the window of the
                  last CTU is clipped to (-64, -64, 44, 14)
    65 x 67       the last CTU column ONE sample wide, the last row 3 tall; at SR 16 the last window is (-16, -16, 8, 10)
    130 x 66      even (the chroma calls take it), w mod 4 = 2; 3 x 2 CTUs; chroma planes of 65 x 33: an odd chroma size, the last chroma block
                  one sample wide and one row tall
    9 x 9         the minimum plus one: a single CTU whose blocks at x = 8 and y = 8 hold one sample
    16384 x 8,    the largest a plane accepts: 256 CTUs in a row / in a column
    8 x 16384
    (128 + 2k)    for k = 1..15, 4:2:0: chroma planes of (64 + k) x 9 -- every partial vector and dword of the plane-set kernels -- next to a
      x 18        luma plane that ends 2k samples past a vector boundary in the same launch
    2048 x 50     4:2:0 with 16 references at 8 bit: 51 planes side by side cap a launch at 20 row blocks per plane, luma has 25 (two rounds:
                  the strided row loop iterates twice) and chroma 7 (its workgroups beyond block 6 leave at once); stat_grid below shows it
    1033 x 66     luma alone with 16 references at 10 bit: rows of 130 vectors (one row per workgroup, the last vector holds 2 of 16 bytes); 17
                  planes / 16 pairs side by side cap a launch at 60 / 64 row blocks, the picture has 66 (two rounds of 33 workgroups)

Host arithmetic only; the window rule is restated here from TEncSearch::xSetSearchRange and TComDataCU::clipMv in Python integers."""
import numpy as np

ODD, NARROW, EVEN, MIN1 = (101, 71), (65, 67), (130, 66), (9, 9)
SLIVERS = ((16384, 8), (8, 16384))
TABLE = (ODD, NARROW, EVEN, MIN1) + SLIVERS
SEARCH_RANGE = {ODD: 64, NARROW: 16, MIN1: 8}
LAST_WINDOW = {ODD: (-64, -64, 44, 14), NARROW: (-16, -16, 8, 10)}      # of the last CTU, for a zero predictor
LAST_CTU = {ODD: (37, 7), NARROW: (1, 3), EVEN: (2, 2), MIN1: (9, 9)}    # width of the last CTU column, height of the last CTU row
PLANE_MIN, PLANE_MAX = 8, 16384
REFUSED_PLANES = ((7, 8), (8, 7), (16385, 8), (8, 16385))
STATS_SIZES = tuple((64 + k, 9) for k in range(1, 16))                    # rows that end 1..15 samples into a 16-sample vector
STATS_SIZES_420 = tuple((128 + 2 * k, 18) for k in range(1, 16))           # luma; chroma (64 + k) x 9: STATS_SIZES, luma 2k samples past a vector boundary
STAT_BLOCKS = 1024                                                        # kWpStatBlocks of hmme.hip
ROUNDS_420 = (2048, 50, 16)                                               # luma width, height, references of the 8-bit case whose luma rows take two rounds
ROUNDS_LUMA = (1033, 66, 16)                                              # width, height, references of the 10-bit luma case whose rows take two rounds
FAR = 4 * 400                                                             # quarter pels: beyond clipMv's range at every size but the slivers' long side
DIRECTIONS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
FUZZ_SEEDS = tuple(range(3000, 3010))


def dims(w, h):
    return (w + 63) // 64, (h + 63) // 64


def n_ctus(w, h):
    cx_n, cy_n = dims(w, h)
    return cx_n * cy_n


def ctu_origin(ctu, w):
    cx_n = (w + 63) // 64
    return (ctu % cx_n) * 64, (ctu // cx_n) * 64


def last_ctu(w, h):
    """(width of the last CTU column, height of the last CTU row) inside the picture"""
    return (w - 1) % 64 + 1, (h - 1) % 64 + 1


def clip_mv(qx, qy, cu_x, cu_y, w, h):
    """TComDataCU::clipMv (TComDataCU.cpp:2907-2920) for a 64 x 64 CTU: quarter pels, 8 samples beyond the picture"""
    hor_max, hor_min = (w + 8 - cu_x - 1) * 4, (-64 - 8 - cu_x + 1) * 4
    ver_max, ver_min = (h + 8 - cu_y - 1) * 4, (-64 - 8 - cu_y + 1) * 4
    return min(hor_max, max(hor_min, qx)), min(ver_max, max(ver_min, qy))


def window(pred_x, pred_y, sr, cu_x, cu_y, w, h):
    """TEncSearch::xSetSearchRange (TEncSearch.cpp:3814-3830): the clipped predictor -+ the range, each corner clipped, in whole pels
    -> (lt_x, lt_y, rb_x, rb_y)"""
    px, py = clip_mv(pred_x, pred_y, cu_x, cu_y, w, h)
    lt = clip_mv(px - 4 * sr, py - 4 * sr, cu_x, cu_y, w, h)
    rb = clip_mv(px + 4 * sr, py + 4 * sr, cu_x, cu_y, w, h)
    return lt[0] >> 2, lt[1] >> 2, rb[0] >> 2, rb[1] >> 2


def is_clipped(win, sr):
    """a window narrower or lower than the 2 * sr + 1 candidates of an unclipped one"""
    return win[2] - win[0] < 2 * sr or win[3] - win[1] < 2 * sr


def stat_grid(width, height, sample_bytes, n_y, stat_blocks=STAT_BLOCKS):
    """stat_grid of hmme.hip restated: the launch geometry of a reduction over a width x height plane, n_y planes (or pairs) side by side in
    one launch whose workgroups are capped at stat_blocks -> dict(lpr_log2, rows_per_block, row_blocks, cap, rounds, blocks): 16-byte vectors
    per row -> lanes per row (a power of two, 256 at most) -> rows per workgroup; the row blocks dealt evenly over the rounds the cap needs"""
    nvec = (width * sample_bytes + 15) // 16
    l = 0
    while (1 << l) < nvec and l < 8:
        l += 1
    rpb = 256 >> l
    row_blocks = (height + rpb - 1) // rpb
    cap = max(1, stat_blocks // n_y)
    rounds = (row_blocks + cap - 1) // cap
    return dict(lpr_log2=l, rows_per_block=rpb, row_blocks=row_blocks, cap=cap, rounds=rounds, blocks=(row_blocks + rounds - 1) // rounds)


def stat_grids_420(w, h, sample_bytes, n_refs, stat_blocks=STAT_BLOCKS):
    """the two set launches of hmme_wp_estimate_420 on a w x h luma picture with n_refs references, every plane distinct: the statistics of
    3 * (n_refs + 1) planes, the SADs of 3 * n_refs pairs -> {"stats" | "sad": (luma's grid, chroma's grid)}; a launch's x extent is the larger
    `blocks` of the two, and a workgroup whose first row block * rows_per_block lies beyond its plane's height leaves at once"""
    return {name: (stat_grid(w, h, sample_bytes, n_y, stat_blocks), stat_grid(w // 2, h // 2, sample_bytes, n_y, stat_blocks))
            for name, n_y in (("stats", 3 * (n_refs + 1)), ("sad", 3 * n_refs))}


def predictors(w, h, seed, max_pel=5):
    from hmme import synth
    return synth.random_predictors(n_ctus(w, h), seed=seed, max_pel=max_pel)


def far_fields(w, h):
    """eight fields of one MV per CTU, every CTU FAR away in one of the eight directions: clipMv leaves the CTU's block 70 or more samples
    outside the picture (where FAR exceeds its range) and the prediction reads the replicated border alone.  The component that does not
    point away carries a fractional MV, so that the interpolation runs there"""
    n = n_ctus(w, h)
    return [np.tile(np.array([dx * FAR + (5 if dx == 0 else 0), dy * FAR + (-7 if dy == 0 else 0)], np.int16), (n, 1, 1)) for dx, dy in DIRECTIONS]


def fuzz_size(seed):
    """w, h in 8..200 with no factor 8; every other seed forces an odd dimension, so that at least half of the cases have one"""
    rng = np.random.default_rng(seed + 77777)
    w, h = int(rng.integers(8, 201)), int(rng.integers(8, 201))
    if seed % 2 == 0:
        if rng.integers(0, 2):
            w = 2 * int(rng.integers(4, 100)) + 1
        else:
            h = 2 * int(rng.integers(4, 100)) + 1
    return w, h


def straddling_leaves(slot_map, w, h, per):
    """how many CUs of a slot map [n_ctu, per] have their origin inside the picture and reach beyond it"""
    import residual_model as rm
    count = 0
    for c in range(slot_map.shape[0]):
        x0, y0 = ctu_origin(c, w)
        for v in np.unique(slot_map[c]):
            if v == rm.NO_SLOT:
                continue
            _, (qx, qy, qs) = rm.slot_geometry(int(v))
            count += (x0 + qx < w < x0 + qx + qs) or (y0 + qy < h < y0 + qy + qs)
    return count
