"""The partition decision of hmme_select_pairs_device restated from the rule in include/hmme.h ("partition decision and motion field from
the 593-slot tables"): recursive, one CU at a time, the geometry from api.slot_index / api.slot_rect, the MV cost the caller's (the oracle's
hmo_mv_cost in the tests).  This is the reference of tests/test_gpu_select.py -- written from the rule, not from the kernel -- and the table
recipe those tests feed.  Host arithmetic only (Python integers: no width to overflow)."""
import functools

import numpy as np

PART_SIZES = (0, 1, 2, 4, 5, 6, 7)
NO_SLOT = 0xFFFF
U32_MAX = 0xFFFFFFFF


def z_index(x, y):
    """z-order address, in 4x4 units, of the sample (x, y) of a CTU"""
    x4, y4, z = x >> 2, y >> 2, 0
    for b in range(4):
        z |= ((x4 >> b) & 1) << (2 * b) | ((y4 >> b) & 1) << (2 * b + 1)
    return z


@functools.lru_cache(maxsize=None)
def cu_shapes(depth, x, y, aligned8):
    """[(part_size, (slot, ...))] of the CU at (x, y) of the CTU: every PartSize the tables hold for it, in enum order; aligned8 keeps only
    those whose PU rectangles are 8-aligned in position and size"""
    from hmme import api
    out = []
    for ps in PART_SIZES:
        slots = tuple(api.slot_index(ps, depth, i, z_index(x, y)) for i in range(1 if ps == 0 else 2))
        if any(s < 0 for s in slots):
            continue
        if aligned8 and any(v % 8 for s in slots for v in api.slot_rect(s)):
            continue
        out.append((ps, slots))
    return out


@functools.lru_cache(maxsize=None)
def rect(slot):
    from hmme import api
    return api.slot_rect(slot)


def select_ctu(mv, cost, sel, ctu_x, ctu_y, pic_w, pic_h, pred=(0, 0), lambda_q16=0, mv_cost=None):
    """mv int16[593, 2], cost uint32[593] of one CTU at (ctu_x, ctu_y) of a pic_w x pic_h picture -> (field int16[per, 2], slot uint16[per],
    cost, leaves) with leaves = [(depth, part_size)] of the coded CUs.  mv_cost(lambda_q16, x, y, pred_x, pred_y, scale) = hmo_mv_cost."""
    per = int(sel.mv_per_ctu)
    g = 8 if per == 64 else 4
    n = 64 // g

    def slot_cost(s):
        c = int(cost[s])
        if sel.price_mv:
            c += int(mv_cost(int(lambda_q16), int(mv[s, 0]), int(mv[s, 1]), int(pred[0]), int(pred[1]), 2 if sel.mv_unit else 0))
        return c

    def own_best(depth, x, y):
        best = None
        for ps, slots in cu_shapes(depth, x, y, per == 64):
            if not (sel.part_mask >> ps) & 1:
                continue
            c = int(sel.cu_cost) + sum(slot_cost(s) + int(sel.pu_cost) for s in slots)
            if best is None or c < best[0]:            # strict: the lower enum wins ties
                best = (c, ps, slots)
        return best

    def decide(depth, x, y):
        """-> (cost, [(depth, part_size, slots)]) of the CU"""
        s = 64 >> depth
        px, py = ctu_x + x, ctu_y + y
        if depth == sel.max_depth:
            if px < pic_w and py < pic_h:              # exists: its origin is inside the picture
                c, ps, slots = own_best(depth, x, y)
                return c, [(depth, ps, slots)]
            return 0, []                               # does not exist: costs 0, codes nothing
        kids = [decide(depth + 1, x + dx * (s // 2), y + dy * (s // 2)) for dy in (0, 1) for dx in (0, 1)]
        split = sum(k[0] for k in kids)
        if depth >= sel.min_depth and px + s <= pic_w and py + s <= pic_h:   # may be a leaf
            c, ps, slots = own_best(depth, x, y)
            if not split < c:                          # the parent wins ties
                return c, [(depth, ps, slots)]
        return split, [leaf for k in kids for leaf in k[1]]

    total, coded = decide(0, 0, 0)
    field = np.zeros((n, n, 2), np.int16)
    slot = np.full((n, n), NO_SLOT, np.uint16)
    for _, _, slots in coded:
        for s in slots:
            x, y, w, h = rect(s)
            v = mv[s].astype(np.int32)
            if sel.mv_unit:
                v = v << 2
            field[y // g:(y + h) // g, x // g:(x + w) // g] = v.astype(np.int16)   # keeps the low 16 bits
            slot[y // g:(y + h) // g, x // g:(x + w) // g] = s
    return field.reshape(per, 2), slot.reshape(per), min(total, U32_MAX), [(d, ps) for d, ps, _ in coded]


def select_picture(mv, cost, sel, pic_w, pic_h, ctu_first=0, pred=None, lambda_q16=0, mv_cost=None):
    """tables of the CTUs [ctu_first, ctu_first + len(mv)) of one picture -> (field [count, per, 2], slot [count, per], cost uint32[count], leaves)"""
    ctus_x = (pic_w + 63) // 64
    fields, slots, costs, leaves = [], [], [], []
    for k in range(mv.shape[0]):
        ctu = ctu_first + k
        p = (0, 0) if pred is None else pred[ctu]
        f, s, c, lv = select_ctu(mv[k], cost[k], sel, (ctu % ctus_x) * 64, (ctu // ctus_x) * 64, pic_w, pic_h, p, lambda_q16, mv_cost)
        fields.append(f); slots.append(s); costs.append(c); leaves += lv
    return np.stack(fields), np.stack(slots), np.array(costs, np.uint32), leaves


def random_tables(n_ctu, seed, noise=2):
    """the table recipe: per CTU a 64x64 map d of integers 1..5; a slot's cost = the sum of d over its rectangle + integers(0, noise * w * h)
    + integers(0, 60); MVs random in +-200 -> (mv int16[n_ctu, 593, 2], cost uint32[n_ctu, 593])"""
    rng = np.random.default_rng(seed)
    mv = rng.integers(-200, 201, size=(n_ctu, 593, 2)).astype(np.int16)
    cost = np.zeros((n_ctu, 593), np.uint32)
    for c in range(n_ctu):
        d = rng.integers(1, 6, size=(64, 64))
        for s in range(593):
            x, y, w, h = rect(s)
            cost[c, s] = int(d[y:y + h, x:x + w].sum()) + int(rng.integers(0, noise * w * h)) + int(rng.integers(0, 60))
    return mv, cost
