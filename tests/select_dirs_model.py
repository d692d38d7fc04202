"""L0, L1 or bi per PU of hmme_select_dirs_device restated from the rule in include/hmme.h ("L0, L1 or bi per PU, and the prediction of a
picture whose blocks are L0, L1 or bi"): per slot the three candidates' costs in Python integers, then select_model.select_ctu -- the
partition rule -- on the merged slots with the MV cost switched off, then the two-list field.  Written from the header text, not from the
kernel: the reference of tests/test_gpu_select_dirs.py, and the table recipes those tests feed."""
import itertools

import numpy as np

import select_model as sm

NO_DIR = 0xFF
LAMBDA_Q16 = 500000                                        # lambda about 7.6 per bit, as tests/select_refs_model.py
HM_BITS = ((3, 3, 5), (2, 1))                              # HM-like: uiMbBits of a 2Nx2N PU {3, 3, 5}; refIdx + MVP bits per list
SIZES = ((64, 64), (100, 70), (136, 72))                   # one CTU; partial CTUs on two edges and the corner; the siblings' size


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def component_bits(v):
    """TComRdCost::xGetComponentBits: the exp-Golomb length of one MV difference"""
    t = ((-v) << 1) + 1 if v <= 0 else v << 1
    return 2 * (t.bit_length() - 1) + 1


def mvb(v, p):
    """HM's getBits at cost scale 0"""
    return component_bits(int(v[0]) - int(p[0])) + component_bits(int(v[1]) - int(p[1]))


def gc(lambda_q16, n):
    """TComRdCost::getCost: the product wraps in 32 bits"""
    return ((int(lambda_q16) * int(n)) & 0xFFFFFFFF) >> 16


def slot_candidates(mu, cu, mb, cb, pred, bits, lambda_q16):
    """rule steps 1 and 2 for one slot: mu / mb [2][2] MVs, cu / cb [2] costs, pred [2][2] -> (C [2], C_B [2])"""
    dir_bits, list_bits = bits
    bu = [mvb(mu[l], pred[l]) for l in range(2)]
    bb = [mvb(mb[l], pred[l]) for l in range(2)]
    c = [max(0, int(cu[l]) - gc(lambda_q16, bu[l])) + gc(lambda_q16, dir_bits[l] + list_bits[l] + bu[l]) for l in range(2)]
    c_b = [(max(0, int(cb[l]) - gc(lambda_q16, bb[l])) >> 1) + gc(lambda_q16, dir_bits[2] + list_bits[0] + list_bits[1] + bb[l] + bu[1 - l])
           for l in range(2)]
    return c, c_b


def decide(c, c_b):
    """rule steps 3 and 4 -> (direction, searched list of the bi candidate, the winner's cost)"""
    bl = 1 if c_b[1] < c_b[0] else 0                       # strict: list 0 is tried first
    if c_b[bl] <= c[0] and c_b[bl] <= c[1]:
        return 3, bl, c_b[bl]
    if c[0] <= c[1]:
        return 1, bl, c[0]
    return 2, bl, c[1]


def merge_ctu(mv_uni, cost_uni, mv_bi, cost_bi, pred, bits, lambda_q16):
    """the four table sets of one CTU (mv [2, 593, 2], cost [2, 593]) -> (mv int16[593, 2] of the winner in its list, cost [593] Python ints,
    direction [593], searched list [593])"""
    out_mv = np.zeros((593, 2), np.int16)
    out_cost, out_dir, out_bl = [0] * 593, [0] * 593, [0] * 593
    for s in range(593):
        c, c_b = slot_candidates(mv_uni[:, s], cost_uni[:, s], mv_bi[:, s], cost_bi[:, s], pred, bits, lambda_q16)
        d, bl, best = decide(c, c_b)
        out_cost[s], out_dir[s], out_bl[s] = best, d, bl
        out_mv[s] = mv_bi[bl, s] if d == 3 else mv_uni[d - 1, s]
    return out_mv, out_cost, out_dir, out_bl


def select_dirs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, pic_w, pic_h, bits, ctu_first=0, pred=None, lambda_q16=LAMBDA_Q16):
    """tables int16[2, count, 593, 2] / uint32[2, count, 593] of the CTUs [ctu_first, ctu_first + count) of one picture, uni_field
    int16[2, n_ctu, 64, 2], pred int16[2, n_ctu, 2] or None -> (field [2, count, 64, 2], dir uint8[count, 64], slot [count, 64],
    cost uint32[count])"""
    assert sel.mv_per_ctu == 64 and sel.mv_unit == 0 and sel.price_mv == 0
    count = mv_uni.shape[1]
    ctus_x = (pic_w + 63) // 64
    field = np.zeros((2, count, 64, 2), np.int16)
    dirs = np.full((count, 64), NO_DIR, np.uint8)
    slots, costs = [], []
    for k in range(count):
        ctu = ctu_first + k
        p = [(0, 0), (0, 0)] if pred is None else [pred[l][ctu] for l in range(2)]
        m_mv, m_cost, m_dir, m_bl = merge_ctu(mv_uni[:, k], cost_uni[:, k], mv_bi[:, k], cost_bi[:, k], p, bits, lambda_q16)
        f, s, c, _ = sm.select_ctu(m_mv, m_cost, sel, (ctu % ctus_x) * 64, (ctu // ctus_x) * 64, pic_w, pic_h)
        for b, v in enumerate(s.tolist()):
            if v == sm.NO_SLOT:
                continue                                   # (0,0) in both lists, no direction
            d, bl = m_dir[v], m_bl[v]
            dirs[k, b] = d
            if d == 3:
                field[bl, k, b] = f[b]
                field[1 - bl, k, b] = uni_field[1 - bl, ctu, b]   # the block's own entry: the motion the bi cost was measured with
            else:
                field[d - 1, k, b] = f[b]
        slots.append(s); costs.append(c)
    return field, dirs, np.stack(slots), np.array(costs, np.uint32)


# ---- table recipes -------------------------------------------------------------------------------------------------------------------------
def predictors(n_ctu, seed):
    """int16[2, n_ctu, 2], drawn independently per list and CTU, no component zero"""
    rng = np.random.default_rng(seed)
    pred = rng.integers(-40, 41, size=(2, n_ctu, 2)).astype(np.int16)
    pred[pred == 0] = 7
    return pred


def mv_cost_table(mv, pred, ctus, lambda_q16):
    """gc(mvb(mv, pred of the CTU)) for mv [count, 593, 2] of the CTUs `ctus`, pred [n_ctu, 2] or None -> int64[count, 593]"""
    out = np.zeros(mv.shape[:2], np.int64)
    for k, ctu in enumerate(ctus):
        p = (0, 0) if pred is None else pred[ctu]
        for s in range(593):
            out[k, s] = gc(lambda_q16, mvb(mv[k, s], p))
    return out


def random_dir_tables(n_ctu, count, seed, pred=None, first=0, lambda_q16=LAMBDA_Q16, base=0):
    """four table sets built as a refinement leaves them, distortion + MV cost: the distortions of select_model.random_tables (+ base) with
    a seed per set, doubled in the bi sets (whose distortion the rule halves); and the lists' fields, drawn apart from the tables
    -> (mv_uni, cost_uni, mv_bi, cost_bi [2, count, ...], uni_field int16[2, n_ctu, 64, 2])"""
    sets = [sm.random_tables(count, seed=seed + 1000 * k) for k in range(4)]
    ctus = range(first, first + count)
    mv = [t[0] for t in sets]
    cost = []
    for k, (m, d) in enumerate(sets):
        dist = (d.astype(np.int64) + base) * (2 if k >= 2 else 1)
        c = dist + mv_cost_table(m, None if pred is None else pred[k & 1], ctus, lambda_q16)
        assert c.max() <= 0xFFFFFFFF
        cost.append(c.astype(np.uint32))
    rng = np.random.default_rng(seed + 77)
    uni_field = rng.integers(-300, 301, size=(2, n_ctu, 64, 2)).astype(np.int16)
    return np.stack(mv[:2]), np.stack(cost[:2]), np.stack(mv[2:]), np.stack(cost[2:]), uni_field


def tie_sel(api):
    """the decision the tie tables are run with: CUs of 16x16 at most, so that a CTU holds enough PUs for every pattern's winner to be coded"""
    return api.SelectParams(64, min_depth=2)


TIE_PATTERNS = tuple(itertools.product((-1, 0, 1), repeat=3))   # (C[1], C_B[0], C_B[1]) - C[0]


def tie_tables(n_ctu, seed, bits, pred=None, lambda_q16=1 << 16):
    """random_dir_tables with list 1's and both bi costs rebuilt so that C[1], C_B[0], C_B[1] lie at C[0] - 1, C[0] or C[0] + 1: each slot
    takes one of the 27 patterns at random, so every tie of rules 3 and 4 and every strict neighbour occurs.  base keeps every distortion
    above the largest bit price (lambda 1 per bit here) -> (the five arrays, pattern index int[count, 593])"""
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = random_dir_tables(n_ctu, n_ctu, seed, pred, 0, lambda_q16, base=1000)
    cost_uni, cost_bi = cost_uni.copy(), cost_bi.copy()
    dir_bits, list_bits = bits
    rng = np.random.default_rng(seed + 5)
    pat = rng.integers(0, len(TIE_PATTERNS), size=(n_ctu, 593))
    for k in range(n_ctu):
        p = [(0, 0), (0, 0)] if pred is None else [pred[l][k] for l in range(2)]
        for s in range(593):
            bu = [mvb(mv_uni[l, k, s], p[l]) for l in range(2)]
            bb = [mvb(mv_bi[l, k, s], p[l]) for l in range(2)]
            c0 = int(cost_uni[0, k, s]) - gc(lambda_q16, bu[0]) + gc(lambda_q16, dir_bits[0] + list_bits[0] + bu[0])
            d1, db0, db1 = TIE_PATTERNS[pat[k, s]]
            cost_uni[1, k, s] = c0 + d1 - gc(lambda_q16, dir_bits[1] + list_bits[1] + bu[1]) + gc(lambda_q16, bu[1])
            for l, db in ((0, db0), (1, db1)):
                total = gc(lambda_q16, dir_bits[2] + list_bits[0] + list_bits[1] + bb[l] + bu[1 - l])
                cost_bi[l, k, s] = 2 * (c0 + db - total) + gc(lambda_q16, bb[l])
            c, c_b = slot_candidates(mv_uni[:, k, s], cost_uni[:, k, s], mv_bi[:, k, s], cost_bi[:, k, s], p, bits, lambda_q16)
            assert (c[1] - c[0], c_b[0] - c[0], c_b[1] - c[0]) == (d1, db0, db1)
    return (mv_uni, cost_uni, mv_bi, cost_bi, uni_field), pat
