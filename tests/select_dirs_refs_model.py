"""L0, L1 or bi and the reference index per list, per PU, of hmme_select_dirs_refs_device restated from the rule in include/hmme.h ("B pictures
with several references per list", the decision): per slot the candidates' costs in Python integers, then select_model.select_ctu -- the
partition rule -- on the merged slots with the MV cost switched off, then the two-list field and the two reference fields.  Built on
select_dirs_model (mvb, gc) and written from the header text, not from the kernel: the reference of tests/test_gpu_select_dirs_refs.py, and
the table recipes those tests feed.  Line numbers are TEncSearch.cpp's."""
import numpy as np

import select_dirs_model as dm
import select_model as sm

NO_REF = 0xFF
NO_DIR = dm.NO_DIR
LAMBDA_Q16 = dm.LAMBDA_Q16


class Bits:
    """hmme_dir_refs_params as the model takes it"""

    def __init__(self, dir_bits, n_refs, ref_bits, l1_valid_mask=None):
        self.dir_bits = tuple(dir_bits)
        self.n_refs = tuple(n_refs)
        self.ref_bits = tuple(tuple(r) for r in ref_bits)
        self.l1_valid_mask = (1 << n_refs[1]) - 1 if l1_valid_mask is None else l1_valid_mask
        assert all(len(self.ref_bits[l]) >= self.n_refs[l] for l in range(2))


def hm_bits(n0, n1, mask=None, mvp_bits=1):
    """HM-like: uiMbBits of a 2Nx2N PU {3, 3, 5}; HM's reference-index bits (:3030-3037) plus one MVP-index bit per reference"""
    from select_refs_model import hm_ref_idx_bits
    return Bits((3, 3, 5), (n0, n1), ([hm_ref_idx_bits(n0, r) + mvp_bits for r in range(n0)], [hm_ref_idx_bits(n1, r) + mvp_bits for r in range(n1)]), mask)


def slot_decide(mu, cu, mb, cb, pred, bits, lambda_q16):
    """one slot.  mu / mb [2][R][2] MVs, cu / cb [2][R] costs, pred [2][R][2] -> (direction, searched list of the bi candidate, the winner's
    cost, its MV, (ref index list 0, list 1) with NO_REF for a list the winner does not name -- under direction 3 the list the bi candidate
    did NOT search is NO_REF here: its index is the block's own entry of uni_ref)"""
    gc, mvb = dm.gc, dm.mvb
    c, ru, mot, c_b, rb = [None, None], [0, 0], [0, 0], [None, None], [0, 0]
    c_v, rv = None, None
    for l in range(2):
        for r in range(bits.n_refs[l]):                     # rule 1 (:3027-3094)
            bu = mvb(mu[l][r], pred[l][r])
            p = max(0, int(cu[l][r]) - gc(lambda_q16, bu)) + gc(lambda_q16, bits.dir_bits[l] + bits.ref_bits[l][r] + bu)
            if c[l] is None or p < c[l]:                    # strict, order 0, 1, ... (:3086)
                c[l], ru[l], mot[l] = p, r, bits.ref_bits[l][r] + bu   # (:3154-3155)
            if l == 1 and (bits.l1_valid_mask >> r) & 1 and (c_v is None or p < c_v):   # rule 2 (:3096-3104, :3282-3285)
                c_v, rv = p, r
    for l in range(2):
        for r in range(bits.n_refs[l]):                     # rule 3 (:3208-3247, :3808)
            bb = mvb(mb[l][r], pred[l][r])
            p = (max(0, int(cb[l][r]) - gc(lambda_q16, bb)) >> 1) + gc(lambda_q16, bits.dir_bits[2] + bits.ref_bits[l][r] + bb + mot[1 - l])
            if c_b[l] is None or p < c_b[l]:                # strict (:3226)
                c_b[l], rb[l] = p, r
    bl = 1 if c_b[1] < c_b[0] else 0                        # list 0's unless list 1's is strictly cheaper
    if c_b[bl] <= c[0] and (c_v is None or c_b[bl] <= c_v):  # rule 4 (:3291)
        refs = [NO_REF, NO_REF]
        refs[bl] = rb[bl]
        return 3, bl, c_b[bl], mb[bl][rb[bl]], tuple(refs)
    if c_v is None or c[0] <= c_v:                          # (:3314)
        return 1, bl, c[0], mu[0][ru[0]], (ru[0], NO_REF)
    return 2, bl, c_v, mu[1][rv], (NO_REF, rv)


def merge_ctu(mv_uni, cost_uni, mv_bi, cost_bi, pred, bits, lambda_q16):
    """the table sets of one CTU (mv [2, R, 593, 2], cost [2, R, 593]), pred [2][R][2] -> (mv int16[593, 2] of the winner in its list, cost
    [593] Python ints, direction [593], searched list [593], refs [593] pairs)"""
    out_mv = np.zeros((593, 2), np.int16)
    out_cost, out_dir, out_bl, out_refs = [0] * 593, [0] * 593, [0] * 593, [None] * 593
    for s in range(593):
        d, bl, best, m, refs = slot_decide(mv_uni[:, :, s], cost_uni[:, :, s], mv_bi[:, :, s], cost_bi[:, :, s], pred, bits, lambda_q16)
        out_cost[s], out_dir[s], out_bl[s], out_refs[s] = best, d, bl, refs
        out_mv[s] = m
    return out_mv, out_cost, out_dir, out_bl, out_refs


def select_dirs_refs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, pic_w, pic_h, bits, ctu_first=0, pred=None, lambda_q16=LAMBDA_Q16):
    """tables int16[2, R, count, 593, 2] / uint32[2, R, count, 593] of the CTUs [ctu_first, ctu_first + count) of one picture, uni_field
    int16[2, n_ctu, 64, 2], uni_ref uint8[2, n_ctu, 64], pred int16[2, R, n_ctu, 2] or None -> (field [2, count, 64, 2], ref uint8[2, count,
    64], dir uint8[count, 64], slot [count, 64], cost uint32[count])"""
    assert sel.mv_per_ctu == 64 and sel.mv_unit == 0 and sel.price_mv == 0
    R, count = mv_uni.shape[1], mv_uni.shape[2]
    ctus_x = (pic_w + 63) // 64
    field = np.zeros((2, count, 64, 2), np.int16)
    ref = np.full((2, count, 64), NO_REF, np.uint8)
    dirs = np.full((count, 64), NO_DIR, np.uint8)
    slots, costs = [], []
    for k in range(count):
        ctu = ctu_first + k
        p = [[(0, 0)] * R, [(0, 0)] * R] if pred is None else [[pred[l][r][ctu] for r in range(R)] for l in range(2)]
        m_mv, m_cost, m_dir, m_bl, m_refs = merge_ctu(mv_uni[:, :, k], cost_uni[:, :, k], mv_bi[:, :, k], cost_bi[:, :, k], p, bits, lambda_q16)
        f, s, c, _ = sm.select_ctu(m_mv, m_cost, sel, (ctu % ctus_x) * 64, (ctu // ctus_x) * 64, pic_w, pic_h)
        for b, v in enumerate(s.tolist()):
            if v == sm.NO_SLOT:
                continue                                   # (0,0), 0xFF and 0xFF
            d, bl = m_dir[v], m_bl[v]
            dirs[k, b] = d
            if d == 3:
                field[bl, k, b] = f[b]
                ref[bl, k, b] = m_refs[v][bl]
                field[1 - bl, k, b] = uni_field[1 - bl, ctu, b]   # the block's own entries: the motion the bi cost was measured with
                ref[1 - bl, k, b] = uni_ref[1 - bl, ctu, b]
            else:
                field[d - 1, k, b] = f[b]
                ref[d - 1, k, b] = m_refs[v][d - 1]
        slots.append(s); costs.append(c)
    return field, ref, dirs, np.stack(slots), np.array(costs, np.uint32)


# ---- hand-made tables: one slot, and the ties of rules 1-4 (tests/test_select_dirs_refs_cpu.py on the model, tests/test_gpu_select_dirs_refs.py on the device) ----
NO_BI = 0xFFFFFFFF
Z = (0, 0)                                                 # mvb((0,0), (0,0)) = 2 bits: gc 2 at lambda 1 per bit
TIE_MVS = ((4, 0), (0, 4), (-4, 0), (0, -4))               # MVs of equal bit count (8 against the zero predictor), told apart in the field
TIE_MASK = 0b110                                           # list 1's reference 0 -- its cheapest in every scenario -- is not allowed for direction 2
TIE_LAMBDA_Q16 = 1 << 16                                   # 1 per bit: gc(a + b) = gc(a) + gc(b)
FAR = 1 << 22                                              # the priced cost of everything that must not win


def slot_of_lists(mu, cu, mb, cb, bits, lq=1 << 16, pred=None):
    """slot_decide on lists of per-reference (mv, cost) with the zero predictor"""
    R = max(len(mu[0]), len(mu[1]))
    pad = lambda a, fill: [list(a[l]) + [fill] * (R - len(a[l])) for l in range(2)]
    p = [[(0, 0)] * R, [(0, 0)] * R] if pred is None else pred
    return slot_decide(pad(mu, (0, 0)), pad(cu, 0), pad(mb, (0, 0)), pad(cb, 0), p, bits, lq)


def tie_bits(mask):
    """the bit counts the tie scenarios are run with, on the model and on the device: HM-like and all zero"""
    return [hm_bits(3, 3, mask), Bits((0, 0, 0), (3, 3), ([0] * 3, [0] * 3), mask)]


def tie_scenarios():
    """name -> (mask, C[0], C[1], C_B[0], C_B[1], (direction, searched list of the bi candidate, reference of the winner in its list)): the
    PRICED costs of three references per list -- what rules 1 and 3 compare, whatever the bit counts -- and what the rule in include/hmme.h
    makes of them (for directions 1 and 2 the searched list is not part of the statement).  tie_mv gives every candidate its MV"""
    M, far = TIE_MASK, [FAR] * 3
    l1 = [4000, FAR, FAR]                                  # list 1's cheapest is reference 0: outside the mask, it never wins direction 2
    return {
        # rule 1: the first of equal uni costs, a strictly cheaper later one
        "uni tie, the first wins":                  (M, [5000, 5000, 5000], l1, far, far, (1, 0, 0)),
        "a later uni reference strictly cheaper":   (M, [5000, 4999, 4999], l1, far, far, (1, 0, 1)),
        # rule 2: the same among the references of the mask
        "masked uni tie, the first wins":           (M, far, [4000, 5000, 5000], far, far, (2, 0, 1)),
        "a later masked reference strictly cheaper": (M, far, [4000, 5000, 4999], far, far, (2, 0, 2)),
        # rule 4, second part: list 0 wins a tie against the masked list-1 candidate
        "masked list 1 equals list 0":              (M, [5000, 6000, 6000], [4000, 5000, 6000], far, far, (1, 0, 0)),
        "masked list 1 strictly cheaper":           (M, [5000, 6000, 6000], [4000, 6000, 4999], far, far, (2, 0, 2)),
        # rule 3: the first of equal bi costs per list; list 0's unless list 1's is strictly cheaper
        "bi tie in list 0, the first wins":         (M, far, l1, [5000, 5000, 5000], [6000, 6000, 6000], (3, 0, 0)),
        "a later bi reference of list 0 strictly cheaper": (M, far, l1, [5000, 4999, 4999], [6000, 6000, 6000], (3, 0, 1)),
        "bi tie in list 1, the first wins":         (M, far, l1, [6000, 6000, 6000], [5000, 5000, 5000], (3, 1, 0)),
        "a later bi reference of list 1 strictly cheaper": (M, far, l1, [6000, 6000, 6000], [5000, 5000, 4999], (3, 1, 2)),
        "list 1's bi equals list 0's":              (M, far, l1, [5000, 5500, 5500], [5500, 5000, 5500], (3, 0, 0)),
        "list 1's bi strictly cheaper":             (M, far, l1, [5000, 5500, 5500], [5500, 4999, 5500], (3, 1, 1)),
        # rule 4, first part: bi wins ties against both lists
        "bi equals both uni":                       (M, [5000, 6000, 6000], [4000, 5000, 6000], [5500, 5000, 5500], far, (3, 0, 1)),
        "bi equals list 0, list 1 one below":       (M, [5000, 6000, 6000], [4000, 6000, 4999], [5000, 5500, 5500], far, (2, 0, 2)),
        "bi equals list 1, list 0 one below":       (M, [6000, 4999, 6000], [4000, 5000, 6000], [5000, 5500, 5500], far, (1, 0, 1)),
        "bi equals list 0, whose winner is its last reference": (M, [6000, 6000, 5000], l1, [5000, 5500, 5500], far, (3, 0, 0)),   # priced with mot[1], not mot[0]
        "bi one above both uni":                   (M, [5000, 6000, 6000], [4000, 5000, 6000], far, [5500, 5500, 5001], (1, 0, 0)),
        # an empty mask: direction 2 never wins, and bi is compared with list 0 alone
        "empty mask, list 1 far cheaper":           (0, [5000, 5000, 6000], [100, 200, 300], far, far, (1, 0, 0)),
        "empty mask, bi equals list 0":             (0, [6000, 5000, 6000], [100, 200, 300], far, [5500, 5000, 5000], (3, 1, 1)),
        "empty mask, bi one above list 0":          (0, [6000, 5000, 5000], [100, 200, 300], [5001, 5001, 5500], far, (1, 0, 1)),
    }


def tie_mv(bi, l, r):
    """the MV of reference r of list l in the uni (bi = 0) or bi set: the three references of a set carry three different MVs of one bit
    count, and a list's bi set another rotation of them than its uni set"""
    return TIE_MVS[(r + 2 * bi + l) % 4]


def tie_slot_tables(c, c1, cb0, cb1, bits, lambda_q16=TIE_LAMBDA_Q16):
    """the table entries (mu, cu, mb, cb as slot_decide takes them, zero predictor) whose priced costs under `bits` are the given ones: the
    bit prices rule 1 and rule 3 add are taken off again, the bi distortion doubled -- mot[] of the unrestricted uni winners included"""
    gc, mvb = dm.gc, dm.mvb
    cs, cbs = (c, c1), (cb0, cb1)
    mu = [[tie_mv(0, l, r) for r in range(3)] for l in range(2)]
    mb = [[tie_mv(1, l, r) for r in range(3)] for l in range(2)]
    cu, cb, mot = [[0] * 3, [0] * 3], [[0] * 3, [0] * 3], [0, 0]
    for l in range(2):
        for r in range(3):
            bu = mvb(mu[l][r], Z)
            cu[l][r] = cs[l][r] - gc(lambda_q16, bits.dir_bits[l] + bits.ref_bits[l][r] + bu) + gc(lambda_q16, bu)
        ru = cs[l].index(min(cs[l]))                       # the first strict minimum
        mot[l] = bits.ref_bits[l][ru] + mvb(mu[l][ru], Z)
    for l in range(2):
        for r in range(3):
            bb = mvb(mb[l][r], Z)
            cb[l][r] = 2 * (cbs[l][r] - gc(lambda_q16, bits.dir_bits[2] + bits.ref_bits[l][r] + bb + mot[1 - l])) + gc(lambda_q16, bb)
    assert all(gc(lambda_q16, 16) <= v <= NO_BI for l in range(2) for v in cu[l] + cb[l])
    return mu, cu, mb, cb


def tie_want(bits_mask, scenario):
    """(direction, searched list, the winner's MV, (ref index list 0, list 1) as slot_decide states them) of a scenario"""
    mask, _, _, _, _, (d, bl, r) = scenario
    assert mask == bits_mask
    refs = [NO_REF, NO_REF]
    l = bl if d == 3 else d - 1
    refs[l] = r
    return d, bl, tie_mv(int(d == 3), l, r), tuple(refs)


def tie_sites():
    """[(slot, depth)]: the 2Nx2N slots of CUs that tile a 64x64 CTU at three depths -- one 32x32 CU, eight 16x16 CUs (two quadrants) and
    sixteen 8x8 CUs (one quadrant) -- for a scenario each; every other slot of the CTU is priced at FAR, so that the partition decision
    codes exactly these CUs and every scenario stays visible in the field"""
    from hmme import api
    cus = [(1, 0, 0)] + [(2, 32 + 16 * i, 16 * j) for j in range(2) for i in range(2)] + [(2, 32 + 16 * i, 32 + 16 * j) for j in range(2) for i in range(2)]
    cus += [(3, 8 * i, 32 + 8 * j) for j in range(4) for i in range(4)]
    return [(api.slot_index(0, d, 0, sm.z_index(x, y)), d) for d, x, y in cus]


def tie_tables(bits, seed=0, lambda_q16=TIE_LAMBDA_Q16):
    """one CTU whose sites (tie_sites) hold the scenarios of bits.l1_valid_mask in turn: the first nine in the 32x32 and the 16x16 CUs, the
    others and -- the sites being more than the scenarios -- the first ones again in 8x8 CUs -> ((mv_uni, cost_uni, mv_bi, cost_bi [2, 3, 1, 593, ...], uni_field [2, 1, 64, 2], uni_ref [2, 1, 64]), {slot: scenario name})"""
    names = [k for k, v in tie_scenarios().items() if v[0] == bits.l1_valid_mask]
    sites = tie_sites()
    mv_uni, mv_bi = np.zeros((2, 3, 1, 593, 2), np.int16), np.zeros((2, 3, 1, 593, 2), np.int16)
    cost_uni, cost_bi = np.zeros((2, 3, 1, 593), np.uint32), np.zeros((2, 3, 1, 593), np.uint32)
    filler = tie_slot_tables([FAR] * 3, [FAR] * 3, [FAR] * 3, [FAR] * 3, bits, lambda_q16)
    placed = {s: names[k % len(names)] for k, (s, d) in enumerate(sites)}   # more sites than scenarios: the first ones come again in 8x8 CUs
    for s in range(593):
        mu, cu, mb, cb = tie_slot_tables(*tie_scenarios()[placed[s]][1:5], bits, lambda_q16) if s in placed else filler
        mv_uni[:, :, 0, s], cost_uni[:, :, 0, s], mv_bi[:, :, 0, s], cost_bi[:, :, 0, s] = mu, cu, mb, cb
    rng = np.random.default_rng(seed + 9)
    uni_field = rng.integers(-300, 301, size=(2, 1, 64, 2)).astype(np.int16)
    uni_ref = rng.integers(0, 3, size=(2, 1, 64)).astype(np.uint8)
    return (mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref), placed


# ---- table recipes -------------------------------------------------------------------------------------------------------------------------
def predictors(R, n_ctu, seed):
    """int16[2, R, n_ctu, 2], drawn independently per list, reference and CTU, no component zero"""
    rng = np.random.default_rng(seed)
    pred = rng.integers(-40, 41, size=(2, R, n_ctu, 2)).astype(np.int16)
    pred[pred == 0] = 7
    return pred


def random_tables(R, n_ctu, count, seed, pred=None, first=0, lambda_q16=LAMBDA_Q16, base=0, bi_gain=150):
    """select_dirs_model.random_dir_tables with a reference dimension: one draw per reference (its own seed, its own predictors), stacked.
    The bi sets' halved distortions lie bi_gain lower (floored at 0), the MV cost on top as before: against the cheapest of several uni
    candidates per list, and with the other list's motion bits to pay, bi would otherwise win next to nothing (tests/test_select_dirs_refs_cpu.py)
    -> (mv_uni, cost_uni, mv_bi, cost_bi [2, R, count, ...], uni_field int16[2, n_ctu, 64, 2], uni_ref uint8[2, n_ctu, 64] in 0..R-1)"""
    per_ref = [dm.random_dir_tables(n_ctu, count, seed + 31 * r, None if pred is None else pred[:, r], first, lambda_q16, base) for r in range(R)]
    tabs = [np.stack([t[k] for t in per_ref], axis=1) for k in range(4)]
    for l in range(2):
        for r in range(R):
            price = dm.mv_cost_table(tabs[2][l, r], None if pred is None else pred[l, r], range(first, first + count), lambda_q16)
            tabs[3][l, r] = (np.maximum(tabs[3][l, r].astype(np.int64) - price - 2 * bi_gain, 0) + price).astype(np.uint32)
    rng = np.random.default_rng(seed + 78)
    uni_ref = rng.integers(0, R, size=(2, n_ctu, 64)).astype(np.uint8)
    return tabs[0], tabs[1], tabs[2], tabs[3], per_ref[0][4], uni_ref
