"""The reference picture per PU of hmme_select_refs_device restated from the rule in include/hmme.h ("the reference picture per PU, and the
prediction from it"): per slot the reference with the smallest priced cost in Python integers, then select_model.select_ctu -- the partition
rule -- on the merged slots with the MV cost switched off.  Written from the header text, not from the kernel: the reference of
tests/test_gpu_select_refs.py, and the table recipes those tests feed."""
import functools

import numpy as np

import select_model as sm

NO_REF = 0xFF


def merge_ctu(mv, cost, sel, ref_cost, pred, lambda_q16, mv_cost):
    """mv int16[n_refs, 593, 2], cost uint32[n_refs, 593] of one CTU, pred [n_refs][2] -> (mv int16[593, 2], priced cost [593] Python ints,
    ref [593]): rule steps 1 and 2"""
    n_refs = mv.shape[0]
    out_mv = np.zeros((593, 2), np.int16)
    out_cost, out_ref = [0] * 593, [0] * 593
    for s in range(593):
        best = None
        for r in range(n_refs):
            p = int(cost[r, s]) + int(ref_cost[r])
            if sel.price_mv:
                p += int(mv_cost(int(lambda_q16), int(mv[r, s, 0]), int(mv[r, s, 1]), int(pred[r][0]), int(pred[r][1]), 2 if sel.mv_unit else 0))
            if best is None or p < best[0]:               # strict: the lowest index wins ties
                best = (p, r)
        out_cost[s], out_ref[s] = best
        out_mv[s] = mv[best[1], s]
    return out_mv, out_cost, out_ref


def select_refs_picture(mv, cost, sel, pic_w, pic_h, ref_cost=None, ctu_first=0, pred=None, lambda_q16=0, mv_cost=None):
    """tables int16[n_refs, count, 593, 2] / uint32[n_refs, count, 593] of the CTUs [ctu_first, ctu_first + count) of one picture, pred
    int16[n_refs, n_ctu, 2] or None -> (field [count, per, 2], ref uint8[count, per], slot [count, per], cost uint32[count], leaves)"""
    n_refs, count = mv.shape[0], mv.shape[1]
    ref_cost = [0] * n_refs if ref_cost is None else ref_cost
    ctus_x = (pic_w + 63) // 64
    # step 3: the MV cost is inside the merged cost already
    plain = type(sel)(sel.mv_per_ctu, sel.mv_unit, 0, sel.part_mask, sel.min_depth, sel.max_depth, sel.cu_cost, sel.pu_cost)
    fields, refs, slots, costs, leaves = [], [], [], [], []
    for k in range(count):
        ctu = ctu_first + k
        p = [(0, 0)] * n_refs if pred is None else [pred[r][ctu] for r in range(n_refs)]
        m_mv, m_cost, m_ref = merge_ctu(mv[:, k], cost[:, k], sel, ref_cost, p, lambda_q16, mv_cost)
        f, s, c, lv = sm.select_ctu(m_mv, m_cost, plain, (ctu % ctus_x) * 64, (ctu // ctus_x) * 64, pic_w, pic_h)
        r = np.array([NO_REF if v == sm.NO_SLOT else m_ref[v] for v in s.tolist()], np.uint8)
        fields.append(f); refs.append(r); slots.append(s); costs.append(c); leaves += lv
    return np.stack(fields), np.stack(refs), np.stack(slots), np.array(costs, np.uint32), leaves


def random_ref_tables(n_refs, n_ctu, seed, noise=2):
    """the recipe of the GPU tests: select_model.random_tables with a different seed per reference -> (mv [n_refs, n_ctu, 593, 2],
    cost [n_refs, n_ctu, 593])"""
    tabs = [sm.random_tables(n_ctu, seed=seed + 1000 * r, noise=noise) for r in range(n_refs)]
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])


def ref_predictors(n_refs, n_ctu, seed):
    """predictors drawn independently per reference and CTU: int16[n_refs, n_ctu, 2], no component zero"""
    rng = np.random.default_rng(seed)
    pred = rng.integers(-40, 41, size=(n_refs, n_ctu, 2)).astype(np.int16)
    pred[pred == 0] = 7
    return pred


# ---- the recipes of the parametrised GPU cases, shared with the CPU test that shows they exercise the reference choice ------------------
LAMBDA_Q16 = 500000                                        # lambda about 58: an MV or reference-index bit costs 7.6
CASE_SIZE = {1: (64, 64), 2: (100, 70), 4: (136, 72), 16: (136, 72)}   # 1, 2x2 and 3x2 CTUs, the last two with partial right / bottom CTUs


def hm_ref_idx_bits(n_refs, ref_idx):
    """TEncSearch.cpp:3030-3037, literally: iRefIdx + 1, one less for the last index, 0 in a list of one"""
    bits = ref_idx + 1
    if ref_idx == n_refs - 1:
        bits -= 1
    if n_refs == 1:
        bits = 0
    return bits


def hm_ref_cost(n_refs, lambda_q16=LAMBDA_Q16):
    """what the header tells a caller who wants HM's price to pass"""
    return [(lambda_q16 * hm_ref_idx_bits(n_refs, r)) >> 16 for r in range(n_refs)]


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


@functools.lru_cache(maxsize=None)
def case(n_refs, price):
    """(w, h, mv, cost, pred, ref_cost, min_depth) of the parametrised case with n_refs references: tables with a different seed per
    reference (the wider noise with the MV cost, as tests/test_gpu_select.py has it), predictors distinct per reference, HM's
    reference-index price.  With 16 references the six CTUs hold about 30 CUs when the decision is free -- too few for every reference to
    win one -- and at 7.6 per bit several of the higher indices win no block at the recipe's costs: there CUs are 16x16 at most
    (min_depth 2) and an index bit costs 1.  tests/test_select_refs_cpu.py shows on the model that every case exercises the choice.  Drawn once and shared:
    read-only"""
    w, h = CASE_SIZE[n_refs]
    n = n_ctus(w, h)
    mv, cost = random_ref_tables(n_refs, n, seed=300 + n_refs, noise=64 if price else 2)
    pred = ref_predictors(n_refs, n, seed=400 + n_refs)
    for a in (mv, cost, pred):
        a.setflags(write=False)
    if n_refs == 16:
        return w, h, mv, cost, pred, hm_ref_cost(n_refs, 1 << 16), 2
    return w, h, mv, cost, pred, hm_ref_cost(n_refs), 0
