"""B pictures from one MV per 4x4 block (the "bi4" family of include/hmme.h: hmme_*_bi4*, hmme_select_dirs4_*, hmme_predict_bi4_*,
hmme_predict_chroma_bi4_*) restated from the rule in the header.  The models of the 64 forms -- select_dirs_model, predict_bi_model,
predict_chroma_model, select_model -- called with 4x4 / 2x2 blocks, as predict4_model does for the P-picture family; the one new rule is
HM's isBipredRestriction for the 8x4 / 4x8 PUs of an 8x8 CU.  Plain numpy / Python integers, no GPU: the reference of
tests/test_bi4_cpu.py and tests/test_gpu_bi4.py, with the fields and tables those tests feed."""
import functools

import numpy as np

import predict4_model as p4
import predict_bi_model as pbm
import predict_chroma_model as cm
import select_dirs_model as sdm
import select_model as sm
from frame_helpers import clip_mv, dims

PER = 256
NO_DIR = 0xFF


# ---- the decision ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restricted_slots():
    """the slots of 8x4 / 4x8 PUs: hmme_slot_key gives depth 3 and part_size 1 or 2 (TComDataCU::isBipredRestriction)"""
    from hmme import api
    out = []
    for s in range(593):
        ps, depth, _, _ = api.slot_key(s)
        if depth == 3 and ps in (1, 2):
            out.append(s)
    return frozenset(out)


def decide4(c, c_b, restricted):
    """rule steps 3 and 4 with difference b: a restricted slot forms no bi candidate"""
    if restricted:
        return (1, 0, c[0]) if c[0] <= c[1] else (2, 0, c[1])
    return sdm.decide(c, c_b)


def merge_ctu4(mv_uni, cost_uni, mv_bi, cost_bi, pred, bits, lambda_q16):
    """select_dirs_model.merge_ctu over all 593 slots with the bi restriction"""
    out_mv = np.zeros((593, 2), np.int16)
    out_cost, out_dir, out_bl = [0] * 593, [0] * 593, [0] * 593
    rs = restricted_slots()
    for s in range(593):
        c, c_b = sdm.slot_candidates(mv_uni[:, s], cost_uni[:, s], mv_bi[:, s], cost_bi[:, s], pred, bits, lambda_q16)
        d, bl, best = decide4(c, c_b, s in rs)
        out_cost[s], out_dir[s], out_bl[s] = best, d, bl
        out_mv[s] = mv_bi[bl, s] if d == 3 else mv_uni[d - 1, s]
    return out_mv, out_cost, out_dir, out_bl


def select_dirs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, pic_w, pic_h, bits, ctu_first=0, pred=None, lambda_q16=sdm.LAMBDA_Q16):
    """select_dirs_model.select_dirs_picture on the 256 layout: uni_field int16[2, n_ctu, 256, 2] -> (field [2, count, 256, 2], dir
    uint8[count, 256], slot [count, 256], cost uint32[count], leaves [(depth, part_size)] per CTU)"""
    assert sel.mv_per_ctu == PER and sel.mv_unit == 0 and sel.price_mv == 0
    count = mv_uni.shape[1]
    ctus_x = (pic_w + 63) // 64
    field = np.zeros((2, count, PER, 2), np.int16)
    dirs = np.full((count, PER), NO_DIR, np.uint8)
    slots, costs, leaves = [], [], []
    for k in range(count):
        ctu = ctu_first + k
        p = [(0, 0), (0, 0)] if pred is None else [pred[l][ctu] for l in range(2)]
        m_mv, m_cost, m_dir, m_bl = merge_ctu4(mv_uni[:, k], cost_uni[:, k], mv_bi[:, k], cost_bi[:, k], p, bits, lambda_q16)
        f, s, c, lv = sm.select_ctu(m_mv, m_cost, sel, (ctu % ctus_x) * 64, (ctu // ctus_x) * 64, pic_w, pic_h)
        for b, v in enumerate(s.tolist()):
            if v == sm.NO_SLOT:
                continue
            d, bl = m_dir[v], m_bl[v]
            dirs[k, b] = d
            if d == 3:
                field[bl, k, b] = f[b]
                field[1 - bl, k, b] = uni_field[1 - bl, ctu, b]   # difference c: the 4x4 block's own entry
            else:
                field[d - 1, k, b] = f[b]
        slots.append(s); costs.append(c); leaves.append(lv)
    return field, dirs, np.stack(slots), np.array(costs, np.uint32), leaves


def random_dir_tables4(n_ctu, count, seed, pred=None, first=0, lambda_q16=sdm.LAMBDA_Q16, base=0):
    """select_dirs_model.random_dir_tables with the lists' fields in the 256 layout, every 4x4 entry drawn on its own"""
    mv_uni, cost_uni, mv_bi, cost_bi, _ = sdm.random_dir_tables(n_ctu, count, seed, pred, first, lambda_q16, base)
    rng = np.random.default_rng(seed + 78)
    return mv_uni, cost_uni, mv_bi, cost_bi, rng.integers(-300, 301, size=(2, n_ctu, PER, 2)).astype(np.int16)


def replicate_lists(field64):
    """[2, n, 64, ...] -> [2, n, 256, ...]"""
    return np.stack([p4.replicate(field64[l]) for l in range(2)])


def block_of(field256):
    """[n, 256, ...] -> [n, 64, 4, ...]: the four entries of every 8x8 block, quadrant order"""
    f = np.asarray(field256)
    n = f.shape[0]
    g = f.reshape((n, 8, 2, 8, 2) + f.shape[2:])
    return np.moveaxis(g, 2, 3).reshape((n, 64, 4) + f.shape[2:])


def mixed_blocks(field, dirs):
    """how many 8x8 blocks carry four entries that differ in direction or MV: field int16[2, n, 256, 2], dirs uint8[n, 256]"""
    n = dirs.shape[0]
    key = np.concatenate([block_of(field[0]).astype(np.int32), block_of(field[1]).astype(np.int32), block_of(dirs).astype(np.int32)[..., None]], axis=3)
    return int((key != key[:, :, :1]).any(axis=(2, 3)).sum())


def pus_of(slot_map, dirs):
    """the coded PUs of a decision: {(ctu, slot): direction}"""
    out = {}
    for k in range(slot_map.shape[0]):
        for b in range(PER):
            s = int(slot_map[k, b])
            if s != sm.NO_SLOT:
                out[(k, s)] = int(dirs[k, b])
    return out


# ---- the prediction --------------------------------------------------------------------------------------------------------------------
def live_blocks(w, h, dirs, ctus=None):
    cx_n, cy_n = dims(w, h)
    for ctu in (range(cx_n * cy_n) if ctus is None else ctus):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(PER):
            bx, by = p4.block_xy(b)
            d = int(dirs[ctu, b])
            if cu_x + bx < w and cu_y + by < h and d in (1, 2, 3):
                yield ctu, b, cu_x, cu_y, bx, by, d


def luma_picture(hmo, planes, w, h, bd, field, dirs, out, ctus=None):
    """what hmme_predict_bi4_frame writes into out ([h, w], changed in place and returned): planes = (list 0, list 1) padded planes, field
    int16[2, n_ctu, 256, 2], dirs uint8[n_ctu, 256]: predict_bi_model.pred_block with 4x4 blocks"""
    from hmme import synth
    m = synth.MARGIN
    for ctu, b, cu_x, cu_y, bx, by, d in live_blocks(w, h, dirs, ctus):
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        x, y = cu_x + bx, cu_y + by
        p = pbm.pred_block(planes, m + x, m + y, 4, mvs, d, bd)
        x1, y1 = min(x + 4, w), min(y + 4, h)
        out[y:y1, x:x1] = p[:y1 - y, :x1 - x]
    return out


def chroma_picture(hmo, comps, w, h, bd, field, dirs, outs, ctus=None):
    """what hmme_predict_chroma_bi4_frame writes into outs = (cb, cr): comps[c] = (list 0, list 1) padded planes of component c, w x h the
    LUMA size: predict_chroma_model.pred_block with 2x2 blocks"""
    from hmme import synth
    m = synth.MARGIN
    for ctu, b, cu_x, cu_y, bx, by, d in live_blocks(w, h, dirs, ctus):
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        x, y = (cu_x + bx) // 2, (cu_y + by) // 2
        x1, y1 = min(x + 2, w // 2), min(y + 2, h // 2)
        for c in range(2):
            p = cm.pred_block(comps[c], m + x, m + y, 2, mvs, d, bd)
            outs[c][y:y1, x:x1] = p[:y1 - y, :x1 - x]
    return outs


def origin_prediction(hmo, plane, w, h, bd, field):
    """the other list's prediction P inside a bi4 origin: EVERY 4x4 block of every CTU's 64x64 block, those beyond the picture edge included,
    from `plane` at its own clamped entry (field int16[n_ctu, 256, 2]) -> [cy_n * 64, cx_n * 64]"""
    from hmme import synth
    import range_content as rc
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    out = np.zeros((cy_n * 64, cx_n * 64), np.int64)
    for ctu in range(cx_n * cy_n):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(PER):
            bx, by = p4.block_xy(b)
            qx, qy = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
            out[cu_y + by:cu_y + by + 4, cu_x + bx:cu_x + bx + 4] = rc.pred_qpel(plane, m + cu_x + bx, m + cu_y + by, 4, 4, qx, qy, bd)
    return out


def quadrant_fields(field, dirs):
    """the four 64-entry (field int16[2, n, 64, 2], dirs uint8[n, 64]) whose every 8x8 block carries the entry of its quadrant q"""
    out = []
    for q in range(4):
        f0, d = p4.quadrant_fields(field[0], dirs)[q]
        f1, _ = p4.quadrant_fields(field[1], dirs)[q]
        out.append((np.stack([f0, f1]), d))
    return out


def random_field_bi4(w, h, seed):
    """random (direction, MV0, MV1) per 4x4 block: directions 1, 2, 3 in thirds plus 0xFF and 0 entries, MVs of up to 40 pels with every
    phase; the four blocks nearest the picture's corners are bi with MVs at +-32767 and just beyond the picture in both lists
    -> (field int16[2, n, 256, 2], dirs uint8[n, 256])"""
    f0, _ = p4.random_field4(w, h, 1, seed)
    f1, _ = p4.random_field4(w, h, 1, seed + 1)
    n = f0.shape[0]
    rng = np.random.default_rng(seed + 2)
    dirs = rng.choice(np.array([1, 2, 3] * 4 + [NO_DIR, 0], np.uint8), size=(n, PER))
    far = (np.abs(f0.astype(np.int32)).max(axis=2) > 200) | (np.abs(f1.astype(np.int32)).max(axis=2) > 200)
    dirs[far] = 3
    f1[far] = -f0[far].astype(np.int32).clip(-32767, 32767).astype(np.int16)
    return np.stack([f0, f1]), dirs


def phase_pairs(w, h, field, dirs):
    """per list the set of (px, py) of the live blocks that use it"""
    seen = (set(), set())
    for ctu, b, *_, d in live_blocks(w, h, dirs):
        for l in range(2):
            if d & (1 << l):
                seen[l].add((int(field[l, ctu, b, 0]) & 3, int(field[l, ctu, b, 1]) & 3))
    return seen


def rotation_ctu(seed):
    """one CTU whose 8x8 block (bx, by) carries the quadrant directions (1, 2, 3, dead) rotated by bx + by, dead being 0 in the left and 0xFF in the
    right half, with four distinct MVs per list -> (field int16[2, 1, 256, 2], dirs uint8[1, 256])"""
    rng = np.random.default_rng(seed)
    field = rng.integers(-90, 91, size=(2, 16, 16, 2)).astype(np.int16)
    dirs = np.zeros((16, 16), np.uint8)
    for by in range(8):
        for bx in range(8):
            base = [1, 2, 3, NO_DIR if bx >= 4 else 0]
            for q in range(4):
                dirs[2 * by + (q >> 1), 2 * bx + (q & 1)] = base[(q + bx + by) % 4]
    return field.reshape(2, 1, PER, 2), dirs.reshape(1, PER)


# ---- one B picture end to end ------------------------------------------------------------------------------------------------------------
E2E_SIZE = (128, 64)
E2E_SEED = 4100
TABLE_SEED, TABLE_LAMBDA_Q16 = 1, 16000   # the table recipe: about 0.24 per bit, so that the 4-wide PUs' bit prices do not drown their distortions
E2E_BITS = sdm.HM_BITS


def b_scene(w, h, bd, seed):
    """a current picture between two unrelated references: 4x4 regions drawn from list 0's texture, list 1's or their average, plus noise,
    so that all three directions win somewhere and neighbours differ -> padded (cur, ref0, ref1)"""
    from hmme import synth
    m = synth.MARGIN
    ref0 = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=2)[1]
    ref1 = synth.make_pair(w, h, seed=seed + 31, bit_depth=bd, max_mv=2)[1]
    a, b = ref0[m:m + h, m:m + w].astype(np.int64), ref1[m:m + h, m:m + w].astype(np.int64)
    rng = np.random.default_rng(seed + 62)
    kind = np.kron(rng.integers(0, 3, size=((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), np.int64))[:h, :w]
    cur = np.where(kind == 0, a, np.where(kind == 1, b, (a + b + 1) >> 1)) + rng.integers(-2, 3, size=(h, w))
    return synth.pad_plane(np.clip(cur, 0, (1 << bd) - 1)), ref0, ref1


def e2e_sel(api, depth):
    return api.SelectParams(PER, min_depth=depth, max_depth=depth)


def chain(oracle_lib, hmo, api, cur, refs, w, h, bd, depth, lambda_q16, had=1):
    """the model of every step of the chain on one B picture (integer MVs (0,0), predictors (0,0)): the oracle's refinement of both lists,
    select_model at 256 per list, the oracle's refinement against the origin built by origin_prediction, select_dirs4_picture -> dict"""
    from hmme import synth
    m = synth.MARGIN
    n = n_ctus(w, h)
    sel = e2e_sel(api, depth)
    imv = np.zeros((n, 593, 2), np.int16)
    uni = [oracle_lib.refine_frame(cur, refs[l], (m, m), w, h, imv, None, lambda_q16, had, bd, n_threads=4) for l in range(2)]
    uni_sel = [sm.select_picture(uni[l][0], uni[l][1], sel, w, h) for l in range(2)]
    uni_field = np.stack([uni_sel[l][0] for l in range(2)])
    bi = []
    for l in range(2):
        p = origin_prediction(hmo, refs[1 - l], w, h, bd, uni_field[1 - l])
        cy, cx = p.shape
        org = (2 * cur[m:m + cy, m:m + cx].astype(np.int64) - p).astype(np.int16)
        bi.append(oracle_lib.refine_frame(np.ascontiguousarray(np.pad(org, m)), refs[l], (m, m), w, h, imv, None, lambda_q16, had, bd, n_threads=4))
    mv_uni, cost_uni = np.stack([u[0] for u in uni]), np.stack([u[1] for u in uni])
    mv_bi, cost_bi = np.stack([u[0] for u in bi]), np.stack([u[1] for u in bi])
    field, dirs, slot, cost, leaves = select_dirs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, w, h, E2E_BITS, lambda_q16=lambda_q16)
    return dict(mv_uni=mv_uni, cost_uni=cost_uni, mv_bi=mv_bi, cost_bi=cost_bi, uni_field=uni_field, uni_slot=[u[1] for u in uni_sel], field=field, dirs=dirs,
                slot=slot, cost=cost, leaves=leaves)


def n_ctus(w, h):
    return sdm.n_ctus(w, h)


def coverage(depth, slot, dirs, field, leaves):
    """what the end-to-end picture must show -> a dict the tests assert on: at depth 3 the PartSizes of the 8x8 CUs and the directions of
    their 8x4 / 4x8 PUs; at depth 2 per AMP PartSize the number of direction-3 PUs; the number of mixed 8x8 blocks"""
    from hmme import api
    pus = pus_of(slot, dirs)
    by_ps = {}
    for (k, s), d in pus.items():
        ps, dep, _, _ = api.slot_key(s)
        assert dep == depth
        by_ps.setdefault(ps, []).append(d)
    return dict(sizes={ps for lv in leaves for _, ps in lv}, dirs_by_ps=by_ps, mixed=mixed_blocks(field, dirs))
