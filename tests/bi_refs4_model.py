"""B pictures with several references per list from one MV per 4x4 block (the "bi_refs4" family of include/hmme.h: hmme_*_frame_bi_refs4*,
hmme_select_dirs_refs4_*, hmme_predict_bi_refs4_*, hmme_predict_chroma_bi_refs4_*) restated from the rule in the header.  Composed from the
models that exist: predict_bi_model / predict_chroma_model blocks as predict_bi_refs_model and predict_chroma_bi_refs_model call them, but
4x4 / 2x2; select_dirs_refs_model's candidates with bi4_model's isBipredRestriction; predict4_model for the two layouts.  Plain numpy /
Python integers, no GPU: the reference of tests/test_bi_refs4_cpu.py and tests/test_gpu_bi_refs4.py, with the fields and tables they feed."""
import numpy as np

import bi4_model as b4
import predict4_model as p4
import predict_bi_model as pbm
import predict_chroma_model as pcm
import select_dirs_model as dm
import select_dirs_refs_model as drm
import select_model as sm
from frame_helpers import clip_mv, dims

PER = 256
NO_REF, NO_DIR = 0xFF, 0xFF


# ---- the two layouts -----------------------------------------------------------------------------------------------------------------------
def replicate3(field64, dirs64, refs64):
    """(int16[2, n, 64, 2], uint8[n, 64], uint8[2, n, 64]) -> the 256 layout: every 4x4 block carries its 8x8 block's entry"""
    return b4.replicate_lists(field64), p4.replicate(dirs64), b4.replicate_lists(refs64)


def quadrant_fields(field, dirs, refs):
    """the four 64-entry (field int16[2, n, 64, 2], dirs uint8[n, 64], refs uint8[2, n, 64]) whose every 8x8 block carries the entry of its
    quadrant q"""
    out = []
    for q in range(4):
        f0, d = p4.quadrant_fields(field[0], dirs)[q]
        f1, r0 = p4.quadrant_fields(field[1], refs[0])[q]
        _, r1 = p4.quadrant_fields(field[1], refs[1])[q]
        out.append((np.stack([f0, f1]), d, np.stack([r0, r1])))
    return out


def distinct_quadrant_blocks(dirs, refs):
    """how many 8x8 blocks name four different (direction, ref0, ref1) in their four quadrants"""
    key = b4.block_of(dirs).astype(np.int32) * 65536 + b4.block_of(refs[0]).astype(np.int32) * 256 + b4.block_of(refs[1]).astype(np.int32)
    return int(sum(len(set(blk.tolist())) == 4 for ctu in key for blk in ctu))


# ---- the prediction ------------------------------------------------------------------------------------------------------------------------
def live_blocks(w, h, dirs, refs, n0, n1, ctus=None):
    """(ctu, b, luma CTU origin, block origin inside the CTU, direction, (index 0, index 1)) of every live 4x4 block: it starts inside the
    w x h luma picture, its direction is 1, 2 or 3, and every list it uses has an index below that list's count"""
    n = (n0, n1)
    for ctu, b, cu_x, cu_y, bx, by, d in b4.live_blocks(w, h, dirs, ctus):
        idx = (int(refs[0, ctu, b]), int(refs[1, ctu, b]))
        if any((d >> l) & 1 and idx[l] >= n[l] for l in range(2)):
            continue
        yield ctu, b, cu_x, cu_y, bx, by, d, idx


def luma_picture(hmo, planes0, planes1, w, h, bd, field, dirs, refs, out, ctus=None):
    """what hmme_predict_bi_refs4_frame writes into out ([h, w], changed in place and returned): planes_l the padded pictures of list l, field
    int16[2, n_ctu, 256, 2], dirs uint8[n_ctu, 256], refs uint8[2, n_ctu, 256]: predict_bi_refs_model's block with 4x4 blocks"""
    from hmme import synth
    m = synth.MARGIN
    lists = (planes0, planes1)
    for ctu, b, cu_x, cu_y, bx, by, d, idx in live_blocks(w, h, dirs, refs, len(planes0), len(planes1), ctus):
        two = [lists[l][idx[l]] if (d >> l) & 1 else None for l in range(2)]   # a list the direction does not name is not looked at
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        x, y = cu_x + bx, cu_y + by
        p = pbm.pred_block(two, m + x, m + y, 4, mvs, d, bd)
        x1, y1 = min(x + 4, w), min(y + 4, h)
        out[y:y1, x:x1] = p[:y1 - y, :x1 - x]
    return out


def chroma_picture(hmo, comps, w, h, bd, field, dirs, refs, outs, ctus=None):
    """what hmme_predict_chroma_bi_refs4_frame writes into outs = (cb, cr): comps[c][l][r] = the padded plane of component c of list l's
    reference r, w x h the LUMA size: predict_chroma_bi_refs_model's block with 2x2 blocks, no weights"""
    from hmme import synth
    m = synth.MARGIN
    n0, n1 = len(comps[0][0]), len(comps[0][1])
    for ctu, b, cu_x, cu_y, bx, by, d, idx in live_blocks(w, h, dirs, refs, n0, n1, ctus):
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        x, y = (cu_x + bx) // 2, (cu_y + by) // 2
        x1, y1 = min(x + 2, w // 2), min(y + 2, h // 2)
        for c in range(2):
            two = [comps[c][l][idx[l]] if (d >> l) & 1 else None for l in range(2)]
            p = pcm.pred_block(two, m + x, m + y, 2, mvs, d, bd)
            outs[c][y:y1, x:x1] = p[:y1 - y, :x1 - x]
    return outs


def origin_prediction(hmo, others, w, h, bd, field, ref_field):
    """the other list's prediction P inside a bi_refs4 origin: EVERY 4x4 block of every CTU's 64x64 block, those beyond the picture edge
    included, from others[its index] -- others[0] where the index is >= len(others) -- at its own clamped entry (field int16[n_ctu, 256, 2],
    ref_field uint8[n_ctu, 256]) -> [cy_n * 64, cx_n * 64]"""
    from hmme import synth
    import range_content as rc
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    out = np.zeros((cy_n * 64, cx_n * 64), np.int64)
    for ctu in range(cx_n * cy_n):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(PER):
            bx, by = p4.block_xy(b)
            idx = int(ref_field[ctu, b])
            plane = others[idx if idx < len(others) else 0]
            qx, qy = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
            out[cu_y + by:cu_y + by + 4, cu_x + bx:cu_x + bx + 4] = rc.pred_qpel(plane, m + cu_x + bx, m + cu_y + by, 4, 4, qx, qy, bd)
    return out


def origin4(hmo, cur, others, w, h, bd, field, ref_field):
    """the origin O = 2 * cur - P over the CTU blocks, int16 [cy_n * 64, cx_n * 64]"""
    from hmme import synth
    m = synth.MARGIN
    p = origin_prediction(hmo, others, w, h, bd, field, ref_field)
    return np.ascontiguousarray((2 * cur[m:m + p.shape[0], m:m + p.shape[1]].astype(np.int64) - p).astype(np.int16))


def random_field_bi_refs4(w, h, n0, n1, seed):
    """bi4_model.random_field_bi4 with a reference index per block and list: indices 0 .. n - 1 three times as likely as 0xFF and n itself;
    the +-32767 blocks at the picture's corners are bi and name reference n - 1 of both lists -> (field int16[2, n, 256, 2], dirs uint8[n,
    256], refs uint8[2, n, 256])"""
    field, dirs = b4.random_field_bi4(w, h, seed)
    rng = np.random.default_rng(seed + 5)
    refs = np.stack([rng.choice(np.array(list(range(k)) * 3 + [NO_REF, k], np.uint8), size=dirs.shape) for k in (n0, n1)])
    far = np.abs(field.astype(np.int32)).max(axis=(0, 3)) > 200
    refs[0][far], refs[1][far] = n0 - 1, n1 - 1
    return field, dirs, refs


def field_coverage(w, h, field, dirs, refs, n0, n1):
    """what a test field shows -> dict: the directions, the live indices per list, whether an index >= n occurs in a used list (the block is
    not live) and in an unused list of a live block, the 8x8 blocks with four different quadrants, the phase pairs of the live blocks per
    list, whether a live bi block carries +-32767"""
    n = (n0, n1)
    inside = [(c, b, d) for c, b, *_, d in b4.live_blocks(w, h, dirs)]   # a direction and a start inside the picture
    live = {(c, b): (d, idx) for c, b, *_, d, idx in live_blocks(w, h, dirs, refs, n0, n1)}
    phases = (set(), set())
    for (c, b), (d, idx) in live.items():
        for l in range(2):
            if (d >> l) & 1:
                phases[l].add((int(field[l, c, b, 0]) & 3, int(field[l, c, b, 1]) & 3))
    return dict(
        dirs=set(dirs.reshape(-1).tolist()),
        live_refs=tuple({idx[l] for d, idx in live.values() if (d >> l) & 1} for l in range(2)),
        dead_by_used_index=any((c, b) not in live for c, b, d in inside),
        live_with_unused_index_beyond=any(not (d >> l) & 1 and idx[l] >= n[l] for d, idx in live.values() for l in range(2)),
        distinct_blocks=distinct_quadrant_blocks(dirs, refs),
        phases=phases,
        far_bi=any(d == 3 and max(abs(int(v)) for v in field[:, c, b].reshape(-1)) >= 32767 for (c, b), (d, idx) in live.items()))


# ---- the decision --------------------------------------------------------------------------------------------------------------------------
def slot_decide4(mu, cu, mb, cb, pred, bits, lambda_q16, restricted):
    """select_dirs_refs_model.slot_decide with difference b: a restricted slot (an 8x4 / 4x8 PU) forms no bi candidate for any reference --
    rule steps 1 and 2 alone, then: C_V absent or C[0] <= C_V gives direction 1, otherwise direction 2"""
    if not restricted:
        return drm.slot_decide(mu, cu, mb, cb, pred, bits, lambda_q16)
    gc, mvb = dm.gc, dm.mvb
    c, ru, c_v, rv = [None, None], [0, 0], None, None
    for l in range(2):
        for r in range(bits.n_refs[l]):
            bu = mvb(mu[l][r], pred[l][r])
            p = max(0, int(cu[l][r]) - gc(lambda_q16, bu)) + gc(lambda_q16, bits.dir_bits[l] + bits.ref_bits[l][r] + bu)
            if c[l] is None or p < c[l]:
                c[l], ru[l] = p, r
            if l == 1 and (bits.l1_valid_mask >> r) & 1 and (c_v is None or p < c_v):
                c_v, rv = p, r
    if c_v is None or c[0] <= c_v:
        return 1, 0, c[0], mu[0][ru[0]], (ru[0], NO_REF)
    return 2, 0, c_v, mu[1][rv], (NO_REF, rv)


def merge_ctu4(mv_uni, cost_uni, mv_bi, cost_bi, pred, bits, lambda_q16):
    """select_dirs_refs_model.merge_ctu over all 593 slots with the bi restriction"""
    out_mv = np.zeros((593, 2), np.int16)
    out_cost, out_dir, out_bl, out_refs = [0] * 593, [0] * 593, [0] * 593, [None] * 593
    rs = b4.restricted_slots()
    for s in range(593):
        d, bl, best, m, refs = slot_decide4(mv_uni[:, :, s], cost_uni[:, :, s], mv_bi[:, :, s], cost_bi[:, :, s], pred, bits, lambda_q16, s in rs)
        out_cost[s], out_dir[s], out_bl[s], out_refs[s] = best, d, bl, refs
        out_mv[s] = m
    return out_mv, out_cost, out_dir, out_bl, out_refs


def select_dirs_refs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, pic_w, pic_h, bits, ctu_first=0, pred=None, lambda_q16=drm.LAMBDA_Q16):
    """select_dirs_refs_model.select_dirs_refs_picture on the 256 layout: tables [2, R, count, 593, ...], uni_field int16[2, n_ctu, 256, 2],
    uni_ref uint8[2, n_ctu, 256] -> (field [2, count, 256, 2], ref uint8[2, count, 256], dir uint8[count, 256], slot [count, 256], cost
    uint32[count])"""
    assert sel.mv_per_ctu == PER and sel.mv_unit == 0 and sel.price_mv == 0
    R, count = mv_uni.shape[1], mv_uni.shape[2]
    ctus_x = (pic_w + 63) // 64
    field = np.zeros((2, count, PER, 2), np.int16)
    ref = np.full((2, count, PER), NO_REF, np.uint8)
    dirs = np.full((count, PER), NO_DIR, np.uint8)
    slots, costs = [], []
    for k in range(count):
        ctu = ctu_first + k
        p = [[(0, 0)] * R, [(0, 0)] * R] if pred is None else [[pred[l][r][ctu] for r in range(R)] for l in range(2)]
        m_mv, m_cost, m_dir, m_bl, m_refs = merge_ctu4(mv_uni[:, :, k], cost_uni[:, :, k], mv_bi[:, :, k], cost_bi[:, :, k], p, bits, lambda_q16)
        f, s, c, _ = sm.select_ctu(m_mv, m_cost, sel, (ctu % ctus_x) * 64, (ctu // ctus_x) * 64, pic_w, pic_h)
        for b, v in enumerate(s.tolist()):
            if v == sm.NO_SLOT:
                continue
            d, bl = m_dir[v], m_bl[v]
            dirs[k, b] = d
            if d == 3:
                field[bl, k, b] = f[b]
                ref[bl, k, b] = m_refs[v][bl]
                field[1 - bl, k, b] = uni_field[1 - bl, ctu, b]   # difference c: the 4x4 block's own entries
                ref[1 - bl, k, b] = uni_ref[1 - bl, ctu, b]
            else:
                field[d - 1, k, b] = f[b]
                ref[d - 1, k, b] = m_refs[v][d - 1]
        slots.append(s); costs.append(c)
    return field, ref, dirs, np.stack(slots), np.array(costs, np.uint32)


def random_tables4(R, n_ctu, count, seed, pred=None, first=0, lambda_q16=drm.LAMBDA_Q16, base=0):
    """select_dirs_refs_model.random_tables with the lists' fields and reference indices in the 256 layout, every 4x4 entry drawn on its own"""
    mv_uni, cost_uni, mv_bi, cost_bi, _, _ = drm.random_tables(R, n_ctu, count, seed, pred, first, lambda_q16, base)
    rng = np.random.default_rng(seed + 79)
    uni_field = rng.integers(-300, 301, size=(2, n_ctu, PER, 2)).astype(np.int16)
    uni_ref = rng.integers(0, R, size=(2, n_ctu, PER)).astype(np.uint8)
    return mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref


def tie_tables4(bits, seed=0, lambda_q16=drm.TIE_LAMBDA_Q16):
    """select_dirs_refs_model.tie_tables through the 4 form, two CTUs (a 128 x 64 picture).  CTU 0 is its CTU: the scenarios on 2Nx2N slots
    at three depths, all above 256.  CTU 1 holds them on slots below 256: the sixteen 8x8 CUs of its lower left quadrant carry two scenarios
    each on their two 2NxN (even rows) or Nx2N (odd rows) PUs.  A restricted slot decides between its uni candidates, which the bi scenarios
    price at FAR, so these CUs' other shapes cost four times that: with 8x8 CUs forced (min_depth = max_depth = 3) the pair that carries
    the scenarios is the one coded -> ((mv_uni, cost_uni, mv_bi, cost_bi [2, 3, 2, 593, ...], uni_field [2, 2, 256, 2], uni_ref [2, 2,
    256]), {(ctu, slot): scenario name})"""
    from hmme import api
    (mv_uni, cost_uni, mv_bi, cost_bi, _, _), placed0 = drm.tie_tables(bits, seed, lambda_q16)
    tabs = [np.concatenate([t, t], axis=2) for t in (mv_uni, cost_uni, mv_bi, cost_bi)]
    names = [k for k, v in drm.tie_scenarios().items() if v[0] == bits.l1_valid_mask]
    filler = drm.tie_slot_tables([drm.FAR] * 3, [drm.FAR] * 3, [drm.FAR] * 3, [drm.FAR] * 3, bits, lambda_q16)
    heavy = drm.tie_slot_tables([4 * drm.FAR] * 3, [4 * drm.FAR] * 3, [4 * drm.FAR] * 3, [4 * drm.FAR] * 3, bits, lambda_q16)
    placed = {(0, s): name for s, name in placed0.items()}

    def put(s, entry):
        for t, v in zip(tabs, entry):
            t[:, :, 1, s] = v

    for s in range(593):
        put(s, filler)
    k = 0
    for j in range(4):
        for i in range(4):
            z = sm.z_index(8 * i, 32 + 8 * j)
            for s in [api.slot_index(0, 3, 0, z)] + [api.slot_index(2 - (j & 1), 3, part, z) for part in range(2)]:
                put(s, heavy)
            for part in range(2):
                s = api.slot_index(1 + (j & 1), 3, part, z)
                placed[(1, s)] = names[k % len(names)]
                put(s, drm.tie_slot_tables(*drm.tie_scenarios()[names[k % len(names)]][1:5], bits, lambda_q16))
                k += 1
    rng = np.random.default_rng(seed + 9)
    uni_field = rng.integers(-300, 301, size=(2, 2, PER, 2)).astype(np.int16)
    uni_ref = rng.integers(0, 3, size=(2, 2, PER)).astype(np.uint8)
    return (*tabs, uni_field, uni_ref), placed


# ---- one B picture with 2 + 2 references end to end ---------------------------------------------------------------------------------------
E2E_DEPTH = 3


def e2e_sel(api):
    return api.SelectParams(PER, min_depth=E2E_DEPTH, max_depth=E2E_DEPTH)


def chain(oracle_lib, hmo, api, cur, lists, w, h, bd, lambda_q16, bits, had=1):
    """the model of steps 1-4 of the chain on one B picture (integer MVs (0,0), predictors (0,0)): the oracle's refinement per (list,
    reference), select_refs_model at 256 per list, the oracle's refinement against the origin built by origin4, select_dirs_refs4_picture
    -> dict"""
    import select_refs_model as srm
    from hmme import synth
    m = synth.MARGIN
    n = dm.n_ctus(w, h)
    sel = e2e_sel(api)
    R = len(lists[0])
    imv = np.zeros((n, 593, 2), np.int16)
    uni = [[oracle_lib.refine_frame(cur, ref, (m, m), w, h, imv, None, lambda_q16, had, bd, n_threads=4) for ref in lists[l]] for l in range(2)]
    mv_uni = np.stack([np.stack([u[0] for u in uni[l]]) for l in range(2)])
    cost_uni = np.stack([np.stack([u[1] for u in uni[l]]) for l in range(2)])
    sel_l = [srm.select_refs_picture(mv_uni[l], cost_uni[l], sel, w, h, srm.hm_ref_cost(R, lambda_q16), 0, None, lambda_q16, None) for l in range(2)]
    uni_field, uni_ref = np.stack([u[0] for u in sel_l]), np.stack([u[1] for u in sel_l])
    q, c = [[], []], [[], []]
    for l in range(2):
        org = np.ascontiguousarray(np.pad(origin4(hmo, cur, lists[1 - l], w, h, bd, uni_field[1 - l], uni_ref[1 - l]), m))
        for ref in lists[l]:
            a, b = oracle_lib.refine_frame(org, ref, (m, m), w, h, imv, None, lambda_q16, had, bd, n_threads=4)
            q[l].append(a); c[l].append(b)
    mv_bi, cost_bi = np.stack([np.stack(x) for x in q]), np.stack([np.stack(x) for x in c])
    field, ref, dirs, slot, cost = select_dirs_refs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, w, h, bits, 0, None, lambda_q16)
    return dict(mv_uni=mv_uni, cost_uni=cost_uni, uni_field=uni_field, uni_ref=uni_ref, mv_bi=mv_bi, cost_bi=cost_bi, field=field, ref=ref, dirs=dirs, slot=slot,
                cost=cost)


def beyond_the_64_form(slot, dirs, ref):
    """what the 64 form cannot express -> (decided PUs with a slot < 384 and a reference index != 0, 8x8 blocks that mix reference indices)"""
    pus = set()
    for k in range(slot.shape[0]):
        for b in range(PER):
            s, d = int(slot[k, b]), int(dirs[k, b])
            if s < 384 and d in (1, 2, 3) and any((d >> l) & 1 and int(ref[l, k, b]) not in (0, NO_REF) for l in range(2)):
                pus.add((k, s))
    key = b4.block_of(ref[0]).astype(np.int32) * 256 + b4.block_of(ref[1]).astype(np.int32)
    return len(pus), int((key != key[:, :, :1]).any(axis=2).sum())


def b_refs_scene(w, h, bd, seed, n_refs=2):
    """bi4_model.b_scene with n_refs references per list: 4x4 regions of the current picture drawn from one of the 2 * n_refs unrelated
    textures or from the average of one of each list, plus noise -- neighbouring 4x4 blocks differ in direction AND reference, so that
    8x4 / 4x8 PUs are chosen and 8x8 blocks mix reference indices -> padded (cur, ((list 0's references), (list 1's)))"""
    from hmme import synth
    m = synth.MARGIN
    lists = tuple(tuple(synth.make_pair(w, h, seed=seed + 31 * (n_refs * l + r), bit_depth=bd, max_mv=2)[1] for r in range(n_refs)) for l in range(2))
    tex = [[lists[l][r][m:m + h, m:m + w].astype(np.int64) for r in range(n_refs)] for l in range(2)]
    rng = np.random.default_rng(seed + 62)
    shape = ((h + 3) // 4, (w + 3) // 4)
    kind, r0, r1 = rng.integers(0, 3, size=shape), rng.integers(0, n_refs, size=shape), rng.integers(0, n_refs, size=shape)
    up = lambda a: np.kron(a, np.ones((4, 4), np.int64))[:h, :w]
    kind, r0, r1 = up(kind), up(r0), up(r1)
    a = sum(np.where(r0 == r, tex[0][r], 0) for r in range(n_refs))
    b = sum(np.where(r1 == r, tex[1][r], 0) for r in range(n_refs))
    cur = np.where(kind == 0, a, np.where(kind == 1, b, (a + b + 1) >> 1)) + rng.integers(-2, 3, size=(h, w))
    return synth.pad_plane(np.clip(cur, 0, (1 << bd) - 1)), lists


# ---- the cases tests/test_gpu_bi_refs4.py runs, whose content tests/test_bi_refs4_cpu.py examines on the model alone -------------------------
E2E_SIZE, E2E_SEED, E2E_LAMBDA_Q16 = (136, 72), 4300, dm.LAMBDA_Q16
# (size, bit depth, (n0, n1), seed) of the random 4x4 fields; chroma runs at the even sizes with at most 4 + 4 references
FIELD_CASES = (((64, 64), 8, (2, 2), 9100), ((101, 71), 10, (4, 4), 9101), ((65, 67), 12, (16, 1), 9102), ((130, 66), 8, (4, 4), 9103), ((16, 16), 10, (2, 2), 9104),
               ((9, 9), 8, (2, 2), 9105), ((136, 72), 8, (2, 3), 9106))
