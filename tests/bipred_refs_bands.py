"""The end-to-end content of a B picture with two references per list, shared by tests/test_select_dirs_refs_cpu.py (the numpy route on
it: the oracle's searches and refinements, the models' decisions) and tests/test_gpu_bipred_refs.py (the device's pipeline on it): a
136x72 picture of four vertical bands, each planted from another (list, reference) pair at its own integer MV -- list 0 reference 0,
list 0 reference 1, the rounded average of list 0 reference 0 and list 1 reference 0, list 1 reference 1.  Every 8x8 block at least 8
samples inside a band must come out with the planted direction and reference indices."""
import ctypes as C

import numpy as np

import select_dirs_refs_model as drm
import select_refs_model as srm
from frame_helpers import clip_mv, dims, oracle_bi_search, origin_picture

W, H, N, R = 136, 72, 6, 2
SR_UNI, SR_BI = 8, 4
NO = drm.NO_REF
# (first column, end column, direction, (reference in list 0, list 1)); the MV of each (list, reference) texture, in samples
BANDS = ((0, 32, 1, (0, NO)), (32, 64, 1, (1, NO)), (64, 96, 3, (0, 0)), (96, 136, 2, (NO, 1)))
MOVES = (((3, -2), (-1, 2)), ((-2, 1), (2, 3)))


def content(seed=4000):
    """-> (padded current picture, ((list 0's padded references), (list 1's))).  Three textures are unrelated; list 1's reference 0 shows,
    at ITS move, list 0's reference 0 at its move plus noise of +-24: an 8x8 block of the averaged band -- the bottom CTU row is 8 samples
    high, so its CUs are 8x8 -- then finds both halves in the uni pass (each within the noise), which two unrelated textures do not
    allow at that size, and bi still beats either list by half the noise"""
    from hmme import synth
    m = synth.MARGIN
    tex = [[synth.make_pair(W, H, seed=seed + 17 * (2 * l + r), max_mv=0)[1] for r in range(R)] for l in range(2)]
    (ax, ay), (bx, by) = MOVES[0][0], MOVES[1][0]
    noise = np.random.default_rng(seed + 1).integers(-24, 25, size=tex[0][0].shape)
    noisy = np.clip(np.roll(tex[0][0], (by - ay, bx - ax), axis=(0, 1)).astype(np.int32) + noise, 0, 255)
    tex[1][0] = synth.pad_plane(noisy[m:m + H, m:m + W])                       # a plane's margins are its edge samples, on the device as here
    lists = tuple(tuple(t) for t in tex)
    moved = [[lists[l][r][m + dy:m + dy + H, m + dx:m + dx + W].astype(np.int32) for r, (dx, dy) in enumerate(MOVES[l])] for l in range(2)]
    cur = np.zeros((H, W), np.int32)
    for x0, x1, d, (r0, r1) in BANDS:
        if d == 3:
            cur[:, x0:x1] = (moved[0][r0][:, x0:x1] + moved[1][r1][:, x0:x1] + 1) >> 1
        else:
            cur[:, x0:x1] = moved[d - 1][r0 if d == 1 else r1][:, x0:x1]
    return synth.pad_plane(cur), lists


def planted_blocks():
    """(ctu, block, direction, (ref 0, ref 1)) of every 8x8 block of the picture that lies at least 8 samples inside a band"""
    cx_n, cy_n = dims(W, H)
    out = []
    for ctu in range(cx_n * cy_n):
        for b in range(64):
            x, y = (ctu % cx_n) * 64 + (b % 8) * 8, (ctu // cx_n) * 64 + (b // 8) * 8
            if y >= H:
                continue
            for x0, x1, d, refs in BANDS:
                if x >= x0 + 8 and x + 8 <= min(x1, W) - 8:
                    out.append((ctu, b, d, refs))
    return out


def bands_hold(dirs, ref):
    """dirs uint8[N, 64], ref uint8[2, N, 64] -> the planted blocks that do NOT carry their direction and indices (empty: the condition holds)"""
    return [(c, b) for c, b, d, refs in planted_blocks() if dirs[c, b] != d or (int(ref[0, c, b]), int(ref[1, c, b])) != refs]


def refs_prediction(hmo, others, w, h, bd, field, ref_field):
    """frame_helpers.oracle_prediction with a plane per block: hmo_pred_block_qpel for every CTU of the picture, whole 64x64 blocks (partial
    edge CTUs too), from others[index] -- others[0] where the index is >= len(others).  field [n_ctu, 1 | 64, 2], ref_field [n_ctu, 1 | 64]
    -> int16 [ctus_y * 64, ctus_x * 64]"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    out = np.zeros((cy_n * 64, cx_n * 64), np.int16)
    os_ = out.shape[1]
    p16 = C.POINTER(C.c_int16)
    per = field.shape[1]
    g = 64 if per == 1 else 8
    for ctu in range(cx_n * cy_n):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(per):
            bx, by = (b % 8) * g, (b // 8) * g
            idx = int(ref_field[ctu, b])
            ref = others[idx if idx < len(others) else 0]
            rs = ref.shape[1]
            qx, qy = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
            src = C.cast(ref.ctypes.data + 2 * ((m + cu_y + by) * rs + m + cu_x + bx), p16)
            dst = C.cast(out.ctypes.data + 2 * ((cu_y + by) * os_ + cu_x + bx), p16)
            hmo.hmo_pred_block_qpel(src, rs, g, g, qx, qy, bd, dst, os_)
    return out


def bits():
    return drm.hm_bits(R, R)


def numpy_route(oracle_lib, hmo, cur, lists, lq, sel):
    """steps 1-4 of the pipeline in include/hmme.h without the engine: the oracle's search and refinement per (list, reference),
    select_refs_model per list, the oracle's bi search and refinement on the origin built here, select_dirs_refs_model
    -> dict(mv_uni, cost_uni, uni_field, uni_ref, mv_bi, cost_bi, field, ref, dirs, slot, cost)"""
    from hmme import synth
    m = synth.MARGIN
    q, c = [[], []], [[], []]
    for l in range(2):
        for ref in lists[l]:
            ox, oy, _ = oracle_lib.search_frame(cur, ref, (m, m), W, H, SR_UNI, None, lq, 1, 8, n_threads=4)
            a, b = oracle_lib.refine_frame(cur, ref, (m, m), W, H, np.stack([ox, oy], axis=-1).astype(np.int16), None, lq, 1, 8, n_threads=4)
            q[l].append(a); c[l].append(b)
    mv_uni, cost_uni = np.stack([np.stack(x) for x in q]), np.stack([np.stack(x) for x in c])
    uni = [srm.select_refs_picture(mv_uni[l], cost_uni[l], sel, W, H, srm.hm_ref_cost(R, lq), 0, None, lq, None) for l in range(2)]
    uni_field, uni_ref = np.stack([u[0] for u in uni]), np.stack([u[1] for u in uni])
    q, c = [[], []], [[], []]
    for l in range(2):
        org = origin_picture(cur, refs_prediction(hmo, lists[1 - l], W, H, 8, uni_field[1 - l], uni_ref[1 - l]), W, H)
        for ref in lists[l]:
            bmv, _ = oracle_bi_search(oracle_lib, org, ref, W, H, SR_BI, None, None, lq, 1, 8, range(N))
            a, b = oracle_lib.refine_frame(np.ascontiguousarray(np.pad(org, m)), ref, (m, m), W, H, bmv, None, lq, 1, 8, n_threads=4)
            q[l].append(a); c[l].append(b)
    mv_bi, cost_bi = np.stack([np.stack(x) for x in q]), np.stack([np.stack(x) for x in c])
    field, ref, dirs, slot, cost = drm.select_dirs_refs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, W, H, bits(), 0, None, lq)
    return dict(mv_uni=mv_uni, cost_uni=cost_uni, uni_field=uni_field, uni_ref=uni_ref, mv_bi=mv_bi, cost_bi=cost_bi, field=field, ref=ref, dirs=dirs, slot=slot,
                cost=cost)
