"""The end-to-end content of a 4:2:0 B picture of a WP slice with two references per list, shared by tests/test_bi_refs_w_cpu.py (the
condition on the models alone) and tests/test_gpu_b_refs_wp_420.py (the device's pipeline): tests/bipred_refs_bands.py's four bands, every
reference stored FADED by its own gain and offset, with the hand-set weight that undoes its fade -- so the weighted searches see the
planted textures, and the weighted prediction is close to the current picture where the unweighted one is off by the fades.  The chroma
planes are synth.make_chroma_pair textures, faded per component."""
import numpy as np

import bipred_refs_bands as bands
from frame_helpers import dims

W, H, N, R = bands.W, bands.H, bands.N, bands.R
# how list l's reference r is stored: ((gain * x + 32) >> 6) + lift -- and the (w0, offset, shift, round) that undoes it, set by hand:
# w0 ~ 4096 / gain, offset ~ -lift * w0 / 64.  One shift for all: one log2WeightDenom per slice
FADES = (((48, 10), (32, 20)), ((56, 5), (40, 30)))
WPS = (((85, -13, 6, 32), (128, -40, 6, 32)), ((73, -6, 6, 32), (102, -48, 6, 32)))
# chroma: CHROMA_WPS[component][list][reference]; Cb and Cr differ in their shift
CHROMA_FADES = ((((52, 8), (60, -4)), ((44, 12), (64, 9))), (((36, 25), (58, 3)), ((50, -6), (40, 14))))
CHROMA_WPS = ((((79, -10, 6, 32), (68, 4, 6, 32)), ((93, -17, 6, 32), (64, -9, 6, 32))),
              (((57, -22, 5, 16), (35, -2, 5, 16)), ((41, 4, 5, 16), (51, -11, 5, 16))))


def fade(plane, gain, lift):
    """sample by sample, so a padded plane's margins stay its edge samples"""
    return np.ascontiguousarray(np.clip(((gain * plane.astype(np.int32) + 32) >> 6) + lift, 0, 255).astype(np.int16))


def content(seed=4000):
    """-> (padded current picture, lists[l][r] padded FADED references, cur_chroma (cb, cr), chroma[l][r] = (cb, cr) padded faded planes)"""
    from hmme import synth
    cur, lists = bands.content(seed)
    luma = tuple(tuple(fade(lists[l][r], *FADES[l][r]) for r in range(R)) for l in range(2))
    still = np.zeros((1, 1, 2), np.int64)
    cur_chroma, _ = synth.make_chroma_pair(W, H, still, seed=seed + 5)
    chroma = tuple(tuple(tuple(fade(p, *CHROMA_FADES[c][l][r]) for c, p in enumerate(synth.make_chroma_pair(W, H, still, seed=seed + 11 + 3 * (2 * l + r))[1]))
                         for r in range(R)) for l in range(2))
    return cur, luma, cur_chroma, chroma


def chroma_comps(chroma):
    """model order: [component][list][reference]"""
    return [[[chroma[l][r][c] for r in range(R)] for l in range(2)] for c in range(2)]


def chroma_flat(things):
    """engine order of planes or weights given as [list][reference] -> (cb, cr): ([cb0, cr0, cb1, cr1] of list 0, of list 1)"""
    return tuple([things[l][r][c] for r in range(R) for c in range(2)] for l in range(2))


def chroma_wps_flat():
    return tuple([CHROMA_WPS[c][l][r] for r in range(R) for c in range(2)] for l in range(2))


def planted_fields():
    """-> (field int16[2, N, 64, 2], dirs uint8[N, 64], refs uint8[2, N, 64]): the motion, direction and reference indices the bands were
    planted with, for every 8x8 block that starts inside the picture (0xFF elsewhere)"""
    cx_n, cy_n = dims(W, H)
    field = np.zeros((2, N, 64, 2), np.int16)
    dirs = np.full((N, 64), 0xFF, np.uint8)
    refs = np.full((2, N, 64), 0xFF, np.uint8)
    for ctu in range(N):
        for b in range(64):
            x, y = (ctu % cx_n) * 64 + (b % 8) * 8, (ctu // cx_n) * 64 + (b // 8) * 8
            if x >= W or y >= H:
                continue
            x0, x1, d, idx = next(band for band in bands.BANDS if band[0] <= x < band[1])
            dirs[ctu, b] = d
            for l in range(2):
                if (d >> l) & 1:
                    refs[l, ctu, b] = idx[l]
                    field[l, ctu, b] = (4 * bands.MOVES[l][idx[l]][0], 4 * bands.MOVES[l][idx[l]][1])
    return field, dirs, refs


def sse(pred, cur):
    """of a [H, W] prediction against the padded current picture"""
    from hmme import synth
    m = synth.MARGIN
    d = np.asarray(pred).astype(np.int64) - cur[m:m + H, m:m + W].astype(np.int64)
    return int((d * d).sum())
