#!/usr/bin/env python3
"""Generate tests/golden/ref_blocks.npz, ref_tails.npz, ref_wp_estimate.npz and ref_dist.npz from the COMPILED REFERENCE
(oracle/_ref/libhmref.so, built by `make -C oracle ref`).  Run where the reference library was built:

    python tests/golden/gen_ref_tails_golden.py [blocks] [tails] [wp] [dist] [refine]

Every file holds inputs and the reference's outputs -- data only -- and is written with fixed archive timestamps, so that two runs give
identical files.  The entry points are those of oracle/ref_harness.cpp (ref_pred_block, ref_add_avg, ref_add_weight_uni, ref_add_weight_bi,
ref_wp_estimate, ref_dist); tests/ref_tails.py reads the files for tests/test_ref_tails_cpu.py and tests/test_gpu_ref_tails.py.

ref_blocks.npz -- TComPrediction::xPredInterBlk, bit depths 8..12
  bds                [5]
  luma_src           [5, 35, 15, 15]     content 0 random, 1 binary {0, maxv}, 2 all maxv; 3 + 2 * phase + k: the tap-sign pattern of
                                         phase = 4 * yFrac + xFrac (k = 0: maxv where tap_x[i] * tap_y[j] > 0, else 0) and its complement (k = 1)
  luma_out           [5, 3, 16, 2, 8, 8] contents 0..2 at all 16 phases, [0] the clipped sample (bi = false), [1] the Pel intermediate
  luma_sign_out      [5, 16, 2, 2, 8, 8] [bd, phase, k, bi]: each tap-sign picture at its own phase
  chroma_src         [5, 131, 7, 7]      the same for a 4x4 block of a 4:2:0 chroma component, 64 phases = 8 * yFrac + xFrac
  chroma_out         [5, 3, 64, 2, 4, 4]
  chroma_sign_out    [5, 64, 2, 2, 4, 4]
  luma_extremes      [5, 2], chroma_extremes [5, 2]   smallest and largest intermediate per bit depth; *_extreme_at [5, 2, 2] = (phase, k)
ref_tails.npz -- TComYuv::addAvg, xWeightedPredictionUni, xWeightedPredictionBi on intermediates of ref_blocks.npz
  ops_luma / ops_chroma [5, 4, 2]        operand (content index, phase): 0 the largest intermediate's block, 1 the smallest's, 2 and 3 random content
  pairs              [4, 2]              operand pairs: max + max, min + min, max + min, random + random
  triples            [60, 3]             HM's (iWeight, iOffset, log2WeightDenom)
  bi_weights         [60, 5]             (iWeight0, iOffset0, iWeight1, iOffset1, log2WeightDenom)
  cr_shift                               component Cr of case k uses entry (k + cr_shift) % 60
  avg_luma [5, 4, 8, 8], avg_chroma [5, 2, 4, 4, 4]
  uni_luma [5, 4, 60, 8, 8] (operand, triple), uni_chroma [5, 2, 4, 60, 4, 4]
  bi_luma  [5, 4, 60, 8, 8] (pair, bi weight), bi_chroma  [5, 2, 4, 60, 4, 4]
  sign_weights [4]                       entries of triples / bi_weights used on the luma tap-sign content of EVERY phase: case n = 2 * phase + k, the
                                         other operand its complement n ^ 1:  sign_avg_luma [5, 32, 8, 8], sign_uni_luma, sign_bi_luma [5, 32, 4, 8, 8]
ref_wp_estimate.npz -- the slice-level estimator (TEncSlice.cpp:675-694)
  n                                      number of cases;  per case i:  c{i}_meta = (chroma format, bit depth, n_l0, n_l1, log2 denom start),
  c{i}_y [1 + n_refs, h, w] (+ c{i}_cb, c{i}_cr for 4:2:0): the current picture, then the references, list 0 first
  c{i}_table, c{i}_final [n_refs, 3, 4] = (bPresentFlag, iWeight, iOffset, log2WeightDenom) after initWpScaling / after xCheckWPEnable,
  c{i}_flags [2] = the slice's test-weight-pred flags;  names: the cases' names;  events: which case shows which event
ref_dist.npz -- TComRdCost::getDistPart
  sizes [25, 2] (w, h), bds [3], org_{w}x{h} / pred_{w}x{h} [3, 4, h, w] (content 0 random, 1 binary, 2 spectral, 3 differences of 1..3),
  dist [25, 3, 4, 3] = DF_SSE, DF_HADS, DF_SAD
ref_refine.npz -- TEncSearch::xPatternSearchFracDIF (ref_frac_refine, ref_frac_refine_bi) on tap-sign pictures, integer MV (0, 0), all 593 slots
  lambda_q16                             of lambda 57.9; a case's lambda is 0 or that
  bds [3] = 8, 10, 12;  sign [4, 2]      the (phase, k) of the four reference pictures: the luma tap-sign pattern tiled over 64x64
  ref [3, 4, 64, 64], cur [3, 4, 2, 64, 64]   per reference: its complement, and a random picture
  plain [3, 4, 2, 2, 593, 3]             [bd, reference, current, SAD | Hadamard, slot] = (qmv x, qmv y, cost);  plain_meta [.., 3] = (lambda_q16, pred x, pred y)
  bi_bds [2] = 8, 10;  bi [2, 4, 2, 593, 3], bi_meta [2, 4, 2, 3]   the bBi call on the origin 2 * cur - other in {2 maxv, -maxv}: cur = sign picture 0,
                                         other = its complement (bi_cur, bi_other [2, 64, 64]), against each of the four references
  origin_bds [4] = 8..11;  origin_cur, origin_ref [4, 64, 64] random pictures;  origin_slots [9] the 8x8 slots at the golden block positions;
  origin [4, 32, 3]                      the bBi call (Hadamard, lambda 57.9, predictor (0, 0)) of golden block case n (phase n >> 1, k = n & 1, nine per
                                         picture as tests/ref_tails.py lays them out) on the origin 2 * cur - P, P = the reference's recorded clipped block
                                         of ref_blocks.npz inside the block and the other picture's own samples elsewhere
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import oracle_py as O  # noqa: E402

BDS = (8, 9, 10, 11, 12)
LUMA_TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]])
CHROMA_TAPS = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
                        [-2, 10, 58, -2]])
SIGN_WEIGHTS = (3, 14, 27, 44)   # entries of triples / bi_weights that run on the tap-sign content of every phase
LIMIT = os.path.getsize(os.path.join(HERE, "frac_wp.npz"))   # no new golden is larger than the largest committed before these


def save(name, d):
    """np.savez_compressed with fixed timestamps: identical inputs give identical bytes"""
    path = os.path.join(HERE, name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= LIMIT, (name, size)


def tap_sign(taps, nfrac, phase, size, maxv):
    """[size, size] picture: maxv where tap_x[i] * tap_y[j] > 0, tiled with the filter's length from the footprint of output sample (0, 0)"""
    n = taps.shape[1]
    tx, ty = taps[phase % nfrac], taps[phase // nfrac]
    pos = np.outer(ty, tx) > 0
    ys, xs = np.mgrid[0:size, 0:size]
    return np.where(pos[ys % n, xs % n], maxv, 0)


def gen_blocks():
    rng = np.random.default_rng(20240)
    d = dict(bds=np.array(BDS))
    for name, taps, nfrac, n, comp in (("luma", LUMA_TAPS, 4, 8, 0), ("chroma", CHROMA_TAPS, 8, 4, 1)):
        s = n + taps.shape[1] - 1
        nph = nfrac * nfrac
        src = np.zeros((len(BDS), 3 + 2 * nph, s, s), np.int16)
        out = np.zeros((len(BDS), 3, nph, 2, n, n), np.int16)
        sign_out = np.zeros((len(BDS), nph, 2, 2, n, n), np.int16)
        ext, ext_at = np.zeros((len(BDS), 2), np.int64), np.zeros((len(BDS), 2, 2), np.int64)
        for i, bd in enumerate(BDS):
            maxv = (1 << bd) - 1
            src[i, 0] = rng.integers(0, maxv + 1, (s, s))
            src[i, 1] = np.where(rng.integers(0, 2, (s, s)) == 1, maxv, 0)
            src[i, 2] = maxv
            for ph in range(nph):
                p = tap_sign(taps, nfrac, ph, s, maxv)
                src[i, 3 + 2 * ph], src[i, 4 + 2 * ph] = p, maxv - p
            for c in range(3):
                for ph in range(nph):
                    for bi in range(2):
                        out[i, c, ph, bi] = O.ref_pred_block(src[i, c], n, n, ph % nfrac, ph // nfrac, bd, bool(bi), comp)
            for ph in range(nph):
                for k in range(2):
                    for bi in range(2):
                        sign_out[i, ph, k, bi] = O.ref_pred_block(src[i, 3 + 2 * ph + k], n, n, ph % nfrac, ph // nfrac, bd, bool(bi), comp)
            if comp:   # Cr goes the same way as Cb: spot check that the harness' component argument reaches the same filter
                assert np.array_equal(O.ref_pred_block(src[i, 0], n, n, 3, 5, bd, True, 2), out[i, 0, 5 * 8 + 3, 1])
            # the tap-sign pictures reach the extremes of ALL cases, at output sample (0, 0); the Pel did not wrap: it is the exact value
            hi, lo = int(sign_out[i, :, 0, 1].max()), int(sign_out[i, :, 1, 1].min())
            assert hi >= int(out[i, :, :, 1].max()) and hi == int(sign_out[i, :, :, 1].max()), (name, bd)
            assert lo <= int(out[i, :, :, 1].min()) and lo == int(sign_out[i, :, :, 1].min()), (name, bd)
            assert hi > int(out[i, :, :, 1].max()) and lo < int(out[i, :, :, 1].min()), (name, bd)
            ph_hi, ph_lo = int(np.argmax(sign_out[i, :, 0, 1, 0, 0])), int(np.argmin(sign_out[i, :, 1, 1, 0, 0]))
            assert sign_out[i, ph_hi, 0, 1, 0, 0] == hi and sign_out[i, ph_lo, 1, 1, 0, 0] == lo
            # ... checked against the exact sums in Python integers: shift 6 - headroom after the first stage, 6 after the second
            head = max(2, 14 - bd)
            for ph, k, got in ((ph_hi, 0, hi), (ph_lo, 1, lo)):
                tx, ty = taps[ph % nfrac], taps[ph // nfrac]
                foot = src[i, 3 + 2 * ph + k][:taps.shape[1], :taps.shape[1]].astype(np.int64)
                if ph // nfrac == 0 or ph % nfrac == 0:   # one stage
                    row = foot[taps.shape[1] // 2 - 1] if ph // nfrac == 0 else foot[:, taps.shape[1] // 2 - 1]
                    exact = (int((row * (tx if ph // nfrac == 0 else ty)).sum()) - (8192 << (6 - head))) >> (6 - head)
                else:
                    mid = [(int((foot[j] * tx).sum()) - (8192 << (6 - head))) >> (6 - head) for j in range(taps.shape[1])]
                    assert all(-32768 <= m <= 32767 for m in mid)
                    exact = int((np.array(mid) * ty).sum()) >> 6
                assert exact == got and -32768 + 4096 < got < 32767 - 4096, (name, bd, ph, k, exact, got)
            ext[i], ext_at[i] = (lo, hi), ((ph_lo, 1), (ph_hi, 0))
            print(f"{name} {bd}-bit: intermediate in [{lo}, {hi}] at phases {ph_lo}, {ph_hi}; other content [{int(out[i, :, :, 1].min())}, {int(out[i, :, :, 1].max())}]")
        d.update({f"{name}_src": src, f"{name}_out": out, f"{name}_sign_out": sign_out, f"{name}_extremes": ext, f"{name}_extreme_at": ext_at})
    save("ref_blocks.npz", d)


def weight_cases(rng):
    triples = [(w, o, d) for d in (0, 7) for w in (-128, -1, 0, 1, 127, 1 << d) for o in (-128, 127)]
    triples += [(int(rng.integers(-128, 128)), int(rng.integers(-128, 128)), int(rng.integers(0, 8))) for _ in range(36)]
    bi = [(w0, o0, w1, o1, d) for d in (0, 7) for w0, w1 in ((-128, -128), (127, 127), (-128, 127), (-1, 1), (0, 1 << d), (1 << d, 1 << d))
          for o0, o1 in ((-128, -128), (127, 127), (-128, 127))]
    bi += [tuple(int(v) for v in rng.integers(-128, 128, 4)) + (int(rng.integers(0, 8)),) for _ in range(24)]
    assert len(triples) == 60 and len(bi) == 60
    return np.array(triples), np.array(bi)


def gen_tails():
    rng = np.random.default_rng(20241)
    with np.load(os.path.join(HERE, "ref_blocks.npz")) as g:
        B = {k: g[k] for k in g.files}
    triples, bi_w = weight_cases(rng)
    pairs = np.array([(0, 0), (1, 1), (0, 1), (2, 3)])
    cr_shift = 7
    d = dict(bds=np.array(BDS), triples=triples, bi_weights=bi_w, pairs=pairs, cr_shift=np.array(cr_shift))

    def operand(name, nph, i, op):
        c, ph = int(op[0]), int(op[1])
        return B[f"{name}_out"][i, c, ph, 1] if c < 3 else B[f"{name}_sign_out"][i, ph, (c - 3) & 1, 1]

    for name, nph, n, comps in (("luma", 16, 8, (0,)), ("chroma", 64, 4, (1, 2))):
        ops = np.zeros((len(BDS), 4, 2), np.int64)
        avg = np.zeros((len(BDS), len(comps), 4, n, n), np.int16)
        uni = np.zeros((len(BDS), len(comps), 4, 60, n, n), np.int16)
        bi = np.zeros((len(BDS), len(comps), 4, 60, n, n), np.int16)
        for i, bd in enumerate(BDS):
            (ph_lo, k_lo), (ph_hi, k_hi) = B[f"{name}_extreme_at"][i]
            ops[i] = ((3 + 2 * ph_hi + k_hi, ph_hi), (3 + 2 * ph_lo + k_lo, ph_lo), (0, int(rng.integers(1, nph))), (0, int(rng.integers(1, nph))))
            P = [operand(name, nph, i, ops[i, o]) for o in range(4)]
            assert P[0].max() == B[f"{name}_extremes"][i, 1] and P[1].min() == B[f"{name}_extremes"][i, 0]
            for ci, comp in enumerate(comps):
                for j, (a, b) in enumerate(pairs):
                    avg[i, ci, j] = O.ref_add_avg(P[a], P[b], bd, comp)
                for k in range(60):
                    kk = (k + cr_shift) % 60 if comp == 2 else k
                    w, o, dn = (int(v) for v in triples[kk])
                    for o_i in range(4):
                        uni[i, ci, o_i, k] = O.ref_add_weight_uni(P[o_i], bd, comp, w, o, dn)
                    w0, o0, w1, o1, dn = (int(v) for v in bi_w[kk])
                    for j, (a, b) in enumerate(pairs):
                        bi[i, ci, j, k] = O.ref_add_weight_bi(P[a], P[b], bd, comp, w0, o0, w1, o1, dn)
        if name == "luma":
            avg, uni, bi = avg[:, 0], uni[:, 0], bi[:, 0]
            # every phase: tap-sign case n (phase n >> 1, k = n & 1) with its complement n ^ 1 as the other operand, four of the weights
            sw = np.array(SIGN_WEIGHTS)
            s_avg, s_uni, s_bi = np.zeros((len(BDS), 32, n, n), np.int16), np.zeros((len(BDS), 32, 4, n, n), np.int16), np.zeros((len(BDS), 32, 4, n, n), np.int16)
            for i, bd in enumerate(BDS):
                for c in range(32):
                    A, Bc = B["luma_sign_out"][i, c >> 1, c & 1, 1], B["luma_sign_out"][i, c >> 1, (c & 1) ^ 1, 1]
                    s_avg[i, c] = O.ref_add_avg(A, Bc, bd, 0)
                    for j, k in enumerate(sw):
                        s_uni[i, c, j] = O.ref_add_weight_uni(A, bd, 0, *[int(v) for v in triples[k]])
                        s_bi[i, c, j] = O.ref_add_weight_bi(A, Bc, bd, 0, *[int(v) for v in bi_w[k]])
            d.update(sign_weights=sw, sign_avg_luma=s_avg, sign_uni_luma=s_uni, sign_bi_luma=s_bi)
        d.update({f"ops_{name}": ops, f"avg_{name}": avg, f"uni_{name}": uni, f"bi_{name}": bi})
    save("ref_tails.npz", d)


# ---- the estimator's pictures ------------------------------------------------------------------------------------------------------------
def checkerboard(w, h, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + yy) & 1, b, a)


def fade(ref, gain, offset, maxv):
    return np.clip(np.floor(gain * ref + 0.5).astype(np.int64) + offset, 0, maxv)


def wp_cases():
    """-> list of (name, chroma format, bit depth, n_l0, n_l1, [current, references...]); a picture is a luma array (400) or (y, cb, cr) (420)"""
    rng = np.random.default_rng(20242)
    cases = []

    def pic(w, h, lo, hi, fmt):
        y = rng.integers(lo, hi, (h, w))
        return y if fmt == 400 else (y, rng.integers(lo, hi, (h // 2, w // 2)), rng.integers(lo, hi, (h // 2, w // 2)))

    def each(p, f):
        return f(p) if not isinstance(p, tuple) else tuple(f(c) for c in p)

    for fmt in (400, 420):
        w, h = (32, 16)
        for gain in (0.5, 1.5, 2.5, 3.5):      # cur = gain * ref + offset: the reference kept where nothing clips
            for off in (-9, 14):
                bd = 10 if gain == 1.5 else 8
                sc = 1 << (bd - 8)
                ref = pic(w, h, 40 * sc, int(min(250, 230 / gain)) * sc, fmt) if gain >= 1 else pic(w, h, 40 * sc, 250 * sc, fmt)
                cases.append((f"fade_{fmt}_{gain}_{off}", fmt, bd, 1, 0, [each(ref, lambda c: fade(c, gain, off * sc, (1 << bd) - 1)), ref]))
        p = pic(w, h, 0, 256, fmt)
        cases.append((f"identical_{fmt}", fmt, 8, 1, 0, [p, each(p, np.copy)]))
        cases.append((f"unrelated_{fmt}", fmt, 8, 1, 0, [pic(w, h, 0, 256, fmt), pic(w, h, 0, 256, fmt)]))
        flat = each(pic(w, h, 0, 256, fmt), lambda c: np.full_like(c, 77))
        cases.append((f"constant_current_{fmt}", fmt, 8, 1, 0, [flat, pic(w, h, 0, 256, fmt)]))
        cases.append((f"constant_reference_{fmt}", fmt, 8, 1, 0, [pic(w, h, 0, 256, fmt), flat]))
        cases.append((f"constant_both_{fmt}", fmt, 8, 1, 0, [flat, each(flat, lambda c: c + 3)]))
        cases.append((f"constant_same_{fmt}", fmt, 8, 1, 0, [flat, each(flat, np.copy)]))
        binary = each(pic(w, h, 0, 2, fmt), lambda c: c * 4095)
        cases.append((f"extremes12_{fmt}", fmt, 12, 2, 0, [binary, each(binary, lambda c: 4095 - c), each(binary, lambda c: np.full_like(c, 4095))]))
        ramp = each(pic(w, h, 0, 4096, fmt), lambda c: c)
        cases.append((f"fade12_{fmt}", fmt, 12, 1, 0, [each(ramp, lambda c: fade(c, 0.75, 500, 4095)), ramp]))
        # several references: an identical one beside a fade whose weight does not fit at the starting denominator
        W, H = 64, 48
        cur = pic(W, H, 30, 200, fmt)
        weak = each(cur, lambda c: fade(c - 100, 1 / 3.5, 100, 255))
        cases.append((f"two_refs_{fmt}", fmt, 8, 2, 0, [cur, each(cur, np.copy), weak]))
        four = [each(cur, np.copy), each(cur, lambda c: fade(c, 0.8, 10, 255)), pic(W, H, 0, 256, fmt), each(cur, lambda c: fade(c, 1.1, -20, 255))]
        cases.append((f"four_refs_{fmt}", fmt, 8, 4, 0, [cur] + four))
        cases.append((f"split_2_2_{fmt}", fmt, 8, 2, 2, [cur, four[1], four[2], weak, four[3]]))
        cases.append((f"split_2_2_plain_{fmt}", fmt, 8, 2, 2, [cur, four[1], four[0], four[3], four[2]]))
    # a ratio of EXACTLY 0.99 (396 / 400): `>=` switches the weight off, `>` would keep it (found by a seeded search over such pairs)
    r99 = np.random.default_rng(649)
    ref = r99.integers(60, 200, (8, 16))
    cases.append(("ratio_exactly_0.99", 400, 8, 1, 0, [np.clip(ref + r99.integers(-12, 13, (8, 16)) + r99.integers(-2, 3), 0, 255), ref]))
    # 4:2:0 only: what the components do to one another
    y = rng.integers(0, 256, (16, 32))
    cases.append(("chroma_lowers_luma", 420, 8, 1, 0, [(y, checkerboard(16, 8, 190, 210), np.full((8, 16), 128)),
                                                        (y.copy(), checkerboard(16, 8, 18, 22), np.full((8, 16), 128))]))
    ry, rcb, rcr = rng.integers(0, 256, (16, 32)), rng.integers(30, 190, (8, 16)), rng.integers(30, 190, (8, 16))
    cases.append(("chroma_carries_ratio", 420, 8, 1, 0, [(rng.integers(0, 256, (16, 32)), rcb + 60, rcr + 60), (ry, rcb, rcr)]))
    ry = rng.integers(30, 200, (16, 32))
    cases.append(("chroma_switches_off", 420, 8, 1, 0, [(ry + 2, checkerboard(16, 8, 100, 135), checkerboard(16, 8, 100, 135)),
                                                         (ry, checkerboard(16, 8, 120, 130), checkerboard(16, 8, 120, 130))]))
    rcb = rng.integers(20, 61, (8, 16))
    cases.append(("chroma_offset_clamps", 420, 8, 1, 0, [(ry + 5, fade(rcb, 0.5, 170, 255), fade(rcb, 2.0, 130, 255)), (ry, rcb, rcb.copy())]))
    cases.append(("chroma_offset_clamps_10", 420, 10, 1, 0, [(4 * ry + 20, fade(4 * rcb, 0.5, 4 * 170, 1023), fade(4 * rcb, 2.0, 4 * 130, 1023)), (4 * ry, 4 * rcb, 4 * rcb)]))
    return cases


def raw_offset(cur, ref, bd, weight, d):
    """WeightPredAnalysis.cpp:236 before any clip, from the reference's own weight and denominator -- only to tell which cases the range rules
    touched (the events below); nothing of it is recorded"""
    n = cur.size
    dc = lambda p: (int(p.sum()) + (n >> 1)) // n
    real = d + bd - 8
    return ((dc(cur) << d) - weight * dc(ref) + (1 << (real - 1))) >> real


def gen_wp():
    cases = wp_cases()
    d = dict(n=np.array(len(cases)), names=np.array([c[0] for c in cases]))
    events = {"weight_lowers_denominator": [], "chroma_lowers_luma_denominator": [], "ratio_switches_off": [], "chroma_offset_clamps": [],
              "all_off_resets_table": [], "nan_ratio_stays_present": [], "ratio_exactly_threshold": []}
    for i, (name, fmt, bd, n_l0, n_l1, pics) in enumerate(cases):
        start = 7 if n_l0 > 3 else 6
        assert all(max(p.shape) <= 64 and min(p.shape) <= 48 for pic in pics for p in (pic if fmt == 420 else [pic]))
        table, final, flags = O.ref_wp_estimate(pics[0], pics[1:], n_l0, n_l1, bd, start)
        lumas = [p[0] if fmt == 420 else p for p in pics]
        d[f"c{i}_meta"] = np.array([fmt, bd, n_l0, n_l1, start])
        d[f"c{i}_y"] = np.stack(lumas).astype(np.int16)
        if fmt == 420:
            d[f"c{i}_cb"], d[f"c{i}_cr"] = (np.stack([p[c] for p in pics]).astype(np.int16) for c in (1, 2))
        d[f"c{i}_table"], d[f"c{i}_final"], d[f"c{i}_flags"] = table, final, flags
        ncomp = 3 if fmt == 420 else 1
        denom = int(table[0, 0, 3])
        assert (table[:, :ncomp, 3] == denom).all()
        if denom < start:
            luma_alone = O.ref_wp_estimate(lumas[0], lumas[1:], n_l0, n_l1, bd, start)[0]
            if fmt == 400 or int(luma_alone[0, 0, 3]) == denom:
                events["weight_lowers_denominator"].append(name)
            else:
                assert int(luma_alone[0, 0, 3]) == start
                events["chroma_lowers_luma_denominator"].append(name)
        if (table[:, 0, 0] == 0).any():
            events["ratio_switches_off"].append(name)
        if not flags.any():
            assert (final[:, :ncomp] == (0, 1, 0, 0)).all()
            events["all_off_resets_table"].append(name)
        else:
            assert np.array_equal(table, final)
        for r in range(n_l0 + n_l1):
            if fmt == 420 and table[r, 0, 0]:
                for c in (1, 2):
                    raw = raw_offset(pics[0][c], pics[1 + r][c], bd, int(table[r, c, 1]), denom)
                    if raw != int(table[r, c, 2]):
                        events["chroma_offset_clamps"].append(name)
            same = all(np.array_equal(a, b) for a, b in zip(pics[0] if fmt == 420 else [pics[0]], pics[1 + r] if fmt == 420 else [pics[1 + r]]))
            if same and table[r, 0, 0]:
                events["nan_ratio_stays_present"].append(name)
        if name == "ratio_exactly_0.99":   # the reference hands out only its decision: the two quotients of xSelectWP (:301-305) computed here, 8 bit
            org, rf = pics[0].astype(np.int64), pics[1].astype(np.int64)
            n = org.size
            dc = lambda p: (int(p.sum()) + (n >> 1)) // n
            ac = lambda p: int(np.abs(p - dc(p)).sum())
            weight = int(0.5 + min(max(-16.0, ac(org) / ac(rf)), 15.0) * 64)
            offset = min(max(-128, raw_offset(org, rf, 8, weight, 6)), 127)
            sad_wp = int(np.abs((org << 6) - (rf * weight + offset * 64)).sum()) // n
            sad_nowp = int(np.abs((org << 6) - (rf << 6)).sum()) // n
            assert (sad_wp, sad_nowp) == (396, 400) and denom == 6 and not table[0, 0, 0], (sad_wp, sad_nowp, weight, offset)
            events["ratio_exactly_threshold"] = [name]
        print(name, "denominator", denom, "flags", flags.tolist(), table[:, :ncomp].tolist())
    for k, v in events.items():
        print(k, sorted(set(v)))
        assert v, k                                 # no case silently stops exercising its branch
        d["event_" + k] = np.array(sorted(set(v)))
    save("ref_wp_estimate.npz", d)


def gen_dist():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spectral_content as sc
    rng = np.random.default_rng(20243)
    sizes = sorted({(int(w), int(h)) for _, _, w, h in O.slot_table()}) + [(4, 4)]
    bds = (8, 10, 12)
    d = dict(sizes=np.array(sizes), bds=np.array(bds))
    dist = np.zeros((len(sizes), len(bds), 4, 3), np.int64)
    dropped = 0
    for s, (w, h) in enumerate(sizes):
        org, pred = np.zeros((len(bds), 4, h, w), np.int16), np.zeros((len(bds), 4, h, w), np.int16)
        for i, bd in enumerate(bds):
            maxv = (1 << bd) - 1
            org[i, 0], pred[i, 0] = rng.integers(0, maxv + 1, (h, w)), rng.integers(0, maxv + 1, (h, w))
            org[i, 1], pred[i, 1] = rng.integers(0, 2, (h, w)) * maxv, rng.integers(0, 2, (h, w)) * maxv
            org[i, 2] = sc.bent_plane(w, h, bd)
            pred[i, 2] = sc.complement(org[i, 2], bd)
            org[i, 3] = rng.integers(3, maxv - 2, (h, w))
            pred[i, 3] = org[i, 3] + rng.integers(1, 4, (h, w)) * rng.choice([-1, 1], (h, w))
            for c in range(4):
                for kind in range(3):
                    dist[s, i, c, kind] = O.ref_dist(org[i, c], pred[i, c], bd, kind)
            if bd > 8:   # differences of 1..3: the per-sample shift drops every square below 1 << 2 (bd - 8) on its own
                total = int(((org[i, 3].astype(np.int64) - pred[i, 3]) ** 2).sum()) >> (2 * (bd - 8))
                dropped += total > dist[s, i, 3, 0]
        d[f"org_{w}x{h}"], d[f"pred_{w}x{h}"] = org, pred
    assert dropped >= len(sizes), dropped
    d["dist"] = dist
    save("ref_dist.npz", d)


def gen_refine():
    from hmme import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_tails as rt
    rng = np.random.default_rng(20244)
    table = O.slot_table()
    lam = 57.9
    lq = int(O.ref().ref_lambda_q16(lam))
    m = synth.MARGIN
    pad = synth.pad_plane
    sign = ((10, 0), (10, 1), (5, 0), (15, 1))

    def all_slots(org_p, ref_p, pred, use_lam, had, bd, bi):
        out = np.zeros((593, 3), np.int32)
        for s in range(593):
            x, y, w, h = (int(v) for v in table[s])
            hx, hy, qx, qy, cost = O.frac_refine(org_p, (m + x, m + y), ref_p, (m + x, m + y), w, h, (0, 0), pred, use_lam, had, bd, use_ref=True, bi=bi)
            out[s] = (2 * hx + qx, 2 * hy + qy, cost)
        return out

    def setting(a, b):
        return (lam if a & 1 else 0.0), ((0, 0) if b & 1 else (0, -2))

    bds = (8, 10, 12)
    d = dict(bds=np.array(bds), sign=np.array(sign), lambda_q16=np.array(lq))
    ref = np.zeros((3, 4, 64, 64), np.int16)
    cur = np.zeros((3, 4, 2, 64, 64), np.int16)
    plain, plain_meta = np.zeros((3, 4, 2, 2, 593, 3), np.int32), np.zeros((3, 4, 2, 2, 3), np.int64)
    for i, bd in enumerate(bds):
        maxv = (1 << bd) - 1
        for r, (ph, k) in enumerate(sign):
            p = tap_sign(LUMA_TAPS, 4, ph, 64, maxv)
            ref[i, r] = maxv - p if k else p
            cur[i, r, 0], cur[i, r, 1] = maxv - ref[i, r], rng.integers(0, maxv + 1, (64, 64))
            for c in range(2):
                for had in range(2):
                    use_lam, pred = setting(r + c, r + had)
                    plain[i, r, c, had] = all_slots(pad(cur[i, r, c]), pad(ref[i, r]), pred, use_lam, had, bd, False)
                    plain_meta[i, r, c, had] = (lq if use_lam else 0, pred[0], pred[1])
        print("refine", bd, "moved slots", int((plain[i, ..., :2] != 0).any(axis=-1).sum()), "of", 16 * 593)
    d.update(ref=ref, cur=cur, plain=plain, plain_meta=plain_meta)
    bi_bds = (8, 10)
    bi, bi_meta = np.zeros((2, 4, 2, 593, 3), np.int32), np.zeros((2, 4, 2, 3), np.int64)
    bi_cur, bi_other = np.zeros((2, 64, 64), np.int16), np.zeros((2, 64, 64), np.int16)
    for j, bd in enumerate(bi_bds):
        i, maxv = bds.index(bd), (1 << bd) - 1
        bi_cur[j], bi_other[j] = ref[i, 0], maxv - ref[i, 0]
        org = (2 * pad(bi_cur[j]).astype(np.int32) - pad(bi_other[j])).astype(np.int16)
        assert org.max() == 2 * maxv and org.min() == -maxv
        for r in range(4):
            for had in range(2):
                use_lam, pred = setting(r + had + 1, r)
                bi[j, r, had] = all_slots(org, pad(ref[i, r]), pred, use_lam, had, bd, True)
                bi_meta[j, r, had] = (lq if use_lam else 0, pred[0], pred[1])
    d.update(bi_bds=np.array(bi_bds), bi=bi, bi_meta=bi_meta, bi_cur=bi_cur, bi_other=bi_other)
    # the origin form of the prediction: 2 * cur - P with P the reference's own recorded block
    origin_bds = (8, 9, 10, 11)
    cases = [(3 + n, n >> 1) for n in range(32)]                 # (content, phase) of the tap-sign pictures of ref_blocks.npz
    slots = []
    for n in range(rt.PER_PICTURE):
        x, y = rt.slot_xy(n)
        slots.append(int(np.flatnonzero((table == (x, y, 8, 8)).all(axis=1))[0]))
    o_cur, o_ref = np.zeros((4, 64, 64), np.int16), np.zeros((4, 64, 64), np.int16)
    origin = np.zeros((4, 32, 3), np.int32)
    for j, bd in enumerate(origin_bds):
        i, maxv = BDS.index(bd), (1 << bd) - 1
        o_cur[j], o_ref[j] = rng.integers(0, maxv + 1, (64, 64)), rng.integers(0, maxv + 1, (64, 64))
        for g in range(0, 32, rt.PER_PICTURE):
            group = cases[g:g + rt.PER_PICTURE]
            P = rt.picture("luma", [rt.source("luma", i, c) for c, _ in group], (1 << bd) >> 1)
            for n, (c, ph) in enumerate(group):
                x, y = rt.slot_xy(n)
                P[y:y + 8, x:x + 8] = rt.block("luma", i, c, ph, 0)
            org = pad(2 * o_cur[j].astype(np.int64) - P)
            for n in range(len(group)):
                x, y = rt.slot_xy(n)
                hx, hy, qx, qy, cost = O.frac_refine(org, (m + x, m + y), pad(o_ref[j]), (m + x, m + y), 8, 8, (0, 0), (0, 0), lam, 1, bd, use_ref=True, bi=True)
                origin[j, g + n] = (2 * hx + qx, 2 * hy + qy, cost)
    d.update(origin_bds=np.array(origin_bds), origin_cur=o_cur, origin_ref=o_ref, origin_slots=np.array(slots), origin=origin)
    save("ref_refine.npz", d)


def main():
    what = sys.argv[1:] or ["blocks", "tails", "wp", "dist", "refine"]
    for name in what:
        {"blocks": gen_blocks, "tails": gen_tails, "wp": gen_wp, "dist": gen_dist, "refine": gen_refine}[name]()


if __name__ == "__main__":
    sys.exit(main())
