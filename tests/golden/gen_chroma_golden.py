#!/usr/bin/env python3
"""Generate tests/golden/chroma_mc.npz from the COMPILED REFERENCE (oracle/_ref/libhmref.so, built by oracle/Makefile).

Run where the reference library was built:   python tests/golden/gen_chroma_golden.py
The file holds inputs and the reference's outputs -- data only.

Blocks come from the reference's own TComInterpolationFilter::filterHor / filterVer with component Cb and format 4:2:0, combined exactly
as the three branches of TComPrediction::xPredInterBlk combine them (TLibCommon/TComPrediction.cpp:689-706).  The class has no data
members, so the two methods are called through ctypes by their mangled names with a dummy `this`.

  bds      [4]                       8, 9, 10, 12
  src4     [4, 3, 7, 7]      int16   per bit depth: random, binary-extreme ({0, maxv}) and all-maximum content around a 4x4 block
  out4     [4, 3, 64, 2, 4, 4] int16 ... at every phase pair 8 * yFrac + xFrac, uni (bi = false) and bi (bi = true) end
  src2 / out2 / at2    a 2x2 block: source [5, 5], outputs [2, 2, 2] (uni, bi), at2 = (bit depth, xFrac, yFrac)
  src32 / out32 / at32 a 32x32 block: source [35, 35], outputs [2, 32, 32], at32 likewise
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libhmref.so")
OUT = os.path.join(HERE, "chroma_mc.npz")

BDS = (8, 9, 10, 12)
COMPONENT_CB, CHROMA_420 = 1, 1
FILTER_HOR = "_ZN23TComInterpolationFilter9filterHorE11ComponentIDPsiS1_iiiib12ChromaFormati"
FILTER_VER = "_ZN23TComInterpolationFilter9filterVerE11ComponentIDPsiS1_iiiibb12ChromaFormati"
TMP_STRIDE = 64

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(REF_LIB)
        p16, i, b = C.POINTER(C.c_int16), C.c_int, C.c_bool
        hor, ver = getattr(L, FILTER_HOR), getattr(L, FILTER_VER)
        hor.restype = ver.restype = None
        hor.argtypes = [C.c_void_p, i, p16, i, p16, i, i, i, i, b, i, i]         # this, compID, src, stride, dst, stride, w, h, frac, isLast, fmt, bd
        ver.argtypes = [C.c_void_p, i, p16, i, p16, i, i, i, i, b, b, i, i]      # ... frac, isFirst, isLast, fmt, bd
        _lib = (hor, ver, C.create_string_buffer(64))
    return _lib


def ref_block(src, n, x_frac, y_frac, bd, bi):
    """the n x n chroma block whose top-left sample is src[1, 1] (src: int16 [n + 3, n + 3]), as xPredInterBlk makes it -> int16 [n, n]"""
    hor, ver, this = lib()
    src = np.ascontiguousarray(src, np.int16)
    assert src.shape == (n + 3, n + 3)
    stride = src.shape[1]
    p16 = C.POINTER(C.c_int16)
    at = lambda a, row, col, s: C.cast(a.ctypes.data + 2 * (row * s + col), p16)
    dst = np.zeros((n, n), np.int16)
    if y_frac == 0:
        hor(this, COMPONENT_CB, at(src, 1, 1, stride), stride, at(dst, 0, 0, n), n, n, n, x_frac, not bi, CHROMA_420, bd)
    elif x_frac == 0:
        ver(this, COMPONENT_CB, at(src, 1, 1, stride), stride, at(dst, 0, 0, n), n, n, n, y_frac, True, not bi, CHROMA_420, bd)
    else:
        tmp = np.zeros((n + 3, TMP_STRIDE), np.int16)
        hor(this, COMPONENT_CB, at(src, 0, 1, stride), stride, at(tmp, 0, 0, TMP_STRIDE), TMP_STRIDE, n, n + 3, x_frac, False, CHROMA_420, bd)
        ver(this, COMPONENT_CB, at(tmp, 1, 0, TMP_STRIDE), TMP_STRIDE, at(dst, 0, 0, n), n, n, n, y_frac, False, not bi, CHROMA_420, bd)
    return dst


def contents(rng, n, bd):
    maxv = (1 << bd) - 1
    return np.stack([rng.integers(0, maxv + 1, size=(n + 3, n + 3)), np.where(rng.integers(0, 2, size=(n + 3, n + 3)) == 1, maxv, 0),
                     np.full((n + 3, n + 3), maxv)]).astype(np.int16)


def main():
    rng = np.random.default_rng(420)
    src4 = np.stack([contents(rng, 4, bd) for bd in BDS])
    out4 = np.zeros((len(BDS), 3, 64, 2, 4, 4), np.int16)
    for i, bd in enumerate(BDS):
        for c in range(3):
            for ph in range(64):
                for bi in range(2):
                    out4[i, c, ph, bi] = ref_block(src4[i, c], 4, ph & 7, ph >> 3, bd, bool(bi))
    d = dict(bds=np.array(BDS), src4=src4, out4=out4)
    for n, at in ((2, (8, 3, 5)), (32, (10, 5, 2))):
        src = contents(rng, n, at[0])[0]
        d[f"src{n}"], d[f"at{n}"] = src, np.array(at)
        d[f"out{n}"] = np.stack([ref_block(src, n, at[1], at[2], at[0], bool(bi)) for bi in range(2)])
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
