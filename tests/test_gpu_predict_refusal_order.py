"""Which refusal wins when a predict call has two faults at once: every public hmme_predict_* entry (luma and chroma, device and _frame
forms) is called with every pair of the faults it can have.  It returns the code of the fault that its order (ORDER) puts first, says so in
hmme_last_error -- the entry's name and a fragment of that fault's message --, and leaves the caller's images alone.  No kernel runs: the
device forms get addresses that are never dereferenced, so for them "nothing written" cannot be observed here, only that they refuse; the
_frame forms' sentinel-filled images are compared after every call.

The faults: one weight the range check refuses (HMME_ERR_UNSUPPORTED) and the argument errors (HMME_ERR_ARG) a null motion field, 256 MVs
per CTU (these two are one check: no order between them), an output pitch below a row, a plane of another size, unequal shifts of a bi
pair and a count of 0.  hmme_bipred_check refuses no bit depth in 8..12 for a prediction (asserted below), so there is no second
HMME_ERR_UNSUPPORTED cause.  An entry that takes no weight has argument errors only.

The orders were recorded from the library before the entries came to share their bodies, and are what they keep.  The whole file takes
about two seconds, nearly all of it the engine's start."""
import ctypes as C
import itertools

import numpy as np
import pytest

import predict_bi_w_model as pbw

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = pbw.ERR_ARG, pbw.ERR_UNSUPPORTED
W, H = 64, 64                                                # luma; chroma 32 x 32; 8 bit
N0, NF, P256, PITCH, SIZE, SHIFT, WEIGHT = "count 0", "null field", "256 MVs per CTU", "pitch below a row", "plane of another size", "unequal shifts", "refused weight"
GOOD, SHIFT5, HUGE = (70, 9, 6, 32), (35, 9, 5, 16), (1 << 20, 0, 6, 32)
DUMMY = 256                                                  # a device address that is never dereferenced
SENTINEL = 0x5C

# which fault answers, first to last.  The _frame forms for chroma check their arguments and sizes before a weight, everything else after it.
UNI = (N0, WEIGHT, NF, P256, PITCH, SIZE)
BI = (N0, SHIFT, WEIGHT, NF, P256, PITCH, SIZE)
ORDER = {
    "hmme_predict_pairs_device": UNI, "hmme_predict_pairs_w_device": UNI, "hmme_predict_frame": UNI, "hmme_predict_frame_w": UNI,
    "hmme_predict_refs_device": UNI, "hmme_predict_refs_w_device": UNI, "hmme_predict_refs_frame": UNI, "hmme_predict_refs_w_frame": UNI,
    "hmme_predict_bi_device": BI, "hmme_predict_bi_w_device": BI, "hmme_predict_bi_frame": BI, "hmme_predict_bi_w_frame": BI,
    "hmme_predict_chroma_pairs_device": UNI, "hmme_predict_chroma_refs_device": UNI, "hmme_predict_chroma_bi_device": BI,
    "hmme_predict_chroma_frame": (NF, P256, SIZE, WEIGHT, PITCH),
    "hmme_predict_chroma_refs_frame": (N0, NF, P256, SIZE, WEIGHT, PITCH),
    "hmme_predict_chroma_bi_frame": BI,                        # the plane of another size is list 1's here: found at the launch, like luma's
}
# what the message of the fault that answers contains (a luma plane of another size never answers in a pair: it is found last)
FRAGMENT = {N0: b"outside 1..", NF: b"MVs per CTU", P256: b"MVs per CTU", PITCH: b"below", SIZE: b"the chroma of a", SHIFT: b"shifts 6 and 5", WEIGHT: b"beyond 32 bits"}


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    yield e
    e.close()


def build_entries(L, engine, planes, images):
    """name -> (the faults the entry can have, call(faults) -> return code)"""
    from hmme import api
    y0, y1, cb0, cr0, cb1, cr1 = planes
    luma_img, cb_img, cr_img = images
    fp = api.FrameParams(1, 0, 8, 0, -1)
    field = np.zeros((2, 1, 64, 2), np.int16)
    dirs, ref_field = np.full((1, 64), 3, np.uint8), np.zeros((1, 64), np.uint8)
    hs = lambda ps: (C.c_void_p * len(ps))(*[p.h for p in ps])
    wa = lambda ws: (api.Weight * len(ws))(*[api.Weight(*w) for w in ws])
    ptrs = lambda n: (C.c_void_p * n)(*([DUMMY] * n))
    couts = (C.c_void_p * 2)(cb_img.ctypes.data, cr_img.ctypes.data)
    h, fpr = engine.h, C.byref(fp)
    per = lambda f: 256 if P256 in f else 64
    heavy = lambda f: HUGE if WEIGHT in f else GOOD
    skew = lambda f: SHIFT5 if SHIFT in f else GOOD
    d_field = lambda f: None if NF in f else DUMMY
    h_field = lambda f: None if NF in f else field.ctypes.data
    pitch = lambda f, w: w - (1 if PITCH in f else 0)        # 8-bit samples: bytes and samples alike
    luma2 = lambda f: hs([y0, cb0 if SIZE in f else y1])
    chroma2 = lambda f: hs([cb0, y0 if SIZE in f else cr0])
    chroma4 = lambda f: hs([cb0, cr0, cb1, y0 if SIZE in f else cr1])
    second = lambda f: hs([cb1, y0 if SIZE in f else cr1])
    dev, frame, bi = {N0, NF, P256, PITCH, SIZE}, {NF, P256, PITCH, SIZE}, {WEIGHT, SHIFT}
    E = {}
    # one picture per plane (or plane pair)
    E["hmme_predict_pairs_device"] = (dev, lambda f: L.hmme_predict_pairs_device(h, luma2(f), 0 if N0 in f else 2, fpr, d_field(f), per(f), ptrs(2), pitch(f, W), None))
    E["hmme_predict_pairs_w_device"] = (dev | {WEIGHT}, lambda f: L.hmme_predict_pairs_w_device(h, luma2(f), 0 if N0 in f else 2, fpr, wa([GOOD, heavy(f)]), d_field(f), per(f),
                                                                                                    ptrs(2), pitch(f, W), None))
    E["hmme_predict_frame"] = (frame - {SIZE}, lambda f: L.hmme_predict_frame(h, y0.h, fpr, h_field(f), per(f), luma_img.ctypes.data, pitch(f, W)))
    E["hmme_predict_frame_w"] = (frame - {SIZE} | {WEIGHT}, lambda f: L.hmme_predict_frame_w(h, y0.h, fpr, wa([heavy(f)]), h_field(f), per(f), luma_img.ctypes.data, pitch(f, W)))
    E["hmme_predict_chroma_pairs_device"] = (dev | {WEIGHT}, lambda f: L.hmme_predict_chroma_pairs_device(h, chroma2(f), 0 if N0 in f else 1, W, H, fpr, wa([GOOD, heavy(f)]),
                                                                                                              d_field(f), per(f), ptrs(2), pitch(f, W // 2), None))
    E["hmme_predict_chroma_frame"] = (frame | {WEIGHT}, lambda f: L.hmme_predict_chroma_frame(h, chroma2(f), W, H, fpr, wa([GOOD, heavy(f)]), h_field(f), per(f), couts,
                                                                                                pitch(f, W // 2)))
    # a reference index per block
    E["hmme_predict_refs_device"] = (dev, lambda f: L.hmme_predict_refs_device(h, luma2(f), 0 if N0 in f else 2, fpr, d_field(f), DUMMY, per(f), DUMMY, pitch(f, W), None))
    E["hmme_predict_refs_w_device"] = (dev | {WEIGHT}, lambda f: L.hmme_predict_refs_w_device(h, luma2(f), 0 if N0 in f else 2, fpr, wa([GOOD, heavy(f)]), d_field(f), DUMMY,
                                                                                                  per(f), DUMMY, pitch(f, W), None))
    E["hmme_predict_refs_frame"] = (dev, lambda f: L.hmme_predict_refs_frame(h, luma2(f), 0 if N0 in f else 2, fpr, h_field(f), ref_field.ctypes.data, per(f),
                                                                               luma_img.ctypes.data, pitch(f, W)))
    E["hmme_predict_refs_w_frame"] = (dev | {WEIGHT}, lambda f: L.hmme_predict_refs_w_frame(h, luma2(f), 0 if N0 in f else 2, fpr, wa([GOOD, heavy(f)]), h_field(f),
                                                                                                ref_field.ctypes.data, per(f), luma_img.ctypes.data, pitch(f, W)))
    E["hmme_predict_chroma_refs_device"] = (dev | {WEIGHT}, lambda f: L.hmme_predict_chroma_refs_device(h, chroma4(f), 0 if N0 in f else 2, W, H, fpr,
                                                                                                            wa([GOOD, GOOD, GOOD, heavy(f)]), d_field(f), DUMMY, per(f), DUMMY, DUMMY,
                                                                                                            pitch(f, W // 2), None))
    E["hmme_predict_chroma_refs_frame"] = (dev | {WEIGHT}, lambda f: L.hmme_predict_chroma_refs_frame(h, chroma4(f), 0 if N0 in f else 2, W, H, fpr,
                                                                                                          wa([GOOD, GOOD, GOOD, heavy(f)]), h_field(f), ref_field.ctypes.data, per(f),
                                                                                                          couts, pitch(f, W // 2)))
    # L0, L1 or bi per block: the refused weight and the unequal shift sit in the same pair of weights
    E["hmme_predict_bi_device"] = (dev, lambda f: L.hmme_predict_bi_device(h, hs([y0]), hs([cb0 if SIZE in f else y1]), 0 if N0 in f else 1, fpr, d_field(f), DUMMY, per(f),
                                                                             ptrs(1), pitch(f, W), None))
    E["hmme_predict_bi_w_device"] = (dev | bi, lambda f: L.hmme_predict_bi_w_device(h, hs([y0]), hs([cb0 if SIZE in f else y1]), 0 if N0 in f else 1, fpr, wa([heavy(f)]),
                                                                                      wa([skew(f)]), d_field(f), DUMMY, per(f), ptrs(1), pitch(f, W), None))
    E["hmme_predict_bi_frame"] = (frame, lambda f: L.hmme_predict_bi_frame(h, y0.h, (cb0 if SIZE in f else y1).h, fpr, h_field(f), dirs.ctypes.data, per(f),
                                                                             luma_img.ctypes.data, pitch(f, W)))
    E["hmme_predict_bi_w_frame"] = (frame | bi, lambda f: L.hmme_predict_bi_w_frame(h, y0.h, (cb0 if SIZE in f else y1).h, fpr, wa([heavy(f)]), wa([skew(f)]), h_field(f),
                                                                                      dirs.ctypes.data, per(f), luma_img.ctypes.data, pitch(f, W)))
    E["hmme_predict_chroma_bi_device"] = (dev | bi, lambda f: L.hmme_predict_chroma_bi_device(h, hs([cb0, cr0]), second(f), 0 if N0 in f else 1, W, H, fpr,
                                                                                                wa([heavy(f), GOOD]), wa([skew(f), GOOD]), d_field(f), DUMMY, per(f), ptrs(2),
                                                                                                pitch(f, W // 2), None))
    E["hmme_predict_chroma_bi_frame"] = (frame | bi, lambda f: L.hmme_predict_chroma_bi_frame(h, hs([cb0, cr0]), second(f), W, H, fpr, wa([heavy(f), GOOD]),
                                                                                                wa([skew(f), GOOD]), h_field(f), dirs.ctypes.data, per(f), couts, pitch(f, W // 2)))
    return E


def test_two_faults_code_name_and_nothing_written(engine):
    from hmme import api
    L = api.load()
    assert all(L.hmme_bipred_check(bd, 0) == 0 for bd in range(8, 13))          # no bit depth in 8..12 is refused: the weight is the one UNSUPPORTED cause
    planes = [engine.plane(W, H), engine.plane(W, H)] + [engine.plane(W // 2, H // 2) for _ in range(4)]
    images = [np.full((H, W), SENTINEL, np.uint8)] + [np.full((H // 2, W // 2), SENTINEL, np.uint8) for _ in range(2)]
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        entries = build_entries(L, engine, planes, images)
        assert len(entries) == 18 and set(ORDER) == set(entries)
        n_pairs = 0
        for entry, (faults, call) in entries.items():
            assert faults <= set(ORDER[entry])
            for pair in itertools.combinations(sorted(faults), 2):
                first = min(pair, key=ORDER[entry].index)
                want = ERR_UNSUPPORTED if first == WEIGHT else ERR_ARG
                rc, msg = call(set(pair)), L.hmme_last_error(engine.h)
                assert rc == want, (entry, pair, rc, want, msg)
                assert entry.encode() in msg and FRAGMENT[first] in msg, (entry, pair, first, msg)
                assert all((i == SENTINEL).all() for i in images), (entry, pair)
                n_pairs += 1
        assert n_pairs == 4 * 10 + 6 * 15 + 3 + 6 + 10 + 2 * 21 + 6 + 2 * 15             # every entry met every pair of its faults: 227
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in planes:
            p.close()
