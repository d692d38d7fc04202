"""The faults a per-CTU call (hmme_search_ctu, hmme_search_ctu_w, hmme_search_refine_ctu, hmme_search_refine_ctu_w, hmme_refine_ctu,
hmme_refine_ctu_w) can be refused for, the order in which they answer when two are present at once (ORDER), and a fragment of each one's
message.  No GPU import: tests/test_gpu_ctu_refusal_order.py makes arrays and calls from `case`, tests/test_ctu_plan_cpu.py gives the
same cases to hmme_test_ctu_plan as ranges.

TEncOpenCL::calcMotionVectors latches a sample width and retries on HMME_ERR_RANGE alone, so a call that is both out of range and beyond
the cost field has to keep answering HMME_ERR_RANGE: the order is part of the boundary.  It was recorded from the library while the
per-CTU body was still one function, and is what the split keeps."""
ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -3, -5

NULLW, SHIFT16, NULLOUT, BD13, PRED, CUR, WIN, REF, PEL, COST, HAD, SF = (
    "null weight", "weight shift 16", "null output", "bit depth 13", "pred_x 40000", "current sample 2 maxv + 1", "window 131 wide at sr_max 64",
    "reference sample maxv + 1", "weight beyond a Pel", "weighted span beyond the cost field", "weighted span beyond the Hadamard sums",
    "shift-free span beyond the cost field")

# which fault answers, first to last; the same for all six entries (an entry meets the faults it can have)
ORDER = (NULLW, SHIFT16, NULLOUT, BD13, PRED, CUR, WIN, REF, PEL, COST, HAD, SF)
CODE = {NULLW: ERR_ARG, SHIFT16: ERR_ARG, NULLOUT: ERR_ARG, BD13: ERR_UNSUPPORTED, PRED: ERR_ARG, CUR: ERR_RANGE, WIN: ERR_ARG, REF: ERR_RANGE,
        PEL: ERR_UNSUPPORTED, COST: ERR_UNSUPPORTED, HAD: ERR_UNSUPPORTED, SF: ERR_UNSUPPORTED}
# every fragment is in the message of the fault that answers (the shift-free message speaks of the cost field as well: the first fragment
# of COST and of SF tells the two apart)
FRAGMENT = {NULLW: (b"null weight",), SHIFT16: (b"shift",), NULLOUT: (b"null argument",), BD13: (b"bit depth",), PRED: (b"int16",), CUR: (b"current-block",),
            WIN: (b"window",), REF: (b"reference sample",), PEL: (b"beyond a Pel",), COST: (b"weighted SADs", b"cost field"), HAD: (b"Hadamard",),
            SF: (b"shift-free", b"cost field")}

# name -> (weighted, searches, refines)
ENTRIES = {"hmme_search_ctu": (False, True, False), "hmme_search_ctu_w": (True, True, False), "hmme_search_refine_ctu": (False, True, True),
           "hmme_search_refine_ctu_w": (True, True, True), "hmme_refine_ctu": (False, False, True), "hmme_refine_ctu_w": (True, False, True)}

SR_MAX = 64           # of the one context: a window of 131 candidates is one too wide for it
SIDE = 131 + 63 + 8   # every array holds the widest staged window any case names
ORIGIN = 65 + 4       # the sample the window's candidate (0, 0) starts at, in both directions


def faults_of(entry):
    weighted, _, refines = ENTRIES[entry]
    f = [NULLOUT, BD13, PRED, CUR, WIN, REF, SF]
    if weighted:
        f += [NULLW, SHIFT16, PEL, COST]
        if refines:
            f.append(HAD)
    return sorted(f, key=ORDER.index)


def compatible(a, b):
    """whether one call can have both faults.  A null weight has no shift and no range.  The Hadamard bound (a span of 4096) lies above
    the cost field's shift-free bound (1938), so a shift-free call never reaches it."""
    pair = {a, b}
    if NULLW in pair and pair & {SHIFT16, PEL, COST, HAD}:
        return False
    return pair != {HAD, SF}


def pairs_of(entry):
    f = faults_of(entry)
    return [(a, b) for i, a in enumerate(f) for b in f[i + 1:] if compatible(a, b)]


def case(entry, faults):
    """the call of `entry` that has exactly these faults (and those a fault brings with it: a weight beyond a Pel is beyond the cost field
    as well) -> dict of bit_depth, shift_free, weight (None: the entry takes none, or NULLW), null_out, pred_x, window (lt_x, lt_y, rb_x,
    rb_y), cur (lo, hi) and ref (lo, hi): the extremes of the block and of the staged window, every other sample is lo"""
    weighted = ENTRIES[entry][0]
    faults = set(faults)
    assert faults <= set(faults_of(entry))
    deep = bool(faults & {HAD, SF})                  # these two are 12-bit faults; everything else is shown at 8 bit
    data_bd = 12 if deep else 8
    maxv = (1 << data_bd) - 1
    weight = None
    if weighted and NULLW not in faults:
        if PEL in faults:
            weight = (64, 33000, 6, 32)              # 33000 .. 33000 + maxv
        elif COST in faults:                         # a span of about 3000 >= 1938 at 8 bit and shift-free; 12 bit: about 32000 >= 30995, within a Pel
            weight = (64, 32000, 6, 32) if HAD in faults else (64, 3000, 6, 32)
        elif HAD in faults:
            weight = (64, 8000, 6, 32)               # 12 bit: a span of 8000 and more, >= 4096 and far below the cost field's 30995
        elif SF in faults:
            weight = (1, 15, 6, 32)                  # the weighted window stays next to the block: only the raw samples are far apart
        else:
            weight = (70, 9, 6, 32)
        if SHIFT16 in faults:
            weight = (weight[0], weight[1], 16, weight[3])
    cur, ref = [10, 20], [10, 20]
    if SF in faults:
        ref = [0, 4000]                              # 3990 from the block: >= 1938
    if CUR in faults:
        cur[1] = 2 * maxv + 1
    if REF in faults:
        ref[1] = maxv + 1
    return dict(bit_depth=13 if BD13 in faults else data_bd, shift_free=1 if SF in faults else 0, weight=weight, null_weight=NULLW in faults,
                null_out=NULLOUT in faults, pred_x=40000 if PRED in faults else 0, window=(-65, -2, 65, 2) if WIN in faults else (-2, -2, 2, 2),
                cur=tuple(cur), ref=tuple(ref))
