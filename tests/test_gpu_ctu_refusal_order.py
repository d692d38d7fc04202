"""Which refusal wins when a per-CTU call has two faults at once: each of the six entries (hmme_search_ctu, hmme_search_ctu_w,
hmme_search_refine_ctu, hmme_search_refine_ctu_w, hmme_refine_ctu, hmme_refine_ctu_w) is called through raw ctypes with every fault it can
have and with every pair of them (tests/ctu_refusal_cases.py).  It returns the code of the fault that ORDER puts first, says so in
hmme_last_error with a fragment of that fault's message, and leaves the caller's sentinel-filled output arrays alone.  No kernel runs:
every call is refused on the host.

Every array holds the widest staged window any case names (131 + 63 + 8 samples square), so a call that a wrong table lets through reads
inside its arrays and shows as a failed assertion.  The whole file takes a couple of seconds, nearly all of it the engine's start."""
import ctypes as C

import numpy as np
import pytest

import ctu_refusal_cases as crc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5C5C


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, crc.SR_MAX)
    yield e
    e.close()


def call_entry(L, api, h, entry, c, outs, int_mv):
    """one raw call of `entry` for the case c (ctu_refusal_cases.case) -> return code"""
    weighted, searches, refines = crc.ENTRIES[entry]
    cur = np.full((64, 64), c["cur"][0], np.int16)
    cur[63, 63] = c["cur"][1]
    ref = np.full((crc.SIDE, crc.SIDE), c["ref"][0], np.int16)
    ref[crc.ORIGIN, crc.ORIGIN] = c["ref"][1]
    ref0 = ref.ctypes.data + 2 * (crc.ORIGIN * crc.SIDE + crc.ORIGIN)
    p = api.SearchParams(*c["window"], c["pred_x"], 0, 1, c["bit_depth"], c["shift_free"])
    ptr = [o.ctypes.data for o in outs]
    if not searches:
        ptr = ptr[2:]
    elif not refines:
        ptr = ptr[:2]
    if c["null_out"]:
        ptr[-1] = None
    args = [h, cur.ctypes.data, 64, ref0, crc.SIDE, C.byref(p)]
    if weighted:
        args.append(None if c["null_weight"] else C.byref(api.Weight(*c["weight"])))
    if not searches:
        args.append(int_mv.ctypes.data)
    if refines:
        args.append(1)
    return getattr(L, entry)(*args, *ptr)


def test_one_and_two_faults_code_fragment_and_nothing_written(engine):
    from hmme import api
    L = api.load()
    outs = [np.full((593, 2), SENTINEL, np.int16), np.full(593, SENTINEL, np.uint32), np.full((593, 2), SENTINEL, np.int16), np.full(593, SENTINEL, np.uint32)]
    int_mv = np.zeros((593, 2), np.int16)
    prev = L.hmme_set_error_printing(engine.h, 0)
    n_calls = 0
    try:
        for entry in crc.ENTRIES:
            for faults in [(f,) for f in crc.faults_of(entry)] + crc.pairs_of(entry):
                first = min(faults, key=crc.ORDER.index)
                rc = call_entry(L, api, engine.h, entry, crc.case(entry, faults), outs, int_mv)
                msg = L.hmme_last_error(engine.h)
                assert rc == crc.CODE[first], (entry, faults, first, rc, msg)
                assert all(f in msg for f in crc.FRAGMENT[first]), (entry, faults, first, msg)
                assert all((o == SENTINEL).all() for o in outs), (entry, faults)
                n_calls += 1
    finally:
        L.hmme_set_error_printing(engine.h, prev)
    # plain entries: 7 faults, 21 pairs.  Weighted search: 11 faults, 55 pairs less the 3 a null weight cannot share.  Weighted refinement:
    # 12 faults, 66 pairs less those 4 and the Hadamard / shift-free one
    assert n_calls == 3 * (7 + 21) + (11 + 52) + 2 * (12 + 61)
