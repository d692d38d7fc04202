"""What the eight selection calls (hmme_select_pairs_device / _frame, hmme_select_refs_*, hmme_select_dirs_*, hmme_select_dirs_refs_*) say
when they refuse: one refusal per layer of their checks -- hmme_select_params, the family's own parameters, the CTU range and, for the device
entries, a missing and a misaligned buffer -- each through the raw C entry.  Three things per refusal: the status code, the entry the message
names, and that no byte of any output changed.  The message of a parameter or buffer refusal begins with the entry that was CALLED (a *_frame
call never answers in the name of the *_device entry it runs on); a CTU range outside the picture is refused by the check every call family
shares, whose message ("CTU range [first, +count) outside 0..n") names no entry.  Every call here is refused, so the inputs are never read:
they are zeros, and all cases share them.  What the calls compute is the matter of tests/test_gpu_select*.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FILL = 0xA5                      # every output byte, before and after
IN_BYTES, OUT_BYTES = 1 << 17, 1 << 15   # above the largest input (2 lists x 2 references x 8 CTUs of tables) and output (2 x 6 CTUs x 64 MVs)

INS = ("mv_uni", "cost_uni", "mv_bi", "cost_bi", "uni_field", "uni_ref", "pred")
OUTS = ("field", "ref", "dir", "slot", "cc")


class Entry:
    """one C entry: the integers between (ctx, width, height) and fp, its family parameters, and its buffers in the order of the signature"""

    def __init__(self, name, lead, family, ins, outs):
        self.name, self.lead, self.family, self.ins, self.outs = name, lead, family, ins, outs
        self.device = name.endswith("_device")


E = {e.name: e for e in (
    Entry("hmme_select_pairs_device", ("n_pics",), None, ("mv_uni", "cost_uni", "pred"), ("field", "slot", "cc")),
    Entry("hmme_select_frame", (), None, ("mv_uni", "cost_uni", "pred"), ("field", "slot", "cc")),
    Entry("hmme_select_refs_device", ("n_pics", "n_refs"), "ref_cost", ("mv_uni", "cost_uni", "pred"), ("field", "ref", "slot", "cc")),
    Entry("hmme_select_refs_frame", ("n_refs",), "ref_cost", ("mv_uni", "cost_uni", "pred"), ("field", "ref", "slot", "cc")),
    Entry("hmme_select_dirs_device", ("n_pics",), "dirs", ("mv_uni", "cost_uni", "mv_bi", "cost_bi", "uni_field", "pred"), ("field", "dir", "slot", "cc")),
    Entry("hmme_select_dirs_frame", (), "dirs", ("mv_uni", "cost_uni", "mv_bi", "cost_bi", "uni_field", "pred"), ("field", "dir", "slot", "cc")),
    Entry("hmme_select_dirs_refs_device", ("n_pics", "n_refs"), "dirs_refs", INS, OUTS),
    Entry("hmme_select_dirs_refs_frame", ("n_refs",), "dirs_refs", INS, OUTS),
)}

BIG = dict(w=136, h=72)          # 3 x 2 CTUs, the right column and the bottom row partial
RANGES = (("past_one_ctu", dict(first=0, count=2)), ("end_past_picture", dict(BIG, first=4, count=3)), ("first_below_zero", dict(BIG, first=-1, count=1)))


def cases():
    out = []
    for e in E.values():
        add = lambda layer, names, **kw: out.append(pytest.param(e.name, names, kw, id=f"{e.name[5:]}-{layer}"))
        add("select_params", e.name, sel=dict(mv_per_ctu=65))
        if e.family is None and e.device:
            add("no_pairs", e.name, n_pics=0)
        if e.family == "ref_cost":
            add("no_references", e.name, n_refs=0)
            # two faults at once: these two entries look at the reference buffer before the parameters
            add("select_params_and_no_ref", e.name, sel=dict(mv_per_ctu=65), null="ref", says="reference")
        if e.family == "dirs":
            add("dir_bits", e.name, dirs=dict(dir_bits=(4097, 0, 0)))
        if e.family == "dirs_refs":
            add("nine_table_sets", e.name, n_refs=9)
            add("mask_at_n_refs", e.name, dirs=dict(n_refs=(2, 2), l1_valid_mask=0b100))
        for layer, kw in RANGES:
            add(layer, "CTU range", **kw)
        if e.device:
            required = {"hmme_select_pairs_device": ("mv_uni", "field"), "hmme_select_refs_device": ("ref", "cost_uni"),
                        "hmme_select_dirs_device": ("mv_bi", "dir", "field"), "hmme_select_dirs_refs_device": ("uni_ref", "ref", "mv_uni")}[e.name]
            odd = {"hmme_select_pairs_device": (("field", 4), ("pred", 1)), "hmme_select_refs_device": (("ref", 1), ("mv_uni", 2)),
                   "hmme_select_dirs_device": (("dir", 1), ("cost_bi", 2), ("slot", 2)),
                   "hmme_select_dirs_refs_device": (("uni_field", 2), ("cc", 2), ("pred", 1))}[e.name]
            for b in required:
                add(f"no_{b}", e.name, null=b)
            for b, off in odd:
                add(f"odd_{b}", e.name, odd=(b, off))
    return out


@pytest.fixture(scope="module")
def engine(buffers):   # (after the buffers: torch's runtime comes up before the first context, as tests/conftest.py has it)
    from hmme import api
    e = api.Engine(0, 64)
    prev = e.L.hmme_set_error_printing(e.h, 0)
    yield e
    e.L.hmme_set_error_printing(e.h, prev)
    e.close()


@pytest.fixture(scope="module")
def buffers():
    """{True: device, False: host} -> ({input: address}, {output: address}, the outputs themselves, as things with .all())"""
    import torch
    dev = torch.device("cuda", 0)
    d_in = {n: torch.zeros(IN_BYTES, dtype=torch.uint8, device=dev) for n in INS}
    d_out = {n: torch.full((OUT_BYTES,), FILL, dtype=torch.uint8, device=dev) for n in OUTS}
    h_in = {n: np.zeros(IN_BYTES, np.uint8) for n in INS}
    h_out = {n: np.full(OUT_BYTES, FILL, np.uint8) for n in OUTS}
    torch.cuda.synchronize()
    return {True: ({n: t.data_ptr() for n, t in d_in.items()}, {n: t.data_ptr() for n, t in d_out.items()}, d_out, d_in),
            False: ({n: a.ctypes.data for n, a in h_in.items()}, {n: a.ctypes.data for n, a in h_out.items()}, h_out, h_in)}


@pytest.mark.parametrize("name, names, kw", cases())
def test_a_refusal_names_its_entry_and_writes_nothing(engine, buffers, name, names, kw):
    import torch
    from hmme import api
    e, L = E[name], engine.L
    ins, outs, out_arrays, _ = buffers[e.device]
    ptr = dict(ins, **outs)
    if "null" in kw:
        ptr[kw["null"]] = None
    if "odd" in kw:
        ptr[kw["odd"][0]] += kw["odd"][1]
    fp = api.FrameParams(1, 0, 8, kw.get("first", 0), kw.get("count", 1))
    sel = api.SelectParams(**kw.get("sel", {}))
    lead = dict(n_pics=kw.get("n_pics", 1), n_refs=kw.get("n_refs", 2))
    family = {None: lambda: [], "ref_cost": lambda: [(C.c_uint32 * 16)()], "dirs": lambda: [(api.DirParams * 1)(api.DirParams(**kw.get("dirs", {})))],
              "dirs_refs": lambda: [(api.DirRefsParams * 1)(api.DirRefsParams(**kw.get("dirs", dict(n_refs=(2, 2)))))]}[e.family]()
    args = [engine.h, kw.get("w", 64), kw.get("h", 64)] + [lead[k] for k in e.lead] + [C.byref(fp), C.byref(sel)] + family
    args += [ptr[b] for b in e.ins] + [ptr[b] for b in e.outs] + ([None] if e.device else [])
    rc = getattr(L, name)(*args)
    msg = L.hmme_last_error(engine.h).decode()
    print(f"{name} -> {rc}: {msg}")
    assert rc == ERR_ARG
    assert msg.startswith(names + (":" if names == name else " ")), msg
    assert kw.get("says", "") in msg, msg
    torch.cuda.synchronize()
    for b in e.outs:
        assert bool((out_arrays[b] == FILL).all()), b
