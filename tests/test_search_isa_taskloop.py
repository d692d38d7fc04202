"""The task loop of the benchmark's kernel, me_search_kernel<1, 0, 2>, outside its two generated bodies, counted in the built ISA with
the block logic of tools/isa_stats.py: everything but the two largest basic blocks (the twin's lane-iteration and the full-task one).
A full task's lane-iteration has a prologue of its own, which the compiler puts into the body's block: one bit count (the row) and four
multiplies, no exec-mask diamond, no validity or marker select.  The running minima are flushed at two sites: ten
registers per task (a full task of a whole-job launch: two of them), and the eight packed ones a wave carried across full tasks -- one
slot-map load (global_load_ushort) and one 64-lane LDS ds_min_u64 per register and site.

Counts are STATIC: the parent commit had 2 889 instructions outside the bodies (1 031 VALU, 81 global loads of which 10 slot-map loads,
10 ds_min_u64, 38 v_writelane) and a full-task block of 6 660 / 4 848 VALU that held no prologue (about 150 instructions per
lane-iteration ran outside it); this build has 3 098 (1 183 VALU, 89 / 18, 18, 47) and 6 723 / 4 883.  The second flush site and the
per-task setup make the loop's code longer; what a wave EXECUTES per job of the 129 x 129 window falls from 20 tasks x 10 flush blocks to
17 x 2 + 3 x 10 + 8 per carried flush.  The bounds sit just above this build's counts.  Needs no GPU."""
import collections
import re

import pytest

import test_search_isa as I


def outside_and_bodies(kernel):
    """-> (Counter of the opcodes outside the two largest basic blocks, Counter of the largest, Counter of the second largest)"""
    s = open(I.ISA).read()
    m = re.search(r"^(%s[^\n:]*):" % re.escape(kernel), s, re.M)
    assert m, kernel
    body = s[m.end():s.index(".Lfunc_end", m.end())].split("\n")
    op = lambda l: l.strip().split(" ")[0] if l.strip() and not l.strip().startswith((";", ".")) else ""
    idx = [i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)] + [len(body)]
    cut = sorted(((b - a, a, b) for a, b in zip([0] + idx[:-1], idx)), reverse=True)
    inside = set(range(cut[0][1], cut[0][2])) | set(range(cut[1][1], cut[1][2]))
    rest = collections.Counter(op(l) for i, l in enumerate(body) if i not in inside and op(l))
    return (rest,) + tuple(collections.Counter(op(l) for l in body[a:b] if op(l)) for n, a, b in cut[:2])


@pytest.fixture(scope="module")
def isa():
    from hmme import api
    api.build()
    return outside_and_bodies(I.KERNEL)


def test_task_loop_outside_the_bodies(isa):
    rest, twin, full = isa
    print("outside the bodies:", sum(rest.values()), "instructions,", I.count(rest, "v_"), "VALU,", I.count(rest, "global_load"), "global loads,",
          rest["global_load_ushort"], "slot-map loads,", rest["ds_min_u64"], "ds_min_u64,", rest["v_writelane_b32"], "v_writelane")
    assert sum(rest.values()) <= 3110 and I.count(rest, "v_") <= 1190
    assert I.count(rest, "global_load") <= 89
    # two flush sites: ten registers per task, eight carried; nothing else takes a 64-bit LDS minimum or reads a slot map
    assert rest["global_load_ushort"] == 18 and rest["ds_min_u64"] == 18
    assert I.count(twin, "ds_min") == 0 and I.count(full, "ds_min") == 0 and I.count(twin, "global_") == 0 and I.count(full, "global_") == 0
    assert rest["v_writelane_b32"] <= 48


def test_full_task_prologue_is_the_lean_one(isa):
    rest, twin, full = isa
    assert I.count(full, "v_min_u16_sdwa") == 512 and I.count(twin, "v_min_u16_sdwa") == 0
    # in the body's block: the row's bit count and the four (lambda * bits) products; the x halves are the task's
    assert I.count(full, "v_ffbh_u32") == 1 and I.count(full, "v_mul_lo_u32") == 4 and I.count(full, "v_perm_b32") == 2
    assert I.count(full, "s_and_saveexec_b64") == 0, "no exec-mask diamond: the row's sign is a select"
    assert I.count(full, "v_") <= 4890 and sum(full.values()) <= 6730
    # the twin's prologue, outside both bodies as before, is the only other place that counts bits and multiplies per lane-iteration
    assert I.count(twin, "v_ffbh_u32") == 0 and I.count(twin, "v_mul_lo_u32") == 0


@pytest.mark.parametrize("split", [1, 2])
def test_split_kernels_keep_the_per_task_flush(split):
    rest, twin, full = outside_and_bodies("_ZN4hmme16me_search_kernelILi1ELi%dELi2E" % split)
    assert rest["global_load_ushort"] == 10 and rest["ds_min_u64"] == 10
    assert I.count(full, "v_min_u16_sdwa") == 512 and I.count(full, "v_mul_lo_u32") == 4 and I.count(full, "v_ffbh_u32") == 1
