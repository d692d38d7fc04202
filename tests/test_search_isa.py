"""The built ISA of the benchmark's kernel, me_search_kernel<1, 0, 2>, counted with the logic of tools/isa_stats.py: its second-largest
basic block is one lane-iteration of the full-task body (me_tree_pk4_fen1.inc; the largest is the packed-minimum twin's).  The packed
subtracts must cost what the generator prices them at -- two v_sub_u32 each, no borrow chain, no masks of a shifted low half -- and
the body must stay below 4 900 VALU instructions (5 063 before the MV costs were carried in the sums).  Needs no GPU: hipcc
cross-compiles, and the build keeps the ISA beside the object it came from."""
import collections
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hm-opencl_amd", "csrc")
ISA = os.path.join(CSRC, "build", "hmme-hip-amdgcn-amd-amdhsa-gfx950.s")
KERNEL = "_ZN4hmme16me_search_kernelILi1ELi0ELi2E"


def blocks(kernel):
    """-> the kernel's basic blocks, largest first, each a Counter of opcodes"""
    s = open(ISA).read()
    m = re.search(r"^(%s[^\n:]*):" % re.escape(kernel), s, re.M)
    assert m, kernel
    body = s[m.end():s.index(".Lfunc_end", m.end())].split("\n")
    op = lambda l: l.strip().split(" ")[0] if l.strip() and not l.strip().startswith((";", ".")) else ""
    idx = [i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l)] + [len(body)]
    cut = sorted(((b - a, a, b) for a, b in zip([0] + idx[:-1], idx)), reverse=True)
    return [collections.Counter(op(l) for l in body[a:b] if op(l)) for n, a, b in cut]


@pytest.fixture(scope="module")
def isa():
    from hmme import api
    api.build()                # nothing to do where the library is up to date; the ISA is a by-product of the same compile
    return blocks(KERNEL)


def count(c, prefix):
    return sum(v for k, v in c.items() if k.startswith(prefix))


def test_full_task_body_pays_two_instructions_per_packed_subtract(isa):
    twin, full = isa[0], isa[1]
    assert count(full, "v_qsad_pk_u16_u8") == 1024 and count(full, "v_min_u16_sdwa") == 512, "the second-largest block is the full-task body"
    assert count(twin, "v_qsad_pk_u16_u8") == 1024 and count(twin, "v_min_u16_sdwa") == 0, "the largest is the packed-minimum twin"
    assert count(full, "v_subb_co_u32") == 0 and count(full, "v_subrev_co_u32") == 0
    assert count(full, "v_and_b32") <= 8
    assert count(full, "v_") <= 4900
    # 32 subtracts (12x16), two instructions each
    assert count(full, "v_sub_u32") == 64


def test_twin_body_pays_two_instructions_per_packed_subtract(isa):
    twin = isa[0]      # the block also holds the lane-iteration's prologue: the one 64-bit negation of the packed MV costs is its borrow pair
    assert count(twin, "v_subb_co_u32") <= 1 and count(twin, "v_subrev_co_u32") == 0 and count(twin, "v_and_b32") <= 8
    assert count(twin, "v_sub_u32") >= 64           # its 32 subtracts; the compiler may write further ones of its own in the _e32 form


def test_check_isa_passes(isa):
    r = subprocess.run(["make", "-s", "-C", CSRC, "check-isa"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
