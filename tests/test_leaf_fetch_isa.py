"""ISA check of the leaf loop's triangle fetch (CPU: hipcc cross-compiles gfx950 assembly).

The leaf test reads one 80-byte GTri per iteration with five 16-byte loads.  The compiler used to
sink the load that feeds only c4 = ro - p2 into the `fabs(S) >= 1e-10` branch, where it became a
sixth load and a second, dependent round trip per triangle test.  In each of the four production
kernels this test finds the innermost loop that fetches GTri records -- the one whose address
computation multiplies by the record stride, 80 -- and asserts that it holds exactly five
vector-memory loads, all of them ahead of the loop body's first conditional branch.
"""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import waitcnt_audit  # noqa: E402

VARIANTS = ["ILi4ELb0ELb0ELi8ELb0EE", "ILi4ELb0ELb0ELi16ELb0EE", "ILi4ELb0ELb0ELi8ELb1EE", "ILi4ELb0ELb0ELi16ELb1EE"]
STRIDE = 80   # sizeof(GTri)

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s*s_c?branch\w*\s+(\.LBB\d+_\d+)")
CBRANCH = re.compile(r"^\s*s_cbranch_")
VMEM_LOAD = re.compile(r"^\s*(global|flat|buffer|scratch)_load_")
MAD64 = re.compile(r"^\s*v_mad_u64_u32\s+(.*)$")
CONST_DEF = re.compile(r"^\s*(?:s_movk_i32|s_mov_b32|v_mov_b32_e32)\s+([sv]\d+),\s*(0x[0-9a-fA-F]+|\d+)\s*$")


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "rt_render.s"
    subprocess.run(["make", "-s", "-C", str(ROOT / "my-raytracer_amd"), "asm", f"ASM_OUT={out}"], check=True,
                   capture_output=True, timeout=900)
    return out


def stride_sites(body):
    """Indices of the 64-bit multiply-adds whose multiplier is the record stride: a literal, or a
    register that the closest constant move above it (within a few instructions) set to it."""
    sites = []
    for i, line in enumerate(body):
        m = MAD64.match(line)
        if not m:
            continue
        ops = [o.strip() for o in m.group(1).split(",")]
        # v_mad_u64_u32 vdst[2], sdst[2], src0, src1, src2: the register pairs contain a comma-free "v[a:b]"
        src = ops[2:4]
        hit = False
        for o in src:
            if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", o):
                hit = hit or int(o, 0) == STRIDE
            elif re.fullmatch(r"[sv]\d+", o):
                for j in range(i - 1, max(-1, i - 12), -1):
                    d = CONST_DEF.match(body[j])
                    if d and d.group(1) == o:
                        hit = hit or int(d.group(2), 0) == STRIDE
                        break
        if hit:
            sites.append(i)
    return sites


def innermost_loop(body, site):
    """(head, back): the smallest [label, backward branch to it] range that contains `site`."""
    labels = {}
    for i, line in enumerate(body):
        m = LABEL.match(line)
        if m:
            labels[m.group(1)] = i
    best = None
    for i, line in enumerate(body):
        m = BRANCH.match(line)
        if m and m.group(1) in labels and labels[m.group(1)] <= i:
            head = labels[m.group(1)]
            if head <= site <= i and (best is None or i - head < best[1] - best[0]):
                best = (head, i)
    return best


def leaf_fetch(body):
    """[(loads in the loop, loads behind its first conditional branch)] per GTri fetch loop."""
    out = []
    for site in stride_sites(body):
        loop = innermost_loop(body, site)
        assert loop is not None, f"the stride multiply at {site} is in no loop"
        head, back = loop
        loads = [i for i in range(head, back + 1) if VMEM_LOAD.match(body[i])]
        # the iteration starts at the block that computes the record's address (the compiler may lay
        # the loop's latch out above it); the body's first conditional branch is the first one below
        start = max(i for i in range(head, site + 1) if LABEL.match(body[i]))
        first_branch = next(i for i in range(site, back + 1) if CBRANCH.match(body[i]))
        out.append((len(loads), sum(1 for i in loads if not start <= i < first_branch)))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
def test_triangle_record_is_fetched_by_five_loads_before_the_first_branch(kernel_asm, variant):
    body = waitcnt_audit.kernel_lines(str(kernel_asm), variant)
    loops = leaf_fetch(body)
    print(variant, loops)
    assert len(loops) >= 1
    for n_loads, late in loops:
        assert n_loads == 5
        assert late == 0


def test_finder_sees_a_late_load():
    # the shape of the code before the pin: five loads up front, a sixth inside the first branch
    body = ["\ts_movk_i32 s2, 0x50", ".LBB0_1:", "\tv_mad_u64_u32 v[18:19], s[2:3], v121, s2, v[18:19]"]
    body += [f"\tglobal_load_dwordx4 v[{4 * k}:{4 * k + 3}], v[18:19], off offset:{16 * k}" for k in range(4)]
    body += ["\tglobal_load_dwordx2 v[20:21], v[18:19], off offset:72", "\ts_and_saveexec_b64 s[4:5], vcc",
             "\ts_cbranch_execz .LBB0_2", "\tglobal_load_dwordx4 v[30:33], v[18:19], off offset:56",
             "\ts_waitcnt vmcnt(0)", ".LBB0_2:", "\ts_or_b64 exec, exec, s[4:5]", "\ts_cbranch_vccnz .LBB0_1",
             "\ts_endpgm"]
    assert leaf_fetch(body) == [(6, 1)]
    del body[10]
    assert leaf_fetch(body) == [(5, 0)]
