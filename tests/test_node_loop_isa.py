"""ISA check of the 4-wide node loop's stack traffic (CPU: hipcc cross-compiles gfx950 assembly).

The kernel source is built three times: as it ships (the default RT_STACK_FAST: steps 1, 8 and 32),
with the three branch-free steps of the plan (-DRT_STACK_FAST=7: pushes of the sorted path, pushes of
any-hit waves, pops; 2 and 4 are switched off in the shipped build and stay guarded here), and with
the parent's algorithm (-DRT_STACK_FAST=0; "parent" below is this build, not the parent commit's
text).  In each of the four production kernels the node loop is the innermost natural loop around
the block that reads a treelet node with seven 16-byte LDS loads.

The shipped build.  Its sorted path is the part of the loop dominated by the block that the wave
enters when it is not a wave of any-hit rays (the nearest wave-uniformly entered block above the
sorting network's compares).  Inside it the capacity test is a wave-uniform branch; the blocks
dominated by the side of it that holds the spill stores are the slow pushes, the rest is what a wave
with room in its rings executes.  The test asserts that this rest holds no spill store, that it
writes the ring three times in blocks without any exec-mask save or exec branch of their own (the
selects that advance the write position were not turned back into branches), and that it holds fewer
exec-mask saves and fewer s_cbranch_exec* than the parent build's whole sorted path.  Counts at the
time of writing (every variant alike): parent's sorted path 12 saves / 11 exec branches; shipped
sorted path with room 7 / 8 (with its slow pushes 13 / 13); whole loop 33 / 31 and 34 / 33.

The build with steps 1, 2 and 4.

The steps keep the parent's pushes as the slow path inside the same loop, so the loop as a whole
holds more exec-mask code than the parent's; what an iteration with room in the ring executes is the
loop without its slow push paths.  The slow push paths are found from the code alone: the blocks
dominated by the nearest ancestor (in the dominator tree) of a spill store that is entered only
through wave-uniform branches (s_cbranch_scc* / s_cbranch_vcc*).  The test asserts that
  - every spill store (global_store_dword fed by v_mad_u64_u32) lies in such a region, and what
    remains of the loop, the fast region, still writes the ring (ds_write_b32: the pushes are
    there) -- in the parent's build the same cut leaves no ring write, which the test checks too;
  - the fast region holds fewer exec-mask saves and fewer s_cbranch_exec* than the parent's loop.
Counts at the time of writing (every variant alike): parent's loop 33 saves / 31 exec branches; with
the steps the whole loop 36 / 37, its fast region 15 / 18.
"""
import collections
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import waitcnt_audit  # noqa: E402

VARIANTS = ["ILi4ELb0ELb0ELi8ELb0EE", "ILi4ELb0ELb0ELi16ELb0EE", "ILi4ELb0ELb0ELi8ELb1EE", "ILi4ELb0ELb0ELi16ELb1EE"]

LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s*s_(cbranch_\w+|branch)\s+(\.LBB\d+_\d+)")
END = re.compile(r"^\s*s_endpgm")
UNIFORM = ("cbranch_scc0", "cbranch_scc1", "cbranch_vccz", "cbranch_vccnz")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa")
    procs = {}
    for name, v in (("shipped", None), ("steps", "7"), ("parent", "0")):
        cmd = ["make", "-s", "-C", str(ROOT / "my-raytracer_amd"), "asm", f"ASM_OUT={d / name}.s"]
        if v is not None:
            cmd.append(f"V=-DRT_STACK_FAST={v}")
        procs[name] = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for name, p in procs.items():
        assert p.wait(timeout=900) == 0, name
    return {name: d / f"{name}.s" for name in procs}


class Cfg:
    def __init__(self, body):
        self.body = body
        starts = {0}
        for i, l in enumerate(body):
            if LABEL.match(l):
                starts.add(i)
            if BRANCH.match(l) or END.match(l):
                starts.add(i + 1)
        starts = sorted(s for s in starts if s < len(body))
        self.blocks = [(s, starts[k + 1] if k + 1 < len(starts) else len(body)) for k, s in enumerate(starts)]
        at = {s: k for k, (s, _) in enumerate(self.blocks)}
        labels = {LABEL.match(body[s]).group(1): k for k, (s, _) in enumerate(self.blocks) if LABEL.match(body[s])}
        self.succ, self.term = [], []
        for s, e in self.blocks:
            m = BRANCH.match(body[e - 1])
            out = []
            if m:
                out.append(labels[m.group(2)])
                if m.group(1) != "branch" and e in at:
                    out.append(at[e])
            elif not END.match(body[e - 1]) and e in at:
                out.append(at[e])
            self.succ.append(out)
            self.term.append(m.group(1) if m else None)
        n = len(self.blocks)
        self.pred = [[] for _ in range(n)]
        for a, ss in enumerate(self.succ):
            for b in ss:
                self.pred[b].append(a)
        self._dominators()

    def _dominators(self):
        order, seen, stack = [], {0}, [(0, iter(self.succ[0]))]
        while stack:
            node, it = stack[-1]
            for b in it:
                if b not in seen:
                    seen.add(b)
                    stack.append((b, iter(self.succ[b])))
                    break
            else:
                order.append(node)
                stack.pop()
        rpo = order[::-1]
        idx = {b: i for i, b in enumerate(rpo)}
        idom = {0: 0}
        changed = True
        while changed:
            changed = False
            for b in rpo[1:]:
                new = None
                for p in self.pred[b]:
                    if p not in idom:
                        continue
                    if new is None:
                        new = p
                        continue
                    x, y = p, new
                    while x != y:
                        while idx[x] > idx[y]:
                            x = idom[x]
                        while idx[y] > idx[x]:
                            y = idom[y]
                    new = x
                if idom.get(b) != new:
                    idom[b] = new
                    changed = True
        self.idom = idom

    def dominates(self, a, b):
        while True:
            if a == b:
                return True
            if b == self.idom[b]:
                return False
            b = self.idom[b]

    def lines(self, k):
        s, e = self.blocks[k]
        return [l for l in self.body[s:e] if not LABEL.match(l)]

    def innermost_loop(self, site):
        loops = collections.defaultdict(set)
        for a, ss in enumerate(self.succ):
            if a not in self.idom:
                continue
            for h in ss:
                if self.dominates(h, a):   # back edge a -> h
                    nodes, work = {h, a}, [a]
                    while work:
                        x = work.pop()
                        if x != h:
                            for p in self.pred[x]:
                                if p in self.idom and p not in nodes:
                                    nodes.add(p)
                                    work.append(p)
                    loops[h] |= nodes
        return min(((len(b), h) for h, b in loops.items() if site in b))[1], loops

    def uniform_entered(self, k, depth=0):
        """Every way into block k is a wave-uniform conditional branch (taken or fallen through), seen
        through blocks that hold nothing but an unconditional branch."""
        if not self.pred[k] or depth > 4:
            return False
        for p in self.pred[k]:
            if self.term[p] in UNIFORM:
                continue
            if self.term[p] == "branch" and len(self.lines(p)) == 1 and self.uniform_entered(p, depth + 1):
                continue
            return False
        return True


def node_loop(path, variant):
    g = Cfg(waitcnt_audit.kernel_lines(str(path), variant))
    site = [k for k in range(len(g.blocks)) if sum(1 for l in g.lines(k) if re.match(r"\s*ds_read_b128", l)) == 7]
    assert len(site) == 1, "one block reads a treelet node with seven 16-byte LDS loads"
    head, loops = g.innermost_loop(site[0])
    return g, head, loops[head]


def count(g, blocks):
    c = collections.Counter(l.split()[0] for k in blocks for l in g.lines(k))
    return {"saves": sum(v for k, v in c.items() if "saveexec" in k),
            "exec_branches": sum(v for k, v in c.items() if k.startswith("s_cbranch_exec")),
            "ring_writes": c["ds_write_b32"], "spill_stores": c["global_store_dword"], "mad64": c["v_mad_u64_u32"]}


def split(g, head, loop):
    """(fast region, spill-store blocks outside any slow region)."""
    spill = [k for k in loop if any(l.split()[0] == "global_store_dword" for l in g.lines(k))]
    slow, stray = set(), []
    for b in spill:
        assert any(l.split()[0] == "v_mad_u64_u32" for l in g.lines(b)), "a spill store computes its address beside it"
        d = b
        while d != head and not g.uniform_entered(d):
            d = g.idom[d]
        if d == head:
            stray.append(b)
        else:
            slow |= {k for k in loop if g.dominates(d, k)}
    return loop - slow, stray


SORT_COMPARE = re.compile(r"\s*v_cmp_lt_f32")


def sorted_path(g, head, loop):
    """(the sorted path's blocks, those of them under the side of its wave-uniform branch that holds the
    spill stores)."""
    sort = [k for k in loop if any(SORT_COMPARE.match(l) for l in g.lines(k))]
    assert sort, "the sorting network's compares"
    above = [k for k in loop if k != head and g.uniform_entered(k) and all(g.dominates(k, s) for s in sort)]
    entry = [k for k in above if all(g.dominates(c, k) for c in above)]
    assert len(entry) == 1
    path = {k for k in loop if g.dominates(entry[0], k)}
    slow = set()
    for b in path:
        if any(l.split()[0] == "global_store_dword" for l in g.lines(b)):
            d = b
            while d != entry[0] and not g.uniform_entered(d):
                d = g.idom[d]
            slow |= {k for k in path if g.dominates(d, k)}   # (all of the path where no branch parts them)
    return path, slow


@pytest.mark.parametrize("variant", VARIANTS)
def test_shipped_sorted_path_with_room(asm, variant):
    g, head, loop = node_loop(asm["shipped"], variant)
    path, slow = sorted_path(g, head, loop)
    pg, phead, ploop = node_loop(asm["parent"], variant)
    ppath, pslow = sorted_path(pg, phead, ploop)
    room = path - slow
    whole, ship, fast, parent = count(g, loop), count(g, path), count(g, room), count(pg, ppath)
    print(variant, "shipped: loop", whole, "sorted path", ship, "with room", fast, "| parent: loop", count(pg, ploop),
          "sorted path", parent)
    assert pslow == ppath                     # the parent's pushes can all spill: no wave-uniform branch parts them
    assert parent["spill_stores"] == 3 and ship["spill_stores"] == 3
    assert slow and fast["spill_stores"] == 0
    writers = [k for k in room if any(l.split()[0] == "ds_write_b32" for l in g.lines(k))]
    assert count(g, writers)["ring_writes"] >= 3
    assert count(g, writers)["saves"] == 0 and count(g, writers)["exec_branches"] == 0
    assert fast["saves"] < parent["saves"]
    assert fast["exec_branches"] < parent["exec_branches"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_fast_paths_push_without_spill_stores_and_with_fewer_exec_branches(asm, variant):
    g, head, loop = node_loop(asm["steps"], variant)
    fast, stray = split(g, head, loop)
    pg, phead, ploop = node_loop(asm["parent"], variant)
    pfast, _ = split(pg, phead, ploop)
    whole, f, parent, pf = count(g, loop), count(g, fast), count(pg, ploop), count(pg, pfast)
    print(variant, "steps: loop", whole, "fast region", f, "| parent: loop", parent, "same cut", pf)
    assert whole["spill_stores"] >= 6 and parent["spill_stores"] >= 6   # three pushes on each of the two paths
    assert stray == [], "a spill store outside the wave-uniform slow paths"
    assert f["spill_stores"] == 0
    assert f["ring_writes"] >= 6          # the fast pushes of both paths
    assert pf["ring_writes"] == 0         # the parent has no push outside the paths that can spill
    assert f["saves"] < parent["saves"]
    assert f["exec_branches"] < parent["exec_branches"]


def test_cut_on_a_small_loop():
    # a loop whose body branches wave-uniformly into a block with a spill store, and one that reaches it
    # through an exec branch only
    def body(uniform):
        enter = ["\ts_cmp_lg_u64 s[2:3], 0", "\ts_cbranch_scc1 .LBB0_3"] if uniform else \
                ["\ts_and_saveexec_b64 s[4:5], vcc", "\ts_cbranch_execnz .LBB0_3"]
        return (["\ts_mov_b32 s0, 0", ".LBB0_1:"] + ["\tds_read_b128 v[0:3], v9"] * 7 + enter +
                [".LBB0_2:", "\tds_write_b32 v8, v7", "\ts_cbranch_vccnz .LBB0_1", "\ts_endpgm", ".LBB0_3:",
                 "\tv_mad_u64_u32 v[4:5], vcc, s6, v1, 0", "\tglobal_store_dword v[4:5], v6, off", "\ts_branch .LBB0_2"])
    for uniform in (True, False):
        g = Cfg(body(uniform))
        head, loops = g.innermost_loop(1)
        fast, stray = split(g, head, loops[head])
        assert (stray == []) == uniform
        assert count(g, fast)["spill_stores"] == (0 if uniform else 1)
