"""The hierarchy optimiser on the host (rt_upload_options.tree_opt), through
rt_debug_tree_report: no GPU, no HIP call.

Every scene of tests/tree_opt_scenes.py with the default options (SBVH; tree_opt by size: on from
2^10 input triangles), with tree_opt = -1 (off), 1 (one pass) and RT_TREE_OPT_MAX (run to convergence):
  * the validity word is clean: internal boxes are the unions of their children, every leaf kept
    its box and its records, every record is referenced exactly once, child ids are above their
    parent's (and, after the optimiser, records follow the leaves left to right);
  * the binary SAH cost and the 4-wide collapse's cost do not rise;
  * the converged tree is a fixed point: the library runs the optimiser on it a second time and
    reports RT_TREE_BAD_FIXPOINT if anything changed;
  * build_threads 1 and 7 give the same report;
  * tree_opt = -1 leaves the node and record counts of the builder's tree.
"""
import pytest

import rtamd
import tree_opt_scenes as tos
from rtamd import abi

# Office, default options: the 4-wide cost relative to tree_opt = -1 in the same call.  The committed
# run gives 10.6596 -> 10.1128, a reduction of 5.13 %; the bound keeps three quarters of it.
OFFICE_DP_REDUCTION = 0.0513
OFFICE_DP_BOUND = 0.75 * OFFICE_DP_REDUCTION


def report(hs, **opts):
    opts.setdefault("build_threads", 1)
    d = rtamd.tree_report(hs, **opts).as_dict()
    d.pop("seconds")
    return d


@pytest.mark.parametrize("name", tos.NAMES)
def test_optimised_tree_is_valid_and_no_worse(tmp_path_factory, name):
    hs = tos.host(name, tmp_path_factory)
    off, dflt, conv = report(hs, tree_opt=-1), report(hs), report(hs, tree_opt=abi.RT_TREE_OPT_MAX)
    one = report(hs, tree_opt=1)
    print(f"{name}: off {off}\n  default {dflt}\n  one pass {one}\n  converged {conv}")
    assert off["invalid"] == 0 and off["passes"] == 0 and off["moved"] == 0
    assert (off["sah_after"], off["dp_after"]) == (off["sah_before"], off["dp_before"])
    for r in (dflt, one, conv):
        assert r["invalid"] == 0
        assert (r["sah_before"], r["dp_before"]) == (off["sah_before"], off["dp_before"])
        assert r["sah_after"] <= r["sah_before"] and r["dp_after"] <= r["dp_before"]
        assert (r["binary_nodes"], r["records"]) == (off["binary_nodes"], off["records"])   # nothing added or lost
        assert 1 <= r["stack4"] <= 4096
    assert one["passes"] == 1
    if name in tos.BY_SIZE_ON:
        assert 1 <= dflt["passes"] <= abi.RT_TREE_OPT_PASSES
    else:   # below 2^10 input triangles the default leaves the builder's tree
        assert dflt == off
    # converged within the cap: the last pass moved nothing and the library's second run (the
    # RT_TREE_BAD_FIXPOINT check above) changed nothing
    assert conv["converged"] == 1 and conv["passes"] < abi.RT_TREE_OPT_MAX
    assert conv["sah_after"] <= dflt["sah_after"]


@pytest.mark.parametrize("name", tos.NAMES)
def test_report_independent_of_build_threads(tmp_path_factory, name):
    hs = tos.host(name, tmp_path_factory)
    assert report(hs, build_threads=1) == report(hs, build_threads=7)


def test_office_wide_cost_falls(tmp_path_factory):
    """Office proxy, default options against tree_opt = -1 in the same call: the 4-wide cost
    (the quantity the collapse minimises) falls from 10.6596 to 10.1128, by 5.13 %; asserted: by at
    least three quarters of that, 3.85 %."""
    hs = tos.host("office", tmp_path_factory)
    off, dflt = report(hs, tree_opt=-1), report(hs)
    red = 1.0 - dflt["dp_after"] / off["dp_after"]
    print(f"office 4-wide cost {off['dp_after']:.4f} -> {dflt['dp_after']:.4f} ({100 * red:.2f} % lower), "
          f"binary SAH {off['sah_after']:.4f} -> {dflt['sah_after']:.4f}, {dflt['moved']} subtrees moved")
    assert dflt["moved"] > 0
    assert red >= OFFICE_DP_BOUND


def test_by_size_rule_and_option_range(tmp_path_factory):
    hs = tos.host("cornell", tmp_path_factory)
    for tree in ("sah", "reference"):   # the comparators stay un-optimised by default, opt in by count
        assert report(hs, tree=tree)["passes"] == 0
        r = report(hs, tree=tree, tree_opt=2)
        assert r["passes"] >= 1 and r["invalid"] == 0 and r["sah_after"] <= r["sah_before"]
    for bad in (-2, abi.RT_TREE_OPT_MAX + 1):
        with pytest.raises(rtamd.RtError):
            rtamd.tree_report(hs, tree_opt=bad)
    assert abi.UploadOptions.tree_opt.offset == abi.UploadOptions.spp_lanes.offset + 4
