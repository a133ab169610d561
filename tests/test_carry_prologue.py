"""Every exported entry of the library that takes a non-const plan drops a carried right-hand side (MGCMT_OPT_CARRY) in its
first statement: entry_drops_carry(plan), once per such argument, or — the readers and the vector operations with a checked
destination — a CarryKeep, which drops it and decides on return.  mgcmt_vcycle, which consumes the carry, is the one
exception.  This reads the sources: an entry added without the prologue fails here, whatever it writes."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = re.compile(r"^int (mgcmt_\w+)\(([^{;]*)\)\s*\{\s*\n((?:[^\n]*\n){2})", re.M)
PLAN_ARG = re.compile(r"(const )?\bmgcmt_plan\* (\w+)")


def _entries():
    for path in sorted(glob.glob(os.path.join(ROOT, "multigridcmt_amd", "csrc", "*.hip"))):
        for m in ENTRY.finditer(open(path).read()):
            names = [n for c, n in PLAN_ARG.findall(m.group(2)) if not c]
            if names:
                yield m.group(1), names, m.group(3)


def test_every_non_const_entry_starts_with_the_prologue():
    seen = {}
    for name, plans, head in _entries():
        seen[name] = plans
        if name == "mgcmt_vcycle":
            continue
        lines = [l.strip() for l in head.split("\n")]
        if lines[0].startswith("CarryKeep "):
            assert lines[0].startswith("CarryKeep keep(%s);" % plans[0]), name
            continue
        for i, p in enumerate(plans):
            assert lines[i] == "entry_drops_carry(%s);" % p, (name, lines)
    # the scan sees what it is meant to see: single- and multi-line signatures, one- and two-plan entries, every host file
    for name in ("mgcmt_upload", "mgcmt_lincomb", "mgcmt_pcg_begin", "mgcmt_pcg_begin_k", "mgcmt_comm_init",
                 "mgcmt_comm_init_external", "mgcmt_halo_exchange", "mgcmt_sharded_vcycle", "mgcmt_plan_set_point_diagonal",
                 "mgcmt_rq_line_step", "mgcmt_twogrid", "mgcmt_vcycle"):
        assert name in seen, name
    assert seen["mgcmt_gather_coarse"] == ["p", "coarse"] and seen["mgcmt_copy_across"] == ["src", "dst"]
    assert len(seen) >= 60


def test_every_declared_non_const_entry_is_defined_where_the_scan_looks():
    """the header's declarations with a non-const plan against the definitions found above"""
    header = open(os.path.join(ROOT, "include", "mgcmt_hip.h")).read()
    declared = set()
    for m in re.finditer(r"^int (mgcmt_\w+)\(([^;]*)\);", header, re.M):
        if any(not c for c, _ in PLAN_ARG.findall(m.group(2))):
            declared.add(m.group(1))
    assert declared and declared == {name for name, _, _ in _entries()}
