#!/usr/bin/env python3
"""tests/golden/gemm_status.json from a status sweep of the PARENT build (the full, line-per-tuple output of
tools/gemm_status_sweep.py; profiles/gemm_host/status_sweep_parent.txt is its digest): the tuples that build rejects
(status 2 / 3) and the m == 0 successes, one per entry, status and set of arguments that differ from the entry's base
tuple (every destination table separately) -- the expected values of tests/test_gemm_status_cpu.py never come from the
code under test.
usage: make_gemm_status_golden.py parent_sweep_lines.txt gemm_status.json"""
import json
import re
import sys

picked, seen = {}, set()
for line in open(sys.argv[1]):
    m = re.match(r"(\S+)  (.*)  -> (\d+)$", line.rstrip("\n"))
    if not m or int(m.group(3)) not in (0, 2, 3):
        continue
    entry, label, status = m.group(1), m.group(2), int(m.group(3))
    if entry.endswith("_size") or (status == 0 and "m=0" not in label.split()):
        continue
    # a destination table or a group stride alone is a check of its own per value; the products of three and more changed arguments
    # are thinned to three per status and number of changed arguments
    parts = label.split()
    names = tuple(sorted(p if len(parts) == 1 and p.split("=")[0] in ("dst", "ndst", "gstride") else p.split("=")[0] for p in parts))
    if len(names) > 2:
        names = (len(names), sum(1 for k in seen if k[:2] == (entry, status) and k[2][:1] == (len(names),)) % 3)
    if (entry, status, names) in seen:
        continue
    seen.add((entry, status, names))
    picked.setdefault(entry, {})[label] = status
with open(sys.argv[2], "w") as f:      # one line per entry: {label: status}
    f.write("{\n" + ",\n".join(f"{json.dumps(e)}:{json.dumps(t, separators=(',', ':'))}" for e, t in picked.items()) + "\n}\n")
print(sum(len(v) for v in picked.values()), "tuples")
