"""rocprofv3 kernel-trace CSV -> the dispatches as `queue kernel grid workgroup`
lines in dispatch order (queues numbered by first appearance).  Prints the
listing's length and SHA-256, then the distinct lines with their counts.
usage: sequence.py TRACE_DIR [FULL_LISTING.txt]"""
import csv
import hashlib
import sys
from collections import Counter
from pathlib import Path

files = sorted(Path(sys.argv[1]).rglob("*kernel_trace.csv"))
assert len(files) == 1, files
rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Dispatch_Id"]))
queues = {}
lines = []
for r in rows:
    q = queues.setdefault(r["Queue_Id"], len(queues))
    grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
    wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
    lines.append(f"q{q} {r['Kernel_Name']} grid {grid} workgroup {wg}")
text = "".join(l + "\n" for l in lines)
if len(sys.argv) > 2:
    Path(sys.argv[2]).write_text(text)
print(f"{len(lines)} dispatches on {len(queues)} queues, sha256 of the ordered listing {hashlib.sha256(text.encode()).hexdigest()}")
for l, n in sorted(Counter(lines).items()):
    print(f"{n:4d} x {l}")
