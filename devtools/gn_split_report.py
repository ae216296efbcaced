"""The pre-split writers in a rocprofv3 run of bench.py, launch by launch of the sampling step.
    python devtools/gn_split_report.py <kernel_trace.csv | counter_collection.csv> [label]
A kernel trace gives, per position of the launch in the step (steps end with pstep_kernel; the first two steps of the file
are dropped), grid, mean and minimum duration over the steps, and the totals per grid = per level.  A counter collection
(one row per dispatch and counter) gives the mean of every counter per position and per grid."""
import collections
import csv
import re
import sys

PAT = ("gn_apply_split_kernel", "split_plain_kernel")
rows = list(csv.DictReader(open(sys.argv[1])))
label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
pmc = "Counter_Name" in rows[0]
key_t = "Start_Timestamp" if not pmc else "Dispatch_Id"
disp = collections.OrderedDict()          # dispatch -> (name, grid, {counter: value} | duration)
for r in sorted(rows, key=lambda r: int(r[key_t])):
    d = int(r["Dispatch_Id"])
    if "Grid_Size_X" in r:
        grid = tuple(int(r[f"Grid_Size_{a}"]) // int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")
    else:                                 # counter collection: threads in all -> blocks in all
        grid = (int(r["Grid_Size"]) // int(r["Workgroup_Size"]),)
    if d not in disp:
        disp[d] = [r["Kernel_Name"], grid, {} if pmc else (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3]
    if pmc:
        disp[d][2][r["Counter_Name"]] = float(r["Counter_Value"])

steps, cur = [], []
for name, grid, val in disp.values():
    if "pstep" in name:
        steps.append(cur)
        cur = []
    elif any(p in name for p in PAT):
        m = re.search(r"(gn_apply_split_kernel|split_plain_kernel)I([^E]*)E", name)
        cur.append((m.group(1)[:14] + "<" + m.group(2).replace("Li", "").replace("E", ",") + ">" if m else name[:30], grid, val))
steps = [s for s in steps[2:] if len(s) == len(steps[-1])]
print(f"# {label}: {len(steps)} steps of {len(steps[-1]) if steps else 0} pre-split writer launches")
if not steps:
    sys.exit(0)
per_grid = collections.defaultdict(list)
for i in range(len(steps[0])):
    name, grid, _ = steps[0][i]
    if not pmc:
        v = [s[i][2] for s in steps]
        per_grid[(name, grid)].append(sum(v) / len(v))
        print(f"{i:3d} {name:22s} grid {str(grid):14s} mean {sum(v) / len(v):6.2f} us  min {min(v):6.2f} us")
    else:
        out = []
        for c in sorted(steps[0][i][2]):
            v = [s[i][2][c] for s in steps if c in s[i][2]]
            out.append(f"{c} {sum(v) / len(v):.0f}")
            per_grid[(name, grid, c)].append(sum(v) / len(v))
        print(f"{i:3d} {name:22s} grid {str(grid):14s} " + "  ".join(out))
print("# per kernel and grid (= level): launches per step, mean")
for k, v in per_grid.items():
    print(f"{str(k):70s} n {len(v):2d}  mean {sum(v) / len(v):12.2f}  sum {sum(v):12.2f}")
