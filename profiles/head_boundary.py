"""The batch boundary of the pipelined HBM path in a rocprofv3 rocpd database:
python profiles/head_boundary.py results.db [n_boundaries]
For each of the last n boundaries (default 7): how long the tile stream is empty between the last camera's
`rasterize_bwd` of one batch and the first `rasterize_fwd` of the next, and every other kernel that runs from the start
of that backward to the start of that forward (offset from the END of the backward: negative = under it), then the
medians over the boundaries.  A boundary is found by its `visibility_emit` launch (one per batch)."""
import sqlite3
import statistics
import sys

db = sys.argv[1]
n_b = int(sys.argv[2]) if len(sys.argv) > 2 else 7
c = sqlite3.connect(db)
rows = list(c.execute("select name, start, end, queue_id from kernels order by start"))


def short(n):
    n = n.split("(")[0].split("<")[0]
    n = n.replace("clmgs::", "").replace("_kernel", "")
    n = n.replace("void ", "").replace("(anonymous namespace)::", "")
    return n.strip()[-36:]


# bench.py's timed steps end with the whole-table flush of the deferred row optimizer (kernel_stats.py's anchor): what
# follows it (evidence passes) is not looked at
flush = [r[1] for r in rows if "adam_catch_up48_kernel<int>" in r[0]]
t_last = max(flush) if flush else max(r[2] for r in rows)
emits = [r for r in rows if "visibility_emit" in r[0] and r[1] < t_last]
gaps, under, per = [], [], {}
for em in emits[-n_b:]:
    bwd = [r for r in rows if "rasterize_bwd" in r[0] and r[1] < em[1]]
    fwd = [r for r in rows if "rasterize_fwd" in r[0] and r[1] > em[1]]
    if not bwd or not fwd:
        continue
    a, b = bwd[-1], fwd[0]
    gap = (b[1] - a[2]) / 1e6
    gaps.append(gap)
    print(f"boundary at visibility_emit {em[1]}: last rasterize_bwd {(a[2] - a[1]) / 1e6:.3f} ms, "
          f"tile stream empty {gap:.3f} ms")
    hid = 0.0
    for r in rows:
        if r[2] <= a[1] or r[1] >= b[1] or "rasterize" in r[0]:
            continue
        nm, dur = short(r[0]), (r[2] - r[1]) / 1e6
        print(f"   {(r[1] - a[2]) / 1e6:8.3f} ms  {dur:7.3f} ms  q{r[3]}  {nm}")
        if "adam_small_deferred" in nm or "visibility_bits" in nm:
            hid += max(0.0, min(r[2], a[2]) - max(r[1], a[1])) / 1e6
            per.setdefault(nm, []).append(dur)
        elif "visibility_emit" in nm:
            per.setdefault(nm, []).append(dur)
    under.append(hid)
print()
if gaps:
    print(f"boundaries {len(gaps)}: tile stream empty median {statistics.median(gaps):.3f} ms "
          f"(min {min(gaps):.3f}, max {max(gaps):.3f})")
    print(f"head kernels (adam_small_deferred, visibility_bits) under the last rasterize_bwd: median "
          f"{statistics.median(under):.3f} ms per boundary")
    for nm, v in sorted(per.items()):
        print(f"  {nm}: {len(v) / len(gaps):.1f} launches per boundary, median {statistics.median(v):.3f} ms "
              f"(min {min(v):.3f}, max {max(v):.3f}), per boundary {sum(v) / len(gaps):.3f} ms")
