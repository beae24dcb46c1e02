"""Times kimimaro_amd.cross_sectional_area on bench.py's volume (default c3): skeletonizes it, then analyses the skeletons it has just
made.  After a warm-up call the analysis runs several times; reported are the medians of the wall time (host clock around the call,
which ends in device-to-host copies), of the kernel time (HIP events around the launches) and of the host driver's parts (path
walking and batching before the first launch, the first launch with its copies, the follow-up rounds), and vertices per second.

    python tools/cross_section_time.py [c3] [runs]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import kimimaro_amd
from kimimaro_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
eng = Engine()
lab, an = bench.make_volume(name, device=eng.device)
t0 = time.perf_counter()
skels = kimimaro_amd.skeletonize(lab, anisotropy=an, dust_threshold=1000, fix_borders=True, progress=False, _engine=eng)
eng.sync()
t_skel = time.perf_counter() - t0
nvert = sum(len(s.vertices) for s in skels.values())
kimimaro_amd.cross_sectional_area(lab, skels, anisotropy=an)                    # warm-up (allocator, code objects)
rows = []
for _ in range(runs):
    stats = {}
    eng.sync()
    t0 = time.perf_counter()
    kimimaro_amd.cross_sectional_area(lab, skels, anisotropy=an, _stats=stats)
    stats["wall_s"] = time.perf_counter() - t0
    rows.append(stats)
med = lambda key: statistics.median(r[key] for r in rows)
wall, kernel_ms = med("wall_s"), med("kernel_ms")
last = rows[-1]
evaluated = sum(int((s.cross_sectional_area > 0).sum()) for s in skels.values())
print("XSTIME %s: %d skeletons, %d vertices (%d with an area), %d occurrences on the paths, %d items in %d launches over %d rounds; "
      "skeletonize %.2f s" % (name, len(skels), nvert, evaluated, last["occurrences"], last["items"], last["launches"], last["rounds"],
                              t_skel))
print("  median of %d runs: wall %.1f ms = %.0f vertices/s; kernel %.2f ms (%.1f %% of the wall, %d waves, scratch %.0f MiB)" % (
    runs, wall * 1e3, nvert / wall, kernel_ms, 100 * kernel_ms * 1e-3 / wall, last["waves"], last["scratch_bytes"] / 2 ** 20))
print("  host driver: paths and batching %.1f ms, first launch with copies %.1f ms, follow-up rounds and means %.1f ms; spread of the "
      "wall %.1f .. %.1f ms" % (med("prepare_s") * 1e3, med("first_launch_s") * 1e3, med("finish_s") * 1e3,
                                min(r["wall_s"] for r in rows) * 1e3, max(r["wall_s"] for r in rows) * 1e3))
print(json.dumps({"workload": name, "skeletons": len(skels), "vertices": nvert, "items": last["items"], "rounds": last["rounds"],
                  "wall_s": wall, "kernel_ms": kernel_ms, "prepare_s": med("prepare_s"), "first_launch_s": med("first_launch_s"),
                  "finish_s": med("finish_s"), "vertices_per_s": nvert / wall, "waves": last["waves"]}))
