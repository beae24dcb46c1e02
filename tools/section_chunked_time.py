"""Times kimimaro_amd.cross_sectional_area_chunked against kimimaro_amd.cross_sectional_area on bench.py's volume (default c3, 512^3):
skeletonizes it, analyses the skeletons with the whole volume resident, then again with the volume handed over as a dataset in chunks
of 256^3 (a host array, as a dataset on disk would be read: every box is cut on the host and uploaded).  After a warm-up call each
analysis runs several times; reported are the medians of the wall time, the chunked run's kernel time (HIP events) and the time it
spends loading boxes, the boxes and items of every growth round, the share of items that were run more than once, and whether the two
results are equal.  It sets no threshold.

    python tools/section_chunked_time.py [c3] [runs] [--chunk N] [--halo N]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import kimimaro_amd
from kimimaro_amd.engine import Engine


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


chunk, halo = option("--chunk", 256), option("--halo", 64)
args, skip = [], False
for a in sys.argv[1:]:
    if skip or a.startswith("--"):
        skip = a.startswith("--")
        continue
    args.append(a)
name = args[0] if len(args) > 0 else "c3"
runs = int(args[1]) if len(args) > 1 else 5
eng = Engine()
lab, an = bench.make_volume(name, device=eng.device)
skels = kimimaro_amd.skeletonize(lab, anisotropy=an, dust_threshold=1000, fix_borders=True, progress=False, _engine=eng)
eng.sync()
host = lab if isinstance(lab, np.ndarray) else np.asfortranarray(lab.cpu().numpy())
nvert = sum(len(s.vertices) for s in skels.values())


def fresh():
    return {k: kimimaro_amd.Skeleton(s.vertices.copy(), s.edges.copy(), segid=k, space=s.space) for k, s in skels.items()}


def timed(run):
    run(fresh(), None)                                   # warm-up (allocator, code objects)
    rows = []
    for _ in range(runs):
        mine, stats = fresh(), {}
        eng.sync()
        t0 = time.perf_counter()
        run(mine, stats)
        stats["wall_s"] = time.perf_counter() - t0
        rows.append(stats)
    return rows, mine


whole_rows, whole = timed(lambda s, stats: kimimaro_amd.cross_sectional_area(lab, s, anisotropy=an, _stats=stats))
chunk_rows, chunked = timed(lambda s, stats: kimimaro_amd.cross_sectional_area_chunked(host, s, chunk_shape=(chunk,) * 3, halo=halo,
                                                                                       anisotropy=an, timings=stats))
equal = all(whole[k].cross_sectional_area.tobytes() == chunked[k].cross_sectional_area.tobytes() and
            np.array_equal(whole[k].cross_sectional_area_contacts, chunked[k].cross_sectional_area_contacts) for k in whole)
med = lambda rows, key: statistics.median(r[key] for r in rows)
last = chunk_rows[-1]
boxes = [sum(c["boxes"][r] for c in last["calls"] if len(c["boxes"]) > r) for r in range(max(len(c["boxes"]) for c in last["calls"]))]
items = [sum(c["items"][r] for c in last["calls"] if len(c["items"]) > r) for r in range(len(boxes))]
share = last["items_rerun"] / max(1, last["items"])
print("XSCHUNKED %s: %d skeletons, %d vertices; chunks of %d^3 at halo %d: %d cores" % (name, len(skels), nvert, chunk, halo, last["cores"]))
print("  whole volume: wall %.1f ms (%.1f .. %.1f), kernel %.2f ms" % (
    med(whole_rows, "wall_s") * 1e3, min(r["wall_s"] for r in whole_rows) * 1e3, max(r["wall_s"] for r in whole_rows) * 1e3,
    med(whole_rows, "kernel_ms")))
print("  chunked:      wall %.1f ms (%.1f .. %.1f), kernel %.2f ms, loading / upload / counting %.1f ms, %.2f Gvoxels loaded" % (
    med(chunk_rows, "wall_s") * 1e3, min(r["wall_s"] for r in chunk_rows) * 1e3, max(r["wall_s"] for r in chunk_rows) * 1e3,
    med(chunk_rows, "kernel_ms"), med(chunk_rows, "load_s") * 1e3, last["voxels_loaded"] / 1e9))
print("  boxes per round %s, items per round %s: %.1f %% of the items run again, %d left clipped (bit 64); results equal: %s" % (
    boxes, items, 100 * share, last["capped_items"], equal))
print(json.dumps({"workload": name, "vertices": nvert, "chunk": chunk, "halo": halo, "whole_wall_s": med(whole_rows, "wall_s"),
                  "whole_kernel_ms": med(whole_rows, "kernel_ms"), "chunked_wall_s": med(chunk_rows, "wall_s"),
                  "chunked_kernel_ms": med(chunk_rows, "kernel_ms"), "chunked_load_s": med(chunk_rows, "load_s"),
                  "boxes_per_round": boxes, "items_per_round": items, "share_rerun": share, "capped_items": last["capped_items"],
                  "equal": bool(equal)}))
