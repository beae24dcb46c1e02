"""Times kimimaro_amd.cross_sectional_area_filled_chunked against kimimaro_amd.cross_sectional_area_filled on bench.py's volume
(default c3, 512^3), as tools/section_chunked_time.py does for the unfilled pair: skeletonizes the volume, analyses the skeletons with
the whole volume resident, then again with the volume handed over as a host array in cores of 256^3 (the region graph of the dataset
from one sweep over the cores, the region store in host memory, then the boxes).  After a warm-up call each analysis runs several
times; reported are the medians and the smallest and largest of the wall time, the whole-volume call's region pass and kernel, and
the chunked call's `timings`: the sweep, of it the seams (per core too), the host merge, the host search for the holes, loading, the
kernel.  It ASSERTS that the two results are equal, areas bit for bit, and sets no threshold on a time.

    python tools/section_filled_chunked_time.py [c3] [runs] [--chunk N] [--halo N]
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


whole_rows, whole = timed(lambda s, stats: kimimaro_amd.cross_sectional_area_filled(lab, s, anisotropy=an, _stats=stats))
chunk_rows, chunked = timed(lambda s, stats: kimimaro_amd.cross_sectional_area_filled_chunked(host, s, chunk_shape=(chunk,) * 3, halo=halo,
                                                                                              anisotropy=an, timings=stats))
for k in whole:
    assert whole[k].cross_sectional_area.tobytes() == chunked[k].cross_sectional_area.tobytes(), k
    assert np.array_equal(whole[k].cross_sectional_area_contacts, chunked[k].cross_sectional_area_contacts), k
med = lambda rows, key: statistics.median(r[key] for r in rows)
span = lambda rows, key, scale=1.0: "%.1f (%.1f .. %.1f)" % (med(rows, key) * scale, min(r[key] for r in rows) * scale,
                                                            max(r[key] for r in rows) * scale)
last = chunk_rows[-1]
holes = whole_rows[-1].get("holes", {})
print("XSFILLEDCHUNKED %s: %d skeletons, %d vertices; cores of %d^3 at halo %d: %d cores" % (name, len(skels), nvert, chunk, halo,
                                                                                          last["cores"]))
print("  whole volume: wall %s ms, kernel %s ms; %d regions, %d listed" % (
    span(whole_rows, "wall_s", 1e3), span(whole_rows, "kernel_ms"), holes.get("regions", -1), holes.get("csr_regions", -1)))
print("  chunked:      wall %s ms, kernel %s ms, loading / upload / counting %s ms" % (
    span(chunk_rows, "wall_s", 1e3), span(chunk_rows, "kernel_ms"), span(chunk_rows, "load_s", 1e3)))
print("  region graph: sweep %s ms, of it seams %s ms = %.2f ms per core; merge %s ms, enclosed %s ms" % (
    span(chunk_rows, "regions_s", 1e3), span(chunk_rows, "seam_ms"), med(chunk_rows, "seam_ms") / last["cores"],
    span(chunk_rows, "merge_s", 1e3), span(chunk_rows, "enclosed_ms")))
print("  %d provisional regions, %d merged, %d seam pairs, %d listed ids; boxes %s, items %s, %d left clipped; results equal: True" % (
    last["provisional_regions"], last["merged_regions"], last["seam_pairs"], last["listed_ids"],
    [c["boxes"] for c in last["calls"]], [c["items"] for c in last["calls"]], last["capped_items"]))
keys = ("wall_s", "kernel_ms", "load_s", "regions_s", "seam_ms", "merge_s", "enclosed_ms")
print(json.dumps({"workload": name, "vertices": nvert, "chunk": chunk, "halo": halo, "runs": runs,
                  "whole_wall_s": [r["wall_s"] for r in whole_rows], "whole_kernel_ms": [r["kernel_ms"] for r in whole_rows],
                  "chunked": {k: [r[k] for r in chunk_rows] for k in keys},
                  "provisional_regions": last["provisional_regions"], "merged_regions": last["merged_regions"],
                  "seam_pairs": last["seam_pairs"], "listed_ids": last["listed_ids"], "equal": True}))
