"""Times kimimaro_amd.oversegment_chunked against kimimaro_amd.oversegment on bench.py's volume (default c3, 512^3): skeletonizes it,
cuts it into segments with the whole volume resident, then again with the volume handed over as a dataset in chunks of 256^3 (a host
array, as a dataset on disk would be read: every box is cut on the host and uploaded, every core written back to the stores).  After
a warm-up call each runs several times; reported are the medians of the wall time, where the chunked run spends it (loading / upload /
write back, the kernels of the visits, the two numbering sweeps), rounds and visits per core of both phases, and whether the two
results are equal.  It sets no threshold.

    python tools/oversegment_chunked_time.py [c3] [runs] [chunk]
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

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 256
eng = Engine()
lab, an = bench.make_volume(name, device=eng.device)
skels = kimimaro_amd.skeletonize(lab, anisotropy=an, dust_threshold=1000, fix_borders=True, progress=False, _engine=eng)
eng.sync()
host = lab if isinstance(lab, np.ndarray) else np.asfortranarray(lab.cpu().numpy())
nvert = sum(len(s.vertices) for s in skels.values())


def timed(run):
    run({})                                              # warm-up (allocator, code objects)
    rows = []
    for _ in range(runs):
        stats = {}
        eng.sync()
        t0 = time.perf_counter()
        out = run(stats)
        eng.sync()
        stats["wall_s"] = time.perf_counter() - t0
        rows.append(stats)
    return rows, out


whole_rows, (whole_f, whole_s) = timed(lambda stats: kimimaro_amd.oversegment(lab, skels, anisotropy=an, _stats=stats))
chunk_rows, (chunk_f, chunk_s) = timed(lambda stats: kimimaro_amd.oversegment_chunked(host, skels, chunk_shape=(chunk,) * 3, anisotropy=an,
                                                                                    timings=stats))
equal = whole_f.dtype == chunk_f.dtype and np.array_equal(whole_f, chunk_f) and all(
    np.array_equal(whole_s[k].segments, chunk_s[k].segments) for k in whole_s)
med = lambda rows, key: statistics.median(r[key] for r in rows)
last = chunk_rows[-1]
whole_wall, chunk_wall = med(whole_rows, "wall_s"), med(chunk_rows, "wall_s")
print("OSCHUNKED %s: %d skeletons, %d vertices, %d segments; chunks of %d^3: %d cores" % (
    name, len(skels), nvert, last["segments"], chunk, last["cores"]))
print("  whole volume: wall %.1f ms (%.1f .. %.1f)" % (whole_wall * 1e3, min(r["wall_s"] for r in whole_rows) * 1e3,
                                                        max(r["wall_s"] for r in whole_rows) * 1e3))
print("  chunked:      wall %.1f ms (%.1f .. %.1f) = %.1f x; loading / upload / write back %.1f ms, kernels of the visits %.1f ms, "
      "numbering sweeps %.1f ms; %.2f Gvoxels loaded in %d boxes" % (
          chunk_wall * 1e3, min(r["wall_s"] for r in chunk_rows) * 1e3, max(r["wall_s"] for r in chunk_rows) * 1e3, chunk_wall / whole_wall,
          med(chunk_rows, "load_s") * 1e3, med(chunk_rows, "relax_ms"), med(chunk_rows, "number_s") * 1e3, last["voxels_loaded"] / 1e9,
          last["boxes_loaded"]))
print("  distances: %d rounds, %d visits (%.2f per core); features: %d rounds, %d visits (%.2f per core); results equal: %s" % (
    last["distance_rounds"], last["distance_visits"], last["distance_visits"] / last["cores"], last["feature_rounds"],
    last["feature_visits"], last["feature_visits"] / last["cores"], equal))
print(json.dumps({"workload": name, "vertices": nvert, "segments": last["segments"], "chunk": chunk, "cores": last["cores"],
                  "whole_wall_s": whole_wall, "chunked_wall_s": chunk_wall, "ratio": chunk_wall / whole_wall,
                  "load_s": med(chunk_rows, "load_s"), "relax_ms": med(chunk_rows, "relax_ms"), "number_s": med(chunk_rows, "number_s"),
                  "distance_rounds": last["distance_rounds"], "distance_visits": last["distance_visits"],
                  "feature_rounds": last["feature_rounds"], "feature_visits": last["feature_visits"],
                  "boxes_loaded": last["boxes_loaded"], "voxels_loaded": last["voxels_loaded"], "equal": bool(equal)}))
