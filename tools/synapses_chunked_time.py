"""Times synapses_to_targets_chunked on bench.py's volume (default c3, 512^3) cut into cores of 128^3 against
kimimaro_amd.synapses_to_targets of the same volume in one piece -- a volume both can hold, both from a host array, so that each
pays for bringing its voxels to the device.  2 000 synapses over 200 labels, for two sets of centroids:

  scattered   uniform float64 centroids all over the volume (tools/points_time.py's): a label's nearest voxel may lie anywhere;
  clustered   a voxel of the label plus a jitter of up to 1.5 voxels: what synapse detection gives.

After a warm-up call each runs `runs` times (default 5), the two taking turns, the device synchronised around every call; median
and spread of the wall time, with cores_visited / cores, pairs and the driver's load_s / visit_s.  Both must return the same items in
the same order.  No label is absent here: an absent label forces every core to be visited, so the speed depends on the input by
design.

    python tools/synapses_chunked_time.py [c3|c2] [runs, default 5] [core edge, default 128]
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
from kimimaro_amd import ops
from kimimaro_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
edge = int(sys.argv[3]) if len(sys.argv) > 3 else 128
eng = Engine()
ops._engine = eng
lab, _ = bench.make_volume(name, device=eng.device)
shape = tuple(int(v) for v in lab.shape)
chunk = (edge, edge, edge)
print("SYNAPSESCHUNKEDTIME %s %s as %d^3 cores" % (name, shape, edge), flush=True)


def clocked(fn):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return out, time.perf_counter() - t0


rng = np.random.default_rng(7)
# voxels drawn at random say which labels there are and give each its voxels for the clustered set
drawn = rng.integers(0, lab.size, size=1 << 20)
drawn_labels = lab.reshape(-1, order="F")[drawn]
values, counts = np.unique(drawn_labels[drawn_labels != 0], return_counts=True)
chosen = rng.choice(values[counts >= 10], size=200, replace=False).tolist()
scattered = {int(L): [(tuple(rng.uniform(0, np.array(shape)).tolist()), k % 4) for k in range(10)] for L in chosen}
clustered = {}
for L in chosen:
    picks = np.stack(np.unravel_index(drawn[drawn_labels == L][:10], shape, order="F"), axis=1)
    clustered[int(L)] = [(tuple((p + rng.uniform(-1.5, 1.5, 3)).tolist()), k % 4) for k, p in enumerate(picks)]

result = {"workload": name, "core_edge": edge, "synapses": 2000, "labels": 200}
print("| centroids | in one piece, ms | in boxes, ms | cores visited | pairs | load / visit, ms |")
print("|---|---|---|---|---|---|")
for tag, synapses in (("scattered", scattered), ("clustered", clustered)):
    whole_s, boxes_s, rows = [], [], []
    for k in range(runs + 1):                                        # the first call of each is the warm-up
        stats = {}
        boxed, dt = clocked(lambda: kimimaro_amd.synapses_to_targets_chunked(lab, synapses, chunk, stats=stats))
        whole, dt_whole = clocked(lambda: kimimaro_amd.synapses_to_targets(lab, synapses))
        assert list(boxed.items()) == list(whole.items()), "synapses_to_targets_chunked and synapses_to_targets disagree"
        if k:
            boxes_s.append(dt), whole_s.append(dt_whole), rows.append(stats)
    last = rows[-1]
    med = lambda key: statistics.median(float(r[key]) for r in rows)
    result[tag] = {"targets": len(boxed), "samples": len(boxes_s), "whole_ms": statistics.median(whole_s) * 1e3,
                   "whole_min_ms": min(whole_s) * 1e3, "whole_max_ms": max(whole_s) * 1e3, "chunked_ms": statistics.median(boxes_s) * 1e3,
                   "chunked_min_ms": min(boxes_s) * 1e3, "chunked_max_ms": max(boxes_s) * 1e3, "cores": last["cores"],
                   "cores_visited": last["cores_visited"], "pairs": last["pairs"], "load_ms": med("load_s") * 1e3,
                   "visit_ms": med("visit_s") * 1e3}
    r = result[tag]
    print("| %s, median of %d (min .. max) | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %d of %d | %d | %.1f / %.1f |" % (
        tag, r["samples"], r["whole_ms"], r["whole_min_ms"], r["whole_max_ms"], r["chunked_ms"], r["chunked_min_ms"], r["chunked_max_ms"],
        r["cores_visited"], r["cores"], r["pairs"], r["load_ms"], r["visit_ms"]), flush=True)
print(json.dumps(result))
