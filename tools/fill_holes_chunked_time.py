"""Times fill_all_holes_chunked on bench.py's volume (default c3, 512^3) cut into chunks of 256^3, with a few hundred
closed pockets planted inside its labels (tools/fill_holes_time.py's: background or a foreign label in a 3 x 3 x 3 box; every
fourth one sits on a cut between two chunks), so that something is filled and some of it only on the dataset.

Two comparisons, in one process:

  fill     fill_all_holes_chunked of a host copy of the volume, with its parts (the first sweep: regions_s, of it the seams; merge_s;
           the resolver; the second sweep: apply_s), against kimimaro_amd.intake.fill_all_holes of a host copy in one piece.  After a
           warm-up call each runs `runs` times (default 3), the two taking turns; median and spread of the wall time.  Both must
           leave the same volume and count.
  skeletons  the `chunks_s` of skeletonize_chunked(fill_holes=True, merge=False) -- every box filled on its own by the per-label loop
           intake.fill_all_holes_device -- against fill_s + chunks_s of skeletonize_chunked(fill_holes_global=True, merge=False).
           ONE sample each, after one warm-up call without any filling (whose chunks_s is printed too).  The two routes do not
           compute the same thing where a pocket lies across a cut; the fragments of each are counted.

    python tools/fill_holes_chunked_time.py [c3|c2|mini] [runs, default 3] [chunk edge, default 256] [lanes, default lanes_for()]
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
from kimimaro_amd import intake, ops
from kimimaro_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
edge = int(sys.argv[3]) if len(sys.argv) > 3 else 256
width = int(sys.argv[4]) if len(sys.argv) > 4 else None
eng = Engine()
ops._engine = eng
lab, an = bench.make_volume(name, device=eng.device)
shape = tuple(int(v) for v in lab.shape)
chunk = (edge, edge, edge)


def plant_pockets(lab, want=300, seed=5):
    """3 x 3 x 3 boxes of background (even ones) or of a label of their own (odd ones) where a 5 x 5 x 5 box holds one label; every
    fourth try has its centre on a cut plane of the chunks, where there is one -> (volume, planted, of them across a cut)"""
    rng = np.random.default_rng(seed)
    out = lab.copy(order="F")
    top = int(lab.max())
    planted = across = 0
    for k in range(200 * want):
        c = [int(rng.integers(3, s - 3)) for s in shape]
        axis = int(rng.integers(0, 3))
        on_cut = k % 4 == 0 and shape[axis] > edge + 3
        if on_cut:
            c[axis] = edge * int(rng.integers(1, (shape[axis] - 4) // edge + 1))
        box = lab[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3]
        now = out[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3]
        if box[0, 0, 0] == 0 or (box != box[0, 0, 0]).any() or (now != box).any():
            continue
        out[c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2, c[2] - 1:c[2] + 2] = 0 if planted % 2 == 0 else top + 1 + planted
        planted += 1
        across += on_cut
        if planted == want:
            break
    return out, planted, across


volume, planted, across = plant_pockets(lab)
print("planted %d pockets, %d of them across a cut" % (planted, across), flush=True)


def clocked(fn):
    eng.sync()
    t0 = time.perf_counter()
    out = fn()
    eng.sync()
    return out, time.perf_counter() - t0


# ---- fill: in boxes against in one piece, taking turns ------------------------------------------------------------------------------
whole_s, boxes_s, rows = [], [], []
for k in range(runs + 1):                                            # the first call of each is the warm-up
    stats = {}
    (boxed, n_boxed), dt = clocked(lambda: kimimaro_amd.fill_all_holes_chunked(volume.copy(order="F"), chunk, return_fill_count=True,
                                                                               stats=stats))
    print("  fill_all_holes_chunked call %d: %.1f ms" % (k, dt * 1e3), flush=True)
    (whole, n_whole), dt_whole = clocked(lambda: intake.fill_all_holes(volume.copy(order="F"), return_fill_count=True))
    print("  fill_all_holes call %d: %.1f ms" % (k, dt_whole * 1e3), flush=True)
    if k:
        boxes_s.append(dt), whole_s.append(dt_whole), rows.append(stats)
    same = bool(np.array_equal(boxed, whole)) and n_boxed == n_whole
    assert same, "fill_all_holes_chunked and fill_all_holes disagree"
    del boxed, whole
med = lambda key: statistics.median(float(r[key]) for r in rows)
last = rows[-1]
fill = {
    "workload": name, "chunk_edge": edge, "pockets": planted, "pockets_across_a_cut": across, "filled": n_boxed, "results_equal": same,
    "samples": len(boxes_s), "chunked_ms": statistics.median(boxes_s) * 1e3, "chunked_min_ms": min(boxes_s) * 1e3,
    "chunked_max_ms": max(boxes_s) * 1e3, "whole_ms": statistics.median(whole_s) * 1e3, "whole_min_ms": min(whole_s) * 1e3,
    "whole_max_ms": max(whole_s) * 1e3, "regions_ms": med("regions_s") * 1e3, "seam_ms": med("seam_ms"), "merge_ms": med("merge_s") * 1e3,
    "resolve_ms": med("resolve_ms"), "apply_ms": med("apply_s") * 1e3, "cores": last["cores"], "cores_painted": last["cores_painted"],
    "provisional_regions": last["provisional_regions"], "merged_regions": last["merged_regions"], "seam_pairs": last["seam_pairs"],
    "labels": last["labels"],
}
# (the copy of the volume that each call fills is made inside the clocked stretch of both)
print("FILLCHUNKEDTIME %s as %d^3 chunks: %d voxels filled, results equal: %s" % (name, edge, n_boxed, same))
print("  in one piece  median of %d: %.1f ms (%.1f .. %.1f)" % (len(whole_s), fill["whole_ms"], fill["whole_min_ms"], fill["whole_max_ms"]))
print("  in boxes      median of %d: %.1f ms (%.1f .. %.1f) = first sweep %.1f (of it seams %.1f) + merge %.1f + resolver %.1f + second "
      "sweep %.1f ms; %d of %d cores painted" % (len(boxes_s), fill["chunked_ms"], fill["chunked_min_ms"], fill["chunked_max_ms"],
                                                fill["regions_ms"], fill["seam_ms"], fill["merge_ms"], fill["resolve_ms"], fill["apply_ms"],
                                                fill["cores_painted"], fill["cores"]))
print(json.dumps(fill), flush=True)

# ---- skeletons: every box filled on its own against the dataset filled first, one sample each ----------------------------------------
params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
kw = dict(teasar_params=params, anisotropy=an, dust_threshold=1000, fix_borders=True, fix_branching=True, merge=False, width=width)
res = {"workload": name, "chunk_edge": edge}
for tag, extra in (("no_fill", dict()), ("per_box", dict(fill_holes=True)), ("global", dict(fill_holes_global=True))):
    timings = {}
    got, dt = clocked(lambda: kimimaro_amd.skeletonize_chunked(volume, chunk, timings=timings, **dict(kw, **extra)))
    res[tag] = dict(total_s=dt, chunks_s=timings["chunks_s"], fill_s=timings.get("fill_s", 0.0), filled=timings.get("filled"),
                    chunks=timings["chunks"], labels=len(got), fragments=timings["fragments"], vertices=timings["vertices"])
    print("  skeletonize_chunked %s: %.2f s, chunks_s %.2f, fill_s %.2f; %d labels, %d fragments, %d vertices" % (
        tag, dt, timings["chunks_s"], timings.get("fill_s", 0.0), len(got), timings["fragments"], timings["vertices"]), flush=True)
    del got
per_box, glob = res["per_box"]["chunks_s"], res["global"]["fill_s"] + res["global"]["chunks_s"]
res["faster"] = "fill_holes_global" if glob < per_box else "fill_holes per box"
print("SKELFILLTIME %s as %d^3 chunks, single samples: per box chunks_s %.2f s; global fill_s %.2f + chunks_s %.2f = %.2f s; without any "
      "filling chunks_s %.2f s -> faster: %s" % (name, edge, per_box, res["global"]["fill_s"], res["global"]["chunks_s"], glob,
                                                 res["no_fill"]["chunks_s"], res["faster"]))
print(json.dumps(res), flush=True)
print("| what | ms |")
print("|---|---|")
print("| `fill_all_holes` of %s in one piece, median of %d (min .. max) | %.1f (%.1f .. %.1f) |" % (
    name, len(whole_s), fill["whole_ms"], fill["whole_min_ms"], fill["whole_max_ms"]))
print("| `fill_all_holes_chunked`, %d^3 chunks, median of %d (min .. max) | %.1f (%.1f .. %.1f) |" % (
    edge, len(boxes_s), fill["chunked_ms"], fill["chunked_min_ms"], fill["chunked_max_ms"]))
print("| its parts: first sweep (seams) / merge / resolver / second sweep | %.1f (%.1f) / %.1f / %.1f / %.1f |" % (
    fill["regions_ms"], fill["seam_ms"], fill["merge_ms"], fill["resolve_ms"], fill["apply_ms"]))
print("| `skeletonize_chunked(fill_holes=True)` `chunks_s`, one sample | %.0f |" % (per_box * 1e3))
print("| `skeletonize_chunked(fill_holes_global=True)` `fill_s` + `chunks_s`, one sample | %.0f + %.0f |" % (
    res["global"]["fill_s"] * 1e3, res["global"]["chunks_s"] * 1e3))
