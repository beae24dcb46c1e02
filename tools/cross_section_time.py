"""Times kimimaro_amd.cross_sectional_area on bench.py's volume (default c3): skeletonizes it, then analyses the skeletons it has just
made.  After a warm-up call the analysis runs several times; reported are the medians of the wall time (host clock around the call,
which ends in device-to-host copies), of the kernel time (HIP events around the launches) and of the host driver's parts (path
walking and batching before the first launch, the first launch with its copies, the follow-up rounds), and vertices per second.

    python tools/cross_section_time.py [c3] [runs] [--fill-holes] [--walk host|device]

--walk device walks the paths and smooths the normals on the GPU (default host): prepare_s, the host driver's time
before the first launch, is printed next to the wall time and the kernel time, with walk_s (the walk's device calls and copies)
and pack_s (the numpy around them) where the device walks, and a checksum of the areas to compare two runs by.

--fill-holes times cross_sectional_area_filled (the reference's fill_holes=True): also reported are what Engine.region_graph says (regions, pairs, the passes' milliseconds), the
host search's milliseconds (kh_host_enclosed_regions), the size of the lists and the number of labels with holes.
The workload `shells` is synthetic: 256^3, a grid of 64 hollow boxes (wall 3) each around a core of another label, every box with a
straight skeleton along x through its centre -- most sections cross a hole.  With --fill-holes it also times the unfilled kernel on
the same items, for the cost per vertex of the region lookups.
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



def shells_volume(device):
    """(labels on the device indexed [x, y, z], anisotropy, {id: Skeleton in voxel units})"""
    import numpy as np
    import torch
    lab = np.zeros((256, 256, 256), dtype=np.uint32, order="F")
    skels = {}
    for k in range(64):
        cx, cy, cz = (32 + 64 * (k % 4), 32 + 64 * ((k // 4) % 4), 32 + 64 * (k // 16))
        shell, core = 2 * k + 1, 2 * k + 2
        lab[cx - 24:cx + 25, cy - 24:cy + 25, cz - 24:cz + 25] = shell
        lab[cx - 21:cx + 22, cy - 21:cy + 22, cz - 21:cz + 22] = 0
        lab[cx - 8:cx + 9, cy - 8:cy + 9, cz - 8:cz + 9] = core
        verts = np.array([[x, cy, cz] for x in range(cx - 24, cx + 25)], dtype=np.float32)
        edges = np.array([[i, i + 1] for i in range(len(verts) - 1)], dtype=np.uint32)
        skels[shell] = kimimaro_amd.Skeleton(verts, edges, segid=shell)
    return torch.from_numpy(lab.transpose(2, 1, 0).copy()).to(device).permute(2, 1, 0), (1, 1, 1), skels


argv = sys.argv[1:]
walk = "host"
if "--walk" in argv:
    at = argv.index("--walk")
    walk = argv[at + 1]
    del argv[at:at + 2]
args = [a for a in argv if not a.startswith("--")]
fill_holes = "--fill-holes" in argv
name = args[0] if len(args) > 0 else "c3"
runs = int(args[1]) if len(args) > 1 else 5
eng = Engine()
t0 = time.perf_counter()
if name == "shells":
    lab, an, skels = shells_volume(eng.device)
else:
    lab, an = bench.make_volume(name, device=eng.device)
    t0 = time.perf_counter()
    skels = kimimaro_amd.skeletonize(lab, anisotropy=an, dust_threshold=1000, fix_borders=True, progress=False, _engine=eng)
eng.sync()
t_skel = time.perf_counter() - t0
nvert = sum(len(s.vertices) for s in skels.values())


def timed(fill):
    run = kimimaro_amd.cross_sectional_area_filled if fill else kimimaro_amd.cross_sectional_area
    run(lab, skels, anisotropy=an, walk=walk)  # warm-up (allocator, code objects)
    out = []
    for _ in range(runs):
        stats = {}
        eng.sync()
        t0 = time.perf_counter()
        run(lab, skels, anisotropy=an, _stats=stats, walk=walk)
        stats["wall_s"] = time.perf_counter() - t0
        out.append(stats)
    return out


plain_rows = timed(False) if fill_holes and name == "shells" else None
rows = timed(fill_holes)
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
import hashlib
import numpy as np
digest = hashlib.sha256(b"".join(np.ascontiguousarray(s.cross_sectional_area).tobytes() + np.ascontiguousarray(s.cross_sectional_area_contacts).tobytes()
                                 for s in skels.values())).hexdigest()[:16]
spread = lambda key: (min(r[key] for r in rows) * 1e3, max(r[key] for r in rows) * 1e3)
print("  walk=%s: wall %.1f ms, prepare_s %.1f ms (%.1f .. %.1f), kernel %.2f ms; walk_s %.1f ms, pack_s %.1f ms, %d paths, %d skeletons walked by "
      "the host; areas and contacts sha256 %s" % ((walk, wall * 1e3, med("prepare_s") * 1e3) + spread("prepare_s") + (
          kernel_ms, statistics.median(r.get("walk_s", 0.0) for r in rows) * 1e3, statistics.median(r.get("pack_s", 0.0) for r in rows) * 1e3,
          last.get("paths", 0), last.get("walk_host", 0), digest)))
result = {"workload": name, "walk": walk, "areas_sha256": digest, "walk_s": statistics.median(r.get("walk_s", 0.0) for r in rows),
          "pack_s": statistics.median(r.get("pack_s", 0.0) for r in rows), "wall_min_s": min(r["wall_s"] for r in rows),
          "wall_max_s": max(r["wall_s"] for r in rows), "prepare_min_s": min(r["prepare_s"] for r in rows),
          "prepare_max_s": max(r["prepare_s"] for r in rows), "occurrences": last["occurrences"], "fill_holes": fill_holes, "skeletons": len(skels), "vertices": nvert, "items": last["items"],
          "rounds": last["rounds"], "wall_s": wall, "kernel_ms": kernel_ms, "prepare_s": med("prepare_s"),
          "first_launch_s": med("first_launch_s"), "finish_s": med("finish_s"), "vertices_per_s": nvert / wall, "waves": last["waves"]}
if fill_holes:
    hmed = lambda key: statistics.median(r["holes"].get(key, 0.0) for r in rows)
    holes = last["holes"]
    print("  fill_holes: %d regions, %d pairs (table %d slots, %d tries); region passes %.2f ms (regions %.2f, table %.2f, pairs %.2f), "
          "compaction %.2f ms; host search %.2f ms; lists %d regions = %.1f KiB, %d labels with holes" % (
              holes["regions"], holes["pairs"], holes["table_capacity"], holes["table_tries"],
              hmed("regions_ms") + hmed("table_ms") + hmed("pairs_ms"), hmed("regions_ms"), hmed("table_ms"), hmed("pairs_ms"),
              hmed("compact_ms"), hmed("enclosed_ms"), holes["csr_regions"], holes["csr_regions"] * 4 / 1024, holes["labels_with_holes"]))
    result.update(regions=holes["regions"], pairs=holes["pairs"], region_passes_ms=hmed("regions_ms") + hmed("table_ms") + hmed("pairs_ms"),
                  compact_ms=hmed("compact_ms"), enclosed_ms=hmed("enclosed_ms"), csr_regions=holes["csr_regions"],
                  labels_with_holes=holes["labels_with_holes"])
if plain_rows is not None:
    plain_ms = statistics.median(r["kernel_ms"] for r in plain_rows)
    print("  kernel per vertex: filled %.3f us over %d items, unfilled %.3f us over %d items (the same vertices; an unfilled seed in a "
          "hole ends at once)" % (1e3 * kernel_ms / nvert, last["items"], 1e3 * plain_ms / nvert, plain_rows[-1]["items"]))
    result.update(unfilled_kernel_ms=plain_ms, unfilled_wall_s=statistics.median(r["wall_s"] for r in plain_rows))
print(json.dumps(result))
