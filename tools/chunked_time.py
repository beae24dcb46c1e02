"""Times skeletonize_chunked on bench.py's volume (default c3, 512^3) cut into chunks of 256^3 (eight boxes of 257^3
at c3), against its two yardsticks on the same tree: kimimaro_amd.skeletonize of the same volume in one piece, and the host stages of
postprocess_many, which are timed one by one here (the function handed to the driver restates postprocess_many with a clock
around every stage; its results are what postprocess_many returns, which is checked on the smaller workloads).  --stages device
(default) restates postprocess_many(stages="device"): remove_dust_many, remove_loops_many, remove_ticks_many, each one pass over all
skeletons, and the join with its parts from components_many; --stages host restates stages="host", the per-skeleton
host functions.  dust_host_decided and loops_host of the device stages are printed with them.

One warm-up skeletonize of the volume, one timed; one skeletonize_chunked.  Printed: the `timings` fields, the stages of the
postprocess in seconds and in microseconds per vertex that goes in, and the vertices that come out.

    python tools/chunked_time.py [c3|c2|mini] [chunk edge, default 256] [lanes, default lanes_for()] [--stages host|device]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import kimimaro_amd
from kimimaro_amd import ops, post
from kimimaro_amd.engine import Engine

argv = list(sys.argv[1:])
which = "device"
if "--stages" in argv:
    at = argv.index("--stages")
    which = argv[at + 1]
    del argv[at:at + 2]
assert which in ("host", "device"), "--stages host|device"
name = argv[0] if len(argv) > 0 else "c3"
edge = int(argv[1]) if len(argv) > 1 else 256
width = int(argv[2]) if len(argv) > 2 else None
eng = Engine()
ops._engine = eng
lab, an = bench.make_volume(name, device=eng.device)
params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
kw = dict(teasar_params=params, anisotropy=an, dust_threshold=1000, fix_borders=True, fix_branching=True, progress=False)

whole_s = []
for _ in range(2):
    eng.sync()
    t0 = time.perf_counter()
    whole = kimimaro_amd.skeletonize(lab, _engine=eng, **kw)
    eng.sync()
    whole_s.append(time.perf_counter() - t0)

stages = {}
stats = {}


def clocked(key, fn, *args, **kwargs):
    t0 = time.perf_counter()
    out = fn(*args, **kwargs)
    stages[key] = stages.get(key, 0.0) + time.perf_counter() - t0
    return out


def staged_device(skeletons, dust_threshold, tick_threshold):
    """post.postprocess_many(stages="device"), stage by stage"""
    cleaned = [clocked("consolidate_s", skeleton.consolidate, True) for skeleton in skeletons]
    cleaned = clocked("remove_dust_s", post.remove_dust_many, cleaned, dust_threshold, stats=stats)
    cleaned = clocked("remove_loops_s", post.remove_loops_many, cleaned, stats=stats)
    joined = clocked("join_s", post.join_close_components_many, cleaned, None, True, timings=stats)
    joined = clocked("remove_ticks_s", post.remove_ticks_many, joined, tick_threshold)
    out = []
    for skeleton, skel in zip(skeletons, joined):
        skel.id = skeleton.id
        out.append(clocked("consolidate_s", skel.consolidate, True))
    return out


def staged_host(skeletons, dust_threshold, tick_threshold):
    """post.postprocess_many(stages="host"), stage by stage"""
    cleaned = []
    for skeleton in skeletons:
        skel = clocked("consolidate_s", skeleton.consolidate, True)
        skel = clocked("remove_dust_s", post.remove_dust, skel, dust_threshold)
        cleaned.append(clocked("remove_loops_s", post.remove_loops, skel))
    joined = clocked("join_s", post.join_close_components_many, cleaned, None, True, timings=stats, parts_from="host")
    out = []
    for skeleton, skel in zip(skeletons, joined):
        skel = clocked("remove_ticks_s", post.remove_ticks, skel, tick_threshold)
        skel.id = skeleton.id
        out.append(clocked("consolidate_s", skel.consolidate, True))
    return out


timings = {}
eng.sync()
t0 = time.perf_counter()
got = kimimaro_amd.skeletonize_chunked(lab, (edge, edge, edge), timings=timings, width=width,
                                       _postprocess=staged_device if which == "device" else staged_host,
                                       **{k: v for k, v in kw.items() if k != "progress"})
eng.sync()
total_s = time.perf_counter() - t0
if lab.size <= 2 ** 24:            # the restated postprocess is the library's (a second full run: small workloads only)
    again = kimimaro_amd.skeletonize_chunked(lab, (edge, edge, edge), width=width, **{k: v for k, v in kw.items() if k != "progress"},
                                             _postprocess=lambda sk, dust, tick: post.postprocess_many(sk, dust, tick, stages=which))
    assert list(again) == list(got) and all(again[k] == got[k] for k in got), "the staged postprocess differs from postprocess_many"

per_vertex = lambda s: 1e6 * s / max(timings["vertices"], 1)
res = dict(timings, workload=name, chunk_edge=edge, total_s=total_s, whole_volume_s=whole_s[-1], whole_volume_first_s=whole_s[0],
           whole_volume_labels=len(whole), whole_volume_vertices=sum(s.vertices.shape[0] for s in whole.values()),
           labels=len(got), vertices_out=sum(s.vertices.shape[0] for s in got.values()), stages=which,
           join_parts_s=stats.get("parts_s", 0.0), components=stats.get("components", 0),
           dust_host_decided=stats.get("dust_host_decided", 0), loops_host=stats.get("loops_host", 0), **stages)
print("CHUNKEDTIME %s as %d^3 chunks: %d boxes, %d fragments, %d vertices -> %d labels, %d vertices" % (
    name, edge, timings["chunks"], timings["fragments"], timings["vertices"], res["labels"], res["vertices_out"]))
print("  skeletonize of the volume in one piece: %.2f s (first call %.2f s), %d labels, %d vertices" % (
    whole_s[-1], whole_s[0], len(whole), res["whole_volume_vertices"]))
print("  skeletonize_chunked: %.2f s = count %.3f + chunks %.2f + place %.3f + fuse %.3f + post %.2f" % (
    total_s, timings["count_s"], timings["chunks_s"], timings["place_s"], timings["fuse_s"], timings["post_s"]))
print("  postprocess stages (%s; of the join %.2f s make its parts; %d components, dust_host_decided %d, loops_host %d): " % (
    which, res["join_parts_s"], res["components"], res["dust_host_decided"], res["loops_host"])
      + ", ".join("%s %.2f s (%.1f us per vertex)" % (k[:-2], v, per_vertex(v)) for k, v in sorted(stages.items())))
print(json.dumps(res))
