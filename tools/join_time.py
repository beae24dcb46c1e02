"""Times join_close_components_many (csrc/join.hip + kh_host_join_plan) against post.join_close_components, the
host function it restates, on the random-walk fragments of tests/join_ref.py (denom=1024, extent=64, rmax=4, seed=5):

  64 fragments of at most 200 vertices, 200 fragments of at most 400; each with radius=inf and with restrict_by_radius=True, the
  device path dense (split=False) and, where the bound is finite, cut into clusters first (split=True);

and, device path only, on a group no single table can hold (seed=6, extent=500, rmax=2: clusters stay small):

  20 000 fragments of at most 98 vertices (about 50), restrict_by_radius=True, split=None.

Host function: one run (wall clock).  Device path: one warm-up call, then REPEATS calls (3 for the large group) with the device
synchronised around each; the median wall clock of the public function and, from the same calls, the medians of its parts: the
broad phase (HIP events around kh_part_clusters), the kernel (HIP events around kh_part_gaps), the tables' copy to the host,
kh_host_join_plan.  The results are compared for equality: device against host, split against dense.

    python tools/join_time.py [small] [--tree DIR]

small: the 64-fragment input only.  --tree DIR: time the package of another checkout (built there) with this script, to compare two
commits in one session; a tree whose join_close_components_many has no `split` runs the dense rows only.
"""
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
TREE = os.path.abspath(args[args.index("--tree") + 1]) if "--tree" in args else ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import join_ref
from kimimaro_amd import ops, post
from kimimaro_amd.engine import Engine

REPEATS = 5
SIZES = [(64, 200), (200, 400)]
LARGE = dict(nfrag=20000, nvert=98, extent=500, rmax=2, denom=1024)
if "small" in args:
    SIZES = SIZES[:1]
HAS_SPLIT = "split" in inspect.signature(post.join_close_components_many).parameters
eng = Engine()
ops._engine = eng
results = []


def timed(frags, repeats, **kwargs):
    """-> (the result, a row of medians) of join_close_components_many([frags], **kwargs)"""
    post.join_close_components_many([frags], **kwargs)                                            # warm-up
    wall, parts = [], []
    for _ in range(repeats):
        timings = {}
        eng.sync()
        t0 = time.perf_counter()
        got = post.join_close_components_many([frags], timings=timings, **kwargs)[0]
        eng.sync()
        wall.append(time.perf_counter() - t0)
        parts.append(timings)
    row = {"device_path_s": statistics.median(wall), "device_path_min_s": min(wall), "device_path_max_s": max(wall), "repeats": repeats}
    for key in ("cluster_ms", "kernel_ms", "copy_s", "plan_s", "clusters", "largest_cluster"):
        row[key] = statistics.median(s.get(key, 0) for s in parts)
    return got, row


def report(row):
    results.append(row)
    print("JOINTIME %d fragments, %d parts, %d vertices, restrict_by_radius=%s, split=%s: host %s s; device path %.4f s (min %.4f, max "
          "%.4f of %d): clusters %.3f ms (%d, largest %d), kernel %.3f ms, table copy %.4f s, plan %.4f s; equal: %s" % (
              row["fragments"], row["parts"], row["vertices"], row["restrict_by_radius"], row["split"],
              "-" if row["host_s"] is None else "%.3f" % row["host_s"], row["device_path_s"], row["device_path_min_s"],
              row["device_path_max_s"], row["repeats"], row["cluster_ms"], row["clusters"], row["largest_cluster"], row["kernel_ms"],
              row["copy_s"], row["plan_s"], row["equal"]), flush=True)


for nfrag, nvert in SIZES:
    frags = join_ref.fragments(5, nfrag, nvert, extent=64, rmax=4, denom=1024)
    nparts = len(post.join_parts(frags))
    vertices = sum(p.vertices.shape[0] for p in post.join_parts(frags))
    for radius, restrict in ((np.inf, False), (np.inf, True)):
        t0 = time.perf_counter()
        want = post.join_close_components(frags, radius=radius, restrict_by_radius=restrict)
        host_s = time.perf_counter() - t0
        for split in ((False, True) if HAS_SPLIT and restrict else (False,)):
            got, row = timed(frags, REPEATS, radius=radius, restrict_by_radius=restrict, **({"split": split} if HAS_SPLIT else {}))
            row.update(fragments=nfrag, parts=nparts, vertices=vertices, restrict_by_radius=restrict, split=split, host_s=host_s,
                       equal=bool(join_ref.same(got, want)), edges_added=int(got.edges.shape[0]))
            report(row)
if HAS_SPLIT and "small" not in args:
    frags = join_ref.fragments(6, **LARGE)
    parts = post.join_parts(frags)
    got, row = timed(frags, 3, restrict_by_radius=True, split=None)
    row.update(fragments=LARGE["nfrag"], parts=len(parts), vertices=sum(p.vertices.shape[0] for p in parts), restrict_by_radius=True,
               split=None, host_s=None, equal=None, edges_added=int(got.edges.shape[0] - sum(p.edges.shape[0] for p in parts)))
    report(row)
print(json.dumps({"tree": TREE, "rows": results}))
