"""Times join_close_components_many (csrc/join.hip + kh_host_join_plan) against post.join_close_components, the
host function it restates, on the random-walk fragments of tests/join_ref.py (denom=1024, extent=64, rmax=4, seed=5):

  64 fragments of at most 200 vertices, 200 fragments of at most 400; each with radius=inf and with restrict_by_radius=True.

Host function: one run (wall clock).  Device path: one warm-up call, then REPEATS calls with the device synchronised around each; the
median wall clock of the public function and, from the same calls, the medians of its parts: the kernel (HIP events around
kh_part_gaps), the tables' copy to the host, kh_host_join_plan.  The two results are compared for equality.

    python tools/join_time.py [small]          (small: the 64-fragment input only)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import join_ref
from kimimaro_amd import ops, post
from kimimaro_amd.engine import Engine

REPEATS = 5
SIZES = [(64, 200), (200, 400)]
if "small" in sys.argv[1:]:
    SIZES = SIZES[:1]
eng = Engine()
ops._engine = eng
results = []
for nfrag, nvert in SIZES:
    frags = join_ref.fragments(5, nfrag, nvert, extent=64, rmax=4, denom=1024)
    nparts = len(post.join_parts(frags))
    vertices = sum(p.vertices.shape[0] for p in post.join_parts(frags))
    for radius, restrict in ((np.inf, False), (np.inf, True)):
        t0 = time.perf_counter()
        want = post.join_close_components(frags, radius=radius, restrict_by_radius=restrict)
        host_s = time.perf_counter() - t0
        post.join_close_components_many([frags], radius=radius, restrict_by_radius=restrict)        # warm-up
        wall, split = [], []
        for _ in range(REPEATS):
            timings = {}
            eng.sync()
            t0 = time.perf_counter()
            got = post.join_close_components_many([frags], radius=radius, restrict_by_radius=restrict, timings=timings)[0]
            eng.sync()
            wall.append(time.perf_counter() - t0)
            split.append(timings)
        row = {"fragments": nfrag, "parts": nparts, "vertices": vertices, "restrict_by_radius": restrict, "host_s": host_s,
               "device_path_s": statistics.median(wall), "device_path_min_s": min(wall), "device_path_max_s": max(wall),
               "kernel_ms": statistics.median(s["kernel_ms"] for s in split), "copy_s": statistics.median(s["copy_s"] for s in split),
               "plan_s": statistics.median(s["plan_s"] for s in split), "equal": bool(join_ref.same(got, want)),
               "edges_added": int(got.edges.shape[0])}
        results.append(row)
        print("JOINTIME %d fragments, %d parts, %d vertices, restrict_by_radius=%s: host %.3f s; device path %.4f s (min %.4f, max %.4f"
              " of %d): kernel %.3f ms, table copy %.4f s, plan %.4f s; equal: %s" % (
                  nfrag, nparts, vertices, restrict, host_s, row["device_path_s"], row["device_path_min_s"], row["device_path_max_s"],
                  REPEATS, row["kernel_ms"], row["copy_s"], row["plan_s"], row["equal"]), flush=True)
print(json.dumps(results))
