"""Times the two routes of fill_holes on bench.py's volume (default c3), resident in HBM: the per-label loop
kimimaro_amd.intake.fill_all_holes_device and the one-pass route Engine.fill_all_holes, each on its own copy of the same component
volume (kh_ccl26 of the workload).  Two volumes: the workload as it is (dense neuropil: nothing to fill), and the workload with a few
hundred closed pockets planted inside its labels (background or a foreign label in a 3 x 3 x 3 box), so that something is filled.

After a warm-up call each route runs `runs` times (default 5), the two taking turns; reported are the median and the spread of the
wall time (host clock around the call, which ends in a device-to-host copy on either route), and for the new route the HIP-event time of every pass, the
host's share, the numbers of regions and pairs and the size of the pair table.  The loop stops sampling early when it has used
`loop_budget` seconds (default 240) -- the number of samples taken is printed.  Both routes must leave the same volume and count.

    python tools/fill_holes_time.py [c3] [runs] [loop_budget_s]
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
from kimimaro_amd import intake
from kimimaro_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
loop_budget = float(sys.argv[3]) if len(sys.argv) > 3 else 240.0
eng = Engine()
t = eng.torch
lab, an = bench.make_volume(name, device=eng.device)
shape = tuple(int(v) for v in lab.shape)


def plant_pockets(lab, want=300, seed=5):
    """3 x 3 x 3 boxes of background (even ones) or of a label of their own (odd ones) where a 5 x 5 x 5 box holds one label"""
    rng = np.random.default_rng(seed)
    out = lab.copy(order="F")
    top = int(lab.max())
    planted = 0
    for _ in range(200 * want):
        c = [int(rng.integers(3, s - 3)) for s in shape]
        box = lab[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3]
        now = out[c[0] - 2:c[0] + 3, c[1] - 2:c[1] + 3, c[2] - 2:c[2] + 3]
        if box[0, 0, 0] == 0 or (box != box[0, 0, 0]).any() or (now != box).any():
            continue
        out[c[0] - 1:c[0] + 2, c[1] - 1:c[1] + 2, c[2] - 1:c[2] + 2] = 0 if planted % 2 == 0 else top + 1 + planted
        planted += 1
        if planted == want:
            break
    return out, planted


def measure(tag, volume):
    d_cc, ncomp, _ = eng.ccl(volume)
    eng.sync()

    def call(fn, k, walls):
        d = d_cc.clone()
        eng.sync()
        t0 = time.perf_counter()
        n = fn(d)
        eng.sync()
        dt = time.perf_counter() - t0
        if k:                                                        # the first call is the warm-up
            walls.append(dt)
        print("  %s %s call %d: %.1f ms" % (tag, fn.__name__, k, dt * 1e3), flush=True)
        return d, n

    def loop(d):
        return intake.fill_all_holes_device(eng, d, shape, ncomp)

    rows = []

    def one_pass(d):
        stats = {}
        n = eng.fill_all_holes(d, 4, shape, stats=stats)
        rows.append(stats)
        return n

    # the two routes take turns (what else the machine does then hits both alike)
    new_walls, old_walls, spent = [], [], 0.0
    for k in range(runs + 1):
        d_new, n_new = call(one_pass, k, new_walls)
        if k < 2 or spent < loop_budget:
            t0 = time.perf_counter()
            d_old, n_old = call(loop, k, old_walls)
            spent += time.perf_counter() - t0
    same = bool(t.equal(d_new, d_old)) and n_new == n_old
    rows = rows[1:]
    med = lambda key: statistics.median(float(r[key]) for r in rows)
    last = rows[-1]
    res = {
        "volume": tag, "workload": name, "components": ncomp, "filled": n_new, "routes_agree": same,
        "loop_ms": statistics.median(old_walls) * 1e3, "loop_min_ms": min(old_walls) * 1e3, "loop_max_ms": max(old_walls) * 1e3,
        "loop_samples": len(old_walls),
        "one_pass_ms": statistics.median(new_walls) * 1e3, "one_pass_min_ms": min(new_walls) * 1e3, "one_pass_max_ms": max(new_walls) * 1e3,
        "one_pass_samples": len(new_walls),
        "regions_ms": med("regions_ms"), "table_ms": med("table_ms"), "pairs_ms": med("pairs_ms"), "apply_ms": med("apply_ms"),
        "compact_ms": med("compact_ms"), "resolve_ms": med("resolve_ms"),
        "regions": last["regions"], "pairs": last["pairs"], "table_capacity": last["table_capacity"], "table_tries": last["table_tries"],
        "labels": last["labels"],
    }
    print("FILLTIME %s/%s: %d components, %d voxels filled, routes agree: %s" % (name, tag, ncomp, n_new, same))
    print("  loop      median of %d: %.1f ms (%.1f .. %.1f)" % (len(old_walls), res["loop_ms"], res["loop_min_ms"], res["loop_max_ms"]))
    print("  one pass  median of %d: %.1f ms (%.1f .. %.1f) = kernels: regions %.2f + table %.2f + pairs %.2f + apply %.2f ms; host: "
          "copies %.2f + resolver %.2f ms" % (len(new_walls), res["one_pass_ms"], res["one_pass_min_ms"], res["one_pass_max_ms"],
                                              res["regions_ms"], res["table_ms"], res["pairs_ms"], res["apply_ms"], res["compact_ms"],
                                              res["resolve_ms"]))
    print("  %d regions, %d pairs, pair table of %d slots (%d tries)" % (res["regions"], res["pairs"], res["table_capacity"],
                                                                       res["table_tries"]))
    print(json.dumps(res), flush=True)
    assert same, "the two routes disagree"
    return res


results = [measure("plain", lab)]
pocketed, planted = plant_pockets(lab)
print("planted %d pockets" % planted)
results.append(measure("pockets", pocketed))
print("| volume | components | filled | loop ms (min .. max, n) | one pass ms (min .. max, n) | regions | table | pairs | apply | host copies | "
      "resolver | regions | pairs | table slots |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in results:
    print("| %s %s | %d | %d | %.0f (%.0f .. %.0f, %d) | %.1f (%.1f .. %.1f, %d) | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f | %d | %d | %d |" % (
        name, r["volume"], r["components"], r["filled"], r["loop_ms"], r["loop_min_ms"], r["loop_max_ms"], r["loop_samples"],
        r["one_pass_ms"], r["one_pass_min_ms"], r["one_pass_max_ms"], r["one_pass_samples"], r["regions_ms"], r["table_ms"],
        r["pairs_ms"], r["apply_ms"], r["compact_ms"], r["resolve_ms"], r["regions"], r["pairs"], r["table_capacity"]))
