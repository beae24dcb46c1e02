"""Times the two point queries of csrc/points.hip on bench.py's volume (default c3, 512^3) against the CPU statements of
tests/points_ref.py and, where oracle/_ref is present, against the reference's compiled extract_edges_from_binary_image:

  synapses_to_targets   2 000 synapses over 200 labels of the volume (uniform float64 centroids, four swc labels);
  extract_edges         the skeleton voxels of that volume (skeletonize's vertices) rasterised into a binary image.

GPU side: one warm-up call, then the median of REPEATS calls, the device synchronised around every call (wall clock of the public
function: uploads of the tables, kernels, scans, downloads of the results).  The CPU side runs once.

    python tools/points_time.py [c3] [noref]
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
import bench
import kimimaro_amd
from kimimaro_amd import ops
from kimimaro_amd.engine import Engine

REPEATS = 5
name = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "noref" else "c3"
with_ref = "noref" not in sys.argv[1:]
eng = Engine()
ops._engine = eng
torch = eng.torch
lab, an = bench.make_volume(name, device=eng.device)
shape = lab.shape
print("POINTSTIME %s %s, %d labels" % (name, shape, len(np.unique(lab))), flush=True)


def gpu_median(fn):
    fn()                                            # warm-up (allocator, code objects)
    times = []
    for _ in range(REPEATS):
        eng.sync()
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def cpu_once(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


# the volume as a tensor on the device, indexed [x, y, z], Fortran ordered in memory (no copy inside the calls)
d_lab = torch.from_numpy(lab.T.view(np.int32)).to(eng.device).permute(2, 1, 0)

rng = np.random.default_rng(7)
chosen = rng.choice(np.unique(lab), size=200, replace=False).tolist()
synapses = {int(L): [(tuple(rng.uniform(0, np.array(shape)).tolist()), k % 4) for k in range(10)] for L in chosen}
t_dev, got = gpu_median(lambda: kimimaro_amd.synapses_to_targets(d_lab, synapses))
t_host, got_host = gpu_median(lambda: kimimaro_amd.synapses_to_targets(lab, synapses))
assert list(got.items()) == list(got_host.items())
result = {"workload": name, "synapses": 2000, "labels": 200, "targets": len(got), "synapses_gpu_resident_s": t_dev,
          "synapses_gpu_from_host_s": t_host}
print("  synapses_to_targets: %d targets; volume resident %.4f s, uploaded from the host %.4f s (median of %d)" % (
    len(got), t_dev, t_host, REPEATS), flush=True)
if with_ref:
    import points_ref
    t_ref, want = cpu_once(lambda: points_ref.synapses_to_targets(lab, synapses))
    result.update(synapses_ref_s=t_ref, synapses_equal=list(got.items()) == list(want.items()))
    print("  points_ref.synapses_to_targets %.2f s -> %.0f x (resident), equal: %s" % (t_ref, t_ref / t_dev, result["synapses_equal"]),
          flush=True)

skels = kimimaro_amd.skeletonize(lab, anisotropy=an, dust_threshold=1000, fix_borders=True, progress=False, _engine=eng)
image = np.zeros(shape, dtype=np.uint8, order="F")
for s in skels.values():
    v = np.round(s.vertices / np.asarray(an, dtype=np.float32)).astype(np.int64)
    image[v[:, 0], v[:, 1], v[:, 2]] = 1
d_img = torch.from_numpy(image.T).to(eng.device).permute(2, 1, 0)
t_dev, (verts, edges) = gpu_median(lambda: ops.extract_edges_from_binary_image(d_img))
t_host, _ = gpu_median(lambda: ops.extract_edges_from_binary_image(image))
result.update(skeleton_voxels=int(image.sum()), vertices=int(len(verts)), edges=int(len(edges)), edges_gpu_resident_s=t_dev,
              edges_gpu_from_host_s=t_host)
print("  extract_edges: %d skeleton voxels -> %d vertices, %d edges; image resident %.4f s, uploaded from the host %.4f s" % (
    int(image.sum()), len(verts), len(edges), t_dev, t_host), flush=True)
if with_ref:
    t_ref, (want_v, want_e) = cpu_once(lambda: points_ref.extract_edges(image))
    result.update(edges_ref_s=t_ref, edges_equal=bool(np.array_equal(verts, want_v) and np.array_equal(edges, want_e)))
    print("  points_ref.extract_edges %.2f s -> %.0f x (resident), equal: %s" % (t_ref, t_ref / t_dev, result["edges_equal"]), flush=True)
    from oracle import build_ref
    refmod = build_ref.load()
    if refmod is not None:
        t_c, (ref_v, ref_e) = cpu_once(lambda: refmod.extract_edges_from_binary_image(image))
        result.update(edges_compiled_reference_s=t_c, edges_compiled_reference_count=int(len(ref_e)))
        print("  compiled reference extract_edges_from_binary_image %.2f s -> %.0f x (resident), %d edges" % (
            t_c, t_c / t_dev, len(ref_e)), flush=True)
    else:
        print("  compiled reference: oracle/_ref is absent here", flush=True)
print(json.dumps(result))
