"""Times kimimaro_amd.oversegment on bench.py's volume (default c3): skeletonizes it, then segments it with the skeletons it has just
made, HIP events per phase on the launch stream (mask, seed, distance sweeps, feature sweeps, renumber), sweeps, bricks visited per
sweep, and the bytes the sweeps move against 8 TB/s.  With `ref` as second argument also the seconds tests/feature_ref.py needs for
the largest case of tests/test_gpu_oversegment.py next to the GPU's time for the same call -- the only yardstick there is.

    python tools/oversegment_time.py [c3] [ref]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
import kimimaro_amd
from kimimaro_amd import _abi
from kimimaro_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "c3"
eng = Engine()
lab, an = bench.make_volume(name, device=eng.device)
t0 = time.perf_counter()
skels = kimimaro_amd.skeletonize(lab, anisotropy=an, dust_threshold=1000, fix_borders=True, progress=False, _engine=eng)
eng.sync()
t_skel = time.perf_counter() - t0
nvert = sum(len(s.vertices) for s in skels.values())
kimimaro_amd.oversegment(lab, skels, anisotropy=an)                    # warm-up (allocator, code objects)
stats = {}
t0 = time.perf_counter()
feats, out = kimimaro_amd.oversegment(lab, skels, anisotropy=an, _stats=stats)
wall = time.perf_counter() - t0
ms = stats["ms"]
nvox = stats["nvox"]
brick_voxels = _abi.BRICK[0] * _abi.BRICK[1] * _abi.BRICK[2]
# per visited voxel a sweep reads its mask word (4 B) and its own value (4 B; the feature phase: distance + feature, 8 B); the
# neighbour words come from the same bricks and their rims (cache); a store only where the value went down
bytes_d = sum(stats["distance_bricks"]) * brick_voxels * 8
bytes_f = sum(stats["feature_bricks"]) * brick_voxels * 12
print("OVERSEGTIME %s: %d skeletons, %d vertices, %d segments (%s); skeletonize %.2f s, oversegment wall %.3f s" % (
    name, len(skels), nvert, int(feats.max()), feats.dtype, t_skel, wall))
print("  phases (ms): " + ", ".join("%s %.3f" % (k, ms.get(k, 0.0)) for k in ("mask", "seed", "distance", "feature", "renumber")))
print("  distance: %d sweeps, bricks visited per sweep %s -> %.1f GB/s = %.4f of 8 TB/s" % (
    stats["distance_sweeps"], stats["distance_bricks"], bytes_d / (ms["distance"] * 1e-3) / 1e9, bytes_d / (ms["distance"] * 1e-3) / 8e12))
print("  feature:  %d sweeps, bricks visited per sweep %s -> %.1f GB/s = %.4f of 8 TB/s" % (
    stats["feature_sweeps"], stats["feature_bricks"], bytes_f / (ms["feature"] * 1e-3) / 1e9, bytes_f / (ms["feature"] * 1e-3) / 8e12))
print("  bricks in the volume: %d of %d voxels" % (stats["bricks"], brick_voxels))
print(json.dumps({"workload": name, "skeletons": len(skels), "vertices": nvert, "segments": int(feats.max()), "wall_s": wall,
                  "ms": ms, "distance_sweeps": stats["distance_sweeps"], "feature_sweeps": stats["feature_sweeps"],
                  "distance_bricks": stats["distance_bricks"], "feature_bricks": stats["feature_bricks"], "bricks": stats["bricks"]}))

if "ref" in sys.argv[2:]:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import feature_ref
    from shapes import voronoi_labels
    an2 = (16, 16, 40)
    lab2 = voronoi_labels((64, 64, 48), 10, seed=5, pts_per_label=5, step=10.0, anisotropy=an2)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 64
    sk2 = kimimaro_amd.skeletonize(lab2, params, anisotropy=an2, dust_threshold=200, fix_borders=True, progress=False, _engine=eng)
    t0 = time.perf_counter()
    want, _, _ = feature_ref.oversegment(lab2, sk2, an2)
    t_ref = time.perf_counter() - t0
    kimimaro_amd.oversegment(lab2, sk2, anisotropy=an2)
    st2 = {}
    t0 = time.perf_counter()
    got, _ = kimimaro_amd.oversegment(lab2, sk2, anisotropy=an2, _stats=st2)
    t_gpu = time.perf_counter() - t0
    assert np.array_equal(got, want)
    print("OVERSEGREF 64x64x48, %d skeletons: feature_ref %.3f s, oversegment %.4f s wall (kernels %.3f ms), equal" % (
        len(sk2), t_ref, t_gpu, sum(st2["ms"].values())))
