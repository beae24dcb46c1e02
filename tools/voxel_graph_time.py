"""Times kh_voxel_graph (csrc/graph.hip) on bench.py's volume (default c3, 512^3 uint32) by HIP events, next to kh_neighbor_mask on
the same volume in the same process -- the kernel that has done the same 26 comparisons per voxel since round 1, from scalar loads:

  plain        kh_voxel_graph, connectivity 26, no pairs;
  pairs_lds    the same with a table of 1 500 label pairs (searched in LDS);
  pairs_global the same with 4 000 pairs (beyond KH_GRAPH_LDS_PAIRS: searched in global memory);
  nbrmask      kh_neighbor_mask.

Half of each table are pairs of labels that do touch in the volume, so that searches end both ways.  WARMUP rounds, then REPEATS
rounds; a round runs the four kernels one after the other (alternating, so that a drift of the clock or a neighbour on the machine
hits all of them), each between two events on the stream; per kernel the median, the smallest and the largest time are reported,
with the bytes it has to move -- nvox * (label_bytes + 4) -- over the median and that rate's share of the 8 TB/s HBM peak.

    python tools/voxel_graph_time.py [c3]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench
from kimimaro_amd import _abi, ops
from kimimaro_amd.engine import Engine

WARMUP, REPEATS = 3, 15
HBM_PEAK = 8.0e12
name = sys.argv[1] if len(sys.argv) > 1 else "c3"
eng = Engine()
torch = eng.torch
lab, _ = bench.make_volume(name, device=eng.device)
lab = np.asfortranarray(lab)
shape = tuple(int(v) for v in lab.shape)
itemsize = lab.dtype.itemsize
nvox = lab.size
print("GRAPHTIME %s %s %s, %d labels" % (name, shape, lab.dtype, len(np.unique(lab))), flush=True)

d_lab = eng.to_device(lab.view("u%d" % itemsize))
d_out = eng.empty(nvox, torch.int32)


def table(rows, seed):
    """`rows` pairs: half of them labels that are x neighbours somewhere in the volume, half random labels"""
    rng = np.random.default_rng(seed)
    a, b = lab[:-1].reshape(-1), lab[1:].reshape(-1)
    touching = np.flatnonzero((a != b) & (a != 0) & (b != 0))
    pick = rng.choice(touching, size=min(rows // 2, touching.size), replace=False)
    ids = np.unique(lab)
    pairs = np.concatenate([np.stack([a[pick], b[pick]], axis=1).astype(np.int64), rng.choice(ids[ids != 0], size=(rows - pick.size, 2)).astype(np.int64)])
    host = ops.merge_pairs(pairs, (0, int(np.iinfo(lab.dtype).max)), itemsize)
    return host.shape[0], torch.from_numpy(host.reshape(-1).view(np.int64)).to(eng.device)


n_lds, d_lds = table(1500, 1)
n_glb, d_glb = table(4000, 2)
assert n_lds <= _abi.GRAPH_LDS_PAIRS < n_glb
P, st = eng.ptr, eng.stream()
sx, sy, sz = shape
runs = {
    "plain": lambda: eng.lib.kh_voxel_graph(P(d_lab), itemsize, sx, sy, sz, 26, None, 0, P(d_out), st),
    "pairs_lds": lambda: eng.lib.kh_voxel_graph(P(d_lab), itemsize, sx, sy, sz, 26, P(d_lds), n_lds, P(d_out), st),
    "pairs_global": lambda: eng.lib.kh_voxel_graph(P(d_lab), itemsize, sx, sy, sz, 26, P(d_glb), n_glb, P(d_out), st),
    "nbrmask": lambda: eng.lib.kh_neighbor_mask(P(d_lab), itemsize, sx, sy, sz, P(d_out), st),
}
times = {k: [] for k in runs}
for rnd in range(WARMUP + REPEATS):
    for k, fn in runs.items():
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _abi.check(fn())
        end.record()
        end.synchronize()
        if rnd >= WARMUP:
            times[k].append(start.elapsed_time(end))

moved = nvox * (itemsize + 4)
result = {"workload": name, "shape": shape, "label_bytes": itemsize, "bytes_moved": moved, "rows_lds": n_lds, "rows_global": n_glb,
          "warmup": WARMUP, "repeats": REPEATS}
for k, ms in times.items():
    med = statistics.median(ms)
    result[k] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "GB_per_s": moved / med / 1e6, "share_of_8TBps": moved / (med * 1e-3) / HBM_PEAK}
    print("  %-13s median %.3f ms (min %.3f, max %.3f): %.0f GB/s of the %.2f GB it has to move = %.1f %% of 8 TB/s" % (
        k, med, min(ms), max(ms), moved / med / 1e6, moved / 1e9, 100 * moved / (med * 1e-3) / HBM_PEAK), flush=True)
print(json.dumps(result))
