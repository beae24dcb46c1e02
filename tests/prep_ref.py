"""The streaming kernels in front of the per-label searches (csrc/prep.hip, kh_level_keys), restated in plain numpy from the
contracts in include/kimi_hip.h -- nothing of the product is imported here.  tests/test_prep_host.py pins every function to an
independent definition (np.bincount, scipy.ndimage, the oracle, Python loops); tests/test_gpu_prep.py compares the kernels with
them bit for bit.

Volumes are (x, y, z) arrays whose linear index is x + sx*(y + sy*z); every per-voxel result is returned flat in that order.
Integers are exact.  Floats are np.float32 arrays and scalars, one rounded operation per statement, in the order of
kimimaro/trace.py:315-356 (compute_pdrf) and dijkstra_invalidation.hpp:310-316 (the flood's key)."""
import numpy as np

NONE = 0xFFFFFFFF                     # the identity of the minima: "no voxel"
PDRF_BASE, PDRF_FINISH = -1, -2       # KH_PDRF_BASE / KH_PDRF_FINISH
PDRF_KEEP_OTHERS = 0x100              # KH_PDRF_KEEP_OTHERS

# The neighbour order of dijkstra_invalidation.hpp:60-124, composed the way that code composes it: the six axis steps, then every
# diagonal and corner as the sum of the axis entries it names.
_AXIS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))           # -x +x -y +y -z +z   (:69-74)
_SUMS = ((0, 2), (0, 3), (1, 2), (1, 3),                                                # xy diagonals        (:88-91)
         (2, 4), (2, 5), (3, 4), (3, 5),                                                # yz diagonals        (:94-97)
         (0, 4), (0, 5), (1, 4), (1, 5),                                                # xz diagonals        (:100-103)
         (0, 2, 4), (1, 2, 4), (0, 3, 4), (0, 2, 5), (1, 3, 4), (1, 2, 5), (0, 3, 5), (1, 3, 5))   # corners  (:116-123)
DIRECTIONS = _AXIS + tuple(tuple(int(sum(_AXIS[a][c] for a in parts)) for c in range(3)) for parts in _SUMS)
assert len(DIRECTIONS) == 26 and len(set(DIRECTIONS)) == 26

# cc3d's voxel-connectivity word, listed BY BIT (cc3d_graphs.hpp, read at dijkstra_invalidation.hpp:152-190): bit b allows the
# step CC3D_STEP_OF_BIT[b] away from the voxel that carries the word.
CC3D_STEP_OF_BIT = (
    (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),                # 0..5    faces
    (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0),                                     # 6..9    xy edges
    (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1),                                       # 10..13  +z edges
    (1, 0, -1), (-1, 0, -1), (0, 1, -1), (0, -1, -1),                                   # 14..17  -z edges
    (1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1),                                     # 18..21  +z corners
    (1, 1, -1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1),                                 # 22..25  -z corners
)
assert sorted(CC3D_STEP_OF_BIT) == sorted(DIRECTIONS)


def _flat(vol):
    """the volume's voxels in linear-index order"""
    return np.asarray(vol).reshape(-1, order="F")


def _shape3(vol):
    return (tuple(np.asarray(vol).shape) + (1, 1, 1))[:3]


def label_stats(lab, dbf, nlabels):
    """kh_label_stats: for every id in [0, nlabels] (counts, dbf_max f32, first_index, xmin, xmax, yz [n1, 4] = ymin ymax zmin zmax),
    all but dbf_max uint32.  Id 0 and ids without a voxel keep the identities: 0, 0.0, NONE, NONE, 0, [NONE, 0, NONE, 0]."""
    sx, sy, sz = _shape3(lab)
    n1 = int(nlabels) + 1
    flat = _flat(lab).astype(np.int64)
    value = _flat(dbf).astype(np.float32)
    index = np.arange(flat.size, dtype=np.int64)
    fg = flat != 0
    ids, index, value = flat[fg], index[fg], value[fg]
    x, y, z = index % sx, (index // sx) % sy, index // (sx * sy)
    counts = np.zeros(n1, dtype=np.int64)
    np.add.at(counts, ids, 1)
    dbf_max = np.zeros(n1, dtype=np.float32)
    np.maximum.at(dbf_max, ids, value)
    least = lambda of: _at(np.minimum, np.full(n1, NONE, dtype=np.int64), ids, of)
    most = lambda of: _at(np.maximum, np.zeros(n1, dtype=np.int64), ids, of)
    yz = np.stack([least(y), most(y), least(z), most(z)], axis=1)
    u32 = lambda a: a.astype(np.uint32)
    return u32(counts), dbf_max, u32(least(index)), u32(least(x)), u32(most(x)), u32(yz)


def _at(ufunc, start, where, values):
    ufunc.at(start, where, values)
    return start


def voxel_lists(lab, slot_of_label):
    """kh_scatter_lists up to the order inside a list: [slot] -> the ascending linear indices (uint32) of the label that
    slot_of_label sends to that slot (-1 = label not selected)"""
    flat = _flat(lab)
    slots = np.asarray(slot_of_label, dtype=np.int64)
    lists = [None] * (int(slots.max()) + 1 if slots.size else 0)
    for label in range(1, slots.size):
        if slots[label] >= 0:
            lists[int(slots[label])] = np.flatnonzero(flat == label).astype(np.uint32)
    return lists


def _pairs(delta, shape):
    """slices (the voxels that have a neighbour at +delta inside the volume, those neighbours)"""
    here = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(delta, shape))
    there = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(delta, shape))
    return here, there


def neighbor_mask(lab):
    """kh_neighbor_mask: bit k = the neighbour at DIRECTIONS[k] is inside the volume and carries the same non-zero label; uint32 per
    voxel, background 0, bits 26..31 clear"""
    lab = np.asarray(lab).reshape(_shape3(lab))
    out = np.zeros(lab.shape, dtype=np.uint32)
    for k, delta in enumerate(DIRECTIONS):
        here, there = _pairs(delta, lab.shape)
        same = (lab[here] == lab[there]) & (lab[here] != 0)
        out[here] |= same.astype(np.uint32) << np.uint32(k)
    return _flat(out)


def allowed_directions(graph):
    """the direction word of a cc3d connectivity word: bit k = the step DIRECTIONS[k] is allowed; bits above 25 of `graph` mean nothing"""
    graph = np.asarray(graph, dtype=np.uint32)
    out = np.zeros(graph.shape, dtype=np.uint32)
    for bit, step in enumerate(CC3D_STEP_OF_BIT):
        out |= ((graph >> np.uint32(bit)) & np.uint32(1)) << np.uint32(DIRECTIONS.index(step))
    return out


def apply_voxel_graph(nbr, graph):
    """kh_apply_voxel_graph -> (nbr', corner_gate): nbr' = nbr & the directions graph[v] allows; corner_gate (uint8) bit j = the yz
    diagonal with corner 18 + j's y and z steps exists in nbr (the word BEFORE the graph) and the graph allows corner 18 + j"""
    nbr = np.asarray(nbr, dtype=np.uint32)
    allowed = allowed_directions(graph)
    gate = np.zeros(nbr.shape, dtype=np.uint32)
    for j in range(8):
        _, dy, dz = DIRECTIONS[18 + j]
        diagonal = DIRECTIONS.index((0, dy, dz))
        both = ((nbr >> np.uint32(diagonal)) & (allowed >> np.uint32(18 + j))) & np.uint32(1)
        gate |= both << np.uint32(j)
    return nbr & allowed, gate.astype(np.uint8)


def _selected(lab, slot_of_label):
    """(is the voxel one of a selected label, its slot or -1), flat"""
    flat = _flat(lab).astype(np.int64)
    slot = np.asarray(slot_of_label, dtype=np.int64)[flat]
    slot[flat == 0] = -1
    return slot >= 0, slot


def alive(lab, slot_of_label):
    """kh_init_alive: uint8 1 where the voxel's label is non-zero and has a slot"""
    return _selected(lab, slot_of_label)[0].astype(np.uint8)


def pdrf(lab, slot_of_label, tasks, dbf, daf, stage, scale, keep=False, pdrf_in=None):
    """kh_pdrf -> (pdrf, daf) as new flat float32 arrays.  tasks: records with "M" and "max_val" per slot; stage: log2 of the
    exponent (0..15), PDRF_BASE or PDRF_FINISH; pdrf_in: the buffer's content before the call (read by PDRF_FINISH, kept at the
    voxels of unselected labels with keep = KH_PDRF_KEEP_OTHERS, which belongs to stages >= 0 only)."""
    f = np.float32
    sel, slot = _selected(lab, slot_of_label)
    assert not (keep and stage < 0)
    out = _flat(pdrf_in).astype(f).copy() if keep else np.full(sel.size, np.inf, dtype=f)
    daf_out = _flat(daf).astype(f).copy()
    M = np.asarray(tasks["M"], dtype=f)[slot[sel]]
    max_daf = np.asarray(tasks["max_val"], dtype=f)[slot[sel]]
    with np.errstate(all="ignore"):
        if stage != PDRF_FINISH:
            p = _flat(dbf).astype(f)[sel] * M                 # np.multiply(DBF, M)          trace.py:341
            p = f(1) - p                                      # np.subtract(f(1), PDRF)      trace.py:342
        else:
            p = _flat(pdrf_in).astype(f)[sel]                 # the host's np.power result   trace.py:347
        if stage == PDRF_BASE:
            out[sel] = p
            return out, daf_out
        for _ in range(max(stage, 0)):
            p = p * p                                         # PDRF *= PDRF                 trace.py:344-345
        p = p * f(scale)                                      # PDRF *= f(pdrf_scale)        trace.py:349
        d = daf_out[sel]
        d[d == np.inf] = f(0)                                 # inf2zero                     trace.py:146
        scaled = max_daf != 0                                 # if max_daf != 0:             trace.py:352
        inverse = f(1) / max_daf[scaled]                      # (1 / max_daf), float32 scalar
        d[scaled] = d[scaled] * inverse                       # DAF *= ...                   trace.py:353
        p[scaled] = p[scaled] + d[scaled]                     # PDRF += DAF                  trace.py:354
    assert p.dtype == f and d.dtype == f
    out[sel] = p
    daf_out[sel] = d
    return out, daf_out


def level_keys(dims, w):
    """kh_level_keys: float32 [ra, rb, rc], keys[a, b, c] = sqrt(fl(fl((wx*a)^2 + (wy*b)^2) + (wz*c)^2)), every operation rounded to
    float32 (dijkstra_invalidation.hpp:310-316)"""
    w = [np.float32(v) for v in w]
    a = (np.arange(dims[0], dtype=np.float32) * w[0]) ** 2
    b = (np.arange(dims[1], dtype=np.float32) * w[1]) ** 2
    c = (np.arange(dims[2], dtype=np.float32) * w[2]) ** 2
    s = ((a[:, None, None] + b[None, :, None]).astype(np.float32) + c[None, None, :]).astype(np.float32)
    return np.sqrt(s).astype(np.float32)


# ---- the label volumes the two test files share -------------------------------------------------------------------------------
PATTERNS = ("solid", "alternating", "voronoi", "last_voxel")


def pattern_labels(shape, pattern, seed=0):
    """int64 (x, y, z) volume with ids <= 7:
       solid        one label everywhere: a run of equal labels continues across every row start;
       alternating  a new id at every voxel, among three ids and 0;
       voronoi      blobs (shapes.voronoi_labels) with 5 % background;
       last_voxel   the last voxel of the volume is foreground and the first background, short runs in between."""
    nvox = int(np.prod(shape))
    i = np.arange(nvox, dtype=np.int64)
    if pattern == "solid":
        flat = np.full(nvox, 3, dtype=np.int64)
    elif pattern == "alternating":
        flat = np.array([2, 0, 5, 7], dtype=np.int64)[(i + i // 5) % 4]
    elif pattern == "voronoi":
        from shapes import voronoi_labels
        blobs = voronoi_labels(shape, 5, seed=seed + 17, pts_per_label=2, step=3.0).reshape(-1, order="F")
        flat = np.unique(blobs, return_inverse=True)[1].reshape(-1).astype(np.int64) + 1
        flat[np.random.default_rng(seed).random(nvox) < 0.05] = 0
        if not flat.any():
            flat[-1] = 1
    elif pattern == "last_voxel":
        flat = np.where(i % 10 < 3, 1, 0).astype(np.int64)
        flat[0] = 0
        flat[-1] = 2
    else:
        raise ValueError(pattern)
    return flat.reshape(shape, order="F")
