"""Restatements of kimimaro.intake.fill_all_holes (kimimaro/intake.py:747-795) in numpy and scipy, for the tests of the one-pass
route.  Two of them, which tests/test_fill_holes_host.py holds against each other:

  sequential(cc)   the reference's loop as it stands: scipy.ndimage.find_objects once, then per label in ascending order the crop
                   `cc[slices] == label`, scipy.ndimage.binary_fill_holes on it (fill_voids.fill's definition: background that no
                   face-connected path joins to a face of the crop), the labels under the fill leave the live set, the crop is painted.
  static(cc)       the form the product implements: hole(L) = the 6-connected components of `cc != L` ON THE INPUT that own no
                   voxel on a face of the volume; then the ascending rule with a dead set.

Both work on arrays of any dimensionality (an axis of extent 1 puts every voxel on a face) and on sparse values: the values are
ranked first, which keeps their order (find_objects indexes a list by value).  Also here: the region table and the adjacency pairs
of a volume built by numpy (region_graph), the input of kh_host_resolve_holes, and the random volumes the tests share."""
import numpy as np
import scipy.ndimage as ndi

PROCESSED, FILLED, KILLED = 1, 2, 4        # kimimaro_amd._abi.HOLES_*


def _ranked(cc):
    """(values ascending with 0 in front, the volume as ranks into them: 0 stays 0)"""
    cc = np.asarray(cc)
    if cc.dtype == np.bool_:
        cc = cc.view(np.uint8)
    nz = np.unique(cc)
    nz = nz[nz != 0]
    dense = np.searchsorted(nz, cc) + 1
    dense[cc == 0] = 0
    return np.concatenate([np.zeros(1, dtype=cc.dtype), nz]), dense.astype(np.int64)


def _finish(cc, values, dense, count, state):
    out = values[dense]
    if np.asarray(cc).dtype == np.bool_:
        out = out.view(np.bool_)
    return out, int(count), {int(values[k]): int(state[k]) for k in range(1, len(values))}


def sequential(cc):
    """-> (filled volume, fill count, {label: PROCESSED | FILLED | KILLED bits})"""
    values, dense = _ranked(cc)
    nlab = len(values) - 1
    state = np.zeros(nlab + 1, dtype=np.int64)
    live = set(range(1, nlab + 1))
    all_slices = ndi.find_objects(dense, max_label=max(nlab, 1))
    count = 0
    for label in range(1, nlab + 1):
        if label not in live:
            continue
        slices = all_slices[label - 1]
        if slices is None:
            continue
        state[label] |= PROCESSED
        binary = dense[slices] == label
        filled = ndi.binary_fill_holes(binary)
        n = int(filled.sum()) - int(binary.sum())
        count += n
        if n == 0:
            continue
        state[label] |= FILLED
        under = set(np.unique(dense[slices] * filled).tolist()) - {0, label}
        for other in under:
            state[other] |= KILLED
        live -= under
        dense[slices] = dense[slices] * ~filled + label * filled
    return _finish(cc, values, dense, count, state)


def _on_a_face(ids):
    found = set()
    for axis in range(ids.ndim):
        for index in (0, -1):
            found.update(np.unique(np.take(ids, index, axis=axis)).tolist())
    return found


def static(cc):
    """-> (filled volume, fill count, {label: bits}), from holes computed on the INPUT alone"""
    values, dense = _ranked(cc)
    nlab = len(values) - 1
    holes = {}
    for label in range(1, nlab + 1):
        comp, _ = ndi.label(dense != label)
        closed = ~np.isin(comp, sorted(_on_a_face(comp) | {0}))
        if closed.any():
            holes[label] = closed
    state = np.zeros(nlab + 1, dtype=np.int64)
    dead = set()
    out = dense.copy()
    count = 0
    for label in range(1, nlab + 1):
        if label in dead:
            continue
        state[label] |= PROCESSED
        if label not in holes:
            continue
        state[label] |= FILLED
        count += int(holes[label].sum())
        for other in set(np.unique(dense[holes[label]]).tolist()) - {0}:
            dead.add(other)
            state[other] |= KILLED
        out[holes[label]] = label
    return _finish(cc, values, out, count, state)


def region_graph(cc):
    """The input of kh_host_resolve_holes built by numpy: (value u64 [R + 1], count u32 [R + 1], face u8 [R + 1], pairs u64, region
    ids per voxel).  Regions: 6-connected components of equal value, 0 included, numbered value by value."""
    cc = np.asarray(cc)
    if cc.dtype == np.bool_:
        cc = cc.view(np.uint8)
    region = np.zeros(cc.shape, dtype=np.int64)
    value = [0]
    for v in np.unique(cc).tolist():
        comp, k = ndi.label(cc == v)
        region[comp > 0] = comp[comp > 0] + len(value) - 1
        value += [v] * k
    nreg = len(value) - 1
    count = np.bincount(region.reshape(-1), minlength=nreg + 1).astype(np.uint32)
    face = np.zeros(nreg + 1, dtype=np.uint8)
    face[sorted(_on_a_face(region))] = 1
    keys = []
    for axis in range(cc.ndim):
        a = np.take(region, range(0, cc.shape[axis] - 1), axis=axis).reshape(-1)
        b = np.take(region, range(1, cc.shape[axis]), axis=axis).reshape(-1)
        differ = a != b
        lo, hi = np.minimum(a, b)[differ], np.maximum(a, b)[differ]
        keys.append((lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64))
    pairs = np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.uint64)
    return np.array(value, dtype=np.uint64), count, face, pairs.astype(np.uint64), region


def owner_volume(cc, owner, region):
    """what kh_region_apply makes of an owner table"""
    cc = np.asarray(cc)
    out = cc.view(np.uint8).copy() if cc.dtype == np.bool_ else cc.copy()
    own = np.asarray(owner)[region]
    out[own != 0] = own[own != 0].astype(out.dtype)
    return out.view(np.bool_) if cc.dtype == np.bool_ else out


def shell(shape, centre, radius, thickness, cube=False):
    """voxels at distance (radius - thickness, radius] from `centre`: Euclidean, or Chebyshev (a box's wall)"""
    grid = np.indices(shape).astype(np.float64)
    off = [grid[a] - centre[a] for a in range(len(shape))]
    d = np.max(np.abs(off), axis=0) if cube else np.sqrt(sum(o * o for o in off))
    return (d <= radius) & (d > radius - thickness)


def random_volume(seed, top=20, dtype=np.uint32):
    """a small label volume with what fill_all_holes has to deal with: shells of random radius and thickness (some nested, some
    around a blob of another label, some cut by the volume's faces), ids drawn with repetition (unconnected labels), noise holes
    and noise labels, now and then an axis of extent 1."""
    rng = np.random.default_rng(seed)
    shape = tuple(int(rng.integers(6, top + 1)) for _ in range(3))
    if rng.random() < 0.1:
        shape = tuple(1 if rng.random() < 0.4 else s for s in shape)
    cc = np.zeros(shape, dtype=dtype)
    if rng.random() < 0.5:                                  # a coarse Voronoi background instead of zeros
        pts = np.stack([rng.integers(0, s, 6) for s in shape], axis=1)
        grid = np.indices(shape)
        d = sum((grid[a][..., None] - pts[:, a]) ** 2 for a in range(3))
        cc[...] = (np.argmin(d, axis=-1) + 1).astype(dtype)
    ids = rng.permutation(np.arange(1, 13))
    for k in range(int(rng.integers(1, 5))):
        centre = [float(rng.integers(0, s)) for s in shape]
        radius = float(rng.integers(2, 8)) + (0.5 if rng.random() < 0.5 else 0.0)
        cube = rng.random() < 0.4
        cc[shell(shape, centre, radius, float(rng.integers(1, 3)), cube)] = ids[k % 4 if rng.random() < 0.3 else k + 4]
        if rng.random() < 0.6 and radius >= 3:              # something inside: a blob, or another shell
            inner = float(rng.integers(1, int(radius) - 1)) if radius >= 4 else 1.0
            what = shell(shape, centre, inner, 1.0 if rng.random() < 0.5 else inner + 1, cube)
            cc[what] = ids[int(rng.integers(0, 12))]
    noise = rng.random(shape)
    cc[noise < 0.01] = 0
    cc[noise > 0.99] = ids[int(rng.integers(0, 12))]
    return cc
