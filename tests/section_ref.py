"""CPU statement of the plane sections: numpy only, independent of the product.

Membership is the definition's expression, operation by operation.  The flood is a plain stack flood.  A voxel's area comes from
clipping a large in-plane square by the six half-spaces of the voxel's box (Sutherland-Hodgman) and the shoelace formula -- not the
closed form the kernel evaluates.  paths / branches / terminals and the driver loop are restated sequentially, one section at a
time."""
import numpy as np


# ---- one section ------------------------------------------------------------------------------------------------------------

def offsets(normal, anisotropy, delta):
    """d of the definition for integer offsets delta (..., 3) from the seed: ((nx ax) dx + (ny ay) dy) + (nz az) dz"""
    n = np.asarray(normal, dtype=np.float64)
    a = np.asarray(anisotropy, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    return ((n[0] * a[0]) * delta[..., 0] + (n[1] * a[1]) * delta[..., 1]) + (n[2] * a[2]) * delta[..., 2]


def half_width(normal, anisotropy):
    n = np.asarray(normal, dtype=np.float64)
    a = np.asarray(anisotropy, dtype=np.float64)
    return 0.5 * ((abs(n[0]) * a[0] + abs(n[1]) * a[1]) + abs(n[2]) * a[2])


def _clip(poly, count, axis, bound, sign):
    """Sutherland-Hodgman against the half-space sign * x[axis] <= bound, for a batch: poly (m, K, 3), count (m,) valid vertices
    in front.  Returns the same for the clipped polygons."""
    m, K, _ = poly.shape
    idx = np.arange(K)[None, :]
    valid = idx < count[:, None]
    nxt_i = np.where(idx + 1 < count[:, None], idx + 1, 0)
    nxt = np.take_along_axis(poly, nxt_i[:, :, None], axis=1)
    f0 = sign * poly[:, :, axis] - bound
    f1 = sign * nxt[:, :, axis] - bound
    in0, in1 = f0 <= 0, f1 <= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        t = f0 / (f0 - f1)
        cross = poly + t[:, :, None] * (nxt - poly)
    out = np.zeros((m, 2 * K, 3))
    keep = np.zeros((m, 2 * K), dtype=bool)
    out[:, 0::2] = poly
    keep[:, 0::2] = valid & in0
    out[:, 1::2] = cross
    keep[:, 1::2] = valid & (in0 != in1)
    order = np.argsort(~keep, axis=1, kind="stable")
    out = np.take_along_axis(out, order[:, :, None], axis=1)
    count = keep.sum(axis=1)
    width = max(int(count.max()) if m else 0, 1)
    return out[:, :width], count


def voxel_areas(normal, anisotropy, d):
    """area of plane /\\ box for boxes of edges `anisotropy` whose centres lie at offset d (array) from the plane, in the units of
    offsets(): a square of half-width R in the plane, clipped by the box's six faces, then the shoelace formula"""
    n = np.asarray(normal, dtype=np.float64)
    a = np.asarray(anisotropy, dtype=np.float64)
    d = np.atleast_1d(np.asarray(d, dtype=np.float64))
    length = np.sqrt(n @ n)
    nu = n / length
    k = int(np.argmin(abs(nu)))
    e1 = np.cross(nu, np.eye(3)[k])
    e1 /= np.sqrt(e1 @ e1)
    e2 = np.cross(nu, e1)
    R = 4.0 * float(np.sqrt(a @ a))
    origin = (-d / length)[:, None] * nu[None, :]                   # n . x = -d, relative to the box's centre
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64) * R
    poly = origin[:, None, :] + corners[None, :, 0, None] * e1 + corners[None, :, 1, None] * e2
    count = np.full(d.size, 4)
    for axis in range(3):
        for sign in (1.0, -1.0):
            poly, count = _clip(poly, count, axis, 0.5 * a[axis], sign)
    # vertices behind the count repeat the first one: they add nothing to the shoelace sum
    idx = np.arange(poly.shape[1])[None, :]
    poly = np.where((idx < count[:, None])[:, :, None], poly, poly[:, :1])
    u = (poly - origin[:, None, :]) @ e1
    v = (poly - origin[:, None, :]) @ e2
    twice = np.sum(u * np.roll(v, -1, axis=1) - np.roll(u, -1, axis=1) * v, axis=1)
    return np.where(count >= 3, 0.5 * abs(twice), 0.0)


def voxel_grid(shape):
    return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)


def section(labels, seed, normal, anisotropy, label, grid=None):
    """-> (voxels (k, 3) of the section, area float64, contact).  labels: any array indexed [x, y, z]; grid: the (sx, sy, sz, 3)
    array of voxel coordinates when the caller has it already."""
    labels = np.asarray(labels)
    shape = labels.shape
    n = np.asarray(normal, dtype=np.float64)
    seed = tuple(int(v) for v in seed)
    none = np.zeros((0, 3), dtype=np.int64), 0.0, 0
    if not np.all(np.isfinite(n)) or not np.any(n != 0):
        return none
    if any(c < 0 or c >= s for c, s in zip(seed, shape)) or labels[seed] != label:
        return none
    h = half_width(n, anisotropy)
    if grid is None:
        grid = voxel_grid(shape)
    d = offsets(n, anisotropy, grid - np.array(seed))
    cut = (abs(d) < h) & (labels == label)
    if not cut[seed]:
        return none
    members = set(map(tuple, np.argwhere(cut).tolist()))
    nbrs = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
    stack, found = [seed], {seed}
    while stack:
        x, y, z = stack.pop()
        for i, j, k in nbrs:
            q = (x + i, y + j, z + k)
            if q in members and q not in found:
                found.add(q)
                stack.append(q)
    vox = np.array(sorted(found), dtype=np.int64)
    area = float(np.sum(voxel_areas(n, anisotropy, d[vox[:, 0], vox[:, 1], vox[:, 2]])))
    contact = 0
    for axis in range(3):
        contact |= (1 << (2 * axis)) * bool(np.any(vox[:, axis] == 0))
        contact |= (2 << (2 * axis)) * bool(np.any(vox[:, axis] == shape[axis] - 1))
    return vox, area, contact


# ---- skeleton traversal -------------------------------------------------------------------------------------------------------

def neighbours(nverts, edges):
    nb = [set() for _ in range(nverts)]
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        if a != b:
            nb[a].add(b)
            nb[b].add(a)
    return [sorted(s) for s in nb]


def branches(nverts, edges):
    return [v for v, nb in enumerate(neighbours(nverts, edges)) if len(nb) >= 3]


def terminals(nverts, edges):
    return [v for v, nb in enumerate(neighbours(nverts, edges)) if len(nb) == 1]


def paths(nverts, edges):
    """index lists, root to leaf (the definition of DESIGN.md 3.12)"""
    nb = neighbours(nverts, edges)
    assigned = [False] * nverts
    out = []
    for start in range(nverts):
        if assigned[start]:
            continue
        hops = {start: 0}
        todo = [start]
        for v in todo:                      # (a list that grows while it is read: breadth first)
            for q in nb[v]:
                if q not in hops:
                    hops[q] = hops[v] + 1
                    todo.append(q)
        for v in hops:
            assigned[v] = True
        if len(hops) == 1:
            continue
        far = max(hops.values())
        root = min(v for v in hops if hops[v] == far)
        visited = {root}
        trail = [root]
        walkers = [iter(nb[root])]
        leaf = [True]
        while trail:
            step = next((q for q in walkers[-1] if q not in visited), None)
            if step is None:
                if leaf[-1]:
                    out.append(list(trail))
                trail.pop()
                walkers.pop()
                leaf.pop()
                continue
            leaf[-1] = False
            visited.add(step)
            trail.append(step)
            walkers.append(iter(nb[step]))
            leaf.append(True)
    return out


# ---- the driver, sequentially ---------------------------------------------------------------------------------------------------

def moving_average(a, n):
    if n <= 0:
        raise ValueError("window")
    if n == 1 or len(a) == 0:
        return a
    pad = [[n, n]] + [[0, 0]] * (a.ndim - 1)
    total = np.cumsum(np.pad(a, pad, mode="symmetric"), dtype=float, axis=0)
    total = (total[n:] - total[:-n])[:-n]
    total /= float(n)
    return total


class SectionCache:
    """sections of one (volume, anisotropy) by (seed, label, normal): the driver cases share most of their items"""

    def __init__(self, labels, anisotropy):
        self.labels, self.anisotropy, self.memo = np.asarray(labels), np.asarray(anisotropy, dtype=np.float64), {}
        self.grid = voxel_grid(self.labels.shape)

    def __call__(self, seed, normal, label):
        key = (tuple(int(v) for v in seed), int(label), np.asarray(normal, dtype=np.float64).tobytes())
        if key not in self.memo:
            vox, area, contact = section(self.labels, seed, normal, self.anisotropy, label, self.grid)
            self.memo[key] = (np.float32(area), contact, len(vox))
        return self.memo[key]


def single_skeleton(sections, shape, vertices, edges, space, label, anisotropy, smoothing_window=1, step=1, offset=(0, 0, 0),
                    areas=None, contacts=None, repair_contacts=False):
    """the loop of kimimaro/utility.py:231-349 for one skeleton, one section after the other.  sections: SectionCache;
    areas / contacts: the existing arrays for multipass / repair_contacts (changed in place), None for a first pass.
    Returns (areas f32, contacts u8)."""
    an = np.asarray(anisotropy, dtype=np.float32)
    vertices = np.asarray(vertices).reshape(-1, 3)
    if space == "physical":
        vox = (vertices / an).round().astype(np.int64)
    else:
        vox = np.round(vertices).astype(np.int64)
    vox = vox - np.asarray(offset, dtype=np.int64)
    nverts = len(vox)
    mapping = {tuple(v): i for i, v in enumerate(vox.tolist())}
    if areas is None:
        areas = np.zeros(nverts, dtype=np.float32)
        contacts = np.zeros(nverts, dtype=np.uint8)
    visited = np.zeros(nverts, dtype=bool)
    branch_pts = set(branches(nverts, edges))
    branch_vals = {}
    for path in paths(nverts, edges):
        pts = vox[path]
        normals = (pts[1:] - pts[:-1]).astype(np.float32)
        normals = np.concatenate([normals, [normals[-1]]])
        normals = moving_average(normals, smoothing_window)
        normals = moving_average(normals[::-1], smoothing_window)[::-1]
        with np.errstate(invalid="ignore", divide="ignore"):
            normals = normals / np.linalg.norm(normals, axis=1, keepdims=True)
        end = len(pts) - 1
        ct = 0
        for i, vert in enumerate(pts.tolist()):
            ct += 1
            if ct < step and not (i == 0 or i == end):
                continue
            elif ct == step:
                ct = 0
            if any(c < 0 or c >= s for c, s in zip(vert, shape)):
                continue
            idx = mapping[tuple(vert)]
            if areas[idx] == 0 or idx in branch_pts or (repair_contacts and contacts[idx] > 0 and not visited[idx]):
                visited[idx] = True
                area, contact, _ = sections(vert, normals[i].astype(np.float64), label)
                areas[idx] = area
                if repair_contacts:
                    contacts[idx] = contact
                else:
                    contacts[idx] |= contact
                if idx in branch_pts:
                    branch_vals.setdefault(idx, []).append(areas[idx])
    for idx, vals in branch_vals.items():
        total = np.float32(0)
        for v in vals:
            total = np.float32(total + v)                  # the float mean: float32, summed in the loop's order
        areas[idx] = np.float32(total / np.float32(len(vals)))
    return areas, contacts
