"""The abstract machine of the order-free invalidation sweep in plain Python: test infrastructure.

A restatement of the MODEL, not of csrc/sweep.h's storage: no chunks, no level window, no filter words, no candidate limit;
Cand(v) is a Python set.  It is the tested successor of experiments/cert_ball3.c.

  Model P     a multiset of nodes (key, source c, voxel v); remove ANY node of minimal key; if v is alive, kill it and add
              (|q - p_c|, c, q) for every alive neighbour q of v with |q - p_c| < r_c (strict).
  The machine evaluates P for all resolutions of "any" at once.  Per voxel: A (alive under every resolution), M (may be dead),
  D (dead under every resolution), Cand(v) = the sources that may own v.
    P event (L, c, v)   if v is not D: c joins Cand(v), and (v, c) hands a P event to every neighbour q that c covers, at level
                        max(L, key of q from c)
    D event (L, v)      v becomes D; every neighbour q that ALL of Cand(v) cover gets a D event at max(L, largest key of q over Cand(v))
  A level is one float32 key value.  Per level: all P events with their same-level cascades, then all D events with theirs, then
  the level is committed.  Sources are the path vertices that are alive; a voxel named twice counts once.  Certified iff no voxel
  is left in M; then D is the reference's dead set.

Keys have the reference's float32 operation order (oracle/kimi_oracle.c, ko_invalidate_ball_graph):
sqrtf(fl(fl((wx a)^2 + (wy b)^2) + (wz c)^2)); the neighbours of a voxel are the entries of ko_nhood26 (with its x-face quirk)
that the voxel's own graph word allows.
"""
import heapq
from types import SimpleNamespace

import numpy as np

# voxel_connectivity_graph bit of neighbourhood entry i (oracle/kimi_oracle.c: ko_graph_bit)
GRAPH_BIT = (1, 0, 3, 2, 5, 4, 9, 7, 8, 6, 17, 13, 16, 12, 15, 11, 14, 10, 25, 24, 23, 21, 22, 20, 19, 18)


def key_table(shape, anisotropy):
    """K[|a|, |b|, |c|] = the flood's float32 key of the offset (a, b, c), for every offset inside an array of `shape`"""
    f = np.float32
    w = [f(v) for v in anisotropy]
    sq = []
    for n, wv in zip(shape, w):
        a = wv * np.arange(int(n), dtype=f)
        sq.append(a * a)
    t = sq[0][:, None, None] + sq[1][None, :, None]
    t = t + sq[2][None, None, :]
    assert t.dtype == f
    return np.sqrt(t)


def ball_radii(dbf, locs, scale, const):
    """skeletontricks.pyx:393-395 / ko_ball_radii: fl(fl(scale * DBF[v]) + const) in float32"""
    f = np.float32
    t = (f(scale) * np.asarray(dbf, dtype=f).reshape(-1, order="F")[np.asarray(locs, dtype=np.int64)]).astype(f)
    return (t + f(const)).astype(f)


def _nhood26(x, y, z, sx, sy, sz, quirk=True):
    """linear offsets of the 26 entries exactly as ko_nhood26 (0 = absent): the corner entries 18..25 are gated on y and z only.
    quirk=False: a corner entry also needs its x step (what the reference does NOT do; for tests of the tests)"""
    sxy = sx * sy
    nb = [0] * 26
    nb[0] = -1 if x > 0 else 0
    nb[1] = 1 if x < sx - 1 else 0
    nb[2] = -sx if y > 0 else 0
    nb[3] = sx if y < sy - 1 else 0
    nb[4] = -sxy if z > 0 else 0
    nb[5] = sxy if z < sz - 1 else 0
    pair = ((0, 2), (0, 3), (1, 2), (1, 3), (2, 4), (2, 5), (3, 4), (3, 5), (0, 4), (0, 5), (1, 4), (1, 5))
    for i, (a, b) in enumerate(pair):
        nb[6 + i] = nb[a] + nb[b] if nb[a] and nb[b] else 0
    corner = ((0, 2, 4), (1, 2, 4), (0, 3, 4), (0, 2, 5), (1, 3, 4), (1, 2, 5), (0, 3, 5), (1, 3, 5))
    for i, (a, b, c) in enumerate(corner):
        nb[18 + i] = nb[a] + nb[b] + nb[c] if nb[b] and nb[c] and (quirk or nb[a]) else 0
    return nb


def sweep_model(mask, anisotropy, path, radii, graph=None, trace=False, x_face_quirk=True, ghosts=None):
    """The machine on one call.  mask: uint8 (x, y, z), non-zero = alive (not changed); path: (n, 3) voxels; radii: float32 per path
    vertex; graph: optional uint32 voxel connectivity graph of the mask's shape; x_face_quirk=False: see _nhood26.
    ghosts: the linear indices of the alive voxels that an earlier call left undecided (csrc/sweep.h:1025-1031, :670-673): a ghost
    takes candidates and hands P events on like any alive voxel; a D event on it makes it D and is counted apart (KG); it sends no
    D events itself -- its candidates' P events went out when they joined.  A path vertex that is a ghost is a source like an alive
    one (sweep.h:1078 tests the alive byte for non-zero): its own D event at level 0 kills it for certain and stops there, its P
    event goes on.  With ghosts the result carries D (every voxel that became D, ghosts among them), KG (the ghosts among D), M
    (every voxel left with candidates, old ghosts among them) and made (M without the old ghosts: the ghosts this call makes).
    Returns a namespace: D, M (sorted arrays of Fortran-order linear indices), certified, count (= |D|), max_cand (largest
    |Cand(v)| any voxel ever held), max_cand_at_death (largest |Cand(v)| of a voxel at its D event), n_many (voxels that ever held
    five candidates or more), levels (non-empty levels), peak_levels (most levels that had events pending at one time) and, with
    `trace`, ahead: the set of (level, key) pairs of the events that were sent to a later level."""
    m = np.asarray(mask)
    sx, sy, sz = (int(v) for v in m.shape)
    sxy = sx * sy
    alive0 = (m.reshape(-1, order="F") != 0)
    dead = (~alive0).tolist()                      # D, plus the voxels outside the object
    g = None if graph is None else np.asarray(graph, dtype=np.uint32).reshape(-1, order="F").tolist()
    K = key_table((sx, sy, sz), anisotropy).tolist()
    pts = np.asarray(path, dtype=np.int64).reshape(-1, 3)
    rad = [float(np.float32(r)) for r in np.asarray(radii, dtype=np.float32).reshape(-1)]
    assert len(rad) == len(pts)
    src = [(int(p[0]), int(p[1]), int(p[2])) for p in pts]
    ghost = frozenset(int(v) for v in np.asarray(ghosts if ghosts is not None else [], dtype=np.int64).reshape(-1))
    assert all(alive0[v] for v in ghost), "a ghost is an alive voxel of the mask"
    KG = []

    nbr_cache = {}

    def nbrs(v):
        """[(q, qx, qy, qz)] of the alive (at the start of the call) voxels v's own entries lead to"""
        got = nbr_cache.get(v)
        if got is None:
            z, r = divmod(v, sxy)
            y, x = divmod(r, sx)
            nb = _nhood26(x, y, z, sx, sy, sz, x_face_quirk)
            gw = g[v] if g is not None else 0xFFFFFFFF
            seen = set()
            got = []
            for i in range(26):
                if nb[i] == 0 or not (gw >> GRAPH_BIT[i]) & 1:
                    continue
                q = v + nb[i]
                if q in seen or not alive0[q]:
                    continue
                seen.add(q)
                qz, qr = divmod(q, sxy)
                qy, qx = divmod(qr, sx)
                got.append((q, qx, qy, qz))
            nbr_cache[v] = got
        return got

    pending = {}
    heap = []
    ahead = set() if trace else None

    def send(level, kind, item, frm):
        e = pending.get(level)
        if e is None:
            e = pending[level] = ([], [])
            heapq.heappush(heap, level)
        e[kind].append(item)
        if ahead is not None:
            ahead.add((frm, level))

    started = set()
    for c, (x, y, z) in enumerate(src):
        v = x + sx * y + sxy * z
        if dead[v] or v in started:
            continue
        started.add(v)
        send(0.0, 0, (v, c), 0.0)
        send(0.0, 1, v, 0.0)

    cand = {}
    D = []
    max_cand = max_death = n_many = levels = peak = 0
    while heap:
        peak = max(peak, len(heap))
        L = heapq.heappop(heap)
        work, dwork = pending.pop(L)
        levels += 1
        # all P events of the level, with their cascades
        i = 0
        while i < len(work):
            v, c = work[i]
            i += 1
            if dead[v]:
                continue
            cs = cand.get(v)
            if cs is None:
                cs = cand[v] = set()
            if c in cs:
                continue
            cs.add(c)
            if len(cs) > max_cand:
                max_cand = len(cs)
            if len(cs) == 5:
                n_many += 1
            cx, cy, cz = src[c]
            r = rad[c]
            for q, qx, qy, qz in nbrs(v):
                if dead[q]:
                    continue
                k = K[abs(qx - cx)][abs(qy - cy)][abs(qz - cz)]
                if k < r:
                    if k <= L:
                        work.append((q, c))
                    else:
                        send(k, 0, (q, c), L)
        # all D events of the level, with their cascades (every Cand is complete now)
        first = len(D)
        i = 0
        while i < len(dwork):
            v = dwork[i]
            i += 1
            if dead[v]:
                continue
            cs = cand.get(v)
            assert cs, "a D event on a voxel without a candidate"
            dead[v] = True
            D.append(v)
            if len(cs) > max_death:
                max_death = len(cs)
            if v in ghost:                         # it may have been dead all along: no D events from it
                KG.append(v)
                continue
            owners = [(src[c], rad[c]) for c in cs]
            for q, qx, qy, qz in nbrs(v):
                if dead[q]:
                    continue
                t = 0.0
                for (cx, cy, cz), r in owners:
                    k = K[abs(qx - cx)][abs(qy - cy)][abs(qz - cz)]
                    if not k < r:
                        t = -1.0
                        break
                    if k > t:
                        t = k
                if t < 0.0:
                    continue
                if t <= L:
                    dwork.append(q)
                else:
                    send(t, 1, q, L)
        # commit
        for v in D[first:]:
            del cand[v]
    M = sorted(v for v, cs in cand.items() if cs)
    return SimpleNamespace(D=np.array(sorted(D), dtype=np.int64), M=np.array(M, dtype=np.int64), certified=not M, count=len(D),
                           max_cand=max_cand, max_cand_at_death=max_death, n_many=n_many, levels=levels, peak_levels=peak,
                           ahead=ahead, KG=np.array(sorted(KG), dtype=np.int64),
                           made=np.array([v for v in M if v not in ghost], dtype=np.int64))


def classify(res):
    """U: certified, every voxel dies with one candidate; K: certified, some voxel dies with 2-4; S: certified, some voxel holds
    5-8; C: some voxel gets a ninth candidate; M: voxels left in M (and no ninth candidate)"""
    if res.max_cand >= 9:
        return "C"
    if not res.certified:
        return "M"
    if res.max_cand_at_death <= 1:
        return "U"
    return "K" if res.max_cand_at_death <= 4 else "S"
