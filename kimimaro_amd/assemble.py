"""Skeleton assembly on the host: the path arrays Engine.run_labels hands over become one Skeleton per original label
(kimimaro/trace.py:182-192 + intake.py:506-517, 587-593)."""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from . import _abi
from .skeleton import Skeleton
from .volume import coords_of, ranges

P = _abi.np_ptr


def paths_of(res, slot, shape):
    """list of (n,3) integer voxel paths of task `slot`."""
    v0, l0, l1 = res["voff"][slot], res["loff"][slot], res["loff"][slot + 1]
    out = []
    pos = v0
    for n in res["lens"][l0:l1]:
        out.append(coords_of(res["verts"][pos:pos + n], shape))
        pos += n
    return out


def consolidate_paths(locs, lens, radii, shape):
    """Skeleton.from_path per path + simple_merge + consolidate (kimimaro/trace.py:182-184) for one label, on
    linear voxel indices: returns (vertices (n,3) f32 sorted lexicographically by (x,y,z) like
    np.unique(axis=0), edges (m,2) u32 sorted/unique without self loops, radii of the first occurrences).
    Same result as kimimaro_amd.skeleton.Skeleton.consolidate (vertices no edge refers to dropped), ~10x cheaper
    (1-D unique on a key)."""
    sx, sy, sz = shape
    x, y, z = locs % sx, (locs // sx) % sy, locs // (sx * sy)
    key = (x * sy + y) * sz + z                      # row-lexicographic order of (x, y, z)
    ukey, first, inv = np.unique(key, return_index=True, return_inverse=True)
    n = locs.size
    starts = np.cumsum(lens)[:-1]
    eidx = np.arange(n - 1)
    if starts.size:
        keep = np.ones(n - 1, dtype=bool)
        keep[starts - 1] = False                     # no edge across two paths
        eidx = eidx[keep]
    a, b = inv[eidx], inv[eidx + 1]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    ok = lo != hi
    ekey = np.unique(lo[ok] * np.int64(ukey.size) + hi[ok])
    edges = np.stack([ekey // ukey.size, ekey % ukey.size], axis=1)
    used = np.zeros(ukey.size, dtype=bool)
    used[edges.ravel()] = True
    if not used.all():      # a one-vertex path off every other path: no edge refers to it (consolidate drops it)
        first, edges = first[used], (np.cumsum(used) - 1)[edges]
    verts = np.stack([x[first], y[first], z[first]], axis=1).astype(np.float32)
    return verts, edges.astype(np.uint32), radii[first]


def consolidate_paths_flat(res, shape):
    """consolidate_paths for EVERY label of a result group in ONE native call outside the interpreter
    (kh_host_consolidate_paths, include/kimi_hip.h: with twenty volumes in flight the lanes reach this point together and what
    holds the interpreter lock is paid twenty times in a row).  Returns None for a group without vertices, else the slots' arrays
    back to back: verts (N,3) f32, radii (N) f32, edges (M,2) u32 with indices local to the slot, vstart / estart [nslots+1].
    Same arrays as consolidate_paths_flat_numpy (tests/test_host.py compares them)."""
    sx, sy, sz = shape
    voff = np.ascontiguousarray(res["voff"], dtype=np.int64)
    loff = np.ascontiguousarray(res["loff"], dtype=np.int64)
    nslots = voff.size - 1
    locs = np.ascontiguousarray(res["verts"], dtype=np.uint32)
    n = int(locs.size)
    if n == 0:
        return None
    lens = np.ascontiguousarray(res["lens"], dtype=np.uint32)
    radii = np.ascontiguousarray(res["radii"], dtype=np.float32)
    oV, oR, oE = np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty((n, 2), np.uint32)
    vstart, estart = np.empty(nslots + 1, np.int64), np.empty(nslots + 1, np.int64)
    got = _abi.lib().kh_host_consolidate_paths(nslots, P(voff), P(loff), P(locs), P(lens), P(radii), int(sx), int(sy), int(sz),
                                               P(oV), P(oR), P(oE), P(vstart), P(estart))
    if got < 0:
        raise MemoryError("kh_host_consolidate_paths failed")
    return {"verts": oV[:got], "radii": oR[:got], "edges": oE[:int(estart[-1])], "vstart": vstart, "estart": estart, "voff": voff}


def consolidate_paths_flat_numpy(res, shape):
    """the numpy form of consolidate_paths_flat, kept as the statement the native call is tested against: consolidate_paths for
    EVERY label of a result group in one go (one sort over all path vertices instead of three np.unique calls per label: the
    per-label numpy overhead, 170 us x 3.4 k labels, was most of the assembly time of a 512^3 volume).  Returns None for a group
    without vertices, else the slots' arrays back to back: verts (N,3) f32, radii (N) f32, edges (M,2) u32 with indices local to
    the slot, vstart / estart [nslots+1]."""
    sx, sy, sz = shape
    voff = np.asarray(res["voff"], dtype=np.int64)
    nslots = voff.size - 1
    locs = res["verts"].astype(np.int64)
    n = locs.size
    if n == 0:
        return None
    V = np.int64(sx) * sy * sz
    slot_of = np.repeat(np.arange(nslots, dtype=np.int64), np.diff(voff))
    x, y, z = locs % sx, (locs // sx) % sy, locs // (sx * sy)
    key = slot_of * V + (x * sy + y) * sz + z                 # slot, then row-lexicographic order of (x, y, z)
    ukey, first, inv = np.unique(key, return_index=True, return_inverse=True)
    nu = ukey.size
    uslot = ukey // V
    ustart = np.searchsorted(uslot, np.arange(nslots + 1, dtype=np.int64))     # unique vertices of slot s: [ustart[s], ustart[s+1])
    # consecutive pairs inside a path are edges: drop the pair that straddles two paths (path ends, incl. label ends)
    lens = res["lens"].astype(np.int64)
    path_end = np.cumsum(lens) - 1
    keep = np.ones(max(n - 1, 0), dtype=bool)
    keep[path_end[path_end < n - 1]] = False
    eidx = np.flatnonzero(keep)
    a, b = inv[eidx], inv[eidx + 1]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    ok = lo != hi
    ekey = np.unique(lo[ok] * np.int64(nu) + hi[ok])           # sorted by (lo, hi): grouped by slot, rows sorted like np.unique(axis=0)
    elo, ehi = ekey // nu, ekey % nu
    used = np.zeros(nu, dtype=bool)
    used[elo] = True
    used[ehi] = True
    # vertices no edge refers to are dropped (Skeleton.consolidate); local index = rank among the slot's used vertices
    cum = np.concatenate([[0], np.cumsum(used)])
    rank = cum[1:] - 1
    base = cum[ustart[:-1]] if nu else np.zeros(nslots, np.int64)
    fu = first[used]
    verts_all = np.stack([x[fu], y[fu], z[fu]], axis=1).astype(np.float32)
    radii_all = res["radii"][fu]
    vstart = cum[ustart]                                       # used vertices of slot s: [vstart[s], vstart[s+1])
    eslot = uslot[elo]
    estart = np.searchsorted(eslot, np.arange(nslots + 1, dtype=np.int64))
    edges_all = np.stack([rank[elo] - base[eslot], rank[ehi] - base[eslot]], axis=1).astype(np.uint32)
    return {"verts": verts_all, "radii": radii_all, "edges": edges_all, "vstart": vstart, "estart": estart, "voff": voff}


def consolidate_paths_batch(res, shape):
    """consolidate_paths_flat slot by slot: yields (slot, vertices (n,3) f32, edges (m,2) u32, radii) for the slots that have
    vertices, the same arrays the per-label function returns."""
    f = consolidate_paths_flat(res, shape)
    if f is None:
        return
    vstart, estart, voff = f["vstart"], f["estart"], f["voff"]
    for s in range(voff.size - 1):
        if voff[s + 1] == voff[s]:
            continue
        yield s, f["verts"][vstart[s]:vstart[s + 1]], f["edges"][estart[s]:estart[s + 1]], f["radii"][vstart[s]:vstart[s + 1]]


class Assembler:
    """Skeleton assembly: kimimaro/trace.py:182-192 + intake.py:506-517, 587-593.  Results arrive in groups of
    labels (Engine.run_labels hands them over as the groups finish on the GPU): `add` consolidates the paths of a group's
    components, `finish` merges the components of every original label.  Nothing here loops over components in Python: with
    twenty volumes in flight the lanes reach this point together and every millisecond of interpreter time is paid twenty times
    in a row (0.8 s of a 7.8 s round before this form)."""

    def __init__(self, shape, anisotropy, remapping):
        self.shape = shape
        self.remapping = remapping
        self.an = np.asarray(anisotropy, dtype=np.float32)
        an = self.an
        self.transform = np.array([[an[0], 0, 0, 0], [0, an[1], 0, 0], [0, 0, an[2], 0]], dtype=np.float32)
        self.skeletons = defaultdict(list)       # original label -> [(component id, verts, edges, radii)]: per-component hand-over (tests)
        self.groups = []                         # (component ids of the group's slots, consolidate_paths_flat of the group)

    def add(self, res):
        flat = consolidate_paths_flat(res, self.shape)
        if flat is not None:
            self.groups.append((np.asarray(res["tasks"]["segid"], dtype=np.int64), flat))

    def _parts(self):
        """the components that have edges (Skeleton.empty() ones are dropped, intake.py:506), in arrival order, as arrays: component
        id, original label (as a code into `labels`), and where their vertices / edges lie in the concatenated arrays"""
        seg, v0, nv, e0, ne, Vs, Rs, Es = [], [], [], [], [], [], [], []
        vbase = ebase = 0
        for segids, f in self.groups:
            cnt_e = np.diff(f["estart"])
            keep = np.flatnonzero(cnt_e > 0)
            seg.append(segids[keep])
            v0.append(f["vstart"][keep] + vbase)
            nv.append(np.diff(f["vstart"])[keep])
            e0.append(f["estart"][keep] + ebase)
            ne.append(cnt_e[keep])
            Vs.append(f["verts"]); Rs.append(f["radii"]); Es.append(f["edges"])
            vbase += f["verts"].shape[0]
            ebase += f["edges"].shape[0]
        for orig, parts in self.skeletons.items():            # (hand-over per component: the same arrays, one part at a time)
            for comp, verts, edges, radii in parts:
                if edges.shape[0] == 0:
                    continue
                seg.append(np.array([-1 - len(self._extra)], dtype=np.int64))
                self._extra.append((orig, comp))
                v0.append(np.array([vbase])); nv.append(np.array([verts.shape[0]]))
                e0.append(np.array([ebase])); ne.append(np.array([edges.shape[0]]))
                Vs.append(np.asarray(verts, dtype=np.float32)); Rs.append(np.asarray(radii, dtype=np.float32))
                Es.append(np.asarray(edges, dtype=np.uint32))
                vbase += verts.shape[0]
                ebase += edges.shape[0]
        if not seg:
            return None
        cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False)
        return (cat(seg, np.int64), cat(v0, np.int64), cat(nv, np.int64), cat(e0, np.int64), cat(ne, np.int64),
                np.concatenate(Vs), np.concatenate(Rs), np.concatenate(Es))

    def finish(self):
        """one Skeleton per original label, in the order in which the labels' first components arrived.  The components of a
        label are disjoint voxel sets, so Skeleton.simple_merge(...).consolidate() (intake.py:587-593) is a concatenation
        re-sorted lexicographically by vertex: done on integer keys for all labels in ONE native call outside the interpreter
        (kh_host_merge_components; same result as np.unique(vertices, axis=0) + edge remap per label)."""
        sx, sy, sz = self.shape
        self._extra = []
        got = self._parts()
        if got is None:
            return {}
        seg, v0, nv, e0, ne, Vall, Rall, Eall = got
        # original label of every part, as a code; the dict of component ids is read once, not once per component
        keys = np.fromiter(self.remapping.keys(), dtype=np.int64, count=len(self.remapping)) if len(self.remapping) else np.zeros(0, np.int64)
        vals = list(self.remapping.values())
        comp_of = seg.copy()
        label_objs = []
        code_of_obj = {}
        if keys.size:
            ks = np.argsort(keys, kind="stable")
            sorted_keys = keys[ks]
            pos = np.searchsorted(sorted_keys, np.maximum(seg, 0))
            found = pos < keys.size
            found[found] = sorted_keys[pos[found]] == seg[found]
            pos[~found] = 0
            idx_in_vals = ks[pos]
        else:
            found = np.zeros(seg.size, dtype=bool)
            idx_in_vals = np.zeros(seg.size, dtype=np.int64)
        absent = np.flatnonzero((seg >= 0) & ~found)
        if absent.size:                                         # the reference's remapping[segid] (intake.py:510): no neighbour's label
            raise KeyError(int(seg[absent[0]]))
        # code per distinct original label VALUE (several component ids map to one label)
        val_code = np.empty(len(vals), dtype=np.int64)
        for i, v in enumerate(vals):
            c = code_of_obj.get(v)
            if c is None:
                c = code_of_obj[v] = len(label_objs)
                label_objs.append(v)
            val_code[i] = c
        code = val_code[idx_in_vals] if len(vals) else np.zeros(seg.size, dtype=np.int64)
        for j in np.flatnonzero(seg < 0):                       # per-component hand-over: (label, component id) given directly
            orig, comp = self._extra[-1 - int(seg[j])]
            c = code_of_obj.get(orig)
            if c is None:
                c = code_of_obj[orig] = len(label_objs)
                label_objs.append(orig)
            code[j] = c
            comp_of[j] = comp
        ucode, first_idx = np.unique(code, return_index=True)
        label_order = ucode[np.argsort(first_idx, kind="stable")]                # labels by first arrival
        rank_of_code = np.empty(len(label_objs), dtype=np.int64)
        rank_of_code[label_order] = np.arange(label_order.size)
        order = np.lexsort((comp_of, rank_of_code[code]))                        # label by label, components by id (intake.py:444)
        nvs, nes = nv[order], ne[order]
        V = np.ascontiguousarray(Vall[ranges(v0[order], nvs)], dtype=np.float32)
        R = np.ascontiguousarray(Rall[ranges(v0[order], nvs)], dtype=np.float32)
        E = np.ascontiguousarray(Eall[ranges(e0[order], nes)], dtype=np.uint32)
        vstart = np.concatenate([[0], np.cumsum(nvs)]).astype(np.int64)
        estart = np.concatenate([[0], np.cumsum(nes)]).astype(np.int64)
        pol = np.concatenate([[0], np.cumsum(np.bincount(rank_of_code[code], minlength=label_order.size))]).astype(np.int64)
        oV, oR, oE = np.empty_like(V), np.empty_like(R), np.empty_like(E)
        if _abi.lib().kh_host_merge_components(int(label_order.size), P(pol), P(vstart), P(estart), P(V), P(R), P(E), int(sy), int(sz),
                                               np.float32(self.an[0]), np.float32(self.an[1]), np.float32(self.an[2]),
                                               P(oV), P(oR), P(oE)) != 0:
            raise MemoryError("kh_host_merge_components failed")
        merged = {}
        va, ea = vstart[pol].tolist(), estart[pol].tolist()       # first vertex / edge of every label
        wrap, tf = Skeleton.wrap, self.transform
        for li, c in enumerate(label_order.tolist()):
            # copies: the public arrays own their memory (a kept Skeleton does not pin the volume's buffers)
            a, b, e0_, e1_ = va[li], va[li + 1], ea[li], ea[li + 1]
            merged[label_objs[c]] = wrap(oV[a:b].copy(), oE[e0_:e1_].copy(), oR[a:b].copy(), label_objs[c], tf.copy(), "physical")
        return merged


def assemble(res, shape, anisotropy, remapping):
    asm = Assembler(shape, anisotropy, remapping)
    asm.add(res)
    return asm.finish()
