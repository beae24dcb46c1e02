"""The avocado pass (fix_avocados=True, kimimaro/intake.py:600-704) on the component volume resident in HBM."""
from __future__ import annotations

import numpy as np

from .volume import last_run_starts


def _avocado_fruit_from_lines(xl, yl, zl, cx, cy, cz, background=0):
    """kimimaro.skeletontricks.find_avocado_fruit (skeletontricks.pyx:905-992) on the three axis-parallel lines of the label volume
    through (cx, cy, cz) (host copies): six rays from the voxel, each ends at the background or at the first other label, which it
    reports; the rays towards smaller coordinates stop BEFORE index 0 (`range(c, 0, -1)`).  Fewer than three reports: (label, label).
    The most frequent report -- the smallest label among equally frequent ones (np.unique order) -- is the fruit if at most one
    report disagrees with it (none when there are exactly three reports)."""
    label = int(xl[cx])
    rays = (xl[cx:], xl[cx:0:-1], yl[cy:], yl[cy:0:-1], zl[cz:], zl[cz:0:-1])
    changes = []
    for ray in rays:
        stop = np.flatnonzero((ray == background) | (ray != label))
        if stop.size and int(ray[stop[0]]) != background:
            changes.append(int(ray[stop[0]]))
    if len(changes) < 3:
        return label, label
    uniq, cts = np.unique(changes, return_counts=True)
    k = int(np.argmax(cts))
    if len(changes) - int(cts[k]) > (1 if len(changes) > 3 else 0):
        return label, label
    return label, int(uniq[k])


def engage_avocado_protection_device(eng, d_cc, shape, nlabels, remapping, anisotropy, black_border, soma_detection_threshold):
    """kimimaro/intake.py:600-704 (fix_avocados=True) on the component volume resident in HBM: a nucleus that carries a label of its
    own inside its cell ("pit" in "fruit") is merged into the cell, holes filled, up to 20 passes for nested ones; then the
    components are renumbered (fastremap.renumber: by first appearance) and mapped back to the original labels
    (skeletontricks.get_mapping, skeletontricks.pyx:490-525).  Device work: the transforms (kh_edt), the bounding boxes
    (kh_label_stats), the 2-D fills of the six faces of a crop and its 3-D fill (kh_fill_voids_nd); selections, arg-max and the
    relabelling are device-side tensor plumbing; the host reads three lines of labels per candidate (find_avocado_fruit's rays)
    and keeps the reference's sets -- INCLUDING their iteration order: the candidates of a pass are a Python set built from the
    sorted unique labels, and the reference edits the volume in that set's order.
    Returns (component volume u32 on the device, number of components, {component: original label}, its EDT)."""
    t = eng.torch
    sx, sy, sz = (int(v) for v in shape)
    nvox = sx * sy * sz
    d_cc = d_cc.clone()                      # (the caller's volume may be shared)
    orig = d_cc.clone()
    v = d_cc.view(sz, sy, sx)                # torch C order (z, y, x) == Fortran order (x, y, z)
    d_dbf = eng.edt(d_cc, 4, shape, anisotropy, black_border)
    thr = float(np.float32(soma_detection_threshold / 2.5))     # numpy compares the f32 field with the scalar in float32
    unchanged = set()
    for _ in range(20):
        vals = t.unique(d_cc[d_dbf > thr]).cpu().numpy().view(np.uint32)       # sorted, like fastremap.unique
        candidates = set([0] + [int(x) for x in vals]) if bool((d_dbf <= thr).any()) else set(int(x) for x in vals)
        candidates -= unchanged
        candidates.discard(0)
        order = [label for label in candidates if label != 0]
        changed, unchanged_now = set(), set()          # (the sets of ONE pass, intake.py:650-651)
        if order:
            stats = eng.label_stats(d_cc, 4, d_dbf, shape, nlabels)
            for label in order:
                lo, hi = stats.bbox(label)
                sub = eng.box(d_cc, shape, lo, hi)
                binimg = (sub == label)
                # paint_walls (:655-666): a 2-D fill on each of the six faces, in the reference's order
                for face in ((-1, 0), (-1, -1), (1, 0), (1, -1), (2, 0), (2, -1)):      # (torch axis, index): z, z, y, y, x, x
                    ax = 0 if face[0] == -1 else face[0]
                    plane = binimg.select(ax, face[1])
                    p2 = plane.to(t.uint8).contiguous()
                    filled, nfill = eng.fill_voids(p2.view(-1), (p2.shape[1], p2.shape[0], 1), ndim=2)
                    if nfill:
                        plane.copy_(filled.view(p2.shape).bool())
                prod = binimg * eng.box(d_dbf, shape, lo, hi)
                k = int(t.argmax(prod.reshape(-1)).item())            # first maximum in the raster (x fastest), like argmax(arr.T)
                nx, ny = hi[0] - lo[0], hi[1] - lo[1]
                cx, cy, cz = lo[0] + k % nx, lo[1] + (k // nx) % ny, lo[2] + k // (nx * ny)
                lines = [a.cpu().numpy().view(np.uint32) for a in (v[cz, cy, :], v[cz, :, cx].contiguous(), v[:, cy, cx].contiguous())]
                pit, fruit = _avocado_fruit_from_lines(lines[0], lines[1], lines[2], cx, cy, cz)
                if pit == fruit and pit not in changed:
                    unchanged_now.add(pit)
                else:
                    unchanged_now.discard(pit)
                    unchanged_now.discard(fruit)
                    changed.add(pit)
                    changed.add(fruit)
                    binimg |= (sub == fruit)
                cshape = (hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])
                filled, _ = eng.fill_voids(binimg.to(t.uint8).contiguous().view(-1), cshape)
                fb = filled.view(cshape[2], cshape[1], cshape[0]).bool()
                sub[fb] = fruit                               # cc_labels[slc] *= ~binimg; cc_labels[slc] += fruit * binimg
        unchanged |= unchanged_now
        if len(changed) == 0:
            break
        d_dbf = eng.edt(d_cc, 4, shape, anisotropy, black_border)
    # fastremap.renumber: 1..N by first appearance in memory; get_mapping: the LAST run start of a component in the raster names it
    flat = d_cc.to(t.int64) & 0xFFFFFFFF
    idx = t.arange(nvox, device=eng.device, dtype=t.int64)
    top = int(flat.max().item()) + 1
    first = t.full((top,), nvox, dtype=t.int64, device=eng.device).scatter_reduce(0, flat, idx, reduce="amin")
    present = t.nonzero(first < nvox).reshape(-1)
    present = present[present != 0]
    by_first = present[t.argsort(first[present], stable=True)]
    lut = t.zeros(top, dtype=t.int64, device=eng.device)
    lut[by_first] = t.arange(1, by_first.numel() + 1, device=eng.device, dtype=t.int64)
    new = lut[flat]
    n_new = int(by_first.numel())
    last = last_run_starts(t, new, n_new)
    last_h = last.cpu().numpy()
    src = (orig.to(t.int64) & 0xFFFFFFFF)[last.clamp(min=0)].cpu().numpy()
    adjusted = {}
    for new_cc in range(0, n_new + 1):
        if last_h[new_cc] >= 0 and int(src[new_cc]) in remapping:
            adjusted[new_cc] = remapping[int(src[new_cc])]
    return new.to(t.int32), n_new, adjusted, d_dbf       # (renumbering does not move a voxel: the last transform stands)
