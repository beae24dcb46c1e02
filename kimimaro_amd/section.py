"""Device plumbing of the plane sections (csrc/section.hip): a batch of (seed voxel, label, normal) items against the
label volume resident in HBM, one launch.  kimimaro_amd.utility.cross_sectional_area and kimimaro_amd.ops.cross_sectional_area are
the callers.  The library allocates nothing: the scratch (visited bitmaps and queue spill of the concurrent waves) is sized here."""
from __future__ import annotations

import time

import numpy as np

from . import _abi
from .holes import enclosed_regions

OUTSIDE = 0xFFFFFFFF               # the seed word of a vertex outside the volume (never a voxel: fewer than 2^32 - 1 voxels)
MAX_WAVES = 2048                   # 256 CUs x 8 resident waves of the kernel
SCRATCH_BUDGET = 4 << 30           # bytes: fewer concurrent waves on volumes whose faces are large


def seed_index(vox, shape):
    """(n, 3) integer voxel coordinates -> u32 linear indices x + sx*(y + sy*z), OUTSIDE for rows outside the volume"""
    vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    sx, sy, sz = (int(v) for v in shape)
    inside = np.all((vox >= 0) & (vox < np.array([sx, sy, sz], dtype=np.int64)), axis=1)
    lin = vox[:, 0] + sx * (vox[:, 1] + sy * vox[:, 2])
    return np.where(inside, lin, OUTSIDE).astype(np.uint32)


def hole_tables(eng, d_lab, label_bytes, shape, words, stats=None):
    """What cross_sections(filled=...) needs for sections of filled(L) = L u hole(L), made once per volume:
    the regions of the label volume (Engine.region_graph, ndim 3) and hole(L) for every device label word in `words`
    (kh_host_enclosed_regions).  Returns (d_region: u32 region id per voxel, resident; word_range: {word: (begin, count)} into
    d_hole_regions: the lists, resident, never empty so that it has an address).  Resident: 4 bytes per voxel plus the lists.
    stats (a dict) receives region_graph's info, enclosed_ms (the host search), csr_regions and labels_with_holes."""
    t = eng.torch
    marks = []

    def mark(name):
        if stats is not None:
            ev = t.cuda.Event(enable_timing=True)
            ev.record(t.cuda.current_stream(eng.device))
            marks.append((name, ev))

    d_region, value, _, face, pairs, info = eng.region_graph(d_lab, label_bytes, tuple(int(v) for v in shape), 3, mark)
    words = sorted(set(int(w) for w in words))
    t0 = time.perf_counter()
    offsets, regions = enclosed_regions(value, face, pairs, np.array(words, dtype=np.uint64))
    t1 = time.perf_counter()
    if regions.size >= 2 ** 32:
        raise ValueError("fewer than 2^32 hole regions in all")
    word_range = {w: (int(offsets[k]), int(offsets[k + 1] - offsets[k])) for k, w in enumerate(words)}
    host = regions if regions.size else np.zeros(1, dtype=np.uint32)
    d_hole_regions = t.from_numpy(host.view(np.int32).copy()).to(eng.device)
    if stats is not None:
        stats.update(info, enclosed_ms=(t1 - t0) * 1e3, csr_regions=int(regions.size),
                     labels_with_holes=sum(1 for w in words if word_range[w][1]))
        eng.sync_stream()
        for (name, a), (_, b) in zip(marks[0::2], marks[1::2]):
            stats[name + "_ms"] = stats.get(name + "_ms", 0.0) + a.elapsed_time(b)
    return d_region, word_range, d_hole_regions


def cross_sections(eng, d_lab, label_bytes, shape, anisotropy, seed_lin, want_label, normals, stats=None, filled=None):
    """d_lab: the label volume on the device (1-D, Fortran order, label_bytes 1 / 2 / 4); seed_lin, want_label: u32 [n] (seed_index;
    the unsigned word the section's voxels carry); normals: f64 [n, 3], any length.  Returns host arrays (area f32 [n], contact u8
    [n], voxels u32 [n]): kh_cross_sections' outputs.  stats (a dict) receives the kernel's milliseconds (HIP events), the items and
    the waves of the launch, accumulated over calls.
    filled = (d_region, hole_begin, hole_count, d_hole_regions) selects kh_cross_sections_filled, the sections of filled(label):
    d_region u32 [nvox] on the device (kh_regions6 on d_lab), hole_begin / hole_count u32 [n] on the host (item i's holes are
    d_hole_regions[hole_begin[i] : hole_begin[i] + hole_count[i]], ascending region ids; hole_tables makes them per label)."""
    return _sections(eng, d_lab, label_bytes, shape, anisotropy, seed_lin, want_label, normals, stats, filled, None)


def cross_sections_box(eng, d_lab, label_bytes, box_lo, box_shape, dataset_shape, anisotropy, seed_lin, want_label, normals, stats=None):
    """cross_sections for a label array that is the box [box_lo, box_lo + box_shape) of a dataset of dataset_shape voxels, which may
    hold 2^32 voxels or more (kh_cross_sections_box).  seed_lin: seed_index(voxel - box_lo, box_shape).  Returns host
    arrays (area f32 [n], contact u8 [n], clip u8 [n], voxels u32 [n]): contact names the faces of the DATASET, clip, in the same bits,
    the faces of the box that are cuts through the dataset.  An item with clip == 0 has the voxels, the contact and, bit for bit, the
    area that cross_sections gives on the whole dataset: the fixed point is the dataset's (kh_cross_sections_fixed_exponent).  The
    scratch is sized from the box: a small box gets small visited bitmaps and more concurrent waves.  stats as cross_sections."""
    lo = tuple(int(v) for v in box_lo)
    whole = tuple(int(v) for v in dataset_shape)
    if len(lo) != 3 or len(whole) != 3:
        raise ValueError("box_lo and dataset_shape have three entries")
    return _sections(eng, d_lab, label_bytes, box_shape, anisotropy, seed_lin, want_label, normals, stats, None, (lo, whole))


def cross_sections_filled_box(eng, d_lab, label_bytes, box_lo, box_shape, dataset_shape, anisotropy, seed_lin, want_label, normals,
                              filled, stats=None):
    """cross_sections_box for the sections of filled(label), hole(label) taken on the DATASET (kh_cross_sections_filled_box; DESIGN.md
    3.17).  filled = (d_region, hole_begin, hole_count, d_hole_regions) as cross_sections takes it, with d_region the box of the
    region store on the device (post.region_graph_chunked's provisional ids, u32 per voxel of the box) and the lists in those ids,
    ascending.  Returns cross_sections_box's four arrays; an item with clip == 0 has what cross_sections(filled=...) gives on the
    whole dataset, bit for bit in the area."""
    lo = tuple(int(v) for v in box_lo)
    whole = tuple(int(v) for v in dataset_shape)
    if len(lo) != 3 or len(whole) != 3:
        raise ValueError("box_lo and dataset_shape have three entries")
    if filled is None:
        raise ValueError("filled: (d_region, hole_begin, hole_count, d_hole_regions)")
    return _sections(eng, d_lab, label_bytes, box_shape, anisotropy, seed_lin, want_label, normals, stats, filled, (lo, whole))


def _sections(eng, d_lab, label_bytes, shape, anisotropy, seed_lin, want_label, normals, stats, filled, box):
    """the body of cross_sections (box None: three arrays) and of cross_sections_box / cross_sections_filled_box (box = (box_lo,
    dataset_shape): four)"""
    t, P = eng.torch, eng.ptr
    sx, sy, sz = (int(v) for v in shape)
    an = np.asarray(anisotropy, dtype=np.float64).reshape(-1)
    if an.shape != (3,) or not np.all(np.isfinite(an)) or not np.all(an > 0):
        raise ValueError("anisotropy must be three finite positive numbers")
    seed_lin = np.ascontiguousarray(seed_lin, dtype=np.uint32).reshape(-1)
    want_label = np.ascontiguousarray(want_label, dtype=np.uint32).reshape(-1)
    normals = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    n = int(seed_lin.size)
    assert want_label.size == n and normals.shape[0] == n
    if filled is not None:
        d_region, hole_begin, hole_count, d_hole_regions = filled
        hole_begin = np.ascontiguousarray(hole_begin, dtype=np.uint32).reshape(-1)
        hole_count = np.ascontiguousarray(hole_count, dtype=np.uint32).reshape(-1)
        assert hole_begin.size == n and hole_count.size == n
        if int(d_region.numel()) != sx * sy * sz or d_region.element_size() != 4:
            raise ValueError("region: one u32 per voxel (kh_regions6)")
        if n and int((hole_begin.astype(np.int64) + hole_count).max()) > int(d_hole_regions.numel()):
            raise ValueError("a hole range ends behind the region list")
    if box is not None:
        lo, whole = box
        if any(o < 0 or o + b > d for o, b, d in zip(lo, (sx, sy, sz), whole)):
            raise ValueError("the box %s + %s does not lie inside a dataset of shape %s" % (lo, (sx, sy, sz), whole))
        exponent = int(eng.lib.kh_cross_sections_fixed_exponent(whole[0], whole[1], whole[2], float(an[0]), float(an[1]), float(an[2])))
        if exponent == -2 ** 31:
            raise ValueError("the extents of the dataset must lie in [1, 2^31)")
    if n == 0:
        none = np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32)
        return none if box is None else none[:2] + (np.zeros(0, dtype=np.uint8), none[2])
    if label_bytes not in (1, 2, 4):
        raise ValueError("labels of 1, 2 or 4 bytes (kimimaro_amd.utility._narrow_labels)")
    per_wave = int(eng.lib.kh_cross_sections_scratch_bytes(sx, sy, sz, 2)) - int(eng.lib.kh_cross_sections_scratch_bytes(sx, sy, sz, 1))
    if per_wave <= 0:
        raise ValueError("the volume must hold fewer than 2^32 - 1 voxels")
    waves = max(1, min(n, MAX_WAVES, SCRATCH_BUDGET // per_wave))
    nbytes = int(eng.lib.kh_cross_sections_scratch_bytes(sx, sy, sz, waves))
    d_scratch = eng.empty((nbytes + 7) // 8, t.int64)
    d_seed = t.from_numpy(seed_lin.view(np.int32)).to(eng.device)
    d_want = t.from_numpy(want_label.view(np.int32)).to(eng.device)
    d_normals = t.from_numpy(normals.reshape(-1)).to(eng.device)
    d_area = eng.empty(n, t.float32)
    d_contact = eng.empty(n, t.uint8)
    d_voxels = eng.empty(n, t.int32)
    if stats is not None:
        stream = t.cuda.current_stream(eng.device)
        before, after = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        before.record(stream)
    if filled is not None:
        d_begin = t.from_numpy(hole_begin.view(np.int32)).to(eng.device)
        d_count = t.from_numpy(hole_count.view(np.int32)).to(eng.device)
    if box is not None:
        d_clip = eng.empty(n, t.uint8)
    if box is not None and filled is not None:
        _abi.check(eng.lib.kh_cross_sections_filled_box(P(d_lab), label_bytes, sx, sy, sz, float(an[0]), float(an[1]), float(an[2]), n,
                                                        P(d_seed), P(d_want), P(d_normals), P(d_region), P(d_begin), P(d_count),
                                                        P(d_hole_regions), lo[0], lo[1], lo[2], whole[0], whole[1], whole[2], exponent,
                                                        P(d_area), P(d_contact), P(d_voxels), P(d_clip), P(d_scratch), nbytes,
                                                        eng.stream()))
    elif box is not None:
        _abi.check(eng.lib.kh_cross_sections_box(P(d_lab), label_bytes, sx, sy, sz, float(an[0]), float(an[1]), float(an[2]), n, P(d_seed),
                                                 P(d_want), P(d_normals), lo[0], lo[1], lo[2], whole[0], whole[1], whole[2], exponent,
                                                 P(d_area), P(d_contact), P(d_voxels), P(d_clip), P(d_scratch), nbytes, eng.stream()))
    elif filled is None:
        _abi.check(eng.lib.kh_cross_sections(P(d_lab), label_bytes, sx, sy, sz, float(an[0]), float(an[1]), float(an[2]), n, P(d_seed),
                                             P(d_want), P(d_normals), P(d_area), P(d_contact), P(d_voxels), P(d_scratch), nbytes,
                                             eng.stream()))
    else:
        _abi.check(eng.lib.kh_cross_sections_filled(P(d_lab), label_bytes, sx, sy, sz, float(an[0]), float(an[1]), float(an[2]), n,
                                                    P(d_seed), P(d_want), P(d_normals), P(d_region), P(d_begin), P(d_count),
                                                    P(d_hole_regions), P(d_area), P(d_contact), P(d_voxels), P(d_scratch), nbytes,
                                                    eng.stream()))
    if stats is not None:
        after.record(stream)
    area = d_area.cpu().numpy()
    if int(d_scratch[1].item()) != 0:
        raise _abi.KimiHipError("kh_cross_sections: a section outgrew its queue")
    if stats is not None:
        stats["kernel_ms"] = stats.get("kernel_ms", 0.0) + before.elapsed_time(after)
        stats["items"] = stats.get("items", 0) + n
        stats["launches"] = stats.get("launches", 0) + 1
        stats["waves"] = waves
        stats["scratch_bytes"] = nbytes
    contact, voxels = d_contact.cpu().numpy(), d_voxels.cpu().numpy().view(np.uint32)
    return (area, contact, voxels) if box is None else (area, contact, d_clip.cpu().numpy(), voxels)
