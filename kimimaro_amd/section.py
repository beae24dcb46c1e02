"""Device plumbing of the plane sections (csrc/section.hip): a batch of (seed voxel, label, normal) items against the
label volume resident in HBM, one launch.  kimimaro_amd.utility.cross_sectional_area and kimimaro_amd.ops.cross_sectional_area are
the callers.  The library allocates nothing: the scratch (visited bitmaps and queue spill of the concurrent waves) is sized here."""
from __future__ import annotations

import numpy as np

from . import _abi

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


def cross_sections(eng, d_lab, label_bytes, shape, anisotropy, seed_lin, want_label, normals, stats=None):
    """d_lab: the label volume on the device (1-D, Fortran order, label_bytes 1 / 2 / 4); seed_lin, want_label: u32 [n] (seed_index;
    the unsigned word the section's voxels carry); normals: f64 [n, 3], any length.  Returns host arrays (area f32 [n], contact u8
    [n], voxels u32 [n]): kh_cross_sections' outputs.  stats (a dict) receives the kernel's milliseconds (HIP events), the items and
    the waves of the launch, accumulated over calls."""
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
    if n == 0:
        return np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32)
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
    _abi.check(eng.lib.kh_cross_sections(P(d_lab), label_bytes, sx, sy, sz, float(an[0]), float(an[1]), float(an[2]), n, P(d_seed),
                                         P(d_want), P(d_normals), P(d_area), P(d_contact), P(d_voxels), P(d_scratch), nbytes,
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
    return area, d_contact.cpu().numpy(), d_voxels.cpu().numpy().view(np.uint32)
