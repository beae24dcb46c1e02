"""CPU statement of kh_cross_sections_box on tests/section_ref.py: the section of the CROPPED box, with the faces of the
dataset (contact) and the cut faces of the box (clip) read off its voxel list.  numpy only, independent of the product."""
import numpy as np

import section_ref

OUTSIDE = 0xFFFFFFFF


def face_bits(vox, box_lo, box_shape, dataset_shape):
    """(contact, clip) of a section's voxel list `vox` (k, 3), box coordinates"""
    contact = clip = 0
    for axis in range(3):
        lo, b, d = int(box_lo[axis]), int(box_shape[axis]), int(dataset_shape[axis])
        low, high = bool(np.any(vox[:, axis] == 0)), bool(np.any(vox[:, axis] == b - 1))
        contact |= (1 << (2 * axis)) * bool(np.any(vox[:, axis] + lo == 0)) | (2 << (2 * axis)) * bool(np.any(vox[:, axis] + lo == d - 1))
        clip |= (1 << (2 * axis)) * (low and lo > 0) | (2 << (2 * axis)) * (high and lo + b < d)
    return contact, clip


def section_in_box(box, box_lo, dataset_shape, seed, normal, anisotropy, label):
    """box: the cropped labels [x, y, z]; seed: box coordinates -> (voxels, area float64, contact, clip)"""
    vox, area, _ = section_ref.section(box, seed, normal, anisotropy, label)
    if len(vox) == 0:
        return 0, 0.0, 0, 0
    contact, clip = face_bits(vox, box_lo, box.shape, dataset_shape)
    return len(vox), area, contact, clip


def halo_box(voxel, chunk_shape, halo, dataset_shape):
    """(lo, hi) of the box of the core that holds `voxel`"""
    v, c, d = np.asarray(voxel, dtype=np.int64), np.asarray(chunk_shape, dtype=np.int64), np.asarray(dataset_shape, dtype=np.int64)
    core_lo = (v // c) * c
    return np.maximum(core_lo - halo, 0), np.minimum(np.minimum(core_lo + c, d) + halo, d)


class FakeSections:
    """A launcher with the signature of kimimaro_amd.section.cross_sections_box on the statement: d_lab is the box as a host array
    [x, y, z], the words are the labels.  `calls` records (box_lo, box_shape, the seeds in dataset coordinates) per launch."""

    def __init__(self):
        self.calls = []

    def __call__(self, eng, d_lab, label_bytes, box_lo, box_shape, dataset_shape, anisotropy, seed_lin, want_label, normals, stats=None):
        assert eng is None and tuple(d_lab.shape) == tuple(int(v) for v in box_shape) and d_lab.dtype.itemsize == label_bytes
        bx, by, bz = (int(v) for v in box_shape)
        lo = np.array([int(v) for v in box_lo], dtype=np.int64)
        n = len(seed_lin)
        area, contact, clip = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        voxels = np.zeros(n, dtype=np.uint32)
        seeds = []
        for i in range(n):
            lin = int(seed_lin[i])
            if lin == OUTSIDE:
                seeds.append(None)
                continue
            seed = (lin % bx, (lin // bx) % by, lin // (bx * by))
            seeds.append(tuple(int(v) for v in lo + seed))
            k, a, c, p = section_in_box(d_lab, lo, dataset_shape, seed, normals[i], anisotropy, int(want_label[i]))
            area[i], contact[i], clip[i], voxels[i] = np.float32(a), c, p, k
        self.calls.append((tuple(lo.tolist()), (bx, by, bz), seeds))
        return area, contact, clip, voxels
