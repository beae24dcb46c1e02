"""CPU statement of the sections of FILLED labels (cross_sectional_area(fill_holes=True)): numpy and scipy
only, independent of the product.  filled(L) = {labels == L} u hole(L), hole(L) = the 6-connected components of {labels != L} that
own no voxel on a face of the array (an axis of extent 1 puts every voxel on a face) -- tests/fill_ref.static's rule; a filled section
is tests/section_ref.section on that mask."""
import numpy as np
import scipy.ndimage as ndi

import section_ref


def filled_mask(labels, L):
    labels = np.asarray(labels)
    comp, _ = ndi.label(labels != L)
    on_face = {0}
    for axis in range(comp.ndim):
        for index in (0, -1):
            on_face.update(np.unique(np.take(comp, index, axis=axis)).tolist())
    return (labels == L) | ~np.isin(comp, sorted(on_face))


def section_filled(labels, seed, normal, anisotropy, L, grid=None, mask=None):
    """-> (voxels, area float64, contact) of the section of filled(L); mask: filled_mask(labels, L) when the caller has it"""
    if mask is None:
        mask = filled_mask(labels, L)
    return section_ref.section(mask, seed, normal, anisotropy, True, grid)
