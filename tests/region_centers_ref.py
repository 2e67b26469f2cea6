"""CPU restatement of RegionCenters (cluster_tools/morphology/region_centers.py:106-133) in numpy,
for integer resolutions, where it is exact.

    d2(p)  for a voxel p of `obj`: the minimum over the box's voxels b outside `obj` of
           sum_a (r_a (p_a - b_a))^2, an exact integer (brute force over the background voxels: the
           boxes of the tests are small); 0 for the voxels outside `obj`
    centre the first voxel in C order with the largest d2.  scipy forms the same d2 exactly in
           float64 and sqrt is strictly increasing on the integers below 2^52, so this is
           `np.argmax(distance_transform_edt(obj, sampling=r))`
    a box without background: scipy 1.15 acts as if one background voxel sat at local (-1, 0, 0),
           d = sqrt(((z + 1) r_z)^2 + (y r_y)^2 + (x r_x)^2), so the centre is the last voxel
"""
import numpy as np


def squared_edt(obj, resolution=(1, 1, 1)):
    """d2 (int64, obj's shape) of a 3-D boolean box that holds at least one background voxel."""
    obj = np.asarray(obj, dtype=bool)
    r = np.array([int(v) for v in resolution], dtype=np.int64)
    assert not obj.all(), "a box without background has no distances"
    fg = np.argwhere(obj).astype(np.int64)
    # The minimum is taken over the background voxels with a 6-neighbour in obj only.  That loses
    # nothing: from the nearest background voxel b of p one step towards p along an axis on which
    # they differ is strictly nearer to p at any positive resolution, so that voxel is in obj.
    near = np.zeros(obj.shape, dtype=bool)
    for a in range(3):
        lo = tuple(slice(None, -1) if d == a else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == a else slice(None) for d in range(3))
        near[lo] |= obj[hi]
        near[hi] |= obj[lo]
    bg = np.argwhere(~obj & near).astype(np.int64)
    if not len(fg):
        return np.zeros(obj.shape, dtype=np.int64)
    d2 = np.zeros(obj.shape, dtype=np.int64)
    step = max(1, (1 << 20) // len(bg))  # bounded memory
    for s in range(0, len(fg), step):
        p = fg[s:s + step]
        diff = (p[:, None, :] - bg[None, :, :]) * r
        d2[tuple(p.T)] = (diff * diff).sum(axis=2).min(axis=1)
    return d2


def box_center(obj, resolution=(1, 1, 1)):
    """(z, y, x) of the centre of a non-empty 3-D boolean box with at least one true voxel, or None
    when it holds none (or is empty)."""
    obj = np.asarray(obj, dtype=bool)
    if obj.size == 0 or not obj.any():
        return None
    if obj.all():
        return tuple(int(s) - 1 for s in obj.shape)
    d2 = squared_edt(obj, resolution)
    return tuple(int(c) for c in np.unravel_index(int(np.argmax(d2)), obj.shape))


def centers_for_crops(crops, ids, resolution=(1, 1, 1)):
    """What Handle.region_centers returns: (centers int64 (k, 3), found bool (k,))."""
    centers = np.zeros((len(crops), 3), dtype=np.int64)
    found = np.zeros(len(crops), dtype=bool)
    for i, (crop, label_id) in enumerate(zip(crops, ids)):
        c = box_center(np.asarray(crop) == np.uint64(label_id), resolution)
        if c is not None:
            centers[i] = c
            found[i] = True
    return centers, found


def centers_for_boxes(labels, ids, boxes, resolution=(1, 1, 1)):
    """The same for (k, 6) boxes [begin, end) inside one volume."""
    crops = [labels[tuple(slice(int(b), max(int(b), int(e))) for b, e in zip(box[:3], box[3:]))] for box in boxes]
    return centers_for_crops(crops, ids, resolution)


def region_centers_table(labels, morphology, number_of_labels, ignore_label=None, resolution=(1, 1, 1)):
    """The task's output table (number_of_labels, 3) float32 from a volume and its morphology table:
    rules 1-6 of DESIGN.md section 3.10.  The box is [min, max) of columns 5:8 and 8:11 cast to
    uint64 (the maxima are inclusive: the last plane of every axis is left out, as the reference
    leaves it out); an id that is ignored, has no table row, an empty box or no voxel in its box
    keeps its zero row."""
    bb_start = morphology[:, 5:8].astype('uint64')
    bb_stop = morphology[:, 8:11].astype('uint64')
    centers = np.zeros((number_of_labels, 3), dtype='float32')
    for label_id in range(number_of_labels):
        if ignore_label == label_id or label_id >= len(morphology):
            continue
        bb = tuple(slice(int(b), int(e)) for b, e in zip(bb_start[label_id], bb_stop[label_id]))
        obj = labels[bb] == label_id
        c = box_center(obj, resolution)
        if c is None:
            continue
        centers[label_id] = [ci + s.start for ci, s in zip(c, bb)]
    return centers
