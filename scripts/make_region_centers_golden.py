#!/usr/bin/env python
"""Writes tests/golden/region_centers_scipy.npz: small boolean boxes and scipy's
`np.argmax(distance_transform_edt(box, sampling=r))` for each of four integer resolutions, the
recorded reference of tests/test_region_centers_ref.py and tests/test_region_centers_gpu.py.

    shapes (n, 3), bits (the boxes' voxels in C order, one after another, np.packbits), kinds (n,)
    resolutions (4, 3), argmax (n, 4) the flat index per box and resolution, scipy_version

Needs scipy; the tests do not."""
import os

import numpy as np
import scipy
from scipy.ndimage import distance_transform_edt

RESOLUTIONS = [(1, 1, 1), (10, 1, 1), (1, 1, 10), (2, 3, 5)]


def boxes():
    rng = np.random.RandomState(2024)
    out = []
    for fill in (.5, .8, .95):
        for _ in range(9):
            shape = tuple(int(s) for s in rng.randint(1, 10, 3))
            box = rng.rand(*shape) < fill
            if not box.any():
                box.flat[rng.randint(box.size)] = True
            out.append(('random%i' % round(100 * fill), box))
    for shape in ((1, 1, 1), (1, 1, 2), (3, 1, 1), (2, 3, 4), (5, 5, 5), (1, 7, 3)):
        out.append(('full', np.ones(shape, dtype=bool)))
    for shape, hole in (((1, 4, 4), (0, 0, 0)), ((3, 3, 3), (1, 1, 1)), ((4, 5, 6), (3, 0, 4)), ((1, 1, 9), (0, 0, 8)),
                        ((2, 2, 2), (1, 1, 1))):
        box = np.ones(shape, dtype=bool)
        box[hole] = False
        out.append(('one_hole', box))
    # a hollow shell: two voxels thick, background inside and outside
    zz, yy, xx = np.ogrid[:9, :9, :9]
    cheb = np.maximum(np.maximum(abs(zz - 4), abs(yy - 4)), abs(xx - 4))
    out.append(('shell', (cheb >= 2) & (cheb <= 3)))
    # two blobs with equal maxima: the first in C order wins
    box = np.zeros((5, 5, 12), dtype=bool)
    box[1:4, 1:4, 1:4] = True
    box[1:4, 1:4, 8:11] = True
    out.append(('two_blobs', box))
    # a slab with a shell of background one voxel thick: flat ties along every axis
    box = np.zeros((7, 9, 70), dtype=bool)
    box[1:-1, 1:-1, 1:-1] = True
    out.append(('slab', box))
    return out


def main():
    cases = boxes()
    shapes = np.array([b.shape for _, b in cases], dtype=np.int64)
    bits = np.packbits(np.concatenate([b.reshape(-1) for _, b in cases]))
    argmax = np.array([[int(np.argmax(distance_transform_edt(b, sampling=r))) for r in RESOLUTIONS]
                       for _, b in cases], dtype=np.int64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden',
                        'region_centers_scipy.npz')
    np.savez_compressed(path, shapes=shapes, bits=bits, kinds=np.array([k for k, _ in cases]),
                        resolutions=np.array(RESOLUTIONS, dtype=np.int64), argmax=argmax,
                        scipy_version=np.array(scipy.__version__))
    print("%i boxes, %i bytes -> %s" % (len(cases), os.path.getsize(path), os.path.normpath(path)))


if __name__ == '__main__':
    main()
