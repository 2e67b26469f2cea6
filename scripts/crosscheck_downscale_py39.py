"""Record `skimage.measure.block_reduce` outputs for the restatement test of the downscaling
(tests/test_downscaling_ref.py).  Run by hand with a python that has scikit-image (recorded with
python 3.9, scikit-image 0.18.3, numpy 1.26); writes tests/golden/downscale_skimage.npz.

Per case the file holds the input `x<i>`, and per function `<func><i>`: what the reference's sampler
computes before its clip / round / cast, `block_reduce(x.astype('float32'), factors, np.<func>)`
(downscaling.py:276-278, :309-310), as float32.  `cases` lists [dtype, fz, fy, fx] per case.  The
integer cases must match the restatement exactly, the float cases within its bound.  The script
also compares against tests/downscaling_ref.py itself and prints the worst float deviation."""
import os
import sys

import numpy as np
from skimage.measure import block_reduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import downscaling_ref as R  # noqa: E402

FACTORS = [(1, 2, 2), (2, 2, 2), (1, 3, 3), (3, 3, 3), (1, 4, 4), (4, 4, 4), (2, 3, 5), (8, 8, 4)]
SHAPES = [(3, 5, 9), (4, 4, 8), (3, 7, 7), (4, 7, 8), (2, 9, 9), (5, 9, 10), (3, 7, 11), (9, 9, 5)]


def inputs(rng, dtype, shape, k):
    if dtype in ('uint8', 'uint16'):
        hi = np.iinfo(dtype).max
        if k % 4 == 3:
            return np.full(shape, hi, dtype=dtype)  # all-maximum: the largest sums
        return rng.randint(0, hi + 1, shape).astype(dtype)
    # floats of both signs over a wide range of magnitudes
    x = rng.standard_normal(shape) * np.exp2(rng.randint(-20, 21, shape))
    return x.astype(dtype)


def main():
    rng = np.random.RandomState(7)
    data, cases, worst = {}, [], 0.
    for k, (factors, shape) in enumerate(zip(FACTORS, SHAPES)):
        for dtype in ('uint8', 'uint16', 'float32', 'float64'):
            i = len(cases)
            x = inputs(rng, dtype, shape, k)
            cases.append([dtype] + [str(f) for f in factors])
            data['x%i' % i] = x
            for func in R.FUNCS:
                out = block_reduce(x.astype('float32'), block_size=factors, func=getattr(np, func))
                assert out.dtype == np.float32, out.dtype
                data['%s%i' % (func, i)] = out
                ref = R.reduce_block(x, factors, func, 'float32')
                if dtype in ('uint8', 'uint16') or func != 'mean':
                    assert np.array_equal(out, ref), (dtype, factors, func)
                else:
                    c = R.cells(x, factors).astype(np.float64)
                    n = int(np.prod(factors))
                    scale = n * 2. ** -24 * np.abs(c).mean(axis=(1, 3, 5))
                    worst = max(worst, float((np.abs(out.astype(np.float64) - c.mean(axis=(1, 3, 5))) / scale).max()))
    data['cases'] = np.array(cases)
    path = os.path.join(ROOT, 'tests', 'golden', 'downscale_skimage.npz')
    np.savez_compressed(path, **data)
    print("%i cases -> %s (%i bytes); skimage's float mean deviates from the exact mean by at most %.3f of "
          "n 2^-24 mean|x|" % (len(cases), path, os.path.getsize(path), worst))


if __name__ == '__main__':
    main()
