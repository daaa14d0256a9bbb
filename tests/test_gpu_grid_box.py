"""The block tail every box reduction shares (gh_box_block, grid.h), through the single-cloud entry ghicp_cloud_bounds (k_bbox, ctx.hip), against
numpy's min / max, exactly.  The batched box kernels (batch.hip, prepare_clouds.hip, refine_recip.hip) call the same tail and are held to this
one byte for byte by test_gpu_batch.py, test_gpu_prepare_clouds.py and test_gpu_refine_reciprocal.py.
Sizes: one point; around a wave (63, 64, 65); around the 256-thread workgroup (255, 256, 257); and 256 * 2048 + 1, one point more than one pass of the
grid-stride loop at its cap of 2048 blocks.  Strides 3 and 4 (the fourth column holds values outside the box: it must not be read as a coordinate).
Clouds: mixed signs with the extreme point LAST (the lane that loads it is the last to have work); all coordinates negative and a cloud that spans
-0.0 / +0.0 (the two branches of the order-preserving float -> int encoding, and its seam: enc(-0.0) = -1, enc(+0.0) = 0).  The sign cases run at
the seven small sizes; the large size runs the extreme-point-last cloud, the one its second pass is about (the file stays cheap on the interpreter)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 256 * 2048 + 1)


def _clouds(n, rng):
    mixed = rng.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    mixed[-1] = (-60.0, 70.0, -80.0)  # min of x and z, max of y: in the last point alone
    yield "extreme point last", mixed
    if n > 257:  # the large size is about the second pass of the grid-stride loop, which loads exactly this last point; the sign cases are the small sizes'
        return
    yield "all negative", -rng.uniform(1e-3, 900.0, (n, 3)).astype(np.float32)
    span = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    span[rng.integers(0, n, max(1, n // 7))] = -0.0
    span[rng.integers(0, n, max(1, n // 7))] = 0.0
    yield "spans zero", span
    zeros = np.zeros((n, 3), np.float32)
    zeros[::2] = -0.0
    yield "only -0.0 and +0.0", zeros


@pytest.mark.parametrize("stride", (3, 4))
@pytest.mark.parametrize("n", SIZES)
def test_cloud_bounds_equal_numpy_min_max(ctx, n, stride):
    rng = np.random.default_rng(1000 * n + stride)
    for name, xyz in _clouds(n, rng):
        cloud = xyz if stride == 3 else np.concatenate([xyz, np.full((n, 1), 1.0e6, np.float32) * rng.choice((-1.0, 1.0), (n, 1)).astype(np.float32)], axis=1)
        b = np.asarray(ctx.cloud_bounds(np.ascontiguousarray(cloud)), np.float64)
        # floats returned as doubles: equality of values is equality of bits (no NaN; -0.0 == +0.0, whose sign min / max leave open)
        np.testing.assert_array_equal(b[:3], xyz.min(axis=0).astype(np.float64), err_msg="%s: min, n = %d, stride %d" % (name, n, stride))
        np.testing.assert_array_equal(b[3:], xyz.max(axis=0).astype(np.float64), err_msg="%s: max, n = %d, stride %d" % (name, n, stride))
