"""The adjoint of jacobian3 with ONE incoming gradient where the LDS-staged kernel's last workgroup is ragged: fewer than 1024 voxels
are left and the spans it stages (the 1024 records one slice up, the X records before its own) would pass the END of the gradient,
not only its beginning.  Those records belong to no voxel and are clamped to the tensor; the results are the oracle's, bit for bit.
Shapes: X % 4 == 0 and X <= 128 (the staged path); a single ragged block, and ragged blocks behind one and two full ones."""
import numpy as np
import pytest

import df_oracle as orc
from gpu_util import dev, host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (1, 4, 3, 12), (1, 2, 2, 128), (1, 3, 4, 100), (2, 3, 5, 40), (1, 17, 2, 64)])
def test_jacobian3_adjoint_of_one_gradient_in_a_ragged_last_block(shape):
    from deep_fluids_amd import ops
    nvox = int(np.prod(shape))
    left = nvox % 1024
    assert shape[3] % 4 == 0 and shape[3] <= 128 and 0 < left < 1024 - shape[2] * shape[3]      # the z-1 span passes the end
    rng = np.random.RandomState(sum(shape))
    x = rng.uniform(-1, 1, shape + (3,)).astype(np.float32)
    gj = rng.uniform(-1, 1, shape + (9,)).astype(np.float32)
    gc = rng.uniform(-1, 1, shape + (3,)).astype(np.float32)
    xt = dev(x).requires_grad_(True)
    j, c = ops.jacobian3(xt)
    (j * dev(gj)).sum().backward(retain_graph=True)
    np.testing.assert_array_equal(host(xt.grad), orc.jacobian3_bwd(gj=gj))
    xt.grad = None
    (c * dev(gc)).sum().backward()
    np.testing.assert_array_equal(host(xt.grad), orc.jacobian3_bwd(gc=gc))
