"""What tests/test_gpu_update_voxels.py and tests/test_gpu_dense_update.py share: the numpy model of VHX_WRITE_UPDATE
(tests/_update_model.py) beside a Raytracer, with the checks of tests/test_gpu_set_voxels.Model after every call --
both palettes, both read_dense planes, get at every position against the model and the walker, structure, a frame
against the oracle, headers and bitmaps against a second context's upload -- and data-carrying bases."""
import numpy as np

from tests import _dense_data_grids as DG
from tests import _simplify_grids as SG
from tests import test_gpu_set_voxels as S
from tests._update_model import UpdateModel

COLOURS, VALUES = S.COLOURS, S.VALUES
to_device, positions, cached, brick_cells = S.to_device, S.positions, S.cached, S.brick_cells


class Model(UpdateModel, S.Model):
    """S.Model (construction from the device, set, clear, check) with the update rule and the dense calls."""

    def update(self, pos, albedo=None, data=None, source="host"):
        dev = (lambda w: w if w is None or np.isscalar(w) else to_device(w)) if source == "tensor" else (lambda w: w)
        self.rt.update_voxels(dev(pos), dev(albedo), dev(data))
        self.apply(pos, albedo, data, "update")

    def write(self, grid, data=None, origin=(0, 0, 0), mode="update", source="host"):
        """`data`: a plane, an integer (fill_data) or None (vhx_write_dense)."""
        dev = (lambda w: w if w is None or np.isscalar(w) else to_device(w)) if source == "tensor" else (lambda w: w)
        self.rt.write_dense(dev(grid), origin, mode, data=dev(data))
        self.apply_box(grid, data, origin, mode)

    def fill(self, origin, extents, albedo, data=0, mode="update"):
        gx, gy, gz = extents
        self.rt.fill_box(origin, extents, albedo, data, mode=mode)
        self.apply_box(np.full((gz, gy, gx), albedo, np.uint32), data, origin, mode)


def data_pair(size):
    """The sparse grid with a data plane: none, colour-only, data-only and both inside one brick."""
    return cached(("update pair", size), lambda: DG.make_pair("sparse", size))


def data_base(rt, size, bd, source="host"):
    g, d = data_pair(size)
    if source == "tensor":
        g, d = to_device(g), to_device(d)
    rt.build_dense(g, size, bd, data=d)
    return Model(rt, size, bd)


def simplified_pair(kind, size, bd):
    """A grid of tests/_simplify_grids with a data plane that is constant over aligned 4 * brick_dim cubes (so Solid
    bricks and UniformLeaf nodes survive) and 0 over a part of them."""
    def make():
        g = DG.extend(SG.make_grid(kind, size, bd), size)
        n = size // (4 * bd)
        coarse = np.array([0, 7, 9], np.uint32)[np.random.default_rng(size + bd).integers(0, 3, (n, n, n))]
        d = coarse.repeat(4 * bd, 0).repeat(4 * bd, 1).repeat(4 * bd, 2)
        return g, np.where(g >> 24 != 0, d, 0).astype(np.uint32)
    return cached(("update simplified", kind, size, bd), make)
