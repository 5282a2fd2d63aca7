"""UpdateModel: the contract of VHX_WRITE_UPDATE in numpy, on top of tests/_points_model.PointsModel. Under mode "update"
a point writes only the halves it has: the colour half of a voxel after the call is that of the highest-index point
naming it whose colour half is present (alpha byte not 0), else the old one; the data half is decided the same way,
independently. A point with neither half is not effective; the palettes grow as under "insert". apply_box is the same
for a dense box (write_dense / fill_box): its voxels as a list in the box's insert order (x outer, then y, z inner)."""
import numpy as np

from tests._points_model import PointsModel, _append_new, _words


def _last_of(key):
    """Index of the last occurrence of every distinct key."""
    _, last = np.unique(key[::-1], return_index=True)
    return key.size - 1 - last


class UpdateModel(PointsModel):
    def apply(self, positions, albedo=None, data=None, mode="replace"):
        if mode != "update":
            return super().apply(positions, albedo, data, mode)
        pos = np.asarray(positions, np.int64).reshape(-1, 3)
        n = pos.shape[0]
        a, d = _words(albedo, n), _words(data, n)
        a = np.where(a >> 24 != 0, a, 0).astype(np.uint32)  # an albedo with alpha 0 is no colour half
        self.colors = _append_new(self.colors, a[a != 0])  # every present half, overridden ones included
        self.values = _append_new(self.values, d[d != 0])
        size = self.vis.shape[0]
        for words, cube in ((a, self.vis), (d, self.dat)):
            has = words != 0
            p, w = pos[has], words[has]
            if not w.size:
                continue
            last = _last_of((p[:, 2] * size + p[:, 1]) * size + p[:, 0])
            cube[p[last, 2], p[last, 1], p[last, 0]] = w[last]

    def apply_box(self, grid, data, origin, mode):
        """A dense box: `grid` and `data` of shape (gz, gy, gx), `data` a plane, an integer or None."""
        grid = np.asarray(grid, np.uint32)
        gz, gy, gx = grid.shape
        plane = np.full(grid.shape, 0 if data is None else data, np.uint32) if data is None or np.isscalar(data) \
            else np.asarray(data, np.uint32)
        ox, oy, oz = origin
        x, y, z = np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij")  # x outer, z inner
        x, y, z = x.ravel(), y.ravel(), z.ravel()
        pos = np.stack([x + ox, y + oy, z + oz], 1)
        self.apply(pos, grid[z, y, x], plane[z, y, x], mode)
