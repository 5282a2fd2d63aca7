"""PointsModel: the contract of vhx_set_voxels in numpy. From a list of positions, albedo words and data words it keeps
the expected cubes -- `vis` and `dat`, what read_dense(data=True) gives, and `val()`, what get gives -- and the two
palettes: the highest index decides a voxel, insert mode skips points without an entry, and new values follow the
palettes in the order of their first appearance among the effective points, overridden ones included."""
import numpy as np

from voxelhex_amd import _native as N

EMPTY = np.uint32(N.VHX_EMPTY)


def _words(w, n):
    return np.full(n, 0 if w is None else w, np.uint32) if w is None or np.isscalar(w) else np.asarray(w, np.uint32)


def _append_new(palette, values):
    """`palette` with the values it does not hold appended in the order of their first appearance in `values`."""
    uniq, first = np.unique(values, return_index=True)
    held = set(int(v) for v in palette)
    return palette + [int(values[i]) for i in np.sort(first) if int(values[i]) not in held]


def _lowest_index(palette, wanted, skip_zero):
    """Lowest index in `palette` of every value of `wanted` (an entry equal to 0 of a data palette is never matched)."""
    pal = np.asarray(palette, np.uint32)
    idx = np.arange(pal.size)
    if skip_zero:
        idx = idx[pal != 0]
    uniq, first = np.unique(pal[idx], return_index=True)
    at = np.searchsorted(uniq, wanted)
    assert wanted.size == 0 or (uniq[np.minimum(at, uniq.size - 1)] == wanted).all(), "a value is not in its palette"
    return idx[first[at]].astype(np.uint32)


class PointsModel:
    def __init__(self, vis, dat, color_palette, data_palette):
        self.vis, self.dat = np.array(vis, np.uint32), np.array(dat, np.uint32)
        self.colors = [int(c) for c in color_palette]
        self.values = [int(v) for v in data_palette]

    def apply(self, positions, albedo=None, data=None, mode="replace"):
        pos = np.asarray(positions, np.int64).reshape(-1, 3)
        n = pos.shape[0]
        a, d = _words(albedo, n), _words(data, n)
        a = np.where(a >> 24 != 0, a, 0).astype(np.uint32)  # an albedo with alpha 0 never reaches the palette
        eff = np.ones(n, bool) if mode == "replace" else (a != 0) | (d != 0)
        pos, a, d = pos[eff], a[eff], d[eff]
        self.colors = _append_new(self.colors, a[a != 0])
        self.values = _append_new(self.values, d[d != 0])
        size = self.vis.shape[0]
        key = (pos[:, 2] * size + pos[:, 1]) * size + pos[:, 0]
        _, last = np.unique(key[::-1], return_index=True)  # the last point of every voxel decides it
        last = key.size - 1 - last
        z, y, x = pos[last, 2], pos[last, 1], pos[last, 0]
        self.vis[z, y, x] = a[last]
        self.dat[z, y, x] = d[last]

    def val(self):
        ci = np.full(self.vis.shape, 0xFFFF, np.uint32)
        di = np.full(self.vis.shape, 0xFFFF, np.uint32)
        ci[self.vis != 0] = _lowest_index(self.colors, self.vis[self.vis != 0], False)
        di[self.dat != 0] = _lowest_index(self.values, self.dat[self.dat != 0], True)
        return np.where((self.vis != 0) | (self.dat != 0), ci | (di << np.uint32(16)), EMPTY).astype(np.uint32)


def random_points(rng, size, n, colours, values, lo=(0, 0, 0), hi=None, none=0.3):
    """n points in [lo, hi) with albedo and data words drawn from `colours` / `values`; about `none` of each half is 0."""
    hi = hi or (size,) * 3
    pos = np.stack([rng.integers(lo[k], hi[k], n) for k in range(3)], 1).astype(np.uint32)
    a = np.asarray(colours, np.uint32)[rng.integers(0, len(colours), n)]
    d = np.asarray(values, np.uint32)[rng.integers(0, len(values), n)]
    a[rng.random(n) < none] = 0
    d[rng.random(n) < none] = 0
    return pos, a, d
