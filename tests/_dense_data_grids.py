"""Dense grids with a data plane, shared by tests/test_dense_data.py (host builder), tests/test_gpu_dense_data.py and
tests/test_gpu_dense_data_write.py (device): the grids of tests/_dense_grids.py with a data plane drawn from an
independent seeded mask over the whole extents, so that none, colour-only, data-only and both occur inside one brick."""
import numpy as np

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from tests import _dense_grids as G

SIZES = G.SIZES + [(64, 1)]  # (64, 1): three node levels
KINDS = G.KINDS
DATA_VALUES = np.array([7, 9, 0x80000000, 0xFFFFFFFF], np.uint32)
EMPTY = np.uint32(N.VHX_EMPTY)


def make_data(shape, seed, density=1 / 5):
    rng = np.random.default_rng(seed * 7919 + 17 + int(np.prod(shape)))
    d = np.zeros(shape, np.uint32)
    mask = rng.random(shape) < density
    d[mask] = DATA_VALUES[rng.integers(0, len(DATA_VALUES), int(mask.sum()))]
    return d


def make_pair(kind, size, seed=0):
    """(albedo grid, data plane) of shape (gz, gy, gx)."""
    g = G.make_grid(kind, size, seed)
    return g, make_data(g.shape, seed)


def visible(grid):
    """The albedo plane with its alpha-0 words zeroed."""
    return np.where(grid >> 24 != 0, grid, 0).astype(np.uint32)


def entry_of(a, d):
    """The entry of a voxel by the rule, or None."""
    a, d = int(a), int(d)
    if (a >> 24) == 0:
        return vhx.BoxTreeEntry.Informative(d) if d else None
    alb = vhx.Albedo.from_packed(a)
    return vhx.BoxTreeEntry.Complex(alb, d) if d else vhx.BoxTreeEntry.Visual(alb)


def insert_tree(grid, data, size, bd):
    """The reference: BoxTree(size, bd) filled by insert in x-outer, y, z-inner order with kinds from the rule."""
    t = vhx.BoxTree(size, bd)
    gz, gy, gx = grid.shape
    some = (grid >> 24 != 0) | (data != 0)
    for x in range(gx):
        for y in range(gy):
            for z in np.flatnonzero(some[:, y, x]):
                t.insert((x, y, int(z)), entry_of(grid[z, y, x], data[z, y, x]))
    return t


def insert_loop(grid, data, size, bd):
    return insert_tree(grid, data, size, bd).flatten()


def extend(plane, size):
    """A plane zero-extended to the root cube."""
    out = np.zeros((size, size, size), np.uint32)
    gz, gy, gx = plane.shape
    out[:gz, :gy, :gx] = plane
    return out


def flat_data(image, values):
    """What vhx_read_dense_data writes for a value: data_palette[v >> 16] when v is not VHX_EMPTY and the index is
    neither 0xFFFF nor past the palette; else 0."""
    v = np.asarray(values, np.uint32)
    dp = image.data_palette
    di = (v >> 16).astype(np.int64)
    ok = (v != EMPTY) & (di != 0xFFFF) & (di < dp.size)
    if not dp.size:
        return np.zeros(v.shape, np.uint32)
    return np.where(ok, dp[np.minimum(di, dp.size - 1)], np.uint32(0)).astype(np.uint32)


def distinct_data_grid(n):
    """(albedo, data) of the 41x40x40 grid of G.distinct_colors_grid: one colour throughout the first n voxels in memory
    order, which carry n distinct data values (the largest ones: bit 31 set)."""
    d = np.zeros(40 * 40 * 41, np.uint32)
    d[:n] = np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32)
    g = np.where(d != 0, G.rgba(3, 2, 1), 0).astype(np.uint32)
    return g.reshape(40, 40, 41), d.reshape(40, 40, 41)


def many_data_grid(n=5000, size=64, seed=5):
    """n distinct data values at random places of a size^3 grid (table collisions), half of them under a colour."""
    rng = np.random.default_rng(seed)
    d = np.zeros(size ** 3, np.uint32)
    at = rng.choice(size ** 3, n, replace=False)
    d[at] = rng.permutation(1 << 24)[:n].astype(np.uint32) + np.uint32(1)
    g = np.zeros(size ** 3, np.uint32)
    g[at[::2]] = G.COLORS[0]
    g[rng.choice(size ** 3, n, replace=False)] = G.COLORS[1]
    return g.reshape(size, size, size), d.reshape(size, size, size)
