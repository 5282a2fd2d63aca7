"""The dense grids shared by tests/test_dense_build.py (host builder) and tests/test_gpu_dense_build.py (device builder):
for every tree size the smallest grids that reach each structural case, generated from seeds."""
import numpy as np

import voxelhex_amd as vhx

# (size, brick_dim): D = 0 (the root is the leaf), D = 1 and D = 2
SIZES = [(4, 1), (16, 1), (16, 4), (32, 2), (64, 4), (64, 16), (32, 8)]
KINDS = ["sparse", "full", "zero", "corner"]


def rgba(r, g, b, a=255):
    return np.uint32(r | (g << 8) | (b << 16) | (a << 24))


# five colours, one of them with alpha 0 (no voxel)
COLORS = np.array([rgba(200, 30, 30), rgba(30, 200, 30), rgba(30, 30, 200, 7), rgba(9, 9, 9, 0), rgba(255, 255, 0)],
                  np.uint32)


def odd_extents(size):
    """Extents (gx, gy, gz) that are no multiples of the brick: (29, 17, 32) in a 32^3 tree."""
    return max(1, size - 3), max(1, size // 2 + 1), size


def make_grid(kind, size, seed=0):
    """A grid of shape (gz, gy, gx)."""
    rng = np.random.default_rng(seed * 1000 + size)
    if kind == "sparse":  # about 1 voxel in 7, extents off the brick grid
        gx, gy, gz = odd_extents(size)
        g = np.zeros((gz, gy, gx), np.uint32)
        mask = rng.random(g.shape) < 1 / 7
        g[mask] = COLORS[rng.integers(0, len(COLORS), int(mask.sum()))]
        return g
    if kind == "full":
        return np.full((size, size, size), rgba(10, 20, 30), np.uint32)
    if kind == "zero":
        return np.zeros((size, size, size), np.uint32)
    if kind == "corner":
        g = np.zeros((size, size, size), np.uint32)
        g[-1, -1, -1] = rgba(1, 2, 3)
        return g
    raise ValueError(kind)


def palette_order_grid():
    """Colour A only at (1,0,0), colour B only at (0,0,1): memory order meets A first, the insert loop B."""
    g = np.zeros((4, 4, 4), np.uint32)
    a, b = rgba(250, 0, 0), rgba(0, 0, 250)
    g[0, 0, 1] = a  # (x, y, z) = (1, 0, 0)
    g[1, 0, 0] = b  # (x, y, z) = (0, 0, 1)
    return g, [b, a]


def many_colors_grid(n=5000, size=64, seed=3):
    """n distinct colours at random places of a size^3 grid (table collisions)."""
    rng = np.random.default_rng(seed)
    g = np.zeros(size ** 3, np.uint32)
    at = rng.choice(size ** 3, n, replace=False)
    g[at] = (rng.permutation(1 << 24)[:n].astype(np.uint32)) | np.uint32(0xFF000000)
    return g.reshape(size, size, size)


def distinct_colors_grid(n):
    """A 41x40x40 grid (gx, gy, gz) whose first n voxels in memory order have n distinct colours."""
    g = np.zeros(40 * 40 * 41, np.uint32)
    g[:n] = np.arange(1, n + 1, dtype=np.uint32) | np.uint32(0xFF000000)
    return g.reshape(40, 40, 41)


def insert_loop(grid, size, bd):
    """The reference: BoxTree(size, bd) filled by insert in x-outer, y, z-inner order, flattened."""
    t = vhx.BoxTree(size, bd)
    gz, gy, gx = grid.shape
    for x in range(gx):
        for y in range(gy):
            col = grid[:, y, x]
            for z in np.flatnonzero(col):
                t.insert((x, y, int(z)), vhx.Albedo.from_packed(int(col[z])))
    return t.flatten()


ARRAYS = ("node_type", "node_ocbits", "node_children", "voxels", "solid_values", "color_palette", "data_palette")


def assert_same_image(got, want, what=""):
    for k in ARRAYS:
        a, b = getattr(got, k), getattr(want, k)
        assert a.shape == b.shape, f"{what}: {k} {a.shape} != {b.shape}"
        assert a.dtype == b.dtype, f"{what}: {k} dtype"
        assert np.array_equal(a, b), f"{what}: {k} differs at {np.flatnonzero(a != b)[:8]}"
    assert got.counts() == want.counts(), what
