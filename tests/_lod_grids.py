"""The grids and host references shared by tests/test_lod_model.py (vhx_flat_lod) and tests/test_gpu_build_lod.py
(vhx_build_lod): sparse grids of few colours from the generators of tests/_dense_grids.py and tests/_dense_data_grids.py,
one per tree shape that samples differently, and the host BoxTree route the LOD image is pinned to."""
import functools

import numpy as np

import voxelhex_amd as vhx
from voxelhex_amd.boxtree import BoxTree, MIPResamplingMethods
from tests import _dense_data_grids as DG
from tests import _dense_grids as G

# name -> (size, brick_dim, leaf depth): two levels; three levels (Internal sampling over Internal MIPs); a parent cell
# spanning eight children; a parent cell sampling an eighth of one child; one cell over a leaf of 64 bricks
SHAPES = {"64/4": (64, 4, 1), "256/4": (256, 4, 2), "128/2": (128, 2, 2), "128/8": (128, 8, 1), "4/1": (4, 1, 0)}
METHODS = ["box", "point"]
PAIR = {"box": MIPResamplingMethods.BoxFilter, "point": MIPResamplingMethods.PointFilter}


@functools.lru_cache(maxsize=None)
def pair(name):
    """(albedo grid, data plane) of shape (gz, gy, gx): the sparse grid of five colours (one of alpha 0) with data values
    on an independent mask, so data-only voxels and voxels of both halves sit in one brick. The larger trees keep a few
    slabs only, which leaves whole subtrees empty and the host reference quick."""
    size = SHAPES[name][0]
    g, d = DG.make_pair("sparse", size)
    if size >= 128:
        keep = np.zeros(g.shape, bool)
        q = size // 4
        keep[: q // 2, : q + 3, : q + 5] = True                   # a corner: neighbouring leaves under one parent
        keep[size - q - 1:, : q // 4, size // 2: size // 2 + 9] = True  # and a far one under another parent
        g, d = np.where(keep, g, 0).astype(np.uint32), np.where(keep, d, 0).astype(np.uint32)
    g.setflags(write=False)
    d.setflags(write=False)
    return g, d


def apply_strategy(tree, method):
    """`method` with a colour-similarity threshold of 0 on every MIP level (a level is log2(node edge / brick_dim))."""
    s = tree.albedo_mip_map_resampling_strategy()
    for level in range(0, 26):
        s.set_method_at(level, PAIR[method])
        s.set_color_similarity_thr_at(level, 0.0)
    return s


def host_lods(tree, method, depths):
    """The host BoxTree route: the strategy, switch_albedo_mip_maps(True), then flatten_lod(d) for every d."""
    apply_strategy(tree, method).switch_albedo_mip_maps(True)
    return {d: tree.flatten_lod(d) for d in depths}


def assert_same_lod(got, want, what=""):
    """All seven buffers, the counts and node_mips."""
    G.assert_same_image(got, want, what)
    a, b = np.asarray(got.node_mips), np.asarray(want.node_mips)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: node_mips differ at {np.flatnonzero(a != b)[:8]}"


def edit_loop_tree(size=32, bd=2, seed=5):
    """A host BoxTree after an insert, clear and update loop, with Complex voxels of alpha 0 and data-only voxels."""
    rng = np.random.default_rng(seed)
    t = BoxTree(size, bd)
    cols = [vhx.Albedo.from_packed(int(c)) for c in G.COLORS]
    pos = rng.integers(0, size, (900, 3))
    pos[:, 1] //= 2  # half the cube stays empty
    for k, p in enumerate(pos):
        c, d = cols[k % len(cols)], int(DG.DATA_VALUES[k % 3])
        e = (vhx.BoxTreeEntry.Visual(c), vhx.BoxTreeEntry.Complex(c, d), vhx.BoxTreeEntry.Informative(d))[k % 3]
        if e.is_some():
            t.insert(tuple(int(v) for v in p), e)
    for p in pos[::7]:
        t.clear(tuple(int(v) for v in p))
    for k, p in enumerate(pos[3::11]):
        t.update(tuple(int(v) for v in p), vhx.BoxTreeEntry.Complex(cols[(k + 1) % len(cols)], 77))
    return t


def tie_tree():
    """A 4^3 / brick_dim 1 tree whose one MIP cell meets colour A twice and colour B twice, A first: "first seen" would
    pick A, the reference's last first-seen group of the highest count picks B."""
    a, b = vhx.Albedo(250, 0, 0, 255), vhx.Albedo(0, 0, 250, 255)
    t = BoxTree(4, 1)
    for p, c in (((0, 0, 0), a), ((0, 0, 1), b), ((1, 0, 0), a), ((1, 0, 1), b)):
        t.insert(p, c)
    return t, a.packed(), b.packed()


def capacity_grid():
    """64,000 distinct random colours in a 64^3 grid: every brick holds some, so the 4,160 MIP cells of the 64 leaves
    and the root average to colours the palette does not hold and push it past 65,535 under BoxFilter."""
    return G.many_colors_grid(64000, 64)
