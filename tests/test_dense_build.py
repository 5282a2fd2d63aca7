"""The bulk builder for a caller's dense grid (vhx_dense_build) writes exactly the flattened tree that inserting the
grid's voxels one by one (x outer, y, z inner) and flattening gives -- for arbitrary grids, not only the procedural
scenes of tests/test_scene_builder.py."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G


@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_dense_equals_insert_loop(kind, size, bd):
    grid = G.make_grid(kind, size)
    G.assert_same_image(FlatTree.from_dense(grid, size, bd, threads=4), G.insert_loop(grid, size, bd),
                        f"{kind} {size}/{bd}")


def test_structure_of_the_corner_cases():
    f = FlatTree.from_dense(G.make_grid("zero", 16), 16, 1)
    assert f.node_type.tolist() == [N.VHX_NODE_NOTHING] and f.voxels.size == 0 and f.color_palette.size == 0
    f = FlatTree.from_dense(G.make_grid("full", 64), 64, 4)  # one colour everywhere: still Parted bricks in Leaf nodes
    assert f.solid_values.size == 0 and set(np.unique(f.node_type)) == {N.VHX_NODE_INTERNAL, N.VHX_NODE_LEAF}
    assert f.desc.brick_count == 16 ** 3 and f.color_palette.tolist() == [int(G.rgba(10, 20, 30))]
    f = FlatTree.from_dense(G.make_grid("sparse", 32), 32, 2)
    assert int(G.COLORS[3]) not in f.color_palette.tolist() and f.color_palette.size == 4  # alpha 0: no voxel


def test_palette_is_in_insert_order_not_memory_order():
    grid, want = G.palette_order_grid()
    f = FlatTree.from_dense(grid, 4, 1)
    assert f.color_palette.tolist() == [int(c) for c in want]
    G.assert_same_image(f, G.insert_loop(grid, 4, 1), "palette order")


def test_many_colours_equal_insert_loop():
    grid = G.many_colors_grid()
    f = FlatTree.from_dense(grid, 64, 4, threads=3)
    assert f.color_palette.size == 5000
    G.assert_same_image(f, G.insert_loop(grid, 64, 4), "5000 colours")


def test_scene_read_back_as_grid_builds_the_scene_image():
    size, bd = 64, 4
    t = BoxTree.from_scene(N.VHX_SCENE_LATTICE_CUBE, size, bd)
    grid = np.zeros((size, size, size), np.uint32)
    for x in range(size):
        for y in range(size):
            for z in range(size):
                e = t.get((x, y, z))
                if e.is_some():
                    grid[z, y, x] = e.albedo().packed()
    G.assert_same_image(FlatTree.from_dense(grid, size, bd), FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, size, bd),
                        "lattice cube")


def test_boxtree_from_dense_is_a_working_tree():
    size, bd = 32, 2
    grid = G.make_grid("sparse", size)
    t = BoxTree.from_dense(grid, size, bd)
    G.assert_same_image(t.flatten(), FlatTree.from_dense(grid, size, bd), "tree of the image")
    gz, gy, gx = grid.shape
    rng = np.random.default_rng(1)
    for x, y, z in zip(rng.integers(0, gx, 200), rng.integers(0, gy, 200), rng.integers(0, gz, 200)):
        c = int(grid[z, y, x])
        want = vhx.BoxTreeEntry.Visual(vhx.Albedo.from_packed(c)) if c >> 24 else vhx.BoxTreeEntry.Empty()
        assert t.get((int(x), int(y), int(z))) == want
    assert t.get((size - 1, size - 1, 0)) == vhx.BoxTreeEntry.Empty()  # beyond the extents
    t.insert((size - 1, size - 1, 0), vhx.Albedo(5, 6, 7, 255))
    assert t.get((size - 1, size - 1, 0)) == vhx.BoxTreeEntry.Visual(vhx.Albedo(5, 6, 7, 255))
    full = np.zeros((size, size, size), np.uint32)
    full[:gz, :gy, :gx] = grid
    full[0, size - 1, size - 1] = vhx.Albedo(5, 6, 7, 255).packed()
    G.assert_same_image(t.flatten(), G.insert_loop(full, size, bd), "insert after the bulk build")


def test_errors():
    grid = np.zeros((4, 4, 4), np.uint32)
    with pytest.raises(Exception) as new:
        BoxTree(256, 8)
    with pytest.raises(type(new.value)):
        FlatTree.from_dense(grid, 256, 8)
    with pytest.raises(type(new.value)):
        BoxTree.from_dense(grid, 256, 8)
    for shape in [(4, 4, 0), (0, 4, 4), (4, 4, 17), (17, 4, 4), (4, 17, 4)]:
        with pytest.raises(N.VhxError) as e:
            FlatTree.from_dense(np.zeros(shape, np.uint32), 16, 1)
        assert e.value.code == N.VHX_E_INVALID_ARG, shape
    d = N.DenseDesc(16, 1, 4, 4, 4, 0, None)
    import ctypes
    h = ctypes.c_void_p()
    assert N.lib().vhx_dense_build(ctypes.byref(d), 0, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    assert N.lib().vhx_dense_build(None, 0, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    with pytest.raises(TypeError):
        FlatTree.from_dense(np.zeros((4, 4, 4), np.int64), 16, 1)


def test_palette_capacity():
    with pytest.raises(N.VhxError) as e:
        FlatTree.from_dense(G.distinct_colors_grid(65600), 64, 4)
    assert e.value.code == N.VHX_E_CAPACITY
    f = FlatTree.from_dense(G.distinct_colors_grid(65535), 64, 4)
    assert f.color_palette.size == 65535
    assert int(f.voxels.max()) == N.VHX_EMPTY and int(f.voxels[f.voxels != N.VHX_EMPTY].max()) == 0xFFFF0000 | 65534
