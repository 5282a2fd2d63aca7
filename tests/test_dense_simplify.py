"""vhx_dense_build_simplified (FlatTree.from_dense(simplify=True)): the simplified image of a dense grid is the dense
tree simplified recursively and flattened, which at small sizes is the voxel-by-voxel insert loop simplified; the plain
image does not change. Every grid is first checked to hold the case it is named for (tests/_simplify_grids.py)."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _simplify_grids as S


def simplified_tree(grid, size, bd):
    t = BoxTree.from_dense(grid, size, bd)
    t.simplify(True)
    return t.flatten()


def simplified_insert_loop(grid, size, bd):
    t = vhx.BoxTree(size, bd)
    gz, gy, gx = grid.shape
    for x in range(gx):
        for y in range(gy):
            col = grid[:, y, x]
            for z in np.flatnonzero(col >> 24):
                t.insert((x, y, int(z)), vhx.Albedo.from_packed(int(col[z])))
    t.simplify(True)
    return t.flatten()


@pytest.mark.parametrize("size,bd", S.SIZES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_simplified_image_equals_simplified_tree(kind, size, bd):
    grid = S.make_grid(kind, size, bd)
    got = FlatTree.from_dense(grid, size, bd, threads=4, simplify=True)
    S.assert_case(kind, size, bd, got)
    G.assert_same_image(got, simplified_tree(grid, size, bd), f"{kind} {size}/{bd}")
    if size <= 32:
        G.assert_same_image(got, simplified_insert_loop(grid, size, bd), f"{kind} {size}/{bd} insert loop")


@pytest.mark.parametrize("size,bd", S.SIZES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_simplification_keeps_nodes_occupancy_and_palette(kind, size, bd):
    grid = S.make_grid(kind, size, bd)
    plain, simple = FlatTree.from_dense(grid, size, bd), FlatTree.from_dense(grid, size, bd, simplify=True)
    assert np.array_equal(plain.node_ocbits, simple.node_ocbits)
    assert np.array_equal(plain.color_palette, simple.color_palette) and simple.data_palette.size == 0
    inner = plain.node_type != N.VHX_NODE_LEAF
    assert np.array_equal(plain.node_type[inner], simple.node_type[inner])
    assert np.array_equal(plain.node_children.reshape(-1, 64)[inner], simple.node_children.reshape(-1, 64)[inner])
    assert np.isin(simple.node_type[~inner], (N.VHX_NODE_LEAF, N.VHX_NODE_UNIFORM_LEAF)).all()


def test_solid_values_follow_the_leaf_walk_not_the_palette():
    grid, a, b = S.solid_order_grid()
    f = FlatTree.from_dense(grid, 64, 4, simplify=True)
    assert f.color_palette.tolist() == [int(b), int(a)]
    assert f.solid_values.tolist() == [0xFFFF0000 | 1, 0xFFFF0000 | 0]  # A's value, then B's
    assert f.desc.brick_count == 0 and (f.node_type == N.VHX_NODE_UNIFORM_LEAF).sum() == 2
    G.assert_same_image(f, simplified_tree(grid, 64, 4), "solid order")


def test_unsimplified_image_is_unchanged():
    for kind, size, bd in (("brick_noise", 64, 4), ("blocks4", 32, 2), ("full", 16, 1)):
        grid = S.make_grid(kind, size, bd)
        plain = FlatTree.from_dense(grid, size, bd, simplify=False)
        G.assert_same_image(plain, FlatTree.from_dense(grid, size, bd), f"{kind} default")
        G.assert_same_image(plain, BoxTree.from_dense(grid, size, bd).flatten(), f"{kind} tree")
        assert plain.solid_values.size == 0 and not (plain.node_type == N.VHX_NODE_UNIFORM_LEAF).any()


def test_errors():
    import ctypes
    h = ctypes.c_void_p()
    d = N.DenseDesc(16, 1, 4, 4, 4, 0, None)
    assert N.lib().vhx_dense_build_simplified(ctypes.byref(d), 0, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    assert N.lib().vhx_dense_build_simplified(None, 0, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    with pytest.raises(N.VhxError) as e:
        FlatTree.from_dense(np.zeros((4, 4, 17), np.uint32), 16, 1, simplify=True)
    assert e.value.code == N.VHX_E_INVALID_ARG
    with pytest.raises(vhx.OctreeError):
        FlatTree.from_dense(np.zeros((4, 4, 4), np.uint32), 256, 8, simplify=True)
