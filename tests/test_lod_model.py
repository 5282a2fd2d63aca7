"""vhx_flat_lod (FlatTree.lod / TreeImage.lod), the CPU twin of vhx_build_lod, pinned to the host BoxTree route: the
strategy with one method and thresholds of 0 on every level, switch_albedo_mip_maps(True), flatten_lod(d). Every image
is compared in all seven buffers and in node_mips, for both methods and every max_depth from 0 to depth + 1."""
import ctypes

import numpy as np
import pytest

from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import BoxTree, FlatTree
from tests import _compact_model as CM
from tests import _lod_grids as L
from tests import _simplify_grids as SG


def _depths(name):
    return range(0, L.SHAPES[name][2] + 2)


@pytest.mark.parametrize("method", L.METHODS)
@pytest.mark.parametrize("name", list(L.SHAPES))
def test_lod_of_a_dense_build_is_the_host_route(name, method):
    size, bd, depth = L.SHAPES[name]
    g, d = L.pair(name)
    image = FlatTree.from_dense(g, size, bd, data=d)
    kinds = image.voxels[image.voxels != N.VHX_EMPTY]
    if name != "4/1":  # the grid holds what the MIP rules distinguish: data-only voxels beside coloured ones
        assert ((kinds & 0xFFFF) == 0xFFFF).any() and ((kinds & 0xFFFF) != 0xFFFF).any(), name
    want = L.host_lods(BoxTree.from_dense(g, size, bd, data=d), method, _depths(name))
    for dd in _depths(name):
        L.assert_same_lod(image.lod(dd, method), want[dd], f"{name} {method} depth {dd}")
    full = want[depth]
    assert (np.asarray(full.node_mips) != N.VHX_EMPTY).any(), "no MIP was built"
    assert full.node_type.size == image.node_type.size  # at the tree's depth every node stays
    L.assert_same_lod(want[depth + 1], full, "past the depth")
    if depth:
        assert want[0].node_type.size == 1 and (want[0].node_children == N.VHX_EMPTY).all()
        assert want[0].node_ocbits[0] == image.node_ocbits[0]  # the occupancy bits are kept


@pytest.mark.parametrize("method", L.METHODS)
@pytest.mark.parametrize("name", list(L.SHAPES) + ["noise"])
def test_lod_of_a_simplified_image_is_the_host_route(name, method):
    if name == "noise":  # Solid bricks, UniformLeaf nodes over Solid and Parted bricks, no data
        size, bd, depth = 64, 4, 1
        g, d = SG.make_grid("brick_noise", 64, 4), None
        g[:16, :16, :16] = SG.make_grid("blocks4", 16, 4)
        g[16:32, :16, :16] = SG.THREE[1]
    else:
        size, bd, depth = L.SHAPES[name]
        g, d = L.pair(name)
    image = FlatTree.from_dense(g, size, bd, data=d, simplify=True)
    if name == "noise":
        assert (image.node_type == N.VHX_NODE_UNIFORM_LEAF).any() and image.solid_values.size > 1
    tree = BoxTree.from_dense(g, size, bd, data=d)
    tree.simplify()
    want = L.host_lods(tree, method, range(0, depth + 2))
    for dd in range(0, depth + 2):
        L.assert_same_lod(image.lod(dd, method), want[dd], f"simplified {name} {method} depth {dd}")
        L.assert_same_lod(CM.copy_image(image).lod(dd, method), want[dd], f"TreeImage {name} {method} depth {dd}")
    if name == "noise":  # a UniformLeaf has no MIP
        full = want[depth]
        assert (np.asarray(full.node_mips)[full.node_type == N.VHX_NODE_UNIFORM_LEAF] == N.VHX_EMPTY).all()


@pytest.mark.parametrize("method", L.METHODS)
def test_lod_of_an_edited_image_is_the_host_route(method):
    """An insert, clear and update loop (Complex voxels of alpha 0 among them), and the image renumbered into edit
    order with orphaned slots in between: not breadth-first."""
    tree = L.edit_loop_tree()
    flat = tree.flatten()
    vals = flat.voxels[flat.voxels != N.VHX_EMPTY]
    ci, di = vals & 0xFFFF, vals >> 16
    both = (ci != 0xFFFF) & (di != 0xFFFF)
    assert (both & (flat.color_palette[np.minimum(ci, flat.color_palette.size - 1)] >> 24 == 0)).any(), \
        "no Complex voxel of alpha 0"
    edited = CM.scramble(flat, np.random.default_rng(9), junk_nodes=7, junk_bricks=33)
    assert not np.array_equal(edited.node_type[:flat.node_type.size], flat.node_type)
    want = L.host_lods(tree, method, range(0, 4))
    for dd in range(0, 4):
        L.assert_same_lod(flat.lod(dd, method), want[dd], f"edit loop {method} depth {dd}")
        L.assert_same_lod(edited.lod(dd, method), want[dd], f"edit loop, edit order, {method} depth {dd}")


def test_point_filter_tie_goes_to_the_last_first_seen_colour():
    tree, a, b = L.tie_tree()
    flat = tree.flatten()
    assert flat.color_palette.tolist() == [a, b]
    lod = flat.lod(0, "point")
    L.assert_same_lod(lod, L.host_lods(tree, "point", [0])[0], "tie")
    mip = int(lod.node_mips[0])  # brick_dim 1: the MIP brick is one cell, numbered after the root's own bricks
    assert mip == lod.voxels.size - 1
    assert lod.voxels[mip] == 0xFFFF0000 | 1, "the tie must go to B, first seen after A"
    assert lod.color_palette.tolist() == [a, b]  # PointFilter creates no colour
    box = flat.lod(0, "box")
    assert box.color_palette.size == 3 and box.voxels[int(box.node_mips[0])] == 0xFFFF0000 | 2


def test_lod_capacity():
    g = L.capacity_grid()
    image = FlatTree.from_dense(g, 64, 4)
    assert image.color_palette.size == 64000
    tree = BoxTree.from_dense(g, 64, 4)
    L.apply_strategy(tree, "box").switch_albedo_mip_maps(True)
    assert tree.info()["colors"] > 65535, "the host route does not overflow on this grid"
    with pytest.raises(N.VhxError) as e:
        image.lod(1, "box")
    assert e.value.code == N.VHX_E_CAPACITY
    lod = image.lod(1, "point")
    assert np.array_equal(lod.color_palette, image.color_palette)  # no colour added
    assert (np.asarray(lod.node_mips) != N.VHX_EMPTY).all()


def test_lod_refusals():
    image = FlatTree.from_dense(*L.pair("4/1")[:1], 4, 1)
    h = ctypes.c_void_p()
    lib = N.lib()
    for method in (2, 3, 4, 99):  # PointFilterBD, Posterize, PosterizeBD, junk
        assert lib.vhx_flat_lod(ctypes.byref(image.desc), 0, method, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
        assert not h.value
    assert lib.vhx_flat_lod(None, 0, 0, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    assert lib.vhx_flat_lod(ctypes.byref(image.desc), 0, 0, None) == N.VHX_E_INVALID_ARG
    with pytest.raises(ValueError):
        image.lod(0, "posterize")
