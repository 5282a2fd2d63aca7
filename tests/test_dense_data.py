"""The host bulk builder with a data plane (vhx_dense_build_data, vhx_dense_build_tree_data) against the insert loop:
every voxel that has an entry inserted in x-outer, y, z-inner order as Visual, Informative or Complex by the rule of
include/vhx_boxtree.h, then flattened. Every comparison is bit for bit in all seven buffers and the counts."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree
from voxelhex_amd import _native as N
from tests import _dense_data_grids as DG
from tests import _dense_grids as G

EMPTY = N.VHX_EMPTY


@pytest.mark.parametrize("size,bd", DG.SIZES)
@pytest.mark.parametrize("kind", DG.KINDS)
def test_builder_equals_the_insert_loop(kind, size, bd):
    g, d = DG.make_pair(kind, size)
    got = FlatTree.from_dense(g, size, bd, data=d)
    G.assert_same_image(got, DG.insert_loop(g, d, size, bd), f"{kind} {size}/{bd}")
    if kind == "sparse" and size >= 16:  # all four kinds of voxel occur
        has_c, has_d = (g >> 24 != 0), d != 0
        for a in (True, False):
            for b in (True, False):
                assert ((has_c == a) & (has_d == b)).any()
        assert got.desc.data_count == len(DG.DATA_VALUES)
        halves = {(int(v) & 0xFFFF == 0xFFFF, int(v) >> 16 == 0xFFFF) for v in np.unique(got.voxels)}
        assert halves >= {(False, True), (True, False), (False, False)}  # Visual, Informative, Complex


@pytest.mark.parametrize("size,bd", [(16, 4), (32, 2), (16, 1)])
def test_host_tree_equals_the_insert_loop(size, bd):
    g, d = DG.make_pair("sparse", size, seed=2)
    tree = BoxTree.from_dense(g, size, bd, data=d)
    G.assert_same_image(tree.flatten(), DG.insert_loop(g, d, size, bd), f"{size}/{bd}")
    x, y, z = np.argwhere((g >> 24 != 0) & (d != 0))[0][::-1]
    e = tree.get((int(x), int(y), int(z)))
    assert e.kind == "Complex" and e.data() == int(d[z, y, x]) and e.albedo().packed() == int(g[z, y, x])


def test_each_palette_is_in_first_appearance_order_of_the_insert_loop():
    a, b = 1234, 0x80000001
    d = np.zeros((4, 4, 4), np.uint32)
    d[0, 0, 1] = a  # (x, y, z) = (1, 0, 0): memory order meets A first
    d[1, 0, 0] = b  # (x, y, z) = (0, 0, 1): the insert loop B
    g = np.zeros_like(d)
    for size, bd in ((4, 1), (16, 4)):
        f = FlatTree.from_dense(g, size, bd, data=d)
        assert f.data_palette.tolist() == [b, a] and f.color_palette.size == 0
        G.assert_same_image(f, DG.insert_loop(g, d, size, bd), "data order")
    # the two palettes ordered oppositely in one grid: the colours A' at (0, 0, 1), B' at (1, 0, 0)
    g, order = G.palette_order_grid()  # colours: [b', a'] with a' at (1, 0, 0)
    d2 = np.zeros_like(d)
    d2[0, 0, 1] = b  # beside colour a', which is second in its palette, the data value that is first in its own
    d2[1, 0, 0] = a
    f = FlatTree.from_dense(g, 4, 1, data=d2)
    assert f.color_palette.tolist() == [int(c) for c in order] and f.data_palette.tolist() == [a, b]
    G.assert_same_image(f, DG.insert_loop(g, d2, 4, 1), "opposite orders")
    assert sorted(int(v) for v in f.voxels if v != EMPTY) == [0 | (0 << 16), 1 | (1 << 16)]


@pytest.mark.parametrize("size,bd", [(16, 1), (64, 4)])
def test_a_data_only_voxel_creates_its_node_chain_and_brick(size, bd):
    g = np.zeros((size, size, size), np.uint32)
    d = np.zeros_like(g)
    d[-1, -1, -1] = 77
    f = FlatTree.from_dense(g, size, bd, data=d)
    G.assert_same_image(f, DG.insert_loop(g, d, size, bd), "far corner")
    levels = {16: 2, 64: 2}[size]
    assert f.desc.node_count == levels and f.desc.brick_count == 1 and f.desc.color_count == 0
    assert f.node_type.tolist() == [N.VHX_NODE_INTERNAL] * (levels - 1) + [N.VHX_NODE_LEAF]
    assert (f.node_ocbits == np.uint64(1 << 63)).all()
    assert f.voxels[-1] == (0xFFFF | (0 << 16)) and (f.voxels[:-1] == EMPTY).all()


def test_a_transparent_colour_beside_data_is_informative():
    g = np.zeros((4, 4, 4), np.uint32)
    d = np.zeros_like(g)
    g[1, 2, 3] = G.rgba(9, 9, 9, 0)
    d[1, 2, 3] = 5
    g[0, 0, 0] = G.rgba(9, 9, 9, 0)  # and one without data: no entry at all
    f = FlatTree.from_dense(g, 4, 1, data=d)
    assert f.color_palette.size == 0 and f.data_palette.tolist() == [5] and f.desc.brick_count == 1
    assert f.voxels.tolist() == [0xFFFF]
    G.assert_same_image(f, DG.insert_loop(g, d, 4, 1), "transparent beside data")
    # the host tree, handed the same voxel as Complex, would put the colour into the palette
    t = BoxTree(4, 1)
    t.insert((3, 2, 1), vhx.BoxTreeEntry.Complex(vhx.Albedo.from_packed(int(g[1, 2, 3])), 5))
    assert t.flatten().color_palette.size == 1


def test_simplified_bricks():
    size, bd = 16, 4
    c = G.rgba(1, 2, 3)
    g = np.zeros((size, size, size), np.uint32)
    d = np.zeros_like(g)
    g[:4, :4, :4] = c  # brick 0 of leaf 0: one (c, d) throughout
    d[:4, :4, :4] = 9
    g[:4, :4, 4:8] = c  # brick 1: one colour, two data values
    d[:4, :4, 4:8] = 9
    d[0, 0, 4] = 7
    f = FlatTree.from_dense(g, size, bd, simplify=True, data=d)
    assert f.color_palette.tolist() == [int(c)] and f.data_palette.tolist() == [9, 7]
    assert f.node_type.tolist() == [N.VHX_NODE_LEAF]  # the root is the leaf
    e0, e1 = (int(v) for v in f.node_children[:2])
    assert e0 & N.VHX_SOLID_BIT and f.solid_values[e0 & 0x7FFFFFFF] == (0 | (0 << 16)), "Solid ci | di << 16"
    assert e1 != EMPTY and not (e1 & N.VHX_SOLID_BIT), "mixed data stays Parted"
    assert f.desc.brick_count == 1 and f.desc.solid_count == 1
    assert sorted(np.unique(f.voxels).tolist()) == [0 | (0 << 16), 0 | (1 << 16)]


@pytest.mark.parametrize("size,bd", [(16, 4), (32, 2), (64, 4), (16, 1)])
@pytest.mark.parametrize("kind", ["sparse", "full"])
def test_simplified_equals_the_host_tree_simplified(kind, size, bd):
    g, d = DG.make_pair(kind, size, seed=1)
    if kind == "full":  # whole leaves of one value, and a region where only the data differs
        d[:] = 7
        d[: size // 2, : size // 4] = 9
    tree = BoxTree.from_dense(g, size, bd, data=d)
    tree.simplify(True)
    got = FlatTree.from_dense(g, size, bd, simplify=True, data=d)
    G.assert_same_image(got, tree.flatten(), f"{kind} {size}/{bd}")
    if kind == "full":
        assert (got.node_type == N.VHX_NODE_UNIFORM_LEAF).any() and got.desc.data_count == 2


def test_data_capacity():
    g, d = DG.distinct_data_grid(65535)
    f = FlatTree.from_dense(g, 64, 4, data=d)
    assert f.desc.data_count == 65535 and f.desc.color_count == 1
    # first-appearance order of the insert loop, not of memory
    gz, gy, gx = d.shape
    z, y, x = np.nonzero(d)
    first = (x.astype(np.int64) * gy + y) * gz + z
    assert np.array_equal(f.data_palette, d[z, y, x][np.argsort(first)])
    g, d = DG.distinct_data_grid(65536)
    for simplify in (False, True):
        with pytest.raises(N.VhxError) as e:
            FlatTree.from_dense(g, 64, 4, simplify=simplify, data=d)
        assert e.value.code == N.VHX_E_CAPACITY
    with pytest.raises(N.VhxError) as e:
        BoxTree.from_dense(g, 64, 4, data=d)
    assert e.value.code == N.VHX_E_CAPACITY


@pytest.mark.parametrize("simplify", [False, True])
def test_no_data_is_the_colour_only_image(simplify):
    for size, bd in ((16, 4), (32, 2)):
        g = G.make_grid("sparse", size)
        want = FlatTree.from_dense(g, size, bd, simplify=simplify)
        G.assert_same_image(FlatTree.from_dense(g, size, bd, simplify=simplify, data=None), want, "data=None")
        G.assert_same_image(FlatTree.from_dense(g, size, bd, simplify=simplify, data=np.zeros_like(g)), want, "zeros")
        assert want.data_palette.size == 0


def test_a_wrong_data_plane_is_refused():
    g = G.make_grid("sparse", 16)
    with pytest.raises(TypeError):
        FlatTree.from_dense(g, 16, 4, data=np.zeros(g.shape, np.int32))
    with pytest.raises(TypeError):
        FlatTree.from_dense(g, 16, 4, data=np.zeros((1,) + g.shape[1:], np.uint32))
