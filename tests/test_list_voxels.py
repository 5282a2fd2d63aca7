"""vhx_flat_list_voxels, the host twin of vhx_list_voxels: the occupied voxels of a box of a flattened image as a list.
The expected lists come from the numpy model (tests/_list_model.py: the key formula) over the planes that the walker of
tests/_flatget.py reads from the same image. Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

from voxelhex_amd import FlatTree, TreeImage
from voxelhex_amd import _native as N
from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._list_model import expected_box

SENTINEL = 0xDEADBEEF
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def planes(image):
    """(albedo, data) planes of the whole root cube, shape (size,) * 3, as read_dense(data=True) defines them."""
    size = int(image.boxtree_size)
    v = F.flat_get(image, cached(("lattice", size), lambda: F.lattice((0, 0, 0), (size,) * 3)))
    return F.flat_albedo(image, v).reshape((size,) * 3), DG.flat_data(image, v).reshape((size,) * 3)


def images(kind, size, bd):
    """(plain image, simplified image, albedo plane, data plane) of a grid with data."""
    def make():
        g, d = DG.make_pair(kind, size)
        plain = FlatTree.from_dense(g, size, bd, data=d)
        vis, dat = planes(plain)
        return plain, plain.simplified(), vis, dat
    return cached(("images", kind, size, bd), make)


def boxes(size, bd, vis, dat):
    """(name, origin, extents): the whole cube, single voxels, a box inside one brick, boxes off every brick boundary."""
    out = [("cube", (0, 0, 0), (size,) * 3)]
    some = (vis != 0) | (dat != 0)
    hit = np.argwhere(some)
    if hit.size:
        z, y, x = (int(v) for v in hit[hit.shape[0] // 2])
        out.append(("occupied voxel", (x, y, z), (1, 1, 1)))
        b0 = tuple(v // bd * bd for v in (x, y, z))
        inset, edge = (1, bd - 2) if bd >= 4 else (0, bd)
        out.append(("inside one brick", tuple(v + inset for v in b0), (edge,) * 3))
    miss = np.argwhere(~some)
    if miss.size:
        z, y, x = (int(v) for v in miss[miss.shape[0] // 3])
        out.append(("empty voxel", (x, y, z), (1, 1, 1)))
    o = tuple(min(v, size - 1) for v in (3, 5, 1))
    out.append(("odd", o, tuple(min(e, size - v) for e, v in zip(G.odd_extents(size), o))))
    if size > 2:  # every face cuts the bricks, Solid bricks and UniformLeaf nodes at the cube's surface
        out.append(("cut", (1, 1, 1), (size - 2, size - 3 if size > 3 else 1, size - 2)))
    return out


def assert_lists(got, want, what):
    for name, a, b in zip(("positions", "albedo", "data"), got, want):
        assert a.dtype == np.uint32 and a.shape == b.shape, f"{what}: {name} {a.shape} != {b.shape}"
        assert np.array_equal(a, b), f"{what}: {name} differs at {np.flatnonzero((a != b).reshape(len(a), -1).any(1))[:4]}"


@pytest.mark.parametrize("kind", DG.KINDS)
@pytest.mark.parametrize("size,bd", DG.SIZES)
def test_lists_of_dense_images(kind, size, bd):
    plain, simple, vis, dat = images(kind, size, bd)
    svis, sdat = planes(simple)
    assert np.array_equal(svis, vis) and np.array_equal(sdat, dat)
    for name, origin, extents in boxes(size, bd, vis, dat):
        what = f"{kind} {size}/{bd} {name}"
        want = expected_box(vis, dat, size, bd, origin, extents)
        a = plain.list_voxels(origin, extents)
        b = simple.list_voxels(origin, extents)
        assert_lists(a, want, what + " (plain)")
        assert_lists(b, want, what + " (simplified)")
        assert plain.count_voxels(origin, extents) == simple.count_voxels(origin, extents) == len(want[0]), what


@pytest.mark.parametrize("kind", ["full", "brick_noise", "blocks4", "cut", "corner"])
@pytest.mark.parametrize("size,bd", [(16, 1), (16, 4), (32, 2), (64, 4), (32, 8)])
def test_lists_of_solid_bricks_and_uniform_leaves(kind, size, bd):
    """Grids whose simplified image holds Solid bricks and both kinds of UniformLeaf (tests/_simplify_grids.py)."""
    g = SG.make_grid(kind, size, bd)
    plain = FlatTree.from_dense(g, size, bd)
    simple = plain.simplified()
    SG.assert_case(kind, size, bd, simple)
    vis, dat = planes(plain)
    for name, origin, extents in boxes(size, bd, vis, dat):
        what = f"{kind} {size}/{bd} {name}"
        want = expected_box(vis, dat, size, bd, origin, extents)
        assert_lists(plain.list_voxels(origin, extents), want, what + " (plain)")
        assert_lists(simple.list_voxels(origin, extents), want, what + " (simplified)")


def raw_list(image, origin, extents, capacity, fields=(True, True, True), slack=4):
    """vhx_flat_list_voxels through the C ABI into sentinel-filled arrays: (rc, count, positions, albedo, data)."""
    n = ctypes.c_uint64(SENTINEL)
    room = capacity + slack
    arrays = [np.full((room, 3), SENTINEL, np.uint32), np.full(room, SENTINEL, np.uint32),
              np.full(room, SENTINEL, np.uint32)]
    q = N.PointsOut(*origin, *extents, capacity, *(a.ctypes.data if on else None for a, on in zip(arrays, fields)),
                    ctypes.pointer(n))
    rc = N.lib().vhx_flat_list_voxels(ctypes.byref(image.desc), ctypes.byref(q))
    return (rc, n.value, *arrays)


@pytest.mark.parametrize("which", ["plain", "simplified"])
def test_capacity_and_null_fields(which):
    size, bd = 32, 2
    plain, simple, vis, dat = images("sparse", size, bd)
    image = plain if which == "plain" else simple
    origin, extents = (3, 5, 1), (20, 11, 30)
    want = expected_box(vis, dat, size, bd, origin, extents)
    count = len(want[0])
    assert count > 8
    for capacity in (0, count - 1, count, count + 5):
        rc, n, *arrays = raw_list(image, origin, extents, capacity, slack=8)
        assert rc == N.VHX_OK and n == count, capacity
        k = min(count, capacity)
        for a, w in zip(arrays, want):
            assert np.array_equal(a[:k], w[:k]), capacity  # the prefix of the full list
            assert (a[k:] == SENTINEL).all(), capacity     # nothing past it is written
        pos, alb, da, total = image.list_voxels(origin, extents, capacity=capacity)
        assert total == count and len(pos) == len(alb) == len(da) == k and np.array_equal(pos, want[0][:k])
    for fields in ((True, False, False), (False, True, False), (False, False, True), (True, False, True),
                   (False, False, False)):
        rc, n, *arrays = raw_list(image, origin, extents, count, fields)
        assert rc == N.VHX_OK and n == count, fields
        for a, w, on in zip(arrays, want, fields):
            assert np.array_equal(a[:count], w) if on else (a == SENTINEL).all(), fields


def hand_image(size, bd, types, children, solids=(), colors=(G.rgba(9, 8, 7),)):
    return TreeImage(size, bd, dict(node_type=np.array(types, np.uint32), node_ocbits=np.zeros(len(types), np.uint64),
                                    node_children=np.array(children, np.uint32).reshape(-1),
                                    voxels=np.zeros(0, np.uint32), solid_values=np.array(solids, np.uint32),
                                    color_palette=np.array(colors, np.uint32), data_palette=np.zeros(0, np.uint32)))


def stretched_image():
    """A root UniformLeaf over a Solid brick, 64 wide at brick_dim 4: a brick stretched over a cube larger than a leaf."""
    entries = np.full(64, N.VHX_EMPTY, np.uint32)
    entries[0] = N.VHX_SOLID_BIT | 0
    return hand_image(64, 4, [N.VHX_NODE_UNIFORM_LEAF], entries, solids=[0xFFFF0000])


def wide_image():
    """A 2^24-wide image of one empty Internal root."""
    return hand_image(1 << 24, 4, [N.VHX_NODE_INTERNAL], np.full(64, N.VHX_EMPTY, np.uint32))


def test_refusals_write_nothing():
    assert ctypes.sizeof(N.PointsOut) == 64  # vhx_points_out: six u32, a u64 and four pointers
    plain = images("sparse", 16, 4)[0]

    def refused(image, origin, extents, code, what):
        rc, n, *arrays = raw_list(image, origin, extents, 16)
        assert rc == code, what
        assert n == SENTINEL and all((a == SENTINEL).all() for a in arrays), what

    refused(plain, (0, 0, 0), (0, 4, 4), N.VHX_E_INVALID_ARG, "an empty box")
    refused(plain, (0, 0, 0), (4, 4, 0), N.VHX_E_INVALID_ARG, "an empty box")
    refused(plain, (13, 0, 0), (4, 4, 4), N.VHX_E_INVALID_ARG, "a box outside the cube")
    refused(plain, (0, 0, 16), (1, 1, 1), N.VHX_E_INVALID_ARG, "a box outside the cube")
    refused(plain, (0, 0xFFFFFFFF, 0), (1, 2, 1), N.VHX_E_INVALID_ARG, "a box that wraps")
    refused(stretched_image(), (0, 0, 0), (64, 64, 64), N.VHX_E_STATE, "a stretched brick")
    refused(stretched_image(), (5, 5, 5), (1, 1, 1), N.VHX_E_STATE, "a stretched brick under one voxel")
    refused(wide_image(), (0, 0, 0), (1 << 24,) * 3, N.VHX_E_CAPACITY, "2^72 voxels")
    refused(wide_image(), (0, 0, 0), (1 << 24, 1 << 24, 1), N.VHX_E_CAPACITY, "2^48 voxels")
    rc, n, *_ = raw_list(wide_image(), (0, 0, 0), (1 << 24, (1 << 24) - 1, 1), 0)  # 2^48 - 2^24 voxels of nothing
    assert rc == N.VHX_OK and n == 0
    q = N.PointsOut(0, 0, 0, 1, 1, 1, 0, None, None, None, None)
    assert N.lib().vhx_flat_list_voxels(ctypes.byref(plain.desc), ctypes.byref(q)) == N.VHX_E_INVALID_ARG  # null count
    assert N.lib().vhx_flat_list_voxels(ctypes.byref(plain.desc), None) == N.VHX_E_INVALID_ARG
    assert N.lib().vhx_flat_list_voxels(None, ctypes.byref(q)) == N.VHX_E_INVALID_ARG


def test_a_lod_cut_view_is_listed_as_it_reads():
    from tests.test_gpu_dense_write import lod_tree
    size = 64
    view = lod_tree(size).flatten_lod(0)
    vis, dat = planes(view)
    for origin, extents in (((0, 0, 0), (size,) * 3), ((3, 5, 1), (40, 33, 60))):
        want = expected_box(vis, dat, size, 4, origin, extents)
        assert_lists(view.list_voxels(origin, extents), want, f"flatten_lod(0) {origin}")
        assert view.count_voxels(origin, extents) == len(want[0])
