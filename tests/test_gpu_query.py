"""vhx_get_voxels and vhx_read_dense on the GPU, bit for bit against tests/_flatget.py (the numpy restatement of
BoxTree::get over the image the device holds, itself pinned against the host tree in tests/test_flatget.py), against
BoxTree.get on samples, and, for trees built from a dense grid, against the grid itself."""
import ctypes
import os

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree, TreeImage
from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import entry_from_value
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._arraytree import ArrayTree
from tests.test_flatget import mixed_tree, sample

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
GINGERBREAD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gingerbread_bd8.npz")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def visible(grid, size):
    """What read_dense of build_dense(grid) gives for the whole cube: alpha-0 entries zeroed, zero-extended."""
    out = np.zeros((size, size, size), np.uint32)
    gz, gy, gx = grid.shape
    out[:gz, :gy, :gx] = np.where(grid >> 24 != 0, grid, 0)
    return out


def grid_256():
    """The grid of tests/test_gpu_dense_build.py::test_device_build_at_256."""
    rng = np.random.default_rng(256)
    grid = np.zeros((256, 256, 256), np.uint32)
    mask = rng.random(grid.shape) < 1 / 40
    grid[mask] = G.COLORS[rng.integers(0, len(G.COLORS), int(mask.sum()))]
    grid[:, :, 100:200] = 0
    grid[64:128] = 0
    grid[:, 129:] = 0
    return grid


def assert_get_everywhere(rt, image, what):
    """get over every position of the cube equals the walker; returns (positions, values)."""
    size = image.boxtree_size
    pos = cached(("lattice", size), lambda: F.lattice((0, 0, 0), (size,) * 3))
    want = F.flat_get(image, pos)
    got = rt.get(pos)
    assert got.dtype == np.uint32 and np.array_equal(got, want), \
        f"{what}: get differs at {pos[np.flatnonzero(got != want)[:4]].tolist()}"
    return pos, want


def assert_get_matches_tree(rt, tree, seed, what):
    flat = tree.flatten()
    pos = sample(flat.boxtree_size, seed)
    for p, v in zip(pos.tolist(), rt.get(pos)):
        assert entry_from_value(v, flat.color_palette, flat.data_palette) == tree.get(p), f"{what}: {p}"


# ------------------------------------------------------------------------------------------------ every position
@pytest.mark.parametrize("simplify", [False, True], ids=["plain", "simplified"])
@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_get_at_every_position_of_a_built_tree(gpu, kind, size, bd, simplify):
    what = f"{kind} {size}/{bd} simplify={simplify}"
    gpu.build_dense(G.make_grid(kind, size), size, bd, simplify=simplify)
    img = gpu.download()
    pos, want = assert_get_everywhere(gpu, img, what)
    assert (want != EMPTY).any() == (kind != "zero"), what
    outside = np.array([(size, 0, 0), (0, size, 0), (0, 0, 0xFFFFFFFF)], np.uint32)
    assert gpu.get(outside).tolist() == [EMPTY] * 3, what
    pick = np.random.default_rng(size + bd).integers(0, len(pos), len(pos))  # a permutation with duplicates
    assert np.array_equal(gpu.get(pos[pick]), want[pick]), f"{what}: permuted"
    got = gpu.get(to_device(np.concatenate([pos[pick], outside])))
    assert got.is_cuda and np.array_equal(to_host(got), np.concatenate([want[pick], [EMPTY] * 3])), f"{what}: tensor"


# ------------------------------------------------------------------------------------------- uploaded host trees
@pytest.mark.parametrize("simplified", [False, True], ids=["mixed", "mixed-simplified"])
def test_get_on_a_host_tree_with_data_entries(gpu, simplified):
    tree = mixed_tree()
    if simplified:
        tree.simplify()
    flat = tree.flatten()
    if simplified:
        uni = flat.node_children.reshape(-1, 64)[flat.node_type == N.VHX_NODE_UNIFORM_LEAF][:, 0]
        assert flat.solid_values.size and ((uni & N.VHX_SOLID_BIT) != 0).any() and ((uni & N.VHX_SOLID_BIT) == 0).any(), \
            "Solid bricks and both UniformLeaf forms"
    gpu.upload(flat)
    _, want = assert_get_everywhere(gpu, flat, "mixed tree")
    some = want[want != EMPTY]
    assert ((some >> 16) != 0xFFFF).any() and ((some & 0xFFFF) == 0xFFFF).any(), "Complex and Informative values"
    assert_get_matches_tree(gpu, tree, 11, "mixed tree")
    whole = gpu.read_dense()
    assert np.array_equal(whole.ravel(), F.flat_albedo(flat, want)), "read_dense of the mixed tree"


@pytest.mark.parametrize("size,bd", SG.SIZES)
@pytest.mark.parametrize("kind", SG.KINDS)
def test_get_on_simplified_host_images(gpu, kind, size, bd):
    what = f"{kind} {size}/{bd}"
    grid = SG.make_grid(kind, size, bd)
    flat = FlatTree.from_dense(grid, size, bd, simplify=True)
    gpu.upload(flat)
    _, want = assert_get_everywhere(gpu, flat, what)
    tree = BoxTree.from_dense(grid, size, bd)
    tree.simplify()
    assert_get_matches_tree(gpu, tree, size + bd, what)
    assert np.array_equal(gpu.read_dense(), visible(grid, size)), f"{what}: read_dense"
    assert np.array_equal(gpu.read_dense().ravel(), F.flat_albedo(flat, want)), f"{what}: read_dense against the walker"


# -------------------------------------------------------------------------------------------- the raw-value quirk
def quirk_image(root_type):
    """Size 16, brick_dim 4: one Parted brick whose cells alternate between an opaque colour and a value whose colour has
    alpha 0 -- the one brick of a UniformLeaf root (stretched over the cube), or sectant 0 of a Leaf root."""
    voxels = np.where(np.arange(64) % 3 == 0, 0xFFFF0001, 0xFFFF0000).astype(np.uint32)
    children = np.full(64, EMPTY, np.uint32)
    children[0] = 0
    return TreeImage(16, 4, dict(node_type=np.array([root_type], np.uint32),
                                 node_ocbits=np.array([1 if root_type == N.VHX_NODE_LEAF else 2 ** 64 - 1], np.uint64),
                                 node_children=children, voxels=voxels, solid_values=np.zeros(0, np.uint32),
                                 color_palette=np.array([G.rgba(200, 30, 30), G.rgba(9, 9, 9, 0)], np.uint32),
                                 data_palette=np.zeros(0, np.uint32)))


@pytest.mark.parametrize("root", ["uniform", "leaf"])
def test_transparent_value_is_raw_in_a_uniform_leaf_and_empty_in_a_leaf(gpu, root):
    img = quirk_image(N.VHX_NODE_UNIFORM_LEAF if root == "uniform" else N.VHX_NODE_LEAF)
    gpu.upload(img)
    pos, want = assert_get_everywhere(gpu, img, root)
    got = gpu.get(pos)
    if root == "uniform":  # cell (x / 4, y / 4, z / 4); cell 0 holds the transparent value
        assert got[0] == 0xFFFF0001 and set(got.tolist()) == {0xFFFF0000, 0xFFFF0001}
        assert (got == 0xFFFF0001).sum() == 22 * 64
    else:  # the brick spans [0, 4)^3; its transparent cells read as empty, like everything outside it
        assert got[0] == EMPTY and set(got.tolist()) == {0xFFFF0000, EMPTY}
        assert (got == 0xFFFF0000).sum() == 64 - 22
    dense = gpu.read_dense()
    assert np.array_equal(dense.ravel(), np.where(want == 0xFFFF0000, G.rgba(200, 30, 30), 0))
    assert dense[0, 0, 0] == 0


# ---------------------------------------------------------------------------------------------------- LOD-cut view
def lod_tree(size):
    tree = BoxTree(size, 4)
    tree.insert_scene(N.VHX_SCENE_LATTICE_CUBE)
    tree.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
    return tree


@pytest.mark.parametrize("size,depth", [(64, 1), (64, 0), (256, 1)])
def test_positions_under_a_lod_cut_are_empty_with_and_without_mips(gpu, size, depth):
    """A 64 / 4 tree has two node levels, so flatten_lod(1) keeps all of it and flatten_lod(0) only the root; a 256 / 4
    tree cut at depth 1 keeps the root and its children and leaves the leaves out."""
    tree = cached(("lod", size), lambda: lod_tree(size))
    full, cut = tree.flatten(), tree.flatten_lod(depth)
    pos = F.lattice((0, 0, 0), (64,) * 3) if size == 64 else F.seeded_positions(size, 200000, 3)
    want_full, want = F.flat_get(full, pos), F.flat_get(cut, pos)
    assert (want_full != EMPTY).sum() > 1000
    if (size, depth) == (64, 1):
        assert cut.desc.node_count == full.desc.node_count and np.array_equal(want, want_full)
    else:
        assert cut.desc.node_count < full.desc.node_count and (want == EMPTY).all(), "every voxel lies under the cut"
    gpu.upload(cut)
    try:
        assert np.array_equal(gpu.get(pos), want), "cut view"
        dense = gpu.read_dense()
        gpu.set_node_mips(cut.node_mips)
        assert np.array_equal(gpu.get(pos), want), "cut view with node MIPs"
        assert np.array_equal(gpu.read_dense(), dense)
        assert np.array_equal(dense[pos[:, 2], pos[:, 1], pos[:, 0]], F.flat_albedo(cut, want))
        assert dense.any() == ((size, depth) == (64, 1))
    finally:
        gpu.set_node_mips(None)


# ------------------------------------------------------------------------------------------------- a real model
def test_gingerbread_model(gpu):
    import torch
    fx = ArrayTree(GINGERBREAD)
    img = TreeImage(fx.boxtree_size, fx.brick_dim, fx.arrays)
    size = img.boxtree_size
    gpu.upload(fx)
    out = torch.empty((size, size, size), dtype=torch.int32, device="cuda:0")
    assert gpu.read_dense(out=out) is out
    found = []  # the non-zero voxels, by slabs of 128 planes
    for z0 in range(0, size, 128):
        slab = out[z0:z0 + 128]
        if bool(slab.any()):
            at = slab.nonzero()
            found.append(np.concatenate([(at + torch.tensor([z0, 0, 0], device=at.device)).cpu().numpy(),
                                         to_host(slab[at[:, 0], at[:, 1], at[:, 2]]).astype(np.int64)[:, None]], 1))
    del out
    found = np.concatenate(found)
    pos, colours = found[:, 2::-1].astype(np.uint32), found[:, 3].astype(np.uint32)
    assert np.array_equal(F.flat_albedo(img, F.flat_get(img, pos)), colours), "the non-zero voxels of the whole cube"
    # ... and they are all of them: every brick is referenced once and spans 8^3 voxels in this model
    desc = img.node_children.reshape(-1, 64)[img.node_type == N.VHX_NODE_LEAF].ravel()
    solid = desc[(desc != EMPTY) & ((desc & N.VHX_SOLID_BIT) != 0)] & 0x7FFFFFFF
    cells = int((F.flat_albedo(img, img.voxels) != 0).sum()) + 512 * int((F.flat_albedo(img, img.solid_values[solid]) != 0).sum())
    assert len(pos) == cells
    rng = np.random.default_rng(8)
    probe = np.concatenate([F.seeded_positions(size, 100000, 8), pos[rng.integers(0, len(pos), 50000)]])
    want = F.flat_get(img, probe)
    assert (want != EMPTY).sum() >= 50000
    assert np.array_equal(gpu.get(probe), want)


# ------------------------------------------------------------------------------------------ read_dense round trips
@pytest.mark.parametrize("simplify", [False, True], ids=["plain", "simplified"])
@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_read_dense_round_trip(gpu, kind, size, bd, simplify):
    import torch
    what = f"{kind} {size}/{bd} simplify={simplify}"
    grid = G.make_grid(kind, size)
    gpu.build_dense(grid, size, bd, simplify=simplify)
    want = visible(grid, size)
    whole = gpu.read_dense()
    assert whole.dtype == np.uint32 and np.array_equal(whole, want), what
    (ox, oy, oz), (gx, gy, gz) = (3, 5, 1), (size - 5, min(7, size - 5), size - 3)
    if min(gx, gy, gz) >= 1:  # a box off every grid
        part = want[oz:oz + gz, oy:oy + gy, ox:ox + gx]
        assert np.array_equal(gpu.read_dense((ox, oy, oz), (gx, gy, gz)), part), f"{what}: box"
        out = torch.full((gz, gy, gx), 0x55, dtype=torch.int32, device="cuda:0")
        assert gpu.read_dense((ox, oy, oz), (gx, gy, gz), out=out) is out
        assert np.array_equal(to_host(out), part), f"{what}: box into a tensor"
    x, y, z = (size - 1,) * 3 if kind == "corner" else (size // 3, size // 4, size // 2)
    assert gpu.read_dense((x, y, z), (1, 1, 1)).tolist() == [[[int(want[z, y, x])]]], f"{what}: one voxel"
    out = np.full((size, size, size), 0x55, np.uint32)
    assert gpu.read_dense(out=out) is out and np.array_equal(out, want), f"{what}: numpy out"
    out = torch.full((size, size, size), 0x55, dtype=torch.int32, device="cuda:0")
    gpu.read_dense(out=out)
    assert np.array_equal(to_host(out), want), f"{what}: tensor out"
    # a box that sticks out of the cube is refused and nothing is written
    for origin, extents, shape in (((1, 0, 0), (size, 1, 1), (1, 1, size)), ((0, size, 0), (1, 1, 1), (1, 1, 1)),
                                   ((0, 0, size - 1), (1, 1, 2), (2, 1, 1))):
        for out in (np.full(shape, 0x55, np.uint32), torch.full(shape, 0x55, dtype=torch.int32, device="cuda:0")):
            with pytest.raises(N.VhxError) as e:
                gpu.read_dense(origin, extents, out=out)
            assert e.value.code == N.VHX_E_INVALID_ARG
            assert (np.asarray(out.cpu() if hasattr(out, "cpu") else out) == 0x55).all(), f"{what}: out was written"


# ------------------------------------------------------------------- more than one level, more than one scan tile
@pytest.mark.parametrize("simplify", [False, True], ids=["plain", "simplified"])
def test_read_and_get_at_256(gpu, simplify):
    grid = cached("grid256", grid_256)
    gpu.build_dense(to_device(grid), 256, 4, simplify=simplify)
    want = cached("visible256", lambda: visible(grid, 256))
    assert np.array_equal(gpu.read_dense(), want), "whole cube"
    img = gpu.download()
    assert img.desc.node_count > 1024
    pos = F.seeded_positions(256, 200000, 256)
    values = F.flat_get(img, pos)
    assert (values != EMPTY).sum() > 500
    assert np.array_equal(gpu.get(pos), values)
    assert np.array_equal(F.flat_albedo(img, values), want[pos[:, 2], pos[:, 1], pos[:, 0]])


# ------------------------------------------------------------------------------------------------ brick_dim above 4
@pytest.mark.parametrize("simplify", [False, True], ids=["plain", "simplified"])
@pytest.mark.parametrize("size,bd", [(64, 16), (128, 32)])
def test_read_and_get_with_large_bricks(gpu, size, bd, simplify):
    grid = G.make_grid("sparse", size)
    gpu.build_dense(grid, size, bd, simplify=simplify)
    want = visible(grid, size)
    assert np.array_equal(gpu.read_dense(), want), "whole cube"
    origin, extents = (5, 17, 2), (size - 9, size - 20, size - 3)  # units cut on every side, rows off 16 bytes
    assert np.array_equal(gpu.read_dense(origin, extents),
                          want[2:2 + extents[2], 17:17 + extents[1], 5:5 + extents[0]]), "box"
    img = gpu.download()
    pos = F.seeded_positions(size, 200000, size)
    values = F.flat_get(img, pos)
    assert np.array_equal(gpu.get(pos), values)
    assert np.array_equal(F.flat_albedo(img, values), want[pos[:, 2], pos[:, 1], pos[:, 0]])


# ---------------------------------------------------------------------------------------------- ordering and state
def test_state_errors_and_empty_calls():
    rt = vhx.Raytracer(0)
    try:
        pos, val = np.zeros(3, np.uint32), np.zeros(1, np.uint32)
        assert N.lib().vhx_get_voxels(rt._h, pos.ctypes.data, 1, val.ctypes.data, 0) == N.VHX_E_STATE
        box = N.DenseOut(0, 0, 0, 1, 1, 1, val.ctypes.data)
        assert N.lib().vhx_read_dense(rt._h, ctypes.byref(box), 0) == N.VHX_E_STATE
        with pytest.raises(N.VhxError) as e:
            rt.get(pos.reshape(1, 3))
        assert e.value.code == N.VHX_E_STATE
        rt.build_dense(G.make_grid("sparse", 16), 16, 4)
        assert N.lib().vhx_get_voxels(rt._h, None, 0, None, 0) == N.VHX_OK
        assert N.lib().vhx_get_voxels(rt._h, None, 0, None, 1) == N.VHX_OK
        assert rt.get(np.zeros((0, 3), np.uint32)).shape == (0,)
        assert N.lib().vhx_get_voxels(rt._h, None, 1, val.ctypes.data, 0) == N.VHX_E_INVALID_ARG
    finally:
        rt.close()


def test_values_overlapping_positions_on_the_device_are_refused(gpu):
    gpu.build_dense(G.make_grid("sparse", 16), 16, 4)
    t = to_device(F.seeded_positions(16, 64, 1))
    before = to_host(t).copy()
    lib, n = N.lib(), t.shape[0]
    for values in (t.data_ptr(), t.data_ptr() + 12 * n - 4, t.data_ptr() - 4 * n + 4):
        assert lib.vhx_get_voxels(gpu._h, t.data_ptr(), n, values, 1) == N.VHX_E_INVALID_ARG
    gpu.sync()
    assert np.array_equal(to_host(t), before)
    out = to_device(np.zeros(2 * n, np.uint32))  # ... and a range that only touches is fine
    assert lib.vhx_get_voxels(gpu._h, t.data_ptr(), n, out.data_ptr() + 4 * n, 1) == N.VHX_OK
    gpu.sync()
    assert np.array_equal(to_host(out)[n:], gpu.get(before.reshape(-1, 3)))


def test_shared_context_reads_the_owners_update():
    grid = G.make_grid("sparse", 64)
    flat = FlatTree.from_dense(grid, 64, 4)
    edited = TreeImage(64, 4, {k: np.array(getattr(flat, k)) for k in G.ARRAYS})
    # one voxel takes another visible colour of the palette
    at = int(np.flatnonzero(flat.voxels != EMPTY)[1234])
    old = int(flat.voxels[at]) & 0xFFFF
    new = next(c for c in range(flat.color_palette.size) if c != old and flat.color_palette[c] >> 24)
    edited.voxels[at] = 0xFFFF0000 | new
    pos = F.lattice((0, 0, 0), (64, 64, 64))
    before, after = F.flat_get(flat, pos), F.flat_get(edited, pos)
    assert (before != after).sum() == 1
    owner = vhx.Raytracer(0)
    try:
        owner.upload(flat)
        sh = owner.shared()
        dpos = to_device(pos)
        assert np.array_equal(to_host(sh.get(dpos)), before)
        owner.update_range(N.VHX_BUF_VOXELS, at, edited.voxels[at:at + 1])
        got = sh.get(dpos)  # no synchronisation in between: the get follows the write on the device
        assert np.array_equal(to_host(got), after)
        assert np.array_equal(sh.read_dense().ravel(), F.flat_albedo(edited, after))
        sh.close()
    finally:
        owner.close()


def test_a_rebuild_on_the_same_context_reads_the_new_tree(gpu):
    a, b = G.make_grid("sparse", 64, seed=1), G.make_grid("sparse", 32, seed=2)
    gpu.build_dense(a, 64, 4)
    assert np.array_equal(gpu.read_dense(), visible(a, 64))
    gpu.build_dense(b, 32, 2, simplify=True)
    assert np.array_equal(gpu.read_dense(), visible(b, 32))
    assert_get_everywhere(gpu, gpu.download(), "second build")
