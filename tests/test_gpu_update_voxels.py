"""vhx_set_voxels with VHX_WRITE_UPDATE on the GPU (Raytracer.update_voxels): a list of points merged into the device
tree in place, each point writing only the halves (colour, data value) it has. The expected cubes and palettes are kept
by the numpy model (tests/_update_model.py, pinned to the host BoxTree.update loop by tests/test_update_model.py); after
every call the checks of tests/test_gpu_set_voxels.Model.check run. Structure and numbering are pinned to
VHX_WRITE_INSERT by downloads that must be equal in all seven buffers. Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _update_gpu as U
from tests._points_model import random_points

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
W = 64
COLOURS, VALUES = U.COLOURS, U.VALUES
to_device = U.to_device
SIZES = [(4, 1), (16, 4), (16, 1), (32, 2), (64, 4), (32, 8), (64, 16)]


@pytest.fixture(scope="module")
def second():
    """A second context that uploads downloaded images: the derived state as an upload derives it."""
    rt = vhx.Raytracer(0)
    yield rt
    rt.close()


def sparse(size):
    return U.cached(("sparse", size), lambda: G.make_grid("sparse", size))


# ------------------------------------------------------------------------------------------------- random points
@pytest.mark.parametrize("size,bd", SIZES)
def test_random_lists_into_a_data_base(gpu, oracle, second, size, bd):
    what = f"{size}/{bd}"
    m = U.data_base(gpu, size, bd)
    assert m.dat.any() and m.vis.any(), what
    rng = np.random.default_rng(size * 10 + bd)
    n = 3000 if size == 64 else min(300, 2 * size ** 3)
    pos, a, d = random_points(rng, size, n, COLOURS, VALUES)
    old_dat = m.dat.copy()
    m.update(pos, a, d, "host")  # both arrays, halves missing
    m.check(oracle, second, f"{what}: both halves, host arrays")
    colour_only = pos[(a >> 24 != 0) & (d == 0)]
    data_named = np.zeros(m.vis.shape, bool)
    data_named[pos[d != 0][:, 2], pos[d != 0][:, 1], pos[d != 0][:, 0]] = True
    kept = colour_only[~data_named[colour_only[:, 2], colour_only[:, 1], colour_only[:, 0]]]
    assert np.array_equal(m.dat[kept[:, 2], kept[:, 1], kept[:, 0]], old_dat[kept[:, 2], kept[:, 1], kept[:, 0]]), what
    pos, a, d = random_points(rng, size, n, COLOURS, VALUES)
    old_dat = m.dat.copy()
    m.update(pos, a, None, "tensor")  # a colour-only list: no data value changes
    m.check(oracle, second, f"{what}: colours only, device tensors")
    assert np.array_equal(m.dat, old_dat), what
    pos = random_points(rng, size, n // 2, COLOURS, VALUES)[0]
    old_vis = m.vis.copy()
    m.update(pos, None, 4242, "tensor")  # a data-only scalar fill: "give these voxels id 4242"
    m.check(oracle, second, f"{what}: a data fill alone")
    assert np.array_equal(m.vis, old_vis) and (m.dat[pos[:, 2], pos[:, 1], pos[:, 0]] == 4242).all(), what
    m.update(pos[: n // 4], int(COLOURS[6]), 17, "host")  # both fills
    m.check(oracle, second, f"{what}: both fills")


def test_three_levels_and_an_internal_node_boundary(gpu, oracle, second):
    size, bd = 256, 4
    m = U.data_base(gpu, size, bd, "tensor")
    rng = np.random.default_rng(256)
    pos, a, d = random_points(rng, size, 400, COLOURS, VALUES, lo=(40, 0, 100), hi=(90, 256, 150))
    assert (pos[:, 0] < 64).any() and (pos[:, 0] >= 64).any() and (pos[:, 2] < 128).any() and (pos[:, 2] >= 128).any()
    m.update(pos, a, d, "tensor")
    m.check(oracle, second, "256/4: both sides of internal-node boundaries", walker=False)


# ------------------------------------------------------------------------------ many points in one brick, duplicates
@pytest.mark.parametrize("size,bd", [(64, 16), (64, 4), (32, 8)])
def test_one_brick_with_more_points_than_a_workgroup(gpu, oracle, second, size, bd):
    m = U.data_base(gpu, size, bd)
    rng = np.random.default_rng(bd)
    cells = U.brick_cells((size - 2 * bd, bd, size - bd), bd)  # every cell of one brick, in a shuffled order ...
    rng.shuffle(cells)
    extra = cells[rng.integers(0, len(cells), 700)]  # ... and 700 more points on top of them
    pos = np.concatenate([cells, extra])
    a = np.asarray(COLOURS, np.uint32)[rng.integers(0, len(COLOURS), len(pos))]
    d = np.asarray(VALUES, np.uint32)[rng.integers(0, len(VALUES), len(pos))]
    half = rng.random(len(pos)) < 0.5  # about half the points colour-only, half data-only
    a[half], d[~half] = 0, 0
    m.update(pos, a, d, "tensor")
    m.check(oracle, second, f"{size}/{bd}: a whole brick and duplicates")


def test_duplicates_each_half_has_its_own_last_point(gpu, oracle, second):
    size, bd = 16, 4
    m = U.data_base(gpu, size, bd)
    img = gpu.download()
    pal, dpal = img.color_palette.tolist(), img.data_palette.tolist()
    five = [int(G.rgba(10 + k, 0, 200)) for k in range(5)]
    c1, c2 = int(G.rgba(9, 9, 200)), int(G.rgba(8, 8, 200))
    p, q, r = (5, 6, 7), (12, 1, 3), (0, 15, 9)
    for v in (q, r):  # two empty voxels
        m.clear(np.array([v], np.uint32))
    pos = np.array([p] * 5 + [q, q] + [r, r], np.uint32)
    a = np.array(five + [c1, 0] + [0, c2], np.uint32)
    d = np.array([0, 501, 0, 502, 0] + [0, 503] + [504, 0], np.uint32)
    m.update(pos, a, d)  # q: Visual, then Informative; r: Informative, then Visual
    img = m.check(oracle, second, "duplicates")
    assert m.vis[7, 6, 5] == five[4] and m.dat[7, 6, 5] == 502
    assert (m.vis[3, 1, 12], m.dat[3, 1, 12]) == (c1, 503) and (m.vis[9, 15, 0], m.dat[9, 15, 0]) == (c2, 504)
    # the overridden colours and values are in the palettes, in list order
    assert img.color_palette.tolist() == pal + five + [c1, c2]
    assert img.data_palette.tolist() == dpal + [501, 502, 503, 504]
    got = gpu.get(np.array([p, q, r], np.uint32)).tolist()
    nc, nd = len(pal), len(dpal)
    assert got == [(nc + 4) | ((nd + 1) << 16), (nc + 5) | ((nd + 2) << 16), (nc + 6) | ((nd + 3) << 16)]  # Complex


# ------------------------------------------------------------------------------------- simplified bases, empty trees
@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8), (16, 1)])
@pytest.mark.parametrize("kind", ["full", "brick_noise", "blocks4", "cut"])
def test_simplified_bases(gpu, oracle, second, kind, size, bd):
    what = f"{kind} {size}/{bd}"
    g, d = U.simplified_pair(kind, size, bd)
    gpu.build_dense(g, size, bd, simplify=True, data=d)
    old = gpu.download()
    solid_entry = (old.node_children != EMPTY) & ((old.node_children & N.VHX_SOLID_BIT) != 0)
    assert (old.node_type == N.VHX_NODE_UNIFORM_LEAF).any() or solid_entry.any(), what
    m = U.Model(gpu, size, bd)
    rng = np.random.default_rng(size + bd)
    pos, a, dd = random_points(rng, size, 40, COLOURS, VALUES)  # few points: most Solid bricks and UniformLeaf nodes stay
    m.update(pos, a, dd)
    img = m.check(oracle, second, f"{what}: both halves")
    assert np.array_equal(img.solid_values, old.solid_values), f"{what}: solid_values changed"
    pos = random_points(rng, size, 40, COLOURS, VALUES)[0]
    before = m.vis.copy()
    m.update(pos, None, 31337, "tensor")  # data-only points: a voxel of a Solid brick or a UniformLeaf keeps its colour
    img = m.check(oracle, second, f"{what}: a data fill alone")
    assert np.array_equal(m.vis, before) and (m.dat[pos[:, 2], pos[:, 1], pos[:, 0]] == 31337).all(), what
    assert (m.dat == 31337).sum() == len(np.unique(pos, axis=0)), f"{what}: the rest of the bricks reads as before"
    uni = np.flatnonzero(old.node_type == N.VHX_NODE_UNIFORM_LEAF)
    if uni.size:  # an expanded UniformLeaf keeps its index
        assert set(img.node_type[uni].tolist()) <= {N.VHX_NODE_LEAF, N.VHX_NODE_UNIFORM_LEAF}
    if kind == "full":
        assert (img.node_type[uni] == N.VHX_NODE_LEAF).any(), f"{what}: no UniformLeaf under the points"


@pytest.mark.parametrize("size,bd", SIZES)
def test_into_an_empty_tree(gpu, oracle, second, size, bd):
    gpu.build_dense(G.make_grid("zero", size), size, bd)
    assert gpu.download().node_type.tolist() == [N.VHX_NODE_NOTHING]
    m = U.Model(gpu, size, bd)
    pos, a, d = random_points(np.random.default_rng(size + bd), size, 100, COLOURS, VALUES)
    pos[0], a[0] = (size - 1,) * 3, COLOURS[0]
    m.update(pos, a, d)  # update of an empty voxel is an insert
    img = m.check(oracle, second, f"{size}/{bd}: points into the empty tree")
    assert img.node_type[0] == (N.VHX_NODE_LEAF if size == 4 * bd else N.VHX_NODE_INTERNAL)
    assert gpu.orphans() == (0, 0)


def test_no_point(gpu):
    size, bd = 32, 2
    m = U.data_base(gpu, size, bd)
    before = gpu.download()
    m.update(np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    gpu.update_voxels(to_device(np.zeros((0, 3), np.uint32)), 5, 5)
    G.assert_same_image(gpu.download(), before, "n = 0")


def test_ineffective_points_over_a_uniform_leaf_touch_nothing(gpu):
    size, bd = 64, 4
    g, d = U.simplified_pair("full", size, bd)
    gpu.build_dense(g, size, bd, simplify=True, data=d)
    before = gpu.download()
    assert (before.node_type == N.VHX_NODE_UNIFORM_LEAF).any()
    pos = random_points(np.random.default_rng(1), size, 200, COLOURS, VALUES)[0]
    gpu.update_voxels(pos, np.full(200, G.rgba(1, 2, 3, 0), np.uint32), None)  # alpha 0, no data: no half
    gpu.update_voxels(to_device(pos), 0, 0)
    gpu.update_voxels(pos, np.full(200, G.rgba(1, 2, 3, 0), np.uint32), np.zeros(200, np.uint32))
    G.assert_same_image(gpu.download(), before, "ineffective points")
    assert gpu.orphans() == (0, 0)


# ------------------------------------------------------------------------------------- differential: update / insert
def distinct_points(rng, size, n):
    at = rng.choice(size ** 3, n, replace=False)
    return np.stack([at % size, (at // size) % size, at // (size * size)], 1).astype(np.uint32)


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8)])
def test_structure_and_numbering_are_those_of_insert(gpu, size, bd):
    what = f"{size}/{bd}"
    rng = np.random.default_rng(size + 1)
    n = 1500 if size == 64 else 400
    pos = distinct_points(rng, size, n)
    a = np.asarray([c for c in COLOURS if c >> 24], np.uint32)[rng.integers(0, len(COLOURS) - 1, n)]
    d = np.asarray(VALUES, np.uint32)[rng.integers(0, len(VALUES), n)]
    g, dg = U.data_pair(size)
    images = {}
    for base in ("data", "plain"):
        for mode in ("update", "insert"):
            for words in ("both", "colour"):
                gpu.build_dense(g, size, bd, data=dg if base == "data" else None)
                gpu.set_voxels(to_device(pos), to_device(a), to_device(d) if words == "both" else None, mode)
                images[base, mode, words] = (gpu.download(), gpu.orphans())
    for base in ("data", "plain"):  # no duplicates, both halves on every point: nothing of the old voxel is kept
        G.assert_same_image(images[base, "update", "both"][0], images[base, "insert", "both"][0], f"{what} {base}: both")
        assert images[base, "update", "both"][1] == images[base, "insert", "both"][1], what
    # colours only on a tree without data values: there is no half to keep
    G.assert_same_image(images["plain", "update", "colour"][0], images["plain", "insert", "colour"][0], f"{what}: colours")
    # on a tree with data values insert drops them and update keeps them
    up, ins = images["data", "update", "colour"][0], images["data", "insert", "colour"][0]
    for k in ("node_type", "node_ocbits", "node_children", "color_palette", "data_palette", "solid_values"):
        assert np.array_equal(getattr(up, k), getattr(ins, k)), f"{what}: {k}"
    assert up.voxels.shape == ins.voxels.shape and not np.array_equal(up.voxels, ins.voxels), what
    assert np.array_equal(up.voxels & 0xFFFF, ins.voxels & 0xFFFF), f"{what}: the colour halves"


# -------------------------------------------------------------------- closure with compact, simplify, compact_palettes
@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8)])
@pytest.mark.parametrize("finish", ["compact", "simplify"])
def test_closure_with_compaction_and_simplification(gpu, size, bd, finish):
    what = f"{size}/{bd} {finish}"
    m = U.data_base(gpu, size, bd)
    rng = np.random.default_rng(size)
    n = 2000 if size == 64 else 400
    pos, a, d = random_points(rng, size, n, COLOURS, VALUES)
    pos[:50] = F.lattice((bd, 0, 2 * bd), (bd, bd, bd))[:50]  # part of one brick in one colour
    a[:50] = COLOURS[0]
    m.update(pos, a, d, "tensor")
    box = F.lattice((0, 0, 0), (4 * bd,) * 3).astype(np.uint32)  # a whole leaf in one colour and one value
    m.update(box, int(COLOURS[1]), 9)
    m.update(pos[: n // 2], None, 606, "tensor")
    getattr(gpu, finish)()
    gpu.compact_palettes()
    host = FlatTree.from_dense(m.vis, size, bd, simplify=finish == "simplify", data=m.dat)
    G.assert_same_image(gpu.download(), host, f"{what}: against the host build of the model's cubes")


def test_the_image_does_not_depend_on_scheduling(gpu):
    size, bd = 64, 4
    rng = np.random.default_rng(7)
    lists = [random_points(rng, size, 3000, COLOURS, VALUES) for _ in range(3)]
    g, d = U.data_pair(size)
    downloads = []
    other = vhx.Raytracer(0)
    try:
        for rt in (gpu, other):
            rt.build_dense(g, size, bd, data=d)
            for k, (pos, a, dd) in enumerate(lists):
                rt.update_voxels(to_device(pos), to_device(a), None if k == 1 else to_device(dd))
            rt.clear_voxels(F.lattice((16, 32, 48), (16,) * 3).astype(np.uint32))  # a whole leaf: orphans
            rt.update_voxels(F.lattice((16, 32, 48), (3, 3, 3)).astype(np.uint32), 0, 5)
            downloads.append((rt.download(), rt.orphans()))
    finally:
        other.close()
    G.assert_same_image(downloads[0][0], downloads[1][0], "the same calls on a second context")
    assert downloads[0][1] == downloads[1][1] and downloads[0][1][0] >= 1 and downloads[0][1][1] > 0


# ------------------------------------------------------------------------------------------------------- ordering
def test_shared_contexts_and_frames_in_flight(oracle):
    size, bd = 64, 4
    cam = vhx.glass_camera(size, W, W, target=(32.0,) * 3)
    owner = vhx.Raytracer(0)
    try:
        owner.build_dense(G.make_grid("sparse", size, seed=4), size, bd)
        old = owner.download()
        sh = owner.shared()  # created before the write
        before = sh.trace_primary(cam)
        pos = F.lattice((10, 20, 30), (30, 30, 30)).astype(np.uint32)
        owner.update_voxels(to_device(pos), int(COLOURS[5]))
        after = sh.trace_primary(cam)  # no synchronisation in between
        new = owner.download()
        for got, img, what in ((before, old, "the frame before the call"), (after, new, "the shared context after it")):
            want = oracle.trace_primary(img, cam, 0, 0, W, W)
            for k in want:
                assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32),
                                      np.ascontiguousarray(want[k]).view(np.uint32)), f"{what}: {k}"
        assert not np.array_equal(before["value"], after["value"])
        with pytest.raises(N.VhxError) as e:
            sh.update_voxels(pos[:3], int(COLOURS[0]))
        assert e.value.code == N.VHX_E_STATE
        G.assert_same_image(owner.download(), new, "after the refused call on the shared context")
        sh.close()
    finally:
        owner.close()


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_tree_as_it_was():
    rt = vhx.Raytracer(0)
    one = np.array([[33, 33, 33]], np.uint32)  # in the scene's solid part: the LOD-cut views hold no child there
    try:
        pts = N.PointsIn(1, one.ctypes.data, None, None, int(COLOURS[0]), 0, N.VHX_WRITE_UPDATE, 0)
        assert N.lib().vhx_set_voxels(rt._h, ctypes.byref(pts), 0) == N.VHX_E_STATE  # before any upload
        tree = BoxTree(64, 4)
        tree.insert_scene(N.VHX_SCENE_LATTICE_CUBE)
        tree.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
        for flat, mips in ((tree.flatten_lod(0), False), (tree.flatten_lod(1), True)):
            rt.upload(flat)
            if mips:
                rt.set_node_mips(flat.node_mips)
            before = rt.download()
            with pytest.raises(N.VhxError) as e:
                rt.update_voxels(one, int(COLOURS[0]))
            assert e.value.code == N.VHX_E_STATE
            G.assert_same_image(rt.download(), before, "after a refused call")
            if mips:
                rt.set_node_mips(None)
                rt.update_voxels(one, int(COLOURS[5]))  # the full-depth view without MIPs takes the call
                assert rt.read_dense((33, 33, 33), (1, 1, 1))[0, 0, 0] == COLOURS[5]
        g, d = U.data_pair(64)
        rt.build_dense(g, 64, 4, data=d)
        before = rt.download()
        pos = random_points(np.random.default_rng(3), 64, 100, COLOURS, VALUES)[0]
        for axis in range(3):
            bad = pos.copy()
            bad[37, axis] = 64
            for albedo in (int(COLOURS[5]), 0):  # an ineffective point counts too
                with pytest.raises(N.VhxError) as e:
                    rt.update_voxels(bad if axis else to_device(bad), albedo, 0)
                assert e.value.code == N.VHX_E_INVALID_ARG
        grid = np.full((2, 2, 2), COLOURS[5], np.uint32)
        for mode in (2, 3, 5):  # no modes, in all three calls
            for call in (lambda: rt.set_voxels(pos, int(COLOURS[5]), 0, mode),
                         lambda: rt.write_dense(grid, (1, 1, 1), mode),
                         lambda: rt.write_dense(grid, (1, 1, 1), mode, data=3)):
                with pytest.raises(N.VhxError) as e:
                    call()
                assert e.value.code == N.VHX_E_INVALID_ARG
        G.assert_same_image(rt.download(), before, "after invalid arguments")
        assert rt.orphans() == (0, 0)
    finally:
        rt.close()


def test_a_list_with_too_many_values_is_refused(gpu):
    size, bd = 64, 4
    gpu.build_dense(sparse(size), size, bd)
    before = gpu.download()
    pos = U.positions(size)[:65536].astype(np.uint32)
    many = np.arange(1, 65537, dtype=np.uint32)
    for albedo, data in ((many | np.uint32(0xFF000000), None), (None, many)):
        with pytest.raises(N.VhxError) as e:
            gpu.update_voxels(to_device(pos), albedo if albedo is None else to_device(albedo),
                              data if data is None else to_device(data))
        assert e.value.code == N.VHX_E_CAPACITY
        G.assert_same_image(gpu.download(), before, "after the refused call")
    assert gpu.orphans() == (0, 0)
    gpu.update_voxels(pos[:60000], many[:60000] | np.uint32(0xFF000000), many[:60000])  # 60,000 of each fit
    counts = gpu.tree_counts()
    assert counts.color_count == before.desc.color_count + 60000 and counts.data_count == 60000
