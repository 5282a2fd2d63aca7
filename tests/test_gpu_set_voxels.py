"""vhx_set_voxels on the GPU: a list of points written into the device tree in place. The expected cubes and palettes
are kept by the numpy model (tests/_points_model.py, pinned to the host BoxTree by tests/test_set_voxels_model.py);
after a call the device's read_dense(data=True), get at every position, both palettes, structure (tests/_treecheck.py),
frame and derived state are checked against it and against the oracle on the downloaded image. Every comparison is bit
for bit."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree
from voxelhex_amd import _native as N
from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._points_model import PointsModel, random_points
from tests._treecheck import check_tree

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
W = 64
COLOURS = list(G.COLORS) + [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3), G.rgba(5, 5, 5)]  # the last three: in no base
VALUES = list(DG.DATA_VALUES) + [11, 0x7FFFFFFF]
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def positions(size):
    return cached(("lattice", size), lambda: F.lattice((0, 0, 0), (size,) * 3))


def sparse(size):
    return cached(("sparse", size), lambda: G.make_grid("sparse", size))


@pytest.fixture(scope="module")
def second():
    """A second context that uploads downloaded images: the derived state as an upload derives it."""
    rt = vhx.Raytracer(0)
    yield rt
    rt.close()


class Model(PointsModel):
    """The numpy model beside a Raytracer."""

    def __init__(self, rt, size, bd):
        self.rt, self.size, self.bd = rt, size, bd
        vis, dat = rt.read_dense(data=True)
        img = rt.download()
        super().__init__(vis, dat, img.color_palette, img.data_palette)

    def set(self, pos, albedo=None, data=None, mode="replace", source="host"):
        dev = (lambda w: w if w is None or np.isscalar(w) else to_device(w)) if source == "tensor" else (lambda w: w)
        self.rt.set_voxels(dev(pos), dev(albedo), dev(data), mode)
        self.apply(pos, albedo, data, mode)

    def clear(self, pos, source="host"):
        self.rt.clear_voxels(to_device(pos) if source == "tensor" else pos)
        self.apply(pos)

    def check(self, oracle, second, what, walker=True):
        rt, size, bd = self.rt, self.size, self.bd
        img = rt.download()
        assert img.color_palette.tolist() == self.colors, f"{what}: the colour palette"
        assert img.data_palette.tolist() == self.values, f"{what}: the data palette"
        a, p = rt.read_dense(data=True)
        assert np.array_equal(a, self.vis), f"{what}: read_dense, the albedo plane"
        assert np.array_equal(p, self.dat), f"{what}: read_dense, the data plane"
        pos = positions(size)
        got, want = rt.get(pos), self.val().ravel()
        assert np.array_equal(got, want), \
            f"{what}: get differs from the contract at {pos[np.flatnonzero(got != want)[:4]].tolist()}"
        if walker:
            assert np.array_equal(got, F.flat_get(img, pos)), f"{what}: get differs from the walker on the download"
        check_tree(img, rt.orphans(), what)
        cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
        frame, ref = rt.trace_primary(cam), oracle.trace_primary(img, cam, 0, 0, W, W)
        for k in ref:
            assert np.array_equal(np.ascontiguousarray(frame[k]).view(np.uint32),
                                  np.ascontiguousarray(ref[k]).view(np.uint32)), f"{what}: frame field {k}"
        second.upload(img)
        n = img.desc
        words = max(1, bd ** 3 // 64)
        assert np.array_equal(rt.read_derived(N.VHX_DERIVED_NODE_HDR, 0, n.node_count),
                              second.read_derived(N.VHX_DERIVED_NODE_HDR, 0, n.node_count)), f"{what}: node headers"
        if n.brick_count:
            assert np.array_equal(rt.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, n.brick_count * words),
                                  second.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, n.brick_count * words)), \
                f"{what}: brick bitmaps"
        return img


def brick_cells(origin, bd):
    return (F.lattice(origin, (bd,) * 3)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------- random points
SIZES = [(4, 1), (16, 4), (16, 1), (32, 2), (64, 4), (32, 8), (64, 16)]


@pytest.mark.parametrize("size,bd", SIZES)
def test_random_points_into_a_sparse_base(gpu, oracle, second, size, bd):
    what = f"{size}/{bd}"
    gpu.build_dense(sparse(size), size, bd)
    m = Model(gpu, size, bd)
    rng = np.random.default_rng(size * 10 + bd)
    n = 3000 if size == 64 else min(300, 2 * size ** 3)
    before = gpu.tree_counts()
    pos, a, d = random_points(rng, size, n, COLOURS, VALUES)
    m.set(pos, a, d, "replace", "host")  # both halves, points without an entry clear
    after = gpu.tree_counts()
    assert after.color_count >= before.color_count and after.data_count > before.data_count, what
    m.check(oracle, second, f"{what}: replace, host arrays, data")
    pos, a, d = random_points(rng, size, n, COLOURS, VALUES)
    kept = m.vis.copy()
    m.set(pos, a, None, "insert", "tensor")  # colours only; points with alpha 0 touch nothing
    m.check(oracle, second, f"{what}: insert, device tensors, no data")
    none = pos[a >> 24 == 0]
    hit = np.zeros(kept.shape, bool)
    hit[pos[a >> 24 != 0][:, 2], pos[a >> 24 != 0][:, 1], pos[a >> 24 != 0][:, 0]] = True
    untouched = none[~hit[none[:, 2], none[:, 1], none[:, 0]]]
    assert np.array_equal(m.vis[untouched[:, 2], untouched[:, 1], untouched[:, 0]],
                          kept[untouched[:, 2], untouched[:, 1], untouched[:, 0]]), what
    pos = random_points(rng, size, n // 2, COLOURS, VALUES)[0]
    m.set(pos, int(COLOURS[6]), 4242, "replace", "tensor")  # scalar fills: every point a Complex entry
    m.check(oracle, second, f"{what}: scalar fills")
    m.set(pos[: n // 4], 0, 17, "insert", "host")  # a data fill alone: Informative entries
    m.check(oracle, second, f"{what}: a data fill alone")
    assert (m.vis[pos[0, 2], pos[0, 1], pos[0, 0]] == 0) and m.dat[pos[0, 2], pos[0, 1], pos[0, 0]] == 17


def test_three_levels_and_an_internal_node_boundary(gpu, oracle, second):
    size, bd = 256, 4
    gpu.build_dense(to_device(sparse(size)), size, bd)
    m = Model(gpu, size, bd)
    rng = np.random.default_rng(256)
    pos, a, d = random_points(rng, size, 400, COLOURS, VALUES, lo=(40, 0, 100), hi=(90, 256, 150))
    assert (pos[:, 0] < 64).any() and (pos[:, 0] >= 64).any() and (pos[:, 2] < 128).any() and (pos[:, 2] >= 128).any()
    m.set(pos, a, d, "replace", "tensor")
    m.check(oracle, second, "256/4: both sides of internal-node boundaries", walker=False)


def test_no_point_and_one_point(gpu, oracle, second):
    size, bd = 32, 2
    gpu.build_dense(sparse(size), size, bd)
    before = gpu.download()
    m = Model(gpu, size, bd)
    m.set(np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    m.clear(np.zeros((0, 3), np.uint32))
    G.assert_same_image(gpu.download(), before, "n = 0")
    m.set(np.array([[31, 0, 17]], np.uint32), np.array([COLOURS[5]], np.uint32), None, "insert", "tensor")
    assert m.vis[17, 0, 31] == COLOURS[5]
    m.check(oracle, second, "n = 1")
    m.clear(np.array([[31, 0, 17]], np.uint32))
    m.check(oracle, second, "n = 1, cleared")


# ------------------------------------------------------------------------------ many points in one brick, duplicates
@pytest.mark.parametrize("size,bd", [(64, 16), (64, 4), (32, 8)])
def test_one_brick_with_more_points_than_a_workgroup(gpu, oracle, second, size, bd):
    gpu.build_dense(sparse(size), size, bd)
    m = Model(gpu, size, bd)
    rng = np.random.default_rng(bd)
    cells = brick_cells((size - 2 * bd, bd, size - bd), bd)  # every cell of one brick, in a shuffled order ...
    rng.shuffle(cells)
    extra = cells[rng.integers(0, len(cells), 700)]  # ... and 700 more points on top of them
    pos = np.concatenate([cells, extra])
    a = np.asarray(COLOURS, np.uint32)[rng.integers(0, len(COLOURS), len(pos))]
    d = np.asarray(VALUES, np.uint32)[rng.integers(0, len(VALUES), len(pos))]
    m.set(pos, a, d, "replace", "tensor")
    m.check(oracle, second, f"{size}/{bd}: a whole brick and duplicates")


def test_duplicates_the_last_point_decides(gpu, oracle, second):
    size, bd = 16, 4
    gpu.build_dense(sparse(size), size, bd)
    pal = gpu.download().color_palette.tolist()
    m = Model(gpu, size, bd)
    five = [int(G.rgba(10 + k, 0, 200)) for k in range(5)]
    p, q, r = (5, 6, 7), (12, 1, 3), (0, 15, 9)
    pos = np.array([p] * 5 + [q, q] + [r, r], np.uint32)
    a = np.array(five + [int(G.rgba(9, 9, 200)), 0] + [0, int(G.rgba(8, 8, 200))], np.uint32)
    m.set(pos, a)  # p five times; q written, then cleared; r cleared, then written
    img = m.check(oracle, second, "duplicates")
    assert m.vis[7, 6, 5] == five[4] and m.vis[3, 1, 12] == 0 and m.vis[9, 15, 0] == G.rgba(8, 8, 200)
    # the overridden colours are in the palette, in list order
    assert img.color_palette.tolist() == pal + five + [int(G.rgba(9, 9, 200)), int(G.rgba(8, 8, 200))]
    assert gpu.get(np.array([p], np.uint32))[0] == (0xFFFF0000 | (len(pal) + 4))


# ------------------------------------------------------------------------------------- simplified bases, empty trees
def test_ineffective_points_over_a_uniform_leaf_touch_nothing(gpu):
    size, bd = 64, 4
    gpu.build_dense(SG.make_grid("full", size, bd), size, bd, simplify=True)
    before = gpu.download()
    assert (before.node_type == N.VHX_NODE_UNIFORM_LEAF).any()
    pos = random_points(np.random.default_rng(1), size, 200, COLOURS, VALUES)[0]
    gpu.set_voxels(pos, np.full(200, G.rgba(1, 2, 3, 0), np.uint32), None, "insert")  # alpha 0, no data: no entry
    gpu.set_voxels(to_device(pos), 0, 0, "insert")
    G.assert_same_image(gpu.download(), before, "ineffective points")
    assert gpu.orphans() == (0, 0)


@pytest.mark.parametrize("size,bd", SIZES)
def test_into_an_empty_tree(gpu, oracle, second, size, bd):
    gpu.build_dense(G.make_grid("zero", size), size, bd)
    assert gpu.download().node_type.tolist() == [N.VHX_NODE_NOTHING]
    m = Model(gpu, size, bd)
    pos, a, d = random_points(np.random.default_rng(size + bd), size, 100, COLOURS, VALUES)
    pos[0], a[0] = (size - 1,) * 3, COLOURS[0]
    m.set(pos, a, d)
    img = m.check(oracle, second, f"{size}/{bd}: points into the empty tree")
    assert img.node_type[0] == (N.VHX_NODE_LEAF if size == 4 * bd else N.VHX_NODE_INTERNAL)
    assert gpu.orphans() == (0, 0)


def test_clearing_a_brick_a_leaf_and_the_whole_tree(gpu, oracle, second):
    size, bd = 64, 4
    gpu.build_dense(np.full((size,) * 3, G.rgba(10, 20, 30), np.uint32), size, bd)
    m = Model(gpu, size, bd)
    m.clear(brick_cells((20, 24, 28), bd))
    assert gpu.orphans() == (0, 1)
    m.check(oracle, second, "a brick cleared")
    m.clear(F.lattice((32, 16, 0), (16,) * 3).astype(np.uint32))
    assert gpu.orphans() == (1, 1 + 64)
    img = m.check(oracle, second, "a leaf cleared")
    assert img.desc.node_count == 1 + 64 and img.desc.brick_count == 64 * 64
    m.clear(positions(size).astype(np.uint32), "tensor")
    img = m.check(oracle, second, "everything cleared")
    assert img.node_type[0] == N.VHX_NODE_NOTHING and not m.vis.any()
    assert gpu.orphans() == (64, 64 * 64)
    m.set(np.array([[1, 2, 3]], np.uint32), int(COLOURS[0]))  # and the levels come back
    img = m.check(oracle, second, "written again")
    assert img.desc.node_count == 1 + 64 + 1 and img.desc.brick_count == 64 * 64 + 1


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8), (16, 1)])
@pytest.mark.parametrize("kind", ["full", "brick_noise", "blocks4", "cut"])
def test_simplified_bases(gpu, oracle, second, kind, size, bd):
    what = f"{kind} {size}/{bd}"
    gpu.build_dense(SG.make_grid(kind, size, bd), size, bd, simplify=True)
    old = gpu.download()
    SG.assert_case(kind, size, bd, old)
    m = Model(gpu, size, bd)
    rng = np.random.default_rng(size + bd)
    pos, a, d = random_points(rng, size, 40, COLOURS, VALUES)  # few points: most Solid bricks and UniformLeaf nodes stay
    m.set(pos, a, d, "replace")
    img = m.check(oracle, second, f"{what}: replace")
    assert np.array_equal(img.solid_values, old.solid_values), f"{what}: solid_values changed"
    pos, a, d = random_points(rng, size, 40, COLOURS, VALUES)
    m.set(pos, a, None, "insert", "tensor")
    img = m.check(oracle, second, f"{what}: insert")
    uni = np.flatnonzero(old.node_type == N.VHX_NODE_UNIFORM_LEAF)
    if uni.size:  # an expanded UniformLeaf keeps its index
        assert set(img.node_type[uni].tolist()) <= {N.VHX_NODE_LEAF, N.VHX_NODE_UNIFORM_LEAF}
    if kind == "full":
        assert (img.node_type[uni] == N.VHX_NODE_LEAF).any(), f"{what}: no UniformLeaf under the points"
    assert img.desc.brick_count > old.desc.brick_count


# -------------------------------------------------------------------- closure with compact, simplify, compact_palette
def resolved(image, values):
    values = np.asarray(values, np.uint32)
    return values & np.uint32(0xFFFF), DG.flat_data(image, values), (values >> 16) == 0xFFFF


def assert_same_up_to_data_palette(got, want, what):
    for k in ("node_type", "node_ocbits", "node_children", "color_palette"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), f"{what}: {k}"
    for k in ("voxels", "solid_values"):
        for x, y in zip(resolved(got, getattr(got, k)), resolved(want, getattr(want, k))):
            assert np.array_equal(x, y), f"{what}: {k} with data halves resolved"


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8)])
@pytest.mark.parametrize("with_data", [False, True])
def test_closure_with_compaction_and_simplification(gpu, size, bd, with_data):
    what = f"{size}/{bd} data={with_data}"
    rng = np.random.default_rng(size)
    pos, a, d = random_points(rng, size, 2000 if size == 64 else 400, COLOURS, VALUES, none=0.0)
    pos[:50] = F.lattice((bd, 0, 2 * bd), (bd, bd, bd))[:50]  # part of one brick in one colour
    a[:50] = COLOURS[0]
    if not with_data:
        d = None
    lo, hi = pos.min(0), pos.max(0) + 1
    images = {}
    for route in ("points", "box"):
        for finish in ("compact", "simplify"):
            gpu.build_dense(sparse(size), size, bd)
            if route == "points":
                m = Model(gpu, size, bd)
                m.set(pos, a, d, "insert", "tensor")
            else:  # the same voxels through write_dense(insert) of their bounding box
                box = m.vis[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].copy()
                keep = np.zeros(m.vis.shape, bool)
                keep[pos[:, 2], pos[:, 1], pos[:, 0]] = True
                box[~keep[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]] = 0
                plane = None
                if with_data:
                    plane = np.where(keep, m.dat, 0)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].astype(np.uint32)
                gpu.write_dense(box, tuple(int(v) for v in lo), "insert", data=plane)
            getattr(gpu, finish)()
            gpu.compact_palette()
            images[route, finish] = gpu.download()
    for finish in ("compact", "simplify"):
        host = FlatTree.from_dense(m.vis, size, bd, simplify=finish == "simplify", data=m.dat if with_data else None)
        if with_data:
            assert_same_up_to_data_palette(images["points", finish], host, f"{what}: {finish} against the host build")
            assert_same_up_to_data_palette(images["box", finish], images["points", finish], f"{what}: {finish}, box route")
        else:
            G.assert_same_image(images["points", finish], host, f"{what}: {finish} against the host build")
            G.assert_same_image(images["box", finish], images["points", finish], f"{what}: {finish}, box route")


def test_the_image_does_not_depend_on_scheduling(gpu):
    size, bd = 64, 4
    rng = np.random.default_rng(7)
    lists = [random_points(rng, size, 3000, COLOURS, VALUES) for _ in range(3)]
    downloads = []
    other = vhx.Raytracer(0)
    try:
        for rt in (gpu, other):
            rt.build_dense(sparse(size), size, bd)
            for k, (pos, a, d) in enumerate(lists):
                rt.set_voxels(to_device(pos), to_device(a), to_device(d), "insert" if k == 1 else "replace")
            rt.clear_voxels(F.lattice((16, 32, 48), (16,) * 3).astype(np.uint32))  # a whole leaf: orphans
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
        owner.set_voxels(to_device(pos), int(COLOURS[5]))
        after = sh.trace_primary(cam)  # no synchronisation in between
        new = owner.download()
        for got, img, what in ((before, old, "the frame before the call"), (after, new, "the shared context after it")):
            want = oracle.trace_primary(img, cam, 0, 0, W, W)
            for k in want:
                assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32),
                                      np.ascontiguousarray(want[k]).view(np.uint32)), f"{what}: {k}"
        assert not np.array_equal(before["value"], after["value"])
        for call in (lambda: sh.set_voxels(pos[:3], int(COLOURS[0])), lambda: sh.clear_voxels(pos[:3])):
            with pytest.raises(N.VhxError) as e:
                call()
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
        assert ctypes.sizeof(N.PointsIn) == 48  # vhx_points_in: a u64, three pointers, four u32
        pts = N.PointsIn(1, one.ctypes.data, None, None, int(COLOURS[0]), 0, N.VHX_WRITE_REPLACE, 0)
        assert N.lib().vhx_set_voxels(rt._h, ctypes.byref(pts), 0) == N.VHX_E_STATE  # before any upload
        tree = BoxTree(64, 4)
        tree.insert_scene(N.VHX_SCENE_LATTICE_CUBE)
        tree.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
        for flat, mips in ((tree.flatten_lod(0), False), (tree.flatten_lod(1), True)):
            rt.upload(flat)
            if mips:
                rt.set_node_mips(flat.node_mips)
            before = rt.download()
            for call in (lambda: rt.set_voxels(one, int(COLOURS[0])), lambda: rt.clear_voxels(one)):
                with pytest.raises(N.VhxError) as e:
                    call()
                assert e.value.code == N.VHX_E_STATE
            G.assert_same_image(rt.download(), before, "after a refused call")
            if mips:
                rt.set_node_mips(None)
                rt.set_voxels(one, int(COLOURS[5]))  # the full-depth view without MIPs takes the call
                assert rt.read_dense((33, 33, 33), (1, 1, 1))[0, 0, 0] == COLOURS[5]
        rt.build_dense(sparse(64), 64, 4)
        before = rt.download()
        assert N.lib().vhx_set_voxels(rt._h, None, 0) == N.VHX_E_INVALID_ARG
        pts = N.PointsIn(1, None, None, None, 0, 0, N.VHX_WRITE_REPLACE, 0)
        assert N.lib().vhx_set_voxels(rt._h, ctypes.byref(pts), 0) == N.VHX_E_INVALID_ARG  # null positions, n > 0
        pos = random_points(np.random.default_rng(3), 64, 100, COLOURS, VALUES)[0]
        for axis in range(3):
            bad = pos.copy()
            bad[37, axis] = 64
            for mode, albedo in (("replace", int(COLOURS[5])), ("insert", 0)):  # an ineffective point counts too
                with pytest.raises(N.VhxError) as e:
                    rt.set_voxels(bad if axis else to_device(bad), albedo, 0, mode)
                assert e.value.code == N.VHX_E_INVALID_ARG
        with pytest.raises(N.VhxError) as e:
            rt.set_voxels(pos, int(COLOURS[5]), 0, 2)
        assert e.value.code == N.VHX_E_INVALID_ARG
        G.assert_same_image(rt.download(), before, "after invalid arguments")
        assert rt.orphans() == (0, 0)
    finally:
        rt.close()


def test_a_list_with_too_many_values_is_refused(gpu):
    size, bd = 64, 4
    gpu.build_dense(sparse(size), size, bd)
    before = gpu.download()
    pos = positions(size)[:65536].astype(np.uint32)
    many = np.arange(1, 65537, dtype=np.uint32)
    for albedo, data in ((many | np.uint32(0xFF000000), None), (int(COLOURS[0]), many)):
        with pytest.raises(N.VhxError) as e:
            gpu.set_voxels(to_device(pos), albedo if np.isscalar(albedo) else to_device(albedo),
                           data if data is None else to_device(data))
        assert e.value.code == N.VHX_E_CAPACITY
        G.assert_same_image(gpu.download(), before, "after the refused call")
    assert gpu.orphans() == (0, 0)
    gpu.set_voxels(pos[:60000], many[:60000] | np.uint32(0xFF000000), many[:60000])  # 60,000 of each fit
    counts = gpu.tree_counts()
    assert counts.color_count == before.desc.color_count + 60000 and counts.data_count == 60000
