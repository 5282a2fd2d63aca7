"""vhx_write_dense_data on the GPU: a box of the device tree replaced in place by voxels that carry user data. As in
tests/test_gpu_dense_write.py the expected cube is kept in numpy beside every write -- here three cubes: the visible
colour, the data value, and what get returns by the call's contract -- and after a write the device's
read_dense(data=True), get at every position, structure (tests/_treecheck.py), frame and derived state are checked
against it and against the oracle on the downloaded image. Every comparison is bit for bit."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree
from voxelhex_amd import _native as N
from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests import _flatget as F
from tests._treecheck import check_tree

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
W = 64
NEW_COLOURS = [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3)]  # colours no base grid holds
NEW_DATA = [11, 0x7FFFFFFF]  # data values no base grid holds
SIZES = [(4, 1), (16, 4), (32, 8), (64, 16), (16, 1), (32, 2), (64, 4)]
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


def base_pair(size):
    return cached(("pair", size), lambda: DG.make_pair("sparse", size))


def odd_box(size):
    origin = (size * 13 // 64, size * 15 // 64, size * 3 // 64)
    extents = (max(1, size * 22 // 64), max(1, size * 18 // 64), max(1, size * 35 // 64))
    return origin, extents


def random_box(rng, extents, density=0.4, new=True):
    """(albedo, data) of a box: none, colour-only, data-only and both."""
    gx, gy, gz = extents
    colours = np.concatenate([G.COLORS, np.array(NEW_COLOURS if new else [], np.uint32)])
    values = np.concatenate([DG.DATA_VALUES, np.array(NEW_DATA if new else [], np.uint32)])
    g = np.zeros((gz, gy, gx), np.uint32)
    d = np.zeros((gz, gy, gx), np.uint32)
    mask = rng.random(g.shape) < density
    g[mask] = colours[rng.integers(0, len(colours), int(mask.sum()))]
    mask = rng.random(g.shape) < density
    d[mask] = values[rng.integers(0, len(values), int(mask.sum()))]
    return g, d


def lowest_index(palette, wanted):
    """Lowest index in `palette` of every value of `wanted` (all present)."""
    uniq, first = np.unique(palette, return_index=True)
    at = np.searchsorted(uniq, wanted)
    assert (uniq[np.minimum(at, max(uniq.size - 1, 0))] == wanted).all(), "a written value is not in its palette"
    return first[at].astype(np.uint32)


@pytest.fixture(scope="module")
def second():
    """A second context that uploads downloaded images: the derived state as an upload derives it."""
    rt = vhx.Raytracer(0)
    yield rt
    rt.close()


class Model:
    """The expected cubes beside a Raytracer: `vis` and `dat` what read_dense(data=True) gives, `val` what get gives."""

    def __init__(self, rt, size, bd):
        self.rt, self.size, self.bd = rt, size, bd
        self.vis, self.dat = rt.read_dense(data=True)
        self.val = rt.get(positions(size)).reshape(size, size, size)

    def expect(self, grid, data, origin, mode):
        """The cubes after a write the device has just done (the palette indices come from its new palettes)."""
        ox, oy, oz = origin
        gz, gy, gx = grid.shape
        g = DG.visible(grid)
        d = np.asarray(data, np.uint32)
        entry = (g != 0) | (d != 0)
        covered = np.ones(g.shape, bool) if mode == "replace" else entry
        counts = self.rt.tree_counts()
        ci = np.full(g.shape, 0xFFFF, np.uint32)
        di = np.full(g.shape, 0xFFFF, np.uint32)
        if (g != 0).any():
            ci[g != 0] = lowest_index(self.rt.read_range(N.VHX_BUF_COLOR_PALETTE, 0, counts.color_count), g[g != 0])
        if (d != 0).any():
            di[d != 0] = lowest_index(self.rt.read_range(N.VHX_BUF_DATA_PALETTE, 0, counts.data_count), d[d != 0])
        value = np.where(entry, ci | (di << np.uint32(16)), np.uint32(EMPTY)).astype(np.uint32)
        sl = (slice(oz, oz + gz), slice(oy, oy + gy), slice(ox, ox + gx))
        self.vis[sl] = np.where(covered, g, self.vis[sl])
        self.dat[sl] = np.where(covered, d, self.dat[sl])
        self.val[sl] = np.where(covered, value, self.val[sl])

    def write(self, grid, data, origin=(0, 0, 0), mode="replace", source="host"):
        """`data`: a plane, or an integer (fill_data)."""
        plane = np.full(grid.shape, data, np.uint32) if isinstance(data, int) else data
        if source == "tensor":
            self.rt.write_dense(to_device(grid), origin, mode, data=data if isinstance(data, int) else to_device(data))
        else:
            self.rt.write_dense(grid, origin, mode, data=data)
        self.expect(grid, plane, origin, mode)

    def fill(self, origin, extents, albedo, data=0, source="host"):
        """`data`: an integer, or a plane."""
        gx, gy, gz = extents
        if isinstance(data, int):
            self.rt.fill_box(origin, extents, albedo, data)
            plane = np.full((gz, gy, gx), data, np.uint32)
        else:
            self.rt.fill_box(origin, extents, albedo, to_device(data) if source == "tensor" else data)
            plane = data
        self.expect(np.full((gz, gy, gx), albedo, np.uint32), plane, origin, "replace")

    def check(self, oracle, second, what):
        rt, size, bd = self.rt, self.size, self.bd
        img = rt.download()
        a, p = rt.read_dense(data=True)
        assert np.array_equal(a, self.vis), f"{what}: read_dense, the albedo plane"
        assert np.array_equal(p, self.dat), f"{what}: read_dense, the data plane"
        pos = positions(size)
        got = rt.get(pos)
        assert np.array_equal(got, self.val.ravel()), \
            f"{what}: get differs from the contract at {pos[np.flatnonzero(got != self.val.ravel())[:4]].tolist()}"
        assert np.array_equal(got, F.flat_get(img, pos)), f"{what}: get differs from the walker on the download"
        check_tree(img, rt.orphans(), what)
        cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
        frame, want = rt.trace_primary(cam), oracle.trace_primary(img, cam, 0, 0, W, W)
        for k in want:
            assert np.array_equal(np.ascontiguousarray(frame[k]).view(np.uint32),
                                  np.ascontiguousarray(want[k]).view(np.uint32)), f"{what}: frame field {k}"
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


# --------------------------------------------------------------------------------------- sizes, boxes and sources
@pytest.mark.parametrize("source", ["host", "tensor"])
@pytest.mark.parametrize("size,bd", SIZES)
def test_boxes_into_a_sparse_data_base(gpu, oracle, second, size, bd, source):
    what = f"{size}/{bd} {source}"
    g, d = base_pair(size)
    gpu.build_dense(g, size, bd, data=d)
    m = Model(gpu, size, bd)
    assert np.array_equal(m.vis, DG.extend(DG.visible(g), size)) and np.array_equal(m.dat, DG.extend(d, size)), what
    rng = np.random.default_rng(size * 10 + bd)
    origin, extents = odd_box(size)
    before = gpu.tree_counts()
    m.write(*random_box(rng, extents), origin, "replace", source)  # both planes
    after = gpu.tree_counts()
    if np.prod(extents) >= 40:
        assert before.data_count < after.data_count <= before.data_count + len(NEW_DATA), what
    m.check(oracle, second, f"{what}: both planes, replace")
    bg, bd_ = random_box(rng, extents, 0.3)
    m.write(bg, bd_, origin, "insert", source)
    m.check(oracle, second, f"{what}: both planes, insert")
    m.write(bg, 12345, (0, 0, 0), "insert", source)  # an albedo plane with fill_data: every voxel of the box is an entry
    m.check(oracle, second, f"{what}: an albedo plane with fill_data")
    m.fill(origin, extents, int(NEW_COLOURS[0]), random_box(rng, extents, 0.5)[1], source)  # fill with a data plane
    m.check(oracle, second, f"{what}: a fill colour with a data plane")
    m.fill((0, 0, 0), (max(1, size // 2),) * 3, int(G.COLORS[1]), 0x80000000)
    m.check(oracle, second, f"{what}: fill_box with a colour and a data value")
    m.fill((0, 0, 0), (max(1, size // 4), size, max(1, size // 3)), 0, 31)  # data-only voxels
    m.check(oracle, second, f"{what}: fill_box with a data value alone")
    m.fill((0, 0, 0), (size, max(1, size // 2), size), 0, 0)
    m.check(oracle, second, f"{what}: fill_box(0, 0) clears")
    assert not m.vis[:, : max(1, size // 2)].any() and not m.dat[:, : max(1, size // 2)].any()


@pytest.mark.parametrize("size,bd", SIZES)
def test_into_an_empty_tree(gpu, oracle, second, size, bd):
    what = f"{size}/{bd}"
    gpu.build_dense(G.make_grid("zero", size), size, bd)
    assert gpu.download().node_type.tolist() == [N.VHX_NODE_NOTHING]
    m = Model(gpu, size, bd)
    origin, extents = odd_box(size)
    m.write(*random_box(np.random.default_rng(size + bd), extents), origin)
    img = m.check(oracle, second, f"{what}: a box into the empty tree")
    assert gpu.orphans() == (0, 0) and img.desc.data_count > 0
    corner = np.zeros((1, 1, 1), np.uint32)
    m.write(corner, np.full((1, 1, 1), 99, np.uint32), (size - 1,) * 3, "insert")  # one data-only voxel
    m.check(oracle, second, f"{what}: a data-only voxel at the far corner")
    assert m.val[-1, -1, -1] != EMPTY and (m.val[-1, -1, -1] & 0xFFFF) == 0xFFFF


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 2), (32, 8), (16, 1)])
def test_into_a_simplified_base(gpu, oracle, second, size, bd):
    what = f"{size}/{bd}"
    g = np.full((size,) * 3, G.rgba(10, 20, 30), np.uint32)
    d = np.full_like(g, 7)
    d[: size // 2, : size // 4] = 9
    gpu.build_dense(g, size, bd, simplify=True, data=d)
    old = gpu.download()
    assert (old.node_type == N.VHX_NODE_UNIFORM_LEAF).any()
    m = Model(gpu, size, bd)
    assert np.array_equal(m.vis, g) and np.array_equal(m.dat, d)
    origin, extents = odd_box(size)
    rng = np.random.default_rng(size)
    m.write(*random_box(rng, extents, 0.5), origin, "replace")
    img = m.check(oracle, second, f"{what}: replace")
    uni = np.flatnonzero(old.node_type == N.VHX_NODE_UNIFORM_LEAF)
    assert (img.node_type[uni] == N.VHX_NODE_LEAF).any(), "a UniformLeaf under the box is expanded"
    assert np.array_equal(img.solid_values, old.solid_values)
    m.write(*random_box(rng, (size, 3, size), 0.5), (0, size - 3, 0), "insert")
    m.check(oracle, second, f"{what}: insert")


# ------------------------------------------------------------------------------------------------------ palettes
def test_new_data_values_follow_the_palette_in_insert_order(gpu, oracle, second):
    g, d = base_pair(16)
    gpu.build_dense(g, 16, 4, data=d)
    pal = gpu.download().data_palette.tolist()
    a, b = 1001, 1002
    box = np.zeros((4, 4, 4), np.uint32)
    box[0, 0, 1] = a  # (x, y, z) = (1, 0, 0): memory order meets A first
    box[1, 0, 0] = b  # (x, y, z) = (0, 0, 1): the insert loop B
    box[2, 3, 3] = pal[1]  # an old value, last in every order
    m = Model(gpu, 16, 4)
    m.write(np.zeros_like(box), box, (5, 6, 7))
    img = m.check(oracle, second, "data palette order")
    assert img.data_palette.tolist() == pal + [b, a]
    assert m.val[7 + 2, 6 + 3, 5 + 3] == (0xFFFF | (1 << 16))
    m.write(np.zeros_like(box), box[::-1].copy(), (1, 1, 1), "insert", "tensor")  # nothing new: the palette stays
    assert m.check(oracle, second, "data palette reuse").data_palette.tolist() == pal + [b, a]


def test_an_uploaded_palette_with_a_zero_and_a_duplicate(gpu, oracle, second):
    size, bd = 16, 4
    g, d = base_pair(size)
    img = FlatTree.from_dense(g, size, bd, data=d)
    arrays = {k: np.array(getattr(img, k)) for k in G.ARRAYS}
    pal = arrays["data_palette"]
    dup = int(pal[1])
    arrays["data_palette"] = np.concatenate([pal, np.array([0, dup, 0], np.uint32)])  # indices n, n + 1, n + 2
    edited = vhx.boxtree.TreeImage(size, bd, arrays)
    gpu.upload(edited)
    m = Model(gpu, size, bd)
    box = np.zeros((2, 2, 2), np.uint32)
    box[0, 0, 0] = dup
    box[1, 1, 1] = 4242
    m.write(np.zeros_like(box), box, (3, 3, 3))
    out = m.check(oracle, second, "a palette with a 0 entry and a duplicate")
    assert m.val[3, 3, 3] == (0xFFFF | (1 << 16)), "the duplicate resolves to the lowest index"
    assert out.data_palette.tolist() == arrays["data_palette"].tolist() + [4242], "the 0 entries are never matched"
    assert m.val[4, 4, 4] == (0xFFFF | ((pal.size + 3) << 16))


def test_a_visual_write_over_a_complex_voxel_drops_its_data(gpu, oracle, second):
    size, bd = 16, 4
    c = G.rgba(50, 60, 70)
    gpu.build_dense(np.full((size,) * 3, c, np.uint32), size, bd, data=np.full((size,) * 3, 5, np.uint32))
    m = Model(gpu, size, bd)
    assert (m.val == (0 | (0 << 16))).all()
    other = np.full((3, 3, 3), G.rgba(1, 1, 1), np.uint32)
    for mode in ("replace", "insert"):
        origin = (2, 2, 2) if mode == "replace" else (9, 9, 9)
        m.write(other, 0, origin, mode)
        m.check(oracle, second, f"Visual over Complex, {mode}")
        x, y, z = origin
        assert (m.dat[z:z + 3, y:y + 3, x:x + 3] == 0).all() and (m.val[z:z + 3, y:y + 3, x:x + 3] == (1 | 0xFFFF0000)).all()
    gpu.write_dense(other, (5, 5, 5))  # the colour-only call does the same
    m.expect(other, np.zeros_like(other), (5, 5, 5), "replace")
    m.check(oracle, second, "write_dense over Complex")
    m.write(np.zeros((2, 2, 2), np.uint32), 8, (12, 12, 12), "insert")  # an Informative entry drops the colour
    m.check(oracle, second, "Informative over Complex")
    assert (m.vis[12:14, 12:14, 12:14] == 0).all()


def test_clearing_the_last_data_only_voxel_unlinks_the_leaf(gpu, oracle, second):
    size, bd = 64, 4
    g = np.zeros((size,) * 3, np.uint32)
    d = np.zeros_like(g)
    d[40, 41, 42] = 3  # alone in its leaf
    g[0, 0, 0] = G.COLORS[0]
    gpu.build_dense(g, size, bd, data=d)
    before = gpu.download()
    assert before.desc.node_count == 3 and before.desc.brick_count == 2
    m = Model(gpu, size, bd)
    m.fill((42, 41, 40), (1, 1, 1), 0, 0)
    img = m.check(oracle, second, "the last data-only voxel cleared")
    assert gpu.orphans() == (1, 1)
    assert bin(int(img.node_ocbits[0])).count("1") == 1 and (img.node_children[:64] != EMPTY).sum() == 1


def test_a_write_past_the_last_data_value_is_refused(gpu):
    g, d = DG.distinct_data_grid(65535)
    gpu.build_dense(to_device(g), 64, 4, data=to_device(d))
    before = gpu.download()
    assert before.desc.data_count == 65535
    one = np.zeros((1, 1, 1), np.uint32)
    for call in (lambda: gpu.write_dense(one, (20, 20, 20), data=np.full((1, 1, 1), 1, np.uint32)),
                 lambda: gpu.fill_box((1, 2, 3), (4, 4, 4), int(G.COLORS[0]), 2),
                 lambda: gpu.write_dense(to_device(one), (63, 63, 63), "insert", data=to_device(one + np.uint32(5)))):
        with pytest.raises(N.VhxError) as e:
            call()
        assert e.value.code == N.VHX_E_CAPACITY
        G.assert_same_image(gpu.download(), before, "after the refused write")
    assert gpu.orphans() == (0, 0)
    gpu.fill_box((50, 50, 50), (2, 2, 2), 0, int(before.data_palette[65534]))  # an old value is fine
    assert gpu.tree_counts().data_count == 65535
    assert (gpu.get(F.lattice((50, 50, 50), (2, 2, 2))) == (0xFFFF | (65534 << 16))).all()


def test_no_data_is_write_dense(gpu):
    size, bd = 32, 2
    g, d = base_pair(size)
    rng = np.random.default_rng(8)
    origin, extents = odd_box(size)
    box = random_box(rng, extents)[0]
    other = vhx.Raytracer(0)
    try:
        for rt, data in ((gpu, None), (other, False)):
            rt.build_dense(g, size, bd, data=d)
            if data is None:
                import ctypes
                b = N.DenseIn(*origin, *extents, N.VHX_WRITE_REPLACE, 0, box.ctypes.data)
                assert N.lib().vhx_write_dense_data(rt._h, ctypes.byref(b), None, 0, 0) == N.VHX_OK
                rt.fill_box((0, 0, 0), (5, 5, 5), int(NEW_COLOURS[1]), 0)
            else:
                rt.write_dense(box, origin)
                rt.fill_box((0, 0, 0), (5, 5, 5), int(NEW_COLOURS[1]))
        G.assert_same_image(gpu.download(), other.download(), "data=None, fill_data=0 against write_dense")
        assert gpu.orphans() == other.orphans()
    finally:
        other.close()


# ------------------------------------------------------------------------------- compaction, simplification, palette
def edited_tree(rt, size, bd):
    g, d = base_pair(size)
    rt.build_dense(g, size, bd, data=d)
    m = Model(rt, size, bd)
    rng = np.random.default_rng(77)
    origin, extents = odd_box(size)
    m.write(*random_box(rng, extents), origin)
    m.fill((0, 0, 0), (size // 2,) * 3, int(G.COLORS[0]), 9)  # whole bricks and leaves of one value
    m.fill((size // 2, 0, 0), (size // 4,) * 3, 0, 0)
    m.write(*random_box(rng, (size, 5, 7), 0.2, new=False), (0, 1, 2), "insert", "tensor")
    return m


@pytest.mark.parametrize("size,bd", [(32, 2), (64, 4)])
def test_compact_simplify_and_compact_palette_keep_both_planes(gpu, oracle, second, size, bd):
    m = edited_tree(gpu, size, bd)
    m.check(oracle, second, "the edited tree")
    assert gpu.orphans()[1] > 0
    for name in ("compact", "simplify", "compact_palette"):
        getattr(gpu, name)()
        a, p = gpu.read_dense(data=True)
        assert np.array_equal(a, m.vis) and np.array_equal(p, m.dat), f"after {name}()"
    # the closure: simplify + compact_palette is the simplified build of the same voxels, up to the order of data_palette
    img = gpu.download()
    gpu.build_dense(m.vis, size, bd, simplify=True, data=m.dat)
    want = gpu.download()
    for k in ("node_type", "node_ocbits", "node_children", "color_palette"):
        assert np.array_equal(getattr(img, k), getattr(want, k)), k
    assert img.counts()["brick_count"] == want.counts()["brick_count"]
    assert img.counts()["solid_count"] == want.counts()["solid_count"]

    def resolved(image, values):
        values = np.asarray(values, np.uint32)
        return values & np.uint32(0xFFFF), DG.flat_data(image, np.where(values == EMPTY, EMPTY, values))

    for k in ("voxels", "solid_values"):
        (ca, da), (cb, db) = resolved(img, getattr(img, k)), resolved(want, getattr(want, k))
        assert np.array_equal(ca, cb) and np.array_equal(da, db), f"{k} with data halves resolved"
        none_a, none_b = (np.asarray(getattr(img, k)) >> 16) == 0xFFFF, (np.asarray(getattr(want, k)) >> 16) == 0xFFFF
        assert np.array_equal(none_a, none_b), f"{k}: data halves that are none"
    assert sorted(set(want.data_palette.tolist())) == sorted(set(np.unique(m.dat[m.dat != 0]).tolist()))
