"""vhx_write_dense on the GPU: a box of the device tree replaced in place. The expected cube G' is kept in numpy beside
every write (the visible colours, and what get returns by the call's contract); after a write the device's read_dense,
get at every position, structure (tests/_treecheck.py), frame and derived state are checked against it, against the
oracle on the downloaded image and, on plain bases, against the oracle on the host builder's image of G'. Every
comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._treecheck import check_tree

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
W = 64
NEW = [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3), G.rgba(5, 5, 5)]  # colours no base grid holds
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def visible(grid, size):
    out = np.zeros((size, size, size), np.uint32)
    gz, gy, gx = grid.shape
    out[:gz, :gy, :gx] = np.where(grid >> 24 != 0, grid, 0)
    return out


def positions(size):
    return cached(("lattice", size), lambda: F.lattice((0, 0, 0), (size,) * 3))


def bits(frame):
    return {k: np.ascontiguousarray(v).view(np.uint32) for k, v in frame.items()}


def assert_same_frame(got, want, what, fields=None):
    got, want = bits(got), bits(want)
    for k in fields or want:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.count_nonzero(got[k] != want[k])} entries"


def assert_same_download(a, b, what):
    G.assert_same_image(a, b, what)


@pytest.fixture(scope="module")
def second():
    """A second context that uploads downloaded images: the derived state as an upload derives it."""
    rt = vhx.Raytracer(0)
    yield rt
    rt.close()


def random_box_grid(rng, extents, density=0.4, new=True):
    gx, gy, gz = extents
    colours = np.concatenate([G.COLORS, np.array(NEW if new else [], np.uint32)])
    g = np.zeros((gz, gy, gx), np.uint32)
    mask = rng.random(g.shape) < density
    g[mask] = colours[rng.integers(0, len(colours), int(mask.sum()))]
    return g


class Model:
    """The expected cube beside a Raytracer: `vis` what read_dense gives, `val` what get gives."""

    def __init__(self, rt, size, bd, plain=True):
        self.rt, self.size, self.bd, self.plain = rt, size, bd, plain
        self.vis = rt.read_dense()
        self.val = rt.get(positions(size)).reshape(size, size, size)

    def expect(self, grid, origin, mode):
        """G -> G' for a write the device has just done (the palette indices come from its new palette)."""
        ox, oy, oz = origin
        gz, gy, gx = grid.shape
        g = np.where(grid >> 24 != 0, grid, 0).astype(np.uint32)
        covered = np.ones(g.shape, bool) if mode == "replace" else g != 0
        pal = self.rt.read_range(N.VHX_BUF_COLOR_PALETTE, 0, self.rt.tree_counts().color_count)
        uniq, first = np.unique(pal, return_index=True)  # a colour's lowest index
        at = np.searchsorted(uniq, g[g != 0])
        assert (uniq[np.minimum(at, uniq.size - 1)] == g[g != 0]).all(), "a written colour is not in the palette"
        value = np.full(g.shape, EMPTY, np.uint32)
        value[g != 0] = first[at].astype(np.uint32) | np.uint32(0xFFFF0000)
        sl = (slice(oz, oz + gz), slice(oy, oy + gy), slice(ox, ox + gx))
        self.vis[sl] = np.where(covered, g, self.vis[sl])
        self.val[sl] = np.where(covered, value, self.val[sl])

    def write(self, grid, origin=(0, 0, 0), mode="replace", source="host"):
        self.rt.write_dense(to_device(grid) if source == "tensor" else grid, origin, mode)
        self.expect(grid, origin, mode)

    def fill(self, origin, extents, albedo):
        self.rt.fill_box(origin, extents, albedo)
        gx, gy, gz = extents
        self.expect(np.full((gz, gy, gx), albedo, np.uint32), origin, "replace")

    def check(self, oracle, second, what, walker=True):
        rt, size, bd = self.rt, self.size, self.bd
        img = rt.download()
        assert np.array_equal(rt.read_dense(), self.vis), f"{what}: read_dense"
        pos = positions(size)
        got = rt.get(pos)
        assert np.array_equal(got, self.val.ravel()), \
            f"{what}: get differs from the contract at {pos[np.flatnonzero(got != self.val.ravel())[:4]].tolist()}"
        if walker:
            assert np.array_equal(got, F.flat_get(img, pos)), f"{what}: get differs from the walker on the download"
        check_tree(img, rt.orphans(), what)
        cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
        frame = rt.trace_primary(cam)
        assert_same_frame(frame, oracle.trace_primary(img, cam, 0, 0, W, W), f"{what}: frame against the download")
        if self.plain:
            host = FlatTree.from_dense(self.vis, size, bd)
            want = oracle.trace_primary(host, cam, 0, 0, W, W)
            hit = want["value"] != EMPTY
            assert np.array_equal(frame["value"] != EMPTY, hit), f"{what}: hit mask against the image of G'"
            assert_same_frame(frame, want, f"{what}: frame against the image of G'",
                              ("cell", "voxel", "impact", "normal", "depth", "rgba"))
            a = img.color_palette[frame["value"][hit] & 0xFFFF]
            b = np.asarray(host.color_palette)[want["value"][hit] & 0xFFFF]
            assert np.array_equal(a, b) and ((frame["value"][hit] >> 16) == 0xFFFF).all(), f"{what}: hit colours"
        second.upload(img)
        d = img.desc
        words = max(1, bd ** 3 // 64)
        assert np.array_equal(rt.read_derived(N.VHX_DERIVED_NODE_HDR, 0, d.node_count),
                              second.read_derived(N.VHX_DERIVED_NODE_HDR, 0, d.node_count)), f"{what}: node headers"
        if d.brick_count:
            assert np.array_equal(rt.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, d.brick_count * words),
                                  second.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, d.brick_count * words)), \
                f"{what}: brick bitmaps"
        return img


def odd_box(size):
    """Off the brick grid, across brick, leaf and internal-node boundaries: (13, 15, 3) + (22, 18, 35) at 64."""
    origin = (size * 13 // 64, size * 15 // 64, size * 3 // 64)
    extents = (max(1, size * 22 // 64), max(1, size * 18 // 64), max(1, size * 35 // 64))
    return origin, extents


# --------------------------------------------------------------------------------------- sizes, boxes and sources
SIZES = [(4, 1), (16, 4), (32, 8), (64, 16), (16, 1), (32, 2), (64, 4), (256, 4)]


@pytest.mark.parametrize("size,bd,source", [(s, b, src) for s, b in SIZES[:-1] for src in ("host", "tensor")] +
                         [(256, 4, "tensor")])
def test_unaligned_boxes_into_a_sparse_base(gpu, oracle, second, size, bd, source):
    what = f"{size}/{bd} {source}"
    base = cached(("sparse", size), lambda: G.make_grid("sparse", size))
    gpu.build_dense(base, size, bd)
    m = Model(gpu, size, bd)
    assert np.array_equal(m.vis, visible(base, size)), what
    rng = np.random.default_rng(size * 10 + bd)
    origin, extents = odd_box(size)
    if size == 256:
        assert origin[0] < 64 < origin[0] + extents[0] and origin[2] < 128 < origin[2] + extents[2]
    before = gpu.tree_counts()
    m.write(random_box_grid(rng, extents), origin, "replace", source)
    after = gpu.tree_counts()
    assert before.color_count < after.color_count <= before.color_count + len(NEW) or np.prod(extents) < 40, what
    assert after.brick_count >= before.brick_count and after.node_count >= before.node_count
    m.check(oracle, second, f"{what}: box", walker=size < 256)
    one = (size // 3, size // 4, size // 2)
    m.write(np.full((1, 1, 1), NEW[2], np.uint32), one, "replace", source)
    assert m.val[one[2], one[1], one[0]] != EMPTY
    if size < 256:
        m.check(oracle, second, f"{what}: one voxel")
    m.write(random_box_grid(rng, (size,) * 3, 0.2), (0, 0, 0), "replace", source)
    m.check(oracle, second, f"{what}: whole cube", walker=size < 256)


@pytest.mark.parametrize("size,bd", SIZES[:-1])
def test_into_an_empty_tree(gpu, oracle, second, size, bd):
    what = f"{size}/{bd}"
    gpu.build_dense(G.make_grid("zero", size), size, bd)
    assert gpu.download().node_type.tolist() == [N.VHX_NODE_NOTHING]
    m = Model(gpu, size, bd)
    m.write(cached(("sparse", size), lambda: G.make_grid("sparse", size)))
    img = m.check(oracle, second, f"{what}: the sparse grid into the empty tree")
    assert img.node_type[0] == (N.VHX_NODE_LEAF if size == 4 * bd else N.VHX_NODE_INTERNAL)
    assert gpu.orphans() == (0, 0)
    m.write(G.make_grid("corner", size)[-1:, -1:, -1:], (size - 1,) * 3)
    m.check(oracle, second, f"{what}: the far corner")


# ------------------------------------------------------------------------------------------------------- clearing
@pytest.mark.parametrize("size", [64, 256])
def test_clearing_unlinks_bricks_leaves_and_nodes(gpu, oracle, second, size):
    bd = 4
    base = cached(("sparse", size), lambda: G.make_grid("sparse", size))
    gpu.build_dense(to_device(base), size, bd)
    m = Model(gpu, size, bd)
    # whole bricks and whole leaves (edge 16) inside (3, 5, 2) + (41, 38, 33); at 256 the level-1 node [0, 64)^3 too
    origin, extents = ((0, 0, 0), (70, 67, 69)) if size == 256 else ((3, 5, 2), (41, 38, 33))
    m.write(np.zeros(extents[::-1], np.uint32), origin)
    nodes, bricks = gpu.orphans()
    assert bricks >= 8 and nodes >= (1 + 64 if size == 256 else 1), (nodes, bricks)
    img = m.check(oracle, second, f"{size}: cleared region", walker=size < 256)
    if size == 256:
        assert img.node_children[0] == EMPTY and (int(img.node_ocbits[0]) & 1) == 0, "the level-1 node left the root"
    m.fill((0, 0, 0), (size,) * 3, 0)
    img = m.check(oracle, second, f"{size}: everything cleared", walker=size < 256)
    assert img.node_type[0] == N.VHX_NODE_NOTHING and not m.vis.any()
    cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
    assert (gpu.trace_primary(cam)["value"] == EMPTY).all(), "all sky"
    assert gpu.orphans()[0] == img.desc.node_count - 1
    origin, extents = odd_box(size)
    m.write(random_box_grid(np.random.default_rng(size), extents), origin)
    m.check(oracle, second, f"{size}: written again", walker=size < 256)


# ----------------------------------------------------------------------------------------------- simplified bases
@pytest.mark.parametrize("size,bd", [(64, 4), (32, 2), (32, 8), (16, 1)])
@pytest.mark.parametrize("kind", ["full", "brick_noise", "blocks4", "cut"])
def test_simplified_bases(gpu, oracle, second, kind, size, bd):
    what = f"{kind} {size}/{bd}"
    base = SG.make_grid(kind, size, bd)
    gpu.build_dense(base, size, bd, simplify=True)
    old = gpu.download()
    SG.assert_case(kind, size, bd, old)
    m = Model(gpu, size, bd, plain=False)
    assert np.array_equal(m.vis, visible(base, size)), what
    rng = np.random.default_rng(size + bd)
    leaf = 4 * bd
    # part of brick 0 of the first leaf, on into the next leaf in z; and a box at the far end, off the grid on every side
    boxes = [((1, 0, bd // 2), (bd, 2 * bd, min(size - bd // 2, leaf + 1))),
             ((size - min(size, leaf + 3), size - 3, size - bd - 1), (min(size, leaf + 3) - 1, 2, bd))]
    touched = 0
    for k, (origin, extents) in enumerate(boxes):
        m.write(random_box_grid(rng, extents, 0.5), origin, "replace" if k == 0 else "insert")
        img = m.check(oracle, second, f"{what}: box {k}")
        touched += int(np.prod([(o + e - 1) // bd - o // bd + 1 for o, e in zip(origin, extents)]))
    assert np.array_equal(img.solid_values, old.solid_values), f"{what}: solid_values changed"
    assert not (img.node_type[:old.desc.node_count][old.node_type == N.VHX_NODE_LEAF] == N.VHX_NODE_UNIFORM_LEAF).any()
    n = old.desc.node_count
    was_leaf = old.node_type == N.VHX_NODE_LEAF
    och, nch = old.node_children.reshape(-1, 64)[was_leaf], img.node_children.reshape(-1, 64)[:n][was_leaf]
    solid = (och != EMPTY) & ((och & N.VHX_SOLID_BIT) != 0)
    assert int((solid & (och != nch)).sum()) <= touched, f"{what}: Solid entries outside the boxes changed"
    uni = np.flatnonzero(old.node_type == N.VHX_NODE_UNIFORM_LEAF)
    if uni.size and kind != "brick_noise":  # an expanded UniformLeaf keeps its index; one with a Solid brick hands it to its untouched bricks
        grown = uni[img.node_type[uni] == N.VHX_NODE_LEAF]
        assert grown.size >= 1, f"{what}: no UniformLeaf under the boxes"
        for node in grown[:4]:
            u = old.node_children[node * 64]
            if u & N.VHX_SOLID_BIT:
                assert (img.node_children[node * 64:node * 64 + 64] == u).sum() >= 64 - touched
    assert img.desc.brick_count > old.desc.brick_count


# ---------------------------------------------------------------------------------------------------- the palette
def test_new_colours_follow_the_palette_in_insert_order(gpu, oracle, second):
    base = G.make_grid("sparse", 16)
    gpu.build_dense(base, 16, 4)
    pal = gpu.download().color_palette.tolist()
    grid, order = G.palette_order_grid()  # A at (1, 0, 0), B at (0, 0, 1): the insert loop meets B first
    grid[2, 3, 3] = pal[1]  # an old colour, last in every order
    m = Model(gpu, 16, 4)
    m.write(grid, (5, 6, 7))
    img = m.check(oracle, second, "palette order")
    assert img.color_palette.tolist() == pal + [int(c) for c in order]
    assert m.val[7 + 2, 6 + 3, 5 + 3] == (0xFFFF0000 | 1)
    m.write(grid[::-1].copy(), (1, 1, 1), "insert", "tensor")  # nothing new: the palette stays
    assert m.check(oracle, second, "palette reuse").color_palette.tolist() == pal + [int(c) for c in order]


def test_a_write_past_the_last_colour_is_refused(gpu, oracle):
    gpu.build_dense(to_device(G.distinct_colors_grid(65535)), 64, 4)
    before = gpu.download()
    assert before.desc.color_count == 65535
    cam = vhx.glass_camera(64, W, W, target=(32.0,) * 3)
    frame = gpu.trace_primary(cam)
    for grid in (np.full((1, 1, 1), G.rgba(1, 2, 3, 4), np.uint32), to_device(G.distinct_colors_grid(300) ^ np.uint32(0x01000000))):
        with pytest.raises(N.VhxError) as e:
            gpu.write_dense(grid, (20, 20, 20))
        assert e.value.code == N.VHX_E_CAPACITY
        assert_same_download(gpu.download(), before, "after the refused write")
        assert_same_frame(gpu.trace_primary(cam), frame, "after the refused write")
    assert gpu.orphans() == (0, 0)
    gpu.write_dense(np.full((2, 2, 2), before.color_palette[65534], np.uint32), (50, 50, 50))  # an old colour is fine
    assert gpu.tree_counts().color_count == 65535
    assert (gpu.get(F.lattice((50, 50, 50), (2, 2, 2))) == (0xFFFF0000 | 65534)).all()


# ------------------------------------------------------------------------------------------ insert mode and fills
def test_insert_mode_and_fills(gpu, oracle, second):
    size, bd = 32, 2
    gpu.build_dense(G.make_grid("sparse", size), size, bd)
    m = Model(gpu, size, bd)
    grid = random_box_grid(np.random.default_rng(5), (20, 9, 13), 0.3)
    kept = m.val[4:17, 11:20, 3:23].copy()
    m.write(grid, (3, 11, 4), "insert")
    assert np.array_equal(m.val[4:17, 11:20, 3:23][grid >> 24 == 0], kept[grid >> 24 == 0])
    m.check(oracle, second, "insert")
    m.fill((7, 0, 9), (11, 32, 6), NEW[1])
    m.check(oracle, second, "fill with a colour")
    m.fill((1, 5, 0), (30, 9, 31), 0)
    m.check(oracle, second, "fill with 0")
    assert gpu.orphans()[1] > 0


# ----------------------------------------------------------------------------------------------------------- fuzz
def fuzz_run(rt, oracle, second):
    size, bd = 64, 4
    rng = np.random.default_rng(2026)
    rt.build_dense(G.make_grid("sparse", size, seed=9), size, bd)
    m = Model(rt, size, bd)
    for k in range(12):
        lo = rng.integers(0, size, 3)
        ext = np.minimum(rng.integers(1, 40, 3), size - lo)
        origin, extents = tuple(int(v) for v in lo), tuple(int(v) for v in ext)
        kind = k % 4
        if kind == 3:
            m.fill(origin, extents, int(rng.choice([0, int(NEW[0]), int(G.COLORS[1])])))
        else:
            grid = random_box_grid(rng, extents, [0.0, 0.5, 0.9][kind] if k < 8 else 0.3, new=k % 2 == 0)
            m.write(grid, origin, "insert" if k % 3 == 1 else "replace", "tensor" if k % 2 else "host")
        if oracle is not None:
            m.check(oracle, second, f"fuzz write {k}: {origin} + {extents}")
    return rt.download(), rt.orphans()


def test_fuzz_and_scheduling_independence(gpu, oracle, second):
    first, orphans = fuzz_run(gpu, oracle, second)
    other = vhx.Raytracer(0)
    try:
        again, orphans2 = fuzz_run(other, None, None)
    finally:
        other.close()
    assert_same_download(again, first, "the same writes on a second context")
    assert orphans == orphans2 and orphans[1] > 0


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
        owner.write_dense(to_device(random_box_grid(np.random.default_rng(1), (30, 30, 30))), (10, 20, 30))
        after = sh.trace_primary(cam)  # no synchronisation in between
        new = owner.download()
        assert_same_frame(before, oracle.trace_primary(old, cam, 0, 0, W, W), "the frame before the write")
        assert_same_frame(after, oracle.trace_primary(new, cam, 0, 0, W, W), "the shared context after the write")
        assert not np.array_equal(before["value"], after["value"])
        for call in (lambda: sh.write_dense(np.zeros((2, 2, 2), np.uint32), (1, 1, 1)),
                     lambda: sh.fill_box((0, 0, 0), (4, 4, 4), int(NEW[0]))):
            with pytest.raises(N.VhxError) as e:
                call()
            assert e.value.code == N.VHX_E_STATE
        assert_same_download(owner.download(), new, "after the refused write on the shared context")
        assert np.array_equal(sh.read_dense(), owner.read_dense())
        sh.close()
    finally:
        owner.close()


# ------------------------------------------------------------------------------------------------------- refusals
def lod_tree(size):
    tree = BoxTree(size, 4)
    tree.insert_scene(N.VHX_SCENE_LATTICE_CUBE)
    tree.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
    return tree


def test_refusals_leave_the_tree_as_it_was():
    rt = vhx.Raytracer(0)
    grid = np.full((3, 3, 3), NEW[0], np.uint32)
    try:
        assert ctypes.sizeof(N.DenseIn) == 40  # vhx_dense_in: eight u32 and a pointer
        box = N.DenseIn(0, 0, 0, 1, 1, 1, 0, 0, grid.ctypes.data)
        assert N.lib().vhx_write_dense(rt._h, ctypes.byref(box), 0) == N.VHX_E_STATE  # before any upload
        nodes, bricks = ctypes.c_uint32(), ctypes.c_uint32()
        assert N.lib().vhx_tree_orphans(rt._h, ctypes.byref(nodes), ctypes.byref(bricks)) == N.VHX_E_STATE
        tree = lod_tree(64)
        for flat, mips, code in ((tree.flatten_lod(0), False, N.VHX_E_STATE), (tree.flatten_lod(1), True, N.VHX_E_STATE)):
            rt.upload(flat)
            if mips:
                rt.set_node_mips(flat.node_mips)
            before = rt.download()
            for call in (lambda: rt.write_dense(grid, (30, 30, 30)), lambda: rt.fill_box((0, 0, 0), (64, 64, 64), 0)):
                with pytest.raises(N.VhxError) as e:
                    call()
                assert e.value.code == code
            assert_same_download(rt.download(), before, "after a refused write")
            if mips:
                rt.set_node_mips(None)
                rt.write_dense(grid, (30, 30, 30))  # the full-depth view without MIPs takes the write
                assert (rt.read_dense((30, 30, 30), (3, 3, 3)) == NEW[0]).all()
        rt.build_dense(G.make_grid("sparse", 64), 64, 4)
        before = rt.download()
        assert N.lib().vhx_write_dense(rt._h, None, 0) == N.VHX_E_INVALID_ARG
        for origin, mode in (((62, 0, 0), "replace"), ((0, 64, 0), "replace"), ((0, 0, 0xFFFFFFFF), "insert"),
                             ((0, 0, 0), 2)):
            with pytest.raises(N.VhxError) as e:
                rt.write_dense(grid, origin, mode)
            assert e.value.code == N.VHX_E_INVALID_ARG
        with pytest.raises(N.VhxError) as e:
            rt.fill_box((0, 0, 0), (0, 1, 1), 0)
        assert e.value.code == N.VHX_E_INVALID_ARG
        assert_same_download(rt.download(), before, "after invalid arguments")
        assert rt.orphans() == (0, 0)
    finally:
        rt.close()


# ---------------------------------------------------------------------------------------- a rebuild between writes
def test_writes_and_builds_in_sequence(oracle, second):
    rt = vhx.Raytracer(0)
    try:
        rt.build_dense(G.make_grid("sparse", 64, seed=1), 64, 4)
        held = rt.device_bytes()
        m = Model(rt, 64, 4)
        m.fill((0, 0, 0), (40, 64, 64), 0)
        m.write(random_box_grid(np.random.default_rng(3), (64, 20, 64), 0.6), (0, 30, 0))
        m.check(oracle, second, "write after the first build")
        assert rt.orphans()[0] > 0 and rt.orphans()[1] > 0 and rt.device_bytes() > held
        small = G.make_grid("sparse", 32, seed=2)
        rt.build_dense(small, 32, 2)
        assert rt.orphans() == (0, 0)
        G.assert_same_image(rt.download(), FlatTree.from_dense(small, 32, 2), "the smaller build")
        m = Model(rt, 32, 2)
        m.write(random_box_grid(np.random.default_rng(4), (9, 30, 17)), (20, 1, 6))
        m.check(oracle, second, "write after the smaller build")
    finally:
        rt.close()
