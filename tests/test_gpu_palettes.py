"""vhx_compact_palettes on the GPU (Raytracer.compact_palettes): the colour half, the data half or both halves of the
resident tree rewritten in place so that color_palette and data_palette are the builders' palettes of the voxels the tree
holds now. The device image is held to the host's (TreeImage.palettes_compacted) and to the numpy model
(tests/_palettes_model.py); after edits with data, simplify() (compact()) and compact_palettes() leave the image of a
fresh simplified (plain) build with data in all seven arrays; a data_palette filled up by edits has room again; frames
change in `value` only, through both maps; refusals leave the tree as it was. Every comparison is bit for bit."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree, TreeImage
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests._compact_model import copy_image
from tests._palettes_model import model_palettes
from tests.test_compact import lod_image, malformed
from tests.test_gpu_compact import W, assert_derived_as_uploaded, bits, refused
from tests.test_palettes import KINDS, SIZES, blocky_pair, built, junk_image, scrambled

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
SOLID = N.VHX_SOLID_BIT
COLOR, DATA = N.VHX_PALETTE_COLOR, N.VHX_PALETTE_DATA
SIZE, BD = 64, 4
NEW_COLOURS = [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3), G.rgba(5, 5, 5)]


@pytest.fixture()
def rt():
    r = vhx.Raytracer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def second():
    r = vhx.Raytracer(0)
    yield r
    r.close()


def through(mapping, dmapping, values):
    v = np.asarray(values, np.uint32)
    return mapping[v & np.uint32(0xFFFF)] | (dmapping[v >> np.uint32(16)] << np.uint32(16))


# ---------------------------------------------------------------------------------------------- 1. scrambled uploads
@pytest.mark.parametrize("size,bd", SIZES)
@pytest.mark.parametrize("simplify", [False, True])
def test_scrambled_upload_comes_back(rt, size, bd, simplify):
    for kind in KINDS:
        if kind == "many" and size != 64:
            continue
        for scr in ("data", "both"):
            what = f"{kind} {size}/{bd} simplify={simplify} scrambled={scr}"
            base, mixed = scrambled(size, bd, kind, simplify, scr)
            rt.upload(mixed)
            held = rt.device_bytes()
            dropped = rt.compact_palettes()
            got = rt.download()
            G.assert_same_image(got, mixed.palettes_compacted(), f"{what}: against the host")
            G.assert_same_image(got, base, f"{what}: against the unscrambled build")
            if kind == "brick_noise" and scr == "both":
                G.assert_same_image(got, model_palettes(mixed)[0], f"{what}: against the model")
            assert dropped == (mixed.desc.color_count - base.desc.color_count,
                               mixed.desc.data_count - base.desc.data_count), what
            counts = rt.tree_counts()
            assert counts.color_count == base.desc.color_count and counts.data_count == base.desc.data_count, what
            assert rt.device_bytes() == held, what


@pytest.mark.parametrize("size,bd", SIZES)
def test_orphaned_slots_and_the_derived_layout(rt, second, size, bd):
    """Junk node and brick slots: their cells are translated and keep no value alive; headers and bitmaps are those of
    a context that uploaded the new image."""
    what = f"{size}/{bd}"
    base, junk, orphans, dead, live = junk_image(size, bd)
    rt.upload(junk)
    want, mapping, dmapping = model_palettes(junk)
    assert rt.compact_palettes() == (junk.desc.color_count - base.desc.color_count,
                                     junk.desc.data_count - base.desc.data_count)
    got = rt.download()
    G.assert_same_image(got, want, f"{what}: against the model")
    G.assert_same_image(got, junk.palettes_compacted(), f"{what}: against the host")
    cells = got.voxels.reshape(-1, bd ** 3)
    assert (cells[orphans[0]] == 0xFFFFFFFF).all() and (cells[orphans[1]] == (0xFFFF | int(dmapping[live]) << 16)).all()
    assert_derived_as_uploaded(rt, second, got, what)


# ------------------------------------------------------------------------------------------------ 2. the closing claim
def edited_tree(rt):
    """A data build, then every edit path that carries data, and a cleared box."""
    g, d = blocky_pair("brick_noise", SIZE, BD)
    rt.build_dense(g, SIZE, BD, data=d)
    rt.fill_box((0, 0, 0), (16, 16, 16), int(NEW_COLOURS[0]), 77)  # a leaf of one value in both halves
    rt.fill_box((16, 0, 0), (8, 8, 4), 0, 1234567)  # data only
    rt.fill_box((33, 5, 7), (9, 6, 5), int(NEW_COLOURS[2]), 31337)
    rt.fill_box((33, 5, 7), (9, 6, 5), int(NEW_COLOURS[2]), 77)  # buries 31337
    rng = np.random.default_rng(21)
    box = (rng.random((11, 18, 21)) < 0.6)
    alb = np.where(box & (rng.random(box.shape) < 0.7), NEW_COLOURS[1], 0).astype(np.uint32)
    dat = np.where(box & (rng.random(box.shape) < 0.7), rng.integers(1, 40, box.shape), 0).astype(np.uint32)
    rt.write_dense(alb, (3, 9, 40), data=dat)
    pts = rng.integers(0, SIZE, (500, 3)).astype(np.uint32)
    rt.set_voxels(pts, albedo=np.where(rng.random(500) < 0.5, G.COLORS[0], 0).astype(np.uint32),
                  data=rng.integers(0, 60, 500).astype(np.uint32))
    rt.fill_box((48, 48, 48), (16, 16, 16), 0)  # a cleared box


def edited_again(rt):
    """Editing goes on: colours and data values come and go again."""
    rng = np.random.default_rng(4)
    ids = rng.integers(1000, 2000, (11, 18, 21)).astype(np.uint32)
    rt.write_dense(np.full(ids.shape, G.rgba(9, 99, 199), np.uint32), (3, 9, 40), data=ids)
    rt.fill_box((20, 20, 20), (12, 12, 12), int(G.rgba(9, 99, 199)), 5555)
    rt.fill_box((40, 40, 40), (4, 4, 4), int(G.rgba(7, 7, 77)), 31337)
    rt.fill_box((40, 40, 40), (4, 4, 4), int(NEW_COLOURS[2]), 77)  # buries colour and value
    rt.set_voxels(np.array([[1, 2, 3], [60, 61, 62]], np.uint32), albedo=0, data=np.array([424242, 0], np.uint32))


@pytest.mark.parametrize("simplify", [True, False])
def test_edits_then_simplify_or_compact_then_palettes_is_a_fresh_build(rt, second, simplify):
    what = f"simplify={simplify}"
    edited_tree(rt)
    tidy = rt.simplify if simplify else rt.compact

    def round_trip(label):
        cube, plane = rt.read_dense(data=True)
        tidy()
        before = rt.download()
        dropped = rt.compact_palettes()
        got = rt.download()
        G.assert_same_image(got, FlatTree.from_dense(cube, SIZE, BD, simplify=simplify, data=plane),
                            f"{what}, {label}: a fresh build")
        G.assert_same_image(got, before.palettes_compacted(), f"{what}, {label}: against the host")
        assert dropped == (before.desc.color_count - got.desc.color_count, before.desc.data_count - got.desc.data_count)
        a, p = rt.read_dense(data=True)
        assert np.array_equal(a, cube) and np.array_equal(p, plane), f"{what}, {label}: read_dense"
        assert_derived_as_uploaded(rt, second, got, f"{what}, {label}")
        return dropped

    assert round_trip("edited")[1] >= 1
    edited_again(rt)
    colours, values = round_trip("edited again")
    assert colours >= 1 and values >= 1


# ------------------------------------------------------------------------------------------------------- 3. the cap
def test_a_full_data_palette_has_room_again(rt):
    n = 32 * 32 * 31
    colour = np.full((31, 32, 32), G.rgba(3, 2, 1), np.uint32)

    def ids(k):
        return (np.arange(n, dtype=np.uint32) + np.uint32(1 + k * n)).reshape(31, 32, 32)

    g = G.make_grid("corner", SIZE)
    rt.build_dense(g, SIZE, BD, data=np.where(g != 0, 0xABCDEF, 0).astype(np.uint32))
    rt.write_dense(colour, (16, 16, 16), data=ids(0))
    rt.write_dense(colour, (16, 16, 16), data=ids(1))  # buries the first
    before = rt.download()
    cube, plane = rt.read_dense(data=True)
    assert before.desc.data_count >= 2 * n
    with pytest.raises(N.VhxError) as e:
        rt.write_dense(colour, (16, 16, 16), data=ids(2))
    assert e.value.code == N.VHX_E_CAPACITY
    G.assert_same_image(rt.download(), before, "after VHX_E_CAPACITY")
    colours, values = rt.compact_palettes(color=False)
    assert colours == 0 and values >= n and rt.tree_counts().data_count == before.desc.data_count - values
    G.assert_same_image(rt.download(), before.palettes_compacted(color=False), "the full palette, compacted")
    a, p = rt.read_dense(data=True)
    assert np.array_equal(a, cube) and np.array_equal(p, plane)
    rt.write_dense(colour, (16, 16, 16), data=ids(2))
    plane[16:47, 16:48, 16:48] = ids(2)
    a, p = rt.read_dense(data=True)
    assert np.array_equal(a, cube) and np.array_equal(p, plane)


# --------------------------------------------------------------------------------------------------------- 4. frames
def test_frames_change_in_value_only(rt):
    edited_tree(rt)
    rt.simplify()
    rt.fill_box((16, 0, 0), (8, 8, 4), int(G.rgba(7, 7, 77)), 31337)
    rt.fill_box((16, 0, 0), (8, 8, 4), int(NEW_COLOURS[0]), 77)  # buries them
    sh = rt.shared()
    try:
        cam = vhx.glass_camera(SIZE, W, W, target=(SIZE / 2,) * 3)
        old = rt.download()
        frames = [bits(rt.trace_primary(cam)), bits(sh.trace_primary(cam))]
        colours, values = rt.compact_palettes()
        assert colours > 0 and values > 0
        assert rt.sync() > 0.0, "the device time of the rewrite pass"
        new = rt.download()
        want, mapping, dmapping = model_palettes(old)
        G.assert_same_image(new, want, "against the model")
        used = np.flatnonzero(dmapping[:old.desc.data_count] != 0xFFFF)
        assert np.array_equal(new.data_palette[dmapping[used]], old.data_palette[used]), "the data map between the downloads"
        hit = frames[0]["value"] != EMPTY
        assert hit.any() and (frames[0]["value"][hit] >> 16 != 0xFFFF).any(), "the frame sees data values"
        assert not np.array_equal(through(mapping, dmapping, frames[0]["value"]) >> 16, frames[0]["value"] >> 16)
        for name, ctx, frame in (("owner", rt, frames[0]), ("shared", sh, frames[1])):
            after = bits(ctx.trace_primary(cam))
            for k, v in frame.items():
                assert np.array_equal(after[k], through(mapping, dmapping, v) if k == "value" else v), f"{name}: {k}"
    finally:
        sh.close()


# --------------------------------------------------------------------------------------------- 5. selection of halves
@pytest.mark.parametrize("size,bd", SIZES)
def test_selection_of_halves(rt, second, size, bd):
    what = f"{size}/{bd}"
    base, junk, orphans, dead, live = junk_image(size, bd)
    second.upload(junk)
    old_dropped = second.compact_palette()
    rt.upload(junk)
    assert rt.compact_palettes(data=False) == (old_dropped, 0)
    col = rt.download()
    G.assert_same_image(col, second.download(), f"{what}: which = COLOR against compact_palette()")
    G.assert_same_image(col, junk.palettes_compacted(data=False), f"{what}: which = COLOR against the host")
    rt.upload(junk)
    colours, values = rt.compact_palettes(color=False)
    assert colours == 0 and values == junk.desc.data_count - base.desc.data_count
    dat = rt.download()
    G.assert_same_image(dat, junk.palettes_compacted(color=False), f"{what}: which = DATA against the host")
    assert np.array_equal(dat.color_palette, junk.color_palette), f"{what}: color_palette"
    assert np.array_equal(dat.voxels & 0xFFFF, junk.voxels & 0xFFFF), f"{what}: colour halves of the cells"
    assert np.array_equal(dat.solid_values & 0xFFFF, junk.solid_values & 0xFFFF), f"{what}: colour halves of the solids"
    rt.compact_palettes(data=False)  # one half after the other is both at once
    G.assert_same_image(rt.download(), junk.palettes_compacted(), f"{what}: data, then colour")


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_tree_as_it_was(rt):
    assert N.lib().vhx_compact_palettes(rt._h, 3, None, None) == N.VHX_E_STATE  # before any upload
    assert N.lib().vhx_compact_palettes(None, 3, None, None) == N.VHX_E_INVALID_ARG
    edited_tree(rt)
    before = rt.download()
    for which in (0, 4):
        assert N.lib().vhx_compact_palettes(rt._h, which, None, None) == N.VHX_E_INVALID_ARG
        G.assert_same_image(rt.download(), before, f"after which = {which}")
    assert N.lib().vhx_compact_palettes(rt._h, 3, None, None) == N.VHX_OK  # both out-pointers may be null
    before = rt.download()
    sh = rt.shared()
    refused(sh.compact_palettes)
    sh.close()
    G.assert_same_image(rt.download(), before, "after the refusal on a shared context")

    flat = lod_image(64, 4, 0)
    rt.upload(flat)
    rt.set_node_mips(flat.node_mips)
    before = rt.download()
    refused(rt.compact_palettes)
    G.assert_same_image(rt.download(), before, "after the refusal under node MIPs")
    rt.set_node_mips(None)

    for kind, word in (("node with two parents", "twice"), ("brick referenced twice", "twice"),
                       ("child at node_count", "index"), ("brick at brick_count", "index")):
        img = malformed(kind)
        rt.upload(img)
        assert word in str(refused(rt.compact_palettes)), kind
        assert word in str(refused(lambda: rt.compact_palettes(color=False))), kind
        G.assert_same_image(rt.download(), img, f"after the refusal of {kind}")

    img = copy_image(built(64, 4, "brick_noise", True))
    sel = np.flatnonzero((img.node_children != EMPTY) & ((img.node_children & SOLID) != 0) &
                         np.repeat(img.node_type == N.VHX_NODE_LEAF, 64))
    img.node_children[sel[0]] = SOLID | img.desc.solid_count
    rt.upload(img)
    assert "index" in str(refused(rt.compact_palettes))
    G.assert_same_image(rt.download(), img, "after the refusal of a Solid index at solid_count")

    deep = built(16, 4, "sparse", False)
    small = TreeImage(8, 4, {k: np.array(getattr(deep, k)) for k in G.ARRAYS})  # a cell would be half a voxel
    rt.upload(small)
    assert "smaller than a voxel" in str(refused(lambda: rt.compact_palettes(color=False)))
    G.assert_same_image(rt.download(), small, "after the refusal of a leaf below the voxel lattice")


# --------------------------------------------------------------------------------------- 7. fixed point, empty cases
@pytest.mark.parametrize("simplify", [False, True])
def test_fresh_build_is_a_fixed_point(rt, simplify):
    g, d = blocky_pair("brick_noise", SIZE, BD)
    rt.build_dense(g, SIZE, BD, simplify=simplify, data=d)
    before = rt.download()
    assert rt.compact_palettes() == (0, 0)
    G.assert_same_image(rt.download(), before, f"simplify={simplify}")
    assert rt.compact_palettes() == (0, 0)
    G.assert_same_image(rt.download(), before, f"simplify={simplify}: twice")


def test_empty_tree(rt):
    zero = FlatTree.from_dense(G.make_grid("zero", SIZE), SIZE, BD)
    rt.upload(zero)
    assert rt.compact_palettes() == (0, 0)
    g, d = blocky_pair("brick_noise", SIZE, BD)
    rt.build_dense(g, SIZE, BD, data=d)
    rt.fill_box((0, 0, 0), (SIZE,) * 3, 0)
    before = rt.download()
    assert rt.compact_palettes() == (before.desc.color_count, before.desc.data_count)
    G.assert_same_image(rt.download(), before.palettes_compacted(), "all cleared")
    counts = rt.tree_counts()
    assert counts.color_count == 0 and counts.data_count == 0
    rng = np.random.default_rng(8)
    alb = np.where(rng.random((35, 18, 22)) < 0.5, NEW_COLOURS[0], 0).astype(np.uint32)
    ids = np.where(rng.random((35, 18, 22)) < 0.5, rng.integers(1, 99, (35, 18, 22)), 0).astype(np.uint32)
    rt.write_dense(alb, (13, 15, 3), data=ids)
    cube, plane = rt.read_dense(data=True)
    rt.compact()
    rt.compact_palettes()
    G.assert_same_image(rt.download(), FlatTree.from_dense(cube, SIZE, BD, data=plane), "written again")
