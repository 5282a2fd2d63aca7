"""vhx_compact_palette on the GPU (Raytracer.compact_palette): the colour half of the resident tree rewritten in place so
that color_palette is the builders' palette of the voxels the tree holds now. The device image is held to the host's
(TreeImage.palette_compacted) and to the numpy model (tests/_palette_model.py); after edits, simplify() (compact()) and
compact_palette() leave the image of a fresh simplified (plain) build, in all seven arrays; a palette filled up by edits
has room again; frames change in `value` only, through the map; refusals leave the tree as it was. Every comparison is
bit for bit."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree, TreeImage
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _simplify_grids as SG
from tests._compact_model import copy_image
from tests._palette_model import model_palette
from tests.test_compact import lod_image, malformed
from tests.test_flat_simplify import images
from tests.test_gpu_compact import (W, assert_derived_as_uploaded, assert_same_frame, bits, camera, positions,
                                    random_box_grid, refused)
from tests.test_gpu_simplify import COLOURS, edited_tree
from tests.test_palette import KINDS, SIZES, junk_image, scrambled

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
SOLID = N.VHX_SOLID_BIT
SIZE, BD = 64, 4


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


def through(mapping, values):
    v = np.asarray(values, np.uint32)
    return (v & np.uint32(0xFFFF0000)) | mapping[v & np.uint32(0xFFFF)]


# ---------------------------------------------------------------------------------------------- 1. scrambled uploads
@pytest.mark.parametrize("size,bd", SIZES)
@pytest.mark.parametrize("simplify", [False, True])
def test_scrambled_upload_comes_back(rt, size, bd, simplify):
    for kind in KINDS:
        what = f"{kind} {size}/{bd} simplify={simplify}"
        base, mixed = scrambled(size, bd, kind, simplify)
        rt.upload(mixed)
        held = rt.device_bytes()
        dropped = rt.compact_palette()
        got = rt.download()
        G.assert_same_image(got, mixed.palette_compacted(), f"{what}: against the host")
        G.assert_same_image(got, model_palette(mixed)[0], f"{what}: against the model")
        G.assert_same_image(got, base, f"{what}: against the unscrambled build")
        assert dropped == mixed.desc.color_count - base.desc.color_count, what
        assert rt.tree_counts().color_count == base.desc.color_count and rt.device_bytes() == held, what


# ------------------------------------------------------------------------- 2. orphaned slots and the derived layout
@pytest.mark.parametrize("size,bd", SIZES)
def test_orphaned_slots_and_the_derived_layout(rt, second, size, bd):
    """Junk node and brick slots: their cells are translated and keep no colour alive; headers, bitmaps, every get and
    a frame are those of a context that uploaded the new image."""
    what = f"{size}/{bd}"
    base, junk, orphans, dead, live = junk_image(size, bd)
    rt.upload(junk)
    pos, cam = positions(size), camera(size)
    values, frame = rt.get(pos), rt.trace_primary(cam)
    want, mapping = model_palette(junk)
    assert rt.compact_palette() == junk.desc.color_count - base.desc.color_count
    got = rt.download()
    G.assert_same_image(got, want, f"{what}: against the model")
    G.assert_same_image(got, junk.palette_compacted(), f"{what}: against the host")
    cells = got.voxels.reshape(-1, bd ** 3)
    assert (cells[orphans[0]] == 0xFFFFFFFF).all() and (cells[orphans[1]] == (0x00070000 | mapping[live])).all()
    assert_derived_as_uploaded(rt, second, got, what)
    after, twin = rt.trace_primary(cam), second.trace_primary(cam)
    assert_same_frame(after, twin, f"{what}: frame against a fresh upload")
    assert np.array_equal(rt.get(pos), second.get(pos)), f"{what}: get against a fresh upload"
    assert np.array_equal(rt.get(pos), through(mapping, values)), f"{what}: get through the map"
    for k, v in bits(frame).items():
        assert np.array_equal(bits(after)[k], through(mapping, v) if k == "value" else v), f"{what}: {k}"


# ------------------------------------------------------------------------------------------------ 3. the closing claim
def plain_edited_tree(rt):
    """test_gpu_simplify.edited_tree on a plain build."""
    rt.build_dense(SG.make_grid("brick_noise", SIZE, BD), SIZE, BD)
    rt.fill_box((0, 0, 0), (16, 16, 16), int(COLOURS[0]))
    rt.fill_box((16, 0, 0), (8, 8, 4), int(COLOURS[1]))
    rt.fill_box((33, 5, 7), (9, 6, 5), int(COLOURS[2]))
    rt.write_dense(np.ascontiguousarray(SG.make_grid("blocks4", SIZE, BD)[16:32, 0:16, 0:16]), (16, 16, 16))
    rt.fill_box((48, 48, 48), (16, 16, 16), 0)


@pytest.mark.parametrize("simplify", [True, False])
def test_edits_then_simplify_or_compact_then_palette_is_a_fresh_build(rt, second, simplify):
    what = f"simplify={simplify}"
    (edited_tree if simplify else plain_edited_tree)(rt)
    tidy = rt.simplify if simplify else rt.compact

    def round_trip(label):
        cube = rt.read_dense()
        tidy()
        before = rt.download()
        dropped = rt.compact_palette()
        got = rt.download()
        G.assert_same_image(got, FlatTree.from_dense(cube, SIZE, BD, simplify=simplify), f"{what}, {label}: a fresh build")
        G.assert_same_image(got, before.palette_compacted(), f"{what}, {label}: against the host")
        assert dropped == before.desc.color_count - got.desc.color_count
        assert np.array_equal(rt.read_dense(), cube), f"{what}, {label}: read_dense"
        assert_derived_as_uploaded(rt, second, got, f"{what}, {label}")
        return dropped

    round_trip("edited")
    # editing goes on: colours come and go again
    rt.write_dense(random_box_grid(np.random.default_rng(4), (21, 18, 11)), (3, 9, 40))
    rt.fill_box((20, 20, 20), (12, 12, 12), int(G.rgba(9, 99, 199)))
    rt.fill_box((40, 40, 40), (4, 4, 4), int(G.rgba(7, 7, 77)))
    rt.fill_box((40, 40, 40), (4, 4, 4), int(COLOURS[2]))  # buries it
    assert round_trip("edited again") >= 1


# ------------------------------------------------------------------------------------------------------- 4. the cap
def test_a_full_palette_has_room_again(rt):
    n = 32 * 32 * 31

    def colours(k):
        c = (np.arange(n, dtype=np.uint32) + np.uint32(1 + k * n)) | np.uint32(0xFF000000)
        return c.reshape(31, 32, 32)

    rt.build_dense(G.make_grid("corner", SIZE), SIZE, BD)
    rt.write_dense(colours(0), (16, 16, 16))
    rt.write_dense(colours(1), (16, 16, 16))
    before, cube = rt.download(), rt.read_dense()
    assert before.desc.color_count >= 2 * n
    with pytest.raises(N.VhxError) as e:
        rt.write_dense(colours(2), (16, 16, 16))
    assert e.value.code == N.VHX_E_CAPACITY
    G.assert_same_image(rt.download(), before, "after VHX_E_CAPACITY")
    dropped = rt.compact_palette()
    assert dropped >= n and rt.tree_counts().color_count == before.desc.color_count - dropped
    G.assert_same_image(rt.download(), before.palette_compacted(), "the full palette, compacted")
    assert np.array_equal(rt.read_dense(), cube)
    rt.write_dense(colours(2), (16, 16, 16))
    cube[16:47, 16:48, 16:48] = colours(2)
    assert np.array_equal(rt.read_dense(), cube)


# --------------------------------------------------------------------------------------------------------- 5. frames
def test_frames_change_in_value_only(rt):
    edited_tree(rt)
    rt.fill_box((16, 0, 0), (8, 8, 4), int(G.rgba(7, 7, 77)))
    rt.fill_box((16, 0, 0), (8, 8, 4), int(COLOURS[0]))  # buries it, and COLOURS[1]
    sh = rt.shared()
    try:
        cam = vhx.glass_camera(SIZE, W, W, target=(SIZE / 2,) * 3)
        old = rt.download()
        frames = [bits(rt.trace_primary(cam)), bits(sh.trace_primary(cam))]
        assert rt.compact_palette() > 0
        assert rt.sync() > 0.0, "the device time of the rewrite pass"
        new = rt.download()
        want, mapping = model_palette(old)
        G.assert_same_image(new, want, "against the model")
        used = np.flatnonzero(mapping[:old.desc.color_count] != 0xFFFF)
        assert np.array_equal(new.color_palette[mapping[used]], old.color_palette[used]), "the map between the downloads"
        assert (frames[0]["value"] != EMPTY).any() and not np.array_equal(through(mapping, frames[0]["value"]),
                                                                          frames[0]["value"])
        for name, ctx, frame in (("owner", rt, frames[0]), ("shared", sh, frames[1])):
            after = bits(ctx.trace_primary(cam))
            for k, v in frame.items():
                assert np.array_equal(after[k], through(mapping, v) if k == "value" else v), f"{name}: {k}"
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_tree_as_it_was(rt):
    assert N.lib().vhx_compact_palette(rt._h, None) == N.VHX_E_STATE  # before any upload
    assert N.lib().vhx_compact_palette(None, None) == N.VHX_E_INVALID_ARG
    edited_tree(rt)
    before = rt.download()
    sh = rt.shared()
    refused(sh.compact_palette)
    sh.close()
    G.assert_same_image(rt.download(), before, "after the refusal on a shared context")

    flat = lod_image(64, 4, 0)
    rt.upload(flat)
    rt.set_node_mips(flat.node_mips)
    before = rt.download()
    refused(rt.compact_palette)
    G.assert_same_image(rt.download(), before, "after the refusal under node MIPs")
    rt.set_node_mips(None)

    for kind, word in (("node with two parents", "twice"), ("brick referenced twice", "twice"),
                       ("child at node_count", "index"), ("brick at brick_count", "index")):
        img = malformed(kind)
        rt.upload(img)
        assert word in str(refused(rt.compact_palette)), kind
        G.assert_same_image(rt.download(), img, f"after the refusal of {kind}")

    img = copy_image(images(64, 4, "brick_noise")[1])
    sel = np.flatnonzero((img.node_children != EMPTY) & ((img.node_children & SOLID) != 0) &
                         np.repeat(img.node_type == N.VHX_NODE_LEAF, 64))
    img.node_children[sel[0]] = SOLID | img.desc.solid_count
    rt.upload(img)
    assert "index" in str(refused(rt.compact_palette))
    G.assert_same_image(rt.download(), img, "after the refusal of a Solid index at solid_count")

    deep = FlatTree.from_dense(G.make_grid("sparse", 16), 16, 4)
    small = TreeImage(8, 4, {k: np.array(getattr(deep, k)) for k in G.ARRAYS})  # a cell would be half a voxel
    rt.upload(small)
    assert "smaller than a voxel" in str(refused(rt.compact_palette))
    G.assert_same_image(rt.download(), small, "after the refusal of a leaf below the voxel lattice")


# ---------------------------------------------------------------------------------------------------- 7. fixed point
@pytest.mark.parametrize("simplify", [False, True])
def test_fresh_build_is_a_fixed_point(rt, simplify):
    rt.build_dense(SG.make_grid("brick_noise", SIZE, BD), SIZE, BD, simplify=simplify)
    before = rt.download()
    assert rt.compact_palette() == 0
    G.assert_same_image(rt.download(), before, f"simplify={simplify}")
    assert rt.compact_palette() == 0
    G.assert_same_image(rt.download(), before, f"simplify={simplify}: twice")


def test_empty_tree(rt):
    zero = FlatTree.from_dense(G.make_grid("zero", SIZE), SIZE, BD)
    rt.upload(zero)
    assert rt.compact_palette() == 0
    rt.build_dense(G.make_grid("sparse", SIZE), SIZE, BD)
    rt.fill_box((0, 0, 0), (SIZE,) * 3, 0)
    before = rt.download()
    assert rt.compact_palette() == before.desc.color_count
    G.assert_same_image(rt.download(), before.palette_compacted(), "all cleared")
    assert rt.tree_counts().color_count == 0
    rt.write_dense(random_box_grid(np.random.default_rng(8), (22, 18, 35)), (13, 15, 3))
    cube = rt.read_dense()
    rt.compact()
    rt.compact_palette()
    G.assert_same_image(rt.download(), FlatTree.from_dense(cube, SIZE, BD), "written again")
