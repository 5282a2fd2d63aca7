"""vhx_flat_compact_palette on the host (FlatTree.palette_compacted / TreeImage.palette_compacted): an image with the
colour palette the builders give the voxels it holds now. Every test holds it to the numpy model of the rules
(tests/_palette_model.py), bit for bit: it undoes any scramble of the palette of a fresh build, plain or simplified, it is
the identity on fresh builds and idempotent, it keeps data values, it translates orphaned cells without letting them keep
a colour alive, and it refuses malformed images."""
import ctypes

import numpy as np
import pytest

from voxelhex_amd import FlatTree, InvalidStructure, TreeImage
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._compact_model import copy_image, scramble
from tests._palette_model import model_palette, scramble_palette, walk
from tests.test_compact import MALFORMED, malformed
from tests.test_flat_simplify import edited_host_tree, images

EMPTY = N.VHX_EMPTY
SOLID = N.VHX_SOLID_BIT
SIZES = [(16, 1), (32, 2), (64, 4), (32, 8)]  # (16, 1): a brick is one dword, the voxel buffer no multiple of 16 bytes
KINDS = ["brick_noise", "blocks4", "cut", "sparse"]
_positions = {}


def assert_same_voxels(got, want, what):
    """Every voxel has the colour, the data half and the emptiness it had: what read_dense and get report."""
    size = int(want.boxtree_size)
    if size not in _positions:
        _positions[size] = F.lattice((0, 0, 0), (size,) * 3)
    a, b = F.flat_get(got, _positions[size]), F.flat_get(want, _positions[size])
    assert np.array_equal(F.flat_albedo(got, a), F.flat_albedo(want, b)), f"{what}: colours"
    assert np.array_equal(a >> 16, b >> 16), f"{what}: data halves"
    assert np.array_equal(F.points_to_empty(got, a), F.points_to_empty(want, b)), f"{what}: emptiness"


def scrambled(size, bd, kind, simplify):
    base = images(size, bd, kind)[1 if simplify else 0]
    return base, scramble_palette(base, np.random.default_rng(size * 11 + bd + simplify))


# ------------------------------------------------------------------------------------------- scrambles and recovery
@pytest.mark.parametrize("size,bd", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("simplify", [False, True])
def test_scrambled_palette_comes_back(size, bd, kind, simplify):
    what = f"{kind} {size}/{bd} simplify={simplify}"
    base, mixed = scrambled(size, bd, kind, simplify)
    assert mixed.desc.color_count > base.desc.color_count
    assert_same_voxels(mixed, base, f"{what}: the scramble")
    got = mixed.palette_compacted()
    want, mapping = model_palette(mixed)
    G.assert_same_image(got, want, f"{what}: against the model")
    G.assert_same_image(got, base, f"{what}: against the unscrambled build")
    assert mapping[0xFFFF] == 0xFFFF and (mapping[mixed.desc.color_count:] == 0xFFFF).all()


def test_the_grids_reach_every_kind_of_value():
    """Solid entries in a Leaf, both kinds of UniformLeaf, and Leaf nodes of Parted bricks all occur in the images above."""
    seen = set()
    for size, bd in SIZES:
        for kind in KINDS:
            img = images(size, bd, kind)[1]
            types, empty, solid, parted = SG.entry_kinds(img)
            leaf, uni = types == N.VHX_NODE_LEAF, types == N.VHX_NODE_UNIFORM_LEAF
            seen |= {name for name, hit in (("leaf solid", (leaf & solid.any(1)).any()),
                                            ("leaf parted", (leaf & parted.any(1)).any()),
                                            ("uniform solid", (uni & solid[:, 0]).any()),
                                            ("uniform parted", (uni & parted[:, 0]).any())) if hit}
    assert seen == {"leaf solid", "leaf parted", "uniform solid", "uniform parted"}


@pytest.mark.parametrize("size,bd", SIZES)
@pytest.mark.parametrize("simplify", [False, True])
def test_fresh_build_is_a_fixed_point_and_the_call_is_idempotent(size, bd, simplify):
    what = f"{size}/{bd} simplify={simplify}"
    base, mixed = scrambled(size, bd, "brick_noise", simplify)
    G.assert_same_image(base.palette_compacted(), base, f"{what}: a fresh build")
    G.assert_same_image(model_palette(base)[0], base, f"{what}: a fresh build, model")
    once = mixed.palette_compacted()
    G.assert_same_image(once.palette_compacted(), once, f"{what}: twice")


def test_first_index_is_x_major():
    """Colour A only at (1,0,0), colour B only at (0,0,1): B comes first, whatever the palette said."""
    grid, (b, a) = G.palette_order_grid()
    base = FlatTree.from_dense(grid, 4, 1)
    img = copy_image(base)
    assert img.color_palette.tolist() == [b, a]
    img.color_palette[:] = [a, b]
    img.voxels[:] = np.where(img.voxels == EMPTY, img.voxels, img.voxels ^ np.uint32(1))
    got = img.palette_compacted()
    G.assert_same_image(got, base, "x outer, z inner")
    G.assert_same_image(got, model_palette(img)[0], "x outer, z inner: model")


# ------------------------------------------------------------------------------------------------------ data values
def test_data_values_stay():
    img = edited_host_tree().flatten()
    assert img.desc.data_count > 0
    for base in (img, img.simplified()):
        mixed = scramble_palette(base, np.random.default_rng(5))
        got = mixed.palette_compacted()
        G.assert_same_image(got, model_palette(mixed)[0], "data values: against the model")
        assert np.array_equal(got.voxels >> 16, mixed.voxels >> 16), "data halves of the cells"
        assert np.array_equal(got.solid_values >> 16, mixed.solid_values >> 16), "data halves of the solid values"
        assert np.array_equal(got.data_palette, mixed.data_palette)
        for k in ("node_type", "node_ocbits", "node_children"):
            assert np.array_equal(getattr(got, k), getattr(mixed, k)), k
        assert_same_voxels(got, base, "data values")
        assert (got.voxels >> 16 != 0xFFFF).any()


# ---------------------------------------------------------------------------------------------------- orphaned slots
def junk_image(size, bd):
    """(the simplified brick_noise build, its palette scrambled and the image renumbered into 7 junk node and 11 junk
    brick slots, the orphaned brick slots, dead, live): orphan 0 is filled with cells naming `dead`, an entry of a
    visible colour that nothing else names; orphan 1 with cells naming the entry `live` of a colour in use."""
    base, mixed = scrambled(size, bd, "brick_noise", True)
    junk = copy_image(scramble(mixed, np.random.default_rng(size + bd), 7, 11))
    orphans = np.setdiff1d(np.arange(junk.desc.brick_count), walk(junk)[2])
    assert orphans.size == 11
    arrays = {k: getattr(junk, k) for k in G.ARRAYS}
    dead = junk.desc.color_count
    arrays["color_palette"] = np.concatenate([junk.color_palette, [G.rgba(3, 1, 4)]]).astype(np.uint32)
    vox = arrays["voxels"].reshape(-1, bd ** 3)
    vox[orphans[0]] = np.uint32(0xFFFF0000 | dead)
    ci = (walk(junk)[0] & np.uint32(0xFFFF)).astype(np.int64)
    ci = ci[ci < dead]
    live = int(ci[(junk.color_palette[ci] >> 24) != 0][0])
    vox[orphans[1]] = np.uint32(0x00070000 | live)
    return base, TreeImage(size, bd, arrays), orphans, dead, live


@pytest.mark.parametrize("size,bd", SIZES)
def test_orphaned_cells_are_translated_and_keep_no_colour_alive(size, bd):
    what = f"{size}/{bd}"
    base, junk, orphans, dead, live = junk_image(size, bd)
    n3 = bd ** 3
    got = junk.palette_compacted()
    want, mapping = model_palette(junk)
    G.assert_same_image(got, want, f"{what}: against the model")
    assert mapping[dead] == 0xFFFF and got.desc.color_count == base.desc.color_count
    assert np.array_equal(got.color_palette, base.color_palette)
    cells = got.voxels.reshape(-1, n3)
    assert (cells[orphans[0]] == 0xFFFFFFFF).all(), "the dead colour's cells name none"
    assert (cells[orphans[1]] == (0x00070000 | mapping[live])).all(), "a live colour's orphaned cells are translated"
    assert got.desc.brick_count == junk.desc.brick_count and got.desc.node_count == junk.desc.node_count
    G.assert_same_image(got.compacted(), base, f"{what}: compacted, the unscrambled build")


# --------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_images_are_refused(kind):
    img = malformed(kind)
    with pytest.raises(InvalidStructure):
        img.palette_compacted()
    with pytest.raises(AssertionError):
        model_palette(img)
    h = ctypes.c_void_p(1)
    assert N.lib().vhx_flat_compact_palette(ctypes.byref(img.desc), ctypes.byref(h)) == N.VHX_E_TREE_INVALID_STRUCTURE
    assert h.value is None, "no image is returned"


def test_solid_index_past_the_count_and_a_leaf_below_the_voxel_lattice():
    img = copy_image(images(64, 4, "brick_noise")[1])
    sel = np.flatnonzero((img.node_children != EMPTY) & ((img.node_children & SOLID) != 0) &
                         np.repeat(img.node_type == N.VHX_NODE_LEAF, 64))
    img.node_children[sel[0]] = SOLID | img.desc.solid_count
    with pytest.raises(InvalidStructure):
        img.palette_compacted()
    with pytest.raises(AssertionError):
        model_palette(img)
    deep = FlatTree.from_dense(G.make_grid("sparse", 16), 16, 4)  # one Leaf of 4^3 bricks ...
    arrays = {k: np.array(getattr(deep, k)) for k in G.ARRAYS}
    small = TreeImage(8, 4, arrays)  # ... in a root cube of half the edge: a cell would be half a voxel
    with pytest.raises(InvalidStructure):
        small.palette_compacted()
    with pytest.raises(AssertionError):
        model_palette(small)


def test_null_arguments():
    assert N.lib().vhx_flat_compact_palette(None, None) == N.VHX_E_INVALID_ARG
    h = ctypes.c_void_p()
    assert N.lib().vhx_flat_compact_palette(None, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    d = N.TreeDesc()
    assert N.lib().vhx_flat_compact_palette(ctypes.byref(d), ctypes.byref(h)) == N.VHX_E_INVALID_ARG  # no nodes
