"""vhx_flat_simplify on the host (FlatTree.simplified / TreeImage.simplified): an image compacted and simplified as
BoxTree::simplify(ROOT, recursive) leaves it. It turns every plain dense build into the simplified build of the same
grid, it agrees with the numpy restatement of the rules (tests/_simplify_model.py) on built, scrambled, hand-made and
flattened host images, it agrees with simplifying the host tree itself, and it refuses malformed images."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree, InvalidStructure
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _simplify_grids as SG
from tests._compact_model import copy_image
from tests._simplify_model import model_simplify
from tests.test_compact import MALFORMED, malformed, scramble, three_level_image

EMPTY = N.VHX_EMPTY
SOLID = N.VHX_SOLID_BIT
CASES = [(size, bd, kind) for size, bd in SG.SIZES for kind in SG.KINDS]
_cache = {}


def images(size, bd, kind):
    """(plain build, simplified build) of a grid, built once."""
    key = (size, bd, kind)
    if key not in _cache:
        grid = SG.noise_256() if kind == "noise_256" else SG.solid_order_grid()[0] if kind == "solid_order" \
            else SG.make_grid(kind, size, bd)
        _cache[key] = (FlatTree.from_dense(grid, size, bd), FlatTree.from_dense(grid, size, bd, simplify=True))
    return _cache[key]


# ------------------------------------------------------------------------------------- the builder's simplified image
@pytest.mark.parametrize("size,bd,kind", CASES)
def test_plain_build_simplifies_to_the_simplified_build(size, bd, kind):
    what = f"{kind} {size}/{bd}"
    plain, want = images(size, bd, kind)
    got = plain.simplified()
    G.assert_same_image(got, want, what)
    SG.assert_case(kind, size, bd, got)
    G.assert_same_image(model_simplify(plain), got, f"model: {what}")


def test_solid_values_by_first_node_and_sectant():
    plain, want = images(64, 4, "solid_order")
    _, a, b = SG.solid_order_grid()
    got = plain.simplified()
    G.assert_same_image(got, want, "solid_order")
    assert [int(plain.color_palette[v & 0xFFFF]) for v in got.solid_values] == [int(a), int(b)]
    G.assert_same_image(model_simplify(plain), got, "model: solid_order")


def test_noise_256():
    plain, want = images(256, 4, "noise_256")
    G.assert_same_image(plain.simplified(), want, "noise_256")


# --------------------------------------------------------------------------------------------------------- scrambled
@pytest.mark.parametrize("size,bd,kind", CASES)
def test_scrambled_images(size, bd, kind):
    what = f"{kind} {size}/{bd}"
    plain, want = images(size, bd, kind)
    mixed = scramble(plain, np.random.default_rng(size * 3 + bd), 5, 9)
    got = mixed.simplified()
    G.assert_same_image(got, want, f"{what}: scrambled plain build")
    G.assert_same_image(model_simplify(mixed), got, f"{what}: model")


# ------------------------------------------------------------------------------------ an already simplified image
@pytest.mark.parametrize("size,bd", [(64, 4), (32, 2), (16, 1), (32, 8)])
def test_simplified_image_with_a_shuffled_solid_table(size, bd):
    """solid_values reversed behind an unused value: the entries are renumbered by first use and the unused one leaves."""
    _, simp = images(size, bd, "brick_noise")
    img = copy_image(simp)
    n = img.desc.solid_count
    assert n >= 2
    arrays = {k: getattr(img, k) for k in G.ARRAYS}
    arrays["solid_values"] = np.concatenate([[np.uint32(0x00010002)], img.solid_values[::-1]]).astype(np.uint32)
    ch = arrays["node_children"]
    leafy = np.repeat((img.node_type == N.VHX_NODE_LEAF) | (img.node_type == N.VHX_NODE_UNIFORM_LEAF), 64)
    sel = leafy & (ch != EMPTY) & ((ch & SOLID) != 0)
    ch[sel] = SOLID | (n - (ch[sel] & ~np.uint32(SOLID)))
    shuffled = vhx.TreeImage(size, bd, arrays)
    got = shuffled.simplified()
    G.assert_same_image(got, simp, f"{size}/{bd}")
    G.assert_same_image(model_simplify(shuffled), got, f"{size}/{bd}: model")
    G.assert_same_image(simp.simplified(), simp, f"{size}/{bd}: a simplified build comes back as it is")


# ------------------------------------------------------------------------------------------------- host tree, data
def edited_host_tree(size=64, bd=4, n=300, seed=11):
    """Random single inserts of Visual, Complex and Informative entries, two whole bricks and a whole leaf of one
    Complex value each, and a brick of one Informative value; auto-simplify off, so all of it sits in Parted bricks."""
    rng = np.random.default_rng(seed)
    tree = BoxTree(size, bd)
    tree.auto_simplify = False
    for k in range(n):
        p = tuple(int(v) for v in rng.integers(0, size, 3))
        albedo = vhx.Albedo.from_packed(int(G.COLORS[rng.integers(0, 3)]))
        entry = [albedo, vhx.BoxTreeEntry.Complex(albedo, int(rng.integers(1, 9))),
                 vhx.BoxTreeEntry.Informative(int(rng.integers(1, 9)))][k % 3]
        tree.insert(p, entry)
    one = vhx.BoxTreeEntry.Complex(vhx.Albedo.from_packed(int(G.COLORS[1])), 77)
    for x in range(8):
        for y in range(4):
            for z in range(4):
                tree.insert((x + 16, y + 32, z + 48), one)
                tree.insert((x + 40 - (x & 4), y + 8, z + 8 + (x & 4)), vhx.BoxTreeEntry.Informative(5))
    for x in range(16):
        for y in range(16):
            for z in range(16):
                tree.insert((48 + x, 48 + y, z), one)
    return tree


@pytest.fixture(scope="module")
def host_tree_image():
    tree = edited_host_tree()
    return tree, tree.flatten()


def test_flattened_host_tree_with_data_values(host_tree_image):
    tree, img = host_tree_image
    assert img.desc.data_count > 0 and img.desc.brick_count > 0 and img.desc.solid_count == 0
    got = img.simplified()
    G.assert_same_image(model_simplify(img), got, "model: random inserts")
    types, empty, solid, parted = SG.entry_kinds(got)
    assert (got.solid_values >> 16 != 0xFFFF).any(), "a Solid value with a data index"
    assert ((types == N.VHX_NODE_UNIFORM_LEAF) & solid[:, 0]).any() and ((types == N.VHX_NODE_LEAF) & solid.any(1)).any()
    assert parted.any() and got.desc.brick_count < img.desc.brick_count
    assert np.array_equal(got.color_palette, img.color_palette) and np.array_equal(got.data_palette, img.data_palette)
    mixed = scramble(img, np.random.default_rng(5), 6, 13)
    G.assert_same_image(mixed.simplified(), got, "random inserts, scrambled")


def test_host_tree_route_agrees(host_tree_image):
    _, img = host_tree_image
    tree = edited_host_tree()
    tree.simplify(recursive=True)
    G.assert_same_image(img.simplified(), tree.flatten(), "flatten().simplified() against simplify() + flatten()")


# ------------------------------------------------------------------------------------------------------- hand-made
def test_internal_node_without_occupied_bits():
    img = copy_image(three_level_image())
    inner = [int(n) for n in np.flatnonzero(img.node_type == N.VHX_NODE_INTERNAL) if n != 0]
    img.node_ocbits[inner[0]] = 0
    got = img.simplified()
    G.assert_same_image(model_simplify(img), got, "ocbits 0")
    below = int((img.node_children.reshape(-1, 64)[inner[0]] != EMPTY).sum())
    assert below > 0 and got.desc.node_count == img.desc.node_count - below
    ch = img.node_children.reshape(-1, 64)
    s = int(np.flatnonzero(ch[0] == inner[0])[0])
    node = int(got.node_children[s])
    assert got.node_type[node] == N.VHX_NODE_NOTHING and got.node_ocbits[node] == 0
    assert (got.node_children.reshape(-1, 64)[node] == EMPTY).all()
    root = copy_image(three_level_image())
    root.node_ocbits[0] = 0
    got = root.simplified()
    assert got.node_type.tolist() == [N.VHX_NODE_NOTHING] and got.desc.brick_count == 0
    G.assert_same_image(model_simplify(root), got, "ocbits 0 at the root")


POINTS_TO_EMPTY = [np.uint32(0xFFFF7000), np.uint32(0x70007000)]  # indices past both palettes


@pytest.mark.parametrize("size,bd", [(16, 4), (32, 2), (32, 8), (16, 1)])
def test_leaf_of_values_that_point_to_empty(size, bd):
    """Every brick of one value that points to empty: the entries become empty and, for brick_dim > 1, rule (c) makes
    the leaf a UniformLeaf over a brick of 0xFFFFFFFF cells, so a second call changes the image again."""
    what = f"{size}/{bd}"
    img = copy_image(FlatTree.from_dense(SG.make_grid("full", size, bd), size, bd))
    img.voxels[:] = POINTS_TO_EMPTY[0]
    got = img.simplified()
    G.assert_same_image(model_simplify(img), got, what)
    types, empty, solid, parted = SG.entry_kinds(got)
    if bd == 1:
        assert (types == N.VHX_NODE_LEAF).all() and empty.all(), what
    else:
        assert (types == N.VHX_NODE_UNIFORM_LEAF).all() and parted[:, 0].all(), what
        assert (got.voxels == EMPTY).all() and got.desc.brick_count == types.size, what
        again = got.simplified()
        G.assert_same_image(model_simplify(got), again, f"{what}: again")
        assert again.desc.brick_count == 0 and (again.node_type != N.VHX_NODE_NOTHING).any(), what
    # two such values in one brick: the brick is not homogeneous and stays
    if bd > 1:
        img.voxels[1::2] = POINTS_TO_EMPTY[1]
        got = img.simplified()
        G.assert_same_image(model_simplify(img), got, f"{what}: two values")
        assert got.desc.brick_count == img.desc.brick_count


def test_uniform_leaf_cases():
    """A UniformLeaf over a Solid value that points to empty becomes Nothing; over a Parted brick of one such value it
    keeps an empty entry; over a Parted brick of one visible value it holds that Solid value."""
    grid = SG.make_grid("blocks4", 64, 4)
    grid[48:64, 48:64, 48:64] = SG.THREE[0]  # a UniformLeaf over a Solid brick
    img = copy_image(FlatTree.from_dense(grid, 64, 4, simplify=True))
    ch = img.node_children.reshape(-1, 64)
    uni = np.flatnonzero(img.node_type == N.VHX_NODE_UNIFORM_LEAF)
    over_parted = [int(n) for n in uni if ch[n, 0] != EMPTY and not ch[n, 0] & SOLID]
    over_solid = [int(n) for n in uni if ch[n, 0] != EMPTY and ch[n, 0] & SOLID]
    assert len(over_parted) >= 2 and over_solid
    n3 = 64
    visible = img.solid_values[0]
    img.voxels[int(ch[over_parted[0], 0]) * n3:][:n3] = POINTS_TO_EMPTY[0]
    img.voxels[int(ch[over_parted[1], 0]) * n3:][:n3] = visible
    img.solid_values[int(ch[over_solid[0], 0] & ~np.uint32(SOLID))] = POINTS_TO_EMPTY[1]
    got = img.simplified()
    G.assert_same_image(model_simplify(img), got, "UniformLeaf cases")
    gch = got.node_children.reshape(-1, 64)
    assert got.node_type[over_parted[0]] == N.VHX_NODE_UNIFORM_LEAF and gch[over_parted[0], 0] == EMPTY
    assert got.solid_values[gch[over_parted[1], 0] & ~np.uint32(SOLID)] == visible and gch[over_parted[1], 0] & SOLID
    assert got.node_type[over_solid[0]] == N.VHX_NODE_NOTHING and (gch[over_solid[0]] == EMPTY).all()


# -------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_images_are_refused(kind):
    img = malformed(kind)
    with pytest.raises(InvalidStructure):
        img.simplified()
    h = ctypes.c_void_p(1)
    assert N.lib().vhx_flat_simplify(ctypes.byref(img.desc), ctypes.byref(h)) == N.VHX_E_TREE_INVALID_STRUCTURE
    assert h.value is None, "no image is returned"


def test_solid_index_past_the_count_and_duplicate_palette_entries():
    _, simp = images(64, 4, "brick_noise")
    img = copy_image(simp)
    sel = np.flatnonzero((img.node_children != EMPTY) & ((img.node_children & SOLID) != 0) &
                         np.repeat(img.node_type == N.VHX_NODE_LEAF, 64))
    img.node_children[sel[0]] = SOLID | img.desc.solid_count
    with pytest.raises(InvalidStructure):
        img.simplified()
    img = copy_image(simp)
    assert img.desc.color_count >= 2
    img.color_palette[1] = img.color_palette[0]
    with pytest.raises(InvalidStructure):
        img.simplified()
    img.compacted()  # the compaction alone does not look at the palettes


def test_null_arguments():
    assert N.lib().vhx_flat_simplify(None, None) == N.VHX_E_INVALID_ARG
    h = ctypes.c_void_p()
    assert N.lib().vhx_flat_simplify(None, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    d = N.TreeDesc()
    assert N.lib().vhx_flat_simplify(ctypes.byref(d), ctypes.byref(h)) == N.VHX_E_INVALID_ARG  # no nodes
