"""vhx_flat_compact on the host (FlatTree.compacted / TreeImage.compacted): an image without its unreachable slots, in the
builders' numbering. It is the identity on every freshly built image, it undoes any renumbering with junk slots in
between, it agrees with the numpy model of the rules (tests/_compact_model.py), and it refuses malformed images."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import BoxTree, FlatTree, InvalidStructure, TreeImage
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._compact_model import copy_image, model_compact, scramble
from tests._treecheck import check_tree

EMPTY = N.VHX_EMPTY
SCRAMBLE_SIZES = [(16, 1), (32, 2), (64, 4), (32, 8), (64, 1)]  # (64, 1): three node levels


# ------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("simplify", [False, True])
def test_identity_on_dense_builds(size, bd, kind, simplify):
    img = FlatTree.from_dense(G.make_grid(kind, size), size, bd, simplify=simplify)
    G.assert_same_image(img.compacted(), img, f"{kind} {size}/{bd} simplify={simplify}")


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 2)])
@pytest.mark.parametrize("kind", SG.KINDS)
@pytest.mark.parametrize("simplify", [False, True])
def test_identity_on_simplify_grids(size, bd, kind, simplify):
    img = FlatTree.from_dense(SG.make_grid(kind, size, bd), size, bd, simplify=simplify)
    G.assert_same_image(img.compacted(), img, f"{kind} {size}/{bd} simplify={simplify}")
    G.assert_same_image(model_compact(img), img, f"model: {kind} {size}/{bd} simplify={simplify}")


def random_insert_tree(size=64, bd=4, n=300, seed=11):
    rng = np.random.default_rng(seed)
    tree = BoxTree(size, bd)
    for k in range(n):
        p = tuple(int(v) for v in rng.integers(0, size, 3))
        albedo = vhx.Albedo.from_packed(int(G.COLORS[rng.integers(0, 3)]))
        entry = [albedo, vhx.BoxTreeEntry.Complex(albedo, int(rng.integers(1, 9))),
                 vhx.BoxTreeEntry.Informative(int(rng.integers(1, 9)))][k % 3]
        tree.insert(p, entry)
    return tree


def test_identity_on_a_flattened_host_tree():
    img = random_insert_tree().flatten()
    assert img.desc.data_count > 0 and img.desc.brick_count > 0
    G.assert_same_image(img.compacted(), img, "flatten() of random inserts")
    G.assert_same_image(model_compact(img), img, "model: flatten() of random inserts")


# ------------------------------------------------------------------------------------------------------- scramble
@pytest.mark.parametrize("size,bd", SCRAMBLE_SIZES)
def test_scrambled_images_compact_back(size, bd):
    what = f"{size}/{bd}"
    img = FlatTree.from_dense(SG.make_grid("brick_noise", size, bd), size, bd, simplify=True)
    if (size, bd) == (64, 1):
        assert (img.node_type == N.VHX_NODE_INTERNAL).sum() > 1, "three node levels"
    mixed = scramble(img, np.random.default_rng(size + bd), 7, 11)
    assert mixed.desc.node_count == img.desc.node_count + 7 and mixed.desc.brick_count == img.desc.brick_count + 11
    assert not np.array_equal(mixed.node_children[:64], img.node_children[:64]) or img.desc.node_count == 1
    got = mixed.compacted()
    G.assert_same_image(got, img, f"{what}: compacted against the original")
    G.assert_same_image(got, model_compact(mixed), f"{what}: compacted against the model")
    assert check_tree(got, (0, 0), what) == (img.desc.node_count, img.desc.brick_count)
    check_tree(mixed, (7, 11), f"{what}: the scrambled image")


# ------------------------------------------------------------------------------------------- non-canonical depth
LOD_CASES = [(64, 1, 0), (64, 1, 1), (64, 4, 0)]  # the depths tests/test_gpu_mips.py cuts at; (64, 1) has three levels


def lod_image(size, bd, depth):
    return FlatTree.build_scene_lod(N.VHX_SCENE_LATTICE_CUBE, size, bd, depth)


@pytest.mark.parametrize("size,bd,depth", LOD_CASES)
def test_lod_cut_images(size, bd, depth):
    what = f"{size}/{bd} depth {depth}"
    img = lod_image(size, bd, depth)
    ch, occ = img.node_children.reshape(-1, 64), img.node_ocbits
    cut = np.flatnonzero(img.node_type == N.VHX_NODE_INTERNAL)
    bits = ((occ[cut, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert (bits & (ch[cut] == EMPTY)).any(), f"{what}: no occupied sectant with an absent child"
    got = img.compacted()
    G.assert_same_image(got, model_compact(img), what)
    assert got.desc.brick_count < img.desc.brick_count, f"{what}: the MIP bricks are unreachable through the entries"
    assert got.node_mips.size == 0
    pos = F.lattice((0, 0, 0), (size,) * 3)
    assert np.array_equal(F.flat_get(got, pos), F.flat_get(img, pos)), f"{what}: get changed"


# ------------------------------------------------------------------------------------------------------- refusals
def three_level_image():
    return FlatTree.from_dense(G.make_grid("sparse", 64), 64, 1)


def first_entry(img, node_type, pred):
    """(node, sectant) of the first entry of a node of `node_type` that satisfies pred(entry)."""
    ch = img.node_children.reshape(-1, 64)
    for n in np.flatnonzero(img.node_type == node_type):
        s = np.flatnonzero(pred(ch[n]))
        if s.size:
            return int(n), int(s[0])
    raise AssertionError("no such entry")


def parted(e):
    return (e != EMPTY) & ((e & N.VHX_SOLID_BIT) == 0)


def malformed(kind):
    img = copy_image(three_level_image())
    ch = img.node_children.reshape(-1, 64)
    if kind == "child at node_count":
        n, s = first_entry(img, N.VHX_NODE_INTERNAL, lambda e: e != EMPTY)
        ch[n, s] = img.desc.node_count
    elif kind == "brick at brick_count":
        n, s = first_entry(img, N.VHX_NODE_LEAF, parted)
        ch[n, s] = img.desc.brick_count
    elif kind == "node with two parents":
        inner = [n for n in np.flatnonzero(img.node_type == N.VHX_NODE_INTERNAL) if n != 0]
        a, b = int(inner[0]), int(inner[1])
        sb = int(np.flatnonzero(ch[b] != EMPTY)[0])
        ch[a, int(np.flatnonzero(ch[a] != EMPTY)[0])] = ch[b, sb]
    elif kind == "brick referenced twice":
        leaves = np.flatnonzero(img.node_type == N.VHX_NODE_LEAF)
        a, b = int(leaves[0]), int(leaves[-1])
        ch[a, int(np.flatnonzero(parted(ch[a]))[0])] = ch[b, int(np.flatnonzero(parted(ch[b]))[0])]
    else:
        raise ValueError(kind)
    return img


MALFORMED = ["child at node_count", "brick at brick_count", "node with two parents", "brick referenced twice"]


@pytest.mark.parametrize("kind", MALFORMED)
def test_malformed_images_are_refused(kind):
    img = malformed(kind)
    with pytest.raises(InvalidStructure):
        img.compacted()
    with pytest.raises(AssertionError):
        model_compact(img)
    h = ctypes.c_void_p(1)
    assert N.lib().vhx_flat_compact(ctypes.byref(img.desc), ctypes.byref(h)) == N.VHX_E_TREE_INVALID_STRUCTURE
    assert h.value is None, "no image is returned"


def test_more_than_eight_levels_are_refused():
    """A chain of nine nodes, each the only child of the one before."""
    n = 9
    arrays = dict(node_type=np.full(n, N.VHX_NODE_INTERNAL, np.uint32), node_ocbits=np.ones(n, np.uint64),
                  node_children=np.full(n * 64, EMPTY, np.uint32), voxels=np.zeros(0, np.uint32),
                  solid_values=np.zeros(0, np.uint32), color_palette=np.zeros(0, np.uint32),
                  data_palette=np.zeros(0, np.uint32))
    arrays["node_type"][-1] = N.VHX_NODE_NOTHING
    arrays["node_children"][np.arange(n - 1) * 64] = np.arange(1, n, dtype=np.uint32)
    with pytest.raises(InvalidStructure):
        TreeImage(4 ** 9, 1, arrays).compacted()
    for k in ("node_type", "node_ocbits"):
        arrays[k] = arrays[k][1:]
    arrays["node_children"] = arrays["node_children"][:-64].copy()
    arrays["node_children"][(n - 2) * 64] = EMPTY
    assert TreeImage(4 ** 9, 1, arrays).compacted().desc.node_count == 8  # eight levels pass


def test_null_arguments():
    assert N.lib().vhx_flat_compact(None, None) == N.VHX_E_INVALID_ARG
    h = ctypes.c_void_p()
    assert N.lib().vhx_flat_compact(None, ctypes.byref(h)) == N.VHX_E_INVALID_ARG
    d = N.TreeDesc()
    assert N.lib().vhx_flat_compact(ctypes.byref(d), ctypes.byref(h)) == N.VHX_E_INVALID_ARG  # no nodes


# ----------------------------------------------------------------------------------------------------- empty tree
def test_empty_trees():
    zero = FlatTree.from_dense(G.make_grid("zero", 64), 64, 4)
    assert zero.node_type.tolist() == [N.VHX_NODE_NOTHING]
    G.assert_same_image(zero.compacted(), zero, "the zero grid")
    img = copy_image(FlatTree.from_dense(G.make_grid("sparse", 64), 64, 4))
    img.node_type[0] = N.VHX_NODE_NOTHING  # as a clear of everything leaves the root, the old slots behind it
    img.node_ocbits[0] = 0
    img.node_children[:64] = EMPTY
    got = img.compacted()
    assert got.counts() == dict(img.counts(), node_count=1, brick_count=0)
    assert got.node_type.tolist() == [N.VHX_NODE_NOTHING] and got.node_ocbits.tolist() == [0]
    assert (got.node_children == EMPTY).all() and got.node_children.size == 64 and got.voxels.size == 0
    assert np.array_equal(got.color_palette, img.color_palette)
    G.assert_same_image(got, model_compact(img), "a Nothing root with garbage behind it")
