"""tests/_treecheck.py holds on the host builder's images, plain and simplified, with no orphans -- and notices the
defects it is there to find."""
import numpy as np
import pytest

from voxelhex_amd import FlatTree, TreeImage
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _simplify_grids as SG
from tests._treecheck import check_tree


def as_image(flat):
    return TreeImage(flat.boxtree_size, flat.brick_dim, {k: np.array(getattr(flat, k)) for k in G.ARRAYS})


@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_validator_holds_on_plain_images(kind, size, bd):
    flat = FlatTree.from_dense(G.make_grid(kind, size), size, bd)
    nodes, bricks = check_tree(flat, (0, 0), f"{kind} {size}/{bd}")
    assert nodes == flat.desc.node_count and bricks == flat.desc.brick_count


@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", ["full", "brick_noise", "blocks4", "cut", "sparse"])
def test_validator_holds_on_simplified_images(kind, size, bd):
    flat = FlatTree.from_dense(SG.make_grid(kind, size, bd), size, bd, simplify=True)
    nodes, bricks = check_tree(flat, (0, 0), f"{kind} {size}/{bd} simplified")
    assert nodes == flat.desc.node_count and bricks == flat.desc.brick_count


def test_validator_finds_defects():
    flat = FlatTree.from_dense(G.make_grid("sparse", 64), 64, 4)
    check_tree(as_image(flat))
    img = as_image(flat)  # an occupied bit without its entry
    s = int(np.flatnonzero(img.node_children[:64] != N.VHX_EMPTY)[0])
    img.node_children[s] = N.VHX_EMPTY
    with pytest.raises(AssertionError):
        check_tree(img)
    img = as_image(flat)  # a brick reached twice
    leaf = int(np.flatnonzero(img.node_type == N.VHX_NODE_LEAF)[0])
    e = img.node_children[leaf * 64:leaf * 64 + 64]
    a, b = np.flatnonzero(e != N.VHX_EMPTY)[:2]
    e[b] = e[a]
    with pytest.raises(AssertionError):
        check_tree(img)
    img = as_image(flat)  # a leaf unlinked from the root (64 / 4 has two levels) whose slot was not cleared
    lost = int(img.node_children[s])
    bricks = int((img.node_children[lost * 64:lost * 64 + 64] != N.VHX_EMPTY).sum())
    img.node_children[s] = N.VHX_EMPTY
    img.node_ocbits[0] &= ~np.uint64(1 << s)
    with pytest.raises(AssertionError, match="unreachable node slot"):
        check_tree(img, (1, bricks))
    img.node_type[lost], img.node_ocbits[lost] = N.VHX_NODE_NOTHING, 0  # cleared: the image is valid with its orphans
    img.node_children[lost * 64:lost * 64 + 64] = N.VHX_EMPTY
    check_tree(img, (1, bricks))
    with pytest.raises(AssertionError, match="orphans"):
        check_tree(img, (0, 0))
    img = as_image(flat)  # a brick whose cells are all empty under a set bit
    entries = img.node_children[leaf * 64:leaf * 64 + 64]
    brick = int(entries[entries != N.VHX_EMPTY][0])
    img.voxels[brick * 64:brick * 64 + 64] = N.VHX_EMPTY
    with pytest.raises(AssertionError):
        check_tree(img)
