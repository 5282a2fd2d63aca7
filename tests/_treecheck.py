"""A structural validator of a flattened tree image (a FlatTree, or the TreeImage Raytracer.download gives): the rules an
image of canonical depth keeps whatever wrote it, and after in-place writes (vhx_write_dense) the slots they unlinked."""
import numpy as np

from voxelhex_amd import _native as N
from tests import _flatget as F

EMPTY = N.VHX_EMPTY
SECTANTS = np.arange(64, dtype=np.uint64)


def levels_of(size, bd):
    """Node levels of a tree of canonical depth: size = bd * 4^levels."""
    levels, edge = 0, bd
    while edge < size:
        edge *= 4
        levels += 1
    assert edge == size and levels >= 1, f"size {size} is not brick_dim {bd} * 4^k"
    return levels


def check_tree(img, orphans=(0, 0), what=""):
    """Walks from the root, level by level. Every occupied bit <=> a non-empty child entry; child and brick indices
    inside their counts; no node or Parted brick reached twice; no reachable node but the root with occupancy 0; leaves
    at the lowest level only and nothing else there; a leaf's bit <=> its brick holds a non-empty cell; every unreachable
    node slot is Nothing with occupancy 0 and empty entries; the unreachable nodes and bricks number `orphans`. Returns
    (reachable nodes, reachable Parted bricks)."""
    size, bd = int(img.boxtree_size), int(img.brick_dim)
    n3 = bd ** 3
    D = levels_of(size, bd) - 1
    types, occ = np.asarray(img.node_type), np.asarray(img.node_ocbits)
    ch = np.asarray(img.node_children).reshape(-1, 64)
    nn, nb, ns = types.size, int(img.desc.brick_count), int(img.desc.solid_count)
    assert nn >= 1 and occ.size == nn and ch.shape[0] == nn, f"{what}: array sizes"
    voxels = np.asarray(img.voxels).reshape(nb, n3)
    seen_node, seen_brick = np.zeros(nn, bool), np.zeros(nb, bool)
    seen_node[0] = True

    def claim(seen, idx, count, name):
        assert (idx < count).all(), f"{what}: {name} index past its count"
        assert np.unique(idx).size == idx.size and not seen[idx].any(), f"{what}: a {name} is reached twice"
        seen[idx] = True

    def brick_full(desc):
        """per descriptor: the brick holds a non-empty cell"""
        solid = (desc & N.VHX_SOLID_BIT) != 0
        assert ((desc[solid] & 0x7FFFFFFF) < ns).all(), f"{what}: solid index past its count"
        full = np.zeros(desc.size, bool)
        if solid.any():
            full[solid] = ~F.points_to_empty(img, np.asarray(img.solid_values)[desc[solid] & 0x7FFFFFFF])
        if (~solid).any():
            full[~solid] = (~F.points_to_empty(img, voxels[desc[~solid]])).any(1)
        return full

    level = np.zeros(1, np.int64)
    for lv in range(D + 1):
        t, o, e = types[level], occ[level], ch[level]
        bits = ((o[:, None] >> SECTANTS[None, :]) & np.uint64(1)).astype(bool)
        internal, leaf, uni = t == N.VHX_NODE_INTERNAL, t == N.VHX_NODE_LEAF, t == N.VHX_NODE_UNIFORM_LEAF
        nothing = t == N.VHX_NODE_NOTHING
        assert (internal | leaf | uni | nothing).all(), f"{what}: unknown node type"
        if lv > 0:
            assert (o != 0).all() and not nothing.any(), f"{what}: a reachable node of level {lv} is empty"
        else:
            assert (o[nothing] == 0).all() and (e[nothing] == EMPTY).all(), f"{what}: a Nothing root with content"
        if lv < D:
            assert not (leaf | uni).any(), f"{what}: a leaf at level {lv} above the lowest level {D}"
        else:
            assert not internal.any(), f"{what}: an internal node at the lowest level"
        il = internal | leaf
        assert ((e[il] != EMPTY) == bits[il]).all(), f"{what}: level {lv}: occupied bits and child entries disagree"
        kids = e[internal][bits[internal]].astype(np.int64)
        claim(seen_node, kids, nn, "node")
        d = e[leaf][bits[leaf]]
        parted = d[(d & N.VHX_SOLID_BIT) == 0].astype(np.int64)
        claim(seen_brick, parted, nb, "brick")
        assert brick_full(d).all(), f"{what}: a leaf's occupied bit over a brick without a non-empty cell"
        assert (e[uni][:, 0] != EMPTY).all() and (e[uni][:, 1:] == EMPTY).all() and (o[uni] != 0).all(), \
            f"{what}: a UniformLeaf holds one brick in entry 0"
        d = e[uni][:, 0]
        claim(seen_brick, d[(d & N.VHX_SOLID_BIT) == 0].astype(np.int64), nb, "brick")
        brick_full(d)
        level = kids
    assert level.size == 0
    lost = ~seen_node
    assert (types[lost] == N.VHX_NODE_NOTHING).all() and (occ[lost] == 0).all() and (ch[lost] == EMPTY).all(), \
        f"{what}: an unreachable node slot is not Nothing / 0 / empty"
    got = (int(lost.sum()), int((~seen_brick).sum()))
    assert got == tuple(orphans), f"{what}: {got} unreachable (nodes, bricks), orphans() says {tuple(orphans)}"
    return int(seen_node.sum()), int(seen_brick.sum())
