"""The canonical colour palette of a flattened image restated in numpy, independent of the C++
(vhx_flat_compact_palette) and of the device pass (vhx_compact_palette), and a scrambler that makes a palette
non-canonical without changing what the image shows.

The rules (include/vhx_boxtree.h): nodes and Parted bricks are reachable as for the compaction; a
reachable value is every cell of a reachable Parted brick and the solid_values entry of every reachable Solid entry; a
value names a colour when its index v & 0xFFFF is not 0xFFFF, below color_count and the entry's alpha byte is not 0;
entries of one 32-bit colour are one colour. Every reachable value sits on a cube (a cell, a whole brick, a whole node)
with min corner (x, y, z) and first index (x * size + y) * size + z; a colour's first index is the minimum over the values
that name it, and the new palette holds the used colours in increasing first index. Every cell of every brick slot and
every solid value gets its colour half translated; an index that named no colour becomes 0xFFFF."""
import numpy as np

from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import TreeImage
from tests._compact_model import _arrays

EMPTY = N.VHX_EMPTY
SOLID = N.VHX_SOLID_BIT
NONE = 0xFFFF


def walk(img):
    """Reachable values with their cubes' min corners: (values, x, y, z) as flat arrays, and the reachable Parted bricks.
    Asserts what the C++ refuses."""
    size, bd = int(img.boxtree_size), int(img.brick_dim)
    n3 = bd ** 3
    a = _arrays(img)
    types, ch = a["node_type"], a["node_children"].reshape(-1, 64)
    nn, nb = types.size, a["voxels"].size // n3
    vox, solids = a["voxels"].reshape(nb, n3), a["solid_values"]
    c = np.arange(n3, dtype=np.uint64)
    cell_xyz = np.stack([c % bd, (c // bd) % bd, c // (bd * bd)], 1)  # a brick's cells, in cell units
    s = np.arange(64, dtype=np.uint64)
    sect_xyz = np.stack([s & 3, (s >> 2) & 3, s >> 4], 1)
    vals, corners, bricks = [], [], []
    seen_nodes, seen_bricks = {0}, set()
    level, depth = [(0, np.zeros(3, np.uint64))], 0
    while level:
        assert depth < 8, "more than 8 node levels"
        edge = size >> (2 * depth)
        nxt = []
        for o, org in level:
            t = types[o]
            if t == N.VHX_NODE_INTERNAL:
                for k in np.flatnonzero(ch[o] != EMPTY):
                    e = int(ch[o, k])
                    assert e < nn, "child index past node_count"
                    assert e not in seen_nodes, "a node is reached twice"
                    seen_nodes.add(e)
                    nxt.append((e, org + sect_xyz[k] * np.uint64(edge // 4)))
                continue
            if t not in (N.VHX_NODE_LEAF, N.VHX_NODE_UNIFORM_LEAF):
                continue
            brick_edge = edge if t == N.VHX_NODE_UNIFORM_LEAF else edge // 4
            cell = brick_edge // bd
            assert cell >= 1, "a leaf whose cells are smaller than a voxel"
            for k in range(1 if t == N.VHX_NODE_UNIFORM_LEAF else 64):
                e = int(ch[o, k])
                if e == EMPTY:
                    continue
                corner = org + sect_xyz[k] * np.uint64(brick_edge)
                if e & SOLID:
                    assert (e & ~SOLID) < solids.size, "Solid index past solid_count"
                    vals.append(solids[[e & ~SOLID]])
                    corners.append(corner[None, :])
                    continue
                assert e < nb, "Parted index past brick_count"
                assert e not in seen_bricks, "a brick is reached twice"
                seen_bricks.add(e)
                bricks.append(e)
                vals.append(vox[e])
                corners.append(corner[None, :] + cell_xyz * np.uint64(cell))
        level, depth = nxt, depth + 1
    if not vals:
        return np.zeros(0, np.uint32), np.zeros((0, 3), np.uint64), bricks
    return np.concatenate(vals), np.concatenate(corners), bricks


def model_palette(img):
    """(the image with the canonical palette, map) -- map[ci] for every 16-bit index."""
    size, bd = int(img.boxtree_size), int(img.brick_dim)
    a = _arrays(img)
    pal = a["color_palette"]
    ncol = min(pal.size, NONE)
    vals, xyz, _ = walk(img)
    ci = (vals & np.uint32(NONE)).astype(np.int64)
    names = ci < ncol
    names[names] = (pal[ci[names]] >> np.uint32(24)) != 0
    S = np.uint64(size)
    index = (xyz[:, 0] * S + xyz[:, 1]) * S + xyz[:, 2]
    colours, inv = np.unique(pal[ci[names]], return_inverse=True)
    first = np.full(colours.size, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(first, inv, index[names])
    assert np.unique(first).size == first.size, "first indices are distinct"
    order = np.argsort(first, kind="stable")
    new_pal = colours[order].astype(np.uint32)
    rank = np.empty(colours.size, np.int64)
    rank[order] = np.arange(colours.size)
    mapping = np.full(1 << 16, NONE, np.uint32)
    for k in range(ncol):
        if (pal[k] >> np.uint32(24)) == 0:
            continue
        at = np.searchsorted(colours, pal[k])
        if at < colours.size and colours[at] == pal[k]:
            mapping[k] = rank[at]
    out = dict(a)
    for name in ("voxels", "solid_values"):
        v = a[name]
        out[name] = (v & np.uint32(0xFFFF0000)) | mapping[v & np.uint32(NONE)]
    out["color_palette"] = new_pal
    return TreeImage(size, bd, out), mapping


def scramble_palette(img, rng, duplicates=3, unused=4, transparent=2):
    """The same voxels under a palette that is not canonical: up to `duplicates` entries get a second entry of the same
    colour, and about half of the cells and solid values that named the first name the second; `unused` entries no value
    names; `transparent` entries of alpha 0, which about one in eight of the cells that were VHX_EMPTY now names (with
    no data, so they still point to empty); and all of it permuted. Emptiness, colours and data halves of every voxel
    stay (assert_same_voxels)."""
    a = _arrays(img)
    pal = a["color_palette"]
    n = pal.size
    d = min(duplicates, n)
    dup_of = rng.permutation(n)[:d]
    fresh = (np.arange(unused, dtype=np.uint32) * np.uint32(0x010203) + np.uint32(0x00A1B2C3)) | np.uint32(0xFF000000)
    assert not np.isin(fresh, pal).any()
    clear = (np.arange(transparent, dtype=np.uint32) + np.uint32(0x00112233)) & np.uint32(0x00FFFFFF)
    pre = np.concatenate([pal, pal[dup_of], fresh, clear]).astype(np.uint32)
    second = np.full(1 << 16, -1, np.int64)
    second[dup_of] = n + np.arange(d)
    perm = rng.permutation(pre.size)
    new_pal = np.empty(pre.size, np.uint32)
    new_pal[perm] = pre

    def moved(v, allow_clear):
        v = v.copy()
        ci = (v & np.uint32(NONE)).astype(np.int64)
        named = ci < n
        swap = named & (second[np.minimum(ci, NONE)] >= 0) & (rng.random(v.size) < 0.5)
        ci[swap] = second[ci[swap]]
        if allow_clear and transparent:
            hole = (v == np.uint32(EMPTY)) & (rng.random(v.size) < 1 / 8)
            ci[hole] = n + d + unused + rng.integers(0, transparent, int(hole.sum()))
            named = named | hole
        v[named] = (v[named] & np.uint32(0xFFFF0000)) | perm[ci[named]].astype(np.uint32)
        return v

    out = dict(a)
    out["voxels"] = moved(a["voxels"], True)
    out["solid_values"] = moved(a["solid_values"], False)
    out["color_palette"] = new_pal
    return TreeImage(int(img.boxtree_size), int(img.brick_dim), out)
