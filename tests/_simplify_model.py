"""Simplification of a flattened image restated in numpy, independent of the C++ (vhx_flat_simplify, which goes through
the host BoxTree) and of the device pass (vhx_simplify_tree).

The rules (include/vhx_boxtree.h). points_to_empty(v): colour index v & 0xFFFF, data index v >> 16; the
colour is none when the index is 0xFFFF, past the palette or names alpha 0, the data is none when the index is 0xFFFF, past
the palette or names 0; both none. Reachability and numbering as compaction, except that an Internal node with
occupied_bits 0 becomes Nothing and reaches nothing. UniformLeaf: Solid v pointing to empty makes the node Nothing; a Parted
brick of one value v becomes VHX_EMPTY or Solid v. Leaf: per entry the same (a Solid v pointing to empty becomes empty);
then (a) 64 equal Solid entries: UniformLeaf over that brick, (b) brick_dim 1: stays, (c) every aligned 4x4x4 block of the
leaf's voxels (empty reads 0xFFFFFFFF) equal to its corner: UniformLeaf over a new Parted brick of the block corners.
solid_values: the distinct values of the Solid entries that remain, by first (new node, sectant)."""
import numpy as np

from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import TREE_ARRAYS, TreeImage

EMPTY = N.VHX_EMPTY
SOLID = N.VHX_SOLID_BIT


def points_to_empty(v, colors, data):
    ci, di = v & 0xFFFF, v >> 16
    cn = ci == 0xFFFF or ci >= len(colors) or (int(colors[ci]) >> 24) == 0
    dn = di == 0xFFFF or di >= len(data) or int(data[di]) == 0
    return cn and dn


def model_simplify(img):
    bd = int(img.brick_dim)
    n3 = bd ** 3
    a = {name: np.array(getattr(img, name), dt) for name, dt in TREE_ARRAYS}
    types, ch, occ = a["node_type"], a["node_children"].reshape(-1, 64), a["node_ocbits"]
    vox = a["voxels"].reshape(-1, n3)
    solids, colors, data = a["solid_values"], a["color_palette"], a["data_palette"]
    nn, nb = types.size, vox.shape[0]

    def pte(v):
        return points_to_empty(int(v), colors, data)

    # breadth-first walk; an Internal node without occupied bits reaches nothing
    order, new_of, level = [0], {0: 0}, [0]
    while level:
        nxt = []
        for o in level:
            if types[o] != N.VHX_NODE_INTERNAL or occ[o] == 0:
                continue
            for s in range(64):
                e = int(ch[o, s])
                if e == EMPTY:
                    continue
                assert e < nn and e not in new_of
                new_of[e] = len(order)
                order.append(e)
                nxt.append(e)
        level = nxt

    def entry(e):
        """("empty",), ("solid", v) or ("parted", cells) of an old entry after brick_simplify."""
        if e == EMPTY:
            return ("empty",)
        if e & SOLID:
            v = int(solids[e & ~SOLID])
            return ("empty",) if pte(v) else ("solid", v)
        assert e < nb
        cells = vox[e]
        if (cells == cells[0]).all():
            v = int(cells[0])
            return ("empty",) if pte(v) else ("solid", v)
        return ("parted", cells)

    out_type, out_occ, out_ch, bricks, solid_index, solid_values = [], [], [], [], {}, []

    def desc(b):
        if b[0] == "empty":
            return EMPTY
        if b[0] == "solid":
            if b[1] not in solid_index:
                solid_index[b[1]] = len(solid_values)
                solid_values.append(b[1])
            return SOLID | solid_index[b[1]]
        bricks.append(b[1])
        return len(bricks) - 1

    for o in order:
        t, row = int(types[o]), np.full(64, EMPTY, np.uint32)
        if t == N.VHX_NODE_INTERNAL:
            if occ[o] == 0:
                t = N.VHX_NODE_NOTHING
            else:
                for s in range(64):
                    if ch[o, s] != EMPTY:
                        row[s] = new_of[int(ch[o, s])]
        elif t == N.VHX_NODE_UNIFORM_LEAF:
            e = int(ch[o, 0])
            b = entry(e)
            if e != EMPTY and e & SOLID and b[0] == "empty":
                t = N.VHX_NODE_NOTHING
            else:
                row[0] = desc(b)
        elif t == N.VHX_NODE_LEAF:
            bs = [entry(int(e)) for e in ch[o]]
            if all(b[0] == "solid" and b[1] == bs[0][1] for b in bs):
                t = N.VHX_NODE_UNIFORM_LEAF
                row[0] = desc(bs[0])
            else:
                uniform = bd > 1
                if uniform:
                    L = 4 * bd
                    cube = np.empty((L, L, L), np.uint32)  # [z, y, x]
                    for s, b in enumerate(bs):
                        x, y, z = (s & 3) * bd, ((s >> 2) & 3) * bd, (s >> 4) * bd
                        cube[z:z + bd, y:y + bd, x:x + bd] = (b[1].reshape(bd, bd, bd) if b[0] == "parted"
                                                              else b[1] if b[0] == "solid" else EMPTY)
                    corners = cube[::4, ::4, ::4]
                    uniform = np.array_equal(corners.repeat(4, 0).repeat(4, 1).repeat(4, 2), cube)
                if uniform:
                    t = N.VHX_NODE_UNIFORM_LEAF
                    row[0] = desc(("parted", corners.reshape(-1).copy()))
                else:
                    for s, b in enumerate(bs):
                        row[s] = desc(b)
        else:
            t = N.VHX_NODE_NOTHING
        out_type.append(t)
        out_occ.append(occ[o])
        out_ch.append(row)
    a["node_type"] = np.asarray(out_type, np.uint32)
    a["node_ocbits"] = np.asarray(out_occ, np.uint64)
    a["node_children"] = np.concatenate(out_ch).astype(np.uint32)
    a["voxels"] = np.concatenate(bricks).astype(np.uint32) if bricks else np.zeros(0, np.uint32)
    a["solid_values"] = np.asarray(solid_values, np.uint32)
    return TreeImage(int(img.boxtree_size), bd, a)
