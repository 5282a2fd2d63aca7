"""BoxTree::get restated over a flattened image, vectorised in numpy: the independent reference of vhx_get_voxels and
vhx_read_dense (tests/test_flatget.py pins it against the host tree's get, tests/test_gpu_query.py the device against it).

It walks the seven arrays of a FlatTree or a TreeImage (Raytracer.download) exactly as get_internal does
(src/boxtree/mod.rs:247-317, get_node_internal in src/boxtree/iterate.rs:293-343), in the reference's f32 arithmetic:
Cube::contains, sectant_for / offset_sectant (src/spatial/mod.rs:54-69, src/spatial/math/mod.rs:27-44), child_bounds_for
(src/spatial/mod.rs:72-77) and matrix_index_for (src/spatial/math/mod.rs:64-95). pix_points_to_empty
(src/boxtree/node.rs:311-333) is computed from the palettes, never from a derived device buffer."""
import numpy as np

from voxelhex_amd import _native as N

f32 = np.float32
EMPTY = np.uint32(N.VHX_EMPTY)
# SECTANT_OFFSET_LUT (src/spatial/lut.rs): sectant s sits at (s & 3, (s >> 2) & 3, s >> 4) / 4 of its node
_S = np.arange(64)
SECTANT_OFFSET = (np.stack([_S & 3, (_S >> 2) & 3, _S >> 4], 1) / 4).astype(f32)


def sectant_for(bmin, bsize, p):
    """Cube::sectant_for: offset_sectant(position - min_position, size), all f32."""
    off = p - bmin
    idx = np.floor((off * f32(4)) / bsize[:, None])
    idx = np.minimum(idx, f32(3))
    return (idx[:, 0] + (idx[:, 1] * f32(4)) + (idx[:, 2] * f32(16))).astype(np.uint8).astype(np.int64)


def child_bounds_for(bmin, bsize, s):
    return bmin + SECTANT_OFFSET[s] * bsize[:, None], bsize / f32(4)


def matrix_index_for(bmin, bsize, p, bd):
    """matrix_index_for, then flat_projection: x + y * dim + z * dim^2."""
    m = np.floor(((p - bmin) * f32(bd)) / bsize[:, None]).astype(np.int64)
    return m[:, 0] + m[:, 1] * bd + m[:, 2] * bd * bd


def points_to_empty(image, v):
    """NodeContent::pix_points_to_empty over the image's palettes (an index past a palette counts as none, as on the
    host tree)."""
    v = np.asarray(v, np.uint32)
    ci, di = (v & 0xFFFF).astype(np.int64), (v >> 16).astype(np.int64)
    cp, dp = image.color_palette, image.data_palette
    cn = (ci == 0xFFFF) | (ci >= cp.size)
    if cp.size:
        cn |= (cp[np.minimum(ci, cp.size - 1)] >> 24) == 0
    dn = (di == 0xFFFF) | (di >= dp.size)
    if dp.size:
        dn |= dp[np.minimum(di, dp.size - 1)] == 0
    return cn & dn


def flat_get(image, positions):
    """get_internal(ROOT, root_bounds, position) for every row (x, y, z) of `positions`: uint32 PaletteIndexValues,
    VHX_EMPTY = none."""
    size, bd = int(image.boxtree_size), int(image.brick_dim)
    n3 = bd ** 3
    types, children = image.node_type, image.node_children
    pos = np.asarray(positions).reshape(-1, 3)
    out = np.full(pos.shape[0], EMPTY, np.uint32)
    pf = pos.astype(np.uint32).astype(f32)  # V3c::<f32>::from(position)
    at = np.flatnonzero((pf < f32(size)).all(1))  # Cube::contains on the root (positions are unsigned: >= 0 holds)
    p = pf[at]
    node = np.zeros(at.size, np.int64)
    bmin = np.zeros((at.size, 3), f32)
    bsize = np.full(at.size, f32(size), f32)
    # get_node_internal: down while the node is Internal and its child at the position's sectant is a valid key
    walk = np.arange(at.size)
    while walk.size:
        walk = walk[types[node[walk]] == N.VHX_NODE_INTERNAL]
        s = sectant_for(bmin[walk], bsize[walk], p[walk])
        child = children[node[walk] * 64 + s]
        ok = (child != EMPTY) & (child < types.size)
        walk, s, child = walk[ok], s[ok], child[ok]
        bmin[walk], bsize[walk] = child_bounds_for(bmin[walk], bsize[walk], s)
        node[walk] = child
    res = np.full(at.size, EMPTY, np.uint32)
    ty = types[node]
    # Leaf: the brick of the position's sectant
    k = np.flatnonzero(ty == N.VHX_NODE_LEAF)
    s = sectant_for(bmin[k], bsize[k], p[k])
    desc = children[node[k] * 64 + s]
    solid = (desc != EMPTY) & ((desc & N.VHX_SOLID_BIT) != 0)
    res[k[solid]] = image.solid_values[desc[solid] & 0x7FFFFFFF]
    parted = (desc & N.VHX_SOLID_BIT) == 0
    kp, sp, dp = k[parted], s[parted], desc[parted].astype(np.int64)
    cmin, csize = child_bounds_for(bmin[kp], bsize[kp], sp)
    v = image.voxels[dp * n3 + matrix_index_for(cmin, csize, p[kp], bd)] if kp.size else np.zeros(0, np.uint32)
    res[kp] = np.where(points_to_empty(image, v), EMPTY, v)
    # UniformLeaf: its one brick over the node's bounds, a Parted brick's cell returned as it is
    k = np.flatnonzero(ty == N.VHX_NODE_UNIFORM_LEAF)
    desc = children[node[k] * 64]
    solid = (desc != EMPTY) & ((desc & N.VHX_SOLID_BIT) != 0)
    res[k[solid]] = image.solid_values[desc[solid] & 0x7FFFFFFF]
    parted = (desc & N.VHX_SOLID_BIT) == 0
    kp, dp = k[parted], desc[parted].astype(np.int64)
    if kp.size:
        res[kp] = image.voxels[dp * n3 + matrix_index_for(bmin[kp], bsize[kp], p[kp], bd)]
    out[at] = res
    return out


def flat_albedo(image, values):
    """What vhx_read_dense writes for a value: color_palette[c] for c = v & 0xFFFF if v is not VHX_EMPTY, c is neither
    0xFFFF nor past the palette and the colour's alpha byte is not 0; else 0."""
    v = np.asarray(values, np.uint32)
    cp = image.color_palette
    c = (v & 0xFFFF).astype(np.int64)
    ok = (v != EMPTY) & (c != 0xFFFF) & (c < cp.size)
    if not cp.size:
        return np.zeros(v.shape, np.uint32)
    col = cp[np.minimum(c, cp.size - 1)]
    return np.where(ok & ((col >> 24) != 0), col, np.uint32(0)).astype(np.uint32)


def lattice(origin, extents):
    """Every position of a box as (n, 3) uint32 rows in the order of a dense grid of shape (gz, gy, gx)."""
    (ox, oy, oz), (gx, gy, gz) = origin, extents
    z, y, x = np.meshgrid(np.arange(oz, oz + gz, dtype=np.uint32), np.arange(oy, oy + gy, dtype=np.uint32),
                          np.arange(ox, ox + gx, dtype=np.uint32), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def seeded_positions(size, n, seed):
    return np.random.default_rng(seed).integers(0, size, (n, 3), dtype=np.int64).astype(np.uint32)
