"""The order of vhx_list_voxels restated in numpy: the key formula of include/vhx.h and nothing else. From the (albedo,
data) planes of a box, as read_dense(data=True) gives them, it lists the voxels that have either word, ascending in key."""
import numpy as np


def key(pos, size, bd):
    """key(x, y, z) of every row of `pos`: the sectant digits of the nodes from the root (size wide) down to the smallest
    leaf (4 * bd wide), the root's most significant, then the flat cell index inside the brick. uint64: trees of up to
    2^21 an edge."""
    lg_size, lg_bd = int(size).bit_length() - 1, int(bd).bit_length() - 1
    assert 1 << lg_size == size and 1 << lg_bd == bd and (lg_size - lg_bd) % 2 == 0 and 3 * lg_size <= 63
    x, y, z = (np.asarray(pos)[:, i].astype(np.uint64) for i in range(3))
    k = np.zeros(x.shape, np.uint64)
    for lg in range(lg_size, lg_bd, -2):  # a node 2^lg wide: bits lg-2 .. lg-1 of each coordinate
        sh = np.uint64(lg - 2)
        three = np.uint64(3)
        digit = ((x >> sh) & three) | (((y >> sh) & three) << np.uint64(2)) | (((z >> sh) & three) << np.uint64(4))
        k = (k << np.uint64(6)) | digit
    m = np.uint64(bd - 1)
    flat = (x & m) + (y & m) * np.uint64(bd) + (z & m) * np.uint64(bd * bd)
    return (k << np.uint64(3 * lg_bd)) | flat


def expected(vis, dat, size, bd, origin=(0, 0, 0)):
    """(positions (n, 3), albedo (n,), data (n,)), uint32, of the box whose planes `vis` and `dat` (shape (gz, gy, gx))
    sit at `origin` (x, y, z) of a tree `size` wide with bricks of `bd`."""
    z, y, x = np.nonzero((vis != 0) | (dat != 0))
    pos = np.stack([x + origin[0], y + origin[1], z + origin[2]], 1).astype(np.uint32)
    order = np.argsort(key(pos, size, bd), kind="stable")
    return pos[order], vis[z, y, x][order].astype(np.uint32), dat[z, y, x][order].astype(np.uint32)


def expected_box(vis, dat, size, bd, origin, extents):
    """The same for a box of planes that cover the whole root cube."""
    (ox, oy, oz), (gx, gy, gz) = origin, extents
    return expected(vis[oz:oz + gz, oy:oy + gy, ox:ox + gx], dat[oz:oz + gz, oy:oy + gy, ox:ox + gx], size, bd, origin)
