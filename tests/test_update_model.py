"""The numpy model of VHX_WRITE_UPDATE (tests/_update_model.py) against the host BoxTree: the same list applied by the
sequential loop `tree.update(position, entry)` gives the same voxels and the same palettes, on plain trees and on
simplified ones (Solid bricks, UniformLeaf nodes). This pins the contract the GPU tests check
(tests/test_gpu_update_voxels.py, tests/test_gpu_dense_update.py) to the reference's semantics, without a GPU."""
import numpy as np
import pytest

from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests import _simplify_grids as SG
from tests._points_model import random_points
from tests._update_model import UpdateModel

COLOURS = list(G.COLORS) + [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3), G.rgba(5, 5, 5)]
VALUES = list(DG.DATA_VALUES) + [11, 0x7FFFFFFF]


def tree_cubes(tree, size):
    """(vis, dat, flat image) of a host tree, from the list of its voxels."""
    flat = tree.flatten()
    pos, alb, dat = flat.list_voxels()
    vis, data = np.zeros((size,) * 3, np.uint32), np.zeros((size,) * 3, np.uint32)
    vis[pos[:, 2], pos[:, 1], pos[:, 0]] = alb
    data[pos[:, 2], pos[:, 1], pos[:, 0]] = dat
    return vis, data, flat


def plain(size, bd):
    g, d = DG.make_pair("sparse", size)
    return DG.insert_tree(g, d, size, bd)


def simplified(kind, size, bd):
    g = DG.extend(SG.make_grid(kind, size, bd), size)
    tree = DG.insert_tree(g, np.zeros_like(g), size, bd)
    tree.simplify(True)
    return tree


BASES = [("plain", 16, 4), ("plain", 16, 1), ("plain", 32, 2),
         ("full", 32, 2), ("brick_noise", 32, 2), ("blocks4", 32, 2), ("cut", 32, 2)]


@pytest.mark.parametrize("kind,size,bd", BASES)
def test_the_model_is_the_sequential_update_loop(kind, size, bd):
    tree = plain(size, bd) if kind == "plain" else simplified(kind, size, bd)
    vis, dat, flat = tree_cubes(tree, size)
    model = UpdateModel(vis, dat, flat.color_palette, flat.data_palette)
    rng = np.random.default_rng(size + bd)
    for k in range(3):
        pos, a, d = random_points(rng, size, 300, COLOURS, VALUES, hi=(size, size, 6) if k == 1 else None)
        pos[-6:] = pos[10]  # the list ends with one voxel six times: colour, data, colour, none, data, none
        a[-6:] = [COLOURS[5], 0, COLOURS[6], 0, 0, 0]
        d[-6:] = [0, 77, 0, 0, 78 + k, 0]
        for (x, y, z), aw, dw in zip(pos.tolist(), a.tolist(), d.tolist()):
            entry = DG.entry_of(aw, dw)
            if entry is not None:
                tree.update((x, y, z), entry)
        model.apply(pos, a, d, "update")
        vis, dat, flat = tree_cubes(tree, size)
        what = f"{kind} {size}/{bd} list {k}"
        assert np.array_equal(vis, model.vis), f"{what}: colours"
        assert np.array_equal(dat, model.dat), f"{what}: data values"
        assert list(flat.color_palette) == model.colors, f"{what}: colour palette"
        assert list(flat.data_palette) == model.values, f"{what}: data palette"
        x, y, z = pos[-1].tolist()
        assert model.vis[z, y, x] == COLOURS[6] and model.dat[z, y, x] == 78 + k, what
        e = tree.get((x, y, z))
        assert e.albedo().packed() == COLOURS[6] and e.data() == 78 + k, what


def test_halves_are_kept_and_a_point_without_one_touches_nothing():
    model = UpdateModel(np.zeros((8,) * 3, np.uint32), np.zeros((8,) * 3, np.uint32), [], [])
    pos = np.array([[1, 2, 3], [4, 5, 6]], np.uint32)
    model.apply(pos, int(COLOURS[0]), 9)
    model.apply(pos[:1], int(COLOURS[1]), None, "update")  # recoloured, the data value stays
    assert model.vis[3, 2, 1] == COLOURS[1] and model.dat[3, 2, 1] == 9
    model.apply(pos[1:], 0, 12, "update")  # retagged, the colour stays
    assert model.vis[6, 5, 4] == COLOURS[0] and model.dat[6, 5, 4] == 12
    model.apply(pos, 0, 0, "update")  # no half: nothing happens
    assert model.vis[3, 2, 1] == COLOURS[1] and model.dat[6, 5, 4] == 12
    model.apply(np.array([[0, 0, 0], [0, 0, 0]]), np.array([COLOURS[2], 0], np.uint32), np.array([0, 5], np.uint32), "update")
    assert model.vis[0, 0, 0] == COLOURS[2] and model.dat[0, 0, 0] == 5  # an empty voxel: Visual, then Complex
    assert model.colors == [int(COLOURS[0]), int(COLOURS[1]), int(COLOURS[2])] and model.values == [9, 12, 5]
    assert model.val()[0, 0, 0] == (2 | (2 << 16))
    box = UpdateModel(model.vis, model.dat, model.colors, model.values)
    box.apply_box(np.zeros((2, 2, 2), np.uint32), 7, (0, 0, 0), "update")  # fill_box(o, e, 0, 7, mode="update")
    assert box.vis[0, 0, 0] == COLOURS[2] and (box.dat[:2, :2, :2] == 7).all() and box.vis[1, 1, 1] == 0
