"""The numpy model of vhx_set_voxels (tests/_points_model.py) against the host BoxTree: the same list applied by the
sequential insert / clear loop gives the same voxels, resolved through the palettes, and the same palettes. This pins
the contract the GPU tests check (tests/test_gpu_set_voxels.py) to the reference's semantics, without a GPU."""
import numpy as np
import pytest

from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests._points_model import PointsModel, random_points

COLOURS = list(G.COLORS) + [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3), G.rgba(5, 5, 5)]
VALUES = list(DG.DATA_VALUES) + [11, 0x7FFFFFFF]


def tree_cubes(tree, size):
    vis = np.zeros((size,) * 3, np.uint32)
    dat = np.zeros((size,) * 3, np.uint32)
    for z in range(size):
        for y in range(size):
            for x in range(size):
                e = tree.get((x, y, z))
                if e.is_some():
                    alb = e.albedo()
                    vis[z, y, x] = 0 if alb is None or alb.is_transparent() else alb.packed()
                    dat[z, y, x] = e.data() or 0
    return vis, dat


def loop(tree, pos, a, d, mode):
    for (x, y, z), aw, dw in zip(pos.tolist(), a.tolist(), d.tolist()):
        entry = DG.entry_of(aw, dw)
        if entry is not None:
            tree.insert((x, y, z), entry)
        elif mode == "replace":
            tree.clear((x, y, z))


@pytest.mark.parametrize("size,bd", [(16, 4), (16, 1)])
@pytest.mark.parametrize("mode", ["replace", "insert"])
def test_the_model_is_the_sequential_loop(size, bd, mode):
    g, d = DG.make_pair("sparse", size)
    tree = DG.insert_tree(g, d, size, bd)
    flat = tree.flatten()
    model = PointsModel(DG.extend(DG.visible(g), size), DG.extend(d, size), flat.color_palette, flat.data_palette)
    vis, dat = tree_cubes(tree, size)
    assert np.array_equal(vis, model.vis) and np.array_equal(dat, model.dat)
    rng = np.random.default_rng(size + bd)
    for k in range(3):
        pos, a, dd = random_points(rng, size, 300, COLOURS, VALUES, hi=(size, size, 6) if k == 1 else None)
        pos[-6:] = pos[10]  # the list ends with one voxel five times: write, clear, write again ...
        a[-6:-1] = [COLOURS[5], 0, COLOURS[6], 0, COLOURS[7]]
        dd[-6:-1] = [0, 0, 77, 0, 0] if k else [0, 0, 77, 0, 78]
        a[-1], dd[-1] = 0, 0  # ... and a point without an entry
        loop(tree, pos, a, dd, mode)
        model.apply(pos, a, dd, mode)
        vis, dat = tree_cubes(tree, size)
        assert np.array_equal(vis, model.vis), f"{mode} list {k}: colours"
        assert np.array_equal(dat, model.dat), f"{mode} list {k}: data values"
        x, y, z = pos[-1].tolist()
        assert (model.vis[z, y, x] == 0) == (mode == "replace")
        flat = tree.flatten()
        assert list(flat.color_palette) == model.colors, f"{mode} list {k}: colour palette"
        assert list(flat.data_palette) == model.values, f"{mode} list {k}: data palette"
        # get through the palettes: the model's value names the voxel's colour and data value
        val = model.val()
        hit = val != np.uint32(0xFFFFFFFF)
        assert np.array_equal(hit, (model.vis != 0) | (model.dat != 0))
        ci, di = val[hit] & 0xFFFF, val[hit] >> 16
        cp, dp = np.array(model.colors + [0], np.uint32), np.array(model.values + [0], np.uint32)
        assert np.array_equal(np.where(ci == 0xFFFF, 0, cp[np.minimum(ci, cp.size - 1)]), model.vis[hit])
        assert np.array_equal(np.where(di == 0xFFFF, 0, dp[np.minimum(di, dp.size - 1)]), model.dat[hit])


def test_scalar_fills_and_a_batched_clear():
    model = PointsModel(np.zeros((8,) * 3, np.uint32), np.zeros((8,) * 3, np.uint32), [], [])
    pos = np.array([[1, 2, 3], [4, 5, 6], [1, 2, 3]], np.uint32)
    model.apply(pos, int(COLOURS[0]), 9)
    assert model.vis[3, 2, 1] == COLOURS[0] and model.dat[6, 5, 4] == 9 and model.colors == [int(COLOURS[0])]
    assert model.val()[3, 2, 1] == 0
    model.apply(pos[:1], 0, 0, "insert")  # no entry: nothing happens
    assert model.vis[3, 2, 1] == COLOURS[0]
    model.apply(pos[:1])  # the batched clear
    assert model.vis[3, 2, 1] == 0 and model.dat[3, 2, 1] == 0 and model.vis[6, 5, 4] == COLOURS[0]
    assert model.colors == [int(COLOURS[0])] and model.values == [9]
