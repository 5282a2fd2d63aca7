"""vhx_write_dense and vhx_write_dense_data with VHX_WRITE_UPDATE on the GPU (Raytracer.write_dense / fill_box with
mode="update"): a box merged into the device tree in place, each voxel of the box writing only the halves (colour, data
value) it has. The expected cubes and palettes are kept by the numpy model (tests/_update_model.py: the box as a list in
its insert order); after every call the checks of tests/test_gpu_set_voxels.Model.check run. Every comparison is bit for
bit."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _update_gpu as U
from tests.test_gpu_dense_data_write import SIZES, odd_box, random_box

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
COLOURS, VALUES = U.COLOURS, U.VALUES
to_device = U.to_device


@pytest.fixture(scope="module")
def second():
    """A second context that uploads downloaded images: the derived state as an upload derives it."""
    rt = vhx.Raytracer(0)
    yield rt
    rt.close()


# --------------------------------------------------------------------------------------- sizes, boxes and sources
@pytest.mark.parametrize("source", ["host", "tensor"])
@pytest.mark.parametrize("size,bd", SIZES)
def test_boxes_into_a_data_base(gpu, oracle, second, size, bd, source):
    what = f"{size}/{bd} {source}"
    m = U.data_base(gpu, size, bd)
    rng = np.random.default_rng(size * 10 + bd)
    origin, extents = odd_box(size)  # (13, 15, 3) + (22, 18, 35) at 64: off the brick grid, across leaves and nodes
    ox, oy, oz = origin
    sl = (slice(oz, oz + extents[2]), slice(oy, oy + extents[1]), slice(ox, ox + extents[0]))
    g, d = random_box(rng, extents)  # a colour plane with holes and a data plane with holes
    m.write(g, d, origin, "update", source)
    m.check(oracle, second, f"{what}: both planes")
    g = random_box(rng, extents, 0.5)[0]
    old = m.dat.copy()
    m.write(g, None, origin, "update", source)  # no data plane: recoloured, the data values under the box stay
    m.check(oracle, second, f"{what}: a colour plane alone")
    assert np.array_equal(m.dat, old), what
    if np.prod(extents) >= 40:
        assert ((g >> 24 != 0) & (m.dat[sl] != 0)).any(), f"{what}: no recoloured voxel with a data value"
    m.write(g, 12345, (0, 0, 0), "update", source)  # a colour plane with fill_data: every voxel of the box is retagged
    m.check(oracle, second, f"{what}: a colour plane with fill_data")
    old_vis = m.vis.copy()
    m.fill(origin, extents, 0, 7)  # every voxel of the box gets 7; occupied ones keep their colour
    m.check(oracle, second, f"{what}: fill_box with a data value alone")
    assert np.array_equal(m.vis, old_vis) and (m.dat[sl] == 7).all(), what
    if np.prod(extents) >= 40:
        assert (m.vis[sl] == 0).any() and (m.vis[sl] != 0).any(), f"{what}: Informative and Complex voxels"
    old_dat = m.dat.copy()
    m.fill((0, 0, 0), (max(1, size // 2),) * 3, int(COLOURS[5]), 0)  # recoloured; the data values stay
    m.check(oracle, second, f"{what}: fill_box with a colour alone")
    assert np.array_equal(m.dat, old_dat) and (m.vis[: max(1, size // 2), : max(1, size // 2), : max(1, size // 2)]
                                               == COLOURS[5]).all(), what
    before = gpu.download()
    m.fill(origin, extents, int(G.rgba(4, 4, 4, 0)), 0)  # neither half: nothing is touched
    m.write(np.zeros((3, 2, 1), np.uint32), np.zeros((3, 2, 1), np.uint32), (0, 0, 0), "update", source)
    G.assert_same_image(gpu.download(), before, f"{what}: a box without a half")


@pytest.mark.parametrize("size,bd", SIZES)
def test_into_an_empty_tree(gpu, oracle, second, size, bd):
    what = f"{size}/{bd}"
    gpu.build_dense(G.make_grid("zero", size), size, bd)
    m = U.Model(gpu, size, bd)
    origin, extents = odd_box(size)
    m.write(*random_box(np.random.default_rng(size + bd), extents), origin)  # update of empty voxels is an insert
    img = m.check(oracle, second, f"{what}: a box into the empty tree")
    assert gpu.orphans() == (0, 0) and img.desc.data_count > 0


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8), (16, 1)])
@pytest.mark.parametrize("kind", ["full", "brick_noise", "blocks4", "cut"])
def test_simplified_bases(gpu, oracle, second, kind, size, bd):
    what = f"{kind} {size}/{bd}"
    g, d = U.simplified_pair(kind, size, bd)
    gpu.build_dense(g, size, bd, simplify=True, data=d)
    old = gpu.download()
    m = U.Model(gpu, size, bd)
    origin, extents = odd_box(size)
    rng = np.random.default_rng(size)
    m.write(*random_box(rng, extents, 0.3), origin, "update", "tensor")
    img = m.check(oracle, second, f"{what}: both planes")
    assert np.array_equal(img.solid_values, old.solid_values), what
    before = m.vis.copy()
    m.fill((1, 2, 3), (size - 2, 3, size - 5), 0, 4040)  # a slab of data values across Solid bricks and UniformLeaf nodes
    m.check(oracle, second, f"{what}: a data fill")
    assert np.array_equal(m.vis, before) and (m.dat == 4040).sum() == (size - 2) * 3 * (size - 5), what
    before = m.dat.copy()
    m.write(random_box(rng, (size, 3, size), 0.5)[0], None, (0, size - 3, 0))  # colours alone
    m.check(oracle, second, f"{what}: a colour plane alone")
    assert np.array_equal(m.dat, before), what


# ------------------------------------------------------------------------------------- differential: update / insert
@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8)])
def test_structure_and_numbering_are_those_of_insert(gpu, size, bd):
    what = f"{size}/{bd}"
    rng = np.random.default_rng(size + 2)
    origin, extents = odd_box(size)
    g, d = random_box(rng, extents)
    both = (g >> 24 != 0) & (d != 0)  # the entry voxels all carry both halves
    g, d = np.where(both, g, 0).astype(np.uint32), np.where(both, d, 0).astype(np.uint32)
    bg, bdat = U.data_pair(size)
    images = {}
    for base in ("data", "plain"):
        for mode in ("update", "insert"):
            for data in (d, None):
                gpu.build_dense(bg, size, bd, data=bdat if base == "data" else None)
                gpu.write_dense(to_device(g), origin, mode, data=None if data is None else to_device(data))
                images[base, mode, data is None] = (gpu.download(), gpu.orphans())
    for base in ("data", "plain"):
        G.assert_same_image(images[base, "update", False][0], images[base, "insert", False][0], f"{what} {base}: both")
        assert images[base, "update", False][1] == images[base, "insert", False][1], what
    G.assert_same_image(images["plain", "update", True][0], images["plain", "insert", True][0], f"{what}: colours")
    up, ins = images["data", "update", True][0], images["data", "insert", True][0]  # insert drops data, update keeps it
    for k in ("node_type", "node_ocbits", "node_children", "color_palette", "data_palette", "solid_values"):
        assert np.array_equal(getattr(up, k), getattr(ins, k)), f"{what}: {k}"
    assert up.voxels.shape == ins.voxels.shape and not np.array_equal(up.voxels, ins.voxels), what
    assert np.array_equal(up.voxels & 0xFFFF, ins.voxels & 0xFFFF), f"{what}: the colour halves"


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8)])
def test_a_point_list_and_its_sparse_box_give_the_same_cubes(gpu, size, bd):
    what = f"{size}/{bd}"
    rng = np.random.default_rng(size + 3)
    origin, extents = odd_box(size)
    g, d = random_box(rng, extents, 0.1)
    ox, oy, oz = origin
    z, y, x = np.nonzero((g >> 24 != 0) | (d != 0))
    pos = np.stack([x + ox, y + oy, z + oz], 1).astype(np.uint32)
    cubes = []
    for route in ("points", "box"):
        U.data_base(gpu, size, bd)
        if route == "points":
            gpu.update_voxels(pos, g[z, y, x], d[z, y, x])
        else:
            gpu.write_dense(g, origin, "update", data=d)
        # the palettes differ in order (list order against the box's insert order), so get is compared for "none" only
        cubes.append(gpu.read_dense(data=True) + (gpu.get(U.positions(size)) == EMPTY,))
    for a, b, name in zip(cubes[0], cubes[1], ("the albedo plane", "the data plane", "the voxels that are none")):
        assert np.array_equal(a, b), f"{what}: {name}"


# -------------------------------------------------------------------------------- closure with simplify and palettes
@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8)])
def test_closure_with_simplification(gpu, size, bd):
    what = f"{size}/{bd}"
    m = U.data_base(gpu, size, bd)
    rng = np.random.default_rng(77)
    origin, extents = odd_box(size)
    m.write(*random_box(rng, extents), origin)
    m.fill((0, 0, 0), (size // 2,) * 3, int(G.COLORS[0]), 9)  # whole bricks and leaves of one value in both halves
    m.fill((0, 0, 0), (size // 4,) * 3, 0, 10)  # retagged, still one colour
    m.write(random_box(rng, (size, 5, 7), 0.2, new=False)[0], None, (0, 1, 2), "update", "tensor")
    gpu.simplify()
    gpu.compact_palettes()
    host = FlatTree.from_dense(m.vis, size, bd, simplify=True, data=m.dat)
    G.assert_same_image(gpu.download(), host, f"{what}: against the host build of the model's cubes")
    assert gpu.orphans() == (0, 0)


def test_fill_box_keeps_its_default(gpu):
    size, bd = 16, 4
    m = U.data_base(gpu, size, bd)
    gpu.fill_box((1, 1, 1), (5, 5, 5), int(COLOURS[0]), 0)  # replace: the data values under the box are dropped
    a, p = gpu.read_dense((1, 1, 1), (5, 5, 5), data=True)
    assert (a == COLOURS[0]).all() and not p.any() and m.dat[1:6, 1:6, 1:6].any()
