"""vhx_build_tree_dense: the tree of a dense grid built on the GPU equals the host bulk builder's image
(FlatTree.from_dense, itself pinned against the insert loop in tests/test_dense_build.py) in all seven buffers and all
counts, from a device tensor and from a host array; the built tree traces like the oracle on the host image; builds
on one context leave no state behind, and a failing build leaves the previous tree traceable."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G

pytestmark = pytest.mark.gpu

_host = {}


def host_image(key, grid, size, bd):
    """The reference image of a grid, computed once per session."""
    if key not in _host:
        _host[key] = FlatTree.from_dense(grid, size, bd)
    return _host[key]


def as_source(grid, source):
    if source == "host":
        return grid
    import torch
    return torch.from_numpy(grid.view(np.int32)).to("cuda:0")


def bits(frame):
    return {k: np.ascontiguousarray(v).view(np.uint32) for k, v in frame.items()}


def assert_same_frame(got, want, what):
    got, want = bits(got), bits(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.count_nonzero(got[k] != want[k])} entries"


@pytest.mark.parametrize("source", ["tensor", "host"])
@pytest.mark.parametrize("size,bd", G.SIZES)
@pytest.mark.parametrize("kind", G.KINDS)
def test_device_build_equals_host_build(gpu, kind, size, bd, source):
    grid = G.make_grid(kind, size)
    gpu.build_dense(as_source(grid, source), size, bd)
    G.assert_same_image(gpu.download(), host_image((kind, size, bd), grid, size, bd), f"{kind} {size}/{bd} {source}")


@pytest.mark.parametrize("source", ["tensor", "host"])
def test_palette_order_and_table_collisions(gpu, source):
    grid, want = G.palette_order_grid()
    gpu.build_dense(as_source(grid, source), 4, 1)
    img = gpu.download()
    assert img.color_palette.tolist() == [int(c) for c in want]
    G.assert_same_image(img, host_image("order", grid, 4, 1), "palette order")
    grid = G.many_colors_grid()
    gpu.build_dense(as_source(grid, source), 64, 4)
    G.assert_same_image(gpu.download(), host_image("many", grid, 64, 4), "5000 colours")


@pytest.mark.parametrize("source", ["tensor", "host"])
def test_device_build_at_256(gpu, source):
    """D = 2 with 4096 possible leaves and more than one scan tile: a sparse 64 MiB grid in a 256^3 tree."""
    rng = np.random.default_rng(256)
    grid = np.zeros((256, 256, 256), np.uint32)
    mask = rng.random(grid.shape) < 1 / 40
    grid[mask] = G.COLORS[rng.integers(0, len(G.COLORS), int(mask.sum()))]
    grid[:, :, 100:200] = 0   # whole leaves and interior nodes empty
    grid[64:128] = 0
    grid[:, 129:] = 0
    host = host_image("256", grid, 256, 4)
    assert host.desc.node_count > 1024 and host.desc.brick_count > 1024  # the image is not trivial: several scan tiles
    gpu.build_dense(as_source(grid, source), 256, 4)
    G.assert_same_image(gpu.download(), host, f"256/4 {source}")


def test_built_tree_traces_like_the_oracle(oracle):
    size, bd, W = 64, 4, 64
    grid = G.make_grid("sparse", size, seed=5)
    host = host_image(("frame", size, bd), grid, size, bd)
    cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
    want = oracle.trace_primary(host, cam, 0, 0, W, W)
    assert (want["value"] != N.VHX_EMPTY).sum() > 500
    rt = vhx.Raytracer(0)
    try:
        rt.upload(FlatTree.from_dense(G.make_grid("corner", 16), 16, 1))
        sh = rt.shared()  # created before the build: it traces the owner's new tree afterwards
        rt.build_dense(as_source(grid, "tensor"), size, bd)
        assert_same_frame(rt.trace_primary(cam), want, "owner")
        assert_same_frame(sh.trace_primary(cam), want, "shared context")
        with pytest.raises(N.VhxError) as e:
            sh.build_dense(grid, size, bd)
        assert e.value.code == N.VHX_E_STATE
        assert_same_frame(sh.trace_primary(cam), want, "shared context after its refused build")
        sh.close()
    finally:
        rt.close()


def test_builds_in_sequence_on_one_context(oracle):
    """Stale scratch, a table that is not reset, or a failed build that damages the tree would show here."""
    W = 64
    rt = vhx.Raytracer(0)
    try:
        big = G.make_grid("sparse", 64, seed=1)
        rt.build_dense(as_source(big, "tensor"), 64, 4)  # 1
        G.assert_same_image(rt.download(), host_image(("seq1", 64, 4), big, 64, 4), "first build")
        small = G.make_grid("sparse", 32, seed=2)
        rt.build_dense(small, 32, 2)  # 2: smaller and different
        host2 = host_image(("seq2", 32, 2), small, 32, 2)
        G.assert_same_image(rt.download(), host2, "second build")
        cam = vhx.glass_camera(32, W, W, target=(16.0,) * 3)
        frame2 = rt.trace_primary(cam)
        assert_same_frame(frame2, oracle.trace_primary(host2, cam, 0, 0, W, W), "second build's frame")
        with pytest.raises(N.VhxError) as e:  # 3
            rt.build_dense(as_source(G.distinct_colors_grid(65600), "tensor"), 64, 4)
        assert e.value.code == N.VHX_E_CAPACITY
        assert N.lib().vhx_last_error(rt._h)
        assert_same_frame(rt.trace_primary(cam), frame2, "after the failed build")  # 4
        G.assert_same_image(rt.download(), host2, "after the failed build")
        third = G.distinct_colors_grid(65535)  # 5: the largest palette
        rt.build_dense(as_source(third, "tensor"), 64, 4)
        G.assert_same_image(rt.download(), host_image("seq3", third, 64, 4), "third build")
    finally:
        rt.close()


def test_read_back_errors():
    import ctypes
    rt = vhx.Raytracer(0)
    try:
        d = N.TreeDesc()
        assert N.lib().vhx_tree_counts(rt._h, ctypes.byref(d)) == N.VHX_E_STATE
        with pytest.raises(N.VhxError) as e:
            rt.read_range(N.VHX_BUF_NODE_TYPE, 0, 1)
        assert e.value.code == N.VHX_E_STATE
        grid = G.make_grid("sparse", 16)
        rt.build_dense(grid, 16, 1)
        c = rt.tree_counts()
        assert (c.boxtree_size, c.brick_dim, c.solid_count, c.data_count) == (16, 1, 0, 0) and not c.node_type
        assert rt.read_range(N.VHX_BUF_NODE_CHILDREN, 64 * (c.node_count - 1), 64).size == 64
        for buf, n in ((N.VHX_BUF_NODE_TYPE, c.node_count), (N.VHX_BUF_VOXELS, c.brick_count),
                       (N.VHX_BUF_SOLID_VALUES, 0)):
            with pytest.raises(N.VhxError) as e:
                rt.read_range(buf, n, 1)
            assert e.value.code == N.VHX_E_CAPACITY
        with pytest.raises(vhx.OctreeError):
            rt.build_dense(grid, 256, 8)
        with pytest.raises(N.VhxError) as e:
            rt.build_dense(np.zeros((4, 4, 17), np.uint32), 16, 1)
        assert e.value.code == N.VHX_E_INVALID_ARG
        G.assert_same_image(rt.download(), FlatTree.from_dense(grid, 16, 1), "after refused builds")
    finally:
        rt.close()
