"""vhx_build_tree_dense_simplified: the simplified tree of a dense grid built on the GPU equals the host image
(FlatTree.from_dense(simplify=True), pinned against BoxTree.simplify in tests/test_dense_simplify.py) in all seven buffers
and all counts, from a device tensor and from a host array; the built tree traces like the oracle on the host image; plain
and simplified builds on one context leave no state behind, and a failing build leaves the previous tree traceable."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _simplify_grids as S

pytestmark = pytest.mark.gpu

_host = {}


def host_image(key, grid, size, bd, simplify=True):
    """The reference image of a grid, computed once per session."""
    if key not in _host:
        _host[key] = FlatTree.from_dense(grid, size, bd, simplify=simplify)
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
@pytest.mark.parametrize("size,bd", S.SIZES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_device_build_equals_host_image(gpu, kind, size, bd, source):
    grid = S.make_grid(kind, size, bd)
    host = host_image((kind, size, bd), grid, size, bd)
    S.assert_case(kind, size, bd, host)
    gpu.build_dense(as_source(grid, source), size, bd, simplify=True)
    G.assert_same_image(gpu.download(), host, f"{kind} {size}/{bd} {source}")


@pytest.mark.parametrize("source", ["tensor", "host"])
def test_solid_values_follow_the_leaf_walk(gpu, source):
    grid, a, b = S.solid_order_grid()
    host = host_image("order", grid, 64, 4)
    assert host.color_palette.tolist() == [int(b), int(a)]
    assert host.solid_values.tolist() == [0xFFFF0000 | 1, 0xFFFF0000 | 0]  # not the palette's order
    gpu.build_dense(as_source(grid, source), 64, 4, simplify=True)
    G.assert_same_image(gpu.download(), host, f"solid order {source}")


@pytest.mark.parametrize("source", ["tensor", "host"])
def test_device_build_at_256(gpu, source):
    """D = 2 with 4096 possible leaves and more than one scan tile of Parted counts."""
    grid = S.noise_256()
    host = host_image("256", grid, 256, 4)
    uniform = int((host.node_type == N.VHX_NODE_UNIFORM_LEAF).sum())
    # the seeded grid's image, so that a drift of the generator shows: several scan tiles of nodes and of bricks
    assert (host.desc.node_count, host.desc.brick_count, uniform, host.desc.solid_count) == (1216, 8829, 11, 3)
    gpu.build_dense(as_source(grid, source), 256, 4, simplify=True)
    G.assert_same_image(gpu.download(), host, f"256/4 {source}")


@pytest.mark.parametrize("kind", ["brick_noise", "blocks4"])
def test_built_tree_traces_like_the_oracle(oracle, kind):
    size, bd, W = 64, 4, 64
    grid = S.make_grid(kind, size, bd)
    host = host_image((kind, size, bd), grid, size, bd)
    S.assert_case(kind, size, bd, host)
    cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
    want = oracle.trace_primary(host, cam, 0, 0, W, W)
    assert (want["value"] != N.VHX_EMPTY).sum() > 500
    rt = vhx.Raytracer(0)
    try:
        rt.upload(FlatTree.from_dense(G.make_grid("corner", 16), 16, 1))
        sh = rt.shared()  # created before the build: it traces the owner's new tree afterwards
        rt.build_dense(as_source(grid, "tensor"), size, bd, simplify=True)
        assert_same_frame(rt.trace_primary(cam), want, "owner")
        assert_same_frame(sh.trace_primary(cam), want, "shared context")
        with pytest.raises(N.VhxError) as e:
            sh.build_dense(grid, size, bd, simplify=True)
        assert e.value.code == N.VHX_E_STATE
        assert_same_frame(sh.trace_primary(cam), want, "shared context after its refused build")
        sh.close()
    finally:
        rt.close()


def test_too_many_colours_beside_solid_bricks():
    """The palette overflows in a grid that also holds Solid bricks and uniform leaves: the classification runs on a
    table that lacks colours, the build fails with VHX_E_CAPACITY and the previous tree stays."""
    rt = vhx.Raytracer(0)
    try:
        small = S.make_grid("brick_noise", 32, 2)
        rt.build_dense(small, 32, 2, simplify=True)
        for source in ("tensor", "host"):
            with pytest.raises(N.VhxError) as e:
                rt.build_dense(as_source(S.overflow_grid(), source), 64, 4, simplify=True)
            assert e.value.code == N.VHX_E_CAPACITY
            G.assert_same_image(rt.download(), host_image(("brick_noise", 32, 2), small, 32, 2), f"after {source}")
    finally:
        rt.close()


def test_plain_and_simplified_builds_in_sequence_on_one_context(oracle):
    """Stale scratch, a table that is not reset, or a failed build that damages the tree would show here."""
    W = 64
    rt = vhx.Raytracer(0)
    try:
        big = S.make_grid("brick_noise", 64, 4, seed=1)
        rt.build_dense(as_source(big, "tensor"), 64, 4)  # 1: plain
        G.assert_same_image(rt.download(), host_image(("seq1", 64, 4), big, 64, 4, simplify=False), "plain build")
        small = S.make_grid("blocks4", 32, 2, seed=2)
        rt.build_dense(small, 32, 2, simplify=True)  # 2: simplified, smaller and different
        host2 = host_image(("seq2", 32, 2), small, 32, 2)
        S.assert_case("blocks4", 32, 2, host2)
        G.assert_same_image(rt.download(), host2, "simplified build")
        cam = vhx.glass_camera(32, W, W, target=(16.0,) * 3)
        frame2 = rt.trace_primary(cam)
        assert_same_frame(frame2, oracle.trace_primary(host2, cam, 0, 0, W, W), "simplified build's frame")
        with pytest.raises(N.VhxError) as e:  # 3: fails
            rt.build_dense(as_source(G.distinct_colors_grid(65600), "tensor"), 64, 4, simplify=True)
        assert e.value.code == N.VHX_E_CAPACITY
        assert N.lib().vhx_last_error(rt._h)
        assert_same_frame(rt.trace_primary(cam), frame2, "after the failed build")
        G.assert_same_image(rt.download(), host2, "after the failed build")
        rt.build_dense(as_source(big, "tensor"), 64, 4)  # 4: plain again
        G.assert_same_image(rt.download(), host_image(("seq1", 64, 4), big, 64, 4, simplify=False), "plain build again")
        rt.build_dense(as_source(big, "tensor"), 64, 4, simplify=True)  # and the same grid simplified
        G.assert_same_image(rt.download(), host_image(("seq4", 64, 4), big, 64, 4), "simplified after plain")
    finally:
        rt.close()
