"""User data through the dense paths on the GPU: vhx_build_tree_dense_data against the host builder's image
(FlatTree.from_dense(data=), itself pinned to the insert loop by tests/test_dense_data.py), the derived state and a frame
of such a tree, and vhx_read_dense_data against BoxTree::get restated over the image (tests/_flatget.py). Every
comparison is bit for bit."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree
from voxelhex_amd import _native as N
from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests import _flatget as F

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
W = 64
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def pair(kind, size, seed=0):
    return cached(("pair", kind, size, seed), lambda: DG.make_pair(kind, size, seed))


def host_image(kind, size, bd, simplify=False, seed=0):
    g, d = pair(kind, size, seed)
    return cached(("host", kind, size, bd, simplify, seed), lambda: FlatTree.from_dense(g, size, bd, simplify=simplify, data=d))


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def odd_box(size):
    origin = (size * 13 // 64, size * 15 // 64, size * 3 // 64)
    extents = (max(1, size * 22 // 64), max(1, size * 18 // 64), max(1, size * 35 // 64))
    return origin, extents


@pytest.fixture(scope="module")
def second():
    rt = vhx.Raytracer(0)
    yield rt
    rt.close()


# ---------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("source", ["host", "tensor"])
@pytest.mark.parametrize("size,bd", DG.SIZES)
@pytest.mark.parametrize("kind", DG.KINDS)
def test_build_equals_the_host_builder(gpu, kind, size, bd, source):
    g, d = pair(kind, size)
    if source == "tensor":
        gpu.build_dense(to_device(g), size, bd, data=to_device(d))
    else:
        gpu.build_dense(g, size, bd, data=d)
    G.assert_same_image(gpu.download(), host_image(kind, size, bd), f"{kind} {size}/{bd} {source}")


@pytest.mark.parametrize("size,bd", [(16, 4), (32, 2), (64, 4), (16, 1), (32, 8)])
@pytest.mark.parametrize("kind", ["sparse", "full"])
def test_simplified_build_equals_the_host_builder(gpu, kind, size, bd):
    g, d = pair(kind, size, 1)
    if kind == "full":
        d = np.full_like(d, 7)
        d[: size // 2, : size // 4] = 9
    want = FlatTree.from_dense(g, size, bd, simplify=True, data=d)
    gpu.build_dense(to_device(g), size, bd, simplify=True, data=to_device(d))
    G.assert_same_image(gpu.download(), want, f"{kind} {size}/{bd}")
    if kind == "full":
        assert (want.node_type == N.VHX_NODE_UNIFORM_LEAF).any()


def test_no_data_is_the_colour_only_build(gpu):
    g = G.make_grid("sparse", 32)
    want = FlatTree.from_dense(g, 32, 2)
    gpu.build_dense(g, 32, 2, data=np.zeros_like(g))
    G.assert_same_image(gpu.download(), want, "a data plane of zeros")
    gpu.build_dense(to_device(g), 32, 2, data=None)
    G.assert_same_image(gpu.download(), want, "data=None")


def test_vector_and_scalar_paths_give_the_same_image(gpu):
    import torch
    size, bd = 64, 4
    g = np.zeros((size,) * 3, np.uint32)
    gs, _ = pair("sparse", size, 3)
    g[: gs.shape[0], : gs.shape[1], : gs.shape[2]] = gs
    d = DG.make_data(g.shape, 3)
    want = FlatTree.from_dense(g, size, bd, data=d)
    tg, td = to_device(g), to_device(d)
    assert tg.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
    gpu.build_dense(tg, size, bd, data=td)  # both planes aligned, gx a multiple of 4: 16-byte loads
    G.assert_same_image(gpu.download(), want, "vector path")
    buf = torch.empty(size ** 3 + 1, dtype=torch.int32, device="cuda:0")
    off = buf[1:].view(size, size, size)
    off.copy_(td)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    gpu.build_dense(tg, size, bd, data=off)  # the data plane is not 16-byte aligned: scalar loads
    G.assert_same_image(gpu.download(), want, "scalar path")


def test_many_data_values(gpu):
    g, d = DG.many_data_grid()
    want = FlatTree.from_dense(g, 64, 4, data=d)
    assert want.desc.data_count == 5000
    first = None
    for k in range(3):  # the image does not depend on scheduling
        gpu.build_dense(to_device(g), 64, 4, data=to_device(d))
        img = gpu.download()
        G.assert_same_image(img, want, f"run {k}")
        first = img if first is None else first
        G.assert_same_image(img, first, f"run {k} against run 0")


def test_data_capacity_and_a_refused_build_keeps_the_tree(gpu):
    g, d = DG.distinct_data_grid(65535)
    gpu.build_dense(g, 64, 4, data=d)
    before = gpu.download()
    assert before.desc.data_count == 65535
    G.assert_same_image(before, FlatTree.from_dense(g, 64, 4, data=d), "65535 data values")
    g, d = DG.distinct_data_grid(65536)
    for src in (lambda a: a, to_device):
        with pytest.raises(N.VhxError) as e:
            gpu.build_dense(src(g), 64, 4, data=src(d))
        assert e.value.code == N.VHX_E_CAPACITY
        G.assert_same_image(gpu.download(), before, "after the refused build")


def test_a_wrong_data_plane_is_refused(gpu):
    g, d = pair("sparse", 16)
    with pytest.raises(TypeError):
        gpu.build_dense(to_device(g), 16, 4, data=d)  # a tensor grid with a host plane
    with pytest.raises(TypeError):
        gpu.build_dense(g, 16, 4, data=to_device(d))
    with pytest.raises(TypeError):
        gpu.build_dense(to_device(g), 16, 4, data=to_device(d[:-1]))


# ----------------------------------------------------------------------------------------- derived state and trace
@pytest.mark.parametrize("size,bd", [(32, 2), (64, 4), (32, 8), (16, 1)])
def test_derived_state_and_frame(gpu, oracle, second, size, bd):
    g, d = pair("sparse", size)
    gpu.build_dense(g, size, bd, data=d)
    img = gpu.download()
    second.upload(img)
    n = img.desc
    words = max(1, bd ** 3 // 64)
    assert np.array_equal(gpu.read_derived(N.VHX_DERIVED_NODE_HDR, 0, n.node_count),
                          second.read_derived(N.VHX_DERIVED_NODE_HDR, 0, n.node_count))
    assert np.array_equal(gpu.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, n.brick_count * words),
                          second.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, n.brick_count * words))
    cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
    want = oracle.trace_primary(host_image("sparse", size, bd), cam, 0, 0, W, W)
    got = gpu.trace_primary(cam)
    for k in want:
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), k
    v = want["value"]
    data_only = (v != EMPTY) & ((v & 0xFFFF) == 0xFFFF)
    assert data_only.any(), "no pixel hits a data-only voxel"
    assert ((v != EMPTY) & ((v & 0xFFFF) != 0xFFFF) & ((v >> 16) != 0xFFFF)).any(), "no pixel hits a Complex voxel"


# ----------------------------------------------------------------------------------------------------------- read
def expected_planes(img, origin, extents):
    v = F.flat_get(img, F.lattice(origin, extents))
    shape = extents[::-1]
    return F.flat_albedo(img, v).reshape(shape), DG.flat_data(img, v).reshape(shape)


@pytest.mark.parametrize("size,bd", DG.SIZES)
@pytest.mark.parametrize("image", ["plain", "simplified", "uploaded"])
def test_read_returns_both_planes(gpu, image, size, bd):
    import torch
    g, d = pair("sparse", size)
    if image == "uploaded":
        gpu.upload(host_image("sparse", size, bd))
    else:
        gpu.build_dense(g, size, bd, simplify=image == "simplified", data=d)
    img = gpu.download()
    if image == "simplified":
        G.assert_same_image(img, host_image("sparse", size, bd, True), "simplified")
    whole = ((0, 0, 0), (size,) * 3)
    a, p = gpu.read_dense(data=True)
    assert np.array_equal(a, DG.extend(DG.visible(g), size)) and np.array_equal(p, DG.extend(d, size)), "the grid back"
    assert np.array_equal(a, gpu.read_dense()), "the albedo plane is read_dense's"
    for origin, extents in (whole, odd_box(size)):
        wa, wp = expected_planes(img, origin, extents)
        a, p = gpu.read_dense(origin, extents, data=True)
        assert np.array_equal(a, wa) and np.array_equal(p, wp), f"{origin} + {extents}: host arrays"
        ta = torch.full(extents[::-1], 5, dtype=torch.int32, device="cuda:0")
        tp = torch.full(extents[::-1], 6, dtype=torch.int32, device="cuda:0")
        ra, rp = gpu.read_dense(origin, extents, out=ta, data=tp)
        assert ra is ta and rp is tp
        assert np.array_equal(to_host(ta), wa) and np.array_equal(to_host(tp), wp), f"{origin} + {extents}: tensors"
        out = np.full(extents[::-1], 9, np.uint32)
        ra, rp = gpu.read_dense(origin, extents, data=out)  # an array passed as data receives the plane
        assert rp is out and np.array_equal(out, wp) and np.array_equal(ra, wa)


def test_data_only_read_and_refusals(gpu):
    import ctypes
    import torch
    size, bd = 32, 2
    g, d = pair("sparse", size)
    gpu.build_dense(g, size, bd, data=d)
    n = size ** 3
    out = np.full((size,) * 3, 3, np.uint32)
    box = N.DenseOut(0, 0, 0, size, size, size, None)  # no albedo plane: data only
    assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(box), out.ctypes.data, 0) == N.VHX_OK
    assert np.array_equal(out, DG.extend(d, size))
    t = torch.full((size,) * 3, 3, dtype=torch.int32, device="cuda:0")
    buf = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()  # the fills run on torch's stream, the raw calls below on the context's
    assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(box), t.data_ptr(), 1) == N.VHX_OK
    gpu.sync()
    assert np.array_equal(to_host(t), DG.extend(d, size))
    # overlapping device planes: refused, both untouched
    for k in (0, 1, n // 2, n - 1):
        box.albedo = buf.data_ptr()
        assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(box), buf.data_ptr() + 4 * k, 1) == N.VHX_E_INVALID_ARG
        box.albedo = buf.data_ptr() + 4 * k
        assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(box), buf.data_ptr(), 1) == N.VHX_E_INVALID_ARG
    gpu.sync()
    assert bool((buf == 7).all())
    box.albedo = buf.data_ptr()
    assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(box), buf.data_ptr() + 4 * n, 1) == N.VHX_OK  # adjacent
    gpu.sync()
    assert np.array_equal(to_host(buf[n:]).reshape((size,) * 3), DG.extend(d, size))
    # a null data plane, a box outside the root cube
    assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(box), None, 0) == N.VHX_E_INVALID_ARG
    bad = N.DenseOut(1, 0, 0, size, size, size, None)
    assert N.lib().vhx_read_dense_data(gpu._h, ctypes.byref(bad), out.ctypes.data, 0) == N.VHX_E_INVALID_ARG
    assert np.array_equal(out, DG.extend(d, size)), "a refused call leaves the plane untouched"
