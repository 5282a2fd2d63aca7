"""vhx_list_voxels on the GPU: the occupied voxels of a box of the device tree as a list. The device's lists are held to
the host twin on the downloaded image (vhx_flat_list_voxels, pinned by tests/test_list_voxels.py) and to the numpy model
(tests/_list_model.py) over the device's own read_dense(data=True). Every comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from tests import _dense_data_grids as DG
from tests import _dense_grids as G
from tests._list_model import expected_box
from tests.test_list_voxels import SENTINEL, assert_lists, boxes, stretched_image, wide_image

pytestmark = pytest.mark.gpu


def to_host(t):
    return t.cpu().numpy().view(np.uint32)


def check_boxes(rt, size, bd, what, tensors=True):
    """Every box of the tree on `rt`: the device list against the host twin and the model; returns the planes."""
    vis, dat = rt.read_dense(data=True)
    image = rt.download()
    for name, origin, extents in boxes(size, bd, vis, dat):
        w = f"{what} {name}"
        want = expected_box(vis, dat, size, bd, origin, extents)
        assert_lists(image.list_voxels(origin, extents), want, w + " (host twin)")
        assert_lists(rt.list_voxels(origin, extents), want, w + " (host arrays)")
        assert rt.count_voxels(origin, extents) == len(want[0]), w
        if tensors:
            got = rt.list_voxels(origin, extents, device=True)
            assert all(t.is_cuda and str(t.dtype) == "torch.int32" for t in got), w
            assert_lists([to_host(t) for t in got], want, w + " (tensors)")
    return vis, dat


@pytest.mark.parametrize("kind", DG.KINDS)
@pytest.mark.parametrize("size,bd", DG.SIZES)
def test_lists_of_built_trees(gpu, kind, size, bd):
    g, d = DG.make_pair(kind, size)
    gpu.build_dense(g, size, bd, data=d)
    vis, dat = check_boxes(gpu, size, bd, f"{kind} {size}/{bd}")
    gpu.simplify()
    svis, sdat = check_boxes(gpu, size, bd, f"{kind} {size}/{bd} simplified")
    assert np.array_equal(svis, vis) and np.array_equal(sdat, dat)


@pytest.mark.parametrize("kind,size,bd", [("full", 64, 4), ("blocks4", 32, 2), ("blocks4", 64, 4), ("cut", 32, 8),
                                          ("brick_noise", 16, 1), ("brick_noise", 64, 4)])
def test_lists_of_solid_bricks_and_uniform_leaves(gpu, kind, size, bd):
    from tests import _simplify_grids as SG
    gpu.build_dense(SG.make_grid(kind, size, bd), size, bd, simplify=True)
    SG.assert_case(kind, size, bd, gpu.download())
    check_boxes(gpu, size, bd, f"{kind} {size}/{bd} simplified build")


def raw_list(rt, origin, extents, capacity, on_device, fields=(True, True, True), slack=8):
    """vhx_list_voxels through the C ABI into sentinel-filled arrays: (rc, count, positions, albedo, data) as numpy."""
    import torch
    n = ctypes.c_uint64(SENTINEL)
    room = capacity + slack
    arrays = [np.full((room, 3), SENTINEL, np.uint32), np.full(room, SENTINEL, np.uint32),
              np.full(room, SENTINEL, np.uint32)]
    if on_device:
        arrays = [torch.from_numpy(a.view(np.int32)).to(f"cuda:{rt.device}") for a in arrays]
        torch.cuda.synchronize()
        ptrs = [a.data_ptr() for a in arrays]
    else:
        ptrs = [a.ctypes.data for a in arrays]
    q = N.PointsOut(*origin, *extents, capacity, *(p if on else None for p, on in zip(ptrs, fields)), ctypes.pointer(n))
    rc = N.lib().vhx_list_voxels(rt._h, ctypes.byref(q), int(on_device))
    return (rc, n.value, *([to_host(a) for a in arrays] if on_device else arrays))


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("simplified", [False, True])
def test_capacity_and_null_fields(gpu, simplified, on_device):
    size, bd = 32, 2
    g, d = DG.make_pair("sparse", size)
    gpu.build_dense(g, size, bd, data=d)
    if simplified:
        gpu.simplify()
    vis, dat = gpu.read_dense(data=True)
    origin, extents = (3, 5, 1), (20, 11, 30)
    want = expected_box(vis, dat, size, bd, origin, extents)
    count = len(want[0])
    assert count > 8
    for capacity in (0, 1, count - 1, count, count + 5):
        rc, n, *arrays = raw_list(gpu, origin, extents, capacity, on_device)
        assert rc == N.VHX_OK and n == count, capacity
        k = min(count, capacity)
        for a, w in zip(arrays, want):
            assert np.array_equal(a[:k], w[:k]), capacity  # the prefix of the full list
            assert (a[k:] == SENTINEL).all(), capacity     # nothing past it is written
        got = gpu.list_voxels(origin, extents, capacity=capacity, device=on_device)
        assert got[3] == count and len(got[0]) == len(got[1]) == len(got[2]) == k
        assert np.array_equal(to_host(got[0]) if on_device else got[0], want[0][:k])
    for fields in ((True, False, False), (False, True, False), (False, False, True), (False, True, True),
                   (False, False, False)):
        rc, n, *arrays = raw_list(gpu, origin, extents, count, on_device, fields)
        assert rc == N.VHX_OK and n == count, fields
        for a, w, on in zip(arrays, want, fields):
            assert np.array_equal(a[:count], w) if on else (a == SENTINEL).all(), fields


def edit(rt, size, bd, seed):
    """A set_voxels / clear_voxels / write_dense sequence: new colours and data values, clears, a box cut out."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, size, (300, 3)).astype(np.uint32)
    alb = np.where(rng.random(300) < 0.7, G.rgba(1, 200, 200), 0).astype(np.uint32)
    dat = np.where(rng.random(300) < 0.4, 11, 0).astype(np.uint32)
    rt.set_voxels(pos, alb, dat)
    rt.clear_voxels(rng.integers(0, size, (200, 3)).astype(np.uint32))
    box = np.zeros((size // 2, 7, 9), np.uint32)
    box[::2, ::3] = G.rgba(5, 5, 5)
    rt.write_dense(box, (2, 3, size // 4))
    rt.set_voxels(rng.integers(0, size // 2, (50, 3)).astype(np.uint32), 0, 0x80000000, "insert")
    rt.fill_box((0, 0, 0), (4 * bd,) * 3, 0)  # a whole leaf emptied: its node and bricks are orphaned


@pytest.mark.parametrize("size,bd,simplified", [(64, 4, False), (32, 2, True)])
def test_lists_after_edits_and_rewrites(gpu, size, bd, simplified):
    g, d = DG.make_pair("sparse", size)
    gpu.build_dense(g, size, bd, data=d)
    if simplified:
        gpu.simplify()
    edit(gpu, size, bd, size + bd)
    assert gpu.orphans() != (0, 0)
    what = f"{size}/{bd} edited"
    vis, dat = check_boxes(gpu, size, bd, what, tensors=False)
    first = gpu.list_voxels()
    for name, rewrite in (("compact", gpu.compact), ("simplify", gpu.simplify), ("compact_palette", gpu.compact_palette)):
        rewrite()
        v, p = check_boxes(gpu, size, bd, f"{what} after {name}", tensors=False)
        assert np.array_equal(v, vis) and np.array_equal(p, dat), name
        assert_lists(gpu.list_voxels(), first, f"{what}: the whole list after {name}")


@pytest.mark.parametrize("size,bd", [(64, 4), (32, 8), (16, 1)])
def test_round_trip_through_set_voxels(gpu, size, bd):
    g, d = DG.make_pair("sparse", size)
    gpu.build_dense(g, size, bd, data=d)
    gpu.simplify()
    pos, alb, dat = gpu.list_voxels(device=True)
    second = vhx.Raytracer(0)
    try:
        second.build_dense(np.zeros_like(g), size, bd)
        assert second.count_voxels() == 0
        second.set_voxels(pos, alb, dat)
        a, b = gpu.read_dense(data=True), second.read_dense(data=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert second.count_voxels() == gpu.count_voxels() == len(pos) > 0
        assert_lists(second.list_voxels(), [to_host(t) for t in (pos, alb, dat)], f"{size}/{bd} round trip")
    finally:
        second.close()


def test_shared_contexts_see_the_owners_writes_and_write_nothing():
    size, bd = 64, 4
    g, d = DG.make_pair("sparse", size)
    owner = vhx.Raytracer(0)
    try:
        owner.build_dense(g, size, bd, data=d)
        sh = owner.shared()
        try:
            before = sh.list_voxels()
            assert_lists(before, owner.list_voxels(), "shared context")
            pos = np.array([[63, 63, 63], [0, 1, 2]], np.uint32)
            owner.set_voxels(pos, G.rgba(7, 7, 7), 5)
            image = owner.download()
            after = sh.list_voxels()  # submitted after the owner's write: it sees it
            vis, dat = owner.read_dense(data=True)
            assert_lists(after, expected_box(vis, dat, size, bd, (0, 0, 0), (size,) * 3), "shared context after a write")
            assert (after[0] == pos[0]).all(1).any() and (after[0] == pos[1]).all(1).any()
            for _ in range(3):
                sh.list_voxels((3, 5, 1), (40, 33, 60), device=True)
                owner.count_voxels()
            G.assert_same_image(owner.download(), image, "the tree after list calls")
        finally:
            sh.close()
    finally:
        owner.close()


def test_lists_and_writes_from_two_threads():
    """Contexts of one tree driven from two host threads, as tests/test_gpu_ordering.py drives traces: the owner writes
    points with a new data value each time (the data palette grows, so its buffer is replaced) and clears them again
    while a shared context lists the cube. Every list must be that of one whole tree version, never a mix."""
    import threading
    size, bd, rounds = 64, 4, 12
    g, d = DG.make_pair("sparse", size)
    rng = np.random.default_rng(99)
    pos = np.unique(rng.integers(0, size, (400, 3)).astype(np.uint32), axis=0)
    colour = G.rgba(7, 7, 7)
    owner = vhx.Raytracer(0)
    try:
        owner.build_dense(g, size, bd, data=d)
        vis, dat = owner.read_dense(data=True)
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]

        def version(albedo, data):
            v, p = vis.copy(), dat.copy()
            v[z, y, x], p[z, y, x] = albedo, data
            return b"".join(a.tobytes() for a in expected_box(v, p, size, bd, (0, 0, 0), (size,) * 3))

        versions = {version(vis[z, y, x], dat[z, y, x]), version(0, 0)}  # as built; with the points cleared
        versions |= {version(colour, 100 + k) for k in range(rounds)}
        sh = owner.shared()
        errors, lists = [], []

        def writer():
            try:
                for k in range(rounds):
                    owner.set_voxels(pos, colour, 100 + k)
                    owner.clear_voxels(pos)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        try:
            th = threading.Thread(target=writer)
            th.start()
            for _ in range(2 * rounds):
                lists.append(sh.list_voxels(capacity=size ** 3)[:3])  # one call: no count ahead of it
            th.join()
            assert not errors, errors
            for k, got in enumerate(lists):
                assert b"".join(a.tobytes() for a in got) in versions, f"list {k} is of no tree version (a torn read)"
            assert b"".join(a.tobytes() for a in sh.list_voxels()) == version(0, 0)
        finally:
            sh.close()
    finally:
        owner.close()


def test_refusals_write_nothing():
    import torch
    assert ctypes.sizeof(N.PointsOut) == 64  # vhx_points_out: six u32, a u64 and four pointers
    rt = vhx.Raytracer(0)

    def refused(origin, extents, code, what, on_device=False):
        rc, n, *arrays = raw_list(rt, origin, extents, 16, on_device)
        assert rc == code, what
        assert n == SENTINEL and all((a == SENTINEL).all() for a in arrays), what

    try:
        refused((0, 0, 0), (1, 1, 1), N.VHX_E_STATE, "before any upload")
        g, d = DG.make_pair("sparse", 16)
        rt.build_dense(g, 16, 4, data=d)
        for on_device in (False, True):
            refused((0, 0, 0), (0, 4, 4), N.VHX_E_INVALID_ARG, "an empty box", on_device)
            refused((13, 0, 0), (4, 4, 4), N.VHX_E_INVALID_ARG, "a box outside the cube", on_device)
            refused((0, 0xFFFFFFFF, 0), (1, 2, 1), N.VHX_E_INVALID_ARG, "a box that wraps", on_device)
        q = N.PointsOut(0, 0, 0, 1, 1, 1, 0, None, None, None, None)
        assert N.lib().vhx_list_voxels(rt._h, ctypes.byref(q), 0) == N.VHX_E_INVALID_ARG  # null count
        assert N.lib().vhx_list_voxels(rt._h, None, 0) == N.VHX_E_INVALID_ARG
        # overlapping device arrays: the data words inside the positions
        n = ctypes.c_uint64(SENTINEL)
        buf = torch.full((16 * 4,), -1, dtype=torch.int32, device="cuda:0")
        other = torch.full((16,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        q = N.PointsOut(0, 0, 0, 16, 16, 16, 16, buf.data_ptr(), other.data_ptr(), buf.data_ptr() + 16 * 4,
                        ctypes.pointer(n))
        assert N.lib().vhx_list_voxels(rt._h, ctypes.byref(q), 1) == N.VHX_E_INVALID_ARG
        assert n.value == SENTINEL and bool((buf == -1).all()) and bool((other == -1).all())
        q.data = None  # the same call without the overlap is accepted
        assert N.lib().vhx_list_voxels(rt._h, ctypes.byref(q), 1) == N.VHX_OK and n.value == rt.count_voxels()
        rt.upload(stretched_image())
        refused((0, 0, 0), (64, 64, 64), N.VHX_E_STATE, "a stretched brick")
        refused((5, 5, 5), (1, 1, 1), N.VHX_E_STATE, "a stretched brick under one voxel", True)
        rt.upload(wide_image())
        refused((0, 0, 0), (1 << 24,) * 3, N.VHX_E_CAPACITY, "2^72 voxels")
        assert rt.count_voxels((0, 0, 0), (1 << 24, (1 << 24) - 1, 1)) == 0  # 2^48 - 2^24 voxels of nothing
    finally:
        rt.close()


def test_a_lod_cut_view_is_listed_as_it_reads(gpu):
    from tests.test_gpu_dense_write import lod_tree
    size = 64
    gpu.upload(lod_tree(size).flatten_lod(0))
    check_boxes(gpu, size, 4, "flatten_lod(0)", tensors=False)
