"""vhx_build_lod (Raytracer.build_lod): the LOD image of a device tree with node MIPs, built on the GPU. The device
result is compared bit for bit with vhx_flat_lod (FlatTree.lod / TreeImage.lod) of the source's download, which
tests/test_lod_model.py pins to the host BoxTree route. The frames here are compared between two GPU contexts, the
built one and one that uploaded the host image with its descriptors: both run the same MIP kernels, so these frames pin
the image and the descriptors, not the kernels. The oracle's trace of the downloaded image against the device's is in
tests/test_gpu_mip_parity.py (test_device_built_lod_vs_oracle)."""
import ctypes

import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import BoxTree
from tests import _dense_grids as G
from tests import _lod_grids as L
from tests._mip_cases import build_lod_source
from tests._skycams import aimed_camera

pytestmark = pytest.mark.gpu

FIELDS = ("value", "cell", "voxel", "impact", "normal", "depth", "rgba")
W, H = 96, 64


@pytest.fixture(scope="module")
def ctxs():
    """(src, lod, ref): the source, the destination, and a context for host images."""
    rts = [vhx.Raytracer(0) for _ in range(3)]
    yield rts
    for r in rts:
        r.close()


def _cams(size):
    c = size / 2
    return [aimed_camera(W, H, (-0.8 * size, 1.3 * size, -1.1 * size), (c, c * 0.4, c)),
            aimed_camera(W, H, (0.2 * size, 0.3 * size, -0.6 * size), (0.1 * size, 0.1 * size, 0.2 * size), fov=2.0)]


@pytest.mark.parametrize("method", L.METHODS)
@pytest.mark.parametrize("kind", ["plain", "simplified", "edited"])
@pytest.mark.parametrize("name", list(L.SHAPES))
def test_build_lod_is_the_host_image(ctxs, name, kind, method):
    src, lod, _ = ctxs
    depth = L.SHAPES[name][2]
    build_lod_source(src, name, kind)
    before = src.download()
    if kind == "edited" and name != "4/1":  # edit order: not the numbering a compaction gives
        assert not np.array_equal(before.node_children, before.compacted().node_children), "the edits renumbered nothing"
    for d in range(0, depth + 2):
        want = before.lod(d, method)
        nodes, bricks, added = lod.build_lod(src, d, method)
        got = lod.download()
        what = f"{name} {kind} {method} depth {d}"
        G.assert_same_image(got, want, what)
        mips = lod.node_mips()
        assert np.array_equal(mips, np.asarray(want.node_mips)), f"{what}: node_mips"
        assert (nodes, bricks) == (want.node_type.size, want.desc.brick_count), what
        assert added == want.color_palette.size - before.color_palette.size, what
        if method == "point":
            assert added == 0, what
    G.assert_same_image(src.download(), before, "the source after build_lod")
    with pytest.raises(N.VhxError) as e:  # and it has no MIPs
        src.node_mips()
    assert e.value.code == N.VHX_E_STATE


@pytest.mark.parametrize("name,method", [("64/4", "box"), ("128/2", "point"), ("256/4", "box")])
def test_lod_frames_equal_an_uploaded_host_lod(ctxs, name, method):
    src, lod, ref = ctxs
    size, bd, depth = L.SHAPES[name]
    build_lod_source(src, name, "plain")
    host = src.download()
    cams = _cams(size)
    exact = [src.trace_primary(c, fields=FIELDS) for c in cams]
    assert any((f["value"] != N.VHX_EMPTY).any() for f in exact), "the cameras see nothing"
    differs = False
    for d in range(0, depth + 2):
        lod.build_lod(src, d, method)
        image = host.lod(d, method)
        ref.upload(image)
        ref.set_node_mips(image.node_mips)
        for k, cam in enumerate(cams):
            got, want = lod.trace_primary(cam, fields=FIELDS), ref.trace_primary(cam, fields=FIELDS)
            for f in FIELDS:
                assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f"{name} depth {d} cam {k}: {f}"
                if d >= depth:  # every node is resident: the MIPs are never probed
                    assert np.array_equal(got[f].view(np.uint32), exact[k][f].view(np.uint32)), \
                        f"{name} depth {d} cam {k}: {f} against the exact frame"
            if d < depth:
                differs |= not np.array_equal(got["value"], exact[k]["value"])
        ref.set_node_mips(None)
    assert differs, "no cut frame showed a MIP"


def test_build_lod_again_after_an_edit_is_ordered_like_an_upload(ctxs):
    """Frames submitted before the second build_lod show the first image, frames after it the second, on the owner and
    on shared contexts with frames in flight (as tests/test_gpu_ordering.py does around a ranged write)."""
    import torch
    src, _, ref = ctxs
    name, d, method, F = "64/4", 0, "box", 4
    size = L.SHAPES[name][0]
    build_lod_source(src, name, "plain")
    cams = [aimed_camera(W, H, (-0.8 * size, (1.0 + 0.1 * i) * size, -1.1 * size), (size / 2, size / 4, size / 2))
            for i in range(F)]
    owner = vhx.Raytracer(0)
    try:
        owner.build_lod(src, d, method)
        versions = [src.download().lod(d, method)]
        ctxs_f = [owner] + [owner.shared() for _ in range(F - 1)]
        dev = torch.device("cuda", 0)

        def outs():
            return [{"value": torch.zeros(W * H, dtype=torch.int32, device=dev),
                     "rgba": torch.zeros(W * H, dtype=torch.int32, device=dev),
                     "depth": torch.zeros(W * H, dtype=torch.float32, device=dev)} for _ in range(F)]
        before, after = outs(), outs()
        torch.cuda.synchronize()  # the zero fills (torch's stream) complete before the context streams write
        for r, c, o in zip(ctxs_f, cams, before):
            r.trace_primary(c, out=o)
        src.fill_box((0, 0, 0), (size, size // 4, size // 2), int(G.rgba(255, 255, 255)))  # the edit of the source
        owner.build_lod(src, d, method)  # ordered after the frames above, before the frames below
        for r, c, o in zip(ctxs_f, cams, after):
            r.trace_primary(c, out=o)
        torch.cuda.synchronize()
        versions.append(src.download().lod(d, method))
        G.assert_same_image(owner.download(), versions[1], "the second image")
        assert np.array_equal(owner.node_mips(), np.asarray(versions[1].node_mips))
        for v, frames in enumerate((before, after)):
            ref.upload(versions[v])
            ref.set_node_mips(versions[v].node_mips)
            wants = [ref.trace_primary(c, fields=("value", "rgba", "depth")) for c in cams]
            ref.set_node_mips(None)
            for i, (o, want) in enumerate(zip(frames, wants)):
                for f in ("value", "rgba", "depth"):
                    got = o[f].cpu().numpy().view(np.uint32)
                    assert np.array_equal(got, want[f].view(np.uint32).reshape(-1)), f"version {v} context {i}: {f}"
            if v == 0:
                first = wants
        assert any(not np.array_equal(a["rgba"], b["rgba"]) for a, b in zip(first, wants)), "the edit is not visible"
        for r in ctxs_f[1:]:
            r.close()
    finally:
        owner.close()


def _refused(dst, src_h, code, d=1, method=N.VHX_MIP_BOX_FILTER, dst_h=None, outs=3):
    """The call returns `code` and leaves dst's image and node MIPs as they were."""
    image, mips = dst.download(), dst.node_mips()
    n = [ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()]
    args = [ctypes.byref(v) if k < outs else None for k, v in enumerate(n)]
    rc = N.lib().vhx_build_lod(dst._h if dst_h is None else dst_h, src_h, d, method, *args)
    assert rc == code, (rc, code)
    G.assert_same_image(dst.download(), image, "the destination after a refused call")
    assert np.array_equal(dst.node_mips(), mips)


def test_build_lod_refusals(ctxs):
    src, lod, other = ctxs
    size, bd, depth = L.SHAPES["64/4"]
    build_lod_source(src, "64/4", "plain")
    before = src.download()
    lod.build_lod(src, 1, "box")
    # arguments
    _refused(lod, None, N.VHX_E_INVALID_ARG)
    _refused(lod, src._h, N.VHX_E_INVALID_ARG, outs=2)
    _refused(lod, src._h, N.VHX_E_INVALID_ARG, outs=0)
    for method in (2, 3, 4, 77):
        _refused(lod, src._h, N.VHX_E_INVALID_ARG, method=method)
    _refused(lod, lod._h, N.VHX_E_INVALID_ARG)  # the same tree ...
    sh = lod.shared()
    _refused(lod, sh._h, N.VHX_E_INVALID_ARG)  # ... through another of its contexts
    _refused(lod, src._h, N.VHX_E_STATE, dst_h=sh._h)  # a shared context is no destination
    sh.close()
    assert N.lib().vhx_build_lod(None, src._h, 0, 0, None, None, None) == N.VHX_E_INVALID_ARG
    # the destination's state
    lod.set_shadow_light((1.0, 2.0, 3.0))
    _refused(lod, src._h, N.VHX_E_STATE)
    lod.set_shadow_light(None)
    # the source's state
    fresh = vhx.Raytracer(0)
    try:
        _refused(lod, fresh._h, N.VHX_E_STATE)  # no tree
    finally:
        fresh.close()
    cut = before.lod(0, "box")
    other.upload(cut)
    _refused(lod, other._h, N.VHX_E_STATE)  # a LOD-cut view: occupied sectants without children
    full = before.lod(depth, "box")
    other.upload(full)
    other.set_node_mips(full.node_mips)
    _refused(lod, other._h, N.VHX_E_STATE)  # node MIPs set
    other.set_node_mips(None)
    t = BoxTree(256, 4)  # leaves sit at depth 2 ...
    t.insert_at_lod((0, 0, 0), 64, vhx.Albedo(9, 8, 7, 255))
    shallow = t.flatten()
    assert shallow.node_type.tolist() == [N.VHX_NODE_INTERNAL, N.VHX_NODE_UNIFORM_LEAF]  # ... and this one at depth 1
    other.upload(shallow)
    _refused(lod, other._h, N.VHX_E_STATE)  # a leaf whose edge is not 4 * brick_dim
    # after all of that the pair still works
    G.assert_same_image(src.download(), before, "the source after refused calls")
    lod.build_lod(src, 0, "point")
    G.assert_same_image(lod.download(), before.lod(0, "point"), "after the refusals")


def test_build_lod_capacity(ctxs):
    src, lod, _ = ctxs
    src.build_dense(L.capacity_grid(), 64, 4)
    before = src.download()
    assert before.color_palette.size == 64000
    lod.build_lod(src, 1, "point")
    _refused(lod, src._h, N.VHX_E_CAPACITY, method=N.VHX_MIP_BOX_FILTER)
    nodes, bricks, added = lod.build_lod(src, 1, "point")
    assert added == 0 and nodes == before.node_type.size
    want = before.lod(1, "point")
    G.assert_same_image(lod.download(), want, "PointFilter on 64,000 colours")
    assert np.array_equal(lod.node_mips(), np.asarray(want.node_mips))
    G.assert_same_image(src.download(), before, "the source")
