"""Voxel removal on the device: clears of the host tree reach the device view through the stream's ranged writes
(vhx_stream_upload -> vhx_update_ranges) or through a fresh vhx_upload_tree, and the GPU traces the result exactly like
the oracle. Removal is the direction in which derived device state shrinks: brick bitmaps lose bits, child records
lose their brick, node headers lose occupancy, and slots are rewritten for other owners."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from tests.test_gpu_parity import assert_same
from tests.test_streaming import FIELDS, _rays_in_box, _tree
from tests.test_streaming_clear import clearing_edit

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size,bd", [(32, 2), (64, 4), (128, 8)])
def test_clears_mid_stream_on_device(oracle, size, bd):
    t = _tree(size, bd)
    rt = vhx.Raytracer(0)
    try:
        S = float(size)
        s = vhx.StreamingView(t, rt, (S / 2, S / 2, S / 2), S)
        s.set_rates(8, 32, 10)
        for _ in range(3):  # a few frames into the stream, then the first edits
            s.upload()
        rng = np.random.default_rng(bd)
        lo, hi = np.full(3, 1.0), np.full(3, S - 1)
        for rnd in range(3):
            clearing_edit(t, rng, size, bd)
            stats, frames, _ = s.upload_all()
            assert stats["pending"] == 0
            o, d = _rays_in_box(rng, lo, hi, 12000)
            got = rt.trace_rays(o, d, fields=FIELDS, count_bytes=True)
            assert_same(got, oracle.trace_rays(s.view(), o, d, fields=FIELDS, count_bytes=True),
                        f"device view vs host mirror, round {rnd}")
            full = oracle.trace_rays(t.flatten(), o, d, fields=FIELDS)
            assert_same({k: got[k] for k in FIELDS}, full, f"device view vs cleared tree, round {rnd}")
            assert (full["value"] != N.VHX_EMPTY).sum() > 500
        s.close()
    finally:
        rt.close()


def _derived(rt, desc):
    words = max(1, desc.brick_dim ** 3 // 64)
    return (rt.read_derived(N.VHX_DERIVED_NODE_HDR, 0, desc.node_count),
            rt.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, desc.brick_count * words))


@pytest.mark.parametrize("size,bd", [(32, 2), (64, 4), (128, 8)])
def test_derived_state_after_clears_equals_a_fresh_upload(size, bd):
    """Node headers and brick bitmaps refreshed by the ranged writes of a round of clears equal those a second
    context computes from a fresh vhx_upload_tree of the same view."""
    t = _tree(size, bd)
    rt, fresh = vhx.Raytracer(0), vhx.Raytracer(0)
    try:
        S = float(size)
        s = vhx.StreamingView(t, rt, (S / 2, S / 2, S / 2), S)
        assert s.upload_all()[0]["pending"] == 0
        hdr0, occ0 = _derived(rt, s.view().desc)
        rng = np.random.default_rng(size)
        clearing_edit(t, rng, size, bd)
        assert s.upload_all()[0]["pending"] == 0
        view = s.view()
        hdr, occ = _derived(rt, view.desc)
        fresh.upload(view)
        fhdr, focc = _derived(fresh, view.desc)
        assert np.array_equal(hdr, fhdr), f"{(hdr != fhdr).any(axis=1).sum()} node headers differ"
        assert np.array_equal(occ, focc), f"{(occ != focc).sum()} bitmap words differ"
        # the clears did take state away: bitmap bits went 1 -> 0 and node headers changed
        assert (occ0[:len(occ)] & ~occ[:len(occ0)]).any() and not np.array_equal(hdr0, hdr[:len(hdr0)])
        s.close()
    finally:
        rt.close()
        fresh.close()


def test_full_residency_reupload_after_clears(oracle):
    size, bd, W = 64, 4, 128
    t = _tree(size, bd)
    cam = vhx.glass_camera(size, W, W, target=(size / 2,) * 3)
    rt = vhx.Raytracer(0)
    try:
        rt.upload(t.flatten())
        first = rt.trace_primary(cam, count_bytes=True)
        assert_same(first, oracle.trace_primary(t.flatten(), cam, 0, 0, W, W, count_bytes=True), "before the clears")
        clearing_edit(t, np.random.default_rng(2), size, bd)
        t.clear_at_lod((32, 32, 32), 16)  # the cube's corner node facing the camera side
        t.clear_at_lod((0, 0, 0), 16)
        flat = t.flatten()
        rt.upload(flat)
        second = rt.trace_primary(cam, count_bytes=True)
        assert_same(second, oracle.trace_primary(flat, cam, 0, 0, W, W, count_bytes=True), "after the clears")
        assert not np.array_equal(first["value"], second["value"])
    finally:
        rt.close()


def test_digging_along_the_centre_ray(oracle):
    """The ray through the centre pixel of a 128x128 glass camera aimed at the solid cube is traced with trace_rays;
    the brick-aligned block around the hit voxel is cleared and the stream settled, six times (into the cube).
    Each step's hit is the oracle's on the edited tree, and the ray reaches deeper as the blocks go."""
    size, bd, W = 64, 4, 128
    t = _tree(size, bd)
    S = float(size)
    rt = vhx.Raytracer(0)
    try:
        s = vhx.StreamingView(t, rt, (S / 2, S / 2, S / 2), 2 * S)
        assert s.upload_all()[0]["pending"] == 0
        # the centre pixel's ray: from the camera's origin through the point that pixel hits in the primary frame
        cam = vhx.glass_camera(size, W, W, target=(0.75 * S,) * 3)  # aimed at the solid cube's centre
        frame = rt.trace_primary(cam, fields=("value", "impact"))
        centre = (W // 2) * W + W // 2
        assert frame["value"].reshape(-1)[centre] != N.VHX_EMPTY
        o = np.array([list(cam.origin)], np.float32)
        d = frame["impact"].reshape(-1, 3)[centre:centre + 1] - o
        d = (d / np.sqrt((d * d).sum())).astype(np.float32)
        depths = []
        for step in range(6):
            got = rt.trace_rays(o, d, fields=FIELDS)
            ref = oracle.trace_rays(t.flatten(), o, d, fields=FIELDS)
            assert_same(got, ref, f"dig step {step}")
            assert ref["value"][0] != N.VHX_EMPTY, f"dig step {step}: nothing left to dig into"
            depths.append(float(ref["depth"][0]))
            inside = ref["impact"][0] - np.float32(1e-2) * ref["normal"][0]  # a point in the hit voxel
            voxel = tuple(int(v) for v in np.clip(np.floor(inside), 0, size - 1))
            assert t.get(voxel).kind != "Empty", (step, voxel)
            t.clear_at_lod(tuple(v // bd * bd for v in voxel), bd)
            assert t.get(voxel).kind == "Empty"
            assert s.upload_all()[0]["pending"] == 0
        assert all(b >= a for a, b in zip(depths, depths[1:])), depths
        assert any(b > a for a, b in zip(depths, depths[1:])), depths
        s.close()
    finally:
        rt.close()


def test_clear_between_frames_in_flight(oracle):
    """The ordering contract of vhx_create_shared under a clear: frame A is submitted on one shared context, a stream
    upload carrying a clear goes through the owner, frame B is submitted on another shared context, with no host
    synchronisation in between. A shows the mirror as it was before the clear, B the mirror after it."""
    import torch
    from tests.test_gpu_ordering import _Snapshot, _frame_out, _host, _same
    size, bd, W, H = 64, 4, 192, 128
    t = _tree(size, bd)
    S = float(size)
    owner = vhx.Raytracer(0)
    try:
        s = vhx.StreamingView(t, owner, (S / 2, S / 2, S / 2), 2 * S)
        assert s.upload_all()[0]["pending"] == 0
        a, b = owner.shared(), owner.shared()
        dev = torch.device("cuda", 0)
        cam = vhx.glass_camera(size, W, H, target=(S / 2,) * 3)
        out_a, out_b = _frame_out(W * H, dev), _frame_out(W * H, dev)
        torch.cuda.synchronize()  # the zero fills (torch's stream) complete before the context streams write
        t.clear_at_lod((32, 32, 32), 16)  # a corner node of the cube, towards the camera
        t.clear_at_lod((0, 16, 16), 16)
        for c in [(48, 0, 0), (0, 0, 0), (0, 0, 48), (0, 48, 0)]:  # lattice nodes this camera looks at
            t.clear_at_lod(c, 16)
        for p in [(40, 50, 33), (50, 40, 35), (36, 36, 50)]:
            t.clear(p)
        snap_a = _Snapshot(s.view())
        a.trace_primary(cam, out=out_a)
        pending, frames = 1, 0
        while pending and frames < 64:  # the queued clears, frame by frame, no host wait
            stats, grow = s.upload()
            assert not grow
            pending, frames = stats["pending"], frames + 1
        assert pending == 0
        snap_b = _Snapshot(s.view())
        b.trace_primary(cam, out=out_b)
        torch.cuda.synchronize()
        ref_a = oracle.trace_primary(snap_a, cam, 0, 0, W, H, fields=("value", "rgba", "depth"))
        ref_b = oracle.trace_primary(snap_b, cam, 0, 0, W, H, fields=("value", "rgba", "depth"))
        assert (ref_a["value"] != ref_b["value"]).sum() > 200  # the clear is visible in this view
        _same(_host(out_a), ref_a, "frame A, submitted before the clear was uploaded")
        _same(_host(out_b), ref_b, "frame B, submitted after it")
        full = oracle.trace_primary(t.flatten(), cam, 0, 0, W, H, fields=("value", "depth"))
        assert np.array_equal(full["value"], ref_b["value"])
        a.close()
        b.close()
        s.close()
    finally:
        owner.close()


def test_streamed_mips_on_device_after_clears(oracle):
    """A MIP-enabled stream on a device context after clears: the device traces like the oracle on the host mirror
    with the mirror's node MIPs."""
    size, bd = 64, 4
    t = _tree(size, bd)
    t.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
    rt = vhx.Raytracer(0)
    try:
        s = vhx.StreamingView(t, rt, (24.0, 20.0, 28.0), 32.0)
        s.set_rates(16, 64, 10)
        assert s.upload_all()[0]["pending"] == 0
        rng = np.random.default_rng(9)
        o, d = _rays_in_box(rng, np.zeros(3), np.full(3, float(size)), 20000)
        with oracle.node_mips(s.node_mips()):
            before = oracle.trace_rays(s.view(), o, d, fields=FIELDS)
        for c in [(16, 0, 16), (0, 16, 32), (32, 16, 0)]:
            t.clear_at_lod(c, 16)
        for _ in range(150):
            x, y, z = (int(v) for v in rng.integers(6, 42, 3))
            t.clear((x, y, z))
        t.clear_at_lod((12, 20, 28), 4)
        assert s.upload_all()[0]["pending"] == 0
        got = rt.trace_rays(o, d, fields=FIELDS)
        with oracle.node_mips(s.node_mips()):
            ref = oracle.trace_rays(s.view(), o, d, fields=FIELDS)
        assert_same(got, ref, "streamed MIP view after clears")
        assert (ref["value"] != N.VHX_EMPTY).mean() > 0.2
        assert (before["value"] != ref["value"]).sum() > 200
        s.close()
    finally:
        rt.close()
