"""The MIP instantiations of the trace kernels (k_trace_primary, k_trace_rays, k_trace_queue with MIP = true, and the
MIP dispatch of vhx_trace_shadows) against the oracle at every brick_dim they are built for (1, 2, 4, 8, 16, 32), on the
views of tests/_mip_cases.py: flatten_lod cuts and hand-cut images of the random trees of tests/test_gpu_fuzz.py (Solid
bricks, UniformLeaf nodes, data and Complex voxels), with sampled MIP bricks and with Solid, VHX_EMPTY and foreign
Parted descriptors, stand-ins under Internal and under Leaf nodes; and on the images vhx_build_lod makes on the device.
tests/test_mip_cases.py states, on the oracle alone, that these views do trace their stand-ins.

Every field is compared as uint32 bits with no tolerance (assert_bits): the oracle's outputs hold no NaN on these
inputs, and the kernels are meant to be bit-exact. Each view is traced under the adaptive schedule, in one unbounded
pass, and under budgets (1, 3, 9), where every ray is abandoned and resumed many times and the MIP queue kernel runs."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from tests import _lod_grids as L
from tests import _mip_cases as M
from tests._skycams import aimed_camera
from tests.test_gpu_parity import _device_hits, rand_rays

pytestmark = pytest.mark.gpu

W, H = M.W, M.H
TILE, STRIDES = 20, 2  # no multiple of the 8x8 wave tile, and tiles that overhang the 96x64 frame


@pytest.fixture(scope="module")
def rt():
    r = vhx.Raytracer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def src():
    r = vhx.Raytracer(0)
    yield r
    r.close()


def _set_schedule(rt, schedule):
    if schedule == "adaptive":
        rt.set_adaptive_schedule(True)
    else:
        rt.set_pass_budgets(schedule)


def _untiled_rgba(rt, cam):
    """The frame traced in VHX_LAYOUT_TILES, one call per stride, mapped back to a framebuffer by vhx_untile_rgba."""
    import torch
    ntiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    per = (ntiles + STRIDES - 1) // STRIDES
    gathered = torch.zeros(STRIDES * per * TILE * TILE, dtype=torch.int32, device="cuda")
    for r in range(STRIDES):
        part = rt.trace_primary(cam, tile_size=TILE, tile_start=r, tile_stride=STRIDES, layout=N.VHX_LAYOUT_TILES,
                                fields=("rgba",))["rgba"]
        at = r * per * TILE * TILE
        gathered[at: at + part.size] = torch.from_numpy(part.view(np.int32)).cuda()
    fb = torch.zeros(W * H, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the fills and copies run on torch's stream, the untile on the context's
    rt.untile_rgba(gathered.data_ptr(), STRIDES, per, TILE, W, H, fb.data_ptr())
    rt.sync()
    return fb.cpu().numpy().view(np.uint32)


def _check_shadows(oracle, rt, image, cam, light, ref_frame, what):
    """vhx_trace_shadows on the frame's device hit records against the oracle's shadow rays from its own frame (call
    inside oracle.node_mips)."""
    hits = rt.trace_primary(cam, out=_device_hits(W * H))
    res = rt.trace_shadows(light, hits)
    rt.sync()
    ref = oracle.trace_shadows(image, light, ref_frame)
    got = {"value": hits["value"].cpu().numpy(), "shadowed": res["shadowed"].cpu().numpy(),
           "rgba": hits["rgba"].cpu().numpy()}
    M.assert_bits(got, {"value": ref_frame["value"], "shadowed": ref["shadowed"], "rgba": ref["rgba"]}, what)
    return int(ref["shadowed"].sum())


@pytest.mark.parametrize("seed,size,bd", M.CASES)
def test_mip_views_vs_oracle(oracle, rt, seed, size, bd):
    c = M.case(seed, size, bd)
    views = M.mip_views(seed, size, bd)
    o, d, cam = c.origins, c.directions, c.camera
    light = (float(size),) * 3
    # shadows: one proper flatten_lod cut (where the case has one) and the "both" hand-cut; tiles: the mixed one
    shadow_views = {"both/sampled"} | {v.name for v in views[:1] if not v.full}
    tile_view = "both/mixed"
    assert {tile_view, "both/sampled"} <= {v.name for v in views}
    try:
        for v in views:
            what = f"seed {seed} {size}/{bd} {v.name}"
            with oracle.node_mips(v.node_mips):
                ref_rays = oracle.trace_rays(v.image, o, d, fields=M.FIELDS)
                ref_frame = oracle.trace_primary(v.image, cam, 0, 0, W, H, fields=M.FIELDS)
            rt.upload(v.image)
            rt.set_node_mips(v.node_mips)
            for schedule in M.SCHEDULES:
                _set_schedule(rt, schedule)
                M.assert_bits(rt.trace_rays(o, d, fields=M.FIELDS), ref_rays, f"{what} rays {schedule}")
                M.assert_bits(rt.trace_primary(cam, fields=M.FIELDS), ref_frame, f"{what} frame {schedule}")
                if v.name == tile_view:
                    M.assert_bits({"rgba": _untiled_rgba(rt, cam)}, {"rgba": ref_frame["rgba"]},
                                  f"{what} tiles {schedule}")
                if v.name in shadow_views:
                    with oracle.node_mips(v.node_mips):
                        n = _check_shadows(oracle, rt, v.image, cam, light, ref_frame, f"{what} shadows {schedule}")
                    if schedule == M.SCHEDULES[0]:
                        print(f"{what}: {int((ref_frame['value'] != N.VHX_EMPTY).sum())} pixels hit, {n} shadowed")
            if v.full:  # every child is present: MIPs on = MIPs off = the reference path
                exact_rays = oracle.trace_rays(v.image, o, d, fields=M.FIELDS)
                exact_frame = oracle.trace_primary(v.image, cam, 0, 0, W, H, fields=M.FIELDS)
                M.assert_bits(ref_rays, exact_rays, f"{what}: the oracle with MIPs against its reference path")
                M.assert_bits(ref_frame, exact_frame, f"{what}: the oracle with MIPs against its reference path")
                rt.set_node_mips(None)
                for schedule in M.SCHEDULES:
                    _set_schedule(rt, schedule)
                    M.assert_bits(rt.trace_rays(o, d, fields=M.FIELDS), exact_rays, f"{what} rays, MIPs off {schedule}")
                    M.assert_bits(rt.trace_primary(cam, fields=M.FIELDS), exact_frame,
                                  f"{what} frame, MIPs off {schedule}")
    finally:
        rt.set_node_mips(None)
        rt.set_adaptive_schedule(True)


LOD_SOURCES = [(name, kind) for name, kind in M.device_lod_sources() if L.SHAPES[name][2] > 0]  # 4/1 has no cut


@pytest.mark.parametrize("name,kind", LOD_SOURCES)
def test_device_built_lod_vs_oracle(oracle, rt, src, name, kind):
    """vhx_build_lod's image and descriptors, read back and traced by the oracle, against the device's own traces of
    them -- the comparison tests/test_gpu_build_lod.py cannot make, where both sides run the MIP kernels."""
    size, bd, depth = L.SHAPES[name]
    M.build_lod_source(src, name, kind)
    o, d = rand_rays(np.random.default_rng(size * 13 + bd), size, M.RAYS)
    c = size / 2
    cam = aimed_camera(W, H, (-0.8 * size, 1.3 * size, -1.1 * size), (c, c * 0.4, c))
    changed = 0
    try:
        for method in L.METHODS:
            for depth_cut in range(depth):
                what = f"{name} {kind} {method} depth {depth_cut}"
                rt.build_lod(src, depth_cut, method)
                image, mips = rt.download(), rt.node_mips()
                with oracle.node_mips(mips):
                    ref_rays = oracle.trace_rays(image, o, d, fields=M.FIELDS)
                    ref_frame = oracle.trace_primary(image, cam, 0, 0, W, H, fields=M.FIELDS)
                changed += int(M.changed_rays(ref_rays, oracle.trace_rays(image, o, d, fields=M.FIELDS)).sum())
                changed += int(M.changed_rays(ref_frame, oracle.trace_primary(image, cam, 0, 0, W, H,
                                                                              fields=M.FIELDS)).sum())
                for schedule in ("adaptive", (1, 3, 9)):
                    _set_schedule(rt, schedule)
                    M.assert_bits(rt.trace_rays(o, d, fields=M.FIELDS), ref_rays, f"{what} rays {schedule}")
                    M.assert_bits(rt.trace_primary(cam, fields=M.FIELDS), ref_frame, f"{what} frame {schedule}")
        print(f"{name} {kind}: the node MIPs change {changed} rays and pixels")
        assert changed > 0, "no cut image showed a stand-in"
    finally:
        rt.set_adaptive_schedule(True)


def test_refusals_with_mips_leave_the_context_usable(oracle, rt):
    """Entry points that have no MIP kernel return VHX_E_INVALID_ARG while node MIPs are set, before any launch, and
    the next valid trace still equals the oracle."""
    import torch
    seed, size, bd = M.CASES[4]
    c = M.case(seed, size, bd)
    v = M.mip_views(seed, size, bd)[0]
    assert not v.full
    o, d, cam = c.origins, c.directions, c.camera
    with oracle.node_mips(v.node_mips):
        ref_rays = oracle.trace_rays(v.image, o, d, fields=M.FIELDS)
        ref_frame = oracle.trace_primary(v.image, cam, 0, 0, W, H, fields=M.FIELDS)
    n = W * H

    def dev(k=1, dtype=torch.int32):
        return torch.zeros((n, k) if k > 1 else (n,), dtype=dtype, device="cuda")

    def refused(call, what):
        with pytest.raises(N.VhxError) as e:
            call()
        assert e.value.code == N.VHX_E_INVALID_ARG, what
        M.assert_bits(rt.trace_rays(o, d, fields=M.FIELDS), ref_rays, f"rays after {what}")
        M.assert_bits(rt.trace_primary(cam, fields=M.FIELDS), ref_frame, f"frame after {what}")

    rt.upload(v.image)
    rt.set_node_mips(v.node_mips)
    try:
        refused(lambda: rt.trace_rays(o, d, count_bytes=True), "trace_rays(count_bytes=True)")
        hits = rt.trace_primary(cam, out=_device_hits(n))
        rt.sync()
        refused(lambda: rt.trace_shadows((float(size),) * 3, hits, count_bytes=True), "trace_shadows(count_bytes=True)")
        outs = [{"value": dev(), "rgba": dev()} for _ in range(2)]
        torch.cuda.synchronize()
        refused(lambda: rt.trace_primary_batch([cam, cam], outs), "trace_primary_batch")
        fused = {"value": dev(), "impact": dev(3, torch.float32), "normal": dev(3, torch.float32), "shadowed": dev(),
                 "rgba": dev()}
        torch.cuda.synchronize()
        rt.set_shadow_light((float(size),) * 3)
        with pytest.raises(N.VhxError) as e:
            rt.trace_primary(cam, out=fused)
        assert e.value.code == N.VHX_E_INVALID_ARG
        rt.set_shadow_light(None)
        M.assert_bits(rt.trace_rays(o, d, fields=M.FIELDS), ref_rays, "rays after a frame with a shadow light")
        M.assert_bits(rt.trace_primary(cam, fields=M.FIELDS), ref_frame, "frame after a frame with a shadow light")
    finally:
        rt.set_shadow_light(None)
        rt.set_node_mips(None)
