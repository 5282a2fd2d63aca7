"""Sky blocks in a batch's pass 0 (tune "skyblocks", vhx_ctx::skyblocks): the 16x16 blocks that k_classify_sky marks
write their miss records and leave before the traversal prologue. With the switch on, every plane of every frame must
equal the switch off bit for bit, and the oracle -- outputs pre-filled with a pattern, all seven planes requested.

The path is taken by vhx_trace_primary_batch of whole frames without fused shadows. The lone-frame kernel, tile sets and
the fused-shadow instantiations keep the full path for every block and are not covered here."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from tests._skycams import aimed_camera
from voxelhex_amd import _native as N

pytestmark = pytest.mark.gpu

FIELDS = ("value", "cell", "voxel", "impact", "normal", "depth", "rgba")
S = 64


def _outs(n):
    import torch
    shapes = {"voxel": (n, 3), "impact": (n, 3), "normal": (n, 3)}
    dts = {"impact": torch.float32, "normal": torch.float32, "depth": torch.float32}
    return {f: torch.full(shapes.get(f, (n,)), 7, dtype=dts.get(f, torch.int32), device="cuda") for f in FIELDS}


def _trace(rt, cams):
    import torch
    outs = [_outs(cams[0].width * cams[0].height) for _ in cams]
    torch.cuda.synchronize()
    rt.trace_primary_batch(cams, outs)
    rt.sync()
    return [{k: v.cpu().numpy().view(np.uint32).reshape(-1) for k, v in o.items()} for o in outs]


def _batch(flat, cams, tune):
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(flat)
        return _trace(rt, cams)
    finally:
        rt.close()


_flat, _ref = {}, {}


def flat_of(size=S, bd=4):
    if (size, bd) not in _flat:
        _flat[(size, bd)] = vhx.FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, size, bd)
    return _flat[(size, bd)]


def oracle_frame(oracle, size, bd, cam):
    """The oracle's frame, computed once per (tree, camera) and shared by the cases."""
    key = (size, bd, bytes(cam))
    if key not in _ref:
        r = oracle.trace_primary(flat_of(size, bd), cam, 0, 0, cam.width, cam.height, fields=FIELDS)
        _ref[key] = {f: r[f].view(np.uint32).reshape(-1) for f in FIELDS}
    return _ref[key]


def orbit(W, H, n, size=S):
    return [vhx.glass_camera(size, W, H, angle=40.0 + 0.3 * k, target=(size / 2,) * 3) for k in range(n)]


def check(oracle, cams, tune, what, size=S, bd=4):
    sep = ";" if tune else ""
    on = _batch(flat_of(size, bd), cams, f"{tune}{sep}skyblocks=1")
    off = _batch(flat_of(size, bd), cams, f"{tune}{sep}skyblocks=0")
    for k, cam in enumerate(cams):
        ref = oracle_frame(oracle, size, bd, cam)
        for f in FIELDS:
            bad = int(np.count_nonzero(on[k][f] != off[k][f]))
            assert bad == 0, f"{what}: frame {k} field {f}: skyblocks=1 differs from skyblocks=0 at {bad} entries"
            bad = int(np.count_nonzero(on[k][f] != ref[f]))
            assert bad == 0, f"{what}: frame {k} field {f} differs from the oracle at {bad} entries"
    return on


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("W,H", [(256, 256), (250, 130)])
def test_batches_of_distinct_cameras(oracle, W, H, n):
    got = check(oracle, orbit(W, H, n), "", f"{W}x{H} batch of {n}")
    hits = (got[0]["value"] != N.VHX_EMPTY).sum()
    assert 100 < hits < 3 * W * H // 4  # tree blocks and sky blocks in one frame


@pytest.mark.parametrize("tune", ["finter=0", "p0lists=0", "p0lists=0;finter=0", "budgets=8,24,72", "budgets=",
                                  "xcdg=0", "qorder=0"])
def test_schedules_and_block_orders(oracle, tune):
    check(oracle, orbit(250, 130, 3), tune, tune)


def test_all_sky_camera_writes_every_pixel(oracle):
    cams = [vhx.glass_camera(S, 250, 130, angle=40.0 + 0.3 * k, target=(S * 4.0, S * 6.0, -S * 4.0)) for k in range(3)]
    for tune in ("", "p0lists=0"):
        got = check(oracle, cams, tune, f"all sky {tune}")
        for g in got:
            assert (g["value"] == N.VHX_EMPTY).all() and (g["rgba"] == 0xFF808080).all()


def test_inside_and_far_cameras(oracle):
    inside = [aimed_camera(250, 130, o, (S * 2.0, -S, S * 3.0)) for o in ((S / 2,) * 3, (1.0, 63.0, 5.0))]
    check(oracle, inside, "", "inside")
    far = [vhx.glass_camera(S, 256, 256, radius=r, target=(S / 2,) * 3) for r in (3000.0, 1e4, 1e6)]
    check(oracle, far, "", "far")
    check(oracle, [inside[0], vhx.glass_camera(S, 250, 130, target=(S / 2,) * 3), inside[1]], "", "mixed")


@pytest.mark.parametrize("bd,size", [(1, 16), (2, 32), (4, 64), (8, 128), (16, 256), (32, 512)])
def test_every_brick_dim(oracle, bd, size):
    check(oracle, orbit(200, 136, 2, size), "", f"bd {bd}", size, bd)


def test_two_contexts_tracing_batches_at_once(oracle):
    """Each context has a mask of its own: batches in flight on two contexts, every frame against its lone trace."""
    import torch
    W, H = 250, 130
    owner = vhx.Raytracer(0, tune="skyblocks=1")
    try:
        owner.upload(flat_of())
        other = owner.shared()
        cams = [vhx.glass_camera(S, W, H, angle=40.0 + 0.2 * k, target=(S / 2,) * 3) for k in range(18)]
        outs = [_outs(W * H) for _ in cams]
        torch.cuda.synchronize()
        for b in range(6):
            (owner if b % 2 == 0 else other).trace_primary_batch(cams[3 * b:3 * b + 3], outs[3 * b:3 * b + 3])
        owner.sync()
        other.sync()
        for k, cam in enumerate(cams):
            ref = owner.trace_primary(cam, fields=FIELDS)
            for f in FIELDS:
                got = outs[k][f].cpu().numpy().view(np.uint32).reshape(-1)
                assert np.array_equal(got, ref[f].view(np.uint32).reshape(-1)), (k, f)
        other.close()
    finally:
        owner.close()
