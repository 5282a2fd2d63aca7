"""Batch pass 0 with its workgroup-uniform values in scalar registers (k_trace_primary_batch: the workgroup's frame and
frame block, the frame's camera and output pointers, the block order's divisions as host-computed multipliers): a wrong
frame index, a wrong hoisted division or a wrong output pointer must show, so every frame of a batch has its own camera
and its own set of outputs, the frame sizes are no whole tiles of the list order and give workgroup counts that are no
multiple of the XCD run, and the block orders (interleaved and frame-major, XCD runs of 0, 16, 64 and the
non-power-of-two 12, listed and row-major) are all run. Every field of every frame is compared bit for bit with the
CPU oracle; the fused-shadow batch with the separate shadow traces (tests/test_gpu_fused_shadows.py).
"""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import _native as N

pytestmark = pytest.mark.gpu

FIELDS = ("value", "cell", "voxel", "impact", "normal", "depth", "rgba")
# the frames of one batch write different sets of outputs (frame k: OUT_SETS[k % 3])
OUT_SETS = (FIELDS, ("rgba", "depth"), ("value",))
SIZES = ((97, 33), (200, 136), (272, 144))
COUNTS = (1, 2, 3, 5, 7)
FILL = 7

_cache = {}


def _flat(size, bd):
    key = ("flat", size, bd)
    if key not in _cache:
        _cache[key] = vhx.FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, size, bd)
    return _cache[key]


def _cam(size, W, H, k):
    return vhx.glass_camera(size, W, H, angle=40.0 + 0.3 * k, target=(size / 2,) * 3)


def _ref(oracle, size, bd, W, H, k):
    """The oracle's frame of camera k (computed once per module, never modified)."""
    key = ("ref", size, bd, W, H, k)
    if key not in _cache:
        r = oracle.trace_primary(_flat(size, bd), _cam(size, W, H, k), 0, 0, W, H, fields=FIELDS)
        _cache[key] = {f: np.ascontiguousarray(r[f]).view(np.uint32).reshape(W * H, -1) for f in FIELDS}
        for a in _cache[key].values():
            a.setflags(write=False)
    return _cache[key]


def _outs(n, fields):
    import torch
    shapes = {"voxel": (n, 3), "impact": (n, 3), "normal": (n, 3)}
    dts = {"impact": torch.float32, "normal": torch.float32, "depth": torch.float32}
    return {f: torch.full(shapes.get(f, (n,)), FILL, dtype=dts.get(f, torch.int32), device="cuda") for f in fields}


def _host(o, n):
    return {k: v.cpu().numpy().view(np.uint32).reshape(n, -1) for k, v in o.items()}


def _check_frames(rt, oracle, size, bd, W, H, nf, what):
    import torch
    cams = [_cam(size, W, H, k) for k in range(nf)]
    outs = [_outs(W * H, OUT_SETS[k % 3]) for k in range(nf)]
    torch.cuda.synchronize()
    rt.trace_primary_batch(cams, outs)
    rt.sync()
    for k in range(nf):
        ref, got = _ref(oracle, size, bd, W, H, k), _host(outs[k], W * H)
        for f in OUT_SETS[k % 3]:
            bad = int(np.count_nonzero(got[f] != ref[f]))
            assert bad == 0, f"{what}: {W}x{H}, {nf} frames, frame {k} field {f} differs at {bad} entries"


@pytest.mark.parametrize("finter", [0, 1])
@pytest.mark.parametrize("xcdg", [0, 16, 64, 12])
def test_batch_block_orders_vs_oracle(oracle, finter, xcdg):
    tune = f"finter={finter};xcdg={xcdg}"
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(_flat(64, 4))
        for W, H in SIZES:
            for nf in COUNTS:
                _check_frames(rt, oracle, 64, 4, W, H, nf, tune)
    finally:
        rt.close()
    assert (_ref(oracle, 64, 4, 200, 136, 0)["value"] != N.VHX_EMPTY).sum() > 1000


@pytest.mark.parametrize("tune", ["p0lists=0;xcdg=12", "p0lists=0;finter=0;xcdg=16"])
def test_batch_row_major_blocks_vs_oracle(oracle, tune):
    """Without pass-0 lists the frame blocks are row-major (the division by the blocks per row)."""
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(_flat(64, 4))
        for W, H in SIZES:
            _check_frames(rt, oracle, 64, 4, W, H, 5, tune)
    finally:
        rt.close()


def test_batch_brick_dim_8_vs_oracle(oracle):
    rt = vhx.Raytracer(0, tune="xcdg=12")
    try:
        rt.upload(_flat(128, 8))  # 64 is no size of a brick_dim 8 tree (8 * 4^k)
        _check_frames(rt, oracle, 128, 8, 200, 136, 3, "brick_dim 8")
        rt.set_tuning("finter=0;xcdg=16")
        _check_frames(rt, oracle, 128, 8, 272, 144, 5, "brick_dim 8, frame-major")
    finally:
        rt.close()


@pytest.mark.parametrize("tlists", [0, 1])
@pytest.mark.parametrize("finter", [0, 1])
def test_tile_set_batch_vs_oracle(oracle, tlists, finter):
    """Unequal tile sets (7, 6 and 1 tiles of the 20; the frame's last tile row is 24 pixels high): every entry of
    every set equals the oracle's pixel of its frame, and the padding entries stay untouched."""
    import torch
    size, W, H, T, stride, starts = 64, 160, 120, 32, 3, (0, 2, 17)
    tiles_x, ntiles = (W + T - 1) // T, ((W + T - 1) // T) * ((H + T - 1) // T)
    cams = [_cam(size, W, H, k) for k in range(3)]
    counts = [(ntiles - s + stride - 1) // stride for s in starts]
    assert counts == [7, 6, 1]
    rt = vhx.Raytracer(0, tune=f"tlists={tlists};finter={finter};xcdg=12")
    try:
        rt.upload(_flat(size, 4))
        outs = [_outs(c * T * T, OUT_SETS[k % 3]) for k, c in enumerate(counts)]
        torch.cuda.synchronize()
        rt.trace_tiles_batch(cams, T, starts, stride, outs)
        rt.sync()
        for k, c in enumerate(counts):
            ref, got = _ref(oracle, size, 4, W, H, k), _host(outs[k], c * T * T)
            # entry j * T * T + ly * T + lx is pixel (tx * T + lx, ty * T + ly) of tile starts[k] + j * stride
            e = np.arange(c * T * T)
            tile = starts[k] + (e // (T * T)) * stride
            px, py = (tile % tiles_x) * T + e % T, (tile // tiles_x) * T + (e // T) % T
            inside = (px < W) & (py < H)
            assert inside.sum() < e.size, "no padding entry: the case tests less than it says"
            for f in OUT_SETS[k % 3]:
                fill = np.full(1, FILL, np.float32 if f in ("impact", "normal", "depth") else np.uint32)
                want = np.full(got[f].shape, fill.view(np.uint32)[0], np.uint32)
                want[inside] = ref[f][(py * W + px)[inside]]
                bad = int(np.count_nonzero(got[f] != want))
                assert bad == 0, f"tlists {tlists} finter {finter}: set {k} field {f} differs at {bad} entries"
    finally:
        rt.close()


def test_fused_shadow_batch_equals_separate_traces():
    """The FUSE instantiation: three frames with a light set against vhx_trace_primary + vhx_trace_shadows per frame."""
    import torch
    from tests.test_gpu_fused_shadows import _assert_same, _host as _shost, _outs as _souts, _separate
    size, W, H = 64, 200, 136
    light = (float(size),) * 3
    cams = [_cam(size, W, H, k) for k in range(3)]
    sep = vhx.Raytracer(0)
    fus = vhx.Raytracer(0, tune="xcdg=12")
    try:
        sep.upload(_flat(size, 4))
        fus.upload(_flat(size, 4))
        fus.set_shadow_light(light)
        outs = [_souts(W * H) for _ in cams]
        torch.cuda.synchronize()
        fus.trace_primary_batch(cams, outs)
        fus.sync()
        shadowed = 0
        for k, cam in enumerate(cams):
            ref = _separate(sep, cam, light)
            _assert_same(_shost(outs[k]), ref, f"fused batch frame {k}")
            shadowed += int((ref["shadowed"] == 1).sum())
        assert shadowed > 0, "no shadowed pixel: the case tests nothing"
    finally:
        sep.close()
        fus.close()
