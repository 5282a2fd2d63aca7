"""The block classification of voxelhex_amd/csrc/skyblock.hpp, compiled for the host (tests/skyblock_c/) and checked
against the oracle pixel by pixel.

A 16x16 block is truly sky when the oracle's primary ray of every one of its pixels inside the frame never enters the
root cube: vhx_oracle_ray_steps gives 0 steps for such a ray and at least one node iteration for any other. That
depends on the tree only through its size, so the trees here hold a single voxel.

Soundness is a condition, not a measurement: no classified block may contain a pixel that enters the cube.
Usefulness: at least 85 % of the headline camera's truly all-sky blocks classify (so that a classifier that rejects
everything cannot pass). The headline camera is checked exhaustively at 3840x2160; the angles round the glass circle
and the orbit's 0.01 rad steps use the same geometry at 960x540, which keeps each case to a second or two."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import voxelhex_amd as vhx
from tests._skycams import aimed_camera, hand_camera
from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import TREE_ARRAYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "skyblock_c", "_build", "libskyblock.so")
f32 = np.float32


class SkyCam(ctypes.Structure):
    _fields_ = [("model", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("o", ctypes.c_float * 3), ("bl", ctypes.c_float * 3), ("r", ctypes.c_float * 3),
                ("u", ctypes.c_float * 3), ("pw", ctypes.c_float), ("ph", ctypes.c_float)]


@pytest.fixture(scope="module")
def shim():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "skyblock_c")], check=True)
    lib = ctypes.CDLL(SHIM)
    lib.vhx_sky_mask.argtypes = [ctypes.POINTER(SkyCam), ctypes.c_uint32, ctypes.c_void_p]
    return lib


_trees = {}


def _tree(size):
    """Any tree of that size will do: the one-node image of a solid cube (a UniformLeaf root over a Solid brick, what
    the simplified dense build gives for a full grid), where a ray that enters the cube hits at its first step -- in an
    empty tree it would restart from the root every 0.1 units along its way."""
    if size not in _trees:
        full = vhx.FlatTree.from_dense(np.full((16, 16, 16), 0xFF0000FF, np.uint32), 16, 4, simplify=True)
        assert full.desc.node_count == 1 and full.desc.brick_count == 0
        _trees[size] = vhx.TreeImage(size, 4, {name: np.array(getattr(full, name)) for name, _ in TREE_ARRAYS})
    return _trees[size]


def classify(shim, cam, size):
    s = SkyCam(cam.ray_model, cam.width, cam.height, cam.origin, cam.glass_bottom_left, cam.glass_right,
               cam.glass_up, cam.pixel_width, cam.pixel_height)
    bx, by = (cam.width + 15) // 16, (cam.height + 15) // 16
    mask = np.zeros(bx * by, np.uint8)
    assert shim.vhx_sky_mask(ctypes.byref(s), size, mask.ctypes.data) == 0
    return mask.reshape(by, bx).astype(bool)


def truly_sky(oracle, cam, size):
    W, H = cam.width, cam.height
    l = oracle.lib
    l.vhx_oracle_ray_steps.argtypes = [ctypes.POINTER(N.TreeDesc), ctypes.POINTER(N.Camera)] + \
        [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_int]
    steps = np.empty(W * H, np.uint32)
    assert l.vhx_oracle_ray_steps(ctypes.byref(_tree(size).desc), ctypes.byref(cam), 0, 0, W, H, steps.ctypes.data,
                                  0) == 0
    bx, by = (W + 15) // 16, (H + 15) // 16
    pad = np.zeros((by * 16, bx * 16), bool)  # pixels past the frame edge are no pixels
    pad[:H, :W] = steps.reshape(H, W) != 0
    return ~pad.reshape(by, 16, bx, 16).any(axis=(1, 3))


def check_sound(shim, oracle, cam, size, what):
    got, sky = classify(shim, cam, size), truly_sky(oracle, cam, size)
    bad = got & ~sky
    assert not bad.any(), f"{what}: {int(bad.sum())} classified blocks hold a pixel that enters the cube, first " \
                          f"(by, bx) = {tuple(np.argwhere(bad)[0])}"
    return got, sky


def test_headline_camera_exhaustive_and_useful(shim, oracle):
    S, W, H = 1024, 3840, 2160
    cam = vhx.glass_camera(S, W, H, target=(S / 2,) * 3)
    got, sky = check_sound(shim, oracle, cam, S, "headline")
    share = got.sum() / sky.sum()
    print(f"headline: {int(sky.sum())} of {sky.size} blocks all-sky, {int(got.sum())} classified ({share:.3f})")
    assert 0.5 < sky.mean() < 0.9  # the frame the issue describes: about two thirds sky
    assert share >= 0.85


@pytest.mark.parametrize("angle", [40.0 + k * math.pi / 6 for k in range(12)] + [40.0 + 0.01 * k for k in range(1, 9)])
def test_angles_round_the_glass_circle_and_orbit_steps(shim, oracle, angle):
    S = 1024
    cam = vhx.glass_camera(S, 960, 540, angle=angle, target=(S / 2,) * 3)
    got, sky = check_sound(shim, oracle, cam, S, f"angle {angle}")
    assert got.sum() >= 0.8 * sky.sum()


def test_1080p_at_256(shim, oracle):
    S = 256
    cam = vhx.glass_camera(S, 1920, 1080, target=(S / 2,) * 3)
    got, sky = check_sound(shim, oracle, cam, S, "1920x1080 at 256")
    assert got.sum() >= 0.85 * sky.sum()


@pytest.mark.parametrize("W,H", [(250, 130), (17, 16), (256, 256), (1, 1), (16, 33)])
@pytest.mark.parametrize("size", [64, 16])
def test_frames_that_are_no_multiple_of_16(shim, oracle, W, H, size):
    cam = vhx.glass_camera(size, W, H, target=(size / 2,) * 3)
    check_sound(shim, oracle, cam, size, f"{W}x{H} at {size}")


def test_camera_inside_the_cube_classifies_nothing(shim, oracle):
    S = 64
    for origin in ((S / 2, S / 2, S / 2), (1.0, 63.0, 5.0), (0.5, 0.5, 0.5)):
        cam = aimed_camera(256, 256, origin, (S * 2.0, -S, S * 3.0))
        got, sky = check_sound(shim, oracle, cam, S, f"inside {origin}")
        assert not sky.any() and not got.any()


def test_camera_aimed_away_from_the_tree(shim, oracle):
    S = 64
    cam = vhx.glass_camera(S, 256, 256, target=(S * 4.0, S * 6.0, -S * 4.0))
    got, sky = check_sound(shim, oracle, cam, S, "aimed away")
    assert sky.all()
    print(f"aimed away: {int(got.sum())} of {got.size} blocks classified")
    assert got.mean() > 0.9


@pytest.mark.parametrize("origin", [(0.0, 160.0, 64.0), (64.0, 0.0, -90.0), (-70.0, 64.0, 0.0), (0.0, 0.0, -100.0),
                                    (64.0, 64.0, 200.0), (0.0, 32.0, 32.0), (32.0, 64.0, 40.0)])
def test_origin_coordinate_exactly_zero_or_size(shim, oracle, origin):
    S = 64
    for target in ((S / 2,) * 3, (S / 2, S / 2, -S * 10.0), (S * 3.0, S / 2, S / 2)):
        if tuple(target) == tuple(origin):
            continue
        check_sound(shim, oracle, aimed_camera(250, 130, origin, target), S, f"origin {origin} -> {target}")


def test_axis_aligned_glass_and_components_zero_across_the_frame(shim, oracle):
    S, W, H = 64, 256, 256
    pw = ph = 4.0 / W
    # looking down -z with right = -x and up = +y: v_z is one value over the whole frame, v_x and v_y cross zero
    o = (S / 2, S / 2, 3.0 * S)
    cams = [hand_camera(W, H, o, (o[0] + 2.0, o[1] - 2.0, o[2] - 3.0), (-1, 0, 0), (0, 1, 0), pw, ph)]
    # v_y exactly zero in every pixel (no up vector, glass at the origin's height): inside the y slab, on its faces, and
    # outside it (every t of that axis infinite or NaN on the exact path)
    for oy in (S / 2, 0.0, float(S), 2.0 * S, -1.0):
        oo = (-S, oy, S / 2)
        cams.append(hand_camera(W, H, oo, (oo[0] + 3.0, oy, oo[2] - 2.0), (0, 0, 1), (0, 0, 0), pw, ph))
    # v_x and v_y both zero everywhere, v_z varies and crosses zero
    cams.append(hand_camera(W, H, (S / 2, S / 2, -S), (S / 2, S / 2, -S - 2.0), (0, 0, 1), (0, 0, 0), pw, ph))
    # a zero direction in every pixel
    cams.append(hand_camera(W, H, (-S, -S, -S), (-S, -S, -S), (0, 0, 0), (0, 0, 0), pw, ph))
    for i, cam in enumerate(cams):
        check_sound(shim, oracle, cam, S, f"axis-aligned camera {i}")


def test_radius_so_large_that_the_cube_covers_less_than_a_block(shim, oracle):
    S = 64
    for radius in (1e4, 1e6):
        cam = vhx.glass_camera(S, 256, 256, radius=radius, target=(S / 2,) * 3)
        got, sky = check_sound(shim, oracle, cam, S, f"radius {radius}")
        assert (~sky).sum() <= 4  # the cube sits inside one block, or on a corner shared by up to four


def test_non_finite_and_huge_cameras_classify_nothing(shim):
    S = 64
    base = vhx.glass_camera(S, 64, 64, target=(S / 2,) * 3)
    for field, k, v in (("origin", 0, float("nan")), ("origin", 1, float("inf")), ("glass_bottom_left", 2, -float("inf")),
                        ("glass_right", 0, float("nan")), ("glass_up", 1, 1e30), ("origin", 2, 3e12)):
        cam = N.Camera.from_buffer_copy(base)
        getattr(cam, field)[k] = v
        assert not classify(shim, cam, S).any(), (field, k, v)
    cam = N.Camera.from_buffer_copy(base)
    cam.pixel_width = float("nan")
    assert not classify(shim, cam, S).any()


def test_matrix_model_camera_classifies_nothing(shim):
    S = 64
    vp = vhx.Viewport(origin=(S * 2.0, S * 2.0, S * 2.0), direction=(-0.577, -0.577, -0.577), frustum=(1.0, 1.0, 1000.0),
                      fov=60.0)
    vp.update_matrices((128, 128))
    cam = vp.camera(128, 128)
    assert cam.ray_model != N.VHX_RAY_GLASS
    assert not classify(shim, cam, S).any()
