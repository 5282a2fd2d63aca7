"""Glass cameras built by hand for the sky-block tests (tests/test_skyblock.py, tests/test_gpu_skyblocks.py)."""
import numpy as np

from voxelhex_amd import _native as N

f32 = np.float32


def hand_camera(W, H, origin, bl, right, up, pw, ph):
    cam = N.Camera()
    cam.ray_model = N.VHX_RAY_GLASS
    cam.width, cam.height = W, H
    cam.origin[:] = [float(f32(v)) for v in origin]
    cam.glass_bottom_left[:] = [float(f32(v)) for v in bl]
    cam.glass_right[:] = [float(f32(v)) for v in right]
    cam.glass_up[:] = [float(f32(v)) for v in up]
    cam.pixel_width, cam.pixel_height = float(f32(pw)), float(f32(ph))
    return cam


def aimed_camera(W, H, origin, target, gw=4.0, fov=3.0):
    """glass_camera's construction from any origin (up = +y)."""
    o, t = np.array(origin, np.float64), np.array(target, np.float64)
    d = (t - o) / np.linalg.norm(t - o)
    up = np.array([0.0, 1.0, 0.0])
    r = np.cross(up, d)
    r /= np.linalg.norm(r)
    gh = gw * H / W
    bl = o + d * fov - up * gh / 2 - r * gw / 2
    return hand_camera(W, H, o, bl, r, up, gw / W, gh / H)
