"""GPU raytracing API: the MI355X replacement of VoxelHex's `src/raytracing` module.

    Ray                      voxelhex::raytracing::Ray (src/spatial/raytracing/mod.rs:8-22)
    Raytracer                a libvhx context: one device, the tree resident in HBM (BoxTreeGPUHost + view,
                             src/raytracing/bevy/mod.rs:164-180, src/raytracing/bevy/view.rs:36-137)
    Raytracer.trace_rays     BoxTree::get_by_ray over a batch (src/raytracing/cpu.rs:296)
    Raytracer.get            BoxTree::get over a batch of positions (src/boxtree/mod.rs:223-317); read_dense: a box of
                             the tree as a dense albedo grid, the inverse of build_dense
    Raytracer.trace_primary  one frame of per-pixel primary rays (VhxRenderNode::run,
                             src/raytracing/bevy/pipeline/mod.rs:96-155, with the CPU frame semantics of
                             examples/gpu_render.rs:196-257)
    Viewport                 src/raytracing/bevy/types.rs:60-88 with update_matrices (src/raytracing/bevy/view.rs:211-239)
    glass_camera             the pinhole camera of benches/performance.rs:29-61

Every call goes through the HIP kernels of libvhx; there is no CPU path here.
"""
import ctypes
from dataclasses import dataclass, field
import math

import numpy as np

from . import _native as N
from .boxtree import V3c, FlatTree, TreeImage, TREE_ARRAYS, _TREE_ERRORS

f32 = np.float32
_libm = ctypes.CDLL("libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]


@dataclass
class Ray:
    origin: V3c
    direction: V3c

    def is_valid(self):
        d = np.array(list(self.direction), f32)
        return abs(f32(1) - _len(d)) < f32(0.000001)


# ---------------------------------------------------------------------------------------------- f32 V3c helpers
def _v(*a):
    return np.array(a, f32)


def _len(v):
    """V3c::length (src/spatial/math/vector.rs:71-73): sqrt((x*x + y*y) + z*z) in f32."""
    return f32(np.sqrt(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2])))


def _normalized(v):
    """V3c::normalized: v / length (three f32 divisions)."""
    l = _len(v)
    return np.array([v[0] / l, v[1] / l, v[2] / l], f32)


def _cross(a, b):
    """V3c::cross (src/spatial/math/vector.rs:196-202)."""
    return np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]),
                     f32(a[0] * b[1]) - f32(a[1] * b[0])], f32)


def glass_camera(tree_size, width, height, angle=40.0, radius=None, target=None, glass_width=4.0,
                 glass_height=None, fov=3.0):
    """Pinhole 'glass' camera of benches/performance.rs:32-61.

    The reference bench renders 128x128 rays through a 4x4 glass at distance 3 from a camera at
    (sin(40) R, R, cos(40) R), R = 2*tree_size, aimed at (0,0,0). Defaults keep that geometry; `target` re-aims it
    (SURVEY.md 8d aims at the tree centre) and glass_height defaults to 4*height/width so pixels stay square.
    Arithmetic is f32 in the reference's op order; sin/cos come from libm's sinf/cosf like Rust's f32::sin.
    """
    S = f32(tree_size)
    R = f32(2.0) * S if radius is None else f32(radius)
    a = f32(angle)
    origin = _v(f32(_libm.sinf(a)) * R, R, f32(_libm.cosf(a)) * R)
    tgt = _v(0, 0, 0) if target is None else np.array(target, f32)
    direction = _normalized(tgt - origin)
    up = _v(0, 1, 0)
    right = _normalized(_cross(up, direction))
    gw = f32(glass_width)
    gh = f32(glass_width * height / width) if glass_height is None else f32(glass_height)
    pw = f32(gw / f32(width))
    ph = f32(gh / f32(height))
    bl = ((origin + direction * f32(fov)) - up * f32(gh / f32(2))) - right * f32(gw / f32(2))
    cam = N.Camera()
    cam.ray_model = N.VHX_RAY_GLASS
    cam.width, cam.height = width, height
    cam.origin[:] = [float(v) for v in origin]
    cam.glass_bottom_left[:] = [float(v) for v in bl]
    cam.glass_right[:] = [float(v) for v in right]
    cam.glass_up[:] = [float(v) for v in up]
    cam.pixel_width = float(pw)
    cam.pixel_height = float(ph)
    return cam


@dataclass
class Viewport:
    """Viewport (src/raytracing/bevy/types.rs:60-88)."""
    origin: tuple
    direction: tuple
    frustum: tuple
    fov: float
    view_matrix: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=f32))
    projection_matrix: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=f32))
    inverse_view_projection_matrix: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=f32))

    def update_matrices(self, resolution):
        """Viewport::update_matrices (src/raytracing/bevy/view.rs:211-239); matrices stored column-major like glam.

        look_at_rh and perspective_rh follow glam 0.29's formulas in f32; the inverse is computed in f64 and
        rounded (glam's cofactor order is not restated: parity for this matrix is unpinned)."""
        fwd = np.array(self.direction, f32)
        right = _normalized(_cross(fwd, _v(0, 1, 0)))
        up = _normalized(_cross(right, fwd))
        eye = np.array(self.origin, f32)
        center = eye + fwd
        f = _normalized(center - eye)
        s = _normalized(_cross(f, up))
        u = _cross(s, f)
        view = np.zeros((4, 4), f32)  # [col][row]
        view[0] = [s[0], u[0], -f[0], 0]
        view[1] = [s[1], u[1], -f[1], 0]
        view[2] = [s[2], u[2], -f[2], 0]
        view[3] = [-np.dot(eye, s), -np.dot(eye, u), np.dot(eye, f), 1]
        aspect = f32(resolution[0]) / f32(resolution[1])
        fov_r = f32(math.radians(self.fov))
        near = f32(self.frustum[1]) / f32(2.0) / f32(_libm.tanf(fov_r / f32(2.0)))
        far = f32(self.frustum[2])
        half = f32(0.5) * fov_r
        h = f32(_libm.cosf(half)) / f32(_libm.sinf(half))
        w = h / aspect
        r = far / (near - far)
        proj = np.zeros((4, 4), f32)
        proj[0] = [w, 0, 0, 0]
        proj[1] = [0, h, 0, 0]
        proj[2] = [0, 0, r, -1]
        proj[3] = [0, 0, r * near, 0]
        # column-major storage: M[col][row]; math matrix = storage.T
        vp = (proj.T.astype(np.float64) @ view.T.astype(np.float64))
        self.view_matrix, self.projection_matrix = view, proj
        self.inverse_view_projection_matrix = np.linalg.inv(vp).T.astype(f32)

    def camera(self, width, height):
        self.update_matrices((width, height))
        cam = N.Camera()
        cam.ray_model = N.VHX_RAY_INVERSE_VP
        cam.width, cam.height = width, height
        cam.origin[:] = [float(v) for v in self.origin]
        cam.inv_view_proj[:] = [float(v) for v in self.inverse_view_projection_matrix.reshape(-1)]
        return cam


HIT_FIELDS = (("value", np.uint32, 1), ("cell", np.uint32, 1), ("voxel", np.uint32, 3), ("impact", np.float32, 3),
              ("normal", np.float32, 3), ("depth", np.float32, 1), ("rgba", np.uint32, 1), ("bytes", np.uint32, 1),
              ("shadowed", np.uint32, 1))


def _hits_struct(arrays):
    h = N.Hits()
    for name, _, _ in HIT_FIELDS:
        a = arrays.get(name)
        setattr(h, name, None if a is None else _ptr(a))
    return h


def _on_device(arrays):
    """1 when every array of an out= dict is a GPU tensor, 0 when every one is host memory (numpy / CPU tensor)."""
    dev = {bool(getattr(a, "is_cuda", False)) for a in arrays.values() if a is not None}
    if len(dev) > 1:
        raise ValueError("out= mixes device and host arrays")
    return 1 if dev == {True} else 0


def _ptr(a):
    if hasattr(a, "data_ptr"):  # torch tensor (device or host)
        return a.data_ptr()
    return a.ctypes.data


class _BuiltOnDevice:
    """Stands for a context's tree that exists only on the device (Raytracer.build_dense)."""


class Raytracer:
    """A libvhx context on one HIP device with a tree resident in HBM."""

    def __init__(self, device=0, tune=None):
        """tune: a vhx_set_tuning spec ("key=value;..."), scheduling knobs of experiments (results never change)."""
        lib = N.lib()
        n = ctypes.c_int()
        rc = lib.vhx_device_count(ctypes.byref(n))
        if rc != N.VHX_OK:
            raise N.VhxError(rc, "vhx_device_count: " + (lib.vhx_device_error() or b"").decode())
        if n.value == 0:
            raise RuntimeError("voxelhex_amd: no HIP device is visible (the raytracer has no CPU fallback)")
        h = ctypes.c_void_p()
        N.check(lib.vhx_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device
        self._tree = None
        if tune:
            self.set_tuning(tune)

    def set_tuning(self, spec):
        """vhx_set_tuning: scheduling knobs as "key=value;..." (include/vhx.h); a dict is joined the same way."""
        if isinstance(spec, dict):
            spec = ";".join(f"{k}={v}" for k, v in spec.items())
        self._check(N.lib().vhx_set_tuning(self._h, spec.encode()))

    def shared(self):
        """vhx_create_shared: another context (its own stream, queues and outputs) tracing this context's tree."""
        if self._tree is None:
            raise RuntimeError("upload a tree before sharing it")
        rt = Raytracer.__new__(Raytracer)
        h = ctypes.c_void_p()
        self._check(N.lib().vhx_create_shared(self._h, ctypes.byref(h)))
        rt._h, rt.device, rt._tree = h, self.device, self._tree
        return rt

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            N.lib().vhx_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except (TypeError, AttributeError):  # interpreter shutdown: module globals already torn down
            pass

    def _check(self, rc):
        return N.check(rc, self._h)

    def upload(self, flat: FlatTree):
        if self._tree is flat:
            return
        self._check(N.lib().vhx_upload_tree(self._h, ctypes.byref(flat.desc)))
        self._tree = flat

    def _data_plane(self, data, like, what):
        """The pointer of a data plane that goes with the grid `like` (a device tensor, or the contiguous numpy array a
        call passes down): the same kind, shape and device, under the same checks. Returns (pointer, keep-alive)."""
        if hasattr(like, "data_ptr"):
            if not hasattr(data, "data_ptr"):
                raise TypeError(f"{what}: the grid is a device tensor, so the data plane must be one")
            if tuple(data.shape) != tuple(like.shape):
                raise TypeError(f"{what}: the data plane has shape {tuple(data.shape)}, the grid {tuple(like.shape)}")
            data = self._device_tensor(data, what)
            return data.data_ptr(), data
        if hasattr(data, "data_ptr"):
            raise TypeError(f"{what}: the grid is a host array, so the data plane must be one")
        from .boxtree import _dense_data
        plane = _dense_data(data, like.shape)
        return plane.ctypes.data, plane

    def build_dense(self, grid, size, brick_dim, simplify=False, data=None):
        """vhx_build_tree_dense: builds the canonical tree of a dense grid on the GPU and makes it this context's tree
        (the image of FlatTree.from_dense + upload, bit for bit); with simplify=True the simplified tree
        (vhx_build_tree_dense_simplified, the image of FlatTree.from_dense(simplify=True)). `grid` has shape (gz, gy, gx) and holds packed albedos
        r | g<<8 | b<<16 | a<<24, alpha 0 = no voxel: a uint32 numpy array (copied to the device first), or a contiguous
        int32 / uint32 torch tensor on this context's device, read in place. The build runs on the context's stream,
        not on torch's: for a tensor, torch's current stream on the device is synchronised before the call, so the
        work that produced the grid has finished. The call returns when the tree is ready (download() reads it).
        `data` (optional) is a plane of user data values, 0 = none, of the same kind, shape and device as `grid`
        (vhx_build_tree_dense_data, the image of FlatTree.from_dense(data=)): a voxel with a colour and a data value is
        a Complex entry, one with a data value and alpha 0 an Informative one, and get / a trace return both palette
        indices. With `data` and simplify=True the call is the data build followed by self.simplify(), which gives the
        image of FlatTree.from_dense(data=, simplify=True); unlike the colour-only simplified build, which leaves the
        previous tree where it fails, a failure of that second step leaves the new, plain tree."""
        if hasattr(grid, "data_ptr"):
            import torch
            if not grid.is_cuda or grid.device.index != self.device:
                raise ValueError(f"build_dense: the tensor must live on device {self.device}")
            if grid.dim() != 3 or grid.dtype not in (torch.int32, torch.uint32) or not grid.is_contiguous():
                raise TypeError("build_dense: a contiguous int32 / uint32 tensor of shape (gz, gy, gx)")
            torch.cuda.current_stream(grid.device).synchronize()
            d = N.DenseDesc()
            d.boxtree_size, d.brick_dim = int(size), int(brick_dim)
            d.gz, d.gy, d.gx = (int(v) for v in grid.shape)
            d.albedo = grid.data_ptr()
            on_device = 1
        else:
            from .boxtree import _dense_desc
            d, grid = _dense_desc(grid, size, brick_dim)
            on_device = 0
        if data is not None:
            ptr, keep = self._data_plane(data, grid, "build_dense")
            rc = N.lib().vhx_build_tree_dense_data(self._h, ctypes.byref(d), ptr, on_device)
            del keep
        else:
            build = N.lib().vhx_build_tree_dense_simplified if simplify else N.lib().vhx_build_tree_dense
            rc = build(self._h, ctypes.byref(d), on_device)
        if rc in _TREE_ERRORS:
            raise _TREE_ERRORS[rc](f"size {size} brick_dim {brick_dim}")
        self._check(rc)
        self._tree = _BuiltOnDevice()
        if data is not None and simplify:
            self.simplify()

    def tree_counts(self):
        """vhx_tree_counts: sizes and counts of the uploaded tree."""
        d = N.TreeDesc()
        self._check(N.lib().vhx_tree_counts(self._h, ctypes.byref(d)))
        return d

    def read_range(self, buffer_id, elem_offset, elem_count):
        """vhx_read_range: elements of one raw tree buffer (VHX_BUF_*) copied back from the device."""
        a = np.empty(elem_count, TREE_ARRAYS[buffer_id][1])
        self._check(N.lib().vhx_read_range(self._h, buffer_id, elem_offset, elem_count, a.ctypes.data))
        return a

    def download(self):
        """The uploaded tree read back from the device (vhx_tree_counts + vhx_read_range): a TreeImage with the seven
        arrays and the counts."""
        d = self.tree_counts()
        n3 = d.brick_dim ** 3
        sizes = (d.node_count, d.node_count, d.node_count * 64, d.brick_count * n3, d.solid_count, d.color_count,
                 d.data_count)
        arrays = {name: self.read_range(i, 0, n) for i, ((name, _), n) in enumerate(zip(TREE_ARRAYS, sizes))}
        return TreeImage(d.boxtree_size, d.brick_dim, arrays)

    def _device_tensor(self, a, what):
        """A contiguous int32 / uint32 tensor on this context's device, with torch's current stream synchronised (the
        query runs on the context's stream, not on torch's)."""
        import torch
        if not a.is_cuda or a.device.index != self.device:
            raise ValueError(f"{what}: the tensor must live on device {self.device}")
        if a.dtype not in (torch.int32, torch.uint32) or not a.is_contiguous():
            raise TypeError(f"{what}: a contiguous int32 / uint32 tensor")
        torch.cuda.current_stream(a.device).synchronize()
        return a

    def get(self, positions):
        """vhx_get_voxels: BoxTree::get for a batch of positions, as PaletteIndexValues (N.VHX_EMPTY = none;
        boxtree.entry_from_value turns one into an entry over the palettes). `positions` is an (n, 3) integer numpy
        array (x, y, z per row), which gives a numpy uint32 array, or a contiguous int32 / uint32 torch tensor of that
        shape on this context's device, which gives a tensor of the same dtype there: torch's current stream is
        synchronised before the call and the context before the tensor is handed back."""
        if hasattr(positions, "data_ptr"):
            import torch
            if positions.dim() != 2 or positions.shape[1] != 3:
                raise TypeError("get: positions of shape (n, 3)")
            p = self._device_tensor(positions, "get")
            out = torch.empty(p.shape[0], dtype=p.dtype, device=p.device)
            self._check(N.lib().vhx_get_voxels(self._h, p.data_ptr(), p.shape[0], out.data_ptr(), 1))
            self.sync()
            return out
        p = np.asarray(positions)
        if p.ndim != 2 or p.shape[1] != 3 or p.dtype.kind not in "iu":
            raise TypeError("get: an integer array of shape (n, 3)")
        if p.size and (int(p.min()) < 0 or int(p.max()) > 0xFFFFFFFF):
            raise ValueError("get: positions are unsigned 32-bit")
        p = np.ascontiguousarray(p.astype(np.uint32, copy=False))
        out = np.empty(p.shape[0], np.uint32)
        self._check(N.lib().vhx_get_voxels(self._h, p.ctypes.data, p.shape[0], out.ctypes.data, 0))
        return out

    def read_dense(self, origin=(0, 0, 0), extents=None, out=None, data=False):
        """vhx_read_dense: the box at `origin` (x, y, z) with `extents` (gx, gy, gz; None = the whole root cube) as a
        dense grid of shape (gz, gy, gx) of packed albedos, 0 where there is no visible voxel -- the inverse of
        build_dense. `out` (optional) receives it: a C-contiguous uint32 numpy array, or a contiguous int32 / uint32
        torch tensor on this context's device (synchronised like get's); without it a numpy array is returned.
        data=True (vhx_read_dense_data) returns (albedo, data): the second grid holds every voxel's user data value,
        0 where it has none, read in the same walk of the tree. An array or tensor passed as `data` (of out's kind and
        shape; with out=None a numpy array) receives the data plane and is returned beside the albedo."""
        want_data = data is not False and data is not None
        ox, oy, oz = (int(v) for v in origin)
        if extents is None:
            extents = (self.tree_counts().boxtree_size,) * 3
        gx, gy, gz = (int(v) for v in extents)
        if min(ox, oy, oz) < 0 or min(gx, gy, gz) < 0:
            raise ValueError("read_dense: origin and extents are unsigned")
        if out is None:
            if want_data and hasattr(data, "data_ptr"):
                import torch
                out = torch.empty((gz, gy, gx), dtype=data.dtype, device=data.device)
            else:
                out = np.empty((gz, gy, gx), np.uint32)
        if want_data:
            if data is True:
                if hasattr(out, "data_ptr"):
                    import torch
                    data = torch.empty_like(out)
                else:
                    data = np.empty((gz, gy, gx), np.uint32)
            if tuple(data.shape) != (gz, gy, gx):
                raise ValueError(f"read_dense: data has shape {tuple(data.shape)}, the box needs {(gz, gy, gx)}")
            if hasattr(data, "data_ptr") != hasattr(out, "data_ptr"):
                raise TypeError("read_dense: out and data are both arrays or both tensors")
        if tuple(out.shape) != (gz, gy, gx):
            raise ValueError(f"read_dense: out has shape {tuple(out.shape)}, the box needs {(gz, gy, gx)}")
        box = N.DenseOut(ox, oy, oz, gx, gy, gz, None)
        if hasattr(out, "data_ptr"):
            box.albedo = self._device_tensor(out, "read_dense").data_ptr()
            if want_data:
                dptr = self._device_tensor(data, "read_dense").data_ptr()
                self._check(N.lib().vhx_read_dense_data(self._h, ctypes.byref(box), dptr, 1))
                self.sync()
                return out, data
            self._check(N.lib().vhx_read_dense(self._h, ctypes.byref(box), 1))
            self.sync()
            return out
        if out.dtype != np.uint32 or not out.flags.c_contiguous:
            raise TypeError("read_dense: out is a C-contiguous uint32 array")
        box.albedo = out.ctypes.data
        if want_data:
            if data.dtype != np.uint32 or not data.flags.c_contiguous:
                raise TypeError("read_dense: data is a C-contiguous uint32 array")
            self._check(N.lib().vhx_read_dense_data(self._h, ctypes.byref(box), data.ctypes.data, 0))
            return out, data
        self._check(N.lib().vhx_read_dense(self._h, ctypes.byref(box), 0))
        return out

    def write_dense(self, grid, origin=(0, 0, 0), mode="replace", data=None):
        """vhx_write_dense: the box at `origin` (x, y, z) with the extents of `grid` (shape (gz, gy, gx), packed albedos as
        for build_dense) replaced on the device, in place -- the inverse of read_dense. mode "replace": every voxel of
        the box becomes the grid's, alpha 0 clears; "insert": grid voxels with alpha 0 leave the tree as it is. `grid` is
        a uint32 numpy array (copied to the device first) or a contiguous int32 / uint32 torch tensor on this context's
        device, read in place (torch's current stream is synchronised before the call). Owner context only; the call
        returns when the tree is ready. Slots are never reused: orphans() counts the unlinked ones and compact() drops
        them.
        `data` (vhx_write_dense_data) gives the box's voxels user data values, 0 = none: a plane of the same kind,
        shape and device as `grid`, or an integer that every voxel of the box gets. A voxel of the box is then an entry
        where it has a colour or a data value ("replace" clears where it has neither, "insert" leaves the tree alone
        there), and a written voxel is replaced wholesale: an old data value does not survive under a colour written
        without one. New data values follow the data palette in the box's insert order.
        mode "update" (VHX_WRITE_UPDATE, the batched BoxTree.update) merges instead: a grid voxel with a colour
        recolours the tree's voxel and keeps its data value, a `data` value other than 0 retags it and keeps its colour,
        a voxel of the box with neither touches nothing, and an empty voxel that receives a half becomes a voxel.
        Without `data` the data values under the box stay as they are."""
        modes = {"replace": N.VHX_WRITE_REPLACE, "insert": N.VHX_WRITE_INSERT, "update": N.VHX_WRITE_UPDATE}
        box = N.DenseIn()
        box.ox, box.oy, box.oz = (int(v) for v in origin)
        box.mode = modes[mode] if mode in modes else int(mode)
        if hasattr(grid, "data_ptr"):
            if grid.dim() != 3:
                raise TypeError("write_dense: a tensor of shape (gz, gy, gx)")
            grid = self._device_tensor(grid, "write_dense")
            box.albedo, on_device = grid.data_ptr(), 1
        else:
            grid = np.ascontiguousarray(grid, np.uint32)
            if grid.ndim != 3:
                raise TypeError("write_dense: an array of shape (gz, gy, gx)")
            box.albedo, on_device = grid.ctypes.data, 0
        box.gz, box.gy, box.gx = (int(v) for v in grid.shape)
        if data is None:
            self._check(N.lib().vhx_write_dense(self._h, ctypes.byref(box), on_device))
        elif isinstance(data, (int, np.integer)):
            self._check(N.lib().vhx_write_dense_data(self._h, ctypes.byref(box), None, int(data), on_device))
        else:
            ptr, keep = self._data_plane(data, grid, "write_dense")
            self._check(N.lib().vhx_write_dense_data(self._h, ctypes.byref(box), ptr, 0, on_device))
            del keep

    def fill_box(self, origin, extents, albedo, data=0, mode="replace"):
        """vhx_write_dense without a grid: every voxel of the box at `origin` with `extents` (gx, gy, gz) becomes the
        packed colour `albedo`; 0 (or any colour with alpha 0) clears the box. `data` (vhx_write_dense_data) is the
        user data value every voxel of the box gets beside the colour, 0 = none -- fill_box(o, e, 0, 7) writes
        data-only voxels, fill_box(o, e, 0, 0) clears -- or a plane of shape (gz, gy, gx) with a value per voxel (a
        uint32 numpy array or a device tensor). `mode` is write_dense's: under "update" only the halves given are
        written -- fill_box(o, e, 0, 7, mode="update") gives every voxel of the box the data value 7, occupied ones
        keep their colour and empty ones become data-only voxels; fill_box(o, e, colour, 0, mode="update") recolours
        the box and keeps its data values."""
        modes = {"replace": N.VHX_WRITE_REPLACE, "insert": N.VHX_WRITE_INSERT, "update": N.VHX_WRITE_UPDATE}
        box = N.DenseIn()
        box.ox, box.oy, box.oz = (int(v) for v in origin)
        box.gx, box.gy, box.gz = (int(v) for v in extents)
        box.mode, box.fill, box.albedo = modes[mode] if mode in modes else int(mode), int(albedo), None
        if isinstance(data, (int, np.integer)):
            if int(data) == 0:
                self._check(N.lib().vhx_write_dense(self._h, ctypes.byref(box), 0))
            else:
                self._check(N.lib().vhx_write_dense_data(self._h, ctypes.byref(box), None, int(data), 0))
            return
        if tuple(data.shape) != (box.gz, box.gy, box.gx):
            raise ValueError(f"fill_box: data has shape {tuple(data.shape)}, the box needs {(box.gz, box.gy, box.gx)}")
        if hasattr(data, "data_ptr"):
            ptr, keep, on_device = self._device_tensor(data, "fill_box").data_ptr(), data, 1
        else:
            from .boxtree import _dense_data
            keep = _dense_data(data, data.shape)
            ptr, on_device = keep.ctypes.data, 0
        self._check(N.lib().vhx_write_dense_data(self._h, ctypes.byref(box), ptr, 0, on_device))
        del keep

    def set_voxels(self, positions, albedo=None, data=None, mode="replace"):
        """vhx_set_voxels: a list of voxels written into the device tree in place -- the batched BoxTree.insert / clear,
        and the counterpart of get. `positions` is an (n, 3) integer numpy array (x, y, z per row; copied to the device
        first), or a contiguous int32 / uint32 torch tensor of that shape on this context's device, read in place
        (torch's current stream is synchronised before the call, as for get and write_dense). `albedo` and `data` are
        arrays of the same kind with n packed colours / user data values (0 = none), or integers that every point gets
        (None = 0). A point with a colour or a data value is written, replacing its voxel wholesale; one with neither
        clears its voxel under mode "replace" and touches nothing under "insert". The result is that of the loop over
        the list: where points repeat a position the last one decides. New colours and data values follow the palettes
        in list order. Owner context only; the call returns when the tree is ready; slots are never reused (orphans(),
        compact()). Cost and scratch follow the points and the bricks they touch, not their bounding box.
        mode "update" (VHX_WRITE_UPDATE, the batched BoxTree.update) merges halves instead of replacing voxels: a
        point's colour (alpha not 0) replaces the voxel's colour, its data value (not 0) the voxel's data value, and
        the half a point does not have stays what it was; a point with neither touches nothing. Where points repeat a
        position, the last one with a colour decides the colour and the last one with a data value the data value."""
        modes = {"replace": N.VHX_WRITE_REPLACE, "insert": N.VHX_WRITE_INSERT, "update": N.VHX_WRITE_UPDATE}
        pts = N.PointsIn()
        pts.mode = modes[mode] if mode in modes else int(mode)
        keep = []
        if hasattr(positions, "data_ptr"):
            if positions.dim() != 2 or positions.shape[1] != 3:
                raise TypeError("set_voxels: positions of shape (n, 3)")
            p = self._device_tensor(positions, "set_voxels")
            n, on_device = int(p.shape[0]), 1
            pts.positions = p.data_ptr()
        else:
            p = np.asarray(positions)
            if p.ndim != 2 or p.shape[1] != 3 or p.dtype.kind not in "iu":
                raise TypeError("set_voxels: an integer array of shape (n, 3)")
            if p.size and (int(p.min()) < 0 or int(p.max()) > 0xFFFFFFFF):
                raise ValueError("set_voxels: positions are unsigned 32-bit")
            p = np.ascontiguousarray(p.astype(np.uint32, copy=False))
            n, on_device = int(p.shape[0]), 0
            pts.positions = p.ctypes.data
        keep.append(p)
        pts.n = n
        for name, words in (("albedo", albedo), ("data", data)):
            fill = "fill" if name == "albedo" else "fill_data"
            if words is None or isinstance(words, (int, np.integer)):
                setattr(pts, fill, int(words or 0))
                continue
            if hasattr(words, "data_ptr") != bool(on_device):
                raise TypeError(f"set_voxels: positions and {name} are both arrays or both device tensors")
            if tuple(words.shape) != (n,):
                raise ValueError(f"set_voxels: {name} has shape {tuple(words.shape)}, the list needs {(n,)}")
            if on_device:
                w = self._device_tensor(words, "set_voxels")
                setattr(pts, name, w.data_ptr())
            else:
                w = np.ascontiguousarray(words, np.uint32)
                setattr(pts, name, w.ctypes.data)
            keep.append(w)
        self._check(N.lib().vhx_set_voxels(self._h, ctypes.byref(pts), on_device))
        del keep

    def update_voxels(self, positions, albedo=None, data=None):
        """set_voxels(..., "update"): the listed voxels recoloured (`albedo`) and / or retagged (`data`), the half that
        is not given -- None, 0, or a 0 in an array -- kept as it is. update_voxels(pos, data=7) gives the voxels the
        data value 7 and keeps their colours; an empty voxel among them becomes a data-only voxel."""
        self.set_voxels(positions, albedo, data, "update")

    def clear_voxels(self, positions):
        """vhx_set_voxels without values: every listed voxel is cleared (the batched BoxTree.clear)."""
        self.set_voxels(positions, 0, 0, "replace")

    def _list_query(self, origin, extents):
        from .boxtree import _list_box
        size = self.tree_counts().boxtree_size if extents is None else 0
        q = N.PointsOut(*_list_box(size, origin, extents))
        n = ctypes.c_uint64()
        q.count = ctypes.pointer(n)
        return q, n

    def count_voxels(self, origin=(0, 0, 0), extents=None):
        """vhx_list_voxels with capacity 0: the number of voxels of the box at `origin` (x, y, z) with `extents` (gx, gy,
        gz; None = the whole root cube) that list_voxels would list."""
        q, n = self._list_query(origin, extents)
        self._check(N.lib().vhx_list_voxels(self._h, ctypes.byref(q), 0))
        return n.value

    def list_voxels(self, origin=(0, 0, 0), extents=None, capacity=None, device=False):
        """vhx_list_voxels: the occupied voxels of the box at `origin` (x, y, z) with `extents` (gx, gy, gz; None = the
        whole root cube) as (positions (n, 3), albedo (n,), data (n,)) -- the sparse form of read_dense(data=True) and
        the inverse of set_voxels. A voxel is listed when read_dense(data=True) gives it a colour or a data value, with
        those two words; the order is positional (sectant digits from the root down, then the flat cell index:
        include/vhx.h), so it does not depend on how the tree is structured. device=False gives uint32 numpy arrays,
        device=True int32 torch tensors on this context's device, complete when the call returns. capacity=None sizes
        the arrays from a count-only call first; with an explicit capacity the first min(count, capacity) entries come
        back, and count as a fourth item. Allowed on shared contexts; cost and scratch follow the nodes and bricks under
        the box, not its volume."""
        q, n = self._list_query(origin, extents)
        if capacity is None:
            self._check(N.lib().vhx_list_voxels(self._h, ctypes.byref(q), 0))
            cap = n.value
        else:
            cap = int(capacity)
            if cap < 0:
                raise ValueError("list_voxels: capacity is unsigned")
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            pos = torch.empty((cap, 3), dtype=torch.int32, device=dev)
            alb = torch.empty(cap, dtype=torch.int32, device=dev)
            dat = torch.empty(cap, dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            q.positions, q.albedo, q.data = pos.data_ptr(), alb.data_ptr(), dat.data_ptr()
        else:
            pos, alb, dat = np.empty((cap, 3), np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.uint32)
            q.positions, q.albedo, q.data = pos.ctypes.data, alb.ctypes.data, dat.ctypes.data
        q.capacity = cap
        if cap or capacity is not None:
            self._check(N.lib().vhx_list_voxels(self._h, ctypes.byref(q), 1 if device else 0))
        k = min(n.value, cap)
        if capacity is None:
            return pos[:k], alb[:k], dat[:k]
        return pos[:k], alb[:k], dat[:k], n.value

    def orphans(self):
        """vhx_tree_orphans: (nodes, bricks) that write_dense / fill_box unlinked since the last upload or build; their
        slots are not reused (compact() drops them)."""
        n, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(N.lib().vhx_tree_orphans(self._h, ctypes.byref(n), ctypes.byref(b)))
        return n.value, b.value

    def compact(self):
        """vhx_compact_tree: rewrites the resident tree on the device without its unreachable node and brick slots and
        in the builders' numbering (download() then equals download().compacted() of before, bit for bit); every get,
        read_dense and trace result stays as it was, the buffers shrink (device_bytes) and orphans() is (0, 0). Returns
        (nodes_dropped, bricks_dropped). Out of place: the peak device memory is the old tree plus the new one. Owner
        context only, not while node MIPs are set, and not under a streamed view (its host cache keeps slot numbers);
        a refused call leaves the tree as it was."""
        n, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(N.lib().vhx_compact_tree(self._h, ctypes.byref(n), ctypes.byref(b)))
        if not isinstance(self._tree, _BuiltOnDevice):
            self._tree = _BuiltOnDevice()  # no longer the uploaded FlatTree: upload() of it must upload again
        return n.value, b.value

    def simplify(self):
        """vhx_simplify_tree: simplifies the resident tree on the device as BoxTree.simplify(recursive=True) does on the
        host, and compacts it in the same pass (download() then equals download().simplified() of before, bit for bit):
        bricks of one value become Solid or empty, leaves of one Solid brick or of homogeneous 4x4x4 blocks become
        UniformLeaf nodes, orphans leave, solid_values are renumbered by first use; cells keep their data values and the
        palettes stay. After write_dense / fill_box edits it leaves the tree build_dense(simplify=True) gives for the same
        voxels. read_dense is unchanged; traces are those of the new image. Returns (nodes_dropped, bricks_dropped), the
        old counts minus the new. Contract as compact(): out of place, owner context only, not while node MIPs are set,
        not under a streamed view; a refused call leaves the tree as it was. VHX_E_CAPACITY (tree unchanged) past 65,535
        distinct Solid values. Against read_dense + build_dense(simplify=True), the only other way back to a simplified
        tree, it needs no dense grid on the host or device, keeps data values and palette order and shrinks the buffers;
        DESIGN.md §8.9 says how the two compare in time. The palettes keep their dead entries and their edit order, so
        the image is the build's only up to the order of the palettes; compact_palettes() after it closes that caveat
        for color_palette and data_palette alike (compact_palette() for the colours alone)."""
        n, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(N.lib().vhx_simplify_tree(self._h, ctypes.byref(n), ctypes.byref(b)))
        if not isinstance(self._tree, _BuiltOnDevice):
            self._tree = _BuiltOnDevice()  # no longer the uploaded FlatTree: upload() of it must upload again
        return n.value, b.value

    def compact_palette(self):
        """vhx_compact_palette: rewrites the colour half of the resident tree on the device, in place, so that
        color_palette is the builders' palette of the voxels the tree holds now (download() then equals
        download().palette_compacted() of before, bit for bit): colours no reachable voxel names leave, entries of one
        colour merge, the rest is in first-appearance order of the builders' insert loop, and every cell and solid value
        is translated. After edits, simplify() then compact_palette() leaves exactly the image build_dense(simplify=True)
        gives for the same voxels, compact() then compact_palette() that of a plain build_dense; and a palette filled up
        by a long editing session (VHX_E_CAPACITY from write_dense) has room again. read_dense and every trace field but
        `value` are unchanged; `value` (trace, get) is the old one with its colour index translated. Returns the colours
        dropped. Buffers are not reallocated. Owner context only, not while node MIPs are set, not under a streamed view
        (its host cache keeps palette indices); a refused call leaves the tree as it was. DESIGN.md §8.10."""
        n = ctypes.c_uint32()
        self._check(N.lib().vhx_compact_palette(self._h, ctypes.byref(n)))
        if not isinstance(self._tree, _BuiltOnDevice):
            self._tree = _BuiltOnDevice()  # no longer the uploaded FlatTree: upload() of it must upload again
        return n.value

    def compact_palettes(self, color=True, data=True):
        """vhx_compact_palettes: compact_palette() for the selected halves, in one walk and one pass over the voxel
        buffer. With data=True data_palette too becomes the builders' palette of the voxels the tree holds now: data
        values no reachable voxel names leave, entries of one value merge, the rest is in first-appearance order of the
        builders' insert loop, and the data half of every cell and solid value is translated (download() then equals
        download().palettes_compacted(color, data) of before, bit for bit). After write_dense(data=), fill_box and
        set_voxels edits, simplify() then compact_palettes() leaves exactly the image build_dense(data=, simplify=True)
        gives for the same voxels, in all seven arrays, and compact() then compact_palettes() that of the plain build; a
        data_palette filled up with ids no voxel holds any more (VHX_E_CAPACITY from the write calls) has room again.
        color=True, data=False is compact_palette(). Returns (colors_dropped, data_dropped), 0 for a half that is not
        selected. read_dense(data=True) is unchanged; contract and refusals as compact_palette(). DESIGN.md §8.14."""
        from .boxtree import _palettes_mask
        nc, nd = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(N.lib().vhx_compact_palettes(self._h, _palettes_mask(color, data), ctypes.byref(nc),
                                                 ctypes.byref(nd)))
        if not isinstance(self._tree, _BuiltOnDevice):
            self._tree = _BuiltOnDevice()  # no longer the uploaded FlatTree: upload() of it must upload again
        return nc.value, nd.value

    def update_range(self, buffer_id, elem_offset, values):
        values = np.ascontiguousarray(values)
        self._check(N.lib().vhx_update_range(self._h, buffer_id, elem_offset, values.size, values.ctypes.data))

    def update_ranges(self, writes):
        """vhx_update_ranges: writes = [(buffer_id, elem_offset, values), ...] in one staged copy + scatter."""
        keep = [np.ascontiguousarray(v) for _, _, v in writes]
        rs = (N.Range * max(1, len(writes)))()
        for r, (bid, off, _), v in zip(rs, writes, keep):
            r.buffer_id, r.elem_offset, r.elem_count, r.src = bid, off, v.size, v.ctypes.data
        self._check(N.lib().vhx_update_ranges(self._h, ctypes.cast(rs, ctypes.c_void_p), len(writes)))

    def read_derived(self, which, offset, count):
        dt = np.uint32 if which == N.VHX_DERIVED_NODE_HDR else np.uint64
        k = 4 if which == N.VHX_DERIVED_NODE_HDR else 1
        a = np.empty(count * k, dt)
        self._check(N.lib().vhx_read_derived(self._h, which, offset, count, a.ctypes.data))
        return a.reshape(count, k) if k > 1 else a

    def device_bytes(self):
        b = ctypes.c_uint64()
        self._check(N.lib().vhx_tree_device_bytes(self._h, ctypes.byref(b)))
        return b.value

    def set_stream(self, stream_ptr):
        self._check(N.lib().vhx_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def stream(self):
        """The context's hipStream_t (vhx_get_stream): the one set by set_stream, else its own (created now if
        needed); wrap it with torch.cuda.ExternalStream to order torch work and events with the traces."""
        s = ctypes.c_void_p()
        self._check(N.lib().vhx_get_stream(self._h, ctypes.byref(s)))
        return s.value

    def set_node_mips(self, node_mips):
        """vhx_set_node_mips: node MIPs stand in for occupied but absent children (the WGSL path's probe_MIP);
        None disables them. `node_mips` is FlatTree.node_mips of the uploaded tree."""
        if node_mips is None:
            self._check(N.lib().vhx_set_node_mips(self._h, None, 0))
            self._mips = None
            return
        self._mips = np.ascontiguousarray(node_mips, np.uint32)
        self._check(N.lib().vhx_set_node_mips(self._h, self._mips.ctypes.data, len(self._mips)))

    def node_mips(self):
        """vhx_read_node_mips: the node MIP descriptors in force (set_node_mips, build_lod), one per node, as a uint32
        array read back from the device. VHX_E_STATE when none are set."""
        a = np.empty(self.tree_counts().node_count, np.uint32)
        self._check(N.lib().vhx_read_node_mips(self._h, a.ctypes.data, a.size))
        return a

    def build_lod(self, source, max_depth, method="box"):
        """vhx_build_lod: makes this context's tree the LOD image of `source`'s resident tree with node MIPs, computed
        on the device without leaving it (download() and node_mips() then equal source.download().lod(max_depth,
        method), bit for bit). Every node's albedo MIP brick is resampled bottom-up with `method` ("box": BoxFilter,
        "point": PointFilter) on every level and colour-similarity thresholds of 0, nodes deeper than max_depth (root =
        0) are left out, and the descriptors are set as set_node_mips sets them, so a trace of this context shows a
        parent's MIP where a child was cut. `source` is only read: it stays MIP-free and editable, and the call is made
        again after edits. Returns (nodes, bricks, colors_added). Owner context only; frames in flight on this context's
        tree finish with the old tree. A refused call leaves both contexts as they were: VHX_E_STATE for a source without
        a tree, with node MIPs, or not of canonical depth, and for a shadow light on this context; VHX_E_INVALID_ARG for
        the same tree on both sides or different devices; VHX_E_CAPACITY past 65,535 colours (BoxFilter appends the
        colours it creates; PointFilter creates none). DESIGN.md §8.16."""
        from .boxtree import mip_method_code
        n, b, k = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(N.lib().vhx_build_lod(self._h, source._h, int(max_depth), mip_method_code(method), ctypes.byref(n),
                                          ctypes.byref(b), ctypes.byref(k)))
        self._tree = _BuiltOnDevice()
        self._mips = None  # the descriptors live on the device (node_mips() reads them)
        return n.value, b.value, k.value

    def set_depth_prepass(self, enable=True, margin=0.0):
        """vhx_set_depth_prepass: the opt-in half-resolution depth-prepass fast mode (not the reference's semantics)."""
        self._check(N.lib().vhx_set_depth_prepass(self._h, 1 if enable else 0, float(margin)))

    def set_shadow_light(self, light=None):
        """vhx_set_shadow_light: fused hard shadows (config 5) in trace_primary / trace_primary_batch /
        trace_tiles_batch, whose outputs then need value, impact, normal and shadowed; None turns them off."""
        lt = None if light is None else (ctypes.c_float * 3)(*[float(v) for v in light])
        self._check(N.lib().vhx_set_shadow_light(self._h, lt))

    def set_pass_budgets(self, budgets):
        """Step budgets of the multi-pass ray scheduler (vhx_set_pass_budgets); () = one unbounded pass."""
        b = (ctypes.c_uint32 * max(1, len(budgets)))(*budgets)
        self._check(N.lib().vhx_set_pass_budgets(self._h, b, len(budgets)))

    def set_adaptive_schedule(self, on=True):
        """Restores (or ends) the adaptive choice between the frames-in-flight and the lone-frame schedule."""
        self._check(N.lib().vhx_set_adaptive_schedule(self._h, 1 if on else 0))

    def tail_info(self):
        """vhx_tail_info: (pixels the next lone frame traces early, (width, height) they were recorded for)."""
        n, w, h = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(N.lib().vhx_tail_info(self._h, ctypes.byref(n), ctypes.byref(w), ctypes.byref(h)))
        return n.value, (w.value, h.value)

    def pass_budgets(self):
        """(budgets of the last trace, schedule): schedule "busy" (frames in flight), "idle" (lone frame) or "fixed"."""
        b = (ctypes.c_uint32 * N.VHX_MAX_BUDGETS)()
        n, sched = ctypes.c_uint32(), ctypes.c_int()
        self._check(N.lib().vhx_get_pass_budgets(self._h, b, ctypes.byref(n), ctypes.byref(sched)))
        return tuple(b[:n.value]), {1: "busy", 0: "idle"}.get(sched.value, "fixed")

    def sync(self):
        ms = ctypes.c_float()
        self._check(N.lib().vhx_sync(self._h, ctypes.byref(ms)))
        return ms.value

    def trace_rays(self, origins, directions, fields=("value", "cell", "voxel", "impact", "normal", "depth", "rgba"),
                   count_bytes=False):
        """Traces rays given as (n,3) f32 origins and directions on the host; returns numpy hit arrays."""
        o = np.ascontiguousarray(origins, f32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, f32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), f32)
        fields = tuple(fields) + (("bytes",) if count_bytes else ())
        out = {name: np.empty((n, k) if k > 1 else (n,), dt) for name, dt, k in HIT_FIELDS if name in fields}
        hs = _hits_struct(out)
        self._check(N.lib().vhx_trace_rays(self._h, rays.ctypes.data, n, ctypes.byref(hs), 0))
        return out

    def trace_primary(self, cam, tile_size=0, tile_start=0, tile_stride=1, layout=N.VHX_LAYOUT_FRAMEBUFFER,
                      fields=("value", "cell", "voxel", "impact", "normal", "depth", "rgba"), count_bytes=False,
                      out=None):
        """Traces one frame (or this rank's tiles). With out=dict of device tensors nothing is copied back; with
        out=dict of host arrays (numpy or CPU tensors, reused across frames) the results are copied into them."""
        if layout == N.VHX_LAYOUT_FRAMEBUFFER:
            n = cam.width * cam.height
        else:
            T = tile_size
            ntiles = ((cam.width + T - 1) // T) * ((cam.height + T - 1) // T)
            n = max(0, (ntiles - tile_start + tile_stride - 1) // tile_stride) * T * T
        if out is not None:
            for name, dt, k in HIT_FIELDS:
                a = out.get(name)
                nbytes = None if a is None else (a.numel() * a.element_size() if hasattr(a, "numel") else a.nbytes)
                if nbytes is not None and nbytes < n * k * 4:
                    raise ValueError(f"out[{name!r}] holds {nbytes} bytes, the trace writes {n * k * 4}")
            hs = _hits_struct(out)
            self._check(N.lib().vhx_trace_primary(self._h, ctypes.byref(cam), tile_size, tile_start, tile_stride,
                                                  layout, ctypes.byref(hs), _on_device(out)))
            return out
        fields = tuple(fields) + (("bytes",) if count_bytes else ())
        alloc = np.empty if layout == N.VHX_LAYOUT_FRAMEBUFFER else np.zeros  # tiles past the frame edge stay 0
        res = {name: alloc((n, k) if k > 1 else (n,), dt) for name, dt, k in HIT_FIELDS if name in fields}
        hs = _hits_struct(res)
        self._check(N.lib().vhx_trace_primary(self._h, ctypes.byref(cam), tile_size, tile_start, tile_stride, layout,
                                              ctypes.byref(hs), 0))
        return res

    def trace_primary_batch(self, cams, outs):
        """vhx_trace_primary_batch: whole frames cams[k] -> outs[k] (dicts of device tensors, framebuffer layout) as one
        pass ladder on this context's stream; results equal one trace_primary per frame."""
        if len(cams) != len(outs) or not cams:
            raise ValueError("trace_primary_batch: one output dict per camera")
        n = cams[0].width * cams[0].height
        for out in outs:
            if _on_device(out) != 1:
                raise ValueError("trace_primary_batch writes device tensors")
            for name, dt, k in HIT_FIELDS:
                a = out.get(name)
                if a is not None and a.numel() * a.element_size() < n * k * 4:
                    raise ValueError(f"out[{name!r}] holds {a.numel() * a.element_size()} bytes, a frame needs {n * k * 4}")
        cs = (N.Camera * len(cams))(*cams)
        hs = (N.Hits * len(outs))(*[_hits_struct(o) for o in outs])
        self._check(N.lib().vhx_trace_primary_batch(self._h, ctypes.cast(cs, ctypes.c_void_p), len(cams),
                                                    ctypes.cast(hs, ctypes.c_void_p)))
        return outs

    def trace_tiles_batch(self, cams, tile_size, tile_starts, tile_stride, outs):
        """vhx_trace_tiles_batch: frame k = the tile set tile_starts[k], +tile_stride, ... of cams[k] (tile layout) into
        outs[k] (dicts of device tensors) as one pass ladder; equal to one trace_primary(layout=TILES) per frame."""
        if len(cams) != len(outs) or len(cams) != len(tile_starts) or not cams:
            raise ValueError("trace_tiles_batch: one output dict and one tile start per camera")
        T = tile_size
        if T < 1 or tile_stride < 1:
            raise ValueError("trace_tiles_batch: tile_size and tile_stride must be >= 1")
        ntiles = ((cams[0].width + T - 1) // T) * ((cams[0].height + T - 1) // T)
        for st, out in zip(tile_starts, outs):
            if _on_device(out) != 1:
                raise ValueError("trace_tiles_batch writes device tensors")
            n = max(0, (ntiles - st + tile_stride - 1) // tile_stride) * T * T
            for name, dt, k in HIT_FIELDS:
                a = out.get(name)
                if a is not None and a.numel() * a.element_size() < n * k * 4:
                    raise ValueError(f"out[{name!r}] holds {a.numel() * a.element_size()} bytes, the set needs {n * k * 4}")
        cs = (N.Camera * len(cams))(*cams)
        st = (ctypes.c_uint32 * len(cams))(*[int(v) for v in tile_starts])
        hs = (N.Hits * len(outs))(*[_hits_struct(o) for o in outs])
        self._check(N.lib().vhx_trace_tiles_batch(self._h, ctypes.cast(cs, ctypes.c_void_p), len(cams), T,
                                                  ctypes.cast(st, ctypes.c_void_p), tile_stride,
                                                  ctypes.cast(hs, ctypes.c_void_p)))
        return outs

    def trace_shadows_batch(self, light, hits_list, shadowed_list=None, darken=True):
        """vhx_trace_shadows_batch: the hard shadows of several frames' device-resident hit records (dicts like
        trace_shadows' `hits`, the same record count each) as one pass ladder; returns the int32 `shadowed` tensors.
        Equal to one trace_shadows per frame."""
        import torch
        if not hits_list:
            raise ValueError("trace_shadows_batch: no frames")
        n = hits_list[0]["value"].numel()
        if any(h["value"].numel() != n for h in hits_list):
            raise ValueError("trace_shadows_batch: every frame needs the same record count")
        for h in hits_list:
            if _on_device(h) != 1:
                raise ValueError("trace_shadows_batch reads device tensors")
        if shadowed_list is None:
            shadowed_list = [torch.empty(n, dtype=torch.int32, device=h["value"].device) for h in hits_list]
        if len(shadowed_list) != len(hits_list):
            raise ValueError("trace_shadows_batch: one shadowed tensor per frame")

        def need(a, words, what):
            # the library trusts n for every array of every frame: a short tensor would be read or written past its end
            if a is None or not hasattr(a, "numel") or not a.is_cuda or a.numel() * a.element_size() < 4 * words:
                raise ValueError(f"trace_shadows_batch: {what} must be a device tensor of at least {4 * words} bytes")

        for k, h in enumerate(hits_list):
            need(h["value"], n, f"frame {k} value")
            need(h["impact"], 3 * n, f"frame {k} impact")
            need(h["normal"], 3 * n, f"frame {k} normal")
            need(shadowed_list[k], n, f"frame {k} shadowed")
            if darken and h.get("rgba") is not None:
                need(h["rgba"], n, f"frame {k} rgba")
        fr = (N.ShadowFrame * len(hits_list))()
        for k, h in enumerate(hits_list):
            rgba = h.get("rgba") if darken else None
            fr[k] = N.ShadowFrame(_ptr(h["value"]), _ptr(h["impact"]), _ptr(h["normal"]), _ptr(shadowed_list[k]),
                                  None if rgba is None else _ptr(rgba))
        lt = (ctypes.c_float * 3)(*[float(v) for v in light])
        self._check(N.lib().vhx_trace_shadows_batch(self._h, lt, len(hits_list), n, ctypes.cast(fr, ctypes.c_void_p)))
        return shadowed_list

    def trace_shadows(self, light, hits, shadowed=None, darken=True, count_bytes=False):
        """Hard shadow rays (vhx_trace_shadows) for the device-resident hit records `hits` of a previous trace
        (dict of torch tensors with value, impact, normal and optionally rgba). Returns a dict with the int32
        `shadowed` flags (and `bytes`); hits["rgba"] is darkened in place when darken."""
        import torch
        n = hits["value"].numel()
        if shadowed is None:
            shadowed = torch.empty(n, dtype=torch.int32, device=hits["value"].device)
        res = {"shadowed": shadowed}
        if count_bytes:
            res["bytes"] = torch.empty(n, dtype=torch.int32, device=hits["value"].device)
        lt = (ctypes.c_float * 3)(*[float(v) for v in light])
        rgba = hits.get("rgba") if darken else None
        self._check(N.lib().vhx_trace_shadows(
            self._h, lt, n, ctypes.c_void_p(_ptr(hits["value"])), ctypes.c_void_p(_ptr(hits["impact"])),
            ctypes.c_void_p(_ptr(hits["normal"])), ctypes.c_void_p(_ptr(shadowed)),
            ctypes.c_void_p(None if rgba is None else _ptr(rgba)),
            ctypes.c_void_p(_ptr(res["bytes"]) if count_bytes else None)))
        return res

    def untile_frame(self, gathered_dev_ptr, planes, ranks, tiles_per_rank, tile_size, width, height, rgba_dev_ptr,
                     depth_dev_ptr=None):
        """vhx_untile_frame: rank-major [RGBA plane | depth plane] tile buffers -> device framebuffers."""
        self._check(N.lib().vhx_untile_frame(self._h, ctypes.c_void_p(gathered_dev_ptr), planes, ranks,
                                             tiles_per_rank, tile_size, width, height, ctypes.c_void_p(rgba_dev_ptr),
                                             ctypes.c_void_p(depth_dev_ptr)))

    def untile_rgba(self, gathered_dev_ptr, ranks, tiles_per_rank, tile_size, width, height, fb_dev_ptr):
        self._check(N.lib().vhx_untile_rgba(self._h, ctypes.c_void_p(gathered_dev_ptr), ranks, tiles_per_rank,
                                            tile_size, width, height, ctypes.c_void_p(fb_dev_ptr), 1))


_default = {}


def default_raytracer(device=None):
    dev = 0 if device is None else device
    if dev not in _default:
        _default[dev] = Raytracer(dev)
    return _default[dev]


class BoxTreeGPUHost:
    """BoxTreeGPUHost (src/raytracing/bevy/types.rs:91-103): owns the tree and renders views of it on a GPU."""

    def __init__(self, tree, device=0):
        self.tree = tree
        self.raytracer = Raytracer(device)

    def create_new_view(self, viewport, resolution):
        return BoxTreeGPUView(self, viewport, resolution)


class BoxTreeGPUView:
    """A view (src/raytracing/bevy/types.rs:134-180): viewport + output resolution, rendered to RGBA8."""

    def __init__(self, host, viewport, resolution):
        self.host, self.viewport, self.resolution = host, viewport, tuple(resolution)

    def render(self, fields=("rgba", "depth")):
        flat = self.host.tree.flatten() if hasattr(self.host.tree, "flatten") else self.host.tree
        self.host.raytracer.upload(flat)
        w, h = self.resolution
        res = self.host.raytracer.trace_primary(self.viewport.camera(w, h), fields=fields)
        if "rgba" in res:
            res["image"] = res["rgba"].view(np.uint8).reshape(h, w, 4)
        return res
