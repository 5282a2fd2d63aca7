"""Host-side BoxTree API, mirroring VoxelHex's `voxelhex::boxtree` (src/boxtree/mod.rs, src/boxtree/types.rs).

The tree itself lives in libvhx (C++ restatement of the reference's insert/get/simplify, include/vhx_boxtree.h);
this module keeps the reference's names, argument meaning and error behaviour:

    BoxTree(size, brick_dim)             BoxTree::new            -> raises OctreeError.InvalidSize / ...
    tree.insert(pos, entry)              BoxTree::insert         -> raises OctreeError.InvalidPosition
    tree.insert_at_lod(pos, size, entry) BoxTree::insert_at_lod
    tree.update(pos, entry)              BoxTree::update
    tree.clear(pos)                      BoxTree::clear          -> raises OctreeError.InvalidPosition
    tree.clear_at_lod(pos, size)         BoxTree::clear_at_lod
    tree.get(pos) -> BoxTreeEntry        BoxTree::get
    tree.get_by_ray(ray)                 BoxTree::get_by_ray (src/raytracing/cpu.rs:296), traced on the GPU
"""
from dataclasses import dataclass
import ctypes

import numpy as np

from . import _native as N


class OctreeError(Exception):
    """OctreeError (src/boxtree/types.rs:9-21)."""


class InvalidSize(OctreeError):
    pass


class InvalidBrickDimension(OctreeError):
    pass


class InvalidStructure(OctreeError):
    pass


class InvalidPosition(OctreeError):
    pass


_TREE_ERRORS = {
    N.VHX_E_TREE_INVALID_SIZE: InvalidSize,
    N.VHX_E_TREE_INVALID_BRICK_DIMENSION: InvalidBrickDimension,
    N.VHX_E_TREE_INVALID_STRUCTURE: InvalidStructure,
    N.VHX_E_TREE_INVALID_POSITION: InvalidPosition,
}


def _tree_check(rc, what=""):
    if rc == N.VHX_OK:
        return
    if rc in _TREE_ERRORS:
        raise _TREE_ERRORS[rc](what)
    raise N.VhxError(rc, what)


@dataclass(frozen=True)
class V3c:
    x: float
    y: float
    z: float

    def __iter__(self):
        return iter((self.x, self.y, self.z))


@dataclass(frozen=True)
class Albedo:
    """Albedo (src/boxtree/types.rs:103-109)."""
    r: int = 0
    g: int = 0
    b: int = 0
    a: int = 0

    @staticmethod
    def from_u32(value):
        """impl From<u32> for Albedo (src/boxtree/detail.rs:72-85): 0xRRGGBBAA."""
        value &= 0xFFFFFFFF
        return Albedo((value >> 24) & 0xFF, (value >> 16) & 0xFF, (value >> 8) & 0xFF, value & 0xFF)

    @staticmethod
    def from_packed(p):
        return Albedo(p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF, (p >> 24) & 0xFF)

    def packed(self):
        """r | g<<8 | b<<16 | a<<24, the palette encoding of include/vhx.h."""
        return (self.r & 0xFF) | ((self.g & 0xFF) << 8) | ((self.b & 0xFF) << 16) | ((self.a & 0xFF) << 24)

    def is_transparent(self):
        return self.a == 0


@dataclass(frozen=True)
class BoxTreeEntry:
    """BoxTreeEntry<u32> (src/boxtree/types.rs:25-37): kind in {Empty, Visual, Informative, Complex}."""
    kind: str = "Empty"
    albedo_: Albedo = None
    data_: int = None

    @staticmethod
    def Empty():
        return BoxTreeEntry("Empty")

    @staticmethod
    def Visual(albedo):
        return BoxTreeEntry("Visual", albedo, None)

    @staticmethod
    def Informative(data):
        return BoxTreeEntry("Informative", None, int(data))

    @staticmethod
    def Complex(albedo, data):
        return BoxTreeEntry("Complex", albedo, int(data))

    def albedo(self):
        return self.albedo_ if self.kind in ("Visual", "Complex") else None

    def data(self):
        return self.data_ if self.kind in ("Informative", "Complex") else None

    def is_none(self):
        """BoxTreeEntry::is_none (src/boxtree/mod.rs:99-106)."""
        if self.kind == "Empty":
            return True
        if self.kind == "Visual":
            return self.albedo_.is_transparent()
        if self.kind == "Informative":
            return self.data_ == 0
        return self.albedo_.is_transparent() and self.data_ == 0

    def is_some(self):
        return not self.is_none()


class MIPResamplingMethods:
    """MIPResamplingMethods (src/boxtree/types.rs:113-149) as (code, threshold) pairs for set_method_at."""
    BoxFilter = (0, 0.0)
    PointFilter = (1, 0.0)
    PointFilterBD = (2, 0.0)

    @staticmethod
    def Posterize(thr):
        return (3, float(thr))

    @staticmethod
    def PosterizeBD(thr):
        return (4, float(thr))


class StrategyUpdater:
    """StrategyUpdater (src/boxtree/mipmap.rs:458-668): chainable MIP-map settings of a BoxTree."""

    def __init__(self, tree):
        self._t = tree

    def switch_albedo_mip_maps(self, enabled):
        N.check(N.lib().vhx_boxtree_switch_mips(self._t._h, int(bool(enabled))))
        self._t._version += 1
        return self

    def set_method_at(self, mip_level, method):
        code, thr = method
        N.check(N.lib().vhx_boxtree_set_mip_method(self._t._h, int(mip_level), code, thr))
        return self

    def set_color_similarity_thr_at(self, mip_level, similarity_thr):
        N.check(N.lib().vhx_boxtree_set_mip_color_threshold(self._t._h, int(mip_level), float(similarity_thr)))
        return self

    def recalculate_mips(self):
        N.check(N.lib().vhx_boxtree_recalculate_mips(self._t._h))
        self._t._version += 1
        return self

    def sample_root_mip(self, sectant, position):
        x, y, z = _pos(position)
        k, a, d = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        N.check(N.lib().vhx_boxtree_sample_root_mip(self._t._h, int(sectant), x, y, z, ctypes.byref(k),
                                                    ctypes.byref(a), ctypes.byref(d)))
        return _entry_of(k.value, a.value, d.value)


def _entry_of(kind, albedo, data):
    if kind == N.VHX_ENTRY_EMPTY:
        return BoxTreeEntry.Empty()
    if kind == N.VHX_ENTRY_VISUAL:
        return BoxTreeEntry.Visual(Albedo.from_packed(albedo))
    if kind == N.VHX_ENTRY_INFORMATIVE:
        return BoxTreeEntry.Informative(data)
    return BoxTreeEntry.Complex(Albedo.from_packed(albedo), data)


def voxel_data(data=None):
    """The reference's voxel_data! macro (src/boxtree/mod.rs:65-72)."""
    return BoxTreeEntry.Empty() if data is None else BoxTreeEntry.Informative(data)


def _entry(e):
    """Into<BoxTreeEntry>: Albedo -> Visual, int -> Informative, (Albedo, int) -> Complex."""
    if isinstance(e, BoxTreeEntry):
        return e
    if isinstance(e, Albedo):
        return BoxTreeEntry.Visual(e)
    if isinstance(e, tuple) and len(e) == 2:
        return BoxTreeEntry.Complex(e[0], e[1])
    if isinstance(e, (int, np.integer)):
        return BoxTreeEntry.Informative(int(e))
    raise TypeError(f"cannot convert {e!r} into a BoxTreeEntry")


def _entry_args(e):
    e = _entry(e)
    kinds = {"Empty": N.VHX_ENTRY_EMPTY, "Visual": N.VHX_ENTRY_VISUAL, "Informative": N.VHX_ENTRY_INFORMATIVE,
             "Complex": N.VHX_ENTRY_COMPLEX}
    alb = e.albedo_.packed() if e.albedo_ is not None else 0
    dat = (e.data_ or 0) & 0xFFFFFFFF
    return kinds[e.kind], alb, dat


def entry_from_value(value, color_palette, data_palette):
    """NodeContent::pix_get_ref (src/boxtree/node.rs:335-373) for a PaletteIndexValues."""
    value = int(value)
    ci, di = value & 0xFFFF, (value >> 16) & 0xFFFF
    cn, dn = ci == 0xFFFF, di == 0xFFFF
    if cn and dn:
        return BoxTreeEntry.Empty()
    alb = Albedo.from_packed(int(color_palette[ci])) if not cn and ci < len(color_palette) else None
    dat = int(data_palette[di]) if not dn and di < len(data_palette) else None
    if dn:
        return BoxTreeEntry.Visual(alb)
    if cn:
        return BoxTreeEntry.Informative(dat)
    return BoxTreeEntry.Complex(alb, dat)


def _pos(p):
    x, y, z = (int(v) for v in p)
    if min(x, y, z) < 0:
        raise InvalidPosition(f"{(x, y, z)}")
    return x, y, z


class _OwnedBuffer:
    """Buffer-protocol view of libvhx-owned memory that keeps its owner alive."""

    def __init__(self, owner, ptr, nbytes):
        self._owner = owner
        self._mem = (ctypes.c_char * nbytes).from_address(ptr)

    @property
    def __array_interface__(self):
        return {"shape": (len(self._mem),), "typestr": "|u1", "data": (ctypes.addressof(self._mem), False),
                "version": 3}


TREE_ARRAYS = (("node_type", np.uint32), ("node_ocbits", np.uint64), ("node_children", np.uint32),
               ("voxels", np.uint32), ("solid_values", np.uint32), ("color_palette", np.uint32),
               ("data_palette", np.uint32))  # in VHX_BUF_* order


def _dense_desc(grid, size, brick_dim):
    """(vhx_dense_desc, the array it points into) of a numpy grid of shape (gz, gy, gx), dtype uint32."""
    g = np.asarray(grid)
    if g.ndim != 3 or g.dtype != np.uint32:
        raise TypeError("a dense grid is a uint32 array of shape (gz, gy, gx)")
    g = np.ascontiguousarray(g)
    d = N.DenseDesc()
    d.boxtree_size, d.brick_dim = int(size), int(brick_dim)
    d.gz, d.gy, d.gx = (int(v) for v in g.shape)
    d.albedo = g.ctypes.data
    return d, g


def _dense_data(data, shape):
    """The data plane of a dense grid of `shape`: a C-contiguous uint32 array (0 = no data), or None."""
    if data is None:
        return None
    p = np.asarray(data)
    if p.dtype != np.uint32 or tuple(p.shape) != tuple(shape):
        raise TypeError(f"a data plane is a uint32 array of the grid's shape {tuple(shape)}")
    return np.ascontiguousarray(p)


def _u32_ptr(a):
    return None if a is None else a.ctypes.data


def _compacted(image):
    """vhx_flat_compact of a FlatTree or TreeImage, as a new FlatTree."""
    h = ctypes.c_void_p()
    _tree_check(N.lib().vhx_flat_compact(ctypes.byref(image.desc), ctypes.byref(h)), "compacted: a malformed image")
    return FlatTree(h.value)


def _simplified(image):
    """vhx_flat_simplify of a FlatTree or TreeImage, as a new FlatTree."""
    h = ctypes.c_void_p()
    _tree_check(N.lib().vhx_flat_simplify(ctypes.byref(image.desc), ctypes.byref(h)), "simplified: a malformed image")
    return FlatTree(h.value)


def _palette_compacted(image):
    """vhx_flat_compact_palette of a FlatTree or TreeImage, as a new FlatTree."""
    h = ctypes.c_void_p()
    _tree_check(N.lib().vhx_flat_compact_palette(ctypes.byref(image.desc), ctypes.byref(h)),
                "palette_compacted: a malformed image")
    return FlatTree(h.value)


def _palettes_mask(color, data):
    """The `which` mask of the palette calls; at least one half must be selected."""
    which = (N.VHX_PALETTE_COLOR if color else 0) | (N.VHX_PALETTE_DATA if data else 0)
    if which == 0:
        raise ValueError("compact_palettes: select the colour half, the data half or both")
    return which


def _palettes_compacted(image, color, data):
    """vhx_flat_compact_palettes of a FlatTree or TreeImage, as a new FlatTree."""
    h = ctypes.c_void_p()
    _tree_check(N.lib().vhx_flat_compact_palettes(ctypes.byref(image.desc), _palettes_mask(color, data),
                                                  ctypes.byref(h)), "palettes_compacted: a malformed image")
    return FlatTree(h.value)


def mip_method_code(method):
    """VHX_MIP_BOX_FILTER / VHX_MIP_POINT_FILTER of "box" / "point", a MIPResamplingMethods pair or the code itself."""
    if isinstance(method, str):
        try:
            return {"box": N.VHX_MIP_BOX_FILTER, "point": N.VHX_MIP_POINT_FILTER}[method]
        except KeyError:
            raise ValueError(f"lod: the method is 'box' or 'point', not {method!r}") from None
    return int(method[0] if isinstance(method, tuple) else method)


def _lod(image, max_depth, method):
    """vhx_flat_lod of a FlatTree or TreeImage, as a new FlatTree with its node_mips."""
    h = ctypes.c_void_p()
    _tree_check(N.lib().vhx_flat_lod(ctypes.byref(image.desc), int(max_depth), mip_method_code(method),
                                     ctypes.byref(h)), "lod: a malformed image, or more than 65,535 colours")
    return FlatTree(h.value)


_LOD_DOC = """vhx_flat_lod: the LOD image of this image with node MIPs, as a FlatTree whose node_mips holds the
        descriptors -- what Raytracer.build_lod(source, max_depth, method) gives the destination on the device, bit for
        bit. `method` is "box" (BoxFilter) or "point" (PointFilter), applied on every level with every colour-similarity
        threshold at 0; the MIPs are those BoxTree's switch_albedo_mip_maps(True) computes under that strategy, their
        new colours appended to color_palette, and nodes deeper than max_depth (root = 0) are left out as
        BoxTree.flatten_lod leaves them out. InvalidStructure for a malformed image and for one the host tree refuses
        (a palette with duplicate entries); VhxError(VHX_E_CAPACITY) past 65,535 colours."""


def _list_box(size, origin, extents):
    """(ox, oy, oz, gx, gy, gz) of a list / count call; extents None = the whole root cube."""
    ox, oy, oz = (int(v) for v in origin)
    gx, gy, gz = (int(size),) * 3 if extents is None else (int(v) for v in extents)
    if min(ox, oy, oz, gx, gy, gz) < 0:
        raise ValueError("list_voxels: origin and extents are unsigned")
    return ox, oy, oz, gx, gy, gz


def _list_voxels(image, origin, extents, capacity):
    """vhx_flat_list_voxels of a FlatTree or TreeImage."""
    q = N.PointsOut(*_list_box(image.boxtree_size, origin, extents))
    n = ctypes.c_uint64()
    q.count = ctypes.pointer(n)
    if capacity is None:  # size the arrays from a count-only call
        _tree_check(N.lib().vhx_flat_list_voxels(ctypes.byref(image.desc), ctypes.byref(q)), "list_voxels")
        cap = n.value
    else:
        cap = int(capacity)
        if cap < 0:
            raise ValueError("list_voxels: capacity is unsigned")
    pos, alb, dat = np.empty((cap, 3), np.uint32), np.empty(cap, np.uint32), np.empty(cap, np.uint32)
    q.capacity, q.positions, q.albedo, q.data = cap, pos.ctypes.data, alb.ctypes.data, dat.ctypes.data
    _tree_check(N.lib().vhx_flat_list_voxels(ctypes.byref(image.desc), ctypes.byref(q)), "list_voxels")
    k = min(n.value, cap)
    if capacity is None:
        return pos[:k], alb[:k], dat[:k]
    return pos[:k], alb[:k], dat[:k], n.value


_LIST_DOC = """vhx_flat_list_voxels: the occupied voxels of the box at `origin` (x, y, z) with `extents` (gx, gy, gz; None =
        the whole root cube) as (positions (n, 3), albedo (n,), data (n,)), uint32 arrays -- what Raytracer.list_voxels
        gives for this image on the device, bit for bit. A voxel is listed when read_dense(data=True) gives it a colour or
        a data value, in the positional order include/vhx.h states. capacity=None sizes the arrays from a count-only
        call; with an explicit capacity the first min(count, capacity) entries come back, and count as a fourth item."""


class TreeImage:
    """A flattened tree held in numpy arrays (Raytracer.download): the seven arrays and counts of a vhx_tree_desc,
    under FlatTree's names; `desc` points into them, so the image uploads, traces on the oracle and saves like one."""

    def list_voxels(self, origin=(0, 0, 0), extents=None, capacity=None):
        return _list_voxels(self, origin, extents, capacity)

    list_voxels.__doc__ = _LIST_DOC

    def count_voxels(self, origin=(0, 0, 0), extents=None):
        """The number of voxels list_voxels lists for the box (a count-only call)."""
        return _list_voxels(self, origin, extents, 0)[3]

    def palette_compacted(self):
        """vhx_flat_compact_palette: this image with the colour palette the builders give the voxels it holds now, as a
        FlatTree -- what Raytracer.compact_palette leaves on the device, bit for bit. Colours no reachable value names
        leave, entries of one colour merge, the rest is ordered by first appearance in the builders' insert loop (x
        outer, y, z inner); the colour half of every cell (orphaned slots included) and solid value is translated, and
        nothing else changes (include/vhx_boxtree.h states every rule). InvalidStructure for a malformed image."""
        return _palette_compacted(self)

    def palettes_compacted(self, color=True, data=True):
        """vhx_flat_compact_palettes: palette_compacted for the selected halves -- with data=True data_palette too
        becomes the builders' palette of the voxels the image holds now (values no reachable value names leave, equal
        entries merge, the rest in first-appearance order) and the data half of every cell and solid value is
        translated; a half that is not selected and its palette stay. What Raytracer.compact_palettes leaves on the
        device, bit for bit; color=True, data=False is palette_compacted()."""
        return _palettes_compacted(self, color, data)

    def lod(self, max_depth, method="box"):
        return _lod(self, max_depth, method)

    lod.__doc__ = _LOD_DOC

    def compacted(self):
        """vhx_flat_compact: this image without its unreachable node and brick slots, renumbered as the builders number
        (nodes breadth-first, bricks in (node, sectant) order), as a FlatTree -- what Raytracer.compact leaves on the
        device, bit for bit. Cells, solid values and palettes are unchanged. InvalidStructure for a malformed image (an
        index past its count, a node or brick reached twice, more than 8 levels)."""
        return _compacted(self)

    def simplified(self):
        """vhx_flat_simplify: compacted(), then the image BoxTree.simplify(recursive=True) leaves of it, as a FlatTree --
        what Raytracer.simplify leaves on the device, bit for bit. Bricks of one value become Solid (or empty where the
        value points to empty), leaves of one Solid brick or of homogeneous 4x4x4 blocks become UniformLeaf nodes, an
        Internal node without occupied bits becomes Nothing; solid_values are renumbered by first use, cells keep their
        words and the palettes stay (include/vhx_boxtree.h states every rule). InvalidStructure for a malformed image
        and for one the host tree refuses (a palette with duplicate entries)."""
        return _simplified(self)

    def __init__(self, boxtree_size, brick_dim, arrays):
        self.desc = N.TreeDesc()
        self.desc.boxtree_size, self.desc.brick_dim = boxtree_size, brick_dim
        for name, dt in TREE_ARRAYS:
            a = np.ascontiguousarray(arrays[name], dt)
            setattr(self, name, a)
            setattr(self.desc, name, a.ctypes.data if a.size else None)
        self.node_mips = np.zeros(0, np.uint32)
        self.desc.node_count = self.node_type.size
        self.desc.brick_count = self.voxels.size // brick_dim ** 3
        self.desc.solid_count = self.solid_values.size
        self.desc.color_count = self.color_palette.size
        self.desc.data_count = self.data_palette.size

    @property
    def boxtree_size(self):
        return self.desc.boxtree_size

    @property
    def brick_dim(self):
        return self.desc.brick_dim

    def counts(self):
        d = self.desc
        return dict(boxtree_size=d.boxtree_size, brick_dim=d.brick_dim, node_count=d.node_count,
                    brick_count=d.brick_count, solid_count=d.solid_count, color_count=d.color_count,
                    data_count=d.data_count)


class FlatTree:
    """Flattened tree (vhx_tree_desc) owned by libvhx; arrays are zero-copy numpy views."""

    def __init__(self, handle):
        self._h = ctypes.c_void_p(handle)
        self.desc = N.TreeDesc()
        N.check(N.lib().vhx_flat_desc(self._h, ctypes.byref(self.desc)))
        d = self.desc
        n3 = d.brick_dim ** 3

        def arr(ptr, n, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dt)
            # a view whose base chain holds this FlatTree, so the buffers outlive any temporary owner
            return np.asarray(_OwnedBuffer(self, ptr, n * np.dtype(dt).itemsize)).view(dt)

        self.node_type = arr(d.node_type, d.node_count, np.uint32)
        self.node_ocbits = arr(d.node_ocbits, d.node_count, np.uint64)
        self.node_children = arr(d.node_children, d.node_count * 64, np.uint32)
        self.voxels = arr(d.voxels, d.brick_count * n3, np.uint32)
        self.solid_values = arr(d.solid_values, d.solid_count, np.uint32)
        self.color_palette = arr(d.color_palette, d.color_count, np.uint32)
        self.data_palette = arr(d.data_palette, d.data_count, np.uint32)
        mp, mc = ctypes.c_void_p(), ctypes.c_uint32()
        N.check(N.lib().vhx_flat_node_mips(self._h, ctypes.byref(mp), ctypes.byref(mc)))
        # per node: its MIP brick descriptor (empty unless the tree was flattened with MIPs)
        self.node_mips = arr(mp.value, mc.value, np.uint32)

    @property
    def boxtree_size(self):
        return self.desc.boxtree_size

    @property
    def brick_dim(self):
        return self.desc.brick_dim

    def nbytes(self):
        return sum(a.nbytes for a in (self.node_type, self.node_ocbits, self.node_children, self.voxels,
                                      self.solid_values, self.color_palette, self.data_palette))

    def compacted(self):
        """vhx_flat_compact (see TreeImage.compacted): a freshly built image comes back equal to itself."""
        return _compacted(self)

    def simplified(self):
        """vhx_flat_simplify (see TreeImage.simplified): from_dense(grid, ...).simplified() is
        from_dense(grid, ..., simplify=True)."""
        return _simplified(self)

    def palette_compacted(self):
        """vhx_flat_compact_palette (see TreeImage.palette_compacted): a freshly built image, plain or simplified, comes
        back equal to itself."""
        return _palette_compacted(self)

    def palettes_compacted(self, color=True, data=True):
        """vhx_flat_compact_palettes (see TreeImage.palettes_compacted): a freshly built image with data, plain or
        simplified, comes back as it is."""
        return _palettes_compacted(self, color, data)

    def list_voxels(self, origin=(0, 0, 0), extents=None, capacity=None):
        return _list_voxels(self, origin, extents, capacity)

    list_voxels.__doc__ = _LIST_DOC

    def count_voxels(self, origin=(0, 0, 0), extents=None):
        """The number of voxels list_voxels lists for the box (a count-only call)."""
        return _list_voxels(self, origin, extents, 0)[3]

    def lod(self, max_depth, method="box"):
        return _lod(self, max_depth, method)

    lod.__doc__ = _LOD_DOC

    @classmethod
    def _from_handle(cls, h):
        t = cls.__new__(cls)
        t._h = h
        t._version = 0
        t._flat = None
        t._flat_version = -1
        return t

    @classmethod
    def from_scene(cls, scene, size, brick_dim, seed=0x5EED, threads=0):
        """The tree insert_scene builds, from the bulk builder's image (vhx_scene_build_tree: seconds at 1024^3 where the
        insert loop takes minutes); occlusion bits and MIP maps are not restored (include/vhx_boxtree.h)."""
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_scene_build_tree(scene, size, brick_dim, seed, threads, ctypes.byref(h)),
                    f"scene {scene} size {size} brick_dim {brick_dim}")
        return cls._from_handle(h)

    @classmethod
    def load_vox_file(cls, filename, brick_dimension):
        """BoxTree::load_vox_file (src/convert/magicavoxel.rs:234-265): MagicaVoxel .vox import (C++,
        voxelhex_amd/csrc/vox.cpp). Raises VhxError for unreadable / unsupported files, InvalidPosition for voxels
        outside the tree (the reference panics)."""
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_boxtree_load_vox(str(filename).encode(), brick_dimension, ctypes.byref(h)),
                    f"{filename}")
        return cls._from_handle(h)

    @classmethod
    def load_vox_bytes(cls, data, brick_dimension):
        """load_vox_file over an in-memory .vox image."""
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(bytes(data))
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_boxtree_load_vox_memory(buf, len(data), brick_dimension, ctypes.byref(h)),
                    "vox bytes")
        return cls._from_handle(h)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            N.lib().vhx_flat_free(self._h)
            self._h = ctypes.c_void_p(None)

    @staticmethod
    def build_scene(scene, size, brick_dim, seed=0x5EED, threads=0):
        """Bulk-builds the canonical tree that inserting `scene` voxel by voxel would produce."""
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_scene_build(scene, size, brick_dim, seed, threads, ctypes.byref(h)),
                    f"scene {scene} size {size} brick_dim {brick_dim}")
        return FlatTree(h.value)

    @staticmethod
    def from_dense(grid, size, brick_dim, threads=0, simplify=False, data=None):
        """Bulk-builds the canonical tree of a dense grid (vhx_dense_build): `grid` is a uint32 numpy array of shape
        (gz, gy, gx) of packed albedos r | g<<8 | b<<16 | a<<24 (alpha 0 = no voxel) sitting at the tree's origin. The
        image equals inserting every voxel (x outer, y, z inner) into BoxTree(size, brick_dim) and flattening; with
        simplify=True, simplifying the tree recursively before flattening (vhx_dense_build_simplified).
        `data` (optional) is a uint32 array of the same shape with a user data value per voxel, 0 = none
        (vhx_dense_build_data): a voxel with a colour and a data value is a Complex entry, one with a data value and
        alpha 0 an Informative entry, and data_palette lists the values in first-appearance order of the insert loop."""
        d, keep = _dense_desc(grid, size, brick_dim)
        plane = _dense_data(data, keep.shape)
        h = ctypes.c_void_p()
        what = f"dense grid {keep.shape[::-1]} size {size} brick_dim {brick_dim}"
        if plane is not None:
            _tree_check(N.lib().vhx_dense_build_data(ctypes.byref(d), _u32_ptr(plane), 1 if simplify else 0, threads,
                                                     ctypes.byref(h)), what)
            return FlatTree(h.value)
        build = N.lib().vhx_dense_build_simplified if simplify else N.lib().vhx_dense_build
        _tree_check(build(ctypes.byref(d), threads, ctypes.byref(h)), what)
        return FlatTree(h.value)

    def counts(self):
        d = self.desc
        return dict(boxtree_size=d.boxtree_size, brick_dim=d.brick_dim, node_count=d.node_count,
                    brick_count=d.brick_count, solid_count=d.solid_count, color_count=d.color_count,
                    data_count=d.data_count)

    @staticmethod
    def build_scene_lod(scene, size, brick_dim, max_depth, seed=0x5EED, threads=0):
        """build_scene with the default MIP maps switched on and flattened like BoxTree.flatten_lod(max_depth): the
        image the insert loop + switch_albedo_mip_maps(True) + flatten_lod would give, without the insert loop."""
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_scene_build_lod(scene, size, brick_dim, seed, threads, int(max_depth), ctypes.byref(h)),
                    f"scene {scene} size {size} brick_dim {brick_dim}")
        return FlatTree(h.value)


class BoxTree:
    """BoxTree<u32> (src/boxtree/types.rs:219-255) backed by libvhx."""

    ROOT_NODE_KEY = 0

    def __init__(self, size, brick_dimension):
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_boxtree_new(size, brick_dimension, ctypes.byref(h)),
                    f"size {size} brick_dim {brick_dimension}")
        self._h = h
        self._version = 0
        self._flat = None
        self._flat_version = -1

    @classmethod
    def _from_handle(cls, h):
        t = cls.__new__(cls)
        t._h = h
        t._version = 0
        t._flat = None
        t._flat_version = -1
        return t

    @classmethod
    def from_scene(cls, scene, size, brick_dim, seed=0x5EED, threads=0):
        """The tree insert_scene builds, from the bulk builder's image (vhx_scene_build_tree: seconds at 1024^3 where the
        insert loop takes minutes); occlusion bits and MIP maps are not restored (include/vhx_boxtree.h)."""
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_scene_build_tree(scene, size, brick_dim, seed, threads, ctypes.byref(h)),
                    f"scene {scene} size {size} brick_dim {brick_dim}")
        return cls._from_handle(h)

    @classmethod
    def from_dense(cls, grid, size, brick_dim, threads=0, data=None):
        """The tree that inserting every voxel of a dense grid (FlatTree.from_dense) builds, from the bulk builder's
        image (vhx_dense_build_tree; with a `data` plane vhx_dense_build_tree_data); occlusion bits and MIP maps are not
        restored, as for from_scene."""
        d, keep = _dense_desc(grid, size, brick_dim)
        plane = _dense_data(data, keep.shape)
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_dense_build_tree_data(ctypes.byref(d), _u32_ptr(plane), threads, ctypes.byref(h)),
                    f"dense grid {keep.shape[::-1]} size {size} brick_dim {brick_dim}")
        return cls._from_handle(h)

    @classmethod
    def load_vox_file(cls, filename, brick_dimension):
        """BoxTree::load_vox_file (src/convert/magicavoxel.rs:234-265): MagicaVoxel .vox import (C++,
        voxelhex_amd/csrc/vox.cpp). Raises VhxError for unreadable / unsupported files, InvalidPosition for voxels
        outside the tree (the reference panics)."""
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_boxtree_load_vox(str(filename).encode(), brick_dimension, ctypes.byref(h)),
                    f"{filename}")
        return cls._from_handle(h)

    @classmethod
    def load_vox_bytes(cls, data, brick_dimension):
        """load_vox_file over an in-memory .vox image."""
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(bytes(data))
        h = ctypes.c_void_p()
        _tree_check(N.lib().vhx_boxtree_load_vox_memory(buf, len(data), brick_dimension, ctypes.byref(h)),
                    "vox bytes")
        return cls._from_handle(h)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            N.lib().vhx_boxtree_free(self._h)
            self._h = ctypes.c_void_p(None)

    # -- reference API -------------------------------------------------------------------------------------------
    @property
    def auto_simplify(self):
        return self._auto_simplify if hasattr(self, "_auto_simplify") else True

    @auto_simplify.setter
    def auto_simplify(self, v):
        self._auto_simplify = bool(v)
        N.check(N.lib().vhx_boxtree_set_auto_simplify(self._h, int(bool(v))))

    def insert(self, position, data):
        x, y, z = _pos(position)
        _tree_check(N.lib().vhx_boxtree_insert(self._h, x, y, z, *_entry_args(data)), f"{(x, y, z)}")
        self._version += 1

    def insert_at_lod(self, position, insert_size, data):
        x, y, z = _pos(position)
        _tree_check(N.lib().vhx_boxtree_insert_at_lod(self._h, x, y, z, insert_size, *_entry_args(data)),
                    f"{(x, y, z)}")
        self._version += 1

    def update(self, position, data):
        x, y, z = _pos(position)
        _tree_check(N.lib().vhx_boxtree_update(self._h, x, y, z, *_entry_args(data)), f"{(x, y, z)}")
        self._version += 1

    def clear(self, position):
        """BoxTree::clear (src/boxtree/update/clear.rs:16-18)."""
        x, y, z = _pos(position)
        _tree_check(N.lib().vhx_boxtree_clear(self._h, x, y, z), f"{(x, y, z)}")
        self._version += 1

    def clear_at_lod(self, position, clear_size):
        """BoxTree::clear_at_lod (src/boxtree/update/clear.rs:23-338): removes the cube of edge `clear_size` at
        `position`."""
        x, y, z = _pos(position)
        _tree_check(N.lib().vhx_boxtree_clear_at_lod(self._h, x, y, z, int(clear_size)), f"{(x, y, z)}")
        self._version += 1

    def get(self, position):
        x, y, z = _pos(position)
        k, a, d = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        N.check(N.lib().vhx_boxtree_get(self._h, x, y, z, ctypes.byref(k), ctypes.byref(a), ctypes.byref(d)))
        return _entry_of(k.value, a.value, d.value)

    def albedo_mip_map_resampling_strategy(self):
        """BoxTree::albedo_mip_map_resampling_strategy (src/boxtree/mod.rs:241-243)."""
        return StrategyUpdater(self)

    def simplify(self, recursive=True):
        N.check(N.lib().vhx_boxtree_simplify(self._h, int(recursive)))
        self._version += 1

    def node_info(self, position):
        """The deepest node containing `position` (get_node_internal): key, content, occupied and occlusion bits."""
        key, content, occ, occl = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
        _tree_check(N.lib().vhx_boxtree_node_info(self._h, *[float(v) for v in position], ctypes.byref(key),
                                                  ctypes.byref(content), ctypes.byref(occ), ctypes.byref(occl)),
                    f"{position}")
        return {"key": key.value, "content": ("Nothing", "Internal", "Leaf", "UniformLeaf")[content.value],
                "occupied_bits": occ.value, "occlusion_bits": occl.value}

    def info(self):
        a = (ctypes.c_uint32 * 5)()
        N.check(N.lib().vhx_boxtree_info(self._h, ctypes.byref(a)))
        return dict(size=a[0], brick_dim=a[1], nodes=a[2], colors=a[3], data=a[4])

    def get_size(self):
        return self.info()["size"]

    def insert_scene(self, scene, seed=0x5EED):
        """Runs the reference insert loop of a procedural scene (vhx_scene_insert)."""
        N.check(N.lib().vhx_scene_insert(self._h, scene, seed))
        self._version += 1

    # -- flattening ------------------------------------------------------------------------------------------------
    def flatten(self):
        """Full-residency flattened image of the tree (cached until the tree changes)."""
        if self._flat is None or self._flat_version != self._version:
            h = ctypes.c_void_p()
            N.check(N.lib().vhx_boxtree_flatten(self._h, ctypes.byref(h)))
            self._flat = FlatTree(h.value)
            self._flat_version = self._version
        return self._flat

    def flatten_lod(self, max_depth):
        """Flattened image with node MIPs and only the nodes down to `max_depth` (root = 0): the deeper nodes are left
        out, their parents' MIPs stand in for them in a MIP-enabled trace (vhx_boxtree_flatten_lod)."""
        h = ctypes.c_void_p()
        N.check(N.lib().vhx_boxtree_flatten_lod(self._h, int(max_depth), ctypes.byref(h)))
        return FlatTree(h.value)

    # -- raytracing (src/raytracing/cpu.rs:296) ----------------------------------------------------------------
    def get_by_ray(self, ray, device=None):
        """Closest hit of `ray`: (BoxTreeEntry, impact_point, impact_normal) or None. Runs on the GPU."""
        from .raytracing import default_raytracer
        rt = default_raytracer(device)
        rt.upload(self.flatten())
        hits = rt.trace_rays(np.array([list(ray.origin)], np.float32), np.array([list(ray.direction)], np.float32))
        if hits["value"][0] == N.VHX_EMPTY:
            return None
        flat = self.flatten()
        entry = entry_from_value(hits["value"][0], flat.color_palette, flat.data_palette)
        return entry, V3c(*map(float, hits["impact"][0])), V3c(*map(float, hits["normal"][0]))
