"""Inputs of the node-MIP parity tests (tests/test_mip_cases.py, tests/test_gpu_mip_parity.py): MIP views of the random
trees of tests/test_gpu_fuzz.py at every brick_dim the kernels are built for, the device sources of
tests/test_gpu_build_lod.py, and a comparison without a tolerance. Nothing here needs a GPU.

A view is (name, image, node_mips): an image whose nodes have occupied sectants without a child entry, and the node MIP
descriptors that stand in for them (vhx_set_node_mips, vhx_oracle_set_node_mips). Per case:

  lod<d>            tree.flatten_lod(d) with its sampled descriptors, from d = 0 up to the first d that holds every node
                    (taken from the image: insert_at_lod of small boxes makes a few nodes below the canonical leaf depth
                    log4(size / (4 * brick_dim)), so the cut at that depth is neither full nor a cut many rays see)
  internal|leaf|both / sampled|mixed
                    hand-cut images: the arrays of the full flatten() with half of the present children of the
                    Internal nodes, of the Leaf nodes, or of both set to VHX_EMPTY, node_ocbits left alone. `sampled`
                    keeps the full image's descriptors (MIP bricks); `mixed` deals the four kinds of descriptor
                    (Solid, VHX_EMPTY, a random Parted brick, the sampled one) over the nodes that probe their MIP, in
                    a seeded order, and draws a kind at random for every other node. An image without a Solid value
                    gets one appended (the value of an occupied voxel), so the Solid branch runs at every brick_dim.

A hand-cut with a single probing node (an `internal` cut of a two-level tree: the root; every cut of the single Leaf
root of 128/32) has one descriptor to give, so `mixed` makes it Solid there; with two or more, a Solid and a VHX_EMPTY
one are always among them. The `internal` cut of a tree without an Internal node does not exist."""
import collections
import functools

import numpy as np

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from voxelhex_amd.boxtree import TREE_ARRAYS
from tests import _dense_grids as G
from tests import _lod_grids as L
from tests import _points_model as PM
from tests.test_gpu_fuzz import CASES, random_tree
from tests.test_gpu_parity import rand_rays

RAYS = 6000
W, H = 96, 64
FIELDS = ("value", "cell", "voxel", "impact", "normal", "depth", "rgba")
SCHEDULES = ("adaptive", (), (1, 3, 9))  # (1, 3, 9): every ray is resumed many times, in the MIP queue kernel
CUTS = ("internal", "leaf", "both")
MIX_SEED = 0x4D4950

# name, image, node_mips as the issue of the tests states them; cut: "lod" or one of CUTS; full: every node is resident
# depth: the flatten_lod depth of a "lod" view, None for a hand-cut
View = collections.namedtuple("View", "name image node_mips cut mixed full depth")
Case = collections.namedtuple("Case", "tree full origins directions camera")


@functools.lru_cache(maxsize=None)
def case(seed, size, bd):
    """The random tree of tests/test_gpu_fuzz.py with MIP maps on, its full image, 6000 rays and a 96x64 glass camera
    at a random viewpoint, drawn from the tree's generator the way test_random_tree_vs_oracle draws them."""
    tree, rng = random_tree(seed, size, bd)
    tree.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
    o, d = rand_rays(rng, size, RAYS)
    cam = vhx.glass_camera(size, W, H, angle=float(rng.uniform(0, 6.3)), radius=float(rng.uniform(0.3, 2.0)) * size,
                           target=tuple(float(v) for v in rng.uniform(0, size, 3)))
    return Case(tree, tree.flatten(), o, d, cam)


def leaf_depth(size, bd):
    """The depth of the leaves of a tree of canonical depth (root = 0): their edge is 4 * brick_dim."""
    return int(round(np.log2(size / (4 * bd)))) // 2


def occupied(image):
    """(node_count, 64) bool: the sectant's bit of node_ocbits."""
    bits = np.asarray(image.node_ocbits, np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)[None, :]
    return (bits & np.uint64(1)) != 0


def reachable(image):
    """bool per node: reached from the root through the child entries of Internal nodes."""
    ntype = np.asarray(image.node_type)
    ch = np.asarray(image.node_children).reshape(-1, 64)
    seen = np.zeros(ntype.size, bool)
    level = np.array([0], np.int64)
    while level.size:
        seen[level] = True
        inner = level[ntype[level] == N.VHX_NODE_INTERNAL]
        nxt = ch[inner].reshape(-1)
        nxt = nxt[nxt < ntype.size].astype(np.int64)
        level = np.unique(nxt[~seen[nxt]])
    return seen


def probing_nodes(image):
    """The nodes whose MIP a trace can probe: reachable Internal and Leaf nodes with an occupied sectant whose child
    entry is VHX_EMPTY."""
    ntype = np.asarray(image.node_type)
    ch = np.asarray(image.node_children).reshape(-1, 64)
    absent = (occupied(image) & (ch == N.VHX_EMPTY)).any(axis=1)
    kind = (ntype == N.VHX_NODE_INTERNAL) | (ntype == N.VHX_NODE_LEAF)
    return np.flatnonzero(absent & kind & reachable(image))


def _arrays(image):
    return {name: np.array(getattr(image, name), dt) for name, dt in TREE_ARRAYS}


def _hand_cut(full, cut, rng):
    """The arrays of `full` with half (rounded up) of the present children of the nodes `cut` names set to VHX_EMPTY;
    None where those nodes have no present child."""
    arrays = _arrays(full)
    ntype = arrays["node_type"]
    ch = arrays["node_children"].reshape(-1, 64)  # a view: the drops below land in the array
    rows = np.zeros(ntype.size, bool)
    if cut in ("internal", "both"):
        rows |= ntype == N.VHX_NODE_INTERNAL
    if cut in ("leaf", "both"):
        rows |= ntype == N.VHX_NODE_LEAF
    present = np.flatnonzero(((ch != N.VHX_EMPTY) & rows[:, None]).reshape(-1))
    if present.size == 0:
        return None
    drop = rng.permutation(present)[: (present.size + 1) // 2]
    ch.reshape(-1)[drop] = N.VHX_EMPTY
    return arrays


def _occupied_voxel(arrays):
    """The value of the first voxel with a visible colour."""
    v = arrays["voxels"]
    pal = arrays["color_palette"]
    ci = v & 0xFFFF
    ok = ci < pal.size
    ok[ok] = (pal[ci[ok]] >> 24) != 0
    return v[np.flatnonzero(ok)[0]]


def _mixed(image, arrays, sampled, rng):
    """Mixed descriptors for the hand-cut `image` (see the module docstring); appends a Solid value to `arrays` where
    there is none. Returns (arrays, node_mips)."""
    if arrays["solid_values"].size == 0:
        arrays = dict(arrays, solid_values=np.array([_occupied_voxel(arrays)], np.uint32))
    n = arrays["node_type"].size
    bricks = arrays["voxels"].size // image.brick_dim ** 3
    kinds = rng.integers(0, 4, n)
    probing = rng.permutation(probing_nodes(image))
    kinds[probing] = np.arange(probing.size) % 4  # Solid, VHX_EMPTY, Parted, sampled: dealt, not drawn
    solid = (N.VHX_SOLID_BIT | rng.integers(0, arrays["solid_values"].size, n)).astype(np.uint32)
    parted = rng.integers(0, bricks, n).astype(np.uint32)
    mips = np.select([kinds == 0, kinds == 1, kinds == 2], [solid, np.uint32(N.VHX_EMPTY), parted],
                     np.asarray(sampled, np.uint32)).astype(np.uint32)
    return arrays, mips


@functools.lru_cache(maxsize=None)
def mip_views(seed, size, bd):
    """The views of one case of tests/test_gpu_fuzz.CASES, as a tuple of View."""
    c = case(seed, size, bd)
    full = c.full
    views = []
    for d in range(0, 9):  # a tree has at most 8 levels
        image = c.tree.flatten_lod(d)
        whole = image.node_type.size == full.node_type.size
        views.append(View(f"lod{d}", image, np.array(image.node_mips), "lod", False, whole, d))
        if whole:
            break
    assert views[-1].full, "no flatten_lod depth holds every node"
    sampled = np.array(full.node_mips)
    assert sampled.size == full.node_type.size
    for k, cut in enumerate(CUTS):
        rng = np.random.default_rng([MIX_SEED, seed, k])
        arrays = _hand_cut(full, cut, rng)
        if arrays is None:  # no Internal node with a child (a single Leaf root): nothing to drop
            continue
        image = vhx.TreeImage(size, bd, arrays)
        views.append(View(f"{cut}/sampled", image, sampled, cut, False, False, None))
        marrays, mips = _mixed(image, arrays, sampled, rng)
        views.append(View(f"{cut}/mixed", vhx.TreeImage(size, bd, marrays), mips, cut, True, False, None))
    return tuple(views)


# ---------------------------------------------------------------------------------------------- device-built images
def device_lod_sources():
    """(shape name, kind) of every source tests/test_gpu_build_lod.py builds on the device: the tests/_lod_grids.SHAPES
    grids, plain, simplified and edited."""
    return [(name, kind) for name in L.SHAPES for kind in ("plain", "simplified", "edited")]


def build_lod_source(src, name, kind):
    """Makes the grid `name` of tests/_lod_grids.SHAPES the tree of the Raytracer `src`: plain, simplified, or plain
    and then edited on the device."""
    size, bd, _ = L.SHAPES[name]
    g, d = L.pair(name)
    src.build_dense(g, size, bd, data=d, simplify=kind == "simplified")
    if kind != "edited":
        return
    # scattered inserts, clears and a dense box, without compaction: orphaned slots and edit-order numbering
    rng = np.random.default_rng(size * 7 + bd)
    q = max(size // 4, 2)
    pos, a, dd = PM.random_points(rng, size, 40 * q, G.COLORS, [0, 5, 9], hi=(q + 5 if size > 4 else 4,) * 3)
    src.set_voxels(pos, a, dd, "insert")
    src.clear_voxels(pos[::3])
    box = np.where(rng.random((q // 2 + 1, 3, q)) < 0.5, G.COLORS[1], 0).astype(np.uint32)
    src.write_dense(box, origin=(1, 0, 1) if size > 4 else (0, 0, 0))
    if size > 4:  # the first leaf cleared as a whole, which unlinks it, and a voxel put back: a new leaf at the end
        src.fill_box((0, 0, 0), (4 * bd,) * 3, 0)
        src.set_voxels(np.array([[1, 1, 1]], np.uint32), G.COLORS[0], 0, "insert")
    src.set_voxels(pos[1::5], G.COLORS[4], 11, "replace")
    if size > 4:
        assert src.orphans() != (0, 0), "the edits left no orphaned slot"


# ------------------------------------------------------------------------------------------------------- comparison
def assert_bits(got, ref, what=""):
    """Every field of `ref` equals `got`'s as uint32 bits, floats included: no tolerance."""
    for k in ref:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.itemsize == 4 and b.itemsize == 4, (k, a.dtype, b.dtype)
        assert a.shape == b.shape, f"{what}: {k} has shape {a.shape}, the reference {b.shape}"
        ua, ub = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero((ua != ub).reshape(ua.shape[0], -1).any(axis=1))
        assert bad.size == 0, (f"{what}: {k} differs in bits at {bad.size} of {ua.shape[0]} rays, first {bad[:5]}: "
                               f"{a[bad[:3]].tolist()} vs {b[bad[:3]].tolist()}")


def changed_rays(on, off):
    """The rays whose value or depth bits differ between two traces."""
    return (on["value"] != off["value"]) | (on["depth"].view(np.uint32) != off["depth"].view(np.uint32))
