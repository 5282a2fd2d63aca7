"""The two DDA walks (the brick-cell walk of probe_brick, the ADVANCE / POP walk of the node loop) trip by trip.

Explicit rays through the smallest trees in which a walk can go wrong -- one leaf node (size 4 * brick_dim), a two-level
tree (size 16 * brick_dim) and, for the restart from the root, a sparse tree deeper than the node stack -- at brick_dim
1, 2, 4 and 8 (8: more than one occupancy word per brick). Every plane is compared bit for bit with the oracle, for one
unbounded pass and for schedules of small budgets that abandon rays between two walks and resume them.

Each class of ray the walks have to get right is aimed by construction; that it is really there is asserted on the CPU
from the oracle's own outputs (hit or miss, the hit voxel, and the byte count, which counts the node iterations and the
cells a walk visits: 12 per node iteration, 4 per leaf probe, 4 per visited cell of a Parted brick plus 4 for an
occupied one's colour, 4 per PUSH) before anything runs on the GPU.
"""
import functools

import numpy as np
import pytest

import voxelhex_amd as vhx
from tests._oracle import Oracle
from voxelhex_amd import _native as N

RED = np.uint32(0xFF0000FF)
FIELDS = ("value", "cell", "voxel", "impact", "normal", "depth", "rgba")
NAN, INF = np.float32("nan"), np.float32("inf")
# zero, NaN and infinite direction components: a walk that makes no progress runs into the iteration bound
DEGENERATE = [(0, 0, 0), (NAN, 0, 0), (NAN, NAN, NAN), (0, NAN, 1), (INF, 0, 0), (INF, INF, 0), (-INF, 1, 1),
              (1e-30, 0, 0), (-0.0, -0.0, -1)]
BUDGETS = [(), (1,), (2, 5), (1, 2, 3), (3, 4, 9)]
DEFAULT_BUDGETS = (32, 128, 768)  # the library default (ctx.hpp), as the other GPU tests leave it


def unit(v):
    v = np.asarray(v, np.float32)
    l = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).astype(np.float32)
    return (v / l).astype(np.float32)


def leaf_grid(bd):
    """One leaf node (4 x 4 x 4 bricks of bd^3 cells), indexed [z, y, x]:
    brick A (sectant 1,1,1) holds one voxel, in its far corner cell; brick B (sectant 3,3,3, the node's far corner) one
    in its near corner cell; brick C (sectant 0,2,0) is full; brick D (sectant 2,1,1) holds its near corner cell; a few
    scattered voxels make the rest."""
    s = 4 * bd
    g = np.zeros((s, s, s), np.uint32)
    g[2 * bd - 1, 2 * bd - 1, 2 * bd - 1] = RED
    g[3 * bd, 3 * bd, 3 * bd] = RED
    g[0:bd, 2 * bd:3 * bd, 0:bd] = RED
    g[bd, bd, 2 * bd] = RED
    rng = np.random.default_rng(bd)
    for x, y, z in rng.integers(0, s, (6, 3)):
        if not (bd <= x < 3 * bd and bd <= y < 2 * bd and bd <= z < 2 * bd) and min(x, y, z) < 3 * bd:
            g[z, y, x] = np.uint32(0xFF00FF00)
    return g


class Rays:
    def __init__(self):
        self.o, self.d, self.cls, self.want = [], [], {}, []

    def add(self, name, o, d, hit=None, voxel=None, nbytes=None, min_bytes=None):
        """A ray of class `name`; what the oracle must report for it so that it is a member of the class."""
        self.cls.setdefault(name, []).append(len(self.o))
        self.o.append(np.asarray(o, np.float32))
        self.d.append(np.asarray(d, np.float32))
        self.want.append((name, hit, voxel, nbytes, min_bytes))


def leaf_rays(r, bd, base, levels):
    """The rays of one leaf node whose cube starts at `base` (a node of `levels` levels below the root: every level
    above adds a node iteration and a PUSH, 16 bytes, before the leaf's first iteration)."""
    b = np.asarray(base, np.float32)
    u = np.float32(1.0)  # a cell
    A = b + bd  # brick A's minimum; its far corner cell is A + bd - 1
    far = A + (bd - 1)
    B = b + 3 * bd
    first = 16 * levels + 12 + 4  # bytes up to the first leaf probe's cell reads
    if bd >= 2:
        # a walk that ends on its first trip by hitting: from the cell before A's voxel, along +x
        r.add("first_trip_hit", far + (-0.5, 0.5, 0.5), unit((1, 1e-3, 2e-3)), True, far, first + 4 + 8)
        # ... and by leaving the brick: from B's far corner cell outwards (the brick's, the node's and the tree's end:
        # one cell read, then the node iteration that pops the root)
        r.add("first_trip_leave", B + (bd - 0.5, bd - 0.25, bd - 0.75), unit((1, 0.3, 0.2)), False,
              nbytes=first + 4 + 12 if levels == 0 else None)
        # the longest walk, 3 * bd - 2 cells: from A's near corner cell to its far corner cell, no two axes at once
        o = A + (0.1, 0.2, 0.3)
        r.add("max_walk", o, unit(far + (0.5, 0.55, 0.6) - o), True, far, first + 4 * (3 * bd - 3) + 8)
        # ties: the cell diagonal (three axes at once, bd cells), both ways, and a face diagonal (two axes)
        r.add("tie3", A + (0.5, 0.5, 0.5), unit((1, 1, 1)), True, far, first + 4 * (bd - 1) + 8)
        r.add("tie3", B + (bd - 0.5, bd - 0.5, bd - 0.5), unit((-1, -1, -1)), True, B, first + 4 * (bd - 1) + 8)
        r.add("tie2", A + (0.5, 0.5, bd - 0.5), unit((1, 1, 0)), True, far, first + 4 * (bd - 1) + 8)
        r.add("tie2", far + (0.5, -bd + 1.5, -bd + 1.5), unit((0, 1, 1)), True, far, first + 4 * (bd - 1) + 8)
        # entering exactly on cell planes: inside the brick on the plane between two cells, and on a cell edge
        r.add("on_plane", far + (-1.0, 0.5, 0.5), unit((1, 1e-3, 1e-3)), True, far)
        r.add("on_plane", far + (-1.0, 0.0, 0.5), unit((1, 1e-3, 0)), True, far)
        r.add("on_plane", far + (-1.0, 0.0, 0.0), unit((1, 1, 1)), None)
        r.add("on_plane", far + (0.5, 0.5, -1.0), (0, 0, 1), True, far, first + 4 + 8)
    # the tree's diagonal from outside: ADVANCE steps over three axes at once, then A's diagonal
    # (brick_dim 1: a brick is one voxel and the diagonal meets the neighbouring leaf's first)
    r.add("tie3_advance", b - 1, unit((1, 1, 1)), True, far if bd >= 2 else None)
    r.add("tie3_advance", b + 4 * bd + 1, unit((-1, -1, -1)), True, B if bd >= 2 else None)
    # axis-parallel rays, zero components of either sign: ADVANCE across the node, then along a row of A's cells
    r.add("axis", (b[0] - 1, far[1] + 0.5, far[2] + 0.5), (1, 0, 0), True, far)
    r.add("axis", (far[0] + 0.5, far[1] + 0.5, b[2] + 4 * bd + 1), (-0.0, 0.0, -1.0), True, far)
    r.add("axis", (far[0] + 0.5, b[1] - 1, far[2] + 0.5), (0, 1, -0.0), True, far)
    r.add("axis", (b[0] + 0.5 * u, b[1] + 4 * bd + 2, b[2] + bd * 3.5), (0, -1, 0), None)
    # from outside exactly on a plane between two rows of cells (and of bricks)
    r.add("on_plane", (b[0] - 1, far[1], far[2] + 0.5), (1, 0, 0), None)
    r.add("on_plane", (b[0] - 1, A[1], A[2]), (1, 0, 0), None)
    # a ray that crosses several bricks before its hit: walks with node iterations between them
    r.add("many_walks", b + (-1, bd + 0.3, bd + 0.6), unit((1, 0.02, 0.01)), True,
          b + (2 * bd, bd, bd) if bd >= 2 else None, min_bytes=16 * levels + 3 * 16 if bd >= 2 else None)
    # no progress: the iteration bound ends the walk (inside A's cells, in an empty brick, and from outside). Each such
    # ray costs the bound's 2^22 trips: a leaf tree takes all of them, a tree with a root above one NaN direction from
    # inside A's cells (brick_dim 4 four), so that every brick_dim meets the bound below an ADVANCE walk too
    if levels == 0:
        deg = DEGENERATE
    else:
        deg = DEGENERATE[:4] if bd == 4 else DEGENERATE[3:4]
    for dd in deg:
        r.add("degenerate", A + (0.5, 0.5, 0.5) if bd >= 2 else b + (0.5, 0.5, 0.5), dd, None)
    if levels == 0:
        for dd in DEGENERATE[:4]:
            r.add("degenerate", b + (2 * bd + 0.5, 3 * bd + 0.5, 0.25), dd, None)
            r.add("degenerate", b + (-3, bd + 0.5, bd + 0.5), dd, None)


@functools.lru_cache(maxsize=None)
def case(bd, kind):
    """(flat tree, origins, directions, the oracle's planes, classes) of one tree; asserts the classes are present."""
    r = Rays()
    rng = np.random.default_rng(100 * bd + len(kind))
    if kind == "leaf":
        size, g = 4 * bd, leaf_grid(bd)
        leaf_rays(r, bd, (0, 0, 0), 0)
    elif kind == "two_level":
        # the leaf node's content in the root's sectants (0,0,0), (1,1,1) and (3,3,3)
        size, n = 16 * bd, 4 * bd
        g = np.zeros((size, size, size), np.uint32)
        for k in (0, 1, 3):
            g[k * n:(k + 1) * n, k * n:(k + 1) * n, k * n:(k + 1) * n] = leaf_grid(bd)
        leaf_rays(r, bd, (n, n, n), 1)
        # POP: out of the leaf at (3,3,3) through the root's far corner (the POP's single step leaves the root), and
        # out of the leaf at (1,1,1) into the root's empty sectants (the POP's step stays, ADVANCE goes on to the end)
        if bd >= 2:  # (brick_dim 1: brick B is its voxel, a ray cannot start in an empty cell of it)
            r.add("pop_leaves_node", np.full(3, 3 * n + 3 * bd, np.float32) + (bd - 0.5, bd - 0.25, bd - 0.75),
                  unit((1, 0.3, 0.2)), False, min_bytes=16 + 16 + 12)
            r.add("pop_stays", np.full(3, n + 3 * bd, np.float32) + (bd - 0.5, bd - 0.25, bd - 0.75),
                  unit((1, 0.1, 0.2)), False, min_bytes=16 + 16 + 12 + 12)
        r.add("pop_stays", (n + 0.5, n + 0.25, -2), unit((0.01, 0.02, 1)), None, min_bytes=16 + 16 + 12 + 12)
    else:
        # five node levels (the node stack holds four): a ray from inside the leaf node at the origin to a wall 256
        # bricks away pops until the stack is empty and restarts from the root on its way. The restart moves the point
        # 0.1 along the ray, into the wall's voxel: the impact lies 0.1 behind the voxel's face, where a ray that
        # stepped there would sit on the face
        size, g = 1024 * bd, None
        tree = vhx.BoxTree(size, bd)
        filled = [(256 * bd, y, z) for y in range(bd, 2 * bd) for z in range(bd, 2 * bd)]
        filled += [(2 * bd - 1, 2 * bd - 1, 2 * bd - 1), (0, 0, 0), (3 * bd, 3 * bd, 3 * bd)]
        for pos in filled:
            tree.insert(pos, vhx.Albedo.from_u32(int(RED)))
        r.add("restart", (2 * bd + 1.5, bd + 0.5, bd + 0.5), unit((1, 1e-4, 2e-4)), True, (256 * bd, bd, bd),
              min_bytes=16 * 4 + 12 * 5)
        r.add("restart", (3 * bd + 0.5, bd + 0.25, bd + 0.5), (1, 0, 0), True, (256 * bd, bd, bd),
              min_bytes=16 * 4 + 12 * 5)
    # scattered rays from outside and from inside the tree, half of them aimed at voxels
    m, ext = 192, float(min(size, 64 * bd))
    vox = np.argwhere(g)[:, ::-1] if g is not None else np.array(filled)
    o = rng.uniform(-0.25 * ext, 1.25 * ext, (m, 3)).astype(np.float32)
    o[::3] = rng.uniform(0.0, min(ext, 16.0 * bd), (len(o[::3]), 3)).astype(np.float32)
    t = rng.uniform(0.0, min(ext, 16.0 * bd), (m, 3)).astype(np.float32)
    t[::2] = (vox[rng.integers(0, len(vox), len(t[::2]))] + rng.uniform(0.1, 0.9, (len(t[::2]), 3))).astype(np.float32)
    for k in range(m):
        r.add("scattered", o[k], unit(t[k] - o[k]), None)
    flat = vhx.FlatTree.from_dense(g, size, bd) if g is not None else tree.flatten()
    o, d = np.array(r.o, np.float32), np.array(r.d, np.float32)
    ref = Oracle().trace_rays(flat, o, d, count_bytes=True, fields=FIELDS)
    for k, (name, hit, voxel, nbytes, min_bytes) in enumerate(r.want):
        got_hit = ref["value"][k] != N.VHX_EMPTY
        ctx = f"bd {bd} {kind} ray {k} ({name}): o {o[k]} d {d[k]} bytes {ref['bytes'][k]} voxel {ref['voxel'][k]}"
        if hit is not None:
            assert bool(got_hit) == hit, ctx
        if voxel is not None:
            assert np.array_equal(ref["voxel"][k], np.asarray(voxel, np.float32).astype(ref["voxel"].dtype)), ctx
        if nbytes is not None:
            assert ref["bytes"][k] == nbytes, f"{ctx}: expected {nbytes} bytes"
        if min_bytes is not None:
            assert ref["bytes"][k] >= min_bytes, f"{ctx}: expected at least {min_bytes} bytes"
    deg = r.cls.get("degenerate", [])
    if deg:  # at least one of them comes back a miss (none of these directions can leave its cell or its tree)
        assert (ref["value"][deg] == N.VHX_EMPTY).any()
    if kind == "leaf":  # ... and among the full set some still hit (an infinite or tiny component still advances)
        assert (ref["value"][deg] != N.VHX_EMPTY).any(), (bd, kind)
    # abandon and resume: some ray must go on past its first node iteration, where the schedules that start with a
    # budget of 1 or 2 steps abandon it between two walks. One node iteration reads at most 12 + 4 + 4 bytes, 4
    # per cell of a brick walk (3 * bd - 2 cells at most) and 4 for the colour of the occupied cell that ends the walk,
    # so more bytes than that took a second iteration
    assert (ref["bytes"] > 24 + 4 * (3 * bd - 2)).sum() >= 8, (bd, kind)
    for k in r.cls.get("restart", []):
        assert ref["impact"][k][0] > np.float32(ref["voxel"][k][0]), (k, ref["impact"][k], ref["voxel"][k])
    sc = r.cls["scattered"]
    assert (ref["value"][sc] != N.VHX_EMPTY).sum() >= 8 and (ref["value"][sc] == N.VHX_EMPTY).sum() >= 8
    return flat, o, d, ref, r.cls


CASES = [(bd, kind) for bd in (4, 1, 2, 8) for kind in ("leaf", "two_level")] + [(4, "deep")]
NEEDED = {"leaf": ("first_trip_hit", "first_trip_leave", "max_walk", "tie3", "tie2", "on_plane", "tie3_advance", "axis",
                   "many_walks", "degenerate"),
          "two_level": ("first_trip_hit", "max_walk", "tie3", "pop_leaves_node", "pop_stays", "degenerate"),
          "deep": ("restart",)}


@pytest.mark.parametrize("bd,kind", CASES)
def test_ray_classes_are_present(bd, kind):
    """The precondition of the GPU comparison, from the oracle alone (runs without a GPU)."""
    cls = case(bd, kind)[4]
    for name in NEEDED[kind]:
        if bd == 1 and name in ("first_trip_hit", "first_trip_leave", "max_walk", "tie3", "tie2", "pop_leaves_node"):
            continue  # a brick of one cell has no walk
        assert cls.get(name), (bd, kind, name)


def same_bits(got, ref, ctx):
    for k in ref:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (ctx, k)
        bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{ctx}: {k} differs at rays {bad[:8]}: {a[bad[:3]]} vs {b[bad[:3]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("bd,kind", CASES)
def test_walk_trips_vs_oracle(gpu, bd, kind):
    """Every plane bit for bit, in one unbounded pass and abandoned at small budgets and resumed."""
    flat, o, d, ref, cls = case(bd, kind)
    gpu.upload(flat)
    try:
        for budgets in BUDGETS:
            gpu.set_pass_budgets(budgets)
            if budgets:
                # the degenerate rays spend the bound's 2^22 trips once per trace: only in the unbounded pass and in one
                # small-budget schedule
                keep = np.ones(len(o), bool)
                if budgets != (1, 2, 3):
                    keep[cls.get("degenerate", [])] = False
                got = gpu.trace_rays(o[keep], d[keep], fields=FIELDS, count_bytes=True)
                same_bits(got, {k: v[keep] for k, v in ref.items()}, f"bd {bd} {kind} budgets {budgets}")
            else:
                whole = gpu.trace_rays(o, d, fields=FIELDS, count_bytes=True)
                same_bits(whole, ref, f"bd {bd} {kind} one pass")
    finally:
        gpu.set_pass_budgets(DEFAULT_BUDGETS)


@pytest.mark.gpu
@pytest.mark.parametrize("bd,kind", [(bd, kind) for bd in (4, 1, 2, 8) for kind in ("leaf", "two_level")])
def test_batch_pass0_walks_vs_oracle(gpu, oracle, bd, kind):
    """The batch pass 0 is the kernel that walks through walk_cells: whole frames of the same trees through
    trace_primary_batch, from a far, a near and an oblique camera (long ADVANCE walks, long brick walks, many ties on
    the axis-aligned rows), every plane the batch writes bit for bit against the oracle's frames; with the default
    budgets and with budgets that end pass 0 between two walks."""
    import torch
    flat = case(bd, kind)[0]
    size = float(flat.boxtree_size)
    gpu.upload(flat)
    W, H = 80, 48  # not a multiple of the 16x16 block: ragged blocks at the right edge
    cams = [vhx.glass_camera(size, W, H, target=(size / 2.0,) * 3),
            vhx.glass_camera(size, W, H, radius=0.6 * size, target=(size / 2.0,) * 3),
            vhx.glass_camera(size, W, H, angle=0.0, radius=0.9 * size, target=(0.0, size / 4.0, size / 2.0))]
    fields = ("value", "rgba", "depth")
    refs = [oracle.trace_primary(flat, cam, 0, 0, W, H, fields=fields) for cam in cams]
    assert any((r["value"] != N.VHX_EMPTY).sum() > 16 for r in refs), "no camera sees the voxels"
    try:
        for budgets in (DEFAULT_BUDGETS, (2, 5), (1, 2, 3)):
            gpu.set_pass_budgets(budgets)
            outs = [{"value": torch.full((W * H,), 7, dtype=torch.int32, device="cuda"),
                     "rgba": torch.full((W * H,), 7, dtype=torch.int32, device="cuda"),
                     "depth": torch.full((W * H,), 7.0, dtype=torch.float32, device="cuda")} for _ in cams]
            torch.cuda.synchronize()  # the fills run on torch's stream, the batch on the context's
            gpu.trace_primary_batch(cams, outs)
            gpu.sync()
            for k, (o, r) in enumerate(zip(outs, refs)):
                for f in fields:
                    a = o[f].cpu().numpy().view(np.uint32).reshape(-1)
                    b = np.ascontiguousarray(r[f]).view(np.uint32).reshape(-1)
                    bad = np.flatnonzero(a != b)
                    assert bad.size == 0, f"bd {bd} {kind} budgets {budgets} camera {k}: {f} differs at {bad[:8]}"
    finally:
        gpu.set_pass_budgets(DEFAULT_BUDGETS)
