"""vhx_compact_tree on the GPU (Raytracer.compact): the resident tree rewritten without its unreachable slots, in the
builders' numbering. The device image is held to the host's (TreeImage.compacted) and to the numpy model
(tests/_compact_model.py); reads, gets and frames must not change; refusals leave the tree as it was. Every comparison is
bit for bit."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import FlatTree
from voxelhex_amd import _native as N
from tests import _dense_grids as G
from tests import _flatget as F
from tests import _simplify_grids as SG
from tests._compact_model import model_compact, scramble
from tests._treecheck import check_tree
from tests.test_compact import LOD_CASES, SCRAMBLE_SIZES, lod_image, malformed

pytestmark = pytest.mark.gpu

EMPTY = N.VHX_EMPTY
W = 64
SIZE, BD = 64, 4
NEW = [G.rgba(1, 200, 200), G.rgba(77, 1, 99, 3), G.rgba(5, 5, 5)]  # colours no base grid holds
_cache = {}


def positions(size):
    if size not in _cache:
        _cache[size] = F.lattice((0, 0, 0), (size,) * 3)
    return _cache[size]


def camera(size=SIZE):
    return vhx.glass_camera(size, W, W, target=(size / 2,) * 3)


def bits(frame):
    return {k: np.ascontiguousarray(v).view(np.uint32) for k, v in frame.items()}


def assert_same_frame(got, want, what):
    got, want = bits(got), bits(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.count_nonzero(got[k] != want[k])} entries"


def random_box_grid(rng, extents, density=0.5):
    gx, gy, gz = extents
    colours = np.concatenate([G.COLORS, np.array(NEW, np.uint32)])
    g = np.zeros((gz, gy, gx), np.uint32)
    mask = rng.random(g.shape) < density
    g[mask] = colours[rng.integers(0, len(colours), int(mask.sum()))]
    return g


@pytest.fixture()
def rt():
    r = vhx.Raytracer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def second():
    r = vhx.Raytracer(0)
    yield r
    r.close()


def assert_derived_as_uploaded(rt, second, img, what):
    """Node headers and brick bitmaps equal those of a context that uploaded `img`; returns that context's bytes."""
    second.upload(img)
    d = img.desc
    words = max(1, int(d.brick_dim) ** 3 // 64)
    assert np.array_equal(rt.read_derived(N.VHX_DERIVED_NODE_HDR, 0, d.node_count),
                          second.read_derived(N.VHX_DERIVED_NODE_HDR, 0, d.node_count)), f"{what}: node headers"
    if d.brick_count:
        assert np.array_equal(rt.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, d.brick_count * words),
                              second.read_derived(N.VHX_DERIVED_BRICK_OCC, 0, d.brick_count * words)), \
            f"{what}: brick bitmaps"
    return second.device_bytes()


# ------------------------------------------------------------------------------------------ 1. identity on the device
@pytest.mark.parametrize("simplify", [False, True])
def test_identity_on_a_built_tree(rt, oracle, simplify):
    grid = SG.make_grid("brick_noise", SIZE, BD)
    rt.build_dense(grid, SIZE, BD, simplify=simplify)
    before, held = rt.download(), rt.device_bytes()
    frame = rt.trace_primary(camera())
    assert rt.compact() == (0, 0)
    G.assert_same_image(rt.download(), before, f"simplify={simplify}")
    assert rt.orphans() == (0, 0) and rt.device_bytes() <= held
    assert_same_frame(rt.trace_primary(camera()), frame, f"simplify={simplify}: frame")


# -------------------------------------------------------------------------------------------- 2. scrambled uploads
@pytest.mark.parametrize("size,bd", SCRAMBLE_SIZES)
def test_scrambled_upload_compacts_back(rt, second, oracle, size, bd):
    what = f"{size}/{bd}"
    img = FlatTree.from_dense(SG.make_grid("brick_noise", size, bd), size, bd, simplify=True)
    mixed = scramble(img, np.random.default_rng(size + bd), 7, 11)
    rt.upload(mixed)
    cam = camera(size)
    frame = rt.trace_primary(cam)
    assert rt.compact() == (7, 11)
    got = rt.download()
    G.assert_same_image(got, img, f"{what}: against the original")
    G.assert_same_image(got, mixed.compacted(), f"{what}: against the host's compaction")
    assert rt.tree_counts().node_count == img.desc.node_count and rt.tree_counts().brick_count == img.desc.brick_count
    assert rt.device_bytes() <= assert_derived_as_uploaded(rt, second, got, what)
    want = oracle.trace_primary(img, cam, 0, 0, W, W)
    assert_same_frame(frame, want, f"{what}: the scrambled tree's frame")
    assert_same_frame(rt.trace_primary(cam), want, f"{what}: the compacted tree's frame")


# ------------------------------------------------------------------------------------------------ 3. after real edits
def edit_base_grid():
    """blocks4 (UniformLeaf nodes over a Parted brick, and the first leaf in 2^3 blocks), one leaf of one colour (a
    UniformLeaf over a Solid brick) and one leaf of brick_noise (Solid bricks in a Leaf)."""
    g = SG.make_grid("blocks4", SIZE, BD)
    g[48:64, 48:64, 48:64] = SG.THREE[0]
    g[32:48, 0:16, 0:16] = SG.make_grid("brick_noise", SIZE, BD)[32:48, 0:16, 0:16]
    g[0:16, 0:16, 16:32] = SG.THREE[1]  # root sectant 1, cleared below
    return g


def uniform_parted_leaf(img, skip=(1,)):
    """Root sectant of a UniformLeaf over a Parted brick (the root's children are the leaves at 64 / 4)."""
    ch = img.node_children.reshape(-1, 64)
    for s in range(64):
        n = ch[0, s]
        if s in skip or n == EMPTY or img.node_type[n] != N.VHX_NODE_UNIFORM_LEAF:
            continue
        if ch[n, 0] != EMPTY and not ch[n, 0] & N.VHX_SOLID_BIT:
            return s
    raise AssertionError("no UniformLeaf over a Parted brick")


def edited_tree(rt):
    """The base and the series of edits; returns the numpy cube of visible colours."""
    rng = np.random.default_rng(42)
    rt.build_dense(edit_base_grid(), SIZE, BD, simplify=True)
    img = rt.download()
    types, empty, solid, parted = SG.entry_kinds(img)
    leaf, uni = types == N.VHX_NODE_LEAF, types == N.VHX_NODE_UNIFORM_LEAF
    assert (uni & solid[:, 0]).any() and (uni & parted[:, 0]).any() and (leaf & solid.any(1)).any(), "the base's cases"
    cube = rt.read_dense()

    def write(grid, origin):
        rt.write_dense(grid, origin)
        (ox, oy, oz), (gz, gy, gx) = origin, grid.shape
        cube[oz:oz + gz, oy:oy + gy, ox:ox + gx] = np.where(grid >> 24 != 0, grid, 0)

    s = uniform_parted_leaf(img)
    x0, y0, z0 = 16 * (s & 3), 16 * ((s >> 2) & 3), 16 * (s >> 4)
    write(random_box_grid(rng, (7, 5, 9)), (x0 + 1, y0 + 2, z0 + 3))  # over a UniformLeaf with a Parted brick
    write(random_box_grid(rng, (7, 5, 9)), (49, 50, 51))              # over the UniformLeaf with a Solid brick
    write(np.zeros((16, 16, 16), np.uint32), (16, 0, 0))              # root sectant 1 leaves
    write(random_box_grid(rng, (14, 13, 12), 0.7), (17, 1, 2))        # into the emptied space: a new leaf node
    write(np.zeros((12, 13, 7), np.uint32), (17, 1, 2))               # half of it cleared
    return cube


def test_after_real_edits_and_editing_goes_on(rt, second, oracle):
    cube = edited_tree(rt)
    pos, cam = positions(SIZE), camera()
    dense, values, frame = rt.read_dense(), rt.get(pos), rt.trace_primary(cam)
    assert np.array_equal(dense, cube)
    orphans, old, held = rt.orphans(), rt.download(), rt.device_bytes()
    assert orphans[0] > 0 and orphans[1] > 0, orphans
    reach = check_tree(old, orphans, "before")

    assert rt.compact() == orphans  # built, not uploaded: every unreachable slot is an orphan
    assert rt.orphans() == (0, 0)
    new, counts = rt.download(), rt.tree_counts()
    assert (counts.node_count, counts.brick_count) == reach
    G.assert_same_image(new, old.compacted(), "against the host's compaction")
    G.assert_same_image(new, model_compact(old), "against the model")
    assert check_tree(new, (0, 0), "after") == reach
    assert np.array_equal(rt.read_dense(), dense) and np.array_equal(rt.get(pos), values)
    after = rt.trace_primary(cam)
    assert_same_frame(after, frame, "frame before and after")
    assert_same_frame(after, oracle.trace_primary(new, cam, 0, 0, W, W), "frame against the oracle on the new image")
    fresh = assert_derived_as_uploaded(rt, second, new, "after")
    assert rt.device_bytes() < held and rt.device_bytes() <= fresh, (rt.device_bytes(), held, fresh)

    # 4. editing goes on
    grid = np.full((9, 20, 11), G.rgba(9, 99, 199), np.uint32)
    rt.write_dense(grid, (5, 30, 40))
    cube[40:49, 30:50, 5:16] = grid
    rt.fill_box((0, 0, 0), (33, 17, 64), 0)
    cube[0:64, 0:17, 0:33] = 0
    assert np.array_equal(rt.read_dense(), cube)
    edited = rt.download()
    check_tree(edited, rt.orphans(), "edited after the compaction")
    assert_same_frame(rt.trace_primary(cam), oracle.trace_primary(edited, cam, 0, 0, W, W), "edited: frame")
    dropped = rt.compact()
    assert dropped == check_orphans(edited)
    G.assert_same_image(rt.download(), model_compact(edited), "the second compaction")
    assert np.array_equal(rt.read_dense(), cube)


def check_orphans(img):
    """(unreachable nodes, unreachable bricks) of an image by the model."""
    m = model_compact(img)
    return img.desc.node_count - m.desc.node_count, img.desc.brick_count - m.desc.brick_count


def test_new_nodes_at_two_levels(rt, oracle):
    """64 / brick_dim 1 has three node levels: a write into a cleared root sectant creates a level-1 node and leaves."""
    size, bd = 64, 1
    rt.build_dense(G.make_grid("sparse", size), size, bd)
    rt.fill_box((16, 0, 0), (16, 16, 16), 0)
    before = rt.tree_counts().node_count
    rt.write_dense(random_box_grid(np.random.default_rng(3), (9, 7, 6)), (19, 2, 3))
    assert rt.tree_counts().node_count >= before + 3
    rt.fill_box((19, 2, 3), (5, 7, 6), 0)
    pos, cam = positions(size), camera(size)
    old, values, frame, orphans = rt.download(), rt.get(pos), rt.trace_primary(cam), rt.orphans()
    assert orphans[0] > 1 and orphans[1] > 0
    assert rt.compact() == orphans
    new = rt.download()
    G.assert_same_image(new, model_compact(old), "64/1")
    G.assert_same_image(new, old.compacted(), "64/1 host")
    check_tree(new, (0, 0), "64/1")
    assert np.array_equal(rt.get(pos), values)
    assert_same_frame(rt.trace_primary(cam), frame, "64/1 frame")


# ------------------------------------------------------------------------------------------------------ 5. all cleared
def test_all_cleared(rt, oracle):
    rt.build_dense(G.make_grid("sparse", SIZE), SIZE, BD)
    rt.fill_box((0, 0, 0), (SIZE,) * 3, 0)
    nodes, bricks = rt.orphans()
    assert rt.compact() == (nodes, bricks) and nodes > 0 and bricks > 0
    counts = rt.tree_counts()
    assert counts.node_count == 1 and counts.brick_count == 0
    img = rt.download()
    assert img.node_type.tolist() == [N.VHX_NODE_NOTHING] and (img.node_children == EMPTY).all()
    cam = camera()
    assert (rt.trace_primary(cam)["value"] == EMPTY).all(), "all sky"
    rt.write_dense(random_box_grid(np.random.default_rng(8), (22, 18, 35)), (13, 15, 3))
    img = rt.download()
    check_tree(img, (0, 0), "written again")
    frame = rt.trace_primary(cam)
    assert (frame["value"] != EMPTY).any()
    assert_same_frame(frame, oracle.trace_primary(img, cam, 0, 0, W, W), "written again: frame")


# -------------------------------------------------------------------------------------------------- 6. frames in flight
def test_frames_in_flight(oracle):
    import torch
    cam = camera()
    fields = ("value", "cell", "depth", "rgba")
    owner = vhx.Raytracer(0)
    try:
        edited_tree(owner)
        old = owner.download()
        want = bits(oracle.trace_primary(old, cam, 0, 0, W, W))
        shared = [owner.shared(), owner.shared()]
        dt = {"value": torch.int32, "cell": torch.int32, "depth": torch.float32, "rgba": torch.int32}
        outs = [[[{f: torch.zeros(W * W, dtype=dt[f], device="cuda:0") for f in fields} for _ in range(3)]
                 for _ in shared] for _ in range(2)]
        torch.cuda.synchronize()
        for sh, o in zip(shared, outs[0]):
            sh.trace_primary_batch([cam] * 3, o)
        dropped = owner.compact()  # no synchronisation before it
        for sh, o in zip(shared, outs[1]):
            sh.trace_primary_batch([cam] * 3, o)
        for sh in shared:
            sh.sync()
        assert dropped[0] > 0 and dropped[1] > 0
        new = owner.download()
        assert_same_frame(oracle.trace_primary(new, cam, 0, 0, W, W), want, "the oracle on the new image")
        for r, round_ in enumerate(outs):
            for k, ctx_outs in enumerate(round_):
                for j, o in enumerate(ctx_outs):
                    for f in fields:
                        got = o[f].cpu().numpy().view(np.uint32)
                        assert np.array_equal(got, want[f].reshape(-1)), \
                            f"{'after' if r else 'before'} the compaction, context {k}, frame {j}: {f}"
        for sh in shared:
            sh.close()
    finally:
        owner.close()


# ------------------------------------------------------------------------------------------------------- 7. refusals
def refused(call):
    with pytest.raises(N.VhxError) as e:
        call()
    assert e.value.code == N.VHX_E_STATE
    return e.value


def test_refusals_leave_the_tree_as_it_was(rt):
    assert N.lib().vhx_compact_tree(rt._h, None, None) == N.VHX_E_STATE  # before any upload
    assert N.lib().vhx_compact_tree(None, None, None) == N.VHX_E_INVALID_ARG
    edited_tree(rt)
    before, orphans = rt.download(), rt.orphans()
    sh = rt.shared()
    refused(sh.compact)
    sh.close()
    G.assert_same_image(rt.download(), before, "after the refusal on a shared context")
    assert rt.orphans() == orphans

    flat = lod_image(64, 4, 0)
    rt.upload(flat)
    rt.set_node_mips(flat.node_mips)
    before = rt.download()
    refused(rt.compact)
    G.assert_same_image(rt.download(), before, "after the refusal under node MIPs")
    assert rt.orphans() == (0, 0)
    rt.set_node_mips(None)

    for kind in ("node with two parents", "brick referenced twice"):
        img = malformed(kind)
        rt.upload(img)
        held = rt.device_bytes()
        assert "twice" in str(refused(rt.compact)), kind
        G.assert_same_image(rt.download(), img, f"after the refusal of {kind}")
        assert rt.orphans() == (0, 0) and rt.device_bytes() == held


# ----------------------------------------------------------------------------------------------------- 8. LOD-cut image
@pytest.mark.parametrize("size,bd,depth", LOD_CASES)
def test_lod_cut_image(rt, size, bd, depth):
    what = f"{size}/{bd} depth {depth}"
    flat = lod_image(size, bd, depth)
    rt.upload(flat)  # a plain image: no MIPs set
    pos = positions(size)
    values = rt.get(pos)
    nodes, bricks = rt.compact()
    got = rt.download()
    G.assert_same_image(got, model_compact(flat), what)
    assert (nodes, bricks) == (flat.desc.node_count - got.desc.node_count, flat.desc.brick_count - got.desc.brick_count)
    assert bricks > 0, f"{what}: the MIP bricks leave"
    assert np.array_equal(rt.get(pos), values), f"{what}: get changed"


def test_compacting_an_empty_upload(rt):
    """A zero-grid image: one Nothing node, no bricks; allocations of zero bricks work."""
    zero = FlatTree.from_dense(G.make_grid("zero", SIZE), SIZE, BD)
    rt.upload(zero)
    assert rt.compact() == (0, 0)
    G.assert_same_image(rt.download(), zero, "the zero grid")
