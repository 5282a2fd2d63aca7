"""Voxel removal under a stream (host-only views, ctx=None): after any mix of inserts, clear and clear_at_lod, once
upload_all() reports nothing pending the view traces exactly like the edited tree (include/vhx_stream.h, "Tree
changes"). The reference's handle_tree_updates barely considers clears (src/raytracing/bevy/streaming/mod.rs:35-286);
the contract and the deviations are written down in voxelhex_amd/csrc/stream.cpp and docs/DESIGN_LOG.md.
"""
import numpy as np
import pytest

import voxelhex_amd as vhx
from voxelhex_amd import _native as N
from tests.test_gpu_parity import assert_same
from tests.test_streaming import FIELDS, _rays_in_box, _tree, _view_arrays

CONFIGS = [(32, 2), (64, 4), (128, 8)]


def rays(size, seed, n=5000):
    S = float(size)
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.5 * S, 1.5 * S, (n, 3)).astype(np.float32)
    tgt = rng.uniform(0, S, (n, 3)).astype(np.float32)
    d = tgt - o
    return o, (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(np.float32)


def clearing_edit(t, rng, size, bd):
    """Inserts into empty space, single-voxel clears, a clear that empties one brick, a clear that frees a whole
    subtree (a lowest node with its 64 bricks, 4 * brick_dim wide) and an unaligned clear inside a brick. The scene
    (lattice + cube, tests/test_streaming.py) is solid where any coordinate is below size/4 or all are above size/2."""
    node = 4 * bd
    for _ in range(30):
        x, y, z = (int(v) for v in rng.integers(0, size, 3))
        t.insert((x, y, z), vhx.Albedo(int(rng.integers(1, 255)), 40, 200, 255))
    for _ in range(40):
        x, y, z = (int(v) for v in rng.integers(0, size, 3))
        t.clear((x, y, z))
    # one brick, in the lattice (x below size/4)
    x, y, z = (int(v) // bd * bd for v in rng.integers(0, size // 4, 3))
    t.clear_at_lod((x, y, z), bd)
    # whole lowest nodes of the solid cube (two on its faces) and of the lattice
    for face in range(2):
        c = [int(v) // node * node for v in rng.integers(size // 2, size, 3)]
        c[int(rng.integers(3))] = size // 2 if face == 0 else size - node
        t.clear_at_lod(tuple(c), node)
    for _ in range(2):
        c = [int(v) // node * node for v in rng.integers(0, size, 3)]
        c[int(rng.integers(3))] = 0
        t.clear_at_lod(tuple(c), node)
    if bd > 1:  # inside one brick, off its grid
        x, y, z = (int(v) // bd * bd + 1 for v in rng.integers(0, size, 3))
        t.clear_at_lod((x, y, z), bd - 1)


def settled_view_equals_tree(oracle, t, s, o, d, what):
    stats, frames, _ = s.upload_all()
    assert stats["pending"] == 0 and frames >= 1, what
    full = oracle.trace_rays(t.flatten(), o, d, fields=FIELDS)
    assert_same(oracle.trace_rays(s.view(), o, d, fields=FIELDS), full, what)
    return full, stats


@pytest.mark.parametrize("size,bd", CONFIGS)
def test_clears_propagate_into_the_stream(oracle, size, bd):
    t = _tree(size, bd)
    S = float(size)
    s = vhx.StreamingView(t, None, (S / 2, S / 2, S / 2), 2 * S)
    s.upload_all()
    o, d = rays(size, size + bd)
    rng = np.random.default_rng(size * bd)
    for rnd in range(3):
        before = oracle.trace_rays(t.flatten(), o, d, fields=FIELDS)
        nodes_before = len(t.flatten().node_type)
        clearing_edit(t, rng, size, bd)
        assert len(t.flatten().node_type) != nodes_before or rnd > 0  # whole nodes went (or came)
        full, _ = settled_view_equals_tree(oracle, t, s, o, d, f"cleared tree, round {rnd}")
        # conditions of the comparison, on the oracle alone: the edits are visible, and enough rays hit
        assert (before["value"] != full["value"]).sum() >= 200, (before["value"] != full["value"]).sum()
        assert (full["value"] != N.VHX_EMPTY).sum() >= 500
    s.close()


@pytest.mark.parametrize("size,bd", CONFIGS)
def test_clears_while_the_view_is_still_filling(oracle, size, bd):
    """Clears made three frames into the stream: brick requests queued for bricks that are emptied, and for nodes that
    are freed, before their turn must not attach unwritten slots."""
    t = _tree(size, bd)
    S = float(size)
    s = vhx.StreamingView(t, None, (S / 2, S / 2, S / 2), S)
    s.set_rates(8, 32, 10)
    for _ in range(3):
        s.upload()
    rng = np.random.default_rng(bd)
    lo, hi = np.full(3, 1.0), np.full(3, S - 1)
    for rnd in range(2):
        clearing_edit(t, rng, size, bd)
        o, d = _rays_in_box(rng, lo, hi, 5000)
        full, _ = settled_view_equals_tree(oracle, t, s, o, d, f"filling view, round {rnd}")
        assert (full["value"] != N.VHX_EMPTY).sum() >= 500
    s.close()


@pytest.mark.parametrize("size,bd", CONFIGS)
def test_freed_keys_reused_before_the_next_upload(oracle, size, bd):
    """A subtree is cleared and new voxels are inserted elsewhere before the stream sees either: the pool hands the
    freed keys to the new nodes, so the queued clear's stack names keys that are other nodes by now."""
    t = _tree(size, bd)
    S = float(size)
    s = vhx.StreamingView(t, None, (S / 2, S / 2, S / 2), 2 * S)
    s.upload_all()
    o, d = rays(size, 3 * size + bd)
    before = oracle.trace_rays(t.flatten(), o, d, fields=FIELDS)
    node = 4 * bd
    lo = size // 2
    freed = set()
    for c in [(lo, lo, lo), (lo + node, lo, lo), (lo, lo + node, lo), (0, 0, 0), (0, node, 0), (node, 0, 0)]:
        info = t.node_info([v + 0.5 for v in c])
        assert info["content"] != "Internal"  # a lowest node, removed whole
        freed.add(info["key"])
        t.clear_at_lod(c, node)
        assert t.node_info([v + 0.5 for v in c])["key"] == 0  # only the root is left there
    # new nodes in space that was empty in the scene (one coordinate in [size/4, size/2), none below size/4)
    q = size // 4
    reused = set()
    for c in [(q, q, q), (q + node, q, q), (q, q + node, q), (q, q, q + node)]:
        assert t.node_info([v + 0.5 for v in c])["key"] == 0
        t.insert_at_lod(c, bd, vhx.Albedo(200, 100, 50, 255))
        t.insert((c[0] + bd, c[1] + 1, c[2]), vhx.Albedo(20, 220, 50, 255))
        reused.add(t.node_info([v + 0.5 for v in c])["key"])
    assert reused & freed, (reused, freed)  # the pool did hand freed keys out again
    full, _ = settled_view_equals_tree(oracle, t, s, o, d, "keys reused")
    assert (before["value"] != full["value"]).sum() >= 200
    assert (full["value"] != N.VHX_EMPTY).sum() >= 500
    s.close()


@pytest.mark.parametrize("size,bd", CONFIGS)
def test_insert_clear_cycles_do_not_grow_the_view(oracle, size, bd):
    t = _tree(size, bd)
    S = float(size)
    s = vhx.StreamingView(t, None, (S / 2, S / 2, S / 2), 2 * S)
    s.upload_all()
    o, d = rays(size, 7)
    q = size // 4  # empty space of the scene
    block = 4 * bd
    caps = []
    for cycle in range(20):
        t.insert_at_lod((q, q, q), block, vhx.Albedo(9, 90, 250, 255))
        for k in range(block):  # several bricks' worth of structure inside the block
            t.insert((q + k, q + (k * 3) % block, q + (k * 5) % block), vhx.Albedo(250, 10 + k, 10, 255))
        stats, _, _ = s.upload_all()
        assert stats["pending"] == 0
        t.clear_at_lod((q, q, q), block)
        stats, _, _ = s.upload_all()
        assert stats["pending"] == 0
        caps.append((stats["nodes_in_view"], stats["bricks_in_view"], stats["nodes_resident"], stats["bricks_resident"]))
    assert caps[19][:2] == caps[1][:2], caps
    assert caps[19][2:] == caps[1][2:], caps  # nothing stays resident for what was cleared
    settled_view_equals_tree(oracle, t, s, o, d, "after 20 cycles")
    s.close()


@pytest.mark.parametrize("batch", [2, 5])
def test_batched_uploads_equal_single_uploads_with_clears(batch):
    size, bd, S = 64, 4, 64.0
    ta, tb = _tree(size, bd), _tree(size, bd)
    a = vhx.StreamingView(ta, None, (S / 2, S / 2, S / 2), S / 4)
    b = vhx.StreamingView(tb, None, (S / 2, S / 2, S / 2), S / 4)
    for s in (a, b):
        s.set_rates(8, 32, 10)
    rng_a, rng_b = np.random.default_rng(5), np.random.default_rng(5)
    for step in range(12):
        if step in (3, 5, 9):
            clearing_edit(ta, rng_a, size, bd)
            clearing_edit(tb, rng_b, size, bd)
        if step == 6:
            for s in (a, b):
                s.set_viewport((0.6 * S, 0.5 * S, 0.5 * S), S)
        _, grow_a = a.upload(frames=batch)
        grow_b = False
        for _ in range(batch):
            _, g = b.upload()
            grow_b = grow_b or g
            if g:
                break
        assert grow_a == grow_b, step
        if grow_a:
            a.resize()
            b.resize()
        va, vb = _view_arrays(a), _view_arrays(b)
        for k in va:
            assert np.array_equal(va[k], vb[k]), f"batch {batch} step {step}: {k} differs"
    a.close()
    b.close()


def test_streamed_mips_follow_clears(oracle):
    """A MIP-enabled stream after clears: the region renders like the tree with the mirror's node MIPs (as
    test_streamed_mips_stand_in_outside_the_region compares), and the MIPs still
    stand in outside it."""
    size, bd = 64, 4
    t = _tree(size, bd)
    t.albedo_mip_map_resampling_strategy().switch_albedo_mip_maps(True)
    center, dist = (24.0, 20.0, 28.0), 32.0
    s = vhx.StreamingView(t, None, center, dist)
    s.set_rates(16, 64, 10)
    assert s.upload_all()[0]["pending"] == 0
    rng = np.random.default_rng(13)
    lo, hi = np.array([11.0, 7.0, 15.0]), np.array([37.0, 33.0, 41.0])  # 3 inside the region
    oi, di = _rays_in_box(rng, lo, hi, 5000)
    before = oracle.trace_rays(t.flatten(), oi, di, fields=FIELDS)
    for c in [(16, 0, 16), (0, 16, 32), (32, 16, 0)]:
        t.clear_at_lod(c, 16)  # whole lowest nodes of the lattice that reach into the region
    for _ in range(150):
        x, y, z = (int(v) for v in rng.integers(6, 42, 3))
        t.clear((x, y, z))
    t.clear_at_lod((12, 20, 28), 4)  # one brick
    assert s.upload_all()[0]["pending"] == 0
    mips = s.node_mips()
    with oracle.node_mips(mips):
        lod_in = oracle.trace_rays(s.view(), oi, di, fields=FIELDS)
    full = oracle.trace_rays(t.flatten(), oi, di, fields=FIELDS)
    inside = (full["value"] != N.VHX_EMPTY) & np.all((full["impact"] >= lo) & (full["impact"] <= hi), axis=1)
    assert inside.sum() >= 500
    assert (before["value"] != full["value"]).sum() >= 200
    assert_same({k: v[inside] for k, v in lod_in.items()}, {k: v[inside] for k, v in full.items()}, "region, MIPs")
    # rays leaving the region still find stand-ins (which nodes stay resident out there depends on the stream's
    # history, so only the region is compared with the tree)
    oo, do = _rays_in_box(rng, np.zeros(3), np.full(3, float(size)), 5000)
    base = oracle.trace_rays(s.view(), oo, do, fields=("value",))
    with oracle.node_mips(mips):
        lod = oracle.trace_rays(s.view(), oo, do, fields=("value",))
    assert ((lod["value"] != N.VHX_EMPTY) & (base["value"] == N.VHX_EMPTY)).sum() > 100
    s.close()
