"""The conditions on the inputs of tests/test_gpu_mip_parity.py (tests/_mip_cases.py), so that no GPU comparison there
passes vacuously. All of them are properties of the oracle's output alone, over the 6000 rays of each case, per view:

  * no output field holds a NaN (which makes pure bit equality the right bar for the GPU);
  * the view's node MIPs change the value or the depth bits of at least 1000 rays for a flatten_lod cut above the
    canonical leaf depth and for a "both"/sampled hand-cut, and of at least 100 rays for every other hand-cut (the
    stand-ins are traced, not merely set). The bounds are caps on what a test may leave out: a view that misses one
    gets a larger dropped share, never a lower bound. The flatten_lod cut at the canonical leaf depth, where a tree has
    a few nodes below it, is a view of the GPU test too, but lacks so few nodes that no bound is put on it;
  * a full image traces the same with its MIPs on and off, in every field;
  * the probing nodes of a mixed view hold a Solid descriptor and, where there are at least two of them, a VHX_EMPTY
    one (a view with a single probing node has one descriptor to give: tests/_mip_cases.py)."""
import numpy as np
import pytest

from voxelhex_amd import _native as N
from tests import _mip_cases as M

FLOATS = ("impact", "normal", "depth")


@pytest.mark.parametrize("seed,size,bd", M.CASES)
def test_views_trace_their_stand_ins(oracle, seed, size, bd):
    c = M.case(seed, size, bd)
    views = M.mip_views(seed, size, bd)
    names = [v.name for v in views]
    assert len(set(names)) == len(names)
    assert views[0].name == "lod0" and sum(v.full for v in views) == 1
    root_is_leaf = c.full.node_type[0] != N.VHX_NODE_INTERNAL
    want = {f"{cut}/{m}" for cut in M.CUTS for m in ("sampled", "mixed") if not (cut == "internal" and root_is_leaf)}
    assert want <= set(names), sorted(want - set(names))
    if not root_is_leaf:
        assert not views[0].full, "no proper flatten_lod cut"
    for v in views:
        what = f"seed {seed} {size}/{bd} {v.name}"
        with oracle.node_mips(v.node_mips):
            on = oracle.trace_rays(v.image, c.origins, c.directions, fields=M.FIELDS)
        off = oracle.trace_rays(v.image, c.origins, c.directions, fields=M.FIELDS)
        for f in FLOATS:
            assert not np.isnan(on[f]).any() and not np.isnan(off[f]).any(), f"{what}: NaN in {f}"
        changed = int(M.changed_rays(on, off).sum())
        probing = M.probing_nodes(v.image)
        print(f"{what}: {v.image.node_type.size} nodes, {probing.size} probing, {changed} of {M.RAYS} rays changed")
        if v.full:
            assert probing.size == 0, what
            M.assert_bits(on, off, f"{what}: MIPs on against MIPs off")
            continue
        assert probing.size > 0, what
        if v.cut == "lod" and v.depth >= M.leaf_depth(size, bd):
            # the few nodes insert_at_lod made below the canonical leaf depth are cut: not full, and no bound to hold
            # either (seed 3 lod2 lacks 8 of 1394 nodes); the GPU comparison takes it as one more view
            assert v.depth == M.leaf_depth(size, bd) and v.image.node_type.size > 0.95 * c.full.node_type.size, what
            continue
        bound = 1000 if v.cut == "lod" or (v.cut == "both" and not v.mixed) else 100
        assert changed >= bound, f"{what}: the node MIPs change {changed} rays, fewer than {bound}"
        # the case's 96x64 frame: the same cap of 100 on every view, so trace_primary and the shadow rays see stand-ins
        with oracle.node_mips(v.node_mips):
            f_on = oracle.trace_primary(v.image, c.camera, 0, 0, M.W, M.H, fields=M.FIELDS)
        f_off = oracle.trace_primary(v.image, c.camera, 0, 0, M.W, M.H, fields=M.FIELDS)
        for f in FLOATS:
            assert not np.isnan(f_on[f]).any(), f"{what}: NaN in the frame's {f}"
        pixels = int(M.changed_rays(f_on, f_off).sum())
        assert pixels >= 100, f"{what}: the node MIPs change {pixels} pixels of the frame, fewer than 100"
        if v.mixed:
            desc = np.asarray(v.node_mips)[probing]
            solid = (desc != N.VHX_EMPTY) & ((desc & N.VHX_SOLID_BIT) != 0)
            assert solid.any(), f"{what}: no Solid descriptor on a probing node"
            assert (desc[solid] & 0x7FFFFFFF).max() < v.image.solid_values.size
            if probing.size >= 2:
                assert (desc == N.VHX_EMPTY).any(), f"{what}: no VHX_EMPTY descriptor on a probing node"
            if probing.size >= 4:
                assert ((desc & N.VHX_SOLID_BIT) == 0).any(), f"{what}: no Parted descriptor on a probing node"


def test_every_brick_dim_has_views_of_every_kind():
    """Across the cases, every brick_dim the kernels are built for has a proper flatten_lod cut, a stand-in under an
    Internal node, one under a Leaf node, and Solid and VHX_EMPTY descriptors on probing nodes."""
    seen = {}
    for seed, size, bd in M.CASES:
        s = seen.setdefault(bd, set())
        for v in M.mip_views(seed, size, bd):
            if v.full:
                continue
            if v.cut != "lod" or v.depth < M.leaf_depth(size, bd):
                s.add(v.cut)
            if v.mixed:
                desc = np.asarray(v.node_mips)[M.probing_nodes(v.image)]
                if (desc == N.VHX_EMPTY).any():
                    s.add("empty")
                if ((desc != N.VHX_EMPTY) & ((desc & N.VHX_SOLID_BIT) != 0)).any():
                    s.add("solid")
    assert sorted(seen) == [1, 2, 4, 8, 16, 32]
    for bd, s in seen.items():
        assert {"lod", "internal", "leaf", "both", "empty", "solid"} <= s, (bd, s)


def test_assert_bits_has_no_tolerance():
    a = {"depth": np.array([1.0, 2.0], np.float32), "value": np.array([3, 4], np.uint32)}
    M.assert_bits(a, {k: v.copy() for k, v in a.items()})
    b = {"depth": np.array([1.0, np.nextafter(np.float32(2.0), np.float32(3.0))], np.float32), "value": a["value"]}
    with pytest.raises(AssertionError, match="depth differs in bits at 1 of 2"):
        M.assert_bits(b, a)
    with pytest.raises(AssertionError, match="depth"):
        M.assert_bits({"depth": np.array([-0.0, 2.0], np.float32)}, {"depth": np.array([0.0, 2.0], np.float32)})
