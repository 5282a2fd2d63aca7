"""Traces with a shadow light (vhx_set_shadow_light) across trees, schedules, layouts and orderings.

include/vhx.h promises that a frame traced with a light equals vhx_trace_primary followed by vhx_trace_shadows bit for
bit, that tuning keys never change results, and that a trace writes only the entries it owns (tile padding and, in a
rank-sharded framebuffer, other calls' pixels are treated as without a light). tests/test_gpu_fused_shadows.py checks
the first on the lattice cube under a handful of schedules; this file adds

  A  the oracle's frame (primary rays, then shadow rays) on fuzz trees with Solid bricks, UniformLeaf nodes and
     data-only voxels, every brick_dim, for the separate path, the shadow batch and the fused frame;
  B  every scheduling key of the primary-ray matrix with a light, the segment node sort (qsort) among them, over a
     single frame, a batch of frames, a batch of tile sets and a lone tile-layout frame;
  C  ownership: tile padding and foreign pixels keep the caller's bytes in all six buffers, shards that fill one set
     of buffers darken every pixel once;
  D  refusals of overlapping outputs before anything is written, on either schedule and in batches;
  E  shared contexts tracing with a light while other frames are in flight.

Frames are 200 x 136 (ragged against 16, 24, 32 and 64), trees at most 256^3. Fused against separate is exact equality
in every field; GPU against oracle uses tests/test_gpu_parity.py::assert_same for the primary fields and exact equality
for `shadowed` and the darkened `rgba`."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from tests._skycams import aimed_camera
from tests._tilemask import tile_mask
from tests.test_gpu_fused_shadows import _host, _outs, _separate
from tests.test_gpu_fuzz import random_tree
from tests.test_gpu_parity import assert_same
from voxelhex_amd import _native as N

pytestmark = pytest.mark.gpu

W, H = 200, 136
SIX = ("value", "impact", "normal", "depth", "rgba", "shadowed")
SENT = 0x5A5A5A5A  # no field of any frame here holds it: not a palette value, a flag, a colour (alpha 0x5A) or a depth
E = N.VHX_EMPTY
DATA_ONLY_RGBA = 0xFF000000  # r, g, b = 0, a = 255: a voxel without an albedo


# ------------------------------------------------------------------------------------------------------- helpers
def _sent_outs(n):
    """The six device buffers of n entries, every word the sentinel."""
    import torch
    i3 = lambda: torch.full((n, 3), SENT, dtype=torch.int32, device="cuda")
    i1 = lambda: torch.full((n,), SENT, dtype=torch.int32, device="cuda")
    return {"value": i1(), "impact": i3().view(torch.float32), "normal": i3().view(torch.float32),
            "depth": i1().view(torch.float32), "rgba": i1(), "shadowed": i1()}


def _six(o):
    """Host copies of the six fields as uint32 words, one row per entry."""
    out = {}
    for k in SIX:
        a = o[k].cpu().numpy() if hasattr(o[k], "cpu") else np.asarray(o[k])
        out[k] = np.ascontiguousarray(a).view(np.uint32).reshape(a.shape[0], -1)
    return out


def _equal_six(got, ref, what):
    for k in SIX:
        bad = int(np.count_nonzero((got[k] != ref[k]).any(axis=1)))
        assert bad == 0, f"{what}: field {k} differs at {bad} entries"


def _separate_six(rt, cam, light):
    """vhx_trace_primary, then vhx_trace_shadows, of a whole frame (no light set on rt): all six fields."""
    import torch
    o = _outs(cam.width * cam.height)
    torch.cuda.synchronize()
    rt.trace_primary(cam, out=o)
    rt.trace_shadows(light, o, shadowed=o["shadowed"])
    rt.sync()
    return _six(o)


def _check_owned(got, ref, owned, pixel, what, pad=SENT):
    """got: an output in the tile layout (pixel = each entry's frame index) or the framebuffer layout (pixel None);
    the entries outside `owned` hold `pad` in every word of every field, the owned ones the reference frame's."""
    assert owned.any() and not owned.all(), f"{what}: the case needs owned entries and others"
    for k in SIX:
        assert got[k].shape[0] == owned.size, (what, k, got[k].shape, owned.size)
        want = ref[k][pixel[owned]] if pixel is not None else ref[k][owned]
        bad = int(np.count_nonzero((got[k][owned] != want).any(axis=1)))
        assert bad == 0, f"{what}: field {k} differs from the reference at {bad} owned entries"
        bad = int(np.count_nonzero((got[k][~owned] != pad).any(axis=1)))
        assert bad == 0, f"{what}: field {k} was written at {bad} entries the trace does not own"


def _tile_entries(T, start, stride):
    return tile_mask(W, H, T, start, stride, N.VHX_LAYOUT_TILES)[0].size


# ------------------------------------------------------------------------------- A: the oracle on trees never seen
# (seed, size, brick_dim, camera angle): random_tree of an even seed is simplified. Chosen on the CPU with the oracle so
# that every condition below holds for the reference alone; the counts the oracle gives for the first camera:
#   seed size bd    hits shadowed  lit  in Solid bricks  data-only
#      0   16  1   11716    11618   98            11716       9044
#      0   32  2    9049     8487  562              269       5260
#      0   64  4    7225     6750  475             1224       3155
#      1   64  4    5487     4512  975               78       2107   (not simplified: Solid bricks from insert_at_lod)
#      0  128  8    4059     3293  766             1333       1005
#      0  256 16    2497     1763  734             1381        351
#    164  128 32    2447     1969  478              491        749   (an even seed whose tree holds a Solid 32^3 brick)
ORACLE_CASES = [(0, 16, 1, 40.0), (0, 32, 2, 40.0), (0, 64, 4, 40.0), (1, 64, 4, 40.0), (0, 128, 8, 40.0),
                (0, 256, 16, 40.0), (164, 128, 32, 41.5)]
_oracle_cache = {}


def _oracle_case(oracle, seed, size, bd, angle):
    """The tree, two cameras and the oracle's frame of each (primary rays, then shadow rays), once per module."""
    key = (seed, size, bd)
    if key not in _oracle_cache:
        flat = random_tree(seed, size, bd)[0].flatten()
        light = (float(size),) * 3
        cams = [vhx.glass_camera(size, W, H, angle=angle + 0.3 * k, radius=1.2 * size, target=(size / 2,) * 3)
                for k in range(2)]
        refs = []
        for cam in cams:
            p = oracle.trace_primary(flat, cam, 0, 0, W, H)
            s = oracle.trace_shadows(flat, light, p)
            refs.append({"primary": {k: p[k] for k in ("value", "impact", "normal", "depth")}, "cell": p["cell"],
                         "lit_rgba": p["rgba"], "shadowed": s["shadowed"], "rgba": s["rgba"]})
        _oracle_cache[key] = (flat, light, cams, refs)
    return _oracle_cache[key]


def _counts(ref):
    hit = ref["primary"]["value"] != E
    return {"shadowed": int((ref["shadowed"] == 1).sum()), "lit": int((hit & (ref["shadowed"] == 0)).sum()),
            "solid": int((hit & (ref["cell"] == E)).sum()),
            "data_only": int((hit & (ref["lit_rgba"] == DATA_ONLY_RGBA)).sum())}


def _check_vs_oracle(o, ref, what):
    got = {k: o[k].cpu().numpy() for k in SIX}
    got["value"] = got["value"].view(np.uint32)
    assert_same({k: got[k] for k in ref["primary"]}, ref["primary"], what)
    for k in ("shadowed", "rgba"):
        bad = int(np.count_nonzero(got[k].view(np.uint32) != ref[k]))
        assert bad == 0, f"{what}: {k} differs from the oracle at {bad} entries"


@pytest.mark.parametrize("seed,size,bd,angle", ORACLE_CASES)
def test_shadow_paths_vs_oracle_on_fuzz_trees(oracle, seed, size, bd, angle):
    """The separate path (single pass and a 1-step first budget), the shadow batch over two cameras and the fused
    frame (the default ladder and one that abandons rays at every step) against oracle.trace_primary followed by
    oracle.trace_shadows with the light at (size, size, size). The reference's counts are in ORACLE_CASES' table."""
    import torch
    flat, light, cams, refs = _oracle_case(oracle, seed, size, bd, angle)
    c = _counts(refs[0])
    assert c["shadowed"] > 20 and c["lit"] > 20 and c["solid"] > 0, c
    n = W * H
    rt = vhx.Raytracer(0)
    try:
        rt.upload(flat)
        for budgets in ((), (1, 3, 9)):
            rt.set_pass_budgets(budgets)
            o = _outs(n)
            torch.cuda.synchronize()
            rt.trace_primary(cams[0], out=o)
            rt.trace_shadows(light, o, shadowed=o["shadowed"])
            rt.sync()
            _check_vs_oracle(o, refs[0], f"seed {seed} {size}/{bd} separate, budgets {budgets}")
        rt.set_adaptive_schedule(True)
        outs = [_outs(n) for _ in cams]
        torch.cuda.synchronize()
        for cam, o in zip(cams, outs):
            rt.trace_primary(cam, out=o)
        rt.trace_shadows_batch(light, outs, [o["shadowed"] for o in outs])
        rt.sync()
        for k, o in enumerate(outs):
            _check_vs_oracle(o, refs[k], f"seed {seed} {size}/{bd} shadow batch, camera {k}")
    finally:
        rt.close()
    for tune in ("adaptive=0", "adaptive=0;budgets=1,3,7,15"):
        fus = vhx.Raytracer(0, tune=tune)
        try:
            fus.upload(flat)
            fus.set_shadow_light(light)
            o = _outs(n)
            torch.cuda.synchronize()
            fus.trace_primary(cams[0], out=o)
            fus.sync()
            _check_vs_oracle(o, refs[0], f"seed {seed} {size}/{bd} fused, tune {tune}")
        finally:
            fus.close()


def test_oracle_cases_hold_data_only_voxels(oracle):
    """Over the parametrisation above the reference hits voxels without an albedo (rgba 0, 0, 0, 255), lit and
    shadowed: the darkening of a data-only hit is part of what the cases compare."""
    total = 0
    for case in ORACLE_CASES:
        total += _counts(_oracle_case(oracle, *case)[3][0])["data_only"]
    assert total > 0


# ------------------------------------------------------------------------------- B: schedule independence with a light
TREES = ("fuzz64", "lattice256")
_trees, _refs = {}, {}


def _tree(name):
    if name not in _trees:
        _trees[name] = ((random_tree(0, 64, 4)[0].flatten(), 64) if name == "fuzz64" else
                        (vhx.FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, 256, 4), 256))
    return _trees[name]


def _cams(size):
    """Centred; the tree in a corner of a frame that is mostly sky (14 or 15 of its 117 16x16 blocks hold a hit);
    centred from a little further round."""
    S = float(size)
    return [vhx.glass_camera(size, W, H, target=(S / 2,) * 3),
            aimed_camera(W, H, (1.49 * S, 2.0 * S, -1.33 * S), (2.2 * S, 0.5 * S, 1.2 * S)),
            vhx.glass_camera(size, W, H, angle=40.3, target=(S / 2,) * 3)]


def _reference(name):
    """The separate path on a default context, per camera, once per module (never modified afterwards)."""
    if name not in _refs:
        flat, size = _tree(name)
        light = (float(size),) * 3
        rt = vhx.Raytracer(0)
        try:
            rt.upload(flat)
            refs = [_separate_six(rt, cam, light) for cam in _cams(size)]
        finally:
            rt.close()
        for r in refs:
            hit = r["value"][:, 0] != E
            assert (r["shadowed"][:, 0] == 1).sum() > 20 and (hit & (r["shadowed"][:, 0] == 0)).sum() > 20
            for a in r.values():
                a.setflags(write=False)
        _refs[name] = (flat, size, light, _cams(size), refs)
    return _refs[name]


def _trace_tiles(rt, cam, T, start, stride):
    import torch
    o = _sent_outs(_tile_entries(T, start, stride))
    torch.cuda.synchronize()
    rt.trace_primary(cam, tile_size=T, tile_start=start, tile_stride=stride, layout=N.VHX_LAYOUT_TILES, out=o)
    rt.sync()
    return _six(o)


def _trace_tiles_batch(rt, cams, T, starts, stride):
    import torch
    outs = [_sent_outs(_tile_entries(T, s, stride)) for s in starts]
    torch.cuda.synchronize()
    rt.trace_tiles_batch(cams, T, starts, stride, outs)
    rt.sync()
    return [_six(o) for o in outs]


def _check_tiles(got, ref, T, start, stride, what):
    owned, pixel = tile_mask(W, H, T, start, stride, N.VHX_LAYOUT_TILES)
    _check_owned(got, ref, owned, pixel, what)


# every entry but the last runs under "adaptive=0" (a lone frame on the frames-in-flight schedule, its shadows fused
# where pass 0 lists its rays); None is the lone frame's schedule
LIGHT_TUNES = ["qsort=256", "qsort=2048;budgets=1,3,7,15", "qsort=256;qsortp=2;budgets=2,9,30", "qsort=256;rpw=0,0;tw=7",
               "qorder=16", "qorder=m32z", "qorder=0", "resume=0", "save_from=1", "qblock=64;rpw=0,3;tw=100000",
               "qxcd=1", "qxcd_all=1;qwavesm=300", "sparse=64,64,64", "tlists=0", "finter=0", "finter=1", "skyblocks=0",
               "stage_slots=3", "sbudget=1;qsort=256", None]
TUNE_BUDGETS = {"qsort=2048;budgets=1,3,7,15": (1, 3, 7, 15), "qsort=256;qsortp=2;budgets=2,9,30": (2, 9, 30)}


@pytest.mark.parametrize("name", TREES)
@pytest.mark.parametrize("tune", LIGHT_TUNES)
def test_tuning_keys_never_change_a_lit_frame(tune, name):
    """A single frame, a batch of three frames, a batch of three tile sets and a lone tile-layout frame on a fresh
    context with the tune and a light: value, depth, rgba, shadowed, impact and normal equal the separate path's on a
    default context bit for bit (tile padding keeps the caller's bytes)."""
    import torch
    flat, size, light, cams, refs = _reference(name)
    spec = None if tune is None else "adaptive=0;" + tune
    n = W * H
    rt = vhx.Raytracer(0, tune=spec)
    try:
        rt.upload(flat)
        rt.set_shadow_light(light)
        for k in (0, 1):
            o = _outs(n)
            torch.cuda.synchronize()
            rt.trace_primary(cams[k], out=o)
            budgets, sched = rt.pass_budgets()
            rt.sync()
            _equal_six(_six(o), refs[k], f"{name} tune {tune} single frame, camera {k}")
            # the schedule the context ran is the intended one
            if tune is None:
                assert sched == "idle", (tune, sched)
            else:
                assert sched == "fixed", (tune, sched)
                assert budgets == TUNE_BUDGETS.get(tune, budgets) and len(budgets) >= 1, (tune, budgets)
        outs = [_outs(n) for _ in cams]
        torch.cuda.synchronize()
        rt.trace_primary_batch(cams, outs)
        rt.sync()
        for k, o in enumerate(outs):
            _equal_six(_six(o), refs[k], f"{name} tune {tune} batch frame {k}")
        starts, stride = (0, 1, 2), 3
        for k, got in enumerate(_trace_tiles_batch(rt, cams, 64, starts, stride)):
            _check_tiles(got, refs[k], 64, starts[k], stride, f"{name} tune {tune} tile set {k}")
        for k in (0, 1):
            for T, start, stride in ((64, 0, 1), (24, 1, 2)):
                _check_tiles(_trace_tiles(rt, cams[k], T, start, stride), refs[k], T, start, stride,
                             f"{name} tune {tune} lone tile frame T {T}, camera {k}")
    finally:
        rt.close()


# ------------------------------------------------------------------------------- C: ownership of entries with a light
@pytest.mark.parametrize("tune", [None, "adaptive=0"])
def test_lone_tile_frame_leaves_padding_untouched(tune):
    """Tile layout, device outputs, the lone frame on both schedules (the shadows after the primary rays, and fused):
    padding keeps the sentinel in all six buffers, owned entries equal the reference frame at their pixel, primary
    misses included (shadowed 0)."""
    flat, size, light, cams, refs = _reference("fuzz64")
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(flat)
        rt.set_shadow_light(light)
        for k in (0, 1):
            miss = refs[k]["value"][:, 0] == E
            assert miss.any() and (refs[k]["shadowed"][miss, 0] == 0).all()
            for T, start, stride in ((64, 0, 1), (64, 1, 3), (24, 0, 2), (32, 2, 3)):
                _check_tiles(_trace_tiles(rt, cams[k], T, start, stride), refs[k], T, start, stride,
                             f"tune {tune} camera {k} T {T} start {start} stride {stride}")
    finally:
        rt.close()


@pytest.mark.parametrize("tlists", [0, 1])
def test_tile_set_batch_leaves_padding_untouched(tlists):
    """The tile-set batch with pass 0 listing its rays (fused shadows) and writing flags (the shadows after it)."""
    flat, size, light, cams, refs = _reference("fuzz64")
    rt = vhx.Raytracer(0, tune=f"tlists={tlists}")
    try:
        rt.upload(flat)
        rt.set_shadow_light(light)
        for T, starts, stride in ((64, (0, 1, 2), 3), (24, (2, 0, 1), 3)):
            for k, got in enumerate(_trace_tiles_batch(rt, cams, T, starts, stride)):
                _check_tiles(got, refs[k], T, starts[k], stride, f"tlists {tlists} T {T} tile set {k}")
    finally:
        rt.close()


@pytest.mark.parametrize("tune", [None, "adaptive=0"])
def test_tile_padding_reads_zero_with_host_outputs(tune):
    """Tile layout, host outputs: padding reads back 0 in every field, `shadowed` included, whatever the arrays held."""
    flat, size, light, cams, refs = _reference("fuzz64")
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(flat)
        rt.set_shadow_light(light)
        for T, start, stride in ((64, 0, 1), (24, 1, 2)):
            owned, pixel = tile_mask(W, H, T, start, stride, N.VHX_LAYOUT_TILES)
            n = owned.size
            host = {"value": np.full(n, SENT, np.uint32), "impact": np.full((n, 3), SENT, np.uint32).view(np.float32),
                    "normal": np.full((n, 3), SENT, np.uint32).view(np.float32),
                    "depth": np.full(n, SENT, np.uint32).view(np.float32), "rgba": np.full(n, SENT, np.uint32),
                    "shadowed": np.full(n, SENT, np.uint32)}
            rt.trace_primary(cams[0], tile_size=T, tile_start=start, tile_stride=stride, layout=N.VHX_LAYOUT_TILES,
                             out=host)
            _check_owned(_six(host), refs[0], owned, pixel, f"host outputs, tune {tune}, T {T}", pad=0)
    finally:
        rt.close()


@pytest.mark.parametrize("budgets", [(1,), None])
def test_sharded_framebuffer_with_a_light(budgets):
    """Framebuffer layout, T = 32, R = 3 shard calls. Each into fresh buffers: the pixels of other shards' tiles keep
    the sentinel in all six buffers. One after another into one shared set of buffers: the whole-frame reference in
    every field -- no call touches, let alone darkens again, what another one wrote."""
    import torch
    flat, size, light, cams, refs = _reference("lattice256")
    T, R, n = 32, 3, W * H
    rt = vhx.Raytracer(0)
    try:
        rt.upload(flat)
        rt.set_shadow_light(light)
        if budgets is not None:
            rt.set_pass_budgets(budgets)
        for k in (0, 1):
            for r in range(R):
                o = _sent_outs(n)
                torch.cuda.synchronize()
                rt.trace_primary(cams[k], tile_size=T, tile_start=r, tile_stride=R, out=o)
                rt.sync()
                owned, _ = tile_mask(W, H, T, r, R, N.VHX_LAYOUT_FRAMEBUFFER)
                _check_owned(_six(o), refs[k], owned, None, f"budgets {budgets} camera {k} shard {r}")
            shared = _sent_outs(n)
            torch.cuda.synchronize()
            for r in range(R):
                rt.trace_primary(cams[k], tile_size=T, tile_start=r, tile_stride=R, out=shared)
            rt.sync()
            _equal_six(_six(shared), refs[k], f"budgets {budgets} camera {k}, {R} shards into one set of buffers")
    finally:
        rt.close()


# ------------------------------------------------------------------------------------------------------ D: refusals
def _alias_cases(n):
    """name -> a function that re-points one output of a sentinel set at another one's memory"""
    import torch

    def shadowed_is_value(o):
        o["shadowed"] = o["value"]

    def shadowed_in_impact(o):
        o["shadowed"] = o["impact"].view(-1)[5:5 + n].view(torch.int32)

    def rgba_is_normal(o):
        o["rgba"] = o["normal"].view(-1)[:n].view(torch.int32)

    def shadowed_is_rgba(o):
        o["shadowed"] = o["rgba"]

    return [shadowed_is_value, shadowed_in_impact, rgba_is_normal, shadowed_is_rgba]


def _all_sentinel(o):
    return all((o[k].cpu().numpy().view(np.uint32) == SENT).all() for k in o)


@pytest.mark.parametrize("tune", [None, "adaptive=0"])
def test_overlapping_outputs_are_refused_before_anything_is_written(tune):
    """With a light, vhx_trace_primary refuses shadowed or rgba over the hit records, and shadowed over rgba, on the
    lone frame's schedule and the fused one alike, and leaves every buffer as it was."""
    import torch
    flat, size, light, cams, refs = _reference("fuzz64")
    n = W * H
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(flat)
        rt.set_shadow_light(light)
        for alias in _alias_cases(n):
            o = _sent_outs(n)
            keep = dict(o)  # the buffer the alias drops from o is still checked
            alias(o)
            torch.cuda.synchronize()
            with pytest.raises(N.VhxError) as e:
                rt.trace_primary(cams[0], out=o)
            assert e.value.code == N.VHX_E_INVALID_ARG, alias.__name__
            rt.sync()
            torch.cuda.synchronize()
            assert _all_sentinel(keep), f"tune {tune} {alias.__name__}: a refused trace wrote an output"
        o = _sent_outs(n)  # and the context still traces
        torch.cuda.synchronize()
        rt.trace_primary(cams[0], out=o)
        rt.sync()
        _equal_six(_six(o), refs[0], f"tune {tune} after the refusals")
    finally:
        rt.close()


@pytest.mark.parametrize("tiles", [False, True])
def test_batches_refuse_overlapping_shadowed_arrays(tiles):
    """vhx_trace_primary_batch / vhx_trace_tiles_batch with a light: two frames sharing one shadowed array, a shadowed
    array over another frame's rgba, or over another frame's value, are refused and nothing is written; without a
    light, where shadowed is ignored, the same batches run."""
    import torch
    flat, size, light, cams, refs = _reference("fuzz64")
    T, starts, stride = 64, (0, 0), 1
    n = _tile_entries(T, 0, 1) if tiles else W * H

    def share_shadowed(outs):
        outs[1]["shadowed"] = outs[0]["shadowed"]

    def shadowed_over_next_rgba(outs):
        outs[0]["shadowed"] = outs[1]["rgba"]

    def shadowed_over_next_value(outs):
        outs[0]["shadowed"] = outs[1]["value"]

    def run(rt, outs):
        if tiles:
            rt.trace_tiles_batch(cams[:2], T, starts, stride, outs)
        else:
            rt.trace_primary_batch(cams[:2], outs)

    rt = vhx.Raytracer(0)
    try:
        rt.upload(flat)
        for alias in (share_shadowed, shadowed_over_next_rgba, shadowed_over_next_value):
            rt.set_shadow_light(light)
            outs = [_sent_outs(n) for _ in range(2)]
            keep = [dict(o) for o in outs]
            alias(outs)
            torch.cuda.synchronize()
            with pytest.raises(N.VhxError) as e:
                run(rt, outs)
            assert e.value.code == N.VHX_E_INVALID_ARG, alias.__name__
            rt.sync()
            assert all(_all_sentinel(o) for o in keep), f"{alias.__name__}: a refused batch wrote an output"
            # without a light the very same batch runs: the fields a light does not change are the reference's, and no
            # shadowed array, shared or not, is touched
            rt.set_shadow_light(None)
            run(rt, outs)
            rt.sync()
            for f in range(2):
                got = _six(keep[f])
                for k in ("value", "impact", "normal", "depth"):
                    if tiles:
                        owned, pixel = tile_mask(W, H, T, 0, 1, N.VHX_LAYOUT_TILES)
                        assert (got[k][owned] == refs[f][k][pixel[owned]]).all(), (alias.__name__, f, k)
                    else:
                        assert (got[k] == refs[f][k]).all(), (alias.__name__, f, k)
                assert (got["shadowed"] == SENT).all(), f"{alias.__name__}: shadowed written without a light"
    finally:
        rt.close()


# ------------------------------------------------------------------------------------ E: frames in flight with a light
def test_lit_frames_in_flight_on_shared_contexts():
    """An owner and three shared contexts, a light set on each, trace a camera each, submitted back to back on the
    adaptive schedule, for two rounds; every frame equals the separate path's. At least one context must have found a
    frame in flight (the frames-in-flight schedule, fused shadows) -- else the case tested only lone frames."""
    import torch
    flat, size = _tree("lattice256")
    light = (float(size),) * 3
    cams = [vhx.glass_camera(size, W, H, angle=40.0 + 0.4 * k, target=(size / 2,) * 3) for k in range(4)]
    sep = vhx.Raytracer(0)
    try:
        sep.upload(flat)
        refs = [_separate(sep, cam, light) for cam in cams]
    finally:
        sep.close()
    owner = vhx.Raytracer(0)
    ctxs = [owner]
    try:
        owner.upload(flat)
        ctxs += [owner.shared() for _ in range(3)]
        for r in ctxs:
            r.set_shadow_light(light)
        busy = 0
        for rnd in range(2):
            outs = [_outs(W * H) for _ in ctxs]
            torch.cuda.synchronize()
            order = [(f + rnd) % 4 for f in range(4)]  # round 1: every context another camera
            for r, ci, o in zip(ctxs, order, outs):
                r.trace_primary(cams[ci], out=o)
            busy += sum(r.pass_budgets()[1] == "busy" for r in ctxs)
            for r in ctxs:
                r.sync()
            for f, (ci, o) in enumerate(zip(order, outs)):
                got = _host(o)
                for k in got:
                    bad = int(np.count_nonzero(got[k] != refs[ci][k]))
                    assert bad == 0, f"round {rnd} context {f}: field {k} differs at {bad} entries"
    finally:
        for r in ctxs[1:]:
            r.close()
        owner.close()
    if busy == 0:
        pytest.skip("no context found a frame in flight: only the lone frame's schedule ran")
