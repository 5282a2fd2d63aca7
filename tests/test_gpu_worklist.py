"""The worklist of a batch's pass 0 (vhx_ctx::skyblocks; k_classify_blocks, k_emit_worklist): the launch's first
workgroups trace the tree blocks in the order of the lists, the next ones write a sky block's miss records with one
wave, the list order's padding ends at once, and the compaction covers the tree blocks' lists only.

Every frame of every batch must equal trace_primary of the same camera alone (the lone frame's kernel, which knows no
worklist) bit for bit in all seven planes. The output arrays are one row longer than the frame and pre-filled with a
sentinel: no word inside the frame may keep it, every word past the frame must.

Which path a schedule takes: the default, finter=0, qstate=1 and every xcdg take the worklist; p0lists=0, qorder=0 and
a single pass (budgets=) list nothing in list order and skyblocks=0 switches it off: every block takes the full path."""
import numpy as np
import pytest

import voxelhex_amd as vhx
from tests._skycams import aimed_camera
from voxelhex_amd import _native as N

pytestmark = pytest.mark.gpu

FIELDS = ("value", "cell", "voxel", "impact", "normal", "depth", "rgba")
WORDS = {"voxel": 3, "impact": 3, "normal": 3}
FLOATS = ("impact", "normal", "depth")
SENTINEL = 0x5EA7C0DE  # no index, colour or coordinate of these scenes
SIZES = [(200, 120), (64, 64), (1, 1)]  # no multiple of 16 or 64; whole blocks; one partial block
SCENES = [64, 256]

_flat, _rt, _lone = {}, {}, {}


def flat_of(S):
    if S not in _flat:
        _flat[S] = vhx.FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, S, 4)
    return _flat[S]


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for rt in _rt.values():
        rt.close()
    _rt.clear()


def raytracer(S):
    """One default-schedule context per scene, shared by the cases (and the source of every lone reference)."""
    if S not in _rt:
        _rt[S] = vhx.Raytracer(0)
        _rt[S].upload(flat_of(S))
    return _rt[S]


def lone(S, cam):
    """trace_primary of the camera alone, once per (scene, camera)."""
    key = (S, bytes(cam))
    if key not in _lone:
        r = raytracer(S).trace_primary(cam, fields=FIELDS)
        _lone[key] = {f: r[f].view(np.uint32).reshape(-1).copy() for f in FIELDS}
    return _lone[key]


def camera(kind, S, W, H, k=0):
    c = (S / 2,) * 3
    if kind == "mixed":  # the tree in the middle of the frame, sky around it
        return vhx.glass_camera(S, W, H, angle=40.0 + 0.3 * k, target=c)
    if kind == "away":  # no pixel reaches the tree: ntree = 0
        return vhx.glass_camera(S, W, H, angle=40.0 + 0.3 * k, target=(S * 4.0, S * 6.0, -S * 4.0))
    if kind == "inside":  # every pixel starts inside the root cube: nsky = 0
        return aimed_camera(W, H, (S / 2 + 0.25 * k, S / 2, S / 2), (S * 2.0, -S, S * 3.0))
    if kind == "plane":  # the origin on the cube's top plane, looking along and down
        return aimed_camera(W, H, (S / 4 + 0.25 * k, float(S), S / 4), (S * 1.0, S * 0.5, S * 1.0))
    raise ValueError(kind)


def new_outs(W, H):
    """All seven planes, one row longer than the frame, every word the sentinel."""
    import torch
    n = W * (H + 1)
    outs = {}
    for f in FIELDS:
        a = torch.full((n * WORDS.get(f, 1),), SENTINEL, dtype=torch.int32, device="cuda")
        outs[f] = a.view(torch.float32) if f in FLOATS else a
    return outs


def words(out):
    return {f: out[f].cpu().numpy().view(np.uint32).reshape(-1) for f in FIELDS}


def compare(S, cams, outs, what):
    for k, (cam, out) in enumerate(zip(cams, outs)):
        ref = lone(S, cam)
        got = words(out)
        for f in FIELDS:
            n = cam.width * cam.height * WORDS.get(f, 1)
            bad = int(np.count_nonzero(got[f][:n] != ref[f]))
            assert bad == 0, f"{what}: frame {k} field {f} differs from the lone frame at {bad} words"
            assert not (got[f][:n] == SENTINEL).any(), f"{what}: frame {k} field {f}: a word inside the frame was not written"
            assert (got[f][n:] == SENTINEL).all(), f"{what}: frame {k} field {f}: a word past the frame was written"


def run_batch(rt, S, cams, what):
    import torch
    W, H = cams[0].width, cams[0].height
    outs = [new_outs(W, H) for _ in cams]
    torch.cuda.synchronize()  # the fills run on torch's stream, the batch on the context's
    rt.trace_primary_batch(cams, outs)
    rt.sync()
    compare(S, cams, outs, what)
    return outs


@pytest.mark.parametrize("kind", ["mixed", "away", "inside", "plane"])
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("S", SCENES)
def test_cameras(S, W, H, kind):
    cams = [camera(kind, S, W, H, k) for k in range(2)]
    outs = run_batch(raytracer(S), S, cams, f"{S}^3 {W}x{H} {kind}")
    hit = words(outs[0])["value"][:W * H] != N.VHX_EMPTY
    if kind == "away":
        assert not hit.any()
    if kind == "mixed" and W == 200:
        assert hit.any() and not hit.all()


def test_mixed_view_against_the_oracle(oracle):
    S, W, H = 64, 200, 120
    cams = [camera("mixed", S, W, H, k) for k in range(2)]
    outs = run_batch(raytracer(S), S, cams, "oracle")
    for cam, out in zip(cams, outs):
        ref = oracle.trace_primary(flat_of(S), cam, 0, 0, W, H, fields=FIELDS)
        got = words(out)
        for f in FIELDS:
            n = W * H * WORDS.get(f, 1)
            assert np.array_equal(got[f][:n], ref[f].view(np.uint32).reshape(-1)), f


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("S", SCENES)
def test_batches_of_distinct_cameras(S, n):
    kinds = ["mixed", "plane", "mixed", "inside", "mixed", "mixed", "plane"]
    cams = [camera(kinds[k], S, 200, 120, k) for k in range(n)]
    run_batch(raytracer(S), S, cams, f"{S}^3 batch of {n}")


@pytest.mark.parametrize("at", [0, 3, 6])
def test_one_sky_frame_among_tree_frames(at):
    S = 64
    cams = [camera("away" if k == at else "mixed", S, 200, 120, k) for k in range(7)]
    run_batch(raytracer(S), S, cams, f"sky frame at {at}")


@pytest.mark.parametrize("tune", ["finter=0", "p0lists=0", "skyblocks=0", "qstate=1", "xcdg=0", "xcdg=3", "xcdg=1",
                                  "qorder=0", "budgets=", "budgets=8,24,72"])
def test_schedules(tune):
    S = 64
    rt = vhx.Raytracer(0, tune=tune)
    try:
        rt.upload(flat_of(S))
        for W, H in SIZES:
            kinds = ["mixed", "away", "inside", "plane", "mixed"]
            run_batch(rt, S, [camera(kinds[k], S, W, H, k) for k in range(5)], f"{tune} {W}x{H}")
    finally:
        rt.close()


def _orbit(ctxs, S, W, H, batches, per):
    """Batches back to back on each context into that context's one set of output arrays, a different camera every
    batch, no host wait in between; after each batch a copy of its outputs is taken on the context's stream. A
    worklist rewritten by the next batch while this batch's pass 0 still read it would show in the copy."""
    import torch
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.ExternalStream(rt.stream(), device=dev) for rt in ctxs]
    outs = [[new_outs(W, H) for _ in range(per)] for _ in ctxs]
    torch.cuda.synchronize()
    cams, copies = {}, {}
    for b in range(batches):
        for i, rt in enumerate(ctxs):
            kind = ["mixed", "away", "plane", "inside", "mixed"][(b + i) % 5]
            cams[i, b] = [camera(kind, S, W, H, 10 * b + 3 * i + k) for k in range(per)]
            rt.trace_primary_batch(cams[i, b], outs[i])
            with torch.cuda.stream(streams[i]):
                copies[i, b] = [{f: o[f].clone() for f in FIELDS} for o in outs[i]]
    for rt in ctxs:
        rt.sync()
    torch.cuda.synchronize()
    for (i, b), got in copies.items():
        compare(S, cams[i, b], got, f"context {i} batch {b}")


@pytest.mark.parametrize("S", SCENES)
def test_five_batches_back_to_back_on_one_context(S):
    owner = vhx.Raytracer(0)
    try:
        owner.upload(flat_of(S))
        _orbit([owner], S, 200, 120, 5, 3)
    finally:
        owner.close()


def test_five_batches_back_to_back_on_three_contexts():
    S = 64
    owner = vhx.Raytracer(0)
    try:
        owner.upload(flat_of(S))
        others = [owner.shared(), owner.shared()]
        try:
            _orbit([owner] + others, S, 200, 120, 5, 3)
        finally:
            for o in others:
                o.close()
    finally:
        owner.close()
