"""Reading voxels back from the device tree (vhx_read_dense, vhx_get_voxels; DESIGN.md "Reading voxels back") on one
MI355X. A scene is generated as a dense int32 device tensor with torch operations (4 GiB at 1024^3) and built with
Raytracer.build_dense:
  bench        VHX_SCENE_LATTICE_CUBE, the scene of bench.py, built plain
  heightfield  the terrain of dense_simplify_bench.py, built simplified: mostly constant fills
In one process, each figure after warm-up runs as the median and the range of the repetitions:
  read_dense   the whole cube into a device tensor: wall time of Raytracer.read_dense, and device time between events
               on the context's stream around vhx_read_dense; the result must equal the grid's visible voxels
  copy         a device-to-device copy of the same bytes (wall, synchronised): the roofline of read_dense
  get_lattice  vhx_get_voxels over the same lattice as one position tensor, in chunks of at most 2^31 positions, device
               time between events (the kernel only)
  get_random   vhx_get_voxels at --random seeded positions, and at the same positions Morton sorted, in Mqueries/s
A run without a GPU fails.
usage: dense_read_bench.py [--scene bench|heightfield] [--size 1024] [--brick-dim 4] [--reps 7] [--out DIR]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--scene", choices=("bench", "heightfield"), default="bench")
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--brick-dim", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--random", type=int, default=1 << 24)
ap.add_argument("--seed", type=int, default=0x5EED)
ap.add_argument("--out", default=os.path.join("profiles", "r10", "dense_read"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def rgba(r, g, b, a=255):
    v = r | (g << 8) | (b << 16) | (a << 24)
    return v - (1 << 32) if v >= 1 << 31 else v  # as int32


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE as an int32 tensor of shape (z, y, x), slab by slab (as in dense_simplify_bench.py)."""
    q, h = size // 4, size // 2
    ax = torch.arange(size, device=dev, dtype=torch.int32)
    chan = torch.where(ax % q == 0, (ax * 255) // size, torch.full_like(ax, 128))
    x, y = ax.view(1, 1, -1), ax.view(1, -1, 1)
    grid = torch.empty((size, size, size), dtype=torch.int32, device=dev)
    alpha = -(1 << 24)  # 255 << 24 as int32
    step = max(1, min(size, (1 << 26) // (size * size)))
    for z0 in range(0, size, step):
        z = ax[z0:z0 + step].view(-1, 1, 1)
        on = (((x < q) | (y < q) | (z < q)) & (x % 2 == 0) & (y % 4 == 0) & (z % 2 == 0)) | \
             ((x >= h) & (y >= h) & (z >= h))
        colour = chan.view(1, 1, -1) | (chan.view(1, -1, 1) << 8) | (chan[z0:z0 + step].view(-1, 1, 1) << 16) | alpha
        grid[z0:z0 + step] = torch.where(on, colour, torch.zeros_like(colour))
    return grid


def heightfield(size, seed):
    """The terrain of dense_simplify_bench.py: soil below a value-noise surface, grass bands and snow caps on it."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    n = torch.zeros((1, 1, size, size))
    amp, cell = 0.5, max(4, size // 4)
    for _ in range(4):
        k = size // cell + 2
        lat = torch.rand((1, 1, k, k), generator=gen)
        up = torch.nn.functional.interpolate(lat, size=((k - 1) * cell + 1,) * 2, mode="bilinear", align_corners=True)
        n += up[:, :, :size, :size] * amp
        amp, cell = amp / 2, max(1, cell // 2)
    h = (size // 16 + n[0, 0] * (size // 4)).clamp(max=size - 1).to(torch.int32).to(dev)  # (z, x)
    grass = torch.tensor([rgba(70, 140 + b * 10, 60) for b in range(5)], dtype=torch.int32, device=dev)
    top = torch.where(h > (size * 3) // 8, torch.full_like(h, rgba(235, 235, 240)), grass[(h % 5).long()])
    grid = torch.empty((size, size, size), dtype=torch.int32, device=dev)
    soil = rgba(110, 84, 60)
    for y in range(size):  # (z, x) planes
        grid[:, y, :] = torch.where(y > h, torch.zeros_like(h), torch.where(y + 2 < h, torch.full_like(h, soil), top))
    return grid


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def repeat(fn):
    """fn() returns one measurement; warm-ups dropped."""
    return summary([fn() for _ in range(args.warmup + args.reps)][args.warmup:])


rt = vhx.Raytracer(0)
grid = lattice_cube(S) if args.scene == "bench" else heightfield(S, args.seed)
torch.cuda.synchronize()
rt.build_dense(grid, S, BD, simplify=args.scene == "heightfield")
counts = rt.tree_counts()
stream = torch.cuda.ExternalStream(rt.stream(), device=dev)
lib, h = N.lib(), rt._h
res = {"scene": args.scene, "simplified": args.scene == "heightfield", "size": S, "brick_dim": BD,
       "bytes": grid.numel() * 4, "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
       "node_count": counts.node_count, "brick_count": counts.brick_count, "solid_count": counts.solid_count}


def device_ms(call):
    """Device time of one stream-ordered libvhx call, between two events on the context's stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    N.check(call(), h)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


# ---- read_dense of the whole cube, and the copy it is measured against
out = torch.empty_like(grid)
box = N.DenseOut(0, 0, 0, S, S, S, out.data_ptr())


def read_wall():
    t0 = time.perf_counter()
    rt.read_dense(out=out)
    return (time.perf_counter() - t0) * 1e3


res["read_dense_wall_ms"] = repeat(read_wall)
res["read_dense_device_ms"] = repeat(lambda: device_ms(lambda: lib.vhx_read_dense(h, ctypes.byref(box), 1)))
if not torch.equal(out, torch.where((grid >> 24) != 0, grid, torch.zeros_like(grid))):
    raise SystemExit("dense_read_bench: read_dense of the built tree differs from the grid's visible voxels")
res["read_dense_equals_grid"] = True


def copy_wall():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out.copy_(grid)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


res["copy_wall_ms"] = repeat(copy_wall)
res["read_over_copy"] = res["read_dense_wall_ms"]["median"] / res["copy_wall_ms"]["median"]

# ---- get over the same lattice, as one position tensor filled slab by slab
n = S ** 3
pos = torch.empty((n, 3), dtype=torch.int32, device=dev)
ax = torch.arange(S, device=dev, dtype=torch.int32)
step = max(1, min(S, (1 << 26) // (S * S)))
for z0 in range(0, S, step):
    slab = pos[z0 * S * S:(z0 + step) * S * S].view(-1, S, S, 3)
    slab[..., 0] = ax.view(1, 1, -1)
    slab[..., 1] = ax.view(1, -1, 1)
    slab[..., 2] = ax[z0:z0 + step].view(-1, 1, 1)
values = torch.empty(n, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
CHUNK = 1 << 31


def get_ms(p, v):
    total = 0.0
    for i in range(0, p.shape[0], CHUNK):
        k = min(CHUNK, p.shape[0] - i)
        total += device_ms(lambda: lib.vhx_get_voxels(h, p[i:i + k].data_ptr(), k, v[i:i + k].data_ptr(), 1))
    return total


res["get_lattice_device_ms"] = repeat(lambda: get_ms(pos, values))
res["get_lattice_over_read_dense"] = res["get_lattice_device_ms"]["median"] / res["read_dense_device_ms"]["median"]
# the same voxels both ways: colour indices of the values against the grid read by read_dense
pal = torch.from_numpy(rt.read_range(N.VHX_BUF_COLOR_PALETTE, 0, counts.color_count).view("int32")).to(dev)
ci = (values & 0xFFFF).long()
seen = torch.where((values != -1) & (ci < pal.numel()), pal[ci.clamp(max=pal.numel() - 1)], torch.zeros_like(values))
rt.read_dense(out=out)
if not torch.equal(torch.where((seen >> 24) != 0, seen, torch.zeros_like(seen)), out.view(-1)):
    raise SystemExit("dense_read_bench: get over the lattice and read_dense disagree")
del pos, values, ci, seen

# ---- get at random positions, and Morton sorted
gen = torch.Generator(device="cpu").manual_seed(args.seed)
rnd = torch.randint(0, S, (args.random, 3), generator=gen, dtype=torch.int32).to(dev)


def spread(v):
    """bits of v (< 2^10 .. 2^21) spread to every third bit"""
    v = v.long()
    r = torch.zeros_like(v)
    for b in range(21):
        r |= ((v >> b) & 1) << (3 * b)
    return r


order = torch.argsort(spread(rnd[:, 0]) | (spread(rnd[:, 1]) << 1) | (spread(rnd[:, 2]) << 2))
srt = rnd[order].contiguous()
val = torch.empty(args.random, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
for name, p in (("get_random", rnd), ("get_random_morton", srt)):
    ms = repeat(lambda: get_ms(p, val))
    res[name + "_device_ms"] = ms
    res[name + "_mqueries_per_s"] = args.random / ms["median"] / 1e3

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"{args.scene}_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
