"""Writing boxes into the device tree in place (vhx_write_dense; DESIGN.md "Writing a box in place") on one MI355X,
beside what the tree offered before for the same change: build_dense of the whole edited grid. The scenes are those of
dense_read_bench.py (generated as dense int32 device tensors and built with Raytracer.build_dense):
  bench        VHX_SCENE_LATTICE_CUBE, the scene of bench.py, built plain
  heightfield  the terrain of dense_simplify_bench.py, built simplified
For boxes of 16^3, 64^3 and 256^3 voxels (origins off every grid), once over occupied voxels and once in empty space,
each repetition, wall time of the synchronous call:
  write    write_dense of a device tensor of random colours (half the voxels set) over the box
  clear    fill_box(box, 0) of what was just written
and then, untimed, the box's first contents written back. Slots are never reused, so every repetition's write takes new
bricks; the orphans at the end are reported. Then the whole cube written from the scene's own grid, and build_dense of
that grid. After warm-up each figure is the median and the range of the repetitions. A run without a GPU fails.
usage: dense_write_bench.py [--scene bench|heightfield] [--size 1024] [--brick-dim 4] [--reps 7] [--out DIR]"""
import argparse
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
ap.add_argument("--seed", type=int, default=0x5EED)
ap.add_argument("--out", default=os.path.join("profiles", "r11", "dense_write"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def rgba(r, g, b, a=255):
    v = r | (g << 8) | (b << 16) | (a << 24)
    return v - (1 << 32) if v >= 1 << 31 else v  # as int32


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE as an int32 tensor of shape (z, y, x), slab by slab (as in dense_read_bench.py)."""
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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


rt = vhx.Raytracer(0)
simplified = args.scene == "heightfield"
grid = lattice_cube(S) if args.scene == "bench" else heightfield(S, args.seed)
torch.cuda.synchronize()
rt.build_dense(grid, S, BD, simplify=simplified)
counts = rt.tree_counts()
res = {"scene": args.scene, "simplified": simplified, "size": S, "brick_dim": BD,
       "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
       "node_count": counts.node_count, "brick_count": counts.brick_count, "device_bytes": rt.device_bytes(),
       "boxes": {}}

# origins off the brick, leaf and node grids; "occupied" lies in the scene's solid part, "empty" in its air
if args.scene == "bench":
    places = {"occupied": (S // 2 + 37, S // 2 + 21, S // 2 + 5), "empty": (S // 4 + 3, S // 4 + 2, S // 4 + 1)}
else:
    places = {"occupied": (S // 2 - 91, 3, S // 2 - 123), "empty": (S // 2 - 91, (S * 5) // 8 + 3, S // 2 - 123)}
gen = torch.Generator(device="cpu").manual_seed(args.seed)
colours = torch.tensor([rgba(200, 30, 30), rgba(30, 200, 30), rgba(30, 30, 200), rgba(240, 240, 20)], dtype=torch.int32)
for edge in (16, 64, 256):
    if edge * 2 > S:
        continue
    pick = torch.randint(0, 8, (edge, edge, edge), generator=gen)
    content = torch.where(pick < 4, colours[pick.clamp(max=3)], torch.zeros((), dtype=torch.int32)).to(dev)
    for place, origin in places.items():
        ox, oy, oz = origin
        first = grid[oz:oz + edge, oy:oy + edge, ox:ox + edge].contiguous()
        w, c = [], []
        for _ in range(args.warmup + args.reps):
            w.append(wall_ms(lambda: rt.write_dense(content, origin)))
            c.append(wall_ms(lambda: rt.fill_box(origin, (edge,) * 3, 0)))
            rt.write_dense(first, origin)
        res["boxes"][f"{edge}_{place}"] = {"origin": origin, "occupied_voxels": int((first != 0).sum()),
                                           "write_ms": summary(w[args.warmup:]), "clear_ms": summary(c[args.warmup:])}
if not torch.equal(torch.from_numpy(rt.read_dense((0, 0, 0), (S, S, 64)).view("int32")).to(dev),
                   torch.where((grid[:64] >> 24) != 0, grid[:64], torch.zeros_like(grid[:64]))):
    raise SystemExit("dense_write_bench: the tree differs from the grid after the boxes were written back")
res["orphans_after_boxes"] = rt.orphans()
res["device_bytes_after_boxes"] = rt.device_bytes()

few = max(3, args.reps // 2)
res["whole_cube_write_ms"] = summary([wall_ms(lambda: rt.write_dense(grid)) for _ in range(1 + few)][1:])
res["device_bytes_after_whole_cube"] = rt.device_bytes()
res["build_dense_ms"] = summary([wall_ms(lambda: rt.build_dense(grid, S, BD, simplify=simplified))
                                 for _ in range(args.warmup + args.reps)][args.warmup:])

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"{args.scene}_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
