"""Simplifying an edited device tree (vhx_simplify_tree; DESIGN.md "Simplifying the device tree") on one MI355X, beside
a plain device copy of the voxel bytes its classify pass reads, beside compact() alone on the same tree, beside a fresh
build_dense(simplify=True) of the same voxels, and beside the only route that existed before: read_dense of the cube plus
build_dense(simplify=True). The scenes and the write series that un-simplifies the tree are those of
dense_compact_bench.py:
  bench        VHX_SCENE_LATTICE_CUBE, the scene of bench.py, built plain
  heightfield  the terrain of dense_simplify_bench.py, built simplified
Each repetition re-creates the edited tree, untimed (build_dense, then for boxes of 16^3, 64^3 and 256^3 voxels over
occupied voxels and in empty space `--series-rounds` rounds of write / clear / write back, then the whole cube written from
the grid, which leaves every touched leaf a Leaf of Parted bricks), and then measures
  simplify    wall time of the synchronous simplify(), and the device time of its classify pass (sync())
  memcpy      a device-to-device hipMemcpyAsync (torch copy_) of the reachable voxel bytes, which classify reads once, and
              of the old tree's whole voxel buffer, device time by events
On the last repetition's trees also: the frame time of one fixed camera (lone frame and a batch of 7, median of
`--frames` after 2 warm-ups) before and after, a check that read_dense of the cube did not change, and the condition that
nodes, bricks and solids equal the fresh simplified build's. Then compact() alone on the same edited tree, and the old
route on it, 2 repetitions after a warm-up. With --short only one warm-up and one repetition run and the route is left
out (for a kernel-trace run of the script on its own). A run without a GPU fails.
usage: dense_simplify_tree_bench.py [--scene bench|heightfield] [--size 1024] [--brick-dim 4] [--reps 7] [--out DIR]"""
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
ap.add_argument("--series-rounds", type=int, default=9, help="rounds per box (dense_write_bench.py: warmup + reps)")
ap.add_argument("--frames", type=int, default=9)
ap.add_argument("--seed", type=int, default=0x5EED)
ap.add_argument("--short", action="store_true")
ap.add_argument("--out", default=os.path.join("profiles", "r13", "simplify"))
args = ap.parse_args()
if args.short:
    args.warmup, args.reps = 1, 1

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")
W, H, BATCH = 1920, 1080, 7


def rgba(r, g, b, a=255):
    v = r | (g << 8) | (b << 16) | (a << 24)
    return v - (1 << 32) if v >= 1 << 31 else v  # as int32


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE as an int32 tensor of shape (z, y, x), slab by slab (as in dense_write_bench.py)."""
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
    """The terrain of dense_write_bench.py: soil below a value-noise surface, grass bands and snow caps on it."""
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

if args.scene == "bench":
    places = {"occupied": (S // 2 + 37, S // 2 + 21, S // 2 + 5), "empty": (S // 4 + 3, S // 4 + 2, S // 4 + 1)}
else:
    places = {"occupied": (S // 2 - 91, 3, S // 2 - 123), "empty": (S // 2 - 91, (S * 5) // 8 + 3, S // 2 - 123)}
gen = torch.Generator(device="cpu").manual_seed(args.seed)
colours = torch.tensor([rgba(200, 30, 30), rgba(30, 200, 30), rgba(30, 30, 200), rgba(240, 240, 20)], dtype=torch.int32)
boxes = []
for edge in (16, 64, 256):
    if edge * 2 > S:
        continue
    pick = torch.randint(0, 8, (edge, edge, edge), generator=gen)
    content = torch.where(pick < 4, colours[pick.clamp(max=3)], torch.zeros((), dtype=torch.int32)).to(dev)
    for origin in places.values():
        ox, oy, oz = origin
        boxes.append((edge, origin, content, grid[oz:oz + edge, oy:oy + edge, ox:ox + edge].contiguous()))


def orphaned_tree():
    rt.build_dense(grid, S, BD, simplify=simplified)
    for edge, origin, content, first in boxes:
        for _ in range(args.series_rounds):
            rt.write_dense(content, origin)
            rt.fill_box(origin, (edge,) * 3, 0)
            rt.write_dense(first, origin)
    for _ in range(2):
        rt.write_dense(grid)


def state():
    c = rt.tree_counts()
    return {"node_count": c.node_count, "brick_count": c.brick_count, "solid_count": c.solid_count,
            "color_count": c.color_count, "device_bytes": rt.device_bytes(), "orphans": rt.orphans()}


def copy_ms(nbytes):
    """Device time of a device-to-device copy of nbytes."""
    a, b = (torch.empty(max(1, nbytes // 4), dtype=torch.int32, device=dev) for _ in range(2))
    b.copy_(a)  # first touch
    torch.cuda.synchronize()
    e0.record()
    b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


cam = vhx.glass_camera(S, W, H, target=(S / 2.0,) * 3)
outs = [{f: torch.empty(W * H, dtype=torch.int32, device=dev) for f in ("value", "rgba")} for _ in range(BATCH)]


def frame_times():
    lone, batch = [], []
    for k in range(2 + args.frames):
        rt.trace_primary(cam, out=outs[0])
        lone.append(rt.sync())
    for k in range(2 + args.frames):
        rt.trace_primary_batch([cam] * BATCH, outs)
        batch.append(rt.sync() / BATCH)
    return {"lone_ms": summary(lone[2:]), "batch_ms_per_frame": summary(batch[2:])}


res = {"scene": args.scene, "built_simplified": simplified, "size": S, "brick_dim": BD,
       "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
       "series_rounds": args.series_rounds, "frame": [W, H], "batch": BATCH}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
rt.build_dense(grid, S, BD, simplify=True)
res["fresh_simplified_build"] = state()

# compact() alone on the edited tree: what is reachable, and what compaction leaves
orphaned_tree()
res["compact_alone"] = {"dropped": rt.compact(), "after": state()}
reach_bytes = res["compact_alone"]["after"]["brick_count"] * BD ** 3 * 4

simplify_ms, classify_ms, copy_reach_ms, copy_all_ms = [], [], [], []
for rep in range(args.warmup + args.reps):
    orphaned_tree()
    last = rep == args.warmup + args.reps - 1
    old_bytes = rt.tree_counts().brick_count * BD ** 3 * 4
    if last:
        res["edited"] = state()
        res["edited"]["frames"] = frame_times()
        image = rt.read_dense(out=torch.empty((S, S, S), dtype=torch.int32, device=dev))
    simplify_ms.append(wall_ms(lambda: res.__setitem__("dropped", rt.simplify())))
    classify_ms.append(rt.sync())
    copy_reach_ms.append(copy_ms(reach_bytes))
    copy_all_ms.append(copy_ms(old_bytes))
    if last:
        res["simplified"] = state()
        res["simplified"]["frames"] = frame_times()
        if not torch.equal(rt.read_dense(out=torch.empty((S, S, S), dtype=torch.int32, device=dev)), image):
            raise SystemExit("dense_simplify_tree_bench: read_dense changed over the simplification")
        del image
        for k in ("node_count", "brick_count", "solid_count"):
            if res["simplified"][k] != res["fresh_simplified_build"][k]:
                raise SystemExit(f"dense_simplify_tree_bench: {k} {res['simplified'][k]} is not the fresh simplified "
                                 f"build's {res['fresh_simplified_build'][k]}")
res["reachable_voxel_bytes"], res["old_voxel_bytes"] = reach_bytes, old_bytes
res["simplify_wall_ms"] = summary(simplify_ms[args.warmup:])
res["classify_device_ms"] = summary(classify_ms[args.warmup:])
res["memcpy_reachable_device_ms"] = summary(copy_reach_ms[args.warmup:])
res["memcpy_old_buffer_device_ms"] = summary(copy_all_ms[args.warmup:])
res["classify_over_memcpy_reachable"] = res["classify_device_ms"]["median"] / res["memcpy_reachable_device_ms"]["median"]
res["classify_over_memcpy_old_buffer"] = res["classify_device_ms"]["median"] / res["memcpy_old_buffer_device_ms"]["median"]
res["classify_read_GBps"] = reach_bytes / res["classify_device_ms"]["median"] / 1e6

# the old route on the same edited tree: read the cube, build it again, simplified
if not args.short:
    route, read_ms, build_ms = [], [], []
    for rep in range(3):
        orphaned_tree()
        dense = torch.empty((S, S, S), dtype=torch.int32, device=dev)
        r = wall_ms(lambda: rt.read_dense(out=dense))
        b = wall_ms(lambda: rt.build_dense(dense, S, BD, simplify=True))
        read_ms.append(r), build_ms.append(b), route.append(r + b)
        del dense
    res["rebuild_route"] = {"read_dense_ms": summary(read_ms[1:]), "build_dense_ms": summary(build_ms[1:]),
                            "total_ms": summary(route[1:]), "scratch_bytes": S ** 3 * 4, "after": state(),
                            "loses": "data values, palette order; keeps the old buffers' sizes"}
    res["simplify_over_route"] = res["simplify_wall_ms"]["median"] / res["rebuild_route"]["total_ms"]["median"]

os.makedirs(args.out, exist_ok=True)
name = f"{args.scene}_{S}_{BD}{'_short' if args.short else ''}.json"
with open(os.path.join(args.out, name), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
