"""Canonicalising the colour palette of an edited device tree (vhx_compact_palette) on one MI355X,
beside a device-to-device copy of the voxel buffer and beside the only other route to the same palette: read_dense of the
cube plus build_dense. The scene is VHX_SCENE_LATTICE_CUBE, the scene of bench.py, built plain at 1024^3 / brick_dim 4.
Each repetition re-creates the edited tree, untimed: build_dense, then boxes of `--colours` new colours each written over
occupied voxels with write_dense / fill_box and buried again under the scene's own voxels, so that the palette holds
dead colours and its live ones are in edit order; then compact() (no orphaned slots, as after a tidy-up). The rewrite
pass stores only the 16-byte words that change: by default the scene's colours keep their indices and few words change;
with --front the surviving box sits at the cube's min corner, so that nearly every word changes. Measured:
  palette   wall time of the synchronous compact_palette(), and the device time of its rewrite pass (sync())
  memcpy    a device-to-device hipMemcpyAsync (torch copy_) of the voxel buffer's bytes, device time by events
and, 2 repetitions after a warm-up, read_dense of the cube into a device tensor plus build_dense of it. The last
repetition checks that read_dense did not change and that the image is the one a fresh build of the cube gives.
A run without a GPU fails.
usage: dense_palette_bench.py [--size 1024] [--brick-dim 4] [--reps 7] [--out DIR]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--brick-dim", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--colours", type=int, default=200, help="new colours per edit box")
ap.add_argument("--front", action="store_true",
                help="the box that stays sits at the min corner of the cube: its colours come first in the new palette, "
                     "every index of the scene's shifts and nearly every word of the voxel buffer is stored")
ap.add_argument("--out", default=os.path.join("profiles", "r15", "palette"))
args = ap.parse_args()

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE as an int32 tensor of shape (z, y, x), slab by slab (as in dense_compact_bench.py)."""
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


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


rt = vhx.Raytracer(0)
grid = lattice_cube(S)
torch.cuda.synchronize()

# edit boxes inside the solid octant: box k holds `--colours` colours of its own; boxes 0 and 1 are buried again
edge = min(64, S // 8)
gen = torch.Generator(device="cpu").manual_seed(0x5EED)
boxes = []
for k in range(3):
    pick = torch.randint(0, args.colours, (edge, edge, edge), generator=gen, dtype=torch.int32)
    content = (pick + (1 + k * args.colours)) | (0x7F << 24)  # alpha 127: no colour of the scene
    origin = (S // 2 + 37 + k * (edge + 5), S // 2 + 21, S // 2 + 5)
    if args.front and k == 2:
        origin = (0, 0, 1)
    ox, oy, oz = origin
    boxes.append((origin, content.to(dev), grid[oz:oz + edge, oy:oy + edge, ox:ox + edge].contiguous()))


def edited_tree():
    rt.build_dense(grid, S, BD)
    for origin, content, _ in boxes:
        rt.write_dense(content, origin)
    rt.fill_box(boxes[0][0], (edge,) * 3, 0x7F0000FF)  # one more colour, over box 0's
    for origin, _, first in boxes[:2]:
        rt.write_dense(first, origin)  # the scene's voxels again: the boxes' colours are dead
    rt.compact()


def state():
    c = rt.tree_counts()
    return {"node_count": c.node_count, "brick_count": c.brick_count, "color_count": c.color_count,
            "device_bytes": rt.device_bytes(), "orphans": rt.orphans()}


res = {"size": S, "brick_dim": BD, "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
       "colours_per_box": args.colours, "box_edge": edge, "front": args.front}
rt.build_dense(grid, S, BD)
res["fresh"] = state()

call_ms, rewrite_ms, copy_ms = [], [], []
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for rep in range(args.warmup + args.reps):
    edited_tree()
    last = rep == args.warmup + args.reps - 1
    if last:
        res["edited"] = state()
        image = rt.read_dense(out=torch.empty((S, S, S), dtype=torch.int32, device=dev))
    call_ms.append(wall_ms(lambda: res.__setitem__("dropped", rt.compact_palette())))
    rewrite_ms.append(rt.sync())
    nbytes = rt.tree_counts().brick_count * BD ** 3 * 4
    a, b = (torch.empty(nbytes // 4, dtype=torch.int32, device=dev) for _ in range(2))
    b.copy_(a)  # first touch
    torch.cuda.synchronize()
    e0.record()
    b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copy_ms.append(e0.elapsed_time(e1))
    del a, b
    if last:
        res["canonical"] = state()
        if not torch.equal(rt.read_dense(out=torch.empty((S, S, S), dtype=torch.int32, device=dev)), image):
            raise SystemExit("dense_palette_bench: read_dense changed over the call")
        res["second_call_ms"] = wall_ms(lambda: res.__setitem__("dropped_again", rt.compact_palette()))
        res["second_call_rewrite_ms"] = rt.sync()
        palette = rt.read_range(N.VHX_BUF_COLOR_PALETTE, 0, rt.tree_counts().color_count).copy()
        rt.build_dense(image, S, BD)
        fresh = rt.read_range(N.VHX_BUF_COLOR_PALETTE, 0, rt.tree_counts().color_count)
        if palette.shape != fresh.shape or (palette != fresh).any():
            raise SystemExit("dense_palette_bench: the palette is not a fresh build's")
        del image
res["voxel_bytes"] = nbytes
res["call_wall_ms"] = summary(call_ms[args.warmup:])
res["rewrite_device_ms"] = summary(rewrite_ms[args.warmup:])
res["memcpy_device_ms"] = summary(copy_ms[args.warmup:])
res["rewrite_over_memcpy"] = res["rewrite_device_ms"]["median"] / res["memcpy_device_ms"]["median"]
res["rest_of_call_ms"] = res["call_wall_ms"]["median"] - res["rewrite_device_ms"]["median"]

# the only other route to the same palette: read the cube, build it again
route, read_ms, build_ms = [], [], []
for rep in range(3):
    edited_tree()
    dense = torch.empty((S, S, S), dtype=torch.int32, device=dev)
    r = wall_ms(lambda: rt.read_dense(out=dense))
    b = wall_ms(lambda: rt.build_dense(dense, S, BD))
    read_ms.append(r), build_ms.append(b), route.append(r + b)
    del dense
res["rebuild_route"] = {"read_dense_ms": summary(read_ms[1:]), "build_dense_ms": summary(build_ms[1:]),
                        "total_ms": summary(route[1:]), "scratch_bytes": S ** 3 * 4, "after": state()}

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"bench_{S}_{BD}{'_front' if args.front else ''}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
