"""Canonicalising both palettes of an edited device tree (vhx_compact_palettes) on one MI355X, beside
the colour-only call it generalises, beside a device-to-device copy of the voxel buffer, and beside the only route to a
canonical data_palette that exists without it: read_dense(data=True) of the cube plus build_dense(data=).
The scene is VHX_SCENE_LATTICE_CUBE, the scene of bench.py, built plain at 1024^3 / brick_dim 4 with the data plane of
dense_data_bench.py (1 + ((x >> 4) + (y >> 4) + (z >> 4)) % 251 on visible voxels). Before each measurement the edited
tree is re-created, untimed: build_dense(data=), then three boxes of `--ids` fresh ids and `--colours` fresh colours each
written over occupied voxels with write_dense(data=), one filled once more, two buried again under the scene's own
voxels, so that both palettes hold dead entries and their live ones are in edit order; then compact().
Within every repetition, alternating:
  colour     wall time of compact_palette(), and the device time of its rewrite pass (sync())
  both       the same for compact_palettes()                                  (only where the library has the call)
  split      compact_palettes(data=False) followed by compact_palettes(color=False), wall time of the two     (likewise)
  route      read_dense(data=True) of the cube into device tensors, then build_dense(data=) of them, wall time of each
  memcpy     a device-to-device hipMemcpyAsync (torch copy_) of the voxel buffer's bytes, device time by events
The script runs on a library without vhx_compact_palettes as well (the measurements that need it are left out), so
that one file measures two commits. The last repetition checks that compact_palettes() left read_dense(data=True)
unchanged and both palettes those of a fresh build of the cube. --trace runs only the calls (3 times each), for a kernel
trace taken in a run of its own. A run without a GPU fails.
usage: palettes_bench.py [--size 1024] [--brick-dim 4] [--reps 7] [--tag NAME] [--out DIR] [--trace]"""
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
ap.add_argument("--ids", type=int, default=5000, help="new data values per edit box")
ap.add_argument("--tag", default="run", help="names the result file: bench_<size>_<brick_dim>_<tag>.json")
ap.add_argument("--trace", action="store_true", help="only the calls, for a kernel trace")
ap.add_argument("--root", default=None, help="the tree whose voxelhex_amd is measured (default: this script's)")
ap.add_argument("--out", default=os.path.join("profiles", "r19", "palettes"))
args = ap.parse_args()

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(args.root) if args.root else os.path.dirname(HERE))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def lattice_cube(size, grid, data):
    """VHX_SCENE_LATTICE_CUBE into `grid` and the data plane into `data`, slab by slab (as in dense_data_bench.py)."""
    q, h = size // 4, size // 2
    ax = torch.arange(size, device=dev, dtype=torch.int32)
    chan = torch.where(ax % q == 0, (ax * 255) // size, torch.full_like(ax, 128))
    x, y = ax.view(1, 1, -1), ax.view(1, -1, 1)
    alpha = -(1 << 24)  # 255 << 24 as int32
    step = max(1, min(size, (1 << 26) // (size * size)))
    for z0 in range(0, size, step):
        z = ax[z0:z0 + step].view(-1, 1, 1)
        on = (((x < q) | (y < q) | (z < q)) & (x % 2 == 0) & (y % 4 == 0) & (z % 2 == 0)) | \
             ((x >= h) & (y >= h) & (z >= h))
        colour = chan.view(1, 1, -1) | (chan.view(1, -1, 1) << 8) | (chan[z0:z0 + step].view(-1, 1, 1) << 16) | alpha
        grid[z0:z0 + step] = torch.where(on, colour, torch.zeros_like(colour))
        value = 1 + ((x >> 4) + (y >> 4) + (z >> 4)) % 251
        data[z0:z0 + step] = torch.where(on, value, torch.zeros_like(value))


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "range": max(xs) - min(xs), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


rt = vhx.Raytracer(0)
has_both = hasattr(rt, "compact_palettes")
planes = torch.empty((2, S, S, S), dtype=torch.int32, device=dev)
grid, data = planes[0], planes[1]
lattice_cube(S, grid, data)
torch.cuda.synchronize()

# edit boxes inside the solid octant: box k holds colours and ids of its own; boxes 0 and 1 are buried again
edge = min(64, S // 8)
gen = torch.Generator(device="cpu").manual_seed(0x5EED)
boxes = []
for k in range(3):
    pick = torch.randint(0, args.colours, (edge, edge, edge), generator=gen, dtype=torch.int32)
    content = (pick + (1 + k * args.colours)) | (0x7F << 24)  # alpha 127: no colour of the scene
    ids = torch.randint(0, args.ids, (edge, edge, edge), generator=gen, dtype=torch.int32) + (1000 + k * args.ids)
    ox, oy, oz = origin = (S // 2 + S // 32 + k * (edge + 5), S // 2 + 21, S // 2 + 5)
    sl = (slice(oz, oz + edge), slice(oy, oy + edge), slice(ox, ox + edge))
    boxes.append((origin, content.to(dev), ids.to(dev), grid[sl].contiguous(), data[sl].contiguous()))


def edited_tree():
    rt.build_dense(grid, S, BD, data=data)
    for origin, content, ids, _, _ in boxes:
        rt.write_dense(content, origin, data=ids)
    rt.fill_box(boxes[0][0], (edge,) * 3, 0x7F0000FF, 999)  # one more colour and id, over box 0's
    for origin, _, _, first, first_data in boxes[:2]:
        rt.write_dense(first, origin, data=first_data)  # the scene's voxels again: the boxes' entries are dead
    rt.compact()


def state():
    c = rt.tree_counts()
    return {"node_count": c.node_count, "brick_count": c.brick_count, "color_count": c.color_count,
            "data_count": c.data_count, "device_bytes": rt.device_bytes(), "orphans": rt.orphans()}


if args.trace:
    for _ in range(3):
        edited_tree()
        rt.compact_palette()
        if has_both:
            edited_tree()
            rt.compact_palettes()
            edited_tree()
            rt.compact_palettes(color=False)
    rt.close()
    raise SystemExit(0)

res = {"size": S, "brick_dim": BD, "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
       "colours_per_box": args.colours, "ids_per_box": args.ids, "box_edge": edge, "tag": args.tag,
       "has_compact_palettes": has_both}
rt.build_dense(grid, S, BD, data=data)
res["fresh"] = state()

names = ("colour_wall", "colour_rewrite", "both_wall", "both_rewrite", "split_wall", "read", "build", "route", "memcpy")
t = {k: [] for k in names}
out = torch.empty((2, S, S, S), dtype=torch.int32, device=dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for rep in range(args.warmup + args.reps):
    last = rep == args.warmup + args.reps - 1
    edited_tree()
    if rep == 0:
        res["edited"] = state()
    t["colour_wall"].append(wall_ms(lambda: res.__setitem__("colour_dropped", rt.compact_palette())))
    t["colour_rewrite"].append(rt.sync())
    if has_both:
        edited_tree()
        if last:
            rt.read_dense(out=out[0], data=out[1])
            image = out.clone()
        t["both_wall"].append(wall_ms(lambda: res.__setitem__("both_dropped", list(rt.compact_palettes()))))
        t["both_rewrite"].append(rt.sync())
        if last:
            res["canonical"] = state()
            rt.read_dense(out=out[0], data=out[1])
            if not torch.equal(out, image):
                raise SystemExit("palettes_bench: read_dense(data=True) changed over the call")
            res["second_call_ms"] = wall_ms(lambda: res.__setitem__("dropped_again", list(rt.compact_palettes())))
            c = rt.tree_counts()
            pals = [rt.read_range(b, 0, n).copy() for b, n in ((N.VHX_BUF_COLOR_PALETTE, c.color_count),
                                                               (N.VHX_BUF_DATA_PALETTE, c.data_count))]
            rt.build_dense(image[0], S, BD, data=image[1])
            c = rt.tree_counts()
            for old, (b, n) in zip(pals, ((N.VHX_BUF_COLOR_PALETTE, c.color_count), (N.VHX_BUF_DATA_PALETTE, c.data_count))):
                fresh = rt.read_range(b, 0, n)
                if old.shape != fresh.shape or (old != fresh).any():
                    raise SystemExit("palettes_bench: a palette is not a fresh build's")
            del image
        edited_tree()
        t["split_wall"].append(wall_ms(lambda: (rt.compact_palettes(data=False), rt.compact_palettes(color=False))))
    edited_tree()
    r = wall_ms(lambda: rt.read_dense(out=out[0], data=out[1]))
    b = wall_ms(lambda: rt.build_dense(out[0], S, BD, data=out[1]))
    t["read"].append(r), t["build"].append(b), t["route"].append(r + b)
    nbytes = rt.tree_counts().brick_count * BD ** 3 * 4
    a, c = (torch.empty(nbytes // 4, dtype=torch.int32, device=dev) for _ in range(2))
    c.copy_(a)  # first touch
    torch.cuda.synchronize()
    e0.record()
    c.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    t["memcpy"].append(e0.elapsed_time(e1))
    del a, c
res["voxel_bytes"] = nbytes
res["ms"] = {k: summary(v[args.warmup:]) for k, v in t.items() if v}
m = res["ms"]
if has_both:
    res["route_minus_both_ms"] = m["route"]["median"] - m["both_wall"]["median"]
    res["sum_of_ranges_ms"] = m["route"]["range"] + m["both_wall"]["range"]
    res["faster_by_more_than_the_ranges"] = res["route_minus_both_ms"] > res["sum_of_ranges_ms"]
    res["both_rewrite_over_memcpy"] = m["both_rewrite"]["median"] / m["memcpy"]["median"]
    res["split_over_both"] = m["split_wall"]["median"] / m["both_wall"]["median"]

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"bench_{S}_{BD}_{args.tag}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
