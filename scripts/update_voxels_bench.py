"""Merging colours or data values into existing voxels of the device tree (VHX_WRITE_UPDATE) on one
MI355X, beside the only route the tree offered before for the same change. The scene is bench.py's
(VHX_SCENE_LATTICE_CUBE as a dense device tensor) built plain with a data plane: every voxel carries an id.
  points  n = 4,096, 262,144 and 4 M distinct occupied positions (device tensors), once scattered over the whole cube
          and once inside a 64^3 region, get n new ids:
            update_voxels(pos, data=ids)
          | get(pos) + the colour palette read back + a palette gather in torch + set_voxels(pos, albedo, ids, "replace")
  boxes   a 64^3 and a 256^3 box of occupied voxels, retagged (a plane of ids) and recoloured (a plane of colours):
            write_dense(zeros, mode="update", data=ids)          | read_dense(data=True) + write_dense(albedo, data=ids)
            write_dense(colours, mode="update")                  | read_dense(data=True) + write_dense(colours, data=old)
Both routes run in the same process and alternate inside each repetition, wall time of the synchronous calls; the tree
is rebuilt (untimed) before each series, and after it the cubes of the touched voxels are checked. After warm-up each
figure is the median and the range of the repetitions. A run without a GPU fails.
usage: update_voxels_bench.py [--size 1024] [--brick-dim 4] [--reps 7] [--warmup 2] [--out DIR]"""
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
ap.add_argument("--seed", type=int, default=0x5EED)
ap.add_argument("--out", default=os.path.join("profiles", "r20", "update_voxels"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE as an int32 tensor of shape (z, y, x), slab by slab (as in dense_write_bench.py), and a
    data plane: an id per aligned 16^3 block under every voxel."""
    q, h = size // 4, size // 2
    ax = torch.arange(size, device=dev, dtype=torch.int32)
    chan = torch.where(ax % q == 0, (ax * 255) // size, torch.full_like(ax, 128))
    x, y = ax.view(1, 1, -1), ax.view(1, -1, 1)
    grid = torch.empty((size, size, size), dtype=torch.int32, device=dev)
    data = torch.empty_like(grid)
    alpha = -(1 << 24)  # 255 << 24 as int32
    step = max(1, min(size, (1 << 26) // (size * size)))
    for z0 in range(0, size, step):
        z = ax[z0:z0 + step].view(-1, 1, 1)
        on = (((x < q) | (y < q) | (z < q)) & (x % 2 == 0) & (y % 4 == 0) & (z % 2 == 0)) | \
             ((x >= h) & (y >= h) & (z >= h))
        colour = chan.view(1, 1, -1) | (chan.view(1, -1, 1) << 8) | (chan[z0:z0 + step].view(-1, 1, 1) << 16) | alpha
        grid[z0:z0 + step] = torch.where(on, colour, torch.zeros_like(colour))
        ids = ((x >> 4) + (y >> 4) * 7 + (z >> 4) * 13) % 1000 + 1
        data[z0:z0 + step] = torch.where(on, ids, torch.zeros_like(ids))
    return grid, data


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def occupied_points(grid, n, lo, edge, gen):
    """n distinct occupied positions in the cube of `edge` at `lo`, shuffled, as an (n, 3) int32 device tensor."""
    cells = edge ** 3
    if cells <= 1 << 26:
        flat = torch.randperm(cells, generator=gen, device=dev)
    else:
        flat = torch.unique(torch.randint(0, cells, (12 * n,), generator=gen, device=dev))
        flat = flat[torch.randperm(flat.numel(), generator=gen, device=dev)]
    x, y, z = flat % edge + lo[0], (flat // edge) % edge + lo[1], flat // (edge * edge) + lo[2]
    keep = grid[z, y, x] != 0
    pos = torch.stack([x[keep], y[keep], z[keep]], 1)[:n]
    if pos.shape[0] < n:
        raise SystemExit(f"update_voxels_bench: only {pos.shape[0]} occupied positions of {n}")
    return pos.to(torch.int32).contiguous()


def new_ids(shape, gen):
    return (torch.randint(0, 1 << 12, shape, generator=gen, device=dev) + 5000).to(torch.int32)


def get_merge_set(rt, pos, ids):
    """The parent's route for points: the voxels read, their colours gathered from the palette, written back whole."""
    v = rt.get(pos)
    pal = torch.from_numpy(rt.read_range(N.VHX_BUF_COLOR_PALETTE, 0, rt.tree_counts().color_count).view("int32")).to(dev)
    ci = (v & 0xFFFF).long()
    none = (v == -1) | (ci == 0xFFFF)
    albedo = torch.where(none, torch.zeros_like(v), pal[ci.clamp(max=pal.numel() - 1)])
    rt.set_voxels(pos, albedo, ids, "replace")


def read_merge_write(rt, origin, planes, what):
    """The parent's route for a box: both planes read, one of them replaced, the box written back whole."""
    ext = tuple(reversed(planes.shape))
    a = torch.empty_like(planes)
    a, d = rt.read_dense(origin, ext, out=a, data=True)
    if what == "retag":
        rt.write_dense(a, origin, data=planes)
    else:
        rt.write_dense(planes, origin, data=d)


rt = vhx.Raytracer(0)
grid, data = lattice_cube(S)
torch.cuda.synchronize()
rt.build_dense(grid, S, BD, data=data)
gen = torch.Generator(device=dev).manual_seed(args.seed)
counts = rt.tree_counts()
res = {"size": S, "brick_dim": BD, "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
       "node_count": counts.node_count, "brick_count": counts.brick_count, "data_count": counts.data_count,
       "points": {}, "boxes": {}}
h = S // 2
region = (h + 67, h + 66, h + 65)  # a 64^3 region of the solid octant: every voxel occupied, off every grid
for n in (4096, 262144, 4 << 20):
    for spread, lo, edge in (("scattered", (0, 0, 0), S), ("region64", region, 64)):
        if n > edge ** 3:
            continue
        pos = occupied_points(grid, n, lo, edge, gen)
        rt.build_dense(grid, S, BD, data=data)
        colour_half = rt.get(pos) & 0xFFFF
        t = {"update": [], "get_merge_set": []}
        for _ in range(args.warmup + args.reps):
            ids = new_ids((n,), gen)
            t["update"].append(wall_ms(lambda: rt.update_voxels(pos, data=ids)))
            ids = new_ids((n,), gen)
            t["get_merge_set"].append(wall_ms(lambda: get_merge_set(rt, pos, ids)))
        for route in ("update", "get_merge_set"):  # both leave the new ids under the old colours
            ids = new_ids((n,), gen)
            rt.update_voxels(pos, data=ids) if route == "update" else get_merge_set(rt, pos, ids)
            v = rt.get(pos)
            dpal = torch.from_numpy(
                rt.read_range(N.VHX_BUF_DATA_PALETTE, 0, rt.tree_counts().data_count).view("int32")).to(dev)
            if not bool(((v & 0xFFFF) == colour_half).all()) or not bool((dpal[((v >> 16) & 0xFFFF).long()] == ids).all()):
                raise SystemExit(f"update_voxels_bench: {route} left other voxels than asked for")
        res["points"][f"{n}_{spread}"] = {"points": n, "orphans": rt.orphans(),
                                           **{k + "_ms": summary(v[args.warmup:]) for k, v in t.items()}}
        print(n, spread, {k: round(statistics.median(v[args.warmup:]), 3) for k, v in t.items()}, flush=True)

for edge in (64, 256):
    origin = (h + 3, h + 2, h + 1)  # in the solid octant, off the brick, leaf and node grids
    rt.build_dense(grid, S, BD, data=data)
    zeros = torch.zeros((edge,) * 3, dtype=torch.int32, device=dev)
    t = {"retag_update": [], "retag_read_merge_write": [], "recolour_update": [], "recolour_read_merge_write": []}
    for _ in range(args.warmup + args.reps):
        ids = new_ids((edge,) * 3, gen)
        t["retag_update"].append(wall_ms(lambda: rt.write_dense(zeros, origin, "update", data=ids)))
        ids = new_ids((edge,) * 3, gen)
        t["retag_read_merge_write"].append(wall_ms(lambda: read_merge_write(rt, origin, ids, "retag")))
        colours = new_ids((edge,) * 3, gen) - (1 << 24)  # alpha 255
        t["recolour_update"].append(wall_ms(lambda: rt.write_dense(colours, origin, "update")))
        colours = new_ids((edge,) * 3, gen) - (1 << 24)
        t["recolour_read_merge_write"].append(wall_ms(lambda: read_merge_write(rt, origin, colours, "recolour")))
    for route in ("update", "read_merge_write"):  # both leave the new plane beside the old one
        ids, colours = new_ids((edge,) * 3, gen), new_ids((edge,) * 3, gen) - (1 << 24)
        if route == "update":
            rt.write_dense(zeros, origin, "update", data=ids)
            rt.write_dense(colours, origin, "update")
        else:
            read_merge_write(rt, origin, ids, "retag")
            read_merge_write(rt, origin, colours, "recolour")
        a, d = rt.read_dense(origin, (edge,) * 3, out=torch.empty_like(zeros), data=True)
        if not bool((a == colours).all()) or not bool((d == ids).all()):
            raise SystemExit(f"update_voxels_bench: {route} left another box than asked for")
    res["boxes"][f"{edge}"] = {"orphans": rt.orphans(), **{k + "_ms": summary(v[args.warmup:]) for k, v in t.items()}}
    print(edge, {k: round(statistics.median(v[args.warmup:]), 3) for k, v in t.items()}, flush=True)

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"bench_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
