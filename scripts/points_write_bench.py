"""Writing scattered voxels into the device tree in place (vhx_set_voxels) on one MI355X, beside the
only route the tree offered before for the same change: read_dense of the points' bounding box, a torch scatter on the
device and write_dense of that box. The scene is bench.py's (VHX_SCENE_LATTICE_CUBE as a dense device tensor, built
plain with Raytracer.build_dense). For n = 1, 4,096, 262,144 and 4 M points (distinct positions, random colours, device
tensors), once scattered over the whole cube and once confined to a 64^3 region, each repetition alternates, wall time
of the synchronous calls:
  write   set_voxels of the list            | read_dense(box) + scatter + write_dense(box)
  clear   clear_voxels of the same list     | the same route with zeros
Both routes run in the same process, the tree rebuilt (untimed) before each series. After warm-up each figure is the
median and the range of the repetitions. A run without a GPU fails.
usage: points_write_bench.py [--size 1024] [--brick-dim 4] [--reps 7] [--warmup 2] [--out DIR] [--once N]
--once N: one set_voxels / clear_voxels pair of N scattered points after one warm-up pair, for a kernel trace."""
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
ap.add_argument("--once", type=int, default=0)
ap.add_argument("--out", default=os.path.join("profiles", "r17", "points_write"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


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


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def points(n, lo, edge, gen):
    """n distinct positions in the cube of `edge` at `lo`, as an (n, 3) int32 device tensor, and n random colours."""
    n = min(n, edge ** 3)
    flat = torch.randperm(edge ** 3, generator=gen)[:n] if edge ** 3 <= 1 << 26 else \
        torch.unique(torch.randint(0, edge ** 3, (n + n // 4,), generator=gen))[:n]
    flat = flat[torch.randperm(flat.numel(), generator=gen)]
    pos = torch.stack([flat % edge + lo[0], (flat // edge) % edge + lo[1], flat // (edge * edge) + lo[2]], 1)
    colours = (torch.randint(0, 1 << 12, (flat.numel(),), generator=gen) * 4099 % (1 << 24)) - (1 << 24)  # alpha 255
    return pos.to(torch.int32).contiguous().to(dev), colours.to(torch.int32).to(dev)


def box_route(rt, pos, colours):
    """The parent's route: the bounding box read, scattered into and written back."""
    lo = pos.min(0).values
    hi = pos.max(0).values + 1
    ext = (hi - lo).tolist()
    box = torch.empty((ext[2], ext[1], ext[0]), dtype=torch.int32, device=dev)
    rt.read_dense(tuple(lo.tolist()), tuple(ext), out=box)
    rel = (pos - lo).long()
    box[rel[:, 2], rel[:, 1], rel[:, 0]] = colours
    rt.write_dense(box, tuple(lo.tolist()))


rt = vhx.Raytracer(0)
grid = lattice_cube(S)
torch.cuda.synchronize()
rt.build_dense(grid, S, BD)
gen = torch.Generator(device="cpu").manual_seed(args.seed)

if args.once:
    pos, colours = points(args.once, (0, 0, 0), S, gen)
    for _ in range(2):
        rt.set_voxels(pos, colours)
        rt.clear_voxels(pos)
    print(json.dumps({"once": args.once, "counts_nodes": rt.tree_counts().node_count}))
    rt.close()
    sys.exit(0)

counts = rt.tree_counts()
res = {"size": S, "brick_dim": BD, "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps,
       "node_count": counts.node_count, "brick_count": counts.brick_count, "series": {}}
region = (S // 4 + 3, S // 4 + 2, S // 4 + 1)  # the 64^3 region: off the brick, leaf and node grids
for n in (1, 4096, 262144, 4 << 20):
    for spread, lo, edge in (("scattered", (0, 0, 0), S), ("region64", region, 64)):
        if n > edge ** 3:
            continue
        pos, colours = points(n, lo, edge, gen)
        zeros = torch.zeros_like(colours)
        rt.build_dense(grid, S, BD)
        t = {"set": [], "clear": [], "box_write": [], "box_clear": []}
        for _ in range(args.warmup + args.reps):
            t["set"].append(wall_ms(lambda: rt.set_voxels(pos, colours)))
            t["box_write"].append(wall_ms(lambda: box_route(rt, pos, colours)))
            t["clear"].append(wall_ms(lambda: rt.clear_voxels(pos)))
            t["box_clear"].append(wall_ms(lambda: box_route(rt, pos, zeros)))
        got = torch.from_numpy(rt.get(pos.cpu().numpy()).view("int32"))
        if not bool((got == -1).all()):
            raise SystemExit("points_write_bench: a cleared voxel is not empty")
        res["series"][f"{n}_{spread}"] = {"points": int(pos.shape[0]), "orphans": rt.orphans(),
                                          **{k + "_ms": summary(v[args.warmup:]) for k, v in t.items()}}
        print(n, spread, {k: round(statistics.median(v[args.warmup:]), 3) for k, v in t.items()}, flush=True)

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"bench_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
