"""Listing the occupied voxels of a box of the device tree (vhx_list_voxels) on one MI355X, beside the
route a caller had before for the same answer: read_dense(data=True) of the box into device tensors, torch.nonzero over
the two planes and two gathers. A scene is generated as a dense int32 device tensor and built with Raytracer.build_dense
(as in dense_read_bench.py):
  bench        VHX_SCENE_LATTICE_CUBE, the scene of bench.py
  heightfield  the terrain of dense_simplify_bench.py
each once plain (Parted bricks) and once simplified (Solid bricks, UniformLeaf nodes). For the whole cube and for 64^3
and 256^3 boxes off the brick, leaf and node grids, placed where the scene is sparse, mixed and full (bench: in the
lattice, across the corner of the solid cube, inside it; heightfield: across the surface, in the soil), each repetition
alternates, wall time of the synchronous calls:
  count   count_voxels(box)                                  (one readback, no array)
  list    list_voxels(box, capacity=count, device=True)      (int32 device tensors)
  dense   read_dense(box, data=True) into device tensors, torch.nonzero, two gathers
The dense route's peak device memory is torch's peak during it plus the tree; the list route's is its output plus the
scratch the context holds afterwards (free device memory before the context's first list call minus after, cumulative
over the boxes in their order; the runtime hands out device memory in chunks of 2 MiB, so small figures are coarse). Once per
box the two routes' results are compared as sets (the list route's order is positional, the dense route's x-major).
After warm-up each figure is the median and the range of the repetitions. A run without a GPU fails.
usage: list_voxels_bench.py [--scene bench|heightfield] [--size 1024] [--brick-dim 4] [--reps 5] [--out DIR] [--once]
--once: one count_voxels / list_voxels pair of the whole cube of the plain tree after one warm-up pair, for a kernel trace."""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--seed", type=int, default=0x5EED)
ap.add_argument("--once", action="store_true")
ap.add_argument("--out", default=os.path.join("profiles", "r18", "list_voxels"))
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
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def dense_route(rt, origin, extents):
    """The route without list_voxels: the box read densely, its occupied voxels found and gathered."""
    gx, gy, gz = extents
    a = torch.empty((gz, gy, gx), dtype=torch.int32, device=dev)
    d = torch.empty_like(a)
    rt.read_dense(origin, extents, out=a, data=d)
    at = torch.nonzero((a != 0) | (d != 0))
    z, y, x = at[:, 0], at[:, 1], at[:, 2]
    return at, a[z, y, x], d[z, y, x]


rt = vhx.Raytracer(0)
grid = lattice_cube(S) if args.scene == "bench" else heightfield(S, args.seed)
torch.cuda.synchronize()

if args.once:
    rt.build_dense(grid, S, BD)
    del grid
    for _ in range(2):
        n = rt.count_voxels()
        rt.list_voxels(capacity=n, device=True)
    print(json.dumps({"once": True, "count": n}))
    rt.close()
    sys.exit(0)

def at(x, y, z):
    return x + 3, y + 2, z + 1  # off the brick, leaf and node grids


h, q = S // 2, S // 4
if args.scene == "bench":  # the lattice (1 voxel in 16), the corner of the solid cube (an eighth of the box), inside it
    boxes = [("box64_lattice", at(0, 0, 0), (64,) * 3), ("box64_corner", at(h - 32, h - 32, h - 32), (64,) * 3),
             ("box64_solid", at(h, h, h), (64,) * 3), ("box256_lattice", at(0, 0, 0), (256,) * 3),
             ("box256_corner", at(h - 128, h - 128, h - 128), (256,) * 3), ("box256_solid", at(h, h, h), (256,) * 3)]
else:  # across the terrain's surface, and in the soil below it (y is up; the surface lies between S/16 and 5S/16)
    boxes = [("box64_surface", at(q, S // 8, q), (64,) * 3), ("box64_soil", at(q, 0, q), (64, 56, 64)),
             ("box256_surface", at(q, S // 16, q), (256,) * 3)]
boxes.append(("cube", (0, 0, 0), (S,) * 3))
res = {"scene": args.scene, "size": S, "brick_dim": BD, "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
       "reps": args.reps, "trees": {}}
for tree in ("plain", "simplified"):
    rt.close()
    rt = vhx.Raytracer(0)  # a fresh context: its list scratch starts empty
    rt.build_dense(grid, S, BD, simplify=tree == "simplified")
    counts = rt.tree_counts()
    tr = {"node_count": counts.node_count, "brick_count": counts.brick_count, "solid_count": counts.solid_count,
          "tree_bytes": rt.device_bytes(), "boxes": {}}
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for name, origin, extents in boxes:
        if any(o + e > S for o, e in zip(origin, extents)):
            continue
        count = rt.count_voxels(origin, extents)
        scratch = free0 - torch.cuda.mem_get_info(dev)[0]  # no torch allocation since free0: libvhx's scratch so far
        t = {"count": [], "list": [], "dense": []}
        dense_peak = 0
        for rep in range(args.warmup + args.reps):
            t["count"].append(wall_ms(lambda: rt.count_voxels(origin, extents))[0])
            ms, got = wall_ms(lambda: rt.list_voxels(origin, extents, capacity=count, device=True))
            t["list"].append(ms)
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            ms, ref = wall_ms(lambda: dense_route(rt, origin, extents))
            t["dense"].append(ms)
            dense_peak = max(dense_peak, torch.cuda.max_memory_allocated(dev) - base)
            if rep == 0:  # the same voxels both ways
                if got[3] != count or ref[0].shape[0] != count:
                    raise SystemExit(f"list_voxels_bench: {name}: counts differ: {got[3]}, {ref[0].shape[0]}, {count}")
                p = got[0].long() - torch.tensor(origin, device=dev)
                order = torch.argsort((p[:, 2] * extents[1] + p[:, 1]) * extents[0] + p[:, 0])
                same = torch.equal(p[order][:, [2, 1, 0]], ref[0]) and torch.equal(got[1][order], ref[1]) and \
                    torch.equal(got[2][order], ref[2])
                if not same:
                    raise SystemExit(f"list_voxels_bench: {name}: the two routes list different voxels")
                del p, order
            del got, ref
        torch.cuda.empty_cache()  # the next box's scratch figure again sees only libvhx's allocations
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(dev)[0] + scratch
        tr["boxes"][name] = {"origin": origin, "extents": extents, "voxels": count,
                             "fill": count / (extents[0] * extents[1] * extents[2]),
                             "list_output_bytes": count * 20, "list_scratch_bytes": scratch,
                             "dense_peak_bytes": dense_peak, "dense_peak_with_tree_bytes": dense_peak + tr["tree_bytes"],
                             **{k + "_ms": summary(v[args.warmup:]) for k, v in t.items()}}
        print(tree, name, count, {k: round(statistics.median(v[args.warmup:]), 3) for k, v in t.items()},
              "scratch", scratch, "dense peak", dense_peak, flush=True)
    res["trees"][tree] = tr

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"{args.scene}_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
