"""Building a LOD image with node MIPs from a device tree (vhx_build_lod; DESIGN.md "A LOD image with node MIPs, built on
the device") on one MI355X, beside the only route that existed before: download() of the source, the host MIP build
(TreeImage.lod: the host BoxTree of the image, switch_albedo_mip_maps, flatten_lod), and upload() plus set_node_mips().
The source is VHX_SCENE_LATTICE_CUBE, the scene of bench.py, built on the device by build_dense. For both methods and for
max_depth at the tree's depth and at two coarser cuts, every repetition runs the device call and then the host route, so
the two alternate; both are wall times of synchronous calls. Per row the two routes' images are compared in all seven
buffers and in the node MIPs, and the row fails where they differ. A row whose palette overflows under BoxFilter
(VHX_E_CAPACITY from both routes) is reported as such. Also reported, not compared: the frame time of one fixed camera
at 3840x2160 on the LOD image against the source's exact frame (lone frame, median of `--frames` after 2 warm-ups), and
the device time of the call's colour passes (sync()). --route-reps limits the repetitions of the host route (it takes
seconds at 1024^3); the figure used is recorded. A run without a GPU fails.
usage: lod_build_bench.py [--size 1024] [--brick-dim 4] [--reps 7] [--warmup 2] [--route-reps N] [--out DIR]"""
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
ap.add_argument("--route-reps", type=int, default=None, help="repetitions of the host route (default: --reps)")
ap.add_argument("--route-warmup", type=int, default=None, help="warm-ups of the host route (default: --warmup)")
ap.add_argument("--methods", default="box,point")
ap.add_argument("--frames", type=int, default=9)
ap.add_argument("--out", default=os.path.join("profiles", "r21", "lod_build"))
args = ap.parse_args()
route_reps = args.reps if args.route_reps is None else args.route_reps
route_warmup = args.warmup if args.route_warmup is None else args.route_warmup

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402
from voxelhex_amd.boxtree import TREE_ARRAYS  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")
W, H = 3840, 2160


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
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)} if xs else None


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def capacity(fn):
    """fn(), or "capacity" where it raises VHX_E_CAPACITY."""
    try:
        return fn()
    except N.VhxError as e:
        if e.code != N.VHX_E_CAPACITY:
            raise
        return "capacity"


src, lod, old = vhx.Raytracer(0), vhx.Raytracer(0), vhx.Raytracer(0)
src.build_dense(lattice_cube(S), S, BD)
torch.cuda.synchronize()
depth = 0
while BD * 4 ** (depth + 1) < S:
    depth += 1
counts = src.tree_counts()
res = {"scene": "bench", "size": S, "brick_dim": BD, "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
       "reps": args.reps, "route_warmup": route_warmup, "route_reps": route_reps, "frame": [W, H], "depth": depth,
       "source": {"node_count": counts.node_count, "brick_count": counts.brick_count, "color_count": counts.color_count,
                  "device_bytes": src.device_bytes()}, "rows": []}

cam = vhx.glass_camera(S, W, H, target=(S / 2.0,) * 3)
out = {f: torch.empty(W * H, dtype=torch.int32, device=dev) for f in ("value", "rgba")}


def frame_ms(rt):
    ts = []
    for _ in range(2 + args.frames):
        rt.trace_primary(cam, out=out)
        ts.append(rt.sync())
    return summary(ts[2:])


def host_route(d, method):
    image = src.download().lod(d, method)
    old.upload(image)
    old.set_node_mips(image.node_mips)
    return image


res["exact_frame_ms"] = frame_ms(src)
for method in args.methods.split(","):
    for d in [x for x in (depth, depth - 1, depth - 2) if x >= 0]:
        row = {"method": method, "max_depth": d}
        dev_ms, colour_ms, route_ms = [], [], []
        overflow = False
        for rep in range(max(args.warmup + args.reps, route_warmup + route_reps)):
            if rep < args.warmup + args.reps:
                t, got = wall_ms(lambda: capacity(lambda: lod.build_lod(src, d, method)))
                overflow |= got == "capacity"
                if rep >= args.warmup:
                    dev_ms.append(t)
                    colour_ms.append(lod.sync())
            if rep < route_warmup + route_reps:
                t, image = wall_ms(lambda: capacity(lambda: host_route(d, method)))
                if (image == "capacity") != overflow:
                    raise SystemExit(f"lod_build_bench: {method} depth {d}: only one route reports the palette overflow")
                if rep >= route_warmup:
                    route_ms.append(t)
        row["device_wall_ms"], row["device_colour_passes_ms"] = summary(dev_ms), summary(colour_ms)
        row["host_route_wall_ms"] = summary(route_ms)
        row["palette_overflow"] = overflow
        if overflow:
            row["note"] = "VHX_E_CAPACITY from both routes: the times are those of the refused calls"
        else:
            row["nodes"], row["bricks"], row["colors_added"] = got
            a, b = lod.download(), old.download()
            for name, _ in TREE_ARRAYS:
                if not np.array_equal(getattr(a, name), getattr(b, name)):
                    raise SystemExit(f"lod_build_bench: {method} depth {d}: {name} differs between the routes")
            if not np.array_equal(lod.node_mips(), old.node_mips()):
                raise SystemExit(f"lod_build_bench: {method} depth {d}: node_mips differ between the routes")
            row["routes_equal"] = True
            row["lod_frame_ms"] = frame_ms(lod)
            row["device_bytes"] = lod.device_bytes()
        if dev_ms and route_ms:
            row["route_over_device"] = row["host_route_wall_ms"]["median"] / row["device_wall_ms"]["median"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"bench_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
for r in (src, lod, old):
    r.close()
