"""Timing of the device tree builder (vhx_build_tree_dense, DESIGN.md "Building the tree on the GPU") on one MI355X.

The bench scene (VHX_SCENE_LATTICE_CUBE, brick_dim 4) is generated as a dense int32 device tensor with torch operations
(4 GiB at 1024^3), built once and checked: download() must equal FlatTree.build_scene in every buffer and count. Then,
in this one process:

  build     wall time of Raytracer.build_dense (the call is synchronous), and the grid's bytes over it
  copy      a device-to-device copy of the same bytes (HIP events): the yardstick for the rate
  parent    FlatTree.build_scene(threads=16) + Raytracer.upload: the only route to this tree before the device builder
  traffic   how often the build reads the grid and what it writes, counted from the tree's counts

Each figure: warm-up runs first, then the median and the range of the repetitions. A run without a GPU fails.
usage: dense_build_bench.py [--size 1024] [--reps 7] [--parent-reps 3] [--out profiles/r08/dense_build]"""
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
ap.add_argument("--parent-reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join("profiles", "r08", "dense_build"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE (flatten.cpp Scene::voxel) as an int32 tensor of shape (z, y, x), slab by slab."""
    q, h = size // 4, size // 2
    ax = torch.arange(size, device=dev, dtype=torch.int32)
    chan = torch.where(ax % q == 0, (ax * 255) // size, torch.full_like(ax, 128))  # (float)c / S * 255 is exact here
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


rt = vhx.Raytracer(0)
grid = lattice_cube(S)
torch.cuda.synchronize()
grid_bytes = grid.numel() * 4

# ---- correctness, once
rt.build_dense(grid, S, BD)
img = rt.download()
t0 = time.perf_counter()
ref = vhx.FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, S, BD, threads=16)
ref_build_s = time.perf_counter() - t0
for name in ("node_type", "node_ocbits", "node_children", "voxels", "solid_values", "color_palette", "data_palette"):
    a, b = getattr(img, name), getattr(ref, name)
    if a.shape != b.shape or not np.array_equal(a, b):
        raise SystemExit(f"dense_build_bench: {name} of the device build differs from FlatTree.build_scene")
assert img.counts() == ref.counts()
counts = img.counts()
del img

# ---- the build
for _ in range(args.warmup):
    rt.build_dense(grid, S, BD)
build_s = []
for _ in range(args.reps):
    t0 = time.perf_counter()
    rt.build_dense(grid, S, BD)
    build_s.append(time.perf_counter() - t0)

# ---- the copy
dst = torch.empty_like(grid)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
copy_s = []
for i in range(args.warmup + args.reps):
    e0.record()
    dst.copy_(grid)
    e1.record()
    e1.synchronize()
    if i >= args.warmup:
        copy_s.append(e0.elapsed_time(e1) * 1e-3)
del dst

# ---- the parent's route: host bulk builder + upload
up = vhx.Raytracer(0)
parent_s, parent_build_s = [], [ref_build_s]
up.upload(ref)  # warm-up of the upload path (the build ran once above)
for _ in range(args.parent_reps):
    t0 = time.perf_counter()
    f = vhx.FlatTree.build_scene(N.VHX_SCENE_LATTICE_CUBE, S, BD, threads=16)
    t1 = time.perf_counter()
    up.upload(f)
    up.sync()
    parent_s.append(time.perf_counter() - t0)
    parent_build_s.append(t1 - t0)
up.close()

# ---- traffic, from the counts: pass A reads every voxel once, the brick emission every cell of a present brick
n3 = BD ** 3
cells = counts["brick_count"] * n3
raw_written = counts["node_count"] * (4 + 8 + 256) + cells * 4 + counts["color_count"] * 4
derived_written = counts["node_count"] * 16 + counts["brick_count"] * max(1, n3 // 64) * 8 + \
    (counts["node_count"] * 64 * 16 if BD <= 4 else 0)
b, c = summary(build_s), summary(copy_s)
p = summary(parent_s) if parent_s else None
res = {
    "scene": "VHX_SCENE_LATTICE_CUBE", "size": S, "brick_dim": BD, "grid_bytes": grid_bytes, "counts": counts,
    "device": torch.cuda.get_device_name(0),
    "build_dense_s": b, "build_grid_TBps": {k: grid_bytes / b[k] / 1e12 for k in ("median", "min", "max")},
    "copy_d2d_s": c, "copy_TBps_one_way": {k: grid_bytes / c[k] / 1e12 for k in ("median", "min", "max")},
    "build_rate_over_copy_rate": c["median"] / b["median"],
    "parent_build_scene_plus_upload_s": p, "parent_build_scene_s": summary(parent_build_s),
    "speedup_over_parent": p["median"] / b["median"] if p else None,
    "grid_reads": 1.0 + cells / grid.numel(), "grid_bytes_read": grid_bytes + cells * 4,
    "raw_bytes_written": raw_written, "derived_bytes_written": derived_written,
    "scratch_bytes_reset": sum(64 ** lv for lv in range(20) if BD * 4 ** (lv + 1) <= S) * 8 + (1 << 18) * 12,
}
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"dense_build_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
