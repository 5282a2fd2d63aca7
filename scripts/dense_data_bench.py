"""Timing of the dense paths with a data plane (vhx_build_tree_dense_data, vhx_read_dense_data, vhx_write_dense_data;
DESIGN.md "User data through the dense paths") beside their colour-only counterparts on one MI355X.

The bench scene (VHX_SCENE_LATTICE_CUBE, brick_dim 4) is generated as a dense int32 device tensor as in
dense_build_bench.py, and a data plane with it: 1 + ((x >> 4) + (y >> 4) + (z >> 4)) % 251 on visible voxels, 0
elsewhere (4 GiB + 4 GiB at 1024^3). Once, at 256^3, the device build with data is checked against
FlatTree.from_dense(data=) in every buffer and count. Then, in this one process, alternating within every repetition:

  build     wall time of Raytracer.build_dense without and with the data plane (the calls are synchronous)
  copy      device-to-device copies of 4 GiB and of 8 GiB (HIP events): the yardsticks for the two rates
  read      read_dense against read_dense(data=True) of the whole cube into device tensors
  write     write_dense of a 256^3 box of random colours (half the voxels set) without and with a data plane

Pass A reads twice the bytes with a data plane, so the figure to compare is the build rate over the copy rate of the
same bytes: grid bytes / build time over bytes / copy time, colour-only (4 GiB) and with data (8 GiB).
Each figure: warm-up runs first, then the median and the range of the repetitions. A run without a GPU fails.
usage: dense_data_bench.py [--size 1024] [--reps 7] [--box 256] [--out profiles/r16/dense_data]"""
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
ap.add_argument("--box", type=int, default=256)
ap.add_argument("--check-size", type=int, default=256)
ap.add_argument("--out", default=os.path.join("profiles", "r16", "dense_data"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402

S, BD = args.size, args.brick_dim
dev = torch.device("cuda:0")


def lattice_cube(size, grid, data):
    """VHX_SCENE_LATTICE_CUBE (dense_build_bench.py) into `grid`, and the data plane into `data`, slab by slab."""
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
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def wall(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def copy_time(dst, src):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dst.copy_(src)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


rt = vhx.Raytracer(0)

# ---- correctness, once, at a size the host builder takes in its stride
C = args.check_size
small = torch.empty((2, C, C, C), dtype=torch.int32, device=dev)
lattice_cube(C, small[0], small[1])
rt.build_dense(small[0], C, BD, data=small[1])
img = rt.download()
host = small.cpu().numpy().view(np.uint32)
ref = vhx.FlatTree.from_dense(host[0], C, BD, threads=16, data=host[1])
for name in ("node_type", "node_ocbits", "node_children", "voxels", "solid_values", "color_palette", "data_palette"):
    a, b = getattr(img, name), getattr(ref, name)
    if a.shape != b.shape or not np.array_equal(a, b):
        raise SystemExit(f"dense_data_bench: {name} of the device build differs from FlatTree.from_dense(data=)")
assert img.counts() == ref.counts()
check_counts = img.counts()
del img, ref, host, small

# ---- the scene: both planes in one allocation (each 16-byte aligned), and the copies' destination
both = torch.empty((2, S, S, S), dtype=torch.int32, device=dev)
grid, data = both[0], both[1]
lattice_cube(S, grid, data)
dst = torch.empty_like(both)
torch.cuda.synchronize()
plane_bytes = grid.numel() * 4

B = min(args.box, S // 2)
origin = (S // 2 + 3, S // 2 + 5, S // 2 + 7)  # off every grid, inside the solid cube
gen = torch.Generator(device=dev).manual_seed(5)
box_grid = torch.randint(0, 1 << 24, (B, B, B), generator=gen, device=dev, dtype=torch.int32) | -(1 << 24)
box_grid = torch.where(torch.rand((B, B, B), generator=gen, device=dev) < 0.5, box_grid, torch.zeros_like(box_grid)) & \
    (-(1 << 24) | 0x0F0F0F)  # 4096 colours at most
box_data = torch.where(torch.rand((B, B, B), generator=gen, device=dev) < 0.5,
                       torch.randint(1, 1000, (B, B, B), generator=gen, device=dev, dtype=torch.int32),
                       torch.zeros((B, B, B), dtype=torch.int32, device=dev))
out_a, out_d = torch.empty_like(grid), torch.empty_like(grid)
torch.cuda.synchronize()

t = {k: [] for k in ("build", "build_data", "copy_plane", "copy_both", "read", "read_data", "write", "write_data")}
for i in range(args.warmup + args.reps):
    row = {
        "build": wall(lambda: rt.build_dense(grid, S, BD)),
        "copy_plane": copy_time(dst[0], grid),
        "build_data": wall(lambda: rt.build_dense(grid, S, BD, data=data)),
        "copy_both": copy_time(dst, both),
        "read": wall(lambda: rt.read_dense(out=out_a)),
        "read_data": wall(lambda: rt.read_dense(out=out_a, data=out_d)),
        "write": wall(lambda: rt.write_dense(box_grid, origin)),
        "write_data": wall(lambda: rt.write_dense(box_grid, origin, data=box_data)),
    }
    if i >= args.warmup:
        for k, v in row.items():
            t[k].append(v)
counts = rt.tree_counts()

s = {k: summary(v) for k, v in t.items()}
rate = lambda nbytes, k: {m: nbytes / s[k][m] / 1e12 for m in ("median", "min", "max")}  # noqa: E731
res = {
    "scene": "VHX_SCENE_LATTICE_CUBE", "size": S, "brick_dim": BD, "plane_bytes": plane_bytes,
    "device": torch.cuda.get_device_name(0), "checked_at": args.check_size, "checked_counts": check_counts,
    "seconds": s,
    "build_grid_TBps": rate(plane_bytes, "build"), "build_data_grid_TBps": rate(2 * plane_bytes, "build_data"),
    "copy_plane_TBps_one_way": rate(plane_bytes, "copy_plane"), "copy_both_TBps_one_way": rate(2 * plane_bytes, "copy_both"),
    "build_rate_over_copy_rate": s["copy_plane"]["median"] / s["build"]["median"],
    "build_data_rate_over_copy_rate": s["copy_both"]["median"] / s["build_data"]["median"],
    "build_data_over_build": s["build_data"]["median"] / s["build"]["median"],
    "read_data_over_read": s["read_data"]["median"] / s["read"]["median"],
    "write_box": B, "write_data_over_write": s["write_data"]["median"] / s["write"]["median"],
    "data_count_after_writes": counts.data_count, "color_count_after_writes": counts.color_count,
}
os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"dense_data_{S}_{BD}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
