"""Plain against simplified device tree builds (vhx_build_tree_dense / vhx_build_tree_dense_simplified, DESIGN.md
"Building the tree on the GPU") on one MI355X: what simplification costs in the build and what it buys in the tree.

A scene is generated as a dense int32 device tensor with torch operations (4 GiB at 1024^3):
  bench        VHX_SCENE_LATTICE_CUBE, the scene of bench.py (as in dense_build_bench.py)
  heightfield  terrain in the manner of VHX_SCENE_HEIGHTFIELD: 4 octaves of seeded value noise, soil below the surface,
               grass bands and snow caps on it (torch's noise, not the C++ scene's: the layers and colours are the same)

Without --simplify only the plain build is timed (the figure to compare across commits). With it, in this one process:
  build     wall time of Raytracer.build_dense (the call is synchronous), plain and simplified alternating
  tree      brick_count, solid_count, node counts by type and vhx_tree_device_bytes of each tree, each built on a
            context of its own (a context keeps the capacity of its largest tree)
  frame     the device time (vhx_sync) of a lone --frame primary frame of each tree with the same camera, and in how
            many pixels the two frames differ (a Solid brick is hit at its boundary without a walk through its cells)
  --check   the simplified tree read back must equal FlatTree.from_dense(simplify=True) of the grid copied to the host
Each figure: warm-up runs first, then the median and the range of the repetitions. A run without a GPU fails.
usage: dense_simplify_bench.py [--scene bench|heightfield] [--simplify] [--check] [--size 1024] [--reps 7]
                               [--out profiles/r09/dense_simplify]"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--scene", choices=("bench", "heightfield"), default="bench")
ap.add_argument("--simplify", action="store_true")
ap.add_argument("--check", action="store_true")
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--brick-dim", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--frame", default="3840x2160", help="WxH of the traced frame; 0x0 = no frame")
ap.add_argument("--seed", type=int, default=0x5EED)
ap.add_argument("--tag", default="", help="suffix of the output file's name")
ap.add_argument("--out", default=os.path.join("profiles", "r09", "dense_simplify"))
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import voxelhex_amd as vhx  # noqa: E402
from voxelhex_amd import _native as N  # noqa: E402

S, BD = args.size, args.brick_dim
W, H = (int(v) for v in args.frame.split("x"))
dev = torch.device("cuda:0")


def rgba(r, g, b, a=255):
    v = r | (g << 8) | (b << 16) | (a << 24)
    return v - (1 << 32) if v >= 1 << 31 else v  # as int32


def lattice_cube(size):
    """VHX_SCENE_LATTICE_CUBE (flatten.cpp Scene::voxel) as an int32 tensor of shape (z, y, x), slab by slab."""
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
    """Height h(x, z) in [S/16, S/16 + S/4) from 4 octaves of bilinear value noise; y <= h is solid: soil two below the
    surface and deeper, above it snow where h > 3S/8, else grass in five bands."""
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


rt = vhx.Raytracer(0)
grid = lattice_cube(S) if args.scene == "bench" else heightfield(S, args.seed)
torch.cuda.synchronize()
modes = ["plain", "simplified"] if args.simplify else ["plain"]


def build(mode, ctx=None):
    if mode == "plain":
        (ctx or rt).build_dense(grid, S, BD)
    else:
        (ctx or rt).build_dense(grid, S, BD, simplify=True)


# ---- the builds, alternating
for _ in range(args.warmup):
    for m in modes:
        build(m)
build_s = {m: [] for m in modes}
for _ in range(args.reps):
    for m in modes:
        t0 = time.perf_counter()
        build(m)
        build_s[m].append(time.perf_counter() - t0)

# ---- the trees and their frames
res = {"scene": args.scene, "size": S, "brick_dim": BD, "grid_bytes": grid.numel() * 4, "frame": [W, H],
       "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "modes": {}}
cam = vhx.glass_camera(S, W, H, target=(S / 2.0,) * 3) if W and H else None
frames = {}
checked = None
for m in modes:
    own = vhx.Raytracer(0)
    build(m, own)
    c = own.tree_counts()
    types = own.read_range(N.VHX_BUF_NODE_TYPE, 0, c.node_count)
    r = {"build_s": summary(build_s[m]), "node_count": c.node_count, "brick_count": c.brick_count,
         "solid_count": c.solid_count, "color_count": c.color_count, "tree_device_bytes": own.device_bytes(),
         "leaf_nodes": int((types == N.VHX_NODE_LEAF).sum()),
         "uniform_leaf_nodes": int((types == N.VHX_NODE_UNIFORM_LEAF).sum())}
    if cam is not None:
        out = {"rgba": torch.zeros(W * H, dtype=torch.int32, device=dev),
               "depth": torch.zeros(W * H, dtype=torch.float32, device=dev)}
        torch.cuda.synchronize()
        ms = []
        for i in range(args.warmup + args.reps):
            own.trace_primary(cam, out=out)
            t = own.sync()
            if i >= args.warmup:
                ms.append(t)
        r["frame_ms"] = summary(ms)
        frames[m] = out
    res["modes"][m] = r
    if args.check and m == "simplified":
        checked = own.download()
    own.close()
if len(frames) == 2:
    # the same voxels are hit; a Solid brick is hit at its boundary without a walk, so depths may differ in rounding
    p, q = frames["plain"], frames["simplified"]
    res["frame_rgba_pixels_differing"] = int((p["rgba"] != q["rgba"]).sum())
    hit = torch.isfinite(p["depth"]) & torch.isfinite(q["depth"])
    res["frame_hit_or_miss_differing"] = int((torch.isfinite(p["depth"]) != torch.isfinite(q["depth"])).sum())
    res["frame_depth_max_abs_difference"] = float((p["depth"] - q["depth"])[hit].abs().max()) if hit.any() else 0.0
frames.clear()

if checked is not None:
    img = checked
    t0 = time.perf_counter()
    ref = vhx.FlatTree.from_dense(grid.cpu().numpy().view(np.uint32), S, BD, threads=16, simplify=True)
    res["host_simplified_s"] = time.perf_counter() - t0
    for name in ("node_type", "node_ocbits", "node_children", "voxels", "solid_values", "color_palette", "data_palette"):
        a, b = getattr(img, name), getattr(ref, name)
        if a.shape != b.shape or not np.array_equal(a, b):
            raise SystemExit(f"dense_simplify_bench: {name} of the device build differs from the host image")
    assert img.counts() == ref.counts()
    res["checked_against_host"] = True

os.makedirs(args.out, exist_ok=True)
with open(os.path.join(args.out, f"{args.scene}_{S}_{BD}{args.tag}.json"), "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
rt.close()
