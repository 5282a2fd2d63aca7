"""Which output entries a primary trace owns (include/vhx.h, vhx_trace_primary): pure numpy, no device.

A W x H frame is cut into T x T tiles in raster order, ceil(W/T) per row; a call traces the tiles start, start + stride,
... In the TILES layout its output holds T * T entries per tile of the set, tile after tile, rows of T inside a tile;
the entries of pixels past the frame's right or bottom edge are padding. In the FRAMEBUFFER layout the output is the
whole frame, row-major, and the pixels of tiles outside the set belong to other calls."""
import numpy as np

from voxelhex_amd import _native as N


def tile_mask(W, H, T, start, stride, layout):
    """(owned, pixel). TILES layout: one entry per tile slot of the set -- owned[i] is False at padding, pixel[i] is
    the frame index y * W + x of entry i (-1 at padding). FRAMEBUFFER layout: owned[y * W + x] is True for the pixels
    of the set's tiles; pixel is None."""
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    tiles = np.arange(start, tiles_x * tiles_y, stride, dtype=np.int64)
    if layout == N.VHX_LAYOUT_FRAMEBUFFER:
        y, x = np.divmod(np.arange(W * H, dtype=np.int64), W)
        return np.isin((y // T) * tiles_x + x // T, tiles), None
    ly, lx = np.divmod(np.arange(T * T, dtype=np.int64), T)
    px = ((tiles % tiles_x) * T)[:, None] + lx[None, :]
    py = ((tiles // tiles_x) * T)[:, None] + ly[None, :]
    owned = (px < W) & (py < H)
    return owned.reshape(-1), np.where(owned, py * W + px, -1).reshape(-1)
