"""tests/_tilemask.py (the ownership mask the shadow-matrix GPU tests rely on) against the C tile plan and by hand."""
import numpy as np
import pytest

from tests._tilemask import tile_mask
from voxelhex_amd import _native as N
from voxelhex_amd import multigpu as M


def test_hand_written_3x2_tiles():
    """A 5 x 3 frame in 2 x 2 tiles: 3 x 2 tiles, the right column one pixel wide, the bottom row one pixel high.
    The set 1, 3, 5 entry by entry."""
    W, H, T = 5, 3, 2
    owned, pixel = tile_mask(W, H, T, 1, 2, N.VHX_LAYOUT_TILES)
    want = [2, 3, 7, 8,        # tile 1: x 2..3, y 0..1
            10, 11, -1, -1,    # tile 3: x 0..1, y 2 (y 3 is past the frame)
            14, -1, -1, -1]    # tile 5: x 4, y 2
    assert pixel.tolist() == want
    assert owned.tolist() == [p >= 0 for p in want]
    fb, none = tile_mask(W, H, T, 1, 2, N.VHX_LAYOUT_FRAMEBUFFER)
    assert none is None
    assert fb.reshape(H, W).astype(int).tolist() == [[0, 0, 1, 1, 0],
                                                      [0, 0, 1, 1, 0],
                                                      [1, 1, 0, 0, 1]]
    # the other set, 0, 2, 4, owns the rest
    other, opix = tile_mask(W, H, T, 0, 2, N.VHX_LAYOUT_TILES)
    assert opix.tolist() == [0, 1, 5, 6, 4, -1, 9, -1, 12, 13, -1, -1]
    assert other.tolist() == [p >= 0 for p in opix.tolist()]
    assert (tile_mask(W, H, T, 0, 2, N.VHX_LAYOUT_FRAMEBUFFER)[0] ^ fb).all()
    # a start past the last tile: nothing
    empty, epix = tile_mask(W, H, T, 6, 2, N.VHX_LAYOUT_TILES)
    assert empty.size == 0 and epix.size == 0
    assert not tile_mask(W, H, T, 6, 2, N.VHX_LAYOUT_FRAMEBUFFER)[0].any()


@pytest.mark.parametrize("W,H,T", [(200, 136, 64), (200, 136, 24), (200, 136, 32), (64, 64, 16), (5, 3, 2), (33, 7, 8)])
@pytest.mark.parametrize("nranks,root_slots", [(1, 1), (3, 1), (2, 2), (8, 3)])
def test_counts_match_the_c_tile_plan(W, H, T, nranks, root_slots):
    """vhx_mgpu_tile_plan deals slot s the tiles s, s + slots, ...: the mask's tile counts and slot sizes are the
    plan's, the slots' owned entries cover every pixel of the frame exactly once, and the framebuffer masks partition
    the frame the same way."""
    plan = M.tile_plan(nranks, root_slots, T, W, H, 0)
    slots = plan["slots"]
    assert plan["tiles"] == plan["tiles_x"] * plan["tiles_y"] == ((W + T - 1) // T) * ((H + T - 1) // T)
    seen = np.zeros(W * H, np.int64)
    fb_seen = np.zeros(W * H, np.int64)
    counts = []
    for s in range(slots):
        owned, pixel = tile_mask(W, H, T, s, slots, N.VHX_LAYOUT_TILES)
        assert owned.size % (T * T) == 0 and owned.size == pixel.size
        counts.append(owned.size // (T * T))
        assert counts[-1] == len(range(s, plan["tiles"], slots)) <= plan["tiles_per_slot"]
        assert ((pixel >= 0) == owned).all()
        np.add.at(seen, pixel[owned], 1)
        fb, _ = tile_mask(W, H, T, s, slots, N.VHX_LAYOUT_FRAMEBUFFER)
        assert fb.shape == (W * H,) and int(fb.sum()) == int(owned.sum())
        assert set(np.flatnonzero(fb).tolist()) == set(pixel[owned].tolist())
        fb_seen += fb
    assert max(counts) == plan["tiles_per_slot"] and sum(counts) == plan["tiles"]
    assert (seen == 1).all() and (fb_seen == 1).all()
    # an entry's pixel lies in its tile, at its place inside the tile
    owned, pixel = tile_mask(W, H, T, 0, 1, N.VHX_LAYOUT_TILES)
    i = np.flatnonzero(owned)
    tile, l = i // (T * T), i % (T * T)
    assert ((pixel[i] % W) == (tile % plan["tiles_x"]) * T + l % T).all()
    assert ((pixel[i] // W) == (tile // plan["tiles_x"]) * T + l // T).all()
