// What the two in-place writes share (vhx_edit.hip: a dense box; vhx_points.hip: a list of points): the counters read
// back, the view of the tree's buffers, the seeding of the colour and data tables from the resident palettes, and the
// compaction and shift of the new values around k_pal_rank (buildtab.hpp).
// Each unit that includes this gets its own copy of the kernels (anonymous namespace).
#pragma once
#include "../../include/vhx.h"
#include "buildtab.hpp"
#include "ctx.hpp"

namespace {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr u64 NEW_BASE = 1ull << 32;  // first indices of the write's colours: above every palette index

struct EditCtl {
    BuildCtl b;  // level_total: new nodes per level; brick_total: new bricks; ncolors starts at the palette's count
    uint32_t bad;  // the tree under the write is not of canonical depth
    uint32_t orphan_nodes, orphan_bricks;
    uint32_t pad;
    BuildCtl d;  // writes with data: the data table's ncolors (starts at data_count), overflow and ncompact
};

struct TreeP {
    uint32_t *type;
    u64 *ocbits;
    uint32_t *children, *voxels;
    const uint32_t *solid, *color, *data;
    uint4 *hdr;
    u64 *occ;
    uint4 *rec;  // null above brick_dim 4
    uint32_t node_count, brick_count, solid_count, color_count, data_count, occ_words;  // before the write
};

// DATA = 1 seeds the data table from data_palette: an entry equal to 0 is skipped (0 is the free key, and a written data
// value is never 0)
template <int DATA>
__global__ __launch_bounds__(256) void k_edit_seed(ColorTable t, const uint32_t *pal, uint32_t n, EditCtl *ctl) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) (DATA ? ctl->d : ctl->b).ncolors = n;  // the leaf pass counts the claims of new values on top
    if (i >= n) return;
    const uint32_t c = pal[i];
    if (DATA ? c == 0 : (c >> 24) == 0) return;  // never looked up: a written voxel's colour has a non-zero alpha byte
    uint32_t h = color_hash(c);
    for (uint32_t probe = 0; probe < TAB_SLOTS; ++probe, h = (h + 1) & TAB_MASK) {
        uint32_t k = t.keys[h];
        if (k == 0) {
            k = atomicCAS(&t.keys[h], 0u, c);
            if (k == 0) k = c;
        }
        if (k == c) {
            atomicMin(&t.vals[h], (u64)i);  // a colour the palette holds twice: its lowest index
            return;
        }
    }
}

// the new colours of the table (first index at or above NEW_BASE), compacted for k_pal_rank; `b` is the table's counters
__global__ __launch_bounds__(256) void k_edit_pal_compact(ColorTable t, BuildCtl *b) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= TAB_SLOTS) return;
    const uint32_t k = t.keys[h];
    if (k == 0 || t.vals[h] < NEW_BASE) return;
    const uint32_t pos = atomicAdd(&b->ncompact, 1u);  // any order: the ranks come from the first indices
    if (pos >= PAL_CAP) return;
    t.ckey[pos] = k;
    t.cidx[pos] = t.vals[h];
    t.cslot[pos] = h;
}

// k_pal_rank left each new colour's rank among the new ones in its slot: its palette index is color_count further
__global__ __launch_bounds__(256) void k_edit_pal_shift(ColorTable t, const BuildCtl *b, uint32_t color_count) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= min(b->ncompact, PAL_CAP)) return;
    t.vals[t.cslot[i]] += color_count;
}

TreeP tree_of(const vhx_ctx *c, const vhx_tree_desc &d) {
    const TreeStore &s = *c->tree;
    TreeP t{};
    t.type = (uint32_t *)s.raw[VHX_BUF_NODE_TYPE].ptr;
    t.ocbits = (u64 *)s.raw[VHX_BUF_NODE_OCBITS].ptr;
    t.children = (uint32_t *)s.raw[VHX_BUF_NODE_CHILDREN].ptr;
    t.voxels = (uint32_t *)s.raw[VHX_BUF_VOXELS].ptr;
    t.solid = (const uint32_t *)s.raw[VHX_BUF_SOLID_VALUES].ptr;
    t.color = (const uint32_t *)s.raw[VHX_BUF_COLOR_PALETTE].ptr;
    t.data = (const uint32_t *)s.raw[VHX_BUF_DATA_PALETTE].ptr;
    t.hdr = (uint4 *)s.hdr.ptr;
    t.occ = (u64 *)s.brick_occ.ptr;
    t.rec = d.brick_dim * d.brick_dim * d.brick_dim <= 64 ? (uint4 *)s.child_rec.ptr : nullptr;
    t.node_count = d.node_count;
    t.brick_count = d.brick_count;
    t.solid_count = d.solid_count;
    t.color_count = d.color_count;
    t.data_count = d.data_count;
    t.occ_words = s.occ_words;
    return t;
}

}  // namespace
