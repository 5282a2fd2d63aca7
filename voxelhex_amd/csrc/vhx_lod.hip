// vhx_build_lod: the LOD image of another context's resident tree with node MIPs, computed on the device (DESIGN.md
// §8.16). The image is a pure function of the source (vhx_flat_lod, flatten.cpp, is the CPU reference, and include/vhx.h
// states the rules): BoxTree::recalculate_mips with one method and every colour-similarity threshold at 0, then
// flatten_tree(max_depth, with MIPs).
//
//   frontier  walk_and_claim  the compaction's walk over the source (treepack.hpp): reachability, breadth-first
//                             numbering, the claims of the Parted bricks, the malformed-tree flags
//   depth     k_lod_depth     per level, a wave per node of that level: depth and post-order key of its children, from
//                             the child masks and ranks the walk left
//             k_lod_check     canonical depth (leaves at the lowest level only, no occupied sectant without a child),
//                             Solid indices, and the first node of every level
//   -- readback 1: the flags and the level bounds; refusals for the source's structure happen here --
//   colours   k_lod_mip       bottom-up, one launch per level, a lane per MIP cell (brick_dim 1 and 2: 64 and 8 nodes to
//                             a wave). A cell reads its 4x4x4 samples -- voxels of a Leaf, cells of the children's
//                             finished MIPs of an Internal node; one entry and 16-byte loads from brick_dim 4 -- and
//                             stores its colour (0 = none). With thresholds of 0 a parent reads back exactly the colour
//                             its child stored, so no palette index is needed before the end. A colour the palette
//                             does not hold goes into the build's colour table with the key (post-order key of the
//                             node, place of the cell in the x-outer scan): its place in the serial order
//   palette   k_edit_pal_compact, k_pal_rank, k_edit_pal_shift   the new colours ranked by those keys (edittab.hpp)
//   cut       k_lod_binfo     per kept node (depth <= max_depth: a prefix of the breadth-first order) its Parted bricks
//                             plus its MIP brick; k_scan_*: its first new brick; k_lod_bfill: the source of every brick
//   solids    k_lod_solids, k_smp_solid_compact, k_smp_solid_rank   the kept Solid values by first (node, sectant)
//   -- readback 2: the counters; capacity refusals happen here; nothing of the destination has been written --
//   emit      k_lod_emit      types, occupancy, entries (an Internal node at max_depth keeps none), MIP descriptors
//   gather    k_cmp_gather*   the Parted bricks (treepack.hpp), leaving the MIP bricks' slots alone
//             k_lod_mipbricks the MIP bricks: every cell's colour through the table
//   derive    bitmaps, headers and child records by the tree unit's kernels (finish_upload); the descriptors are copied
//             device to device
//
// Nothing of the source is written. The atomics feed only flags, claims and minima, every index that reaches a buffer
// comes from a scan or a rank, and every global write is a plain vector store. Every index read from the source is
// checked against its count before it is used as an address.
#include <algorithm>
#include <optional>
#include <string>

#include "../../include/vhx.h"
#include "../../include/vhx_boxtree.h"
// not every shared kernel is used here (the bitmaps are derived, not gathered)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "treepack.hpp"
#include "edittab.hpp"
#pragma clang diagnostic pop
#include "ctx.hpp"
#include "treewalk.hpp"

namespace {

constexpr uint32_t BAD_DEPTH = 8u;  // the source is not of canonical depth
// Post-order key of a node: one digit per level below the root, base 65 -- the sectant on the node's path, 64 past its
// depth, so that a node follows everything below it. 65^7 < 2^43, and the key times brick_dim^3 (at most 2^15) plus
// NEW_BASE stays below 2^63.
constexpr uint32_t KEY_DIGITS = MAX_LEVELS - 1;
__host__ __device__ constexpr u64 key_weight(uint32_t digit) {  // digit 1 .. KEY_DIGITS, the first the heaviest
    u64 w = 1;
    for (uint32_t k = digit; k < KEY_DIGITS; ++k) w *= 65ull;
    return w;
}
__host__ __device__ constexpr u64 root_key() {
    u64 k = 0;
    for (uint32_t d = 1; d <= KEY_DIGITS; ++d) k += 64ull * key_weight(d);
    return k;
}

struct LodCtl {
    CompactCtl w;    // the walk's
    EditCtl e;       // e.d: the colour table's counters, seeded with the source's whole palette
    BuildCtl b;      // the table of the kept Solid values
    u64 zero_key;    // the Solid value 0: its first key, ~0 = unused
    uint32_t zero_rank, pad;
    u64 new_bricks;  // bricks of the image
    uint32_t level_begin[MAX_LEVELS];  // first node (new index) of every level, VHX_EMPTY = none
};

struct LodIn {
    const uint32_t *type;
    const u64 *ocbits;
    const uint32_t *children, *vox, *solids, *color, *data;
    uint32_t node_count, brick_count, solid_count, ncolor, ndata;
};

struct LodMaps {
    uint32_t *depth;  // [node_count] by new index
    u64 *pkey;        // [node_count]
    uint32_t *mcol;   // [reachable nodes << 3 bsh] the MIP cells' colours, 0 = none
    uint32_t *has;    // [reachable nodes] 1: a cell was sampled
    u64 *binfo, *bfirst;  // [kept nodes]
    uint32_t *bsrc;   // [bricks of the image] the old brick, VHX_EMPTY for a MIP brick
    uint32_t *mips;   // [kept nodes]
};

__global__ void k_lod_root(LodMaps lm) {
    lm.depth[0] = 0;
    lm.pkey[0] = root_key();
}

// launched over the source's node count; a wave whose node is not of level lv leaves at once
__global__ __launch_bounds__(256) void k_lod_depth(Maps m, const LodCtl *ctl, LodMaps lm, uint32_t lv, uint32_t node_count) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= min(ctl->w.end, node_count)) return;  // the whole wave
    if (lm.depth[i] != lv) return;
    const u64 mask = m.nmask[i];
    if (((mask >> lane) & 1ull) == 0) return;
    const u64 nw = 1ull + m.nrank[i] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (nw >= node_count) return;  // the walk has raised its flag
    lm.depth[nw] = lv + 1u;
    lm.pkey[nw] = lm.pkey[i] - (u64)(64u - lane) * key_weight(lv + 1u);
}

// a wave per reachable node, lane = sectant; D is the depth of the leaves of a tree of the source's sizes
__global__ __launch_bounds__(256) void k_lod_check(LodIn in, Maps m, LodMaps lm, LodCtl *ctl, uint32_t D) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= min(ctl->w.end, in.node_count)) return;  // the whole wave
    const uint32_t o = m.old_of[i];
    if (o >= in.node_count) return;  // a slot whose claim was lost: the flag is up
    const uint32_t d = lm.depth[i], ty = in.type[o];
    if (lane == 0 && d < MAX_LEVELS && (i == 0 || lm.depth[i - 1] != d)) ctl->level_begin[d] = (uint32_t)i;
    uint32_t bad = 0;
    const uint32_t e = in.children[(uint64_t)o * 64u + lane];
    if (ty == VHX_NODE_INTERNAL) {
        if (d >= D) bad = BAD_DEPTH;
        if (e == VHX_EMPTY && ((in.ocbits[o] >> lane) & 1ull)) bad = BAD_DEPTH;  // occupied, the child not in this view
    } else if (ty == VHX_NODE_LEAF || ty == VHX_NODE_UNIFORM_LEAF) {
        if (d != D) bad = BAD_DEPTH;
        if ((ty == VHX_NODE_LEAF || lane == 0) && e != VHX_EMPTY && (e & VHX_SOLID_BIT) &&
            (e & ~VHX_SOLID_BIT) >= in.solid_count)
            bad |= BAD_INDEX;
    }
    if (bad) atomicOr(&ctl->w.bad, bad);
}

// the colour of a voxel's value: the palette entry of its colour index (BoxTree::albedo_of)
__device__ __forceinline__ bool albedo_of(const LodIn &in, uint32_t v, uint32_t &c) {
    const uint32_t ci = v & 0xFFFFu;
    if (ci == 0xFFFFu || ci >= in.ncolor) return false;
    c = in.color[ci];
    return true;
}

// BoxFilter: per channel sqrt(sum(c^2) / n), min(., 255), truncated. The sums are integers below 2^24: exact in f32
__device__ __forceinline__ uint32_t box_channel(uint32_t sum, float n) {
    return (uint32_t)fminf(sqrtf((float)sum / n), 255.f) & 0xFFu;
}

template <uint32_t METHOD>
__device__ __forceinline__ uint32_t mip_pick(const uint32_t (&c)[64], u64 valid) {
    if (METHOD == VHX_MIP_BOX_FILTER) {
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) {
            const uint32_t v = (valid >> k) & 1ull ? c[k] : 0u;
            const uint32_t r = v & 0xFFu, g = (v >> 8) & 0xFFu, b = (v >> 16) & 0xFFu, a = v >> 24;
            s0 += r * r, s1 += g * g, s2 += b * b, s3 += a * a;
        }
        const float n = (float)__popcll(valid);
        return box_channel(s0, n) | (box_channel(s1, n) << 8) | (box_channel(s2, n) << 16) | (box_channel(s3, n) << 24);
    } else {
        // the most frequent colour; groups in first-seen order, the last group of the highest count wins
        u64 seen = 0;
        uint32_t best = 0, out = 0;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) {
            if (((valid & ~seen) >> k) & 1ull) {
                uint32_t cnt = 0;
                u64 eqm = 0;
#pragma unroll
                for (uint32_t j = k; j < 64; ++j) {
                    const bool eq = ((valid >> j) & 1ull) && c[j] == c[k];
                    cnt += eq ? 1u : 0u;
                    eqm |= eq ? 1ull << j : 0ull;
                }
                seen |= eqm;
                if (cnt >= best) {
                    best = cnt;
                    out = c[k];
                }
            }
        }
        return out;
    }
}

// One lane per MIP cell of the nodes [begin, end) of one level (new indices). Sample k = (dx * 4 + dy) * 4 + dz of cell
// (x, y, z) is position (4x + dx, 4y + dy, 4z + dz) of the node read as 4 * brick_dim places an edge.
template <uint32_t METHOD, uint32_t BSH>
__global__ __launch_bounds__(256) void k_lod_mip(LodIn in, Maps m, LodMaps lm, uint32_t begin, uint32_t end,
                                                 ColorTable tab, LodCtl *ctl) {
    constexpr uint32_t N3SH = 3 * BSH, BD = 1u << BSH, BDM = BD - 1u;
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = (uint64_t)begin + (gid >> N3SH);
    if (i >= end) return;
    const uint32_t f = (uint32_t)gid & ((1u << N3SH) - 1u);
    const uint32_t x = f & BDM, y = (f >> BSH) & BDM, z = f >> (2 * BSH);
    const uint32_t o = m.old_of[i];
    const uint32_t ty = o < in.node_count ? in.type[o] : VHX_NODE_NOTHING;
    uint32_t c[64];
    u64 valid = 0;
#pragma unroll
    for (uint32_t k = 0; k < 64; ++k) c[k] = 0;
    if (ty == VHX_NODE_LEAF || ty == VHX_NODE_INTERNAL) {
        const uint32_t *ent = in.children + (uint64_t)o * 64u;
        if (BSH >= 2) {  // the 64 samples lie in one sectant, in runs of 4 along x
            const uint32_t px = 4u * x, py = 4u * y, pz = 4u * z;
            const uint32_t e = ent[(px >> BSH) | ((py >> BSH) << 2) | ((pz >> BSH) << 4)];
            const uint32_t q = (px & BDM) | ((py & BDM) << BSH) | ((pz & BDM) << (2 * BSH));
            const uint32_t *cells = nullptr;
            if (ty == VHX_NODE_INTERNAL) {
                const uint32_t ch = e < in.node_count ? m.new_of[e] : VHX_EMPTY;
                if (ch != VHX_EMPTY) cells = lm.mcol + ((uint64_t)ch << N3SH) + q;
            } else if (e != VHX_EMPTY && (e & VHX_SOLID_BIT)) {
                const uint32_t idx = e & ~VHX_SOLID_BIT;
                uint32_t col;
                if (idx < in.solid_count && albedo_of(in, in.solids[idx], col)) {
                    valid = ~0ull;
#pragma unroll
                    for (uint32_t k = 0; k < 64; ++k) c[k] = col;
                }
            } else if (e < in.brick_count) {
                cells = in.vox + ((uint64_t)e << N3SH) + q;
            }
            if (cells) {
                uint4 v[16];
#pragma unroll
                for (uint32_t dy = 0; dy < 4; ++dy)
#pragma unroll
                    for (uint32_t dz = 0; dz < 4; ++dz)
                        v[dy * 4 + dz] = *(const uint4 *)(cells + (dy << BSH) + (dz << (2 * BSH)));
#pragma unroll
                for (uint32_t r = 0; r < 16; ++r) {
                    const uint32_t w[4] = {v[r].x, v[r].y, v[r].z, v[r].w};
#pragma unroll
                    for (uint32_t dx = 0; dx < 4; ++dx) {
                        const uint32_t k = dx * 16 + r;
                        bool ok;
                        uint32_t col = w[dx];
                        if (ty == VHX_NODE_INTERNAL)
                            ok = col != 0;
                        else
                            ok = !cell_empty(w[dx], in.color, in.ncolor, in.data, in.ndata) && albedo_of(in, w[dx], col);
                        if (ok) {
                            c[k] = col;
                            valid |= 1ull << k;
                        }
                    }
                }
            }
        } else {  // brick_dim 1 and 2: a cell spans 64 or 8 entries
#pragma unroll
            for (uint32_t k = 0; k < 64; ++k) {
                const uint32_t px = 4u * x + (k >> 4), py = 4u * y + ((k >> 2) & 3u), pz = 4u * z + (k & 3u);
                const uint32_t e = ent[(px >> BSH) | ((py >> BSH) << 2) | ((pz >> BSH) << 4)];
                const uint32_t q = (px & BDM) | ((py & BDM) << BSH) | ((pz & BDM) << (2 * BSH));
                bool ok = false;
                uint32_t col = 0;
                if (ty == VHX_NODE_INTERNAL) {
                    const uint32_t ch = e < in.node_count ? m.new_of[e] : VHX_EMPTY;
                    if (ch != VHX_EMPTY) {
                        col = lm.mcol[((uint64_t)ch << N3SH) + q];
                        ok = col != 0;
                    }
                } else if (e != VHX_EMPTY && (e & VHX_SOLID_BIT)) {
                    const uint32_t idx = e & ~VHX_SOLID_BIT;
                    ok = idx < in.solid_count && albedo_of(in, in.solids[idx], col);
                } else if (e < in.brick_count) {
                    const uint32_t v = in.vox[((uint64_t)e << N3SH) + q];
                    ok = !cell_empty(v, in.color, in.ncolor, in.data, in.ndata) && albedo_of(in, v, col);
                }
                if (ok) {
                    c[k] = col;
                    valid |= 1ull << k;
                }
            }
        }
    }
    if (valid == 0) return;  // the cell keeps its 0
    const uint32_t col = mip_pick<METHOD>(c, valid);
    lm.mcol[((uint64_t)i << N3SH) + f] = col;
    lm.has[i] = 1u;  // every writer stores the same word
    if (col != 0) {
        const u64 place = ((u64)x << (2 * BSH)) | ((u64)y << BSH) | z;  // the cell's turn in the x-outer scan
        color_insert(tab, &ctl->e.d, col, NEW_BASE + (lm.pkey[i] << N3SH) + place);
    }
}

// per kept node: its Parted bricks and its MIP brick (scan MODE 2 reads the low 7 bits)
__global__ __launch_bounds__(256) void k_lod_binfo(Maps m, LodMaps lm, uint32_t kept) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kept) return;
    lm.binfo[i] = (u64)__popcll(m.bmask[i]) + (lm.has[i] ? 1u : 0u);
}

// one thread per (kept node, sectant): the source of every Parted brick; the MIP bricks' slots keep VHX_EMPTY
__global__ __launch_bounds__(256) void k_lod_bfill(LodIn in, Maps m, LodMaps lm, uint32_t kept, uint64_t cap) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= kept) return;
    const u64 mask = m.bmask[i];
    if (((mask >> lane) & 1ull) == 0) return;
    const u64 j = lm.bfirst[i] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (j < cap) lm.bsrc[j] = in.children[(uint64_t)m.old_of[i] * 64u + lane];  // bmask: a node inside the count
}

// a wave per kept node, lane = sectant: the Solid values the image will hold, each with its first key
__global__ __launch_bounds__(256) void k_lod_solids(LodIn in, Maps m, uint32_t kept, ColorTable stab, LodCtl *ctl) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= kept) return;  // the whole wave
    const uint32_t o = m.old_of[i];
    const uint32_t ty = in.type[o];
    uint32_t v = 0;
    bool cand = false;
    if (ty == VHX_NODE_LEAF || (ty == VHX_NODE_UNIFORM_LEAF && lane == 0)) {
        const uint32_t e = in.children[(uint64_t)o * 64u + lane];
        if (e != VHX_EMPTY && (e & VHX_SOLID_BIT) && (e & ~VHX_SOLID_BIT) < in.solid_count) {
            v = in.solids[e & ~VHX_SOLID_BIT];
            cand = true;
        }
    }
    u64 pending = __ballot(cand);
    while (pending) {  // the same in every lane: the lowest sectant of a value records it for the node
        const uint32_t leader = (uint32_t)__ffsll((long long)pending) - 1u;
        const uint32_t lv = __shfl(v, leader);
        if (lane == leader) solid_insert(stab, ctl, v, (u64)i * 64ull + lane);
        pending &= ~__ballot(cand && v == lv);
    }
}

// one thread per (kept node, sectant); runs only for a source that passed the checks
__global__ __launch_bounds__(256) void k_lod_emit(LodIn in, Maps m, LodMaps lm, ColorTable stab, const LodCtl *ctl,
                                                  uint32_t kept, uint32_t max_depth, uint32_t *type, u64 *ocbits,
                                                  uint32_t *children) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = gid >> 6;
    const uint32_t s = (uint32_t)gid & 63u;
    if (i >= kept) return;
    const uint32_t o = m.old_of[i];
    const uint32_t ty = in.type[o];
    const u64 mask = m.bmask[i];
    if (s == 0) {
        type[i] = ty;
        ocbits[i] = in.ocbits[o];
        lm.mips[i] = lm.has[i] ? (uint32_t)lm.bfirst[i] + (uint32_t)__popcll(mask) : VHX_EMPTY;
    }
    const uint32_t e = in.children[(uint64_t)o * 64u + s];
    uint32_t child = VHX_EMPTY;
    if (ty == VHX_NODE_INTERNAL) {
        if (e != VHX_EMPTY && lm.depth[i] < max_depth) child = m.new_of[e];
    } else if (ty == VHX_NODE_LEAF || (ty == VHX_NODE_UNIFORM_LEAF && s == 0)) {
        if ((mask >> s) & 1ull) {
            child = (uint32_t)lm.bfirst[i] + (uint32_t)__popcll(mask & ((1ull << s) - 1ull));
        } else if (e != VHX_EMPTY) {  // Solid, its index checked by k_lod_check
            const uint32_t v = in.solids[e & ~VHX_SOLID_BIT];
            child = VHX_SOLID_BIT | (v == 0 ? ctl->zero_rank : color_lookup(stab, v));
        }
    }
    children[gid] = child;
}

// one thread per cell of the kept nodes' MIP bricks: pix_visual(palette index of the colour), VHX_EMPTY for none
__global__ __launch_bounds__(256) void k_lod_mipbricks(LodMaps lm, ColorTable tab, uint32_t kept, uint32_t n3sh,
                                                       uint32_t *voxels) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = gid >> n3sh;
    if (i >= kept) return;
    const uint32_t b = lm.mips[i];
    if (b == VHX_EMPTY) return;
    const uint32_t f = (uint32_t)gid & ((1u << n3sh) - 1u);
    const uint32_t col = lm.mcol[gid];
    voxels[((uint64_t)b << n3sh) + f] = col == 0 ? VHX_EMPTY : 0xFFFF0000u | color_lookup(tab, col);
}

template <uint32_t METHOD>
void launch_mip(vhx_ctx *c, uint32_t bsh, const LodIn &in, const Maps &m, const LodMaps &lm, uint32_t begin,
                uint32_t end, const ColorTable &tab, LodCtl *ctl) {
    const unsigned blocks = blocks_for((uint64_t)(end - begin) << (3 * bsh));
    switch (bsh) {
        case 0: k_lod_mip<METHOD, 0><<<blocks, 256, 0, c->stream>>>(in, m, lm, begin, end, tab, ctl); break;
        case 1: k_lod_mip<METHOD, 1><<<blocks, 256, 0, c->stream>>>(in, m, lm, begin, end, tab, ctl); break;
        case 2: k_lod_mip<METHOD, 2><<<blocks, 256, 0, c->stream>>>(in, m, lm, begin, end, tab, ctl); break;
        case 3: k_lod_mip<METHOD, 3><<<blocks, 256, 0, c->stream>>>(in, m, lm, begin, end, tab, ctl); break;
        case 4: k_lod_mip<METHOD, 4><<<blocks, 256, 0, c->stream>>>(in, m, lm, begin, end, tab, ctl); break;
        default: k_lod_mip<METHOD, 5><<<blocks, 256, 0, c->stream>>>(in, m, lm, begin, end, tab, ctl); break;
    }
}

struct LodFill {
    vhx_ctx *c;
    const TreeStore *src;
    LodIn in;
    Maps m;
    LodMaps lm;
    ColorTable tab, stab;
    LodCtl *ctl;
    uint32_t kept, max_depth, n3sh, added;
};

// the seven raw buffers of the image, on c's stream
int fill_image(const LodFill &a, const vhx_tree_desc &counts) {
    vhx_ctx *c = a.c;
    const TreeStore &ts = *c->tree;
    const uint64_t n3 = 1ull << a.n3sh;
    k_lod_emit<<<blocks_for((uint64_t)a.kept * 64), 256, 0, c->stream>>>(
        a.in, a.m, a.lm, a.stab, a.ctl, a.kept, a.max_depth, (uint32_t *)ts.raw[VHX_BUF_NODE_TYPE].ptr,
        (u64 *)ts.raw[VHX_BUF_NODE_OCBITS].ptr, (uint32_t *)ts.raw[VHX_BUF_NODE_CHILDREN].ptr);
    if (counts.brick_count) {
        gather_voxels<true>(c, a.src->raw[VHX_BUF_VOXELS].ptr, ts.raw[VHX_BUF_VOXELS].ptr, a.lm.bsrc, counts.brick_count,
                            n3);
        k_lod_mipbricks<<<blocks_for((uint64_t)a.kept << a.n3sh), 256, 0, c->stream>>>(
            a.lm, a.tab, a.kept, a.n3sh, (uint32_t *)ts.raw[VHX_BUF_VOXELS].ptr);
    }
    VHX_HIP(c, hipGetLastError());
    if (counts.solid_count)
        VHX_HIP(c, hipMemcpyAsync(ts.raw[VHX_BUF_SOLID_VALUES].ptr, a.stab.pal, (uint64_t)counts.solid_count * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
    const uint32_t old_colors = counts.color_count - a.added;
    if (old_colors)
        VHX_HIP(c, hipMemcpyAsync(ts.raw[VHX_BUF_COLOR_PALETTE].ptr, a.src->raw[VHX_BUF_COLOR_PALETTE].ptr,
                                  (uint64_t)old_colors * 4, hipMemcpyDeviceToDevice, c->stream));
    if (a.added)
        VHX_HIP(c, hipMemcpyAsync((uint32_t *)ts.raw[VHX_BUF_COLOR_PALETTE].ptr + old_colors, a.tab.pal,
                                  (uint64_t)a.added * 4, hipMemcpyDeviceToDevice, c->stream));
    if (counts.data_count)
        VHX_HIP(c, hipMemcpyAsync(ts.raw[VHX_BUF_DATA_PALETTE].ptr, a.src->raw[VHX_BUF_DATA_PALETTE].ptr,
                                  (uint64_t)counts.data_count * 4, hipMemcpyDeviceToDevice, c->stream));
    return VHX_OK;
}

// the call between its scopes: src's tree is held for reading, c's for writing, and c's stream follows src's last write
int build_lod(vhx_ctx *c, const vhx_ctx *src, uint32_t max_depth, uint32_t method, uint32_t D, uint32_t *nodes,
              uint32_t *bricks, uint32_t *colors_added) {
    const TreeStore &ss = *src->tree;
    const vhx_tree_desc d = ss.desc;
    const uint64_t nn = d.node_count, nb = d.brick_count;
    const uint32_t bsh = lg2(d.brick_dim), n3sh = 3 * bsh;
    int rc;
    Maps m;
    CompactCtl *own_ctl;  // the compaction's counters; the walk here counts in LodCtl::w
    if ((rc = ensure_maps(c, nn, nb, &m, &own_ctl))) return rc;
    vhx_ctx::LodScratch &ls = c->lod;
    if ((rc = vhx::ensure(c, ls.depth, nn * 4))) return rc;
    if ((rc = vhx::ensure(c, ls.pkey, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, ls.ctl, sizeof(LodCtl)))) return rc;
    if ((rc = vhx::ensure(c, c->build.table, TAB_BYTES))) return rc;
    if ((rc = vhx::ensure(c, c->build.dtable, TAB_BYTES))) return rc;
    LodCtl *ctl = (LodCtl *)ls.ctl.ptr;
    const ColorTable tab = table_of(c->build.table.ptr), stab = table_of(c->build.dtable.ptr);
    const OldTree t{(const uint32_t *)ss.raw[VHX_BUF_NODE_TYPE].ptr, (const u64 *)ss.raw[VHX_BUF_NODE_OCBITS].ptr,
                    (const uint32_t *)ss.raw[VHX_BUF_NODE_CHILDREN].ptr, d.node_count, d.brick_count};
    const LodIn in{t.type, t.ocbits, t.children,
                   (const uint32_t *)ss.raw[VHX_BUF_VOXELS].ptr,
                   (const uint32_t *)ss.raw[VHX_BUF_SOLID_VALUES].ptr,
                   (const uint32_t *)ss.raw[VHX_BUF_COLOR_PALETTE].ptr,
                   (const uint32_t *)ss.raw[VHX_BUF_DATA_PALETTE].ptr,
                   d.node_count, d.brick_count, d.solid_count, d.color_count, d.data_count};
    LodMaps lm{};
    lm.depth = (uint32_t *)ls.depth.ptr;
    lm.pkey = (u64 *)ls.pkey.ptr;

    // reachability, depth, structure
    VHX_HIP(c, hipMemsetAsync(ctl, 0, sizeof(LodCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(&ctl->zero_key, 0xFF, sizeof(u64), c->stream));
    VHX_HIP(c, hipMemsetAsync(ctl->level_begin, 0xFF, sizeof(ctl->level_begin), c->stream));
    VHX_HIP(c, hipMemsetAsync(lm.depth, 0xFF, nn * 4, c->stream));
    if ((rc = walk_and_claim(c, t, m, &ctl->w, false))) return rc;  // (resets ctl->w itself)
    k_lod_root<<<1, 1, 0, c->stream>>>(lm);
    for (uint32_t lv = 0; lv + 1 < MAX_LEVELS; ++lv)
        k_lod_depth<<<blocks_for(nn * 64), 256, 0, c->stream>>>(m, ctl, lm, lv, d.node_count);
    k_lod_check<<<blocks_for(nn * 64), 256, 0, c->stream>>>(in, m, lm, ctl, D);
    VHX_HIP(c, hipGetLastError());
    LodCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.w.bad & BAD_INDEX)
        return fail(c, VHX_E_STATE, "vhx_build_lod: a child, brick or solid value index of the source at or past its count");
    if (h.w.bad & BAD_TWICE) return fail(c, VHX_E_STATE, "vhx_build_lod: a node or Parted brick of the source is reached twice");
    if (h.w.bad & BAD_DEEP) return fail(c, VHX_E_STATE, "vhx_build_lod: more than 8 node levels in the source");
    if (h.w.end == 0 || h.w.end > nn || h.w.brick_total > nb)
        return fail(c, VHX_E_STATE, "vhx_build_lod: inconsistent counts in the source");
    if (h.w.bad & BAD_DEPTH)
        return fail(c, VHX_E_STATE, "vhx_build_lod: the source is not of canonical depth (a LOD-cut or streamed view, or "
                                    "a leaf whose edge is not 4 * brick_dim)");
    const uint32_t reach = h.w.end;
    uint32_t lbegin[MAX_LEVELS + 1];  // level lv is [lbegin[lv], lbegin[lv + 1])
    lbegin[MAX_LEVELS] = reach;
    for (uint32_t lv = MAX_LEVELS; lv-- > 0;)
        lbegin[lv] = h.level_begin[lv] == VHX_EMPTY ? lbegin[lv + 1] : std::min(h.level_begin[lv], lbegin[lv + 1]);
    const uint32_t kept = lbegin[std::min(max_depth, MAX_LEVELS - 1) + 1];

    // MIP colours, bottom-up
    const uint64_t bsrc_cap = h.w.brick_total + kept;
    if ((rc = vhx::ensure(c, ls.mcol, ((uint64_t)reach << n3sh) * 4))) return rc;
    if ((rc = vhx::ensure(c, ls.has, (uint64_t)reach * 4))) return rc;
    if ((rc = vhx::ensure(c, ls.binfo, (uint64_t)kept * 8))) return rc;
    if ((rc = vhx::ensure(c, ls.bfirst, (uint64_t)kept * 8))) return rc;
    if ((rc = vhx::ensure(c, ls.bsrc, bsrc_cap * 4))) return rc;
    if ((rc = vhx::ensure(c, ls.mips, (uint64_t)kept * 4))) return rc;
    lm.mcol = (uint32_t *)ls.mcol.ptr;
    lm.has = (uint32_t *)ls.has.ptr;
    lm.binfo = (u64 *)ls.binfo.ptr;
    lm.bfirst = (u64 *)ls.bfirst.ptr;
    lm.bsrc = (uint32_t *)ls.bsrc.ptr;
    lm.mips = (uint32_t *)ls.mips.ptr;
    VHX_HIP(c, hipMemsetAsync(lm.mcol, 0, ((uint64_t)reach << n3sh) * 4, c->stream));
    VHX_HIP(c, hipMemsetAsync(lm.has, 0, (uint64_t)reach * 4, c->stream));
    VHX_HIP(c, hipMemsetAsync(lm.bsrc, 0xFF, bsrc_cap * 4, c->stream));
    for (const ColorTable *tb : {&tab, &stab}) {
        VHX_HIP(c, hipMemsetAsync(tb->keys, 0, TAB_KEYS_BYTES, c->stream));
        VHX_HIP(c, hipMemsetAsync(tb->vals, 0xFF, TAB_VALS_BYTES, c->stream));
    }
    // the whole palette, entries of alpha 0 included: a MIP colour may equal one (the data flavour skips only the word 0)
    k_edit_seed<1><<<blocks_for(std::max(d.color_count, 1u)), 256, 0, c->stream>>>(tab, in.color, d.color_count, &ctl->e);
    const bool stamped = hipEventRecord(c->ev0, c->stream) == hipSuccess;  // vhx_sync reports the colour passes
    for (uint32_t lv = MAX_LEVELS; lv-- > 0;) {
        if (lbegin[lv] == lbegin[lv + 1]) continue;
        if (method == VHX_MIP_BOX_FILTER)
            launch_mip<VHX_MIP_BOX_FILTER>(c, bsh, in, m, lm, lbegin[lv], lbegin[lv + 1], tab, ctl);
        else
            launch_mip<VHX_MIP_POINT_FILTER>(c, bsh, in, m, lm, lbegin[lv], lbegin[lv + 1], tab, ctl);
    }
    c->timed = hipEventRecord(c->ev1, c->stream) == hipSuccess && stamped;
    k_edit_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(tab, &ctl->e.d);
    k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->e.d);
    k_edit_pal_shift<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->e.d, d.color_count);
    // the cut: bricks and Solid values of the kept nodes
    k_lod_binfo<<<blocks_for(kept), 256, 0, c->stream>>>(m, lm, kept);
    if ((rc = scan_level<2>(c, lm.binfo, kept, false, lm.bfirst, &ctl->new_bricks))) return rc;
    k_lod_bfill<<<blocks_for((uint64_t)kept * 64), 256, 0, c->stream>>>(in, m, lm, kept, bsrc_cap);
    k_lod_solids<<<blocks_for((uint64_t)kept * 64), 256, 0, c->stream>>>(in, m, kept, stab, ctl);
    k_smp_solid_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(stab, ctl);
    k_smp_solid_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(stab, ctl);
    VHX_HIP(c, hipGetLastError());

    // the second readback; neither tree has been written
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    const BuildCtl &cc = h.e.d;
    if (cc.overflow || cc.ncolors > MAX_COLORS || cc.ncompact != cc.ncolors - d.color_count)
        return fail(c, VHX_E_CAPACITY, "vhx_build_lod: more than 65535 colours with the MIP colours");
    const uint64_t solids = (uint64_t)h.b.ncolors + (h.zero_key != ~0ull ? 1u : 0u);
    if (h.b.overflow || solids > MAX_COLORS || h.b.ncompact != h.b.ncolors)
        return fail(c, VHX_E_CAPACITY, "vhx_build_lod: more than 65535 distinct Solid values");
    if (h.new_bricks >= (1ull << 31)) return fail(c, VHX_E_CAPACITY, "vhx_build_lod: 2^31 bricks or more");
    if (h.new_bricks > bsrc_cap) return fail(c, VHX_E_STATE, "vhx_build_lod: inconsistent counts");
    vhx_tree_desc counts{};
    counts.boxtree_size = d.boxtree_size;
    counts.brick_dim = d.brick_dim;
    counts.node_count = kept;
    counts.brick_count = (uint32_t)h.new_bricks;
    counts.solid_count = (uint32_t)solids;
    counts.color_count = cc.ncolors;
    counts.data_count = d.data_count;

    // the image into c's tree, as an upload fills it; from here on a failure is a HIP error
    if ((rc = vhx::alloc_tree(c, &counts))) return rc;
    const LodFill fa{c, &ss, in, m, lm, tab, stab, ctl, kept, max_depth, n3sh, cc.ncompact};
    if ((rc = fill_image(fa, counts))) return rc;
    if ((rc = vhx::finish_upload(c))) return rc;  // derived layout (synchronises)
    if ((rc = vhx::ensure(c, c->tree->mips, (uint64_t)kept * 4))) return rc;
    VHX_HIP(c, hipMemcpyAsync(c->tree->mips.ptr, lm.mips, (uint64_t)kept * 4, hipMemcpyDeviceToDevice, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    c->tree->mips_on = true;
    *nodes = kept;
    *bricks = counts.brick_count;
    *colors_added = cc.ncompact;
    return VHX_OK;
}

}  // namespace

extern "C" {

int vhx_build_lod(vhx_ctx *dst, vhx_ctx *src, uint32_t max_depth, uint32_t method, uint32_t *nodes, uint32_t *bricks,
                  uint32_t *colors_added) {
    if (!dst) return VHX_E_INVALID_ARG;
    if (!src || !nodes || !bricks || !colors_added) return fail(dst, VHX_E_INVALID_ARG, "vhx_build_lod: null argument");
    if (method != VHX_MIP_BOX_FILTER && method != VHX_MIP_POINT_FILTER)
        return fail(dst, VHX_E_INVALID_ARG, "vhx_build_lod: the method is neither VHX_MIP_BOX_FILTER nor VHX_MIP_POINT_FILTER");
    if (dst->tree == src->tree) return fail(dst, VHX_E_INVALID_ARG, "vhx_build_lod: dst and src hold the same tree");
    if (dst->device != src->device) return fail(dst, VHX_E_INVALID_ARG, "vhx_build_lod: dst and src are on different devices");
    if (dst->shared) return fail(dst, VHX_E_STATE, "vhx_build_lod into a shared context: build through the owner");
    if (dst->shadow_on) return fail(dst, VHX_E_STATE, "vhx_build_lod into a context with a shadow light: no node MIPs with a light set");

    VHX_HIP(dst, hipSetDevice(dst->device));
    VHX_STREAM(dst);
    if (!src->stream) {  // VHX_STREAM for src, its error reported on dst
        if (!src->own_stream) VHX_HIP(dst, hipStreamCreateWithFlags(&src->own_stream, hipStreamNonBlocking));
        src->stream = src->own_stream;
    }
    // src is held as a trace holds it, dst as a write; two calls that cross (A into B, B into A) take the trees in one
    // order, so neither waits for the other with a tree in hand
    std::optional<vhx::TraceScope> rs;
    std::optional<vhx::WriteScope> ws;
    int rc;
    if (src->tree.get() < dst->tree.get()) {
        rs.emplace(src);
        if ((rc = rs->rc)) return fail(dst, rc, src->err);
        ws.emplace(dst);
        if ((rc = ws->rc)) return rc;
    } else {
        ws.emplace(dst);
        if ((rc = ws->rc)) return rc;
        rs.emplace(src);
        if ((rc = rs->rc)) return fail(dst, rc, src->err);
    }
    // the source as of now, under the scope
    if (!src->tree->uploaded)
        return fail(dst, VHX_E_STATE, "vhx_build_lod: src has no tree");
    if (src->tree->mips_on) return fail(dst, VHX_E_STATE, "vhx_build_lod: src has node MIPs set");
    const vhx_tree_desc &d = src->tree->desc;
    const uint32_t bd = d.brick_dim, S = d.boxtree_size;
    uint32_t D = 0;
    while (D < MAX_LEVELS && ((uint64_t)bd << (2 * (D + 1))) < S) ++D;
    if (bd == 0 || (bd & (bd - 1)) != 0 || bd > 32 || D >= MAX_LEVELS || ((uint64_t)bd << (2 * (D + 1))) != S)
        return fail(dst, VHX_E_STATE, "vhx_build_lod: the size of src is not brick_dim * 4^k, or it has more than 8 levels");
    // dst's stream follows src's last write (src's stream already does: trace_begin)
    if (src->stream != dst->stream) {
        hipEvent_t ev = nullptr;
        VHX_HIP(dst, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, src->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst->stream, ev, 0);
        (void)hipEventDestroy(ev);
        VHX_HIP(dst, e);
    }
    rc = build_lod(dst, src, max_depth, method, D, nodes, bricks, colors_added);
    // whatever was enqueued has read src before its scope ends
    const hipError_t e = hipStreamSynchronize(dst->stream);
    if (rc) return rc;
    VHX_HIP(dst, e);
    if ((rc = rs->end())) return fail(dst, rc, src->err);
    return ws->end();  // the next trace of every context of dst's tree waits for this write
}

}  // extern "C"
