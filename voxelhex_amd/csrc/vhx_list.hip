// vhx_list_voxels: the occupied voxels of a box of the device tree as a list. The sparse form of
// vhx_read_dense_data and the inverse of vhx_set_voxels; vhx_flat_list_voxels (flatten.cpp) is the CPU reference.
//
// Kernels
//   k_list_seed      the root as the first frontier, the counters cleared
//   k_list_mask      one wave per frontier node, one lane per sectant: the 64-bit mask of the sectants that meet the box
//                    and hold something (a child node; at the smallest leaf level a brick), by __ballot
//   k_dscan_*        buildtab.hpp's u64 scans with the element count read on the device: the popcounts of the masks give
//                    every child its place ("by their parent's order, then by sectant", as vhx_points.hip orders its
//                    touched cubes), the voxel counts of the units every unit its first rank
//   k_list_push      the surviving children into the next frontier; at the smallest leaf level the brick-sized units
//   k_list_units     one wave per unit over its brick_dim^3 voxels in flat order, 64 at a time: COUNT ballots and
//                    popcounts the listed voxels, EMIT stores those whose rank is below the capacity
// Host side: vhx_list_voxels. Ordered like a trace (TraceScope); the tree is only read, every global store goes to the
// scratch or the caller's arrays, and no atomic decides a place: every rank comes from a scan or a ballot.
//
// The list order is the depth-first order of the canonical tree, which is what a level-by-level descent that keeps each
// frontier in (parent's order, sectant) order produces without ever forming the key. The element counts of the levels
// stay on the device (launches are sized by bounds and stride up to the count they read), so the call has one readback:
// the counters with the total, ahead of the emit pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/vhx.h"
// of buildtab.hpp only the scans with a device-side count (k_dscan_*) are used here
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "buildtab.hpp"
#pragma clang diagnostic pop
#include "ctx.hpp"
#include "trace.hpp"
#include "treewalk.hpp"

using namespace vhx;

namespace {

constexpr uint32_t LIST_MAX_LEVELS = 12;  // a device tree is at most 2^24 wide: 12 node levels at brick_dim 1

struct LShape {
    uint32_t lg_size, lg_bd;
    uint32_t levels;  // node levels: the root is level 0, the smallest leaf (4 * brick_dim wide) level levels - 1
    uint32_t brick_count, solid_count;
    uint32_t dcount;
    const uint32_t *dpal;  // the tree's data_palette
};

struct LBox {
    uint32_t ox, oy, oz, gx, gy, gz;
};

// the counters, read back once
struct LCtl {
    u64 count[LIST_MAX_LEVELS + 1];  // frontier nodes per level; count[levels]: the units
    u64 total;                       // listed voxels
    uint32_t bad;                    // a Leaf or UniformLeaf above the smallest leaf level
    uint32_t overflow;               // more survivors than a tree's nodes can have: the image is not a tree
};

struct LOut {
    uint32_t *pos, *albedo, *data;
    u64 capacity;
};

// what vhx_read_dense_data writes for a value (vhx_query.hip): the colour, unless none, out of the palette or transparent
__device__ __forceinline__ uint32_t list_albedo(const DevTree &t, uint32_t v) {
    const uint32_t ci = v & 0xFFFFu;
    if (ci == 0xFFFFu || ci >= t.color_count) return 0u;
    const uint32_t a = t.color[ci];
    return (a >> 24) != 0u ? a : 0u;
}
// ... and the data value, unless the value is VHX_EMPTY or the index none or out of the palette
__device__ __forceinline__ uint32_t list_data(const LShape &q, uint32_t v) {
    const uint32_t di = v >> 16;
    if (v == VHX_EMPTY || di == 0xFFFFu || di >= q.dcount) return 0u;
    return q.dpal[di];
}

__global__ void __launch_bounds__(64) k_list_seed(uint4 *fr, LCtl *ctl) {
    uint32_t *w = (uint32_t *)ctl;
    for (uint32_t i = threadIdx.x; i < sizeof(LCtl) / 4u; i += 64u) w[i] = (i == 0u) ? 1u : 0u;  // count[0] = 1
    if (threadIdx.x == 0) fr[0] = make_uint4(0u, 0u, 0u, 0u);
}

// Sectant s of frontier node f = {node, x, y, z} (2^lg wide, at level lv): does it meet the box and hold something?
// *origin receives the sectant's cube, *stretched whether the node is a Leaf or UniformLeaf above the smallest leaf level.
__device__ __forceinline__ bool sectant_live(const DevTree &t, const LShape &q, const LBox &b, uint4 f, uint32_t s,
                                             uint32_t lg, uint32_t lv, uint4 *child, bool *stretched) {
    const uint32_t el = lg - 2u, edge = 1u << el;
    const uint32_t x = f.y + ((s & 3u) << el), y = f.z + (((s >> 2) & 3u) << el), z = f.w + ((s >> 4) << el);
    const bool meets = x < b.ox + b.gx && x + edge > b.ox && y < b.oy + b.gy && y + edge > b.oy && z < b.oz + b.gz &&
                       z + edge > b.oz;
    const uint32_t type = ((const uint32_t *)&t.hdr[f.x])[2];
    const bool last = lv + 1u == q.levels;
    *stretched = false;
    if (type == VHX_NODE_INTERNAL) {
        if (last || !meets) return false;  // no node is smaller than 4 * brick_dim
        const uint32_t e = t.children[(uint64_t)f.x * 64u + s];
        *child = make_uint4(e, x, y, z);
        return e != VHX_EMPTY && e < t.node_count;  // an empty sectant, or a child that is not in this view
    }
    if (type != VHX_NODE_LEAF && type != VHX_NODE_UNIFORM_LEAF) return false;
    if (!last) {
        *stretched = true;
        return false;
    }
    if (!meets) return false;
    const uint32_t desc = t.children[(uint64_t)f.x * 64u + (type == VHX_NODE_UNIFORM_LEAF ? 0u : s)];
    *child = make_uint4(f.x, x, y, z);  // a unit: the leaf and the brick-sized cube of its sectant
    return desc != VHX_EMPTY;
}

__global__ void __launch_bounds__(256) k_list_mask(DevTree t, LShape q, LBox b, const uint4 *__restrict__ fr, LCtl *ctl,
                                                   uint32_t lv, u64 cap, u64 *__restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u, lg = q.lg_size - 2u * lv;
    const u64 n = min(ctl->count[lv], cap), stride = (u64)gridDim.x * 4u;
    for (u64 i = (u64)blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += stride) {
        uint4 child;
        bool stretched;
        const bool live = sectant_live(t, q, b, fr[i], lane, lg, lv, &child, &stretched);
        const u64 m = __ballot(live);
        if (lane == 0) {
            mask[i] = m;
            if (stretched) ctl->bad = 1u;
        }
    }
}

__global__ void __launch_bounds__(256) k_list_push(DevTree t, LShape q, LBox b, const uint4 *__restrict__ fr, LCtl *ctl,
                                                   uint32_t lv, u64 cap, const u64 *__restrict__ mask,
                                                   const u64 *__restrict__ first, uint4 *__restrict__ next, u64 cap_next) {
    const uint32_t lane = threadIdx.x & 63u, lg = q.lg_size - 2u * lv;
    const u64 n = min(ctl->count[lv], cap), stride = (u64)gridDim.x * 4u;
    for (u64 i = (u64)blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += stride) {
        const u64 m = mask[i];
        if (((m >> lane) & 1ull) == 0ull) continue;
        uint4 child;
        bool stretched;
        (void)sectant_live(t, q, b, fr[i], lane, lg, lv, &child, &stretched);
        const u64 at = first[i] + (u64)__popcll(m & ((1ull << lane) - 1ull));
        if (at < cap_next)
            next[at] = child;
        else
            ctl->overflow = 1u;
    }
}

// A unit is the brick-sized cube of one sectant of a smallest leaf: a Leaf's Parted or Solid brick, or a 64th of the
// cube a UniformLeaf's brick spans (its cells are then 4 voxels wide, and read raw). One wave walks the unit's voxels in
// flat order, 64 at a time with wave-uniform bounds; the unit's record, brick descriptor, Solid value and first rank are
// wave-uniform and live in scalar registers. COUNT: ucnt[u] = the unit's listed voxels. EMIT: ucnt[u] is the unit's first
// rank (the scan ran in place), a listed voxel's rank is that plus the listed voxels before it in the unit, and the
// voxels whose rank is below the capacity are stored.
template <bool EMIT>
__global__ void __launch_bounds__(256) k_list_units(DevTree t, LShape q, LBox b, const uint4 *__restrict__ unit, u64 nunits,
                                                    const LCtl *ctl, u64 cap_units, u64 *ucnt, LOut o) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bd = 1u << q.lg_bd, m = bd - 1u, nvox = 1u << (3u * q.lg_bd);
    const u64 n = EMIT ? nunits : min(ctl->count[q.levels], cap_units), stride = (u64)gridDim.x * 4u;
    const u64 w0 = (u64)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (u64 u = w0; u < n; u += stride) {
        const uint32_t *rec = (const uint32_t *)&unit[u];
        const uint32_t node = __builtin_amdgcn_readfirstlane(uload(rec)), X = __builtin_amdgcn_readfirstlane(uload(rec + 1)),
                       Y = __builtin_amdgcn_readfirstlane(uload(rec + 2)), Z = __builtin_amdgcn_readfirstlane(uload(rec + 3));
        u64 base = 0;
        if (EMIT) {
            const u64 r = ucnt[u];
            base = ((u64)__builtin_amdgcn_readfirstlane((uint32_t)(r >> 32)) << 32) |
                   __builtin_amdgcn_readfirstlane((uint32_t)r);
            if (base >= o.capacity) continue;  // nothing of this unit is within the capacity
        }
        const uint32_t type = __builtin_amdgcn_readfirstlane(uload((const uint32_t *)&t.hdr[node] + 2));
        const bool uniform = type == VHX_NODE_UNIFORM_LEAF;
        const uint32_t s = uniform ? 0u : sectant_of(X, Y, Z, q.lg_bd + 2u);
        const uint32_t desc = __builtin_amdgcn_readfirstlane(uload(&t.children[(uint64_t)node * 64u + s]));
        const bool solid = (desc & VHX_SOLID_BIT) != 0u;
        uint32_t sv = VHX_EMPTY;
        if (solid) {
            const uint32_t i = desc & 0x7FFFFFFFu;
            if (desc != VHX_EMPTY && i < q.solid_count) sv = __builtin_amdgcn_readfirstlane(uload(&t.solid[i]));
        }
        const bool parted = !solid && desc < q.brick_count;
        if (!EMIT && (solid || !parted)) {
            // a constant unit: nothing, or the Solid value throughout the part of the unit inside the box
            const uint32_t a = list_albedo(t, sv), d = list_data(q, sv);
            const uint32_t x0 = max(X, b.ox), x1 = min(X + bd, b.ox + b.gx), y0 = max(Y, b.oy), y1 = min(Y + bd, b.oy + b.gy),
                           z0 = max(Z, b.oz), z1 = min(Z + bd, b.oz + b.gz);
            if (lane == 0) ucnt[u] = (a | d) != 0u ? (u64)(x1 - x0) * (y1 - y0) * (z1 - z0) : 0ull;
            continue;
        }
        const uint32_t *brick = t.voxels + ((uint64_t)(parted ? desc : 0u) << (3u * q.lg_bd));
        u64 run = 0;
        for (uint32_t i0 = 0; i0 < nvox; i0 += 64u) {
            const uint32_t flat = i0 + lane;
            const uint32_t x = X + (flat & m), y = Y + ((flat >> q.lg_bd) & m), z = Z + (flat >> (2u * q.lg_bd));
            // unsigned differences: a coordinate below the origin wraps past the extent
            const bool in = flat < nvox && x - b.ox < b.gx && y - b.oy < b.gy && z - b.oz < b.gz;
            uint32_t v = sv;
            if (in && parted) {
                if (uniform) {  // the brick spans the leaf
                    const uint32_t um = 4u * bd - 1u;
                    v = brick[((x & um) >> 2) + ((((y & um) >> 2) + (((z & um) >> 2) << q.lg_bd)) << q.lg_bd)];
                } else {  // a Leaf's cell that points to nothing reads as empty
                    const uint64_t word = t.brick_occ[(uint64_t)desc * t.occ_words + (flat >> 6)];
                    v = ((word >> (flat & 63u)) & 1ull) != 0ull ? brick[flat] : VHX_EMPTY;
                }
            }
            uint32_t a = 0u, d = 0u;
            if (in) {
                a = list_albedo(t, v);
                d = list_data(q, v);
            }
            const bool listed = (a | d) != 0u;
            const u64 bal = __ballot(listed);
            if (EMIT && listed) {
                const u64 rank = base + run +
                                 __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                if (rank < o.capacity) {
                    if (o.pos) {
                        o.pos[3u * rank] = x;
                        o.pos[3u * rank + 1u] = y;
                        o.pos[3u * rank + 2u] = z;
                    }
                    if (o.albedo) o.albedo[rank] = a;
                    if (o.data) o.data[rank] = d;
                }
            }
            run += (u64)__popcll(bal);
            if (EMIT && base + run >= o.capacity) break;  // wave-uniform
        }
        if (!EMIT && lane == 0) ucnt[u] = run;
    }
}

DevTree list_tree(const vhx_ctx *c) {
    const TreeStore &s = *c->tree;
    DevTree t{};
    t.hdr = (const uint4 *)s.hdr.ptr;
    t.children = (const uint32_t *)s.raw[VHX_BUF_NODE_CHILDREN].ptr;
    t.voxels = (const uint32_t *)s.raw[VHX_BUF_VOXELS].ptr;
    t.brick_occ = (const uint64_t *)s.brick_occ.ptr;
    t.solid = (const uint32_t *)s.raw[VHX_BUF_SOLID_VALUES].ptr;
    t.color = (const uint32_t *)s.raw[VHX_BUF_COLOR_PALETTE].ptr;
    t.color_count = s.desc.color_count;
    t.node_count = s.desc.node_count;
    t.size = s.desc.boxtree_size;
    t.bd = s.desc.brick_dim;
    t.occ_words = s.occ_words;
    return t;
}

// aligned cubes 2^lg wide that [o, o + g) meets on one axis
uint64_t cubes_on_axis(uint32_t o, uint32_t g, uint32_t lg) { return (uint64_t)((o + g - 1u) >> lg) - (o >> lg) + 1u; }

// ... that the box meets, but no more than `limit` (the products stay below 2^64)
uint64_t cubes_under(const LBox &b, uint32_t lg, uint64_t limit) {
    const uint64_t xy = std::min(cubes_on_axis(b.ox, b.gx, lg) * cubes_on_axis(b.oy, b.gy, lg), limit);
    return std::min(xy * cubes_on_axis(b.oz, b.gz, lg), limit);
}

bool overlap(const void *a, uint64_t abytes, const void *b, uint64_t bbytes) {
    const char *a0 = (const char *)a, *b0 = (const char *)b;
    return a && b && a0 < b0 + bbytes && b0 < a0 + abytes;
}

template <int MODE>
int lscan(vhx_ctx *c, const u64 *in, const u64 *n_dev, uint64_t cap, u64 *out, u64 *total) {
    u64 *part = (u64 *)c->list.part.ptr;
    const unsigned nb = (unsigned)((cap + SCAN_TILE - 1) / SCAN_TILE);
    k_dscan_sums<MODE><<<nb, 256, 0, c->stream>>>(in, n_dev, cap, part);
    k_dscan_top<<<1, 256, 0, c->stream>>>(part, n_dev, cap, total);
    k_dscan_apply<MODE><<<nb, 256, 0, c->stream>>>(in, n_dev, cap, part, out);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}

// workgroups of a launch of one wave per item: four waves each, and no more than fill the device a few times over (the
// waves stride over the items, whose number they read on the device)
unsigned wave_blocks(uint64_t items) { return (unsigned)std::min<uint64_t>((items + 3u) / 4u, 8192u); }

int list_voxels(vhx_ctx *c, const vhx_points_out *p, int on_device) {
    if (!c) return VHX_E_INVALID_ARG;
    if (!p || !p->count) return fail(c, VHX_E_INVALID_ARG, "vhx_list_voxels: null argument or null count");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_list_voxels before vhx_upload_tree");
    if (p->gx == 0 || p->gy == 0 || p->gz == 0)
        return fail(c, VHX_E_INVALID_ARG, "vhx_list_voxels: an extent of 0");
    // the box's volume needs no tree; the box is held against the root cube inside the scope, below
    const uint64_t lim = 1ull << 48, gxy = (uint64_t)p->gx * p->gy;
    const bool huge = gxy >= lim || p->gz > (lim - 1u) / gxy;
    // no more entries than the box has voxels are ever written
    const uint64_t cap_out = huge ? 0 : std::min<uint64_t>(p->capacity, gxy * p->gz);
    const bool want = cap_out > 0 && (p->positions || p->albedo || p->data);
    if (want && on_device &&
        (overlap(p->positions, cap_out * 12, p->albedo, cap_out * 4) || overlap(p->positions, cap_out * 12, p->data, cap_out * 4) ||
         overlap(p->albedo, cap_out * 4, p->data, cap_out * 4)))
        return fail(c, VHX_E_INVALID_ARG, "vhx_list_voxels: the output arrays overlap");
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    // Everything that is read from the tree's store -- its size, counts and buffer pointers -- is read inside the scope:
    // trace_begin waits for a write of the tree in progress on another thread (which may replace buffers and counts),
    // and writers wait for the scope's end
    TraceScope scope(c);
    if (scope.rc) return scope.rc;
    const vhx_tree_desc &d = c->tree->desc;
    const uint64_t S = d.boxtree_size;
    if ((uint64_t)p->ox + p->gx > S || (uint64_t)p->oy + p->gy > S || (uint64_t)p->oz + p->gz > S)
        return fail(c, VHX_E_INVALID_ARG, "vhx_list_voxels: a box outside the root cube");
    if (huge) return fail(c, VHX_E_CAPACITY, "vhx_list_voxels: a box of 2^48 voxels or more");
    LShape q{};
    while ((1u << q.lg_size) < d.boxtree_size && q.lg_size < 31u) ++q.lg_size;
    while ((1u << q.lg_bd) < d.brick_dim && q.lg_bd < 31u) ++q.lg_bd;
    if (d.brick_dim == 0u || (1u << q.lg_size) != d.boxtree_size || (1u << q.lg_bd) != d.brick_dim ||
        q.lg_size < q.lg_bd + 2u || ((q.lg_size - q.lg_bd) & 1u))
        return fail(c, VHX_E_INVALID_ARG, "vhx_list_voxels: the tree's size is not brick_dim * 4^k");
    q.levels = (q.lg_size - q.lg_bd) / 2u;
    if (q.levels > LIST_MAX_LEVELS) return fail(c, VHX_E_STATE, "vhx_list_voxels: more than 12 node levels");
    if (q.lg_bd > 10u)
        return fail(c, VHX_E_CAPACITY, "vhx_list_voxels: brick_dim above 1024 (a unit's voxels are counted in 32 bits)");
    if (d.node_count == 0u) {
        *p->count = 0;
        return scope.end();
    }
    q.brick_count = d.brick_count;
    q.solid_count = d.solid_count;
    q.dpal = (const uint32_t *)c->tree->raw[VHX_BUF_DATA_PALETTE].ptr;
    q.dcount = q.dpal ? d.data_count : 0u;
    const LBox b{p->ox, p->oy, p->oz, p->gx, p->gy, p->gz};

    // a level's frontier holds no more nodes than the tree has and than aligned cubes of its size meet the box; the
    // units are at most 64 per smallest leaf and no more than the brick-sized cubes that meet the box
    uint64_t cap[LIST_MAX_LEVELS + 1], cap_max = 1;
    for (uint32_t lv = 0; lv < q.levels; ++lv) {
        cap[lv] = cubes_under(b, q.lg_size - 2u * lv, d.node_count);
        cap_max = std::max(cap_max, cap[lv]);
    }
    const uint64_t cap_units = cubes_under(b, q.lg_bd, cap[q.levels - 1u] * 64u);
    cap[q.levels] = cap_units;

    int rc;
    vhx_ctx::ListScratch &ls = c->list;
    if ((rc = ensure(c, ls.fr[0], cap_max * 16))) return rc;
    if ((rc = ensure(c, ls.fr[1], cap_max * 16))) return rc;
    if ((rc = ensure(c, ls.mask, cap_max * 8))) return rc;
    if ((rc = ensure(c, ls.first, cap_max * 8))) return rc;
    if ((rc = ensure(c, ls.unit, cap_units * 16))) return rc;
    if ((rc = ensure(c, ls.ucnt, cap_units * 8))) return rc;
    if ((rc = ensure(c, ls.part, ((std::max(cap_max, cap_units) + SCAN_TILE - 1) / SCAN_TILE) * 8))) return rc;
    if ((rc = ensure(c, ls.ctl, sizeof(LCtl)))) return rc;
    uint4 *fr[2] = {(uint4 *)ls.fr[0].ptr, (uint4 *)ls.fr[1].ptr};
    u64 *mask = (u64 *)ls.mask.ptr, *first = (u64 *)ls.first.ptr, *ucnt = (u64 *)ls.ucnt.ptr;
    uint4 *unit = (uint4 *)ls.unit.ptr;
    LCtl *ctl = (LCtl *)ls.ctl.ptr;
    const DevTree t = list_tree(c);

    k_list_seed<<<1, 64, 0, c->stream>>>(fr[0], ctl);
    for (uint32_t lv = 0; lv < q.levels; ++lv) {
        const uint4 *cur = fr[lv & 1u];
        uint4 *next = lv + 1u < q.levels ? fr[(lv + 1u) & 1u] : unit;
        k_list_mask<<<wave_blocks(cap[lv]), 256, 0, c->stream>>>(t, q, b, cur, ctl, lv, cap[lv], mask);
        if ((rc = lscan<1>(c, mask, &ctl->count[lv], cap[lv], first, &ctl->count[lv + 1u]))) return rc;
        k_list_push<<<wave_blocks(cap[lv]), 256, 0, c->stream>>>(t, q, b, cur, ctl, lv, cap[lv], mask, first, next,
                                                                 cap[lv + 1u]);
    }
    k_list_units<false><<<wave_blocks(cap_units), 256, 0, c->stream>>>(t, q, b, unit, 0, ctl, cap_units, ucnt, LOut{});
    if ((rc = lscan<3>(c, ucnt, &ctl->count[q.levels], cap_units, ucnt, &ctl->total))) return rc;
    VHX_HIP(c, hipGetLastError());

    // the one readback: the total, with the refusals the descent found
    LCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.bad)
        return fail(c, VHX_E_STATE, "vhx_list_voxels: a Leaf or UniformLeaf under the box lies above the smallest leaf level");
    if (h.overflow) return fail(c, VHX_E_STATE, "vhx_list_voxels: the image is not a tree (a node reached twice)");
    const uint64_t nunits = std::min<uint64_t>(h.count[q.levels], cap_units);
    const uint64_t nout = std::min<uint64_t>(h.total, cap_out);
    if (want && nout > 0) {
        LOut o{p->positions, p->albedo, p->data, cap_out};
        if (!on_device) {  // positions, then the albedo and data words
            const uint64_t words = nout * ((p->positions ? 3u : 0u) + (p->albedo ? 1u : 0u) + (p->data ? 1u : 0u));
            if ((rc = ensure(c, ls.out, words * 4))) return rc;
            uint32_t *at = (uint32_t *)ls.out.ptr;
            if (p->positions) o.pos = at, at += nout * 3;
            if (p->albedo) o.albedo = at, at += nout;
            if (p->data) o.data = at;
        }
        k_list_units<true><<<wave_blocks(nunits), 256, 0, c->stream>>>(t, q, b, unit, nunits, ctl, cap_units, ucnt, o);
        VHX_HIP(c, hipGetLastError());
        if (!on_device) {
            if (p->positions) VHX_HIP(c, hipMemcpyAsync(p->positions, o.pos, nout * 12, hipMemcpyDeviceToHost, c->stream));
            if (p->albedo) VHX_HIP(c, hipMemcpyAsync(p->albedo, o.albedo, nout * 4, hipMemcpyDeviceToHost, c->stream));
            if (p->data) VHX_HIP(c, hipMemcpyAsync(p->data, o.data, nout * 4, hipMemcpyDeviceToHost, c->stream));
        }
        VHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    *p->count = h.total;
    return scope.end();
}

}  // namespace

extern "C" {

int vhx_list_voxels(vhx_ctx *c, const vhx_points_out *q, int on_device) { return list_voxels(c, q, on_device); }

}  // extern "C"
