// The passes that the compaction (vhx_compact.hip), the simplification (vhx_simplify.hip) and the LOD build
// (vhx_lod.hip) of the resident tree share: the frontier walk that renumbers the reachable nodes breadth-first, the
// claims of the reachable Parted bricks with their source map, the gathers that move whole bricks and their bitmaps by
// such a map, and the ranking of the distinct Solid values of a new image.
// Each unit that includes this gets its own copy of the kernels (anonymous namespace), as with buildtab.hpp.
//
// Nothing of the old tree is written. A node or brick is claimed by compare-and-swap from VHX_EMPTY, and a lost claim
// raises the "reached twice" flag; the atomics feed only flags and claims, every index that reaches a buffer comes from
// a scan, and every global write is a plain store. Every index read from the tree is checked against its count before
// it is used as an address.
#pragma once
#include <algorithm>

#include "../../include/vhx.h"
#include "buildtab.hpp"
#include "ctx.hpp"

namespace {

constexpr uint32_t BAD_INDEX = 1u, BAD_TWICE = 2u, BAD_DEEP = 4u;

struct CompactCtl {
    u64 scan_total;   // entries of the new nodes so far: the nodes after the root
    u64 brick_total;  // reachable Parted bricks
    uint32_t begin, end;  // the frontier: new indices of the level at hand; at last `end` is the reachable node count
    uint32_t bad;
    uint32_t pad;
};

struct OldTree {
    const uint32_t *type;
    const u64 *ocbits;
    const uint32_t *children;
    uint32_t node_count, brick_count;
};

struct Maps {
    uint32_t *new_of, *old_of;  // [node_count]
    u64 *nmask, *nrank;         // [node_count] by new index
    u64 *bmask, *bfirst;        // [node_count] by new index
    uint32_t *bnew, *bsrc;      // [brick_count]
};

__device__ inline bool is_parted(uint32_t e) { return e != VHX_EMPTY && (e & VHX_SOLID_BIT) == 0; }

__global__ void k_cmp_init(Maps m, CompactCtl *ctl) {
    m.new_of[0] = 0;
    m.old_of[0] = 0;
    ctl->begin = 0;
    ctl->end = 1;
}

// launched over an upper bound of the level's nodes; the waves past the frontier leave at once
// occupied_only: an Internal node whose occupied_bits are 0 reaches nothing (the simplification turns it into Nothing)
__global__ __launch_bounds__(256) void k_cmp_front(OldTree t, Maps m, const CompactCtl *ctl, int occupied_only) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = ctl->begin + (gid >> 6);
    if (i >= ctl->end) return;  // the whole wave
    const uint32_t o = m.old_of[i];
    bool has = false;
    if (o < t.node_count && t.type[o] == VHX_NODE_INTERNAL && !(occupied_only && t.ocbits[o] == 0))
        has = t.children[(uint64_t)o * 64u + lane] != VHX_EMPTY;
    const u64 mask = __ballot(has);
    if (lane == 0) m.nmask[i] = mask;
}

__global__ __launch_bounds__(256) void k_cmp_expand(OldTree t, Maps m, CompactCtl *ctl) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = ctl->begin + (gid >> 6);
    if (i >= ctl->end) return;
    const uint32_t o = m.old_of[i];
    if (o >= t.node_count) return;  // a slot whose claim was lost: the flag is up
    const u64 mask = m.nmask[i];
    if (((mask >> lane) & 1ull) == 0) return;
    const uint32_t e = t.children[(uint64_t)o * 64u + lane];
    if (e >= t.node_count) {
        atomicOr(&ctl->bad, BAD_INDEX);
        return;
    }
    const u64 nw = 1ull + m.nrank[i] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (nw >= t.node_count) {  // more entries than nodes: some node is named twice
        atomicOr(&ctl->bad, BAD_TWICE);
        return;
    }
    if (atomicCAS(&m.new_of[e], VHX_EMPTY, (uint32_t)nw) != VHX_EMPTY)
        atomicOr(&ctl->bad, BAD_TWICE);
    else
        m.old_of[nw] = e;
}

__global__ void k_cmp_advance(CompactCtl *ctl, uint32_t node_count, int last) {
    const uint32_t nb = ctl->end;
    u64 ne = 1ull + ctl->scan_total;
    if (ne > node_count) {
        ctl->bad |= BAD_TWICE;
        ne = node_count;
    }
    ctl->begin = nb;
    ctl->end = (uint32_t)ne;
    if (last && ne > nb) ctl->bad |= BAD_DEEP;
}

__global__ __launch_bounds__(256) void k_cmp_bmask(OldTree t, Maps m, const CompactCtl *ctl) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= ctl->end) return;
    const uint32_t o = m.old_of[i];
    bool parted = false;
    if (o < t.node_count) {
        const uint32_t ty = t.type[o];
        if (ty == VHX_NODE_LEAF || (ty == VHX_NODE_UNIFORM_LEAF && lane == 0))
            parted = is_parted(t.children[(uint64_t)o * 64u + lane]);
    }
    const u64 mask = __ballot(parted);
    if (lane == 0) m.bmask[i] = mask;
}

__global__ __launch_bounds__(256) void k_cmp_bfill(OldTree t, Maps m, CompactCtl *ctl) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= ctl->end) return;
    const u64 mask = m.bmask[i];
    if (((mask >> lane) & 1ull) == 0) return;
    const uint32_t e = t.children[(uint64_t)m.old_of[i] * 64u + lane];  // bmask is set only for a node inside the count
    if (e >= t.brick_count) {
        atomicOr(&ctl->bad, BAD_INDEX);
        return;
    }
    const u64 j = m.bfirst[i] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (j >= t.brick_count) {
        atomicOr(&ctl->bad, BAD_TWICE);
        return;
    }
    if (atomicCAS(&m.bnew[e], VHX_EMPTY, (uint32_t)j) != VHX_EMPTY)
        atomicOr(&ctl->bad, BAD_TWICE);
    else
        m.bsrc[j] = e;
}

// The gather, driven from the destination. A workgroup owns GATHER_ITEMS * 256 consecutive 16-byte words of the new
// voxels: its stores are contiguous, and its loads are whole bricks (1 << lgw words each). The loads of a thread are
// issued before its stores. HOLES: a brick whose source is VHX_EMPTY is left alone (the simplification writes it anew).
constexpr uint32_t GATHER_ITEMS = 4;
template <bool HOLES>
__global__ __launch_bounds__(256) void k_cmp_gather(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                    const uint32_t *__restrict__ bsrc, uint64_t w0, uint64_t nwords,
                                                    uint32_t lgw) {
    const uint64_t base = w0 + (uint64_t)blockIdx.x * (256u * GATHER_ITEMS) + threadIdx.x;
    const uint64_t kmask = (1ull << lgw) - 1ull;
    uint4 v[GATHER_ITEMS];
    bool have[GATHER_ITEMS];
#pragma unroll
    for (uint32_t u = 0; u < GATHER_ITEMS; ++u) {
        const uint64_t w = base + 256ull * u;
        have[u] = w < nwords;
        if (have[u]) {
            const uint32_t b = bsrc[w >> lgw];
            if (HOLES && b == VHX_EMPTY)
                have[u] = false;
            else
                v[u] = src[((uint64_t)b << lgw) + (w & kmask)];
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < GATHER_ITEMS; ++u) {
        const uint64_t w = base + 256ull * u;
        if (have[u]) dst[w] = v[u];
    }
}

// brick_dim 1: a brick is one dword
template <bool HOLES>
__global__ __launch_bounds__(256) void k_cmp_gather1(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                     const uint32_t *__restrict__ bsrc, uint32_t bricks) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= bricks) return;
    const uint32_t b = bsrc[j];
    if (HOLES && b == VHX_EMPTY) return;
    dst[j] = src[b];
}

// the bitmaps: 1 << lgo words of 64 bits per brick
template <bool HOLES>
__global__ __launch_bounds__(256) void k_cmp_gather_occ(const u64 *__restrict__ src, u64 *__restrict__ dst,
                                                        const uint32_t *__restrict__ bsrc, uint64_t w0, uint64_t nwords,
                                                        uint32_t lgo) {
    const uint64_t w = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const uint32_t b = bsrc[w >> lgo];
    if (HOLES && b == VHX_EMPTY) return;
    dst[w] = src[((uint64_t)b << lgo) + (w & ((1ull << lgo) - 1ull))];
}

inline uint32_t lg2(uint64_t v) {
    uint32_t l = 0;
    while ((1ull << l) < v) ++l;
    return l;
}

// The frontier walk and the claims of the reachable Parted bricks on c's stream: resets the maps and *ctl, renumbers
// the nodes level by level (no readback between levels) and fills bmask / bfirst / bnew / bsrc. Afterwards ctl->end is
// the reachable node count, ctl->brick_total the reachable Parted bricks and ctl->bad the flags; the caller reads them
// back. c->build.part must hold the scans' block sums for node_count words.
inline int walk_and_claim(vhx_ctx *c, const OldTree &t, const Maps &m, CompactCtl *ctl, bool occupied_only) {
    const uint64_t nn = t.node_count, nb = t.brick_count;
    int rc;
    // reset: nothing claimed, no slot filled, no entries beyond the frontier
    VHX_HIP(c, hipMemsetAsync(ctl, 0, sizeof(CompactCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(m.new_of, 0xFF, nn * 4, c->stream));
    VHX_HIP(c, hipMemsetAsync(m.old_of, 0xFF, nn * 4, c->stream));
    VHX_HIP(c, hipMemsetAsync(m.nmask, 0, nn * 8, c->stream));
    VHX_HIP(c, hipMemsetAsync(m.bmask, 0, nn * 8, c->stream));
    if (nb) {
        VHX_HIP(c, hipMemsetAsync(m.bnew, 0xFF, nb * 4, c->stream));
        VHX_HIP(c, hipMemsetAsync(m.bsrc, 0xFF, nb * 4, c->stream));
    }
    k_cmp_init<<<1, 1, 0, c->stream>>>(m, ctl);
    // level lv holds at most 64^lv nodes, the levels up to it (64^(lv+1) - 1) / 63
    uint64_t level_cap = 1, upto_cap = 1;
    for (uint32_t lv = 0; lv < MAX_LEVELS; ++lv) {
        const uint64_t waves = std::min(level_cap, nn), scan_n = std::min(upto_cap, nn);
        k_cmp_front<<<blocks_for(waves * 64), 256, 0, c->stream>>>(t, m, ctl, occupied_only ? 1 : 0);
        if ((rc = scan_level<1>(c, m.nmask, scan_n, false, m.nrank, &ctl->scan_total))) return rc;
        k_cmp_expand<<<blocks_for(waves * 64), 256, 0, c->stream>>>(t, m, ctl);
        k_cmp_advance<<<1, 1, 0, c->stream>>>(ctl, t.node_count, lv + 1 == MAX_LEVELS ? 1 : 0);
        if (level_cap >= nn) level_cap = nn; else level_cap *= 64;
        upto_cap = std::min(nn, upto_cap + level_cap);
    }
    k_cmp_bmask<<<blocks_for(nn * 64), 256, 0, c->stream>>>(t, m, ctl);
    if ((rc = scan_level<1>(c, m.bmask, nn, false, m.bfirst, &ctl->brick_total))) return rc;
    k_cmp_bfill<<<blocks_for(nn * 64), 256, 0, c->stream>>>(t, m, ctl);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}

// the compaction's scratch (vhx_ctx::compact) sized for a tree of nn nodes and nb bricks, as Maps
inline int ensure_maps(vhx_ctx *c, uint64_t nn, uint64_t nb, Maps *m, CompactCtl **ctl) {
    vhx_ctx::CompactScratch &cs = c->compact;
    int rc;
    if ((rc = vhx::ensure(c, cs.new_of, nn * 4))) return rc;
    if ((rc = vhx::ensure(c, cs.old_of, nn * 4))) return rc;
    if ((rc = vhx::ensure(c, cs.nmask, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, cs.nrank, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, cs.bmask, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, cs.bfirst, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, cs.bnew, nb * 4))) return rc;
    if ((rc = vhx::ensure(c, cs.bsrc, nb * 4))) return rc;
    if ((rc = vhx::ensure(c, cs.ctl, sizeof(CompactCtl)))) return rc;
    if ((rc = vhx::ensure(c, c->build.part, ((nn + SCAN_TILE - 1) / SCAN_TILE) * 8))) return rc;
    *m = Maps{(uint32_t *)cs.new_of.ptr, (uint32_t *)cs.old_of.ptr, (u64 *)cs.nmask.ptr, (u64 *)cs.nrank.ptr,
              (u64 *)cs.bmask.ptr,       (u64 *)cs.bfirst.ptr,      (uint32_t *)cs.bnew.ptr, (uint32_t *)cs.bsrc.ptr};
    *ctl = (CompactCtl *)cs.ctl.ptr;
    return VHX_OK;
}

// ---- the distinct Solid values of a new image, ranked by their first key (new node * 64 + sectant), in a table of the
// colour table's shape (vhx_simplify.hip, vhx_lod.hip). Ctl is the unit's counters: `b` the table's (ncolors distinct
// values that are not 0, overflow, ncompact), `zero_key` the first key of the value 0 -- a legal word, but the table's
// free-slot marker; ~0 = unused -- and `zero_rank` its index.
template <class Ctl>
__device__ inline void solid_insert(const ColorTable tab, Ctl *ctl, uint32_t v, u64 key) {
    if (v == 0) {
        if (ctl->zero_key > key) atomicMin(&ctl->zero_key, key);
    } else {
        color_insert(tab, &ctl->b, v, key);
    }
}

// the table's entries compacted for the ranking (any order: the ranks come from the keys)
template <class Ctl>
__global__ __launch_bounds__(256) void k_smp_solid_compact(ColorTable t, Ctl *ctl) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= TAB_SLOTS) return;
    const uint32_t k = t.keys[h];
    if (k == 0) return;
    const uint32_t pos = atomicAdd(&ctl->b.ncompact, 1u);
    if (pos >= PAL_CAP) return;
    t.ckey[pos] = k;
    t.cidx[pos] = t.vals[h];
    t.cslot[pos] = h;
}

// index of a value in solid_values = how many values have a smaller key (the keys are distinct). Element n stands for
// the value 0, which the table cannot hold. t.pal receives solid_values, the value's table slot its index.
template <class Ctl>
__global__ __launch_bounds__(256) void k_smp_solid_rank(ColorTable t, Ctl *ctl) {
    __shared__ u64 tile[256];
    const uint32_t n = min(ctl->b.ncompact, MAX_COLORS);
    const u64 zkey = ctl->zero_key;
    if (blockIdx.x * 256u > n) return;  // the whole block
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const u64 mine = i < n ? t.cidx[i] : i == n ? zkey : ~0ull;
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += 256) {
        tile[threadIdx.x] = j0 + threadIdx.x < n ? t.cidx[j0 + threadIdx.x] : ~0ull;
        __syncthreads();
        const uint32_t m = min(256u, n - j0);
        for (uint32_t j = 0; j < m; ++j) rank += tile[j] < mine;
        __syncthreads();
    }
    if (i < n) {
        rank += zkey < mine;
        if (rank < PAL_CAP) t.pal[rank] = t.ckey[i];
        t.vals[t.cslot[i]] = rank;
    } else if (i == n && zkey != ~0ull) {
        if (rank < PAL_CAP) t.pal[rank] = 0;
        ctl->zero_rank = rank;
    }
}

// the gather of the voxels of `bricks` new bricks by the map bsrc, on c's stream
template <bool HOLES>
inline void gather_voxels(vhx_ctx *c, const void *vsrc, void *vdst, const uint32_t *bsrc, uint32_t bricks, uint64_t n3) {
    if (n3 < 4) {
        k_cmp_gather1<HOLES><<<blocks_for(bricks), 256, 0, c->stream>>>((const uint32_t *)vsrc, (uint32_t *)vdst, bsrc,
                                                                         bricks);
    } else {
        const uint32_t lgw = lg2(n3 / 4);
        const uint64_t nwords = (uint64_t)bricks << lgw, per_block = 256ull * GATHER_ITEMS;
        const uint64_t chunk = per_block << 22;  // launches of at most 2^22 workgroups
        for (uint64_t w0 = 0; w0 < nwords; w0 += chunk) {
            const uint64_t n = std::min(chunk, nwords - w0);
            k_cmp_gather<HOLES><<<(unsigned)((n + per_block - 1) / per_block), 256, 0, c->stream>>>(
                (const uint4 *)vsrc, (uint4 *)vdst, bsrc, w0, nwords, lgw);
        }
    }
}

// the gathers of the voxels and bitmaps of `bricks` new bricks by the map bsrc, on c's stream
template <bool HOLES>
inline void gather_bricks(vhx_ctx *c, const void *vsrc, void *vdst, const u64 *osrc, u64 *odst, const uint32_t *bsrc,
                          uint32_t bricks, uint64_t n3, uint32_t occ_words) {
    gather_voxels<HOLES>(c, vsrc, vdst, bsrc, bricks, n3);
    const uint32_t lgo = lg2(occ_words);
    const uint64_t owords = (uint64_t)bricks << lgo, ochunk = 1ull << 30;
    for (uint64_t w0 = 0; w0 < owords; w0 += ochunk)
        k_cmp_gather_occ<HOLES><<<blocks_for(std::min(ochunk, owords - w0)), 256, 0, c->stream>>>(osrc, odst, bsrc, w0,
                                                                                                   owords, lgo);
}

}  // namespace
