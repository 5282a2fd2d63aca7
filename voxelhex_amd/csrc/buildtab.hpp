// The pieces of the dense build (vhx_build.hip) that the in-place dense write (vhx_edit.hip) uses as well: the colour
// table with its insert, lookup, compaction and ranking, the scans over occupancy words, and the counters read back.
// The compaction (vhx_compact.hip) uses the scans; the simplification (vhx_simplify.hip) the scans and the table, for
// the distinct Solid values; the listing (vhx_list.hip) the scans whose element count stays on the device.
// Each unit that includes this gets its own copy of the kernels (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctx.hpp"

namespace {

typedef unsigned long long u64;

constexpr uint32_t TAB_SLOTS = 1u << 18;  // four times the colours a palette holds: short probe chains
constexpr uint32_t TAB_MASK = TAB_SLOTS - 1;
constexpr uint32_t MAX_COLORS = 0xFFFFu;  // the palette index has 16 bits, 0xFFFF = none
constexpr uint32_t PAL_CAP = 1u << 16;
// color_lookup answers 0xFFFF for a colour the table does not hold (a build whose table overflowed, which fails at the
// readback): arrays indexed by palette index have PAL_CAP entries, so that index stays inside them
static_assert(PAL_CAP > MAX_COLORS, "a palette index, 0xFFFF = none included, must index a PAL_CAP array");
constexpr uint32_t MAX_LEVELS = 8;
constexpr uint64_t MAX_LEAVES = 1ull << 28;  // possible leaf nodes (scratch words per array)
constexpr uint32_t SCAN_ITEMS = 4, SCAN_TILE = 256 * SCAN_ITEMS;
constexpr uint32_t SCAN_ROWS = 4;  // grid rows per thread of pass A

// the counters of a build, read back once
struct BuildCtl {
    u64 level_total[MAX_LEVELS];  // nodes per level
    u64 brick_total;
    uint32_t ncolors;   // table slots claimed
    uint32_t overflow;  // more than MAX_COLORS colours
    uint32_t ncompact;
    uint32_t solid_count;  // simplified build: distinct Solid values
};

// vhx_ctx::build.table
struct ColorTable {
    u64 *vals;        // [TAB_SLOTS] smallest insert-order index of the slot's colour; after k_pal_rank its palette index
    u64 *cidx;        // [PAL_CAP]   compacted: first index
    uint32_t *keys;   // [TAB_SLOTS] colour, 0 = free (a voxel's colour has a non-zero alpha byte)
    uint32_t *ckey;   // [PAL_CAP]   compacted: colour
    uint32_t *cslot;  // [PAL_CAP]   compacted: table slot
    uint32_t *pal;    // [PAL_CAP]   the palette
};
constexpr uint64_t TAB_VALS_BYTES = (uint64_t)TAB_SLOTS * 8, TAB_CIDX_BYTES = (uint64_t)PAL_CAP * 8,
                   TAB_KEYS_BYTES = (uint64_t)TAB_SLOTS * 4, TAB_BYTES = TAB_VALS_BYTES + TAB_CIDX_BYTES +
                                                                        TAB_KEYS_BYTES + 3ull * PAL_CAP * 4;
ColorTable table_of(void *base) {
    ColorTable t;
    uint8_t *p = (uint8_t *)base;
    t.vals = (u64 *)p;
    t.cidx = (u64 *)(p + TAB_VALS_BYTES);
    t.keys = (uint32_t *)(p + TAB_VALS_BYTES + TAB_CIDX_BYTES);
    t.ckey = t.keys + TAB_SLOTS;
    t.cslot = t.ckey + PAL_CAP;
    t.pal = t.cslot + PAL_CAP;
    return t;
}


__device__ inline uint32_t color_hash(uint32_t c) {
    c *= 0x9E3779B1u;
    c ^= c >> 15;
    c *= 0x85EBCA77u;
    c ^= c >> 13;
    return c & TAB_MASK;
}


// Records colour c seen at insert-order index idx. The slot of a colour is claimed by compare-and-swap (whoever wins,
// the slot then holds c); the count of claims detects a table that would hold more colours than a palette can, after
// which inserts stop (the build fails) -- so the probe loop ends even when a grid holds millions of colours.
__device__ inline void color_insert(const ColorTable t, BuildCtl *ctl, uint32_t c, u64 idx) {
    uint32_t h = color_hash(c);
    for (uint32_t probe = 0; probe < TAB_SLOTS; ++probe, h = (h + 1) & TAB_MASK) {
        if ((probe & 63u) == 0 && __hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        uint32_t k = t.keys[h];  // a stale 0 is settled by the compare-and-swap; a colour never leaves its slot
        if (k == 0) {
            k = atomicCAS(&t.keys[h], 0u, c);
            if (k == 0) {
                if (atomicAdd(&ctl->ncolors, 1u) >= MAX_COLORS) atomicOr(&ctl->overflow, 1u);
                k = c;
            }
        }
        if (k == c) {
            // the index only ever shrinks, so a larger one needs no atomic (a stale read only costs the atomic)
            if (t.vals[h] > idx) atomicMin(&t.vals[h], idx);
            return;
        }
    }
}

// palette index of colour c (after k_pal_rank); 0xFFFF where the table does not hold it
__device__ inline uint32_t color_lookup(const ColorTable t, uint32_t c) {
    uint32_t h = color_hash(c);
    for (uint32_t probe = 0; probe < TAB_SLOTS; ++probe, h = (h + 1) & TAB_MASK) {
        const uint32_t k = t.keys[h];
        if (k == c) return (uint32_t)t.vals[h] & 0xFFFFu;
        if (k == 0) break;
    }
    return 0xFFFFu;
}


// ---- scans over the occupancy words of a level: MODE 0 "the node exists" (the root always does), MODE 1 its bricks
// (MODE 2: of a simplified build, from SimpTable::linfo; MODE 3: the word is a count below 2^32, vhx_points.hip)
template <int MODE>
__device__ inline uint32_t scan_value(u64 w, bool root) {
    return MODE == 0   ? (uint32_t)(w != 0 || root)
           : MODE == 1 ? (uint32_t)__popcll(w)
           : MODE == 2 ? (uint32_t)(w & 0x7Fu)
                       : (uint32_t)w;
}

// inclusive scan over the block's 256 threads (lds: 4 words)
__device__ inline u64 block_scan(u64 v, u64 *lds) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 1; k < 64; k <<= 1) {
        const u64 o = __shfl_up(v, k);
        if (lane >= k) v += o;
    }
    if (lane == 63) lds[w] = v;
    __syncthreads();
    u64 add = 0;
    for (uint32_t i = 0; i < w; ++i) add += lds[i];
    __syncthreads();
    return v + add;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_scan_sums(const u64 *occ, uint64_t n, int root, u64 *part) {
    __shared__ u64 lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    u64 s = 0;
    for (uint32_t i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) s += scan_value<MODE>(occ[base + i], root != 0);
    s = block_scan(s, lds);
    if (threadIdx.x == 255) part[blockIdx.x] = s;
}

// exclusive scan of the nb block sums in place (one block), the total to *total
__global__ __launch_bounds__(256) void k_scan_top(u64 *part, uint64_t nb, u64 *total) {
    __shared__ u64 lds[4];
    __shared__ u64 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < nb; c0 += 256) {
        const uint64_t i = c0 + threadIdx.x;
        const u64 v = i < nb ? part[i] : 0;
        const u64 incl = block_scan(v, lds);
        if (i < nb) part[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_scan_apply(const u64 *occ, uint64_t n, int root, const u64 *part, u64 *out) {
    __shared__ u64 lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    u64 s = 0;
    for (uint32_t i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = base + i < n ? scan_value<MODE>(occ[base + i], root != 0) : 0u;
        s += v[i];
    }
    u64 run = part[blockIdx.x] + block_scan(s, lds) - s;
    for (uint32_t i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
}

// ---- the same three scans over the first min(*n_dev, cap) words, for a caller whose element count stays on the device
// (vhx_list.hip): the launches are sized by cap, and the blocks past the count leave at once
template <int MODE>
__global__ __launch_bounds__(256) void k_dscan_sums(const u64 *in, const u64 *n_dev, u64 cap, u64 *part) {
    __shared__ u64 lds[4];
    const u64 n = min(*n_dev, cap);
    if ((u64)blockIdx.x * SCAN_TILE >= n) return;  // the whole block
    const u64 base = (u64)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    u64 s = 0;
    for (uint32_t i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) s += scan_value<MODE>(in[base + i], false);
    s = block_scan(s, lds);
    if (threadIdx.x == 255) part[blockIdx.x] = s;
}

[[maybe_unused]] __global__ __launch_bounds__(256) void k_dscan_top(u64 *part, const u64 *n_dev, u64 cap, u64 *total) {
    __shared__ u64 lds[4];
    __shared__ u64 carry;
    const u64 nb = (min(*n_dev, cap) + SCAN_TILE - 1) / SCAN_TILE;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (u64 c0 = 0; c0 < nb; c0 += 256) {
        const u64 i = c0 + threadIdx.x;
        const u64 v = i < nb ? part[i] : 0;
        const u64 incl = block_scan(v, lds);
        if (i < nb) part[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// out may be in: a thread reads its own words before it writes them
template <int MODE>
__global__ __launch_bounds__(256) void k_dscan_apply(const u64 *in, const u64 *n_dev, u64 cap, const u64 *part, u64 *out) {
    __shared__ u64 lds[4];
    const u64 n = min(*n_dev, cap);
    if ((u64)blockIdx.x * SCAN_TILE >= n) return;  // the whole block
    const u64 base = (u64)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    u64 s = 0;
    for (uint32_t i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = base + i < n ? scan_value<MODE>(in[base + i], false) : 0u;
        s += v[i];
    }
    u64 run = part[blockIdx.x] + block_scan(s, lds) - s;
    for (uint32_t i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
}

// ---- palette
// palette position of a colour = how many colours appear before it (first indices are distinct)
__global__ __launch_bounds__(256) void k_pal_rank(ColorTable t, const BuildCtl *ctl) {
    __shared__ u64 tile[256];
    const uint32_t n = min(ctl->ncompact, PAL_CAP);
    if (blockIdx.x * 256u >= n) return;  // the whole block
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const u64 mine = i < n ? t.cidx[i] : 0;
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += 256) {
        tile[threadIdx.x] = j0 + threadIdx.x < n ? t.cidx[j0 + threadIdx.x] : ~0ull;
        __syncthreads();
        const uint32_t m = min(256u, n - j0);
        for (uint32_t j = 0; j < m; ++j) rank += tile[j] < mine;
        __syncthreads();
    }
    if (i < n) {
        t.pal[rank] = t.ckey[i];
        t.vals[t.cslot[i]] = rank;
    }
}


inline unsigned blocks_for(uint64_t threads) { return (unsigned)((threads + 255) / 256); }


template <int MODE>
int scan_level(vhx_ctx *c, const u64 *occ, uint64_t n, bool root, u64 *out, u64 *total) {
    u64 *part = (u64 *)c->build.part.ptr;
    const uint64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    k_scan_sums<MODE><<<(unsigned)nb, 256, 0, c->stream>>>(occ, n, root ? 1 : 0, part);
    k_scan_top<<<1, 256, 0, c->stream>>>(part, nb, total);
    k_scan_apply<MODE><<<(unsigned)nb, 256, 0, c->stream>>>(occ, n, root ? 1 : 0, part, out);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}


}  // namespace
