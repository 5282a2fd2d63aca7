// vhx_compact_palette / vhx_compact_palettes: the colour half, the data half or both halves of the resident tree
// rewritten in place, so that color_palette and data_palette are the builders' palettes of the voxels the tree holds now
// (DESIGN.md §8.10, §8.14). The passes are described for the colour half; the data half runs the same passes on arrays
// of its own (dfirst, build.dtable, dmap; "the entry is not 0" in place of "alpha is not 0"), and the kernels that read
// or write cells are templates on the mask of halves H, so that a word is loaded once for both. H = VHX_PALETTE_COLOR
// is the kernel of vhx_compact_palette as it was before the data half existed. The image is a pure function of the old one
// (vhx_flat_compact_palette, flatten.cpp, is the CPU reference, and include/vhx_boxtree.h states the rules): the colours
// that a reachable value names, entries of one colour merged, ordered by the first index (x * S + y) * S + z of the min
// corner of the cubes that hold them; every cell and solid value translated through the map old index -> new index.
//
//   frontier  walk_and_claim  the compaction's walk (treepack.hpp): reachability, the claims, the malformed-tree flags
//   origins   k_plt_origin    per level, a wave per node of that level: origin and level of its children, from the
//                             child masks and ranks the walk left (no readback between levels)
//   mark      k_plt_mark      the hot pass, a workgroup per new node: reads a leaf's entries and the cells of its Parted
//                             bricks once, in 16-byte words, and records per palette index the smallest first index
//                             of a cell or Solid entry that names it. A thread keeps one cell per index of its word, the
//                             wave one lane per index with the smallest position of its lanes (a 21-bit key inside the
//                             node, min over the wave), and that lane issues the atomic only where a plain read shows
//                             a larger index stored. A cell whose index already holds a first index at or below the
//                             node's min corner is dropped before the wave's round. The table is indexed by palette
//                             index: no hash and no palette read per cell; alpha and equal colours are settled per
//                             entry, not per cell. With both halves the word's data indices go the same way into
//                             dfirst[] after its colour indices, on the same position keys
//   merge     k_plt_merge     per used entry of alpha != 0: color_insert(colour, first index) into the build's colour
//                             table, which makes entries of one colour one colour
//   rank      k_plt_compact, k_pal_rank   the table compacted and ranked by first index (buildtab.hpp): the new palette
//   map       k_plt_map       per old index the new index of its colour, 0xFFFF where it names none or is unused
//   -- one readback of the counters; refusals happen here; nothing of the tree has been written --
//   rewrite   k_plt_rewrite   one flat pass over the voxel buffer, orphaned slots included: 16-byte loads, the colour
//                             half of each cell through the map, 16-byte stores of the words that changed
//                             (k_plt_rewrite1: brick_dim 1, a dword per thread)
//             k_plt_tail      solid_values through the map(s), and the new palette(s)
//   derive    brick bitmaps and node headers do not change for a reachable brick (emptiness is preserved) and the child
//             records embed no value; where the tree has orphaned slots, whose cells may have named a colour that left,
//             the tree unit rebuilds bitmaps and child records (rederive_bricks)
//
// The atomics feed only claims, minima and flags, every index that reaches a buffer comes from a scan or a rank, and
// every global write is a plain store. Every index read from the tree is checked against its count before it is used
// as an address; the 64 Ki-entry arrays (first, dfirst, map, dmap) take any 16-bit index. Each map has 64 Ki u16 entries
// in global memory (see DESIGN.md §8.10 for why not in LDS; the two together would not fit a CU's LDS at all).
#include <algorithm>
#include <string>

#include "../../include/vhx.h"
// the gathers of treepack.hpp are not used here (the rewrite is in place)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "treepack.hpp"
#pragma clang diagnostic pop
#include "ctx.hpp"

namespace {

constexpr uint32_t BAD_SMALL = 8u;  // a Leaf or UniformLeaf whose bricks' cells are smaller than a voxel

struct PaletteCtl {
    CompactCtl w;  // the walk's
    BuildCtl b;    // the colour table: ncolors distinct used colours, overflow, ncompact
    BuildCtl d;    // the data table: the same counters for the distinct used data values
};

constexpr uint32_t H_COLOR = VHX_PALETTE_COLOR, H_DATA = VHX_PALETTE_DATA;

struct MarkIn {
    const uint32_t *vox, *solids;
    uint32_t solid_count;
    uint32_t bsh;   // log2(brick_dim)
    uint32_t size;  // boxtree_size
};

__global__ void k_plt_origin_root(uint4 *org) { org[0] = make_uint4(0u, 0u, 0u, 0u); }

// org[i] = (x, y, z, level) of new node i. Launched over an upper bound of the nodes up to level lv; a wave whose node
// is not of that level leaves at once. The children's new indices are the walk's: 1 + nrank + the entries before.
__global__ __launch_bounds__(256) void k_plt_origin(Maps m, const PaletteCtl *ctl, uint4 *org, uint32_t lv,
                                                    uint32_t size, uint32_t node_count) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= min(ctl->w.end, node_count)) return;  // the whole wave
    const uint4 o = org[i];
    if (o.w != lv) return;
    const u64 mask = m.nmask[i];
    if (((mask >> lane) & 1ull) == 0) return;
    const u64 nw = 1ull + m.nrank[i] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (nw >= node_count) return;  // the walk has raised its flag
    const uint32_t q = (size >> (2u * lv)) >> 2;
    org[nw] = make_uint4(o.x + (lane & 3u) * q, o.y + ((lane >> 2) & 3u) * q, o.z + (lane >> 4) * q, lv + 1u);
}

// Position key of a cube inside its node, in cells: 7 bits per axis (4 bricks of at most 32 cells), x first -- the
// order of the first index.
__device__ inline uint32_t cube_key(uint32_t x, uint32_t y, uint32_t z) { return (x << 14) | (y << 7) | z; }

// One atomic per palette index per wave: among the lanes with cand set and the same index, the smallest key goes to
// first[]. Called by all 64 lanes.
__device__ inline void mark_wave(bool cand, uint32_t ci, uint32_t key, uint4 og, uint32_t cell, uint32_t size,
                                 u64 *first) {
    const uint32_t lane = threadIdx.x & 63u;
    u64 pending = __ballot(cand);
    while (pending) {  // the same in every lane
        const uint32_t leader = (uint32_t)__ffsll((long long)pending) - 1u;
        const uint32_t lc = __shfl(ci, leader);
        const bool mine = cand && ci == lc;
        uint32_t mk = mine ? key : 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t s = 1; s < 64; s <<= 1) mk = min(mk, (uint32_t)__shfl_xor(mk, s));
        if (lane == leader) {
            const u64 x = og.x + (u64)(mk >> 14) * cell, y = og.y + (u64)((mk >> 7) & 127u) * cell,
                      z = og.z + (u64)(mk & 127u) * cell;
            const u64 idx = (x * size + y) * size + z;
            // the index only ever shrinks, so a larger one needs no atomic (a stale read only costs the atomic)
            if (first[lc] > idx) atomicMin(&first[lc], idx);
        }
        pending &= ~__ballot(mine);
    }
}

constexpr uint32_t MARK_LOADS = 4;  // 16-byte loads a thread has in flight

// One workgroup per new node at a time. The loop bounds are the same for every thread of a block, so the wave operations
// run with all 64 lanes. H selects the halves: first[] takes the colour indices, dfirst[] the data indices.
template <uint32_t H>
__global__ __launch_bounds__(256) void k_plt_mark(OldTree t, Maps m, MarkIn in, const uint4 *org, u64 *first,
                                                  PaletteCtl *ctl, u64 *dfirst) {
    __shared__ uint32_t s_np;
    __shared__ uint32_t s_sect[64], s_brick[64];
    const uint32_t tid = threadIdx.x;
    const uint32_t bsh = in.bsh, n3sh = 3 * bsh, bdm = (1u << bsh) - 1u;
    const uint32_t nodes = min(ctl->w.end, t.node_count);
    for (uint32_t i = blockIdx.x; i < nodes; i += gridDim.x) {
        const uint32_t o = m.old_of[i];
        const uint32_t ty = o < t.node_count ? t.type[o] : VHX_NODE_NOTHING;
        if (ty != VHX_NODE_LEAF && ty != VHX_NODE_UNIFORM_LEAF) continue;  // the whole block
        const uint4 og = org[i];
        if (og.w >= MAX_LEVELS) continue;  // never placed: the walk has raised a flag
        const uint32_t nsize = in.size >> (2u * og.w);
        const uint32_t cell = (ty == VHX_NODE_UNIFORM_LEAF ? nsize : nsize >> 2) >> bsh;
        if (cell == 0) {
            if (tid == 0) atomicOr(&ctl->w.bad, BAD_SMALL);
            continue;
        }
        const u64 node_min = ((u64)og.x * in.size + og.y) * in.size + og.z;  // the first index of the node's min corner
        if (tid < 64) {  // wave 0: a lane per sectant
            uint32_t e = VHX_EMPTY;
            if (ty == VHX_NODE_LEAF || tid == 0) e = t.children[(uint64_t)o * 64u + tid];
            const bool parted = is_parted(e) && e < t.brick_count;  // past the count: the walk has raised its flag
            const u64 pm = __ballot(parted);
            const uint32_t k = (uint32_t)__popcll(pm & ((1ull << tid) - 1ull));
            if (parted) {
                s_sect[k] = tid;
                s_brick[k] = e;
            }
            if (tid == 0) s_np = (uint32_t)__popcll(pm);
            // the values the entries hold themselves: a Solid entry's, and the one cell of a brick of brick_dim 1
            uint32_t v = VHX_EMPTY;
            if (parted) {
                if (bsh == 0) v = in.vox[e];
            } else if (e != VHX_EMPTY && (e & VHX_SOLID_BIT)) {
                const uint32_t idx = e & ~VHX_SOLID_BIT;
                if (idx >= in.solid_count)
                    atomicOr(&ctl->w.bad, BAD_INDEX);
                else
                    v = in.solids[idx];
            }
            const uint32_t key = cube_key((tid & 3u) << bsh, ((tid >> 2) & 3u) << bsh, (tid >> 4) << bsh);
            if (H & H_COLOR) {
                const uint32_t ci = v & 0xFFFFu;
                mark_wave(ci != 0xFFFFu, ci, key, og, cell, in.size, first);
            }
            if (H & H_DATA) {
                const uint32_t di = v >> 16;
                mark_wave(di != 0xFFFFu, di, key, og, cell, in.size, dfirst);
            }
        }
        __syncthreads();
        if (bsh >= 1) {
            const uint32_t n4sh = n3sh - 2;
            const uint32_t items = s_np << n4sh;  // 16-byte words of the node's Parted bricks
            const uint4 *vox4 = (const uint4 *)in.vox;
            for (uint32_t base = 0; base < items; base += 256u * MARK_LOADS) {
                uint4 v[MARK_LOADS];
#pragma unroll
                for (uint32_t u = 0; u < MARK_LOADS; ++u) {
                    const uint32_t q = base + tid + 256u * u;
                    v[u] = make_uint4(VHX_EMPTY, VHX_EMPTY, VHX_EMPTY, VHX_EMPTY);
                    if (q < items) v[u] = vox4[((uint64_t)s_brick[q >> n4sh] << n4sh) + (q & ((1u << n4sh) - 1u))];
                }
#pragma unroll
                for (uint32_t u = 0; u < MARK_LOADS; ++u) {
                    const uint32_t q = min(base + tid + 256u * u, items - 1u);
                    const uint32_t sect = s_sect[q >> n4sh], c0 = (q & ((1u << n4sh) - 1u)) << 2;
                    const uint32_t bx = (sect & 3u) << bsh, by = ((sect >> 2) & 3u) << bsh, bz = (sect >> 4) << bsh;
                    const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    // the selected halves of the word, one after the other: colour (bits 0..15 into first[]), data
                    // (bits 16..31 into dfirst[]); the keys are the same
#pragma unroll
                    for (uint32_t half = 0; half < 2; ++half) {
                        if ((H & (1u << half)) == 0) continue;
                        u64 *const fst = half ? dfirst : first;
                        uint32_t ci[4], key[4];
                        bool cand[4];
#pragma unroll
                        for (uint32_t k = 0; k < 4; ++k) {
                            const uint32_t c = c0 + k;
                            ci[k] = (w[k] >> (16u * half)) & 0xFFFFu;
                            key[k] = cube_key(bx + (c & bdm), by + ((c >> bsh) & bdm), bz + (c >> (2 * bsh)));
                            cand[k] = ci[k] != 0xFFFFu;
                        }
                        // of the thread's cells with one index, the one with the smallest key
                        bool keep[4];
#pragma unroll
                        for (uint32_t k = 0; k < 4; ++k) {
                            keep[k] = cand[k];
#pragma unroll
                            for (uint32_t e = 0; e < 4; ++e)
                                if (e != k && cand[e] && ci[e] == ci[k] && key[e] < key[k]) keep[k] = false;
                        }
#pragma unroll
                        for (uint32_t k = 0; k < 4; ++k) {
                            // no cell of this node can lower an index that is at or below the node's own (a stale
                            // read only costs the wave's round)
                            if (keep[k]) keep[k] = fst[ci[k]] > node_min;
                            mark_wave(keep[k], ci[k], key[k], og, cell, in.size, fst);
                        }
                    }
                }
            }
        }
        __syncthreads();  // the shared words are rewritten for the next node
    }
}

// what a palette entry must be to name something: a colour of alpha != 0, a data value != 0 (key 0 is the free slot of
// either table)
template <bool DATA>
__device__ inline bool entry_names(uint32_t e) {
    return DATA ? e != 0 : (e >> 24) != 0;
}

// entries of one colour become one colour: the table takes the smallest first index of them. Entries of alpha 0 (data:
// of value 0) and entries no reachable value names stay out
template <bool DATA>
__global__ __launch_bounds__(256) void k_plt_merge(const uint32_t *color, uint32_t ncolor, const u64 *first,
                                                   ColorTable tab, BuildCtl *ctl) {
    const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
    if (ci >= ncolor || ci >= MAX_COLORS) return;
    const u64 f = first[ci];
    const uint32_t col = color[ci];
    if (f != ~0ull && entry_names<DATA>(col)) color_insert(tab, ctl, col, f);
}

// the table's entries compacted for k_pal_rank (any order: the ranks come from the first indices)
__global__ __launch_bounds__(256) void k_plt_compact(ColorTable t, BuildCtl *ctl) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= TAB_SLOTS) return;
    const uint32_t k = t.keys[h];
    if (k == 0) return;
    const uint32_t pos = atomicAdd(&ctl->ncompact, 1u);
    if (pos >= PAL_CAP) return;
    t.ckey[pos] = k;
    t.cidx[pos] = t.vals[h];
    t.cslot[pos] = h;
}

template <bool DATA>
__global__ __launch_bounds__(256) void k_plt_map(const uint32_t *color, uint32_t ncolor, ColorTable tab, uint16_t *map) {
    const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
    if (ci >= PAL_CAP) return;
    uint32_t r = 0xFFFFu;
    if (ci < ncolor && ci < MAX_COLORS) {
        const uint32_t col = color[ci];
        if (entry_names<DATA>(col)) r = color_lookup(tab, col);  // 0xFFFF where no reachable value names the colour
    }
    map[ci] = (uint16_t)r;
}

// the selected halves of v through their maps; a half of 0xFFFF names nothing and stays
template <uint32_t H>
__device__ inline uint32_t remap(uint32_t v, const uint16_t *__restrict__ map, const uint16_t *__restrict__ dmap) {
    const uint32_t ci = v & 0xFFFFu, di = v >> 16;
    if (H == H_COLOR) return ci == 0xFFFFu ? v : (v & 0xFFFF0000u) | map[ci];
    if (H == H_DATA) return di == 0xFFFFu ? v : ci | (uint32_t)dmap[di] << 16;
    const uint32_t lo = ci == 0xFFFFu ? ci : map[ci], hi = di == 0xFFFFu ? di : dmap[di];
    return lo | hi << 16;
}

// The rewrite: a workgroup owns REWRITE_ITEMS * 256 consecutive 16-byte words of the voxel buffer. The loads of a thread
// are issued before its stores; a word that does not change is not stored.
constexpr uint32_t REWRITE_ITEMS = 4;
template <uint32_t H>
__global__ __launch_bounds__(256) void k_plt_rewrite(uint4 *vox, uint64_t w0, uint64_t nwords,
                                                     const uint16_t *__restrict__ map,
                                                     const uint16_t *__restrict__ dmap) {
    const uint64_t base = w0 + (uint64_t)blockIdx.x * (256u * REWRITE_ITEMS) + threadIdx.x;
    uint4 v[REWRITE_ITEMS];
#pragma unroll
    for (uint32_t u = 0; u < REWRITE_ITEMS; ++u) {
        const uint64_t w = base + 256ull * u;
        if (w < nwords) v[u] = vox[w];
    }
#pragma unroll
    for (uint32_t u = 0; u < REWRITE_ITEMS; ++u) {
        const uint64_t w = base + 256ull * u;
        if (w >= nwords) continue;
        const uint4 a = v[u];
        uint4 r;
        r.x = remap<H>(a.x, map, dmap);
        r.y = a.y == a.x ? r.x : remap<H>(a.y, map, dmap);
        r.z = a.z == a.y ? r.y : remap<H>(a.z, map, dmap);
        r.w = a.w == a.z ? r.z : remap<H>(a.w, map, dmap);
        if (r.x != a.x || r.y != a.y || r.z != a.z || r.w != a.w) vox[w] = r;
    }
}

// brick_dim 1: a brick is one dword, and the buffer no multiple of 16 bytes
template <uint32_t H>
__global__ __launch_bounds__(256) void k_plt_rewrite1(uint32_t *vox, uint64_t ncells, const uint16_t *__restrict__ map,
                                                      const uint16_t *__restrict__ dmap) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ncells) return;
    const uint32_t a = vox[i], r = remap<H>(a, map, dmap);
    if (r != a) vox[i] = r;
}

// solid_values through the maps, and the new palettes of the selected halves (new_count <= color_count, new_dcount <=
// data_count: checked at the readback)
template <uint32_t H>
__global__ __launch_bounds__(256) void k_plt_tail(uint32_t *solids, uint32_t solid_count, uint32_t *color,
                                                  uint32_t new_count, const uint32_t *pal,
                                                  const uint16_t *__restrict__ map, uint32_t *data, uint32_t new_dcount,
                                                  const uint32_t *dpal, const uint16_t *__restrict__ dmap) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < solid_count) solids[i] = remap<H>(solids[i], map, dmap);
    if ((H & H_COLOR) && i < new_count) color[i] = pal[i];
    if ((H & H_DATA) && i < new_dcount) data[i] = dpal[i];
}

// the launches that are templates on the halves, for the mask of this call
#define PLT_DISPATCH(which, CALL)    \
    switch (which) {                 \
        case H_COLOR: CALL(1u); break; \
        case H_DATA: CALL(2u); break;  \
        default: CALL(3u); break;      \
    }

// vhx_compact_palette (which = H_COLOR, fn its name) and vhx_compact_palettes
int compact_palettes(vhx_ctx *c, uint32_t which, uint32_t *colors_dropped, uint32_t *data_dropped, const char *fn) {
    if (!c) return VHX_E_INVALID_ARG;
    const std::string name(fn);
    if (which == 0 || (which & ~(H_COLOR | H_DATA)))
        return fail(c, VHX_E_INVALID_ARG, name + ": which must be VHX_PALETTE_COLOR, VHX_PALETTE_DATA or both");
    if (c->shared) return fail(c, VHX_E_STATE, name + " on a shared context: call it through the owner");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, name + " before vhx_upload_tree");
    if (c->tree->mips_on) return fail(c, VHX_E_STATE, name + " while node MIPs are set");
    const bool do_color = (which & H_COLOR) != 0, do_data = (which & H_DATA) != 0;
    const vhx_tree_desc d = c->tree->desc;
    const uint64_t nn = d.node_count, nb = d.brick_count;
    const uint64_t n3 = (uint64_t)d.brick_dim * d.brick_dim * d.brick_dim;

    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    vhx::WriteScope ws(c);  // frames in flight on the tree's other contexts finish reading it first
    int rc = ws.rc;
    if (rc) return rc;
    Maps m;
    CompactCtl *wctl;
    if ((rc = ensure_maps(c, nn, nb, &m, &wctl))) return rc;
    vhx_ctx::PaletteScratch &ps = c->palette;
    if ((rc = vhx::ensure(c, ps.org, nn * 16))) return rc;
    if ((rc = vhx::ensure(c, ps.ctl, sizeof(PaletteCtl)))) return rc;
    if (do_color) {
        if ((rc = vhx::ensure(c, ps.first, (uint64_t)PAL_CAP * 8))) return rc;
        if ((rc = vhx::ensure(c, ps.map, (uint64_t)PAL_CAP * 2))) return rc;
        if ((rc = vhx::ensure(c, c->build.table, TAB_BYTES))) return rc;
    }
    if (do_data) {
        if ((rc = vhx::ensure(c, ps.dfirst, (uint64_t)PAL_CAP * 8))) return rc;
        if ((rc = vhx::ensure(c, ps.dmap, (uint64_t)PAL_CAP * 2))) return rc;
        if ((rc = vhx::ensure(c, c->build.dtable, TAB_BYTES))) return rc;
    }
    uint4 *org = (uint4 *)ps.org.ptr;
    // the arrays of a half that is not selected are null, and no kernel instantiated without the half touches them
    u64 *first = do_color ? (u64 *)ps.first.ptr : nullptr, *dfirst = do_data ? (u64 *)ps.dfirst.ptr : nullptr;
    uint16_t *map = do_color ? (uint16_t *)ps.map.ptr : nullptr, *dmap = do_data ? (uint16_t *)ps.dmap.ptr : nullptr;
    PaletteCtl *ctl = (PaletteCtl *)ps.ctl.ptr;
    const ColorTable tab = do_color ? table_of(c->build.table.ptr) : ColorTable{};
    const ColorTable dtab = do_data ? table_of(c->build.dtable.ptr) : ColorTable{};
    TreeStore &ts = *c->tree;
    const OldTree t{(const uint32_t *)ts.raw[VHX_BUF_NODE_TYPE].ptr, (const u64 *)ts.raw[VHX_BUF_NODE_OCBITS].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_NODE_CHILDREN].ptr, d.node_count, d.brick_count};
    uint32_t *vox = (uint32_t *)ts.raw[VHX_BUF_VOXELS].ptr;
    uint32_t *solids = (uint32_t *)ts.raw[VHX_BUF_SOLID_VALUES].ptr;
    uint32_t *color = (uint32_t *)ts.raw[VHX_BUF_COLOR_PALETTE].ptr;
    uint32_t *data = (uint32_t *)ts.raw[VHX_BUF_DATA_PALETTE].ptr;
    const MarkIn in{vox, solids, d.solid_count, lg2(d.brick_dim), d.boxtree_size};
    // reset: no counts, no node placed, no index seen, empty tables
    VHX_HIP(c, hipMemsetAsync(ctl, 0, sizeof(PaletteCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(org, 0xFF, nn * 16, c->stream));
    if (do_color) {
        VHX_HIP(c, hipMemsetAsync(first, 0xFF, (uint64_t)PAL_CAP * 8, c->stream));
        VHX_HIP(c, hipMemsetAsync(tab.keys, 0, TAB_KEYS_BYTES, c->stream));
        VHX_HIP(c, hipMemsetAsync(tab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    }
    if (do_data) {
        VHX_HIP(c, hipMemsetAsync(dfirst, 0xFF, (uint64_t)PAL_CAP * 8, c->stream));
        VHX_HIP(c, hipMemsetAsync(dtab.keys, 0, TAB_KEYS_BYTES, c->stream));
        VHX_HIP(c, hipMemsetAsync(dtab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    }
    if ((rc = walk_and_claim(c, t, m, &ctl->w, false))) return rc;  // (resets ctl->w itself)

    k_plt_origin_root<<<1, 1, 0, c->stream>>>(org);
    {
        uint64_t level_cap = 1, upto_cap = 1;  // as the walk: level lv holds at most 64^lv nodes
        for (uint32_t lv = 0; lv + 1 < MAX_LEVELS; ++lv) {
            k_plt_origin<<<blocks_for(std::min(upto_cap, nn) * 64), 256, 0, c->stream>>>(m, ctl, org, lv, d.boxtree_size,
                                                                                        d.node_count);
            if (level_cap >= nn) level_cap = nn; else level_cap *= 64;
            upto_cap = std::min(nn, upto_cap + level_cap);
        }
    }
    const unsigned mark_blocks = (unsigned)std::min<uint64_t>(nn, (uint64_t)c->cus * 32);
#define PLT_MARK(H) k_plt_mark<H><<<mark_blocks, 256, 0, c->stream>>>(t, m, in, org, first, ctl, dfirst)
    PLT_DISPATCH(which, PLT_MARK)
#undef PLT_MARK
    if (do_color) {
        k_plt_merge<false><<<PAL_CAP / 256, 256, 0, c->stream>>>(color, d.color_count, first, tab, &ctl->b);
        k_plt_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(tab, &ctl->b);
        k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->b);
        k_plt_map<false><<<PAL_CAP / 256, 256, 0, c->stream>>>(color, d.color_count, tab, map);
    }
    if (do_data) {
        k_plt_merge<true><<<PAL_CAP / 256, 256, 0, c->stream>>>(data, d.data_count, dfirst, dtab, &ctl->d);
        k_plt_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(dtab, &ctl->d);
        k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(dtab, &ctl->d);
        k_plt_map<true><<<PAL_CAP / 256, 256, 0, c->stream>>>(data, d.data_count, dtab, dmap);
    }
    VHX_HIP(c, hipGetLastError());

    // the one readback; the tree has only been read
    PaletteCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.w.bad & BAD_INDEX)
        return fail(c, VHX_E_STATE, name + ": a child, brick or solid value index at or past its count");
    if (h.w.bad & BAD_TWICE) return fail(c, VHX_E_STATE, name + ": a node or Parted brick is reached twice");
    if (h.w.bad & BAD_DEEP) return fail(c, VHX_E_STATE, name + ": more than 8 node levels");
    if (h.w.bad & BAD_SMALL) return fail(c, VHX_E_STATE, name + ": a leaf whose cells are smaller than a voxel");
    if (h.w.end == 0 || h.w.end > nn || h.w.brick_total > nb || h.b.overflow || h.b.ncompact != h.b.ncolors ||
        h.b.ncolors > d.color_count || h.d.overflow || h.d.ncompact != h.d.ncolors || h.d.ncolors > d.data_count)
        return fail(c, VHX_E_STATE, name + ": inconsistent counts");
    const uint32_t new_count = do_color ? h.b.ncolors : d.color_count;
    const uint32_t new_dcount = do_data ? h.d.ncolors : d.data_count;

    const bool stamped = hipEventRecord(c->ev0, c->stream) == hipSuccess;  // vhx_sync reports the rewrite pass
    const uint64_t ncells = nb * n3;
    if (n3 < 4) {
#define PLT_REWRITE1(H) k_plt_rewrite1<H><<<blocks_for(ncells), 256, 0, c->stream>>>(vox, ncells, map, dmap)
        if (ncells) PLT_DISPATCH(which, PLT_REWRITE1)
#undef PLT_REWRITE1
    } else {
        const uint64_t nwords = ncells / 4, per_block = 256ull * REWRITE_ITEMS;
        const uint64_t chunk = per_block << 22;  // launches of at most 2^22 workgroups
        for (uint64_t w0 = 0; w0 < nwords; w0 += chunk) {
            const uint64_t n = std::min(chunk, nwords - w0);
            const unsigned blocks = (unsigned)((n + per_block - 1) / per_block);
#define PLT_REWRITE(H) k_plt_rewrite<H><<<blocks, 256, 0, c->stream>>>((uint4 *)vox, w0, nwords, map, dmap)
            PLT_DISPATCH(which, PLT_REWRITE)
#undef PLT_REWRITE
        }
    }
    c->timed = hipEventRecord(c->ev1, c->stream) == hipSuccess && stamped;
    // the palettes of a half that is not selected are not written (the kernel is instantiated without that store)
    const uint32_t tail_n = std::max(d.solid_count, std::max(do_color ? new_count : 0u, do_data ? new_dcount : 0u));
#define PLT_TAIL(H)                                                                                              \
    k_plt_tail<H><<<blocks_for(tail_n), 256, 0, c->stream>>>(solids, d.solid_count, color, new_count, tab.pal, map, \
                                                             data, new_dcount, dtab.pal, dmap)
    if (tail_n) PLT_DISPATCH(which, PLT_TAIL)
#undef PLT_TAIL
    hipError_t e = hipGetLastError();
    ts.desc.color_count = new_count;
    ts.desc.data_count = new_dcount;
    // an orphaned slot may hold cells whose colour or data value left its palette: its bitmap follows its cells, as
    // after an upload
    if (e == hipSuccess && h.w.brick_total < nb && vhx::rederive_bricks(c) != VHX_OK)
        e = hipErrorUnknown;
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, VHX_E_HIP, name + ": " + hipGetErrorString(e));
    if (colors_dropped) *colors_dropped = d.color_count - new_count;
    if (data_dropped) *data_dropped = d.data_count - new_dcount;
    return ws.end();  // the next trace of every context of the tree waits for this write
}

}  // namespace

extern "C" {

int vhx_compact_palette(vhx_ctx *c, uint32_t *colors_dropped) {
    return compact_palettes(c, VHX_PALETTE_COLOR, colors_dropped, nullptr, "vhx_compact_palette");
}

int vhx_compact_palettes(vhx_ctx *c, uint32_t which, uint32_t *colors_dropped, uint32_t *data_dropped) {
    return compact_palettes(c, which, colors_dropped, data_dropped, "vhx_compact_palettes");
}

}  // extern "C"
