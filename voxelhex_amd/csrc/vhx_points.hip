// vhx_set_voxels: a list of points written into (or cleared from) the device tree, in place.
//
// vhx_write_dense (vhx_edit.hip) with sparse per-level lists of touched cubes in place of the box's lattices: the work
// and the scratch follow the points and the bricks they touch, not their bounding box. A point is effective when its
// mode lets it decide its voxel (replace: every point; insert and update: a point with a colour or a data value). The
// passes:
//
//   first    k_pts_first     bounds, the points' colours and data values into the tables (first index NEW_BASE + i), the
//                            root's sectants that hold an effective point
//   descend  k_pts_descend   per level, after a scan of the popcounts of the level's sectant masks: the old node of
//                            every touched child cube from its parent's old node and children[] (the canonical-depth
//                            flag is raised as k_edit_walk raises it), every point on to its child cube
//                            (first[parent] + popcount(mask[parent] below its sectant)), and its sectant there ORed in.
//                            A touched leaf whose UniformLeaf brick is Parted touches all its 64 bricks
//   -- a readback of the counts: refusals for positions outside the cube and foreign depth; the brick lists are sized --
//   group    k_pts_count, k_scan_*, k_pts_scatter   point indices in per-brick segments (any order inside a segment)
//   bricks   k_pts_brick<0>  a wave per touched brick: the highest point index per cell by atomicMax in LDS (chunks of
//                            1024 cells), the old bitmap, Solid value or uniform cell for the undecided cells, the
//                            brick's bitmap after the write by ballot; "exists", "needs a new slot", "orphaned".
//                            VHX_WRITE_UPDATE (UPD = 1) keeps two maxima per cell, the highest point
//                            with a colour half and the highest with a data half, and splices them into the old cell
//   levels   k_pts_leaf, k_pts_reduce   occupancy after the write, upwards; "must exist and does not" per cube
//   scans, palette  as vhx_write_dense
//   -- the last readback of counters; nothing of the tree has been written so far; then the buffers grow --
//   emit     k_pts_brick<1>  voxels, bitmaps, entries and child records of the touched bricks
//            k_pts_nodes     types, occupancy, headers, entries and child records of the touched cubes, per level
//
// Numbering: the touched cubes of a level are ordered by their parent's order, then by sectant, so every rank below is
// a pure function of the old image and the list. Every global write of the tree is a plain store; the atomics are ORs,
// maxima and minima, table claims and counts.
#include <algorithm>
#include <string>

#include "../../include/vhx.h"
#include "buildtab.hpp"
#include "ctx.hpp"
#include "edittab.hpp"
#include "treewalk.hpp"

namespace {

constexpr uint32_t CHUNK = 1024;  // cells of a brick a wave decides at a time (4 KiB of LDS per wave)
constexpr uint32_t B_EXISTS = 1u, B_NEWSLOT = 2u, B_ORPHAN = 4u;

struct PtsCtl {
    EditCtl e;
    u64 count[MAX_LEVELS + 2];  // touched cubes per level (the root: 1), [D + 1] touched bricks, [D + 2] effective points
    uint32_t oob;               // a position outside the root cube
    uint32_t neff;              // an effective point exists
};

struct PtsP {
    const uint32_t *pos, *albedo, *data;  // albedo / data null: every point's word is fill / dfill
    uint64_t n;
    uint32_t fill, dfill, mode;
    uint32_t lg_size, lg_bd, D;
    uint64_t off[MAX_LEVELS];       // the level's first cube in the per-cube arrays
    uint32_t new_base[MAX_LEVELS];  // emission: index of the level's first new node
};

struct PtsS {
    uint32_t *cur;    // [n]      the point's cube in the current level, at last its brick; NONE = not effective
    u64 *mask;        // [total]  sectants of the cube that hold an effective point
    u64 *first;       // [total]  index of the cube's first touched child in the next level
    uint32_t *oldn;   // [total]  old node of the cube, NONE = none
    u64 *aft;         // [total]  occupancy after the write
    u64 *need;        // [total]  1 = the cube needs a new node
    u64 *rank;        // [total]  rank of that node among the level's new nodes
    uint32_t *ltype;  // [leaves] old type of the leaf cube's node
    uint32_t *lu;     // [leaves] a UniformLeaf's brick descriptor, else VHX_EMPTY
    u64 *nmask;       // [leaves] bricks that need a new slot
    u64 *bfirst;      // [leaves] rank of the leaf's first new brick
    u64 *binfo;       // [bricks] leaf cube * 64 + sectant
    u64 *bcnt;        // [bricks] points of the brick (counted down again by the scatter)
    u64 *bseg;        // [bricks] the brick's first entry in idx
    uint32_t *bflag;  // [bricks] B_EXISTS, B_NEWSLOT
    uint32_t *idx;    // [n]      point indices, grouped by brick
};

__device__ inline void point_words(const PtsP &p, uint64_t i, uint32_t &a, uint32_t &d) {
    a = p.albedo ? p.albedo[i] : p.fill;
    d = p.data ? p.data[i] : p.dfill;
}

__device__ inline bool is_uparted(const TreeP &t, uint32_t ty, uint32_t u) {
    return ty == VHX_NODE_UNIFORM_LEAF && u != VHX_EMPTY && (u & VHX_SOLID_BIT) == 0 && u < t.brick_count;
}

// raises *p once per wave; every lane of the wave calls it
__device__ inline void wave_flag(uint32_t *p, bool f) {
    if (__any(f) && (threadIdx.x & 63u) == 0) atomicOr(p, 1u);
}

// adds the wave's sum of v to *p with one atomic; every lane of the wave calls it
__device__ inline void wave_add(uint32_t *p, uint32_t v) {
#pragma unroll
    for (uint32_t k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k);
    if (v && (threadIdx.x & 63u) == 0) atomicAdd(p, v);
}

// ORs `bit` into mask[cube] for the lanes with `on`. Every lane of the wave calls it: a wave whose points share the cube
// (the upper levels) reduces its bits first, and a bit that is already there costs no atomic (bits are only ever set).
__device__ inline void mark(u64 *mask, uint64_t cube, u64 bit, bool on) {
    const u64 act = __ballot(on);
    if (act == 0) return;
    const uint64_t c0 = __shfl(cube, (int)__ffsll((long long)act) - 1);
    u64 m = on ? bit : 0ull;
    if (__all(!on || cube == c0)) {
#pragma unroll
        for (uint32_t k = 1; k < 64; k <<= 1) m |= __shfl_xor(m, k);
        if ((threadIdx.x & 63u) == 0 && (mask[c0] & m) != m) atomicOr(&mask[c0], m);
    } else if (on && (mask[cube] & m) != m) {
        atomicOr(&mask[cube], m);
    }
}

// old type and uniform brick of a touched leaf cube; true for a UniformLeaf whose brick is Parted
__device__ inline bool leaf_info(const TreeP &t, const PtsS &s, uint64_t leaf, uint32_t node) {
    const uint32_t ty = node != NONE ? t.type[node] : VHX_NODE_NOTHING;
    const uint32_t u = ty == VHX_NODE_UNIFORM_LEAF ? t.children[(uint64_t)node * 64u] : VHX_EMPTY;
    s.ltype[leaf] = ty;
    s.lu[leaf] = u;
    return is_uparted(t, ty, u);
}

__global__ __launch_bounds__(256) void k_pts_first(PtsP p, TreeP t, PtsS s, ColorTable tab, ColorTable dtab, PtsCtl *ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {  // the root: the one cube of level 0
        const uint32_t ty = t.type[0];
        const bool is_leaf = ty == VHX_NODE_LEAF || ty == VHX_NODE_UNIFORM_LEAF;
        if (p.D > 0 ? is_leaf : ty == VHX_NODE_INTERNAL) atomicOr(&ctl->e.bad, 1u);
        s.oldn[0] = 0;
        ctl->count[0] = 1;
        if (p.D == 0 && leaf_info(t, s, 0, 0)) atomicOr(&s.mask[0], ~0ull);
    }
    bool oob = false, eff = false;
    u64 bit = 0;
    if (i < p.n) {
        const uint32_t x = p.pos[3 * i], y = p.pos[3 * i + 1], z = p.pos[3 * i + 2];
        const uint32_t size = 1u << p.lg_size;
        oob = x >= size || y >= size || z >= size;
        uint32_t a, d;
        point_words(p, i, a, d);
        const bool col = (a >> 24) != 0;
        eff = !oob && (p.mode == VHX_WRITE_REPLACE || col || d != 0);
        s.cur[i] = eff ? 0u : NONE;
        if (eff) {
            bit = 1ull << sectant_of(x, y, z, p.lg_size);
            // the values of every effective point, overridden ones included: the sequential loop would add them too.
            // A run of points with one value records it once, at the run's first point
            uint32_t pa = 0, pd = 0;
            bool peff = false;  // the point before is effective
            if (i > 0) {
                point_words(p, i - 1, pa, pd);
                peff = p.mode == VHX_WRITE_REPLACE || (pa >> 24) != 0 || pd != 0;
            }
            if (col && !(peff && pa == a)) color_insert(tab, &ctl->e.b, a, NEW_BASE + i);
            if (d != 0 && !(peff && pd == d)) color_insert(dtab, &ctl->e.d, d, NEW_BASE + i);
        }
    }
    wave_flag(&ctl->oob, oob);
    wave_flag(&ctl->neff, eff);
    mark(s.mask, 0, bit, eff);
}

// level lv <= D. One thread per (cube, sectant): the touched child's old node. One thread per point: on to its child.
__global__ __launch_bounds__(256) void k_pts_descend(PtsP p, TreeP t, PtsS s, PtsCtl *ctl, uint32_t lv) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t off = p.off[lv];
    if (lv < p.D && (gid >> 6) < ctl->count[lv]) {
        const uint64_t cube = gid >> 6;
        const uint32_t sec = (uint32_t)gid & 63u;
        const u64 m = s.mask[off + cube];
        if ((m >> sec) & 1ull) {
            const uint64_t child = s.first[off + cube] + (uint32_t)__popcll(m & ((1ull << sec) - 1ull));
            uint32_t node = s.oldn[off + cube];
            bool bad = false;
            if (node != NONE) {
                const uint32_t ty = t.type[node];
                if (ty != VHX_NODE_INTERNAL) {
                    bad = !(lv == 0 && ty == VHX_NODE_NOTHING);  // an empty tree's root; else a leaf above the lowest level
                    node = NONE;
                } else {
                    const uint32_t e = t.children[(uint64_t)node * 64u + sec];
                    if (e == VHX_EMPTY || e >= t.node_count) {
                        bad = e != VHX_EMPTY || ((t.ocbits[node] >> sec) & 1ull) != 0;  // occupied, the child not in this view
                        node = NONE;
                    } else {
                        node = e;
                        const uint32_t cty = t.type[e];
                        const bool is_leaf = cty == VHX_NODE_LEAF || cty == VHX_NODE_UNIFORM_LEAF;
                        if (lv + 1 < p.D ? is_leaf : cty == VHX_NODE_INTERNAL) bad = true;
                    }
                }
            }
            s.oldn[p.off[lv + 1] + child] = node;
            if (bad) atomicOr(&ctl->e.bad, 1u);
            if (lv + 1 == p.D && leaf_info(t, s, child, node)) atomicOr(&s.mask[p.off[p.D] + child], ~0ull);
        }
    }
    bool on = false;
    uint64_t child = 0;
    u64 bit = 0;
    if (gid < p.n) {
        const uint32_t cube = s.cur[gid];
        if (cube != NONE) {
            const uint32_t x = p.pos[3 * gid], y = p.pos[3 * gid + 1], z = p.pos[3 * gid + 2];
            const uint32_t sec = sectant_of(x, y, z, p.lg_size - 2u * lv);
            const u64 m = s.mask[off + cube];
            child = s.first[off + cube] + (uint32_t)__popcll(m & ((1ull << sec) - 1ull));
            s.cur[gid] = (uint32_t)child;  // below 2^31 (checked at the readback before a brick index is used)
            if (lv < p.D) {
                on = true;
                bit = 1ull << sectant_of(x, y, z, p.lg_size - 2u * (lv + 1u));
            }
        }
    }
    if (lv < p.D) mark(s.mask + p.off[lv + 1], child, bit, on);
}

// one thread per (leaf cube, sectant): the touched brick's place; one thread per point: its brick's count
__global__ __launch_bounds__(256) void k_pts_count(PtsP p, PtsS s, uint64_t nleaf) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if ((gid >> 6) < nleaf) {
        const uint32_t sec = (uint32_t)gid & 63u;
        const u64 m = s.mask[p.off[p.D] + (gid >> 6)];
        if ((m >> sec) & 1ull) s.binfo[s.first[p.off[p.D] + (gid >> 6)] + (uint32_t)__popcll(m & ((1ull << sec) - 1ull))] = gid;
    }
    const uint32_t b = gid < p.n ? s.cur[gid] : NONE;
    const bool on = b != NONE;
    const u64 act = __ballot(on);
    if (act == 0) return;
    const uint32_t b0 = __shfl(b, (int)__ffsll((long long)act) - 1);
    if (__all(!on || b == b0)) {  // the wave's points share the brick: one count
        if ((threadIdx.x & 63u) == 0) atomicAdd(&s.bcnt[b0], (u64)__popcll(act));
    } else if (on) {
        atomicAdd(&s.bcnt[b], 1ull);
    }
}

// the point's index into its brick's segment: the count, counted down, gives the places (their order is free)
__global__ __launch_bounds__(256) void k_pts_scatter(PtsP p, PtsS s) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t b = gid < p.n ? s.cur[gid] : NONE;
    if (b == NONE) return;
    const u64 left = atomicAdd(&s.bcnt[b], ~0ull);  // minus one
    s.idx[s.bseg[b] + left - 1ull] = (uint32_t)gid;
}

// The wave's winners in LDS. REPLACE and INSERT keep their static 4 x 1024 words; UPDATE has two arrays per wave (colour
// winners, then data winners), sized to the chunk at launch: 2 KiB per workgroup at brick_dim 4, 32 KiB from brick_dim 16.
template <int UPD>
__device__ __forceinline__ uint32_t *win_lds(uint32_t wave, uint32_t ch);
template <>
__device__ __forceinline__ uint32_t *win_lds<0>(uint32_t wave, uint32_t) {
    __shared__ uint32_t s_win[4][CHUNK];
    return s_win[wave];
}
template <>
__device__ __forceinline__ uint32_t *win_lds<1>(uint32_t wave, uint32_t ch) {
    extern __shared__ uint32_t s_dyn[];
    return s_dyn + wave * ch;
}

// The touched bricks, a wave each. EMIT = 0 analyses (reads the tree only), EMIT = 1 writes; both derive the brick's
// bitmap after the write the same way. Loop bounds are wave uniform: the ballots run with all 64 lanes.
// UPD = 1 (VHX_WRITE_UPDATE): a cell has two winners, the highest point with a colour half and the highest with a data
// half (a second array of the chunk's size); a decided cell is the old raw cell with the decided halves replaced, and
// is never empty.
template <int EMIT, int UPD>
__global__ __launch_bounds__(256) void k_pts_brick(PtsP p, TreeP t, PtsS s, ColorTable tab, ColorTable dtab, PtsCtl *ctl,
                                                   uint64_t nb) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * 4u + wave;
    if (b >= nb) return;  // the whole wave; the kernel has no workgroup barrier
    // per cell of the chunk: the highest index of a point there, plus 1; 0 = none
    uint32_t *win = win_lds<UPD>(wave, min(1u << (3u * p.lg_bd), CHUNK));
    uint32_t *wind = win + (UPD ? 4u * min(1u << (3u * p.lg_bd), CHUNK) : 0u);  // UPD: the data halves' winners
    const uint64_t info = s.binfo[b];
    const uint64_t L = info >> 6, LL = p.off[p.D] + L;
    const uint32_t sec = (uint32_t)info & 63u;
    const u64 bit = 1ull << sec;
    const u64 laft = EMIT ? s.aft[LL] : 0ull;
    if (EMIT && laft == 0) return;  // k_pts_nodes clears a leaf that leaves
    const uint32_t node = s.oldn[LL], ty = s.ltype[L], u = s.lu[L];
    const bool leaf = ty == VHX_NODE_LEAF;
    const bool uparted = is_uparted(t, ty, u);
    uint32_t d = leaf ? t.children[(uint64_t)node * 64u + sec] : u;
    const bool dsolid = d != VHX_EMPTY && (d & VHX_SOLID_BIT) != 0;
    if (d != VHX_EMPTY && !dsolid && d >= t.brick_count) d = VHX_EMPTY;  // not a brick of this tree
    const bool own = leaf && d != VHX_EMPTY && !dsolid;
    const uint32_t ni = EMIT ? (node != NONE ? node : p.new_base[p.D] + (uint32_t)s.rank[LL]) : 0u;
    const uint64_t at = (uint64_t)ni * 64u + sec;
    if (EMIT && ((laft >> sec) & 1ull) == 0) {  // the brick leaves, or never was
        if (lane == 0) {
            t.children[at] = VHX_EMPTY;
            if (t.rec) t.rec[at] = make_uint4(VHX_EMPTY, 0u, 0u, 0u);
        }
        return;
    }
    uint32_t sraw = VHX_EMPTY;
    if (dsolid && (d & 0x7FFFFFFFu) < t.solid_count) sraw = t.solid[d & 0x7FFFFFFFu];
    const bool sne = !cell_empty(sraw, t.color, t.color_count, t.data, t.data_count);
    const uint32_t slot =
        !EMIT ? 0u : own ? d : t.brick_count + (uint32_t)s.bfirst[L] + (uint32_t)__popcll(s.nmask[L] & (bit - 1ull));
    const uint32_t bd = 1u << p.lg_bd, n3 = 1u << (3u * p.lg_bd), ch = min(n3, CHUNK);
    const uint64_t j0 = s.bseg[b], j1 = b + 1 < nb ? s.bseg[b + 1] : ctl->count[p.D + 2];
    u64 any = 0, word0 = 0;
    for (uint32_t c0 = 0; c0 < n3; c0 += ch) {
        for (uint32_t k = lane; k < ch; k += 64u) {
            win[k] = 0u;
            if (UPD) wind[k] = 0u;
        }
        __threadfence_block();  // the wave's LDS operations run in order; this keeps the compiler from moving them
        for (uint64_t j = j0 + lane; j < j1; j += 64u) {
            const uint32_t i = s.idx[j];
            const uint32_t x = p.pos[3ull * i], y = p.pos[3ull * i + 1], z = p.pos[3ull * i + 2];
            const uint32_t c = (x & (bd - 1u)) | ((y & (bd - 1u)) << p.lg_bd) | ((z & (bd - 1u)) << (2u * p.lg_bd));
            if (c - c0 < ch) {
                if (UPD) {  // every point of a segment is effective: it has one half at least
                    uint32_t pa, pd;
                    point_words(p, i, pa, pd);
                    if ((pa >> 24) != 0) atomicMax(&win[c - c0], i + 1u);
                    if (pd != 0) atomicMax(&wind[c - c0], i + 1u);
                } else {
                    atomicMax(&win[c - c0], i + 1u);
                }
            }
        }
        __threadfence_block();
        for (uint32_t k0 = 0; k0 < ch; k0 += 64u) {
            const uint32_t k = k0 + lane, c = c0 + k;
            const bool valid = k < ch;
            const uint32_t w = valid ? win[k] : 0u;
            const uint32_t wd = UPD && valid ? wind[k] : 0u;
            const bool decided = (w | wd) != 0u;
            uint32_t a = 0, dv = 0;
            if (UPD) {  // each half from its own winner
                if (w) a = p.albedo ? p.albedo[w - 1u] : p.fill;
                if (wd) dv = p.data ? p.data[wd - 1u] : p.dfill;
            } else if (decided) {
                point_words(p, w - 1u, a, dv);
            }
            const bool col = (a >> 24) != 0;
            const bool vis = col || dv != 0;  // the deciding point writes an entry; else it clears (replace mode)
            uint32_t raw = VHX_EMPTY;
            bool ne = false;
            if (own) {
                const u64 word = t.occ[(uint64_t)d * t.occ_words + (c >> 6)];
                ne = ((word >> (c & 63u)) & 1ull) != 0;
            } else if (dsolid) {
                raw = sraw;
                ne = sne;
            } else if (uparted && valid) {  // the uniform brick's cell over this voxel
                const uint32_t vx = ((sec & 3u) << p.lg_bd) + (c & (bd - 1u)),
                               vy = (((sec >> 2) & 3u) << p.lg_bd) + ((c >> p.lg_bd) & (bd - 1u)),
                               vz = ((sec >> 4) << p.lg_bd) + (c >> (2u * p.lg_bd));
                const uint32_t ucell = (vx >> 2) + (((vy >> 2) + ((vz >> 2) << p.lg_bd)) << p.lg_bd);
                raw = t.voxels[((uint64_t)u << (3u * p.lg_bd)) + ucell];
                ne = !cell_empty(raw, t.color, t.color_count, t.data, t.data_count);
            }
            const bool after = valid && (decided ? vis : ne);
            const u64 word = __ballot(after);
            any |= word;
            if (c0 + k0 == 0) word0 = word;
            if (EMIT) {
                const uint64_t va = ((uint64_t)slot << (3u * p.lg_bd)) + c;
                if (UPD && decided) {
                    // pix_overwrite_color / pix_overwrite_data on the old raw cell (VHX_EMPTY where there was none); an
                    // own brick's cell is read here, and only where a half of it is kept
                    uint32_t v = own ? ((col && dv) ? 0u : t.voxels[va]) : raw;
                    if (col) v = (v & 0xFFFF0000u) | color_lookup(tab, a);
                    if (dv) v = (v & 0x0000FFFFu) | (color_lookup(dtab, dv) << 16);
                    t.voxels[va] = v;
                } else if (decided) {
                    uint32_t v = VHX_EMPTY;
                    // pix_visual, pix_informative, pix_complex: 0xFFFF for the half that is none
                    if (vis) v = (col ? color_lookup(tab, a) : 0xFFFFu) | ((dv ? color_lookup(dtab, dv) : 0xFFFFu) << 16);
                    t.voxels[va] = v;
                } else if (valid && !own) {
                    t.voxels[va] = raw;
                }
                if (lane == 0) t.occ[(uint64_t)slot * t.occ_words + ((c0 + k0) >> 6)] = word;
            }
        }
        __threadfence_block();  // the chunk is read before it is cleared for the next one
    }
    if (lane != 0) return;
    if (!EMIT) {
        // an emptied brick's slot is orphaned: k_pts_leaf counts those
        s.bflag[b] = (any ? B_EXISTS : 0u) | (any && !own ? B_NEWSLOT : 0u) | (!any && own ? B_ORPHAN : 0u);
    } else {
        t.children[at] = slot;
        if (t.rec) t.rec[at] = make_uint4(slot, (uint32_t)word0, (uint32_t)(word0 >> 32), 0u);
    }
}

// level D, one thread per touched leaf cube: its bricks after the write
__global__ __launch_bounds__(256) void k_pts_leaf(PtsP p, TreeP t, PtsS s, PtsCtl *ctl, uint64_t nleaf) {
    const uint64_t L = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t orph_b = 0, orph_n = 0;
    if (L < nleaf) {
        const uint64_t LL = p.off[p.D] + L;
        const uint32_t node = s.oldn[LL], ty = s.ltype[L], u = s.lu[L];
        const bool leaf = ty == VHX_NODE_LEAF;
        const u64 m = s.mask[LL];
        const uint64_t fb = s.first[LL];
        u64 a = 0, nm = 0;
        for (uint32_t sec = 0; sec < 64u; ++sec) {
            const u64 bit = 1ull << sec;
            if (m & bit) {
                const uint32_t f = s.bflag[fb + (uint32_t)__popcll(m & (bit - 1ull))];
                if (f & B_EXISTS) a |= bit;
                if (f & B_NEWSLOT) nm |= bit;
                if (f & B_ORPHAN) ++orph_b;
            } else {  // the brick stays as it is
                uint32_t d = leaf ? t.children[(uint64_t)node * 64u + sec] : u;
                if (d != VHX_EMPTY && (d & VHX_SOLID_BIT) == 0 && d >= t.brick_count) d = VHX_EMPTY;
                if (d != VHX_EMPTY) a |= bit;
            }
        }
        s.aft[LL] = a;
        s.nmask[L] = nm;
        s.need[LL] = (a != 0 && node == NONE) ? 1ull : 0ull;
        if (is_uparted(t, ty, u)) ++orph_b;  // an expanded leaf's uniform brick
        if (a == 0 && node != NONE && p.D != 0) orph_n = 1;
    }
    wave_add(&ctl->e.orphan_bricks, orph_b);
    wave_add(&ctl->e.orphan_nodes, orph_n);
}

// level lv < D, one thread per touched cube
__global__ __launch_bounds__(256) void k_pts_reduce(PtsP p, TreeP t, PtsS s, PtsCtl *ctl, uint32_t lv, uint64_t ncube) {
    const uint64_t cube = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t orph_n = 0;
    if (cube < ncube) {
        const uint64_t at = p.off[lv] + cube;
        const uint32_t node = s.oldn[at];
        u64 m = node != NONE ? t.ocbits[node] : 0ull;
        uint64_t child = p.off[lv + 1] + s.first[at];
        for (u64 left = s.mask[at]; left; left &= left - 1ull, ++child) {
            const u64 bit = left & (~left + 1ull);
            if (s.aft[child])
                m |= bit;
            else
                m &= ~bit;
        }
        s.aft[at] = m;
        s.need[at] = (m != 0 && node == NONE) ? 1ull : 0ull;
        if (m == 0 && node != NONE && lv != 0) orph_n = 1;
    }
    wave_add(&ctl->e.orphan_nodes, orph_n);
}

// level lv, one thread per (touched cube, sectant): the node's type, occupancy and header, and its entries outside the
// touched bricks (those are k_pts_brick<1>'s). A new node's other entries are empty (an expanded UniformLeaf's: its
// Solid brick), an old node's stay. A node that lost everything becomes Nothing.
__global__ __launch_bounds__(256) void k_pts_nodes(PtsP p, TreeP t, PtsS s, uint32_t lv, uint64_t ncube) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t cube = gid >> 6;
    const uint32_t sec = (uint32_t)gid & 63u;
    if (cube >= ncube) return;
    const uint64_t cc = p.off[lv] + cube;
    const uint32_t node = s.oldn[cc];
    const u64 a = s.aft[cc];
    if (node == NONE && a == 0) return;
    const uint32_t ni = node != NONE ? node : p.new_base[lv] + (uint32_t)s.rank[cc];
    const uint64_t at = (uint64_t)ni * 64u + sec;
    const uint32_t ty = a == 0 ? VHX_NODE_NOTHING : lv < p.D ? VHX_NODE_INTERNAL : VHX_NODE_LEAF;
    if (sec == 0) {
        t.type[ni] = ty;
        t.ocbits[ni] = a;
        t.hdr[ni] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), ty, 0u);
    }
    uint32_t e = VHX_EMPTY;
    if (a != 0) {
        const u64 m = s.mask[cc];
        const bool touched = ((m >> sec) & 1ull) != 0;
        if (lv == p.D) {
            if (touched) return;  // k_pts_brick wrote the entry
            if (node != NONE && s.ltype[cube] != VHX_NODE_UNIFORM_LEAF) return;  // an old leaf's entry stays
            e = s.lu[cube];
        } else if (!touched) {
            if (node != NONE) return;  // an old node's entry over no point
        } else {
            const uint64_t ci = p.off[lv + 1] + s.first[cc] + (uint32_t)__popcll(m & ((1ull << sec) - 1ull));
            if (s.aft[ci]) {
                const uint32_t cn = s.oldn[ci];
                e = cn != NONE ? cn : p.new_base[lv + 1] + (uint32_t)s.rank[ci];
            }
        }
    }
    t.children[at] = e;
    if (t.rec) t.rec[at] = make_uint4(e, 0u, 0u, 0u);
}

int set_voxels(vhx_ctx *c, const vhx_points_in *pts, int on_device) {
    if (!c || !pts) return fail(c, VHX_E_INVALID_ARG, "vhx_set_voxels: null argument");
    if (pts->n > 0 && !pts->positions) return fail(c, VHX_E_INVALID_ARG, "vhx_set_voxels: null positions");
    if (pts->n > (1ull << 31)) return fail(c, VHX_E_INVALID_ARG, "vhx_set_voxels: more than 2^31 points");
    if (pts->mode != VHX_WRITE_REPLACE && pts->mode != VHX_WRITE_INSERT && pts->mode != VHX_WRITE_UPDATE)
        return fail(c, VHX_E_INVALID_ARG, "vhx_set_voxels: unknown mode");
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_set_voxels on a shared context: write through the owner");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_set_voxels before vhx_upload_tree");
    if (c->tree->mips_on) return fail(c, VHX_E_STATE, "vhx_set_voxels while node MIPs are set");
    if (pts->n == 0) return VHX_OK;
    const vhx_tree_desc d = c->tree->desc;
    PtsP p{};
    p.n = pts->n;
    p.mode = pts->mode;
    p.fill = pts->fill;
    p.dfill = pts->fill_data;
    while ((1u << p.lg_size) < d.boxtree_size) ++p.lg_size;
    while ((1u << p.lg_bd) < d.brick_dim) ++p.lg_bd;
    if ((1u << p.lg_size) != d.boxtree_size || (1u << p.lg_bd) != d.brick_dim || p.lg_size < p.lg_bd + 2u ||
        ((p.lg_size - p.lg_bd) & 1u) || (p.lg_size - p.lg_bd) / 2u > MAX_LEVELS)
        return fail(c, VHX_E_STATE, "vhx_set_voxels: the tree's size is not brick_dim * 4^k");
    p.D = (p.lg_size - p.lg_bd) / 2u - 1u;
    // a level holds at most min(n, 64^lv) touched cubes
    uint64_t cap[MAX_LEVELS], total = 0, cap_max = 1;
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        cap[lv] = 6u * lv >= 31u ? p.n : std::min<uint64_t>(p.n, 1ull << (6u * lv));
        p.off[lv] = total;
        total += cap[lv];
        cap_max = std::max(cap_max, cap[lv]);
    }
    const bool with_data = pts->data != nullptr || pts->fill_data != 0u;

    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    vhx::WriteScope ws(c);  // frames in flight on the tree's other contexts finish reading it first
    int rc = ws.rc;
    if (rc) return rc;
    if ((rc = vhx::refresh_child_rec(c))) return rc;
    vhx_ctx::PointsScratch &ps = c->points;
    if ((rc = vhx::ensure(c, ps.cur, p.n * 4))) return rc;
    if ((rc = vhx::ensure(c, ps.idx, p.n * 4))) return rc;
    if ((rc = vhx::ensure(c, ps.mask, total * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.first, total * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.oldn, total * 4))) return rc;
    if ((rc = vhx::ensure(c, ps.aft, total * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.need, total * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.rank, total * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.ltype, cap[p.D] * 4))) return rc;
    if ((rc = vhx::ensure(c, ps.lu, cap[p.D] * 4))) return rc;
    if ((rc = vhx::ensure(c, ps.nmask, cap[p.D] * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.bfirst, cap[p.D] * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.ctl, sizeof(PtsCtl)))) return rc;
    if ((rc = vhx::ensure(c, c->build.part, ((cap_max + SCAN_TILE - 1) / SCAN_TILE) * 8))) return rc;
    if ((rc = vhx::ensure(c, c->build.table, TAB_BYTES))) return rc;
    if (with_data && (rc = vhx::ensure(c, c->build.dtable, TAB_BYTES))) return rc;
    p.pos = pts->positions;
    p.albedo = pts->albedo;
    p.data = pts->data;
    if (!on_device) {  // host arrays: positions, then the albedo and data words
        const uint64_t words = p.n * (3u + (pts->albedo ? 1u : 0u) + (pts->data ? 1u : 0u));
        if ((rc = vhx::ensure(c, ps.in, words * 4))) return rc;
        uint32_t *at = (uint32_t *)ps.in.ptr;
        VHX_HIP(c, hipMemcpyAsync(at, pts->positions, p.n * 12, hipMemcpyHostToDevice, c->stream));
        p.pos = at;
        at += p.n * 3;
        if (pts->albedo) {
            VHX_HIP(c, hipMemcpyAsync(at, pts->albedo, p.n * 4, hipMemcpyHostToDevice, c->stream));
            p.albedo = at;
            at += p.n;
        }
        if (pts->data) {
            VHX_HIP(c, hipMemcpyAsync(at, pts->data, p.n * 4, hipMemcpyHostToDevice, c->stream));
            p.data = at;
        }
    }
    PtsS s{};
    s.cur = (uint32_t *)ps.cur.ptr;
    s.idx = (uint32_t *)ps.idx.ptr;
    s.mask = (u64 *)ps.mask.ptr;
    s.first = (u64 *)ps.first.ptr;
    s.oldn = (uint32_t *)ps.oldn.ptr;
    s.aft = (u64 *)ps.aft.ptr;
    s.need = (u64 *)ps.need.ptr;
    s.rank = (u64 *)ps.rank.ptr;
    s.ltype = (uint32_t *)ps.ltype.ptr;
    s.lu = (uint32_t *)ps.lu.ptr;
    s.nmask = (u64 *)ps.nmask.ptr;
    s.bfirst = (u64 *)ps.bfirst.ptr;
    PtsCtl *ctl = (PtsCtl *)ps.ctl.ptr;
    const ColorTable tab = table_of(c->build.table.ptr);
    const ColorTable dtab = with_data ? table_of(c->build.dtable.ptr) : ColorTable{};
    TreeP t = tree_of(c, d);
    // reset: counters, sectant masks, table keys free, first indices at maximum (every other scratch word is written
    // before it is read)
    VHX_HIP(c, hipMemsetAsync(ctl, 0, sizeof(PtsCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(s.mask, 0, total * 8, c->stream));
    VHX_HIP(c, hipMemsetAsync(tab.keys, 0, TAB_KEYS_BYTES, c->stream));
    VHX_HIP(c, hipMemsetAsync(tab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    if (with_data) {
        VHX_HIP(c, hipMemsetAsync(dtab.keys, 0, TAB_KEYS_BYTES, c->stream));
        VHX_HIP(c, hipMemsetAsync(dtab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    }
    k_edit_seed<0><<<blocks_for((uint64_t)d.color_count + 1), 256, 0, c->stream>>>(tab, t.color, d.color_count, &ctl->e);
    if (with_data)
        k_edit_seed<1><<<blocks_for((uint64_t)d.data_count + 1), 256, 0, c->stream>>>(dtab, t.data, d.data_count, &ctl->e);
    k_pts_first<<<blocks_for(p.n), 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        if ((rc = scan_level<1>(c, s.mask + p.off[lv], cap[lv], false, s.first + p.off[lv], &ctl->count[lv + 1])))
            return rc;
        const uint64_t threads = std::max(p.n, lv < p.D ? cap[lv] * 64u : 0u);
        k_pts_descend<<<blocks_for(threads), 256, 0, c->stream>>>(p, t, s, ctl, lv);
    }
    VHX_HIP(c, hipGetLastError());

    // the counts of the touched cubes and bricks; the tree has only been read
    PtsCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.oob) return fail(c, VHX_E_INVALID_ARG, "vhx_set_voxels: a position outside the root cube");
    if (h.e.bad)
        return fail(c, VHX_E_STATE, "vhx_set_voxels: the tree under a point is not of canonical depth (a LOD-cut or "
                                    "streamed view)");
    if (!h.neff) return ws.end();  // insert or update mode, and no point has an entry
    const uint64_t nleaf = h.count[p.D], nb = h.count[p.D + 1];
    if (nleaf > MAX_LEAVES) return fail(c, VHX_E_CAPACITY, "vhx_set_voxels: more than 2^28 touched leaf cubes");
    if (nb >= 0x80000000ull) return fail(c, VHX_E_CAPACITY, "vhx_set_voxels: 2^31 touched bricks or more");
    if ((rc = vhx::ensure(c, ps.binfo, nb * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.bcnt, nb * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.bseg, nb * 8))) return rc;
    if ((rc = vhx::ensure(c, ps.bflag, nb * 4))) return rc;
    if ((rc = vhx::ensure(c, c->build.part, ((std::max(cap_max, nb) + SCAN_TILE - 1) / SCAN_TILE) * 8))) return rc;
    s.binfo = (u64 *)ps.binfo.ptr;
    s.bcnt = (u64 *)ps.bcnt.ptr;
    s.bseg = (u64 *)ps.bseg.ptr;
    s.bflag = (uint32_t *)ps.bflag.ptr;
    VHX_HIP(c, hipMemsetAsync(s.bcnt, 0, nb * 8, c->stream));
    k_pts_count<<<blocks_for(std::max(p.n, nleaf * 64u)), 256, 0, c->stream>>>(p, s, nleaf);
    if ((rc = scan_level<3>(c, s.bcnt, nb, false, s.bseg, &ctl->count[p.D + 2]))) return rc;
    k_pts_scatter<<<blocks_for(p.n), 256, 0, c->stream>>>(p, s);
    const unsigned brick_blocks = (unsigned)((nb + 3) / 4);
    const bool upd = p.mode == VHX_WRITE_UPDATE;
    const size_t upd_lds = 8u * std::min<size_t>((size_t)1 << (3u * p.lg_bd), CHUNK) * sizeof(uint32_t);
    if (upd)
        k_pts_brick<0, 1><<<brick_blocks, 256, upd_lds, c->stream>>>(p, t, s, tab, dtab, ctl, nb);
    else
        k_pts_brick<0, 0><<<brick_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl, nb);
    k_pts_leaf<<<blocks_for(nleaf), 256, 0, c->stream>>>(p, t, s, ctl, nleaf);
    for (uint32_t lv = p.D; lv-- > 0;)
        k_pts_reduce<<<blocks_for(h.count[lv]), 256, 0, c->stream>>>(p, t, s, ctl, lv, h.count[lv]);
    VHX_HIP(c, hipGetLastError());
    for (uint32_t lv = 0; lv <= p.D; ++lv)
        if ((rc = scan_level<2>(c, s.need + p.off[lv], h.count[lv], false, s.rank + p.off[lv], &ctl->e.b.level_total[lv])))
            return rc;
    if ((rc = scan_level<1>(c, s.nmask, nleaf, false, s.bfirst, &ctl->e.b.brick_total))) return rc;
    k_edit_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(tab, &ctl->e.b);
    k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->e.b);
    k_edit_pal_shift<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->e.b, d.color_count);
    if (with_data) {  // the new data values, ranked on their own after data_count
        k_edit_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(dtab, &ctl->e.d);
        k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(dtab, &ctl->e.d);
        k_edit_pal_shift<<<PAL_CAP / 256, 256, 0, c->stream>>>(dtab, &ctl->e.d, d.data_count);
    }
    VHX_HIP(c, hipGetLastError());

    // the last readback; the tree has only been read so far
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.e.b.overflow || h.e.b.ncolors > MAX_COLORS)
        return fail(c, VHX_E_CAPACITY, "vhx_set_voxels: more than 65535 colours");
    if (with_data && (h.e.d.overflow || h.e.d.ncolors > MAX_COLORS))
        return fail(c, VHX_E_CAPACITY, "vhx_set_voxels: more than 65535 data values");
    if ((uint64_t)d.brick_count + h.e.b.brick_total >= 0x80000000ull)
        return fail(c, VHX_E_CAPACITY, "vhx_set_voxels: 2^31 bricks or more");
    uint64_t nodes = d.node_count;
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        p.new_base[lv] = (uint32_t)nodes;
        nodes += h.e.b.level_total[lv];
    }
    if (nodes >= 0xFFFFFFFFull) return fail(c, VHX_E_CAPACITY, "vhx_set_voxels: 2^32 nodes or more");
    vhx_tree_desc nd = d;
    nd.node_count = (uint32_t)nodes;
    nd.brick_count = d.brick_count + (uint32_t)h.e.b.brick_total;
    nd.color_count = h.e.b.ncolors;
    if (with_data) nd.data_count = h.e.d.ncolors;
    if ((rc = vhx::grow_tree(c, &nd))) return rc;
    t = tree_of(c, d);  // the buffers may have moved; the counts stay the old ones

    if (upd)
        k_pts_brick<1, 1><<<brick_blocks, 256, upd_lds, c->stream>>>(p, t, s, tab, dtab, ctl, nb);
    else
        k_pts_brick<1, 0><<<brick_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl, nb);
    for (uint32_t lv = 0; lv <= p.D; ++lv)
        k_pts_nodes<<<blocks_for(h.count[lv] * 64u), 256, 0, c->stream>>>(p, t, s, lv, h.count[lv]);
    VHX_HIP(c, hipGetLastError());
    if (nd.color_count > d.color_count)
        VHX_HIP(c, hipMemcpyAsync((uint32_t *)c->tree->raw[VHX_BUF_COLOR_PALETTE].ptr + d.color_count, tab.pal,
                                  (uint64_t)(nd.color_count - d.color_count) * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nd.data_count > d.data_count)
        VHX_HIP(c, hipMemcpyAsync((uint32_t *)c->tree->raw[VHX_BUF_DATA_PALETTE].ptr + d.data_count, dtab.pal,
                                  (uint64_t)(nd.data_count - d.data_count) * 4, hipMemcpyDeviceToDevice, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    c->tree->desc = nd;
    c->tree->orphan_nodes += h.e.orphan_nodes;
    c->tree->orphan_bricks += h.e.orphan_bricks;
    return ws.end();  // the next trace of every context of the tree waits for this write
}

}  // namespace

extern "C" {

int vhx_set_voxels(vhx_ctx *c, const vhx_points_in *pts, int on_device) { return set_voxels(c, pts, on_device); }

}  // extern "C"
