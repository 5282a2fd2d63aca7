// vhx_write_dense: an axis-aligned box of the device tree replaced by a dense albedo grid, in place.
//
// The box touches a regular range of aligned cubes at every level (level lv: cubes of edge boxtree_size / 4^lv, the
// leaves' at level D are 4 * brick_dim wide), so the passes run over that lattice, numbered x fastest, then y, then z:
//
//   walk     k_edit_walk    the old node of every lattice cube (or none), by a descent from the root; raises the
//                           structure flag where the tree under the box is not of canonical depth
//   seed     k_edit_seed    the palette's colours into the build's colour table with their indices as first indices
//   leaves   k_edit_leaf<0> one workgroup per touched leaf cube, a wave per brick at a time: the grid part and the old
//                           occupancy of every brick the box meets give the brick's bitmap after the write; the leaf's
//                           mask of bricks, the mask of bricks that need a new slot, the orphaned bricks; the box's
//                           colours go into the table with first indices above the palette's
//   levels   k_edit_reduce  occupancy after the write, upwards: the old bits of the sectants outside the lattice, the
//                           lattice children's "not empty" inside it; "must exist and does not" per cube
//   scans    k_scan_*       ranks of the new nodes per level and of the new bricks (lattice order; bricks in (leaf cube,
//                           sectant) order): new nodes follow node_count level by level from the top, new bricks
//                           follow brick_count
//   palette  k_edit_pal_compact, k_pal_rank, k_edit_pal_shift   the new colours ranked by first index, after color_count
//   -- one readback of the counters; nothing of the tree has been written so far; then the buffers grow --
//   emit     k_edit_leaf<1> entries, voxels, bitmaps and child records of the touched leaves (before k_edit_nodes: it
//                           reads the old leaf types)
//            k_edit_nodes   types, occupancy, headers, entries and child records of the lattice nodes, per level
//
// vhx_write_dense_data runs the same passes with DATA = 1: a box voxel is an entry where it has a
// colour or a data value, the data values have a table of their own (build.dtable, seeded from data_palette, entries
// equal to 0 skipped) with the colours' compact / rank / shift triple, and the emission writes both halves.
//
// The emission writes the derived state of what it writes (headers, bitmaps of written bricks, child records of written
// entries) itself: a bitmap is the ballot the leaf pass already needs to decide whether the brick exists. Every global
// write is a plain store; the atomics are ORs, minima, table claims and counts, as in vhx_build.hip, so the image does
// not depend on scheduling. What vhx_points.hip uses as well (the counters, the view of the tree's buffers, k_edit_seed,
// k_edit_pal_compact, k_edit_pal_shift) is in edittab.hpp.
#include <algorithm>
#include <string>

#include "../../include/vhx.h"
#include "buildtab.hpp"
#include "ctx.hpp"
#include "edittab.hpp"
#include "treewalk.hpp"

namespace {

struct Lattice {
    uint32_t lo[3], n[3];  // first cube and cubes per axis
    uint64_t off;          // the level's first cell in the scratch arrays
};

struct EditP {
    uint32_t ox, oy, oz, gx, gy, gz, mode, fill;
    const uint32_t *grid;  // null: every voxel of the box is `fill`
    const uint32_t *dgrid;  // vhx_write_dense_data: the box's data plane; null: every voxel's data value is `dfill`
    uint32_t dfill;
    uint32_t lg_size, lg_bd, D;
    uint64_t total;  // cells of all levels
    Lattice lv[MAX_LEVELS];
    uint32_t new_base[MAX_LEVELS];  // emission: index of the level's first new node
};

struct Scratch {
    uint32_t *oldn;  // [total]  old node of the cube, NONE = none
    u64 *aft;        // [total]  occupancy after the write
    u64 *need;       // [total]  1 = the cube needs a new node
    u64 *rank;       // [total]  rank of that node among the level's new nodes
    u64 *nmask;      // [leaves] bricks that need a new slot
    u64 *first;      // [leaves] rank of the leaf's first new brick
};

__device__ inline void cell_coord(const Lattice &l, uint64_t cell, uint32_t &x, uint32_t &y, uint32_t &z) {
    x = l.lo[0] + (uint32_t)(cell % l.n[0]);
    y = l.lo[1] + (uint32_t)((cell / l.n[0]) % l.n[1]);
    z = l.lo[2] + (uint32_t)(cell / ((uint64_t)l.n[0] * l.n[1]));
}

// cell index of cube (x, y, z) in the level's lattice, or ~0 outside it (unsigned differences wrap past the extent)
__device__ inline uint64_t cell_index(const Lattice &l, uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t dx = x - l.lo[0], dy = y - l.lo[1], dz = z - l.lo[2];
    if (dx >= l.n[0] || dy >= l.n[1] || dz >= l.n[2]) return ~0ull;
    return ((uint64_t)dz * l.n[1] + dy) * l.n[0] + dx;
}

__global__ __launch_bounds__(256) void k_edit_walk(EditP p, TreeP t, Scratch s, EditCtl *ctl) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= p.total) return;
    uint32_t lv = 0;
    while (lv < p.D && gid >= p.lv[lv + 1].off) ++lv;
    uint32_t cx, cy, cz;
    cell_coord(p.lv[lv], gid - p.lv[lv].off, cx, cy, cz);
    uint32_t node = 0;
    bool bad = false;
    for (uint32_t i = 0; i < lv; ++i) {
        const uint32_t ty = t.type[node];
        if (ty != VHX_NODE_INTERNAL) {
            bad = !(i == 0 && ty == VHX_NODE_NOTHING);  // an empty tree's root; else a leaf above the lowest level
            node = NONE;
            break;
        }
        const uint32_t sh = 2u * (lv - i - 1u);
        const uint32_t sec = ((cx >> sh) & 3u) | (((cy >> sh) & 3u) << 2) | (((cz >> sh) & 3u) << 4);
        const uint32_t e = t.children[(uint64_t)node * 64u + sec];
        if (e == VHX_EMPTY || e >= t.node_count) {
            bad = e != VHX_EMPTY || ((t.ocbits[node] >> sec) & 1ull) != 0;  // occupied, the child not in this view
            node = NONE;
            break;
        }
        node = e;
    }
    if (node != NONE) {
        const uint32_t ty = t.type[node];
        const bool is_leaf = ty == VHX_NODE_LEAF || ty == VHX_NODE_UNIFORM_LEAF;
        if (lv < p.D ? is_leaf : ty == VHX_NODE_INTERNAL) bad = true;
    }
    s.oldn[gid] = node;
    if (bad) atomicOr(&ctl->bad, 1u);
}

// The touched leaves. EMIT = 0 analyses (reads the tree only), EMIT = 1 writes; both derive a brick's bitmap after the
// write the same way, so the second pass reproduces what the first one counted. Loop bounds are wave uniform: the
// ballots run with all 64 lanes.
// DATA = 1 (vhx_write_dense_data): a box voxel is an entry where it has a colour or a data value, its data values go
// into `dtab`, and the emission writes both halves.
// UPD = 1 (VHX_WRITE_UPDATE): a box voxel with an entry is covered, and its value is the old raw cell
// with the halves the entry has replaced (pix_overwrite_color / pix_overwrite_data); without DATA the data half stays.
template <int EMIT, int DATA, int UPD>
__global__ __launch_bounds__(256) void k_edit_leaf(EditP p, TreeP t, Scratch s, ColorTable tab, ColorTable dtab,
                                                   EditCtl *ctl) {
    __shared__ uint32_t s_ty, s_u, s_orph;
    __shared__ u64 s_aft, s_nm;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const Lattice &L = p.lv[p.D];
    const uint64_t nleaf = (uint64_t)L.n[0] * L.n[1] * L.n[2];
    const uint32_t bd = 1u << p.lg_bd, n3 = 1u << (3u * p.lg_bd), lsh = p.lg_bd + 2u;
    uint32_t last_c = 0, last_d = 0, last_v = VHX_EMPTY;
    uint32_t last_ci = 0xFFFFu, last_di = 0xFFFFu;  // UPD: the two looked-up indices; the spliced value is per cell
    for (uint64_t cell = blockIdx.x; cell < nleaf; cell += gridDim.x) {
        const uint32_t node = s.oldn[L.off + cell];
        const u64 aft = EMIT ? s.aft[L.off + cell] : 0ull;
        if (EMIT && aft == 0) continue;  // the whole block: k_edit_nodes clears a leaf that leaves
        if (tid == 0) {
            const uint32_t ty = node != NONE ? t.type[node] : VHX_NODE_NOTHING;
            s_ty = ty;
            s_u = ty == VHX_NODE_UNIFORM_LEAF ? t.children[(uint64_t)node * 64u] : VHX_EMPTY;
            s_aft = 0;
            s_nm = 0;
            s_orph = 0;
        }
        __syncthreads();  // the old type and uniform brick are read before anything of the leaf is written
        const uint32_t ty = s_ty, u = s_u;
        const bool leaf = ty == VHX_NODE_LEAF, uniform = ty == VHX_NODE_UNIFORM_LEAF;
        const bool uparted = uniform && u != VHX_EMPTY && (u & VHX_SOLID_BIT) == 0 && u < t.brick_count;
        uint32_t lx, ly, lz;
        cell_coord(L, cell, lx, ly, lz);
        const uint32_t LX = lx << lsh, LY = ly << lsh, LZ = lz << lsh;
        const uint32_t ni = EMIT ? (node != NONE ? node : p.new_base[p.D] + (uint32_t)s.rank[L.off + cell]) : 0u;
        const u64 nm = EMIT ? s.nmask[cell] : 0ull;
        const uint32_t fb = EMIT ? t.brick_count + (uint32_t)s.first[cell] : 0u;
        u64 w_aft = 0, w_nm = 0;
        uint32_t w_orph = 0;
        for (uint32_t sec = wave; sec < 64u; sec += 4u) {
            const u64 bit = 1ull << sec;
            const uint32_t bx = LX + ((sec & 3u) << p.lg_bd), by = LY + (((sec >> 2) & 3u) << p.lg_bd),
                           bz = LZ + ((sec >> 4) << p.lg_bd);
            const bool inter = bx < p.ox + p.gx && bx + bd > p.ox && by < p.oy + p.gy && by + bd > p.oy &&
                               bz < p.oz + p.gz && bz + bd > p.oz;
            uint32_t d = leaf ? t.children[(uint64_t)node * 64u + sec] : u;
            const bool dsolid = d != VHX_EMPTY && (d & VHX_SOLID_BIT) != 0;
            if (d != VHX_EMPTY && !dsolid && d >= t.brick_count) d = VHX_EMPTY;  // not a brick of this tree
            const bool own = leaf && d != VHX_EMPTY && !dsolid;
            if (!inter && !uparted) {  // the brick stays as it is; an expanded or new leaf still needs its entry
                const bool exists = d != VHX_EMPTY;
                if (!EMIT) {
                    if (exists) w_aft |= bit;
                } else if ((node == NONE || uniform) && lane == 0) {
                    const uint64_t at = (uint64_t)ni * 64u + sec;
                    t.children[at] = d;
                    if (t.rec) t.rec[at] = make_uint4(d, 0u, 0u, 0u);
                }
                continue;
            }
            const uint64_t at = (uint64_t)ni * 64u + sec;
            if (EMIT && ((aft >> sec) & 1ull) == 0) {  // the brick leaves, or never was
                if (lane == 0) {
                    t.children[at] = VHX_EMPTY;
                    if (t.rec) t.rec[at] = make_uint4(VHX_EMPTY, 0u, 0u, 0u);
                }
                continue;
            }
            uint32_t sraw = VHX_EMPTY;
            if (dsolid && (d & 0x7FFFFFFFu) < t.solid_count) sraw = t.solid[d & 0x7FFFFFFFu];
            const bool sne = !cell_empty(sraw, t.color, t.color_count, t.data, t.data_count);
            const uint32_t slot = own ? d : fb + (uint32_t)__popcll(nm & (bit - 1ull));
            u64 any = 0, word0 = 0;
            for (uint32_t c0 = 0; c0 < n3; c0 += 64u) {
                const uint32_t c = c0 + lane;
                const bool valid = c < n3;
                const uint32_t cx = c & (bd - 1u), cy = (c >> p.lg_bd) & (bd - 1u), cz = c >> (2u * p.lg_bd);
                const uint32_t vx = bx + cx, vy = by + cy, vz = bz + cz;
                const uint32_t rx = vx - p.ox, ry = vy - p.oy, rz = vz - p.oz;
                const bool inbox = valid && rx < p.gx && ry < p.gy && rz < p.gz;
                uint32_t g = 0, gd = 0;
                if (inbox) g = p.grid ? p.grid[((uint64_t)rz * p.gy + ry) * p.gx + rx] : p.fill;
                if (DATA && inbox) gd = p.dgrid ? p.dgrid[((uint64_t)rz * p.gy + ry) * p.gx + rx] : p.dfill;
                const bool col = (g >> 24) != 0;  // the voxel has a colour
                const bool vis = col || (DATA && gd != 0);  // the box's voxel is an entry
                const bool covered = inbox && ((!UPD && p.mode == VHX_WRITE_REPLACE) || vis);
                uint32_t raw = VHX_EMPTY;
                bool ne = false;
                if (own) {
                    const u64 word = t.occ[(uint64_t)d * t.occ_words + (c0 >> 6)];
                    ne = ((word >> (c & 63u)) & 1ull) != 0;
                } else if (dsolid) {
                    raw = sraw;
                    ne = sne;
                } else if (uparted && valid) {  // the uniform brick's cell over this voxel
                    const uint32_t ucell = ((vx - LX) >> 2) + ((((vy - LY) >> 2) + (((vz - LZ) >> 2) << p.lg_bd)) << p.lg_bd);
                    raw = t.voxels[((uint64_t)u << (3u * p.lg_bd)) + ucell];
                    ne = !cell_empty(raw, t.color, t.color_count, t.data, t.data_count);
                }
                const bool after = valid && (covered ? vis : ne);
                const u64 word = __ballot(after);
                any |= word;
                if (c0 == 0) word0 = word;
                if (!EMIT) {
                    {  // a voxel whose left neighbour in its row holds its colour has the larger index; a fill's
                       // one colour is recorded by the box's first voxel
                        const bool cand = covered && col && (p.grid || (rx | ry | rz) == 0u);
                        const uint32_t pg = __shfl_up(g, 1);
                        const bool pc = __shfl_up((int)cand, 1) != 0;
                        if (cand && !(lane > 0 && cx > 0 && pc && pg == g))
                            color_insert(tab, &ctl->b, g, NEW_BASE + ((u64)rx * p.gy + ry) * p.gz + rz);
                    }
                    if (DATA) {  // the data values, the same way
                        const bool cand = covered && gd != 0 && (p.dgrid || (rx | ry | rz) == 0u);
                        const uint32_t pg = __shfl_up(gd, 1);
                        const bool pc = __shfl_up((int)cand, 1) != 0;
                        if (cand && !(lane > 0 && cx > 0 && pc && pg == gd))
                            color_insert(dtab, &ctl->d, gd, NEW_BASE + ((u64)rx * p.gy + ry) * p.gz + rz);
                    }
                } else {
                    const uint64_t va = ((uint64_t)slot << (3u * p.lg_bd)) + c;
                    if (UPD && covered) {
                        // the old raw cell (VHX_EMPTY where there was none); an own brick's is read only where a half
                        // of it is kept
                        uint32_t v = own ? ((col && gd) ? 0u : t.voxels[va]) : raw;
                        if (col) {
                            if (g != last_c) {
                                last_c = g;
                                last_ci = color_lookup(tab, g);
                            }
                            v = (v & 0xFFFF0000u) | last_ci;
                        }
                        if (DATA && gd) {
                            if (gd != last_d) {
                                last_d = gd;
                                last_di = color_lookup(dtab, gd);
                            }
                            v = (v & 0x0000FFFFu) | (last_di << 16);
                        }
                        t.voxels[va] = v;
                    } else if (covered) {
                        uint32_t v = VHX_EMPTY;
                        if (vis) {
                            const uint32_t gc = col ? g : 0u;
                            if (gc != last_c || gd != last_d) {
                                last_c = gc;
                                last_d = gd;
                                // pix_visual, pix_informative, pix_complex: 0xFFFF for the half that is none
                                last_v = (gc ? color_lookup(tab, gc) : 0xFFFFu) |
                                         ((gd ? color_lookup(dtab, gd) : 0xFFFFu) << 16);
                            }
                            v = last_v;
                        }
                        t.voxels[va] = v;
                    } else if (valid && !own) {
                        t.voxels[va] = raw;
                    }
                    if (lane == 0) t.occ[(uint64_t)slot * t.occ_words + (c0 >> 6)] = word;
                }
            }
            if (!EMIT) {
                if (any) {
                    w_aft |= bit;
                    if (!own) w_nm |= bit;
                } else if (own) {
                    ++w_orph;
                }
            } else if (lane == 0) {
                t.children[at] = slot;
                if (t.rec) t.rec[at] = make_uint4(slot, (uint32_t)word0, (uint32_t)(word0 >> 32), 0u);
            }
        }
        if (!EMIT) {
            if (lane == 0) {
                if (w_aft) atomicOr(&s_aft, w_aft);
                if (w_nm) atomicOr(&s_nm, w_nm);
                if (w_orph) atomicAdd(&s_orph, w_orph);
            }
            __syncthreads();
            if (tid == 0) {
                const u64 a = s_aft;
                s.aft[L.off + cell] = a;
                s.nmask[cell] = s_nm;
                s.need[L.off + cell] = (a != 0 && node == NONE) ? 1ull : 0ull;
                const uint32_t orph = s_orph + (uparted ? 1u : 0u);  // an expanded leaf's uniform brick
                if (orph) atomicAdd(&ctl->orphan_bricks, orph);
                if (a == 0 && node != NONE && p.D != 0) atomicAdd(&ctl->orphan_nodes, 1u);
            }
        }
        __syncthreads();  // the shared words are rewritten for the next leaf
    }
}

// level lv < D, one thread per cube
__global__ __launch_bounds__(256) void k_edit_reduce(EditP p, TreeP t, Scratch s, uint32_t lv, EditCtl *ctl) {
    const Lattice &L = p.lv[lv], &C = p.lv[lv + 1];
    const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= (uint64_t)L.n[0] * L.n[1] * L.n[2]) return;
    uint32_t cx, cy, cz;
    cell_coord(L, cell, cx, cy, cz);
    const uint32_t node = s.oldn[L.off + cell];
    u64 m = node != NONE ? t.ocbits[node] : 0ull;
    for (uint32_t sec = 0; sec < 64u; ++sec) {
        const uint64_t ci = cell_index(C, 4u * cx + (sec & 3u), 4u * cy + ((sec >> 2) & 3u), 4u * cz + (sec >> 4));
        if (ci == ~0ull) continue;
        if (s.aft[C.off + ci])
            m |= 1ull << sec;
        else
            m &= ~(1ull << sec);
    }
    s.aft[L.off + cell] = m;
    s.need[L.off + cell] = (m != 0 && node == NONE) ? 1ull : 0ull;
    if (m == 0 && node != NONE && lv != 0) atomicAdd(&ctl->orphan_nodes, 1u);
}

// level lv, one thread per (cube, sectant): the node's type, occupancy and header, and for lv < D its entries inside
// the lattice (a new node's other entries are empty, an old node's stay). A node that lost everything becomes Nothing.
__global__ __launch_bounds__(256) void k_edit_nodes(EditP p, TreeP t, Scratch s, uint32_t lv) {
    const Lattice &L = p.lv[lv];
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t cell = gid >> 6;
    const uint32_t sec = (uint32_t)gid & 63u;
    if (cell >= (uint64_t)L.n[0] * L.n[1] * L.n[2]) return;
    const uint32_t node = s.oldn[L.off + cell];
    const u64 a = s.aft[L.off + cell];
    if (node == NONE && a == 0) return;
    const uint32_t ni = node != NONE ? node : p.new_base[lv] + (uint32_t)s.rank[L.off + cell];
    const uint64_t at = (uint64_t)ni * 64u + sec;
    const uint32_t ty = a == 0 ? VHX_NODE_NOTHING : lv < p.D ? VHX_NODE_INTERNAL : VHX_NODE_LEAF;
    if (sec == 0) {
        t.type[ni] = ty;
        t.ocbits[ni] = a;
        t.hdr[ni] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), ty, 0u);
    }
    uint32_t e = VHX_EMPTY;
    if (a != 0) {
        if (lv == p.D) return;  // k_edit_leaf wrote the entries
        uint32_t cx, cy, cz;
        cell_coord(L, cell, cx, cy, cz);
        const Lattice &C = p.lv[lv + 1];
        const uint64_t ci = cell_index(C, 4u * cx + (sec & 3u), 4u * cy + ((sec >> 2) & 3u), 4u * cz + (sec >> 4));
        if (ci == ~0ull) {
            if (node != NONE) return;  // an old node's entry outside the box
        } else if (s.aft[C.off + ci]) {
            const uint32_t cn = s.oldn[C.off + ci];
            e = cn != NONE ? cn : p.new_base[lv + 1] + (uint32_t)s.rank[C.off + ci];
        }
    }
    t.children[at] = e;
    if (t.rec) t.rec[at] = make_uint4(e, 0u, 0u, 0u);
}

// both dense writes: `with_data` is vhx_write_dense_data with a data plane or a data fill
int write_dense(vhx_ctx *c, const vhx_dense_in *box, const uint32_t *data, uint32_t fill_data, bool with_data,
                int on_device) {
    if (!c || !box) return fail(c, VHX_E_INVALID_ARG, "vhx_write_dense: null argument");
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_write_dense on a shared context: write through the owner");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_write_dense before vhx_upload_tree");
    if (c->tree->mips_on) return fail(c, VHX_E_STATE, "vhx_write_dense while node MIPs are set");
    const vhx_tree_desc d = c->tree->desc;
    const uint64_t S = d.boxtree_size;
    if (box->gx == 0 || box->gy == 0 || box->gz == 0 || (uint64_t)box->ox + box->gx > S ||
        (uint64_t)box->oy + box->gy > S || (uint64_t)box->oz + box->gz > S)
        return fail(c, VHX_E_INVALID_ARG, "vhx_write_dense: an extent of 0, or a box outside the root cube");
    if (box->mode != VHX_WRITE_REPLACE && box->mode != VHX_WRITE_INSERT && box->mode != VHX_WRITE_UPDATE)
        return fail(c, VHX_E_INVALID_ARG, "vhx_write_dense: unknown mode");
    EditP p{};
    p.ox = box->ox, p.oy = box->oy, p.oz = box->oz;
    p.gx = box->gx, p.gy = box->gy, p.gz = box->gz;
    p.mode = box->mode;
    p.fill = box->fill;
    p.dfill = fill_data;
    while ((1u << p.lg_size) < d.boxtree_size) ++p.lg_size;
    while ((1u << p.lg_bd) < d.brick_dim) ++p.lg_bd;
    if ((1u << p.lg_size) != d.boxtree_size || (1u << p.lg_bd) != d.brick_dim || p.lg_size < p.lg_bd + 2u ||
        ((p.lg_size - p.lg_bd) & 1u) || (p.lg_size - p.lg_bd) / 2u > MAX_LEVELS)
        return fail(c, VHX_E_STATE, "vhx_write_dense: the tree's size is not brick_dim * 4^k");
    p.D = (p.lg_size - p.lg_bd) / 2u - 1u;
    const uint32_t o[3] = {p.ox, p.oy, p.oz}, g[3] = {p.gx, p.gy, p.gz};
    uint64_t cells_max = 1;
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        const uint32_t lg = p.lg_size - 2u * lv;
        uint64_t n = 1;
        for (int a = 0; a < 3; ++a) {
            p.lv[lv].lo[a] = o[a] >> lg;
            p.lv[lv].n[a] = ((o[a] + g[a] - 1u) >> lg) - p.lv[lv].lo[a] + 1u;
            n *= p.lv[lv].n[a];
        }
        p.lv[lv].off = p.total;
        p.total += n;
        cells_max = std::max(cells_max, n);
    }
    const Lattice &LL = p.lv[p.D];
    const uint64_t nleaf = (uint64_t)LL.n[0] * LL.n[1] * LL.n[2];
    if (nleaf > MAX_LEAVES) return fail(c, VHX_E_CAPACITY, "vhx_write_dense: more than 2^28 touched leaf cubes");

    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    vhx::WriteScope ws(c);  // frames in flight on the tree's other contexts finish reading it first
    int rc = ws.rc;
    if (rc) return rc;
    if ((rc = vhx::refresh_child_rec(c))) return rc;
    if ((rc = vhx::ensure(c, c->edit.oldn, p.total * 4))) return rc;
    if ((rc = vhx::ensure(c, c->edit.aft, p.total * 8))) return rc;
    if ((rc = vhx::ensure(c, c->edit.need, p.total * 8))) return rc;
    if ((rc = vhx::ensure(c, c->edit.rank, p.total * 8))) return rc;
    if ((rc = vhx::ensure(c, c->edit.nmask, nleaf * 8))) return rc;
    if ((rc = vhx::ensure(c, c->edit.first, nleaf * 8))) return rc;
    if ((rc = vhx::ensure(c, c->edit.ctl, sizeof(EditCtl)))) return rc;
    if ((rc = vhx::ensure(c, c->build.part, ((cells_max + SCAN_TILE - 1) / SCAN_TILE) * 8))) return rc;
    if ((rc = vhx::ensure(c, c->build.table, TAB_BYTES))) return rc;
    if (with_data && (rc = vhx::ensure(c, c->build.dtable, TAB_BYTES))) return rc;
    p.grid = box->albedo;
    p.dgrid = data;
    if ((box->albedo || data) && !on_device) {  // host planes: the data plane follows the albedo plane
        const uint64_t bytes = (uint64_t)p.gx * p.gy * p.gz * 4;
        if ((rc = vhx::ensure(c, c->build.grid, bytes * ((box->albedo ? 1u : 0u) + (data ? 1u : 0u))))) return rc;
        char *at = (char *)c->build.grid.ptr;
        if (box->albedo) {
            VHX_HIP(c, hipMemcpyAsync(at, box->albedo, bytes, hipMemcpyHostToDevice, c->stream));
            p.grid = (const uint32_t *)at;
            at += bytes;
        }
        if (data) {
            VHX_HIP(c, hipMemcpyAsync(at, data, bytes, hipMemcpyHostToDevice, c->stream));
            p.dgrid = (const uint32_t *)at;
        }
    }
    Scratch s{(uint32_t *)c->edit.oldn.ptr, (u64 *)c->edit.aft.ptr,   (u64 *)c->edit.need.ptr,
              (u64 *)c->edit.rank.ptr,      (u64 *)c->edit.nmask.ptr, (u64 *)c->edit.first.ptr};
    EditCtl *ctl = (EditCtl *)c->edit.ctl.ptr;
    const ColorTable tab = table_of(c->build.table.ptr);
    const ColorTable dtab = with_data ? table_of(c->build.dtable.ptr) : ColorTable{};
    TreeP t = tree_of(c, d);
    // reset: counters, table keys free, first indices at maximum (every scratch word is written before it is read)
    VHX_HIP(c, hipMemsetAsync(ctl, 0, sizeof(EditCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(tab.keys, 0, TAB_KEYS_BYTES, c->stream));
    VHX_HIP(c, hipMemsetAsync(tab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    if (with_data) {
        VHX_HIP(c, hipMemsetAsync(dtab.keys, 0, TAB_KEYS_BYTES, c->stream));
        VHX_HIP(c, hipMemsetAsync(dtab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    }

    k_edit_walk<<<blocks_for(p.total), 256, 0, c->stream>>>(p, t, s, ctl);
    k_edit_seed<0><<<blocks_for((uint64_t)d.color_count + 1), 256, 0, c->stream>>>(tab, t.color, d.color_count, ctl);
    if (with_data)
        k_edit_seed<1><<<blocks_for((uint64_t)d.data_count + 1), 256, 0, c->stream>>>(dtab, t.data, d.data_count, ctl);
    const unsigned leaf_blocks = (unsigned)std::min<uint64_t>(nleaf, (uint64_t)c->cus * 32);
    const bool upd = p.mode == VHX_WRITE_UPDATE;
    if (upd && with_data)
        k_edit_leaf<0, 1, 1><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    else if (upd)
        k_edit_leaf<0, 0, 1><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    else if (with_data)
        k_edit_leaf<0, 1, 0><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    else
        k_edit_leaf<0, 0, 0><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    for (uint32_t lv = p.D; lv-- > 0;) {
        const Lattice &L = p.lv[lv];
        k_edit_reduce<<<blocks_for((uint64_t)L.n[0] * L.n[1] * L.n[2]), 256, 0, c->stream>>>(p, t, s, lv, ctl);
    }
    VHX_HIP(c, hipGetLastError());
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        const Lattice &L = p.lv[lv];
        if ((rc = scan_level<2>(c, s.need + L.off, (uint64_t)L.n[0] * L.n[1] * L.n[2], false, s.rank + L.off,
                                &ctl->b.level_total[lv])))
            return rc;
    }
    if ((rc = scan_level<1>(c, s.nmask, nleaf, false, s.first, &ctl->b.brick_total))) return rc;
    k_edit_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(tab, &ctl->b);
    k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->b);
    k_edit_pal_shift<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, &ctl->b, d.color_count);
    if (with_data) {  // the new data values, ranked on their own after data_count
        k_edit_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(dtab, &ctl->d);
        k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(dtab, &ctl->d);
        k_edit_pal_shift<<<PAL_CAP / 256, 256, 0, c->stream>>>(dtab, &ctl->d, d.data_count);
    }
    VHX_HIP(c, hipGetLastError());

    // the one readback; the tree has only been read so far
    EditCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.bad)
        return fail(c, VHX_E_STATE, "vhx_write_dense: the tree under the box is not of canonical depth (a LOD-cut or "
                                    "streamed view)");
    if (h.b.overflow || h.b.ncolors > MAX_COLORS)
        return fail(c, VHX_E_CAPACITY, "vhx_write_dense: more than 65535 colours");
    if (with_data && (h.d.overflow || h.d.ncolors > MAX_COLORS))
        return fail(c, VHX_E_CAPACITY, "vhx_write_dense_data: more than 65535 data values");
    if ((uint64_t)d.brick_count + h.b.brick_total >= 0x80000000ull)
        return fail(c, VHX_E_CAPACITY, "vhx_write_dense: 2^31 bricks or more");
    uint64_t nodes = d.node_count;
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        p.new_base[lv] = (uint32_t)nodes;
        nodes += h.b.level_total[lv];
    }
    if (nodes >= 0xFFFFFFFFull) return fail(c, VHX_E_CAPACITY, "vhx_write_dense: 2^32 nodes or more");
    vhx_tree_desc nd = d;
    nd.node_count = (uint32_t)nodes;
    nd.brick_count = d.brick_count + (uint32_t)h.b.brick_total;
    nd.color_count = h.b.ncolors;
    if (with_data) nd.data_count = h.d.ncolors;
    if ((rc = vhx::grow_tree(c, &nd))) return rc;
    t = tree_of(c, d);  // the buffers may have moved; the counts stay the old ones

    if (upd && with_data)
        k_edit_leaf<1, 1, 1><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    else if (upd)
        k_edit_leaf<1, 0, 1><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    else if (with_data)
        k_edit_leaf<1, 1, 0><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    else
        k_edit_leaf<1, 0, 0><<<leaf_blocks, 256, 0, c->stream>>>(p, t, s, tab, dtab, ctl);
    for (uint32_t lv = 0; lv <= p.D; ++lv) {
        const Lattice &L = p.lv[lv];
        k_edit_nodes<<<blocks_for((uint64_t)L.n[0] * L.n[1] * L.n[2] * 64), 256, 0, c->stream>>>(p, t, s, lv);
    }
    VHX_HIP(c, hipGetLastError());
    if (nd.color_count > d.color_count)
        VHX_HIP(c, hipMemcpyAsync((uint32_t *)c->tree->raw[VHX_BUF_COLOR_PALETTE].ptr + d.color_count, tab.pal,
                                  (uint64_t)(nd.color_count - d.color_count) * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nd.data_count > d.data_count)
        VHX_HIP(c, hipMemcpyAsync((uint32_t *)c->tree->raw[VHX_BUF_DATA_PALETTE].ptr + d.data_count, dtab.pal,
                                  (uint64_t)(nd.data_count - d.data_count) * 4, hipMemcpyDeviceToDevice, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    c->tree->desc = nd;
    c->tree->orphan_nodes += h.orphan_nodes;
    c->tree->orphan_bricks += h.orphan_bricks;
    return ws.end();  // the next trace of every context of the tree waits for this write
}

}  // namespace

extern "C" {

int vhx_write_dense(vhx_ctx *c, const vhx_dense_in *box, int on_device) {
    return write_dense(c, box, nullptr, 0u, false, on_device);
}

int vhx_write_dense_data(vhx_ctx *c, const vhx_dense_in *box, const uint32_t *data, uint32_t fill_data, int on_device) {
    return write_dense(c, box, data, fill_data, data != nullptr || fill_data != 0u, on_device);
}

}  // extern "C"
