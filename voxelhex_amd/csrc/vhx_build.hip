// vhx_build_tree_dense: the canonical flattened tree of a dense voxel grid, built on the GPU into the context's tree
// buffers (the image vhx_dense_build of flatten.cpp writes on the host, bit for bit), and the read-back of a device tree
// (vhx_tree_counts, vhx_read_range).
//
// The image is a pure function of the grid (flatten.cpp, top): leaves are the nodes of edge 4*brick_dim, a node exists
// where a voxel lies below it, nodes are numbered breadth-first level by level in path-code order, bricks in (leaf,
// sectant) order, colours by their first appearance in the insert loop (x outer, y, z inner). With
// boxtree_size = brick_dim * 4^(D+1) the tree has levels 0..D and 64^lv possible nodes at level lv, addressed by their
// path code (6 bits per level, the root's sectant first).
//
//   pass A   k_dense_scan      reads the grid once in memory order: ORs every non-empty brick's bit into its leaf's
//                              mask (occ level D) and records every colour's smallest insert-order index
//                              (x*gy + y)*gz + z in an open-addressing table; both deduplicated inside the wave first
//   levels   k_reduce_level    occ[lv][p] = which of p's 64 children have a non-zero word (one wave per parent, ballot)
//   scans    k_scan_*          per level: exclusive scan of "node present" = the node's rank inside its level; for the
//                              leaves also of popcount(mask) = the leaf's first brick index
//   palette  k_pal_*           the table's entries compacted and ranked by first index: the palette, and each table
//                              entry's palette index
//   -- one readback of the counters; nothing of the context's tree has been touched so far --
//   fill     k_emit_nodes      node types, occupancy and children, level by level, into the tree's raw buffers
//            k_emit_bricks     the cells of every present brick gathered from the grid and translated through the table
//
// Every atomic is an OR, a minimum, a constant store, the claim of a table slot or the count of such events (colours
// claimed, entries compacted, solid values: only the total is used), and every order that reaches a buffer comes from a
// scan or from the first indices, so the buffers do not depend on scheduling. Grid offsets are
// 64-bit; nothing outside [0,gx) x [0,gy) x [0,gz) is read.
//
// vhx_build_tree_dense_data builds from a grid with a data plane beside its albedo plane (the image of
// vhx_dense_build_data): a voxel is an entry where it has a colour (alpha byte not 0) or a data value (not 0), its cell
// is colour index | data index << 16 with 0xFFFF for the half that is none, and the data values get a table, a
// compaction and a ranking of their own, exactly as the colours (counters: a second BuildCtl behind the first). The
// passes are the same ones, instantiated with DATA = 1; the colour-only instantiations are unchanged.
//
// vhx_build_tree_dense_simplified writes the image BoxTree::simplify(ROOT, recursive) leaves of that tree
// (vhx_dense_build_simplified of flatten.cpp, bit for bit). Nodes, their numbering, occupancy and the palette stay;
// only the leaves change. A brick all of whose cells hold one colour is Solid(palette index | 0xFFFF0000); a leaf whose
// 64 bricks are the same Solid brick is a UniformLeaf with that descriptor as entry 0; otherwise, with brick_dim > 1, a
// leaf whose aligned 4x4x4 voxel blocks are all homogeneous (one colour, or empty) is a UniformLeaf with one Parted brick
// holding the blocks' values; every other leaf keeps per-sectant entries: empty, Solid, or a brick index. Only Parted
// bricks are numbered, and solid_values lists the distinct Solid values by their first (leaf, sectant). The plain passes
// run unchanged up to the palette; then, in place of the brick scan:
//   classify k_classify        one workgroup per present leaf reads its voxels once more: a lane ORs a brick's "not solid"
//                              bit where a cell differs from the brick's corner cell (or is empty) and a "not
//                              block-uniform" flag where a voxel differs from its block's corner voxel; OR inside the
//                              wave, then in LDS. The leaf's class, its mask of Parted bricks and their count follow, and
//                              every Solid entry's colour takes the minimum of its key leaf_code * 64 + sectant
//   scan     k_scan_*          MODE 2: the leaf's first brick index from the Parted counts
//   rank     k_solid_rank      the keys ranked as k_pal_rank ranks first indices: solid_values and each colour's index
//   fill     k_emit_leaves     leaf types and entries by class; k_emit_bricks over the Parted masks;
//            k_emit_uniform    the one brick of a block-uniform leaf, sampled at the block corners
#include <algorithm>
#include <string>

#include "../../include/vhx_boxtree.h"
#include "buildtab.hpp"
#include "ctx.hpp"

namespace {

// vhx_ctx::build.simp (simplified build)
struct SimpTable {
    u64 *pmask;       // [nleaf]   the leaf's Parted bricks (0 for a UniformLeaf)
    u64 *linfo;       // [nleaf]   bits 0..6 bricks the leaf contributes, bits 8..9 its class (LEAF_*)
    u64 *skey;        // [PAL_CAP] by palette index: smallest leaf_code * 64 + sectant of a Solid entry of the colour
    uint32_t *srank;  // [PAL_CAP] by palette index: the colour's index in solid_values
    uint32_t *svals;  // [PAL_CAP] solid_values
};
constexpr uint64_t SKEY_BYTES = (uint64_t)PAL_CAP * 8;
inline uint64_t simp_bytes(uint64_t nleaf) { return nleaf * 16 + SKEY_BYTES + 2ull * PAL_CAP * 4; }
SimpTable simp_of(void *base, uint64_t nleaf) {
    SimpTable sp;
    uint8_t *p = (uint8_t *)base;
    sp.pmask = (u64 *)p;
    sp.linfo = sp.pmask + nleaf;
    sp.skey = sp.linfo + nleaf;
    sp.srank = (uint32_t *)(sp.skey + PAL_CAP);
    sp.svals = sp.srank + PAL_CAP;
    return sp;
}
constexpr uint32_t LEAF_PLAIN = 0, LEAF_UNIFORM_SOLID = 1, LEAF_UNIFORM_PARTED = 2;

struct GridP {
    const uint32_t *a;
    uint32_t gx, gy, gz;
    uint32_t bsh;  // log2(brick_dim)
    uint32_t D;    // leaf level
    const uint32_t *d;  // the data plane (vhx_build_tree_dense_data), indexed as a; null without one
};

// path code of the leaf with coordinates (lx, ly, lz): digit i (from the top) = the sectant taken at depth i
__device__ inline uint32_t leaf_code(uint32_t lx, uint32_t ly, uint32_t lz, uint32_t D) {
    uint32_t code = 0;
    for (uint32_t i = 0; i < D; ++i)
        code |= (((lx >> (2 * i)) & 3u) | (((ly >> (2 * i)) & 3u) << 2) | (((lz >> (2 * i)) & 3u) << 4)) << (6 * i);
    return code;
}

// Pass A, the values of one plane (colours, or data values) in a thread's row j: a voxel is skipped when a voxel of its
// value further left in its row is in this wave: that one's insert-order index is smaller. First the left neighbour and
// the thread's own voxels; then, per value, the lowest lane of a row group records it for the group (x grows with the
// lane there). Called by all 64 lanes.
template <int VEC>
__device__ __forceinline__ void scan_record(const uint32_t (&row)[VEC], bool row_start, uint32_t lane, uint32_t sub,
                                            const GridP &g, uint32_t x0, uint32_t y, uint32_t z, ColorTable t,
                                            BuildCtl *ctl) {
    uint32_t left = __shfl_up(row[VEC - 1], 1);
    if (row_start) left = 0;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const uint32_t c = row[i];
        bool cand = c != 0 && c != left;
#pragma unroll
        for (int e = 0; e + 1 < i; ++e) cand = cand && row[e] != c;
        left = c;
        u64 pending = __ballot(cand);
        while (pending) {  // the same in every lane
            const uint32_t leader = (uint32_t)__ffsll((long long)pending) - 1u;
            const uint32_t lc = __shfl(c, leader), lsub = __shfl(sub, leader);
            const bool mine = cand && c == lc && sub == lsub;
            if (lane == leader) color_insert(t, ctl, c, ((u64)(x0 + i) * g.gy + y) * g.gz + z);
            pending &= ~__ballot(mine);
        }
    }
}

// Pass A. A block covers `tpr` = 2^xsh vector columns of 256 / tpr row groups; a thread reads VEC voxels consecutive in
// x (VEC = 4: one 16-byte load; gx is then a multiple of 4 and the grid 16-byte aligned) of SCAN_ROWS = 4 rows
// consecutive in y, starting at a multiple of 4: a leaf's edge is a multiple of 4, so all of a thread's voxels share a
// leaf. The loops are the same for every thread of a block, so the wave operations below always run with all 64 lanes.
// DATA = 1 reads the data plane beside the albedo plane (VEC = 4: both 16-byte aligned): a voxel with a data value sets
// its brick's bit whatever its colour, and the data values go into their own table `dt` with the counters of ctl[1].
template <int VEC, int DATA>
__global__ __launch_bounds__(256) void k_dense_scan(GridP g, uint32_t xsh, u64 *leaf_mask, ColorTable t, ColorTable dt,
                                                    BuildCtl *ctl) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tpr = 1u << xsh, rpb = 256u >> xsh;
    const uint32_t gxv = (g.gx + VEC - 1) / VEC;
    const uint32_t xv = blockIdx.x * tpr + (tid & (tpr - 1u));
    const uint32_t x0 = xv * VEC;
    const uint32_t sub = tid >> xsh;  // the thread's row group inside the block
    const uint32_t ytiles = (g.gy + rpb * SCAN_ROWS - 1) / (rpb * SCAN_ROWS);
    const uint32_t lsh = g.bsh + 2;
    const bool row_start = lane == 0 || (tid & (tpr - 1u)) == 0;  // the previous lane is not this thread's left neighbour
    for (uint32_t z = blockIdx.z; z < g.gz; z += gridDim.z)
        for (uint32_t yt = blockIdx.y; yt < ytiles; yt += gridDim.y) {
            const uint32_t yb = (yt * rpb + sub) * SCAN_ROWS;
            uint32_t v[SCAN_ROWS][VEC];
            uint32_t w[DATA ? SCAN_ROWS : 1][VEC];  // the data values
#pragma unroll
            for (uint32_t j = 0; j < SCAN_ROWS; ++j) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) v[j][i] = 0;
                if constexpr (DATA != 0) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) w[j][i] = 0;
                }
                if (xv < gxv && yb + j < g.gy) {
                    const uint64_t at = ((uint64_t)z * g.gy + (yb + j)) * g.gx + (uint64_t)xv * VEC;
                    if constexpr (VEC == 4) {
                        const uint4 q = *reinterpret_cast<const uint4 *>(g.a + at);
                        v[j][0] = q.x;
                        v[j][1] = q.y;
                        v[j][2] = q.z;
                        v[j][3] = q.w;
                    } else {
                        v[j][0] = g.a[at];
                    }
                    if constexpr (DATA != 0) {
                        if constexpr (VEC == 4) {
                            const uint4 q = *reinterpret_cast<const uint4 *>(g.d + at);
                            w[j][0] = q.x;
                            w[j][1] = q.y;
                            w[j][2] = q.z;
                            w[j][3] = q.w;
                        } else {
                            w[j][0] = g.d[at];
                        }
                    }
                }
            }
            u64 m = 0;
#pragma unroll
            for (uint32_t j = 0; j < SCAN_ROWS; ++j) {
                const uint32_t y = yb + j;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    if ((v[j][i] >> 24) == 0) v[j][i] = 0;  // alpha 0: no voxel
                    bool entry = v[j][i] != 0;
                    if constexpr (DATA != 0) entry = entry || w[j][i] != 0;  // a data-only voxel is an entry too
                    if (entry) {
                        const uint32_t s = (((x0 + i) >> g.bsh) & 3u) | (((y >> g.bsh) & 3u) << 2) | (((z >> g.bsh) & 3u) << 4);
                        m |= 1ull << s;
                    }
                }
                scan_record<VEC>(v[j], row_start, lane, sub, g, x0, y, z, t, ctl);
                if constexpr (DATA != 0) scan_record<VEC>(w[j], row_start, lane, sub, g, x0, y, z, dt, ctl + 1);
            }
            // brick bits: OR over each run of lanes in the same leaf, one atomic per run, and none where the mask already
            // holds the bits (a stale read only costs the atomic)
            const uint32_t key = m ? leaf_code(x0 >> lsh, yb >> lsh, z >> lsh, g.D) : 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t k = 1; k < 64; k <<= 1) {
                const uint32_t ok = __shfl_down(key, k);
                const u64 om = __shfl_down(m, k);
                if (lane + k < 64 && ok == key) m |= om;
            }
            const uint32_t pk = __shfl_up(key, 1);
            if (m && (lane == 0 || pk != key) && (leaf_mask[key] & m) != m) atomicOr(&leaf_mask[key], m);
        }
}

// occ[lv][p]: bit s = child s of p (occ[lv + 1][64 p + s]) is not empty. One wave per parent.
__global__ __launch_bounds__(256) void k_reduce_level(const u64 *child, u64 *parent, uint64_t nparent) {
    const uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (p >= nparent) return;  // the whole wave
    const u64 b = __ballot(child[p * 64 + lane] != 0);
    if (lane == 0) parent[p] = b;
}

// ---- palette: the table's entries compacted for k_pal_rank
__global__ __launch_bounds__(256) void k_pal_compact(ColorTable t, BuildCtl *ctl) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= TAB_SLOTS) return;
    const uint32_t k = t.keys[h];
    if (k == 0) return;
    const uint32_t pos = atomicAdd(&ctl->ncompact, 1u);  // any order: the ranks below come from the first indices
    if (pos >= PAL_CAP) return;
    t.ckey[pos] = k;
    t.cidx[pos] = t.vals[h];
    t.cslot[pos] = h;
}

// ---- emission into the tree's raw buffers
// One thread per (possible node c of level lv, sectant s). Children: the child's breadth-first index (lv < D) or the
// brick index of the leaf's sectant (lv == D).
__global__ __launch_bounds__(256) void k_emit_nodes(uint32_t lv, uint32_t D, uint64_t n, const u64 *occ, const u64 *rank,
                                                    const u64 *rank_child, const u64 *first, uint32_t base,
                                                    uint32_t base_child, uint32_t *node_type, u64 *node_ocbits,
                                                    uint32_t *node_children) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t c = gid >> 6;
    const uint32_t s = (uint32_t)gid & 63u;
    if (c >= n) return;
    const u64 w = occ[c];
    if (w == 0 && lv != 0) return;  // no such node
    const uint64_t ni = (uint64_t)base + rank[c];
    if (s == 0) {
        node_type[ni] = w ? (lv < D ? VHX_NODE_INTERNAL : VHX_NODE_LEAF) : VHX_NODE_NOTHING;
        node_ocbits[ni] = w;
    }
    uint32_t child = VHX_EMPTY;
    if ((w >> s) & 1ull)
        child = lv < D ? base_child + (uint32_t)rank_child[c * 64 + s]
                       : (uint32_t)(first[c] + (u64)__popcll(w & ((1ull << s) - 1ull)));
    node_children[ni * 64 + s] = child;
}

// One block per leaf at a time: the cells of its bricks are one contiguous run of the voxel buffer, written in order.
// DATA = 1 gathers the data plane as well: a cell is colour index | data index << 16, 0xFFFF for a half that is none.
template <int DATA>
__global__ __launch_bounds__(256) void k_emit_bricks(GridP g, const u64 *leaf_mask, const u64 *first, uint64_t nleaf,
                                                     ColorTable t, ColorTable dt, uint32_t *voxels) {
    __shared__ uint8_t sect[64];
    const uint32_t tid = threadIdx.x;
    const uint32_t bd = 1u << g.bsh, n3sh = 3 * g.bsh, lsh = g.bsh + 2;
    uint32_t last_c = 0, last_d = 0, last_v = VHX_EMPTY;
    for (uint64_t code = blockIdx.x; code < nleaf; code += gridDim.x) {
        const u64 m = leaf_mask[code];
        if (m == 0) continue;  // the whole block
        if (tid < 64 && ((m >> tid) & 1ull)) sect[__popcll(m & ((1ull << tid) - 1ull))] = (uint8_t)tid;
        __syncthreads();
        uint32_t lx = 0, ly = 0, lz = 0;
        for (uint32_t i = 0; i < g.D; ++i) {
            const uint32_t d = (uint32_t)(code >> (6 * i)) & 63u;
            lx |= (d & 3u) << (2 * i);
            ly |= ((d >> 2) & 3u) << (2 * i);
            lz |= (d >> 4) << (2 * i);
        }
        const uint32_t total = (uint32_t)__popcll(m) << n3sh;
        uint32_t *dst = voxels + (first[code] << n3sh);
        for (uint32_t j = tid; j < total; j += 256) {
            const uint32_t s = sect[j >> n3sh], i = j & ((1u << n3sh) - 1u);
            const uint32_t x = (lx << lsh) + ((s & 3u) << g.bsh) + (i & (bd - 1u));
            const uint32_t y = (ly << lsh) + (((s >> 2) & 3u) << g.bsh) + ((i >> g.bsh) & (bd - 1u));
            const uint32_t z = (lz << lsh) + ((s >> 4) << g.bsh) + (i >> (2 * g.bsh));
            uint32_t c = 0, d = 0;
            if (x < g.gx && y < g.gy && z < g.gz) {
                const uint64_t at = ((uint64_t)z * g.gy + y) * g.gx + x;
                c = g.a[at];
                if constexpr (DATA != 0) d = g.d[at];
            }
            if ((c >> 24) == 0) c = 0;  // alpha 0: no colour
            uint32_t v = VHX_EMPTY;
            if (c | d) {
                if (c != last_c || d != last_d) {
                    last_c = c;
                    last_d = d;
                    // pix_visual, pix_informative, pix_complex: 0xFFFF for the half that is none
                    last_v = (c ? color_lookup(t, c) : 0xFFFFu) | ((d ? color_lookup(dt, d) : 0xFFFFu) << 16);
                }
                v = last_v;
            }
            dst[j] = v;
        }
        __syncthreads();  // sect is rewritten for the next leaf
    }
}

// ---- the simplified image
// voxel (x, y, z) of the tree: 0 outside the grid and for alpha 0
__device__ inline uint32_t grid_at(const GridP &g, uint32_t x, uint32_t y, uint32_t z) {
    if (x >= g.gx || y >= g.gy || z >= g.gz) return 0;
    const uint32_t c = g.a[((uint64_t)z * g.gy + y) * g.gx + x];
    return (c >> 24) ? c : 0u;
}

// leaf coordinates of a path code
__device__ inline void leaf_coord(uint64_t code, uint32_t D, uint32_t &lx, uint32_t &ly, uint32_t &lz) {
    lx = ly = lz = 0;
    for (uint32_t i = 0; i < D; ++i) {
        const uint32_t d = (uint32_t)(code >> (6 * i)) & 63u;
        lx |= (d & 3u) << (2 * i);
        ly |= ((d >> 2) & 3u) << (2 * i);
        lz |= (d >> 4) << (2 * i);
    }
}

// One block per present leaf at a time. Both tests compare a voxel with a fixed corner, so a lane only ever ORs: bit s
// of `ns` where a cell of brick s differs from the brick's corner cell or is empty (the brick is not Solid), `nb` where
// a voxel differs from the corner of its aligned 4x4x4 block. The loop bounds are the same for every thread of a block,
// so the wave operations run with all 64 lanes.
__global__ __launch_bounds__(256) void k_classify(GridP g, const u64 *leaf_mask, uint64_t nleaf, ColorTable t,
                                                  SimpTable sp) {
    __shared__ u64 s_ns;
    __shared__ uint32_t s_nb;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t lsh = g.bsh + 2, L = 1u << lsh, nvox = 1u << (3 * lsh);
    for (uint64_t code = blockIdx.x; code < nleaf; code += gridDim.x) {
        const u64 m = leaf_mask[code];
        if (m == 0) continue;  // the whole block
        if (tid == 0) {
            s_ns = 0;
            s_nb = 0;
        }
        __syncthreads();
        uint32_t lx, ly, lz;
        leaf_coord(code, g.D, lx, ly, lz);
        const uint32_t ox = lx << lsh, oy = ly << lsh, oz = lz << lsh;
        u64 ns = 0;
        bool nb = false;
        for (uint32_t j = tid; j < nvox; j += 256) {
            const uint32_t x = j & (L - 1u), y = (j >> lsh) & (L - 1u), z = j >> (2 * lsh);
            const uint32_t c = grid_at(g, ox + x, oy + y, oz + z);
            const uint32_t bx = x >> g.bsh, by = y >> g.bsh, bz = z >> g.bsh;
            const uint32_t cb = grid_at(g, ox + (bx << g.bsh), oy + (by << g.bsh), oz + (bz << g.bsh));
            const uint32_t ck = grid_at(g, ox + (x & ~3u), oy + (y & ~3u), oz + (z & ~3u));
            if (c == 0 || c != cb) ns |= 1ull << (bx | (by << 2) | (bz << 4));
            nb = nb || c != ck;
        }
#pragma unroll
        for (uint32_t k = 1; k < 64; k <<= 1) ns |= __shfl_xor(ns, k);
        const bool wave_nb = __ballot(nb) != 0;
        if (lane == 0) {
            if (ns) atomicOr(&s_ns, ns);
            if (wave_nb) atomicOr(&s_nb, 1u);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: a lane per sectant
            const u64 solid = m & ~s_ns;
            const uint32_t cs = grid_at(g, ox + ((tid & 3u) << g.bsh), oy + (((tid >> 2) & 3u) << g.bsh),
                                        oz + ((tid >> 4) << g.bsh));  // the colour of a Solid brick
            const bool one_value = __ballot(cs == __shfl(cs, 0)) == ~0ull;
            uint32_t cls = LEAF_PLAIN;
            if (solid == ~0ull && one_value)
                cls = LEAF_UNIFORM_SOLID;
            else if (g.bsh > 0 && s_nb == 0)
                cls = LEAF_UNIFORM_PARTED;
            const u64 pm = cls == LEAF_PLAIN ? m & ~solid : 0ull;
            if (tid == 0) {
                sp.pmask[code] = pm;
                sp.linfo[code] = (u64)(cls == LEAF_UNIFORM_PARTED ? 1u : (uint32_t)__popcll(pm)) | ((u64)cls << 8);
            }
            // the Solid entries the leaf will hold: the lowest sectant of a colour records it for the leaf
            const bool cand = ((solid >> tid) & 1ull) && (cls == LEAF_PLAIN || (cls == LEAF_UNIFORM_SOLID && tid == 0));
            const uint32_t idx = cand ? color_lookup(t, cs) : 0xFFFFu;
            u64 pending = __ballot(cand);
            while (pending) {  // the same in every lane
                const uint32_t leader = (uint32_t)__ffsll((long long)pending) - 1u;
                const uint32_t li = __shfl(idx, leader);
                if (lane == leader) {
                    const u64 key = code * 64ull + tid;
                    if (sp.skey[idx] > key) atomicMin(&sp.skey[idx], key);  // as color_insert
                }
                pending &= ~__ballot(cand && idx == li);
            }
        }
        __syncthreads();  // s_ns and s_nb are reset for the next leaf
    }
}

// index of a colour in solid_values = how many colours have a smaller key (keys of used colours are distinct, an unused
// colour's is ~0); their number is the solid count
__global__ __launch_bounds__(256) void k_solid_rank(SimpTable sp, BuildCtl *ctl) {
    __shared__ u64 tile[256];
    const uint32_t n = min(ctl->ncolors, MAX_COLORS);
    if (blockIdx.x * 256u >= n) return;  // the whole block
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const u64 mine = i < n ? sp.skey[i] : ~0ull;
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += 256) {
        tile[threadIdx.x] = j0 + threadIdx.x < n ? sp.skey[j0 + threadIdx.x] : ~0ull;
        __syncthreads();
        const uint32_t m = min(256u, n - j0);
        for (uint32_t j = 0; j < m; ++j) rank += tile[j] < mine;
        __syncthreads();
    }
    const bool used = mine != ~0ull;
    if (used) {
        sp.srank[i] = rank;
        sp.svals[rank] = i | 0xFFFF0000u;  // pix_visual: colour index, no data
    }
    const u64 b = __ballot(used);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(&ctl->solid_count, (uint32_t)__popcll(b));
}

// k_emit_nodes for the leaf level of a simplified image: one thread per (possible leaf c, sectant s)
__global__ __launch_bounds__(256) void k_emit_leaves(GridP g, uint64_t n, const u64 *occ, const u64 *rank,
                                                     const u64 *first, uint32_t base, ColorTable t, SimpTable sp,
                                                     uint32_t *node_type, u64 *node_ocbits, uint32_t *node_children) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t c = gid >> 6;
    const uint32_t s = (uint32_t)gid & 63u;
    if (c >= n) return;
    const u64 w = occ[c];
    if (w == 0 && g.D != 0) return;  // no such node
    const uint64_t ni = (uint64_t)base + rank[c];
    const uint32_t cls = (uint32_t)(sp.linfo[c] >> 8) & 3u;
    if (s == 0) {
        node_type[ni] = w ? (cls == LEAF_PLAIN ? VHX_NODE_LEAF : VHX_NODE_UNIFORM_LEAF) : VHX_NODE_NOTHING;
        node_ocbits[ni] = w;
    }
    uint32_t child = VHX_EMPTY;
    if (cls == LEAF_UNIFORM_PARTED) {
        if (s == 0) child = (uint32_t)first[c];
    } else if (((w >> s) & 1ull) && (cls == LEAF_PLAIN || s == 0)) {
        const u64 pm = sp.pmask[c];
        if ((pm >> s) & 1ull) {
            child = (uint32_t)(first[c] + (u64)__popcll(pm & ((1ull << s) - 1ull)));
        } else {
            uint32_t lx, ly, lz;
            leaf_coord(c, g.D, lx, ly, lz);
            const uint32_t lsh = g.bsh + 2;
            const uint32_t cs = grid_at(g, (lx << lsh) + ((s & 3u) << g.bsh), (ly << lsh) + (((s >> 2) & 3u) << g.bsh),
                                        (lz << lsh) + ((s >> 4) << g.bsh));
            child = VHX_SOLID_BIT | sp.srank[color_lookup(t, cs)];
        }
    }
    node_children[ni * 64 + s] = child;
}

// The one brick of every block-uniform leaf: cell (x, y, z) is the value of the leaf's block (x, y, z), read at the
// block's corner voxel.
__global__ __launch_bounds__(256) void k_emit_uniform(GridP g, const u64 *first, uint64_t nleaf, ColorTable t,
                                                      SimpTable sp, uint32_t *voxels) {
    const uint32_t bd = 1u << g.bsh, n3sh = 3 * g.bsh, lsh = g.bsh + 2;
    for (uint64_t code = blockIdx.x; code < nleaf; code += gridDim.x) {
        if (((uint32_t)(sp.linfo[code] >> 8) & 3u) != LEAF_UNIFORM_PARTED) continue;  // the whole block
        uint32_t lx, ly, lz;
        leaf_coord(code, g.D, lx, ly, lz);
        uint32_t *dst = voxels + (first[code] << n3sh);
        for (uint32_t i = threadIdx.x; i < (1u << n3sh); i += 256) {
            const uint32_t c = grid_at(g, (lx << lsh) + ((i & (bd - 1u)) << 2), (ly << lsh) + (((i >> g.bsh) & (bd - 1u)) << 2),
                                       (lz << lsh) + ((i >> (2 * g.bsh)) << 2));
            dst[i] = c ? (color_lookup(t, c) | 0xFFFF0000u) : VHX_EMPTY;
        }
    }
}

struct FillArg {
    vhx_ctx *c;
    GridP g;
    bool simplified;
    uint32_t solid_count;
    uint32_t levels;
    uint64_t level_off[MAX_LEVELS];
    uint32_t level_base[MAX_LEVELS];
    uint32_t color_count;
    uint32_t data_count;  // vhx_build_tree_dense_data; 0 without a data plane
};

// receive_tree's fill step: the emission kernels write straight into the tree's raw buffers
int fill_from_scratch(void *arg, void *const dst[7], const uint64_t bytes[7]) {
    const FillArg &a = *(const FillArg *)arg;
    vhx_ctx *c = a.c;
    const u64 *occ = (const u64 *)c->build.occ.ptr, *rank = (const u64 *)c->build.rank.ptr;
    const u64 *first = (const u64 *)c->build.first.ptr;
    const ColorTable t = table_of(c->build.table.ptr);
    const ColorTable dt = a.g.d ? table_of(c->build.dtable.ptr) : ColorTable{};
    const uint32_t D = a.levels - 1;
    const uint64_t nleaf = 1ull << (6 * D);
    const SimpTable sp = a.simplified ? simp_of(c->build.simp.ptr, nleaf) : SimpTable{};
    for (uint32_t lv = 0; lv <= D; ++lv) {
        const uint64_t n = 1ull << (6 * lv);
        const uint64_t child_off = lv < D ? a.level_off[lv + 1] : 0;
        if (a.simplified && lv == D)
            k_emit_leaves<<<blocks_for(n * 64), 256, 0, c->stream>>>(
                a.g, n, occ + a.level_off[lv], rank + a.level_off[lv], first, a.level_base[lv], t, sp,
                (uint32_t *)dst[VHX_BUF_NODE_TYPE], (u64 *)dst[VHX_BUF_NODE_OCBITS], (uint32_t *)dst[VHX_BUF_NODE_CHILDREN]);
        else
            k_emit_nodes<<<blocks_for(n * 64), 256, 0, c->stream>>>(
                lv, D, n, occ + a.level_off[lv], rank + a.level_off[lv], rank + child_off, first, a.level_base[lv],
                lv < D ? a.level_base[lv + 1] : 0u, (uint32_t *)dst[VHX_BUF_NODE_TYPE], (u64 *)dst[VHX_BUF_NODE_OCBITS],
                (uint32_t *)dst[VHX_BUF_NODE_CHILDREN]);
    }
    VHX_HIP(c, hipGetLastError());
    if (bytes[VHX_BUF_VOXELS]) {
        const unsigned blocks = (unsigned)std::min<uint64_t>(nleaf, (uint64_t)c->cus * 16);
        // a simplified image copies the Parted bricks only
        if (a.g.d)
            k_emit_bricks<1><<<blocks, 256, 0, c->stream>>>(a.g, occ + a.level_off[D], first, nleaf, t, dt,
                                                            (uint32_t *)dst[VHX_BUF_VOXELS]);
        else
            k_emit_bricks<0><<<blocks, 256, 0, c->stream>>>(a.g, a.simplified ? sp.pmask : occ + a.level_off[D], first,
                                                            nleaf, t, dt, (uint32_t *)dst[VHX_BUF_VOXELS]);
        if (a.simplified && a.g.bsh > 0)
            k_emit_uniform<<<blocks, 256, 0, c->stream>>>(a.g, first, nleaf, t, sp, (uint32_t *)dst[VHX_BUF_VOXELS]);
        VHX_HIP(c, hipGetLastError());
    }
    if (bytes[VHX_BUF_SOLID_VALUES])
        VHX_HIP(c, hipMemcpyAsync(dst[VHX_BUF_SOLID_VALUES], sp.svals, (uint64_t)a.solid_count * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
    if (bytes[VHX_BUF_COLOR_PALETTE])
        VHX_HIP(c, hipMemcpyAsync(dst[VHX_BUF_COLOR_PALETTE], t.pal, (uint64_t)a.color_count * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
    if (a.data_count && bytes[VHX_BUF_DATA_PALETTE])
        VHX_HIP(c, hipMemcpyAsync(dst[VHX_BUF_DATA_PALETTE], dt.pal, (uint64_t)a.data_count * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
    return VHX_OK;
}

// the entry points; `name` is the one called, for the error texts. `data` (null: none) lives where grid->albedo lives
// and is not combined with `simplified`.
int build_tree(vhx_ctx *c, const vhx_dense_desc *grid, const uint32_t *data, int on_device, bool simplified,
               const char *name) {
    const auto fail_in = [&](int code, const char *what) { return fail(c, code, std::string(name) + what); };
    if (!c || !grid) return fail_in(VHX_E_INVALID_ARG, ": null argument");
    if (c->shared) return fail_in(VHX_E_STATE, " on a shared context: build through the owner");
    {
        vhx_boxtree *probe = nullptr;  // the validity rules of BoxTree::new
        const int rc = vhx_boxtree_new(grid->boxtree_size, grid->brick_dim, &probe);
        if (rc) return fail_in(rc, ": invalid boxtree_size / brick_dim");
        vhx_boxtree_free(probe);
    }
    const uint32_t S = grid->boxtree_size, bd = grid->brick_dim;
    if (!grid->albedo || grid->gx == 0 || grid->gy == 0 || grid->gz == 0 || grid->gx > S || grid->gy > S || grid->gz > S)
        return fail_in(VHX_E_INVALID_ARG, ": null grid, or an extent of 0 or above boxtree_size");
    if ((bd & (bd - 1)) != 0 || (S & (S - 1)) != 0 || S < 4 * bd)
        return fail_in(VHX_E_INVALID_ARG, ": sizes must be powers of two");
    GridP g{};
    g.gx = grid->gx;
    g.gy = grid->gy;
    g.gz = grid->gz;
    while ((1u << g.bsh) < bd) ++g.bsh;
    const uint32_t nl = S / (4 * bd);  // leaf nodes per axis = 4^D
    while ((1u << (2 * g.D)) < nl) ++g.D;
    if ((1u << (2 * g.D)) != nl)
        return fail_in(VHX_E_INVALID_ARG, ": boxtree_size is not brick_dim * 4^k");
    const uint32_t D = g.D, levels = D + 1;
    const uint64_t nleaf = 1ull << (6 * D);
    if (levels > MAX_LEVELS || nleaf > MAX_LEAVES)
        return fail_in(VHX_E_CAPACITY, ": more than 2^28 possible leaf nodes");
    FillArg fa{};
    fa.c = c;
    fa.levels = levels;
    fa.simplified = simplified;
    uint64_t words = 0;
    for (uint32_t lv = 0; lv < levels; ++lv) {
        fa.level_off[lv] = words;
        words += 1ull << (6 * lv);
    }

    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    // scratch: a buffer that grows is reallocated, which waits for the device (the previous build has completed: the
    // call is synchronous)
    int rc;
    if ((rc = vhx::ensure(c, c->build.occ, words * 8))) return rc;
    if ((rc = vhx::ensure(c, c->build.rank, words * 8))) return rc;
    if ((rc = vhx::ensure(c, c->build.first, nleaf * 8))) return rc;
    if ((rc = vhx::ensure(c, c->build.part, ((nleaf + SCAN_TILE - 1) / SCAN_TILE) * 8))) return rc;
    if ((rc = vhx::ensure(c, c->build.table, TAB_BYTES))) return rc;
    if (data && (rc = vhx::ensure(c, c->build.dtable, TAB_BYTES))) return rc;
    if ((rc = vhx::ensure(c, c->build.ctl, 2 * sizeof(BuildCtl)))) return rc;  // [1]: the data table's counters
    if (simplified && (rc = vhx::ensure(c, c->build.simp, simp_bytes(nleaf)))) return rc;
    const uint64_t voxels = (uint64_t)g.gx * g.gy * g.gz;
    if (on_device) {
        g.a = grid->albedo;
        g.d = data;
    } else {
        if ((rc = vhx::ensure(c, c->build.grid, voxels * (data ? 8 : 4)))) return rc;
        VHX_HIP(c, hipMemcpyAsync(c->build.grid.ptr, grid->albedo, voxels * 4, hipMemcpyHostToDevice, c->stream));
        g.a = (const uint32_t *)c->build.grid.ptr;
        if (data) {  // the data plane follows the albedo plane
            VHX_HIP(c, hipMemcpyAsync((uint32_t *)c->build.grid.ptr + voxels, data, voxels * 4, hipMemcpyHostToDevice,
                                      c->stream));
            g.d = g.a + voxels;
        }
    }
    fa.g = g;
    u64 *occ = (u64 *)c->build.occ.ptr, *rank = (u64 *)c->build.rank.ptr, *first = (u64 *)c->build.first.ptr;
    BuildCtl *ctl = (BuildCtl *)c->build.ctl.ptr;
    const ColorTable t = table_of(c->build.table.ptr);
    const ColorTable dt = data ? table_of(c->build.dtable.ptr) : ColorTable{};
    // full reset: leaf masks (the other levels are overwritten), counters, table keys free, first indices at maximum
    VHX_HIP(c, hipMemsetAsync(occ, 0, words * 8, c->stream));
    VHX_HIP(c, hipMemsetAsync(ctl, 0, 2 * sizeof(BuildCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(t.keys, 0, TAB_KEYS_BYTES, c->stream));
    VHX_HIP(c, hipMemsetAsync(t.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    if (data) {
        VHX_HIP(c, hipMemsetAsync(dt.keys, 0, TAB_KEYS_BYTES, c->stream));
        VHX_HIP(c, hipMemsetAsync(dt.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    }
    const SimpTable sp = simplified ? simp_of(c->build.simp.ptr, nleaf) : SimpTable{};
    if (simplified) {  // absent leaves have no bricks; no colour has a Solid entry yet
        VHX_HIP(c, hipMemsetAsync(sp.pmask, 0, nleaf * 16, c->stream));
        VHX_HIP(c, hipMemsetAsync(sp.skey, 0xFF, SKEY_BYTES, c->stream));
    }

    // pass A
    {
        const bool vec = (g.gx % 4u) == 0 && ((uintptr_t)g.a % 16u) == 0 && ((uintptr_t)g.d % 16u) == 0;
        const uint32_t gxv = vec ? g.gx / 4 : g.gx;
        uint32_t xsh = 0;
        while (xsh < 8 && (1u << xsh) < gxv) ++xsh;
        const uint32_t tpr = 1u << xsh, rpb = 256u >> xsh;
        const dim3 blocks((gxv + tpr - 1) / tpr, std::min<uint32_t>((g.gy + rpb * SCAN_ROWS - 1) / (rpb * SCAN_ROWS), 65535u),
                          std::min<uint32_t>(g.gz, 65535u));
        if (data && vec)
            k_dense_scan<4, 1><<<blocks, 256, 0, c->stream>>>(g, xsh, occ + fa.level_off[D], t, dt, ctl);
        else if (data)
            k_dense_scan<1, 1><<<blocks, 256, 0, c->stream>>>(g, xsh, occ + fa.level_off[D], t, dt, ctl);
        else if (vec)
            k_dense_scan<4, 0><<<blocks, 256, 0, c->stream>>>(g, xsh, occ + fa.level_off[D], t, dt, ctl);
        else
            k_dense_scan<1, 0><<<blocks, 256, 0, c->stream>>>(g, xsh, occ + fa.level_off[D], t, dt, ctl);
        VHX_HIP(c, hipGetLastError());
    }
    // occupancy upwards, ranks per level, first brick of every leaf
    for (uint32_t lv = D; lv-- > 0;) {
        const uint64_t np = 1ull << (6 * lv);
        k_reduce_level<<<blocks_for(np * 64), 256, 0, c->stream>>>(occ + fa.level_off[lv + 1], occ + fa.level_off[lv], np);
    }
    VHX_HIP(c, hipGetLastError());
    for (uint32_t lv = 0; lv < levels; ++lv)
        if ((rc = scan_level<0>(c, occ + fa.level_off[lv], 1ull << (6 * lv), lv == 0, rank + fa.level_off[lv],
                                &ctl->level_total[lv])))
            return rc;
    if (!simplified && (rc = scan_level<1>(c, occ + fa.level_off[D], nleaf, false, first, &ctl->brick_total))) return rc;
    // palette
    k_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(t, ctl);
    k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(t, ctl);
    if (data) {  // the data palette, ranked on its own
        k_pal_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(dt, ctl + 1);
        k_pal_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(dt, ctl + 1);
    }
    VHX_HIP(c, hipGetLastError());
    if (simplified) {  // leaf classes, the first brick of every leaf from its Parted bricks, the solid values
        k_classify<<<(unsigned)std::min<uint64_t>(nleaf, (uint64_t)c->cus * 16), 256, 0, c->stream>>>(
            g, occ + fa.level_off[D], nleaf, t, sp);
        VHX_HIP(c, hipGetLastError());
        if ((rc = scan_level<2>(c, sp.linfo, nleaf, false, first, &ctl->brick_total))) return rc;
        k_solid_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(sp, ctl);
        VHX_HIP(c, hipGetLastError());
    }

    // the one readback before allocation
    BuildCtl hb[2];
    VHX_HIP(c, hipMemcpyAsync(hb, ctl, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    const BuildCtl &h = hb[0];
    if (h.overflow || h.ncolors > MAX_COLORS)
        return fail_in(VHX_E_CAPACITY, ": more than 65535 distinct colours");
    if (hb[1].overflow || hb[1].ncolors > MAX_COLORS)
        return fail_in(VHX_E_CAPACITY, ": more than 65535 distinct data values");
    if (h.brick_total >= 0x80000000ull) return fail_in(VHX_E_CAPACITY, ": 2^31 bricks or more");
    uint64_t nodes = 0;
    for (uint32_t lv = 0; lv < levels; ++lv) {
        fa.level_base[lv] = (uint32_t)nodes;
        nodes += h.level_total[lv];
    }
    if (nodes >= 0xFFFFFFFFull) return fail_in(VHX_E_CAPACITY, ": 2^32 nodes or more");
    fa.color_count = h.ncolors;
    fa.data_count = hb[1].ncolors;
    fa.solid_count = simplified ? h.solid_count : 0u;
    vhx_tree_desc counts{};
    counts.boxtree_size = S;
    counts.brick_dim = bd;
    counts.node_count = (uint32_t)nodes;
    counts.brick_count = (uint32_t)h.brick_total;
    counts.solid_count = fa.solid_count;
    counts.color_count = h.ncolors;
    counts.data_count = hb[1].ncolors;
    return vhx::receive_tree(c, counts, fill_from_scratch, &fa);
}

}  // namespace

extern "C" {

int vhx_build_tree_dense(vhx_ctx *c, const vhx_dense_desc *grid, int on_device) {
    return build_tree(c, grid, nullptr, on_device, false, "vhx_build_tree_dense");
}

int vhx_build_tree_dense_simplified(vhx_ctx *c, const vhx_dense_desc *grid, int on_device) {
    return build_tree(c, grid, nullptr, on_device, true, "vhx_build_tree_dense_simplified");
}

int vhx_build_tree_dense_data(vhx_ctx *c, const vhx_dense_desc *grid, const uint32_t *data, int on_device) {
    if (!data) return vhx_build_tree_dense(c, grid, on_device);
    return build_tree(c, grid, data, on_device, false, "vhx_build_tree_dense_data");
}

int vhx_tree_counts(const vhx_ctx *c, vhx_tree_desc *counts) {
    if (!c || !counts) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return VHX_E_STATE;
    *counts = c->tree->desc;  // its array pointers are null
    return VHX_OK;
}

int vhx_read_range(vhx_ctx *c, int id, uint64_t off, uint64_t count, void *dst) {
    if (!c || id < 0 || id > 6 || (!dst && count)) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_read_range before vhx_upload_tree");
    const uint64_t cap = vhx::elem_count(c->tree->desc, id), es = vhx::elem_size(id);
    if (off > cap || count > cap - off) return fail(c, VHX_E_CAPACITY, "vhx_read_range: range beyond the uploaded buffer");
    if (count == 0) return VHX_OK;
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    vhx::TraceScope tscope(c);  // after the tree's last write
    if (tscope.rc) return tscope.rc;
    VHX_HIP(c, hipMemcpyAsync(dst, (const char *)c->tree->raw[id].ptr + off * es, count * es, hipMemcpyDeviceToHost,
                              c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    return tscope.end();
}

}  // extern "C"
