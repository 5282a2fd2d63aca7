// vhx_simplify_tree: the resident tree after BoxTree::simplify(ROOT, recursive), without its unreachable slots and in
// the builders' numbering, on the device and out of place. The image is a pure function of the old
// one (vhx_flat_simplify, flatten.cpp, is the CPU reference, and include/vhx_boxtree.h states the rules): Parted
// bricks of one value become Solid, or Empty where the value points to empty; a Leaf of 64 equal Solid bricks becomes a
// UniformLeaf over that brick, a Leaf whose aligned 4x4x4 voxel blocks are all homogeneous a UniformLeaf over one new
// Parted brick; an Internal node without occupied bits becomes Nothing and its subtree leaves; solid_values are the
// distinct values of the Solid entries that remain, by first (new node, sectant).
//
//   frontier  walk_and_claim  the compaction's walk (treepack.hpp), an Internal node without occupied bits reaching
//                             nothing; it also claims every reachable Parted brick: the compaction's checks
//   classify  k_smp_classify  the hot pass, a workgroup per new node: reads a leaf's 64 entries and the cells of its
//                             Parted bricks once, in 16-byte words; a lane ORs bit s where a cell of brick s differs
//                             from the brick's corner cell, and a flag where a cell differs from the corner of its
//                             4x4x4 block (brick_dim >= 8; below that the blocks follow from the bricks). OR inside
//                             the wave, then in LDS. Wave 0 decides the node's class, the bricks it keeps and the
//                             value of every entry, and records each Solid value's first key node * 64 + sectant
//   bricks    k_scan_*        MODE 2: the node's first new brick, from the brick counts of the classes
//             k_smp_bfill     src[new brick] = old brick for the kept ones; VHX_EMPTY stays for the bricks written anew
//   solids    k_smp_solid_compact, k_smp_solid_rank   the values ranked by their keys: solid_values, each value's index
//   -- one readback of the counters; refusals happen here; the new buffers are allocated --
//   emit      k_smp_emit      types, occupancy and entries by class
//   gather    k_cmp_gather*   the kept bricks and their bitmaps (treepack.hpp), leaving the new bricks' slots alone
//             k_smp_uniform   the one brick of every block-uniform leaf, sampled at the block corners
//   derive    the new bricks' bitmaps, headers and child records by the tree unit's kernels
//
// Nothing of the old tree is written. The atomics feed only flags, claims and minima, every index that reaches a buffer
// comes from a scan or a rank, and every global write is a plain store. Every index read from the tree is checked
// against its count before it is used as an address.
#include <algorithm>
#include <string>

#include "../../include/vhx.h"
// the palette ranking of buildtab.hpp is not used here (the Solid values have a ranking of their own, which
// vhx_lod.hip shares: solid_insert, k_smp_solid_compact and k_smp_solid_rank live in treepack.hpp)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "treepack.hpp"
#pragma clang diagnostic pop
#include "ctx.hpp"
#include "treewalk.hpp"

namespace {

// what a new node is: the brick count it contributes sits in bits 0..6 of its binfo word, this in bits 8..10
constexpr uint32_t CLS_NOTHING = 0, CLS_INTERNAL = 1, CLS_LEAF = 2;
constexpr uint32_t CLS_UNIFORM = 3;      // a UniformLeaf whose entry 0 is empty, Solid or a kept brick
constexpr uint32_t CLS_UNIFORM_NEW = 4;  // a UniformLeaf over a new Parted brick of block values

struct SimplifyCtl {
    CompactCtl w;    // the walk's
    BuildCtl b;      // the table of Solid values: ncolors distinct values that are not 0, overflow, ncompact
    u64 new_bricks;  // Parted bricks of the new image
    u64 zero_key;    // the Solid value 0 (a legal word, but the table's free-slot marker): its first key, ~0 = unused
    uint32_t zero_rank, pad;
};

struct SimpIn {
    const uint32_t *vox, *solids, *color, *data;
    uint32_t solid_count, ncolor, ndata;
    uint32_t bsh;  // log2(brick_dim)
};

struct SimpMaps {
    u64 *binfo, *pmask, *gmask, *bfirst;  // [node_count] by new index
    uint32_t *ent;                        // [node_count * 64]: VHX_EMPTY, a Solid value, or (pmask) an old brick
    uint32_t *bsrc;                       // [brick_count + node_count]
    uint32_t *newb;                       // [node_count] the brick written anew for a block-uniform leaf, else VHX_EMPTY
};

constexpr uint32_t CLS_LOADS = 4;  // 16-byte loads a thread has in flight

// One workgroup per new node at a time. `nodes` is read from the walk's counters; the loop bounds are the same for
// every thread of a block, so the wave operations run with all 64 lanes.
__global__ __launch_bounds__(256) void k_smp_classify(OldTree t, Maps m, SimpIn in, SimpMaps sm, ColorTable tab,
                                                      SimplifyCtl *ctl) {
    __shared__ u64 s_ns;
    __shared__ uint32_t s_nb, s_np;
    __shared__ uint32_t s_sect[64], s_brick[64], s_c0[64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t bsh = in.bsh, n3sh = 3 * bsh, bdm = (1u << bsh) - 1u;
    const uint32_t nodes = min(ctl->w.end, t.node_count);
    for (uint32_t i = blockIdx.x; i < nodes; i += gridDim.x) {
        const uint32_t o = m.old_of[i];
        const uint32_t ty = o < t.node_count ? t.type[o] : VHX_NODE_NOTHING;
        if (ty != VHX_NODE_LEAF && ty != VHX_NODE_UNIFORM_LEAF) {  // the whole block
            if (tid == 0) {
                const uint32_t cls = ty == VHX_NODE_INTERNAL && t.ocbits[o] != 0 ? CLS_INTERNAL : CLS_NOTHING;
                sm.binfo[i] = (u64)cls << 8;
                sm.pmask[i] = 0;
                sm.gmask[i] = 0;
            }
            continue;
        }
        uint32_t e = VHX_EMPTY, k = 0;
        bool parted = false;
        if (tid < 64) {  // wave 0: a lane per sectant
            if (ty == VHX_NODE_LEAF || tid == 0) e = t.children[(uint64_t)o * 64u + tid];
            parted = is_parted(e) && e < t.brick_count;  // past the count: the walk has raised its flag
            const u64 pm = __ballot(parted);
            k = (uint32_t)__popcll(pm & ((1ull << tid) - 1ull));
            if (parted) {
                s_sect[k] = tid;
                s_brick[k] = e;
                s_c0[k] = in.vox[(uint64_t)e << n3sh];
            }
            if (tid == 0) {
                s_np = (uint32_t)__popcll(pm);
                s_ns = 0;
                s_nb = 0;
            }
        }
        __syncthreads();
        if (bsh >= 1) {
            const uint32_t n4sh = n3sh - 2;
            const uint32_t items = s_np << n4sh;  // 16-byte words of the node's Parted bricks
            const uint4 *vox4 = (const uint4 *)in.vox;
            u64 ns = 0;
            bool nb = false;
            for (uint32_t q0 = tid; q0 < items; q0 += 256u * CLS_LOADS) {
                uint4 v[CLS_LOADS];
                uint32_t cv[CLS_LOADS];
#pragma unroll
                for (uint32_t u = 0; u < CLS_LOADS; ++u) {
                    const uint32_t q = q0 + 256u * u;
                    if (q < items) {
                        const uint32_t kk = q >> n4sh, w = q & ((1u << n4sh) - 1u);
                        const uint32_t b = s_brick[kk];
                        v[u] = vox4[((uint64_t)b << n4sh) + w];
                        if (bsh >= 3) {  // the word is a run along x inside one block: the block's corner cell
                            const uint32_t c = w << 2;
                            const uint32_t corner = (c & bdm) | ((((c >> bsh) & bdm) & ~3u) << bsh) |
                                                    (((c >> (2 * bsh)) & ~3u) << (2 * bsh));
                            cv[u] = in.vox[((uint64_t)b << n3sh) + corner];
                        }
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < CLS_LOADS; ++u) {
                    const uint32_t q = q0 + 256u * u;
                    if (q < items) {
                        const uint32_t kk = q >> n4sh;
                        const uint32_t c0 = s_c0[kk];
                        if (v[u].x != c0 || v[u].y != c0 || v[u].z != c0 || v[u].w != c0) ns |= 1ull << s_sect[kk];
                        if (bsh >= 3) nb = nb || v[u].x != cv[u] || v[u].y != cv[u] || v[u].z != cv[u] || v[u].w != cv[u];
                    }
                }
            }
#pragma unroll
            for (uint32_t s = 1; s < 64; s <<= 1) ns |= __shfl_xor(ns, s);
            const bool wave_nb = __ballot(nb) != 0;
            if (lane == 0) {
                if (ns) atomicOr(&s_ns, ns);
                if (wave_nb) atomicOr(&s_nb, 1u);
            }
            __syncthreads();
        }
        if (tid < 64) {
            // the entry after BoxTree::brick_simplify: r = VHX_EMPTY, the Solid value, or the old index of a kept brick
            uint32_t r = VHX_EMPTY;
            bool solid = false, keep = false;
            if (parted) {
                if ((s_ns >> tid) & 1ull) {
                    keep = true;
                    r = e;
                } else {
                    const uint32_t v = s_c0[k];
                    if (!cell_empty(v, in.color, in.ncolor, in.data, in.ndata)) {
                        solid = true;
                        r = v;
                    }
                }
            } else if (e != VHX_EMPTY && (e & VHX_SOLID_BIT)) {
                const uint32_t idx = e & ~VHX_SOLID_BIT;
                if (idx >= in.solid_count) {
                    atomicOr(&ctl->w.bad, BAD_INDEX);
                } else {
                    const uint32_t v = in.solids[idx];
                    if (!cell_empty(v, in.color, in.ncolor, in.data, in.ndata)) {
                        solid = true;
                        r = v;
                    }
                }
            }
            const u64 solidm = __ballot(solid), keepm = __ballot(keep);
            uint32_t cls, cnt = 0;
            u64 gm = 0;
            if (ty == VHX_NODE_UNIFORM_LEAF) {
                const uint32_t e0 = __shfl(e, 0);
                const bool was_solid = e0 != VHX_EMPTY && (e0 & VHX_SOLID_BIT);
                if (was_solid && !(solidm & 1ull)) {
                    cls = CLS_NOTHING;  // a Solid brick that points to empty
                } else {
                    cls = CLS_UNIFORM;
                    gm = keepm & 1ull;
                    cnt = (uint32_t)gm;
                }
            } else {
                const bool same = __ballot(r == __shfl(r, 0)) == ~0ull;
                if (solidm == ~0ull && same) {
                    cls = CLS_UNIFORM;
                } else if (bsh == 0) {
                    cls = CLS_LEAF;
                } else {
                    bool uniform;
                    if (bsh == 1)  // a block spans 2x2x2 bricks: none kept, and each equal to the block's corner brick
                        uniform = keepm == 0 && __ballot(r == __shfl(r, tid & 0x2Au)) == ~0ull;
                    else if (bsh == 2)  // a block is a brick
                        uniform = keepm == 0;
                    else
                        uniform = s_nb == 0;
                    if (uniform) {
                        cls = CLS_UNIFORM_NEW;
                        cnt = 1;
                    } else {
                        cls = CLS_LEAF;
                        gm = keepm;
                        cnt = (uint32_t)__popcll(gm);
                    }
                }
            }
            sm.ent[(uint64_t)i * 64u + tid] = r;
            if (tid == 0) {
                sm.binfo[i] = (u64)cnt | ((u64)cls << 8);
                sm.pmask[i] = keepm;
                sm.gmask[i] = gm;
            }
            // the Solid entries the node will hold: the lowest sectant of a value records it for the node
            const bool cand = solid && (cls == CLS_LEAF || (cls == CLS_UNIFORM && tid == 0));
            u64 pending = __ballot(cand);
            while (pending) {  // the same in every lane
                const uint32_t leader = (uint32_t)__ffsll((long long)pending) - 1u;
                const uint32_t lv = __shfl(r, leader);
                if (lane == leader) solid_insert(tab, ctl, r, (u64)i * 64ull + tid);
                pending &= ~__ballot(cand && r == lv);
            }
        }
        __syncthreads();  // the shared words are rewritten for the next node
    }
}

// one thread per (new node, sectant): the source of every kept brick; the index comes from the scan
__global__ __launch_bounds__(256) void k_smp_bfill(SimpMaps sm, const SimplifyCtl *ctl, uint32_t node_count,
                                                   uint64_t cap) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = gid >> 6;
    if (i >= min(ctl->w.end, node_count)) return;
    const u64 mask = sm.gmask[i];
    if (((mask >> lane) & 1ull) == 0) return;
    const u64 j = sm.bfirst[i] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    if (j < cap) sm.bsrc[j] = sm.ent[i * 64u + lane];
}

// one thread per (new node, sectant); runs only for a tree that passed the checks
__global__ __launch_bounds__(256) void k_smp_emit(OldTree t, Maps m, SimpMaps sm, ColorTable tab,
                                                  const SimplifyCtl *ctl, uint32_t nodes, uint32_t *type, u64 *ocbits,
                                                  uint32_t *children) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = gid >> 6;
    const uint32_t s = (uint32_t)gid & 63u;
    if (i >= nodes) return;
    const uint32_t o = m.old_of[i];
    const uint32_t cls = (uint32_t)(sm.binfo[i] >> 8) & 7u;
    if (s == 0) {
        type[i] = cls == CLS_NOTHING ? VHX_NODE_NOTHING : cls == CLS_INTERNAL ? VHX_NODE_INTERNAL
                  : cls == CLS_LEAF  ? VHX_NODE_LEAF                                              : VHX_NODE_UNIFORM_LEAF;
        ocbits[i] = t.ocbits[o];
        sm.newb[i] = cls == CLS_UNIFORM_NEW ? (uint32_t)sm.bfirst[i] : VHX_EMPTY;
    }
    uint32_t child = VHX_EMPTY;
    if (cls == CLS_INTERNAL) {
        const uint32_t e = t.children[(uint64_t)o * 64u + s];
        if (e != VHX_EMPTY) child = m.new_of[e];
    } else if (cls == CLS_UNIFORM_NEW) {
        if (s == 0) child = (uint32_t)sm.bfirst[i];
    } else if (cls == CLS_LEAF || (cls == CLS_UNIFORM && s == 0)) {
        const uint32_t r = sm.ent[gid];
        const u64 gm = sm.gmask[i];
        if ((gm >> s) & 1ull)
            child = (uint32_t)sm.bfirst[i] + (uint32_t)__popcll(gm & ((1ull << s) - 1ull));
        else if (r != VHX_EMPTY)
            child = VHX_SOLID_BIT | (r == 0 ? ctl->zero_rank : color_lookup(tab, r));
    }
    children[gid] = child;
}

// The one brick of every block-uniform leaf: cell (x, y, z) is voxel (4x, 4y, 4z) of the leaf -- the value of the entry
// that holds it, or that cell of a kept Parted brick (brick_dim >= 8).
__global__ __launch_bounds__(256) void k_smp_uniform(SimpIn in, SimpMaps sm, uint32_t nodes, uint32_t *voxels) {
    const uint32_t bsh = in.bsh, n3sh = 3 * bsh, bdm = (1u << bsh) - 1u;
    for (uint32_t i = blockIdx.x; i < nodes; i += gridDim.x) {
        if (((uint32_t)(sm.binfo[i] >> 8) & 7u) != CLS_UNIFORM_NEW) continue;  // the whole block
        const u64 pm = sm.pmask[i];
        uint32_t *dst = voxels + (sm.bfirst[i] << n3sh);
        for (uint32_t c = threadIdx.x; c < (1u << n3sh); c += 256) {
            const uint32_t vx = (c & bdm) << 2, vy = ((c >> bsh) & bdm) << 2, vz = (c >> (2 * bsh)) << 2;
            const uint32_t s = (vx >> bsh) | ((vy >> bsh) << 2) | ((vz >> bsh) << 4);
            uint32_t r = sm.ent[(uint64_t)i * 64u + s];
            if ((pm >> s) & 1ull)
                r = in.vox[((uint64_t)r << n3sh) + ((vx & bdm) | ((vy & bdm) << bsh) | ((vz & bdm) << (2 * bsh)))];
            dst[c] = r;
        }
    }
}

}  // namespace

extern "C" {

int vhx_simplify_tree(vhx_ctx *c, uint32_t *nodes_dropped, uint32_t *bricks_dropped) {
    if (!c) return VHX_E_INVALID_ARG;
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_simplify_tree on a shared context: simplify through the owner");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_simplify_tree before vhx_upload_tree");
    if (c->tree->mips_on) return fail(c, VHX_E_STATE, "vhx_simplify_tree while node MIPs are set");
    const vhx_tree_desc d = c->tree->desc;
    const uint64_t nn = d.node_count, nb = d.brick_count;
    const uint64_t n3 = (uint64_t)d.brick_dim * d.brick_dim * d.brick_dim;
    const uint64_t bsrc_cap = nb + nn;  // a node keeps bricks it had, or gains one

    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    vhx::WriteScope ws(c);  // frames in flight on the tree's other contexts finish reading it first
    int rc = ws.rc;
    if (rc) return rc;
    Maps m;
    CompactCtl *wctl;
    if ((rc = ensure_maps(c, nn, nb, &m, &wctl))) return rc;
    vhx_ctx::SimplifyScratch &ss = c->simplify;
    if ((rc = vhx::ensure(c, ss.binfo, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, ss.pmask, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, ss.gmask, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, ss.bfirst, nn * 8))) return rc;
    if ((rc = vhx::ensure(c, ss.ent, nn * 64 * 4))) return rc;
    if ((rc = vhx::ensure(c, ss.bsrc, bsrc_cap * 4))) return rc;
    if ((rc = vhx::ensure(c, ss.newb, nn * 4))) return rc;
    if ((rc = vhx::ensure(c, ss.ctl, sizeof(SimplifyCtl)))) return rc;
    if ((rc = vhx::ensure(c, c->build.table, TAB_BYTES))) return rc;
    const SimpMaps sm{(u64 *)ss.binfo.ptr, (u64 *)ss.pmask.ptr, (u64 *)ss.gmask.ptr,
                      (u64 *)ss.bfirst.ptr, (uint32_t *)ss.ent.ptr, (uint32_t *)ss.bsrc.ptr,
                      (uint32_t *)ss.newb.ptr};
    SimplifyCtl *ctl = (SimplifyCtl *)ss.ctl.ptr;
    const ColorTable tab = table_of(c->build.table.ptr);
    const TreeStore &ts = *c->tree;
    const OldTree t{(const uint32_t *)ts.raw[VHX_BUF_NODE_TYPE].ptr, (const u64 *)ts.raw[VHX_BUF_NODE_OCBITS].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_NODE_CHILDREN].ptr, d.node_count, d.brick_count};
    const SimpIn in{(const uint32_t *)ts.raw[VHX_BUF_VOXELS].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_SOLID_VALUES].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_COLOR_PALETTE].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_DATA_PALETTE].ptr,
                    d.solid_count, d.color_count, d.data_count, lg2(d.brick_dim)};
    // reset: no counts, no key, an empty table, every new brick without a source
    VHX_HIP(c, hipMemsetAsync(ctl, 0, sizeof(SimplifyCtl), c->stream));
    VHX_HIP(c, hipMemsetAsync(&ctl->zero_key, 0xFF, sizeof(u64), c->stream));
    VHX_HIP(c, hipMemsetAsync(sm.binfo, 0, nn * 8, c->stream));
    VHX_HIP(c, hipMemsetAsync(sm.gmask, 0, nn * 8, c->stream));
    VHX_HIP(c, hipMemsetAsync(sm.bsrc, 0xFF, bsrc_cap * 4, c->stream));
    VHX_HIP(c, hipMemsetAsync(tab.keys, 0, TAB_KEYS_BYTES, c->stream));
    VHX_HIP(c, hipMemsetAsync(tab.vals, 0xFF, TAB_VALS_BYTES, c->stream));
    if ((rc = walk_and_claim(c, t, m, &ctl->w, true))) return rc;  // (resets ctl->w itself)

    const bool stamped = hipEventRecord(c->ev0, c->stream) == hipSuccess;  // vhx_sync reports the classify pass
    k_smp_classify<<<(unsigned)std::min<uint64_t>(nn, (uint64_t)c->cus * 32), 256, 0, c->stream>>>(t, m, in, sm, tab, ctl);
    c->timed = hipEventRecord(c->ev1, c->stream) == hipSuccess && stamped;
    if ((rc = scan_level<2>(c, sm.binfo, nn, false, sm.bfirst, &ctl->new_bricks))) return rc;
    k_smp_bfill<<<blocks_for(nn * 64), 256, 0, c->stream>>>(sm, ctl, d.node_count, bsrc_cap);
    k_smp_solid_compact<<<TAB_SLOTS / 256, 256, 0, c->stream>>>(tab, ctl);
    k_smp_solid_rank<<<PAL_CAP / 256, 256, 0, c->stream>>>(tab, ctl);
    VHX_HIP(c, hipGetLastError());

    // the one readback; the tree has only been read
    SimplifyCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.w.bad & BAD_INDEX)
        return fail(c, VHX_E_STATE, "vhx_simplify_tree: a child, brick or solid value index at or past its count");
    if (h.w.bad & BAD_TWICE) return fail(c, VHX_E_STATE, "vhx_simplify_tree: a node or Parted brick is reached twice");
    if (h.w.bad & BAD_DEEP) return fail(c, VHX_E_STATE, "vhx_simplify_tree: more than 8 node levels");
    if (h.w.end == 0 || h.w.end > nn || h.w.brick_total > nb || h.new_bricks > bsrc_cap)
        return fail(c, VHX_E_STATE, "vhx_simplify_tree: inconsistent counts");
    const uint64_t solids = (uint64_t)h.b.ncolors + (h.zero_key != ~0ull ? 1u : 0u);
    if (h.b.overflow || solids > MAX_COLORS || h.b.ncompact != h.b.ncolors)
        return fail(c, VHX_E_CAPACITY, "vhx_simplify_tree: more than 65,535 distinct Solid values");
    if (h.new_bricks >= (1ull << 31)) return fail(c, VHX_E_CAPACITY, "vhx_simplify_tree: 2^31 bricks or more");
    vhx_tree_desc ndesc = d;
    ndesc.node_count = h.w.end;
    ndesc.brick_count = (uint32_t)h.new_bricks;
    ndesc.solid_count = (uint32_t)solids;

    vhx::FreshTree fresh;
    if ((rc = vhx::alloc_fresh_tree(c, ndesc, &fresh, true))) return rc;
    k_smp_emit<<<blocks_for((uint64_t)ndesc.node_count * 64), 256, 0, c->stream>>>(
        t, m, sm, tab, ctl, ndesc.node_count, (uint32_t *)fresh.raw[VHX_BUF_NODE_TYPE].ptr,
        (u64 *)fresh.raw[VHX_BUF_NODE_OCBITS].ptr, (uint32_t *)fresh.raw[VHX_BUF_NODE_CHILDREN].ptr);
    hipError_t e = hipSuccess;
    if (ndesc.solid_count)
        e = hipMemcpyAsync(fresh.raw[VHX_BUF_SOLID_VALUES].ptr, tab.pal, (uint64_t)ndesc.solid_count * 4,
                           hipMemcpyDeviceToDevice, c->stream);
    if (ndesc.brick_count) {
        gather_bricks<true>(c, ts.raw[VHX_BUF_VOXELS].ptr, fresh.raw[VHX_BUF_VOXELS].ptr, (const u64 *)ts.brick_occ.ptr,
                            (u64 *)fresh.brick_occ.ptr, sm.bsrc, ndesc.brick_count, n3, ts.occ_words);
        if (n3 > 1)
            k_smp_uniform<<<(unsigned)std::min<uint64_t>(ndesc.node_count, (uint64_t)c->cus * 32), 256, 0, c->stream>>>(
                in, sm, ndesc.node_count, (uint32_t *)fresh.raw[VHX_BUF_VOXELS].ptr);
        if (e == hipSuccess && vhx::derive_fresh_occ(c, ndesc, fresh, sm.newb, ndesc.node_count) != VHX_OK) e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        vhx::free_fresh_tree(&fresh);
        return fail(c, VHX_E_HIP, std::string("vhx_simplify_tree: launch: ") + hipGetErrorString(e));
    }
    if ((rc = vhx::adopt_fresh_tree(c, ndesc, &fresh, true))) return rc;
    if (nodes_dropped) *nodes_dropped = d.node_count - ndesc.node_count;
    if (bricks_dropped) *bricks_dropped = d.brick_count > ndesc.brick_count ? d.brick_count - ndesc.brick_count : 0u;
    return ws.end();  // the next trace of every context of the tree waits for this write
}

}  // extern "C"
