// vhx_compact_tree: the resident tree rewritten without its unreachable slots and in the builders' numbering, on the
// device and out of place. The image is a pure function of the old one (vhx_flat_compact, flatten.cpp,
// is the CPU reference): nodes breadth-first from the root, level by level in (parent's new index, sectant) order,
// Parted bricks in (owning node's new index, sectant) order.
//
//   frontier  k_cmp_front    per level, a wave per frontier node: the mask of its child entries (Internal nodes only)
//             k_scan_*       popcount scan over the new nodes so far: node i's first child is 1 + the entries before it
//             k_cmp_expand   a wave per frontier node, lane = sectant: the next level's old_of / new_of
//             k_cmp_advance  the next frontier's bounds, on the device: no readback between levels
//   bricks    k_cmp_bmask    per new node the mask of its Parted entries (a Leaf's 64, a UniformLeaf's entry 0)
//             k_scan_*       the node's first new brick
//             k_cmp_bfill    brick_src[new brick] = old brick
//   -- one readback of the counters; a malformed tree is refused here; the new buffers are allocated --
//   emit      k_cmp_emit     types, occupancy and the 64 entries of every new node, remapped
//   gather    k_cmp_gather   the hot pass, driven from the destination: thread w owns 16-byte words of the new voxels,
//                            finds their brick j and loads from brick_src[j] (k_cmp_gather1: bricks of one cell);
//             k_cmp_gather_occ  the bricks' occupancy bitmaps by the same map (a bitmap is a function of the cells and
//                            the palettes, and neither changes)
//   derive    headers and child records by the tree unit's own kernels (adopt_fresh_tree)
//
// Nothing of the old tree is written. A node or brick is claimed by compare-and-swap from VHX_EMPTY, and a lost claim
// raises the "reached twice" flag; as in vhx_edit.hip the atomics feed only flags and claims, every index that reaches a
// buffer comes from a scan, and every global write is a plain store. Every index read from the tree is checked against
// its count before it is used as an address.
#include <algorithm>
#include <string>

#include "../../include/vhx.h"
// the scans are used here; the colour table of the same header is not
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "buildtab.hpp"
#pragma clang diagnostic pop
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
__global__ __launch_bounds__(256) void k_cmp_front(OldTree t, Maps m, const CompactCtl *ctl) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = ctl->begin + (gid >> 6);
    if (i >= ctl->end) return;  // the whole wave
    const uint32_t o = m.old_of[i];
    bool has = false;
    if (o < t.node_count && t.type[o] == VHX_NODE_INTERNAL) has = t.children[(uint64_t)o * 64u + lane] != VHX_EMPTY;
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

// one thread per (new node, sectant); runs only for a tree that passed the checks
__global__ __launch_bounds__(256) void k_cmp_emit(OldTree t, Maps m, uint32_t nodes, uint32_t *type, u64 *ocbits,
                                                  uint32_t *children) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = gid >> 6;
    const uint32_t s = (uint32_t)gid & 63u;
    if (i >= nodes) return;
    const uint32_t o = m.old_of[i];
    const uint32_t ty = t.type[o];
    if (s == 0) {
        type[i] = ty;
        ocbits[i] = t.ocbits[o];
    }
    uint32_t e = t.children[(uint64_t)o * 64u + s];
    if (ty == VHX_NODE_INTERNAL) {
        if (e != VHX_EMPTY) e = m.new_of[e];
    } else {
        const u64 mask = m.bmask[i];
        if ((mask >> s) & 1ull) e = (uint32_t)m.bfirst[i] + (uint32_t)__popcll(mask & ((1ull << s) - 1ull));
    }
    children[gid] = e;
}

// The gather, driven from the destination. A workgroup owns GATHER_ITEMS * 256 consecutive 16-byte words of the new
// voxels: its stores are contiguous, and its loads are whole bricks (1 << lgw words each). The loads of a thread are
// issued before its stores.
constexpr uint32_t GATHER_ITEMS = 4;
__global__ __launch_bounds__(256) void k_cmp_gather(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                    const uint32_t *__restrict__ bsrc, uint64_t w0, uint64_t nwords,
                                                    uint32_t lgw) {
    const uint64_t base = w0 + (uint64_t)blockIdx.x * (256u * GATHER_ITEMS) + threadIdx.x;
    const uint64_t kmask = (1ull << lgw) - 1ull;
    uint4 v[GATHER_ITEMS];
#pragma unroll
    for (uint32_t u = 0; u < GATHER_ITEMS; ++u) {
        const uint64_t w = base + 256ull * u;
        if (w < nwords) v[u] = src[((uint64_t)bsrc[w >> lgw] << lgw) + (w & kmask)];
    }
#pragma unroll
    for (uint32_t u = 0; u < GATHER_ITEMS; ++u) {
        const uint64_t w = base + 256ull * u;
        if (w < nwords) dst[w] = v[u];
    }
}

// brick_dim 1: a brick is one dword
__global__ __launch_bounds__(256) void k_cmp_gather1(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst,
                                                     const uint32_t *__restrict__ bsrc, uint32_t bricks) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < bricks) dst[j] = src[bsrc[j]];
}

// the bitmaps: 1 << lgo words of 64 bits per brick
__global__ __launch_bounds__(256) void k_cmp_gather_occ(const u64 *__restrict__ src, u64 *__restrict__ dst,
                                                        const uint32_t *__restrict__ bsrc, uint64_t w0, uint64_t nwords,
                                                        uint32_t lgo) {
    const uint64_t w = w0 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    dst[w] = src[((uint64_t)bsrc[w >> lgo] << lgo) + (w & ((1ull << lgo) - 1ull))];
}

uint32_t lg2(uint64_t v) {
    uint32_t l = 0;
    while ((1ull << l) < v) ++l;
    return l;
}

}  // namespace

extern "C" {

int vhx_compact_tree(vhx_ctx *c, uint32_t *nodes_dropped, uint32_t *bricks_dropped) {
    if (!c) return VHX_E_INVALID_ARG;
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_compact_tree on a shared context: compact through the owner");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_compact_tree before vhx_upload_tree");
    if (c->tree->mips_on) return fail(c, VHX_E_STATE, "vhx_compact_tree while node MIPs are set");
    const vhx_tree_desc d = c->tree->desc;
    const uint64_t nn = d.node_count, nb = d.brick_count;
    const uint64_t n3 = (uint64_t)d.brick_dim * d.brick_dim * d.brick_dim;

    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    vhx::WriteScope ws(c);  // frames in flight on the tree's other contexts finish reading it first
    int rc = ws.rc;
    if (rc) return rc;
    vhx_ctx::CompactScratch &cs = c->compact;
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
    const Maps m{(uint32_t *)cs.new_of.ptr, (uint32_t *)cs.old_of.ptr, (u64 *)cs.nmask.ptr, (u64 *)cs.nrank.ptr,
                 (u64 *)cs.bmask.ptr,       (u64 *)cs.bfirst.ptr,      (uint32_t *)cs.bnew.ptr, (uint32_t *)cs.bsrc.ptr};
    CompactCtl *ctl = (CompactCtl *)cs.ctl.ptr;
    const TreeStore &ts = *c->tree;
    const OldTree t{(const uint32_t *)ts.raw[VHX_BUF_NODE_TYPE].ptr, (const u64 *)ts.raw[VHX_BUF_NODE_OCBITS].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_NODE_CHILDREN].ptr, d.node_count, d.brick_count};
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
        k_cmp_front<<<blocks_for(waves * 64), 256, 0, c->stream>>>(t, m, ctl);
        if ((rc = scan_level<1>(c, m.nmask, scan_n, false, m.nrank, &ctl->scan_total))) return rc;
        k_cmp_expand<<<blocks_for(waves * 64), 256, 0, c->stream>>>(t, m, ctl);
        k_cmp_advance<<<1, 1, 0, c->stream>>>(ctl, d.node_count, lv + 1 == MAX_LEVELS ? 1 : 0);
        if (level_cap >= nn) level_cap = nn; else level_cap *= 64;
        upto_cap = std::min(nn, upto_cap + level_cap);
    }
    k_cmp_bmask<<<blocks_for(nn * 64), 256, 0, c->stream>>>(t, m, ctl);
    if ((rc = scan_level<1>(c, m.bmask, nn, false, m.bfirst, &ctl->brick_total))) return rc;
    k_cmp_bfill<<<blocks_for(nn * 64), 256, 0, c->stream>>>(t, m, ctl);
    VHX_HIP(c, hipGetLastError());

    // the one readback; the tree has only been read
    CompactCtl h;
    VHX_HIP(c, hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    if (h.bad & BAD_INDEX)
        return fail(c, VHX_E_STATE, "vhx_compact_tree: a child or brick index at or past its count");
    if (h.bad & BAD_TWICE) return fail(c, VHX_E_STATE, "vhx_compact_tree: a node or Parted brick is reached twice");
    if (h.bad & BAD_DEEP) return fail(c, VHX_E_STATE, "vhx_compact_tree: more than 8 node levels");
    if (h.end == 0 || h.end > nn || h.brick_total > nb)
        return fail(c, VHX_E_STATE, "vhx_compact_tree: inconsistent counts");
    vhx_tree_desc ndesc = d;
    ndesc.node_count = h.end;
    ndesc.brick_count = (uint32_t)h.brick_total;

    vhx::FreshTree fresh;
    if ((rc = vhx::alloc_fresh_tree(c, ndesc, &fresh))) return rc;
    k_cmp_emit<<<blocks_for((uint64_t)ndesc.node_count * 64), 256, 0, c->stream>>>(
        t, m, ndesc.node_count, (uint32_t *)fresh.raw[VHX_BUF_NODE_TYPE].ptr, (u64 *)fresh.raw[VHX_BUF_NODE_OCBITS].ptr,
        (uint32_t *)fresh.raw[VHX_BUF_NODE_CHILDREN].ptr);
    const bool stamped = hipEventRecord(c->ev0, c->stream) == hipSuccess;  // vhx_sync reports the gather's device time
    if (ndesc.brick_count) {
        const void *vsrc = ts.raw[VHX_BUF_VOXELS].ptr;
        void *vdst = fresh.raw[VHX_BUF_VOXELS].ptr;
        if (n3 < 4) {
            k_cmp_gather1<<<blocks_for(ndesc.brick_count), 256, 0, c->stream>>>((const uint32_t *)vsrc, (uint32_t *)vdst,
                                                                                m.bsrc, ndesc.brick_count);
        } else {
            const uint32_t lgw = lg2(n3 / 4);
            const uint64_t nwords = (uint64_t)ndesc.brick_count << lgw, per_block = 256ull * GATHER_ITEMS;
            const uint64_t chunk = per_block << 22;  // launches of at most 2^22 workgroups
            for (uint64_t w0 = 0; w0 < nwords; w0 += chunk) {
                const uint64_t n = std::min(chunk, nwords - w0);
                k_cmp_gather<<<(unsigned)((n + per_block - 1) / per_block), 256, 0, c->stream>>>(
                    (const uint4 *)vsrc, (uint4 *)vdst, m.bsrc, w0, nwords, lgw);
            }
        }
        const uint32_t lgo = lg2(ts.occ_words);
        const uint64_t owords = (uint64_t)ndesc.brick_count << lgo, ochunk = 1ull << 30;
        for (uint64_t w0 = 0; w0 < owords; w0 += ochunk)
            k_cmp_gather_occ<<<blocks_for(std::min(ochunk, owords - w0)), 256, 0, c->stream>>>(
                (const u64 *)ts.brick_occ.ptr, (u64 *)fresh.brick_occ.ptr, m.bsrc, w0, owords, lgo);
    }
    {
        hipError_t e = hipEventRecord(c->ev1, c->stream);
        c->timed = stamped && e == hipSuccess;
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            vhx::free_fresh_tree(&fresh);
            return fail(c, VHX_E_HIP, std::string("vhx_compact_tree: launch: ") + hipGetErrorString(e));
        }
    }
    if ((rc = vhx::adopt_fresh_tree(c, ndesc, &fresh))) return rc;
    if (nodes_dropped) *nodes_dropped = d.node_count - ndesc.node_count;
    if (bricks_dropped) *bricks_dropped = d.brick_count - ndesc.brick_count;
    return ws.end();  // the next trace of every context of the tree waits for this write
}

}  // extern "C"
