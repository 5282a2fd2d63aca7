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
// The frontier walk, the brick pass and the gathers live in treepack.hpp, which vhx_simplify.hip shares; k_cmp_emit and
// the call are here.
// Nothing of the old tree is written. A node or brick is claimed by compare-and-swap from VHX_EMPTY, and a lost claim
// raises the "reached twice" flag; as in vhx_edit.hip the atomics feed only flags and claims, every index that reaches a
// buffer comes from a scan, and every global write is a plain store. Every index read from the tree is checked against
// its count before it is used as an address.
#include <algorithm>
#include <string>

#include "../../include/vhx.h"
// the frontier walk, the brick claims and the gathers are shared with vhx_simplify.hip; the colour table of buildtab.hpp
// is not used here
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "treepack.hpp"
#pragma clang diagnostic pop
#include "ctx.hpp"

namespace {

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
    Maps m;
    CompactCtl *ctl;
    if ((rc = ensure_maps(c, nn, nb, &m, &ctl))) return rc;
    const TreeStore &ts = *c->tree;
    const OldTree t{(const uint32_t *)ts.raw[VHX_BUF_NODE_TYPE].ptr, (const u64 *)ts.raw[VHX_BUF_NODE_OCBITS].ptr,
                    (const uint32_t *)ts.raw[VHX_BUF_NODE_CHILDREN].ptr, d.node_count, d.brick_count};
    if ((rc = walk_and_claim(c, t, m, ctl, false))) return rc;

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
    if (ndesc.brick_count)
        gather_bricks<false>(c, ts.raw[VHX_BUF_VOXELS].ptr, fresh.raw[VHX_BUF_VOXELS].ptr, (const u64 *)ts.brick_occ.ptr,
                             (u64 *)fresh.brick_occ.ptr, m.bsrc, ndesc.brick_count, n3, ts.occ_words);
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
