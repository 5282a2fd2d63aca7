// libvhx device side, tree unit: the device copy of a tree and everything derived from it.
//
// Kernels
//   k_brick_occ_ballot / k_brick_occ_small  brick occupancy bitmaps from pix_points_to_empty (src/boxtree/node.rs:311-333)
//   k_brick_occ_list  the same for the bricks a list names (vhx_simplify_tree's new bricks)
//   k_pack_hdr        node type + occupied_bits -> one 16-byte record per node
//   k_child_rec       DevTree::child_rec (brick_dim <= 4): one record per child entry
//   k_scatter_ranges  ranged writes: staged pieces copied to their device addresses
// Host side: upload (vhx_upload_tree*, receive_tree), ranged updates (vhx_update_range(s)), node MIPs, read-back of the
// derived layout, content-preserving growth of the buffers for vhx_write_dense (grow_tree), the buffer swap of
// vhx_compact_tree and vhx_simplify_tree (alloc_fresh_tree, derive_fresh_occ, adopt_fresh_tree), vhx_tree_orphans. Launches no kernel of another unit; the trace unit (vhx_device.hip) calls refresh_child_rec.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vhx.h"
#include "ctx.hpp"
#include "treewalk.hpp"

using namespace vhx;

// ------------------------------------------------------------------------------------------------ upload kernels
// bd^3 >= 64: one lane per cell, the wave's ballot is one 64-bit occupancy word
__global__ void __launch_bounds__(256) k_brick_occ_ballot(const uint32_t *__restrict__ vox, uint64_t ncells,
                                                          uint64_t cell0, const uint32_t *__restrict__ color,
                                                          uint32_t ncolor, const uint32_t *__restrict__ data,
                                                          uint32_t ndata, uint64_t *__restrict__ words) {
    const uint64_t i = cell0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < cell0 + ncells;
    const bool full = in && !cell_empty(vox[in ? i : cell0], color, ncolor, data, ndata);
    const uint64_t m = __ballot(full);
    if ((threadIdx.x & 63u) == 0 && in) words[i >> 6] = m;
}

// bd^3 < 64 (bd = 1, 2): one lane per brick
__global__ void __launch_bounds__(256) k_brick_occ_small(const uint32_t *__restrict__ vox, uint32_t nbricks,
                                                         uint32_t brick0, uint32_t n3,
                                                         const uint32_t *__restrict__ color, uint32_t ncolor,
                                                         const uint32_t *__restrict__ data, uint32_t ndata,
                                                         uint64_t *__restrict__ words) {
    const uint32_t b = brick0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= brick0 + nbricks) return;
    uint64_t m = 0;
    for (uint32_t c = 0; c < n3; ++c)
        if (!cell_empty(vox[(uint64_t)b * n3 + c], color, ncolor, data, ndata)) m |= 1ull << c;
    words[b] = m;
}

// ... of the bricks a list names (the bricks a simplification wrote anew instead of gathering them with their bitmaps): a
// wave per list entry, VHX_EMPTY entries skipped; bit order as the two kernels above
__global__ void __launch_bounds__(256) k_brick_occ_list(const uint32_t *__restrict__ vox,
                                                        const uint32_t *__restrict__ list, uint32_t n, uint32_t n3,
                                                        const uint32_t *__restrict__ color, uint32_t ncolor,
                                                        const uint32_t *__restrict__ data, uint32_t ndata,
                                                        uint64_t *__restrict__ words) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    if ((gid >> 6) >= n) return;  // the whole wave
    const uint32_t b = list[gid >> 6];
    if (b == VHX_EMPTY) return;
    if (n3 < 64) {
        const uint32_t v = vox[(uint64_t)b * n3 + (lane < n3 ? lane : 0u)];
        const bool full = lane < n3 && !cell_empty(v, color, ncolor, data, ndata);
        const uint64_t m = __ballot(full);
        if (lane == 0) words[b] = m;
        return;
    }
    const uint32_t nw = n3 >> 6;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint64_t m = __ballot(!cell_empty(vox[(uint64_t)b * n3 + w * 64u + lane], color, ncolor, data, ndata));
        if (lane == 0) words[(uint64_t)b * nw + w] = m;
    }
}

// DevTree::child_rec for brick_dim <= 4: one record per child entry. Entries [e0, e1) are visited; with sel, only the
// entries of nodes [node_lo, node_hi) and those holding a Parted brick in [brick_lo, brick_hi) are rewritten (a ranged
// update: the records of written nodes and of the nodes whose bricks were written)
struct RecSel {
    uint32_t sel, node_lo, node_hi, brick_lo, brick_hi;
};
__global__ void __launch_bounds__(256) k_child_rec(const uint32_t *__restrict__ type,
                                                   const uint32_t *__restrict__ children,
                                                   const uint64_t *__restrict__ words, uint32_t brick_count,
                                                   uint64_t e0, uint64_t e1, RecSel s, uint4 *__restrict__ rec) {
    const uint64_t i = e0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e1) return;
    const uint32_t node = (uint32_t)(i >> 6);
    const uint32_t ty = type[node];
    const bool uniform = ty == VHX_NODE_UNIFORM_LEAF;
    const uint32_t v = children[uniform ? (i & ~63ull) : i];
    const bool parted = (uniform || ty == VHX_NODE_LEAF) && v != VHX_EMPTY && (v & VHX_SOLID_BIT) == 0 && v < brick_count;
    if (s.sel && !(node >= s.node_lo && node < s.node_hi) && !(parted && v >= s.brick_lo && v < s.brick_hi)) return;
    const uint64_t o = parted ? words[v] : 0ull;
    rec[i] = make_uint4(v, (uint32_t)o, (uint32_t)(o >> 32), 0u);
}

// Ranged writes: job j copies `words` 32-bit words from the staging buffer at src_off to the device address dst (a
// range cut into pieces of at most 16 KiB, one workgroup per piece)
struct UpdJob {
    uint64_t dst, src_off;
    uint32_t words, pad0;
    uint64_t pad1;
};
#define UPD_PIECE_BYTES 16384u
__global__ void __launch_bounds__(256) k_scatter_ranges(const uint8_t *__restrict__ stage, uint32_t j0, uint32_t j1) {
    const UpdJob *jobs = (const UpdJob *)stage;
    for (uint32_t j = j0 + blockIdx.x; j < j1; j += gridDim.x) {
        const UpdJob jb = jobs[j];
        const uint32_t *src = (const uint32_t *)(stage + jb.src_off);
        uint32_t *dst = (uint32_t *)jb.dst;
        for (uint32_t w = threadIdx.x; w < jb.words; w += blockDim.x) dst[w] = src[w];
    }
}

__global__ void __launch_bounds__(256) k_pack_hdr(const uint32_t *__restrict__ type, const uint64_t *__restrict__ occ,
                                                  uint32_t n0, uint32_t n, uint4 *__restrict__ hdr) {
    const uint32_t i = n0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n0 + n) return;
    const uint64_t o = occ[i];
    hdr[i] = make_uint4((uint32_t)o, (uint32_t)(o >> 32), type[i], 0u);
}

void vhx::pack_counts(const vhx_tree_desc &d, uint32_t counts[8]) {
    const uint32_t v[8] = {d.boxtree_size, d.brick_dim, d.node_count, d.brick_count,
                           d.solid_count, d.color_count, d.data_count, 0};
    std::memcpy(counts, v, sizeof(v));
}

vhx_tree_desc vhx::unpack_counts(const uint32_t counts[8]) {
    vhx_tree_desc d{};
    d.boxtree_size = counts[0];
    d.brick_dim = counts[1];
    d.node_count = counts[2];
    d.brick_count = counts[3];
    d.solid_count = counts[4];
    d.color_count = counts[5];
    d.data_count = counts[6];
    return d;
}

uint64_t vhx::elem_size(int id) {
    switch (id) {
        case VHX_BUF_NODE_OCBITS: return 8;
        default: return 4;
    }
}
uint64_t vhx::elem_count(const vhx_tree_desc &d, int id) {
    const uint64_t n3 = (uint64_t)d.brick_dim * d.brick_dim * d.brick_dim;
    switch (id) {
        case VHX_BUF_NODE_TYPE: return d.node_count;
        case VHX_BUF_NODE_OCBITS: return d.node_count;
        case VHX_BUF_NODE_CHILDREN: return (uint64_t)d.node_count * 64;
        case VHX_BUF_VOXELS: return (uint64_t)d.brick_count * n3;
        case VHX_BUF_SOLID_VALUES: return d.solid_count;
        case VHX_BUF_COLOR_PALETTE: return d.color_count;
        case VHX_BUF_DATA_PALETTE: return d.data_count;
    }
    return 0;
}

static int rebuild_hdr(vhx_ctx *c, uint32_t n0, uint32_t n) {
    if (n == 0) return VHX_OK;
    k_pack_hdr<<<(n + 255) / 256, 256, 0, c->stream>>>((const uint32_t *)c->tree->raw[VHX_BUF_NODE_TYPE].ptr,
                                                       (const uint64_t *)c->tree->raw[VHX_BUF_NODE_OCBITS].ptr, n0, n,
                                                       (uint4 *)c->tree->hdr.ptr);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}

static bool has_child_rec(const vhx_ctx *c) {
    const uint32_t bd = c->tree->desc.brick_dim;
    return bd * bd * bd <= 64;
}

// DevTree::child_rec depends on node types, children and brick occupancy: updates mark it stale and the next trace
// rebuilds it whole (one pass over the child entries, ~n_nodes * 64 * 24 bytes)
int vhx::refresh_child_rec(vhx_ctx *c) {
    if (!has_child_rec(c) || !c->tree->child_rec_stale) return VHX_OK;
    const uint64_t n = (uint64_t)c->tree->desc.node_count * 64;
    k_child_rec<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(
        (const uint32_t *)c->tree->raw[VHX_BUF_NODE_TYPE].ptr, (const uint32_t *)c->tree->raw[VHX_BUF_NODE_CHILDREN].ptr,
        (const uint64_t *)c->tree->brick_occ.ptr, c->tree->desc.brick_count, 0, n, RecSel{0, 0, 0, 0, 0},
        (uint4 *)c->tree->child_rec.ptr);
    VHX_HIP(c, hipGetLastError());
    c->tree->child_rec_stale = false;
    return VHX_OK;
}

// The child records of nodes [node_lo, node_hi) and of the nodes holding Parted bricks [brick_lo, brick_hi) (either
// range may be empty): a pass over the written nodes' entries, or over every child entry when bricks were written (the
// brick -> holder relation lives only in the children array; reading it is 256 B per node, the records are 1 KB).
static int refresh_child_rec_sel(vhx_ctx *c, uint32_t node_lo, uint32_t node_hi, uint32_t brick_lo, uint32_t brick_hi) {
    if (!has_child_rec(c) || c->tree->child_rec_stale) return VHX_OK;  // a stale buffer is rebuilt whole anyway
    const bool bricks = brick_lo < brick_hi, nodes = node_lo < node_hi;
    if (!bricks && !nodes) return VHX_OK;
    const uint64_t e0 = bricks ? 0 : (uint64_t)node_lo * 64, e1 = bricks ? (uint64_t)c->tree->desc.node_count * 64
                                                                           : (uint64_t)node_hi * 64;
    k_child_rec<<<(unsigned)((e1 - e0 + 255) / 256), 256, 0, c->stream>>>(
        (const uint32_t *)c->tree->raw[VHX_BUF_NODE_TYPE].ptr, (const uint32_t *)c->tree->raw[VHX_BUF_NODE_CHILDREN].ptr,
        (const uint64_t *)c->tree->brick_occ.ptr, c->tree->desc.brick_count, e0, e1,
        RecSel{1, node_lo, node_hi, brick_lo, brick_hi}, (uint4 *)c->tree->child_rec.ptr);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}

static int rebuild_occ(vhx_ctx *c, uint32_t brick0, uint32_t nbricks) {
    if (nbricks == 0) return VHX_OK;
    const uint32_t bd = c->tree->desc.brick_dim;
    const uint32_t n3 = bd * bd * bd;
    const uint32_t *vox = (const uint32_t *)c->tree->raw[VHX_BUF_VOXELS].ptr;
    const uint32_t *col = (const uint32_t *)c->tree->raw[VHX_BUF_COLOR_PALETTE].ptr;
    const uint32_t *dat = (const uint32_t *)c->tree->raw[VHX_BUF_DATA_PALETTE].ptr;
    if (n3 >= 64) {
        const uint64_t cell0 = (uint64_t)brick0 * n3, ncells = (uint64_t)nbricks * n3;
        // grid-stride chunks keep gridDim.x within range for multi-GB voxel buffers
        const uint64_t chunk = 1ull << 30;
        for (uint64_t s = 0; s < ncells; s += chunk) {
            const uint64_t n = std::min(chunk, ncells - s);
            k_brick_occ_ballot<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(
                vox, n, cell0 + s, col, c->tree->desc.color_count, dat, c->tree->desc.data_count, (uint64_t *)c->tree->brick_occ.ptr);
            VHX_HIP(c, hipGetLastError());
        }
    } else {
        k_brick_occ_small<<<(nbricks + 255) / 256, 256, 0, c->stream>>>(vox, nbricks, brick0, n3, col,
                                                                         c->tree->desc.color_count, dat, c->tree->desc.data_count,
                                                                         (uint64_t *)c->tree->brick_occ.ptr);
        VHX_HIP(c, hipGetLastError());
    }
    return VHX_OK;
}

int vhx::rederive_bricks(vhx_ctx *c) {
    int rc = rebuild_occ(c, 0, c->tree->desc.brick_count);
    if (rc || !has_child_rec(c)) return rc;
    c->tree->child_rec_stale = true;
    return refresh_child_rec(c);
}

int vhx::derive_fresh_occ(vhx_ctx *c, const vhx_tree_desc &counts, const FreshTree &fresh, const uint32_t *list,
                          uint32_t n) {
    if (counts.brick_count == 0 || n == 0) return VHX_OK;
    const TreeStore &ts = *c->tree;
    const uint32_t bd = ts.desc.brick_dim;
    k_brick_occ_list<<<(unsigned)(((uint64_t)n * 64 + 255) / 256), 256, 0, c->stream>>>(
        (const uint32_t *)fresh.raw[VHX_BUF_VOXELS].ptr, list, n, bd * bd * bd,
        (const uint32_t *)ts.raw[VHX_BUF_COLOR_PALETTE].ptr, ts.desc.color_count,  // the palettes do not change
        (const uint32_t *)ts.raw[VHX_BUF_DATA_PALETTE].ptr, ts.desc.data_count, (uint64_t *)fresh.brick_occ.ptr);
    VHX_HIP(c, hipGetLastError());
    return VHX_OK;
}

int vhx::alloc_tree(vhx_ctx *c, const vhx_tree_desc *t) {
    const uint32_t bd = t->brick_dim;
    if (t->node_count == 0 || bd == 0 || t->boxtree_size == 0 || (bd & (bd - 1)) != 0 || bd > 32 ||
        (t->boxtree_size & (t->boxtree_size - 1)) != 0 || t->boxtree_size > (1u << 24))
        return fail(c, VHX_E_INVALID_ARG, "vhx_upload_tree: invalid sizes");
    VHX_HIP(c, hipSetDevice(c->device));
    // a buffer that grows is freed and reallocated: the frames in flight on the tree's contexts (which c's stream
    // already waits for, write_begin) finish first
    bool grows = false;
    for (int id = 0; id < 7; ++id) grows |= c->tree->raw[id].bytes < elem_count(*t, id) * elem_size(id);
    if (grows && c->stream) VHX_HIP(c, hipStreamSynchronize(c->stream));
    c->tree->uploaded = false;
    c->tree->mips_on = false;  // a new tree has no MIPs until vhx_set_node_mips
    c->tree->orphan_nodes = c->tree->orphan_bricks = 0;
    for (int id = 0; id < 7; ++id) {
        int rc = ensure(c, c->tree->raw[id], elem_count(*t, id) * elem_size(id));
        if (rc) return rc;
    }
    c->tree->desc = *t;
    for (const void **q : {(const void **)&c->tree->desc.node_type, (const void **)&c->tree->desc.node_ocbits,
                           (const void **)&c->tree->desc.node_children, (const void **)&c->tree->desc.voxels,
                           (const void **)&c->tree->desc.solid_values, (const void **)&c->tree->desc.color_palette,
                           (const void **)&c->tree->desc.data_palette})
        *q = nullptr;  // only the counts are kept
    return VHX_OK;
}

int vhx::grow_tree(vhx_ctx *c, const vhx_tree_desc *t) {
    TreeStore &ts = *c->tree;
    const vhx_tree_desc &d = ts.desc;
    struct Want {
        DevBuf *b;
        uint64_t used, need;
    } want[10];
    uint32_t n = 0;
    for (int id = 0; id < 7; ++id)
        want[n++] = {&ts.raw[id], elem_count(d, id) * elem_size(id), elem_count(*t, id) * elem_size(id)};
    want[n++] = {&ts.hdr, (uint64_t)d.node_count * 16, (uint64_t)t->node_count * 16};
    want[n++] = {&ts.brick_occ, (uint64_t)d.brick_count * ts.occ_words * 8, (uint64_t)t->brick_count * ts.occ_words * 8};
    if (has_child_rec(c)) want[n++] = {&ts.child_rec, (uint64_t)d.node_count * 1024, (uint64_t)t->node_count * 1024};
    void *old[10];
    uint32_t nold = 0;
    for (uint32_t i = 0; i < n; ++i) {
        DevBuf &b = *want[i].b;
        if (b.ptr && b.bytes >= want[i].need) continue;
        const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(want[i].need, b.bytes + b.bytes / 2), 16);
        void *p = nullptr;
        VHX_HIP(c, hipMalloc(&p, cap));
        if (b.ptr && want[i].used)
            VHX_HIP(c, hipMemcpyAsync(p, b.ptr, std::min(want[i].used, b.bytes), hipMemcpyDeviceToDevice, c->stream));
        if (b.ptr) old[nold++] = b.ptr;
        b.ptr = p;
        b.bytes = cap;
    }
    if (nold) {
        VHX_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < nold; ++i) VHX_HIP(c, hipFree(old[i]));
    }
    return VHX_OK;
}

int vhx::finish_upload(vhx_ctx *c) {
    const vhx_tree_desc *t = &c->tree->desc;
    const uint64_t bd = t->brick_dim, n3 = bd * bd * bd;
    c->tree->occ_words = n3 >= 64 ? (uint32_t)(n3 / 64) : 1u;
    int rc = ensure(c, c->tree->hdr, (uint64_t)t->node_count * 16);
    if (rc) return rc;
    rc = ensure(c, c->tree->brick_occ, (uint64_t)t->brick_count * c->tree->occ_words * 8);
    if (rc) return rc;
    if ((rc = rebuild_hdr(c, 0, t->node_count))) return rc;
    if ((rc = rebuild_occ(c, 0, t->brick_count))) return rc;
    if (has_child_rec(c)) {
        if ((rc = ensure(c, c->tree->child_rec, (uint64_t)t->node_count * 64 * 16))) return rc;
        c->tree->child_rec_stale = true;
        if ((rc = refresh_child_rec(c))) return rc;
    }
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    c->tree->uploaded = true;
    return VHX_OK;
}

uint64_t vhx::raw_bytes(const vhx_tree_desc &counts, int id) {
    const uint64_t b = elem_count(counts, id) * elem_size(id);
    return b ? b : 16;
}

void vhx::free_fresh_tree(FreshTree *f) {
    DevBuf *all[10] = {&f->raw[0], &f->raw[1], &f->raw[2], &f->raw[3], &f->raw[4],
                       &f->raw[5], &f->raw[6], &f->hdr,    &f->brick_occ, &f->child_rec};
    for (DevBuf *b : all) {
        if (b->ptr) (void)hipFree(b->ptr);
        *b = DevBuf{};
    }
}

int vhx::alloc_fresh_tree(vhx_ctx *c, const vhx_tree_desc &counts, FreshTree *f, bool new_solids) {
    const TreeStore &ts = *c->tree;
    struct Want {
        DevBuf *b;
        uint64_t bytes;
    } want[10];
    uint32_t n = 0;
    for (int id = 0; id < 7; ++id) {
        const bool palette = id >= VHX_BUF_SOLID_VALUES;
        const bool fresh = new_solids && id == VHX_BUF_SOLID_VALUES;
        if (palette && !fresh && ts.raw[id].bytes <= raw_bytes(counts, id)) continue;  // kept as it is
        want[n++] = {&f->raw[id], raw_bytes(counts, id)};
    }
    const uint64_t occ_bytes = (uint64_t)counts.brick_count * ts.occ_words * 8;
    want[n++] = {&f->hdr, (uint64_t)counts.node_count * 16};
    want[n++] = {&f->brick_occ, occ_bytes ? occ_bytes : 16};
    if (has_child_rec(c)) want[n++] = {&f->child_rec, (uint64_t)counts.node_count * 64 * 16};
    for (uint32_t i = 0; i < n; ++i) {
        const hipError_t e = hipMalloc(&want[i].b->ptr, want[i].bytes);
        if (e != hipSuccess) {
            want[i].b->ptr = nullptr;
            free_fresh_tree(f);
            (void)hipGetLastError();
            return fail(c, VHX_E_HIP,
                        std::string("vhx_compact_tree / vhx_simplify_tree: hipMalloc: ") + hipGetErrorString(e));
        }
        want[i].b->bytes = want[i].bytes;
    }
    return VHX_OK;
}

int vhx::adopt_fresh_tree(vhx_ctx *c, const vhx_tree_desc &counts, FreshTree *f, bool new_solids) {
    TreeStore &ts = *c->tree;
    for (int id = VHX_BUF_SOLID_VALUES; id < 7; ++id) {
        const uint64_t used = elem_count(counts, id) * elem_size(id);
        if (f->raw[id].ptr && used && !(new_solids && id == VHX_BUF_SOLID_VALUES))
            VHX_HIP(c, hipMemcpyAsync(f->raw[id].ptr, ts.raw[id].ptr, used, hipMemcpyDeviceToDevice, c->stream));
    }
    for (int id = 0; id < 7; ++id)
        if (f->raw[id].ptr) std::swap(ts.raw[id], f->raw[id]);
    std::swap(ts.hdr, f->hdr);
    std::swap(ts.brick_occ, f->brick_occ);
    if (has_child_rec(c)) std::swap(ts.child_rec, f->child_rec);
    ts.desc.node_count = counts.node_count;
    ts.desc.brick_count = counts.brick_count;
    if (new_solids) ts.desc.solid_count = counts.solid_count;
    ts.orphan_nodes = ts.orphan_bricks = 0;
    int rc = rebuild_hdr(c, 0, counts.node_count);
    if (!rc && has_child_rec(c)) {
        ts.child_rec_stale = true;
        rc = refresh_child_rec(c);
    }
    // the frames in flight read the old buffers, now in *f: c's stream waits for them (write_begin)
    const hipError_t e = hipStreamSynchronize(c->stream);
    free_fresh_tree(f);
    if (rc) return rc;
    VHX_HIP(c, e);
    return VHX_OK;
}

extern "C" {

int vhx_upload_tree(vhx_ctx *c, const vhx_tree_desc *t) {
    if (!c || !t) return VHX_E_INVALID_ARG;
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_upload_tree on a shared context: upload through the owner");
    const void *src[7] = {t->node_type, t->node_ocbits, t->node_children, t->voxels,
                          t->solid_values, t->color_palette, t->data_palette};
    for (int id = 0; id < 7; ++id)
        if (elem_count(*t, id) && !src[id])
            return fail(c, VHX_E_INVALID_ARG, "vhx_upload_tree: null array with non-zero count");
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    WriteScope ws(c);  // frames in flight on the tree's other contexts finish reading it first
    int rc = ws.rc;
    if (!rc) rc = alloc_tree(c, t);
    if (rc) return rc;
    for (int id = 0; id < 7; ++id) {
        const uint64_t bytes = elem_count(*t, id) * elem_size(id);
        if (bytes) VHX_HIP(c, hipMemcpyAsync(c->tree->raw[id].ptr, src[id], bytes, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = finish_upload(c))) return rc;
    return ws.end();
}

}  // extern "C"

int vhx::receive_tree(vhx_ctx *c, const vhx_tree_desc &counts,
                      int (*fill)(void *, void *const[7], const uint64_t[7]), void *arg) {
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    WriteScope ws(c);
    int rc = ws.rc;
    if (!rc) rc = alloc_tree(c, &counts);
    if (rc) return rc;
    void *dst[7];
    uint64_t bytes[7];
    for (int id = 0; id < 7; ++id) {
        dst[id] = c->tree->raw[id].ptr;
        bytes[id] = elem_count(c->tree->desc, id) * elem_size(id);
    }
    if ((rc = fill(arg, dst, bytes))) return rc;  // the transfers, enqueued on c's stream
    if ((rc = finish_upload(c))) return rc;       // derived layout from the received buffers (synchronises)
    return ws.end();
}

extern "C" {

static int fill_device_copies(void *arg, void *const dst[7], const uint64_t bytes[7]) {
    const std::pair<vhx_ctx *, const vhx_tree_desc *> &a = *(const std::pair<vhx_ctx *, const vhx_tree_desc *> *)arg;
    vhx_ctx *c = a.first;
    const void *src[7] = {a.second->node_type,  a.second->node_ocbits,    a.second->node_children, a.second->voxels,
                          a.second->solid_values, a.second->color_palette, a.second->data_palette};
    for (int id = 0; id < 7; ++id)
        if (bytes[id]) VHX_HIP(c, hipMemcpyAsync(dst[id], src[id], bytes[id], hipMemcpyDefault, c->stream));
    return VHX_OK;
}

int vhx_upload_tree_device(vhx_ctx *c, const vhx_tree_desc *t) {
    if (!c || !t) return VHX_E_INVALID_ARG;
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_upload_tree_device on a shared context: upload through the owner");
    const void *src[7] = {t->node_type, t->node_ocbits, t->node_children, t->voxels,
                          t->solid_values, t->color_palette, t->data_palette};
    for (int id = 0; id < 7; ++id)
        if (elem_count(*t, id) && !src[id])
            return fail(c, VHX_E_INVALID_ARG, "vhx_upload_tree_device: null array with non-zero count");
    std::pair<vhx_ctx *, const vhx_tree_desc *> arg{c, t};
    return receive_tree(c, *t, fill_device_copies, &arg);
}

int vhx_update_ranges(vhx_ctx *c, const vhx_range *r, uint32_t n) {
    if (!c || (n && !r)) return VHX_E_INVALID_ARG;
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_update_range(s) on a shared context: update through the owner");
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_update_range(s) before vhx_upload_tree");
    // validate every range first: a failing call writes nothing
    uint64_t data_bytes = 0, njobs = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (r[k].buffer_id < 0 || r[k].buffer_id > 6 || (!r[k].src && r[k].elem_count)) return VHX_E_INVALID_ARG;
        const uint64_t cap = elem_count(c->tree->desc, r[k].buffer_id);
        if (r[k].elem_offset > cap || r[k].elem_count > cap - r[k].elem_offset)
            return fail(c, VHX_E_CAPACITY, "vhx_update_range(s): range beyond the uploaded buffer");
        const uint64_t bytes = r[k].elem_count * elem_size(r[k].buffer_id);
        data_bytes += (bytes + 15) & ~15ull;
        njobs += (bytes + UPD_PIECE_BYTES - 1) / UPD_PIECE_BYTES;
    }
    if (data_bytes == 0) return VHX_OK;
    if (njobs > 0xFFFFFFFFull) return fail(c, VHX_E_INVALID_ARG, "vhx_update_ranges: too much data in one call");
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    // the scatter and the derived-state rebuilds write the tree: frames in flight on the other contexts first
    WriteScope ws(c);
    int rc = ws.rc;
    if (rc) return rc;
    // pinned staging slot (the one used two calls ago: its copy has normally long completed)
    vhx_ctx::Pinned &P = c->pinned[c->pinned_next];
    c->pinned_next ^= 1u;
    if (P.used) VHX_HIP(c, hipEventSynchronize(P.done));
    const uint64_t jobs_bytes = (njobs * sizeof(UpdJob) + 255) & ~255ull, total = jobs_bytes + data_bytes;
    if (P.bytes < total) {
        if (P.ptr) VHX_HIP(c, hipHostFree(P.ptr));
        P.ptr = nullptr;
        P.bytes = 0;
        const uint64_t want = std::max<uint64_t>(total + total / 4, 1ull << 20);
        VHX_HIP(c, hipHostMalloc(&P.ptr, want, hipHostMallocDefault));
        P.bytes = want;
    }
    if (!P.done) VHX_HIP(c, hipEventCreateWithFlags(&P.done, hipEventDisableTiming));
    // the device staging buffer: the previous batch's scatter may still read it (on this stream, or on the stream the
    // context used then), so a growth or a stream change waits for it
    if (c->upd_stream && (c->upd_stream != c->stream || c->upd.bytes < P.bytes))
        VHX_HIP(c, hipStreamSynchronize(c->upd_stream));
    rc = ensure(c, c->upd, P.bytes);
    if (rc) return rc;
    c->upd_stream = c->stream;
    // pack: the job table, then each range's data (16-byte aligned)
    UpdJob *jobs = (UpdJob *)P.ptr;
    uint64_t off = jobs_bytes, j = 0;
    // ranges of one scatter launch are written in no particular order, so a range that overlaps an earlier range of
    // the call starts a new launch (launches on a stream run in order: the later write wins, as in a sequence of
    // write_range_to_buffer calls)
    std::vector<uint32_t> group_start{0};
    std::vector<std::pair<uint64_t, uint64_t>> group_spans[7];  // byte spans of the current group, per buffer
    uint32_t node_lo = UINT32_MAX, node_hi = 0, hdr_lo = UINT32_MAX, hdr_hi = 0, brick_lo = UINT32_MAX, brick_hi = 0;
    bool palette = false;
    const uint64_t n3 = (uint64_t)c->tree->desc.brick_dim * c->tree->desc.brick_dim * c->tree->desc.brick_dim;
    for (uint32_t k = 0; k < n; ++k) {
        const int id = r[k].buffer_id;
        const uint64_t es = elem_size(id), bytes = r[k].elem_count * es;
        if (!bytes) continue;
        std::memcpy((uint8_t *)P.ptr + off, r[k].src, bytes);
        const uint64_t dst = (uint64_t)(uintptr_t)c->tree->raw[id].ptr + r[k].elem_offset * es;
        {
            const uint64_t b0 = r[k].elem_offset * es, b1 = b0 + bytes;
            bool overlaps = false;
            for (const auto &sp : group_spans[id]) overlaps |= b0 < sp.second && sp.first < b1;
            if (overlaps) {
                group_start.push_back((uint32_t)j);
                for (auto &g : group_spans) g.clear();
            }
            group_spans[id].push_back({b0, b1});
        }
        for (uint64_t p = 0; p < bytes; p += UPD_PIECE_BYTES) {
            UpdJob &jb = jobs[j++];
            jb.dst = dst + p;
            jb.src_off = off + p;
            jb.words = (uint32_t)(std::min<uint64_t>(UPD_PIECE_BYTES, bytes - p) / 4);
            jb.pad0 = 0;
            jb.pad1 = 0;
        }
        off += (bytes + 15) & ~15ull;
        const uint64_t e0 = r[k].elem_offset, e1 = e0 + r[k].elem_count;
        if (id == VHX_BUF_NODE_TYPE || id == VHX_BUF_NODE_OCBITS) {
            hdr_lo = std::min<uint32_t>(hdr_lo, (uint32_t)e0);
            hdr_hi = std::max<uint32_t>(hdr_hi, (uint32_t)e1);
        }
        if (id == VHX_BUF_NODE_TYPE) {
            node_lo = std::min<uint32_t>(node_lo, (uint32_t)e0);
            node_hi = std::max<uint32_t>(node_hi, (uint32_t)e1);
        } else if (id == VHX_BUF_NODE_CHILDREN) {
            node_lo = std::min<uint32_t>(node_lo, (uint32_t)(e0 / 64));
            node_hi = std::max<uint32_t>(node_hi, (uint32_t)((e1 + 63) / 64));
        } else if (id == VHX_BUF_VOXELS) {
            brick_lo = std::min<uint32_t>(brick_lo, (uint32_t)(e0 / n3));
            brick_hi = std::max<uint32_t>(brick_hi, (uint32_t)((e1 + n3 - 1) / n3));
        } else if (id == VHX_BUF_COLOR_PALETTE || id == VHX_BUF_DATA_PALETTE) {
            palette = true;
        }
    }
    // one host-to-device copy of the packed batch, one scatter kernel
    VHX_HIP(c, hipMemcpyAsync(c->upd.ptr, P.ptr, total, hipMemcpyHostToDevice, c->stream));
    VHX_HIP(c, hipEventRecord(P.done, c->stream));
    P.used = true;
    group_start.push_back((uint32_t)j);
    for (size_t g = 0; g + 1 < group_start.size(); ++g) {
        const uint32_t j0 = group_start[g], j1 = group_start[g + 1];
        if (j1 > j0)
            k_scatter_ranges<<<std::min<uint32_t>(j1 - j0, 8192u), 256, 0, c->stream>>>((const uint8_t *)c->upd.ptr,
                                                                                         j0, j1);
    }
    VHX_HIP(c, hipGetLastError());
    // derived state, stream-ordered
    if (hdr_lo < hdr_hi && (rc = rebuild_hdr(c, hdr_lo, hdr_hi - hdr_lo))) return rc;
    if (palette) {
        // emptiness of any cell may change: every bitmap and record
        if ((rc = rebuild_occ(c, 0, c->tree->desc.brick_count))) return rc;
        c->tree->child_rec_stale = true;
        rc = refresh_child_rec(c);
    } else {
        if (brick_lo < brick_hi && (rc = rebuild_occ(c, brick_lo, brick_hi - brick_lo))) return rc;
        rc = refresh_child_rec_sel(c, node_lo, node_hi, brick_lo, brick_hi);
    }
    if (rc) return rc;
    return ws.end();  // the next trace of every context of the tree waits for this write
}

int vhx_update_range(vhx_ctx *c, int id, uint64_t off, uint64_t count, const void *src) {
    if (!c || id < 0 || id > 6 || (!src && count)) return VHX_E_INVALID_ARG;
    vhx_range r{};
    r.buffer_id = id;
    r.elem_offset = off;
    r.elem_count = count;
    r.src = src;
    return vhx_update_ranges(c, &r, 1);
}

int vhx_read_derived(vhx_ctx *c, int which, uint64_t off, uint64_t count, void *dst) {
    if (!c || (!dst && count) || which < 0 || which > 1) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_read_derived before vhx_upload_tree");
    const uint64_t es = which == VHX_DERIVED_NODE_HDR ? 16 : 8;
    const uint64_t cap = which == VHX_DERIVED_NODE_HDR ? c->tree->desc.node_count
                                                       : (uint64_t)c->tree->desc.brick_count * c->tree->occ_words;
    if (off + count > cap) return fail(c, VHX_E_CAPACITY, "vhx_read_derived: range beyond the buffer");
    const DevBuf &b = which == VHX_DERIVED_NODE_HDR ? c->tree->hdr : c->tree->brick_occ;
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    TraceScope tscope(c);  // after the tree's last write
    if (tscope.rc) return tscope.rc;
    VHX_HIP(c, hipMemcpyAsync(dst, (const char *)b.ptr + off * es, count * es, hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    return tscope.end();
}

int vhx_tree_device_bytes(const vhx_ctx *c, uint64_t *bytes) {
    if (!c || !bytes) return VHX_E_INVALID_ARG;
    uint64_t b = c->tree->hdr.bytes + c->tree->brick_occ.bytes + c->tree->child_rec.bytes;
    for (auto &r : c->tree->raw) b += r.bytes;
    *bytes = b;
    return VHX_OK;
}

int vhx_tree_orphans(const vhx_ctx *c, uint32_t *nodes, uint32_t *bricks) {
    if (!c || !nodes || !bricks) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return VHX_E_STATE;
    *nodes = c->tree->orphan_nodes;
    *bricks = c->tree->orphan_bricks;
    return VHX_OK;
}

int vhx_set_node_mips(vhx_ctx *c, const uint32_t *node_mips, uint32_t count) {
    if (!c) return VHX_E_INVALID_ARG;
    if (c->shared) return fail(c, VHX_E_STATE, "vhx_set_node_mips on a shared context: set them through the owner");
    if (!node_mips) {
        // switching MIPs off is a tree write too: frames in flight finish with the descriptors they started with, and
        // traces on other host threads see the switch in submission order (TreeStore ordering)
        VHX_HIP(c, hipSetDevice(c->device));
        VHX_STREAM(c);
        WriteScope ws(c);
        if (ws.rc) return ws.rc;
        c->tree->mips_on = false;
        return ws.end();
    }
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_set_node_mips: no tree uploaded");
    const vhx_tree_desc &d = c->tree->desc;
    if (count != d.node_count) return fail(c, VHX_E_INVALID_ARG, "vhx_set_node_mips: count != node_count");
    for (uint32_t i = 0; i < count; ++i) {  // every descriptor must name an uploaded brick or solid value
        const uint32_t m = node_mips[i];
        if (m == VHX_EMPTY) continue;
        if ((m & VHX_SOLID_BIT) ? (m & 0x7FFFFFFFu) >= d.solid_count : m >= d.brick_count)
            return fail(c, VHX_E_INVALID_ARG, "vhx_set_node_mips: descriptor out of range");
    }
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    WriteScope ws(c);  // frames in flight may still read the previous descriptors
    int rc = ws.rc;
    if (!rc && c->tree->mips.bytes < (uint64_t)count * 4) VHX_HIP(c, hipStreamSynchronize(c->stream));  // regrowth
    if (!rc) rc = ensure(c, c->tree->mips, (uint64_t)count * 4);
    if (rc) return rc;
    VHX_HIP(c, hipMemcpyAsync(c->tree->mips.ptr, node_mips, (uint64_t)count * 4, hipMemcpyHostToDevice, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    c->tree->mips_on = true;
    return ws.end();
}

int vhx_read_node_mips(vhx_ctx *c, uint32_t *out, uint32_t count) {
    if (!c || !out) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded || !c->tree->mips_on) return fail(c, VHX_E_STATE, "vhx_read_node_mips: no node MIPs are set");
    if (count != c->tree->desc.node_count) return fail(c, VHX_E_INVALID_ARG, "vhx_read_node_mips: count != node_count");
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    TraceScope tscope(c);  // after the tree's last write
    if (tscope.rc) return tscope.rc;
    if (!c->tree->mips_on) return fail(c, VHX_E_STATE, "vhx_read_node_mips: no node MIPs are set");
    VHX_HIP(c, hipMemcpyAsync(out, c->tree->mips.ptr, (uint64_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    return tscope.end();
}

}  // extern "C"
