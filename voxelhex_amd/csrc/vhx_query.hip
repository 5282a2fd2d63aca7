// libvhx device side, query unit: reading voxels back out of the device tree.
//
// Kernels
//   k_get_voxels     BoxTree::get (src/boxtree/mod.rs:223-317) for a batch of positions, one lane per position
//   k_read_dense     a box of the tree as a dense albedo grid, tree driven: one workgroup per aligned cube of voxels
//                    (DATA: and as a dense grid of data values, in the same walk -- vhx_read_dense_data)
// Host side: vhx_get_voxels, vhx_read_dense, vhx_read_dense_data. All are ordered like a trace (TraceScope) and launch no kernel of another
// unit except through refresh_child_rec. Wave-uniform loads and the sectant of a position come from treewalk.hpp.
//
// The walk runs in integers (DESIGN.md §8.6 argues why that equals the reference's f32 sectant_for / matrix_index_for):
// boxtree_size = brick_dim * 4^k with brick_dim a power of two, so a node's cube is 2^lg voxels wide and aligned to its
// size, the sectant of a position is bits lg-2 .. lg-1 of each coordinate and a brick cell the bits below them. A device
// tree is at most 2^24 wide (alloc_tree), so every position inside it is an f32 and the reference's conversion is exact.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/vhx.h"
#include "ctx.hpp"
#include "trace.hpp"
#include "treewalk.hpp"

using namespace vhx;

namespace {

// what the integer walk needs beyond DevTree
struct QShape {
    uint32_t lg_size;  // log2(boxtree_size)
    uint32_t lg_bd;    // log2(brick_dim)
    uint32_t levels;   // node levels: the root is level 0, the smallest leaf (4 * brick_dim wide) level levels - 1
    uint32_t brick_count, solid_count;
};

// the colour vhx_read_dense writes for a value: the palette entry of its colour index unless that is none, out of the
// palette or transparent (VHX_EMPTY has colour index 0xFFFF)
__device__ __forceinline__ uint32_t albedo_of(const DevTree &t, uint32_t v) {
    const uint32_t ci = v & 0xFFFFu;
    if (ci == 0xFFFFu || ci >= t.color_count) return 0u;
    const uint32_t a = t.color[ci];
    return (a >> 24) != 0u ? a : 0u;
}
__device__ __forceinline__ uint4 albedo_of(const DevTree &t, uint4 v) {
    return make_uint4(albedo_of(t, v.x), albedo_of(t, v.y), albedo_of(t, v.z), albedo_of(t, v.w));
}

// get_internal's match on the node the descent stopped at (mod.rs:264-316). `node` is 2^lg wide, `entry` its child entry
// at the position's sectant (with REC the child record's, whose occupancy word is cocc; a UniformLeaf's record holds its
// brick in every entry). Indices out of their tables (an image that is not a tree's) read as empty.
template <bool REC>
__device__ __forceinline__ uint32_t leaf_value(const DevTree &t, const QShape &q, uint32_t node, uint32_t type,
                                               uint32_t entry, uint64_t cocc, uint32_t lg, uint32_t x, uint32_t y,
                                               uint32_t z) {
    const bool uniform = type == VHX_NODE_UNIFORM_LEAF;
    if (!uniform && type != VHX_NODE_LEAF) return VHX_EMPTY;  // Nothing, or an Internal node without that child
    uint32_t desc = entry;
    if (!REC && uniform) desc = t.children[(uint64_t)node * 64u];
    if (desc == VHX_EMPTY) return VHX_EMPTY;
    if (desc & VHX_SOLID_BIT) {
        const uint32_t i = desc & 0x7FFFFFFFu;
        return i < q.solid_count ? t.solid[i] : VHX_EMPTY;
    }
    if (desc >= q.brick_count) return VHX_EMPTY;
    // matrix_index_for over the cube the brick spans: the node's for a UniformLeaf, the sectant's for a Leaf
    const uint32_t lgb = uniform ? lg : lg - 2u;
    const uint32_t m = (1u << lgb) - 1u, sh = lgb - q.lg_bd;
    const uint32_t cx = (x & m) >> sh, cy = (y & m) >> sh, cz = (z & m) >> sh;
    const uint32_t flat = cx + ((cy + (cz << q.lg_bd)) << q.lg_bd);
    if (!uniform) {  // a Leaf's cell that points to nothing reads as empty; a UniformLeaf's is returned raw
        const uint64_t word = REC ? cocc : t.brick_occ[(uint64_t)desc * t.occ_words + (flat >> 6)];
        if (((word >> (flat & 63u)) & 1ull) == 0ull) return VHX_EMPTY;
    }
    return t.voxels[((uint64_t)desc << (3u * q.lg_bd)) + flat];
}

// BoxTree::get_internal(ROOT, root_bounds, position), mod.rs:247-317 with get_node_internal (iterate.rs:293-343)
template <bool REC>
__device__ __forceinline__ uint32_t get_value(const DevTree &t, const QShape &q, uint32_t x, uint32_t y, uint32_t z) {
    // Cube::contains on the root (size <= 2^24: a position converts to an f32 below the size iff it is below it)
    if (x >= t.size || y >= t.size || z >= t.size) return VHX_EMPTY;
    uint32_t node = 0, lg = q.lg_size;
    for (uint32_t lvl = 0;; ++lvl) {
        const uint64_t at = (uint64_t)node * 64u + sectant_of(x, y, z, lg);
        // the header and the child entry are independent loads: one memory latency per level
        const uint4 h = t.hdr[node];
        uint32_t entry;
        uint64_t cocc = 0;
        if (REC) {
            const uint4 cr = t.child_rec[at];
            entry = cr.x;
            cocc = ((uint64_t)cr.z << 32) | (uint64_t)cr.y;
        } else {
            entry = t.children[at];
        }
        if (h.z != VHX_NODE_INTERNAL) return leaf_value<REC>(t, q, node, h.z, entry, cocc, lg, x, y, z);
        // an empty sectant, or a child that is not in this view; no node is smaller than 4 * brick_dim
        if (entry == VHX_EMPTY || entry >= t.node_count || lvl + 1u >= q.levels) return VHX_EMPTY;
        node = entry;
        lg -= 2u;
    }
}

template <bool REC>
__global__ void __launch_bounds__(256) k_get_voxels(DevTree t, QShape q, const uint32_t *__restrict__ pos, uint64_t n,
                                                    uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = get_value<REC>(t, q, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
}

struct DenseBox {
    uint32_t ox, oy, oz, gx, gy, gz;
    uint32_t *out;           // vhx_read_dense_data: may be null (data only)
    uint32_t *dout;          // vhx_read_dense_data: the data plane
    const uint32_t *dpal;    // the tree's data_palette
    uint32_t dcount;
    uint32_t lgu;            // log2 of the work unit's edge U
    uint32_t ux0, uy0, uz0;  // first unit of the box per axis (in units)
    uint32_t nux, nuy, nuz;  // units per axis
    uint32_t vec;            // rows of the output (of both planes) start and end on 16-byte boundaries
};

// the data value vhx_read_dense_data writes for a value: the palette entry of its data index unless the value is
// VHX_EMPTY or the index none or out of the palette
__device__ __forceinline__ uint32_t data_of(const DenseBox &b, uint32_t v) {
    const uint32_t di = v >> 16;
    if (v == VHX_EMPTY || di == 0xFFFFu || di >= b.dcount) return 0u;
    return b.dpal[di];
}
__device__ __forceinline__ uint4 data_of(const DenseBox &b, uint4 v) {
    return make_uint4(data_of(b, v.x), data_of(b, v.y), data_of(b, v.z), data_of(b, v.w));
}

// How a work unit is filled, chosen once per unit from its wave-uniform descent
enum : uint32_t {
    FILL_CONST = 0,  // an empty sectant at any level, Nothing, an Empty brick (zeros); a Solid brick (its colour)
    FILL_ROWS = 1,   // part of one Parted brick whose cells are voxels (brick_dim >= 8): its rows are contiguous runs
    FILL_LEAF4 = 2,  // a whole smallest leaf at brick_dim 4: 64 bricks of 64 contiguous values
    FILL_CELLS = 3   // anything else (bricks stretched over larger cubes, brick_dim 1 and 2): leaf_value per voxel
};

// A work unit is an aligned cube of U^3 voxels, U = 4 * brick_dim for brick_dim <= 4 (a smallest leaf's cube) and
// min(brick_dim, 16) above (a brick, or a 16^3 part of one): at most 4096 voxels, and never cut by a node or brick
// boundary except, at brick_dim <= 4, by the bricks of the one leaf it is. The workgroup walks to the unit's node once,
// turns the unit into output colours in LDS (constant fills skip that) and writes the part inside the box as rows.
// DATA: the same walk fills a second tile with the unit's data values and writes the data plane beside the albedo plane
// (which may then be absent).
template <bool REC, bool DATA>
__global__ void __launch_bounds__(256) k_read_dense(DevTree t, QShape q, DenseBox b, uint64_t nunits) {
    __shared__ uint4 tile4[DATA ? 2048 : 1024];
    uint32_t *tile = (uint32_t *)tile4;
    uint4 *dtile4 = tile4 + (DATA ? 1024 : 0);
    uint32_t *dtile = (uint32_t *)dtile4;
    const uint32_t lgu = b.lgu, U = 1u << lgu, um = U - 1u;
    const uint32_t nvox = 1u << (3u * lgu);
    for (uint64_t u = blockIdx.x; u < nunits; u += gridDim.x) {
        const uint32_t X = (b.ux0 + (uint32_t)(u % b.nux)) << lgu, Y = (b.uy0 + (uint32_t)((u / b.nux) % b.nuy)) << lgu,
                       Z = (b.uz0 + (uint32_t)(u / ((uint64_t)b.nux * b.nuy))) << lgu;
        // the descent, the same for every voxel of the unit: every node above it is at least 4 units wide
        uint32_t node = 0, lg = q.lg_size, type, entry;
        for (uint32_t lvl = 0;; ++lvl) {
            const uint64_t at = (uint64_t)node * 64u + sectant_of(X, Y, Z, lg);
            type = __builtin_amdgcn_readfirstlane(uload((const uint32_t *)&t.hdr[node] + 2));
            entry = __builtin_amdgcn_readfirstlane(REC ? uload((const uint32_t *)&t.child_rec[at]) : uload(&t.children[at]));
            if (type != VHX_NODE_INTERNAL) break;
            if (entry == VHX_EMPTY || entry >= t.node_count || lvl + 1u >= q.levels) {
                type = VHX_NODE_NOTHING;
                break;
            }
            node = entry;
            lg -= 2u;
        }
        const bool uniform = type == VHX_NODE_UNIFORM_LEAF, leaf = type == VHX_NODE_LEAF;
        uint32_t mode = FILL_CONST, fill = 0u, dfill = 0u, desc = VHX_EMPTY;
        if (uniform || (leaf && lg - 2u >= lgu)) {  // one brick for the whole unit
            desc = (!REC && uniform) ? __builtin_amdgcn_readfirstlane(uload(&t.children[(uint64_t)node * 64u])) : entry;
            if (desc == VHX_EMPTY) {
            } else if (desc & VHX_SOLID_BIT) {
                const uint32_t i = desc & 0x7FFFFFFFu;
                if (i < q.solid_count) {
                    const uint32_t sv = uload(&t.solid[i]);
                    fill = __builtin_amdgcn_readfirstlane(albedo_of(t, sv));
                    if (DATA) dfill = __builtin_amdgcn_readfirstlane(data_of(b, sv));
                }
            } else if (desc < q.brick_count) {
                mode = (!uniform && lg - 2u == q.lg_bd && q.lg_bd >= 3u) ? FILL_ROWS : FILL_CELLS;
            }
        } else if (leaf) {  // the unit is the whole leaf
            mode = (q.lg_bd == 2u && lg == 4u && lgu == 4u) ? FILL_LEAF4 : FILL_CELLS;
        }

        if (mode == FILL_ROWS) {
            const uint32_t bm = (1u << q.lg_bd) - 1u;
            const uint32_t *brick = t.voxels + ((uint64_t)desc << (3u * q.lg_bd));
            for (uint32_t i = threadIdx.x; i < nvox / 4u; i += 256u) {
                const uint32_t qx = i & (U / 4u - 1u), cy = (i >> (lgu - 2u)) & um, cz = i >> (2u * lgu - 2u);
                const uint32_t sx = (X & bm) + 4u * qx, sy = (Y & bm) + cy, sz = (Z & bm) + cz;
                const uint32_t src = (((sz << q.lg_bd) + sy) << q.lg_bd) + sx;
                const uint4 raw = *(const uint4 *)(brick + src);
                tile4[i] = albedo_of(t, raw);
                if (DATA) dtile4[i] = data_of(b, raw);
            }
        } else if (mode == FILL_LEAF4) {
            for (uint32_t i = threadIdx.x; i < 1024u; i += 256u) {
                const uint32_t s = i >> 4, r = i & 15u;  // brick, and its row (y, z)
                const uint32_t d = t.children[(uint64_t)node * 64u + s];
                uint4 c = make_uint4(0u, 0u, 0u, 0u), dv = c;
                if (d == VHX_EMPTY) {
                } else if (d & VHX_SOLID_BIT) {
                    const uint32_t k = d & 0x7FFFFFFFu;
                    const uint32_t sv = k < q.solid_count ? t.solid[k] : VHX_EMPTY;
                    const uint32_t a = albedo_of(t, sv);
                    c = make_uint4(a, a, a, a);
                    if (DATA) {
                        const uint32_t e = data_of(b, sv);
                        dv = make_uint4(e, e, e, e);
                    }
                } else if (d < q.brick_count) {
                    const uint4 raw = *(const uint4 *)(t.voxels + (uint64_t)d * 64u + r * 4u);
                    c = albedo_of(t, raw);
                    if (DATA) dv = data_of(b, raw);
                }
                const uint32_t ty = ((s >> 2) & 3u) * 4u + (r & 3u), tz = (s >> 4) * 4u + (r >> 2);
                tile4[(tz * 16u + ty) * 4u + (s & 3u)] = c;
                if (DATA) dtile4[(tz * 16u + ty) * 4u + (s & 3u)] = dv;
            }
        } else if (mode == FILL_CELLS) {
            for (uint32_t i = threadIdx.x; i < nvox; i += 256u) {
                const uint32_t x = X + (i & um), y = Y + ((i >> lgu) & um), z = Z + (i >> (2u * lgu));
                const uint64_t at = (uint64_t)node * 64u + sectant_of(x, y, z, lg);
                uint32_t e;
                uint64_t cocc = 0;
                if (REC) {
                    const uint4 cr = t.child_rec[at];
                    e = cr.x;
                    cocc = ((uint64_t)cr.z << 32) | (uint64_t)cr.y;
                } else {
                    e = t.children[at];
                }
                const uint32_t val = leaf_value<REC>(t, q, node, type, e, cocc, lg, x, y, z);
                tile[i] = albedo_of(t, val);
                if (DATA) dtile[i] = data_of(b, val);
            }
        }
        if (mode != FILL_CONST) __syncthreads();

        // the unit's rows, clipped to the box (unsigned differences: a coordinate below the origin wraps past the extent)
        if (b.vec) {
            const uint4 f4 = make_uint4(fill, fill, fill, fill);
            for (uint32_t i = threadIdx.x; i < nvox / 4u; i += 256u) {
                const uint32_t x = X + 4u * (i & (U / 4u - 1u)) - b.ox, y = Y + ((i >> (lgu - 2u)) & um) - b.oy,
                               z = Z + (i >> (2u * lgu - 2u)) - b.oz;
                if (x < b.gx && y < b.gy && z < b.gz) {
                    const uint64_t at = ((uint64_t)z * b.gy + y) * b.gx + x;
                    if (!DATA || b.out) {
                        uint4 v = f4;
                        if (mode != FILL_CONST) v = tile4[i];
                        *(uint4 *)(b.out + at) = v;
                    }
                    if (DATA) {
                        uint4 v = make_uint4(dfill, dfill, dfill, dfill);
                        if (mode != FILL_CONST) v = dtile4[i];
                        *(uint4 *)(b.dout + at) = v;
                    }
                }
            }
        } else {
            for (uint32_t i = threadIdx.x; i < nvox; i += 256u) {
                const uint32_t x = X + (i & um) - b.ox, y = Y + ((i >> lgu) & um) - b.oy, z = Z + (i >> (2u * lgu)) - b.oz;
                if (x < b.gx && y < b.gy && z < b.gz) {
                    const uint64_t at = ((uint64_t)z * b.gy + y) * b.gx + x;
                    if (!DATA || b.out) {
                        uint32_t v = fill;
                        if (mode != FILL_CONST) v = tile[i];
                        b.out[at] = v;
                    }
                    if (DATA) {
                        uint32_t v = dfill;
                        if (mode != FILL_CONST) v = dtile[i];
                        b.dout[at] = v;
                    }
                }
            }
        }
        if (mode != FILL_CONST) __syncthreads();  // the tile is free for the next unit
    }
}

DevTree query_tree(const vhx_ctx *c) {
    const TreeStore &s = *c->tree;
    DevTree t;
    t.hdr = (const uint4 *)s.hdr.ptr;
    t.children = (const uint32_t *)s.raw[VHX_BUF_NODE_CHILDREN].ptr;
    t.voxels = (const uint32_t *)s.raw[VHX_BUF_VOXELS].ptr;
    t.brick_occ = (const uint64_t *)s.brick_occ.ptr;
    t.child_rec = (const uint4 *)s.child_rec.ptr;
    t.solid = (const uint32_t *)s.raw[VHX_BUF_SOLID_VALUES].ptr;
    t.color = (const uint32_t *)s.raw[VHX_BUF_COLOR_PALETTE].ptr;
    t.mips = nullptr;  // get never consults a node's MIP
    t.color_count = s.desc.color_count;
    t.node_count = s.desc.node_count;
    t.size = s.desc.boxtree_size;
    t.bd = s.desc.brick_dim;
    t.occ_words = s.occ_words;
    return t;
}

uint32_t log2u(uint32_t v) {
    uint32_t l = 0;
    while ((1u << l) < v && l < 31u) ++l;
    return l;
}

// What both entry points do before their launch: the device, the stream, the trace's place in the tree-write ordering
// (scope), the child records and the tree as the kernels read it.
int begin_query(vhx_ctx *c, const char *name, DevTree &t, QShape &q) {
    const vhx_tree_desc &d = c->tree->desc;
    if ((d.brick_dim & (d.brick_dim - 1u)) != 0u || (d.boxtree_size & (d.boxtree_size - 1u)) != 0u ||
        d.brick_dim == 0u || d.boxtree_size < 4u * d.brick_dim || ((log2u(d.boxtree_size) - log2u(d.brick_dim)) & 1u))
        return fail(c, VHX_E_INVALID_ARG, std::string(name) + ": the tree's size is not brick_dim * 4^k");
    int rc = refresh_child_rec(c);
    if (rc) return rc;
    t = query_tree(c);
    q.lg_size = log2u(d.boxtree_size);
    q.lg_bd = log2u(d.brick_dim);
    q.levels = (q.lg_size - q.lg_bd) / 2u;
    q.brick_count = d.brick_count;
    q.solid_count = d.solid_count;
    return VHX_OK;
}

bool has_child_rec(const vhx_ctx *c) {
    const uint32_t bd = c->tree->desc.brick_dim;
    return bd * bd * bd <= 64;
}

// both dense reads; `name` is the one called, for the error texts. with_data: `data` receives the data plane and
// box->albedo may be null.
int read_dense(vhx_ctx *c, const vhx_dense_out *box, uint32_t *data, bool with_data, int on_device, const char *name) {
    if (!c || !box) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, std::string(name) + " before vhx_upload_tree");
    const uint64_t S = c->tree->desc.boxtree_size;
    if ((with_data ? !data : !box->albedo) || box->gx == 0 || box->gy == 0 || box->gz == 0 ||
        (uint64_t)box->ox + box->gx > S || (uint64_t)box->oy + box->gy > S || (uint64_t)box->oz + box->gz > S)
        return fail(c, VHX_E_INVALID_ARG, std::string(name) + ": a null grid, an extent of 0, or a box outside the root cube");
    const uint64_t voxels = (uint64_t)box->gx * box->gy * box->gz;
    if (with_data && on_device && box->albedo) {
        const char *a0 = (const char *)box->albedo, *d0 = (const char *)data;
        if (a0 < d0 + voxels * 4 && d0 < a0 + voxels * 4)
            return fail(c, VHX_E_INVALID_ARG, std::string(name) + ": the data plane overlaps the albedo plane");
    }
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    TraceScope scope(c);
    if (scope.rc) return scope.rc;
    int rc;
    DenseBox b{};
    b.ox = box->ox, b.oy = box->oy, b.oz = box->oz;
    b.gx = box->gx, b.gy = box->gy, b.gz = box->gz;
    b.out = box->albedo;
    b.dout = data;
    if (!on_device) {  // the data plane follows the albedo plane
        if ((rc = ensure(c, c->query, voxels * (with_data ? 8 : 4)))) return rc;
        b.out = (!with_data || box->albedo) ? (uint32_t *)c->query.ptr : nullptr;
        if (with_data) b.dout = (uint32_t *)c->query.ptr + voxels;
    }
    DevTree t;
    QShape q;
    if ((rc = begin_query(c, name, t, q))) return rc;
    b.dpal = (const uint32_t *)c->tree->raw[VHX_BUF_DATA_PALETTE].ptr;
    b.dcount = b.dpal ? c->tree->desc.data_count : 0u;
    const bool rec = has_child_rec(c);
    b.lgu = q.lg_bd <= 2u ? q.lg_bd + 2u : std::min(q.lg_bd, 4u);
    b.ux0 = b.ox >> b.lgu, b.uy0 = b.oy >> b.lgu, b.uz0 = b.oz >> b.lgu;
    b.nux = ((b.ox + b.gx - 1u) >> b.lgu) - b.ux0 + 1u;
    b.nuy = ((b.oy + b.gy - 1u) >> b.lgu) - b.uy0 + 1u;
    b.nuz = ((b.oz + b.gz - 1u) >> b.lgu) - b.uz0 + 1u;
    b.vec = ((uintptr_t)b.out % 16u) == 0 && ((uintptr_t)b.dout % 16u) == 0 && (b.gx % 4u) == 0 && (b.ox % 4u) == 0;
    const uint64_t nunits = (uint64_t)b.nux * b.nuy * b.nuz;
    // a launch holds fewer than 2^32 threads: past 2^23 units the workgroups stride over them
    const unsigned blocks = (unsigned)std::min<uint64_t>(nunits, 1ull << 23);
    if (with_data) {
        if (rec)
            k_read_dense<true, true><<<blocks, 256, 0, c->stream>>>(t, q, b, nunits);
        else
            k_read_dense<false, true><<<blocks, 256, 0, c->stream>>>(t, q, b, nunits);
    } else if (rec) {
        k_read_dense<true, false><<<blocks, 256, 0, c->stream>>>(t, q, b, nunits);
    } else {
        k_read_dense<false, false><<<blocks, 256, 0, c->stream>>>(t, q, b, nunits);
    }
    VHX_HIP(c, hipGetLastError());
    if (!on_device) {
        if (b.out) VHX_HIP(c, hipMemcpyAsync(box->albedo, b.out, voxels * 4, hipMemcpyDeviceToHost, c->stream));
        if (with_data) VHX_HIP(c, hipMemcpyAsync(data, b.dout, voxels * 4, hipMemcpyDeviceToHost, c->stream));
        VHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return scope.end();
}

}  // namespace

extern "C" {

int vhx_get_voxels(vhx_ctx *c, const uint32_t *positions, uint64_t n, uint32_t *values, int on_device) {
    if (!c || (n && (!positions || !values))) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_get_voxels before vhx_upload_tree");
    if (n == 0) return VHX_OK;
    if (n > 0x80000000ull) return fail(c, VHX_E_INVALID_ARG, "vhx_get_voxels: more than 2^31 positions");
    if (on_device) {
        const char *p0 = (const char *)positions, *v0 = (const char *)values;
        if (p0 < v0 + n * 4 && v0 < p0 + n * 12)
            return fail(c, VHX_E_INVALID_ARG, "vhx_get_voxels: values overlaps positions");
    }
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_STREAM(c);
    TraceScope scope(c);
    if (scope.rc) return scope.rc;
    int rc;
    const uint32_t *dpos = positions;
    uint32_t *dval = values;
    if (!on_device) {
        const uint64_t voff = (n * 12 + 255) & ~255ull;
        if ((rc = ensure(c, c->query, voff + n * 4))) return rc;
        VHX_HIP(c, hipMemcpyAsync(c->query.ptr, positions, n * 12, hipMemcpyHostToDevice, c->stream));
        dpos = (const uint32_t *)c->query.ptr;
        dval = (uint32_t *)((char *)c->query.ptr + voff);
    }
    DevTree t;
    QShape q;
    if ((rc = begin_query(c, "vhx_get_voxels", t, q))) return rc;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (has_child_rec(c))
        k_get_voxels<true><<<blocks, 256, 0, c->stream>>>(t, q, dpos, n, dval);
    else
        k_get_voxels<false><<<blocks, 256, 0, c->stream>>>(t, q, dpos, n, dval);
    VHX_HIP(c, hipGetLastError());
    if (!on_device) {
        VHX_HIP(c, hipMemcpyAsync(values, dval, n * 4, hipMemcpyDeviceToHost, c->stream));
        VHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return scope.end();
}

int vhx_read_dense(vhx_ctx *c, const vhx_dense_out *box, int on_device) {
    return read_dense(c, box, nullptr, false, on_device, "vhx_read_dense");
}

int vhx_read_dense_data(vhx_ctx *c, const vhx_dense_out *box, uint32_t *data, int on_device) {
    return read_dense(c, box, data, true, on_device, "vhx_read_dense_data");
}

}  // extern "C"
