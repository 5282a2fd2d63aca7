// Flattening of the host BoxTree into the vhx_tree_desc layout, bulk procedural-scene builder, and the C ABI of
// include/vhx_boxtree.h.
//
// The flattened layout replaces the reference's streamed GPU buffers (BoxTreeRenderData,
// src/raytracing/bevy/types.rs:203-256, filled by add_node/add_brick, src/raytracing/bevy/streaming/cache.rs:226-455,
// 608-716) with a full-residency image: nodes breadth-first from the root, bricks and solid values in node order.
//
// Bulk builder: a tree filled only through BoxTree::insert of single voxels is canonical — insert never simplifies
// (insert.rs:371-373 calls simplify on the invalid bottom child key, which returns false, so `simplifyable` drops
// to false before any node is touched), leaf nodes are exactly the nodes of edge 4*brick_dim, every brick that
// received a voxel is Parted, and occupied_bits has a bit per non-empty child (post_process_node_insert,
// insert.rs:428-449). vhx_scene_build writes that canonical image directly; tests check it buffer-equal against
// vhx_scene_insert + vhx_boxtree_flatten. The image is a pure function of the voxels, so the same builder takes a caller's
// dense grid (vhx_dense_build); vhx_build_tree_dense (vhx_build.hip) writes the same image on the GPU.
// vhx_dense_build_simplified is that tree simplified recursively and flattened: the image
// vhx_build_tree_dense_simplified is held to.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <new>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/vhx_boxtree.h"
#include "boxtree.hpp"

using namespace vhx;

struct vhx_flat {
    uint32_t size = 0, brick_dim = 0;
    std::vector<uint32_t> node_type;
    std::vector<uint64_t> node_ocbits;
    std::vector<uint32_t> node_children;
    std::unique_ptr<uint32_t[]> voxels;  // uninitialised storage (GB scale)
    uint64_t voxel_count = 0;
    uint32_t brick_count = 0;
    std::vector<uint32_t> solid_values;
    std::vector<uint32_t> color_palette;
    std::vector<uint32_t> data_palette;
    // per node: its MIP brick descriptor (same encoding as a leaf's child entry; node_mips of
    // src/raytracing/bevy/types.rs:245-247); empty unless the tree's MIP maps are enabled
    std::vector<uint32_t> node_mips;
};

// ---------------------------------------------------------------------------------------------- parallel helper
template <class F>
static void parallel_for(int64_t n, int threads, F &&f) {
    if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
    threads = (int)std::min<int64_t>(threads, std::max<int64_t>(n, 1));
    if (threads <= 1) {
        for (int64_t i = 0; i < n; ++i) f(i);
        return;
    }
    std::atomic<int64_t> next{0};
    auto worker = [&] {
        for (;;) {
            int64_t i = next.fetch_add(1);
            if (i >= n) break;
            f(i);
        }
    };
    // the calling thread is one of the workers; a helper that cannot be created (std::system_error) is missing and the
    // shared counter lets the others finish, so no exception crosses the C ABI
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) {
        try {
            pool.emplace_back(worker);
        } catch (const std::system_error &) {
            break;
        }
    }
    worker();
    for (auto &th : pool) th.join();
}

// ---------------------------------------------------------------------------------------------- scenes
static inline uint32_t rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
    return (r & 0xFFu) | ((g & 0xFFu) << 8) | ((b & 0xFFu) << 16) | ((a & 0xFFu) << 24);
}
static inline uint32_t u8_of(float f) {  // Rust `as u8` on f32 (saturating)
    if (std::isnan(f) || f <= 0.f) return 0;
    if (f >= 255.f) return 255;
    return (uint32_t)f;
}
static inline uint64_t splitmix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct Scene {
    uint32_t id, S;
    uint64_t seed;
    uint32_t extent;  // voxels are only set inside [0, extent)^3
    // value-noise heightfield cache (per (x,z) column), built lazily for VHX_SCENE_HEIGHTFIELD
    std::vector<uint16_t> height;

    // returns packed albedo, 0 = no voxel
    inline uint32_t voxel(uint32_t x, uint32_t y, uint32_t z) const {
        const uint32_t q = S / 4, h = S / 2;
        switch (id) {
            case VHX_SCENE_LATTICE_CUBE: {  // examples/gpu_render.rs:57-82
                bool set = ((x < q || y < q || z < q) && (0 == x % 2 && 0 == y % 4 && 0 == z % 2)) ||
                           (h <= x && h <= y && h <= z);
                if (!set) return 0;
                uint32_t r = (0 == x % q) ? (uint32_t)((float)x / (float)S * 255.f) : 128u;
                uint32_t g = (0 == y % q) ? (uint32_t)((float)y / (float)S * 255.f) : 128u;
                uint32_t b = (0 == z % q) ? (uint32_t)((float)z / (float)S * 255.f) : 128u;
                return rgba(r, g, b, 255);
            }
            case VHX_SCENE_BENCH_REGION: {  // benches/performance.rs:13-26, Albedo::from(0x00ABCDEF)
                if (x >= 100 || y >= 100 || z >= 100) return 0;
                bool set = x < q || y < q || z < q || (h <= x && h <= y && h <= z);
                return set ? rgba(0x00, 0xAB, 0xCD, 0xEF) : 0;
            }
            case VHX_SCENE_LATTICE: {  // src/raytracing/tests.rs:777-789
                bool set = (x < q || y < q || z < q) && (0 == x % 2 && 0 == y % 4 && 0 == z % 2);
                if (!set) return 0;
                return rgba(u8_of(255.f * (float)x / (float)S), u8_of(255.f * (float)y / (float)S),
                            u8_of(255.f * (float)z / (float)S), 255);
            }
            case VHX_SCENE_CUBE: {  // src/raytracing/tests.rs:736-748
                if (!(h <= x && h <= y && h <= z)) return 0;
                return rgba(u8_of(255.f * (float)x / (float)S), u8_of(255.f * (float)y / (float)S),
                            u8_of(255.f * (float)z / (float)S), 255);
            }
            case VHX_SCENE_BOUNDARY: {  // src/raytracing/tests.rs:692-703
                bool set = ((x < q || y < q || z < q) && (0 == x % 2 && 0 == y % 4 && 0 == z % 2)) ||
                           (h <= x && h <= y && h <= z);
                if (!set) return 0;
                return rgba(u8_of(255.f * (float)(x % 6) / 6.0f), u8_of(255.f * (float)(y % 6) / 6.0f),
                            u8_of(255.f * (float)(z % 6) / 6.0f), 255);
            }
            case VHX_SCENE_HEIGHTFIELD: {
                uint32_t hh = height[(size_t)x * S + z];
                if (y > hh) return 0;
                if (y + 2 < hh) return rgba(110, 84, 60, 255);               // soil
                if (hh > (S * 3) / 8) return rgba(235, 235, 240, 255);       // snow caps
                return rgba(70, 140 + (hh % 5) * 10, 60, 255);               // grass bands
            }
            default: return 0;
        }
    }

    void prepare() {
        extent = id == VHX_SCENE_BENCH_REGION ? std::min(S, 100u) : S;
        if (id != VHX_SCENE_HEIGHTFIELD) return;
        // seeded 4-octave value noise, height in [S/16, S/16 + S/4)
        height.assign((size_t)S * S, 0);
        auto lattice = [&](int64_t ix, int64_t iz, int oct) {
            uint64_t k = splitmix(seed ^ splitmix((uint64_t)ix * 0x9E37u + (uint64_t)oct * 0x1234567ull) ^
                                  splitmix((uint64_t)iz * 0x85EBCA77ull));
            return (float)(k >> 40) / (float)(1ull << 24);
        };
        auto smooth = [](float t) { return t * t * (3.f - 2.f * t); };
        for (uint32_t x = 0; x < S; ++x)
            for (uint32_t z = 0; z < S; ++z) {
                float n = 0.f, amp = 0.5f, cell = (float)std::max(4u, S / 4);
                for (int o = 0; o < 4; ++o) {
                    float fx = (float)x / cell, fz = (float)z / cell;
                    int64_t ix = (int64_t)std::floor(fx), iz = (int64_t)std::floor(fz);
                    float tx = smooth(fx - (float)ix), tz = smooth(fz - (float)iz);
                    float a = lattice(ix, iz, o), b = lattice(ix + 1, iz, o), c = lattice(ix, iz + 1, o),
                          d = lattice(ix + 1, iz + 1, o);
                    float v = (a + (b - a) * tx) + ((c + (d - c) * tx) - (a + (b - a) * tx)) * tz;
                    n += v * amp;
                    amp *= 0.5f;
                    cell = std::max(1.f, cell / 2.f);
                }
                height[(size_t)x * S + z] = (uint16_t)std::min<float>((float)(S - 1), (float)(S / 16) + n * (float)(S / 4));
            }
    }
};

static bool scene_valid(uint32_t id) { return id >= VHX_SCENE_LATTICE_CUBE && id <= VHX_SCENE_HEIGHTFIELD; }

// ---------------------------------------------------------------------------------------------- flatten
static uint32_t brick_desc(const Brick &b, vhx_flat &f, std::vector<const std::vector<uint32_t> *> &parted,
                           std::unordered_map<uint32_t, uint32_t> &solid_index) {
    switch (b.kind) {
        case BrickKind::Empty: return VHX_EMPTY;
        case BrickKind::Solid: {
            auto it = solid_index.find(b.solid);
            uint32_t idx;
            if (it == solid_index.end()) {
                idx = (uint32_t)f.solid_values.size();
                solid_index.emplace(b.solid, idx);
                f.solid_values.push_back(b.solid);
            } else {
                idx = it->second;
            }
            return VHX_SOLID_BIT | idx;
        }
        default:
            parted.push_back(&b.parted);
            return (uint32_t)(parted.size() - 1);
    }
}

// max_depth: nodes deeper than this (root = depth 0) are left out; their parent's child entries are VHX_EMPTY while its
// occupancy bits stay, so a MIP-enabled trace shows the parent's MIP there (the WGSL's stand-in for a child that is
// not resident, viewport_render.wgsl:438-454). MIP bricks are numbered with the bricks, after the node's own.
static vhx_flat *flatten_tree(const BoxTree &t, uint32_t max_depth = 0xFFFFFFFFu, bool with_mips = false) {
    auto *f = new vhx_flat();
    f->size = t.boxtree_size;
    f->brick_dim = t.brick_dim;
    std::unordered_map<size_t, uint32_t> index;  // pool key -> BFS index
    std::deque<size_t> queue;
    std::vector<const std::vector<uint32_t> *> parted;
    std::unordered_map<uint32_t, uint32_t> solid_index;
    std::vector<uint32_t> depth{0};  // by BFS index
    index.emplace(0, 0);
    queue.push_back(0);
    while (!queue.empty()) {
        size_t key = queue.front();
        queue.pop_front();
        const Node &n = t.nodes.get(key);
        uint32_t idx = (uint32_t)f->node_type.size();
        uint32_t type = n.content == Content::Nothing   ? VHX_NODE_NOTHING
                        : n.content == Content::Internal ? VHX_NODE_INTERNAL
                        : n.content == Content::Leaf     ? VHX_NODE_LEAF
                                                         : VHX_NODE_UNIFORM_LEAF;
        f->node_type.push_back(type);
        f->node_ocbits.push_back(n.occupied_bits);
        f->node_children.resize((size_t)(idx + 1) * 64, VHX_EMPTY);
        uint32_t *ch = &f->node_children[(size_t)idx * 64];
        if (n.content == Content::Internal && n.has_children && depth[idx] < max_depth) {
            for (int s = 0; s < 64; ++s) {
                size_t c = n.children[s];
                if (!t.nodes.key_is_valid(c)) continue;  // freed / missing child: traced as empty
                auto it = index.find(c);
                if (it == index.end()) {
                    uint32_t ni = (uint32_t)index.size();
                    index.emplace(c, ni);
                    queue.push_back(c);
                    depth.push_back(depth[idx] + 1);
                    ch[s] = ni;
                } else {
                    ch[s] = it->second;
                }
            }
        } else if (n.content == Content::Leaf) {
            for (int s = 0; s < 64; ++s) ch[s] = brick_desc(n.bricks[s], *f, parted, solid_index);
        } else if (n.content == Content::UniformLeaf) {
            ch[0] = brick_desc(n.bricks[0], *f, parted, solid_index);
        }
        if (with_mips) f->node_mips.push_back(brick_desc(n.mip, *f, parted, solid_index));
    }
    size_t n3 = (size_t)t.brick_dim * t.brick_dim * t.brick_dim;
    f->brick_count = (uint32_t)parted.size();
    f->voxel_count = (uint64_t)parted.size() * n3;
    f->voxels.reset(new uint32_t[std::max<uint64_t>(f->voxel_count, 1)]);
    for (size_t i = 0; i < parted.size(); ++i) std::memcpy(&f->voxels[i * n3], parted[i]->data(), n3 * 4);
    f->color_palette = t.color_palette;
    f->data_palette = t.data_palette;
    return f;
}

// A BoxTree holding a flattened image's nodes, bricks and palettes (pool key = breadth-first index, so the depth-first
// child order and therefore the MIP palette growth are those of the tree the image came from). Occlusion bits and the
// insert bookkeeping are not restored: the tree only serves recalculate_mips + flatten_tree inside this file.
static BoxTree *tree_of_flat(const vhx_flat &f) {
    BoxTree *t = nullptr;
    if (BoxTree::create(f.size, f.brick_dim, &t) != 0) return nullptr;
    const size_t n3 = (size_t)f.brick_dim * f.brick_dim * f.brick_dim;
    auto brick_of = [&](uint32_t desc) {
        Brick b;
        if (desc == VHX_EMPTY) return b;
        if (desc & VHX_SOLID_BIT) {
            b.kind = BrickKind::Solid;
            b.solid = f.solid_values[desc & ~VHX_SOLID_BIT];
        } else {
            b.kind = BrickKind::Parted;
            b.parted.assign(&f.voxels[(size_t)desc * n3], &f.voxels[(size_t)desc * n3] + n3);
        }
        return b;
    };
    for (size_t i = 0; i < f.node_type.size(); ++i) {
        Node n;
        const uint32_t *ch = &f.node_children[i * 64];
        n.occupied_bits = f.node_ocbits[i];
        switch (f.node_type[i]) {
            case VHX_NODE_INTERNAL:
                n.content = Content::Internal;
                n.has_children = true;
                for (int s = 0; s < 64; ++s) n.children[s] = ch[s] == VHX_EMPTY ? kEmpty32 : ch[s];
                break;
            case VHX_NODE_LEAF:
                n.content = Content::Leaf;
                for (int s = 0; s < 64; ++s) n.bricks.push_back(brick_of(ch[s]));
                break;
            case VHX_NODE_UNIFORM_LEAF:
                n.content = Content::UniformLeaf;
                n.bricks.push_back(brick_of(ch[0]));
                break;
            default: n.content = Content::Nothing; break;
        }
        if (i == 0) {
            t->nodes.get(0) = std::move(n);
        } else if (t->nodes.push(std::move(n)) != i) {
            delete t;
            return nullptr;
        }
    }
    for (uint32_t c : f.color_palette) t->add_to_palette(Entry{VHX_ENTRY_VISUAL, c, 0});
    for (uint32_t d : f.data_palette) t->add_to_palette(Entry{VHX_ENTRY_INFORMATIVE, 0, d});
    if (t->color_palette != f.color_palette || t->data_palette != f.data_palette) {
        delete t;
        return nullptr;
    }
    return t;
}

// ---------------------------------------------------------------------------------------------- bulk builder
// The voxel source of the bulk builder: a procedural scene, or a caller's dense grid (vhx_dense_desc). voxel() returns
// the packed albedo, 0 = no voxel, and is defined for every position of the tree; voxels are only set inside
// [0, ex) x [0, ey) x [0, ez).
struct SceneSource {
    const Scene &sc;
    uint32_t ex, ey, ez;
    explicit SceneSource(const Scene &s) : sc(s), ex(s.extent), ey(s.extent), ez(s.extent) {}
    inline uint32_t voxel(uint32_t x, uint32_t y, uint32_t z) const { return sc.voxel(x, y, z); }
};
struct DenseSource {
    const uint32_t *albedo;
    uint32_t ex, ey, ez;
    inline uint32_t voxel(uint32_t x, uint32_t y, uint32_t z) const {
        if (x >= ex || y >= ey || z >= ez) return 0;
        const uint32_t c = albedo[((uint64_t)z * ey + y) * ex + x];
        return (c >> 24) ? c : 0;  // alpha 0: BoxTreeEntry::is_none of a Visual entry (boxtree.cpp entry_is_none)
    }
};
// A dense grid with a data plane beside the albedo plane: voxel() is the albedo (0 where its alpha byte is 0) in the low
// word and the data value (0 = none, is_empty of T = u32) in the high word, so 0 is still "no entry": the albedo alone
// is a Visual entry, the data alone an Informative one, both a Complex one.
struct DenseDataSource {
    const uint32_t *albedo, *data;
    uint32_t ex, ey, ez;
    inline uint64_t voxel(uint32_t x, uint32_t y, uint32_t z) const {
        if (x >= ex || y >= ey || z >= ez) return 0;
        const uint64_t at = ((uint64_t)z * ey + y) * ex + x;
        const uint32_t c = albedo[at];
        return (uint64_t)((c >> 24) ? c : 0u) | ((uint64_t)data[at] << 32);
    }
};

// Palette in first-appearance order of the reference insert loop (x outer, y, z inner), slab by slab: the order a
// procedural scene is evaluated in.
static void palette_by_slabs(const SceneSource &src, int threads, std::vector<uint32_t> &palette) {
    std::vector<std::vector<uint32_t>> slab_colors(src.ex);
    parallel_for(src.ex, threads, [&](int64_t x) {
        std::unordered_set<uint32_t> seen;
        uint32_t last = 0;
        for (uint32_t y = 0; y < src.ey; ++y)
            for (uint32_t z = 0; z < src.ez; ++z) {
                uint32_t c = src.voxel((uint32_t)x, y, z);
                if (c == 0 || c == last) continue;
                last = c;
                if (seen.insert(c).second) slab_colors[x].push_back(c);
            }
    });
    std::unordered_set<uint32_t> seen;
    for (auto &sl : slab_colors)
        for (uint32_t c : sl)
            if (seen.insert(c).second) palette.push_back(c);
}

// The same palette for a dense grid, read in memory order (x runs fastest there, and the insert loop's z-inner walk
// would touch a cache line per voxel): every colour's smallest insert-order index (x*gy + y)*gz + z, z plane by z plane,
// then the colours sorted by it. A voxel whose left neighbour has its colour is skipped (the neighbour's index is smaller).
// `half(x, y, z)` is the colour of the voxel, or, for the data palette, its data value; 0 = none in both.
template <class Source, class Half>
static int palette_by_first_index(const Source &src, int threads, Half half, std::vector<uint32_t> &palette) {
    std::vector<std::unordered_map<uint32_t, uint64_t>> plane(src.ez);
    parallel_for(src.ez, threads, [&](int64_t z) {
        auto &first = plane[z];
        for (uint32_t y = 0; y < src.ey; ++y) {
            uint32_t last = 0;
            for (uint32_t x = 0; x < src.ex; ++x) {
                const uint32_t c = half(x, y, (uint32_t)z);
                if (c == last) continue;
                last = c;
                if (c == 0) continue;
                const uint64_t idx = ((uint64_t)x * src.ey + y) * src.ez + (uint64_t)z;
                auto it = first.emplace(c, idx);
                if (!it.second && idx < it.first->second) it.first->second = idx;
            }
        }
    });
    std::unordered_map<uint32_t, uint64_t> first;
    for (auto &pl : plane) {
        for (auto &kv : pl) {
            auto it = first.emplace(kv.first, kv.second);
            if (!it.second && kv.second < it.first->second) it.first->second = kv.second;
        }
        pl.clear();
        if (first.size() > 0xFFFFu) return VHX_E_CAPACITY;  // 16-bit palette index, 0xFFFF = none
    }
    std::vector<std::pair<uint64_t, uint32_t>> order;
    order.reserve(first.size());
    for (auto &kv : first) order.emplace_back(kv.second, kv.first);
    std::sort(order.begin(), order.end());
    for (auto &o : order) palette.push_back(o.second);
    return VHX_OK;
}

// Writes the canonical image of `src` into *f, whose size, brick_dim and palettes are set. A source's voxel() is the
// albedo, with the data value in the high word where the source has a data plane.
template <class Source>
static int build_image(const Source &sc, int threads, vhx_flat *f) {
    const uint32_t S = f->size, bd = f->brick_dim;
    const uint32_t L = 4 * bd;         // leaf node edge
    const uint32_t nl = S / L;         // leaf nodes per axis = 4^D
    uint32_t D = 0;
    while ((1u << (2 * D)) < nl) ++D;  // nl == 4^D
    const uint64_t nleaf = 1ull << (6 * D);

    std::unordered_map<uint32_t, uint32_t> color_index;
    for (uint32_t c : f->color_palette) color_index.emplace(c, (uint32_t)color_index.size());
    std::unordered_map<uint32_t, uint32_t> data_index;
    for (uint32_t d : f->data_palette) data_index.emplace(d, (uint32_t)data_index.size());

    // leaf path code -> leaf coordinates (digit i of the code = sectant taken at depth i)
    auto leaf_coord = [&](uint64_t code, uint32_t &lx, uint32_t &ly, uint32_t &lz) {
        lx = ly = lz = 0;
        for (uint32_t i = 0; i < D; ++i) {
            uint32_t d = (uint32_t)((code >> (6 * (D - 1 - i))) & 63u);
            lx = lx * 4 + (d & 3u);
            ly = ly * 4 + ((d >> 2) & 3u);
            lz = lz * 4 + (d >> 4);
        }
    };
    // 2) brick masks of every leaf node
    std::vector<uint64_t> leaf_mask(nleaf, 0);
    parallel_for((int64_t)nleaf, threads, [&](int64_t code) {
        uint32_t lx, ly, lz;
        leaf_coord((uint64_t)code, lx, ly, lz);
        uint32_t x0 = lx * L, y0 = ly * L, z0 = lz * L;
        if (x0 >= sc.ex || y0 >= sc.ey || z0 >= sc.ez) return;
        uint64_t m = 0;
        for (uint32_t s = 0; s < 64; ++s) {
            uint32_t bx = x0 + (s & 3u) * bd, by = y0 + ((s >> 2) & 3u) * bd, bz = z0 + (s >> 4) * bd;
            bool any = false;
            for (uint32_t x = bx; x < bx + bd && !any; ++x)
                for (uint32_t y = by; y < by + bd && !any; ++y)
                    for (uint32_t z = bz; z < bz + bd && !any; ++z) any = sc.voxel(x, y, z) != 0;
            if (any) m |= 1ull << s;
        }
        leaf_mask[code] = m;
    });
    // 3) presence per level (level D = leaves), BFS numbering level by level in path order
    std::vector<std::vector<uint64_t>> occ(D + 1);  // occupancy bits of every possible node per level
    occ[D] = leaf_mask;
    for (int lv = (int)D - 1; lv >= 0; --lv) {
        occ[lv].assign(1ull << (6 * lv), 0);
        for (uint64_t c = 0; c < occ[lv + 1].size(); ++c)
            if (occ[lv + 1][c]) occ[lv][c >> 6] |= 1ull << (c & 63);
    }
    std::vector<std::vector<uint32_t>> bfs(D + 1);  // BFS index of each present node per level
    uint32_t next = 0;
    for (uint32_t lv = 0; lv <= D; ++lv) {
        bfs[lv].assign(occ[lv].size(), VHX_EMPTY);
        for (uint64_t c = 0; c < occ[lv].size(); ++c)
            if (occ[lv][c] || (lv == 0)) bfs[lv][c] = next++;
    }
    const uint32_t node_count = next;
    f->node_type.assign(node_count, VHX_NODE_INTERNAL);
    f->node_ocbits.assign(node_count, 0);
    f->node_children.assign((size_t)node_count * 64, VHX_EMPTY);
    for (uint32_t lv = 0; lv <= D; ++lv)
        for (uint64_t c = 0; c < occ[lv].size(); ++c) {
            uint32_t i = bfs[lv][c];
            if (i == VHX_EMPTY) continue;
            f->node_ocbits[i] = occ[lv][c];
            if (lv < D) {
                f->node_type[i] = occ[lv][c] ? VHX_NODE_INTERNAL : VHX_NODE_NOTHING;
                for (uint32_t s = 0; s < 64; ++s) f->node_children[(size_t)i * 64 + s] = bfs[lv + 1][(c << 6) | s];
            } else {
                f->node_type[i] = occ[lv][c] ? VHX_NODE_LEAF : VHX_NODE_NOTHING;
            }
        }
    // 4) bricks numbered in (leaf BFS order, sectant) order; fill voxels
    std::vector<uint64_t> leaf_first(nleaf + 1, 0);
    for (uint64_t c = 0; c < nleaf; ++c) leaf_first[c + 1] = leaf_first[c] + (uint64_t)__builtin_popcountll(leaf_mask[c]);
    const uint64_t nbricks = leaf_first[nleaf];
    if (nbricks >= 0x80000000ull) return VHX_E_CAPACITY;
    const size_t n3 = (size_t)bd * bd * bd;
    f->brick_count = (uint32_t)nbricks;
    f->voxel_count = nbricks * n3;
    f->voxels.reset(new (std::nothrow) uint32_t[std::max<uint64_t>(f->voxel_count, 1)]);
    if (!f->voxels) return VHX_E_CAPACITY;
    uint32_t *vox = f->voxels.get();
    parallel_for((int64_t)nleaf, threads, [&](int64_t code) {
        uint64_t m = leaf_mask[code];
        if (!m) return;
        uint32_t li = bfs[D][code];
        uint32_t lx, ly, lz;
        leaf_coord((uint64_t)code, lx, ly, lz);
        uint64_t b = leaf_first[code];
        decltype(sc.voxel(0, 0, 0)) last_c = 0;
        uint32_t last_v = VHX_EMPTY;
        for (uint32_t s = 0; s < 64; ++s) {
            if (!((m >> s) & 1ull)) continue;
            f->node_children[(size_t)li * 64 + s] = (uint32_t)b;
            uint32_t bx = lx * L + (s & 3u) * bd, by = ly * L + ((s >> 2) & 3u) * bd, bz = lz * L + (s >> 4) * bd;
            uint32_t *dst = vox + b * n3;
            for (uint32_t z = 0; z < bd; ++z)
                for (uint32_t y = 0; y < bd; ++y)
                    for (uint32_t x = 0; x < bd; ++x) {
                        const auto c = sc.voxel(bx + x, by + y, bz + z);
                        uint32_t v = VHX_EMPTY;
                        if (c != 0) {
                            if (c != last_c) {
                                last_c = c;
                                // pix_visual, pix_informative or pix_complex: 0xFFFF for the half that is none
                                const uint32_t a = (uint32_t)c, d = (uint32_t)((uint64_t)c >> 32);
                                last_v = (a ? color_index.at(a) : 0xFFFFu) | ((d ? data_index.at(d) : 0xFFFFu) << 16);
                            }
                            v = last_v;
                        }
                        dst[x + y * bd + z * bd * bd] = v;
                    }
            ++b;
        }
    });
    return VHX_OK;
}

static int check_sizes(uint32_t S, uint32_t bd) {
    BoxTree *probe = nullptr;
    int rc = BoxTree::create(S, bd, &probe);  // same validity rules as BoxTree::new
    if (rc != 0) return rc;
    delete probe;
    return VHX_OK;
}

static int build_scene(uint32_t scene_id, uint32_t S, uint32_t bd, uint64_t seed, int threads, vhx_flat **out) {
    int rc = check_sizes(S, bd);
    if (rc != 0) return rc;
    Scene sc{scene_id, S, seed, S, {}};
    sc.prepare();
    SceneSource src(sc);
    std::unique_ptr<vhx_flat> f(new vhx_flat());
    f->size = S;
    f->brick_dim = bd;
    palette_by_slabs(src, threads, f->color_palette);
    if ((rc = build_image(src, threads, f.get())) != 0) return rc;
    *out = f.release();
    return VHX_OK;
}

static int build_dense(const vhx_dense_desc *g, const uint32_t *data, int threads, vhx_flat **out) {
    if (!g) return VHX_E_INVALID_ARG;
    int rc = check_sizes(g->boxtree_size, g->brick_dim);
    if (rc != 0) return rc;
    const uint32_t S = g->boxtree_size;
    if (!g->albedo || g->gx == 0 || g->gy == 0 || g->gz == 0 || g->gx > S || g->gy > S || g->gz > S)
        return VHX_E_INVALID_ARG;
    std::unique_ptr<vhx_flat> f(new vhx_flat());
    f->size = S;
    f->brick_dim = g->brick_dim;
    if (data) {  // each palette in first-appearance order of its own half
        DenseDataSource src{g->albedo, data, g->gx, g->gy, g->gz};
        const auto color = [&](uint32_t x, uint32_t y, uint32_t z) { return (uint32_t)src.voxel(x, y, z); };
        const auto datum = [&](uint32_t x, uint32_t y, uint32_t z) { return (uint32_t)(src.voxel(x, y, z) >> 32); };
        if ((rc = palette_by_first_index(src, threads, color, f->color_palette)) != 0) return rc;
        if ((rc = palette_by_first_index(src, threads, datum, f->data_palette)) != 0) return rc;
        if ((rc = build_image(src, threads, f.get())) != 0) return rc;
    } else {
        DenseSource src{g->albedo, g->gx, g->gy, g->gz};
        const auto color = [&](uint32_t x, uint32_t y, uint32_t z) { return src.voxel(x, y, z); };
        if ((rc = palette_by_first_index(src, threads, color, f->color_palette)) != 0) return rc;
        if ((rc = build_image(src, threads, f.get())) != 0) return rc;
    }
    *out = f.release();
    return VHX_OK;
}

// ---------------------------------------------------------------------------------------------- compaction
// The image without its unreachable slots, in the builders' numbering: nodes breadth-first from the
// root, level by level in (parent's new index, sectant) order; Parted bricks in (owning node's new index, sectant)
// order. Reachability goes by the entries, never by occupied_bits. The CPU reference of vhx_compact_tree.
static constexpr uint32_t COMPACT_MAX_LEVELS = 8;  // node levels, as the device builders' MAX_LEVELS

static int compact_image(const vhx_tree_desc &t, vhx_flat **out) {
    const uint32_t nn = t.node_count, nb = t.brick_count;
    const uint64_t n3 = (uint64_t)t.brick_dim * t.brick_dim * t.brick_dim;
    if (nn == 0 || n3 == 0 || !t.node_type || !t.node_ocbits || !t.node_children || (nb && !t.voxels) ||
        (t.solid_count && !t.solid_values) || (t.color_count && !t.color_palette) || (t.data_count && !t.data_palette))
        return VHX_E_INVALID_ARG;
    std::vector<uint32_t> new_of(nn, VHX_EMPTY), old_of{0};
    new_of[0] = 0;
    uint32_t levels = 0;
    for (size_t begin = 0; begin < old_of.size();) {
        if (++levels > COMPACT_MAX_LEVELS) return VHX_E_TREE_INVALID_STRUCTURE;
        const size_t end = old_of.size();
        for (size_t i = begin; i < end; ++i) {
            const uint32_t o = old_of[i];
            if (t.node_type[o] != VHX_NODE_INTERNAL) continue;
            for (uint32_t s = 0; s < 64; ++s) {
                const uint32_t e = t.node_children[(size_t)o * 64 + s];
                if (e == VHX_EMPTY) continue;
                if (e >= nn || new_of[e] != VHX_EMPTY) return VHX_E_TREE_INVALID_STRUCTURE;  // past the count, or twice
                new_of[e] = (uint32_t)old_of.size();
                old_of.push_back(e);
            }
        }
        begin = end;
    }
    auto parted = [](uint32_t e) { return e != VHX_EMPTY && (e & VHX_SOLID_BIT) == 0; };
    std::vector<uint32_t> brick_new(nb, VHX_EMPTY), brick_src;
    for (uint32_t o : old_of) {
        const uint32_t ty = t.node_type[o];
        const uint32_t entries = ty == VHX_NODE_LEAF ? 64u : ty == VHX_NODE_UNIFORM_LEAF ? 1u : 0u;
        for (uint32_t s = 0; s < entries; ++s) {
            const uint32_t e = t.node_children[(size_t)o * 64 + s];
            if (!parted(e)) continue;
            if (e >= nb || brick_new[e] != VHX_EMPTY) return VHX_E_TREE_INVALID_STRUCTURE;
            brick_new[e] = (uint32_t)brick_src.size();
            brick_src.push_back(e);
        }
    }
    std::unique_ptr<vhx_flat> f(new vhx_flat());
    f->size = t.boxtree_size;
    f->brick_dim = t.brick_dim;
    const size_t n = old_of.size();
    f->node_type.resize(n);
    f->node_ocbits.resize(n);
    f->node_children.resize(n * 64);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t o = old_of[i], ty = t.node_type[o];
        f->node_type[i] = ty;
        f->node_ocbits[i] = t.node_ocbits[o];
        const uint32_t entries = ty == VHX_NODE_LEAF ? 64u : ty == VHX_NODE_UNIFORM_LEAF ? 1u : 0u;
        for (uint32_t s = 0; s < 64; ++s) {
            uint32_t e = t.node_children[(size_t)o * 64 + s];
            if (ty == VHX_NODE_INTERNAL) {
                if (e != VHX_EMPTY) e = new_of[e];
            } else if (s < entries && parted(e)) {
                e = brick_new[e];
            }
            f->node_children[i * 64 + s] = e;
        }
    }
    f->brick_count = (uint32_t)brick_src.size();
    f->voxel_count = (uint64_t)brick_src.size() * n3;
    f->voxels.reset(new uint32_t[std::max<uint64_t>(f->voxel_count, 1)]);
    for (size_t j = 0; j < brick_src.size(); ++j)
        std::memcpy(&f->voxels[j * n3], t.voxels + (size_t)brick_src[j] * n3, n3 * 4);
    f->solid_values.assign(t.solid_values, t.solid_values + t.solid_count);
    f->color_palette.assign(t.color_palette, t.color_palette + t.color_count);
    f->data_palette.assign(t.data_palette, t.data_palette + t.data_count);
    *out = f.release();
    return VHX_OK;
}

// ---------------------------------------------------------------------------------------------- palette
// The image with the palettes the builders give the voxels it holds now (include/vhx_boxtree.h
// states the rules): per selected half (VHX_PALETTE_COLOR, VHX_PALETTE_DATA) the used entries by the first index of the
// cubes that hold them, every cell and solid value translated, nothing else touched. One walk serves both halves. The
// CPU reference of vhx_compact_palettes (and, with the colour half alone, of vhx_compact_palette).
static int palettes_image(const vhx_tree_desc &t, uint32_t which, vhx_flat **out) {
    const uint32_t nn = t.node_count, nb = t.brick_count, bd = t.brick_dim;
    const uint64_t n3 = (uint64_t)bd * bd * bd, S = t.boxtree_size;
    if (nn == 0 || n3 == 0 || !t.node_type || !t.node_ocbits || !t.node_children || (nb && !t.voxels) ||
        (t.solid_count && !t.solid_values) || (t.color_count && !t.color_palette) || (t.data_count && !t.data_palette))
        return VHX_E_INVALID_ARG;
    const bool do_color = (which & VHX_PALETTE_COLOR) != 0, do_data = (which & VHX_PALETTE_DATA) != 0;
    // per palette entry of a half: the smallest first index of a value naming it
    std::vector<uint64_t> first(do_color ? 0x10000 : 0, ~0ull), dfirst(do_data ? 0x10000 : 0, ~0ull);
    auto see = [&](uint32_t v, uint64_t x, uint64_t y, uint64_t z) {
        const uint32_t ci = v & 0xFFFFu, di = v >> 16;
        const uint64_t idx = (x * S + y) * S + z;
        if (do_color && ci != 0xFFFFu) first[ci] = std::min(first[ci], idx);
        if (do_data && di != 0xFFFFu) dfirst[di] = std::min(dfirst[di], idx);
    };
    struct At {
        uint32_t node, level;
        uint64_t x, y, z;
    };
    std::vector<At> order{{0, 0, 0, 0, 0}};
    std::vector<uint8_t> seen_node(nn, 0), seen_brick(nb, 0);
    seen_node[0] = 1;
    for (size_t i = 0; i < order.size(); ++i) {
        const At a = order[i];
        if (a.level >= COMPACT_MAX_LEVELS) return VHX_E_TREE_INVALID_STRUCTURE;
        const uint32_t ty = t.node_type[a.node];
        const uint64_t size = S >> (2 * a.level), quarter = size >> 2;
        const uint32_t *ent = t.node_children + (size_t)a.node * 64;
        if (ty == VHX_NODE_INTERNAL) {
            for (uint32_t s = 0; s < 64; ++s) {
                const uint32_t e = ent[s];
                if (e == VHX_EMPTY) continue;
                if (e >= nn || seen_node[e]) return VHX_E_TREE_INVALID_STRUCTURE;  // past the count, or twice
                seen_node[e] = 1;
                order.push_back({e, a.level + 1, a.x + (s & 3u) * quarter, a.y + ((s >> 2) & 3u) * quarter,
                                 a.z + (s >> 4) * quarter});
            }
            continue;
        }
        const bool uniform = ty == VHX_NODE_UNIFORM_LEAF;
        if (!uniform && ty != VHX_NODE_LEAF) continue;
        const uint64_t edge = uniform ? size : quarter, cell = edge / bd;  // of a brick, of one of its cells
        if (cell == 0) return VHX_E_TREE_INVALID_STRUCTURE;  // a brick below the voxel lattice
        for (uint32_t s = 0; s < (uniform ? 1u : 64u); ++s) {
            const uint32_t e = ent[s];
            if (e == VHX_EMPTY) continue;
            const uint64_t bx = a.x + (s & 3u) * edge, by = a.y + ((s >> 2) & 3u) * edge, bz = a.z + (s >> 4) * edge;
            if (e & VHX_SOLID_BIT) {
                if ((e & ~VHX_SOLID_BIT) >= t.solid_count) return VHX_E_TREE_INVALID_STRUCTURE;
                see(t.solid_values[e & ~VHX_SOLID_BIT], bx, by, bz);
                continue;
            }
            if (e >= nb || seen_brick[e]) return VHX_E_TREE_INVALID_STRUCTURE;
            seen_brick[e] = 1;
            const uint32_t *cells = t.voxels + (size_t)e * n3;
            for (uint32_t cz = 0, c = 0; cz < bd; ++cz)
                for (uint32_t cy = 0; cy < bd; ++cy)
                    for (uint32_t cx = 0; cx < bd; ++cx, ++c) see(cells[c], bx + cx * cell, by + cy * cell, bz + cz * cell);
        }
    }
    // One half: entries of one value are one value; an entry the half's test rejects (alpha 0, the value 0) names none.
    // Leaves the new palette in `pal` and the map old index -> new index, 0xFFFF where the entry names nothing
    auto settle = [](const uint32_t *old, uint32_t count, const std::vector<uint64_t> &fst, bool data,
                     std::vector<uint32_t> &pal, std::vector<uint32_t> &map) {
        const uint32_t n = std::min<uint32_t>(count, 0xFFFFu);  // what a 16-bit index can name
        const auto names = [&](uint32_t e) { return data ? e != 0 : (e >> 24) != 0; };
        std::unordered_map<uint32_t, uint64_t> value_first;
        for (uint32_t i = 0; i < n; ++i) {
            if (fst[i] == ~0ull || !names(old[i])) continue;
            auto it = value_first.emplace(old[i], fst[i]).first;
            it->second = std::min(it->second, fst[i]);
        }
        std::vector<std::pair<uint64_t, uint32_t>> ranked;
        ranked.reserve(value_first.size());
        for (const auto &kv : value_first) ranked.emplace_back(kv.second, kv.first);
        std::sort(ranked.begin(), ranked.end());
        std::unordered_map<uint32_t, uint32_t> index_of;
        for (size_t r = 0; r < ranked.size(); ++r) index_of[ranked[r].second] = (uint32_t)r;
        map.assign(0x10000, 0xFFFFu);
        for (uint32_t i = 0; i < n; ++i) {
            if (!names(old[i])) continue;
            const auto it = index_of.find(old[i]);
            if (it != index_of.end()) map[i] = it->second;
        }
        pal.resize(ranked.size());
        for (size_t r = 0; r < ranked.size(); ++r) pal[r] = ranked[r].second;
    };
    std::unique_ptr<vhx_flat> f(new vhx_flat());
    std::vector<uint32_t> map, dmap;
    if (do_color)
        settle(t.color_palette, t.color_count, first, false, f->color_palette, map);
    else
        f->color_palette.assign(t.color_palette, t.color_palette + t.color_count);
    if (do_data)
        settle(t.data_palette, t.data_count, dfirst, true, f->data_palette, dmap);
    else
        f->data_palette.assign(t.data_palette, t.data_palette + t.data_count);
    auto mapped = [&](uint32_t v) {
        const uint32_t lo = do_color ? map[v & 0xFFFFu] : v & 0xFFFFu, hi = do_data ? dmap[v >> 16] : v >> 16;
        return lo | hi << 16;
    };

    f->size = t.boxtree_size;
    f->brick_dim = bd;
    f->node_type.assign(t.node_type, t.node_type + nn);
    f->node_ocbits.assign(t.node_ocbits, t.node_ocbits + nn);
    f->node_children.assign(t.node_children, t.node_children + (size_t)nn * 64);
    f->brick_count = nb;
    f->voxel_count = (uint64_t)nb * n3;
    f->voxels.reset(new uint32_t[std::max<uint64_t>(f->voxel_count, 1)]);
    for (uint64_t i = 0; i < f->voxel_count; ++i) f->voxels[i] = mapped(t.voxels[i]);  // orphaned slots included
    f->solid_values.resize(t.solid_count);
    for (uint32_t i = 0; i < t.solid_count; ++i) f->solid_values[i] = mapped(t.solid_values[i]);
    *out = f.release();
    return VHX_OK;
}

// ---------------------------------------------------------------------------------------------- vhx_flat_list_voxels
// The plain walk of vhx_list_voxels (include/vhx.h): depth-first, sectants ascending, cells in flat order, clipped to the
// box. Run once to count and to find a refusal, then once more to write, so that a refused call writes nothing.
namespace {
struct ListWalk {
    const vhx_tree_desc &t;
    const vhx_points_out &q;
    uint32_t lg_bd = 0, levels = 0;
    bool write = false, bad = false;
    uint64_t total = 0;

    bool meets(uint32_t x, uint32_t y, uint32_t z, uint32_t edge) const {
        return x < q.ox + q.gx && x + edge > q.ox && y < q.oy + q.gy && y + edge > q.oy && z < q.oz + q.gz &&
               z + edge > q.oz;
    }
    uint32_t albedo_of(uint32_t v) const {
        const uint32_t ci = v & 0xFFFFu;
        if (ci == 0xFFFFu || ci >= t.color_count || !t.color_palette) return 0u;
        const uint32_t a = t.color_palette[ci];
        return (a >> 24) != 0u ? a : 0u;
    }
    uint32_t data_of(uint32_t v) const {
        const uint32_t di = v >> 16;
        if (v == VHX_EMPTY || di == 0xFFFFu || di >= t.data_count || !t.data_palette) return 0u;
        return t.data_palette[di];
    }
    // the cells of the brick-sized cube at (X, Y, Z), sectant s of the smallest leaf `node`
    void unit(uint32_t node, bool uniform, uint32_t s, uint32_t X, uint32_t Y, uint32_t Z) {
        const uint32_t bd = t.brick_dim, m = bd - 1u;
        const uint32_t desc = t.node_children[(uint64_t)node * 64u + (uniform ? 0u : s)];
        if (desc == VHX_EMPTY) return;
        const bool solid = (desc & VHX_SOLID_BIT) != 0u;
        uint32_t sv = VHX_EMPTY;
        if (solid) {
            const uint32_t i = desc & 0x7FFFFFFFu;
            if (i < t.solid_count && t.solid_values) sv = t.solid_values[i];
        } else if (desc >= t.brick_count || !t.voxels) {
            return;
        }
        const uint32_t *brick = solid ? nullptr : t.voxels + ((uint64_t)desc << (3u * lg_bd));
        for (uint32_t flat = 0; flat < bd * bd * bd; ++flat) {
            const uint32_t cx = flat & m, cy = (flat >> lg_bd) & m, cz = flat >> (2u * lg_bd);
            const uint32_t x = X + cx, y = Y + cy, z = Z + cz;
            if (x - q.ox >= q.gx || y - q.oy >= q.gy || z - q.oz >= q.gz) continue;
            uint32_t v = sv;
            if (!solid) {
                if (uniform) {  // the brick spans the leaf: a cell is 4 voxels wide, and comes back raw
                    const uint32_t um = 4u * bd - 1u;
                    v = brick[((x & um) >> 2) + ((((y & um) >> 2) + (((z & um) >> 2) << lg_bd)) << lg_bd)];
                } else {
                    v = brick[flat];
                }
            }
            const uint32_t a = albedo_of(v), d = data_of(v);
            if (a == 0u && d == 0u) continue;
            if (write && total < q.capacity) {
                if (q.positions) {
                    q.positions[3 * total] = x;
                    q.positions[3 * total + 1] = y;
                    q.positions[3 * total + 2] = z;
                }
                if (q.albedo) q.albedo[total] = a;
                if (q.data) q.data[total] = d;
            }
            ++total;
        }
    }
    void walk(uint32_t node, uint32_t lvl, uint32_t X, uint32_t Y, uint32_t Z, uint32_t lg) {
        const uint32_t type = t.node_type[node], edge = 1u << (lg - 2u);
        if (type != VHX_NODE_INTERNAL && type != VHX_NODE_LEAF && type != VHX_NODE_UNIFORM_LEAF) return;
        if (type != VHX_NODE_INTERNAL && lvl + 1u != levels) {  // a brick stretched over a larger cube
            bad = true;
            return;
        }
        if (type == VHX_NODE_INTERNAL && lvl + 1u >= levels) return;  // no node is smaller than 4 * brick_dim
        for (uint32_t s = 0; s < 64u && !bad; ++s) {
            const uint32_t x = X + (s & 3u) * edge, y = Y + ((s >> 2) & 3u) * edge, z = Z + (s >> 4) * edge;
            if (!meets(x, y, z, edge)) continue;
            if (type == VHX_NODE_INTERNAL) {
                const uint32_t e = t.node_children[(uint64_t)node * 64u + s];
                if (e != VHX_EMPTY && e < t.node_count) walk(e, lvl + 1u, x, y, z, lg - 2u);
            } else {
                unit(node, type == VHX_NODE_UNIFORM_LEAF, s, x, y, z);
            }
        }
    }
};
}  // namespace

static int list_image(const vhx_tree_desc &t, const vhx_points_out &q) {
    const uint32_t S = t.boxtree_size, bd = t.brick_dim;
    if (!t.node_type || !t.node_children || t.node_count == 0) return VHX_E_INVALID_ARG;
    uint32_t lg_size = 0, lg_bd = 0;
    while (lg_size < 31u && (1u << lg_size) < S) ++lg_size;
    while (lg_bd < 31u && (1u << lg_bd) < bd) ++lg_bd;
    if (S == 0 || bd == 0 || (1u << lg_size) != S || (1u << lg_bd) != bd || lg_size < lg_bd + 2u ||
        ((lg_size - lg_bd) & 1u))
        return VHX_E_INVALID_ARG;
    if (q.gx == 0 || q.gy == 0 || q.gz == 0 || (uint64_t)q.ox + q.gx > S || (uint64_t)q.oy + q.gy > S ||
        (uint64_t)q.oz + q.gz > S)
        return VHX_E_INVALID_ARG;
    const uint64_t lim = 1ull << 48, gxy = (uint64_t)q.gx * q.gy;
    if (gxy >= lim || q.gz > (lim - 1u) / gxy) return VHX_E_CAPACITY;
    if (lg_bd > 10u) return VHX_E_CAPACITY;  // a brick's cells are counted in 32 bits
    ListWalk w{t, q};
    w.lg_bd = lg_bd;
    w.levels = (lg_size - lg_bd) / 2u;
    w.walk(0, 0, 0, 0, 0, lg_size);
    if (w.bad) return VHX_E_STATE;
    const uint64_t total = w.total;
    if (q.capacity > 0 && total > 0 && (q.positions || q.albedo || q.data)) {
        w.write = true;
        w.total = 0;
        w.walk(0, 0, 0, 0, 0, lg_size);
    }
    *q.count = total;
    return VHX_OK;
}

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" {

int vhx_boxtree_new(uint32_t size, uint32_t brick_dim, vhx_boxtree **out) {
    if (!out) return VHX_E_INVALID_ARG;
    BoxTree *t = nullptr;
    int rc = BoxTree::create(size, brick_dim, &t);
    if (rc != 0) return rc;
    *out = new vhx_boxtree{t};
    return VHX_OK;
}
void vhx_boxtree_free(vhx_boxtree *tree) {
    if (!tree) return;
    delete tree->tree;
    delete tree;
}
int vhx_boxtree_set_auto_simplify(vhx_boxtree *tree, int enabled) {
    if (!tree) return VHX_E_INVALID_ARG;
    tree->tree->auto_simplify = enabled != 0;
    return VHX_OK;
}
int vhx_boxtree_insert(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t kind, uint32_t albedo,
                       uint32_t data) {
    if (!tree || kind > VHX_ENTRY_COMPLEX) return VHX_E_INVALID_ARG;
    return tree->tree->insert(U3{x, y, z}, Entry{kind, albedo, data});
}
int vhx_boxtree_insert_at_lod(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t insert_size,
                              uint32_t kind, uint32_t albedo, uint32_t data) {
    if (!tree || kind > VHX_ENTRY_COMPLEX) return VHX_E_INVALID_ARG;
    return tree->tree->insert_at_lod(U3{x, y, z}, insert_size, Entry{kind, albedo, data});
}
int vhx_boxtree_update(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t kind, uint32_t albedo,
                       uint32_t data) {
    if (!tree || kind > VHX_ENTRY_COMPLEX) return VHX_E_INVALID_ARG;
    return tree->tree->update(U3{x, y, z}, Entry{kind, albedo, data});
}
int vhx_boxtree_clear(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z) {
    if (!tree) return VHX_E_INVALID_ARG;
    return tree->tree->clear(U3{x, y, z});
}
int vhx_boxtree_clear_at_lod(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t clear_size) {
    if (!tree) return VHX_E_INVALID_ARG;
    return tree->tree->clear_at_lod(U3{x, y, z}, clear_size);
}
int vhx_boxtree_get(const vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t *kind, uint32_t *albedo,
                    uint32_t *data) {
    if (!tree || !kind || !albedo || !data) return VHX_E_INVALID_ARG;
    Entry e = tree->tree->get(U3{x, y, z});
    *kind = e.kind;
    *albedo = e.albedo;
    *data = e.data;
    return VHX_OK;
}
int vhx_boxtree_node_info(const vhx_boxtree *tree, float x, float y, float z, uint64_t *key, uint32_t *content,
                          uint64_t *occupied_bits, uint32_t *occlusion_bits) {
    if (!tree || !key || !content || !occupied_bits || !occlusion_bits) return VHX_E_INVALID_ARG;
    const BoxTree &t = *tree->tree;
    const float S = (float)t.boxtree_size;
    if (!(x >= 0.f && y >= 0.f && z >= 0.f && x < S && y < S && z < S)) return VHX_E_TREE_INVALID_POSITION;
    Cube bounds{F3{0.f, 0.f, 0.f}, S};
    const size_t k = t.get_node_internal(0, bounds, F3{x, y, z});
    if (k == SIZE_MAX) return VHX_E_TREE_INVALID_POSITION;
    const Node &n = t.nodes.get(k);
    *key = k;
    *content = (uint32_t)n.content;
    *occupied_bits = n.occupied_bits;
    *occlusion_bits = n.occlusion_bits;
    return VHX_OK;
}

int vhx_boxtree_simplify(vhx_boxtree *tree, int recursive) {
    if (!tree) return VHX_E_INVALID_ARG;
    tree->tree->simplify(0, recursive != 0);
    return VHX_OK;
}
int vhx_boxtree_info(const vhx_boxtree *tree, uint32_t info[5]) {
    if (!tree || !info) return VHX_E_INVALID_ARG;
    info[0] = tree->tree->boxtree_size;
    info[1] = tree->tree->brick_dim;
    info[2] = (uint32_t)tree->tree->nodes.len();
    info[3] = (uint32_t)tree->tree->color_palette.size();
    info[4] = (uint32_t)tree->tree->data_palette.size();
    return VHX_OK;
}
int vhx_scene_insert(vhx_boxtree *tree, uint32_t scene, uint64_t seed) {
    if (!tree || !scene_valid(scene)) return VHX_E_INVALID_ARG;
    Scene sc{scene, tree->tree->boxtree_size, seed, 0, {}};
    sc.prepare();
    for (uint32_t x = 0; x < sc.extent; ++x)
        for (uint32_t y = 0; y < sc.extent; ++y)
            for (uint32_t z = 0; z < sc.extent; ++z) {
                uint32_t c = sc.voxel(x, y, z);
                if (c == 0) continue;
                int rc = tree->tree->insert(U3{x, y, z}, Entry{VHX_ENTRY_VISUAL, c, 0});
                if (rc != 0) return rc;
            }
    return VHX_OK;
}
int vhx_boxtree_flatten(const vhx_boxtree *tree, vhx_flat **out) {
    if (!tree || !out) return VHX_E_INVALID_ARG;
    *out = flatten_tree(*tree->tree, 0xFFFFFFFFu, tree->tree->mip_strategy.enabled);
    return VHX_OK;
}
int vhx_boxtree_flatten_lod(const vhx_boxtree *tree, uint32_t max_depth, vhx_flat **out) {
    if (!tree || !out) return VHX_E_INVALID_ARG;
    *out = flatten_tree(*tree->tree, max_depth, true);
    return VHX_OK;
}
int vhx_flat_node_mips(const vhx_flat *f, const uint32_t **node_mips, uint32_t *count) {
    if (!f || !node_mips || !count) return VHX_E_INVALID_ARG;
    *node_mips = f->node_mips.empty() ? nullptr : f->node_mips.data();
    *count = (uint32_t)f->node_mips.size();
    return VHX_OK;
}
int vhx_boxtree_switch_mips(vhx_boxtree *tree, int enabled) {
    if (!tree) return VHX_E_INVALID_ARG;
    tree->tree->switch_albedo_mip_maps(enabled != 0);
    return VHX_OK;
}
int vhx_boxtree_set_mip_method(vhx_boxtree *tree, uint32_t level, uint32_t method, float threshold) {
    if (!tree || method > VHX_MIP_POSTERIZE_BD || !(threshold == threshold)) return VHX_E_INVALID_ARG;
    // set_method_at_internal (mipmap.rs:414-431): Posterize thresholds are clamped to [0, 1]
    if (method == VHX_MIP_POSTERIZE || method == VHX_MIP_POSTERIZE_BD) threshold = std::clamp(threshold, 0.f, 1.f);
    tree->tree->mip_strategy.methods[level] = MipMethodCfg{method, threshold};
    return VHX_OK;
}
int vhx_boxtree_set_mip_color_threshold(vhx_boxtree *tree, uint32_t level, float threshold) {
    if (!tree || !(threshold == threshold)) return VHX_E_INVALID_ARG;
    // set_color_similarity_thr_internal (mipmap.rs:365-379): clamped to [0, 1]
    tree->tree->mip_strategy.color_thresholds[level] = std::clamp(threshold, 0.f, 1.f);
    return VHX_OK;
}
int vhx_boxtree_set_mip_options(int direct, int threads) {
    if (threads < 0 || threads > 256) return VHX_E_INVALID_ARG;
    g_mip_direct.store(direct ? 1 : 0);
    g_mip_threads.store(threads);
    return VHX_OK;
}
int vhx_boxtree_recalculate_mips(vhx_boxtree *tree) {
    if (!tree) return VHX_E_INVALID_ARG;
    if (tree->tree->nodes.get(0).content != Content::Nothing) tree->tree->recalculate_mips();
    return VHX_OK;
}
int vhx_boxtree_sample_root_mip(const vhx_boxtree *tree, uint32_t sectant, uint32_t x, uint32_t y, uint32_t z,
                                uint32_t *kind, uint32_t *albedo, uint32_t *data) {
    const uint32_t bd = tree ? tree->tree->brick_dim : 0;
    if (!tree || !kind || !albedo || !data || sectant > 64 || x >= bd || y >= bd || z >= bd) return VHX_E_INVALID_ARG;
    const Entry e = tree->tree->entry_of(tree->tree->sample_root_mip((uint8_t)sectant, U3{x, y, z}));
    *kind = e.kind;
    *albedo = e.albedo;
    *data = e.data;
    return VHX_OK;
}
int vhx_scene_build(uint32_t scene, uint32_t size, uint32_t brick_dim, uint64_t seed, int threads, vhx_flat **out) {
    if (!out || !scene_valid(scene)) return VHX_E_INVALID_ARG;
    try {
        return build_scene(scene, size, brick_dim, seed, threads, out);
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_scene_build_lod(uint32_t scene, uint32_t size, uint32_t brick_dim, uint64_t seed, int threads,
                        uint32_t max_depth, vhx_flat **out) {
    if (!out || !scene_valid(scene)) return VHX_E_INVALID_ARG;
    try {
        vhx_flat *full = nullptr;
        int rc = build_scene(scene, size, brick_dim, seed, threads, &full);
        if (rc != VHX_OK) return rc;
        std::unique_ptr<vhx_flat> owned(full);
        std::unique_ptr<BoxTree> t(tree_of_flat(*full));
        if (!t) return VHX_E_STATE;
        owned.reset();
        t->switch_albedo_mip_maps(true);
        *out = flatten_tree(*t, max_depth, true);
        return VHX_OK;
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_scene_build_tree(uint32_t scene, uint32_t size, uint32_t brick_dim, uint64_t seed, int threads,
                         vhx_boxtree **out) {
    if (!out || !scene_valid(scene)) return VHX_E_INVALID_ARG;
    *out = nullptr;
    try {
        vhx_flat *full = nullptr;
        int rc = build_scene(scene, size, brick_dim, seed, threads, &full);
        if (rc != VHX_OK) return rc;
        std::unique_ptr<vhx_flat> owned(full);
        BoxTree *t = tree_of_flat(*full);
        if (!t) return VHX_E_STATE;
        *out = new vhx_boxtree{t};
        return VHX_OK;
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_dense_build_tree_data(const vhx_dense_desc *grid, const uint32_t *data, int threads, vhx_boxtree **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    try {
        vhx_flat *full = nullptr;
        int rc = build_dense(grid, data, threads, &full);
        if (rc != VHX_OK) return rc;
        std::unique_ptr<vhx_flat> owned(full);
        BoxTree *t = tree_of_flat(*full);
        if (!t) return VHX_E_STATE;
        *out = new vhx_boxtree{t};
        return VHX_OK;
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_dense_build_data(const vhx_dense_desc *grid, const uint32_t *data, int simplified, int threads, vhx_flat **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    try {
        if (!simplified) return build_dense(grid, data, threads, out);
        vhx_flat *full = nullptr;
        int rc = build_dense(grid, data, threads, &full);
        if (rc != VHX_OK) return rc;
        std::unique_ptr<vhx_flat> owned(full);
        std::unique_ptr<BoxTree> t(tree_of_flat(*full));
        if (!t) return VHX_E_STATE;
        owned.reset();
        t->simplify(0, true);
        *out = flatten_tree(*t);
        return VHX_OK;
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_dense_build(const vhx_dense_desc *grid, int threads, vhx_flat **out) {
    return vhx_dense_build_data(grid, nullptr, 0, threads, out);
}
int vhx_dense_build_tree(const vhx_dense_desc *grid, int threads, vhx_boxtree **out) {
    return vhx_dense_build_tree_data(grid, nullptr, threads, out);
}
int vhx_dense_build_simplified(const vhx_dense_desc *grid, int threads, vhx_flat **out) {
    return vhx_dense_build_data(grid, nullptr, 1, threads, out);
}
int vhx_flat_desc(const vhx_flat *f, vhx_tree_desc *d) {
    if (!f || !d) return VHX_E_INVALID_ARG;
    std::memset(d, 0, sizeof(*d));
    d->boxtree_size = f->size;
    d->brick_dim = f->brick_dim;
    d->node_count = (uint32_t)f->node_type.size();
    d->brick_count = f->brick_count;
    d->solid_count = (uint32_t)f->solid_values.size();
    d->color_count = (uint32_t)f->color_palette.size();
    d->data_count = (uint32_t)f->data_palette.size();
    d->node_type = f->node_type.data();
    d->node_ocbits = f->node_ocbits.data();
    d->node_children = f->node_children.data();
    d->voxels = f->voxels.get();
    d->solid_values = f->solid_values.data();
    d->color_palette = f->color_palette.data();
    d->data_palette = f->data_palette.data();
    return VHX_OK;
}
int vhx_flat_compact(const vhx_tree_desc *tree, vhx_flat **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    if (!tree) return VHX_E_INVALID_ARG;
    try {
        return compact_image(*tree, out);
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_flat_compact_palette(const vhx_tree_desc *tree, vhx_flat **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    if (!tree) return VHX_E_INVALID_ARG;
    try {
        return palettes_image(*tree, VHX_PALETTE_COLOR, out);
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_flat_compact_palettes(const vhx_tree_desc *tree, uint32_t which, vhx_flat **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    if (!tree || which == 0 || (which & ~(uint32_t)(VHX_PALETTE_COLOR | VHX_PALETTE_DATA))) return VHX_E_INVALID_ARG;
    try {
        return palettes_image(*tree, which, out);
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_flat_list_voxels(const vhx_tree_desc *tree, const vhx_points_out *q) {
    if (!tree || !q || !q->count) return VHX_E_INVALID_ARG;
    return list_image(*tree, *q);
}
}  // extern "C"

// the host BoxTree of the compacted image of `tree` (vhx_flat_simplify, vhx_flat_lod)
static int host_tree_of_image(const vhx_tree_desc &tree, std::unique_ptr<BoxTree> &t) {
    vhx_flat *packed = nullptr;
    int rc = compact_image(tree, &packed);
    if (rc != VHX_OK) return rc;
    std::unique_ptr<vhx_flat> owned(packed);
    // tree_of_flat reads solid_values by the entries' indices
    for (size_t i = 0; i < packed->node_type.size(); ++i) {
        const uint32_t ty = packed->node_type[i];
        const uint32_t entries = ty == VHX_NODE_LEAF ? 64u : ty == VHX_NODE_UNIFORM_LEAF ? 1u : 0u;
        for (uint32_t s = 0; s < entries; ++s) {
            const uint32_t e = packed->node_children[i * 64 + s];
            if (e != VHX_EMPTY && (e & VHX_SOLID_BIT) && (e & ~VHX_SOLID_BIT) >= packed->solid_values.size())
                return VHX_E_TREE_INVALID_STRUCTURE;
        }
    }
    t.reset(tree_of_flat(*packed));
    return t ? VHX_OK : VHX_E_TREE_INVALID_STRUCTURE;
}

extern "C" {

int vhx_flat_simplify(const vhx_tree_desc *tree, vhx_flat **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    if (!tree) return VHX_E_INVALID_ARG;
    try {
        std::unique_ptr<BoxTree> t;
        const int rc = host_tree_of_image(*tree, t);
        if (rc != VHX_OK) return rc;
        t->simplify(0, true);
        *out = flatten_tree(*t);
        return VHX_OK;
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
int vhx_flat_lod(const vhx_tree_desc *tree, uint32_t max_depth, uint32_t method, vhx_flat **out) {
    if (!out) return VHX_E_INVALID_ARG;
    *out = nullptr;
    if (!tree || (method != VHX_MIP_BOX_FILTER && method != VHX_MIP_POINT_FILTER)) return VHX_E_INVALID_ARG;
    try {
        std::unique_ptr<BoxTree> t;
        const int rc = host_tree_of_image(*tree, t);
        if (rc != VHX_OK) return rc;
        // one method and a colour-similarity threshold of 0 on every level (a level is log2(node edge / brick_dim))
        for (size_t level = 0; level <= 32; ++level) {
            t->mip_strategy.methods[level] = MipMethodCfg{method, 0.f};
            t->mip_strategy.color_thresholds[level] = 0.f;
        }
        t->switch_albedo_mip_maps(true);
        if (t->color_palette.size() > 0xFFFFu) return VHX_E_CAPACITY;  // a palette index has 16 bits, 0xFFFF = none
        *out = flatten_tree(*t, max_depth, true);
        return VHX_OK;
    } catch (const std::bad_alloc &) {
        return VHX_E_CAPACITY;
    }
}
void vhx_flat_free(vhx_flat *f) { delete f; }

}  // extern "C"
