// Stand-alone host sanitizer check of vhx_flat_list_voxels (flatten.cpp): a hand-made 64-wide image at brick_dim 4 with a
// Leaf of Parted, Solid and empty bricks, a UniformLeaf over a Parted brick and one over a Solid brick, listed for the
// box shapes of tests/test_list_voxels.py into heap arrays of exactly the capacity, so that a store past the capacity is
// an AddressSanitizer report. Built and run by scripts/asan_list_voxels.sh; exits 0 when every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/vhx_boxtree.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                  \
        }                                                                \
    } while (0)

struct Image {
    std::vector<uint32_t> type, children, voxels, solids, colors, data;
    std::vector<uint64_t> occ;
    vhx_tree_desc desc() const {
        vhx_tree_desc d{};
        d.boxtree_size = 64, d.brick_dim = 4;
        d.node_count = (uint32_t)type.size(), d.brick_count = (uint32_t)voxels.size() / 64u;
        d.solid_count = (uint32_t)solids.size(), d.color_count = (uint32_t)colors.size();
        d.data_count = (uint32_t)data.size();
        d.node_type = type.data(), d.node_ocbits = occ.data(), d.node_children = children.data();
        d.voxels = voxels.data(), d.solid_values = solids.data(), d.color_palette = colors.data();
        d.data_palette = data.data();
        return d;
    }
};

static Image make_image() {
    Image im;
    im.colors = {0xFF102030u, 0x00FFFFFFu /* transparent */, 0x07AABBCCu};
    im.data = {7u, 0u /* an entry that is 0 */, 0x80000000u};
    im.solids = {0xFFFF0000u /* colour 0 */, 0x0001FFFFu /* data only, and that entry is 0: empty */,
                 0x00020001u /* transparent colour, data 0x80000000 */};
    im.type = {VHX_NODE_INTERNAL, VHX_NODE_LEAF, VHX_NODE_UNIFORM_LEAF, VHX_NODE_UNIFORM_LEAF, VHX_NODE_NOTHING};
    im.occ.assign(im.type.size(), 0);
    im.children.assign(im.type.size() * 64, VHX_EMPTY);
    im.children[0] = 1, im.children[21] = 2, im.children[63] = 3, im.children[5] = 4;
    im.children[9] = 77;  // a child that is not in this image: reads as empty
    // bricks 0 and 1 of the Leaf, brick 2 of the first UniformLeaf
    im.voxels.assign(3 * 64, VHX_EMPTY);
    for (uint32_t i = 0; i < 64; ++i) {
        if (i % 3 == 0) im.voxels[i] = 0xFFFF0000u | (i % 2 ? 2u : 0u);    // colours 0 and 2
        if (i % 5 == 0) im.voxels[64 + i] = 0x0000FFFFu | ((i % 3) << 16);  // data only: 7, 0 (empty), 0x80000000
        im.voxels[128 + i] = i % 4 == 0 ? 0xFFFF0001u /* transparent: raw, still empty */ : 0x00020000u;
    }
    im.voxels[64 + 7] = 0x00090009u;  // both indices past their palettes
    im.children[64 + 0] = 0, im.children[64 + 22] = 1, im.children[64 + 63] = VHX_SOLID_BIT | 0u;
    im.children[64 + 1] = VHX_SOLID_BIT | 1u, im.children[64 + 2] = VHX_SOLID_BIT | 2u;
    im.children[64 + 3] = VHX_SOLID_BIT | 9u;  // past solid_count: empty
    im.children[64 + 4] = 40;                  // past brick_count: empty
    im.children[128] = 2;
    im.children[192] = VHX_SOLID_BIT | 2u;
    return im;
}

struct List {
    int rc;
    uint64_t count;
    std::vector<uint32_t> pos, albedo, data;
};

// fields: bit 0 positions, 1 albedo, 2 data
static List list(const vhx_tree_desc &d, const uint32_t box[6], uint64_t capacity, unsigned fields = 7u) {
    List l;
    l.count = ~0ull;
    l.pos.assign(capacity * 3, 0xDEADBEEFu), l.albedo.assign(capacity, 0xDEADBEEFu), l.data.assign(capacity, 0xDEADBEEFu);
    vhx_points_out q{};
    q.ox = box[0], q.oy = box[1], q.oz = box[2], q.gx = box[3], q.gy = box[4], q.gz = box[5];
    q.capacity = capacity;
    q.positions = (fields & 1u) && capacity ? l.pos.data() : nullptr;
    q.albedo = (fields & 2u) && capacity ? l.albedo.data() : nullptr;
    q.data = (fields & 4u) && capacity ? l.data.data() : nullptr;
    q.count = &l.count;
    l.rc = vhx_flat_list_voxels(&d, &q);
    return l;
}

int main() {
    const Image im = make_image();
    const vhx_tree_desc d = im.desc();
    const uint32_t boxes[][6] = {{0, 0, 0, 64, 64, 64}, {0, 0, 0, 1, 1, 1},  {2, 0, 0, 1, 1, 1},    {1, 1, 1, 2, 2, 2},
                                 {3, 5, 1, 61, 33, 63}, {1, 1, 1, 62, 61, 62}, {17, 18, 19, 13, 7, 5}, {47, 47, 47, 3, 3, 3},
                                 {0, 16, 0, 16, 4, 4}};
    uint64_t cube = 0;
    for (const auto &box : boxes) {
        const List full = list(d, box, 0);
        CHECK(full.rc == VHX_OK && full.count != ~0ull);
        if (full.rc != VHX_OK) continue;
        if (box[3] == 64) cube = full.count;
        const uint64_t n = full.count;
        const List all = list(d, box, n);
        CHECK(all.rc == VHX_OK && all.count == n);
        for (uint64_t i = 0; i < n; ++i) {
            CHECK(all.pos[3 * i] - box[0] < box[3] && all.pos[3 * i + 1] - box[1] < box[4] && all.pos[3 * i + 2] - box[2] < box[5]);
            CHECK(all.albedo[i] != 0u || all.data[i] != 0u);
        }
        for (uint64_t cap : {n ? n - 1 : 0, n + 5}) {
            const List part = list(d, box, cap);
            CHECK(part.rc == VHX_OK && part.count == n);
            const uint64_t k = cap < n ? cap : n;
            for (uint64_t i = 0; i < k; ++i)
                CHECK(part.pos[3 * i] == all.pos[3 * i] && part.pos[3 * i + 2] == all.pos[3 * i + 2] &&
                      part.albedo[i] == all.albedo[i] && part.data[i] == all.data[i]);
            for (uint64_t i = k; i < cap; ++i) CHECK(part.albedo[i] == 0xDEADBEEFu && part.pos[3 * i + 1] == 0xDEADBEEFu);
        }
        for (unsigned fields = 0; fields < 7u; ++fields) CHECK(list(d, box, n, fields).count == n);
    }
    CHECK(cube > 64);
    // refusals leave the count alone
    const uint32_t empty[6] = {0, 0, 0, 4, 0, 4}, outside[6] = {61, 0, 0, 4, 4, 4}, wraps[6] = {0, 0xFFFFFFFFu, 0, 1, 2, 1};
    for (const auto *box : {empty, outside, wraps}) {
        const List l = list(d, box, 4);
        CHECK(l.rc == VHX_E_INVALID_ARG && l.count == ~0ull && l.albedo[0] == 0xDEADBEEFu);
    }
    Image stretched = make_image();
    stretched.type[0] = VHX_NODE_UNIFORM_LEAF;
    stretched.children[0] = VHX_SOLID_BIT | 0u;
    const uint32_t whole[6] = {0, 0, 0, 64, 64, 64};
    const List s = list(stretched.desc(), whole, 4);
    CHECK(s.rc == VHX_E_STATE && s.count == ~0ull && s.pos[0] == 0xDEADBEEFu);
    vhx_tree_desc wide = d;
    wide.boxtree_size = 1u << 24;
    const uint32_t all24[6] = {0, 0, 0, 1u << 24, 1u << 24, 1u << 24};
    const List w = list(wide, all24, 4);
    CHECK(w.rc == VHX_E_CAPACITY && w.count == ~0ull);
    CHECK(vhx_flat_list_voxels(&d, nullptr) == VHX_E_INVALID_ARG && vhx_flat_list_voxels(nullptr, nullptr) == VHX_E_INVALID_ARG);
    std::printf("vhx_flat_list_voxels: %llu voxels in the cube, %d failed checks\n", (unsigned long long)cube, failures);
    return failures ? 1 : 0;
}
