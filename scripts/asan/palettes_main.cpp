// Stand-alone host sanitizer check of vhx_flat_compact_palettes (flatten.cpp): a hand-made 64-wide image at brick_dim 4
// with a Leaf of two Parted bricks and a Solid entry, a UniformLeaf over a Solid brick, two orphaned brick slots, an
// unused solid value, and palettes that hold duplicate, transparent / zero and unused entries. It is compacted for the
// three masks and every array of the result is held to values written out here. Built and run by
// scripts/asan_palettes.sh; exits 0 when every check held.
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

constexpr uint32_t C0 = 0xFF000011u, C1 = 0xFF000022u;

// The cells that are not VHX_EMPTY: brick 0 at (0,0,0) and brick 1 at (4,0,0) belong to the Leaf at the origin (cells of
// one voxel), bricks 2 and 3 are orphaned. Cell c of a brick is (c & 3, (c >> 2) & 3, c >> 4).
static Image make_image() {
    Image im;
    im.colors = {C0, C1, C1 /* a second entry of C1 */, 0x00333333u /* transparent */, 0xFF000044u /* unused */};
    im.data = {100u, 0u /* an entry that is 0 */, 200u, 200u /* a second entry of 200 */, 300u /* unused */, 400u};
    im.type = {VHX_NODE_INTERNAL, VHX_NODE_LEAF, VHX_NODE_UNIFORM_LEAF, VHX_NODE_NOTHING /* orphaned */};
    im.occ.assign(im.type.size(), 0);
    im.children.assign(im.type.size() * 64, VHX_EMPTY);
    im.children[0] = 1, im.children[21] = 2;  // the UniformLeaf spans (16,16,16) .. (31,31,31)
    im.children[64 + 0] = 0, im.children[64 + 1] = 1, im.children[64 + 2] = VHX_SOLID_BIT | 0u;  // Solid at (8,0,0)
    im.children[128] = VHX_SOLID_BIT | 1u;
    im.solids = {0x0000FFFFu /* data 100 alone, first index 32768 */, 0xFFFF0000u /* C0 alone */,
                 0x00040004u /* no entry names it: the unused colour and value */};
    im.voxels.assign(4 * 64, VHX_EMPTY);
    im.voxels[0] = 0x00050001u;    // (0,0,0): C1, 400             first index 0
    im.voxels[1] = 0x0003FFFFu;    // (1,0,0): the second 200      first index 4096
    im.voxels[16] = 0x00010000u;   // (0,0,1): C0, the entry 0     first index 1
    im.voxels[4] = 0x00010003u;    // (0,1,0): transparent and 0: points to empty
    im.voxels[64 + 0] = 0x00020002u;   // (4,0,0): the second C1, the first 200   first index 16384
    im.voxels[64 + 63] = 0x00000000u;  // (7,3,3): C0, 100                        first index 28867
    for (uint32_t i = 0; i < 64; ++i) {
        im.voxels[128 + i] = 0x00040004u;  // orphaned: names the unused entries, and keeps them not alive
        im.voxels[192 + i] = 0x00020001u;  // orphaned: live entries, translated
    }
    return im;
}

struct Want {
    uint32_t which;
    std::vector<uint32_t> colors, data, solids;
    uint32_t b0c0, b0c1, b0c16, b0c4, b1c0, b1c63, orphan2, orphan3;
};

static void check(const Image &im, const Want &w) {
    const vhx_tree_desc d = im.desc();
    vhx_flat *f = nullptr;
    CHECK(vhx_flat_compact_palettes(&d, w.which, &f) == VHX_OK && f);
    if (!f) return;
    vhx_tree_desc g{};
    CHECK(vhx_flat_desc(f, &g) == VHX_OK);
    CHECK(g.node_count == d.node_count && g.brick_count == d.brick_count && g.solid_count == d.solid_count);
    CHECK(g.boxtree_size == 64 && g.brick_dim == 4);
    for (uint32_t i = 0; i < d.node_count; ++i) CHECK(g.node_type[i] == im.type[i] && g.node_ocbits[i] == im.occ[i]);
    for (uint32_t i = 0; i < d.node_count * 64; ++i) CHECK(g.node_children[i] == im.children[i]);
    CHECK(g.color_count == w.colors.size() && g.data_count == w.data.size());
    for (uint32_t i = 0; i < g.color_count && i < w.colors.size(); ++i) CHECK(g.color_palette[i] == w.colors[i]);
    for (uint32_t i = 0; i < g.data_count && i < w.data.size(); ++i) CHECK(g.data_palette[i] == w.data[i]);
    for (uint32_t i = 0; i < g.solid_count; ++i) CHECK(g.solid_values[i] == w.solids[i]);
    std::vector<uint32_t> vox(4 * 64, VHX_EMPTY);
    vox[0] = w.b0c0, vox[1] = w.b0c1, vox[16] = w.b0c16, vox[4] = w.b0c4, vox[64] = w.b1c0, vox[64 + 63] = w.b1c63;
    for (uint32_t i = 0; i < 64; ++i) vox[128 + i] = w.orphan2, vox[192 + i] = w.orphan3;
    for (uint32_t i = 0; i < 4 * 64; ++i) CHECK(g.voxels[i] == vox[i]);
    // idempotent
    vhx_flat *again = nullptr;
    CHECK(vhx_flat_compact_palettes(&g, w.which, &again) == VHX_OK && again);
    if (again) {
        vhx_tree_desc h{};
        CHECK(vhx_flat_desc(again, &h) == VHX_OK && h.color_count == g.color_count && h.data_count == g.data_count);
        for (uint32_t i = 0; i < 4 * 64; ++i) CHECK(h.voxels[i] == g.voxels[i]);
        for (uint32_t i = 0; i < g.solid_count; ++i) CHECK(h.solid_values[i] == g.solid_values[i]);
        vhx_flat_free(again);
    }
    if (w.which == VHX_PALETTE_COLOR) {  // the older entry point gives the same image
        vhx_flat *old = nullptr;
        CHECK(vhx_flat_compact_palette(&d, &old) == VHX_OK && old);
        if (old) {
            vhx_tree_desc h{};
            CHECK(vhx_flat_desc(old, &h) == VHX_OK && h.color_count == g.color_count && h.data_count == g.data_count);
            for (uint32_t i = 0; i < 4 * 64; ++i) CHECK(h.voxels[i] == g.voxels[i]);
            for (uint32_t i = 0; i < g.solid_count; ++i) CHECK(h.solid_values[i] == g.solid_values[i]);
            for (uint32_t i = 0; i < g.color_count; ++i) CHECK(h.color_palette[i] == g.color_palette[i]);
            vhx_flat_free(old);
        }
    }
    vhx_flat_free(f);
}

int main() {
    const Image im = make_image();
    // colours: C1 first (index 0), then C0 (index 1); map 0 -> 1, 1 -> 0, 2 -> 0, 3 and 4 -> none
    // data: 400 (0), 200 (4096), 100 (28867); dmap 0 -> 2, 1 -> none, 2 -> 1, 3 -> 1, 4 -> none, 5 -> 0
    const Want both{VHX_PALETTE_COLOR | VHX_PALETTE_DATA, {C1, C0}, {400u, 200u, 100u},
                    {0x0002FFFFu, 0xFFFF0001u, 0xFFFFFFFFu},
                    0x00000000u, 0x0001FFFFu, 0xFFFF0001u, 0xFFFFFFFFu, 0x00010000u, 0x00020001u, 0xFFFFFFFFu, 0x00010000u};
    const Want color{VHX_PALETTE_COLOR, {C1, C0}, im.data,
                     {0x0000FFFFu, 0xFFFF0001u, 0x0004FFFFu},
                     0x00050000u, 0x0003FFFFu, 0x00010001u, 0x0001FFFFu, 0x00020000u, 0x00000001u, 0x0004FFFFu, 0x00020000u};
    const Want data{VHX_PALETTE_DATA, im.colors, {400u, 200u, 100u},
                    {0x0002FFFFu, 0xFFFF0000u, 0xFFFF0004u},
                    0x00000001u, 0x0001FFFFu, 0xFFFF0000u, 0xFFFF0003u, 0x00010002u, 0x00020000u, 0xFFFF0004u, 0x00010001u};
    check(im, both);
    check(im, color);
    check(im, data);

    // refusals return no image
    const vhx_tree_desc d = im.desc();
    for (uint32_t which : {0u, 4u, 7u, 0x80000001u}) {
        vhx_flat *f = (vhx_flat *)(uintptr_t)1;
        CHECK(vhx_flat_compact_palettes(&d, which, &f) == VHX_E_INVALID_ARG && f == nullptr);
    }
    CHECK(vhx_flat_compact_palettes(&d, 3u, nullptr) == VHX_E_INVALID_ARG);
    vhx_flat *f = nullptr;
    CHECK(vhx_flat_compact_palettes(nullptr, 3u, &f) == VHX_E_INVALID_ARG);
    Image bad = make_image();
    bad.children[64 + 2] = VHX_SOLID_BIT | 3u;  // a Solid index at solid_count
    vhx_tree_desc b = bad.desc();
    CHECK(vhx_flat_compact_palettes(&b, 2u, &f) == VHX_E_TREE_INVALID_STRUCTURE && f == nullptr);
    bad = make_image();
    bad.children[64 + 5] = 1;  // brick 1 reached twice
    b = bad.desc();
    CHECK(vhx_flat_compact_palettes(&b, 3u, &f) == VHX_E_TREE_INVALID_STRUCTURE && f == nullptr);
    bad = make_image();
    bad.children[64 + 5] = 4;  // a Parted index at brick_count
    b = bad.desc();
    CHECK(vhx_flat_compact_palettes(&b, 1u, &f) == VHX_E_TREE_INVALID_STRUCTURE && f == nullptr);
    std::printf("vhx_flat_compact_palettes: three masks, %d failed checks\n", failures);
    return failures ? 1 : 0;
}
