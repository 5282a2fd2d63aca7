// Stand-alone host sanitizer check of vhx_flat_lod (flatten.cpp): a hand-made 64-wide image at brick_dim 4 in edit
// order (junk slots between the reachable ones) with a Leaf of Parted, Solid and empty bricks, a UniformLeaf and a
// Nothing node, turned into LOD images for both methods and every cut, and checked against values worked out by hand.
// The result arrays are heap copies of exactly their counts, so that a read past a count is an AddressSanitizer report.
// Built and run by scripts/asan_lod.sh; exits 0 when every check held.
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

static const uint32_t RED = 0xFF0000FAu, BLUE = 0xFFFA0000u, CLEAR = 0x00102030u;

static Image make_image() {
    Image im;
    im.colors = {RED, BLUE, CLEAR};
    im.data = {7u};
    im.solids = {0xFFFF0001u /* blue */, 0x0000FFFFu /* data only */};
    // node 0 the root, 3 a Leaf (sectant 0), 1 a UniformLeaf (sectant 21), 4 a Nothing node (sectant 63), 2 junk
    im.type = {VHX_NODE_INTERNAL, VHX_NODE_UNIFORM_LEAF, VHX_NODE_LEAF, VHX_NODE_LEAF, VHX_NODE_NOTHING};
    im.occ = {(1ull << 0) | (1ull << 21), ~0ull, 5ull, 3ull, 0ull};
    im.children.assign(im.type.size() * 64, VHX_EMPTY);
    im.children[0] = 3, im.children[21] = 1, im.children[63] = 4;
    im.children[64] = VHX_SOLID_BIT | 0u;
    // the Leaf: brick 2 at sectant 0 (Parted), Solid blue at sectant 1, Solid data-only at sectant 2
    im.children[3 * 64 + 0] = 2, im.children[3 * 64 + 1] = VHX_SOLID_BIT | 0u, im.children[3 * 64 + 2] = VHX_SOLID_BIT | 1u;
    im.voxels.assign(3 * 64, 0x12345678u);  // bricks 0 and 1 are junk
    for (uint32_t i = 0; i < 64; ++i) im.voxels[128 + i] = VHX_EMPTY;
    // cell (0,0,0) red, (0,0,1) blue, (1,0,0) red, (1,0,1) blue: red seen first, two each;
    // (2,0,0) data only, (3,0,0) the transparent colour alone (points to empty), (2,1,0) transparent with data
    im.voxels[128 + 0] = 0xFFFF0000u, im.voxels[128 + 16] = 0xFFFF0001u;
    im.voxels[128 + 1] = 0xFFFF0000u, im.voxels[128 + 17] = 0xFFFF0001u;
    im.voxels[128 + 2] = 0x0000FFFFu, im.voxels[128 + 3] = 0xFFFF0002u, im.voxels[128 + 6] = 0x00000002u;
    return im;
}

struct Lod {
    int rc = 0;
    vhx_tree_desc d{};
    std::vector<uint32_t> type, children, voxels, solids, colors, mips;
};

static Lod lod(const vhx_tree_desc &t, uint32_t depth, uint32_t method) {
    Lod l;
    vhx_flat *f = nullptr;
    l.rc = vhx_flat_lod(&t, depth, method, &f);
    if (l.rc != VHX_OK) {
        CHECK(f == nullptr);
        return l;
    }
    CHECK(vhx_flat_desc(f, &l.d) == VHX_OK);
    const uint32_t *m = nullptr;
    uint32_t mc = 0;
    CHECK(vhx_flat_node_mips(f, &m, &mc) == VHX_OK && mc == l.d.node_count);
    l.type.assign(l.d.node_type, l.d.node_type + l.d.node_count);
    l.children.assign(l.d.node_children, l.d.node_children + (size_t)l.d.node_count * 64);
    l.voxels.assign(l.d.voxels, l.d.voxels + (size_t)l.d.brick_count * 64);
    l.solids.assign(l.d.solid_values, l.d.solid_values + l.d.solid_count);
    l.colors.assign(l.d.color_palette, l.d.color_palette + l.d.color_count);
    l.mips.assign(m, m + mc);
    vhx_flat_free(f);
    return l;
}

int main() {
    const Image im = make_image();
    const vhx_tree_desc d = im.desc();
    // PointFilter, every node kept: breadth-first order root, Leaf, UniformLeaf, Nothing
    const Lod p = lod(d, 1, VHX_MIP_POINT_FILTER);
    CHECK(p.rc == VHX_OK);
    if (p.rc == VHX_OK) {
        CHECK(p.type == (std::vector<uint32_t>{VHX_NODE_INTERNAL, VHX_NODE_LEAF, VHX_NODE_UNIFORM_LEAF, VHX_NODE_NOTHING}));
        CHECK(p.d.brick_count == 3 && p.colors == im.colors && p.solids == im.solids);
        // bricks in node order: the root's MIP (it has no brick of its own), the Leaf's Parted brick, the Leaf's MIP
        CHECK(p.mips == (std::vector<uint32_t>{0u, 2u, VHX_EMPTY, VHX_EMPTY}));
        CHECK(p.children[64] == 1u && p.children[64 + 1] == (VHX_SOLID_BIT | 0u) && p.children[64 + 2] == (VHX_SOLID_BIT | 1u));
        CHECK(p.children[128] == (VHX_SOLID_BIT | 0u));
        // the Leaf's MIP: cell 0 over brick 0 -- red and blue twice each, blue first seen last; the transparent colour
        // with data counts once. Cell 1 over the Solid blue brick. Cell 2 over the data-only brick: nothing
        CHECK(p.voxels[128 + 0] == 0xFFFF0001u && p.voxels[128 + 1] == 0xFFFF0001u && p.voxels[128 + 2] == VHX_EMPTY);
        CHECK(p.voxels[64 + 0] == 0xFFFF0000u && p.voxels[64 + 16] == 0xFFFF0001u);  // the Leaf's own brick moved as it is
        // the root's MIP: cell 0 over the Leaf's MIP cells 0..3 of each axis: blue twice; the UniformLeaf gives nothing
        CHECK(p.voxels[0] == 0xFFFF0001u);
        for (uint32_t i = 1; i < 64; ++i) CHECK(p.voxels[i] == VHX_EMPTY);
    }
    // the cut at the root: one node, its entries empty, its occupancy kept, its MIP the only brick
    const Lod c = lod(d, 0, VHX_MIP_POINT_FILTER);
    CHECK(c.rc == VHX_OK && c.d.node_count == 1 && c.d.brick_count == 1 && c.solids.empty());
    if (c.rc == VHX_OK) {
        for (uint32_t s = 0; s < 64; ++s) CHECK(c.children[s] == VHX_EMPTY);
        CHECK(c.mips == (std::vector<uint32_t>{0u}) && c.voxels[0] == 0xFFFF0001u);
    }
    // BoxFilter: cell 0 of the Leaf averages red, red, blue, blue and the transparent colour: a new colour
    const Lod b = lod(d, 7, VHX_MIP_BOX_FILTER);
    CHECK(b.rc == VHX_OK && b.d.node_count == 4 && b.d.brick_count == 3);
    if (b.rc == VHX_OK) {
        CHECK(b.colors.size() > im.colors.size() && b.colors[0] == RED && b.colors[1] == BLUE && b.colors[2] == CLEAR);
        CHECK(b.voxels[128 + 0] == (0xFFFF0000u | 3u));  // the first colour appended: the post-order meets the Leaf first
        CHECK(b.voxels[128 + 1] == 0xFFFF0001u);         // the average of one colour is that colour
        CHECK(b.voxels[0] == (0xFFFF0000u | 4u) && b.colors.size() == 5);  // the root's cell averages the two
        // r: sqrt((250^2 * 2 + 0x30^2) / 5) = 159.5 -> 159; g: sqrt(0x20^2 / 5) = 14.3; b: sqrt((250^2 * 2 + 0x10^2) / 5)
        // = 158.2; a: sqrt(255^2 * 4 / 5) = 228.07
        CHECK(b.colors[3] == (159u | (14u << 8) | (158u << 16) | (228u << 24)));
    }
    // refusals
    vhx_flat *f = nullptr;
    for (uint32_t method : {VHX_MIP_POINT_FILTER_BD, VHX_MIP_POSTERIZE, VHX_MIP_POSTERIZE_BD, 99u})
        CHECK(vhx_flat_lod(&d, 0, method, &f) == VHX_E_INVALID_ARG && f == nullptr);
    CHECK(vhx_flat_lod(nullptr, 0, 0, &f) == VHX_E_INVALID_ARG && vhx_flat_lod(&d, 0, 0, nullptr) == VHX_E_INVALID_ARG);
    Image twice = make_image();
    twice.children[5] = 3;  // the Leaf is reached twice
    CHECK(vhx_flat_lod(&(const vhx_tree_desc &)twice.desc(), 1, 0, &f) == VHX_E_TREE_INVALID_STRUCTURE && f == nullptr);
    Image past = make_image();
    past.children[3 * 64 + 5] = VHX_SOLID_BIT | 9u;  // a Solid entry past solid_count
    CHECK(vhx_flat_lod(&(const vhx_tree_desc &)past.desc(), 1, 0, &f) == VHX_E_TREE_INVALID_STRUCTURE && f == nullptr);
    std::printf("vhx_flat_lod: %d failed checks\n", failures);
    return failures ? 1 : 0;
}
