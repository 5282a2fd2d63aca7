/*
 * vhx_boxtree.h — C ABI of the host-side BoxTree (libvhx.so, host code only, no GPU needed).
 *
 * The reference keeps the voxel tree in Rust (`BoxTree<T>`); its toolchain is not available to this build, so the
 * host side of the raytracing drop-in is restated in C++ behind this ABI:
 *
 *   vhx_boxtree_new            <- BoxTree::new            (src/boxtree/mod.rs:188-219)
 *   vhx_boxtree_insert         <- BoxTree::insert         (src/boxtree/update/insert.rs:21-30)
 *   vhx_boxtree_insert_at_lod  <- BoxTree::insert_at_lod  (src/boxtree/update/insert.rs:37-47)
 *   vhx_boxtree_update         <- BoxTree::update         (src/boxtree/update/insert.rs:53-62)
 *   vhx_boxtree_clear          <- BoxTree::clear          (src/boxtree/update/clear.rs:16-22)
 *   vhx_boxtree_clear_at_lod   <- BoxTree::clear_at_lod   (src/boxtree/update/clear.rs:23-338)
 *   vhx_boxtree_get            <- BoxTree::get            (src/boxtree/mod.rs:223-233)
 *   vhx_boxtree_simplify       <- BoxTree::simplify(ROOT, recursive) (src/boxtree/update/mod.rs:617-867)
 *   vhx_boxtree_flatten        <- BoxTreeGPUDataHandler::add_node/add_brick with every node resident
 *                                 (src/raytracing/bevy/streaming/cache.rs:226-455, 608-716)
 *   vhx_boxtree_load_vox       <- BoxTree::load_vox_file  (src/convert/magicavoxel.rs:234-374)
 *   vhx_boxtree_switch_mips    <- StrategyUpdater::switch_albedo_mip_maps (src/boxtree/mipmap.rs:588-609)
 *   vhx_boxtree_set_mip_method <- StrategyUpdater::set_method_at (mipmap.rs:414-431, 505-513)
 *   vhx_boxtree_set_mip_color_threshold <- StrategyUpdater::set_color_similarity_thr_at (mipmap.rs:365-379, 482-488)
 *   vhx_boxtree_recalculate_mips <- StrategyUpdater::recalculate_mips (mipmap.rs:536-586)
 *   vhx_boxtree_sample_root_mip <- StrategyUpdater::sample_root_mip (mipmap.rs:635-668, a test helper there)
 *   vhx_boxtree_flatten_lod    <- the streamed view with every node above a depth resident and the rest not: node_mips
 *                                 (src/raytracing/bevy/types.rs:245-247) stand in for the missing children
 *   vhx_scene_build            <- bulk builder producing exactly the flattened tree that inserting a procedural
 *                                 scene voxel by voxel (x, then y, then z loops) would produce
 *   vhx_dense_build            <- the same for a caller's dense voxel grid (vhx_dense_desc, vhx.h)
 *   vhx_dense_build_simplified <- that tree after BoxTree::simplify(ROOT, recursive), as load_vox_file leaves a model
 *   vhx_flat_compact           <- no reference counterpart: an edited image without its orphaned slots, renumbered
 *   vhx_flat_simplify          <- that image after BoxTree::simplify(ROOT, recursive), as insert / clear leave a tree
 *                                 with auto-simplify on
 *   vhx_flat_compact_palette   <- no reference counterpart: an edited image with the colour palette of a fresh build
 *   vhx_flat_compact_palettes  <- the same for the selected halves: the colour palette, the data palette or both
 *   vhx_flat_list_voxels       <- no single counterpart (BoxTree::get iterated over a box): its occupied voxels as a list
 *
 * Tree type parameter: T = u32 (the reference default, BoxTree<T = u32>, src/boxtree/types.rs:219).
 */
#ifndef VHX_BOXTREE_H
#define VHX_BOXTREE_H

#include "vhx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OctreeError (src/boxtree/types.rs:9-21) */
#define VHX_E_TREE_INVALID_SIZE (-10)
#define VHX_E_TREE_INVALID_BRICK_DIMENSION (-11)
#define VHX_E_TREE_INVALID_STRUCTURE (-12)
#define VHX_E_TREE_INVALID_POSITION (-13)
/* .vox import */
#define VHX_E_VOX_FORMAT (-14) /* not a .vox file the importer supports (see vhx_boxtree_load_vox) */
#define VHX_E_VOX_IO (-15)     /* the file could not be read */

/* BoxTreeEntry kinds (src/boxtree/types.rs:25-37) */
#define VHX_ENTRY_EMPTY 0u
#define VHX_ENTRY_VISUAL 1u      /* albedo only  */
#define VHX_ENTRY_INFORMATIVE 2u /* data only    */
#define VHX_ENTRY_COMPLEX 3u     /* albedo+data  */

/* Procedural scenes for vhx_scene_build / vhx_scene_insert */
#define VHX_SCENE_LATTICE_CUBE 1u /* examples/gpu_render.rs:57-82: lattice where any coord < S/4 + cube >= S/2, axis-plane colours */
#define VHX_SCENE_BENCH_REGION 2u /* benches/performance.rs:11-27: [0,100)^3 slab where x|y|z < S/4 or all >= S/2, 0x00ABCDEF */
#define VHX_SCENE_LATTICE 3u      /* src/raytracing/tests.rs:777-789 (context_bleed): lattice only, colour 255*c/S            */
#define VHX_SCENE_CUBE 4u         /* src/raytracing/tests.rs:736-748 (cube_flaps): cube >= S/2, colour 255*c/S                 */
#define VHX_SCENE_BOUNDARY 5u     /* src/raytracing/tests.rs:692-703 (brick_boundary): lattice+cube, colour 255*(c%6)/6         */
#define VHX_SCENE_HEIGHTFIELD 6u  /* seeded value-noise terrain (no reference equivalent; SURVEY.md 8d config 3 secondary)   */

typedef struct vhx_boxtree vhx_boxtree;
typedef struct vhx_flat vhx_flat;

int vhx_boxtree_new(uint32_t size, uint32_t brick_dim, vhx_boxtree **out);
void vhx_boxtree_free(vhx_boxtree *tree);
int vhx_boxtree_set_auto_simplify(vhx_boxtree *tree, int enabled);
/* albedo packed r | g<<8 | b<<16 | a<<24 */
int vhx_boxtree_insert(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t kind, uint32_t albedo,
                       uint32_t data);
int vhx_boxtree_insert_at_lod(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t insert_size,
                              uint32_t kind, uint32_t albedo, uint32_t data);
int vhx_boxtree_update(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t kind, uint32_t albedo,
                       uint32_t data);
/* Removal: the voxel at a position, or every voxel of the cube [position, position + clear_size) that lies in the tree.
 * A position outside the tree returns VHX_E_TREE_INVALID_POSITION; clear_size 0 changes nothing. Emptied bricks and
 * nodes are released (a node's pool key is handed out again by later inserts), occupied bits shrink, and with MIP maps
 * on the MIPs of the nodes on the path follow. Where this differs from the reference is listed in docs/DESIGN_LOG.md. */
int vhx_boxtree_clear(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z);
int vhx_boxtree_clear_at_lod(vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t clear_size);
int vhx_boxtree_get(const vhx_boxtree *tree, uint32_t x, uint32_t y, uint32_t z, uint32_t *kind, uint32_t *albedo,
                    uint32_t *data);
int vhx_boxtree_simplify(vhx_boxtree *tree, int recursive);
/* The deepest node containing a position (BoxTree::get_node_internal from the root, src/boxtree/iterate.rs:293-343):
 * its pool key, content (0 Nothing, 1 Internal, 2 Leaf, 3 UniformLeaf), occupied bits and occlusion bits. */
int vhx_boxtree_node_info(const vhx_boxtree *tree, float x, float y, float z, uint64_t *key, uint32_t *content,
                          uint64_t *occupied_bits, uint32_t *occlusion_bits);
/* size, brick_dim, node count (pool length), color and data palette sizes */
int vhx_boxtree_info(const vhx_boxtree *tree, uint32_t info[5]);
/* Runs the reference insert loop (x outer, z inner) of a procedural scene on `tree` (for cross-checking the bulk
 * builder at small sizes; O(size^3) inserts). */
int vhx_scene_insert(vhx_boxtree *tree, uint32_t scene, uint64_t seed);

/* Flattened trees ------------------------------------------------------------------------------------------- */
/* Nodes are renumbered breadth-first from the root; bricks and solid values are numbered in that node order. */
int vhx_boxtree_flatten(const vhx_boxtree *tree, vhx_flat **out);
int vhx_scene_build(uint32_t scene, uint32_t size, uint32_t brick_dim, uint64_t seed, int threads, vhx_flat **out);
/* MIP maps (src/boxtree/mipmap.rs): off by default (MIPMapStrategy::default, mipmap.rs:341-354: level 1 Posterize(0.05),
 * levels 2-4 BoxFilter, colour-matching thresholds {2: 0.1, 3: 0.05, 4: 0.02}). Once switched on, every insert updates
 * the MIPs of the nodes on its path (insert.rs:494); switching on recalculates all of them. A node's MIP level is
 * log2(node edge / brick_dim). Methods (MIPResamplingMethods, src/boxtree/types.rs:113-149): */
#define VHX_MIP_BOX_FILTER 0u      /* gamma-2 average of the cell's colours                                     */
#define VHX_MIP_POINT_FILTER 1u    /* most frequent colour                                                      */
#define VHX_MIP_POINT_FILTER_BD 2u /* most frequent colour, sampled from the voxels instead of the child MIPs    */
#define VHX_MIP_POSTERIZE 3u       /* average of the largest group of colours within threshold*255              */
#define VHX_MIP_POSTERIZE_BD 4u    /* as POSTERIZE (the reference samples it like POSTERIZE too, mipmap.rs:51-55) */
int vhx_boxtree_switch_mips(vhx_boxtree *tree, int enabled);
int vhx_boxtree_set_mip_method(vhx_boxtree *tree, uint32_t level, uint32_t method, float threshold);
int vhx_boxtree_set_mip_color_threshold(vhx_boxtree *tree, uint32_t level, float threshold);
int vhx_boxtree_recalculate_mips(vhx_boxtree *tree);
/* Process-wide options of the MIP generation (no reference counterpart; results never depend on them): direct = 1 runs
 * the direct restatement (get_internal per sample, full palette scans) instead of the exact shortcuts (tests compare the
 * two); threads caps the leaf-resampling workers (0 = up to 16). */
int vhx_boxtree_set_mip_options(int direct, int threads);
/* The root's MIP (sectant 64) or its child's (sectant < 64) at cell (x, y, z) of the brick, as an entry. */
int vhx_boxtree_sample_root_mip(const vhx_boxtree *tree, uint32_t sectant, uint32_t x, uint32_t y, uint32_t z,
                                uint32_t *kind, uint32_t *albedo, uint32_t *data);
/* Flattened tree with node MIPs: nodes deeper than max_depth (root = 0) are left out (their parents' child entries
 * are VHX_EMPTY, occupancy kept); every node's MIP brick is appended to the bricks / solid values and its descriptor
 * stored in node_mips (VHX_EMPTY where the node has no MIP). vhx_boxtree_flatten does the same with every node
 * included when the tree's MIPs are enabled, and leaves node_mips empty otherwise. */
int vhx_boxtree_flatten_lod(const vhx_boxtree *tree, uint32_t max_depth, vhx_flat **out);
/* vhx_scene_build, then the tree's MIP maps switched on with the default strategy and the LOD image of
 * vhx_boxtree_flatten_lod: the same buffers as vhx_scene_insert + vhx_boxtree_switch_mips(1) + vhx_boxtree_flatten_lod
 * without the voxel-by-voxel insert loop (minutes at 1024^3). */
int vhx_scene_build_lod(uint32_t scene, uint32_t size, uint32_t brick_dim, uint64_t seed, int threads,
                        uint32_t max_depth, vhx_flat **out);
/* The host BoxTree of vhx_scene_build's image without the voxel-by-voxel insert loop (a 1024^3 tree in seconds instead
 * of minutes): nodes (pool key = breadth-first index), bricks, occupancy and palettes as vhx_scene_insert builds them,
 * so vhx_boxtree_flatten gives vhx_scene_build's buffers. Not restored: occlusion bits (they record which siblings
 * existed when a node became full, an insert-history fact; all clear here, so a stream's upload walk may descend into
 * nodes the reference would skip) and MIP maps (off; vhx_boxtree_switch_mips builds them). */
int vhx_scene_build_tree(uint32_t scene, uint32_t size, uint32_t brick_dim, uint64_t seed, int threads,
                         vhx_boxtree **out);
/* The bulk builder for a caller's dense grid (vhx_dense_desc, vhx.h): the flattened tree that inserting every voxel of
 * the grid as a Visual entry (x outer, then y, z inner; voxels of alpha 0 skipped) and flattening would give -- only
 * Parted bricks, no solid values, the colour palette in first-appearance order of that loop, no data palette.
 * Sizes are refused as vhx_boxtree_new refuses them; a null grid or an extent of 0 or above boxtree_size:
 * VHX_E_INVALID_ARG; more than 65,535 distinct colours (the palette index has 16 bits, 0xFFFF = none) or 2^31 bricks or
 * more: VHX_E_CAPACITY. */
int vhx_dense_build(const vhx_dense_desc *grid, int threads, vhx_flat **out);
/* The host BoxTree of that image (as vhx_scene_build_tree: occlusion bits and MIP maps not restored); inserts, clears,
 * MIPs and a stream continue from it. */
int vhx_dense_build_tree(const vhx_dense_desc *grid, int threads, vhx_boxtree **out);
/* The simplified image of a dense grid: vhx_dense_build_tree, vhx_boxtree_simplify(tree, recursive = 1) and
 * vhx_boxtree_flatten in one call (no algorithm of its own). Nodes, occupancy and palettes are those of vhx_dense_build;
 * the leaves hold Solid bricks where a brick is one colour throughout and become UniformLeaf nodes where all their bricks
 * are the same Solid brick or every aligned 4x4x4 block of their voxels is homogeneous. vhx_build_tree_dense_simplified
 * (vhx.h) writes the same image on the GPU. Errors as vhx_dense_build. */
int vhx_dense_build_simplified(const vhx_dense_desc *grid, int threads, vhx_flat **out);
/* The bulk builders for a dense grid that carries user data beside its colours. `data` is a second plane with the
 * extents and indexing of grid->albedo: voxel (x,y,z) at data[((uint64_t)z*gy + y)*gx + x], 0 = no data (is_empty of
 * T = u32). Per voxel, with a the albedo word and d the data word:
 *   alpha byte of a == 0, d == 0   no entry (skipped)
 *   alpha byte of a != 0, d == 0   Visual(a):       value  ci | 0xFFFF0000
 *   alpha byte of a == 0, d != 0   Informative(d):  value  0xFFFF | di << 16  (a never reaches the colour palette)
 *   alpha byte of a != 0, d != 0   Complex(a, d):   value  ci | di << 16
 * ci / di index color_palette / data_palette, 0xFFFF = none. The image is the one vhx_boxtree_insert of every voxel that
 * has an entry, with that kind, in x-outer, y, z-inner order and vhx_boxtree_flatten give: each palette in
 * first-appearance order of that loop, counted per palette on its own; a node or brick exists where any entry lies
 * below it, a data-only one included. simplified = 1: that tree after vhx_boxtree_simplify(tree, recursive = 1), as
 * vhx_dense_build_simplified (a brick is Solid where all its cells hold one value, both halves). data == NULL: the call
 * is vhx_dense_build / vhx_dense_build_simplified, bit for bit. Errors as vhx_dense_build; more than 65,535 distinct
 * data values: VHX_E_CAPACITY. vhx_build_tree_dense_data (vhx.h) writes the plain image on the GPU. */
int vhx_dense_build_data(const vhx_dense_desc *grid, const uint32_t *data, int simplified, int threads, vhx_flat **out);
/* The host BoxTree of that image, as vhx_dense_build_tree; data == NULL: vhx_dense_build_tree. */
int vhx_dense_build_tree_data(const vhx_dense_desc *grid, const uint32_t *data, int threads, vhx_boxtree **out);
int vhx_flat_node_mips(const vhx_flat *flat, const uint32_t **node_mips, uint32_t *count);
/* Fills *desc with pointers into the flat object (valid until vhx_flat_free). */
int vhx_flat_desc(const vhx_flat *flat, vhx_tree_desc *desc);
/* The image `tree` (host arrays, e.g. a downloaded device tree after vhx_write_dense) without its unreachable slots and
 * in the builders' numbering: the CPU counterpart of vhx_compact_tree (vhx.h), bit for bit. A node or Parted brick is
 * reachable when a walk from node 0 finds it through the entries (an Internal node's entries that are not VHX_EMPTY, a
 * Leaf's 64, a UniformLeaf's entry 0; occupied_bits are not consulted, so a LOD-cut view compacts like any tree). Nodes
 * are renumbered breadth-first, level by level in (parent's new index, sectant) order, bricks in (owning node's new
 * index, sectant) order; types, occupancy, cells, solid values and palettes move unchanged, and only child indices and
 * Parted brick indices are rewritten. A freshly built image is returned as it is. Node MIPs are not carried over.
 * VHX_E_INVALID_ARG for null arrays or a count of 0 nodes; VHX_E_TREE_INVALID_STRUCTURE, and no image, for a child
 * index at or past node_count, a Parted index at or past brick_count, a node or Parted brick reached twice, or more
 * than 8 node levels. */
int vhx_flat_compact(const vhx_tree_desc *tree, vhx_flat **out);
/* The simplified image of `tree`: vhx_flat_compact, the host BoxTree of that image, vhx_boxtree_simplify(tree,
 * recursive = 1) and vhx_boxtree_flatten in one call (no algorithm of its own); the CPU counterpart of
 * vhx_simplify_tree (vhx.h), bit for bit. The result is a pure function of the image, with the reference's quirks kept:
 *   points_to_empty(v): colour index v & 0xFFFF and data index v >> 16; the colour is none when the index is 0xFFFF, at
 *     or past color_count, or names a colour of alpha 0; the data is none when the index is 0xFFFF, at or past
 *     data_count, or names the value 0; v points to empty when both are none.
 *   Reachability and numbering as vhx_flat_compact, except that an Internal node whose occupied_bits are 0 becomes
 *     Nothing and its subtree leaves the image (tested top-down, before its children are looked at). Internal nodes
 *     never collapse otherwise (the reference tests the parent's content there, which never holds). occupied_bits
 *     move unchanged.
 *   UniformLeaf: an empty entry 0 stays; Solid v: the node becomes Nothing if v points to empty; a Parted brick whose
 *     cells all equal v: entry 0 becomes VHX_EMPTY if v points to empty, else Solid v; any other brick stays. Entries
 *     1..63 are VHX_EMPTY.
 *   Leaf, per entry: Solid v becomes empty if v points to empty; a Parted brick whose cells all equal v becomes empty
 *     if v points to empty, else Solid v; other entries stay. Then, as a whole: (a) 64 Solid entries of one value: a
 *     UniformLeaf over that Solid brick; (b) else, brick_dim 1: a Leaf of those entries; (c) else read the leaf as a
 *     cube of 4 * brick_dim voxels an edge (an empty entry reads 0xFFFFFFFF, a Solid brick its value, a Parted brick
 *     its cell): if every voxel of every aligned 4x4x4 block equals the block's corner voxel, a UniformLeaf over one
 *     new Parted brick whose cell (x, y, z) is voxel (4x, 4y, 4z); otherwise a Leaf of those entries. A Leaf whose
 *     entries all became empty falls into (c) and becomes a UniformLeaf over a brick of 0xFFFFFFFF cells, so the
 *     function is not idempotent there.
 *   solid_values: the distinct values of the result's Solid entries, each once, in order of first (new node,
 *     sectant); unused old values leave. Both palettes and their counts are untouched; cells keep their words.
 * Errors as vhx_flat_compact; VHX_E_TREE_INVALID_STRUCTURE also for a Solid entry at or past solid_count and where the
 * host tree refuses the image (sizes vhx_boxtree_new refuses, a palette with duplicate or empty entries). */
int vhx_flat_simplify(const vhx_tree_desc *tree, vhx_flat **out);
/* The image `tree` with a canonical colour palette: color_palette becomes the palette the builders (vhx_dense_build)
 * give the voxels the image holds now, and every cell and solid value is translated to it; the CPU counterpart of
 * vhx_compact_palette (vhx.h), bit for bit. Nothing is renumbered or dropped but colours: counts of nodes, bricks and
 * solids, the order of solid_values, node types, occupancy, entries, data halves and data_palette stay.
 *   Reachability: nodes and Parted bricks are reachable as for vhx_flat_compact. A reachable value is every cell of a
 *     reachable Parted brick and the solid_values entry of every Solid entry of a reachable Leaf (its 64 entries) or
 *     UniformLeaf (entry 0).
 *   A value v names a colour when ci = v & 0xFFFF is not 0xFFFF, ci < color_count and the alpha byte of
 *     color_palette[ci] is not 0 (the colour half of points_to_empty, above). A colour is used when a reachable value
 *     names it; palette entries holding the same 32-bit colour are one colour.
 *   Every reachable value sits on an axis-aligned cube: a cell of a Leaf's Parted brick, the whole brick of a Leaf's
 *     Solid entry, a cell of a UniformLeaf's brick, or the whole node where that brick is Solid. A node at level l
 *     (the root is level 0) has the edge boxtree_size / 4^l and a Leaf's brick a quarter of it; a UniformLeaf's brick
 *     spans the node; a cell is a brick_dim-th of its brick. The first index of a cube with min corner (x, y, z) is
 *     (x * boxtree_size + y) * boxtree_size + z -- the position of that voxel in the builders' insert loop (x outer,
 *     then y, z inner), which meets the min corner of a cube of one value before the rest of it. The first index of
 *     a colour is the smallest one among the reachable values that name it.
 *   The new color_palette holds the used colours in increasing first index; color_count is their number.
 *   map[ci] is the new index of the colour of entry ci, and 0xFFFF where the entry is unused or of alpha 0 and for
 *     every ci that names no colour. Every cell of every brick slot [0, brick_count), orphaned ones included (they keep
 *     no colour alive), and every entry of solid_values becomes (v & 0xFFFF0000) | map[v & 0xFFFF]. So vhx_read_dense
 *     and emptiness are unchanged, and a value whose colour half named nothing carries 0xFFFF there afterwards.
 * The image of a dense build, plain or simplified, is returned as it is, and the function is idempotent.
 * Errors as vhx_flat_simplify: VHX_E_INVALID_ARG for null arrays or a count of 0 nodes; VHX_E_TREE_INVALID_STRUCTURE,
 * and no image, for vhx_flat_compact's cases, a reachable Solid entry at or past solid_count, and a reachable Leaf or
 * UniformLeaf so deep that a cell of its bricks would be smaller than a voxel (its cubes would have no corner of their
 * own). Duplicate palette entries are accepted. Node MIPs are not carried over. */
int vhx_flat_compact_palette(const vhx_tree_desc *tree, vhx_flat **out);
/* The image `tree` with canonical palettes for the halves selected by `which`, a mask of VHX_PALETTE_COLOR and
 * VHX_PALETTE_DATA (vhx.h): the CPU counterpart of vhx_compact_palettes (vhx.h), bit for bit. With which ==
 * VHX_PALETTE_COLOR the result is vhx_flat_compact_palette's. The data rule is the colour rule above with the data half
 * of points_to_empty in place of the colour half:
 *   A reachable value v names a data value when di = v >> 16 is not 0xFFFF, di < data_count and data_palette[di] is not
 *     0. Reachability, the cubes on which values sit and the first index of a cube's min corner, (x * boxtree_size +
 *     y) * boxtree_size + z, are those of the colour rule. Entries holding the same 32-bit value are one value.
 *   The new data_palette holds the used values in increasing first index; data_count is their number.
 *   dmap[di] is the new index of the value of entry di, and 0xFFFF where the entry is 0 or unused and for every di that
 *     names nothing.
 *   Every cell of every brick slot [0, brick_count), orphaned ones included, and every entry of solid_values is
 *     rewritten: with both halves selected to map[v & 0xFFFF] | dmap[v >> 16] << 16, with one half selected with only
 *     that half translated. VHX_EMPTY stays VHX_EMPTY, and a value that pointed to empty still does. solid_values is
 *     translated, never deduplicated or reordered. The palette of a half that is not selected stays as it is.
 * The image of a dense build with data (vhx_dense_build_data), plain or simplified, is returned as it is, and the
 * function is idempotent.
 * Errors as vhx_flat_compact_palette, and VHX_E_INVALID_ARG for which == 0 or a bit outside the two. */
int vhx_flat_compact_palettes(const vhx_tree_desc *tree, uint32_t which, vhx_flat **out);
/* vhx_list_voxels (vhx.h, which states the contract) over the host image `tree`, with host arrays: the CPU counterpart
 * of the device call, bit for bit in *count and in every array. It is the plain walk -- depth-first from node 0, sectants
 * ascending, the cells of a brick in flat order, clipped to the box -- with a voxel's two words computed as
 * vhx_read_dense_data computes them (a Leaf's cell that points to empty, by the image's palettes, reads as empty).
 * Refusals as the device call, with VHX_E_INVALID_ARG also for a null tree, null node arrays, a count of 0 nodes and a
 * size that is not brick_dim * 4^k. */
int vhx_flat_list_voxels(const vhx_tree_desc *tree, const vhx_points_out *q);
/* The LOD image of `tree` with node MIPs: vhx_flat_compact, the host BoxTree of that image, `method`
 * (VHX_MIP_BOX_FILTER or VHX_MIP_POINT_FILTER) with a colour-similarity threshold of 0 set on every MIP level,
 * vhx_boxtree_switch_mips(1) and vhx_boxtree_flatten_lod(max_depth) in one call (no algorithm of its own); the CPU
 * counterpart of vhx_build_lod (vhx.h, which states the rules), bit for bit in all seven buffers and in the node MIPs
 * (vhx_flat_node_mips). The MIPs are computed for the whole tree before the cut, so the colours of the nodes that are
 * left out are in color_palette as well. Errors as vhx_flat_simplify (a palette with duplicate or empty entries is
 * refused); VHX_E_INVALID_ARG for any other method; VHX_E_CAPACITY where the palette would pass 65,535 colours. */
int vhx_flat_lod(const vhx_tree_desc *tree, uint32_t max_depth, uint32_t method, vhx_flat **out);
void vhx_flat_free(vhx_flat *flat);

/* MagicaVoxel .vox import — BoxTree::<u32>::load_vox_file(filename, brick_dimension) (src/convert/magicavoxel.rs:
 * 234-374): walks the scene graph at frame 0 (translations "_t", rotations "_r" composed like the reference, which
 * resets to identity where "_r" is absent), sizes the tree with model_size_to_tree_size (magicavoxel.rs:55-60),
 * converts Rz-up to Ly-up and inserts every voxel as BoxTreeEntry::Visual(palette colour), then simplifies the tree
 * recursively when auto-simplify is on (the default). The .vox reader is restated from the file format (the
 * reference's dot_vox 5.1.1 is not vendored): files without an RGBA palette or without a scene graph are rejected
 * with VHX_E_VOX_FORMAT. Voxels landing outside the tree return VHX_E_TREE_INVALID_POSITION (the reference panics). */
int vhx_boxtree_load_vox(const char *path, uint32_t brick_dim, vhx_boxtree **out);
int vhx_boxtree_load_vox_memory(const uint8_t *data, uint64_t size, uint32_t brick_dim, vhx_boxtree **out);
/* helpers of the import, exported for tests: model_size_to_tree_size and parse_rotation_matrix (row-major m[9]) */
uint32_t vhx_vox_tree_size(int32_t sx, int32_t sy, int32_t sz, uint32_t brick_dim);
int vhx_vox_rotation(uint8_t b, int32_t m[9]);

#ifdef __cplusplus
}
#endif
#endif /* VHX_BOXTREE_H */
