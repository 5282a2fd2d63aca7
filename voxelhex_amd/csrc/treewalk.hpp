// What the units that read the device tree share (vhx_tree.hip, vhx_query.hip, vhx_edit.hip): the one predicate for an
// empty cell, wave-uniform loads and the integer sectant of a position.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// pix_points_to_empty (src/boxtree/node.rs:311-333): neither a visible colour nor a data value
__device__ __forceinline__ bool cell_empty(uint32_t v, const uint32_t *color, uint32_t ncolor, const uint32_t *data,
                                           uint32_t ndata) {
    const uint32_t ci = v & 0xFFFFu, di = v >> 16;
    const bool cn = ci == 0xFFFFu || ci >= ncolor || ((color[ci] >> 24) & 0xFFu) == 0;
    const bool dn = di == 0xFFFFu || di >= ndata || data[di] == 0;
    return cn && dn;
}

// A load the whole wave makes at one address: through the constant address space, so that it is a scalar load where the
// compiler can prove the address uniform. Only for memory that no launch in flight writes.
__device__ __forceinline__ uint32_t uload(const uint32_t *p) {
    return *(const __attribute__((address_space(4))) uint32_t *)(uintptr_t)p;
}

// the sectant of (x, y, z) in a node 2^lg voxels wide
__device__ __forceinline__ uint32_t sectant_of(uint32_t x, uint32_t y, uint32_t z, uint32_t lg) {
    const uint32_t sh = lg - 2u;
    return ((x >> sh) & 3u) | (((y >> sh) & 3u) << 2) | (((z >> sh) & 3u) << 4);
}
