// Host shim around voxelhex_amd/csrc/skyblock.hpp (tests/test_skyblock.py): the sky mask of one frame, a byte per
// 16x16 block in raster order, computed by the host compiler from the same header the device unit includes.
#include "../../voxelhex_amd/csrc/skyblock.hpp"

extern "C" int vhx_sky_mask(const vhx::SkyCam *cam, uint32_t tree_size, uint8_t *mask) {
    const uint32_t bx = (cam->width + 15u) / 16u, by = (cam->height + 15u) / 16u;
    for (uint32_t y = 0; y < by; ++y)
        for (uint32_t x = 0; x < bx; ++x) {
            const uint32_t x1 = x * 16u + 15u < cam->width ? x * 16u + 15u : cam->width - 1u;
            const uint32_t y1 = y * 16u + 15u < cam->height ? y * 16u + 15u : cam->height - 1u;
            mask[y * bx + x] = vhx::block_is_sky(*cam, tree_size, x * 16u, y * 16u, x1, y1) ? 1 : 0;
        }
    return 0;
}
