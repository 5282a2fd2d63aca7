// libvhx device side, trace unit: every kernel that traces rays, the pass scheduler and the trace entry points of
// include/vhx.h.
//
// Kernels
//   k_trace_primary, k_trace_primary_batch  pass 0 of a primary frame / a batch of frames: per-pixel primary rays
//                    (examples/gpu_render.rs:196-257, benches/performance.rs:29-66) traced with get_by_ray semantics
//                    (src/raytracing/cpu.rs:296-458); replaces the WGSL `update` kernel dispatched by
//                    VhxRenderNode::run (src/raytracing/bevy/pipeline/mod.rs:96-155)
//   k_classify_blocks, k_emit_worklist  a batch's pass-0 worklist: its tree blocks in logical order, then the 16x16
//                    blocks whose every pixel misses the root cube (skyblock.hpp)
//   k_trace_rays     pass 0 of an explicit ray batch (BoxTree::get_by_ray over many rays)
//   k_trace_queue    the queue passes: the rays an earlier pass abandoned at its step budget, and shadow rays
//   k_trace_tail, k_tail_mask  the early tail of a lone frame
//   k_count_flags, k_emit_flags, k_scan_counts, k_scan_sums, k_gather_chunks, k_sort_segments  a pass's abandoned
//                    rays (flags or chunk lists) compacted into the next pass's queue
//   k_put_queue_args, k_chain (VHX_CHAIN builds)
// The tree these kernels read is built by vhx_tree.hip; contexts, ordering and settings live in vhx_ctx.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vhx.h"
#include "trace.hpp"
#define VHX_SKY_FN __host__ __device__
#include "skyblock.hpp"
static_assert(VHX_RAY_GLASS == 1u, "skyblock.hpp spells the glass model's number out (it includes no header)");

using namespace vhx;

#include "ctx.hpp"

// ------------------------------------------------------------------------------------------------ trace kernels
struct CamD {
    uint32_t model, width, height;
    float ox, oy, oz;
    float blx, bly, blz, rx, ry, rz, ux, uy, uz, pw, ph;
    float m[16];
};

struct OutD {
    uint32_t *value, *cell, *voxel, *rgba, *bytes;
    float *impact, *normal, *depth;
    uint32_t *shadowed;  // fused hard shadows (vhx_set_shadow_light)
};

// examples/gpu_render.rs:199, 236-251
#define VHX_MISS_RGBA (128u | (128u << 8) | (128u << 16) | (255u << 24))
__device__ __forceinline__ uint32_t shade(const DevTree &t, const HitOut &h) {
    if (!h.hit) return VHX_MISS_RGBA;
    const uint32_t ci = h.value & 0xFFFFu;
    if (ci == 0xFFFFu || ci >= t.color_count) return 255u << 24;
    const uint32_t c = t.color[ci];
    const F3d L = vnorm(mk(0.0f, -1.0f, 1.0f));
    const float dot = (h.nx * L.x + h.ny * L.y) + h.nz * L.z;
    const float s = 1.0f - (dot / 2.0f + 0.5f);
    const uint32_t r = ras_u8((float)(c & 0xFFu) * s), g = ras_u8((float)((c >> 8) & 0xFFu) * s),
                   b = ras_u8((float)((c >> 16) & 0xFFu) * s);
    return r | (g << 8) | (b << 16) | (255u << 24);
}

__device__ __forceinline__ void store(const DevTree &t, const OutD &o, uint64_t i, F3d org, const HitOut &h) {
    if (o.value) o.value[i] = h.hit ? h.value : VHX_EMPTY;
    if (o.cell) o.cell[i] = h.hit ? h.cell : VHX_EMPTY;
    if (o.voxel) {
        o.voxel[3 * i] = h.hit ? h.vx : VHX_EMPTY;
        o.voxel[3 * i + 1] = h.hit ? h.vy : VHX_EMPTY;
        o.voxel[3 * i + 2] = h.hit ? h.vz : VHX_EMPTY;
    }
    if (o.impact) {
        o.impact[3 * i] = h.hit ? h.ix : 0.0f;
        o.impact[3 * i + 1] = h.hit ? h.iy : 0.0f;
        o.impact[3 * i + 2] = h.hit ? h.iz : 0.0f;
    }
    if (o.normal) {
        o.normal[3 * i] = h.hit ? h.nx : 0.0f;
        o.normal[3 * i + 1] = h.hit ? h.ny : 0.0f;
        o.normal[3 * i + 2] = h.hit ? h.nz : 0.0f;
    }
    if (o.depth) o.depth[i] = h.hit ? vlen(vsub(mk(h.ix, h.iy, h.iz), org)) : __builtin_huge_valf();
    if (o.rgba) o.rgba[i] = shade(t, h);
    if (o.bytes) o.bytes[i] = h.bytes;
}

// The miss record of a whole 16x16 block (bx, by) of a W x H framebuffer frame, written by one wave: what store()
// writes for a miss, to every non-null plane, for the block's pixels inside the frame only. Lane l covers pixels
// 4 (l & 3) .. + 3 of the block's row l >> 2: one 16-byte store per one-word plane and three per three-word plane where
// the four pixels lie inside the frame and the plane's address there is 16-byte aligned (a frame width that is a
// multiple of 4 on an aligned array), else word by word.
template <int WORDS, class T, class T4>
__device__ __forceinline__ void fill_miss(T *plane, uint64_t i, uint32_t npx, T v) {
    if (!plane) return;
    T *a = plane + WORDS * i;
    if (npx == 4u && ((uintptr_t)a & 15u) == 0u) {
        T4 v4;
        v4.x = v4.y = v4.z = v4.w = v;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) ((T4 *)a)[k] = v4;
    } else {
        for (uint32_t k = 0; k < WORDS * npx; ++k) a[k] = v;
    }
}
__device__ __forceinline__ void store_miss_block(const OutD &o, uint32_t bx, uint32_t by, uint32_t W, uint32_t H) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = bx * 16u + (lane & 3u) * 4u, y = by * 16u + (lane >> 2);
    if (x >= W || y >= H) return;
    const uint64_t i = (uint64_t)y * W + x;
    const uint32_t npx = W - x < 4u ? W - x : 4u;
    fill_miss<1, uint32_t, uint4>(o.value, i, npx, VHX_EMPTY);
    fill_miss<1, uint32_t, uint4>(o.cell, i, npx, VHX_EMPTY);
    fill_miss<3, uint32_t, uint4>(o.voxel, i, npx, VHX_EMPTY);
    fill_miss<3, float, float4>(o.impact, i, npx, 0.0f);
    fill_miss<3, float, float4>(o.normal, i, npx, 0.0f);
    fill_miss<1, float, float4>(o.depth, i, npx, __builtin_huge_valf());
    fill_miss<1, uint32_t, uint4>(o.rgba, i, npx, VHX_MISS_RGBA);
}

// benches/performance.rs:54-61 (glass) and examples/gpu_render.rs:203-224 (inverse VP, glam op order)
__device__ __forceinline__ void primary_ray(const CamD &c, uint32_t px, uint32_t py, F3d &o, F3d &d) {
    const uint32_t x = px, y = c.height - 1u - py;
    o = mk(c.ox, c.oy, c.oz);
    if (c.model == VHX_RAY_GLASS) {
        const F3d gp = vadd(vadd(mk(c.blx, c.bly, c.blz), vmul(vmul(mk(c.rx, c.ry, c.rz), (float)x), c.pw)),
                            vmul(vmul(mk(c.ux, c.uy, c.uz), (float)y), c.ph));
        d = vnorm(vsub(gp, o));
    } else {
        const float nx = ((float)x + 0.5f) / (float)c.width * 2.0f - 1.0f;
        const float ny = ((float)y + 0.5f) / (float)c.height * 2.0f - 1.0f;
        float nr[4], fr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nr[k] = ((c.m[k] * nx + c.m[4 + k] * ny) + c.m[8 + k] * -1.0f) + c.m[12 + k] * 1.0f;
            fr[k] = ((c.m[k] * nx + c.m[4 + k] * ny) + c.m[8 + k] * 1.0f) + c.m[12 + k] * 1.0f;
        }
        const F3d np = mk(nr[0] / nr[3], nr[1] / nr[3], nr[2] / nr[3]);
        const F3d fp = mk(fr[0] / fr[3], fr[1] / fr[3], fr[2] / fr[3]);
        const F3d dd = vsub(fp, np);
        const float rcp = 1.0f / __builtin_sqrtf((dd.x * dd.x + dd.y * dd.y) + dd.z * dd.z);
        d = vmul(dd, rcp);
    }
}

// A glass-camera ray that misses the root cube by a clear margin (the sky around the tree: two thirds of the bench
// frame's pass-0 waves hold no ray that enters it) ends as the miss record whatever its exact direction, so the exact
// setup -- normalising the direction (3 divisions, a square root) and the root slab test (6 divisions; cpu.rs:302-313,
// spatial/raytracing/mod.rs:33-62) -- is skipped. The test runs on the unnormalised direction v = gp - o with
// approximate reciprocals: t'_k = (bound - o_k) * rcp(v_k) and the exact t_k = (bound - o_k) / (v_k / |v|) agree up to
// the common factor |v| within a few roundings (6 ulp, 4e-7 relative), so tmax' < -m or tmin' - tmax' > m with
// m = 1e-5 * max(|tmin'|, |tmax'|) implies the exact test's miss (tmax < 0 or tmin > tmax). A zero, tiny or non-finite
// component, or anything closer, takes the exact path.
__device__ __forceinline__ bool glass_clear_miss(const CamD &c, uint32_t px, uint32_t py, float tsize) {
    if (c.model != VHX_RAY_GLASS) return false;
    const uint32_t x = px, y = c.height - 1u - py;
    const F3d o = mk(c.ox, c.oy, c.oz);
    const F3d gp = vadd(vadd(mk(c.blx, c.bly, c.blz), vmul(vmul(mk(c.rx, c.ry, c.rz), (float)x), c.pw)),
                        vmul(vmul(mk(c.ux, c.uy, c.uz), (float)y), c.ph));
    const F3d v = vsub(gp, o);
    const float vk[3] = {v.x, v.y, v.z}, ok[3] = {o.x, o.y, o.z};
    float tmin = -__builtin_huge_valf(), tmax = __builtin_huge_valf();
    bool safe = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        safe = safe && __builtin_fabsf(vk[k]) > 1e-20f;  // false for NaN too
        const float r = __builtin_amdgcn_rcpf(vk[k]);
        const float t1 = (0.0f - ok[k]) * r, t2 = (tsize - ok[k]) * r;
        tmin = __builtin_fmaxf(tmin, __builtin_fminf(t1, t2));
        tmax = __builtin_fminf(tmax, __builtin_fmaxf(t1, t2));
    }
    if (!safe || !__builtin_isfinite(tmin) || !__builtin_isfinite(tmax)) return false;
    const float m = 1e-5f * __builtin_fmaxf(__builtin_fabsf(tmin), __builtin_fabsf(tmax));
    return tmax < -m || tmin - tmax > m;
}

// ------------------------------------------------------------------------------------------- multi-pass scheduling
// Per-ray work is heavy-tailed (bench frame: mean 14 steps, p99 311, max 2160), and a wave64 runs as long as its
// longest lane. Pass 0 traces every ray with a small step budget; the rays that exhaust it are listed per chunk (a
// workgroup's 16x16 pixel block, or a queue pass's chunk) in lane order, a scan over the chunk counts and a gather
// turn the lists into the next pass's queue, and the next pass traces them again from scratch, 64 long rays per
// wave, with a larger budget; the last pass is unbounded (VHX_MAX_ITERS). Keeping the queue in spatial order keeps
// neighbouring rays together in a wave: the bench frame's long rays take 1.17 ms in frame order and 1.48 ms in
// completion (atomic-append) order. Every ray's result comes from one uninterrupted, deterministic traversal, so the
// output is bit-identical to a single pass.
struct PassQ {
    uint32_t budget;   // VHX_MAX_ITERS on the final pass
    uint32_t rpw;      // queue passes: rays per wave (lanes >= rpw idle); 0 = adaptive (pass_rpw)
    uint32_t tw;       // adaptive rays per wave: the pass spreads its rays over about this many waves
    uint32_t resume;   // queue passes: the input rays continue from their saved state (else traced from scratch)
    uint32_t *tmp;     // chunk-local lists of abandoned rays (null on the final pass)
    uint32_t *counts;  // per chunk
    uint8_t *flags;    // primary pass 0: abandoned flag per output index (every entry written, no clearing needed)
    uint4 *state;      // per output index, 4 x uint4: saved traversal state of an abandoned ray (null: re-trace); in the
                       // queue-state mode per slot of this pass's chunk lists instead
    const uint4 *sin;  // queue-state mode: the input rays' states in queue order (k_gather_chunks moved them there)
    uint32_t qmode;    // 1: queue-state mode (states saved by list slot, resumed by queue position), 0: by output index
    uint32_t xcd_group;  // pass 0: XCD-aware block runs (xcd_block), 0 = dispatch order
    uint32_t qxcd;       // queue passes: runs of this many chunks dealt over the 8 XCDs, one counter each (0 = off)
    uint32_t sparse;     // budgeted passes with saved state: abandon a wave's rays once fewer lanes trace (0 = off)
    uint32_t *zero;      // pass 0 with block lists: the queue passes' work counters, zeroed by workgroup 0
    float lx, ly, lz;    // fused hard shadows (the FUSE kernels): the light
    uint32_t sbud;       // fused: a shadow ray's steps in the budgeted pass its primary ray finished (0 = the rest)
    // early tail (vhx_ctx::tail_*): pass 0 skips the pixels set in `skip` (the early tail traces them); the final pass
    // appends the pixels of rays that took >= tail_min steps to tail_out (count at word 0, entries from word 64)
    const uint32_t *skip;
    uint32_t *tail_out;
    uint32_t tail_min, tail_cap;
    uint32_t finter;  // batch pass 0: frames interleaved block by block (vhx_ctx::frame_interleave)
};

// one more pixel of the early-tail list (at most cap; the count keeps growing past it, the entries stop)
__device__ __forceinline__ void tail_record(uint32_t *list, uint32_t cap, uint32_t idx) {
    const uint32_t k = atomicAdd(list, 1u);
    if (k < cap) list[64u + k] = idx;
}

// Rays per wave of a queue pass over n rays: fixed, or (rpw == 0) as many as spread the pass over about `tw` waves.
// Long rays traced 64 per wave pay for their divergence (the bench frame's 256 longest: 1.05 ms at 64 per wave,
// 0.56 ms at one per wave and one wave per workgroup); short queues are better spread thin.
__device__ __forceinline__ uint32_t pass_rpw(uint32_t rpw, uint32_t tw, uint32_t n) {
    if (rpw) return rpw;
    const uint32_t k = (n + tw - 1) / tw;
    return k < 1u ? 1u : (k > 64u ? 64u : k);
}

// Block-level ordered append (all 256 threads of the workgroup call it): the workgroup's rays with push set are
// listed at tmp[pos * 256 ...] in thread order, their number at counts[pos] (pos: the workgroup's chunk position).
__device__ __forceinline__ void block_append(bool push, uint32_t idx, uint32_t *tmp, uint32_t *counts,
                                             uint32_t pos) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t m = __ballot(push);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += s_cnt[w];
    if (push) tmp[(uint64_t)pos * 256u + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = idx;
    if (threadIdx.x == 0) counts[pos] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// Exclusive scan of the chunk counts in one workgroup of SCAN_THREADS threads; nchunks = ceil(*n_in / per_chunk) when
// n_in is given (a queue pass: its input length is only known on the device), else nchunks_host. Writes *total.
// Each wave scans 1024 consecutive counts per segment as 16 coalesced rows of 64 (a wave-wide scan per row), the
// waves' totals are combined through LDS. Four waves, not sixteen: with other frames in flight the GPU is full, and a
// 1024-thread workgroup waited up to 0.25 ms for a CU with room for it (kernel trace of three frames in flight).
#define SCAN_THREADS 256u
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(v, d);
        if (lane >= d) v += x;
    }
    return v;
}
#define SCAN_SEG (SCAN_THREADS * 16u)  // counts per segment
__device__ __forceinline__ uint32_t scan_nchunks(uint32_t nchunks_host, const uint32_t *n_in, uint32_t per_chunk,
                                                 uint32_t tw) {
    if (!n_in) return nchunks_host;
    const uint32_t pc = pass_rpw(per_chunk, tw, *n_in);
    return (*n_in + pc - 1) / pc;
}
// seg_base == null: one workgroup walks every segment and writes *total. seg_base != null (a large scan, launch_scan):
// workgroup b scans segment b only, starting from seg_base[b] (the exclusive scan of the segments' sums).
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_counts(const uint32_t *__restrict__ counts,
                                                              uint32_t nchunks_host, const uint32_t *n_in,
                                                              uint32_t per_chunk, uint32_t tw,
                                                              uint32_t *__restrict__ offsets, uint32_t *total,
                                                              const uint32_t *__restrict__ seg_base = nullptr) {
    constexpr uint32_t NW = SCAN_THREADS / 64u;
    __shared__ uint32_t s_wave[NW];
    __shared__ uint32_t s_carry;
    const uint32_t nchunks = scan_nchunks(nchunks_host, n_in, per_chunk, tw);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    constexpr uint32_t K = 16;  // rows of 64 per wave per segment; loads issued together
    uint32_t seg0 = 0, seg_end = nchunks;
    if (seg_base) {
        seg0 = blockIdx.x * SCAN_SEG;
        if (seg0 >= nchunks) return;  // the whole workgroup
        seg_end = seg0 + 1u;
    }
    if (t == 0) s_carry = seg_base ? seg_base[blockIdx.x] : 0u;
    __syncthreads();
    for (uint32_t seg = seg0; seg < seg_end; seg += SCAN_THREADS * K) {
        const uint32_t b = seg + wave * (64u * K) + lane;
        uint32_t v[K];
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) v[k] = b + 64u * k < nchunks ? counts[b + 64u * k] : 0u;
        uint32_t run = 0;  // the wave's sum of the rows before row k
#pragma unroll
        for (uint32_t k = 0; k < K; ++k) {
            const uint32_t inc = wave_incl_scan(v[k], lane);
            const uint32_t row = __shfl(inc, 63);
            v[k] = run + inc - v[k];  // exclusive within the wave's 1024 counts
            run += row;
        }
        if (lane == 0) s_wave[wave] = run;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
#pragma unroll
        for (uint32_t k = 0; k < K; ++k)
            if (b + 64u * k < nchunks) offsets[b + 64u * k] = before + v[k];
        __syncthreads();
        if (t == 0) {
            uint32_t sum = s_carry;
            for (uint32_t w = 0; w < NW; ++w) sum += s_wave[w];
            s_carry = sum;
        }
        __syncthreads();
    }
    if (t == 0 && !seg_base) *total = s_carry;
}
// sums[b] = the sum of segment b's counts (0 past the end)
__global__ void __launch_bounds__(SCAN_THREADS) k_scan_sums(const uint32_t *__restrict__ counts, uint32_t nchunks_host,
                                                            const uint32_t *n_in, uint32_t per_chunk, uint32_t tw,
                                                            uint32_t *__restrict__ sums) {
    __shared__ uint32_t s_wave[SCAN_THREADS / 64u];
    const uint32_t nchunks = scan_nchunks(nchunks_host, n_in, per_chunk, tw);
    const uint32_t t = threadIdx.x, base = blockIdx.x * SCAN_SEG;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint32_t i = base + k * SCAN_THREADS + t;
        v += base < nchunks && i < nchunks ? counts[i] : 0u;
    }
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if ((t & 63u) == 0) s_wave[t >> 6] = v;
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < SCAN_THREADS / 64u; ++w) sum += s_wave[w];
        sums[blockIdx.x] = sum;
    }
}

// Flag compaction in output-index order, 1024 entries per workgroup, 4 per thread. The flag of entry i is flags[i]
// (primary pass 0: the ray was abandoned) or, with HITS, value[i] != VHX_EMPTY (the hit pixels a shadow pass starts
// from).
template <bool HITS>
__device__ __forceinline__ uint32_t flag_bits(const void *src, uint64_t i, uint64_t n) {
    uint32_t bits = 0;  // bit k: flag of entry i + k
    if (i + 3 < n) {
        if (HITS) {
            const uint32_t *v = (const uint32_t *)src + i;  // the caller's array: no alignment beyond 4 B assumed
            bits = (v[0] != VHX_EMPTY ? 1u : 0u) | (v[1] != VHX_EMPTY ? 2u : 0u) | (v[2] != VHX_EMPTY ? 4u : 0u) |
                   (v[3] != VHX_EMPTY ? 8u : 0u);
        } else {
            const uint32_t w = *(const uint32_t *)((const uint8_t *)src + i);
            bits = (w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u);
        }
    } else {
        for (uint64_t k = i; k < n && k < i + 4; ++k) {
            const bool f = HITS ? ((const uint32_t *)src)[k] != VHX_EMPTY : (((const uint8_t *)src)[k] & 1u) != 0;
            if (f) bits |= 1u << (k - i);
        }
    }
    return bits;
}

// qctl: [0..7] queue lengths written after pass p (7: shadow hit list), [16 + QCTL_PASS_WORDS p ..] pass p's work
// counters: the single counter, then the 8 XCD counters, each on a 256-byte line of its own (with the XCD counters in
// one line, the drain of a budgeted pass over many short chunks, every wave probing every exhausted counter, took 2.5 -
// 3.6 times as long as with one counter: DESIGN.md §3)
#define QCTL_PASS_WORDS (9u * 64u)
#define QCTL_WORDS (16u + QCTL_PASS_WORDS * (VHX_MAX_BUDGETS + 1u))
// Order of the pass-0 queue of a primary frame (vhx_ctx::qorder): W = 0 keeps output-index order (row-major in the
// framebuffer layout); W > 0 lists the rays tile by tile -- TS x TS pixel tiles (TS = 1 << tsl >= 8), the tiles
// row-major over the frame (tx per row) or, with mdim > 0, in Morton order over a 2^mdim x 2^mdim grid (tiles outside
// the frame hold no rays), and inside a tile either its 8x8 sub-tiles row-major with their pixels row-major (a pass-0
// wave's footprint), or (zin 1) every pixel in Morton order, or (zin 2) the tile's rows. 2-D neighbourhoods instead
// of frame rows: a queue wave's 64 rays are neighbours in both directions. Only the order of the queue changes, never
// a result.
struct FlagOrder {
    uint32_t W, H, tx, ty, tsl, mdim, zin;
    // a batch of frames (vhx_trace_primary_batch): positions [f * fpos, (f + 1) * fpos) are frame f's, in the order
    // above, and its pixels are output indices [f * fpix, (f + 1) * fpix); fpos = 0: one frame
    uint64_t fpos, fpix;
    // a shadow batch (vhx_trace_shadows_batch): frame f's hit values are the array at fvals[f] (entry i of the batch
    // is fvals[i / fpix][i % fpix]), not one array
    const uint64_t *fvals;
};
__device__ __forceinline__ bool frame_hit(const FlagOrder &o, uint64_t i) {
    const uint64_t f = i / o.fpix;
    return ((const uint32_t *)o.fvals[f])[i - f * o.fpix] != VHX_EMPTY;
}
__device__ __forceinline__ uint32_t compact_bits(uint32_t v) {  // even bits of v -> low half
    v &= 0x55555555u;
    v = (v | (v >> 1)) & 0x33333333u;
    v = (v | (v >> 2)) & 0x0F0F0F0Fu;
    v = (v | (v >> 4)) & 0x00FF00FFu;
    return (v | (v >> 8)) & 0x0000FFFFu;
}
// pixel of position k; false if it lies outside the frame
__device__ __forceinline__ bool order_pixel(const FlagOrder &o, uint64_t k, uint32_t &px, uint32_t &py) {
    const uint32_t t = (uint32_t)(k >> (2u * o.tsl)), r = (uint32_t)k & ((1u << (2u * o.tsl)) - 1u);
    uint32_t gx, gy;
    if (o.mdim) {
        gx = compact_bits(t);
        gy = compact_bits(t >> 1);
    } else {
        gx = t % o.tx;
        gy = t / o.tx;
    }
    uint32_t ix, iy;
    if (o.zin == 2u) {  // rows of the tile
        ix = r & ((1u << o.tsl) - 1u);
        iy = r >> o.tsl;
    } else if (o.zin) {
        ix = compact_bits(r);
        iy = compact_bits(r >> 1);
    } else {
        const uint32_t spr = 1u << (o.tsl - 3u), sub = r >> 6, u = r & 63u;
        ix = (sub % spr) * 8u + (u & 7u);
        iy = (sub / spr) * 8u + (u >> 3);
    }
    px = (gx << o.tsl) + ix;
    py = (gy << o.tsl) + iy;
    return gx < o.tx && gy < o.ty && px < o.W && py < o.H;
}
// output index of position k; false if it names no pixel
__device__ __forceinline__ bool order_index(const FlagOrder &o, uint64_t k, uint64_t &i) {
    uint64_t base = 0;
    if (o.fpos) {
        const uint64_t f = k / o.fpos;
        k -= f * o.fpos;
        base = f * o.fpix;
    }
    uint32_t px, py;
    if (!order_pixel(o, k, px, py)) return false;
    i = base + (uint64_t)py * o.W + px;
    return true;
}
// flags of positions k..k+3 (bit j: position k + j): a pass-0 flag byte, or with HITS a hit value != VHX_EMPTY
template <bool HITS>
__device__ __forceinline__ uint32_t order_bits(const void *src, const FlagOrder &o, uint64_t k) {
    uint32_t bits = 0;
    for (uint32_t j = 0; j < 4u; ++j) {
        uint64_t i;
        if (!order_index(o, k + j, i)) continue;
        // a pass-0 flag byte: 1 = abandoned
        const bool hit = HITS && o.fvals ? frame_hit(o, i) : ((const uint32_t *)src)[i] != VHX_EMPTY;
        if (HITS ? hit : (((const uint8_t *)src)[i] & 1u) != 0) bits |= 1u << j;
    }
    return bits;
}

// hit flags of entries i..i+3 of a shadow batch in output-index order (FlagOrder::fvals)
__device__ __forceinline__ uint32_t frame_bits(const FlagOrder &o, uint64_t i, uint64_t n) {
    uint32_t bits = 0;
    for (uint64_t k = i; k < n && k < i + 4; ++k)
        if (frame_hit(o, k)) bits |= 1u << (k - i);
    return bits;
}

// k_count_flags: the number of set flags per 1024 positions. zero: the queue passes' work counters (qctl[16..79]),
// zeroed here instead of by a separate memset launch; clear (optional, nclear entries): an output array zeroed
// alongside (the shadow flags of a shadow frame)
template <bool HITS>
__global__ void __launch_bounds__(256) k_count_flags(const void *__restrict__ src, uint64_t n,
                                                     uint32_t *__restrict__ counts, uint32_t *zero,
                                                     uint32_t *__restrict__ clear = nullptr, FlagOrder ord = {},
                                                     uint64_t nclear = 0) {
    __shared__ uint32_t s_cnt[4];
    if (blockIdx.x == 0)
        for (uint32_t w = threadIdx.x; w < QCTL_WORDS - 16u; w += blockDim.x) zero[w] = 0u;
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (clear)
        for (uint64_t k = i; k < nclear && k < i + 4u; ++k) clear[k] = 0u;
    uint32_t c = __popc(ord.W ? (i < n ? order_bits<HITS>(src, ord, i) : 0u)
                              : (HITS && ord.fvals ? frame_bits(ord, i, n) : flag_bits<HITS>(src, i, n)));
    for (uint32_t d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

template <bool HITS>
__global__ void __launch_bounds__(256) k_emit_flags(const void *__restrict__ src, uint64_t n,
                                                    const uint32_t *__restrict__ offsets, uint32_t *__restrict__ out,
                                                    FlagOrder ord = {}) {
    __shared__ uint32_t s_wave[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    const uint32_t bits = ord.W ? (i < n ? order_bits<HITS>(src, ord, i) : 0u)
                                : (HITS && ord.fvals ? frame_bits(ord, i, n) : flag_bits<HITS>(src, i, n));
    const uint32_t c = __popc(bits);
    uint32_t inc = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(inc, d);
        if (lane >= d) inc += x;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t o = offsets[blockIdx.x] + inc - c;
    for (uint32_t w = 0; w < wave; ++w) o += s_wave[w];
    for (uint32_t k = 0; k < 4; ++k)
        if (bits & (1u << k)) {
            uint64_t ix = i + k;
            if (ord.W) order_index(ord, i + k, ix);
            out[o++] = (uint32_t)ix;
        }
}

// The output entries a primary trace owns (vhx_trace_primary's geometry: T x T tiles, tiles_x per row, the tiles
// start, start + stride, ... of a W x H frame). Tile layout (tiles = 1): entry i is pixel i % (T * T) of the set's
// tile i / (T * T), owned where that pixel lies inside the frame (the rest is tile padding). Framebuffer layout: entry
// i is pixel (i % W, i / W), owned where its tile is one of the set's (the rest belongs to other ranks' calls).
struct OwnGeom {
    uint32_t W, H, T, tiles_x, start, stride, tiles;
};
__device__ __forceinline__ bool owned_entry(const OwnGeom &g, uint64_t i) {
    if (g.tiles) {
        const uint64_t tt = (uint64_t)g.T * g.T, j = i / tt;
        const uint32_t l = (uint32_t)(i - j * tt), tile = g.start + (uint32_t)j * g.stride;
        return (tile % g.tiles_x) * g.T + l % g.T < g.W && (tile / g.tiles_x) * g.T + l / g.T < g.H;
    }
    const uint32_t py = (uint32_t)(i / g.W), px = (uint32_t)(i - (uint64_t)py * g.W);
    const uint32_t tile = (py / g.T) * g.tiles_x + px / g.T;
    return tile >= g.start && (tile - g.start) % g.stride == 0u;
}
// hit flags of the owned entries among i..i+3 (output-index order), and the owned entries of `clear` zeroed
__device__ __forceinline__ uint32_t owned_hit_bits(const uint32_t *value, const OwnGeom &g, uint64_t i, uint64_t n,
                                                   uint32_t *clear = nullptr) {
    uint32_t bits = 0;
    for (uint64_t k = i; k < n && k < i + 4u; ++k) {
        if (!owned_entry(g, k)) continue;
        if (clear) clear[k] = 0u;
        if (value[k] != VHX_EMPTY) bits |= 1u << (k - i);
    }
    return bits;
}
// k_count_flags<true> / k_emit_flags<true> over the entries a primary trace owns, for the shadow rays that follow it
// inside vhx_trace_primary and the batches (a light set, shadows not fused): entries outside `g` are neither read,
// cleared nor listed. Output-index order.
__global__ void __launch_bounds__(256) k_count_owned_hits(const uint32_t *__restrict__ value, uint64_t n,
                                                          uint32_t *__restrict__ counts, uint32_t *zero,
                                                          uint32_t *__restrict__ clear, OwnGeom g) {
    __shared__ uint32_t s_cnt[4];
    if (blockIdx.x == 0)
        for (uint32_t w = threadIdx.x; w < QCTL_WORDS - 16u; w += blockDim.x) zero[w] = 0u;
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    uint32_t c = __popc(owned_hit_bits(value, g, i, n, clear));
    for (uint32_t d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}
__global__ void __launch_bounds__(256) k_emit_owned_hits(const uint32_t *__restrict__ value, uint64_t n,
                                                         const uint32_t *__restrict__ offsets,
                                                         uint32_t *__restrict__ out, OwnGeom g) {
    __shared__ uint32_t s_wave[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
    const uint32_t bits = owned_hit_bits(value, g, i, n);
    const uint32_t c = __popc(bits);
    uint32_t inc = c;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(inc, d);
        if (lane >= d) inc += x;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t o = offsets[blockIdx.x] + inc - c;
    for (uint32_t w = 0; w < wave; ++w) o += s_wave[w];
    for (uint32_t k = 0; k < 4; ++k)
        if (bits & (1u << k)) out[o++] = (uint32_t)(i + k);
}

// One wave per chunk: copies the chunk's list to the queue at its offset; in the queue-state mode (st_q) the listed
// rays' saved states too, from their list slots to their queue positions (64 B each, coalesced both ways), so that the
// next pass reads a ray's state at its queue position, in the same load round as its output index.
__global__ void __launch_bounds__(256) k_gather_chunks(const uint32_t *__restrict__ tmp, uint32_t stride,
                                                       const uint32_t *__restrict__ counts,
                                                       const uint32_t *__restrict__ offsets, uint32_t nchunks_host,
                                                       const uint32_t *n_in, uint32_t per_chunk, uint32_t tw,
                                                       uint32_t *__restrict__ out,
                                                       const uint4 *__restrict__ st_slot = nullptr,
                                                       uint4 *__restrict__ st_q = nullptr) {
    const uint32_t pc = n_in ? pass_rpw(per_chunk, tw, *n_in) : per_chunk;
    const uint32_t nchunks = n_in ? (*n_in + pc - 1) / pc : nchunks_host;
    if (n_in) stride = pc;  // a queue pass lists its chunk c at tmp[c * rays per wave]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * 4u;
    for (uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6); c < nchunks; c += waves) {
        const uint32_t n = counts[c], o = offsets[c];
        for (uint32_t k = lane; k < n; k += 64u) out[o + k] = tmp[(uint64_t)c * stride + k];
        if (st_q)
            for (uint32_t k = lane; k < n; k += 64u) {
                const uint4 *src = st_slot + 4ull * ((uint64_t)c * stride + k);
                uint4 *dst = st_q + 4ull * ((uint64_t)o + k);
                const uint4 a = src[0], b = src[1], e = src[2], f = src[3];
                dst[0] = a;
                dst[1] = b;
                dst[2] = e;
                dst[3] = f;
            }
    }
}

// Segment node sort of a queue pass's input (docs/DESIGN_LOG.md §15.3): every segment of `seg` consecutive entries (a power of two
// <= VHX_QSORT_MAX) is reordered by the node each ray's saved state stands at (the NodeStack top, state word 12), ties
// in queue order, so that a wave's 64 rays start their first node iteration together and at the same node loads, while
// the segments keep the queue's 2-D order. Bitonic sort of {node, position} keys in LDS; the queue length is read on the
// device, and the workgroups stride over its segments. Only the order of the queue changes, never a result.
// A fused trace (vhx_set_shadow_light) tags the entry of a leftover shadow ray with VHX_QSHADOW (bit 31; a trace of
// 2^31 rays or more runs a single pass and queues nothing): the state index is the entry without the tag, and the
// entry keeps its tag through the sort.
#define VHX_QSHADOW 0x80000000u
#define QSORT_THREADS 256u
__global__ void __launch_bounds__(QSORT_THREADS) k_sort_segments(uint32_t *__restrict__ q, const uint32_t *n_ptr,
                                                                 const uint32_t *__restrict__ state, uint32_t seg) {
    __shared__ unsigned long long key[VHX_QSORT_MAX];
    __shared__ uint32_t val[VHX_QSORT_MAX];
    const uint32_t n = *n_ptr, t = threadIdx.x;
    for (uint64_t base = (uint64_t)blockIdx.x * seg; base < n; base += (uint64_t)gridDim.x * seg) {
        const uint32_t cnt = (uint32_t)min<uint64_t>(seg, n - base);
        for (uint32_t i = t; i < seg; i += QSORT_THREADS) {
            uint32_t v = 0;
            unsigned long long k = ~0ull;  // past the queue's end: sorts last, never written back
            if (i < cnt) {
                v = q[base + i];
                k = ((unsigned long long)state[16ull * (v & ~VHX_QSHADOW) + 12u] << 32) | i;
            }
            key[i] = k;
            val[i] = v;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= seg; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t i = t; i < seg; i += QSORT_THREADS) {
                    const uint32_t l = i ^ j;
                    if (l > i) {
                        const unsigned long long a = key[i], b = key[l];
                        if ((a > b) == ((i & k) == 0u)) {
                            key[i] = b;
                            key[l] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (uint32_t i = t; i < cnt; i += QSORT_THREADS) q[base + i] = val[(uint32_t)key[i]];
        __syncthreads();
    }
}

// One frame of a shadow batch on the device (vhx_shadow_frame)
struct ShD {
    const uint32_t *value;
    const float *impact, *normal;
    uint32_t *shadowed, *rgba;
};

// Where a queued output index comes from: a primary-ray frame (framebuffer or tile layout) or an explicit ray batch.
struct RaySrc {
    uint32_t kind;  // 0 framebuffer, 1 tiles, 2 explicit rays, 3 shadow rays from hit records, 4 a batch of frames,
                    // 5 a batch of shadow frames
    uint32_t T, tiles_x, tile_start, tile_stride;
    const float *rays;
    const float *impact, *normal;  // kind 3
    float lx, ly, lz;               // kind 3: light position
    // kind 4 (vhx_trace_primary_batch): frame f = idx / npix of the batch has camera cams[f] and outputs outs[f]
    // (framebuffer layout, index idx - f * npix); device arrays of the batch
    const CamD *cams;
    const OutD *outs;
    uint32_t npix;
    const ShD *shs;  // kind 5: frame f = idx / npix is shs[f], entry idx - f * npix
    // kind 4 with T > 0 (vhx_trace_tiles_batch): frame f is the tile set starts[f], starts[f] + tile_stride, ... of
    // T x T tiles (tiles_x per row) in the tile layout; npix = the per-frame index stride (the largest set's entries)
    const uint32_t *starts;
};

// Hard-shadow ray of hit record idx (BASELINE config 5; semantics in docs/DESIGN_LOG.md §9): from impact + normal * 1e-3
// toward the light, direction normalised like V3c::normalized (src/spatial/math/vector.rs).
__device__ __forceinline__ void shadow_ray(const RaySrc &src, uint32_t idx, F3d &o, F3d &d) {
    const float *ip, *np;
    if (src.kind == 5u) {  // a shadow batch: frame f's records
        const uint32_t f = idx / src.npix, local = idx - f * src.npix;
        ip = src.shs[f].impact + 3ull * local;
        np = src.shs[f].normal + 3ull * local;
    } else {
        ip = src.impact + 3ull * idx;
        np = src.normal + 3ull * idx;
    }
    o = mk(ip[0] + np[0] * 1e-3f, ip[1] + np[1] * 1e-3f, ip[2] + np[2] * 1e-3f);
    d = vnorm(mk(src.lx - o.x, src.ly - o.y, src.lz - o.z));
}

__device__ __forceinline__ void ray_of(const CamD &cam, const RaySrc &src, uint32_t idx, F3d &o, F3d &d) {
    if (src.kind == 3u || src.kind == 5u) {
        shadow_ray(src, idx, o, d);
        return;
    }
    if (src.kind == 2u) {
        o = mk(src.rays[6ull * idx], src.rays[6ull * idx + 1], src.rays[6ull * idx + 2]);
        d = mk(src.rays[6ull * idx + 3], src.rays[6ull * idx + 4], src.rays[6ull * idx + 5]);
        return;
    }
    if (src.kind == 4u) {  // a batch: the frame's camera, read where the ray is set up
        const uint32_t f = idx / src.npix, local = idx - f * src.npix;
        const CamD *cf = src.cams + f;
        if (src.T) {  // a batch of tile sets: entry local of frame f's set in the tile layout
            const uint32_t tt = src.T * src.T, j = local / tt, l = local - j * tt;
            const uint32_t tile = src.starts[f] + j * src.tile_stride;
            primary_ray(*cf, (tile % src.tiles_x) * src.T + l % src.T, (tile / src.tiles_x) * src.T + l / src.T, o, d);
            return;
        }
        const uint32_t W = cf->width, py = local / W;
        primary_ray(*cf, local - py * W, py, o, d);
        return;
    }
    uint32_t px, py;
    if (src.kind == 0u) {
        py = idx / cam.width;
        px = idx - py * cam.width;
    } else {
        const uint32_t tt = src.T * src.T;
        const uint32_t j = idx / tt, local = idx - j * tt;
        const uint32_t tile = src.tile_start + j * src.tile_stride;
        px = (tile % src.tiles_x) * src.T + local % src.T;
        py = (tile / src.tiles_x) * src.T + local / src.T;
    }
    primary_ray(cam, px, py, o, d);
}

// XCD-aware block order: the dispatcher deals workgroups round-robin over the 8 XCDs (blockIdx % 8 share one XCD and
// its L2; MI355X_MICROARCH.md, workgroup dispatch), so with G > 0 each XCD's blocks are taken in runs of G
// consecutive frame blocks (neighbouring pixels walk the same nodes and bricks). A bijection on [0, n) for any n (the
// last n mod 8G blocks keep their order); only the speed depends on the placement. G = 0: dispatch order.
__device__ __forceinline__ uint32_t xcd_block(uint32_t bid, uint32_t n, uint32_t G) {
    if (G == 0u) return bid;
    const uint32_t full = n / (8u * G) * (8u * G);
    if (bid >= full) return bid;
    const uint32_t x = bid & 7u, k = bid >> 3;
    return ((k / G) * 8u + x) * G + k % G;
}

// occupancy of the queue kernel (waves per SIMD the register allocation must allow): the queue kernel of brick_dim 1
// and 4 fits 96 VGPRs (5 waves per SIMD instead of 4, no spills under the iterative-ilp scheduler of _build.py);
// brick_dim 2 would spill 4 VGPRs and 8..32 16, so they keep 4 waves (the minimum of 4 compiles to the same code as no
// attribute)
#define VHX_QUEUE_ATTR __attribute__((amdgpu_waves_per_eu(!COUNT && (BD == 1 || BD == 4) ? 5 : 4)))

// One workgroup = 256 lanes = a 16x16 pixel block made of four 8x8 wave tiles (wave64-coherent ray bundles, the
// 8x8 footprint of the reference's @workgroup_size(8, 8, 1)). Blocks are dealt tile by tile.
// Depth-prepass mode (opt-in, not the reference path; SURVEY.md 8f #4, viewport_render.wgsl:702-726): a half-resolution
// depth frame traced first; a full-resolution ray starts at the minimum of the 4 depth texels (x/2, y/2) .. (x/2 + 1,
// y/2 + 1) (clamped at the edge) minus `margin`, and misses outright where that minimum is +inf (all four missed)
struct FastD {
    const float *depth;
    uint32_t w, h;
    float margin;
};
__device__ __forceinline__ float prepass_start(const FastD &f, uint32_t px, uint32_t py) {
    const uint32_t x0 = px >> 1, y0 = py >> 1;
    const uint32_t x1 = x0 + 1 < f.w ? x0 + 1 : f.w - 1, y1 = y0 + 1 < f.h ? y0 + 1 : f.h - 1;
    const float m = __builtin_fminf(__builtin_fminf(f.depth[(uint64_t)y0 * f.w + x0], f.depth[(uint64_t)y1 * f.w + x0]),
                                    __builtin_fminf(f.depth[(uint64_t)y0 * f.w + x1], f.depth[(uint64_t)y1 * f.w + x1]));
    return m - f.margin;
}

// Pass 0's abandoned rays listed per workgroup in the order of the pass-1 queue (ListOrder, lo.tx > 0; the
// framebuffer layout): workgroup position b is block (bx, by) of a tile of 2^tbl x 2^tbl blocks, the tiles row-major
// (tx per row), the blocks of a tile and the pixels of a block in Morton order -- the 16x16 block's four 8x8 waves are
// its Morton quadrants, and lane l is pixel (even bits of l, odd bits of l) of its wave's 8x8 -- so the lists in
// position order are the frame's abandoned rays in the FlagOrder of 2^(tbl+4)-pixel tiles with Morton inside (zin 1),
// without a flag per pixel and the compaction kernels over every pixel. A wave holds the same 64 pixels either way.
struct ListOrder {
    uint32_t tx, tbl;
    // tl = 1: the tile layout (a rank's tile set, vhx_mgpu) lists its abandoned rays too, in its own block order --
    // tile by tile, 16x16 blocks row-major inside a tile, a block's four 8x8 waves, each wave's 64 pixels row-major:
    // the queue order of its flags (output-index order) up to the order of the waves inside a 16x16 block
    uint32_t tl;
};
__device__ __forceinline__ void list_block(const ListOrder &lo, uint32_t b, uint32_t &bx, uint32_t &by) {
    const uint32_t tb = b >> (2u * lo.tbl), m = b & ((1u << (2u * lo.tbl)) - 1u);
    bx = ((tb % lo.tx) << lo.tbl) + compact_bits(m);
    by = ((tb / lo.tx) << lo.tbl) + compact_bits(m >> 1);
}
// Wave-level ordered append (no barrier: a wave that finishes early leaves at once): the wave's rays with push set are
// listed at tmp[pos * 64 ...] in lane order, their number at counts[pos].
__device__ __forceinline__ void wave_append(bool push, uint32_t idx, uint32_t *tmp, uint32_t *counts, uint32_t pos) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t m = __ballot(push);
    if (push) tmp[(uint64_t)pos * 64u + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = idx;
    if (lane == 0) counts[pos] = (uint32_t)__popcll(m);
}
__device__ __forceinline__ void zero_ctl(uint32_t *zero) {
    if (zero && blockIdx.x == 0)
        for (uint32_t w = threadIdx.x; w < QCTL_WORDS - 16u; w += blockDim.x) zero[w] = 0u;
}

// Fused hard shadows (vhx_set_shadow_light; the FUSE instantiations, BASELINE config 5): a lane whose primary ray
// finished goes on, in the same pass, with the hit's shadow ray -- the shadow semantics of vhx_trace_shadows (from
// impact + normal * 1e-3 toward the light) -- while the nodes of the hit's descent are still in this
// CU's caches. A shadow ray abandoned at the pass budget saves its state at its pixel's index (the primary ray's is
// done by then) and is listed with VHX_QSHADOW (defined above k_sort_segments); a queue pass recomputes its ray from
// the stored hit record.
__device__ __forceinline__ void hit_shadow_ray(const PassQ &q, float ix, float iy, float iz, float nx, float ny,
                                               float nz, F3d &o, F3d &d) {
    o = mk(ix + nx * 1e-3f, iy + ny * 1e-3f, iz + nz * 1e-3f);  // shadow_ray's op order
    d = vnorm(mk(q.lx - o.x, q.ly - o.y, q.lz - o.z));
}
__device__ __forceinline__ void store_fused_shadow(const OutD &o, uint64_t i, bool shadowed) {
    o.shadowed[i] = shadowed ? 1u : 0u;  // store_shadow's darkening
    if (shadowed && o.rgba) o.rgba[i] = ((o.rgba[i] >> 1) & 0x007F7F7Fu) | (o.rgba[i] & 0xFF000000u);
}
// the steps a pass's budget leaves a shadow ray started after a primary ray that used `used` of them (at least 1;
// any split is bit-identical, the traversal being deterministic)
__device__ __forceinline__ uint32_t rest_budget(uint32_t budget, uint32_t used) {
    return budget >= VHX_MAX_ITERS ? budget : (budget > used + 1u ? budget - used : 1u);
}
// the shadow continuation of a finished primary ray h (output entry li of o, state index sidx); false: abandoned
template <int BD>
__device__ __forceinline__ bool fused_shadow(const DevTree &t, const uint64_t *occ_tab, const PassQ &q, const OutD &o,
                                             uint64_t li, const HitOut &h, uint32_t sidx) {
    if (!h.hit) {
        o.shadowed[li] = 0u;
        return true;
    }
    F3d so, sd;
    hit_shadow_ray(q, h.ix, h.iy, h.iz, h.nx, h.ny, h.nz, so, sd);
    HitOut hs;
    hs.bytes = 0;
    const bool fin =
        get_by_ray<false, BD>(t, occ_tab, so, sd, hs,
                              q.sbud && q.budget < VHX_MAX_ITERS ? q.sbud : rest_budget(q.budget, h.iters), q.state,
                              sidx, false, 0.0f, q.sparse);
    if (fin) store_fused_shadow(o, li, hs.hit);
    return fin;
}

template <bool COUNT, int BD, bool FAST = false, bool MIP = false, bool FUSE = false>
__global__ void __launch_bounds__(256) k_trace_primary(DevTree t, CamD cam, OutD out, uint32_t T, uint32_t tiles_x,
                                                       uint32_t tile_start, uint32_t tile_stride, uint32_t layout,
                                                       uint32_t blocks_per_tile_x, uint32_t blocks_per_tile,
                                                       PassQ q, FastD fast = FastD{}, ListOrder lo = ListOrder{}) {
    __shared__ uint64_t occ_tab[OCC_TAB_WORDS];
    fill_occ_tab(occ_tab);
    zero_ctl(q.zero);
    __syncthreads();
    const uint32_t bid = xcd_block(blockIdx.x, gridDim.x, q.xcd_group);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t lx, ly, px, py;
    if (lo.tx) {  // framebuffer layout (T = 16: a tile per block), workgroups in list order
        uint32_t bx, by;
        list_block(lo, bid, bx, by);
        lx = (wave & 1u) * 8u + compact_bits(lane);
        ly = (wave >> 1) * 8u + compact_bits(lane >> 1);
        px = bx * 16u + lx;
        py = by * 16u + ly;
    } else {
        const uint32_t j = bid / blocks_per_tile;  // j-th tile of this rank
        const uint32_t sb = bid - j * blocks_per_tile;
        const uint32_t tile = tile_start + j * tile_stride;
        // 8x8 pixels per wave, four waves per 16x16 block
        lx = (sb % blocks_per_tile_x) * 16u + (wave & 1u) * 8u + (lane & 7u);
        ly = (sb / blocks_per_tile_x) * 16u + (wave >> 1) * 8u + (lane >> 3);
        px = (tile % tiles_x) * T + lx;
        py = (tile / tiles_x) * T + ly;
    }
    const uint32_t j = lo.tx ? 0u : bid / blocks_per_tile;
    const bool valid = lx < T && ly < T && px < cam.width && py < cam.height;
    const uint64_t idx = layout == VHX_LAYOUT_FRAMEBUFFER ? (uint64_t)py * cam.width + px
                                                          : (uint64_t)j * T * T + (uint64_t)ly * T + lx;
    bool done = true;
    uint32_t tag = 0u;  // FUSE: VHX_QSHADOW when the ray left over is the hit's shadow ray
    // the early tail traces the pixels in q.skip (its kernel stores them): done here, no store, no flag
    const bool skipped = valid && q.skip && ((q.skip[idx >> 5] >> (idx & 31u)) & 1u) != 0u;
    if (valid && !skipped) {
        F3d o, d;
        HitOut h;
        h.bytes = 0;
        if (glass_clear_miss(cam, px, py, (float)t.size)) {  // the miss record, as get_by_ray's root test gives it
            o = mk(cam.ox, cam.oy, cam.oz);
            h.hit = false;
            h.iters = 0;
        } else {
            primary_ray(cam, px, py, o, d);
            const float start = FAST ? prepass_start(fast, px, py) : 0.0f;
            // queue-state mode (listed pass 0 only): this wave's abandoned rays take the slots of its list
            done = get_by_ray<COUNT, BD, FAST, MIP>(t, occ_tab, o, d, h, q.budget, q.state,
                                                    q.qmode ? (bid * 4u + wave) * 64u : (uint32_t)idx, false, start,
                                                    q.sparse, nullptr, 0, q.qmode != 0);
        }
        if (done) {
            store(t, out, idx, o, h);
            if (FUSE && !fused_shadow<BD>(t, occ_tab, q, out, idx, h, (uint32_t)idx)) {
                done = false;
                tag = VHX_QSHADOW;
            }
        } else if (COUNT && q.state) {
            out.bytes[idx] = h.bytes;  // the running count, continued by the pass that resumes the ray
        }
    }
    // every entry of the output gets its flag, so the flags need no clearing between frames: in the tile layout
    // every in-tile entry (frame padding included, done = true there); in the framebuffer layout only pixels of the
    // frame (a lane past the frame edge has no entry of its own: its idx aliases the next row or runs past the end)
    if (q.flags && (layout == VHX_LAYOUT_FRAMEBUFFER ? valid : (lx < T && ly < T)))
        q.flags[idx] = done ? 0 : 1;
    if ((lo.tx || lo.tl) && q.tmp) wave_append(!done, (uint32_t)idx | tag, q.tmp, q.counts, bid * 4u + wave);
}

// Pass 0 of a batch of frames (vhx_trace_primary_batch): frame f's 16x16 pixel blocks are blocks [f * nblocks_frame,
// (f + 1) * nblocks_frame) of one launch (XCD-dealt like k_trace_primary), with the frame's camera and outputs read from
// the batch arrays (block-uniform: scalar loads). Framebuffer layout; output index f * npix + y * width + x.
// A batch of tile sets (vhx_trace_tiles_batch; tb.T > 0): frame f's blocks cover the T x T tiles starts[f] +
// j * stride, j < the largest set's tile count, 16x16 blocks row-major inside a tile (k_trace_primary's tile layout);
// output index f * npix + j * T * T + y * T + x inside the tile.
struct TileB {
    uint32_t T, tiles_x, ntiles, stride, bpx, bpt;
};
// VHX_BATCH_WAVES (a variant build): waves per SIMD the batch pass 0 must allow (0: the compiler's choice, 70 VGPRs
// for brick_dim 4 = 7 waves)
#ifndef VHX_BATCH_WAVES
#define VHX_BATCH_WAVES 0
#endif
#if VHX_BATCH_WAVES
#define VHX_BATCH_ATTR __attribute__((amdgpu_waves_per_eu(VHX_BATCH_WAVES)))
#else
#define VHX_BATCH_ATTR
#endif
// Division of a workgroup-uniform index by a launch constant d as a multiply and a shift (Granlund & Montgomery,
// "Division by invariant integers using multiplication", theorem 4.2 with N = 31): m = ceil(2^(31 + l) / d),
// l = ceil(log2 d), fits 32 bits and floor(n * m / 2^(31 + l)) = n / d for every n < 2^31 -- block, tile and frame
// indices all are (trace_batch refuses larger batches). Three scalar instructions instead of a division sequence.
struct UDiv {
    uint32_t m, sh;  // d = 0 (a path the launch does not take): m = 0, every quotient 0
};
static UDiv udiv_of(uint32_t d) {
    if (d == 0u) return UDiv{0u, 0u};
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    return UDiv{(uint32_t)(((1ull << (31u + l)) + d - 1u) / d), 31u + l};
}
__device__ __forceinline__ uint32_t udiv(uint32_t n, const UDiv &d) { return (uint32_t)(((uint64_t)n * d.m) >> d.sh); }

// What the batch pass 0 derives from its launch parameters, computed once on the host (batch_grid): the kernel reads
// no grid size and divides nothing.
struct BatchGrid {
    uint32_t nfr;     // frames in the batch
    uint32_t xfull;   // xcd_block: the workgroups below this are permuted (0: dispatch order)
    uint32_t xshift;  // ... log2 of the run length when it is a power of two (shifts), else ~0u (xg)
    UDiv xg;          // by the run length
    UDiv split;       // workgroup -> (frame, frame block): by nfr (interleaved) or by nblocks_frame (frame-major)
    UDiv ltx, bx;     // frame block -> block coordinates: by lo.tx (list order) or by blocks_x (row-major)
    UDiv bpt, bpx, tiles_x;  // tile sets: by TileB's bpt, bpx and tiles_x
    // the worklist (k_classify_blocks, the kernel's `work`): the frame's 16x16 raster blocks and the frames' common size
    uint32_t sbx, sby, W, H;
};
static BatchGrid batch_grid(uint32_t nblocks, uint32_t nfr, uint32_t nblocks_frame, uint32_t blocks_x, const PassQ &q,
                            const ListOrder &lo, const TileB &tb) {
    BatchGrid g{};
    const uint32_t G = q.xcd_group;
    g.nfr = nfr;
    // 8 * G in 64 bits: a run length of 2^29 and more leaves every workgroup in the tail (xcd_block)
    g.xfull = G && 8ull * G <= nblocks ? (uint32_t)(nblocks / (8ull * G) * (8ull * G)) : 0u;
    g.xshift = ~0u;
    if (G && (G & (G - 1u)) == 0u)
        for (g.xshift = 0; (1u << g.xshift) < G;) ++g.xshift;
    g.xg = udiv_of(G);
    g.split = udiv_of(q.finter ? nfr : nblocks_frame);
    g.ltx = udiv_of(lo.tx);
    g.bx = udiv_of(blocks_x);
    g.bpt = udiv_of(tb.bpt);
    g.bpx = udiv_of(tb.bpx);
    g.tiles_x = udiv_of(tb.tiles_x);
    return g;
}
// xcd_block and list_block on a workgroup-uniform index with the host's constants: scalar code throughout
__device__ __forceinline__ uint32_t xcd_block(uint32_t bid, uint32_t G, const BatchGrid &g) {
    if (bid >= g.xfull) return bid;
    const uint32_t x = bid & 7u, k = bid >> 3;
    if (g.xshift != ~0u) return ((((k >> g.xshift) << 3) + x) << g.xshift) + (k & (G - 1u));
    const uint32_t kq = udiv(k, g.xg);
    return (kq * 8u + x) * G + (k - kq * G);
}
__device__ __forceinline__ void list_block(const ListOrder &lo, const UDiv &ltx, uint32_t b, uint32_t &bx,
                                           uint32_t &by) {
    const uint32_t tb = b >> (2u * lo.tbl), m = b & ((1u << (2u * lo.tbl)) - 1u);
    const uint32_t ty = udiv(tb, ltx);
    bx = ((tb - ty * lo.tx) << lo.tbl) + compact_bits(m);
    by = (ty << lo.tbl) + compact_bits(m >> 1);
}
// xcd_block over the first n workgroups of the launch, n read on the device (the worklist's tree part, n < 2^31)
__device__ __forceinline__ uint32_t xcd_block_n(uint32_t bid, uint32_t n, uint32_t G, const BatchGrid &g) {
    if (G == 0u) return bid;
    uint32_t full;  // n / 8G * 8G
    if (g.xshift != ~0u) full = g.xshift >= 29u ? 0u : (n >> (g.xshift + 3u)) << (g.xshift + 3u);
    else full = udiv(n >> 3, g.xg) * 8u * G;
    if (bid >= full) return bid;
    const uint32_t x = bid & 7u, k = bid >> 3;
    if (g.xshift != ~0u) return ((((k >> g.xshift) << 3) + x) << g.xshift) + (k & (G - 1u));
    const uint32_t kq = udiv(k, g.xg);
    return (kq * 8u + x) * G + (k - kq * G);
}
// a logical workgroup index of a batch's pass 0 -> its frame and frame block (interleaved or frame-major)
__device__ __forceinline__ void batch_split(uint32_t bid, uint32_t finter, uint32_t nblocks_frame, const BatchGrid &g,
                                            uint32_t &f, uint32_t &sb) {
    const uint32_t bq = udiv(bid, g.split);
    f = finter ? bid - bq * g.nfr : bq;
    sb = finter ? bq : bid - bq * nblocks_frame;
}

// The worklist of a batch's pass 0 (vhx_ctx::skyblocks; whole frames in list order without fused shadows): the
// launch's logical workgroup indices -- position p is frame block sb of frame f after the frame interleave, in list
// order: the order of the lists and of the pass-1 queue -- partitioned. work[WORK_HDR ...] holds first the ntree
// blocks with a pixel that may enter the tree, ascending in p, then the nsky blocks inside the frame whose every pixel
// misses the root cube on the exact path (block_is_sky, skyblock.hpp); the blocks of the list order's padding past
// the frame are in neither part. work[0] = ntree, work[1] = ntree + nsky, work[2] = 256 ntree (the pass-0 lists'
// extent in rays, the device-side length its compaction takes).
// k_classify_blocks: one thread per position; per wave of 64 positions the two ballots, per workgroup of 256 their
// counts (tree counts at counts[g], sky counts at counts[ng + g]: one exclusive scan over 2 ng counts places the sky
// part behind the tree part and leaves ntree at offsets[ng], the sum at work[1]). k_emit_worklist, on the same grid,
// writes the entries.
#define WORK_HDR 64u
__global__ void __launch_bounds__(256) k_classify_blocks(const CamD *__restrict__ cams, BatchGrid bg, ListOrder lo,
                                                         uint32_t nblocks_frame, uint32_t finter, uint32_t nblocks,
                                                         uint32_t tree_size, uint64_t *__restrict__ masks,
                                                         uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_cnt[8];
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool tree = false, sky = false;
    if (p < nblocks) {
        uint32_t f, sb, bx, by;
        batch_split(p, finter, nblocks_frame, bg, f, sb);
        list_block(lo, bg.ltx, sb, bx, by);
        if (bx < bg.sbx && by < bg.sby) {
            const CamD &c = cams[f];
            const SkyCam s{c.model, c.width, c.height, {c.ox, c.oy, c.oz}, {c.blx, c.bly, c.blz}, {c.rx, c.ry, c.rz},
                           {c.ux, c.uy, c.uz}, c.pw, c.ph};
            const uint32_t x1 = min(bx * 16u + 15u, c.width - 1u), y1 = min(by * 16u + 15u, c.height - 1u);
            sky = block_is_sky(s, tree_size, bx * 16u, by * 16u, x1, y1);
            tree = !sky;
        }
    }
    const uint64_t mt = __ballot(tree), ms = __ballot(sky);
    const uint32_t w = p >> 6, wave = threadIdx.x >> 6;  // (the ballots hold four words per workgroup of the grid)
    if ((threadIdx.x & 63u) == 0u) {
        masks[2u * w] = mt;
        masks[2u * w + 1u] = ms;
        s_cnt[wave] = (uint32_t)__popcll(mt);
        s_cnt[4u + wave] = (uint32_t)__popcll(ms);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        counts[gridDim.x + blockIdx.x] = s_cnt[4] + s_cnt[5] + s_cnt[6] + s_cnt[7];
    }
}
__global__ void __launch_bounds__(256) k_emit_worklist(const uint64_t *__restrict__ masks,
                                                       const uint32_t *__restrict__ offsets,
                                                       uint32_t *__restrict__ work) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x, w = p >> 6, lane = threadIdx.x & 63u;
    if (p == 0u) {
        work[0] = offsets[gridDim.x];
        work[2] = offsets[gridDim.x] * 256u;
    }
    const uint64_t mt = masks[2u * w], ms = masks[2u * w + 1u], below = (1ull << lane) - 1ull;
    uint32_t ot = offsets[blockIdx.x], os = offsets[gridDim.x + blockIdx.x];
    for (uint32_t v = blockIdx.x * 4u; v < w; ++v) {  // the workgroup's waves ahead of this one
        ot += (uint32_t)__popcll(masks[2u * v]);
        os += (uint32_t)__popcll(masks[2u * v + 1u]);
    }
    if ((mt >> lane) & 1ull) work[WORK_HDR + ot + (uint32_t)__popcll(mt & below)] = p;
    if ((ms >> lane) & 1ull) work[WORK_HDR + os + (uint32_t)__popcll(ms & below)] = p;
}

// The workgroup's position, frame and frame block are the same in every lane by construction; readfirstlane says so
// to the compiler, which then keeps them, everything derived from them (the block's coordinates, the tile, the
// addresses of cams[f], outs[f] and starts[f]) and the frame's camera and output pointers in scalar registers: scalar
// arithmetic, scalar loads, and scalar branches on the null output pointers in store(). Left to itself it computed
// all of that per lane (about 125 of the 150 vector instructions ahead of the sky test) and read cams[f] and outs[f]
// with per-lane loads, outs[f] field by field between the stores at the end of every wave. The fixed cost of a wave
// on the headline path (brick_dim 4, list order, interleaved frames), straight-line instructions: kernel entry to the
// sky test 307 (169 vector ALU, 11 vector loads) -> 176 (33, 1); sky test to the end of a wave that holds sky only
// 209 (107 vector ALU, 14 vector memory, 15 waits) -> 185 (83, 6, 4). Pass 0 of the bench frame: 167.2 M -> 146.6 M
// wave64 VALU instructions, 77 -> 70 VGPRs (6 -> 7 waves per SIMD); profiles/r07/uniform/, DESIGN.md §3.
// The nine output pointers are read after the traversal, so they hold no scalar registers across it.
template <int BD, bool FUSE = false>
__global__ void __launch_bounds__(256) VHX_BATCH_ATTR k_trace_primary_batch(DevTree t, const CamD *__restrict__ cams,
                                                             const OutD *__restrict__ outs, uint32_t nblocks_frame,
                                                             uint32_t blocks_x, uint32_t npix, PassQ q, BatchGrid bg,
                                                             ListOrder lo = ListOrder{}, TileB tb = TileB{},
                                                             const uint32_t *__restrict__ starts = nullptr,
                                                             const uint32_t *__restrict__ work = nullptr) {
    __shared__ uint64_t occ_tab[OCC_TAB_WORDS];
    zero_ctl(q.zero);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    // bid: the workgroup's logical index (frame and frame block); pos: its position among the pass's lists
    uint32_t bid, pos;
    if (!FUSE && work) {
        // The worklist (k_classify_blocks): the launch's first ntree workgroups trace the tree blocks, XCD-dealt among
        // themselves, and list their rays at the block's rank -- the lists in position order are those of the whole
        // launch without its empty ones; the next nsky workgroups write a sky block's miss records, one wave of each
        // (no occupancy table, no barrier, no camera, no list entry); the rest, the list order's padding, end here.
        // Tree work starts first and the fills are the launch's tail. Every branch is workgroup-uniform (scalar).
        const uint32_t ntree = work[0], nall = work[1];
        if (blockIdx.x >= nall) return;
        if (blockIdx.x >= ntree) {
            if (wave != 0u) return;
            uint32_t f, sb, bx, by;
            batch_split(__builtin_amdgcn_readfirstlane(work[WORK_HDR + blockIdx.x]), q.finter, nblocks_frame, bg, f, sb);
            list_block(lo, bg.ltx, sb, bx, by);
            // the plane pointers in scalar loads issued together, one wait (the empty asm keeps the compiler from
            // reading each behind the branch on the one before)
            const OutD out = outs[f];
            asm volatile("" ::"s"(out.value), "s"(out.cell), "s"(out.voxel), "s"(out.rgba), "s"(out.impact),
                         "s"(out.normal), "s"(out.depth));
            store_miss_block(out, bx, by, bg.W, bg.H);
            return;
        }
        pos = __builtin_amdgcn_readfirstlane(xcd_block_n(blockIdx.x, ntree, q.xcd_group, bg));
        bid = __builtin_amdgcn_readfirstlane(work[WORK_HDR + pos]);
    } else {
        pos = bid = __builtin_amdgcn_readfirstlane(xcd_block(blockIdx.x, q.xcd_group, bg));
    }
    // frame-major (all of frame 0's blocks, then frame 1's, ...) or interleaved (block sb of every frame in turn: the
    // frames' rays through one screen region run together and share the caches)
    uint32_t f, sb;
    batch_split(bid, q.finter, nblocks_frame, bg, f, sb);
    f = __builtin_amdgcn_readfirstlane(f);
    sb = __builtin_amdgcn_readfirstlane(sb);
    uint32_t px = 0, py = 0, local;
    if (!tb.T) {
        uint32_t bx, by;
        if (lo.tx) {  // this frame's blocks in list order (k_trace_primary)
            list_block(lo, bg.ltx, sb, bx, by);
            px = bx * 16u + (wave & 1u) * 8u + compact_bits(lane);
            py = by * 16u + (wave >> 1) * 8u + compact_bits(lane >> 1);
        } else {
            by = udiv(sb, bg.bx);
            bx = sb - by * blocks_x;
            px = bx * 16u + (wave & 1u) * 8u + (lane & 7u);
            py = by * 16u + (wave >> 1) * 8u + (lane >> 3);
        }
    }
    fill_occ_tab(occ_tab);
    __syncthreads();
    const CamD cam = cams[f];
    bool valid, entry;  // entry: the position has an output entry (its flag is written)
    if (tb.T) {
        const uint32_t j = __builtin_amdgcn_readfirstlane(udiv(sb, bg.bpt)), sbb = sb - j * tb.bpt;
        const uint32_t sby = udiv(sbb, bg.bpx);
        const uint32_t lx = (sbb - sby * tb.bpx) * 16u + (wave & 1u) * 8u + (lane & 7u);
        const uint32_t ly = sby * 16u + (wave >> 1) * 8u + (lane >> 3);
        // a tile past 2^31 (starts or stride out of range) gets a wrong quotient below and is not valid anyway
        const uint32_t tile = __builtin_amdgcn_readfirstlane(starts[f] + j * tb.stride);
        const uint32_t tyy = udiv(tile, bg.tiles_x);
        px = (tile - tyy * tb.tiles_x) * tb.T + lx;
        py = tyy * tb.T + ly;
        entry = lx < tb.T && ly < tb.T;
        valid = entry && tile < tb.ntiles && px < cam.width && py < cam.height;
        local = (j * tb.T + ly) * tb.T + lx;
    } else {
        valid = entry = px < cam.width && py < cam.height;
        local = py * cam.width + px;
    }
    const uint64_t idx = (uint64_t)f * npix + local;
    bool done = true;
    uint32_t tag = 0u;  // FUSE: VHX_QSHADOW when the ray left over is the hit's shadow ray
    if (valid) {
        F3d o, d;
        HitOut h;
        h.bytes = 0;
        if (glass_clear_miss(cam, px, py, (float)t.size)) {  // k_trace_primary
            o = mk(cam.ox, cam.oy, cam.oz);
            h.hit = false;
            h.iters = 0;
        } else {
            primary_ray(cam, px, py, o, d);
            // FLAT: the walks in the form that full SIMDs run fastest (trace.hpp, walk_cells)
            done = get_by_ray<false, BD, false, false, true>(t, occ_tab, o, d, h, q.budget, q.state,
                                         q.qmode ? (pos * 4u + wave) * 64u : (uint32_t)idx, false, 0.0f, q.sparse,
                                         nullptr, 0, q.qmode != 0);
        }
        if (done) {
            const OutD out = outs[f];  // one scalar load of the nine pointers
            store(t, out, local, o, h);
            if (FUSE && !fused_shadow<BD>(t, occ_tab, q, out, local, h, (uint32_t)idx)) {
                done = false;
                tag = VHX_QSHADOW;
            }
        }
    }
    // every entry gets its flag (a tile set's entries past the frame edge or past a smaller set's tiles: 0)
    if (q.flags && entry) q.flags[idx] = done ? 0 : 1;
    if ((lo.tx || lo.tl) && q.tmp) wave_append(!done, (uint32_t)idx | tag, q.tmp, q.counts, pos * 4u + wave);
}

template <bool COUNT, int BD, bool MIP = false>
__global__ void __launch_bounds__(256) k_trace_rays(DevTree t, const float *__restrict__ rays, uint64_t n, OutD out,
                                                    PassQ q) {
    __shared__ uint64_t occ_tab[OCC_TAB_WORDS];
    fill_occ_tab(occ_tab);
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool done = true;
    if (i < n) {
        const F3d o = mk(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        const F3d d = mk(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
        HitOut h;
        h.bytes = 0;
        done = get_by_ray<COUNT, BD, false, MIP>(t, occ_tab, o, d, h, q.budget, q.state, (uint32_t)i);
        if (done)
            store(t, out, i, o, h);
        else if (COUNT && q.state)
            out.bytes[i] = h.bytes;
    }
    if (q.tmp) block_append(!done, (uint32_t)i, q.tmp, q.counts, blockIdx.x);
}


#if VHX_CHAIN
// One ray per wave (lane 0; a workgroup of one wave per ray), traced whole with the chain stamps (trace.hpp,
// VHX_CHAIN): per ray VHX_CHAIN_WORDS words -- [0] cycles of the traversal, [1] node-load waits, [2] probes, [3] POP /
// PUSH bookkeeping, [4] ADVANCE walks, [5] loop overhead, [6] node iterations, [7] probes, [8] ADVANCE walks,
// [9] steps, [10] hit value, [16..16+VHX_CHAIN_HIST) node-load wait histogram (64-cycle buckets)
#define VHX_CHAIN_WORDS 64u
template <int BD>
__global__ void __launch_bounds__(64) k_chain(DevTree t, CamD cam, const uint32_t *__restrict__ pix, uint32_t n,
                                              unsigned long long *__restrict__ out) {
    __shared__ uint64_t occ_tab[OCC_TAB_WORDS];
    fill_occ_tab(occ_tab);
    __syncthreads();
    if (threadIdx.x != 0 || blockIdx.x >= n) return;
    const uint32_t idx = pix[blockIdx.x], py = idx / cam.width, px = idx - py * cam.width;
    F3d o, d;
    primary_ray(cam, px, py, o, d);
    HitOut h;
    h.bytes = 0;
    h.chain = ChainAcc{};
    const unsigned long long t0 = chain_stamp();
    get_by_ray<false, BD>(t, occ_tab, o, d, h, VHX_MAX_ITERS);
    const unsigned long long t1 = chain_stamp();
    unsigned long long *w = out + (uint64_t)blockIdx.x * VHX_CHAIN_WORDS;
    const unsigned long long v[11] = {t1 - t0,        h.chain.load,   h.chain.probe, h.chain.move,
                                      h.chain.adv,    h.chain.other,  h.chain.nload, h.chain.nprobe,
                                      h.chain.nadv,   h.iters,        h.hit ? h.value : VHX_EMPTY};
    for (uint32_t k = 0; k < 11u; ++k) w[k] = v[k];
    for (uint32_t k = 0; k < VHX_CHAIN_HIST; ++k) w[16 + k] = h.chain.hist[k];
}
#endif

// Queue pass: each wave takes 64 consecutive queue entries at a time from a shared counter until the queue written
// by the previous pass is drained (its length is read on the device; the host never synchronises between passes).
// Store of a shadow ray's result: shadowed flag (in out.value), rgb halved in place when shadowed, byte count.
__device__ __forceinline__ void store_shadow(const OutD &o, uint64_t i, const HitOut &h) {
    o.value[i] = h.hit ? 1u : 0u;
    if (o.rgba && h.hit) o.rgba[i] = ((o.rgba[i] >> 1) & 0x007F7F7Fu) | (o.rgba[i] & 0xFF000000u);
    if (o.bytes) o.bytes[i] = h.bytes;
}

// Camera, ray source and outputs of a queue pass: read through a pointer where a wave picks up or stores a ray, so
// they do not occupy scalar registers across the traversal (as kernel arguments they did, and spilled ~100 SGPRs)
struct QueueArgs {
    CamD cam;
    RaySrc src;
    OutD out;
};
__global__ void k_put_queue_args(QueueArgs a, QueueArgs *dst) {
    if (threadIdx.x == 0) *dst = a;
}

// QM: the queue-state mode (PassQ::qmode) as a separate instantiation: carried as a run-time flag, its state pointers
// and slot indices cost the default kernel 2 VGPRs and 4 spilled ones
template <bool COUNT, int BD, bool MIP = false, bool FUSE = false, bool QM = false>
__global__ void __launch_bounds__(256) VHX_QUEUE_ATTR k_trace_queue(DevTree t, const QueueArgs *qa, const uint32_t *__restrict__ in,
                                                     const uint32_t *in_n, uint32_t *grab, PassQ q) {
    __shared__ uint64_t occ_tab[OCC_TAB_WORDS];
    fill_occ_tab(occ_tab);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = *in_n;
    const uint32_t rpw = pass_rpw(q.rpw, q.tw, n);
    // q.qxcd = G > 0: chunk runs of G are dealt round-robin over the XCDs (blockIdx % 8 runs on one XCD and shares
    // its L2), each XCD's waves take its runs in order from their own counter (grab[64 (x + 1)]) and move on to the next
    // XCD's runs once theirs are taken
    uint32_t xcd = blockIdx.x & 7u, tries = 0;
    // only a queue with more chunks than waves is dealt over the XCDs (a smaller one starts every chunk at once
    // anyway and measured slower dealt)
    const uint32_t qxcd = (n + rpw - 1) / rpw > gridDim.x * (blockDim.x / 64u) ? q.qxcd : 0u;
    for (;;) {
        uint32_t base = 0;
        if (qxcd == 0u) {
            if (lane == 0) base = atomicAdd(grab, rpw);
            base = __shfl(base, 0);
            if (base >= n) break;  // wave-uniform
        } else {
            const uint32_t G = qxcd;
            const uint32_t nch = (n + rpw - 1) / rpw, nfull = nch / G, rem = nch % G;
            uint32_t chunk = 0xFFFFFFFFu;
            while (tries < 8u) {
                // XCD xcd owns runs xcd, xcd + 8, ...: kmax of its takes are valid (the last run may be partial); an
                // exhausted counter is recognised by a plain load, so finished waves do not queue atomics on it
                const uint32_t kmax = (nfull > xcd ? (nfull - xcd + 7u) / 8u : 0u) * G +
                                      (rem > 0u && nfull % 8u == xcd ? rem : 0u);
                uint32_t k = 0xFFFFFFFFu;
                uint32_t *ctr = grab + 64u * (xcd + 1u);
                if (lane == 0 && __atomic_load_n(ctr, __ATOMIC_RELAXED) < kmax) k = atomicAdd(ctr, 1u);
                k = __builtin_amdgcn_readfirstlane(__shfl(k, 0));
                if (k < kmax) {
                    chunk = ((k / G) * 8u + xcd) * G + k % G;
                    break;
                }
                xcd = (xcd + 1u) & 7u;
                ++tries;
            }
            if (chunk == 0xFFFFFFFFu) break;
            base = chunk * rpw;
        }
        const uint32_t i = base + lane;
        bool push = false;
        uint32_t idx = 0, tag = 0;
        if (lane < rpw && i < n) {
            idx = in[i];
            F3d o, d;
            const QueueArgs *a = qa;
            asm volatile("" : "+s"(a));  // loads through `a` stay here (not hoisted into live registers)
            // FUSE: the entry's frame outputs (a batch's frame, or the frame's); a shadow entry's ray from its hit record
            bool sh = false;
            OutD fo{};
            uint64_t li = 0;
            if (FUSE) {
                sh = (idx & VHX_QSHADOW) != 0u;
                idx &= ~VHX_QSHADOW;
                if (a->src.kind == 4u) {
                    const uint32_t f = idx / a->src.npix;
                    fo = a->src.outs[f];
                    li = idx - f * a->src.npix;
                } else {
                    fo = a->out;
                    li = idx;
                }
            }
            if (FUSE && sh)
                hit_shadow_ray(q, fo.impact[3 * li], fo.impact[3 * li + 1], fo.impact[3 * li + 2], fo.normal[3 * li],
                               fo.normal[3 * li + 1], fo.normal[3 * li + 2], o, d);
            else
                ray_of(a->cam, a->src, idx, o, d);
            HitOut h;
            h.bytes = COUNT && q.resume ? a->out.bytes[idx] : 0u;
            // queue-state mode: resumed from queue position i, abandoned into this chunk's list slots (base = chunk *
            // rays per wave, the chunk's list position)
            const bool fin = get_by_ray<COUNT, BD, false, MIP>(
                t, occ_tab, o, d, h, q.budget, q.state, QM ? base : idx, q.resume != 0, 0.0f, q.sparse,
                QM ? q.sin : nullptr, QM ? i : 0u, QM && q.tmp);
            const QueueArgs *b = qa;
            asm volatile("" : "+s"(b));
            if (!fin) {
                push = true;
                tag = FUSE && sh ? VHX_QSHADOW : 0u;
                if (COUNT && q.state) b->out.bytes[idx] = h.bytes;
            } else if (FUSE) {
                if (sh) {
                    store_fused_shadow(fo, li, h.hit);
                } else {  // a primary ray finished here: its shadow ray goes on in this lane
                    store(t, fo, li, o, h);
                    if (!fused_shadow<BD>(t, occ_tab, q, fo, li, h, idx)) {
                        push = true;
                        tag = VHX_QSHADOW;
                    }
                }
            } else if (b->src.kind == 3u) {
                store_shadow(b->out, idx, h);
            } else if (b->src.kind == 5u) {
                const uint32_t f = idx / b->src.npix;
                OutD so{};
                so.value = b->src.shs[f].shadowed;
                so.rgba = b->src.shs[f].rgba;
                store_shadow(so, idx - f * b->src.npix, h);
            } else if (b->src.kind == 4u) {
                const uint32_t f = idx / b->src.npix;
                store(t, b->src.outs[f], idx - f * b->src.npix, o, h);
            } else {
                store(t, b->out, idx, o, h);
                if (q.tail_out && h.iters >= q.tail_min) tail_record(q.tail_out, q.tail_cap, idx);
            }
        }
        if (q.tmp) {  // this chunk's abandoned rays, in lane order
            const uint32_t chunk = base / rpw;
            const uint64_t m = __ballot(push);
            if (push) q.tmp[(uint64_t)chunk * rpw + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = idx | tag;
            if (lane == 0) q.counts[chunk] = (uint32_t)__popcll(m);
        }
    }
}

// Early tail (vhx_ctx::tail_*): the pixels of a recorded list as bits of the frame's skip mask (cleared before)
__global__ void k_tail_mask(const uint32_t *__restrict__ list, uint32_t cap, uint32_t npix, uint32_t *mask) {
    const uint32_t n = min(list[0], cap);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t idx = list[64u + i];
        if (idx < npix) atomicOr(mask + (idx >> 5), 1u << (idx & 31u));
    }
}

// Early tail: the listed pixels of a framebuffer frame traced to the end from the start of the frame, rpw to a wave
// (entry i of the list in wave i / rpw), on the context's second stream while pass 0 skips them; each still-long ray
// is listed again for the next lone frame. Same ray, traversal and store as k_trace_primary + the queue passes.
template <int BD>
__global__ void __launch_bounds__(256) k_trace_tail(DevTree t, CamD cam, OutD out, const uint32_t *__restrict__ list,
                                                    uint32_t *next, uint32_t cap, uint32_t tail_min, uint32_t rpw,
                                                    uint32_t prio) {
    __shared__ uint64_t occ_tab[OCC_TAB_WORDS];
    fill_occ_tab(occ_tab);
    __syncthreads();
    // issue priority of these waves over the frame's other waves on their SIMD (a serial chain is what they carry)
    if (prio == 3u) __builtin_amdgcn_s_setprio(3);
    else if (prio == 2u) __builtin_amdgcn_s_setprio(2);
    else if (prio == 1u) __builtin_amdgcn_s_setprio(1);
    const uint32_t n = min(list[0], cap);
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t i = wave * rpw + lane;
    if (lane >= rpw || i >= n) return;
    const uint32_t idx = list[64u + i];
    if (idx >= cam.width * cam.height) return;
    const uint32_t px = idx % cam.width, py = idx / cam.width;
    F3d o, d;
    HitOut h;
    h.bytes = 0;
    if (glass_clear_miss(cam, px, py, (float)t.size)) {
        o = mk(cam.ox, cam.oy, cam.oz);
        h.hit = false;
        h.iters = 0;
    } else {
        primary_ray(cam, px, py, o, d);
        get_by_ray<false, BD>(t, occ_tab, o, d, h, VHX_MAX_ITERS, nullptr, 0u, false, 0.0f, 0u);
    }
    store(t, out, idx, o, h);
    if (h.iters >= tail_min) tail_record(next, cap, idx);
}

// ------------------------------------------------------------------------------------------------ host helpers
template <int V>
struct BdTag {
    static constexpr int value = V;
};
// brick_dim is a template parameter of the traversal kernels (exact / brick_dim as a constant multiply)
template <class F>
static bool dispatch_bd(uint32_t bd, F &&f) {
    switch (bd) {
        case 1: f(BdTag<1>{}); return true;
        case 2: f(BdTag<2>{}); return true;
        case 4: f(BdTag<4>{}); return true;
        case 8: f(BdTag<8>{}); return true;
        case 16: f(BdTag<16>{}); return true;
        case 32: f(BdTag<32>{}); return true;
        default: return false;
    }
}
static DevTree dev_tree(const vhx_ctx *c) {
    DevTree t;
    t.hdr = (const uint4 *)c->tree->hdr.ptr;
    t.children = (const uint32_t *)c->tree->raw[VHX_BUF_NODE_CHILDREN].ptr;
    t.voxels = (const uint32_t *)c->tree->raw[VHX_BUF_VOXELS].ptr;
    t.brick_occ = (const uint64_t *)c->tree->brick_occ.ptr;
    t.child_rec = (const uint4 *)c->tree->child_rec.ptr;
    t.solid = (const uint32_t *)c->tree->raw[VHX_BUF_SOLID_VALUES].ptr;
    t.color = (const uint32_t *)c->tree->raw[VHX_BUF_COLOR_PALETTE].ptr;
    t.color_count = c->tree->desc.color_count;
    t.node_count = c->tree->desc.node_count;
    t.size = c->tree->desc.boxtree_size;
    t.bd = c->tree->desc.brick_dim;
    t.occ_words = c->tree->occ_words;
    t.mips = c->tree->mips_on ? (const uint32_t *)c->tree->mips.ptr : nullptr;
    return t;
}

struct HostOut {
    OutD dev{};
    std::vector<std::pair<void *, std::pair<void *, uint64_t>>> copies;  // (host dst, (dev src, bytes))
};

// Maps the caller's vhx_hits onto device pointers (scratch-backed when the caller passed host memory).
// zero_fill: staging is cleared first (tile layout: pixels past the frame edge are never written and read back as 0)
static int map_out(vhx_ctx *c, const vhx_hits *h, uint64_t n, int on_device, HostOut &ho, bool zero_fill = false) {
    struct F {
        void *user;
        uint64_t per;
        void **dst;
    } fields[] = {{h->value, 4, (void **)&ho.dev.value},   {h->cell, 4, (void **)&ho.dev.cell},
                  {h->voxel, 12, (void **)&ho.dev.voxel},  {h->impact, 12, (void **)&ho.dev.impact},
                  {h->normal, 12, (void **)&ho.dev.normal}, {h->depth, 4, (void **)&ho.dev.depth},
                  {h->rgba, 4, (void **)&ho.dev.rgba},     {h->bytes, 4, (void **)&ho.dev.bytes},
                  {h->shadowed, 4, (void **)&ho.dev.shadowed}};
    if (on_device) {
        for (auto &f : fields) *f.dst = f.user;
        return VHX_OK;
    }
    uint64_t total = 0;
    for (auto &f : fields)
        if (f.user) total += (f.per * n + 255) & ~255ull;
    int rc = ensure(c, c->scratch, total);
    if (rc) return rc;
    if (zero_fill && total) VHX_HIP(c, hipMemsetAsync(c->scratch.ptr, 0, total, c->stream));
    uint64_t off = 0;
    for (auto &f : fields) {
        if (!f.user) continue;
        void *p = (char *)c->scratch.ptr + off;
        *f.dst = p;
        ho.copies.push_back({f.user, {p, f.per * n}});
        off += (f.per * n + 255) & ~255ull;
    }
    return VHX_OK;
}

static int finish_out(vhx_ctx *c, HostOut &ho) {
    for (auto &cp : ho.copies)
        VHX_HIP(c, hipMemcpyAsync(cp.first, cp.second.first, cp.second.second, hipMemcpyDeviceToHost, c->stream));
    if (!ho.copies.empty()) VHX_HIP(c, hipStreamSynchronize(c->stream));
    return VHX_OK;
}

// Multi-pass plumbing: allocates queues, chunk lists and counters for `nout` rays whose pass 0 runs in `nblocks0`
// workgroups of 256 (may synchronise; called before the trace is timed). Returns the number of passes to run.
// Adaptive scheduling (ctx.hpp, Sched): the busy schedule while another context of the tree has a frame in flight on
// another stream (its last trace's use event not yet reached), else the idle one. A host-side query per other context;
// no waits.
static void select_schedule(vhx_ctx *c, bool batch = false, bool shadow = false) {
    if (!c->adaptive) {
        c->last_sched = -1;
        c->qsort = c->qsort_force >= 0 ? (uint32_t)c->qsort_force : c->sched_busy.qsort;  // a fixed schedule: the busy one's
        return;
    }
    // a batch of frames is a throughput job by itself: the frames-in-flight schedule (its passes re-pack the surviving
    // rays of every frame of the batch; the last pass's tail is shared by them all)
    bool busy = batch;
    if (!busy) {
        std::lock_guard<std::mutex> lock(c->tree->mu);
        for (vhx_ctx *u : c->tree->users)
            if (u != c && u->use_recorded && u->use_stream != c->stream && hipEventQuery(u->use_ev) == hipErrorNotReady) {
                busy = true;
                break;
            }
    }
    const vhx_ctx::Sched &s = busy ? c->sched_busy : c->sched_idle;
    std::memcpy(c->budgets, shadow ? s.shadow_budgets : s.budgets, sizeof(c->budgets));
    std::memcpy(c->sparse, s.sparse, sizeof(c->sparse));
    c->npass = shadow ? s.shadow_npass : s.npass;
    c->queue_waves = s.queue_waves_per_cu * c->cus;
    c->queue_waves0 = c->queue_waves0_force ? c->queue_waves0_force : s.queue_waves0_per_cu * c->cus;
    c->qorder = s.qorder;
    c->qsort = c->qsort_force >= 0 ? (uint32_t)c->qsort_force : s.qsort;
    c->last_sched = busy ? 1 : 0;
}

static int prepare_passes(vhx_ctx *c, uint64_t nout, uint64_t nblocks0, uint32_t &npass, bool shadow = false,
                          bool batch = false) {
    select_schedule(c, batch, shadow);
    npass = nout < 0x7FFFFFFFull ? c->npass : 1u;
    if (npass < 2 && !shadow) return VHX_OK;
    uint64_t chunks = std::max(nblocks0, (nout + 1023) / 1024), list = nblocks0 * 256;
    for (uint32_t p = 1; p < npass; ++p) {  // queue passes: chunk = one grab of rpw rays (adaptive: >= 1)
        const uint64_t r = c->rpw[p] ? c->rpw[p] : 1u;
        const uint64_t ch = (nout + r - 1) / r;
        chunks = std::max(chunks, ch);
        list = std::max(list, ch * r + 64u);
    }
    int rc = ensure(c, c->queue[0], nout * 4);
    if (!rc && (npass > 2 || shadow)) rc = ensure(c, c->queue[1], nout * 4);
    if (!rc) rc = ensure(c, c->qctl, QCTL_WORDS * sizeof(uint32_t));
    if (!rc) rc = ensure(c, c->qargs, 2 * sizeof(QueueArgs));
    if (!rc) rc = ensure(c, c->tmp, list * 4);
    if (!rc) rc = ensure(c, c->counts, chunks * 4);
    if (!rc) rc = ensure(c, c->offsets, chunks * 4);
    if (!rc) rc = ensure(c, c->scan_part, ((chunks + SCAN_SEG - 1) / SCAN_SEG) * 8);
    if (!rc) rc = ensure(c, c->flags, ((nout + 3) & ~3ull));
    if (!rc && c->resume && npass > 1) rc = ensure(c, c->state, std::max<uint64_t>(nout, c->qstate ? list : 0ull) * 64);
    if (!rc && c->resume && c->qstate && npass > 1) rc = ensure(c, c->stateq, nout * 64);
    return rc;
}

// Stream-ordered per-trace reset of the pass state (inside the timed region) for ray batches; primary and shadow
// frames zero the counters in their first compaction kernel instead.
static int reset_passes(vhx_ctx *c, uint32_t npass) {
    if (npass < 2) return VHX_OK;
    VHX_HIP(c, hipMemsetAsync(c->qctl.ptr, 0, QCTL_WORDS * sizeof(uint32_t), c->stream));
    return VHX_OK;
}

// Pass 0 traces fresh rays (the grid kernel of primary and explicit rays, or the shadow path's first queue pass);
// every later pass resumes the rays its predecessor abandoned.
static PassQ pass_q(const vhx_ctx *c, uint32_t p, uint32_t npass, bool qm = false) {
    PassQ q{};  // every field a kernel reads is set below or zero (q.zero, q.flags: null unless a caller sets them)
    const bool last = p + 1 >= npass;
    q.budget = last ? VHX_MAX_ITERS : c->budgets[p];
    q.rpw = c->rpw[p];
    q.tw = c->tw;
    q.xcd_group = c->xcd_group;
    // the unbounded last pass only: dealing the budgeted passes too measured the same (shadow frames 2.90 against
    // 2.87 ms, primary frames equal) once the XCD counters had cache lines of their own; tune "qxcd_all=1" deals every
    // queue pass (diagnostics)
    q.qxcd = last || c->qxcd_all ? c->qxcd : 0u;
    q.tmp = last ? nullptr : (uint32_t *)c->tmp.ptr;
    q.counts = (uint32_t *)c->counts.ptr;
    q.flags = nullptr;
    // the state buffer is written by every pass that can abandon rays and read by every pass after the first
    q.state = c->resume && npass > 1 && p >= c->save_from ? (uint4 *)c->state.ptr : nullptr;
    q.resume = c->resume && p > c->save_from ? 1u : 0u;
    q.sparse = last || !q.state ? 0u : c->sparse[p];
    q.qmode = qm && q.state ? 1u : 0u;
    q.sin = q.qmode ? (const uint4 *)c->stateq.ptr : nullptr;
    q.lx = c->shadow_light[0];
    q.ly = c->shadow_light[1];
    q.lz = c->shadow_light[2];
    q.sbud = c->shadow_budget;
    q.skip = nullptr;
    q.tail_out = last ? c->tail_rec : nullptr;
    q.tail_min = c->tail_min;
    q.tail_cap = c->tail_cap;
    q.finter = c->frame_interleave ? 1u : 0u;
    return q;
}

// Whether a trace runs in the queue-state mode (PassQ::qmode): its pass 0 lists its abandoned rays per wave or chunk
// (listed: the ordered primary pass 0; first_queue: pass 0 is itself a queue pass, the shadow path), every pass saves
// (save_from 0, resume on), and no queue is node-sorted (the sort reorders a queue by the states at output indices)
static bool queue_state_mode(const vhx_ctx *c, bool listed, bool first_queue, uint32_t npass) {
    // (fused shadows keep states at output indices: a pixel's primary and shadow ray are never pending together)
    // (and MIP frames: the queue kernel's queue-state instantiation is built for the exact path only)
    if (!c->qstate || !c->resume || c->save_from != 0 || npass < 2 || !(listed || first_queue) || c->shadow_on ||
        c->tree->mips_on)
        return false;
    if (!c->stateq.ptr) return false;
    for (uint32_t p = 1; p < npass && p < 32u; ++p)
        if (c->qsort && ((c->qsort_passes >> p) & 1u)) return false;
    return true;
}

// VHX_DEBUG_PASSES=1 (a diagnostic build only): synchronise after every pass step and print the queue counters
#ifndef VHX_DEBUG_PASSES
#define VHX_DEBUG_PASSES 0
#endif
static void debug_passes(vhx_ctx *c, const char *what) {
    if (!VHX_DEBUG_PASSES || !c->qctl.ptr) return;
    uint32_t v[16];
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpy(v, c->qctl.ptr, sizeof(v), hipMemcpyDeviceToHost);
    fprintf(stderr, "[vhx passes] %-24s counts %u %u %u %u ... %u  grabs %u %u %u %u\n", what, v[0], v[1], v[2], v[3],
            v[7], v[8], v[9], v[10], v[11]);
}

// Exclusive scan of nchunks counts (nchunks_host, or derived on the device from *n_in) into offsets, their sum at
// *total. At most max_chunks counts: up to c->scan_multi segments one workgroup walks them (a frame's scans); a larger
// scan (a batch of frames: one workgroup took ~10 us per segment while the rest of the GPU waited) sums the segments,
// scans the sums and scans every segment from its base, one workgroup per segment.
static void launch_scan(vhx_ctx *c, const uint32_t *counts, uint32_t nchunks_host, const uint32_t *n_in,
                        uint32_t per_chunk, uint32_t *offsets, uint32_t *total, uint64_t max_chunks) {
    const uint64_t nseg = (max_chunks + SCAN_SEG - 1) / SCAN_SEG;
    if (nseg <= c->scan_multi || c->scan_multi == 0 || !c->scan_part.ptr || c->scan_part.bytes < nseg * 8) {
        k_scan_counts<<<1, SCAN_THREADS, 0, c->stream>>>(counts, nchunks_host, n_in, per_chunk, c->tw, offsets, total);
        return;
    }
    uint32_t *sums = (uint32_t *)c->scan_part.ptr, *base = sums + nseg;
    k_scan_sums<<<(unsigned)nseg, SCAN_THREADS, 0, c->stream>>>(counts, nchunks_host, n_in, per_chunk, c->tw, sums);
    k_scan_counts<<<1, SCAN_THREADS, 0, c->stream>>>(sums, (uint32_t)nseg, nullptr, 1, c->tw, base, total);
    k_scan_counts<<<(unsigned)nseg, SCAN_THREADS, 0, c->stream>>>(counts, nchunks_host, n_in, per_chunk, c->tw,
                                                                   offsets, nullptr, base);
}

// Chunk lists -> queue `out` with its length at *total: pass-0 style (nchunks_host workgroup chunks of stride 256) or
// queue-pass style (chunks of per_chunk rays, their number derived from the device-side input length n_in).
static int compact_chunks(vhx_ctx *c, uint32_t nchunks_host, const uint32_t *n_in, uint32_t per_chunk,
                          uint32_t stride, uint32_t *out, uint32_t *total, uint64_t max_chunks, bool move_state = false) {
    const uint32_t *counts = (const uint32_t *)c->counts.ptr;
    uint32_t *offsets = (uint32_t *)c->offsets.ptr;
    // adaptive rays per chunk (pass_rpw, per_chunk 0; max_chunks is then the ray count): ceil(n / ceil(n / tw)) <= tw
    // chunks, or ceil(n / 64) once a chunk holds 64 rays
    const uint64_t scan_max = n_in && per_chunk == 0u
                                  ? std::min<uint64_t>(max_chunks, std::max<uint64_t>(c->tw, (max_chunks + 63) / 64))
                                  : max_chunks;
    launch_scan(c, counts, nchunks_host, n_in, per_chunk, offsets, total, scan_max);
    const uint64_t want = (max_chunks + 3) / 4;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, c->queue_blocks));
    k_gather_chunks<<<grid, 256, 0, c->stream>>>((const uint32_t *)c->tmp.ptr, stride, counts, offsets,
                                                 nchunks_host, n_in, per_chunk, c->tw, out,
                                                 move_state ? (const uint4 *)c->state.ptr : nullptr,
                                                 move_state ? (uint4 *)c->stateq.ptr : nullptr);
    VHX_HIP(c, hipGetLastError());
    debug_passes(c, "compacted");
    return VHX_OK;
}

// k_sort_segments over the queue of pass p (its length at *n_dev, at most nmax entries) when the schedule sorts and the
// rays of that pass resume from saved state (the node is read there)
static int sort_segments(vhx_ctx *c, uint32_t p, uint32_t npass, uint32_t *queue, const uint32_t *n_dev, uint64_t nmax) {
    const PassQ q = pass_q(c, p, npass);
    if (!c->qsort || !q.resume || !q.state || p >= 32u || !((c->qsort_passes >> p) & 1u)) return VHX_OK;
    const uint64_t segs = (nmax + c->qsort - 1) / c->qsort;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(segs, c->qsort_blocks));
    k_sort_segments<<<grid, QSORT_THREADS, 0, c->stream>>>(queue, n_dev, (const uint32_t *)q.state, c->qsort);
    VHX_HIP(c, hipGetLastError());
    debug_passes(c, "sorted segments");
    return VHX_OK;
}

// The FlagOrder of code `qorder` for a W x H framebuffer frame (W = 0 or qorder = 0: output-index order) and the
// number of positions its compaction scans (npos: in / out)
static FlagOrder flag_order(uint32_t qorder, uint32_t W, uint32_t H, uint64_t &npos, uint32_t frames = 1) {
    FlagOrder ord{};
    if (!qorder || !W || !H) return ord;
    const uint32_t tsl = qorder & 15u, ts = 1u << tsl;
    ord = FlagOrder{W, H, (W + ts - 1u) / ts, (H + ts - 1u) / ts, tsl, 0u, (qorder & 64u) ? 2u : (qorder & 32u) ? 1u : 0u,
                    0u, 0u};
    if (qorder & 16u)  // Morton order over the smallest 2^m x 2^m grid of tiles covering the frame
        while ((1u << ord.mdim) < std::max(ord.tx, ord.ty)) ++ord.mdim;
    const uint64_t np = (ord.mdim ? 1ull << (2u * ord.mdim) : (uint64_t)ord.tx * ord.ty) << (2u * tsl);
    // the chunk counts are sized for ceil(pixels / 256) chunks, the compaction needs ceil(npos / 1024): a tile far
    // larger than the frame keeps output-index order
    if (np > 4ull * W * H) return FlagOrder{};
    npos = np * frames;
    if (frames > 1) {
        ord.fpos = np;
        ord.fpix = (uint64_t)W * H;
    }
    return ord;
}

// The ListOrder of code `qorder` for a W x H framebuffer frame, when pass 0 can list its rays in that order itself:
// tiles row-major (no Morton over the tiles), Morton inside, at least 16 pixels per side (the default, 38); nblocks =
// the workgroups of pass 0 over whole tiles. Else false (pass 0 writes flags, flag_order compacts them).
static bool list_order(uint32_t qorder, uint32_t W, uint32_t H, ListOrder &lo, uint64_t &nblocks) {
    const uint32_t tsl = qorder & 15u;
    if (!qorder || !W || !H || (qorder & (16u | 64u)) || !(qorder & 32u) || tsl < 4u) return false;
    const uint32_t ts = 1u << tsl, ty = (H + ts - 1u) / ts;
    lo = ListOrder{(W + ts - 1u) / ts, tsl - 4u};
    nblocks = ((uint64_t)lo.tx * ty) << (2u * lo.tbl);
    // flag_order keeps output-index order for tiles far larger than the frame
    return nblocks * 256u <= 4ull * W * H;
}

// Pass 0's workgroups over whole tiles of the list order: the buffers of its per-workgroup lists
static int ensure_lists(vhx_ctx *c, uint64_t nblocks) {
    int rc = ensure(c, c->tmp, nblocks * 256 * 4);
    // the queue-state mode saves pass 0's abandoned rays at their list slots (every slot of whole tiles)
    if (!rc && c->resume && c->qstate) rc = ensure(c, c->state, nblocks * 256 * 64);
    if (!rc) rc = ensure(c, c->counts, nblocks * 4 * 4);
    if (!rc) rc = ensure(c, c->offsets, nblocks * 4 * 4);
    if (!rc) rc = ensure(c, c->scan_part, ((nblocks * 4 + SCAN_SEG - 1) / SCAN_SEG) * 8);
    return rc;
}

// The QueueArgs slot of a frame (camera, ray source, outputs) on c's stream. They rarely change between frames: the
// device copy is rewritten only when they do.
static int put_qargs(vhx_ctx *c, const CamD &cam, const RaySrc &src, const OutD &o, QueueArgs *&qa) {
    const uint32_t slot = src.kind == 3u || src.kind == 5u ? 1u : 0u;  // a shadow frame alternates with its primary
    qa = (QueueArgs *)c->qargs.ptr + slot;
    QueueArgs a;
    std::memset(&a, 0, sizeof(a));  // padding included, for the comparison
    a.cam = cam;
    a.src = src;
    a.out = o;
    const uint8_t *ab = (const uint8_t *)&a;
    if (c->qargs_host_ptr[slot] != c->qargs.ptr || c->qargs_host[slot].size() != sizeof(a) ||
        std::memcmp(c->qargs_host[slot].data(), ab, sizeof(a)) != 0) {
        k_put_queue_args<<<1, 64, 0, c->stream>>>(a, qa);
        VHX_HIP(c, hipGetLastError());
        c->qargs_host[slot].assign(ab, ab + sizeof(a));
        c->qargs_host_ptr[slot] = c->qargs.ptr;
    }
    return VHX_OK;
}

// How a grid pass 0 hands its abandoned rays to the queue passes (launch_queue_passes)
enum { P0_LISTS = 0, P0_FLAGS = 1, P0_ORDERED = 2 };

// Flags -> queue: the set flags of `npos` positions in the order `ord` (HITS false: pass 0's flag byte per output
// index; HITS true: a hit value != VHX_EMPTY, the hit pixels a shadow pass starts from) listed at `out`, their number at
// *total. The count kernel also zeroes the queue passes' work counters and, when given, the nclear entries of `clear`.
template <bool HITS>
static int compact_flags(vhx_ctx *c, const void *src, uint64_t npos, const FlagOrder &ord, uint32_t *total,
                         uint32_t *out, uint32_t *clear = nullptr, uint64_t nclear = 0) {
    const unsigned nb = (unsigned)((npos + 1023) / 1024);
    // a shadow batch in a tile order scans more positions than prepare_passes sized the chunk counts for
    if ((uint64_t)nb * 4 > c->counts.bytes || (uint64_t)nb * 4 > c->offsets.bytes) {
        const int rc = ensure_lists(c, nb);
        if (rc) return rc;
    }
    uint32_t *counts = (uint32_t *)c->counts.ptr, *offsets = (uint32_t *)c->offsets.ptr;
    k_count_flags<HITS><<<nb, 256, 0, c->stream>>>(src, npos, counts, (uint32_t *)c->qctl.ptr + 16, clear, ord, nclear);
    launch_scan(c, counts, nb, nullptr, 1, offsets, total, nb);
    k_emit_flags<HITS><<<nb, 256, 0, c->stream>>>(src, npos, offsets, out, ord);
    VHX_HIP(c, hipGetLastError());
    debug_passes(c, "compacted flags");
    return VHX_OK;
}

// compact_flags<true> over the entries of `value` that the primary trace of geometry `own` wrote: its hits listed at
// `out` in output-index order, their number at *total, and `clear` zeroed at the owned entries only
static int compact_owned_hits(vhx_ctx *c, const uint32_t *value, uint64_t n, const OwnGeom &own, uint32_t *total,
                              uint32_t *out, uint32_t *clear) {
    const unsigned nb = (unsigned)((n + 1023) / 1024);
    if ((uint64_t)nb * 4 > c->counts.bytes || (uint64_t)nb * 4 > c->offsets.bytes) {
        const int rc = ensure_lists(c, nb);
        if (rc) return rc;
    }
    uint32_t *counts = (uint32_t *)c->counts.ptr, *offsets = (uint32_t *)c->offsets.ptr;
    k_count_owned_hits<<<nb, 256, 0, c->stream>>>(value, n, counts, (uint32_t *)c->qctl.ptr + 16, clear, own);
    launch_scan(c, counts, nb, nullptr, 1, offsets, total, nb);
    k_emit_owned_hits<<<nb, 256, 0, c->stream>>>(value, n, offsets, out, own);
    VHX_HIP(c, hipGetLastError());
    debug_passes(c, "compacted owned hits");
    return VHX_OK;
}

// A trace's queue passes (launch_queue_passes): what they trace, and how pass 0 handed over its abandoned rays
struct QueueRun {
    CamD cam{};
    RaySrc src{};
    OutD out{};
    uint32_t first = 1;  // the first queue pass: 1 after a grid pass 0, 0 where pass 0 is itself a queue pass
    uint32_t npass = 1;
    uint64_t nout = 0;      // rays of the trace
    uint64_t nblocks0 = 0;  // workgroups of the grid pass 0
    int pass0 = P0_LISTS;
    uint32_t order_w = 0, order_h = 0;  // P0_FLAGS: the frame in whose queue order (c->qorder) the flags are compacted
    uint32_t frames = 1;                // frames of a batch
    bool qm = false;                    // queue-state mode (queue_state_mode)
    // P0_ORDERED behind a worklist: the extent of pass 0's lists in rays, 256 per tree block, read on the device (the
    // compaction covers what was traced; null: all of nblocks0)
    const uint32_t *n0 = nullptr;
};

// Queue passes first..npass-1: pass p re-traces the queue of pass p-1 (pass 0's queue, for first == 0, is the list
// in queue[1] with its length in qctl[7]); what exceeds its budget is listed per chunk and compacted into the next
// pass's queue. For first == 1, pass 0 (a grid kernel of nblocks0 workgroups) has just run and is compacted first:
// its per-workgroup lists (P0_LISTS, in workgroup order; P0_ORDERED, already in the queue order, ListOrder), or its
// per-ray flags in the queue order (P0_FLAGS).
template <bool COUNT, int BD, bool MIP = false, bool FUSE = false>
static int launch_queue_passes(vhx_ctx *c, const DevTree &t, const QueueRun &r) {
    const uint32_t npass = r.npass;
    uint32_t *ctl = (uint32_t *)c->qctl.ptr, *queue0 = (uint32_t *)c->queue[0].ptr;
    int rc = VHX_OK;
    if (r.first > 0 && npass > 1) {
        if (r.pass0 == P0_FLAGS) {  // primary frames: per-ray flags compacted in output-index (frame) order
            // tile order (c->qorder, framebuffer layout only): positions over the frame's tiles
            uint64_t npos = r.nout;
            const FlagOrder ord = flag_order(c->qorder, r.order_w, r.order_h, npos, r.frames);
            if ((rc = compact_flags<false>(c, c->flags.ptr, npos, ord, ctl, queue0))) return rc;
            if ((rc = sort_segments(c, 1, npass, queue0, ctl, r.nout))) return rc;
        } else if (r.pass0 == P0_ORDERED) {  // per-wave lists (wave_append): 4 chunks of 64 per workgroup
            rc = compact_chunks(c, (uint32_t)(r.nblocks0 * 4), r.n0, 64, 64, queue0, ctl, r.nblocks0 * 4, r.qm);
            if (!rc) rc = sort_segments(c, 1, npass, queue0, ctl, r.nout);
        } else {
            rc = compact_chunks(c, (uint32_t)r.nblocks0, nullptr, 256, 256, queue0, ctl, r.nblocks0);
        }
    }
    QueueArgs *qa = nullptr;
    if (r.first < npass && (rc = put_qargs(c, r.cam, r.src, r.out, qa))) return rc;
    for (uint32_t p = r.first; p < npass && !rc; ++p) {
        const uint32_t *in = (const uint32_t *)c->queue[(p - 1) & 1u].ptr;  // p = 0: queue[1]
        const uint32_t *in_n = p > 0 ? ctl + (p - 1) : ctl + 7;
        const PassQ q = pass_q(c, p, npass, r.qm);
        // a first pass over fresh rays (the shadow path) is throughput-bound like a grid launch: more waves
        uint32_t qwaves = p == 0 ? c->queue_waves0
                          : (p + 1 < npass && c->queue_waves_mid ? c->queue_waves_mid : c->queue_waves);
        // a batch of frames: the waves the same frames would bring as frames in flight (one frame's queue waves each),
        // up to the queue kernel's residency (5 waves per SIMD): its queue passes are memory-latency bound and need
        // the waves in flight
        if (r.frames > 1 && p > 0) qwaves = (uint32_t)std::min<uint64_t>((uint64_t)qwaves * r.frames, 20ull * c->cus);
        const unsigned qgrid = (qwaves * 64u + c->qblock - 1) / c->qblock;
        uint32_t *grab = ctl + 16u + QCTL_PASS_WORDS * p;
        if constexpr (!FUSE && !MIP) {  // (the queue-state mode excludes fused shadows; MIP frames never list pass 0)
            if (q.qmode)
                k_trace_queue<COUNT, BD, MIP, FUSE, true><<<qgrid, c->qblock, 0, c->stream>>>(t, qa, in, in_n, grab, q);
            else
                k_trace_queue<COUNT, BD, MIP, FUSE><<<qgrid, c->qblock, 0, c->stream>>>(t, qa, in, in_n, grab, q);
        } else {
            k_trace_queue<COUNT, BD, MIP, FUSE><<<qgrid, c->qblock, 0, c->stream>>>(t, qa, in, in_n, grab, q);
        }
        debug_passes(c, "queue pass");
        if (p + 1 < npass) {
            rc = compact_chunks(c, 0, in_n, q.rpw, q.rpw, (uint32_t *)c->queue[p & 1u].ptr, ctl + p,
                                q.rpw ? (r.nout + q.rpw - 1) / q.rpw : r.nout, r.qm);
            if (!rc) rc = sort_segments(c, p + 1, npass, (uint32_t *)c->queue[p & 1u].ptr, ctl + p, r.nout);
        }
    }
    return rc;
}

// The kernel variants that exist besides brick_dim: MIP stand-ins, byte counting, fused shadows, the depth prepass's
// start (FAST, pass 0 of a primary frame only), or none of them -- never two at once, which the entry points refuse.
// f(BdTag, VarTag) is instantiated for these five tags only, so no other combination of a kernel is built.
template <bool C, bool M, bool F, bool S>
struct VarTag {
    static constexpr bool COUNT = C, MIP = M, FUSE = F, FAST = S;
};
template <class Fn>
static bool dispatch_variant(uint32_t bd, bool mip, bool count, bool fuse, bool fast, Fn &&f) {
    return dispatch_bd(bd, [&](auto b) {
        if (mip) f(b, VarTag<false, true, false, false>{});
        else if (count) f(b, VarTag<true, false, false, false>{});
        else if (fuse) f(b, VarTag<false, false, true, false>{});
        else if (fast) f(b, VarTag<false, false, false, true>{});
        else f(b, VarTag<false, false, false, false>{});
    });
}

// ------------------------------------------------------------------------------------------ trace entry points
// What every trace entry point does around its launches. The constructor selects the device and the context's stream
// and opens the trace's scope in the tree-write ordering: the trace follows the tree's last write (an update through the
// owner, on its stream). nested: the depth prepass's inner frame, which runs inside its outer frame's scope and time.
// rc != 0 after construction: the entry point returns it.
struct TraceCall {
    vhx_ctx *c;
    const bool nested;
    int rc;
    TraceScope scope;
    explicit TraceCall(vhx_ctx *ctx, bool nested_ = false)
        : c(ctx), nested(nested_), rc(use_stream(ctx)), scope(ctx, nested_ || rc != VHX_OK) {
        if (!rc) rc = scope.rc;
    }
    static int use_stream(vhx_ctx *c) {
        VHX_HIP(c, hipSetDevice(c->device));
        VHX_STREAM(c);
        return VHX_OK;
    }
    // the tree as the kernels read it, its child records rebuilt first where an update left them stale
    int tree(DevTree &t) {
        const int r = refresh_child_rec(c);
        if (!r) t = dev_tree(c);
        return r;
    }
    // the start of the time vhx_sync reports; a shadow trace that completes a frame (keep_ev0) keeps the start of the
    // frame's primary trace
    int start() {
        if (!nested && !c->keep_ev0) VHX_HIP(c, hipEventRecord(c->ev0, c->stream));
        return VHX_OK;
    }
    // after the last launch (qrc: what the launches returned): the end of the timed region and of the scope -- a later
    // write of the tree waits for this trace
    int end(int qrc) {
        if (qrc) return qrc;
        VHX_HIP(c, hipGetLastError());
        if (nested) return VHX_OK;  // the outer call records the end
        VHX_HIP(c, hipEventRecord(c->ev1, c->stream));
        c->timed = true;
        return scope.end();
    }
};

// Whether a written range meets a read range (1) or another written range (2), else 0; null and empty ranges meet
// nothing. With both kinds present, the kind of the first written range, in the caller's order, that meets anything.
struct MemRange {
    const void *p;
    uint64_t bytes;
};
static int ranges_meet(const std::vector<MemRange> &written, const std::vector<MemRange> &read) {
    struct E {
        const char *p, *end;
        bool w;
    };
    std::vector<E> es;
    for (const MemRange &r : written)
        if (r.p && r.bytes) es.push_back({(const char *)r.p, (const char *)r.p + r.bytes, true});
    for (const MemRange &r : read)
        if (r.p && r.bytes) es.push_back({(const char *)r.p, (const char *)r.p + r.bytes, false});
    // in address order, a range that starts before the end of an earlier one meets it (two read ranges may)
    std::sort(es.begin(), es.end(), [](const E &a, const E &b) { return a.p < b.p; });
    const char *wend = nullptr, *rend = nullptr;
    bool any = false;
    for (const E &e : es) {
        if (e.p < wend || (e.w && e.p < rend)) any = true;
        const char *&end = e.w ? wend : rend;
        end = std::max(end, e.end);
    }
    if (!any) return 0;
    auto meet = [](const MemRange &a, const MemRange &b) {
        return a.p && b.p && a.bytes && b.bytes && (const char *)a.p < (const char *)b.p + b.bytes &&
               (const char *)b.p < (const char *)a.p + a.bytes;
    };
    for (size_t i = 0; i < written.size(); ++i) {
        for (const MemRange &r : read)
            if (meet(written[i], r)) return 1;
        for (size_t j = i + 1; j < written.size(); ++j)
            if (meet(written[i], written[j])) return 2;
    }
    return 0;
}

// Staged batch arguments (a batch's cameras and outputs, a shadow batch's frame records): the next slot of a pinned
// staging ring, sized for `bytes`, and the device buffer it is copied to. The host waits only if that slot's previous
// copy (VHX_STAGE_SLOTS batches ago on this context) has not run yet. The caller fills P->ptr, then stage_commit.
static int stage_acquire(vhx_ctx *c, vhx_ctx::Pinned *ring, uint32_t &next, DevBuf &dev, uint64_t bytes,
                         vhx_ctx::Pinned *&out) {
    vhx_ctx::Pinned &P = ring[next];
    next = (next + 1) % std::max<uint32_t>(1u, std::min(c->stage_slots, vhx_ctx::VHX_STAGE_SLOTS));
    if (P.used) VHX_HIP(c, hipEventSynchronize(P.done));
    if (P.bytes < bytes) {
        if (P.ptr) VHX_HIP(c, hipHostFree(P.ptr));
        P.ptr = nullptr;
        P.bytes = 0;
        VHX_HIP(c, hipHostMalloc(&P.ptr, bytes, hipHostMallocDefault));
        P.bytes = bytes;
    }
    if (!P.done) VHX_HIP(c, hipEventCreateWithFlags(&P.done, hipEventDisableTiming));
    out = &P;
    // the device copy is read by this context's earlier batches: a stream change waits for them
    if (c->use_recorded && c->use_stream != c->stream) VHX_HIP(c, hipStreamWaitEvent(c->stream, c->use_ev, 0));
    return ensure(c, dev, bytes);
}
// one copy to the device ahead of the launches on the context's stream (back-to-back batches on one context do not
// wait on the host until the ring wraps onto a copy that has not run)
static int stage_commit(vhx_ctx *c, vhx_ctx::Pinned &P, const DevBuf &dev, uint64_t bytes) {
    VHX_HIP(c, hipMemcpyAsync(dev.ptr, P.ptr, bytes, hipMemcpyHostToDevice, c->stream));
    VHX_HIP(c, hipEventRecord(P.done, c->stream));
    P.used = true;
    return VHX_OK;
}

// How pass 0 of a primary frame, or of a batch of them, hands its abandoned rays to the queue passes
struct Pass0Plan {
    bool listed = false;  // pass 0 lists them per wave, in the queue order (lo); else it writes a flag per ray
    ListOrder lo{};
    uint64_t nbf = 0;     // pass-0 workgroups per frame: over whole tiles of the list order when listed by it
    bool qm = false;      // the trace runs in the queue-state mode
    bool fuse = false;    // its shadow rays are fused into the ladder
    int p0() const { return listed ? P0_ORDERED : P0_FLAGS; }
};
// fb_lists: whole W x H framebuffer frames in 16x16 blocks, which pass 0 can list in the default queue order itself
// (ListOrder). tile_lists: tile sets, listed in their own block order (ListOrder::tl) -- no flag per entry, no
// compaction over every entry, and the queue-state mode. nbf: a frame's pass-0 workgroups; shadows: a shadow light is
// in force. Lists of more than 2^31 chunks: refused (refuse_oversize) or replaced by flags.
static int plan_pass0(vhx_ctx *c, uint32_t npass, bool fb_lists, bool tile_lists, uint32_t W, uint32_t H, uint64_t nbf,
                      uint32_t frames, bool shadows, bool refuse_oversize, Pass0Plan &p) {
    const bool lists = c->p0lists && npass > 1;
    const auto unlisted = [&] {
        p = Pass0Plan{};
        p.nbf = nbf;
    };
    unlisted();
    if (lists && fb_lists && list_order(c->qorder, W, H, p.lo, p.nbf)) p.listed = true;
    else unlisted();
    if (!p.listed && lists && tile_lists && c->tile_lists) {
        p.listed = true;
        p.lo.tl = 1;
    }
    const bool oversize = p.nbf * frames * 4 > 0x7FFFFFFFull;  // four chunk counts per workgroup
    if (p.listed && oversize && !refuse_oversize) unlisted();
    int rc = VHX_OK;
    if (p.listed && (rc = ensure_lists(c, p.nbf * frames))) return rc;
    if (p.listed && oversize) return fail(c, VHX_E_INVALID_ARG, "frame too large");
    p.qm = queue_state_mode(c, p.listed, false, npass);
    // shadows fuse into the ladder where pass 0 lists its rays (the list entries carry the shadow tag); a single pass
    // or the lone frame's flag compaction traces them after the primary rays instead
    p.fuse = shadows && p.listed && npass > 1;
    return VHX_OK;
}

// Pass 0's PassQ. A pass that lists its rays in the queue order zeroes the queue passes' counters itself (no flag
// compaction follows it to do so); one compacted from flags writes them; a ray batch's block lists (P0_LISTS) need neither.
static PassQ pass0_q(const vhx_ctx *c, uint32_t npass, int p0, bool qm = false) {
    PassQ q = pass_q(c, 0, npass, qm);
    if (p0 == P0_ORDERED)
        q.zero = (uint32_t *)c->qctl.ptr + 16;
    else if (p0 == P0_FLAGS && npass > 1)
        q.flags = (uint8_t *)c->flags.ptr;
    return q;
}

// The depth prepass of a frame (vhx_set_depth_prepass): its half-resolution camera ...
static vhx_camera half_camera(const vhx_camera *cam) {
    vhx_camera hc = *cam;
    hc.width = (cam->width + 1) / 2;
    hc.height = (cam->height + 1) / 2;
    if (cam->ray_model == VHX_RAY_GLASS) {
        // texel (X, Y) looks through the centre of full pixels 2X..2X+1, 2Y..2Y+1 (y counted upward in the glass)
        const float ox = 0.5f * cam->pixel_width, oy = ((float)cam->height + 0.5f - 2.0f * (float)hc.height) * cam->pixel_height;
        for (int k = 0; k < 3; ++k)
            hc.glass_bottom_left[k] = cam->glass_bottom_left[k] + cam->glass_right[k] * ox + cam->glass_up[k] * oy;
        hc.pixel_width = 2.0f * cam->pixel_width;
        hc.pixel_height = 2.0f * cam->pixel_height;
    }
    return hc;
}
// ... and its half-resolution depth frame, traced by a nested call on the same stream; the full frame starts from it
static int trace_prepass(vhx_ctx *c, const vhx_camera *cam, FastD &fd) {
    const vhx_camera hc = half_camera(cam);
    int rc = ensure(c, c->prepass_depth, (uint64_t)hc.width * hc.height * 4);
    if (rc) return rc;
    vhx_hits dh{};
    dh.depth = (float *)c->prepass_depth.ptr;
    c->in_prepass = true;
    rc = vhx_trace_primary(c, &hc, 0, 0, 1, VHX_LAYOUT_FRAMEBUFFER, &dh, 1);
    c->in_prepass = false;
    if (rc) return rc;
    fd = FastD{(const float *)c->prepass_depth.ptr, hc.width, hc.height, c->prepass_margin};
    return VHX_OK;
}

// Early tail (vhx_ctx::tail_*), set-up: the lists, the mask and the second stream; the list this frame records
// (c->tail_rec) is cleared; `use`: this context's last lone frame of the same size recorded a list, whose pixels the
// early tail traces on the second stream (forked here) while pass 0 skips them (tail_mask)
static int tail_begin(vhx_ctx *c, uint32_t W, uint32_t H, uint64_t nout, bool &use) {
    const uint64_t lbytes = (64ull + c->tail_cap) * 4ull, mbytes = ((nout + 31) / 32) * 4;
    int rc;
    if ((rc = ensure(c, c->tail_list[0], lbytes)) || (rc = ensure(c, c->tail_list[1], lbytes)) ||
        (rc = ensure(c, c->tail_mask, mbytes)))
        return rc;
    if (!c->tail_stream) {
        int least = 0, greatest = 0;
        VHX_HIP(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        VHX_HIP(c, hipStreamCreateWithPriority(&c->tail_stream, hipStreamNonBlocking, greatest));
        VHX_HIP(c, hipEventCreateWithFlags(&c->tail_fork, hipEventDisableTiming));
        VHX_HIP(c, hipEventCreateWithFlags(&c->tail_join, hipEventDisableTiming));
    }
    uint32_t *next = (uint32_t *)c->tail_list[c->tail_cur ^ 1u].ptr;
    VHX_HIP(c, hipMemsetAsync(next, 0, 4, c->stream));
    use = c->tail_valid && c->tail_w == W && c->tail_h == H;
    if (use) {
        VHX_HIP(c, hipMemsetAsync(c->tail_mask.ptr, 0, mbytes, c->stream));
        k_tail_mask<<<16, 256, 0, c->stream>>>((const uint32_t *)c->tail_list[c->tail_cur].ptr, c->tail_cap,
                                               (uint32_t)nout, (uint32_t *)c->tail_mask.ptr);
        VHX_HIP(c, hipEventRecord(c->tail_fork, c->stream));
        VHX_HIP(c, hipStreamWaitEvent(c->tail_stream, c->tail_fork, 0));
    }
    c->tail_rec = next;
    return VHX_OK;
}
// ... and end: the frame ends with its early tail (joined before ev1 and the trace's use event); its record is the next
// frame's list (the list it traced stays valid: an error later still leaves two well-formed lists)
static int tail_end(vhx_ctx *c, uint32_t W, uint32_t H, bool use) {
    if (use) {
        VHX_HIP(c, hipEventRecord(c->tail_join, c->tail_stream));
        VHX_HIP(c, hipStreamWaitEvent(c->stream, c->tail_join, 0));
    }
    c->tail_cur ^= 1u;
    c->tail_valid = true;
    c->tail_w = W;
    c->tail_h = H;
    return VHX_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int vhx_set_pass_budgets(vhx_ctx *c, const uint32_t *budgets, uint32_t n) {
    if (!c || n > VHX_MAX_BUDGETS || (n && !budgets)) return VHX_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i)
        if (budgets[i] == 0 || budgets[i] >= VHX_MAX_ITERS || (i && budgets[i] <= budgets[i - 1]))
            return fail(c, VHX_E_INVALID_ARG, "pass budgets must be increasing, > 0 and < 2^22");
    for (uint32_t i = 0; i < VHX_MAX_BUDGETS; ++i) c->budgets[i] = i < n ? budgets[i] : 0u;
    c->npass = n + 1;
    if (c->adaptive) {  // leaving the adaptive choice: the rest of the schedule is the busy one's
        std::memcpy(c->sparse, c->sched_busy.sparse, sizeof(c->sparse));
        c->queue_waves = c->sched_busy.queue_waves_per_cu * c->cus;
        c->queue_waves0 = c->queue_waves0_force ? c->queue_waves0_force : c->sched_busy.queue_waves0_per_cu * c->cus;
        c->qorder = c->sched_busy.qorder;
        c->adaptive = false;
    }
    c->last_sched = -1;
    return VHX_OK;
}

static int trace_shadows_of(vhx_ctx *c, const float light[3], uint64_t n, const uint32_t *value, const float *impact,
                            const float *normal, uint32_t *shadowed, uint32_t *rgba, uint32_t *bytes,
                            const OwnGeom *own);

static CamD cam_of(const vhx_camera *cam) {
    CamD d;
    d.model = cam->ray_model;
    d.width = cam->width;
    d.height = cam->height;
    d.ox = cam->origin[0];
    d.oy = cam->origin[1];
    d.oz = cam->origin[2];
    d.blx = cam->glass_bottom_left[0];
    d.bly = cam->glass_bottom_left[1];
    d.blz = cam->glass_bottom_left[2];
    d.rx = cam->glass_right[0];
    d.ry = cam->glass_right[1];
    d.rz = cam->glass_right[2];
    d.ux = cam->glass_up[0];
    d.uy = cam->glass_up[1];
    d.uz = cam->glass_up[2];
    d.pw = cam->pixel_width;
    d.ph = cam->pixel_height;
    std::memcpy(d.m, cam->inv_view_proj, sizeof(d.m));
    return d;
}

int vhx_trace_primary(vhx_ctx *c, const vhx_camera *cam, uint32_t T, uint32_t tile_start, uint32_t tile_stride,
                      uint32_t layout, const vhx_hits *out, int on_device) {
    if (!c || !cam || !out) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_trace_primary before vhx_upload_tree");
    if (cam->width == 0 || cam->height == 0 || cam->ray_model > VHX_RAY_GLASS || layout > VHX_LAYOUT_TILES)
        return fail(c, VHX_E_INVALID_ARG, "vhx_trace_primary: bad camera or layout");
    if (T == 0) {
        if (layout != VHX_LAYOUT_FRAMEBUFFER) return fail(c, VHX_E_INVALID_ARG, "tile_size 0 needs the framebuffer layout");
        T = 16;
        tile_start = 0;
        tile_stride = 1;
    }
    if (tile_stride == 0) return fail(c, VHX_E_INVALID_ARG, "tile_stride 0");
    const uint32_t tiles_x = (cam->width + T - 1) / T, tiles_y = (cam->height + T - 1) / T;
    const uint32_t ntiles = tiles_x * tiles_y;
    if (tile_start >= ntiles) return VHX_OK;
    const uint32_t my_tiles = (ntiles - tile_start + tile_stride - 1) / tile_stride;
    const uint32_t bpx = (T + 15) / 16, bpt = bpx * bpx;
    const uint64_t nblocks = (uint64_t)my_tiles * bpt;
    if (nblocks > 0x7FFFFFFFull) return fail(c, VHX_E_INVALID_ARG, "frame too large");
    const bool fb = layout == VHX_LAYOUT_FRAMEBUFFER;
    const bool whole_fb = fb && tile_start == 0 && tile_stride == 1;  // the whole frame in the framebuffer layout ...
    const bool whole_fb16 = whole_fb && T == 16;                      // ... a 16x16 block per tile
    const uint64_t nout = fb ? (uint64_t)cam->width * cam->height : (uint64_t)my_tiles * T * T;
    TraceCall tr(c, c->in_prepass);
    int rc = tr.rc;
    if (rc) return rc;
    HostOut ho;
    if ((rc = map_out(c, out, nout, on_device, ho, layout == VHX_LAYOUT_TILES))) return rc;
    DevTree t;
    if ((rc = tr.tree(t))) return rc;
    if (t.mips && (out->bytes || (c->prepass && !c->in_prepass)))
        return fail(c, VHX_E_INVALID_ARG, "vhx_trace_primary: byte counting and the depth prepass are not available "
                                          "with node MIPs (vhx_set_node_mips)");
    // fused hard shadows (vhx_set_shadow_light): the shadow rays start from the stored hit records
    const bool shadows = c->shadow_on && !c->in_prepass;
    if (shadows && (!out->value || !out->impact || !out->normal || !out->shadowed || out->bytes || t.mips || c->prepass))
        return fail(c, VHX_E_INVALID_ARG, "vhx_trace_primary with a shadow light: value, impact, normal and shadowed "
                                          "outputs needed; no byte counting, node MIPs or depth prepass");
    // the shadow rays read the hit records while shadowed and rgba are written, fused or after the primary rays:
    // refused here, before any launch, whichever schedule the trace would take (host outputs are staged apart)
    if (shadows && on_device &&
        ranges_meet({{out->shadowed, nout * 4}, {out->rgba, nout * 4}},
                    {{out->value, nout * 4}, {out->impact, nout * 12}, {out->normal, nout * 12}}))
        return fail(c, VHX_E_INVALID_ARG, "vhx_trace_primary with a shadow light: shadowed and rgba must not overlap "
                                          "value, impact, normal or each other");
    uint32_t npass = 1;
    if ((rc = prepare_passes(c, nout, nblocks, npass))) return rc;
    // pass 0's list buffers for either schedule's queue order: a context's first frames often run alone (the idle
    // schedule), and growing the buffers at its first frame among others would hipFree -- a device-wide
    // synchronisation that drains every frame in flight (measured: 0.61 against 0.54 ms per bench frame)
    if (c->p0lists && whole_fb16) {
        const uint32_t orders[2] = {c->sched_busy.qorder, c->qorder};
        for (uint32_t o : orders) {
            ListOrder l2{};
            uint64_t nb2 = 0;
            if (list_order(o, cam->width, cam->height, l2, nb2) && (rc = ensure_lists(c, nb2))) return rc;
        }
    }
    if ((rc = tr.start())) return rc;
    // depth-prepass mode (vhx_set_depth_prepass): a whole framebuffer frame without byte counting first traces the
    // half-resolution depth frame, then starts from it
    const bool fast = c->prepass && !c->in_prepass && whole_fb && !out->bytes;
    FastD fd{};
    if (fast && (rc = trace_prepass(c, cam, fd))) return rc;
    // no reset_passes: the flag compaction after pass 0 zeroes the queue passes' counters.
    // A rank-sharded framebuffer (tile_start > 0 or tile_stride > 1) leaves the flags of other ranks' pixels unwritten,
    // while the compaction scans every pixel: they are cleared first (stale flags would queue foreign pixels)
    if (npass > 1 && fb && !whole_fb) VHX_HIP(c, hipMemsetAsync(c->flags.ptr, 0, nout, c->stream));

    // a whole framebuffer frame in the default queue order lists its rays in that order itself; a tile set (the rank's
    // share of a multi-GPU frame) lists them under the frames-in-flight schedule (a queue order is in force)
    Pass0Plan p0;
    if ((rc = plan_pass0(c, npass, whole_fb16, layout == VHX_LAYOUT_TILES && c->qorder != 0, cam->width, cam->height,
                         nblocks, 1, shadows, true, p0)))
        return rc;
    QueueRun run;
    run.cam = cam_of(cam);
    run.src.kind = fb ? 0u : 1u;
    run.src.T = T;
    run.src.tiles_x = tiles_x;
    run.src.tile_start = tile_start;
    run.src.tile_stride = tile_stride;
    run.out = ho.dev;
    run.npass = npass;
    run.nout = nout;
    run.nblocks0 = p0.nbf;
    run.pass0 = p0.p0();
    // the queue order's frame (c->qorder): the framebuffer layout only. The tile layout's output index is already
    // tile-major with T-wide rows inside a tile (config 4 on one rank, 64x64 tiles: 2.019-2.025 ms per frame in that
    // order against 2.071-2.074 with the tiles re-ordered Morton inside, profiles/r03/qorder/mgpu1_*.log)
    run.order_w = fb ? cam->width : 0u;
    run.order_h = cam->height;
    run.qm = p0.qm;
    const bool count = ho.dev.bytes != nullptr;
    // early tail (vhx_ctx::tail_*): a lone frame (the idle schedule) of a whole framebuffer on the exact path records
    // its longest rays; with a list recorded by this context's last such frame of the same size, they start now
    const bool tail = c->tail_on && !fast && !count && !t.mips && !shadows && !p0.listed && npass > 1 &&
                      c->last_sched == 0 && whole_fb16 && c->tail_cap > 0;
    bool tail_use = false;
    if (tail && (rc = tail_begin(c, cam->width, cam->height, nout, tail_use))) return rc;
    PassQ q0 = pass0_q(c, npass, run.pass0, p0.qm);
    if (tail_use) q0.skip = (const uint32_t *)c->tail_mask.ptr;  // the early tail's kernel stores them
    const uint32_t tail_blocks = (c->tail_cap + c->tail_rpw * 4u - 1u) / (c->tail_rpw * 4u);
    int qrc = VHX_OK;
    const bool bd_ok = dispatch_variant(c->tree->desc.brick_dim, t.mips != nullptr, count, p0.fuse, fast, [&](auto bd_tag, auto v) {
        constexpr int BD = decltype(bd_tag)::value;
        using V = decltype(v);
        if (tail_use)  // the listed long rays first, on the second stream
            k_trace_tail<BD><<<tail_blocks, 256, 0, c->tail_stream>>>(
                t, run.cam, ho.dev, (const uint32_t *)c->tail_list[c->tail_cur].ptr, c->tail_rec, c->tail_cap,
                c->tail_min, c->tail_rpw, c->tail_prio);
        k_trace_primary<V::COUNT, BD, V::FAST, V::MIP, V::FUSE><<<(unsigned)p0.nbf, 256, 0, c->stream>>>(
            t, run.cam, ho.dev, T, tiles_x, tile_start, tile_stride, layout, bpx, bpt, q0, fd, p0.lo);
        qrc = launch_queue_passes<V::COUNT, BD, V::MIP, V::FUSE>(c, t, run);
    });
    c->tail_rec = nullptr;
    if (tail && (rc = tail_end(c, cam->width, cam->height, tail_use))) return rc;
    if (!bd_ok) return fail(c, VHX_E_INVALID_ARG, "unsupported brick_dim");
    if ((rc = tr.end(qrc)) || c->in_prepass) return rc;  // (the prepass's outer call copies its outputs)
    // a shadow trace of this frame's hit records lists them in the same tile order (vhx_trace_shadows)
    c->last_fb_w = fb ? cam->width : 0u;
    c->last_fb_h = fb ? cam->height : 0u;
    if (shadows && !p0.fuse) {
        // the frame's shadow rays after its primary rays (vhx_trace_shadows on the same stream); the frame's time then
        // spans both (ev0 of the primary trace, ev1 re-recorded by the shadow trace)
        // over the entries this trace wrote: a whole framebuffer frame owns them all; tile padding and, in a
        // rank-sharded framebuffer, the other ranks' pixels hold no record of this call and stay as they are
        const OwnGeom own{cam->width, cam->height, T, tiles_x, tile_start, tile_stride, fb ? 0u : 1u};
        c->keep_ev0 = true;
        rc = trace_shadows_of(c, c->shadow_light, nout, ho.dev.value, ho.dev.impact, ho.dev.normal, ho.dev.shadowed,
                              ho.dev.rgba, nullptr, whole_fb ? nullptr : &own);
        c->keep_ev0 = false;
        if (rc) return rc;
    }
    return finish_out(c, ho);
}

// A batch of whole frames (T == 0: vhx_trace_primary_batch) or of tile sets (T > 0: vhx_trace_tiles_batch; frame k is
// the tiles starts[k], starts[k] + stride, ... of its camera's T x T tile grid, in the tile layout) as one pass ladder.
static int trace_batch(vhx_ctx *c, const vhx_camera *cams, uint32_t n, const vhx_hits *outs, uint32_t T,
                       const uint32_t *starts, uint32_t stride, const char *fn) {
    if (!c || !cams || !outs || n == 0 || (T && (!starts || stride == 0 || T > 4096))) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, std::string(fn) + " before vhx_upload_tree");
    const uint32_t W = cams[0].width, H = cams[0].height;
    for (uint32_t k = 0; k < n; ++k) {
        if (cams[k].width != W || cams[k].height != H || W == 0 || H == 0 || cams[k].ray_model > VHX_RAY_GLASS)
            return fail(c, VHX_E_INVALID_ARG, std::string(fn) + ": every frame needs one valid camera model and the "
                                              "same non-empty width x height");
        if (outs[k].bytes)
            return fail(c, VHX_E_INVALID_ARG, std::string(fn) + ": byte counting is a vhx_trace_primary option");
        if (c->shadow_on && (!outs[k].value || !outs[k].impact || !outs[k].normal || !outs[k].shadowed))
            return fail(c, VHX_E_INVALID_ARG, std::string(fn) + " with a shadow light: value, impact, normal and "
                                              "shadowed outputs needed");
    }
    // per frame: its output entries (a tile set: its tiles' entries), the index stride between frames (npix) and the
    // pass-0 workgroups (nbf)
    const uint32_t tiles_x = T ? (W + T - 1) / T : 0u, ntiles = T ? tiles_x * ((H + T - 1) / T) : 0u;
    const uint32_t bpx = T ? (T + 15) / 16 : 0u, bpt = bpx * bpx;
    auto set_tiles = [&](uint32_t k) -> uint64_t {
        return starts[k] >= ntiles ? 0ull : (uint64_t)(ntiles - starts[k] + stride - 1) / stride;
    };
    uint64_t max_tiles = 0;
    if (T)
        for (uint32_t k = 0; k < n; ++k) max_tiles = std::max(max_tiles, set_tiles(k));
    if (T && max_tiles == 0) return VHX_OK;  // no frame holds a tile
    const uint64_t npix = T ? max_tiles * T * T : (uint64_t)W * H, nout = npix * n;
    // the frames are traced concurrently: two frames writing one output range would leave a result that depends on the
    // schedule instead of equalling n single-frame calls
    {
        std::vector<MemRange> written;
        for (uint32_t k = 0; k < n; ++k) {
            const vhx_hits &o = outs[k];
            const uint64_t ent = T ? set_tiles(k) * T * T : npix;
            const void *f[7] = {o.value, o.cell, o.rgba, o.depth, o.voxel, o.impact, o.normal};
            const uint64_t w[7] = {1, 1, 1, 1, 3, 3, 3};
            for (int j = 0; j < 7; ++j) written.push_back({f[j], ent * 4 * w[j]});
            if (c->shadow_on) written.push_back({o.shadowed, ent * 4});  // without a light it is ignored
        }
        if (ranges_meet(written, {}))
            return fail(c, VHX_E_INVALID_ARG, std::string(fn) + ": output arrays overlap each other");
    }
    const uint32_t bx = (W + 15) / 16, by = (H + 15) / 16;
    const uint64_t nbf = T ? max_tiles * bpt : (uint64_t)bx * by, nblocks = nbf * n;
    if (nout > 0x7FFFFFFFull || nblocks > 0x7FFFFFFFull)
        return fail(c, VHX_E_INVALID_ARG, std::string(fn) + ": more than 2^31 rays in one batch");
    TraceCall tr(c);
    int rc = tr.rc;
    if (rc) return rc;
    DevTree t;
    if ((rc = tr.tree(t))) return rc;
    if (t.mips) return fail(c, VHX_E_INVALID_ARG, std::string(fn) + ": not available with node MIPs");
    // the batch's cameras, outputs (and tile-set starts), staged for one copy to the device
    const uint64_t cam_bytes = ((uint64_t)n * sizeof(CamD) + 255) & ~255ull;
    const uint64_t out_bytes = ((uint64_t)n * sizeof(OutD) + 255) & ~255ull;
    const uint64_t args_bytes = cam_bytes + out_bytes + (T ? (uint64_t)n * 4 : 0ull);
    vhx_ctx::Pinned *P = nullptr;
    if ((rc = stage_acquire(c, c->batch_pinned, c->batch_next, c->batch_args, args_bytes, P))) return rc;
    CamD *hc = (CamD *)P->ptr;
    OutD *ho = (OutD *)((uint8_t *)P->ptr + cam_bytes);
    for (uint32_t k = 0; k < n; ++k) {
        hc[k] = cam_of(&cams[k]);
        ho[k] = OutD{outs[k].value, outs[k].cell,   outs[k].voxel, outs[k].rgba,
                     nullptr,       outs[k].impact, outs[k].normal, outs[k].depth, outs[k].shadowed};
    }
    if (T) std::memcpy((uint8_t *)P->ptr + cam_bytes + out_bytes, starts, (size_t)n * 4);
    uint32_t npass = 1;
    if ((rc = prepare_passes(c, nout, nblocks, npass, false, n > 1))) return rc;
    if ((rc = tr.start()) || (rc = stage_commit(c, *P, c->batch_args, args_bytes))) return rc;
    const CamD *dcams = (const CamD *)c->batch_args.ptr;
    const OutD *douts = (const OutD *)((const uint8_t *)c->batch_args.ptr + cam_bytes);
    const uint32_t *dstarts = T ? (const uint32_t *)((const uint8_t *)c->batch_args.ptr + cam_bytes + out_bytes) : nullptr;
    const TileB tb{T, tiles_x, ntiles, stride, bpx, bpt};
    // the frames' blocks over whole tiles of the list order (k_trace_primary), or flags in the flag order; a batch of
    // tile sets lists its rays in its own block order (ListOrder::tl) or compacts flags in output-index order
    Pass0Plan p0;
    if ((rc = plan_pass0(c, npass, !T, T != 0, W, H, nbf, n, c->shadow_on, false, p0))) return rc;
    QueueRun run;
    run.src.kind = 4u;
    run.src.cams = dcams;
    run.src.outs = douts;
    run.src.npix = (uint32_t)npix;
    run.src.T = T;
    run.src.tiles_x = tiles_x;
    run.src.tile_stride = stride;
    run.src.starts = dstarts;
    run.npass = npass;
    run.nout = nout;
    run.nblocks0 = p0.nbf * n;
    run.pass0 = p0.p0();
    run.order_w = T ? 0u : W;
    run.order_h = H;
    run.frames = n;
    run.qm = p0.qm;
    const PassQ q0 = pass0_q(c, npass, run.pass0, p0.qm);
    // everything the kernel would derive from the grid size, and its divisions, as constants
    BatchGrid bg = batch_grid((uint32_t)run.nblocks0, n, (uint32_t)p0.nbf, bx, q0, p0.lo, tb);
    // The worklist (k_classify_blocks): whole frames listed in the list order, without fused shadows. Three launches
    // ahead of pass 0 on the same stream; the buffer (header, entries, and the build's ballots, counts and offsets)
    // keeps the upper bound of the launch and grows only when a larger batch comes. The lists' extent, 256 rays per
    // tree block, must fit the 32 bits of a device-side length; a batch of more (tiny frames by the million) takes the
    // full path for every block, like skyblocks = 0.
    const uint32_t *dwork = nullptr;  // null: every block takes the full path
    if (c->skyblocks && !T && p0.listed && p0.lo.tx && !p0.fuse && ((uint64_t)bx * by * n + 1) * 256 <= 0xFFFFFFFFull) {
        const uint32_t nb0 = (uint32_t)run.nblocks0, ng = (nb0 + 255u) / 256u;  // the build's grid
        const uint64_t ent_words = (WORK_HDR + (uint64_t)nb0 + 1) & ~1ull;  // the ballots that follow are 8-byte words
        if ((rc = ensure(c, c->work, (ent_words + 20ull * ng) * 4))) return rc;
        uint32_t *work = (uint32_t *)c->work.ptr;
        uint64_t *masks = (uint64_t *)(work + ent_words);  // two per wave of the grid
        uint32_t *wcounts = work + ent_words + 16ull * ng, *woffsets = wcounts + 2ull * ng;
        bg.sbx = bx;
        bg.sby = by;
        bg.W = W;
        bg.H = H;
        k_classify_blocks<<<ng, 256, 0, c->stream>>>(dcams, bg, p0.lo, (uint32_t)p0.nbf, q0.finter, nb0, t.size, masks,
                                                      wcounts);
        launch_scan(c, wcounts, 2u * ng, nullptr, 1, woffsets, work + 1, 2ull * ng);
        k_emit_worklist<<<ng, 256, 0, c->stream>>>(masks, woffsets, work);
        dwork = work;
        run.n0 = work + 2;
    }
    int qrc = VHX_OK;
    const bool bd_ok = dispatch_variant(c->tree->desc.brick_dim, false, false, p0.fuse, false, [&](auto bd_tag, auto v) {
        constexpr int BD = decltype(bd_tag)::value;
        constexpr bool FUSE = decltype(v)::FUSE;
        k_trace_primary_batch<BD, FUSE><<<(unsigned)run.nblocks0, 256, 0, c->stream>>>(
            t, dcams, douts, (uint32_t)p0.nbf, bx, (uint32_t)npix, q0, bg, p0.lo, tb, dstarts, dwork);
        qrc = launch_queue_passes<false, BD, false, FUSE>(c, t, run);
    });
    if (!bd_ok) return fail(c, VHX_E_INVALID_ARG, "unsupported brick_dim");
    if ((rc = tr.end(qrc))) return rc;
    // a shadow trace (or shadow batch) of these frames' hit records lists them in the same tile order
    c->last_fb_w = T ? 0u : W;
    c->last_fb_h = T ? 0u : H;
    if (c->shadow_on && !p0.fuse) {  // the frames' shadow rays after their primary rays (vhx_trace_primary's fallback)
        c->keep_ev0 = true;
        for (uint32_t k = 0; k < n && !rc; ++k) {
            const uint64_t ent = T ? set_tiles(k) * T * T : npix;
            // a tile set owns its in-frame entries only (tile padding stays as it is), a whole frame all of them
            const OwnGeom own{W, H, T, tiles_x, T ? starts[k] : 0u, stride, 1u};
            if (ent)
                rc = trace_shadows_of(c, c->shadow_light, ent, outs[k].value, outs[k].impact, outs[k].normal,
                                      outs[k].shadowed, outs[k].rgba, nullptr, T ? &own : nullptr);
        }
        c->keep_ev0 = false;
    }
    return rc;
}

int vhx_trace_primary_batch(vhx_ctx *c, const vhx_camera *cams, uint32_t n, const vhx_hits *outs) {
    return trace_batch(c, cams, n, outs, 0, nullptr, 1, "vhx_trace_primary_batch");
}

int vhx_trace_tiles_batch(vhx_ctx *c, const vhx_camera *cams, uint32_t n, uint32_t tile_size, const uint32_t *tile_starts,
                          uint32_t tile_stride, const vhx_hits *outs) {
    if (tile_size == 0) return c ? fail(c, VHX_E_INVALID_ARG, "vhx_trace_tiles_batch: tile_size 0") : VHX_E_INVALID_ARG;
    return trace_batch(c, cams, n, outs, tile_size, tile_starts, tile_stride, "vhx_trace_tiles_batch");
}


int vhx_tail_info(vhx_ctx *c, uint32_t *listed, uint32_t *width, uint32_t *height) {
    if (!c) return VHX_E_INVALID_ARG;
    uint32_t n = 0;
    if (c->tail_on && c->tail_valid && c->tail_list[c->tail_cur].ptr) {
        VHX_HIP(c, hipSetDevice(c->device));
        VHX_STREAM(c);
        VHX_HIP(c, hipMemcpyAsync(&n, c->tail_list[c->tail_cur].ptr, 4, hipMemcpyDeviceToHost, c->stream));
        VHX_HIP(c, hipStreamSynchronize(c->stream));
        n = std::min(n, c->tail_cap);
    }
    if (listed) *listed = n;
    if (width) *width = c->tail_valid ? c->tail_w : 0u;
    if (height) *height = c->tail_valid ? c->tail_h : 0u;
    return VHX_OK;
}

int vhx_chain_profile(vhx_ctx *c, const vhx_camera *cam, const uint32_t *pixels, uint32_t n, uint64_t *out) {
    if (!c || !cam || (n && (!pixels || !out))) return VHX_E_INVALID_ARG;
#if VHX_CHAIN
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_chain_profile before vhx_upload_tree");
    if (n == 0) return VHX_OK;
    for (uint32_t k = 0; k < n; ++k)
        if (pixels[k] >= (uint64_t)cam->width * cam->height) return fail(c, VHX_E_INVALID_ARG, "vhx_chain_profile: pixel outside the frame");
    TraceCall tr(c);
    int rc = tr.rc;
    if (rc) return rc;
    DevTree t;
    if ((rc = tr.tree(t))) return rc;
    if (t.mips) return fail(c, VHX_E_INVALID_ARG, "vhx_chain_profile: not with node MIPs");
    const uint64_t pbytes = ((uint64_t)n * 4 + 255) & ~255ull, obytes = (uint64_t)n * VHX_CHAIN_WORDS * 8;
    if ((rc = ensure(c, c->scratch, pbytes + obytes))) return rc;
    uint32_t *dpix = (uint32_t *)c->scratch.ptr;
    unsigned long long *dout = (unsigned long long *)((uint8_t *)c->scratch.ptr + pbytes);
    VHX_HIP(c, hipMemcpyAsync(dpix, pixels, (uint64_t)n * 4, hipMemcpyHostToDevice, c->stream));
    const CamD cd = cam_of(cam);
    auto launch = [&](auto bd_tag) {
        constexpr int BD = decltype(bd_tag)::value;
        k_chain<BD><<<n, 64, 0, c->stream>>>(t, cd, dpix, n, dout);
    };
    if (!dispatch_bd(c->tree->desc.brick_dim, launch)) return fail(c, VHX_E_INVALID_ARG, "unsupported brick_dim");
    VHX_HIP(c, hipGetLastError());
    VHX_HIP(c, hipMemcpyAsync(out, dout, obytes, hipMemcpyDeviceToHost, c->stream));
    VHX_HIP(c, hipStreamSynchronize(c->stream));
    return tr.scope.end();
#else
    return fail(c, VHX_E_STATE, "vhx_chain_profile: libvhx was built without VHX_CHAIN");
#endif
}

int vhx_profile_counters(vhx_ctx *c, uint64_t *out, uint32_t n, int reset) {
    if (!c || (n && !out)) return VHX_E_INVALID_ARG;
#if VHX_PROF
    uint64_t v[5 * 16 * 2];
    VHX_HIP(c, hipSetDevice(c->device));
    VHX_HIP(c, hipDeviceSynchronize());
    VHX_HIP(c, hipMemcpyFromSymbol(v, HIP_SYMBOL(vhx::g_prof), sizeof(v)));
    for (uint32_t i = 0; i < n && i < 5 * 16 * 2; ++i) out[i] = v[i];
    if (reset) {
        std::memset(v, 0, sizeof(v));
        VHX_HIP(c, hipMemcpyToSymbol(HIP_SYMBOL(vhx::g_prof), v, sizeof(v)));
    }
    return VHX_OK;
#else
    (void)reset;
    return fail(c, VHX_E_STATE, "vhx_profile_counters: libvhx was built without VHX_PROF");
#endif
}

int vhx_trace_rays(vhx_ctx *c, const float *rays, uint64_t n, const vhx_hits *out, int on_device) {
    if (!c || !out || (!rays && n)) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_trace_rays before vhx_upload_tree");
    if (n == 0) return VHX_OK;
    if ((n + 255) / 256 > 0x7FFFFFFFull) return fail(c, VHX_E_INVALID_ARG, "too many rays");
    TraceCall tr(c);
    int rc = tr.rc;
    if (rc) return rc;
    HostOut ho;
    if ((rc = map_out(c, out, n, on_device, ho))) return rc;
    const float *drays = rays;
    if (!on_device) {
        // context-owned staging buffer (a stream-ordered hipMallocAsync buffer here intermittently handed the
        // kernel stale ray data after a pageable host copy on ROCm 7.2)
        if ((rc = ensure(c, c->rays, n * 24))) return rc;
        VHX_HIP(c, hipMemcpyAsync(c->rays.ptr, rays, n * 24, hipMemcpyHostToDevice, c->stream));
        drays = (const float *)c->rays.ptr;
    }
    DevTree t;
    if ((rc = tr.tree(t))) return rc;
    if (t.mips && out->bytes)
        return fail(c, VHX_E_INVALID_ARG, "vhx_trace_rays: byte counting is not available with node MIPs");
    QueueRun run;
    run.src.kind = 2u;
    run.src.rays = drays;
    run.out = ho.dev;
    run.nout = n;
    run.nblocks0 = (n + 255) / 256;
    if ((rc = prepare_passes(c, n, run.nblocks0, run.npass))) return rc;
    if ((rc = tr.start()) || (rc = reset_passes(c, run.npass))) return rc;
    const PassQ q0 = pass0_q(c, run.npass, P0_LISTS);
    int qrc = VHX_OK;
    const bool bd_ok = dispatch_variant(c->tree->desc.brick_dim, t.mips != nullptr, ho.dev.bytes != nullptr, false, false,
                                        [&](auto bd_tag, auto v) {
        constexpr int BD = decltype(bd_tag)::value;
        using V = decltype(v);
        k_trace_rays<V::COUNT, BD, V::MIP><<<(unsigned)run.nblocks0, 256, 0, c->stream>>>(t, drays, n, ho.dev, q0);
        qrc = launch_queue_passes<V::COUNT, BD, V::MIP, V::FUSE>(c, t, run);
    });
    if (!bd_ok) return fail(c, VHX_E_INVALID_ARG, "unsupported brick_dim");
    if ((rc = tr.end(qrc))) return rc;
    return finish_out(c, ho);
}

// The flag order of a shadow trace over `frames` frames of n hit records each: when n is the pixel count of this
// context's last framebuffer frame, the tile order of c->qorder (any order is a permutation of 0..n-1, so the records
// need not even be that frame's for the result to be exact), else output-index order. npos: the positions to scan.
static FlagOrder shadow_order(const vhx_ctx *c, uint64_t n, uint32_t frames, uint64_t &npos) {
    const bool fb = c->last_fb_w && (uint64_t)c->last_fb_w * c->last_fb_h == n;
    npos = n * frames;
    const FlagOrder ord = flag_order(fb ? c->qorder : 0u, c->last_fb_w, c->last_fb_h, npos, frames);
    if (!ord.W) npos = n * frames;
    return ord;
}

// vhx_trace_shadows; own (the shadow rays that follow a primary trace inside vhx_trace_primary and the batches): only
// the entries that trace owns are read, cleared, listed and written -- tile padding and other ranks' pixels stay as
// they are. Null: every i < n, the public contract, through the same kernels as ever.
static int trace_shadows_of(vhx_ctx *c, const float light[3], uint64_t n, const uint32_t *value, const float *impact,
                            const float *normal, uint32_t *shadowed, uint32_t *rgba, uint32_t *bytes,
                            const OwnGeom *own) {
    if (!c || !light || (n && (!value || !impact || !normal || !shadowed))) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_trace_shadows before vhx_upload_tree");
    if (n == 0) return VHX_OK;
    if (n >= 0x7FFFFFFFull) return fail(c, VHX_E_INVALID_ARG, "too many rays");
    // the outputs are written while the hit records are still being read (the flags are cleared by the compaction
    // kernel that reads value[]): they must not overlap them or each other
    const int meet = ranges_meet({{shadowed, n * 4}, {rgba, n * 4}, {bytes, n * 4}},
                                 {{value, n * 4}, {impact, n * 12}, {normal, n * 12}});
    if (meet == 1) return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows: an output overlaps the hit records");
    if (meet == 2) return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows: outputs overlap each other");
    TraceCall tr(c);
    int rc = tr.rc;
    if (rc) return rc;
    QueueRun run;
    run.first = 0;
    run.nout = n;
    run.nblocks0 = (n + 255) / 256;
    if ((rc = prepare_passes(c, n, run.nblocks0, run.npass, true))) return rc;
    DevTree t;
    if ((rc = tr.tree(t))) return rc;
    if (t.mips && bytes)
        return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows: byte counting is not available with node MIPs");
    run.src.kind = 3u;
    run.src.impact = impact;
    run.src.normal = normal;
    run.src.lx = light[0];
    run.src.ly = light[1];
    run.src.lz = light[2];
    run.out.value = shadowed;
    run.out.rgba = rgba;
    run.out.bytes = bytes;
    run.qm = queue_state_mode(c, false, true, run.npass);
    if ((rc = tr.start())) return rc;
    // no reset_passes: the hit compaction (k_count_flags) zeroes the queue passes' counters
    if (bytes) VHX_HIP(c, hipMemsetAsync(bytes, 0, n * 4, c->stream));
    // wave-dense secondary rays: the hit pixels, in the frame's queue order, are pass 0's queue
    uint64_t npos = 0;
    const FlagOrder ord = shadow_order(c, n, 1, npos);
    if (own)
        rc = compact_owned_hits(c, value, n, *own, (uint32_t *)c->qctl.ptr + 7, (uint32_t *)c->queue[1].ptr, shadowed);
    else
        rc = compact_flags<true>(c, value, npos, ord, (uint32_t *)c->qctl.ptr + 7, (uint32_t *)c->queue[1].ptr, shadowed, n);
    if (rc) return rc;
    int qrc = VHX_OK;
    const bool bd_ok = dispatch_variant(c->tree->desc.brick_dim, t.mips != nullptr, bytes != nullptr, false, false,
                                        [&](auto bd_tag, auto v) {
        using V = decltype(v);
        qrc = launch_queue_passes<V::COUNT, decltype(bd_tag)::value, V::MIP, V::FUSE>(c, t, run);
    });
    if (!bd_ok) return fail(c, VHX_E_INVALID_ARG, "unsupported brick_dim");
    return tr.end(qrc);
}

int vhx_trace_shadows(vhx_ctx *c, const float light[3], uint64_t n, const uint32_t *value, const float *impact,
                      const float *normal, uint32_t *shadowed, uint32_t *rgba, uint32_t *bytes) {
    return trace_shadows_of(c, light, n, value, impact, normal, shadowed, rgba, bytes, nullptr);
}

int vhx_trace_shadows_batch(vhx_ctx *c, const float light[3], uint32_t nf, uint64_t n, const vhx_shadow_frame *frames) {
    if (!c || !light || nf == 0 || !frames) return VHX_E_INVALID_ARG;
    if (!c->tree->uploaded) return fail(c, VHX_E_STATE, "vhx_trace_shadows_batch before vhx_upload_tree");
    if (n == 0) return VHX_OK;
    // tested before the product is formed (a huge n would wrap n * nf)
    if (n >= 0x7FFFFFFFull / nf) return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows_batch: more than 2^31 records");
    const uint64_t ntot = n * nf;
    // every frame's outputs are written while every frame's hit records are read: no overlaps anywhere in the batch
    {
        std::vector<MemRange> outs, ins;
        for (uint32_t k = 0; k < nf; ++k) {
            const vhx_shadow_frame &f = frames[k];
            if (!f.value || !f.impact || !f.normal || !f.shadowed)
                return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows_batch: a frame lacks value, impact, normal or shadowed");
            outs.push_back({f.shadowed, n * 4});
            outs.push_back({f.rgba, n * 4});
            ins.push_back({f.value, n * 4});
            ins.push_back({f.impact, n * 12});
            ins.push_back({f.normal, n * 12});
        }
        const int meet = ranges_meet(outs, ins);
        if (meet == 1) return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows_batch: an output overlaps the hit records");
        if (meet == 2) return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows_batch: outputs overlap each other");
    }
    TraceCall tr(c);
    int rc = tr.rc;
    if (rc) return rc;
    DevTree t;
    if ((rc = tr.tree(t))) return rc;
    if (t.mips) return fail(c, VHX_E_INVALID_ARG, "vhx_trace_shadows_batch: not available with node MIPs");
    QueueRun run;
    run.first = 0;
    run.nout = ntot;
    run.nblocks0 = (ntot + 255) / 256;
    run.frames = nf;
    if ((rc = prepare_passes(c, ntot, run.nblocks0, run.npass, true, nf > 1))) return rc;
    // the frames' ShD records, then their value pointers (FlagOrder::fvals), staged like vhx_trace_primary_batch's
    const uint64_t sh_bytes = ((uint64_t)nf * sizeof(ShD) + 255) & ~255ull, args_bytes = sh_bytes + (uint64_t)nf * 8;
    vhx_ctx::Pinned *P = nullptr;
    if ((rc = stage_acquire(c, c->shadow_pinned, c->shadow_next, c->shadow_args, args_bytes, P))) return rc;
    ShD *hs = (ShD *)P->ptr;
    uint64_t *hv = (uint64_t *)((uint8_t *)P->ptr + sh_bytes);
    for (uint32_t k = 0; k < nf; ++k) {
        hs[k] = ShD{frames[k].value, frames[k].impact, frames[k].normal, frames[k].shadowed, frames[k].rgba};
        hv[k] = (uint64_t)(uintptr_t)frames[k].value;
    }
    if ((rc = tr.start()) || (rc = stage_commit(c, *P, c->shadow_args, args_bytes))) return rc;
    // shadowed = 0 where no shadow ray is cast (vhx_trace_shadows clears inside its count kernel)
    for (uint32_t k = 0; k < nf; ++k) VHX_HIP(c, hipMemsetAsync(frames[k].shadowed, 0, n * 4, c->stream));
    run.src.kind = 5u;
    run.src.lx = light[0];
    run.src.ly = light[1];
    run.src.lz = light[2];
    run.src.npix = (uint32_t)n;
    run.src.shs = (const ShD *)c->shadow_args.ptr;
    run.qm = queue_state_mode(c, false, true, run.npass);
    // every frame's hit records in the tile order of the frames they came from (c->last_fb_*), frame by frame
    uint64_t npos = 0;
    FlagOrder ord = shadow_order(c, n, nf, npos);
    ord.fpix = n;
    ord.fvals = (const uint64_t *)((const uint8_t *)c->shadow_args.ptr + sh_bytes);
    if ((rc = compact_flags<true>(c, nullptr, npos, ord, (uint32_t *)c->qctl.ptr + 7, (uint32_t *)c->queue[1].ptr)))
        return rc;
    int qrc = VHX_OK;
    const bool bd_ok = dispatch_bd(c->tree->desc.brick_dim, [&](auto bd_tag) {
        qrc = launch_queue_passes<false, decltype(bd_tag)::value>(c, t, run);
    });
    if (!bd_ok) return fail(c, VHX_E_INVALID_ARG, "unsupported brick_dim");
    return tr.end(qrc);
}


}  // extern "C"
