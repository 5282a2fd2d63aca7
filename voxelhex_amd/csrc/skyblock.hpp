// Sky blocks: whether every pixel of a pixel rectangle of a glass-camera frame is certain to miss the root cube on the
// exact path -- primary_ray (vhx_device.hip) followed by the slab test of Trav::begin (trace.hpp). Pass 0 of a batch
// asks this once per 16x16 block before the block's workgroup starts (k_classify_blocks); a block that is sky in every
// pixel writes its miss records and leaves without the traversal prologue.
//
// Self-contained: no includes beyond <stdint.h>, only + - * / and comparisons in double precision (IEEE, no fused
// operations under -ffp-contract=off, no approximate reciprocals), so the host compiler and the device compiler give
// the same answer and the function is tested on the CPU against the oracle pixel by pixel (tests/test_skyblock.py).
// VHX_SKY_FN supplies the function qualifiers (__host__ __device__ in the device unit, nothing on the host).
//
// The exact path, per pixel (px, py), every operation rounded to f32, x = px, y = height - 1 - py:
//     v_k = ((bl_k + (r_k * x) * pw) + (u_k * y) * ph) - o_k            k = x, y, z
//     L   = sqrt((v_x^2 + v_y^2) + v_z^2),   d_k = v_k / L
//     t_k0 = (0 - o_k) / d_k,   t_k1 = (S - o_k) / d_k                  (0 - o_k is exact; a_k1 = fl(S - o_k) below)
//     near_k = fmin(t_k0, t_k1), far_k = fmax(t_k0, t_k1)               (fmin / fmax ignore a NaN operand)
//     tmin = max_k near_k, tmax = min_k far_k;   the ray misses iff tmax < 0 or tmin > tmax.
//
// Soundness argument.
//  1. Guards. The function answers false unless every camera value is finite and below 2^40 in magnitude, the frame is
//     narrower than 2^24 pixels each way (x and y are then exact as f32), and M_k = |bl_k| + |r_k| xmax |pw| +
//     |u_k| ymax |ph| + |o_k| < 2^40. No f32 operation of the v_k chain overflows then (|r_k x| < 2^64, times pw < 2^104),
//     NaN and +-inf inputs never get further than this test (the comparisons are written so that a NaN fails them).
//  2. Range of v_k. The real value w_k(x, y) = bl_k + r_k x pw + u_k y ph - o_k is affine in the pixel, so over the
//     rectangle it lies between the least and the greatest of its four corner values. The f32 evaluation makes seven
//     roundings, each at most 2^-24 relative to a partial result that is at most M_k in magnitude (or 2^-150 absolute
//     where a partial result is subnormal, amplified by |pw|, |ph| < 2^40 at most): |v_k - w_k| < 5.1 * 2^-24 M_k +
//     2^-108. The corners are evaluated in double (errors of 2^-53 M_k each). The range is widened by
//     E_k = 2^-20 M_k + 2^-100, more than three times what these add up to. Every pixel's f32 v_k is in [lo_k, hi_k].
//  3. Axes used. An axis is used only if its range excludes zero by 2^-40: lo_k > 2^-40 or hi_k < -2^-40. For a used axis
//     and any pixel, 2^-40 < |v_k| < 2^41, so v_k^2 is a normal f32, L is positive, finite and at most 2^42, d_k is a normal
//     f32 with the sign of v_k and one rounding, and t_kj = fl(a_kj / d_k) is finite (below 2^41 * 2^42 * 2^40), never NaN,
//     and zero only if a_kj is zero:
//         t_kj = L * (a_kj / v_k) * (1 + e),  |e| < 2.1 * 2^-24   (plus at most 2^-150 absolute when subnormal),
//     with the same L > 0 on every axis of that pixel. An axis that is not used is dropped. That is conservative
//     whatever its f32 values are: fmin / fmax skip a NaN, and any other value, infinite ones included, can only lower
//     tmax = min_k far_k and raise tmin = max_k near_k, so tmax <= min over used axes of far_k and tmin >= max over used
//     axes of near_k. (The values of the used axes are not NaN, so those bounds are ordinary comparisons.)
//  4. Bounds per used axis. q = a_kj / v is monotone in v on a range that excludes zero, so over [lo_k, hi_k] it lies
//     between a_kj / lo_k and a_kj / hi_k. Nlow_k, the least of the four quotients (j = 0, 1 at lo_k and hi_k), is a lower
//     bound of every pixel's near_k / L up to the relative error above; Fhigh_k, the greatest, an upper bound of far_k / L.
//     T is the greatest magnitude among all these quotients, N = max_k Nlow_k, F = min_k Fhigh_k, m = 2^-20 T + 2^-100:
//     sixteen f32 roundings relative to the largest t involved, against the 4.2 needed for two values (the quotients'
//     own double rounding, 2^-53, and the subnormal term 2^-150 / L < 2^-110 are far inside it).
//  5. F < -m: on the axis k that gives F both quotients are negative for every pixel, so a_k0 and a_k1 are non-zero and
//     differ in sign from v_k; t_k0 and t_k1 are then negative, non-zero f32 values (|t| >= |a| (1 - 2^-23) > 0: no
//     underflow to -0), far_k < 0 and tmax <= far_k < 0: a miss.
//     N - F > m with N from axis a and F from axis b: for every pixel near_a >= L (N - 2.1 * 2^-24 T - ...) and
//     far_b <= L (F + 2.1 * 2^-24 T + ...), so near_a - far_b >= L (N - F - 4.3 * 2^-24 T - ...) > 0 and
//     tmin >= near_a > far_b >= tmax: a miss.
//  6. The matrix camera model is never classified (like glass_clear_miss).
// A rectangle is given in frame pixels, inclusive, already clipped to the frame: x0 <= x1 < width, y0 <= y1 < height.
#pragma once
#include <stdint.h>

#ifndef VHX_SKY_FN
#define VHX_SKY_FN
#endif

namespace vhx {

// the glass camera as the kernels hold it (the CamD fields, in its order)
struct SkyCam {
    uint32_t model, width, height;
    float o[3], bl[3], r[3], u[3], pw, ph;
};

VHX_SKY_FN inline double sky_abs(double a) { return a < 0.0 ? -a : a; }
// false for NaN and +-inf as well
VHX_SKY_FN inline bool sky_small(double a) { return sky_abs(a) < 1099511627776.0; }  // 2^40

VHX_SKY_FN inline bool block_is_sky(const SkyCam &c, uint32_t tree_size, uint32_t x0, uint32_t y0, uint32_t x1,
                                    uint32_t y1) {
    if (c.model != 1u /* VHX_RAY_GLASS */) return false;
    if (c.width >= (1u << 24) || c.height >= (1u << 24) || x0 > x1 || y0 > y1 || x1 >= c.width || y1 >= c.height)
        return false;
    if (!sky_small((double)c.pw) || !sky_small((double)c.ph)) return false;
    const double pw = (double)c.pw, ph = (double)c.ph;
    // the glass counts y upward: pixel row py is y = height - 1 - py
    const double xa = (double)x0, xb = (double)x1, ya = (double)(c.height - 1u - y1), yb = (double)(c.height - 1u - y0);
    const float tsize = (float)tree_size;
    const double E_REL = 1.0 / 1048576.0;                    // 2^-20
    const double TINY = 7.888609052210118e-31;               // 2^-100
    const double VMIN = 9.094947017729282e-13;               // 2^-40
    bool any = false;
    double N = 0.0, F = 0.0, T = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double o = (double)c.o[k], bl = (double)c.bl[k], r = (double)c.r[k], u = (double)c.u[k];
        if (!sky_small(o) || !sky_small(bl) || !sky_small(r) || !sky_small(u)) return false;
        const double M = sky_abs(bl) + sky_abs(r) * xb * sky_abs(pw) + sky_abs(u) * yb * sky_abs(ph) + sky_abs(o);
        if (!sky_small(M)) return false;
        // the four corners of the affine v_k
        const double rxa = r * xa * pw, rxb = r * xb * pw, uya = u * ya * ph, uyb = u * yb * ph;
        const double w0 = bl + rxa + uya - o, w1 = bl + rxb + uya - o, w2 = bl + rxa + uyb - o, w3 = bl + rxb + uyb - o;
        double lo = w0, hi = w0;
        lo = w1 < lo ? w1 : lo;
        lo = w2 < lo ? w2 : lo;
        lo = w3 < lo ? w3 : lo;
        hi = w1 > hi ? w1 : hi;
        hi = w2 > hi ? w2 : hi;
        hi = w3 > hi ? w3 : hi;
        const double E = E_REL * M + TINY;
        lo -= E;
        hi += E;
        if (!(lo > VMIN || hi < -VMIN)) continue;  // the range touches zero: the axis is dropped
        // the slab planes as the exact path forms them: 0 - o_k (exact) and S - o_k rounded to f32
        const double a0 = (double)(0.0f - c.o[k]), a1 = (double)(tsize - c.o[k]);
        const double q0 = a0 / lo, q1 = a0 / hi, q2 = a1 / lo, q3 = a1 / hi;
        double nl = q0, fh = q0;
        nl = q1 < nl ? q1 : nl;
        nl = q2 < nl ? q2 : nl;
        nl = q3 < nl ? q3 : nl;
        fh = q1 > fh ? q1 : fh;
        fh = q2 > fh ? q2 : fh;
        fh = q3 > fh ? q3 : fh;
        const double t = sky_abs(nl) > sky_abs(fh) ? sky_abs(nl) : sky_abs(fh);
        if (!any) {
            N = nl;
            F = fh;
            T = t;
            any = true;
        } else {
            N = nl > N ? nl : N;
            F = fh < F ? fh : F;
            T = t > T ? t : T;
        }
    }
    if (!any) return false;
    const double m = E_REL * T + TINY;
    return F < -m || N - F > m;
}

}  // namespace vhx
