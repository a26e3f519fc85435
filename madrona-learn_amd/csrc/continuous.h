// Continuous (diagonal Gaussian) action distribution math shared by the
// device kernels and the host sampler of continuous.hip.
// ContinuousActionDistributions (dists.py:211-284): per dimension
//   m = tanh(x), s = (hi - lo) sigmoid(y + 2) + lo, z = (a - m) / s,
//   logp = -z^2 / 2 - ln s - ln(2 pi) / 2, ent = ln s + ln(2 pi) / 2 + 1/2.
#pragma once
#include <math.h>

#include "common.h"

namespace ml {

constexpr float kHalfLn2Pi = 0.918938533204672742f;

// ---------------------------------------------------------------------------
// sin(2 pi u), cos(2 pi u) of u = k 2^-24 (u32_to_unit's values).  Only exact
// IEEE operations, contraction off, so host C and the GPU agree bit for bit.
// Octant reduction on the exact u: 8u = q + f with q in 0..7 and f in [0, 1)
// a multiple of 2^-21, both exact; r = f (q even) or 1 - f (q odd, exact
// too) puts the angle (pi/4) r in [0, pi/4], where the Taylor polynomials in
// r (coefficients (pi/4)^n / n! rounded to f32) are evaluated by Horner with
// fmaf.  Truncation < 2e-9; measured max abs error over all 2^23 inputs is
// below 2^-23 (bound required: 2^-22).
// ---------------------------------------------------------------------------
__host__ __device__ inline void det_sincos2pi(float u, float* sn, float* cs) {
#pragma clang fp contract(off)
    const float t = u * 8.0f;
    const int q = (int)t;
    const float f = t - (float)q;
    const float r = (q & 1) ? 1.0f - f : f;
    const float r2 = r * r;
    float ps = 3.13361681492097e-07f;
    ps = __builtin_fmaf(ps, r2, -3.657620254671201e-05f);
    ps = __builtin_fmaf(ps, r2, 2.490394515916705e-03f);
    ps = __builtin_fmaf(ps, r2, -8.074551075696945e-02f);
    ps = __builtin_fmaf(ps, r2, 0.7853981852531433f);
    const float s = ps * r;
    float pc = 1.1501159052906829e-10f;
    pc = __builtin_fmaf(pc, r2, -2.461136894282845e-08f);
    pc = __builtin_fmaf(pc, r2, 3.5908603877032874e-06f);
    pc = __builtin_fmaf(pc, r2, -3.259918885305524e-04f);
    pc = __builtin_fmaf(pc, r2, 1.585434377193451e-02f);
    pc = __builtin_fmaf(pc, r2, -0.3084251284599304f);
    const float c = __builtin_fmaf(pc, r2, 1.0f);
    // octants 1, 2, 5, 6 exchange the two; sin < 0 in 4..7, cos < 0 in 2..5
    const bool swap = ((q + 1) & 2) != 0;
    const float sv = swap ? c : s, cv = swap ? s : c;
    *sn = (q & 4) ? -sv : sv;
    *cs = ((q + 2) & 4) ? -cv : cv;
}

// Box-Muller over two Philox words: r cos(2 pi u2), r sin(2 pi u2) with
// r = sqrt(-2 ln u1), ln as det_gumbel takes it; sqrtf is correctly rounded
// on both sides.
__host__ __device__ inline void det_normal_pair(uint32_t w0, uint32_t w1, float* z0, float* z1) {
#pragma clang fp contract(off)
    const float LN2 = 0.693147182464599609375f;
    const float l = det_log2(u32_to_unit(w0)) * LN2;  // ln u1 < 0
    const float r = __builtin_sqrtf(-2.0f * l);
    float sn, cs;
    det_sincos2pi(u32_to_unit(w1), &sn, &cs);
    *z0 = r * cs;
    *z1 = r * sn;
}

// The four standard normals of columns 4b .. 4b + 3 of env `env` at `step`.
// Counter {env, 0x80000000 | b, step lo, step hi}: bit 31 of word 1 keeps the
// stream apart from the discrete sampler's (sample_uniform: j >> 2 <= 7).
__host__ __device__ inline void cont_normals4(uint32_t k0, uint32_t k1, uint32_t env,
                                              uint64_t step, uint32_t b, float z[4]) {
    u32x4 c;
    c.x = env;
    c.y = 0x80000000u | b;
    c.z = (uint32_t)step;
    c.w = (uint32_t)(step >> 32);
    const u32x4 r = philox4x32(c, k0, k1);
    det_normal_pair(r.x, r.y, &z[0], &z[1]);
    det_normal_pair(r.z, r.w, &z[2], &z[3]);
}

// dists.py:237-238 (library tanh / exp: accurate to a few ulp, not
// bit-identical between host and device)
__host__ __device__ inline float cont_sigmoid(float y) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-(y + 2.0f)));
}
__host__ __device__ inline float cont_std(float sg, float lo, float hi) {
#pragma clang fp contract(off)
    return (hi - lo) * sg + lo;
}
// jax.scipy.stats.norm.logpdf (dists.py:243, 276) from the standardised z
// and ls = ln s
__host__ __device__ inline float cont_logp(float z, float ls) {
#pragma clang fp contract(off)
    return -0.5f * (z * z) - ls - kHalfLn2Pi;
}
// 0.5 ln(2 pi s^2) + 0.5 (dists.py:278)
__host__ __device__ inline float cont_entropy(float ls) {
#pragma clang fp contract(off)
    return ls + kHalfLn2Pi + 0.5f;
}

// sample() / best() of the (up to) four columns e0 .. e0 + cnt of one row from
// their raw means x, raw stds y and normals z (dists.py:223-258): the action
// fmaf(z, s, m) (tanh(mean) for best()) and, with want_lp, its
// log-prob from the standardised (a - m) / s, as action_stats forms it from
// the stored action.
__host__ __device__ inline void cont_sample4(const float x[4], const float y[4], const float z[4],
                                             const mlearn_continuous_layout& lay, int e0, int cnt,
                                             int sample, bool want_lp, float a[4], float lp[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = 0.f;
        lp[j] = 0.f;
        if (j >= cnt) continue;
        const int g = (e0 + j) / lay.num_dims;
        const float m = tanhf(x[j]);
        const float s = cont_std(cont_sigmoid(y[j]), lay.std_min[g], lay.std_max[g]);
        a[j] = sample ? __builtin_fmaf(z[j], s, m) : m;
        if (want_lp) lp[j] = cont_logp((a[j] - m) / s, logf(s));
    }
}

// Element i of an f32 / bf16 array upcast to f32 (dists.py:221); bf16 -> f32
// is a 16-bit shift on either side.
__host__ __device__ inline float cont_load(const void* p, int32_t dtype, int64_t i) {
    if (dtype == MLEARN_DTYPE_F32) return ((const float*)p)[i];
    const uint32_t bits = (uint32_t)((const uint16_t*)p)[i] << 16;
    float v;
    __builtin_memcpy(&v, &bits, 4);
    return v;
}

}  // namespace ml
