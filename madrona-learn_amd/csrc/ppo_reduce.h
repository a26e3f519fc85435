// The flat parameter layout and the fixed-order reduction of split-K slabs and
// column partials into the flat gradient.  Part of ppo.hip's translation unit.
#pragma once

#include "ppo_defs.h"

namespace ml {

// ---------------------------------------------------------------------------
// Fixed-order reduction into the flat gradient.
// ---------------------------------------------------------------------------
LayoutK make_layout(const mlearn_mlp_policy& p) {
    LayoutK k{};
    k.L = p.num_layers;
    k.D = p.obs_dim;
    k.H = p.hidden;
    k.A1 = p.actions.num_logits + p.critic_bins;
    k.HC = head_cols(p);
    int64_t o = 0;
    for (int l = 0; l < k.L; ++l) {
        k.w_off[l] = o;
        o += (int64_t)(l == 0 ? k.D : k.H) * k.H;
        k.s_off[l] = o;
        o += k.H;
        k.b_off[l] = o;
        o += k.H;
    }
    k.hw_off = o;
    o += (int64_t)k.H * k.A1;
    k.hb_off = o;
    o += k.A1;
    k.total = o;
    k.mlp_total = o;
    k.lstm_off = o;
    k.lstm_H = 0;
    return k;
}

LayoutK make_layout_lstm(const mlearn_mlp_policy& p, const mlearn_lstm& r) {
    LayoutK k = make_layout(p);
    const int64_t H = r.hidden;
    k.lstm_H = (int)H;
    k.lstm_off = (k.mlp_total + 63) / 64 * 64;
    k.total = k.lstm_off + 8 * H * H + 4 * H;
    return k;
}

// Fixed-order reduction of the split-K slabs and column partials into the
// flat gradient.  A block owns 64 consecutive parameters (every segment of
// the flat layout but the head bias is a multiple of 64 long): 16 column
// threads x 16 split groups; group g sums splits g, g + 16, ... and the
// groups are combined in order through LDS.
constexpr int kRgGroups = 16;
// v += ld(k) for k = g, g + 16, ... < n, in that order, with four loads in
// flight (a plain loop waits for each load before issuing the next)
template <typename F>
__device__ inline void rg_sum4(float (&v)[4], int g, int n, F ld) {
    for (int k0 = g; k0 < n; k0 += 4 * kRgGroups) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k0 + u * kRgGroups < n) x[u] = ld(k0 + u * kRgGroups);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k0 + u * kRgGroups < n) {
                v[0] += x[u].x;
                v[1] += x[u].y;
                v[2] += x[u].z;
                v[3] += x[u].w;
            }
    }
}
__global__ __launch_bounds__(256) void reduce_grads_kernel(LayoutK Lk, WsK ws, float* grad,
                                                           double* sumsq) {
    __shared__ float red[kRgGroups][65];
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int H = Lk.H, L = Lk.L;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (Lk.lstm_H && p0 >= Lk.lstm_off) {  // LSTM segment (64-aligned)
        const int64_t q0 = p0 - Lk.lstm_off, HH = Lk.lstm_H, G = 4 * HH * HH;
        if (q0 >= 2 * G) {  // bias: column partials of d gate pre-activations
            const int col = L * 2 * H + Lk.HC + (int)(q0 - 2 * G) + 4 * c;
            rg_sum4(v, g, kColChunks,
                    [&](int k) { return *(const float4*)(ws.colpart2 + (int64_t)k * ws.CP + col); });
        } else {  // Wi / Wh: split-K slabs [split][H][4H]
            const int which = (int)(q0 / G);
            const float* sp = ws.slab + ws.slab_off[L + 1 + which] + (q0 - which * G) + 4 * c;
            rg_sum4(v, g, ws.splits[L + 1 + which],
                    [&](int k) { return *(const float4*)(sp + (int64_t)k * G); });
        }
    } else if (p0 >= Lk.hw_off) {  // head weight (slab [split][H][32]) and head bias
        // per parameter e: a strided sequence (base, stride, n) summed in
        // order; the four parameters' loads are issued together
        const float* base[4];
        int64_t stride[4];
        int n[4];
        int nmax = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t p = p0 + 4 * c + e;
            base[e] = ws.colpart2;
            stride[e] = 0;
            n[e] = 0;
            if (p >= Lk.mlp_total) continue;  // (recurrent policies: alignment padding)
            if (p >= Lk.hb_off) {
                base[e] = ws.colpart2 + L * 2 * H + (int)(p - Lk.hb_off);
                stride[e] = ws.CP;
                n[e] = kColChunks;
            } else {
                const int64_t q = p - Lk.hw_off;
                const int i = (int)(q / Lk.A1), j = (int)(q % Lk.A1);
                base[e] = ws.slab + ws.slab_off[L] + (int64_t)i * Lk.HC + j;
                stride[e] = (int64_t)H * Lk.HC;
                n[e] = ws.splits[L];
            }
            nmax = n[e] > nmax ? n[e] : nmax;
        }
        for (int k0 = g; k0 < nmax; k0 += 4 * kRgGroups) {
            float x[4][4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + u * kRgGroups;
                    x[e][u] = k < n[e] ? base[e][k * stride[e]] : 0.f;
                }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (k0 + u * kRgGroups < n[e]) v[e] += x[e][u];
        }
    } else {
        int l = L - 1;
        while (l > 0 && p0 < Lk.w_off[l]) --l;
        if (p0 >= Lk.s_off[l]) {  // LayerNorm scale / bias: column partials
            const int which = p0 >= Lk.b_off[l] ? 0 : 1;  // 0: bias (beta), 1: scale (gamma)
            const int col = (l * 2 + which) * H + (int)(p0 - (which ? Lk.s_off[l] : Lk.b_off[l])) + 4 * c;
            rg_sum4(v, g, kColChunks,
                    [&](int k) { return *(const float4*)(ws.colpart2 + (int64_t)k * ws.CP + col); });
        } else {  // Dense kernel: split-K slabs
            const int I = l == 0 ? Lk.D : H;
            const float* sp = ws.slab + ws.slab_off[l] + (p0 - Lk.w_off[l]) + 4 * c;
            const int64_t stride = (int64_t)I * H;
            rg_sum4(v, g, ws.splits[l], [&](int k) { return *(const float4*)(sp + k * stride); });
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[g][4 * c + e] = v[e];
    __syncthreads();
    if (threadIdx.x < 64) {  // wave 0
        const int64_t p = p0 + threadIdx.x;
        float t = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kRgGroups; ++k) t += red[k][threadIdx.x];
        if (p < Lk.total) grad[p] = t;
        if (sumsq) {  // this block's partial of the clip_by_global_norm sum (ppo.py:84-90)
            const double q = p < Lk.total ? (double)t * (double)t : 0.0;
            const double w = wave_sum64d(q);
            if (threadIdx.x == 0) sumsq[blockIdx.x] = w;
        }
    }
}

}  // namespace ml
