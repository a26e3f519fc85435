// Entity self-attention core for gfx950: out = softmax(scale * q k^T) v over
// tiny problems (seq <= 32 entities, head_dim 16/32/64), one problem per
// (batch row, head), forward and exact backward.
//
// One wave owns one problem and every output slice of it: no atomics, no
// cross-workgroup reduction, bit-deterministic.  A workgroup is four such
// waves that never synchronise with each other.
//
// All products are 32x32 MFMA tiles (bf16 32x32x16, exact-f32 32x32x2), rows
// and key/query positions beyond seq zero-filled:
//   first level   W[a][b] = sum_c X[a][c] Y[b][c]   (c = channel)
//       Both operands are "row on the lane" fragments: lane (r, h) holds a
//       run of channels of row r, loaded straight from HBM with 16-byte
//       loads.  The same registers serve as the A operand (rows of W) and as
//       the B operand (columns of W), so S = q k^T and S^T = k q^T cost one
//       set of loads.  The channel -> (k-step, lane half) order is free as
//       long as both operands share it: bf16 uses the natural one, f32 gives
//       lane half h the contiguous half [h D/2, (h+1) D/2) of the row.
//   second level  Y^T[c][b] = sum_a Z[a][c] X[a][b]
//       X is a first-level accumulator (row a in the 16 registers, column b
//       on the lane) used as the B operand with no lane movement; register t
//       of lane half h is row acc_row(t) = (t&3) + 8(t>>2) + 4h, so the A
//       operand's k order follows that permutation.  Z^T is gathered from a
//       row-major LDS image of Z (the only LDS use: one transpose per
//       second-level product, private to the wave).
// Forward:  S^T = k q^T (keys in registers, query on the lane), softmax over a
//   lane's 16 registers plus one exchange with the other lane half,
//   O^T = v^T P^T.
// Backward: both orientations are recomputed (the problem is HBM-bound, the
//   extra MFMAs are free): P, dS with the query in registers feed
//   dV^T = dO^T P and dK^T = q^T dS; dS^T with the key in registers feeds
//   dQ^T = k^T dS^T.
//
// f32 problems of seq <= 16 run the same scheme on 16x16 tiles (16x16x4 f32
// MFMA, a quarter of the cycles; second half of this file).
//
// bf16: P and dS are rounded to bf16 only as MFMA operands, statistics and
// accumulation are f32, outputs are rounded once on store.  f32: the f32 MFMA
// (a k-ordered fmaf chain), never through bf16.
#include <math.h>

#include "common.h"

namespace ml {
namespace {

constexpr int kAttnWaves = 4;

// A problem row's channels as one lane's first-level fragment.
template <typename T, int D> struct RowFrag;

template <int D> struct RowFrag<bf16, D> {
    static constexpr int NV = D / 16;
    static constexpr int PAD = 8;  // LDS row padding (elements): 16 bytes
    bf16x8 v[NV];                  // v[s][e] = channel 16 s + 8 h + e

    __device__ void load(const bf16* row, bool valid, int h) {
#pragma unroll
        for (int s = 0; s < NV; ++s) {
            uint4 u = make_uint4(0, 0, 0, 0);
            if (valid) u = *(const uint4*)(row + 16 * s + 8 * h);
            v[s] = __builtin_bit_cast(bf16x8, u);
        }
    }
    __device__ void store_lds(bf16* row, int h) const {
#pragma unroll
        for (int s = 0; s < NV; ++s) *(bf16x8*)(row + 16 * s + 8 * h) = v[s];
    }
    __device__ static f32x16 mma(const RowFrag& a, const RowFrag& b, f32x16 c) {
#pragma unroll
        for (int s = 0; s < NV; ++s)
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[s], b.v[s], c, 0, 0, 0);
        return c;
    }
};

template <int D> struct RowFrag<float, D> {
    static constexpr int NV = D / 8;
    static constexpr int PAD = 4;
    f32x4 v[NV];  // v[u][e] = channel h D/2 + 4 u + e

    __device__ void load(const float* row, bool valid, int h) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (valid) x = *(const f32x4*)(row + h * (D / 2) + 4 * u);
            v[u] = x;
        }
    }
    __device__ void store_lds(float* row, int h) const {
#pragma unroll
        for (int u = 0; u < NV; ++u) *(f32x4*)(row + h * (D / 2) + 4 * u) = v[u];
    }
    __device__ static f32x16 mma(const RowFrag& a, const RowFrag& b, f32x16 c) {
#pragma unroll
        for (int u = 0; u < NV; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[u][e], b.v[u][e], c, 0, 0, 0);
        return c;
    }
};

// Second level: Y^T[c][b] = sum_a Z[a][c] X[a][b] for the 32 channels
// c = 32 tile + r of the LDS image z[a][LD]; channels >= D contribute zero rows.
template <int D, int LD>
__device__ inline f32x16 acc_product(const bf16* z, const f32x16& x, int tile, int r, int h) {
    const bool cv = 32 * tile + r < D;
    f32x16 c = {};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        bf16x8 fa, fb;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int a = (e & 3) + 8 * (2 * s + (e >> 2)) + 4 * h;  // acc row of register 8 s + e
            fa[e] = cv ? z[a * LD + 32 * tile + r] : (bf16)0.f;
            fb[e] = (bf16)x[8 * s + e];
        }
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, c, 0, 0, 0);
    }
    return c;
}

template <int D, int LD>
__device__ inline f32x16 acc_product(const float* z, const f32x16& x, int tile, int r, int h) {
    const bool cv = 32 * tile + r < D;
    f32x16 c = {};
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int a = (t & 3) + 8 * (t >> 2) + 4 * h;
        const float fa = cv ? z[a * LD + 32 * tile + r] : 0.f;
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, x[t], c, 0, 0, 0);
    }
    return c;
}

__device__ inline void store4(bf16* p, float a, float b, float c, float d) {
    typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
    bf16x4 o;
    o[0] = (bf16)a;
    o[1] = (bf16)b;
    o[2] = (bf16)c;
    o[3] = (bf16)d;
    *(bf16x4*)p = o;
}
__device__ inline void store4(float* p, float a, float b, float c, float d) {
    f32x4 o = {a, b, c, d};
    *(f32x4*)p = o;
}

// Y[b = r][32 tile + ...] = mul * Y^T tile; registers 4 g .. 4 g + 3 are four
// consecutive channels 32 tile + 8 g + 4 h + (0..3) of column r.
template <typename T, int D>
__device__ inline void store_tile(T* row, bool valid, const f32x16& y, float mul, int tile, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c0 = 32 * tile + 8 * g + 4 * h;
        if (valid && c0 < D)
            store4(row + c0, y[4 * g] * mul, y[4 * g + 1] * mul, y[4 * g + 2] * mul,
                   y[4 * g + 3] * mul);
    }
}

// LDS ops of one wave execute in order; this only keeps the compiler from
// moving a transposed read across the image's write (or the next write
// across the reads).
__device__ inline void lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

template <typename T, int D> struct Geo {
    typedef RowFrag<T, D> F;
    static constexpr int LD = D + F::PAD;
    static constexpr int TILES = (D + 31) / 32;
};

template <typename T, int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
    float* __restrict__ lse, int64_t nprob, int seq, int heads, float scale) {
    typedef Geo<T, D> G;
    typedef typename G::F F;
    __shared__ __attribute__((aligned(16))) T lds[kAttnWaves][32 * G::LD];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;  // whole wave; waves never synchronise
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;  // this lane's row (r < seq)
    const bool rv = r < seq;
    T* z = lds[wid];

    F qf, kf, vf;
    qf.load(q + ro, rv, h);
    kf.load(k + ro, rv, h);
    vf.load(v + ro, rv, h);
    vf.store_lds(z + r * G::LD, h);

    // st[t] = S[query r][key acc_row(t)]
    f32x16 st = {};
    st = F::mma(kf, qf, st);
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const float s = acc_row(t, lane) < seq ? st[t] * scale : -INFINITY;
        st[t] = s;
        m = fmaxf(m, s);
    }
    m = fmaxf(m, __shfl_xor(m, 32));  // seq >= 1: finite
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const float e = acc_row(t, lane) < seq ? expf(st[t] - m) : 0.f;
        st[t] = e;
        sum += e;
    }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.f / sum;
#pragma unroll
    for (int t = 0; t < 16; ++t) st[t] *= inv;
    if (rv && h == 0) lse[p * seq + r] = m + logf(sum);

    lds_order();
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile) {
        const f32x16 o = acc_product<D, G::LD>(z, st, tile, r, h);  // O^T[channel][query r]
        store_tile<T, D>(out + ro, rv, o, 1.f, tile, h);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ out, const float* __restrict__ lse, const T* __restrict__ dout,
    T* __restrict__ dq, T* __restrict__ dk, T* __restrict__ dv, int64_t nprob, int seq, int heads,
    float scale) {
    typedef Geo<T, D> G;
    typedef typename G::F F;
    __shared__ __attribute__((aligned(16))) T lds[kAttnWaves][32 * G::LD];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;
    const bool rv = r < seq;
    T* z = lds[wid];

    // per row r (both lane halves hold it): lse_r and D_r = dO_r . O_r, the
    // diagonal of dO O^T from the same MFMA chain as dP = dO V^T, so that the
    // cancellation dP - D sees one summation order (exactly 0 where O_r = V_j).
    // Row r of column r is register (r & 3) + 4 (r >> 3) of lane half (r >> 2) & 1.
    F dof, qf, kf, vf;
    dof.load(dout + ro, rv, h);
    float dl = 0.f;
    {
        F of;
        of.load(out + ro, rv, h);
        f32x16 e = {};
        e = F::mma(dof, of, e);
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (t == (r & 3) + 4 * (r >> 3)) dl = e[t];
    }
    dl = __shfl(dl, r + 32 * ((r >> 2) & 1));
    const float ll = rv ? lse[p * seq + r] : 0.f;
    qf.load(q + ro, rv, h);
    kf.load(k + ro, rv, h);
    vf.load(v + ro, rv, h);

    // query acc_row(t) in the registers, key r on the lane
    f32x16 pm = {}, ds = {};
    {
        f32x16 s = {}, dp = {};
        s = F::mma(qf, kf, s);
        dp = F::mma(dof, vf, dp);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int i = acc_row(t, lane);
            const float li = __shfl(ll, i), di = __shfl(dl, i);
            const float pp = (rv && i < seq) ? expf(s[t] * scale - li) : 0.f;
            pm[t] = pp;
            ds[t] = pp * (dp[t] - di);
        }
    }
    // key acc_row(t) in the registers, query r on the lane
    f32x16 dst = {};
    {
        f32x16 s = {}, dp = {};
        s = F::mma(kf, qf, s);
        dp = F::mma(vf, dof, dp);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float pp = (rv && acc_row(t, lane) < seq) ? expf(s[t] * scale - ll) : 0.f;
            dst[t] = pp * (dp[t] - dl);
        }
    }

    // dV^T[c][key r] = sum_i dO[i][c] P[i][r]
    dof.store_lds(z + r * G::LD, h);
    lds_order();
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile)
        store_tile<T, D>(dv + ro, rv, acc_product<D, G::LD>(z, pm, tile, r, h), 1.f, tile, h);
    // dK^T[c][key r] = scale sum_i q[i][c] dS[i][r]
    lds_order();
    qf.store_lds(z + r * G::LD, h);
    lds_order();
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile)
        store_tile<T, D>(dk + ro, rv, acc_product<D, G::LD>(z, ds, tile, r, h), scale, tile, h);
    // dQ^T[c][query r] = scale sum_j k[j][c] dS^T[j][r]
    lds_order();
    kf.store_lds(z + r * G::LD, h);
    lds_order();
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile)
        store_tile<T, D>(dq + ro, rv, acc_product<D, G::LD>(z, dst, tile, r, h), scale, tile, h);
}

// ---------------------------------------------------------------------------
// f32 with seq <= 16: the same scheme on 16x16 tiles of v_mfma_f32_16x16x4_f32
// (a quarter of the 32x32x2 form's cycles per problem; the f32 forms run at
// 1/16 of the bf16 MFMA rate, so at small seq the 32x32 tiles' padding is what
// the f32 kernel spends its time on).  Lane l: r = l & 15, g = l >> 4;
// A[row r][k = g], B[k = g][col r]; accumulator register t = row 4 g + t of
// column r.  Lane group g holds the contiguous channel quarter
// [g D/4, (g+1) D/4) of its row.
// ---------------------------------------------------------------------------
template <int D> struct RowFrag16 {
    static constexpr int NV = D / 16;
    static constexpr int LD = D + 4;  // LDS row: 16 bytes of padding
    f32x4 v[NV];                      // v[u][e] = channel g D/4 + 4 u + e

    __device__ void load(const float* row, bool valid, int g) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (valid) x = *(const f32x4*)(row + g * (D / 4) + 4 * u);
            v[u] = x;
        }
    }
    __device__ void store_lds(float* row, int g) const {
#pragma unroll
        for (int u = 0; u < NV; ++u) *(f32x4*)(row + g * (D / 4) + 4 * u) = v[u];
    }
    __device__ static f32x4 mma(const RowFrag16& a, const RowFrag16& b, f32x4 c) {
#pragma unroll
        for (int u = 0; u < NV; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[u][e], b.v[u][e], c, 0, 0, 0);
        return c;
    }
    // Y^T[16 tile + ..][b] = sum_a Z[a][c] X[a][b] from the LDS image z, stored
    // as Y[b = r][16 tile + 4 g + (0..3)] * mul
    __device__ static void product_store(const float* z, const f32x4& x, float* row, bool valid,
                                         float mul, int r, int g) {
#pragma unroll
        for (int tile = 0; tile < D / 16; ++tile) {
            f32x4 c = {};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(z[(4 * g + t) * LD + 16 * tile + r], x[t],
                                                         c, 0, 0, 0);
            if (valid) store4(row + 16 * tile + 4 * g, c[0] * mul, c[1] * mul, c[2] * mul, c[3] * mul);
        }
    }
};

__device__ inline float max16(float m) {  // over the four lane groups of a column
    m = fmaxf(m, __shfl_xor(m, 16));
    return fmaxf(m, __shfl_xor(m, 32));
}
__device__ inline float sum16(float s) {
    s += __shfl_xor(s, 16);
    return s + __shfl_xor(s, 32);
}

template <int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_fwd16_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    float* __restrict__ out, float* __restrict__ lse, int64_t nprob, int seq, int heads,
    float scale) {
    typedef RowFrag16<D> F;
    __shared__ __attribute__((aligned(16))) float lds[kAttnWaves][16 * F::LD];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;
    const bool rv = r < seq;
    float* z = lds[wid];

    F qf, kf, vf;
    qf.load(q + ro, rv, g);
    kf.load(k + ro, rv, g);
    vf.load(v + ro, rv, g);
    vf.store_lds(z + r * F::LD, g);

    f32x4 st = {};
    st = F::mma(kf, qf, st);  // st[t] = S[query r][key 4 g + t]
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float s = 4 * g + t < seq ? st[t] * scale : -INFINITY;
        st[t] = s;
        m = fmaxf(m, s);
    }
    m = max16(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float e = 4 * g + t < seq ? expf(st[t] - m) : 0.f;
        st[t] = e;
        sum += e;
    }
    sum = sum16(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int t = 0; t < 4; ++t) st[t] *= inv;
    if (rv && g == 0) lse[p * seq + r] = m + logf(sum);

    lds_order();
    F::product_store(z, st, out + ro, rv, 1.f, r, g);  // O^T = v^T P^T
}

template <int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_bwd16_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ dout,
    float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv, int64_t nprob, int seq,
    int heads, float scale) {
    typedef RowFrag16<D> F;
    __shared__ __attribute__((aligned(16))) float lds[kAttnWaves][16 * F::LD];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;
    const bool rv = r < seq;
    float* z = lds[wid];

    // D_r: row r of column r of dO O^T is register r & 3 of lane group r >> 2
    F dof, qf, kf, vf;
    dof.load(dout + ro, rv, g);
    float dl = 0.f;
    {
        F of;
        of.load(out + ro, rv, g);
        f32x4 e = {};
        e = F::mma(dof, of, e);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t == (r & 3)) dl = e[t];
    }
    dl = __shfl(dl, r + 16 * (r >> 2));
    const float ll = rv ? lse[p * seq + r] : 0.f;
    qf.load(q + ro, rv, g);
    kf.load(k + ro, rv, g);
    vf.load(v + ro, rv, g);

    // query 4 g + t in the registers, key r on the lane
    f32x4 pm = {}, ds = {};
    {
        f32x4 s = {}, dp = {};
        s = F::mma(qf, kf, s);
        dp = F::mma(dof, vf, dp);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * g + t;
            const float li = __shfl(ll, i), di = __shfl(dl, i);
            const float pp = (rv && i < seq) ? expf(s[t] * scale - li) : 0.f;
            pm[t] = pp;
            ds[t] = pp * (dp[t] - di);
        }
    }
    // key 4 g + t in the registers, query r on the lane
    f32x4 dst = {};
    {
        f32x4 s = {}, dp = {};
        s = F::mma(kf, qf, s);
        dp = F::mma(vf, dof, dp);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float pp = (rv && 4 * g + t < seq) ? expf(s[t] * scale - ll) : 0.f;
            dst[t] = pp * (dp[t] - dl);
        }
    }

    dof.store_lds(z + r * F::LD, g);
    lds_order();
    F::product_store(z, pm, dv + ro, rv, 1.f, r, g);  // dV^T = dO^T P
    lds_order();
    qf.store_lds(z + r * F::LD, g);
    lds_order();
    F::product_store(z, ds, dk + ro, rv, scale, r, g);  // dK^T = scale q^T dS
    lds_order();
    kf.store_lds(z + r * F::LD, g);
    lds_order();
    F::product_store(z, dst, dq + ro, rv, scale, r, g);  // dQ^T = scale k^T dS^T
}

int check_shape(const char* what, int32_t dtype, int64_t batch, int32_t seq, int32_t heads,
                int32_t head_dim, float scale, int64_t* nprob) {
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d (MLEARN_DTYPE_F32 or MLEARN_DTYPE_BF16)", what, dtype);
    ML_REQUIRE(seq >= 1 && seq <= 32, "%s: seq %d outside 1..32", what, seq);
    ML_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64,
               "%s: head_dim %d (16, 32 or 64)", what, head_dim);
    ML_REQUIRE(heads >= 1 && heads <= 65536, "%s: heads %d outside 1..65536", what, heads);
    ML_REQUIRE(batch >= 1, "%s: batch %lld < 1", what, (long long)batch);
    ML_REQUIRE(isfinite(scale), "%s: scale is not finite", what);
    // one wave per (batch, head); kAttnWaves per workgroup, grid.x < 2^31
    ML_REQUIRE(batch <= (((int64_t)1 << 31) - 1) * kAttnWaves / heads,
               "%s: batch %lld x heads %d exceeds one launch", what, (long long)batch, heads);
    *nprob = batch * heads;
    return MLEARN_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int launch_fwd(const void* q, const void* k, const void* v, int64_t nprob, int32_t seq,
               int32_t heads, int32_t head_dim, float scale, void* out, float* lse,
               hipStream_t st) {
    const dim3 grid((unsigned)((nprob + kAttnWaves - 1) / kAttnWaves)), block(kAttnWaves * kWave);
    (void)hipGetLastError();  // check_launch reports this launch, not an earlier call's error
#define ML_ATTN_FWD(DD)                                                                       \
    hipLaunchKernelGGL((attn_fwd_kernel<T, DD>), grid, block, 0, st, (const T*)q, (const T*)k, \
                       (const T*)v, (T*)out, lse, nprob, seq, heads, scale)
#define ML_ATTN_FWD16(DD)                                                                   \
    hipLaunchKernelGGL((attn_fwd16_kernel<DD>), grid, block, 0, st, (const float*)q,       \
                       (const float*)k, (const float*)v, (float*)out, lse, nprob, seq, heads, \
                       scale)
    if (sizeof(T) == 4 && seq <= 16) {  // f32: 16x16 tiles
        if (head_dim == 16) ML_ATTN_FWD16(16);
        else if (head_dim == 32) ML_ATTN_FWD16(32);
        else ML_ATTN_FWD16(64);
    } else if (head_dim == 16) ML_ATTN_FWD(16);
    else if (head_dim == 32) ML_ATTN_FWD(32);
    else ML_ATTN_FWD(64);
#undef ML_ATTN_FWD16
#undef ML_ATTN_FWD
    return check_launch("attention_fwd");
}

template <typename T>
int launch_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse,
               const void* dout, int64_t nprob, int32_t seq, int32_t heads, int32_t head_dim,
               float scale, void* dq, void* dk, void* dv, hipStream_t st) {
    const dim3 grid((unsigned)((nprob + kAttnWaves - 1) / kAttnWaves)), block(kAttnWaves * kWave);
    (void)hipGetLastError();  // check_launch reports this launch, not an earlier call's error
#define ML_ATTN_BWD(DD)                                                                       \
    hipLaunchKernelGGL((attn_bwd_kernel<T, DD>), grid, block, 0, st, (const T*)q, (const T*)k, \
                       (const T*)v, (const T*)out, lse, (const T*)dout, (T*)dq, (T*)dk, (T*)dv, \
                       nprob, seq, heads, scale)
#define ML_ATTN_BWD16(DD)                                                                    \
    hipLaunchKernelGGL((attn_bwd16_kernel<DD>), grid, block, 0, st, (const float*)q,        \
                       (const float*)k, (const float*)v, (const float*)out, lse,            \
                       (const float*)dout, (float*)dq, (float*)dk, (float*)dv, nprob, seq, heads, \
                       scale)
    if (sizeof(T) == 4 && seq <= 16) {  // f32: 16x16 tiles
        if (head_dim == 16) ML_ATTN_BWD16(16);
        else if (head_dim == 32) ML_ATTN_BWD16(32);
        else ML_ATTN_BWD16(64);
    } else if (head_dim == 16) ML_ATTN_BWD(16);
    else if (head_dim == 32) ML_ATTN_BWD(32);
    else ML_ATTN_BWD(64);
#undef ML_ATTN_BWD16
#undef ML_ATTN_BWD
    return check_launch("attention_bwd");
}

}  // namespace
}  // namespace ml

extern "C" {

int mlearn_attention_fwd(const void* q, const void* k, const void* v, int32_t dtype, int64_t batch,
                         int32_t seq, int32_t heads, int32_t head_dim, float scale, void* out,
                         float* lse, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(q && k && v && out && lse, "attention_fwd: null pointer");
    int64_t nprob = 0;
    if (int rc = check_shape("attention_fwd", dtype, batch, seq, heads, head_dim, scale, &nprob))
        return rc;
    ML_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out),
               "attention_fwd: q, k, v, out must be 16-byte aligned");
    if (dtype == MLEARN_DTYPE_BF16)
        return launch_fwd<bf16>(q, k, v, nprob, seq, heads, head_dim, scale, out, lse, S(stream));
    return launch_fwd<float>(q, k, v, nprob, seq, heads, head_dim, scale, out, lse, S(stream));
}

int mlearn_attention_bwd(const void* q, const void* k, const void* v, const void* out,
                         const float* lse, const void* dout, int32_t dtype, int64_t batch,
                         int32_t seq, int32_t heads, int32_t head_dim, float scale, void* dq,
                         void* dk, void* dv, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(q && k && v && out && lse && dout && dq && dk && dv, "attention_bwd: null pointer");
    int64_t nprob = 0;
    if (int rc = check_shape("attention_bwd", dtype, batch, seq, heads, head_dim, scale, &nprob))
        return rc;
    ML_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) &&
                   aligned16(dq) && aligned16(dk) && aligned16(dv),
               "attention_bwd: q, k, v, out, dout, dq, dk, dv must be 16-byte aligned");
    if (dtype == MLEARN_DTYPE_BF16)
        return launch_bwd<bf16>(q, k, v, out, lse, dout, nprob, seq, heads, head_dim, scale, dq, dk,
                                dv, S(stream));
    return launch_bwd<float>(q, k, v, out, lse, dout, nprob, seq, heads, head_dim, scale, dq, dk,
                             dv, S(stream));
}

}  // extern "C"
