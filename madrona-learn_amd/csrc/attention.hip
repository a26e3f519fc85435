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
//
// The pooled form (mean over the queries folded in) keeps the fragments and
// tile forms and never forms O or a dO.
//
// The long form (seq 33..128, last kernels of this file) splits one problem
// over the ceil(seq / 32) waves of a workgroup: NT x NT tiles of the same
// forms, operands staged once in LDS, one writer per output row.
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
// c continues a chain over several 32-row blocks a (the long form below).
template <int D, int LD>
__device__ inline f32x16 acc_product(const bf16* z, const f32x16& x, int tile, int r, int h,
                                     f32x16 c = {}) {
    const bool cv = 32 * tile + r < D;
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
__device__ inline f32x16 acc_product(const float* z, const f32x16& x, int tile, int r, int h,
                                     f32x16 c = {}) {
    const bool cv = 32 * tile + r < D;
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

// ---------------------------------------------------------------------------
// Pooled form: pooled = mean_q O[q,:] = pbar V with pbar[k] = (1/S) sum_q P[q,k],
// the only thing EntitySelfAttentionNet keeps of O.  O itself, a [B,S,H,D] dO
// and the second-level product O^T = v^T P^T are never formed.
//   forward   S^T = k q^T and the softmax as above (keys in the registers, the
//       query on the lane); padded query lanes are set to exactly 0, then the
//       probability registers are summed over the query lanes by a fixed xor
//       butterfly (every lane ends with the same bits) and divided by S.
//       pbar V is a matrix-vector product and stays on the VALU: lane (r, h)
//       sums its half's 16 keys for channel 32 tile + r from the LDS image of
//       v (consecutive lanes, consecutive channels: conflict-free), one
//       exchange with the other half.  pbar is never rounded to bf16.
//   backward  g = d pooled [D].  dP[q,k] = u[k] = (1/S) g . v[k,:] for every q,
//       so dV[k,:] = pbar[k] g is an outer product written from the key's lane
//       in the RowFrag layout, and only dQ and dK stay matrix products:
//       u[k]: lane-local over the key's RowFrag, one exchange; to LDS.
//       key in the registers (S^T): u per register from LDS (16-byte reads,
//         registers 4 j .. 4 j + 3 are four consecutive keys), D_q = sum_k
//         P[q,k] u[k] lane-local plus one exchange, dS^T = P^T (u - D_q)
//         -> dQ^T = k^T dS^T; D_q and lse_q to LDS.
//       query in the registers (S): lse and D per register from LDS, u of the
//         lane's key, dS = P (u - D) -> dK^T = q^T dS; pbar[k] = the lane's
//         register sum plus one exchange -> dV.
//       u and D reach both orientations with the same bits, and a row that
//       attends to one key has D_q = 1 * u[k] + 0 + ... = u[k] exactly: dS = 0
//       (dq = dk = 0 exactly at seq 1).
// LDS per wave: the row-major image (v; then k, then q) and 3 x 32 floats for
// u, D and lse.  Every sum has a fixed order: identical bits on every call.
// ---------------------------------------------------------------------------
constexpr int kXch = 96;  // u [0,32), D [32,64), lse [64,96)

// s * scale - l with the product rounded on its own (never contracted into an
// fma): at seq 1 the backward then recomputes P = expf(0) = 1 from the forward's
// lse = round(s * scale), and the forward's max is that same rounded product.
__device__ inline float logit(float s, float scale, float l) {
#pragma clang fp contract(off)
    return s * scale - l;
}

template <int D> __device__ inline float frag_dot(const RowFrag<bf16, D>& a, const RowFrag<bf16, D>& b) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < RowFrag<bf16, D>::NV; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf((float)a.v[s][e], (float)b.v[s][e], acc);
    return acc;
}
template <int D> __device__ inline float frag_dot(const RowFrag<float, D>& a, const RowFrag<float, D>& b) {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < RowFrag<float, D>::NV; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(a.v[u][e], b.v[u][e], acc);
    return acc;
}
// row[this lane's channels] = mul * a, in the fragment's own layout
template <int D> __device__ inline void frag_store_scaled(bf16* row, const RowFrag<bf16, D>& a, float mul, int h) {
#pragma unroll
    for (int s = 0; s < RowFrag<bf16, D>::NV; ++s) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)a.v[s][e] * mul);
        *(bf16x8*)(row + 16 * s + 8 * h) = o;
    }
}
template <int D> __device__ inline void frag_store_scaled(float* row, const RowFrag<float, D>& a, float mul, int h) {
#pragma unroll
    for (int u = 0; u < RowFrag<float, D>::NV; ++u) *(f32x4*)(row + h * (D / 2) + 4 * u) = a.v[u] * mul;
}

template <typename T, int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_pooled_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    T* __restrict__ pooled, float* __restrict__ lse, int64_t nprob, int seq, int heads,
    float scale) {
    typedef Geo<T, D> G;
    typedef typename G::F F;
    __shared__ __attribute__((aligned(16))) T lds[kAttnWaves][32 * G::LD];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;  // whole wave; waves never synchronise
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;
    const bool rv = r < seq;
    T* z = lds[wid];

    F qf, kf, vf;
    qf.load(q + ro, rv, h);
    kf.load(k + ro, rv, h);
    vf.load(v + ro, rv, h);
    vf.store_lds(z + r * G::LD, h);  // all 32 rows: padded keys are zero rows

    // st[t] = S[query r][key acc_row(t)]
    f32x16 st = {};
    st = F::mma(kf, qf, st);
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const float s = acc_row(t, lane) < seq ? logit(st[t], scale, 0.f) : -INFINITY;
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
    if (rv && h == 0) lse[p * seq + r] = m + logf(sum);

    // pbar[key acc_row(t)] = (1/S) sum over the real query lanes, same bits on
    // every lane of the half; a padded query (uniform over the real keys) adds 0
    const float fs = (float)seq;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        float x = rv ? st[t] * inv : 0.f;
#pragma unroll
        for (int d = 1; d < 32; d *= 2) x += __shfl_xor(x, d);
        st[t] = x / fs;
    }

    lds_order();
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile) {
        const int c = 32 * tile + r;
        float acc = 0.f;
        if (c < D) {
#pragma unroll
            for (int t = 0; t < 16; ++t)
                acc = fmaf(st[t], (float)z[acc_row(t, lane) * G::LD + c], acc);
        }
        acc += __shfl_xor(acc, 32);
        if (h == 0 && c < D) pooled[p * D + c] = (T)acc;
    }
}

template <typename T, int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_pooled_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const float* __restrict__ lse, const T* __restrict__ dpooled, T* __restrict__ dq,
    T* __restrict__ dk, T* __restrict__ dv, int64_t nprob, int seq, int heads, float scale) {
    typedef Geo<T, D> G;
    typedef typename G::F F;
    __shared__ __attribute__((aligned(16))) T lds[kAttnWaves][32 * G::LD];
    __shared__ __attribute__((aligned(16))) float xch[kAttnWaves][kXch];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;
    const bool rv = r < seq;
    T* z = lds[wid];
    float* xu = xch[wid];
    float* xd = xu + 32;
    float* xl = xu + 64;
    const float fs = (float)seq;

    F gf, qf, kf, vf;
    gf.load(dpooled + p * D, true, h);  // every lane: its channels of g
    qf.load(q + ro, rv, h);
    kf.load(k + ro, rv, h);
    vf.load(v + ro, rv, h);
    const float ll = rv ? lse[p * seq + r] : 0.f;

    // u[row r] on both lane halves (0 for a padded key: v's row is zero)
    float u = frag_dot<D>(gf, vf);
    u = (u + __shfl_xor(u, 32)) / fs;
    if (h == 0) {
        xu[r] = u;
        xl[r] = ll;
    }
    kf.store_lds(z + r * G::LD, h);
    lds_order();

    // key acc_row(t) in the registers, query r on the lane
    f32x16 dst = {};
    {
        f32x16 s = {};
        s = F::mma(kf, qf, s);
        f32x4 u4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u4[j] = *(const f32x4*)(xu + 8 * j + 4 * h);
        float dl = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float pp = (rv && acc_row(t, lane) < seq) ? expf(logit(s[t], scale, ll)) : 0.f;
            dst[t] = pp;
            dl = fmaf(pp, u4[t >> 2][t & 3], dl);
        }
        dl += __shfl_xor(dl, 32);
#pragma unroll
        for (int t = 0; t < 16; ++t) dst[t] *= u4[t >> 2][t & 3] - dl;
        if (h == 0) xd[r] = dl;
    }
    // dQ^T[c][query r] = scale sum_j k[j][c] dS^T[j][r]
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile)
        store_tile<T, D>(dq + ro, rv, acc_product<D, G::LD>(z, dst, tile, r, h), scale, tile, h);
    lds_order();
    qf.store_lds(z + r * G::LD, h);
    lds_order();

    // query acc_row(t) in the registers, key r on the lane
    f32x16 ds = {};
    float pbar = 0.f;
    {
        f32x16 s = {};
        s = F::mma(qf, kf, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 l4 = *(const f32x4*)(xl + 8 * j + 4 * h);
            const f32x4 d4 = *(const f32x4*)(xd + 8 * j + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int t = 4 * j + e;
                const float pp =
                    (rv && acc_row(t, lane) < seq) ? expf(logit(s[t], scale, l4[e])) : 0.f;
                pbar += pp;
                ds[t] = pp * (u - d4[e]);
            }
        }
        pbar = (pbar + __shfl_xor(pbar, 32)) / fs;
    }
    // dV[key r][:] = pbar[r] g
    if (rv) frag_store_scaled<D>(dv + ro, gf, pbar, h);
    // dK^T[c][key r] = scale sum_i q[i][c] dS[i][r]
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile)
        store_tile<T, D>(dk + ro, rv, acc_product<D, G::LD>(z, ds, tile, r, h), scale, tile, h);
}

// f32 with seq <= 16 on 16x16 tiles: lane (r = l & 15, g = l >> 4), accumulator
// register t is row 4 g + t of column r, lane group g holds the channel quarter
// [g D/4, (g+1) D/4) of its row.
template <int D> __device__ inline float frag_dot16(const RowFrag16<D>& a, const RowFrag16<D>& b) {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < RowFrag16<D>::NV; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(a.v[u][e], b.v[u][e], acc);
    return acc;
}

template <int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_pooled_fwd16_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    float* __restrict__ pooled, float* __restrict__ lse, int64_t nprob, int seq, int heads,
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
        const float s = 4 * g + t < seq ? logit(st[t], scale, 0.f) : -INFINITY;
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
    if (rv && g == 0) lse[p * seq + r] = m + logf(sum);

    const float fs = (float)seq;
#pragma unroll
    for (int t = 0; t < 4; ++t) {  // pbar[key 4 g + t], over the 16 query lanes of the group
        float x = rv ? st[t] * inv : 0.f;
#pragma unroll
        for (int d = 1; d < 16; d *= 2) x += __shfl_xor(x, d);
        st[t] = x / fs;
    }

    lds_order();
#pragma unroll
    for (int tile = 0; tile < D / 16; ++tile) {
        const int c = 16 * tile + r;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = fmaf(st[t], z[(4 * g + t) * F::LD + c], acc);
        acc = sum16(acc);
        if (g == 0) pooled[p * D + c] = acc;
    }
}

template <int D>
__global__ __launch_bounds__(kAttnWaves* kWave) void attn_pooled_bwd16_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ lse, const float* __restrict__ dpooled, float* __restrict__ dq,
    float* __restrict__ dk, float* __restrict__ dv, int64_t nprob, int seq, int heads,
    float scale) {
    typedef RowFrag16<D> F;
    __shared__ __attribute__((aligned(16))) float lds[kAttnWaves][16 * F::LD];
    __shared__ __attribute__((aligned(16))) float xch[kAttnWaves][kXch];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int64_t p = (int64_t)blockIdx.x * kAttnWaves + wid;
    if (p >= nprob) return;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int64_t ro = ((b * seq + r) * heads + hd) * D;
    const bool rv = r < seq;
    float* z = lds[wid];
    float* xu = xch[wid];
    float* xd = xu + 32;
    float* xl = xu + 64;
    const float fs = (float)seq;

    F gf, qf, kf, vf;
    gf.load(dpooled + p * D, true, g);
    qf.load(q + ro, rv, g);
    kf.load(k + ro, rv, g);
    vf.load(v + ro, rv, g);
    const float ll = rv ? lse[p * seq + r] : 0.f;

    const float u = sum16(frag_dot16<D>(gf, vf)) / fs;  // u[row r] on all four lane groups
    if (g == 0) {
        xu[r] = u;
        xl[r] = ll;
    }
    kf.store_lds(z + r * F::LD, g);
    lds_order();

    // key 4 g + t in the registers, query r on the lane
    f32x4 dst = {};
    {
        f32x4 s = {};
        s = F::mma(kf, qf, s);
        const f32x4 u4 = *(const f32x4*)(xu + 4 * g);
        float dl = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float pp = (rv && 4 * g + t < seq) ? expf(logit(s[t], scale, ll)) : 0.f;
            dst[t] = pp;
            dl = fmaf(pp, u4[t], dl);
        }
        dl = sum16(dl);
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[t] *= u4[t] - dl;
        if (g == 0) xd[r] = dl;
    }
    F::product_store(z, dst, dq + ro, rv, scale, r, g);  // dQ^T = scale k^T dS^T
    lds_order();
    qf.store_lds(z + r * F::LD, g);
    lds_order();

    // query 4 g + t in the registers, key r on the lane
    f32x4 ds = {};
    float pbar = 0.f;
    {
        f32x4 s = {};
        s = F::mma(qf, kf, s);
        const f32x4 l4 = *(const f32x4*)(xl + 4 * g);
        const f32x4 d4 = *(const f32x4*)(xd + 4 * g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float pp = (rv && 4 * g + t < seq) ? expf(logit(s[t], scale, l4[t])) : 0.f;
            pbar += pp;
            ds[t] = pp * (u - d4[t]);
        }
        pbar = sum16(pbar) / fs;
    }
    if (rv) {  // dV[key r][:] = pbar[r] g
#pragma unroll
        for (int w = 0; w < F::NV; ++w) *(f32x4*)(dv + ro + g * (D / 4) + 4 * w) = gf.v[w] * pbar;
    }
    F::product_store(z, ds, dk + ro, rv, scale, r, g);  // dK^T = scale q^T dS
}

// ---------------------------------------------------------------------------
// Long form, seq 33..128: one workgroup of NT = ceil(seq / 32) waves owns one
// (batch row, head) problem; the problem is NT x NT score tiles of the forms
// above.  Wave w stages rows 32 w .. 32 w + 31 of every operand from HBM
// (16-byte loads, once per workgroup) into row-major LDS images of 32 NT rows
// (rows >= seq are zero rows), one __syncthreads, and from then on the waves
// run independently:
//   forward   wave w owns query tile w (its q rows never leave the registers):
//       S^T_j = k_j q^T for every key tile j, k_j a first-level fragment read
//       back from the k image with 16-byte LDS loads -> the whole score row of
//       a query sits in the lane's 16 NT registers and those of the other lane
//       half: an exact two-pass softmax, no online rescaling.  O^T = sum_j
//       v_j^T P_j^T is one MFMA chain over the key tiles (acc_product with the
//       accumulator carried) and is stored once.
//   backward  D_i = dO_i . O_i of the wave's own rows as above (the diagonal of
//       the dO O^T chain: dP - D sees one summation order); D and lse are
//       shared through 2 x 32 NT floats of LDS at the staging barrier.
//       As owner of key tile w (k_w, v_w in the registers) the wave loops over
//       the query tiles i: P_iw, dS_iw with the query in the registers feed
//       the chains dV_w^T += dO_i^T P_iw and dK_w^T += q_i^T dS_iw.  As owner
//       of query tile w (q_w, dO_w in the registers) it loops over the key
//       tiles j: dS_wj^T feeds dQ_w^T += k_j^T dS_wj^T.  Both orientations are
//       recomputed; nothing is transposed through LDS.
// Every output row has one writer and every sum one order: no atomics, no
// cross-wave reduction, identical bits on every call.  LDS: 2 images in the
// forward (k, v), 4 in the backward (q, k, v, dO): at most 68 KiB / 137 KiB
// (f32, head_dim 64, NT 4), dynamic.
// ---------------------------------------------------------------------------
constexpr int kLongMaxSeq = 128;

template <typename T, int D, int NT> struct LongGeo {
    typedef Geo<T, D> G;
    static constexpr int ROWS = 32 * NT;
    static constexpr int IMG = ROWS * G::LD;  // elements of one row image (a multiple of 16 bytes)
    static constexpr int FWD_LDS = 2 * IMG * (int)sizeof(T);
    static constexpr int BWD_LDS = 4 * IMG * (int)sizeof(T) + 2 * ROWS * (int)sizeof(float);
};

template <typename T, int D, int NT>
__global__ __launch_bounds__(NT* kWave) void attn_long_fwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
    float* __restrict__ lse, int seq, int heads, float scale) {
    typedef LongGeo<T, D, NT> L;
    typedef typename L::G G;
    typedef typename G::F F;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* zk = (T*)smem;
    T* zv = zk + L::IMG;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t p = blockIdx.x;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int row = 32 * w + r;  // this lane's query, and the row it stages
    const bool rv = row < seq;
    const int64_t ro = ((b * seq + row) * heads + hd) * D;  // (read and written only where rv)

    F qf;
    qf.load(q + ro, rv, h);
    {
        F xf;
        xf.load(k + ro, rv, h);
        xf.store_lds(zk + row * G::LD, h);
        xf.load(v + ro, rv, h);
        xf.store_lds(zv + row * G::LD, h);
    }
    __syncthreads();

    // st[j][t] = S[query row][key 32 j + acc_row(t)]
    f32x16 st[NT];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        F kf;
        kf.load(zk + (32 * j + r) * G::LD, true, h);
        f32x16 s = {};
        s = F::mma(kf, qf, s);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float x = 32 * j + acc_row(t, lane) < seq ? s[t] * scale : -INFINITY;
            s[t] = x;
            m = fmaxf(m, x);
        }
        st[j] = s;
    }
    m = fmaxf(m, __shfl_xor(m, 32));  // key 0 is real: finite
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const float e = 32 * j + acc_row(t, lane) < seq ? expf(st[j][t] - m) : 0.f;
            st[j][t] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32);
    const float inv = 1.f / sum;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int t = 0; t < 16; ++t) st[j][t] *= inv;
    if (rv && h == 0) lse[p * seq + row] = m + logf(sum);

    // O^T[channel][query row] = sum_j v_j^T P_j^T, one chain over the key tiles
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile) {
        f32x16 o = {};
#pragma unroll
        for (int j = 0; j < NT; ++j)
            o = acc_product<D, G::LD>(zv + 32 * j * G::LD, st[j], tile, r, h, o);
        store_tile<T, D>(out + ro, rv, o, 1.f, tile, h);
    }
}

template <typename T, int D, int NT>
__global__ __launch_bounds__(NT* kWave) void attn_long_bwd_kernel(
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const T* __restrict__ out, const float* __restrict__ lse, const T* __restrict__ dout,
    T* __restrict__ dq, T* __restrict__ dk, T* __restrict__ dv, int seq, int heads, float scale) {
    typedef LongGeo<T, D, NT> L;
    typedef typename L::G G;
    typedef typename G::F F;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* zq = (T*)smem;
    T* zk = zq + L::IMG;
    T* zv = zk + L::IMG;
    T* zd = zv + L::IMG;
    float* xd = (float*)(zd + L::IMG);  // D_i, i < 32 NT
    float* xl = xd + L::ROWS;           // lse_i
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t p = blockIdx.x;
    const int64_t b = p / heads;
    const int hd = (int)(p - b * heads);
    const int row = 32 * w + r;  // this lane's query and key, and the row it stages
    const bool rv = row < seq;
    const int64_t ro = ((b * seq + row) * heads + hd) * D;

    // D of the wave's own rows: the diagonal of dO O^T from the chain that also
    // makes dP = dO V^T (attn_bwd_kernel); 0 for a padded row
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
    const float ll = rv ? lse[p * seq + row] : 0.f;
    qf.load(q + ro, rv, h);
    kf.load(k + ro, rv, h);
    vf.load(v + ro, rv, h);
    qf.store_lds(zq + row * G::LD, h);
    kf.store_lds(zk + row * G::LD, h);
    vf.store_lds(zv + row * G::LD, h);
    dof.store_lds(zd + row * G::LD, h);
    if (h == 0) {
        xd[row] = dl;
        xl[row] = ll;
    }
    __syncthreads();

    // owner of key tile w: key `row` on the lane, query 32 i + acc_row(t) in the
    // registers (registers 4 g .. 4 g + 3 are the four queries 32 i + 8 g + 4 h + ..)
    {
        f32x16 dva[G::TILES], dka[G::TILES];
#pragma unroll
        for (int tile = 0; tile < G::TILES; ++tile) dva[tile] = dka[tile] = f32x16{};
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            F qi, di;
            qi.load(zq + (32 * i + r) * G::LD, true, h);
            di.load(zd + (32 * i + r) * G::LD, true, h);
            f32x16 s = {}, dp = {};
            s = F::mma(qi, kf, s);
            dp = F::mma(di, vf, dp);
            f32x16 pm, ds;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 l4 = *(const f32x4*)(xl + 32 * i + 8 * g + 4 * h);
                const f32x4 d4 = *(const f32x4*)(xd + 32 * i + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = 4 * g + e;
                    const float pp = (rv && 32 * i + acc_row(t, lane) < seq)
                                         ? expf(s[t] * scale - l4[e]) : 0.f;
                    pm[t] = pp;
                    ds[t] = pp * (dp[t] - d4[e]);
                }
            }
#pragma unroll
            for (int tile = 0; tile < G::TILES; ++tile) {
                // dV^T[c][key] += sum_i dO[i][c] P[i][key]; dK^T[c][key] += sum_i q[i][c] dS[i][key]
                dva[tile] = acc_product<D, G::LD>(zd + 32 * i * G::LD, pm, tile, r, h, dva[tile]);
                dka[tile] = acc_product<D, G::LD>(zq + 32 * i * G::LD, ds, tile, r, h, dka[tile]);
            }
        }
#pragma unroll
        for (int tile = 0; tile < G::TILES; ++tile) {
            store_tile<T, D>(dv + ro, rv, dva[tile], 1.f, tile, h);
            store_tile<T, D>(dk + ro, rv, dka[tile], scale, tile, h);
        }
    }

    // owner of query tile w: query `row` on the lane, key 32 j + acc_row(t) in
    // the registers; dQ^T[c][query] = scale sum_j k[j][c] dS^T[j][query]
    {
        f32x16 dqa[G::TILES];
#pragma unroll
        for (int tile = 0; tile < G::TILES; ++tile) dqa[tile] = f32x16{};
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            F kj, vj;
            kj.load(zk + (32 * j + r) * G::LD, true, h);
            vj.load(zv + (32 * j + r) * G::LD, true, h);
            f32x16 s = {}, dp = {};
            s = F::mma(kj, qf, s);
            dp = F::mma(vj, dof, dp);
            f32x16 dst;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float pp = (rv && 32 * j + acc_row(t, lane) < seq)
                                     ? expf(s[t] * scale - ll) : 0.f;
                dst[t] = pp * (dp[t] - dl);
            }
#pragma unroll
            for (int tile = 0; tile < G::TILES; ++tile)
                dqa[tile] = acc_product<D, G::LD>(zk + 32 * j * G::LD, dst, tile, r, h, dqa[tile]);
        }
#pragma unroll
        for (int tile = 0; tile < G::TILES; ++tile)
            store_tile<T, D>(dq + ro, rv, dqa[tile], scale, tile, h);
    }
}

int check_shape(const char* what, int32_t dtype, int64_t batch, int32_t seq, int32_t heads,
                int32_t head_dim, float scale, int64_t* nprob, int32_t seq_lo = 1,
                int32_t seq_hi = 32, int per_wg = kAttnWaves) {
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d (MLEARN_DTYPE_F32 or MLEARN_DTYPE_BF16)", what, dtype);
    ML_REQUIRE(seq >= seq_lo && seq <= seq_hi, "%s: seq %d outside %d..%d", what, seq, seq_lo,
               seq_hi);
    ML_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64,
               "%s: head_dim %d (16, 32 or 64)", what, head_dim);
    ML_REQUIRE(heads >= 1 && heads <= 65536, "%s: heads %d outside 1..65536", what, heads);
    ML_REQUIRE(batch >= 1, "%s: batch %lld < 1", what, (long long)batch);
    ML_REQUIRE(isfinite(scale), "%s: scale is not finite", what);
    // per_wg (batch, head) problems per workgroup, grid.x < 2^31
    ML_REQUIRE(batch <= (((int64_t)1 << 31) - 1) * per_wg / heads,
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

template <typename T>
int launch_pooled_fwd(const void* q, const void* k, const void* v, int64_t nprob, int32_t seq,
                      int32_t heads, int32_t head_dim, float scale, void* pooled, float* lse,
                      hipStream_t st) {
    const dim3 grid((unsigned)((nprob + kAttnWaves - 1) / kAttnWaves)), block(kAttnWaves * kWave);
    (void)hipGetLastError();  // check_launch reports this launch, not an earlier call's error
#define ML_ATTN_PFWD(DD)                                                                   \
    hipLaunchKernelGGL((attn_pooled_fwd_kernel<T, DD>), grid, block, 0, st, (const T*)q,  \
                       (const T*)k, (const T*)v, (T*)pooled, lse, nprob, seq, heads, scale)
#define ML_ATTN_PFWD16(DD)                                                                  \
    hipLaunchKernelGGL((attn_pooled_fwd16_kernel<DD>), grid, block, 0, st, (const float*)q, \
                       (const float*)k, (const float*)v, (float*)pooled, lse, nprob, seq,   \
                       heads, scale)
    if (sizeof(T) == 4 && seq <= 16) {  // f32: 16x16 tiles
        if (head_dim == 16) ML_ATTN_PFWD16(16);
        else if (head_dim == 32) ML_ATTN_PFWD16(32);
        else ML_ATTN_PFWD16(64);
    } else if (head_dim == 16) ML_ATTN_PFWD(16);
    else if (head_dim == 32) ML_ATTN_PFWD(32);
    else ML_ATTN_PFWD(64);
#undef ML_ATTN_PFWD16
#undef ML_ATTN_PFWD
    return check_launch("attention_pooled_fwd");
}

template <typename T>
int launch_pooled_bwd(const void* q, const void* k, const void* v, const float* lse,
                      const void* dpooled, int64_t nprob, int32_t seq, int32_t heads,
                      int32_t head_dim, float scale, void* dq, void* dk, void* dv, hipStream_t st) {
    const dim3 grid((unsigned)((nprob + kAttnWaves - 1) / kAttnWaves)), block(kAttnWaves * kWave);
    (void)hipGetLastError();  // check_launch reports this launch, not an earlier call's error
#define ML_ATTN_PBWD(DD)                                                                   \
    hipLaunchKernelGGL((attn_pooled_bwd_kernel<T, DD>), grid, block, 0, st, (const T*)q,  \
                       (const T*)k, (const T*)v, lse, (const T*)dpooled, (T*)dq, (T*)dk,  \
                       (T*)dv, nprob, seq, heads, scale)
#define ML_ATTN_PBWD16(DD)                                                                  \
    hipLaunchKernelGGL((attn_pooled_bwd16_kernel<DD>), grid, block, 0, st, (const float*)q, \
                       (const float*)k, (const float*)v, lse, (const float*)dpooled,        \
                       (float*)dq, (float*)dk, (float*)dv, nprob, seq, heads, scale)
    if (sizeof(T) == 4 && seq <= 16) {  // f32: 16x16 tiles
        if (head_dim == 16) ML_ATTN_PBWD16(16);
        else if (head_dim == 32) ML_ATTN_PBWD16(32);
        else ML_ATTN_PBWD16(64);
    } else if (head_dim == 16) ML_ATTN_PBWD(16);
    else if (head_dim == 32) ML_ATTN_PBWD(32);
    else ML_ATTN_PBWD(64);
#undef ML_ATTN_PBWD16
#undef ML_ATTN_PBWD
    return check_launch("attention_pooled_bwd");
}

// One workgroup of NT = ceil(seq / 32) waves per problem.  The LDS attribute is
// set once per instantiation and device, kept out of graph capture.
template <typename T, int D, int NT>
int launch_long_fwd_nt(const void* q, const void* k, const void* v, int64_t nprob, int32_t seq,
                       int32_t heads, float scale, void* out, float* lse, hipStream_t st) {
    auto fn = attn_long_fwd_kernel<T, D, NT>;
    constexpr int lds = LongGeo<T, D, NT>::FWD_LDS;
    if (int rc = set_lds_attr((const void*)fn, lds, "attention_long_fwd")) return rc;
    (void)hipGetLastError();  // check_launch reports this launch, not an earlier call's error
    hipLaunchKernelGGL(fn, dim3((unsigned)nprob), dim3(NT * kWave), lds, st, (const T*)q,
                       (const T*)k, (const T*)v, (T*)out, lse, seq, heads, scale);
    return check_launch("attention_long_fwd");
}

template <typename T, int D, int NT>
int launch_long_bwd_nt(const void* q, const void* k, const void* v, const void* out,
                       const float* lse, const void* dout, int64_t nprob, int32_t seq,
                       int32_t heads, float scale, void* dq, void* dk, void* dv, hipStream_t st) {
    auto fn = attn_long_bwd_kernel<T, D, NT>;
    constexpr int lds = LongGeo<T, D, NT>::BWD_LDS;
    if (int rc = set_lds_attr((const void*)fn, lds, "attention_long_bwd")) return rc;
    (void)hipGetLastError();  // check_launch reports this launch, not an earlier call's error
    hipLaunchKernelGGL(fn, dim3((unsigned)nprob), dim3(NT * kWave), lds, st, (const T*)q,
                       (const T*)k, (const T*)v, (const T*)out, lse, (const T*)dout, (T*)dq,
                       (T*)dk, (T*)dv, seq, heads, scale);
    return check_launch("attention_long_bwd");
}

// f<T, D, NT>(args...) for the runtime (head_dim, seq): NT 2, 3 or 4
#define ML_ATTN_LONG_NT(f, DD, ...)                                  \
    (seq <= 64 ? f<T, DD, 2>(__VA_ARGS__)                            \
               : seq <= 96 ? f<T, DD, 3>(__VA_ARGS__) : f<T, DD, 4>(__VA_ARGS__))
#define ML_ATTN_LONG(f, ...)                                         \
    (head_dim == 16 ? ML_ATTN_LONG_NT(f, 16, __VA_ARGS__)            \
                    : head_dim == 32 ? ML_ATTN_LONG_NT(f, 32, __VA_ARGS__) \
                                     : ML_ATTN_LONG_NT(f, 64, __VA_ARGS__))

template <typename T>
int launch_long_fwd(const void* q, const void* k, const void* v, int64_t nprob, int32_t seq,
                    int32_t heads, int32_t head_dim, float scale, void* out, float* lse,
                    hipStream_t st) {
    return ML_ATTN_LONG(launch_long_fwd_nt, q, k, v, nprob, seq, heads, scale, out, lse, st);
}

template <typename T>
int launch_long_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse,
                    const void* dout, int64_t nprob, int32_t seq, int32_t heads, int32_t head_dim,
                    float scale, void* dq, void* dk, void* dv, hipStream_t st) {
    return ML_ATTN_LONG(launch_long_bwd_nt, q, k, v, out, lse, dout, nprob, seq, heads, scale, dq,
                        dk, dv, st);
}
#undef ML_ATTN_LONG
#undef ML_ATTN_LONG_NT

}  // namespace
}  // namespace ml

extern "C" {

int mlearn_attention_long_fwd(const void* q, const void* k, const void* v, int32_t dtype,
                              int64_t batch, int32_t seq, int32_t heads, int32_t head_dim,
                              float scale, void* out, float* lse, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(q && k && v && out && lse, "attention_long_fwd: null pointer");
    int64_t nprob = 0;
    if (int rc = check_shape("attention_long_fwd", dtype, batch, seq, heads, head_dim, scale,
                             &nprob, 33, kLongMaxSeq, 1))
        return rc;
    ML_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out),
               "attention_long_fwd: q, k, v, out must be 16-byte aligned");
    if (dtype == MLEARN_DTYPE_BF16)
        return launch_long_fwd<bf16>(q, k, v, nprob, seq, heads, head_dim, scale, out, lse,
                                     S(stream));
    return launch_long_fwd<float>(q, k, v, nprob, seq, heads, head_dim, scale, out, lse,
                                  S(stream));
}

int mlearn_attention_long_bwd(const void* q, const void* k, const void* v, const void* out,
                              const float* lse, const void* dout, int32_t dtype, int64_t batch,
                              int32_t seq, int32_t heads, int32_t head_dim, float scale, void* dq,
                              void* dk, void* dv, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(q && k && v && out && lse && dout && dq && dk && dv,
               "attention_long_bwd: null pointer");
    int64_t nprob = 0;
    if (int rc = check_shape("attention_long_bwd", dtype, batch, seq, heads, head_dim, scale,
                             &nprob, 33, kLongMaxSeq, 1))
        return rc;
    ML_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) &&
                   aligned16(dq) && aligned16(dk) && aligned16(dv),
               "attention_long_bwd: q, k, v, out, dout, dq, dk, dv must be 16-byte aligned");
    if (dtype == MLEARN_DTYPE_BF16)
        return launch_long_bwd<bf16>(q, k, v, out, lse, dout, nprob, seq, heads, head_dim, scale,
                                     dq, dk, dv, S(stream));
    return launch_long_bwd<float>(q, k, v, out, lse, dout, nprob, seq, heads, head_dim, scale, dq,
                                  dk, dv, S(stream));
}

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

int mlearn_attention_pooled_fwd(const void* q, const void* k, const void* v, int32_t dtype,
                                int64_t batch, int32_t seq, int32_t heads, int32_t head_dim,
                                float scale, void* pooled, float* lse, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(q && k && v && pooled && lse, "attention_pooled_fwd: null pointer");
    int64_t nprob = 0;
    if (int rc = check_shape("attention_pooled_fwd", dtype, batch, seq, heads, head_dim, scale,
                             &nprob))
        return rc;
    ML_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(pooled),
               "attention_pooled_fwd: q, k, v, pooled must be 16-byte aligned");
    if (dtype == MLEARN_DTYPE_BF16)
        return launch_pooled_fwd<bf16>(q, k, v, nprob, seq, heads, head_dim, scale, pooled, lse,
                                       S(stream));
    return launch_pooled_fwd<float>(q, k, v, nprob, seq, heads, head_dim, scale, pooled, lse,
                                    S(stream));
}

int mlearn_attention_pooled_bwd(const void* q, const void* k, const void* v, const float* lse,
                                const void* dpooled, int32_t dtype, int64_t batch, int32_t seq,
                                int32_t heads, int32_t head_dim, float scale, void* dq, void* dk,
                                void* dv, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(q && k && v && lse && dpooled && dq && dk && dv,
               "attention_pooled_bwd: null pointer");
    int64_t nprob = 0;
    if (int rc = check_shape("attention_pooled_bwd", dtype, batch, seq, heads, head_dim, scale,
                             &nprob))
        return rc;
    ML_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(dpooled) &&
                   aligned16(dq) && aligned16(dk) && aligned16(dv),
               "attention_pooled_bwd: q, k, v, dpooled, dq, dk, dv must be 16-byte aligned");
    if (dtype == MLEARN_DTYPE_BF16)
        return launch_pooled_bwd<bf16>(q, k, v, lse, dpooled, nprob, seq, heads, head_dim, scale,
                                       dq, dk, dv, S(stream));
    return launch_pooled_bwd<float>(q, k, v, lse, dpooled, nprob, seq, heads, head_dim, scale, dq,
                                    dk, dv, S(stream));
}

}  // extern "C"
