// Fused LayerNorm + activation of the torch path's trunks (include/mlearn.h
// "LayerNorm + activation"; models.py:46-56 LayerNorm followed by the ReLU of
// MLP or the leaky ReLU of the entity encoder).
//
//   One row per aligned group of G lanes of a 256-thread workgroup (256 / G
//   rows per pass), G by the width F:
//       F <= 128: G 16, 8 elements a lane     F <= 512:  G 64, 8 elements
//       F <= 256: G 32, 8 elements            F <= 1024: G 64, 16 elements
//   A lane owns 16-byte chunks of its row (4 f32 or 8 bf16 columns): chunk
//   sub + k G of the row for k = 0, 1, ...; consecutive lanes read consecutive
//   16 bytes.  The row is read once, held in registers as f32, and its sums
//   are taken across the group by cross-lane shuffles.  Where every base
//   pointer is 16-byte aligned and F and every row stride are multiples of
//   the chunk, a chunk moves as one 16-byte load or store; elsewhere the same
//   lane moves the same columns one element at a time, so the two forms add
//   in one order and give the same bits.  Columns from F on are neither read
//   nor written (they enter the sums as zeros).
//
//   A workgroup walks a contiguous share of the passes, the parameters of
//   its columns in registers.  The backward keeps each lane's partial sums of
//   dscale and dbias in registers over its share, adds the groups of a wave
//   by shuffles and the four waves through LDS, both in a fixed order, and
//   stores one [2][F] partial row; ln_param_sum_kernel adds the partial rows:
//   32 slices of consecutive rows each in index order, then the slices in
//   index order.  No atomics, no counters: dscale and dbias are a function of
//   (rows, F, CU count).
//
// No contraction and no fast-math in this file: with every operation a
// rounded IEEE one, the 16-byte and the element-wise instantiations cannot
// differ.
#pragma clang fp contract(off)
#include "common.h"

namespace ml {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxF = 1024;
constexpr int kMaxParts = 2048;      // partial rows of the workspace at most
constexpr int kSumCols = 8;          // ln_param_sum_kernel: columns per workgroup
constexpr int kSumSlices = kThreads / kSumCols;
constexpr float kLeakySlope = 0.01f;

enum { kActNone = 0, kActRelu = 1, kActLeaky = 2 };

template <typename T> struct Chunk;
template <> struct Chunk<float> { static constexpr int V = 4; };
template <> struct Chunk<bf16> { static constexpr int V = 8; };

__device__ inline float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ inline uint32_t bf16_bits(float v) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (bf16)v);
}

// One chunk of a row as f32: n valid columns (0 <= n <= V) from p on.
template <bool VEC>
__device__ inline void load_chunk(const float* p, int n, float* o) {
    if (VEC) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n > 0) v = *(const f32x4*)p;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = j < n ? p[j] : 0.f;
    }
}

template <bool VEC>
__device__ inline void load_chunk(const bf16* p, int n, float* o) {
    if (VEC) {
        uint4 v = {0u, 0u, 0u, 0u};
        if (n > 0) v = *(const uint4*)p;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[2 * j] = bits_f32(w[j] << 16);
            o[2 * j + 1] = bits_f32(w[j] & 0xffff0000u);
        }
    } else {
        const uint16_t* q = (const uint16_t*)p;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = j < n ? bits_f32((uint32_t)q[j] << 16) : 0.f;
    }
}

template <bool VEC>
__device__ inline void store_chunk(float* p, int n, const float* o) {
    if (VEC) {
        if (n > 0) *(f32x4*)p = f32x4{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) p[j] = o[j];
    }
}

template <bool VEC>
__device__ inline void store_chunk(bf16* p, int n, const float* o) {
    if (VEC) {
        if (n > 0) {
            uint4 v;
            v.x = bf16_bits(o[0]) | (bf16_bits(o[1]) << 16);
            v.y = bf16_bits(o[2]) | (bf16_bits(o[3]) << 16);
            v.z = bf16_bits(o[4]) | (bf16_bits(o[5]) << 16);
            v.w = bf16_bits(o[6]) | (bf16_bits(o[7]) << 16);
            *(uint4*)p = v;
        }
    } else {
        uint16_t* q = (uint16_t*)p;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < n) q[j] = (uint16_t)bf16_bits(o[j]);
    }
}

// Sum over the aligned group of G lanes, the same value in each of them.
template <int G>
__device__ inline float group_sum(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// The rows of pass `it` of this lane's group, its columns' validity and the
// parameters of its columns.
template <typename T, int G, int E>
struct Lane {
    static constexpr int V = Chunk<T>::V, K = E / V, kRows = kThreads / G;
    int grp, sub, nv[K];   // nv[k]: valid columns of chunk k
    int col0[K];           // its first column

    __device__ Lane(int F) {
        grp = threadIdx.x / G;
        sub = threadIdx.x % G;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            col0[k] = (sub + k * G) * V;
            const int left = F - col0[k];
            nv[k] = left < 0 ? 0 : (left > V ? V : left);
        }
    }
    __device__ void params(const float* p, float* o) const {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) o[k * V + j] = j < nv[k] ? p[col0[k] + j] : 0.f;
    }
    template <bool VEC>
    __device__ void load(const T* base, int64_t ld, int64_t row, bool valid, float* o) const {
#pragma unroll
        for (int k = 0; k < K; ++k)
            load_chunk<VEC>(base + row * ld + col0[k], valid ? nv[k] : 0, o + k * V);
    }
    template <bool VEC>
    __device__ void store(T* base, int64_t ld, int64_t row, bool valid, const float* o) const {
#pragma unroll
        for (int k = 0; k < K; ++k)
            store_chunk<VEC>(base + row * ld + col0[k], valid ? nv[k] : 0, o + k * V);
    }
};

// z rounded to T: the pre-activation the module hands to its activation
template <typename T>
__device__ inline float pre_act(float x, float mean, float rstd, float sc, float bi) {
    return rnd<T>((x - mean) * (rstd * sc) + bi);
}

struct Share {
    int64_t passes;      // ceil(rows / rows per pass)
    int64_t per_part;    // passes of one workgroup
    int parts;           // workgroups
};

template <typename T, int G, int E, bool VEC>
__global__ __launch_bounds__(kThreads) void ln_fwd_kernel(
    const T* __restrict__ x, int64_t ldx, const float* __restrict__ scale,
    const float* __restrict__ bias, int64_t rows, int F, float eps, int act, Share sh,
    T* __restrict__ y, int64_t ldy, float* __restrict__ mean, float* __restrict__ rstd) {
    const Lane<T, G, E> ln(F);
    float sc[E], bi[E];
    ln.params(scale, sc);
    ln.params(bias, bi);
    const float Ff = (float)F;
    const int64_t it0 = (int64_t)blockIdx.x * sh.per_part;
    const int64_t it1 = it0 + sh.per_part < sh.passes ? it0 + sh.per_part : sh.passes;
    for (int64_t it = it0; it < it1; ++it) {
        const int64_t row = it * ln.kRows + ln.grp;
        const bool valid = row < rows;
        float xv[E];
        ln.template load<VEC>(x, ldx, row, valid, xv);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            s1 += xv[e];
            s2 += xv[e] * xv[e];
        }
        s1 = group_sum<G>(s1);
        s2 = group_sum<G>(s2);
        const float m = s1 / Ff;
        const float var = fmaxf(s2 / Ff - m * m, 0.f);
        const float r = 1.0f / sqrtf(var + eps);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const float z = pre_act<T>(xv[e], m, r, sc[e], bi[e]);
            float a = z;
            if (act == kActRelu) a = z > 0.f ? z : 0.f;
            if (act == kActLeaky) a = z > 0.f ? z : z * kLeakySlope;
            xv[e] = a;
        }
        ln.template store<VEC>(y, ldy, row, valid, xv);
        if (valid && ln.sub == 0) {
            mean[row] = m;
            rstd[row] = r;
        }
    }
}

template <typename T, int G, int E, bool VEC>
__global__ __launch_bounds__(kThreads) void ln_bwd_kernel(
    const T* __restrict__ x, int64_t ldx, const float* __restrict__ scale,
    const float* __restrict__ bias, const float* __restrict__ mean,
    const float* __restrict__ rstd, const T* __restrict__ dy, int64_t lddy, int64_t rows, int F,
    int act, Share sh, T* __restrict__ dx, int64_t lddx, float* __restrict__ ws) {
    __shared__ float s_part[kWaves][2][G * E];
    const Lane<T, G, E> ln(F);
    float sc[E], bi[E], acc_s[E], acc_b[E];
    ln.params(scale, sc);
    ln.params(bias, bi);
#pragma unroll
    for (int e = 0; e < E; ++e) acc_s[e] = acc_b[e] = 0.f;
    const float Ff = (float)F;
    const int64_t it0 = (int64_t)blockIdx.x * sh.per_part;
    const int64_t it1 = it0 + sh.per_part < sh.passes ? it0 + sh.per_part : sh.passes;
    for (int64_t it = it0; it < it1; ++it) {
        const int64_t row = it * ln.kRows + ln.grp;
        const bool valid = row < rows;
        float xv[E], gv[E];
        ln.template load<VEC>(x, ldx, row, valid, xv);
        ln.template load<VEC>(dy, lddy, row, valid, gv);
        const float m = valid ? mean[row] : 0.f;
        const float r = valid ? rstd[row] : 0.f;
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const float z = pre_act<T>(xv[e], m, r, sc[e], bi[e]);
            const float xh = (xv[e] - m) * r;
            float g = gv[e];
            if (act == kActRelu) g = z > 0.f ? g : 0.f;
            if (act == kActLeaky) g = z > 0.f ? g : g * kLeakySlope;
            acc_b[e] += g;
            acc_s[e] += g * xh;
            const float wg = g * sc[e];
            c1 += wg;
            c2 += wg * xh;
            xv[e] = xh;
            gv[e] = wg;
        }
        c1 = group_sum<G>(c1) / Ff;
        c2 = group_sum<G>(c2) / Ff;
#pragma unroll
        for (int e = 0; e < E; ++e) gv[e] = r * (gv[e] - c1 - xv[e] * c2);
        ln.template store<VEC>(dx, lddx, row, valid, gv);
    }
    // the groups of a wave (lanes sub, sub + G, ...), then the waves in order
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int o = G; o < kWave; o <<= 1) {
            acc_s[e] += __shfl_xor(acc_s[e], o);
            acc_b[e] += __shfl_xor(acc_b[e], o);
        }
    }
    if (lane < G) {
#pragma unroll
        for (int k = 0; k < ln.K; ++k)
#pragma unroll
            for (int j = 0; j < ln.V; ++j) {
                s_part[wave][0][ln.col0[k] + j] = acc_s[k * ln.V + j];
                s_part[wave][1][ln.col0[k] + j] = acc_b[k * ln.V + j];
            }
    }
    __syncthreads();
    float* out = ws + (int64_t)blockIdx.x * 2 * F;
    for (int which = 0; which < 2; ++which)
        for (int c = threadIdx.x; c < F; c += kThreads) {
            float v = s_part[0][which][c];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) v += s_part[w][which][c];
            out[which * F + c] = v;
        }
}

// ws [parts][2 F] -> dscale [F], dbias [F]
__global__ __launch_bounds__(kThreads) void ln_param_sum_kernel(
    const float* __restrict__ ws, int parts, int F, float* __restrict__ dscale,
    float* __restrict__ dbias) {
    __shared__ float s[kSumSlices][kSumCols];
    const int c = threadIdx.x % kSumCols, slice = threadIdx.x / kSumCols;
    const int col = blockIdx.x * kSumCols + c;
    const int per = (parts + kSumSlices - 1) / kSumSlices;
    const int p0 = slice * per, p1 = p0 + per < parts ? p0 + per : parts;
    float acc = 0.f;
    if (col < 2 * F) {
#pragma unroll 8
        for (int p = p0; p < p1; ++p) acc += ws[(int64_t)p * 2 * F + col];
    }
    s[slice][c] = acc;
    __syncthreads();
    if (slice == 0 && col < 2 * F) {
        float v = s[0][c];
        for (int i = 1; i < kSumSlices; ++i) v += s[i][c];
        if (col < F) dscale[col] = v;
        else dbias[col - F] = v;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
inline int lanes_per_row(int F) { return F <= 128 ? 16 : (F <= 256 ? 32 : 64); }

// The workgroups' shares of the passes; cus <= 0: the workspace's upper bound.
Share make_share(int64_t rows, int F, int cus) {
    const int rows_per_pass = kThreads / lanes_per_row(F);
    Share sh;
    sh.passes = (rows + rows_per_pass - 1) / rows_per_pass;
    int64_t cap = kMaxParts;
    if (cus > 0 && (int64_t)cus * 8 < cap) cap = (int64_t)cus * 8;
    const int64_t want = sh.passes < cap ? sh.passes : cap;
    sh.per_part = (sh.passes + want - 1) / want;
    sh.parts = (int)((sh.passes + sh.per_part - 1) / sh.per_part);
    return sh;
}

int device_share(Share* sh, int64_t rows, int F) {
    const int cus = device_cus();
    *sh = make_share(rows, F, cus > 0 ? cus : 256);
    return MLEARN_OK;
}

int check_common(const char* what, const void* x, int64_t ldx, int32_t dtype, const float* scale,
                 const float* bias, int64_t rows, int32_t F, int32_t act) {
    ML_REQUIRE(F >= 1 && F <= kMaxF, "%s: features = %d outside 1..%d", what, F, kMaxF);
    ML_REQUIRE(rows >= 1, "%s: rows = %lld must be >= 1", what, (long long)rows);
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(act >= kActNone && act <= kActLeaky, "%s: act %d outside 0..2", what, act);
    ML_REQUIRE(x && scale && bias, "%s: null pointer (x, scale or bias)", what);
    ML_REQUIRE(ldx >= F, "%s: ldx = %lld below features = %d", what, (long long)ldx, F);
    return MLEARN_OK;
}

inline bool chunked(const void* p, int64_t ld, int V) {
    return ((uintptr_t)p & 15) == 0 && ld % V == 0;
}

struct FwdArgs {
    const void* x; int64_t ldx; const float* scale; const float* bias; int64_t rows; int F;
    float eps; int act; Share sh; void* y; int64_t ldy; float* mean; float* rstd;
};
struct BwdArgs {
    const void* x; int64_t ldx; const float* scale; const float* bias; const float* mean;
    const float* rstd; const void* dy; int64_t lddy; int64_t rows; int F; int act; Share sh;
    void* dx; int64_t lddx; float* ws;
};

template <typename T, int G, int E, bool VEC>
void launch_one(const FwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((ln_fwd_kernel<T, G, E, VEC>), dim3(a.sh.parts), dim3(kThreads), 0, st,
                       (const T*)a.x, a.ldx, a.scale, a.bias, a.rows, a.F, a.eps, a.act, a.sh,
                       (T*)a.y, a.ldy, a.mean, a.rstd);
}
template <typename T, int G, int E, bool VEC>
void launch_one(const BwdArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((ln_bwd_kernel<T, G, E, VEC>), dim3(a.sh.parts), dim3(kThreads), 0, st,
                       (const T*)a.x, a.ldx, a.scale, a.bias, a.mean, a.rstd, (const T*)a.dy,
                       a.lddy, a.rows, a.F, a.act, a.sh, (T*)a.dx, a.lddx, a.ws);
}

template <typename T, bool VEC, typename Args>
void launch_width(const Args& a, hipStream_t st) {
    if (a.F <= 128) launch_one<T, 16, 8, VEC>(a, st);
    else if (a.F <= 256) launch_one<T, 32, 8, VEC>(a, st);
    else if (a.F <= 512) launch_one<T, 64, 8, VEC>(a, st);
    else launch_one<T, 64, 16, VEC>(a, st);
}

template <typename Args>
void launch_any(const Args& a, int32_t dtype, bool vec, hipStream_t st) {
    if (dtype == MLEARN_DTYPE_F32) {
        if (vec) launch_width<float, true>(a, st);
        else launch_width<float, false>(a, st);
    } else {
        if (vec) launch_width<bf16, true>(a, st);
        else launch_width<bf16, false>(a, st);
    }
}

}  // namespace
}  // namespace ml

extern "C" {

int64_t mlearn_layernorm_workspace_bytes(int64_t rows, int32_t features) {
    using namespace ml;
    if (features < 1 || features > kMaxF || rows < 1) return -1;
    return (int64_t)make_share(rows, features, 0).parts * 2 * features * (int64_t)sizeof(float);
}

int mlearn_layernorm_fwd(const void* x, int64_t ldx, int32_t dtype, const float* scale,
                         const float* bias, int64_t rows, int32_t features, float eps,
                         int32_t act, void* y, int64_t ldy, float* mean, float* rstd,
                         mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_common("layernorm_fwd", x, ldx, dtype, scale, bias, rows, features, act))
        return rc;
    ML_REQUIRE(eps > 0.f && eps < INFINITY, "layernorm_fwd: eps %g is not a positive finite number",
               (double)eps);
    ML_REQUIRE(y && mean && rstd, "layernorm_fwd: null pointer (y, mean or rstd)");
    ML_REQUIRE(ldy >= features, "layernorm_fwd: ldy = %lld below features = %d", (long long)ldy,
               features);
    FwdArgs a = {x, ldx, scale, bias, rows, features, eps, act, {}, y, ldy, mean, rstd};
    device_share(&a.sh, rows, features);
    const int V = dtype == MLEARN_DTYPE_F32 ? 4 : 8;
    const bool vec = features % V == 0 && chunked(x, ldx, V) && chunked(y, ldy, V);
    (void)hipGetLastError();
    launch_any(a, dtype, vec, S(stream));
    return check_launch("layernorm_fwd");
}

int mlearn_layernorm_bwd(const void* x, int64_t ldx, int32_t dtype, const float* scale,
                         const float* bias, const float* mean, const float* rstd, const void* dy,
                         int64_t lddy, int64_t rows, int32_t features, int32_t act, void* dx,
                         int64_t lddx, float* dscale, float* dbias, void* workspace,
                         mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_common("layernorm_bwd", x, ldx, dtype, scale, bias, rows, features, act))
        return rc;
    ML_REQUIRE(mean && rstd && dy && dx && dscale && dbias && workspace,
               "layernorm_bwd: null pointer (mean, rstd, dy, dx, dscale, dbias or workspace)");
    ML_REQUIRE(lddy >= features && lddx >= features,
               "layernorm_bwd: lddy = %lld or lddx = %lld below features = %d", (long long)lddy,
               (long long)lddx, features);
    BwdArgs a = {x, ldx, scale, bias, mean, rstd, dy, lddy, rows, features, act, {}, dx, lddx,
                 (float*)workspace};
    device_share(&a.sh, rows, features);
    const int V = dtype == MLEARN_DTYPE_F32 ? 4 : 8;
    const bool vec = features % V == 0 && chunked(x, ldx, V) && chunked(dy, lddy, V) &&
                     chunked(dx, lddx, V);
    (void)hipGetLastError();
    launch_any(a, dtype, vec, S(stream));
    if (int rc = check_launch("layernorm_bwd")) return rc;
    const unsigned blocks = (unsigned)((2 * features + kSumCols - 1) / kSumCols);
    hipLaunchKernelGGL(ln_param_sum_kernel, dim3(blocks), dim3(kThreads), 0, S(stream),
                       (const float*)workspace, a.sh.parts, features, dscale, dbias);
    return check_launch("layernorm_bwd (parameter sums)");
}

}  // extern "C"
