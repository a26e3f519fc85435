// One trunk layer of the torch path as one kernel: y = act(LN(x W)), the
// Dense (no bias) -> LayerNorm -> activation of models.MLP, _EntityEmbed and
// the entity encoder's ff_0 / ff_norm (include/mlearn.h "Dense + LayerNorm +
// activation").
//
//   x [rows][K] in the compute dtype T (f32 or bf16), W the f32 parameter
//   [K][F], F a multiple of 32 up to 256, K 1..512, any rows >= 1.
//
//   A workgroup is four independent waves, a wave owns tiles of 32 rows (row =
//   lane & 31).  The product is transposed as in rowtile.h, Z^T = W^T X^T: the
//   weight image is the MFMA A operand, the row's natural-order fragments,
//   streamed from memory, the B operand, and F / 32 accumulators hold the
//   whole LayerNorm row of the lane's row: the statistics are sums over the
//   lane's registers plus one exchange with lane ^ 32, and the pre-activation
//   never goes to memory.  Rows from `rows` on in the last tile multiply
//   zeros; nothing of them is loaded or stored.
//
//   dense_ln_image_kernel (one small launch per call: the weights change every
//   minibatch) casts W to T and lays the forward image (n = feature, natural k
//   order, K zero-padded to a whole k-step) and the backward image (n = input
//   column zero-padded to 32, k = feature in the ImgK perm order) into the
//   workspace.
//
//   Forward: product, f32 statistics of the unrounded accumulators (flax's
//   fast variance clamped at 0), LN rounded to T, activation on the rounded
//   value, rounded again; y in 4-feature quads, mean and rstd as f32 [rows].
//
//   Backward: the same product code recomputes z (the same bits), from it
//   x_hat and the mask (the sign of the rounded LN output); dz is formed in
//   registers, rounded to T and stored for the caller's weight-gradient GEMM;
//   the rounded dz accumulators are, with no lane movement, the B fragments of
//   dX^T = W dz^T over the backward image (skipped when dx is null).  dscale
//   and dbias: each tile's column sums over its 32 rows in the wave
//   (col_sum16), accumulated over the workgroup's contiguous share of the
//   tiles, the four waves added in order through LDS into one [2][F] workspace
//   row per workgroup; dense_ln_param_sum_kernel adds the rows in index order.
//   No atomics, no counters: the same inputs give the same bits.
//
// No contraction and no fast-math in this file, as in layernorm.hip.
#pragma clang fp contract(off)
#include "rowtile.h"

namespace ml {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxF = 256, kMaxK = 512;
constexpr int kMaxParts = 512;  // partial rows of the workspace at most
constexpr float kEps = 1e-6f;
constexpr float kLeakySlope = 0.01f;

enum { kActNone = 0, kActRelu = 1, kActLeaky = 2 };

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
inline int esize(int32_t dtype) { return dtype == MLEARN_DTYPE_F32 ? 4 : 2; }
inline int kstep(int32_t dtype) { return dtype == MLEARN_DTYPE_F32 ? 2 : 16; }
inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// Workspace: forward image | backward image | [parts][2][F] f32 partial rows.
struct Layout {
    int KP, KP32;           // K padded to a k-step / to 32 input columns
    int64_t bwd_off, part_off, total;
};
Layout make_layout(int K, int F, int32_t dtype, int parts) {
    Layout l;
    l.KP = pad_to(K, kstep(dtype));
    l.KP32 = pad_to(K, 32);
    l.bwd_off = align256((int64_t)F * l.KP * esize(dtype));
    l.part_off = l.bwd_off + align256((int64_t)F * l.KP32 * esize(dtype));
    l.total = l.part_off + (int64_t)parts * 2 * F * (int64_t)sizeof(float);
    return l;
}

// The workgroups' contiguous shares of the tile groups (four tiles, one per
// wave); cus <= 0: the workspace's upper bound.
struct Share {
    int64_t groups;    // ceil(tiles / 4)
    int64_t per_part;  // tile groups of one workgroup
    int parts;         // workgroups
};
Share make_share(int64_t rows, int cus) {
    Share sh;
    sh.groups = (rows + 32 * kWaves - 1) / (32 * kWaves);
    int64_t cap = kMaxParts;
    if (cus > 0 && (int64_t)cus * 2 < cap) cap = (int64_t)cus * 2;
    const int64_t want = sh.groups < cap ? sh.groups : cap;
    sh.per_part = (sh.groups + want - 1) / want;
    sh.parts = (int)((sh.groups + sh.per_part - 1) / sh.per_part);
    return sh;
}

// W [K][F] f32 -> the two images in T; one thread per (input column of the
// padded range, feature).
template <typename T>
__global__ __launch_bounds__(kThreads) void dense_ln_image_kernel(
    const float* __restrict__ w, int K, int F, int KP, int KP32, T* __restrict__ fwd,
    T* __restrict__ bwd) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= KP32 * F) return;
    const int k = idx / F, f = idx - k * F;
    const T v = cvt<T>(k < K ? w[(int64_t)k * F + f] : 0.f);
    if (k < KP) fwd[img_index<T>(f, k, KP, false)] = v;
    if (bwd) bwd[img_index<T>(k, f, F, true)] = v;
}

// ---------------------------------------------------------------------------
// Row fragments: C k-steps of this lane's row.  VEC: the row base is 16-byte
// aligned and K a multiple of the 16-byte chunk, so a chunk lies wholly inside
// or wholly outside the row; elsewhere element by element, zeros from K on.
// ---------------------------------------------------------------------------
template <typename T, int C, bool VEC> struct RowFrags;

template <int C, bool VEC> struct RowFrags<bf16, C, VEC> {
    bf16x8 f[C];
    __device__ void clear() {
#pragma unroll
        for (int i = 0; i < C; ++i) f[i] = RT<bf16>::zero();
    }
    __device__ void load(const bf16* row, bool live, int s0, int h, int K) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int k0 = 16 * (s0 + i) + 8 * h;
            f[i] = RT<bf16>::zero();
            if (live && k0 < K) {
                if (VEC) {
                    f[i] = *(const bf16x8*)(row + k0);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (k0 + e < K) f[i][e] = row[k0 + e];
                }
            }
        }
    }
    __device__ bf16x8 get(int i, int h) const { return f[i]; }
};

template <int C, bool VEC> struct RowFrags<float, C, VEC> {
    // VEC: one float4 = two k-steps for both lane halves (k = 2 s + h)
    static_assert(C % 2 == 0, "two k-steps per 16-byte chunk");
    f32x4 v[C / 2];
    __device__ void clear() {
#pragma unroll
        for (int j = 0; j < C / 2; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ void load(const float* row, bool live, int s0, int h, int K) {
#pragma unroll
        for (int j = 0; j < C / 2; ++j) {
            const int k0 = 2 * s0 + 4 * j;
            v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && k0 < K) {
                if (VEC) {
                    v[j] = *(const f32x4*)(row + k0);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k0 + e < K) v[j][e] = row[k0 + e];
                }
            }
        }
    }
    __device__ float get(int i, int h) const {
        const f32x4 q = v[i >> 1];
        return (i & 1) ? (h ? q[3] : q[2]) : (h ? q[1] : q[0]);
    }
};

// k-steps of A and B fragments in flight ahead of the MFMAs (a ring of two
// chunks; NB A fragments and one B fragment per step)
template <typename T, int NB> constexpr int chunk_steps() {
    return sizeof(T) == 4 ? 8 : (NB == 1 ? 8 : (NB <= 4 ? 4 : 2));
}

// acc[nb] += sum_s Img[block nb][step s] x (fragment s of this lane's row):
// lstm_seq.hip's gemm_rows with NB output blocks and guarded row fragments.
// The forward and the backward both call it, so z has the same bits in both.
template <typename T, int NB, bool VEC>
__device__ inline void product(f32x16 (&acc)[NB], const T* __restrict__ row, bool live, int K,
                               int nks, const T* __restrict__ img, int lane) {
    typedef typename RT<T>::frag frag;
    constexpr int C = chunk_steps<T, NB>();
    constexpr int FB = 64 * RT<T>::E * (int)sizeof(T);
    const __amdgpu_buffer_rsrc_t rs = img_rsrc(img);
    const int voff = lane * RT<T>::E * (int)sizeof(T);
    const int h = lane >> 5;
    frag a[C][NB], an[C][NB];
    RowFrags<T, C, VEC> b, bn;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            a[i][nb] = an[i][nb] = RT<T>::zero();
            if (i < nks) a[i][nb] = img_load<T>(rs, voff, (nb * nks + i) * FB);
        }
    b.load(row, live, 0, h, K);
    bn.clear();
    for (int s0 = 0; s0 < nks; s0 += C) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int s = s0 + C + i;
            if (s < nks) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) an[i][nb] = img_load<T>(rs, voff, (nb * nks + s) * FB);
            }
        }
        bn.load(row, live, s0 + C, h, K);  // (loads nothing from K on)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < C; ++i)
            if (s0 + i < nks) {
                const frag bf = b.get(i, h);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[nb] = MT<T>::mma(a[i][nb], bf, acc[nb]);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < C; ++i)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) a[i][nb] = an[i][nb];
        b = bn;
    }
}

__device__ inline float activate(float z, int act) {
    if (act == kActRelu) return z > 0.f ? z : 0.f;
    if (act == kActLeaky) return z > 0.f ? z : z * kLeakySlope;
    return z;
}

struct FwdK {
    const void* x;
    const void* img;
    const float *scale, *bias;
    void* y;
    float *mean, *rstd;
    int64_t rows;
    int K, F, nks, act;
};

template <typename T, int NB, bool VEC>
__global__ __launch_bounds__(kThreads) void dense_ln_fwd_kernel(FwdK a) {
    __shared__ float gm[2 * kMaxF];  // scale | bias
    constexpr int F = NB * 32;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < F; i += kThreads) {
        gm[i] = a.scale[i];
        gm[F + i] = a.bias[i];
    }
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * kWaves + wave;
    if (tile * 32 >= a.rows) return;
    const int64_t m = tile * 32 + r;
    const bool live = m < a.rows;
    f32x16 acc[NB];
    zero_acc(acc);
    product<T, NB, VEC>(acc, (const T*)a.x + m * a.K, live, a.K, a.nks, (const T*)a.img, lane);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            s1 += acc[nb][q];
            s2 += acc[nb][q] * acc[nb][q];
        }
    s1 = sum_halves(s1);
    s2 = sum_halves(s2);
    const float Ff = (float)F;
    const float mu = s1 / Ff;
    const float var = fmaxf(s2 / Ff - mu * mu, 0.f);
    const float rs = 1.0f / sqrtf(var + kEps);
    if (!live) return;
    if (h == 0) {
        a.mean[m] = mu;
        a.rstd[m] = rs;
    }
    T* yrow = (T*)a.y + m * F;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int f0 = nb * 32 + 8 * g + 4 * h;
            const float4 G = *(const float4*)(gm + f0), B = *(const float4*)(gm + F + f0);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ln = rnd<T>((acc[nb][4 * g + e] - mu) * (rs * f4get(G, e)) + f4get(B, e));
                o[e] = activate(ln, a.act);
            }
            store4(yrow + f0, o[0], o[1], o[2], o[3]);
        }
}

struct BwdK {
    const void* x;
    const void *img, *img_bwd;
    const float *scale, *bias, *mean, *rstd;
    const void* dy;
    void *dz, *dx;  // dx null: no input gradient
    float* part;    // [parts][2][F]
    int64_t rows;
    Share sh;
    int K, F, nks, act, dx_vec;
};

// dX^T = W dz^T for this tile: output blocks of 32 input columns, the k-steps
// over the features taken straight from the rounded dz accumulators (perm
// order); A fragments one chunk of steps ahead, across block boundaries.
template <typename T, int NB>
__device__ inline void input_grad(const f32x16 (&dz)[NB], const T* __restrict__ img, T* dxrow,
                                  bool live, int K, bool vec, int lane) {
    typedef typename RT<T>::frag frag;
    constexpr int SPB = RT<T>::SPB, NS = NB * SPB;
    constexpr int CH = NS < 16 ? NS : (sizeof(T) == 4 ? 16 : 8);
    constexpr int NCH = NS / CH;
    constexpr int FB = 64 * RT<T>::E * (int)sizeof(T);
    const __amdgpu_buffer_rsrc_t rs = img_rsrc(img);
    const int voff = lane * RT<T>::E * (int)sizeof(T);
    const int h = lane >> 5, nob = (K + 31) / 32;
    frag a[CH], an[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) a[i] = an[i] = img_load<T>(rs, voff, i * FB);
    for (int ob = 0; ob < nob; ++ob) {
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            // the next chunk: of this block, or the first of the next block
            const bool wrap = c + 1 == NCH;
            if (!wrap || ob + 1 < nob) {
                const int base = (wrap ? (ob + 1) * NS : ob * NS + (c + 1) * CH);
#pragma unroll
                for (int i = 0; i < CH; ++i) an[i] = img_load<T>(rs, voff, (base + i) * FB);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int s = c * CH + i;
                acc = MT<T>::mma(a[i], RT<T>::from_acc(dz[s / SPB], s % SPB), acc);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < CH; ++i) a[i] = an[i];
        }
        if (live) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c0 = ob * 32 + 8 * g + 4 * h;
                if (vec) {
                    if (c0 < K)
                        store4(dxrow + c0, acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c0 + e < K) dxrow[c0 + e] = cvt<T>(acc[4 * g + e]);
                }
            }
        }
    }
}

template <typename T, int NB, bool VEC>
__global__ __launch_bounds__(kThreads) void dense_ln_bwd_kernel(BwdK a) {
    __shared__ float gm[2 * kMaxF];            // scale | bias
    __shared__ float red[kWaves][2 * kMaxF];   // the waves' dscale | dbias
    constexpr int F = NB * 32;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < F; i += kThreads) {
        gm[i] = a.scale[i];
        gm[F + i] = a.bias[i];
    }
    __syncthreads();
    float ds[NB], db[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) ds[nb] = db[nb] = 0.f;
    const float Ff = (float)F;
    const int64_t g0 = (int64_t)blockIdx.x * a.sh.per_part;
    const int64_t g1 = g0 + a.sh.per_part < a.sh.groups ? g0 + a.sh.per_part : a.sh.groups;
    for (int64_t grp = g0; grp < g1; ++grp) {
        const int64_t tile = grp * kWaves + wave;
        if (tile * 32 >= a.rows) break;  // (wave-uniform; only in the last group)
        const int64_t m = tile * 32 + r;
        const bool live = m < a.rows;
        f32x16 acc[NB], wg[NB];
        zero_acc(acc);
        product<T, NB, VEC>(acc, (const T*)a.x + m * a.K, live, a.K, a.nks, (const T*)a.img, lane);
        const float mu = live ? a.mean[m] : 0.f;
        const float rs = live ? a.rstd[m] : 0.f;
        const T* dyrow = (const T*)a.dy + m * F;
        float c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float gv[16], gx[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int f0 = nb * 32 + 8 * g + 4 * h;
                const float4 G = *(const float4*)(gm + f0), B = *(const float4*)(gm + F + f0);
                const float4 D = live ? load4(dyrow + f0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = 4 * g + e;
                    const float z = acc[nb][q], sc = f4get(G, e);
                    const float ln = rnd<T>((z - mu) * (rs * sc) + f4get(B, e));
                    const float xh = (z - mu) * rs;
                    float gr = f4get(D, e);
                    if (a.act == kActRelu) gr = ln > 0.f ? gr : 0.f;
                    if (a.act == kActLeaky) gr = ln > 0.f ? gr : gr * kLeakySlope;
                    gv[q] = gr;
                    gx[q] = gr * xh;
                    const float w = gr * sc;
                    c1 += w;
                    c2 += w * xh;
                    acc[nb][q] = xh;
                    wg[nb][q] = w;
                }
            }
            db[nb] += col_sum16(gv, lane);
            ds[nb] += col_sum16(gx, lane);
        }
        c1 = sum_halves(c1) / Ff;
        c2 = sum_halves(c2) / Ff;
        T* dzrow = (T*)a.dz + m * F;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int q = 0; q < 16; ++q)
                wg[nb][q] = rnd<T>(rs * (wg[nb][q] - c1 - acc[nb][q] * c2));
            if (live) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    store4(dzrow + nb * 32 + 8 * g + 4 * h, wg[nb][4 * g], wg[nb][4 * g + 1],
                           wg[nb][4 * g + 2], wg[nb][4 * g + 3]);
            }
        }
        if (a.dx)
            input_grad<T, NB>(wg, (const T*)a.img_bwd, (T*)a.dx + m * a.K, live, a.K, a.dx_vec != 0,
                              lane);
    }
    // lanes r and r ^ 16 hold the same totals: one of them writes the wave's
    // row, then the four waves are added in index order
    if ((lane & 16) == 0) {
        const int q = col_sum16_index(lane);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            red[wave][feat(nb, q, h)] = ds[nb];
            red[wave][F + feat(nb, q, h)] = db[nb];
        }
    }
    __syncthreads();
    float* out = a.part + (int64_t)blockIdx.x * 2 * F;
    for (int c = tid; c < 2 * F; c += kThreads) {
        float v = red[0][c];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) v += red[w][c];
        out[c] = v;
    }
}

// part [parts][2 F] -> dscale [F], dbias [F], the rows added in index order
__global__ __launch_bounds__(64) void dense_ln_param_sum_kernel(
    const float* __restrict__ part, int parts, int F, float* __restrict__ dscale,
    float* __restrict__ dbias) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= 2 * F) return;
    float v = 0.f;
#pragma unroll 8
    for (int p = 0; p < parts; ++p) v += part[(int64_t)p * 2 * F + col];
    if (col < F) dscale[col] = v;
    else dbias[col - F] = v;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int check_shape(const char* what, int64_t rows, int32_t K, int32_t F, int32_t dtype, int32_t act) {
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(F >= 32 && F <= kMaxF && F % 32 == 0,
               "%s: features = %d is not a multiple of 32 in 32..%d", what, F, kMaxF);
    ML_REQUIRE(K >= 1 && K <= kMaxK, "%s: in_features = %d outside 1..%d", what, K, kMaxK);
    ML_REQUIRE(rows >= 1 && (rows + 127) / 128 <= 0x7fffffff, "%s: rows = %lld outside 1..2^38",
               what, (long long)rows);
    ML_REQUIRE(act >= kActNone && act <= kActLeaky, "%s: act %d outside 0..2", what, act);
    return MLEARN_OK;
}

inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

// 16-byte row fragments: an aligned base and K a multiple of the chunk
inline bool rows_vec(const void* x, int K, int32_t dtype) {
    return aligned(x, 16) && K % (16 / esize(dtype)) == 0;
}

template <typename T>
void launch_image(const float* w, int K, int F, const Layout& l, void* ws, bool both,
                  hipStream_t st) {
    const unsigned blocks = (unsigned)((l.KP32 * F + kThreads - 1) / kThreads);
    hipLaunchKernelGGL((dense_ln_image_kernel<T>), dim3(blocks), dim3(kThreads), 0, st, w, K, F,
                       l.KP, l.KP32, (T*)ws, both ? (T*)((char*)ws + l.bwd_off) : (T*)nullptr);
}

template <typename T, int NB, bool VEC> void launch_one(const FwdK& a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((dense_ln_fwd_kernel<T, NB, VEC>), dim3(grid), dim3(kThreads), 0, st, a);
}
template <typename T, int NB, bool VEC> void launch_one(const BwdK& a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((dense_ln_bwd_kernel<T, NB, VEC>), dim3(grid), dim3(kThreads), 0, st, a);
}

template <typename T, bool VEC, typename Args>
void launch_width(const Args& a, unsigned grid, hipStream_t st) {
    switch (a.F / 32) {
    case 1: launch_one<T, 1, VEC>(a, grid, st); break;
    case 2: launch_one<T, 2, VEC>(a, grid, st); break;
    case 3: launch_one<T, 3, VEC>(a, grid, st); break;
    case 4: launch_one<T, 4, VEC>(a, grid, st); break;
    case 5: launch_one<T, 5, VEC>(a, grid, st); break;
    case 6: launch_one<T, 6, VEC>(a, grid, st); break;
    case 7: launch_one<T, 7, VEC>(a, grid, st); break;
    default: launch_one<T, 8, VEC>(a, grid, st); break;
    }
}

template <typename Args>
void launch_any(const Args& a, int32_t dtype, bool vec, unsigned grid, hipStream_t st) {
    if (dtype == MLEARN_DTYPE_F32) {
        if (vec) launch_width<float, true>(a, grid, st);
        else launch_width<float, false>(a, grid, st);
    } else {
        if (vec) launch_width<bf16, true>(a, grid, st);
        else launch_width<bf16, false>(a, grid, st);
    }
}

}  // namespace
}  // namespace ml

extern "C" {

int64_t mlearn_dense_ln_workspace_bytes(int64_t rows, int32_t in_features, int32_t features,
                                        int32_t dtype) {
    using namespace ml;
    if (features < 32 || features > kMaxF || features % 32 != 0) return -1;
    if (in_features < 1 || in_features > kMaxK || rows < 1) return -1;
    if (dtype != MLEARN_DTYPE_F32 && dtype != MLEARN_DTYPE_BF16) return -1;
    return make_layout(in_features, features, dtype, make_share(rows, 0).parts).total;
}

int mlearn_dense_ln_fwd(const void* x, const float* w, const float* scale, const float* bias,
                        int64_t rows, int32_t in_features, int32_t features, int32_t dtype,
                        int32_t act, void* y, float* mean, float* rstd, void* workspace,
                        int64_t workspace_bytes, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_shape("dense_ln_fwd", rows, in_features, features, dtype, act)) return rc;
    ML_REQUIRE(x && w && scale && bias && y && mean && rstd && workspace,
               "dense_ln_fwd: null pointer (x, w, scale, bias, y, mean, rstd or workspace)");
    ML_REQUIRE(aligned(y, 16), "dense_ln_fwd: y is not 16-byte aligned");
    ML_REQUIRE(aligned(x, esize(dtype)) && aligned(workspace, 16),
               "dense_ln_fwd: x is not aligned to its element or the workspace not to 16 bytes");
    const int64_t need = mlearn_dense_ln_workspace_bytes(rows, in_features, features, dtype);
    ML_REQUIRE(workspace_bytes >= need, "dense_ln_fwd: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)need);
    const Layout l = make_layout(in_features, features, dtype, 0);
    const FwdK a = {x, workspace, scale, bias, y, mean, rstd, rows, in_features, features,
                    l.KP / kstep(dtype), act};
    const unsigned grid = (unsigned)((rows + 32 * kWaves - 1) / (32 * kWaves));
    (void)hipGetLastError();
    if (dtype == MLEARN_DTYPE_F32) launch_image<float>(w, in_features, features, l, workspace, false, S(stream));
    else launch_image<bf16>(w, in_features, features, l, workspace, false, S(stream));
    if (int rc = check_launch("dense_ln_fwd (weight image)")) return rc;
    launch_any(a, dtype, rows_vec(x, in_features, dtype), grid, S(stream));
    return check_launch("dense_ln_fwd");
}

int mlearn_dense_ln_bwd(const void* x, const float* w, const float* scale, const float* bias,
                        const float* mean, const float* rstd, const void* dy, int64_t rows,
                        int32_t in_features, int32_t features, int32_t dtype, int32_t act,
                        void* dz, void* dx, float* dscale, float* dbias, void* workspace,
                        int64_t workspace_bytes, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_shape("dense_ln_bwd", rows, in_features, features, dtype, act)) return rc;
    ML_REQUIRE(x && w && scale && bias && mean && rstd && dy && dz && dscale && dbias && workspace,
               "dense_ln_bwd: null pointer (x, w, scale, bias, mean, rstd, dy, dz, dscale, dbias "
               "or workspace; only dx may be null)");
    ML_REQUIRE(aligned(dz, 16) && aligned(dy, 16), "dense_ln_bwd: dz or dy is not 16-byte aligned");
    ML_REQUIRE(aligned(x, esize(dtype)) && (!dx || aligned(dx, esize(dtype))) &&
                   aligned(workspace, 16),
               "dense_ln_bwd: x or dx is not aligned to its element or the workspace not to 16 "
               "bytes");
    const int64_t need = mlearn_dense_ln_workspace_bytes(rows, in_features, features, dtype);
    ML_REQUIRE(workspace_bytes >= need, "dense_ln_bwd: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)need);
    const int cus = device_cus();
    const Share sh = make_share(rows, cus > 0 ? cus : 256);
    const Layout l = make_layout(in_features, features, dtype, sh.parts);
    float* part = (float*)((char*)workspace + l.part_off);
    // whole 4-column stores of dx: every row's quads aligned to 4 elements
    const int dx_vec = dx && aligned(dx, 4 * esize(dtype)) && in_features % 4 == 0;
    const BwdK a = {x, workspace, (char*)workspace + l.bwd_off, scale, bias, mean, rstd, dy, dz, dx,
                    part, rows, sh, in_features, features, l.KP / kstep(dtype), act, dx_vec};
    (void)hipGetLastError();
    if (dtype == MLEARN_DTYPE_F32) launch_image<float>(w, in_features, features, l, workspace, true, S(stream));
    else launch_image<bf16>(w, in_features, features, l, workspace, true, S(stream));
    if (int rc = check_launch("dense_ln_bwd (weight images)")) return rc;
    launch_any(a, dtype, rows_vec(x, in_features, dtype), (unsigned)sh.parts, S(stream));
    if (int rc = check_launch("dense_ln_bwd")) return rc;
    hipLaunchKernelGGL(dense_ln_param_sum_kernel, dim3((unsigned)((2 * features + 63) / 64)),
                       dim3(64), 0, S(stream), (const float*)part, sh.parts, features, dscale,
                       dbias);
    return check_launch("dense_ln_bwd (parameter sums)");
}

}  // extern "C"
