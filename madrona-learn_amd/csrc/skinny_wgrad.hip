// Tall-skinny weight gradient of the torch path's Dense layers (include/mlearn.h
// "Tall-skinny weight gradient"): dW[k][f] = sum_r x[r][k] dy[r][f] and, on
// request, db[f] = sum_r dy[r][f], for very many rows and a small output.
//
//   x [rows][K], dy [rows][F] row-major and contiguous in T (f32 or bf16),
//   dW [K][F] and db [F] f32; K 1..512, F 1..256, any rows >= 1.
//
//   One workgroup of four waves holds a whole output tile of at most 64 (K) x
//   256 (F): NKB = 1 or 2 blocks of 32 input columns times ceil(F / 32)
//   feature blocks, wave w owning feature blocks w and w + 4 (NFW = 1 or 2), so
//   at most four 32 x 32 accumulators (64 registers) per wave; every wave
//   reads the same x fragments out of LDS.  K <= 64 is one K-tile: x and dy are
//   read from memory exactly once.  K > 64 adds K-tiles as blockIdx.y, each
//   re-reading dy.
//
//   The reduction index is the row, so both MFMA operands are COLUMNS of the
//   row-major operands.  Row chunks (128 bytes of rows: 32 in f32, 64 in bf16)
//   of the x tile and of dy go through LDS in 16-byte pieces, one piece per
//   thread and pass: where the operand's base is 16-byte aligned and its width
//   a multiple of the piece, one 16-byte load, elsewhere element by element.
//   Columns from K / F up to the padded block and rows past the share's end
//   are staged as zeros, so the MFMA loop has no tail case and no byte outside
//   a row or past the last row is read.  bf16 fragments come out of LDS through
//   ds_read_b64_tr_b16, f32 fragments through plain reads with lane = column.
//
//   LDS row stride (lds_stride): a tile of w columns (a multiple of 32) gets
//   rows of ld = 64 floor((w + 31) / 64) + 32 elements, the smallest ld >= w
//   with ld = 32 (mod 64).  f32: the lanes of a half-wave read 32 consecutive
//   dwords of row 2 ks + h, and the two rows start 32 (mod 64) banks apart, so
//   the wave covers all 64 banks.  bf16: a half-wave's transposed read takes
//   four rows of 64 bytes (4 rows x 32 columns); ld elements are ld / 2 = 16
//   (mod 32) dwords, so the four rows start at banks 0, 16, 32, 48 (in some
//   order) and cover all 64 banks.  Rows stay 16-byte aligned for the staging
//   stores.  Tile widths 32, 64, .., 256 give 32, 96, 96, 160, 160, 224, 224,
//   288.
//
//   Pipeline: two LDS stages and two register sets of staged pieces; while
//   chunk c is multiplied out of LDS, the global loads of chunks c + 1 and
//   c + 2 are in flight (sched_barrier keeps the compiler from sinking them
//   below the MFMAs).
//
//   Each workgroup takes one contiguous share of the rows (make_plan: a
//   function of rows, K, F and the CU count) and writes one f32 slab
//   [K][F] + [F] of the workspace: its dW tile and, from the first K-tile, the
//   db row.  db is summed from the staged pieces, each thread over the rows it
//   stages at its fixed columns; the threads' partials are added through LDS
//   in thread order (so wave by wave).  skinny_wgrad_sum_kernel adds the slabs
//   in a fixed order: sixteen contiguous groups of slabs, each in index order,
//   then the sixteen sums in index order.  No atomics, no counters: the same
//   inputs give the same bits.
//
// No contraction and no fast-math in this file.
#pragma clang fp contract(off)
#include "common.h"

namespace ml {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxF = 256, kMaxK = 512;
constexpr int kTileK = 64;            // input columns of one K-tile
constexpr int kMaxParts = 1024;       // slabs at most
constexpr int kChunkRowBytes = 128;   // rows of a chunk x element size
constexpr int kLdsPerCu = 160 * 1024;
constexpr int kSumSegs = 16, kSumCols = 16;

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));

inline int esize(int32_t dtype) { return dtype == MLEARN_DTYPE_F32 ? 4 : 2; }
inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }
__host__ __device__ constexpr int lds_stride(int w) { return (w + 31) / 64 * 64 + 32; }

// How a problem is cut; cus <= 0: the workspace's upper bound.
struct Plan {
    int ktiles, nkb, nfw, ldy, lds;  // K-tiles; 32-blocks of a K-tile; feature blocks per wave
    int64_t share_rows;              // rows of one share (whole chunks)
    int64_t slab;                    // floats of one slab: K F + F
    int parts;                       // shares = slabs
};
Plan make_plan(int64_t rows, int K, int F, int32_t dtype, int cus) {
    Plan p;
    p.ktiles = (K + kTileK - 1) / kTileK;
    p.nkb = K > 32 ? 2 : 1;
    p.nfw = F > 128 ? 2 : 1;
    p.ldy = lds_stride((F + 31) / 32 * 32);
    p.lds = 2 * kChunkRowBytes * (lds_stride(32 * p.nkb) + p.ldy);
    p.slab = (int64_t)K * F + F;
    const int ch = kChunkRowBytes / esize(dtype);
    const int64_t chunks = (rows + ch - 1) / ch;
    // as many shares as workgroups stay resident (at most four per CU, fewer
    // where the LDS stages are large), but no more slab elements than a
    // quarter of the operands' elements
    int occ = kLdsPerCu / p.lds;
    occ = occ < 1 ? 1 : (occ > 4 ? 4 : occ);
    int64_t cap = kMaxParts;
    if (cus > 0 && (int64_t)cus * occ < cap) cap = (int64_t)cus * occ;
    const int64_t traffic = rows * (int64_t)(K + F) / (4 * p.slab);
    if (traffic < cap) cap = traffic < 1 ? 1 : traffic;
    const int64_t want = chunks < cap ? chunks : cap;
    const int64_t per_part = (chunks + want - 1) / want;
    p.parts = (int)((chunks + per_part - 1) / per_part);
    p.share_rows = per_part * ch;
    return p;
}

// ---------------------------------------------------------------------------
// One 16-byte piece of row-major src [..][W]: columns col .. col + VPC of one
// row, zeros where !live and from column W on.
// ---------------------------------------------------------------------------
template <typename T>
__device__ inline u4 load_piece(const T* __restrict__ src, int64_t row, int W, int col, bool live,
                                bool vec) {
    constexpr int VPC = 16 / (int)sizeof(T);
    u4 v = {0u, 0u, 0u, 0u};
    if (!live || col >= W) return v;
    const T* p = src + row * W + col;
    if (vec) return *(const u4*)p;
    T e[VPC];
#pragma unroll
    for (int i = 0; i < VPC; ++i) e[i] = cvt<T>(0.f);
#pragma unroll
    for (int i = 0; i < VPC; ++i)
        if (col + i < W) e[i] = p[i];
    __builtin_memcpy(&v, e, 16);
    return v;
}

__device__ inline void add_piece(float (&s)[4], u4 v, float*) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t w = v[i];  // (a copy: bit_cast of the element lvalue reads element 0)
        s[i] += __builtin_bit_cast(float, w);
    }
}
__device__ inline void add_piece(float (&s)[8], u4 v, bf16*) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = v[i] << 16, hi = v[i] & 0xffff0000u;
        s[2 * i] += __builtin_bit_cast(float, lo);
        s[2 * i + 1] += __builtin_bit_cast(float, hi);
    }
}

// MFMA fragment of the k-step ks (rows of the chunk) at columns c0 .. c0 + 31
// of an LDS tile with rows of ld elements.
template <typename T> struct Frag;
template <> struct Frag<bf16> {
    // lane (r, h): tile[16 ks + 8 h + e][c0 + r], e = 0..7
    __device__ static bf16x8 load(const bf16* tile, int ld, int ks, int c0, int lane) {
        const int g = lane >> 4, hh = g >> 1, cc = g & 1, q = (lane >> 2) & 3, p = lane & 3;
        const bf16* base = tile + (16 * ks + 8 * hh + q) * ld + c0 + 16 * cc + 4 * p;
        typedef __attribute__((address_space(3))) short4v* lp;
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(base));
        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(base + 4 * ld));
        const short8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    }
};
template <> struct Frag<float> {
    // lane (r, h): tile[2 ks + h][c0 + r]
    __device__ static float load(const float* tile, int ld, int ks, int c0, int lane) {
        return tile[(2 * ks + (lane >> 5)) * ld + c0 + (lane & 31)];
    }
};

struct Args {
    const void *x, *dy;
    float* slabs;
    int64_t rows, share_rows, slab;
    int K, F, ldy, want_db, vec_x, vec_y;
};

template <typename T, int NKB, int NFW>
__global__ __launch_bounds__(kThreads) void skinny_wgrad_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CH = kChunkRowBytes / (int)sizeof(T);  // rows of a chunk
    constexpr int VPC = 16 / (int)sizeof(T);             // elements of a piece
    constexpr int KP = 32 * NKB, LDX = lds_stride(KP);
    constexpr int CPRX = KP / VPC, RPPX = kThreads / CPRX, PX = CH / RPPX;  // x: pieces per row,
    static_assert(PX == NKB && RPPX * PX == CH, "x staging passes");        // rows per pass, passes
    constexpr int PY = 4 * NFW;                                             // dy passes at most
    constexpr int KSTEPS = CH / MT<T>::KS;
    constexpr int NS = 2;  // register sets = chunks in flight ahead of the MFMAs

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nfb = (a.F + 31) / 32, FP = 32 * nfb, ldy = a.ldy;
    // dy: cpry pieces per row, rppy rows per pass (threads past rppy rows idle), npy passes
    const int cpry = FP / VPC, rppy = kThreads / cpry, npy = (CH + rppy - 1) / rppy;
    const int xr = tid / CPRX, xc = (tid - xr * CPRX) * VPC;
    const int yr = tid / cpry, yc = (tid - yr * cpry) * VPC;
    const bool y_on = yr < rppy;
    const int k0 = blockIdx.y * kTileK;
    const bool do_db = a.want_db && blockIdx.y == 0;
    const int64_t r0 = (int64_t)blockIdx.x * a.share_rows;
    const int64_t r1 = r0 + a.share_rows < a.rows ? r0 + a.share_rows : a.rows;
    const int nchunks = (int)((r1 - r0 + CH - 1) / CH);
    const T* X = (const T*)a.x;
    const T* Y = (const T*)a.dy;
    T* lds = (T*)smem;  // [stage][x tile CH x LDX | dy tile CH x ldy]
    const int stage_el = CH * (LDX + ldy);
    const bool vec_x = a.vec_x != 0, vec_y = a.vec_y != 0;

    u4 rx[NS][PX], ry[NS][PY];
    float dbv[VPC];
#pragma unroll
    for (int e = 0; e < VPC; ++e) dbv[e] = 0.f;

    auto gload = [&](int c, int set) {
        const int64_t m0 = r0 + (int64_t)c * CH;
#pragma unroll
        for (int u = 0; u < PX; ++u) {
            const int64_t m = m0 + xr + u * RPPX;
            rx[set][u] = load_piece<T>(X, m, a.K, k0 + xc, m < r1, vec_x);
        }
#pragma unroll
        for (int u = 0; u < PY; ++u)
            if (u < npy) {
                const int rl = yr + u * rppy;
                const int64_t m = m0 + rl;
                ry[set][u] = load_piece<T>(Y, m, a.F, yc, y_on && rl < CH && m < r1, vec_y);
            }
    };
    auto sstore = [&](int stage, int set) {
        T* xs = lds + stage * stage_el;
        T* ys = xs + CH * LDX;
#pragma unroll
        for (int u = 0; u < PX; ++u) *(u4*)(xs + (xr + u * RPPX) * LDX + xc) = rx[set][u];
#pragma unroll
        for (int u = 0; u < PY; ++u)
            if (u < npy) {
                const int rl = yr + u * rppy;
                if (y_on && rl < CH) {
                    *(u4*)(ys + rl * ldy + yc) = ry[set][u];
                    if (do_db) add_piece(dbv, ry[set][u], (T*)nullptr);
                }
            }
    };

    f32x16 acc[NKB][NFW];
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
        for (int j = 0; j < NFW; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;
    // this wave's feature blocks: wave and, with NFW = 2, wave + 4
    const bool on0 = wave < nfb, on1 = NFW == 2 && wave + kWaves < nfb;
    auto compute = [&](int stage) {
        if (!on0) return;
        const T* xs = lds + stage * stage_el;
        const T* ys = xs + CH * LDX;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            typename MT<T>::frag fa[NKB], fb[NFW];
#pragma unroll
            for (int i = 0; i < NKB; ++i) fa[i] = Frag<T>::load(xs, LDX, ks, 32 * i, lane);
            fb[0] = Frag<T>::load(ys, ldy, ks, 32 * wave, lane);
            if (NFW == 2 && on1) fb[1] = Frag<T>::load(ys, ldy, ks, 32 * (wave + kWaves), lane);
#pragma unroll
            for (int i = 0; i < NKB; ++i) {
                acc[i][0] = MT<T>::mma(fa[i], fb[0], acc[i][0]);
                if (NFW == 2 && on1) acc[i][NFW - 1] = MT<T>::mma(fa[i], fb[NFW - 1], acc[i][NFW - 1]);
            }
        }
    };

#pragma unroll
    for (int k = 0; k < NS; ++k)
        if (k < nchunks) gload(k, k);
    sstore(0, 0);
    if (NS < nchunks) gload(NS, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; c += NS) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            // chunk c + k: LDS stage k; chunk c + k + 1 waits in set (k + 1) % NS
            if (c + k >= nchunks) break;
            __builtin_amdgcn_sched_barrier(0);
            compute(k);
            __builtin_amdgcn_sched_barrier(0);
            if (c + k + 1 < nchunks) {
                sstore((k + 1) % 2, (k + 1) % NS);
                if (c + k + 1 + NS < nchunks) gload(c + k + 1 + NS, (k + 1) % NS);
            }
            __syncthreads();
        }
    }

    float* out = a.slabs + (int64_t)blockIdx.x * a.slab;
    if (do_db) {
        // (the stages are free: the loop ends in a barrier)
        float* red = (float*)smem;  // [rppy][FP]
        if (y_on) {
#pragma unroll
            for (int e = 0; e < VPC; ++e) red[yr * FP + yc + e] = dbv[e];
        }
        __syncthreads();
        for (int f = tid; f < a.F; f += kThreads) {
            float v = red[f];
            for (int g = 1; g < rppy; ++g) v += red[g * FP + f];
            out[(int64_t)a.K * a.F + f] = v;
        }
    }
    if (!on0) return;
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
        for (int j = 0; j < NFW; ++j) {
            if (j == 1 && !on1) continue;
            const int f = 32 * (wave + kWaves * j) + (lane & 31);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int k = k0 + 32 * i + acc_row(q, lane);
                if (k < a.K && f < a.F) out[(int64_t)k * a.F + f] = acc[i][j][q];
            }
        }
}

// slabs [parts][slab] -> dw [K F] and db [F] (n = K F or K F + F columns):
// thread (seg, col) adds its contiguous group of slabs in index order, then the
// groups are added in index order.
__global__ __launch_bounds__(kSumSegs * kSumCols) void skinny_wgrad_sum_kernel(
    const float* __restrict__ slabs, int parts, int64_t slab, int n, int KF,
    float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float red[kSumSegs][kSumCols];
    const int c = threadIdx.x % kSumCols, seg = threadIdx.x / kSumCols;
    const int col = blockIdx.x * kSumCols + c;
    const int per = (parts + kSumSegs - 1) / kSumSegs;
    const int p0 = seg * per, p1 = p0 + per < parts ? p0 + per : parts;
    float v = 0.f;
    if (col < n) {
#pragma unroll 8
        for (int p = p0; p < p1; ++p) v += slabs[(int64_t)p * slab + col];
    }
    red[seg][c] = v;
    __syncthreads();
    if (seg != 0 || col >= n) return;
#pragma unroll
    for (int s = 1; s < kSumSegs; ++s) v += red[s][c];
    if (col < KF) dw[col] = v;
    else db[col - KF] = v;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool in_range(int64_t rows, int32_t K, int32_t F, int32_t dtype) {
    return rows >= 1 && K >= 1 && K <= kMaxK && F >= 1 && F <= kMaxF &&
           (dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16);
}

template <typename T, int NKB, int NFW>
int launch_one(const Args& a, const Plan& p, hipStream_t st) {
    const void* fn = (const void*)skinny_wgrad_kernel<T, NKB, NFW>;
    if (p.lds > 64 * 1024)
        if (int rc = set_lds_attr(fn, 2 * kChunkRowBytes * (lds_stride(64) + lds_stride(kMaxF)),
                                  "skinny_wgrad"))
            return rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL((skinny_wgrad_kernel<T, NKB, NFW>), dim3((unsigned)p.parts, (unsigned)p.ktiles),
                       dim3(kThreads), (size_t)p.lds, st, a);
    return check_launch("skinny_wgrad");
}

template <typename T> int launch_any(const Args& a, const Plan& p, hipStream_t st) {
    if (p.nkb == 1) return p.nfw == 1 ? launch_one<T, 1, 1>(a, p, st) : launch_one<T, 1, 2>(a, p, st);
    return p.nfw == 1 ? launch_one<T, 2, 1>(a, p, st) : launch_one<T, 2, 2>(a, p, st);
}

}  // namespace
}  // namespace ml

extern "C" {

int64_t mlearn_skinny_wgrad_workspace_bytes(int64_t rows, int32_t in_features, int32_t features,
                                            int32_t dtype) {
    using namespace ml;
    if (!in_range(rows, in_features, features, dtype)) return -1;
    const Plan p = make_plan(rows, in_features, features, dtype, 0);
    return (int64_t)p.parts * p.slab * (int64_t)sizeof(float);
}

int mlearn_skinny_wgrad(const void* x, const void* dy, int64_t rows, int32_t in_features,
                        int32_t features, int32_t dtype, float* dw, float* db, void* workspace,
                        int64_t workspace_bytes, mlearn_stream_t stream) {
    using namespace ml;
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "skinny_wgrad: dtype %d is neither f32 nor bf16", dtype);
    ML_REQUIRE(features >= 1 && features <= kMaxF, "skinny_wgrad: features = %d outside 1..%d",
               features, kMaxF);
    ML_REQUIRE(in_features >= 1 && in_features <= kMaxK,
               "skinny_wgrad: in_features = %d outside 1..%d", in_features, kMaxK);
    ML_REQUIRE(rows >= 1, "skinny_wgrad: rows = %lld below 1", (long long)rows);
    ML_REQUIRE(x && dy && dw && workspace,
               "skinny_wgrad: null pointer (x, dy, dw or workspace; only db may be null)");
    ML_REQUIRE(aligned(x, esize(dtype)) && aligned(dy, esize(dtype)) && aligned(workspace, 16),
               "skinny_wgrad: x or dy is not aligned to its element or the workspace not to 16 "
               "bytes");
    const int64_t need = mlearn_skinny_wgrad_workspace_bytes(rows, in_features, features, dtype);
    ML_REQUIRE(workspace_bytes >= need, "skinny_wgrad: workspace of %lld bytes, %lld needed",
               (long long)workspace_bytes, (long long)need);
    const int cus = device_cus();
    const Plan p = make_plan(rows, in_features, features, dtype, cus > 0 ? cus : 256);
    const int vpc = 16 / esize(dtype);
    // 16-byte pieces: an aligned base and a width that is a multiple of the piece
    const Args a = {x, dy, (float*)workspace, rows, p.share_rows, p.slab, in_features, features,
                    p.ldy, db != nullptr, aligned(x, 16) && in_features % vpc == 0,
                    aligned(dy, 16) && features % vpc == 0};
    if (int rc = dtype == MLEARN_DTYPE_F32 ? launch_any<float>(a, p, S(stream))
                                           : launch_any<bf16>(a, p, S(stream)))
        return rc;
    const int KF = in_features * features, n = KF + (db ? features : 0);
    hipLaunchKernelGGL(skinny_wgrad_sum_kernel, dim3((unsigned)((n + kSumCols - 1) / kSumCols)),
                       dim3(kSumSegs * kSumCols), 0, S(stream), (const float*)workspace, p.parts,
                       p.slab, n, KF, dw, db);
    return check_launch("skinny_wgrad (slab sums)");
}

}  // extern "C"
