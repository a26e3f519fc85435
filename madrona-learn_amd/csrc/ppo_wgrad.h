// Weight gradients of the PPO minibatch step: dW = X^T Y for every weight in
// one launch (with the column-partial and loss-metric blocks riding along),
// followed by the fixed-order reduction (ppo_reduce.h).  Part of ppo.hip's
// translation unit.
#pragma once

#include "ppo_defs.h"
#include "ppo_reduce.h"

namespace ml {

// ---------------------------------------------------------------------------
// Weight gradients dW[i][j] = sum_m X[m][i] * Y[m][j] for every weight of the
// policy in one launch (X, Y row-major [Mp][I] / [Mp][J], written by the step
// kernel).  Workgroup tile 128 (i) x 128 (j): 4 waves in 2x2, each 64x64 =
// 2x2 MFMA blocks.  K = minibatch rows in chunks of 32, double-buffered
// through LDS; the MFMA wants both operands k-contiguous, i.e. COLUMNS of the
// row-major tiles: bf16 fragments come from ds_read_b64_tr_b16 (4 rows x 16
// columns per 16-lane group, delivered column-major), f32 from plain reads.
// LDS rows are 160 elements (80 dwords = 16 mod 64): the 32 lanes of a half
// wave cover all 64 banks on the transposed reads.  Split-K over the rows;
// each split writes an f32 slab that reduce_grads sums in split order.
// ---------------------------------------------------------------------------
struct WgJob {
    const void* X;
    const void* Y;
    float* out;
    int64_t rps;
    int I, J, ti, tj, splits, wg0;
    int grouped;  // wgrad_form 4: one workgroup per (tile, split group), kRgGroups slabs
};
struct WgJobs {
    WgJob job[kMaxJobs];
    int n;
    int64_t Mp;
    int nwg, ncol, ncolx;  // weight-gradient blocks, column-sum blocks (ncolx per chunk)
};

template <typename T> struct WgCfg {
    static constexpr int LD = sizeof(T) == 2 ? 160 : 132;  // LDS row (elements)
    static constexpr size_t buf = (size_t)wg_chunk<T>() * LD * sizeof(T);  // one operand, one stage
    // register-staged form: 2 stages x 2 operands; LDS-DMA form (bf16): ML_WG_STAGES stages of
    // two 32-row x 256-B operand images
    static constexpr size_t glds = (size_t)ML_WG_STAGES * 2 * 32 * 256;
    static constexpr size_t lds =
        (sizeof(T) == 2 && glds > 4 * buf) ? glds : 4 * buf;
};

typedef short short4v __attribute__((ext_vector_type(4)));

template <typename T> struct WgFrag;
template <> struct WgFrag<bf16> {
    typedef bf16x8 frag;
    // lane (r, h): tile[k = 16 ks + 8 h + e][c0 + r], e = 0..7
    __device__ static frag load(const bf16* tile, int ks, int c0, int lane) {
        const int g = lane >> 4, hh = g >> 1, cc = g & 1, q = (lane >> 2) & 3, p = lane & 3;
        const bf16* base = tile + (16 * ks + 8 * hh + q) * WgCfg<bf16>::LD + c0 + 16 * cc + 4 * p;
        typedef __attribute__((address_space(3))) short4v* lp;
        short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(base));
        short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(base + 4 * WgCfg<bf16>::LD));
        typedef short short8v __attribute__((ext_vector_type(8)));
        short8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(frag, v);
    }
};
template <> struct WgFrag<float> {
    typedef float frag;
    // lane (r, h): tile[k = 2 ks + h][c0 + r]
    __device__ static frag load(const float* tile, int ks, int c0, int lane) {
        return tile[(2 * ks + (lane >> 5)) * WgCfg<float>::LD + c0 + (lane & 31)];
    }
};

__device__ inline void colsum_block(const WsK& ws, int bx, int c);
template <bool WEIGHTED = false>
__device__ inline void loss_block(const WsK& ws, const HpK& hp, int64_t M, int K, float* out);

// Weight-gradient tile (i0, j0) of job J over its split's rows.
template <typename T>
__device__ inline void wgrad_tile(const WgJobs& jobs, const WgJob& J, int local, char* smem) {
    constexpr int kWgChunk = wg_chunk<T>();
    constexpr int VPC = 16 / sizeof(T);                  // elements per 16-B chunk
    constexpr int CPR = kWgTile / VPC;                   // chunks per tile row
    constexpr int PER = kWgChunk * CPR / 256;            // chunks per thread per operand
    constexpr int LD = WgCfg<T>::LD, KSTEPS = kWgChunk / MT<T>::KS;
    typedef __attribute__((ext_vector_type(4))) uint32_t u4;
    T* lds = (T*)smem;  // [stage][operand][kWgChunk][LD]

    const int nt = J.ti * J.tj;
    int split, t;
    if ((J.splits & 7) == 0 && (J.wg0 & 7) == 0) {
        // XCD-aware: blocks are dealt round-robin over the 8 XCDs (b % 8), so
        // the nt tiles of one split (which read the same minibatch rows of X
        // and Y) get block ids 8 apart and share an XCD's L2: the rows come
        // from HBM once instead of once per tile (speed only, never correctness)
        const int x = local & 7, q = local >> 3;
        t = q % nt;
        split = (q / nt) * 8 + x;
    } else {
        split = local / nt;
        t = local - split * nt;
    }
    const int i0 = (t % J.ti) * kWgTile, j0 = (t / J.ti) * kWgTile;
    const int64_t m0 = split * J.rps;
    const int64_t m1 = m0 + J.rps < jobs.Mp ? m0 + J.rps : jobs.Mp;  // whole chunks
    const int nchunks = (int)((m1 - m0) / kWgChunk);
    const T* X = (const T*)J.X;
    const T* Y = (const T*)J.Y;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int iw = (w & 1) * 64, jw = (w >> 1) * 64;
    const bool wi_on = i0 + iw < J.I, wj_on = j0 + jw < J.J;

    // NS register sets of staged rows: chunks c + 1 .. c + NS are in flight
    // while chunk c is multiplied out of LDS (two LDS stages); the chunk loop
    // is unrolled by lcm(NS, 2) so that every set / stage index is static
    constexpr int NS = ML_WG_SETS;
    constexpr int U = NS % 2 ? 2 * NS : NS;
    u4 rx[NS][PER], ry[NS][PER];
    auto gload = [&](int c, int set) {
        const int64_t mb0 = m0 + (int64_t)c * kWgChunk;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = tid + 256 * u;
            const int rr = idx / CPR, cc = (idx - rr * CPR) * VPC;
            const u4 zero = {0u, 0u, 0u, 0u};
            rx[set][u] = i0 + cc < J.I ? *(const u4*)(X + (mb0 + rr) * J.I + i0 + cc) : zero;
            ry[set][u] = j0 + cc < J.J ? *(const u4*)(Y + (mb0 + rr) * J.J + j0 + cc) : zero;
        }
    };
    auto sstore = [&](int stage, int set) {
        T* xs = lds + (size_t)stage * 2 * kWgChunk * LD;
        T* ys = xs + kWgChunk * LD;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = tid + 256 * u;
            const int rr = idx / CPR, cc = (idx - rr * CPR) * VPC;
            *(u4*)(xs + rr * LD + cc) = rx[set][u];
            *(u4*)(ys + rr * LD + cc) = ry[set][u];
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) zero_acc<2>(acc[a]);
    auto compute = [&](int stage) {
        if (!(wi_on && wj_on)) return;
        const T* xs = lds + (size_t)stage * 2 * kWgChunk * LD;
        const T* ys = xs + kWgChunk * LD;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            typename WgFrag<T>::frag fa[2], fb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                fa[a] = WgFrag<T>::load(xs, ks, iw + 32 * a, lane);
                fb[a] = WgFrag<T>::load(ys, ks, jw + 32 * a, lane);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = MT<T>::mma(fa[a], fb[b], acc[a][b]);
        }
    };
#pragma unroll
    for (int k = 0; k < NS; ++k)
        if (k < nchunks) gload(k, k);
    sstore(0, 0);
    if (NS < nchunks) gload(NS, 0);
    __syncthreads();
    for (int c = 0; c < nchunks; c += U) {
#pragma unroll
        for (int k = 0; k < U; ++k) {
            // chunk c + k: LDS stage k % 2; chunk c + k + 1 waits in set (k + 1) % NS
            if (c + k >= nchunks) break;
            compute(k % 2);
            if (c + k + 1 < nchunks) {
                sstore((k + 1) % 2, (k + 1) % NS);
                if (c + k + 1 + NS < nchunks) gload(c + k + 1 + NS, (k + 1) % NS);
            }
            __syncthreads();
        }
    }
    if (!wi_on || !wj_on) return;
    float* out = J.out + (int64_t)split * J.I * J.J;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = i0 + iw + 32 * a + acc_row(e, lane);
                const int j = j0 + jw + 32 * b + (lane & 31);
                // nontemporal: the slabs are read once, by the next launch
                // (reduce_grads), so they need not sit dirty in L2 at the
                // kernel boundary (headline 9.08 / 9.11 -> 8.97 / 9.00 ms per
                // update, profiles/r06_wgrad_variants_ab.txt)
                if (i < J.I && j < J.J)
                    __builtin_nontemporal_store(acc[a][b][e], out + (int64_t)i * J.J + j);
            }
}

// ---------------------------------------------------------------------------
// The bf16 weight-gradient tile with its operand chunks staged by LDS-DMA
// (global_load_lds_dwordx4: no staging registers, no LDS write pass), S
// stages deep: chunk c + S - 1 is issued right after the barrier that opens
// chunk c.  The launch is not bound by where its operands live (a second
// back-to-back launch on cache-hot operands: 28.9 vs 29.4 us) but by its
// chunk loop; 2 stages measured best (27.6 vs 29.0 us register-staged; 3 / 4
// stages 29.8 / 31.6 us: more bytes in flight only congest,
// profiles/r06_spill_probes.txt).  Same MFMA fragments in the same order as
// wgrad_tile<bf16>, so the slabs are bit-identical.
//
// LDS image of one operand chunk: 32 rows of P bytes (P = 256 for a 128-
// column tile, 128 for a tile of <= 64 columns), no padding; one DMA
// instruction writes 1 KB lane-linearly (lane l -> bytes 16 l), so the XOR
// swizzle that keeps the transposed fragment reads conflict-free is applied
// to each lane's SOURCE address: 16-byte unit u of row r sits at unit
// u ^ swz(r), swz = 4 (r & 3) at P = 256, 4 ((r >> 1) & 1) at P = 128 (the
// four rows of a half-wave's ds_read_b64_tr_b16 land on four 64-byte bank
// groups).  Columns past the operand's width load unit 0 of the tile again:
// they meet only output rows / columns that are never stored.
// ---------------------------------------------------------------------------
template <int P> __device__ inline int wg_swz(int row) {
    return P == 256 ? 4 * (row & 3) : 4 * ((row >> 1) & 1);
}

// one 16-byte-per-lane LDS-DMA piece: LDS bytes [lds_dst + 16 lane, +16) <- gsrc
// (M0 written and restored in the same statement; hipcc does not count these
// loads, the caller's s_waitcnt vmcnt does)
__device__ inline void wg_glds16(const void* gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}
template <int N> __device__ inline void wg_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int PX, int PY, int CH>
__device__ inline void wgrad_tile_glds(const WgJobs& jobs, const WgJob& J, int local, char* smem) {
    constexpr int S = ML_WG_STAGES;
    static_assert(S >= 2, "at least two stages");
    constexpr int XB = CH * PX, YB = CH * PY, SB = XB + YB;  // bytes per operand / stage
    constexpr int NXW = XB / 1024 / 4, NYW = YB / 1024 / 4;  // DMA pieces per wave
    constexpr int G = NXW + NYW;
    const int nt = J.ti * J.tj;
    int split, t;
    if ((J.splits & 7) == 0 && (J.wg0 & 7) == 0) {  // XCD-aware, as wgrad_tile
        const int x = local & 7, q = local >> 3;
        t = q % nt;
        split = (q / nt) * 8 + x;
    } else {
        split = local / nt;
        t = local - split * nt;
    }
    const int i0 = (t % J.ti) * kWgTile, j0 = (t / J.ti) * kWgTile;
    const int64_t m0 = split * J.rps;
    const int64_t m1 = m0 + J.rps < jobs.Mp ? m0 + J.rps : jobs.Mp;
    const int nchunks = (int)((m1 - m0) / CH);
    const bf16* X = (const bf16*)J.X;
    const bf16* Y = (const bf16*)J.Y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (w & 1) * 64, jw = (w >> 1) * 64;
    const bool wi_on = i0 + iw < J.I, wj_on = j0 + jw < J.J;

    // per-lane source offsets (elements, relative to the chunk's first row)
    int ox[NXW], oy[NYW];
#pragma unroll
    for (int k = 0; k < NXW; ++k) {
        const int b = (w * NXW + k) * 1024 + lane * 16, r = b / PX;
        const int u = ((b % PX) >> 4) ^ wg_swz<PX>(r);
        const int col = i0 + 8 * u < J.I ? i0 + 8 * u : i0;
        ox[k] = r * J.I + col;
    }
#pragma unroll
    for (int k = 0; k < NYW; ++k) {
        const int b = (w * NYW + k) * 1024 + lane * 16, r = b / PY;
        const int u = ((b % PY) >> 4) ^ wg_swz<PY>(r);
        const int col = j0 + 8 * u < J.J ? j0 + 8 * u : j0;
        oy[k] = r * J.J + col;
    }
    const uint32_t lbase =
        (uint32_t)(size_t)(const __attribute__((address_space(3))) char*)smem;
    auto issue = [&](int c, int st) {
        const bf16* xb = X + (m0 + CH * (int64_t)c) * J.I;
        const bf16* yb = Y + (m0 + CH * (int64_t)c) * J.J;
        const uint32_t sb = lbase + (uint32_t)(st * SB);
#pragma unroll
        for (int k = 0; k < NXW; ++k)
            wg_glds16(xb + ox[k], __builtin_amdgcn_readfirstlane(sb + (uint32_t)((w * NXW + k) * 1024)));
#pragma unroll
        for (int k = 0; k < NYW; ++k)
            wg_glds16(yb + oy[k],
                      __builtin_amdgcn_readfirstlane(sb + (uint32_t)(XB + (w * NYW + k) * 1024)));
    };

    // fragment reads: lane (g = lane >> 4: hh = g >> 1, cc = g & 1; q, p) reads rows
    // 16 ks + 8 hh + q (+ 4) at columns c0 + 16 cc + 4 p .. + 3 (wgrad_tile's WgFrag)
    const int g = lane >> 4, hh = g >> 1, cc = g & 1, q = (lane >> 2) & 3, p = lane & 3;
    auto fofs = [&](int c0, int P, int swz) {
        const int u = (c0 >> 3) + 2 * cc + (p >> 1);
        return (8 * hh + q) * P + ((u ^ swz) << 4) + (p & 1) * 8;
    };
    int fx[2], fy[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        fx[a] = fofs(iw + 32 * a, PX, wg_swz<PX>(q));
        fy[a] = fofs(jw + 32 * a, PY, wg_swz<PY>(q));
    }
    typedef __attribute__((address_space(3))) short4v* lp;
    typedef short short8v __attribute__((ext_vector_type(8)));
    auto frag = [&](const char* base, int ofs, int ks, int P) {
        const char* a = base + ks * 16 * P + ofs;
        short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a));
        short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a + 4 * P));
        short8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) zero_acc<2>(acc[a]);
    const bool on = wi_on && wj_on;

#pragma unroll
    for (int k = 0; k < S - 1; ++k)
        if (k < nchunks) issue(k, k);
    int st = 0;  // stage of chunk c
    for (int c = 0; c < nchunks; ++c) {
        // chunk c's pieces (this wave's) have landed: S - 2 younger chunks may
        // stay in flight (fewer near the end)
        if (c + S - 2 < nchunks) wg_vmcnt<G * (S - 2)>();
        else wg_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave's pieces in; stage (c - 1) % S read out
        __builtin_amdgcn_sched_barrier(0);
        if (c + S - 1 < nchunks) issue(c + S - 1, st == 0 ? S - 1 : st - 1);
        if (on) {
            const char* xs = smem + st * SB;
            const char* ys = xs + XB;
#pragma unroll
            for (int ks = 0; ks < CH / 16; ++ks) {
                bf16x8 fa[2], fb[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    fa[a] = frag(xs, fx[a], ks, PX);
                    fb[a] = frag(ys, fy[a], ks, PY);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = MT<bf16>::mma(fa[a], fb[b], acc[a][b]);
            }
        }
        st = st + 1 == S ? 0 : st + 1;
    }
    if (!on) return;
    float* out = J.out + (int64_t)split * J.I * J.J;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = i0 + iw + 32 * a + acc_row(e, lane);
                const int j = j0 + jw + 32 * b + (lane & 31);
                if (i < J.I && j < J.J)
                    __builtin_nontemporal_store(acc[a][b][e], out + (int64_t)i * J.J + j);
            }
}

// ---------------------------------------------------------------------------
// The group-major bf16 weight-gradient tile (mlearn_ppo_hparams.wgrad_form 4).
// reduce_grads' split group g sums the slabs of splits g, g + 16, g + 32, ...
// in that order, starting from 0.f, before the 16 group values meet.  Here
// one workgroup owns (output tile, group g) and forms that group value
// itself: it walks the group's splits in order, each split from zeroed MFMA
// accumulators over the split's own rows (the plan's rps, 32-row chunks, the
// k-steps of wgrad_tile_glds), and after each split adds the accumulators to
// a running f32 sum that starts at 0.f.  It stores one slab per group, so
// reduce_grads finds kRgGroups slabs instead of `splits` and adds them in the
// order it always did: the flat gradient keeps its bits while the slab
// traffic of both launches falls by splits / 16.
//
// Output tile TI x TJ per workgroup (four waves in 2 x 2, each TI/2 x TJ/2),
// smaller than the per-split form's 128 x 128 because a workgroup now has
// splits / 16 times the rows.  The chunks of all the group's splits form one
// LDS-DMA stream, S stages of R chunks deep (one barrier per stage: with one
// MFMA block per wave a 32-row stage is all barrier and LDS latency), so the
// pipeline does not drain at a split boundary.  Operand images, swizzle and fragment reads as wgrad_tile_glds.
// ---------------------------------------------------------------------------
#ifndef ML_WGG_TI
#define ML_WGG_TI 128  // group-major output tile rows
#endif
#ifndef ML_WGG_TJ
#define ML_WGG_TJ 64  // group-major output tile columns
#endif
#ifndef ML_WGG_STAGES
#define ML_WGG_STAGES 2  // group-major LDS stages (S - 1 in flight)
#endif
#ifndef ML_WGG_R
#define ML_WGG_R 4  // group-major: 32-row chunks per LDS stage (one barrier per stage)
#endif
struct WgGroupsCfg {
    static constexpr int TI = ML_WGG_TI, TJ = ML_WGG_TJ, S = ML_WGG_STAGES, R = ML_WGG_R;
    static_assert((TI == 64 || TI == 128) && (TJ == 64 || TJ == 128), "operand image rows of 128 / 256 B");
    static constexpr size_t tile_lds = (size_t)S * R * 32 * 2 * (TI + TJ);
    // the launch also runs the per-split LDS-DMA tile for the jobs that are not grouped
    static constexpr size_t lds = tile_lds > WgCfg<bf16>::glds ? tile_lds : WgCfg<bf16>::glds;
};

template <int TI, int TJ, int S, int R>
__device__ inline void wgrad_tile_groups(const WgJobs& jobs, const WgJob& J, int local, char* smem) {
    static_assert(S >= 2, "at least two stages");
    constexpr int CH = 32, PX = 2 * TI, PY = 2 * TJ;
    constexpr int XB = CH * PX, YB = CH * PY, SB = XB + YB;
    constexpr int NXW = XB / 1024 / 4, NYW = YB / 1024 / 4;
    constexpr int G = NXW + NYW;
    constexpr int AI = TI / 64, BJ = TJ / 64;  // MFMA blocks per wave
    static_assert(G * R * (S - 2) < 64, "vmcnt range");
    const int nt = J.ti * J.tj;
    int g, t;
    if ((J.wg0 & 7) == 0) {
        // XCD-aware, as wgrad_tile: the nt tiles of one group walk the same
        // rows at the same time and get block ids 8 apart (speed only)
        const int x = local & 7, q = local >> 3;
        t = q % nt;
        g = (q / nt) * 8 + x;
    } else {
        g = local / nt;
        t = local - g * nt;
    }
    const int i0 = (t % J.ti) * TI, j0 = (t / J.ti) * TJ;
    // the group's chunk stream: splits g, g + 16, ... of `per` chunks each;
    // only the plan's last split can be shorter, and it ends its group's stream
    const int per = (int)(J.rps / CH);
    const int nsp = (J.splits - g + kRgGroups - 1) / kRgGroups;
    const int64_t lm0 = (int64_t)(g + kRgGroups * (nsp - 1)) * J.rps;
    const int64_t lm1 = lm0 + J.rps < jobs.Mp ? lm0 + J.rps : jobs.Mp;
    const int total = (nsp - 1) * per + (int)((lm1 - lm0) / CH);
    const bf16* X = (const bf16*)J.X;
    const bf16* Y = (const bf16*)J.Y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int iw = (w & 1) * (TI / 2), jw = (w >> 1) * (TJ / 2);
    const bool on = i0 + iw < J.I && j0 + jw < J.J;

    int ox[NXW], oy[NYW];
#pragma unroll
    for (int k = 0; k < NXW; ++k) {
        const int b = (w * NXW + k) * 1024 + lane * 16, r = b / PX;
        const int u = ((b % PX) >> 4) ^ wg_swz<PX>(r);
        const int col = i0 + 8 * u < J.I ? i0 + 8 * u : i0;
        ox[k] = r * J.I + col;
    }
#pragma unroll
    for (int k = 0; k < NYW; ++k) {
        const int b = (w * NYW + k) * 1024 + lane * 16, r = b / PY;
        const int u = ((b % PY) >> 4) ^ wg_swz<PY>(r);
        const int col = j0 + 8 * u < J.J ? j0 + 8 * u : j0;
        oy[k] = r * J.J + col;
    }
    const uint32_t lbase =
        (uint32_t)(size_t)(const __attribute__((address_space(3))) char*)smem;
    // next chunk of the stream: its first row, its index within its split, its stage
    int64_t irow = (int64_t)g * J.rps;
    int ic = 0, islot = 0, issued = 0;
    auto issue_chunk = [&]() {
        const bf16* xb = X + irow * J.I;
        const bf16* yb = Y + irow * J.J;
        const uint32_t sb = lbase + (uint32_t)(islot * SB);
#pragma unroll
        for (int k = 0; k < NXW; ++k)
            wg_glds16(xb + ox[k], __builtin_amdgcn_readfirstlane(sb + (uint32_t)((w * NXW + k) * 1024)));
#pragma unroll
        for (int k = 0; k < NYW; ++k)
            wg_glds16(yb + oy[k],
                      __builtin_amdgcn_readfirstlane(sb + (uint32_t)(XB + (w * NYW + k) * 1024)));
        irow += CH;
        if (++ic == per) {  // on to split + 16
            ic = 0;
            irow += (int64_t)(kRgGroups - 1) * J.rps;
        }
        islot = islot + 1 == S * R ? 0 : islot + 1;
        ++issued;
    };
    // one stage: the stream's next R chunks (fewer at its end; the slots stay R apart)
    auto issue = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (issued < total) issue_chunk();
            else islot = islot + 1 == S * R ? 0 : islot + 1;
        }
    };

    const int lg = lane >> 4, hh = lg >> 1, cc = lg & 1, q = (lane >> 2) & 3, p = lane & 3;
    auto fofs = [&](int c0, int P, int swz) {
        const int u = (c0 >> 3) + 2 * cc + (p >> 1);
        return (8 * hh + q) * P + ((u ^ swz) << 4) + (p & 1) * 8;
    };
    int fx[AI], fy[BJ];
#pragma unroll
    for (int a = 0; a < AI; ++a) fx[a] = fofs(iw + 32 * a, PX, wg_swz<PX>(q));
#pragma unroll
    for (int b = 0; b < BJ; ++b) fy[b] = fofs(jw + 32 * b, PY, wg_swz<PY>(q));
    typedef __attribute__((address_space(3))) short4v* lp;
    typedef short short8v __attribute__((ext_vector_type(8)));
    auto frag = [&](const char* base, int ofs, int ks, int P) {
        const char* a = base + ks * 16 * P + ofs;
        short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a));
        short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a + 4 * P));
        short8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };
    f32x16 acc[AI][BJ], sum[AI][BJ];
#pragma unroll
    for (int a = 0; a < AI; ++a) {
        zero_acc<BJ>(acc[a]);
        zero_acc<BJ>(sum[a]);
    }

    const int nst = (total + R - 1) / R;  // stages of the stream
#pragma unroll
    for (int k = 0; k < S - 1; ++k)
        if (k < nst) issue();
    int st = 0, cs = 0;  // stage of iteration it, the next chunk's index within its split
    for (int it = 0; it < nst; ++it) {
        // stage it has landed (this wave's pieces): the S - 2 younger stages
        // may stay in flight where all of them are whole
        if ((it + S - 1) * R <= total) wg_vmcnt<G * R * (S - 2)>();
        else wg_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave's pieces in; stage (it - 1) % S read out
        __builtin_amdgcn_sched_barrier(0);
        if (it + S - 1 < nst) issue();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (it * R + r >= total) break;
            if (on) {
                const char* xs = smem + (st * R + r) * SB;
                const char* ys = xs + XB;
#pragma unroll
                for (int ks = 0; ks < CH / 16; ++ks) {
                    bf16x8 fa[AI], fb[BJ];
#pragma unroll
                    for (int a = 0; a < AI; ++a) fa[a] = frag(xs, fx[a], ks, PX);
#pragma unroll
                    for (int b = 0; b < BJ; ++b) fb[b] = frag(ys, fy[b], ks, PY);
#pragma unroll
                    for (int a = 0; a < AI; ++a)
#pragma unroll
                        for (int b = 0; b < BJ; ++b)
                            acc[a][b] = MT<bf16>::mma(fa[a], fb[b], acc[a][b]);
                }
            }
            if (++cs == per || it * R + r + 1 == total) {
                // end of a split: reduce_grads' v += slab[split] (the first one onto 0.f)
                cs = 0;
#pragma unroll
                for (int a = 0; a < AI; ++a)
#pragma unroll
                    for (int b = 0; b < BJ; ++b) {
                        sum[a][b] = sum[a][b] + acc[a][b];
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
                    }
            }
        }
        st = st + 1 == S ? 0 : st + 1;
    }
    if (!on) return;
    float* out = J.out + (int64_t)g * J.I * J.J;
#pragma unroll
    for (int a = 0; a < AI; ++a)
#pragma unroll
        for (int b = 0; b < BJ; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = i0 + iw + 32 * a + acc_row(e, lane);
                const int j = j0 + jw + 32 * b + (lane & 31);
                if (i < J.I && j < J.J)
                    __builtin_nontemporal_store(sum[a][b][e], out + (int64_t)i * J.J + j);
            }
}

// The per-split LDS-DMA tile of one job: operand image rows of 128 B (<= 64
// columns) or 256 B.
__device__ inline void wgrad_job_glds(const WgJobs& jobs, const WgJob& J, int local, char* smem) {
    static_assert(kWgTile == 128, "LDS-DMA tile shape");
    if (J.I <= 64) {
        if (J.J <= 64) wgrad_tile_glds<128, 128, 32>(jobs, J, local, smem);
        else wgrad_tile_glds<128, 256, 32>(jobs, J, local, smem);
    } else {
        if (J.J <= 64) wgrad_tile_glds<256, 128, 32>(jobs, J, local, smem);
        else wgrad_tile_glds<256, 256, 32>(jobs, J, local, smem);
    }
}

// Blocks [0, nwg) compute weight gradients; the next ncol blocks the first
// level of the column partials; one more (if loss_out) the loss metrics.
// (The fixed-order reduction into the flat gradient is the next launch,
// reduce_grads_kernel: folding it in as trailing blocks that wait on a
// device-scope counter measured 2.4x slower, profiles/r04_fused_reduce_ab.txt.)
template <typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ML_WG_WAVES, 8))) void wgrad_kernel(
    WgJobs jobs, WsK ws, HpK hp, int64_t M, int K, float* loss_out) {
    if ((int)blockIdx.x >= jobs.nwg) {
        const int b = blockIdx.x - jobs.nwg;
        if (b < jobs.ncol) colsum_block(ws, b % jobs.ncolx, b / jobs.ncolx);
        else loss_block(ws, hp, M, K, loss_out);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int jb = 0;
    while (jb + 1 < jobs.n && (int)blockIdx.x >= jobs.job[jb + 1].wg0) ++jb;
    const WgJob& J = jobs.job[jb];
    if constexpr (sizeof(T) == 2) {
        if (hp.wg_form != 1) {  // mlearn_ppo_hparams.wgrad_form: 2 = LDS-DMA
            wgrad_job_glds(jobs, J, blockIdx.x - J.wg0, smem);
            return;
        }
    }
    wgrad_tile<T>(jobs, J, blockIdx.x - J.wg0, smem);
}

// The launch of wgrad_form 4 (bf16): the grouped jobs' workgroups run the
// group-major tile, every other job's the per-split LDS-DMA tile of form 2;
// column-partial and loss blocks as wgrad_kernel.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ML_WG_WAVES, 8))) void
wgrad_groups_kernel(WgJobs jobs, WsK ws, HpK hp, int64_t M, int K, float* loss_out) {
    if ((int)blockIdx.x >= jobs.nwg) {
        const int b = blockIdx.x - jobs.nwg;
        if (b < jobs.ncol) colsum_block(ws, b % jobs.ncolx, b / jobs.ncolx);
        else loss_block(ws, hp, M, K, loss_out);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int jb = 0;
    while (jb + 1 < jobs.n && (int)blockIdx.x >= jobs.job[jb + 1].wg0) ++jb;
    const WgJob& J = jobs.job[jb];
    const int local = blockIdx.x - J.wg0;
    if (J.grouped) wgrad_tile_groups<WgGroupsCfg::TI, WgGroupsCfg::TJ, WgGroupsCfg::S, WgGroupsCfg::R>(jobs, J, local, smem);
    else wgrad_job_glds(jobs, J, local, smem);
}

// First level of the per-tile column partials (LayerNorm scale/bias grads,
// head-bias grad): colpart2[c][col] = sum over tiles t = c, c + kColChunks, ...
// (8 independent accumulators, combined in fixed order).  Runs as extra
// blocks of the weight-gradient launch.
__device__ inline void colsum_block(const WsK& ws, int bx, int c) {
    const int col = bx * 256 + threadIdx.x;
    if (col >= ws.CP) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int t = c;
    for (; t + 7 * kColChunks < ws.ncp; t += 8 * kColChunks)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] += ws.colpart[(int64_t)(t + u * kColChunks) * ws.CP + col];
    for (int u = 0; t < ws.ncp; t += kColChunks, ++u) acc[u] += ws.colpart[(int64_t)t * ws.CP + col];
    ws.colpart2[(int64_t)c * ws.CP + col] =
        ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// loss_out: five Metric vectors {mean, m2, min, max, count} in the order of
// PPO.add_metrics (ppo.py:95-106): 'Loss' (scalar: {loss, 0, loss, loss, 1}),
// 'Action Obj', 'Value Loss', 'Value Errors', 'Entropy'.
// WEIGHTED (the importance-weighted step, weighted_loss_kernel): the value-loss
// term of 'Loss' from the sum of w * vl (slot 18; slots 16 and 17 then hold
// the weighted sums too); the four metric vectors stay unweighted.
template <bool WEIGHTED>
__device__ inline void loss_block(const WsK& ws, const HpK& hp, int64_t M, int K, float* out) {
    __shared__ double sh[4][kLossSlots];
    __shared__ double tot[kLossSlots];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double v[kLossSlots];
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) {
        const int kind = (s < 16) ? (s & 3) : 0;
        v[s] = kind == 2 ? 3.4e38 : (kind == 3 ? -3.4e38 : 0.0);
    }
    for (int t = tid; t < ws.nlp; t += 256) {
#pragma unroll
        for (int s = 0; s < kLossSlots; ++s) {
            const int kind = (s < 16) ? (s & 3) : 0;
            double u = ws.loss_part[(int64_t)t * kLossSlots + s];
            v[s] = kind == 2 ? fmin(v[s], u) : (kind == 3 ? fmax(v[s], u) : v[s] + u);
        }
    }
#pragma unroll
    for (int s = 0; s < kLossSlots; ++s) {
        const int kind = (s < 16) ? (s & 3) : 0;
        double x = v[s];
        for (int o = 1; o < 64; o <<= 1) {
            double u = __shfl_xor(x, o);
            x = kind == 2 ? fmin(x, u) : (kind == 3 ? fmax(x, u) : x + u);
        }
        if (lane == 0) sh[w][s] = x;
    }
    __syncthreads();
    if (tid < kLossSlots) {
        const int kind = (tid < 16) ? (tid & 3) : 0;
        double x = sh[0][tid];
        for (int i = 1; i < 4; ++i) {
            double u = sh[i][tid];
            x = kind == 2 ? fmin(x, u) : (kind == 3 ? fmax(x, u) : x + u);
        }
        tot[tid] = x;
    }
    __syncthreads();
    if (tid == 0) {
        const double nk = (double)M * K, n = (double)M;
        const double vl_mean = tot[WEIGHTED ? 18 : 4] / n;
        // loss = -sum_key mean(obj_key) + c_v * mean(vl) - sum_key c_e[key] * mean(H_key)
        // (ppo.py:221-252); the per-sub-action weights K / K_key are in slots 16, 17
        const double loss = -tot[17] / nk + hp.vcoef * vl_mean - tot[16] / nk;
        out[0] = (float)loss;
        out[1] = 0.f;
        out[2] = (float)loss;
        out[3] = (float)loss;
        out[4] = 1.f;
        const double cnt[4] = {nk, n, n, nk};
        for (int m = 0; m < 4; ++m) {
            double mean = tot[4 * m] / cnt[m];
            double m2 = tot[4 * m + 1] - cnt[m] * mean * mean;
            out[5 + 5 * m + 0] = (float)mean;
            out[5 + 5 * m + 1] = (float)(m2 > 0 ? m2 : 0);
            out[5 + 5 * m + 2] = (float)tot[4 * m + 2];
            out[5 + 5 * m + 3] = (float)tot[4 * m + 3];
            out[5 + 5 * m + 4] = (float)cnt[m];
        }
    }
}

// mlearn_ppo_minibatch_grad_weighted: loss_out once more from the same
// partials in the same order, 'Loss' now from the weighted sums (its own
// launch after the weight-gradient launch, whose code stays as it is).
__global__ __launch_bounds__(256) void weighted_loss_kernel(WsK ws, HpK hp, int64_t M, int K,
                                                            float* loss_out) {
    loss_block<true>(ws, hp, M, K, loss_out);
}

// The gradient launches: weight-gradient tiles, column partials and loss
// metrics; then the reduction into grad, one 64-parameter chunk per block.
template <typename T>
static int launch_wgrad(const WgJobs& jobs, const WsK& ws, const HpK& hp, int64_t M, int K,
                        float* loss_out, const LayoutK& Lk, float* grad, double* sumsq,
                        hipStream_t s) {
    const int blocks = jobs.nwg + jobs.ncol + (loss_out ? 1 : 0);
    // reduce_grads' view of the slabs: a grouped job left kRgGroups of them,
    // and every job's slabs start where make_wg_jobs put them
    WsK rws = ws;
    bool grouped = false;
    for (int l = 0; l < jobs.n; ++l) {
        const WgJob& J = jobs.job[l];
        grouped |= J.grouped != 0;
        rws.splits[l] = J.grouped ? kRgGroups : J.splits;
        rws.slab_off[l] = J.out - ws.slab;
    }
    // (the LDS attribute: once per kernel and device, kept out of graph capture)
    if (grouped) {
        if (int rc = set_lds_attr((const void*)wgrad_groups_kernel, (int)WgGroupsCfg::lds, "ppo_wgrad_groups"))
            return rc;
        hipLaunchKernelGGL(wgrad_groups_kernel, dim3(blocks), dim3(256), WgGroupsCfg::lds, s, jobs, ws, hp,
                           M, K, loss_out);
    } else {
        if (int rc = set_lds_attr((const void*)wgrad_kernel<T>, (int)WgCfg<T>::lds, "ppo_wgrad"))
            return rc;
        hipLaunchKernelGGL((wgrad_kernel<T>), dim3(blocks), dim3(256), WgCfg<T>::lds, s, jobs, ws, hp,
                           M, K, loss_out);
    }
    hipLaunchKernelGGL(reduce_grads_kernel, dim3((unsigned)((Lk.total + 63) / 64)), dim3(256), 0, s,
                       Lk, rws, grad, sumsq);
    return MLEARN_OK;
}

// Leading jobs of a table that wgrad_form 4 may group (the MLP trunk and head
// weights; the LSTM gate weights keep the per-split tile): bf16 only.
template <typename T> static int wg_groupable(const HpK& hp, int n) {
    return sizeof(T) == 2 && hp.wg_form == 4 ? n : 0;
}

// One weight-gradient job per table row (dW = X^T Y, I x J), in slab order:
// tiles, splits and first workgroup of each, and the launch's block counts.
struct WgOperands {
    int I, J;
    const void *X, *Y;
};
// groupable: the first `groupable` jobs take the group-major form (wgrad_form
// 4) when the plan gives them more than kRgGroups splits; their slabs shrink
// to kRgGroups, and the later jobs' slabs follow (the area carved for the
// plan's splits is never exceeded).
static WgJobs make_wg_jobs(const WgOperands* tab, int n, const WsK& ws, int groupable = 0) {
    WgJobs jobs{};
    jobs.n = n;
    jobs.Mp = ws.Mp;
    int wg = 0;
    int64_t so = 0;
    for (int l = 0; l < n; ++l) {
        WgJob& J = jobs.job[l];
        J.I = tab[l].I;
        J.J = tab[l].J;
        J.X = tab[l].X;
        J.Y = tab[l].Y;
        J.rps = ws.rps[l];
        J.splits = ws.splits[l];
        J.grouped = l < groupable && J.splits > kRgGroups;
        const int ti = J.grouped ? WgGroupsCfg::TI : kWgTile, tj = J.grouped ? WgGroupsCfg::TJ : kWgTile;
        const int slabs = J.grouped ? kRgGroups : J.splits;
        J.out = ws.slab + so;
        so += (int64_t)slabs * J.I * J.J;
        J.ti = (J.I + ti - 1) / ti;
        J.tj = (J.J + tj - 1) / tj;
        J.wg0 = wg;
        wg += J.ti * J.tj * slabs;
    }
    jobs.nwg = wg;
    jobs.ncolx = (ws.CP + 255) / 256;
    jobs.ncol = jobs.ncolx * kColChunks;
    return jobs;
}

}  // namespace ml
