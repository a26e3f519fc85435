// The feature-split rollout policy step: its tuning macros, workgroup shape,
// LDS layout, launch-argument structs, the device body every feature-split
// policy kernel runs (policy_step_body) and the per-step kernel.  Part of
// policy.hip's translation unit (policy_gathered.h and policy_rollout.h
// instantiate the same body, so every kernel computes the same bits).
#pragma once

#include "common.h"
#include "dists.h"
#include "env.h"
#include "rowtile.h"

// One workgroup = 32 environments (one per lane pair); its W waves split the
// hidden features (wave w owns blocks w*NBW .. w*NBW+NBW-1 of every layer).
// Per layer: each wave's MFMAs over the full input (B fragments from LDS),
// LayerNorm statistics combined across the waves through LDS, and the
// post-activation fragments written back to LDS for the next layer.  The
// heads split the reduction instead: each wave multiplies its own features,
// partials are summed in wave order.
#ifndef ML_POL_MAXW
#define ML_POL_MAXW 4  // waves per workgroup, feed-forward policy (feature split; 8 measured 54.3 vs 42.4 us)
#endif
#ifndef ML_POL_RNN_MAXW
#define ML_POL_RNN_MAXW 8  // waves per workgroup, recurrent policy (4: 284 VGPRs, one wave per SIMD)
#endif
#ifndef ML_POL_WAVES
#define ML_POL_WAVES 1  // waves per SIMD the recurrent rollout policy kernel is register-budgeted for (1: compiler choice)
#endif
#ifndef ML_POL_MLP_WAVES
#define ML_POL_MLP_WAVES 3  // the feed-forward kernel: 3 waves per SIMD (<= 168 VGPRs, 3 workgroups per CU)
#endif
#ifndef ML_POL_W1_RING
#define ML_POL_W1_RING 8  // k-steps of the second layer's weights in flight from the start (0: all)
#endif
#ifndef ML_ROLL_MLP_WAVES
#define ML_ROLL_MLP_WAVES 3  // whole-rollout kernel, feed-forward: 3 waves per SIMD (3 workgroups per CU)
#endif
#ifndef ML_ROLL_RNN_WAVES
#define ML_ROLL_RNN_WAVES 3  // whole-rollout kernel, recurrent: 3 waves per SIMD (no spill; 4: 11.71 vs 11.65 ms)
#endif

namespace ml {

template <int H, int MAXW = ML_POL_MAXW> struct PolCfg {
    static constexpr int NB = H / 32;
    static constexpr int W = NB < MAXW ? NB : MAXW;
    static constexpr int NBW = NB / W;
};
// The feature split of a policy kernel (the per-step and the whole-rollout
// kernels use the same one, so they compute the same bits).
template <bool RNN> constexpr int pol_maxw() { return RNN ? ML_POL_RNN_MAXW : ML_POL_MAXW; }
template <int H, bool RNN> constexpr int pol_threads() { return 64 * PolCfg<H, pol_maxw<RNN>()>::W; }

// Dynamic LDS of a feature-split policy kernel with W waves: the B fragments
// [KSH][64], then an f32 region whose offsets (in floats) depend on the
// policy's depth L, then (RNN) the carry fragments [KSH][64].  The one place
// that knows the regions' order and sizes: the body, rollout_stage and every
// launcher's size come from here.
template <typename T, int H, bool RNN, int HC, int W> struct PolLds {
    typedef typename RT<T>::frag frag;
    static constexpr int KSH = H / RT<T>::KS;
    static constexpr int LGS = HC + 1;  // row stride of the head outputs
    static constexpr size_t F32 = (size_t)KSH * 64 * sizeof(frag);  // byte offset of the f32 region
    // offsets in floats from the f32 region (constexpr: callable from host and device)
    static constexpr int gb = 0;                            // [L][2][H] LayerNorm scale, bias
    static constexpr int hbias(int L) { return L * 2 * H; }  // [HC] head bias
    static constexpr int npar(int L) { return hbias(L) + HC; }  // gb + hbias: pol_param's range
    static constexpr int red(int L) { return npar(L); }      // [W][32][2] LayerNorm statistics
    static constexpr int lgp(int L) { return red(L) + W * 64; }  // [head_parts][32][LGS] partials
    static constexpr int lg(int L) { return lgp(L) + head_parts<HC, W>() * 32 * LGS; }  // [32][LGS]
    static constexpr int rbias(int L) { return lg(L) + 32 * LGS; }  // [4H] LSTM bias (RNN)
    static constexpr int bins(int L) { return rbias(L) + (RNN ? 4 * H : 0); }  // [HC] two-hot bins
    static constexpr int frh(int L) { return bins(L) + HC; }  // [KSH][64] carry fragments (RNN)
    static constexpr size_t bytes(int L) { return F32 + (size_t)frh(L) * 4 + (RNN ? F32 : 0); }
};

// Entry i < PolLds::npar(L) of the staged parameters: LayerNorm scale / bias
// of layer i / 2H, then the head bias.
template <int H>
__device__ __forceinline__ float pol_param(const PolicyK& P, int L, int i) {
    if (i < L * 2 * H) {
        const int l = i / (2 * H), c = i - l * 2 * H;
        return c < H ? P.lns[l][c] : P.lnb[l][c - H];
    }
    return P.head_b[i - L * 2 * H];
}

// Post-step of the previous env step, fused into the next policy launch.
struct PostK {
    const float* rew;
    const uint8_t* done;
    float* srew;
    uint8_t* sdone;
    float* env_ret;
    float* trace;
    float gamma;
};

// Train-space outputs of the matched step (mlearn_policy_rollout_step_matched):
// sim row n stores to column tcol[n] of the [ncol]-wide train store, rows with
// tcol[n] outside [0, ncol) (opponents) store nothing.
struct MatchK {
    const int32_t* tcol;  // [N]
    int32_t* sact;        // [ncol][K] store actions (the sim-order actions are the body's `actions`)
    int64_t ncol;
};

// Store column of env row n: n itself, or (MATCHED) its column of the train
// store, -1 if it has none.
template <bool MATCHED>
__device__ __forceinline__ int64_t store_col(const MatchK* mkp, int64_t n) {
    if constexpr (MATCHED) {
        const int32_t c = mkp->tcol[n];
        return (uint64_t)(int64_t)c < (uint64_t)mkp->ncol ? (int64_t)c : -1;
    } else {
        return n;
    }
}

// Where env row `row` stores its observation: its column of the step's store,
// if it has one.
template <bool MATCHED, typename T>
__device__ __forceinline__ T* obs_store_row(T* obs_store, int64_t row, int D, const MatchK* mkp) {
    const int64_t c = store_col<MATCHED>(mkp, row);
    return (!MATCHED || c >= 0) ? obs_store + c * D : nullptr;
}

// rollouts.py:933-973: store reward/done, env_returns = r + gamma * env_returns
// (traced for the 'Env Returns' metric), zeroed where done.  The store writes
// go to the row's store column, env_returns is kept for every row.
template <bool MATCHED>
__device__ inline void post_step_row(const PostK& p, const MatchK* mkp, int64_t n) {
#pragma clang fp contract(off)
    const float r = p.rew[n];
    const uint8_t d = p.done[n] ? 1 : 0;
    const float er = r + p.gamma * p.env_ret[n];
    const int64_t c = store_col<MATCHED>(mkp, n);
    if (!MATCHED || c >= 0) {
        if (p.trace) p.trace[c] = er;
        p.srew[c] = r;
        p.sdone[c] = d;
    }
    p.env_ret[n] = d ? 0.f : er;
}

// Carry of a recurrent policy (mlearn_lstm_carry).
struct CarryK {
    void* h;
    void* c;
    void* sh;
    void* sc;
    int commit;
    const uint8_t* clear;  // extra reset mask (ActorCritic.update's sequence breaks)
};

// ActorCritic.update forward (evaluate mode): given actions in, per
// sub-action entropies out (log-probs go to logp).
struct EvalK {
    const int32_t* actions;
    float* entropies;
    uint64_t* stamps;  // diagnostic builds only (ML_STAMPS): [blocks][W][16]
};

#ifdef ML_STAMPS
static uint64_t* g_pol_stamp_buf = nullptr;
#define PSTAMP(i)                                                                      \
    do {                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                             \
        if (ev.stamps && actions && lane == 0)                                         \
            ev.stamps[((int64_t)tile * W + w) * 16 + (i)] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);                                             \
    } while (0)
#else
#define PSTAMP(i) \
    do {          \
    } while (0)
#endif

// The rows of a gathered tile (policy_gathered.h): tile lane rr < live runs
// env row map[tile * 32 + rr]; mk (MATCHED) maps env rows to store columns.
struct GatherK {
    const int32_t* map;
    int live;
    const MatchK* mk;
};

// Env row of tile lane rr, N for none.  GATHER: the tile's mapped row instead
// of row0 + rr; every output and the Philox counter keep the env index.
template <bool GATHER>
__device__ __forceinline__ int64_t tile_env_row(const GatherK& ga, int64_t row0, int rr, int64_t N) {
    if constexpr (GATHER)
        return rr < ga.live ? (int64_t)ga.map[row0 + rr] : N;
    else
        return row0 + rr;
}

// RNN: the LSTM cell (RecurrentBackboneEncoder, actor_critic.py:173-177)
// sits between the trunk and the heads.  The trunk output fragments (from
// the accumulators, permuted k order) and the carry rows (from HBM, natural k
// order) are staged in LDS; each wave computes the 4 gates of its own 64
// hidden units (8 accumulator blocks, weight images in unit-block gate
// order), so the cell update is register-local and h' lands in exactly the
// layout the heads consume.
template <typename T, int H, bool RNN, int HC, int MAXW, bool STAGED = false, bool GATHER = false,
          bool MATCHED = false>
__device__ __forceinline__ void policy_step_body(
    const PolicyK& P, const float* __restrict__ obs, int64_t N, T* obs_store, int32_t* actions,
    float* logp, float* values, uint32_t k0, uint32_t k1, const uint64_t* step_ctr,
    uint64_t step_add, uint32_t eoff, int sample, const PostK& post, const LstmK& R,
    const CarryK& cy, const EvalK& ev, const EnvK& env, int tile, const GatherK& ga = GatherK{}) {
    typedef typename RT<T>::frag frag;
    typedef PolCfg<H, MAXW> C;
    constexpr int NBW = C::NBW, W = C::W, THREADS = 64 * W;
    constexpr int E = RT<T>::E, KS = RT<T>::KS, SPB = RT<T>::SPB, KSH = H / KS;
    constexpr int KSD = 256 / KS;
    typedef PolLds<T, H, RNN, HC, W> LY;
    constexpr int LGS = LY::LGS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = P.D, L = P.L;
    // (opaque copy of the lane index: in the rollout kernel's step loop the
    // body's lane-derived addresses are then recomputed per step instead of
    // hoisted out of the loop and held live across it)
    int tid_o = (int)threadIdx.x;
    asm volatile("" : "+v"(tid_o));
    const int tid = tid_o, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform (SGPR) for the buffer descriptors
    frag* fr = (frag*)smem;  // [KSH][64] B fragments
    float* gb = (float*)(smem + LY::F32) + LY::gb;
    float* hbias = gb + LY::hbias(L);
    float* red = gb + LY::red(L);
    float* lgp = gb + LY::lgp(L);
    float* lg = gb + LY::lg(L);
    float* rbias = gb + LY::rbias(L);
    float* bins = gb + LY::bins(L);
    frag* frh = (frag*)(gb + LY::frh(L));
    // LayerNorm / head-bias parameters: loads issued now, written to LDS after
    // the first product (their latency hides under the observation loads)
    // (STAGED: the whole-rollout kernel staged them once, before its step loop)
    constexpr int NPAR = STAGED ? 1 : (MLEARN_MAX_LAYERS * 2 * H + HC + THREADS - 1) / THREADS;
    float parv[NPAR];
    if constexpr (!STAGED) {
#pragma unroll
        for (int k = 0; k < NPAR; ++k) {
            const int i = tid + k * THREADS;
            parv[k] = i < LY::npar(L) ? pol_param<H>(P, L, i) : 0.f;
        }
        if constexpr (RNN)
            for (int i = tid; i < 4 * H; i += THREADS) rbias[i] = R.bias[i];
        stage_critic_bins(P, bins, nullptr, tid, THREADS);
    }
    const int64_t row0 = (int64_t)tile * 32;
    const int64_t row = tile_env_row<GATHER>(ga, row0, r, N);
    const bool live = row < N;
    // (a gathered tile's rows are not [row0, row0 + 32): its kernel runs the post-step)
    if (post.rew && tid < 32 && row0 + tid < N) post_step_row<false>(post, nullptr, row0 + tid);
    const uint64_t step = (step_ctr ? *step_ctr : 0ull) + step_add;
    const float invH = 1.0f / (float)H;
    PSTAMP(0);

    // layer 0: observation fragments straight from the env output (cast to
    // the compute dtype = ObservationsCaster); wave 0 copies them to the store
    // the second layer's weights (this wave's blocks) are in flight from the start
    constexpr int W1R = ML_POL_W1_RING > 0 && ML_POL_W1_RING < KSH ? ML_POL_W1_RING : KSH;
    frag w1[W1R][NBW];
    if (L > 1) {
        if constexpr (W1R == KSH)
            prefetch_img<T, NBW, KSH>(w1, (const T*)P.wt[1] + (int64_t)w * NBW * KSH * 64 * E, lane);
        else
            gemm_lds_issue<T, NBW, KSH, W1R>(w1, (const T*)P.wt[1] + (int64_t)w * NBW * KSH * 64 * E,
                                             lane);
    }
    f32x16 acc[NBW];
    zero_acc<NBW>(acc);
    gemm_first<T, NBW>(acc, obs + (live ? row : 0) * D, live, D / KS,
                       (const T*)P.wt[0] + (int64_t)w * NBW * (D / KS) * 64 * E,
                       (w == 0 && obs_store && live) ? obs_store_row<MATCHED>(obs_store, row, D, ga.mk)
                                                     : nullptr,
                       lane, P.obs_mu, P.obs_inv);
    PSTAMP(1);
    if constexpr (!STAGED) {
#pragma unroll
        for (int k = 0; k < NPAR; ++k)
            if (tid + k * THREADS < LY::npar(L)) gb[tid + k * THREADS] = parv[k];
    }
    // LayerNorm parameters staged: the first LayerNorm's statistics barrier
    // orders them (and the LSTM bias / critic bins) before their first read
    typedef typename Pk<T>::word word;
    word aw[NBW][8];
    for (int l = 0;; ++l) {
        // LayerNorm + ReLU (models.py:46-56); row statistics over all waves
        f2 x2[NBW][8];
        word zw[NBW][8];
        float sum, sq;
        ln_pack_stats<T, NBW>(acc, zw, x2, sum, sq);
        sum = sum_halves(sum);
        sq = sum_halves(sq);
        if (h == 0) {
            red[(w * 32 + r) * 2] = sum;
            red[(w * 32 + r) * 2 + 1] = sq;
        }
        __syncthreads();
        sum = red[r * 2];
        sq = red[r * 2 + 1];
#pragma unroll
        for (int v = 1; v < W; ++v) {
            sum += red[(v * 32 + r) * 2];
            sq += red[(v * 32 + r) * 2 + 1];
        }
        const float mean = sum * invH;
        const float var = fmaxf(sq * invH - mean * mean, 0.f);
        const float rstd = rsqrtf(var + 1e-6f);
        PSTAMP(2 + 2 * (l < 1 ? l : 1));
        ln_apply<T, NBW>(x2, mean, rstd, gb + l * 2 * H, H, w * NBW, h, aw);
        if (l + 1 == L && !RNN) break;
#pragma unroll
        for (int i = 0; i < NBW; ++i)
#pragma unroll
            for (int t = 0; t < SPB; ++t)
                fr[((w * NBW + i) * SPB + t) * 64 + lane] = Pk<T>::frag(aw[i], t);
        if (l + 1 == L) break;
        __syncthreads();
        zero_acc<NBW>(acc);
        if (l == 0)
        {
            if constexpr (W1R == KSH)
                gemm_pre_lds<T, NBW, KSH>(acc, w1, fr, lane);
            else
                gemm_lds_run<T, NBW, KSH, W1R>(acc, w1, fr,
                                               (const T*)P.wt[1] + (int64_t)w * NBW * KSH * 64 * E,
                                               lane);
        }
        else
            gemm_lds<T, NBW, KSH, 8>(acc, fr,
                                     (const T*)P.wt[l + 1] + (int64_t)w * NBW * KSH * 64 * E, lane);
        PSTAMP(3);
    }
    PSTAMP(5);

    if constexpr (RNN) {
        // carry rows, cleared where the previous env step was done (rollouts.py:942)
        const bool clr = live && ((post.rew && post.done[row] != 0) ||
                                  (cy.clear && cy.clear[row] != 0));
        const T* hrow = (const T*)cy.h + (live ? row : 0) * H;
        constexpr int SPW = KSH / W;  // k-steps staged per wave
#pragma unroll
        for (int ss = 0; ss < SPW; ++ss) {
            const int s = w * SPW + ss;
            frh[s * 64 + lane] = (live && !clr) ? RT<T>::row(hrow, s, h) : RT<T>::zero();
        }
        __syncthreads();
        constexpr int NG = NBW * 4;
        f32x16 g8[NG];
        zero_acc<NG>(g8);
        gemm_lds<T, NG, KSH, 2>(g8, fr, (const T*)R.wi_perm + (int64_t)w * NG * KSH * 64 * E, lane);
        gemm_lds<T, NG, KSH, 2>(g8, frh, (const T*)R.wh_nat + (int64_t)w * NG * KSH * 64 * E, lane);
        T* hs = (T*)cy.h + row * H;
        T* cs = (T*)cy.c + row * H;
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int u0 = (w * NBW + i) * 32 + 8 * j + 4 * h;  // units of regs 4j .. 4j+3
                float4 hin = make_float4(0.f, 0.f, 0.f, 0.f), cin = hin;
                if (live && !clr) {
                    hin = load4(hs + u0);
                    cin = load4(cs + u0);
                }
                float hn[4], cn[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = 4 * j + e, u = u0 + e;
                    const CellOut o = lstm_cell_fwd<T>(
                        g8[i * 4 + 0][q] + rbias[u], g8[i * 4 + 1][q] + rbias[H + u],
                        g8[i * 4 + 2][q] + rbias[2 * H + u], g8[i * 4 + 3][q] + rbias[3 * H + u],
                        f4get(cin, e));
                    hn[e] = o.h;
                    cn[e] = o.c;
                }
                if (live) {
                    if (cy.sh) {
                        store4((T*)cy.sh + row * H + u0, hin.x, hin.y, hin.z, hin.w);
                        store4((T*)cy.sc + row * H + u0, cin.x, cin.y, cin.z, cin.w);
                    }
                    if (cy.commit) {
                        store4(hs + u0, hn[0], hn[1], hn[2], hn[3]);
                        store4(cs + u0, cn[0], cn[1], cn[2], cn[3]);
                    } else if (clr) {
                        store4(hs + u0, 0.f, 0.f, 0.f, 0.f);
                        store4(cs + u0, 0.f, 0.f, 0.f, 0.f);
                    }
                }
                aw[i][2 * j] = Pk<T>::pack(hn[0], hn[1]);
                aw[i][2 * j + 1] = Pk<T>::pack(hn[2], hn[3]);
            }
        }
    }

    // fused env step (mlearn_policy_rollout_step_env): the next observations
    // depend only on the env state, not on the actions, so they are drawn
    // here, behind the trunk, and stored once every wave is past its reads of
    // this launch's observation rows (after the heads' barrier; with the
    // observation statistics, which read the rows last, at the end)
    const bool fenv = env.state && actions;
    const int EQ = D >> 2;  // quads per env (D is a multiple of 16)
    constexpr int kEnvQ = 2;  // quads per thread drawn early (32 * EQ <= kEnvQ * THREADS)
    const bool env_early = fenv && 32 * EQ <= kEnvQ * THREADS;
    float4 enq[kEnvQ];
    if (env_early) {
#pragma unroll
        for (int u = 0; u < kEnvQ; ++u) {
            const int task = tid + u * THREADS, rr = task / EQ, q = task - rr * EQ;
            const int64_t n = row0 + rr;
            if (task < 32 * EQ && n < N) {
                const u32x4 wv = env_obs_words(env.k0, env.k1, env.eoff + (uint32_t)n, q,
                                               env_step_of(env.state[n]));
                enq[u] = make_float4(env_obs_word(wv.x), env_obs_word(wv.y), env_obs_word(wv.z),
                                     env_obs_word(wv.w));
            }
        }
    }
    auto env_store_obs = [&]() {
#pragma unroll
        for (int u = 0; u < kEnvQ; ++u) {
            const int task = tid + u * THREADS, rr = task / EQ, q = task - rr * EQ;
            const int64_t n = row0 + rr;
            if (task < 32 * EQ && n < N) *(float4*)(env.obs + n * D + 4 * q) = enq[u];
        }
    };

    // actor + critic heads (dists.py:22, models.py:154): lg[row][j] =
    // rnd(rnd(a . W) + rnd(b)).  Head width 32: each wave multiplies its own
    // features (B fragments from registers), partials summed in wave order.
    // Head width 96: the features of every wave staged in LDS, wave w computes
    // column block w / KSPLIT over k-slice w % KSPLIT.
    {
        constexpr int HB = HC / 32;
        constexpr int KSPLIT = head_parts<HC, W>();
        constexpr int KPS = KSH / KSPLIT;
        if constexpr (HB == 1) {
            frag hb[NBW * SPB];
#pragma unroll
            for (int i = 0; i < NBW; ++i)
#pragma unroll
                for (int t = 0; t < SPB; ++t) hb[i * SPB + t] = Pk<T>::frag(aw[i], t);
            f32x16 ha[1];
            zero_acc<1>(ha);
            gemm_ring<T, 1, NBW * SPB, NBW * SPB < 8 ? NBW * SPB : 8>(
                ha, hb, NBW * SPB, (const T*)P.head_t + (int64_t)w * NBW * SPB * 64 * E, lane);
#pragma unroll
            for (int q = 0; q < 16; ++q) lgp[(w * 32 + r) * LGS + feat(0, q, h)] = ha[0][q];
        } else {
            if constexpr (RNN) __syncthreads();  // every wave is done reading fr (Wi product)
#pragma unroll
            for (int i = 0; i < NBW; ++i)
#pragma unroll
                for (int t = 0; t < SPB; ++t)
                    fr[((w * NBW + i) * SPB + t) * 64 + lane] = Pk<T>::frag(aw[i], t);
            __syncthreads();
            for (int u = w; u < HB * KSPLIT; u += W) {
                const int nb = u / KSPLIT, part = u % KSPLIT;
                f32x16 ha[1];
                zero_acc<1>(ha);
                gemm_lds<T, 1, KPS, 8>(ha, fr + part * KPS * 64,
                                       (const T*)P.head_t + ((int64_t)nb * KSH + part * KPS) * 64 * E,
                                       lane);
#pragma unroll
                for (int q = 0; q < 16; ++q) lgp[(part * 32 + r) * LGS + feat(nb, q, h)] = ha[0][q];
            }
        }
        __syncthreads();
        for (int i = tid; i < 32 * HC; i += THREADS) {
            const int rr = i / HC, j = i - rr * HC;
            float x = lgp[rr * LGS + j];
#pragma unroll
            for (int v = 1; v < KSPLIT; ++v) x += lgp[(v * 32 + rr) * LGS + j];
            lg[rr * LGS + j] = rnd<T>(rnd<T>(x) + rnd<T>(hbias[j]));
        }
        __syncthreads();
    }
    if (env_early && !P.obs_stats) env_store_obs();
    PSTAMP(6);

    // sample + store.  Gumbel noise first, one Philox block per 4 logits of a
    // row ((env, logit quad) tasks; the head partials' LDS is free now), then
    // one (env, group) task per thread: argmax of the perturbed logits,
    // log-prob from the logits (bit-identical to sample_group, dists.h)
    if (actions) {
        float* nz = lgp;  // [32][LGS] perturbed logits
        if (sample) {
            const int nq = (P.A + 3) >> 2;
            for (int task = tid; task < 32 * nq; task += THREADS) {
                const int rr = task / nq, q = task - rr * nq;
                const int64_t n = tile_env_row<GATHER>(ga, row0, rr, N);
                if (n >= N) continue;
                const u32x4 u = philox4x32(
                    u32x4{eoff + (uint32_t)n, (uint32_t)q, (uint32_t)step, (uint32_t)(step >> 32)},
                    k0, k1);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * q + e;
                    if (j < P.A)
                        nz[rr * LGS + j] = lg[rr * LGS + j] + det_gumbel(u32_to_unit(u32x4_get(u, e)));
                }
            }
            __syncthreads();
        }
        PSTAMP(7);
        for (int task = tid; task < 32 * P.K; task += THREADS) {
            const int rr = task / P.K, g = task - rr * P.K;
            const int64_t n = tile_env_row<GATHER>(ga, row0, rr, N);
            if (n >= N) continue;
            int a;
            float lp;
            pick_group(lg + rr * LGS + P.off[g], sample ? nz + rr * LGS + P.off[g] : nullptr,
                       P.off[g + 1] - P.off[g], &a, &lp);
            actions[n * P.K + g] = a;
            const int64_t c = store_col<MATCHED>(ga.mk, n);
            if (!MATCHED || c >= 0) {
                if constexpr (MATCHED) ga.mk->sact[c * P.K + g] = a;
                if (logp) logp[c * P.K + g] = lp;
            }
            // fused env: reward, done and state advance of env n from its first
            // action (every lane's state read above is behind the heads' barrier)
            if (fenv && g == 0) {
                const int4 st = env.state[n];
                if (!env_early) {  // the late observation draws read the pre-step counter here
                    ((uint32_t*)red)[2 * rr] = (uint32_t)st.y;
                    ((uint32_t*)red)[2 * rr + 1] = (uint32_t)st.z;
                }
                env_advance_a0(env.state, n, env.eoff + (uint32_t)n, env.k0, env.k1, (float)a,
                               env.rew, env.done, st);
            }
        }
        PSTAMP(8);
    } else if (ev.actions) {
        for (int task = tid; task < 32 * P.K; task += THREADS) {
            const int rr = task / P.K, g = task - rr * P.K;
            const int64_t n = row0 + rr;
            if (n >= N) continue;
            float lp, ent;
            eval_group(lg + rr * LGS + P.off[g], P.off[g + 1] - P.off[g], ev.actions[n * P.K + g],
                       &lp, &ent);
            logp[n * P.K + g] = lp;
            ev.entropies[n * P.K + g] = ent;
        }
    }
    // observation statistics of this step (update_obs_stats, rollouts.py:670-676):
    // the tile's {mean, M2} of the raw observations per feature, 4 lanes per
    // feature (rows q, q + 4, ...), two passes
    if (P.obs_stats && actions && step_add < (uint64_t)P.obs_steps) {
        const int nrow = (int)(N - row0 < 32 ? N - row0 : 32);
        float* out = P.obs_stats + ((int64_t)step_add * P.obs_tiles + tile) * D * 2;
        for (int f0 = 0; f0 < D; f0 += THREADS / 4) {
            const int f = f0 + tid / 4, q = tid % 4;
            const float* col = obs + row0 * D + (f < D ? f : 0);
            float sx = 0.f;
            for (int rr = q; rr < nrow; rr += 4) sx += col[(int64_t)rr * D];
            const float mean = group_sum<4>(sx) / (float)nrow;
            float m2 = 0.f;
            for (int rr = q; rr < nrow; rr += 4) {
                const float d = col[(int64_t)rr * D] - mean;
                m2 += d * d;
            }
            m2 = group_sum<4>(m2);
            if (q == 0 && f < D) {
                out[f * 2] = mean;
                out[f * 2 + 1] = m2;
            }
        }
    }
    if (values) {
        // store column of tile lane rr's value, -1 for none
        auto vcol = [&](int rr) -> int64_t {
            const int64_t n = tile_env_row<GATHER>(ga, row0, rr, N);
            return n < N ? store_col<MATCHED>(ga.mk, n) : -1;
        };
        if (P.CB == 1) {
            if (tid < 32) {
                const int64_t c = vcol(tid);
                if (c >= 0) values[c] = lg[tid * LGS + P.A];
            }
        } else {
            // SymExpTwoHotDistribution.mean() (rollouts.py:601-605): 8 lanes per env
            constexpr int G = 8;
            for (int vt = tid; vt < 32 * G; vt += THREADS) {
                const int rr = vt / G, sub = vt % G;
                float mx, se;
                const float v = twohot_mean_g<G>(lg + rr * LGS + P.A, P.CB, bins, sub, &mx, &se);
                const int64_t c = sub == 0 ? vcol(rr) : -1;
                if (c >= 0) values[c] = v;
            }
        }
    }
    // fused env, late path: observation statistics read this launch's rows
    // last, or the observation is too wide for the early draws
    if (fenv && (P.obs_stats || !env_early)) {
        __syncthreads();
        if (env_early) {
            env_store_obs();
        } else {
            // pre-step counters from the pick loop (LDS)
            const uint32_t* sc = (const uint32_t*)red;
            for (int task = tid; task < 32 * EQ; task += THREADS) {
                const int rr = task / EQ, q = task - rr * EQ;
                const int64_t n = row0 + rr;
                if (n >= N) continue;
                const uint64_t step = ((uint64_t)sc[2 * rr + 1] << 32) | sc[2 * rr];
                env_obs_quad(env.obs + n * D + 4 * q, D, env.k0, env.k1, env.eoff + (uint32_t)n, q,
                             step, true);
            }
        }
    }
    PSTAMP(9);
}

template <typename T, int H, bool RNN, int HC>
__global__ __launch_bounds__((pol_threads<H, RNN>())) __attribute__((amdgpu_waves_per_eu(RNN ? ML_POL_WAVES : ML_POL_MLP_WAVES, 8))) void policy_step_kernel(
    PolicyK P, const float* __restrict__ obs, int64_t N, T* obs_store, int32_t* actions,
    float* logp, float* values, uint32_t k0, uint32_t k1, const uint64_t* step_ctr,
    uint64_t step_add, uint32_t eoff, int sample, PostK post, LstmK R, CarryK cy, EvalK ev,
    EnvK env) {
    policy_step_body<T, H, RNN, HC, pol_maxw<RNN>()>(P, obs, N, obs_store, actions, logp, values, k0, k1,
                                                 step_ctr, step_add, eoff, sample, post, R, cy, ev,
                                                 env, blockIdx.x);
}

}  // namespace ml
