// The feature-split PPO minibatch step kernel (the general step: b1, two-hot
// critic, LSTM trunk / heads / backward phases, H = 64 / 128, f32) and its
// launchers.  Part of ppo.hip's translation unit.
#pragma once

#include "dispatch.h"
#include "ppo_defs.h"

namespace ml {

// ---------------------------------------------------------------------------
// Fused minibatch step: one workgroup per 32 rows; its W waves split the
// hidden features (wave w owns blocks w*NBW .. w*NBW+NBW-1 of every layer).
// Per layer the waves run their MFMAs over the full input (B fragments from
// LDS), combine LayerNorm row statistics through LDS, and exchange
// post-activation (forward) or dZ (backward) fragments through LDS.  Each
// wave keeps its own Dense outputs in registers for the backward pass.
// LDS: B fragments [KSH][64], LayerNorm scale/bias [L][2][H], head bias, row
// statistics [W][32][2], head partials [head_parts][32][HC+1], logits /
// d logits [32][HC+1], loss partials [W][kLossSlots], critic bins [HC],
// (HLG) HL-Gauss bin bounds [HC].
// ---------------------------------------------------------------------------
// Every spill store of the step kernel is issued AFTER the weight loads of
// the product that follows it (vmcnt counts loads and stores in issue order,
// so a store batch issued first delays the product's first load wait).
#ifndef ML_STEP_RING
#define ML_STEP_RING 8  // k-steps of weight fragments in flight in the step kernel's trunk products
#endif
#ifndef ML_STEP_MAXW
#define ML_STEP_MAXW 8  // waves per workgroup of the fused step kernel (feature split)
#endif
template <int H> struct StepCfg {
    static constexpr int NB = H / 32;
    static constexpr int W = NB < ML_STEP_MAXW ? NB : ML_STEP_MAXW;
    static constexpr int NBW = NB / W;
};

// Per row tile: B fragments [KSH][64], row statistics [W][32][2], head
// partials and outputs, loss partials; shared by the RTW row tiles of a
// workgroup: LayerNorm scale/bias [L][2][H], head bias [HC], critic bins [HC],
// (HLG) HL-Gauss bin bounds [HC].
template <typename T, int H, int HC> constexpr size_t step_tile_lds() {
    typedef StepCfg<H> C;
    return (size_t)(H / RT<T>::KS) * 64 * sizeof(typename RT<T>::frag) +
           (size_t)(C::W * 64 + (head_parts<HC, C::W>() + 1) * 32 * (HC + 1) + C::W * kLossSlots) * 4;
}
template <typename T, int H, int L, int HC, int RTW = 1, bool HLG = false> static size_t step_lds() {
    return RTW * step_tile_lds<T, H, HC>() + (size_t)(L * 2 * H + (HLG ? 3 : 2) * HC) * 4;
}

// Phases of the step kernel.  kFused: the MLP policy's whole minibatch step.
// Recurrent policies (the LSTM scan runs in between, across time):
//   kTrunkFwd: trunk forward only (writes X_0 and the activations A_l; the
//              last one is the LSTM input);
//   kHeads:    heads + loss + d head from the LSTM outputs (rows of rec.hout,
//              natural k order), writes d loss / d LSTM output rows;
//   kTrunkBwd: trunk forward recomputed, then its backward from the rows of
//              d loss / d trunk output (rec.dfeat).
constexpr int kFused = 0, kTrunkFwd = 1, kHeads = 2, kTrunkBwd = 3;
struct RecK {
    const void* hout;        // [Mp][H] LSTM outputs (kHeads)
    void* dhout;             // [Mp][H] d loss / d LSTM outputs (kHeads)
    const void* dfeat;       // [Mp][H] d loss / d trunk output (kTrunkBwd)
    const void* head_t_nat;  // head image, natural k order (kHeads)
};

// Row-major stores of a wave's NBW 32-feature blocks of its row (bf16), 16
// bytes per lane: lane (r, h) holds features {4h..4h+3, 8+4h..8+4h+3} of
// each 16-feature half s (Pk words 4s .. 4s+3); one v_permlane32_swap per
// word pair trades half h = 0's second quad for half h = 1's first, after
// which lane (r, h) holds the natural features 16s + 8h .. 16s + 8h + 7: two
// 16-byte stores per block instead of four 8-byte row pieces (the A_l / dZ_l
// spill is the step kernel's largest store stream; a tile-native layout with
// 1 KB per store instruction made the step faster and the weight-gradient
// read slower: profiles/r04_spill_layout_ab.txt).  In place (the swap is an
// involution: RESTORE swaps back for a caller that reads the words again; no
// temporaries at the register peak).
template <int NBW, bool RESTORE>
__device__ inline void store_rows16(bf16* rowp, int w, uint32_t (&wd)[NBW][8], int h) {
    typedef __attribute__((ext_vector_type(4))) uint32_t u4;
    auto swap = [&](int i, int s) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const auto v = __builtin_amdgcn_permlane32_swap(wd[i][4 * s + k], wd[i][4 * s + 2 + k],
                                                            false, false);
            wd[i][4 * s + k] = v[0];
            wd[i][4 * s + 2 + k] = v[1];
        }
    };
#pragma unroll
    for (int i = 0; i < NBW; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            swap(i, s);
            *(u4*)(rowp + (w * NBW + i) * 32 + 16 * s + 8 * h) =
                u4{wd[i][4 * s], wd[i][4 * s + 1], wd[i][4 * s + 2], wd[i][4 * s + 3]};
            if (RESTORE) swap(i, s);
        }
}
template <int NBW, bool RESTORE>
__device__ inline void store_rows16(float*, int, f2 (&)[NBW][8], int) {}

// The per-sequence loss weights of the importance-sampled update
// (mlearn_ppo_minibatch_grad_weighted): the step kernel's last argument, empty
// in the unweighted instantiations (WT = false), whose arguments, code and
// results it therefore leaves where they were.
template <bool WT> struct StepWeights {};
template <> struct StepWeights<true> {
    const float* seq_weight;  // [C * N], by sequence id
};
// Weight of minibatch row f: seq_weight[mb_seq[f % mb]] (store_row's index math).
__device__ inline float row_weight(const StepWeights<true>& sw, const int32_t* mb_seq, int mb,
                                   int64_t f) {
    const uint32_t fu = (uint32_t)f, mbu = (uint32_t)mb;
    return sw.seq_weight[mb_seq[fu - (fu / mbu) * mbu]];
}

// What the weighted step adds to the loss tasks of a thread.  The heads
// (ppo_defs.h) run as they are, on a copy of the hyper-parameters whose
// loss_scale is hp.loss_scale * w of the task's row (formed once per row task,
// f32), and into the same accumulators, so the metric sums stay unweighted
// (the recorded metric slots themselves come from an unweighted launch of the
// same minibatch, launch_minibatch: the two instantiations need not contract
// their sums of squares alike).
// The three sums of 'Loss' (ppo.py:220-239) come from the prefix values the
// accumulators pass through: with S_i the sum after task i (S_0 = 0),
//   sum_i w_i (S_i - S_{i-1}) = w_n S_n + sum_{i<n} (w_i - w_{i+1}) S_i,
// which is w S_n exactly when all weights are equal.
template <bool WT> struct LossWeights {};  // unweighted: nothing (the heads see hp itself)
template <> struct LossWeights<true> {
    HpK hl;
    float base;                          // hp.loss_scale
    float pw = 0.f;                      // weight of the previous task's row
    float so = 0.f, se = 0.f, sv = 0.f;  // weighted surrogate / entropy / value-loss sums
    __device__ void init(const HpK& hp) {
        hl = hp;
        base = hp.loss_scale;
    }
    __device__ void begin(float w, const LossAcc& m) {  // before a task of a row of weight w
        const float d = pw - w;
        so += d * m.sobjw;
        se += d * m.sentw;
        sv += d * m.svl;
        pw = w;
        hl.loss_scale = base * w;
    }
    __device__ void finish(const LossAcc& m) {  // after the thread's last task
        so += pw * m.sobjw;
        se += pw * m.sentw;
        sv += pw * m.svl;
    }
};

// RTW row tiles of 32 rows per workgroup (kFused): waves w and w + W * rt own
// the same features of different rows, released by the same barriers, so
// their weight-fragment loads of every product meet in the CU's L1.
// HLG: the HL-Gauss critic (PolicyK.CK = 1) -- a template parameter, so that
// the scalar / two-hot instantiations compile to the code they had before it
// (as a runtime branch it moved their register allocation).
// WT: the importance-weighted step, its own instantiation for the same reason.
template <typename T, int H, int L, int MODE = kFused, int HC = MLEARN_HEAD_COLS, int RTW = 1,
          bool HLG = false, bool WT = false>
__global__ __launch_bounds__(64 * StepCfg<H>::W * RTW) __attribute__((amdgpu_waves_per_eu(ML_STEP_WAVES, 8))) void ppo_step_kernel(
    PolicyK P, RolloutK ro, const int32_t* __restrict__ mb_seq, int mb, int64_t M,
    const float* __restrict__ adv_st, HpK hp, WsK ws, RecK rec, StepWeights<WT> sw) {
    constexpr bool kFwd = MODE != kHeads;                     // runs the trunk forward
    constexpr bool kLoss = MODE == kFused || MODE == kHeads;  // heads + loss
    constexpr bool kBwd = MODE == kFused || MODE == kTrunkBwd;  // trunk backward
    typedef typename RT<T>::frag frag;
    typedef StepCfg<H> C;
    constexpr int NBW = C::NBW, W = C::W, THREADS = 64 * W;
    constexpr int E = RT<T>::E, KS = RT<T>::KS, SPB = RT<T>::SPB;
    constexpr int KSH = H / KS, KSHD = HC / KS, KSD = 256 / KS;
    constexpr int LGS = HC + 1;  // LDS row stride of the head outputs
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = P.D, K = P.K;
    // wave-uniform (SGPR) indices for the buffer descriptors: row tile rt of
    // the workgroup, wave w of that tile
    const int wg_wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rt = wg_wave / W, w = wg_wave - rt * W;
    const int tid = (int)threadIdx.x - rt * THREADS, lane = tid & 63, r = lane & 31, h = lane >> 5;
    char* tsm = smem + (size_t)rt * step_tile_lds<T, H, HC>();
    frag* fr = (frag*)tsm;                     // [KSH][64]
    float* red = (float*)(fr + KSH * 64);      // [W][32][2]
    float* lgp = red + W * 64;                 // [kHeadParts][32][LGS] head partials
    float* lg = lgp + head_parts<HC, W>() * 32 * LGS;  // [32][LGS]
    float* lred = lg + 32 * LGS;               // [W][kLossSlots]
    float* gb = (float*)(smem + (size_t)RTW * step_tile_lds<T, H, HC>());  // [L][2][H] (shared)
    float* hbias = gb + L * 2 * H;             // [HC]
    float* bins = hbias + HC;                  // [HC] critic bins (two-hot) / centres (HL-Gauss)
    float* bounds = bins + HC;                 // (HLG) [HC] HL-Gauss bin bounds (CB + 1 <= HC)
    if constexpr (HLG) {
        if (kLoss) stage_critic_bins(P, bins, bounds, tid, THREADS);
    } else {
        if (kLoss && P.CB > 1)
            for (int i = tid; i < P.CB; i += THREADS) bins[i] = twohot_bin(i, P.CB);
    }
    // LayerNorm / head-bias parameters: loads issued now, written to LDS after
    // the first product (their latency hides under the observation gather)
    constexpr int NPAR = (L * 2 * H + HC + THREADS - 1) / THREADS;
    float parv[NPAR];
#pragma unroll
    for (int k = 0; k < NPAR; ++k) {
        const int i = tid + k * THREADS;
        float v = 0.f;
        if (i < L * 2 * H) {
            const int l = i / (2 * H), c = i - l * 2 * H;
            v = c < H ? P.lns[l][c] : P.lnb[l][c - H];
        } else if (i < L * 2 * H + HC) {
            v = P.head_b[i - L * 2 * H];
        }
        parv[k] = v;
    }
    const int tile = (int)blockIdx.x * RTW + rt;
    const int64_t row0 = (int64_t)tile * 32;
    const int64_t row = row0 + r;
    const bool live = row < M;
    const int64_t sr = live ? store_row(ro, mb_seq, mb, row) : 0;
    // first loss task of this thread: row tr, task tg (group, or value if tg == K)
    const int tr = tid & 31, tg = tid >> 5;
    const bool tlive = kLoss && row0 + tr < M && tg <= K;
    const int64_t tsr = tlive ? store_row(ro, mb_seq, mb, row0 + tr) : 0;
    int t_act = 0;
    float t_lp = 0.f, t_adv = 0.f, t_ret = 0.f, t_val = 0.f;
    [[maybe_unused]] float t_w = 1.f;
    if constexpr (WT)
        if (tlive) t_w = row_weight(sw, mb_seq, mb, row0 + tr);
    if (tlive) {
        t_adv = ro.adv[tsr];
        if (tg < K) {
            t_act = ro.actions[tsr * K + tg];
            t_lp = ro.logp[tsr * K + tg];
        } else {
            t_ret = ret_at(ro, tsr);
            if (ro.values) t_val = ro.values[tsr];
        }
    }

    STAMP(0);
    // ---- forward ----
    f32x16 acc[NBW];
    zero_acc<NBW>(acc);
    if constexpr (kFwd)
        gemm_first<T, NBW>(acc, (const T*)ro.obs + sr * D, live, D / KS,
                           (const T*)P.wt[0] + (int64_t)w * NBW * (D / KS) * 64 * E,
                           (w == 0 && MODE != kTrunkBwd) ? (T*)ws.x0 + row * D : nullptr, lane);
    STAMP(1);
#pragma unroll
    for (int k = 0; k < NPAR; ++k)
        if (tid + k * THREADS < L * 2 * H + HC) gb[tid + k * THREADS] = parv[k];
    // LayerNorm parameters staged: the first LayerNorm's statistics barrier
    // orders them before their first read (ln_apply)
    if constexpr (!kFwd) __syncthreads();
    typedef typename Pk<T>::word word;
    word zr[L][NBW][8];  // this wave's Dense outputs (exact in the compute dtype)
    word aw[NBW][8];     // post-activation of the current layer
    float mean_r[L], rstd_r[L];
    const float invH = 1.0f / (float)H;
    // post-activation rows A_l (weight-gradient operands), row-major
    // (keep: the caller reads aw again -- the bf16 store permutes it in place)
    auto store_act = [&](int l, auto keep) {
        if (MODE == kTrunkBwd) return;
        T* arow = (T*)ws.a[l] + row * H;
        if constexpr (std::is_same<T, bf16>::value) {
            store_rows16<NBW, decltype(keep)::value>(arow, w, aw, h);
            return;
        }
#pragma unroll
        for (int i = 0; i < NBW; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                Pk<T>::store4(arow + (w * NBW + i) * 32 + 8 * g + 4 * h, aw[i][2 * g],
                              aw[i][2 * g + 1]);
    };
#pragma unroll
    for (int l = 0; l < (kFwd ? L : 0); ++l) {
        if (l > 0) {
            zero_acc<NBW>(acc);
            const T* img = (const T*)P.wt[l] + (int64_t)w * NBW * KSH * 64 * E;
            frag ra[ML_STEP_RING][NBW];
            gemm_lds_issue<T, NBW, KSH, ML_STEP_RING>(ra, img, lane);
            store_act(l - 1, std::false_type{});  // A_{l-1}, behind this product's first weight loads
            gemm_lds_run<T, NBW, KSH, ML_STEP_RING>(acc, ra, fr, img, lane);
            STAMP(4);
        }
        f2 x2[NBW][8];
        float sum, sq;
        ln_pack_stats<T, NBW>(acc, zr[l], x2, sum, sq);
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
        mean_r[l] = mean;
        rstd_r[l] = rstd;
        STAMP(2 + 3 * l);
        ln_apply<T, NBW>(x2, mean, rstd, gb + l * 2 * H, H, w * NBW, h, aw);
        // the last layer's rows go out behind the head's weight loads (HC = 32)
        if (l + 1 == L && (MODE != kFused || HC != 32)) store_act(l, std::true_type{});
        if (l + 1 < L) {
#pragma unroll
            for (int i = 0; i < NBW; ++i)
#pragma unroll
                for (int t = 0; t < SPB; ++t)
                    fr[((w * NBW + i) * SPB + t) * 64 + lane] = Pk<T>::frag(aw[i], t);
            __syncthreads();
        }
    }
    STAMP(6);
    if constexpr (MODE == kTrunkFwd) return;
    if constexpr (kLoss) {
    // heads (dists.py:22, models.py:154): lg[row][j] = rnd(rnd(a . W) + rnd(b)).
    // Head width 32: each wave multiplies its own features (B fragments from
    // its registers), partials summed in wave order.  Head width 96: the
    // backbone output of every wave is staged in LDS and wave w computes
    // column block w / KSPLIT over k-slice w % KSPLIT of the full K.
    {
        constexpr int HB = HC / 32;
        constexpr int KSPLIT = head_parts<HC, W>();
        constexpr int KPS = KSH / KSPLIT;  // k-steps per slice
        if constexpr (HB == 1) {
            frag hb[NBW * SPB];
            if constexpr (MODE == kHeads) {
                // this wave's slice of the LSTM output row (natural k order)
                const T* hrow = (const T*)rec.hout + row * H;
#pragma unroll
                for (int j = 0; j < NBW * SPB; ++j) hb[j] = RT<T>::row(hrow, w * NBW * SPB + j, h);
            } else {
#pragma unroll
                for (int i = 0; i < NBW; ++i)
#pragma unroll
                    for (int t = 0; t < SPB; ++t) hb[i * SPB + t] = Pk<T>::frag(aw[i], t);
            }
            const T* himg = (const T*)(MODE == kHeads ? rec.head_t_nat : P.head_t);
            f32x16 ha[1];
            zero_acc<1>(ha);
            if constexpr (MODE == kFused) {
                // every head weight fragment of this wave in flight, then the
                // last layer's rows, then the product
                constexpr int HS = NBW * SPB;
                constexpr int FB = 64 * E * (int)sizeof(T);
                const __amdgpu_buffer_rsrc_t hrs = img_rsrc(himg + (int64_t)w * HS * 64 * E);
                frag hA[HS];
#pragma unroll
                for (int s2 = 0; s2 < HS; ++s2) hA[s2] = img_load<T>(hrs, lane * E * (int)sizeof(T), s2 * FB);
                store_act(L - 1, std::false_type{});
#pragma unroll
                for (int s2 = 0; s2 < HS; ++s2) ha[0] = MT<T>::mma(hA[s2], hb[s2], ha[0]);
            } else
            gemm_ring<T, 1, NBW * SPB, NBW * SPB < 8 ? NBW * SPB : 8>(
                ha, hb, NBW * SPB, himg + (int64_t)w * NBW * SPB * 64 * E, lane);
#pragma unroll
            for (int q = 0; q < 16; ++q) lgp[(w * 32 + r) * LGS + feat(0, q, h)] = ha[0][q];
        } else {
            if constexpr (MODE == kHeads) {
                // LSTM output rows (natural k order), k-steps split over the waves
                const T* hrow = (const T*)rec.hout + row * H;
                for (int s = w; s < KSH; s += W) fr[s * 64 + lane] = RT<T>::row(hrow, s, h);
            } else {
#pragma unroll
                for (int i = 0; i < NBW; ++i)
#pragma unroll
                    for (int t = 0; t < SPB; ++t)
                        fr[((w * NBW + i) * SPB + t) * 64 + lane] = Pk<T>::frag(aw[i], t);
            }
            __syncthreads();
            const T* himg = (const T*)(MODE == kHeads ? rec.head_t_nat : P.head_t);
            for (int u = w; u < HB * KSPLIT; u += W) {
                const int nb = u / KSPLIT, part = u % KSPLIT;
                f32x16 ha[1];
                zero_acc<1>(ha);
                gemm_lds<T, 1, KPS, 8>(ha, fr + part * KPS * 64,
                                       himg + ((int64_t)nb * KSH + part * KPS) * 64 * E, lane);
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

    STAMP(7);
    // ---- loss: one (row, group | value) task per thread (ppo.py:129-262) ----
    {
        LossAcc m;
        [[maybe_unused]] LossWeights<WT> lw;
        if constexpr (WT) lw.init(hp);
        bool did = false;  // this lane ran a task (waves without any skip the reductions)
        const float as0 = adv_st[0], as1 = adv_st[1];
        const float* vn = hp.norm_vals ? adv_st + 2 : nullptr;
        // two-hot critic: the value rows run in groups of 8 lanes (below); with
        // 512 threads they take the last 256 while the first ones do the groups
        const bool th = P.CB > 1;
        const bool split = th && THREADS >= 512;
        const int tstride = split ? THREADS - 256 : THREADS;
        const int ntask = 32 * (th ? K : K + 1);
        for (int task = (split && tid >= THREADS - 256) ? ntask : tid; task < ntask;
             task += tstride) {
            const int rr = task & 31, g = task >> 5;
            did = true;
            float* lr = lg + rr * LGS;
            const int64_t f = row0 + rr;
            if (f >= M) {  // padding row: zero its d logits
                if (g < K)
                    for (int j = P.off[g]; j < P.off[g + 1]; ++j) lr[j] = 0.f;
                else
                    for (int j = P.A; j < HC; ++j) lr[j] = 0.f;
                continue;
            }
            int act;
            float olp, adv, ret, oval;
            if (task == tid) {
                act = t_act, olp = t_lp, adv = t_adv, ret = t_ret, oval = t_val;
                if constexpr (WT) lw.begin(t_w, m);
            } else {
                if constexpr (WT) lw.begin(row_weight(sw, mb_seq, mb, f), m);
                const int64_t q = store_row(ro, mb_seq, mb, f);
                adv = ro.adv[q];
                act = g < K ? ro.actions[q * K + g] : 0;
                olp = g < K ? ro.logp[q * K + g] : 0.f;
                ret = g < K ? 0.f : ret_at(ro, q);
                oval = (g < K || !ro.values) ? 0.f : ro.values[q];
            }
            if (g < K) {
                if (hp.norm_adv) adv = (adv - as0) * as1;
                if constexpr (WT)
                    loss_group(lw.hl, lr + P.off[g], P.off[g + 1] - P.off[g], act, olp, adv,
                               hp.ecoef[g], hp.objw[g], m);
                else
                loss_group(hp, lr + P.off[g], P.off[g + 1] - P.off[g], act, olp, adv, hp.ecoef[g],
                           hp.objw[g], m);
            } else {
                if constexpr (WT) loss_value(lw.hl, lr, P.A, HC, ret, oval, m, vn);
                else
                loss_value(hp, lr, P.A, HC, ret, oval, m, vn);
            }
        }
        if (th) {
            constexpr int G = 8;
            const int vt0 = split ? tid - (THREADS - 256) : tid;
            const int vstride = split ? 256 : THREADS;
            for (int vt = vt0 < 0 ? 32 * G : vt0; vt < 32 * G; vt += vstride) {
                const int rr = vt / G, sub = vt % G;
                did = true;
                float* lr = lg + rr * LGS;
                const int64_t f = row0 + rr;
                if (f >= M) {  // padding row: zero its d critic logits
                    for (int j = P.A + sub; j < HC; j += G) lr[j] = 0.f;
                    continue;
                }
                const float R = ret_at(ro, store_row(ro, mb_seq, mb, f));
                if constexpr (WT) lw.begin(row_weight(sw, mb_seq, mb, f), m);
                if constexpr (WT) {
                    if constexpr (HLG)
                        loss_value_hlgauss_g<G>(lw.hl, lr, P.A, P.CB, HC, bins, bounds,
                                                P.head_b[HC + 2 * P.CB + 1], lgp + rr * LGS, R, sub,
                                                m);
                    else
                        loss_value_twohot_g<G>(lw.hl, lr, P.A, P.CB, HC, bins, R, sub, m);
                } else
                if constexpr (HLG)  // smoothness ends the table; scratch = the row's head partials
                    loss_value_hlgauss_g<G>(hp, lr, P.A, P.CB, HC, bins, bounds,
                                            P.head_b[HC + 2 * P.CB + 1], lgp + rr * LGS, R, sub, m);
                else
                    loss_value_twohot_g<G>(hp, lr, P.A, P.CB, HC, bins, R, sub, m);
            }
        }
        typedef typename std::conditional<WT, float, const float>::type slot_t;
        slot_t vals[kLossSlots] = {m.sobj, m.qobj, m.mnobj, m.mxobj, m.svl, m.qvl, m.mnvl,
                                   m.mxvl, m.serr, m.qerr, m.mnerr, m.mxerr, m.sent, m.qent,
                                   m.mnent, m.mxent, m.sentw, m.sobjw, 0.f, 0.f};
        if constexpr (WT) {  // the three weighted sums of 'Loss' (loss_block<true>)
            lw.finish(m);
            vals[16] = lw.se;
            vals[17] = lw.so;
            vals[18] = lw.sv;
        }
        constexpr int kUsed = WT ? 19 : 18;  // the slots above are padding
        if (!hp.metrics) {
        } else if (__any(did)) {
#pragma unroll
            for (int s = 0; s < kUsed; ++s) {
                const int kind = (s < 16) ? (s & 3) : 0;
                float v = vals[s];
                v = kind == 2 ? wave_reduce<2>(v)
                              : (kind == 3 ? wave_reduce<3>(v) : wave_reduce<0>(v));
                if (lane == 0) lred[w * kLossSlots + s] = v;
            }
            if (lane >= kUsed && lane < kLossSlots) lred[w * kLossSlots + lane] = 0.f;
        } else if (lane < kLossSlots) {  // identities of sum / min / max
            const int kind = (lane < 16) ? (lane & 3) : 0;
            lred[w * kLossSlots + lane] = kind == 2 ? 3.4e38f : (kind == 3 ? -3.4e38f : 0.f);
        }
    }
    __syncthreads();
    if (hp.metrics && tid < kLossSlots) {
        const int kind = (tid < 16) ? (tid & 3) : 0;
        double v = lred[tid];
        for (int u = 1; u < W; ++u) {
            const double x = lred[u * kLossSlots + tid];
            v = kind == 2 ? fmin(v, x) : (kind == 3 ? fmax(v, x) : v + x);
        }
        // (the weighted step writes its three sums of 'Loss' only: the metric
        // slots are the unweighted launch's that ran before it, launch_minibatch)
        if (!WT || (tid >= 16 && tid < 19)) ws.loss_part[(int64_t)tile * kLossSlots + tid] = v;
    }
    STAMP(8);
    // the backward head product's weight fragments go out before the stores below
    constexpr int kHeadPre = KSHD * NBW <= 16 ? KSHD : 0;
    frag hbw[kHeadPre > 0 ? kHeadPre : 1][NBW];
    const T* hbimg = (const T*)P.head + (int64_t)w * NBW * KSHD * 64 * E;
    if constexpr (kHeadPre > 0) {
        const __amdgpu_buffer_rsrc_t hrs = img_rsrc(hbimg);
#pragma unroll
        for (int s2 = 0; s2 < kHeadPre; ++s2)
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb)
                hbw[s2][nb] = img_load<T>(hrs, lane * E * (int)sizeof(T), (nb * KSHD + s2) * 64 * E * (int)sizeof(T));
    }
    // d head: row-major store (wgrad operand) and the head-bias column
    // partials (one 32-column block per wave)
    if (w == 0) {
        const float* lr = lg + r * LGS + (HC / 2) * h;
        T* drow = (T*)ws.dhead + row * HC + (HC / 2) * h;
#pragma unroll
        for (int j = 0; j < HC / 2; j += 4) store4(drow + j, lr[j], lr[j + 1], lr[j + 2], lr[j + 3]);
    }
    for (int cb = w; cb < HC / 32; cb += W) {
        float cs = 0.f;
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) cs += rnd<T>(lg[(16 * h + mm) * LGS + 32 * cb + r]);
        cs = sum_halves(cs);
        if (h == 0) ws.colpart[(int64_t)tile * ws.CP + L * 2 * H + 32 * cb + r] = cs;
    }

    STAMP(9);
    // ---- backward ----
    {
        frag db[KSHD];
#pragma unroll
        for (int s = 0; s < KSHD; ++s) db[s] = RT<T>::row_lds(lg + r * LGS, s, h);
        zero_acc<NBW>(acc);
        // dA_{L-1}^T = Head . dHead^T  (this wave's feature blocks)
        if constexpr (kHeadPre > 0) {
#pragma unroll
            for (int s2 = 0; s2 < kHeadPre; ++s2)
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) acc[nb] = MT<T>::mma(hbw[s2][nb], db[s2], acc[nb]);
        } else {
            gemm_ring<T, NBW, KSHD, 2>(acc, db, KSHD,
                                       (const T*)P.head + (int64_t)w * NBW * KSHD * 64 * E, lane);
        }
    }
    }  // kLoss
    if constexpr (MODE == kHeads) {
        // d loss / d LSTM output rows, rounded to the compute dtype (the
        // cotangent of a compute-dtype tensor)
        T* drow = (T*)rec.dhout + row * H;
#pragma unroll
        for (int i = 0; i < NBW; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                Pk<T>::store4(drow + (w * NBW + i) * 32 + 8 * g + 4 * h,
                              Pk<T>::pack(acc[i][4 * g], acc[i][4 * g + 1]),
                              Pk<T>::pack(acc[i][4 * g + 2], acc[i][4 * g + 3]));
        return;
    }
    if constexpr (MODE == kTrunkBwd) {
        // d loss / d trunk output (from the LSTM's reverse scan) into the
        // accumulator layout of this wave's feature blocks
        const T* frow = (const T*)rec.dfeat + row * H;
#pragma unroll
        for (int i = 0; i < NBW; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 v = live ? load4(frow + (w * NBW + i) * 32 + 8 * g + 4 * h)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
                acc[i][4 * g] = v.x;
                acc[i][4 * g + 1] = v.y;
                acc[i][4 * g + 2] = v.z;
                acc[i][4 * g + 3] = v.w;
            }
    }
    const int qs = col_sum16_index(lane);
    const float thr = relu_thr<T>();
#pragma unroll
    for (int l = L - 1; l >= 0; --l) {
        const float mean = mean_r[l], rstd = rstd_r[l];
        const f2 m2 = {mean, mean}, r2 = {rstd, rstd};
        const float* gm = gb + l * 2 * H;
        float* cp = ws.colpart + (int64_t)tile * ws.CP + l * 2 * H;
        f2 su2 = {0.f, 0.f}, sv2 = {0.f, 0.f};
        f2 zc2[NBW][8], u2[NBW][8];
        float cpb[NBW], cpg[NBW];  // this lane's LayerNorm bias / scale column partials
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
            const int nb = w * NBW + i;
            float pg[16], pb[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int f0 = nb * 32 + 8 * g + 4 * h;
                const float4 G = *(const float4*)(gm + f0), B = *(const float4*)(gm + H + f0);
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int k = 2 * g + p;
                    const f2 gg = p ? f2{G.z, G.w} : f2{G.x, G.y};
                    const f2 bb = p ? f2{B.z, B.w} : f2{B.x, B.y};
                    const f2 zc = Pk<T>::unpack(zr[l][i][k]) - m2;
                    const f2 xh = zc * r2;
                    const f2 y = __builtin_elementwise_fma(zc, r2 * gg, bb);
                    // ReLU' (rnd<T>(y) > 0 <=> y > thr); padding rows carry no gradient
                    const f2 dy = {((y.x > thr) & live) ? acc[i][2 * k] : 0.f,
                                   ((y.y > thr) & live) ? acc[i][2 * k + 1] : 0.f};
                    const f2 u = dy * gg;
                    const f2 pgk = dy * xh;
                    zc2[i][k] = zc;
                    u2[i][k] = u;
                    su2 += u;
                    sv2 = u * xh + sv2;
                    pg[2 * k] = pgk.x;
                    pg[2 * k + 1] = pgk.y;
                    pb[2 * k] = dy.x;
                    pb[2 * k + 1] = dy.y;
                }
            }
            // LayerNorm scale/bias partials: column sums over the tile's rows
            cpg[i] = col_sum16(pg, lane);
            cpb[i] = col_sum16(pb, lane);
        }
        auto store_cp = [&]() {
            if ((lane & 16) == 0)
#pragma unroll
                for (int i = 0; i < NBW; ++i) {
                    const int f = feat(w * NBW + i, qs, h);
                    cp[f] = cpb[i];
                    cp[H + f] = cpg[i];
                }
        };
        STAMP(10 + 3 * (L - 1 - l));
        float su = sum_halves(su2.x + su2.y);
        float sv = sum_halves(sv2.x + sv2.y);
        if (h == 0) {
            red[(w * 32 + r) * 2] = su;
            red[(w * 32 + r) * 2 + 1] = sv;
        }
        __syncthreads();
        su = red[r * 2];
        sv = red[r * 2 + 1];
#pragma unroll
        for (int v = 1; v < W; ++v) {
            su += red[(v * 32 + r) * 2];
            sv += red[(v * 32 + r) * 2 + 1];
        }
        // dZ = rstd (u - mean(u) - xh mean(u xh)) = rstd u + (-rstd^2 mean(u xh)) zc - rstd mean(u)
        const float ca = -(rstd * rstd) * (sv * invH), cb = -rstd * (su * invH);
        const f2 ca2 = {ca, ca}, cb2 = {cb, cb};
        word dzw[NBW][8];
        T* dzrow = (T*)ws.dz[l] + row * H;
#pragma unroll
        for (int i = 0; i < NBW; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const f2 d = r2 * u2[i][k] + (ca2 * zc2[i][k] + cb2);
                dzw[i][k] = Pk<T>::pack(d.x, d.y);
            }
        auto store_dz = [&]() {
            if constexpr (std::is_same<T, bf16>::value) {
                store_rows16<NBW, false>(dzrow, w, dzw, h);
                return;
            }
#pragma unroll
            for (int i = 0; i < NBW; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    Pk<T>::store4(dzrow + (w * NBW + i) * 32 + 8 * g + 4 * h, dzw[i][2 * g],
                                  dzw[i][2 * g + 1]);
        };
        if (l == 0) {
            store_cp();
            store_dz();
        }
        STAMP(11 + 3 * (L - 1 - l));
        if (l > 0) {
#pragma unroll
            for (int i = 0; i < NBW; ++i)
#pragma unroll
                for (int t = 0; t < SPB; ++t)
                    fr[((w * NBW + i) * SPB + t) * 64 + lane] = Pk<T>::frag(dzw[i], t);
            const T* img = (const T*)P.w[l] + (int64_t)w * NBW * KSH * 64 * E;
            // dA_{l-1}^T = W_l . dZ_l^T (this wave's feature blocks): weight loads
            // first, then this layer's column partials and dZ rows
            frag ra[ML_STEP_RING][NBW];
            gemm_lds_issue<T, NBW, KSH, ML_STEP_RING>(ra, img, lane);
            store_cp();
            store_dz();
            __syncthreads();
            zero_acc<NBW>(acc);
            gemm_lds_run<T, NBW, KSH, ML_STEP_RING>(acc, ra, fr, img, lane);
            STAMP(12 + 3 * (L - 1 - l));
        }
    }
    STAMP(15);
}


#ifndef ML_STEP_RTW
#define ML_STEP_RTW 1  // row tiles per workgroup of the fused MLP step (kFused; 2 measured slower)
#endif
template <typename T, int H, int L, int MODE, int HC, bool HLG = false, bool WT = false>
static int launch_step_hc(const PolicyK& P, const RolloutK& R, const int32_t* mb_seq, int mb,
                          int64_t M, const float* adv_st, const HpK& hp, const WsK& ws,
                          hipStream_t s, const RecK& rec, StepWeights<WT> sw = {}) {
    // ntiles = Mp / 32 is even (Mp is a multiple of 64)
    constexpr int RTW = (MODE == kFused && StepCfg<H>::W * ML_STEP_RTW <= 16) ? ML_STEP_RTW : 1;
    // (only the phases with the loss have an HL-Gauss instantiation)
    if constexpr (!HLG && (MODE == kFused || MODE == kHeads))
        if (P.CK)
            return launch_step_hc<T, H, L, MODE, HC, true, WT>(P, R, mb_seq, mb, M, adv_st, hp, ws,
                                                               s, rec, sw);
    auto k = ppo_step_kernel<T, H, L, MODE, HC, RTW, HLG, WT>;
    // (once per instantiation and device, kept out of graph capture)
    if (int rc = set_lds_attr((const void*)k, 160 * 1024, "ppo_step")) return rc;
    const size_t lds = step_lds<T, H, L, HC, RTW, HLG>();
    const int threads = 64 * StepCfg<H>::W * RTW;
    hipLaunchKernelGGL(k, dim3(ws.ntiles / RTW), dim3(threads), lds, s, P, R, mb_seq, mb, M,
                       adv_st, hp, ws, rec, sw);
    return MLEARN_OK;
}
// The step kernel of the policy's depth and head width (MODE: the whole
// step, or one of the recurrent update's three parts).
template <typename T, int H, int MODE = kFused>
static int launch_step(const PolicyK& P, const RolloutK& R, const int32_t* mb_seq, int mb,
                       int64_t M, const float* adv_st, const HpK& hp, const WsK& ws,
                       hipStream_t s, const RecK& rec = RecK{}) {
    return dispatch_layers(P.L, [&](auto l) {
        constexpr int L = l;
        return dispatch_head(P.HC, [&](auto hc) {
            return launch_step_hc<T, H, L, MODE, hc>(P, R, mb_seq, mb, M, adv_st, hp, ws, s, rec);
        });
    });
}
// The importance-weighted whole step (kFused): row weights seq_weight[mb_seq[f % mb]].
template <typename T, int H>
static int launch_step_weighted(const PolicyK& P, const RolloutK& R, const int32_t* mb_seq, int mb,
                                int64_t M, const float* adv_st, const HpK& hp, const WsK& ws,
                                const float* seq_weight, hipStream_t s) {
    return dispatch_layers(P.L, [&](auto l) {
        constexpr int L = l;
        return dispatch_head(P.HC, [&](auto hc) {
            return launch_step_hc<T, H, L, kFused, hc, false, true>(
                P, R, mb_seq, mb, M, adv_st, hp, ws, s, RecK{}, StepWeights<true>{seq_weight});
        });
    });
}

}  // namespace ml
