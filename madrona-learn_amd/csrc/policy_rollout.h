// Whole rollouts of the built-in synthetic sim on the feature-split policy
// body (mlearn_policy_rollout_env, mlearn_policy_rollout_env_pop): the
// rollout's store descriptor, the arguments of one step of it, and the
// single-policy and population kernels (feature split and row split).  Part
// of policy.hip's translation unit.
#pragma once

#include "policy_step.h"
#include "r16_common.h"

namespace ml {

// Whole rollout of the built-in synthetic sim in one launch
// (mlearn_policy_rollout_env): the sim step depends only on its own env, so a
// workgroup runs all T steps of its 32 envs back to back — policy step t
// (with the post-step of t - 1 and the fused env step), then the bootstrap
// critic at t = T — and takes its next env tile after that.  Identical
// per-step arithmetic and counters to T + 1 launches of policy_step_kernel.
struct RollK {
    void* obs;           // [T][ld][D] store rows (compute dtype) or null
    int32_t* actions;    // [T][ld][K]
    float* logp;         // [T][ld][K]
    float* values;       // [T][ld]
    float* rewards;      // [T][ld] store rewards
    uint8_t* dones;      // [T][ld] store dones
    float* trace;        // [T][ld] env-return trace or null
    float* bootstrap;    // [N]
    float* env_returns;  // [N]
    void* start_h;       // [C][ld][H] rnn start states (recurrent)
    void* start_c;
    int T, bptt;
    int64_t ld;
    float gamma;
    int max_wg;          // mlearn_rollout_out.max_workgroups
    float* adv;          // [T][ld] GAE advantages fused into the row-split epilogue, or null
    float gae_gamma, gae_gl;
};

#include "rollout_rows16.h"

// Launch arguments of step t of a whole rollout (t = T: the bootstrap
// critic, which stores only its values).
template <typename T> struct RollStepK {
    bool act;       // t < T: the step samples, stores and steps the env
    PostK post;     // post-step of step t - 1 into its store rows
    CarryK cy;      // (recurrent) start-state rows at the head of a bptt chunk
    EnvK env;
    T* obs_store;   // store rows of step t
    int32_t* actions;
    float* logp;
    float* values;  // the bootstrap row at t = T
};

// The one derivation of a rollout step's arguments: rollout_tile runs it in
// the kernel, launch_policy_rollout's per-step launches on the host, so both
// paths hand the body the same arguments.
template <typename T, bool RNN>
__host__ __device__ inline RollStepK<T> roll_step(int t, const RollK& rk, const EnvK& env,
                                                  const CarryK& cy0, int D, int K, int H) {
    RollStepK<T> s;
    s.act = t < rk.T;
    const int64_t so = (int64_t)t * rk.ld;
    s.post = PostK{};
    if (t > 0)
        s.post = PostK{env.rew, env.done, rk.rewards + so - rk.ld, rk.dones + so - rk.ld,
                       rk.env_returns, rk.trace ? rk.trace + so - rk.ld : nullptr, rk.gamma};
    s.cy = cy0;
    if constexpr (RNN) {
        const bool cs = s.act && t % rk.bptt == 0;
        const int64_t co = (int64_t)(t / rk.bptt) * rk.ld * H;
        s.cy.sh = cs ? (void*)((T*)rk.start_h + co) : nullptr;
        s.cy.sc = cs ? (void*)((T*)rk.start_c + co) : nullptr;
        s.cy.commit = s.act ? 1 : 0;
    }
    s.env = s.act ? env : EnvK{};
    s.obs_store = (s.act && rk.obs) ? (T*)rk.obs + so * D : nullptr;
    s.actions = s.act ? rk.actions + so * K : nullptr;
    s.logp = s.act ? rk.logp + so * K : nullptr;
    s.values = s.act ? rk.values + so : rk.bootstrap;
    return s;
}

// LayerNorm / head-bias parameters, LSTM bias, critic bins of policy P
// staged in LDS for every step of a tile (the body's first statistics
// barrier orders them)
template <typename T, int H, bool RNN, int HC>
__device__ inline void rollout_stage(const PolicyK& P, const LstmK& R) {
    constexpr int THREADS = pol_threads<H, RNN>();
    typedef PolLds<T, H, RNN, HC, THREADS / 64> LY;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* gb = (float*)(smem + LY::F32) + LY::gb;
    float* rbias = gb + LY::rbias(P.L);
    float* bins = gb + LY::bins(P.L);
    const int tid = threadIdx.x;
    for (int i = tid; i < LY::npar(P.L); i += THREADS) gb[i] = pol_param<H>(P, P.L, i);
    if constexpr (RNN)
        for (int i = tid; i < 4 * H; i += THREADS) rbias[i] = R.bias[i];
    stage_critic_bins(P, bins, nullptr, tid, THREADS);
}

// All T steps + the bootstrap of one 32-env tile (first: the workgroup's
// first tile, whose step 0 needs no leading barrier; RESTAGE: a later tile
// may belong to another policy, whose parameters are staged after that
// barrier).
template <typename T, int H, bool RNN, int HC, bool RESTAGE>
__device__ inline void rollout_tile(const PolicyK& P, const float* __restrict__ obs, int64_t N,
                                    const RollK& rk, uint32_t k0, uint32_t k1,
                                    const uint64_t* step_ctr, uint32_t eoff, const LstmK& R,
                                    const CarryK& cy0, const EnvK& env, int tile, bool first) {
#pragma clang loop unroll(disable)
    for (int t = 0; t <= rk.T; ++t) {
        // the previous step's LDS reads (and its env outputs, read by this
        // step's post-step and first product) are ordered by the barrier
        if (t > 0 || !first) __syncthreads();
        if (RESTAGE && t == 0 && !first) rollout_stage<T, H, RNN, HC>(P, R);
        const RollStepK<T> s = roll_step<T, RNN>(t, rk, env, cy0, P.D, P.K, H);
        policy_step_body<T, H, RNN, HC, pol_maxw<RNN>(), true>(
            P, obs, N, s.obs_store, s.actions, s.logp, s.values, k0, k1, step_ctr, (uint64_t)t, eoff,
            1, s.post, R, s.cy, EvalK{}, s.env, tile);
    }
}

template <typename T, int H, bool RNN, int HC>
__global__ __launch_bounds__((pol_threads<H, RNN>())) __attribute__((amdgpu_waves_per_eu(RNN ? ML_ROLL_RNN_WAVES : ML_ROLL_MLP_WAVES, 8))) void policy_rollout_kernel(
    PolicyK P, const float* __restrict__ obs, int64_t N, RollK rk, uint32_t k0, uint32_t k1,
    const uint64_t* step_ctr, uint32_t eoff, LstmK R, CarryK cy0, EnvK env) {
    const int ntiles = (int)((N + 31) / 32);
    rollout_stage<T, H, RNN, HC>(P, R);  // once: every tile has the same policy
    for (int tile = blockIdx.x; tile < ntiles; tile += (int)gridDim.x)
        rollout_tile<T, H, RNN, HC, false>(P, obs, N, rk, k0, k1, step_ctr, eoff, R, cy0, env,
                                           tile, tile == (int)blockIdx.x);
}

// A population's whole rollouts in one launch (mlearn_policy_rollout_env_pop):
// policy p's launch arguments are entry p of a device array written once by
// mlearn_policy_pop_prepare; global tile g is tile g % tpp of policy g / tpp,
// dealt round-robin over one workgroup per resident slot like the
// single-policy launch, so P launches of B / 32 workgroups become one launch
// that fills the chip.  Per tile the same body and arguments as policy p's own
// launch: the same bits.
struct PopEntry {
    PolicyK P;
    const float* obs;
    RollK rk;
    uint32_t eoff;
    LstmK R;
    CarryK cy;
    EnvK env;
};

template <typename T, int H, bool RNN, int HC>
__global__ __launch_bounds__((pol_threads<H, RNN>())) __attribute__((amdgpu_waves_per_eu(RNN ? ML_ROLL_RNN_WAVES : ML_ROLL_MLP_WAVES, 8))) void policy_rollout_pop_kernel(
    const PopEntry* __restrict__ pop, int npol, int64_t N, uint32_t k0, uint32_t k1,
    const uint64_t* step_ctr) {
    const int tpp = (int)((N + 31) / 32);
    const int ntiles = npol * tpp;
    for (int g = blockIdx.x; g < ntiles; g += (int)gridDim.x) {
        const int p = __builtin_amdgcn_readfirstlane(g / tpp);
        const PopEntry& e = pop[p];
        const bool first = g == (int)blockIdx.x;
        if (first) rollout_stage<T, H, RNN, HC>(e.P, e.R);
        rollout_tile<T, H, RNN, HC, true>(e.P, e.obs, N, e.rk, k0, k1, step_ctr, e.eoff, e.R,
                                          e.cy, e.env, g - p * tpp, first);
    }
}

// A population's whole rollouts on the row-split kernel (the library's
// choice where rollout16_pop_eligible): global 16-env tile g is tile g % tpp
// of policy g / tpp (tpp = N / 16, a multiple of 8), dealt in rounds of 8
// consecutive tiles per workgroup, so all 8 waves of a workgroup hold tiles of
// one policy in every round; a workgroup restages that policy's W1 / head /
// LayerNorm images when its round's policy is not the one staged (the
// barriers are workgroup-uniform).  Per tile the body and arguments of the
// policy's own rollout16_kernel launch: the same bits.
__global__ __launch_bounds__(64 * kR16Waves) __attribute__((amdgpu_waves_per_eu(2, 2))) void rollout16_pop_kernel(
    const PopEntry* __restrict__ pop, int npol, int64_t N, uint32_t k0, uint32_t k1,
    const uint64_t* step_ctr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* tab = (int*)(smem + R16Lay<kR16HC>::OffTab);
    const uint64_t step0 = step_ctr ? *step_ctr : 0ull;
    const int tpp = (int)(N / 16), ntile = npol * tpp;
    const int TW = (int)gridDim.x * kR16Waves;
    int cur = -1;
#pragma clang loop unroll(disable)
    for (int t0 = (int)blockIdx.x * kR16Waves; t0 < ntile; t0 += TW) {
        const int p = __builtin_amdgcn_readfirstlane(t0 / tpp);
        const PopEntry& e = pop[p];
        if (p != cur) {
            if (cur >= 0) __syncthreads();  // every wave is past its reads of the old images
            r16_stage(e.P, smem, tid);
            if (tid <= MLEARN_MAX_GROUPS) tab[tid] = e.P.off[tid];
            __syncthreads();
            cur = p;
        }
        if (wave >= kR16Waves / 2 && t0 + TW >= ntile) __builtin_amdgcn_s_setprio(1);  // (rollout16_kernel)
        r16_roll_tile(e.P, e.obs, e.rk, k0, k1, step0, e.eoff, e.env, t0 + wave - p * tpp, tid,
                      smem);
    }
}

}  // namespace ml
