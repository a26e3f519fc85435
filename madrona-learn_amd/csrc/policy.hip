// Fused rollout step: ObservationsCaster -> MLP trunk (Dense no-bias ->
// LayerNorm -> ReLU per layer) -> actor logits + critic -> Gumbel-max sample
// -> rollout store, in ONE launch per step (the reference runs these as
// dozens of XLA fusions per step inside rollout_loop, rollouts.py:867-901).
//
// Reference numerics mirrored (models.py:46-56, 99-154; flax 0.8.1):
//   Dense output rounded to the compute dtype; LayerNorm statistics in f32
//   with fast variance max(E[x^2]-E[x]^2, 0), eps 1e-6, y = (x-mean)*(rstd*g)+b
//   rounded to the compute dtype; heads: rnd(rnd(x.W) + rnd(b)); critic and
//   logits upcast to f32 (dists.py:22, models.py:154).

#include <string>
#include <vector>

#include "dispatch.h"
#include "policy_gathered.h"
#include "policy_rollout.h"
#include "policy_step.h"

namespace ml {

PolicyK make_policy_k(const mlearn_mlp_policy& p) {
    PolicyK k;
    k.D = p.obs_dim;
    k.H = p.hidden;
    k.L = p.num_layers;
    k.K = p.actions.num_groups;
    k.A = p.actions.num_logits;
    k.CB = p.critic_bins;
    k.HC = head_cols(p);
    k.CK = p.critic_kind;
    for (int i = 0; i <= MLEARN_MAX_GROUPS; ++i) k.off[i] = p.actions.offsets[i];
    for (int l = 0; l < MLEARN_MAX_LAYERS; ++l) {
        k.wt[l] = p.w_t[l];
        k.w[l] = p.w[l];
        k.lns[l] = p.ln_scale[l];
        k.lnb[l] = p.ln_bias[l];
    }
    k.head_t = p.head_t;
    k.head = p.head;
    k.head_b = p.head_bias;
    k.obs_mu = p.obs_mu;
    k.obs_inv = p.obs_inv_sigma;
    k.obs_stats = p.obs_stats;
    k.obs_tiles = p.obs_stats_tiles;
    k.obs_steps = p.obs_stats_steps;
    return k;
}

int validate_policy(const mlearn_mlp_policy* p) {
    ML_REQUIRE(p, "policy: null descriptor");
    ML_REQUIRE(p->dtype == MLEARN_DTYPE_F32 || p->dtype == MLEARN_DTYPE_BF16, "policy: bad dtype");
    ML_REQUIRE(p->hidden == 64 || p->hidden == 128 || p->hidden == 256,
               "policy: hidden must be 64, 128 or 256 (got %d)", p->hidden);
    ML_REQUIRE(p->obs_dim >= 16 && p->obs_dim <= 256 && p->obs_dim % 16 == 0,
               "policy: obs_dim must be a multiple of 16 in [16, 256] (got %d)", p->obs_dim);
    ML_REQUIRE(p->num_layers >= 1 && p->num_layers <= MLEARN_MAX_LAYERS, "policy: bad num_layers");
    const mlearn_action_layout& l = p->actions;
    ML_REQUIRE(l.num_groups >= 1 && l.num_groups <= MLEARN_MAX_GROUPS, "policy: bad num_groups");
    ML_REQUIRE(p->critic_bins == 1 || (p->critic_bins >= 3 && p->critic_bins % 2 == 1),
               "policy: critic_bins must be 1 (scalar critic) or odd >= 3 (two-hot), got %d",
               p->critic_bins);
    ML_REQUIRE(p->critic_kind == 0 || (p->critic_kind == 1 && p->critic_bins >= 3),
               "policy: critic_kind must be 0, or 1 (HL-Gauss) with odd critic_bins >= 3 (got "
               "kind %d, %d bins)", p->critic_kind, p->critic_bins);
    ML_REQUIRE(l.num_logits >= 1 && l.num_logits + p->critic_bins <= MLEARN_HEAD_COLS_MAX,
               "policy: actor logits + critic outputs must be <= %d (got %d + %d)",
               MLEARN_HEAD_COLS_MAX, l.num_logits, p->critic_bins);
    ML_REQUIRE(l.offsets[0] == 0 && l.offsets[l.num_groups] == l.num_logits,
               "policy: bad action offsets");
    for (int k = 0; k < l.num_groups; ++k)
        ML_REQUIRE(l.offsets[k + 1] > l.offsets[k], "policy: empty action group %d", k);
    for (int i = 0; i < p->num_layers; ++i)
        ML_REQUIRE(p->w_t[i] && (i == 0 || p->w[i]) && p->ln_scale[i] && p->ln_bias[i],
                   "policy: null layer %d weights", i);
    ML_REQUIRE(p->head_t && p->head && p->head_bias, "policy: null head weights");
    ML_REQUIRE(!p->obs_mu == !p->obs_inv_sigma, "policy: obs_mu / obs_inv_sigma");
    ML_REQUIRE(!p->obs_stats || (p->obs_stats_steps >= 1 && p->obs_stats_tiles >= 1),
               "policy: obs_stats needs obs_stats_steps and obs_stats_tiles");
    return MLEARN_OK;
}

// A feed-forward policy, or a recurrent one when lstm is given.
static int validate_any(const mlearn_mlp_policy* policy, const mlearn_lstm* lstm) {
    return lstm ? validate_lstm(policy, lstm) : validate_policy(policy);
}

// mlearn_post_step -> PostK (null: no post-step)
static int make_post_k(const mlearn_post_step* post, const char* who, PostK* pk) {
    *pk = PostK{};
    if (!post) return MLEARN_OK;
    ML_REQUIRE(post->rewards && post->dones && post->store_rewards && post->store_dones &&
                   post->env_returns,
               "%s: null post-step pointer", who);
    *pk = PostK{post->rewards, post->dones, post->store_rewards, post->store_dones,
                post->env_returns, post->env_returns_trace, post->gamma};
    return MLEARN_OK;
}

static int launch_rollout16_pop(const PopEntry* pop, int npol, int64_t N, uint32_t k0, uint32_t k1,
                                const uint64_t* step_ctr, hipStream_t s) {
    constexpr int lds = (int)R16Lay<kR16HC>::Lds;
    // (once per device, kept out of graph capture)
    if (set_lds_attr((const void*)rollout16_pop_kernel, lds, "rollout16_pop")) return MLEARN_EHIP;
    const int cus = device_cus();
    const int64_t rounds_of_8 = (int64_t)npol * (N / 16) / kR16Waves;
    int64_t grid = cus > 0 ? cus : 256;
    if (grid > rounds_of_8) grid = rounds_of_8;
    hipLaunchKernelGGL(rollout16_pop_kernel, dim3((unsigned)grid), dim3(64 * kR16Waves), lds, s, pop,
                       npol, N, k0, k1, step_ctr);
    return check_launch("policy_rollout_env_pop (row split)");
}

constexpr int kPolLdsLimit = 128 * 1024;  // dynamic-LDS limit the feature-split policy kernels ask for

// f(T, H, HC, RNN) for a validated policy (recurrent when lstm is given)
template <typename F>
static auto dispatch_policy(const mlearn_mlp_policy& p, const mlearn_lstm* lstm, F&& f) {
    return dispatch_policy(p.dtype, p.hidden, head_cols(p), lstm != nullptr, f);
}

// Launch shape of one instantiation of the feature-split policy kernels.
template <typename T, int H, bool RNN, int HC> struct PolLaunch {
    static constexpr int threads = pol_threads<H, RNN>();
    static size_t lds(int L) { return PolLds<T, H, RNN, HC, threads / 64>::bytes(L); }
    // the kernel's dynamic-LDS limit (once per instantiation and device, kept
    // out of graph capture)
    static int prepare(const void* kern, const char* name) {
        return set_lds_attr(kern, kPolLdsLimit, name);
    }
};

template <typename T, int H, bool RNN, int HC>
static int launch_policy_step(const PolicyK& P, const float* obs, int64_t N, void* obs_store,
                              int32_t* actions, float* logp, float* values, uint32_t k0, uint32_t k1,
                              const uint64_t* step_ctr, uint64_t step, uint32_t eoff, int sample,
                              const PostK& post, const LstmK& R, const CarryK& cy, const EvalK& ev,
                              const EnvK& env, hipStream_t s) {
    typedef PolLaunch<T, H, RNN, HC> PL;
    auto kern = policy_step_kernel<T, H, RNN, HC>;
    if (int rc = PL::prepare((const void*)kern, "policy_rollout_step")) return rc;
    const int grid = (int)((N + 31) / 32);
#ifdef ML_STAMPS
    EvalK evs = ev;
    evs.stamps = g_pol_stamp_buf;
#else
    const EvalK& evs = ev;
#endif
    hipLaunchKernelGGL(kern, dim3(grid), dim3(PL::threads), PL::lds(P.L), s, P, obs, N,
                       (T*)obs_store, actions, logp, values, k0, k1, step_ctr, step, eoff, sample,
                       post, R, cy, evs, env);
    return check_launch("policy_rollout_step");
}

// Workgroups of a whole-rollout launch of `kern` over `tiles` env tiles: one
// per resident slot, at most max_wg (> 0) and one per tile; -1 without an
// occupancy answer.
template <typename PL>
static int64_t capped_slots(const void* kern, const char* name, int L, int64_t tiles, int max_wg) {
    // (the occupancy answer needs the raised limit; a refusal reads as no answer
    // here, and the launcher reports it)
    if (PL::prepare(kern, name)) return -1;
    int64_t slots = resident_slots(kern, PL::threads, PL::lds(L));
    if (slots <= 0) return -1;
    if (max_wg > 0 && max_wg < slots) slots = max_wg;
    return tiles < slots ? tiles : slots;
}

// Workgroups of the whole-rollout launch (-1: per-step launches): max_wg < 0
// asks for the per-step launches.
template <typename T, int H, bool RNN, int HC>
static int64_t rollout_grid(int L, int64_t N, int max_wg) {
    if (max_wg < 0) return -1;
    // one workgroup per resident slot, tiles dealt round-robin (tile =
    // blockIdx + k * grid): at the headline's 2 048 tiles on 768 slots every
    // CU holds workgroups b, b + 256, b + 512 with 3 + 3 + 2 = 8 tiles, the
    // chip's mean.  The earlier grid of ceil(tiles / 3) = 683 workgroups left
    // CUs with 9 or 6 tiles: 1.66 -> 1.45 ms per rollout, 10.01 -> 9.80 ms
    // per update (profiles/r04_rollout_grid_ab.txt).  The W = 8 share (256
    // tiles) keeps one tile per workgroup.
    return capped_slots<PolLaunch<T, H, RNN, HC>>((const void*)policy_rollout_kernel<T, H, RNN, HC>,
                                                  "policy_rollout_env", L, (N + 31) / 32, max_wg);
}

// The whole rollout as one launch (every env tile gets a resident workgroup,
// or tiles run in series inside the workgroups), or T + 1 per-step launches
// of the same body when max_wg < 0.
template <typename T, int H, bool RNN, int HC>
static int launch_policy_rollout(const PopEntry& e, int64_t N, uint32_t k0, uint32_t k1,
                                 const uint64_t* step_ctr, hipStream_t s) {
    typedef PolLaunch<T, H, RNN, HC> PL;
    auto kern = policy_rollout_kernel<T, H, RNN, HC>;
    if (int rc = PL::prepare((const void*)kern, "policy_rollout_env")) return rc;
    const int64_t grid = rollout_grid<T, H, RNN, HC>(e.P.L, N, e.rk.max_wg);
    if (grid > 0) {
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(PL::threads), PL::lds(e.P.L), s, e.P,
                           e.obs, N, e.rk, k0, k1, step_ctr, e.eoff, e.R, e.cy, e.env);
        return check_launch("policy_rollout_env");
    }
    // max_workgroups < 0 (or no occupancy answer): the same body as
    // T + 1 launches of the per-step kernel (same bits)
    for (int t = 0; t <= e.rk.T; ++t) {
        const RollStepK<T> st = roll_step<T, RNN>(t, e.rk, e.env, e.cy, e.P.D, e.P.K, H);
        if (int rc = launch_policy_step<T, H, RNN, HC>(
                e.P, e.obs, N, st.obs_store, st.actions, st.logp, st.values, k0, k1, step_ctr,
                (uint64_t)t, e.eoff, 1, st.post, e.R, st.cy, EvalK{}, st.env, s))
            return rc;
    }
    return MLEARN_OK;
}

// Workgroups of the population launch: one per resident slot of the
// population kernel, at most one per tile; max_wg > 0 caps the grid (tiles of
// several policies in series per workgroup, each move to another policy's
// tile restaging its parameters).
template <typename T, int H, bool RNN, int HC>
static int64_t rollout_pop_grid(int L, int64_t tiles, int max_wg) {
    return capped_slots<PolLaunch<T, H, RNN, HC>>(
        (const void*)policy_rollout_pop_kernel<T, H, RNN, HC>, "policy_rollout_env_pop", L, tiles,
        max_wg);
}

template <typename T, int H, bool RNN, int HC>
static int launch_policy_rollout_pop(int L, const PopEntry* pop, int npol, int64_t N, uint32_t k0,
                                     uint32_t k1, const uint64_t* step_ctr, int max_wg,
                                     hipStream_t s) {
    typedef PolLaunch<T, H, RNN, HC> PL;
    auto kern = policy_rollout_pop_kernel<T, H, RNN, HC>;
    if (int rc = PL::prepare((const void*)kern, "policy_rollout_env_pop")) return rc;
    const int64_t grid =
        rollout_pop_grid<T, H, RNN, HC>(L, (int64_t)npol * ((N + 31) / 32), max_wg);
    ML_REQUIRE(grid > 0, "policy_rollout_env_pop: no occupancy answer for the population kernel");
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(PL::threads), PL::lds(L), s, pop, npol, N,
                       k0, k1, step_ctr);
    return check_launch("policy_rollout_env_pop");
}

static int rollout_step_entry(const mlearn_mlp_policy* policy, const mlearn_lstm* lstm,
                              const mlearn_lstm_carry* carry, const float* obs, int64_t N,
                              void* obs_store, int32_t* actions, float* log_probs, float* values,
                              uint32_t k0, uint32_t k1, const uint64_t* step_ctr, uint64_t step,
                              uint32_t env_offset, int32_t sample, const mlearn_post_step* post,
                              mlearn_stream_t stream, EvalK ev = EvalK{},
                              const mlearn_dummy_env* denv = nullptr) {
    if (int rc = validate_any(policy, lstm)) return rc;
    ML_REQUIRE(N >= 0, "policy_rollout_step: N < 0");
    if (N == 0) return MLEARN_OK;
    ML_REQUIRE(obs, "policy_rollout_step: null obs");
    ML_REQUIRE(!actions || log_probs || !sample, "policy_rollout_step: sampling needs log_probs");
    ML_REQUIRE(!ev.actions || (!actions && log_probs && ev.entropies),
               "policy_evaluate: needs log_probs and entropies outputs");
    ML_REQUIRE(actions || values || ev.actions, "policy_rollout_step: nothing to compute");
    ML_REQUIRE(!policy->obs_stats || !actions || policy->obs_stats_tiles >= (N + 31) / 32,
               "policy_rollout_step: obs_stats_tiles %lld < ceil(N / 32)",
               (long long)policy->obs_stats_tiles);
    ML_REQUIRE((uintptr_t)obs % 16 == 0, "policy_rollout_step: obs must be 16-byte aligned");
    ML_REQUIRE(!obs_store || (uintptr_t)obs_store % 16 == 0,
               "policy_rollout_step: obs_store must be 16-byte aligned");
    PostK pk;
    if (int rc = make_post_k(post, "policy_rollout_step", &pk)) return rc;
    EnvK ek{};
    if (denv) {
        ML_REQUIRE(actions, "policy_rollout_step_env: the fused env step needs actions");
        ML_REQUIRE(denv->state && denv->obs && denv->rewards && denv->dones,
                   "policy_rollout_step_env: null env pointer");
        ML_REQUIRE(denv->obs == obs,
                   "policy_rollout_step_env: env->obs must be the launch's obs input (the next "
                   "observations overwrite it in place)");
        ML_REQUIRE((uintptr_t)denv->state % 16 == 0, "policy_rollout_step_env: state alignment");
        ML_REQUIRE(!post || (post->rewards == denv->rewards && post->dones == denv->dones),
                   "policy_rollout_step_env: post-step must read the env's rewards / dones");
        ek = EnvK{(int4*)denv->state, denv->obs, denv->rewards, denv->dones, denv->k0, denv->k1,
                  denv->env_offset};
    }
    LstmK R{};
    CarryK cy{};
    if (lstm) {
        ML_REQUIRE(carry && carry->h && carry->c, "lstm rollout step: null carry");
        ML_REQUIRE(!carry->start_h == !carry->start_c, "lstm rollout step: start_h / start_c");
        ML_REQUIRE((uintptr_t)carry->h % 16 == 0 && (uintptr_t)carry->c % 16 == 0,
                   "lstm rollout step: carry must be 16-byte aligned");
        R = make_lstm_k(*lstm);
        cy = CarryK{carry->h, carry->c, carry->start_h, carry->start_c, carry->commit, carry->clear};
    }
    PolicyK P = make_policy_k(*policy);
    hipStream_t s = S(stream);
    return dispatch_policy(*policy, lstm, [&](auto t, auto h, auto hc, auto rnn) {
        return launch_policy_step<tag_t<decltype(t)>, h, rnn, hc>(
            P, obs, N, obs_store, actions, log_probs, values, k0, k1, step_ctr, step, env_offset,
            sample, pk, R, cy, ev, ek, s);
    });
}

}  // namespace ml

using namespace ml;

extern "C" int mlearn_policy_rollout_step(const mlearn_mlp_policy* policy, const float* obs,
                                          int64_t N, void* obs_store, int32_t* actions,
                                          float* log_probs, float* values, uint32_t k0,
                                          uint32_t k1, const uint64_t* step_ctr, uint64_t step,
                                          uint32_t env_offset, int32_t sample,
                                          const mlearn_post_step* post, mlearn_stream_t stream) {
    return rollout_step_entry(policy, nullptr, nullptr, obs, N, obs_store, actions, log_probs,
                              values, k0, k1, step_ctr, step, env_offset, sample, post, stream);
}

// Validated launch arguments of one policy's whole rollout
// (mlearn_policy_rollout_env / one entry of a population).
static int rollout_env_args(const mlearn_mlp_policy* policy, const mlearn_lstm* lstm,
                            const mlearn_lstm_carry* carry, const float* obs, int64_t N,
                            const mlearn_rollout_out* out, uint32_t env_offset,
                            const mlearn_dummy_env* denv, PopEntry* e) {
    if (int rc = validate_any(policy, lstm)) return rc;
    ML_REQUIRE(N >= 0, "policy_rollout_env: N < 0");
    ML_REQUIRE(obs && out && denv, "policy_rollout_env: null obs / out / env");
    ML_REQUIRE(out->T >= 1 && out->bptt_len >= 1 && out->T % out->bptt_len == 0 && out->ld >= N,
               "policy_rollout_env: bad T / bptt / ld");
    ML_REQUIRE(out->actions && out->log_probs && out->values && out->rewards && out->dones &&
                   out->bootstrap && out->env_returns,
               "policy_rollout_env: null store pointer");
    ML_REQUIRE(denv->state && denv->obs == obs && denv->rewards && denv->dones,
               "policy_rollout_env: env->obs must be the obs input; null env pointer");
    ML_REQUIRE((uintptr_t)obs % 16 == 0 && (uintptr_t)denv->state % 16 == 0 &&
                   (!out->obs || (uintptr_t)out->obs % 16 == 0),
               "policy_rollout_env: obs / state / store alignment");
    ML_REQUIRE(!policy->obs_stats || policy->obs_stats_tiles >= (N + 31) / 32,
               "policy_rollout_env: obs_stats_tiles %lld < ceil(N / 32)",
               (long long)policy->obs_stats_tiles);
    *e = PopEntry{};
    if (lstm) {
        ML_REQUIRE(carry && carry->h && carry->c && out->start_h && out->start_c,
                   "lstm rollout: null carry / start states");
        e->R = make_lstm_k(*lstm);
        e->cy = CarryK{carry->h, carry->c, nullptr, nullptr, 1, nullptr};
    }
    e->rk = RollK{out->obs, out->actions, out->log_probs, out->values, out->rewards, out->dones,
                  out->env_returns_trace, out->bootstrap, out->env_returns, out->start_h,
                  out->start_c, out->T, out->bptt_len, out->ld, out->gamma, out->max_workgroups,
                  nullptr, out->gae_gamma, out->gae_gamma_lambda};
    e->env = EnvK{(int4*)denv->state, denv->obs, denv->rewards, denv->dones, denv->k0, denv->k1,
                  denv->env_offset};
    e->P = make_policy_k(*policy);
    e->obs = obs;
    e->eoff = env_offset;
    return MLEARN_OK;
}

extern "C" int mlearn_policy_rollout_env(const mlearn_mlp_policy* policy, const mlearn_lstm* lstm,
                                         const mlearn_lstm_carry* carry, const float* obs,
                                         int64_t N, const mlearn_rollout_out* out, uint32_t k0,
                                         uint32_t k1, const uint64_t* step_ctr,
                                         uint32_t env_offset, const mlearn_dummy_env* denv,
                                         mlearn_stream_t stream) {
    PopEntry e;
    const int rc = rollout_env_args(policy, lstm, carry, obs, N, out, env_offset, denv, &e);
    if (rc) return rc;
    if (N == 0) return MLEARN_OK;
    hipStream_t s = S(stream);
    ML_REQUIRE(out->policy_kernel >= 0 && out->policy_kernel <= 2,
               "policy_rollout_env: policy_kernel %d", out->policy_kernel);
    const bool r16 = rollout16_eligible(e.P, N, out->max_workgroups,
                                        policy->dtype == MLEARN_DTYPE_BF16, lstm != nullptr);
    ML_REQUIRE(out->policy_kernel != 2 || r16,
               "policy_rollout_env: policy_kernel 2 (row split) needs the row-split step's policy "
               "shape, <= 8 action groups, no observation normaliser, max_workgroups 0 and N of "
               "32768 or a multiple of 256 from 65536");
    ML_REQUIRE(!out->advantages || out->ld == N,
               "policy_rollout_env: advantages need ld == N (ld %lld, N %lld)",
               (long long)out->ld, (long long)N);
    RollK rk2 = e.rk;
    int rc2;
    if (r16 && out->policy_kernel != 1) {
        if (out->advantages && out->T <= 32) rk2.adv = out->advantages;  // fused GAE
        rc2 = launch_rollout16(e.P, obs, N, rk2, k0, k1, step_ctr, env_offset, e.env, s);
    } else {  // the feature-split kernel for the policy's dtype / width / head
        rc2 = dispatch_policy(*policy, lstm, [&](auto t, auto h, auto hc, auto rnn) {
            return launch_policy_rollout<tag_t<decltype(t)>, h, rnn, hc>(e, N, k0, k1, step_ctr, s);
        });
    }
    // GAE as its own launch, unless the row-split rollout fused it
    if (rc2 || !out->advantages || rk2.adv) return rc2;
    return mlearn_gae_f32(out->rewards, out->values, out->dones, out->bootstrap, out->advantages,
                          nullptr, out->T, N, out->gae_gamma, out->gae_gamma_lambda, stream);
}

extern "C" int64_t mlearn_policy_pop_bytes(int32_t num_policies) {
    return num_policies > 0 ? (int64_t)num_policies * (int64_t)sizeof(PopEntry) : 0;
}

extern "C" int mlearn_policy_pop_prepare(const mlearn_mlp_policy* policies,
                                         const mlearn_lstm* lstms,
                                         const mlearn_lstm_carry* carries,
                                         const float* const* obs, int64_t N,
                                         const mlearn_rollout_out* outs,
                                         const uint32_t* env_offsets,
                                         const mlearn_dummy_env* envs, int32_t num_policies,
                                         void* pop, mlearn_stream_t stream) {
    ML_REQUIRE(num_policies >= 1 && policies && obs && outs && env_offsets && envs && pop,
               "policy_pop_prepare: null argument or no policies");
    for (int p = 0; p < num_policies; ++p)
        ML_REQUIRE(!outs[p].advantages,
                   "policy_pop_prepare: advantages (fused GAE) is a single-policy rollout option");
    ML_REQUIRE(N >= 1, "policy_pop_prepare: N < 1");
    std::vector<PopEntry> h((size_t)num_policies);
    for (int p = 0; p < num_policies; ++p) {
        const mlearn_mlp_policy& a = policies[p];
        const mlearn_mlp_policy& b = policies[0];
        ML_REQUIRE(a.dtype == b.dtype && a.hidden == b.hidden && a.num_layers == b.num_layers &&
                       a.obs_dim == b.obs_dim && head_cols(a) == head_cols(b) &&
                       a.critic_kind == b.critic_kind,
                   "policy_pop_prepare: policy %d's shape differs from policy 0's", p);
        ML_REQUIRE(!lstms == !carries, "policy_pop_prepare: lstms and carries go together");
        const int rc = rollout_env_args(&a, lstms ? &lstms[p] : nullptr,
                                        carries ? &carries[p] : nullptr, obs[p], N, &outs[p],
                                        env_offsets[p], &envs[p], &h[(size_t)p]);
        if (rc) return rc;
        ML_REQUIRE(outs[p].max_workgroups == 0,
                   "policy_pop_prepare: the population launch has its own grid (max_workgroups 0)");
        ML_REQUIRE(!a.obs_mu == !b.obs_mu && !a.obs_stats == !b.obs_stats,
                   "policy_pop_prepare: policy %d's observation normaliser differs from policy 0's",
                   p);
    }
    // ordered after the caller's earlier work on its stream (a previous
    // population launch may still read the buffer), and complete on return
    // (the host staging vector dies with this call)
    hipError_t err = hipMemcpyAsync(pop, h.data(), h.size() * sizeof(PopEntry),
                                    hipMemcpyHostToDevice, S(stream));
    if (err == hipSuccess) err = hipStreamSynchronize(S(stream));
    if (err != hipSuccess) {
        set_error("policy_pop_prepare: hipMemcpy: %s", hipGetErrorString(err));
        return MLEARN_EHIP;
    }
    return MLEARN_OK;
}

extern "C" int mlearn_policy_rollout_env_pop(const mlearn_mlp_policy* policy0,
                                             const mlearn_lstm* lstm0, const void* pop,
                                             int32_t num_policies, int64_t N, uint32_t k0,
                                             uint32_t k1, const uint64_t* step_ctr,
                                             int32_t max_workgroups, mlearn_stream_t stream) {
    if (int rc = validate_any(policy0, lstm0)) return rc;
    ML_REQUIRE(pop && num_policies >= 1 && N >= 1 && step_ctr,
               "policy_rollout_env_pop: null pop / step counter, or no work");
    ML_REQUIRE(max_workgroups >= 0, "policy_rollout_env_pop: max_workgroups < 0");
    const int L = policy0->num_layers;
    const PopEntry* e = (const PopEntry*)pop;
    hipStream_t s = S(stream);
    if (rollout16_pop_eligible(make_policy_k(*policy0), N, num_policies, max_workgroups,
                               policy0->dtype == MLEARN_DTYPE_BF16, lstm0 != nullptr))
        return launch_rollout16_pop(e, num_policies, N, k0, k1, step_ctr, s);
    return dispatch_policy(*policy0, lstm0, [&](auto t, auto h, auto hc, auto rnn) {
        return launch_policy_rollout_pop<tag_t<decltype(t)>, h, rnn, hc>(
            L, e, num_policies, N, k0, k1, step_ctr, max_workgroups, s);
    });
}

extern "C" int32_t mlearn_policy_rollout_pop_kernel(const mlearn_mlp_policy* policy,
                                                    const mlearn_lstm* lstm, int64_t N,
                                                    int32_t num_policies,
                                                    int32_t max_workgroups) {
    if (validate_any(policy, lstm) || N < 1 || num_policies < 1 || max_workgroups < 0) return -1;
    return rollout16_pop_eligible(make_policy_k(*policy), N, num_policies, max_workgroups,
                                  policy->dtype == MLEARN_DTYPE_BF16, lstm != nullptr)
               ? 2
               : 1;
}

extern "C" int64_t mlearn_policy_rollout_pop_workgroups(const mlearn_mlp_policy* policy,
                                                        const mlearn_lstm* lstm, int64_t N,
                                                        int32_t num_policies,
                                                        int32_t max_workgroups) {
    if (validate_any(policy, lstm) || N < 1 || num_policies < 1 || max_workgroups < 0) return -1;
    const int L = policy->num_layers;
    const int64_t tiles = (int64_t)num_policies * ((N + 31) / 32);
    return dispatch_policy(*policy, lstm, [&](auto t, auto h, auto hc, auto rnn) {
        return rollout_pop_grid<tag_t<decltype(t)>, h, rnn, hc>(L, tiles, max_workgroups);
    });
}

extern "C" int64_t mlearn_policy_rollout_workgroups(const mlearn_mlp_policy* policy,
                                                    const mlearn_lstm* lstm, int64_t N,
                                                    int32_t max_workgroups) {
    if (validate_any(policy, lstm) || N < 1) return -1;
    const int L = policy->num_layers;
    return dispatch_policy(*policy, lstm, [&](auto t, auto h, auto hc, auto rnn) {
        return rollout_grid<tag_t<decltype(t)>, h, rnn, hc>(L, N, max_workgroups);
    });
}

extern "C" int32_t mlearn_policy_rollout_kernel(const mlearn_mlp_policy* policy,
                                                const mlearn_lstm* lstm, int64_t N,
                                                int32_t max_workgroups, int32_t requested) {
    if (validate_any(policy, lstm) || N < 1 || requested < 0 || requested > 2) return -1;
    const bool r16 = rollout16_eligible(make_policy_k(*policy), N, max_workgroups,
                                        policy->dtype == MLEARN_DTYPE_BF16, lstm != nullptr);
    if (requested == 2 && !r16) return -1;
    return r16 && requested != 1 ? 2 : 1;
}

extern "C" int mlearn_policy_rollout_step_env(const mlearn_mlp_policy* policy, const float* obs,
                                              int64_t N, void* obs_store, int32_t* actions,
                                              float* log_probs, float* values, uint32_t k0,
                                              uint32_t k1, const uint64_t* step_ctr, uint64_t step,
                                              uint32_t env_offset, int32_t sample,
                                              const mlearn_post_step* post,
                                              const mlearn_dummy_env* env, mlearn_stream_t stream) {
    ML_REQUIRE(env, "policy_rollout_step_env: null env descriptor");
    return rollout_step_entry(policy, nullptr, nullptr, obs, N, obs_store, actions, log_probs,
                              values, k0, k1, step_ctr, step, env_offset, sample, post, stream,
                              EvalK{}, env);
}

extern "C" int mlearn_lstm_policy_rollout_step_env(
    const mlearn_mlp_policy* policy, const mlearn_lstm* lstm, const mlearn_lstm_carry* carry,
    const float* obs, int64_t N, void* obs_store, int32_t* actions, float* log_probs,
    float* values, uint32_t k0, uint32_t k1, const uint64_t* step_ctr, uint64_t step,
    uint32_t env_offset, int32_t sample, const mlearn_post_step* post, const mlearn_dummy_env* env,
    mlearn_stream_t stream) {
    ML_REQUIRE(lstm, "lstm rollout step: null lstm descriptor");
    ML_REQUIRE(env, "policy_rollout_step_env: null env descriptor");
    return rollout_step_entry(policy, lstm, carry, obs, N, obs_store, actions, log_probs, values,
                              k0, k1, step_ctr, step, env_offset, sample, post, stream, EvalK{},
                              env);
}

extern "C" int mlearn_lstm_policy_rollout_step(
    const mlearn_mlp_policy* policy, const mlearn_lstm* lstm, const mlearn_lstm_carry* carry,
    const float* obs, int64_t N, void* obs_store, int32_t* actions, float* log_probs,
    float* values, uint32_t k0, uint32_t k1, const uint64_t* step_ctr, uint64_t step,
    uint32_t env_offset, int32_t sample, const mlearn_post_step* post, mlearn_stream_t stream) {
    ML_REQUIRE(lstm, "lstm rollout step: null lstm descriptor");
    return rollout_step_entry(policy, lstm, carry, obs, N, obs_store, actions, log_probs, values,
                              k0, k1, step_ctr, step, env_offset, sample, post, stream);
}

extern "C" int mlearn_policy_evaluate(const mlearn_mlp_policy* policy, const float* obs,
                                      int64_t N, const int32_t* actions, float* log_probs,
                                      float* entropies, float* values, mlearn_stream_t stream) {
    ML_REQUIRE(actions, "policy_evaluate: null actions");
    return rollout_step_entry(policy, nullptr, nullptr, obs, N, nullptr, nullptr, log_probs, values,
                              0, 0, nullptr, 0, 0, 0, nullptr, stream, EvalK{actions, entropies});
}

extern "C" int mlearn_lstm_policy_evaluate(const mlearn_mlp_policy* policy,
                                           const mlearn_lstm* lstm,
                                           const mlearn_lstm_carry* carry, const float* obs,
                                           int64_t N, const int32_t* actions, float* log_probs,
                                           float* entropies, float* values,
                                           mlearn_stream_t stream) {
    ML_REQUIRE(lstm, "lstm policy_evaluate: null lstm descriptor");
    ML_REQUIRE(actions, "lstm policy_evaluate: null actions");
    return rollout_step_entry(policy, lstm, carry, obs, N, nullptr, nullptr, log_probs, values, 0,
                              0, nullptr, 0, 0, 0, nullptr, stream, EvalK{actions, entropies});
}

// A table policy of mlearn_policy_step_assigned: a valid feed-forward
// descriptor without the rollout's observation statistics.
static int validate_assigned_policy(const mlearn_mlp_policy* p, const char* who) {
    if (int rc = validate_policy(p)) return rc;
    ML_REQUIRE(!p->obs_stats, "%s: obs_stats must be null (no observation statistics here)", who);
    return MLEARN_OK;
}

static int validate_assigned_count(int32_t num_policies, const char* who) {
    ML_REQUIRE(num_policies >= 1 && num_policies <= kAssignMaxPolicies,
               "%s: num_policies must be in [1, %d] (got %d)", who, kAssignMaxPolicies,
               num_policies);
    return MLEARN_OK;
}

// Count, policy and N checks of the two gathered entry points.
static int validate_gathered(const char* who, const mlearn_mlp_policy* policy0,
                             int32_t num_policies, int64_t N) {
    if (int rc = validate_assigned_count(num_policies, who)) return rc;
    if (int rc = validate_assigned_policy(policy0, who)) return rc;
    ML_REQUIRE(N >= 0 && N <= (int64_t)1 << 30, "%s: N must be in [0, 2^30] (got %lld)", who,
               (long long)N);
    return MLEARN_OK;
}

template <typename T, int H, int HC, bool MATCHED>
static int gathered_prepare() {
    return PolLaunch<T, H, false, HC>::prepare(
        (const void*)policy_step_gathered_kernel<T, H, HC, MATCHED>,
        MATCHED ? "policy_rollout_step_matched" : "policy_step_assigned");
}

// The gathered step of both entry points, behind their own argument checks
// (N >= 1): the alignment checks, the bucket launch and the step's launch.
template <bool MATCHED>
static int launch_gathered(const char* who, const mlearn_mlp_policy* policy0, int32_t num_policies,
                           const int32_t* assignments, const float* obs, int64_t N, void* obs_store,
                           int32_t* actions, float* log_probs, float* values, uint32_t k0,
                           uint32_t k1, const uint64_t* step_ctr, uint64_t step, uint32_t env_offset,
                           int32_t sample, const PostK& pk, const MatchK& mk, void* workspace,
                           mlearn_stream_t stream) {
    ML_REQUIRE((uintptr_t)obs % 16 == 0 && (uintptr_t)assignments % 16 == 0 &&
                   (uintptr_t)workspace % 16 == 0 && (uintptr_t)obs_store % 16 == 0,
               "%s: %s must be 16-byte aligned", who,
               MATCHED ? "obs, assignments, workspace and obs_store"
                       : "obs, assignments and workspace");
    const AssignWs ws = assign_ws(workspace, N, num_policies);
    hipStream_t s = S(stream);
    hipLaunchKernelGGL(assign_bucket_kernel, dim3((unsigned)((N + kBktSweep - 1) / kBktSweep)),
                       dim3(kBktThreads), 0, s, assignments, N, (int)num_policies, ws.tiles, ws.map,
                       ws.ntiles);
    if (int rc = check_launch((std::string(who) + " (buckets)").c_str())) return rc;
    const int L = policy0->num_layers;
    return dispatch_policy(*policy0, nullptr, [&](auto t, auto hh, auto hc, auto) {
        typedef tag_t<decltype(t)> T;
        constexpr int H = decltype(hh)::value, HC = decltype(hc)::value;
        typedef PolLaunch<T, H, false, HC> PL;
        if (int rc = gathered_prepare<T, H, HC, MATCHED>()) return rc;
        hipLaunchKernelGGL((policy_step_gathered_kernel<T, H, HC, MATCHED>),
                           dim3((unsigned)ws.ntiles), dim3(PL::threads), PL::lds(L), s,
                           (const PolicyK*)ws.tab, (int)num_policies, (const int2*)ws.tiles,
                           (const int32_t*)ws.map, obs, N, (T*)obs_store, actions, log_probs, values,
                           k0, k1, step_ctr, step, env_offset, (int)sample, pk, mk);
        return check_launch(who);
    });
}

extern "C" int64_t mlearn_policy_assigned_bytes(int64_t N, int32_t num_policies) {
    if (N < 1 || N > (int64_t)1 << 30 || num_policies < 1 || num_policies > kAssignMaxPolicies)
        return 0;
    return assign_ws(nullptr, N, num_policies).bytes;
}

extern "C" int mlearn_policy_assigned_prepare(const mlearn_mlp_policy* policies,
                                              int32_t num_policies, void* workspace,
                                              mlearn_stream_t stream) {
    const char* who = "policy_assigned_prepare";
    if (int rc = validate_assigned_count(num_policies, who)) return rc;
    ML_REQUIRE(policies && workspace, "%s: null policies / workspace", who);
    std::vector<PolicyK> h((size_t)num_policies);
    const mlearn_mlp_policy& b = policies[0];
    for (int p = 0; p < num_policies; ++p) {
        const mlearn_mlp_policy& a = policies[p];
        if (int rc = validate_assigned_policy(&a, who)) return rc;
        ML_REQUIRE(a.dtype == b.dtype && a.obs_dim == b.obs_dim && a.hidden == b.hidden &&
                       a.num_layers == b.num_layers && a.critic_bins == b.critic_bins &&
                       a.critic_kind == b.critic_kind,
                   "%s: policy %d's dtype / obs_dim / hidden / num_layers / critic_bins / "
                   "critic_kind differ from policy 0's", who, p);
        bool same = a.actions.num_groups == b.actions.num_groups;
        for (int g = 0; same && g <= b.actions.num_groups; ++g)
            same = a.actions.offsets[g] == b.actions.offsets[g];
        ML_REQUIRE(same, "%s: policy %d's action layout differs from policy 0's", who, p);
        h[(size_t)p] = make_policy_k(a);
    }
    ML_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    // the kernel's LDS limit, here so that a captured step finds it set
    if (int rc = dispatch_policy(b, nullptr, [&](auto t, auto hh, auto hc, auto) {
            typedef tag_t<decltype(t)> T;
            if (int rc = gathered_prepare<T, hh, hc, false>()) return rc;
            return gathered_prepare<T, hh, hc, true>();
        }))
        return rc;
    // ordered after the caller's earlier work on its stream (a step may still
    // read the table), complete on return (the staging vector dies here)
    hipError_t err = hipMemcpyAsync(workspace, h.data(), h.size() * sizeof(PolicyK),
                                    hipMemcpyHostToDevice, S(stream));
    if (err == hipSuccess) err = hipStreamSynchronize(S(stream));
    if (err != hipSuccess) {
        set_error("%s: hipMemcpy: %s", who, hipGetErrorString(err));
        return MLEARN_EHIP;
    }
    return MLEARN_OK;
}

extern "C" int mlearn_policy_step_assigned(const mlearn_mlp_policy* policy0, int32_t num_policies,
                                           const int32_t* assignments, const float* obs, int64_t N,
                                           int32_t* actions, float* log_probs, float* values,
                                           uint32_t k0, uint32_t k1, const uint64_t* step_ctr,
                                           uint64_t step, uint32_t env_offset, int32_t sample,
                                           void* workspace, mlearn_stream_t stream) {
    const char* who = "policy_step_assigned";
    if (int rc = validate_gathered(who, policy0, num_policies, N)) return rc;
    ML_REQUIRE(assignments, "%s: null assignments", who);
    if (N == 0) return MLEARN_OK;
    ML_REQUIRE(obs && actions && workspace, "%s: null obs / actions / workspace", who);
    ML_REQUIRE(log_probs || !sample, "%s: sampling needs log_probs", who);
    return launch_gathered<false>(who, policy0, num_policies, assignments, obs, N, nullptr, actions,
                                  log_probs, values, k0, k1, step_ctr, step, env_offset, sample,
                                  PostK{}, MatchK{}, workspace, stream);
}

extern "C" int mlearn_policy_rollout_step_matched(
    const mlearn_mlp_policy* policy0, int32_t num_policies, const int32_t* assignments,
    const int32_t* train_col, int64_t num_train_cols, const float* obs, int64_t N,
    void* obs_store, int32_t* store_actions, float* store_log_probs, float* store_values,
    int32_t* actions, uint32_t k0, uint32_t k1, const uint64_t* step_ctr, uint64_t step,
    uint32_t env_offset, int32_t sample, const mlearn_post_step* post, void* workspace,
    mlearn_stream_t stream) {
    const char* who = "policy_rollout_step_matched";
    if (int rc = validate_gathered(who, policy0, num_policies, N)) return rc;
    ML_REQUIRE(assignments && train_col, "%s: null assignments / train_col", who);
    ML_REQUIRE(num_train_cols >= 0 && num_train_cols <= N,
               "%s: num_train_cols must be in [0, N] (got %lld)", who, (long long)num_train_cols);
    if (N == 0) return MLEARN_OK;
    ML_REQUIRE(obs && workspace, "%s: null obs / workspace", who);
    ML_REQUIRE(store_values, "%s: null store_values (the bootstrap row when actions is null)", who);
    ML_REQUIRE(!actions || (store_actions && (store_log_probs || !sample)),
               "%s: an acting step needs store_actions, and store_log_probs when sampling", who);
    ML_REQUIRE(actions || (!obs_store && !store_actions && !store_log_probs),
               "%s: the critic-only call (actions null) writes store_values only", who);
    PostK pk;
    if (int rc = make_post_k(post, who, &pk)) return rc;
    return launch_gathered<true>(who, policy0, num_policies, assignments, obs, N, obs_store, actions,
                                 store_log_probs, store_values, k0, k1, step_ctr, step, env_offset,
                                 sample, pk, MatchK{train_col, store_actions, num_train_cols},
                                 workspace, stream);
}

extern "C" int32_t mlearn_head_cols(const mlearn_mlp_policy* policy) {
    if (validate_policy(policy)) return -1;
    return head_cols(*policy);
}

#ifdef ML_STAMPS
// diagnostic builds only: phase timestamps of the rollout policy kernel
extern "C" void mlearn_debug_set_policy_stamp_buffer(uint64_t* buf) { ml::g_pol_stamp_buf = buf; }
#endif
