// PPO minibatch step up to the flat gradient (ppo.py:109-364): the launch
// sequences of the feed-forward and the recurrent update, their argument
// checks and the C ABI.  Three launches per minibatch:
//
//   step    gathers the minibatch rows straight from the [T][N] rollout store
//           (no RolloutData.minibatch copy, rollouts.py:319-329), runs trunk,
//           heads, loss and the backward pass, and writes the weight-gradient
//           operands X_l / dZ_l row-major plus column partials: the feature
//           split (ppo_step.h) or, for the headline shape, the row split
//           (ppo_rows16.h); the recurrent update runs the LSTM scans
//           (lstm_scan.h) between the feature-split kernel's phases;
//   wgrad   dW_l = X_l^T dZ_l for every weight in one launch (ppo_wgrad.h);
//   reduce  fixed-order sum of slabs and partials into the flat f32 gradient
//           and the loss / metric outputs (ppo_reduce.h).  No atomics.
// mlearn_ppo_minibatch_grad_weighted (importance-sampled minibatches) runs the
// feature split's weighted instantiation; when the metrics are recorded, the
// unweighted step before it (the recorded metric partials) and one more
// workgroup after the weight gradients ('Loss' from the weighted sums).
//
// Minibatch row f (time-major like mb['obs'] of shape [T/C, mb]):
//   tl = f / mb, m = f % mb, seq = mb_seq[m], c = seq / N, b = seq % N,
//   store row = (c * bptt + tl) * N + b  (store_row, ppo_defs.h).

#include "dispatch.h"
#include "ppo_defs.h"
#include "r16_common.h"

// (these two headers are written to be included inside namespace ml; the
// three below open it themselves)
namespace ml {
#include "lstm_scan.h"
#include "ppo_rows16.h"
}  // namespace ml

#include "ppo_reduce.h"
#include "ppo_step.h"
#include "ppo_wgrad.h"

namespace ml {

int validate_lstm(const mlearn_mlp_policy* p, const mlearn_lstm* r) {
    int rc = validate_policy(p);
    if (rc) return rc;
    ML_REQUIRE(r, "lstm: null descriptor");
    ML_REQUIRE(r->num_layers == 1, "lstm: one LSTM layer supported (got %d)", r->num_layers);
    ML_REQUIRE(r->hidden == p->hidden, "lstm: width %d must equal the MLP width %d", r->hidden,
               p->hidden);
    ML_REQUIRE(r->wi_perm && r->wi_nat && r->wh_nat && r->w_bwd && r->head_t_nat && r->bias,
               "lstm: null weight image");
    return MLEARN_OK;
}

// The kernels' view of the hyper-parameters for M rows per minibatch.
static int make_hp(const mlearn_ppo_hparams& h, int64_t M, int num_groups, bool metrics, HpK* out) {
    // (3 is not a form: the group-major launch is 4)
    ML_REQUIRE((h.wgrad_form >= 0 && h.wgrad_form <= 2) || h.wgrad_form == 4, "ppo: wgrad_form %d",
               h.wgrad_form);
    HpK hp{};
    hp.clip = h.clip_coef;
    hp.vcoef = h.value_loss_coef;
    for (int i = 0; i < MLEARN_MAX_GROUPS; ++i) {
        hp.ecoef[i] = h.entropy_coef[i];
        hp.objw[i] = h.obj_weight[i] != 0.f ? h.obj_weight[i] : 1.f;
    }
    hp.norm_adv = h.normalize_advantages;
    hp.clip_vl = h.clip_value_loss;
    hp.norm_vals = h.normalize_values;
    hp.huber = h.huber_value_loss;
    hp.loss_scale = h.loss_scale;
    hp.metrics = metrics;
    hp.wg_form = h.wgrad_form ? h.wgrad_form : ML_WG_FORM;  // 0: the library's choice
    hp.inv_s = (float)(1.0 / (double)M);
    hp.inv_sk = (float)(1.0 / ((double)M * num_groups));
    *out = hp;
    return MLEARN_OK;
}

static RolloutK make_rollout_k(const mlearn_rollout_view& ro) {
    return RolloutK{ro.obs, ro.actions, ro.log_probs, ro.advantages, ro.returns, ro.values, ro.dones,
                    ro.T, ro.bptt_len, ro.N, ro.ld ? ro.ld : ro.N};
}

template <typename T, int H>
static int launch_minibatch(const mlearn_mlp_policy& p, const mlearn_rollout_view& ro,
                            const int32_t* mb_seq, int mb, const float* adv_st,
                            const mlearn_ppo_hparams& h, float* grad, float* loss_out, void* wsp,
                            bool step_only, hipStream_t s, const float* seq_weight = nullptr) {
    const int64_t M = (int64_t)mb * ro.bptt_len;
    WsK ws;
    carve(p, M, (char*)wsp, &ws);
#ifdef ML_STAMPS
    ws.stamps = g_stamp_buf;
#endif
    PolicyK P = make_policy_k(p);
    RolloutK R = make_rollout_k(ro);
    HpK hp;
    if (int rc = make_hp(h, M, p.actions.num_groups, loss_out != nullptr, &hp)) return rc;

    const bool rows16 = rows16_eligible(P, ws.Mp, head_cols(p), p.num_layers, H,
                                        std::is_same<T, bf16>::value);
    ML_REQUIRE(h.step_kernel >= 0 && h.step_kernel <= 2, "ppo: step_kernel %d", h.step_kernel);
    ML_REQUIRE(h.step_kernel != 2 || (rows16 && !seq_weight), "%s",
               seq_weight
                   ? "ppo: step_kernel 2 (row-split) takes no per-sequence weights; the weighted "
                     "step runs the feature-split kernel (step_kernel 0 or 1)"
                   : "ppo: step_kernel 2 (row-split) needs bf16, hidden 256, 2 layers, a scalar critic, "
                     "head width 32, obs_dim 64, <= 7 action groups and (padded) rows of 32768 or a "
                     "multiple of 256 from 65536");
    if (seq_weight) {
        // the importance-weighted step: the feature split's weighted instantiation.
        // In the minibatch that records metrics (once per update) the unweighted
        // step runs first: its per-tile metric partials are the recorded 'Action
        // Obj' .. 'Entropy' (unweighted by definition, ppo.py:351-362, and so the
        // same bits as mlearn_ppo_minibatch_grad's); the weighted step then
        // overwrites the operands and adds the three weighted sums of 'Loss'.
        if (hp.metrics)
            if (int rc = launch_step<T, H>(P, R, mb_seq, mb, M, adv_st, hp, ws, s)) return rc;
        if (int rc = launch_step_weighted<T, H>(P, R, mb_seq, mb, M, adv_st, hp, ws, seq_weight, s))
            return rc;
    } else if (rows16 && h.step_kernel != 1) {
        ws.ncp = 2 * ws.ntiles;  // one column-partials row per 16-row tile
        if (rows16_cfg(ws.Mp).nt == 1) ws.nlp = 2 * ws.ntiles;  // one loss-partials row per wave
        launch_rows16(P, R, mb_seq, mb, M, adv_st, hp, ws, s);
    } else if (int rc = launch_step<T, H>(P, R, mb_seq, mb, M, adv_st, hp, ws, s)) {
        return rc;
    }
    if (step_only) return check_launch("ppo_minibatch_fwd_bwd");
    // weight gradients: the trunk layers, then the head
    const int L = p.num_layers;
    WgOperands tab[MLEARN_MAX_LAYERS + 1];
    for (int l = 0; l < L; ++l)
        tab[l] = WgOperands{l == 0 ? p.obs_dim : H, H, l == 0 ? ws.x0 : ws.a[l - 1], ws.dz[l]};
    tab[L] = WgOperands{H, head_cols(p), ws.a[L - 1], ws.dhead};
    if (int rc = launch_wgrad<T>(make_wg_jobs(tab, L + 1, ws, wg_groupable<T>(hp, L + 1)), ws, hp, M, p.actions.num_groups,
                                 loss_out, make_layout(p), grad, h.grad_sumsq_out, s))
        return rc;
    if (seq_weight && loss_out)  // 'Loss' from the weighted sums
        hipLaunchKernelGGL(weighted_loss_kernel, dim3(1), dim3(256), 0, s, ws, hp, M,
                           p.actions.num_groups, loss_out);
    return check_launch("ppo_minibatch_grad");
}

// ---------------------------------------------------------------------------
// Recurrent update: the LSTM scan over the minibatch's sequences
// (LSTM.sequence, rnn.py:81-111) and its reverse (BPTT), one launch per
// time step and direction (lstm_scan.h).  Rows f = t * mb + m.
// ---------------------------------------------------------------------------

template <typename T, int H>
static int launch_minibatch_lstm(const mlearn_mlp_policy& p, const mlearn_lstm& lstm,
                                 const mlearn_rollout_view& ro, const void* start_h,
                                 const void* start_c, const int32_t* mb_seq, int mb,
                                 const float* adv_st, const mlearn_ppo_hparams& h, float* grad,
                                 float* loss_out, void* wsp, hipStream_t s) {
    const int bptt = ro.bptt_len;
    const int64_t M = (int64_t)mb * bptt;
    WsK ws;
    LstmWsK lw;
    carve(p, M, (char*)wsp, &ws, &lstm, mb, &lw);
    PolicyK P = make_policy_k(p);
    LstmK RK = make_lstm_k(lstm);
    RolloutK R = make_rollout_k(ro);
    HpK hp;
    if (int rc = make_hp(h, M, p.actions.num_groups, loss_out != nullptr, &hp)) return rc;
    const int L = p.num_layers;
    RecK rec{lw.hout, lw.dhout, lw.dfeat, lstm.head_t_nat};
    // trunk forward over every row (the LSTM input F = A_{L-1})
    if (int rc = launch_step<T, H, kTrunkFwd>(P, R, mb_seq, mb, M, adv_st, hp, ws, s, rec)) return rc;
    const T* feat = (const T*)ws.a[L - 1];
    // forward scan: one launch per step over (mb / 32) x (H / 32) four-wave
    // workgroups (the input product F_t Wi inside each step)
    for (int t = 0; t < bptt; ++t)
        hipLaunchKernelGGL((lstm_fwd_step4_kernel<T, H>), dim3(mb / 32, H / 32), dim3(256), 0, s, RK,
                           R, mb_seq, mb, (const T*)start_h, (const T*)start_c, lw, t, feat);
    // heads + loss from the LSTM outputs
    if (int rc = launch_step<T, H, kHeads>(P, R, mb_seq, mb, M, adv_st, hp, ws, s, rec)) return rc;
    // reverse scan: dh_t and dF_{t+1} per step, then dF_0 from dG_0
    const int cp0 = L * 2 * H + head_cols(p);
    for (int t = bptt - 1; t >= -1; --t)
        hipLaunchKernelGGL((lstm_bwd_step4_kernel<T, H>), dim3(mb / 32, H / 32), dim3(256), 0, s,
                           RK, R, mb_seq, mb, lw, ws.colpart, ws.CP, cp0, t);
    // trunk backward from d features
    if (int rc = launch_step<T, H, kTrunkBwd>(P, R, mb_seq, mb, M, adv_st, hp, ws, s, rec)) return rc;
    // weight gradients: trunk, head (from the LSTM outputs), Wi, Wh
    WgOperands tab[MLEARN_MAX_LAYERS + 3];
    for (int l = 0; l < L; ++l)
        tab[l] = WgOperands{l == 0 ? p.obs_dim : H, H, l == 0 ? ws.x0 : ws.a[l - 1], ws.dz[l]};
    tab[L] = WgOperands{H, head_cols(p), lw.hout, ws.dhead};
    tab[L + 1] = WgOperands{H, 4 * H, feat, lw.dg};
    tab[L + 2] = WgOperands{H, 4 * H, lw.hin, lw.dg};
    if (int rc = launch_wgrad<T>(make_wg_jobs(tab, L + 3, ws, wg_groupable<T>(hp, L + 1)), ws, hp, M, p.actions.num_groups,
                                 loss_out, make_layout_lstm(p, lstm), grad, h.grad_sumsq_out, s))
        return rc;
    return check_launch("lstm_ppo_minibatch_grad");
}

}  // namespace ml

using namespace ml;

extern "C" {

#ifdef ML_STAMPS
// diagnostic builds only: phase timestamps of the fused minibatch kernel
void mlearn_debug_set_stamp_buffer(uint64_t* buf) { g_stamp_buf = buf; }
#endif

int64_t mlearn_grad_sumsq_parts(int64_t param_count) {
    return param_count < 1 ? -1 : (param_count + 63) / 64;
}

int64_t mlearn_param_count(const mlearn_mlp_policy* policy) {
    if (validate_policy(policy)) return -1;
    return make_layout(*policy).total;
}

int64_t mlearn_ppo_workspace_bytes(const mlearn_mlp_policy* policy, int64_t rows) {
    if (validate_policy(policy) || rows < 1) return -1;
    return (int64_t)carve(*policy, rows, nullptr, nullptr);
}

int32_t mlearn_ppo_step_kernel(const mlearn_mlp_policy* policy, int64_t rows, int32_t requested) {
    if (validate_policy(policy) || rows < 1 || requested < 0 || requested > 2) return -1;
    const int64_t Mp = (rows + kRowAlign - 1) / kRowAlign * kRowAlign;
    const PolicyK P = make_policy_k(*policy);
    const bool rows16 = rows16_eligible(P, Mp, head_cols(*policy), policy->num_layers,
                                        policy->hidden, policy->dtype == MLEARN_DTYPE_BF16);
    if (requested == 2 && !rows16) return -1;
    return rows16 && requested != 1 ? 2 : 1;
}

int32_t mlearn_ppo_wgrad_plan(const mlearn_mlp_policy* policy, int64_t rows, int32_t requested,
                              int32_t job, int32_t* splits, int64_t* rows_per_split,
                              int32_t* slabs) {
    if (validate_policy(policy) || rows < 1 || requested < 0 || requested == 3 || requested > 4 ||
        job < 0 ||
        job > policy->num_layers)
        return -1;
    WsK ws;
    carve(*policy, rows, nullptr, &ws);
    const bool bf = policy->dtype == MLEARN_DTYPE_BF16;
    const int form = bf ? (requested ? requested : ML_WG_FORM) : 1;
    const bool grouped = form == 4 && ws.splits[job] > kRgGroups;
    if (splits) *splits = ws.splits[job];
    if (rows_per_split) *rows_per_split = ws.rps[job];
    if (slabs) *slabs = grouped ? kRgGroups : ws.splits[job];
    return form == 4 && !grouped ? 2 : form;
}

// The argument checks the feed-forward and the recurrent update share; who
// ("ppo" / "lstm ppo") prefixes the message.
static int validate_minibatch(const char* who, const mlearn_mlp_policy* policy,
                              const mlearn_rollout_view* ro, const int32_t* mb_seq,
                              int32_t mb_size, const float* adv_stats,
                              const mlearn_ppo_hparams* hp, const void* workspace) {
    ML_REQUIRE(ro && mb_seq && adv_stats && hp && workspace, "%s: null pointer", who);
    ML_REQUIRE(ro->N >= 1 && ro->N < (1ll << 31) && (int64_t)mb_size * ro->bptt_len < (1ll << 31),
               "%s: N and rows per minibatch must be < 2^31", who);
    ML_REQUIRE(ro->bptt_len >= 1 && ro->T % ro->bptt_len == 0, "%s: bad bptt_len", who);
    ML_REQUIRE(ro->ld == 0 || ro->ld >= ro->N, "%s: ld %lld < N %lld", who, (long long)ro->ld,
               (long long)ro->N);
    ML_REQUIRE(ro->obs && ro->actions && ro->log_probs && ro->advantages &&
                   (ro->returns || ro->values),
               "%s: null rollout array", who);
    ML_REQUIRE(!hp->clip_value_loss || ro->values, "%s: clip_value_loss needs values", who);
    ML_REQUIRE(!hp->normalize_values || policy->critic_bins == 1,
               "%s: normalize_values needs the scalar critic (ppo.py:54-57)", who);
    return MLEARN_OK;
}

static int ppo_entry(const mlearn_mlp_policy* policy, const mlearn_rollout_view* ro,
                     const int32_t* mb_seq, int32_t mb_size, const float* adv_stats,
                     const mlearn_ppo_hparams* hp, float* grad, float* loss_out, void* workspace,
                     bool step_only, mlearn_stream_t stream, const float* seq_weight = nullptr) {
    int rc = validate_policy(policy);
    if (rc) return rc;
    rc = validate_minibatch("ppo", policy, ro, mb_seq, mb_size, adv_stats, hp, workspace);
    if (rc) return rc;
    ML_REQUIRE(step_only || grad, "ppo: null grad");
    ML_REQUIRE(mb_size >= 1, "ppo: mb_size must be >= 1");
    hipStream_t s = S(stream);
    return dispatch_th(policy->dtype, policy->hidden, [&](auto t, auto h) {
        return launch_minibatch<tag_t<decltype(t)>, h>(*policy, *ro, mb_seq, mb_size, adv_stats,
                                                       *hp, grad, loss_out, workspace, step_only, s,
                                                       seq_weight);
    });
}

int mlearn_ppo_minibatch_grad(const mlearn_mlp_policy* policy, const mlearn_rollout_view* ro,
                              const int32_t* mb_seq, int32_t mb_size, const float* adv_stats,
                              const mlearn_ppo_hparams* hp, float* grad, float* loss_out,
                              void* workspace, mlearn_stream_t stream) {
    return ppo_entry(policy, ro, mb_seq, mb_size, adv_stats, hp, grad, loss_out, workspace, false,
                     stream);
}

int mlearn_ppo_minibatch_grad_weighted(const mlearn_mlp_policy* policy,
                                       const mlearn_rollout_view* ro, const int32_t* mb_seq,
                                       int32_t mb_size, const float* adv_stats,
                                       const mlearn_ppo_hparams* hp, const float* seq_weight,
                                       float* grad, float* loss_out, void* workspace,
                                       mlearn_stream_t stream) {
    ML_REQUIRE(seq_weight, "ppo: null seq_weight");
    return ppo_entry(policy, ro, mb_seq, mb_size, adv_stats, hp, grad, loss_out, workspace, false,
                     stream, seq_weight);
}

int64_t mlearn_lstm_ppo_workspace_bytes(const mlearn_mlp_policy* policy, const mlearn_lstm* lstm,
                                        int64_t rows, int32_t mb_size) {
    if (validate_lstm(policy, lstm) || rows < 1 || mb_size < 1) return -1;
    return (int64_t)carve(*policy, rows, nullptr, nullptr, lstm, mb_size, nullptr);
}

int mlearn_lstm_ppo_minibatch_grad(const mlearn_mlp_policy* policy, const mlearn_lstm* lstm,
                                   const mlearn_rollout_view* ro, const void* start_h,
                                   const void* start_c, const int32_t* mb_seq, int32_t mb_size,
                                   const float* adv_stats, const mlearn_ppo_hparams* hp,
                                   float* grad, float* loss_out, void* workspace,
                                   mlearn_stream_t stream) {
    int rc = validate_lstm(policy, lstm);
    if (rc) return rc;
    rc = validate_minibatch("lstm ppo", policy, ro, mb_seq, mb_size, adv_stats, hp, workspace);
    if (rc) return rc;
    ML_REQUIRE(grad && start_h && start_c, "lstm ppo: null pointer");
    ML_REQUIRE(ro->dones, "lstm ppo: the rollout view needs dones (sequence breaks)");
    ML_REQUIRE(mb_size >= 32 && mb_size % 32 == 0, "lstm ppo: mb_size must be a multiple of 32");
    ML_REQUIRE(((int64_t)mb_size * ro->bptt_len) % 64 == 0,
               "lstm ppo: mb_size * bptt_len must be a multiple of 64");
    hipStream_t s = S(stream);
    return dispatch_th(policy->dtype, policy->hidden, [&](auto t, auto h) {
        return launch_minibatch_lstm<tag_t<decltype(t)>, h>(*policy, *lstm, *ro, start_h, start_c,
                                                            mb_seq, mb_size, adv_stats, *hp, grad,
                                                            loss_out, workspace, s);
    });
}

int mlearn_ppo_minibatch_fwd_bwd(const mlearn_mlp_policy* policy, const mlearn_rollout_view* ro,
                                 const int32_t* mb_seq, int32_t mb_size, const float* adv_stats,
                                 const mlearn_ppo_hparams* hp, void* workspace,
                                 mlearn_stream_t stream) {
    return ppo_entry(policy, ro, mb_seq, mb_size, adv_stats, hp, nullptr, nullptr, workspace, true,
                     stream);
}

}  // extern "C"
