// Discrete PPO actor objective on the torch path (include/mlearn.h "Discrete
// PPO actor objective"): log-probs, entropies, the clipped surrogate and the
// two scalar terms of the loss in one launch (+ a one-workgroup finish), the
// gradient of those terms w.r.t. the logits in another.
//
//   One row per aligned group of 16 lanes of a 256-thread workgroup (16 rows
//   per pass, 4 rows per wave).  The group loads its row's A <= 95 logits
//   coalesced into one LDS row as f32 (f32 or bf16 in memory, any row stride
//   and base alignment: 16-byte chunks where base and stride allow, element by
//   element elsewhere and for a ragged last chunk, the same bits either way);
//   lane k < K then runs sub-action k on its group's logits from LDS
//   (eval_group of dists.h, the fused step's statement of the softmax
//   statistics).  The backward's lane k overwrites its group's logits in LDS
//   with their gradient and the 16 lanes store the row back coalesced, each
//   element rounded once.  LDS rows are 97 floats apart (the 4 rows of a wave
//   start in different banks); 6.2 KB per workgroup.
//
//   Every workgroup takes a fixed contiguous share of the rows (a function of
//   `rows` alone), every lane runs every pass (rows past the end recompute row
//   rows - 1 and store nothing), so the barriers are unconditional.  A lane
//   sums oc_k w_r obj and ec_k w_r H of its passes, the workgroup adds its
//   lanes in a fixed order (butterfly per wave, then the 4 waves) into one
//   [2] row of the workspace and the finish launch adds those rows in a fixed
//   order in f64: no atomics, the same bits on every call and graph replay.
#pragma clang fp contract(off)
#include "continuous.h"  // cont_load
#include "dists.h"

namespace ml {
namespace {

constexpr int kThreads = 256;
constexpr int kG = 16;                 // lanes per row
constexpr int kRows = kThreads / kG;   // rows per pass of a workgroup
constexpr int kMaxA = MLEARN_HEAD_COLS_MAX - 1;  // 95 logits
constexpr int kLd = 97;                // LDS row stride (floats)
constexpr int kMaxParts = 1024;        // workgroups (workspace rows) at most

struct Share {
    int parts;        // workgroups
    int64_t passes;   // passes of kRows rows per workgroup
};

Share share_of(int64_t rows) {
    const int64_t tiles = (rows + kRows - 1) / kRows;
    Share s;
    s.passes = (tiles + kMaxParts - 1) / kMaxParts;
    s.parts = (int)((tiles + s.passes - 1) / s.passes);
    return s;
}

struct ObjArgs {
    const void* logits;
    int64_t ld;
    int32_t dtype;
    int64_t rows, M, passes;
    const int32_t* actions;
    const float* old_logp;
    const float* adv;
    const float* adv_stats;
    const float* seq_weights;
    // forward
    float *logp, *ent, *obj, *ws;
    // backward
    const float* G;
    void* d;
    int64_t ldd;
};

// The row's A logits -> lg[0..A) (f32).  VEC: p + row ld is 16-byte aligned for
// every row; whole 16-byte chunks move as one access.
template <bool VEC>
__device__ inline void load_row(const void* p, int32_t dtype, int64_t base, int A, int sub,
                                float* lg) {
    if (VEC) {
        const int V = dtype == MLEARN_DTYPE_F32 ? 4 : 8;
        for (int c = sub * V; c < A; c += kG * V) {
            if (c + V <= A) {
                if (dtype == MLEARN_DTYPE_F32) {
                    const float4 v = *(const float4*)((const float*)p + base + c);
                    lg[c] = v.x, lg[c + 1] = v.y, lg[c + 2] = v.z, lg[c + 3] = v.w;
                } else {
                    const uint4 v = *(const uint4*)((const uint16_t*)p + base + c);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        lg[c + 2 * i] = __builtin_bit_cast(float, w[i] << 16);
                        lg[c + 2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
                    }
                }
            } else {
                for (int j = c; j < A; ++j) lg[j] = cont_load(p, dtype, base + j);
            }
        }
    } else {
        for (int j = sub; j < A; j += kG) lg[j] = cont_load(p, dtype, base + j);
    }
}

__device__ inline uint32_t bf16_bits(float v) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (bf16)v);
}

template <bool VEC>
__device__ inline void store_row(void* p, int32_t dtype, int64_t base, int A, int sub,
                                 const float* lg) {
    if (VEC) {
        const int V = dtype == MLEARN_DTYPE_F32 ? 4 : 8;
        for (int c = sub * V; c < A; c += kG * V) {
            if (c + V <= A) {
                if (dtype == MLEARN_DTYPE_F32) {
                    *(float4*)((float*)p + base + c) =
                        make_float4(lg[c], lg[c + 1], lg[c + 2], lg[c + 3]);
                } else {
                    uint4 v;
                    v.x = bf16_bits(lg[c]) | (bf16_bits(lg[c + 1]) << 16);
                    v.y = bf16_bits(lg[c + 2]) | (bf16_bits(lg[c + 3]) << 16);
                    v.z = bf16_bits(lg[c + 4]) | (bf16_bits(lg[c + 5]) << 16);
                    v.w = bf16_bits(lg[c + 6]) | (bf16_bits(lg[c + 7]) << 16);
                    *(uint4*)((uint16_t*)p + base + c) = v;
                }
            } else {
                for (int j = c; j < A; ++j) {
                    if (dtype == MLEARN_DTYPE_F32) ((float*)p)[base + j] = lg[j];
                    else ((uint16_t*)p)[base + j] = (uint16_t)bf16_bits(lg[j]);
                }
            }
        }
    } else {
        for (int j = sub; j < A; j += kG) {
            if (dtype == MLEARN_DTYPE_F32) ((float*)p)[base + j] = lg[j];
            else ((uint16_t*)p)[base + j] = (uint16_t)bf16_bits(lg[j]);
        }
    }
}

// The layout and the coefficients into LDS with constant indices into the
// kernel arguments (an index by lane would copy the structs to scratch).
__device__ inline void stage_tables(const mlearn_action_layout& lay,
                                    const mlearn_actor_obj_coefs& cf, int tid, int* s_off,
                                    float* s_oc, float* s_ec) {
#pragma unroll
    for (int i = 0; i <= MLEARN_MAX_GROUPS; ++i)
        if (tid == i) s_off[i] = lay.offsets[i];
#pragma unroll
    for (int i = 0; i < MLEARN_MAX_GROUPS; ++i)
        if (tid == 32 + i) s_oc[i] = cf.obj_coef[i], s_ec[i] = cf.ent_coef[i];
}

// The surrogate of one (row, sub-action): A-hat rho and A-hat clip(rho).
struct Surr {
    float ah, rho, s1, s2;
};
__device__ inline Surr surrogate(float logp, float old_logp, float adv, const float* adv_stats,
                                 float lo, float hi) {
    Surr s;
    s.ah = adv_stats ? (adv - adv_stats[0]) * adv_stats[1] : adv;
    s.rho = expf(logp - old_logp);
    s.s1 = s.ah * s.rho;
    s.s2 = s.ah * fminf(fmaxf(s.rho, lo), hi);
    return s;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void actor_obj_fwd_kernel(mlearn_action_layout lay,
                                                                 mlearn_actor_obj_coefs cf,
                                                                 ObjArgs a) {
    __shared__ float s_lg[kRows][kLd];
    __shared__ int s_off[MLEARN_MAX_GROUPS + 1];
    __shared__ float s_oc[MLEARN_MAX_GROUPS], s_ec[MLEARN_MAX_GROUPS];
    __shared__ float s_red[kThreads / kWave][2];
    const int tid = threadIdx.x, g = tid / kG, sub = tid % kG;
    const int K = lay.num_groups, A = lay.num_logits;
    stage_tables(lay, cf, tid, s_off, s_oc, s_ec);
    float acc_o = 0.f, acc_e = 0.f;
    const int64_t row0 = (int64_t)blockIdx.x * a.passes * kRows + g;
    for (int64_t ps = 0; ps < a.passes; ++ps) {
        const int64_t row = row0 + ps * kRows;
        const bool valid = row < a.rows;
        const int64_t rr = valid ? row : a.rows - 1;
        __syncthreads();  // the tables (first pass); the previous pass' reads of the row
        load_row<VEC>(a.logits, a.dtype, rr * a.ld, A, sub, s_lg[g]);
        __syncthreads();
        if (sub < K) {
            const int o = s_off[sub], nb = s_off[sub + 1] - o;
            const int64_t i = rr * K + sub;
            float lp, en;
            eval_group(s_lg[g] + o, nb, a.actions[i], &lp, &en);
            const Surr s = surrogate(lp, a.old_logp[i], a.adv[rr], a.adv_stats, cf.clip_lo,
                                     cf.clip_hi);
            const float ob = fminf(s.s1, s.s2);
            if (valid) {
                a.logp[i] = lp;
                a.ent[i] = en;
                a.obj[i] = ob;
                const float w = a.seq_weights ? a.seq_weights[row % a.M] : 1.0f;
                acc_o += s_oc[sub] * (w * ob);
                acc_e += s_ec[sub] * (w * en);
            }
        }
    }
    acc_o = wave_sum64(acc_o);
    acc_e = wave_sum64(acc_e);
    if (tid % kWave == 0) s_red[tid / kWave][0] = acc_o, s_red[tid / kWave][1] = acc_e;
    __syncthreads();
    if (tid < 2) {
        float v = s_red[0][tid];
        for (int w = 1; w < kThreads / kWave; ++w) v += s_red[w][tid];
        a.ws[2 * blockIdx.x + tid] = v;
    }
}

// terms[i] = (sum over the workgroups' partial sums, fixed order, f64) / rows
__global__ __launch_bounds__(kThreads) void actor_obj_finish_kernel(const float* ws, int parts,
                                                                    int64_t rows, float* terms) {
    __shared__ double s_red[kThreads / kWave][2];
    const int tid = threadIdx.x;
    double v[2] = {0.0, 0.0};
    for (int p = tid; p < parts; p += kThreads) v[0] += ws[2 * p], v[1] += ws[2 * p + 1];
    for (int i = 0; i < 2; ++i) {
        v[i] = wave_sum64d(v[i]);
        if (tid % kWave == 0) s_red[tid / kWave][i] = v[i];
    }
    __syncthreads();
    if (tid < 2) {
        double t = s_red[0][tid];
        for (int w = 1; w < kThreads / kWave; ++w) t += s_red[w][tid];
        terms[tid] = (float)(t / (double)rows);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void actor_obj_bwd_kernel(mlearn_action_layout lay,
                                                                 mlearn_actor_obj_coefs cf,
                                                                 ObjArgs a) {
    __shared__ float s_lg[kRows][kLd];
    __shared__ int s_off[MLEARN_MAX_GROUPS + 1];
    __shared__ float s_oc[MLEARN_MAX_GROUPS], s_ec[MLEARN_MAX_GROUPS];
    const int tid = threadIdx.x, g = tid / kG, sub = tid % kG;
    const int K = lay.num_groups, A = lay.num_logits;
    stage_tables(lay, cf, tid, s_off, s_oc, s_ec);
    const float g0 = a.G[0], g1 = a.G[1], nrows = (float)a.rows;
    const int64_t row0 = (int64_t)blockIdx.x * a.passes * kRows + g;
    for (int64_t ps = 0; ps < a.passes; ++ps) {
        const int64_t row = row0 + ps * kRows;
        const bool valid = row < a.rows;
        const int64_t rr = valid ? row : a.rows - 1;
        __syncthreads();  // the tables (first pass); the previous pass' store of the row
        load_row<VEC>(a.logits, a.dtype, rr * a.ld, A, sub, s_lg[g]);
        __syncthreads();
        if (sub < K) {
            const int o = s_off[sub], nb = s_off[sub + 1] - o;
            const int64_t i = rr * K + sub;
            float* lg = s_lg[g] + o;
            int act = a.actions[i];
            act = act < 0 ? 0 : (act >= nb ? nb - 1 : act);
            float lp, en;
            eval_group(lg, nb, act, &lp, &en);  // the forward's bits: the same rho
            const Surr s = surrogate(lp, a.old_logp[i], a.adv[rr], a.adv_stats, cf.clip_lo,
                                     cf.clip_hi);
            // minimum / maximum split their gradient evenly at a tie
            const float m = s.s1 < s.s2 ? 1.f : (s.s1 == s.s2 ? 0.5f : 0.f);
            const float dc = (s.rho > cf.clip_lo && s.rho < cf.clip_hi) ? 1.f
                             : ((s.rho == cf.clip_lo || s.rho == cf.clip_hi) ? 0.5f : 0.f);
            const float dobj = s.s1 * (m + (1.f - m) * dc);
            const float w = a.seq_weights ? a.seq_weights[rr % a.M] : 1.0f;
            const float wr = w / nrows;
            const float ca = (g0 * s_oc[sub]) * wr * dobj, cb = (g1 * s_ec[sub]) * wr;
            // eval_group's max, sum and log-sum-exp again (the same loops)
            float mx = lg[0];
            for (int j = 1; j < nb; ++j) mx = fmaxf(mx, lg[j]);
            float se = 0.f;
            for (int j = 0; j < nb; ++j) se += __expf(lg[j] - mx);
            const float lse = mx + __logf(se), inv = 1.0f / se;
            for (int j = 0; j < nb; ++j) {
                const float l = lg[j], p = __expf(l - mx) * inv;
                lg[j] = ca * ((j == act ? 1.f : 0.f) - p) - cb * (p * ((l - lse) + en));
            }
        }
        __syncthreads();
        if (valid) store_row<VEC>(a.d, a.dtype, row * a.ldd, A, sub, s_lg[g]);
    }
}

// ---------------------------------------------------------------------------
// argument checks (before any pointer is followed or the device is touched)
// ---------------------------------------------------------------------------
int check_args(const char* what, const void* logits, int64_t ld, int32_t dtype,
               const mlearn_action_layout& lay, int64_t rows, int64_t M, const int32_t* actions,
               const float* old_logp, const float* adv, const float* seq_weights,
               const mlearn_actor_obj_coefs* cf) {
    ML_REQUIRE(lay.num_groups >= 1 && lay.num_groups <= MLEARN_MAX_GROUPS,
               "%s: %d action groups outside 1..%d", what, lay.num_groups, MLEARN_MAX_GROUPS);
    ML_REQUIRE(lay.num_logits >= 1 && lay.num_logits <= kMaxA, "%s: %d logits outside 1..%d",
               what, lay.num_logits, kMaxA);
    ML_REQUIRE(lay.offsets[0] == 0 && lay.offsets[lay.num_groups] == lay.num_logits,
               "%s: the layout's offsets do not span its %d logits", what, lay.num_logits);
    for (int k = 0; k < lay.num_groups; ++k)
        ML_REQUIRE(lay.offsets[k + 1] > lay.offsets[k], "%s: action group %d is empty", what, k);
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(rows >= 1, "%s: rows = %lld (at least 1)", what, (long long)rows);
    ML_REQUIRE(ld >= lay.num_logits, "%s: ld_logits = %lld below the %d logits", what,
               (long long)ld, lay.num_logits);
    ML_REQUIRE(logits && actions && old_logp && adv && cf,
               "%s: null pointer (logits, actions, old_logp, adv or coefs)", what);
    ML_REQUIRE(!seq_weights || M >= 1, "%s: seq_weights with M = %lld (at least 1)", what,
               (long long)M);
    ML_REQUIRE(cf->clip_lo <= cf->clip_hi && cf->clip_lo > -INFINITY && cf->clip_hi < INFINITY,
               "%s: clip range [%g, %g] is not a finite interval", what, (double)cf->clip_lo,
               (double)cf->clip_hi);
    return MLEARN_OK;
}

bool aligned16(const void* p, int64_t ld, int32_t dtype) {
    const int64_t es = dtype == MLEARN_DTYPE_F32 ? 4 : 2;
    return (uintptr_t)p % 16 == 0 && (ld * es) % 16 == 0;
}

}  // namespace
}  // namespace ml

extern "C" {

int64_t mlearn_actor_obj_workspace_bytes(int64_t rows) {
    if (rows < 1) return -1;
    return (int64_t)ml::share_of(rows).parts * 2 * (int64_t)sizeof(float);
}

int mlearn_actor_obj_fwd(const void* logits, int64_t ld, int32_t dtype, mlearn_action_layout layout,
                         int64_t rows, int64_t M, const int32_t* actions, const float* old_logp,
                         const float* adv, const float* adv_stats, const float* seq_weights,
                         const mlearn_actor_obj_coefs* coefs, float* logp, float* ent, float* obj,
                         float* terms, void* workspace, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("actor_obj_fwd", logits, ld, dtype, layout, rows, M, actions, old_logp,
                            adv, seq_weights, coefs))
        return rc;
    ML_REQUIRE(logp && ent && obj && terms && workspace,
               "actor_obj_fwd: null pointer (logp, ent, obj, terms or workspace)");
    const Share sh = share_of(rows);
    ObjArgs a = {};
    a.logits = logits, a.ld = ld, a.dtype = dtype, a.rows = rows, a.M = M, a.passes = sh.passes;
    a.actions = actions, a.old_logp = old_logp, a.adv = adv, a.adv_stats = adv_stats;
    a.seq_weights = seq_weights;
    a.logp = logp, a.ent = ent, a.obj = obj, a.ws = (float*)workspace;
    (void)hipGetLastError();
    if (aligned16(logits, ld, dtype))
        hipLaunchKernelGGL(actor_obj_fwd_kernel<true>, dim3(sh.parts), dim3(kThreads), 0, S(stream),
                           layout, *coefs, a);
    else
        hipLaunchKernelGGL(actor_obj_fwd_kernel<false>, dim3(sh.parts), dim3(kThreads), 0,
                           S(stream), layout, *coefs, a);
    if (int rc = check_launch("actor_obj_fwd")) return rc;
    hipLaunchKernelGGL(actor_obj_finish_kernel, dim3(1), dim3(kThreads), 0, S(stream),
                       (const float*)workspace, sh.parts, rows, terms);
    return check_launch("actor_obj_fwd (finish)");
}

int mlearn_actor_obj_bwd(const void* logits, int64_t ld, int32_t dtype, mlearn_action_layout layout,
                         int64_t rows, int64_t M, const int32_t* actions, const float* old_logp,
                         const float* adv, const float* adv_stats, const float* seq_weights,
                         const mlearn_actor_obj_coefs* coefs, const float* g_terms, void* d_logits,
                         int64_t ld_d, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("actor_obj_bwd", logits, ld, dtype, layout, rows, M, actions, old_logp,
                            adv, seq_weights, coefs))
        return rc;
    ML_REQUIRE(g_terms && d_logits, "actor_obj_bwd: null pointer (g_terms or d_logits)");
    ML_REQUIRE(ld_d >= layout.num_logits, "actor_obj_bwd: ld_d_logits = %lld below the %d logits",
               (long long)ld_d, layout.num_logits);
    const Share sh = share_of(rows);
    ObjArgs a = {};
    a.logits = logits, a.ld = ld, a.dtype = dtype, a.rows = rows, a.M = M, a.passes = sh.passes;
    a.actions = actions, a.old_logp = old_logp, a.adv = adv, a.adv_stats = adv_stats;
    a.seq_weights = seq_weights;
    a.G = g_terms, a.d = d_logits, a.ldd = ld_d;
    (void)hipGetLastError();
    if (aligned16(logits, ld, dtype) && aligned16(d_logits, ld_d, dtype))
        hipLaunchKernelGGL(actor_obj_bwd_kernel<true>, dim3(sh.parts), dim3(kThreads), 0, S(stream),
                           layout, *coefs, a);
    else
        hipLaunchKernelGGL(actor_obj_bwd_kernel<false>, dim3(sh.parts), dim3(kThreads), 0,
                           S(stream), layout, *coefs, a);
    return check_launch("actor_obj_bwd");
}

}  // extern "C"
