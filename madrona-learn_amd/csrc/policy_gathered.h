// The gathered policy step: one rollout step with the policy chosen per env
// row (mlearn_policy_step_assigned, mlearn_policy_rollout_step_matched): the
// workspace, the bucket kernel that partitions the rows by policy, and the
// kernel that runs policy_step_body on the gathered tiles.  Part of
// policy.hip's translation unit.
#pragma once

#include "policy_step.h"

namespace ml {

// One rollout step with the policy chosen per env row
// (mlearn_policy_step_assigned).  Workspace: the PolicyK table (written once
// by mlearn_policy_assigned_prepare), then per step the tile table
// {policy, live rows} and the row map [tiles][32] of env indices, both
// rebuilt from `assignments` by assign_bucket_kernel.  Policy p's rows take
// ceil(count_p / 32) consecutive tiles, in ascending env order; the tiles of
// all policies are at most ceil(N / 32) + P, the step's grid; the bucket
// kernel's is ceil(N / 4096).  Both are functions of N and P alone and
// nothing on the host reads device data, so a captured step replays after
// `assignments` changed in place.
constexpr int kAssignMaxPolicies = 64;  // one lane per policy in the bucket kernel
constexpr int kBktWaves = 16, kBktThreads = 64 * kBktWaves;
constexpr int kBktSweep = 4 * kBktThreads;  // rows per sweep: one int4 per lane of a workgroup

struct AssignWs {
    PolicyK* tab;    // [P]
    int2* tiles;     // [ntiles] {policy, live rows (0: no tile)}
    int32_t* map;    // [ntiles][32] env index of tile lane r < live rows
    int64_t ntiles;  // ceil(N / 32) + P
    int64_t bytes;
};

static AssignWs assign_ws(void* ws, int64_t N, int P) {
    auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
    AssignWs a;
    a.ntiles = (N + 31) / 32 + P;
    const int64_t o_tiles = up((int64_t)P * (int64_t)sizeof(PolicyK));
    const int64_t o_map = o_tiles + up(a.ntiles * (int64_t)sizeof(int2));
    a.bytes = o_map + up(a.ntiles * 32 * (int64_t)sizeof(int32_t));
    a.tab = (PolicyK*)ws;
    a.tiles = (int2*)((char*)ws + o_tiles);
    a.map = (int32_t*)((char*)ws + o_map);
    return a;
}

// The 4 assignments of rows i .. i + 3 (-1 past N: matches no policy).
__device__ inline int4 load_assign4(const int32_t* __restrict__ asg, int64_t N, int64_t i) {
    if (i + 3 < N) return *(const int4*)(asg + i);
    return make_int4(i < N ? asg[i] : -1, i + 1 < N ? asg[i + 1] : -1, i + 2 < N ? asg[i + 2] : -1,
                     -1);
}

// Lane p's count of policy p among the wave's 256 assignments v (0 for lanes >= P).
__device__ inline int count_lane_policy(int4 v, int P, int lane) {
    int c = 0;
    for (int p = 0; p < P; ++p) {
        const int n = __popcll(__ballot(v.x == p)) + __popcll(__ballot(v.y == p)) +
                      __popcll(__ballot(v.z == p)) + __popcll(__ballot(v.w == p));
        if (lane == p) c = n;
    }
    return c;
}

// Lanes below this one set in m.
__device__ inline int lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// Stable partition of the env rows by assignment, integer work only.
// Workgroup b owns the rows of sweep b, [b * 4096, (b + 1) * 4096): wave w the
// 256 rows from w * 256 of it, lane l four consecutive ones.  Every workgroup
// counts each policy's rows in the sweeps ahead of its own and over all N
// (wave ballots, lane p = policy p), so it needs no other workgroup's result
// -- ceil(N / 4096) workgroups that each read all N assignments: 16 x 256 KiB
// at N = 65 536 -- and then ranks its own rows behind them.  Rows assigned
// outside [0, P) match no policy: never counted, never written.  Workgroup 0
// writes the tile table.
__global__ __launch_bounds__(kBktThreads) void assign_bucket_kernel(
    const int32_t* __restrict__ asg, int64_t N, int P, int2* __restrict__ tiles,
    int32_t* __restrict__ map, int64_t ntiles) {
    __shared__ int s_cnt[3][kBktWaves][kAssignMaxPolicies];  // sweeps ahead / own sweep / behind, per wave
    __shared__ int s_ahead[kAssignMaxPolicies], s_total[kAssignMaxPolicies];
    __shared__ int s_base[kAssignMaxPolicies + 1];  // first tile of policy p
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t nsweep = (N + kBktSweep - 1) / kBktSweep;
    const int64_t own = blockIdx.x;
    const int64_t col = (int64_t)w * 256 + lane * 4;  // this lane's rows inside a sweep
    int n_ahead = 0, n_own = 0, n_behind = 0;
    int4 mine = make_int4(-1, -1, -1, -1);
    constexpr int U = 8;  // loads in flight
    for (int64_t k0 = 0; k0 < nsweep; k0 += U) {
        int4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            v[u] = load_assign4(asg, N, k0 + u < nsweep ? (k0 + u) * kBktSweep + col : N);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t k = k0 + u;
            if (k >= nsweep) break;
            const int c = count_lane_policy(v[u], P, lane);
            if (k < own) {
                n_ahead += c;
            } else if (k > own) {
                n_behind += c;
            } else {
                n_own = c;
                mine = v[u];
            }
        }
    }
    s_cnt[0][w][lane] = n_ahead;
    s_cnt[1][w][lane] = n_own;
    s_cnt[2][w][lane] = n_behind;
    __syncthreads();
    if (w == 0) {
        int ahead = 0, total = 0;
        for (int v = 0; v < kBktWaves; ++v) {
            ahead += s_cnt[0][v][lane];
            total += s_cnt[1][v][lane] + s_cnt[2][v][lane];
        }
        total += ahead;
        // first tile of every policy: inclusive scan of ceil(total / 32) over the lanes
        int incl = (total + 31) >> 5;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        s_ahead[lane] = ahead;
        s_total[lane] = total;
        s_base[lane + 1] = incl;
        if (lane == 0) s_base[0] = 0;
    }
    __syncthreads();
    // rank of policy p's first row of this wave among all of p's rows (lane p):
    // the sweeps ahead, then the waves ahead in the own sweep
    int off = s_ahead[lane];
    for (int v = 0; v < w; ++v) off += s_cnt[1][v][lane];
    const int64_t row = own * kBktSweep + col;
    for (int p = 0; p < P; ++p) {
        const unsigned long long m0 = __ballot(mine.x == p), m1 = __ballot(mine.y == p);
        const unsigned long long m2 = __ballot(mine.z == p), m3 = __ballot(mine.w == p);
        if ((m0 | m1 | m2 | m3) == 0) continue;
        // ascending env index: the lanes below (all four rows each), then this lane's rows
        int64_t slot = (int64_t)s_base[p] * 32 + __builtin_amdgcn_readlane(off, p) +
                       lanes_below(m0) + lanes_below(m1) + lanes_below(m2) + lanes_below(m3);
        if (mine.x == p) map[slot++] = (int32_t)row;
        if (mine.y == p) map[slot++] = (int32_t)(row + 1);
        if (mine.z == p) map[slot++] = (int32_t)(row + 2);
        if (mine.w == p) map[slot] = (int32_t)(row + 3);
    }
    if (blockIdx.x == 0) {
        for (int64_t g = tid; g < ntiles; g += kBktThreads) {
            int2 t = make_int2(0, 0);
            for (int p = 0; p < P; ++p)
                if (g >= s_base[p] && g < s_base[p + 1]) {
                    const int left = s_total[p] - (int)(g - s_base[p]) * 32;
                    t = make_int2(p, left < 32 ? left : 32);
                }
            tiles[g] = t;
        }
    }
}

// The gathered step: tile g runs policy tiles[g].x on the env rows
// map[g * 32 + r], r < tiles[g].y, with the body and the counters of that
// policy's own policy_step_kernel launch (the same bits per env row).
// MATCHED = false (mlearn_policy_step_assigned): inference only, obs_store,
// post and mk are not read.  MATCHED (mlearn_policy_rollout_step_matched): a
// full rollout step; the store rows go through mk.tcol into the train store,
// the sim-order actions are written for every row of a table policy.  The
// post-step of the previous env step runs over the sim rows in launch order
// (workgroup b: rows [32 b, 32 b + 32); the grid has at least ceil(N / 32)
// workgroups), ahead of the tile's own early exit: the body reads nothing
// the post-step writes.
template <typename T, int H, int HC, bool MATCHED>
__global__ __launch_bounds__((pol_threads<H, false>())) __attribute__((amdgpu_waves_per_eu(ML_POL_MLP_WAVES, 8))) void policy_step_gathered_kernel(
    const PolicyK* __restrict__ tab, int npol, const int2* __restrict__ tiles,
    const int32_t* __restrict__ map, const float* __restrict__ obs, int64_t N, T* obs_store,
    int32_t* actions, float* logp, float* values, uint32_t k0, uint32_t k1,
    const uint64_t* step_ctr, uint64_t step_add, uint32_t eoff, int sample, PostK post, MatchK mk) {
    if constexpr (MATCHED) {
        if (post.rew && threadIdx.x < 32) {
            const int64_t n = (int64_t)blockIdx.x * 32 + threadIdx.x;
            if (n < N) post_step_row<true>(post, &mk, n);
        }
    }
    const int2 t = tiles[blockIdx.x];
    const int p = __builtin_amdgcn_readfirstlane(t.x);
    const int nlive = __builtin_amdgcn_readfirstlane(t.y);
    // no rows (workgroup-uniform, ahead of every barrier); the table is never
    // indexed outside [0, npol)
    if (nlive <= 0 || nlive > 32 || (unsigned)p >= (unsigned)npol) return;
    policy_step_body<T, H, false, HC, pol_maxw<false>(), false, true, MATCHED>(
        tab[p], obs, N, MATCHED ? obs_store : nullptr, actions, logp, values, k0, k1, step_ctr,
        step_add, eoff, sample, PostK{}, LstmK{}, CarryK{}, EvalK{}, EnvK{}, blockIdx.x,
        GatherK{map, nlive, MATCHED ? &mk : nullptr});
}

}  // namespace ml
