// Importance-sampled trajectory minibatches (ppo.py:407-435): the draw of S of
// the n = C * B sequences without replacement from softmax(score) and the
// per-sequence loss weights, all on the device (no host read: the update's
// HIP graphs capture it).
//
//   keys     score_s = mean_t |adv| + mean_t |value - return|, key_s = score_s
//            + Gumbel noise (Gumbel top-k = jax.random.choice(replace=False,
//            p=softmax(score))); per-block (max, sum exp) partials of the
//            scores' log-sum-exp;
//   select   ascending ids of the k largest keys: an MSB-first radix select
//            on the order-preserving u32 image of the key, 8 bits per pass
//            (per-block LDS histograms written out as rows, a one-workgroup
//            scan that picks the bucket), then a counted compaction with a
//            prefix over blocks.  Ties at the threshold go to the lower id.
//            Ten launches, no host read-back, no allocation; integer LDS
//            atomics only (sums of integers: no arrival-order dependence);
//   weights  w_s = (1 / n) / softmax(score)_s = exp(lse - score_s) / n.

#include <math.h>

#include "common.h"

namespace ml {

constexpr uint32_t kImpKey0 = 0x494D5053u, kImpKey1 = 0x54524A53u;  // "IMPS", "TRJS"
constexpr int kImpBlock = 256;

// ---------------------------------------------------------------------------
// Scores, keys and the log-sum-exp partials.  One thread per sequence s =
// c * B + b; the threads of a wave read consecutive env columns of each store
// row (GAE's access pattern).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kImpBlock) void importance_keys_kernel(
    mlearn_rollout_view ro, uint32_t k0, uint32_t k1, const uint64_t* __restrict__ epoch_ctr,
    int n, float* __restrict__ scores, float* __restrict__ keys, double* __restrict__ lse_part) {
#pragma clang fp contract(off)
    __shared__ float shm[kImpBlock / 64];
    __shared__ double shs[kImpBlock / 64];
    const int s = (int)blockIdx.x * kImpBlock + (int)threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool live = s < n;
    float score = -INFINITY;
    if (live) {
        const int64_t c = s / ro.N, b = s - c * ro.N;
        const int bptt = ro.bptt_len;
        const float* adv = ro.advantages + (c * bptt) * ro.ld + b;
        const float* val = ro.values + (c * bptt) * ro.ld + b;
        const float* ret = ro.returns ? ro.returns + (c * bptt) * ro.ld + b : nullptr;
        float a = 0.f, v = 0.f;
        for (int t = 0; t < bptt; ++t) {
            const int64_t o = (int64_t)t * ro.ld;
            const float ad = adv[o], vl = val[o];
            const float rt = ret ? ret[o] : ad + vl;  // ret_at (ppo_defs.h)
            a = a + fabsf(ad);
            v = v + fabsf(vl - rt);
        }
        score = a / (float)bptt + v / (float)bptt;
        const uint64_t epoch = epoch_ctr ? *epoch_ctr : 0ull;
        scores[s] = score;
        keys[s] = score + det_gumbel(sample_uniform(k0 ^ kImpKey0, k1 ^ kImpKey1, (uint32_t)s,
                                                    epoch, 0));
    }
    // block maximum, then the block's sum of exp(score - max) in double
    float mx = score;
    for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) shm[w] = mx;
    __syncthreads();
    mx = shm[0];
    for (int i = 1; i < kImpBlock / 64; ++i) mx = fmaxf(mx, shm[i]);
    double e = live ? exp((double)score - (double)mx) : 0.0;
    e = wave_sum64d(e);
    if (lane == 0) shs[w] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = shs[0];
        for (int i = 1; i < kImpBlock / 64; ++i) t += shs[i];
        lse_part[2 * (int64_t)blockIdx.x] = (double)mx;
        lse_part[2 * (int64_t)blockIdx.x + 1] = t;
    }
}

// Every block folds the partials into the same log-sum-exp (same order, same
// bits), then its 256 sequences take w_s = exp(lse - score_s) / n.
__global__ __launch_bounds__(kImpBlock) void importance_weights_kernel(
    const float* __restrict__ scores, const double* __restrict__ lse_part, int n, int nparts,
    float* __restrict__ weights) {
    __shared__ double shm[kImpBlock / 64];
    __shared__ double shs[kImpBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double mx = -INFINITY;
    for (int i = threadIdx.x; i < nparts; i += kImpBlock) mx = fmax(mx, lse_part[2 * (int64_t)i]);
    for (int o = 1; o < 64; o <<= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane == 0) shm[w] = mx;
    __syncthreads();
    mx = shm[0];
    for (int i = 1; i < kImpBlock / 64; ++i) mx = fmax(mx, shm[i]);
    double sum = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kImpBlock)
        sum += lse_part[2 * (int64_t)i + 1] * exp(lse_part[2 * (int64_t)i] - mx);
    sum = wave_sum64d(sum);
    if (lane == 0) shs[w] = sum;
    __syncthreads();
    sum = shs[0];
    for (int i = 1; i < kImpBlock / 64; ++i) sum += shs[i];
    const double lse = mx + log(sum);
    const int s = (int)blockIdx.x * kImpBlock + (int)threadIdx.x;
    if (s < n) weights[s] = (float)(exp(lse - (double)scores[s]) / (double)n);
}

// ---------------------------------------------------------------------------
// Radix select of the k largest f32 keys.
// ---------------------------------------------------------------------------
constexpr int kSelMaxBlocks = 256;  // blocks of the histogram / count / write launches
constexpr int kSelMinChunk = 2048;  // ids per block at least (a multiple of 256)

// Block b owns ids [b * chunk, min(n, (b + 1) * chunk)).
struct SelPlan {
    int nb, chunk;
};
static SelPlan sel_plan(int64_t n) {
    int64_t nb = (n + kSelMinChunk - 1) / kSelMinChunk;
    if (nb > kSelMaxBlocks) nb = kSelMaxBlocks;
    if (nb < 1) nb = 1;
    int64_t chunk = (n + nb - 1) / nb;
    chunk = (chunk + 255) / 256 * 256;
    nb = (n + chunk - 1) / chunk;
    return SelPlan{(int)nb, (int)chunk};
}

// Workspace: state {prefix, k left, -, -} (256 B), hist [nb][256] u32, counts
// [nb][2] u32.
struct SelWs {
    uint32_t* state;
    uint32_t* hist;
    uint32_t* cnt;
};
static size_t sel_carve(const SelPlan& p, char* base, SelWs* w) {
    const size_t hist = 256, cnt = hist + (size_t)p.nb * 256 * 4;
    const size_t total = cnt + (((size_t)p.nb * 2 * 4 + 255) & ~(size_t)255);
    if (w) *w = SelWs{(uint32_t*)base, (uint32_t*)(base + hist), (uint32_t*)(base + cnt)};
    return total;
}

// Order-preserving u32 image of an f32 key (-0.0 as +0.0: equal keys, equal
// images): a > b as floats <=> image(a) > image(b).
__device__ inline uint32_t key_image(float x) {
    uint32_t b = x == 0.f ? 0u : __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Pass p = 0..3 over digit (image >> (24 - 8p)) & 255 of the keys whose higher
// digits equal the selected prefix: per-block histogram in LDS, written out as
// row hist[block][256].
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ keys, int n,
                                                          int chunk, int pass,
                                                          const uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t prefix = pass ? state[0] : 0u;
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const uint32_t u = key_image(keys[i]);
        // (pass 0 has no higher digits: every key matches)
        const bool match = pass == 0 || ((u ^ prefix) >> ((shift + 8) & 31)) == 0u;
        if (match) atomicAdd(&h[(u >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// One workgroup of 1024 threads: column sums of the histogram rows (four
// groups of 256 threads take every fourth row, sixteen loads in flight), a
// suffix scan over the digits, and the bucket holding the k-th largest of the
// matching keys: the one digit d with (keys of a larger digit) < (keys still
// to take) <= (keys of digit >= d).
__global__ __launch_bounds__(1024) void select_scan_kernel(const uint32_t* __restrict__ hist,
                                                           int nb, int pass, uint32_t k,
                                                           uint32_t* __restrict__ state) {
    __shared__ uint32_t part[4][256];
    __shared__ uint32_t wtot[4];
    const int d = threadIdx.x & 255, q = threadIdx.x >> 8;
    // (the state is read here, before the barriers, and written after them)
    const uint32_t left = pass ? state[1] : k;
    const uint32_t prefix = pass ? state[0] : 0u;
    uint32_t t = 0u;
    int b = q;
    for (; b + 60 < nb; b += 64) {
        uint32_t x[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) x[u] = hist[(int64_t)(b + 4 * u) * 256 + d];
#pragma unroll
        for (int u = 0; u < 16; ++u) t += x[u];
    }
    for (; b < nb; b += 4) t += hist[(int64_t)b * 256 + d];
    part[q][d] = t;
    __syncthreads();
    t = part[0][d] + part[1][d] + part[2][d] + part[3][d];
    // inclusive suffix sums over the digits: inside the wave, then across the
    // four waves of a group (the four groups compute the same values; group 0
    // publishes and writes)
    const int lane = d & 63, w = d >> 6;
    uint32_t incl = t;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = __shfl_down(incl, o);
        if (lane + o < 64) incl += x;
    }
    if (q == 0 && lane == 0) wtot[w] = incl;
    __syncthreads();
    for (int v = w + 1; v < 4; ++v) incl += wtot[v];
    const uint32_t above = incl - t;  // keys with a larger digit
    if (q == 0 && above < left && left <= incl) {
        const int shift = 24 - 8 * pass;
        state[0] = prefix | ((uint32_t)d << shift);
        state[1] = left - above;
    }
}

// Per block: keys above the threshold image and keys equal to it.
__global__ __launch_bounds__(256) void select_count_kernel(const float* __restrict__ keys, int n,
                                                           int chunk,
                                                           const uint32_t* __restrict__ state,
                                                           uint32_t* __restrict__ cnt) {
    __shared__ uint32_t c[2];
    if (threadIdx.x < 2) c[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t thr = state[0];
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    uint32_t gt = 0u, eq = 0u;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const uint32_t u = key_image(keys[i]);
        gt += u > thr;
        eq += u == thr;
    }
    atomicAdd(&c[0], gt);
    atomicAdd(&c[1], eq);
    __syncthreads();
    if (threadIdx.x < 2) cnt[2 * (int64_t)blockIdx.x + threadIdx.x] = c[threadIdx.x];
}

// Counted compaction: id i is taken if its key is above the threshold, or
// equal to it with fewer than `left` equal keys at lower ids; it lands at
// (taken ids below i) = (keys above below i) + min(equal keys below i, left).
__global__ __launch_bounds__(256) void select_write_kernel(const float* __restrict__ keys, int n,
                                                           int chunk, uint32_t k,
                                                           const uint32_t* __restrict__ state,
                                                           const uint32_t* __restrict__ cnt,
                                                           int32_t* __restrict__ ids_out) {
    __shared__ uint32_t base[2];
    __shared__ uint32_t wv[2][4][2];  // [buffer][wave][gt, eq]
    if (threadIdx.x < 2) base[threadIdx.x] = 0u;
    __syncthreads();
    // this block's prefix over the blocks before it (at most 256 of them)
    if ((int)threadIdx.x < (int)blockIdx.x) {
        atomicAdd(&base[0], cnt[2 * threadIdx.x]);
        atomicAdd(&base[1], cnt[2 * threadIdx.x + 1]);
    }
    __syncthreads();
    uint32_t run_gt = base[0], run_eq = base[1];
    const uint32_t thr = state[0], left = state[1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const int64_t i0 = (int64_t)blockIdx.x * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    int buf = 0;
    for (int64_t t0 = i0; t0 < i1; t0 += 256, buf ^= 1) {
        const int64_t i = t0 + threadIdx.x;
        bool gt = false, eq = false;
        if (i < i1) {
            const uint32_t u = key_image(keys[i]);
            gt = u > thr;
            eq = u == thr;
        }
        const uint64_t mg = __ballot(gt), me = __ballot(eq);
        if (lane == 0) {
            wv[buf][w][0] = (uint32_t)__popcll(mg);
            wv[buf][w][1] = (uint32_t)__popcll(me);
        }
        __syncthreads();  // (two buffers: the next tile's writes do not race these reads)
        uint32_t pg = run_gt + (uint32_t)__popcll(mg & below);
        uint32_t pe = run_eq + (uint32_t)__popcll(me & below);
        uint32_t tg = 0u, te = 0u;
        for (int v = 0; v < 4; ++v) {
            if (v < w) {
                pg += wv[buf][v][0];
                pe += wv[buf][v][1];
            }
            tg += wv[buf][v][0];
            te += wv[buf][v][1];
        }
        const uint32_t pos = pg + (pe < left ? pe : left);
        if ((gt || (eq && pe < left)) && pos < k) ids_out[pos] = (int32_t)i;
        run_gt += tg;
        run_eq += te;
    }
}

}  // namespace ml

using namespace ml;

extern "C" {

int mlearn_traj_importance_keys(const mlearn_rollout_view* ro, uint32_t k0, uint32_t k1,
                                const uint64_t* epoch_ctr, float* scores, float* keys,
                                double* lse_partials, mlearn_stream_t stream) {
    ML_REQUIRE(ro && scores && keys && lse_partials, "importance keys: null pointer");
    ML_REQUIRE(ro->advantages && ro->values, "importance keys: the view needs advantages and values");
    ML_REQUIRE(ro->bptt_len >= 1 && ro->T >= 1 && ro->T % ro->bptt_len == 0,
               "importance keys: bad bptt_len");
    ML_REQUIRE(ro->N >= 1 && (ro->T / ro->bptt_len) * ro->N <= (1ll << 30),
               "importance keys: sequences must be in [1, 2^30]");
    mlearn_rollout_view v = *ro;
    if (v.ld == 0) v.ld = v.N;
    ML_REQUIRE(v.ld >= v.N, "importance keys: ld %lld < N %lld", (long long)v.ld, (long long)v.N);
    const int n = (int)((v.T / v.bptt_len) * v.N);
    hipLaunchKernelGGL(importance_keys_kernel, dim3((n + kImpBlock - 1) / kImpBlock),
                       dim3(kImpBlock), 0, S(stream), v, k0, k1, epoch_ctr, n, scores, keys,
                       lse_partials);
    return check_launch("traj_importance_keys");
}

int mlearn_traj_importance_weights(const float* scores, const double* lse_partials, int32_t n,
                                   float* weights, mlearn_stream_t stream) {
    ML_REQUIRE(scores && lse_partials && weights, "importance weights: null pointer");
    ML_REQUIRE(n >= 1 && n <= (1 << 30), "importance weights: n must be in [1, 2^30], got %d", n);
    const int nparts = (n + kImpBlock - 1) / kImpBlock;
    hipLaunchKernelGGL(importance_weights_kernel, dim3(nparts), dim3(kImpBlock), 0, S(stream),
                       scores, lse_partials, n, nparts, weights);
    return check_launch("traj_importance_weights");
}

int64_t mlearn_select_topk_workspace_bytes(int32_t n) {
    if (n < 1 || n > (1 << 30)) return -1;
    return (int64_t)sel_carve(sel_plan(n), nullptr, nullptr);
}

int mlearn_select_topk_f32(const float* keys, int32_t n, int32_t k, int32_t* ids_out,
                           void* workspace, mlearn_stream_t stream) {
    ML_REQUIRE(keys && ids_out && workspace, "select_topk: null pointer");
    ML_REQUIRE(n >= 1 && n <= (1 << 30), "select_topk: n must be in [1, 2^30], got %d", n);
    ML_REQUIRE(k >= 1 && k <= n, "select_topk: k must be in [1, n = %d], got %d", n, k);
    const SelPlan p = sel_plan(n);
    SelWs w;
    sel_carve(p, (char*)workspace, &w);
    hipStream_t s = S(stream);
    for (int pass = 0; pass < 4; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(p.nb), dim3(256), 0, s, keys, n, p.chunk, pass,
                           w.state, w.hist);
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(1024), 0, s, w.hist, p.nb, pass,
                           (uint32_t)k, w.state);
    }
    hipLaunchKernelGGL(select_count_kernel, dim3(p.nb), dim3(256), 0, s, keys, n, p.chunk, w.state,
                       w.cnt);
    hipLaunchKernelGGL(select_write_kernel, dim3(p.nb), dim3(256), 0, s, keys, n, p.chunk,
                       (uint32_t)k, w.state, w.cnt, ids_out);
    return check_launch("select_topk");
}

}  // extern "C"
