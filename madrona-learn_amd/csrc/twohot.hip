// Two-hot critic head on the torch path (include/mlearn.h "Two-hot critic
// head"): mean(), two_hot_cross_entropy_loss (+ mean) and their gradient of a
// SymExpTwoHotDistribution over num_bins logits, one launch each.
//
//   One row per aligned group of 32 lanes of a 256-thread workgroup (8 rows
//   per pass).  The workgroup forms the bin table (twohot_bin: one expm1f per
//   bin) in LDS once and then walks its passes, workgroup b taking passes b,
//   b + grid, ...: at most 2048 workgroups, so the table's cost is spread over
//   the rows.  Each group stages its row's logits as f32 (lane `sub` loads
//   bins sub, sub + 32, ...: 128-byte segments, any row stride, any base
//   alignment, f32 or bf16) and runs the group functions of dists.h on them
//   (twohot_mean_g / twohot_ce_g, the fused step's own arithmetic).  9 KB of
//   LDS per workgroup.  Every lane runs every pass of its workgroup (rows past
//   R recompute row R - 1 and store nothing), so the barriers are
//   unconditional.  Every output element has one writer, nothing is
//   accumulated across rows: a row's results do not depend on the grid or on
//   the other rows.
//
// No contraction in this file, the group functions of dists.h included: the
// mirrored pairs of mean() cancel exactly at zero logits only as two rounded
// products (an fma of one pair would leave the other product's rounding).
#pragma clang fp contract(off)
#include "continuous.h"  // cont_load
#include "dists.h"

namespace ml {
namespace {

constexpr int kThreads = 256;
constexpr int kG = 32;                  // lanes per row
constexpr int kRows = kThreads / kG;    // rows per pass
constexpr int kMaxBins = 255;
constexpr int kLd = kMaxBins + 1;       // LDS row length
constexpr int kPerLane = kLd / kG;      // bins of one lane
constexpr int kMaxBlocks = 2048;

enum { kMean = 0, kLoss = 1, kBwd = 2 };

struct ThArgs {
    const void* lg;
    int64_t ld;
    void* d;
    int64_t ldd;
    int32_t dtype, nb;
    int64_t R, tiles;
    const float *targets, *g_loss, *g_mean;
    float *loss, *mean;
};

template <int MODE>
__global__ __launch_bounds__(kThreads) void twohot_kernel(ThArgs a) {
    __shared__ float s_b[kLd];
    __shared__ float s_lg[kRows][kLd];
    const int tid = threadIdx.x, g = tid / kG, sub = tid % kG;
    const int nb = a.nb;
    for (int j = tid; j < nb; j += kThreads) s_b[j] = twohot_bin(j, nb);
    float* lg = s_lg[g];
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t row = tile * kRows + g;
        const bool valid = row < a.R;
        const int64_t rr = valid ? row : a.R - 1;
        __syncthreads();  // the table (first pass); the previous pass' reads of this row
        for (int j = sub; j < nb; j += kG) lg[j] = cont_load(a.lg, a.dtype, rr * a.ld + j);
        __syncthreads();
        if (MODE == kMean) {
            float mx, se;
            const float m = twohot_mean_g<kG>(lg, nb, s_b, sub, &mx, &se);
            if (valid && sub == 0) a.mean[row] = m;
        } else if (MODE == kLoss) {
            float m;
            const float l = twohot_ce_g<kG>(lg, nb, a.targets[rr], s_b, 0.f, sub, &m);
            if (valid && sub == 0) {
                a.loss[row] = l;
                if (a.mean) a.mean[row] = m;
            }
        } else {
            // g_mean p_j (bin_j - mean) of this lane's bins, from the logits
            // before twohot_ce_g replaces them by g_loss (p_j - twohot_j)
            float extra[kPerLane];
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) extra[k] = 0.f;
            if (a.g_mean) {
                const float gm = a.g_mean[rr];
                float mx, se;
                const float m = twohot_mean_g<kG>(lg, nb, s_b, sub, &mx, &se);
#pragma unroll
                for (int k = 0; k < kPerLane; ++k) {
                    const int j = sub + k * kG;
                    if (j < nb) extra[k] = gm * mean_dlogit(lg, s_b, j, mx, se, m);
                }
            }
            float m;
            (void)twohot_ce_g<kG>(lg, nb, a.targets[rr], s_b, a.g_loss ? a.g_loss[rr] : 0.f, sub,
                                  &m);
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) {
                const int j = sub + k * kG;
                if (j < nb && valid) {
                    const float v = lg[j] + extra[k];
                    if (a.dtype == MLEARN_DTYPE_F32) ((float*)a.d)[row * a.ldd + j] = v;
                    else ((uint16_t*)a.d)[row * a.ldd + j] = __builtin_bit_cast(uint16_t, (bf16)v);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// argument checks (before any pointer is followed or the device is touched)
// ---------------------------------------------------------------------------
int check_args(const char* what, const void* lg, int64_t ld, int32_t dtype, int32_t nb,
               int64_t R) {
    ML_REQUIRE(nb >= 3 && nb <= kMaxBins && nb % 2 == 1,
               "%s: num_bins = %d must be odd and within 3..%d", what, nb, kMaxBins);
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(R >= 0, "%s: R = %lld is negative", what, (long long)R);
    ML_REQUIRE(ld >= nb, "%s: ld_logits = %lld below num_bins = %d", what, (long long)ld, nb);
    if (R > 0) ML_REQUIRE(lg, "%s: logits is null", what);
    return MLEARN_OK;
}

template <int MODE> int launch(const char* what, ThArgs a, mlearn_stream_t stream) {
    a.tiles = (a.R + kRows - 1) / kRows;
    const unsigned blocks = (unsigned)(a.tiles < kMaxBlocks ? a.tiles : kMaxBlocks);
    (void)hipGetLastError();
    hipLaunchKernelGGL(twohot_kernel<MODE>, dim3(blocks), dim3(kThreads), 0, S(stream), a);
    return check_launch(what);
}

}  // namespace
}  // namespace ml

extern "C" {

int mlearn_twohot_mean(const void* logits, int64_t ld, int32_t dtype, int32_t num_bins, int64_t R,
                       float* mean, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("twohot_mean", logits, ld, dtype, num_bins, R)) return rc;
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(mean, "twohot_mean: mean is null");
    ThArgs a = {};
    a.lg = logits, a.ld = ld, a.dtype = dtype, a.nb = num_bins, a.R = R, a.mean = mean;
    return launch<kMean>("twohot_mean", a, stream);
}

int mlearn_twohot_loss(const void* logits, int64_t ld, int32_t dtype, int32_t num_bins,
                       const float* targets, int64_t R, float* loss, float* mean,
                       mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("twohot_loss", logits, ld, dtype, num_bins, R)) return rc;
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(targets, "twohot_loss: targets is null");
    ML_REQUIRE(loss, "twohot_loss: loss is null");
    ThArgs a = {};
    a.lg = logits, a.ld = ld, a.dtype = dtype, a.nb = num_bins, a.R = R;
    a.targets = targets, a.loss = loss, a.mean = mean;
    return launch<kLoss>("twohot_loss", a, stream);
}

int mlearn_twohot_loss_bwd(const void* logits, int64_t ld, int32_t dtype, int32_t num_bins,
                           const float* targets, const float* g_loss, const float* g_mean,
                           void* d_logits, int64_t ld_d, int64_t R, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("twohot_loss_bwd", logits, ld, dtype, num_bins, R)) return rc;
    ML_REQUIRE(ld_d >= num_bins, "twohot_loss_bwd: ld_d_logits = %lld below num_bins = %d",
               (long long)ld_d, num_bins);
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(targets, "twohot_loss_bwd: targets is null");
    ML_REQUIRE(d_logits, "twohot_loss_bwd: d_logits is null");
    ThArgs a = {};
    a.lg = logits, a.ld = ld, a.d = d_logits, a.ldd = ld_d, a.dtype = dtype, a.nb = num_bins;
    a.R = R, a.targets = targets, a.g_loss = g_loss, a.g_mean = g_mean;
    return launch<kBwd>("twohot_loss_bwd", a, stream);
}

}  // extern "C"
