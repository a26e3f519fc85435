// HL-Gauss critic heads on the torch path (include/mlearn.h "HL-Gauss
// heads"): mean(), loss (+ mean) and the loss' gradient of HLGaussDist over
// one part, or of HLGaussTwoPartDist over two (small head, large head), one
// launch each.
//
//   One row per aligned group of 32 lanes of a 256-thread workgroup (8 rows
//   per workgroup).  The tables of both parts are staged into LDS once per
//   workgroup; each group stages its row's logits of one part as f32 (lane
//   `sub` loads bins sub, sub + 32, ...: 128-byte segments per group, any row
//   stride, any base alignment, f32 or bf16), runs the group functions of
//   dists.h on them (twohot_mean_g / hlgauss_ce_g, the fused step's own
//   arithmetic) and then does the same for the second part in the same LDS
//   row.  20 KB of LDS per workgroup: 8 workgroups (8 waves per SIMD) per CU.
//   Every lane of the workgroup runs the whole body (rows past R recompute
//   row R - 1 and store nothing), so the barriers are unconditional.
//   Every output element has one writer, nothing is accumulated across rows:
//   a row's results do not depend on the grid or on the other rows.
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
constexpr int kRows = kThreads / kG;    // rows per workgroup
constexpr int kMaxBins = 255;
constexpr int kLd = kMaxBins + 1;       // LDS row length (bounds: num_bins + 1 <= 256)
constexpr int kPerLane = kLd / kG;      // bins of one lane

struct HlIo {
    const void* lg[2];   // logits of each part
    int64_t ld[2];       // their row strides (elements)
    void* d[2];          // d_logits of each part (bwd)
    int64_t ldd[2];
};

enum { kMean = 0, kLoss = 1, kBwd = 2 };

__device__ inline void hl_store(void* p, int32_t dtype, int64_t i, float v) {
    if (dtype == MLEARN_DTYPE_F32) ((float*)p)[i] = v;
    else ((uint16_t*)p)[i] = __builtin_bit_cast(uint16_t, (bf16)v);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void hlgauss_kernel(
    mlearn_hlgauss_tables tab, HlIo io, int32_t dtype, int64_t R, const float* targets,
    const float* g_loss, const float* g_mean, float* loss, float* mean) {
    __shared__ float s_c[2][kLd];
    __shared__ float s_b[2][kLd];
    __shared__ float s_lg[kRows][kLd];
    __shared__ float s_cw[kRows][kLd];
    const int tid = threadIdx.x, g = tid / kG, sub = tid % kG;
    for (int p = 0; p < tab.num_parts; ++p) {
        const int nb = tab.num_bins[p];
        for (int j = tid; j < nb; j += kThreads) s_c[p][j] = tab.centers[p][j];
        if (MODE != kMean)
            for (int j = tid; j <= nb; j += kThreads) s_b[p][j] = tab.bounds[p][j];
    }
    const int64_t row = (int64_t)blockIdx.x * kRows + g;
    const bool valid = row < R;
    const int64_t rr = valid ? row : R - 1;
    // HLGaussTwoPartDist.loss: small = t mod (sign(t) 2) = fmod(t, 2), large = t - small
    float tp[2] = {0.f, 0.f};
    if (MODE != kMean) {
        const float t = targets[rr];
        if (tab.num_parts == 2) {
            tp[0] = fmodf(t, 2.0f);
            tp[1] = t - tp[0];
        } else {
            tp[0] = t;
        }
    }
    const float gl = (MODE == kBwd && g_loss) ? g_loss[rr] : 0.f;
    const float gm = (MODE == kBwd && g_mean) ? g_mean[rr] : 0.f;
    float lsum = 0.f, msum = 0.f;
    for (int p = 0; p < tab.num_parts; ++p) {
        const int nb = tab.num_bins[p];
        float* lg = s_lg[g];
        __syncthreads();  // the tables (p = 0); the previous part's reads of this row
        for (int j = sub; j < nb; j += kG) lg[j] = cont_load(io.lg[p], dtype, rr * io.ld[p] + j);
        __syncthreads();
        if (MODE == kMean) {
            float mx, se;
            msum = p == 0 ? twohot_mean_g<kG>(lg, nb, s_c[p], sub, &mx, &se)
                          : msum + twohot_mean_g<kG>(lg, nb, s_c[p], sub, &mx, &se);
        } else if (MODE == kLoss) {
            float m;
            const float l = hlgauss_ce_g<kG>(lg, nb, tp[p], s_c[p], s_b[p], tab.smoothness, 0.f,
                                             sub, s_cw[g], &m);
            lsum = p == 0 ? l : lsum + l;
            msum = p == 0 ? m : msum + m;
        } else {
            // g_mean p_j (center_j - mean_part) of this lane's bins, from the
            // logits before hlgauss_ce_g replaces them by g_loss (sum c p_j - c_j)
            float extra[kPerLane];
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) extra[k] = 0.f;
            if (g_mean) {
                float mx, se;
                const float m = twohot_mean_g<kG>(lg, nb, s_c[p], sub, &mx, &se);
#pragma unroll
                for (int k = 0; k < kPerLane; ++k) {
                    const int j = sub + k * kG;
                    if (j < nb) extra[k] = gm * mean_dlogit(lg, s_c[p], j, mx, se, m);
                }
            }
            float m;
            (void)hlgauss_ce_g<kG>(lg, nb, tp[p], s_c[p], s_b[p], tab.smoothness, gl, sub,
                                   s_cw[g], &m);
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) {
                const int j = sub + k * kG;
                if (j < nb && valid)
                    hl_store(io.d[p], dtype, row * io.ldd[p] + j, lg[j] + extra[k]);
            }
        }
    }
    if (MODE != kBwd && valid && sub == 0) {
        if (MODE == kLoss) loss[row] = lsum;
        if (mean) mean[row] = msum;
    }
}

// ---------------------------------------------------------------------------
// argument checks (before any pointer is followed or the device is touched)
// ---------------------------------------------------------------------------
int check_args(const char* what, const mlearn_hlgauss_tables* t, const void* const lg[2],
               const int64_t ld[2], int32_t dtype, int64_t R) {
    ML_REQUIRE(t, "%s: tables is null", what);
    ML_REQUIRE(t->num_parts == 1 || t->num_parts == 2, "%s: num_parts %d outside {1, 2}", what,
               t->num_parts);
    for (int p = 0; p < t->num_parts; ++p) {
        const int nb = t->num_bins[p];
        ML_REQUIRE(nb >= 3 && nb <= kMaxBins && nb % 2 == 1,
                   "%s: num_bins[%d] = %d must be odd and within 3..%d", what, p, nb, kMaxBins);
        ML_REQUIRE(t->centers[p], "%s: centers[%d] is null", what, p);
        ML_REQUIRE(t->bounds[p], "%s: bounds[%d] is null", what, p);
    }
    ML_REQUIRE(t->smoothness > 0.f && t->smoothness < INFINITY,
               "%s: smoothness %g is not a positive finite number", what, (double)t->smoothness);
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(R >= 0, "%s: R = %lld is negative", what, (long long)R);
    ML_REQUIRE((R + kRows - 1) / kRows <= 0x7fffffff, "%s: R = %lld is too large", what,
               (long long)R);
    for (int p = 0; p < t->num_parts; ++p)
        ML_REQUIRE(ld[p] >= t->num_bins[p], "%s: ld_logits[%d] = %lld below num_bins[%d] = %d",
                   what, p, (long long)ld[p], p, t->num_bins[p]);
    if (R > 0)
        for (int p = 0; p < t->num_parts; ++p)
            ML_REQUIRE(lg[p], "%s: logits[%d] is null", what, p);
    return MLEARN_OK;
}

template <int MODE>
int launch(const char* what, const mlearn_hlgauss_tables* t, const HlIo& io, int32_t dtype,
           int64_t R, const float* targets, const float* g_loss, const float* g_mean, float* loss,
           float* mean, mlearn_stream_t stream) {
    const unsigned blocks = (unsigned)((R + kRows - 1) / kRows);
    (void)hipGetLastError();
    hipLaunchKernelGGL(hlgauss_kernel<MODE>, dim3(blocks), dim3(kThreads), 0, S(stream), *t, io,
                       dtype, R, targets, g_loss, g_mean, loss, mean);
    return check_launch(what);
}

}  // namespace
}  // namespace ml

extern "C" {

int mlearn_hlgauss_mean(const mlearn_hlgauss_tables* tables, const void* logits0, int64_t ld0,
                        const void* logits1, int64_t ld1, int32_t dtype, int64_t R, float* mean,
                        mlearn_stream_t stream) {
    using namespace ml;
    const void* const lg[2] = {logits0, logits1};
    const int64_t ld[2] = {ld0, ld1};
    if (int rc = check_args("hlgauss_mean", tables, lg, ld, dtype, R)) return rc;
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(mean, "hlgauss_mean: mean is null");
    const HlIo io = {{logits0, logits1}, {ld0, ld1}, {nullptr, nullptr}, {0, 0}};
    return launch<kMean>("hlgauss_mean", tables, io, dtype, R, nullptr, nullptr, nullptr, nullptr,
                         mean, stream);
}

int mlearn_hlgauss_loss(const mlearn_hlgauss_tables* tables, const void* logits0, int64_t ld0,
                        const void* logits1, int64_t ld1, int32_t dtype, const float* targets,
                        int64_t R, float* loss, float* mean, mlearn_stream_t stream) {
    using namespace ml;
    const void* const lg[2] = {logits0, logits1};
    const int64_t ld[2] = {ld0, ld1};
    if (int rc = check_args("hlgauss_loss", tables, lg, ld, dtype, R)) return rc;
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(targets, "hlgauss_loss: targets is null");
    ML_REQUIRE(loss, "hlgauss_loss: loss is null");
    const HlIo io = {{logits0, logits1}, {ld0, ld1}, {nullptr, nullptr}, {0, 0}};
    return launch<kLoss>("hlgauss_loss", tables, io, dtype, R, targets, nullptr, nullptr, loss,
                         mean, stream);
}

int mlearn_hlgauss_loss_bwd(const mlearn_hlgauss_tables* tables, const void* logits0, int64_t ld0,
                            const void* logits1, int64_t ld1, int32_t dtype, const float* targets,
                            const float* g_loss, const float* g_mean, void* d_logits0,
                            int64_t ld_d0, void* d_logits1, int64_t ld_d1, int64_t R,
                            mlearn_stream_t stream) {
    using namespace ml;
    const void* const lg[2] = {logits0, logits1};
    const int64_t ld[2] = {ld0, ld1};
    if (int rc = check_args("hlgauss_loss_bwd", tables, lg, ld, dtype, R)) return rc;
    void* const d[2] = {d_logits0, d_logits1};
    const int64_t ldd[2] = {ld_d0, ld_d1};
    for (int p = 0; p < tables->num_parts; ++p)
        ML_REQUIRE(ldd[p] >= tables->num_bins[p],
                   "hlgauss_loss_bwd: ld_d_logits[%d] = %lld below num_bins[%d] = %d", p,
                   (long long)ldd[p], p, tables->num_bins[p]);
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(targets, "hlgauss_loss_bwd: targets is null");
    for (int p = 0; p < tables->num_parts; ++p)
        ML_REQUIRE(d[p], "hlgauss_loss_bwd: d_logits[%d] is null", p);
    const HlIo io = {{logits0, logits1}, {ld0, ld1}, {d_logits0, d_logits1}, {ld_d0, ld_d1}};
    return launch<kBwd>("hlgauss_loss_bwd", tables, io, dtype, R, targets, g_loss, g_mean, nullptr,
                        nullptr, stream);
}

}  // extern "C"
