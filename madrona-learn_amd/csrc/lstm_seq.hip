// The recurrent part of one LSTM layer over a whole BPTT chunk for the torch
// path (include/mlearn.h "LSTM sequence"; rnn.py MultiLayerLSTMCell: gates
// i, f, g, o, hidden kernel wh [R][4R] with bias b [4R], input kernel without
// bias).  The input projection zx = x wi of all T steps and the two weight
// gradients are single large GEMMs and stay with the caller; these kernels own
// what the time loop serialises.
//
//   One launch per time step over (ceil(N / 32), R / 32) workgroups of four
//   waves, one workgroup per (32 sequences, 32-unit block), the launch shape of
//   lstm_scan.h with a runtime width R (every multiple of 32 up to 512) and an
//   arbitrary N.  Products are transposed as in rowtile.h, Z^T = W^T X^T: the
//   weight image is the MFMA A operand, the 32 rows' natural-order fragments
//   (RT<T>::row) the B operand, so accumulator register q of lane (r, h) holds
//   unit (q & 3) + 8 (q >> 2) + 4 h of the block for row r.
//     forward step t:   wave g forms gate g's block of h_{t-1} wh over the
//                       whole K = R in one accumulator; the four blocks meet
//                       in LDS and wave j runs the cell for register quad j.
//     reverse step t:   wave g forms the K quarter g (gate g's columns of
//                       dG_{t+1}) of dh_t = dG_{t+1} wh^T; the quarters are
//                       added in the fixed order ((p0 + p1) + p2) + p3, then
//                       wave j runs the cell backward for register quad j.
//                       A trailing launch (t = -1) forms dh0 from dG_0.
//   The carries cross the launch boundary through memory: h into step t is the
//   row hprev[t] that step t - 1 wrote (zero where seq_ends[t - 1]; h0 at
//   t = 0, copied so that hprev is the weight gradient's operand), c into step
//   t is cs[t - 1] under the same mask, the c cotangent is one f32 [N][R] row
//   set in the workspace that each (row, unit)'s owner reads and overwrites.
//   A small launch ahead of each scan re-lays wh into the A-operand image of
//   that direction (img_index, natural k order).
//   Rows from N on in the last tile: their B fragments are zeros, nothing of
//   them is loaded or stored.  No atomics, no counters: the same inputs give
//   the same bits.
//
// f32 takes expf / tanhf / IEEE division in the cell, bf16 the hardware forms
// of rowtile.h (sigmoidf, tanh_fast): their ~1 ulp sits far below a bf16
// rounding, in f32 it would be the whole error budget of the parity bound.
#include "rowtile.h"

namespace ml {
namespace {

constexpr int kThreads = 256;
constexpr int kMinR = 32, kMaxR = 512;
constexpr int kChunk = 8;  // k-steps of A and B fragments in flight ahead of the MFMAs

template <typename T> struct Act;
template <> struct Act<bf16> {
    __device__ static float sig(float x) { return sigmoidf(x); }
    __device__ static float tanh(float x) { return tanh_fast(x); }
};
template <> struct Act<float> {
    __device__ static float sig(float x) { return 1.0f / (1.0f + expf(-x)); }
    __device__ static float tanh(float x) { return tanhf(x); }
};

inline int64_t image_bytes(int R, int32_t dtype) {
    const int64_t b = (int64_t)4 * R * R * (dtype == MLEARN_DTYPE_F32 ? 4 : 2);
    return (b + 255) / 256 * 256;
}

// wh [R][4R] -> the forward image Wimg[n = column][k = row] (K = R) or the
// reverse image Wimg[n = row][k = column] (K = 4R)
template <typename T>
__global__ __launch_bounds__(kThreads) void seq_image_kernel(const T* __restrict__ wh, int R,
                                                             int reverse, T* __restrict__ img) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= 4 * R * R) return;
    const int row = idx / (4 * R), col = idx - row * 4 * R;
    const int64_t o = reverse ? img_index<T>(row, col, 4 * R, false) : img_index<T>(col, row, R, false);
    img[o] = wh[idx];
}

// acc += sum_s Img[step s] x (fragment s of this lane's row), both streamed,
// kChunk steps of each loaded ahead of the MFMAs that use them; a lane whose
// row is not live multiplies zeros and loads nothing of it.  rowtile.h's
// gemm_stream is this product with a compile-time step count and a fully
// unrolled ring; here the count is a runtime value (2 .. 256 k-steps over the
// widths and dtypes), so the ring is a loop over chunks, and rows can be dead.
template <typename T>
__device__ inline void gemm_rows(f32x16& acc, const T* __restrict__ brow, bool live, int nks,
                                 const T* __restrict__ img, int lane) {
    typedef typename RT<T>::frag frag;
    constexpr int FB = 64 * RT<T>::E * (int)sizeof(T);
    const __amdgpu_buffer_rsrc_t rs = img_rsrc(img);
    const int voff = lane * RT<T>::E * (int)sizeof(T);
    const int h = lane >> 5;
    frag a[kChunk], b[kChunk], an[kChunk], bn[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
        a[i] = an[i] = RT<T>::zero();
        b[i] = bn[i] = RT<T>::zero();
        if (i < nks) {
            a[i] = img_load<T>(rs, voff, i * FB);
            if (live) b[i] = RT<T>::row(brow, i, h);
        }
    }
    for (int s0 = 0; s0 < nks; s0 += kChunk) {
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            const int s = s0 + kChunk + i;
            if (s < nks) {
                an[i] = img_load<T>(rs, voff, s * FB);
                if (live) bn[i] = RT<T>::row(brow, s, h);
            }
        }
        // (fences as in rowtile.h's rings: the next chunk's loads stay ahead
        // of this chunk's MFMAs instead of sinking down to their uses)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < kChunk; ++i)
            if (s0 + i < nks) acc = MT<T>::mma(a[i], b[i], acc);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < kChunk; ++i) {
            a[i] = an[i];
            b[i] = bn[i];
        }
    }
}

struct FwdK {
    const void *zx, *b, *h0, *c0;
    const uint8_t* ends;  // null: no step ends a sequence
    const void* img;
    void *hs, *cs, *gates, *hprev;
    int64_t N;
    int T, R;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void seq_fwd_step_kernel(FwdK a, int t) {
    __shared__ float part[4][16][64];  // gate block, accumulator register q, lane
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.y, R = a.R, nks = R / RT<T>::KS;
    const int64_t N = a.N, m = (int64_t)blockIdx.x * 32 + r;
    const bool live = m < N;
    const int64_t f = (int64_t)t * N + m;
    const T* hrow = t == 0 ? (const T*)a.h0 + m * R : (const T*)a.hprev + f * R;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const T* img = (const T*)a.img + (int64_t)(g * (R / 32) + w) * nks * 64 * RT<T>::E;
    gemm_rows<T>(acc, hrow, live, nks, img, lane);
#pragma unroll
    for (int q = 0; q < 16; ++q) part[g][q][lane] = acc[q];
    __syncthreads();
    if (!live) return;
    const int j = g, u0 = w * 32 + 8 * j + 4 * h;
    float4 cv;
    if (t == 0) {
        cv = load4((const T*)a.c0 + m * R + u0);
        const float4 hv = load4(hrow + u0);
        store4((T*)a.hprev + f * R + u0, hv.x, hv.y, hv.z, hv.w);
    } else if (a.ends && a.ends[f - N] != 0) {
        cv = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        cv = load4((const T*)a.cs + (f - N) * R + u0);
    }
    const bool more = t + 1 < a.T;
    const float keep = more && a.ends && a.ends[f] != 0 ? 0.f : 1.f;
    const T* zrow = (const T*)a.zx + f * 4 * R;
    float4 zv[4], bv[4];
#pragma unroll
    for (int gt = 0; gt < 4; ++gt) {
        zv[gt] = load4(zrow + gt * R + u0);
        bv[gt] = load4((const T*)a.b + gt * R + u0);
    }
    float gi[4], gf[4], gg[4], go[4], cn[4], hn[4], hc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = 4 * j + e;
        float z[4];
#pragma unroll
        for (int gt = 0; gt < 4; ++gt)
            z[gt] = f4get(zv[gt], e) + (part[gt][q][lane] + f4get(bv[gt], e));
        gi[e] = rnd<T>(Act<T>::sig(z[0]));
        gf[e] = rnd<T>(Act<T>::sig(z[1]));
        gg[e] = rnd<T>(Act<T>::tanh(z[2]));
        go[e] = rnd<T>(Act<T>::sig(z[3]));
        cn[e] = rnd<T>(gf[e] * f4get(cv, e) + gi[e] * gg[e]);
        hn[e] = rnd<T>(go[e] * Act<T>::tanh(cn[e]));
        hc[e] = keep * hn[e];
    }
    T* gts = (T*)a.gates + f * 4 * R;
    store4(gts + u0, gi[0], gi[1], gi[2], gi[3]);
    store4(gts + R + u0, gf[0], gf[1], gf[2], gf[3]);
    store4(gts + 2 * R + u0, gg[0], gg[1], gg[2], gg[3]);
    store4(gts + 3 * R + u0, go[0], go[1], go[2], go[3]);
    store4((T*)a.cs + f * R + u0, cn[0], cn[1], cn[2], cn[3]);
    store4((T*)a.hs + f * R + u0, hn[0], hn[1], hn[2], hn[3]);
    if (more) store4((T*)a.hprev + (f + N) * R + u0, hc[0], hc[1], hc[2], hc[3]);
}

struct BwdK {
    const void *dhs, *c0, *cs, *gates;
    const uint8_t* ends;
    const void* img;
    float* dcc;  // [N][R] c cotangent into the step being run
    void *dg, *dh0, *dc0;
    int64_t N;
    int T, R;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void seq_bwd_step_kernel(BwdK a, int t) {
    __shared__ float part[4][16][64];  // K quarter, accumulator register q, lane
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = blockIdx.y, R = a.R, nq = R / RT<T>::KS;
    const int64_t N = a.N, m = (int64_t)blockIdx.x * 32 + r;
    const bool live = m < N;
    const bool cell = t >= 0, prod = t + 1 < a.T;
    const int64_t f = (int64_t)t * N + m;  // (not dereferenced at t = -1)
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    if (prod) {
        const T* brow = (const T*)a.dg + (f + N) * 4 * R + g * R;
        const T* img = (const T*)a.img + (int64_t)(w * 4 + g) * nq * 64 * RT<T>::E;
        gemm_rows<T>(acc, brow, live, nq, img, lane);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) part[g][q][lane] = acc[q];
    __syncthreads();
    if (!live) return;
    const int j = g, u0 = w * 32 + 8 * j + 4 * h;
    float dhh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = 4 * j + e;
        dhh[e] = ((part[0][q][lane] + part[1][q][lane]) + part[2][q][lane]) + part[3][q][lane];
    }
    if (!cell) {
        store4((T*)a.dh0 + m * R + u0, dhh[0], dhh[1], dhh[2], dhh[3]);
        return;
    }
    const bool cut = !prod || (a.ends && a.ends[f] != 0);
    const T* gts = (const T*)a.gates + f * 4 * R;
    const float4 dho = load4((const T*)a.dhs + f * R + u0);
    const float4 gi = load4(gts + u0), gf = load4(gts + R + u0);
    const float4 gg = load4(gts + 2 * R + u0), go = load4(gts + 3 * R + u0);
    const float4 c4 = load4((const T*)a.cs + f * R + u0);
    float4 ci;
    if (t == 0) ci = load4((const T*)a.c0 + m * R + u0);
    else if (a.ends && a.ends[f - N] != 0) ci = make_float4(0.f, 0.f, 0.f, 0.f);
    else ci = load4((const T*)a.cs + (f - N) * R + u0);
    float* dcrow = a.dcc + m * R + u0;
    const float4 dcin = cut ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)dcrow;
    float dpi[4], dpf[4], dpg[4], dpo[4], dco[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float i_ = f4get(gi, e), f_ = f4get(gf, e), g_ = f4get(gg, e), o_ = f4get(go, e);
        const float dh = f4get(dho, e) + (cut ? 0.f : dhh[e]);
        const float tc = Act<T>::tanh(f4get(c4, e));
        const float dc = f4get(dcin, e) + dh * o_ * (1.f - tc * tc);
        dpi[e] = rnd<T>((dc * g_) * i_ * (1.f - i_));
        dpf[e] = rnd<T>((dc * f4get(ci, e)) * f_ * (1.f - f_));
        dpg[e] = rnd<T>((dc * i_) * (1.f - g_ * g_));
        dpo[e] = rnd<T>((dh * tc) * o_ * (1.f - o_));
        dco[e] = dc * f_;
    }
    if (t > 0) *(float4*)dcrow = make_float4(dco[0], dco[1], dco[2], dco[3]);
    else store4((T*)a.dc0 + m * R + u0, dco[0], dco[1], dco[2], dco[3]);
    T* dgs = (T*)a.dg + f * 4 * R;
    store4(dgs + u0, dpi[0], dpi[1], dpi[2], dpi[3]);
    store4(dgs + R + u0, dpf[0], dpf[1], dpf[2], dpf[3]);
    store4(dgs + 2 * R + u0, dpg[0], dpg[1], dpg[2], dpg[3]);
    store4(dgs + 3 * R + u0, dpo[0], dpo[1], dpo[2], dpo[3]);
}

int check_shape(const char* what, int32_t T, int64_t N, int32_t R, int32_t dtype) {
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(R >= kMinR && R <= kMaxR && R % 32 == 0,
               "%s: hidden = %d is not a multiple of 32 in %d..%d", what, R, kMinR, kMaxR);
    ML_REQUIRE(T >= 1, "%s: steps = %d must be >= 1", what, T);
    ML_REQUIRE(N >= 1 && (N + 31) / 32 <= 0x7fffffff, "%s: rows = %lld outside 1..2^36",
               what, (long long)N);
    return MLEARN_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
void launch_image(const void* wh, int R, int reverse, void* img, hipStream_t st) {
    const unsigned blocks = (unsigned)((4 * R * R + kThreads - 1) / kThreads);
    hipLaunchKernelGGL((seq_image_kernel<T>), dim3(blocks), dim3(kThreads), 0, st, (const T*)wh, R,
                       reverse, (T*)img);
}

}  // namespace
}  // namespace ml

extern "C" {

int64_t mlearn_lstm_seq_workspace_bytes(int64_t N, int32_t hidden, int32_t dtype) {
    using namespace ml;
    if (hidden < kMinR || hidden > kMaxR || hidden % 32 != 0 || N < 1) return -1;
    if (dtype != MLEARN_DTYPE_F32 && dtype != MLEARN_DTYPE_BF16) return -1;
    return image_bytes(hidden, dtype) + N * hidden * (int64_t)sizeof(float);
}

int mlearn_lstm_seq_fwd(const void* zx, const void* wh, const void* b, const void* h0,
                        const void* c0, const uint8_t* seq_ends, int32_t T, int64_t N,
                        int32_t hidden, int32_t dtype, void* hs, void* cs, void* gates,
                        void* hprev, void* workspace, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_shape("lstm_seq_fwd", T, N, hidden, dtype)) return rc;
    ML_REQUIRE(zx && wh && b && h0 && c0 && hs && cs && gates && hprev && workspace,
               "lstm_seq_fwd: null pointer (zx, wh, b, h0, c0, hs, cs, gates, hprev or workspace)");
    ML_REQUIRE(aligned16(zx) && aligned16(wh) && aligned16(b) && aligned16(h0) && aligned16(c0) &&
                   aligned16(hs) && aligned16(cs) && aligned16(gates) && aligned16(hprev) &&
                   aligned16(workspace),
               "lstm_seq_fwd: a tensor or the workspace is not 16-byte aligned");
    const FwdK a = {zx, b, h0, c0, seq_ends, workspace, hs, cs, gates, hprev, N, T, hidden};
    const dim3 grid((unsigned)((N + 31) / 32), (unsigned)(hidden / 32));
    (void)hipGetLastError();
    if (dtype == MLEARN_DTYPE_F32) launch_image<float>(wh, hidden, 0, workspace, S(stream));
    else launch_image<bf16>(wh, hidden, 0, workspace, S(stream));
    if (int rc = check_launch("lstm_seq_fwd (weight image)")) return rc;
    for (int t = 0; t < T; ++t) {
        if (dtype == MLEARN_DTYPE_F32)
            hipLaunchKernelGGL((seq_fwd_step_kernel<float>), grid, dim3(kThreads), 0, S(stream), a, t);
        else
            hipLaunchKernelGGL((seq_fwd_step_kernel<bf16>), grid, dim3(kThreads), 0, S(stream), a, t);
    }
    return check_launch("lstm_seq_fwd");
}

int mlearn_lstm_seq_bwd(const void* dhs, const void* wh, const void* c0, const uint8_t* seq_ends,
                        const void* cs, const void* gates, int32_t T, int64_t N, int32_t hidden,
                        int32_t dtype, void* dg, void* dh0, void* dc0, void* workspace,
                        mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_shape("lstm_seq_bwd", T, N, hidden, dtype)) return rc;
    ML_REQUIRE(dhs && wh && c0 && cs && gates && dg && dh0 && dc0 && workspace,
               "lstm_seq_bwd: null pointer (dhs, wh, c0, cs, gates, dg, dh0, dc0 or workspace)");
    ML_REQUIRE(aligned16(dhs) && aligned16(wh) && aligned16(c0) && aligned16(cs) &&
                   aligned16(gates) && aligned16(dg) && aligned16(dh0) && aligned16(dc0) &&
                   aligned16(workspace),
               "lstm_seq_bwd: a tensor or the workspace is not 16-byte aligned");
    float* dcc = (float*)((char*)workspace + image_bytes(hidden, dtype));
    const BwdK a = {dhs, c0, cs, gates, seq_ends, workspace, dcc, dg, dh0, dc0, N, T, hidden};
    const dim3 grid((unsigned)((N + 31) / 32), (unsigned)(hidden / 32));
    (void)hipGetLastError();
    if (dtype == MLEARN_DTYPE_F32) launch_image<float>(wh, hidden, 1, workspace, S(stream));
    else launch_image<bf16>(wh, hidden, 1, workspace, S(stream));
    if (int rc = check_launch("lstm_seq_bwd (weight image)")) return rc;
    for (int t = T - 1; t >= -1; --t) {
        if (dtype == MLEARN_DTYPE_F32)
            hipLaunchKernelGGL((seq_bwd_step_kernel<float>), grid, dim3(kThreads), 0, S(stream), a, t);
        else
            hipLaunchKernelGGL((seq_bwd_step_kernel<bf16>), grid, dim3(kThreads), 0, S(stream), a, t);
    }
    return check_launch("lstm_seq_bwd");
}

}  // extern "C"
