// Continuous actions on the torch path (include/mlearn.h "Continuous
// actions"): the sampler, action_stats and its gradient.  Streaming kernels:
// no reuse, no LDS, no atomics; every output element has one writer, so the
// results do not depend on the grid.
//
//   sampler: one lane per (row, block of 4 columns) = one Philox block, four
//     normals; 16-byte action / log-prob stores when A % 4 == 0, vector input
//     loads when the row bases are aligned as well.
//   stats / stats_bwd: a grid-stride loop (grid from device_cus(), not from
//     R) over 16-byte chunks of the flat [R * A] index when every row stride
//     equals A and the bases are aligned (4 f32 or 8 bf16 inputs per lane and
//     trip), else one element per lane and trip through the row strides.
//   The per-group (std_min, std_max) come from the by-value layout struct.
#include "continuous.h"

namespace ml {
namespace {

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;

__device__ inline float bf16_bits_to_f32(uint16_t b) {
    const uint32_t bits = (uint32_t)b << 16;
    return __builtin_bit_cast(float, bits);
}
__device__ inline uint16_t f32_to_bf16_bits(float x) {
    return __builtin_bit_cast(uint16_t, (bf16)x);
}
__device__ inline void cont_store(void* p, int32_t dtype, int64_t i, float v) {
    if (dtype == MLEARN_DTYPE_F32) ((float*)p)[i] = v;
    else ((uint16_t*)p)[i] = f32_to_bf16_bits(v);
}

// V elements of T (float, or uint16_t holding bf16 bits) as one 16-byte
// access, to / from f32
template <typename T> struct Chunk;
template <> struct Chunk<float> {
    static constexpr int V = 4;
    __device__ static void load(const void* p, int64_t i, float* o) {
        const f32x4 v = *(const f32x4*)((const float*)p + i);
        for (int j = 0; j < 4; ++j) o[j] = v[j];
    }
    __device__ static void store(void* p, int64_t i, const float* x) {
        f32x4 v;
        for (int j = 0; j < 4; ++j) v[j] = x[j];
        *(f32x4*)((float*)p + i) = v;
    }
};
template <> struct Chunk<uint16_t> {
    static constexpr int V = 8;
    __device__ static void load(const void* p, int64_t i, float* o) {
        const u16x8 v = *(const u16x8*)((const uint16_t*)p + i);
        for (int j = 0; j < 8; ++j) o[j] = bf16_bits_to_f32(v[j]);
    }
    __device__ static void store(void* p, int64_t i, const float* x) {
        u16x8 v;
        for (int j = 0; j < 8; ++j) v[j] = f32_to_bf16_bits(x[j]);
        *(u16x8*)((uint16_t*)p + i) = v;
    }
};
// V consecutive f32 (V = 4 or 8) as 16-byte accesses
template <int V> __device__ inline void load_f32(const float* p, int64_t i, float* o) {
    for (int c = 0; c < V; c += 4) Chunk<float>::load(p, i + c, o + c);
}
template <int V> __device__ inline void store_f32(float* p, int64_t i, const float* x) {
    for (int c = 0; c < V; c += 4) Chunk<float>::store(p, i + c, x + c);
}

// ---------------------------------------------------------------------------
// sampler
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void cont_sample_kernel(
    const void* means, int64_t ldm, const void* stds, int64_t lds_, int32_t dtype,
    mlearn_continuous_layout lay, int64_t N, int32_t nb, int32_t vin, int32_t vout, uint32_t k0,
    uint32_t k1, const uint64_t* step_ctr, uint64_t step_add, uint32_t env_offset, int32_t sample,
    float* actions, float* logp) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= N * nb) return;
    const int64_t n = i / nb;
    const int b = (int)(i - n * nb);
    const int A = lay.num_groups * lay.num_dims;
    const int e0 = 4 * b, cnt = min(4, A - e0);
    float x[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f};
    if (vin) {  // A % 4 == 0: cnt == 4, every quad of the row is aligned
        if (dtype == MLEARN_DTYPE_F32) {
            Chunk<float>::load(means, n * ldm + e0, x);
            Chunk<float>::load(stds, n * lds_ + e0, y);
        } else {
            const u16x4 mx = *(const u16x4*)((const uint16_t*)means + n * ldm + e0);
            const u16x4 my = *(const u16x4*)((const uint16_t*)stds + n * lds_ + e0);
            for (int j = 0; j < 4; ++j) {
                x[j] = bf16_bits_to_f32(mx[j]);
                y[j] = bf16_bits_to_f32(my[j]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) {
                x[j] = cont_load(means, dtype, n * ldm + e0 + j);
                y[j] = cont_load(stds, dtype, n * lds_ + e0 + j);
            }
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (sample) {
        const uint64_t step = (step_ctr ? *step_ctr : 0ull) + step_add;
        cont_normals4(k0, k1, env_offset + (uint32_t)n, step, (uint32_t)b, z);
    }
    float a[4], lp[4];
    cont_sample4(x, y, z, lay, e0, cnt, sample, logp != nullptr, a, lp);
    const int64_t o = n * A + e0;
    if (vout) {
        Chunk<float>::store(actions, o, a);
        if (logp) Chunk<float>::store(logp, o, lp);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) {
                actions[o + j] = a[j];
                if (logp) logp[o + j] = lp[j];
            }
    }
}

// ---------------------------------------------------------------------------
// action_stats and its gradient, one column
// ---------------------------------------------------------------------------
__device__ inline void stats_elem(float x, float y, float a, float lo, float hi, float* lp,
                                  float* en) {
#pragma clang fp contract(off)
    const float m = tanhf(x);
    const float s = cont_std(cont_sigmoid(y), lo, hi);
    const float ls = logf(s);
    *lp = cont_logp((a - m) / s, ls);
    *en = cont_entropy(ls);
}

__device__ inline void stats_bwd_elem(float x, float y, float a, float lo, float hi, float glp,
                                      float gen, float* dx, float* dy) {
#pragma clang fp contract(off)
    const float m = tanhf(x);
    const float sg = cont_sigmoid(y);
    const float s = cont_std(sg, lo, hi);
    const float z = (a - m) / s;
    *dx = glp * (z / s) * (1.0f - m * m);
    *dy = (glp * (z * z - 1.0f) / s + gen / s) * ((hi - lo) * (sg * (1.0f - sg)));
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cont_stats_vec_kernel(
    const void* means, const void* stds, mlearn_continuous_layout lay, int64_t total,
    const float* actions, float* logp, float* ent) {
    constexpr int V = Chunk<T>::V;
    const int A = lay.num_groups * lay.num_dims, D = lay.num_dims;
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    const int64_t nv = total / V;
    for (int64_t c = tid; c < nv; c += nthreads) {
        const int64_t i0 = c * V;
        float x[V], y[V], a[V], lp[V], en[V];
        Chunk<T>::load(means, i0, x);
        Chunk<T>::load(stds, i0, y);
        load_f32<V>(actions, i0, a);
        int e = (int)(i0 % A);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int g = e / D;
            stats_elem(x[j], y[j], a[j], lay.std_min[g], lay.std_max[g], &lp[j], &en[j]);
            e = e + 1 == A ? 0 : e + 1;
        }
        store_f32<V>(logp, i0, lp);
        store_f32<V>(ent, i0, en);
    }
    const int64_t i = nv * V + tid;  // the < V elements past the last whole chunk
    if (i < total) {
        const int g = (int)(i % A) / D;
        const int32_t dt = sizeof(T) == 4 ? MLEARN_DTYPE_F32 : MLEARN_DTYPE_BF16;
        stats_elem(cont_load(means, dt, i), cont_load(stds, dt, i), actions[i], lay.std_min[g],
                   lay.std_max[g], &logp[i], &ent[i]);
    }
}

__global__ __launch_bounds__(kThreads) void cont_stats_kernel(
    const void* means, int64_t ldm, const void* stds, int64_t lds_, int32_t dtype,
    mlearn_continuous_layout lay, int64_t total, const float* actions, float* logp, float* ent) {
    const int A = lay.num_groups * lay.num_dims, D = lay.num_dims;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += nthreads) {
        const int64_t r = i / A;
        const int e = (int)(i - r * A), g = e / D;
        stats_elem(cont_load(means, dtype, r * ldm + e), cont_load(stds, dtype, r * lds_ + e),
                   actions[i], lay.std_min[g], lay.std_max[g], &logp[i], &ent[i]);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void cont_stats_bwd_vec_kernel(
    const void* means, const void* stds, mlearn_continuous_layout lay, int64_t total,
    const float* actions, const float* g_lp, const float* g_en, void* d_means, void* d_stds) {
    constexpr int V = Chunk<T>::V;
    const int A = lay.num_groups * lay.num_dims, D = lay.num_dims;
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    const int64_t nv = total / V;
    for (int64_t c = tid; c < nv; c += nthreads) {
        const int64_t i0 = c * V;
        float x[V], y[V], a[V], gl[V], ge[V], dx[V], dy[V];
        Chunk<T>::load(means, i0, x);
        Chunk<T>::load(stds, i0, y);
        load_f32<V>(actions, i0, a);
#pragma unroll
        for (int j = 0; j < V; ++j) gl[j] = ge[j] = 0.f;
        if (g_lp) load_f32<V>(g_lp, i0, gl);
        if (g_en) load_f32<V>(g_en, i0, ge);
        int e = (int)(i0 % A);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int g = e / D;
            stats_bwd_elem(x[j], y[j], a[j], lay.std_min[g], lay.std_max[g], gl[j], ge[j], &dx[j],
                           &dy[j]);
            e = e + 1 == A ? 0 : e + 1;
        }
        Chunk<T>::store(d_means, i0, dx);
        Chunk<T>::store(d_stds, i0, dy);
    }
    const int64_t i = nv * V + tid;
    if (i < total) {
        const int g = (int)(i % A) / D;
        const int32_t dt = sizeof(T) == 4 ? MLEARN_DTYPE_F32 : MLEARN_DTYPE_BF16;
        float dx, dy;
        stats_bwd_elem(cont_load(means, dt, i), cont_load(stds, dt, i), actions[i], lay.std_min[g],
                       lay.std_max[g], g_lp ? g_lp[i] : 0.f, g_en ? g_en[i] : 0.f, &dx, &dy);
        cont_store(d_means, dt, i, dx);
        cont_store(d_stds, dt, i, dy);
    }
}

__global__ __launch_bounds__(kThreads) void cont_stats_bwd_kernel(
    const void* means, int64_t ldm, const void* stds, int64_t lds_, int32_t dtype,
    mlearn_continuous_layout lay, int64_t total, const float* actions, const float* g_lp,
    const float* g_en, void* d_means, int64_t ld_dm, void* d_stds, int64_t ld_ds) {
    const int A = lay.num_groups * lay.num_dims, D = lay.num_dims;
    const int64_t nthreads = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += nthreads) {
        const int64_t r = i / A;
        const int e = (int)(i - r * A), g = e / D;
        float dx, dy;
        stats_bwd_elem(cont_load(means, dtype, r * ldm + e), cont_load(stds, dtype, r * lds_ + e),
                       actions[i], lay.std_min[g], lay.std_max[g], g_lp ? g_lp[i] : 0.f,
                       g_en ? g_en[i] : 0.f, &dx, &dy);
        cont_store(d_means, dtype, r * ld_dm + e, dx);
        cont_store(d_stds, dtype, r * ld_ds + e, dy);
    }
}

// ---------------------------------------------------------------------------
// argument checks (before the device is touched) and launch shapes
// ---------------------------------------------------------------------------
int check_args(const char* what, int32_t dtype, const mlearn_continuous_layout& l, int64_t rows,
               int64_t ld_a, int64_t ld_b) {
    ML_REQUIRE(dtype == MLEARN_DTYPE_F32 || dtype == MLEARN_DTYPE_BF16,
               "%s: dtype %d is neither f32 nor bf16", what, dtype);
    ML_REQUIRE(l.num_groups >= 1 && l.num_groups <= MLEARN_MAX_GROUPS,
               "%s: num_groups %d outside 1..%d", what, l.num_groups, MLEARN_MAX_GROUPS);
    ML_REQUIRE(l.num_dims >= 1 && l.num_dims <= 1024, "%s: num_dims %d outside 1..1024", what,
               l.num_dims);
    const int A = l.num_groups * l.num_dims;
    ML_REQUIRE(A <= 1024, "%s: %d x %d action columns exceed 1024", what, l.num_groups,
               l.num_dims);
    for (int g = 0; g < l.num_groups; ++g)
        ML_REQUIRE(l.std_min[g] > 0.f && l.std_min[g] <= l.std_max[g] && l.std_max[g] < INFINITY,
                   "%s: group %d needs 0 < std_min <= std_max (got %g, %g)", what, g,
                   (double)l.std_min[g], (double)l.std_max[g]);
    ML_REQUIRE(rows >= 0 && rows <= ((int64_t)1 << 40), "%s: bad row count", what);
    ML_REQUIRE(ld_a >= A && ld_b >= A, "%s: row stride below the %d action columns", what, A);
    return MLEARN_OK;
}

inline bool aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

// grid of a grid-stride kernel over `work` lane-trips: every CU gets up to
// 8 workgroups of 256 (2 waves per SIMD per workgroup), never more than the work
unsigned stride_grid(int64_t work) {
    int cus = device_cus();
    if (cus <= 0) cus = 256;
    const int64_t blocks = (work + kThreads - 1) / kThreads;
    const int64_t cap = (int64_t)cus * 8;
    return (unsigned)(blocks < cap ? (blocks < 1 ? 1 : blocks) : cap);
}

}  // namespace
}  // namespace ml

extern "C" {

int mlearn_continuous_sample_host(const void* means, int64_t ld_means, const void* stds,
                                  int64_t ld_stds, int32_t dtype,
                                  mlearn_continuous_layout layout, int64_t N, uint32_t k0,
                                  uint32_t k1, const uint64_t* step_ctr, uint64_t step,
                                  uint32_t env_offset, int32_t sample, float* actions_f32,
                                  float* log_probs_f32) {
    using namespace ml;
    if (int rc = check_args("continuous_sample_host", dtype, layout, N, ld_means, ld_stds))
        return rc;
    if (N == 0) return MLEARN_OK;
    ML_REQUIRE(means && stds && actions_f32, "continuous_sample_host: null pointer");
    const int A = layout.num_groups * layout.num_dims, nb = (A + 3) / 4;
    const uint64_t st = (step_ctr ? *step_ctr : 0ull) + step;
    for (int64_t n = 0; n < N; ++n)
        for (int b = 0; b < nb; ++b) {
            const int e0 = 4 * b, cnt = A - e0 < 4 ? A - e0 : 4;
            float x[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f};
            float z[4] = {0.f, 0.f, 0.f, 0.f}, a[4], lp[4];
            for (int j = 0; j < cnt; ++j) {
                x[j] = cont_load(means, dtype, n * ld_means + e0 + j);
                y[j] = cont_load(stds, dtype, n * ld_stds + e0 + j);
            }
            if (sample) cont_normals4(k0, k1, env_offset + (uint32_t)n, st, (uint32_t)b, z);
            cont_sample4(x, y, z, layout, e0, cnt, sample, log_probs_f32 != nullptr, a, lp);
            for (int j = 0; j < cnt; ++j) {
                actions_f32[n * A + e0 + j] = a[j];
                if (log_probs_f32) log_probs_f32[n * A + e0 + j] = lp[j];
            }
        }
    return MLEARN_OK;
}

int mlearn_continuous_sample(const void* means, int64_t ld_means, const void* stds,
                             int64_t ld_stds, int32_t dtype, mlearn_continuous_layout layout,
                             int64_t N, uint32_t k0, uint32_t k1, const uint64_t* step_ctr,
                             uint64_t step, uint32_t env_offset, int32_t sample,
                             float* actions_f32, float* log_probs_f32, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("continuous_sample", dtype, layout, N, ld_means, ld_stds)) return rc;
    if (N == 0) return MLEARN_OK;
    ML_REQUIRE(means && stds && actions_f32, "continuous_sample: null pointer");
    const int A = layout.num_groups * layout.num_dims, nb = (A + 3) / 4;
    const size_t quad = dtype == MLEARN_DTYPE_F32 ? 16 : 8;  // bytes of 4 inputs
    const int vout = A % 4 == 0 && aligned(actions_f32, 16) &&
                     (!log_probs_f32 || aligned(log_probs_f32, 16));
    const int vin = A % 4 == 0 && ld_means % 4 == 0 && ld_stds % 4 == 0 && aligned(means, quad) &&
                    aligned(stds, quad);
    const int64_t blocks = (N * nb + kThreads - 1) / kThreads;
    ML_REQUIRE(blocks <= 0x7fffffff, "continuous_sample: N too large");
    (void)hipGetLastError();
    hipLaunchKernelGGL(cont_sample_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, S(stream),
                       means, ld_means, stds, ld_stds, dtype, layout, N, nb, vin, vout, k0, k1,
                       step_ctr, step, env_offset, sample, actions_f32, log_probs_f32);
    return check_launch("continuous_sample");
}

int mlearn_continuous_stats(const void* means, int64_t ld_means, const void* stds,
                            int64_t ld_stds, int32_t dtype, mlearn_continuous_layout layout,
                            int64_t R, const float* actions, float* log_probs, float* entropies,
                            mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("continuous_stats", dtype, layout, R, ld_means, ld_stds)) return rc;
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(means && stds && actions && log_probs && entropies,
               "continuous_stats: null pointer");
    const int A = layout.num_groups * layout.num_dims;
    const int64_t total = R * A;
    const bool vec = ld_means == A && ld_stds == A && aligned(means, 16) && aligned(stds, 16) &&
                     aligned(actions, 16) && aligned(log_probs, 16) && aligned(entropies, 16);
    (void)hipGetLastError();
    if (vec && dtype == MLEARN_DTYPE_F32) {
        hipLaunchKernelGGL(cont_stats_vec_kernel<float>, dim3(stride_grid(total / 4 + 4)),
                           dim3(kThreads), 0, S(stream), means, stds, layout, total, actions,
                           log_probs, entropies);
    } else if (vec) {
        hipLaunchKernelGGL(cont_stats_vec_kernel<uint16_t>, dim3(stride_grid(total / 8 + 8)),
                           dim3(kThreads), 0, S(stream), means, stds, layout, total, actions,
                           log_probs, entropies);
    } else {
        hipLaunchKernelGGL(cont_stats_kernel, dim3(stride_grid(total)), dim3(kThreads), 0,
                           S(stream), means, ld_means, stds, ld_stds, dtype, layout, total,
                           actions, log_probs, entropies);
    }
    return check_launch("continuous_stats");
}

int mlearn_continuous_stats_bwd(const void* means, int64_t ld_means, const void* stds,
                                int64_t ld_stds, int32_t dtype, mlearn_continuous_layout layout,
                                int64_t R, const float* actions, const float* g_log_probs,
                                const float* g_entropies, void* d_means, int64_t ld_dm,
                                void* d_stds, int64_t ld_ds, mlearn_stream_t stream) {
    using namespace ml;
    if (int rc = check_args("continuous_stats_bwd", dtype, layout, R, ld_means, ld_stds))
        return rc;
    const int A = layout.num_groups * layout.num_dims;
    ML_REQUIRE(ld_dm >= A && ld_ds >= A,
               "continuous_stats_bwd: gradient row stride below the %d action columns", A);
    if (R == 0) return MLEARN_OK;
    ML_REQUIRE(means && stds && actions && d_means && d_stds,
               "continuous_stats_bwd: null pointer");
    const int64_t total = R * A;
    const bool vec = ld_means == A && ld_stds == A && ld_dm == A && ld_ds == A &&
                     aligned(means, 16) && aligned(stds, 16) && aligned(actions, 16) &&
                     aligned(d_means, 16) && aligned(d_stds, 16) &&
                     (!g_log_probs || aligned(g_log_probs, 16)) &&
                     (!g_entropies || aligned(g_entropies, 16));
    (void)hipGetLastError();
    if (vec && dtype == MLEARN_DTYPE_F32) {
        hipLaunchKernelGGL(cont_stats_bwd_vec_kernel<float>, dim3(stride_grid(total / 4 + 4)),
                           dim3(kThreads), 0, S(stream), means, stds, layout, total, actions,
                           g_log_probs, g_entropies, d_means, d_stds);
    } else if (vec) {
        hipLaunchKernelGGL(cont_stats_bwd_vec_kernel<uint16_t>, dim3(stride_grid(total / 8 + 8)),
                           dim3(kThreads), 0, S(stream), means, stds, layout, total, actions,
                           g_log_probs, g_entropies, d_means, d_stds);
    } else {
        hipLaunchKernelGGL(cont_stats_bwd_kernel, dim3(stride_grid(total)), dim3(kThreads), 0,
                           S(stream), means, ld_means, stds, ld_stds, dtype, layout, total,
                           actions, g_log_probs, g_entropies, d_means, ld_dm, d_stds, ld_ds);
    }
    return check_launch("continuous_stats_bwd");
}

}  // extern "C"
