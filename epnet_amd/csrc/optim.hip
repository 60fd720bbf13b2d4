// optim.hip -- the adam_onecycle optimiser step as a multi-tensor apply (include/epnet_ops.h, epnet_adam_onecycle_step) for
// gfx950: gradient clipping by the global norm, true weight decay, Adam and the one-cycle schedule in three launches, nothing
// read back, every scalar that changes from step to step read from device memory (so a captured graph replays the step).
//
// Parameters and gradients stay where they are: a tensor table names them, a chunk table deals fixed-size pieces of them to the
// workgroups. kChunk = 4096 elements per workgroup of 256 lanes: in the full-chunk path a lane holds 4 x 16 bytes of each of p,
// g, m, v -- 16 loads in flight per lane, 64 KiB per workgroup, twice the ~32 KiB per CU at which the chip streams -- and a
// 15.7 M-parameter model in 240 tensors is 3996 workgroups, 15 per CU.
//
// epnet_adam_onecycle_step_scaled is the same three launches with dynamic loss scaling: the kernels' bodies are templates on
// kScaled, the unscaled instantiations are the kernels above with nothing added, the scaled ones unscale every gradient as
// they read it (g * inv, rounded to fp32), and the finish kernel -- whose float64 sum of squares is finite exactly when every
// unscaled gradient is -- decides whether the step is applied, moves the scale and hands inv and the skip flag to the update
// kernel in ScalX.
#include "common.h"

namespace epnet {
namespace optim {

constexpr int kThreads = 256;
constexpr int kChunk = EPNET_OPTIM_CHUNK;
constexpr int kGroups = kChunk / (kThreads * 4);  // 16-byte groups per lane and array
constexpr int kScalBytes = 64;                    // the step's scalars at the head of the workspace
static_assert(kGroups * kThreads * 4 == kChunk, "chunk = whole 16-byte groups per lane");

typedef float f4 __attribute__((ext_vector_type(4)));

// what the finish kernel leaves for the update kernel
struct Scal {
    float coef, decay, b1, omb1, step_size, bc2_sqrt, lr, mom;
};
static_assert(sizeof(Scal) <= kScalBytes, "scalars fit their slot");

// the scaled step's: inv is what this step's gradients are multiplied by (the scale itself has moved on by the time the update
// kernel runs), skip != 0 when the step is not applied
struct ScalX {
    Scal s;
    float inv;
    int skip;
};
static_assert(sizeof(ScalX) <= kScalBytes, "scalars fit their slot");

// 1 / scale as every kernel of the scaled step computes it
__device__ __forceinline__ float inverse_scale(const float *scale) { return (float)(1.0 / (double)scale[0]); }

struct Chunk {
    float *p, *g, *m, *v;
    int count;
};

__device__ __forceinline__ Chunk chunk_of(const epnet_optim_tensor *tensors, const int *chunks, float *exp_avg, float *exp_avg_sq) {
    const int t = chunks[2 * blockIdx.x], first = chunks[2 * blockIdx.x + 1];
    const epnet_optim_tensor T = tensors[t];
    Chunk c;
    const long long left = T.numel - first;
    c.count = left < kChunk ? (int)left : kChunk;
    c.p = T.param + first;
    c.g = T.grad ? T.grad + first : nullptr;
    c.m = exp_avg + T.state_offset + first;
    c.v = exp_avg_sq + T.state_offset + first;
    return c;
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// Sum of squares of one chunk's gradient, in double. Element e of the chunk belongs to lane (e / 4) % 256, and a lane adds its
// elements in ascending order, whether the gradient's address allows 16-byte loads or not: the partial is the same bits for a
// gradient that is a tensor of its own and for one that is a view at an odd offset of a bucket. kScaled: of g * inv, rounded to fp32.
template <bool kScaled>
__device__ __forceinline__ void norm_body(const epnet_optim_tensor *__restrict__ tensors, const int *__restrict__ chunks,
                                          double *__restrict__ partial, const float *__restrict__ scale) {
    __shared__ double wave_sum[kThreads / kWave];
    const int t = chunks[2 * blockIdx.x], first = chunks[2 * blockIdx.x + 1];
    const float *g = tensors[t].grad;
    const long long left = tensors[t].numel - first;
    const int count = left < kChunk ? (int)left : kChunk;
    double acc = 0.0;
    float inv = 1.f;
    if constexpr (kScaled) inv = inverse_scale(scale);
    if (g) {
        g += first;
        if (count == kChunk && aligned16(g)) {
            f4 x[kGroups];
#pragma unroll
            for (int k = 0; k < kGroups; ++k) x[k] = reinterpret_cast<const f4 *>(g)[k * kThreads + threadIdx.x];
#pragma unroll
            for (int k = 0; k < kGroups; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float gu = x[k][j];
                    if constexpr (kScaled) gu = gu * inv;
                    acc += (double)gu * (double)gu;
                }
        } else {
            for (int k = 0; k < kGroups; ++k)
                for (int j = 0; j < 4; ++j) {
                    const int e = (k * kThreads + (int)threadIdx.x) * 4 + j;
                    if (e < count) {
                        float gu = g[e];
                        if constexpr (kScaled) gu = gu * inv;
                        acc += (double)gu * (double)gu;
                    }
                }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane_id() == 0) wave_sum[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < kThreads / kWave; ++w) s += wave_sum[w];
        partial[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kThreads) void norm_kernel(const epnet_optim_tensor *__restrict__ tensors, const int *__restrict__ chunks,
                                                        double *__restrict__ partial) {
    norm_body<false>(tensors, chunks, partial, nullptr);
}

__global__ __launch_bounds__(kThreads) void norm_scaled_kernel(const epnet_optim_tensor *__restrict__ tensors,
                                                               const int *__restrict__ chunks, double *__restrict__ partial,
                                                               const float *__restrict__ scale) {
    norm_body<true>(tensors, chunks, partial, scale);
}

// the scaled step's arguments that do not change from step to step
struct ScaleRule {
    double growth_factor, backoff_factor;
    long long growth_interval;
    float min_scale;
};

// One workgroup: the partials in a fixed order (lane i takes i, i + 256, ...; then a tree), the step's row, the scalars, stats,
// and the counter moves on. kScaled: a sum that is not finite skips the step -- the counter stays, coef is reported as 0 --, and
// the scale moves by torch._amp_update_scale_'s rule AFTER its value was taken for this step.
template <bool kScaled>
__device__ __forceinline__ void finish_body(long long nchunks, const double *__restrict__ partial, const float *__restrict__ rows,
                                            long long total_steps, double clip, long long *__restrict__ counter,
                                            void *__restrict__ scal_slot, double *__restrict__ stats, float *__restrict__ scale,
                                            long long *__restrict__ scaler_state, const ScaleRule &rule) {
    __shared__ double red[kThreads];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < nchunks; i += kThreads) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total_norm = sqrt(red[0]);
        const double c = clip / (total_norm + 1e-6);
        const float coef = (float)(c < 1.0 ? c : 1.0);  // a NaN norm gives coef 1 and NaN gradients, as the reference's clamp
        const long long t = counter[0];
        const long long used = t < total_steps ? (t < 0 ? 0 : t) : total_steps - 1;
        const float *r = rows + used * EPNET_OPTIM_ROW;
        Scal s;
        s.coef = coef; s.decay = r[0]; s.b1 = r[1]; s.omb1 = r[2]; s.step_size = r[3]; s.bc2_sqrt = r[4]; s.lr = r[5]; s.mom = r[6];
        if constexpr (!kScaled) {
            *(Scal *)scal_slot = s;
            stats[0] = total_norm; stats[1] = (double)coef; stats[2] = (double)s.lr; stats[3] = (double)s.mom;
            stats[4] = (double)used; stats[5] = t >= total_steps ? 1.0 : 0.0; stats[6] = 0.0; stats[7] = 0.0;
            counter[0] = t + 1;
        } else {
            const bool skip = !isfinite(red[0]);
            const float used_scale = scale[0];
            ScalX x;
            x.s = s; x.inv = inverse_scale(scale); x.skip = skip ? 1 : 0;
            *(ScalX *)scal_slot = x;
            long long tracker = scaler_state[0], skipped = scaler_state[1];
            float next = used_scale;
            if (skip) {
                next = (float)((double)used_scale * rule.backoff_factor);
                if (next < rule.min_scale) next = rule.min_scale;
                tracker = 0;
                skipped += 1;
            } else {
                tracker += 1;
                if (tracker == rule.growth_interval) {
                    const float grown = (float)((double)used_scale * rule.growth_factor);
                    if (isfinite(grown)) next = grown;
                    tracker = 0;
                }
            }
            if (rule.growth_interval > 0) scale[0] = next;  // 0: a static scale
            scaler_state[0] = tracker; scaler_state[1] = skipped;
            stats[0] = total_norm; stats[1] = skip ? 0.0 : (double)coef; stats[2] = (double)s.lr; stats[3] = (double)s.mom;
            stats[4] = (double)used; stats[5] = t >= total_steps ? 1.0 : 0.0; stats[6] = (double)used_scale; stats[7] = (double)skipped;
            if (!skip) counter[0] = t + 1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(long long nchunks, const double *__restrict__ partial,
                                                          const float *__restrict__ rows, long long total_steps, double clip,
                                                          long long *__restrict__ counter, Scal *__restrict__ scal,
                                                          double *__restrict__ stats) {
    finish_body<false>(nchunks, partial, rows, total_steps, clip, counter, scal, stats, nullptr, nullptr, ScaleRule{});
}

__global__ __launch_bounds__(kThreads) void finish_scaled_kernel(long long nchunks, const double *__restrict__ partial,
                                                                 const float *__restrict__ rows, long long total_steps, double clip,
                                                                 long long *__restrict__ counter, ScalX *__restrict__ scal,
                                                                 double *__restrict__ stats, float *__restrict__ scale,
                                                                 long long *__restrict__ scaler_state, ScaleRule rule) {
    finish_body<true>(nchunks, partial, rows, total_steps, clip, counter, scal, stats, scale, scaler_state, rule);
}

// the update of one element, fp32 in source order (no contraction; / and sqrt correctly rounded)
__device__ __forceinline__ void adam(float &p, float g, float &m, float &v, const Scal &s, float b2, float omb2, float eps) {
    const float gc = g * s.coef;
    p = p * s.decay;
    m = m * s.b1 + s.omb1 * gc;
    v = v * b2 + omb2 * gc * gc;
    p = p - s.step_size * (m / (sqrtf(v) / s.bc2_sqrt + eps));
}

// kScaled: the slot holds a ScalX; a skipped step touches nothing but the gradients (zeroed when zero_grads is set), an applied one
// is the unscaled step on g * inv
template <bool kScaled>
__device__ __forceinline__ void update_body(const epnet_optim_tensor *__restrict__ tensors, const int *__restrict__ chunks,
                                            float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                            const void *__restrict__ scal_slot, float b2, float omb2, float eps, int zero_grads) {
    const Chunk c = chunk_of(tensors, chunks, exp_avg, exp_avg_sq);
    const Scal s = *(const Scal *)scal_slot;
    float inv = 1.f;
    if constexpr (kScaled) {
        const ScalX *x = (const ScalX *)scal_slot;
        inv = x->inv;
        if (x->skip) {
            if (zero_grads && c.g) {
                if (c.count == kChunk && aligned16(c.g)) {
#pragma unroll
                    for (int k = 0; k < kGroups; ++k) reinterpret_cast<f4 *>(c.g)[k * kThreads + threadIdx.x] = f4{0.f, 0.f, 0.f, 0.f};
                } else {
                    for (int e = threadIdx.x; e < c.count; e += kThreads) c.g[e] = 0.f;
                }
            }
            return;
        }
    }
    const bool full = c.count == kChunk && aligned16(c.p);
    if (!c.g) {  // no gradient: the decay loop runs, Adam skips the tensor
        if (full) {
            f4 p[kGroups];
#pragma unroll
            for (int k = 0; k < kGroups; ++k) p[k] = reinterpret_cast<const f4 *>(c.p)[k * kThreads + threadIdx.x];
#pragma unroll
            for (int k = 0; k < kGroups; ++k) reinterpret_cast<f4 *>(c.p)[k * kThreads + threadIdx.x] = p[k] * s.decay;
        } else {
            for (int e = threadIdx.x; e < c.count; e += kThreads) c.p[e] = c.p[e] * s.decay;
        }
        return;
    }
    if (full && aligned16(c.m) && aligned16(c.v)) {
        // p, m and v in 16-byte pieces; so is g where its address allows. A gradient that is a view at an odd offset of a bucket is
        // read (and zeroed) as the same four elements in four dword accesses, which keeps the other 28 of the 32 bytes per element wide
        const bool gvec = aligned16(c.g);
        f4 p[kGroups], g[kGroups], m[kGroups], v[kGroups];
#pragma unroll
        for (int k = 0; k < kGroups; ++k) {
            const int q = k * kThreads + threadIdx.x;
            p[k] = reinterpret_cast<const f4 *>(c.p)[q];
            m[k] = reinterpret_cast<const f4 *>(c.m)[q];
            v[k] = reinterpret_cast<const f4 *>(c.v)[q];
        }
        if (gvec) {
#pragma unroll
            for (int k = 0; k < kGroups; ++k) g[k] = reinterpret_cast<const f4 *>(c.g)[k * kThreads + threadIdx.x];
        } else {
#pragma unroll
            for (int k = 0; k < kGroups; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) g[k][j] = c.g[(k * kThreads + threadIdx.x) * 4 + j];
        }
#pragma unroll
        for (int k = 0; k < kGroups; ++k) {
            const int q = k * kThreads + threadIdx.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pe = p[k][j], me = m[k][j], ve = v[k][j];
                adam(pe, kScaled ? g[k][j] * inv : g[k][j], me, ve, s, b2, omb2, eps);
                p[k][j] = pe; m[k][j] = me; v[k][j] = ve;
            }
            reinterpret_cast<f4 *>(c.p)[q] = p[k];
            reinterpret_cast<f4 *>(c.m)[q] = m[k];
            reinterpret_cast<f4 *>(c.v)[q] = v[k];
            if (zero_grads) {
                if (gvec) {
                    reinterpret_cast<f4 *>(c.g)[q] = f4{0.f, 0.f, 0.f, 0.f};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) c.g[q * 4 + j] = 0.f;
                }
            }
        }
        return;
    }
    // a short chunk (a small tensor, a tensor's tail) or a parameter / state address that is no multiple of 16: one element per
    // lane and pass
    for (int e = threadIdx.x; e < c.count; e += kThreads) {
        float pe = c.p[e], me = c.m[e], ve = c.v[e];
        adam(pe, kScaled ? c.g[e] * inv : c.g[e], me, ve, s, b2, omb2, eps);
        c.p[e] = pe; c.m[e] = me; c.v[e] = ve;
        if (zero_grads) c.g[e] = 0.f;
    }
}

__global__ __launch_bounds__(kThreads) void update_kernel(const epnet_optim_tensor *__restrict__ tensors, const int *__restrict__ chunks,
                                                          float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                          const Scal *__restrict__ scal, float b2, float omb2, float eps,
                                                          int zero_grads) {
    update_body<false>(tensors, chunks, exp_avg, exp_avg_sq, scal, b2, omb2, eps, zero_grads);
}

__global__ __launch_bounds__(kThreads) void update_scaled_kernel(const epnet_optim_tensor *__restrict__ tensors,
                                                                 const int *__restrict__ chunks, float *__restrict__ exp_avg,
                                                                 float *__restrict__ exp_avg_sq, const ScalX *__restrict__ scal, float b2,
                                                                 float omb2, float eps, int zero_grads) {
    update_body<true>(tensors, chunks, exp_avg, exp_avg_sq, scal, b2, omb2, eps, zero_grads);
}

inline size_t workspace_bytes(long long chunks) { return (size_t)kScalBytes + (size_t)chunks * sizeof(double); }

}  // namespace optim
}  // namespace epnet

using namespace epnet;

extern "C" size_t epnet_adam_onecycle_workspace_bytes(long long chunks) {
    if (chunks <= 0 || chunks > 0x7fffffffll) return 0;
    return optim::workspace_bytes(chunks);
}

// the checks both entry points share; EPNET_OK with *empty set when there is nothing to do
static int check_step_args(int tensors, long long chunks, long long max_numel, const epnet_optim_tensor *tensor_table,
                           const int *chunk_table, const float *rows, long long total_steps, double clip, double eps, double b2,
                           long long *counter, float *exp_avg, float *exp_avg_sq, double *stats, void *workspace,
                           size_t workspace_bytes, bool *empty) {
    *empty = false;
    EPNET_REQUIRE(tensors >= 0 && chunks >= 0 && max_numel >= 0 && total_steps >= 1);
    EPNET_REQUIRE(clip > 0 && eps >= 0 && b2 >= 0 && b2 < 1);  // !(clip > 0) also refuses NaN
    if (tensors == 0 || chunks == 0) {
        *empty = true;
        return EPNET_OK;
    }
    EPNET_REQUIRE(tensor_table && chunk_table && rows && counter && exp_avg && exp_avg_sq && stats);
    if (max_numel > 0x7fffffffll || chunks > 0x7fffffffll) return EPNET_ELIMIT;
    if (!workspace || workspace_bytes < optim::workspace_bytes(chunks)) return EPNET_ENOMEM;
    EPNET_REQUIRE(((uintptr_t)workspace & 15) == 0);
    return EPNET_OK;
}

extern "C" int epnet_adam_onecycle_step(int tensors, long long chunks, long long max_numel, const epnet_optim_tensor *tensor_table,
                                        const int *chunk_table, const float *rows, long long total_steps, double clip, double eps,
                                        double b2, int zero_grads, long long *counter, float *exp_avg, float *exp_avg_sq,
                                        double *stats, void *workspace, size_t workspace_bytes, epnet_stream_t stream) {
    bool empty;
    const int rc = check_step_args(tensors, chunks, max_numel, tensor_table, chunk_table, rows, total_steps, clip, eps, b2, counter,
                                   exp_avg, exp_avg_sq, stats, workspace, workspace_bytes, &empty);
    if (rc != EPNET_OK || empty) return rc;
    optim::Scal *scal = (optim::Scal *)workspace;
    double *partial = (double *)((char *)workspace + optim::kScalBytes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(optim::norm_kernel, dim3((unsigned)chunks), dim3(optim::kThreads), 0, st, tensor_table, chunk_table, partial);
    hipLaunchKernelGGL(optim::finish_kernel, dim3(1), dim3(optim::kThreads), 0, st, chunks, (const double *)partial, rows, total_steps,
                       clip, counter, scal, stats);
    hipLaunchKernelGGL(optim::update_kernel, dim3((unsigned)chunks), dim3(optim::kThreads), 0, st, tensor_table, chunk_table, exp_avg,
                       exp_avg_sq, (const optim::Scal *)scal, (float)b2, (float)(1.0 - b2), (float)eps, zero_grads ? 1 : 0);
    return check_launch("adam_onecycle_step");
}

extern "C" int epnet_adam_onecycle_step_scaled(int tensors, long long chunks, long long max_numel,
                                               const epnet_optim_tensor *tensor_table, const int *chunk_table, const float *rows,
                                               long long total_steps, double clip, double eps, double b2, int zero_grads,
                                               long long *counter, float *exp_avg, float *exp_avg_sq, double *stats, float *scale,
                                               long long *scaler_state, double growth_factor, double backoff_factor,
                                               long long growth_interval, double min_scale, void *workspace, size_t workspace_bytes,
                                               epnet_stream_t stream) {
    // written so that a NaN fails every one of them
    EPNET_REQUIRE(growth_factor >= 1 && growth_factor <= 3.0e38 && backoff_factor > 0 && backoff_factor <= 1 && growth_interval >= 0);
    EPNET_REQUIRE(min_scale > 0 && min_scale <= 3.0e38 && (float)min_scale > 0);
    bool empty;
    const int rc = check_step_args(tensors, chunks, max_numel, tensor_table, chunk_table, rows, total_steps, clip, eps, b2, counter,
                                   exp_avg, exp_avg_sq, stats, workspace, workspace_bytes, &empty);
    if (rc != EPNET_OK || empty) return rc;
    EPNET_REQUIRE(scale && scaler_state);
    optim::ScalX *scal = (optim::ScalX *)workspace;
    double *partial = (double *)((char *)workspace + optim::kScalBytes);
    optim::ScaleRule rule;
    rule.growth_factor = growth_factor; rule.backoff_factor = backoff_factor; rule.growth_interval = growth_interval;
    rule.min_scale = (float)min_scale;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(optim::norm_scaled_kernel, dim3((unsigned)chunks), dim3(optim::kThreads), 0, st, tensor_table, chunk_table, partial,
                       (const float *)scale);
    hipLaunchKernelGGL(optim::finish_scaled_kernel, dim3(1), dim3(optim::kThreads), 0, st, chunks, (const double *)partial, rows,
                       total_steps, clip, counter, scal, stats, scale, scaler_state, rule);
    hipLaunchKernelGGL(optim::update_scaled_kernel, dim3((unsigned)chunks), dim3(optim::kThreads), 0, st, tensor_table, chunk_table,
                       exp_avg, exp_avg_sq, (const optim::ScalX *)scal, (float)b2, (float)(1.0 - b2), (float)eps, zero_grads ? 1 : 0);
    return check_launch("adam_onecycle_step_scaled");
}
