// What stands around the Adam step of misc.hip in a training loop: the global gradient norm, global-norm clipping, weight decay
// (coupled L2 or decoupled AdamW) and a guard that skips a step whose gradient is not finite - all on the device, beside the plain
// step (adam_flat_kernel is untouched; FlatAdam at its defaults still launches it alone).
//
//   grad_norm_partial_kernel   workgroup w squares and sums the chunk [w*GN_CHUNK, min((w+1)*GN_CHUNK, n)) of the flat gradient
//                              buffer in fp64 and writes ONE fp64 partial (a plain vector store)
//   grad_norm_finish_kernel    ONE workgroup sums the partials in a fixed order and writes the clip record
//   adam_clipped_kernel        reads scale / nonfinite from the record on the device; g' = g * scale (+ wd * p), p *= 1 - lr wd, then
//                              adam_update - the expression of the plain step (common.h)
//
// The launch boundary is the only synchronisation between them: no floating-point atomics, no ticket, no cooperative launch, no
// wait across workgroups.  The number of partials is a function of n alone, and every sum runs in a fixed order (per thread in
// ascending element order, wave butterfly 32..1, (w0 + w1) + (w2 + w3)), so the same gradients give the same record bits on every
// call and on every device.  An fp32 square is exact in fp64, so only the fp64 additions round: the norm is good to the final
// rounding to fp32 (torch.nn.utils.clip_grad_norm_ sums in fp32: ~200 fp32 eps off at a million elements).
#include <math.h>
#include "common.h"
#include "kernels.h"

namespace s2vt {

constexpr int GN_BLOCK = 256;
constexpr int GN_ITERS = GN_CHUNK / (4 * GN_BLOCK);      // f32x4 loads per thread of a full chunk
static_assert(GN_CHUNK % 1024 == 0 && GN_CHUNK % (4 * GN_BLOCK) == 0, "a chunk is whole f32x4 rounds of the workgroup");

// fixed-order sum over the 256 threads of a workgroup (every thread returns it); lds: 4 doubles
__device__ __forceinline__ double block_sum_f64(double acc, double* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);     // (IEEE addition commutes: all 64 lanes hold the same bits)
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// Thread t owns elements 4 (k * 256 + t) .. + 3 of its workgroup's chunk in round k, whichever path loads them: the 16-byte
// path (g 16-byte aligned; GN_CHUNK is a multiple of 4, so every chunk is aligned with it) and the scalar path (any fp32
// pointer, and the ragged end of the last chunk) add the same squares in the same order.
__global__ __launch_bounds__(GN_BLOCK) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n, int aligned,
                                                                     double* __restrict__ partial) {
    __shared__ double lds[4];
    const int64_t base = (int64_t)blockIdx.x * GN_CHUNK;
    const int64_t left = n - base;
    const int len = left < GN_CHUNK ? (int)left : GN_CHUNK;
    const float* gc = g + base;
    double acc = 0.0;
    auto add4 = [&](const f32x4& x) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)x[j] * (double)x[j];
    };
    if (len == GN_CHUNK && aligned) {           // the streaming path: GN_ITERS independent 16-byte loads, no branch between them
        f32x4 x[GN_ITERS];
#pragma unroll
        for (int k = 0; k < GN_ITERS; ++k) x[k] = reinterpret_cast<const f32x4*>(gc)[k * GN_BLOCK + threadIdx.x];
#pragma unroll
        for (int k = 0; k < GN_ITERS; ++k) add4(x[k]);
    } else {
        for (int k = 0; k < GN_ITERS; ++k) {
            const int e = 4 * (k * GN_BLOCK + (int)threadIdx.x);
            if (e + 4 <= len) {
                f32x4 x;
                if (aligned) {
                    x = *reinterpret_cast<const f32x4*>(gc + e);
                } else {
                    x[0] = gc[e], x[1] = gc[e + 1], x[2] = gc[e + 2], x[3] = gc[e + 3];
                }
                add4(x);
            } else {
                for (int j = e; j < len; ++j) acc += (double)gc[j] * (double)gc[j];      // at most 3 elements, one thread
            }
        }
    }
    const double total = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(GN_BLOCK) void grad_norm_finish_kernel(const double* __restrict__ partial, int64_t n_partial, float max_norm,
                                                                    int skip_nonfinite, ClipRecord* __restrict__ rec) {
    __shared__ double lds[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n_partial; i += GN_BLOCK) acc += partial[i];
    const double total = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        float scale = 1.0f;
        if (max_norm > 0.f) {                   // clip_grad_norm_'s rule in fp32; a NaN coefficient stays NaN, as torch.clamp leaves it
            const float coef = max_norm / (norm + 1e-6f);
            scale = coef >= 1.0f ? 1.0f : coef;
        }
        const int bad = isfinite(norm) ? 0 : 1;
        rec->grad_norm = norm;
        rec->scale = scale;
        rec->nonfinite = bad;
        rec->pad = 0;
        if (skip_nonfinite) rec->skipped_total += bad;
    }
}

size_t grad_norm_workspace_bytes(int64_t n) { return n <= 0 ? 0 : (size_t)((n + GN_CHUNK - 1) / GN_CHUNK) * sizeof(double); }

int grad_norm(hipStream_t s, const float* g, int64_t n, double max_norm, int skip_nonfinite, void* workspace, size_t workspace_bytes,
              ClipRecord* rec) {
    S2VT_REQUIRE(n > 0, "grad_norm: n must be positive");
    S2VT_REQUIRE(g && (reinterpret_cast<uintptr_t>(g) & 3) == 0, "grad_norm: null / unaligned gradient buffer");
    S2VT_REQUIRE(rec && (reinterpret_cast<uintptr_t>(rec) & 15) == 0, "grad_norm: null / unaligned record (16 bytes)");
    S2VT_REQUIRE(!(max_norm != max_norm) && !(max_norm < 0 && isinf(max_norm)), "grad_norm: max_norm is NaN or -inf");
    const int64_t np = (n + GN_CHUNK - 1) / GN_CHUNK;
    S2VT_REQUIRE(np <= 0x7fffffff, "grad_norm: n too large");
    S2VT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= grad_norm_workspace_bytes(n),
                 "grad_norm: null / unaligned workspace or workspace too small (%zu < %zu bytes)", workspace_bytes,
                 grad_norm_workspace_bytes(n));
    double* partial = static_cast<double*>(workspace);
    const int aligned = (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)np), dim3(GN_BLOCK), 0, s, g, n, aligned, partial);
    S2VT_LAUNCH_CHECK("grad_norm_partial_kernel");
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(GN_BLOCK), 0, s, partial, np, max_norm > 0 ? (float)max_norm : 0.f,
                       skip_nonfinite ? 1 : 0, rec);
    S2VT_LAUNCH_CHECK("grad_norm_finish_kernel");
    return 0;
}

// ---- the clipped step
// Segment ends in the launch arguments (ascending, the last one n, unused ones n) and one decay bit per segment.  Every index is a
// compile-time constant after unrolling, so the table stays in scalar registers.
struct AdamSegs {
    int64_t end[ADAM_MAX_SEGS];
    uint32_t decay_mask;       // bit k: segment k is decayed; 0: no decay anywhere
    uint32_t all_mask;         // the value of decay_mask at which every segment is decayed
};

__device__ __forceinline__ int seg_of(const AdamSegs& sg, int64_t e) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < ADAM_MAX_SEGS; ++k) s += e >= sg.end[k] ? 1 : 0;
    return s;
}
// the two products that precede adam_update are rounded on their own (the definition forms g * scale and wd * p in fp32):
// never contracted into the additions that follow
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__global__ __launch_bounds__(256) void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int64_t n4, int64_t n, float w1, float beta2, float w2,
                                                           float step_size, float bc2_sqrt, float eps, float wd, float decay_f,
                                                           int decoupled, AdamSegs sg, int skip_nonfinite, const ClipRecord* __restrict__ rec) {
    float scale = 1.0f;
    if (rec) {
        if (skip_nonfinite && rec->nonfinite != 0) return;      // every thread, before touching p, m, v
        scale = rec->scale;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    auto upd = [&](float& pp, float gg, float& mm, float& vv, bool decay) {
        gg = mul_rn(gg, scale);
        if (decay) {
            if (decoupled) pp = mul_rn(pp, decay_f);
            else gg = add_rn(gg, mul_rn(wd, pp));
        }
        adam_update(pp, gg, mm, vv, w1, beta2, w2, step_size, bc2_sqrt, eps);
    };
    if (i < n4) {
        unsigned dm = 0;                        // bit j: element 4 i + j is decayed
        if (sg.decay_mask == sg.all_mask) {
            dm = 0xF;
        } else if (sg.decay_mask != 0) {
            const int s0 = seg_of(sg, 4 * i), s3 = seg_of(sg, 4 * i + 3);
            if (s0 == s3) {
                dm = (sg.decay_mask >> s0) & 1 ? 0xF : 0;
            } else {                            // the f32x4 straddles a boundary: each element takes its own segment's flag
#pragma unroll
                for (int j = 0; j < 4; ++j) dm |= ((sg.decay_mask >> seg_of(sg, 4 * i + j)) & 1) << j;
            }
        }
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i], mv = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pp = pv[j], mm = mv[j], v2 = vv[j];
            upd(pp, gv[j], mm, v2, (dm >> j) & 1);
            pv[j] = pp, mv[j] = mm, vv[j] = v2;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    } else if (i == n4) {
        for (int64_t j = 4 * n4; j < n; ++j) upd(p[j], g[j], m[j], v[j], (sg.decay_mask >> seg_of(sg, j)) & 1);
    }
}

int adam_flat_clipped(hipStream_t s, float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                      double eps, int64_t step, double weight_decay, int decoupled, const int64_t* seg_end, const int32_t* seg_decay,
                      int n_seg, int skip_nonfinite, const ClipRecord* rec) {
    S2VT_REQUIRE(n > 0, "adam_flat_clipped: n must be positive");
    auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    S2VT_REQUIRE(p && g && m && v && al(p) && al(g) && al(m) && al(v), "adam_flat_clipped: null / unaligned buffers");
    S2VT_REQUIRE(step >= 1, "adam_flat_clipped: step < 1");
    S2VT_REQUIRE(weight_decay >= 0 && !isinf(weight_decay), "adam_flat_clipped: weight_decay is negative or not finite");
    S2VT_REQUIRE(n_seg >= 0 && n_seg <= ADAM_MAX_SEGS, "adam_flat_clipped: n_seg outside [0, %d]", ADAM_MAX_SEGS);
    S2VT_REQUIRE(n_seg == 0 || (seg_end && seg_decay), "adam_flat_clipped: null segment arrays");
    S2VT_REQUIRE(al(rec) && (rec || !skip_nonfinite), "adam_flat_clipped: unaligned record, or skip_nonfinite without a record");
    AdamSegs sg;
    sg.decay_mask = 0;
    if (n_seg == 0) {                           // one segment, decayed
        sg.end[0] = n;
        sg.decay_mask = 1;
        n_seg = 1;
    } else {
        int64_t prev = 0;
        for (int k = 0; k < n_seg; ++k) {
            S2VT_REQUIRE(seg_end[k] > prev, "adam_flat_clipped: segment ends must ascend (segment %d ends at %lld)", k, (long long)seg_end[k]);
            sg.end[k] = prev = seg_end[k];
            if (seg_decay[k]) sg.decay_mask |= 1u << k;
        }
        S2VT_REQUIRE(prev == n, "adam_flat_clipped: the last segment must end at n (%lld != %lld)", (long long)prev, (long long)n);
    }
    for (int k = n_seg; k < ADAM_MAX_SEGS; ++k) sg.end[k] = n;
    sg.all_mask = (1u << n_seg) - 1u;
    if (weight_decay == 0) sg.decay_mask = 0;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(adam_clipped_kernel, dim3((unsigned)((n4 + 1 + 255) / 256)), dim3(256), 0, s, p, g, m, v, n4, n, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), step_size, bc2_sqrt, (float)eps, (float)weight_decay,
                       (float)(1.0 - lr * weight_decay), decoupled ? 1 : 0, sg, skip_nonfinite ? 1 : 0, rec);
    S2VT_LAUNCH_CHECK("adam_clipped_kernel");
    return 0;
}

}  // namespace s2vt
