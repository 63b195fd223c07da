// The frame of the row kernels (ce.hip: the three criteria, their gradients, the beam searches' top-20 fan-out; split.hip: the
// fused criterion backward): 256-thread block reductions in ONE fixed order, the [:, 1:] read of a [B, L] matrix by flat row, the
// clamp of a bad target and the CE gradient of one element.  Device code only.
#pragma once
#include "common.h"

namespace s2vt {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Block reductions of a 256-thread workgroup through the caller's four LDS words: wave butterfly, the four waves combined in
// order.  Every thread gets the result.  The barrier in front lets a caller reduce again through the same words at once; the
// FIRST reduction of a kernel, whose words nobody has read yet, leaves it out (FRONT = false).
template <bool FRONT = true>
__device__ __forceinline__ float block_max_256(float v, float* sred) {
    v = wave_max(v);
    if (FRONT) __syncthreads();
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sred[0], sred[1]), fmaxf(sred[2], sred[3]));
}
template <bool FRONT = true>
__device__ __forceinline__ float block_sum_256(float s, float* sred) {
    s = wave_sum(s);
    if (FRONT) __syncthreads();
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = s;
    __syncthreads();
    return (sred[0] + sred[1]) + (sred[2] + sred[3]);
}
// Keyed maximum: the larger value wins, equal values -> the lower index.  (v, ix) in, the block's winner out, in every thread.
// NO barrier in front: the caller has one between the last read of red_v / red_i and this call (the extraction loop of the top-20
// kernel places it behind the owner's rescan; in front of the butterfly it costs the register forms 3 VGPRs and <48> a wave).
__device__ __forceinline__ void block_argmax_256(float& v, int& ix, float* red_v, int* red_i) {
    for (int o = 32; o; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(ix, o);
        if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
    }
    if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = v; red_i[threadIdx.x >> 6] = ix; }
    __syncthreads();
    v = red_v[0]; ix = red_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (red_v[w] > v || (red_v[w] == v && red_i[w] < ix)) { v = red_v[w]; ix = red_i[w]; }     // (red_i read on a tie only)
}

// x[:, 1:] of a [B, L] matrix (row stride ld) by flat row r = b * Lm1 + j  ->  x[b * ld + j + 1]: targets, masks, weights
// (R: the caller's row type - the division is 32-bit where its row index is)
template <typename T, typename R>
__device__ __forceinline__ T shifted_col(const T* x, R r, int Lm1, int64_t ld) {
    return x[(int64_t)(r / Lm1) * ld + (r % Lm1) + 1];
}
// a target outside [0, V) is flagged by the forward (ce_row_kernel); every reader of it takes the nearest valid id
__device__ __forceinline__ int64_t clamp_target(int64_t t, int V) { return t < 0 ? 0 : (t >= V ? V - 1 : t); }
// d(CE of a row)/d(logit x) * scale, hit = [this column is the row's target]: the materialised backwards (ce.hip) and the fused
// one (split.hip) come out bit for bit alike because both evaluate THIS expression
__device__ __forceinline__ float ce_grad(float x, float lse, bool hit, float scale) { return (expf(x - lse) - (hit ? 1.f : 0.f)) * scale; }

}  // namespace s2vt
