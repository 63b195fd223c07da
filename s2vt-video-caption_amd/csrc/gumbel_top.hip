// The fan-out head of stochastic beam search (S2VT.sample_distinct; Kool, van Hoof, Welling, ICML 2019; include/s2vt_hip.h
// "stochastic beam"): per logits row the 20 words with the largest PERTURBED log-probability g_v = lp_v + gumbel(seed, step, row, v),
// in the order (g descending, v ascending), with their unperturbed log-probs and their g.  One 256-thread workgroup per row on the
// Row policies of row_frame.h (RegRow<16/32/48/64>, LdsRow) with top20_logprob's vocabulary brackets and its fixed-order block
// reductions; no atomics: the same inputs give the same bits.
//   phase 1   load the row, scale it in place (s_v = x_v * inv_t, one fp32 product), max and sum-exp in the shared fixed order:
//             lse = max + logf(sum expf(s - max)).  max(s) = max(x) * inv_t bit for bit: inv_t > 0 and the rounded product is monotone.
//   phase 2   the row is rewritten in place - registers or LDS - with g_v = fminf(s_v - lse, 0) + noise(v)
//   phase 3   20 keyed extractions (block_argmax_256: the larger g, equal g -> the lower id), only the owner of an extracted element
//             rescans; the winners stay in extraction order
//   phase 4   thread k < 20 stores winner k: its id, its g, and its lp RECOMPUTED from the logits row as fminf(x * inv_t - lse, 0) -
//             the expression of phase 2 on the same operands, so the same bits; subtracting the noise back out of g would lose the
//             low bits of lp wherever |noise| > |lp|
// Noise and ownership.  A Philox block holds the draws of v / 4 = const, and thread tid owns the elements tid + 256 j of a row: no two
// of a thread's elements share a block, so EVERY ELEMENT RUNS ITS OWN BLOCK and keeps one of its four words (truncate.hip's tr_noise
// does the same for the kept elements of a truncated draw).  The four lanes 4q .. 4q+3 of a quad do compute the same block; sharing
// it (each lane one block of four slots, a rotation through the quad) would cut the ten rounds to a quarter but leave the three
// logarithms of the draw, which are most of the work, and would make a slot's register a lane-dependent choice.  Not done: the
// ownership stays the one of the Row policies, and an element's noise stays independent of the tiling (philox.h).
// The noise call is not inlined (tr_noise's reason: up to 64 unrolled slots of ten rounds and three logarithms spill).
#include <math.h>

#include "common.h"
#include "kernels.h"
#include "philox.h"
#include "row_frame.h"

namespace s2vt {

__device__ __noinline__ float gt_noise(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t row, uint32_t v) {
    const Philox4 r = philox4x32_10(v >> 2, row, step, GUMBEL_STREAM_TAG, seed_lo, seed_hi);
    return gumbel_from_bits((v & 2) ? ((v & 1) ? r.w[3] : r.w[2]) : ((v & 1) ? r.w[1] : r.w[0]));
}

// s_v = x_v * inv_t, rounded to fp32 on its own: contraction is off for this body, so that the subtraction of lse behind it never
// becomes one FMA with it - phase 2 and phase 4 then evaluate lp from the same rounded product
__device__ __forceinline__ float gt_scaled(float x, float inv_t) {
#pragma clang fp contract(off)
    const float s = x * inv_t;
    return s;
}

template <class Row>
__global__ __launch_bounds__(256) void top20_gumbel_kernel(const float* logits, int64_t ld, int V, GumbelArgs ga, int32_t* top_ix,
                                                           float* top_lp, float* top_g) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ float sel_v[TOPK_N];
    __shared__ int sel_i[TOPK_N];
    const int tid = threadIdx.x;
    const float* src = logits + (int64_t)blockIdx.x * ld;
    const float inv_t = ga.inv_temperature;
    const uint32_t nrow = ga.row0 + blockIdx.x;
    Row row;
    const float mx = block_max_256<false>(row.load_max(src, V), red_v) * inv_t;
    row.slots(V, [&](int, int, float& v) { v = gt_scaled(v, inv_t); });            // (a pad slot: -inf * inv_t = -inf)
    const float lse = mx + logf(block_sum_256(row.sum_exp(mx, V), red_v));
    row.each(V, [&](int, int i, float& v) { v = fminf(v - lse, 0.f) + gt_noise(ga.seed_lo, ga.seed_hi, ga.step, nrow, (uint32_t)i); });
    __syncthreads();                                 // (block_argmax_256 has no barrier in front; LdsRow: the rewritten row)
    float bv;
    int bi;
    row.best(bv, bi, V);
    for (int k = 0; k < TOPK_N; ++k) {
        float v = bv;
        int ix = bi;
        block_argmax_256(v, ix, red_v, red_i);
        if (tid == 0) { sel_v[k] = v; sel_i[k] = ix; }
        if ((ix & 255) == tid && ix < V) {           // owner: remove it and find the next best of its elements
            row.remove(ix);
            row.best(bv, bi, V);
        }
        __syncthreads();                             // (red_v / red_i free again, sel_* visible)
    }
    if (tid < TOPK_N) {                              // extraction order IS the output order
        const int ix = sel_i[tid];
        const int64_t o = (int64_t)blockIdx.x * TOPK_N + tid;
        const bool ok = ix >= 0 && ix < V;           // (always, for a row of 20 or more words that are not NaN)
        top_ix[o] = ok ? ix : 0;
        top_g[o] = sel_v[tid];
        top_lp[o] = ok ? fminf(gt_scaled(src[ix], inv_t) - lse, 0.f) : -INFINITY;
    }
}

int top20_gumbel(hipStream_t s, const float* logits, int64_t ld, int64_t rows, int V, const GumbelArgs& ga, int32_t* top_ix,
                 float* top_lp, float* top_g) {
    if (rows <= 0) return 0;
    S2VT_REQUIRE(logits && top_ix && top_lp && top_g && ld >= V && rows < (1ll << 31), "top20_gumbel: bad arguments");
    S2VT_REQUIRE(V >= TOPK_N && (size_t)V * sizeof(float) <= ROW_MAX_LDS, "top20_gumbel: 20 <= vocab_size <= 38400");
    const dim3 grid((unsigned)rows), block(256);
    const size_t lds = (size_t)V * sizeof(float);          // (the LDS form's dynamic LDS)
    if (V <= 256 * 16) hipLaunchKernelGGL(top20_gumbel_kernel<RegRow<16>>, grid, block, 0, s, logits, ld, V, ga, top_ix, top_lp, top_g);
    else if (V <= 256 * 32) hipLaunchKernelGGL(top20_gumbel_kernel<RegRow<32>>, grid, block, 0, s, logits, ld, V, ga, top_ix, top_lp, top_g);
    else if (V <= 256 * 48) hipLaunchKernelGGL(top20_gumbel_kernel<RegRow<48>>, grid, block, 0, s, logits, ld, V, ga, top_ix, top_lp, top_g);
    else if (V <= 256 * 64) hipLaunchKernelGGL(top20_gumbel_kernel<RegRow<64>>, grid, block, 0, s, logits, ld, V, ga, top_ix, top_lp, top_g);
    else {
        if (lds > 48 * 1024)
            S2VT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(top20_gumbel_kernel<LdsRow>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(top20_gumbel_kernel<LdsRow>, grid, block, lds, s, logits, ld, V, ga, top_ix, top_lp, top_g);
    }
    S2VT_LAUNCH_CHECK("top20_gumbel_kernel");
    return 0;
}

}  // namespace s2vt

using namespace s2vt;

extern "C" int s2vt_top20_gumbel(const float* logits, int64_t ld, int64_t rows, int32_t V, float inv_temperature, uint64_t seed, int32_t step,
                                 int32_t row0, int32_t* top_ix, float* top_lp, float* top_g, void* stream) {
    S2VT_REQUIRE(logits && top_ix && top_lp && top_g && rows > 0 && rows < (1ll << 31) && ld >= V && step >= 0 && row0 >= 0,
                 "s2vt_top20_gumbel: null/invalid argument");
    S2VT_REQUIRE(V >= TOPK_N && (size_t)V * sizeof(float) <= ROW_MAX_LDS, "s2vt_top20_gumbel: vocab_size %d outside [20, 38400]", (int)V);
    S2VT_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.4028234e38f, "s2vt_top20_gumbel: inv_temperature must be finite and > 0 (got %g)",
                 (double)inv_temperature);
    const GumbelArgs ga{inv_temperature, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)row0,
                        (uint32_t)row0 + (uint32_t)rows};
    return top20_gumbel((hipStream_t)stream, logits, ld, rows, V, ga, top_ix, top_lp, top_g);
}
