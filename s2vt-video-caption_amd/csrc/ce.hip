// Mean cross-entropy over vocabulary logits (utils.py:11,22: nn.CrossEntropyLoss() with the default
// 'mean' reduction over all B*(L-1) rows against target[:, 1:]) and its gradient.
// One 256-thread workgroup per logits row: 16-B vector loads, wave shuffles + LDS for the row max and
// the exp-sum; per-row losses are then summed in a fixed order by a single workgroup (deterministic).
#include <stdlib.h>

#include "common.h"
#include "kernels.h"
#include "row_frame.h"

namespace s2vt {

__global__ __launch_bounds__(256) void ce_row_kernel(const float* logits, int V, const int64_t* target, int Lm1,
                                                     int64_t ldt, float* lse, float* rowloss, int* err) {
    __shared__ float sred[4];
    const int64_t r = blockIdx.x;
    const float* row = logits + r * V;
    const int tid = threadIdx.x;
    const bool vec = (V % 4 == 0) && ((reinterpret_cast<uintptr_t>(row) & 15) == 0);
    // Rows of up to 16384 logits are held in registers between the max pass and the exp-sum pass (16 x f32x4 per
    // thread): the row is read from memory once.  Same operations in the same order as the two-pass form.
    constexpr int NBUF = 16;
    const bool reg = vec && V <= NBUF * 1024;
    f32x4 buf[NBUF];
    float m = -INFINITY;
    if (reg) {
#pragma unroll
        for (int i = 0; i < NBUF; ++i) {
            const int c = tid * 4 + i * 1024;
            if (c < V) {
                buf[i] = *reinterpret_cast<const f32x4*>(row + c);
                m = fmaxf(fmaxf(m, fmaxf(buf[i][0], buf[i][1])), fmaxf(buf[i][2], buf[i][3]));
            }
        }
    } else if (vec) {
        for (int c = tid * 4; c < V; c += 1024) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
            m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
        }
    } else {
        for (int c = tid; c < V; c += 256) m = fmaxf(m, row[c]);
    }
    m = block_max_256<false>(m, sred);
    float s = 0.f;
    if (reg) {
#pragma unroll
        for (int i = 0; i < NBUF; ++i) {
            const int c = tid * 4 + i * 1024;
            if (c < V) s += expf(buf[i][0] - m) + expf(buf[i][1] - m) + expf(buf[i][2] - m) + expf(buf[i][3] - m);
        }
    } else if (vec) {
        for (int c = tid * 4; c < V; c += 1024) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
            s += expf(v[0] - m) + expf(v[1] - m) + expf(v[2] - m) + expf(v[3] - m);
        }
    } else {
        for (int c = tid; c < V; c += 256) s += expf(row[c] - m);
    }
    const float tot = block_sum_256(s, sred);
    if (tid == 0) {
        const float l = logf(tot) + m;
        const int64_t t = shifted_col(target, r, Lm1, ldt);
        if ((t < 0 || t >= V) && err) atomicExch(err, 2);
        lse[r] = l;
        rowloss[r] = l - row[clamp_target(t, V)];
    }
}

// loss = (sum_r rowloss[r]) / rows, fixed summation order (one workgroup, fp32 pairwise per thread strip).
__global__ __launch_bounds__(256) void ce_mean_kernel(const float* rowloss, int64_t rows, float* loss_out) {
    __shared__ float sred[4];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int64_t r = tid; r < rows; r += 256) s += rowloss[r];
    s = block_sum_256<false>(s, sred);
    if (tid == 0) loss_out[0] = s / (float)rows;
}

// The forward of every criterion: ce_row_kernel over the rows, then ONE workgroup of the finisher handed in.
template <typename... P, typename... A>
static int ce_fwd(hipStream_t s, const float* logits, int64_t rows, int V, const int64_t* target, int Lm1, int64_t ldt, float* lse,
                  float* rowloss, int* err_flag, void (*finisher)(P...), const char* name, A... args) {
    hipLaunchKernelGGL(ce_row_kernel, dim3((unsigned)rows), dim3(256), 0, s, logits, V, target, Lm1, ldt, lse, rowloss, err_flag);
    S2VT_LAUNCH_CHECK("ce_row_kernel");
    hipLaunchKernelGGL(finisher, dim3(1), dim3(256), 0, s, args...);
    S2VT_LAUNCH_CHECK(name);
    return 0;
}
int mean_ce_fwd(hipStream_t s, const float* logits, int64_t rows, int V, const int64_t* target, int Lm1, int64_t ldt,
                float* lse, float* rowloss, float* loss_out, int* err_flag) {
    S2VT_REQUIRE(rows > 0 && V > 0 && logits && target && lse && rowloss && loss_out, "mean_ce_fwd: bad arguments");
    return ce_fwd(s, logits, rows, V, target, Lm1, ldt, lse, rowloss, err_flag, ce_mean_kernel, "ce_mean_kernel", rowloss, rows,
                  loss_out);
}

// ---------------------------------------------------------------------------------- MaskCriterion's outer arithmetic
// utils.py:23-25 of the reference around the mean CE: w = mask[:, 1:] flattened, loss = sum(mean_ce * w) / sum(w) (NaN for an
// all-zero mask, as upstream), evaluated product by product as the reference does - ONE workgroup behind the per-row kernel
// instead of a dozen elementwise / reduction launches of the host framework.  out[0] = loss, out[1] = mean_ce, out[2] = sum(w).
// Fixed summation order (thread strips, wave butterfly, four waves in order): deterministic.
__global__ __launch_bounds__(256) void mask_criterion_fwd_kernel(const float* rowloss, int64_t rows, const float* mask, int64_t ldm,
                                                                 int Lm1, float* out) {
    __shared__ float sred[4];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int64_t r = tid; r < rows; r += 256) s += rowloss[r];
    const float mean_ce = block_sum_256(s, sred) / (float)rows;          // (ce_mean_kernel's arithmetic)
    float num = 0.f, den = 0.f;
    for (int64_t r = tid; r < rows; r += 256) {
        const float w = shifted_col(mask, r, Lm1, ldm);
        num += mean_ce * w;
        den += w;
    }
    num = block_sum_256(num, sred);
    den = block_sum_256(den, sred);
    if (tid == 0) { out[0] = num / den; out[1] = mean_ce; out[2] = den; }
}
// autograd of the same three lines: d loss / d mean_ce = sum_i (gout / sum(w)) * w_i  ->  g_ce[0]
__global__ __launch_bounds__(256) void mask_criterion_bwd_kernel(const float* mask, int64_t ldm, int64_t rows, int Lm1, const float* fwd_out,
                                                                 const float* gout, float* g_ce) {
    __shared__ float sred[4];
    const int tid = threadIdx.x;
    const float q = gout[0] / fwd_out[2];
    float s = 0.f;
    for (int64_t r = tid; r < rows; r += 256) s += q * shifted_col(mask, r, Lm1, ldm);
    s = block_sum_256(s, sred);
    if (tid == 0) g_ce[0] = s;
}

int mask_criterion_fwd(hipStream_t s, const float* logits, int64_t rows, int V, const int64_t* target, int Lm1, int64_t ldt,
                       const float* mask, int64_t ldm, float* lse, float* rowloss, float* out3, int* err_flag) {
    S2VT_REQUIRE(rows > 0 && V > 0 && logits && target && mask && lse && rowloss && out3, "mask_criterion_fwd: bad arguments");
    return ce_fwd(s, logits, rows, V, target, Lm1, ldt, lse, rowloss, err_flag, mask_criterion_fwd_kernel, "mask_criterion_fwd_kernel",
                  rowloss, rows, mask, ldm, Lm1, out3);
}
int mask_criterion_bwd(hipStream_t s, const float* mask, int64_t ldm, int64_t rows, int Lm1, const float* fwd_out, const float* gout,
                       float* g_ce) {
    S2VT_REQUIRE(rows > 0 && mask && fwd_out && gout && g_ce, "mask_criterion_bwd: bad arguments");
    hipLaunchKernelGGL(mask_criterion_bwd_kernel, dim3(1), dim3(256), 0, s, mask, ldm, rows, Lm1, fwd_out, gout, g_ce);
    S2VT_LAUNCH_CHECK("mask_criterion_bwd_kernel");
    return 0;
}

// One row of a criterion's gradient: drow[v] = ce_grad(row[v], lse, v == t, scale), 16-byte accesses where V and both rows allow
__device__ __forceinline__ void ce_grad_row(const float* row, float* drow, int V, int64_t t, float lse, float scale) {
    const int tid = threadIdx.x;
    const bool vec = (V % 4 == 0) && ((reinterpret_cast<uintptr_t>(row) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(drow) & 15) == 0);
    if (vec) {
        for (int c = tid * 4; c < V; c += 1024) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
            f32x4 d;
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = ce_grad(v[j], lse, (c + j) == t, scale);
            *reinterpret_cast<f32x4*>(drow + c) = d;
        }
    } else {
        for (int c = tid; c < V; c += 256) drow[c] = ce_grad(row[c], lse, c == t, scale);
    }
}

// dlogits[r][v] = (exp(logit - lse_r) - [v == target_r]) * gout / rows
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* logits, int64_t rows, int V, const int64_t* target,
                                                     int Lm1, int64_t ldt, const float* lse, const float* gout,
                                                     float* dlogits) {
    const int64_t r = blockIdx.x;
    ce_grad_row(logits + r * V, dlogits + r * V, V, clamp_target(shifted_col(target, r, Lm1, ldt), V), lse[r], gout[0] / (float)rows);
}

int mean_ce_bwd(hipStream_t s, const float* logits, int64_t rows, int V, const int64_t* target, int Lm1, int64_t ldt,
                const float* lse, const float* gout, float* dlogits) {
    S2VT_REQUIRE(rows > 0 && V > 0 && logits && target && lse && gout && dlogits, "mean_ce_bwd: bad arguments");
    hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, s, logits, rows, V, target, Lm1, ldt, lse,
                       gout, dlogits);
    S2VT_LAUNCH_CHECK("ce_bwd_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------- reward-weighted CE (utils.RewardCriterion)
// loss = sum_r w_r * (lse_r - logit_r[target_r]) / norm,  w_r = weight[b][j + 1] of row r = b * Lm1 + j (read at [:, 1:] like the
// mask above), norm = max(number of rows with w_r != 0, 1): the mean over the tokens that carry a weight - a self-critical
// advantage of either sign, or a 0/1 padding mask - and 0 (not NaN) when none does.  out2 = {loss, norm}.  The per-row kernel is
// the mean CE's; ONE workgroup sums in a fixed order (thread strips, wave butterfly, four waves in order): deterministic.
__global__ __launch_bounds__(256) void weighted_ce_fwd_kernel(const float* rowloss, int64_t rows, const float* weight, int64_t ldw,
                                                              int Lm1, float* out) {
    __shared__ float sred[4];
    const int tid = threadIdx.x;
    float num = 0.f, cnt = 0.f;
    for (int64_t r = tid; r < rows; r += 256) {
        const float w = shifted_col(weight, r, Lm1, ldw);
        if (w != 0.f) { num += w * rowloss[r]; cnt += 1.f; }       // (a zero weight drops the row even where its loss is inf)
    }
    num = block_sum_256(num, sred);
    cnt = block_sum_256(cnt, sred);                                // (integers below 2^24: exact)
    if (tid == 0) {
        const float norm = fmaxf(cnt, 1.f);
        out[0] = num / norm; out[1] = norm;
    }
}
// dlogits[r][v] = w_r * (exp(logit - lse_r) - [v == target_r]) * gout / norm; rows without a weight are written as zeros
__global__ __launch_bounds__(256) void weighted_ce_bwd_kernel(const float* logits, int V, const int64_t* target, int Lm1, int64_t ldt,
                                                              const float* weight, int64_t ldw, const float* lse, const float* fwd_out,
                                                              const float* gout, float* dlogits) {
    const int64_t r = blockIdx.x;
    float* drow = dlogits + r * V;
    const float w = shifted_col(weight, r, Lm1, ldw);
    if (w == 0.f) {                                                // (its lse may be inf or NaN: never read)
        for (int c = threadIdx.x; c < V; c += 256) drow[c] = 0.f;
        return;
    }
    ce_grad_row(logits + r * V, drow, V, clamp_target(shifted_col(target, r, Lm1, ldt), V), lse[r], w * (gout[0] / fwd_out[1]));
}

int weighted_ce_fwd(hipStream_t s, const float* logits, int64_t rows, int V, const int64_t* target, int Lm1, int64_t ldt,
                    const float* weight, int64_t ldw, float* lse, float* rowloss, float* out2, int* err_flag) {
    S2VT_REQUIRE(rows > 0 && V > 0 && logits && target && weight && lse && rowloss && out2, "weighted_ce_fwd: bad arguments");
    return ce_fwd(s, logits, rows, V, target, Lm1, ldt, lse, rowloss, err_flag, weighted_ce_fwd_kernel, "weighted_ce_fwd_kernel",
                  rowloss, rows, weight, ldw, Lm1, out2);
}
int weighted_ce_bwd(hipStream_t s, const float* logits, int64_t rows, int V, const int64_t* target, int Lm1, int64_t ldt,
                    const float* weight, int64_t ldw, const float* lse, const float* fwd_out, const float* gout, float* dlogits) {
    S2VT_REQUIRE(rows > 0 && V > 0 && logits && target && weight && lse && fwd_out && gout && dlogits, "weighted_ce_bwd: bad arguments");
    hipLaunchKernelGGL(weighted_ce_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, s, logits, V, target, Lm1, ldt, weight, ldw, lse,
                       fwd_out, gout, dlogits);
    S2VT_LAUNCH_CHECK("weighted_ce_bwd_kernel");
    return 0;
}


// ---------------------------------------------------------------------------------- beam-search fan-out
// Per logits row: log_softmax (S2VTModel.py:214) and the 20 most probable tokens with their log-probs, returned in
// ASCENDING token order - the order in which the reference pushes them (it scans the vocabulary and keeps the ids that
// are in topk(20), S2VTModel.py:216-219).  One workgroup per row: the row is reduced to max and sum-exp, then the largest
// remaining element is extracted 20 times (ties -> the lower token id).  Thread tid owns the elements i = tid + 256 j; where
// they live is the kernel's Row policy:
//   load_max(src, V)   fetch the thread's elements, return their maximum
//   sum_exp(mx, V)     sum of expf(x - mx) over them, ascending i
//   best(v, ix, V)     the largest of them still there and its token id (ascending i: the first, i.e. lowest id, of equal
//                      values is kept); (-inf, 0x7fffffff) when none is left
//   remove(ix)         take element ix (one of the thread's) out
// (RegRow<VPT> / LdsRow and the extraction loop with TOPK_N = 20: row_frame.h, shared with the truncated draw of truncate.hip and
// the ensemble head of ensemble.hip)
// Same arithmetic in the same order for every Row: max, then the sum of expf(x - max) per thread in ascending i, wave
// butterflies, (w0 + w1) + (w2 + w3); ties -> the lower token id.
template <class Row>
__device__ __forceinline__ void top20_logprob_row(const float* logits, int64_t ld, int V, int32_t* top_ix, float* top_lp) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    Row row;
    const float mx = block_max_256<false>(row.load_max(logits + (int64_t)blockIdx.x * ld, V), red_v);
    const float lse = mx + logf(block_sum_256(row.sum_exp(mx, V), red_v));
    top20_extract_row(row, V, lse, red_v, red_i, top_ix, top_lp);        // (row_frame.h, shared with the ensemble head)
}
template <class Row>
__global__ __launch_bounds__(256) void top20_logprob_kernel(const float* logits, int64_t ld, int V, int32_t* top_ix, float* top_lp) {
    top20_logprob_row<Row>(logits, ld, V, top_ix, top_lp);
}
// The fan-out of the CONSTRAINED cumulative beam search (S2VT.beam_constrained; include/s2vt_hip.h "constrained beam"): the
// constraint phase of the constrained draw (row_frame.h, constrain_row) in front of the same row work, in the same launch - the
// row of `logits` is EDITED IN PLACE, then loaded: max, sum-exp and the 20 extractions see the edited row, so the log-probs are
// renormalised over the surviving words and a banned word (-inf) is never extracted while 20 finite words are left (the callers
// refuse shapes that could leave fewer: V >= 20 + t + n_banned + 1).  The row's history is beam slot blockIdx.x's own words,
// int32 hist[row * hist_ld + i] (beam_policy.hip keeps them).  expf(-inf - max) is +0: an edited element adds nothing to the sum.
// LDS: the phase's 1057 * 5 bytes + 176 here, beside LdsRow's 150 KiB (row_frame.h asserts the sum against 160 KiB).
template <class Row>
__global__ __launch_bounds__(256) void top20_logprob_constrained_kernel(float* logits, int64_t ld, int V, ConstrainArgs c, BeamHist hist,
                                                                        int32_t* top_ix, float* top_lp) {
    constrain_row(c, hist, logits + (int64_t)blockIdx.x * ld, V);
    top20_logprob_row<Row>(logits, ld, V, top_ix, top_lp);
}

int top20_logprob_constrained(hipStream_t s, float* logits, int64_t ld, int64_t rows, int V, const ConstrainArgs& c, const int32_t* hist,
                              int64_t hist_ld, int32_t* top_ix, float* top_lp) {
    if (rows <= 0) return 0;
    S2VT_REQUIRE(logits && top_ix && top_lp && ld >= V && rows < (1ll << 31), "top20_logprob_constrained: bad arguments");
    S2VT_REQUIRE(V >= TOPK_N && (size_t)V * sizeof(float) <= ROW_MAX_LDS, "top20_logprob_constrained: 20 <= vocab_size <= 38400");
    S2VT_REQUIRE(c.t >= 0 && c.t <= CONSTRAIN_MAX_T && c.n_banned >= 0 && c.n_banned <= CONSTRAIN_MAX_BANNED && c.ngram >= 0 &&
                     c.eos < V && (c.t == 0 || (hist && hist_ld >= c.t)),
                 "top20_logprob_constrained: bad constraints");
    for (int i = 0; i < c.n_banned; ++i)
        S2VT_REQUIRE(c.banned[i] >= 0 && c.banned[i] < V, "top20_logprob_constrained: banned id outside [0, V)");
    S2VT_REQUIRE(V >= TOPK_N + c.t + c.n_banned + 1,
                 "top20_logprob_constrained: vocab_size %d < 20 + t + n_banned + 1 = %d: a row could keep fewer than 20 words", V,
                 TOPK_N + c.t + c.n_banned + 1);
    const BeamHist h{hist, hist_ld};
    const dim3 grid((unsigned)rows), block(256);
    const size_t lds = (size_t)V * sizeof(float);          // (the LDS form's dynamic LDS)
    if (V <= 256 * 16) hipLaunchKernelGGL(top20_logprob_constrained_kernel<RegRow<16>>, grid, block, 0, s, logits, ld, V, c, h, top_ix, top_lp);
    else if (V <= 256 * 32) hipLaunchKernelGGL(top20_logprob_constrained_kernel<RegRow<32>>, grid, block, 0, s, logits, ld, V, c, h, top_ix, top_lp);
    else if (V <= 256 * 48) hipLaunchKernelGGL(top20_logprob_constrained_kernel<RegRow<48>>, grid, block, 0, s, logits, ld, V, c, h, top_ix, top_lp);
    else if (V <= 256 * 64) hipLaunchKernelGGL(top20_logprob_constrained_kernel<RegRow<64>>, grid, block, 0, s, logits, ld, V, c, h, top_ix, top_lp);
    else {
        if (lds > 48 * 1024)
            S2VT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(top20_logprob_constrained_kernel<LdsRow>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(top20_logprob_constrained_kernel<LdsRow>, grid, block, lds, s, logits, ld, V, c, h, top_ix, top_lp);
    }
    S2VT_LAUNCH_CHECK("top20_logprob_constrained_kernel");
    return 0;
}

int top20_logprob(hipStream_t s, const float* logits, int64_t ld, int64_t rows, int V, int32_t* top_ix, float* top_lp) {
    if (rows <= 0) return 0;
    S2VT_REQUIRE(V >= TOPK_N && (size_t)V * sizeof(float) <= 150 * 1024, "top20_logprob: 20 <= vocab_size <= 38400");
    const dim3 grid((unsigned)rows), block(256);
    const size_t lds = (size_t)V * sizeof(float);          // (the LDS form's dynamic LDS)
    if (V <= 256 * 16) hipLaunchKernelGGL(top20_logprob_kernel<RegRow<16>>, grid, block, 0, s, logits, ld, V, top_ix, top_lp);
    else if (V <= 256 * 32) hipLaunchKernelGGL(top20_logprob_kernel<RegRow<32>>, grid, block, 0, s, logits, ld, V, top_ix, top_lp);
    else if (V <= 256 * 48) hipLaunchKernelGGL(top20_logprob_kernel<RegRow<48>>, grid, block, 0, s, logits, ld, V, top_ix, top_lp);
    else if (V <= 256 * 64) hipLaunchKernelGGL(top20_logprob_kernel<RegRow<64>>, grid, block, 0, s, logits, ld, V, top_ix, top_lp);
    else {
        if (lds > 48 * 1024)
            S2VT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(top20_logprob_kernel<LdsRow>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(top20_logprob_kernel<LdsRow>, grid, block, lds, s, logits, ld, V, top_ix, top_lp);
    }
    S2VT_LAUNCH_CHECK("top20_logprob_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------- caption scoring (S2VT.forward(mode='score'))
// Per logits row: the log-probability of ONE given token, lp = min(x[t] - max - logf(sum_i expf(x[i] - max)), 0) - log_softmax
// (S2VTModel.py:214) read at the target instead of fanned out.  One workgroup per row, the row read from memory twice (max pass,
// exp-sum pass): nothing of it is kept in LDS or registers, so V is unbounded.  Order of the sums as in ce_row_kernel: thread strips
// in ascending i (16-byte loads over the multiple-of-4 part of a 16-byte-aligned row, the last V % 4 elements scalar; a row that
// is not aligned scalar throughout), wave butterfly, (w0 + w1) + (w2 + w3).  A target outside [0, V) raises *err and reads the
// clamped column (clamp_target).
__global__ __launch_bounds__(256) void pick_logprob_kernel(const float* logits, int64_t ld, int V, const int32_t* target, float* lp_out,
                                                           int* err) {
    __shared__ float sred[4];
    const int64_t r = blockIdx.x;
    const float* row = logits + r * ld;
    const int tid = threadIdx.x;
    const int V4 = ((reinterpret_cast<uintptr_t>(row) & 15) == 0) ? (V & ~3) : 0;       // the part read by 16-byte loads
    float m = -INFINITY;
    for (int c = tid * 4; c < V4; c += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
        m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    for (int c = V4 + tid; c < V; c += 256) m = fmaxf(m, row[c]);
    m = block_max_256<false>(m, sred);
    float s = 0.f;
    for (int c = tid * 4; c < V4; c += 1024) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + c);
        s += expf(v[0] - m) + expf(v[1] - m) + expf(v[2] - m) + expf(v[3] - m);
    }
    for (int c = V4 + tid; c < V; c += 256) s += expf(row[c] - m);
    const float tot = block_sum_256(s, sred);
    if (tid == 0) {
        const int64_t t = target[r];
        if ((t < 0 || t >= V) && err) atomicExch(err, 2);
        lp_out[r] = fminf(row[clamp_target(t, V)] - m - logf(tot), 0.f);
    }
}
int pick_logprob(hipStream_t s, const float* logits, int64_t ld, int64_t rows, int V, const int32_t* target, float* lp_out, int* err_flag) {
    if (rows <= 0) return 0;
    S2VT_REQUIRE(V > 0 && ld >= V && logits && target && lp_out, "pick_logprob: bad arguments");
    hipLaunchKernelGGL(pick_logprob_kernel, dim3((unsigned)rows), dim3(256), 0, s, logits, ld, V, target, lp_out, err_flag);
    S2VT_LAUNCH_CHECK("pick_logprob_kernel");
    return 0;
}

// The captions of a scoring call, caps[b][k][j] at b * stride_b + k * stride_k + j (either stride may be 0: a broadcast view), as
// what the word steps and the head read: tok [T][Rp] int32, time-major over the fixed rows r = b * K + k (rows R..Rp: token 0),
// and row_b [Rp] = r / K (pad rows: 0).  EVERY id of the tensor is checked, also behind the first <eos> (nn.Embedding would have
// seen it, S2VTModel.py:71): one outside [0, V) raises *err and is stored clamped, so nothing downstream indexes with it.
__global__ __launch_bounds__(256) void score_prep_kernel(const int64_t* caps, int64_t stride_b, int64_t stride_k, int R, int K, int T,
                                                         int Rp, int V, int32_t* tok, int32_t* row_b, int* err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)T * Rp) return;
    const int j = (int)(i / Rp), r = (int)(i % Rp);
    int32_t t = 0;
    if (r < R) {
        const int64_t c = caps[(int64_t)(r / K) * stride_b + (int64_t)(r % K) * stride_k + j];
        if (c < 0 || c >= V) atomicExch(err, 1);
        t = (int32_t)clamp_target(c, V);
    }
    tok[i] = t;
    if (j == 0) row_b[r] = r < R ? r / K : 0;
}
int score_prep(hipStream_t s, const int64_t* caps, int64_t stride_b, int64_t stride_k, int R, int K, int T, int Rp, int V, int32_t* tok,
               int32_t* row_b, int* err_flag) {
    S2VT_REQUIRE(caps && tok && row_b && err_flag && R > 0 && K > 0 && T > 1 && Rp >= R && V > 0, "score_prep: bad arguments");
    const int64_t n = (int64_t)T * Rp;
    hipLaunchKernelGGL(score_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, caps, stride_b, stride_k, R, K, T, Rp, V,
                       tok, row_b, err_flag);
    S2VT_LAUNCH_CHECK("score_prep_kernel");
    return 0;
}

// The finisher of a scoring call, one lane per caption: n = the position of the first <eos> among tok[1..T-1] counted from 1 (none:
// T - 1), token_lp[r][j] = lp[j][r] for j < n and 0 behind, score = (their fp32 sum, j ascending) / powa[n], powa[n] = fp32(n **
// alpha) from the host's table (beam_policy.hip's power rule).  Sequential per caption: deterministic.
__global__ __launch_bounds__(256) void score_finish_kernel(const float* lp, const int32_t* tok, int R, int Rp, int T, int eos,
                                                           const float* powa, float* token_lp, float* score, int64_t* length) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const int S = T - 1;
    int n = S;
    for (int j = 0; j < S; ++j)
        if (tok[(int64_t)(j + 1) * Rp + r] == eos) { n = j + 1; break; }
    float sum = 0.f;
    for (int j = 0; j < S; ++j) {
        const float l = j < n ? lp[(int64_t)j * Rp + r] : 0.f;
        token_lp[(int64_t)r * S + j] = l;
        if (j < n) sum += l;
    }
    score[r] = sum / powa[n];
    length[r] = n;
}
int score_finish(hipStream_t s, const float* lp, const int32_t* tok, int R, int Rp, int T, int eos, const float* powa, float* token_lp,
                 float* score, int64_t* length) {
    S2VT_REQUIRE(lp && tok && powa && token_lp && score && length && R > 0 && Rp >= R && T > 1, "score_finish: bad arguments");
    hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, lp, tok, R, Rp, T, eos, powa, token_lp,
                       score, length);
    S2VT_LAUNCH_CHECK("score_finish_kernel");
    return 0;
}

}  // namespace s2vt
