// The frame of the row kernels (ce.hip: the three criteria, their gradients, the beam searches' top-20 fan-out; split.hip: the
// fused criterion backward; truncate.hip: the truncated draw; ensemble.hip: the ensemble beam's fan-out): 256-thread block
// reductions in ONE fixed order, the two places a one-workgroup-per-row kernel keeps its row (RegRow<VPT> / LdsRow), the extraction
// loop of the fan-out heads (top20_extract_row), the constraint phase that the constrained draw and the
// constrained fan-out run in front of their row's load (constrain_row), the [:, 1:] read of a [B, L] matrix by flat row, the
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

// ---- where a one-workgroup-per-row kernel keeps its row (the top-20 fan-out of ce.hip, the truncated draw of truncate.hip).
// Thread tid owns the elements i = tid + 256 j; the interface is described at top20_logprob_kernel (ce.hip), plus
//   each(V, f)         f(slot, i, v) for every element i < V of the thread in ascending i, v a reference to its value; slot is the
//                      element's register index (a compile-time constant after unrolling) or 0 where the row is not in registers
//   slots(V, f)        the same over every slot the thread holds: the register forms' pad slots (i >= V, value -inf after
//                      load_max) included, WITHOUT a guard - in a kernel that walks the row many times 64 loop-invariant lane
//                      masks would otherwise be kept in (and spilled from) SGPRs; the caller gives the pads a neutral value
//   SLOTS              registers per thread that hold the row (0: none) - what a kernel sizes a second per-element array by
// The row in REGISTERS (VPT elements per thread): the owner's rescan after an extraction is VPT register compares instead of VPT
// dependent LDS reads (the LDS form spent 1.4 of its 4.7 us per extraction there: 95 us per launch at V = 12000, 640 rows; this
// one ~25).  Every access is unrolled with a compile-time index: vals never leaves the register file.
template <int VPT>
struct RegRow {
    static constexpr int SLOTS = VPT;
    float vals[VPT];
    __device__ __forceinline__ float load_max(const float* src, int V) {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int i = threadIdx.x + 256 * j;
            vals[j] = (i < V) ? src[i] : -INFINITY;
            mx = fmaxf(mx, vals[j]);
        }
        return mx;
    }
    __device__ __forceinline__ float sum_exp(float mx, int V) const {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < VPT; ++j)
            if ((int)threadIdx.x + 256 * j < V) sum += expf(vals[j] - mx);
        return sum;
    }
    __device__ __forceinline__ void best(float& bv, int& bi, int V) const {
        int bj = -1;
        bv = -INFINITY;
#pragma unroll
        for (int j = 0; j < VPT; ++j)
            if (vals[j] > bv) { bv = vals[j]; bj = j; }
        bi = bj >= 0 ? (int)threadIdx.x + 256 * bj : 0x7fffffff;
    }
    __device__ __forceinline__ void remove(int ix) {
        const int jj = ix >> 8;
#pragma unroll
        for (int j = 0; j < VPT; ++j) vals[j] = (j == jj) ? -INFINITY : vals[j];
    }
    template <class F>
    __device__ __forceinline__ void each(int V, F f) {
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < V) f(j, i, vals[j]);
        }
    }
    template <class F>
    __device__ __forceinline__ void slots(int V, F f) {
#pragma unroll
        for (int j = 0; j < VPT; ++j) f(j, (int)threadIdx.x + 256 * j, vals[j]);
    }
};
// The row staged in dynamic LDS (V floats): vocabularies beyond 64 elements per thread
struct LdsRow {
    static constexpr int SLOTS = 0;
    float* row;
    __device__ __forceinline__ float load_max(const float* src, int V) {
        extern __shared__ float top20_row[];
        row = top20_row;
        float mx = -INFINITY;
        for (int i = threadIdx.x; i < V; i += 256) {
            const float v = src[i];
            row[i] = v;
            mx = fmaxf(mx, v);
        }
        return mx;
    }
    __device__ __forceinline__ float sum_exp(float mx, int V) const {
        float sum = 0.f;
        for (int i = threadIdx.x; i < V; i += 256) sum += expf(row[i] - mx);
        return sum;
    }
    __device__ __forceinline__ void best(float& bv, int& bi, int V) const {
        bv = -INFINITY; bi = 0x7fffffff;
        for (int i = threadIdx.x; i < V; i += 256) {
            const float v = row[i];
            if (v > bv) { bv = v; bi = i; }
        }
    }
    __device__ __forceinline__ void remove(int ix) { row[ix] = -INFINITY; }
    template <class F>
    __device__ __forceinline__ void each(int V, F f) {
        for (int i = threadIdx.x; i < V; i += 256) f(0, i, row[i]);
    }
    template <class F>
    __device__ __forceinline__ void slots(int V, F f) { each(V, f); }       // (no pad slots)
};

// ---- the extraction loop of the fan-out heads (ce.hip: top20_logprob_row; ensemble.hip: the ensemble head): the largest element
// still in the row is taken out TOPK_N times (ties -> the lower token id), then the winners are ranked by token id and stored in
// ASCENDING token order as (id, value - sub): sub is the row's log-sum-exp where the row holds raw logits, 0 where it holds
// log-probs already.  Every thread keeps the best of its own elements; only the owner of an extracted element rescans.  red_v /
// red_i: the caller's four reduction words (free again once the barrier in front has passed).
constexpr int TOPK_N = 20;
template <class Row>
__device__ __forceinline__ void top20_extract_row(Row& row, int V, float sub, float* red_v, int* red_i, int32_t* top_ix, float* top_lp) {
    __shared__ float sel_v[TOPK_N];
    __shared__ int sel_i[TOPK_N];
    const int tid = threadIdx.x;
    __syncthreads();                                 // (block_argmax_256 has no barrier in front)
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
    if (tid < TOPK_N) {                              // rank by token id (ids are distinct)
        const int my = sel_i[tid];
        int rank = 0;
#pragma unroll
        for (int j = 0; j < TOPK_N; ++j) rank += (sel_i[j] < my);
        top_ix[(int64_t)blockIdx.x * TOPK_N + rank] = my;
        top_lp[(int64_t)blockIdx.x * TOPK_N + rank] = sel_v[tid] - sub;
    }
}

// ---- the constraint phase of the constrained row kernels (include/s2vt_hip.h "constrained draw"; sampling.constrain_logits restates
// it in numpy): repetition penalty, no-repeat n-gram blocking, banned ids and a minimum length, applied to the RAW logits row x
// IN PLACE in global memory, in front of the row's load and in the same launch - truncate.hip's constrained draw and ce.hip's
// constrained top-20 fan-out.  The row's history h[0..t) comes through an accessor (hist(i) = word i of THIS workgroup's row):
//   PackedHist   the decode drivers' packed words, hist[i * ld + row]; the token is 0xFFFFFFFF - the low half
//   BeamHist     the cumulative beam search's per-slot words (beam_policy.hip), int32 hist[row * ld + i]
//   candidates   c in [0, C), C = t + n_banned (+ 1): the t history tokens, the banned ids, <eos> while t < min_length - kept in
//                static LDS (tok) with one flag byte each (ban): the "edit list"
//   n-gram       one thread per start position i in [0, t - n]: n - 1 compares of h[i ..] against the suffix h[t-n+1 ..]; a match
//                flags position i + n - 1 (its own byte: no two threads write one)
//   edit         one thread per candidate c scans the list once: an EARLIER candidate with the same token owns the element (this
//                thread leaves), otherwise c is the element's only writer - it ORs the ban flags of every candidate with its token,
//                and writes -inf (a ban wins) or, where the token is in the history, the penalised value
// One barrier behind the stores orders them against the loads of row.load_max for the whole workgroup (its waves share a compute
// unit and its vector cache; not a threadgroup-split build).  Every loop runs to t, n, C or a compile-time count.  Tokens outside
// [0, V) (a history that no driver wrote) are matched like any other but never stored to.
// LDS: 1057 * 5 bytes here + the caller's few hundred - beside LdsRow's 150 KiB inside the 160 KiB of a workgroup.
constexpr int CONSTRAIN_MAX_T = 1023, CONSTRAIN_MAX_BANNED = 32;
constexpr int CONSTRAIN_MAX_C = CONSTRAIN_MAX_T + CONSTRAIN_MAX_BANNED + 1;
constexpr int ROW_MAX_LDS = 150 * 1024;                    // LdsRow's dynamic LDS at the largest vocabulary the row kernels take
static_assert(ROW_MAX_LDS + CONSTRAIN_MAX_C * 5 + 1024 <= 160 * 1024,
              "LdsRow's row + the constraint phase's edit list + a row kernel's own words must fit a workgroup's 160 KiB of LDS");

struct PackedHist {
    const unsigned long long* hist; int64_t ld;
    __device__ __forceinline__ int operator()(int i) const {
        return (int)(0xFFFFFFFFu - (uint32_t)(hist[(int64_t)i * ld + blockIdx.x] & 0xFFFFFFFFull));
    }
};
struct BeamHist {
    const int32_t* hist; int64_t ld;
    __device__ __forceinline__ int operator()(int i) const { return hist[(int64_t)blockIdx.x * ld + i]; }
};

// CA: kernels.h's ConstrainArgs (t, ngram, theta, inv_theta, eos, n_banned, banned); x: the workgroup's row
template <class Hist, class CA>
__device__ __forceinline__ void constrain_row(const CA& c, const Hist& hist, float* x, int V) {
    __shared__ int tok[CONSTRAIN_MAX_C];
    __shared__ unsigned char ban[CONSTRAIN_MAX_C];
    const int t = c.t, n = c.ngram, nb = c.n_banned;
    const int C = t + nb + (c.eos >= 0 ? 1 : 0);
    if (n > 0 || nb > 0 || c.eos >= 0 || c.theta != 1.f) {      // (block-uniform; nothing to edit: the caller's row work alone)
        for (int i = threadIdx.x; i < C; i += 256) {
            int v;
            if (i < t) v = hist(i);
            else if (i < t + nb) v = c.banned[i - t];
            else v = c.eos;
            tok[i] = v;
            ban[i] = i < t ? 0 : 1;
        }
        __syncthreads();
        if (n > 0) {
            for (int i = threadIdx.x; i <= t - n; i += 256) {
                bool same = true;
                for (int k = 0; k < n - 1; ++k) same = same && tok[i + k] == tok[t - n + 1 + k];
                if (same) ban[i + n - 1] = 1;
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < C; i += 256) {
            const int v = tok[i];
            const bool valid = (unsigned)v < (unsigned)V;
            const float xv = valid ? x[v] : 0.f;               // (issued in front of the scan: its latency runs beside it)
            bool first = true, banned = false, seen = false;
            // (no early exit: a plain reduction over the list, whose LDS reads the compiler batches)
#pragma unroll 8
            for (int k = 0; k < C; ++k) {
                const bool same = tok[k] == v;
                first = first && !(same && k < i);
                banned = banned || (same && ban[k] != 0);
                seen = seen || (same && k < t);
            }
            if (!(valid && first)) continue;
            if (banned) x[v] = -INFINITY;
            else if (seen && c.theta != 1.f) x[v] = xv > 0.f ? xv * c.inv_theta : xv * c.theta;
        }
        __syncthreads();                                       // the stores above -> the loads of load_max, workgroup scope
    }
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
