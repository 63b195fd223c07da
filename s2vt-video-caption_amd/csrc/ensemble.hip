// The fan-out head of the ensemble beam search (include/s2vt_hip.h "ensemble beam"; tests/ensemble_ref.py restates it in numpy):
// M members' raw logits rows of one beam slot -> the log of the weighted mean of their word distributions and its 20 best words,
// in ascending token order as top20_logprob (ce.hip) returns them.  One 256-thread workgroup per row on the Row policies of
// row_frame.h (RegRow<16/32/48/64>, LdsRow) with top20_logprob's vocabulary brackets, its fixed-order block reductions and its
// extraction loop (top20_extract_row); no atomics: the same inputs give the same bits.
//   phase 1   per member m: load_max, sum_exp -> lse_m by top20_logprob_row's arithmetic, kept in LDS (s_lse)
//   phase 2   per element of the thread: the M values x_m[v] are read a SECOND time (M * V * 4 bytes the workgroup has just read:
//             cache hits) into registers, a_m[v] = (x_m[v] - lse_m) + lw_m, amax[v] = max_m a_m[v], c[v] = amax[v] + logf(sum_m
//             expf(a_m[v] - amax[v])), m ascending, into the row the thread keeps.  Unrolled over the 8 possible members with a
//             guard: no dynamically indexed register array.  The other form - amax kept in a second register row while x_m is
//             still in registers, so that phase 2 reads each member once more and nothing twice - was measured and lost: 168 us
//             against 120 us on 640 rows x 12000 words with M = 3 (profiles/beam_ensemble.txt); its 207 VGPRs at RegRow<48> leave
//             2 waves per SIMD where this form's 83 leave 5
//   phase 3   the extraction loop; top_lp = c (the mean of normalised distributions is normalised: nothing is subtracted)
// An element at -inf in every member has amax = -inf: c = -inf, never NaN (the sum is not looked at).
// The constrained form runs constrain_row on every member's row of the slot, in place, in front of phase 1 - the slot's own words
// (BeamHist) and the same spec for every member; each call ends in the barrier that orders its stores against the loads.
#include "common.h"
#include "kernels.h"
#include "row_frame.h"

namespace s2vt {

struct EnsembleArgs {
    const float* logits;             // member m's row r: logits + m * member_stride + r * ld
    int64_t member_stride, ld;
    int M, V;
    float lw[ENSEMBLE_MAX_M];        // fp32(log w_m), by value in the launch arguments
};

template <class Row>
__device__ __forceinline__ void ensemble_top20_row(const EnsembleArgs& e, int32_t* top_ix, float* top_lp) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    __shared__ float s_lse[ENSEMBLE_MAX_M], s_lw[ENSEMBLE_MAX_M];
    const int V = e.V, M = e.M;
    const float* x0 = e.logits + (int64_t)blockIdx.x * e.ld;
#pragma unroll
    for (int m = 0; m < ENSEMBLE_MAX_M; ++m)                   // (compile-time indices into the launch arguments)
        if ((int)threadIdx.x == m) s_lw[m] = e.lw[m];
    Row row;
    for (int m = 0; m < M; ++m) {
        // (the barrier in front of each reduction also publishes s_lw before its first read)
        const float mx = block_max_256(row.load_max(x0 + m * e.member_stride, V), red_v);
        const float lse = mx + logf(block_sum_256(row.sum_exp(mx, V), red_v));
        if (threadIdx.x == 0) s_lse[m] = lse;
    }
    __syncthreads();                                           // s_lse visible
    // (the register forms' pad slots, i >= V, keep the -inf of the last load_max: each() does not visit them)
    row.each(V, [&](int, int i, float& v) {
        float a[ENSEMBLE_MAX_M];
        float am = -INFINITY;
#pragma unroll
        for (int m = 0; m < ENSEMBLE_MAX_M; ++m) {
            a[m] = m < M ? (x0[m * e.member_stride + i] - s_lse[m]) + s_lw[m] : -INFINITY;
            am = fmaxf(am, a[m]);
        }
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < ENSEMBLE_MAX_M; ++m)
            if (m < M) s += expf(a[m] - am);
        v = am > -INFINITY ? am + logf(s) : -INFINITY;
    });
    top20_extract_row(row, V, 0.f, red_v, red_i, top_ix, top_lp);
}

template <class Row>
__global__ __launch_bounds__(256) void ensemble_top20_kernel(EnsembleArgs e, int32_t* top_ix, float* top_lp) {
    ensemble_top20_row<Row>(e, top_ix, top_lp);
}
template <class Row>
__global__ __launch_bounds__(256) void ensemble_top20_constrained_kernel(EnsembleArgs e, ConstrainArgs c, BeamHist hist, int32_t* top_ix,
                                                                         float* top_lp) {
    for (int m = 0; m < e.M; ++m)
        constrain_row(c, hist, const_cast<float*>(e.logits) + m * e.member_stride + (int64_t)blockIdx.x * e.ld, e.V);
    ensemble_top20_row<Row>(e, top_ix, top_lp);
}

// One launch of K<Row> for the vocabulary's bracket (top20_logprob's brackets)
#define S2VT_ENSEMBLE_LAUNCH(K, ...)                                                                                                  \
    do {                                                                                                                              \
        const dim3 grid((unsigned)rows), block(256);                                                                                  \
        const size_t lds = (size_t)V * sizeof(float);                                                                                 \
        if (V <= 256 * 16) hipLaunchKernelGGL(K<RegRow<16>>, grid, block, 0, s, __VA_ARGS__);                                         \
        else if (V <= 256 * 32) hipLaunchKernelGGL(K<RegRow<32>>, grid, block, 0, s, __VA_ARGS__);                                    \
        else if (V <= 256 * 48) hipLaunchKernelGGL(K<RegRow<48>>, grid, block, 0, s, __VA_ARGS__);                                    \
        else if (V <= 256 * 64) hipLaunchKernelGGL(K<RegRow<64>>, grid, block, 0, s, __VA_ARGS__);                                    \
        else {                                                                                                                        \
            if (lds > 48 * 1024)                                                                                                      \
                S2VT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K<LdsRow>), hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                             (int)lds));                                                                              \
            hipLaunchKernelGGL(K<LdsRow>, grid, block, lds, s, __VA_ARGS__);                                                          \
        }                                                                                                                             \
    } while (0)

static int ensemble_args(const char* fn, const float* logits, int64_t member_stride, int64_t ld, int M, int64_t rows, int V,
                         const float* log_w, const void* top_ix, const void* top_lp, EnsembleArgs* e) {
    S2VT_REQUIRE(logits && log_w && top_ix && top_lp, "%s: null argument", fn);
    S2VT_REQUIRE(M >= 1 && M <= ENSEMBLE_MAX_M, "%s: M %d outside [1, %d]", fn, M, ENSEMBLE_MAX_M);
    S2VT_REQUIRE(rows > 0 && rows < (1ll << 31), "%s: rows outside [1, 2^31)", fn);
    S2VT_REQUIRE(V >= TOPK_N && (size_t)V * sizeof(float) <= ROW_MAX_LDS, "%s: vocab_size %d outside [20, 38400]", fn, V);
    S2VT_REQUIRE(ld >= V, "%s: ld %lld < V %d", fn, (long long)ld, V);
    S2VT_REQUIRE(member_stride >= rows * ld, "%s: member_stride %lld < rows * ld = %lld", fn, (long long)member_stride,
                 (long long)(rows * ld));
    *e = EnsembleArgs{};
    e->logits = logits; e->member_stride = member_stride; e->ld = ld; e->M = M; e->V = V;
    for (int m = 0; m < M; ++m) {
        S2VT_REQUIRE(log_w[m] <= 0.f && log_w[m] >= -3.4028234e38f, "%s: log_w[%d] = %g must be finite and <= 0", fn, m, (double)log_w[m]);
        e->lw[m] = log_w[m];
    }
    return 0;
}
// one member of weight 1: c = a_0 = x - lse exactly, the head IS top20_logprob (bit for bit; that kernel runs)
static bool single_member(const EnsembleArgs& e) { return e.M == 1 && e.lw[0] == 0.f; }

int ensemble_top20(const char* fn, hipStream_t s, const float* logits, int64_t member_stride, int64_t ld, int M, int64_t rows, int V,
                   const float* log_w, int32_t* top_ix, float* top_lp) {
    EnsembleArgs e;
    int rc;
    if ((rc = ensemble_args(fn, logits, member_stride, ld, M, rows, V, log_w, top_ix, top_lp, &e))) return rc;
    if (single_member(e)) return top20_logprob(s, logits, ld, rows, V, top_ix, top_lp);
    S2VT_ENSEMBLE_LAUNCH(ensemble_top20_kernel, e, top_ix, top_lp);
    S2VT_LAUNCH_CHECK("ensemble_top20_kernel");
    return 0;
}

int ensemble_top20_constrained(const char* fn, hipStream_t s, float* logits, int64_t member_stride, int64_t ld, int M, int64_t rows,
                               int V, const float* log_w, const ConstrainArgs& c, const int32_t* hist, int64_t hist_ld, int32_t* top_ix,
                               float* top_lp) {
    EnsembleArgs e;
    int rc;
    if ((rc = ensemble_args(fn, logits, member_stride, ld, M, rows, V, log_w, top_ix, top_lp, &e))) return rc;
    S2VT_REQUIRE(c.t >= 0 && c.t <= CONSTRAIN_MAX_T && c.n_banned >= 0 && c.n_banned <= CONSTRAIN_MAX_BANNED && c.ngram >= 0 &&
                     c.eos < V && (c.t == 0 || (hist && hist_ld >= c.t)),
                 "%s: bad constraints", fn);
    for (int i = 0; i < c.n_banned; ++i) S2VT_REQUIRE(c.banned[i] >= 0 && c.banned[i] < V, "%s: banned id outside [0, V)", fn);
    S2VT_REQUIRE(V >= TOPK_N + c.t + c.n_banned + 1,
                 "%s: vocab_size %d < 20 + t + n_banned + 1 = %d: a row could keep fewer than 20 words", fn, V,
                 TOPK_N + c.t + c.n_banned + 1);
    if (single_member(e)) return top20_logprob_constrained(s, logits, ld, rows, V, c, hist, hist_ld, top_ix, top_lp);
    const BeamHist h{hist, hist_ld};
    S2VT_ENSEMBLE_LAUNCH(ensemble_top20_constrained_kernel, e, c, h, top_ix, top_lp);
    S2VT_LAUNCH_CHECK("ensemble_top20_constrained_kernel");
    return 0;
}

}  // namespace s2vt
