// (Behind the truncated draw, in this file: the constrained draw - the same row kernel with a constraint phase in front of its load.)
// Top-k / nucleus (top-p) truncation ahead of the sampled draw (include/s2vt_hip.h "truncated draw" states the definition;
// sampling.truncation_mask restates it in numpy).  The fused sampling heads never hold a logits row, so no element knows its rank;
// here the row exists ([rows, V] fp32 from the logits GEMM) and ONE 256-thread workgroup per row holds it - in registers
// (RegRow<16/32/48/64>) or dynamic LDS (LdsRow) - from the load to the draw.  Per row, with s_v = x_v * inv_t:
//   top-k     tau = the k-th largest s counted with multiplicity; survivors {v : s_v >= tau} (ties at the k-th place all stay)
//   nucleus   over the survivors: m = max s, e_v = expf(s_v - m), Z = sum e; v stays iff A(s_v) < p * Z, A(y) = sum of e_u over
//             s_u > y - the shortest descending prefix whose mass reaches p; equal values stay or go together, the maximum stays
//   draw      argmax over the kept v of s_v + g_v, g the heads' noise (philox.h: counter (v / 4, row, step, tag), word v % 4);
//             the lowest index wins a tie; written as the heads' packed word by a plain 64-bit store (the workgroup owns the row)
//
// How the two thresholds are found: by bisection over the 32 bits of the order-preserving key of s, MSB first, one block
// reduction per bit - an integer count of {key >= candidate} for top-k, the fixed-order fp32 sum A(candidate) for the nucleus.
//   - Every sum is per thread in ascending element order, wave butterfly, (w0 + w1) + (w2 + w3) (row_frame.h's order): no
//     floating-point atomics, same inputs -> same bits.  Raising the candidate only replaces terms of that sum by +0 in place;
//     with round-to-nearest and non-negative terms such a sum is monotone in each term, so "A(y) < p * Z" is a monotone
//     predicate of y in fp32 as well - that is what allows a threshold search instead of a sort.
//   - Chosen over an 8-bit radix select through a 256-bin LDS histogram: that form needs VPT LDS atomics per thread and pass,
//     and logits with many equal values (a saturated or quantised row) send whole waves to ONE bin, where the LDS serialises
//     them - its time depends on the data.  The bit passes are VPT register compares + 6 shuffles + one barrier (the four wave
//     partials alternate between two sets of LDS words), the same for every input, and the nucleus needs the float sums per
//     candidate anyway.  Measured on 640 rows x 12 000 (profiles/sample_trunc.txt): 73 us with top-k, 126 us with the nucleus,
//     beside 47 us for the top-20 fan-out's 20 extractions and 169 us for the logits GEMM in front.  Two bits per pass (three
//     candidates and three sums per pass, 16 + 16 passes) was built and measured no faster: 78 and 130 us - the passes are
//     bound by their register work, not by the barrier - so the simpler form stays.
//   - Registers: the register forms keep s (VPT) and e (VPT) - 2 * 48 = 96 at V = 12 000, 128 at VPT = 64, inside the 512 of
//     a SIMD's one wave per 256-thread workgroup; e is stored because recomputing expf in each of the 32 passes would be
//     32 * VPT transcendental sequences.  LdsRow has no second V floats of LDS left and does recompute it (V > 16 384 only).
// Every loop has a compile-time trip count (32 key bits, VPT) or runs to V; nothing spins, nothing crosses workgroups.  The
// index written is an element the workgroup read, i.e. in [0, V), whatever the input: if no comparison keeps an element (NaN
// scores), the row maximum by key is written.
#include "common.h"
#include "kernels.h"
#include "row_frame.h"

namespace s2vt {

__device__ __forceinline__ uint32_t tr_key(float x) {          // order-preserving: a < b  <=>  key(a) < key(b)
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Block sum of a 256-thread workgroup through four of the caller's 2 x 4 LDS words: wave butterfly, the four waves in the order
// (w0 + w1) + (w2 + w3).  Consecutive calls alternate `set`: a wave that already writes set 1 cannot overtake a reader of set 0,
// because the barrier of the call in between lies behind that read - ONE barrier per reduction.
template <typename T>
__device__ __forceinline__ T tr_block_sum(T v, T* red, int set) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    T* r = red + 4 * set;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// g of vocabulary index v, batch row `row`: gumbel4's mapping (block v / 4, word v % 4) for ONE element - a thread's elements are
// 256 apart, no two share a block.  Not inlined: the draw walks up to 64 register slots, and 64 inlined copies of the ten Philox
// rounds and three logarithms made the register forms spill; only kept elements call it.
__device__ __noinline__ float tr_noise(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t row, uint32_t v) {
    const Philox4 r = philox4x32_10(v >> 2, row, step, GUMBEL_STREAM_TAG, seed_lo, seed_hi);
    return gumbel_from_bits((v & 2) ? ((v & 1) ? r.w[3] : r.w[2]) : ((v & 1) ? r.w[1] : r.w[0]));
}

struct TruncArgs {
    const float* logits; int64_t ld; int V;
    int top_k;                       // 0: off
    float top_p;                     // >= 1: off
    unsigned long long* packed;      // [rows]
    int32_t* kept;                   // [rows] or null
};

// The body of both row kernels below: steps 1-5 of the truncated draw on the row the workgroup owns.
template <class Row>
__device__ __forceinline__ void truncated_draw_row(const TruncArgs& p, const GumbelArgs& ga) {
    __shared__ float red_f[8];
    __shared__ int red_i[8];
    __shared__ unsigned long long red_w[4];
    const int V = p.V;
    Row row;
    row.load_max(p.logits + (int64_t)blockIdx.x * p.ld, V);
    // 1. scores (-0 -> +0: equal values have equal keys) and the row maximum.  A register form's pad slots (i >= V) become the
    // NaN of key 0: below every candidate threshold (those are >= 1), so the passes that follow need no i < V guard (row_frame.h)
    float m = -INFINITY;
    row.slots(V, [&](int, int i, float& v) {
        float s = v * ga.inv_temperature;
        if (s == 0.f) s = 0.f;
        v = i < V ? s : __uint_as_float(0xFFFFFFFFu);
        m = fmaxf(m, v);                                   // (fmaxf returns the number where one operand is NaN)
    });
    m = block_max_256<false>(m, red_f);
    __syncthreads();                                       // (red_f is reused by the sums below)
    int set = 0;
    // 2. top-k: the largest key T with #{key >= T} >= k is the k-th largest key
    uint32_t tau = 1u;                                     // (every score but a pad or a negative NaN)
    if (p.top_k > 0 && p.top_k < V) {
        uint32_t kth = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = kth | (1u << bit);
            int c = 0;
            row.slots(V, [&](int, int, float& v) { c += tr_key(v) >= cand ? 1 : 0; });
            if (tr_block_sum(c, red_i, set) >= p.top_k) kth = cand;
            set ^= 1;
        }
        tau = kth > tau ? kth : tau;
    }
    // 3. nucleus over the survivors: the smallest key T with A(T) < p * Z, as 1 + the largest key with A >= p * Z
    uint32_t thr = tau;
    if (p.top_p < 1.f) {
        constexpr int NE = Row::SLOTS > 0 ? Row::SLOTS : 1;
        float e[NE];
        auto mass = [&](int slot, float v) -> float {
            if constexpr (Row::SLOTS > 0) return e[slot];
            else return tr_key(v) >= tau ? expf(v - m) : 0.f;
        };
        float z = 0.f;
        row.slots(V, [&](int slot, int, float& v) {
            const float ev = tr_key(v) >= tau ? expf(v - m) : 0.f;
            if constexpr (Row::SLOTS > 0) e[slot] = ev;
            z += ev;
        });
        const float pz = p.top_p * tr_block_sum(z, red_f, set);
        set ^= 1;
        uint32_t below = 0u;                               // (A(0) = Z >= p * Z: the predicate is false at key 0)
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = below | (1u << bit);
            float a = 0.f;
            row.slots(V, [&](int slot, int, float& v) { a += tr_key(v) > cand ? mass(slot, v) : 0.f; });
            if (!(tr_block_sum(a, red_f, set) < pz)) below = cand;
            set ^= 1;
        }
        const uint32_t t = below == 0xFFFFFFFFu ? below : below + 1u;
        thr = t > tau ? t : tau;
    }
    // 4. the draw over the kept elements; `all` (the row maximum by key, lowest index) stands in when nothing is kept
    unsigned long long best = 0ull, all = 0ull;
    int nkept = 0;
    row.slots(V, [&](int, int i, float& v) {
        const unsigned long long low = (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
        const unsigned long long wa = i < V ? ((unsigned long long)tr_key(v) << 32) | low : 0ull;
        all = wa > all ? wa : all;
        if (tr_key(v) >= thr) {                            // (thr >= 1: never a pad)
            ++nkept;
            const float g = tr_noise(ga.seed_lo, ga.seed_hi, ga.step, ga.row0 + blockIdx.x, (uint32_t)i);
            const unsigned long long w = ((unsigned long long)tr_key(v + g) << 32) | low;
            best = w > best ? w : best;
        }
    });
    nkept = tr_block_sum(nkept, red_i, set);
    if (nkept == 0) best = all;                            // (block-uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) red_w[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long w = red_w[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) w = red_w[k] > w ? red_w[k] : w;
        p.packed[blockIdx.x] = w;
        if (p.kept) p.kept[blockIdx.x] = nkept;
    }
}

template <class Row>
__global__ __launch_bounds__(256) void truncated_draw_kernel(TruncArgs p, GumbelArgs ga) {
    truncated_draw_row<Row>(p, ga);
}

// ---- the constrained draw (include/s2vt_hip.h "constrained draw"; sampling.constrain_logits restates it in numpy): repetition
// penalty, no-repeat n-gram blocking, banned ids and a minimum length, applied to the RAW logits row IN PLACE in global memory in
// front of the load - the same launch, the same workgroup per row; then either the truncated draw above on the edited row or the
// plain arg-max (GREEDY: no noise, no bisection).  The row's history h[0..t) comes from the drivers' packed words.
// The phase itself - edit list, suffix match, one writer per distinct word, one barrier - is row_frame.h's constrain_row, shared
// with the constrained top-20 fan-out of ce.hip; here it reads the history through PackedHist.
// LDS: 1057 * 5 bytes of the phase + 96 of the draw - beside LdsRow's 150 KiB inside the 160 KiB of a workgroup.

template <class Row>
__device__ __forceinline__ void greedy_pick_row(const TruncArgs& p) {
    __shared__ unsigned long long red_g[4];
    const int V = p.V;
    Row row;
    row.load_max(p.logits + (int64_t)blockIdx.x * p.ld, V);
    unsigned long long best = 0ull;
    row.each(V, [&](int, int i, float& v) {
        float s = v;
        if (s == 0.f) s = 0.f;                             // (-0 -> +0: equal values have equal keys, the lowest index wins)
        const unsigned long long w = ((unsigned long long)tr_key(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
        best = w > best ? w : best;
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) red_g[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long w = red_g[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) w = red_g[k] > w ? red_g[k] : w;
        p.packed[blockIdx.x] = w;
        if (p.kept) p.kept[blockIdx.x] = V;
    }
}

template <class Row, bool GREEDY>
__global__ __launch_bounds__(256) void constrained_draw_kernel(TruncArgs p, GumbelArgs ga, ConstrainArgs c, float* x_rows) {
    constrain_row(c, PackedHist{c.hist, c.hist_ld}, x_rows + (int64_t)blockIdx.x * p.ld, p.V);
    if constexpr (GREEDY) greedy_pick_row<Row>(p);
    else truncated_draw_row<Row>(p, ga);
}

template <bool GREEDY>
static int constrained_launch(hipStream_t s, const TruncArgs& a, const GumbelArgs& ga, const ConstrainArgs& c, float* x, int64_t rows) {
    const int V = a.V;
    const dim3 grid((unsigned)rows), block(256);
    const size_t lds = (size_t)V * sizeof(float);          // (the LDS form's dynamic LDS)
    if (V <= 256 * 16) hipLaunchKernelGGL((constrained_draw_kernel<RegRow<16>, GREEDY>), grid, block, 0, s, a, ga, c, x);
    else if (V <= 256 * 32) hipLaunchKernelGGL((constrained_draw_kernel<RegRow<32>, GREEDY>), grid, block, 0, s, a, ga, c, x);
    else if (V <= 256 * 48) hipLaunchKernelGGL((constrained_draw_kernel<RegRow<48>, GREEDY>), grid, block, 0, s, a, ga, c, x);
    else if (V <= 256 * 64) hipLaunchKernelGGL((constrained_draw_kernel<RegRow<64>, GREEDY>), grid, block, 0, s, a, ga, c, x);
    else {
        if (lds > 48 * 1024)
            S2VT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(constrained_draw_kernel<LdsRow, GREEDY>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((constrained_draw_kernel<LdsRow, GREEDY>), grid, block, lds, s, a, ga, c, x);
    }
    S2VT_LAUNCH_CHECK("constrained_draw_kernel");
    return 0;
}

int constrained_draw(hipStream_t s, float* logits, int64_t ld, int64_t rows, int V, const ConstrainArgs& c, bool greedy, int top_k,
                     float top_p, const GumbelArgs& ga, unsigned long long* packed, int32_t* kept) {
    if (rows <= 0) return 0;
    S2VT_REQUIRE(logits && packed && V > 0 && ld >= V && rows < (1ll << 31), "constrained_draw: bad arguments");
    S2VT_REQUIRE((size_t)V * sizeof(float) <= 150 * 1024, "constrained_draw: vocab_size <= 38400");
    S2VT_REQUIRE(truncation_ok(top_k, top_p, V), "constrained_draw: top_k in [0, V], top_p in (0, 1]");
    S2VT_REQUIRE(c.t >= 0 && c.t <= CONSTRAIN_MAX_T && c.n_banned >= 0 && c.n_banned <= CONSTRAIN_MAX_BANNED && c.ngram >= 0 &&
                     c.eos < V && (c.t == 0 || (c.hist && c.hist_ld >= rows)),
                 "constrained_draw: bad constraints");
    for (int i = 0; i < c.n_banned; ++i) S2VT_REQUIRE(c.banned[i] >= 0 && c.banned[i] < V, "constrained_draw: banned id outside [0, V)");
    const TruncArgs a{logits, ld, V, top_k, top_p, packed, kept};
    return greedy ? constrained_launch<true>(s, a, ga, c, logits, rows) : constrained_launch<false>(s, a, ga, c, logits, rows);
}

bool truncation_ok(int top_k, float top_p, int V) { return top_k >= 0 && top_k <= V && top_p > 0.f && top_p <= 1.f; }

int truncated_draw(hipStream_t s, const float* logits, int64_t ld, int64_t rows, int V, int top_k, float top_p, const GumbelArgs& ga,
                   unsigned long long* packed, int32_t* kept) {
    if (rows <= 0) return 0;
    S2VT_REQUIRE(logits && packed && V > 0 && ld >= V && rows < (1ll << 31), "truncated_draw: bad arguments");
    S2VT_REQUIRE((size_t)V * sizeof(float) <= 150 * 1024, "truncated_draw: vocab_size <= 38400");
    S2VT_REQUIRE(truncation_ok(top_k, top_p, V), "truncated_draw: top_k in [0, V], top_p in (0, 1]");
    const TruncArgs a{logits, ld, V, top_k, top_p, packed, kept};
    const dim3 grid((unsigned)rows), block(256);
    const size_t lds = (size_t)V * sizeof(float);          // (the LDS form's dynamic LDS)
    if (V <= 256 * 16) hipLaunchKernelGGL(truncated_draw_kernel<RegRow<16>>, grid, block, 0, s, a, ga);
    else if (V <= 256 * 32) hipLaunchKernelGGL(truncated_draw_kernel<RegRow<32>>, grid, block, 0, s, a, ga);
    else if (V <= 256 * 48) hipLaunchKernelGGL(truncated_draw_kernel<RegRow<48>>, grid, block, 0, s, a, ga);
    else if (V <= 256 * 64) hipLaunchKernelGGL(truncated_draw_kernel<RegRow<64>>, grid, block, 0, s, a, ga);
    else {
        if (lds > 48 * 1024)
            S2VT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(truncated_draw_kernel<LdsRow>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(truncated_draw_kernel<LdsRow>, grid, block, lds, s, a, ga);
    }
    S2VT_LAUNCH_CHECK("truncated_draw_kernel");
    return 0;
}

}  // namespace s2vt
