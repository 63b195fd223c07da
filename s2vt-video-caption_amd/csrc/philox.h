// Counter-based Gumbel noise of the sampled decode (mode='sample'): Philox4x32-10 (Salmon et al., "Parallel random numbers:
// as easy as 1, 2, 3", SC'11) in plain 32-bit integer arithmetic, and the map from one 32-bit word to one standard Gumbel
// draw.  Stated once here for the device; sampling.py restates it in numpy (what the tests compare against).
//
// One draw per (call seed, decode step, batch row, vocabulary index v):
//     key     = (seed & 0xFFFFFFFF, seed >> 32)
//     counter = (v / 4, batch row, decode step, GUMBEL_STREAM_TAG)
//     x       = word v % 4 of philox4x32_10(counter, key)
//     u       = ((x >> 9) + 0.5) * 2^-23            exact in fp32, strictly inside (0, 1)
//     g       = -log(-log(u))                        in [-2.82, 16.64]
// Nothing of a kernel's tiling, of the batch padding or of the launch enters: an element has the same noise wherever it is
// computed.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace s2vt {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl key increments
constexpr uint32_t GUMBEL_STREAM_TAG = 0x47554D42u;                       // "GUMB": counter word 3 of the sampler's stream
constexpr uint32_t SS_STREAM_TAG = 0x53534D58u;                           // "SSMX": counter word 3 of the scheduled-sampling coins

struct GumbelArgs {                  // what a sampling launch adds to its greedy sibling's arguments
    float inv_temperature;           // score = logit * inv_temperature + g
    uint32_t seed_lo, seed_hi;
    uint32_t step;                   // decode step of the launch
    uint32_t row0;                   // batch row of the launch's row 0 (a launch over one half of the batch)
    uint32_t rows;                   // rows of the caller's batch: rows past it (batch padding of the plane path) generate no noise
};

struct Philox4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0;
        c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// One standard Gumbel draw from one 32-bit word.  t = -log(u) is taken from 1 - u (exact: both are multiples of 2^-24) with
// log1p where u is next to 1 - there log(u) itself would lose every digit of the small result, and g = -log(t) depends on its
// RELATIVE error.  logf / log1pf are the accurate library functions (about 1 ulp), not the fast-math intrinsics: |g| reaches
// 16.6 where one fp32 ulp is 1.9e-6, and the tests hold the device to 2 ulp of the float64 value there.
__device__ __forceinline__ float gumbel_from_bits(uint32_t x) {
    const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
    const float t = (u > 0.5f) ? -log1pf(-(1.0f - u)) : -logf(u);
    return -logf(t);
}

// the four draws of vocabulary indices 4 * v4 .. 4 * v4 + 3 of batch row `row`
__device__ __forceinline__ void gumbel4(const GumbelArgs& a, uint32_t v4, uint32_t row, float g[4]) {
    const Philox4 r = philox4x32_10(v4, row, a.step, GUMBEL_STREAM_TAG, a.seed_lo, a.seed_hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = gumbel_from_bits(r.w[e]);
}

// ---- scheduled sampling (S2VT.forward(mode='train', ss_prob > 0)): the coin that decides, per batch row and decode step,
// whether the step is fed the model's own previous draw or the ground-truth word.
//     coin(b, j) = ((x >> 9) + 0.5) * 2^-23,  x = word 0 of philox4x32_10(counter = (0, b, j, SS_STREAM_TAG), key = seed halves)
// exact in fp32 and strictly inside (0, 1): compared in fp32 with p, p = 0 never and p = 1 always takes the model's word.
// b is the row of the CALLER's batch (row0 + the launch's row); padding, tiles and schedules do not enter.
struct SsArgs {                      // what a scheduled-sampling launch adds to a token step's arguments (forced == null: absent)
    const int64_t* forced;           // ground-truth words, row 0 = the launch's row 0: row b, step j at forced[b * ld + j]
    int64_t ld;
    float p;                         // probability of taking the model's word
    uint32_t seed_lo, seed_hi;
    uint32_t step;                   // decode step j of the launch (step 0 has no previous draw: always the forced word)
    uint32_t row0;                   // batch row of the launch's row 0
    uint32_t rows;                   // rows of the caller's batch: rows past it (batch padding) have no forced word
};

__host__ __device__ __forceinline__ float ss_coin(uint32_t seed_lo, uint32_t seed_hi, uint32_t row, uint32_t step) {
    const Philox4 r = philox4x32_10(0u, row, step, SS_STREAM_TAG, seed_lo, seed_hi);
    return ((float)(r.w[0] >> 9) + 0.5f) * 0x1p-23f;
}

// token index of a packed arg-max word (ordered score << 32 | 0xFFFFFFFF - index)
__host__ __device__ __forceinline__ int64_t packed_token(unsigned long long w) {
    return (int64_t)(0xFFFFFFFFu - (uint32_t)(w & 0xFFFFFFFFull));
}

// The token a scheduled step feeds row b of its launch: `packed` = the previous step's packed words of the launch's rows (null
// at step 0).  *has = false for a padding row (the caller keeps its own rule there).
__host__ __device__ __forceinline__ int64_t ss_token(const SsArgs& s, const unsigned long long* packed, int b, bool* has) {
    const uint32_t row = s.row0 + (uint32_t)b;
    *has = row < s.rows;
    if (!*has) return 0;
    if (packed && s.step > 0 && ss_coin(s.seed_lo, s.seed_hi, row, s.step) < s.p) return packed_token(packed[b]);
    return s.forced[(int64_t)b * s.ld + s.step];
}

// ---- where a token step (an embedding K segment or a per-token gate-input table: lstm.hip, lstm_gemv.hip, gru.hip,
// lstm_stack.hip) takes the word of batch row b from
struct TokenSrc {
    const int32_t* tok_idx;                  // int32 token per batch row, or
    const unsigned long long* tok_packed;    // packed argmax word of the previous decode step, or
    int tok_const;                           // one token for every row (<sos>); used when both null
    // guard of the token path (tok_idx / tok_packed / tok_const): an id outside [0, tok_limit) is read as token 0 and raises
    // *tok_err (the S2VT_ERR_INDEX flag word of the caller's workspace) instead of addressing memory outside the table - a
    // producer bug (e.g. a packed argmax word that no workgroup wrote) then surfaces as an error code, not as a GPU fault.
    // tok_limit == 0: no token segment in use
    int tok_limit; int* tok_err;
    // optional (scheduled sampling): with ss.forced the token of row b is the packed word only where the row's coin falls below
    // ss.p, the forced ground-truth id otherwise; tok_idx is then not read.  Same guard for a forced id.
    SsArgs ss;
};

// the token of row b of the launch (b inside the launch's batch: the caller guards)
__host__ __device__ __forceinline__ int64_t token_of(const TokenSrc& s, int b) {
    int64_t tok = s.tok_const;
    bool forced = false;
    if (s.ss.forced) {       // (wave-uniform: a kernel argument)
        const int64_t t = ss_token(s.ss, s.tok_packed, b, &forced);
        if (forced) tok = t;
    }
    if (!forced) {
        if (s.tok_idx) tok = s.tok_idx[b];
        else if (s.tok_packed) tok = packed_token(s.tok_packed[b]);
    }
    if ((uint64_t)tok >= (uint64_t)(int64_t)s.tok_limit) {
        if (s.tok_err) *s.tok_err = 1;
        tok = 0;
    }
    return tok;
}

}  // namespace s2vt
