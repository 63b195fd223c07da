// What the device-side beam policy (beam_policy.hip) is built from: the fan-out of the depth step, the width limit and the
// 64-bit keyed wave-wide max that selects candidates with the tie rule in one reduction.
#pragma once

#include "common.h"

namespace s2vt {

constexpr int BC_FAN = 20;          // tokens per row that s2vt_beam_step returns (top20_logprob, ce.hip)
constexpr int BC_MAXBW = 8;
constexpr int BC_CPL = (BC_MAXBW * BC_FAN + 63) / 64;       // candidates per lane

// fp32 -> uint32 whose unsigned order is the float order (no NaN reaches it: fminf(lp, 0) maps a NaN log-prob to 0)
__device__ __forceinline__ unsigned int bc_ordered(float x) {
    const unsigned int u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bc_unordered(unsigned int o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ unsigned long long bc_wave_max(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const unsigned int hi = (unsigned int)__shfl_xor((int)(v >> 32), o), lo = (unsigned int)__shfl_xor((int)(unsigned int)v, o);
        const unsigned long long ov = ((unsigned long long)hi << 32) | lo;
        v = ov > v ? ov : v;
    }
    return v;
}


// ---- the stochastic beam's selection (sbs_policy.hip): candidates carry an fp64 score, which the 64-bit keyed max above has no room
// for beside the candidate index.  fp64 -> uint64 whose unsigned order is the double order (-0 folded to +0 first: one score; no NaN
// reaches it), 0 reserved for "no candidate" (the image of -inf is 0x000F...F + 1 > 0), and a wave-wide max over the PAIR (key, c):
// the larger key wins, equal keys -> the lower c.  Three shuffles per butterfly step; every lane ends with the winner.
__device__ __forceinline__ unsigned long long bc_ordered64(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x == 0.0 ? 0.0 : x);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ void bc_wave_max_f64c(unsigned long long& key, int& c) {
    for (int o = 32; o; o >>= 1) {
        const unsigned int hi = (unsigned int)__shfl_xor((int)(key >> 32), o), lo = (unsigned int)__shfl_xor((int)(unsigned int)key, o);
        const int oc = __shfl_xor(c, o);
        const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
        if (ok > key || (ok == key && oc < c)) { key = ok; c = oc; }
    }
}

}  // namespace s2vt
