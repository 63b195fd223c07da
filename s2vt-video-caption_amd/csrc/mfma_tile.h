// The fp32 MFMA tile machinery of the launch-per-timestep recurrence kernels (lstm.hip, gru.hip, lstm_stack.hip, through the
// frame of step_frame.h): guarded 16-byte staging
// loads, the K-split wave contraction on v_mfma_f32_16x16x4_f32 with a register prefetch, the fixed-order reduction of the
// waves' partial tiles through LDS, and the XCD-aware workgroup placement.
#pragma once
#include "common.h"

namespace s2vt {

#ifndef S2VT_KC
#define S2VT_KC 32
#endif
constexpr int KC = S2VT_KC;      // k chunk per wave iteration (64: 256-B row segments; 32: half the LDS, one line)
constexpr int SLD = KC + 4;      // LDS row stride in floats (68 / 36: conflict-free ds_read_b128)
constexpr int LPR = KC / 4;      // lanes per staged row (one float4 each)
constexpr int RPL = 64 / LPR;    // rows covered by one wave-wide load
constexpr int LPT = 16 / RPL;    // loads per lane per 16 rows of tile
#ifndef S2VT_PF
#define S2VT_PF 2
#endif
constexpr int PF = S2VT_PF;            // staging chunks in flight per wave (register prefetch depth)

// Branch-free guarded 4-float load (see gemm.hip load4_guard): out-of-range accesses read a safe address and
// are zeroed by a select, so the staging burst stays a run of independent loads.
template <bool VEC>
__device__ __forceinline__ f32x4 ld4(const float* base, const float* row, int c, int limit) {
    // Out-of-range accesses read a 16-byte block of zeros instead of being masked afterwards: the loaded value
    // then has NO consumer before the LDS staging store, so the loads stay in flight across the MFMA phase
    // (a select on the result would pull the vmcnt wait in front of the MFMAs).
    f32x4 v;
    if (VEC) {
        const bool ok = (row != nullptr) && (c < limit);
        const float* q = ok ? row + c : g_zero4;
        v = *reinterpret_cast<const f32x4*>(q);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool ok = (row != nullptr) && (c + j < limit);
            const float* q = ok ? row + c + j : g_zero4;
            v[j] = *q;
        }
    }
    return v;
}

// acc[mi][ni][a] += A[16*MT rows, 0:K] · B[16*NT rows, 0:K]^T over this wave's chunks (NPF chunks in flight per wave).
// arow/brow: per-lane row pointers for rows (lane/16 + 4 i); sA/sB: wave-private LDS images.
template <int MT, int NT, int NA, bool VEC, int NWAVE, int NPF = PF>
__device__ __forceinline__ void wave_gemm_nt(f32x4 (&acc)[MT][NT][NA], const float* abase, const float* bbase,
                                             const float* const (&arow)[MT * LPT], const float* const (&brow)[NT * LPT],
                                             int K, float* sA, float* sB, int wave, int lane) {
    // Wave w owns chunks w, w+NWAVE, ...; NPF of them are in flight (registers) at any time.  Loads are issued
    // unconditionally (chunks past K read the zero block), so the body is straight-line code and the compiler's
    // counted vmcnt leaves the younger chunks in flight while the oldest is staged and multiplied.
    const int nch = (K + KC - 1) / KC;
    const int per_wave = (nch + NWAVE - 1) / NWAVE;
    const int n_round = (per_wave + NPF - 1) / NPF;
    const int lrow = lane / LPR, kq = (lane % LPR) * 4;
    const int fi = lane & 15, fq = lane >> 4;
    f32x4 ra[NPF][MT * LPT], rb[NPF][NT * LPT];
#pragma unroll
    for (int d = 0; d < NPF; ++d) {
        const int k0 = (wave + d * NWAVE) * KC + kq;
#pragma unroll
        for (int i = 0; i < MT * LPT; ++i) ra[d][i] = ld4<VEC>(abase, arow[i], k0, K);
#pragma unroll
        for (int i = 0; i < NT * LPT; ++i) rb[d][i] = ld4<VEC>(bbase, brow[i], k0, K);
    }
    for (int r = 0; r < n_round; ++r) {
#pragma unroll
        for (int d = 0; d < NPF; ++d) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int i = 0; i < MT * LPT; ++i) *reinterpret_cast<f32x4*>(&sA[(lrow + RPL * i) * SLD + kq]) = ra[d][i];
#pragma unroll
            for (int i = 0; i < NT * LPT; ++i) *reinterpret_cast<f32x4*>(&sB[(lrow + RPL * i) * SLD + kq]) = rb[d][i];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            {   // refill this stage with the chunk NPF rounds ahead
                const int k0 = (wave + ((r + 1) * NPF + d) * NWAVE) * KC + kq;
#pragma unroll
                for (int i = 0; i < MT * LPT; ++i) ra[d][i] = ld4<VEC>(abase, arow[i], k0, K);
#pragma unroll
                for (int i = 0; i < NT * LPT; ++i) rb[d][i] = ld4<VEC>(bbase, brow[i], k0, K);
            }
#pragma unroll
            for (int s = 0; s < KC / 16; ++s) {
                f32x4 a[MT], b[NT];
#pragma unroll
                for (int mi = 0; mi < MT; ++mi)
                    a[mi] = *reinterpret_cast<const f32x4*>(&sA[(mi * 16 + fi) * SLD + 16 * s + 4 * fq]);
#pragma unroll
                for (int ni = 0; ni < NT; ++ni)
                    b[ni] = *reinterpret_cast<const f32x4*>(&sB[(ni * 16 + fi) * SLD + 16 * s + 4 * fq]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NT; ++ni)
                            acc[mi][ni][j & (NA - 1)] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                a[mi][j], b[ni][j], acc[mi][ni][j & (NA - 1)], 0, 0, 0);
            }
        }
    }
}

// Sum the NWAVE waves' partial tiles: every wave writes its accumulators to red[wave][row][col],
// after which red holds 4 partials per output.  16x16 C/D layout: col = lane&15, row = 4*(lane>>4)+reg.
// RLD = row stride of the partial tiles in floats, chosen per kernel so that the EPILOGUE's read pattern is free of bank
// conflicts (ds_read_b32: 32 banks, conflicts counted per 32-lane half).
template <int MT, int NT, int NA, int RLD = 16 * NT + 1>
__device__ __forceinline__ void write_partials(const f32x4 (&acc)[MT][NT][NA], float* red, int wave, int lane) {
    constexpr int TM = 16 * MT;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[mi][ni][0][r];
                if (NA == 2) v += acc[mi][ni][NA - 1][r];
                red[(wave * TM + mi * 16 + 4 * (lane >> 4) + r) * RLD + ni * 16 + (lane & 15)] = v;
            }
}

template <int MT, int NT, int NWAVE, int RLD = 16 * NT + 1>
__device__ __forceinline__ float read_sum(const float* red, int row, int col) {
    constexpr int TM = 16 * MT;
    float s = red[row * RLD + col];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) s += red[(w * TM + row) * RLD + col];
    return s;
}

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the XCD group).  All NY batch tiles of
// one column tile read the same weight slice, so they are given ids that differ by a multiple of 8: the slice
// is then fetched into ONE XCD's L2 (16 MB of W_hh / 8 XCDs = 2 MB per 4 MB L2) instead of NY of them.
// Speed only: any placement is correct.  Grid = ceil(NX/8)*8*NY blocks; ids with x >= NX exit.
__device__ __forceinline__ bool xcd_tile(int NX, int NY, int& x, int& y, int id = -1) {
    if (id < 0) id = blockIdx.x;
    const int xcd = id & 7, j = id >> 3;
    x = (j / NY) * 8 + xcd;
    y = j % NY;
    return x < NX;
}
static inline int xcd_grid(int NX, int NY) { return ((NX + 7) / 8) * 8 * NY; }

static inline bool vec_ok(const void* ptr, int64_t ld) {
    return ptr != nullptr && (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(ptr) & 15) == 0);
}

}  // namespace s2vt
