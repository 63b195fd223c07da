// Layer-wavefront kernels of a stacked LSTM chain (S2VT with num_layers > 1) for gfx950.
//
// A stacked S2VT is one chain of layers in which layer j at step t reads the output of layer j-1 at the same t.  Launch d of
// the forward runs every layer-step (j, t = d - j) at once: they are independent, so a chain of n layers over T steps takes
// T + n - 1 launches instead of n * T.  The backward runs the mirror image, the top of the chain leading.
//
// The tiles are those of lstm.hip's timestep kernels (v_mfma_f32_16x16x4_f32 through mfma_tile.h, the whole cell in the
// epilogue); a launch holds up to CHAIN_MAX layer-steps of one (B, H), and workgroup blockIdx.x serves layer-step
// blockIdx.x / tiles, tile blockIdx.x % tiles (every layer-step has the same tile count, a multiple of 8, so the XCD
// placement of xcd_tile holds inside each).
//   forward   G = gate input (rows or bias) + x_t W_in^T + h_{t-1} W_hh^T (+ Emb[tok] W_e^T); x_t is the layer below's
//             output at t (its masked copy under dropout).  The epilogue writes h, c, the activated gates and m ⊙ h.
//   backward  dh = dh_ext + dG_{t+1} W_hh + m ⊙ (dG^{up}_t W_in^{up}); both against transposed weight copies.  The masked
//             segment runs first and its partial accumulators are scaled by the mask before the recurrent segment adds to
//             them (exact by linearity; one accumulator set).
#include "common.h"
#include "kernels.h"
#include "mfma_tile.h"

namespace s2vt {

constexpr int NW_CHAIN = 8;      // waves per workgroup (K split), as the one-layer kernels

__device__ __forceinline__ float chain_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float chain_tanh(float x) { return 1.0f - 2.0f / (1.0f + __expf(2.0f * x)); }

// ------------------------------------------------------------------------------ forward diagonal
template <int MT, bool VEC>
__device__ __forceinline__ void chain_fwd_body(const ChainFwdStep& p, int B, int H, int bid) {
    constexpr int NT = 2;
    constexpr int TM = 16 * MT, TN = 16 * NT, UN = TN / 4;
    constexpr int NWAVE = NW_CHAIN, NTHR = NWAVE * 64;
    constexpr int NA = (MT * NT == 1) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float smem[NWAVE * (TM + TN) * SLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* sA = smem + wave * (TM + TN) * SLD;
    float* sB = sA + TM * SLD;
    int tx, ty;
    if (!xcd_tile((H + UN - 1) / UN, (B + TM - 1) / TM, tx, ty, bid)) return;
    const int b0 = ty * TM, u0 = tx * UN;
    const int lrow = lane / LPR;

    f32x4 acc[MT][NT][NA];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[mi][ni][a] = f32x4{0.f, 0.f, 0.f, 0.f};

    // epilogue operands requested ahead of the K loop (one output cell per thread)
    static_assert(TM * UN <= NTHR, "one epilogue element per thread");
    const int ebl = tid / UN, eu = tid % UN;
    const int eb = b0 + ebl, eunit = u0 + eu;
    const bool evalid = (tid < TM * UN) && (eb < B) && (eunit < H);
    float gxv[4], cpv, mv;
    {
        const float* gsrc = p.gx ? p.gx + (int64_t)eb * 4 * H : p.bias;
#pragma unroll
        for (int g = 0; g < 4; ++g) gxv[g] = *(evalid ? gsrc + (int64_t)g * H + eunit : g_zero4);
        cpv = *((evalid && p.c_prev) ? p.c_prev + (int64_t)eb * H + eunit : g_zero4);
        mv = *((evalid && p.mask) ? p.mask + (int64_t)eb * H + eunit : g_zero4);
    }

    const float* arow[MT * LPT];
    const float* brow[NT * LPT];
    if (p.h_prev) {     // recurrent segment h_{t-1} · W_hh^T
#pragma unroll
        for (int i = 0; i < MT * LPT; ++i) {
            const int b = b0 + lrow + RPL * i;
            arow[i] = (b < B) ? p.h_prev + (int64_t)b * H : nullptr;
        }
#pragma unroll
        for (int i = 0; i < NT * LPT; ++i) {
            const int r = lrow + RPL * i, g = r / UN, u = u0 + r % UN;
            brow[i] = (u < H) ? p.w_hh + ((int64_t)g * H + u) * H : nullptr;
        }
        wave_gemm_nt<MT, NT, NA, VEC, NWAVE>(acc, p.h_prev, p.w_hh, arow, brow, H, sA, sB, wave, lane);
    }
    if (p.x) {          // dense input segment x_t · W_in^T (the layer below's output at the same step)
#pragma unroll
        for (int i = 0; i < MT * LPT; ++i) {
            const int b = b0 + lrow + RPL * i;
            arow[i] = (b < B) ? p.x + (int64_t)b * H : nullptr;
        }
#pragma unroll
        for (int i = 0; i < NT * LPT; ++i) {
            const int r = lrow + RPL * i, g = r / UN, u = u0 + r % UN;
            brow[i] = (u < H) ? p.w_in + ((int64_t)g * H + u) * p.ldw_in : nullptr;
        }
        wave_gemm_nt<MT, NT, NA, VEC, NWAVE>(acc, p.x, p.w_in, arow, brow, H, sA, sB, wave, lane);
    }
    if (p.emb) {        // token segment Emb[tok] · W_e^T (greedy decode); an id outside [0, tok_limit) reads row 0
#pragma unroll
        for (int i = 0; i < MT * LPT; ++i) {
            const int b = b0 + lrow + RPL * i;
            int64_t tok = p.tok_const;
            bool forced = false;
            if (b < B && p.ss.forced) {       // scheduled sampling (wave-uniform on the argument): the coin picks the word
                const int64_t t = ss_token(p.ss, p.tok_packed, b, &forced);
                if (forced) tok = t;
            }
            if (!forced && b < B && p.tok_packed) tok = (int64_t)(0xFFFFFFFFu - (uint32_t)(p.tok_packed[b] & 0xFFFFFFFFull));
            if ((uint64_t)tok >= (uint64_t)(int64_t)p.tok_limit) {
                if (p.tok_err) *p.tok_err = 1;
                tok = 0;
            }
            arow[i] = (b < B) ? p.emb + tok * p.E : nullptr;
        }
#pragma unroll
        for (int i = 0; i < NT * LPT; ++i) {
            const int r = lrow + RPL * i, g = r / UN, u = u0 + r % UN;
            brow[i] = (u < H) ? p.w_e + ((int64_t)g * H + u) * p.ldw_e : nullptr;
        }
        wave_gemm_nt<MT, NT, NA, VEC, NWAVE>(acc, p.emb, p.w_e, arow, brow, p.E, sA, sB, wave, lane);
    }

    constexpr int RLD = TN + 8;      // conflict-free epilogue reads (see lstm.hip)
    static_assert(UN == 8 && NWAVE * TM * RLD <= NWAVE * (TM + TN) * SLD, "partial tiles fit the staging area");
    __syncthreads();
    float* red = smem;
    write_partials<MT, NT, NA, RLD>(acc, red, wave, lane);
    __syncthreads();

    if (evalid) {
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = read_sum<MT, NT, NWAVE, RLD>(red, ebl, g * UN + eu) + gxv[g];
        const float ig = chain_sigmoid(pre[0]);
        const float fg = chain_sigmoid(pre[1]);
        const float gg = chain_tanh(pre[2]);
        const float og = chain_sigmoid(pre[3]);
        const float c = fg * cpv + ig * gg;
        const float h = og * chain_tanh(c);
        const int64_t o = (int64_t)eb * H + eunit;
        p.h_out[o] = h;
        p.c_out[o] = c;
        if (p.hm_out) p.hm_out[o] = mv * h;
        if (p.stash) {
            float* st = p.stash + (int64_t)eb * 4 * H + eunit;
            st[0] = ig;
            st[(int64_t)H] = fg;
            st[(int64_t)2 * H] = gg;
            st[(int64_t)3 * H] = og;
        }
    }
}

// 4 waves per SIMD at most: two 8-wave workgroups (and their LDS) share a CU
template <int MT, bool VEC>
__global__ __launch_bounds__(NW_CHAIN * 64, NW_CHAIN / 2) void lstm_chain_fwd_kernel(ChainFwdLaunch p) {
    const int s = (int)blockIdx.x / p.tiles;
    chain_fwd_body<MT, VEC>(p.s[s], p.B, p.H, (int)blockIdx.x - s * p.tiles);
}

static bool vec_rows(const float* ptr, int64_t ld) { return ptr == nullptr || vec_ok(ptr, ld); }

int lstm_chain_fwd_launch(hipStream_t stream, const ChainFwdLaunch& a) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.n > 0 && a.n <= CHAIN_MAX, "lstm_chain_fwd: bad launch");
    bool vec = a.H % 4 == 0;
    for (int i = 0; i < a.n; ++i) {
        const ChainFwdStep& s = a.s[i];
        S2VT_REQUIRE(s.h_out && s.c_out && (s.gx || s.bias) && s.w_hh && (!s.x || s.w_in) && (!s.mask || s.hm_out) &&
                     (!s.emb || (s.w_e && s.E > 0 && s.tok_limit > 0)), "lstm_chain_fwd: bad layer-step");
        vec = vec && vec_rows(s.h_prev, a.H) && vec_rows(s.w_hh, a.H) && vec_rows(s.x, a.H) && vec_rows(s.w_in, s.ldw_in) &&
              (!s.emb || (s.E % 4 == 0 && vec_ok(s.emb, s.E) && vec_ok(s.w_e, s.ldw_e)));
    }
    ChainFwdLaunch p = a;
    // 32-row tiles on the vector path only: the scalar-load form of that tile spills
    if (a.B <= 16 || !vec) {
        p.tiles = xcd_grid(cdiv(a.H, 8), cdiv(a.B, 16));
        dim3 grid((unsigned)(p.tiles * a.n));
        if (vec) hipLaunchKernelGGL((lstm_chain_fwd_kernel<1, true>), grid, dim3(NW_CHAIN * 64), 0, stream, p);
        else hipLaunchKernelGGL((lstm_chain_fwd_kernel<1, false>), grid, dim3(NW_CHAIN * 64), 0, stream, p);
    } else {
        p.tiles = xcd_grid(cdiv(a.H, 8), cdiv(a.B, 32));
        dim3 grid((unsigned)(p.tiles * a.n));
        hipLaunchKernelGGL((lstm_chain_fwd_kernel<2, true>), grid, dim3(NW_CHAIN * 64), 0, stream, p);
    }
    S2VT_LAUNCH_CHECK("lstm_chain_fwd_kernel");
    return 0;
}

// ----------------------------------------------------------------------------- backward diagonal
template <bool VEC>
__device__ __forceinline__ void chain_bwd_body(const ChainBwdStep& p, int B, int H, int bid) {
    constexpr int MT = 1, NT = 1;
    constexpr int TM = 16 * MT, TN = 16 * NT;
    constexpr int NWAVE = NW_CHAIN, NTHR = NWAVE * 64;
    constexpr int NA = 2;
    __shared__ __attribute__((aligned(16))) float smem[NWAVE * (TM + TN) * SLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* sA = smem + wave * (TM + TN) * SLD;
    float* sB = sA + TM * SLD;
    int tx, ty;
    if (!xcd_tile((H + TN - 1) / TN, (B + TM - 1) / TM, tx, ty, bid)) return;
    const int b0 = ty * TM, n0 = tx * TN;
    const int lrow = lane / LPR;

    f32x4 acc[MT][NT][NA];
    acc[0][0][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[0][0][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    static_assert(TM * TN <= NTHR, "one epilogue element per thread");
    const int ebl = tid / TN, eul = tid % TN;
    const int eb = b0 + ebl, eunit = n0 + eul;
    const bool evalid = (tid < TM * TN) && (eb < B) && (eunit < H);
    float stv[4], cv, cpv, dcv, dhv;
    {
        const int64_t o = (int64_t)eb * H + eunit;
#pragma unroll
        for (int g = 0; g < 4; ++g) stv[g] = *(evalid ? p.stash + (int64_t)eb * 4 * H + (int64_t)g * H + eunit : g_zero4);
        cv = *(evalid ? p.c + o : g_zero4);
        cpv = *((evalid && p.c_prev) ? p.c_prev + o : g_zero4);
        dcv = *(evalid ? p.dc + o : g_zero4);
        dhv = *((evalid && p.dh_ext) ? p.dh_ext + o : g_zero4);
    }

    const float* arow[LPT];
    const float* brow[LPT];
    if (p.dg_up) {      // m ⊙ (dG^{up}_t · W_in^{up}): first, so that the mask scales this segment alone
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int b = b0 + lrow + RPL * i, n = n0 + lrow + RPL * i;
            arow[i] = (b < B) ? p.dg_up + (int64_t)b * 4 * H : nullptr;
            brow[i] = (n < H) ? p.w_in_t + (int64_t)n * 4 * H : nullptr;
        }
        wave_gemm_nt<MT, NT, NA, VEC, NWAVE>(acc, p.dg_up, p.w_in_t, arow, brow, 4 * H, sA, sB, wave, lane);
        if (p.mask) {   // 16x16 C layout: col = lane & 15, row = 4 (lane >> 4) + r
            const int col = n0 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = b0 + 4 * (lane >> 4) + r;
                const float m = *((row < B && col < H) ? p.mask + (int64_t)row * H + col : g_zero4);
                acc[0][0][0][r] *= m;
                acc[0][0][1][r] *= m;
            }
        }
    }
    if (p.dg_next) {    // dG_{t+1} · W_hh
#pragma unroll
        for (int i = 0; i < LPT; ++i) {
            const int b = b0 + lrow + RPL * i, n = n0 + lrow + RPL * i;
            arow[i] = (b < B) ? p.dg_next + (int64_t)b * 4 * H : nullptr;
            brow[i] = (n < H) ? p.w_hh_t + (int64_t)n * 4 * H : nullptr;
        }
        wave_gemm_nt<MT, NT, NA, VEC, NWAVE>(acc, p.dg_next, p.w_hh_t, arow, brow, 4 * H, sA, sB, wave, lane);
    }
    __syncthreads();
    float* red = smem;
    write_partials<MT, NT, NA>(acc, red, wave, lane);
    __syncthreads();

    if (evalid) {
        const int64_t o = (int64_t)eb * H + eunit;
        const float dh = read_sum<MT, NT, NWAVE>(red, ebl, eul) + dhv;
        const float ig = stv[0], fg = stv[1], gg = stv[2], og = stv[3];
        const float tc = chain_tanh(cv);
        const float dc = dh * og * (1.0f - tc * tc) + dcv;
        const float d_o = dh * tc;
        float* dg = p.dg + (int64_t)eb * 4 * H + eunit;
        dg[0] = dc * gg * ig * (1.0f - ig);
        dg[(int64_t)H] = dc * cpv * fg * (1.0f - fg);
        dg[(int64_t)2 * H] = dc * ig * (1.0f - gg * gg);
        dg[(int64_t)3 * H] = d_o * og * (1.0f - og);
        p.dc[o] = dc * fg;
    }
}

template <bool VEC>
__global__ __launch_bounds__(NW_CHAIN * 64, NW_CHAIN / 2) void lstm_chain_bwd_kernel(ChainBwdLaunch p) {
    const int s = (int)blockIdx.x / p.tiles;
    chain_bwd_body<VEC>(p.s[s], p.B, p.H, (int)blockIdx.x - s * p.tiles);
}

int lstm_chain_bwd_launch(hipStream_t stream, const ChainBwdLaunch& a) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.n > 0 && a.n <= CHAIN_MAX, "lstm_chain_bwd: bad launch");
    bool vec = a.H % 4 == 0;
    for (int i = 0; i < a.n; ++i) {
        const ChainBwdStep& s = a.s[i];
        S2VT_REQUIRE(s.stash && s.c && s.dc && s.dg && (!s.dg_next || s.w_hh_t) && (!s.dg_up || s.w_in_t),
                     "lstm_chain_bwd: bad layer-step");
        vec = vec && vec_rows(s.dg_next, 4 * (int64_t)a.H) && vec_rows(s.w_hh_t, 4 * (int64_t)a.H) &&
              vec_rows(s.dg_up, 4 * (int64_t)a.H) && vec_rows(s.w_in_t, 4 * (int64_t)a.H);
    }
    ChainBwdLaunch p = a;
    p.tiles = xcd_grid(cdiv(a.H, 16), cdiv(a.B, 16));
    dim3 grid((unsigned)(p.tiles * a.n));
    if (vec) hipLaunchKernelGGL((lstm_chain_bwd_kernel<true>), grid, dim3(NW_CHAIN * 64), 0, stream, p);
    else hipLaunchKernelGGL((lstm_chain_bwd_kernel<false>), grid, dim3(NW_CHAIN * 64), 0, stream, p);
    S2VT_LAUNCH_CHECK("lstm_chain_bwd_kernel");
    return 0;
}

}  // namespace s2vt
