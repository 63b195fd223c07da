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
#include "step_frame.h"

namespace s2vt {

constexpr int NW_CHAIN = 8;      // waves per workgroup (K split), as the one-layer kernels

// ------------------------------------------------------------------------------ forward diagonal
template <int MT, bool VEC>
__device__ __forceinline__ void chain_fwd_body(const ChainFwdStep& p, int B, int H, int bid) {
    constexpr int NT = 2;
    constexpr int TM = 16 * MT, TN = 16 * NT, UN = TN / 4;
    constexpr int NWAVE = NW_CHAIN;
    constexpr int NA = (MT * NT == 1) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(MT, NT, NWAVE)];
    StepTile t;
    if (!step_tile<MT, NT, NWAVE, UN>(t, smem, H, B, bid)) return;
    const int ebl = t.ebl, eu = t.ecl, eb = t.eb, eunit = t.ecol;
    const bool evalid = t.evalid;
    f32x4 acc[MT][NT][NA];
    zero_acc(acc);

    // epilogue operands requested ahead of the K loop (one output cell per thread)
    float gxv[4], cpv, mv;
    {
        const float* gsrc = p.gx ? p.gx + (int64_t)eb * 4 * H : p.bias;
#pragma unroll
        for (int g = 0; g < 4; ++g) gxv[g] = *(evalid ? gsrc + (int64_t)g * H + eunit : g_zero4);
        cpv = *((evalid && p.c_prev) ? p.c_prev + (int64_t)eb * H + eunit : g_zero4);
        mv = *((evalid && p.mask) ? p.mask + (int64_t)eb * H + eunit : g_zero4);
    }

    // recurrent segment h_{t-1} · W_hh^T, dense input segment x_t · W_in^T (the layer below's output at the same step),
    // token segment Emb[tok] · W_e^T (greedy decode)
    if (p.h_prev) segment_gate_major<VEC, NWAVE, UN>(acc, t, p.h_prev, DenseRows{p.h_prev, H}, B, p.w_hh, H, H, H);
    if (p.x) segment_gate_major<VEC, NWAVE, UN>(acc, t, p.x, DenseRows{p.x, H}, B, p.w_in, p.ldw_in, H, H);
    if (p.emb)
        segment_gate_major<VEC, NWAVE, UN>(acc, t, p.emb, [&](int b) { return p.emb + token_of(p.tok, b) * p.E; }, B, p.w_e, p.ldw_e, H, p.E);

    constexpr int RLD = TN + 8;      // conflict-free epilogue reads (see lstm.hip)
    static_assert(UN == 8 && NWAVE * TM * RLD <= step_lds_floats(MT, NT, NWAVE), "partial tiles fit the staging area");
    reduce_partials<RLD>(acc, t);

    if (evalid) {
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = read_sum<MT, NT, NWAVE, RLD>(t.red, ebl, g * UN + eu) + gxv[g];
        const LstmCell k = lstm_cell(pre, cpv);
        const int64_t o = (int64_t)eb * H + eunit;
        p.h_out[o] = k.h;
        p.c_out[o] = k.c;
        if (p.hm_out) p.hm_out[o] = mv * k.h;
        if (p.stash) {
            float* st = p.stash + (int64_t)eb * 4 * H + eunit;
            st[0] = k.i;
            st[(int64_t)H] = k.f;
            st[(int64_t)2 * H] = k.g;
            st[(int64_t)3 * H] = k.o;
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
                     (!s.emb || (s.w_e && s.E > 0 && s.tok.tok_limit > 0)), "lstm_chain_fwd: bad layer-step");
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
    constexpr int TN = 16 * NT;
    constexpr int NWAVE = NW_CHAIN;
    constexpr int NA = 2;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(MT, NT, NWAVE)];
    StepTile t;
    if (!step_tile<MT, NT, NWAVE, TN>(t, smem, H, B, bid)) return;
    const int eb = t.eb, eunit = t.ecol;
    const bool evalid = t.evalid;
    f32x4 acc[MT][NT][NA];
    zero_acc(acc);

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

    const int64_t H4 = 4 * (int64_t)H;
    if (p.dg_up) {      // m ⊙ (dG^{up}_t · W_in^{up}): first, so that the mask scales this segment alone
        segment_plain<VEC, NWAVE>(acc, t, p.dg_up, DenseRows{p.dg_up, H4}, B, p.w_in_t, H4, H, 4 * H);
        if (p.mask) {   // 16x16 C layout: col = lane & 15, row = 4 (lane >> 4) + r
            const int col = t.n0 + (t.lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t.b0 + 4 * (t.lane >> 4) + r;
                const float m = *((row < B && col < H) ? p.mask + (int64_t)row * H + col : g_zero4);
                acc[0][0][0][r] *= m;
                acc[0][0][1][r] *= m;
            }
        }
    }
    if (p.dg_next) segment_plain<VEC, NWAVE>(acc, t, p.dg_next, DenseRows{p.dg_next, H4}, B, p.w_hh_t, H4, H, 4 * H);   // dG_{t+1} · W_hh
    reduce_partials(acc, t);

    if (evalid) {
        const float dh = read_sum<MT, NT, NWAVE>(t.red, t.ebl, t.ecl) + dhv;
        const LstmCellGrad d = lstm_cell_grad(dh, stv, cv, cpv, dcv);
        float* dg = p.dg + (int64_t)eb * 4 * H + eunit;
#pragma unroll
        for (int g = 0; g < 4; ++g) dg[(int64_t)g * H] = d.dg[g];
        p.dc[(int64_t)eb * H + eunit] = d.dc_prev;
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
