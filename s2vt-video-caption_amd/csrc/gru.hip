// Fused GRU timestep kernels (forward cell, BPTT cell) for gfx950: what nn.GRU runs per step when S2VT is built with
// rnn_type='gru' (S2VTModel.py:11-22), gate order r, z, n as in torch:
//   r = sigmoid(gx_r + h W_hr^T + b_hr)      z = sigmoid(gx_z + h W_hz^T + b_hz)
//   n = tanh(gx_n + r * (h W_hn^T + b_hn))   h' = n + z * (h - n)        (gx = x W_ih^T + b_ih)
// The scheme is lstm.hip's: one launch per timestep, the recurrent contraction on the matrix cores (v_mfma_f32_16x16x4_f32,
// exact fp32 products) with K split over the 8 waves of a workgroup and the partial tiles summed through LDS in a fixed order,
// and the whole cell in the epilogue, so no pre-activation goes to HBM.
//   forward:  a workgroup owns 16 batch rows x 16 hidden units, i.e. the 48 rows {r, z, n} x 16 units of W_hh: complete
//             cells.  b_hn stays inside the r product, so the n column tile is kept apart from the input half of the gate; the
//             token variant (greedy decode) adds Emb[tok]·W_e^T as a second K segment whose n tile is kept on its own.
//   backward: dh_t = dh_out_t + dh_{t+1} * z_{t+1} + dGh_{t+1}·W_hh (K = 3H, against W_hh^T rows), then the gate derivatives
//             dGx_t = [dr, dz, dn] (d gate input) and dGh_t = [dr, dz, dn * r] (d of h W_hh^T + b_hh), both plain [B,3H] rows:
//             the weight gradients are the row-major GEMMs dW_ih = dGx^T x, dW_hh = dGh^T h_{t-1}.
// One 16-row batch tile per workgroup at every B (guarded rows): at B = 64, H = 1000 that is 63 x 4 = 252 workgroups for the
// 256 compute units, each reading a 192 KB slice of W_hh (the four batch tiles of a slice on one XCD, xcd_tile).
#include <stdlib.h>
#include "common.h"
#include "kernels.h"
#include "step_frame.h"

namespace s2vt {

constexpr int GRU_NW = 8;            // waves per workgroup = K-split factor
constexpr int GRU_TM = 16;           // batch rows per workgroup
constexpr int GRU_UN = 16;           // hidden units per forward workgroup (3 gate tiles of 16 columns)

// ------------------------------------------------------------------------------ forward step
// (two workgroups per CU: 73.7 KB of LDS each, <= 128 VGPRs)
template <bool VEC, bool TOK>
__global__ __launch_bounds__(GRU_NW * 64, GRU_NW / 2) void gru_step_fwd_kernel(GruFwdArgs p) {
    constexpr int TM = GRU_TM, UN = GRU_UN, NT = 3, TN = 16 * NT;
    constexpr int NWAVE = GRU_NW;
    // partial tiles: 3 gate tiles (+ the n tile of the token segment); a half-wave of the epilogue reads 2 rows x 16 columns,
    // a row stride of 16 (mod 64) banks puts them on disjoint banks
    constexpr int NP = TOK ? 4 : 3, RLD = 16 * NP + 16;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(1, NT, NWAVE)];
    static_assert(NWAVE * TM * RLD <= step_lds_floats(1, NT, NWAVE), "partial tiles fit the staging area");
    StepTile t;
    if (!step_tile<1, NT, NWAVE, UN>(t, smem, p.H, p.B)) return;
    const int ebl = t.ebl, eu = t.ecl, eb = t.eb, eunit = t.ecol;
    const bool evalid = t.evalid;

    // epilogue operands (one output element per thread): requested ahead of the K loop, so that their latency hides behind the
    // contraction - except in the token variant, whose two segments leave no registers for them (loaded after the loop there)
    float gxv[3], bhv[3], hpv;
    auto load_epilogue = [&]() {
        const float* gsrc = p.gx ? p.gx + (int64_t)eb * p.ldgx : p.b_ih;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            gxv[g] = *((evalid && gsrc) ? gsrc + (int64_t)g * p.H + eunit : g_zero4);
            bhv[g] = *(evalid ? p.b_hh + (int64_t)g * p.H + eunit : g_zero4);
        }
        hpv = *((evalid && p.h_prev) ? p.h_prev + (int64_t)eb * p.ldh + eunit : g_zero4);
    };
    if (!TOK) load_epilogue();

    // the token segment (greedy decode) runs FIRST into the same accumulators; its n tile is then set aside (it stays outside
    // the r product) and the recurrent contraction continues on r and z: 4 live registers more instead of a second tile set
    // prefetch depth: the scalar-load path only serves odd shapes, and the token segment runs once per decode step - one chunk in
    // flight keeps both spill-free within the 128 registers of two workgroups per CU
    constexpr int NPF = VEC ? PF : 1;
    constexpr int NPFX = 1;
    f32x4 acc[1][NT][1];
    zero_acc(acc);
    f32x4 xn = f32x4{0.f, 0.f, 0.f, 0.f};
    if (TOK) {
        segment_gate_major<VEC, NWAVE, UN, NPFX>(acc, t, p.x2, [&](int b) { return p.x2 + token_of(p.tok, b) * p.ldx2; }, p.B, p.w2, p.ldw2, p.H, p.K2);
        xn = acc[0][2][0];
        acc[0][2][0] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (p.h_prev) segment_gate_major<VEC, NWAVE, UN, NPF>(acc, t, p.h_prev, DenseRows{p.h_prev, p.ldh}, p.B, p.w_hh, p.ldw, p.H, p.H);

    if (TOK) load_epilogue();
    if (TOK) {
        f32x4 accw[1][4][1];
        accw[0][0][0] = acc[0][0][0];
        accw[0][1][0] = acc[0][1][0];
        accw[0][2][0] = acc[0][2][0];
        accw[0][3][0] = xn;
        reduce_partials<RLD>(accw, t);
    } else {
        reduce_partials<RLD>(acc, t);
    }
    const float* red = t.red;

    if (evalid) {
        const float sr = read_sum<1, NP, NWAVE, RLD>(red, ebl, eu);
        const float sz = read_sum<1, NP, NWAVE, RLD>(red, ebl, UN + eu);
        const float sn = read_sum<1, NP, NWAVE, RLD>(red, ebl, 2 * UN + eu);
        const float sx = TOK ? read_sum<1, NP, NWAVE, RLD>(red, ebl, 3 * UN + eu) : 0.f;
        const float r = sigmoidf_(gxv[0] + (sr + bhv[0]));
        const float z = sigmoidf_(gxv[1] + (sz + bhv[1]));
        const float ghn = sn + bhv[2];
        const float n = tanhf_((gxv[2] + sx) + r * ghn);
        const float h = n + z * (hpv - n);
        p.h_out[(int64_t)eb * p.ldho + eunit] = h;
        if (p.stash) {
            float* st = p.stash + (int64_t)eb * p.ldst + eunit;
            st[0] = r;
            st[(int64_t)p.H] = z;
            st[(int64_t)2 * p.H] = n;
            st[(int64_t)3 * p.H] = ghn;
        }
    }
}

int gru_step_fwd(hipStream_t stream, const GruFwdArgs& a) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.w_hh && a.b_hh && a.h_out && (a.gx || a.b_ih), "gru_step_fwd: bad arguments");
    S2VT_REQUIRE(a.ldh >= a.H && a.ldw >= a.H && a.ldho >= a.H && (!a.gx || a.ldgx >= 3 * (int64_t)a.H) &&
                 (!a.stash || a.ldst >= 4 * (int64_t)a.H), "gru_step_fwd: row stride below the row length");
    S2VT_REQUIRE(!a.x2 || (a.w2 && a.K2 > 0 && a.ldx2 >= a.K2 && a.ldw2 >= a.K2 && a.tok.tok_limit > 0),
                 "gru_step_fwd: a token segment needs W_e, K2 and tok_limit (rows of the table)");
    const bool vec = (!a.h_prev || (vec_ok(a.h_prev, a.ldh) && vec_ok(a.w_hh, a.ldw) && a.H % 4 == 0)) &&
                     (!a.x2 || (vec_ok(a.x2, a.ldx2) && vec_ok(a.w2, a.ldw2) && a.K2 % 4 == 0));
    const dim3 grid(xcd_grid(cdiv(a.H, GRU_UN), cdiv(a.B, GRU_TM))), block(GRU_NW * 64);
    if (a.x2) {
        if (vec) hipLaunchKernelGGL((gru_step_fwd_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((gru_step_fwd_kernel<false, true>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((gru_step_fwd_kernel<true, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((gru_step_fwd_kernel<false, false>), grid, block, 0, stream, a);
    }
    S2VT_LAUNCH_CHECK("gru_step_fwd_kernel");
    return 0;
}

// ----------------------------------------------------------------------------- backward step
template <bool VEC>
__global__ __launch_bounds__(GRU_NW * 64) void gru_step_bwd_kernel(GruBwdArgs p) {
    constexpr int TM = GRU_TM, TN = 16;
    constexpr int NWAVE = GRU_NW;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(1, 1, NWAVE)];
    StepTile t;
    if (!step_tile<1, 1, NWAVE, TN>(t, smem, p.H, p.B)) return;
    const int eb = t.eb, eunit = t.ecol;
    const bool evalid = t.evalid;
    const bool next = p.dgh_next != nullptr;
    float stv[4], hpv, dhov, dhnv, znv;
    {
#pragma unroll
        for (int g = 0; g < 4; ++g) stv[g] = *(evalid ? p.stash + (int64_t)eb * p.ldst + (int64_t)g * p.H + eunit : g_zero4);
        hpv = *((evalid && p.h_prev) ? p.h_prev + (int64_t)eb * p.ldhp + eunit : g_zero4);
        dhov = *((evalid && p.dh_out) ? p.dh_out + (int64_t)eb * p.lddho + eunit : g_zero4);
        dhnv = *((evalid && next) ? p.dh + (int64_t)eb * p.lddh + eunit : g_zero4);
        znv = *((evalid && next) ? p.stash_next + (int64_t)eb * p.ldstn + (int64_t)p.H + eunit : g_zero4);
    }

    f32x4 acc[1][1][2];
    zero_acc(acc);
    if (next) segment_plain<VEC, NWAVE>(acc, t, p.dgh_next, DenseRows{p.dgh_next, p.lddgh}, p.B, p.w_hh_t, p.ldwt, p.H, 3 * p.H);
    reduce_partials(acc, t);

    if (evalid) {
        const float dh = read_sum<1, 1, NWAVE>(t.red, t.ebl, t.ecl) + dhov + dhnv * znv;
        const float r = stv[0], z = stv[1], n = stv[2], ghn = stv[3];
        const float dn = dh * (1.0f - z);
        const float dz = dh * (hpv - n);
        const float dnp = dn * (1.0f - n * n);
        const float drp = dnp * ghn * r * (1.0f - r);
        const float dzp = dz * z * (1.0f - z);
        float* gx = p.dgx + (int64_t)eb * p.lddgx + eunit;
        gx[0] = drp;
        gx[(int64_t)p.H] = dzp;
        gx[(int64_t)2 * p.H] = dnp;
        float* gh = p.dgh + (int64_t)eb * p.lddgh_out + eunit;
        gh[0] = drp;
        gh[(int64_t)p.H] = dzp;
        gh[(int64_t)2 * p.H] = dnp * r;
        p.dh[(int64_t)eb * p.lddh + eunit] = dh;
    }
}

int gru_step_bwd(hipStream_t stream, const GruBwdArgs& a) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.stash && a.dh && a.dgx && a.dgh, "gru_step_bwd: bad arguments");
    S2VT_REQUIRE(!a.dgh_next || (a.w_hh_t && a.stash_next), "gru_step_bwd: a step with a successor needs W_hh^T and its stash");
    S2VT_REQUIRE(a.ldst >= 4 * (int64_t)a.H && a.lddh >= a.H && a.lddgx >= 3 * (int64_t)a.H && a.lddgh_out >= 3 * (int64_t)a.H &&
                 (!a.dgh_next || (a.lddgh >= 3 * (int64_t)a.H && a.ldwt >= 3 * (int64_t)a.H && a.ldstn >= 4 * (int64_t)a.H)),
                 "gru_step_bwd: row stride below the row length");
    const bool vec = !a.dgh_next || (vec_ok(a.dgh_next, a.lddgh) && vec_ok(a.w_hh_t, a.ldwt));
    const dim3 grid(xcd_grid(cdiv(a.H, 16), cdiv(a.B, GRU_TM))), block(GRU_NW * 64);
    if (vec) hipLaunchKernelGGL((gru_step_bwd_kernel<true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((gru_step_bwd_kernel<false>), grid, block, 0, stream, a);
    S2VT_LAUNCH_CHECK("gru_step_bwd_kernel");
    return 0;
}

}  // namespace s2vt
