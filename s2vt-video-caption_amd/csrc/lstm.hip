// Fused LSTM timestep kernels (forward cell, BPTT cell, decode logits+argmax) for gfx950.
//
// One launch per timestep computes, for a [16*MT batch rows] x [16*NT columns] tile per workgroup,
// the recurrent contraction on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32) and the
// whole pointwise cell in the epilogue, so gate pre-activations never touch HBM:
//   forward  (S2VTModel.py:67,77,86,93,103 -> nn.LSTM step):   G = gx_t + h_{t-1} W_hh^T (+ Emb[tok] W_e^T)
//            columns of a tile = {i,f,g,o} x UN hidden units, so one workgroup owns complete cells;
//   backward (autograd of the same, train.py:124):  dh = dh_out_t + dG_{t+1} W_hh, then the gate
//            derivatives -> dG_t, dc_{t-1};
//   decode   (S2VTModel.py:95-96,105-106): logits tile + first-max argmax folded into one 64-bit
//            atomicMax per (row, tile).
// The 8 waves of a workgroup split K in 32-wide chunks (wave w takes chunks w, w+8, ...), each
// staging its operands through a wave-private LDS image with coalesced 16-B loads and a register
// prefetch of its next two chunks, and the 8 partial tiles are summed through LDS.
// Both operands are k-contiguous (h/dG rows, W_hh rows / W_hh^T rows), LDS row stride 36 floats:
// 16-B aligned staging writes and conflict-free ds_read_b128 operand reads.  Within each 16-wide
// k block lane quarter q owns k = 4q..4q+3 for both operands (fixed summation order).
// (These are the launch-per-timestep kernels: the fp32 training path (two layers on two streams, overlapped with the
// batched GEMMs), decode and beam search; the persistent kernels of lstm_persist*.hip are the bf16 configuration's.)
#include <stdlib.h>
#include "common.h"
#include "experiment.h"
#include "kernels.h"
#include "step_frame.h"

namespace s2vt {

#ifndef S2VT_NWAVE_FWD
#define S2VT_NWAVE_FWD 8
#endif
#ifndef S2VT_NWAVE_BWD
#define S2VT_NWAVE_BWD 8
#endif
// waves per workgroup = K-split factor inside the workgroup.  Both choices keep the LDS footprint at 69.6 KB so
// that two workgroups (e.g. a vid_rnn step and a word_rnn step launched on two streams) fit one CU.
constexpr int NW_FWD = S2VT_NWAVE_FWD;
constexpr int NW_BWD = S2VT_NWAVE_BWD;

// ------------------------------------------------------------------------------ forward step
// (two workgroups must fit a CU: with 8 waves each that is 4 waves per SIMD -> <= 128 VGPRs, see launch bounds)
template <int MT, int NT, bool VEC>
__device__ __forceinline__ void lstm_step_fwd_body(const StepFwdArgs& p, int bid);

// Up to TWO independent timesteps per launch (blocks [0, na): pa, blocks [na, ...): pb), co-resident by construction
// (one workgroup of each per CU).  The training drivers launch one timestep per dispatch on two streams (measured
// faster); the two-step form is exercised by the kernel tests.
template <int MT, int NT, bool VEC>
__global__ __launch_bounds__(NW_FWD * 64, NW_FWD / 2) void lstm_step_fwd_kernel(StepFwdArgs pa, StepFwdArgs pb, int na) {
    if ((int)blockIdx.x < na) lstm_step_fwd_body<MT, NT, VEC>(pa, blockIdx.x);
    else lstm_step_fwd_body<MT, NT, VEC>(pb, blockIdx.x - na);
}

// gates -> (c_t, h_t) and every optional output of a step, for one cell (shared by the fused epilogue and the stand-alone
// cell kernel: one expression, one rounding sequence)
__device__ __forceinline__ void step_cell_outputs(const StepFwdArgs& p, int b, int unit, const float (&pre)[4], float cpv) {
    const LstmCell k = lstm_cell(pre, cpv);
    p.h_out[(int64_t)b * p.ldho + unit] = k.h;
    if (p.h_out2) p.h_out2[(int64_t)b * p.ldho2 + unit] = k.h;
    p.c_out[(int64_t)b * p.ldco + unit] = k.c;
    if (p.stash) {
        float* st = p.stash + (int64_t)b * p.ldst + unit;
        st[0] = k.i;
        st[(int64_t)p.H] = k.f;
        st[(int64_t)2 * p.H] = k.g;
        st[(int64_t)3 * p.H] = k.o;
    }
    // the 8 threads of a row hold the 8 consecutive units u0..u0+7 (u0 % 8 == 0): one 16-byte slot of the plane image
    if (p.h_planes) store_h_planes(p.h_planes, p.ldhp, b, unit, k.h);
}

template <int MT, int NT, bool VEC>
__device__ __forceinline__ void lstm_step_fwd_body(const StepFwdArgs& p, int bid) {
    constexpr int TM = 16 * MT, TN = 16 * NT, UN = TN / 4;
    constexpr int NWAVE = NW_FWD;
    constexpr int NA = (MT * NT == 1) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(MT, NT, NWAVE)];
    StepTile t;
    if (!step_tile<MT, NT, NWAVE, UN>(t, smem, p.H, p.B, bid)) return;
    const int ebl = t.ebl, eu = t.ecl, eb = t.eb, eunit = t.ecol;
    const bool evalid = t.evalid;
    f32x4 acc[MT][NT][NA];
    zero_acc(acc);

    // Epilogue operands (gate inputs, c_{t-1}) are requested NOW, ahead of the K loop, so their HBM/MALL latency
    // is hidden behind the contraction instead of being exposed after it (one output element per thread).
    float gxv[4] = {0.f, 0.f, 0.f, 0.f}, cpv = 0.f;
    if (!p.z_out) {
        const float* gsrc = p.gx ? p.gx + (int64_t)((p.gx_idx && evalid) ? p.gx_idx[eb] : eb) * p.ldgx : p.bias;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float* q = (evalid && gsrc) ? gsrc + (int64_t)g * p.H + eunit : g_zero4;
            gxv[g] = *q;
        }
        const float* q = (evalid && p.c_prev) ? p.c_prev + (int64_t)eb * p.ldc + eunit : g_zero4;
        cpv = *q;
    }
    float gtv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.gx_tab && !p.z_out) {       // embedded-word half of the gate input from the per-token table (two dependent loads, behind the K loop)
        const int64_t tok = evalid ? token_of(p.tok, eb) : 0;
        const float* trow = p.gx_tab + tok * p.ldtab;
#pragma unroll
        for (int g = 0; g < 4; ++g) gtv[g] = *(evalid ? trow + (int64_t)g * p.H + eunit : g_zero4);
    }

    if (p.h_prev) segment_gate_major<VEC, NWAVE, UN>(acc, t, p.h_prev, DenseRows{p.h_prev, p.ldh}, p.B, p.w_hh, p.ldw, p.H, p.H);
    if (p.x2 && !p.z_out)
        segment_gate_major<VEC, NWAVE, UN>(acc, t, p.x2, [&](int b) { return p.x2 + token_of(p.tok, b) * p.ldx2; }, p.B, p.w2, p.ldw2, p.H, p.K2);

    // a half-wave of the epilogue reads 4 rows x UN = 8 consecutive columns per gate: row stride 8 (mod 32) puts the 32
    // lanes on 32 banks (stride 33 put them on 11: 4-way conflicts on each of the 32 reads of a thread)
    constexpr int RLD = TN + 8;
    static_assert(UN == 8 && NWAVE * TM * RLD <= step_lds_floats(MT, NT, NWAVE), "partial tiles fit the staging area");
    reduce_partials<RLD>(acc, t);
    const float* red = t.red;

    if (evalid && p.z_out) {           // contraction only: the cell update is lstm_cell_pointwise's
#pragma unroll
        for (int g = 0; g < 4; ++g)
            p.z_out[(int64_t)eb * p.ldz + (int64_t)g * p.H + eunit] = read_sum<MT, NT, NWAVE, RLD>(red, ebl, g * UN + eu);
        return;
    }
    if (evalid) {
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = read_sum<MT, NT, NWAVE, RLD>(red, ebl, g * UN + eu) + gxv[g] + gtv[g];
        step_cell_outputs(p, eb, eunit, pre, cpv);
    }
}

// The epilogue of lstm_step_fwd_body on a contraction that ran as its own launch (z_out): one thread per NU consecutive cells
// of a batch row (NU = 4: 16-byte loads and stores, H % 4 == 0 and 16-byte aligned rows; NU = 1 otherwise).
template <int NU>
__global__ __launch_bounds__(256) void lstm_cell_pointwise_kernel(StepFwdArgs p) {
    const int upr = p.H / NU;                          // threads per batch row
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= p.B * upr) return;
    const int b = i / upr, unit = (i % upr) * NU;
    typedef float vec __attribute__((ext_vector_type(NU)));
    const float* gsrc = p.gx ? p.gx + (int64_t)(p.gx_idx ? p.gx_idx[b] : b) * p.ldgx : p.bias;
    const float* zsrc = p.z_out + (int64_t)b * p.ldz + unit;
    const float* trow = p.gx_tab ? p.gx_tab + token_of(p.tok, b) * p.ldtab + unit : nullptr;
    vec zv[4], gxv[4], gtv[4], cpv;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        zv[g] = *reinterpret_cast<const vec*>(zsrc + (int64_t)g * p.H);
        gxv[g] = *reinterpret_cast<const vec*>(gsrc + (int64_t)g * p.H + unit);
        gtv[g] = trow ? *reinterpret_cast<const vec*>(trow + (int64_t)g * p.H) : (vec)(0.f);
    }
    cpv = p.c_prev ? *reinterpret_cast<const vec*>(p.c_prev + (int64_t)b * p.ldc + unit) : (vec)(0.f);
#pragma unroll
    for (int e = 0; e < NU; ++e) {
        float pre[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = zv[g][e] + gxv[g][e] + gtv[g][e];
        step_cell_outputs(p, b, unit + e, pre, cpv[e]);
    }
}

static bool step_fwd_vec(const StepFwdArgs& a) {
    // vector path: 16-B aligned rows whose length is a multiple of 4 floats, for every operand in use
    return (!a.h_prev || (vec_ok(a.h_prev, a.ldh) && vec_ok(a.w_hh, a.ldw) && a.H % 4 == 0)) &&
           (!a.x2 || (vec_ok(a.x2, a.ldx2) && vec_ok(a.w2, a.ldw2) && a.K2 % 4 == 0));
}

// b == nullptr: one timestep; otherwise two independent timesteps of the same (B, H) in one launch
int lstm_step_fwd2(hipStream_t stream, const StepFwdArgs& a, const StepFwdArgs* b) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && ((a.h_out && a.c_out) || a.z_out), "lstm_step_fwd: bad arguments");
    S2VT_REQUIRE(a.gx || a.bias || a.z_out, "lstm_step_fwd: need gx or bias");
    S2VT_REQUIRE(!a.z_out || (a.h_prev && !b && a.ldz >= 4 * (int64_t)a.H), "lstm_step_fwd: a contraction-only step needs h_prev and runs alone");
    S2VT_REQUIRE(!(a.x2 || a.gx_tab) || a.tok.tok_limit > 0, "lstm_step_fwd: a token segment needs tok_limit (rows of the table)");
    S2VT_REQUIRE(!b || (b->B == a.B && b->H == a.H && b->h_out && b->c_out && (b->gx || b->bias)),
                 "lstm_step_fwd: paired steps must have the same batch and hidden size");
    // B <= 4: gate GEMVs (lstm_gemv.hip) - measured faster than the 16-row tile up to there (a B = 1 greedy decode 3.07 vs 3.67 ms,
    // B = 4 3.47 vs 3.73, B = 6 4.01 vs 3.81: profiles/round5_gemv_small_batch.txt); option gemv = 2 sends every B <= 8 there
    if (!b && lstm_step_fwd_gemv_ok(a) && (option(O_GEMV) == 2 || (option(O_GEMV) == 1 && a.B <= 4))) return lstm_step_fwd_gemv(stream, a);
    const bool vec = step_fwd_vec(a) && (!b || step_fwd_vec(*b));
    const StepFwdArgs& bb = b ? *b : a;
    if (a.B <= 16) {
        const int na = xcd_grid(cdiv(a.H, 8), cdiv(a.B, 16));
        dim3 grid(b ? 2 * na : na);
        if (vec) hipLaunchKernelGGL((lstm_step_fwd_kernel<1, 2, true>), grid, dim3(NW_FWD * 64), 0, stream, a, bb, na);
        else hipLaunchKernelGGL((lstm_step_fwd_kernel<1, 2, false>), grid, dim3(NW_FWD * 64), 0, stream, a, bb, na);
    } else {
        const int na = xcd_grid(cdiv(a.H, 8), cdiv(a.B, 32));
        dim3 grid(b ? 2 * na : na);
        if (vec) hipLaunchKernelGGL((lstm_step_fwd_kernel<2, 2, true>), grid, dim3(NW_FWD * 64), 0, stream, a, bb, na);
        else hipLaunchKernelGGL((lstm_step_fwd_kernel<2, 2, false>), grid, dim3(NW_FWD * 64), 0, stream, a, bb, na);
    }
    S2VT_LAUNCH_CHECK("lstm_step_fwd_kernel");
    return 0;
}
int lstm_step_fwd(hipStream_t stream, const StepFwdArgs& a) { return lstm_step_fwd2(stream, a, nullptr); }

int lstm_cell_pointwise(hipStream_t stream, const StepFwdArgs& a) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.h_out && a.c_out && a.z_out && a.ldz >= 4 * (int64_t)a.H, "lstm_cell_pointwise: bad arguments");
    S2VT_REQUIRE(a.gx || a.bias, "lstm_cell_pointwise: need gx or bias");
    S2VT_REQUIRE(!a.x2, "lstm_cell_pointwise: the token segment must be the per-token table (gx_tab), not a second K segment");
    S2VT_REQUIRE(!a.gx_tab || a.tok.tok_limit > 0, "lstm_cell_pointwise: a token segment needs tok_limit (rows of the table)");
    const bool v4 = a.H % 4 == 0 && vec_ok(a.z_out, a.ldz) && (!a.gx || vec_ok(a.gx, a.ldgx)) && (!a.bias || vec_ok(a.bias, 4)) &&
                    (!a.gx_tab || vec_ok(a.gx_tab, a.ldtab)) && (!a.c_prev || vec_ok(a.c_prev, a.ldc));
    if (v4) hipLaunchKernelGGL(lstm_cell_pointwise_kernel<4>, dim3((unsigned)cdiv(a.B * (a.H / 4), 256)), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(lstm_cell_pointwise_kernel<1>, dim3((unsigned)cdiv(a.B * a.H, 256)), dim3(256), 0, stream, a);
    S2VT_LAUNCH_CHECK("lstm_cell_pointwise_kernel");
    return 0;
}

// ----------------------------------------------------------------------------- backward step
template <int MT, int NT, bool VEC>
__device__ __forceinline__ void lstm_step_bwd_body(const StepBwdArgs& p, int bid);

template <int MT, int NT, bool VEC>
__global__ __launch_bounds__(NW_BWD * 64) void lstm_step_bwd_kernel(StepBwdArgs pa, StepBwdArgs pb, int na) {
    if ((int)blockIdx.x < na) lstm_step_bwd_body<MT, NT, VEC>(pa, blockIdx.x);
    else lstm_step_bwd_body<MT, NT, VEC>(pb, blockIdx.x - na);
}

template <int MT, int NT, bool VEC>
__device__ __forceinline__ void lstm_step_bwd_body(const StepBwdArgs& p, int bid) {
    constexpr int TN = 16 * NT;
    constexpr int NWAVE = NW_BWD;
    constexpr int NA = (MT * NT == 1) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(MT, NT, NWAVE)];
    StepTile t;
    if (!step_tile<MT, NT, NWAVE, TN>(t, smem, p.H, p.B, bid)) return;
    const int eb = t.eb, eunit = t.ecol;
    const bool evalid = t.evalid;
    f32x4 acc[MT][NT][NA];
    zero_acc(acc);

    // epilogue operands requested ahead of the K loop (see the forward kernel)
    float stv[4], cv, cpv, dcv, dhov;
    {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float* q = evalid ? p.stash + (int64_t)eb * p.ldst + (int64_t)g * p.H + eunit : g_zero4;
            stv[g] = *q;
        }
        const float* q1 = evalid ? p.c + (int64_t)eb * p.ldc + eunit : g_zero4;
        const float* q2 = (evalid && p.c_prev) ? p.c_prev + (int64_t)eb * p.ldcp + eunit : g_zero4;
        const float* q3 = (evalid && !p.dc_is_zero) ? p.dc + (int64_t)eb * p.lddc + eunit : g_zero4;
        const float* q4 = (evalid && p.dh_out) ? p.dh_out + (int64_t)eb * p.lddho + eunit : g_zero4;
        cv = *q1; cpv = *q2; dcv = *q3; dhov = *q4;
    }

    if (p.dg_next) segment_plain<VEC, NWAVE>(acc, t, p.dg_next, DenseRows{p.dg_next, p.lddg}, p.B, p.w_hh_t, p.ldwt, p.H, 4 * p.H);
    reduce_partials(acc, t);

    if (evalid) {
        const float dh = read_sum<MT, NT, NWAVE>(t.red, t.ebl, t.ecl) + dhov;
        const LstmCellGrad d = lstm_cell_grad(dh, stv, cv, cpv, dcv);
        float* dg = p.dg + (int64_t)eb * p.lddg_out + eunit;
#pragma unroll
        for (int g = 0; g < 4; ++g) dg[(int64_t)g * p.H] = d.dg[g];
        p.dc[(int64_t)eb * p.lddc + eunit] = d.dc_prev;
    }
}

int lstm_step_bwd2(hipStream_t stream, const StepBwdArgs& a, const StepBwdArgs* b) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.stash && a.c && a.dc && a.dg, "lstm_step_bwd: bad arguments");
    S2VT_REQUIRE(!b || (b->B == a.B && b->H == a.H && b->stash && b->c && b->dc && b->dg),
                 "lstm_step_bwd: paired steps must have the same batch and hidden size");
    auto okv = [](const StepBwdArgs& x) { return !x.dg_next || (vec_ok(x.dg_next, x.lddg) && vec_ok(x.w_hh_t, x.ldwt)); };
    const bool vec = okv(a) && (!b || okv(*b));
    const StepBwdArgs& bb = b ? *b : a;
    // 32-row tiles where they still fill the chip (B >= 128 at H = 1000): a workgroup then takes
    // in dG of 32 rows + one W_hh^T slice (768 KB) where two 16-row workgroups take in 1 MB - config-3-shard step (B = 128)
    // 20.56 -> 20.11 ms; at B = 64 they would leave half the compute units idle (11.6 -> 12.0 ms)
    const bool wide = vec && cdiv(a.H, 16) * cdiv(a.B, 32) >= 240;
    if (wide) {
        const int na = xcd_grid(cdiv(a.H, 16), cdiv(a.B, 32));
        hipLaunchKernelGGL((lstm_step_bwd_kernel<2, 1, true>), dim3(b ? 2 * na : na), dim3(NW_BWD * 64), 0, stream, a, bb, na);
        S2VT_LAUNCH_CHECK("lstm_step_bwd_kernel");
        return 0;
    }
    const int na = xcd_grid(cdiv(a.H, 16), cdiv(a.B, 16));
    dim3 grid(b ? 2 * na : na);
    if (vec) hipLaunchKernelGGL((lstm_step_bwd_kernel<1, 1, true>), grid, dim3(NW_BWD * 64), 0, stream, a, bb, na);
    else hipLaunchKernelGGL((lstm_step_bwd_kernel<1, 1, false>), grid, dim3(NW_BWD * 64), 0, stream, a, bb, na);
    S2VT_LAUNCH_CHECK("lstm_step_bwd_kernel");
    return 0;
}
int lstm_step_bwd(hipStream_t stream, const StepBwdArgs& a) { return lstm_step_bwd2(stream, a, nullptr); }

// -------------------------------------------------------------------- decode: logits + argmax
__device__ __forceinline__ uint32_t ordered_bits(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// SAMPLE: score = logit * inv_temperature + Gumbel noise ahead of the packed max - the arg-max is then a draw from
// softmax(logit / temperature) (Gumbel-max; philox.h).  A thread's CPT = 4 columns are four consecutive vocabulary indices from a
// multiple of 4: one Philox block serves them.  A compile-time variant: the greedy instantiations keep their code and registers.
template <int MT, int NT, bool VEC, int NWAVE, bool SAMPLE = false>
__global__ __launch_bounds__(NWAVE * 64, 4) void logits_argmax_kernel(LogitsArgmaxArgs p, GumbelArgs ga) {
    constexpr int TM = 16 * MT, TN = 16 * NT;
    constexpr int NTHR = NWAVE * 64;
    constexpr int NA = (MT * NT == 1) ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float smem[step_lds_floats(MT, NT, NWAVE)];
    StepTile t;
    if (!step_tile<MT, NT, NWAVE, TN, false>(t, smem, p.V, p.B)) return;
    const int tid = t.tid, b0 = t.b0, n0 = t.n0;
    const int xrec = p.stamps ? (int)blockIdx.x : -1;
    XSTAMP(p.stamps, xrec, 0);

    // epilogue role: 8 threads per batch row, TN/8 columns each; the bias of those columns is requested NOW, ahead of the
    // contraction (in-kernel stamps: fetched in the epilogue it cost every tile ~1.5 us of exposed latency)
    constexpr int CPT = TN / 8;
    static_assert(TM * 8 == 256 && TM * 8 <= NTHR, "one pass over the tile");
    const int bl = (tid >> 3) % TM, sub = tid & 7;
    const bool active = tid < TM * 8;
    float bv[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int n = n0 + sub * CPT + j;
        bv[j] = *((active && p.b_out && n < p.V) ? p.b_out + n : g_zero4);
    }

    f32x4 acc[MT][NT][NA];
    zero_acc(acc);
    segment_plain<VEC, NWAVE>(acc, t, p.h, DenseRows{p.h, p.ldh}, p.B, p.w_out, p.ldw, p.V, p.H);
    XSTAMP(p.stamps, xrec, 1);
    __syncthreads();
    XSTAMP(p.stamps, xrec, 2);       // (a stamp inside the reduction: it stays longhand here)
    float* red = t.red;
    write_partials<MT, NT, NA>(acc, red, t.wave, t.lane);
    __syncthreads();
    XSTAMP(p.stamps, xrec, 3);

    // 8 threads per batch row, TN/8 columns each; first-max (lowest index) wins ties.
    const int b = b0 + bl;
    unsigned long long best = 0ull;
    float gn[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SAMPLE) {
        static_assert(CPT == 4 && TN % 4 == 0, "one Philox block per thread");
        if (active && b < p.B && ga.row0 + (uint32_t)b < ga.rows && n0 + sub * CPT < p.V) gumbel4(ga, (uint32_t)(n0 + sub * CPT) >> 2, ga.row0 + (uint32_t)b, gn);
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        const int nl = sub * CPT + j, n = n0 + nl;
        if (active && b < p.B && n < p.V) {
            float v = read_sum<MT, NT, NWAVE>(red, bl, nl) + bv[j];
            if constexpr (SAMPLE) v = v * ga.inv_temperature + gn[j];
            const unsigned long long key =
                ((unsigned long long)ordered_bits(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)n);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if (active && sub == 0 && b < p.B && best) atomicMax(&p.packed[b], best);
    XSTAMP(p.stamps, xrec, 4);
}

int logits_argmax(hipStream_t stream, const LogitsArgmaxArgs& a, const GumbelArgs* sample) {
    S2VT_REQUIRE(a.B > 0 && a.H > 0 && a.V > 0 && a.h && a.w_out && a.packed, "logits_argmax: bad arguments");
    const bool vec = vec_ok(a.h, a.ldh) && vec_ok(a.w_out, a.ldw) && a.H % 4 == 0;
    dim3 grid(xcd_grid(cdiv(a.V, 32), cdiv(a.B, 32)));
    // 4 waves per tile (K split four ways, 36.9 KB LDS, four workgroups per CU): with eight (two workgroups per CU) every
    // workgroup of a CU sat in its reduction / argmax phase at about the same time and the CU's ingest idled meanwhile
    // (in-kernel stamps of all 1500 workgroups, tools/bench_argmax_stamps.py; 2 % on a greedy decode)
    const GumbelArgs ga = sample ? *sample : GumbelArgs{1.f, 0u, 0u, 0u, 0u, 0u};
    if (sample) {
        if (vec) hipLaunchKernelGGL((logits_argmax_kernel<2, 2, true, 4, true>), grid, dim3(256), 0, stream, a, ga);
        else hipLaunchKernelGGL((logits_argmax_kernel<2, 2, false, 4, true>), grid, dim3(256), 0, stream, a, ga);
    } else if (vec) hipLaunchKernelGGL((logits_argmax_kernel<2, 2, true, 4>), grid, dim3(256), 0, stream, a, ga);
    else hipLaunchKernelGGL((logits_argmax_kernel<2, 2, false, 4>), grid, dim3(256), 0, stream, a, ga);
    S2VT_LAUNCH_CHECK("logits_argmax_kernel");
    return 0;
}

}  // namespace s2vt
