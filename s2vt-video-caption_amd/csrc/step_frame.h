// The frame of the launch-per-timestep cell kernels on the fp32 matrix cores (lstm.hip, lstm_stack.hip, gru.hip): what
// surrounds the contraction of mfma_tile.h in every one of them, stated once -
//   the tile prologue   LDS carve, thread roles, XCD placement, tile origin, the one-cell-per-thread epilogue mapping;
//   the K segments      per-lane operand row pointers by one of two weight-row rules, then wave_gemm_nt;
//   the reduction       barrier, the waves' partial tiles to LDS, barrier;
// and the LSTM cell with its derivative and the blocked-plane store of h_t, which lstm_gemv.hip and lstm_bf16.hip share too.
// Everything is __forceinline__ and StepTile a plain struct of ints and pointers: it dissolves into the registers the
// kernels held before (they sit at 128 VGPRs for two workgroups per CU).
#pragma once
#include "mfma_tile.h"

namespace s2vt {

// floats of LDS of a workgroup of NWAVE waves on a 16*MT x 16*NT tile: one staging image of A and of B per wave; the
// partial tiles of the reduction reuse them.  The __shared__ array itself is declared by the kernel body.
constexpr int step_lds_floats(int MT, int NT, int NWAVE) { return NWAVE * 16 * (MT + NT) * SLD; }

struct StepTile {
    int tid, lane, wave, lrow;      // lrow: the staged row of this lane within a wave-wide load
    int b0, n0;                     // first batch row / first column (hidden unit, or weight row of a plain tile) of the tile
    float *sA, *sB, *red;           // the wave's staging images; the partial tiles (the same LDS after the contraction)
    int ebl, ecl, eb, ecol;         // epilogue, one cell per thread: row / column within the tile and in the batch
    bool evalid;
};

// Tile `bid` (default: blockIdx.x) of a grid of xcd_grid(cdiv(ncols, CW), cdiv(nrows, 16*MT)) workgroups; CW = columns a
// tile owns in the unit of n0 (the UN hidden units of a gate-major tile, the 16*NT rows of a plain one).  false: no tile.
// CELL: thread tid of the first 16*MT*CW owns cell (tid / CW, tid % CW) of the epilogue.
template <int MT, int NT, int NWAVE, int CW, bool CELL = true>
__device__ __forceinline__ bool step_tile(StepTile& t, float* smem, int ncols, int nrows, int bid = -1) {
    constexpr int TM = 16 * MT, TN = 16 * NT;
    t.tid = threadIdx.x; t.lane = t.tid & 63; t.wave = t.tid >> 6;
    t.lrow = t.lane / LPR;
    t.sA = smem + t.wave * (TM + TN) * SLD;
    t.sB = t.sA + TM * SLD;
    t.red = smem;
    int tx, ty;
    if (!xcd_tile((ncols + CW - 1) / CW, (nrows + TM - 1) / TM, tx, ty, bid)) return false;
    t.b0 = ty * TM; t.n0 = tx * CW;
    if constexpr (CELL) {
        static_assert(TM * CW <= NWAVE * 64, "one epilogue element per thread");
        t.ebl = t.tid / CW; t.ecl = t.tid % CW;
        t.eb = t.b0 + t.ebl; t.ecol = t.n0 + t.ecl;
        t.evalid = (t.tid < TM * CW) && (t.eb < nrows) && (t.ecol < ncols);
    }
    return true;
}

template <int MT, int NT, int NA>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MT][NT][NA]) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[mi][ni][a] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---- K segments: acc += A[rows b0.., 0:K] · W[the tile's rows, 0:K]^T.  arow_of(b) = row b of A for b < B: DenseRows, or a
// lambda over token_of() for an embedding gather.
struct DenseRows {
    const float* a; int64_t ld;
    __device__ __forceinline__ const float* operator()(int b) const { return a + (int64_t)b * ld; }
};

template <int MT, class ARow>
__device__ __forceinline__ void a_row_ptrs(const float* (&arow)[MT * LPT], const StepTile& t, ARow arow_of, int B) {
#pragma unroll
    for (int i = 0; i < MT * LPT; ++i) {
        const int b = t.b0 + t.lrow + RPL * i;
        arow[i] = (b < B) ? arow_of(b) : nullptr;
    }
}

// gate-major weight rows: tile row r is unit n0 + r % UN of gate r / UN, i.e. row g * H + u of W [gates * H, ldw]
template <bool VEC, int NWAVE, int UN, int NPF = PF, int MT, int NT, int NA, class ARow>
__device__ __forceinline__ void segment_gate_major(f32x4 (&acc)[MT][NT][NA], const StepTile& t, const float* abase, ARow arow_of, int B,
                                                   const float* w, int64_t ldw, int H, int K) {
    const float* arow[MT * LPT];
    const float* brow[NT * LPT];
    a_row_ptrs<MT>(arow, t, arow_of, B);
#pragma unroll
    for (int i = 0; i < NT * LPT; ++i) {
        const int r = t.lrow + RPL * i, g = r / UN, u = t.n0 + r % UN;
        brow[i] = (u < H) ? w + ((int64_t)g * H + u) * ldw : nullptr;
    }
    wave_gemm_nt<MT, NT, NA, VEC, NWAVE, NPF>(acc, abase, w, arow, brow, K, t.sA, t.sB, t.wave, t.lane);
}

// plain weight rows: tile row r is row n0 + r of W [N, ldw]
template <bool VEC, int NWAVE, int NPF = PF, int MT, int NT, int NA, class ARow>
__device__ __forceinline__ void segment_plain(f32x4 (&acc)[MT][NT][NA], const StepTile& t, const float* abase, ARow arow_of, int B,
                                              const float* w, int64_t ldw, int N, int K) {
    const float* arow[MT * LPT];
    const float* brow[NT * LPT];
    a_row_ptrs<MT>(arow, t, arow_of, B);
#pragma unroll
    for (int i = 0; i < NT * LPT; ++i) {
        const int n = t.n0 + t.lrow + RPL * i;
        brow[i] = (n < N) ? w + (int64_t)n * ldw : nullptr;
    }
    wave_gemm_nt<MT, NT, NA, VEC, NWAVE, NPF>(acc, abase, w, arow, brow, K, t.sA, t.sB, t.wave, t.lane);
}

// ---- the reduction: every wave's partial tile to t.red (row stride RLD, default write_partials'), read back with read_sum
template <int RLD = 0, int MT, int NT, int NA>
__device__ __forceinline__ void reduce_partials(const f32x4 (&acc)[MT][NT][NA], const StepTile& t) {
    constexpr int R = RLD ? RLD : 16 * NT + 1;
    __syncthreads();
    write_partials<MT, NT, NA, R>(acc, t.red, t.wave, t.lane);
    __syncthreads();
}

// ---- the LSTM cell (nn.LSTM gate order i, f, g, o): one expression, one rounding sequence for every kernel that runs it
struct LstmCell { float i, f, g, o, c, h; };
__device__ __forceinline__ LstmCell lstm_cell(const float (&pre)[4], float c_prev) {
    LstmCell r;
    r.i = sigmoidf_(pre[0]);
    r.f = sigmoidf_(pre[1]);
    r.g = tanhf_(pre[2]);
    r.o = sigmoidf_(pre[3]);
    r.c = r.f * c_prev + r.i * r.g;
    r.h = r.o * tanhf_(r.c);
    return r;
}

// its derivative from the activated gates st = {i, f, g, o}: dh = dL/dh_t, dc_in = dL/dc_t carried from t + 1;
// dg = dL/d(pre-activations), dc_prev = dL/dc_{t-1}
struct LstmCellGrad { float dg[4]; float dc_prev; };
__device__ __forceinline__ LstmCellGrad lstm_cell_grad(float dh, const float (&st)[4], float c, float c_prev, float dc_in) {
    const float ig = st[0], fg = st[1], gg = st[2], og = st[3];
    const float tc = tanhf_(c);
    const float dc = dh * og * (1.0f - tc * tc) + dc_in;
    const float d_o = dh * tc;
    LstmCellGrad r;
    r.dg[0] = dc * gg * ig * (1.0f - ig);
    r.dg[1] = dc * c_prev * fg * (1.0f - fg);
    r.dg[2] = dc * ig * (1.0f - gg * gg);
    r.dg[3] = d_o * og * (1.0f - og);
    r.dc_prev = dc * fg;
    return r;
}

// h_t of (batch row b, hidden unit) as three bf16 planes in the blocked operand layout of split.hip: element (row b, k = unit,
// plane pl) at (b/64)*(64*ld) + (k/16)*3072 + (pl*2 + (k%16)/8)*512 + (b%64)*8 + k%8.  Threads that hold 8 consecutive units
// from a multiple of 8 of one row fill one 16-byte slot with their 2-byte stores, the rows of a tile consecutive slots.
__device__ __forceinline__ void store_h_planes(unsigned short* h_planes, int64_t ldhp, int b, int unit, float h) {
    unsigned short pl3[3];
    split3_bits(h, pl3);
    unsigned short* q = h_planes + (int64_t)(b >> 6) * (64 * ldhp) + (int64_t)(unit >> 4) * 3072 + ((unit >> 3) & 1) * 512 +
                        (b & 63) * 8 + (unit & 7);
    q[0] = pl3[0];
    q[1024] = pl3[1];
    q[2048] = pl3[2];
}

}  // namespace s2vt
