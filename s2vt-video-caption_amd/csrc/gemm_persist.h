// The frame the two persistent LDS-DMA GEMM kernels share - gemm_x3_kernel (gemm_x3.hip: three bf16 planes, blocked layout) and
// gemm_b1_kernel (gemm_b1.hip: one plane, bf16 rows): the argument struct, the XCD-chunked tile walk, the epilogue and the host
// side that picks tile height, split-K factor and grid.  What differs between the kernels - the stage image, the loader, the
// fragment reads and the MFMA schedule - stays in their own files.
#pragma once
#include "common.h"

namespace s2vt {

struct PersistGemmArgs {
    int M, N, K;                              // K = padded k extent of this call (multiple of 64)
    const unsigned short* A; int64_t lda;     // x3: blocked planes, row-block stride = 64 * lda elements; b1: bf16 rows
    const unsigned short* B; int64_t ldb;
    float* C; int64_t ldc; RowMap cmap;
    const float* bias;
    int accumulate;
    int ksplit;                               // k extent of a split-K slice (blockIdx.y), multiple of 64
    float* slabs;
    int ntm, ntn;                             // tile grid of this launch's tile height
};

// ---- a workgroup's share of the tiles: the XCD of blockIdx % 8 owns a contiguous chunk of the (grouped) tile order, its
// gridDim / 8 workgroups walk that chunk side by side (tiles q, q + gx, ... below q_end: neighbouring tiles that share operand
// panels in the XCD's L2); blockIdx.y = the split-K slice [kbeg, kend)
struct PersistWalk {
    int q, q_end, gx, kbeg, kend, ntm, ntn;
    __device__ __forceinline__ PersistWalk(const PersistGemmArgs& p, dim3 bid, dim3 gdim) {
        const int items = p.ntm * p.ntn;
        const int cpx = (items + 7) >> 3, xcd = bid.x & 7;
        gx = (int)gdim.x >> 3;
        q_end = ((xcd + 1) * cpx < items) ? (xcd + 1) * cpx : items;
        q = xcd * cpx + (int)(bid.x >> 3);
        kbeg = bid.y * p.ksplit;
        kend = (kbeg + p.ksplit < p.K) ? kbeg + p.ksplit : p.K;
        ntm = p.ntm; ntn = p.ntn;
    }
    // first row and column of tile t of the order: groups of GM tile rows, column-major inside a group
    template <int TILE_ROWS>
    __device__ __forceinline__ void tile_of(int t, int& m0, int& n0) const {
        constexpr int GM = 4;
        const int gsz = GM * ntn, grp = t / gsz, first_m = grp * GM;
        const int gm = (ntm - first_m < GM) ? (ntm - first_m) : GM;
        m0 = (first_m + (t % gsz) % gm) * TILE_ROWS;
        n0 = ((t % gsz) / gm) * 256;
    }
};

template <int MI>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MI][2]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
}

// 4x4 transpose inside every quad of lanes: lane t of a quad holds (a0..a3) = column t of a 4x4 block whose rows are the four
// registers; afterwards it holds row t (two butterfly rounds of DPP quad_perm exchanges: lanes t <-> t ^ 1 exchange (a0, a1) and
// (a2, a3) crosswise, then t <-> t ^ 2 (a0, a2) and (a1, a3))
__device__ __forceinline__ void quad_transpose4(float& a0, float& a1, float& a2, float& a3, bool odd, bool hi) {
    float s, r;
    s = odd ? a0 : a1; r = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s), 0xB1, 0xF, 0xF, false));
    a0 = odd ? r : a0; a1 = odd ? a1 : r;
    s = odd ? a2 : a3; r = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s), 0xB1, 0xF, 0xF, false));
    a2 = odd ? r : a2; a3 = odd ? a3 : r;
    s = hi ? a0 : a2; r = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s), 0x4E, 0xF, 0xF, false));
    a0 = hi ? r : a0; a2 = hi ? a2 : r;
    s = hi ? a1 : a3; r = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s), 0x4E, 0xF, 0xF, false));
    a1 = hi ? r : a1; a3 = hi ? a3 : r;
}

// The epilogue of wave (wm, wn)'s (32 MI) x 64 part of the tile at (m0, n0) issues at least 8 MI vector-memory instructions: all
// rows valid and both column groups of the wave inside N.  The next stage's counted vmcnt wait relies on that lower bound: "at
// most 8 MI (+ the stage's own requests) operations outstanding" then says that the requests issued BEFORE those stores have
// landed (the counter retires in issue order) without sitting out the stores.
template <int MI>
__device__ __forceinline__ bool store_tile_counted(const PersistGemmArgs& p, int m0, int n0, int wn) {
    return m0 + 64 * MI <= p.M && n0 + wn * 64 + 64 <= p.N;
}

// ---- epilogue (the next tile's first stages are in flight under these stores).  The 32x32 accumulator layout gives a lane ONE
// column and 16 rows; stored as it stands that is 32 MI dword store instructions per wave, and a tile's epilogue is bound by
// their issue (16 us of a 44-us gemm_b1 tile at K = 1024: with a quarter of them, timing only, the K = 1000 shapes ran 20-25 %
// faster).  So every 4x4 block (registers 4j..4j+3 x the lanes of a quad) is transposed inside the quad and a lane stores FOUR
// consecutive columns of one row as 16 bytes: a wave instruction then writes 8 rows x 128 B, a quarter of the instructions for
// the same bytes.  Split-K slices (slabs) leave plain [M][N] slabs for splitk_reduce, bias and accumulate with them.
// (The output fields of the kernel's PersistGemmArgs come BY VALUE: with the struct passed by reference the register allocation of
// the whole kernel shifts - SGPR spills in the transposed forms, profiles/gemm_frame_refactor.txt.)
template <int MI>
__device__ __forceinline__ void store_tile(const f32x16 (&acc)[MI][2], int m0, int n0, int wm, int wn, int li, int lh, int M, int N, float* C,
                                           int64_t ldc, RowMap cmap, const float* bias, int accumulate, float* slabs) {
    // (the lane's coordinates are made opaque here: address arithmetic of the epilogue that does not depend on the tile
    // would otherwise be hoisted out of the tile loop and held in registers across the stage pipeline)
    int e_li = li, e_lh = lh;
    asm volatile("" : "+v"(e_li), "+v"(e_lh));
    const int t = e_li & 3;
    const bool odd = t & 1, hi = t & 2;
    const int ncol = n0 + wn * 64 + (e_li & ~3);                   // first of this lane's four columns (ni = 0)
    const bool vec = slabs ? ((N & 3) == 0 && (reinterpret_cast<uintptr_t>(slabs) & 15) == 0)
                             : ((ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0);      // 16-byte rows
    f32x4 bv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (bias && !slabs) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int n = ncol + ni * 32 + k;
                bv[ni][k] = n < N ? bias[n] : 0.f;
            }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + wm * 32 * MI + mi * 32 + 8 * j + 4 * e_lh + t;      // this lane's row after the transpose
            f32x4 v[2];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                float a0 = acc[mi][ni][4 * j], a1 = acc[mi][ni][4 * j + 1], a2 = acc[mi][ni][4 * j + 2], a3 = acc[mi][ni][4 * j + 3];
                quad_transpose4(a0, a1, a2, a3, odd, hi);
                v[ni] = f32x4{a0, a1, a2, a3};
            }
            if (m >= M) continue;
            float* row = slabs ? slabs + ((int64_t)blockIdx.y * M + m) * N : C + (int64_t)map_row(cmap, m) * ldc;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int n = ncol + ni * 32;
                f32x4 o = v[ni];
                if (!slabs) { o[0] += bv[ni][0]; o[1] += bv[ni][1]; o[2] += bv[ni][2]; o[3] += bv[ni][3]; }
                if (vec && n + 4 <= N) {
                    f32x4* q4 = reinterpret_cast<f32x4*>(row + n);
                    if (accumulate && !slabs) { const f32x4 c = *q4; o[0] += c[0]; o[1] += c[1]; o[2] += c[2]; o[3] += c[3]; }
                    *q4 = o;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (n + k < N) {
                            float x = o[k];
                            if (accumulate && !slabs) x += row[n + k];
                            row[n + k] = x;
                        }
                }
            }
        }
    }
}

// ---- host side: tile height, split-K factor and grid of a launch by a time model.  A launch is at most ONE workgroup per compute
// unit; every workgroup walks ceil(its XCD's chunk / workgroups of the XCD) tiles of K / stage_k stages + an epilogue; split-K adds
// the fixed-order slab combine ((n + 1) passes over M x N floats at ~3.5 TB/s + a launch).
struct PersistPlanIn {
    // the call.  ws_floats = split-K scratch the caller gave (0: none); force_mi / force_n = the *_tune overrides (0: the model's)
    bool tt;
    int M, N, K;
    int64_t ldmax;                  // larger row stride of the two operands (tt: elements per image row)
    size_t ws_floats;
    int force_mi, force_n;
    // the kernel: tile heights in the order they are tried (a later one must beat an earlier one by 2 %), per-tile cost tables (us,
    // indexed by MI) of a stage of stage_k k columns and of the epilogue
    const int* order; int norder;
    bool tt_mi4_only;               // the transposed form exists for 256-row tiles alone (and then ignores force_mi)
    int stage_k;
    const double* stage_us; const double* epi_us;
    // Transposed reads address a k slice of a row image through ONE buffer descriptor and 32-bit offsets: a slice (ks image rows of
    // ldmax elements) must stay below tt_span bytes.  An image beyond that (dlogits from B = 768 on at V = 12000) is cut into k
    // slices - the split-K path with its fixed-order combine - instead of being refused.
    int64_t tt_span;
};
struct PersistPlan {
    int mi;                         // tile height / 64; 0: refused - a transposed image beyond tt_span that cannot be sliced
    int nsplit, ksplit, grid;       // split-K slices (grid.y) of ksplit k columns each, workgroups per slice (grid.x)
};

// pure: no HIP call, no global (ncu = planned_compute_units() of the caller)
static inline PersistPlan plan_persistent_gemm(const PersistPlanIn& in, int ncu) {
    const int M = in.M, N = in.N, K = in.K, ntn = cdiv(N, 256);
    int best_mi = 4, best_ns = 1, best_g = 8;
    double best = 1e30;
    for (int oi = 0; oi < in.norder; ++oi) {
        const int mi = in.order[oi];
        if ((in.tt && in.tt_mi4_only) ? mi != 4 : (in.force_mi && in.force_mi != mi)) continue;
        const int tiles = cdiv(M, 64 * mi) * ntn;
        for (int n = 1; n <= 16; ++n) {
            if (n > 1 && (K < 512 || K / n < 256 || (size_t)n * M * N > in.ws_floats)) break;
            if (in.force_n && n != in.force_n) continue;
            const int ks = cdiv(cdiv(K, n), 64) * 64, nn = cdiv(K, ks);
            if (nn != n) continue;
            if (in.tt && (int64_t)ks * in.ldmax * 2 >= in.tt_span) continue;
            int g = ncu / nn / 8 * 8;
            if (g < 8) g = 8;
            if (g > cdiv(tiles, 8) * 8) g = cdiv(tiles, 8) * 8;
            const int per_wg = cdiv(cdiv(tiles, 8), g / 8);
            const double rounds = (double)cdiv(g * nn, ncu);           // (more workgroups than compute units: they queue)
            const double t = rounds * per_wg * ((ks / in.stage_k) * in.stage_us[mi] + in.epi_us[mi]) + 3.0 +
                             (nn > 1 ? (nn + 1.0) * M * (double)N * 4.0 / 3.5e6 + 8.0 : 0.0);
            if (t < best * 0.98) { best = t; best_mi = mi; best_ns = nn; best_g = g; }
        }
    }
    if (best > 1e29) {      // (an override that no candidate met: one slice of 256-row tiles)
        if (in.tt && (int64_t)K * in.ldmax * 2 >= in.tt_span) return PersistPlan{0, 0, 0, 0};
        best_mi = 4; best_ns = 1;
        best_g = cdiv(cdiv(M, 256) * ntn, 8) * 8;
        if (best_g > ncu) best_g = ncu;
    }
    const int ksplit = (best_ns > 1) ? cdiv(cdiv(K, best_ns), 64) * 64 : K;
    return PersistPlan{best_mi, (best_ns > 1) ? cdiv(K, ksplit) : 1, ksplit, best_g};
}

int splitk_reduce(hipStream_t stream, const float* slabs, int nsplit, int M, int N, float* C, int64_t ldc, RowMap cmap,
                  const float* bias, bool accumulate);

// Plan, launch and combine one call (the operands already checked by the caller).  in.ws_floats must be 0 without splitk_ws.
// refusal = the caller's message for a transposed image that cannot be sliced (arguments: its bytes, splitk_ws_floats);
// launch(mi, grid, args) starts the caller's kernel of tile height 64 mi.
template <class Launch>
static int launch_persistent_gemm(hipStream_t stream, const PersistPlanIn& in, const unsigned short* A, int64_t lda, const unsigned short* B,
                                  int64_t ldb, float* C, int64_t ldc, RowMap cmap, const float* bias, bool accumulate, float* splitk_ws,
                                  size_t splitk_ws_floats, const char* kernel_name, const char* refusal, Launch launch) {
    // option "cu_reserve" = n: plan the persistent grids for n compute units fewer.  A launch is sized to ONE workgroup per compute
    // unit with a static share of the tiles each; a long-lived foreign kernel on some of the units (a communication kernel of a
    // data-parallel run) makes the workgroups that find no unit wait for a whole share (multi-GPU).
    const PersistPlan plan = plan_persistent_gemm(in, planned_compute_units());
    S2VT_REQUIRE(plan.mi, refusal, (long long)((int64_t)in.K * in.ldmax * 2), splitk_ws_floats);
    PersistGemmArgs p;
    p.M = in.M; p.N = in.N; p.K = in.K;
    p.A = A; p.lda = lda;
    p.B = B; p.ldb = ldb;
    p.C = C; p.ldc = ldc; p.cmap = cmap; p.bias = bias; p.accumulate = accumulate ? 1 : 0;
    p.ntm = cdiv(in.M, 64 * plan.mi); p.ntn = cdiv(in.N, 256);
    p.ksplit = plan.ksplit;
    p.slabs = (plan.nsplit > 1) ? splitk_ws : nullptr;
    launch(plan.mi, dim3(plan.grid, plan.nsplit), p);
    S2VT_LAUNCH_CHECK(kernel_name);
    if (plan.nsplit > 1) return splitk_reduce(stream, splitk_ws, plan.nsplit, in.M, in.N, C, ldc, cmap, bias, accumulate);
    return 0;
}

}  // namespace s2vt
