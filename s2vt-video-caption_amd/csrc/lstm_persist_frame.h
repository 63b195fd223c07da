// The frame the four persistent recurrence kernels share - lstm_seq_{fwd,bwd}_bf16_persist_kernel (lstm_persist.hip) and
// lstm_seq_{fwd,bwd}_x3_persist_kernel (lstm_persist_x3.hip): 32-row chains x 16 or 32 hidden units per workgroup, one hand-off
// counter per chain polled with a bounded spin, two layers side by side in one launch, XCD-aware block dealing; on the host the
// chain planner, the capacity rule, the XCD plan and the launcher.  What differs between the kernels - the W_hh slice and its
// register pinning, loader and fragment addressing, every MFMA / request / counted-wait schedule, the hand-off stores and who
// drains them - stays in their own files.
#pragma once
#include <mutex>

#include "common.h"
#include "kernels.h"

namespace s2vt {

constexpr int PF_SR = 32;                         // batch rows per sub-step (= per chain)
constexpr int PF_MAXNS = 4;                       // chains per workgroup, at most
constexpr unsigned long long PF_SPIN_TICKS = 100000000ull;     // 1 s of the 100-MHz wall clock

// ============================================================================================================== device
// Everything here is __forceinline__ and issues its memory operations in the order it is written: the kernels' counted
// vmcnt / lgkmcnt waits depend on the number and order of the operations in front of them.
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned int gu32;

__device__ __forceinline__ unsigned short f2bf_rn(float x) {
    unsigned int u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// 16 bytes per lane, global -> LDS, sc1: the hand-off loads
#ifdef S2VT_EXPERIMENT_PLAIN_LOADS      // timing experiment only (tools/bench_bptt_stamps.py): what would hand-off loads without sc1 cost?
#define PF_LOAD_AUX 0                   // (an experiment build: the switch applies to all four kernels)
#else
#define PF_LOAD_AUX 16 /* sc1 */
#endif
__device__ __forceinline__ void glds16_sc1(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, PF_LOAD_AUX);
}
#define PF_DSR(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(ADDR), "n"(OFF))
// workgroup barrier WITHOUT the vmcnt(0) drain __syncthreads() implies: global loads/stores stay in flight across it
#define PF_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// one lane waits for *cnt >= target (relaxed agent-scope = sc1 loads); false on time-out
__device__ __forceinline__ bool spin_until(const unsigned int* cnt, unsigned int target) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        const unsigned int v = __hip_atomic_load((gu32*)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v >= target) return true;
        if (__builtin_amdgcn_s_memrealtime() - t0 > PF_SPIN_TICKS) return false;
        __builtin_amdgcn_s_sleep(2);
    }
}
// The wait for a chain: lane 0 polls, the workgroup meets at a barrier.  false: timed out (*err is set) - the caller returns.
__device__ __forceinline__ bool chain_arrived(const unsigned int* cnt, unsigned int target, int* err, int& s_flag) {
    if (threadIdx.x == 0) {
        const bool ok = spin_until(cnt, target);
        s_flag = ok ? 1 : 0;
        if (!ok) atomicExch(err, 1);
    }
    PF_BARRIER();
    return s_flag != 0;
}
// the counter of the 32-row chain that starts at batch row rbase: one per chain, whatever NS a launch uses, so launches of one
// layer with different NS continue each other (32 counters apart: a cache line of its own)
__device__ __forceinline__ unsigned int* chain_counter(unsigned int* sync, int rbase) { return sync + (rbase / PF_SR) * 32; }

// Which role a block plays: (layer, workgroup index inside the layer = rg * nC + cs).  xg == 0: blocks [0, na) are layer A in
// order, the rest layer B.  xg = G > 0 (XCD-aware, plan_xcd): the hardware deals workgroups to the 8 XCDs round-robin (block b ->
// XCD b % 8, speed only - nothing depends on it for correctness); a GROUP is the nC column slices of one (layer, row group), i.e.
// the workgroups that read the SAME rows in every sub-step and exchange one chain's tiles, and group g is dealt to the XCDs
// {g, g + G, ..}: its rows then enter 8/G L2s instead of all eight, a line is shared by nC * G / 8 readers of one L2 instead of
// nC / 8, and a consumer's sc1 loads find the tile in the L2 its producers wrote through.  A padded grid (XCD_PADDED) has
// 8 * ceil(nC / (8 / G)) blocks; the few whose slice index falls past nC are idle (-1) and exit at once: nobody waits for them,
// the counters count the nC real slices.
__device__ __forceinline__ int persist_role(int bid, int na, int nC, int xg, bool& layer_b) {
    if (xg <= 0) { layer_b = bid >= na; return layer_b ? bid - na : bid; }
    const int x = bid & 7, q = bid >> 3, per = 8 / xg;
    const int g = x % xg, cs = q * per + x / xg;
    const int rgs = na / nC;                         // row groups of layer A (= of layer B: the launcher checked)
    layer_b = g >= rgs;
    return cs < nC ? (layer_b ? g - rgs : g) * nC + cs : -1;
}

// The cell role of a thread: 2 adjacent units (unit, unit + 1 = u0 + ul ..) of one row of the sub-step, the same in every step.
template <int UN>
struct CellLane {
    int row, ul, unit;
    bool ok0, ok1;          // unit, unit + 1 < H
    bool vec;               // 8-byte accesses: both units valid and rows 8-byte aligned
    __device__ __forceinline__ CellLane(int tid, int u0, int H)
        : row(tid / (UN / 2)), ul((tid % (UN / 2)) * 2), unit(u0 + ul), ok0(unit < H), ok1(unit + 1 < H), vec(ok1 && ((H & 1) == 0)) {}
    __device__ __forceinline__ bool ok(int j) const { return j ? ok1 : ok0; }
    // q = address of the first unit's value.  A pair as a whole (the caller knows it is valid or not as a whole) ...
    static __device__ __forceinline__ f32x2 load_pair(const float* q, bool ok) { return *reinterpret_cast<const f32x2*>(ok ? q : g_zero4); }
    static __device__ __forceinline__ void store_pair(float* q, f32x2 v) { *reinterpret_cast<f32x2*>(q) = v; }
    // ... or as two guarded scalars where H is odd / the pair straddles H; rok: the row (and whatever else) is valid
    __device__ __forceinline__ f32x2 load(const float* q, bool rok) const {
        if (vec) return load_pair(q, rok);
        f32x2 v;
        v[0] = *((rok && ok0) ? q : g_zero4);
        v[1] = *((rok && ok1) ? q + 1 : g_zero4);
        return v;
    }
    __device__ __forceinline__ void store(float* q, f32x2 v) const {      // (the caller checked the row)
        if (vec) { store_pair(q, v); return; }
        if (ok0) q[0] = v[0];
        if (ok1) q[1] = v[1];
    }
    // the state a launch takes over from the one before it: the valid part of the pair (the caller checked the row)
    __device__ __forceinline__ f32x2 carry(const float* q) const {
        f32x2 v = {0.f, 0.f};
        if (ok0) v[0] = q[0];
        if (ok1) v[1] = q[1];
        return v;
    }
};

// sigmoid / tanh on the hardware exp and reciprocal (1 ulp each): absolute error ~2e-7, far below the bf16 rounding of
// the operands the bf16 kernels work on; the split-precision kernels use the fp32 timestep kernels' (common.h)
struct ActFast {
    static __device__ __forceinline__ float sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
    static __device__ __forceinline__ float tanh(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f; }
};
struct ActExact {
    static __device__ __forceinline__ float sigmoid(float x) { return sigmoidf_(x); }
    static __device__ __forceinline__ float tanh(float x) { return tanhf_(x); }
};

// One cell forward: pre-activations -> activated gates {i, f, g, o}, c_t (zero where !ok), h_t.  h_t is NOT masked here: the
// split-precision kernel zeroes it on pad lanes, the bf16 kernel does not.
template <class Act>
__device__ __forceinline__ void cell_forward(float pi, float pf, float pg, float po, float cprev, bool ok, float (&gate)[4], float& c, float& h) {
    gate[0] = Act::sigmoid(pi);
    gate[1] = Act::sigmoid(pf);
    gate[2] = Act::tanh(pg);
    gate[3] = Act::sigmoid(po);
    c = ok ? gate[1] * cprev + gate[0] * gate[2] : 0.f;
    h = gate[3] * Act::tanh(c);
}
// One cell of the BPTT: dh (everything that arrives at h_t), the activated gates, c_t, c_{t-1}, dL/dc carried from t + 1 ->
// dG {i, f, g, o} and the carry for t - 1.  Nothing is masked here: the split-precision kernel masks every dg, the bf16 kernel
// the carry and its packed store.
template <class Act>
__device__ __forceinline__ void cell_backward(float dh, float ig, float fg, float gg, float og, float c, float cprev, float dcin,
                                              float (&dg)[4], float& dcn) {
    const float tc = Act::tanh(c);
    const float dc = dh * og * (1.0f - tc * tc) + dcin;
    const float d_o = dh * tc;
    dg[0] = dc * gg * ig * (1.0f - ig);
    dg[1] = dc * cprev * fg * (1.0f - fg);
    dg[2] = dc * ig * (1.0f - gg * gg);
    dg[3] = d_o * og * (1.0f - og);
    dcn = dc * fg;
}

// ================================================================================================================ host
// All workgroups of a launch must be co-resident: they wait for each other inside it.
inline int coresident_capacity(const void* kernel, int block) {
    struct Entry { int dev; const void* k; int cap; };
    static Entry cache[32];
    static int n = 0;
    static std::mutex mu;               // the forward (caller's thread) and the backward (autograd's thread) both size launches
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    for (int i = 0; i < n; ++i)
        if (cache[i].dev == dev && cache[i].k == kernel) return cache[i].cap;
    int cus = 0, occ = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, block, 0) != hipSuccess) occ = 0;
    (void)hipGetLastError();
    const int cap = (cus > 0 && occ > 0) ? cus * occ : 0;
    if (n < 32) cache[n++] = Entry{dev, kernel, cap};
    return cap;
}
// ... capped at the kernel's design point
template <class Kernel>
static int persist_capacity_of(Kernel* kernel, int block, int design) {
    const int cap = coresident_capacity(reinterpret_cast<const void*>(kernel), block);
    return cap < design ? cap : design;
}

// Chains per workgroup of a layer of B rows and nC column slices such that its workgroups number at most `lim` (0: they cannot):
// row groups (one 32-row chain each) are merged two by two until they do.  lim = the capacity for a launch with ONE layer, half
// of it for a layer of a pair.  rg_bound: at most 64 row groups (lstm_persist_sync_bytes() and the bf16 kernels' images).
// pure: no HIP call, no global
static inline int plan_chains(int B, int nC, int lim, bool rg_bound) {
    int R = B / PF_SR, ns = 1;
    while (R * nC > lim && ns < PF_MAXNS && R % 2 == 0) { R /= 2; ns *= 2; }
    return (R * nC <= lim && (!rg_bound || R <= 64)) ? ns : 0;
}

// The launcher's side of persist_role(): G groups (xg) and the grid, or xg = 0 and the plain order [na | nb].  A group is the nC
// column slices of one (layer, row group); dealing needs both layers of one shape and a G that divides the 8 XCDs.
//   XCD_EXACT  (bf16 BPTT): only when the groups fill the XCDs exactly - no padding;
//   XCD_PADDED (both split-precision kernels): the grid is padded to 8 * ceil(nC / (8 / G)) blocks if that still fits `cap`.
// pure: no HIP call, no global
enum XcdPolicy { XCD_NONE, XCD_EXACT, XCD_PADDED };
struct XcdPlan { int xg, grid; };
static inline XcdPlan plan_xcd(XcdPolicy policy, int na, int nb, int nC, bool same_shape, int cap) {
    XcdPlan plan = {0, na + nb};
    if (policy == XCD_NONE || !same_shape || nC <= 0) return plan;
    const int G = (na + nb) / nC;
    if (!(G > 0 && G <= 8 && 8 % G == 0)) return plan;
    if (policy == XCD_EXACT) {
        if (na % nC == 0 && nb % nC == 0 && (!nb || nb == na) && (na + nb) % 8 == 0) plan.xg = G;
    } else {
        const int padded = 8 * cdiv(nC, 8 / G);
        if (padded <= cap) { plan.xg = G; plan.grid = padded; }
    }
    return plan;
}

// what a kernel file's prep reports about a layer: hidden units per workgroup, capacity of the kernel it will run
struct PersistLayer { int un, cap; };

// One layer (b == nullptr) or two layers side by side in one launch.  BPTT: the launch runs backwards in time (the sequence's
// first block is then t1 == T, not t0 == 0).
//   prep(args, single, &layer)  the file's argument checks; sets NS / RB (single: a launch with ONE layer may take the whole device)
//   pair(a, b, la, lb)          the file's extra requirement on a pair: nullptr, or the message of the one that failed
//   launch(grid, a, b, na, xg, la)
template <bool BPTT, class Args, class Prep, class Pair, class Launch>
static int launch_persistent_layers(hipStream_t stream, Args a, const Args* b, XcdPolicy policy, const char* who, const char* counters_msg,
                                    const char* kernel_name, Prep prep, Pair pair, Launch launch) {
    int rc;
    PersistLayer la, lb;
    if ((rc = prep(a, b == nullptr, &la))) return rc;
    Args bb = b ? *b : a;
    lb = la;
    if (b) {
        if ((rc = prep(bb, false, &lb))) return rc;
        const char* why = (bb.sync == a.sync) ? counters_msg : pair(a, bb, la, lb);
        S2VT_REQUIRE(!why, "%s", why);
    }
    const int nC = cdiv(a.H, la.un);
    const int na = (a.B / a.RB) * nC, nb = b ? (bb.B / bb.RB) * cdiv(bb.H, lb.un) : 0;
    S2VT_REQUIRE(na + nb <= la.cap, "%s: %d workgroups would not be co-resident (device capacity %d)", who, na + nb, la.cap);
    // the hand-off counters count finished timesteps of the whole sequence: zeroed with its first block only (a memset
    // is a 5-us kernel of its own on this stream: 28 of them per train step when every launch zeroed its counters)
    auto first = [](const Args& x) {
        if constexpr (BPTT) return x.t1 == x.T;
        else return x.t0 == 0;
    };
    if (first(a)) S2VT_HIP(hipMemsetAsync(a.sync, 0, lstm_persist_sync_bytes(), stream));
    if (b && first(bb)) S2VT_HIP(hipMemsetAsync(bb.sync, 0, lstm_persist_sync_bytes(), stream));
    const XcdPlan x = plan_xcd(policy, na, nb, nC, !b || (bb.B == a.B && bb.H == a.H), la.cap);
    launch(dim3(x.grid), a, bb, na, x.xg, la);
    S2VT_LAUNCH_CHECK(kernel_name);
    return 0;
}

}  // namespace s2vt
