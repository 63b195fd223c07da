// The policy of STOCHASTIC BEAM SEARCH on the device (S2VT.sample_distinct; Kool, van Hoof, Welling, ICML 2019; not in the reference):
// W pairwise distinct captions per clip, drawn WITHOUT REPLACEMENT from the model's distribution over whole sentences, in the order a
// sequential without-replacement sampler would draw them.  On the row protocol of beam_policy.hip (fixed rows r = b * W + slot of the
// depth step, nothing compacted, nothing crosses PCIe per depth; depth = 1 initialise, 2..D consume step depth - 1, 0 consume step D).
//
// Definition (include/s2vt_hip.h "stochastic beam"; tests/sbs_ref.py restates it in numpy), per clip: W slots, each
// empty, live or finished, carrying phi (fp32: the sum of its words' log-probs), G (fp64: its perturbed score), a back-trace node and
// a length.  Start: slot 0 live with phi = 0, G = 0, <sos>, the encoder state; kappa = -inf.  For t = 1..D the depth step's head
// (gumbel_top.hip) gives every live slot j its 20 children by perturbed log-prob g, best first: top_ix, top_lp, top_g.  Child f of
// slot j: phi' = phi_j + top_lp[f] (one fp32 add, -0 folded to +0), and with Z = top_g[0], g = top_g[f] widened exactly to fp64
//     d = g - Z;   l = d > -ln 2 ? log(-expm1(d)) : log1p(-exp(d));   u = (G_j - g) + l;   G~ = (G_j - max(u, 0)) - log1p(exp(-|u|))
// - the stable form of -log(exp(-G_j) - exp(-Z) + exp(-g)): the children's perturbed scores conditioned on their maximum being the
// parent's G_j.  f = 0 gives G~ = G_j exactly; every G~ <= G_j.  A finished slot is one candidate, itself, with its own G.  Candidate
// index c = j * 20 + f (f = 0 for a finished slot).  The min(W, count) best by (G~ descending, c ascending) become slots 0, 1, ... in
// that order: a finished candidate as it is, a child with a new back-trace node - <eos> finishes it with length t, anything else is
// live with row_state its parent's row and row_tok its word.  kappa = max(kappa, the best G~ that was not selected).  A clip with no
// live slot after the walk is FROZEN: its candidates are its finished slots, all selected, in order - nothing of it can change.
// After depth D the live slots stay as unfinished samples of length D.  The answer is the W slots in order: non-increasing G.
//
// Fan-out 20 is exact: G~ is increasing in g for one parent, so a parent's selected children are a prefix of its g-order; at most
// W <= 8 are selected and its best unselected child is at most its 9th.
//
// One WAVE per clip.  All W * 20 candidates are computed once (c over the lanes, three per lane, G~ in fp64 registers); selection is
// W + 1 rounds of a wave-wide max on the pair (order-preserving image of the fp64 G~, c) - beam_wave.h, bc_wave_max_f64c: the 32-bit
// keyed max of the cumulative policy has no room for an fp64 - the last round being the threshold's.  The pair is unique per
// candidate, so a round has exactly one winner; the owner clears its key, and G~ is read back out of the winning key (the image is
// invertible), no shuffle of the value.  The walk is lane 0's: at most 8 slots, reading the old slots from LDS copies.  Rows of slots
// that are not live are cleared (state 0 / token 0) as beam_policy.hip clears a frozen sample's.  The frozen-clip counter is the
// int32 at byte 0 of the state (beam.py polls it).
#include <math.h>

#include "beam_wave.h"
#include "common.h"
#include "kernels.h"

namespace s2vt {

enum { SBS_EMPTY = 0, SBS_LIVE = 1, SBS_FINISHED = 2 };

struct SbsP {
    int B, W, D, NN, sos, eos, depth;
    int* done_count; int* done; int* n_nodes;
    int* node_tok; int* node_prev;                           // [B][NN]: every selected child, for the back-trace
    int* kind; float* phi; double* G; int* nid; int* len;    // [B][W]
    double* kappa;                                           // [B]
    const int* top_ix; const float* top_lp; const float* top_g;        // [B*W][20] of the depth just stepped, best g first
    int* row_b; int* row_state; int* row_tok;                // [B*W] for the next depth step
};

// the child's perturbed score (the definition at the top); every operation is an fp64 add / subtract or a libm call: nothing contracts
__device__ __forceinline__ double sbs_child(double Gj, double Z, double g) {
    const double d = g - Z;
    const double l = d > -0.6931471805599453 ? log(-expm1(d)) : log1p(-exp(d));
    const double u = (Gj - g) + l;
    return (Gj - fmax(u, 0.0)) - log1p(exp(-fabs(u)));
}
__device__ __forceinline__ double sbs_unordered64(unsigned long long k) {
    const unsigned long long u = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__global__ __launch_bounds__(64) void sbs_policy_kernel(SbsP q) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int W = q.W;
    int* ntok = q.node_tok + (int64_t)b * q.NN;
    int* nprev = q.node_prev + (int64_t)b * q.NN;
    if (q.depth == 1) {            // slot 0: the empty hypothesis on the encoder state (row b of the first state table)
        if (lane < W) {
            const bool first = lane == 0;
            const int e = b * W + lane;
            q.kind[e] = first ? SBS_LIVE : SBS_EMPTY; q.phi[e] = 0.0f; q.G[e] = 0.0; q.nid[e] = first ? 0 : -1; q.len[e] = 0;
            q.row_b[e] = b; q.row_state[e] = first ? b : 0; q.row_tok[e] = first ? q.sos : 0;
        }
        if (lane == 0) {
            q.done[b] = 0; q.n_nodes[b] = 1; q.kappa[b] = -INFINITY;
            ntok[0] = q.sos; nprev[0] = -1;
        }
        return;
    }
    if (q.done[b]) return;         // frozen: its rows were cleared when it stopped
    const int t = q.depth == 0 ? q.D : q.depth - 1;
    __shared__ int o_kind[BC_MAXBW], o_nid[BC_MAXBW], o_len[BC_MAXBW];
    __shared__ float o_phi[BC_MAXBW];
    __shared__ double o_G[BC_MAXBW];
    if (lane < BC_MAXBW) {
        const bool in = lane < W;
        const int e = b * W + (in ? lane : 0);
        o_kind[lane] = in ? q.kind[e] : SBS_EMPTY; o_nid[lane] = in ? q.nid[e] : -1; o_len[lane] = in ? q.len[e] : 0;
        o_phi[lane] = in ? q.phi[e] : 0.0f; o_G[lane] = in ? q.G[e] : 0.0;
    }
    __syncthreads();
    // ---- candidates c = slot * 20 + f: key 0 = none (an empty slot, f > 0 of a finished one)
    unsigned long long key[BC_CPL];
#pragma unroll
    for (int k = 0; k < BC_CPL; ++k) {
        const int c = lane + 64 * k;
        key[k] = 0;
        if (c < W * BC_FAN) {
            const int slot = c / BC_FAN, f = c - slot * BC_FAN;
            const int kd = o_kind[slot];
            if (kd == SBS_LIVE) {
                const int64_t r = (int64_t)(b * W + slot) * BC_FAN;
                key[k] = bc_ordered64(sbs_child(o_G[slot], (double)q.top_g[r], (double)q.top_g[r + f]));
            } else if (kd == SBS_FINISHED && f == 0) {
                key[k] = bc_ordered64(o_G[slot]);
            }
        }
    }
    // ---- selection: W rounds, then one more for the threshold; every lane ends with the same lists
    int selc[BC_MAXBW];
    double selG[BC_MAXBW];
    double best_out = -INFINITY;
    bool have_out = false;
#pragma unroll
    for (int i = 0; i <= BC_MAXBW; ++i) {
        if (i < BC_MAXBW) { selc[i] = -1; selG[i] = 0.0; }
        if (i <= W) {
            unsigned long long mk = 0;
            int mc = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < BC_CPL; ++k)
                if (key[k] > mk) { mk = key[k]; mc = lane + 64 * k; }          // (ascending c: the first of equal keys stays)
            bc_wave_max_f64c(mk, mc);
            if (mk != 0) {
#pragma unroll
                for (int k = 0; k < BC_CPL; ++k) key[k] = (lane + 64 * k == mc) ? 0 : key[k];
                const double gt = sbs_unordered64(mk);
                if (i < W) {
                    if (i < BC_MAXBW) { selc[i] = mc; selG[i] = gt; }
                } else {
                    best_out = gt; have_out = true;
                }
            }
        }
    }
    if (lane != 0) return;
    // ---- the walk: the selected candidates become slots 0, 1, ... in order
    int nn = q.n_nodes[b], nlive = 0;
#pragma unroll
    for (int i = 0; i < BC_MAXBW; ++i) {
        if (i >= W) break;
        const int e = b * W + i;
        int kd = SBS_EMPTY, id = -1, ln = 0, rs = 0, rt = 0;
        float ph = 0.0f;
        double G = 0.0;
        const int c = selc[i];
        if (c >= 0) {
            const int j = c / BC_FAN, f = c - j * BC_FAN;
            G = selG[i];
            if (o_kind[j] == SBS_FINISHED) {
                kd = SBS_FINISHED; ph = o_phi[j]; id = o_nid[j]; ln = o_len[j];
            } else {
                const int64_t r = (int64_t)(b * W + j) * BC_FAN + f;
                const int v = q.top_ix[r];
                const float s = o_phi[j] + q.top_lp[r];
                ph = s == 0.0f ? 0.0f : s;                      // (-0 and +0 are one sum)
                id = nn < q.NN ? nn : q.NN - 1;                 // (NN = 1 + D * W: never exceeded)
                ntok[id] = v; nprev[id] = o_nid[j];
                ++nn;
                ln = t;
                if (v == q.eos) {
                    kd = SBS_FINISHED;
                } else {
                    kd = SBS_LIVE; rs = b * W + j; rt = v;
                    ++nlive;
                }
            }
        }
        q.kind[e] = kd; q.phi[e] = ph; q.G[e] = G; q.nid[e] = id; q.len[e] = ln;
        q.row_state[e] = rs; q.row_tok[e] = rt;
    }
    q.n_nodes[b] = nn < q.NN ? nn : q.NN;
    if (have_out) q.kappa[b] = fmax(q.kappa[b], best_out);
    if (nlive == 0) {
        q.done[b] = 1;
        atomicAdd(q.done_count, 1);
    }
}

// back-trace of the W slots: one thread per (clip, slot)
__global__ void sbs_result_kernel(SbsP q, int32_t* out, int32_t* out_len, float* out_lp, float* out_g, float* out_kappa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.B * q.W) return;
    const int b = i / q.W;
    const int* ntok = q.node_tok + (int64_t)b * q.NN;
    const int* nprev = q.node_prev + (int64_t)b * q.NN;
    int32_t* o = out + (int64_t)i * q.D;
    const bool have = q.kind[i] != SBS_EMPTY;                  // (always after depth 1: a live slot has 20 >= W children)
    int len = have ? q.len[i] : 0;
    len = len < 0 ? 0 : (len < q.D ? len : q.D);
    for (int p = len; p < q.D; ++p) o[p] = q.eos;
    int node = have ? q.nid[i] : -1;
    for (int p = len - 1; p >= 0 && node > 0 && node < q.NN; --p, node = nprev[node]) o[p] = ntok[node];
    out_len[i] = len;
    out_lp[i] = have ? q.phi[i] : -INFINITY;
    out_g[i] = have ? (float)q.G[i] : -INFINITY;
    if (i == b * q.W) out_kappa[b] = (float)q.kappa[b];
}

static SbsP carve_sbs(int B, int W, int D, void* base, size_t* bytes) {
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) { off = align_up(off, 256); char* r = base ? p + off : nullptr; off += n; return r; };
    const size_t slots = (size_t)B * W;
    SbsP q = {};
    q.B = B; q.W = W; q.D = D; q.NN = 1 + D * W;
    q.done_count = reinterpret_cast<int*>(take(sizeof(int)));          // (first: the frozen-clip counter is at byte 0)
    q.done = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.n_nodes = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.node_tok = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * q.NN));
    q.node_prev = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * q.NN));
    q.kind = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.phi = reinterpret_cast<float*>(take(sizeof(float) * slots));
    q.G = reinterpret_cast<double*>(take(sizeof(double) * slots));
    q.nid = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.len = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.kappa = reinterpret_cast<double*>(take(sizeof(double) * B));
    if (bytes) *bytes = align_up(off, 256);
    return q;
}

static bool sbs_dims_ok(int B, int W, int D) {
    return B > 0 && W >= 1 && W <= BC_MAXBW && D >= 1 && (int64_t)B * (1 + (int64_t)D * W) < (1ll << 28);
}

}  // namespace s2vt

using namespace s2vt;

extern "C" {

size_t s2vt_sbs_bytes(int32_t B, int32_t n_samples, int32_t max_depth) {
    if (!sbs_dims_ok(B, n_samples, max_depth)) return 0;
    size_t n = 0;
    carve_sbs(B, n_samples, max_depth, nullptr, &n);
    return n;
}

int s2vt_sbs_step(int32_t B, int32_t n_samples, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, int32_t depth, void* state,
                  size_t state_bytes, const int32_t* top_ix, const float* top_lp, const float* top_g, int32_t* row_b, int32_t* row_state,
                  int32_t* row_tok, void* stream) {
    S2VT_REQUIRE(sbs_dims_ok(B, n_samples, max_depth) && depth >= 0 && depth <= max_depth && state && row_b && row_state && row_tok,
                 "s2vt_sbs_step: null/invalid argument (B >= 1, 1 <= n_samples <= %d, max_depth >= 1, 0 <= depth <= max_depth)", BC_MAXBW);
    S2VT_REQUIRE(depth == 1 || (top_ix && top_lp && top_g), "s2vt_sbs_step: the step's top-20 arrays are needed from depth 2 on");
    size_t need = 0;
    SbsP q = carve_sbs(B, n_samples, max_depth, state, &need);
    S2VT_REQUIRE(state_bytes >= need, "s2vt_sbs_step: state %zu < %zu bytes", state_bytes, need);
    q.sos = sos_ix; q.eos = eos_ix; q.depth = depth;
    q.top_ix = top_ix; q.top_lp = top_lp; q.top_g = top_g;
    q.row_b = row_b; q.row_state = row_state; q.row_tok = row_tok;
    hipStream_t st = (hipStream_t)stream;
    if (depth == 1) S2VT_HIP(hipMemsetAsync(q.done_count, 0, sizeof(int), st));
    hipLaunchKernelGGL(sbs_policy_kernel, dim3(B), dim3(64), 0, st, q);
    S2VT_LAUNCH_CHECK("sbs_policy_kernel");
    return 0;
}

int s2vt_sbs_result(int32_t B, int32_t n_samples, int32_t max_depth, int32_t eos_ix, void* state, size_t state_bytes, int32_t* out_tokens,
                    int32_t* out_len, float* out_logprob, float* out_perturbed, float* out_kappa, void* stream) {
    S2VT_REQUIRE(sbs_dims_ok(B, n_samples, max_depth) && state && out_tokens && out_len && out_logprob && out_perturbed && out_kappa,
                 "s2vt_sbs_result: null/invalid argument (B >= 1, 1 <= n_samples <= %d, max_depth >= 1)", BC_MAXBW);
    size_t need = 0;
    SbsP q = carve_sbs(B, n_samples, max_depth, state, &need);
    S2VT_REQUIRE(state_bytes >= need, "s2vt_sbs_result: state %zu < %zu bytes", state_bytes, need);
    q.eos = eos_ix;
    hipLaunchKernelGGL(sbs_result_kernel, dim3(cdiv(B * n_samples, 64)), dim3(64), 0, (hipStream_t)stream, q, out_tokens, out_len,
                       out_logprob, out_perturbed, out_kappa);
    S2VT_LAUNCH_CHECK("sbs_result_kernel");
    return 0;
}

}  // extern "C"
