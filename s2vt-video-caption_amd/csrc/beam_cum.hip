// Cumulative-score beam search (S2VT.forward(mode='beam'); not in the reference): the search policy ON THE DEVICE, for all samples of a
// batch at once, on the row protocol of beam_queue.hip (fixed rows r = b * beam_width + slot of s2vt_beam_step, nothing compacted,
// nothing crosses PCIe per depth).  Definition, per sample, W = beam_width, D = max_depth:
//   live = [(tokens [], S = 0, <sos>)], pool = []; for t = 1..D:
//     candidates (j, v) of every live slot j and token v score S_j + lp_j[v] (one fp32 add);
//     the min(W, count) best by (S descending, j ascending, v ascending) are walked in that order: v == <eos> enters the pool with
//     score S / t**alpha, anything else becomes the next live slot; live empty -> done; t == D -> every live hypothesis enters the
//     pool with S / D**alpha (no <eos> appended), done.
//   pool is kept ordered by (score descending, insertion ascending), its best W entries only; the answer is its first n_best.
// Fan-out 20 is exact for W <= 8: a candidate outside its parent's top W has W better candidates of the SAME parent in front of it.
// top_ix rows are in ascending token order, so the candidate index c = j * 20 + f already IS (j ascending, v ascending): one 64-bit
// key (order-preserving score bits high, ~c low) and W rounds of a wave-wide max select with the tie rule, no replay path.
//
// Early stop.  A sample is frozen after a depth when its pool holds W entries and pool[W-1].score >= live[0].S / D**alpha.  This
// cannot change an output: the kernel clamps every log-prob to <= 0 (fminf(lp, 0)), so S never rises along a hypothesis and live[0]
// (the first selected, unfinished candidate) holds the largest live S.  Any hypothesis finished later has S' <= live[0].S <= 0 and a
// length t' <= D; the divisor table is non-decreasing in the length for alpha >= 0 (pow and the rounding to fp32 are monotone), so
// S' / t'**alpha <= S' / D**alpha <= live[0].S / D**alpha, and the rounded fp32 quotients keep that order (division is monotone in
// both operands here).  Its score is therefore <= pool[W-1].score, and an equal score loses to the earlier insertion: it never
// enters the best W.
//
// Constrained form (S2VT.beam_constrained; include/s2vt_hip.h "constrained beam").  The depth step's fan-out head edits a slot's logits
// row by the rules of the constrained draw with the slot's own words as history, then takes log_softmax and the top 20 of the EDITED
// row (ce.hip).  The policy above is unchanged; it only has to keep every live slot's words where that head can read them:
// beam_cum_kernel<true> carries hist[2][B][W][D] int32 in its state, ping-ponged by depth parity - the slots that are live after
// depth t (t words each) are in buffer t & 1.  When candidate (j, v) becomes live slot s, the wave copies parent j's t-1 words from
// buffer (t-1) & 1 into slot s of buffer t & 1 (lanes over the words: W * (t-1) independent loads for a wave whose lanes 1..63 are
// otherwise idle behind the selection) and appends v.  Both buffers are zeroed at depth 1, and nothing else is ever written to
// them: the row of an unused slot or of a frozen sample stays readable - defined words in [0, V) - and its fan-out is never consumed.
// Chosen over walking node_prev inside the head: that is t DEPENDENT global loads in front of every row's load, on the critical path
// of every depth.  The early stop holds as it stands: its proof needs lp <= 0 only, which the log_softmax of any edited row gives (and
// the clamp enforces).  Fan-out 20 stays exact for W <= 8: the top 20 are taken from the edited row, on which the argument above
// runs unchanged; a banned word is -inf there and is never among the 20 while V >= 20 + D + n_banned + 1 (checked by the callers).
#include <math.h>

#include <map>
#include <mutex>

#include "beam_wave.h"
#include "common.h"
#include "kernels.h"

namespace s2vt {

struct BeamC {
    int B, bw, D, NN, sos, eos, depth;         // depth: 1 = initialise; 2..D = consume step depth-1; 0 = consume step D
    int* done_count; int* done; int* n_live; int* n_nodes;
    int* node_tok; int* node_prev;                           // [B][NN]: every selected candidate, for the back-trace
    float* live_S; int* live_nid;                            // [B][bw]
    int* pool_n; float* pool_score; int* pool_nid; int* pool_len;      // [B], [B][bw] x 3
    float* powa;                                             // fp32(len ** alpha): double pow, then fp32
    const int* top_ix; const float* top_lp;                  // [B*bw][20] of the depth just stepped
    int* row_b; int* row_state; int* row_tok;                // [B*bw] for the next s2vt_beam_step
    int* hist;                                               // [2][B][bw][D] words of the live slots (the constrained form only)
};

// (bc_ordered / bc_unordered / bc_wave_max, the keyed wave-wide max: beam_wave.h)
// One WAVE per sample.  Keys are distinct (the low word is the candidate index), so every round has exactly one winner.
// HIST: the constrained form - the same policy, and the live slots' words kept in q.hist (the comment at the top).
template <bool HIST>
__global__ __launch_bounds__(64) void beam_cum_kernel(BeamC q) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int bw = q.bw;
    float* lS = q.live_S + b * bw;
    int* lnid = q.live_nid + b * bw;
    int* ntok = q.node_tok + (int64_t)b * q.NN;
    int* nprev = q.node_prev + (int64_t)b * q.NN;
    if (q.depth == 1) {            // live = one empty hypothesis on the encoder state (row b of the first state table)
        if constexpr (HIST) {      // both buffers of the sample: defined words for every slot, live or not
            const int per = bw * q.D;
            for (int i = lane; i < per; i += 64) {
                q.hist[(int64_t)b * per + i] = 0;
                q.hist[((int64_t)q.B + b) * per + i] = 0;
            }
        }
        if (lane == 0) {
            q.done[b] = 0; q.n_live[b] = 1; q.n_nodes[b] = 1; q.pool_n[b] = 0;
            ntok[0] = q.sos; nprev[0] = -1;
            lS[0] = 0.0f; lnid[0] = 0;
            for (int j = 0; j < bw; ++j) {
                q.row_b[b * bw + j] = b;
                q.row_state[b * bw + j] = j == 0 ? b : 0;
                q.row_tok[b * bw + j] = j == 0 ? q.sos : 0;
            }
        }
        return;
    }
    if (q.done[b]) return;         // frozen: its rows were cleared when it stopped
    const int t = q.depth == 0 ? q.D : q.depth - 1;
    const int nl = q.n_live[b];
    const int n = nl * BC_FAN;
    // ---- candidates: c = j * 20 + f, score S_j + min(lp, 0)
    unsigned long long key[BC_CPL];
#pragma unroll
    for (int k = 0; k < BC_CPL; ++k) {
        const int c = lane + 64 * k;
        key[k] = 0;
        if (c < n) {
            const int j = c / BC_FAN;
            float s = lS[j] + fminf(q.top_lp[(int64_t)(b * bw + j) * BC_FAN + (c - j * BC_FAN)], 0.0f);
            s = s == 0.0f ? 0.0f : s;                       // (-0 and +0 are one score)
            key[k] = ((unsigned long long)bc_ordered(s) << 32) | (unsigned int)~(unsigned int)c;
        }
    }
    // ---- selection: W rounds of a wave-wide max; every lane ends with the same list
    const int m = n < bw ? n : bw;
    float selS[BC_MAXBW];
    int selc[BC_MAXBW];
#pragma unroll
    for (int r = 0; r < BC_MAXBW; ++r) {
        if (r < m) {
            unsigned long long mx = 0;
#pragma unroll
            for (int k = 0; k < BC_CPL; ++k) mx = key[k] > mx ? key[k] : mx;
            mx = bc_wave_max(mx);
#pragma unroll
            for (int k = 0; k < BC_CPL; ++k) key[k] = key[k] == mx ? 0 : key[k];
            selS[r] = bc_unordered((unsigned int)(mx >> 32));
            selc[r] = (int)~(unsigned int)mx;
        }
    }
    if (!HIST && lane != 0) return;
    __shared__ int new_parent[HIST ? BC_MAXBW : 1], new_tok[HIST ? BC_MAXBW : 1], new_n[1];
    if (lane == 0) {               // (the constrained form keeps lanes 1..63 for the copy of the words below)
        // ---- walk the selected candidates: <eos> -> pool, anything else -> next live slot
        float pS[BC_MAXBW];
        int pnid[BC_MAXBW], plen[BC_MAXBW], oldnid[BC_MAXBW];
        int pn = q.pool_n[b];
#pragma unroll
        for (int i = 0; i < BC_MAXBW; ++i) {
            const bool in = i < pn;
            pS[i] = in ? q.pool_score[b * bw + i] : 0.0f;
            pnid[i] = in ? q.pool_nid[b * bw + i] : 0;
            plen[i] = in ? q.pool_len[b * bw + i] : 0;
            oldnid[i] = i < nl ? lnid[i] : 0;
        }
        auto pool_insert = [&](float score, int nid, int len) {
            int p = 0;
            while (p < pn && !(score > pS[p])) ++p;             // behind every entry that is not worse: insertion order breaks ties
            if (p >= bw) return;
            const int last = pn < bw ? pn : bw - 1;
            for (int i = last; i > p; --i) { pS[i] = pS[i - 1]; pnid[i] = pnid[i - 1]; plen[i] = plen[i - 1]; }
            pS[p] = score; pnid[p] = nid; plen[p] = len;
            pn = pn < bw ? pn + 1 : bw;
        };
        const float div_t = q.powa[t], div_D = q.powa[q.D];
        float nS[BC_MAXBW];
        int nnid[BC_MAXBW], nrow[BC_MAXBW], ntk[BC_MAXBW];
        int nn = q.n_nodes[b], nnl = 0;
        for (int r = 0; r < m; ++r) {
            const int c = selc[r], j = c / BC_FAN;
            const int v = q.top_ix[(int64_t)(b * bw + j) * BC_FAN + (c - j * BC_FAN)];
            const int id = nn < q.NN ? nn : q.NN - 1;          // (NN = 1 + D * W: never exceeded)
            ntok[id] = v; nprev[id] = oldnid[j];
            ++nn;
            if (v == q.eos) {
                pool_insert(selS[r] / div_t, id, t);
            } else {
                nS[nnl] = selS[r]; nnid[nnl] = id; nrow[nnl] = b * bw + j; ntk[nnl] = v;
                ++nnl;
            }
        }
        q.n_nodes[b] = nn < q.NN ? nn : q.NN;
        if (t == q.D) {                // unfinished at the depth limit: into the pool as they are, no <eos> appended
            for (int i = 0; i < nnl; ++i) pool_insert(nS[i] / div_D, nnid[i], t);
            nnl = 0;
        }
        const bool stop = nnl == 0 || (pn == bw && pS[bw - 1] >= nS[0] / div_D);     // (the early stop: see the proof at the top)
        q.pool_n[b] = pn;
        for (int i = 0; i < pn; ++i) { q.pool_score[b * bw + i] = pS[i]; q.pool_nid[b * bw + i] = pnid[i]; q.pool_len[b * bw + i] = plen[i]; }
        if (stop) {
            nnl = 0;
            q.done[b] = 1;
            atomicAdd(q.done_count, 1);
        }
        q.n_live[b] = nnl;
        for (int j = 0; j < bw; ++j) {
            const bool in = j < nnl;
            if (in) { lS[j] = nS[j]; lnid[j] = nnid[j]; }
            q.row_state[b * bw + j] = in ? nrow[j] : 0;
            q.row_tok[b * bw + j] = in ? ntk[j] : 0;
            if constexpr (HIST) {
                if (in) { new_parent[j] = nrow[j] - b * bw; new_tok[j] = ntk[j]; }
            }
        }
        if constexpr (HIST) new_n[0] = nnl;
    }
    if constexpr (HIST) {
        // ---- the new live slots' words: parent's t-1 words from buffer (t-1) & 1, then the slot's own, into buffer t & 1
        __syncthreads();
        const int per = bw * q.D;
        const int* src = q.hist + ((int64_t)((t - 1) & 1) * q.B + b) * per;
        int* dst = q.hist + ((int64_t)(t & 1) * q.B + b) * per;
        const int nnl = new_n[0];                               // (0 at t == D and for a sample that has just stopped)
        for (int s = 0; s < nnl; ++s) {
            const int* from = src + new_parent[s] * q.D;
            for (int i = lane; i < t - 1; i += 64) dst[s * q.D + i] = from[i];
            if (lane == 0) dst[s * q.D + t - 1] = new_tok[s];
        }
    }
}

// back-trace of the pool's first n_best entries: one thread per (sample, rank)
__global__ void beam_cum_result_kernel(BeamC q, int n_best, int32_t* out, int32_t* out_len, float* out_score) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.B * n_best) return;
    const int b = i / n_best, k = i - b * n_best;
    const int* ntok = q.node_tok + (int64_t)b * q.NN;
    const int* nprev = q.node_prev + (int64_t)b * q.NN;
    int32_t* o = out + (int64_t)i * q.D;
    const bool have = k < q.pool_n[b];                     // (always, once the sample is done)
    int len = have ? q.pool_len[b * q.bw + k] : 0;
    len = len < q.D ? len : q.D;
    for (int p = len; p < q.D; ++p) o[p] = q.eos;
    int node = have ? q.pool_nid[b * q.bw + k] : -1;
    for (int p = len - 1; p >= 0 && node > 0; --p, node = nprev[node]) o[p] = ntok[node];
    out_len[i] = len;
    out_score[i] = have ? q.pool_score[b * q.bw + k] : -INFINITY;
}

static BeamC carve_beamc(int B, int bw, int D, void* base, size_t* bytes, bool hist = false) {
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) { off = align_up(off, 256); char* r = base ? p + off : nullptr; off += n; return r; };
    const size_t slots = (size_t)B * bw;
    BeamC q;
    q.B = B; q.bw = bw; q.D = D; q.NN = 1 + D * bw;
    q.done_count = reinterpret_cast<int*>(take(sizeof(int)));          // (first: the frozen-sample counter is at byte 0)
    q.done = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.n_live = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.n_nodes = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.node_tok = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * q.NN));
    q.node_prev = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * q.NN));
    q.live_S = reinterpret_cast<float*>(take(sizeof(float) * slots));
    q.live_nid = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.pool_n = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.pool_score = reinterpret_cast<float*>(take(sizeof(float) * slots));
    q.pool_nid = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.pool_len = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.powa = reinterpret_cast<float*>(take(sizeof(float) * (size_t)(D + 1)));
    // (last: the constrained form's state is the plain one with the words behind it - s2vt_beam_cum_result serves both)
    q.hist = hist ? reinterpret_cast<int*>(take(sizeof(int) * 2 * slots * (size_t)D)) : nullptr;
    if (bytes) *bytes = align_up(off, 256);
    return q;
}

static bool beamc_dims_ok(int B, int bw, int D) {
    return B > 0 && bw >= 1 && bw <= BC_MAXBW && D >= 1 && (int64_t)B * (1 + (int64_t)D * bw) < (1ll << 28);
}

// fp32(len ** alpha) for len = 0..D, evaluated as beam_queue.hip evaluates len ** 0.7 (libm double pow, then fp32), in pinned host
// memory that lives for the life of the process: the copy to the device is asynchronous (no host synchronisation at the start of a
// search), so a table is never freed or rewritten - one per distinct alpha, regrown (the shorter one stays) for a larger D.
const float* length_pow_table(double alpha, int D) {       // (kernels.h: the scoring finisher divides by the same table)
    static std::mutex mu;
    static std::map<double, std::pair<float*, int>> tabs;
    std::lock_guard<std::mutex> lock(mu);
    auto& e = tabs[alpha];
    if (e.second < D + 1) {
        float* grown = nullptr;
        const int len = (D + 1 + 1023) / 1024 * 1024;
        if (hipHostMalloc(reinterpret_cast<void**>(&grown), (size_t)len * sizeof(float), hipHostMallocDefault) != hipSuccess) return nullptr;
        for (int l = 0; l < len; ++l) grown[l] = l > 0 ? (float)pow((double)l, alpha) : 1.0f;
        e = {grown, len};
    }
    return e.first;
}

}  // namespace s2vt

using namespace s2vt;

extern "C" {

static size_t beamc_bytes(int32_t B, int32_t beam_width, int32_t max_depth, bool hist) {
    if (!beamc_dims_ok(B, beam_width, max_depth)) return 0;
    size_t bytes = 0;
    carve_beamc(B, beam_width, max_depth, nullptr, &bytes, hist);
    return bytes;
}
size_t s2vt_beam_cum_bytes(int32_t B, int32_t beam_width, int32_t max_depth) { return beamc_bytes(B, beam_width, max_depth, false); }
size_t s2vt_beam_cum_hist_bytes(int32_t B, int32_t beam_width, int32_t max_depth) { return beamc_bytes(B, beam_width, max_depth, true); }

// both step entries (fn names the one that was called); hist: the constrained form, whose state carries the live slots' words
static int beamc_step(const char* fn, bool hist, int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix,
                      double length_alpha, int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp,
                      int32_t* row_b, int32_t* row_state, int32_t* row_tok, const int32_t** hist_out, int64_t* hist_ld_out, void* stream) {
    S2VT_REQUIRE(beamc_dims_ok(B, beam_width, max_depth) && depth >= 0 && depth <= max_depth && state && row_b && row_state && row_tok,
                 "%s: null/invalid argument (1 <= beam_width <= %d, 0 <= depth <= max_depth)", fn, BC_MAXBW);
    S2VT_REQUIRE(isfinite(length_alpha) && length_alpha >= 0.0, "%s: length_alpha must be finite and >= 0", fn);
    S2VT_REQUIRE(depth == 1 || (top_ix && top_lp), "%s: the step's top-20 arrays are needed from depth 2 on", fn);
    S2VT_REQUIRE(!hist || (hist_out && hist_ld_out), "%s: null hist_out / hist_ld_out", fn);
    size_t need = 0;
    BeamC q = carve_beamc(B, beam_width, max_depth, state, &need, hist);
    S2VT_REQUIRE(state_bytes >= need, "%s: state %zu < %zu bytes", fn, state_bytes, need);
    q.sos = sos_ix; q.eos = eos_ix; q.depth = depth;
    q.top_ix = top_ix; q.top_lp = top_lp;
    q.row_b = row_b; q.row_state = row_state; q.row_tok = row_tok;
    hipStream_t st = (hipStream_t)stream;
    if (depth == 1) {
        const float* tab = length_pow_table(length_alpha, max_depth);
        S2VT_REQUIRE(tab, "%s: no pinned memory for the length table", fn);
        S2VT_HIP(hipMemcpyAsync(q.powa, tab, (size_t)(max_depth + 1) * sizeof(float), hipMemcpyHostToDevice, st));
        S2VT_HIP(hipMemsetAsync(q.done_count, 0, sizeof(int), st));
    }
    if (hist) hipLaunchKernelGGL(beam_cum_kernel<true>, dim3(B), dim3(64), 0, st, q);
    else hipLaunchKernelGGL(beam_cum_kernel<false>, dim3(B), dim3(64), 0, st, q);
    S2VT_LAUNCH_CHECK("beam_cum_kernel");
    if (hist) {
        // the slots that are live after this call hold depth - 1 words each (depth 1: none), in buffer (depth - 1) & 1
        const int t = depth == 0 ? max_depth : depth - 1;
        *hist_out = q.hist + (size_t)(t & 1) * B * beam_width * max_depth;
        *hist_ld_out = max_depth;
    }
    return 0;
}

int s2vt_beam_cum_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, double length_alpha, int32_t depth,
                       void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b, int32_t* row_state,
                       int32_t* row_tok, void* stream) {
    return beamc_step("s2vt_beam_cum_step", false, B, beam_width, max_depth, sos_ix, eos_ix, length_alpha, depth, state, state_bytes, top_ix,
                      top_lp, row_b, row_state, row_tok, nullptr, nullptr, stream);
}
int s2vt_beam_cum_hist_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, double length_alpha,
                            int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b,
                            int32_t* row_state, int32_t* row_tok, const int32_t** hist_out, int64_t* hist_ld_out, void* stream) {
    return beamc_step("s2vt_beam_cum_hist_step", true, B, beam_width, max_depth, sos_ix, eos_ix, length_alpha, depth, state, state_bytes,
                      top_ix, top_lp, row_b, row_state, row_tok, hist_out, hist_ld_out, stream);
}

int s2vt_beam_cum_result(int32_t B, int32_t beam_width, int32_t max_depth, int32_t eos_ix, int32_t n_best, void* state, size_t state_bytes,
                         int32_t* out_tokens, int32_t* out_len, float* out_score, void* stream) {
    S2VT_REQUIRE(beamc_dims_ok(B, beam_width, max_depth) && n_best >= 1 && n_best <= beam_width && state && out_tokens && out_len && out_score,
                 "s2vt_beam_cum_result: null/invalid argument (1 <= n_best <= beam_width <= %d)", BC_MAXBW);
    size_t need = 0;
    BeamC q = carve_beamc(B, beam_width, max_depth, state, &need);
    S2VT_REQUIRE(state_bytes >= need, "s2vt_beam_cum_result: state %zu < %zu bytes", state_bytes, need);
    q.sos = 0; q.eos = eos_ix; q.depth = 0;
    q.top_ix = nullptr; q.top_lp = nullptr; q.row_b = q.row_state = q.row_tok = nullptr;
    hipLaunchKernelGGL(beam_cum_result_kernel, dim3(cdiv(B * n_best, 64)), dim3(64), 0, (hipStream_t)stream, q, n_best, out_tokens, out_len,
                       out_score);
    S2VT_LAUNCH_CHECK("beam_cum_result_kernel");
    return 0;
}

}  // extern "C"
