// The beam policy ON THE DEVICE (not in the reference): group (diverse) beam search, Vijayakumar et al., 2016 (S2VT.beam_diverse), whose
// one-group case is the cumulative-score search (S2VT.forward(mode='beam'), S2VT.beam_constrained, S2VTModel.Ensemble.beam).  One
// kernel, one state, one back-trace for all of them, for every sample of a batch at once, on the row protocol of beam_queue.hip (fixed
// rows r = b * beam_width + slot of s2vt_beam_step, nothing compacted, nothing crosses PCIe per depth).
//
// Definition (include/s2vt_hip.h "diverse beam"), per sample: W = beam_width slots, G groups of Wg = W / G slots,
// lambda >= 0, D = max_depth.  Group g owns slots g*Wg .. (g+1)*Wg-1, a live list that starts as one empty hypothesis (S = 0, <sos>,
// the encoder state) and a pool of at most Wg entries.  For t = 1..D: cnt[v] = 0 for every word; the groups run in order; a group
// whose live list is empty is closed, skipped, and adds nothing to cnt.  Candidate (j, v) of live slot j has the score
// s = S_j + lp_j[v] and the selection key a = s - lambda * cnt[v] (cnt as the EARLIER groups of this depth left it).  The
// min(Wg, count) best by (a descending, j ascending, v ascending) are walked in that order: every one does cnt[v] += 1 (<eos>
// included); v == <eos> enters the group's pool with s / t**alpha - the unpenalised sum: the penalty steers the selection and is
// never accumulated - anything else is the group's next live slot with S = s.  At t == D every live hypothesis enters its group's
// pool with S / D**alpha, no <eos> appended.  A pool is ordered by (score descending, insertion ascending); the answer is every
// group's first n_best.
// fp32 form: s = S_j + fminf(lp, 0) with -0 folded to +0; a = s where cnt == 0, else s - (fp32(lambda) * fp32(cnt)), product and
// difference each rounded to fp32 (div_key below, compiled with contraction off: never one FMA); pool scores divide by length_pow_table.
//
// One WAVE per sample; the G groups are walked sequentially inside the launch.  All W * 20 candidates are loaded once (c = slot * 20
// + f over the lanes, score and word in registers).  A group computes its keys - order-preserving bits of a high, ~c low with
// c = j_local * 20 + f, which IS (j ascending, v ascending) since top_ix rows are in ascending token order - and takes Wg rounds of the
// keyed wave-wide max (beam_wave.h); keys are distinct, so every round has exactly one winner, no replay path.  The winner's s and
// word come from its owner lane by one shuffle each.  The words selected so far at this depth (at most 7 matter) are wave-uniform
// registers, so every lane counts cnt for its own candidates: no sort, no floating-point atomic, the same inputs give the same bits.
// The walk (pool inserts, next live slots) is lane 0's, on LDS copies of the pools that lanes 0..W-1 load and write back.  A slot
// that is not live has live_nid < 0; a group's live slots are compact from its first slot, in selection order.
//
// Fan-out 20 is exact for W <= 8: in group g at most g * Wg <= W - Wg distinct words are penalised; a candidate outside its
// parent's unpenalised top W has W candidates of the same parent in front of it, at least Wg of them unpenalised - their keys are >=
// its key and they win every tie - so it is never selected, and W <= 8 < 20.  With constraints the argument runs on the edited row.
//
// Early stop.  A group is SETTLED when it is closed, or when its pool holds Wg entries and pool[Wg-1].score >= max_j(live S_j) /
// D**alpha.  The maximum over the live S_j is needed because the live slots are ordered by a, not by s: live[0] need not hold the
// largest S.  A settled group's pool can never change again: the kernel clamps every log-prob to <= 0 (fminf(lp, 0)), so S never
// rises along a hypothesis; any hypothesis the group finishes later has S' <= max_j(live S_j) <= 0 and a length t' <= D; the divisor
// table is non-decreasing in the length for alpha >= 0 (pow and the rounding to fp32 are monotone), so S' / t'**alpha <= S' / D**alpha
// <= max_j(live S_j) / D**alpha <= pool[Wg-1].score, and the rounded fp32 quotients keep that order (division is monotone in both
// operands here); an equal score loses to the earlier insertion, so it never enters the best Wg.  (The penalty never enters S or a
// pool score, so it plays no part.)  "Settled" is monotone: the pool's Wg-th score only rises and the live maximum only falls.  A
// SAMPLE is frozen only when every one of its groups is settled: until then a settled group keeps stepping and keeps adding to cnt,
// because the later groups' selections depend on its choices.  Once all are settled no pool of the sample changes any more, so
// freezing it changes no output.
//
// HIST (the constrained forms; include/s2vt_hip.h "constrained beam").  The depth step's fan-out head edits a slot's logits row by the
// rules of the constrained draw with the slot's own words as history, then takes log_softmax and the top 20 of the EDITED row (ce.hip).
// The policy is unchanged; it only has to keep every live slot's words where that head can read them: hist[2][B][W][D] int32 behind
// the plain state, ping-ponged by depth parity - the slots that are live after depth t (t words each) are in buffer t & 1.  When
// candidate (j, v) becomes live slot s, the wave copies parent j's t-1 words from buffer (t-1) & 1 into slot s of buffer t & 1 (lanes
// over the words: W * (t-1) independent loads for a wave whose lanes 1..63 are otherwise idle behind the selection) and appends v.
// Both buffers are zeroed at depth 1, and nothing else is ever written to them - nothing at t == D, nothing for a sample that has
// just stopped: the row of an unused slot or of a frozen sample stays readable - defined words in [0, V) - and its fan-out is never
// consumed.  Chosen over walking node_prev inside the head: that is t DEPENDENT global loads in front of every row's load, on the
// critical path of every depth.  The early stop holds as it stands: its proof needs lp <= 0 only, which the log_softmax of any edited
// row gives (and the clamp enforces).  A banned word is -inf in the edited row and is never among the 20 while V >= 20 + D + n_banned
// + 1 (checked by the callers).
//
// One group (the s2vt_beam_cum_* entries: G = 1, lambda = 0).  Keys are computed once per group, before its first round, from the
// words the EARLIER groups selected: at G = 1 there are none, cnt is 0 for every candidate, the key is the plain score s and div_key is
// never evaluated - lambda is inert.  c = j * 20 + f over the whole beam.  The selection order is then s descending, the live slots
// keep it, so live[0].S is max_j(live S_j) bit for bit (-0 is folded away before the keys) and the early stop reads
// pool[W-1].score >= live[0].S / D**alpha; "every group settled" is "the group settled".  The definition reduces to: the W best
// candidates of all live slots by (S descending, j ascending, v ascending), <eos> into the one pool, n_best out.
#include <math.h>

#include <map>
#include <mutex>

#include "beam_wave.h"
#include "common.h"
#include "kernels.h"

namespace s2vt {

struct BeamP {
    int B, bw, G, Wg, D, NN, sos, eos, depth;  // depth: 1 = initialise; 2..D = consume step depth-1; 0 = consume step D
    float lam;                                               // fp32(diversity_lambda)
    int* done_count; int* done; int* n_nodes;
    int* node_tok; int* node_prev;                           // [B][NN]: every selected candidate, for the back-trace
    float* live_S; int* live_nid;                            // [B][bw]; live_nid < 0: the slot is not live
    int* pool_n; float* pool_score; int* pool_nid; int* pool_len;      // [B][G], [B][bw] x 3 (group g's entries from g * Wg)
    float* powa;                                             // fp32(len ** alpha): double pow, then fp32
    const int* top_ix; const float* top_lp;                  // [B*bw][20] of the depth just stepped
    int* row_b; int* row_state; int* row_tok;                // [B*bw] for the next s2vt_beam_step
    int* hist;                                               // [2][B][bw][D] words of the live slots (the constrained forms only)
};

// The selection key a = s - (lam * cnt), the product and the difference each rounded to fp32.  __fmul_rn / __fsub_rn are plain * and -
// in this toolchain's headers and hipcc contracts them to one v_fma_f32 by default, which rounds once: contraction is switched off
// for this body (it holds for the instructions after inlining; tests/test_gpu_beam_div.py has an input that tells the two apart).
__device__ __forceinline__ float div_key(float s, float lam, int cnt) {
#pragma clang fp contract(off)
    const float pen = lam * (float)cnt;
    return s - pen;
}

// HIST: the constrained forms - the same policy, and the live slots' words kept in q.hist (the comment at the top).
template <bool HIST>
__global__ __launch_bounds__(64) void beam_policy_kernel(BeamP q) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int bw = q.bw, G = q.G, Wg = q.Wg;
    float* lS = q.live_S + b * bw;
    int* lnid = q.live_nid + b * bw;
    int* ntok = q.node_tok + (int64_t)b * q.NN;
    int* nprev = q.node_prev + (int64_t)b * q.NN;
    if (q.depth == 1) {            // every group: one empty hypothesis on the encoder state (row b of the first state table)
        if constexpr (HIST) {      // both buffers of the sample: defined words for every slot, live or not
            const int per = bw * q.D;
            for (int i = lane; i < per; i += 64) {
                q.hist[(int64_t)b * per + i] = 0;
                q.hist[((int64_t)q.B + b) * per + i] = 0;
            }
        }
        if (lane < bw) {
            const bool first = lane % Wg == 0;
            lS[lane] = 0.0f; lnid[lane] = first ? 0 : -1;
            q.pool_score[b * bw + lane] = 0.0f; q.pool_nid[b * bw + lane] = 0; q.pool_len[b * bw + lane] = 0;
            q.row_b[b * bw + lane] = b;
            q.row_state[b * bw + lane] = first ? b : 0;
            q.row_tok[b * bw + lane] = first ? q.sos : 0;
        }
        if (lane < G) q.pool_n[b * G + lane] = 0;
        if (lane == 0) {
            q.done[b] = 0; q.n_nodes[b] = 1;
            ntok[0] = q.sos; nprev[0] = -1;
        }
        return;
    }
    if (q.done[b]) return;         // frozen: its rows were cleared when it stopped
    const int t = q.depth == 0 ? q.D : q.depth - 1;
    __shared__ float sh_pS[BC_MAXBW], sh_nS[BC_MAXBW], sh_selS[BC_MAXBW];
    __shared__ int sh_pnid[BC_MAXBW], sh_plen[BC_MAXBW], sh_pn[BC_MAXBW], sh_oldnid[BC_MAXBW];
    __shared__ int sh_nnid[BC_MAXBW], sh_nrow[BC_MAXBW], sh_ntk[BC_MAXBW], sh_npar[BC_MAXBW];
    __shared__ int sh_selv[BC_MAXBW], sh_selj[BC_MAXBW];
    if (lane < bw) {               // the pools and the live slots' node ids; the next live slots start empty
        sh_pS[lane] = q.pool_score[b * bw + lane]; sh_pnid[lane] = q.pool_nid[b * bw + lane]; sh_plen[lane] = q.pool_len[b * bw + lane];
        sh_oldnid[lane] = lnid[lane];
        sh_nS[lane] = 0.0f; sh_nnid[lane] = -1; sh_nrow[lane] = 0; sh_ntk[lane] = 0; sh_npar[lane] = 0;
    }
    if (lane < G) sh_pn[lane] = q.pool_n[b * G + lane];
    // ---- candidates of all groups: cg = slot * 20 + f, score S_slot + min(lp, 0) and the word; cgrp < 0: none (slot not live)
    float cs[BC_CPL];
    int cv[BC_CPL], cgrp[BC_CPL], cloc[BC_CPL];
#pragma unroll
    for (int k = 0; k < BC_CPL; ++k) {
        const int cg = lane + 64 * k;
        cs[k] = 0.0f; cv[k] = -1; cgrp[k] = -1; cloc[k] = 0;
        if (cg < bw * BC_FAN) {
            const int slot = cg / BC_FAN, g = slot / Wg;
            if (lnid[slot] >= 0) {
                float s = lS[slot] + fminf(q.top_lp[(int64_t)(b * bw + slot) * BC_FAN + (cg - slot * BC_FAN)], 0.0f);
                cs[k] = s == 0.0f ? 0.0f : s;                   // (-0 and +0 are one score)
                cv[k] = q.top_ix[(int64_t)(b * bw + slot) * BC_FAN + (cg - slot * BC_FAN)];
                cgrp[k] = g;
                cloc[k] = cg - g * Wg * BC_FAN;                 // c = j_local * 20 + f
            }
        }
    }
    // ---- selection, slot by slot (group i / Wg, round i % Wg): every lane ends with the same lists
    unsigned long long key[BC_CPL];
    float selS[BC_MAXBW];
    int selv[BC_MAXBW], selj[BC_MAXBW];          // selv < 0: nothing selected into this place (its group is closed)
#pragma unroll
    for (int i = 0; i < BC_MAXBW; ++i) {
        selS[i] = 0.0f; selv[i] = -1; selj[i] = 0;
        if (i < bw) {
            const int g = i / Wg, r = i - g * Wg;
            if (r == 0) {          // the group's keys, with cnt as the earlier groups left it
#pragma unroll
                for (int k = 0; k < BC_CPL; ++k) {
                    key[k] = 0;
                    if (cgrp[k] == g) {
                        int cnt = 0;
#pragma unroll
                        for (int p = 0; p < i; ++p) cnt += selv[p] == cv[k] ? 1 : 0;
                        const float a = cnt == 0 ? cs[k] : div_key(cs[k], q.lam, cnt);
                        key[k] = ((unsigned long long)bc_ordered(a) << 32) | (unsigned int)~(unsigned int)cloc[k];
                    }
                }
            }
            unsigned long long mx = 0;
#pragma unroll
            for (int k = 0; k < BC_CPL; ++k) mx = key[k] > mx ? key[k] : mx;
            mx = bc_wave_max(mx);
            if (mx != 0) {         // (0: the group is closed - no candidate; an open group has 20 >= Wg of them)
#pragma unroll
                for (int k = 0; k < BC_CPL; ++k) key[k] = key[k] == mx ? 0 : key[k];
                const int c = (int)~(unsigned int)mx;
                const int cg = g * Wg * BC_FAN + c, owner = cg & 63, kk = cg >> 6;
                const float sv = kk == 0 ? cs[0] : (kk == 1 ? cs[1] : cs[2]);
                const int vv = kk == 0 ? cv[0] : (kk == 1 ? cv[1] : cv[2]);
                selS[i] = __shfl(sv, owner);
                selv[i] = __shfl(vv, owner);
                selj[i] = c / BC_FAN;
            }
        }
    }
    static_assert(BC_CPL == 3, "the owner-lane select above reads three candidates per lane");
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < BC_MAXBW; ++i) { sh_selS[i] = selS[i]; sh_selv[i] = selv[i]; sh_selj[i] = selj[i]; }
    }
    __syncthreads();
    if (lane == 0) {
        // ---- walk every group's selected candidates: <eos> -> its pool, anything else -> its next live slot
        const float div_t = q.powa[t], div_D = q.powa[q.D];
        int nn = q.n_nodes[b];
        bool all_settled = true;
        for (int g = 0; g < G; ++g) {
            const int base = g * Wg;
            int pn = sh_pn[g], nnl = 0;
            auto pool_insert = [&](float score, int nid, int len) {
                int p = 0;
                while (p < pn && !(score > sh_pS[base + p])) ++p;       // behind every entry that is not worse: insertion order breaks ties
                if (p >= Wg) return;
                const int last = pn < Wg ? pn : Wg - 1;
                for (int i = last; i > p; --i) {
                    sh_pS[base + i] = sh_pS[base + i - 1]; sh_pnid[base + i] = sh_pnid[base + i - 1]; sh_plen[base + i] = sh_plen[base + i - 1];
                }
                sh_pS[base + p] = score; sh_pnid[base + p] = nid; sh_plen[base + p] = len;
                pn = pn < Wg ? pn + 1 : Wg;
            };
            for (int r = 0; r < Wg; ++r) {
                const int v = sh_selv[base + r];
                if (v < 0) break;                               // (a closed group)
                const float s = sh_selS[base + r];
                const int j = sh_selj[base + r];
                const int id = nn < q.NN ? nn : q.NN - 1;       // (NN = 1 + D * W: never exceeded)
                ntok[id] = v; nprev[id] = sh_oldnid[base + j];
                ++nn;
                if (v == q.eos) {
                    pool_insert(s / div_t, id, t);
                } else {
                    sh_nS[base + nnl] = s; sh_nnid[base + nnl] = id; sh_nrow[base + nnl] = b * bw + base + j; sh_ntk[base + nnl] = v;
                    sh_npar[base + nnl] = base + j;
                    ++nnl;
                }
            }
            if (t == q.D) {            // unfinished at the depth limit: into the pool as they are, no <eos> appended
                for (int i = 0; i < nnl; ++i) {
                    pool_insert(sh_nS[base + i] / div_D, sh_nnid[base + i], t);
                    sh_nnid[base + i] = -1; sh_nrow[base + i] = 0; sh_ntk[base + i] = 0;
                }
                nnl = 0;
            }
            sh_pn[g] = pn;
            bool settled = nnl == 0;                            // closed
            if (!settled && pn == Wg) {                         // (the early stop: see the proof at the top)
                float mxS = sh_nS[base];
                for (int i = 1; i < nnl; ++i) mxS = fmaxf(mxS, sh_nS[base + i]);
                settled = sh_pS[base + Wg - 1] >= mxS / div_D;
            }
            all_settled = all_settled && settled;
        }
        q.n_nodes[b] = nn < q.NN ? nn : q.NN;
        if (all_settled) {
            for (int i = 0; i < bw; ++i) { sh_nnid[i] = -1; sh_nrow[i] = 0; sh_ntk[i] = 0; }
            q.done[b] = 1;
            atomicAdd(q.done_count, 1);
        }
    }
    __syncthreads();
    if (lane < bw) {
        q.pool_score[b * bw + lane] = sh_pS[lane]; q.pool_nid[b * bw + lane] = sh_pnid[lane]; q.pool_len[b * bw + lane] = sh_plen[lane];
        lS[lane] = sh_nS[lane]; lnid[lane] = sh_nnid[lane];
        q.row_state[b * bw + lane] = sh_nrow[lane];
        q.row_tok[b * bw + lane] = sh_ntk[lane];
    }
    if (lane < G) q.pool_n[b * G + lane] = sh_pn[lane];
    if constexpr (HIST) {
        // ---- the new live slots' words: parent's t-1 words from buffer (t-1) & 1, then the slot's own, into buffer t & 1
        const int per = bw * q.D;
        const int* src = q.hist + ((int64_t)((t - 1) & 1) * q.B + b) * per;
        int* dst = q.hist + ((int64_t)(t & 1) * q.B + b) * per;
        for (int s = 0; s < bw; ++s) {
            if (sh_nnid[s] < 0) continue;                       // (every slot at t == D and in a sample that has just stopped)
            const int* from = src + sh_npar[s] * q.D;
            for (int i = lane; i < t - 1; i += 64) dst[s * q.D + i] = from[i];
            if (lane == 0) dst[s * q.D + t - 1] = sh_ntk[s];
        }
    }
}

// back-trace of every group's first n_best pool entries: one thread per (sample, group, rank)
__global__ void beam_policy_result_kernel(BeamP q, int n_best, int32_t* out, int32_t* out_len, float* out_score) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.B * q.G * n_best) return;
    const int bg = i / n_best, k = i - bg * n_best;
    const int b = bg / q.G, g = bg - b * q.G;
    const int e = b * q.bw + g * q.Wg + k;
    const int* ntok = q.node_tok + (int64_t)b * q.NN;
    const int* nprev = q.node_prev + (int64_t)b * q.NN;
    int32_t* o = out + (int64_t)i * q.D;
    const bool have = k < q.pool_n[bg];                    // (always, once the sample is done)
    int len = have ? q.pool_len[e] : 0;
    len = len < q.D ? len : q.D;
    for (int p = len; p < q.D; ++p) o[p] = q.eos;
    int node = have ? q.pool_nid[e] : -1;
    for (int p = len - 1; p >= 0 && node > 0 && node < q.NN; --p, node = nprev[node]) o[p] = ntok[node];
    out_len[i] = len;
    out_score[i] = have ? q.pool_score[e] : -INFINITY;
}

static BeamP carve_beamp(int B, int bw, int G, int D, void* base, size_t* bytes, bool hist) {
    char* p = reinterpret_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) { off = align_up(off, 256); char* r = base ? p + off : nullptr; off += n; return r; };
    const size_t slots = (size_t)B * bw;
    BeamP q;
    q.B = B; q.bw = bw; q.G = G; q.Wg = bw / G; q.D = D; q.NN = 1 + D * bw;
    q.done_count = reinterpret_cast<int*>(take(sizeof(int)));          // (first: the frozen-sample counter is at byte 0)
    q.done = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.n_nodes = reinterpret_cast<int*>(take(sizeof(int) * B));
    q.node_tok = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * q.NN));
    q.node_prev = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * q.NN));
    q.live_S = reinterpret_cast<float*>(take(sizeof(float) * slots));
    q.live_nid = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.pool_n = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * G));
    q.pool_score = reinterpret_cast<float*>(take(sizeof(float) * slots));
    q.pool_nid = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.pool_len = reinterpret_cast<int*>(take(sizeof(int) * slots));
    q.powa = reinterpret_cast<float*>(take(sizeof(float) * (size_t)(D + 1)));
    // (last: a state with words is the plain one with the words behind it - the result entries serve both)
    q.hist = hist ? reinterpret_cast<int*>(take(sizeof(int) * 2 * slots * (size_t)D)) : nullptr;
    if (bytes) *bytes = align_up(off, 256);
    return q;
}

static bool beamp_dims_ok(int B, int bw, int G, int D) {
    return B > 0 && bw >= 1 && bw <= BC_MAXBW && G >= 1 && G <= bw && bw % G == 0 && D >= 1 && (int64_t)B * (1 + (int64_t)D * bw) < (1ll << 28);
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

// Every exported entry below is its arguments over these three (fn names the entry that was called); the s2vt_beam_cum_* entries are
// G = 1, lambda = 0.
static size_t bytes(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, bool hist) {
    if (!beamp_dims_ok(B, beam_width, num_groups, max_depth)) return 0;
    size_t n = 0;
    carve_beamp(B, beam_width, num_groups, max_depth, nullptr, &n, hist);
    return n;
}

// hist_out / hist_ld_out both non-null: the form that keeps the live slots' words (the constrained searches); both null: the plain form
static int step(const char* fn, int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t sos_ix, int32_t eos_ix,
                double length_alpha, double diversity_lambda, int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix,
                const float* top_lp, int32_t* row_b, int32_t* row_state, int32_t* row_tok, const int32_t** hist_out, int64_t* hist_ld_out,
                void* stream) {
    S2VT_REQUIRE(beamp_dims_ok(B, beam_width, num_groups, max_depth) && depth >= 0 && depth <= max_depth && state && row_b && row_state &&
                 row_tok, "%s: null/invalid argument (B >= 1, 1 <= num_groups <= beam_width <= %d, beam_width a multiple of num_groups, "
                 "0 <= depth <= max_depth)", fn, BC_MAXBW);
    S2VT_REQUIRE(isfinite(length_alpha) && length_alpha >= 0.0, "%s: length_alpha must be finite and >= 0", fn);
    S2VT_REQUIRE(isfinite(diversity_lambda) && diversity_lambda >= 0.0 && isfinite((float)diversity_lambda),
                 "%s: diversity_lambda must be finite (in fp32) and >= 0", fn);
    S2VT_REQUIRE(depth == 1 || (top_ix && top_lp), "%s: the step's top-20 arrays are needed from depth 2 on", fn);
    S2VT_REQUIRE((hist_out == nullptr) == (hist_ld_out == nullptr), "%s: hist_out and hist_ld_out go together", fn);
    const bool hist = hist_out != nullptr;
    size_t need = 0;
    BeamP q = carve_beamp(B, beam_width, num_groups, max_depth, state, &need, hist);
    S2VT_REQUIRE(state_bytes >= need, "%s: state %zu < %zu bytes", fn, state_bytes, need);
    q.sos = sos_ix; q.eos = eos_ix; q.depth = depth; q.lam = (float)diversity_lambda;
    q.top_ix = top_ix; q.top_lp = top_lp;
    q.row_b = row_b; q.row_state = row_state; q.row_tok = row_tok;
    hipStream_t st = (hipStream_t)stream;
    if (depth == 1) {
        const float* tab = length_pow_table(length_alpha, max_depth);
        S2VT_REQUIRE(tab, "%s: no pinned memory for the length table", fn);
        S2VT_HIP(hipMemcpyAsync(q.powa, tab, (size_t)(max_depth + 1) * sizeof(float), hipMemcpyHostToDevice, st));
        S2VT_HIP(hipMemsetAsync(q.done_count, 0, sizeof(int), st));
    }
    if (hist) hipLaunchKernelGGL(beam_policy_kernel<true>, dim3(B), dim3(64), 0, st, q);
    else hipLaunchKernelGGL(beam_policy_kernel<false>, dim3(B), dim3(64), 0, st, q);
    S2VT_LAUNCH_CHECK("beam_policy_kernel");
    if (hist) {
        // the slots that are live after this call hold depth - 1 words each (depth 1: none), in buffer (depth - 1) & 1
        const int t = depth == 0 ? max_depth : depth - 1;
        *hist_out = q.hist + (size_t)(t & 1) * B * beam_width * max_depth;
        *hist_ld_out = max_depth;
    }
    return 0;
}

static int result(const char* fn, int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t eos_ix, int32_t n_best,
                  void* state, size_t state_bytes, int32_t* out_tokens, int32_t* out_len, float* out_score, void* stream) {
    S2VT_REQUIRE(beamp_dims_ok(B, beam_width, num_groups, max_depth) && state && out_tokens && out_len && out_score,
                 "%s: null/invalid argument (B >= 1, 1 <= num_groups <= beam_width <= %d, beam_width a multiple of num_groups)", fn, BC_MAXBW);
    S2VT_REQUIRE(n_best >= 1 && n_best <= beam_width / num_groups, "%s: 1 <= n_best <= beam_width / num_groups = %d", fn,
                 beam_width / num_groups);
    size_t need = 0;                                       // (the plain state: the words, where there are any, lie behind it)
    BeamP q = carve_beamp(B, beam_width, num_groups, max_depth, state, &need, false);
    S2VT_REQUIRE(state_bytes >= need, "%s: state %zu < %zu bytes", fn, state_bytes, need);
    q.sos = 0; q.eos = eos_ix; q.depth = 0; q.lam = 0.0f;
    q.top_ix = nullptr; q.top_lp = nullptr; q.row_b = q.row_state = q.row_tok = nullptr;
    hipLaunchKernelGGL(beam_policy_result_kernel, dim3(cdiv(B * num_groups * n_best, 64)), dim3(64), 0, (hipStream_t)stream, q, n_best,
                       out_tokens, out_len, out_score);
    S2VT_LAUNCH_CHECK("beam_policy_result_kernel");
    return 0;
}

size_t s2vt_beam_cum_bytes(int32_t B, int32_t beam_width, int32_t max_depth) { return bytes(B, beam_width, 1, max_depth, false); }
size_t s2vt_beam_cum_hist_bytes(int32_t B, int32_t beam_width, int32_t max_depth) { return bytes(B, beam_width, 1, max_depth, true); }
size_t s2vt_beam_div_bytes(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t hist) {
    return bytes(B, beam_width, num_groups, max_depth, hist != 0);
}

int s2vt_beam_cum_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, double length_alpha, int32_t depth,
                       void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b, int32_t* row_state,
                       int32_t* row_tok, void* stream) {
    return step("s2vt_beam_cum_step", B, beam_width, 1, max_depth, sos_ix, eos_ix, length_alpha, 0.0, depth, state, state_bytes, top_ix,
                top_lp, row_b, row_state, row_tok, nullptr, nullptr, stream);
}
int s2vt_beam_cum_hist_step(int32_t B, int32_t beam_width, int32_t max_depth, int32_t sos_ix, int32_t eos_ix, double length_alpha,
                            int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix, const float* top_lp, int32_t* row_b,
                            int32_t* row_state, int32_t* row_tok, const int32_t** hist_out, int64_t* hist_ld_out, void* stream) {
    S2VT_REQUIRE(hist_out && hist_ld_out, "s2vt_beam_cum_hist_step: null hist_out / hist_ld_out");
    return step("s2vt_beam_cum_hist_step", B, beam_width, 1, max_depth, sos_ix, eos_ix, length_alpha, 0.0, depth, state, state_bytes, top_ix,
                top_lp, row_b, row_state, row_tok, hist_out, hist_ld_out, stream);
}
int s2vt_beam_div_step(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t sos_ix, int32_t eos_ix,
                       double length_alpha, double diversity_lambda, int32_t depth, void* state, size_t state_bytes, const int32_t* top_ix,
                       const float* top_lp, int32_t* row_b, int32_t* row_state, int32_t* row_tok, const int32_t** hist_out,
                       int64_t* hist_ld_out, void* stream) {
    return step("s2vt_beam_div_step", B, beam_width, num_groups, max_depth, sos_ix, eos_ix, length_alpha, diversity_lambda, depth, state,
                state_bytes, top_ix, top_lp, row_b, row_state, row_tok, hist_out, hist_ld_out, stream);
}

int s2vt_beam_cum_result(int32_t B, int32_t beam_width, int32_t max_depth, int32_t eos_ix, int32_t n_best, void* state, size_t state_bytes,
                         int32_t* out_tokens, int32_t* out_len, float* out_score, void* stream) {
    return result("s2vt_beam_cum_result", B, beam_width, 1, max_depth, eos_ix, n_best, state, state_bytes, out_tokens, out_len, out_score,
                  stream);
}
int s2vt_beam_div_result(int32_t B, int32_t beam_width, int32_t num_groups, int32_t max_depth, int32_t eos_ix, int32_t n_best, void* state,
                         size_t state_bytes, int32_t* out_tokens, int32_t* out_len, float* out_score, void* stream) {
    return result("s2vt_beam_div_result", B, beam_width, num_groups, max_depth, eos_ix, n_best, state, state_bytes, out_tokens, out_len,
                  out_score, stream);
}

}  // extern "C"
