// Self-critical rewards on the device (train.py --sc-reward device): CIDEr of a batch of id rows against a reference table that
// self_critical.DeviceCiderRewarder builds once (s2vt_cider_table of include/s2vt_hip.h), and the <sos>-prefixed captions and
// advantage weights the train step takes; and consensus (MBR) selection among the K candidates of a clip (consensus.select,
// eval.py --consensus), the same score with the clip's other candidates as the references; and sentence BLEU-4 beside both
// (s2vt_mixed_rewards, s2vt_mixed_consensus: w_cider * CIDEr + w_bleu * BLEU-4 from one candidate phase).  fp64 throughout; every
// factor that needs log / exp comes precomputed from the host, so the kernels only add, multiply, divide, take sqrt and min - in a
// fixed order, without floating-point atomics.
#include "api_internal.h"

// a * b + c stays two roundings, as in the host's arithmetic
#pragma clang fp contract(off)

namespace s2vt {

constexpr int kCiderThreads = 256;
constexpr int kCiderMaxT = S2VT_CIDER_MAX_T;
constexpr int kCiderMaxN = 4 * kCiderMaxT;          // 1..4-grams of kCiderMaxT words: fewer than 4 per word; a power of two
static_assert((kCiderMaxN & (kCiderMaxN - 1)) == 0, "the bitonic sort needs a power of two");
static_assert(kCiderThreads == 4 * 64, "one wavefront per n-gram order");

// order of a key = its number of non-zero 16-bit fields (tokens are never 0), counted from the top
__device__ __forceinline__ int cider_key_order(uint64_t k) {
    return (k & 0xFFFFull) ? 4 : (k & 0xFFFF0000ull) ? 3 : (k & 0xFFFF00000000ull) ? 2 : 1;
}
// index of `key` in the ascending keys[lo, hi), or -1
__device__ __forceinline__ int64_t cider_find(const uint64_t* keys, int64_t lo, int64_t hi, uint64_t key) {
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && keys[lo] == key ? lo : -1;
}
// butterfly sum over the 64 lanes: the same association order in every lane and on every call
__device__ __forceinline__ double cider_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// What the candidate phase leaves in LDS: the sorted 1..4-gram keys of a row, tf * idf at the first entry of every run of equal keys
// (0 elsewhere), the norm per order.  34 KB of the 160 KB a workgroup may use.
struct CiderRowLds {
    int32_t words[kCiderMaxT];
    uint64_t keys[kCiderMaxN];
    double wts[kCiderMaxN];
    double hn[4];
    int m;
};
struct CiderRow { int total, n2; };               // entries of keys / wts in use; the scorer's length (the number of bigrams)

// The candidate phase of one id row, by the whole workgroup (every thread calls it; it holds barriers and ends behind one): strip,
// keys, sort, run heads carrying tf * idf, per-order norms.  cider_rewards_kernel and the consensus kernels share it.
__device__ __forceinline__ CiderRow cider_candidate(const s2vt_cider_table& tb, const int64_t* row, int T, int sos, int eos,
                                                    CiderRowLds& L, int* err) {
    int32_t* words = L.words;
    uint64_t* keys = L.keys;
    double* wts = L.wts;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- the words of the row (strip_caption): one wavefront walks it in chunks of 64 and compacts with ballots
    if (wave == 0) {
        int m = 0;
        bool bad = false;
        for (int base = 0; base < T; base += 64) {
            const int i = base + lane;
            const int64_t t = i < T ? row[i] : 0;
            const unsigned long long eosm = __ballot(i < T && t == (int64_t)eos);
            const bool before = eosm == 0 || lane < __ffsll((long long)eosm) - 1;
            const bool oor = before && (t < 0 || t > 65535);
            bad |= oor;
            const bool keep = i < T && before && !oor && t != 0 && !(i == 0 && t == (int64_t)sos);
            const unsigned long long km = __ballot(keep);
            if (keep) words[m + __popcll(km & ((1ull << lane) - 1ull))] = (int32_t)t;
            m += __popcll(km);
            if (eosm) break;
        }
        if (__ballot(bad) && lane == 0) atomicExch(err, 2);
        if (lane == 0) L.m = m;
    }
    __syncthreads();
    const int m = L.m;
    const int n1 = m, n2 = m > 1 ? m - 1 : 0, n3 = m > 2 ? m - 2 : 0, n4 = m > 3 ? m - 3 : 0;
    const int total = n1 + n2 + n3 + n4;
    int N = 1;
    while (N < total) N <<= 1;                    // <= kCiderMaxN since m <= T <= kCiderMaxT
    // ---- every 1..4-gram as a key; the tail of the power of two is filled with the largest value and stays behind the sort
    for (int i = tid; i < N; i += kCiderThreads) {
        uint64_t key = ~0ull;
        if (i < total) {
            int k, p;
            if (i < n1) { k = 1; p = i; }
            else if (i < n1 + n2) { k = 2; p = i - n1; }
            else if (i < n1 + n2 + n3) { k = 3; p = i - n1 - n2; }
            else { k = 4; p = i - n1 - n2 - n3; }
            key = 0;
            for (int j = 0; j < k; ++j) key |= (uint64_t)(uint32_t)words[p + j] << (48 - 16 * j);
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N; i += kCiderThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t a = keys[i], c = keys[x];
                    if ((a > c) == ((i & k) == 0)) {
                        keys[i] = c;
                        keys[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // ---- unique n-grams: the first entry of a run carries tf (the run's length) * idf
    for (int i = tid; i < N; i += kCiderThreads) {
        double w = 0.0;
        if (i < total) {
            const uint64_t key = keys[i];
            if (i == 0 || keys[i - 1] != key) {
                int tf = 1;
                while (i + tf < total && keys[i + tf] == key) ++tf;
                const int64_t at = cider_find(tb.idf_keys, 0, tb.n_idf, key);
                w = (double)tf * (at >= 0 ? tb.idf_vals[at] : tb.log_n);
            }
        }
        wts[i] = w;
    }
    __syncthreads();
    // ---- the candidate's norm per order: wavefront k takes order k + 1
    {
        double s = 0.0;
        for (int i = lane; i < total; i += 64) {
            const double w = wts[i];
            if (w != 0.0 && cider_key_order(keys[i]) == wave + 1) s += w * w;
        }
        s = cider_wave_sum(s);
        if (lane == 0) L.hn[wave] = sqrt(s);
    }
    __syncthreads();
    return CiderRow{total, n2};
}

// The reference phase of one row, by the whole workgroup (every thread calls it; it holds one barrier): the candidate that
// cider_candidate left in L against the references of clip crow.  Thread 0 returns the score, the others 0.  cider_rewards_kernel and
// mixed_rewards_kernel share it, so the two give the same bits.
__device__ __forceinline__ double cider_reference(const s2vt_cider_table& tb, int crow, CiderRow cr, const CiderRowLds& L,
                                                  double (*s_tot)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = cr.total, n2 = cr.n2;
    const uint64_t* keys = L.keys;
    const double* wts = L.wts;
    const double* s_hn = L.hn;
    // ---- against the references of the clip: wavefront w takes references w, w + 4, ..; its lanes share the n-grams
    const int r0 = tb.clip_ref_off[crow], r1 = tb.clip_ref_off[crow + 1];
    double tot0 = 0.0, tot1 = 0.0, tot2 = 0.0, tot3 = 0.0;
    for (int r = r0 + wave; r < r1; r += kCiderThreads / 64) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int i = lane; i < total; i += 64) {
            const double w = wts[i];
            if (w == 0.0) continue;               // not the head of a run, or idf 0: contributes exactly 0
            const uint64_t key = keys[i];
            const int k = cider_key_order(key) - 1;
            const int64_t at = cider_find(tb.ent_keys, tb.ent_off[4 * (int64_t)r + k], tb.ent_off[4 * (int64_t)r + k + 1], key);
            if (at < 0) continue;
            const double wr = tb.ent_w[at];
            const double c = (w < wr ? w : wr) * wr;
            if (k == 0) a0 += c;
            else if (k == 1) a1 += c;
            else if (k == 2) a2 += c;
            else a3 += c;
        }
        a0 = cider_wave_sum(a0);
        a1 = cider_wave_sum(a1);
        a2 = cider_wave_sum(a2);
        a3 = cider_wave_sum(a3);
        int d = n2 - tb.ref_len[r];
        d = d < 0 ? -d : d;
        const double pen = tb.pen[d < tb.n_pen ? d : tb.n_pen - 1];
        const double* rn = tb.ref_norm + 4 * (int64_t)r;
        if (s_hn[0] != 0.0 && rn[0] != 0.0) a0 /= s_hn[0] * rn[0];
        if (s_hn[1] != 0.0 && rn[1] != 0.0) a1 /= s_hn[1] * rn[1];
        if (s_hn[2] != 0.0 && rn[2] != 0.0) a2 /= s_hn[2] * rn[2];
        if (s_hn[3] != 0.0 && rn[3] != 0.0) a3 /= s_hn[3] * rn[3];
        tot0 += a0 * pen;
        tot1 += a1 * pen;
        tot2 += a2 * pen;
        tot3 += a3 * pen;
    }
    if (lane == 0) {
        s_tot[wave][0] = tot0;
        s_tot[wave][1] = tot1;
        s_tot[wave][2] = tot2;
        s_tot[wave][3] = tot3;
    }
    __syncthreads();
    if (tid != 0) return 0.0;
    double t[4];
    for (int k = 0; k < 4; ++k) t[k] = ((s_tot[0][k] + s_tot[1][k]) + s_tot[2][k]) + s_tot[3][k];
    const double mean = (((t[0] + t[1]) + t[2]) + t[3]) / 4.0;
    return mean / (double)(r1 - r0) * 10.0;
}

// One workgroup = one candidate row.
__global__ __launch_bounds__(kCiderThreads) void cider_rewards_kernel(s2vt_cider_table tb, const int32_t* clip_rows, const int64_t* ids,
                                                                      int T, int64_t ld, int sos, int eos, double* out, int* err) {
    __shared__ CiderRowLds L;
    __shared__ double s_tot[kCiderThreads / 64][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int crow = clip_rows[b];
    if (crow < 0 || crow >= tb.n_clips) {         // the whole workgroup leaves together, before the first barrier
        if (tid == 0) {
            atomicExch(err, 2);
            out[b] = 0.0;
        }
        return;
    }
    const CiderRow cr = cider_candidate(tb, ids + (int64_t)b * ld, T, sos, eos, L, err);
    const double score = cider_reference(tb, crow, cr, L, s_tot);
    if (tid == 0) out[b] = score;
}

// ---------------------------------------------------------------- sentence BLEU-4 beside CIDEr (train.py --sc-bleu-weight)
// The arithmetic of include/s2vt_hip.h "sentence BLEU-4": integer clipped matches per order, then one fp64 chain on thread 0.  The
// brevity penalty needs exp and comes from the host (s2vt_bleu_table.bp).
struct BleuLds {
    int match[kCiderThreads / 64][4];
    unsigned long long near[kCiderThreads / 64];
};
// (|l - c|, l) of a reference length as one key: the minimum is the closest length, ties to the shorter
__device__ __forceinline__ unsigned long long bleu_near_key(int l, int c) {
    const int d = l < c ? c - l : l - c;
    return ((unsigned long long)(unsigned)d << 32) | (unsigned)l;
}
// number of entries equal to keys[at] from `at` on, in the ascending keys[0, n)
__device__ __forceinline__ int bleu_run(const uint64_t* keys, int at, int n) {
    const uint64_t key = keys[at];
    int tf = 1;
    while (at + tf < n && keys[at + tf] == key) ++tf;
    return tf;
}
// Every thread brings its part of the four match counts and of the keyed minimum over the reference lengths (every thread calls this;
// one barrier): sums and minimum over the workgroup - integers, exact in any order - and on thread 0 the chain
//   prod = (((1.0 * f_1) * f_2) * f_3) * f_4, f_k = (match_k + 1e-15) / (max(0, c - (k-1)) + 1e-9);  sqrt(sqrt(prod)) * bp[c][rl].
// The others return 0.
__device__ __forceinline__ double bleu_close(int c, int m0, int m1, int m2, int m3, unsigned long long near, const double* bp, int n_rl,
                                             BleuLds& S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m0 += __shfl_xor(m0, o, 64);
        m1 += __shfl_xor(m1, o, 64);
        m2 += __shfl_xor(m2, o, 64);
        m3 += __shfl_xor(m3, o, 64);
        const unsigned long long other = __shfl_xor(near, o, 64);
        near = other < near ? other : near;
    }
    if (lane == 0) {
        S.match[wave][0] = m0;
        S.match[wave][1] = m1;
        S.match[wave][2] = m2;
        S.match[wave][3] = m3;
        S.near[wave] = near;
    }
    __syncthreads();
    if (tid != 0) return 0.0;
    unsigned long long best = S.near[0];
    for (int w = 1; w < kCiderThreads / 64; ++w) best = S.near[w] < best ? S.near[w] : best;
    const unsigned url = (unsigned)(best & 0xFFFFFFFFull);
    const int rl = url < (unsigned)n_rl ? (int)url : n_rl - 1;      // (a length the table does not cover: its last column)
    double prod = 1.0;
    for (int k = 0; k < 4; ++k) {
        const int match = ((S.match[0][k] + S.match[1][k]) + S.match[2][k]) + S.match[3][k];
        const int guess = c - k > 0 ? c - k : 0;
        prod = prod * (((double)match + 1e-15) / ((double)guess + 1e-9));
    }
    return sqrt(sqrt(prod)) * bp[(int64_t)c * n_rl + rl];
}

// The BLEU phase of one row against the references of clip crow, on the sorted keys cider_candidate left in L (every thread calls it):
// a run head is an entry that differs from its predecessor - NOT wts != 0, a head whose idf is 0 weighs 0 -, the run's length is tf,
// a binary search in the clip's key range gives the largest count among the references.
__device__ __forceinline__ double bleu_reference(const s2vt_bleu_table& bt, int crow, int total, const CiderRowLds& L, BleuLds& S) {
    const int tid = threadIdx.x;
    const int c = L.m;
    const int64_t k0 = bt.clip_key_off[crow], k1 = bt.clip_key_off[crow + 1];
    int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int i = tid; i < total; i += kCiderThreads) {
        const uint64_t key = L.keys[i];
        if (i > 0 && L.keys[i - 1] == key) continue;
        const int64_t at = cider_find(bt.keys, k0, k1, key);
        if (at < 0) continue;
        const int tf = bleu_run(L.keys, i, total), rmax = bt.max_count[at], hit = tf < rmax ? tf : rmax;
        const int k = cider_key_order(key);
        if (k == 1) m0 += hit;
        else if (k == 2) m1 += hit;
        else if (k == 3) m2 += hit;
        else m3 += hit;
    }
    unsigned long long near = ~0ull;
    for (int r = bt.clip_ref_off[crow] + tid; r < bt.clip_ref_off[crow + 1]; r += kCiderThreads) {
        const unsigned long long key = bleu_near_key(bt.ref_words[r], c);
        near = key < near ? key : near;
    }
    return bleu_close(c, m0, m1, m2, m3, near, bt.bp, bt.n_rl, S);
}

// One workgroup = one candidate row; ONE candidate phase serves both scores.
__global__ __launch_bounds__(kCiderThreads) void mixed_rewards_kernel(s2vt_cider_table tb, s2vt_bleu_table bt, const int32_t* clip_rows,
                                                                      const int64_t* ids, int T, int64_t ld, int sos, int eos,
                                                                      double w_cider, double w_bleu, double* out, double* out_cider,
                                                                      double* out_bleu, int* err) {
    __shared__ CiderRowLds L;
    __shared__ double s_tot[kCiderThreads / 64][4];
    __shared__ BleuLds S;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int crow = clip_rows[b];
    if (crow < 0 || crow >= tb.n_clips) {         // the whole workgroup leaves together, before the first barrier
        if (tid == 0) {
            atomicExch(err, 2);
            out[b] = 0.0;
            if (out_cider) out_cider[b] = 0.0;
            if (out_bleu) out_bleu[b] = 0.0;
        }
        return;
    }
    const CiderRow cr = cider_candidate(tb, ids + (int64_t)b * ld, T, sos, eos, L, err);
    const double cider = cider_reference(tb, crow, cr, L, s_tot);
    const double bleu = bleu_reference(bt, crow, cr.total, L, S);
    if (tid == 0) {
        out[b] = w_cider * cider + w_bleu * bleu;
        if (out_cider) out_cider[b] = cider;
        if (out_bleu) out_bleu[b] = bleu;
    }
}

// ---------------------------------------------------------------- consensus (MBR) selection among the K candidates of a clip
// s2vt_cider_consensus in three launches over a per-call workspace of fixed-size slots, one per candidate row r = b * K + k:
//   keys / wts [R][slot]   the row's sorted keys and run-head weights as cider_candidate leaves them (slot = 4 T >= total entries)
//   norm [R][4], meta [R][2] = {total, n2}
// The lookup of a key in another candidate's slot is a lower bound over ALL its entries: equal keys are adjacent, the lower bound
// is the run's head, which carries the weight; a key names its own order, so the orders need no segments of their own.
struct ConsensusWs { uint64_t* keys; double* wts; double* norm; int32_t* meta; int64_t slot; };

// Phase 1.  One workgroup = one candidate row; a row that is not valid is not read (its meta says "no entries").
__global__ __launch_bounds__(kCiderThreads) void consensus_candidate_kernel(s2vt_cider_table tb, const int64_t* ids, int T, int64_t ld,
                                                                            int sos, int eos, const uint8_t* valid, ConsensusWs ws,
                                                                            int* err) {
    __shared__ CiderRowLds L;
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    if (valid && !valid[r]) {                     // the whole workgroup leaves together, before the first barrier
        if (tid == 0) ws.meta[2 * r] = ws.meta[2 * r + 1] = 0;
        return;
    }
    const CiderRow cr = cider_candidate(tb, ids + r * ld, T, sos, eos, L, err);
    uint64_t* keys = ws.keys + r * ws.slot;
    double* wts = ws.wts + r * ws.slot;
    for (int i = tid; i < cr.total; i += kCiderThreads) {        // total <= 4 T = slot
        keys[i] = L.keys[i];
        wts[i] = L.wts[i];
    }
    if (tid < 4) ws.norm[4 * r + tid] = L.hn[tid];
    if (tid == 0) {
        ws.meta[2 * r] = cr.total;
        ws.meta[2 * r + 1] = cr.n2;
    }
}

struct PairLds {
    uint64_t keys[kCiderMaxN];
    double wts[kCiderMaxN];
    double term[S2VT_CONSENSUS_MAX_K][4];
    double tot[4];
};
// Phase 2.  One workgroup = one (clip b, candidate i): CIDEr-D of i with the clip's other valid candidates as its references.
// Wavefront w takes the others j = w, w + 4, ..; its lanes share i's run heads (entry e to lane e mod 64, ascending) and a butterfly
// closes each per-order sum, as cider_rewards_kernel does against a reference.  The pair's four terms dot / norms * penalty wait in
// LDS; one thread per order then adds them in ascending j from 0.0 - the host's order over the others - whatever wavefront made them.
// consensus_pair_cider is that phase for valid candidate row r = r0 + i, by the whole workgroup (every thread calls it; it holds barriers): loads r's slot into
// P and leaves it there; thread 0 returns the CIDEr utility (0.0 without another valid candidate) and, in *others_out, the number of
// others; the rest return 0.  consensus_pair_kernel and mixed_pair_kernel share it, so the two give the same bits.
__device__ __forceinline__ double consensus_pair_cider(const s2vt_cider_table& tb, int K, const uint8_t* valid, const ConsensusWs& ws,
                                                       int64_t r, PairLds& P, int* others_out) {
    uint64_t* keys = P.keys;
    double* wts = P.wts;
    double (*s_term)[4] = P.term;
    double* s_tot = P.tot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = r - r % K;                 // the clip's first row
    const int i = (int)(r - r0);
    const int total = ws.meta[2 * r], n2 = ws.meta[2 * r + 1];
    for (int e = tid; e < total; e += kCiderThreads) {
        keys[e] = ws.keys[r * ws.slot + e];
        wts[e] = ws.wts[r * ws.slot + e];
    }
    __syncthreads();
    const double* hn = ws.norm + 4 * r;
    for (int j = wave; j < K; j += kCiderThreads / 64) {
        const int64_t rj = r0 + j;
        if (j == i || (valid && !valid[rj])) continue;           // (uniform over the wavefront)
        const uint64_t* jk = ws.keys + rj * ws.slot;
        const double* jw = ws.wts + rj * ws.slot;
        const int tj = ws.meta[2 * rj];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int e = lane; e < total; e += 64) {
            const double w = wts[e];
            if (w == 0.0) continue;               // not the head of a run, or idf 0: contributes exactly 0
            const uint64_t key = keys[e];
            const int64_t at = cider_find(jk, 0, tj, key);
            if (at < 0) continue;
            const double wr = jw[at];
            const double c = (w < wr ? w : wr) * wr;
            const int k = cider_key_order(key) - 1;
            if (k == 0) a0 += c;
            else if (k == 1) a1 += c;
            else if (k == 2) a2 += c;
            else a3 += c;
        }
        a0 = cider_wave_sum(a0);
        a1 = cider_wave_sum(a1);
        a2 = cider_wave_sum(a2);
        a3 = cider_wave_sum(a3);
        int d = n2 - ws.meta[2 * rj + 1];
        d = d < 0 ? -d : d;
        const double pen = tb.pen[d < tb.n_pen ? d : tb.n_pen - 1];
        const double* rn = ws.norm + 4 * rj;
        if (hn[0] != 0.0 && rn[0] != 0.0) a0 /= hn[0] * rn[0];
        if (hn[1] != 0.0 && rn[1] != 0.0) a1 /= hn[1] * rn[1];
        if (hn[2] != 0.0 && rn[2] != 0.0) a2 /= hn[2] * rn[2];
        if (hn[3] != 0.0 && rn[3] != 0.0) a3 /= hn[3] * rn[3];
        if (lane == 0) {
            s_term[j][0] = a0 * pen;
            s_term[j][1] = a1 * pen;
            s_term[j][2] = a2 * pen;
            s_term[j][3] = a3 * pen;
        }
    }
    __syncthreads();
    int others = 0;
    if (tid < 4) {
        double t = 0.0;
        for (int j = 0; j < K; ++j) {
            if (j == i || (valid && !valid[r0 + j])) continue;
            t += s_term[j][tid];
            ++others;
        }
        s_tot[tid] = t;
    }
    __syncthreads();
    *others_out = others;
    if (tid != 0) return 0.0;
    const double mean = (((s_tot[0] + s_tot[1]) + s_tot[2]) + s_tot[3]) / 4.0;
    return others ? mean / (double)others * 10.0 : 0.0;
}

__global__ __launch_bounds__(kCiderThreads) void consensus_pair_kernel(s2vt_cider_table tb, int K, const uint8_t* valid, ConsensusWs ws,
                                                                       double* utility) {
    __shared__ PairLds P;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (valid && !valid[r]) {                     // the whole workgroup leaves together, before the first barrier
        if (tid == 0) utility[r] = -__builtin_inf();
        return;
    }
    int others;
    const double u = consensus_pair_cider(tb, K, valid, ws, r, P, &others);
    if (tid == 0) utility[r] = u;
}

// The same with the BLEU utility beside it: for every run head of candidate i the largest run length at the key's lower bound in the
// slots of the other valid j (equal keys are adjacent there as well), rl from the others' word counts, then w_cider * CIDEr +
// w_bleu * BLEU-4 in fp64.  A slot's word count follows from its meta: 0 or 1 entries are 0 or 1 words, else bigrams + 1.
__device__ __forceinline__ int consensus_words(const int32_t* meta, int64_t r) {
    const int total = meta[2 * r];
    return total < 2 ? total : meta[2 * r + 1] + 1;
}
__global__ __launch_bounds__(kCiderThreads) void mixed_pair_kernel(s2vt_cider_table tb, const double* bp, int n_rl, int K,
                                                                   const uint8_t* valid, ConsensusWs ws, double w_cider, double w_bleu,
                                                                   double* utility) {
    __shared__ PairLds P;
    __shared__ BleuLds S;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (valid && !valid[r]) {                     // the whole workgroup leaves together, before the first barrier
        if (tid == 0) utility[r] = -__builtin_inf();
        return;
    }
    int others;
    const double cider = consensus_pair_cider(tb, K, valid, ws, r, P, &others);
    const int64_t r0 = r - r % K;
    const int i = (int)(r - r0);
    const int total = ws.meta[2 * r], c = consensus_words(ws.meta, r);
    int m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int e = tid; e < total; e += kCiderThreads) {
        const uint64_t key = P.keys[e];
        if (e > 0 && P.keys[e - 1] == key) continue;
        int rmax = 0;
        for (int j = 0; j < K; ++j) {
            const int64_t rj = r0 + j;
            if (j == i || (valid && !valid[rj])) continue;
            const uint64_t* jk = ws.keys + rj * ws.slot;
            const int tj = ws.meta[2 * rj];
            const int64_t at = cider_find(jk, 0, tj, key);
            if (at < 0) continue;
            const int run = bleu_run(jk, (int)at, tj);
            rmax = run > rmax ? run : rmax;
        }
        const int tf = bleu_run(P.keys, e, total), hit = tf < rmax ? tf : rmax;
        const int k = cider_key_order(key);
        if (k == 1) m0 += hit;
        else if (k == 2) m1 += hit;
        else if (k == 3) m2 += hit;
        else m3 += hit;
    }
    unsigned long long near = ~0ull;
    for (int j = tid; j < K; j += kCiderThreads) {
        if (j == i || (valid && !valid[r0 + j])) continue;
        const unsigned long long key = bleu_near_key(consensus_words(ws.meta, r0 + j), c);
        near = key < near ? key : near;
    }
    const double bleu = bleu_close(c, m0, m1, m2, m3, near, bp, n_rl, S);      // (without others: near stays ~0, the value is not used)
    if (tid == 0) utility[r] = others ? w_cider * cider + w_bleu * bleu : 0.0;
}

// Phase 3.  One wavefront = one clip, lane k its candidate k (K <= 64): the smallest valid k whose utility is the maximum, 0 without
// a valid one.  max is exact in any order; the ballot picks the first lane.
__global__ __launch_bounds__(64) void consensus_best_kernel(int K, const uint8_t* valid, const double* utility, int32_t* best) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t r = (int64_t)b * K + lane;
    const bool ok = lane < K && (!valid || valid[r]);
    const double u = ok ? utility[r] : -__builtin_inf();
    double m = u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    const unsigned long long hit = __ballot(ok && u == m);
    if (lane == 0) best[b] = hit ? __ffsll((long long)hit) - 1 : 0;
}

// One workgroup = one row of sampled ids.
__global__ __launch_bounds__(kCiderThreads) void sc_weights_kernel(const int64_t* sampled, const double* r_sample, const double* r_greedy,
                                                                   int T, int sos, int eos, int64_t* caps, float* weight) {
    __shared__ int s_first;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t* row = sampled + (int64_t)b * T;
    if (tid == 0) s_first = T;
    __syncthreads();
    for (int i = tid; i < T; i += kCiderThreads)
        if (row[i] == (int64_t)eos) atomicMin(&s_first, i);
    __syncthreads();
    const int first = s_first;                    // index of the first <eos>, T without one
    const float adv = (float)(r_sample[b] - r_greedy[b]);
    int64_t* crow = caps + (int64_t)b * (T + 1);
    float* wrow = weight + (int64_t)b * (T + 1);
    if (tid == 0) {
        crow[0] = sos;
        wrow[0] = 0.0f;
    }
    for (int i = tid; i < T; i += kCiderThreads) {
        crow[1 + i] = row[i];
        wrow[1 + i] = (i <= first ? 1.0f : 0.0f) * adv;
    }
}

// One wavefront = one clip and its K rows r = b * K + k.  Baseline of row k: r_greedy[b], or without it the mean of the OTHER K - 1
// rewards - the K rewards summed in ascending k from 0.0, minus the row's own, divided by K - 1: adds, one subtract, one divide in
// fp64, no product (nothing to contract); a clip whose K rewards compare equal takes that reward itself.  Every lane walks the same K
// numbers, so the sum needs no exchange.
constexpr int kGroupThreads = 64;
__global__ __launch_bounds__(kGroupThreads) void sc_weights_group_kernel(const int64_t* sampled, const double* r_sample,
                                                                         const double* r_greedy, int K, int T, int sos, int eos,
                                                                         int64_t* caps, float* weight, double* baseline) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* rs = r_sample + (int64_t)b * K;
    double sum = 0.0;
    bool same = !r_greedy;                        // all K rewards equal: the baseline IS that reward (see the header)
    if (!r_greedy)
        for (int j = 0; j < K; ++j) {
            sum += rs[j];
            same = same && rs[j] == rs[0];
        }
    for (int k = 0; k < K; ++k) {
        const int64_t r = (int64_t)b * K + k;
        const int64_t* row = sampled + r * T;
        int first = T;                            // index of the first <eos>, T without one
        for (int i = lane; i < T; i += kGroupThreads)
            if (row[i] == (int64_t)eos) { first = i; break; }
        for (int o = kGroupThreads / 2; o > 0; o >>= 1) {
            const int other = __shfl_xor(first, o, kGroupThreads);
            first = other < first ? other : first;
        }
        const double base = r_greedy ? r_greedy[b] : same ? rs[k] : (sum - rs[k]) / (double)(K - 1);
        const float adv = (float)(rs[k] - base);
        int64_t* crow = caps + r * (T + 1);
        float* wrow = weight + r * (T + 1);
        if (lane == 0) {
            crow[0] = sos;
            wrow[0] = 0.0f;
            if (baseline) baseline[r] = base;
        }
        for (int i = lane; i < T; i += kGroupThreads) {
            crow[1 + i] = row[i];
            wrow[1 + i] = i <= first ? adv : 0.0f;
        }
    }
}

// Without-replacement weights (include/s2vt_hip.h, "without-replacement weights"): the K rows of a clip are the K distinct captions of
// one stochastic beam search, logprob their log-probs phi and kappa the search's threshold.  The same shape as the kernel above - one
// wavefront per clip, every lane walking the same K numbers, no exchange - with the header's steps 1-6 in fp64 in front of the rows'
// copy: each sum in ascending i from 0.0, exp / expm1 / log the only calls, products and sums kept apart (contraction is off in this
// file).  K <= S2VT_SWOR_MAX_K and the loops are unrolled to it, so the per-row values stay in registers.
constexpr int kSworMaxK = S2VT_SWOR_MAX_K;
__global__ __launch_bounds__(kGroupThreads) void sc_weights_swor_kernel(const int64_t* sampled, const float* logprob, const float* kappa,
                                                                        const double* r_sample, const double* r_greedy, int K, int T,
                                                                        int sos, int eos, int64_t* caps, float* weight, double* coef,
                                                                        double* baseline) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double inf = __builtin_inf();
    const double* rs = r_sample + (int64_t)b * K;
    const float* lp = logprob + (int64_t)b * K;
    const double kap = (double)kappa[b];
    bool bad = kap != kap || kap == inf || (r_greedy && !(fabs(r_greedy[b]) < inf));
    bool same = !r_greedy;                        // all K rewards equal: every advantage is exactly 0 (see the header)
    double lw[kSworMaxK], phi[kSworMaxK], m = -inf;
#pragma unroll
    for (int i = 0; i < kSworMaxK; ++i) {
        lw[i] = phi[i] = 0.0;
        if (i < K) {
            phi[i] = (double)lp[i];
            bad = bad || !(fabs(phi[i]) < inf) || phi[i] > 0.0 || !(fabs(rs[i]) < inf);
            same = same && rs[i] == rs[0];
            const double a = phi[i] - kap;        // +inf for kap = -inf: e = +inf, lq = log(1) = 0
            const double e = exp(a);
            const double lq = a < -30.0 ? a - 0.5 * e : log(-expm1(-e));
            lw[i] = phi[i] - lq;
            m = lw[i] > m ? lw[i] : m;
        }
    }
    double om[kSworMaxK], W = 0.0, N = 0.0;
#pragma unroll
    for (int i = 0; i < kSworMaxK; ++i) {
        om[i] = 0.0;
        if (i < K && !bad) {
            om[i] = exp(lw[i] - m);
            W += om[i];
            N += om[i] * rs[i];
        }
    }
    const double base = bad ? __builtin_nan("") : r_greedy ? r_greedy[b] : same ? rs[0] : N / W;
    double c[kSworMaxK], adv[kSworMaxK];
#pragma unroll
    for (int i = 0; i < kSworMaxK; ++i) {
        c[i] = adv[i] = 0.0;
        if (i < K && !bad) {
            const double Wi = (W - om[i]) + exp(phi[i] - m);
            c[i] = om[i] / Wi;
            adv[i] = same ? 0.0 : c[i] * (rs[i] - base);
        }
    }
    bool wild = false;                            // a weight that fp32 does not hold (finite rewards can be that large): a bad clip
#pragma unroll
    for (int i = 0; i < kSworMaxK; ++i)
        if (i < K) wild = wild || !(fabsf((float)adv[i]) < __builtin_inff());
    if (lane == 0 && baseline) baseline[b] = wild ? __builtin_nan("") : base;
#pragma unroll
    for (int k = 0; k < kSworMaxK; ++k) {
        if (k >= K) break;
        const int64_t r = (int64_t)b * K + k;
        const int64_t* row = sampled + r * T;
        int first = T;                            // index of the first <eos>, T without one
        for (int i = lane; i < T; i += kGroupThreads)
            if (row[i] == (int64_t)eos) { first = i; break; }
        for (int o = kGroupThreads / 2; o > 0; o >>= 1) {
            const int other = __shfl_xor(first, o, kGroupThreads);
            first = other < first ? other : first;
        }
        const float w = wild ? 0.0f : (float)adv[k];
        int64_t* crow = caps + r * (T + 1);
        float* wrow = weight + r * (T + 1);
        if (lane == 0) {
            crow[0] = sos;
            wrow[0] = 0.0f;
            if (coef) coef[r] = wild ? 0.0 : c[k];
        }
        for (int i = lane; i < T; i += kGroupThreads) {
            crow[1 + i] = row[i];
            wrow[1 + i] = i <= first ? w : 0.0f;
        }
    }
}

}  // namespace s2vt

using namespace s2vt;

extern "C" {

int s2vt_cider_rewards(const s2vt_cider_table* table, const int32_t* clip_rows, const int64_t* ids, int32_t B, int32_t T, int64_t ld,
                       int32_t sos, int32_t eos, double* out, void* stream) {
    S2VT_REQUIRE(table && clip_rows && ids && out, "s2vt_cider_rewards: null argument");
    S2VT_REQUIRE(B > 0 && T > 0 && ld >= T, "s2vt_cider_rewards: bad dims (B %d, T %d, ld %lld)", (int)B, (int)T, (long long)ld);
    S2VT_REQUIRE(T <= S2VT_CIDER_MAX_T, "s2vt_cider_rewards: T = %d ids per row, the n-gram list in LDS holds rows of up to %d", (int)T,
                 S2VT_CIDER_MAX_T);
    const s2vt_cider_table& tb = *table;
    S2VT_REQUIRE(tb.clip_ref_off && tb.ent_off && tb.ref_norm && tb.ref_len && tb.pen && tb.n_clips > 0 && tb.n_refs > 0 && tb.n_pen > 0 &&
                     tb.n_idf >= 0 && (tb.n_idf == 0 || (tb.idf_keys && tb.idf_vals)),
                 "s2vt_cider_rewards: incomplete table");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    hipLaunchKernelGGL(cider_rewards_kernel, dim3((unsigned)B), dim3(kCiderThreads), 0, st, tb, clip_rows, ids, (int)T, ld, (int)sos,
                       (int)eos, out, flags.p);
    S2VT_LAUNCH_CHECK("cider_rewards_kernel");
    // two calls per self-critical step: the ring of records, so that a call never waits for the copy of the one before it
    return flags.close(st, 3);
}

// the consensus workspace: keys, wts [R][4 T], norm [R][4], meta [R][2], each part on a 256-byte boundary
static bool consensus_dims_ok(int32_t B, int32_t K, int32_t T) {
    return B > 0 && K >= 1 && K <= S2VT_CONSENSUS_MAX_K && T >= 1 && T <= S2VT_CIDER_MAX_T;
}
static size_t carve_consensus(int32_t B, int32_t K, int32_t T, void* base, ConsensusWs* ws) {
    Carver c{static_cast<char*>(base), 0, 0};
    const size_t R = (size_t)B * (size_t)K, slot = 4 * (size_t)T;
    ConsensusWs w;
    w.keys = c.take<uint64_t>(R * slot);
    w.wts = c.take<double>(R * slot);
    w.norm = c.take<double>(R * 4);
    w.meta = c.take<int32_t>(R * 2);
    w.slot = (int64_t)slot;
    if (ws) *ws = w;
    return align_up(c.off, 256);
}

size_t s2vt_cider_consensus_workspace_bytes(int32_t B, int32_t K, int32_t T) {
    return consensus_dims_ok(B, K, T) ? carve_consensus(B, K, T, nullptr, nullptr) : 0;
}

int s2vt_cider_consensus(const s2vt_cider_table* table, const int64_t* ids, int32_t B, int32_t K, int32_t T, int64_t ld, int32_t sos,
                         int32_t eos, const uint8_t* valid, double* utility, int32_t* best, void* workspace, size_t workspace_bytes,
                         void* stream) {
    S2VT_REQUIRE(table && ids && utility && best && workspace, "s2vt_cider_consensus: null argument");
    S2VT_REQUIRE(consensus_dims_ok(B, K, T) && ld >= T,
                 "s2vt_cider_consensus: bad dims (B %d, K %d of 1..%d, T %d of 1..%d: the n-gram list in LDS, ld %lld)", (int)B, (int)K,
                 S2VT_CONSENSUS_MAX_K, (int)T, S2VT_CIDER_MAX_T, (long long)ld);
    S2VT_REQUIRE((int64_t)B * K <= 0x7FFFFFFF, "s2vt_cider_consensus: B * K = %lld rows, one workgroup each", (long long)B * K);
    S2VT_REQUIRE(workspace_bytes >= s2vt_cider_consensus_workspace_bytes(B, K, T), "s2vt_cider_consensus: workspace of %zu bytes, %zu needed",
                 workspace_bytes, s2vt_cider_consensus_workspace_bytes(B, K, T));
    const s2vt_cider_table& tb = *table;          // the kernels read idf_keys, idf_vals, n_idf, log_n, pen and n_pen alone
    S2VT_REQUIRE(tb.pen && tb.n_pen > 0 && tb.n_idf >= 0 && (tb.n_idf == 0 || (tb.idf_keys && tb.idf_vals)),
                 "s2vt_cider_consensus: incomplete table");
    hipStream_t st = (hipStream_t)stream;
    ConsensusWs ws;
    carve_consensus(B, K, T, workspace, &ws);
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    const unsigned R = (unsigned)((int64_t)B * K);
    hipLaunchKernelGGL(consensus_candidate_kernel, dim3(R), dim3(kCiderThreads), 0, st, tb, ids, (int)T, ld, (int)sos, (int)eos, valid, ws,
                       flags.p);
    S2VT_LAUNCH_CHECK("consensus_candidate_kernel");
    hipLaunchKernelGGL(consensus_pair_kernel, dim3(R), dim3(kCiderThreads), 0, st, tb, (int)K, valid, ws, utility);
    S2VT_LAUNCH_CHECK("consensus_pair_kernel");
    hipLaunchKernelGGL(consensus_best_kernel, dim3((unsigned)B), dim3(64), 0, st, (int)K, valid, utility, best);
    S2VT_LAUNCH_CHECK("consensus_best_kernel");
    return flags.close(st, 3);
}

static bool finite_weight(double w) { return w - w == 0.0; }

int s2vt_mixed_rewards(const s2vt_cider_table* table, const s2vt_bleu_table* bleu, const int32_t* clip_rows, const int64_t* ids, int32_t B,
                       int32_t T, int64_t ld, int32_t sos, int32_t eos, double w_cider, double w_bleu, double* out, double* out_cider,
                       double* out_bleu, void* stream) {
    S2VT_REQUIRE(table && bleu && clip_rows && ids && out, "s2vt_mixed_rewards: null argument");
    S2VT_REQUIRE(B > 0 && T > 0 && ld >= T, "s2vt_mixed_rewards: bad dims (B %d, T %d, ld %lld)", (int)B, (int)T, (long long)ld);
    S2VT_REQUIRE(T <= S2VT_CIDER_MAX_T, "s2vt_mixed_rewards: T = %d ids per row, the n-gram list in LDS holds rows of up to %d", (int)T,
                 S2VT_CIDER_MAX_T);
    S2VT_REQUIRE(finite_weight(w_cider) && finite_weight(w_bleu), "s2vt_mixed_rewards: the weights must be finite");
    const s2vt_cider_table& tb = *table;
    S2VT_REQUIRE(tb.clip_ref_off && tb.ent_off && tb.ref_norm && tb.ref_len && tb.pen && tb.n_clips > 0 && tb.n_refs > 0 && tb.n_pen > 0 &&
                     tb.n_idf >= 0 && (tb.n_idf == 0 || (tb.idf_keys && tb.idf_vals)),
                 "s2vt_mixed_rewards: incomplete table");
    const s2vt_bleu_table& bt = *bleu;
    S2VT_REQUIRE(bt.clip_key_off && bt.clip_ref_off && bt.ref_words && bt.bp && bt.n_clips == tb.n_clips && bt.n_refs > 0 &&
                     bt.n_rl > S2VT_CIDER_MAX_T && bt.n_keys >= 0 && (bt.n_keys == 0 || (bt.keys && bt.max_count)),
                 "s2vt_mixed_rewards: incomplete BLEU table (or one of other clips than the CIDEr table's)");
    hipStream_t st = (hipStream_t)stream;
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    hipLaunchKernelGGL(mixed_rewards_kernel, dim3((unsigned)B), dim3(kCiderThreads), 0, st, tb, bt, clip_rows, ids, (int)T, ld, (int)sos,
                       (int)eos, w_cider, w_bleu, out, out_cider, out_bleu, flags.p);
    S2VT_LAUNCH_CHECK("mixed_rewards_kernel");
    return flags.close(st, 3);
}

size_t s2vt_mixed_consensus_workspace_bytes(int32_t B, int32_t K, int32_t T) {
    return consensus_dims_ok(B, K, T) ? carve_consensus(B, K, T, nullptr, nullptr) : 0;
}

int s2vt_mixed_consensus(const s2vt_cider_table* table, const s2vt_bleu_table* bleu, const int64_t* ids, int32_t B, int32_t K, int32_t T,
                         int64_t ld, int32_t sos, int32_t eos, const uint8_t* valid, double w_cider, double w_bleu, double* utility,
                         int32_t* best, void* workspace, size_t workspace_bytes, void* stream) {
    S2VT_REQUIRE(table && bleu && ids && utility && best && workspace, "s2vt_mixed_consensus: null argument");
    S2VT_REQUIRE(consensus_dims_ok(B, K, T) && ld >= T,
                 "s2vt_mixed_consensus: bad dims (B %d, K %d of 1..%d, T %d of 1..%d: the n-gram list in LDS, ld %lld)", (int)B, (int)K,
                 S2VT_CONSENSUS_MAX_K, (int)T, S2VT_CIDER_MAX_T, (long long)ld);
    S2VT_REQUIRE((int64_t)B * K <= 0x7FFFFFFF, "s2vt_mixed_consensus: B * K = %lld rows, one workgroup each", (long long)B * K);
    S2VT_REQUIRE(workspace_bytes >= s2vt_mixed_consensus_workspace_bytes(B, K, T), "s2vt_mixed_consensus: workspace of %zu bytes, %zu needed",
                 workspace_bytes, s2vt_mixed_consensus_workspace_bytes(B, K, T));
    S2VT_REQUIRE(finite_weight(w_cider) && finite_weight(w_bleu), "s2vt_mixed_consensus: the weights must be finite");
    const s2vt_cider_table& tb = *table;          // as s2vt_cider_consensus: idf_keys, idf_vals, n_idf, log_n, pen and n_pen alone
    S2VT_REQUIRE(tb.pen && tb.n_pen > 0 && tb.n_idf >= 0 && (tb.n_idf == 0 || (tb.idf_keys && tb.idf_vals)),
                 "s2vt_mixed_consensus: incomplete table");
    S2VT_REQUIRE(bleu->bp && bleu->n_rl > S2VT_CIDER_MAX_T, "s2vt_mixed_consensus: incomplete BLEU table (bp)");
    hipStream_t st = (hipStream_t)stream;
    ConsensusWs ws;
    carve_consensus(B, K, T, workspace, &ws);
    PostedFlags flags;
    int rc;
    if ((rc = flags.open(st))) return rc;
    const unsigned R = (unsigned)((int64_t)B * K);
    hipLaunchKernelGGL(consensus_candidate_kernel, dim3(R), dim3(kCiderThreads), 0, st, tb, ids, (int)T, ld, (int)sos, (int)eos, valid, ws,
                       flags.p);
    S2VT_LAUNCH_CHECK("consensus_candidate_kernel");
    hipLaunchKernelGGL(mixed_pair_kernel, dim3(R), dim3(kCiderThreads), 0, st, tb, bleu->bp, (int)bleu->n_rl, (int)K, valid, ws, w_cider,
                       w_bleu, utility);
    S2VT_LAUNCH_CHECK("mixed_pair_kernel");
    hipLaunchKernelGGL(consensus_best_kernel, dim3((unsigned)B), dim3(64), 0, st, (int)K, valid, utility, best);
    S2VT_LAUNCH_CHECK("consensus_best_kernel");
    return flags.close(st, 3);
}

int s2vt_sc_weights(const int64_t* sampled, const double* r_sample, const double* r_greedy, int32_t B, int32_t T, int32_t sos,
                    int32_t eos, int64_t* caps, float* weight, void* stream) {
    S2VT_REQUIRE(sampled && r_sample && r_greedy && caps && weight, "s2vt_sc_weights: null argument");
    S2VT_REQUIRE(B > 0 && T > 0, "s2vt_sc_weights: bad dims (B %d, T %d)", (int)B, (int)T);
    hipLaunchKernelGGL(sc_weights_kernel, dim3((unsigned)B), dim3(kCiderThreads), 0, (hipStream_t)stream, sampled, r_sample, r_greedy,
                       (int)T, (int)sos, (int)eos, caps, weight);
    S2VT_LAUNCH_CHECK("sc_weights_kernel");
    return 0;
}

int s2vt_sc_weights_group(const int64_t* sampled, const double* r_sample, const double* r_greedy, int32_t B, int32_t K, int32_t T,
                          int32_t sos, int32_t eos, int64_t* caps, float* weight, double* baseline, void* stream) {
    S2VT_REQUIRE(sampled && r_sample && caps && weight, "s2vt_sc_weights_group: null argument");
    S2VT_REQUIRE(B > 0 && K > 0 && T > 0, "s2vt_sc_weights_group: bad dims (B %d, K %d, T %d)", (int)B, (int)K, (int)T);
    S2VT_REQUIRE(r_greedy || K >= 2, "s2vt_sc_weights_group: the mean of the other K - 1 rewards needs K >= 2 (got K = %d)", (int)K);
    hipLaunchKernelGGL(sc_weights_group_kernel, dim3((unsigned)B), dim3(kGroupThreads), 0, (hipStream_t)stream, sampled, r_sample,
                       r_greedy, (int)K, (int)T, (int)sos, (int)eos, caps, weight, baseline);
    S2VT_LAUNCH_CHECK("sc_weights_group_kernel");
    return 0;
}

int s2vt_sc_weights_swor(const int64_t* sampled, const float* logprob, const float* kappa, const double* r_sample, const double* r_greedy,
                         int32_t B, int32_t K, int32_t T, int32_t sos, int32_t eos, int64_t* caps, float* weight, double* coef,
                         double* baseline, void* stream) {
    S2VT_REQUIRE(sampled && logprob && kappa && r_sample && caps && weight, "s2vt_sc_weights_swor: null argument");
    S2VT_REQUIRE(B > 0 && K >= 2 && K <= S2VT_SWOR_MAX_K && T > 0, "s2vt_sc_weights_swor: bad dims (B %d, K %d of 2..%d, T %d)", (int)B,
                 (int)K, S2VT_SWOR_MAX_K, (int)T);
    hipLaunchKernelGGL(sc_weights_swor_kernel, dim3((unsigned)B), dim3(kGroupThreads), 0, (hipStream_t)stream, sampled, logprob, kappa,
                       r_sample, r_greedy, (int)K, (int)T, (int)sos, (int)eos, caps, weight, coef, baseline);
    S2VT_LAUNCH_CHECK("sc_weights_swor_kernel");
    return 0;
}

}  // extern "C"
