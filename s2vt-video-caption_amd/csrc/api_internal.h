// Host-side internals shared by the C-ABI units of libs2vt_hip.so:
//   api_runtime.hip  errors, asynchronous device-side errors, live timing, launch-sequence capture, the side stream, setters
//   api_shared.hip   plane-operand helpers (split / GEMM wrappers), the drivers' lane frame and shared prologues, recurrence loops, argument builders
//   api_train.hip    s2vt_train_forward / s2vt_train_backward (+ dropout, fused criterion backward, gradient-group events): the plane drivers
//   api_train_f32.hip  the fp32-MFMA launch-per-timestep train driver, plain (behind s2vt_train_forward / _backward) and grouped
//                    (s2vt_train_group_forward / _backward: mode='train' on K captions per clip, one encode per clip)
//   api_decode.hip   greedy / sampled / scheduled decode and the encode phase for the beam search (DecodeDriver: one function per
//                    schedule, chosen by decode_plan below), the decode step's argmax entry points
//   api_beam.hip     the batched beam-search depth step
//   api_score.hip    teacher-forced caption scoring (S2VT.forward(mode='score'))
//   api_sample_rows.hip  K sampled captions per clip on one encode (S2VT.sample), plain and with top-k / nucleus truncation; the
//                    truncated draw and the top-20 fan-out as per-op entry points
//   api_ops.hip      per-op entry points (GEMM, split, timestep / sequence kernels, criterion)
// Host code only; every kernel lives in gemm* / lstm* / ce / truncate / misc / group / split / argmax_x3 / beam_queue / beam_policy.hip.
#pragma once
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/s2vt_hip.h"
#include "common.h"
#include "kernels.h"

namespace s2vt {

// ------------------------------------------------------------------ api_runtime.hip
#ifdef S2VT_EXPERIMENT_STAMPS
extern unsigned long long* g_xstamps;     // timing experiments only (experiment.h)
extern int g_xstamp_block;
#endif
const char* last_error_text();

// asynchronous device-side errors (kind: 0 forward / decode, 1 backward, 2 loss, 3 a ring of eight for the beam depth steps)
int poll_async_error(bool wait);
int post_async_error(hipStream_t st, const int* dev_flags, int kind = 0);
int device_flags(int** out);
// The flag words of a per-op entry point that has no workspace of its own, and the protocol around them: open() before the
// work - fetch the device's words, poll (an earlier call's error, if its flags have arrived, is kept), zero the words on st;
// close() after it - that earlier error if there was one, else post this call's flags as a record of `kind`.  A PostedFlags
// that was never opened (p == nullptr: the call reads no id of the caller's) closes as 0 without posting.
struct PostedFlags {
    int* p = nullptr;
    int rc0 = 0;
    int open(hipStream_t st);
    int close(hipStream_t st, int kind);
};

// live kernel timing: launch sites bracket kernels of one kind with hipEvents on the launch stream while s2vt_prof_enable(1)
enum { K_GEMM = 0, K_STEP_FWD = 1, K_STEP_BWD = 2, K_CE = 3, K_ARGMAX = 4, K_GEMM_CORUN = 5, K_NKINDS = 6 };   // (5: a GEMM planned for PART of the
                                                                                                               //  compute units, beside a one-layer persistent launch)
struct ProfRec { hipEvent_t a, b; int kind; int64_t launches; };
struct ProfScope {
    hipStream_t s; bool on; ProfRec r;
    ProfScope(hipStream_t stream, int kind, int64_t launches);
    ~ProfScope();
};
bool prof_on();

// launch-sequence capture (option "graph"): see api_runtime.hip
bool graph_on();
bool graph_capturing();                   // this thread is inside a capture (nothing may record an external event)
int run_graphed(hipStream_t st, const std::vector<uint64_t>& key, const std::function<int(hipStream_t)>& enqueue, bool* graphed = nullptr);
static inline void key_ptr(std::vector<uint64_t>& k, const void* p) { k.push_back((uint64_t)(uintptr_t)p); }

static const RowMap ID = {nullptr, 0, 0};
static inline RowMap perm(int inner, int outer) { return RowMap{nullptr, inner, outer}; }
static inline RowMap gather(const int32_t* idx) { return RowMap{idx, 0, 0}; }

// split-K scratch of the driver that is running (set by the whole-path entry points from their workspace)
extern thread_local float* g_gws;
extern thread_local size_t g_gws_floats;
struct GemmWsScope {
    GemmWsScope(float* p, size_t n) { g_gws = p; g_gws_floats = n; }
    ~GemmWsScope() { g_gws = nullptr; g_gws_floats = 0; }
};
// fp32-MFMA GEMM with the split-K scratch of the running driver
int gemm(hipStream_t st, bool ak, bool bk, int M, int N, int K, const float* A, int64_t lda, RowMap am, const float* B, int64_t ldb,
         RowMap bm, float* C, int64_t ldc, RowMap cm, const float* bias, bool acc);
size_t gemm_ws_floats(const s2vt_dims& d);      // scratch floats for split-K slabs of a whole-path driver

struct Carver {
    char* base; size_t off; size_t cap;
    template <typename T> T* take(size_t n) {
        off = align_up(off, 256);
        T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
        off += n * sizeof(T);
        return p;
    }
};
// Batches that are not multiples of 64 in a plane mode: from option pad_min_batch rows on (default 33; a greedy decode: three
// quarters of it, 24) the whole-path drivers pad them to the next multiple of 64 inside their workspace; smaller batches run as
// they are on the launch-per-timestep fp32-MFMA path, which is faster there (train step at B = 16, H = 512: 4.4 vs 5.8 ms, at
// B = 48: 6.8 vs 6.1; decode at B = 16, H = 1000: 4.2 vs 4.5 ms, at B = 32: 5.5 vs 4.6; profiles/round5_ragged_batches.txt)
static inline bool batch_pads(int B, bool decode = false) {
    const int from = decode ? option(O_PAD_MIN_BATCH) * 3 / 4 : option(O_PAD_MIN_BATCH);
    return option(O_GEMM_MODE) != 0 && B % 64 != 0 && B >= (from > 0 ? from : 1);
}
static inline bool batch_padded(const s2vt_dims& d) { return batch_pads(d.B); }       // (the train drivers' rule)
static inline s2vt_dims padded_dims(const s2vt_dims& d) { s2vt_dims q = d; q.B = (d.B + 63) / 64 * 64; return q; }
static inline bool dims_ok(const s2vt_dims* d) { return d && d->B > 0 && d->L > 1 && d->F > 0 && d->H > 0 && d->E > 0 && d->V > 0; }
static inline int pad64(int x) { return (x + 63) / 64 * 64; }

// ---- options as the drivers read them (csrc/options.hip)
static inline int pipe_block() { return option(O_PIPE_BLOCK); }      // timesteps per pipeline block; 0 = both layers on the caller's stream
// 0: fp32-input MFMA GEMMs; 3: split precision, 3 bf16 planes (fp32-equivalent); 1: plain bf16 operands (config 3: bf16
// storage, fp32 accumulate) for the batched GEMMs AND the timestep kernels (lstm_bf16.hip)
static inline int gemm_mode() { return option(O_GEMM_MODE); }
// planes per operand of the TRAIN plane drivers: bf16 rows in gemm mode 1, the blocked 3-plane images otherwise
static inline int train_planes() { return gemm_mode() == 1 ? 1 : 3; }
// ... of the decode, beam and score drivers: a greedy decode must stay fp32-equivalent (bit-exact ids) - split precision in every plane mode
static constexpr int DECODE_PLANES = 3;
// plane modes need every k-offset inside a packed operand to be a multiple of 64 (k = time*B + b): B % 64 == 0
static inline bool planes_ok(const s2vt_dims& d) { return gemm_mode() != 0 && d.B % 64 == 0; }
// Recurrence schedule of the train drivers (option "persist"): 1 (default) = one persistent launch per block of timesteps with
// the W_hh slices resident per CU - lstm_persist.hip in the bf16 configuration (both directions), lstm_persist_x3.hip in the
// fp32-equivalent one (forward: option "persist_x3_fwd", default on; BPTT: option "persist_x3_bwd"); 0 = launches per timestep
// everywhere (lstm.hip / lstm_bf16.hip: a card shared with another process, whose kernels could keep a persistent launch from
// becoming resident).  Round 2's exact-fp32 persistent pair (MFMA-bound, slower end to end: docs/history) is gone.
static inline int persist_mode() { return option(O_PERSIST); }
static inline bool persist_on() { return persist_mode() >= 1; }
static inline bool persist_x3_fwd_on() { return option(O_PERSIST_X3_FWD) != 0 && persist_on(); }
// split-precision persistent BPTT (reduce-scatter over the gate columns, lstm_persist_x3.hip): option persist_x3_bwd = 1 wherever
// the shape is supported, 2 (default) only where a workgroup carries ONE 32-row chain (B = 64 at H = 1000).  There a one-layer
// launch holds half of the compute units and the backward's GEMMs run beside it (options corun / bptt_solo, api_train.hip:
// 9.9-10.2 ms per config-2 step; two layers per launch with nothing beside them 10.7-11.0, the launch-per-timestep BPTT on two
// lanes 11.1); with two or more chains per workgroup (B = 128, 256) no unit is left idle and the two-lane launch-per-timestep
// schedule is 6-8 % faster (20.4 vs 19.2 ms, 39.4 vs 36.5)
static inline bool persist_x3_bwd_on(int B, int H) {
    const int m = option(O_PERSIST_X3_BWD);
    if (m == 0 || !persist_on()) return false;
    return m == 1 || lstm_seq_bwd_x3_persist_supported(B, H) == 1;
}
// Which recurrence the whole-path train drivers run for (B, H) under the current modes and options - the ONE statement of it: the
// drivers (api_train.hip) switch on it and s2vt_recurrence_plan reports it (the enum's values are that entry point's).  The plane
// drivers run at B % 64 == 0 in gemm modes 1 and 3; everything else is the fp32-MFMA driver's launches per timestep.  A driver ANDs
// on what only it knows (its workspace provides the images / rings, the bf16 images' k paddings match) and falls back to
// REC_PER_STEP otherwise.  carve_train's predicates are deliberately broader and free of device queries (a workspace-size function
// works without a GPU): wherever this plan selects a persistent kernel, the workspace has been carved for it.
enum RecKind { REC_PER_STEP = 0, REC_BF16_PERSIST = 1, REC_X3_PERSIST = 3 };
struct RecurrencePlan { RecKind fwd, bwd; };
static inline RecurrencePlan train_recurrence_plan(int B, int H) {
    RecurrencePlan pl = {REC_PER_STEP, REC_PER_STEP};
    const int gm = gemm_mode();
    if (pipe_block() <= 0 || gm == 0 || B % 64 != 0) return pl;
    if (gm == 1) {
        if (persist_on() && lstm_seq_fwd_bf16_persist_supported(B, H, pad64(H))) pl.fwd = REC_BF16_PERSIST;
        if (persist_on() && lstm_seq_bwd_bf16_persist_supported(B, H, pad64(4 * H))) pl.bwd = REC_BF16_PERSIST;
    } else if (H <= 1024) {
        if (persist_x3_fwd_on() && lstm_seq_fwd_x3_persist_supported(B, H)) pl.fwd = REC_X3_PERSIST;
        if (persist_x3_bwd_on(B, H) && lstm_seq_bwd_x3_persist_supported(B, H)) pl.bwd = REC_X3_PERSIST;
    }
    return pl;
}
// Which path a decode of d (as the caller hands it over) takes under the current modes and options - the ONE statement of it, as
// train_recurrence_plan is for the train drivers: the driver (api_decode.hip) switches on it, the size / cache queries and the beam
// step (api_beam.hip) read it, s2vt_decode_plan reports it (the enum's values are that entry point's).
//   padded / B      ragged batches run padded to the next multiple of 64: a plain decode from three quarters of option pad_min_batch
//                   on (batch_pads), the encode phase for the beam search (encode_only) always
//   planes          split-precision plane path (gemm modes 1 and 3, B % 64 == 0 after padding): plane GEMMs, gate table, argmax_x3
//   persist_encode  both layers' encode steps and vid_rnn's decode steps as persistent split-precision launches; behind them the token
//   schedule / nh   steps fused, or a step + an argmax launch per step as nh chains over the batch halves; else DEC_PER_STEP: the
//                   two-lane launch-per-timestep loop over all T steps
// device = false leaves out the one device query (does the persistent kernel fit?): carve_decode and the size queries work without a
// GPU that way, and their answer is never narrower than the plan's.
enum DecSchedule { DEC_PER_STEP = 0, DEC_TWO_CHAINS = 1, DEC_FUSED = 2 };
struct DecodePlan { bool padded; int B; bool planes, persist_encode; DecSchedule schedule; int nh; };
static inline DecodePlan decode_plan(const s2vt_dims& d, bool encode_only, bool device = true) {
    DecodePlan pl;
    pl.padded = encode_only ? (gemm_mode() != 0 && d.B % 64 != 0) : batch_pads(d.B, true);
    pl.B = pl.padded ? padded_dims(d).B : d.B;
    pl.planes = gemm_mode() != 0 && pl.B % 64 == 0;
    pl.persist_encode = pl.planes && d.H <= 1024 && pipe_block() > 0 && persist_x3_fwd_on() &&
                        (!device || lstm_seq_fwd_x3_persist_supported(pl.B, d.H));
    pl.schedule = !pl.persist_encode ? DEC_PER_STEP : option(O_DECODE_FUSED) == 1 ? DEC_FUSED : DEC_TWO_CHAINS;
    pl.nh = (pl.persist_encode && pl.B % 128 == 0) ? 2 : 1;      // (chains of the two-chain schedule, whichever is selected)
    return pl;
}
// the recurrence options that decide how a train workspace is carved and which images a forward leaves in it
static inline int persist_bits() { return persist_mode() | (persist_x3_fwd_on() ? 2 : 0) | (option(O_PERSIST_X3_BWD) << 2); }

// ---- two-lane execution (api_runtime.hip): the two LSTM layers as a software pipeline on two streams
struct Lane {
    hipStream_t s;
    float* gws;
    size_t gws_floats;
    float* colsum;
};
int side_stream(hipStream_t caller, hipStream_t* out);
int side_stream_overlaps();               // 1 verified concurrent, 0 no candidate overlapped, -1 before the first pipelined call
int get_event(size_t i, hipEvent_t* out);
int handoff(hipStream_t from, hipStream_t to, size_t ev_index);       // `to` waits for everything enqueued so far on `from`
int lgemm(const Lane& ln, bool ak, bool bk, int M, int N, int K, const float* A, int64_t lda, RowMap am, const float* B, int64_t ldb,
          RowMap bm, float* C, int64_t ldc, RowMap cm, const float* bias, bool acc);
// The frame of one call of a two-lane driver (api_shared.hip): the caller's stream st and the side stream sx (the same stream when
// pipe_block is 0), a Lane on each (la: st, lb: sx) and the running index into the event pool.
struct Lanes {
    hipStream_t st = nullptr, sx = nullptr;
    Lane la{}, lb{};
    size_t ev = 0;
    int open(hipStream_t caller, float* gws_a, float* gws_b, size_t gws_floats, float* colsum_a, float* colsum_b);
    int hand(hipStream_t from, hipStream_t to) { return handoff(from, to, ev++); }      // `to` waits for everything enqueued on `from`
    int record(hipStream_t s, long* idx);     // an event behind everything enqueued on s so far; *idx names it for wait()
    int wait(hipStream_t s, long idx);
};

// ------------------------------------------------------------------ api_shared.hip
// LSTM layer forward over steps [t0, t1) / BPTT over steps t1-1 .. t0 as launches per timestep (time-major buffers)
int seq_fwd(hipStream_t st, int t0, int t1, int B, int H, float* gx_stash, int n_gx, const float* bias, const float* w_hh, float* h_all,
            float* c_all, bool write_stash);
int seq_bwd(hipStream_t st, int T, int t0, int t1, int B, int H, const float* w_hh_t, const float* dh_out, int dh_first,
            const float* c_all, float* stash_dg, float* dc);
int balanced_block(int L, int blk);
std::vector<int> pipe_bounds(int T, int L, int blk);

// packed planes of a k-major operand [rows][k]: 1 plane = bf16 rows, 3 = the blocked 3-plane image (gemm_x3.hip); ld = planes * kpad.
// PB{} (planes 0) is the operand a mode does not provide.
struct PB { unsigned short* p = nullptr; int64_t ld = 0; int kpad = 0; int planes = 0; };
// One k16 record of the blocked 3-plane layout - 16 k columns of a 64-row block: [3 planes][2 halves of 8 columns][64 rows] 16-byte slots
static constexpr size_t K16_HALF_ELEMS = 64 * 8;                        // 512 elements = 1024 bytes
static constexpr size_t K16_REC_ELEMS = 3 * 2 * K16_HALF_ELEMS;         // 3072 elements = 6144 bytes
// element offset of k index k0 (a multiple of 64) inside an operand: row layout (1 plane) k0; blocked 3-plane layout k0/16 records
static inline int64_t koff(const PB& b, int k0) { return b.planes == 3 ? (int64_t)k0 * 192 : (int64_t)k0 * b.planes; }
static inline size_t rows64(size_t r) { return (r + 63) / 64 * 64; }
// a packed operand of `planes` planes carved from c: rows rounded up to 64, k to a multiple of 64
static inline PB take_planes(Carver& c, size_t rows, size_t k, int planes) {
    const int kpad = pad64((int)k);
    return PB{c.take<unsigned short>(rows64(rows) * (size_t)planes * kpad), (int64_t)planes * kpad, kpad, planes};
}
// zero the k16 records from cdiv(H, 16) to the end of the k padding in every 64-row block of the first `rows` rows of a blocked
// 3-plane image (the kernel that writes the image's H valid columns itself leaves them alone); nothing where there are none
int zero_k16_tail(hipStream_t st, const PB& img, int H, size_t rows);
// The plane count of a call is its operands': psplit / pdual write dst's / r's and t's (which must agree), the GEMMs require A's == B's.
int psplit(const Lane& ln, const PB& dst, int r0, const float* in, int64_t ld, RowMap imap, int rows, int cols);
int pdual(const Lane& ln, const float* in, int64_t ld, RowMap imap, int rows, int cols, const PB* r, int r0, const PB* t, int k0,
          float* colpart);
// pdual with no image to write, the 64-row partial column sums alone: the split kernel of `planes` planes (no operand names them)
int pcolpart(const Lane& ln, int planes, const float* in, int64_t ld, RowMap imap, int rows, int cols, float* colpart);
int pgemm(const Lane& ln, int M, int N, int K, const PB& A, int a0, int ka, const PB& B, int b0, int kb, float* C, int64_t ldc,
          RowMap cm, const float* bias, bool acc);
int pgemm_tt(const Lane& ln, int M, int N, int K, const PB& A, int a_row0, const PB& B, int b_row0, float* C, int64_t ldc, RowMap cm,
             const float* bias, bool acc);
int lcolsum_finish(const Lane& ln, const float* partial, int nchunks, int cols, float* out, bool accumulate);   // colsum_finish on ln.s
// every driver's prologue: bsum1 = vid_rnn's b_ih + b_hh, bsum2 = word_rnn's (4H each)
int bias_sums(hipStream_t st, const s2vt_params* p, int H, float* bsum1, float* bsum2);
// fp32-MFMA feature projection on ln: x1 (time-major) = feats·W_f^T + b_f, gx1 = x1·W_ih1^T + bsum1          S2VTModel.py:54, 64-67
int project_features_f32(const Lane& ln, const s2vt_dims& d, const s2vt_params* p, const float* feats, float* x1, float* gx1, const float* bsum1);
// Test support (s2vt_test_lane_delay): inside a LaneDelayScope - the train backward drivers, `caller` = their own stream - every
// launch of the Lane helpers above (and lgemm) on a selected lane (bit 0: the caller's stream, bit 1: the side lane) is preceded
// on its stream by one occupy_kernel workgroup (no LDS) that spins for g_lane_delay_us.  Off (the default): no launch at all.
extern int g_lane_delay_lanes;
extern long long g_lane_delay_us;
struct LaneDelayScope {
    explicit LaneDelayScope(hipStream_t caller);
    ~LaneDelayScope();
};
int lane_delay(hipStream_t s);

int seq_fwd_bf16(hipStream_t st, int t0, int t1, int B, int H, float* gx_stash, int n_gx, const float* bias, const PB& wb, const PB& hb,
                 float* h_all, float* c_all);
int seq_bwd_bf16(hipStream_t st, int T, int t0, int t1, int B, int H, const PB& wt, const float* dh_out, int dh_first,
                 const float* c_all, float* stash_dg, const PB& dgb, float* dc);
SeqBwdX3Args persist_bwd_x3_args(int T, int t0, int t1, int B, int H, int64_t Kp, int64_t Hp, const unsigned short* wtp,
                                 const float* dh_out, int dh_first, const float* c_all, float* stash_dg, float* dc, float* part,
                                 int64_t part_slot, int nslots, unsigned int* sync, int* err);
SeqFwdX3Args persist_fwd_x3_args(int t0, int t1, int B, int H, int T, int64_t Kp, float* gx_stash, int n_gx, const float* bias,
                                 const unsigned short* wp, unsigned short* hp, float* h_all, float* c_all, unsigned int* sync, int* err);
bool persist_fwd_ok(int B, int H, const PB& wb, const PB& hb);
SeqFwdBf16Args persist_fwd_args(int t0, int t1, int B, int H, float* gx_stash, int n_gx, const float* bias, const PB& wb, const PB& hb,
                                float* h_all, float* c_all, unsigned int* sync, int* err);
SeqBwdBf16Args seq_bwd_bf16_args(int T, int t0, int t1, int B, int H, const PB& wt, const PB& dgb, const float* dh_out, int dh_first,
                                 const float* c_all, float* stash_dg, float* dc, unsigned int* sync, int* err);

// ------------------------------------------------------------------ api_train.hip (shared with the fp32 train driver, api_train_f32.hip)
// "gradient group `group` is final behind everything enqueued on s" of the backward that is being enqueued (s2vt_backward_wait_grads:
// 0 = out_linear, 1 = word_rnn + embedding); backward_order_reset() at the start of every backward (s2vt_backward_order)
int grads_ready(int group, hipStream_t s);
void backward_order_reset();
// Every backward entry point opens with one: s2vt_backward_order describes THIS backward, whichever driver it takes, and option
// cu_reserve is off until gradient group 0 is released and off again when the backward is enqueued
struct BackwardScope {
    BackwardScope() { backward_order_reset(); cu_reserve_window(false); }
    ~BackwardScope() { cu_reserve_window(false); }
};

// What a forward left in its workspace, keyed by the workspace: its backward takes the record and refuses a workspace no forward
// filled.  Forwards that never ran a backward (validation, forward-only tools) leave theirs behind: above 64 the OLDEST goes, never
// one of a forward still awaiting its backward.  Host-side only; the mutex because autograd runs the backward on its own thread.
template <typename Rec> class RecordTable {
    struct Slot { Rec rec; unsigned long long seq; };
    std::map<const void*, Slot> slots;
    std::mutex mutex;
    unsigned long long seq = 0;
public:
    void put(const void* ws, const Rec& rec) {
        std::lock_guard<std::mutex> lock(mutex);
        if (slots.size() >= 64 && !slots.count(ws)) {
            auto oldest = slots.begin();
            for (auto it = slots.begin(); it != slots.end(); ++it)
                if (it->second.seq < oldest->second.seq) oldest = it;
            slots.erase(oldest);
        }
        slots[ws] = Slot{rec, ++seq};
    }
    // find + erase
    bool take(const void* ws, Rec* out) {
        std::lock_guard<std::mutex> lock(mutex);
        auto it = slots.find(ws);
        if (it == slots.end()) return false;
        *out = it->second.rec;
        slots.erase(it);
        return true;
    }
    // f(record) under the lock, its answer handed on; false where the workspace has no record
    template <typename F> bool with(const void* ws, F f) {
        std::lock_guard<std::mutex> lock(mutex);
        auto it = slots.find(ws);
        return it != slots.end() && f(it->second.rec);
    }
};

// The buffers of a train workspace that the fp32-MFMA driver works with (time-major images; layer 1 = vid_rnn, 2 = word_rnn): the
// head of TrainWS (api_train.hip, shared with the plane drivers) and of the grouped workspace (api_train_f32.hip)
struct TrainBufs {
    float *bsum1, *bsum2, *x1, *s1, *h1, *c1, *s2, *h2, *c2;
    float *wt1, *wt2, *dh1, *dh2dec, *dx1, *de, *dc1, *dc2, *colsum_a, *colsum_b, *gws_a, *gws_b;
    size_t gws_floats;
    int32_t* tok;
    int* embws;              // embedding_grad scratch (heavy-token list)
    int* err;                // [0] target id out of range, [1] persistent-recurrence hand-off timed out
};

// ------------------------------------------------------------------ api_train_f32.hip
// The launch-per-timestep fp32-MFMA driver (gemm mode 0, and batches the plane drivers do not take): fp32 operands read in place
int train_forward_f32(const s2vt_dims* d, const s2vt_params* p, const float* feats, const int64_t* targets, int64_t targets_ld,
                      float* logits, const TrainBufs& w, hipStream_t st, const float* out_mask);
int train_backward_f32(const s2vt_dims* d, const s2vt_params* p, const float* feats, const float* dlogits, const s2vt_grads* g,
                       float* dfeats, const TrainBufs& w, hipStream_t st, const float* out_mask);

// ------------------------------------------------------------------ sampling arguments (api_decode.hip, api_ops.hip)
// finite and > 0 with a finite reciprocal - what the kernels multiply by: NaN fails the compares, inf gives 0, a subnormal gives inf
static inline bool temperature_ok(float t) { const float r = 1.0f / t; return t > 0.f && r > 0.f && r <= 3.4028234e38f; }
static inline GumbelArgs gumbel_args(float temperature, uint64_t seed, uint32_t step, uint32_t row0, uint32_t rows) {
    return GumbelArgs{1.0f / temperature, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), step, row0, rows};
}

// ------------------------------------------------------------------ api_decode.hip (shared with the beam step)
// What a decode derives from the WEIGHTS alone (plane images of W_f, W_ih1, W_v, W_o and the per-token gate-input table):
// carved from the tail of the call's workspace, or from a caller-kept cache that outlives the call (s2vt_greedy_decode_cached)
struct DecodeConst { PB wf, wih1, wv, wo; float* gtab; unsigned short *xw1, *xw2; PB whh; size_t bytes; };   // xw: W_hh planes [3][4H][Kp]; whh: word_rnn's W_hh, blocked
DecodeConst carve_decode_const(const s2vt_dims& d, void* base);

// ------------------------------------------------------------------ api_beam.hip (shared with the scoring driver, api_score.hip)
// One word_rnn step over R fixed rows: row r reads gate-input row gx_idx[r] of gx (null: row r), its own h_prev / c_prev row and
// its token - tok[r], or with tok == null the packed arg-max word tok_packed[r] of the step before (the rows' sampled decode), or
// with both null tok_const for every row (outside [0, V): token 0, *err raised).  kc != null: plane path - the gate table of the decode cache
// stands for the embedded word and h_t also leaves as blocked planes (h_planes, k padding zeroed by the caller); kc == null: the
// embedding rows against W_e in the kernel's second K segment.
struct RowsStep {
    int R; const int32_t* tok; int* err;
    const unsigned long long* tok_packed; int tok_const;
    const float* gx; const int32_t* gx_idx;
    const float *h_prev, *c_prev; float *h_out, *c_out;
    unsigned short* h_planes; int64_t ldhp;
};
int rows_word_step(hipStream_t st, const s2vt_dims& d, const s2vt_params* p, const DecodeConst* kc, const RowsStep& r);

// ------------------------------------------------------------------ api_score.hip (shared with the rows' sampled decode, api_sample_rows.hip)
// The library-kept scratch of an encode phase, one buffer per (device, stream), grown on demand (a call that grows it synchronises
// the device once); calls on one stream are stream-ordered and share it.
int encode_scratch(hipStream_t st, size_t bytes, void** out);
// The encode phase as launches per timestep on the fp32-input MFMA, once per clip: leaves vid_h, vid_c, word_h, word_c [B][H] after
// the L frames in `states` and vid_rnn's half of word_rnn's gate input (+ biases) of the S decode steps in gx_dec [S][B][4H].
int score_encode_per_step(const s2vt_dims& d, const s2vt_params* p, const float* feats, int S, float* states, float* gx_dec, const Lane& ln);

// ------------------------------------------------------------------ api_sample_rows.hip (shared with the constrained depth step, api_beam.hip)
// The constrained beam's fan-out head (ce.hip, top20_logprob_constrained) behind the host-side argument checks of
// s2vt_constrained_draw, V >= 20 and V >= 20 + t + n_banned + 1; fn names the entry point in the messages.  EDITS `logits`.  With
// every constraint off it runs top20_logprob.
int top20_constrained_checked(const char* fn, hipStream_t st, float* logits, int64_t ld, int64_t rows, int V, const int32_t* hist,
                              int64_t hist_ld, int t, const s2vt_constraints* c, int32_t* top_ix, float* top_lp);

}  // namespace s2vt
