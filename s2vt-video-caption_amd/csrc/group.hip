// Row-group helpers of the K-captions-per-clip train driver (api_train_f32.hip): the caption rows r = g * K + k of a clip (or of
// a (timestep, clip) pair of a time-major image: (t * B + b) * K + k) against the clip's one row g.
//   group_sum_rows     out[g] = in[g*K] + in[g*K+1] + ... + in[g*K+K-1]: the gradients arriving at the shared encode
//   group_expand_rows  out[g*K+k] (+)= in[g]: the clip's state / gate-input half handed to its K caption rows
//   group_tokens       the captions [B][K][S] (any strides) as time-major int32 tokens over the rows r = b * K + k
// All three are memory-bound: one thread per 16 bytes of a clip row where both row images are 16-byte aligned (row starts and
// strides), one per float otherwise and for the columns past the last whole float4; grid-stride over a capped grid.
#include "common.h"
#include "kernels.h"

namespace s2vt {

static inline bool rows_aligned16(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

// A row of `cols` floats as nv4 float4 units followed by cols - 4 * nv4 single floats (nv4 = 0: no vector access at all)
struct RowUnits { int nv4, upr; };
static inline RowUnits row_units(int cols, bool vec) {
    const int nv4 = vec ? cols / 4 : 0;
    return RowUnits{nv4, nv4 + (cols - 4 * nv4)};
}
static inline unsigned capped_grid(int64_t n) {
    const int64_t blocks = (n + 255) / 256;
    return (unsigned)(blocks < 2048 ? blocks : 2048);
}

// fp32 adds in the order k = 0, 1, ..., K-1 and nothing else: no atomics, one thread owns an output element - bit-reproducible.
// (four loads in flight per round; the adds stay one chain in k order)
template <typename V>
__device__ __forceinline__ V group_sum_one(const float* src, int64_t ld, int K) {
    V acc = *reinterpret_cast<const V*>(src);
    int k = 1;
    for (; k + 3 < K; k += 4) {
        const V x0 = *reinterpret_cast<const V*>(src + (int64_t)k * ld);
        const V x1 = *reinterpret_cast<const V*>(src + (int64_t)(k + 1) * ld);
        const V x2 = *reinterpret_cast<const V*>(src + (int64_t)(k + 2) * ld);
        const V x3 = *reinterpret_cast<const V*>(src + (int64_t)(k + 3) * ld);
        acc = acc + x0;
        acc = acc + x1;
        acc = acc + x2;
        acc = acc + x3;
    }
    for (; k < K; ++k) acc = acc + *reinterpret_cast<const V*>(src + (int64_t)k * ld);
    return acc;
}
__global__ __launch_bounds__(256) void group_sum_rows_kernel(const float* __restrict__ in, int64_t ld_in, float* __restrict__ out,
                                                             int64_t ld_out, int64_t groups, int K, int nv4, int upr) {
    const int64_t n = groups * upr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t g = i / upr;
        const int u = (int)(i % upr);
        const float* src = in + g * K * ld_in;
        float* dst = out + g * ld_out;
        if (u < nv4) *reinterpret_cast<f32x4*>(dst + 4 * u) = group_sum_one<f32x4>(src + 4 * u, ld_in, K);
        else dst[3 * nv4 + u] = group_sum_one<float>(src + 3 * nv4 + u, ld_in, K);      // column 4 * nv4 + (u - nv4)
    }
}
int group_sum_rows(hipStream_t s, const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t groups, int K, int cols) {
    if (groups <= 0 || cols <= 0) return 0;
    S2VT_REQUIRE(in && out && K >= 1 && ld_in >= cols && ld_out >= cols, "group_sum_rows: bad arguments");
    const RowUnits ru = row_units(cols, rows_aligned16(in, ld_in) && rows_aligned16(out, ld_out));
    hipLaunchKernelGGL(group_sum_rows_kernel, dim3(capped_grid(groups * ru.upr)), dim3(256), 0, s, in, ld_in, out, ld_out, groups, K,
                       ru.nv4, ru.upr);
    S2VT_LAUNCH_CHECK("group_sum_rows_kernel");
    return 0;
}

template <typename V>
__device__ __forceinline__ void group_expand_one(const float* src, float* dst, int64_t ld, int K, int accumulate) {
    const V v = *reinterpret_cast<const V*>(src);
    for (int k = 0; k < K; ++k) {
        V* o = reinterpret_cast<V*>(dst + (int64_t)k * ld);
        *o = accumulate ? *o + v : v;
    }
}
__global__ __launch_bounds__(256) void group_expand_rows_kernel(const float* __restrict__ in, int64_t ld_in, float* __restrict__ out,
                                                                int64_t ld_out, int64_t groups, int K, int nv4, int upr, int accumulate) {
    const int64_t n = groups * upr;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t g = i / upr;
        const int u = (int)(i % upr);
        const float* src = in + g * ld_in;
        float* dst = out + g * K * ld_out;
        if (u < nv4) group_expand_one<f32x4>(src + 4 * u, dst + 4 * u, ld_out, K, accumulate);
        else group_expand_one<float>(src + 3 * nv4 + u, dst + 3 * nv4 + u, ld_out, K, accumulate);
    }
}
int group_expand_rows(hipStream_t s, const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t groups, int K, int cols,
                      bool accumulate) {
    if (groups <= 0 || cols <= 0) return 0;
    S2VT_REQUIRE(in && out && K >= 1 && ld_in >= cols && ld_out >= cols, "group_expand_rows: bad arguments");
    const RowUnits ru = row_units(cols, rows_aligned16(in, ld_in) && rows_aligned16(out, ld_out));
    hipLaunchKernelGGL(group_expand_rows_kernel, dim3(capped_grid(groups * ru.upr)), dim3(256), 0, s, in, ld_in, out, ld_out, groups, K,
                       ru.nv4, ru.upr, accumulate ? 1 : 0);
    S2VT_LAUNCH_CHECK("group_expand_rows_kernel");
    return 0;
}

// caps[b][k][j] at b * stride_b + k * stride_k + j (either stride may be 0: a broadcast view) -> tok[j * R + b * K + k], R = B * K;
// an id outside [0, V) is clamped and flagged, as targets_to_time_major does it
__global__ __launch_bounds__(256) void group_tokens_kernel(const int64_t* caps, int64_t stride_b, int64_t stride_k, int R, int K, int S,
                                                           int V, int32_t* tok, int* err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)S * R) return;
    const int j = (int)(i / R), r = (int)(i % R);
    int64_t c = caps[(int64_t)(r / K) * stride_b + (int64_t)(r % K) * stride_k + j];
    if (c < 0 || c >= V) {
        if (err) atomicExch(err, 1);
        c = c < 0 ? 0 : V - 1;
    }
    tok[i] = (int32_t)c;
}
int group_tokens(hipStream_t s, const int64_t* caps, int64_t stride_b, int64_t stride_k, int B, int K, int S, int V, int32_t* tok,
                 int* err_flag) {
    S2VT_REQUIRE(caps && tok && B > 0 && K > 0 && S > 0 && V > 0 && stride_b >= 0 && stride_k >= 0, "group_tokens: bad arguments");
    const int64_t n = (int64_t)S * B * K;
    hipLaunchKernelGGL(group_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, caps, stride_b, stride_k, B * K, K, S, V,
                       tok, err_flag);
    S2VT_LAUNCH_CHECK("group_tokens_kernel");
    return 0;
}

}  // namespace s2vt
