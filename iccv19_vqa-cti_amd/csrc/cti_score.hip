// cti_score.hip -- answer scoring and the device-side meter of the training / evaluation loops.
//
// The reference scores a batch in torch: FFOE (src/FFOE/trainer.py:296-303) max -> zeros(B, N) -> scatter_ -> mul -> sum, MC
// (src/MC/trainer.py:292-300) softmax -> one max per group of 4 -> stack -> gather, and its loops add `loss.item()` and `grad_norm` on the host
// once per update (src/FFOE/train.py:83-86).  Here:
//   score_rows_kernel   one workgroup per row: arg-max of the logits row + the label under it + the row's largest label, each array read once
//   score_mc_kernel     one thread per group of 4 rows: the fp32 class-0 softmax probability of each, the first maximum of the four
//   meter_scores_kernel ONE workgroup: the batch's scores / upper bounds summed in double in a fixed order, added to the caller's 64-byte block
//   meter_scalar_kernel one thread: block.slot += a device-resident fp32 scalar (a loss, a gradient norm)
// The arg-max has to reproduce torch.max(x, 1)[1] on the CPU (ties, NaNs): it is a reduction over (value, index) pairs under `beats()` of cti_argmax.h,
// which cti_predict.hip shares, together with the split of a 4-byte aligned row into 16-byte loads.
// Nothing here allocates, synchronises, uses a float atomic or takes a per-step value as an argument (capturable, bitwise reproducible).
#include "cti_argmax.h"

namespace cti {
namespace {

constexpr int SC_THREADS = 256;

__global__ __launch_bounds__(SC_THREADS) void score_rows_kernel(const float* __restrict__ logits, const float* __restrict__ labels, int n,
                                                                long long* __restrict__ pred, float* __restrict__ score, float* __restrict__ upper,
                                                                float* __restrict__ dense) {
    __shared__ float red_v[SC_THREADS / WAVE];
    __shared__ int red_i[SC_THREADS / WAVE];
    __shared__ float red_u[SC_THREADS / WAVE];
    __shared__ int best_s;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* x = logits + r * n;
    const float* y = labels + r * n;

    ArgMax am = {-INFINITY, INT_MAX};
    {
        const RowSplit s = split_row(x, n);
        const int tail0 = s.head + 4 * s.quads;
        if (tid < s.head) am.take(x[tid], tid);
        if (tid < n - tail0) am.take(x[tail0 + tid], tail0 + tid);
        const float4* x4 = reinterpret_cast<const float4*>(x + s.head);
        for (int k = tid; k < s.quads; k += SC_THREADS) {
            const float4 q = x4[k];
            const int c = s.head + 4 * k;
            am.take(q.x, c); am.take(q.y, c + 1); am.take(q.z, c + 2); am.take(q.w, c + 3);
        }
    }
    float u = -INFINITY;
    {
        const RowSplit s = split_row(y, n);
        const int tail0 = s.head + 4 * s.quads;
        if (tid < s.head) u = fmaxf(u, y[tid]);
        if (tid < n - tail0) u = fmaxf(u, y[tail0 + tid]);
        const float4* y4 = reinterpret_cast<const float4*>(y + s.head);
        for (int k = tid; k < s.quads; k += SC_THREADS) {
            const float4 q = y4[k];
            u = fmaxf(fmaxf(u, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                 // the same order between lanes ...
        const float ov = __shfl_xor(am.v, o, 64);
        const int oi = __shfl_xor(am.i, o, 64);
        am.take(ov, oi);
    }
    u = wave_max(u);
    if ((tid & 63) == 0) { red_v[tid >> 6] = am.v; red_i[tid >> 6] = am.i; red_u[tid >> 6] = u; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SC_THREADS / WAVE; ++w) {  // ... and between waves
            am.take(red_v[w], red_i[w]);
            u = fmaxf(u, red_u[w]);
        }
        best_s = am.i;                                 // < n: every element beats the identity's INT_MAX at worst on the index
        pred[r] = am.i;
        score[r] = y[am.i];
        upper[r] = u;
    }
    if (dense == nullptr) return;                      // (uniform over the workgroup)
    __syncthreads();
    const int best = best_s;
    float* d = dense + r * n;
    for (int c = tid; c < n; c += SC_THREADS) d[c] = (c == best ? 1.f : 0.f) * y[c];     // the reference's `one_hots * labels`
}

__global__ __launch_bounds__(SC_THREADS) void score_mc_kernel(const float* __restrict__ logits, const float* __restrict__ labels, int64_t ld, int64_t rows,
                                                              long long* __restrict__ pred, float* __restrict__ score, float* __restrict__ upper) {
    const int64_t t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (t < rows) upper[t] = labels[t * ld];
    if (t >= rows / 4) return;
    ArgMax am = {-INFINITY, INT_MAX};
    for (int i = 0; i < 4; ++i) {
        const float x0 = logits[(4 * t + i) * 2], x1 = logits[(4 * t + i) * 2 + 1];
        // torch.softmax's own formula in fp32: the comparison must see its saturation to 1.0f / 0.0f (ties the reference breaks by position).
        // (fmaxf skips a NaN, but the NaN then enters through its own exponential: p0 is NaN whenever x0 or x1 is, as in the reference)
        const float m = fmaxf(x0, x1);
        const float e0 = expf(x0 - m), e1 = expf(x1 - m);
        am.take(e0 / (e0 + e1), i);
    }
    const int64_t p = 4 * t + am.i;
    pred[t] = p;
    score[t] = labels[p * ld];
}

__global__ __launch_bounds__(SC_THREADS) void meter_scores_kernel(double* __restrict__ block, const float* __restrict__ score, int64_t n_score,
                                                                  const float* __restrict__ upper, int64_t n_upper, long long samples) {
    __shared__ double red_s[SC_THREADS], red_u[SC_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0, u = 0.0;
    for (int64_t i = tid; i < n_score; i += SC_THREADS) s += (double)score[i];
    for (int64_t i = tid; i < n_upper; i += SC_THREADS) u += (double)upper[i];
    red_s[tid] = s; red_u[tid] = u;
    __syncthreads();
    for (int o = SC_THREADS / 2; o > 0; o >>= 1) {     // a fixed tree: thread t adds the partial of thread t + o
        if (tid < o) { red_s[tid] += red_s[tid + o]; red_u[tid] += red_u[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        block[CTI_METER_SCORE] += red_s[0];
        block[CTI_METER_UPPER] += red_u[0];
        reinterpret_cast<long long*>(block)[4] += samples;
    }
}

__global__ void meter_scalar_kernel(double* __restrict__ block, int slot, const float* __restrict__ value) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    block[slot] += (double)value[0];
    if (slot == CTI_METER_LOSS) reinterpret_cast<long long*>(block)[5] += 1;
}

}  // namespace
}  // namespace cti

using namespace cti;

extern "C" int cti_score_rows(const float* logits, const float* labels, int64_t rows, int n, int64_t* pred, float* score, float* upper, float* dense,
                              void* stream) {
    CTI_REQUIRE_PTR(logits); CTI_REQUIRE_PTR(labels); CTI_REQUIRE_PTR(pred); CTI_REQUIRE_PTR(score); CTI_REQUIRE_PTR(upper);
    CTI_REQUIRE(rows >= 0 && rows <= INT_MAX && n > 0, CTI_E_SHAPE, "cti_score_rows: rows=%lld n=%d", (long long)rows, n);
    if (rows == 0) return CTI_OK;
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)rows), dim3(SC_THREADS), 0, as_stream(stream), logits, labels, n,
                       reinterpret_cast<long long*>(pred), score, upper, dense);
    return launch_status("cti_score_rows");
}

extern "C" int cti_score_mc(const float* logits, const float* labels, int64_t ld_labels, int64_t rows, int64_t* pred, float* score, float* upper,
                            void* stream) {
    CTI_REQUIRE_PTR(logits); CTI_REQUIRE_PTR(labels); CTI_REQUIRE_PTR(upper);
    CTI_REQUIRE(rows >= 0 && rows <= (int64_t)INT_MAX * SC_THREADS && ld_labels >= 1, CTI_E_SHAPE, "cti_score_mc: rows=%lld ld_labels=%lld", (long long)rows,
                (long long)ld_labels);
    if (rows >= 4) { CTI_REQUIRE_PTR(pred); CTI_REQUIRE_PTR(score); }
    if (rows == 0) return CTI_OK;
    hipLaunchKernelGGL(score_mc_kernel, dim3((unsigned)((rows + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, as_stream(stream), logits, labels,
                       ld_labels, rows, reinterpret_cast<long long*>(pred), score, upper);
    return launch_status("cti_score_mc");
}

extern "C" int cti_meter_add_scores(void* block, const float* score, int64_t n_score, const float* upper, int64_t n_upper, int64_t samples, void* stream) {
    CTI_REQUIRE_PTR(block);
    CTI_REQUIRE(n_score >= 0 && n_upper >= 0 && samples >= 0, CTI_E_SHAPE, "cti_meter_add_scores: n_score=%lld n_upper=%lld samples=%lld", (long long)n_score,
                (long long)n_upper, (long long)samples);
    if (n_score > 0) CTI_REQUIRE_PTR(score);
    if (n_upper > 0) CTI_REQUIRE_PTR(upper);
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(block) & 7) == 0, CTI_E_ALIGN, "cti_meter_add_scores: the meter block is not 8-byte aligned");
    hipLaunchKernelGGL(meter_scores_kernel, dim3(1), dim3(SC_THREADS), 0, as_stream(stream), static_cast<double*>(block), score, n_score, upper, n_upper,
                       (long long)samples);
    return launch_status("cti_meter_add_scores");
}

extern "C" int cti_meter_add_scalar(void* block, int slot, const float* value, void* stream) {
    CTI_REQUIRE_PTR(block); CTI_REQUIRE_PTR(value);
    CTI_REQUIRE(slot >= CTI_METER_SCORE && slot <= CTI_METER_GRAD_NORM, CTI_E_SHAPE, "cti_meter_add_scalar: slot %d is not one of the four sums (0 .. 3)", slot);
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(block) & 7) == 0, CTI_E_ALIGN, "cti_meter_add_scalar: the meter block is not 8-byte aligned");
    hipLaunchKernelGGL(meter_scalar_kernel, dim3(1), dim3(64), 0, as_stream(stream), static_cast<double*>(block), slot, value);
    return launch_status("cti_meter_add_scalar");
}
