// cti_predict.hip -- the test pass and the TDIUC tallies, kept on the device.
//
// The reference's test pass (src/FFOE/test.py:78-130) copies every batch of logits to the host (`pred[idx:idx+B].copy_(logits)`: one blocking
// device-to-host copy per batch), then takes one host arg-max and one np.float16 per question; its TDIUC metric (src/evaluate_TDIUC.py:26-94) is a
// host loop over Python lists.  Here:
//   predict_rows_kernel     one workgroup per logits row, read once: the arg-max (the order of cti_argmax.h, on the fp32 values), the question id and,
//                           when the buffer keeps logits, the row rounded to float16, written at the buffer's DEVICE-resident cursor
//   predict_advance_kernel  one thread: cursor += rows (stream order puts it behind the first kernel's read of the cursor)
//   type_tally_kernel       one thread per row: table[qtype][gt + 1] += {1, prediction == gt}, 64-bit integer atomics
// The cursor, the sticky overflow word, the capacity and the row length live in a 32-byte state block owned by the caller: an append that does not fit
// writes NOTHING but the overflow word, and every later append is dropped as well.  Nothing here allocates, synchronises, uses a float atomic or takes a
// per-step value as an argument (capturable: a replayed append lands behind the previous one; bitwise reproducible: integer sums in any order).
#include "cti_argmax.h"

namespace cti {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_CHUNK = 4096;                         // floats of a row staged in LDS at a time (16 KiB; n = 3129 is one chunk)

// numpy's astype(np.float16) bit for bit: round to nearest even (v_cvt_f16_f32 under the default mode: overflow to inf from 65520, subnormal halves
// kept, -0 kept); a NaN keeps its sign and the top ten payload bits, as numpy's conversion does (the instruction would quieten a signalling one).
__device__ __forceinline__ unsigned half_bits(float x) {
    unsigned h = __builtin_bit_cast(unsigned short, (_Float16)x);
    if (x != x) {
        const unsigned u = __float_as_uint(x);
        h = ((u >> 16) & 0x8000u) | 0x7c00u | ((u >> 13) & 0x3ffu);
        if ((h & 0x3ffu) == 0) h |= 1u;
    }
    return h;
}

// The input row is only 4-byte aligned and the output row only 2-byte aligned (n = 3129), and the two aligned spans differ from row to row.  So the
// row goes through LDS: 16-byte loads over the aligned middle of the INPUT chunk (split_row), the arg-max taken on the way, then 16-byte stores
// over the aligned middle of the OUTPUT chunk, eight halves each; the <= 7 halves in front of it and behind it are stored one by one.
__global__ __launch_bounds__(PR_THREADS) void predict_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ qid, long long rows, int n,
                                                                  long long* __restrict__ state, long long* __restrict__ answers,
                                                                  long long* __restrict__ qids, unsigned short* __restrict__ half) {
    __shared__ float stage[PR_CHUNK];
    __shared__ float red_v[PR_THREADS / WAVE];
    __shared__ int red_i[PR_THREADS / WAVE];
    const int tid = threadIdx.x;
    const long long cur = state[CTI_PREDICT_CURSOR];
    // the same words in every workgroup, so all of them decide alike (the one store below writes what made them return)
    if (state[CTI_PREDICT_OVERFLOW] != 0 || cur < 0 || cur + rows > state[CTI_PREDICT_CAPACITY] || state[CTI_PREDICT_N] != n) {
        if (blockIdx.x == 0 && tid == 0) state[CTI_PREDICT_OVERFLOW] = 1;
        return;
    }
    const long long r = blockIdx.x, slot = cur + r;
    const float* x = logits + r * n;
    unsigned short* out = half != nullptr ? half + slot * n : nullptr;         // (uniform over the workgroup)

    ArgMax am = {-INFINITY, INT_MAX};
    for (int c0 = 0, m; c0 < n; c0 += m) {
        m = n - c0 < PR_CHUNK ? n - c0 : PR_CHUNK;
        const float* xc = x + c0;
        const RowSplit s = split_row(xc, m);
        const int tail0 = s.head + 4 * s.quads;
        if (tid < s.head) { const float v = xc[tid]; am.take(v, c0 + tid); if (out != nullptr) stage[tid] = v; }
        if (tid < m - tail0) { const float v = xc[tail0 + tid]; am.take(v, c0 + tail0 + tid); if (out != nullptr) stage[tail0 + tid] = v; }
        const float4* x4 = reinterpret_cast<const float4*>(xc + s.head);
        for (int k = tid; k < s.quads; k += PR_THREADS) {
            const float4 q = x4[k];
            const int c = s.head + 4 * k;
            am.take(q.x, c0 + c); am.take(q.y, c0 + c + 1); am.take(q.z, c0 + c + 2); am.take(q.w, c0 + c + 3);
            if (out != nullptr) { stage[c] = q.x; stage[c + 1] = q.y; stage[c + 2] = q.z; stage[c + 3] = q.w; }
        }
        if (out == nullptr) continue;
        __syncthreads();
        unsigned short* oc = out + c0;
        int ohead = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(oc) & 15u)) & 15u) >> 1);
        if (ohead > m) ohead = m;
        const int octs = (m - ohead) >> 3, otail0 = ohead + 8 * octs;
        if (tid < ohead) oc[tid] = (unsigned short)half_bits(stage[tid]);
        if (tid < m - otail0) oc[otail0 + tid] = (unsigned short)half_bits(stage[otail0 + tid]);
        uint4* o4 = reinterpret_cast<uint4*>(oc + ohead);
        for (int k = tid; k < octs; k += PR_THREADS) {
            const float* p = stage + ohead + 8 * k;
            uint4 w;
            w.x = half_bits(p[0]) | (half_bits(p[1]) << 16);
            w.y = half_bits(p[2]) | (half_bits(p[3]) << 16);
            w.z = half_bits(p[4]) | (half_bits(p[5]) << 16);
            w.w = half_bits(p[6]) | (half_bits(p[7]) << 16);
            o4[k] = w;
        }
        __syncthreads();                               // the next chunk overwrites the stage
    }
    am.wave_reduce();
    if ((tid & 63) == 0) { red_v[tid >> 6] = am.v; red_i[tid >> 6] = am.i; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PR_THREADS / WAVE; ++w) am.take(red_v[w], red_i[w]);
        answers[slot] = am.i;                          // < n: every element beats the identity's INT_MAX at worst on the index
        qids[slot] = qid[r];
    }
}

__global__ void predict_advance_kernel(long long* __restrict__ state, long long rows) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state[CTI_PREDICT_OVERFLOW] == 0) state[CTI_PREDICT_CURSOR] += rows;
}

__global__ __launch_bounds__(PR_THREADS) void type_tally_kernel(const long long* __restrict__ pred, const long long* __restrict__ lut, long long n_labels,
                                                                const long long* __restrict__ gt, const long long* __restrict__ qtype, long long rows, int T,
                                                                int K, unsigned long long* __restrict__ table, unsigned long long* __restrict__ invalid) {
    const long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= rows) return;
    long long p = pred[i];
    const long long g = gt[i], t = qtype[i];
    bool ok = t >= 0 && t < T && g >= -1 && g < K;
    if (lut != nullptr) {
        ok = ok && p >= 0 && p < n_labels;
        if (ok) { p = lut[p]; ok = p < K; }            // < 0: the model's answer is not in the key, never a hit
    } else {
        ok = ok && p >= 0 && p < K;
    }
    if (!ok) { atomicAdd(invalid, 1ull); return; }
    unsigned long long* cell = table + ((t * (K + 1)) + g + 1) * 2;
    atomicAdd(cell, 1ull);
    if (g >= 0 && p == g) atomicAdd(cell + 1, 1ull);
}

}  // namespace
}  // namespace cti

using namespace cti;

extern "C" int cti_predict_rows(const float* logits, const int64_t* qid, int64_t rows, int n, int64_t* state, int64_t* answers, int64_t* qids, void* half,
                                void* stream) {
    CTI_REQUIRE_PTR(logits); CTI_REQUIRE_PTR(qid); CTI_REQUIRE_PTR(state); CTI_REQUIRE_PTR(answers); CTI_REQUIRE_PTR(qids);
    CTI_REQUIRE(rows >= 0 && rows <= INT_MAX && n > 0, CTI_E_SHAPE, "cti_predict_rows: rows=%lld n=%d", (long long)rows, n);
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(half) & 1) == 0, CTI_E_ALIGN,
                "cti_predict_rows: the state block is not 8-byte aligned or the float16 table not 2-byte aligned");
    if (rows == 0) return CTI_OK;
    hipLaunchKernelGGL(predict_rows_kernel, dim3((unsigned)rows), dim3(PR_THREADS), 0, as_stream(stream), logits, reinterpret_cast<const long long*>(qid),
                       (long long)rows, n, reinterpret_cast<long long*>(state), reinterpret_cast<long long*>(answers), reinterpret_cast<long long*>(qids),
                       static_cast<unsigned short*>(half));
    return launch_status("cti_predict_rows");
}

extern "C" int cti_predict_advance(int64_t* state, int64_t rows, void* stream) {
    CTI_REQUIRE_PTR(state);
    CTI_REQUIRE(rows >= 0, CTI_E_SHAPE, "cti_predict_advance: rows=%lld", (long long)rows);
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0, CTI_E_ALIGN, "cti_predict_advance: the state block is not 8-byte aligned");
    if (rows == 0) return CTI_OK;
    hipLaunchKernelGGL(predict_advance_kernel, dim3(1), dim3(64), 0, as_stream(stream), reinterpret_cast<long long*>(state), (long long)rows);
    return launch_status("cti_predict_advance");
}

extern "C" int cti_type_tally(const int64_t* pred, const int64_t* lut, int64_t n_labels, const int64_t* gt, const int64_t* qtype, int64_t rows, int T, int K,
                              int64_t* table, int64_t* invalid, void* stream) {
    CTI_REQUIRE_PTR(pred); CTI_REQUIRE_PTR(gt); CTI_REQUIRE_PTR(qtype); CTI_REQUIRE_PTR(table); CTI_REQUIRE_PTR(invalid);
    CTI_REQUIRE(rows >= 0 && rows <= (int64_t)INT_MAX * PR_THREADS && T >= 1 && K >= 1 && K < INT_MAX && (lut == nullptr || n_labels >= 1), CTI_E_SHAPE,
                "cti_type_tally: rows=%lld T=%d K=%d n_labels=%lld", (long long)rows, T, K, (long long)n_labels);
    CTI_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(invalid)) & 7) == 0, CTI_E_ALIGN,
                "cti_type_tally: the table or the invalid counter is not 8-byte aligned");
    if (rows == 0) return CTI_OK;
    hipLaunchKernelGGL(type_tally_kernel, dim3((unsigned)((rows + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, as_stream(stream),
                       reinterpret_cast<const long long*>(pred), reinterpret_cast<const long long*>(lut), (long long)n_labels,
                       reinterpret_cast<const long long*>(gt), reinterpret_cast<const long long*>(qtype), (long long)rows, T, K,
                       reinterpret_cast<unsigned long long*>(table), reinterpret_cast<unsigned long long*>(invalid));
    return launch_status("cti_type_tally");
}
