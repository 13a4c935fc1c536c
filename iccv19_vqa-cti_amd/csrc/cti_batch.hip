// cti_batch.hip -- a training / test batch assembled on the device from tables that stay there.
//
// The reference builds a batch on the host: Dataset.__getitem__ per question (src/FFOE/dataset.py:350-376: two ragged tables sliced through pos_boxes
// and cut to max_boxes, a sparse answer `scatter_`ed into a zeroed row, a float16 teacher row widened), utils.trim_collate (src/utils.py:120-169: every
// image zero-padded to the batch's largest object count), then .to(device) from pageable memory.  Here the tables are resident and a batch is named by
// a DEVICE vector of entry indices:
//   batch_objects_kernel   out[b, 0:n, :] = table[s : s + n, :], out[b, n:Vpad, :] = 0 with [s, t) = pos[image[idx[b]]], n = min(t - s, max_boxes); a pure
//                          copy-and-zero stream, each sample's block cut into BA_CHUNK-byte pieces, one workgroup each
//   batch_targets_kernel   one workgroup per row: the CSR answer of the entry scattered into a row staged (zeroed) in LDS, stored once
//   batch_rows_kernel      out[b, :] = src[idx[b], :] with int32 -> int64 / float16 -> float32 widening, one thread per element
// Guard: an index, an image, a pos pair or a CSR span outside its table is never dereferenced; the sample comes out as zeros and a sticky word of
// the caller's state block is set.  Nothing here allocates, synchronises, uses an atomic or takes a per-step value as an argument: an assemble call
// can be captured and replayed with another `idx`.
#include "cti_common.h"

#include <limits.h>

namespace cti {
namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_CHUNK = 16384;                        // bytes of a sample's destination block per workgroup (64 per thread: four 16-byte stores)
constexpr int BT_CHUNK = 4096;                         // floats of a target row staged in LDS at a time (n = 3129 is one chunk)

__device__ __forceinline__ void flag(long long* state, int word) { state[word] = 1; }

// The entry of sample b, or -1 (never dereference anything through it).  `report`: this thread writes the sticky word.
__device__ __forceinline__ long long entry_of(const long long* __restrict__ idx, long long N, long long b, long long* state, bool report) {
    const long long e = idx[b];
    if (e < 0 || e >= N) {
        if (report) flag(state, CTI_BATCH_BAD_INDEX);
        return -1;
    }
    return e;
}

// element o of a piece: copied below cb, zero from there on
template <typename U>
__device__ __forceinline__ void put_global(char* dst, const char* src, int o, int cb) {
    *reinterpret_cast<U*>(dst + o) = o < cb ? *reinterpret_cast<const U*>(src + o) : (U)0;
}

// Source and destination of a sample are aligned independently: the destination block starts Vpad * row_bytes * b into `out`, the source s * row_bytes
// into the table (24-byte spatial rows: 8-byte aligned only).  Where the two agree mod 16 (2048-wide rows always do) the aligned middle of the
// destination piece is one 16-byte load and one 16-byte store per vector.  Where they differ the piece goes through LDS, as the rows of
// predict_rows_kernel do: 16-byte loads over the aligned middle of the SOURCE span, written into an LDS image laid out like the destination, then
// 16-byte LDS reads and stores over the aligned middle of the DESTINATION.  U is the element (2 or 4 bytes): the unit of every narrow access.
template <typename U>
__global__ __launch_bounds__(BA_THREADS) void batch_objects_kernel(const char* __restrict__ table, long long table_rows, long long row_bytes,
                                                                   const long long* __restrict__ idx, long long N, const long long* __restrict__ image,
                                                                   const long long* __restrict__ pos, long long n_img, int max_boxes, int Vpad, int chunks,
                                                                   char* __restrict__ out, int* __restrict__ counts, unsigned char* __restrict__ mask,
                                                                   long long* __restrict__ state) {
    __shared__ uint4 stage4[BA_CHUNK / 16 + 1];
    constexpr int E = (int)sizeof(U);
    const int tid = threadIdx.x;
    const long long b = blockIdx.x / chunks;
    const int c = (int)(blockIdx.x - b * chunks);
    const bool report = c == 0 && tid == 0;

    // the dependent lookups idx -> image -> pos, the same in every thread of the workgroup
    long long s = 0;
    int n = 0;
    const long long e = entry_of(idx, N, b, state, report);
    if (e >= 0) {
        const long long img = image[e];
        if (img < 0 || img >= n_img) {
            if (report) flag(state, CTI_BATCH_BAD_IMAGE);
        } else {
            const long long s0 = pos[2 * img], t0 = pos[2 * img + 1];
            if (s0 < 0 || t0 < s0 || t0 > table_rows) {
                if (report) flag(state, CTI_BATCH_BAD_POS);
            } else {
                long long k = t0 - s0;
                if (k > max_boxes) k = max_boxes;
                if (k > Vpad) {                        // the host checks pad_to against the table once; a smaller pad never writes past the block
                    if (report) flag(state, CTI_BATCH_BAD_PAD);
                    k = Vpad;
                }
                s = s0;
                n = (int)k;
            }
        }
    }
    if (c == 0) {
        if (counts != nullptr && tid == 0) counts[b] = n;
        if (mask != nullptr)
            for (int r = tid; r < Vpad; r += BA_THREADS) mask[b * Vpad + r] = r >= n ? 1 : 0;
    }

    const long long block = (long long)Vpad * row_bytes, lo = (long long)c * BA_CHUNK;
    const int m = (int)(block - lo < BA_CHUNK ? block - lo : BA_CHUNK);        // bytes of this piece
    long long left = (long long)n * row_bytes - lo;
    const int cb = (int)(left < 0 ? 0 : left > m ? m : left);                  // of which the first cb are copied, the rest is padding
    char* dst = out + b * block + lo;
    const char* src = table + s * row_bytes + lo;                              // read below cb only: inside rows [s, s + n) of the table
    int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    if (head > m) head = m;
    const int vecs = (m - head) >> 4, tail0 = head + 16 * vecs;

    if (cb == 0 || ((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        if (tid * E < head) put_global<U>(dst, src, tid * E, cb);
        if (tail0 + tid * E < m) put_global<U>(dst, src, tail0 + tid * E, cb);
#pragma unroll 4
        for (int k = tid; k < vecs; k += BA_THREADS) {
            const int o = head + 16 * k;
            if (o + 16 <= cb) {
                *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(src + o);
            } else if (o >= cb) {
                *reinterpret_cast<uint4*>(dst + o) = make_uint4(0u, 0u, 0u, 0u);
            } else {                                   // the one vector in which the copy ends
#pragma unroll
                for (int j = 0; j < 16; j += E) put_global<U>(dst, src, o + j, cb);
            }
        }
        return;
    }

    // the LDS image: byte o of the piece at byte pad + o, so that the destination's aligned vectors are aligned in LDS too
    U* stage = reinterpret_cast<U*>(stage4);
    const int pad = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
    int shead = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u);
    if (shead > cb) shead = cb;
    const int svecs = (cb - shead) >> 4, stail0 = shead + 16 * svecs;
    if (tid * E < shead) stage[(pad + tid * E) / E] = *reinterpret_cast<const U*>(src + tid * E);
    if (stail0 + tid * E < cb) stage[(pad + stail0 + tid * E) / E] = *reinterpret_cast<const U*>(src + stail0 + tid * E);
    {
        int z = cb + tid * E;                          // zeros behind the copy, up to the end of the vector in which it ends
        if (tid * E < 16 && z < m) stage[(pad + z) / E] = (U)0;
    }
    for (int k = tid; k < svecs; k += BA_THREADS) {
        const int o = shead + 16 * k;
        const uint4 v = *reinterpret_cast<const uint4*>(src + o);
        U* p = stage + (pad + o) / E;
        if (E == 4) {
            p[0] = (U)v.x; p[1] = (U)v.y; p[2] = (U)v.z; p[3] = (U)v.w;
        } else {
            p[0] = (U)(v.x & 0xffffu); p[1] = (U)(v.x >> 16); p[2] = (U)(v.y & 0xffffu); p[3] = (U)(v.y >> 16);
            p[4] = (U)(v.z & 0xffffu); p[5] = (U)(v.z >> 16); p[6] = (U)(v.w & 0xffffu); p[7] = (U)(v.w >> 16);
        }
    }
    __syncthreads();
    if (tid * E < head) *reinterpret_cast<U*>(dst + tid * E) = tid * E < cb ? stage[(pad + tid * E) / E] : (U)0;
    if (tail0 + tid * E < m) *reinterpret_cast<U*>(dst + tail0 + tid * E) = tail0 + tid * E < cb ? stage[(pad + tail0 + tid * E) / E] : (U)0;
    for (int k = tid; k < vecs; k += BA_THREADS) {
        const int o = head + 16 * k;                   // pad + o is a multiple of 16
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (o <= cb) v = stage4[(pad + o) >> 4];       // o <= cb: copied bytes and the zeros staged behind them
        *reinterpret_cast<uint4*>(dst + o) = v;
    }
}

// target[b, :] = 0, target[b, labels[k]] = scores[k] for k in [off[e], off[e + 1]): the row is zeroed and scattered in LDS (labels of one entry are
// unique, so no two threads write one word) and stored once, 16-byte stores over its aligned middle.
__global__ __launch_bounds__(BA_THREADS) void batch_targets_kernel(const long long* __restrict__ off, const int* __restrict__ labels,
                                                                   const float* __restrict__ scores, long long nnz, const long long* __restrict__ idx,
                                                                   long long N, int n, float* __restrict__ out, long long* __restrict__ state) {
    __shared__ float4 stage4[BT_CHUNK / 4 + 1];
    float* stage = reinterpret_cast<float*>(stage4);
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    long long k0 = 0, k1 = 0;
    const long long e = entry_of(idx, N, b, state, tid == 0);
    if (e >= 0) {
        k0 = off[e]; k1 = off[e + 1];
        if (k0 < 0 || k1 < k0 || k1 > nnz) {
            if (tid == 0) flag(state, CTI_BATCH_BAD_ANSWER);
            k0 = k1 = 0;
        }
    }
    float* row = out + b * n;
    for (int c0 = 0, m; c0 < n; c0 += m) {
        m = n - c0 < BT_CHUNK ? n - c0 : BT_CHUNK;
        float* dst = row + c0;
        const int pad = (int)((reinterpret_cast<uintptr_t>(dst) & 15u) >> 2);       // element j of the chunk at stage[pad + j]
        int head = (4 - pad) & 3;
        if (head > m) head = m;
        const int quads = (m - head) >> 2, tail0 = head + 4 * quads;
        for (int j = tid; j < m + pad; j += BA_THREADS) stage[j] = 0.f;
        __syncthreads();
        for (long long k = k0 + tid; k < k1; k += BA_THREADS) {
            const int l = labels[k];
            if (l < 0 || l >= n) {
                if (c0 == 0) flag(state, CTI_BATCH_BAD_ANSWER);
            } else if (l >= c0 && l < c0 + m) {
                stage[pad + l - c0] = scores[k];
            }
        }
        __syncthreads();
        if (tid < head) dst[tid] = stage[pad + tid];
        if (tail0 + tid < m) dst[tail0 + tid] = stage[pad + tail0 + tid];
        float4* d4 = reinterpret_cast<float4*>(dst + head);
        for (int k = tid; k < quads; k += BA_THREADS) d4[k] = stage4[(pad + head + 4 * k) >> 2];
        __syncthreads();                               // the next chunk zeroes the stage
    }
}

// float16 bits -> the float32 of the same value: the conversion is exact (subnormal halves become normal floats, +-0 and +-inf keep their sign); a NaN
// keeps its sign and its ten payload bits in the top of the fraction, the inverse of half_bits() in cti_predict.hip (v_cvt_f32_f16 alone would quieten a
// signalling one).
__device__ __forceinline__ float widen_half(unsigned short h) {
    if ((h & 0x7c00u) == 0x7c00u && (h & 0x3ffu) != 0)
        return __uint_as_float(((unsigned)(h & 0x8000u) << 16) | 0x7f800000u | ((unsigned)(h & 0x3ffu) << 13));
    return (float)__builtin_bit_cast(_Float16, h);
}
__device__ __forceinline__ long long widen(int x) { return x; }
__device__ __forceinline__ long long widen(long long x) { return x; }
__device__ __forceinline__ float widen(unsigned short x) { return widen_half(x); }
__device__ __forceinline__ float widen(float x) { return x; }

template <typename S, typename D>
__global__ __launch_bounds__(BA_THREADS) void batch_rows_kernel(const S* __restrict__ src, const long long* __restrict__ idx, long long B, long long N, int w,
                                                                D* __restrict__ out, long long* __restrict__ state) {
    const long long i = (long long)blockIdx.x * BA_THREADS + threadIdx.x;
    if (i >= B * w) return;
    const long long b = i / w;
    const int j = (int)(i - b * w);
    const long long e = entry_of(idx, N, b, state, j == 0);
    out[i] = e >= 0 ? widen(src[e * w + j]) : (D)0;
}

}  // namespace
}  // namespace cti

using namespace cti;

#define BATCH_REQUIRE_STATE(name) \
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(idx) & 7) == 0, CTI_E_ALIGN, \
                name ": the state block or idx is not 8-byte aligned")

extern "C" int cti_batch_objects(const void* table, int64_t table_rows, int64_t d, int elem_bytes, const int64_t* idx, int64_t B, int64_t N,
                                 const int64_t* image, const int64_t* pos, int64_t n_img, int max_boxes, int Vpad, void* out, int32_t* counts,
                                 uint8_t* mask, int64_t* state, void* stream) {
    CTI_REQUIRE_PTR(table); CTI_REQUIRE_PTR(idx); CTI_REQUIRE_PTR(image); CTI_REQUIRE_PTR(pos); CTI_REQUIRE_PTR(out); CTI_REQUIRE_PTR(state);
    CTI_REQUIRE(table_rows >= 0 && d >= 1 && (elem_bytes == 2 || elem_bytes == 4) && B >= 0 && N >= 1 && n_img >= 1 && max_boxes >= 0 && Vpad >= 1 &&
                d <= (int64_t)INT_MAX / 4 && (int64_t)Vpad * d * elem_bytes <= ((int64_t)1 << 40), CTI_E_SHAPE,
                "cti_batch_objects: table_rows=%lld d=%lld elem_bytes=%d B=%lld N=%lld n_img=%lld max_boxes=%d Vpad=%d", (long long)table_rows, (long long)d,
                elem_bytes, (long long)B, (long long)N, (long long)n_img, max_boxes, Vpad);
    const int64_t row_bytes = d * elem_bytes, chunks = ((int64_t)Vpad * row_bytes + BA_CHUNK - 1) / BA_CHUNK;
    CTI_REQUIRE(B * chunks <= (int64_t)INT_MAX, CTI_E_SHAPE, "cti_batch_objects: B=%lld samples of %lld pieces exceed one grid", (long long)B, (long long)chunks);
    BATCH_REQUIRE_STATE("cti_batch_objects");
    CTI_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & (uintptr_t)(elem_bytes - 1)) == 0 &&
                ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(pos)) & 7) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0, CTI_E_ALIGN,
                "cti_batch_objects: the table or the batch is not aligned to its element, image / pos not to 8 bytes or counts not to 4");
    if (B == 0) return CTI_OK;
    const dim3 grid((unsigned)(B * chunks)), blk(BA_THREADS);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, blk, 0, as_stream(stream), static_cast<const char*>(table), (long long)table_rows, (long long)row_bytes,
                           reinterpret_cast<const long long*>(idx), (long long)N, reinterpret_cast<const long long*>(image),
                           reinterpret_cast<const long long*>(pos), (long long)n_img, max_boxes, Vpad, (int)chunks, static_cast<char*>(out), counts, mask,
                           reinterpret_cast<long long*>(state));
    };
    if (elem_bytes == 4) go(batch_objects_kernel<unsigned int>);
    else go(batch_objects_kernel<unsigned short>);
    return launch_status("cti_batch_objects");
}

extern "C" int cti_batch_targets(const int64_t* off, const int32_t* labels, const float* scores, int64_t nnz, const int64_t* idx, int64_t B, int64_t N, int n,
                                 float* out, int64_t* state, void* stream) {
    CTI_REQUIRE_PTR(off); CTI_REQUIRE_PTR(idx); CTI_REQUIRE_PTR(out); CTI_REQUIRE_PTR(state);
    CTI_REQUIRE(nnz >= 0 && B >= 0 && B <= INT_MAX && N >= 1 && n >= 1, CTI_E_SHAPE, "cti_batch_targets: nnz=%lld B=%lld N=%lld n=%d", (long long)nnz,
                (long long)B, (long long)N, n);
    if (nnz > 0) { CTI_REQUIRE_PTR(labels); CTI_REQUIRE_PTR(scores); }
    BATCH_REQUIRE_STATE("cti_batch_targets");
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(off) & 7) == 0 &&
                ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, CTI_E_ALIGN,
                "cti_batch_targets: off is not 8-byte aligned or labels / scores / out not 4-byte aligned");
    if (B == 0) return CTI_OK;
    hipLaunchKernelGGL(batch_targets_kernel, dim3((unsigned)B), dim3(BA_THREADS), 0, as_stream(stream), reinterpret_cast<const long long*>(off), labels, scores,
                       (long long)nnz, reinterpret_cast<const long long*>(idx), (long long)N, n, out, reinterpret_cast<long long*>(state));
    return launch_status("cti_batch_targets");
}

extern "C" int cti_batch_rows(const void* src, int mode, const int64_t* idx, int64_t B, int64_t N, int w, void* out, int64_t* state, void* stream) {
    CTI_REQUIRE_PTR(src); CTI_REQUIRE_PTR(idx); CTI_REQUIRE_PTR(out); CTI_REQUIRE_PTR(state);
    CTI_REQUIRE(B >= 0 && N >= 1 && w >= 1 && B * (int64_t)w <= (int64_t)INT_MAX * BA_THREADS, CTI_E_SHAPE, "cti_batch_rows: B=%lld N=%lld w=%d", (long long)B,
                (long long)N, w);
    CTI_REQUIRE(mode >= CTI_BATCH_I32_I64 && mode <= CTI_BATCH_F32_F32, CTI_E_UNSUPPORTED, "cti_batch_rows: mode %d", mode);
    BATCH_REQUIRE_STATE("cti_batch_rows");
    const uintptr_t sa = mode == CTI_BATCH_I64_I64 ? 7 : mode == CTI_BATCH_F16_F32 ? 1 : 3, da = mode <= CTI_BATCH_I64_I64 ? 7 : 3;
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(src) & sa) == 0 && (reinterpret_cast<uintptr_t>(out) & da) == 0, CTI_E_ALIGN,
                "cti_batch_rows: src or out is not aligned to its element");
    if (B == 0) return CTI_OK;
    const dim3 grid((unsigned)((B * w + BA_THREADS - 1) / BA_THREADS)), blk(BA_THREADS);
    const long long* ix = reinterpret_cast<const long long*>(idx);
    long long* st = reinterpret_cast<long long*>(state);
    switch (mode) {
    case CTI_BATCH_I32_I64:
        hipLaunchKernelGGL((batch_rows_kernel<int, long long>), grid, blk, 0, as_stream(stream), static_cast<const int*>(src), ix, (long long)B, (long long)N, w,
                           static_cast<long long*>(out), st);
        break;
    case CTI_BATCH_I64_I64:
        hipLaunchKernelGGL((batch_rows_kernel<long long, long long>), grid, blk, 0, as_stream(stream), static_cast<const long long*>(src), ix, (long long)B,
                           (long long)N, w, static_cast<long long*>(out), st);
        break;
    case CTI_BATCH_F16_F32:
        hipLaunchKernelGGL((batch_rows_kernel<unsigned short, float>), grid, blk, 0, as_stream(stream), static_cast<const unsigned short*>(src), ix, (long long)B,
                           (long long)N, w, static_cast<float*>(out), st);
        break;
    default:
        hipLaunchKernelGGL((batch_rows_kernel<float, float>), grid, blk, 0, as_stream(stream), static_cast<const float*>(src), ix, (long long)B, (long long)N, w,
                           static_cast<float*>(out), st);
        break;
    }
    return launch_status("cti_batch_rows");
}
