// cti_argmax.h -- the arg-max order and the row split shared by cti_score.hip and cti_predict.hip (device code only).
//
// The arg-max has to reproduce torch.max(x, 1)[1] on the CPU: the lowest index among equal maxima, a NaN counts as the maximum, the lowest index
// among several NaNs.  wave_max / block_max (fmaxf) drop NaNs and carry no index, so the reduction runs on (value, index) pairs under `beats()`,
// a TOTAL order (value, NaN on top, then the lower index): commutative and associative, so the lane loop, the wave butterfly and the combine of
// the four waves may visit the elements in any order and agree.  Its identity (-inf, INT_MAX) makes a row of -inf come out as index 0.
#pragma once
#include "cti_common.h"

#include <limits.h>
#include <math.h>

namespace cti {

// does (vb, ib) come before (va, ia) in the arg-max order?  ib != ia for distinct elements, so exactly one of beats(a, b) / beats(b, a) holds
__device__ __forceinline__ bool beats(float vb, int ib, float va, int ia) {
    const bool nb = vb != vb, na = va != va;
    if (nb != na) return nb;                       // a NaN beats any number
    if (!nb && vb != va) return vb > va;           // two numbers: the larger (-0 == +0, inf == inf: ties)
    return ib < ia;                                // equal values, or NaN against NaN: the lower index
}

struct ArgMax {
    float v; int i;
    __device__ __forceinline__ void take(float x, int idx) { if (beats(x, idx, v, i)) { v = x; i = idx; } }
    // the butterfly over the 64 lanes of a wave: every lane ends with the wave's winner
    __device__ __forceinline__ void wave_reduce() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            take(ov, oi);
        }
    }
};

// Row r of a (rows, n) array starts 4 n r bytes into it: only 4-byte aligned in general (n = 3129).  The 16-byte loads therefore cover the aligned
// middle [head, head + 4 * quads) of each row; the <= 3 elements in front of it and behind it are read one by one.
struct RowSplit { int head, quads; };
__device__ __forceinline__ RowSplit split_row(const float* row, int n) {
    RowSplit s;
    s.head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);
    if (s.head > n) s.head = n;
    s.quads = (n - s.head) >> 2;
    return s;
}

}  // namespace cti
