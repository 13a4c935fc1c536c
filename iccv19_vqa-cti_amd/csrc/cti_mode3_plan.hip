// cti_mode3_plan.hip -- which row tiles of the mode-3 product a call computes, and the copy that fills the rest (layout and rationale: cti_f16f6.h, "tile plan").
//
// Every image-side operation of TCNet.forward is per object row, so two objects of a sample with bit-identical feature rows have bit-identical blocks
// out[b, v, :, :, :].  The collate function pads every sample to the batch's object count with all-zero rows: all padded objects of a sample share one block
// (relu(bias) pushed through the rank nets: not zero).  The plan keeps the row tiles up to and including ONE padded object per sample -- the representative,
// n_rep = the first object of the TRAILING run of all-zero objects; interior zero objects are simply live -- and mode3_fill_kernel writes the skipped rows,
// ONE contiguous range of out[b], as a periodic copy of the representative's block.  Both kernels read device memory only: no host read, capturable.
#include "cti_common.h"
#include "cti_f16f6.h"

namespace cti {
namespace {

typedef unsigned pu4 __attribute__((ext_vector_type(4)));
typedef float pf4 __attribute__((ext_vector_type(4)));

// One workgroup.  Samples in chunks of 256: thread t finds its sample's n_rep (a backward walk over at most V mask bytes) and live row tiles, an LDS scan gives the
// sample's first live row tile, and the thread writes its sample's entries.  The head goes last.
__global__ __launch_bounds__(256) void mode3_plan_kernel(const uint8_t* __restrict__ mask, unsigned* __restrict__ plan, int nb, int V, int rows_per_obj, int bm, int tiles_m,
                                                         int tiles_n) {
    __shared__ unsigned sc[256];
    __shared__ unsigned filled_s;
    const int t = threadIdx.x;
    if (t == 0) filled_s = 0u;
    pu4* const row_e = reinterpret_cast<pu4*>(plan + M3P_HEAD_WORDS);
    pu4* const smp_e = row_e + (int64_t)nb * tiles_m;
    const unsigned M = (unsigned)V * (unsigned)rows_per_obj;
    unsigned carry = 0u;
    for (int base = 0; base < nb; base += 256) {
        const int b = base + t;
        unsigned L = 0u, nrep = 0u;
        if (b < nb) {
            const uint8_t* m = mask + (int64_t)b * V;
            int n = V;
            while (n > 0 && m[n - 1] != 0) --n;
            nrep = (unsigned)n;
            const unsigned live_objs = (unsigned)(n + 1 < V ? n + 1 : V);
            L = (live_objs * (unsigned)rows_per_obj + (unsigned)bm - 1u) / (unsigned)bm;
        }
        __syncthreads();                                            // (the previous chunk's sc[255] has been read)
        sc[t] = L;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const unsigned x = t >= o ? sc[t - o] : 0u;
            __syncthreads();
            sc[t] += x;
            __syncthreads();
        }
        const unsigned first = carry + sc[t] - L;
        if (b < nb) {
            smp_e[b] = pu4{first, L, nrep, 0u};
            for (unsigned j = 0; j < L; ++j) row_e[first + j] = pu4{(unsigned)b, first, L, nrep};
            const unsigned done = L * (unsigned)bm;
            if (done < M) atomicAdd(&filled_s, M - done);
        }
        carry += sc[255];
    }
    __syncthreads();
    if (t == 0) {
        plan[M3P_W_TILES] = carry * (unsigned)tiles_n;
        plan[M3P_W_ROW_TILES] = carry;
        plan[M3P_W_FILLED_ROWS] = filled_s;
        plan[M3P_W_SAMPLES] = (unsigned)nb;
        plan[4] = plan[5] = plan[6] = plan[7] = 0u;
    }
}

// out[b][off] = out[b][n_rep * obj_floats + off % obj_floats] for off in [live row tiles * tile_floats, sample_floats).  The source block has just been written by the
// product: all workgroups of a sample sit on ONE XCD (ids congruent mod 8 share an L2), so its 350 KB (configs[1]) come out of that L2 and the kernel is a store stream.
// Workgroup (sample, chunk) takes the 4-KiB pieces chunk, chunk + nx, ... of the range: 16-B loads and stores where every offset involved is a multiple of 16 B.
__global__ __launch_bounds__(256) void mode3_fill_kernel(const unsigned* __restrict__ plan, int tiles_m, float* out, int nb, int64_t sample_floats, unsigned obj_floats,
                                                         int64_t tile_floats, int nx, int vec) {
    const int id = blockIdx.x, s = id >> 3;
    const int b = (s / nx) * 8 + (id & 7), chunk = s % nx;
    if (b >= nb) return;
    const pu4 e = reinterpret_cast<const pu4*>(plan + M3P_HEAD_WORDS)[(int64_t)nb * tiles_m + b];
    const int64_t start = (int64_t)e[1] * tile_floats;
    if (start >= sample_floats) return;
    float* const dst = out + (int64_t)b * sample_floats;
    const float* const src = dst + (int64_t)e[2] * obj_floats;
    if (vec) {
        const unsigned step = (unsigned)nx * 1024u;
        int64_t off = start + ((int64_t)chunk * 256 + threadIdx.x) * 4;
        unsigned so = (unsigned)(off % obj_floats);
        for (; off < sample_floats; off += step) {
            *reinterpret_cast<pf4*>(dst + off) = *reinterpret_cast<const pf4*>(src + so);
            so += step;
            if (so >= obj_floats) so %= obj_floats;
        }
    } else {
        const unsigned step = (unsigned)nx * 256u;
        int64_t off = start + (int64_t)chunk * 256 + threadIdx.x;
        unsigned so = (unsigned)(off % obj_floats);
        for (; off < sample_floats; off += step) {
            dst[off] = src[so];
            so += step;
            if (so >= obj_floats) so %= obj_floats;
        }
    }
}

}  // namespace

int mode3_plan(const uint8_t* mask, unsigned* plan, int nb, int V, int rows_per_obj, int bm, int tiles_n, hipStream_t st) {
    if (nb <= 0 || V <= 0 || rows_per_obj <= 0 || bm <= 0 || tiles_n <= 0) return fail(CTI_E_SHAPE, "mode3_plan: nb=%d V=%d rows_per_obj=%d", nb, V, rows_per_obj);
    const int tiles_m = (int)(((int64_t)V * rows_per_obj + bm - 1) / bm);
    hipLaunchKernelGGL(mode3_plan_kernel, dim3(1), dim3(256), 0, st, mask, plan, nb, V, rows_per_obj, bm, tiles_m, tiles_n);
    return launch_status("mode3_plan");
}

int mode3_fill(const unsigned* plan, int tiles_m, float* out, int nb, int64_t sample_floats, int64_t obj_floats, int64_t tile_floats, hipStream_t st) {
    if (nb <= 0 || obj_floats <= 0 || obj_floats >= (1ll << 30) || tile_floats <= 0 || sample_floats % obj_floats != 0)
        return fail(CTI_E_SHAPE, "mode3_fill: nb=%d sample=%lld object=%lld tile=%lld floats", nb, (long long)sample_floats, (long long)obj_floats, (long long)tile_floats);
    if (tile_floats >= sample_floats) return CTI_OK;               // one row tile per sample: always live
    const int vec = ((sample_floats | obj_floats | tile_floats) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    // workgroups per sample: ~64 KiB of the longest possible range each, at most 32 (configs[1]: up to 9.6 MB per sample -> 32 workgroups of 75 pieces)
    const int64_t most = (sample_floats - tile_floats) * 4;
    const int nx = (int)(most >= 32 * 65536ll ? 32 : (most + 65535) / 65536);
    const int64_t grid = ((int64_t)nb + 7) / 8 * 8 * nx;
    if (grid > 0x7fffffffLL) return fail(CTI_E_SHAPE, "mode3_fill: %lld workgroups exceed the grid", (long long)grid);
    hipLaunchKernelGGL(mode3_fill_kernel, dim3((unsigned)grid), dim3(256), 0, st, plan, tiles_m, out, nb, sample_floats, (unsigned)obj_floats, tile_floats, nx, vec);
    return launch_status("mode3_fill");
}

}  // namespace cti
