// cti_mode3_plan.hip -- which row tiles of the mode-3 product a call computes, and the copy that fills the rest (layout and rationale: cti_f16f6.h, "tile plan").
//
// Every image-side operation of TCNet.forward is per object row, so two objects of a sample with bit-identical feature rows have bit-identical blocks
// out[b, v, :, :, :].  The collate function pads every sample to the batch's object count with all-zero rows: all padded objects of a sample share one block
// (relu(bias) pushed through the rank nets: not zero).  The plan keeps the row tiles up to and including ONE padded object per sample -- the representative,
// n_rep = the first object of the TRAILING run of all-zero objects; interior zero objects are simply live -- and mode3_fill_kernel writes the skipped rows,
// ONE contiguous range of out[b], as a periodic copy of the representative's block: every workgroup loads a chunk of that block once and stores it into all
// the objects of the range (a store stream: the block is read once per sample, not once per object).  Both kernels read device memory only: no host read, capturable.
#include "cti_common.h"
#include "cti_f16f6.h"

namespace cti {
namespace {

typedef unsigned pu4 __attribute__((ext_vector_type(4)));
typedef float pf4 __attribute__((ext_vector_type(4)));

// One workgroup.  Samples in chunks of 256: thread t finds its sample's n_rep and live row tiles, an LDS scan gives the sample's first live row tile, and the thread
// writes its sample's entries.  The head goes last.  n_rep is the mask row's length less its trailing run of non-zero bytes: the row's bytes are fetched 64 at a time,
// from the end, with loads that do not depend on one another (V <= 64, the models' 36 among them: ONE round trip; a further group is read only behind 64 zero
// objects) and gathered into a bit set whose trailing ones are counted.
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
            while (n > 0) {
                const int g = n < 64 ? n : 64;
                unsigned long long zero = 0ull;                     // bit i: object n - 1 - i is all zero
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const unsigned x = i < g ? (unsigned)m[n - 1 - i] : 0u;
                    zero |= (unsigned long long)(x != 0u) << i;
                }
                const int run = ~zero == 0ull ? 64 : __builtin_ctzll(~zero);
                n -= run;
                if (run < g) break;
            }
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

// Pieces a thread holds: a workgroup's chunk of the source block is 256 * FILL_PIECES pieces.  Measured at configs[1] (0.69 GB filled; profiles/r08_mode3_fill.txt):
// 1 / 2 / 4 / 8 pieces 150 / 146 / 150 / 153 us with plain stores, 201 / 200 / 199 / 207 us with non-temporal ones.
constexpr int FILL_PIECES = 2;

// out[b][off] = out[b][n_rep * obj_floats + off % obj_floats] for off in [live row tiles * tile_floats, sample_floats): the rest of one object (the live tiles end
// inside it or at its end) and then whole objects, every one a copy of the representative's block.  Workgroup (sample, chunk) loads ITS chunk of that block once --
// thread t the pieces chunk * 256 * P + j * 256 + t, j < P, all loads in flight together -- and stores it from registers into every object of the range, in the
// first one only at or behind the range's start.  A piece is T: 16 B where every offset involved is a multiple of 16 B, one float otherwise.  A sample with nothing
// to fill costs its workgroups' read of the plan entry.
template <typename T, int P>
__global__ __launch_bounds__(256) void mode3_fill_kernel(const unsigned* __restrict__ plan, int tiles_m, float* out, int nb, int64_t sample_floats, unsigned obj_floats,
                                                         int64_t tile_floats, int nchunks, int n_objs) {
    constexpr unsigned U = sizeof(T) / 4;                           // floats per piece
    const int b = (int)(blockIdx.x / (unsigned)nchunks), chunk = (int)(blockIdx.x - (unsigned)b * (unsigned)nchunks);
    const pu4 e = reinterpret_cast<const pu4*>(plan + M3P_HEAD_WORDS)[(int64_t)nb * tiles_m + b];
    const int64_t start = (int64_t)e[1] * tile_floats;
    if (start >= sample_floats) return;
    float* const dst = out + (int64_t)b * sample_floats;
    const float* const src = dst + (int64_t)e[2] * obj_floats;
    const unsigned off0 = ((unsigned)chunk * (unsigned)(P * 256) + threadIdx.x) * U;      // (< obj_floats + P * 256 * U: obj_floats < 2^30)
    T r[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const unsigned off = off0 + (unsigned)j * 256u * U;
        if (off < obj_floats) r[j] = *reinterpret_cast<const T*>(src + off);
    }
    int k = (int)(start / obj_floats);                              // (> n_rep: the live tiles hold the representative)
    const unsigned first = (unsigned)(start - (int64_t)k * obj_floats);
    float* d = dst + (int64_t)k * obj_floats;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const unsigned off = off0 + (unsigned)j * 256u * U;
        if (off < obj_floats && off >= first) *reinterpret_cast<T*>(d + off) = r[j];
    }
    for (++k, d += obj_floats; k < n_objs; ++k, d += obj_floats) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const unsigned off = off0 + (unsigned)j * 256u * U;
            if (off < obj_floats) *reinterpret_cast<T*>(d + off) = r[j];
        }
    }
}

// one workgroup per (sample, chunk of 256 * P pieces of the source block): configs[1], 16-B pieces, P = 2: 43 chunks of 8 KiB per sample, 11 008 workgroups
template <typename T, int P>
int fill_launch(const unsigned* plan, int tiles_m, float* out, int nb, int64_t sample_floats, int64_t obj_floats, int64_t tile_floats, hipStream_t st) {
    const int64_t pieces = obj_floats / (int64_t)(sizeof(T) / 4);
    const int nchunks = (int)((pieces + P * 256 - 1) / (P * 256));
    const int64_t grid = (int64_t)nb * nchunks;
    if (grid > 0x7fffffffLL) return fail(CTI_E_SHAPE, "mode3_fill: %lld workgroups exceed the grid", (long long)grid);
    hipLaunchKernelGGL((mode3_fill_kernel<T, P>), dim3((unsigned)grid), dim3(256), 0, st, plan, tiles_m, out, nb, sample_floats, (unsigned)obj_floats, tile_floats, nchunks,
                       (int)(sample_floats / obj_floats));
    return launch_status("mode3_fill");
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
    return vec ? fill_launch<pf4, FILL_PIECES>(plan, tiles_m, out, nb, sample_floats, obj_floats, tile_floats, st)
               : fill_launch<float, FILL_PIECES>(plan, tiles_m, out, nb, sample_floats, obj_floats, tile_floats, st);
}

}  // namespace cti
