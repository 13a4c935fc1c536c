// cti_gemm_f16f6.hip -- fp32-grade NT GEMM on f16 + block-scaled fp6 matrix-core products (format and rationale: cti_f16f6.h).
//
// Per 32-wide K block and 32x32 output tile: two v_mfma_f32_32x32x16_f16 (hi x hi) and ONE v_mfma_scale_f32_32x32x64_f8f6f4
// whose lane halves carry the two cross terms (lanes 0-31: fp6(A_hi) x fp6(B_lo), lanes 32-63: fp6(A_lo) x fp6(B_hi)), all into
// the same fp32 accumulator: 96 MFMA cycles per block and tile against 192 for the three-bf16-product form.  The fp6 codes of the
// hi parts are not stored: a lane converts the 16 f16 values it has just read (v_cvt_scalef32_pk32_fp6_f16) and trades halves with
// its SIMD-half partner (v_permlane32_swap).
//
// KERNEL.  256 x 192 tile, 8 waves (4 x 2, each 64 x 96 = 2 x 3 MFMA tiles, 96 accumulator registers), a 4-slot LDS ring of 32-deep
// K blocks (40 KiB per slot = exactly 40 LDS-DMA pieces of 1 KiB, five per wave: f16 rows of 64 B, lo-code rows of 24 B, scale
// bytes), counted vmcnt and one raw s_barrier per block, persistent XCD-aware tile walk.  A workgroup's tiles are ONE stream of K
// blocks: the ring is refilled across tile boundaries and the epilogue's stores overlap with loads in flight.  LDS images: the f16
// rows are XOR-swizzled at the SOURCE (16-B chunk c of row r lands at chunk c ^ ((r >> 2) & 3)): conflict-free ds_read_b128
// fragments; the fp6 rows are linear (24-B pitch, each lane half reads 12 B as one 8-B and one 4-B load: conflict-free).
// What bounds it (round-2 measurements): a wave issues at most one instruction per four cycles and needs ~250 of them per
// K block beside its 18 MFMAs; with two waves per SIMD the matrix pipe is busy ~45 % of the time.  Removing any one of DMA, MFMAs,
// conversions or stores takes 10-18 % off; no single phase dominates.
#include "cti_common.h"
#include "cti_f16f6.h"
#include <cstdlib>

namespace cti {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));   // 8-B LDS loads.  NOT HIP's uint2 / uint8_t: loads through struct or char types make hipcc
                                                              // drain vmcnt(0) -- every LDS-DMA in flight -- in front of them (may-alias with the DMA's LDS store)

__device__ __forceinline__ void dma16(const char* src, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ---- encoder: fp32 rows -> f16f6 planes.  A wave stages a 64-row x 32-column tile through a private LDS patch: the global loads are
// coalesced (8 lanes x 16 B = one row's block, 8 rows per instruction), then every lane encodes one row from LDS (pitch 36 floats:
// conflict-free 16-B row reads) with the streaming encoder the GEMM epilogues use.
__global__ __launch_bounds__(256) void quantize_f16f6_kernel(const float* __restrict__ x, int64_t ld, int64_t rows, int K, F6Planes p,
                                                              const float* __restrict__ row_scale, int scale_div) {
    __shared__ __attribute__((aligned(16))) float patch[4][64 * 36];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // the K block is the FAST grid axis: workgroups dispatched together read adjacent 128-B pieces of the same 256 rows (whole DRAM pages and
    // shared cache lines when the row length is not a multiple of 128 B) instead of one piece of every row per pass over the matrix
    const int kb = blockIdx.x, k0 = kb * 32;
    const int64_t row0 = (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * 4 + wid) * 64;
    if (row0 >= rows) return;
    float* st = patch[wid];
    const int c4 = lane & 7, rsub = lane >> 3;
    const bool vec = (k0 + 32 <= K) && ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int rr = it * 8 + rsub;
        const int64_t row = row0 + rr;
        f6_f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < rows) {
            const float* src = x + row * ld + k0 + c4 * 4;
            if (vec) v = *reinterpret_cast<const f6_f32x4*>(src);
            else {
#pragma unroll
                for (int u = 0; u < 4; ++u) if (k0 + c4 * 4 + u < K) v[u] = src[u];
            }
            if (row_scale) v *= row_scale[row / scale_div];
        }
        *reinterpret_cast<f6_f32x4*>(st + rr * 36 + c4 * 4) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // same wave writes and reads its patch: in-order LDS, no barrier
    const int64_t row = row0 + lane;
    if (row < rows) f6_encode_row32_lds(st + lane * 36, p, f6_prow(p, row), kb);
}

// ---- the same encoder for a DENSE matrix (ld == K) of short rows: a workgroup takes QR CONSECUTIVE rows -- one contiguous run of QR x K floats -- into LDS
// by LDS-DMA (whole 1-KiB pieces, no straddled cache lines, no over-fetch: the kernel above reads a 128-B piece of every row per block, and rows of
// 1 200 B start at 48 r mod 128), then wave w encodes K blocks w, w + 4, ... with lane = row.  Row pitch K floats: for K = 300 a 16-lane group's 16-B reads
// fall on 16 distinct 4-bank groups (44 r mod 64).  Same planes, bit for bit.  configs[1]'s `a` (801 024 x 300): 0.53 -> see profiles/r04_quantize.txt.
constexpr int QR = 48;              // rows per workgroup: 48 x 1 200 B + the four waves' output images = 75 KB: two workgroups per CU
__global__ __launch_bounds__(256) void quantize_rows_f16f6_kernel(const float* __restrict__ x, int64_t rows, int K, F6Planes p, const float* __restrict__ row_scale,
                                                                   int scale_div) {
    extern __shared__ __attribute__((aligned(16))) char qsm[];
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row0 = (int64_t)blockIdx.x * QR;
    const int nrows = (int)(rows - row0 < QR ? rows - row0 : QR);
    const int nbytes = nrows * K * 4;                                   // valid bytes of this workgroup's run (a multiple of 16: K % 4 == 0)
    const int npieces = (QR * K * 4 + 1023) / 1024;
    const char* src0 = reinterpret_cast<const char*>(x + row0 * K);
    for (int pc = wid; pc < npieces; pc += 4) {
        int off = pc * 1024 + lane * 16;
        if (off > nbytes - 16) off = nbytes - 16;                       // a short last workgroup / the last piece's tail: re-read valid bytes (rows beyond nrows are not encoded)
        dma16(src0 + off, qsm + pc * 1024);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int Kb = (K + 31) / 32;
    const int64_t row = row0 + lane;
    const float rs = (row_scale && lane < nrows) ? row_scale[row / scale_div] : 1.f;
    const int64_t prow = f6_prow(p, lane < nrows ? row : row0);
    const float* rsrc = reinterpret_cast<const float*>(qsm) + lane * K;
    // Every (row, block) item is encoded in registers into a wave-private LDS image of the three plane runs it belongs to -- 64 rows of one K block are
    // 4 KiB of H, 1.5 KiB of FL and 128 B of S, each CONTIGUOUS in its plane when the 64 plane rows are consecutive -- and leaves as whole 16-B pieces of
    // consecutive addresses (the direct form's stores are 16-B / 8-B / 2-B pieces 64 / 24 / 2 B apart across the lanes).
    __shared__ __attribute__((aligned(16))) char stage[4][QR * 64 + QR * 24 + 128];
    char* const sH = stage[wid]; char* const sF = sH + QR * 64; char* const sS = sF + QR * 24;
    const int64_t prow_first = f6_prow(p, row0);
    const bool run_ok = f6_prow(p, row0 + nrows - 1) - prow_first == nrows - 1 && (prow_first & 7) == 0;     // consecutive plane rows, 16-B aligned runs
    for (int kb = wid; kb < Kb; kb += 4) {
        const int nv = K - kb * 32;
        float xv[32];
        if (lane < nrows) {
#pragma unroll
            for (int q4 = 0; q4 < 8; ++q4) {
                f6_f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (q4 * 4 < nv) v = *reinterpret_cast<const f6_f32x4*>(rsrc + kb * 32 + q4 * 4);       // K % 4 == 0: a 16-B piece is all valid or all tail
                v *= rs;
                xv[q4 * 4] = v[0]; xv[q4 * 4 + 1] = v[1]; xv[q4 * 4 + 2] = v[2]; xv[q4 * 4 + 3] = v[3];
            }
            const int64_t o = (int64_t)kb * p.rows_alloc + prow;
            if (run_ok) f6_encode_row32_regs(xv, -__builtin_huge_valf(), sH + lane * 64, sF + lane * 24, sS + lane * 2);
            else f6_encode_row32_regs(xv, -__builtin_huge_valf(), reinterpret_cast<char*>(p.H) + o * 64, reinterpret_cast<char*>(p.FL) + o * 24,
                                      reinterpret_cast<char*>(p.S) + ((int64_t)kb * p.rows_allocS + prow) * 2);
        }
        if (!run_ok) continue;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the wave's own image: in-order LDS, no barrier
        typedef unsigned qu4 __attribute__((ext_vector_type(4)));
        char* gH = reinterpret_cast<char*>(p.H) + ((int64_t)kb * p.rows_alloc + prow_first) * 64;
        char* gF = reinterpret_cast<char*>(p.FL) + ((int64_t)kb * p.rows_alloc + prow_first) * 24;
        char* gS = reinterpret_cast<char*>(p.S) + ((int64_t)kb * p.rows_allocS + prow_first) * 2;
        const int nH = nrows * 64, nF = nrows * 24, nS = nrows * 2;      // bytes of the three runs (nrows < 64 only in the last workgroup)
#pragma unroll
        for (int u = 0; u < (QR * 64 + 1023) / 1024; ++u) { const int off = (u * 64 + lane) * 16; if (off < nH) *reinterpret_cast<qu4*>(gH + off) = *reinterpret_cast<const qu4*>(sH + off); }
#pragma unroll
        for (int u = 0; u < (QR * 24 + 1023) / 1024; ++u) { const int off = (u * 64 + lane) * 16; if (off + 16 <= nF) *reinterpret_cast<qu4*>(gF + off) = *reinterpret_cast<const qu4*>(sF + off);
                                      else if (off < nF) *reinterpret_cast<u32x2*>(gF + off) = *reinterpret_cast<const u32x2*>(sF + off); }
        { const int off = lane * 2; if (off < nS) *reinterpret_cast<unsigned short*>(gS + off) = *reinterpret_cast<const unsigned short*>(sS + off); }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the image is read before the next block's items overwrite it
    }
}

// (Round 3, measured and removed: a row-walking form -- one wave keeps its 64 rows and walks all their K blocks, block kb + 1 loaded into registers under the
// encoding of block kb, so that the two pieces of a straddled cache line are read by the same CU (the counters show 1.35x the algorithmic read bytes at an L2 hit
// rate of 63 % for the form above) -- 0.446 against 0.388 ms on the configs[1] `a`, 4.75 against 4.69 ms per step: Kb times fewer, longer-lived waves at three
// per SIMD keep fewer bytes in flight than the many short ones.)

// ---- GEMM --------------------------------------------------------------------------------------------------------------
struct F6P {
    const char* AH; const char* AFL; const char* AS;
    const char* BH; const char* BFL; const char* BS;
    int64_t pA, pAS, pB, pBS;                  // rows_alloc / rows_allocS of the two operands
    int64_t rA, rB;
    int M, N, Kb, total_tiles;
    float* C; int64_t ldc_m, ldc_n, sC; int gdiv;
    const float* scale; int scale_div; const float* bias; int relu;
    float* sm_part; const uint8_t* sm_mask; int sm_rows_per_obj, sm_objs; unsigned sm_magic;      // row / rows_per_obj = umulhi(row, magic) (rows < 2^24)
    char* oH; char* oFL; char* oS; int64_t o_ra, o_ras; int o_rdiv, o_rstride;                    // F6_EPI_PLANES_T: the output planes
    const unsigned* plan;                      // F6_EPI_INTERLEAVE2, optional: the tile plan (cti_mode3_plan.hip): which tiles this launch walks
};
// the kernels' only parameter, as it sits at the head of the kernel-argument segment (constant address space: scalar loads)
typedef const __attribute__((address_space(4))) F6P F6P_K;
__device__ __forceinline__ const F6P_K* f6_kernarg() { return __builtin_bit_cast(const F6P_K*, __builtin_amdgcn_kernarg_segment_ptr()); }
enum { F6_EPI_F32 = 0, F6_EPI_INTERLEAVE2 = 2, F6_EPI_INTERLEAVE = 3, F6_EPI_INTERLEAVE2_SM = 5, F6_EPI_PLANES_T = 6 };   // _SM: + softmax partials; _T: see F6GemmArgs

// ---- tile walk from a plan (cti_f16f6.h, "tile plan"): virtual tile `id` of `total` live ones -> (sample, row tile, column tile).  As tile_coords has it, each XCD
// walks a contiguous chunk of the virtual sequence; a sample's LIVE row tiles run fastest, so that one column tile of the B operand serves them back to back out of
// one L2.  A sample's tiles are tiles_n x (its live row tiles) consecutive ids, so id / tiles_n is a row-tile index of that sample: ONE 16-B scalar load of that
// entry gives the sample, its first row tile and its count.  The plan was written by an earlier kernel and is constant here (constant address space: scalar loads,
// no vmcnt).
typedef unsigned f6p_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) f6p_u32x4 F6PlanEntry_K;
typedef const __attribute__((address_space(4))) unsigned F6PlanWord_K;
__device__ __forceinline__ void plan_coords(const unsigned* plan, int id, int total, int tiles_n, int& z, int& tm, int& tn) {
    const int q = total >> 3, r = total & 7, xcd = id & 7, slot = id >> 3;
    const int vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    const f6p_u32x4 e = __builtin_bit_cast(F6PlanEntry_K*, plan + M3P_HEAD_WORDS)[vid / tiles_n];
    const int t = vid - (int)e[1] * tiles_n, live = (int)e[2];
    z = (int)e[0]; tn = t / live; tm = t - tn * live;
}

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// 256 x 192 tile, 8 waves.  One ring slot = one 32-deep K block of both operands:
//   A_H 256 rows x 64 B | B_H 192 x 64 B | A_FL 256 x 24 B | B_FL 192 x 24 B | A_S 256 x 2 B | B_S 192 x 2 B
// = 40 pieces (one LDS-DMA wave-instruction each; the last one 384 B), five per wave; four slots + the bias KiB fill the CU's 160 KiB.
template <int WM_, int WN_, int TM_, int TN_, int NST_ = 4>
struct GeoF6T {
    static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, NST = NST_;
    static constexpr int BM = WM * TM * 32, BN = WN * TN * 32, NTHR = WM * WN * 64, NW = WM * WN;
    static constexpr int PAH = BM / 16, PBH = BN / 16, PAF = BM * 24 / 1024, PBF = BN * 24 / 1024;      // whole pieces; B_FL leaves a 512-B tail
    static constexpr int OFF_AH = 0, OFF_BH = OFF_AH + BM * 64, OFF_AFL = OFF_BH + BN * 64, OFF_BFL = OFF_AFL + BM * 24;
    static constexpr int OFF_AS = OFF_BFL + BN * 24, OFF_BS = OFF_AS + 512;                            // (the A scales' half piece always moves 512 B = 256 rows)
    // Round 5: the B scales' piece moves its BN * 2 real bytes only (lanes >= BS_LANES sit the instruction out; the first form moved a whole KiB and the slot
    // ended in 640 B of slack): 2.5 KiB of the CU's LDS come free -- 1 KiB of it holds the transposed products' BIAS (the accumulators' initial value), which
    // was 32 registers per lane of a kernel at its 256-register ceiling.
    static constexpr int BS_LANES = BN * 2 / 16;
    static constexpr int SLOT = OFF_BS + BN * 2;
    static constexpr int BIAS_BYTES = BM * 4;
    static constexpr int NREAL = PAH + PBH + PAF + PBF + 2;          // pieces a slot needs
    static constexpr int CNT = (NREAL + NW - 1) / NW;                // pieces per wave and slot
    static constexpr int NPIECE = CNT * NW;                          // issued: the NPIECE - NREAL extra ones repeat the first pieces (same bytes, same place)
    static constexpr int LDS = NST * SLOT + BIAS_BYTES;
    static constexpr int MINW = 160 * 1024 / LDS >= 2 ? 2 * NW / 4 : NW / 4;     // waves per SIMD the launch bounds promise (two co-resident workgroups when the LDS allows)
    static_assert(BM * 24 % 1024 == 0 && BN * 24 % 1024 == 512 && BM * 2 <= 512, "the B_FL tail and the A scales share one piece");
    static_assert(BN * 2 % 16 == 0 && SLOT % 16 == 0, "slots stay 16-B aligned");
    static_assert(OFF_AS == OFF_BFL + PBF * 1024 + 512, "the shared piece is contiguous in LDS");
    static_assert(NST >= 2 && LDS <= 160 * 1024, "ring exceeds the CU's LDS");
};
#ifndef CTI_F6_TN
#define CTI_F6_TN 3          // column tiles per wave.  -DCTI_F6_TN=1 (timing experiments only): 256 x 64 tiles -- the K loops of a Tucker -> rank chain that keeps a 64-token a~
#endif                       // tile on chip and re-streams both weight matrices per tile (VERDICT r4 #1 iv; profiles/r05_aside_chain_ablation.txt)
using GeoF6 = GeoF6T<4, 2, 2, CTI_F6_TN>;            // 8 waves of 64 x 96, two per SIMD
// Round 3 experiment (d): 128 x 192 tiles, FOUR waves of 64 x 96 (the same wave tile, so the same fragment reads / conversions / MFMAs per wave
// and K block), a 2-slot ring of 31 KiB -- TWO independent workgroups per CU, each with its own barriers: one workgroup's epilogue (and every
// other phase) overlaps the other's K loop instead of idling the matrix pipe.  Price: 43 % more DMA bytes per flop and one block in flight.
// Round 5: compiled only with -DCTI_F6_WITH_HALF_GEO (tools/ab_f6_geo.sh builds that variant): its transposed-planes instantiation spills two registers to
// SCRATCH, and round 4 saw a scratch row corrupted beside another stream's kernel -- no kernel of the product library may own a private segment.
#ifdef CTI_F6_WITH_HALF_GEO
using GeoF6Half = GeoF6T<2, 2, 2, 3, 2>;
#endif


#ifndef CTI_F6_PHASE
#define CTI_F6_PHASE 0
#endif
#ifndef CTI_F6_ABL          // timing-only ablations (wrong results): 1 no refill DMA, 2 no MFMA, 4 no fp6 conversion, 8 no epilogue stores, 64 no lane swaps,
#define CTI_F6_ABL 0        // 256 the A operand's LDS fragment reads only in a tile's first K block, 512 no conversion of the A fragments, 1024 no DMA of the A
#endif                      // operand's pieces  (256 | 512 | 1024 = "the A operand is free": the ceiling of any scheme that takes it out of the LDS path)

typedef _Float16 f16x32 __attribute__((ext_vector_type(32)));
typedef unsigned u32x6 __attribute__((ext_vector_type(6)));

// e2m3 codes of the 16 f16 values a lane holds of its row's K block (k-steps 0 and 1 of the f16 MFMA), scaled by 2^(sbyte - 127): three
// dwords.  The instruction converts 32 values; its upper 16 inputs (and the three dwords they produce) are don't-cares.
__device__ __forceinline__ u32x6 f6_codes_of_f16(f16x8 k0, f16x8 k1, int sbyte) {
    const f16x32 in = __builtin_shufflevector(__builtin_shufflevector(k0, k1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
                                              __builtin_shufflevector(k0, k1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
                                              0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
    u32x6 out;
#if CTI_F6_ABL & 4
    out[0] = __builtin_bit_cast(unsigned, __builtin_shufflevector(k0, k0, 0, 1)); out[1] = __builtin_bit_cast(unsigned, __builtin_shufflevector(k1, k1, 0, 1)); out[2] = sbyte; return out;
#endif
    asm("v_cvt_scalef32_pk32_fp6_f16 %0, %1, %2" : "=&v"(out) : "v"(in), "v"(__builtin_bit_cast(float, (unsigned)(sbyte & 0xff) << 23)));
    return out;
}

// ---- epilogue of the tile at (z, m0, n0): the wave's TM x TN accumulator tiles -> C
template <int EPI, class G>
__device__ __forceinline__ void f6_epilogue(const f32x16 (&acc)[G::TM][G::TN], const F6P& p, int z, int cm0, int cn0, int wm, int wn, int lane, int tile_in_batch, int tiles_per_batch) {
    constexpr int TM = G::TM, TN = G::TN;
    const int r = lane & 31, h = lane >> 5;
    if (EPI == F6_EPI_PLANES_T) {
        // Transposed product: GEMM rows m = output features, columns n = activation rows; the result leaves as f16f6 planes of the
        // (N x M) matrix.  Register e of a 32 x 32 accumulator tile is feature 8 (e >> 2) + 4 h + (e & 3) of column r = lane & 31, so a
        // lane and its SIMD-half partner hold all 32 features of one (row, block) item between them -- and the wave's two row tiles are
        // two such blocks.  Sixteen v_permlane32_swap(tile 0 register, tile 1 register) hand the lower lanes all of tile 0 and the upper
        // lanes all of tile 1: every lane then encodes ONE complete item in registers (f6_encode_row32_regs).  No LDS, and NO global loads
        // (the bias came in as the accumulators' initial value): the ring keeps streaming the next tile's K blocks underneath, and nothing
        // here waits on vmcnt -- a load's wait would also wait for the previous item's stores.
        static_assert(EPI != F6_EPI_PLANES_T || TM == 2, "a lane pair owns the wave's two row tiles");
        const F6P_K* q = f6_kernarg();
        asm volatile("" : "+s"(q));
        const int mblk = cm0 + (wm * TM + h) * 32;                  // first feature of this lane's block
        const int kb = mblk >> 5;
        char* const oH = q->oH; char* const oFL = q->oFL; char* const oS = q->oS;
        const int64_t o_ra = q->o_ra, o_ras = q->o_ras;
        const int o_rdiv = q->o_rdiv, o_rstride = q->o_rstride;
        const bool mok = mblk < p.M;                                // M % 32 == 0: a block is all real or all padding
        const float lo_bound = p.relu ? 0.f : -__builtin_huge_valf();
        unsigned nq = 0, nr = 0;
        // (Round 5: the H stores -- 16 B per lane into 32 cache lines per lane half -- were also staged through the ring slot the tile's last K block frees and stored as
        // 512-B runs: 4-5 % faster per product on its own, nothing in the step; tools/experiments/f16f6_staged_h_stores.patch, profiles/r05_aside_hstage_ab.txt.)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            __builtin_amdgcn_sched_barrier(0);
            f32x16 t0 = acc[0][j], t1 = acc[1][j];
            asm volatile("" : "+v"(t0), "+v"(t1));
            float x[32];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                // (inline asm: given vector elements, the builtin form of this swap was folded to ONE instruction for all sixteen registers)
                float lo_ = t0[e], hi_ = t1[e];
                asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(lo_), "+v"(hi_));
                const int k = 8 * (e >> 2) + (e & 3);                // lo_: the lower-lane register (features k), hi_: the upper-lane one (k + 4)
                x[k] = lo_; x[k + 4] = hi_;
            }
            const int n = cn0 + (wn * TN + j) * 32 + r;
            const bool valid = !(n >= p.N || !mok || ((CTI_F6_ABL & 8) && x[0] != 12345.f));
            if (!valid) continue;
            // plane row of n: batches of o_rdiv rows start at multiples of o_rstride.  One division per tile (column tile 0); the wave's other column
            // tiles are 32 rows further on -- at most one batch boundary when a batch has 32 rows or more
            if (j == 0 || o_rdiv < 32) {
                nq = o_rdiv > 0 ? (unsigned)n / (unsigned)o_rdiv : 0u; nr = o_rdiv > 0 ? (unsigned)n - nq * (unsigned)o_rdiv : (unsigned)n;
            } else {
                nr += 32u;
                if (nr >= (unsigned)o_rdiv) { nr -= (unsigned)o_rdiv; ++nq; }
            }
            const int64_t prow = (int64_t)nq * o_rstride + nr;
            const int64_t o = (int64_t)kb * o_ra + prow;
#if CTI_F6_ABL & 4096     // timing-only: the four H pieces of the wave's 32 rows as four fully coalesced 512-B runs per lane half (WRONG placement): what staging the H rows through LDS could buy at most
            f6_encode_row32_regs(x, lo_bound, oH + ((int64_t)kb * o_ra + ((int64_t)nq * o_rstride + nr - r)) * 64 + r * 16, oFL + o * 24, oS + ((int64_t)kb * o_ras + prow) * 2, 32);
#else
            f6_encode_row32_regs(x, lo_bound, oH + o * 64, oFL + o * 24, oS + ((int64_t)kb * o_ras + prow) * 2);
#endif
        }
        return;
    }
    float* C = p.C + (int64_t)z * p.sC;
    if (EPI == F6_EPI_INTERLEAVE2 || EPI == F6_EPI_INTERLEAVE2_SM) {
        if (EPI == F6_EPI_INTERLEAVE2_SM) {
            // Softmax partials of this wave's 64 x 96 outputs.  Register e of a tile is row 8 (e >> 2) + 4 h + (e & 3) of its 32, so g = e & 1.
            // Two sweeps over the accumulators -- maxima, then one FMA and one v_exp_f32 per element: exp2(x log2e - max log2e) -- skipping what
            // must not count (rows beyond M or of a masked object, columns beyond N).
            constexpr float L2E = 1.4426950408889634f;
            const float ninf = -__builtin_huge_valf();
            float mx[2] = {ninf, ninf}, sum[2] = {0.f, 0.f};
            const F6P_K* q = f6_kernarg();                          // the partials' own parameters, loaded here rather than held across the K loops
            asm volatile("" : "+s"(q));
            const uint8_t* sm_mask = q->sm_mask + (int64_t)z * q->sm_objs;
            const unsigned sm_magic = q->sm_magic;
            bool cok[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) cok[j] = cn0 + (wn * TN + j) * 32 + r < p.N;
            // row predicates (one per (v,q) row = pair of registers per tile), kept as VGPR integers and compared where they are used: sixteen
            // live lane masks cost the K loop its scalar registers.  The mask bytes are loaded unconditionally (clamped row).
            int okv[TM][4][2];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int eg = 0; eg < 4; ++eg)
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        const int m = cm0 + (wm * TM + i) * 32 + 8 * eg + 4 * h + 2 * pr;
                        const unsigned mc = (unsigned)min(m, p.M - 1);
                        const uint8_t mb = sm_mask[sm_magic ? __umulhi(mc, sm_magic) : mc];
                        okv[i][eg][pr] = (int)(m < p.M) & (int)(mb == 0);
                    }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (okv[i][e >> 2][(e >> 1) & 1] != 0 && cok[j]) mx[e & 1] = fmaxf(mx[e & 1], acc[i][j][e]);
            const float sh[2] = {mx[0] == ninf ? 0.f : mx[0] * L2E, mx[1] == ninf ? 0.f : mx[1] * L2E};
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (okv[i][e >> 2][(e >> 1) & 1] != 0 && cok[j]) sum[e & 1] += __builtin_amdgcn_exp2f(fmaf(acc[i][j][e], L2E, -sh[e & 1]));
            float* o = q->sm_part + (((int64_t)z * tiles_per_batch + tile_in_batch) * G::NW + wm * G::WN + wn) * 4;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const float wmx = wave_max(mx[g]);
                const float ws = wave_sum(mx[g] == ninf ? 0.f : sum[g] * __builtin_amdgcn_exp2f((mx[g] - wmx) * L2E));
                if (lane == 0) { o[g * 2] = wmx; o[g * 2 + 1] = ws; }
            }
        }
        // GEMM rows (2m, 2m+1) are the two glimpses of one (v,q) row: registers e, e+1 (e even) of a lane are the adjacent floats
        // out[b, vq, a, 0:2] of column a = n.  Neighbouring lanes (columns n, n+1) trade halves through a DPP quad swap so that the even lane
        // stores out[vq, n:n+2, 0:2] and the odd lane out[vq+1, n-1:n+1, 0:2]: ONE 16-B store per four registers instead of two 8-B ones --
        // the epilogue is store-ISSUE bound (cdna_hip_programming.md T21), so this halves it.
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const bool odd = lane & 1;
        auto swap1 = [](float x) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true)); };
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = cn0 + (wn * TN + j) * 32 + r - (odd ? 1 : 0);      // even column: this lane's 16 B start here
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                // One accumulator tile at a time through an explicit VGPR copy: used directly, the allocator moves ALL accumulators out of
                // the AGPRs in front of the epilogue and spills the next block's operands to make room.
                __builtin_amdgcn_sched_barrier(0);
                f32x16 tv = acc[i][j];
                asm volatile("" : "+v"(tv));
#pragma unroll
                for (int e = 0; e < 16; e += 4) {
                    const float r0 = tv[e], r1 = tv[e + 1], r2 = tv[e + 2], r3 = tv[e + 3];
                    const float t0 = swap1(odd ? r0 : r2), t1 = swap1(odd ? r1 : r3);
                    const int m = cm0 + (wm * TM + i) * 32 + 8 * (e >> 2) + 4 * h + (odd ? 2 : 0);      // even GEMM row = (vq, g = 0)
                    if (m >= p.M || col >= p.N || ((CTI_F6_ABL & 8) && r0 != 12345.f)) continue;
                    float* dst = C + (int64_t)(m >> 1) * p.ldc_m + (int64_t)col * 2;
                    if (col + 1 < p.N) {
                        f32x4 v4; v4[0] = odd ? t0 : r0; v4[1] = odd ? t1 : r1; v4[2] = odd ? r2 : t0; v4[3] = odd ? r3 : t1;
                        *reinterpret_cast<f32x4*>(dst) = v4;
                    } else {
                        f32x2 v2; v2[0] = odd ? t0 : r0; v2[1] = odd ? t1 : r1;
                        *reinterpret_cast<f32x2*>(dst) = v2;
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = cn0 + (wn * TN + j) * 32 + r;
            if (n >= p.N) continue;
            const float sc = p.scale ? p.scale[n / p.scale_div] : 1.f;
            const float bi = p.bias ? p.bias[n] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = cm0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (m < p.M && !((CTI_F6_ABL & 8) && sc != 12345.f)) {
                        float x = acc[i][j][e] * sc + bi;
                        if (p.relu) x = relu_nan(x);
                        C[(int64_t)(m / p.gdiv) * p.ldc_m + (m % p.gdiv) + (int64_t)n * p.ldc_n] = x;
                    }
                }
        }
    }
}

template <int EPI, class G>
__global__ __launch_bounds__(G::NTHR, G::MINW) void gemm_f16f6_kernel(F6P p) {
    constexpr int WN = G::WN, TM = G::TM, TN = G::TN, NST = G::NST, BM = G::BM, BN = G::BN, NW = G::NW, SLOT = G::SLOT, CNT = G::CNT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wid = __builtin_amdgcn_readfirstlane(t >> 6);        // scalar: every piece address below is SGPR base + VGPR lane offset
    const int wm = wid / WN, wn = wid % WN;
    const int r = lane & 31, h = lane >> 5;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    // F6_EPI_INTERLEAVE2 with a tile plan: the number of tiles is the plan's first word -- what the device found live in THIS call's inputs -- and the two per-tile
    // set-ups below map a tile index through the plan.  The plan's pointer is re-read from the kernel-argument segment where it is needed, like their other operands.
    int total_tiles = p.total_tiles;
    if (EPI == F6_EPI_INTERLEAVE2) {
        const F6P_K* q = f6_kernarg();
        asm volatile("" : "+s"(q));
        const unsigned* plan = q->plan;
        if (plan) total_tiles = (int)__builtin_bit_cast(F6PlanWord_K*, plan)[M3P_W_TILES];
    }
    if ((int)blockIdx.x >= total_tiles) return;
    // The workgroup's tiles (blockIdx.x, + gridDim.x, ...) are ONE stream of K blocks through the ring: the DMA of the next tile's first
    // blocks is issued during the current tile's last ones, so that the ring never drains at a tile boundary and the epilogue's stores
    // overlap with loads already in flight.
    const int nkb = p.Kb;
    const int nblk = ((total_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1) * nkb;
    // ---- DMA side.  Piece g = wid + 8 u (u = 0 .. 4) of the slot's list [A_H x16 | B_H x12 | A_FL x6 | B_FL x4 | B_FL tail + A_S | B_S]; the
    // last but one (wave 6, u = 4) takes its lower 32 lanes from the B_FL tail and its upper 32 from the A scales.  Every piece has a per-lane
    // 64-bit source pointer (H pieces: rows (lane >> 2) of the piece, 16-B chunk (lane & 3) ^ ((row >> 2) & 3); the others 16 B per lane) that
    // walks the K blocks of the tile being issued: one VALU add per piece and block, no scalar address arithmetic in the loop.
    const char* vp[CNT]; int64_t kstride[CNT]; int ldsoff[CNT];
    bool piece_is_a[CNT];                                           // (ablation 1024 only)
    bool piece_is_bs[CNT];                                          // the B scales: BS_LANES lanes take part
    const bool shared_piece_wave = (G::NREAL - 2) % NW == wid;
    constexpr int U_SHARED = (G::NREAL - 2) / NW;                   // which of that wave's pieces is the shared one
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
        int g = wid + u * NW;
        if (g >= G::NREAL) g -= G::NREAL;                          // padding pieces repeat the slot's first ones
        piece_is_a[u] = g < G::PAH || (g >= G::PAH + G::PBH && g < G::PAH + G::PBH + G::PAF);
        if (g < G::PAH)                   { kstride[u] = p.pA * 64; ldsoff[u] = G::OFF_AH + g * 1024; }
        else if ((g -= G::PAH) < G::PBH)  { kstride[u] = p.pB * 64; ldsoff[u] = G::OFF_BH + g * 1024; }
        else if ((g -= G::PBH) < G::PAF)  { kstride[u] = p.pA * 24; ldsoff[u] = G::OFF_AFL + g * 1024; }
        else if ((g -= G::PAF) <= G::PBF) { kstride[u] = p.pB * 24; ldsoff[u] = G::OFF_BFL + g * 1024; }   // g == PBF: the tail
        else                              { kstride[u] = p.pBS * 2; ldsoff[u] = G::OFF_BS; }
        piece_is_bs[u] = ldsoff[u] == G::OFF_BS;
    }
    const int64_t vks_shared = (shared_piece_wave && h) ? p.pAS * 2 : kstride[U_SHARED];    // per lane: the shared piece's halves walk different planes
    int iss_tile = blockIdx.x, iss_kb = 0, issued = 0;
    auto issue_tile_setup = [&]() {
        // The plane pointers and batch strides are needed once per tile: they are re-read from the kernel-argument segment here (scalar loads
        // through a pointer the optimiser cannot see through) instead of living in ~24 scalar registers across every K block.
        const F6P_K* q = f6_kernarg();
        asm volatile("" : "+s"(q));
        int zz, tm, tn;
        const unsigned* plan = EPI == F6_EPI_INTERLEAVE2 ? q->plan : nullptr;
        if (EPI == F6_EPI_INTERLEAVE2 && plan) plan_coords(plan, iss_tile, total_tiles, tiles_n, zz, tm, tn);
        else tile_coords(iss_tile, total_tiles, tiles_m, tiles_n, zz, tm, tn);
        const int64_t ra = (int64_t)zz * q->rA + tm * BM, rb = (int64_t)zz * q->rB + tn * BN;
        int w = wid;
        asm volatile("" : "+s"(w));                                 // (keeps the descriptor arithmetic below out of the K loop's live registers)
        const unsigned hoff = (unsigned)((lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4)), loff = (unsigned)lane * 16u;
#pragma unroll
        for (int u = 0; u < CNT; ++u) {
            int g = w + u * NW;
            if (g >= G::NREAL) g -= G::NREAL;
            if (g < G::PAH)                   vp[u] = q->AH + (ra + g * 16) * 64 + hoff;
            else if ((g -= G::PAH) < G::PBH)  vp[u] = q->BH + (rb + g * 16) * 64 + hoff;
            else if ((g -= G::PBH) < G::PAF)  vp[u] = q->AFL + ra * 24 + g * 1024 + loff;
            else if ((g -= G::PAF) <= G::PBF) vp[u] = q->BFL + rb * 24 + g * 1024 + loff;
            else                              vp[u] = q->BS + rb * 2 + loff;
        }
        if (shared_piece_wave && h) vp[U_SHARED] = q->AS + ra * 2 - 512 + loff;     // upper 32 lanes: the A scales, 16 B per lane from lane 32 on
    };
    auto issue_next = [&](int pos) {                                // the stream's next K block into ring slot `pos`
        if (issued >= nblk || (CTI_F6_ABL & 1)) return;
        char* slot = smem + pos * SLOT;
#pragma unroll
        for (int u = 0; u < CNT; ++u) {
            // (round 6: only piece NREAL - 1 = (wave (NREAL - 1) % NW, u = (NREAL - 1) / NW) can be the B scales: the other u issue unconditionally -- the test was a
            // run-time exec-mask sequence in front of EVERY piece of every K block)
            if (u == (G::NREAL - 1) / NW && piece_is_bs[u]) { if (lane < G::BS_LANES) dma16(vp[u], slot + ldsoff[u]); }      // (wave-uniform branch; the piece's upper lanes would write past the slot)
            else if (!((CTI_F6_ABL & 1024) && piece_is_a[u])) dma16(vp[u], slot + ldsoff[u]);
            vp[u] += u == U_SHARED ? vks_shared : kstride[u];
        }
        ++issued;
        if (++iss_kb == nkb) {
            iss_kb = 0; iss_tile += (int)gridDim.x;
            if (iss_tile < total_tiles) issue_tile_setup();
        }
    };
    // vmcnt part of "block b has landed": the pieces this wave issued for the blocks after b may still be in flight -- min(NST - 2, blocks
    // left) of them at every point this is called from.  vmcnt retires in issue order (stores included), so epilogue stores issued after
    // those pieces only ever make the wait conservative.
    // (Measured and dropped: looking past an interior tile's 24 epilogue stores with vmcnt(2 CNT + 24) for the two waits that have them inside
    // their window, instead of waiting for all but the last few stores one K block after they were issued: 2.06 against 2.04 ms -- the stores'
    // retirement is not what the epilogue costs.)
    auto wait_block = [&](int b) {
        const int rem = nblk - 1 - b;
        if (rem >= NST - 2) wait_vm<(NST - 2) * CNT>();
        else if (NST >= 4 && rem == 1) wait_vm<CNT>();
        else wait_vm<0>();
    };

#if CTI_F6_ABL & 128                                                 // clock probe: shader cycles / 100 MHz ticks of this workgroup -> C[2 bx], C[2 bx + 1]
    const unsigned long long probe_c0 = __builtin_readcyclecounter(), probe_r0 = __builtin_amdgcn_s_memrealtime();
#endif
#if CTI_F6_PHASE > 0                                                 // workgroups start up to CTI_F6_PHASE us apart (bit-reversed index: neighbours far apart in time)
    if (p.total_tiles > 2 * (int)gridDim.x) {
        const unsigned long long ph_t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned ph_d = (__builtin_bitreverse32(blockIdx.x) >> 24) * (CTI_F6_PHASE * 100u) / 256u;
        while (__builtin_amdgcn_s_memrealtime() - ph_t0 < ph_d) __builtin_amdgcn_s_sleep(16);
    }
#endif
    issue_tile_setup();
#pragma unroll
    for (int i = 0; i < NST - 1; ++i) issue_next(i);

    // ---- compute side
    int vtile = blockIdx.x, z = 0, m0 = 0, n0 = 0;
    auto compute_tile_setup = [&]() {
        int tm, tn;
        if (EPI == F6_EPI_INTERLEAVE2) {
            const F6P_K* q = f6_kernarg();
            asm volatile("" : "+s"(q));
            const unsigned* plan = q->plan;
            if (plan) plan_coords(plan, vtile, total_tiles, tiles_n, z, tm, tn);
            else tile_coords(vtile, total_tiles, tiles_m, tiles_n, z, tm, tn);
        } else tile_coords(vtile, total_tiles, tiles_m, tiles_n, z, tm, tn);
        m0 = tm * BM; n0 = tn * BN;
    };
    compute_tile_setup();
    f32x16 acc[TM][TN];
    // F6_EPI_PLANES_T: the accumulators start from the bias of their GEMM row (register e of row tile i: row 8 (e >> 2) + 4 h + (e & 3)).  Round 5: the workgroup's
    // BM bias values live in the KiB behind the ring (written once: with a power-of-two number of row tiles <= 32 a workgroup's row tile never changes) and every tile
    // reads its 32 values per lane from there (eight ds_read_b128) -- they were 32 registers per lane for the whole kernel.
    float* const bias_lds = reinterpret_cast<float*>(smem + NST * SLOT);
    int bv_m0 = -1;
    auto load_bias = [&]() {
        if (EPI != F6_EPI_PLANES_T || bv_m0 == m0) return;
        const bool first = bv_m0 < 0;
        bv_m0 = m0;
        if (!first) __builtin_amdgcn_s_barrier();                   // (mid-stream: every wave has read the old row tile's values)
        if (t < BM) {
            const int m = m0 + t;
            float b1 = 0.f;
            if (p.bias && m < p.M) {
                const float* src = p.bias + m;
                if (first) b1 = src[0];
                else       // mid-stream: an opaque load with its own wait, so that the compiler's vmcnt bookkeeping of the tile loop stays as it is
                    asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(b1) : "v"(src) : "memory");
            }
            bias_lds[t] = b1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    auto zero_acc = [&]() {
        load_bias();
        if (EPI == F6_EPI_PLANES_T) {
            typedef float f32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_lds + (wm * TM + i) * 32 + 8 * g4 + 4 * h);
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[i][j][4 * g4 + u] = b4[u];
                }
            return;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    };
    zero_acc();

    // per-lane fragment addresses inside a slot; tile i / j of the wave adds a compile-time constant (32 rows) that folds into the ds_read
    // offset.  fp6 rows: the lower lane half reads dwords 0-2 of its row's 24 B, the upper half dwords 3-5 (the permlane swaps below put them
    // where the MFMA wants them).  Scales: the dword that holds the row's (hi, lo) byte pair, and the shifts that bring the wanted byte down.
    const int sw = (r >> 2) & 3;                                    // (row >> 2) & 3: rows of a tile start at multiples of 32
    const int c0 = ((0 + h) ^ sw) << 4, c1 = ((2 + h) ^ sw) << 4;   // swizzled chunk offsets of k-steps 0 and 1
    const int rowA = wm * TM * 32 + r, rowB = wn * TN * 32 + r;
    const int aH0 = G::OFF_AH + rowA * 64 + c0, aH1 = G::OFF_AH + rowA * 64 + c1, bH0 = G::OFF_BH + rowB * 64 + c0, bH1 = G::OFF_BH + rowB * 64 + c1;
    const int aF = G::OFF_AFL + rowA * 24 + 8 * h, bF = G::OFF_BFL + rowB * 24 + 8 * h;           // dwords (0,1) / (3,4) of the row as stored [0 1 3 4 2 5]
    const int aF2 = G::OFF_AFL + rowA * 24 + 16 + 4 * h, bF2 = G::OFF_BFL + rowB * 24 + 16 + 4 * h;  // dword 2 / 5
    const int aS = G::OFF_AS + ((rowA * 2) & ~3), bS = G::OFF_BS + ((rowB * 2) & ~3);
    const int shS = (r & 1) * 16;                                   // the row's (hi, lo) scale bytes inside that dword (tile rows are even offsets apart)
    const int shA = shS + h * 8, shB = shS + (1 - h) * 8;           // the byte the MFMA takes: A lower lanes hi / upper lo, B the other way round

    auto epilogue = [&]() { f6_epilogue<EPI, G>(acc, p, z, m0, n0, wm, wn, lane, (m0 / BM) * tiles_n + n0 / BN, tiles_m * tiles_n); };

    // ---- the stream.  Per block b: [vmcnt: my pieces of b have landed] raw barrier (everyone's have, and block b - 1 is free) -> the
    // stream's next block is issued into the freed slot -> fragments -> MFMAs; after a tile's last block its epilogue.
    // TILE BOUNDARY: the vmcnt wait that the first barrier after an epilogue needs is taken BEFORE the stores (the block in question was
    // issued two K blocks earlier), so that no wave waits for its stores to retire before the next tile's first MFMAs.
    // (s_setprio 1 / 3 around the MFMA cluster: 2.00 against 1.97 ms.)
    // (Measured and dropped with the continuous stream in place, each within +-2 %: a half-block stagger of the two waves of a SIMD,
    // spreading the workgroups' start times over one tile, issuing the refill behind the MFMAs, and reloading operands in place as they die
    // so that block b + 1's reads and conversions run under block b's MFMAs (2.08 against 2.00 ms): the partner wave of the SIMD was
    // already filling those gaps.  tools/mb/mb_issue.hip: 18 MFMAs + 100 VALU + 5 conversions per wave in registers take 1.09 us per
    // block against 0.84 for the MFMAs alone; this loop takes 1.56 with LDS reads, DMA and barriers on top.)
    // Fragments of one K block.  A lane (row r of a 32-row tile, SIMD half h) reads its 2 x 8 f16 values (k = 8h .. 8h+7 and 16+8h .. 16+8h+7),
    // converts them to fp6 under the row's hi scale, and trades with its partner lane: v_permlane32_swap(X, Y) exchanges X's upper lanes
    // with Y's lower lanes.  A operand: X = own codes, Y = the lane's half of the lo codes from LDS; after the swap the lower lanes hold
    // [own | partner's] = the hi codes of the whole block in the f6_pi order, the upper lanes the six lo dwords.  B operand: X = lo codes
    // from LDS, Y = own; afterwards the lower lanes hold the lo dwords, the upper ones [partner's | own] hi codes.
#if CTI_F6_ABL & 64
#define CTI_F6_SWAP(x, y) u32x2{(unsigned)(x), (unsigned)(y)}
#else
#define CTI_F6_SWAP(x, y) __builtin_amdgcn_permlane32_swap((unsigned)(x), (unsigned)(y), false, false)
#endif
#if CTI_F6_ABL & 256
    f16x8 keep_a16[TM][2]; int keep_fa[TM][3], keep_spa[TM];
#endif
#define CTI_F6_A_READ_REAL(i)                                                                                                         \
            a16[i][0] = *reinterpret_cast<const f16x8*>(s_a0 + i * 2048);                                                             \
            a16[i][1] = *reinterpret_cast<const f16x8*>(s_a1 + i * 2048);                                                             \
            { const u32x2 f01 = *reinterpret_cast<const u32x2*>(s_af + i * 768); fa[i][0] = f01.x; fa[i][1] = f01.y; }                  \
            fa[i][2] = *reinterpret_cast<const int*>(s_af2 + i * 768);                                                                \
            spa[i] = *reinterpret_cast<const int*>(s_as + i * 64);
#if CTI_F6_ABL & 256
#define CTI_F6_ABL_A_READ(i)                                                                                                          \
            if (kb == 0) { CTI_F6_A_READ_REAL(i)                                                                                      \
                keep_a16[i][0] = a16[i][0]; keep_a16[i][1] = a16[i][1]; keep_fa[i][0] = fa[i][0]; keep_fa[i][1] = fa[i][1]; keep_fa[i][2] = fa[i][2]; keep_spa[i] = spa[i]; } \
            else { a16[i][0] = keep_a16[i][0]; a16[i][1] = keep_a16[i][1]; fa[i][0] = keep_fa[i][0]; fa[i][1] = keep_fa[i][1]; fa[i][2] = keep_fa[i][2]; spa[i] = keep_spa[i]; }
#else
#define CTI_F6_ABL_A_READ(i) CTI_F6_A_READ_REAL(i)
#endif
#define CTI_F6_READ_FRAGS(s)                                                                                                          \
    f16x8 a16[TM][2], b16[TN][2]; i32x8 a6[TM], b6[TN]; int sa[TM], sb[TN]; int fa[TM][3], fb[TN][3], spa[TM], spb[TN];               \
    {                                                                                                                                 \
        const char *s_a0 = (s) + aH0, *s_a1 = (s) + aH1, *s_b0 = (s) + bH0, *s_b1 = (s) + bH1, *s_af = (s) + aF, *s_bf = (s) + bF, *s_as = (s) + aS, *s_bs = (s) + bS; \
        const char *s_af2 = (s) + aF2, *s_bf2 = (s) + bF2;                                                                            \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) {         /* every LDS read of the block first: one latency, not five */        \
            CTI_F6_ABL_A_READ(i)                                                                                                      \
        }                                                                                                                             \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                                              \
            b16[j][0] = *reinterpret_cast<const f16x8*>(s_b0 + j * 2048);                                                             \
            b16[j][1] = *reinterpret_cast<const f16x8*>(s_b1 + j * 2048);                                                             \
            { const u32x2 f01 = *reinterpret_cast<const u32x2*>(s_bf + j * 768); fb[j][0] = f01.x; fb[j][1] = f01.y; }                  \
            fb[j][2] = *reinterpret_cast<const int*>(s_bf2 + j * 768);                                                                \
            spb[j] = *reinterpret_cast<const int*>(s_bs + j * 64);                                                                    \
        }                                                                                                                             \
    }                                                                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                           /* (the scheduler would otherwise pair each read with its conversion) */ \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) {                                                                                  \
        const u32x6 own = (CTI_F6_ABL & 512) ? u32x6{(unsigned)fa[i][0], (unsigned)fa[i][1], (unsigned)fa[i][2], 0u, 0u, 0u} : f6_codes_of_f16(a16[i][0], a16[i][1], spa[i] >> shS); \
        const auto w0 = CTI_F6_SWAP(own[0], fa[i][0]);                                                                                \
        const auto w1 = CTI_F6_SWAP(own[1], fa[i][1]);                                                                                \
        const auto w2 = CTI_F6_SWAP(own[2], fa[i][2]);                                                                                \
        a6[i][0] = w0[0]; a6[i][1] = w1[0]; a6[i][2] = w2[0]; a6[i][3] = w0[1]; a6[i][4] = w1[1]; a6[i][5] = w2[1]; a6[i][6] = 0; a6[i][7] = 0; \
        sa[i] = spa[i] >> shA;                                      /* the MFMA takes byte 0: lower lanes multiply hi codes, upper lanes lo codes */ \
    }                                                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                                                  \
        const u32x6 own = f6_codes_of_f16(b16[j][0], b16[j][1], spb[j] >> shS);                                                       \
        const auto w0 = CTI_F6_SWAP(fb[j][0], own[0]);                                                                                \
        const auto w1 = CTI_F6_SWAP(fb[j][1], own[1]);                                                                                \
        const auto w2 = CTI_F6_SWAP(fb[j][2], own[2]);                                                                                \
        b6[j][0] = w0[0]; b6[j][1] = w1[0]; b6[j][2] = w2[0]; b6[j][3] = w0[1]; b6[j][4] = w1[1]; b6[j][5] = w2[1]; b6[j][6] = 0; b6[j][7] = 0; \
        sb[j] = spb[j] >> shB;                                                                                                        \
    }
#define CTI_F6_MFMAS()                                                                                                                \
    if (!(CTI_F6_ABL & 2) || p.Kb < 0) {         /* ablation: never true, the fragments stay live, the MFMAs do not issue */          \
        _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                                                \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) {                                                                          \
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a6[i], b6[j], acc[i][j], 2, 2, 0, sa[i], 0, sb[j]);       \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[i][0], b16[j][0], acc[i][j], 0, 0, 0);                         \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a16[i][1], b16[j][1], acc[i][j], 0, 0, 0);                         \
            }                                                                                                                         \
    }
    int kb = 0, pos = 0;
    bool waited = false;                                            // the vmcnt wait of the next barrier has been taken already
    for (int b = 0;;) {
        if (!waited) wait_block(b);
        waited = false;
        __builtin_amdgcn_s_barrier();
        issue_next(pos == 0 ? NST - 1 : pos - 1);
        const char* s = smem + pos * SLOT;
        CTI_F6_READ_FRAGS(s)
        CTI_F6_MFMAS()
        pos = pos == NST - 1 ? 0 : pos + 1;
        ++b;
        if (++kb == nkb) {
            if (b < nblk) { wait_block(b); waited = true; }
            epilogue();
            if (b >= nblk) break;
            kb = 0; vtile += (int)gridDim.x; compute_tile_setup(); zero_acc();
        }
    }
#undef CTI_F6_READ_FRAGS
#undef CTI_F6_ABL_A_READ
#undef CTI_F6_A_READ_REAL
#undef CTI_F6_SWAP
#undef CTI_F6_MFMAS
#if CTI_F6_ABL & 128
    if (t == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        p.C[2 * blockIdx.x] = (float)(__builtin_readcyclecounter() - probe_c0); p.C[2 * blockIdx.x + 1] = (float)(__builtin_amdgcn_s_memrealtime() - probe_r0);
    }
#endif
}

#ifndef CTI_F6_OVERSUB_DEFAULT
#define CTI_F6_OVERSUB_DEFAULT 1
#endif
// CTI_F6_GEO=half selects the two-workgroups-per-CU geometry (GeoF6Half) for the plain mode-3 product and the transposed a-side products
// (experiment (d) of round 3; the softmax-partials variant keeps the layout of its partials and stays on GeoF6).
#ifdef CTI_F6_WITH_HALF_GEO
static int f6_geo() { static const int g = [] { const char* e = getenv("CTI_F6_GEO"); return (e && e[0] == 'h') ? 1 : 0; }(); return g; }
#endif

template <int EPI, class G>
int launch_f6g(const F6P& p0, long long nb, int ncols, hipStream_t st) {
    auto kern = gemm_f16f6_kernel<EPI, G>;
    static thread_local int attr_dev = -1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (attr_dev != dev) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS);
        if (e != hipSuccess) return fail((int)e, "gemm_nt_f16f6: hipFuncSetAttribute: %s", hipGetErrorString(e));
        attr_dev = dev;
    }
    const long long total = nb * ((p0.M + G::BM - 1) / G::BM) * ((ncols + G::BN - 1) / G::BN);
    if (total > 0x7fffffffLL) return fail(CTI_E_SHAPE, "gemm_nt_f16f6: %lld tiles exceed the grid", total);
    F6P p = p0;
    p.total_tiles = (int)total;
    static thread_local int n_cu = 0;
    if (n_cu == 0) { (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev); if (n_cu <= 0) n_cu = 256; }
    // Workgroups per CU.  One = fully persistent: every workgroup walks total / n_cu tiles, assigned statically -- a CU that starts late because a
    // kernel of the other stream sat on it (the M build: one workgroup per CU, all of its LDS) finishes late, and the stream-ordered GEMM behind
    // this one waits for it.  With a few workgroups per CU the hardware dispatcher balances that: a delayed CU simply takes fewer of them; the
    // price is one ring refill per workgroup.  CTI_F6_OVERSUB overrides (experiments).  Geometries whose ring leaves room for two workgroups
    // per CU launch two per CU: they are co-resident, not queued.
    static const int oversub = [] { const char* e = getenv("CTI_F6_OVERSUB"); const int v = e ? atoi(e) : CTI_F6_OVERSUB_DEFAULT; return v < 1 ? 1 : v; }();
    long long grid = (long long)n_cu * oversub * (160 * 1024 / G::LDS >= 2 ? 2 : 1);
    if (grid > total) grid = total;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(G::NTHR), G::LDS, st, p);
    return launch_status("gemm_nt_f16f6");
}

template <int EPI>
int launch_f6(const F6P& p0, long long nb, int ncols, hipStream_t st) {
#ifdef CTI_F6_WITH_HALF_GEO
    if ((EPI == F6_EPI_INTERLEAVE2 || EPI == F6_EPI_PLANES_T) && f6_geo() == 1) return launch_f6g<EPI == F6_EPI_INTERLEAVE2 ? F6_EPI_INTERLEAVE2 : F6_EPI_PLANES_T, GeoF6Half>(p0, nb, ncols, st);
#endif
    return launch_f6g<EPI, GeoF6>(p0, nb, ncols, st);
}

}  // namespace

int quantize_f16f6(const float* x, int64_t ld, int64_t rows, int K, const F6Planes& p, hipStream_t st, const float* row_scale, int scale_div) {
    if (rows <= 0 || K <= 0) return fail(CTI_E_SHAPE, "quantize_f16f6: rows=%lld K=%d", (long long)rows, K);
#ifndef CTI_F6_QROWS
#define CTI_F6_QROWS 1
#endif
    static const bool qrows = [] { const char* e = getenv("CTI_F6_QROWS"); return e ? e[0] != '0' : (CTI_F6_QROWS != 0); }();
    if (qrows && ld == K && (K & 3) == 0 && K >= 32 && QR * K * 4 <= 72 * 1024 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (rows + QR - 1) / QR < (1ll << 31)) {
        // dense short rows (configs[1]'s `a`: 300 floats): whole 64-row runs through LDS-DMA
        const int lds = ((QR * K * 4 + 1023) / 1024) * 1024;
        static thread_local int attr_dev = -1;
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (attr_dev != dev) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(quantize_rows_f16f6_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 73 * 1024);
            if (e != hipSuccess) return fail((int)e, "quantize_f16f6: hipFuncSetAttribute: %s", hipGetErrorString(e));
            attr_dev = dev;
        }
        hipLaunchKernelGGL(quantize_rows_f16f6_kernel, dim3((unsigned)((rows + QR - 1) / QR)), dim3(256), lds, st, x, rows, K, p, row_scale, scale_div > 0 ? scale_div : 1);
        return launch_status("quantize_f16f6(rows)");
    }
    const int64_t bx = (rows + 255) / 256;
    const int64_t gz = (bx + 65534) / 65535, gy = (bx + gz - 1) / gz;          // row blocks spread over (y, z): y <= 65535
    if (gz > 65535) return fail(CTI_E_SHAPE, "quantize_f16f6: rows=%lld K=%d exceed the grid", (long long)rows, K);
    hipLaunchKernelGGL(quantize_f16f6_kernel, dim3((unsigned)p.Kb, (unsigned)gy, (unsigned)gz), dim3(256), 0, st, x, ld, rows, K, p, row_scale, scale_div > 0 ? scale_div : 1);
    return launch_status("quantize_f16f6");
}

int f6_mode3_tile_rows() {
#ifdef CTI_F6_WITH_HALF_GEO
    if (f6_geo() == 1) return GeoF6Half::BM;
#endif
    return GeoF6::BM;
}
int f6_mode3_tile_cols() {
#ifdef CTI_F6_WITH_HALF_GEO
    if (f6_geo() == 1) return GeoF6Half::BN;
#endif
    return GeoF6::BN;
}

int f6_sm_chunks(int M, int N) { return ((M + GeoF6::BM - 1) / GeoF6::BM) * ((N + GeoF6::BN - 1) / GeoF6::BN) * GeoF6::NW; }

int gemm_nt_f16f6(const F6GemmArgs& a, hipStream_t st) {
    if (a.A.Kb != a.B.Kb || a.A.Kb <= 0) return fail(CTI_E_SHAPE, "gemm_nt_f16f6: K blocks %d vs %d", a.A.Kb, a.B.Kb);
    if (a.M <= 0 || a.N <= 0 || a.nb <= 0) return fail(CTI_E_SHAPE, "gemm_nt_f16f6: M=%d N=%d nb=%d", a.M, a.N, a.nb);
    if ((a.A.rows_alloc | a.A.rows_allocS | a.B.rows_alloc | a.B.rows_allocS) & 7) return fail(CTI_E_ALIGN, "gemm_nt_f16f6: plane row counts must be multiples of 8");
    if (a.nb > 1 && ((a.rA | a.rB) & 7)) return fail(CTI_E_ALIGN, "gemm_nt_f16f6: batch strides rA=%lld rB=%lld must be multiples of 8 rows", (long long)a.rA, (long long)a.rB);
    F6P p{};
    p.AH = reinterpret_cast<const char*>(a.A.H); p.AFL = reinterpret_cast<const char*>(a.A.FL); p.AS = reinterpret_cast<const char*>(a.A.S);
    p.BH = reinterpret_cast<const char*>(a.B.H); p.BFL = reinterpret_cast<const char*>(a.B.FL); p.BS = reinterpret_cast<const char*>(a.B.S);
    p.pA = a.A.rows_alloc; p.pAS = a.A.rows_allocS; p.pB = a.B.rows_alloc; p.pBS = a.B.rows_allocS;
    p.rA = a.rA; p.rB = a.rB; p.M = a.M; p.N = a.N; p.Kb = a.A.Kb;
    p.C = a.C; p.ldc_m = a.ldc_m; p.ldc_n = a.ldc_n; p.sC = a.sC; p.gdiv = a.gdiv > 0 ? a.gdiv : 1;
    p.scale = a.scale; p.scale_div = a.scale_div > 0 ? a.scale_div : 1; p.bias = a.bias; p.relu = a.relu;
    p.sm_part = a.sm_part; p.sm_mask = a.sm_mask; p.sm_rows_per_obj = a.sm_rows_per_obj > 0 ? a.sm_rows_per_obj : 1; p.sm_objs = a.sm_objs;
    p.sm_magic = p.sm_rows_per_obj > 1 ? (unsigned)(((1ull << 32) + p.sm_rows_per_obj - 1) / p.sm_rows_per_obj) : 0u;
    switch (a.epi) {
        case 0: p.gdiv = 1; return launch_f6<F6_EPI_F32>(p, a.nb, a.N, st);
        case 3:
            if (a.sm_part && (a.M >= (1 << 24) || a.sm_rows_per_obj >= 256)) return fail(CTI_E_SHAPE, "gemm_nt_f16f6: softmax partials need M < 2^24 and rows per object < 256");
            if (a.sm_part && !(p.gdiv == 2 && a.ldc_n == 2 && a.sm_mask)) return fail(CTI_E_UNSUPPORTED, "gemm_nt_f16f6: softmax partials need gdiv = 2, ldc_n = 2 and a mask");
            if (a.plan && (a.sm_part || p.gdiv != 2 || a.ldc_n != 2)) return fail(CTI_E_UNSUPPORTED, "gemm_nt_f16f6: a tile plan needs gdiv = 2, ldc_n = 2 and no softmax partials");
            p.plan = a.plan;
            if (p.gdiv == 2 && a.ldc_n == 2) return a.sm_part ? launch_f6<F6_EPI_INTERLEAVE2_SM>(p, a.nb, a.N, st) : launch_f6<F6_EPI_INTERLEAVE2>(p, a.nb, a.N, st);
            return launch_f6<F6_EPI_INTERLEAVE>(p, a.nb, a.N, st);
        case 6:
            if (!a.out || a.nb != 1 || a.M % 32 != 0 || a.scale || a.out->Kb * 32 < a.M || a.N >= (1 << 30))
                return fail(CTI_E_UNSUPPORTED, "gemm_nt_f16f6: transposed planes output needs nb = 1, M %% 32 == 0, no epilogue scale and planes of >= M features");
            p.oH = reinterpret_cast<char*>(a.out->H); p.oFL = reinterpret_cast<char*>(a.out->FL); p.oS = reinterpret_cast<char*>(a.out->S);
            p.o_ra = a.out->rows_alloc; p.o_ras = a.out->rows_allocS; p.o_rdiv = (int)a.out->rdiv; p.o_rstride = (int)a.out->rstride; p.gdiv = 1;
            return launch_f6<F6_EPI_PLANES_T>(p, a.nb, a.N, st);
        default: return fail(CTI_E_UNSUPPORTED, "gemm_nt_f16f6: epi=%d", a.epi);
    }
}

}  // namespace cti

using namespace cti;

extern "C" size_t cti_f16f6_planes_bytes(int64_t rows, int K, int64_t batch_rows) {
    return rows > 0 && K > 0 && batch_rows >= 0 ? f6_planes_bytes(rows, K, batch_rows) : 0;
}

extern "C" int cti_quantize_f16f6(const float* x, int64_t ld, int64_t rows, int K, int64_t batch_rows, void* planes, size_t planes_bytes, void* stream) {
    CTI_REQUIRE_PTR(x); CTI_REQUIRE_PTR(planes);
    CTI_REQUIRE(rows > 0 && K > 0 && ld >= K && batch_rows >= 0, CTI_E_SHAPE, "cti_quantize_f16f6: rows=%lld K=%d ld=%lld batch_rows=%lld", (long long)rows, K, (long long)ld, (long long)batch_rows);
    CTI_REQUIRE(planes_bytes >= f6_planes_bytes(rows, K, batch_rows), CTI_E_WORKSPACE, "cti_quantize_f16f6: block %zu < %zu", planes_bytes, f6_planes_bytes(rows, K, batch_rows));
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(planes) & 255) == 0, CTI_E_ALIGN, "cti_quantize_f16f6: the plane block must be 256-B aligned");
    hipError_t e = hipMemsetAsync(planes, 0, f6_planes_bytes(rows, K, batch_rows), as_stream(stream));       // slack / padding rows: defined scales, zero codes
    if (e != hipSuccess) return fail((int)e, "cti_quantize_f16f6: hipMemsetAsync: %s", hipGetErrorString(e));
    return quantize_f16f6(x, ld, rows, K, f6_carve(planes, rows, K, batch_rows), as_stream(stream));
}

// The encoder alone, as cti_tcnet_forward launches it (round 5, VERDICT r4 #8: bench.py's stand-alone record of this pass timed the memset above with it):
// `planes` is a block cti_quantize_f16f6 has filled before, or one the caller zero-filled -- slack and padding rows are left as they are.
extern "C" int cti_quantize_f16f6_into(const float* x, int64_t ld, int64_t rows, int K, int64_t batch_rows, void* planes, size_t planes_bytes, void* stream) {
    CTI_REQUIRE_PTR(x); CTI_REQUIRE_PTR(planes);
    CTI_REQUIRE(rows > 0 && K > 0 && ld >= K && batch_rows >= 0, CTI_E_SHAPE, "cti_quantize_f16f6_into: rows=%lld K=%d ld=%lld batch_rows=%lld", (long long)rows, K, (long long)ld, (long long)batch_rows);
    CTI_REQUIRE(planes_bytes >= f6_planes_bytes(rows, K, batch_rows), CTI_E_WORKSPACE, "cti_quantize_f16f6_into: block %zu < %zu", planes_bytes, f6_planes_bytes(rows, K, batch_rows));
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(planes) & 255) == 0, CTI_E_ALIGN, "cti_quantize_f16f6_into: the plane block must be 256-B aligned");
    return quantize_f16f6(x, ld, rows, K, f6_carve(planes, rows, K, batch_rows), as_stream(stream));
}

extern "C" int cti_gemm_nt_f16f6(const void* A_planes, int64_t rowsA_total, int64_t batch_rowsA, const void* B_planes, int64_t rowsB_total, int64_t batch_rowsB,
                                 float* C, int64_t ldc_m, int64_t ldc_n, int64_t sC, int gdiv, int nb, int M, int N, int K, const float* scale, int scale_div,
                                 const float* bias, int act, void* stream) {
    CTI_REQUIRE_PTR(A_planes); CTI_REQUIRE_PTR(B_planes); CTI_REQUIRE_PTR(C);
    CTI_REQUIRE(M > 0 && N > 0 && K > 0 && nb > 0 && gdiv > 0, CTI_E_SHAPE, "cti_gemm_nt_f16f6: M=%d N=%d K=%d nb=%d gdiv=%d", M, N, K, nb, gdiv);
    CTI_REQUIRE(nb == 1 ? (M <= rowsA_total && N <= rowsB_total) : (M <= batch_rowsA && N <= batch_rowsB && (int64_t)nb * batch_rowsA <= rowsA_total && (int64_t)nb * batch_rowsB <= rowsB_total),
                CTI_E_SHAPE, "cti_gemm_nt_f16f6: batches run past the operand rows");
    CTI_REQUIRE(act == CTI_ACT_NONE || act == CTI_ACT_RELU, CTI_E_UNSUPPORTED, "cti_gemm_nt_f16f6: act=%d", act);
    F6GemmArgs g{};
    g.A = f6_carve(const_cast<void*>(A_planes), rowsA_total, K, batch_rowsA); g.B = f6_carve(const_cast<void*>(B_planes), rowsB_total, K, batch_rowsB);
    g.rA = g.A.rstride; g.rB = g.B.rstride; g.nb = nb; g.M = M; g.N = N;
    g.epi = gdiv > 1 ? 3 : 0; g.C = C; g.ldc_m = ldc_m; g.ldc_n = ldc_n; g.sC = sC; g.gdiv = gdiv;
    g.scale = scale; g.scale_div = scale_div; g.bias = bias; g.relu = act == CTI_ACT_RELU;
    return gemm_nt_f16f6(g, as_stream(stream));
}

extern "C" int cti_gemm_nt_f16f6_planes(const void* W_planes, int64_t rowsW_total, const void* X_planes, int64_t rowsX_total, void* Y_planes, size_t Y_bytes,
                                        int64_t batch_rows_out, int M, int N, int K, const float* bias, int act, void* stream) {
    CTI_REQUIRE_PTR(W_planes); CTI_REQUIRE_PTR(X_planes); CTI_REQUIRE_PTR(Y_planes);
    CTI_REQUIRE(M > 0 && N > 0 && K > 0 && M <= rowsW_total && N <= rowsX_total && batch_rows_out >= 0, CTI_E_SHAPE, "cti_gemm_nt_f16f6_planes: M=%d N=%d K=%d", M, N, K);
    CTI_REQUIRE(act == CTI_ACT_NONE || act == CTI_ACT_RELU, CTI_E_UNSUPPORTED, "cti_gemm_nt_f16f6_planes: act=%d", act);
    CTI_REQUIRE(Y_bytes >= f6_planes_bytes(N, M, batch_rows_out), CTI_E_WORKSPACE, "cti_gemm_nt_f16f6_planes: output block %zu < %zu", Y_bytes, f6_planes_bytes(N, M, batch_rows_out));
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(Y_planes) & 255) == 0, CTI_E_ALIGN, "cti_gemm_nt_f16f6_planes: the output block must be 256-B aligned");
    F6GemmArgs g{};
    g.A = f6_carve(const_cast<void*>(W_planes), rowsW_total, K, 0); g.B = f6_carve(const_cast<void*>(X_planes), rowsX_total, K, 0);
    const F6Planes out = f6_carve(Y_planes, N, M, batch_rows_out);
    g.nb = 1; g.M = M; g.N = N; g.epi = 6; g.out = &out;
    g.bias = bias; g.relu = act == CTI_ACT_RELU;
    return gemm_nt_f16f6(g, as_stream(stream));
}

extern "C" int cti_quantize_f16f6_scaled(const float* x, int64_t ld, int64_t rows, int K, int64_t batch_rows, const float* row_scale, int scale_div, void* planes,
                                         size_t planes_bytes, void* stream) {
    CTI_REQUIRE_PTR(x); CTI_REQUIRE_PTR(planes); CTI_REQUIRE_PTR(row_scale);
    CTI_REQUIRE(rows > 0 && K > 0 && ld >= K && batch_rows >= 0 && scale_div > 0, CTI_E_SHAPE, "cti_quantize_f16f6_scaled: rows=%lld K=%d ld=%lld batch_rows=%lld scale_div=%d", (long long)rows, K, (long long)ld, (long long)batch_rows, scale_div);
    CTI_REQUIRE(planes_bytes >= f6_planes_bytes(rows, K, batch_rows), CTI_E_WORKSPACE, "cti_quantize_f16f6_scaled: block %zu < %zu", planes_bytes, f6_planes_bytes(rows, K, batch_rows));
    CTI_REQUIRE((reinterpret_cast<uintptr_t>(planes) & 255) == 0, CTI_E_ALIGN, "cti_quantize_f16f6_scaled: the plane block must be 256-B aligned");
    hipError_t e = hipMemsetAsync(planes, 0, f6_planes_bytes(rows, K, batch_rows), as_stream(stream));
    if (e != hipSuccess) return fail((int)e, "cti_quantize_f16f6_scaled: hipMemsetAsync: %s", hipGetErrorString(e));
    return quantize_f16f6(x, ld, rows, K, f6_carve(planes, rows, K, batch_rows), as_stream(stream), row_scale, scale_div);
}
