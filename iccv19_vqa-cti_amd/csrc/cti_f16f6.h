// cti_f16f6.h -- the "f16f6" operand format and its device-side encoders (gfx950).
//
// WHY.  An fp32-grade product on the matrix cores needs the operands split into pieces the MFMA can multiply.  The bf16x3 mode
// (cti_gemm_bf16x3.hip) issues three bf16 MFMAs per product: a*b ~= ah*bh + ah*bl + al*bh.  Only the first term needs 8+ bits on
// BOTH sides; the two cross terms are corrections of relative size 2^-9 whose own precision requirement is a few bits.  gfx950 runs
// block-scaled fp6 (e2m3, 4 significant bits, one E8M0 scale per 32 elements) at FOUR times the 16-bit MFMA rate, so
//
//     a*b ~= a16*b16  +  fp6(a16)*fp6(b - b16)  +  fp6(a - a16)*fp6(b16)
//
// with a16 = f16(a) (11 significant bits; the residual is 2^-12 relative) costs 1 + 2 * 1/4 = 1.5 sixteen-bit-MFMA units per
// product instead of 3, at about the same accuracy as bf16x3 (residual 2^-12 times a 2^-4 rounding = 2^-16 per cross term;
// tools/emu_f16f6.py emulates it on the BASELINE configs[1] operands: 2.4e-5 normalised max error on the mode-3 GEMM against
// 6.7e-6 for bf16x3, tolerance 1e-4).  Measured on MI355X (tools/mb/mb_f16f6.hip, random operands in registers): 1003 algorithmic
// TFLOP/s against 550 for bf16x3.  Both cross terms of one 32-wide K block ride in ONE v_mfma_scale_f32_32x32x64_f8f6f4:
// its lanes 0-31 carry (A: fp6 of the hi part, B: fp6 of the lo part), lanes 32-63 carry (A: lo, B: hi), each with its own scale.
// The fp6 codes of the HI part never touch memory: the GEMM derives them from the f16 fragment it has just read (one
// v_cvt_scalef32_pk32_fp6_f16 per fragment, the SIMD-half partner's 16 codes fetched with v_permlane32_swap).
//
// PLANES of an operand X (rows x K), Kb = ceil(K / 32) blocks, block-major like the bf16 planes (one K block of a GEMM tile is a
// contiguous run of rows):
//   H   f16   [Kb][rows_alloc][32]      hi part, saturated to +-65504                        64 B per (row, block)
//   FL  e2m3  [Kb][rows_alloc][24 B]    fp6 codes of (x - H) / 2^el, position p at bits 6p of the row's six dwords, which are       24 B
//                                      STORED in the order [0 1 3 4 2 5]: a GEMM lane half reads dwords (0,1,2) or (3,4,5) as one aligned 8-B and one 4-B load
//   S   e8m0  [Kb][rows_allocS][2]      byte 0 = eh + 127, byte 1 = el + 127                  2 B     (2.81 B per element in all)
// eh / el are the smallest exponents with max|.| / 2^e <= 7.5 (the largest e2m3 value) over the block (eh: of the hi part, which the GEMM
// needs to derive its codes).  FL holds the block in the ORDER THE GEMM'S LANES MEET IT, position p <-> element k = F6_PI(p): a lane of the
// f16 MFMA holds k = 8h .. 8h+7 and 16+8h .. 16+8h+7 of a row (h = its SIMD half), so the derived hi codes of lane half 0 come as
// [0-7, 16-23 | 8-15, 24-31]; the lo codes they multiply must come in the same order.  rows_alloc = rows + 256 and rows_allocS = rows + 512
// (a GEMM tile may over-read that many rows; their contents only feed discarded outputs).
//
// DOMAIN.  f16 carries 5 exponent bits: the hi part is exact-to-11-bits for 6.1e-5 <= |x| <= 65504.  Smaller values degrade
// gracefully (absolute error <= 2^-29, the lo part picks up what the subnormal hi part drops); larger ones saturate in H and leave
// the excess to the 4-bit lo part.  Tensors whose significant magnitudes leave [2^-12, 65504] should use the bf16x3 mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cti {

constexpr int F6_BLK = 32;                       // K elements per scale block
constexpr int F6_SLACK_ROWS = 256;               // H / FL rows a tile may over-read
constexpr int F6_SLACK_ROWS_S = 512;             // S rows a tile may over-read (its DMA always moves 1 KiB = 512 rows of scales)

// Rows: a producer maps logical row m of its (flat) matrix to plane row (m / rdiv) * rstride + m % rdiv -- batches of rdiv rows start at
// multiples of rstride (a multiple of 8), because the GEMM's LDS-DMA reads 16 B per lane from batch_start * 24 B (codes) and
// batch_start * 2 B (scales): every tile origin must be a multiple of 8 rows.  rdiv = 0: identity (one batch).
constexpr int f6_pi(int p) { return (p >= 8 && p < 16) ? p + 8 : ((p >= 16 && p < 24) ? p - 8 : p); }   // position -> element (an involution)
struct F6Planes {
    _Float16* H; uint8_t* FL; uint8_t* S;
    int64_t rows_alloc, rows_allocS;           // multiples of 8
    int Kb;
    int64_t rdiv, rstride;
};
inline int64_t f6_round8(int64_t x) { return (x + 7) & ~(int64_t)7; }
// plane rows of a matrix of `rows` logical rows in batches of rdiv (0 = unbatched)
inline int64_t f6_plane_rows(int64_t rows, int64_t rdiv) { return rdiv > 0 ? (rows + rdiv - 1) / rdiv * f6_round8(rdiv) : rows; }
inline size_t f6_planes_bytes(int64_t rows, int K, int64_t rdiv = 0) {
    const size_t kb = (size_t)((K + F6_BLK - 1) / F6_BLK);
    const size_t pr = (size_t)f6_plane_rows(rows, rdiv);
    const size_t ra = (size_t)f6_round8(pr + F6_SLACK_ROWS), rs = (size_t)f6_round8(pr + F6_SLACK_ROWS_S);
    return kb * (ra * 64 + ra * 24 + rs * 2) + 3 * 256;
}
// carve the four planes out of one block (256-B aligned pieces); base may be NULL (sizes only)
inline F6Planes f6_carve(void* base, int64_t rows, int K, int64_t rdiv = 0) {
    F6Planes p{};
    p.Kb = (K + F6_BLK - 1) / F6_BLK;
    const int64_t pr = f6_plane_rows(rows, rdiv);
    p.rows_alloc = f6_round8(pr + F6_SLACK_ROWS); p.rows_allocS = f6_round8(pr + F6_SLACK_ROWS_S);
    p.rdiv = rdiv; p.rstride = rdiv > 0 ? f6_round8(rdiv) : 0;
    char* b = static_cast<char*>(base);
    size_t off = 0;
    auto take = [&](size_t n) { char* r = b ? b + off : nullptr; off = (off + n + 255) & ~(size_t)255; return r; };
    p.H = reinterpret_cast<_Float16*>(take((size_t)p.Kb * p.rows_alloc * 64));
    p.FL = reinterpret_cast<uint8_t*>(take((size_t)p.Kb * p.rows_alloc * 24));
    p.S = reinterpret_cast<uint8_t*>(take((size_t)p.Kb * p.rows_allocS * 2));
    return p;
}

#if defined(__HIPCC__)
__device__ __forceinline__ int64_t f6_prow(const F6Planes& p, int64_t m) { return p.rdiv > 0 ? (m / p.rdiv) * p.rstride + m % p.rdiv : m; }
// ---- device-side encoders -------------------------------------------------------------------------------------------
// exponent e (as E8M0 byte e + 127, clamped to [1, 254]) of the smallest power of two with m / 2^e <= 7.5;  m >= 0 finite
__device__ __forceinline__ int f6_scale_byte(float m) {
    const unsigned u = __builtin_bit_cast(unsigned, m);
    const int E = (int)((u >> 23) & 0xff);                 // biased exponent of m (0 for zero / subnormal)
    int byte = E - ((u & 0x7fffffu) > 0x700000u ? 1 : 2);  // m / 2^(E-127) in (1.875, 2) needs one binade more
    return byte < 1 ? 1 : (byte > 254 ? 254 : byte);
}
// 2^-(byte - 127) as a float (byte in [1, 254])
__device__ __forceinline__ float f6_inv_scale(int byte) { return __builtin_bit_cast(float, (unsigned)(254 - byte) << 23); }
// e2m3 code (6 bits: sign | 5-bit magnitude index) of y, |y| <= 7.5 expected (saturating); round to nearest even.
// The grid is monotone in the 5-bit index: 0..16 -> 0..2 in steps of 1/8, 16..24 -> 2..4 in steps of 1/4, 24..31 -> 4..7.5 in steps of 1/2.
__device__ __forceinline__ unsigned f6_code(float y) {
    const float ay = fabsf(y);
    float idx;
    if (ay < 2.f) idx = rintf(ay * 8.f);
    else if (ay < 4.f) idx = 16.f + rintf((ay - 2.f) * 4.f);
    else idx = fminf(24.f + rintf((ay - 4.f) * 2.f), 31.f);
    return (unsigned)idx | ((__builtin_bit_cast(unsigned, y) >> 26) & 32u);
}
__device__ __forceinline__ float f6_sat_f16(float x) { return fminf(fmaxf(x, -65504.f), 65504.f); }

#endif

// GEMM on f16f6 planes: C[z][m, n] = epilogue(sum_k A[z][m,k] B[z][n,k]); batches z < nb use rows [z*rA, +M) of A and [z*rB, +N) of B.
struct F6GemmArgs {
    F6Planes A, B;
    int64_t rA, rB;
    int nb, M, N;                              // K = 32 * A.Kb = 32 * B.Kb
    int epi;                                   // 0: fp32 C[z*sC + m*ldc_m + n*ldc_n] = act(scale[n / scale_div] * acc + bias[n])
                                               // 3: rows interleaved by gdiv (the mode-3 product: row m' = m*gdiv + g -> C[(m'/gdiv)*ldc_m + m'%gdiv + n*ldc_n])
    float* C; int64_t ldc_m, ldc_n, sC; int gdiv;
    const float* scale; int scale_div; const float* bias; int relu;
    // epi 3 with gdiv = 2 only, optional: softmax partials of the product (the Tri softmax of attention.py:55-58 runs over all of a
    // batch's outputs per g = m % 2).  Every wave of every tile writes (max, sum exp(x - max)) per g over its VALID outputs whose row is
    // not masked -- row m belongs to object m / sm_rows_per_obj, masked iff sm_mask[z * sm_objs + object] != 0 -- to
    // sm_part[((z * f6_sm_chunks(M, N) + chunk) * 2 + g) * 2 + {0, 1}]: the layout of the softmax's own partial pass.
    float* sm_part; const uint8_t* sm_mask; int sm_rows_per_obj, sm_objs;
    // epi 6 ("transposed planes"): the product is taken with the roles swapped -- A = the layer's weight (M = output features, a multiple of 32),
    // B = the activations (N = their rows) -- and act(acc + bias[m]) of column n is written as f16f6 planes of a (N rows x M features)
    // matrix: plane row f6_prow(*out, n), K block m / 32.  In that orientation a lane PAIR of the MFMA accumulator holds the 32 features of
    // one row's block, so the encoder runs in registers and the tile stream never pauses for LDS (cti_gemm_f16f6.hip).  The bias enters as
    // the accumulators' initial value; a weight-norm scale belongs in the weight planes (quantize_f16f6's row_scale).  nb = 1.
    const F6Planes* out;
    // epi 3 with gdiv = 2, ldc_n = 2 and no softmax partials only, optional: the tile plan of cti_mode3_plan.hip (device memory).  The kernel then walks the plan's
    // live tiles only -- their number is the plan's first word, read on the device -- instead of all nb x row tiles x column tiles.
    const unsigned* plan;
};
// ---- tile plan of the mode-3 product (cti_mode3_plan.hip).  The output rows of two objects of a sample with identical feature rows are identical, and the
// zero-padded objects that close a sample are exactly that: the product computes the row tiles that hold the sample's live objects and ONE padded object
// (the representative, object n_rep = the first of the trailing run of all-zero objects), and a periodic copy fills the rest of out[b] from the
// representative's block.  Words:  [M3P_W_*] head | per live row tile j (at most nb x row tiles) {sample, its first live row tile, its live row tiles, n_rep}
// | per sample {first live row tile, live row tiles, n_rep, 0}.
constexpr int M3P_HEAD_WORDS = 8, M3P_W_TILES = 0, M3P_W_ROW_TILES = 1, M3P_W_FILLED_ROWS = 2, M3P_W_SAMPLES = 3;
inline size_t mode3_plan_bytes(int64_t nb, int tiles_m) { return sizeof(unsigned) * (size_t)(M3P_HEAD_WORDS + 4 * nb * tiles_m + 4 * nb); }
int f6_mode3_tile_rows();                      // BM of the geometry gemm_nt_f16f6 launches the mode-3 product with
int f6_mode3_tile_cols();
// mask: (nb, V) bytes, 1 = all-zero object.  rows_per_obj GEMM rows per object, M = V * rows_per_obj, row tiles of bm rows, tiles_n column tiles
int mode3_plan(const uint8_t* mask, unsigned* plan, int nb, int V, int rows_per_obj, int bm, int tiles_n, hipStream_t st);
// out[b]: sample_floats floats, an object's block obj_floats, a row tile's rows tile_floats; fills [live row tiles x tile_floats, sample_floats) of every sample
int mode3_fill(const unsigned* plan, int tiles_m, float* out, int nb, int64_t sample_floats, int64_t obj_floats, int64_t tile_floats, hipStream_t st);
// ---- range guard (cti_f16f6_guard.hip): the guard block is GUARD_WORDS uint32 at the head of cti_tcnet_forward's workspace
constexpr int GUARD_WORDS = 64, GUARD_W_STATUS = 0, GUARD_W_DONE = 1, GUARD_W_RATIO = 2, GUARD_W_SEG = 4, GUARD_MAX_SEG = 12;
constexpr int GUARD_W_ABSMAX = 16, GUARD_W_DOTMAX = 17;      // guard_cancel: float bits of the largest sum_k |m_k a_k| / the largest |sum_k m_k a_k| over ALL batches' sampled pairs
struct GuardSeg {
    const void* p;                             // kind 0: an S plane ([Kb][rows_allocS][2 B]); kind 1: fp32 values
    int kind, Kb, slot;                        // slot: which word of the guard block collects this tensor's maximum
    int64_t rows_allocS, nb, rdiv, rstride, rows_total;   // kind 0: nb batches of rdiv real rows (rows_total in all) starting at multiples of rstride
    int64_t n;                                 // kind 1: element count
};
// One scan launch: its segments; `final`: the last workgroup evaluates slots [0, n_slots) (bit k of f32_slots: slot k is a non-finite flag)
struct GuardArgs { GuardSeg seg[GUARD_MAX_SEG]; int nseg; unsigned* words; int final, n_slots; unsigned f32_slots; float rho_bf16x3, rho_fp32; };   // rho_*: filled in by guard_scan (cti_set_tuning)
inline GuardSeg guard_seg_planes(const F6Planes& P, int64_t rows, int slot) {
    GuardSeg s{};
    s.p = P.S; s.kind = 0; s.Kb = P.Kb; s.rows_allocS = P.rows_allocS; s.slot = slot;
    if (P.rdiv > 0) { s.nb = (rows + P.rdiv - 1) / P.rdiv; s.rdiv = P.rdiv; s.rstride = P.rstride; s.rows_total = s.nb * P.rdiv; }
    else            { s.rdiv = s.rstride = 4096; s.nb = (rows + 4095) / 4096; s.rows_total = rows; }     // unbatched rows: virtual batches, so that many workgroups share a K block
    return s;
}
inline GuardSeg guard_seg_f32(const float* x, int64_t n, int slot) { GuardSeg s{}; s.p = x; s.kind = 1; s.n = n; s.slot = slot; return s; }
int guard_reset(unsigned* words, hipStream_t st);
int guard_scan(const GuardArgs& g, hipStream_t st);
int guard_poison(const unsigned* words, float* out, int64_t n, hipStream_t st);      // NaN-fills out when status & tuning_guard_poison_bits()
// Cancellation estimate of the mode-3 product (round 4): per batch, 32 x 32 sampled (row of M, row of A^) pairs from the f16 hi planes ->
// rho = max over ALL batches' pairs of sum_k |m_k a_k|  /  max over ALL batches' pairs of |sum_k m_k a_k|  (words GUARD_W_ABSMAX / _DOTMAX, float bits, atomicMax;
// the verdict kernel forms the quotient into GUARD_W_RATIO).  Round 5: numerator and denominator are maxima over the whole call, as the tolerance is -- 1e-4 of the
// LARGEST output of the tensor; round 4 took the largest PER-BATCH quotient, whose denominator rests on 1 024 pairs: over 256 batches the unluckiest one read
// 3.2-3.5 on the bench inputs where two batches read 1.9.
// Measured at the BASELINE configs[1] widths against the float64 oracle (tests/test_accuracy_envelope_gpu.py): the whole TCNet.forward's error
// normalised by the largest output is ~1e-5 rho in the f16f6 mode (rho 2-4 on the synthetic tensors: 2.7e-5), ~4e-6 rho as bf16x3 (the
// operands M and A^ carry their own 2^-17 relative errors, which a cancelling sum amplifies just the same), ~5e-8 rho in exact fp32.  The final
// guard scan turns rho into CTI_GUARD_CANCEL (f16f6 -> bf16x3) / CTI_GUARD_CANCEL_HEAVY (-> fp32) at the thresholds of cti_set_tuning (CTI_TUNE_GUARD_RHO_*:
// 2.75 / 5.5 by default: a factor two under 1e-4 on the measured laws ~1.8e-5 rho (f16f6) / ~0.9e-5 rho (bf16x3); round 4's 10 / 20 left no margin).  A no-op (rho 0) when K > 1024.
int guard_cancel(const F6Planes& M, int64_t mrows, const F6Planes& A, int64_t arows, int nb, unsigned* words, hipStream_t st);

int f6_sm_chunks(int M, int N);                // partial (max, sum) pairs per batch and g that gemm_nt_f16f6 writes for an M x N product
int gemm_nt_f16f6(const F6GemmArgs& a, hipStream_t st);
// row_scale != NULL: row m is multiplied by row_scale[m / scale_div] on the way in (a weight-normalised layer's g / ||V|| per matrix)
int quantize_f16f6(const float* x, int64_t ld, int64_t rows, int K, const F6Planes& p, hipStream_t st, const float* row_scale = nullptr, int scale_div = 1);
#if defined(__HIPCC__)
// Encode and store one (row, block) whose 32 fp32 values sit in LDS (16-B aligned, contiguous) -- the form GEMM epilogues and the encoder
// kernel use: two streaming passes over the LDS copy instead of 32 + 32 + 32 live registers (pass 1: f16 hi part stored 8 values at a time,
// block maxima; then the lo codes from the hardware converter, in the f6_pi order).  Same codes, value for value, as f6_code.
typedef float f6_f32x4 __attribute__((ext_vector_type(4)));       // LDS reads as plain vectors (a HIP float4 struct read drains vmcnt(0))
typedef float f6_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned f6_u32x6 __attribute__((ext_vector_type(6)));
// 32 fp32 values -> 32 e2m3 codes (6 dwords) of x / 2^floor(log2 scale) in ONE instruction: v_cvt_scalef32_2xpk16_fp6_f32 takes the even
// elements in its first source and the odd ones in its second (code 2i <- a[i], code 2i+1 <- b[i]); round-to-nearest-even and saturation
// at 7.5 agree code for code with f6_code (tools/mb/mb_cvt6.hip).  Inline asm with an EARLY-CLOBBER destination: hipcc's builtin of the
// same name lets the 6-register destination overlap the sources, and the instruction then reads operands it has already overwritten.
__device__ __forceinline__ f6_u32x6 f6_hw_codes(const f6_f32x16 even, const f6_f32x16 odd, float scale) {
    f6_u32x6 r;
    asm volatile("v_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, %3" : "=&v"(r) : "v"(even), "v"(odd), "v"(scale));
    return r;
}
__device__ __forceinline__ void f6_encode_row32_lds(const float* src, const F6Planes& p, int64_t prow, int kb) {
    const int64_t o = (int64_t)kb * p.rows_alloc + prow;
    uint4* hd = reinterpret_cast<uint4*>(p.H + o * 32);
    float mh = 0.f, ml = 0.f;
    float lf[32];                                              // residuals, element order
#pragma unroll
    for (int q8 = 0; q8 < 4; ++q8) {
        const f6_f32x4 a = *reinterpret_cast<const f6_f32x4*>(src + q8 * 8), b = *reinterpret_cast<const f6_f32x4*>(src + q8 * 8 + 4);
        const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        _Float16 h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            h[u] = static_cast<_Float16>(f6_sat_f16(x[u]));
            const float hf = static_cast<float>(h[u]);
            lf[q8 * 8 + u] = x[u] - hf;
            mh = fmaxf(mh, fabsf(hf)); ml = fmaxf(ml, fabsf(lf[q8 * 8 + u]));
        }
        hd[q8] = *reinterpret_cast<const uint4*>(h);
    }
    if (!(ml < 3.0e38f)) ml = 0.f;
    if (!(mh < 3.0e38f)) mh = 65504.f;
    const int sh = f6_scale_byte(mh), sl = f6_scale_byte(ml);
    f6_f32x16 le, lo;                                          // the converter's two sources: positions 2i and 2i + 1, element f6_pi(position)
#pragma unroll
    for (int i = 0; i < 16; ++i) { le[i] = lf[f6_pi(2 * i)]; lo[i] = lf[f6_pi(2 * i + 1)]; }
    const f6_u32x6 fl = f6_hw_codes(le, lo, __builtin_bit_cast(float, (unsigned)sl << 23));     // 2^(byte - 127)
    uint2* fd = reinterpret_cast<uint2*>(p.FL + o * 24);
    fd[0] = make_uint2(fl[0], fl[1]); fd[1] = make_uint2(fl[3], fl[4]); fd[2] = make_uint2(fl[2], fl[5]);     // dword order [0 1 3 4 2 5]: see the format notes
    *reinterpret_cast<unsigned short*>(p.S + ((int64_t)kb * p.rows_allocS + prow) * 2) = (unsigned short)(sh | (sl << 8));
}
// The same (row, block) item from 32 values a lane holds in registers (element order) -- the register-only epilogue of the transposed
// f16f6 GEMM -- with max(x, lo_bound) applied first (lo_bound = 0: ReLU; -inf: none).  Same planes, bit for bit, as f6_encode_row32_lds on
// max(x, lo_bound), in ~4 VALU instructions per element: v_med3_f32 (lower bound and f16 saturation in one), v_cvt_pk_f16_f32 (gfx950: two
// values per instruction, round to nearest even), the residual as a packed fp32 subtraction, both maxima as v_max3 with |.| modifiers.  A block that holds a saturated value (|x| >= 65504, outside the format's domain) recomputes its residuals from the
// unsaturated values in a rarely taken branch.  Plain vector stores (no HIP structs): nothing here may alias the GEMM's LDS-DMA ring,
// which stays in flight around it.
typedef unsigned f6_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned f6_u32x2 __attribute__((ext_vector_type(2)));
typedef float f6_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f6_f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short f6_u16x2 __attribute__((ext_vector_type(2)));
#ifndef CTI_F6_ABL
#define CTI_F6_ABL 0
#endif
// SAT_EXCESS = false drops that branch (a saturated value then decodes to +-65504): for callers at their register ceiling -- the branch keeps
// all 32 inputs and the 16 packed hi words alive to the end.
typedef __attribute__((address_space(3))) f6_u32x4 f6_lds_u32x4;
// h_lds != NULL (round 6, the M build): the row's four H pieces go to that LDS address (consecutive 16-B units) instead of Hrow -- the caller re-reads them so that four
// lanes store one row's 64 B (a lane storing its own row's pieces makes every store instruction touch 64 cache lines)
template <bool SAT_EXCESS = true>
__device__ __forceinline__ void f6_encode_row32_regs(const float (&x)[32], float lo_bound, char* Hrow, char* FLrow, char* Srow, int hstep = 1, f6_lds_u32x4* h_lds = nullptr) {      // hstep: 16-B units between the row's four H pieces (1 = the row as it lies in the plane; timing experiments only otherwise)
    if ((CTI_F6_ABL & 16) && x[31] != 12345.f) { Hrow = FLrow = Srow = nullptr; }      // timing-only ablation: the arithmetic without the stores
    const float lo_sat = fmaxf(lo_bound, -65504.f);
    float ml = 0.f, mx = 0.f;                                       // mx: max |hi part|
    float lf[32];
    unsigned hw[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        f6_f32x2 v = {__builtin_amdgcn_fmed3f(x[2 * u], lo_sat, 65504.f), __builtin_amdgcn_fmed3f(x[2 * u + 1], lo_sat, 65504.f)};
        const f6_f16x2 h = __builtin_convertvector(v, f6_f16x2);
        const f6_f32x2 hf = __builtin_convertvector(h, f6_f32x2);
        const f6_f32x2 l = v - hf;
        lf[2 * u] = l[0]; lf[2 * u + 1] = l[1];
        ml = fmaxf(fmaxf(ml, fabsf(l[0])), fabsf(l[1]));            // (this nesting becomes ONE v_max3_f32 with |.| modifiers)
        if (SAT_EXCESS) mx = fmaxf(fmaxf(mx, fabsf(hf[0])), fabsf(hf[1]));
        else            mx = fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1])));   // (of the inputs: rounding is monotone; frees the converted pair earlier -- the M build's ceiling)
        hw[u] = __builtin_bit_cast(unsigned, h);
        if ((u & 3) == 3 && h_lds) h_lds[u >> 2] = f6_u32x4{hw[u - 3], hw[u - 2], hw[u - 1], hw[u]};
        else if ((u & 3) == 3 && (!(CTI_F6_ABL & 16) || Hrow)) reinterpret_cast<f6_u32x4*>(Hrow)[(u >> 2) * hstep] = f6_u32x4{hw[u - 3], hw[u - 2], hw[u - 1], hw[u]};
    }
    const float mh = SAT_EXCESS ? mx : static_cast<float>(static_cast<_Float16>(mx));
    if (SAT_EXCESS && mh >= 65504.f) {                                          // a saturated value: its residual carries the excess (as the LDS encoder has it)
        ml = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const f6_f32x2 hf = __builtin_convertvector(__builtin_bit_cast(f6_f16x2, hw[u]), f6_f32x2);
            lf[2 * u] = fmaxf(x[2 * u], lo_bound) - hf[0]; lf[2 * u + 1] = fmaxf(x[2 * u + 1], lo_bound) - hf[1];
            ml = fmaxf(ml, fmaxf(fabsf(lf[2 * u]), fabsf(lf[2 * u + 1])));
        }
        if (!(ml < 3.0e38f)) ml = 0.f;
    }
    const int sh = f6_scale_byte(mh), sl = f6_scale_byte(ml);
    f6_f32x16 le, lo;
#pragma unroll
    for (int i = 0; i < 16; ++i) { le[i] = lf[f6_pi(2 * i)]; lo[i] = lf[f6_pi(2 * i + 1)]; }
    const f6_u32x6 fl = f6_hw_codes(le, lo, __builtin_bit_cast(float, (unsigned)sl << 23));
    if ((CTI_F6_ABL & 16) && !Hrow) { if (fl[0] == 0x12345u && sh == 77) *reinterpret_cast<volatile unsigned*>(16) = fl[5] + sl; return; }
    f6_u32x2* fd = reinterpret_cast<f6_u32x2*>(FLrow);
    fd[0] = f6_u32x2{fl[0], fl[1]}; fd[1] = f6_u32x2{fl[3], fl[4]}; fd[2] = f6_u32x2{fl[2], fl[5]};
    *reinterpret_cast<unsigned short*>(Srow) = (unsigned short)(sh | (sl << 8));
}
#endif

}  // namespace cti
