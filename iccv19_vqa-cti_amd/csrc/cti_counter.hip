// cti_counter.hip -- the counting module (src/counting.py:30-145, Zhang et al. ICLR 2018) as the BAN models call it (src/FFOE/base_model.py:56-58),
// one workgroup per row, a row being one (sample, glimpse) pair.
//
// Forward, per row (m = objects, n = 16 segments, f_0 .. f_7 the piecewise-linear functions):
//     s_v        = max_q logits[v, q]  (and the position of that maximum)              the models' `logits[:, g].max(2)`; Q = 1: the plain module call
//     top m of s over the V boxes; ties go to the LOWER box index (keys (s, -v) are distinct, so the selection is a total order: m rounds of a
//                  workgroup-wide maximum below the previous round's key; the result is sorted by score, which no later stage depends on)
//     a_i        = sigmoid(s_i)  (s_i itself when already_sigmoided);  the m boxes gathered from the strided (B, 4, V) view
//     r_ij = a_i a_j;   d_ij = 1 - IoU(box_i, box_j)  (the reference's 1e-12 in the denominator)
//     X_ij       = f3(r_ij) f4(d_ij)                                                    dedup_score
//     sim_ij     = f2(1 - |a_i - a_j|) prod_k f2(1 - |X_ki - X_kj|);   rs_i = sum_j sim_ij
//     S          = sum_ij f0(r_ij) f1(d_ij) / (rs_i rs_j) + sum_i f0(a_i^2) / rs_i;   sq = sqrt(S + 1e-20)
//     conf       = f7(mean_i |f5(a_i) - 1/2| + mean_i mean_j |f6(d_ij) - 1/2|)
//     out[k]     = conf * ((1 - frac) [k == min(i0, m)] + frac [k == min(i0 + 1, m)]),   i0 = trunc(clamp(sq, 0, m)), frac = its fractional part
// f(x) from the raw weights w (n + 1 of them), for ANY weights: wn = |w| / sum |w|, cs = running sum of wn, y = n x, i = trunc(y),
//     f(x) = cs[min(i, n)] + (y - i) wn[min(i + 1, n)]
// (an x outside [0, 1] -- already_sigmoided with an attention that is not -- indexes cs[0] / cs[n] instead of failing as the reference's gather does).
// A thread per (i, j) pair (m <= 16: 256 threads), every matrix in LDS, every sum in a fixed order.
//
// Backward: the forward is recomputed from the save block (selected indices, arg-max positions, a_i) with the m^3 factors of the product kept
// in LDS, then reversed by hand with autograd's conventions at the kinks: |x|' = sign(x) (0 at 0), clamp passes the gradient on its bounds,
// frac' = 1, trunc / gathers by index pass nothing, the gradient of a factor of the product is the product of the OTHER m - 1 factors (no
// division).  Boxes get no gradient, so d_ij only feeds the weights of f1, f4, f6.  Every evaluation f(x) that received a gradient g adds g to
// bin min(i, n) of d cs and g frac to bin min(i + 1, n) of d wn; the evaluations of a function are binned slab by slab (256 at a time) by
// 15 x 17 threads, each over a fixed range in a fixed order, and the 15 partial histograms are summed in order: no atomics, bitwise
// reproducible.  d wn -> d w through the normalisation and |.|.  The weight gradients leave as per-row partials (rows, 8, n + 1), reduced
// over the rows by the caller (cti_col_sum); the logit gradient is written densely: zero except at (selected box, its arg-max position).
#include "cti_common.h"

#include <math.h>

namespace cti {
namespace {

constexpr int CNT_THREADS = 256;
constexpr int CNT_MAXM = 16;              // objects <= 16: m^2 <= the workgroup's threads
constexpr int CNT_N = 16;                 // segments of a piecewise-linear function (what Counter constructs)
constexpr int CNT_NW = CNT_N + 1;
constexpr int CNT_F = 8;
constexpr int CNT_SAVE_WORDS = 3 * CNT_MAXM;      // per row: int idx[16], int amax[16], float a[16]
constexpr int CNT_CHUNKS = 15;            // 15 x 17 = 255 threads bin a slab of evaluations
constexpr int CNT_MAX_V = 8192;           // the forward keeps one key per box in (dynamic) LDS

struct CntWeights { const float* w[CNT_F]; };

struct CntShared {
    float wn[CNT_F][CNT_NW], cs[CNT_F][CNT_NW], wsum[CNT_F];
    float a[CNT_MAXM], box[4][CNT_MAXM], area[CNT_MAXM];
    int idx[CNT_MAXM], amax[CNT_MAXM];
    float X[256], P[256], sim[256], score[256], c6[256];
    float rs[CNT_MAXM], corr[CNT_MAXM], rowsum[CNT_MAXM], row6[CNT_MAXM], a5[CNT_MAXM];
    float sq, conf, c;
    unsigned red_hi[CNT_THREADS / 64], red_lo[CNT_THREADS / 64];
};

struct Pw { float val, slope, frac; int i0, i1; };

__device__ __forceinline__ Pw pw_eval(const float* wn, const float* cs, float x) {
    const float y = (float)CNT_N * x;
    const float t = truncf(y);
    Pw r;
    r.frac = y - t;
    r.i0 = (int)fminf(fmaxf(t, 0.f), (float)CNT_N);          // (NaN -> 0: always a valid index)
    r.i1 = min(r.i0 + 1, CNT_N);
    r.val = cs[r.i0] + r.frac * wn[r.i1];
    r.slope = (float)CNT_N * wn[r.i1];
    return r;
}

__device__ __forceinline__ float sgn(float x) { return (float)(x > 0.f) - (float)(x < 0.f); }

// |w| / sum |w| and its running sum for the eight functions (threads 0 .. 8 * 17 - 1; two barriers)
__device__ __forceinline__ void cnt_load_weights(CntShared& sh, const CntWeights& W, int tid) {
    const int f = tid / CNT_NW, l = tid - f * CNT_NW;
    if (tid < CNT_F * CNT_NW) sh.wn[f][l] = fabsf(W.w[f][l]);
    __syncthreads();
    float wl = 0.f, run = 0.f;
    if (tid < CNT_F * CNT_NW) {
        float T = 0.f;
        for (int k = 0; k < CNT_NW; ++k) T += sh.wn[f][k];
        for (int k = 0; k <= l; ++k) run += sh.wn[f][k] / T;
        wl = sh.wn[f][l] / T;
        if (l == 0) sh.wsum[f] = T;
    }
    __syncthreads();
    if (tid < CNT_F * CNT_NW) { sh.wn[f][l] = wl; sh.cs[f][l] = run; }
    __syncthreads();
}

// Everything of the forward behind the selection: sh.a / sh.box are set.  cube != nullptr: the factors f2(1 - |X_ki - X_kj|) are kept at
// cube[k * 256 + p] for the backward.  Leaves r, d of this thread's pair; sh.sq, sh.conf, sh.c and the matrices for the caller.
__device__ __forceinline__ void cnt_core(CntShared& sh, int m, int tid, float* cube, float& r_out, float& d_out) {
    const int mm = m * m;
    const bool pair = tid < mm;
    const int i = pair ? tid / m : 0, j = pair ? tid - i * m : 0;
    if (tid < m) sh.area[tid] = fmaxf(sh.box[2][tid] - sh.box[0][tid], 0.f) * fmaxf(sh.box[3][tid] - sh.box[1][tid], 0.f);
    __syncthreads();
    const float ai = sh.a[i], aj = sh.a[j];
    const float r = ai * aj;
    const float ix = fmaxf(fminf(sh.box[2][i], sh.box[2][j]) - fmaxf(sh.box[0][i], sh.box[0][j]), 0.f);
    const float iy = fmaxf(fminf(sh.box[3][i], sh.box[3][j]) - fmaxf(sh.box[1][i], sh.box[1][j]), 0.f);
    const float inter = ix * iy;
    const float d = 1.f - inter / (sh.area[i] + sh.area[j] - inter + 1e-12f);
    r_out = r; d_out = d;
    float A = 0.f;
    if (pair) {
        sh.X[tid] = pw_eval(sh.wn[3], sh.cs[3], r).val * pw_eval(sh.wn[4], sh.cs[4], d).val;
        A = pw_eval(sh.wn[0], sh.cs[0], r).val * pw_eval(sh.wn[1], sh.cs[1], d).val;
        sh.c6[tid] = fabsf(pw_eval(sh.wn[6], sh.cs[6], d).val - 0.5f);
    }
    __syncthreads();
    if (pair) {
        float P = 1.f;
        for (int k = 0; k < m; ++k) {
            const float F = pw_eval(sh.wn[2], sh.cs[2], 1.f - fabsf(sh.X[k * m + i] - sh.X[k * m + j])).val;
            if (cube) cube[k * 256 + tid] = F;
            P *= F;
        }
        sh.P[tid] = P;
        sh.sim[tid] = P * pw_eval(sh.wn[2], sh.cs[2], 1.f - fabsf(ai - aj)).val;
    }
    __syncthreads();
    if (tid < m) {
        float t = 0.f;
        for (int k = 0; k < m; ++k) t += sh.sim[tid * m + k];
        sh.rs[tid] = t;
        sh.corr[tid] = pw_eval(sh.wn[0], sh.cs[0], sh.a[tid] * sh.a[tid]).val / t;
        sh.a5[tid] = fabsf(pw_eval(sh.wn[5], sh.cs[5], sh.a[tid]).val - 0.5f);
    }
    __syncthreads();
    if (pair) sh.score[tid] = A / (sh.rs[i] * sh.rs[j]);
    __syncthreads();
    if (tid < m) {
        float t = 0.f, u = 0.f;
        for (int k = 0; k < m; ++k) { t += sh.score[tid * m + k]; u += sh.c6[tid * m + k]; }
        sh.rowsum[tid] = t;
        sh.row6[tid] = u / (float)m;
    }
    __syncthreads();
    if (tid == 0) {
        float S = 0.f, C = 0.f, ma = 0.f, md = 0.f;
        for (int k = 0; k < m; ++k) { S += sh.rowsum[k]; C += sh.corr[k]; ma += sh.a5[k]; md += sh.row6[k]; }
        sh.sq = sqrtf(S + C + 1e-20f);
        sh.c = ma / (float)m + md / (float)m;
        sh.conf = pw_eval(sh.wn[7], sh.cs[7], sh.c).val;
    }
    __syncthreads();
}

// to_one_hot's support: clamp(sq, 0, m) -> (il, ir, frac)
__device__ __forceinline__ void cnt_one_hot(float sq, int m, int& il, int& ir, float& fr) {
    const float sc = fminf(fmaxf(sq, 0.f), (float)m);
    const float t = truncf(sc);
    fr = sc - t;
    const int i0 = (int)t;
    il = min(i0, m); ir = min(i0 + 1, m);
}

__device__ __forceinline__ unsigned score_key(float x) {        // order-preserving float -> uint (NaN above +inf, as torch.topk ranks it; -0 = +0)
    const unsigned u = __float_as_uint(x + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(CNT_THREADS) void counter_fwd_kernel(const float* __restrict__ logits, int64_t sLb, int64_t sLg, int64_t sLv, int64_t sLq,
                                                                const float* __restrict__ boxes, int64_t sBb, int64_t sBc, int64_t sBv, CntWeights W, int sigm,
                                                                float* __restrict__ out, int64_t sOb, int64_t sOg, int* __restrict__ save, int G, int V, int Q,
                                                                int m) {
    __shared__ CntShared sh;
    extern __shared__ unsigned keys[];                              // V keys
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = row / G, g = row - b * G;
    const float* L = logits + (int64_t)b * sLb + (int64_t)g * sLg;
    cnt_load_weights(sh, W, tid);

    // 1. s_v = max_q (the first maximum's position is recomputed for the selected boxes below)
    for (int v = tid; v < V; v += CNT_THREADS) {
        float best = L[(int64_t)v * sLv];
        for (int q = 1; q < Q; ++q) {
            const float x = L[(int64_t)v * sLv + (int64_t)q * sLq];
            if (x > best || (x != x && best == best)) best = x;
        }
        keys[v] = score_key(best);
    }
    __syncthreads();

    // 2. m rounds: the largest (key, -v) below the previous round's
    unsigned phi = 0xffffffffu, plo = 0xffffffffu;
    for (int round = 0; round < m; ++round) {
        unsigned bhi = 0u, blo = 0u;                               // (0, 0) = nothing: every real candidate has lo = ~v >= 0xffffffff - 8191 > 0
        for (int v = tid; v < V; v += CNT_THREADS) {
            const unsigned khi = keys[v], klo = 0xffffffffu - (unsigned)v;
            const bool below = round == 0 || khi < phi || (khi == phi && klo < plo);
            const bool above = khi > bhi || (khi == bhi && klo > blo);
            if (below && above) { bhi = khi; blo = klo; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned ohi = (unsigned)__shfl_xor((int)bhi, o, 64), olo = (unsigned)__shfl_xor((int)blo, o, 64);
            if (ohi > bhi || (ohi == bhi && olo > blo)) { bhi = ohi; blo = olo; }
        }
        if (lane == 0) { sh.red_hi[wv] = bhi; sh.red_lo[wv] = blo; }
        __syncthreads();
        bhi = sh.red_hi[0]; blo = sh.red_lo[0];
        for (int w = 1; w < CNT_THREADS / 64; ++w) {
            const unsigned ohi = sh.red_hi[w], olo = sh.red_lo[w];
            if (ohi > bhi || (ohi == bhi && olo > blo)) { bhi = ohi; blo = olo; }
        }
        phi = bhi; plo = blo;
        if (tid == 0) sh.idx[round] = min((int)(0xffffffffu - blo), V - 1);      // (V >= m: a candidate always exists; the clamp only guards the index)
        __syncthreads();
    }

    // 3. the selected boxes: score, arg-max position, sigmoid, box gather; the save block
    if (tid < m) {
        const int v = sh.idx[tid];
        float best = L[(int64_t)v * sLv];
        int bq = 0;
        for (int q = 1; q < Q; ++q) {
            const float x = L[(int64_t)v * sLv + (int64_t)q * sLq];
            if (x > best || (x != x && best == best)) { best = x; bq = q; }
        }
        const float a = sigm ? 1.f / (1.f + expf(-best)) : best;
        sh.a[tid] = a;
        sh.amax[tid] = bq;
        const float* bx = boxes + (int64_t)b * sBb + (int64_t)v * sBv;
#pragma unroll
        for (int c = 0; c < 4; ++c) sh.box[c][tid] = bx[(int64_t)c * sBc];
        int* sv = save + (int64_t)row * CNT_SAVE_WORDS;
        sv[tid] = v;
        sv[CNT_MAXM + tid] = bq;
        sv[2 * CNT_MAXM + tid] = __float_as_int(a);
    } else if (tid < CNT_MAXM) {                                     // (the unused slots: a defined save block)
        int* sv = save + (int64_t)row * CNT_SAVE_WORDS;
        sv[tid] = 0; sv[CNT_MAXM + tid] = 0; sv[2 * CNT_MAXM + tid] = 0;
    }
    __syncthreads();

    float r, d;
    cnt_core(sh, m, tid, nullptr, r, d);
    if (tid <= m) {
        int il, ir; float fr;
        cnt_one_hot(sh.sq, m, il, ir, fr);
        out[(int64_t)b * sOb + (int64_t)g * sOg + tid] = sh.conf * ((tid == il ? 1.f - fr : 0.f) + (tid == ir ? fr : 0.f));
    }
}

struct CntBwdShared {
    float cube[CNT_MAXM * 256];
    int ebin[256];
    float eg[256], egf[256];
    float T[256], dX[256];
    float part[CNT_CHUNKS][CNT_NW][2];
    float hist[CNT_F][2][CNT_NW];                 // [f][0] = d cs, [f][1] = d wn (direct)
    float da[CNT_MAXM], drs[CNT_MAXM];
    float dS, dc, dconf;
};

// one evaluation's entry of the current slab (g = 0: none)
__device__ __forceinline__ void cnt_entry(CntBwdShared& bs, int tid, const Pw& e, float g) {
    bs.ebin[tid] = e.i0; bs.eg[tid] = g; bs.egf[tid] = g * e.frac;
}

// bin the slab's `count` entries: thread (chunk, bin) over a fixed range in order (between two barriers of the caller)
__device__ __forceinline__ void cnt_scan(const CntBwdShared& bs, int tid, int count, float& acc_cs, float& acc_w) {
    if (tid >= CNT_CHUNKS * CNT_NW) return;
    const int ch = tid / CNT_NW, bin = tid - ch * CNT_NW;
    const int per = (count + CNT_CHUNKS - 1) / CNT_CHUNKS;
    const int e0 = ch * per, e1 = min(e0 + per, count);
    for (int e = e0; e < e1; ++e) {
        const int b0 = bs.ebin[e];
        acc_cs += b0 == bin ? bs.eg[e] : 0.f;
        acc_w += min(b0 + 1, CNT_N) == bin ? bs.egf[e] : 0.f;
    }
}

// the 15 partial histograms of function f summed in chunk order (three barriers; the accumulators restart)
__device__ __forceinline__ void cnt_flush(CntBwdShared& bs, int tid, int f, float& acc_cs, float& acc_w) {
    if (tid < CNT_CHUNKS * CNT_NW) {
        const int ch = tid / CNT_NW, bin = tid - ch * CNT_NW;
        bs.part[ch][bin][0] = acc_cs; bs.part[ch][bin][1] = acc_w;
    }
    acc_cs = 0.f; acc_w = 0.f;
    __syncthreads();
    if (tid < 2 * CNT_NW) {
        const int which = tid / CNT_NW, bin = tid - which * CNT_NW;
        float t = 0.f;
        for (int ch = 0; ch < CNT_CHUNKS; ++ch) t += bs.part[ch][bin][which];
        bs.hist[f][which][bin] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(CNT_THREADS) void counter_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ boxes, int64_t sBb, int64_t sBc, int64_t sBv,
                                                                CntWeights W, int sigm, const int* __restrict__ save, float* __restrict__ dlogits,
                                                                float* __restrict__ dw_part, int G, int V, int Q, int m) {
    __shared__ CntShared sh;
    __shared__ CntBwdShared bs;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int b = row / G;
    const int mm = m * m;
    const bool pair = tid < mm;
    const int i = pair ? tid / m : 0, j = pair ? tid - i * m : 0;
    cnt_load_weights(sh, W, tid);
    if (tid < m) {
        const int* sv = save + (int64_t)row * CNT_SAVE_WORDS;
        const int v = min(max(sv[tid], 0), V - 1);                 // (a damaged save block must not become a wild address)
        sh.idx[tid] = v;
        sh.amax[tid] = min(max(sv[CNT_MAXM + tid], 0), Q - 1);
        sh.a[tid] = __int_as_float(sv[2 * CNT_MAXM + tid]);
        const float* bx = boxes + (int64_t)b * sBb + (int64_t)v * sBv;
#pragma unroll
        for (int c = 0; c < 4; ++c) sh.box[c][tid] = bx[(int64_t)c * sBc];
    }
    __syncthreads();
    float r, d;
    cnt_core(sh, m, tid, bs.cube, r, d);
    const float fm = (float)m;
    float acc_cs = 0.f, acc_w = 0.f;

    // out = one_hot(sq) conf
    if (tid == 0) {
        int il, ir; float fr;
        cnt_one_hot(sh.sq, m, il, ir, fr);
        const float* g = dout + (int64_t)row * (m + 1);
        const float dconf = g[il] * (il == ir ? 1.f : 1.f - fr) + (il == ir ? 0.f : g[ir] * fr);      // sum_k g_k one_hot_k
        const float dfr = (g[ir] - g[il]) * sh.conf;
        const float dsq = (sh.sq >= 0.f && sh.sq <= fm) ? dfr : 0.f;
        bs.dS = dsq / (2.f * sh.sq);
        const Pw e7 = pw_eval(sh.wn[7], sh.cs[7], sh.c);
        bs.dc = dconf * e7.slope;
        bs.dconf = dconf;
        cnt_entry(bs, 0, e7, dconf);
    }
    __syncthreads();
    const float dS = bs.dS, dc = bs.dc;
    cnt_scan(bs, tid, 1, acc_cs, acc_w);
    __syncthreads();
    cnt_flush(bs, tid, 7, acc_cs, acc_w);

    // f5: mean_i |f5(a_i) - 1/2|
    if (tid < m) {
        const Pw e5 = pw_eval(sh.wn[5], sh.cs[5], sh.a[tid]);
        const float g5 = dc / fm * sgn(e5.val - 0.5f);
        cnt_entry(bs, tid, e5, g5);
        bs.da[tid] = g5 * e5.slope;
    }
    __syncthreads();
    cnt_scan(bs, tid, m, acc_cs, acc_w);
    __syncthreads();
    cnt_flush(bs, tid, 5, acc_cs, acc_w);

    // f6: mean_i mean_j |f6(d_ij) - 1/2|
    if (pair) {
        const Pw e6 = pw_eval(sh.wn[6], sh.cs[6], d);
        cnt_entry(bs, tid, e6, dc / (fm * fm) * sgn(e6.val - 0.5f));
    }
    __syncthreads();
    cnt_scan(bs, tid, mm, acc_cs, acc_w);
    __syncthreads();
    cnt_flush(bs, tid, 6, acc_cs, acc_w);

    // f0 f1 / (rs_i rs_j) and f0(a_i^2) / rs_i
    const Pw e0 = pw_eval(sh.wn[0], sh.cs[0], r), e1 = pw_eval(sh.wn[1], sh.cs[1], d);
    const float dA = dS / (sh.rs[i] * sh.rs[j]);
    float dr = dA * e1.val * e0.slope;
    if (pair) cnt_entry(bs, tid, e0, dA * e1.val);
    __syncthreads();
    cnt_scan(bs, tid, mm, acc_cs, acc_w);
    __syncthreads();
    if (tid < m) {
        const float a = sh.a[tid];
        const Pw ed = pw_eval(sh.wn[0], sh.cs[0], a * a);
        const float gd = dS / sh.rs[tid];
        cnt_entry(bs, tid, ed, gd);
        bs.da[tid] += gd * ed.slope * 2.f * a;
        float col = 0.f;
        for (int k = 0; k < m; ++k) col += sh.score[k * m + tid];
        bs.drs[tid] = -(dS / sh.rs[tid]) * (sh.rowsum[tid] + col + sh.corr[tid]);
    }
    __syncthreads();
    cnt_scan(bs, tid, m, acc_cs, acc_w);
    __syncthreads();
    cnt_flush(bs, tid, 0, acc_cs, acc_w);
    if (pair) cnt_entry(bs, tid, e1, dA * e0.val);
    __syncthreads();
    cnt_scan(bs, tid, mm, acc_cs, acc_w);
    __syncthreads();
    cnt_flush(bs, tid, 1, acc_cs, acc_w);

    // sim_ij = P_ij f2(1 - |a_i - a_j|),  rs_i = sum_j sim_ij
    const float dsim = bs.drs[i];
    float dP = 0.f;
    if (pair) {
        const float ai = sh.a[i], aj = sh.a[j];
        const Pw eA = pw_eval(sh.wn[2], sh.cs[2], 1.f - fabsf(ai - aj));
        dP = dsim * eA.val;
        const float dFa = dsim * sh.P[tid];
        cnt_entry(bs, tid, eA, dFa);
        bs.T[tid] = -dFa * eA.slope * sgn(ai - aj);
    }
    __syncthreads();
    cnt_scan(bs, tid, mm, acc_cs, acc_w);
    if (tid < m) {
        float t = 0.f;
        for (int k = 0; k < m; ++k) t += bs.T[tid * m + k] - bs.T[k * m + tid];
        bs.da[tid] += t;
    }
    __syncthreads();
    // the m^3 factors, a slab per k: d F_kij = d P_ij prod_{k' != k} F_k'ij
    for (int k = 0; k < m; ++k) {
        if (pair) {
            float oth = 1.f;
            for (int kk = 0; kk < m; ++kk) oth *= kk == k ? 1.f : bs.cube[kk * 256 + tid];
            const float xi = sh.X[k * m + i], xj = sh.X[k * m + j];
            const Pw eF = pw_eval(sh.wn[2], sh.cs[2], 1.f - fabsf(xi - xj));
            const float dF = dP * oth;
            cnt_entry(bs, tid, eF, dF);
            bs.T[tid] = -dF * eF.slope * sgn(xi - xj);
        }
        __syncthreads();
        cnt_scan(bs, tid, mm, acc_cs, acc_w);
        if (tid < m) {
            float t = 0.f;
            for (int q = 0; q < m; ++q) t += bs.T[tid * m + q] - bs.T[q * m + tid];
            bs.dX[k * m + tid] = t;
        }
        __syncthreads();
    }
    cnt_flush(bs, tid, 2, acc_cs, acc_w);

    // X_ki = f3(r_ki) f4(d_ki): this thread's pair is (k, i) = (i, j)
    const Pw e3 = pw_eval(sh.wn[3], sh.cs[3], r), e4 = pw_eval(sh.wn[4], sh.cs[4], d);
    const float dXp = pair ? bs.dX[tid] : 0.f;
    dr += dXp * e4.val * e3.slope;
    if (pair) cnt_entry(bs, tid, e3, dXp * e4.val);
    __syncthreads();
    cnt_scan(bs, tid, mm, acc_cs, acc_w);
    __syncthreads();
    cnt_flush(bs, tid, 3, acc_cs, acc_w);
    if (pair) { cnt_entry(bs, tid, e4, dXp * e3.val); bs.T[tid] = dr; }
    __syncthreads();
    cnt_scan(bs, tid, mm, acc_cs, acc_w);
    // r_ij = a_i a_j;  a = sigmoid(s)
    if (tid < m) {
        float t = 0.f;
        for (int k = 0; k < m; ++k) t += (bs.T[tid * m + k] + bs.T[k * m + tid]) * sh.a[k];
        const float a = sh.a[tid];
        const float da = bs.da[tid] + t;
        bs.da[tid] = sigm ? da * a * (1.f - a) : da;
    }
    __syncthreads();
    cnt_flush(bs, tid, 4, acc_cs, acc_w);

    // the dense logit gradient: zero except at (selected box, its arg-max position)
    float* dL = dlogits + (int64_t)row * V * Q;
    for (int e = tid; e < V * Q; e += CNT_THREADS) {
        const int v = e / Q, q = e - v * Q;
        float x = 0.f;
        for (int k = 0; k < m; ++k) x = (sh.idx[k] == v && sh.amax[k] == q) ? bs.da[k] : x;
        dL[e] = x;
    }

    // d wn = direct + suffix sums of d cs;  wn = |w| / sum |w|
    const int f = tid / CNT_NW, l = tid - f * CNT_NW;
    if (tid < CNT_F * CNT_NW) {
        float t = 0.f;
        for (int k = CNT_N; k >= l; --k) t += bs.hist[f][0][k];
        bs.cube[tid] = t + bs.hist[f][1][l];                        // (the cube is done: its first 136 words hold d wn)
    }
    __syncthreads();
    if (tid < CNT_F * CNT_NW) {
        float s = 0.f;
        for (int k = 0; k < CNT_NW; ++k) s += bs.cube[f * CNT_NW + k] * sh.wn[f][k];
        dw_part[(int64_t)row * (CNT_F * CNT_NW) + tid] = (bs.cube[tid] - s) / sh.wsum[f] * sgn(W.w[f][l]);
    }
}

}  // namespace
}  // namespace cti

using namespace cti;

static int counter_args(const char* fn, const float* const* weights, CntWeights& W, int B, int G, int V, int Q, int objects, int n) {
    CTI_REQUIRE(B > 0 && G > 0 && V > 0 && Q > 0 && objects > 0 && (int64_t)B * G < (1ll << 31), CTI_E_SHAPE, "%s: B=%d G=%d V=%d Q=%d objects=%d", fn, B, G, V, Q, objects);
    CTI_REQUIRE(objects <= CNT_MAXM && n == CNT_N, CTI_E_UNSUPPORTED, "%s: objects=%d (1 .. %d) with n=%d segments (%d) is what this kernel takes", fn, objects,
                CNT_MAXM, n, CNT_N);
    CTI_REQUIRE(V >= objects, CTI_E_SHAPE, "%s: %d boxes, but the counter keeps the %d with the highest attention (V >= objects)", fn, V, objects);
    CTI_REQUIRE(V <= CNT_MAX_V && (int64_t)V * Q < (1ll << 31), CTI_E_UNSUPPORTED, "%s: V=%d boxes (at most %d) x Q=%d", fn, V, CNT_MAX_V, Q);
    for (int f = 0; f < CNT_F; ++f) {
        if (weights[f] == nullptr) return fail(CTI_E_NULL, "%s: weights[%d] is NULL", fn, f);
        W.w[f] = weights[f];
    }
    return CTI_OK;
}

extern "C" size_t cti_counter_save_bytes(int64_t rows) { return rows > 0 ? (size_t)rows * CNT_SAVE_WORDS * sizeof(int) : 0; }

extern "C" int cti_counter_fwd(const float* logits, int64_t sLb, int64_t sLg, int64_t sLv, int64_t sLq, const float* boxes, int64_t sBb, int64_t sBc, int64_t sBv,
                               const float* const* weights, int already_sigmoided, float* out, int64_t sOb, int64_t sOg, void* save, size_t save_bytes, int B, int G,
                               int V, int Q, int objects, int n, void* stream) {
    CTI_REQUIRE_PTR(logits); CTI_REQUIRE_PTR(boxes); CTI_REQUIRE_PTR(weights); CTI_REQUIRE_PTR(out); CTI_REQUIRE_PTR(save);
    CntWeights W;
    const int rc = counter_args("cti_counter_fwd", weights, W, B, G, V, Q, objects, n);
    if (rc) return rc;
    CTI_REQUIRE(sLb >= 0 && sLg >= 0 && sLv >= 0 && sLq >= 0 && sBb >= 0 && sBc >= 0 && sBv >= 0, CTI_E_SHAPE, "cti_counter_fwd: negative stride");
    CTI_REQUIRE(sOb > objects && sOg > objects && (sOb >= (int64_t)G * sOg || sOg >= (int64_t)B * sOb), CTI_E_SHAPE,
                "cti_counter_fwd: output strides sOb=%lld sOg=%lld do not hold B=%d x G=%d rows of %d without overlap", (long long)sOb, (long long)sOg, B, G, objects + 1);
    CTI_REQUIRE(save_bytes >= cti_counter_save_bytes((int64_t)B * G), CTI_E_WORKSPACE, "cti_counter_fwd: save block %zu < %zu", save_bytes,
                cti_counter_save_bytes((int64_t)B * G));
    hipLaunchKernelGGL(counter_fwd_kernel, dim3((unsigned)(B * G)), dim3(CNT_THREADS), (size_t)V * sizeof(unsigned), as_stream(stream), logits, sLb, sLg, sLv, sLq,
                       boxes, sBb, sBc, sBv, W, already_sigmoided ? 0 : 1, out, sOb, sOg, static_cast<int*>(save), G, V, Q, objects);
    return launch_status("cti_counter_fwd");
}

extern "C" int cti_counter_bwd(const float* dout, const float* boxes, int64_t sBb, int64_t sBc, int64_t sBv, const float* const* weights, int already_sigmoided,
                               const void* save, size_t save_bytes, float* dlogits, float* dw_part, int B, int G, int V, int Q, int objects, int n, void* stream) {
    CTI_REQUIRE_PTR(dout); CTI_REQUIRE_PTR(boxes); CTI_REQUIRE_PTR(weights); CTI_REQUIRE_PTR(save); CTI_REQUIRE_PTR(dlogits); CTI_REQUIRE_PTR(dw_part);
    CntWeights W;
    const int rc = counter_args("cti_counter_bwd", weights, W, B, G, V, Q, objects, n);
    if (rc) return rc;
    CTI_REQUIRE(sBb >= 0 && sBc >= 0 && sBv >= 0, CTI_E_SHAPE, "cti_counter_bwd: negative stride");
    CTI_REQUIRE(save_bytes >= cti_counter_save_bytes((int64_t)B * G), CTI_E_WORKSPACE, "cti_counter_bwd: save block %zu < %zu", save_bytes,
                cti_counter_save_bytes((int64_t)B * G));
    hipLaunchKernelGGL(counter_bwd_kernel, dim3((unsigned)(B * G)), dim3(CNT_THREADS), 0, as_stream(stream), dout, boxes, sBb, sBc, sBv, W, already_sigmoided ? 0 : 1,
                       static_cast<const int*>(save), dlogits, dw_part, G, V, Q, objects);
    return launch_status("cti_counter_bwd");
}
