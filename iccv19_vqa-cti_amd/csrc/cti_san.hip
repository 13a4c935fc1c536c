// cti_san.hip -- the attention step of the SAN baseline's StackedAttention (src/attention.py:90-152), one workgroup per sample.
//
// Forward, per sample b (P: the sample's projected rows N x A, qv: the q-side vector A, X: the pool source N x Dx = P itself or v):
//     h[n,a]    = tanh(qv[a] + P[n,a])                     (dropout on h: keep[n,a] / (1 - p_drop), train mode only)
//     logit[n]  = bias + sum_a w[a] h[n,a],  -inf where every element of P[n,:] is +-0 (v_mask; the reference tests the PROJECTED rows)
//     prob      = softmax(logit) over n                    (all rows masked: NaN, as torch.softmax gives)
//     pooled[d] = sum_n prob[n] X[n,d]
// Three passes over one sample: the logits (a wave per row, P read once), the softmax over N values, the pool (X read once).  No (N x A)
// intermediate is written; logits and prob are the (B, N) outputs the passes hand on through the workgroup's own global writes.
//
// Backward (prob saved by the forward, tanh recomputed from P and qv):
//     dp[n]  = dpooled . X[n,:];  dl[n] = prob[n] (dp[n] - sum_m prob[m] dp[m])
//     dz[n,a] = dl[n] w[a] s[n,a] (1 - h^2)   (s = the dropout factor)
//     dP[n,a] = dz[n,a] (+ prob[n] dpooled[a] when X = P);  dqv[a] = sum_n dz[n,a]
//     dw_part[b,a] = sum_n dl[n] s[n,a] h[n,a];  db_part[b] = sum_n dl[n]     (reduced over b by the caller: cti_col_sum)
//     dX[n,d] = prob[n] dpooled[d]            (only on request)
// Every sum has a fixed order (no atomics): gradients are bitwise reproducible from run to run.
#include "cti_common.h"

#include <math.h>

namespace cti {
namespace {

constexpr int SAN_THREADS = 256;

__device__ __forceinline__ unsigned wave_or(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x |= (unsigned)__shfl_xor((int)x, o, 64);
    return x;
}

// fixed-order reductions over the workgroup: per-wave butterflies, then the wave results in wave order
__device__ __forceinline__ float block_sum(float x, float* red) {
    x = wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}
__device__ __forceinline__ float block_max(float x, float* red) {
    x = wave_max(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) t = fmaxf(t, red[i]);
    return t;
}

__device__ __forceinline__ float drop_factor(const uint8_t* k, float ks) { return k == nullptr ? 1.f : (*k ? ks : 0.f); }

// VA = 4: A, ldp, sP, sq % 4 == 0 and P, qv, w (keep) aligned -> float4 rows; VX = 4: the same for the pool source and its output
template <int VA, int VX>
__global__ __launch_bounds__(SAN_THREADS) void san_fwd_kernel(const float* __restrict__ P, int64_t ldp, int64_t sP, const float* __restrict__ qv, int64_t sq,
                                                            const float* __restrict__ w, const float* __restrict__ bias, const uint8_t* __restrict__ keep,
                                                            float ks, int v_mask, const float* __restrict__ X, int64_t ldx, int64_t sX,
                                                            float* __restrict__ logits, float* __restrict__ prob, float* __restrict__ pooled, int64_t ldo,
                                                            int N, int A, int Dx) {
    __shared__ float red[SAN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const float* Pb = P + (int64_t)b * sP;
    const float* qb = qv + (int64_t)b * sq;
    const uint8_t* kb = keep ? keep + (int64_t)b * N * A : nullptr;
    float* lg = logits + (int64_t)b * N;
    float* pr = prob + (int64_t)b * N;
    const float b0 = bias ? bias[0] : 0.f;

    // 1. logits: a wave per row
    for (int n = wv; n < N; n += nw) {
        const float* row = Pb + (int64_t)n * ldp;
        const uint8_t* kr = kb ? kb + (int64_t)n * A : nullptr;
        float acc = 0.f;
        unsigned nz = 0;
        if (VA == 4) {
            for (int a = lane * 4; a < A; a += 256) {
                const float4 p = *reinterpret_cast<const float4*>(row + a);
                const float4 q = *reinterpret_cast<const float4*>(qb + a);
                const float4 ww = *reinterpret_cast<const float4*>(w + a);
                nz |= (__float_as_uint(p.x) | __float_as_uint(p.y) | __float_as_uint(p.z) | __float_as_uint(p.w)) & 0x7fffffffu;
                float h0 = tanhf(q.x + p.x), h1 = tanhf(q.y + p.y), h2 = tanhf(q.z + p.z), h3 = tanhf(q.w + p.w);
                if (kr) {
                    const uchar4 k = *reinterpret_cast<const uchar4*>(kr + a);
                    h0 = k.x ? h0 * ks : 0.f; h1 = k.y ? h1 * ks : 0.f; h2 = k.z ? h2 * ks : 0.f; h3 = k.w ? h3 * ks : 0.f;
                }
                acc += ww.x * h0 + ww.y * h1 + ww.z * h2 + ww.w * h3;
            }
        } else {
            for (int a = lane; a < A; a += 64) {
                const float p = row[a];
                nz |= __float_as_uint(p) & 0x7fffffffu;
                acc += w[a] * (tanhf(qb[a] + p) * drop_factor(kr ? kr + a : nullptr, ks));
            }
        }
        acc = wave_sum(acc);
        nz = wave_or(nz);
        if (lane == 0) lg[n] = (v_mask && nz == 0) ? -INFINITY : acc + b0;
    }
    __syncthreads();

    // 2. softmax over the N logits (all -inf: NaN)
    float m = -INFINITY;
    for (int n = tid; n < N; n += blockDim.x) m = fmaxf(m, lg[n]);
    m = block_max(m, red);
    float s = 0.f;
    for (int n = tid; n < N; n += blockDim.x) s += expf(lg[n] - m);
    s = block_sum(s, red);
    for (int n = tid; n < N; n += blockDim.x) pr[n] = expf(lg[n] - m) / s;
    __syncthreads();

    // 3. pooled = sum_n prob[n] X[n,:]: a thread per (4) columns, rows in order
    const float* Xb = X + (int64_t)b * sX;
    float* ob = pooled + (int64_t)b * ldo;
    if (VX == 4) {
        for (int d = tid * 4; d < Dx; d += blockDim.x * 4) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
            for (int n = 0; n < N; ++n) {
                const float p = pr[n];
                const float4 x = *reinterpret_cast<const float4*>(Xb + (int64_t)n * ldx + d);
                acc.x += p * x.x; acc.y += p * x.y; acc.z += p * x.z; acc.w += p * x.w;
            }
            *reinterpret_cast<float4*>(ob + d) = acc;
        }
    } else {
        for (int d = tid; d < Dx; d += blockDim.x) {
            float acc = 0.f;
#pragma unroll 4
            for (int n = 0; n < N; ++n) acc += pr[n] * Xb[(int64_t)n * ldx + d];
            ob[d] = acc;
        }
    }
}

template <int VA, int VX>
__global__ __launch_bounds__(SAN_THREADS) void san_bwd_kernel(const float* __restrict__ P, int64_t ldp, int64_t sP, const float* __restrict__ qv, int64_t sq,
                                                            const float* __restrict__ w, const uint8_t* __restrict__ keep, float ks,
                                                            const float* __restrict__ X, int64_t ldx, int64_t sX, int x_is_p,
                                                            const float* __restrict__ prob, const float* __restrict__ dpooled, int64_t ldg,
                                                            float* __restrict__ dP, int64_t lddp, int64_t sdP, float* __restrict__ dqv, int64_t sdq,
                                                            float* __restrict__ dw_part, float* __restrict__ db_part, float* __restrict__ dlogit,
                                                            float* __restrict__ dX, int64_t lddx, int64_t sdX, int N, int A, int Dx) {
    __shared__ float red[SAN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const float* Pb = P + (int64_t)b * sP;
    const float* qb = qv + (int64_t)b * sq;
    const uint8_t* kb = keep ? keep + (int64_t)b * N * A : nullptr;
    const float* pr = prob + (int64_t)b * N;
    const float* g = dpooled + (int64_t)b * ldg;
    const float* Xb = x_is_p ? Pb : X + (int64_t)b * sX;
    const int64_t ldxx = x_is_p ? ldp : ldx;
    float* dl = dlogit + (int64_t)b * N;

    // 1. dp[n] = dpooled . X[n,:]: a wave per row
    for (int n = wv; n < N; n += nw) {
        const float* row = Xb + (int64_t)n * ldxx;
        float acc = 0.f;
        if (VX == 4) {
            for (int d = lane * 4; d < Dx; d += 256) {
                const float4 x = *reinterpret_cast<const float4*>(row + d);
                const float4 gg = *reinterpret_cast<const float4*>(g + d);
                acc += gg.x * x.x + gg.y * x.y + gg.z * x.z + gg.w * x.w;
            }
        } else {
            for (int d = lane; d < Dx; d += 64) acc += g[d] * row[d];
        }
        acc = wave_sum(acc);
        if (lane == 0) dl[n] = acc;
    }
    __syncthreads();

    // 2. dl[n] = prob[n] (dp[n] - sum_m prob[m] dp[m]);  db_part = sum_n dl[n]
    float t = 0.f;
    for (int n = tid; n < N; n += blockDim.x) t += pr[n] * dl[n];
    const float sdot = block_sum(t, red);
    t = 0.f;
    for (int n = tid; n < N; n += blockDim.x) {
        const float v = pr[n] * (dl[n] - sdot);
        dl[n] = v;
        t += v;
    }
    t = block_sum(t, red);                           // (its barriers also publish dl[] to the whole workgroup)
    if (tid == 0) db_part[b] = t;

    // 3. per column a: recompute h, form dz, write dP, sum dqv and the dw partial over the rows in order
    float* dPb = dP + (int64_t)b * sdP;
    if (VA == 4) {
        for (int a = tid * 4; a < A; a += blockDim.x * 4) {
            const float4 q = *reinterpret_cast<const float4*>(qb + a);
            const float4 ww = *reinterpret_cast<const float4*>(w + a);
            const float4 ga = x_is_p ? *reinterpret_cast<const float4*>(g + a) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 dwa = make_float4(0.f, 0.f, 0.f, 0.f), dqa = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int n = 0; n < N; ++n) {
                const float4 p = *reinterpret_cast<const float4*>(Pb + (int64_t)n * ldp + a);
                const float dln = dl[n], pn = pr[n];
                float s0 = 1.f, s1 = 1.f, s2 = 1.f, s3 = 1.f;
                if (kb) {
                    const uchar4 k = *reinterpret_cast<const uchar4*>(kb + (int64_t)n * A + a);
                    s0 = k.x ? ks : 0.f; s1 = k.y ? ks : 0.f; s2 = k.z ? ks : 0.f; s3 = k.w ? ks : 0.f;
                }
                const float h0 = tanhf(q.x + p.x), h1 = tanhf(q.y + p.y), h2 = tanhf(q.z + p.z), h3 = tanhf(q.w + p.w);
                dwa.x += dln * (h0 * s0); dwa.y += dln * (h1 * s1); dwa.z += dln * (h2 * s2); dwa.w += dln * (h3 * s3);
                float4 dz;
                dz.x = dln * ww.x * s0 * (1.f - h0 * h0); dz.y = dln * ww.y * s1 * (1.f - h1 * h1);
                dz.z = dln * ww.z * s2 * (1.f - h2 * h2); dz.w = dln * ww.w * s3 * (1.f - h3 * h3);
                dqa.x += dz.x; dqa.y += dz.y; dqa.z += dz.z; dqa.w += dz.w;
                if (x_is_p) { dz.x += pn * ga.x; dz.y += pn * ga.y; dz.z += pn * ga.z; dz.w += pn * ga.w; }
                *reinterpret_cast<float4*>(dPb + (int64_t)n * lddp + a) = dz;
            }
            *reinterpret_cast<float4*>(dw_part + (int64_t)b * A + a) = dwa;
            *reinterpret_cast<float4*>(dqv + (int64_t)b * sdq + a) = dqa;
        }
    } else {
        for (int a = tid; a < A; a += blockDim.x) {
            const float q = qb[a], wa = w[a], ga = x_is_p ? g[a] : 0.f;
            float dwa = 0.f, dqa = 0.f;
            for (int n = 0; n < N; ++n) {
                const float s = drop_factor(kb ? kb + (int64_t)n * A + a : nullptr, ks);
                const float h = tanhf(q + Pb[(int64_t)n * ldp + a]);
                const float dln = dl[n];
                dwa += dln * (h * s);
                const float dz = dln * wa * s * (1.f - h * h);
                dqa += dz;
                dPb[(int64_t)n * lddp + a] = x_is_p ? dz + pr[n] * ga : dz;
            }
            dw_part[(int64_t)b * A + a] = dwa;
            dqv[(int64_t)b * sdq + a] = dqa;
        }
    }

    // 4. dX[n,:] = prob[n] dpooled (the pool source as an input of its own; X = P is folded into dP above)
    if (dX != nullptr) {
        float* dXb = dX + (int64_t)b * sdX;
        if (VX == 4) {
            for (int d = tid * 4; d < Dx; d += blockDim.x * 4) {
                const float4 gg = *reinterpret_cast<const float4*>(g + d);
                for (int n = 0; n < N; ++n) {
                    const float pn = pr[n];
                    *reinterpret_cast<float4*>(dXb + (int64_t)n * lddx + d) = make_float4(pn * gg.x, pn * gg.y, pn * gg.z, pn * gg.w);
                }
            }
        } else {
            for (int d = tid; d < Dx; d += blockDim.x) {
                const float gd = g[d];
                for (int n = 0; n < N; ++n) dXb[(int64_t)n * lddx + d] = pr[n] * gd;
            }
        }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace cti

using namespace cti;

extern "C" int cti_san_attend_fwd(const float* P, int64_t ldp, int64_t sP, const float* qv, int64_t sq, const float* w, const float* bias,
                                  const uint8_t* keep, float p_drop, int v_mask, const float* X, int64_t ldx, int64_t sX,
                                  float* logits, float* prob, float* pooled, int64_t ldo, int B, int N, int A, int Dx, void* stream) {
    CTI_REQUIRE_PTR(P); CTI_REQUIRE_PTR(qv); CTI_REQUIRE_PTR(w); CTI_REQUIRE_PTR(X);
    CTI_REQUIRE_PTR(logits); CTI_REQUIRE_PTR(prob); CTI_REQUIRE_PTR(pooled);
    CTI_REQUIRE(B > 0 && N > 0 && A > 0 && Dx > 0, CTI_E_SHAPE, "cti_san_attend_fwd: B=%d N=%d A=%d Dx=%d", B, N, A, Dx);
    CTI_REQUIRE(ldp >= A && sP >= (int64_t)(N - 1) * ldp + A && sq >= A && ldx >= Dx && sX >= (int64_t)(N - 1) * ldx + Dx && ldo >= Dx, CTI_E_SHAPE,
                "cti_san_attend_fwd: strides ldp=%lld sP=%lld sq=%lld ldx=%lld sX=%lld ldo=%lld too small for N=%d A=%d Dx=%d",
                (long long)ldp, (long long)sP, (long long)sq, (long long)ldx, (long long)sX, (long long)ldo, N, A, Dx);
    CTI_REQUIRE(keep == nullptr || (p_drop >= 0.f && p_drop < 1.f), CTI_E_SHAPE, "cti_san_attend_fwd: p_drop=%g outside [0, 1)", (double)p_drop);
    const float ks = keep ? 1.f / (1.f - p_drop) : 1.f;
    const bool va = A % 4 == 0 && ldp % 4 == 0 && sP % 4 == 0 && sq % 4 == 0 && al16(P) && al16(qv) && al16(w) &&
                    (keep == nullptr || (reinterpret_cast<uintptr_t>(keep) & 3) == 0);
    const bool vx = Dx % 4 == 0 && ldx % 4 == 0 && sX % 4 == 0 && ldo % 4 == 0 && al16(X) && al16(pooled);
    auto k = va ? (vx ? san_fwd_kernel<4, 4> : san_fwd_kernel<4, 1>) : (vx ? san_fwd_kernel<1, 4> : san_fwd_kernel<1, 1>);
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(SAN_THREADS), 0, as_stream(stream), P, ldp, sP, qv, sq, w, bias, keep, ks, v_mask, X, ldx, sX,
                       logits, prob, pooled, ldo, N, A, Dx);
    return launch_status("cti_san_attend_fwd");
}

extern "C" int cti_san_attend_bwd(const float* P, int64_t ldp, int64_t sP, const float* qv, int64_t sq, const float* w, const uint8_t* keep, float p_drop,
                                  const float* X, int64_t ldx, int64_t sX, int x_is_p, const float* prob, const float* dpooled, int64_t ldg,
                                  float* dP, int64_t lddp, int64_t sdP, float* dqv, int64_t sdq, float* dw_part, float* db_part, float* dlogit,
                                  float* dX, int64_t lddx, int64_t sdX, int B, int N, int A, int Dx, void* stream) {
    CTI_REQUIRE_PTR(P); CTI_REQUIRE_PTR(qv); CTI_REQUIRE_PTR(w); CTI_REQUIRE_PTR(prob); CTI_REQUIRE_PTR(dpooled);
    CTI_REQUIRE_PTR(dP); CTI_REQUIRE_PTR(dqv); CTI_REQUIRE_PTR(dw_part); CTI_REQUIRE_PTR(db_part); CTI_REQUIRE_PTR(dlogit);
    if (!x_is_p) CTI_REQUIRE_PTR(X);
    CTI_REQUIRE(B > 0 && N > 0 && A > 0 && Dx > 0, CTI_E_SHAPE, "cti_san_attend_bwd: B=%d N=%d A=%d Dx=%d", B, N, A, Dx);
    CTI_REQUIRE(!x_is_p || (Dx == A && dX == nullptr), CTI_E_SHAPE, "cti_san_attend_bwd: pooling P itself needs Dx == A (%d, %d) and no dX", Dx, A);
    CTI_REQUIRE(ldp >= A && sP >= (int64_t)(N - 1) * ldp + A && sq >= A && ldg >= Dx && lddp >= A && sdP >= (int64_t)(N - 1) * lddp + A && sdq >= A &&
                (x_is_p || (ldx >= Dx && sX >= (int64_t)(N - 1) * ldx + Dx)) && (dX == nullptr || (lddx >= Dx && sdX >= (int64_t)(N - 1) * lddx + Dx)),
                CTI_E_SHAPE, "cti_san_attend_bwd: a stride is too small for N=%d A=%d Dx=%d", N, A, Dx);
    CTI_REQUIRE(keep == nullptr || (p_drop >= 0.f && p_drop < 1.f), CTI_E_SHAPE, "cti_san_attend_bwd: p_drop=%g outside [0, 1)", (double)p_drop);
    const float ks = keep ? 1.f / (1.f - p_drop) : 1.f;
    if (x_is_p) { X = P; ldx = ldp; sX = sP; }
    const bool va = A % 4 == 0 && ldp % 4 == 0 && sP % 4 == 0 && sq % 4 == 0 && lddp % 4 == 0 && sdP % 4 == 0 && sdq % 4 == 0 && al16(P) && al16(qv) &&
                    al16(w) && al16(dP) && al16(dqv) && al16(dw_part) && (keep == nullptr || (reinterpret_cast<uintptr_t>(keep) & 3) == 0) &&
                    (!x_is_p || (ldg % 4 == 0 && al16(dpooled)));
    const bool vx = Dx % 4 == 0 && ldx % 4 == 0 && sX % 4 == 0 && ldg % 4 == 0 && al16(X) && al16(dpooled) &&
                    (dX == nullptr || (lddx % 4 == 0 && sdX % 4 == 0 && al16(dX)));
    auto k = va ? (vx ? san_bwd_kernel<4, 4> : san_bwd_kernel<4, 1>) : (vx ? san_bwd_kernel<1, 4> : san_bwd_kernel<1, 1>);
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(SAN_THREADS), 0, as_stream(stream), P, ldp, sP, qv, sq, w, keep, ks, X, ldx, sX, x_is_p ? 1 : 0, prob,
                       dpooled, ldg, dP, lddp, sdP, dqv, sdq, dw_part, db_part, dlogit, dX, lddx, sdX, N, A, Dx);
    return launch_status("cti_san_attend_bwd");
}
