"""Float64 references, error scales and seeded inputs for the small kernels of csrc/cti_model.hip and csrc/cti_backward.hip (the two losses,
the backward primitives, the elementwise and sequence kernels).  CPU only: numpy and torch, no GPU and no import of the package, so
tests/test_small_kernel_refs_cpu.py can validate every function here on any machine and tests/test_small_kernels_gpu.py compares the
kernels with them.

A bound is always  c * EPS32 * scale:  the scale is computed here in float64 from the inputs (never from a kernel's output), the constant c
comes from the arithmetic (see each function) and is applied by the test."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23                      # float32 machine epsilon (one ulp of 1.0)
F32 = np.float32
F64 = np.float64


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F64))


# =============================================================================================================================
# 1. losses
# =============================================================================================================================
LOSS_SHAPES = [(1, 1), (3, 2), (5, 63), (5, 255), (4, 256), (4, 257), (300, 7), (2, 3129)]
LOSS_STDS = (1.0, 8.0, 30.0)
KD_TEMPS = (0.5, 1.5, 4.0)
SOFT_SCORES = np.array([0.0, 0.3, 0.6, 0.9, 1.0], dtype=F32)
LOSS_C_FWD = 4.0                        # emulated worst ratio (< 1, asserted on the CPU) times 4 for __expf / __logf
N_SPECIAL = 4                           # rows appended by loss_inputs
TINY32 = 2.0 ** -126                    # smallest normal float32


def loss_ratio(err, S, n):
    """error of a row loss in units of EPS32 * S, after an absolute allowance of n * TINY32: a row of -100 whose targets are all 0 has
    S = n * log1p(exp(-100)) = n * 3.7e-44, below the normal range of float32, where a float32 result (denormals kept or flushed) cannot be within
    EPS32 * S of anything; one smallest normal per element is the precision of the number format there."""
    return np.maximum(0.0, np.asarray(err, F64) - n * TINY32) / (EPS32 * np.asarray(S, F64))


def loss_inputs(rows, n, std, seed=0):
    """x, k (student / teacher logits) and t (soft VQA scores), float32, (rows + 4, n).  Rows [0, rows) are N(0, std^2); then one row of +100,
    one of -100, one random row with a single logit 60 above its maximum, and one row whose teacher equals the student bit for bit."""
    rs = np.random.RandomState(1000003 * seed + 7919 * rows + 31 * n + int(std))
    R = rows + N_SPECIAL
    x = (rs.standard_normal((R, n)) * std).astype(F32)
    k = (rs.standard_normal((R, n)) * std).astype(F32)
    t = SOFT_SCORES[rs.randint(0, len(SOFT_SCORES), size=(R, n))]
    x[rows] = 100.0
    x[rows + 1] = -100.0
    x[rows + 2, rs.randint(0, n)] = x[rows + 2].max() + F32(60.0)
    k[rows + 3] = x[rows + 3]
    return {"x": x, "k": k, "t": t, "plus": rows, "minus": rows + 1, "dominant": rows + 2, "equal": rows + 3}


MODULE_BATCHES = (1, 31, 32, 33, 257)   # either side of the nb = 32 switch of cti_sum_batches, which adds the B row losses


def module_inputs(B, n=37, std=8.0):
    """x, k, t (B, n) float32 for the two loss modules"""
    rs = np.random.RandomState(555 + B)
    x = (rs.standard_normal((B, n)) * std).astype(F32)
    k = (rs.standard_normal((B, n)) * std).astype(F32)
    return x, k, SOFT_SCORES[rs.randint(0, len(SOFT_SCORES), size=(B, n))]


def bce_rows_ref(x, t):
    """per-row sum of F.binary_cross_entropy_with_logits(reduction='none') in float64 -> (rows,)"""
    return F.binary_cross_entropy_with_logits(t64(x), t64(t), reduction="none").sum(1).numpy()


def bce_rows_scale(x, t):
    """S = sum_c |max(x,0)| + |x t| + log1p(exp(-|x|)): what the row sum adds up, in magnitude."""
    x = np.asarray(x, F64); t = np.asarray(t, F64)
    return (np.maximum(x, 0.0) + np.abs(x * t) + np.log1p(np.exp(-np.abs(x)))).sum(1)


def bce_grad_ref(x, t, cu):
    """float64 autograd of cu * sum(BCE) with respect to x"""
    xx = t64(x).requires_grad_(True)
    (F.binary_cross_entropy_with_logits(xx, t64(t), reduction="sum") * cu).backward()
    return xx.grad.numpy()


def kd_rows_ref(x, k, T):
    """per-row KL(softmax(k/T) || softmax(x/T)) in float64 -> (rows,)"""
    return F.kl_div(F.log_softmax(t64(x) / T, dim=1), F.softmax(t64(k) / T, dim=1), reduction="none").sum(1).numpy()


def kd_rows_scale(x, k, T):
    """S = (2 + max|b|) sum pk |lb - la| + 2 (max|a| + max|b| + log n),  a = x/T, b = k/T: the first term carries the relative error of
    exp(lk), which grows with |k/T|; the second the rounding of the four O(|logit|/T) quantities the log-softmaxes are differences of."""
    a = t64(x) / T; b = t64(k) / T
    la = F.log_softmax(a, dim=1); lb = F.log_softmax(b, dim=1)
    pk = lb.exp()
    ma = a.abs().max(1).values; mb = b.abs().max(1).values
    return ((2.0 + mb) * (pk * (lb - la).abs()).sum(1) + 2.0 * (ma + mb + math.log(x.shape[1]))).numpy()


def kd_grad_ref(x, k, T, cu):
    """float64 autograd of cu * sum_rows KL with respect to x"""
    xx = t64(x).requires_grad_(True)
    (F.kl_div(F.log_softmax(xx / T, dim=1), F.softmax(t64(k) / T, dim=1), reduction="none").sum() * cu).backward()
    return xx.grad.numpy()


def distillation_ref(x, k, t, T, alpha, up):
    """The reference module in float64: mean_b KL * alpha T^2 + BCE_sum / B * (1 - alpha); returns (loss, d(up * loss)/dx)."""
    xx = t64(x).requires_grad_(True)
    kl = F.kl_div(F.log_softmax(xx / T, dim=1), F.softmax(t64(k) / T, dim=1), reduction="none").sum(1).mean()
    loss = kl * (alpha * T * T) + F.binary_cross_entropy_with_logits(xx, t64(t), reduction="sum") / x.shape[0] * (1.0 - alpha)
    (loss * up).backward()
    return float(loss.detach()), xx.grad.numpy()


# ---- float32 emulation of the two forward kernels: 256 strided partial sums, a 6-level xor tree per wave, the 4 wave sums in order ----------
def _emu_block_sum(p):
    """p (rows, 256) float32 -> (rows,) as block_sum() adds it"""
    p = p.reshape(p.shape[0], 4, 64).astype(F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = (p + p[:, :, lane ^ o]).astype(F32)
    s = np.zeros(p.shape[0], F32)
    for w in range(4):
        s = (s + p[:, w, 0]).astype(F32)
    return s


def _emu_strided(fn, n, rows):
    """sum over c = tid, tid + 256, ... of fn(columns) per thread, then the block sum"""
    part = np.zeros((rows, 256), F32)
    for c0 in range(0, n, 256):
        w = min(256, n - c0)
        part[:, :w] = (part[:, :w] + fn(slice(c0, c0 + w))).astype(F32)
    return _emu_block_sum(part)


def bce_rows_emulated(x, t):
    x = np.asarray(x, F32); t = np.asarray(t, F32)

    def term(c):
        v = x[:, c]
        return ((np.maximum(v, F32(0)) - v * t[:, c]).astype(F32) + np.log1p(np.exp(-np.abs(v)).astype(F32)).astype(F32)).astype(F32)
    return _emu_strided(term, x.shape[1], x.shape[0])


def kd_rows_emulated(x, k, T):
    x = np.asarray(x, F32); k = np.asarray(k, F32)
    invT = F32(1.0) / F32(T)
    a = (x * invT).astype(F32); b = (k * invT).astype(F32)
    mx = a.max(1, keepdims=True); mk = b.max(1, keepdims=True)
    rows, n = x.shape
    sx = _emu_strided(lambda c: np.exp((a[:, c] - mx).astype(F32)).astype(F32), n, rows)
    sk = _emu_strided(lambda c: np.exp((b[:, c] - mk).astype(F32)).astype(F32), n, rows)
    lsx = (mx[:, 0] + np.log(sx).astype(F32)).astype(F32)[:, None]
    lsk = (mk[:, 0] + np.log(sk).astype(F32)).astype(F32)[:, None]

    def term(c):
        lk = (b[:, c] - lsk).astype(F32); ls = (a[:, c] - lsx).astype(F32)
        return (np.exp(lk).astype(F32) * (lk - ls).astype(F32)).astype(F32)
    return _emu_strided(term, n, rows)


# =============================================================================================================================
# 2. backward primitives
# =============================================================================================================================
def sum_c(depth):
    """constant of a float32 sum whose longest chain has `depth` additions, in units of EPS32 * sum |addends|: 8 up to 17 additions, depth / 2 + 4
    beyond (depth / 2 * EPS32 = depth * 2^-24 is the textbook bound of a chain; 4 covers the scaling and the beta term)"""
    return 8.0 if depth <= 17 else depth / 2.0 + 4.0


def sum_batches_tall(nb, n):
    return nb >= 32 and n < (1 << 20)


def sum_batches_depth(nb, n):
    """cti_sum_batches: the tall kernel adds ceil(nb / 4) values per batch lane, then two tree levels; the plain kernel adds nb in a row"""
    return (nb + 3) // 4 + 2 if sum_batches_tall(nb, n) else nb


def sum_batches_ref(src, alpha, beta, out0):
    """src (nb, n) -> (ref, scale), ref = alpha * sum_b src[b] + beta * out0"""
    s = np.asarray(src, F64)
    o = np.zeros(s.shape[1]) if beta == 0 else np.asarray(out0, F64)
    return alpha * s.sum(0) + beta * o, abs(alpha) * np.abs(s).sum(0) + np.abs(beta * o)


def col_groups(rows):
    return min(256, max(1, (rows + 31) // 32))


def col_sum_depth(rows, n):
    """cti_col_sum: `groups` row groups of rpg rows, four row lanes each (ceil(rpg / 4) additions, then 3 in a row), summed by cti_sum_batches"""
    g = col_groups(rows)
    rpg = (rows + g - 1) // g
    return (rpg + 3) // 4 + 3 + sum_batches_depth(g, n)


def col_sum_empty_groups(rows):
    g = col_groups(rows)
    rpg = (rows + g - 1) // g
    return sum(1 for i in range(g) if i * rpg >= rows)


def col_sum_ref(x, alpha):
    x = np.asarray(x, F64)
    return alpha * x.sum(0), abs(alpha) * np.abs(x).sum(0)


def act_chunks(rows):
    return min(1024, max(1, (rows + 63) // 64))


def act_bwd_route(n, aligned=True):
    if n >= 256 and n % 4 == 0 and aligned:
        return "v4"
    return "cw16" if n <= 16 else ("cw32" if n <= 32 else "cw64")


def act_bwd_depth(rows, n, aligned=True):
    """bias gradient of cti_act_bwd: a row lane adds ceil(rpc / RL) values, the lanes meet (2 tree levels for float4, RL in a row otherwise),
    cti_sum_batches adds the chunks"""
    ch = act_chunks(rows)
    rpc = (rows + ch - 1) // ch
    route = act_bwd_route(n, aligned)
    rl = 4 if route == "v4" else 256 // int(route[2:])
    lanes = 2 if route == "v4" else rl
    return (rpc + rl - 1) // rl + lanes + sum_batches_depth(ch, n)


def act_bwd_ref(dy, y, scale, scale_div, relu):
    """-> dzs (rows, n), dbias (n,), dbias scale (n,), gate (rows, n) bool: entries the ReLU closes"""
    dy = np.asarray(dy, F64)
    gate = ~(np.asarray(y) > 0) if relu else np.zeros(dy.shape, bool)
    g = np.where(gate, 0.0, dy)
    s = np.ones(dy.shape[1]) if scale is None else np.asarray(scale, F64)[np.arange(dy.shape[1]) // scale_div]
    return g * s[None, :], g.sum(0), np.abs(g).sum(0), gate


def wn_bwd_depth(elems):
    """cti_wn_bwd's dot product: one workgroup: ceil(elems / 1024) fmas, 6 xor levels, 16 wave sums in a row; chunked: 16 fmas, 6 levels, 2 tree
    levels per 4096-element chunk, then ceil(chunks / 256) additions, 6 levels and 2 tree levels over the chunks"""
    if elems <= 4096:
        return (elems + 1023) // 1024 + 6 + 16
    cpm = (elems + 4095) // 4096
    return 16 + 6 + 2 + (cpm + 255) // 256 + 6 + 2


def wn_bwd_route(elems, aligned=True):
    if elems <= 4096:
        return "one workgroup"
    return "chunked float4" if elems % 4 == 0 and aligned else "chunked scalar"


def wn_bwd_ref(G, V, g):
    """G, V (n_mats, elems), g (n_mats,) -> dV, dg, dV scale (per entry), dg scale (per matrix):
    dot = <G, V>, dg = dot / g, dV = G - (dot / |V|^2) V"""
    G = np.asarray(G, F64); V = np.asarray(V, F64); g = np.asarray(g, F64)
    dot = (G * V).sum(1); nn = (V * V).sum(1); adot = np.abs(G * V).sum(1)
    dV = G - (dot / nn)[:, None] * V
    return dV, dot / g, np.abs(G) + (adot / nn)[:, None] * np.abs(V), adot / np.abs(g)


def wn_bwd_autograd(G, V, g):
    """float64 autograd of <G / s, g V / |V|> with s = g / |V| held constant: G is the gradient with respect to V through the direct path,
    i.e. s times the gradient with respect to W = g V / |V| (cti_backward.hip, above wn_bwd_kernel)"""
    Gt, Vt, gt = t64(G), t64(V).requires_grad_(True), t64(g).requires_grad_(True)
    s = (gt / Vt.norm(dim=1)).detach()
    W = gt[:, None] * Vt / Vt.norm(dim=1, keepdim=True)
    ((Gt / s[:, None]) * W).sum().backward()
    return Vt.grad.numpy(), gt.grad.numpy()


def transpose_ref(src, dst0, rows, cols):
    """src (batch, rows, ld_src), dst0 (batch, cols, ld_dst): dst[b][c][r] = src[b][r][c]; the padding columns of dst0 are kept"""
    out = np.array(dst0, copy=True)
    out[:, :, :rows] = np.asarray(src)[:, :, :cols].transpose(0, 2, 1)
    return out


def dropout_ref(x, mask, p):
    """x * mask / (1 - p) in float64 with p as the kernel receives it (a float32); the kernel rounds 1 / (1 - p) and the product once each, so it
    is within EPS32 * |ref|, one ulp in the sense of this file"""
    return np.asarray(x, F64) * np.asarray(mask, F64) / (1.0 - float(F32(p)))


def keep_rate_bound(count, p, sigmas=5.0):
    return sigmas * math.sqrt(p * (1.0 - p) / count)


# =============================================================================================================================
# 3. elementwise and sequence kernels
# =============================================================================================================================
SWISH_SPECIAL = np.array([0.0, 1e-4, -1e-4, 20.0, -20.0, 100.0, -100.0], dtype=F32)


def swish_inputs(n, seed=0):
    rs = np.random.RandomState(4242 + 17 * n + seed)
    x = (rs.standard_normal(n) * 3.0).astype(F32)
    m = min(n, len(SWISH_SPECIAL))
    x[:m] = SWISH_SPECIAL[(np.arange(m) + n) % len(SWISH_SPECIAL)]    # n = 1 takes one of them, the larger sizes all seven
    dy = rs.standard_normal(n).astype(F32)
    return x, dy


def swish_ref(x):
    xx = t64(x)
    return (xx * torch.sigmoid(xx)).numpy()


def swish_bwd_ref(x, dy):
    x = np.asarray(x, F64)
    s = torch.sigmoid(t64(x)).numpy()
    return np.asarray(dy, F64) * (s + x * s * (1.0 - s))


def seq_sum_ref(x, beta, out0):
    """x (B, L, H) -> (ref, scale) of beta * out0 + sum_l x"""
    x = np.asarray(x, F64)
    o = np.zeros((x.shape[0], x.shape[2])) if beta == 0 else np.asarray(out0, F64)
    return beta * o + x.sum(1), np.abs(beta * o) + np.abs(x).sum(1)


def seq_bcast_add_ref(x, y, L):
    """float32: (x or 0) + y[:, None, :]"""
    y = np.asarray(y, F32)
    base = np.zeros((y.shape[0], L, y.shape[1]), F32) if x is None else np.asarray(x, F32)
    return (base + y[:, None, :]).astype(F32)


def axpby_ref(x, a, y, b):
    ax = float(F32(a)) * np.asarray(x, F64); by = float(F32(b)) * np.asarray(y, F64)
    return ax + by, np.abs(ax) + np.abs(by)


def embedding_ref(tokens, t0, t1=None):
    """float32 rows; a token outside [0, rows) gives a NaN row"""
    tok = np.asarray(tokens).reshape(-1)
    tab = np.asarray(t0, F32) if t1 is None else np.concatenate([np.asarray(t0, F32), np.asarray(t1, F32)], axis=1)
    ok = (tok >= 0) & (tok < tab.shape[0])
    out = np.full((len(tok), tab.shape[1]), np.nan, F32)
    out[ok] = tab[tok[ok]]
    return out.reshape(tuple(np.asarray(tokens).shape) + (tab.shape[1],)), ok.reshape(np.asarray(tokens).shape)


def bf16_bits(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even, through torch's own conversion"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def embedding_bwd_emulated(tokens, dout, col_off, rows, dim, padding_idx, reverse=False):
    """float32 accumulation in the documented order: per table row, 0 + g_j1 + g_j2 + ... over its occurrences in ascending position (reverse: in
    descending position, for the order-sensitivity check), then added onto the zero table."""
    tok = np.asarray(tokens).reshape(-1)
    g = np.asarray(dout, F32).reshape(len(tok), -1)[:, col_off:col_off + dim]
    out = np.zeros((rows, dim), F32)
    for k in np.unique(tok):
        if k < 0 or k >= rows or k == padding_idx:
            continue
        pos = np.nonzero(tok == k)[0]
        if reverse:
            pos = pos[::-1]
        acc = np.zeros(dim, F32)
        for j in pos:
            acc = (acc + g[j]).astype(F32)
        out[k] = (out[k] + acc).astype(F32)
    return out


EMB_ROWS = 40
EMB_PAD = 0


def embedding_bwd_tokens(seed=0):
    """1000 positions over a 40-row table: token 31 first occurs at position 600 (the third 256-token chunk), token 32 at positions 3 and 700 (more
    than 256 apart), token 33 at 300 random positions, the padding row 0, and the out-of-range tokens -1, 40 and 2^40 (ignored)."""
    rs = np.random.RandomState(99 + seed)
    tok = rs.randint(0, 31, size=1000).astype(np.int64)              # 0 (padding) .. 30
    free = np.setdiff1d(np.arange(1000), [600, 601, 900, 3, 700, 10, 520, 999])
    tok[rs.choice(free, size=300, replace=False)] = 33
    tok[[600, 601, 900]] = 31
    tok[[3, 700]] = 32
    tok[[10, 520, 999]] = [-1, EMB_ROWS, 1 << 40]
    return tok


def embedding_bwd_big_tokens(seed=0):
    """65 539 positions, 50 distinct tokens: more positions than the 65 535 workgroups of the grid"""
    rs = np.random.RandomState(7 + seed)
    return rs.randint(1, 51, size=65539).astype(np.int64)
