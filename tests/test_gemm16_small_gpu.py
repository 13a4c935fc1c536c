"""The small tiles of the plain-bf16 GEMM (csrc/cti_gemm16.hip: G16Small = 128 x 128 tile on an 8-slot LDS ring, G16Tall = 256 x 128 on a 6-slot ring; the
default route of gemm_nt_planes() for the model forwards' mid-size products since round 6 -- FCNet.forward of reference src/fc.py:33-34 in the
precision='bf16' mode) against float64 on bf16-ROUNDED operands, EVERY entry, as tests/test_gemm16_gpu.py does for the 256 x 256 tile: with the operands
rounded the only error left is the fp32 accumulation order (3e-6 of the largest entry; 4e-3 for bf16 rows out: one rounding to 8 bits), so a wrong tile /
wave / lane mapping, a missed ring wait or a lost epilogue constant shows as an O(1) error somewhere.

Every case names the route it means to test and asserts it through ops.last_gemm_route() (CTI_TUNE_LAST_GEMM_ROUTE): which kernel ran, on which tile, from
which form of A, into which epilogue.  Two routes reach the small tiles entry by entry:
  * "planes": ops.gemm_nt(..., prec='bf16', B_planes=...) under ops.tuning(gemm_cfg=0 / 1): A split into planes first.  Needs nb * M > 256 (fewer rows are handed
    over as fp32 rows, which cti_gemm16.hip does not read) and N % 4 == 0; where plan_ksplit splits K (K >= 256 and at most 96 tiles of 128 x 128) the inner,
    constant-free product reaches the kernel and the reduce kernel applies scale / bias / ReLU;
  * "rows": ops.gemm_bf16_rows(...) under the same forced geometry: A read as bf16 rows, fp32 or bf16 rows out.
(The planes epilogue is met through the fused TCNet.forward only: test_gemm16_gpu.py::test_planes_epilogue_through_the_fused_forward.)

The rule under test besides the numbers: bias / scale of a tile travel through a DOUBLE buffer in LDS that the issue side -- NS - 1 stages ahead of the compute
side -- refills when it opens the tile after next, so a product with bias or scale needs K / 32 >= NS stages per tile (8 / 6 / 4 for the 128 x 128 /
256 x 128 / 256 x 256 tile): below that the planes route falls back to the planes kernel of cti_gemm_bf16x3.hip and the rows route refuses the call.  Before
that rule knew the tile (it asked for 4 stages whatever the ring) a workgroup with three or more tiles could apply tile p + 2's constants to tile p.

A workgroup owns tiles w, w + 256, w + 512, ...; tile_coords (csrc/cti_common.h) maps a step of 256 tile ids to a step of 32 in the XCD-chunked order, so when
the number of column tiles divides 32 all tiles of a workgroup share their column block and a swapped bias would be invisible: the multi-tile shapes have
N = 3072 (24 column tiles), 3000, 4112 (33) or 520 x 3 -- never a divisor of 32 -- except where a model's own shape is the point.  Needs an MI355X."""
import pytest
import torch

import cti_amd

pytestmark = pytest.mark.gpu
DEV = "cuda"
ops = cti_amd.ops
NS = {0: 8, 1: 6, 2: 4}                      # ring slots of the tile behind each cfg
TILE = {0: (128, 128), 1: (256, 128), 2: (256, 256)}


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def reference(a, w, M, N, nb, s, scale_div, scale_bs, b, bias_bs, relu):
    """float64: C[z][m, n] = act(scale[z * scale_bs + n // scale_div] * sum_k a[m, k] w[z * N + n, k] + bias[z * bias_bs + n]) for the calls below (rA1 = 0, rB1 = N)"""
    ref = (a.double() @ w.double().t()).view(M, nb, N).permute(1, 0, 2)
    cols = torch.arange(N)
    if s is not None:
        ref = ref * torch.stack([s[z * scale_bs + cols // scale_div] for z in range(nb)]).double()[:, None, :]
    if b is not None:
        ref = ref + torch.stack([b[z * bias_bs + cols] for z in range(nb)]).double()[:, None, :]
    return torch.relu(ref) if relu else ref


def _product(route, cfg, M, N, K, nb=1, scale=False, bias=False, relu=False, out_dtype=torch.float32, scale_div=1, twice=False):
    """One product on `route` ('planes' / 'rows') with tile `cfg` forced (None: the library's own choice).  Returns (error relative to the largest reference entry over
    EVERY entry, the route word).  twice: launched again, the same bits."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + nb)                      # seeded from the shape
    a = bf16r(torch.randn(M, K, generator=g))
    w = bf16r(torch.randn(nb * N, K, generator=g) / 4)
    sbs = (N + scale_div - 1) // scale_div
    s = (torch.rand(nb * sbs, generator=g) + 0.5) if scale else None
    b = torch.randn(nb * N, generator=g) if bias else None
    kw = dict(nb1=nb, rA1=0, rB1=N, M=M, N=N, scale=None if s is None else s.to(DEV), scale_div=scale_div, scale_bs=sbs if scale else 0,
              bias=None if b is None else b.to(DEV), bias_bs=N if bias else 0, relu=relu)
    wd = w.to(DEV)
    wp = ops.split_operand(wd, prec="bf16")
    ad = a.to(DEV) if route == "planes" else a.to(torch.bfloat16).to(DEV)

    def run():
        if route == "planes":
            return ops.gemm_nt(ad, wd, prec="bf16", B_planes=wp, **kw)
        return ops.gemm_bf16_rows(ad, wp, nb * N, out_dtype=out_dtype, **kw)

    def forced():
        if cfg is None:
            return run(), ops.last_gemm_route()
        with ops.tuning(gemm_cfg=cfg):
            return run(), ops.last_gemm_route()
    y, word = forced()
    assert y.dtype == out_dtype
    if twice:
        y2, _ = forced()
        assert torch.equal(y, y2), "two launches of the same product differ"
    ref = reference(a, w, M, N, nb, s, scale_div, sbs, b, N, relu)
    err = float((y.double().cpu().view(nb, M, N) - ref).abs().max() / ref.abs().max())
    return err, word


def _check(route, cfg, M, N, K, expect, **kw):
    """expect: 'gemm16' = cti_gemm16.hip on tile cfg, whole K; 'split_k' = the same kernel on the partials of a split-K; 'planes' = the fallback, the planes kernel of
    cti_gemm_bf16x3.hip on tile cfg; 'refused' = the rows route has no fallback: the call must raise, not compute"""
    out_dtype = kw.get("out_dtype", torch.float32)
    if expect == "refused":
        with pytest.raises(cti_amd.pkg._lib.CtiError, match="K / 32 >= %d with bias or scale" % NS[cfg]):      # THIS refusal: the ring-depth rule's own message
            _product(route, cfg, M, N, K, **kw)
        return
    err, word = _product(route, cfg, M, N, K, **kw)
    print("gemm16 small %s cfg=%s %dx%dx%d nb=%d %s: err %.2e route %s" % (route, cfg, M, N, K, kw.get("nb", 1), str(out_dtype).split(".")[-1], err, word))
    assert word is not None
    assert word["kernel"] == ("planes" if expect == "planes" else "gemm16"), word
    if cfg is not None:
        assert word["cfg"] == cfg, word
    assert word["a_form"] == ("planes" if route == "planes" else "bf16_rows"), word
    assert word["epi"] == ("bf16" if out_dtype == torch.bfloat16 else "f32"), word
    assert word["split_k"] == (expect == "split_k"), word
    assert err < (3e-6 if out_dtype == torch.float32 else 4e-3), err


def _with_constants(route, cfg, K):
    """where a product WITH bias or scale runs: the ring-depth rule of the module docstring"""
    if K // 32 >= NS[cfg]:
        return "gemm16"
    return "planes" if route == "planes" else "refused"


CONSTS = [dict(), dict(scale=True, bias=True, relu=True)]
CONST_IDS = ["plain", "scale-bias-relu"]


@pytest.mark.parametrize("consts", CONSTS, ids=CONST_IDS)
@pytest.mark.parametrize("K", [32, 64, 96, 128, 160])
@pytest.mark.parametrize("cfg", [0, 1])
def test_fewer_stages_than_ring_slots(cfg, K, consts):
    """the ring's prologue / tail only: ONE tile on the rows route (the planes route has no one-tile case: at most 256 rows go as fp32 rows) and 300 x 132 on the
    planes route (ragged rows, 4 live columns in the last column tile).  With bias or scale every one of these has fewer stages than the ring has slots: the fallback
    kernel must be right (planes route), the rows route must refuse."""
    bm, bn = TILE[cfg]
    _check("rows", cfg, bm, bn, K, _with_constants("rows", cfg, K) if consts else "gemm16", **consts)
    _check("planes", cfg, 300, 132, K, _with_constants("planes", cfg, K) if consts else "gemm16", **consts)


@pytest.mark.parametrize("consts", CONSTS, ids=CONST_IDS)
@pytest.mark.parametrize("cfg,K", [(0, 224), (0, 256), (0, 288), (1, 160), (1, 192), (1, 224)])
def test_ring_depth_boundary(cfg, K, consts):
    """nk = NS - 1, NS, NS + 1 stages per tile: one tile (rows route) and 9216 x 3072 (planes route; 1 728 / 864 tiles, 24 column tiles; K >= 256 does not split: more
    than 96 tiles).  With constants nk = NS - 1 is the last depth the double buffer cannot serve."""
    bm, bn = TILE[cfg]
    expect_c = "gemm16" if K // 32 >= NS[cfg] else None
    _check("rows", cfg, bm, bn, K, (expect_c or "refused") if consts else "gemm16", **consts)
    _check("planes", cfg, 9216, 3072, K, (expect_c or "planes") if consts else "gemm16", twice=True, **consts)


@pytest.mark.parametrize("K", [128, 160, 192, 224])
@pytest.mark.parametrize("cfg", [0, 1])
def test_epilogue_constants_under_a_deep_ring(cfg, K):
    """9216 x 3072 with scale AND bias random per column (scale_div = 1): 1 728 tiles of 128 x 128 = 6-7 per workgroup, 864 of 256 x 128 = 3-4; 24 column tiles, so the
    tiles of one workgroup lie in different column blocks.  K = 128 .. 224 are the depths at which the 4-stage rule let these through to cti_gemm16.hip, whose
    constants' double buffer then held tile p + 2's values when tile p's epilogue read it (K = 128: overwritten three intervals before the read; nk = NS - 1: in the
    same interval).  Observed at the parent commit's library on an MI355X: errors of 0.60 .. 0.70 of the largest entry on every row with nk < NS, 2.2e-7 on the two
    others (profiles/gemm16_small_tiles_tests.txt).  Now: nk < NS runs on the fallback kernel,
    nk >= NS (cfg 1 at K = 192, 224) stays on cti_gemm16.hip; the numbers are checked either way."""
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the shape is chosen for 256 compute units")
    expect = _with_constants("planes", cfg, K)
    assert expect == ("gemm16" if (cfg, K) in ((1, 192), (1, 224)) else "planes")
    _check("planes", cfg, 9216, 3072, K, expect, scale=True, bias=True, relu=False, twice=True)
    _check("planes", cfg, 9216, 3072, K, expect, scale=True, bias=True, relu=True)


@pytest.mark.parametrize("K", [128, 160])
def test_epilogue_constants_on_the_default_route(K):
    """no forced geometry: gemm_nt_planes()'s makespan model gives 7744 x 4112 the 256 x 128 tile (1 023 tiles: four rounds at 2.86 beat three rounds of 527 tiles of
    256 x 256 at 4.0) -- four tiles per workgroup over 33 column tiles, 4 or 5 stages each on a 6-slot ring.  With bias + scale + ReLU this product now takes the
    fallback kernel ON THE SAME TILE (the route word's cfg says which tile the model picked)."""
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the makespan model's choice is stated for 256 compute units")
    err, word = _product("planes", None, 7744, 4112, K, scale=True, bias=True, relu=True, twice=True)
    print("gemm16 small default route 7744x4112x%d: err %.2e route %s" % (K, err, word))
    assert word["cfg"] == 1 and word["kernel"] == "planes" and word["a_form"] == "planes" and not word["split_k"], word
    assert err < 3e-6, err


@pytest.mark.parametrize("consts", CONSTS, ids=CONST_IDS)
@pytest.mark.parametrize("cfg", [0, 1])
def test_store_window_across_partial_edge_tiles(cfg, consts):
    """9000 x 3000 x 512: the last row tile (40 of 128 rows / 40 of 256) and the last column tile (56 of 128 columns) are partial, so a workgroup's stream of tiles
    switches the counted store window (full tiles with nk > NS - 2 only) on and off; 24 column tiles"""
    _check("planes", cfg, 9000, 3000, 512, "gemm16", twice=True, **consts)
    _check("rows", cfg, 9000, 3000, 512, "gemm16", twice=True, **consts)


@pytest.mark.parametrize("consts", CONSTS, ids=CONST_IDS)
@pytest.mark.parametrize("cfg", [0, 1])
def test_ragged_edges_that_reach_the_kernel(cfg, consts):
    """N % 4 == 0, so cti_gemm16.hip takes them (N % 4 != 0 never does: test_gemm16_gpu.py pins that fallback): 1000 x 776 (a last row tile of 104 / 232 rows, a last
    column tile of 8 columns), 513 x 260 (ONE live row in the last row tile, 4 live columns in the last column tile), 257 x 132"""
    c = bool(consts)
    _check("planes", cfg, 1000, 776, 224, _with_constants("planes", cfg, 224) if c else "gemm16", twice=True, **consts)      # (56 tiles of 128 x 128, K < 256: no split-K)
    _check("rows", cfg, 1000, 776, 320, "gemm16", twice=True, **consts)                                                       # (the rows route never splits K)
    _check("planes", cfg, 513, 260, 160, _with_constants("planes", cfg, 160) if c else "gemm16", twice=True, **consts)
    _check("rows", cfg, 513, 260, 160, _with_constants("rows", cfg, 160) if c else "gemm16", **consts)
    _check("planes", cfg, 257, 132, 224, _with_constants("planes", cfg, 224) if c else "gemm16", twice=True, **consts)
    _check("rows", cfg, 257, 132, 288, "gemm16", twice=True, **consts)


@pytest.mark.parametrize("cfg", [0, 1])
def test_batches_with_per_batch_bias_and_scale(cfg):
    """scale[b1 * scale_bs + n / scale_div] with scale_div = 8 and bias[b1 * bias_bs + n], three and two weight sets: 700 x 520 x 224 x 3 (at K = 256 its 90 tiles would
    be split; 5 column tiles a batch) and 3072 x 1024 x 1024 x 2 (the c3 forward's shape in profiles/r06_gemm_mid_size.txt; 384 tiles: no split)"""
    kw = dict(scale=True, bias=True, relu=True, scale_div=8, twice=True)
    _check("planes", cfg, 700, 520, 224, _with_constants("planes", cfg, 224), nb=3, **kw)
    _check("rows", cfg, 700, 520, 256, "gemm16", nb=3, **kw)
    _check("planes", cfg, 3072, 1024, 1024, "gemm16", nb=2, **kw)
    _check("rows", cfg, 3072, 1024, 1024, "gemm16", nb=2, **kw)


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("M,N,K,nb,expect", [
    (9216, 512, 512, 1, "gemm16"), (3584, 512, 512, 1, "gemm16"),
    (768, 512, 512, 1, "split_k"),             # 24 tiles of 128 x 128: plan_ksplit cuts K in four; cti_gemm16.hip writes the partials, the reduce kernel applies the constants
    (3584, 1024, 1024, 2, "gemm16"),
])
def test_the_shapes_the_models_run(cfg, M, N, K, nb, expect):
    """the c3 / c4 forwards' products (profiles/r06_model_c3_kernel_stats.txt), with the layer's weight-norm scale (one per weight set: scale_div = N), bias and ReLU.
    (4 or 8 column tiles: these are the models' own shapes, not chosen to expose a swapped constant.)"""
    _check("planes", cfg, M, N, K, expect, nb=nb, scale=True, bias=True, relu=True, scale_div=N, twice=True)
    _check("rows", cfg, M, N, K, "gemm16", nb=nb, scale=True, bias=True, relu=True, scale_div=N, twice=True)


@pytest.mark.parametrize("cfg", [0, 1])
def test_bf16_rows_out_with_odd_tails(cfg):
    """EPI_BF16 (8-B stores, 2-B tails): 513 x 260 x 160 (without constants: five stages cannot carry them on these rings) and 2305 x 1024 x 2048 with bias + ReLU"""
    _check("rows", cfg, 513, 260, 160, "gemm16", out_dtype=torch.bfloat16, twice=True)
    _check("rows", cfg, 513, 260, 256, "gemm16", out_dtype=torch.bfloat16, scale=True, bias=True, relu=True, twice=True)
    _check("rows", cfg, 2305, 1024, 2048, "gemm16", out_dtype=torch.bfloat16, bias=True, relu=True, twice=True)
