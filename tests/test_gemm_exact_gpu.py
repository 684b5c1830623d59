"""Every bf16-weight GEMM launch path against the exact-arithmetic oracle (tests/gemm_oracle.py):
integer operands with power-of-two row scales whose products and partial sums are exact in
fp32, so slabs, bf16 outputs and LM-head picks are fixed to the bit and compared with zero
tolerance.  SwiGLU / bias / GELU / residual epilogues get the exact product as input and the
row-op oracle's per-element bf16 rule.

Every case launches three times (ring races are intermittent) and compares each result; X is
rows 1..M of a buffer whose other rows, through the next multiple of 16 past M and one tile
more, are NaN -- a GEMM row depends on its own X row only, so a NaN in the output is a tail row
mixed in; and the output must have exactly the oracle's shape.

Instantiations the launchers dispatch at default knobs, and the case that reaches each:

  dgemm.hip  dgemm_kernel<EPI, MT, NT>      MT in {1, 2, 4, 8, 12}: M in RING_M (1, 16 | 17, 32 |
                                            33, 64 | 65, 128 | 129, 192)
    EPI_BF16     NT 4                       test_ring_bf16 (S = 1), with splitk_reduce (S = 2)
    EPI_PARTIAL  NT 4 / NT 8                test_ring_slabs tile 64 / 128 (XCD remap at N = 256)
    EPI_GLU      NT 4 / NT 7, MT <= 8       test_ring_glu N = 128 / N = 21504 (N / 112 >= 192)
    EPI_ARGMAX   NT 4                       test_ring_argmax
    EPI_PARTIAL  MT 1, NORM                 test_ring_add_rmsnorm
    EPI_PARTIAL / EPI_GLU (NT 4, 7), XN     test_ring_xn
  dgemm.hip  gemv_kernel<R, C, EPI, XN, nt = true>
    EPI_PARTIAL  (16,1) (16,2) (8,2) (8,4) (4,4) (4,7) (8,1) (4,2) (4,1)   test_gemv_slabs
    EPI_GLU      (16,1) (16,2)              test_gemv_glu
    EPI_ARGMAX   (16,1) (16,2)              test_gemv_argmax (K = 2048 / 4096)
    XN           C <= 2 (K <= 4096)         test_gemv_xn
  mgemm.hip  mgemm_kernel, cfg 1..7         test_mgemm_bf16 / _slabs (remap 0: S = 2, remap 1:
                                            S = 8, remap 2: S = 16) / _slab16 / _glu (cfg 1..6:
                                            cfg 7 has 32 columns per wave and no SwiGLU) / _argmax
  pgemm.hip  pgemm_kernel<EPI>              test_pgemm_bf16 / _glu / _partial
  gemm.hip   gemm_kernel<EPI>               test_gemm_epilogues (epi 0..4)

Not covered: mgemm cfg 8..14 (probes: they skip the MFMAs or the fragment reads, or read a
stage-tiled weight copy, and do not compute the product from a plain weight), and the
instantiations selected by knobs that are read once per process.  The knobs are tested at
their defaults, asserted by test_knobs_at_defaults: DOCQA_DGEMM_NS unset (4-slot ring; the 6-
and 8-slot rings are not run), DOCQA_GLU_NT unset (112-row SwiGLU tiles where N / 112 >= 192),
DOCQA_DGEMM_XA unset (X one stage ahead; the 3-ahead MT = 8 variant is not run), DOCQA_DGEMM_XCD
unset (XCD slice remap on), DOCQA_GEMV_NT unset (non-temporal weight loads; the nt = false GEMV
instantiations are not run).

The quantized SwiGLU entry points (gemv8, gemv4, dgemm8_glu, dgemm8w_glu, dgemm4_glu) share the
silu helper: each gets one planted overflow case (test_quantized_glu_overflow)."""
import functools
import os

import pytest
import torch

from docqa_amd import ops
from tests import gemm_oracle as G
from tests import rowop_oracle as RO

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# ----------------------------------------------------------------------------- case tables
# (imported by tests/test_gemm_oracle_cpu.py, which proves the certificate for every entry)
RING_M = (1, 16, 17, 32, 33, 64, 65, 128, 129, 192)
RING_KS = ((512, 1), (1024, 1), (1024, 2), (2048, 2))          # K / S in {512, 1024}: one, two ring turns
RING_SLABS = [(t, M, 128, K, S) for t in (64, 128) for M in RING_M for K, S in RING_KS]
RING_SLABS += [(t, M, 256, 1024, 2) for t in (64, 128) for M in (1, 33, 129)]     # XCD slice remap
RING_GLU = [(M, 128, K) for M in RING_M if M <= 128 for K in (512, 1024)]
RING_GLU += [(M, 21504, 512) for M in (1, 17, 33, 65, 128)]                        # 112-row tiles
RING_ARGMAX = [(M, 256, K, 200) for M in RING_M for K in (512, 1024)]
RING_ARGMAX += [(M, 256, 512, nv) for M in (1, 17, 129) for nv in (40, 256)]       # first tile / all valid
RING_NORM = [(M, 128, K, S) for M in (1, 2, 4) for K, S in ((512, 1), (1024, 2))]
RING_XN = [(128, 512, 1, 1), (128, 1024, 2, 2), (128, 1024, 1, 5), (128, 512, 0, 2), (21504, 512, 0, 3)]

GEMV_RC = ((16, 1), (16, 2), (8, 2), (8, 4), (4, 4), (4, 7), (8, 1), (4, 2), (4, 1))
GEMV_SLABS = [(R, C, S) for R, C in GEMV_RC for S in (1, 2)]
GEMV_GLU = [(1, False), (1, True), (2, False), (2, True)]                          # (C, one-hot X)
GEMV_ARGMAX = [(K, nv, swap) for K in (2048, 4096) for nv in (40, 12) for swap in (False, True)]
GEMV_XN = [(R, C, S) for R, C in GEMV_RC if C <= 2 for S in (1,)] + [(8, 1, 2)]

MG_BN = {1: 128, 2: 128, 3: 256, 4: 256, 5: 256, 6: 256, 7: 64}
MG_BKS = {1: 64, 2: 64, 3: 32, 4: 32, 5: 64, 6: 64, 7: 64}
MG_WN = {1: 2, 2: 2, 3: 4, 4: 2, 5: 2, 6: 4, 7: 2}              # waves along N: BN / WN columns per wave
MG_M = (1, 255, 256, 257, 512)
MG_CFG = tuple(range(1, 8))


def mg_ks(cfg):
    """K per slice: one stage pair, and enough pairs that every ring (2..4 slots) wraps twice."""
    return (2 * MG_BKS[cfg], 512)


MG_BF16 = [(c, M, ks) for c in MG_CFG for M in MG_M for ks in mg_ks(c)]
MG_SLABS = [(c, M, ks, S) for c in MG_CFG for M in MG_M for ks in mg_ks(c) for S in (2, 8)]
MG_SLABS += [(2, M, 128, 16) for M in (1, 257)]                                    # remap 2
MG_SLABS += [(0, M, 512, 1) for M in (193, 256)]                                   # S = 1 fp32: dgemm_partial at 193..256 rows
MG_SLAB16 = [(c, M, ks, S) for c in MG_CFG for M in MG_M for ks in mg_ks(c) for S in (1, 2, 8)]
MG_GLU = [(c, M, ks) for c in MG_CFG if MG_BN[c] // MG_WN[c] >= 64 for M in MG_M for ks in mg_ks(c)]
MG_ARGMAX = [(c, M, ks, nv) for c in MG_CFG for M in MG_M for ks in mg_ks(c) for nv in ("mid", 40)]

PG_M = (1, 255, 256, 257, 513)
PG_N = (256, 512)
PG_K = (128, 256, 1024)
PG_BF16 = [(M, N, K) for M in PG_M for N in PG_N for K in PG_K]
PG_PARTIAL = [(M, N, K, S) for M, N, K in PG_BF16 for S in (1, 2, 4) if K % (S * 128) == 0]

GEMM_SHAPES = [(M, N, K) for M in (1, 127, 128, 129, 300) for N in (128, 384) for K in (64, 128, 384)]
GEMM_WSHIFT = -15            # brings the products (~2^16) into the GELU's interesting range

RANDN = [("ring_slabs", 33, 128, 1024, 2), ("ring_bf16", 17, 128, 1024, 1), ("gemv", 1, 32, 4096, 1),
         ("mgemm_slabs", 257, 256, 1024, 2), ("mgemm_bf16", 257, 512, 512, 1), ("mgemm_slab16", 255, 256, 1024, 2),
         ("pgemm_bf16", 257, 256, 1024, 1), ("pgemm_partial", 255, 256, 1024, 2), ("gemm", 129, 128, 384, 1)]


def fill_keys():
    """Every (M, N, K, S, wide, wshift) fill the cases below build: the CPU test asserts the
    certificate for each."""
    keys = set()

    def add(M, N, K, S, wshift=0):
        for wide in G.fills(K, S):
            keys.add((M, N, K, S, wide, wshift))

    for M in RING_M:
        for K, _ in RING_KS:
            add(M, 128, K, 1)
    for _, M, N, K, S in RING_SLABS:
        add(M, N, K, S)
    for M, N, K in RING_GLU:
        add(M, N, K, 1)
    for M, N, K, _ in RING_ARGMAX:
        add(M, N, K, 1)
    for M, N, K, S in RING_NORM:
        add(M, N, K, S)
    for R, C, S in GEMV_SLABS:
        add(1, 4 * R, 2048 * C * S, S)
    for C, _ in GEMV_GLU:
        add(1, 64, 2048 * C, 1)
    for K, _, _ in GEMV_ARGMAX:
        add(1, 64, K, 1)
    for c, M, ks in MG_BF16:
        add(M, 2 * MG_BN[c], ks, 1)
    for c, M, ks, S in MG_SLABS + MG_SLAB16:
        add(M, 2 * MG_BN[c or 2], ks * S, S)
    for M, N, K in PG_BF16:
        add(M, N, K, 1)
    for M, N, K, S in PG_PARTIAL:
        add(M, N, K, S)
    for M, N, K in GEMM_SHAPES:
        add(M, N, K, 1)
        add(M, N, K, 1, GEMM_WSHIFT)
    return sorted(keys)


# ----------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module", autouse=True)
def native():
    assert ops.load_native(build_if_missing=True)
    return ops


@functools.lru_cache(maxsize=4)
def _fill(M, N, K, S, wide, wshift=0):
    return G.exact_xw(M, N, K, S, seed=K // 64 + S, wide=wide, wshift=wshift, device="cuda")


def _certified(f):
    """The certificate again, on the tensors the kernel is about to read."""
    G.certificate(f)
    return f


def _poisoned(x):
    """x as rows 1..M of a NaN buffer (through the next multiple of 16 past M and one tile
    more); the row offset keeps the 16-byte alignment the bindings check."""
    M, K = x.shape
    buf = torch.full(((M + 15) // 16 * 16 + 17, K), float("nan"), dtype=BF16, device=x.device)
    buf[1:M + 1] = x
    v = buf[1:M + 1]
    assert v.is_contiguous() and v.data_ptr() % 16 == 0
    return v


def _three(fn, check):
    for i in range(3):
        check(fn(), f"launch {i}")


def _bits(fn, want, what, ksize=None):
    _three(fn, lambda got, tag: G.assert_bits(got, want, what=f"{what} {tag}", ksize=ksize))


def _rule(fn, y, m, what):
    def check(got, tag):
        assert got.dtype == BF16 and got.shape == y.shape, f"{what}: output {tuple(got.shape)} {got.dtype}"
        RO.assert_oracle(got, y, m, what=f"{what} {tag}")
    _three(fn, check)


def _argmax(fn, f, n_valid, what):
    ids, vals = G.argmax(f.x, f.w, n_valid)

    def check(got, tag):
        gi, gv = got if isinstance(got, tuple) else (got, None)
        assert gi.dtype == torch.int64 and gi.shape == ids.shape
        bad = (gi != ids).nonzero().flatten().tolist()
        assert not bad, (f"{what} {tag}: {len(bad)} of {ids.numel()} rows pick another id; row {bad[0]}: "
                         f"got {int(gi[bad[0]])}, want {int(ids[bad[0]])}")
        if gv is not None:
            G.assert_bits(gv, vals, what=f"{what} {tag} values")
    _three(fn, check)


def _nv(nv, bn):
    return bn + bn // 2 if nv == "mid" else nv


def test_knobs_at_defaults():
    for k in ("DOCQA_DGEMM_NS", "DOCQA_GLU_NT", "DOCQA_DGEMM_XA", "DOCQA_DGEMM_XCD", "DOCQA_GEMV_NT"):
        assert k not in os.environ, f"{k} is set: the instantiation table in this file is for the defaults"


# ----------------------------------------------------------------------------- ring kernel
@pytest.mark.parametrize("K,S", RING_KS)
@pytest.mark.parametrize("M", RING_M)
def test_ring_bf16(M, K, S):
    for wide in G.fills(K):
        f = _certified(_fill(M, 128, K, 1, wide))
        x = _poisoned(f.x)
        _bits(lambda: torch.ops.docqa.dgemm(x, f.w, S), G.product_bf16(f.x, f.w), f"dgemm S={S} fill {wide}")


@pytest.mark.parametrize("tile,M,N,K,S", RING_SLABS)
def test_ring_slabs(tile, M, N, K, S):
    f = _certified(_fill(M, N, K, S, "x"))
    x = _poisoned(f.x)
    _bits(lambda: ops.dgemm_partial(x, f.w, S, tile), G.slabs(f.x, f.w, S), f"dgemm_partial tile {tile}", K // S)


@pytest.mark.parametrize("M,N,K", RING_GLU)
def test_ring_glu(M, N, K):
    base = _fill(M, N, K, 1, "x")
    for f in [G.plant_glu(base)] + ([base] if M in (1, 16) else []):
        x = _poisoned(_certified(f).x)
        _rule(lambda: torch.ops.docqa.dgemm_glu(x, f.w), *G.glu(f.x, f.w), "dgemm_glu")


@pytest.mark.parametrize("M,N,K,n_valid", RING_ARGMAX)
def test_ring_argmax(M, N, K, n_valid):
    f = _certified(G.plant_argmax(_fill(M, N, K, 1, "x"), n_valid, 64))
    x = _poisoned(f.x)
    _argmax(lambda: tuple(torch.ops.docqa.dgemm_argmax_val(x, f.w, n_valid)), f, n_valid, "dgemm_argmax_val")


@pytest.mark.parametrize("M,N,K,S", RING_NORM)
def test_ring_add_rmsnorm(M, N, K, S):
    """The fused projection + add + RMSNorm == its unfused pair bit for bit, and the unfused
    pair's slabs are the exact ones."""
    f = _certified(_fill(M, N, K, S, "x"))
    x = _poisoned(f.x)
    P = ops.dgemm_partial(x, f.w, S, 64)
    G.assert_bits(P, G.slabs(f.x, f.w, S), what="dgemm_partial", ksize=K // S)
    gam = RO.make_weight(N, 7, "cuda")
    r0 = RO.make_rows(M, N, 8, "cuda")
    r_ref = r0.clone()
    o_ref = ops.add_rmsnorm_splitk(P, r_ref, gam, 1e-5)
    tick = torch.zeros(1, device="cuda", dtype=torch.int32)
    for _ in range(3):
        r = r0.clone()
        o = ops.dgemm_add_rmsnorm(x, f.w, S, r, gam, 1e-5, tick)
        assert torch.equal(RO.bits(o), RO.bits(o_ref)) and torch.equal(RO.bits(r), RO.bits(r_ref))
        assert int(tick.item()) == 0


def _xn_case(N, K, S, Sin, onehot):
    """(Pin, res_in, gamma, fill) of an in-kernel input row that is known exactly: slabs that
    sum to 2 r and a residual of -r or -3 r with r = +-1, so the summed row h is +-1 everywhere,
    its mean square is 1 and the normed row is h * gamma -- gamma's odd integers (or, ``onehot``,
    a single 1 under the SwiGLU overflow plants), exact in bf16 whatever the last bit of rsqrt."""
    g = torch.Generator().manual_seed(11 + K + Sin)
    r = (2 * torch.randint(0, 2, (K,), generator=g) - 1).double()
    extra = torch.randint(-3, 4, (max(Sin - 1, 0), K), generator=g).double()
    Pin = torch.cat([(2 * r - extra.sum(0))[None], extra])[:, None, :].float().contiguous()
    flip = torch.randint(0, 2, (K,), generator=g).double()
    r[5], flip[5] = 1.0, 0.0                                     # h[5] = +1: the one-hot column
    Pin[0, 0, 5] = 2.0 - float(extra[:, 5].sum())
    res = (-r - 2 * r * flip)[None]
    gamma = G._odd((K,), 127, g)
    if onehot:
        gamma = torch.zeros(K, dtype=torch.float64)
        gamma[5] = 1.0
    want_x = ((2 * r + res[0]) * gamma)[None].cuda()
    wf = _fill(1, N, K, max(S, 1), "x")
    f = G.finish(want_x, wf.wi, torch.ones(1, dtype=torch.float64, device="cuda"), wf.ws, max(S, 1))
    return Pin.cuda(), res.to(BF16).cuda(), gamma.to(BF16).cuda(), (G.plant_glu(f, 5) if onehot else f)


@pytest.mark.parametrize("N,K,S,Sin", RING_XN)
def test_ring_xn(N, K, S, Sin):
    """The in-kernel input row: == add_rmsnorm_splitk + the plain projection bit for bit, and
    (the row being known exactly) the slabs / SwiGLU it emits are the exact ones.  S = 0:
    dgemm_glu_xn, once on the integer row and once on a one-hot row over the overflow plants."""
    for onehot in ((False, True) if S == 0 else (False,)):
        Pin, r0, gam, f = _xn_case(N, K, S, Sin, onehot)
        _certified(f)
        r_ref = r0.clone()
        xrow = ops.add_rmsnorm_splitk(Pin, r_ref, gam, 1e-6)
        assert torch.equal(xrow.double(), f.x.double()), "the normed input row is not the planned one"
        ref = ops.dgemm_partial(xrow, f.w, S, 64) if S else torch.ops.docqa.dgemm_glu(xrow, f.w)
        for i in range(3):
            r_in, r_out = r0.clone(), torch.empty_like(r0)
            if S:
                got = ops.dgemm_partial_xn(Pin, r_in, r_out, gam, 1e-6, f.w, S)
                G.assert_bits(got, G.slabs(f.x, f.w, S), what=f"dgemm_partial_xn launch {i}", ksize=K // S)
            else:
                got = ops.dgemm_glu_xn(Pin, r_in, r_out, gam, 1e-6, f.w)
                RO.assert_oracle(got, *G.glu(f.x, f.w), what=f"dgemm_glu_xn launch {i}")
            assert torch.equal(r_in, r0) and torch.equal(RO.bits(r_out), RO.bits(r_ref))
            assert torch.equal(RO.bits(got), RO.bits(ref))


# ----------------------------------------------------------------------------- batch-1 GEMV
@pytest.mark.parametrize("R,C,S", GEMV_SLABS)
def test_gemv_slabs(R, C, S):
    N, K = 4 * R, 2048 * C * S
    for wide in G.fills(K, S):
        f = _certified(_fill(1, N, K, S, wide))
        x = _poisoned(f.x)
        _bits(lambda: torch.ops.docqa.gemv(x, f.w, S, R, False), G.slabs(f.x, f.w, S), f"gemv ({R},{C}) fill {wide}",
              K // S)


@pytest.mark.parametrize("C,onehot", GEMV_GLU)
def test_gemv_glu(C, onehot):
    N, K = 64, 2048 * C
    for wide in G.fills(K):
        f = _fill(1, N, K, 1, wide)
        f = _certified(G.plant_glu(f) if onehot else f)
        x = _poisoned(f.x)
        _rule(lambda: torch.ops.docqa.gemv(x, f.w, 1, 16, True), *G.glu(f.x, f.w), f"gemv glu (16,{C}) fill {wide}")


@pytest.mark.parametrize("K,n_valid,swap", GEMV_ARGMAX)
def test_gemv_argmax(K, n_valid, swap):
    for wide in G.fills(K):
        f = _certified(G.plant_argmax(_fill(1, 64, K, 1, wide), n_valid, 16, swap))
        x = _poisoned(f.x)
        _argmax(lambda: tuple(torch.ops.docqa.gemv_argmax_val(x, f.w, n_valid)), f, n_valid, f"gemv_argmax fill {wide}")


@pytest.mark.parametrize("R,C,S", GEMV_XN)
def test_gemv_xn(R, C, S):
    """The GEMV's in-kernel input row (see test_ring_xn): exact slabs, and at R = 16 the SwiGLU
    on the integer row and on the one-hot row."""
    K = 2048 * C * S
    for glu, onehot in [(False, False)] + ([(True, False), (True, True)] if R == 16 else []):
        N = 64 if glu else 4 * R
        Pin, r0, gam, f = _xn_case(N, K, 0 if glu else S, 3, onehot)
        _certified(f)
        r_ref = r0.clone()
        xrow = ops.add_rmsnorm_splitk(Pin, r_ref, gam, 1e-6)
        assert torch.equal(xrow.double(), f.x.double()), "the normed input row is not the planned one"
        for i in range(3):
            r_in, r_out = r0.clone(), torch.empty_like(r0)
            if glu:
                got = ops.gemv_glu_xn(Pin, r_in, r_out, gam, 1e-6, f.w)
                RO.assert_oracle(got, *G.glu(f.x, f.w), what=f"gemv_glu_xn launch {i}")
            else:
                got = ops.gemv_partial_xn(Pin, r_in, r_out, gam, 1e-6, f.w, S, R)
                G.assert_bits(got, G.slabs(f.x, f.w, S), what=f"gemv_partial_xn ({R},{C}) launch {i}", ksize=K // S)
            assert torch.equal(r_in, r0) and torch.equal(RO.bits(r_out), RO.bits(r_ref))


# ----------------------------------------------------------------------------- mid-M GEMM
@pytest.mark.parametrize("cfg,M,ks", MG_BF16)
def test_mgemm_bf16(cfg, M, ks):
    f = _certified(_fill(M, 2 * MG_BN[cfg], ks, 1, "x"))
    x = _poisoned(f.x)
    _bits(lambda: torch.ops.docqa.mgemm(x, f.w, 1, cfg), G.product_bf16(f.x, f.w), f"mgemm cfg {cfg}")


@pytest.mark.parametrize("cfg,M,ks,S", MG_SLABS)
def test_mgemm_slabs(cfg, M, ks, S):
    f = _certified(_fill(M, 2 * MG_BN[cfg or 2], ks * S, S, "x"))
    x = _poisoned(f.x)
    fn = (lambda: torch.ops.docqa.mgemm(x, f.w, S, cfg)) if cfg else (lambda: torch.ops.docqa.dgemm_partial(x, f.w, S, 64))
    _bits(fn, G.slabs(f.x, f.w, S), f"mgemm slabs cfg {cfg} S={S}", ks)


@pytest.mark.parametrize("cfg,M,ks,S", MG_SLAB16)
def test_mgemm_slab16(cfg, M, ks, S):
    f = _certified(_fill(M, 2 * MG_BN[cfg], ks * S, S, "x"))
    x = _poisoned(f.x)
    _bits(lambda: torch.ops.docqa.mgemm_slab16(x, f.w, S, cfg), G.slab16(f.x, f.w, S), f"mgemm_slab16 cfg {cfg} S={S}", ks)


@pytest.mark.parametrize("cfg,M,ks", MG_GLU)
def test_mgemm_glu(cfg, M, ks):
    base = _fill(M, 2 * MG_BN[cfg], ks, 1, "x")
    for f in [G.plant_glu(base)] + ([base] if M == 1 else []):
        x = _poisoned(_certified(f).x)
        _rule(lambda: torch.ops.docqa.mgemm_glu(x, f.w, cfg), *G.glu(f.x, f.w), f"mgemm_glu cfg {cfg}")


@pytest.mark.parametrize("cfg,M,ks,nv", MG_ARGMAX)
def test_mgemm_argmax(cfg, M, ks, nv):
    bn = MG_BN[cfg]
    n_valid = _nv(nv, bn)
    f = _certified(G.plant_argmax(_fill(M, 2 * bn, ks, 1, "x"), n_valid, bn))
    x = _poisoned(f.x)
    _argmax(lambda: tuple(torch.ops.docqa.mgemm_argmax_val(x, f.w, n_valid, cfg)), f, n_valid, f"mgemm_argmax_val cfg {cfg}")
    _argmax(lambda: torch.ops.docqa.mgemm_argmax(x, f.w, n_valid, cfg), f, n_valid, f"mgemm_argmax cfg {cfg}")


# ----------------------------------------------------------------------------- prefill GEMM
@pytest.mark.parametrize("M,N,K", PG_BF16)
def test_pgemm_bf16(M, N, K):
    f = _certified(_fill(M, N, K, 1, "x"))
    x = _poisoned(f.x)
    _bits(lambda: torch.ops.docqa.pgemm(x, f.w, 0), G.product_bf16(f.x, f.w), "pgemm")


@pytest.mark.parametrize("M,N,K", PG_BF16)
def test_pgemm_glu(M, N, K):
    base = _fill(M, N, K, 1, "x")
    for f in [G.plant_glu(base)] + ([base] if M == 1 else []):
        x = _poisoned(_certified(f).x)
        _rule(lambda: torch.ops.docqa.pgemm(x, f.w, 1), *G.glu(f.x, f.w), "pgemm glu")


@pytest.mark.parametrize("M,N,K,S", PG_PARTIAL)
def test_pgemm_partial(M, N, K, S):
    f = _certified(_fill(M, N, K, S, "x"))
    x = _poisoned(f.x)
    _bits(lambda: ops.pgemm_partial(x, f.w, S), G.slabs(f.x, f.w, S), f"pgemm_partial S={S}", K // S)


# ----------------------------------------------------------------------------- encoder GEMM
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_epilogues(M, N, K, epi):
    f = _fill(M, N, K, 1, "x", GEMM_WSHIFT if epi in (1, 2, 3) else 0)
    if epi == 4:
        f = G.plant_glu(f)
    x = _poisoned(_certified(f).x)
    bias = RO.make_weight(N, 61 + N, "cuda") if epi in (1, 2, 3) else None
    res = RO.make_rows(M, N, 62 + N, "cuda") if epi == 3 else None
    fn = lambda: torch.ops.docqa.gemm(x, f.w, bias, res, epi)
    if epi == 0:
        _bits(fn, G.product_bf16(f.x, f.w), "gemm epi 0")
    else:
        _rule(fn, *G.gemm_epi(f.x, f.w, bias, res, epi), f"gemm epi {epi}")


# ----------------------------------------------------------------------------- secondary class
@pytest.mark.parametrize("kind,M,N,K,S", RANDN)
def test_random_significands(kind, M, N, K, S):
    """N(0,1) operands: one fp32 rounding per added term is the worst case of any order."""
    x0, w = G.randn_xw(M, N, K, seed=K + M, device="cuda")
    x = _poisoned(x0)
    y, m = G.randn_bound(x0, w, S)
    fn = {"ring_slabs": lambda: ops.dgemm_partial(x, w, S, 64),
          "ring_bf16": lambda: torch.ops.docqa.dgemm(x, w, 1),
          "gemv": lambda: torch.ops.docqa.gemv(x, w, S, 8, False),
          "mgemm_slabs": lambda: torch.ops.docqa.mgemm(x, w, S, 2),
          "mgemm_bf16": lambda: torch.ops.docqa.mgemm(x, w, 1, 6),
          "mgemm_slab16": lambda: torch.ops.docqa.mgemm_slab16(x, w, S, 2),
          "pgemm_bf16": lambda: torch.ops.docqa.pgemm(x, w, 0),
          "pgemm_partial": lambda: ops.pgemm_partial(x, w, S),
          "gemm": lambda: torch.ops.docqa.gemm(x, w, None, None, 0)}[kind]
    got = fn()
    if got.dim() == 2:
        y, m = y.sum(0), m.sum(0)
    RO.assert_oracle(got, y, m, slack=(K // S if got.dim() == 3 else K) * 2.0 ** -24, what=kind)


# ----------------------------------------------------------------------------- quantized SwiGLU
HOT = (5, 9, 37, 41)          # X columns: 5, 9 in the first 32-block (MXFP4 scale 16), 37, 41 in the second
# gate = sum over HOT of the row's entries: -96 + 6, -96 + 4 + 4, -96 + 16, 96 - 6 -- every term an
# e4m3 and an e2m1-times-block-scale value
Q_GATES = ((-96.0, 0.0, 6.0, 0.0), (-96.0, 0.0, 4.0, 4.0), (-96.0, 16.0, 0.0, 0.0), (96.0, 0.0, -6.0, 0.0))


def _quantized_case(fmt, M, N, K):
    """x [M, K] with ones (row m: 2^-(m % 3)) at HOT and zero elsewhere; W' a random image of the
    format whose first 16 rows (gate rows 0..7, up rows 8..15) are zero except at HOT, where they
    sum to the gates -90, -88, -80, +90 and the ups 2^8, 2^-8.  Every output is a sum of four
    terms of a few bits: exact in fp32 in any order, for any weight format."""
    quant, dequant = (ops.quantize_fp8_rows, ops.dequantize_fp8_rows) if fmt == "fp8" else \
        (ops.quantize_mxfp4_rows, ops.dequantize_mxfp4_rows)
    g = torch.Generator().manual_seed(K + N)
    w = dequant(*quant((torch.randn(N, K, generator=g) / 8).to(BF16).cuda()), BF16)
    w[:16] = 0
    for j in range(8):
        w[j, list(HOT)] = torch.tensor(Q_GATES[j % 4], dtype=BF16, device="cuda")
        w[8 + j, HOT[0]] = G.GLU_UPS[j // 4]
    q, s = quant(w)
    assert torch.equal(dequant(q, s, BF16), w), "the planted rows are not values of the format"
    x = torch.zeros(M, K, dtype=BF16, device="cuda")
    x[:, list(HOT)] = torch.exp2(-(torch.arange(M, device="cuda") % 3).float()).to(BF16)[:, None]
    gu = G.product_bf16(x, w)
    assert gu[0, :16].tolist() == [-90.0, -88.0, -80.0, 90.0] * 2 + [256.0] * 4 + [2.0 ** -8] * 4
    return x, q, s, RO.silu_mul(gu.to(BF16), interleaved=True)


@pytest.mark.parametrize("entry", ["gemv8", "gemv4", "dgemm8_glu", "dgemm8w_glu", "dgemm4_glu"])
def test_quantized_glu_overflow(entry):
    fmt = "fp4" if "4" in entry else "fp8"
    M, N, K = {"gemv8": (1, 64, 2048), "gemv4": (1, 64, 2048), "dgemm8_glu": (5, 128, 1024),
               "dgemm8w_glu": (40, 128, 512), "dgemm4_glu": (5, 128, 2048)}[entry]
    x, q, s, (y, m) = _quantized_case(fmt, M, N, K)
    fn = {"gemv8": lambda: ops.gemv8_glu(x, q, s), "gemv4": lambda: ops.gemv4_glu(x, q, s),
          "dgemm8_glu": lambda: ops.dgemm8_glu(x, q, s), "dgemm8w_glu": lambda: ops.dgemm8w_glu(x, q, s),
          "dgemm4_glu": lambda: ops.dgemm4_glu(x, q, s)}[entry]
    _rule(fn, y, m, entry)
