"""The exact-arithmetic GEMM oracle (tests/gemm_oracle.py) is sound and bites.  CPU only.

Sound: the certificate holds for every fill the GPU file (tests/test_gemm_exact_gpu.py) builds
-- its case tables are imported, so the two cannot drift apart -- and on such data fp32
arithmetic reproduces the fp64 slabs bit for bit in any order: torch's fp32 matmul, and a
blocked fp32 emulation in 32-deep k-steps taken in a shuffled order.  The fixtures hold the
bf16 rounding classes and the argmax ties the checks need, and the CPU fallbacks of ``ops``
agree with the oracle.

Bites: faults planted into the oracle's output or inputs are all rejected.  Each fault test
also records whether the suite's old rule, ``max|a - b| <= 2e-2 + 1e-2 max|b|`` (``agree >
0.97`` for the LM-head picks), accepts the same output; the last test prints the table (run
with ``-s``)."""
import functools

import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as R
from tests import gemm_oracle as G
from tests import rowop_oracle as RO
from tests import test_gemm_exact_gpu as CASES

BF16 = torch.bfloat16
OLD_RULE: dict[str, bool] = {}
OLD_RULE_RANDN: dict[str, bool] = {}      # the old rule on the old tests' data
FAULTS = ("dropped k-step", "duplicated k-step", "wrong slice", "swapped rows", "transposed tile", "truncation",
          "rounding half away", "tail mix", "tie rule", "n_valid + 1", "n_valid - 1", "silu -0")

# per X row of a fixture with tie rows: two ties with an even lower neighbour, two with an odd one
MIN_TIES_PER_ROW = 2


# ----------------------------------------------------------------------------- certificate
def test_certificate_for_every_gpu_fill():
    """exact_xw asserts the certificate, the bf16 round trip and distinct rows itself; here every
    fill of the GPU file is built, and the ranges are the ones the certificate allows."""
    keys = CASES.fill_keys()
    assert len(keys) > 300
    for M, N, K, S, wide, wshift in keys:
        f = G.exact_xw(M, N, K, S, seed=K // 64 + S, wide=wide, wshift=wshift)
        terms = K // S
        nar = G.narrow_range(terms)
        ax, aw = (127, nar) if wide == "x" else (nar, 127)
        assert float(f.xi.abs().max()) <= ax and float(f.wi.abs().max()) <= aw
        assert 127 * nar * terms < 2 ** 24 and (nar == 127 or 127 * (2 * nar + 1) * terms >= 2 ** 24)
        assert f.xs.unique().numel() == min(M, 5) and f.ws.unique().numel() == min(N, 7)
    assert G.narrow_range(1024) == 127 and G.narrow_range(14336) == 7


def test_certificate_refuses_an_inexact_fill():
    f = G.exact_xw(4, 32, 4096, 1, wide="x")
    with pytest.raises(AssertionError, match="certificate"):          # both operands wide over 4096 terms
        G.finish(f.xi, torch.sign(f.wi) * 127.0, f.xs, f.ws, 1)
    with pytest.raises(AssertionError, match="not exact in bf16"):
        G.finish(f.xi * 3.0, f.wi, f.xs, f.ws, 2)


def test_planted_fills_keep_the_certificate():
    for M, N, K, nv in CASES.RING_ARGMAX[:4] + CASES.RING_ARGMAX[-6:]:
        G.plant_argmax(G.exact_xw(M, N, K, 1, seed=K // 64 + 1), nv, 64)
    for K, nv, swap in CASES.GEMV_ARGMAX:
        for wide in G.fills(K):
            G.plant_argmax(G.exact_xw(1, 64, K, 1, seed=K // 64 + 1, wide=wide), nv, 16, swap)
    for c, M, ks, nv in CASES.MG_ARGMAX:
        if M in (1, 257):
            G.plant_argmax(G.exact_xw(M, 2 * CASES.MG_BN[c], ks, 1, seed=ks // 64 + 1), CASES._nv(nv, CASES.MG_BN[c]),
                           CASES.MG_BN[c])
    for M, N, K in [(1, 128, 512), (128, 128, 1024), (1, 64, 4096), (300, 384, 64), (513, 512, 128)]:
        f = G.plant_glu(G.exact_xw(M, N, K, 1, seed=K // 64 + 1))
        gu = G.product_bf16(f.x, f.w)
        assert gu[-1, :16].tolist() == [-90.0, -88.0, -80.0, 90.0] * 2 + [256.0] * 4 + [2.0 ** -8] * 4


# ----------------------------------------------------------------------------- order independence
SMALL = [(17, 128, 512, 1, "x"), (33, 128, 1024, 2, "x"), (129, 128, 2048, 2, "x"), (5, 256, 128, 1, "x"),
         (1, 16, 14336, 1, "x"), (1, 16, 14336, 1, "w"), (1, 64, 4096, 1, "w"), (3, 64, 8192, 2, "x")]


@pytest.mark.parametrize("M,N,K,S,wide", SMALL)
def test_fp32_reproduces_the_slabs_in_any_order(M, N, K, S, wide):
    f = G.exact_xw(M, N, K, S, seed=3, wide=wide)
    want = G.slabs(f.x, f.w, S)
    ks = K // S
    xs = f.x.float().reshape(M, S, ks).permute(1, 0, 2)
    wt = f.w.float().reshape(N, S, ks).permute(1, 2, 0)
    G.assert_bits(xs @ wt, want, what="torch fp32 matmul", ksize=ks)
    # 32-deep k-steps accumulated in fp32, block order shuffled
    order = torch.randperm(ks // 32, generator=torch.Generator().manual_seed(K)).tolist()
    acc = torch.zeros(S, M, N)
    for b in order:
        acc = acc + xs[:, :, 32 * b:32 * b + 32] @ wt[:, 32 * b:32 * b + 32, :]
    G.assert_bits(acc, want, what="blocked fp32, shuffled k-steps", ksize=ks)
    # and element by element inside a k-step, reversed
    acc = torch.zeros(S, M, N)
    for k in reversed(range(min(ks, 64))):
        acc = acc + xs[:, :, k:k + 1] * wt[:, k:k + 1, :]
    G.assert_bits(acc, G.slabs(f.x.reshape(M, S, ks)[:, :, :64].reshape(M, -1),
                               f.w.reshape(N, S, ks)[:, :, :64].reshape(N, -1), S), what="serial fp32")


# ----------------------------------------------------------------------------- what the fixtures hold
def test_rounding_classes_in_every_fixture():
    """Every fill whose weights keep |w| <= 127 (all but the first of the two fills of a long
    sum) has, per X row, at least two exact bf16 ties with an even lower neighbour, two with an
    odd one, and plain inexact values."""
    seen = 0
    for M, N, K, S, wide, wshift in CASES.fill_keys():
        if M > 33 or N > 512 or (wide == "x" and G.narrow_range(K // S) < 127):
            continue
        f = G.exact_xw(M, N, K, S, seed=K // 64 + S, wide=wide, wshift=wshift)
        even, odd, inexact = G.rounding_classes(G.slabs(f.x, f.w, S))
        assert even >= MIN_TIES_PER_ROW * M and odd >= MIN_TIES_PER_ROW * M and inexact >= M, (M, N, K, S, wide)
        seen += 1
    assert seen > 50
    p = G.product_bf16(f.x, f.w)[:, -4:] / (f.xs[:, None] * f.ws[-4:][None])
    assert p[0].tolist() == [256.0, 260.0, 260.0, 264.0]          # 257, 261 down to even; 259, 263 up to even


def test_rounding_helpers():
    v = torch.tensor([257.0, 259.0, 258.5, -257.0, -259.0, 256.0], dtype=torch.float64)
    assert G.rne_bf16(v).tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 256.0]
    assert G.trunc_bf16(v).tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 256.0]
    assert G.half_away_bf16(v).tolist() == [258.0, 260.0, 258.0, -258.0, -260.0, 256.0]
    assert G.rounding_classes(v) == (2, 2, 1)


@pytest.mark.parametrize("M,N,K,n_valid,tile", [(33, 256, 512, 200, 64), (1, 64, 2048, 40, 16), (257, 256, 128, 192, 128),
                                                (17, 512, 512, 384, 256)])
def test_argmax_fixtures_have_real_ties(M, N, K, n_valid, tile):
    for swap in (False, True):
        f = G.plant_argmax(G.exact_xw(M, N, K, 1, seed=5, wide="w"), n_valid, tile, swap)
        ids, vals = G.argmax(f.x, f.w, n_valid)
        tiles = G.argmax_tiles(f.x, f.w, n_valid, tile)
        pos = (f.xi[:, 3] > 0) != swap
        assert torch.equal(ids[pos], torch.full_like(ids[pos], 2)) and bool((tiles[pos] >= 2).all())
        assert torch.equal(ids[~pos], torch.full_like(ids[~pos], n_valid - 1))
        if M > 1:
            assert bool(pos.any()) and bool((~pos).any()) and vals.unique().numel() > 2
        # the rows past n_valid hold larger logits
        assert bool((G.product_bf16(f.x, f.w)[:, n_valid:].max(-1).values > vals).all())


def test_argmax_fixture_inside_the_first_tile():
    f = G.plant_argmax(G.exact_xw(17, 256, 512, 1, seed=5), 40, 64)
    ids, _ = G.argmax(f.x, f.w, 40)
    assert set(ids.tolist()) == {2, 39}


# ----------------------------------------------------------------------------- the check itself
def test_message_names_tile_and_slice():
    f = G.exact_xw(33, 128, 1024, 2, seed=1)
    want = G.slabs(f.x, f.w, 2)
    got = want.float()
    got[1, 20, 37] += 64.0
    with pytest.raises(AssertionError, match=r"1 of 8448 .*row 20, col 37.*tile \(1, 2\), k-slice 1 = k \[512, 1024\)"):
        G.assert_bits(got, want, what="demo", ksize=512)
    got = want.float()
    got[0, 3, 5] = float("nan")
    with pytest.raises(AssertionError, match=r"row 3, col 5.*got nan"):
        G.assert_bits(got, want, what="demo")
    z = torch.zeros(2, 16, dtype=torch.float64)
    with pytest.raises(AssertionError, match="differ in their bits"):
        G.assert_bits(-z.to(BF16), z, what="minus zero")
    with pytest.raises(AssertionError, match="shape"):
        G.assert_bits(want.float()[:, :32], want, what="coverage")


# ----------------------------------------------------------------------------- planted faults
def _reject_bits(name, got, want, **kw):
    with pytest.raises(AssertionError, match="differ in their bits"):
        G.assert_bits(got, want, what=name, **kw)
    OLD_RULE[name] = G.old_rule_accepts(got, want)


TILE = (slice(16, 32), slice(32, 48))


def _f32(v64):
    return v64.float().double()


def _slab_faults(x, w, tail):
    """name -> (got, want) of every slab / pack fault planted into the oracle's own arithmetic on
    x [33, K], w [128, K] (two K slices) and a garbage tail row ``tail`` [1, K]."""
    K = x.shape[1]
    P, out = G.slabs(x, w, 2), {}
    k0 = K // 2 + 96                                   # the fourth 32-deep k-step of slice 1
    step = x[TILE[0], k0:k0 + 32].double() @ w[TILE[1], k0:k0 + 32].double().t()
    for name, sign in (("dropped k-step", -1.0), ("duplicated k-step", 1.0)):
        got = P.clone()
        got[1][TILE] += sign * step
        out[name] = (got.float(), P)
        out[name + " (bf16 slabs)"] = (got.float().to(BF16), G.rne_bf16(_f32(P)))
    got = P.clone()
    got[0][TILE] = P[1][TILE]
    out["wrong slice"] = (got.float(), P)
    ws = w.clone()
    ws[[35, 43]] = ws[[43, 35]]                        # 8 apart inside the 16-row group 32..47
    out["swapped rows"] = (G.slabs(x, ws, 2).float(), P)
    got = P.clone()
    got[0][TILE] = P[0][TILE].t()
    out["transposed tile"] = (got.float(), P)
    p = _f32(G.slabs(x, w, 1)[0])
    out["truncation"] = (G.trunc_bf16(p).to(BF16), G.rne_bf16(p))
    out["rounding half away"] = (G.half_away_bf16(p).to(BF16), G.rne_bf16(p))
    got = P.clone()
    got[:, 32] += G.slabs(tail, w, 2)[:, 0]            # the last valid row takes the tail row's sums
    out["tail mix"] = (got.float(), P)
    return out


def test_slab_and_pack_faults():
    f = G.exact_xw(34, 128, 1024, 2, seed=1)           # 33 valid rows and the tail's garbage row
    faults = _slab_faults(f.x[:33], f.w, f.x[33:])
    for name, (got, want) in faults.items():
        _reject_bits(name, got, want)
    for name in ("dropped k-step", "duplicated k-step"):
        OLD_RULE[name] = OLD_RULE[name] and OLD_RULE.pop(name + " (bf16 slabs)")
    # half-away differs from RNE on the ties with an even lower neighbour only
    p = G.slabs(f.x[:33], f.w, 1)[0]
    assert int((G.half_away_bf16(p) != G.rne_bf16(p)).sum()) == G.rounding_classes(p)[0] >= 2 * 33
    # a poisoned tail row (the GPU tests' NaN rows) shows as well
    got = faults["tail mix"][1].float()
    got[:, 32] = float("nan")
    with pytest.raises(AssertionError, match="got nan"):
        G.assert_bits(got, faults["tail mix"][1], what="NaN tail")
    # the same faults on the data the old tests used: N(0,1) x, N(0,1)/sqrt(K) w at K = 4096
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(34, 4096, generator=g).to(BF16), (torch.randn(128, 4096, generator=g) / 64).to(BF16)
    for name, (got, want) in _slab_faults(x[:33], w, x[33:]).items():
        OLD_RULE_RANDN[name] = G.old_rule_accepts(got, want)
    for name in ("dropped k-step", "duplicated k-step"):
        OLD_RULE_RANDN[name] = OLD_RULE_RANDN[name] and OLD_RULE_RANDN.pop(name + " (bf16 slabs)")


def _ids_rejected(name, ids, want):
    assert not torch.equal(ids, want), name
    OLD_RULE[name] = bool((ids == want).float().mean() > 0.97)


def test_fault_argmax():
    n_valid = 200
    f = G.plant_argmax(G.exact_xw(33, 256, 512, 1, seed=5), n_valid, 64)
    want, vals = G.argmax(f.x, f.w, n_valid)
    v = G.product_bf16(f.x, f.w)
    top = v[:, :n_valid].max(-1, keepdim=True).values
    idx = torch.arange(n_valid).expand(33, -1)
    highest = torch.where(v[:, :n_valid] == top, idx, torch.full_like(idx, -1)).max(-1).values
    _ids_rejected("tie rule", highest, want)
    for name, nv in (("n_valid + 1", n_valid + 1), ("n_valid - 1", n_valid - 1)):
        ids, got_vals = G.lowest_argmax(v[:, :nv])
        _ids_rejected(name, ids, want)
        with pytest.raises(AssertionError, match="differ in their bits"):
            G.assert_bits(got_vals.float(), vals, what=name)


def test_fault_old_silu():
    f = G.plant_glu(G.exact_xw(17, 128, 512, 1, seed=4))
    gu = G.product_bf16(f.x, f.w).to(BF16)
    y, m = G.glu(f.x, f.w)
    v = gu.float().unflatten(-1, (-1, 2, 8))
    g, u = v[..., 0, :].flatten(-2), v[..., 1, :].flatten(-2)
    old = (g / (1.0 + torch.exp(-g)) * u).to(BF16)
    # gate -90 (columns 0 and 4 of the one-hot row): exp(90) overflows, -0 where -1.9e-35 is due
    assert RO.bits(old)[-1, [0, 4]].tolist() == [-32768] * 2 and float(y[-1, 0]) < -1e-36
    with pytest.raises(AssertionError, match="outside the bound"):
        RO.assert_oracle(old, y, m, what="silu -0")
    OLD_RULE["silu -0"] = G.old_rule_accepts(old, y)
    # the formula of act.hip / ops.reference passes, and equals the old one above -80
    new = R.silu_mul(gu, interleaved=True)
    RO.assert_oracle(new, y, m, what="silu_times")
    keep = (g >= -80.0)
    assert torch.equal(RO.bits(new)[keep], RO.bits(old)[keep])


# ----------------------------------------------------------------------------- CPU fallbacks
@pytest.mark.parametrize("M,N,K,S", [(17, 128, 512, 1), (33, 128, 1024, 2), (5, 256, 1024, 4)])
def test_cpu_fallbacks_agree(M, N, K, S):
    f = G.exact_xw(M, N, K, S, seed=6)
    want = G.slabs(f.x, f.w, S)
    G.assert_bits(ops.dgemm_partial(f.x, f.w, S), want, what="dgemm_partial", ksize=K // S)
    G.assert_bits(ops.pgemm_partial(f.x, f.w, S), want, what="pgemm_partial", ksize=K // S)
    G.assert_bits(ops.mgemm_partial(f.x, f.w, S, bf16=True), G.slab16(f.x, f.w, S), what="mgemm_partial bf16")
    if S > 1:
        G.assert_bits(ops.mgemm_partial(f.x, f.w, S), want, what="mgemm_partial", ksize=K // S)
    else:
        G.assert_bits(ops.mgemm_partial(f.x, f.w, 1), G.product_bf16(f.x, f.w), what="mgemm_partial S=1")


@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_cpu_linear_fused_agrees(epi):
    M, N, K = 33, 128, 384
    f = G.exact_xw(M, N, K, 1, seed=7, wshift=CASES.GEMM_WSHIFT if epi else 0)
    bias = RO.make_weight(N, 61 + N) if epi else None
    res = RO.make_rows(M, N, 62 + N) if epi == 3 else None
    got = ops.linear_fused(f.x, f.w, bias, res, epi)
    if epi == 0:
        G.assert_bits(got, G.product_bf16(f.x, f.w), what="linear_fused epi 0")
    else:
        y, m = G.gemm_epi(f.x, f.w, bias, res, epi)
        RO.assert_oracle(got, y, m, what=f"linear_fused epi {epi}")
        assert float(y.abs().median()) < 16.0          # the GELU sees arguments of its own scale


def test_zz_print_fault_table():
    if any(k not in OLD_RULE for k in FAULTS):       # selected alone: plant the faults now
        for fn in (test_slab_and_pack_faults, test_fault_argmax, test_fault_old_silu):
            fn()
    assert all(k in OLD_RULE for k in FAULTS)
    word = {True: "ACCEPTS", False: "rejects", None: "-"}
    print("\nold rule: max|a - b| <= 2e-2 + 1e-2 max|b| (LM-head picks: agree > 0.97)")
    print(f"{'planted fault':<22}{'exact check':<14}{'old rule, exact data':<23}old rule, N(0,1) data at K = 4096")
    for k in FAULTS:
        print(f"{k:<22}{'rejects':<14}{word[OLD_RULE[k]]:<23}{word[OLD_RULE_RANDN.get(k)]}")
    assert any(OLD_RULE.values()) and any(OLD_RULE_RANDN.values())
