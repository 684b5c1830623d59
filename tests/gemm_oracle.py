"""Exact-arithmetic oracle for the bf16-weight GEMM family (gemm.hip, pgemm.hip, mgemm.hip and
the ring kernel / batch-1 GEMV of dgemm.hip).

A bound on fp32 accumulation over K terms has to allow ~K * 2^-24 * sum|x||w|: several bf16
ulps at K = 4096, which hides a dropped k-step, a tile from the wrong K slice or a truncating
pack.  So the inputs are chosen to make the product exact instead:

* X and W hold odd integers (exact in bf16) times one power of two per row.  The row scales
  differ from row to row, so a row mix-up shows; they move only the exponent.
* every bf16 x bf16 product is exact in fp32;
* the **certificate**: if ``m = sum_k |x||w|`` over one accumulation (K / S terms), taken on
  the integers before the row scales, is below 2^24, every partial sum in any order is an
  integer below 2^24 and is exact in fp32.  :func:`certificate` asserts that per element.

The kernel's result is then fixed to the bit whatever its tiling, ring depth, wave split or
MFMA internals: an fp32 slab element equals the fp64 slab sum, a bf16 output equals
RNE_bf16(fp64 sum), a bf16 slab equals RNE_bf16 of its fp32 slab, and the LM-head epilogues
return the lowest index of the maximum of RNE_bf16(fp64 logits[:n_valid]) and that value.
:func:`assert_bits` compares bit images; the tolerance is zero.

The value ranges follow from the certificate: up to 1024 terms both operands use |v| <= 127;
longer sums narrow one operand (``wide`` names the one that keeps |v| <= 127) to the largest
2^b - 1 with 127 * (2^b - 1) * terms < 2^24 (7 at the GEMV's 14336 terms).

Epilogues that are not exact take an exact input: the gate|up values of a fused SwiGLU are known
to the bit, so :func:`glu` feeds them to ``rowop_oracle.silu_mul`` and the result is checked
with ``rowop_oracle.assert_oracle`` under that file's bf16 rule.  :func:`gemm_epi` does the same
for gemm.hip's bias / GELU / residual epilogues with the magnitude of ``rowop_oracle.bias_act``
(|product| + |bias| (+ |residual|)).  That rule was derived for ``bias_act``, whose input is a
bf16 tensor; gemm.hip adds the bias to the fp32 accumulator instead, which here holds the exact
product.  The epilogue then performs the same fp32 operations on an input that carries no
rounding of its own (bias_act's bf16 input is exact too), so the count of fp32 roundings --
one per add, a handful in the GELU -- is the same and the derivation carries over unchanged;
with ordinary data the fp32 accumulator is closer to the true product than its bf16 image, so
the fused path errs less, not more.

The secondary input class (:func:`randn_xw`: N(0,1) x, N(0,1)/sqrt(K) w, the same row scales)
has full random significands and cannot be exact.  Its rule is one rounding per added term,
the worst case of any summation order: fp32 slabs ``|got - y| <= (K/S) * 2^-24 * m`` and bf16
outputs ``0.5 ulp_bf16(y) + K * 2^-24 * m`` with ``m = sum|x||w|`` on the scaled tensors.  It
only exists to catch an operand whose low significand bits are lost on a path the integer
fill cannot reach.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import torch

from tests import rowop_oracle as RO

LIMIT = float(2 ** 24)
BF16 = torch.bfloat16
TIE_EVEN = (257.0, 261.0)      # 9-bit integers: a tie whose lower bf16 neighbour is even (256, 260)
TIE_ODD = (259.0, 263.0)       # ... whose lower neighbour is odd (258, 262): RNE goes up
TIE_COLS = 3                   # X columns 0..2 are the constant 1 that the tie rows multiply
DOMINANT = 2.0 ** 22           # row scale of the planted argmax rows: beats any certified logit


# ----------------------------------------------------------------------------- rounding
def exact_f32(v64):
    f = v64.float()
    assert torch.equal(f.double(), v64), "value is not an fp32 number"
    return f


def rne_bf16(v64):
    """RNE_bf16 of fp64 values that are fp32 numbers (so that no double rounding occurs)."""
    return exact_f32(v64).bfloat16().double()


def trunc_bf16(v64):
    """The bf16 pack done by truncation (a planted fault)."""
    i = exact_f32(v64).contiguous().view(torch.int32)
    return (i & -65536).view(torch.float32).double()


def half_away_bf16(v64):
    """The bf16 pack rounding ties away from zero (a planted fault)."""
    i = exact_f32(v64).contiguous().view(torch.int32)
    return ((i + 0x8000) & -65536).view(torch.float32).double()


def rounding_classes(v64):
    """(ties with an even lower neighbour, ties with an odd one, plain inexact) counts of the
    bf16 pack of ``v64``."""
    i = exact_f32(v64).contiguous().view(torch.int32)
    low, odd = i & 0xFFFF, (i >> 16) & 1
    tie = low == 0x8000
    return int((tie & (odd == 0)).sum()), int((tie & (odd == 1)).sum()), int(((low != 0) & ~tie).sum())


# ----------------------------------------------------------------------------- the check
def assert_bits(got, want, *, what="", ksize=None):
    """``got`` (bf16 / fp32, [.., M, N] or [S, M, N]) must hold exactly the fp64 values ``want``:
    bit images are compared, so -0 and NaN are seen.  ``ksize``: K terms per slice, for the
    report."""
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype in (BF16, torch.float32), f"{what}: dtype {got.dtype}"
    w = want.to(got.dtype)
    assert torch.equal(w.double(), want), f"{what}: the oracle value is not a {got.dtype} number"
    bad = RO.bits(got) != RO.bits(w)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    err = torch.nan_to_num((got.double() - want).abs(), nan=float("inf"), posinf=float("inf"))
    err = torch.where(bad, err, torch.full_like(err, -1.0))
    i = int(err.reshape(-1).argmax())
    N = want.shape[-1] if want.dim() else 1
    M = want.shape[-2] if want.dim() >= 2 else 1
    r, c = divmod(i % (M * N), N)
    s = i // (M * N)
    where = f"(row {r}, col {c}), 16 x 16 tile ({r // 16}, {c // 16})"
    if want.dim() == 3:
        where += f", k-slice {s}" + (f" = k [{s * ksize}, {(s + 1) * ksize})" if ksize else "")
    raise AssertionError(
        f"{what}: {nbad} of {want.numel()} elements differ in their bits; worst at {where}: "
        f"got {float(got.reshape(-1)[i])!r} (0x{int(RO.bits(got).reshape(-1)[i]) & 0xFFFFFFFF:x}), "
        f"want {float(want.reshape(-1)[i])!r} (0x{int(RO.bits(w).reshape(-1)[i]) & 0xFFFFFFFF:x})")


def old_rule_accepts(got, want):
    """The rule the GEMM tests used before: one number for the whole tensor."""
    return bool((got.double() - want).abs().max() <= 2e-2 + 1e-2 * want.abs().max())


# ----------------------------------------------------------------------------- inputs
@dataclass(frozen=True, eq=False)
class Fill:
    """Integer operands and their power-of-two row scales; ``x`` / ``w`` are the bf16 tensors
    the kernel sees.  ``S``: the K slices each output element is summed over separately."""
    xi: torch.Tensor     # [M, K] fp64 integers
    wi: torch.Tensor     # [N, K] fp64 integers
    xs: torch.Tensor     # [M] fp64 powers of two
    ws: torch.Tensor     # [N] fp64 powers of two
    S: int
    x: torch.Tensor      # [M, K] bf16 = xi * xs
    w: torch.Tensor      # [N, K] bf16 = wi * ws

    def to(self, device):
        return replace(self, **{k: getattr(self, k).to(device) for k in ("xi", "wi", "xs", "ws", "x", "w")})


def _bf16_exact(v64):
    b = v64.to(BF16)
    assert torch.equal(b.double(), v64), "an operand is not exact in bf16"
    assert torch.equal(b.double().to(BF16).view(torch.int16), b.view(torch.int16)), "bf16 -> fp64 -> bf16"
    return b


def finish(xi, wi, xs, ws, S):
    """Build the bf16 tensors of a fill and assert everything the method rests on."""
    f = Fill(xi, wi, xs, ws, S, _bf16_exact(xi * xs[:, None]), _bf16_exact(wi * ws[:, None]))
    certificate(f)
    return f


def magnitude(f: Fill):
    """m [S, M, N] = sum_k |x||w| per K slice, on the integers (before the row scales)."""
    M, K = f.xi.shape
    a = f.xi.abs().reshape(M, f.S, K // f.S)
    b = f.wi.abs().reshape(-1, f.S, K // f.S)
    return torch.einsum("msk,nsk->smn", a, b)


def certificate(f: Fill):
    """Assert that every accumulation of the fill is exact in fp32 in any order; returns m."""
    for t in (f.xi, f.wi):
        assert torch.equal(t, t.round()), "operands must be integers before the row scales"
    for s in (f.xs, f.ws):
        assert torch.equal(torch.exp2(torch.log2(s).round()), s), "row scales must be powers of two"
    assert torch.equal((f.xi * f.xs[:, None]).to(BF16), f.x) and torch.equal((f.wi * f.ws[:, None]).to(BF16), f.w)
    assert f.xi.shape[1] % f.S == 0
    m = magnitude(f)
    worst = float(m.max())
    assert worst < LIMIT, f"certificate: sum|x||w| = {worst} >= 2^24"
    return m


def narrow_range(terms):
    """Largest 2^b - 1 <= 127 with 127 * (2^b - 1) * terms < 2^24."""
    a = 127
    while 127 * a * terms >= 2 ** 24:
        a //= 2
    assert a >= 1
    return a


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _odd(shape, amax, g):
    """Odd integers uniform in +-{1, 3, .., amax} (amax odd)."""
    mag = 2 * torch.randint(0, (amax + 1) // 2, shape, generator=g) + 1
    sign = 2 * torch.randint(0, 2, shape, generator=g) - 1
    return (mag * sign).double()


def x_scales(M):
    return torch.exp2(((torch.arange(M) % 5) - 2).double())


def w_scales(N, shift=0):
    return torch.exp2(((torch.arange(N) % 7) - 3 + shift).double())


def _unique_rows(t):
    return torch.unique(t, dim=0).shape[0] == t.shape[0]


@functools.lru_cache(maxsize=16)
def _exact_x(M, K, amax, ties, seed):
    xi = _odd((M, K), amax, _gen(seed))
    if ties:
        xi[:, :TIE_COLS] = 1.0
    assert _unique_rows(xi * x_scales(M)[:, None]), "X rows must be pairwise different"
    return xi


@functools.lru_cache(maxsize=16)
def _exact_w(N, K, amax, ties, seed):
    wi = _odd((N, K), amax, _gen(seed))
    if ties:      # the last four rows: 127 + 127 + t on the constant X columns, zero elsewhere
        for j, t in enumerate(TIE_EVEN + TIE_ODD):
            wi[N - 4 + j] = 0.0
            wi[N - 4 + j, :TIE_COLS] = torch.tensor([127.0, 127.0, t - 254.0], dtype=torch.float64)
    assert _unique_rows(wi * w_scales(N)[:, None]), "W rows must be pairwise different"
    return wi


def exact_xw(M, N, K, S=1, seed=0, wide="x", *, wshift=0, device="cpu") -> Fill:
    """The exact fill: odd integers, |v| <= 127 on the ``wide`` operand and on both where the
    K / S terms of one sum allow it, times row scales 2^((m % 5) - 2) / 2^((n % 7) - 3 + wshift).
    Where the weights keep |w| <= 127 the last four weight rows are tie rows: with X columns
    0..2 set to 1 they make every X row's last four outputs 257, 261 (bf16 ties with an even
    lower neighbour) and 259, 263 (odd) times the row scales.  Asserts the certificate, the
    bf16 round trip and that rows are pairwise different."""
    assert wide in ("x", "w") and K % S == 0
    nar = narrow_range(K // S)
    ax, aw = (127, nar) if wide == "x" else (nar, 127)
    ties = aw == 127 and N >= 16
    xi = _exact_x(M, K, ax, ties, 1000 + 7 * seed + M).to(device, copy=True)
    wi = _exact_w(N, K, aw, ties, 2000 + 7 * seed + N).to(device, copy=True)
    return finish(xi, wi, x_scales(M).to(device), w_scales(N, wshift).to(device), S)


def fills(K, S=1):
    """The fills a case runs: both operands have a full significand at <= 1024 terms; longer
    sums run a second fill with the widths swapped."""
    return ("x",) if narrow_range(K // S) == 127 else ("x", "w")


def randn_xw(M, N, K, seed=0, device="cpu"):
    """The secondary class: N(0,1) x, N(0,1)/sqrt(K) w, the exact fill's row scales."""
    g = _gen(3000 + seed)
    x = torch.randn(M, K, generator=g) * x_scales(M).float()[:, None]
    w = torch.randn(N, K, generator=g) / K ** 0.5 * w_scales(N).float()[:, None]
    return x.to(BF16).to(device), w.to(BF16).to(device)


def randn_bound(x, w, S):
    """(y [S, M, N], m [S, M, N]) of the secondary class; the slack per added term is 2^-24:
    ``assert_oracle(P, y, m, slack=(K / S) * 2^-24)`` for fp32 slabs and
    ``assert_oracle(Y, y.sum(0), m.sum(0), slack=K * 2^-24)`` for bf16 outputs."""
    return slabs(x, w, S), slabs(x.double().abs(), w.double().abs(), S)


# ----------------------------------------------------------------------------- plants
def plant_argmax(f: Fill, n_valid: int, tile: int, swap: bool = False) -> Fill:
    """LM-head plants on top of a fill.  X column 3 decides each row's winner: rows with
    x[m, 3] > 0 (< 0 with ``swap``) take the P rows, identical weight rows at three ids
    ``lo < mid < hi`` below n_valid -- ``mid`` in the next column tile where n_valid reaches
    it -- so the lowest must win; the other X rows take the single Q row at n_valid - 1.  A row
    with twice the logit sits at n_valid, its mirror at n_valid + 1, and four times the logit
    in the last tile: all must be ignored.  Returns the new fill."""
    N, K = f.wi.shape
    assert 6 <= n_valid <= N
    sgn = -1.0 if swap else 1.0
    lo, mid, hi, q = 2, min(tile + 7, n_valid - 3), n_valid - 2, n_valid - 1
    assert lo < mid < hi
    wi, ws = f.wi.clone(), f.ws.clone()

    def put(row, coef, scale):
        wi[row] = 0.0
        wi[row, 3] = coef
        ws[row] = scale

    for row in (lo, mid, hi):
        put(row, sgn * 127.0, DOMINANT)
    put(q, -sgn * 127.0, DOMINANT)
    past = [(n_valid, sgn, 2.0), (n_valid + 1, -sgn, 2.0), (N - 1, sgn, 4.0), (N - 2, -sgn, 4.0)]
    for row, s, k in past:
        if n_valid <= row < N:
            put(row, s * 127.0, DOMINANT * k)
    return finish(f.xi, wi, f.xs, ws, f.S)


GLU_GATES = (-90.0, -88.0, -80.0, 90.0)
GLU_UPS = (2.0 ** 8, 2.0 ** -8)


def plant_glu(f: Fill, k0: int = 5) -> Fill:
    """SwiGLU overflow plants: the last X row becomes one-hot (1 at column ``k0``, scale 1) and
    the first 8-interleaved group of W (gate rows 0..7, up rows 8..15) is zero except at
    ``k0``, where the gates hold -90, -88, -80, +90 (twice) and the ups 2^8 (four) and 2^-8
    (four).  The one-hot row's first eight gate|up pairs are then exactly those values: the
    exp overflow branch of silu and its neighbourhood, with every gate against both ups."""
    xi, xs, wi, ws = f.xi.clone(), f.xs.clone(), f.wi.clone(), f.ws.clone()
    xi[-1] = 0.0
    xi[-1, k0] = 1.0
    xs[-1] = 1.0
    wi[:16] = 0.0
    for j in range(8):
        wi[j, k0], ws[j] = GLU_GATES[j % 4], 1.0
        wi[8 + j, k0], ws[8 + j] = 1.0, GLU_UPS[j // 4]
    return finish(xi, wi, xs, ws, f.S)


# ----------------------------------------------------------------------------- oracles
def slabs(x, w, S):
    """fp64 [S, M, N]: x @ w^T per K slice."""
    M, K = x.shape
    a = x.double().reshape(M, S, K // S)
    b = w.double().reshape(-1, S, K // S)
    return torch.einsum("msk,nsk->smn", a, b)


def product_bf16(x, w):
    """fp64 [M, N] = RNE_bf16(x @ w^T)."""
    return rne_bf16(slabs(x, w, 1)[0])


def slab16(x, w, S):
    """fp64 [S, M, N]: every fp32 slab rounded to bf16."""
    return rne_bf16(slabs(x, w, S))


def glu(x, w):
    """(y, m) of silu(gate) * up over the 8-interleaved gate|up rows of w, both inputs rounded
    to bf16 first, as every kernel here does."""
    return RO.silu_mul(product_bf16(x, w).to(BF16), interleaved=True)


def gemm_epi(x, w, bias, residual, epi):
    """(y, m) of gemm.hip's epilogues on the exact product: 0 none, 1 bias, 2 bias + GELU(erf),
    3 bias + residual, 4 SwiGLU.  m as in ``rowop_oracle.bias_act``: |product| + |bias|
    (+ |residual|); epi 0 is exact (use :func:`product_bf16` and :func:`assert_bits`)."""
    if epi == 4:
        return glu(x, w)
    p = slabs(x, w, 1)[0]
    if epi == 0:
        return p, p.abs()
    v, m = p + bias.double(), p.abs() + bias.double().abs()
    if epi == 3:
        v, m = v + residual.double(), m + residual.double().abs()
    if epi == 2:
        v = 0.5 * v * (1.0 + torch.special.erf(v * 0.7071067811865476))
    return v, m


def lowest_argmax(v):
    """(ids int64, values) of the row maxima, ties to the lowest index."""
    top = v.max(-1, keepdim=True).values
    idx = torch.arange(v.shape[-1], device=v.device).expand_as(v)
    ids = torch.where(v == top, idx, torch.full_like(idx, v.shape[-1])).min(-1).values
    return ids, top[..., 0]


def argmax(x, w, n_valid):
    """(ids, values): the lowest index of the maximum of RNE_bf16(fp64 logits[:, :n_valid])."""
    return lowest_argmax(product_bf16(x, w)[:, :n_valid])


def argmax_tiles(x, w, n_valid, tile):
    """Per row: in how many different column tiles the maximum occurs (the planted ties)."""
    v = product_bf16(x, w)[:, :n_valid]
    hit = v == v.max(-1, keepdim=True).values
    pad = (-n_valid) % tile
    hit = torch.nn.functional.pad(hit, (0, pad)).reshape(v.shape[0], -1, tile)
    return hit.any(-1).sum(-1)
