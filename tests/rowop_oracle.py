"""fp64 oracles and the one tolerance rule for the row-wise and element-wise kernels
(norm.hip, act.hip, rope_cache.hip, pool.hip and the embedding kernels of embed_sample.hip).

Every oracle is plain torch float64 on whatever device its inputs live on.  Inputs are the
bf16 (or fp32) tensors the kernel sees, upcast exactly.  Each returns ``(y, m)``: ``y`` the
fp64 result and ``m`` the per-element magnitude -- the same formula with every additive term
replaced by its absolute value, so ``m`` bounds what fp32 rounding of the terms can move.

The assertion (:func:`assert_oracle`) is per element, no max-norm over the tensor:

* bf16 outputs: ``|got - y| <= 0.5 * ulp_bf16(y) + 2^-16 * m`` with
  ``ulp_bf16(v) = 2^(floor(log2(max(|v|, 2^-126))) - 7)``.  Round-to-nearest-even on the final
  pack costs at most half an ulp; the fp32 evaluation costs at most ~136 sequential and tree
  roundings on the reductions (<= 128 per lane at H = 8192 plus 8 shuffle / LDS steps), halved
  by the square root and followed by a few multiplies: under 2^-17 relative.  2^-16 is a
  factor two on top.
* fp32 outputs (pool_l2): ``|got - y| <= 2^-14 * m``: a sequential fp32 sum of L <= 512 rows
  (<= 2^-15 relative, worst case) followed by the norm.

The numbers are derived, not measured.  The input builders at the bottom are shared by the
CPU soundness tests and the GPU tests, so both see the same tensors.
"""
from __future__ import annotations

import torch

SLACK_BF16 = 2.0 ** -16
SLACK_F32 = 2.0 ** -14


# ----------------------------------------------------------------------------- the rule
def _ulp(v, mant_bits: int):
    """2^(floor(log2(max(|v|, 2^-126))) - mant_bits), exactly (frexp, no log)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))      # |v| = f * 2^e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 1 - mant_bits)


def ulp_bf16(v):
    return _ulp(v, 7)


def tolerance(got_dtype, y, m, slack=None, extra=None):
    if got_dtype == torch.bfloat16:
        tol = 0.5 * ulp_bf16(y) + (SLACK_BF16 if slack is None else slack) * m
    elif got_dtype == torch.float32:
        tol = (SLACK_F32 if slack is None else slack) * m
    else:
        raise TypeError(f"no tolerance rule for {got_dtype}")
    return tol if extra is None else tol + extra


def assert_oracle(got, y, m, *, slack=None, extra=None, what=""):
    """Per-element check of a kernel output against ``(y, m)``.  ``extra``: an additional
    per-element absolute allowance (split-K consumers).  A NaN or inf in ``got`` fails."""
    assert got.shape == y.shape, f"{what}: shape {tuple(got.shape)} != {tuple(y.shape)}"
    g = got.double()
    tol = tolerance(got.dtype, y, m, slack, extra)
    err = (g - y).abs()
    bad = ~(err <= tol)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    cols = y.shape[-1] if y.dim() else 1
    unit = _ulp(y, 7 if got.dtype == torch.bfloat16 else 23)
    over = torch.where(bad, torch.nan_to_num(err / unit, nan=float("inf")), torch.full_like(err, -1.0))
    i = int(over.reshape(-1).argmax())
    r, c = divmod(i, cols)
    gf, yf, ef, uf, tf = (float(t.reshape(-1)[i]) for t in (g, y, err, unit, tol))
    raise AssertionError(
        f"{what}: {nbad} of {y.numel()} elements outside the bound; worst at (row {r}, col {c}): "
        f"got {gf!r}, want {yf!r}, err {ef:.3e} = {ef / uf:.3f} ulp (allowed {tf / uf:.3f} ulp)")


def bits(t):
    """Bit image of a bf16 / fp32 tensor, for exact comparisons that also see -0 and NaN."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ----------------------------------------------------------------------------- oracles
def rmsnorm(x, w, eps):
    xd = x.double()
    inv = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)
    y = xd * inv * w.double()
    return y, y.abs()


def add_rmsnorm(x, residual, w, eps):
    """(s, ms), (y, m): the fp64 residual sum x + r, and rmsnorm of that sum.  The GPU tests
    check the kernel's residual against ``s`` and then its output against
    ``rmsnorm(kernel residual)``, so a half-ulp tie in the residual does not compound."""
    s = x.double() + residual.double()
    return (s, x.double().abs() + residual.double().abs()), rmsnorm(s, w, eps)


def _ln(xs, gamma, beta, eps):
    mean = xs.mean(-1, keepdim=True)
    d = xs - mean
    inv = torch.rsqrt(d.pow(2).mean(-1, keepdim=True) + eps)
    g, b = gamma.double(), beta.double()
    y = d * inv * g + b
    m = (d.abs() + xs.abs().mean(-1, keepdim=True)) * inv * g.abs() + b.abs()
    return y, m


def layernorm(x, residual, gamma, beta, eps):
    xs = x.double()
    if residual is not None:
        xs = xs + residual.double()
    return _ln(xs, gamma, beta, eps)


def _clamp_ids(ids, n):
    ids = ids.long()
    return torch.where((ids >= 0) & (ids < n), ids, torch.zeros_like(ids))


def embedding(ids, table):
    """Out-of-range ids read row 0."""
    return table[_clamp_ids(ids, table.shape[0])]


def bert_embed_ln(ids, pos, token_type, wte, wpe, wtt, gamma, beta, eps):
    """Out-of-range token / position / type indices read row 0 of their table."""
    tt = token_type if token_type is not None else torch.zeros_like(ids)
    xs = (wte[_clamp_ids(ids, wte.shape[0])].double() + wpe[_clamp_ids(pos, wpe.shape[0])].double()
          + wtt[_clamp_ids(tt, wtt.shape[0])].double())
    return _ln(xs, gamma, beta, eps)


def silu_mul(gu, interleaved=False):
    v = gu.double()
    if interleaved:
        v = v.unflatten(-1, (-1, 2, 8))
        g, u = v[..., 0, :].flatten(-2), v[..., 1, :].flatten(-2)
    else:
        g, u = v.chunk(2, dim=-1)
    y = g / (1.0 + torch.exp(-g)) * u          # exp(-g) = inf for g < -709 only: g / inf = -0
    return y, y.abs()


def bias_act(x, bias, residual, gelu):
    v = x.double() + bias.double()
    m = x.double().abs() + bias.double().abs()
    if residual is not None:
        v = v + residual.double()
        m = m + residual.double().abs()
    if gelu:
        v = 0.5 * v * (1.0 + torch.special.erf(v * 0.7071067811865476))
    return v, m


def rope(qkv, positions, cos_sin, Hq, Hkv, D):
    """Rotate-half RoPE of the Q and K heads of packed rows [T, (Hq + 2 Hkv) D], taking the
    fp32 [max_pos, D] (cos | sin) table as given.  Returns [T, (Hq + Hkv) D]."""
    T, half = qkv.shape[0], D // 2
    x = qkv.double().reshape(T, Hq + 2 * Hkv, D)[:, : Hq + Hkv]
    cs = cos_sin.double()[positions.long()]
    c, s = cs[:, None, :half], cs[:, None, half:]
    x1, x2 = x[..., :half], x[..., half:]
    y = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    m = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return y.reshape(T, -1), m.reshape(T, -1)


def pool_l2(h, cu_seqlens, mean, normalize):
    cu = cu_seqlens.tolist()
    B, H = len(cu) - 1, h.shape[-1]
    y = torch.zeros(B, H, dtype=torch.float64, device=h.device)
    m = torch.zeros_like(y)
    for b in range(B):
        s0, s1 = cu[b], cu[b + 1]
        if s1 > s0:
            seg = h[s0:s1].double() if mean else h[s0:s0 + 1].double()
            y[b] = seg.mean(0)
            m[b] = seg.abs().mean(0)
    if normalize:
        inv = 1.0 / y.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
        y, m = y * inv, m * inv
    return y, m


# ----------------------------------------------------------------------------- rope + cache
SENTINEL_BITS = 0x4D2B      # a finite bf16 (~1.8e8) no rotation of the inputs below produces


def sentinel_cache(nb, Hkv, BS, D, device):
    c = torch.full((nb, Hkv, BS, D), SENTINEL_BITS, dtype=torch.int16, device=device)
    return c.view(torch.bfloat16)


def check_rope_cache(before, after, positions, slots, cos_sin, k_cache, v_cache, Hq, Hkv, D):
    """Everything a bf16-cache rope_cache call must leave behind.  ``before`` / ``after``: the
    packed rows [T, W]; ``slots`` None: the caches (if given) must be untouched."""
    T = before.shape[0]
    qk = (Hq + Hkv) * D
    y, m = rope(before, positions, cos_sin, Hq, Hkv, D)
    assert_oracle(after[:, :qk], y, m, what="rope q/k")
    assert torch.equal(bits(after[:, qk:]), bits(before[:, qk:])), "V columns of qkv changed"
    p0 = positions.long() == 0
    assert torch.equal(bits(after[p0]), bits(before[p0])), "position 0 must leave q and k bit-unchanged"
    if k_cache is None:
        return
    BS = k_cache.shape[2]
    kw = torch.ones(k_cache.shape[:3], dtype=torch.bool, device=k_cache.device)    # still sentinel?
    if slots is not None:
        sm = slots.long()
        valid = sm >= 0
        blk, off = sm[valid] // BS, sm[valid] % BS
        kv = after[valid][:, Hq * D:].reshape(-1, 2 * Hkv, D)
        assert torch.equal(bits(k_cache[blk, :, off]), bits(kv[:, :Hkv])), "K cache != rotated K left in qkv"
        assert torch.equal(bits(v_cache[blk, :, off]), bits(kv[:, Hkv:])), "V cache != V"
        kw[blk, :, off] = False
    for name, c in (("K", k_cache), ("V", v_cache)):
        untouched = bits(c)[kw]
        assert bool((untouched == SENTINEL_BITS).all()), f"{name} cache written outside the mapped slots"
    assert T == positions.numel()


# ----------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def zero_row(rows):
    """Index of the all-zero row of :func:`make_rows` (None for a single row)."""
    return 1 if rows >= 2 else None


def make_rows(rows, H, seed, device="cpu"):
    """bf16 [rows, H]: randn with row i scaled by 2^((i % 21) - 10), so another row's statistics
    are visible, and one all-zero row."""
    x = torch.randn(rows, H, generator=_gen(seed))
    x *= torch.exp2(((torch.arange(rows) % 21) - 10).float())[:, None]
    z = zero_row(rows)
    if z is not None:
        x[z] = 0.0
    return x.bfloat16().to(device)


def make_weight(H, seed, device="cpu"):
    """bf16 [H]: sign alternating per 8-chunk, magnitude 2^U(-2, 2) in [0.25, 4]: neighbouring
    chunks differ, so a chunk applied to the wrong columns shows."""
    mag = torch.exp2(torch.rand(H, generator=_gen(seed)) * 4.0 - 2.0)
    sign = 1.0 - 2.0 * ((torch.arange(H) // 8) % 2).float()
    return (mag * sign).bfloat16().to(device)


def make_offset_rows(rows, H, seed, device="cpu"):
    """bf16 [rows, H] of x = 1024 + 4 k, k a small integer: mean^2 is ~1e5 times the variance,
    which a one-pass E[x^2] - mean^2 in fp32 cannot resolve.  Even rows draw k from {-2..2};
    odd rows are 1024 with one element in eight at 1020.  (bf16 steps by 4 below 1024 but by 8
    above it, so k = 1 rounds to 1024: the values are {1016, 1020, 1024, 1032}, all exact.)"""
    g = _gen(seed)
    k = torch.randint(-2, 3, (rows, H), generator=g).float()
    sparse = -(torch.rand(rows, H, generator=g) < 0.125).float()
    odd = (torch.arange(rows) % 2 == 1)[:, None]
    return (1024.0 + 4.0 * torch.where(odd, sparse, k)).bfloat16().to(device)


GATE_SPECIALS = (-100.0, -96.0, -92.0, -90.0, -89.0, -88.5, -88.0, -87.0, 0.0, -0.0, 1e4, 100.0, -20.0, 20.0,
                 -1e-3, 88.0)
UP_SPECIALS = (1.0, -1.0, 0.0, 3.0, -0.5, 2.0, 0.0, -7.0)


def make_gate_up(T, I, seed, interleaved=False, device="cpu"):
    """bf16 [T, 2 I] gate|up (or 8-interleaved).  Gates: a third uniform in [-100, 100], the rest
    3 randn, and the first gates of the tensor set to GATE_SPECIALS: below -88.7 (where
    exp(-x) overflows in fp32), +-0, 1e4.  Ups: 2 randn with zeros and negatives."""
    g = _gen(seed)
    gate = 3.0 * torch.randn(T, I, generator=g)
    wide = torch.rand(T, I, generator=g) < 1.0 / 3.0
    gate = torch.where(wide, torch.rand(T, I, generator=g) * 200.0 - 100.0, gate)
    up = 2.0 * torch.randn(T, I, generator=g)
    up[torch.rand(T, I, generator=g) < 0.05] = 0.0
    n = min(len(GATE_SPECIALS), T * I)
    gate.view(-1)[:n] = torch.tensor(GATE_SPECIALS[:n])
    up.view(-1)[:n] = torch.tensor((UP_SPECIALS * 2)[:n])
    if interleaved:
        gu = torch.stack([gate.view(T, I // 8, 8), up.view(T, I // 8, 8)], 2).reshape(T, 2 * I)
    else:
        gu = torch.cat([gate, up], -1)
    return gu.bfloat16().to(device)


def make_bias_act(T, N, seed, device="cpu"):
    """x uniform in [-10, 10] (the gelu arguments), bias chunk-alternating, residual randn."""
    g = _gen(seed)
    x = (torch.rand(T, N, generator=g) * 20.0 - 10.0).bfloat16()
    r = torch.randn(T, N, generator=g).bfloat16()
    return x.to(device), make_weight(N, seed + 1, device), r.to(device)


def make_bert(T, H, seed, token_type, device="cpu", V=300, NP=64, NT=2):
    """ids include 0 and V - 1, pos includes NP - 1."""
    g = _gen(seed)
    wte = (0.5 * torch.randn(V, H, generator=g)).bfloat16()
    wpe = (0.5 * torch.randn(NP, H, generator=g)).bfloat16()
    wtt = (0.5 * torch.randn(NT, H, generator=g)).bfloat16()
    ids = torch.randint(0, V, (T,), generator=g).int()
    pos = torch.randint(0, NP, (T,), generator=g).int()
    ids[0], pos[0] = V - 1, NP - 1
    if T > 1:
        ids[1] = 0
    tt = torch.randint(0, NT, (T,), generator=g).int() if token_type else None
    gamma, beta = make_weight(H, seed + 1), make_weight(H, seed + 2)
    out = dict(ids=ids, pos=pos, token_type=tt, wte=wte, wpe=wpe, wtt=wtt, gamma=gamma, beta=beta)
    return {k: (v.to(device) if v is not None else None) for k, v in out.items()}


ROPE_MAX_POS = 1024


def make_rope(Hq, Hkv, D, T, BS, seed, device="cpu"):
    """Packed qkv rows, positions including 0 and max_pos - 1, and a slot mapping that is a random
    permutation including slot 0, the last slot of the last block and (T >= 4) two -1 entries.
    With T == 1 the single token sits at position 0 / the last slot (BS 16) or at
    max_pos - 1 / slot 0 (BS 32)."""
    from docqa_amd.ops import reference as R

    g = _gen(seed)
    W = (Hq + 2 * Hkv) * D
    qkv = torch.randn(T, W, generator=g) * torch.exp2(((torch.arange(T) % 5) - 2).float())[:, None]
    nb = (T + BS - 1) // BS + 2
    pos = torch.randint(1, ROPE_MAX_POS - 1, (T,), generator=g).int()
    slots = torch.randperm(nb * BS - 2, generator=g)[:T].int() + 1      # interior slots, unique
    if T == 1:
        pos[0] = 0 if BS == 16 else ROPE_MAX_POS - 1
        slots[0] = nb * BS - 1 if BS == 16 else 0
    else:
        pos[0], pos[T - 1] = 0, ROPE_MAX_POS - 1
        slots[0], slots[T - 1] = nb * BS - 1, 0
    if T >= 4:
        slots[2] = -1
        slots[T - 2] = -1
    cs = R.rope_cos_sin(ROPE_MAX_POS, D, 500000.0)
    return dict(qkv=qkv.bfloat16().to(device), pos=pos.to(device), slots=slots.to(device), cos_sin=cs.to(device),
                nb=nb)


POOL_LENS = (1, 2, 63, 64, 0, 512, 33)


def make_pool(H, seed, device="cpu"):
    T = sum(POOL_LENS)
    h = torch.randn(T, H, generator=_gen(seed)) * torch.exp2(((torch.arange(T) % 7) - 3).float())[:, None]
    cu = torch.tensor([0] + list(torch.tensor(POOL_LENS).cumsum(0)), dtype=torch.int32)
    return h.bfloat16().to(device), cu.to(device)


# ----------------------------------------------------------------------------- cases
# One builder per op, the seeds a function of the shape alone: the CPU soundness tests and the
# GPU tests call these, so a shape means the same tensors in both.
def rms_case(rows, H, device="cpu"):
    """x, residual, weight"""
    return make_rows(rows, H, 100 + H, device), make_rows(rows, H, 200 + H, device), make_weight(H, 300 + H, device)


def ln_case(rows, H, res, kind, device="cpu"):
    """x, residual (None without ``res``), gamma, beta; kind "scaled" or "offset" (offset rows
    take a zero residual, so that the sum stays on the offset grid)"""
    if kind == "offset":
        x = make_offset_rows(rows, H, 20 + H, device)
        r = torch.zeros_like(x) if res else None
    else:
        x = make_rows(rows, H, 20 + H, device)
        r = make_rows(rows, H, 21 + H, device) if res else None
    return x, r, make_weight(H, 22 + H, device), make_weight(H, 23 + H, device)


def bert_case(T, H, token_type, device="cpu"):
    return make_bert(T, H, 30 + H + T, token_type, device)


def silu_case(T, I, interleaved, device="cpu"):
    return make_gate_up(T, I, 50 + I, interleaved, device)


def bias_case(T, N, device="cpu"):
    return make_bias_act(T, N, 60 + N, device)


def rope_case(Hq, Hkv, D, T, BS, device="cpu"):
    return make_rope(Hq, Hkv, D, T, BS, 70 + D + T + BS, device)


def pool_case(H, device="cpu"):
    return make_pool(H, 80 + H, device)


# shapes small enough for the CPU soundness test; the GPU tests run them too
SMALL_RMS = [(1, 8), (3, 384), (5, 520), (8, 1016), (3, 1024), (3, 2056), (3, 4104), (1, 8192)]
SMALL_LN = [(1, 8), (3, 384), (3, 520), (77, 768), (3, 2048), (3, 4096)]
SMALL_BERT = [(1, 384), (3, 768), (99, 384), (3, 2048)]
SMALL_ACT = [(1, 8), (19, 1536)]
SMALL_ROPE = [(8, 2, 128, 50, 16), (14, 2, 128, 50, 32), (32, 8, 64, 50, 16), (4, 4, 32, 1, 16), (4, 4, 32, 1, 32)]
SMALL_POOL = [8, 384, 768, 1024]
