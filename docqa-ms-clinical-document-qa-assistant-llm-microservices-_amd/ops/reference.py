"""Plain-PyTorch (fp32-accumulating) reference implementations of every native op.

These serve two purposes:
  * the numerics oracle the GPU tests compare the HIP kernels against;
  * the CPU execution path, so services, models and the distributed code can be
    exercised in CI without a GPU.  On a GPU tensor the dispatcher in
    ``docqa_amd.ops`` never falls back here: it raises if the native extension is
    missing (see ``ops/__init__.py``).
Layouts mirror the kernels exactly (paged cache ``[num_blocks, Hkv, BS, D]``, packed
QKV rows ``[(Hq + 2*Hkv) * D]``, FAISS distance conventions).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def rmsnorm(x, w, eps):
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * w.float()).to(x.dtype)


def add_rmsnorm(x, residual, w, eps):
    s = (x.float() + residual.float()).to(x.dtype)
    residual.copy_(s)
    return rmsnorm(s, w, eps)


def layernorm(x, residual, gamma, beta, eps):
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    return F.layer_norm(xf, (x.shape[-1],), gamma.float(), beta.float(), eps).to(x.dtype)


def rope_inv_freq(head_dim: int, theta: float, scaling: dict | None = None) -> torch.Tensor:
    """fp64 RoPE inverse frequencies, with Hugging Face ``rope_scaling`` applied.

    * ``None`` / ``"default"``: theta^(-2i/d).
    * ``"linear"``: every frequency divided by ``factor`` (position interpolation).
    * ``"llama3"`` (Llama-3.1 / 3.2): wavelengths longer than
      ``original_max_position_embeddings / low_freq_factor`` are divided by ``factor``,
      shorter than ``.../high_freq_factor`` kept, and the band between is blended with
      ``s = (L_orig / wavelen - low) / (high - low)``: ``(1 - s) * f / factor + s * f``.
    Anything else raises: a checkpoint must not load with silently wrong positions."""
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if not scaling:
        return inv
    kind = scaling.get("rope_type", scaling.get("type", "default"))
    if kind == "default":
        return inv
    factor = float(scaling["factor"])
    if kind == "linear":
        return inv / factor
    if kind == "llama3":
        low, high = float(scaling["low_freq_factor"]), float(scaling["high_freq_factor"])
        orig = float(scaling["original_max_position_embeddings"])
        wavelen = 2 * math.pi / inv
        scaled = torch.where(wavelen > orig / low, inv / factor, inv)
        smooth = (orig / wavelen - low) / (high - low)
        blended = (1 - smooth) * scaled / factor + smooth * scaled
        medium = (wavelen >= orig / high) & (wavelen <= orig / low)
        return torch.where(medium, blended, scaled)
    raise NotImplementedError(f"rope_scaling type {kind!r} is not supported")


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, device=None,
                 scaling: dict | None = None) -> torch.Tensor:
    """fp32 table [max_pos, head_dim]: first half cos, second half sin (rotate-half RoPE)."""
    inv_freq = rope_inv_freq(head_dim, theta, scaling)
    t = torch.arange(max_pos, dtype=torch.float64)
    freqs = torch.outer(t, inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).float().to(device)


def rope_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D):
    T = qkv.shape[0]
    x = qkv.view(T, Hq + 2 * Hkv, D)
    cs = cos_sin[positions.long()]  # [T, D]
    half = D // 2
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    qk = x[:, : Hq + Hkv].float()
    x1, x2 = qk[..., :half], qk[..., half:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(qkv.dtype)
    x[:, : Hq + Hkv] = rot
    if slot_mapping is not None:
        BS = k_cache.shape[2]
        sm = slot_mapping.long()
        valid = sm >= 0
        sm = sm[valid]
        blk, off = sm // BS, sm % BS
        if k_cache.dtype == KV_FP8:
            # FP8 KV cache: the codes are the e4m3 image of the bf16 values the bf16 path would
            # have stored, and the rotated K and the V left in ``qkv`` become the codes' exact
            # image -- the un-paged prefill over ``qkv`` and every paged read attend one model
            kv8 = kv_fp8_codes(x[:, Hq:])
            x[:, Hq:] = kv8.to(qkv.dtype)
            bits = kv8.view(torch.uint8)       # indexing on the code bytes (any device)
            k_cache.view(torch.uint8)[blk, :, off] = bits[valid, :Hkv]
            v_cache.view(torch.uint8)[blk, :, off] = bits[valid, Hkv:]
            return
        k = x[valid, Hq : Hq + Hkv]
        v = x[valid, Hq + Hkv :]
        k_cache[blk, :, off] = k
        v_cache[blk, :, off] = v


KV_FP8 = torch.float8_e4m3fn   # the FP8 paged-KV format: OCP e4m3 codes, no scales


def _kv_gather(cache, blocks):
    """cache[blocks]; an FP8 cache is indexed through its code bytes."""
    if cache.dtype == KV_FP8:
        return cache.view(torch.uint8)[blocks].view(KV_FP8)
    return cache[blocks]


def kv_fp8_codes(x):
    """e4m3 codes of K/V values: clamped to +-448 first (the NaN codes 0x7f / 0xff are never
    produced), then round-to-nearest-even.  A NaN input becomes -448 (code 0xfe), as in the
    kernel, whose ``fminf(fmaxf(x, -448), 448)`` returns the non-NaN operand."""
    return torch.nan_to_num(x.float(), nan=-448.0).clamp(-448.0, 448.0).to(KV_FP8)


def silu_mul(gu, interleaved: bool = False):
    """SwiGLU; ``interleaved``: gate|up rows in blocks of 8 (glu_interleave layout)."""
    if interleaved:
        v = gu.float().unflatten(-1, (-1, 2, 8))
        g, u = v[..., 0, :].flatten(-2), v[..., 1, :].flatten(-2)
    else:
        g, u = gu.float().chunk(2, dim=-1)
    # below g = -88.7 exp(-g) overflows in fp32 and silu(g) becomes -0 although silu(g) * u is
    # still a (sub)normal bf16 value: there silu(g) = g * e^g, with e^g as two e^(g/2) factors
    t = torch.exp(0.5 * g)
    return torch.where(g >= -80.0, F.silu(g) * u, g * t * u * t).to(gu.dtype)


def glu_interleave(gate, up):
    """[I, K] gate and up -> [2I, K] with rows in blocks of 8: g0..g7 u0..u7 g8..g15 ..."""
    I, K = gate.shape
    return torch.stack([gate.view(I // 8, 8, K), up.view(I // 8, 8, K)], 1).reshape(2 * I, K)


def glu_split(gu):
    """Inverse of :func:`glu_interleave`."""
    v = gu.view(-1, 2, 8, gu.shape[-1])
    return v[:, 0].reshape(-1, gu.shape[-1]), v[:, 1].reshape(-1, gu.shape[-1])


FP8_MAX = 448.0          # largest finite OCP e4m3fn value
# amax / scale lands in (232, 464]: 464 is the midpoint between 448 and the next (absent) code,
# so everything up to it rounds to 448 anyway, and the top code is never below 240 -- which is
# what makes quantizing the dequantized image again give the same (q, s).  (With 448 as the
# bound a row whose amax / scale falls in (224, 232] rounds to a top code of 224 and would
# re-quantize to (2 q, s / 2).)  An amax of exactly 448 * 2^e gets scale 2^e either way.
_FP8_BOUND = 464.0
_FP8_MIN_EXP = -100      # q * s stays a normal bf16 / fp32 number down to the smallest code


def quantize_fp8_rows(w):
    """Per-row FP8 weight format: ``w`` [N, K] -> (q [N, K] float8_e4m3fn, s [N] fp32) with
    ``s[n]`` an exact power of two, ``2^ceil(log2(amax_n / 464))`` (1 for an all-zero row), and
    ``q = rne(w / s)`` saturated to +-448 -- the NaN codes 0x7f / 0xff are never produced.
    ``q * s`` has a 3-bit mantissa, so it is exact in bf16 (:func:`dequantize_fp8_rows`)."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    # amax = m * 2^e, m in [0.5, 1); 464 = 0.90625 * 2^9 -- compared exactly, no division
    m, e = torch.frexp(amax)
    ex = torch.where(m > _FP8_BOUND / 512.0, e - 8, e - 9).clamp_(min=_FP8_MIN_EXP)
    s = torch.ldexp(torch.ones_like(amax), ex)
    s = torch.where(amax > 0, s, torch.ones_like(s))
    q = (wf / s[:, None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q, s


def dequantize_fp8_rows(q, s, dtype=torch.bfloat16):
    """``q * s`` of :func:`quantize_fp8_rows` in ``dtype`` (exact in bf16 and fp32); ``q`` as
    float8_e4m3fn or its uint8 codes."""
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    return (q.float() * s.float()[:, None]).to(dtype)


MXFP4_BLOCK = 32         # k per OCP e8m0 block scale
# magnitudes of the OCP e2m1 codes 0..7 (bit 3 of a code is the sign)
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# amax / scale lands in (3.5, 7]: 7 is the rounding boundary above the top code 6 (everything up
# to it rounds to 6 anyway), so a non-zero block's top code is 4 or 6 and quantizing the image
# again gives the same (q, e) -- the 464 of the FP8 rule above
_MXFP4_MIN_EXP, _MXFP4_MAX_EXP = -126, 125


def quantize_mxfp4_rows(w):
    """OCP MXFP4 weight format: ``w`` [N, K], K % 32 == 0 -> (q [N, K / 2] uint8, e [N, K / 32]
    uint8).  ``q`` holds two e2m1 codes per byte, element 2j in bits 0..3 and 2j + 1 in bits 4..7
    (the torch.float4_e2m1fn_x2 order); ``e`` one e8m0 scale 2^(e - 127) per block of 32
    consecutive k, ``2^ceil(log2(amax / 7))`` with the exponent clamped to [-126, 125] (e = 127 for
    an all-zero block; 255 = NaN is never produced).  Elements round to the nearest code, ties to
    the even code, saturating at +-6; NaN -> 0, +-inf saturates.  ``code * scale`` has a 1-bit
    mantissa, so the image is exact in bf16 (:func:`dequantize_mxfp4_rows`)."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"MXFP4 rows need K % {MXFP4_BLOCK} == 0 (got K = {K})")
    wf = torch.nan_to_num(w.detach().float(), nan=0.0, posinf=3e38, neginf=-3e38).clamp_(-3e38, 3e38)
    wb = wf.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wb.abs().amax(dim=2)
    # amax = m * 2^ex, m in [0.5, 1); 7 = 0.875 * 2^3 -- compared exactly, no division
    m, ex = torch.frexp(amax)
    p = torch.where(m > 0.875, ex - 2, ex - 3).clamp_(_MXFP4_MIN_EXP, _MXFP4_MAX_EXP)
    p = torch.where(amax > 0, p, torch.zeros_like(p))
    v = torch.ldexp(wb, -p[:, :, None])                     # exact: a power of two
    a = v.abs().clamp_(max=6.0)
    # code index of the nearest magnitude; torch.round is half-to-even, which on each of the three
    # uniform stretches (step 0.5 below 2, 1 below 4, 2 above) is ties-to-even-code
    idx = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, torch.round(a) + 2, torch.round(a / 2) + 4))
    idx = idx.to(torch.uint8)
    code = idx | (((v < 0) & (idx > 0)).to(torch.uint8) << 3)     # no negative zero
    code = code.view(N, K // 2, 2)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    return q.contiguous(), (p + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4_rows(q, e, dtype=torch.bfloat16):
    """The image ``code * 2^(e - 127)`` [N, K] of :func:`quantize_mxfp4_rows` in ``dtype`` (exact in
    bf16 and fp32)."""
    N, K = q.shape[0], q.shape[1] * 2
    lut = torch.tensor(_E2M1 + tuple(-x for x in _E2M1), dtype=torch.float32, device=q.device)
    codes = torch.stack([q & 0xF, q >> 4], dim=2).view(N, K).int()
    vals = lut[codes].view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    return torch.ldexp(vals, e.to(torch.int32)[:, :, None] - 127).view(N, K).to(dtype)


def bias_act(x, bias, residual, gelu):
    y = x.float()
    if residual is not None:
        y = y + residual.float()
    y = y + bias.float()
    if gelu:
        y = F.gelu(y)  # erf form
    return y.to(x.dtype)


def linear_fused(x, w, bias, residual, epi):
    """epi: 0 none, 1 bias, 2 bias+gelu, 3 bias+residual (fp32 accumulate, bf16 out)."""
    y = x.float() @ w.float().T
    if epi >= 1:
        y = y + bias.float()
    if epi == 2:
        y = F.gelu(y)
    if epi == 3:
        y = y + residual.float()
    return y.to(x.dtype)


def embedding(ids, table):
    return table[ids.long()]


def bert_embed_ln(ids, pos, token_type, wte, wpe, wtt, gamma, beta, eps):
    tt = token_type.long() if token_type is not None else torch.zeros_like(ids, dtype=torch.long)
    e = wte[ids.long()].float() + wpe[pos.long()].float() + wtt[tt].float()
    return F.layer_norm(e, (wte.shape[1],), gamma.float(), beta.float(), eps).to(wte.dtype)


def argmax(logits):
    return logits.float().argmax(dim=-1)


def token_cls_argmax(h, w, bias, n_valid):
    logits = h.float() @ w[:n_valid].float().t() + bias[:n_valid].float()
    return logits.argmax(dim=-1)


def sample(logits, inv_temp, top_k, top_p, u):
    out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    for r in range(logits.shape[0]):
        x = logits[r].float() * float(inv_temp[r])
        k = int(top_k[r])
        if k == 1:      # greedy row: the lowest index of the maximum, whatever u and top_p are
            out[r] = int(torch.nonzero(x == x.max())[0])
            continue
        if 0 < k < x.numel():
            th = torch.topk(x, k).values[-1]
            x = torch.where(x >= th, x, torch.full_like(x, -math.inf))
        p = torch.softmax(x, -1)
        tp = float(top_p[r])
        if 0.0 < tp < 1.0:
            sp, si = torch.sort(p, descending=True)
            keep = torch.cumsum(sp, 0) - sp < tp
            mask = torch.zeros_like(p, dtype=torch.bool)
            mask[si[keep]] = True
            p = torch.where(mask, p, torch.zeros_like(p))
            p = p / p.sum()
        # first index whose cumulative mass exceeds u: a dropped token (p == 0) never
        # satisfies that, and a u the rounded total falls short of takes the last kept token
        c = torch.cumsum(p, 0)
        idx = int(torch.searchsorted(c, torch.tensor([float(u[r])], device=c.device), right=True))
        out[r] = min(idx, int(torch.nonzero(p > 0)[-1]))
    return out


_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32(counter, key, rounds: int = 10):
    """Philox4x32 (Salmon et al., Random123) in Python integers: ``counter`` four and ``key`` two
    32-bit words -> the four output words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(rounds):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def seeded_uniform(seed, index):
    """fp32 [R] in [0, 1): the first word of philox4x32 with key (seed & 0xffffffff, seed >> 32)
    and counter (index, 0, 0, 0), as ``float(w0 >> 8) * 2^-24`` -- exact in fp32, at most
    1 - 2^-24.  Integer arithmetic throughout: the device kernel agrees bit for bit."""
    out = torch.empty(len(seed), dtype=torch.float32)
    for r, (s, i) in enumerate(zip(seed.tolist(), index.tolist())):
        s &= 0xFFFFFFFFFFFFFFFF
        w0 = philox4x32((i, 0, 0, 0), (s & _M32, s >> 32))[0]
        out[r] = (w0 >> 8) * 2.0 ** -24
    return out.to(seed.device)


def sample_tokens(logits, n_valid, inv_temp, top_k, top_p, min_p, u=None, seed=None, index=None, valid=None):
    """:func:`sample` over the columns below ``n_valid`` plus the ``min_p`` filter
    (``x >= max(x) + log(min_p)``, in fp32 like the kernel), the row's uniform either ``u`` or
    :func:`seeded_uniform`; rows with ``valid == 0`` get token 0."""
    R = logits.shape[0]
    if u is None:
        u = seeded_uniform(seed[:R], index[:R])
    out = torch.zeros(R, dtype=torch.long, device=logits.device)
    for r in range(R):
        if valid is not None and int(valid[r]) == 0:
            continue
        x = logits[r, :n_valid].float() * inv_temp[r].float()
        k = int(top_k[r])
        if k == 1:      # greedy row: the lowest index of the maximum, whatever else is set
            out[r] = int(torch.nonzero(x == x.max())[0])
            continue
        keep = torch.ones_like(x, dtype=torch.bool)
        if 0 < k < x.numel():
            keep = x >= torch.topk(x, k).values[-1]
        p = torch.softmax(torch.where(keep, x, torch.full_like(x, -math.inf)), -1)
        tp = float(top_p[r])
        if 0.0 < tp < 1.0:
            sx = torch.sort(torch.where(keep, x, torch.full_like(x, -math.inf)), descending=True).values
            sp = torch.softmax(sx, -1)
            n = int((torch.cumsum(sp, 0) - sp < tp).sum())      # the prefix; then its ties
            keep = keep & (x >= sx[n - 1])
        mp = float(min_p[r]) if min_p is not None else 0.0
        if mp > 0.0:
            keep = keep & (x >= x.max() + torch.log(torch.tensor(min(mp, 1.0), dtype=torch.float32)))
        p = torch.where(keep, p, torch.zeros_like(p))
        p = p / p.sum()
        c = torch.cumsum(p, 0)
        idx = int(torch.searchsorted(c, torch.tensor([float(u[r])], device=c.device), right=True))
        out[r] = min(idx, int(torch.nonzero(p > 0)[-1]))
    return out


def paged_decode(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context, scale):
    B = q.shape[0]
    NB, Hkv, BS, D = k_cache.shape
    G = Hq // Hkv
    out = torch.empty(B, Hq * D, dtype=q.dtype, device=q.device)
    for b in range(B):
        L = int(context_lens[b])
        nblk = (L + BS - 1) // BS
        blocks = block_tables[b, :nblk].long()
        k = _kv_gather(k_cache, blocks).permute(1, 0, 2, 3).reshape(Hkv, nblk * BS, D)[:, :L].float()
        v = _kv_gather(v_cache, blocks).permute(1, 0, 2, 3).reshape(Hkv, nblk * BS, D)[:, :L].float()
        qb = q[b, : Hq * D].view(Hkv, G, D).float()
        s = torch.einsum("hgd,htd->hgt", qb, k) * scale
        p = torch.softmax(s, -1)
        o = torch.einsum("hgt,htd->hgd", p, v)
        out[b] = o.reshape(-1).to(q.dtype)
    return out


def paged_decode_cascade(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context, scale,
                         prefix_table, prefix_len, nchunk=8):
    """Cascade decode attention: keys [0, P) come from the shared ``prefix_table`` blocks,
    keys [P, L) from each sequence's own block table (one softmax over both)."""
    B = q.shape[0]
    NB, Hkv, BS, D = k_cache.shape
    G = Hq // Hkv
    P = int(prefix_len.reshape(-1)[0])
    pb = prefix_table.reshape(-1)[: P // BS].long()
    kp = _kv_gather(k_cache, pb).permute(1, 0, 2, 3).reshape(Hkv, -1, D).float()
    vp = _kv_gather(v_cache, pb).permute(1, 0, 2, 3).reshape(Hkv, -1, D).float()
    out = torch.zeros(B, Hq * D, dtype=q.dtype, device=q.device)
    for b in range(B):
        L = int(context_lens[b])
        if L <= P:
            continue
        nblk = (L + BS - 1) // BS
        blocks = block_tables[b, P // BS:nblk].long()
        ks = _kv_gather(k_cache, blocks).permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, : L - P].float()
        vs = _kv_gather(v_cache, blocks).permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, : L - P].float()
        k, v = torch.cat([kp, ks], 1), torch.cat([vp, vs], 1)
        qb = q[b, : Hq * D].view(Hkv, G, D).float()
        p = torch.softmax(torch.einsum("hgd,htd->hgt", qb, k) * scale, -1)
        out[b] = torch.einsum("hgt,htd->hgd", p, v).reshape(-1).to(q.dtype)
    return out


def flash_prefill(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, causal):
    T = qkv.shape[0]
    x = qkv.view(T, Hq + 2 * Hkv, D)
    G = Hq // Hkv
    out = torch.empty(T, Hq * D, dtype=qkv.dtype, device=qkv.device)
    cu = cu_seqlens.tolist()
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        L = s1 - s0
        if L == 0:
            continue
        q = x[s0:s1, :Hq].float().transpose(0, 1)  # [Hq, L, D]
        k = x[s0:s1, Hq : Hq + Hkv].float().transpose(0, 1).repeat_interleave(G, 0)
        v = x[s0:s1, Hq + Hkv :].float().transpose(0, 1).repeat_interleave(G, 0)
        s = torch.einsum("hld,hmd->hlm", q, k) * scale
        if causal:
            mask = torch.ones(L, L, dtype=torch.bool, device=qkv.device).triu(1)
            s = s.masked_fill(mask, -math.inf)
        o = torch.einsum("hlm,hmd->hld", torch.softmax(s, -1), v)
        out[s0:s1] = o.transpose(0, 1).reshape(L, Hq * D).to(qkv.dtype)
    return out


def flash_prefill_paged(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, k_cache, v_cache,
                        block_tables, ctx_start):
    """Causal attention of the new tokens over (cached prefix + new) keys read from the
    paged cache (the new keys must already be written there)."""
    T = qkv.shape[0]
    x = qkv.view(T, Hq + 2 * Hkv, D)
    G = Hq // Hkv
    BS = k_cache.shape[2]
    out = torch.empty(T, Hq * D, dtype=qkv.dtype, device=qkv.device)
    cu = cu_seqlens.tolist()
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        L = s1 - s0
        if L == 0:
            continue
        P0 = int(ctx_start[b])
        Lk = P0 + L
        nblk = (Lk + BS - 1) // BS
        blocks = block_tables[b, :nblk].long()
        k = _kv_gather(k_cache, blocks).permute(1, 0, 2, 3).reshape(Hkv, nblk * BS, D)[:, :Lk].float()
        v = _kv_gather(v_cache, blocks).permute(1, 0, 2, 3).reshape(Hkv, nblk * BS, D)[:, :Lk].float()
        k = k.repeat_interleave(G, 0)
        v = v.repeat_interleave(G, 0)
        q = x[s0:s1, :Hq].float().transpose(0, 1)
        s = torch.einsum("hld,hmd->hlm", q, k) * scale
        qpos = torch.arange(P0, Lk, device=qkv.device)[:, None]
        kpos = torch.arange(Lk, device=qkv.device)[None, :]
        s = s.masked_fill(kpos > qpos, -math.inf)
        o = torch.einsum("hlm,hmd->hld", torch.softmax(s, -1), v)
        out[s0:s1] = o.transpose(0, 1).reshape(L, Hq * D).to(qkv.dtype)
    return out


def knn(xb, xb_norms, xq, k, inner_product, id_offset):
    """FAISS IndexFlat semantics: L2 -> ascending squared distances, IP -> descending."""
    nq = xq.shape[0]
    N = xb.shape[0]
    D = torch.full((nq, k), -3.4028234663852886e38 if inner_product else 3.4028234663852886e38,
                   dtype=torch.float32, device=xq.device)
    I = torch.full((nq, k), -1, dtype=torch.long, device=xq.device)
    if N == 0 or nq == 0:
        return D, I
    xbf = xb.float()
    xqf = xq.float()
    ip = xqf @ xbf.T
    if inner_product:
        vals, idx = torch.topk(ip, min(k, N), dim=1, largest=True)
    else:
        norms = xb_norms.float() if xb_norms is not None else (xbf * xbf).sum(1)
        d = (xqf * xqf).sum(1, keepdim=True) + norms[None, :] - 2 * ip
        vals, idx = torch.topk(d, min(k, N), dim=1, largest=False)
    D[:, : vals.shape[1]] = vals
    I[:, : idx.shape[1]] = idx + id_offset
    return D, I


def knn_scoped(xb, xb_norms, tags, days, xq, scope, k, inner_product, id_offset):
    """:func:`knn` among the rows inside each query's scope.  tags / days int32 [N], scope
    int32 [nq, 4] = (tag, alt_tag, day_lo, day_hi); a row matches iff

        row_tag == alt_tag || ((tag < 0 || row_tag == tag) && day_lo <= row_day && row_day <= day_hi)

    (tag -1 = any, alt_tag -1 = none, 0 = also the knowledge base, exempt from the window;
    (INT32_MIN, INT32_MAX) = no window; an undated row carries day INT32_MIN).  Slots past
    the number of matching rows hold -1 and the sentinel distance."""
    nq = xq.shape[0]
    N = xb.shape[0]
    sent = -3.4028234663852886e38 if inner_product else 3.4028234663852886e38
    D = torch.full((nq, k), sent, dtype=torch.float32, device=xq.device)
    I = torch.full((nq, k), -1, dtype=torch.long, device=xq.device)
    if N == 0 or nq == 0:
        return D, I
    rt, rd = tags.reshape(-1)[None, :].int(), days.reshape(-1)[None, :].int()
    sc = scope.int()
    tag, alt, lo, hi = (sc[:, j:j + 1] for j in range(4))
    match = (rt == alt) | (((tag < 0) | (rt == tag)) & (lo <= rd) & (rd <= hi))
    xbf = xb.float()
    xqf = xq.float()
    ip = xqf @ xbf.T
    if inner_product:
        score = ip.masked_fill(~match, -math.inf)
        vals, idx = torch.topk(score, min(k, N), dim=1, largest=True)
    else:
        norms = xb_norms.float() if xb_norms is not None else (xbf * xbf).sum(1)
        score = ((xqf * xqf).sum(1, keepdim=True) + norms[None, :] - 2 * ip).masked_fill(~match, math.inf)
        vals, idx = torch.topk(score, min(k, N), dim=1, largest=False)
    ok = torch.gather(match, 1, idx)
    D[:, : vals.shape[1]] = torch.where(ok, vals, torch.full_like(vals, sent))
    I[:, : idx.shape[1]] = torch.where(ok, idx + id_offset, torch.full_like(idx, -1))
    return D, I


def bm25_topk(row_ptr, terms, tfs, dl, qterms, qweights, k, avgdl, k1=1.2, b=0.75, tags=None, days=None,
              scope=None, id_offset=0):
    """BM25 (Lucene >= 8: no ``(k1 + 1)`` factor) over CSR term columns, fp32 throughout:

        K_r   = k1 * ((1 - b) + (b * dl_r) / avgdl)
        s_q,r = sum over the row's entries, in entry order, of  w_q,t * (tf / (tf + K_r))

    row_ptr int64 [N+1], terms int32 [E] (32-bit hashes, unique per row), tfs uint8 [E], dl
    int32 [N]; qterms int32 / qweights fp32 [nq, 32], ``0xFFFFFFFF`` pads and a term repeated in
    one query row counts once (its first slot).  A row competes iff it holds one of the
    query's terms and passes its scope row (``knn_scoped``'s predicate; ``scope`` None:
    unscoped).  -> (S fp32 [nq, k] descending, ties towards the lower row, I int64 [nq, k]);
    missing slots hold ``-FLT_MAX`` / -1.  The sum order is the kernel's (csrc/kernels/lexical.hip)."""
    dev = row_ptr.device
    N, nq = row_ptr.numel() - 1, qterms.shape[0]
    S = torch.full((nq, k), -3.4028234663852886e38, dtype=torch.float32, device=dev)
    I = torch.full((nq, k), -1, dtype=torch.long, device=dev)
    if N <= 0 or nq == 0:
        return S, I
    rp = row_ptr.long()
    E = int(rp[-1])
    row_of = torch.repeat_interleave(torch.arange(N, device=dev), rp[1:] - rp[:-1])
    t = terms[:E].long() & 0xFFFFFFFF
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)  # noqa: E731 - every scalar rounded once
    Kr = f32(k1) * (f32(1.0 - b) + (f32(b) * dl.float()) / f32(avgdl))
    tf = tfs[:E].float()
    x = tf / (tf + Kr[row_of])
    match = None
    if scope is not None:
        rt, rd = tags.reshape(-1)[None, :].int(), days.reshape(-1)[None, :].int()
        tag, alt, lo, hi = (scope.int()[:, j:j + 1] for j in range(4))
        match = (rt == alt) | (((tag < 0) | (rt == tag)) & (lo <= rd) & (rd <= hi))
    qt_host = (qterms.long() & 0xFFFFFFFF).tolist()
    for q in range(nq):
        first: dict[int, int] = {}
        for j, h in enumerate(qt_host[q]):
            if h != 0xFFFFFFFF and h not in first:
                first[h] = j
        if not first or E == 0:
            continue
        st = torch.tensor(sorted(first), dtype=torch.long, device=dev)
        sw = qweights[q].float()[torch.tensor([first[h] for h in sorted(first)], dtype=torch.long, device=dev)]
        pos = torch.searchsorted(st, t).clamp(max=st.numel() - 1)
        he = (st[pos] == t).nonzero().squeeze(1)            # hit entries, ascending
        if he.numel() == 0:
            continue
        c = sw[pos[he]] * x[he]
        r = row_of[he]
        idx = torch.arange(he.numel(), device=dev)
        new = torch.ones_like(r, dtype=torch.bool)
        new[1:] = r[1:] != r[:-1]
        level = idx - torch.cummax(torch.where(new, idx, torch.zeros_like(idx)), 0).values
        score = torch.zeros(N, dtype=torch.float32, device=dev)
        for lv in range(int(level.max()) + 1):              # the lv-th hit of every row: one add per row
            m = level == lv
            score[r[m]] = score[r[m]] + c[m]
        cand = torch.zeros(N, dtype=torch.bool, device=dev)
        cand[r] = True
        if match is not None:
            cand &= match[q]
        vals, order = torch.sort(score.masked_fill(~cand, -math.inf), descending=True, stable=True)
        vals, order = vals[:k], order[:k]
        ok = cand[order]
        S[q, : vals.numel()] = torch.where(ok, vals, torch.full_like(vals, -3.4028234663852886e38))
        I[q, : order.numel()] = torch.where(ok, order + id_offset, torch.full_like(order, -1))
    return S, I


def rank_fuse(I_dense, I_lex, mode, k, c=60):
    """Per query (mode 0 / 1 / 2): the first k ids of ``I_dense``, of ``I_lex``, or of their
    reciprocal rank fusion -- an id scores the sum over the lists holding it of
    ``1 / (c + rank)``, rank = its 1-based position; negative ids are ignored and a repeated
    id counts at its first position.  Order: score descending, compared exactly
    (``fractions.Fraction``), ties towards the lower id.  -> (F fp32 [nq, k] = num / den of the
    score, I int64 [nq, k]); missing slots hold 0 / -1."""
    from fractions import Fraction

    dev = I_dense.device
    a_all, b_all, modes = I_dense.tolist(), I_lex.tolist(), mode.tolist()
    nq = len(modes)
    num = torch.zeros((nq, k), dtype=torch.float32)
    den = torch.ones((nq, k), dtype=torch.float32)
    I = torch.full((nq, k), -1, dtype=torch.long)
    for q in range(nq):
        score: dict[int, Fraction] = {}
        for use, ids in ((modes[q] != 1, a_all[q]), (modes[q] != 0, b_all[q])):
            seen = set()
            for pos, i in enumerate(ids if use else ()):
                if i >= 0 and i not in seen:
                    seen.add(i)
                    score[i] = score.get(i, Fraction(0)) + Fraction(1, c + pos + 1)
        for j, (i, s) in enumerate(sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))[:k]):
            # the kernel's (num, den) are unreduced: (a + b, a b) or (1, a); both are exact in fp32
            num[q, j], den[q, j], I[q, j] = s.numerator, s.denominator, i
    return (num / den).to(dev), I.to(dev)


def mmr_select(xb, xb_norms, xq, cand, ncand, lam, k):
    """Maximal marginal relevance over ranked candidate lists (LangChain's
    ``maximal_marginal_relevance``, all fp32).  cand int64 [nq, F] (best first; only the first
    ``ncand[q]`` entries with an id in ``[0, N)`` are candidates), lam fp32 [nq]:

        cos(a, b) = dot(a, b) / sqrt(|a|^2 * |b|^2), 0 when that root is 0
        pick 0    = argmax cos(q, c)
        pick t    = argmax over the unpicked c of  lam * cos(q, c) - (1 - lam) * max_s cos(c, s)

    ``|row|^2`` is ``xb_norms``; ties go to the earlier position; min(k, candidates) picks.
    ``lam < 0``: the row's first k entries pass through (S = 0, P = 0..k-1).  -> (S fp32 = the
    value that won each pick, I int64 = its id, P int32 = its position in ``cand``), missing
    slots 0 / -1 / -1.  The same id at two positions is two candidates."""
    dev = xq.device
    nq, F = cand.shape
    N = xb.shape[0]
    S = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    I = torch.full((nq, k), -1, dtype=torch.long, device=dev)
    P = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    if nq == 0:
        return S, I, P
    cand = cand.long()
    lam = lam.float().reshape(nq)
    kk = min(k, F)
    off = lam < 0
    pos = torch.arange(F, device=dev)
    I[:, :kk] = torch.where(off[:, None], cand[:, :kk], I[:, :kk])
    P[:, :kk] = torch.where(off[:, None], pos[None, :kk].int(), P[:, :kk])
    if N == 0 or F == 0:
        return S, I, P
    valid = (pos[None, :] < ncand.reshape(nq, 1)) & (cand >= 0) & (cand < N) & ~off[:, None]
    idx = cand.clamp(0, N - 1)
    rows = xb[idx.reshape(-1)].float().reshape(nq, F, -1) * valid[:, :, None]
    nb = xb_norms.float()[idx] * valid
    q = xq.float()
    qn = (q * q).sum(1)

    def cosine(dot, na, nb_):
        den = torch.sqrt(na * nb_)
        return torch.where(den > 0, dot / den, torch.zeros_like(dot))

    rel = cosine(torch.bmm(rows, q[:, :, None])[:, :, 0], qn[:, None], nb)
    sim = cosine(torch.bmm(rows, rows.transpose(1, 2)), nb[:, :, None], nb[:, None, :])
    avail = valid.clone()
    red = torch.zeros_like(rel)
    lm, oml = lam[:, None], (1.0 - lam)[:, None]
    ar = torch.arange(nq, device=dev)
    for t in range(kk):
        score = rel if t == 0 else lm * rel - oml * red
        p = torch.where(avail, score, torch.full_like(score, -math.inf)).argmax(1)
        on = avail.any(1)
        S[:, t] = torch.where(on, score[ar, p], S[:, t])
        I[:, t] = torch.where(on, cand[ar, p], I[:, t])
        P[:, t] = torch.where(on, p.int(), P[:, t])
        avail[ar, p] = False
        red = sim[ar, p] if t == 0 else torch.maximum(red, sim[ar, p])
    return S, I, P


def pool_l2(h, cu_seqlens, mean, normalize):
    cu = cu_seqlens.tolist()
    out = torch.zeros(len(cu) - 1, h.shape[-1], dtype=torch.float32, device=h.device)
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        if s1 > s0:
            out[b] = h[s0:s1].float().mean(0) if mean else h[s0].float()
    if normalize:
        out = F.normalize(out, dim=-1, eps=1e-12)
    return out


def decode_slots(block_tables, positions, valid, BS: int):
    blk = torch.gather(block_tables, 1, (positions // BS).long().clamp(max=block_tables.shape[1] - 1)[:, None])[:, 0]
    return torch.where(valid.bool(), blk * BS + positions % BS, torch.full_like(blk, -1)).int()


def decode_advance(nxt, out, tokens, positions, context_lens, valid) -> None:
    out.copy_(nxt)
    tokens.copy_(nxt.int())
    positions.add_(valid)
    context_lens.add_(valid)


PENALTY_WINDOW = 256   # ring capacity W of the token history (embed_sample.hip kPenaltyWindow)


def penalty_neutral(last_n: int, rp: float, pp: float, fp: float) -> bool:
    return last_n == 0 or (rp == 1.0 and pp == 0.0 and fp == 0.0)


def _window_counts(hist_row, hist_n: int, last_n: int, V: int) -> dict:
    """{token: count} over the newest min(hist_n, last_n, W) ring entries (stream entry j sits
    at hist_row[j % W]; last_n < 0 or above W means W); ids outside [0, V) are ignored."""
    W = hist_row.numel()
    n = max(0, min(hist_n, W))
    if 0 <= last_n < n:
        n = last_n
    ring = hist_row.tolist()
    counts: dict = {}
    for j in range(hist_n - n, hist_n):
        t = ring[j % W]
        if 0 <= t < V:
            counts[t] = counts.get(t, 0) + 1
    return counts


def _penalize_row(x, counts: dict, rp, pp, fp) -> None:
    """In place on the fp32 row ``x``; rp / pp / fp are fp32 0-d tensors.  Every operation is
    rounded to fp32 on its own, in the kernels' order: l = l <= 0 ? l * rp : l / rp, then
    l = l - (c * fp + pp)."""
    for t, c in counts.items():
        l = x[t]
        l = l * rp if bool(l <= 0) else l / rp
        x[t] = l - (torch.tensor(float(c), dtype=torch.float32) * fp + pp)


def _row_params(r, hist_n, last_n, rep_pen, pres_pen, freq_pen):
    f32 = lambda v: v[r].detach().to("cpu", torch.float32)   # noqa: E731
    return int(hist_n[r]), int(last_n[r]), f32(rep_pen), f32(pres_pen), f32(freq_pen)


def apply_penalties(logits, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid=None) -> None:
    """llama.cpp's repeat / presence / frequency penalties, in place on fp32 logits [R, V]."""
    assert logits.dtype == torch.float32
    V = logits.shape[1]
    for r in range(logits.shape[0]):
        hn, ln, rp, pp, fp = _row_params(r, hist_n, last_n, rep_pen, pres_pen, freq_pen)
        if (valid is not None and int(valid[r]) == 0) or penalty_neutral(ln, float(rp), float(pp), float(fp)):
            continue
        counts = _window_counts(hist[r].cpu(), hn, ln, V)
        if counts:
            idx = torch.tensor(list(counts), dtype=torch.long)
            x = logits[r, idx].cpu()
            _penalize_row(x, {i: c for i, c in enumerate(counts.values())}, rp, pp, fp)
            logits[r, idx.to(logits.device)] = x.to(logits.device)


def penalized_argmax(logits, n_valid: int, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid=None):
    """argmax over t < n_valid of the penalised logits (unpenalised entries as float(logit)),
    ties to the lowest index; the input is left unchanged here."""
    x = logits[:, :n_valid].float().clone()
    apply_penalties(x, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid)
    return x.argmax(dim=-1)


TOP_LOGPROBS_MAX = 20   # columns of the top list (logprobs.hip kTop)


def token_logprobs(logits, n_valid: int, chosen, top_n, lp, top_ids, top_lp) -> None:
    """Per-token log-probabilities in fp32, in place on lp [R], top_ids / top_lp [R, 20]:
    lp[r] = logit[r, chosen[r]] - logsumexp(logit[r, :n_valid]) and the top_n[r] most likely
    tokens in descending order, ties to the lower id; entries past top_n[r] (or past n_valid)
    are (-1, -inf).  Rows with top_n[r] < 0 are left untouched.  Values are formed as
    (x - max) - log(sum exp(x - max)), like the kernel."""
    x = logits[:, :n_valid].float()
    for r in range(x.shape[0]):
        tn = min(int(top_n[r]), TOP_LOGPROBS_MAX)
        if tn < 0:
            continue
        d = x[r] - x[r].max()
        rel = d - torch.log(torch.exp(d).sum())
        c = int(chosen[r])
        lp[r] = rel[c] if 0 <= c < n_valid else -math.inf
        top_ids[r] = -1
        top_lp[r] = -math.inf
        k = min(tn, n_valid)
        if k > 0:
            ids = torch.sort(x[r], descending=True, stable=True).indices[:k]   # stable: the lower id first
            top_ids[r, :k] = ids.to(top_ids.dtype)
            top_lp[r, :k] = rel[ids]


def decode_advance_hist(nxt, out, tokens, positions, context_lens, valid, hist, hist_n) -> None:
    W = hist.shape[1]
    rows = torch.nonzero(valid.bool())[:, 0]
    hist[rows, (hist_n[rows] % W).long()] = nxt[rows].int()
    hist_n.add_(valid)
    decode_advance(nxt, out, tokens, positions, context_lens, valid)


def coarse_probes(xq, centroids, cnorm, nprobe: int):
    """fp32 reference of csrc/kernels/coarse.hip: ||c||^2 - 2 q.c per (query, centroid),
    the nprobe smallest in ascending order, ties to the lower centroid id (stable sort)."""
    d = cnorm.float()[None, :] - 2.0 * (xq.float() @ centroids.float().t())
    order = torch.sort(d, dim=1, stable=True).indices
    return order[:, :nprobe].contiguous()


# ----------------------------------------------------------------------------- grammar (format: "json")
def _grammar_allowed(state: int, n: int, off, data, tab, eos_id: int):
    """bool [n]: which of the tokens [0, n) a row in ``state`` (non-zero) may emit -- every token
    walked at once, one byte position per numpy pass over the tokens still alive."""
    import numpy as np

    from . import grammar as G

    allowed = np.zeros(n, dtype=bool)
    if G.is_done(state):
        if 0 <= eos_id < n:
            allowed[eos_id] = True
        return allowed
    nt = min(n, len(off) - 1)
    lens = (off[1:nt + 1] - off[:nt]).astype(np.int64)
    idx = np.nonzero(lens > 0)[0]
    lex0, ws0, depth0, stack0 = G.unpack(state)
    lex = np.full(idx.size, lex0, dtype=np.int64)
    ws = np.full(idx.size, ws0, dtype=np.int64)
    depth = np.full(idx.size, depth0, dtype=np.int64)
    stack = np.full(idx.size, stack0, dtype=np.int64)
    j = 0
    while idx.size:
        ok = lex < tab.shape[0]
        e = tab[np.minimum(lex, tab.shape[0] - 1), data[off[idx] + j]].astype(np.int64)
        nxt, op = e & 0xFF, e >> 8
        top = stack >> np.maximum(depth - 1, 0) & 1
        is_ws, push, pop = op == G.OP_WS, (op == G.OP_PUSH_OBJ) | (op == G.OP_PUSH_ARR), \
            (op == G.OP_POP_OBJ) | (op == G.OP_POP_ARR)
        ok &= op != G.OP_REJECT
        ok &= ~(is_ws & (ws >= G.WS_CAP))
        ok &= ~(push & (depth >= G.DEPTH_CAP))
        ok &= ~(pop & ((depth == 0) | (top != (op == G.OP_POP_ARR))))
        ok &= ~((op == G.OP_COMMA) & (depth == 0))
        ws = np.where(is_ws, ws + 1, 0)
        stack = np.where(push, stack | (op == G.OP_PUSH_ARR).astype(np.int64) << np.minimum(depth, 62), stack)
        depth = depth + push - pop
        stack = np.where(pop, stack & ~(np.int64(1) << np.maximum(depth, 0)), stack)
        lex = np.where(pop, np.where(depth == 0, G.DONE, G.AFTER_VALUE),
                       np.where(op == G.OP_COMMA, np.where(top == 1, G.EXPECT_VALUE, G.EXPECT_KEY), nxt))
        j += 1
        ended = ok & (lens[idx] == j)
        allowed[idx[ended]] = True
        go = ok & ~ended
        idx, lex, ws, depth, stack = idx[go], lex[go], ws[go], depth[go], stack[go]
    if 0 <= eos_id < n:
        allowed[eos_id] = False      # EOS only in DONE, whatever bytes it has
    return allowed


def grammar_mask(logits, n_valid: int, state, tok_off, tok_bytes, table, eos_id: int, valid=None) -> None:
    """In place: -inf into every column t < n_valid of a constrained row (state != 0, valid != 0)
    whose token the row's automaton state does not allow (ops.grammar); nothing else is written.
    Rows in the same state share one walk of the vocabulary."""
    off, data, tab = tok_off.cpu().numpy(), tok_bytes.cpu().numpy(), table.cpu().numpy()
    states = state.tolist()
    cache: dict = {}
    for r in range(logits.shape[0]):
        s = states[r]
        if s == 0 or (valid is not None and int(valid[r]) == 0):
            continue
        if s not in cache:
            cache[s] = torch.from_numpy(~_grammar_allowed(s, int(n_valid), off, data, tab, int(eos_id)))
        logits[r, :n_valid].masked_fill_(cache[s].to(logits.device), -math.inf)


def grammar_advance(state, nxt, tok_off, tok_bytes, table, eos_id: int, valid=None) -> None:
    """In place on state int64 [R]: the automaton after the bytes of token nxt[i]; 0 and DONE
    stay, EOS and a token that would be rejected leave the state unchanged."""
    from . import grammar as G

    off, data = tok_off.cpu().numpy(), tok_bytes.cpu().numpy()
    tab = table.cpu().numpy().astype("int32").tolist()
    states, toks = state.tolist(), nxt.tolist()
    for r, (s, t) in enumerate(zip(states, toks)):
        if s == 0 or G.is_done(s) or t == eos_id or (valid is not None and int(valid[r]) == 0):
            continue
        if not 0 <= t < len(off) - 1 or off[t + 1] == off[t]:
            continue
        for b in data[off[t]:off[t + 1]].tolist():
            s = G.step(s, b, tab)
            if s < 0:
                break
        if s >= 0:
            state[r] = s


# ----------------------------------------------------------------------------- JSON schema (format: a schema)
def _schema_allowed(word: int, n: int, off, data, tables, eos_id: int):
    """bool [n]: which of the tokens [0, n) a row with state ``word`` (non-zero) may emit; ``tables``
    is the (cls, trans) of the row's pool slot, or None (nothing is allowed)."""
    return _schema_walk(word, n, off, data, tables, eos_id)[0]


def _schema_walk(word: int, n: int, off, data, tables, eos_id: int):
    """(allowed bool [n], after int64 [n]) of a row with state ``word`` (non-zero): which of the
    tokens [0, n) it may emit, and its word after each of them (``word`` itself where the token
    leaves it unchanged: not allowed, EOS, no bytes) -- every token walked at once, one byte
    position per numpy pass over the tokens still alive."""
    import numpy as np

    from . import json_schema as J

    allowed = np.zeros(n, dtype=bool)
    after = np.full(n, word, dtype=np.int64)
    if J.is_done(word):
        if 0 <= eos_id < n:
            allowed[eos_id] = True
        return allowed, after
    st0, ws0, slot = J.unpack(word)
    if tables is None or st0 >= tables[1].shape[0]:
        return allowed, after
    cls, trans = tables
    ns, nc = trans.shape
    flat = trans.reshape(-1).astype(np.int64)
    nt = min(n, len(off) - 1)
    lens = (off[1:nt + 1] - off[:nt]).astype(np.int64)
    idx = np.nonzero(lens > 0)[0]
    st = np.full(idx.size, st0, dtype=np.int64)
    ws = np.full(idx.size, ws0, dtype=np.int64)
    j = 0
    while idx.size:
        c = cls[data[off[idx] + j]].astype(np.int64)
        ok = c < nc
        e = flat[st * nc + np.minimum(c, nc - 1)]
        nxt, is_ws = e & J.NEXT_MASK, (e & J.WS_FLAG) != 0
        ok &= (e != 0) & (nxt < ns) & ~(is_ws & (ws >= J.WS_CAP))
        ws = np.where(is_ws, ws + 1, 0)
        st = np.minimum(nxt, ns - 1)
        j += 1
        ended = ok & (lens[idx] == j)
        allowed[idx[ended]] = True
        after[idx[ended]] = st[ended] | ws[ended] << 16 | slot << 21
        go = ok & ~ended
        idx, st, ws = idx[go], st[go], ws[go]
    if 0 <= eos_id < n:
        allowed[eos_id] = False      # EOS only in DONE, whatever bytes it has
        after[eos_id] = word
    return allowed, after


def schema_mask(logits, n_valid: int, sstate, tok_off, tok_bytes, pool, eos_id: int, valid=None) -> None:
    """In place: -inf into every column t < n_valid of a schema row (word != 0, valid != 0) whose
    token the automaton of the row's pool slot does not allow in the row's state
    (ops.json_schema); nothing else is written.  Rows with the same word share one walk."""
    from . import json_schema as J

    off, data, pool_np = tok_off.cpu().numpy(), tok_bytes.cpu().numpy(), pool.cpu().numpy()
    words = sstate.tolist()
    cache: dict = {}
    for r in range(logits.shape[0]):
        w = words[r]
        if w == 0 or (valid is not None and int(valid[r]) == 0):
            continue
        if w not in cache:
            tables = J.pool_tables(pool_np, J.unpack(w)[2])
            cache[w] = torch.from_numpy(~_schema_allowed(w, int(n_valid), off, data, tables, int(eos_id)))
        logits[r, :n_valid].masked_fill_(cache[w].to(logits.device), -math.inf)


def schema_advance(sstate, nxt, tok_off, tok_bytes, pool, eos_id: int, valid=None) -> None:
    """In place on sstate int64 [R]: the word after the bytes of token nxt[i]; 0 and DONE stay,
    EOS and a token that would be rejected (or has no bytes) leave the word unchanged."""
    from . import json_schema as J

    off, data, pool_np = tok_off.cpu().numpy(), tok_bytes.cpu().numpy(), pool.cpu().numpy()
    words, toks = sstate.tolist(), nxt.tolist()
    tabs: dict = {}
    # many rows in one word (a test's sweep over the vocabulary): one walk of every token
    import collections

    walked = {w: None for w, c in collections.Counter(words).items() if c > 8 and w != 0 and not J.is_done(w)}
    for r, (w, t) in enumerate(zip(words, toks)):
        if w == 0 or J.is_done(w) or t == eos_id or (valid is not None and int(valid[r]) == 0):
            continue
        if w in walked:
            if walked[w] is None:
                walked[w] = _schema_walk(w, len(off) - 1, off, data, J.pool_tables(pool_np, J.unpack(w)[2]),
                                         int(eos_id))[1]
            if 0 <= t < len(off) - 1:
                sstate[r] = int(walked[w][t])
            continue
        if not 0 <= t < len(off) - 1 or off[t + 1] == off[t]:
            continue
        st, ws, slot = J.unpack(w)
        if slot not in tabs:
            got = J.pool_tables(pool_np, slot)
            tabs[slot] = None if got is None else (got[0].tolist(), got[1].astype("int32").tolist())
        if tabs[slot] is None or st >= len(tabs[slot][1]):
            continue
        cls, trans = tabs[slot]
        nc = len(trans[0])
        for b in data[off[t]:off[t + 1]].tolist():
            c = cls[b]
            e = trans[st][c] if c < nc else 0
            if e == 0 or (e & J.NEXT_MASK) >= len(trans) or (e & J.WS_FLAG and ws >= J.WS_CAP):
                st = -1
                break
            st, ws = e & J.NEXT_MASK, (ws + 1 if e & J.WS_FLAG else 0)
        if st >= 0:
            sstate[r] = J.pack(st, ws, slot)


# ----------------------------------------------------------------------------- row compaction
def masked_scan(keep, w=None):
    """pos int64 [n+1]: exclusive prefix sum of ``keep[r] ? w[r] : 0`` (``w`` = 1 when None);
    ``pos[n]`` is the surviving total."""
    k = keep.reshape(-1) != 0
    v = k.to(torch.int64) if w is None else torch.where(k, w.reshape(-1).to(torch.int64), 0)
    pos = torch.zeros(k.numel() + 1, dtype=torch.int64, device=keep.device)
    if k.numel():
        pos[1:] = torch.cumsum(v, 0)
    return pos


def gather_rows(src, keep, pos, out):
    """``out[pos[r]] = src[r]`` for kept rows (boolean indexing: surviving rows keep their
    order); ``pos`` is only used for the count it implies."""
    rows = src[keep.reshape(-1) != 0]
    out[: rows.shape[0]] = rows[: out.shape[0]]
    return out


def csr_gather(row_ptr, keep, pos, epos, terms, tfs, n_out: int, e_out: int):
    """(row_ptr', terms', tfs') of the kept rows of a CSR."""
    k = keep.reshape(-1) != 0
    lens = row_ptr[1:] - row_ptr[:-1]
    new_ptr = torch.zeros(n_out + 1, dtype=torch.int64, device=row_ptr.device)
    new_ptr[1:] = torch.cumsum(lens[k], 0)[:n_out]
    emask = torch.repeat_interleave(k, lens)
    return new_ptr, terms[: emask.numel()][emask][:e_out].clone(), tfs[: emask.numel()][emask][:e_out].clone()


def remap_ids(ids, pos):
    """``pos[ids]``; ids outside ``[0, n)`` become -1."""
    n = pos.numel() - 1
    ok = (ids >= 0) & (ids < n)
    return torch.where(ok, pos[ids.clamp(0, max(n - 1, 0))], torch.full_like(ids, -1))
