"""The row-op oracle (tests/rowop_oracle.py) is sound and bites.  CPU only.

Sound: the fp32 reference of every op (docqa_amd.ops.reference) stays inside the bound with
the slack term quartered (2^-18 m for bf16 outputs, 2^-16 m for pool_l2), on the inputs the
GPU tests use at the small shapes.  If it did not, the oracle's ``m`` would be wrong.

Bites: faults planted into the reference's output, or into a copy of its arithmetic, are all
rejected.  Each fault test also records whether the suite's old rule,
``max|a - b| <= 2e-2 + 1e-2 max|b|``, accepts the same output (``OLD_RULE``; run with ``-s``
to see the table the last test prints).
"""
import pytest
import torch
import torch.nn.functional as F

from docqa_amd.ops import reference as R
from tests import rowop_oracle as O

Q_BF16 = O.SLACK_BF16 / 4
Q_F32 = O.SLACK_F32 / 4
EPS = 1e-5
LN_EPS = 1e-12

OLD_RULE: dict[str, bool] = {}


def _old_close(a, b, atol=2e-2, rtol=1e-2):
    a, b = a.float(), b.float()
    return bool((a - b).abs().max() <= atol + rtol * b.abs().max())


def _rejected(name, got, ref, y, m, **kw):
    """The oracle must reject ``got``; note whether the old rule accepts it against ``ref``."""
    with pytest.raises(AssertionError, match="outside the bound"):
        O.assert_oracle(got, y, m, what=name, **kw)
    OLD_RULE[name] = _old_close(got, ref)


# ----------------------------------------------------------------------------- the rule
def test_ulp_bf16():
    v = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0, 2.0 ** -126, 2.0 ** -130, 255.0, 0.75], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133,
                         1.0, 2.0 ** -8], dtype=torch.float64)
    assert torch.equal(O.ulp_bf16(v), want)
    # the spacing of bf16 itself
    b = torch.tensor([1.0, 2.0, 100.0, 0.3], dtype=torch.bfloat16)
    nxt = (O.bits(b) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - b.double()), O.ulp_bf16(b.double()))


def test_message_names_the_element():
    y = torch.zeros(3, 16, dtype=torch.float64) + 1.0
    got = torch.ones(3, 16).bfloat16()
    got[2, 5] = 1.0 + 2.0 ** -6
    with pytest.raises(AssertionError, match=r"row 2, col 5.*got 1\.015625.*want 1\.0.*2\.000 ulp"):
        O.assert_oracle(got, y, y.abs(), what="demo")
    got[2, 5] = float("nan")
    with pytest.raises(AssertionError, match="row 2, col 5"):
        O.assert_oracle(got, y, y.abs(), what="demo")


# ----------------------------------------------------------------------------- soundness
@pytest.mark.parametrize("rows,H", O.SMALL_RMS)
def test_reference_rmsnorm(rows, H):
    x, r, w = O.rms_case(rows, H)
    O.assert_oracle(R.rmsnorm(x, w, EPS), *O.rmsnorm(x, w, EPS), slack=Q_BF16, what="rmsnorm")
    res = r.clone()
    out = R.add_rmsnorm(x, res, w, EPS)
    (s, ms), _ = O.add_rmsnorm(x, r, w, EPS)
    O.assert_oracle(res, s, ms, slack=Q_BF16, what="add_rmsnorm residual")
    O.assert_oracle(out, *O.rmsnorm(res, w, EPS), slack=Q_BF16, what="add_rmsnorm out")
    z = O.zero_row(rows)
    if z is not None:
        assert not out[z].any() and not res[z].any()


@pytest.mark.parametrize("rows,H", O.SMALL_LN)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("offset", [False, True])
def test_reference_layernorm(rows, H, res, offset):
    x, r, g, b = O.ln_case(rows, H, res, "offset" if offset else "scaled")
    O.assert_oracle(R.layernorm(x, r, g, b, LN_EPS), *O.layernorm(x, r, g, b, LN_EPS), slack=Q_BF16,
                    what="layernorm")


@pytest.mark.parametrize("T,H", O.SMALL_BERT)
@pytest.mark.parametrize("tt", [False, True])
def test_reference_bert_embed_ln(T, H, tt):
    c = O.bert_case(T, H, tt)
    O.assert_oracle(R.bert_embed_ln(**c, eps=LN_EPS), *O.bert_embed_ln(**c, eps=LN_EPS), slack=Q_BF16,
                    what="bert_embed_ln")


@pytest.mark.parametrize("T,I", O.SMALL_ACT)
@pytest.mark.parametrize("il", [False, True])
def test_reference_silu_mul(T, I, il):
    gu = O.silu_case(T, I, il)
    O.assert_oracle(R.silu_mul(gu, il), *O.silu_mul(gu, il), slack=Q_BF16, what="silu_mul")


@pytest.mark.parametrize("T,N", O.SMALL_ACT)
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("res", [False, True])
def test_reference_bias_act(T, N, gelu, res):
    x, b, r = O.bias_case(T, N)
    r = r if res else None
    O.assert_oracle(R.bias_act(x, b, r, gelu), *O.bias_act(x, b, r, gelu), slack=Q_BF16, what="bias_act")


def _run_rope(c, Hq, Hkv, D, BS, slots="given"):
    sl = c["slots"] if slots == "given" else slots
    kc, vc = O.sentinel_cache(c["nb"], Hkv, BS, D, "cpu"), O.sentinel_cache(c["nb"], Hkv, BS, D, "cpu")
    q = c["qkv"].clone()
    R.rope_cache(q, c["pos"], c["cos_sin"], sl, kc, vc, Hq, Hkv, D)
    return q, kc, vc


@pytest.mark.parametrize("Hq,Hkv,D,T,BS", O.SMALL_ROPE)
def test_reference_rope_cache(Hq, Hkv, D, T, BS):
    c = O.rope_case(Hq, Hkv, D, T, BS)
    q, kc, vc = _run_rope(c, Hq, Hkv, D, BS)
    qk = (Hq + Hkv) * D
    O.assert_oracle(q[:, :qk], *O.rope(c["qkv"], c["pos"], c["cos_sin"], Hq, Hkv, D), slack=Q_BF16, what="rope")
    O.check_rope_cache(c["qkv"], q, c["pos"], c["slots"], c["cos_sin"], kc, vc, Hq, Hkv, D)
    q, kc, vc = _run_rope(c, Hq, Hkv, D, BS, slots=None)
    O.check_rope_cache(c["qkv"], q, c["pos"], None, c["cos_sin"], kc, vc, Hq, Hkv, D)


@pytest.mark.parametrize("H", O.SMALL_POOL)
@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("normalize", [True, False])
def test_reference_pool_l2(H, mean, normalize):
    h, cu = O.pool_case(H)
    got = R.pool_l2(h, cu, mean, normalize)
    O.assert_oracle(got, *O.pool_l2(h, cu, mean, normalize), slack=Q_F32, what="pool_l2")
    assert not got[O.POOL_LENS.index(0)].any()


# ----------------------------------------------------------------------------- planted faults
def _rms_case(rows=5, H=4096):
    x, w = O.make_rows(rows, H, 21), O.make_weight(H, 22)
    return x, w, R.rmsnorm(x, w, EPS), O.rmsnorm(x, w, EPS)


def test_fault_weight_chunk_shifted():
    """weight chunk c applied to chunk c + 1 on the last chunk pair of one row"""
    x, w, ref, (y, m) = _rms_case()
    wf = w.clone()
    wf[-8:] = w[-16:-8]
    got = ref.clone()
    got[3] = R.rmsnorm(x[3:4], wf, EPS)[0]
    _rejected("weight chunk c applied to chunk c+1", got, ref, y, m)


def test_fault_chunk_missing_from_sum_of_squares():
    """one 8-element chunk of 512 left out of one row's sum of squares at H = 4096"""
    x, w, ref, (y, m) = _rms_case()
    xf = x[3].float()
    ss = xf.pow(2).sum() - xf[1000:1008].pow(2).sum()
    got = ref.clone()
    got[3] = (xf * torch.rsqrt(ss / 4096 + EPS) * w.float()).bfloat16()
    _rejected("one chunk missing from the sum of squares", got, ref, y, m)


def test_fault_neighbour_inv():
    """inv of row r + 1 used for row r: on the scaled rows, and on plain randn rows of similar
    scale (what the old tests fed the kernel)"""
    x, w, ref, (y, m) = _rms_case()
    inv = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS)
    got = ref.clone()
    got[3] = (x[3].float() * inv[4] * w.float()).bfloat16()
    _rejected("inv of row r+1 (rows scaled 2x apart)", got, ref, y, m)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(5, 4096, generator=gen).bfloat16()
    w = (torch.rand(4096, generator=gen) + 0.5).bfloat16()
    ref, (y, m) = R.rmsnorm(x, w, EPS), O.rmsnorm(x, w, EPS)
    inv = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS)
    got = ref.clone()
    got[3] = (x[3].float() * inv[4] * w.float()).bfloat16()
    _rejected("inv of row r+1 (randn rows, weights in [0.5, 1.5])", got, ref, y, m)


def test_fault_one_pass_variance():
    """LayerNorm variance as E[x^2] - mean^2 in fp32 on the offset rows"""
    H = 768
    x, g, b = O.make_offset_rows(4, H, 24), O.make_weight(H, 25), O.make_weight(H, 26)
    ref, (y, m) = R.layernorm(x, None, g, b, LN_EPS), O.layernorm(x, None, g, b, LN_EPS)
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = (xf * xf).mean(-1, keepdim=True) - mean * mean
    got = ((xf - mean) * torch.rsqrt(var.clamp_min(0) + LN_EPS) * g.float() + b.float()).bfloat16()
    _rejected("one-pass variance on offset rows", got, ref, y, m)


def _rope_case():
    Hq, Hkv, D, T, BS = 8, 2, 128, 50, 16
    c = O.make_rope(Hq, Hkv, D, T, BS, 27)
    q, kc, vc = _run_rope(c, Hq, Hkv, D, BS)
    return c, q, kc, vc, (Hq, Hkv, D, BS)


def _rope_rejected(name, c, q, kc, vc, dims, ref):
    Hq, Hkv, D, BS = dims
    with pytest.raises(AssertionError):
        O.check_rope_cache(c["qkv"], q, c["pos"], c["slots"], c["cos_sin"], kc, vc, Hq, Hkv, D)
    rq, rkc, rvc = ref
    # the old test: zero-initialised caches, so the sentinel reads as the zero it would have been
    z = lambda t: torch.where(O.bits(t) == O.SENTINEL_BITS, torch.zeros_like(t), t)
    OLD_RULE[name] = _old_close(q, rq) and _old_close(z(kc), z(rkc)) and _old_close(z(vc), z(rvc), 0.0, 0.0)


def _flip_sine(c, q, D, t, h, i):
    cs = c["cos_sin"][c["pos"][t].long()]
    x1, x2 = c["qkv"][t, h * D + i].float(), c["qkv"][t, h * D + D // 2 + i].float()
    bad = q.clone()
    bad[t, h * D + i] = (x1 * cs[i] + x2 * cs[D // 2 + i]).bfloat16()
    bad[t, h * D + D // 2 + i] = (x2 * cs[i] - x1 * cs[D // 2 + i]).bfloat16()
    return bad


def test_fault_sine_sign_on_one_pair():
    """sine sign flipped on one rotation pair of one Q head: an ordinary pair, and a small one
    (a row scaled by 1/4, frequency 56 of 64: an angle of a few 1e-3 rad)"""
    c, q, kc, vc, dims = _rope_case()
    D = dims[2]
    bad = _flip_sine(c, q, D, 7, 3, 5)
    _rope_rejected("sine sign flipped on one rotation pair", c, bad, kc, vc, dims, (q, kc, vc))
    quarter = torch.arange(5, c["pos"].numel(), 5)          # rows scaled by 2^-2, position > 0
    t = int(quarter[c["pos"][quarter].argmax()])
    bad = _flip_sine(c, q, D, t, 3, 56)
    _rope_rejected("sine sign flipped on a small rotation pair", c, bad, kc, vc, dims, (q, kc, vc))


def test_fault_adjacent_pairing():
    """rotation pairs (i, i + 1) instead of (i, i + D/2)"""
    c, q, kc, vc, dims = _rope_case()
    Hq, Hkv, D, BS = dims
    T, half = c["qkv"].shape[0], D // 2
    x = c["qkv"].float().view(T, Hq + 2 * Hkv, D)[:, : Hq + Hkv]
    cs = c["cos_sin"][c["pos"].long()]
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    x1, x2 = x[..., 0::2], x[..., 1::2]
    rot = torch.stack([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1).flatten(-2)
    bad = q.clone()
    bad.view(T, Hq + 2 * Hkv, D)[:, : Hq + Hkv] = rot.bfloat16()
    _rope_rejected("rotation pairing (i, i+1)", c, bad, kc, vc, dims, (q, kc, vc))


def test_fault_k_slot_off_by_one():
    """K written at slot off + 1 (V at the right slot)"""
    c, q, kc, vc, dims = _rope_case()
    Hq, Hkv, D, BS = dims
    nslots = c["nb"] * BS
    shifted = torch.where(c["slots"] >= 0, (c["slots"] + 1) % nslots, c["slots"])
    _, kc_bad, _ = _run_rope(c, Hq, Hkv, D, BS, slots=shifted)
    _rope_rejected("K written at slot off+1", c, q, kc_bad, vc, dims, (q, kc, vc))


def test_fault_padding_slot_written():
    """a -1 slot written into block 0 (C division: -1 / BS == 0)"""
    c, q, kc, vc, dims = _rope_case()
    Hq, Hkv, D, BS = dims
    t = int((c["slots"] < 0).nonzero()[0])
    kv = q[t, Hq * D:].view(2 * Hkv, D)
    kc_bad, vc_bad = kc.clone(), vc.clone()
    kc_bad[0, :, BS - 1] = kv[:Hkv]
    vc_bad[0, :, BS - 1] = kv[Hkv:]
    _rope_rejected("-1 slot written to block 0", c, q, kc_bad, vc_bad, dims, (q, kc, vc))


def test_fault_silu_halves_swapped():
    """gate and up halves swapped for one 8-chunk"""
    T, I = 19, 1536
    gu = O.make_gate_up(T, I, 28)
    ref, (y, m) = R.silu_mul(gu), O.silu_mul(gu)
    g, u = gu.float().chunk(2, -1)
    got = ref.clone()
    got[5, 64:72] = (F.silu(u[5, 64:72]) * g[5, 64:72]).bfloat16()
    _rejected("silu gate / up swapped for one chunk", got, ref, y, m)


def test_fault_silu_overflowed_exp():
    """silu(x) as x / (1 + exp(-x)) in fp32 for every x: exp(-x) is inf below -88.7 and the
    quotient -0, while silu(x) * u is still a normal bf16 value (what act.hip and the reference
    computed before they took x * e^x there)"""
    T, I = 19, 1536
    gu = O.make_gate_up(T, I, 28)
    ref, (y, m) = R.silu_mul(gu), O.silu_mul(gu)
    g, u = gu.float().chunk(2, -1)
    got = (g / (1.0 + torch.exp(-g)) * u).bfloat16()
    _rejected("silu as x / (1 + exp(-x)) below -88.7", got, ref, y, m)


def test_fault_interleaved_read_as_plain():
    T, I = 19, 1536
    gu = O.make_gate_up(T, I, 29, interleaved=True)
    ref, (y, m) = R.silu_mul(gu, True), O.silu_mul(gu, True)
    _rejected("interleaved layout read as plain", R.silu_mul(gu, False), ref, y, m)


def test_fault_truncation_on_pack():
    """truncation instead of round-to-nearest-even when packing to bf16"""
    x, w, ref, (y, m) = _rms_case()
    f = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS) * w.float()
    got = (f.view(torch.int32) & -65536).view(torch.float32).bfloat16()
    _rejected("truncation instead of round-to-nearest", got, ref, y, m)


def test_fault_mean_pool_divisor():
    """mean pool divided by L + 1 (normalize off: the L2 norm would cancel it)"""
    h, cu = O.make_pool(384, 30)
    ref, (y, m) = R.pool_l2(h, cu, True, False), O.pool_l2(h, cu, True, False)
    lens = torch.tensor(O.POOL_LENS, dtype=torch.float32)[:, None]
    got = ref * lens / (lens + 1)
    _rejected("mean pool divided by L+1", got, ref, y, m)
    # at L = 512 alone the factor is 1 - 1/513: 2e-3 relative, far under the old tolerance
    b = O.POOL_LENS.index(512)
    with pytest.raises(AssertionError, match="outside the bound"):
        O.assert_oracle(got[b:b + 1], y[b:b + 1], m[b:b + 1], what="L = 512")
    OLD_RULE["mean pool divided by L+1 (L = 512 row)"] = _old_close(got[b:b + 1], ref[b:b + 1])


def test_old_rule_table():
    """Every fault above is rejected by the oracle; print what the old rule makes of them."""
    for name, fn in sorted(globals().items()):
        if name.startswith("test_fault_"):
            fn()
    assert len(OLD_RULE) >= 12
    for name, accepted in OLD_RULE.items():
        print(f"{'old rule ACCEPTS' if accepted else 'old rule rejects'} : {name}")
