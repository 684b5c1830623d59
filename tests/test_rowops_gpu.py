"""Row-wise and element-wise kernels against the per-element fp64 oracle (tests/rowop_oracle.py),
on every launch path, at the smallest shape that reaches it.  GPU only; the native extension
must be loaded (no silent fallback).  Tolerances are the derived ones of the oracle module.

Case -> template instantiation (names as in the launchers):

launch_rms (norm.hip), ADD = false for rmsnorm / true for add_rmsnorm, every case runs both:
  row-{1,3,2048}x1024, x2048          rmsnorm_row_kernel<1>   (1024: half the threads idle)
  row-*x2056, x4096                   rmsnorm_row_kernel<2>   (2056: one spill chunk)
  row-*x4104, x8192                   rmsnorm_row_kernel<4>   (4104: one spill chunk)
  wave-{1,3,5,8}x{8,384,512}          rmsnorm_kernel<1>       (rows 1,3,5: dead waves in the tail)
  wave-*x{520,1016}                   rmsnorm_kernel<2>
  wave-2049x1024                      rmsnorm_kernel<2>       (last workgroup: one live wave)
  wave-2049x2048 / x4096 / x8192      rmsnorm_kernel<4> / <8> / <16>
add_rmsnorm_splitk (fp32 and bf16 slabs): H 1024 / 4096 / 8192 -> NV 1 / 2 / 4;
  S 1, 2, 8 -> NS = S, S 9 -> NS = 0 (runtime slab count)
docqa_layernorm, ADD = residual given:
  H 8, 384, 512 -> layernorm_kernel<1>; 520, 768, 1024 -> <2>; 2048 -> <4>; 4096 -> <8>
docqa_bert_embed_ln: H 384 -> bert_embed_ln_kernel<1>; 768, 1024 -> <2>; 2048 -> <4>
docqa_embed_rmsnorm: H 256, 1024 -> embed_rmsnorm_kernel<1>; 2056 -> <2>; 4104, 8192 -> <4>
docqa_embedding: H 8, 384 one trip of the gather loop; 4096, 8192 a second trip
docqa_silu_mul: plain -> silu_mul_kernel<false>, interleaved -> <true>; (300, 14336) grid-strides
docqa_bias_act: gelu x residual -> bias_act_kernel<G, R>, all four; (2731, 1536) grid-strides
docqa_rope_cache: rope_cache_kernel<false, 0, float>; D 128 / 64 / 32 -> 16 / 32 / 64 heads per
  workgroup; (14, 2, 128) and (32, 8, 64) have a ragged second head block, (32, 8, 128) is
  three full ones, (8, 2, 128) and (4, 4, 32) one partly filled block
rope_cache_splitk: rope_cache_kernel<true, NS, float | uint16_t>, NS as above
docqa_pool_l2: mean -> pool_l2_kernel<true>, CLS -> <false>; H 384: second wave idle, 1024: limit
"""
import pytest
import torch

from tests import rowop_oracle as O

pytestmark = pytest.mark.gpu

EPS = 1e-5
LN_EPS = 1e-12
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops.native_loaded()
    torch.manual_seed(0)
    return torch.ops.docqa


def _unchanged(t, t0, what):
    assert torch.equal(O.bits(t), O.bits(t0)), f"{what} was modified"


# ----------------------------------------------------------------------------- rmsnorm
_RMS = ([("row", r, h) for r in (1, 3, 2048) for h in (1024, 2048, 2056, 4096, 4104, 8192)]
        + [("wave", r, h) for r in (1, 3, 5, 8) for h in (8, 384, 512, 520, 1016)]
        + [("wave", 2049, h) for h in (1024, 2048, 4096, 8192)])


def _check_rms(C, x, r, w, add):
    x0 = x.clone()
    if add:
        res = r.clone()
        out = C.add_rmsnorm(x, res, w, EPS)
        (s, ms), _ = O.add_rmsnorm(x, r, w, EPS)
        O.assert_oracle(res, s, ms, what="add_rmsnorm residual")
        O.assert_oracle(out, *O.rmsnorm(res, w, EPS), what="add_rmsnorm out")    # of the kernel's residual
    else:
        out = C.rmsnorm(x, w, EPS)
        O.assert_oracle(out, *O.rmsnorm(x, w, EPS), what="rmsnorm")
    _unchanged(x, x0, "x")
    z = O.zero_row(x.shape[0])
    if z is not None:
        assert not out[z].any(), "all-zero row must give zeros"
    return out


@pytest.mark.parametrize("add", [False, True], ids=["rmsnorm", "add_rmsnorm"])
@pytest.mark.parametrize("path,rows,H", _RMS, ids=[f"{p}-{r}x{h}" for p, r, h in _RMS])
def test_rmsnorm_paths(native, path, rows, H, add):
    assert (path == "row") == (rows <= 2048 and H >= 1024)      # the dispatch rule of launch_rms
    x, r, w = O.rms_case(rows, H, DEV)
    _check_rms(native, x, r, w, add)


@pytest.mark.parametrize("add", [False, True], ids=["rmsnorm", "add_rmsnorm"])
def test_rmsnorm_dispatch_seam(native, add):
    """2048 rows take the row kernel, 2049 the wave kernel: identical leading rows, both inside
    the bound."""
    H = 1024
    x, r, w = O.rms_case(2049, H, DEV)
    _check_rms(native, x, r, w, add)
    _check_rms(native, x[:2048].contiguous(), r[:2048].contiguous(), w, add)


def test_rmsnorm_refusals(native):
    for H in (8200, 12):
        x, w = O.make_rows(3, H, 4, DEV), O.make_weight(H, 5, DEV)
        with pytest.raises(RuntimeError):
            native.rmsnorm(x, w, EPS)
        with pytest.raises(RuntimeError):
            native.add_rmsnorm(x, x.clone(), w, EPS)
    x, w = O.make_rows(3, 1024, 4, DEV), O.make_weight(1024, 5, DEV)
    with pytest.raises(RuntimeError):
        native.add_rmsnorm(x, x.clone(), w[:512], EPS)                   # weight of the wrong size
    with pytest.raises(RuntimeError):
        native.add_rmsnorm(x, x.clone(), O.make_weight(2048, 5, DEV)[::2], EPS)   # strided weight
    e = torch.empty(0, 1024, device=DEV, dtype=torch.bfloat16)
    assert native.rmsnorm(e, w, EPS).shape == (0, 1024)
    assert native.add_rmsnorm(e, e.clone(), w, EPS).shape == (0, 1024)


# ----------------------------------------------------------------------------- split-K consumers
def _slab_sum(P):
    """x = P[0]; x = x + P[s] sequentially in fp32, in slab order; rounded to bf16."""
    x = P[0].float()
    for s in range(1, P.shape[0]):
        x = x + P[s].float()
    return x.bfloat16()


def _slabs(S, M, W, seed, dtype):
    P = torch.randn(S, M, W, generator=torch.Generator().manual_seed(seed)) / S ** 0.5
    return P.to(dtype).to(DEV)


@pytest.mark.parametrize("slab", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [1024, 4096, 8192])
@pytest.mark.parametrize("M", [1, 70])
@pytest.mark.parametrize("S", [1, 2, 8, 9])
def test_add_rmsnorm_splitk_bit_exact(native, S, M, H, slab):
    """The kernel's claim: the fused consumer equals projection -> bf16 -> add_rmsnorm bit for
    bit (both on the 256-thread row map: rows <= 2048, H >= 1024)."""
    P = _slabs(S, M, H, S * 1000 + M + H, slab)
    r, w = O.make_rows(M, H, 7, DEV), O.make_weight(H, 8, DEV)
    r1, r2 = r.clone(), r.clone()
    o1 = native.add_rmsnorm_splitk(P, r1, w, EPS)
    o2 = native.add_rmsnorm(_slab_sum(P), r2, w, EPS)
    assert torch.equal(O.bits(r1), O.bits(r2)), "residual differs from the unfused path"
    assert torch.equal(O.bits(o1), O.bits(o2)), "output differs from the unfused path"


def _rope_caches(c, Hkv, BS, D):
    return O.sentinel_cache(c["nb"], Hkv, BS, D, DEV), O.sentinel_cache(c["nb"], Hkv, BS, D, DEV)


@pytest.mark.parametrize("slab", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Hq,Hkv,D", [(14, 2, 128), (32, 8, 64)])
@pytest.mark.parametrize("M", [1, 70])
@pytest.mark.parametrize("S", [1, 2, 8, 9])
def test_rope_cache_splitk_bit_exact(native, S, M, Hq, Hkv, D, slab):
    BS = 16
    c = O.make_rope(Hq, Hkv, D, M, BS, 9, DEV)
    P = _slabs(S, M, (Hq + 2 * Hkv) * D, S * 1000 + M + D, slab)
    kc1, vc1 = _rope_caches(c, Hkv, BS, D)
    kc2, vc2 = _rope_caches(c, Hkv, BS, D)
    q1 = native.rope_cache_splitk(P, c["pos"], c["cos_sin"], c["slots"], kc1, vc1, Hq, Hkv, D)
    q2 = _slab_sum(P)
    native.rope_cache(q2, c["pos"], c["cos_sin"], c["slots"], kc2, vc2, Hq, Hkv, D)
    assert torch.equal(O.bits(q1), O.bits(q2)), "qkv differs from the unfused path"
    assert torch.equal(O.bits(kc1), O.bits(kc2)) and torch.equal(O.bits(vc1), O.bits(vc2))


def test_splitk_consumers_oracle(native):
    """The fused consumers against fp64 directly.  The slack is widened by S 2^-24 sum_s |P_s|
    (the fp32 slab sum) plus one bf16 ulp of the summed input (its rounding before the op),
    carried through the op."""
    S, M, H = 8, 70, 4096
    P = _slabs(S, M, H, 11, torch.float32)
    r, w = O.make_rows(M, H, 12, DEV), O.make_weight(H, 13, DEV)
    Pd = P.double()
    x, ax = Pd.sum(0), Pd.abs().sum(0)
    dx = S * 2.0 ** -24 * ax + O.ulp_bf16(x)
    res = r.clone()
    out = native.add_rmsnorm_splitk(P, res, w, EPS)
    O.assert_oracle(res, x + r.double(), ax + r.double().abs(), extra=dx, what="add_rmsnorm_splitk residual")
    O.assert_oracle(out, *O.rmsnorm(res, w, EPS), what="add_rmsnorm_splitk out")
    Hq, Hkv, D, BS = 14, 2, 128, 16
    c = O.make_rope(Hq, Hkv, D, M, BS, 14, DEV)
    W = (Hq + 2 * Hkv) * D
    P = _slabs(S, M, W, 15, torch.float32)
    Pd = P.double()
    x, ax = Pd.sum(0), Pd.abs().sum(0)
    dx = (S * 2.0 ** -24 * ax + O.ulp_bf16(x)).view(M, Hq + 2 * Hkv, D)[:, : Hq + Hkv]
    cs = c["cos_sin"].double()[c["pos"].long()].abs()
    ca, sa = cs[:, None, : D // 2], cs[:, None, D // 2:]
    d1, d2 = dx[..., : D // 2], dx[..., D // 2:]
    extra = torch.cat([d1 * ca + d2 * sa, d2 * ca + d1 * sa], -1).reshape(M, -1)
    kc, vc = _rope_caches(c, Hkv, BS, D)
    q = native.rope_cache_splitk(P, c["pos"], c["cos_sin"], c["slots"], kc, vc, Hq, Hkv, D)
    y, m = O.rope(x, c["pos"], c["cos_sin"], Hq, Hkv, D)
    O.assert_oracle(q[:, : (Hq + Hkv) * D], y, m, extra=extra, what="rope_cache_splitk q/k")
    vx = x[:, (Hq + Hkv) * D:]
    O.assert_oracle(q[:, (Hq + Hkv) * D:], vx, ax[:, (Hq + Hkv) * D:], slack=S * 2.0 ** -24, what="splitk v")


# ----------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize("kind", ["scaled", "offset"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("H", [8, 384, 512, 520, 768, 1024, 2048, 4096])
@pytest.mark.parametrize("rows", [1, 3, 77])
def test_layernorm(native, rows, H, res, kind):
    x, r, g, b = O.ln_case(rows, H, res, kind, DEV)   # offset: x = 1024 + 4 k, no one-pass variance passes
    x0 = x.clone()
    out = native.layernorm(x, r, g, b, LN_EPS)
    O.assert_oracle(out, *O.layernorm(x, r, g, b, LN_EPS), what="layernorm")
    _unchanged(x, x0, "x")
    z = O.zero_row(rows)
    if kind == "scaled" and z is not None:
        assert torch.equal(O.bits(out[z]), O.bits(b)), "all-zero row must give beta exactly"


def test_layernorm_refusals(native):
    H = 4104
    x, g = O.make_rows(3, H, 24, DEV), O.make_weight(H, 25, DEV)
    with pytest.raises(RuntimeError):
        native.layernorm(x, None, g, g, LN_EPS)
    x, g = O.make_rows(3, 768, 24, DEV), O.make_weight(768, 25, DEV)
    with pytest.raises(RuntimeError):
        native.layernorm(x, None, g[:384], g, LN_EPS)
    with pytest.raises(RuntimeError):
        native.layernorm(x, None, g, g[:384], LN_EPS)
    with pytest.raises(RuntimeError):
        native.layernorm(x, None, O.make_weight(1536, 25, DEV)[::2], g, LN_EPS)


# ----------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("tt", [False, True], ids=["notype", "type"])
@pytest.mark.parametrize("H", [384, 768, 1024, 2048])
@pytest.mark.parametrize("T", [1, 3, 99])
def test_bert_embed_ln(native, T, H, tt):
    c = O.bert_case(T, H, tt, DEV)
    out = native.bert_embed_ln(*c.values(), LN_EPS)
    O.assert_oracle(out, *O.bert_embed_ln(**c, eps=LN_EPS), what="bert_embed_ln")


def test_bert_embed_ln_out_of_range_and_refusals(native):
    """Out-of-range token / position / type indices read row 0 (like embedding_gather_kernel)."""
    H, V, NP, NT = 384, 300, 64, 2
    c = O.make_bert(8, H, 31, True, DEV, V=V, NP=NP, NT=NT)
    big = 2 ** 31 - 1
    c["ids"] = torch.tensor([0, V - 1, -1, V, big, 5, 6, 7], dtype=torch.int32, device=DEV)
    c["pos"] = torch.tensor([NP - 1, 0, 1, 2, 3, -1, NP, big], dtype=torch.int32, device=DEV)
    c["token_type"] = torch.tensor([0, 1, -1, NT, big, 1, 0, 1], dtype=torch.int32, device=DEV)
    out = native.bert_embed_ln(*c.values(), LN_EPS)
    O.assert_oracle(out, *O.bert_embed_ln(**c, eps=LN_EPS), what="bert_embed_ln out-of-range")
    ok = dict(c)
    for k, n in (("ids", V), ("pos", NP), ("token_type", NT)):
        ok[k] = torch.where((c[k] >= 0) & (c[k] < n), c[k], torch.zeros_like(c[k]))
    assert torch.equal(O.bits(out), O.bits(native.bert_embed_ln(*ok.values(), LN_EPS)))

    def refused(**kw):
        with pytest.raises(RuntimeError):
            native.bert_embed_ln(*{**ok, **kw}.values(), LN_EPS)

    c2 = O.make_bert(8, 2056, 32, False, DEV)
    with pytest.raises(RuntimeError):
        native.bert_embed_ln(*c2.values(), LN_EPS)                  # H = 2056: no instantiation
    wide = O.make_rows(NP, 2 * H, 33, DEV)
    refused(wpe=wide)                                               # H columns
    refused(wpe=wide[:, :H])                                        # contiguity
    refused(wtt=wide[:NT])
    refused(gamma=ok["gamma"][:H - 8])
    refused(beta=ok["beta"][:H - 8])
    refused(pos=ok["pos"][:4])
    refused(token_type=ok["token_type"][:4])


@pytest.mark.parametrize("H", [8, 384, 4096, 8192])
def test_embedding_gather(native, H):
    V = 50
    table = O.make_rows(V, H, 40 + H, DEV)
    ids = torch.tensor([0, V - 1, -1, V, 2 ** 31 - 1, 17], dtype=torch.int32, device=DEV)
    got = native.embedding(ids, table)
    assert torch.equal(O.bits(got), O.bits(O.embedding(ids, table)))
    assert torch.equal(O.bits(got[2:5]), O.bits(table[:1].expand(3, H))), "out-of-range ids read row 0"


@pytest.mark.parametrize("H", [256, 1024, 2056, 4104, 8192])
def test_embed_rmsnorm(native, H):
    V = 50
    table, w = O.make_rows(V, H, 41 + H, DEV), O.make_weight(H, 42 + H, DEV)
    ids = torch.tensor([0, V - 1, -1, V, 2 ** 31 - 1, 17, 1], dtype=torch.int32, device=DEV)   # row 1: zeros
    h, x = native.embed_rmsnorm(ids, table, w, EPS)
    assert torch.equal(O.bits(h), O.bits(O.embedding(ids, table))), "h must be the gather, bit for bit"
    O.assert_oracle(x, *O.rmsnorm(h, w, EPS), what="embed_rmsnorm x")
    assert not x[6].any()


def test_embed_rmsnorm_refusals(native):
    H = 8200
    table, w = O.make_rows(4, H, 43, DEV), O.make_weight(H, 44, DEV)
    with pytest.raises(RuntimeError):
        native.embed_rmsnorm(torch.zeros(2, dtype=torch.int32, device=DEV), table, w, EPS)


# ----------------------------------------------------------------------------- activations
@pytest.mark.parametrize("il", [False, True], ids=["plain", "interleaved"])
@pytest.mark.parametrize("T,I", [(1, 8), (19, 1536), (300, 14336)])
def test_silu_mul(native, T, I, il):
    """(300, 14336) is 537,600 chunks: past the 524,288-chunk grid cap, the grid-stride loop takes
    a second trip.  Gates reach below -88.7, where exp(-x) overflows in fp32."""
    gu = O.silu_case(T, I, il, DEV)
    gu0 = gu.clone()
    out = native.silu_mul(gu, il)
    O.assert_oracle(out, *O.silu_mul(gu, il), what="silu_mul")
    _unchanged(gu, gu0, "gate|up")


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("gelu", [False, True], ids=["bias", "gelu"])
@pytest.mark.parametrize("T,N", [(1, 8), (19, 1536), (2731, 1536)])
def test_bias_act(native, T, N, gelu, res):
    """(2731, 1536) is 524,352 chunks: the grid-stride loop's second trip."""
    x, b, r = O.bias_case(T, N, DEV)
    r = r if res else None
    out = native.bias_act(x, b, r, gelu)
    O.assert_oracle(out, *O.bias_act(x, b, r, gelu), what="bias_act")


def test_bias_act_refusals(native):
    x, b, r = O.make_bias_act(19, 1536, 61, DEV)
    with pytest.raises(RuntimeError):
        native.bias_act(x, b, r[:10], False)                         # residual of the wrong size
    with pytest.raises(RuntimeError):
        native.bias_act(x, O.make_weight(3072, 62, DEV)[::2], None, False)   # strided bias


# ----------------------------------------------------------------------------- rope + cache
_ROPE = [(8, 2, 128), (14, 2, 128), (32, 8, 128), (32, 8, 64), (4, 4, 32)]


@pytest.mark.parametrize("BS", [16, 32])
@pytest.mark.parametrize("T", [1, 50])
@pytest.mark.parametrize("Hq,Hkv,D", _ROPE, ids=[f"{a}-{b}-{d}" for a, b, d in _ROPE])
def test_rope_cache(native, Hq, Hkv, D, T, BS):
    c = O.rope_case(Hq, Hkv, D, T, BS, DEV)
    kc, vc = _rope_caches(c, Hkv, BS, D)
    q = c["qkv"].clone()
    native.rope_cache(q, c["pos"], c["cos_sin"], c["slots"], kc, vc, Hq, Hkv, D)
    O.check_rope_cache(c["qkv"], q, c["pos"], c["slots"], c["cos_sin"], kc, vc, Hq, Hkv, D)
    # slot_mapping None: nothing but the Q/K columns of qkv changes (the caches are not even read)
    kn, vn = _rope_caches(c, Hkv, BS, D)
    qn = c["qkv"].clone()
    native.rope_cache(qn, c["pos"], c["cos_sin"], None, kn, vn, Hq, Hkv, D)
    O.check_rope_cache(c["qkv"], qn, c["pos"], None, c["cos_sin"], kn, vn, Hq, Hkv, D)
    assert torch.equal(O.bits(qn), O.bits(q))
    # qkv as a column slice of a wider sentinel-filled buffer: same bits, padding untouched
    W, pad = q.shape[1], 24
    wide = torch.full((T, pad + W + 8), O.SENTINEL_BITS, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    qs = wide[:, pad:pad + W]
    qs.copy_(c["qkv"])
    ks, vs = _rope_caches(c, Hkv, BS, D)
    native.rope_cache(qs, c["pos"], c["cos_sin"], c["slots"], ks, vs, Hq, Hkv, D)
    assert torch.equal(O.bits(qs), O.bits(q)), "strided qkv differs from the contiguous run"
    assert torch.equal(O.bits(ks), O.bits(kc)) and torch.equal(O.bits(vs), O.bits(vc))
    wb = O.bits(wide)
    assert bool((wb[:, :pad] == O.SENTINEL_BITS).all()) and bool((wb[:, pad + W:] == O.SENTINEL_BITS).all()), \
        "padding columns next to a strided qkv were written"


def test_rope_cache_refusals(native):
    Hq, Hkv, D, T, BS = 8, 2, 128, 50, 16
    c = O.make_rope(Hq, Hkv, D, T, BS, 71, DEV)
    kc, vc = _rope_caches(c, Hkv, BS, D)
    W = c["qkv"].shape[1]

    def refused(qkv=None, pos=c["pos"], slots=c["slots"], k=kc, v=vc):
        with pytest.raises(RuntimeError):
            native.rope_cache(c["qkv"].clone() if qkv is None else qkv, pos, c["cos_sin"], slots, k, v, Hq, Hkv, D)

    wide = torch.zeros(T, W + 12, device=DEV, dtype=torch.bfloat16)
    refused(qkv=wide[:, :W])                                       # row stride not a multiple of 8
    refused(qkv=torch.zeros(2 * T, W, device=DEV, dtype=torch.bfloat16)[::2].unflatten(0, (5, 10)))   # 3-D strided
    refused(pos=c["pos"][: T - 1])
    refused(slots=c["slots"][: T - 1])
    refused(pos=torch.cat([c["pos"], c["pos"]])[::2])
    refused(k=kc[:, :, :, : D // 2])                                # not contiguous, wrong D
    refused(k=kc.view(-1, BS, D))                                  # rank
    refused(v=vc[1:])                                              # shapes differ
    refused(k=kc.transpose(1, 2), v=vc.transpose(1, 2))


# ----------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("normalize", [True, False], ids=["l2", "raw"])
@pytest.mark.parametrize("mean", [True, False], ids=["mean", "cls"])
@pytest.mark.parametrize("H", [8, 384, 768, 1024])
def test_pool_l2(native, H, mean, normalize):
    h, cu = O.pool_case(H, DEV)
    out = native.pool_l2(h, cu, mean, normalize)
    assert out.dtype == torch.float32
    O.assert_oracle(out, *O.pool_l2(h, cu, mean, normalize), what="pool_l2")
    assert not out[O.POOL_LENS.index(0)].any(), "empty sequence: a zero row, no NaN"


def test_pool_l2_refusals(native):
    h, cu = O.make_pool(1032, 81, DEV)
    with pytest.raises(RuntimeError):
        native.pool_l2(h, cu, True, True)


# ----------------------------------------------------------------------------- alignment
def _off1(t):
    """A contiguous view of ``t``'s values whose storage starts one element off 16-byte alignment."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def test_vector_load_kernels_refuse_misaligned_views(native):
    """Every tensor these ops read or write as uint4 / uint2 / float4 is refused by the binding
    when its storage offset breaks 16-byte alignment.  The refusals are host-side checks that
    come before any launch (CHECK_ALIGN16 in bindings.cpp)."""
    def refused(fn, *args):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            fn(*args)

    H = 1024
    x, r, w, g = O.make_rows(3, H, 90, DEV), O.make_rows(3, H, 91, DEV), O.make_weight(H, 92, DEV), \
        O.make_weight(H, 93, DEV)
    refused(native.rmsnorm, _off1(x), w, EPS)
    refused(native.rmsnorm, x, _off1(w), EPS)
    refused(native.add_rmsnorm, _off1(x), r.clone(), w, EPS)
    refused(native.add_rmsnorm, x, _off1(r), w, EPS)
    refused(native.add_rmsnorm, x, r.clone(), _off1(w), EPS)
    refused(native.layernorm, _off1(x), None, w, g, LN_EPS)
    refused(native.layernorm, x, _off1(r), w, g, LN_EPS)
    refused(native.layernorm, x, None, _off1(w), g, LN_EPS)
    refused(native.layernorm, x, None, w, _off1(g), LN_EPS)
    gu = O.make_gate_up(3, 512, 94, False, DEV)
    refused(native.silu_mul, _off1(gu), False)
    refused(native.silu_mul, _off1(gu), True)
    for gelu in (False, True):
        refused(native.bias_act, _off1(x), w, None, gelu)
        refused(native.bias_act, x, _off1(w), None, gelu)
        refused(native.bias_act, x, w, _off1(r), gelu)
    h, cu = O.make_pool(384, 95, DEV)
    refused(native.pool_l2, _off1(h), cu, True, True)
    Hq, Hkv, D, T, BS = 8, 2, 128, 50, 16
    c = O.make_rope(Hq, Hkv, D, T, BS, 96, DEV)
    kc, vc = _rope_caches(c, Hkv, BS, D)
    refused(native.rope_cache, _off1(c["qkv"]), c["pos"], c["cos_sin"], c["slots"], kc, vc, Hq, Hkv, D)
    refused(native.rope_cache, c["qkv"].clone(), c["pos"], _off1(c["cos_sin"]), c["slots"], kc, vc, Hq, Hkv, D)
    refused(native.rope_cache, c["qkv"].clone(), c["pos"], c["cos_sin"], c["slots"], _off1(kc), vc, Hq, Hkv, D)
    refused(native.rope_cache, c["qkv"].clone(), c["pos"], c["cos_sin"], c["slots"], kc, _off1(vc), Hq, Hkv, D)
    P = _slabs(2, 3, H, 97, torch.float32)
    refused(native.add_rmsnorm_splitk, _off1(P), r.clone(), w, EPS)
    refused(native.add_rmsnorm_splitk, P, _off1(r), w, EPS)
    refused(native.add_rmsnorm_splitk, P, r.clone(), _off1(w), EPS)
