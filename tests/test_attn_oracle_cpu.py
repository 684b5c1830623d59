"""The tracer oracle of tests/attn_oracle.py has teeth: ``ops.reference`` passes it on tracer
inputs, and hand-mutated copies of the reference attention -- a key dropped, counted twice or
read past the end, a causal mask one row off, the cascade seam key lost -- fail it at a window
that covers the mutated key.  Also: the relative-L2 bound of the long-context random tests is
four times what an emulation of the kernels' arithmetic measures, and it rejects a 64-key
block dropped at L = 2560.  No GPU, no native code."""
import math

import pytest
import torch

from docqa_amd.ops import reference as R
from tests import attn_oracle as O

D, BS = 128, 64
BF = torch.bfloat16


# ------------------------------------------------------------- mutated reference copies
def _decode_mut(q, kc, vc, bt, cl, Hq, scale, keys_of):
    """ops.reference.paged_decode with the attended key positions of row b given by
    ``keys_of(b, L)`` (a LongTensor; the clean kernel attends arange(L)): a copy of the
    reference a mutation can drop, repeat or over-read keys in."""
    B, Hkv = q.shape[0], kc.shape[1]
    G = Hq // Hkv
    out = torch.zeros(B, Hq * D, dtype=q.dtype)
    for b in range(B):
        idx = keys_of(b, int(cl[b]))
        if idx.numel() == 0:
            continue
        k = O.logical_v(kc, bt[b])[:, idx].float()
        v = O.logical_v(vc, bt[b])[:, idx].float()
        qb = q[b, :Hq * D].view(Hkv, G, D).float()
        p = torch.softmax(torch.einsum("hgd,htd->hgt", qb, k) * scale, -1)
        out[b] = torch.einsum("hgt,htd->hgd", p, v).reshape(-1).to(q.dtype)
    return out


def _prefill_mut(qkv, cu, Hq, Hkv, scale, widen, kl=None, vl=None, ctx=None, Dh=D):
    """ops.reference.flash_prefill / flash_prefill_paged (kl / vl: per-sequence logical keys,
    ctx: prefix lengths) with the causal mask ``kpos > qpos + widen``."""
    T = qkv.shape[0]
    x = qkv.view(T, Hq + 2 * Hkv, Dh)
    G = Hq // Hkv
    out = torch.zeros(T, Hq * Dh, dtype=qkv.dtype)
    for b in range(len(cu) - 1):
        s0, s1 = cu[b], cu[b + 1]
        L = s1 - s0
        P0 = 0 if ctx is None else ctx[b]
        if kl is None:
            k = x[s0:s1, Hq:Hq + Hkv].float().transpose(0, 1)
            v = x[s0:s1, Hq + Hkv:].float().transpose(0, 1)
        else:
            k, v = kl[b][:, :P0 + L].float(), vl[b][:, :P0 + L].float()
        k, v = k.repeat_interleave(G, 0), v.repeat_interleave(G, 0)
        q = x[s0:s1, :Hq].float().transpose(0, 1)
        s = torch.einsum("hld,hmd->hlm", q, k) * scale
        qpos = torch.arange(P0, P0 + L)[:, None]
        kpos = torch.arange(P0 + L)[None, :]
        s = s.masked_fill(kpos > qpos + widen, -math.inf)
        o = torch.einsum("hlm,hmd->hld", torch.softmax(s, -1), v)
        out[s0:s1] = o.transpose(0, 1).reshape(L, Hq * Dh).to(qkv.dtype)
    return out


# ------------------------------------------------------------------------ decode inputs
def _decode_case(lens, Hkv, G, maxb, windows, seed=0):
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    NB = B * maxb
    bt = torch.randperm(NB, generator=g).view(B, maxb)
    kc = torch.randn(NB, Hkv, BS, D, generator=g).to(BF)
    v = O.paged_v(NB, Hkv, BS, D, bt.tolist(), windows)
    q = torch.zeros(B, (G + 2) * Hkv * D, dtype=BF)
    return q, kc, v, bt, torch.tensor(lens, dtype=torch.int32)


def _decode_fails(out, v, bt, lens, G):
    fails = []
    for b, tab in enumerate(bt.tolist()):
        e, k = O.expect_rows(O.logical_v(v, tab), [lens[b]])
        fails += O.check_rows(out[b:b + 1], e, k, G, rows=[b])
    return fails


LENS = [1, 63, 64, 65, 129, 300, 0]
SEAM = 192       # a partition seam of the 300-key row (split_chunk(300, 5) = 64: 64, 128, 192, 256)


def _windows(lens, Hkv, seams):
    """The first launch's windows of every row, plus (for the long row) the launch that covers
    SEAM and L."""
    sets = [O.cover_windows(L, seams, Hkv, D) for L in lens]
    return O.launches(sets)


@pytest.mark.parametrize("G", [1, 4])
def test_clean_reference_passes_decode(G):
    Hkv = 2
    assert O.split_seams(300, 5) == [64, 128, 192, 256] and O.split_chunk(300, 5) == 64
    for win in _windows(LENS, Hkv, O.split_seams(300, 5)):
        q, kc, v, bt, cl = _decode_case(LENS, Hkv, G, 6, win)
        vc = v.to(BF)
        out = R.paged_decode(q[:-1], kc, vc, bt[:-1], cl[:-1], G * Hkv, 6 * BS, 1 / math.sqrt(D))
        out = torch.cat([out, torch.zeros(1, G * Hkv * D, dtype=BF)])        # the padded row: zeros
        assert not _decode_fails(out, v, bt, LENS, G)
        same = _decode_mut(q, kc, vc, bt, cl, G * Hkv, 1 / math.sqrt(D), lambda b, L: torch.arange(L))
        assert torch.equal(same, out)


MUTANTS = {
    "last key dropped": (lambda b, L: torch.arange(max(L - 1, 0)), lambda L: L - 1),
    "seam key dropped": (lambda b, L: torch.tensor([j for j in range(L) if j != SEAM]), lambda L: SEAM),
    "key before the seam dropped": (lambda b, L: torch.tensor([j for j in range(L) if j != SEAM - 1]),
                                    lambda L: SEAM - 1),
    "seam key counted twice": (lambda b, L: torch.cat([torch.arange(L), torch.tensor([SEAM] if L > SEAM else [],
                                                                                     dtype=torch.long)]),
                               lambda L: SEAM),
    "one key past L read": (lambda b, L: torch.arange(L + 1), lambda L: L),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_decode_mutant_fails_at_its_key(name):
    keys_of, where = MUTANTS[name]
    Hkv, G = 2, 4
    lens = [65, 300]
    named = set()
    for win in _windows(lens, Hkv, O.split_seams(300, 5)):
        q, kc, v, bt, cl = _decode_case(lens, Hkv, G, 6, win)
        out = _decode_mut(q, kc, v.to(BF), bt, cl, G * Hkv, 1 / math.sqrt(D), keys_of)
        fails = _decode_fails(out, v, bt, lens, G)
        named |= {(f.split(" ")[1], k) for f in fails for k in O.failed_keys([f])}
    assert ("1", where(300)) in named, (name, sorted(named)[:8])     # the 300-key row, at the mutated key
    if "seam" not in name:
        assert ("0", where(65)) in named, (name, sorted(named)[:8])


# ------------------------------------------------------------------------------ cascade
@pytest.mark.parametrize("Lp,nchunk", [(0, 1), (192, 3), (448, 8)])
def test_cascade_reference_and_seam_mutants(Lp, nchunk):
    Hkv, G, maxb = 8, 4, 12
    npb = Lp // BS
    lens = [Lp + 1, Lp + 64, Lp, 700]
    B = len(lens)
    tables = [list(range(npb)) + list(range(npb + b * (maxb - npb), npb + (b + 1) * (maxb - npb))) for b in range(B)]
    NB = npb + B * (maxb - npb)
    assert O.cascade_seams(448, 8) == [64, 128, 192, 256, 320, 384, 448] and O.cascade_seams(192, 3) == [64, 128, 192]
    win = [O.tile_windows(Hkv, D)] * B               # 1024 keys: every key and seam of a 768-key table
    v = O.paged_v(NB, Hkv, BS, D, tables, win)
    g = torch.Generator().manual_seed(Lp)
    kc = torch.randn(NB, Hkv, BS, D, generator=g).to(BF)
    q = torch.zeros(B, 6 * Hkv * D, dtype=BF)
    bt = torch.tensor(tables)
    cl = torch.tensor(lens, dtype=torch.int32)
    st = torch.zeros(maxb, dtype=torch.int32)
    st[:npb] = torch.arange(npb)
    out = R.paged_decode_cascade(q, kc, v.to(BF), bt, cl, G * Hkv, maxb * BS, 0.1, st, torch.tensor([Lp]), nchunk)
    counts = [L if L > Lp else 0 for L in lens]       # a row with no suffix key gives zeros
    assert not _decode_fails(out, v, bt, counts, G)
    assert bool((out[2] == 0).all())
    for lost in (Lp, Lp - 1) if Lp else (Lp,):        # the first suffix key / the last prefix key lost
        mut = _decode_mut(q, kc, v.to(BF), bt, cl, G * Hkv, 0.1,
                          lambda b, L: torch.tensor([j for j in range(L if L > Lp else 0) if j != lost],
                                                    dtype=torch.long))
        fails = _decode_fails(mut, v, bt, counts, G)
        assert lost in O.failed_keys(fails), (lost, fails[:4])


def _named(fails):
    """{(row, key position)} of check_rows failures."""
    return {(int(f.split(" ")[1]), k) for f in fails for k in O.failed_keys([f])}


# ------------------------------------------------------------------------------ prefill
PRE_LENS = [1, 63, 64, 65, 129, 257]


@pytest.mark.parametrize("Dh,Hq,Hkv", [(128, 8, 2), (128, 16, 2), (128, 8, 1), (64, 6, 6), (32, 6, 6)])
@pytest.mark.parametrize("causal", [True, False])
def test_flash_prefill_reference_and_mask_mutants(Dh, Hq, Hkv, causal):
    G = Hq // Hkv
    cu = [0]
    for L in PRE_LENS:
        cu.append(cu[-1] + L)
    sets = O.launches([O.cover_windows(L, [64, 128, 192], Hkv, Dh) for L in PRE_LENS])
    caught = {}
    for win in sets:
        vt = O.packed_v(PRE_LENS, Hkv, Dh, win)
        g = torch.Generator().manual_seed(Dh)
        x = torch.zeros(cu[-1], Hq + 2 * Hkv, Dh, dtype=BF)
        x[:, Hq:Hq + Hkv] = torch.randn(cu[-1], Hkv, Dh, generator=g).to(BF)
        x[:, Hq + Hkv:] = vt.to(BF)
        qkv = x.view(cu[-1], -1)
        out = R.flash_prefill(qkv, torch.tensor(cu), max(PRE_LENS), Hq, Hkv, Dh, 0.1, causal)

        def fails_of(o):
            fails = []
            for b, L in enumerate(PRE_LENS):
                vl = vt[cu[b]:cu[b + 1]].transpose(0, 1)
                e, k = O.expect_rows(vl, [i + 1 if causal else L for i in range(L)])
                fails += O.check_rows(o[cu[b]:cu[b + 1]], e, k, G, rows=list(range(cu[b], cu[b + 1])))
            return fails

        assert not fails_of(out)
        if causal:
            for widen in (1, -1):
                mut = _prefill_mut(qkv, cu, Hq, Hkv, 0.1, widen, Dh=Dh)
                mut = torch.nan_to_num(mut.float()).to(BF)       # a row with no key left: 0 / 0
                caught.setdefault(widen, set()).update(_named(fails_of(mut)))
    if causal:      # row 10 of the 65-token sequence: one key too many is key 11, one too few loses key 10
        row = cu[3] + 10
        assert (row, 11) in caught[1], sorted(caught[1])[:8]
        assert (row, 10) in caught[-1], sorted(caught[-1])[:8]


@pytest.mark.parametrize("G", [4, 8])
def test_flash_prefill_paged_reference_and_mask_mutants(G):
    Hkv, maxb = 2, 10
    Hq = G * Hkv
    prefix, new = [0, 17, 64, 130, 448], [1, 5, 64, 130, 40]
    B = len(new)
    cu = [0]
    for L in new:
        cu.append(cu[-1] + L)
    g = torch.Generator().manual_seed(G)
    bt = torch.randperm(B * maxb, generator=g).view(B, maxb)
    kc = torch.randn(B * maxb, Hkv, BS, D, generator=g).to(BF)
    sets = O.launches([O.cover_windows(P + L, [P, P + L - 1], Hkv, D) for P, L in zip(prefix, new)])
    qkv = torch.zeros(cu[-1], (Hq + 2 * Hkv) * D, dtype=BF)
    caught = {}
    for win in sets:
        v = O.paged_v(B * maxb, Hkv, BS, D, bt.tolist(), win)
        out = R.flash_prefill_paged(qkv, torch.tensor(cu), max(new), Hq, Hkv, D, 0.1, kc, v.to(BF), bt,
                                    torch.tensor(prefix))

        def fails_of(o):
            fails = []
            for b in range(B):
                e, k = O.expect_rows(O.logical_v(v, bt[b]), [prefix[b] + i + 1 for i in range(new[b])])
                fails += O.check_rows(o[cu[b]:cu[b + 1]], e, k, G, rows=list(range(cu[b], cu[b + 1])))
            return fails

        assert not fails_of(out)
        kl = [O.logical_v(kc, bt[b]) for b in range(B)]
        vl = [O.logical_v(v.to(BF), bt[b]) for b in range(B)]
        for widen in (1, -1):
            mut = _prefill_mut(qkv, cu, Hq, Hkv, 0.1, widen, kl, vl, prefix)
            mut = torch.nan_to_num(mut.float()).to(BF)
            caught.setdefault(widen, set()).update(_named(fails_of(mut)))
    # new row 10 of the sequence with P0 = 64: one key too many is key P0 + 11, one too few loses P0 + 10
    row, P0 = cu[2] + 10, prefix[2]
    assert (row, P0 + 11) in caught[1], sorted(caught[1])[:8]
    assert (row, P0 + 10) in caught[-1], sorted(caught[-1])[:8]


# ---------------------------------------------------------------------- relative metric
def test_relative_bound_is_four_times_the_emulation():
    """REL_MEASURED is the worst per-(row, head) relative L2 error of the emulated kernel
    arithmetic (bf16 P, fp32 accumulation, bf16 output) against float64 at the shapes and
    seeds of the GPU tests; REL_BOUND allows four times that."""
    worst = 0.0
    for seed, Hq, Hkv, L in O.REL_CASES:
        q, k, v = O.rel_case(seed, 2, Hq, Hkv, L)
        G = Hq // Hkv
        ref = O.rel_reference(q, k, v, 1 / math.sqrt(D))
        emu = torch.stack([O.attention_emulated(q[b], k[b].repeat_interleave(G, 0), v[b].repeat_interleave(G, 0),
                                                1 / math.sqrt(D)).reshape(-1) for b in range(2)])
        worst = max(worst, float(O.rel_l2(emu, ref, Hq).max()))
    print(f"emulation worst rel L2 {worst:.6g}; REL_MEASURED {O.REL_MEASURED:.6g}")
    assert worst <= O.REL_MEASURED <= 1.05 * worst
    assert O.REL_BOUND == 4 * O.REL_MEASURED


def test_relative_bound_rejects_a_dropped_block_at_2560():
    """The absolute tolerance of the random tests passes a whole missing 64-key block at
    L = 2560; the relative bound does not, wherever the block lies."""
    L, Hq, Hkv = 2560, 8, 2
    q, k, v = O.rel_case(1, 1, Hq, Hkv, L)
    scale = 1 / math.sqrt(D)
    ref = O.rel_reference(q, k, v, scale)
    for blk in (0, 17, 39):
        keep = torch.cat([torch.arange(0, blk * 64), torch.arange((blk + 1) * 64, L)])
        mut = O.rel_reference(q, k[:, :, keep], v[:, :, keep], scale)
        r = O.rel_l2(mut, ref, Hq)
        assert float(r.min()) > O.REL_BOUND, (blk, float(r.min()))
        assert float((mut - ref).abs().max()) < 2e-2 + 1e-2 * float(ref.abs().max())   # what the old metric saw
