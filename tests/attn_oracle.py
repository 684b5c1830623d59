"""Tracer oracle for key visibility in the attention kernels (plain torch, no native code).

Random Q / K / V hide the commonest attention bug: with diffuse softmax weights one key
carries ~1/L of an output that itself shrinks with L, far below the absolute tolerances of
the random-data tests.  The inputs built here make every single key visible instead:

* **Q = 0**: every score is 0 whatever K holds (random, finite) and whatever RoPE does, so
  the softmax over a row's n visible keys is exactly uniform, 1/n each.
* **V is a tracer**: the V row of key position ``j`` of KV head ``h`` is the one-hot
  ``e_{j mod D}`` when ``j`` lies in a window ``[w, w + D)`` chosen for that head, and the
  zero row otherwise (0 and 1 are exact in bf16 and e4m3).  Inside one window the columns
  ``j mod D`` are the ``e_{j-w}`` of a window starting at ``w`` rotated by ``w mod D``; keying
  the column on the position alone makes rows that share physical blocks (cascade prefix,
  prefix-cache tries) agree on what a shared block holds.
* **the expected output is closed form**, in float64, from the V actually built and the
  visible-key count of each query row -- never from a kernel: element ``d`` of every query
  head of KV head ``h`` is ``k / n`` with ``k`` the number of visible keys marked in column
  ``d`` (1 for a witnessed key, 0 otherwise; 2 only where two windows of rows sharing
  blocks collide), and 0 for a row with n = 0.

``check_rows`` demands that elements expected 0 are exactly 0 and the others are within
``BOUND`` of k/n, relative, and names row, head and key position of every miss.

BOUND.  The kernels keep the row sum and the P.V accumulator in fp32, so what is rounded is
  * the output, to bf16: 2^-9 relative (attn_decode.hip finish_partition
    ``out[...] = f2bf(lsum > 0.f ? v / lsum : 0.f)``, paged_decode_reduce ``f2bf(den > 0.f ?
    num / den : 0.f)``, the MFMA / group epilogues ``pack2(o[dd][0] * inv, ...)``;
    attn_prefill.hip epilogue ``v.x = pack2(o[dt][4 * g4 + 0] * inv, ...)``);
  * P, to bf16 ahead of the P.V MFMA where a kernel has one: another 2^-9 (attn_decode.hip
    ``pb[r] = (short)f2bf(x[c][r])`` in the MFMA, group, wave and persist kernels -- the FP8
    wave kernel has the same line, its codes are widened to bf16 first, nothing coarser;
    attn_prefill.hip ``pb[j] = (__bf16)x[kt][8 * s + j]``).  The VALU kernels (attend_rows:
    ``acc[g][j] += p * vf[j]``) keep P in fp32.
BOUND = 4 x (2^-9 + 2^-9) = 2^-6, far below the 1/4 that separates every mutant: a dropped,
doubled or over-read key moves its element to 0, to 2/n or from 0 to 1/(n+1).
"""
from __future__ import annotations

import torch

BOUND = 4 * (2.0 ** -9 + 2.0 ** -9)      # = 2^-6, see the module docstring
assert BOUND == 2.0 ** -6 and BOUND < 0.25


# ------------------------------------------------------------------------------ windows
def tile_windows(Hkv: int, D: int, start: int = 0) -> list:
    """Window starts that tile [start, start + Hkv * D): head h witnesses [start + h D, + D)."""
    return [start + h * D for h in range(Hkv)]


def cover_windows(L: int, seams, Hkv: int, D: int) -> list:
    """Window sets (one per launch, ``Hkv`` window starts or None each) for a row of L keys.

    A row with ``L + D / 2 <= Hkv * D`` gets one set tiling from 0: every key and every
    over-read position up to Hkv * D has its witness.  A longer row gets ``[s - D/2, s + D/2)``
    around every seam ``s`` and around L; overlapping intervals are merged and tiled with
    D-wide windows, Hkv per launch."""
    if L + D // 2 <= Hkv * D:
        return [tile_windows(Hkv, D)]
    iv = sorted({(max(0, s - D // 2), s + D // 2) for s in set(seams) | {L} if 0 <= s <= L})
    merged = []
    for a, b in iv:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    starts = [w for a, b in merged for w in range(a, b, D)]
    starts += [None] * (-len(starts) % Hkv)
    return [starts[i:i + Hkv] for i in range(0, len(starts), Hkv)]


def witnessed(sets: list, pos: int, D: int) -> bool:
    """Does some window of a row's window sets cover key position ``pos``?"""
    return any(w is not None and w <= pos < w + D for ws in sets for w in ws)


def launches(per_row_sets: list) -> list:
    """[row][launch][head] -> [launch][row][head], rows with fewer sets padded with no window."""
    n = max(len(s) for s in per_row_sets)
    Hkv = len(per_row_sets[0][0])
    return [[s[i] if i < len(s) else [None] * Hkv for s in per_row_sets] for i in range(n)]


# ------------------------------------------------------------------------------ tracer V
def paged_v(NB: int, Hkv: int, BS: int, D: int, tables, windows) -> torch.Tensor:
    """uint8 [NB, Hkv, BS, D] tracer cache: for row b and head h with window start
    w = windows[b][h] (None: no window), key j in [w, w + D) within the table's capacity
    is marked at V[tables[b][j // BS], h, j % BS, j % D]."""
    v = torch.zeros(NB, Hkv, BS, D, dtype=torch.uint8)
    for b, tab in enumerate(tables):
        cap = len(tab) * BS
        for h in range(Hkv):
            w = windows[b][h]
            if w is None:
                continue
            j = torch.arange(max(w, 0), max(min(w + D, cap), max(w, 0)))
            if j.numel():
                blk = torch.as_tensor(tab, dtype=torch.long)[j // BS]
                v[blk, h, j % BS, j % D] = 1
    return v


def logical_v(v: torch.Tensor, table) -> torch.Tensor:
    """[Hkv, cap, D] view of one row's keys through its block table."""
    g = v[torch.as_tensor(table, dtype=torch.long)]            # [nb, Hkv, BS, D]
    return g.permute(1, 0, 2, 3).reshape(v.shape[1], -1, v.shape[3])


def packed_v(lens, Hkv: int, D: int, windows) -> torch.Tensor:
    """uint8 [T, Hkv, D] tracer V rows of packed (un-paged) sequences: sequence b, head h,
    key j in [windows[b][h], + D) is marked in column j % D."""
    T = sum(lens)
    v = torch.zeros(T, Hkv, D, dtype=torch.uint8)
    s0 = 0
    for b, L in enumerate(lens):
        for h in range(Hkv):
            w = windows[b][h]
            if w is None:
                continue
            j = torch.arange(max(w, 0), max(min(w + D, L), max(w, 0)))
            if j.numel():
                v[s0 + j, h, j % D] = 1
        s0 += L
    return v


# ------------------------------------------------------------------------------ expected
def expect_rows(vl: torch.Tensor, counts):
    """vl [Hkv, cap, D] (one sequence's keys), counts: visible-key count n of each query row
    (keys [0, n)).  -> (exp float64 [R, Hkv, D] = marks among the visible keys / n, keys long
    [Hkv, D] = the first marked position of each column anywhere in the capacity, -1: none)."""
    Hkv, cap, D = vl.shape
    c = torch.cat([torch.zeros(Hkv, 1, D, dtype=torch.float64), vl.to(torch.float64).cumsum(1)], 1)
    n = torch.as_tensor(counts, dtype=torch.long).clamp(min=0, max=cap)
    exp = c[:, n].permute(1, 0, 2) / n.clamp(min=1)[:, None, None].to(torch.float64)
    assert int(c[:, -1].max()) <= 2, "more than two windows collide in one column"
    keys = torch.where(vl.bool().any(1), vl.to(torch.int8).argmax(1), torch.full((Hkv, D), -1))
    return exp, keys


def check_rows(out, exp, keys, G: int, rows=None, bound: float = BOUND) -> list:
    """out [R, Hq * D] (any float dtype / device) against exp [R, Hkv, D]; keys [Hkv, D] or
    [R, Hkv, D].  -> list of failure strings (empty: pass), each naming the row, query head,
    element and the key position that element witnesses."""
    R, Hkv, D = exp.shape
    o = out.detach().to("cpu", torch.float64).reshape(R, Hkv, G, D)
    e = exp[:, :, None, :].expand(R, Hkv, G, D)
    bad = torch.where(e == 0, o != 0, ~((o - e).abs() <= bound * e))     # a NaN fails too
    fails = []
    for r, h, g, d in bad.nonzero().tolist():
        key = int(keys[h, d] if keys.dim() == 2 else keys[r, h, d])
        row = r if rows is None else rows[r]
        fails.append(f"row {row} head {h * G + g} element {d} (key position {key}): got {o[r, h, g, d].item():.6g}, "
                     f"expected {e[r, h, g, d].item():.6g}")
    return fails


def failed_keys(fails: list) -> set:
    """The key positions named by ``check_rows`` failures."""
    return {int(f.split("key position ")[1].split(")")[0]) for f in fails}


def assert_rows(out, exp, keys, G: int, rows=None, label: str = "") -> None:
    fails = check_rows(out, exp, keys, G, rows)
    assert not fails, f"{label}: {len(fails)} tracer elements wrong, first:\n  " + "\n  ".join(fails[:12])


def check_paged(out, v, tables, counts, G: int, label: str = "") -> None:
    """One query row per sequence (decode): row b sees keys [0, counts[b]) of tables[b]."""
    exps, keys = [], []
    for b, tab in enumerate(tables):
        e, k = expect_rows(logical_v(v, tab), [counts[b]])
        exps.append(e)
        keys.append(k[None])
    assert_rows(out, torch.cat(exps), torch.cat(keys), G, label=label)


# ------------------------------------------------------------------ seams of the launchers
def decode_splits(B: int, Hkv: int, max_context: int) -> int:
    """attn_decode.hip docqa_decode_splits (default target of 512 workgroups):
    min(ceil(512 / (B Hkv)), ceil(max_context / 64), 64), at least 1."""
    return max(1, min(-(-512 // (B * Hkv)), -(-max_context // 64), 64))


def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def split_chunk(L: int, nsplit: int) -> int:
    """attn_decode.hip split_chunk: the slice ceil(L / nsplit) rounded up to 64, at least 64."""
    return max(64, _ceil(_ceil(L, nsplit), 64) * 64)


def cascade_chunk(Lp: int, nchunk: int) -> int:
    """docqa_cascade.h cascade_chunk: ceil(Lp / nchunk) rounded up to 64, at least 64."""
    return max(64, _ceil(_ceil(Lp, nchunk), 64) * 64)


def split_seams(L: int, max_parts: int, start: int = 0) -> list:
    """Partition seams of the keys [start, L) cut by split_chunk(L - start, max_parts)."""
    if L <= start:
        return []
    c = split_chunk(L - start, max_parts)
    return list(range(start + c, L, c))


def cascade_seams(Lp: int, nchunk: int) -> list:
    """Chunk edges inside the shared prefix, and the prefix / suffix seam Lp itself."""
    if Lp <= 0:
        return []
    return list(range(cascade_chunk(Lp, nchunk), Lp, cascade_chunk(Lp, nchunk))) + [Lp]


# ------------------------------------------------------------------- relative L2 metric
def rel_l2(o, ref, Hq: int):
    """Per (row, head) ||o - ref||_2 / ||ref||_2 over the head dim, float64 -> [R, Hq]."""
    a = o.detach().to("cpu", torch.float64).reshape(o.shape[0], Hq, -1)
    r = ref.detach().to("cpu", torch.float64).reshape(o.shape[0], Hq, -1)
    return (a - r).norm(dim=-1) / r.norm(dim=-1)


def attention_f64(q, k, v, scale: float):
    """q [H, D], k / v [H, n, D] -> softmax(q k^T scale) v in float64."""
    q, k, v = q.double(), k.double(), v.double()
    p = torch.softmax(torch.einsum("hd,hnd->hn", q, k) * scale, -1)
    return torch.einsum("hn,hnd->hd", p, v)


def attention_emulated(q, k, v, scale: float, tile: int = 64):
    """The kernels' documented arithmetic on the CPU: scores and online softmax in fp32 over
    ``tile``-key tiles, P rounded to bf16 ahead of the P.V product, fp32 accumulation, fp32 row
    sum of the unrounded P, bf16 output."""
    q, k, v = q.float(), k.float(), v.float()
    H, n, D = k.shape
    m = torch.full((H,), -float("inf"))
    l = torch.zeros(H)
    acc = torch.zeros(H, D)
    for t0 in range(0, n, tile):
        s = torch.einsum("hd,hnd->hn", q, k[:, t0:t0 + tile]) * scale
        mn = torch.maximum(m, s.max(-1).values)
        a = torch.exp(m - mn)
        p = torch.exp(s - mn[:, None])
        l = l * a + p.sum(-1)
        acc = acc * a[:, None] + torch.einsum("hn,hnd->hd", p.bfloat16().float(), v[:, t0:t0 + tile])
        m = mn
    return (acc / l[:, None]).bfloat16()


# Worst per-(row, head) rel_l2 of ``attention_emulated`` against ``attention_f64`` over REL_CASES
# (measured by tests/test_attn_oracle_cpu.py::test_relative_bound_is_four_times_the_emulation,
# which recomputes it); the GPU tests allow REL_BOUND = 4 x that.
REL_CASES = tuple((seed, Hq, Hkv, L) for seed, (Hq, Hkv) in enumerate(((8, 2), (16, 2))) for L in (1000, 2560))
REL_MEASURED = 2.7e-3
REL_BOUND = 4 * REL_MEASURED


def rel_case(seed: int, B: int, Hq: int, Hkv: int, L: int, D: int = 128):
    """bf16 q [B, Hq, D], k / v [B, Hkv, L, D] ~ N(0, 1) from a CPU generator."""
    g = torch.Generator().manual_seed(1000 + seed)
    q = torch.randn(B, Hq, D, generator=g).bfloat16()
    k = torch.randn(B, Hkv, L, D, generator=g).bfloat16()
    v = torch.randn(B, Hkv, L, D, generator=g).bfloat16()
    return q, k, v


def rel_reference(q, k, v, scale: float, counts=None):
    """float64 attention of the bf16 inputs, row b over keys [0, counts[b]) -> [B, Hq * D]."""
    B, Hq, D = q.shape
    G = Hq // k.shape[1]
    out = []
    for b in range(B):
        n = k.shape[2] if counts is None else counts[b]
        out.append(attention_f64(q[b], k[b, :, :n].repeat_interleave(G, 0), v[b, :, :n].repeat_interleave(G, 0),
                                 scale).reshape(-1))
    return torch.stack(out)
