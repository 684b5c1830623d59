"""The row-compaction kernels (csrc/kernels/compact.hip: ``ops.masked_scan``, ``gather_rows``,
``csr_gather``, ``remap_ids``) against numpy (``np.cumsum``, boolean indexing).

Everything here is copying and integer sums, so every comparison is exact equality.  Sizes sit
on the boundaries of the scan tile (``ops.SCAN_TILE``) and reach the one size that needs every
scan level (``SCAN_TILE ** (SCAN_LEVELS - 1) + 1`` rows); row widths cover the three lane forms
of the gather (16-byte, 4-byte, bytes), each also from bases that break 16-byte and 4-byte
alignment.  Offsets past 2^31 entries are not reachable in a test of seconds: the int64 index
arithmetic of the kernels is checked by review.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASKS = ("all", "none", "first", "last", "alternating", "run", "random1", "random50")
WIDTHS = (1, 4, 6, 8, 48, 768, 1536)
# (source offset, destination offset) in bytes from a 256-byte aligned base
BASES = ((0, 0), (4, 4), (1, 1), (0, 4), (16, 2))


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops._native().compact_scan_tile() == ops.SCAN_TILE
    assert ops._native().compact_scan_levels() == ops.SCAN_LEVELS
    return ops


def sizes(ops):
    t = ops.SCAN_TILE
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1]


def every_level(ops) -> int:
    return ops.SCAN_TILE ** (ops.SCAN_LEVELS - 1) + 1


def make_mask(n: int, kind: str, tile: int, seed: int = 0) -> np.ndarray:
    keep = np.ones(n, dtype=np.uint8)
    rng = np.random.default_rng(seed + n)
    if kind == "none":
        keep[:] = 0
    elif kind == "first":
        keep[:1] = 0
    elif kind == "last":
        keep[-1:] = 0
    elif kind == "alternating":
        keep[1::2] = 0
    elif kind == "run":            # one removed run straddling a tile boundary
        b = tile if n > tile else max(0, n // 2)
        keep[max(0, b - 3):b + 3] = 0
    elif kind == "random1":
        keep[rng.random(n) < 0.01] = 0
    elif kind == "random50":
        keep[rng.random(n) < 0.5] = 0
    return keep


def np_scan(keep: np.ndarray, w: np.ndarray | None = None) -> np.ndarray:
    v = (keep != 0).astype(np.int64) if w is None else np.where(keep != 0, w, 0).astype(np.int64)
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(v, dtype=np.int64)])


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a).to(DEV)


# ------------------------------------------------------------------ masked scan
@pytest.mark.parametrize("kind", MASKS)
def test_masked_scan_sizes(native, kind):
    for n in sizes(native) + [every_level(native)]:
        keep = make_mask(n, kind, native.SCAN_TILE)
        pos = native.masked_scan(dev(keep))
        assert pos.dtype == torch.int64 and pos.shape == (n + 1,)
        assert np.array_equal(pos.cpu().numpy(), np_scan(keep)), (kind, n)


def test_masked_scan_weighted_with_zero_length_rows(native):
    rng = np.random.default_rng(7)
    for n in sizes(native) + [every_level(native)]:
        keep = make_mask(n, "random50", native.SCAN_TILE, seed=3)
        w = rng.integers(0, 6, size=n).astype(np.int64)
        w[rng.random(n) < 0.3] = 0                       # zero-length rows
        if n:
            w[rng.integers(0, n, size=min(n, 4))] = (1 << 33) + 5      # sums past 32 bits
        pos = native.masked_scan(dev(keep), dev(w))
        assert np.array_equal(pos.cpu().numpy(), np_scan(keep, w)), n


def test_masked_scan_is_deterministic(native):
    n = every_level(native)
    keep = dev(make_mask(n, "random50", native.SCAN_TILE))
    a = native.masked_scan(keep)
    for _ in range(3):
        assert torch.equal(native.masked_scan(keep), a)


# ------------------------------------------------------------------ fixed-width row gather
def gather_case(ops, n: int, W: int, keep: np.ndarray, so: int, do: int, seed: int = 0):
    rng = np.random.default_rng(seed + 31 * n + W)
    data = rng.integers(0, 256, size=(n, W), dtype=np.uint8)
    n_out = int((keep != 0).sum())
    sbuf = torch.zeros(n * W + 64, dtype=torch.uint8, device=DEV)
    src = sbuf[so:so + n * W].view(n, W)
    src.copy_(dev(data))
    guard = 0xA5
    dbuf = torch.full((n_out * W + 64,), guard, dtype=torch.uint8, device=DEV)
    out = dbuf[do:do + n_out * W].view(n_out, W)
    k = dev(keep)
    pos = ops.masked_scan(k)
    got = ops.gather_rows(src, k, pos, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), data[keep != 0]), (n, W, so, do)
    host = dbuf.cpu().numpy()                                # nothing written outside the destination
    assert (host[:do] == guard).all() and (host[do + n_out * W:] == guard).all(), (n, W, so, do)
    assert np.array_equal(src.cpu().numpy(), data)           # out of place: the source is untouched


@pytest.mark.parametrize("W", WIDTHS)
def test_gather_rows_widths_masks_and_bases(native, W):
    t = native.SCAN_TILE
    for n in (1, 65, t + 1, 2 * t + 1):
        for kind in MASKS:
            keep = make_mask(n, kind, t)
            for so, do in BASES:
                gather_case(native, n, W, keep, so, do)


@pytest.mark.parametrize("W", WIDTHS)
def test_gather_rows_small_sizes(native, W):
    t = native.SCAN_TILE
    for n in (0, 63, 64, t - 1, t):
        for kind in ("all", "none", "first", "last", "random50"):
            gather_case(native, n, W, make_mask(n, kind, t), 0, 0)
            gather_case(native, n, W, make_mask(n, kind, t), 1, 4)


@pytest.mark.parametrize("kind", MASKS)
def test_gather_rows_every_scan_level(native, kind):
    n = every_level(native)
    keep = make_mask(n, kind, native.SCAN_TILE)
    gather_case(native, n, 4, keep, 0, 0)


def test_grid_stride_loops_take_more_than_one_round(native):
    """Every gather grid is capped at 8192 workgroups and strides over the rest: one exactness case
    each past the cap -- more than 8192 chunks of 1024 lane units in the row gather (90k rows of
    1536 B are 8.4M 16-byte units), more than 8192 x 16 rows in the CSR gather, more than
    8192 x 256 ids in the remap."""
    n, d = 90_000, 384
    keep = make_mask(n, "random1", native.SCAN_TILE)
    keep[:3] = 0
    k = dev(keep)
    pos = native.masked_scan(k)
    sel = torch.from_numpy(keep != 0).to(DEV)
    src = torch.randn(n, d, device=DEV)
    out = native.gather_rows(src, k, pos, int(keep.sum()))
    assert torch.equal(out, src[sel])
    del src, out
    n = 140_000
    rng = np.random.default_rng(17)
    lens = rng.integers(0, 12, size=n)
    csr_case(native, lens, make_mask(n, "random50", native.SCAN_TILE))
    csr_case(native, lens, make_mask(n, "last", native.SCAN_TILE))
    n = 2_200_000
    keep = make_mask(n, "random50", native.SCAN_TILE)
    ids = rng.permutation(np.nonzero(keep)[0]).astype(np.int64)
    ids = np.concatenate([ids, ids[:1_200_000]])           # 2.3M entries
    got = native.remap_ids(dev(ids), native.masked_scan(dev(keep)))
    assert np.array_equal(got.cpu().numpy(), np_scan(keep)[ids])


def test_gather_rows_serves_every_column_dtype(native):
    n, t = 2 * native.SCAN_TILE + 1, native.SCAN_TILE
    keep = make_mask(n, "random50", t)
    k = dev(keep)
    pos = native.masked_scan(k)
    n_out = int(keep.sum())
    g = torch.Generator().manual_seed(5)
    cols = [torch.randn(n, 384, generator=g), torch.randn(n, 384, generator=g).to(torch.bfloat16),
            torch.randn(n, generator=g), torch.randint(-5, 1 << 30, (n,), generator=g, dtype=torch.int32),
            torch.randint(0, 256, (n, 48), generator=g, dtype=torch.uint8),
            torch.randint(-(1 << 40), 1 << 40, (n,), generator=g, dtype=torch.int64)]
    sel = torch.from_numpy(keep != 0)
    for c in cols:
        out = native.gather_rows(c.to(DEV), k, pos, n_out)
        assert out.dtype == c.dtype and out.shape == (n_out,) + tuple(c.shape[1:])
        assert torch.equal(out.cpu(), c[sel]), c.dtype


def test_gather_rows_into_a_larger_buffer_leaves_the_tail(native):
    n = 300
    keep = make_mask(n, "alternating", native.SCAN_TILE)
    k = dev(keep)
    src = torch.arange(n * 4, dtype=torch.float32, device=DEV).view(n, 4)
    out = torch.full((n + 10, 4), -1.0, device=DEV)
    native.gather_rows(src, k, native.masked_scan(k), out=out)
    m = int(keep.sum())
    assert torch.equal(out[:m], src[torch.from_numpy(keep != 0).to(DEV)])
    assert bool((out[m:] == -1).all())


# ------------------------------------------------------------------ CSR gather
def csr_case(ops, lens: np.ndarray, keep: np.ndarray, seed: int = 0, slack: int = 5):
    rng = np.random.default_rng(seed)
    n = lens.size
    row_ptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens, dtype=np.int64)])
    E = int(row_ptr[-1])
    terms = rng.integers(-(1 << 31), 1 << 31, size=E + slack).astype(np.int32)   # capacity past the entries
    tfs = rng.integers(0, 256, size=E + slack).astype(np.uint8)
    k = dev(keep)
    pos = ops.masked_scan(k)
    epos = ops.masked_scan(k, dev(lens.astype(np.int64)))
    sel = keep != 0
    esel = np.repeat(sel, lens)
    n_out, e_out = int(sel.sum()), int(esel.sum())
    new_ptr, new_terms, new_tfs = ops.csr_gather(dev(row_ptr), k, pos, epos, dev(terms), dev(tfs), n_out, e_out)
    want_ptr = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens[sel], dtype=np.int64)])
    assert np.array_equal(new_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(new_terms.cpu().numpy(), terms[:E][esel])
    assert np.array_equal(new_tfs.cpu().numpy(), tfs[:E][esel])
    assert new_ptr.dtype == torch.int64 and new_terms.dtype == torch.int32 and new_tfs.dtype == torch.uint8


def test_csr_gather(native):
    t = native.SCAN_TILE
    rng = np.random.default_rng(11)
    for n in (1, 2, 17, 65, t + 1, 2 * t + 1):
        lens = rng.integers(0, 70, size=n)
        lens[rng.random(n) < 0.25] = 0                     # empty rows
        for kind in MASKS:
            csr_case(native, lens, make_mask(n, kind, t))
        first = lens.copy(); first[0] = 0                  # an empty first row, kept and removed
        csr_case(native, first, make_mask(n, "all", t))
        csr_case(native, first, make_mask(n, "first", t))
        last = lens.copy(); last[-1] = 0                   # an empty last row, kept and removed
        csr_case(native, last, make_mask(n, "all", t))
        csr_case(native, last, make_mask(n, "last", t))
        csr_case(native, lens, make_mask(n, "none", t))    # all rows removed
        csr_case(native, np.zeros(n, dtype=np.int64), make_mask(n, "random50", t), slack=0)   # an empty CSR
    csr_case(native, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8), slack=0)       # no rows at all


# ------------------------------------------------------------------ id remap
def test_remap_ids(native):
    t = native.SCAN_TILE
    rng = np.random.default_rng(13)
    for n in (1, 65, 2 * t + 1, every_level(native)):
        keep = make_mask(n, "random50", t)
        pos = native.masked_scan(dev(keep))
        ids = rng.permutation(np.nonzero(keep)[0]).astype(np.int64)     # a list that survived, list order
        got = native.remap_ids(dev(ids), pos)
        assert np.array_equal(got.cpu().numpy(), np_scan(keep)[ids])
        # the surviving ids land on 0..n'-1, each once
        assert np.array_equal(np.sort(got.cpu().numpy()), np.arange(ids.size))
    bad = torch.tensor([-1, 5, 0], dtype=torch.int64, device=DEV)
    assert native.remap_ids(bad, native.masked_scan(dev(np.ones(3, np.uint8)))).tolist() == [-1, -1, 0]


# ------------------------------------------------------------------ kill switch / envelope
def test_kill_switch_and_out_of_envelope_equal_the_reference(native, monkeypatch):
    from docqa_amd.ops import reference as ref

    t = native.SCAN_TILE
    n = 2 * t + 1
    keep_np = make_mask(n, "random50", t)
    keep = dev(keep_np)
    lens = dev(np.random.default_rng(1).integers(0, 9, size=n).astype(np.int64))
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    row_ptr[1:] = torch.cumsum(lens, 0)
    E = int(row_ptr[-1])
    terms = torch.arange(E, dtype=torch.int32, device=DEV)
    tfs = (torch.arange(E, device=DEV) % 251).to(torch.uint8)
    src = torch.randn(n, 6, device=DEV)
    ids = dev(np.nonzero(keep_np)[0].astype(np.int64))

    def run():
        pos = native.masked_scan(keep)
        epos = native.masked_scan(keep, lens)
        n_out, e_out = int(pos[-1]), int(epos[-1])
        return (pos, epos, native.gather_rows(src, keep, pos, n_out), native.remap_ids(ids, pos),
                *native.csr_gather(row_ptr, keep, pos, epos, terms, tfs, n_out, e_out))

    on = run()
    called = []
    real = native._native
    monkeypatch.setattr(native, "_native", lambda: called.append(1) or real())
    monkeypatch.setenv("DOCQA_COMPACT", "0")
    off = run()
    assert not called, "DOCQA_COMPACT=0 must not reach the native kernels"
    monkeypatch.delenv("DOCQA_COMPACT")
    pos, epos = ref.masked_scan(keep), ref.masked_scan(keep, lens)
    n_out, e_out = int(pos[-1]), int(epos[-1])
    want = (pos, epos, ref.gather_rows(src, keep, pos, torch.empty(n_out, 6, device=DEV)), ref.remap_ids(ids, pos),
            *ref.csr_gather(row_ptr, keep, pos, epos, terms, tfs, n_out, e_out))
    for a, b, c in zip(on, off, want):
        assert a.is_cuda and b.is_cuda and torch.equal(a, c) and torch.equal(b, c)

    # outside the envelope: a bool mask, a strided source, rows wider than the gather serves
    assert torch.equal(native.masked_scan(keep.bool()), pos)
    assert not called
    wide = torch.randn(n, 12, device=DEV)[:, ::2]
    assert torch.equal(native.gather_rows(wide, keep, pos, n_out), wide[keep.bool()])
    assert not called
    big = torch.zeros(3, native.GATHER_MAX_ROW_BYTES + 16, dtype=torch.uint8, device=DEV)
    big[1] = 7
    k3 = torch.tensor([0, 1, 1], dtype=torch.uint8, device=DEV)
    assert torch.equal(native.gather_rows(big, k3, ref.masked_scan(k3), 2), big[1:])
    assert not called


def test_cpu_tensors_take_the_reference(native):
    keep = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    pos = native.masked_scan(keep)
    assert pos.tolist() == [0, 1, 1, 2, 3, 3]
    src = torch.arange(10.).view(5, 2)
    assert torch.equal(native.gather_rows(src, keep, pos, 3), src[[0, 2, 3]])
