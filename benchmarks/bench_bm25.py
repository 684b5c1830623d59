"""The BM25 scan (``ops.bm25_topk``, csrc/kernels/lexical.hip) and the three-launch hybrid
search against the dense scan (``ops.knn``) on the same rows in the same process.

d = 384 fp32 dense rows beside term columns of about 60 entries per row (lengths 20..100,
terms Zipf-like over 100k values, tf 1..8), N = 1M (and 10M with --big), nq = 1 and 256, k = 3.
Query rows hold 8 real terms drawn from the same distribution.  Arms:

  a  ``ops.knn`` alone
  b  ``ops.bm25_topk`` alone
  c  hybrid: ``ops.knn`` and ``ops.bm25_topk`` at depth 16, then ``ops.rank_fuse``

The vectors (1.5 GB at 1M rows) and the columns (about 300 MB) are both larger than the 256 MB
last-level cache, so every scan streams from HBM.  Device events around ITERS calls, median of
WINDOWS windows, launch gaps included.

python benchmarks/bench_bm25.py [--big] [--n 1000000] -> one JSON line per measurement, then a
table."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

D = 384
VOCAB = 100_000
WINDOWS, ITERS = 5, 6


def _events(fn):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for w in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ITERS):
            fn(3 + w * ITERS + i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return statistics.median(ts), min(ts), max(ts)


def _zipf(n, g):
    """n draws over VOCAB values with p(rank) ~ 1 / rank (inverse CDF of the continuous law)."""
    u = torch.rand(n, device="cuda", generator=g)
    return torch.exp(u * torch.log(torch.tensor(float(VOCAB)))).long().clamp_(1, VOCAB) - 1


def columns(N, g):
    """CSR columns: sorted unique hashed terms per row (duplicate draws are dropped)."""
    lens = torch.randint(20, 101, (N,), device="cuda", generator=g)
    ptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    ptr[1:] = lens.cumsum(0)
    terms, tfs, counts = [], [], []
    step = 1 << 18
    for s in range(0, N, step):          # chunks: the sort temporaries stay small
        e = min(N, s + step)
        row = torch.repeat_interleave(torch.arange(s, e, device="cuda"), lens[s:e])
        h = (_zipf(row.numel(), g) * 2654435761) & 0xFFFFFFFF          # hash-like 32-bit values
        key = torch.unique(row * (1 << 32) + h)                        # by row, then unsigned term
        terms.append((key & 0xFFFFFFFF).to(torch.int32))               # wraps to the bit pattern
        counts.append(torch.bincount((key >> 32) - s, minlength=e - s))
        tfs.append(torch.randint(1, 9, (key.numel(),), device="cuda", generator=g, dtype=torch.uint8))
    cnt = torch.cat(counts)
    ptr[1:] = cnt.cumsum(0)
    return ptr, torch.cat(terms), torch.cat(tfs), cnt.to(torch.int32)


def queries(nq, g):
    qt = torch.full((nq, 32), -1, dtype=torch.int32, device="cuda")
    qw = torch.zeros(nq, 32, device="cuda")
    h = ((_zipf(nq * 8, g) * 2654435761) & 0xFFFFFFFF).to(torch.int32).reshape(nq, 8)
    for q in range(nq):                  # a repeated draw would count once: keep rows unique
        u = torch.unique(h[q])
        qt[q, : u.numel()] = u
        qw[q, : u.numel()] = torch.rand(u.numel(), device="cuda", generator=g) * 8 + 0.5
    return qt, qw


def bench(N, rows_out):
    g = torch.Generator(device="cuda").manual_seed(1)
    xb = torch.empty(N, D, device="cuda")
    for s in range(0, N, 1 << 20):
        e = min(N, s + (1 << 20))
        xb[s:e] = torch.nn.functional.normalize(torch.randn(e - s, D, device="cuda", generator=g), dim=1)
    norms = torch.cat([(xb[s:s + (1 << 20)] ** 2).sum(1) for s in range(0, N, 1 << 20)])
    ptr, terms, tfs, dl = columns(N, g)
    avgdl = float(dl.float().mean())
    k, depth = 3, 16
    for nq in (1, 256):
        xq = torch.nn.functional.normalize(torch.randn(nq, D, device="cuda", generator=g), dim=1)
        qt, qw = queries(nq, g)
        mode = torch.full((nq,), 2, dtype=torch.int32, device="cuda")
        base = None

        def emit(arm, what, med, lo, hi):
            nonlocal base
            base = med if base is None else base
            rows_out.append({"arm": arm, "what": what, "N": N, "entries": int(terms.numel()), "nq": nq, "k": k,
                             "us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                             "x_a": round(med / base, 3)})
            print(json.dumps(rows_out[-1]), flush=True)

        def hybrid(i):
            _, Id = ops.knn(xb, norms, xq, depth, False, 0)
            _, Il = ops.bm25_topk(ptr, terms, tfs, dl, qt, qw, depth, avgdl)
            return ops.rank_fuse(Id, Il, mode, k)

        emit("a", "knn", *_events(lambda i: ops.knn(xb, norms, xq, k, False, 0)))
        emit("b", "bm25_topk", *_events(lambda i: ops.bm25_topk(ptr, terms, tfs, dl, qt, qw, k, avgdl)))
        emit("c", "hybrid: knn + bm25_topk (depth 16) + rank_fuse", *_events(hybrid))
    del xb, norms, ptr, terms, tfs, dl
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--big", action="store_true", help="also N = 10M (15 GB of fp32 vectors)")
    a = ap.parse_args()
    assert ops.load_native()
    rows = []
    with torch.inference_mode():
        for N in [a.n] + ([10_000_000] if a.big else []):
            bench(N, rows)
    print("\n%-4s %-48s %9s %10s %4s %3s %11s %11s %11s %8s" % (
        "arm", "what", "N", "entries", "nq", "k", "median", "min", "max", "x arm a"))
    for r in rows:
        print("%-4s %-48s %9d %10d %4d %3d %8.1f us %8.1f us %8.1f us %7.3fx" % (
            r["arm"], r["what"], r["N"], r["entries"], r["nq"], r["k"], r["us"], r["min_us"], r["max_us"], r["x_a"]))


if __name__ == "__main__":
    main()
