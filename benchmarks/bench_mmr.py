"""What ``search_type=mmr`` costs: the MMR re-selection (``ops.mmr_select``,
csrc/kernels/mmr.hip) beside the dense scan it follows, and against the host way.

N = 1M unit rows (fp32), d = 384 and 768, nq = 1 / 32 / 256.  Arms:

  a   ``ops.knn`` at depth 3                                  (what a plain request runs)
  b   ``ops.knn`` at depth 20 and at depth 64                 (what fetching deeper costs)
  c   ``ops.mmr_select`` alone, F = 20 / 64 candidates, k = 3 / 10, lambda_mult 0.5
  d   the host way on the same candidates: one ``index_select`` of the batch's candidate rows,
      the cosine matrices by two torch ``bmm``, one ``.tolist()``, then LangChain's greedy loop
      in Python per question.  HOST CLOCK (the loop is host work), one synchronize per call.

Arms a-c: device events around ITERS calls, median of WINDOWS windows, launch gaps included.

python benchmarks/bench_mmr.py [--n 1000000] -> one JSON line per measurement, then a table."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

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


def _host(fn, iters):
    fn(0)
    torch.cuda.synchronize()
    ts = []
    for w in range(WINDOWS):
        t0 = time.perf_counter()
        for i in range(iters):
            fn(i)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6 / iters)
    return statistics.median(ts), min(ts), max(ts)


def host_mmr(xb, xq, cand, lam, k):
    """LangChain's maximal_marginal_relevance per question, the matrices made on the device."""
    nq, F = cand.shape
    rows = xb.index_select(0, cand.reshape(-1)).reshape(nq, F, -1)
    rn = rows / rows.norm(dim=2, keepdim=True).clamp_min(1e-30)
    qn = xq / xq.norm(dim=1, keepdim=True).clamp_min(1e-30)
    rel = torch.bmm(rn, qn[:, :, None])[:, :, 0].tolist()
    sim = torch.bmm(rn, rn.transpose(1, 2)).tolist()
    ids = cand.tolist()
    out = []
    for q in range(nq):
        r, s = rel[q], sim[q]
        best = max(range(F), key=r.__getitem__)
        sel = [best]
        while len(sel) < k:
            bs, bi = -2.0, -1
            for i in range(F):
                if i in sel:
                    continue
                red = max(s[i][j] for j in sel)
                sc = lam * r[i] - (1 - lam) * red
                if sc > bs:
                    bs, bi = sc, i
            sel.append(bi)
        out.append([ids[q][i] for i in sel])
    return out


def bench(N, d, rows_out):
    g = torch.Generator(device="cuda").manual_seed(1)
    xb = torch.empty(N, d, device="cuda")
    for s in range(0, N, 1 << 19):
        e = min(N, s + (1 << 19))
        xb[s:e] = torch.nn.functional.normalize(torch.randn(e - s, d, device="cuda", generator=g), dim=1)
    norms = torch.cat([(xb[s:s + (1 << 19)] ** 2).sum(1) for s in range(0, N, 1 << 19)])
    for nq in (1, 32, 256):
        xq = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda", generator=g), dim=1)
        base = None

        def emit(arm, what, clock, med, lo, hi):
            nonlocal base
            base = med if base is None else base
            rows_out.append({"arm": arm, "what": what, "clock": clock, "N": N, "d": d, "nq": nq,
                             "us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                             "x_a": round(med / base, 3)})
            print(json.dumps(rows_out[-1]), flush=True)

        emit("a", "knn depth 3", "device", *_events(lambda i: ops.knn(xb, norms, xq, 3, False, 0)))
        for depth in (20, 64):
            emit("b", f"knn depth {depth}", "device", *_events(lambda i: ops.knn(xb, norms, xq, depth, False, 0)))
        _, C64 = ops.knn(xb, norms, xq, 64, False, 0)
        lam = torch.full((nq,), 0.5, device="cuda")
        for F in (20, 64):
            cand = C64[:, :F].contiguous()
            ncand = torch.full((nq,), F, dtype=torch.int32, device="cuda")
            for k in (3, 10):
                emit("c", f"mmr_select F={F} k={k}", "device",
                     *_events(lambda i: ops.mmr_select(xb, norms, xq, cand, ncand, lam, k)))
                emit("d", f"host way F={F} k={k}", "host",
                     *_host(lambda i: host_mmr(xb, xq, cand, 0.5, k), 6 if nq == 1 else 2 if nq == 32 else 1))
    del xb, norms
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    assert ops.load_native()
    rows = []
    with torch.inference_mode():
        for d in (384, 768):
            bench(a.n, d, rows)
    print("\n%-4s %-24s %-6s %8s %4s %4s %11s %11s %11s %8s" % (
        "arm", "what", "clock", "N", "d", "nq", "median", "min", "max", "x arm a"))
    for r in rows:
        print("%-4s %-24s %-6s %8d %4d %4d %8.1f us %8.1f us %8.1f us %7.3fx" % (
            r["arm"], r["what"], r["clock"], r["N"], r["d"], r["nq"], r["us"], r["min_us"], r["max_us"], r["x_a"]))


if __name__ == "__main__":
    main()
