"""Scoped exact search (``ops.knn_scoped``, csrc/kernels/knn.hip SCOPED) against the unscoped
kernel and against the host-side patient lookup it replaces.

d = 384, fp32 and bf16 storage, N = 1M (and 10M with --big), k = 3 and 10, nq = 1 / 32 / 256.
Row tags come in contiguous runs of 32 rows (a document's chunks are appended together), every
eighth run is the knowledge base (tag 0); row days are scattered over 1000 values.  Arms:

  a  ``ops.knn``, unscoped
  b  ``ops.knn_scoped`` with the any-scope row
  c  one patient (32 rows) per query, distinct patients across the batch
  d  as c plus the knowledge base (alt_tag 0: an eighth of the rows)
  e  any tag, a date window about 10 % of the (scattered) rows pass
  f  the host way of c, as ``SemanticIndexer.patient_snippets`` does it: a host row list ->
     ``index_select`` -> torch distance -> ``argsort().tolist()``, once (nq = 1) or serially per
     query; host clock, it ends in its own device-to-host copy

The vectors (>= 768 MB) are far larger than the 256 MB last-level cache, so every full scan
streams from HBM.  The small working sets are rotated past it instead: arms c / d / f take other
patients on every call, and the tag / day columns (8 MB at 1M rows) rotate through copies that
total more than 256 MB.  Arms a-e: device events around ITERS calls, median of WINDOWS windows,
launch gaps included.

python benchmarks/bench_knn_scoped.py [--big] [--n 1000000] -> one JSON line per measurement,
then a table."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

D = 384
RUN = 32
WINDOWS, ITERS = 5, 6
IMIN, IMAX = -(1 << 31), (1 << 31) - 1


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


def _host(fn):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for w in range(WINDOWS):
        t0 = time.perf_counter()
        for i in range(ITERS):
            fn(3 + w * ITERS + i)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6 / ITERS)
    return statistics.median(ts), min(ts), max(ts)


def bench(N, dtype, rows_out):
    g = torch.Generator(device="cuda").manual_seed(1)
    xb = torch.empty(N, D, device="cuda", dtype=dtype)
    for s in range(0, N, 1 << 20):       # chunks: no N x d fp32 temporary at 10M rows
        e = min(N, s + (1 << 20))
        xb[s:e] = torch.nn.functional.normalize(torch.randn(e - s, D, device="cuda", generator=g), dim=1).to(dtype)
    norms = torch.cat([(xb[s:s + (1 << 20)].float() ** 2).sum(1) for s in range(0, N, 1 << 20)])
    runs = (N + RUN - 1) // RUN
    run_tag = torch.arange(1, runs + 1, dtype=torch.int32, device="cuda")
    run_tag[7::8] = 0
    tags0 = run_tag.repeat_interleave(RUN)[:N].contiguous()
    days0 = torch.randint(0, 1000, (N,), device="cuda", generator=g, dtype=torch.int32)
    copies = max(2, (272 << 20) // (8 * N) + 1)
    cols = [(tags0.clone(), days0.clone()) for _ in range(copies)]
    patients = run_tag[run_tag > 0].cpu()            # tags of the patient runs, in row order
    npat = len(patients)
    for nq in (1, 32, 256):
        xq = torch.nn.functional.normalize(torch.randn(nq, D, device="cuda", generator=g), dim=1)

        def scope_set(kind):
            """A scope tensor per call, over distinct patients / windows."""
            out = []
            for i in range(3 + WINDOWS * ITERS):
                pt = patients[(torch.arange(nq) * 97 + i * 256 * 97) % npat].tolist()
                if kind == "any":
                    rows = [(-1, -1, IMIN, IMAX)] * nq
                elif kind == "patient":
                    rows = [(t, -1, IMIN, IMAX) for t in pt]
                elif kind == "patient_kb":
                    rows = [(t, 0, IMIN, IMAX) for t in pt]
                else:
                    lo = (i * 37) % 900
                    rows = [(-1, -1, lo, lo + 99)] * nq
                out.append(torch.tensor(rows, dtype=torch.int32, device="cuda").reshape(nq, 4))
            return out

        for k in (3, 10):
            base = None

            def emit(arm, what, med, lo, hi, clock):
                nonlocal base
                base = med if base is None else base
                rows_out.append({"arm": arm, "what": what, "N": N, "storage": str(dtype).split(".")[-1], "nq": nq,
                                 "k": k, "us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                                 "x_a": round(med / base, 3), "clock": clock})
                print(json.dumps(rows_out[-1]), flush=True)

            emit("a", "knn unscoped", *_events(lambda i: ops.knn(xb, norms, xq, k, False, 0)), "device")
            for arm, kind, what in (("b", "any", "scoped, any-scope"), ("c", "patient", "scoped, one patient"),
                                    ("d", "patient_kb", "scoped, patient + KB"),
                                    ("e", "window", "scoped, 10 % date window")):
                sc = scope_set(kind)
                emit(arm, what, *_events(lambda i: ops.knn_scoped(xb, norms, *cols[i % copies], xq, sc[i], k, False, 0)),
                     "device")

            def host_lookup(i):
                res = []
                for q in range(nq):
                    r0 = ((q * 97 + i * 256 * 97) % (runs - 1)) * RUN
                    ids = torch.tensor(list(range(r0, r0 + RUN)), device="cuda")
                    x = xb.index_select(0, ids).float()
                    dist = ((x - xq[q:q + 1]) ** 2).sum(1)
                    res.append(dist.argsort().tolist()[:k])
                return res

            emit("f", "host list + index_select + argsort x nq", *_host(host_lookup), "host")
    del xb, norms, cols
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
            for dtype in (torch.float32, torch.bfloat16):
                bench(N, dtype, rows)
    print("\n%-4s %-42s %9s %8s %4s %3s %11s %11s %11s %8s" % (
        "arm", "what", "N", "storage", "nq", "k", "median", "min", "max", "x arm a"))
    for r in rows:
        print("%-4s %-42s %9d %8s %4d %3d %8.1f us %8.1f us %8.1f us %7.3fx  (%s clock)" % (
            r["arm"], r["what"], r["N"], r["storage"], r["nq"], r["k"], r["us"], r["min_us"], r["max_us"], r["x_a"],
            r["clock"]))


if __name__ == "__main__":
    main()
