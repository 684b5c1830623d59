"""fp64 oracle and checker for the temperature / top-k / top-p sampler (``ops.sample``).

``oracle`` computes, in float64, which tokens a row keeps and the CDF of the kept tokens in
vocabulary-index order, plus the margins a test needs to prove that its input is unambiguous
for a sampler that finds its thresholds by a 24-round fp32 bisection.  ``check`` holds a set
of draws against that CDF.  ``p_star`` derives a top-p that has the margins by construction,
and ``make_row`` / ``CASES`` / ``case_params`` are the inputs the CPU and GPU tests share.
"""
from __future__ import annotations

import numpy as np

# Interval slack of ``check``, derived, not measured: each __expf(x - mx) term is good to
# ~3e-6 relative for |x - mx| <= 30 (rounding of the log2(e) product + v_exp_f32); the sums
# are at worst 501 sequential fp32 adds per thread (ceil(128256 / 256)) plus a 256-term
# prefix, <= ~5e-5 of the total mass.  DELTA is twice that bound.
DELTA = 1e-4

VS = (16, 255, 256, 257, 1000, 32000, 128256)

# (inv_temp, top_k, top_p); "V", "V-1", "V+7" are resolved against the row, "p*" by p_star
CASES = (
    (1.0, 0, 1.0),
    (1.25, 40, 1.0),
    (1.25, 0, "p*"),
    (1.25, 40, "p*"),
    (2.0, 5, "p*"),
    (100.0, 0, 1.0),
    (0.5, "V-1", 1.0),
    (1.0, "V", 1.0),
    (1.0, "V+7", 1.0),
)


def scaled(logits_row, inv_temp) -> np.ndarray:
    """The product the kernel forms, float32(logit) * float32(inv_temp), as float64."""
    return (np.asarray(logits_row, dtype=np.float32) * np.float32(inv_temp)).astype(np.float64)


def oracle(logits_row, inv_temp, top_k, top_p):
    """-> (keep [V] bool, cdf [V] float64, info dict).

    top-k (0 < k < V) keeps x >= the k-th largest x, ties included; top-p (0 < p < 1) keeps, of
    the survivors by descending probability, the shortest prefix whose mass is >= p * Z (ties at
    the cutoff value included); ``cdf`` is the cumulative mass of the kept tokens in index order
    over its total.  ``info``: ``res`` the resolution of a 24-round bisection over [min x, max x];
    ``kgap`` the gap between the k-th value and the largest dropped one (the (k+1)-th when the
    k-th is not tied); ``pgap`` the value gap below the top-p cutoff; ``pm_lo`` / ``pm_hi`` the
    distances of p from the cumulative masses just below and at the cutoff, as a share of Z.
    Gaps and margins of an inactive filter are inf.
    """
    x = scaled(logits_row, inv_temp)
    V = x.size
    mx = x.max()
    info = {"res": (mx - x.min()) * 2.0 ** -24, "kgap": np.inf, "pgap": np.inf, "pm_lo": np.inf,
            "pm_hi": np.inf, "x": x}
    keep = np.ones(V, dtype=bool)
    k = int(top_k)
    if 0 < k < V:
        kth = np.partition(x, V - k)[V - k]
        keep = x >= kth
        if not keep.all():
            info["kgap"] = kth - x[~keep].max()
    p = float(top_p)
    if 0.0 < p < 1.0:
        xs = np.sort(x[keep])[::-1]
        cum = np.cumsum(np.exp(xs - mx))
        Z = cum[-1]
        n = int(np.searchsorted(cum, p * Z, side="left"))      # first n with cum[n] >= p * Z
        n = min(n, xs.size - 1)
        keep = keep & (x >= xs[n])
        if n + 1 < xs.size:
            info["pgap"] = xs[n] - xs[n + 1]
        info["pm_lo"] = (p * Z - (cum[n - 1] if n else 0.0)) / Z
        info["pm_hi"] = (cum[n] - p * Z) / Z
    w = np.where(keep, np.exp(x - mx), 0.0)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    info["n_keep"] = int(keep.sum())
    return keep, cdf, info


def p_star(logits_row, inv_temp, top_k, target=0.9, delta=DELTA) -> float:
    """A top-p for this row with the margins ``check``'s callers assert, by construction: the
    midpoint between two consecutive cumulative masses of the (top-k survivors') sorted
    distribution, at a cutoff token whose own probability exceeds 4 * delta and whose value gap
    to the next token exceeds 4 * res; of those cutoffs the one whose midpoint is nearest
    ``target``.  Returned rounded to fp32, the value the sampler reads."""
    x = scaled(logits_row, inv_temp)
    V = x.size
    res = (x.max() - x.min()) * 2.0 ** -24
    k = int(top_k)
    xs = np.sort(x)[::-1]
    if 0 < k < V:
        xs = xs[xs >= xs[k - 1]]
    q = np.exp(xs - xs[0])
    q /= q.sum()
    cum = np.cumsum(q)
    gap = np.append(xs[:-1] - xs[1:], np.inf)
    mid = cum - 0.5 * q
    ok = (q > 4 * delta) & (gap > 4 * res) & (mid < 1.0)
    assert ok.any(), "no top-p cutoff with the margins on this row"
    cand = np.nonzero(ok)[0]
    n = cand[np.argmin(np.abs(mid[cand] - target))]
    return float(np.float32(mid[n]))


def make_row(V: int, seed: int, spread: float = 4.0) -> np.ndarray:
    """LLM-like fp32 logits: randn * spread, so the top tokens carry percent-level mass."""
    return (np.random.default_rng(seed).standard_normal(V) * spread).astype(np.float32)


def penalised_row(V: int, seed: int, n: int = 64) -> np.ndarray:
    """``make_row`` with ``n`` scattered entries lowered by 1e4, as presence_penalty = 1e4 leaves
    the window's tokens."""
    row = make_row(V, seed)
    idx = np.random.default_rng(seed + 7919).choice(V, size=n, replace=False)
    row[idx] -= np.float32(1e4)
    return row


def tied_kth_row(V: int = 1000, seed: int = 3, rank: int = 40, copies: int = 3) -> np.ndarray:
    """``make_row`` with ``copies`` tokens exactly equal at rank ``rank`` (1-based), so a top-k
    of ``rank`` keeps ``rank + copies - 1`` tokens."""
    row = make_row(V, seed)
    order = np.argsort(-row, kind="stable")
    row[order[rank - 1:rank - 1 + copies]] = row[order[rank - 1]]
    return row


def peaked_row(V: int, seed: int, above: float = 50.0, at: int | None = None) -> tuple[np.ndarray, int]:
    """``make_row`` with one logit ``above`` over the maximum of the rest -> (row, its index)."""
    row = make_row(V, seed)
    at = V // 3 if at is None else at
    row[at] = -np.inf
    row[at] = row.max() + np.float32(above)
    return row, at


def case_params(row, case):
    """Resolve a ``CASES`` entry against a row -> (inv_temp, top_k, top_p) as python numbers."""
    it, k, p = case
    V = len(row)
    k = {"V": V, "V-1": V - 1, "V+7": V + 7}.get(k, k)
    if p == "p*":
        p = p_star(row, it, k)
    return float(it), int(k), float(p)


def uniforms(n: int, seed: int) -> np.ndarray:
    """``n`` fp32 values in [0, 1), one per stratum of width 1 / n, in shuffled order."""
    rng = np.random.default_rng(seed)
    u = ((np.arange(n) + rng.random(n)) / n).astype(np.float32)
    return rng.permutation(np.minimum(u, np.float32(1.0 - 2.0 ** -24)))


def build_case(row, case, n_u: int = 256, seed: int = 0):
    """One row under one ``CASES`` entry (or an explicit (inv_temp, top_k, top_p)): resolves the
    parameters, runs the oracle, asserts the preconditions -> (params, u, keep, cdf, info)."""
    params = case_params(row, case)
    keep, cdf, info = oracle(row, *params)
    assert_preconditions(info, params[1], params[2], len(row))
    return params, uniforms(n_u, seed), keep, cdf, info


def assert_preconditions(info, top_k, top_p, V, delta=DELTA):
    """The input is unambiguous for a 24-round bisection sampler with ``delta`` of mass error."""
    if 0 < top_k < V:
        assert info["kgap"] > 4 * info["res"], f"kgap {info['kgap']:.3e} <= 4 res {info['res']:.3e}"
    if 0.0 < top_p < 1.0:
        assert info["pgap"] > 4 * info["res"], f"pgap {info['pgap']:.3e} <= 4 res {info['res']:.3e}"
        assert info["pm_lo"] > 2 * delta, f"pm_lo {info['pm_lo']:.3e} <= 2 delta"
        assert info["pm_hi"] > 2 * delta, f"pm_hi {info['pm_hi']:.3e} <= 2 delta"


def check(tokens, u, keep, cdf, delta=DELTA) -> float:
    """Every draw ``tokens[i]`` at ``u[i]`` is a kept token and
    ``cdf[tok - 1] - delta <= u < cdf[tok] + delta`` (``cdf[-1] = 0``).  No draw is left out.
    Returns the largest distance of a ``u`` from its token's exact interval (0.0 when every draw
    is inside), the overshoot that ``delta`` allows for."""
    tokens = np.asarray(tokens).astype(np.int64).reshape(-1)
    u = np.asarray(u, dtype=np.float32).astype(np.float64).reshape(-1)
    assert tokens.shape == u.shape
    V = keep.size
    assert ((tokens >= 0) & (tokens < V)).all(), f"token out of range: {tokens[(tokens < 0) | (tokens >= V)][:8]}"
    bad = ~keep[tokens]
    assert not bad.any(), (f"{int(bad.sum())} of {tokens.size} draws returned a dropped token, "
                           f"e.g. token {tokens[bad][0]} at u={u[bad][0]:.6f}")
    lo = np.where(tokens > 0, cdf[np.maximum(tokens - 1, 0)], 0.0)
    hi = cdf[tokens]
    over = np.maximum(np.maximum(lo - u, u - hi), 0.0)
    over = np.where((u >= lo) & (u < hi), 0.0, over)
    bad = ~((lo - delta <= u) & (u < hi + delta))
    assert not bad.any(), (f"{int(bad.sum())} of {tokens.size} draws outside their CDF interval by more than "
                           f"{delta:g}: e.g. token {tokens[bad][0]} at u={u[bad][0]:.6f}, interval "
                           f"[{lo[bad][0]:.6f}, {hi[bad][0]:.6f}); worst {over.max():.3e}")
    return float(over.max()) if over.size else 0.0
