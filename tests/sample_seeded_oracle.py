"""fp64 oracle for ``ops.sample_tokens``: the oracle of tests/sample_oracle.py plus the ``min_p``
filter, and the inputs the seeded-sampler CPU and GPU tests share.

``min_p`` keeps ``x >= max(x) + log(min_p)`` -- a ratio to the maximum, which survives every other
filter, so it is an intersection with the top-k / top-p set and needs no ordering rule.  ``m_star``
derives a ``min_p`` whose cutoff lies in the middle of a value gap wider than ``M_GAP``, three
orders above the fp32 error of ``max + logf(min_p)`` for |x| up to about 30 (an ulp of 30 is
1.9e-6; logf is good to an ulp of its result, at most 4.8e-7 for min_p >= 1e-3).
"""
from __future__ import annotations

import numpy as np
import torch

from tests.sample_oracle import DELTA, assert_preconditions, case_params, oracle, scaled

M_GAP = 1e-3

# the grid of the uniform tests: seeds x absolute positions
SEEDS = (1, 2 ** 31, 2 ** 32 + 5, 2 ** 63 - 1)
INDICES = (0, 1, 4095, 2 ** 31 - 1)


def to_bf16(row) -> np.ndarray:
    """The row rounded to bf16, as fp32: what a bf16 logits tensor holds."""
    return torch.from_numpy(np.ascontiguousarray(row, dtype=np.float32)).bfloat16().float().numpy()


def m_star(row, inv_temp, target: float) -> float:
    """A ``min_p`` for this row whose cutoff ``max + log(min_p)`` is the midpoint of two
    neighbouring distinct values more than ``M_GAP`` apart; of those the one nearest ``target``.
    Returned rounded to fp32, the value the sampler reads."""
    x = scaled(row, inv_temp)
    xs = np.unique(x)[::-1]                       # distinct values, descending
    gap = xs[:-1] - xs[1:]
    ok = gap > M_GAP
    assert ok.any(), "no min_p cutoff with the margin on this row"
    mid = np.exp(0.5 * (xs[:-1] + xs[1:]) - xs[0])[ok]
    return float(np.float32(mid[np.argmin(np.abs(mid - target))]))


def oracle_min_p(row, inv_temp, top_k, top_p, min_p):
    """``sample_oracle.oracle`` with ``keep &= x >= max(x) + log(min_p)`` in float64 (``min_p`` as
    the fp32 the sampler reads; <= 0: off) -> (keep, cdf, info); ``info['mgap']`` is the distance of
    the cutoff from the nearest value (inf when the filter is off or ``min_p == 1``, whose cutoff
    is the maximum itself, exactly)."""
    keep, cdf, info = oracle(row, inv_temp, top_k, top_p)
    x = info["x"]
    info["mgap"] = np.inf
    mp = float(np.float32(min_p))
    if mp > 0.0:
        cut = x.max() + np.log(min(mp, 1.0))
        keep = keep & (x >= cut)
        if mp < 1.0:
            info["mgap"] = float(np.abs(x - cut).min())
        w = np.where(keep, np.exp(x - x.max()), 0.0)
        cdf = np.cumsum(w)
        cdf /= cdf[-1]
        info["n_keep"] = int(keep.sum())
    return keep, cdf, info


def build_case_min_p(row, case, min_p):
    """One row under a ``CASES`` entry (or explicit parameters) and ``min_p`` (a number, or
    ("m*", target)): resolves the parameters, runs the oracle, asserts the preconditions
    -> ((inv_temp, top_k, top_p, min_p), keep, cdf, info)."""
    it, k, p = case_params(row, case)
    if isinstance(min_p, tuple):
        min_p = m_star(row, it, min_p[1])
    keep, cdf, info = oracle_min_p(row, it, k, p, min_p)
    assert_preconditions(info, k, p, len(row))
    if 0.0 < min_p < 1.0:
        assert info["mgap"] > M_GAP / 4, f"mgap {info['mgap']:.3e} <= {M_GAP / 4:g}"
    return (it, k, p, float(min_p)), keep, cdf, info


__all__ = ["DELTA", "INDICES", "M_GAP", "SEEDS", "build_case_min_p", "m_star", "oracle_min_p", "to_bf16"]
