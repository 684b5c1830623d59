"""The sampler's fp64 oracle and checker (tests/sample_oracle.py) on the CPU: the oracle on
hand-computed rows, ``reference.sample`` through ``check`` on the case matrix the GPU tests
run, deliberately wrong samplers that ``check`` must reject, and the reference's contracts
(``top_k == 1`` is an argmax, a dropped token is never returned)."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from docqa_amd.ops import reference as R
from tests.sample_oracle import (CASES, DELTA, assert_preconditions, build_case, check, make_row, oracle,
                                 peaked_row, penalised_row, tied_kth_row)

CPU_VS = (16, 255, 256, 257, 1000, 32000)


def _ref(row, params, u):
    """reference.sample of one row at every u -> tokens."""
    it, k, p = params
    n = len(u)
    logits = torch.from_numpy(np.asarray(row, dtype=np.float32)).expand(n, -1)
    return R.sample(logits, torch.full((n,), it), torch.full((n,), k, dtype=torch.int32),
                    torch.full((n,), p), torch.from_numpy(np.asarray(u, dtype=np.float32))).numpy()


# ---- the oracle itself ---------------------------------------------------------------------

def test_oracle_hand_computed_row():
    # probabilities 0.1, 0.4, 0.2, 0.3 at inv_temp 1
    row = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    keep, cdf, info = oracle(row, 1.0, 0, 1.0)
    assert keep.all() and np.allclose(cdf, [0.1, 0.5, 0.7, 1.0], atol=1e-7)
    keep, cdf, info = oracle(row, 1.0, 2, 1.0)                 # top-2: tokens 1 and 3
    assert keep.tolist() == [False, True, False, True]
    assert np.allclose(cdf, [0, 4 / 7, 4 / 7, 1.0], atol=1e-7)
    assert math.isclose(info["kgap"], math.log(0.3 / 0.2), rel_tol=1e-6)
    keep, cdf, info = oracle(row, 1.0, 0, 0.8)                 # 0.4 + 0.3 < 0.8 <= 0.4 + 0.3 + 0.2
    assert keep.tolist() == [False, True, True, True]
    assert math.isclose(info["pm_lo"], 0.1, abs_tol=1e-6) and math.isclose(info["pm_hi"], 0.1, abs_tol=1e-6)
    assert math.isclose(info["pgap"], math.log(2.0), rel_tol=1e-6)
    keep, cdf, info = oracle(row, 1.0, 3, 0.5)                 # of {1, 3, 2}: 0.4/0.9 < 0.5 <= 0.7/0.9
    assert keep.tolist() == [False, True, False, True]
    keep, cdf, info = oracle(row, 2.0, 0, 1.0)                 # temperature: p ~ (0.01, 0.16, 0.04, 0.09)
    assert np.allclose(cdf, np.cumsum([0.01, 0.16, 0.04, 0.09]) / 0.3, atol=1e-6)
    for k in (4, 11):                                          # k >= V: no top-k
        assert oracle(row, 1.0, k, 1.0)[0].all()


def test_oracle_keeps_ties_at_the_kth_value():
    row = tied_kth_row()
    keep, _, info = oracle(row, 1.25, 40, 1.0)
    assert keep.sum() == 42
    assert_preconditions(info, 40, 1.0, len(row))


def test_check_accepts_the_exact_draw_and_rejects_neighbours():
    row = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    keep, cdf, _ = oracle(row, 1.0, 0, 1.0)
    u = np.array([0.05, 0.1, 0.49999, 0.5, 0.75, 0.99], dtype=np.float32)
    assert check([0, 1, 1, 2, 3, 3], u, keep, cdf) == 0.0
    assert 0 < check([1], [0.09995], keep, cdf) <= DELTA        # inside the slack, and reported
    with pytest.raises(AssertionError):
        check([0, 1, 1, 2, 3, 2], u, keep, cdf)
    with pytest.raises(AssertionError):
        check([1], [0.0995], keep, cdf)
    keep2, cdf2, _ = oracle(row, 1.0, 2, 1.0)
    with pytest.raises(AssertionError, match="dropped"):
        check([2], [0.5], keep2, cdf2)


# ---- reference.sample on the case matrix ---------------------------------------------------

@pytest.mark.parametrize("ci", range(len(CASES)))
@pytest.mark.parametrize("V", CPU_VS)
def test_reference_case_matrix(V, ci):
    row = make_row(V, seed=100 * ci + V)
    params, u, keep, cdf, _ = build_case(row, CASES[ci], seed=ci)
    check(_ref(row, params, u), u, keep, cdf)


def test_reference_u_sweep():
    row = make_row(1000, seed=11)
    params, _, keep, cdf, _ = build_case(row, (1.25, 40, "p*"))
    u = ((np.arange(4096) + 0.5) / 4096).astype(np.float32)
    tok = _ref(row, params, u)
    check(tok, u, keep, cdf)
    mass = np.diff(cdf, prepend=0.0)
    assert set(np.nonzero(keep & (mass > 2 / 4096 + 2 * DELTA))[0]) <= set(tok.tolist()) <= set(np.nonzero(keep)[0])


@pytest.mark.parametrize("case", [(1.25, 40, 1.0), (1.25, 40, "p*")])
def test_reference_penalised_rows(case):
    row = penalised_row(1000, seed=2)     # a seed the asserted preconditions accept
    params, u, keep, cdf, info = build_case(row, case)
    assert info["res"] > 5e-4 and not keep[row < -5e3].any()
    check(_ref(row, params, u), u, keep, cdf)


def test_reference_ties_at_the_kth_value():
    row = tied_kth_row()
    params, u, keep, cdf, _ = build_case(row, (1.25, 40, 1.0))
    check(_ref(row, params, u), u, keep, cdf)


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_reference_peaked_row(ci):
    row, at = peaked_row(1000, seed=ci)
    params, _, keep, cdf, _ = build_case(row, CASES[ci])
    u = ((np.arange(64) + 0.5) / 64).astype(np.float32)
    tok = _ref(row, params, u)
    check(tok, u, keep, cdf)
    assert (tok == at).all()


# ---- the reference's contracts -------------------------------------------------------------

@pytest.mark.parametrize("copies", [2, 3, 200])
def test_reference_top_k_1_is_the_lowest_index_of_the_maximum(copies):
    V = 4096
    row = torch.from_numpy(make_row(V, seed=copies)).bfloat16().float()
    at = np.sort(np.random.default_rng(copies).choice(V, size=copies, replace=False))
    row[torch.from_numpy(at)] = row.max() + 0.125
    for it, p in ((1.0, 1.0), (1.25, 0.9)):
        for u in (0.0, 0.5, 0.999999):
            tok = R.sample(row[None], torch.tensor([it]), torch.tensor([1], dtype=torch.int32), torch.tensor([p]),
                           torch.tensor([u]))
            assert int(tok) == int(at[0]) == int(row.argmax())


def test_reference_never_returns_a_dropped_token():
    row = make_row(1000, seed=21)
    order = np.argsort(-row)
    row[[0, 999]] = row[order[500]]                 # first and last ids: mid-rank, dropped by top-k 40
    keep, cdf, info = oracle(row, 1.25, 40, 1.0)
    assert not keep[0] and not keep[999]
    u = np.array([0.0, np.float32(1 - 2.0 ** -24)], dtype=np.float32)
    tok = _ref(row, (1.25, 40, 1.0), u)
    check(tok, u, keep, cdf)
    assert tok[0] == np.nonzero(keep)[0][0]
    # fp32 cumsum that ends below u: whatever the rounding, the answer is a kept token
    flat = np.zeros(32000, dtype=np.float32)
    flat[-1] = -30.0
    keep, cdf, _ = oracle(flat, 1.0, 31999, 1.0)
    assert not keep[-1]
    tok = _ref(flat, (1.0, 31999, 1.0), u[1:])
    assert keep[tok].all()


# ---- deliberately wrong samplers: check must reject each -----------------------------------

def _np_sampler(row, params, u, *, strict=False, ignore_p=False, drop_temp=False, k_off=0, serial=False):
    """A numpy model of the HIP sampler: exact thresholds, fp32 masses summed in the kernel's
    order (256 contiguous slices, a serial prefix over the slice totals), inverse CDF in index
    order.  The keyword arguments each break one thing."""
    it, k, p = params
    x = np.asarray(row, dtype=np.float32) * np.float32(it)
    V = x.size
    mx = x.max()
    th = -np.inf
    k = k + k_off if 0 < k < V else k
    if 0 < k < V:
        th = np.sort(x)[::-1][k - 1]
    keep = x > th if strict else x >= th
    w = np.exp((x - mx).astype(np.float64)).astype(np.float32)
    if 0.0 < p < 1.0 and not ignore_p:
        xs = np.sort(x[keep])[::-1]
        cum = np.cumsum(np.exp((xs - mx).astype(np.float64)))
        n = min(int(np.searchsorted(cum, np.float64(np.float32(p)) * cum[-1], side="left")), xs.size - 1)
        keep &= x >= xs[n]
    if drop_temp:
        r = np.asarray(row, dtype=np.float32)
        w = np.exp((r - r.max()).astype(np.float64)).astype(np.float32)
    w = np.where(keep, w, np.float32(0))
    per = -(-V // 256)
    wp = np.pad(w, (0, 256 * per - V))
    if serial:
        c = np.cumsum(w, dtype=np.float32)
    else:
        loc = np.cumsum(wp.reshape(256, per), axis=1, dtype=np.float32)
        pre = np.concatenate([[np.float32(0)], np.cumsum(loc[:-1, -1], dtype=np.float32)])
        c = np.maximum.accumulate((pre[:, None] + loc).astype(np.float32).reshape(-1)[:V])
    # the total the draw is scaled by: thread t sums i = t, t + 256, ..., then the 256 partials
    z = np.cumsum(wp.reshape(per, 256), axis=0, dtype=np.float32)[-1].sum(dtype=np.float32)
    target = np.asarray(u, dtype=np.float32) * z
    tok = np.searchsorted(c, target, side="right")
    return np.where(tok >= V, int(np.argmax(x)), tok)


@pytest.mark.parametrize("ci", range(len(CASES)))
@pytest.mark.parametrize("V", [257, 128256])
def test_model_sampler_passes(V, ci):
    """The harness of the rejections below is sound: unbroken, the model passes, at the largest V too."""
    row = make_row(V, seed=100 * ci + V)
    params, u, keep, cdf, _ = build_case(row, CASES[ci], seed=ci)
    check(_np_sampler(row, params, u), u, keep, cdf)


def test_check_rejects_strict_threshold_on_ties():
    row = tied_kth_row()
    params, u, keep, cdf, _ = build_case(row, (1.25, 40, 1.0))
    check(_np_sampler(row, params, u), u, keep, cdf)
    with pytest.raises(AssertionError):
        check(_np_sampler(row, params, u, strict=True), u, keep, cdf)


@pytest.mark.parametrize("case", [(1.25, 0, "p*"), (1.25, 40, "p*"), (2.0, 5, "p*")])
def test_check_rejects_ignored_top_p(case):
    row = make_row(1000, seed=31)
    params, u, keep, cdf, _ = build_case(row, case)
    with pytest.raises(AssertionError):
        check(_np_sampler(row, params, u, ignore_p=True), u, keep, cdf)


@pytest.mark.parametrize("case", [(1.25, 40, 1.0), (2.0, 5, "p*"), (0.5, "V-1", 1.0)])
def test_check_rejects_temperature_dropped_from_the_cdf(case):
    row = make_row(1000, seed=32)
    params, u, keep, cdf, _ = build_case(row, case)
    with pytest.raises(AssertionError):
        check(_np_sampler(row, params, u, drop_temp=True), u, keep, cdf)


@pytest.mark.parametrize("k_off", [-1, 1])
def test_check_rejects_top_k_off_by_one(k_off):
    # a flat row, where the 40th and 41st tokens carry percent-level mass: on a peaked row
    # their mass is below delta and no check of draws can see them
    row = make_row(1000, seed=33, spread=1.0)
    params, u, keep, cdf, _ = build_case(row, (1.25, 40, 1.0))
    check(_np_sampler(row, params, u), u, keep, cdf)
    with pytest.raises(AssertionError):
        check(_np_sampler(row, params, u, k_off=k_off), u, keep, cdf)


def test_check_rejects_one_serial_fp32_cumsum_at_llama_vocab():
    """A single sequential fp32 prefix over V = 128256 (against the total of the block sum) loses
    ~1.9e-4 of the mass on this row, past delta; the chunked sums of the kernel (and of the model
    above) do not."""
    row = make_row(128256, seed=34)
    params, u, keep, cdf, _ = build_case(row, (1.0, 0, 1.0), n_u=1024)
    check(_np_sampler(row, params, u), u, keep, cdf)
    with pytest.raises(AssertionError):
        check(_np_sampler(row, params, u, serial=True), u, keep, cdf)
