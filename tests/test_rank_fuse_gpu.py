"""``ops.rank_fuse`` on the GPU (csrc/kernels/lexical.hip, one wave per query) against an
exact-rational oracle (``fractions.Fraction``) written out here: ids must be equal, F within
one fp32 rounding of the fraction."""
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    return ops


def oracle(a, b, mode, k, c=60):
    score = {}
    for use, ids in ((mode != 1, a), (mode != 0, b)):
        for pos, i in enumerate(ids if use else ()):
            if i >= 0:
                score[i] = score.get(i, Fraction(0)) + Fraction(1, c + pos + 1)
    top = sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))[:k]
    return [i for i, _ in top] + [-1] * (k - len(top)), [s for _, s in top]


def make_lists(nq, L, seed, base=0):
    """Per query one of: disjoint, identical, partly overlapping lists, with -1 tails of
    random length; ids spread over 64 bits."""
    rng = np.random.default_rng(seed)
    A = np.full((nq, L), -1, np.int64)
    B = np.full((nq, L), -1, np.int64)
    for q in range(nq):
        la, lb = int(rng.integers(1, L + 1)), int(rng.integers(1, L + 1))
        pool = rng.permutation(3 * L) + base
        kind = q % 3
        if kind == 0:
            a, b = pool[:la], pool[L:L + lb]
        elif kind == 1:
            a = b = pool[:min(la, lb)]
        else:
            a, b = pool[:la], rng.permutation(pool[: 2 * L])[:lb]
        A[q, : len(a)], B[q, : len(b)] = a, b
    return A, B


def check(native, A, B, modes, k, c=60):
    F, I = native.rank_fuse(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(),
                            torch.tensor(modes, dtype=torch.int32).cuda(), k, c)
    assert F.is_cuda and F.dtype == torch.float32 and I.dtype == torch.int64 and F.shape == I.shape == (len(modes), k)
    F, I = F.cpu().numpy(), I.cpu().numpy()
    for q, m in enumerate(modes):
        ids, scores = oracle(A[q].tolist(), B[q].tolist(), m, k, c)
        assert I[q].tolist() == ids, (q, m)
        for j, s in enumerate(scores):
            exact = float(s)
            assert abs(float(F[q, j]) - exact) <= 2.0 ** -24 * exact, (q, j)
        assert (F[q, len(scores):] == 0).all()
    return I


@pytest.mark.parametrize("nq", [1, 33, 70])
@pytest.mark.parametrize("L", [1, 16, 64])
def test_rank_fuse_matches_fractions(native, nq, L):
    A, B = make_lists(nq, L, seed=nq * 100 + L, base=(1 << 40) if L == 16 else 0)
    modes = [(2, 0, 1, 2, 2)[q % 5] for q in range(nq)]         # every mode in one batch
    for k in (1, 3, 10, 64):
        check(native, A, B, modes, k)
    check(native, A, B, modes, 10, c=0)


def test_rank_fuse_rational_tie_goes_to_the_lower_id(native):
    """Ranks (12, 30) and (20, 20) both give 1/40 at c = 60; in fp32, 1/72 + 1/90 and 1/80 + 1/80
    need not be equal, so only exact compares order them by id."""
    assert Fraction(1, 72) + Fraction(1, 90) == Fraction(1, 80) + Fraction(1, 80) == Fraction(1, 40)
    a = np.arange(1000, 1064, dtype=np.int64)
    b = np.arange(2000, 2064, dtype=np.int64)
    rows_a, rows_b = [], []
    for lo, hi in ((100, 900), (900, 100)):      # whichever pair holds the lower id wins
        x, y = a.copy(), b.copy()
        x[11], y[29] = hi, hi
        x[19], y[19] = lo, lo
        rows_a.append(x)
        rows_b.append(y)
        x, y = a.copy(), b.copy()
        x[11], y[29] = lo, lo
        x[19], y[19] = hi, hi
        rows_a.append(x)
        rows_b.append(y)
    I = check(native, np.stack(rows_a), np.stack(rows_b), [2] * 4, 5)
    for q in range(4):
        assert I[q, :2].tolist() == [100, 900]
