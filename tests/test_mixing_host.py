"""No GPU: the NumPy restatement of the mixing contract (tests/mixing_util.py) against plain loops and exact enumeration, every
ratio of `mixing.MixingStats` against exact rational arithmetic and networkx, the handling of node labels, and the inputs of the
GPU test "sampling agrees with expectation" checked on the host reference of the sampler before a GPU sees them."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

from tests.mixing_util import (SAMPLING_CASE, check_sampling_against_expectation, expected_mixing_np, mixing_np,
                               sampling_case_inputs)

U = 2.0 ** -53


def _random_samples(seed, S, L, N, p=0.4):
    g = np.random.RandomState(seed)
    return (g.rand(S, L, N, N) < p).astype(np.uint8) * g.randint(1, 4, (S, L, N, N)).astype(np.uint8)


@pytest.mark.parametrize("skip", [True, False])
def test_mixing_np_against_plain_loops(skip):
    S, L, N, C = 3, 2, 7, 3
    Ys = _random_samples(5, S, L, N)
    groups = np.array([0, 1, 2, -1, 0, 1, 2])
    assert all(Ys[:, l, np.arange(N), np.arange(N)].any() for l in range(L))
    got = mixing_np(Ys, groups, C, skip)
    mix, mut, ov = np.zeros((S, L, C, C), np.int64), np.zeros((S, L, C, C), np.int64), np.zeros((S, L, L), np.int64)
    for s in range(S):
        for i in range(N):
            for j in range(N):
                if skip and i == j:
                    continue
                for l in range(L):
                    if Ys[s, l, i, j] > 0:
                        if groups[i] >= 0 and groups[j] >= 0:
                            mix[s, l, groups[i], groups[j]] += 1
                            if Ys[s, l, j, i] > 0:
                                mut[s, l, groups[i], groups[j]] += 1
                        for l2 in range(L):
                            if Ys[s, l2, i, j] > 0:
                                ov[s, l, l2] += 1
    assert mix.sum() > 0 and mut.sum() > 0 and ov[:, 0, 1].sum() > 0
    assert np.array_equal(got["mix"], mix) and np.array_equal(got["mutual"], mut) and np.array_equal(got["overlap"], ov)
    assert np.array_equal(got["mutual"], got["mutual"].transpose(0, 1, 3, 2))
    only = mixing_np(Ys, None, 0, skip)
    assert only["mix"].shape == (S, L, 0, 0) and np.array_equal(only["overlap"], ov)


@pytest.mark.parametrize("skip", [True, False])
def test_expected_mixing_np_against_exact_enumeration(skip):
    """L = 2, N = 2, K = 2: all 2^8 networks with their probabilities under q(Y) = prod rho.  The one place where the contract is
    not the expectation of the count: a kept self-loop counts once in `mutual` (probability p_ii) and enters as p_ii^2."""
    L, N, K, C = 2, 2, 2, 2
    g = np.random.RandomState(3)
    rho = g.rand(L, N, N, K)
    rho /= rho.sum(-1, keepdims=True)
    p = rho[..., 1]
    groups = np.array([0, 1])
    want = {k: 0.0 for k in ("mix", "mutual", "overlap")}
    for bits in itertools.product((0, 1), repeat=L * N * N):
        Y = np.array(bits, np.uint8).reshape(L, N, N)
        pr = np.prod(np.where(Y > 0, p, 1.0 - p))
        c = mixing_np([Y], groups, C, skip)
        for k in want:
            want[k] = want[k] + pr * c[k][0]
    got = expected_mixing_np(rho, groups, C, skip)
    if not skip:
        for l in range(L):
            for i in range(N):
                want["mutual"][l, groups[i], groups[i]] -= p[l, i, i] * (1.0 - p[l, i, i])
    for k in want:
        assert (want[k] > 0).any()
        np.testing.assert_allclose(got[k], want[k], rtol=1e-13, atol=1e-15, err_msg=k)   # 256 terms of 9 factors: < 3000 roundings


def _stats(Ys, groups, C, skip, labels=None):
    from vimure_amd.mixing import MixingStats
    return MixingStats(Ys.shape[2], mixing_np(Ys, groups, C, skip), codes=groups, labels=labels, skip_diagonal=skip)


def _frac(n, d):
    return float(Fraction(int(n), int(d))) if d else np.nan


def _close(got, want, tol):
    if np.isnan(want):
        assert np.isnan(got)
    else:
        assert abs(got - want) <= tol, (got, want, tol)


@pytest.mark.parametrize("skip", [True, False])
def test_ratios_against_rational_arithmetic(skip):
    S, L, N, C = 4, 2, 9, 4
    Ys = _random_samples(11, S, L, N, p=0.3)
    Ys[3, 1] = 0                                       # a sample without edges: every ratio is NaN there
    groups = np.array([0, 1, 2, 0, 1, 2, 0, -1, 1])   # group 3 is empty: its ratios are NaN
    st = _stats(Ys, groups, C, skip)
    assert np.array_equal(st.group_sizes, [3, 3, 2, 0])
    mix, mut, ov = st.mix, st.mutual, st.overlap
    n = [int(x) for x in st.group_sizes]
    for s in range(S):
        for l in range(L):
            m = [[int(x) for x in row] for row in mix[s, l]]
            tot = sum(map(sum, m))
            internal = sum(m[a][a] for a in range(C))
            _close(st.ei_index[s, l], _frac(tot - 2 * internal, tot), 2 * U)            # exact integers, one division
            if tot:
                ab = sum(Fraction(sum(m[a]), tot) * Fraction(sum(m[b][a] for b in range(C)), tot) for a in range(C))
                r = (Fraction(internal, tot) - ab) / (1 - ab) if ab != 1 else None
            else:
                r = None
            if r is None:
                assert np.isnan(st.assortativity[s, l])
            else:
                # at most 4 C^2 rounded operations on quantities bounded by 1, then the division
                assert abs(st.assortativity[s, l] - float(r)) <= 8 * C * C * U / float(1 - ab)
            for a in range(C):
                _close(st.within_share[s, l, a], _frac(m[a][a], sum(m[a])), 2 * U)
                for b in range(C):
                    pairs = n[a] * n[b] - (n[a] if (skip and a == b) else 0)
                    _close(st.block_density[s, l, a, b], _frac(m[a][b], pairs), 2 * U)
                    _close(st.block_reciprocity[s, l, a, b], _frac(mut[s, l, a, b], m[a][b]), 2 * U)
            for l2 in range(L):
                e1, e2, o = int(ov[s, l, l]), int(ov[s, l2, l2]), int(ov[s, l, l2])
                _close(st.jaccard[s, l, l2], _frac(o, e1 + e2 - o), 2 * U)
    assert np.isnan(st.assortativity[3, 1]) and np.isnan(st.jaccard[3, 1, 1]) and np.isnan(st.within_share[0, 0, 3])
    assert not np.isnan(st.assortativity[:3]).any()
    assert len(st.summary()) == L * len(st.statistics())
    fr = st.frame()
    assert list(fr.columns[:4]) == ["layer", "from", "to", "mean"] and len(fr) == L * C * C
    assert fr["mean"][0] == mix[:, 0, 0, 0].mean()


def test_assortativity_against_networkx():
    import networkx as nx
    S, L, N, C = 3, 2, 12, 3
    Ys = _random_samples(21, S, L, N, p=0.25)
    groups = np.arange(N) % C
    groups[5] = -1
    st = _stats(Ys, groups, C, True)
    for s in range(S):
        for l in range(L):
            G = nx.DiGraph()
            G.add_nodes_from((i, {"g": int(groups[i])}) for i in range(N) if groups[i] >= 0)
            G.add_edges_from((i, j) for i in range(N) for j in range(N)
                             if i != j and Ys[s, l, i, j] > 0 and groups[i] >= 0 and groups[j] >= 0)
            e = st.mix[s, l] / st.mix[s, l].sum()
            ab = float((e.sum(1) * e.sum(0)).sum())
            want = nx.attribute_assortativity_coefficient(G, "g")
            assert abs(st.assortativity[s, l] - want) <= 2 * 8 * C * C * U / (1.0 - ab)


def test_label_handling():
    import pandas as pd
    from vimure_amd.mixing import encode_groups, groups_from_frame
    codes, labels = encode_groups(["b", "a", None, "b", float("nan"), "c"], 6)
    assert list(labels) == ["a", "b", "c"] and list(codes) == [1, 0, -1, 1, -1, 2] and codes.dtype == np.int32
    codes, labels = encode_groups(np.array([3.0, np.nan, 1.0, 3.0]), 4)
    assert list(labels) == [1.0, 3.0] and list(codes) == [1, -1, 0, 1]
    codes, labels = encode_groups([7, 7, 2], 3)
    assert list(labels) == [2, 7] and list(codes) == [1, 1, 0]
    names = ["n%d" % i for i in range(5)]
    codes, labels = encode_groups({"n3": "x", "n0": "y", "n4": None}, 5, names)
    assert list(labels) == ["x", "y"] and list(codes) == [1, -1, -1, 0, -1]
    codes2, labels2 = encode_groups(pd.Series({"n3": "x", "n0": "y"}), 5, names)
    assert list(codes2) == list(codes) and list(labels2) == list(labels)
    codes, labels = encode_groups({2: "u", 0: "v"}, 3)               # without names the keys are the nodes' indices
    assert list(codes) == [1, -1, 0]
    with pytest.raises(ValueError, match="n9"):
        encode_groups({"n9": "x"}, 5, names)
    with pytest.raises(ValueError, match="labels"):
        encode_groups(["a", "b"], 3)
    codes, labels = encode_groups([None, None], 2)
    assert list(codes) == [-1, -1] and len(labels) == 0
    meta = pd.DataFrame({"pid": ["n1", "n0"], "caste": ["OBC", "SC"], "gender": [1, 2]})
    assert groups_from_frame(meta, "caste") == {"n1": "OBC", "n0": "SC"}
    assert groups_from_frame(meta, "gender", id="pid") == {"n1": 1, "n0": 2}
    with pytest.raises(ValueError, match="religion"):
        groups_from_frame(meta, "religion")


def test_sampling_case_holds_on_the_host_reference():
    """The fixed seeds of tests/test_hip_mixing.py::test_sampling_agrees_with_expectation, on the host reference of the sampler
    (tests/draws_ref.sample_ref) and the NumPy restatements: every bin compared lies within 5 standard errors."""
    from tests.draws_ref import sample_ref
    c = SAMPLING_CASE
    X, st, groups = sampling_case_inputs()
    rho = st[-1]
    counts = mixing_np([sample_ref(rho, c["seed"] + s, 1) for s in range(c["S"])], groups, c["C"], True)
    expected = expected_mixing_np(rho, groups, c["C"], True)
    n = check_sampling_against_expectation(counts, expected, counts)
    assert n == 2 * c["L"] * c["C"] ** 2 + c["L"] ** 2            # every bin of the three tables is large enough to be compared
