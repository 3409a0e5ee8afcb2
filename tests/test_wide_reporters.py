"""Host routing of tensors with more than 8192 reporters (no GPU): coordinate containers are never densified beyond
M_COO_NARROW, the coordinate route holds M <= 65535, and the self-reporter mask's coordinate lists keep the reader's order."""
import numpy as np
import pytest

from vimure_amd import tensor as vt
from vimure_amd._io import self_reporter_coo
from vimure_amd.tensor import M_COO_MAX, SparseTensor, engine_data, is_sparse_like


def _no_dense(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("dense conversion called for a wide coordinate container")
    monkeypatch.setattr(vt, "to_dense_u8", boom)


def _wide(M=9000, N=9000, n=500, seed=0, vmax=300):
    g = np.random.RandomState(seed)
    i = g.randint(0, N, n)
    j = (i + 1 + g.randint(0, N - 1, n)) % N
    m = np.where(g.rand(n) < 0.5, i, j)
    l = np.zeros(n, np.int64)
    key = np.unique(np.ravel_multi_index((l, i, j, m), (1, N, N, M)))
    l, i, j, m = np.unravel_index(key, (1, N, N, M))
    v = 1 + g.randint(0, vmax, len(key))
    v[0] = vmax
    return SparseTensor((l, i, j, m), v, shape=(1, N, N, M))


def test_wide_container_goes_to_the_coordinate_route_as_it_is(monkeypatch):
    _no_dense(monkeypatch)
    X = _wide()
    assert int(X.vals.max()) == 300
    assert engine_data(X) is X


def test_wide_container_drops_explicit_zeros_instead_of_densifying(monkeypatch):
    _no_dense(monkeypatch)
    X = _wide(vmax=200)
    v = np.array(X.vals)
    v[[3, 10]] = 0
    Xz = SparseTensor(X.subs, v, shape=X.shape)
    out = engine_data(Xz)
    assert is_sparse_like(out) and tuple(out.shape) == tuple(X.shape)
    keep = v != 0
    assert len(out.vals) == len(v) - 2 and int(np.asarray(out.vals).min()) >= 1
    for a, b in zip(out.subs, X.subs):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b)[keep])
    np.testing.assert_array_equal(np.asarray(out.vals), v[keep])


def test_narrow_container_with_zeros_is_densified_as_before():
    X = _wide(M=64, N=12, n=40, vmax=5)
    v = np.array(X.vals)
    v[0] = 0
    out = engine_data(SparseTensor(X.subs, v, shape=X.shape))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (1, 12, 12, 64)


def test_m_beyond_the_coordinate_limit_is_rejected_naming_it():
    assert M_COO_MAX == 65535
    X = SparseTensor((np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.int64), np.full(1, 65535)), np.ones(1),
                     shape=(1, 2, 2, 65536))
    with pytest.raises(ValueError, match="65535"):
        engine_data(X)


def test_wide_dense_counts_are_refused_but_the_same_container_is_taken(monkeypatch):
    """A dense array with counts above 255 and M > 8192 is refused as before; the same tensor as a coordinate container goes to
    the coordinate route."""
    A = np.full((1, 2, 2, 9000), 300, np.int64)
    with pytest.raises(ValueError, match="M <= 8192"):
        engine_data(A)
    _no_dense(monkeypatch)
    X = SparseTensor.fromarray(A)
    assert engine_data(X) is X


def _self_reporter_loop(L, N, reporter_ids):
    """The reader's self-reporter mask, one reporter at a time (a plain restatement of the reference's loop)."""
    rep = np.asarray(sorted(reporter_ids), dtype=np.int64)
    others = np.arange(N, dtype=np.int64)
    subs = [[], [], [], []]
    for l in range(L):
        for r in rep:
            o = others[others != r]
            i = np.concatenate([np.full(N - 1, r), o])
            j = np.concatenate([o, np.full(N - 1, r)])
            order = np.lexsort((j, i))
            subs[0].append(np.full(2 * (N - 1), l))
            subs[1].append(i[order])
            subs[2].append(j[order])
            subs[3].append(np.full(2 * (N - 1), r))
    if not subs[0]:
        return tuple(np.zeros(0, np.int64) for _ in range(4))
    return tuple(np.concatenate(s) for s in subs)


@pytest.mark.parametrize("L,N,reporters", [(1, 1, [0]), (2, 2, [1, 0]), (2, 7, [0, 3, 6]), (3, 13, list(range(13))),
                                           (1, 50, [49, 3, 17, 0]), (2, 301, list(range(0, 301, 7))), (1, 5, [])])
def test_self_reporter_coo_matches_the_loop(L, N, reporters):
    got = self_reporter_coo(L, N, reporters)
    want = _self_reporter_loop(L, N, reporters)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
