"""GPU: the graph read-outs (triads.hip, connectivity.hip, centrality.hip, betweenness.hip, cores.hip) at the launch shapes the
other files do not enter.  The shape comes from N alone (tests/graph_shapes_util.shape_of restates it): N = 513, 1024 and 1025 are
8 and 16 lanes per bit row with one and with two trips of the word stride, three, four and five nodes per thread on the rungs 4
and 8; N = 2048 is the node bound of connectivity; for triads N = 256, 512, 1024 and 2048 are the register path with 4 to 32 words,
N = 2049 and 4097 two and three blocks of 32 words, and 4097 the 64-lane stride with a second trip of the degree loop.
tests/test_graph_shapes_host.py names the classes and holds the designs' preconditions.

Every handle is a coordinate-list handle whose rho is one-hot on the design (tests/graph_shapes_util.design): every sample is the
design whatever the seed, asserted once per handle.  S = 2 samples with VMR_NETSTATS_CHUNK = 1, so that the per-node fold crosses
a chunk boundary.  No tolerance is new: integers are equal, centrality is bit for bit under `exact_ok`, betweenness within the
bound tests/test_hip_betweenness.py derives and exact on the path."""
import numpy as np
import pytest

from tests.betweenness_util import DIRECTIONS as BTW_DIRECTIONS
from tests.centrality_util import DIRECTIONS as CENT_DIRECTIONS
from tests.centrality_util import reduce_values
from tests.connectivity_util import NDIST, connectivity_np
from tests.cores_util import MODES, cores_np
from tests.cores_util import reduce_values as reduce_cores
from tests.graph_shapes_util import (BOUND_N, MAIN_NS, Q, T, TRIAD_FOUR_NS, TRIAD_LARGE_NS, betweenness_values, centrality_values, design,
                                     design_large, one_hot_rho, path_betweenness, repeat_samples, triads_sparse)
from tests.test_hip_betweenness import _assert_own_reductions, _assert_path_length_identity, _assert_values, _stateless
from tests.test_hip_centrality import _assert_equal_cent, _coo_engine_with_rho
from tests.test_hip_connectivity import _assert_equal_conn
from tests.test_hip_cores import SUMMARY, _assert_equal_cores
from tests.test_hip_triads import _assert_equal_triads

pytestmark = pytest.mark.gpu

S, SEED, TOP_K, K_MIN = 2, 40, 5, 3
BOUND_LAYERS = [0, 3]


def _design_engine(Y):
    """A coordinate-list handle whose every sample is (Y > 0): K = 2, so the sampled calls see entries 0 and 1 only, and the
    design's entries above 1 are exercised by the calls that take networks."""
    rho = one_hot_rho(Y)
    eng = _coo_engine_with_rho(rho)
    del rho
    try:
        assert np.array_equal(eng.sample(SEED) > 0, Y > 0)
    except BaseException:
        eng.close()
        raise
    return eng


@pytest.fixture(scope="module")
def handles():
    """get(N): the handle of `design(N)` -- layers 0 and 3 at the node bound -- shared by the units' tests of that N and closed
    with the module; created with VMR_NETSTATS_CHUNK = 1 (the switch is read once per handle)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("VMR_NETSTATS_CHUNK", "1")
    made = {}

    def get(N):
        if N not in made:
            made[N] = _design_engine(design(N)[BOUND_LAYERS] if N == BOUND_N else design(N))
        return made[N]

    try:
        yield get
    finally:
        for eng in made.values():
            eng.close()
        mp.undo()


@pytest.mark.parametrize("N", MAIN_NS)
def test_cores(N, handles):
    """Every mode, every key of `sample_cores` against `cores_np`; `network_cores` on a handle with no state, the four layers as
    four networks of one call (entries above 1 and the diagonal as they are in the design)."""
    Y, eng = design(N), handles(N)
    net = _stateless(1, N)
    try:
        for m in MODES:
            vals = cores_np([Y], m)["values"]
            assert vals[0, [0, 2, 3]].max(axis=1).min() >= 1, m       # (the directed path has no 1-core of in- or out-degrees)
            want = reduce_cores(np.repeat(vals, S, axis=0), K_MIN, TOP_K)
            want["values"] = np.repeat(vals, S, axis=0)
            _assert_equal_cores(eng.sample_cores(SEED, S, mode=m, k_min=K_MIN, top_k=TOP_K, values=True), want)
            got, sm = net.network_cores(Y[:, None], mode=m, k_min=K_MIN, summary=True)
            assert got.dtype == np.uint16 and np.array_equal(got[:, 0], vals[0]), m
            for k in SUMMARY:
                assert sm[k].dtype == np.int64 and np.array_equal(sm[k][:, 0], want[k][0]), (m, k)
    finally:
        net.close()


def _check_connectivity(eng, Y):
    want = repeat_samples(connectivity_np([Y]), S)
    got = eng.sample_connectivity(SEED, S, nodes=True, hist=True)
    assert sorted(got) == sorted(want)
    _assert_equal_conn(got, want)
    return want


@pytest.mark.parametrize("N", MAIN_NS)
def test_connectivity(N, handles):
    """Every key against `connectivity_np`.  On the path the diameter is N - 1 and the histogram's last bin takes the
    (N - 64)(N - 63) / 2 pairs at distance 64 and beyond."""
    want = _check_connectivity(handles(N), design(N))
    assert want["diameter"][0, 1] == N - 1 and want["dist_hist"][0, 1, NDIST - 1] == (N - 64) * (N - 63) // 2
    assert (want["components_s"][0, [0, 1]] > 1).all() and (want["components_s"][0, [2, 3]] == 1).all()


@pytest.mark.parametrize("N", MAIN_NS)
def test_centrality(N, handles):
    """q = 1/2, T = 4, the three directions: bit for bit `centrality_np`, after `exact_ok` on every layer."""
    eng = handles(N)
    for d in CENT_DIRECTIONS:
        want = reduce_values(np.repeat(centrality_values(N, d)[None], S, axis=0), TOP_K)
        got = eng.sample_centrality(SEED, S, Q, T, direction=d, top_k=TOP_K, values=True)
        _assert_equal_cent(got, want)


@pytest.mark.parametrize("N", MAIN_NS)
def test_betweenness(N, handles):
    """Both directions: the values within 10 N 2^-53 of `betweenness_np` (the path layer: of its closed form, and equal to it),
    the reductions bit for bit on the device's own values, the total against `sample_connectivity`'s integers, and
    `network_betweenness` of the same networks the same bytes."""
    Y, eng = design(N), handles(N)
    for d in BTW_DIRECTIONS:
        want = betweenness_values(N, d)
        got = eng.sample_betweenness(SEED, S, direction=d, top_k=TOP_K, values=True)
        assert got["values"].shape == (S, 4, N) and got["values"].dtype == np.float64
        for s in range(S):
            _assert_values(got["values"][s], want, N, "N %d %s sample %d" % (N, d, s))
            assert np.array_equal(got["values"][s, 1], path_betweenness(N)), (d, s)
        _assert_own_reductions(got, TOP_K, N)
        if d == "directed":
            _assert_path_length_identity(eng, got, SEED, S)
        net = eng.network_betweenness(np.stack([Y] * S), direction=d)
        assert net.dtype == np.float64 and net.shape == (S, 4, N) and net.tobytes() == got["values"].tobytes(), d


def _check_triads(eng, Y, n_samples):
    want = repeat_samples(triads_sparse([Y]), n_samples)
    assert want["node_tri"].max() > 0 and want["transitive"].max() > 0 and want["cyclic"].max() > 0
    _assert_equal_triads(eng.sample_triads(SEED, n_samples, nodes=True), want)


@pytest.mark.parametrize("N", MAIN_NS)
def test_triads(N, handles):
    """The six counts, the triangles through every node and its degree against `triads_sparse`."""
    _check_triads(handles(N), design(N), S)


@pytest.mark.parametrize("unit", ["connectivity", "triads"])
def test_the_node_bound(unit, handles):
    """N = 2048, the sparse and the hub layer: connectivity at its node bound -- 32 words per bit row, 32 source blocks, threads
    own eight nodes, 48 KiB of LDS -- and the register path of triads with 32 words."""
    Y, eng = design(BOUND_N)[BOUND_LAYERS], handles(BOUND_N)
    if unit == "connectivity":
        want = _check_connectivity(eng, Y)
        assert (want["reach_pairs"] > 0).all() and (want["diameter"] >= 2).all()
    else:
        _check_triads(eng, Y, S)


@pytest.mark.parametrize("N", TRIAD_FOUR_NS)
def test_triads_register_path(N, monkeypatch):
    """N = 256 and 512, four layers: a lane meets one word of a row, W = 4 and 8."""
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "1")
    eng = _design_engine(design(N))
    try:
        _check_triads(eng, design(N), S)
    finally:
        eng.close()


@pytest.mark.parametrize("N", TRIAD_LARGE_NS)
def test_triads_beyond_one_block_of_words(N):
    """N = 2049 and 4097, one layer (the union of the sparse and the hub layer), one sample: the neighbour list is built from two
    and from three blocks of 32 words; at 4097 the hub fills two lists to the last slot, 64 lanes stride a row in two trips and
    the degree loop takes a second trip."""
    Y = design_large(N)
    eng = _design_engine(Y)
    try:
        _check_triads(eng, Y, 1)
    finally:
        eng.close()
