"""GPU: the seed of the chunked sampled calls (sample_stats, sample_triads, sample_mixing, ppc_replicates) crossing 2^64 at a chunk
boundary and inside a chunk.  Sample s of a call of S samples from `seed`, cut into chunks of 3, is held bit for bit to the same
call for one sample at `(seed + s) % 2^64` on a handle whose chunks are sized from free memory."""
import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

SEED = 2 ** 64 - 2   # samples 0, 1 below 2^64, sample 2 at seed 0: the wrap is inside the first chunk of 3
SEED_X = 2 ** 64 - 4   # ppc_replicates' second seed wraps at another sample, inside the second chunk
CHUNK = 3


def _calls(eng):
    """name -> call(seed, first sample, S) returning a list of arrays with the sample axis first"""
    g = np.random.RandomState(5)
    groups = (np.arange(eng.N) % 4).astype(np.int64)
    groups[::7] = -1
    theta = g.gamma(2.0, 0.3, (8, eng.L, eng.M))
    lam = np.sort(g.gamma(2.0, 0.5, (8, eng.L, eng.K)), -1)
    eta = g.uniform(0.0, 0.8, 8)

    def stats(seed, s, S):
        r = eng.sample_stats(seed, S, n_trials=2, degrees=True)
        return [r[k] for k in sorted(r)]

    def triads(seed, s, S):
        r = eng.sample_triads(seed, S, n_trials=2, nodes=True)
        return [r[k] for k in sorted(r)]

    def mixing(seed, s, S):
        r = eng.sample_mixing(seed, S, groups=groups, C=4, n_trials=2)
        return [r[k] for k in sorted(r)]

    def ppc(seed, s, S):   # replicate s of the long call has the parameters of row s and the second seed SEED_X + s
        return list(eng.ppc_replicates(theta[s:s + S], lam[s:s + S], eta[s:s + S], seed, (SEED_X + s) % 2 ** 64, n_trials=2,
                                       by_reporter=True))

    return {"sample_stats": stats, "sample_triads": triads, "sample_mixing": mixing, "ppc_replicates": ppc}


def _engine():
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    return _engine_for(d["X"], d["R"], K, mut, _golden_state(d))


@pytest.fixture(scope="module")
def one_by_one():
    """every call for one sample at (SEED + s) % 2^64, s in [0, 7), on a handle without the cap: computed once"""
    mp = pytest.MonkeyPatch()
    mp.delenv("VMR_NETSTATS_CHUNK", raising=False)
    try:
        eng = _engine()
    finally:
        mp.undo()
    try:
        return {name: [call((SEED + s) % 2 ** 64, s, 1) for s in range(7)] for name, call in _calls(eng).items()}
    finally:
        eng.close()


@pytest.mark.parametrize("S", [7, 6], ids=["3+3+1", "3+3"])
@pytest.mark.parametrize("name", ["sample_stats", "sample_triads", "sample_mixing", "ppc_replicates"])
def test_seed_wraps_across_chunks(name, S, one_by_one, monkeypatch):
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", str(CHUNK))   # (read when the handle is created)
    eng = _engine()
    try:
        got = _calls(eng)[name](SEED, 0, S)
    finally:
        eng.close()
    for s in range(S):
        want = one_by_one[name][s]
        assert len(got) == len(want)
        for q, (a, b) in enumerate(zip(got, want)):
            assert a.shape[0] == S and b.shape[0] == 1 and a.dtype == b.dtype, (name, q)
            assert np.array_equal(a[s], b[0]), (name, s, q)
    assert any(a.any() for a in got), name   # (the samples are not empty networks)
