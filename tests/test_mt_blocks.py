"""CPU: the block descriptors of the device draw of the rho prior (`_hostlib.mt_block_states`, vmr_host_mt_states).  Block b
starts at tie cuts[b] with the RandomState's MT19937 state after cuts[b] * K doubles, and the generator ends where
`rand(L, N, N, K)` leaves it, whatever position it started from."""
import numpy as np
import pytest

from vimure_amd import _hostlib

pytestmark = pytest.mark.skipif(_hostlib.load() is None, reason="no C compiler for the host helper")


def _start(kind, seed=11):
    g = np.random.RandomState(seed)
    if kind == "odd":
        g.randint(1, 500)               # one 32-bit word: an odd position
    elif kind == "mid":
        g.random_sample(157)            # 314 words into the buffer
    st = g.get_state()
    assert (kind == "fresh") == (st[2] == 624) and (kind != "odd" or st[2] % 2 == 1)
    return g


@pytest.mark.parametrize("start", ["fresh", "odd", "mid"])
@pytest.mark.parametrize("L,N,K,nblk", [(1, 7, 2, 1), (1, 7, 2, 49), (2, 9, 12, 5), (1, 13, 2, 40), (1, 4, 256, 3),
                                        (3, 20, 2, 17), (1, 6, 256, 36)])
def test_block_states_are_the_generators_states(start, L, N, K, nblk):
    g = _start(start)
    ref = np.random.RandomState()
    ref.set_state(g.get_state())
    cuts, keys, pos = _hostlib.mt_block_states(g, L, N, K, nblk)
    ties = L * N * N
    assert cuts.dtype == np.int64 and keys.dtype == np.uint32 and pos.dtype == np.int32
    assert cuts.shape == (nblk + 1,) and keys.shape == (nblk, 624) and pos.shape == (nblk,)
    assert cuts[0] == 0 and cuts[-1] == ties and np.all(np.diff(cuts) > 0)
    for b in range(nblk):
        walk = np.random.RandomState()
        walk.set_state(ref.get_state())
        walk.random_sample(int(cuts[b]) * K)
        st = walk.get_state()
        assert int(pos[b]) == st[2], b
        assert np.array_equal(keys[b], st[1]), b
    # the generator ends where the host draw ends: the gamma draws and the seed chain after it are unchanged
    ref.rand(L, N, N, K)
    a, b = g.get_state(), ref.get_state()
    assert a[2] == b[2] and np.array_equal(a[1], b[1])
    assert np.array_equal(g.random_sample(9), ref.random_sample(9)) and g.randint(1, 500) == ref.randint(1, 500)


@pytest.mark.parametrize("start", ["fresh", "odd"])
def test_blocks_shorter_than_a_refill_and_positions_at_a_refill(start):
    """K = 2, one tie per block (4 words): many block starts fall mid-buffer, at odd positions (after a randint) or exactly on
    624 (a refill still to come)."""
    g = _start(start, seed=3)
    ref = np.random.RandomState()
    ref.set_state(g.get_state())
    cuts, keys, pos = _hostlib.mt_block_states(g, 1, 30, 2, 900)
    assert np.array_equal(cuts, np.arange(901))
    if start == "fresh":
        assert (pos == 624).sum() > 1
    else:
        assert np.all(pos % 2 == 1)
    w = np.random.RandomState()
    w.set_state(ref.get_state())
    for b in range(900):
        st = w.get_state()
        assert st[2] == pos[b] and np.array_equal(st[1], keys[b]), b
        w.random_sample(2)


def test_default_block_count():
    assert _hostlib.block_count(4, 2000, 2) == 1954                  # BASELINE config 3: 64 M words, blocks of 32 K words
    assert _hostlib.block_count(1, 9000, 11) == _hostlib.MAX_BLOCKS   # 1.8 G words: the 2.5 KB states stay at 20 MB
    assert _hostlib.block_count(1, 3, 2) == 1 and _hostlib.block_count(1, 1, 256) == 1
    assert _hostlib.block_count(1, 300, 9) == 50
    g = np.random.RandomState(0)
    cuts, keys, pos = _hostlib.mt_block_states(g, 1, 50, 4)
    assert len(pos) == _hostlib.block_count(1, 50, 4) and cuts[-1] == 2500


def test_nblk_is_clamped_to_the_ties():
    cuts, keys, pos = _hostlib.mt_block_states(np.random.RandomState(1), 1, 2, 2, 100)
    assert np.array_equal(cuts, [0, 1, 2, 3, 4]) and keys.shape == (4, 624)


def test_not_an_mt19937_state():
    class Other:
        def get_state(self):
            return ("PCG64",)
    assert _hostlib.mt_block_states(Other(), 1, 4, 2) is None
