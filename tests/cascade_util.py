"""The cascade calls restated in NumPy / SciPy from the contract in include/vimure_hip.h (vmr_sample_outreach,
vmr_sample_seed_outreach, vmr_network_outreach, vmr_network_seed_outreach); nothing here imports vimure_amd.

The model.  Per layer l, A = (Y > 0) with the diagonal cleared, U = A | A.T.  Cascade k of network s keeps tie (l, i, j) iff
u < q_l, u the sampler's uniform (tests/draws_ref.sample_uniform) of words 0 and 1 of Philox4x32-10 with key = (cascade_seed + s)
mod 2^64 and counter = (t low, t high, k, 1), t = (l N + i) N + j; under "union" the pair {i, j} draws once, at (l, min, max).
The uniforms are drawn only at the ties that exist.  The spread follows A ("out"), A.T ("in") or U ("union"); active_0 is the seed
set, a period adds every node a live tie leads to from the nodes the previous period added, and the outreach after T periods is
|active_T| - |active_0|.  Everything after the comparison u < q_l is an integer, so the device must be met with `==`.

Also the designed graphs of the tests (path, star, two cliques joined by a bridge beside a mutual pair and isolated nodes) and
their closed forms at q = 1."""
import numpy as np
import scipy.sparse as sp

from tests.draws_ref import _M32, _S32, _split, philox4x32_10, sample_uniform

DIRECTIONS = ("out", "in", "union")
NPER = 64
NODE_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "total", "max")


def adjacency(Y):
    """bool [..., N, N]: Y > 0 with the diagonal cleared."""
    A = np.asarray(Y) > 0
    N = A.shape[-1]
    return A & ~np.eye(N, dtype=bool)


def tie_uniforms(key, k, t):
    """The uniform of cascade k at the ties t (indices in [L, N, N] order) under the key `key`: float64, exact."""
    t = np.asarray(t, dtype=np.uint64)
    k0, k1 = _split(key)
    w = philox4x32_10(t & _M32, t >> _S32, np.uint64(k), np.uint64(1), k0, k1)
    return sample_uniform(w[0], w[1])


def live_graph(A, key, k, q, direction):
    """G bool [L, N, N] of cascade k: G[l, u, v] says that u informs v -- the live ties of A ("out"), their transpose ("in") or
    the live pairs of A | A.T, both ways ("union").  A: bool [L, N, N] without diagonal; q: [L]."""
    L, N, _ = A.shape
    G = np.zeros((L, N, N), dtype=bool)
    for l in range(L):
        if direction == "union":
            i, j = np.nonzero(np.triu(A[l] | A[l].T, 1))
        else:
            i, j = np.nonzero(A[l])
        t = (np.uint64(l) * np.uint64(N) + i.astype(np.uint64)) * np.uint64(N) + j.astype(np.uint64)
        live = tie_uniforms(key, k, t) < float(q[l])
        i, j = i[live], j[live]
        if direction == "out":
            G[l, i, j] = True
        elif direction == "in":
            G[l, j, i] = True
        else:
            G[l, i, j] = True
            G[l, j, i] = True
    return G


def spread(G, init, T):
    """The cascade over G bool [N, N] from the B seed sets init bool [B, N]: (active_T bool [B, N], new int64 [periods, B], the
    nodes each period added; the periods end with T or with the first that adds nothing)."""
    Gs = sp.csr_matrix(G.astype(np.int32))
    active = init.copy()
    front = init.copy()
    new = []
    for _ in range(int(T)):
        nxt = np.asarray((sp.csr_matrix(front.astype(np.int32)) @ Gs).todense()) > 0
        nxt &= ~active
        if not nxt.any():
            break
        active |= nxt
        front = nxt
        new.append(nxt.sum(axis=1).astype(np.int64))
    return active, np.asarray(new, dtype=np.int64).reshape(len(new), init.shape[0])


def _q(q, L):
    return np.broadcast_to(np.asarray(q, dtype=np.float64), (L,))


def outreach_values(Ys, cascade_seed, n_cascades, q, T, direction):
    """values uint32 [n, L, N] of vmr_sample_outreach / vmr_network_outreach for the networks Ys [n, L, N, N] (network s is
    sample s of the call): sum_k of the outreach of {v} in cascade k."""
    A = adjacency(Ys)
    n, L, N, _ = A.shape
    q = _q(q, L)
    out = np.zeros((n, L, N), dtype=np.int64)
    eye = np.eye(N, dtype=bool)
    for s in range(n):
        for k in range(n_cascades):
            G = live_graph(A[s], (int(cascade_seed) + s) % 2 ** 64, k, q, direction)
            for l in range(L):
                out[s, l] += spread(G[l], eye, T)[0].sum(axis=1) - 1
    return out.astype(np.uint32)


def reduce_values(values, n_cascades, top_k):
    """Every other output of vmr_sample_outreach from its values [S, L, N], with the dtypes of `CaviEngine.sample_outreach`: the
    node score c = values / n_cascades, its sums in ascending s (the square rounded, then added), rank[v] = #{u : c[u] > c[v]},
    and per sample (sum_v values mod 2^32, max_v values)."""
    v = np.asarray(values)
    S, L, N = v.shape
    c = v.astype(np.float64) / float(n_cascades)
    node_sum, node_sumsq = np.zeros((L, N)), np.zeros((L, N))
    rank_sum, top = np.zeros((L, N), np.int64), np.zeros((L, N), np.int64)
    for s in range(S):
        node_sum = node_sum + c[s]
        node_sumsq = node_sumsq + c[s] * c[s]
        rank = (c[s][:, None, :] > c[s][:, :, None]).sum(axis=-1)
        rank_sum += rank
        top += rank < top_k
    return {"node_sum": node_sum, "node_sumsq": node_sumsq, "node_rank_sum": rank_sum, "node_top": top,
            "total": v.astype(np.int64).sum(axis=-1) % 2 ** 32, "max": v.astype(np.int64).max(axis=-1)}


def outreach_np(Ys, cascade_seed, n_cascades, q, T, direction, top_k):
    """The dict of `CaviEngine.sample_outreach(.., values=True)` for the samples Ys."""
    vals = outreach_values(Ys, cascade_seed, n_cascades, q, T, direction)
    out = reduce_values(vals, n_cascades, top_k)
    out["values"] = vals
    return out


def set_matrix(sets, N):
    """bool [n_sets, N] of seed sets given as index sequences."""
    init = np.zeros((len(sets), N), dtype=bool)
    for b, nodes in enumerate(sets):
        init[b, np.asarray(list(nodes), dtype=np.int64)] = True
    return init


def set_words(sets, N):
    """uint64 [N]: bit b of word v is set iff node v is in set b."""
    init = set_matrix(sets, N)
    w = np.zeros(N, dtype=np.uint64)
    for b in range(len(sets)):
        w |= init[b].astype(np.uint64) << np.uint64(b)
    return w


def seed_outreach_np(Ys, cascade_seed, n_cascades, q, T, direction, sets):
    """The dict of `CaviEngine.sample_seed_outreach(.., curve=True, node_hits=True)` for the samples Ys and the seed sets `sets`
    (index sequences): values uint32 [n, L, n_sets], curve int64 [L, n_sets, 64] (bin t - 1: the nodes period t added, the last
    bin every period >= 64), node_hits int64 [L, n_sets, N] (the (s, k) with v in active_T, seeds included)."""
    A = adjacency(Ys)
    n, L, N, _ = A.shape
    q = _q(q, L)
    init = set_matrix(sets, N)
    B = len(sets)
    vals = np.zeros((n, L, B), dtype=np.int64)
    curve = np.zeros((L, B, NPER), dtype=np.int64)
    hits = np.zeros((L, B, N), dtype=np.int64)
    for s in range(n):
        for k in range(n_cascades):
            G = live_graph(A[s], (int(cascade_seed) + s) % 2 ** 64, k, q, direction)
            for l in range(L):
                active, new = spread(G[l], init, T)
                vals[s, l] += active.sum(axis=1) - init.sum(axis=1)
                hits[l] += active
                for d, c in enumerate(new):
                    curve[l, :, min(d + 1, NPER) - 1] += c
    return {"values": vals.astype(np.uint32), "curve": curve, "node_hits": hits}


# ------------------------------------------------------------------------------------------------ designed graphs
def path(N):
    """0 -> 1 -> .. -> N - 1."""
    Y = np.zeros((N, N), np.uint8)
    Y[np.arange(N - 1), np.arange(1, N)] = 1
    return Y


def path_outreach(N, T, direction):
    """The outreach of every node of path(N) at q = 1: min(T, N - 1 - i) nodes ahead, min(T, i) behind."""
    i = np.arange(N)
    ahead, behind = np.minimum(T, N - 1 - i), np.minimum(T, i)
    return {"out": ahead, "in": behind, "union": ahead + behind}[direction]


def star(N):
    """The hub 0 -> every other node."""
    Y = np.zeros((N, N), np.uint8)
    Y[0, 1:] = 1
    return Y


def star_outreach(N, T, direction):
    """The outreach of every node of star(N) at q = 1: the hub reaches its N - 1 leaves along the ties, a leaf its hub against
    them, and over the symmetrised star a leaf reaches the hub in one period and everybody from the second."""
    out = np.zeros(N, np.int64)
    if direction == "out":
        out[0] = N - 1
    elif direction == "in":
        out[1:] = 1
    else:
        out[0] = N - 1
        out[1:] = 1 if T == 1 else N - 1
    return out


def two_cliques(N, c=20):
    """Nodes [0, c) and [c, 2 c): two cliques, every tie both ways; the bridge c - 1 -> c one way; 2 c <-> 2 c + 1 a mutual
    pair; the rest isolated, with a few diagonal entries that must be ignored."""
    assert N >= 2 * c + 4
    Y = np.zeros((N, N), np.uint8)
    Y[:c, :c] = 1
    Y[c:2 * c, c:2 * c] = 1
    Y[c - 1, c] = 3
    Y[2 * c, 2 * c + 1] = Y[2 * c + 1, 2 * c] = 1
    Y[np.arange(N), np.arange(N)] = np.arange(N) % 2
    return Y


def two_cliques_outreach(N, T, direction, c=20):
    """The outreach of every node of two_cliques(N, c) at q = 1."""
    i = np.arange(N)
    first, second = i < c, (i >= c) & (i < 2 * c)
    own = np.where(first | second, c - 1, 0)
    # across the bridge c - 1 -> c: c - 1 is one period from c and two from the rest of the second clique; the other nodes of
    # the first clique one period more
    d_tail = np.where(i == c - 1, 0, 1)            # periods from a node of the first clique to the bridge's tail
    d_head = np.where(i == c, 0, 1)                # periods from the bridge's head to a node of the second clique
    fwd = np.where(first, (T >= d_tail + 1).astype(np.int64) + (c - 1) * (T >= d_tail + 2), 0)
    bwd = np.where(second, (T >= d_head + 1).astype(np.int64) + (c - 1) * (T >= d_head + 2), 0)
    pair = np.where((i == 2 * c) | (i == 2 * c + 1), 1, 0)
    return own + pair + {"out": fwd, "in": bwd, "union": fwd + bwd}[direction]


def random_digraph(N, per_node, seed, diag=True):
    """A random digraph with `per_node` ties per node in expectation, entries in 1 .. 3, and random diagonal entries."""
    rng = np.random.RandomState(seed)
    Y = (rng.random_sample((N, N)) < per_node / float(N)).astype(np.uint8) * rng.randint(1, 4, (N, N)).astype(np.uint8)
    if diag:
        d = np.arange(0, N, 3)
        Y[d, d] = 1
    return Y
