"""NumPy restatements of the k-core decomposition of vmr_sample_cores / vmr_network_cores (include/vimure_hip.h): the peeling in
rounds the device runs, and -- independent of it -- the definition applied literally."""
import numpy as np

MODES = ("union", "total", "in", "out")
CORE_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "node_main", "node_atleast", "degeneracy", "main_core_size",
             "core_sum", "kcore_size")


def adjacency(Y):
    """A [N, N] bool of one layer of one network: Y > 0 without its diagonal."""
    A = np.asarray(Y) > 0
    return A & ~np.eye(A.shape[0], dtype=bool)


def degrees_inside(A, mode, S):
    """int64 [N]: the degree of every node counted inside the node set S (bool [N]) -- for the nodes outside S too."""
    B = A & S[None, :] & S[:, None]
    if mode == "union":
        return (B | B.T).sum(axis=1).astype(np.int64)
    if mode == "total":
        return (B.sum(axis=1) + B.sum(axis=0)).astype(np.int64)
    if mode == "in":
        return B.sum(axis=0).astype(np.int64)
    assert mode == "out"
    return B.sum(axis=1).astype(np.int64)


def core_definition(A, mode):
    """int64 [N] straight from the definition: for k = 1, 2, .. start from ALL nodes and delete the nodes of degree < k inside the
    set until nothing changes; what is left is the k-core, and core[v] is the largest k whose core holds v."""
    N = A.shape[0]
    core = np.zeros(N, np.int64)
    for k in range(1, 2 * N):
        S = np.ones(N, bool)
        while True:
            drop = S & (degrees_inside(A, mode, S) < k)
            if not drop.any():
                break
            S &= ~drop
        if not S.any():
            break
        core[S] = k
    return core


def core_peel(A, mode):
    """(core int64 [N], rounds): the peeling in rounds.  k = 0; per round the alive nodes with deg <= k (a snapshot) get core = k
    and leave together, and every alive node loses what the mode says per leaving neighbour: union 1 per distinct neighbour,
    total 1 per tie either way (a mutual neighbour costs 2), in 1 per tie from a leaving node, out 1 per tie to one.  A round in
    which nobody can leave sets k to the smallest deg alive.  Rounds are counted until no node is alive."""
    N = A.shape[0]
    Ai = A.astype(np.int64)
    U = (A | A.T).astype(np.int64)
    alive = np.ones(N, bool)
    deg = degrees_inside(A, mode, alive)
    core = np.zeros(N, np.int64)
    k, rounds = 0, 0
    while alive.any():
        rounds += 1
        assert rounds <= 2 * N
        marked = alive & (deg <= k)
        if not marked.any():
            k = int(deg[alive].min())
            continue
        core[marked] = k
        alive &= ~marked
        if mode == "union":
            loss = U[marked].sum(axis=0)
        elif mode == "total":
            loss = Ai[marked].sum(axis=0) + Ai[:, marked].sum(axis=1)
        elif mode == "in":
            loss = Ai[marked].sum(axis=0)
        else:
            loss = Ai[:, marked].sum(axis=1)
        deg[alive] -= loss[alive]
        assert (deg[alive] >= 0).all()
    return core, rounds


def reduce_values(values, k_min, top_k):
    """Everything `CaviEngine.sample_cores` returns beside `values`, from values [S, L, N]."""
    v = np.asarray(values).astype(np.int64)
    S, L, N = v.shape
    rank = np.zeros((S, L, N), np.int64)   # #{u : v[u] > v[w]}
    for s in range(S):
        for l in range(L):
            rank[s, l] = N - np.searchsorted(np.sort(v[s, l]), v[s, l], side="right")
    dg = v.max(axis=2)
    return {"node_sum": v.sum(axis=0).astype(np.float64), "node_sumsq": (v * v).sum(axis=0).astype(np.float64),
            "node_rank_sum": rank.sum(axis=0).astype(np.int64), "node_top": (rank < top_k).sum(axis=0).astype(np.int64),
            "node_main": (v == dg[:, :, None]).sum(axis=0).astype(np.int64), "node_atleast": (v >= k_min).sum(axis=0).astype(np.int64),
            "degeneracy": dg, "main_core_size": (v == dg[:, :, None]).sum(axis=2), "core_sum": v.sum(axis=2),
            "kcore_size": (v >= k_min).sum(axis=2)}


def cores_np(Ys, mode="union", k_min=0, top_k=10):
    """Ys: networks [S][L, N, N] (a list or an array).  Returns the dict `CaviEngine.sample_cores(..., values=True)` returns."""
    Ys = np.asarray(Ys)
    S, L, N, _ = Ys.shape
    vals = np.zeros((S, L, N), np.uint16)
    for s in range(S):
        for l in range(L):
            vals[s, l] = core_peel(adjacency(Ys[s, l]), mode)[0]
    out = reduce_values(vals, k_min, top_k)
    out["values"] = vals
    return out


def clique(n):
    """every tie, the diagonal's too."""
    return np.ones((n, n), np.uint8)


def path(n, directed=True):
    """0 -> 1 -> .. -> n - 1, with every diagonal entry set."""
    Y = np.eye(n, dtype=np.uint8)
    Y[np.arange(n - 1), np.arange(1, n)] = 1
    return Y if directed else Y | Y.T


def cycle(n, directed=True):
    Y = np.eye(n, dtype=np.uint8)
    Y[np.arange(n), (np.arange(n) + 1) % n] = 1
    return Y if directed else Y | Y.T


def out_star(n):
    """ties leave node 0 only; the diagonal set."""
    Y = np.eye(n, dtype=np.uint8)
    Y[0, 1:] = 1
    return Y


def mixed_design(N=300):
    """uint8 [N, N], N >= 210: a 40-clique (nodes 0..39, every tie mutual), a directed path 40 -> 41 -> .. -> 199, a mutual pair
    (200, 201), the rest isolated; every diagonal entry set.  Coreness, union: 39 / 1 / 1 / 0 -- k jumps 0 -> 1 -> 39, and the
    pair's two nodes leave in the same round; total: 78, 1 along the path (its ends have one tie), 2 for the pair."""
    Y = np.eye(N, dtype=np.uint8)
    Y[:40, :40] = 1
    Y[np.arange(40, 199), np.arange(41, 200)] = 1
    Y[200, 201] = Y[201, 200] = 1
    return Y


def mixed_design_cores(N=300):
    """{mode: int64 [N]} of `mixed_design(N)`, in closed form."""
    z = np.zeros(N, np.int64)
    u, t, i, o = z.copy(), z.copy(), z.copy(), z.copy()
    u[:40], u[40:200], u[200:202] = 39, 1, 1
    t[:40], t[40:200], t[200:202] = 78, 1, 2
    i[:40], i[200:202] = 39, 1          # along a directed path the head has no in-tie: it leaves, then the next one: all 0
    o[:40], o[200:202] = 39, 1
    return {"union": u, "total": t, "in": i, "out": o}


def random_planted(N, p_ties, n_clique, seed):
    """uint8 [N, N]: a random digraph with p_ties expected out-ties per node, a mutual n_clique-clique planted on nodes spread
    over the whole index range (the last node among them), and random diagonal entries."""
    g = np.random.RandomState(seed)
    Y = (g.rand(N, N) < p_ties / N).astype(np.uint8)
    members = np.unique(np.r_[g.choice(N - 1, n_clique - 1, replace=False), N - 1])
    Y[np.ix_(members, members)] = 1
    return Y
