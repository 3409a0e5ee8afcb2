"""GPU: the held-out report log-likelihood on the device (vmr_heldout_loglik) against its NumPy restatement
(`crossval.heldout_loglik_np`) fed with the rho given to `set_state`.  Counts exact; `mean` within (2 K + 2) 2^-52 mean (K products,
K adds); `logp` within C_LOGP 2^-52 T, T the size of the terms that cancel; the layer sums within n 2^-52 sum |v| plus the
per-entry bounds, whatever the tree.  Both data layouts, no mask and a random mask over two mask words with empty and all-ones
rows, a coordinate-list handle with a self-reporter mask (rho by sorted position), K = 2, 3 and 12 (one lane per entry; a group of
lanes per entry), lists that end inside a workgroup's chunk with the layer boundary inside one, a list of layer 1 only, n = 1,
planted one-hot rows, a zero inside a row, a zero rate against x > 0, mirrored counts, a count of 100000, repeated entries;
bit-identical between calls, between host and device pointers and across snapshot / restore; every refusal.

C_LOGP and the bounds: tests/heldout_util.py (the measured worst ratio and the constant chosen from it are stated there)."""
import numpy as np
import pytest

from tests.heldout_util import compare_entries, compare_sums, term_size

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
L, N = 2, 70                  # N: no multiple of 64
CHUNK = 1024                  # entries of a workgroup (HO_CHUNK, heldout.hip)
N0, N1 = 1700, 1301           # entries of layer 0 and 1: 3001 in all, two chunks each, the layer boundary inside the list's second chunk

_CASES = {}


def _rho(g, K, shape):
    """Random normalised rows with planted ones: one-hot on category 0 and on category 1, and (K >= 3) a zero in the middle."""
    rho = g.rand(*shape, K)
    rho[..., 0] *= 6.0
    rho = rho / rho.sum(-1, keepdims=True)
    e0, e1 = np.zeros(K), np.zeros(K)
    e0[0], e1[1] = 1.0, 1.0
    rho[:, 3, ::7], rho[:, 4, ::7] = e0, e1
    if K >= 3:
        z = np.full(K, 1.0 / (K - 1))
        z[1] = 0.0
        rho[:, 5, ::7] = z
    return np.ascontiguousarray(rho)


def _tables(g, nl, M, K):
    theta = g.gamma(2.0, 0.5, (nl, M)) + 0.05
    lam = g.gamma(2.0, 1.0, (nl, K)) + 0.05
    lam[:, 0] = 0.0               # category 0: rate 0 without a mirrored count
    return theta, lam


def _list(g, nl, n_by_layer, n_nodes, M):
    """A list sorted by layer only, with entries on the planted rows (x > 0 and x = 0 there), mirrored counts, and repeats."""
    cols = []
    for l, n in enumerate(n_by_layer):
        if n == 0:
            continue
        i, j, m = g.randint(0, n_nodes, n), g.randint(0, n_nodes, n), g.randint(0, M, n)
        q = max(1, n // 6)
        i[:q] = 3 + g.randint(0, 3, q)                      # the planted rows 3, 4, 5 ...
        j[:q] = 7 * g.randint(0, (n_nodes + 6) // 7, q)     # ... at the planted columns
        r = max(1, n // 20)
        i[-r:], j[-r:], m[-r:] = i[:r], j[:r], m[:r]        # repeated entries (with other counts)
        cols.append((np.full(n, l), i, j, m))
    subs = tuple(np.concatenate([c[q] for c in cols]).astype(np.int64) for q in range(4))
    n = len(subs[0])
    x = (g.rand(n) < 0.5) * g.randint(1, 6, n)
    xt = (g.rand(n) < 0.3) * g.randint(1, 4, n)
    return subs, x.astype(np.int64), xt.astype(np.int64)


def _case(K, M):
    key = (K, M)
    if key not in _CASES:
        g = np.random.RandomState(170 + K + M)
        X = ((g.rand(L, N, N, M) < 0.05) * g.randint(1, 4, (L, N, N, M))).astype(np.uint8)
        rho = _rho(g, K, (L, N, N))
        gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
        ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
        R = (g.rand(L, N, N, M) < 0.5).astype(np.uint8)             # density 0.5, M = 70: two mask words
        R[:, 7] = 0                                                  # empty rows
        R[:, 8], R[0, :, 20] = 1, 1                                  # rows made all ones
        theta, lam = _tables(g, L, M, K)
        subs, x, xt = _list(g, L, (N0, N1), N, M)
        _CASES[key] = dict(X=X, R=R, rho=rho, st=(gs, gr, ps, pr, 3.0, 2.5, rho), theta=theta, lam=lam, subs=subs, x=x, xt=xt, want={})
    return _CASES[key]


def _engine(X, R, K, st, mut=True, coo=False):
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    eng.set_priors(*PRI)
    if st is not None:
        eng.set_state(*st)
    return eng


def _want(c, key, subs, x, xt, eta, R):
    from vimure_amd.crossval import heldout_loglik_np
    if key not in c["want"]:
        c["want"][key] = (heldout_loglik_np(c["rho"], subs, x, xt, c["theta"], c["lam"], eta, R=R),
                          term_size(c["rho"], subs, x, xt, c["theta"], c["lam"], eta))
    return c["want"][key]


def _planted_inf(c, subs, x, xt, eta):
    """Entries on a row that is one-hot on category 0 (rate 0 without a mirrored count) with x > 0 and no mirrored count."""
    r = c["rho"][subs[0], subs[1], subs[2]]
    return int(((r[:, 0] == 1.0) & (x > 0) & ((xt == 0) | (eta == 0.0))).sum())


def _run_case(K, fmt):
    for M, masked in ((5, False), (70, True)):
        c = _case(K, M)
        R = c["R"] if masked else None
        eng = _engine(c["X"], R, K, c["st"])
        try:
            assert eng.data_format()[0] == fmt
            subs, x, xt = c["subs"], c["x"], c["xt"]
            assert len(x) % CHUNK and len(x) > 2 * CHUNK and N0 % CHUNK and N1 % CHUNK
            for eta, use_xt in ((0.4, True), (0.0, False)):
                xq = xt if use_xt else None
                want, T = _want(c, ("full", masked, use_xt), subs, x, xq, eta, R)
                got = eng.heldout_loglik(subs, x, xq, theta=c["theta"], lam=c["lam"], eta=eta)
                compare_entries(got, want, T, K, f"K {K} M {M} eta {eta}")
                compare_sums(got["sums"], want, subs, x, T, K, f"K {K} M {M} eta {eta}")
                cn = got["counts"]
                assert cn[:, 0].tolist() == [N0, N1] and cn[:, 2].sum() == _planted_inf(c, subs, x, xt if use_xt else np.zeros_like(x), eta) > 0
                assert (cn[:, 3] == cn[:, 0]).all() if not masked else (0 < cn[:, 3].sum() < len(x))
                only = eng.heldout_loglik(subs, x, xq, theta=c["theta"], lam=c["lam"], eta=eta, per_entry=False)
                assert only["logp"] is None and np.array_equal(only["sums"].view(np.uint64), got["sums"].view(np.uint64))
            # the sorted list (the fast case): the same entries, so the same per-entry values, bit for bit
            order = np.lexsort(subs[::-1])
            srt = eng.heldout_loglik(tuple(s[order] for s in subs), x[order], xt[order], theta=c["theta"], lam=c["lam"], eta=0.4)
            full = eng.heldout_loglik(subs, x, xt, theta=c["theta"], lam=c["lam"], eta=0.4)
            assert np.array_equal(srt["logp"], full["logp"][order]) and np.array_equal(srt["mean"], full["mean"][order])
            assert np.array_equal(srt["counts"], full["counts"])
            # layer 1 only, and a single entry
            w = subs[0] == 1
            s1 = tuple(s[w] for s in subs)
            want1, T1 = _want(c, ("l1", masked), s1, x[w], xt[w], 0.4, R)
            got1 = eng.heldout_loglik(s1, x[w], xt[w], theta=c["theta"], lam=c["lam"], eta=0.4)
            compare_entries(got1, want1, T1, K, f"K {K} M {M} layer 1 only")
            assert got1["counts"][0].tolist() == [0, 0, 0, 0] and not got1["sums"][0].any()
            assert np.array_equal(got1["logp"], full["logp"][w])
            assert np.array_equal(got1["sums"][1].view(np.uint64), full["sums"][1].view(np.uint64))   # the tree is the segment's alone
            for e in (0, len(x) - 1):
                one = eng.heldout_loglik(tuple(s[e:e + 1] for s in subs), x[e:e + 1], xt[e:e + 1], theta=c["theta"], lam=c["lam"], eta=0.4)
                assert one["logp"][0] == full["logp"][e] and one["mean"][0] == full["mean"][e] and one["counts"][:, 0].sum() == 1
        finally:
            eng.close()


@pytest.mark.parametrize("K", [2, 3])
def test_against_the_restatement(K, vmr_format):
    _run_case(K, vmr_format)


def test_against_the_restatement_group_of_lanes_k12():
    """More than 8 categories: a group of lanes per entry (handles of the general kernels, over the report lists only)."""
    _run_case(12, "sparse")


@pytest.mark.parametrize("K", [2, 12])
def test_from_coo_handle_with_self_reporter_mask(K):
    """rho is stored by sorted position; the mask is held as reporter lists; one held-out count of 100000."""
    from vimure_amd.crossval import heldout_loglik_np
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(9 + K)
    n = 70
    R = np.asarray(self_reporter_mask(1, n, n)).astype(np.uint8)
    X = ((g.rand(1, n, n, n) < 0.3) * g.randint(1, 3, (1, n, n, n))).astype(np.uint8) * R
    rho = _rho(g, K, (1, n, n))
    gs, gr = g.gamma(2.0, 1.0, (1, n)) + 0.1, g.gamma(2.0, 1.0, (1, n)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (1, K)) + 0.1, g.gamma(2.0, 1.0, (1, K)) + 0.1
    theta, lam = _tables(g, 1, n, K)
    subs, x, xt = _list(g, 1, (2500,), n, n)
    half = len(x) // 2                                      # half of the list inside the mask: m = i or m = j
    subs[3][:half] = np.where(g.rand(half) < 0.5, subs[1][:half], subs[2][:half])
    big = int(np.flatnonzero(subs[1] > 5)[0])               # (not on a planted row)
    x[big] = 100000
    eng = _engine(X, R, K, (gs, gr, ps, pr, 3.0, 2.5, rho), True, coo=True)
    try:
        assert eng.mask_format()[0] == "lists" and eng.data_format()[0] == "sparse"
        want = heldout_loglik_np(rho, subs, x, xt, theta, lam, 0.4, R=R)
        T = term_size(rho, subs, x, xt, theta, lam, 0.4)
        got = eng.heldout_loglik(subs, x, xt, theta=theta, lam=lam, eta=0.4)
        c = dict(rho=rho)
        compare_entries(got, want, T, K, f"coo K {K}")
        compare_sums(got["sums"], want, subs, x, T, K, f"coo K {K}")
        assert got["counts"][0, 3] == int(R[subs].sum()) and half <= got["counts"][0, 3] < len(x)
        assert got["counts"][0, 2] == _planted_inf(c, subs, x, xt, 0.4) > 0
        assert np.isfinite(got["logp"][big]) and got["logp"][big] < -1e5 and T[big] > 1e5
    finally:
        eng.close()


def test_bit_identical_between_calls_pointers_and_after_restore():
    import torch
    from oracle import vimure_oracle as vo
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    c = _case(3, 70)
    eng = _engine(c["X"], c["R"], 3, c["st"])
    try:
        subs, x, xt = c["subs"], c["x"], c["xt"]
        kw = dict(theta=c["theta"], lam=c["lam"], eta=0.4)
        a, b = eng.heldout_loglik(subs, x, xt, **kw), eng.heldout_loglik(subs, x, xt, **kw)
        dev = torch.device("cuda", eng.device)
        ts = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32), device=dev) for v in list(subs) + [x, xt]]
        d = eng.heldout_loglik(tuple(ts[:4]), ts[4], ts[5], device=True, **kw)
        assert d["logp"].is_cuda and d["mean"].is_cuda
        for o in (b, {**d, "logp": d["logp"].cpu().numpy(), "mean": d["mean"].cpu().numpy()}):
            assert np.array_equal(a["counts"], o["counts"]) and np.array_equal(a["sums"].view(np.uint64), o["sums"].view(np.uint64))
            assert np.array_equal(a["logp"].view(np.uint64), o["logp"].view(np.uint64))
            assert np.array_equal(a["mean"].view(np.uint64), o["mean"].view(np.uint64))
    finally:
        eng.close()
    net = standard_sbm(N=24, M=12, L=2, K=2, avg_degree=4.0, eta=0.4, seed=3)
    X = np.asarray(net.X).astype(np.uint8)
    R = (np.random.RandomState(0).rand(*X.shape) < 0.8).astype(np.uint8)
    pr = vo.make_priors(2, 12, 2)
    st = vo.init_state(vo.Problem(X, R, 2, True, pr), np.random.RandomState(1))
    g = np.random.RandomState(4)
    subs, x, xt = _list(g, 2, (300, 200), 24, 12)
    theta, lam = _tables(g, 2, 12, 2)
    eng = CaviEngine(X, R, K=2, mutuality=True)
    try:
        eng.set_priors(pr.alpha_theta, pr.beta_theta, pr.alpha_lambda, pr.beta_lambda, pr.alpha_eta, pr.beta_eta)
        eng.set_state(st.gamma_shp, st.gamma_rte, st.phi_shp, st.phi_rte, st.nu_shp, st.nu_rte, st.pr_rho)
        eng.step(2)
        kw = dict(theta=theta, lam=lam, eta=0.3)
        at_snap = eng.heldout_loglik(subs, x, xt, **kw)
        eng.snapshot()
        eng.step(4)
        later = eng.heldout_loglik(subs, x, xt, **kw)
        eng.restore()
        back = eng.heldout_loglik(subs, x, xt, **kw)
        for k in ("logp", "mean", "sums"):
            assert np.array_equal(back[k].view(np.uint64), at_snap[k].view(np.uint64)), k
        assert np.array_equal(back["counts"], at_snap["counts"]) and not np.array_equal(later["logp"], back["logp"])
    finally:
        eng.close()


def test_refusals():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, HeldoutArgumentError
    c = _case(2, 5)
    M, K = 5, 2
    eng = _engine(c["X"], None, K, None)          # no state yet: an argument is refused before the state is even looked at
    try:
        n = 40
        cols = [np.ascontiguousarray(v[:n], dtype=np.int32) for v in list(c["subs"]) + [c["x"], c["xt"]]]
        cols[0][:] = np.sort(cols[0])
        p = [a.ctypes.data for a in cols]
        th, la = np.ascontiguousarray(c["theta"]), np.ascontiguousarray(c["lam"])
        lp, mn = np.zeros(n), np.zeros(n)
        sm, cn = np.zeros((L, _lib.HO_NSUM)), np.zeros((L, _lib.HO_NCOUNT), np.uint64)
        outs = (lp.ctypes.data, mn.ctypes.data, 0, sm.ctypes.data, cn.ctypes.data)
        fn = eng.lib.vmr_heldout_loglik

        def call(n_=n, ptrs=p, theta=th, lam=la, eta=0.3, out=outs):
            return fn(eng._h, n_, *ptrs, 0, None if theta is None else theta.ctypes.data, None if lam is None else lam.ctypes.data, eta, *out)
        assert fn(None, n, *p, 0, th.ctypes.data, la.ctypes.data, 0.3, *outs) == _lib.VMR_EINVAL
        bad_t, inf_l = th.copy(), la.copy()
        bad_t[1, 2], inf_l[0, 1] = -0.5, np.inf
        for kw, word in ((dict(ptrs=p[:1] + [None] + p[2:]), b"NULL"), (dict(ptrs=p[:4] + [None, p[5]]), b"NULL"),
                         (dict(out=(None, None, 0, None, None)), b"output"), (dict(n_=0), b"n must"), (dict(n_=2 ** 31), b"n must"),
                         (dict(theta=None), b"theta"), (dict(lam=None), b"lambda"), (dict(theta=bad_t), b"theta"),
                         (dict(lam=inf_l), b"lambda"), (dict(eta=float("nan")), b"eta"), (dict(eta=-0.1), b"eta")):
            assert call(**kw) == _lib.VMR_EINVAL, kw
            msg = eng.lib.vmr_last_error(eng._h)
            assert b"vmr_heldout_loglik" in msg and word in msg, (kw, msg)
        assert call() == _lib.VMR_ESTATE and b"vmr_set_state" in eng.lib.vmr_last_error(eng._h)
        assert not lp.any() and not sm.any() and not cn.any()                               # nothing was launched or written
        assert call(ptrs=p[:5] + [None]) == _lib.VMR_ESTATE                                 # (ext may be NULL)
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.heldout_loglik(c["subs"], c["x"], theta=th, lam=la)
        assert not isinstance(ei.value, HeldoutArgumentError)
        eng.set_state(*c["st"])
        ok = eng.heldout_loglik(c["subs"], c["x"], c["xt"], theta=th, lam=la, eta=0.3)
        # what the kernels refuse: the list's other entries are valid, the entry itself reads nothing
        subs, x, xt = c["subs"], c["x"], c["xt"]
        at = len(x) // 2
        for col, val, word in ((1, N, "out of range"), (2, -1, "out of range"), (3, M, "out of range"), (3, -7, "out of range"),
                               (1, 2 ** 31 - 1, "out of range"), (0, L, "out of range"), (0, -1, "out of range"),
                               (4, -1, "negative"), (5, -3, "negative"), (0, None, "non-decreasing")):
            v = [a.copy() for a in list(subs) + [x, xt]]
            if val is None:
                v[0][0] = 1                                                                 # layer 1 before layer 0
            else:
                v[col][at] = val
            with pytest.raises(HeldoutArgumentError, match=word) as ei:
                eng.heldout_loglik(tuple(v[:4]), v[4], v[5], theta=th, lam=la, eta=0.3)
            assert "vmr_heldout_loglik" in str(ei.value)
        for kw in (dict(theta=None), dict(theta=th[:1]), dict(lam=la[:, :1])):
            with pytest.raises(HeldoutArgumentError):
                eng.heldout_loglik(subs, x, xt, **{**dict(theta=th, lam=la), **kw})
        with pytest.raises(HeldoutArgumentError):
            eng.heldout_loglik(subs[:3], x, xt, theta=th, lam=la)
        with pytest.raises(HeldoutArgumentError):
            eng.heldout_loglik(subs, x[:-1], xt, theta=th, lam=la)
        import torch
        dev = torch.device("cuda", eng.device)
        on = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32), device=dev) for v in list(subs) + [x, xt]]
        for mixed in ((tuple(on[:4]), x, xt), (subs, on[4], xt), (subs, x, on[5]), ((on[0],) + tuple(subs[1:]), x, xt)):
            with pytest.raises(HeldoutArgumentError, match="all NumPy arrays or all GPU tensors"):
                eng.heldout_loglik(*mixed, theta=th, lam=la)
        again = eng.heldout_loglik(subs, x, xt, theta=th, lam=la, eta=0.3)                  # the handle is as good as before
        assert np.array_equal(again["logp"].view(np.uint64), ok["logp"].view(np.uint64))
        # a NaN in rho, at a tie of the list
        rho = c["rho"].copy()
        rho[subs[0][at], subs[1][at], subs[2][at]] = np.nan
        eng.set_state(*c["st"][:6], rho)
        with pytest.raises(ValueError, match="NaN") as ei:
            eng.heldout_loglik(subs, x, xt, theta=th, lam=la, eta=0.3)
        assert not isinstance(ei.value, HeldoutArgumentError)
    finally:
        eng.close()


def test_through_the_model():
    import warnings
    from vimure_amd import VimureModel
    from vimure_amd.crossval import heldout_loglik_np, mirror_counts, plug_in_tables
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=30, M=30, L=1, K=2, avg_degree=4.0, eta=0.3, seed=5, flag_self_reporter=True)
    X, R = np.asarray(net.X), np.asarray(net.R)
    sup = np.nonzero(R)
    pick = np.sort(np.random.RandomState(0).choice(len(sup[0]), 200, replace=False))
    out = tuple(s[pick] for s in sup)
    Rt = R.copy()
    Rt[out] = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(X, R=Rt, K=2, seed=1, max_iter=20, num_realisations=1, keep_engine=True)
    try:
        assert m._rho_f is None
        got = m.heldout_loglik(out, X[out], mirror_counts(X, out), estimate="geometric")
        assert m._rho_f is None                           # scored where rho lives
        assert got["counts"][0].tolist()[0] == 200 and got["counts"][0, 3] == 0
        theta, lam, eta = plug_in_tables(m, m._engine, "geometric")
        assert np.allclose(theta, m.G_exp_theta_f) and np.allclose(lam, m.G_exp_lambda_f) and np.isclose(eta, m.G_exp_nu_f)
        want = heldout_loglik_np(m.rho_f, out, X[out], mirror_counts(X, out), theta, lam, eta, R=Rt)
        compare_entries(got, want, term_size(m.rho_f, out, X[out], mirror_counts(X, out), theta, lam, eta), 2, "model")
        mean = m.heldout_loglik(out, X[out], mirror_counts(X, out))                       # the posterior means
        assert not np.array_equal(mean["logp"], got["logp"])
        tmp = m.heldout_loglik(out, X[out], estimate="geometric", X=X, R=Rt)              # a temporary engine; mirror counts from X
        assert np.allclose(tmp["logp"], got["logp"], rtol=1e-12) and tmp["counts"][0, 3] == 0
        with pytest.raises(ValueError):
            m.heldout_loglik(out, X[out], estimate="mode")
    finally:
        m.close()
