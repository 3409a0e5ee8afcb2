"""GPU: the leave-one-reporter-out posterior of every element of the support (vmr_reporter_influence) against its NumPy
restatement (`influence.influence_np`), with the state set from synthetic arrays at the smallest shapes that reach every branch
and from the golden fits (the `fit_*_f` arrays).  tests/influence_util.py states what is compared exactly, why that is fair, and
the bounds of what is not.

Measured on an MI355X: see C_INF in tests/influence_util.py."""
import warnings

import numpy as np
import pytest

from tests.golden_util import load_case
from tests.influence_util import ROWS, VALS, bits, compare_sums, compare_values, engine, golden, pick, reference, synthetic

pytestmark = pytest.mark.gpu


def _slice(res, layer):
    """A result of all layers cut to one: the aggregates' row, the rows of that layer."""
    if layer is None:
        return res
    w = res["l"] == layer
    out = {k: (v[layer:layer + 1] if k in ("counts", "sums", "hist") and v is not None else v) for k, v in res.items()}
    out.update({k: res[k][w] for k in ROWS + VALS + ("lost", "gained")})
    return out


def _check(eng, c, what, method="rho_max", threshold=0.0, select="both", layer=None):
    from vimure_amd.engine import ReporterInfluenceArgumentError
    from vimure_amd.influence import influence_np
    ref = reference(c, method, threshold)
    al = ref["al"]
    min_tv, edges = pick(c, ref)
    kw = dict(method=method, threshold=threshold, select=select, min_tv=min_tv, layer=layer)
    want = influence_np(c["rho"], c["X"], c["R"], *c["tabs"], mutuality=c["mut"], edges=edges, **kw)
    got = eng.reporter_influence(*c["tabs"], edges=edges, **kw)
    # exact integers, and the set and order of the rows
    for k in ("counts", "hist"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ROWS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    for k in ("lost", "gained"):
        assert np.array_equal(got[k], want[k]), (what, k)
    n = int(want["counts"][:, :, 3].sum())
    assert len(got["l"]) == n and got["hist"].sum() == want["counts"][:, :, 0].sum()
    # every element's prob, prob_loo and tv, and the sums
    full = eng.reporter_influence(*c["tabs"], method=method, threshold=threshold, select="none", min_tv=0.0, layer=layer, flips=False)
    w = np.ones(len(al["l"]), bool) if layer is None else al["l"] == layer
    for k in ROWS:
        assert np.array_equal(full[k], al[k][w]), (what, "all rows", k)
    worst = compare_values(full, ref, w, what)
    if c["K"] == 2:
        r1 = np.ascontiguousarray(c["rho"][al["l"][w], al["i"][w], al["j"][w], 1])
        assert np.array_equal(bits(full["prob"]), bits(r1)), what             # prob is rho_1 bit for bit
    layers = list(range(c["rho"].shape[0])) if layer is None else [layer]
    compare_sums(got["sums"], got["counts"], ref, layers, c["X"].shape[1], what)
    assert np.array_equal(bits(full["sums"]), bits(got["sums"])) and np.array_equal(full["counts"][:, :, :3], got["counts"][:, :, :3])
    at = np.isin(np.ravel_multi_index(tuple(full[k] for k in "lijm"), c["X"].shape),
                 np.ravel_multi_index(tuple(got[k] for k in "lijm"), c["X"].shape))
    for k in VALS:
        assert np.array_equal(bits(full[k][at]), bits(got[k])), (what, k)
    # determinism
    again = eng.reporter_influence(*c["tabs"], edges=edges, **kw)
    for k in ("counts", "hist", "lost", "gained") + ROWS:
        assert np.array_equal(again[k], got[k]), (what, k)
    for k in ("sums",) + VALS:
        assert np.array_equal(bits(again[k]), bits(got[k])), (what, k)
    # size, capacity, aggregates alone
    assert eng.reporter_influence_size(*c["tabs"], **kw) == n
    if n:
        out = {k: np.full(n - 1, -7, np.int32) for k in ROWS}
        out.update({k: np.full(n - 1, -7.0) for k in VALS})
        with pytest.raises(ReporterInfluenceArgumentError, match="flagged"):
            eng.reporter_influence(*c["tabs"], out=out, **kw)
        assert all((v == -7).all() for v in out.values())
    agg = eng.reporter_influence(*c["tabs"], edges=edges, rows=False, **kw)
    assert agg["l"] is None and agg["tv"] is None
    for k in ("counts", "hist"):
        assert np.array_equal(agg[k], got[k]), (what, k)
    assert np.array_equal(bits(agg["sums"]), bits(got["sums"]))
    # the scope is the reporter table's
    rt = eng.reporter_table(layer=layer, outputs=("counts",))["counts"]
    assert np.array_equal(got["counts"][:, :, 0], rt[:, :, 0]), what
    print(f"{what}: {n} rows of {int(w.sum())} elements, lost {int(got['counts'][:, :, 1].sum())}, gained "
          f"{int(got['counts'][:, :, 2].sum())}; WORST RATIO {worst:.4f}")
    return got, want


# (the dense tiles hold at most 8 categories: K = 12 has the report lists alone)
@pytest.mark.parametrize("shape,layout", [(s, f) for s in ("M70_K3", "M70_K2", "N48_K2", "K12") for f in ("sparse", "dense", "coo")
                                          if (s, f) != ("K12", "dense")])
def test_synthetic_shapes(shape, layout, monkeypatch):
    if layout != "coo":
        monkeypatch.setenv("VMR_FORMAT", layout)
    c = synthetic(shape)
    eng = engine(c, coo=layout == "coo")
    try:
        assert eng.data_format()[0] == ("sparse" if layout == "coo" else layout) or c["K"] > 2
        got, _ = _check(eng, c, f"{shape} {layout}")
        if c["R"] is not None:      # both flip classes occur in the masked cases
            assert got["counts"][:, :, 1].sum() > 0 and got["counts"][:, :, 2].sum() > 0
            assert got["counts"][:, :, 0].sum() == int(c["R"].sum())
        else:
            assert got["counts"][:, :, 0].sum() == c["X"].size
    finally:
        eng.close()


def test_two_mask_words(monkeypatch):
    """The mask words of partial rows (the short reporter lists switched off): M = 70 takes two words."""
    monkeypatch.setenv("VMR_NO_RLISTS", "1")
    c = synthetic("M70_K3")
    eng = engine(c)
    try:
        assert eng.mask_format()[0] == "words"
        _check(eng, c, "M70_K3 words")
    finally:
        eng.close()


def test_mutuality_off():
    c = synthetic("M70_K2", mut=False)
    eng = engine(c)
    try:
        got, _ = _check(eng, c, "M70_K2 nomut")
        assert c["tabs"][4] == 0.0 and not got["xt"].any() and len(got["l"]) > 0
    finally:
        eng.close()


def test_threshold_readout_and_selections():
    c = synthetic("M70_K2")
    eng = engine(c)
    try:
        got, _ = _check(eng, c, "M70_K2 threshold 0.3", method="threshold", threshold=0.3)
        assert got["counts"][:, :, 1].sum() > 0 and got["counts"][:, :, 2].sum() > 0
        for select in ("none", "lost", "gained"):
            _check(eng, c, f"M70_K2 threshold 0.3 {select}", method="threshold", threshold=0.3, select=select)
        # min_tv = +inf: the flips alone
        only = eng.reporter_influence(*c["tabs"], method="threshold", threshold=0.3)
        assert len(only["l"]) == only["counts"][:, :, 1:3].sum() == only["counts"][:, :, 3].sum() and (only["lost"] ^ only["gained"]).all()
    finally:
        eng.close()


def test_one_layer_is_the_slice_of_all():
    c = synthetic("M70_K3")
    eng = engine(c)
    try:
        ref = reference(c)
        min_tv, edges = pick(c, ref)
        al = eng.reporter_influence(*c["tabs"], min_tv=min_tv, edges=edges)
        for layer in (0, 1):
            got, _ = _check(eng, c, f"M70_K3 layer {layer}", layer=layer)
            cut = _slice(al, layer)
            assert got["counts"].shape == (1, 70, 4) and set(got["l"].tolist()) == {layer}
            for k in ("counts", "hist", "lost", "gained") + ROWS:
                assert np.array_equal(got[k], cut[k]), k
            for k in ("sums",) + VALS:
                assert np.array_equal(bits(got[k]), bits(cut[k])), k
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "L_default_K12"])
def test_golden_fits(name):
    c = golden(name)
    eng = engine(c)
    try:
        got, _ = _check(eng, c, name)
        assert got["counts"][:, :, 0].sum() == (c["X"].size if c["R"] is None else int(c["R"].sum()))
    finally:
        eng.close()


def test_refusals():
    import ctypes
    from vimure_amd import CaviEngine, _lib
    from vimure_amd.engine import EngineError, ReporterInfluenceArgumentError
    from tests.influence_util import PRI
    c = golden("B_random_mask_K3")
    eng = CaviEngine(c["X"].astype(np.uint8), c["R"], K=c["K"], mutuality=c["mut"])
    eng.set_priors(*PRI)                          # no state yet: an argument is refused before the state is even looked at
    try:
        tabs = [np.ascontiguousarray(a, dtype=np.float64) for a in c["tabs"][:4]]
        L, M = tabs[0].shape
        cn, sm = np.zeros((L, M, _lib.INF_NCOUNT), np.uint64), np.zeros((L, M, _lib.INF_NSUM))
        ed = np.array([0.1, 0.2, 0.2, 0.9])
        hist = np.zeros((L, len(ed) + 1, 2), np.uint64)
        fn, fs = eng.lib.vmr_reporter_influence, eng.lib.vmr_reporter_influence_size
        n_out = ctypes.c_uint64(7)

        def call(h=eng._h, layer=-1, t=tabs, g_nu=0.3, method=0, select=3, min_tv=0.5, n_edges=len(ed), edges=ed, hist_=hist, outs=True):
            return fn(h, layer, *[None if a is None else a.ctypes.data for a in t], g_nu, method, 0.0, select, min_tv, n_edges,
                      None if edges is None else edges.ctypes.data, None if hist_ is None else hist_.ctypes.data,
                      cn.ctypes.data if outs else None, sm.ctypes.data if outs else None, 0, *([None] * 9), 0)

        def swap(q, v):
            t = [a.copy() for a in tabs]
            t[q][1, 2] = v
            return t
        assert call(h=None) == _lib.VMR_EINVAL
        for kw, word in ((dict(t=[None] + tabs[1:]), b"NULL"), (dict(t=swap(0, -0.5)), b"e_theta"), (dict(t=swap(0, np.inf)), b"e_theta"),
                         (dict(t=swap(1, np.nan)), b"elog_theta"), (dict(t=swap(1, -np.inf)), b"elog_theta"), (dict(t=swap(2, -1.0)), b"e_lambda"),
                         (dict(t=swap(3, np.inf)), b"elog_lambda"), (dict(g_nu=float("nan")), b"g_nu"), (dict(g_nu=-0.1), b"g_nu"),
                         (dict(method=1), b"method"), (dict(select=-1), b"select"), (dict(select=4), b"select"),
                         (dict(min_tv=float("nan")), b"min_tv"), (dict(min_tv=-0.1), b"min_tv"), (dict(layer=L), b"layer"),
                         (dict(hist_=None, outs=False), b"output"), (dict(n_edges=-1), b"n_edges"), (dict(n_edges=4097), b"n_edges"),
                         (dict(edges=None), b"edges"), (dict(edges=np.array([0.5, 0.4, 0.6, 0.7])), b"edges"),
                         (dict(edges=np.array([0.5, 0.6, np.inf, np.inf])), b"edges")):
            assert call(**kw) == _lib.VMR_EINVAL, kw
            msg = eng.lib.vmr_last_error(eng._h)
            assert b"vmr_reporter_influence" in msg and word in msg, (kw, msg)
        p4 = [a.ctypes.data for a in tabs]
        assert fs(eng._h, -1, *p4, 0.3, 0, 0.0, 4, 0.5, n_out) == _lib.VMR_EINVAL
        assert b"vmr_reporter_influence_size" in eng.lib.vmr_last_error(eng._h)
        assert call() == _lib.VMR_ESTATE and b"vmr_set_state" in eng.lib.vmr_last_error(eng._h)
        assert fs(eng._h, -1, *p4, 0.3, 0, 0.0, 3, 0.5, n_out) == _lib.VMR_ESTATE and n_out.value == 7
        assert not cn.any() and not sm.any() and not hist.any()                              # nothing was launched or written
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.reporter_influence(*c["tabs"])
        assert not isinstance(ei.value, ReporterInfluenceArgumentError)
        eng.set_state(*c["st"])
        assert call(min_tv=np.inf, select=0) == _lib.VMR_OK                                  # +inf and no flips: nothing is flagged
        assert cn[:, :, 0].sum() == int(c["R"].sum()) and cn[:, :, 3].sum() == 0 and hist.sum() == cn[:, :, 0].sum()
        for kw in (dict(select="all"), dict(layer=2), dict(edges=[1.0, 0.5]), dict(edges=np.zeros(4097)), dict(method="rho_mean"),
                   dict(method="mean"), dict(min_tv=-1.0)):
            with pytest.raises(ReporterInfluenceArgumentError):
                eng.reporter_influence(*c["tabs"], **kw)
        for t in ((tabs[0][:1],) + tuple(tabs[1:]), tuple(tabs[:3]) + (tabs[3][:, :1],), (None,) + tuple(tabs[1:])):
            with pytest.raises(ReporterInfluenceArgumentError):
                eng.reporter_influence(*t, 0.3)
        # a NaN in rho: reported after the pass, as a ValueError that is no argument error
        rho = c["rho"].copy()
        rho[0, 3, 4] = np.nan
        eng.set_state(*c["st"][:6], rho)
        with pytest.raises(ValueError, match="NaN") as ei:
            eng.reporter_influence(*c["tabs"])
        assert not isinstance(ei.value, ReporterInfluenceArgumentError)
    finally:
        eng.close()


def test_device_rows_and_snapshot_restore():
    import torch
    c = golden("B_random_mask_K3")
    eng = engine(c)
    try:
        min_tv, edges = pick(c, reference(c))
        host = eng.reporter_influence(*c["tabs"], min_tv=min_tv, edges=edges)
        dev = eng.reporter_influence(*c["tabs"], min_tv=min_tv, edges=edges, device=True)
        assert dev["tv"].is_cuda and dev["l"].dtype == torch.int32 and "lost" not in dev
        for k in ROWS:
            assert np.array_equal(dev[k].cpu().numpy(), host[k]), k
        for k in VALS:
            assert np.array_equal(bits(dev[k].cpu().numpy()), bits(host[k])), k
        assert np.array_equal(dev["hist"], host["hist"]) and np.array_equal(bits(dev["sums"]), bits(host["sums"]))
        eng.snapshot()
        eng.step(3)
        later = eng.reporter_influence(*c["tabs"], min_tv=min_tv, edges=edges)
        eng.restore()
        back = eng.reporter_influence(*c["tabs"], min_tv=min_tv, edges=edges)
        assert not np.array_equal(bits(later["sums"]), bits(host["sums"]))
        for k in ("sums",) + VALS:
            assert np.array_equal(bits(back[k]), bits(host[k])), k
        assert np.array_equal(back["hist"], host["hist"]) and np.array_equal(back["counts"], host["counts"])
    finally:
        eng.close()


def test_top_20_through_the_model():
    from vimure_amd import VimureModel
    d = load_case("A_ones_mut")
    X = np.asarray(d["X"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        assert m._rho_f is None
        full = m.reporter_influence(select="none", min_shift=0.0)                # the full table
        top = m.reporter_influence(top=20)
        flips = m.reporter_influence()
        assert m._rho_f is None                                                  # computed where rho lives
        f, t = full.rows(), top.rows()
        assert len(f) == X.size == full.counts[:, :, 0].sum() and len(t) == 20 == top.top
        order = np.lexsort((f["reporter"], f["target"], f["source"], f["layer"], -f["tv"]))[:20]
        want = f.iloc[order].reset_index(drop=True)
        for k in ("layer", "source", "target", "reporter", "x", "x_mirror", "lost", "gained"):
            assert np.array_equal(t[k], want[k]), k
        for k in ("prob", "prob_loo", "tv"):
            assert np.array_equal(bits(t[k]), bits(want[k])), k
        assert (np.diff(t["tv"]) <= 0).all() and t["tv"].iloc[-1] >= np.sort(f["tv"].to_numpy())[-20]
        assert top.hist.shape == (1, 4097, 2) and top.hist.sum() == X.size and top.edges[1] == 2.0 ** -12
        # the flips alone, and the frame
        assert len(flips) == flips.counts[:, :, 1:3].sum() == (f["lost"] | f["gained"]).sum()
        assert len(flips.fragile_ties()) == flips.counts[:, :, 1].sum() == f["lost"].sum()
        fr = full.frame()
        assert len(fr) == X.shape[3] and np.array_equal(fr["n_scope"], np.full(X.shape[3], X.shape[1] ** 2))
        assert np.array_equal(fr["lost"], flips.frame()["lost"]) and (fr["mean_tv"] >= 0).all()
        one = m.reporter_influence(top=10 ** 9)                                   # more than there are: everything, sorted
        assert len(one) == X.size
        with pytest.raises(ValueError, match="max_rows"):
            m.reporter_influence(top=10 ** 9, max_rows=10)
    finally:
        m.close()
