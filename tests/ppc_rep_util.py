"""The contract of vmr_ppc_replicates / vmr_ppc_observed restated in NumPy, and the dense replicate composed from the entry
points that existed before them (CaviEngine.sample, a gather of lambda, vmr_generate_x): what the GPU tests hold the reduced
replicates to."""
import numpy as np

STAT_NAMES = ("n_pos", "total", "sumsq", "mutual", "ties_reported", "ties_agreed")


def stats_np(X, R=None):
    """(counts int64 [L, 6], by_reporter int64 [L, M, 2]) of dense X [L, N, N, M] over the support of R (None: everything)."""
    X = np.asarray(X).astype(np.int64)
    L, N, _, M = X.shape
    x = X if R is None else np.where(np.asarray(R) != 0, X, 0)
    pos = x > 0
    off = ~np.eye(N, dtype=bool)
    mutual = pos & pos.transpose(0, 2, 1, 3) & off[None, :, :, None]     # the mirror report is in S and positive too
    per_tie = pos.sum(axis=3)
    counts = np.stack([pos.sum(axis=(1, 2, 3)), x.sum(axis=(1, 2, 3)), (x * x).sum(axis=(1, 2, 3)), mutual.sum(axis=(1, 2, 3)),
                       (per_tie > 0).sum(axis=(1, 2)), (per_tie >= 2).sum(axis=(1, 2))], axis=1).astype(np.int64)
    by_reporter = np.stack([pos.sum(axis=(1, 2)), x.sum(axis=(1, 2))], axis=2).astype(np.int64)
    return counts, by_reporter


def stats_coo(subs, vals, r_subs, shape):
    """`stats_np` from coordinate lists (subs, vals of X; r_subs of the mask, None: everything), without a dense tensor."""
    L, N, _, M = shape
    key = np.ravel_multi_index(tuple(np.asarray(s, np.int64) for s in subs), shape)
    vals = np.asarray(vals, np.int64)
    keep = vals > 0
    if r_subs is not None:
        keep &= np.isin(key, np.ravel_multi_index(tuple(np.asarray(s, np.int64) for s in r_subs), shape))
    l, i, j, m = (np.asarray(s, np.int64)[keep] for s in subs)
    key, x = key[keep], vals[keep]
    mirror = np.ravel_multi_index((l, j, i, m), shape)
    mut = np.isin(mirror, key) & (i != j)
    tie = (l * N + i) * N + j
    ut, cnt = np.unique(tie, return_counts=True)
    tl = ut // (N * N)
    counts = np.zeros((L, 6), np.int64)
    by_reporter = np.zeros((L, M, 2), np.int64)
    for q in range(L):
        s = l == q
        counts[q] = [s.sum(), x[s].sum(), (x[s] * x[s]).sum(), mut[s].sum(), (tl == q).sum(), ((tl == q) & (cnt >= 2)).sum()]
        by_reporter[q, :, 0] = np.bincount(m[s], minlength=M)
        by_reporter[q, :, 1] = np.bincount(m[s], weights=x[s], minlength=M).astype(np.int64)
    return counts, by_reporter


def compose_replicate(eng, r, theta, lam, eta, seed_y, seed_x, n_trials=1):
    """Replicate r as a dense int64 [L, N, N, M] array, from the entry points that existed before vmr_ppc_replicates:
    Y = eng.sample(seed_y + r) on the device, lambda gathered from lam[r] at Y in torch, X = vmr_generate_x(lam, theta[r],
    eta[r], seed_x + r) with no mask (the caller applies R: a draw does not depend on it).  Counts are clamped at 255 there."""
    import torch
    from vimure_amd.synthetic import device_build_x
    dev = torch.device("cuda", eng.device)
    Y = torch.empty((eng.L, eng.N, eng.N), dtype=torch.uint8, device=dev)
    eng.sample((int(seed_y) + r) % 2 ** 64, n_trials, out=Y)
    table = torch.as_tensor(np.ascontiguousarray(lam[r], dtype=np.float64), device=dev)          # [L, K]
    lam_t = torch.gather(table, 1, Y.reshape(eng.L, -1).long()).reshape(eng.L, eng.N, eng.N).contiguous()
    X = device_build_x(None, np.asarray(theta[r], dtype=np.float64), float(eta[r]), (int(seed_x) + r) % 2 ** 64, lam=lam_t)
    torch.cuda.synchronize(dev)
    return X.cpu().numpy().astype(np.int64)
