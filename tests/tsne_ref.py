"""fp64 numpy restatement of the t-SNE pieces icsg3d_amd/csrc/tsne.hip computes (a helper, like h5ref.py): brute-force
neighbours, the perplexity search, the symmetrisation, the exact (all-pairs) gradient / KL divergence, the update rule
and trustworthiness.  Dense N x N work: for test sizes only.  No scikit-learn here; tests/golden/make_tsne_golden.py
records how far this file is from scikit-learn, and the tests hold the device to multiples of that distance."""
import numpy as np


def clustered_codes(seed, n, dim=256, clusters=8, spread=4.0):
    """the test inputs: `clusters` Gaussian blobs of float32 codes"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(clusters, dim)) * spread
    lab = rng.integers(0, clusters, size=n)
    return (centres[lab] + rng.normal(size=(n, dim))).astype(np.float32), lab


def sqdist(x):
    """(N, N) squared distances of float32 rows: differences and squares in fp64, summed in dimension order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    d = np.zeros((len(x), len(x)))
    for j in range(x.shape[1]):
        t = x[:, None, j] - x[None, :, j]
        d += t * t
    return d


def sqdist_block(x, r0, r1):
    """rows r0:r1 of sqdist(x) in one broadcast (fp64 differences, numpy's summation order: within 2^-45 of sqdist)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    t = x[r0:r1, None, :] - x[None, :, :]
    return np.einsum("ijk,ijk->ij", t, t)


def knn(x, k):
    """idx (N, k), dist2 (N, k): the k nearest other rows sorted by (distance, index)"""
    d = sqdist(x)
    n = len(d)
    np.fill_diagonal(d, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d), axis=1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(d, order, axis=1)


def entropy_gap(dist2, p, perplexity):
    """H(p) - log(perplexity) per row, fp64, for conditional probabilities p over distances dist2: with
    p_j = exp(-beta d_j) / s,  H = log s + beta sum d_j p_j = -sum p_j log p_j"""
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.sum(np.where(p > 0, p * np.log(p), 0.0), axis=1)
    return h - np.log(perplexity)


def perplexity_search(dist2, perplexity, cast32=False):
    """_binary_search_perplexity in fp64.  cast32=False: on the fp64 distances, tolerance 1e-5 as a double -- the plain
    fp64 form; cast32=True: on float32(dist2) with the C-float constants, scikit-learn's own arithmetic."""
    d = np.asarray(dist2, np.float64)
    tol, floor = 1e-5, 1e-8
    if cast32:
        d = d.astype(np.float32).astype(np.float64)
        tol, floor = float(np.float32(1e-5)), float(np.float32(1e-8))
        perplexity = float(np.float32(perplexity))
    want = np.log(perplexity)
    out = np.zeros_like(d)
    for i in range(len(d)):
        lo, hi, beta = -np.inf, np.inf, 1.0
        for _ in range(100):
            p = np.exp(-d[i] * beta)
            s = p.sum()
            if s == 0.0:
                s = floor
            p = p / s
            diff = np.log(s) + beta * np.sum(d[i] * p) - want
            if abs(diff) <= tol:
                break
            if diff > 0.0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        out[i] = p
    return out


def symmetrise(idx, cond_p):
    """P = (C + C^T) / sum as CSR with ascending columns: indptr int64, indices int32, vals float64"""
    n, k = idx.shape
    dense = np.zeros((n, n))
    dense[np.arange(n)[:, None], idx] = cond_p
    dense = dense + dense.T
    mask = np.zeros((n, n), bool)
    mask[np.arange(n)[:, None], idx] = True
    mask |= mask.T
    total = max(dense[mask].sum(), np.finfo(np.float64).eps)
    indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(mask)
    return indptr, cols.astype(np.int32), dense[rows, cols] / total


def csr_dense(indptr, indices, vals, n):
    out = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    out[rows, indices] = vals
    return out


def kl_gradient(y, indptr, indices, vals, exaggeration=1.0):
    """(kl, grad (N, 2)) of the t-SNE objective with exact repulsion, everything fp64, on float32(P * exaggeration) and
    the float32 embedding -- the inputs _kl_divergence_bh hands its kernel."""
    y = np.asarray(y, np.float32).astype(np.float64)
    n = len(y)
    p = (np.asarray(vals, np.float64) * exaggeration).astype(np.float32).astype(np.float64)
    diff = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + np.sum(diff * diff, axis=2))
    np.fill_diagonal(q, 0.0)
    z = max(q.sum(), np.finfo(np.float64).eps)
    rep = np.einsum("ij,ijc->ic", q * q, diff) / z
    rows = np.repeat(np.arange(n), np.diff(indptr))
    qe = q[rows, indices]
    att = np.zeros((n, 2))
    np.add.at(att, rows, (p * qe)[:, None] * diff[rows, indices])
    tiny = float(np.finfo(np.float32).tiny)
    kl = float(np.sum(p * np.log(np.maximum(p, tiny) / np.maximum(qe / z, tiny))))
    return kl, 4.0 * (att - rep)


def descent(objective, y0, n_iter, momentum, learning_rate, n_iter_check=50, keep=()):
    """_gradient_descent's update rule in float32 on objective(y) -> (kl, grad): returns the embeddings at the
    iterations in `keep` (1-based: after that many updates) and {iteration: kl} at the checks."""
    p = np.asarray(y0, np.float32).copy()
    update = np.zeros_like(p)
    gains = np.ones_like(p)
    kept, errors = {}, {}
    for i in range(n_iter):
        kl, grad = objective(p)
        grad = np.asarray(grad, np.float32)
        inc = update * grad < 0.0
        gains[inc] += np.float32(0.2)
        gains[~inc] *= np.float32(0.8)
        np.clip(gains, np.float32(0.01), np.inf, out=gains)
        grad = grad * gains
        update = np.float32(momentum) * update - np.float32(learning_rate) * grad
        p = p + update
        if (i + 1) % n_iter_check == 0:
            errors[i + 1] = kl
        if i + 1 in keep:
            kept[i + 1] = p.copy()
    return kept, errors


def trustworthiness(x, emb, n_neighbors=10):
    """sklearn.manifold.trustworthiness(X, E, n_neighbors) restated: ranks in the input space of each point's
    n_neighbors nearest embedded neighbours"""
    x = np.asarray(x, np.float64)
    e = np.asarray(emb, np.float64)
    n = len(x)
    dx = np.sqrt(np.maximum(sqdist_fast(x), 0.0))
    np.fill_diagonal(dx, np.inf)
    ind_x = np.argsort(dx, axis=1)
    de = sqdist_fast(e)
    np.fill_diagonal(de, np.inf)
    ind_e = np.argsort(de, axis=1, kind="stable")[:, :n_neighbors]
    inv = np.zeros((n, n), dtype=int)
    inv[np.arange(n)[:, None], ind_x] = np.arange(1, n + 1)
    ranks = inv[np.arange(n)[:, None], ind_e] - n_neighbors
    t = np.sum(ranks[ranks > 0])
    return 1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0)))


def sqdist_fast(x):
    """(N, N) squared distances by broadcasting over blocks (fp64), for the larger N of trustworthiness"""
    x = np.asarray(x, np.float64)
    sq = np.sum(x * x, axis=1)
    d = sq[:, None] + sq[None, :] - 2.0 * (x @ x.T)
    return np.maximum(d, 0.0)


def tensor_rel(a, b):
    """|a - b| / |b| over the whole tensor (2-norms)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
