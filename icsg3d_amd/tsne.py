"""The two-dimensional t-SNE map of the VAE's latent space (reference viz.py tsne_latent:
sklearn.manifold.TSNE(n_components=2).fit_transform(Zs)) on the MI355X engine, without scikit-learn.

- knn          exact k nearest neighbours of every row, squared euclidean distances in fp64 (ics_op_tsne_knn)
- affinities   scikit-learn's perplexity search on those distances (ics_op_tsne_affinities)
- Tsne         the handle: codes in (host rows or a VaeEngine's encoder output, device to device), P = (C + C^T) / sum,
               gradient descent with the repulsion summed exactly over all pairs -- scikit-learn's objective at angle = 0
- tsne         fit_transform: the embedding, kl_divergence_ and n_iter_
- latent_map   encode -> append -> run for batches of grids; the codes never reach the host
- pca_init     TSNE(init="pca")'s starting embedding, from the D x D covariance on the host

The schedule is TSNE._tsne's: early exaggeration 12 for 250 iterations at momentum 0.5, then momentum 0.8;
learning_rate "auto" = max(N / early_exaggeration / 4, 50); KL divergence and gradient norm every 50 iterations, with the
two stopping rules (n_iter_without_progress = 300, min_grad_norm = 1e-7).  Results are bit-identical run to run.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def n_neighbors(n, perplexity):
    """TSNE._fit: min(n_samples - 1, int(3 * perplexity + 1))"""
    return min(int(n) - 1, int(3.0 * perplexity + 1))


def knn(x, k):
    """x (N, D) float32 -> idx (N, k) int32, dist2 (N, k) float64, rows sorted by (distance, index), self excluded."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2:
        raise ValueError("x must be (N, D), got %s" % (x.shape,))
    n, dim = x.shape
    k = int(k)
    idx = np.empty((n, max(k, 0)), np.int32)
    d2 = np.empty((n, max(k, 0)), np.float64)
    L.check(L.load().ics_op_tsne_knn(L.fptr(x), n, dim, k, L.i32ptr(idx), L.f64ptr(d2)))
    return idx, d2


def conditional_probabilities(dist2, perplexity):
    """_binary_search_perplexity on float32(dist2 (N, k)) -> (N, k) float64."""
    d2 = np.ascontiguousarray(dist2, np.float64)
    if d2.ndim != 2:
        raise ValueError("dist2 must be (N, k), got %s" % (d2.shape,))
    p = np.empty_like(d2)
    L.check(L.load().ics_op_tsne_affinities(L.f64ptr(d2), d2.shape[0], d2.shape[1], float(perplexity), L.f64ptr(p)))
    return p


def affinities(x, perplexity=30.0):
    """x (N, D) -> idx (N, k), dist2 (N, k), cond_p (N, k): the neighbour graph and its conditional probabilities."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2 or len(x) < 2:
        raise ValueError("x must be (N >= 2, D), got %s" % (x.shape,))
    if perplexity >= len(x):
        raise ValueError("perplexity must be less than n_samples")
    idx, d2 = knn(x, n_neighbors(len(x), perplexity))
    return idx, d2, conditional_probabilities(d2, perplexity)


def pca_init(x):
    """TSNE(init="pca"): the first two principal components (signs as sklearn's svd_flip: the entry of largest magnitude
    of each component is positive), float32, scaled so that the first column's standard deviation is 1e-4.  Computed in
    float64 from the D x D covariance; a column that carries no variance (D = 1) is zero."""
    x = np.asarray(x, np.float64)
    n, dim = x.shape
    xc = x - x.mean(axis=0)
    w, v = np.linalg.eigh(xc.T @ xc)
    comp = v[:, ::-1][:, :2].T                                      # rows: components by decreasing eigenvalue
    if comp.shape[0] < 2:
        comp = np.concatenate([comp, np.zeros((2 - comp.shape[0], dim))])
    j = np.argmax(np.abs(comp), axis=1)
    sign = np.sign(comp[np.arange(2), j])
    sign[sign == 0] = 1.0
    y = (xc @ (comp * sign[:, None]).T).astype(np.float32)
    return (y / np.std(y[:, 0]) * 1e-4).astype(np.float32)


class Tsne:
    """One t-SNE problem on the device (include/icsg3d.h, ics_op_tsne_*)."""

    def __init__(self, dim, capacity, perplexity=30.0, early_exaggeration=12.0, max_iter=1000, exaggeration_iter=250,
                 n_iter_check=50, n_iter_without_progress=300, min_grad_norm=1e-7, learning_rate="auto",
                 n_components=2):
        self._lib = L.load()
        self._h = L._H(None)
        lr = -1.0 if learning_rate == "auto" else float(learning_rate)
        cfg = L.TsneConfig(int(dim), int(capacity), int(n_components), float(perplexity), float(early_exaggeration),
                           min(int(exaggeration_iter), int(max_iter)), int(max_iter), int(n_iter_check),
                           int(n_iter_without_progress), float(min_grad_norm), lr)
        L.check(self._lib.ics_op_tsne_create(C.byref(cfg), C.byref(self._h)))
        self.dim, self.capacity, self.perplexity = int(dim), int(capacity), float(perplexity)
        self.count = 0
        self.seconds = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ics_op_tsne_destroy(self._h)
            self._h = L._H(None)

    __del__ = close

    def append(self, codes):
        codes = np.ascontiguousarray(codes, np.float32)
        if codes.ndim != 2 or codes.shape[1] != self.dim:
            raise ValueError("codes must be (rows, %d), got %s" % (self.dim, codes.shape))
        L.check(self._lib.ics_op_tsne_append(self._h, L.fptr(codes), len(codes)))
        self.count += len(codes)

    def append_vae(self, vae, batch):
        """the z_mean rows of `vae`'s (VaeEngine) most recent encoder pass, device to device"""
        L.check(self._lib.ics_op_tsne_append_vae(self._h, vae._h, int(batch)))
        self.count += int(batch)

    def codes(self, rows=None):
        rows = self.count if rows is None else int(rows)
        out = np.empty((max(rows, 0), self.dim), np.float32)
        L.check(self._lib.ics_op_tsne_get_codes(self._h, L.fptr(out), rows))
        return out

    def prepare(self, init):
        """neighbours, affinities, symmetrisation; embedding = init (N, 2).  self.seconds = the three stages' wall time."""
        init = np.ascontiguousarray(init, np.float32)
        rows, cols = (init.shape if init.ndim == 2 else (init.size, 1))
        sec = np.zeros(3, np.float64)
        L.check(self._lib.ics_op_tsne_prepare(self._h, L.fptr(init), rows, cols, L.f64ptr(sec)))
        self.seconds = {"knn": sec[0], "affinities": sec[1], "symmetrise": sec[2]}

    def set_graph(self, indptr, indices, vals, init):
        indptr = np.ascontiguousarray(indptr, np.int64)
        indices = np.ascontiguousarray(indices, np.int32)
        vals = np.ascontiguousarray(vals, np.float64)
        init = np.ascontiguousarray(init, np.float32)
        rows, cols = (init.shape if init.ndim == 2 else (init.size, 1))
        L.check(self._lib.ics_op_tsne_set_graph(self._h, len(indptr) - 1, L.i64ptr(indptr), L.i32ptr(indices),
                                                L.f64ptr(vals), L.fptr(init), rows, cols))

    def graph(self):
        """P as CSR: indptr (N + 1) int64, indices int32, vals float64"""
        nnz, n = C.c_size_t(0), C.c_int(0)
        L.check(self._lib.ics_op_tsne_get_graph(self._h, None, None, None, 0, C.byref(nnz)))
        L.check(self._lib.ics_op_tsne_read(self._h, None, None, None, None, C.byref(n)))
        indptr = np.empty(n.value + 1, np.int64)
        indices = np.empty(nnz.value, np.int32)
        vals = np.empty(nnz.value, np.float64)
        L.check(self._lib.ics_op_tsne_get_graph(self._h, L.i64ptr(indptr), L.i32ptr(indices), L.f64ptr(vals), nnz.value,
                                                C.byref(nnz)))
        return indptr, indices, vals

    def gradient(self, y, exaggeration=1.0):
        """_kl_divergence_bh(angle=0) at y (N, 2) -> (kl, grad (N, 2) float32)"""
        y = np.ascontiguousarray(y, np.float32)
        grad = np.empty_like(y)
        kl = C.c_double(0.0)
        L.check(self._lib.ics_op_tsne_gradient(self._h, L.fptr(y), float(exaggeration), L.fptr(grad), C.byref(kl)))
        return kl.value, grad

    def run(self, iters):
        """up to `iters` more iterations; True once the descent has finished"""
        done = C.c_int(0)
        L.check(self._lib.ics_op_tsne_run(self._h, int(iters), C.byref(done)))
        return bool(done.value)

    def read(self, embedding=True):
        """-> dict(embedding (N, 2) float32 or None, kl_divergence, grad_norm, n_iter, count)"""
        kl, gn, it, n = C.c_double(0.0), C.c_double(0.0), C.c_int(0), C.c_int(0)
        L.check(self._lib.ics_op_tsne_read(self._h, None, C.byref(kl), C.byref(gn), C.byref(it), C.byref(n)))
        emb = None
        if embedding:
            emb = np.empty((n.value, 2), np.float32)
            L.check(self._lib.ics_op_tsne_read(self._h, L.fptr(emb), None, None, None, None))
        return {"embedding": emb, "kl_divergence": kl.value, "grad_norm": gn.value, "n_iter": it.value,
                "count": n.value}


class TsneResult:
    def __init__(self, embedding, kl_divergence, n_iter, seconds=None):
        self.embedding_, self.kl_divergence_, self.n_iter_, self.seconds = embedding, kl_divergence, n_iter, seconds

    def __iter__(self):                                            # embedding, kl, n_iter = tsne(x)
        return iter((self.embedding_, self.kl_divergence_, self.n_iter_))


def _finish(t, init, chunk):
    if isinstance(init, str):
        if init != "pca":
            raise ValueError("init must be 'pca' or an (N, 2) array")
        # the one host copy of the codes, D x D work; fewer than 2 codes: prepare refuses below
        init = pca_init(t.codes()) if t.count >= 2 else np.zeros((t.count, 2), np.float32)
    t.prepare(init)
    while not t.run(chunk):
        pass
    r = t.read()
    return TsneResult(r["embedding"], r["kl_divergence"], r["n_iter"], t.seconds)


def tsne(x, perplexity=30.0, early_exaggeration=12.0, max_iter=1000, init="pca", learning_rate="auto",
         exaggeration_iter=250, n_iter_without_progress=300, min_grad_norm=1e-7, n_components=2, chunk=250):
    """sklearn.manifold.TSNE(n_components=2, angle=0).fit(x): returns a TsneResult that unpacks as
    (embedding (N, 2) float32, kl_divergence_, n_iter_).  init: "pca" or an (N, 2) array."""
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 2:
        raise ValueError("x must be (N, D), got %s" % (x.shape,))
    t = Tsne(x.shape[1], max(len(x), 2), perplexity, early_exaggeration, max_iter, exaggeration_iter,
             n_iter_without_progress=n_iter_without_progress, min_grad_norm=min_grad_norm,
             learning_rate=learning_rate, n_components=n_components)
    try:
        if len(x):
            t.append(x)
        return _finish(t, init, chunk)
    finally:
        t.close()


def latent_map(vae, batches, capacity, perplexity=30.0, early_exaggeration=12.0, max_iter=1000, init="pca",
               learning_rate="auto", exaggeration_iter=250, chunk=250):
    """The map of the z_mean codes of `batches` -- an iterable of (x, cond) with at most vae.max_batch grids each --
    under `vae`, a VaeEngine (or a LatticeDFCVAE, whose engine is used): each batch is encoded and its z_mean appended
    device to device, then the descent runs.  capacity: an upper bound of the number of grids.  Equal bit for bit to
    tsne() on the same codes.  Returns a TsneResult."""
    eng = vae._engine(vae.batch_size, grow=True) if hasattr(vae, "_engine") else vae
    t = Tsne(eng.latent_dim, max(int(capacity), 2), perplexity, early_exaggeration, max_iter, exaggeration_iter,
             learning_rate=learning_rate)
    try:
        for x, cond in batches:
            x = np.asarray(x, np.float32)
            if len(x) > eng.max_batch:
                raise ValueError("a batch holds %d grids, the engine's max_batch is %d" % (len(x), eng.max_batch))
            eng.encode(x, cond, np.zeros((len(x), eng.latent_dim), np.float32))   # z_mean does not depend on eps
            t.append_vae(eng, len(x))
        return _finish(t, init, chunk)
    finally:
        t.close()
