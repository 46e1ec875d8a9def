#!/usr/bin/env python3
"""Records tests/golden/tsne_golden.npz from scikit-learn (1.7.2 when this was run): what sklearn.manifold's own
functions return on inputs the tests regenerate from seeds, and how far tests/tsne_ref.py (the fp64 restatement) is from
them.  Results only -- no dense N x N array, no inputs other than embeddings that cannot be regenerated.

    python tests/golden/make_tsne_golden.py          (CPU, needs scikit-learn and scipy; a few minutes)

Cases (seeds and shapes are the CASES / RUNS tables below; the tests import them from here):
  cond_*      _binary_search_perplexity on float32 of the restatement's fp64 neighbour distances, rows in (distance,
              index) order; err_cond_* = max |restatement(fp64 distances) - sklearn| over the largest entry, and
              err_joint_* the same for the symmetrised P.
  grad_*      _kl_divergence_bh(angle=0.0) at a random and at a near-converged embedding (N = 600): gradient, KL, and the
              tensor-relative distance of each from the restatement (err_grad_*, err_kl_*).
  traj_*      _gradient_descent on that objective with P * 12, momentum 0.5, from a stored init: embeddings after 10, 30
              and 60 iterations, the KL at iteration 50; the same from the init perturbed by 1e-6 relative.
  run_*       TSNE(...).fit at N = 600 and 2000, 1000 iterations: kl_divergence_, n_iter_ and trustworthiness at angle = 0
              from the PCA init and from two 1e-6 perturbed inits, and at the default angle = 0.5.
  traj_init   is PCA(n_components=2, svd_solver="full").fit_transform scaled as TSNE scales it (the PCA test reads it).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tsne_ref as R  # noqa: E402

# name: (seed, N, D, perplexity, rows stored)
COND_CASES = {"a": (11, 300, 256, 5.0, 300), "b": (12, 120, 256, 30.0, 16)}
GRAD_CASE = (21, 600, 256, 30.0)          # seed, N, D, perplexity; the random embedding is random_embedding(22, 600)
TRAJ_CASE = (31, 300, 256, 30.0)
TRAJ_ITERS = (10, 30, 60)
RUN_CASES = {"600": (41, 600), "2000": (42, 2000)}
EXAGGERATION = 12.0


def random_embedding(seed, n):
    return (np.random.default_rng(seed).normal(size=(n, 2)) * 5.0).astype(np.float32)


def perturbed(init, seed):
    g = np.random.default_rng(seed).normal(size=init.shape)
    return (init.astype(np.float64) * (1.0 + 1e-6 * g)).astype(np.float32)


def learning_rate(n):
    return max(n / EXAGGERATION / 4.0, 50.0)


def faithful_graph(x, perplexity):
    """the restatement's P in scikit-learn's own arithmetic (float32 distances): indptr, indices, vals"""
    k = min(len(x) - 1, int(3.0 * perplexity + 1))
    idx, d2 = R.knn(x, k)
    return R.symmetrise(idx, R.perplexity_search(d2, perplexity, cast32=True))


def sk_pca_init(x):
    from sklearn.decomposition import PCA
    y = PCA(n_components=2, svd_solver="full").fit_transform(x).astype(np.float32, copy=False)
    return (y / np.std(y[:, 0]) * 1e-4).astype(np.float32)


def main():
    from scipy.sparse import csr_matrix
    from sklearn.manifold import TSNE, _t_sne, _utils, trustworthiness
    out = {}

    for name, (seed, n, dim, perp, rows) in COND_CASES.items():
        x, _ = R.clustered_codes(seed, n, dim)
        k = min(n - 1, int(3.0 * perp + 1))
        idx, d2 = R.knn(x, k)
        sk = _utils._binary_search_perplexity(d2.astype(np.float32), perp, 0)
        ref = R.perplexity_search(d2, perp)
        out["cond_" + name] = sk[:rows]
        out["err_cond_" + name] = np.max(np.abs(ref - sk)) / np.max(sk)
        pj_sk, pj_ref = R.symmetrise(idx, sk)[2], R.symmetrise(idx, ref)[2]
        out["err_joint_" + name] = np.max(np.abs(pj_ref - pj_sk)) / np.max(pj_sk)
        print("cond", name, "restatement vs sklearn:", out["err_cond_" + name], "joint:", out["err_joint_" + name])

    def objective(P, n, exaggeration):
        Pm = csr_matrix((P[2] * exaggeration, P[1], P[0]), shape=(n, n))
        return lambda y, compute_error=True: _t_sne._kl_divergence_bh(
            np.asarray(y, np.float32).ravel(), Pm, 1, n, 2, angle=0.0, skip_num_points=0, verbose=0,
            compute_error=compute_error, num_threads=1)

    # whole runs first: the near-converged embedding of the gradient case comes from one of them
    seed, n, dim, perp = GRAD_CASE
    xg, _ = R.clustered_codes(seed, n, dim)
    y_conv = TSNE(n_components=2, perplexity=perp, init=sk_pca_init(xg), angle=0.0, random_state=0).fit_transform(xg)
    out["grad_y_conv"] = y_conv.astype(np.float32)
    P = faithful_graph(xg, perp)
    for tag, y in (("rand", random_embedding(seed + 1, n)), ("conv", out["grad_y_conv"])):
        kl, g = objective(P, n, 1.0)(y)
        kl_ref, g_ref = R.kl_gradient(y, *P)
        out["grad_" + tag] = g.reshape(n, 2).astype(np.float32)
        out["kl_" + tag] = np.float64(kl)
        out["err_grad_" + tag] = R.tensor_rel(g.reshape(n, 2), g_ref)
        out["err_kl_" + tag] = abs(kl - kl_ref) / abs(kl_ref)
        print("grad", tag, "sklearn vs restatement:", out["err_grad_" + tag], "kl:", out["err_kl_" + tag], kl, kl_ref)

    seed, n, dim, perp = TRAJ_CASE
    xt, _ = R.clustered_codes(seed, n, dim)
    P = faithful_graph(xt, perp)
    obj = objective(P, n, EXAGGERATION)
    init = sk_pca_init(xt)
    out["traj_init"] = init
    for tag, y0 in (("", init), ("_pert", perturbed(init, seed + 1))):
        for it in TRAJ_ITERS + (50,):
            p, err, _ = _t_sne._gradient_descent(obj, y0.ravel().copy(), it=0, max_iter=it, n_iter_check=50, momentum=0.5,
                                                 learning_rate=learning_rate(n), n_iter_without_progress=250,
                                                 min_grad_norm=1e-7, verbose=0)
            if it == 50:
                out["traj_kl50" + tag] = np.float64(err)
            else:
                out["traj_y%d%s" % (it, tag)] = p.reshape(n, 2).astype(np.float32)
    for it in TRAJ_ITERS:
        print("trajectory: perturbed vs unperturbed at", it,
              R.tensor_rel(out["traj_y%d_pert" % it], out["traj_y%d" % it]))
    print("trajectory kl50:", out["traj_kl50"], out["traj_kl50_pert"])

    for name, (seed, n) in RUN_CASES.items():
        x, _ = R.clustered_codes(seed, n, 256)
        init = sk_pca_init(x)
        kls, trusts, iters = [], [], []
        for tag, y0, angle in (("pca", init, 0.0), ("p1", perturbed(init, seed + 1), 0.0),
                               ("p2", perturbed(init, seed + 2), 0.0), ("bh", init, 0.5)):
            t = TSNE(n_components=2, perplexity=30.0, init=y0, angle=angle, random_state=0)
            e = t.fit_transform(x)
            kls.append(t.kl_divergence_); iters.append(t.n_iter_)
            trusts.append(trustworthiness(x, e, n_neighbors=10))
            if tag == "pca":
                out["run_trust_check_" + name] = np.float64(R.trustworthiness(x, e, 10))
                if n == 600:
                    out["run_emb_600"] = e.astype(np.float32)
            print("run", name, tag, kls[-1], iters[-1], trusts[-1])
        out["run_kl_" + name] = np.array(kls)              # [pca, p1, p2 at angle 0; angle 0.5]
        out["run_trust_" + name] = np.array(trusts)
        out["run_iter_" + name] = np.array(iters)

    path = os.path.join(HERE, "tsne_golden.npz")
    np.savez_compressed(path, sklearn_version=np.array(__import__("sklearn").__version__), **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
