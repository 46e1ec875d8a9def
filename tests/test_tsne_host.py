"""t-SNE without a GPU: tests/tsne_ref.py (the fp64 restatement the GPU tests hold the kernels to) reproduces what
scikit-learn recorded in tests/golden/tsne_golden.npz -- conditional probabilities, gradients, KL divergence, the
60-iteration trajectory, trustworthiness -- within twice the distance tests/golden/make_tsne_golden.py measured; the PCA
init of icsg3d_amd.tsne equals scikit-learn's; latent_map.py carries its flags; the script and the bench compile."""
import os
import py_compile
import subprocess
import sys

import numpy as np

import tsne_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_tsne_golden as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_golden.npz")


def _rank_unit(n, k=10):
    """what one rank changes trustworthiness by: embedded distances that tie to rounding (float32 embedding, scikit-learn's
    neighbour search against the restatement's fp64 distances) may order either way, a handful of units at most"""
    return 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))


def test_golden_file_is_small_and_complete():
    assert os.path.getsize(GOLDEN) < 100_000
    g = np.load(GOLDEN)
    for k in ("cond_a", "cond_b", "grad_rand", "grad_conv", "traj_y10", "traj_y60_pert", "run_kl_600", "run_kl_2000"):
        assert k in g.files
    assert all(g[k].ndim <= 2 and g[k].size <= 300 * 16 for k in g.files), "no dense N x N array belongs here"


def test_restatement_reproduces_the_conditional_probabilities():
    g = np.load(GOLDEN)
    for name, (seed, n, dim, perp, rows) in G.COND_CASES.items():
        x = R.clustered_codes(seed, n, dim)[0]
        idx, d2 = R.knn(x, min(n - 1, int(3.0 * perp + 1)))
        assert (idx != np.arange(n)[:, None]).all() and (np.diff(d2, axis=1) >= 0).all()
        sk = g["cond_" + name]
        plain = R.perplexity_search(d2[:rows], perp)
        faithful = R.perplexity_search(d2[:rows], perp, cast32=True)
        e_plain, e_faithful = np.max(np.abs(plain - sk)) / sk.max(), np.max(np.abs(faithful - sk)) / sk.max()
        print("cond %s: fp64-distance restatement %.3e (recorded %.3e), float32-distance restatement %.3e" %
              (name, e_plain, float(g["err_cond_" + name]), e_faithful))
        assert e_plain <= 2.0 * float(g["err_cond_" + name])
        assert e_faithful <= 1e-12
        assert (np.abs(R.entropy_gap(d2[:rows], faithful, perp)) <= 1e-5 + 1e-7).all()


def test_restatement_symmetrisation():
    seed, n, dim, perp, _ = G.COND_CASES["b"]
    x = R.clustered_codes(seed, n, dim)[0]
    idx, d2 = R.knn(x, 91)
    indptr, indices, vals = R.symmetrise(idx, R.perplexity_search(d2, perp, cast32=True))
    P = R.csr_dense(indptr, indices, vals, n)
    assert abs(vals.sum() - 1.0) <= 1e-12 and np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    assert indptr[-1] == len(indices) == len(vals) and (np.diff(indptr) >= 91).all()


def test_restatement_reproduces_gradient_and_kl():
    g = np.load(GOLDEN)
    seed, n, dim, perp = G.GRAD_CASE
    P = G.faithful_graph(R.clustered_codes(seed, n, dim)[0], perp)
    for tag, y in (("rand", G.random_embedding(seed + 1, n)), ("conv", g["grad_y_conv"])):
        kl, grad = R.kl_gradient(y, *P)
        e_g, e_kl = R.tensor_rel(g["grad_" + tag], grad), abs(float(g["kl_" + tag]) - kl) / abs(kl)
        print("gradient %s: sklearn vs restatement %.3e (recorded %.3e), KL %.3e (recorded %.3e)" %
              (tag, e_g, float(g["err_grad_" + tag]), e_kl, float(g["err_kl_" + tag])))
        assert e_g <= 2.0 * float(g["err_grad_" + tag]) and e_kl <= 2.0 * float(g["err_kl_" + tag])
        assert float(g["err_grad_" + tag]) < 1e-3 and float(g["err_kl_" + tag]) < 1e-5


def test_restatement_reproduces_the_trajectory():
    """the update rule in float32 on the fp64 gradient: inside scikit-learn's own sensitivity to a 1e-6 perturbation"""
    g = np.load(GOLDEN)
    seed, n, dim, perp = G.TRAJ_CASE
    P = G.faithful_graph(R.clustered_codes(seed, n, dim)[0], perp)
    kept, errors = R.descent(lambda y: R.kl_gradient(y, *P, exaggeration=G.EXAGGERATION), g["traj_init"], 60, 0.5,
                             G.learning_rate(n), keep=G.TRAJ_ITERS)
    for it in G.TRAJ_ITERS:
        mine = R.tensor_rel(kept[it], g["traj_y%d" % it])
        own = R.tensor_rel(g["traj_y%d_pert" % it], g["traj_y%d" % it])
        print("trajectory at %d: restatement vs sklearn %.3e, sklearn perturbed vs itself %.3e" % (it, mine, own))
        assert mine <= 2.0 * own
    assert abs(errors[50] - float(g["traj_kl50"])) <= 2.0 * abs(float(g["traj_kl50_pert"]) - float(g["traj_kl50"]))


def test_restated_trustworthiness_equals_sklearns():
    g = np.load(GOLDEN)
    x = R.clustered_codes(G.RUN_CASES["600"][0], 600, 256)[0]
    assert abs(R.trustworthiness(x, g["run_emb_600"], 10) - float(g["run_trust_600"][0])) <= 5 * _rank_unit(600)
    for name in G.RUN_CASES:
        assert abs(float(g["run_trust_check_" + name]) - float(g["run_trust_" + name][0])) <= 5 * _rank_unit(int(name))
        assert (g["run_iter_" + name] == 999).all()
        kls = g["run_kl_" + name]
        assert kls[:3].max() - kls[:3].min() < 0.01 * kls[0] and kls[3] > kls[:3].max()   # angle 0.5 ends higher


def test_pca_init_equals_sklearns():
    from icsg3d_amd.tsne import pca_init
    g = np.load(GOLDEN)
    seed, n, dim, _ = G.TRAJ_CASE
    got = pca_init(R.clustered_codes(seed, n, dim)[0])
    want = g["traj_init"]
    assert got.dtype == np.float32 and got.shape == want.shape
    print("pca init: max |difference| / max |entry| = %.3e" % (np.abs(got - want).max() / np.abs(want).max()))
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert abs(np.std(got[:, 0]) - 1e-4) <= 1e-9
    one = pca_init(np.arange(10, dtype=np.float32)[:, None])           # D = 1: the second column carries nothing
    assert one.shape == (10, 2) and (one[:, 1] == 0).all() and abs(np.std(one[:, 0]) - 1e-4) <= 1e-9


def test_package_does_not_import_sklearn_or_the_oracle():
    text = open(os.path.join(ROOT, "icsg3d_amd", "tsne.py")).read() + open(os.path.join(ROOT, "latent_map.py")).read()
    for word in ("import sklearn", "from sklearn", "import oracle", "from oracle", "import scipy", "from scipy"):
        assert word not in text


def test_latent_map_help_carries_the_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "latent_map.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    for flag in ("--name", "--samples", "--split", "--nrot", "--batch_size", "--d", "--ncond", "--target", "--perplexity",
                 "--max_iter", "--which", "--synthetic"):
        assert flag in r.stdout, flag
    assert "{val,train,all}" in r.stdout


def test_script_and_bench_compile(tmp_path):
    for f in ("latent_map.py", os.path.join("scripts", "tsne_bench.py"), os.path.join("tests", "golden", "make_tsne_golden.py")):
        py_compile.compile(os.path.join(ROOT, f), cfile=str(tmp_path / (os.path.basename(f) + "c")), doraise=True)
