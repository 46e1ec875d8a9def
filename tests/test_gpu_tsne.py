"""The t-SNE map on the MI355X (icsg3d_amd/csrc/tsne.hip) held to scikit-learn through tests/golden/tsne_golden.npz
(recorded by tests/golden/make_tsne_golden.py) and to the fp64 restatement tests/tsne_ref.py: neighbours under derived
bounds; affinities by scikit-learn's own acceptance and against its recorded probabilities; gradient, KL divergence and
a 60-iteration trajectory under multiples of scikit-learn's own recorded error / sensitivity; whole runs; determinism; the
device-resident path; the refusals; the script.  The whole file also passes under ICSG3D_DEBUG_CANARY=1."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tsne_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_tsne_golden as G  # noqa: E402  (the case tables and input generators; its sklearn imports are inside main)

GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_golden.npz")


def _rank_unit(n, k=10):
    """what one rank changes trustworthiness by: embedded distances that tie to rounding (float32 embedding, scikit-learn's
    neighbour search against the restatement's fp64 distances) may order either way, a handful of units at most"""
    return 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ---------------------------------------------------------------- 1. neighbours
def _check_knn(x, k, exact=None):
    """the issue's bounds: every returned neighbour within (1 + 2^-40) of the restated k-th smallest distance, no
    duplicates, no self, returned distances within 1e-12 relative, non-decreasing, ties to the lower index"""
    from icsg3d_amd.tsne import knn
    idx, d2 = knn(x, k)
    n = len(x)
    assert idx.shape == (n, k) and d2.shape == (n, k) and idx.dtype == np.int32 and d2.dtype == np.float64
    assert (idx >= 0).all() and (idx < n).all()
    assert (idx != np.arange(n)[:, None]).all(), "self among the neighbours"
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all(), "duplicate neighbours"
    assert (np.diff(d2, axis=1) >= 0).all(), "distances decrease along a row"
    tie = np.diff(d2, axis=1) == 0
    assert (np.diff(idx, axis=1)[tie] > 0).all(), "ties are not in index order"
    worst_kth, worst_rel = 0.0, 0.0
    small = R.sqdist(x) if exact is None and n <= 400 else None      # dimension order; blocks above that
    for r0 in range(0, n, 32):
        r1 = min(n, r0 + 32)
        full = small[r0:r1].copy() if small is not None else R.sqdist_block(x, r0, r1)
        rows = np.arange(r0, r1)
        full[rows - r0, rows] = np.inf
        kth = np.partition(full, k - 1, axis=1)[:, k - 1]
        mine = np.take_along_axis(full, idx[r0:r1].astype(np.int64), axis=1)
        assert (mine <= kth[:, None] * (1 + 2.0 ** -40)).all(), "a returned neighbour is not among the k nearest"
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(mine > 0, np.abs(d2[r0:r1] - mine) / mine, np.abs(d2[r0:r1]))
        worst_rel = max(worst_rel, float(rel.max()))
        worst_kth = max(worst_kth, float((mine / np.maximum(kth[:, None], 1e-300)).max()))
    print("knn N=%d D=%d k=%d: max returned/kth = 1 + %.2e, max distance error %.2e" %
          (n, x.shape[1], k, worst_kth - 1, worst_rel))
    assert worst_rel <= 1e-12
    return idx, d2


@pytest.mark.parametrize("n,dim,perp", [(2, 1, 1.0), (3, 7, 2.0), (92, 300, 30.0), (93, 256, 30.0), (93, 1, 30.0),
                                        (300, 7, 5.0), (200, 256, 60.0)])
def test_knn_odd_shapes(n, dim, perp):
    from icsg3d_amd.tsne import n_neighbors
    x = R.clustered_codes(100 + n + dim, n, dim, clusters=min(3, n))[0]
    _check_knn(x, n_neighbors(n, perp))


def test_knn_5000_by_256():
    x = R.clustered_codes(7, 5000, 256)[0]
    _check_knn(x, 91, exact=False)


def test_knn_duplicated_points_tie_to_the_lower_index():
    x = R.clustered_codes(8, 150, 16, clusters=2)[0]
    x[50:100] = x[:50]                      # every point of the first 50 twice
    x[140:150] = x[139]                     # and one point eleven times
    idx, d2 = _check_knn(x, 20)
    assert (d2[:50, 0] == 0).all() and (idx[:50, 0] == np.arange(50, 100)).all()
    assert (idx[50:100, 0] == np.arange(50)).all()
    assert (idx[149, :10] == np.arange(139, 149)).all() and (d2[149, :10] == 0).all()


# ---------------------------------------------------------------- 2. affinities
@pytest.mark.parametrize("name", sorted(G.COND_CASES))
def test_affinities_meet_sklearns_acceptance_and_its_probabilities(name):
    from icsg3d_amd.tsne import Tsne, affinities, pca_init
    g = np.load(GOLDEN)
    seed, n, dim, perp, rows = G.COND_CASES[name]
    x = R.clustered_codes(seed, n, dim)[0]
    idx, d2, cp = affinities(x, perp)
    ref_idx, ref_d2 = R.knn(x, idx.shape[1])
    assert np.array_equal(idx, ref_idx)
    # scikit-learn's own acceptance per row, recomputed in fp64 on the float32 distances it searches on
    d32 = d2.astype(np.float32).astype(np.float64)
    beta_h = -np.sum(np.where(cp > 0, cp * np.log(np.where(cp > 0, cp, 1.0)), 0.0), axis=1)
    gap = np.abs(beta_h - np.log(perp))
    print("affinities %s: worst |H - log(perplexity)| = %.3e over %d rows" % (name, gap.max(), n))
    assert (gap <= 1e-5 + 1e-7).all()
    assert np.allclose(cp.sum(axis=1), 1.0, rtol=0, atol=1e-12) and (cp >= 0).all() and d32.shape == cp.shape
    err = np.max(np.abs(cp[:rows] - g["cond_" + name])) / np.max(g["cond_" + name])
    bound = 2.0 * float(g["err_cond_" + name])
    print("affinities %s: device vs sklearn %.3e of the largest entry (bound %.3e)" % (name, err, bound))
    assert err <= bound
    # the symmetrised P of the handle
    t = Tsne(dim, n, perplexity=perp)
    t.append(x)
    t.prepare(pca_init(x))
    indptr, indices, vals = t.graph()
    t.close()
    assert abs(vals.sum() - 1.0) <= 1e-12
    P = R.csr_dense(indptr, indices, vals, n)
    assert np.array_equal(_bits(P), _bits(P.T.copy())), "P is not exactly symmetric"
    assert (np.diff(indptr) >= idx.shape[1]).all()
    for i in (0, n // 2, n - 1):
        assert (np.diff(indices[indptr[i]:indptr[i + 1]]) > 0).all(), "columns of a row are not ascending"
    ri, rj, rv = R.symmetrise(idx, cp)
    assert np.array_equal(indptr, ri) and np.array_equal(indices, rj)
    assert np.max(np.abs(vals - rv)) <= 1e-15 * np.max(rv) * 4


# ---------------------------------------------------------------- 3. gradient and KL
def _graph_handle(x, perp, init, **kw):
    from icsg3d_amd.tsne import Tsne
    P = G.faithful_graph(x, perp)
    t = Tsne(x.shape[1], len(x), perplexity=perp, **kw)
    t.set_graph(P[0], P[1], P[2], init)
    return t, P


@pytest.mark.parametrize("tag", ["rand", "conv"])
def test_gradient_and_kl_within_twice_sklearns_own_error(tag):
    g = np.load(GOLDEN)
    seed, n, dim, perp = G.GRAD_CASE
    x = R.clustered_codes(seed, n, dim)[0]
    y = G.random_embedding(seed + 1, n) if tag == "rand" else g["grad_y_conv"]
    t, P = _graph_handle(x, perp, y)
    kl, grad = t.gradient(y)
    t.close()
    kl_ref, g_ref = R.kl_gradient(y, *P)
    e_g, e_kl = R.tensor_rel(grad, g_ref), abs(kl - kl_ref) / abs(kl_ref)
    sk_g, sk_kl = R.tensor_rel(g["grad_" + tag], g_ref), abs(float(g["kl_" + tag]) - kl_ref) / abs(kl_ref)
    print("gradient %s: device vs restatement %.3e (sklearn %.3e, recorded %.3e); KL %.9f, error %.3e (sklearn %.3e)" %
          (tag, e_g, sk_g, float(g["err_grad_" + tag]), kl, e_kl, float(g["err_kl_" + tag])))
    assert e_g <= 2.0 * float(g["err_grad_" + tag])
    assert e_kl <= 2.0 * float(g["err_kl_" + tag])


# ---------------------------------------------------------------- 4. trajectory
def test_trajectory_within_twice_sklearns_own_sensitivity():
    g = np.load(GOLDEN)
    seed, n, dim, perp = G.TRAJ_CASE
    x = R.clustered_codes(seed, n, dim)[0]
    t, _ = _graph_handle(x, perp, g["traj_init"])
    done = 0
    for it in G.TRAJ_ITERS:
        assert not t.run(it - done)
        done = it
        r = t.read()
        assert r["n_iter"] == it - 1
        mine = R.tensor_rel(r["embedding"], g["traj_y%d" % it])
        own = R.tensor_rel(g["traj_y%d_pert" % it], g["traj_y%d" % it])
        print("trajectory at %d: device vs sklearn %.3e, sklearn perturbed vs itself %.3e" % (it, mine, own))
        assert mine <= 2.0 * own
    kl50, own = r["kl_divergence"], abs(float(g["traj_kl50_pert"]) - float(g["traj_kl50"]))
    print("KL at iteration 50: device %.6f sklearn %.6f (perturbed differs by %.3e)" % (kl50, float(g["traj_kl50"]), own))
    assert abs(kl50 - float(g["traj_kl50"])) <= 2.0 * own
    t.close()


# ---------------------------------------------------------------- 5. whole runs
@pytest.mark.parametrize("name", sorted(G.RUN_CASES))
def test_whole_run_matches_sklearn_quality(name):
    from icsg3d_amd.tsne import tsne
    g = np.load(GOLDEN)
    seed, n = G.RUN_CASES[name]
    x = R.clustered_codes(seed, n, 256)[0]
    if name == "600":                       # the trustworthiness restatement on scikit-learn's own embedding
        assert abs(R.trustworthiness(x, g["run_emb_600"], 10) - float(g["run_trust_600"][0])) <= 5 * _rank_unit(600)
    assert abs(float(g["run_trust_check_" + name]) - float(g["run_trust_" + name][0])) <= 5 * _rank_unit(int(name))
    emb, kl, n_iter = tsne(x, perplexity=30.0, max_iter=1000, init="pca")
    kls, trusts = g["run_kl_" + name][:3], g["run_trust_" + name][:3]
    trust = R.trustworthiness(x, emb, 10)
    print("run N=%d: KL %.4f (sklearn angle=0 %.4f..%.4f, angle=0.5 %.4f), trustworthiness %.4f (sklearn %.4f..%.4f), "
          "n_iter %d" % (n, kl, kls.min(), kls.max(), g["run_kl_" + name][3], trust, trusts.min(), trusts.max(), n_iter))
    assert n_iter == int(g["run_iter_" + name][0]) == 999
    assert np.isfinite(emb).all() and emb.shape == (n, 2) and emb.dtype == np.float32
    assert kl <= kls[0] + 3.0 * (kls.max() - kls.min())
    assert trust >= trusts[0] - 3.0 * (trusts.max() - trusts.min())


def test_schedule_switches_after_the_exaggeration_phase():
    """250 iterations with P * 12 at momentum 0.5, then P at momentum 0.8 with fresh gains: the KL reported at the check of
    iteration 250 is that of the exaggerated P, at 300 that of P -- the restatement tells which"""
    seed, n, dim, perp = G.TRAJ_CASE
    x = R.clustered_codes(seed, n, dim)[0]
    g = np.load(GOLDEN)
    t, P = _graph_handle(x, perp, g["traj_init"])
    t.run(249)
    y249 = t.read()["embedding"]
    t.run(1)
    kl250 = t.read()["kl_divergence"]
    ref250 = R.kl_gradient(y249, *P, exaggeration=12.0)[0]
    t.run(49)
    y299 = t.read()["embedding"]
    t.run(1)
    r = t.read()
    ref300 = R.kl_gradient(y299, *P, exaggeration=1.0)[0]
    t.close()
    print("KL at 250: %.6f (restated, exaggerated P: %.6f); at 300: %.6f (restated, P: %.6f)" % (kl250, ref250, r["kl_divergence"], ref300))
    assert abs(kl250 - ref250) <= 1e-5 * abs(ref250) and abs(r["kl_divergence"] - ref300) <= 1e-5 * abs(ref300)
    assert r["n_iter"] == 299


# ---------------------------------------------------------------- 6. determinism
def test_two_runs_give_the_same_bits():
    from icsg3d_amd.tsne import tsne
    x = R.clustered_codes(5, 700, 64)[0]
    a = tsne(x, max_iter=300)
    b = tsne(x, max_iter=300)
    assert np.array_equal(_bits(a.embedding_), _bits(b.embedding_))
    assert np.float64(a.kl_divergence_).tobytes() == np.float64(b.kl_divergence_).tobytes() and a.n_iter_ == b.n_iter_ == 299


# ---------------------------------------------------------------- 7. the device-resident path
def _vae(C, d, mb, seed=3):
    from icsg3d_amd.synthetic import random_engines
    return random_engines(d, C, mb, seed, unet=False)[0]


def test_device_resident_codes_and_latent_map_bit_for_bit():
    from icsg3d_amd import _lib as L
    from icsg3d_amd.synthetic import synthetic_batch
    from icsg3d_amd.tsne import Tsne, latent_map, tsne
    C, d, mb, nb = 1, 16, 32, 8
    ve = _vae(C, d, mb)
    batches = []
    for b in range(nb):
        X, _, cond = synthetic_batch(mb if b else mb - 5, d, C, seed=50 + b, noise=1e-3)
        batches.append((X.astype(np.float32), cond[:, :10].astype(np.float32)))
    n = sum(len(x) for x, _ in batches)
    t = Tsne(256, n)
    host = []
    for x, cond in batches:
        host.append(ve.encode(x, cond, np.zeros((len(x), 256), np.float32))[0])
        t.append_vae(ve, len(x))
    host = np.concatenate(host)
    assert np.array_equal(_bits(t.codes()), _bits(host)), "appended codes differ from encode(...)[0]"
    t.close()
    assert np.unique(host, axis=0).shape[0] > n // 2
    a = latent_map(ve, batches, capacity=n, perplexity=20.0, max_iter=300)
    b = tsne(host, perplexity=20.0, max_iter=300)
    assert a.embedding_.shape == (n, 2) and np.isfinite(a.embedding_).all()
    assert np.array_equal(_bits(a.embedding_), _bits(b.embedding_))
    assert np.float64(a.kl_divergence_).tobytes() == np.float64(b.kl_divergence_).tobytes() and a.n_iter_ == b.n_iter_
    dirty = L.C.c_int(-1)
    L.check(L.load().ics_net_check_canaries(ve._h, L.C.byref(dirty)))
    assert dirty.value == 0


# ---------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_outputs_untouched():
    from icsg3d_amd import _lib as L
    from icsg3d_amd.tsne import Tsne
    lib = L.load()
    C = L.C
    x = R.clustered_codes(1, 40, 8)[0]
    idx = np.full((40, 5), -7, np.int32); d2 = np.full((40, 5), -7.0); cp = np.full((40, 5), -7.0)

    def refused(rc, msg):
        err = lib.ics_last_error().decode()
        assert rc != 0 and msg in err, (rc, msg, err)

    bad = x.copy(); bad[3, 2] = np.nan
    refused(lib.ics_op_tsne_knn(L.fptr(bad), 40, 8, 5, L.i32ptr(idx), L.f64ptr(d2)), "not finite")
    refused(lib.ics_op_tsne_knn(L.fptr(x), 1, 8, 1, L.i32ptr(idx), L.f64ptr(d2)), "n must be")
    refused(lib.ics_op_tsne_knn(L.fptr(x), 40, 8, 40, L.i32ptr(idx), L.f64ptr(d2)), "k must be")
    refused(lib.ics_op_tsne_knn(L.fptr(x), 40, 4097, 5, L.i32ptr(idx), L.f64ptr(d2)), "dim must be")
    dd = np.abs(R.clustered_codes(2, 40, 5)[0]).astype(np.float64)
    refused(lib.ics_op_tsne_affinities(L.f64ptr(dd), 40, 5, 0.0, L.f64ptr(cp)), "perplexity")
    dd[0, 0] = np.inf
    refused(lib.ics_op_tsne_affinities(L.f64ptr(dd), 40, 5, 3.0, L.f64ptr(cp)), "finite")
    assert (idx == -7).all() and (d2 == -7).all() and (cp == -7).all()

    h = L._H(None)
    cfg = L.TsneConfig(8, 40, 3, 5.0, 12.0, 250, 1000, 50, 300, 1e-7, -1.0)
    refused(lib.ics_op_tsne_create(C.byref(cfg), C.byref(h)), "n_components")
    assert not h.value
    with pytest.raises(L.IcsError, match="n_components"):
        Tsne(8, 40, n_components=3)

    init = np.zeros((40, 2), np.float32)
    t = Tsne(8, 40, perplexity=5.0)
    t.append(x[:1])
    with pytest.raises(L.IcsError, match="at least 2 codes"):
        t.prepare(init[:1])
    t.append(x[1:5])
    with pytest.raises(L.IcsError, match="perplexity must be less than n_samples"):
        t.prepare(init[:5])
    with pytest.raises(L.IcsError, match="not finite"):
        t.append(bad[3:4])
    t.append(x[5:])
    for wrong in (init[:39], np.zeros((40, 3), np.float32), np.zeros((2, 40), np.float32)):
        with pytest.raises(L.IcsError, match="init must be"):
            t.prepare(wrong)
    with pytest.raises(L.IcsError, match="no graph yet"):
        t.run(1)
    emb = np.full((40, 2), -7, np.float32)
    refused(lib.ics_op_tsne_read(t._h, L.fptr(emb), None, None, None, None), "no embedding yet")
    assert (emb == -7).all()
    t.prepare(init + np.float32(1e-4) * x[:, :2])                  # still usable
    assert t.run(10) is False and np.isfinite(t.read()["embedding"]).all()
    t.close()

    # non-finite codes that arrived device to device are refused by prepare (a grid with a NaN voxel encodes to NaN)
    from icsg3d_amd.synthetic import synthetic_batch
    ve = _vae(1, 16, 4)
    X, _, cond = synthetic_batch(4, 16, 1, seed=1)
    X = X.astype(np.float32); X[2, 3, 4, 5, 0] = np.nan
    zm = ve.encode(X, cond[:, :10], np.zeros((4, 256), np.float32))[0]
    assert not np.isfinite(zm[2]).all()
    t = Tsne(256, 4, perplexity=1.0)
    t.append_vae(ve, 4)
    with pytest.raises(L.IcsError, match="codes are not finite"):
        t.prepare(np.zeros((4, 2), np.float32))
    t.close()


# ---------------------------------------------------------------- 9. the script
def test_script_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "latent_map.py"), "--name", "t", "--synthetic", "--samples", "200",
                        "--batch_size", "20", "--d", "16", "--channels", "1", "--perplexity", "10", "--max_iter", "300"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = tmp_path / "output" / "latent"
    g = np.load(out / "t_tsne.npz")
    assert g["embedding"].shape == (200, 2) and g["embedding"].dtype == np.float32 and np.isfinite(g["embedding"]).all()
    assert g["ids"].shape == (200,) and g["cond_bin"].shape == (200,) and g["target"].shape == (200,)
    assert (g["cond_bin"] >= 0).all() and (g["cond_bin"] < 10).all()
    assert np.isfinite(g["kl_divergence"]) and int(g["n_iter"]) == 299
    run = json.load(open(out / "run.json"))
    assert run["n"] == 200 and run["perplexity"] == 10 and set(run["seconds"]) == {"knn", "affinities", "symmetrise"}
    try:
        import matplotlib  # noqa: F401
        assert run["figure"] and (out / "t_tsne.svg").stat().st_size > 1000
    except ImportError:
        assert not run["figure"]
