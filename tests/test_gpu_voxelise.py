"""ics_op_voxelise and the engine feeds on the MI355X: held to the reference's own voxeliser (tests/golden/voxel_golden.npz)
and to the fp64 restatement of tests/test_voxelise_host.py (which is held to the same fixture on the CPU); invalid
arguments; the engine feeds bit-identical to upload_batch of the loaders' arrays; create_matrices.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_voxelise_host as H  # noqa: E402


def _structs(rng, count, max_ns, ncls=95, nan_pad=True, sigma_scale=(0.5, 2.0)):
    from icsg3d_amd.matrices import Structures
    ns = rng.integers(1, max_ns + 1, count)
    ns[0] = max_ns
    xyz = np.full((count, max_ns, 3), np.nan if nan_pad else 0.0)
    z = np.full((count, max_ns), np.nan if nan_pad else 0.0)
    sg = np.full((count, max_ns), np.nan if nan_pad else 0.0)
    abc = rng.uniform(3.0, 9.0, (count, 3))
    for i in range(count):
        f = rng.uniform(0, 1, (ns[i], 3))
        xyz[i, :ns[i]] = (f - f.min(0)) * abc[i]
        z[i, :ns[i]] = rng.integers(1, ncls, ns[i])
        sg[i, :ns[i]] = rng.uniform(*sigma_scale, ns[i])
    return Structures(ns, xyz, z, sg, abc)


def test_op_equals_the_reference_voxeliser(relerr):
    from icsg3d_amd.matrices import Structures, voxelise
    g = np.load(H.GOLDEN)
    for i in range(len(g["d"])):
        n, d = int(g["nsites"][i]), int(g["d"][i])
        s = Structures([n], g["xyz"][i:i + 1, :n], g["z"][i:i + 1, :n], g["sigma"][i:i + 1, :n], g["abc"][i:i + 1])
        rots = [(-1, -1, -1)] + [tuple(a) for c, a in zip(g["rot_case"], g["rot_axes"]) if c == i]
        ks = [k for k, c in enumerate(g["rot_case"]) if c == i]
        jobs = np.array([(0, *r) for r in rots], np.int32)
        M, S, p = voxelise(s, jobs=jobs, d=d, eps_frac=float(g["eps_frac"][i]), label_frac=float(g["label_frac"][i]))
        Mg, idx, Sg, pg = H.golden_case(g, i)
        ref = [(Mg, Sg, pg)] + [(g["rot_M_%d" % k], g["rot_S_%d" % k], g["rot_p_%d" % k]) for k in ks]
        for j, (Mr, Sr, pr) in enumerate(ref):
            assert np.array_equal(S[j], Sr), (i, j, int((S[j] != Sr).sum()))
            assert relerr(M[j][idx] if j == 0 else M[j], Mr) <= 1e-13, (i, j)
            if j == 0:
                assert np.array_equal(p[j], pr), i
            else:
                assert np.abs(p[j] - pr).max() <= 1e-13 * np.abs(pr).max(), (i, j)


def test_functions_with_the_reference_signatures(relerr):
    from icsg3d_amd.matrices import coordinate_grid, density_matrix
    g = np.load(H.GOLDEN)
    i = 5                                                            # d = 32, label_frac 0.6
    n, d = int(g["nsites"][i]), int(g["d"][i])
    Mg, idx, Sg, pg = H.golden_case(g, i)
    M, S = density_matrix(g["xyz"][i, :n], g["z"][i, :n], l=list(g["abc"][i]), sigma=g["sigma"][i, :n], dims=(d, d, d),
                          label_frac=float(g["label_frac"][i]), eps_frac=float(g["eps_frac"][i]))
    assert M.shape == S.shape == (d, d, d) and np.array_equal(S, Sg) and relerr(M[idx], Mg) <= 1e-13
    lat = np.r_[g["abc"][i], 90.0, 90.0, 90.0]
    assert np.array_equal(coordinate_grid(lat, dim=d, eps_frac=float(g["eps_frac"][i])), pg)


@pytest.mark.parametrize("d,count,max_ns", [(16, 6, 40), (32, 5, 24), (64, 3, 12), (128, 2, 4)])
def test_op_random_batches_all_rotations(d, count, max_ns, relerr):
    from icsg3d_amd.matrices import voxelise
    rng = np.random.default_rng(d)
    s = _structs(rng, count, max_ns)
    triples = [(a, b, c) for a in range(3) for b in range(3) for c in range(3)]
    if d >= 64:    # keep the host restatement small at the large grids: a sample of the triples, and partial ones
        triples = [triples[k] for k in rng.choice(27, 4, replace=False)] + [(-1, 2, -1), (1, -1, 0)]
    jobs = [(st, -1, -1, -1) for st in range(count)] + [(int(rng.integers(count)), *t) for t in triples]
    jobs = np.array(jobs, np.int32)
    M, S, p = voxelise(s, jobs=jobs, d=d, eps_frac=0.25 if d != 32 else 0.1, label_frac=1.0 if d != 32 else 0.6)
    lf, ef = (1.0, 0.25) if d != 32 else (0.6, 0.1)
    base = [H.restate_grids(s.xyz[st, :s.nsites[st]], s.z[st, :s.nsites[st]], s.sigma[st, :s.nsites[st]], s.abc[st], d,
                            ef, lf) for st in range(count)]
    for j, (st, *rot) in enumerate(jobs):
        Mr, Sr, pr = (H.rotate(a, rot) for a in base[st])
        assert np.array_equal(S[j], Sr), (j, rot, int((S[j] != Sr).sum()))
        assert relerr(M[j], Mr) <= 1e-13, (j, rot)
        assert np.array_equal(p[j], pr), (j, rot)


def test_op_chunks_large_job_counts():
    from icsg3d_amd.matrices import voxelise
    rng = np.random.default_rng(5)
    s = _structs(rng, 7, 9)
    jobs = np.array([(k % 7, k % 4 - 1, (k // 4) % 4 - 1, (k // 16) % 4 - 1) for k in range(1300)], np.int32)
    _, S, _ = voxelise(s, jobs=jobs, d=16, want=("S",))              # 1300 jobs: more than one chunk
    M, _, p = voxelise(s, jobs=jobs[:5], d=128, want=("M", "p"))   # 67 MB per job: several chunks
    base = [H.restate_grids(s.xyz[st, :s.nsites[st]], s.z[st, :s.nsites[st]], s.sigma[st, :s.nsites[st]], s.abc[st], 16,
                            0.25, 1.0)[1] for st in range(7)]
    for j, (st, *rot) in enumerate(jobs):
        assert np.array_equal(S[j], H.rotate(base[st], rot)), j
    M1, _, p1 = voxelise(s, jobs=jobs[4:5], d=128, want=("M", "p"))
    assert np.array_equal(M[4], M1[0]) and np.array_equal(p[4], p1[0])


def test_invalid_arguments_are_refused_and_the_library_stays_usable():
    from icsg3d_amd import _lib as L
    from icsg3d_amd.matrices import Structures, voxelise
    from icsg3d_amd.engine import UnetEngine
    rng = np.random.default_rng(9)
    s = _structs(rng, 3, 5)
    ok = np.array([(0, -1, -1, -1), (1, 0, 1, 2)], np.int32)

    def bad(msg, **kw):
        args = dict(jobs=ok, d=16)
        args.update(kw)
        st = args.pop("structs", s)
        with pytest.raises(L.IcsError, match=msg):
            voxelise(st, **args)

    bad("structure index", jobs=np.array([(3, -1, -1, -1)], np.int32))
    bad("rotation index", jobs=np.array([(0, 3, -1, -1)], np.int32))
    bad("grid edge", d=1)
    bad("grid edge", d=512)
    bad("eps_frac", eps_frac=-1.0)
    bad("label_frac", label_frac=float("nan"))
    def edit(fn):                                                    # structure 1, site 0: what job 1 reads
        t = Structures(s.nsites.copy(), s.xyz.copy(), s.z.copy(), s.sigma.copy(), s.abc.copy())
        fn(t)
        return t

    for fn, msg in ((lambda t: t.nsites.__setitem__(1, 0), "nsites"), (lambda t: t.nsites.__setitem__(1, 6), "nsites"),
                    (lambda t: t.sigma.__setitem__((1, 0), 0.0), "sigma"),
                    (lambda t: t.sigma.__setitem__((1, 0), np.inf), "sigma"),
                    (lambda t: t.abc.__setitem__((1, 1), -2.0), "lattice"),
                    (lambda t: t.xyz.__setitem__((1, 0, 2), np.nan), "coordinates"),
                    (lambda t: t.z.__setitem__((1, 0), -1.0), "Z")):
        bad(msg, structs=edit(fn))
    big = _structs(rng, 1, 257, nan_pad=False)
    bad("nsites", structs=big, jobs=np.array([(0, -1, -1, -1)], np.int32))
    M, S, p = voxelise(s, jobs=ok, d=16)                            # the library is still usable
    assert np.isfinite(M).all() and np.isfinite(p).all()

    ue = UnetEngine(in_channels=4, d=16, max_batch=2)
    cls = Structures(s.nsites.copy(), s.xyz.copy(), s.z.copy(), s.sigma.copy(), s.abc.copy())
    cls.z[1, 0] = 95.0
    with pytest.raises(L.IcsError, match="class id"):
        ue.voxelise_batch(cls, ok)
    cls.z[1, 0] = 2.5
    with pytest.raises(L.IcsError, match="class id"):
        ue.voxelise_batch(cls, ok)
    with pytest.raises(L.IcsError, match="max_batch"):
        ue.voxelise_batch(s, np.array([(0, -1, -1, -1)] * 3, np.int32))
    ue3 = UnetEngine(in_channels=3, d=16, max_batch=2)
    with pytest.raises(L.IcsError, match="input channels"):
        ue3.voxelise_batch(s, ok)
    ue.voxelise_batch(s, ok)                                        # still usable
    assert np.isfinite(ue.train_step_resident(want_metrics=True)).all()


def _loader_arrays(s, jobs, d, C, ef, lf):
    """What UnetDataGenerator / VAEDataGenerator build from the files create_matrices.py would write for these jobs."""
    from icsg3d_amd.matrices import voxelise
    M, S, p = voxelise(s, jobs=jobs, d=d, eps_frac=ef, label_frac=lf)
    X = np.empty((len(jobs), d, d, d, C), np.float32)
    y = np.empty((len(jobs), d, d, d), np.uint8)
    for i in range(len(jobs)):
        X[i] = M[i].reshape(d, d, d, 1) if C == 1 else np.concatenate((M[i].reshape(d, d, d, 1), p[i]), axis=-1)
        y[i] = S[i]
    return X, y


def _same_weights(a, b):
    wa, wb = a.get_weights(), b.get_weights()
    return sorted(wa) == sorted(wb) and all(np.array_equal(wa[k], wb[k]) for k in wa)


@pytest.mark.parametrize("C", [1, 4])
def test_unet_feed_is_bit_identical_to_upload(C):
    from icsg3d_amd.engine import UnetEngine
    d, B, ef, lf = 16, 3, 0.25, 0.8
    rng = np.random.default_rng(C)
    s = _structs(rng, 4, 10, sigma_scale=(1.0, 3.0))
    jobs = np.array([(0, -1, -1, -1), (2, 0, 2, 1), (3, 1, 1, -1)], np.int32)
    X, y = _loader_arrays(s, jobs, d, C, ef, lf)
    assert (y > 0).mean() > 0.05
    a = UnetEngine(in_channels=C, d=d, max_batch=B, lr=1e-3)
    b = UnetEngine(in_channels=C, d=d, max_batch=B, lr=1e-3)
    b.set_weights(a.get_weights())
    a.voxelise_batch(s, jobs, eps_frac=ef, label_frac=lf)
    b.upload_batch(X, y)
    a.predict_resident(labels_only=True)
    b.predict_resident(labels_only=True)
    assert np.array_equal(a.get_activation("c1", (B, d, d, d, 32)), b.get_activation("c1", (B, d, d, d, 32)))
    for _ in range(2):
        ma, mb = a.train_step_resident(want_metrics=True), b.train_step_resident(want_metrics=True)
        assert np.array_equal(ma, mb) and np.isfinite(ma).all(), (ma, mb)
    assert _same_weights(a, b)
    # a second voxelised batch replaces the first (the pinned staging is reused)
    a.voxelise_batch(s, jobs[::-1].copy(), eps_frac=ef, label_frac=lf)
    b.upload_batch(X[::-1].copy(), y[::-1].copy())
    assert np.array_equal(a.train_step_resident(want_metrics=True), b.train_step_resident(want_metrics=True))
    assert _same_weights(a, b)


def test_vae_feed_is_bit_identical_to_upload():
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    d, B, C, ef, lf = 16, 2, 4, 0.25, 1.0
    rng = np.random.default_rng(11)
    s = _structs(rng, 3, 8)
    jobs = np.array([(1, 2, -1, 0), (0, -1, -1, -1)], np.int32)
    X, _ = _loader_arrays(s, jobs, d, C, ef, lf)
    cond = np.eye(10, dtype=np.float32)[[3, 7]]
    eps = rng.standard_normal((B, 256)).astype(np.float32)
    ua = UnetEngine(in_channels=C, d=d, max_batch=B)
    ub = UnetEngine(in_channels=C, d=d, max_batch=B)
    ub.set_weights(ua.get_weights())
    va = VaeEngine(ua, in_channels=C, d=d, max_batch=B)
    vb = VaeEngine(ub, in_channels=C, d=d, max_batch=B)
    vb.set_weights(va.get_weights())
    va.voxelise_batch(s, jobs, cond, eps, eps_frac=ef, label_frac=lf)
    vb.upload_batch(X, cond, eps)
    for _ in range(2):
        ma, mb = va.train_step_resident(want_metrics=True), vb.train_step_resident(want_metrics=True)
        assert np.array_equal(ma, mb) and np.isfinite(ma).all(), (ma, mb)
    assert _same_weights(va, vb)


def test_create_matrices_end_to_end(tmp_path):
    root = str(tmp_path)
    rng = np.random.default_rng(4)
    H._write_sites(root, "toy", rng, n=6)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_matrices.py"), "--name", "toy", "--root", root,
                        "--d", "16", "--nrot", "2", "--batch", "4", "--seed", "5"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from icsg3d_amd.matrices import Structures, voxelise
    sdir = os.path.join(root, "toy", "matrices")
    rs = np.random.RandomState(5)
    for i in range(6):
        sid = "mp-%d" % (100 + i)
        f = np.load(os.path.join(root, "toy", "sites", sid + ".npz"))
        s = Structures.from_sites([(f["frac_coords"], f["Z"], f["radii"], f["lattice"])])
        M, S, p = voxelise(s, d=16)
        got = [np.load(os.path.join(sdir, k, sid + ".npy")) for k in ("density_matrices", "species_matrices", "coordinate_grids")]
        assert all(np.array_equal(a, b) for a, b in zip(got, (M[0], S[0], p[0]))), sid
        for k in range(2):
            axes = rs.choice(3, 3)
            for kind, base in (("density_matrices", M[0]), ("species_matrices", S[0]), ("coordinate_grids", p[0])):
                got = np.load(os.path.join(sdir, kind, "%s_rot_%d.npy" % (sid, k)))
                assert np.array_equal(got, H.rotate(base, axes)), (sid, kind, k)
    # one AtomUnet train step over the result
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.utils import data_split
    tr, _ = data_split(sdir, n_rot=2)
    gen = UnetDataGenerator(tr, sdir, batch_size=4, dim=(16, 16, 16), n_channels=4)
    X, yb = gen[0]
    unet = AtomUnet(input_shape=(16, 16, 16, 4), max_batch=4)
    m = unet.model.train_on_batch(X, yb)
    assert np.isfinite(m).all()
