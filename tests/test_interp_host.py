"""interpolate() without a GPU: the numpy path of icsg3d_amd.interpolate (a `vae` with encoder.predict / decoder.predict
and no engine) held bit for bit to the reference's own function run by tests/golden/make_interp_golden.py; the script's
flags held to the reference's add_argument calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interp_golden.npz")
GRID = (2, 2, 2, 1)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _decoder_output(z):
    """make_interp_golden.py's stand-in decoder"""
    z = np.asarray(z, np.float32)
    base = np.arange(int(np.prod(GRID)), dtype=np.float32).reshape(GRID)
    return np.stack([base + np.float32(k) + np.tanh(r[0]) for k, r in enumerate(z)]).astype(np.float32)


class StandInVae:
    def __init__(self, z_a, z_b):
        self.batch_size = 20
        self.decoder_inputs = []
        codes = [z_a, z_b]
        outer = self

        class Enc:
            def predict(self, inputs, **_):
                z = codes.pop(0)
                return np.zeros_like(z), np.zeros_like(z), z

        class Dec:
            def predict(self, inputs, **_):
                z, cond = inputs
                outer.decoder_inputs.append((np.asarray(z, np.float32), np.asarray(cond, np.float32)))
                return _decoder_output(z)
        self.encoder, self.decoder = Enc(), Dec()


def _cases():
    g = np.load(GOLDEN)
    return g, range(len(g["num_interps"]))


def test_golden_holds_the_cases():
    g, ks = _cases()
    got = {(int(g["za_%d" % k].shape[1]), int(g["num_interps"][k]), float(g["max_alpha"][k])) for k in ks}
    for latent in (256, 7):
        for n, m in [(8, 1.0), (5, 0.5), (2, 1.0), (1, 1.0), (8, 1.5)]:
            assert (latent, n, m) in got
    assert np.array_equal(g["alpha_%d" % [k for k in ks if g["num_interps"][k] == 1][0]], [0.0])
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_numpy_path_reproduces_the_reference_bit_for_bit():
    from icsg3d_amd.interpolate import interpolate, lerp_path
    g, ks = _cases()
    for k in ks:
        n, m = int(g["num_interps"][k]), float(g["max_alpha"][k])
        z_a, z_b = g["za_%d" % k], g["zb_%d" % k]
        vae = StandInVae(z_a, z_b)
        out, zs = interpolate(g["a_%d" % k], g["b_%d" % k], g["cond_%d" % k], vae, n, True, m)
        assert vae.batch_size == n == int(g["batch_size_after"][k])            # the reference's side effect
        (dec_z, dec_cond), = vae.decoder_inputs                                 # one decoder call for the whole line
        ref_z = g["dec_z_%d" % k]
        assert dec_z.dtype == np.float32 and dec_z.shape == ref_z.shape == (n, z_a.shape[1])
        assert np.array_equal(_bits(dec_z), _bits(ref_z)), k
        assert np.array_equal(_bits(dec_cond), _bits(g["dec_cond_%d" % k])), k
        ref_out = g["out_%d" % k]
        assert out.dtype == np.float32 and out.shape == ref_out.shape == (n + 2,) + GRID
        assert np.array_equal(_bits(out), _bits(ref_out)), k                     # [a, M_interps, b]
        assert np.array_equal(out[0], g["a_%d" % k][0]) and np.array_equal(out[-1], g["b_%d" % k][0])
        # zs: [z_a, the codes the decoder received, z_b] -- float32; the reference's is the float64 line before the cast
        assert zs.dtype == np.float32 and tuple(zs.shape) == tuple(g["zs_shape_%d" % k])
        assert np.array_equal(_bits(zs[0]), _bits(z_a[0])) and np.array_equal(_bits(zs[-1]), _bits(z_b[0]))
        assert np.array_equal(_bits(zs[1:-1]), _bits(ref_z))
        if "zs_%d" % k in g.files:
            with np.errstate(all="ignore"):
                assert np.array_equal(_bits(zs), _bits(g["zs_%d" % k].astype(np.float32)))
        assert np.array_equal(_bits(lerp_path(z_a, z_b, g["alpha_%d" % k])[0]), _bits(ref_z))
        # without return_zs: the array alone
        only = interpolate(g["a_%d" % k], g["b_%d" % k], g["cond_%d" % k], StandInVae(z_a, z_b), n, max_alpha=m)
        assert isinstance(only, np.ndarray) and np.array_equal(_bits(only), _bits(ref_out))


def test_the_line_is_not_a_float32_lerp():
    """the reason the arithmetic is pinned: evaluating the line in float32 gives other bits on the golden codes"""
    g, _ = _cases()
    z_a, z_b, alpha = g["za_0"], g["zb_0"], g["alpha_0"]
    with np.errstate(all="ignore"):
        f32 = z_a + alpha.astype(np.float32)[:, None] * (z_b - z_a)
    assert f32.dtype == np.float32 and not np.array_equal(_bits(f32), _bits(g["dec_z_0"]))


def test_pairs_and_slerp_on_the_numpy_path():
    from icsg3d_amd.interpolate import interpolate, interpolate_pairs, latent_path_numpy, slerp_path
    rng = np.random.default_rng(3)
    P, lat, n = 3, 7, 4
    za, zb = rng.standard_normal((P, lat)).astype(np.float32), rng.standard_normal((P, lat)).astype(np.float32)
    A = rng.uniform(0, 1, (P,) + GRID).astype(np.float32)
    B = rng.uniform(0, 1, (P,) + GRID).astype(np.float32)
    conds = np.eye(10, dtype=np.float32)[:P]

    class Many(StandInVae):
        def __init__(self):
            StandInVae.__init__(self, None, None)
            seq = [z[None] for pair in zip(za, zb) for z in pair]
            self.encoder.predict = lambda inputs, **_: (None, None, seq.pop(0))
    for mode in ("lerp", "slerp"):
        rows, zs = interpolate_pairs(A, B, conds, Many(), n, True, 1.5, mode=mode)
        assert rows.shape == (P, n + 2) + GRID and zs.shape == (P, n + 2, lat)
        for p in range(P):
            r1, z1 = interpolate(A[p:p + 1], B[p:p + 1], conds[p:p + 1], StandInVae(za[p:p + 1], zb[p:p + 1]), n, True, 1.5,
                                 mode=mode)
            assert np.array_equal(_bits(rows[p]), _bits(r1)) and np.array_equal(_bits(zs[p]), _bits(z1))
    # slerp: the endpoints at t = 0 / 1, constant norm between codes of equal norm, the lerp for (anti)parallel pairs
    alpha = np.linspace(0, 1, 5)
    a = za[:1] / np.linalg.norm(za[0]); b = zb[:1] / np.linalg.norm(zb[0])
    s = slerp_path(a.astype(np.float32), b.astype(np.float32), alpha)[0]
    assert np.allclose(s[0], a[0], atol=1e-6) and np.allclose(s[-1], b[0], atol=1e-6)
    assert np.allclose(np.linalg.norm(s, axis=1), 1.0, atol=1e-6)
    for other in (za[:1], -za[:1], 2 * za[:1], np.zeros_like(za[:1])):
        assert np.array_equal(_bits(slerp_path(za[:1], other, alpha)), _bits(latent_path_numpy(za[:1], other, alpha, "lerp")))
    with pytest.raises(ValueError):
        interpolate_pairs(A, B, conds, Many(), n, mode="cubic")


def test_script_lists_the_reference_flags_with_their_defaults():
    g, _ = _cases()
    names, types, defaults = list(g["flag_names"]), list(g["flag_types"]), list(g["flag_defaults"])
    assert names == ["--name", "--ninterps", "--projection", "--enda", "--endb", "--ncond"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "interpolate.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for n in names + ["--synthetic", "--channels", "--d", "--seed", "--mode", "--atoms", "--batch_size"]:
        assert n in r.stdout, n
    sys.path.insert(0, ROOT)
    import importlib.util
    spec = importlib.util.spec_from_file_location("interpolate_script", os.path.join(ROOT, "interpolate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    ns = parser.parse_args([])
    acts = {a.option_strings[0]: a for a in parser._actions if a.option_strings}
    for n, t, dflt in zip(names, types, defaults):
        assert repr(getattr(ns, n[2:])) == dflt, (n, getattr(ns, n[2:]), dflt)
        assert acts[n].type.__name__ == t, n


def test_latent_path_refuses_null_codes_before_any_device_call():
    from icsg3d_amd import _lib as L
    lib = L.load()
    za, zb, alpha = np.zeros((1, 4), np.float32), np.ones((1, 4), np.float32), np.linspace(0.0, 1.0, 3)
    path = np.zeros((1, 3, 4), np.float32)
    for a, b, p in ((None, zb, path), (za, None, path), (za, zb, None)):
        rc = lib.ics_op_latent_path(L.fptr(a), L.fptr(b), 1, 4, L.f64ptr(alpha), 3, 0, L.fptr(p))
        msg = (lib.ics_last_error() or b"").decode()
        assert rc != 0 and msg.startswith("ics_op_latent_path: null argument (za, zb, path are required) ("), msg
