"""Generates tests/golden/interp_golden.npz by running the REFERENCE's own `interpolate` (interpolate.py:47-64).
The module cannot be imported (keras / matplotlib / pymatgen at its top), so the FunctionDef is pulled out of the file
with `ast`, compiled and executed with numpy in scope, as make_eval_golden.py does -- it is the reference's code that runs,
nothing of its text is written to the repo.  `vae` is a stand-in: encoder.predict returns fixed float32 codes (first call
z_a, second z_b), decoder.predict records its inputs after the float32 cast Keras applies to a model input and returns a
small deterministic array.  interpolate.py's argparse flags (names, types, defaults) are read from its add_argument calls.

Cases (case k): num_interps / max_alpha = 8/1, 5/0.5, 2/1, 1/1 (linspace(0, 1, 1) = [0]), 8/1.5, 5/2, 8/0.5, each at latent
256 and 7.  The codes mix magnitudes from 1e-30 to 1e4 with float32 denormals, equal elements in z_a and z_b, signed
zeros and opposite values.
Contents per case: za_k, zb_k (1, latent) float32; alpha_k float64; dec_z_k (S, latent) float32 and dec_cond_k = what the
decoder received; a_k, b_k, cond_k the inputs; out_k = the returned array; zs_k = the returned codes (float64: the
reference concatenates the float64 line) for the latent-7 cases, zs_shape_k for all -- at latent 256 the script asserts
that zs is [z_a, the float64 line whose float32 cast the decoder received, z_b] and leaves the 20 KB per case out; plus
num_interps, max_alpha, batch_size_after (the vae.batch_size side effect) and flag_names / flag_types / flag_defaults.

    python tests/golden/make_interp_golden.py <reference root>
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = (2, 2, 2, 1)


def reference_function(path, name):
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(fns) == 1, name
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def reference_flags(path):
    tree = ast.parse(open(path).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", None) == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            typ = kw["type"].id if "type" in kw else ""
            default = repr(ast.literal_eval(kw["default"])) if "default" in kw else "None"
            out.append((node.lineno, node.args[0].value, typ, default))
    out.sort()
    return [o[1:] for o in out]


def decoder_output(z):
    """the stand-in decoder: deterministic, float32, depends on the code it was given"""
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
                z32, c32 = np.asarray(z, np.float32), np.asarray(cond, np.float32)   # Keras casts to the input dtype
                outer.decoder_inputs.append((z32, c32))
                return decoder_output(z32)
        self.encoder, self.decoder = Enc(), Dec()


def codes(rng, latent):
    with np.errstate(all="ignore"):
        mag_a = 10.0 ** rng.uniform(-30, 4, latent)
        mag_b = 10.0 ** rng.uniform(-30, 4, latent)
        z_a = (rng.standard_normal(latent) * mag_a).astype(np.float32)
        z_b = (rng.standard_normal(latent) * mag_b).astype(np.float32)
    special = [(0.0, -0.0), (-0.0, 0.0), (1e-40, -3e-41), (1.5, 1.5), (-2.0, 2.0), (1e4, 1e-30), (3e-39, 1e4)]
    for j, (x, y) in enumerate(special[:latent]):
        z_a[j], z_b[j] = np.float32(x), np.float32(y)
    if latent > 16:
        z_b[10:14] = z_a[10:14]                          # equal elements: the difference is +0
        z_b[14:16] = -z_a[14:16]
    return z_a.reshape(1, latent), z_b.reshape(1, latent)


def main():
    ref = os.path.join(sys.argv[1], "interpolate.py")
    interpolate = reference_function(ref, "interpolate")
    rng = np.random.default_rng(2027)
    out = {}
    k = 0
    nums, maxs, after = [], [], []
    for latent in (256, 7):
        for num_interps, max_alpha in [(8, 1), (5, 0.5), (2, 1), (1, 1), (8, 1.5), (5, 2), (8, 0.5)]:
            z_a, z_b = codes(rng, latent)
            a = rng.uniform(0, 1, (1,) + GRID).astype(np.float32)
            b = rng.uniform(0, 1, (1,) + GRID).astype(np.float32)
            cond = np.eye(10, dtype=np.float32)[k % 10].reshape(1, 10)
            vae = StandInVae(z_a, z_b)
            with np.errstate(all="ignore"):
                M, zs = interpolate(a, b, cond, vae, num_interps=num_interps, return_zs=True, max_alpha=max_alpha)
            (dec_z, dec_cond), = vae.decoder_inputs
            assert M.shape == (num_interps + 2,) + GRID and zs.shape == (num_interps + 2, latent)
            out.update({"za_%d" % k: z_a, "zb_%d" % k: z_b, "alpha_%d" % k: np.linspace(0, max_alpha, num_interps),
                        "dec_z_%d" % k: dec_z, "dec_cond_%d" % k: dec_cond, "a_%d" % k: a, "b_%d" % k: b,
                        "cond_%d" % k: cond, "out_%d" % k: M, "zs_shape_%d" % k: np.array(zs.shape)})
            assert zs.dtype == np.float64 and np.array_equal(zs[0], z_a[0]) and np.array_equal(zs[-1], z_b[0])
            assert np.array_equal(zs[1:-1].astype(np.float32).view(np.uint32), dec_z.view(np.uint32))
            if latent <= 16:
                out["zs_%d" % k] = zs
            nums.append(num_interps); maxs.append(max_alpha); after.append(vae.batch_size)
            k += 1
    flags = reference_flags(ref)
    out.update(num_interps=np.array(nums), max_alpha=np.array(maxs, np.float64), batch_size_after=np.array(after),
               flag_names=np.array([f[0] for f in flags]), flag_types=np.array([f[1] for f in flags]),
               flag_defaults=np.array([f[2] for f in flags]))
    path = os.path.join(HERE, "interp_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", k, "cases;", flags)


if __name__ == "__main__":
    main()
