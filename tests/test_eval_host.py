"""eval.py's host side, held to the reference's own code (tests/golden/eval_golden.npz, tests/golden/make_eval_golden.py):
the voxel-to-Angstrom shift of predicted atoms and the lattice / voxel parameters behind it, and eval.py's flags.  The
EMD itself is a device op (ics_op_match_emd): tests/test_gpu_eval.py holds it to the same fixture."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_golden.npz")


def _minmax(p):
    return np.stack([p.min(axis=(0, 1, 2)), p.max(axis=(0, 1, 2))], axis=-1)[None]      # (1, 3, 2)


def test_lattice_and_voxel_parameters_equal_the_reference():
    from icsg3d_amd.utils import to_lattice_params, to_lattice_params_from_minmax, to_voxel_params
    g = np.load(GOLDEN)
    for k, d in enumerate(g["grid_d"]):
        p = g["grid_%d" % k]
        d = int(d)
        lp = to_lattice_params(p[None], d=d)
        np.testing.assert_allclose(lp[0], g["lp"][k], rtol=1e-14, atol=0)
        np.testing.assert_allclose(to_lattice_params_from_minmax(_minmax(p), d=d)[0], g["lp"][k], rtol=1e-14, atol=0)
        np.testing.assert_allclose(to_voxel_params(lp, d=d)[0], g["dv"][k], rtol=1e-14, atol=0)


def test_predicted_coordinates_equal_the_reference_shift():
    from icsg3d_amd.evaluate import predicted_coordinates
    g = np.load(GOLDEN)
    for k, d in enumerate(g["grid_d"]):
        mu = g["mu_%d" % k]
        atoms = [(list(range(len(mu))), [tuple(r) for r in mu])]
        got = predicted_coordinates(atoms, _minmax(g["grid_%d" % k]), eps_frac=float(g["shift_eps"][k]), d=int(d))
        assert len(got) == 1 and got[0].shape == mu.shape
        np.testing.assert_allclose(got[0], g["shifted_%d" % k], rtol=1e-13, atol=1e-13)


def test_predicted_coordinates_of_an_empty_sample():
    from icsg3d_amd.evaluate import predicted_coordinates
    mm = np.array([[[0.0, 5.0], [0.0, 6.0], [0.0, 7.0]]] * 2)
    got = predicted_coordinates([([], []), ([3], [(1.0, 2.0, 3.0)])], mm, d=16)
    assert got[0].shape == (0, 3) and got[1].shape == (1, 3)


def test_eval_flags_are_the_references():
    sys.path.insert(0, ROOT)
    import eval as E
    g = np.load(GOLDEN)
    acts = {a.option_strings[0]: a for a in E.build_parser()._actions if a.option_strings}
    for name, typ, default in zip(g["flag_names"], g["flag_types"], g["flag_defaults"]):
        assert name in acts, name
        a = acts[name]
        assert (a.type.__name__ if a.type else "") == typ, (name, a.type)
        assert repr(a.default) == default, (name, a.default, default)
    a = E.build_parser().parse_args([])
    assert (a.channels, a.from_sites, a.sigma_frac, a.label_frac) == (4, False, 1.0, 1.0)


def test_data_split_names_equals_data_split(tmp_path):
    from icsg3d_amd.utils import data_split, data_split_names
    names = ["mp-%d.npy" % i for i in range(13)]
    os.makedirs(tmp_path / "density_matrices")
    for n in names:
        open(tmp_path / "density_matrices" / n, "w").close()
    assert data_split(str(tmp_path), 11, frac=0.8, n_rot=0) == data_split_names(sorted(names), 11, frac=0.8, n_rot=0)
