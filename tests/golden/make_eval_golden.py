"""Generates tests/golden/eval_golden.npz in THIS container by running the REFERENCE's own scoring code:
`emd` (/root/reference/eval.py:45-53, cdist + scipy's linear_sum_assignment), `to_lattice_params` / `to_voxel_params`
(/root/reference/utils.py:160-190) and the two statements of eval.py:207-209 that shift atom centroids from voxels to
Angstrom.  Neither module can be imported (matplotlib / pymatgen / skimage at their tops), so the FunctionDefs and
statements are pulled out of the files with `ast`, compiled and executed with numpy / scipy in scope, as
make_data_split_golden.py does -- it is the reference's code that runs, nothing of its text is written to the repo.
eval.py's argparse flags (names, types, defaults) are read from its add_argument calls the same way.

Contents (all float64):
  emd cases        a_xyz / a_off, b_xyz / b_off (CSR), emd (B,), case_name (B,): square and rectangular sets in both
                   orientations from 1 x 1 up to 256 x 2048, identical sets (EMD 0), exact ties (lattice points,
                   duplicated points), an empty predicted set (NaN)
  lattice cases    grid_<k> (d, d, d, 3) coordinate grids (float64, as create_matrices.py stores them; d = 8 / 16),
                   grid_d, grid_eps, lp (K, 3) = to_lattice_params, dv (K, 3) = to_voxel_params,
                   mu_<k> centroids in voxels, shifted_<k> = the eval.py:207-209 shift with --eps_frac shift_eps[k]
  flags            flag_names, flag_types, flag_defaults (str)

    python tests/golden/make_eval_golden.py
"""
import ast
import os

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))
REF_EVAL = "/root/reference/eval.py"
REF_UTILS = "/root/reference/utils.py"


def _functions(path, names, ns):
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(fns) == len(names), names
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def reference_shift():
    """The statements `lpp = ...` and `mu = ... - lpp + ...` of eval.py's scoring loop, as one callable."""
    tree = ast.parse(open(REF_EVAL).read())
    stmts = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            t, src = node.targets[0].id, ast.unparse(node.value)
            if t == "lpp" or (t == "mu" and "dv_pred" in src):
                stmts.append(node)
    stmts.sort(key=lambda n: n.lineno)
    assert [s.targets[0].id for s in stmts] == ["lpp", "mu"], [ast.unparse(s) for s in stmts]
    code = compile(ast.Module(body=stmts, type_ignores=[]), REF_EVAL, "exec")

    def shift(mu, l_pred, dv_pred, i, eps):
        ns = {"np": np, "mu": mu, "l_pred": l_pred, "dv_pred": dv_pred, "i": i, "eps": eps}
        exec(code, ns)
        return ns["mu"]
    return shift


def reference_flags():
    tree = ast.parse(open(REF_EVAL).read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", None) == "add_argument":
            name = node.args[0].value
            kw = {k.arg: k.value for k in node.keywords}
            typ = kw["type"].id if "type" in kw else ""
            default = repr(ast.literal_eval(kw["default"])) if "default" in kw else "None"
            out.append((node.lineno, name, typ, default))
    out.sort()
    return [o[1:] for o in out]


def _cases(rng):
    cases = []
    for n, m in [(1, 1), (1, 6), (6, 1), (2, 3), (7, 7), (40, 37), (37, 40), (40, 40), (64, 65), (129, 100),
                 (100, 129), (256, 300), (256, 2048), (2048, 256)]:
        cases.append(("random_%dx%d" % (n, m), rng.uniform(0, 10, (n, 3)), rng.uniform(0, 10, (m, 3))))
    x = rng.uniform(0, 8, (30, 3))
    cases.append(("identical_permuted", x, x[rng.permutation(30)]))
    y = rng.uniform(0, 8, (256, 3))
    cases.append(("identical_256", y, y.copy()))
    g = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cases.append(("lattice_vs_shifted", g, g + 0.5))                       # many equal distances
    cases.append(("lattice_vs_sub", g, g[::2] * 1.0))
    cases.append(("lattice_vs_sub_rev", g[1::3] + 0.25, g))
    cases.append(("duplicates", np.repeat(g[:5], 3, axis=0), g[:9]))       # duplicated points
    cases.append(("duplicates_both", np.repeat(g[:4], 2, axis=0), np.repeat(g[2:6], 2, axis=0)))
    cases.append(("empty_pred", np.zeros((0, 3)), rng.uniform(0, 5, (7, 3))))
    return cases


def main():
    ns = {"np": np, "cdist": cdist, "linear_sum_assignment": linear_sum_assignment}
    (emd,) = _functions(REF_EVAL, ["emd"], ns)
    to_lattice_params, to_voxel_params = _functions(REF_UTILS, ["to_lattice_params", "to_voxel_params"], {"np": np})
    shift = reference_shift()
    rng = np.random.default_rng(2026)
    cases = _cases(rng)
    with np.errstate(invalid="ignore"):
        e = np.array([emd(a, b) for _, a, b in cases], np.float64)
    out = {"case_name": np.array([c[0] for c in cases]), "emd": e}
    for k, key in ((1, "a"), (2, "b")):
        sets = [c[k] for c in cases]
        off = np.zeros(len(sets) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in sets])
        out[key + "_xyz"] = np.concatenate(sets).astype(np.float64)
        out[key + "_off"] = off

    # coordinate grids -> lattice / voxel parameters -> shifted centroids
    lps, dvs, gd, ge, se = [], [], [], [], []
    for k, (d, eps_grid, eps_shift) in enumerate([(8, 0.25, 0.25), (16, 0.25, 0.25), (16, 0.1, 0.25), (8, 0.25, 0.1)]):
        abc = rng.uniform(3, 9, 3)
        ax = [np.linspace(0, a + 2 * eps_grid * a, d + 1)[:-1] for a in abc]     # coordinate_grid's layout
        p = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
        lp = to_lattice_params(p[None], d=d)
        dv = to_voxel_params(lp, d=d)
        mu = rng.uniform(0, d - 1, (5 + k, 3))
        out["grid_%d" % k] = p
        out["mu_%d" % k] = mu
        out["shifted_%d" % k] = shift(mu.copy(), lp, dv, 0, eps_shift)
        lps.append(lp[0]); dvs.append(dv[0]); gd.append(d); ge.append(eps_grid); se.append(eps_shift)
    out.update(lp=np.array(lps), dv=np.array(dvs), grid_d=np.array(gd), grid_eps=np.array(ge), shift_eps=np.array(se))

    flags = reference_flags()
    out.update(flag_names=np.array([f[0] for f in flags]), flag_types=np.array([f[1] for f in flags]),
               flag_defaults=np.array([f[2] for f in flags]))
    path = os.path.join(HERE, "eval_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "emd cases;", [f[0] for f in flags])


if __name__ == "__main__":
    main()
