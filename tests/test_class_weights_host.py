"""Per-class loss weights, the part that needs no GPU: the case builders of tests/class_weight_cases.py checked against the
oracle, the class API's numpy loss against the oracle's with a weight vector, and the Python surface (AtomUnet's argument
check, train_unet.py's flag)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import class_weight_cases as K
from oracle import numpy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ncls", [2, 17, 95, 127])
def test_weight_vectors(ncls):
    w = K.weight_vector(ncls)
    assert w.shape == (ncls,) and w[0] == 0.0
    nz = w[w > 0]
    assert np.array_equal(nz * 64, np.round(nz * 64)) and nz.min() >= 0.25 and nz.max() <= 8.0
    assert np.array_equal(w.astype(np.float32).astype(np.float64), w)       # what the device table holds
    z = K.second_zero_class(ncls)
    assert (w == 0).sum() == (1 if z is None else 2) and (z is None) == (ncls == 2)
    assert np.unique(nz).size >= min(nz.size, 4)                            # non-uniform


@pytest.mark.parametrize("ncls,M", [(2, 1037), (17, 1037), (95, 1037), (127, 1037), (95, 16 * 2085)])
def test_head_cases_are_not_vacuous(ncls, M):
    """head_case's own assertions run when it is built; here what they leave: the reference with the vector is the sum of
    the per-class scalar references, so R.wcce_loss / R.wcce_bwd do broadcast a (C,) weight the way the kernels index it."""
    c = K.head_case(ncls, M)
    w, lab = c["w"], c["lab"]
    assert M % 4 == 1 or M // 16 > 4 * 512
    z = c["x"].astype(np.float64) @ c["ws"].astype(np.float64) + c["bs"].astype(np.float64)
    p = R.softmax(z)
    per_voxel = -w[lab] * np.log(np.clip(p[np.arange(M), lab] / p.sum(-1), R.K_EPSILON, 1 - R.K_EPSILON))
    np.testing.assert_allclose(c["lsoft"], per_voxel.mean(), rtol=1e-13)
    dz = (w[lab] / M)[:, None] * (p - R.one_hot(lab, ncls))
    np.testing.assert_allclose(c["dzs"], dz, rtol=1e-9, atol=1e-15 * np.abs(dz).max())
    assert 0 < c["zero_rows"].sum() < M
    if K.second_zero_class(ncls) is not None:
        assert (lab == K.second_zero_class(ncls)).any()


@pytest.mark.parametrize("ncls,B", [(95, 2), (95, 3), (17, 2)])
def test_network_batches_cover_the_classes(ncls, B):
    X, lab = K.unet_batch(B, 16, ncls)
    assert X.shape == (B, 16, 16, 16, 1) and lab.shape == (B, 16, 16, 16) and lab.dtype == np.uint8
    K.check_batch(lab, ncls)
    if ncls == 95:
        assert np.unique(lab).size >= 40
    _, plain, _ = R.synthetic_batch(B, 16, 1, seed=0)
    assert np.unique(plain).size <= 9                                      # what the remap is for
    assert np.array_equal(lab == 0, plain == 0)                             # the sigmoid head's targets are unchanged


def test_class_api_loss_equals_the_oracle_with_a_vector():
    """weighted_categorical_crossentropy(w) of icsg3d_amd/unet/unet.py against R.wcce_loss, w of shape (C,)."""
    from icsg3d_amd.unet.unet import weighted_categorical_crossentropy
    ncls, B, d = 17, 2, 4
    rng = np.random.default_rng(4)
    w = K.weight_vector(ncls)
    lab = rng.integers(0, ncls, size=(B, d, d, d))
    y = R.one_hot(lab, ncls)
    p = R.softmax(rng.normal(size=(B, d, d, d, ncls)) * 3)
    p[0, 0, 0, 0] = np.eye(ncls)[lab[0, 0, 0, 0]]                           # the clip at both ends
    p[0, 0, 0, 1] = np.eye(ncls)[(lab[0, 0, 0, 1] + 1) % ncls]
    got, ref = weighted_categorical_crossentropy(w)(y, p), R.wcce_loss(y, p, w)
    assert got.shape == (B,) and ref.min() > 0
    np.testing.assert_allclose(got, ref, rtol=1e-13)
    scalar = R.wcce_loss(y, p, float(ncls))
    assert np.all(np.abs(scalar - ref) > 0.1 * ref)


def test_oracle_step_with_a_vector_is_not_the_scalar_step():
    """UnetOracle(loss_weight=w): lsoft moves away from the scalar run and the background carries no softmax loss."""
    ncls, B, d = 17, 2, 16
    X, lab = K.unet_batch(B, d, ncls)
    w = K.weight_vector(ncls)
    m_w = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1, loss_weight=w).test_on_batch(X, lab)
    m_s = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1).test_on_batch(X, lab)
    assert m_w[1] > 1e-3 and m_w[1] < 0.5 * m_s[1]
    np.testing.assert_array_equal(m_w[2:], m_s[2:])


@pytest.mark.parametrize("cw", [None, np.ones(94), np.ones((95, 1)), np.where(np.arange(95) == 7, -1.0, 1.0),
                                np.where(np.arange(95) == 7, np.nan, 1.0)],
                         ids=["none", "short", "2d", "negative", "nan"])
def test_atom_unet_weighted_loss_needs_a_usable_vector(cw):
    from icsg3d_amd.unet.unet import AtomUnet
    with pytest.raises(ValueError, match="weighted_loss"):
        AtomUnet(class_weights=cw, input_shape=(16, 16, 16, 1), weighted_loss=True)
    u = AtomUnet(class_weights=cw, input_shape=(16, 16, 16, 1))              # without the flag the vector is only stored
    assert u.weighted_loss is False and u._cw_table is None


def test_atom_unet_keeps_the_table_for_its_engines():
    from icsg3d_amd.unet.unet import AtomUnet
    w = K.weight_vector(95)
    u = AtomUnet(class_weights=w, input_shape=(16, 16, 16, 1), weighted_loss=True)
    w[3] = 99.0                                                              # a copy: the caller's array is not the table
    assert u._cw_table.dtype == np.float32 and u._cw_table[3] != 99.0 and u._eng is None


def test_get_weights_host_loop_is_unchanged(tmp_path):
    from icsg3d_amd.unet.get_weights import get_weights
    assert np.array_equal(get_weights(), np.ones(95)) and np.array_equal(get_weights(n_classes=17), np.ones(17))
    folder = tmp_path / "species_matrices"
    folder.mkdir()
    a = np.zeros((4, 4, 4)); a[0, 0, :3] = [1, 1, 5]
    np.save(str(folder / "a.npy"), a)
    np.save(str(folder / "a_rot_1.npy"), np.full((4, 4, 4), 7.0))
    np.save(str(folder / "b.npy"), np.full((4, 4, 4), 9.0))
    w = get_weights(str(tmp_path), ["a.npy", "a_rot_1.npy"], 10)
    ref = np.zeros(10); ref[0], ref[1], ref[5] = 64 / 61, 64 / 2, 64 / 1
    np.testing.assert_array_equal(w, ref)


def test_train_unet_help_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_unet.py"), "--help"], capture_output=True, text=True,
                         cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--weighted_loss" in out.stdout
