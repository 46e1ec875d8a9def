"""The training monitors without a GPU: the numpy restatement of the KDE against scipy's recorded densities, the 1-2-5
ticks and the axes polylines on closed cases, the monitors' file lists and sidecars with the three ops replaced by the
restatement, and the monitor switch of the two train entry points."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import monitor_ref as MR  # noqa: E402
from make_kde_golden import CASES, STORED, codes  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kde_golden.npz")
PNG = b"\x89PNG\r\n\x1a\n"


@pytest.mark.parametrize("name", list(CASES))
def test_kde_restatement_matches_scipy(name):
    g = np.load(GOLD)
    z = codes(name)
    assert float(z.astype(np.float64).sum()) == float(g["sum_" + name]), "the regenerated codes differ from the recorded ones"
    if name in STORED:
        assert np.array_equal(z, g["codes_" + name])
    dens, bw, status = MR.kde(z, g["x50"])
    assert (status == 0).all() and np.isfinite(bw).all()
    np.testing.assert_allclose(dens, g["dens_" + name], rtol=1e-11, atol=1e-300)
    narrow = CASES[name][3]
    if narrow is not None:
        assert (dens[narrow] == 0).all() and (g["dens_" + name][narrow] == 0).all()
    if name == "65x5":
        np.testing.assert_allclose(MR.kde(z, g["x1"])[0], g["dens_65x5_p1"], rtol=1e-11, atol=1e-300)
        np.testing.assert_allclose(MR.kde(z, g["x65"])[0], g["dens_65x5_p65"], rtol=1e-11, atol=1e-300)


def test_ticks_follow_the_1_2_5_rule():
    from icsg3d_amd.monitor import ticks_125
    assert ticks_125(0, 10) == [0, 2, 4, 6, 8, 10]
    assert ticks_125(-3, 3) == [-2, 0, 2]
    assert ticks_125(0, 1) == [0, 0.2, 0.4, 0.6, 0.8, 1.0]
    assert ticks_125(0, 0.45, 5) == [0, 0.1, 0.2, 0.3, 0.4]
    assert ticks_125(0, 99, 5) == [0, 20, 40, 60, 80]
    assert ticks_125(0, 2400, 4) == [0, 1000, 2000]
    assert ticks_125(3, -3) == [-2, 0, 2]
    assert ticks_125(1, 1) == [] and ticks_125(0, np.inf) == []


def test_axes_curves_are_a_frame_and_nan_padded_ticks():
    from icsg3d_amd.monitor import axes_curves, pad_curves
    cur, xt, yt = axes_curves((0.0, 10.0, -1.0, 1.0))
    assert xt == [0, 2, 4, 6, 8, 10] and yt == [-1.0, -0.5, 0.0, 0.5, 1.0]
    assert cur.shape == (1 + len(xt) + len(yt), 5, 2)
    assert cur[0].tolist() == [[0, -1], [10, -1], [10, 1], [0, 1], [0, -1]]
    assert cur[1, :2].tolist() == [[0, -1], [0, -1 + 0.015 * 2]] and np.isnan(cur[1, 2:]).all()
    assert cur[1 + len(xt), :2].tolist() == [[0, -1], [0.015 * 10, -1]]
    p = pad_curves([[(0, 0), (1, 1), (2, 2)], [(5, 5)]])
    assert p.shape == (2, 3, 2) and np.isnan(p[1, 1:]).all() and p[1, 0].tolist() == [5, 5]


class _FakeEngine:
    """Stands where a UnetEngine / VaeEngine stands: keeps what was uploaded, predicts constants."""

    def __init__(self, d, latent=8, vae=False):
        self.d, self.max_batch, self.latent_dim, self.vae = d, 64, latent, vae
        self._h = None

    def upload_batch(self, X, lab):
        self.X, self.lab = X, lab

    def predict_resident(self, labels_only=False, thresh=0.8):
        self.last = "labels" if labels_only else "probabilities"

    def encode(self, M, cond, eps):
        self.X = np.asarray(M)
        z = np.asarray(eps, np.float32) * 0.5 + 0.1
        self.z = z
        return z, z, z

    def decode(self, z, cond):
        self.recon = np.full((len(z), self.d, self.d, self.d, 1), 0.5, np.float32)
        return self.recon


def _patch_ops(monkeypatch):
    """the three ops -> tests/monitor_ref.py; resident slices read the fake engine's arrays"""
    from icsg3d_amd import monitor as M
    from icsg3d_amd import render as R
    lut = np.asarray(R.VIRIDIS, np.float32)

    def slices(vol, channel=0, axis=2, index=None, zoom=1, vrange=None, lut_=None):
        vol = np.asarray(vol)
        vol = vol[..., None] if vol.ndim == 4 else vol
        return MR.slice_rgba(vol, channel, axis, vol.shape[1] // 2 if index is None else index, zoom, lut, vrange)

    def resident(engine, which, count, channel=0, axis=2, index=None, zoom=1, vrange=None, lut_=None):
        if engine.vae:
            vol = (engine.X, engine.recon)[which]
        else:
            vol = {0: engine.X, 1: engine.lab, 2: engine.X[..., 0], 3: engine.lab}[which]
        return slices(np.asarray(vol)[:count], channel, axis, index, zoom, vrange)

    class Kde:
        def __init__(self, dim, capacity):
            self.rows = []

        def append_vae(self, engine, batch, which="z"):
            self.rows.append(engine.z[:batch])

        def evaluate(self, x):
            z = np.concatenate(self.rows)
            z[:, 2] = 0.0                                           # a collapsed dimension
            return MR.kde(z, x) + (len(z),)

        def close(self):
            pass

    def line_plot(curves, window, size=(640, 480), width_px=1.5, alpha=1.0, palette=None):
        w, h = R._size(size)
        return MR.lines(curves[:3], window, M.CYCLE if palette is None else palette, width_px, alpha, w, h)

    monkeypatch.setattr(M, "slices", slices)
    monkeypatch.setattr(M, "resident_slices", resident)
    monkeypatch.setattr(M, "Kde", Kde)
    monkeypatch.setattr(M, "line_plot", line_plot)


def _png_size(path):
    b = open(path, "rb").read()
    assert b[:8] == PNG
    return int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")


def test_unet_monitor_writes_its_sheets_and_sidecars(tmp_path, monkeypatch):
    from icsg3d_amd import monitor as M
    from icsg3d_amd.unet.data import SyntheticUnetGenerator
    _patch_ops(monkeypatch)
    d = 8
    gen = SyntheticUnetGenerator(12 * 2, 2, (d, d, d), 1, 95, seed=3)

    class Model:
        num_classes = 95
        eng = _FakeEngine(d)

        def _engine(self, batch):
            return self.eng

    mon = M.UnetMonitor(gen, str(tmp_path), zoom=2)
    mon.set_model(Model())
    mon.on_epoch_end(0, {"loss": 2.0, "val_loss": 1.5})
    mon.on_epoch_end(1, {"loss": 1.8, "val_loss": 1.7})            # not a new best: the sheets stay, the curve is redrawn
    names = sorted(os.listdir(tmp_path))
    assert names == ["segmentations_best.json", "segmentations_best.png", "segmentations_binary_best.json",
                     "segmentations_binary_best.png", "unet_loss.json", "unet_loss.png"]
    side, pad = d * 2, 4
    for stem in ("segmentations_best", "segmentations_binary_best"):
        assert _png_size(tmp_path / (stem + ".png")) == (2 * (side + pad) + pad, 10 * (side + pad) + pad)
        meta = json.load(open(tmp_path / (stem + ".json")))
        assert meta["rows"] == 10 and meta["epoch"] == 0 and meta["val_loss"] == 1.5 and len(meta["columns"]) == 2
    assert _png_size(tmp_path / "unet_loss.png") == (640, 480)
    meta = json.load(open(tmp_path / "unet_loss.json"))
    assert meta["series"] == ["train_loss", "val_loss"] and meta["epochs"] == 2 and meta["last"] == [1.8, 1.7]
    assert len(meta["window"]) == 4 and meta["xticks"] and meta["yticks"]


def test_vae_monitor_writes_its_pictures_and_the_kde_report(tmp_path, monkeypatch):
    from icsg3d_amd import monitor as M
    from icsg3d_amd.vae.data import SyntheticVAEGenerator
    _patch_ops(monkeypatch)
    d, bs, latent = 8, 6, 8
    gen = SyntheticVAEGenerator(3 * bs, bs, (d, d, d), 1, 10, seed=4)

    class Vae:
        latent_dim, cond_shape, batch_size = latent, 10, bs
        eng = _FakeEngine(d, latent, vae=True)

        def _engine(self, batch):
            return self.eng

        class decoder:
            @staticmethod
            def predict(inputs):
                return np.random.RandomState(0).uniform(size=(len(inputs[0]), d, d, d, 1)).astype(np.float32)

    state = np.random.get_state()
    mon = M.VaeMonitor(Vae(), gen, str(tmp_path), seed=5, zoom=2)
    mon.best(3)
    mon.losses(np.array([[3.0, 2.5], [2.0, 2.2], [9.0, 9.0]]), 2)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:], \
        "the monitor drew from training's np.random stream"
    assert sorted(os.listdir(tmp_path)) == ["vae_kde.json", "vae_kde.png", "vae_kde.svg", "vae_losses.json",
                                            "vae_losses.png", "vae_reconstructions.json", "vae_reconstructions.png",
                                            "vae_samples.json", "vae_samples.png"]
    side, pad = d * 2, 4
    assert _png_size(tmp_path / "vae_reconstructions.png") == (2 * (side + pad) + pad, (bs // 2) * (side + pad) + pad)
    assert _png_size(tmp_path / "vae_samples.png") == (2 * (side + pad) + pad, (bs // 2) * (side + pad) + pad)
    assert _png_size(tmp_path / "vae_kde.png") == (640, 480) and _png_size(tmp_path / "vae_losses.png") == (640, 480)
    k = json.load(open(tmp_path / "vae_kde.json"))
    assert k["x"] == [float(v) for v in np.linspace(-3, 3, 50)]
    assert k["count"] >= 1000 and k["count"] % bs == 0 and k["count"] - bs < 1000
    assert len(k["bandwidth"]) == latent and k["status"] == [0, 0, 1, 0, 0, 0, 0, 0] and k["collapsed"] == 1
    assert k["y_range"][0] == 0.0 and k["y_range"][1] > 0 and k["epoch"] == 3
    assert open(tmp_path / "vae_kde.svg").read().count("<polyline") == latent - 1
    r = json.load(open(tmp_path / "vae_reconstructions.json"))
    assert r["rows"] == bs // 2 and len(r["ids"]) == bs // 2 and r["columns"] == ["input", "reconstruction"]
    assert json.load(open(tmp_path / "vae_losses.json"))["epochs"] == 2


def test_train_entry_points_take_the_monitor_switch_and_default_to_off(monkeypatch):
    """monitor=True is accepted by both; with it off no monitor object is made and no monitor module is imported."""
    from icsg3d_amd.unet.unet import AtomUnet, TrainingPlot, _BestCheckpoint
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    for fn in (AtomUnet.train_generator, LatticeDFCVAE.train):
        p = inspect.signature(fn).parameters
        assert "monitor" in p and p["monitor"].default is False
    seen = []
    unet = AtomUnet.__new__(AtomUnet)
    unet.filepath = "/nonexistent/unet.hdf5"
    unet._dp = None

    class Model:
        def fit_generator(self, **kw):
            seen.append(kw)

        def save(self, path):
            pass
    unet.model = Model()
    sys.modules.pop("icsg3d_amd.monitor", None)
    unet.train_generator("T", "V", epochs=2, output_dir="out")
    assert "icsg3d_amd.monitor" not in sys.modules
    kw = seen[-1]
    assert [type(c) for c in kw["callbacks"]] == [_BestCheckpoint, TrainingPlot]
    assert kw["generator"] == "T" and kw["validation_data"] == "V" and kw["epochs"] == 2 and kw["workers"] == 4
    unet.train_generator("T", "V", epochs=2, output_dir="out", monitor=True)
    from icsg3d_amd.monitor import UnetMonitor
    cbs = seen[-1]["callbacks"]
    assert [type(c) for c in cbs] == [_BestCheckpoint, TrainingPlot, UnetMonitor]
    assert cbs[-1].model is unet and cbs[-1].sdir == "out" and cbs[-1].val_gen == "V"
    for script in ("train_unet.py", "train_vae.py"):
        text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), script)).read()
        assert '"--monitor"' in text and "monitor=a.monitor" in text


def test_render_slice_refuses_a_null_volume_before_any_device_call():
    from icsg3d_amd import _lib as L
    lib = L.load()
    lut, out = np.zeros((256, 3), np.float32), np.zeros((1, 4, 4, 4), np.float32)
    rc = lib.ics_op_render_slice(None, 0, 1, 4, 1, 0, 2, 0, L.fptr(lut), None, 1, L.fptr(out))
    msg = (lib.ics_last_error() or b"").decode()
    assert rc != 0 and msg.startswith("ics_op_render_slice: null vol ("), msg
