"""Fed steps on the GPU (include/icsg3d.h "fed steps", csrc/feed.h): the pack kernel against its numpy statement, fed
train / test steps against the synchronous ones, the class-level loops with feed=True against feed=False, and every
refusal.  Everything is compared bit for bit: a fed step runs the same resident step on the same bytes, so a difference
is a finding about ordering, not a tolerance to add."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 16


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ 1. the pack kernel alone
def cast_probes(dtype):
    """values whose float32 image depends on the rounding rule, the denormal handling, the sign of zero and the range"""
    if dtype == np.float64:
        v = [1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, -(1.0 + 2.0 ** -24),   # halfway cases
             1e-40, -3e-45, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * 1.5, 5e-324, 2.0 ** -126 * (1 - 2.0 ** -25),   # denormals
             -0.0, 0.0, 1e39, -1e39, 3.4028235677973366e38, float(np.finfo(np.float32).max), np.inf, -np.inf]
    else:
        v = [np.float32(1e-40), np.float32(-1e-45), -0.0, 0.0, np.inf, -np.inf, np.finfo(np.float32).max,
             np.finfo(np.float32).tiny]
    return np.array(v, dtype)


def one_hot_cases(rng, B, d, ncls):
    y = np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, (B, d, d, d))]
    flat = y.reshape(-1, ncls)
    flat[0] = 0.0                                               # an all-zero row -> 0
    flat[1] = 0.0; flat[1, [ncls - 1, ncls // 2]] = 1.0         # two equal maxima -> the lower index
    flat[2] = 0.0; flat[2, [0, ncls - 1]] = 2.5
    flat[3] = -1.0; flat[3, ncls - 1] = -0.5                    # negative rows: the maximum is not the first column
    flat[4] = -np.inf                                           # nothing above -inf -> 0
    n = min(len(flat) - 8, 64)
    flat[5:5 + n] = rng.integers(0, 4, (n, ncls)).astype(np.float32)     # soft rows with many ties
    flat[5 + n - 1, :] = 7.0                                    # every column equal
    flat[5 + n] = 1.0; flat[5 + n, [ncls - 1, ncls // 2]] = np.nan   # np.argmax: the first NaN wins
    flat[6 + n] = np.nan                                        # nothing but NaN -> 0
    flat[7 + n] = np.inf; flat[7 + n, ncls - 1] = np.nan        # a NaN is above +inf
    return y


@pytest.mark.parametrize("mix", [(np.float64, np.float64), (np.float32, np.float64), (np.float32, np.float32)],
                         ids=["f64f64", "f32f64", "f32f32"])
@pytest.mark.parametrize("channels", [1, 4])
def test_pack_kernel_matches_its_numpy_statement(channels, mix):
    from icsg3d_amd.engine import feed_pack
    from icsg3d_amd.feed import pack_reference
    d = 8
    rng = np.random.default_rng(channels * 10 + len(str(mix)))
    label_cases = [("u8", 0), ("f64", 0), ("f32", 0), ("onehot", 2), ("onehot", 95), ("onehot", 127), ("none", 0)]
    for B in (1, 3):
        parts = []
        for c, t in zip((1,) if channels == 1 else (1, 3), mix):
            a = ((rng.random((B, d, d, d, c)) - 0.5) * 10.0 ** rng.integers(-3, 4, (B, d, d, d, c))).astype(t)
            p = cast_probes(t)
            a.reshape(-1)[:len(p)] = p
            a.reshape(-1)[-len(p):] = p[::-1]
            parts.append(a)
        for kind, ncls in label_cases:
            if kind == "onehot":
                lab = one_hot_cases(rng, B, d, ncls)
            elif kind == "none":
                lab = None
            else:
                lab = rng.integers(0, 256, (B, d, d, d)).astype({"u8": np.uint8, "f64": np.float64, "f32": np.float32}[kind])
                lab.reshape(-1)[:4] = [0, 255, 94, 1]
            with np.errstate(over="ignore"):
                want_x, want_l = pack_reference(parts, lab, kind)
            got_x, got_l = feed_pack(parts, lab, kind, ncls)
            assert same_bits(got_x, want_x), (B, kind, np.flatnonzero(bits(got_x).ravel() != bits(want_x).ravel())[:8])
            if kind == "none":
                assert got_l is None
            else:
                assert same_bits(got_l, want_l), (B, kind, ncls, np.flatnonzero(got_l.ravel() != want_l.ravel())[:8])
    # one part with several channels (a generator's float64 X): a cast copy
    X = np.concatenate([np.asarray(p, np.float64) for p in parts], axis=-1) if channels == 4 else parts[0]
    with np.errstate(over="ignore"):
        assert same_bits(feed_pack([X])[0], pack_reference([X])[0])


def test_pack_kernel_general_channel_split():
    """splits other than 1 and 1 + 3 take the element-wise path"""
    from icsg3d_amd.engine import feed_pack
    from icsg3d_amd.feed import pack_reference
    rng = np.random.default_rng(5)
    for c0, c1, t0, t1 in ((2, 3, np.float64, np.float32), (3, 1, np.float32, np.float64), (1, 1, np.float64, np.float64)):
        parts = [rng.standard_normal((2, 8, 8, 8, c0)).astype(t0), rng.standard_normal((2, 8, 8, 8, c1)).astype(t1)]
        lab = rng.integers(0, 95, (2, 8, 8, 8)).astype(np.float64)
        gx, gl = feed_pack(parts, lab, "f64")
        wx, wl = pack_reference(parts, lab, "f64")
        assert same_bits(gx, wx) and same_bits(gl, wl)


# ------------------------------------------------------------------------------------------ 2. / 3. fed step == synchronous step
BATCHES = [3, 5, 2, 5, 3, 4]
MAXB = 5


def unet_engine(C=4, seed=1):
    from icsg3d_amd.engine import UnetEngine
    from icsg3d_amd.synthetic import glorot_params, unet_param_shapes
    e = UnetEngine(in_channels=C, num_classes=95, d=D, max_batch=MAXB, lr=1e-4)
    e.set_weights(glorot_params(unet_param_shapes(C, 95), seed))
    return e


def vae_engine(ue, C):
    from icsg3d_amd.engine import VaeEngine
    from icsg3d_amd.synthetic import glorot_params, vae_param_shapes
    e = VaeEngine(ue, in_channels=C, d=D, max_batch=MAXB, lr=5e-4)
    e.set_weights(glorot_params(vae_param_shapes(C, d=D), 3))
    return e


def raw_batches(C, seed):
    """per step: raw float64 parts (M, p), float64 ids, cond, eps -- different data every step; the ops in order"""
    from icsg3d_amd.synthetic import synthetic_batch
    rng = np.random.default_rng(seed)
    ops = [("train", b) for b in BATCHES]
    ops.insert(3, ("test", 4))
    out = []
    for k, (kind, b) in enumerate(ops):
        X, lab, cond = synthetic_batch(b, D, C, seed=seed + 11 * k, noise=1e-3)
        X = X.astype(np.float64) + rng.random(X.shape) * 1e-9          # doubles a float cannot hold
        out.append({"kind": kind, "B": b, "parts": [X[..., :1].copy(), X[..., 1:].copy()] if C == 4 else [X],
                    "ids": lab.astype(np.float64), "cond": cond[:, :10].astype(np.float32),
                    "eps": rng.standard_normal((b, 256)).astype(np.float32)})
    return out


def state(e):
    m, v, t = e.get_optimizer_state()
    return e.get_weights(), m, v, t


def assert_same_state(a, b):
    wa, ma, va, ta = a
    wb, mb, vb, tb = b
    assert ta == tb and sorted(wa) == sorted(wb)
    for k in wa:
        assert same_bits(wa[k], wb[k]), k
    assert same_bits(ma, mb) and same_bits(va, vb)


def scribble(views):
    for a in views["x"] + [views["labels"], views["cond"], views["eps"]]:
        if a is not None:
            a.reshape(-1).view(np.uint8)[:] = 0xA5


def fill(views, item, contract):
    """item into a slot's pinned views, after overwriting all of them with garbage"""
    scribble(views)
    B = item["B"]
    if contract == "files":
        for v, p in zip(views["x"], item["parts"]):
            v[:B] = p
        if views["labels"] is not None:
            views["labels"][:B] = item["ids"]
    else:                      # the reference's generator: one float64 X, a one-hot y
        views["x"][0][:B] = np.concatenate(item["parts"], axis=-1)
        if views["labels"] is not None:
            views["labels"][:B] = np.eye(95, dtype=np.float32)[item["ids"].astype(np.int64)]
    if views["cond"] is not None:
        views["cond"][:B] = item["cond"]
        views["eps"][:B] = item["eps"]


def run_fed(eng, items, slots, contract, vae):
    """All slots are submitted before any is stepped, each slot is scribbled over as soon as feed_slot hands it back
    (also between its submit and its step), and each ticket is read two steps late.  Returns the metrics per step."""
    C = sum(p.shape[-1] for p in items[0]["parts"])
    if contract == "files":
        xc, xt = ((1, 3), (np.float64, np.float64)) if C == 4 else ((1,), (np.float64,))
        kind = "none" if vae else "f64"
    else:
        xc, xt, kind = (C,), (np.float64,), "none" if vae else "onehot"
    eng.feed_open(xc, xt, kind, slots)
    n = len(items)
    for k in range(min(slots, n)):
        fill(eng.feed_slot(k), items[k], contract)
        eng.feed_submit(k, items[k]["B"])
    for k in range(min(slots, n)):
        scribble(eng.feed_slot(k))          # the upload has left the pinned memory: the step must not see this
    tickets, out = [], [None] * n
    for k in range(n):
        slot = k % slots
        step = eng.train_step_fed if items[k]["kind"] == "train" else eng.test_step_fed
        tickets.append(step(slot))
        if k + slots < n:
            fill(eng.feed_slot(slot), items[k + slots], contract)
            eng.feed_submit(slot, items[k + slots]["B"])
        if k >= 2:
            out[k - 2] = eng.feed_metrics(tickets[k - 2]).copy()
    for k in range(max(0, n - 2), n):
        out[k] = eng.feed_metrics(tickets[k]).copy()
    assert tickets == list(range(n))
    assert same_bits(eng.feed_metrics(tickets[0]), out[0])      # a ticket inside the ring can be read again
    eng.feed_close()
    return out


def host_arrays(item):
    """what the synchronous loop uploads: the host-side cast, concatenate and label conversion"""
    from icsg3d_amd.feed import pack_reference
    return pack_reference(item["parts"], item["ids"], "f64")


@pytest.mark.parametrize("slots,contract", [(2, "files"), (3, "generator")])
def test_fed_unet_steps_equal_the_synchronous_steps(slots, contract, monkeypatch):
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")       # guard bytes behind every buffer, the staging slots included
    items = raw_batches(4, 100)
    ref, fed = unet_engine(), unet_engine()
    want = []
    for it in items:
        x, lab = host_arrays(it)
        want.append((ref.train_step if it["kind"] == "train" else ref.test_step)(x, lab))
    got = run_fed(fed, items, slots, contract, vae=False)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (5,) and same_bits(g, w), (k, items[k]["kind"], g, w)
    assert_same_state(state(fed), state(ref))
    assert fed.check_canaries()[0] == 0
    # the engine is an ordinary engine again: the synchronous step still agrees
    x, lab = host_arrays(items[0])
    assert same_bits(fed.train_step(x, lab), ref.train_step(x, lab))


@pytest.mark.parametrize("C,slots,contract", [(4, 2, "files"), (1, 3, "files"), (4, 2, "generator")])
def test_fed_vae_steps_equal_the_synchronous_steps(C, slots, contract):
    items = raw_batches(C, 200 + C)
    ru, fu = unet_engine(C), unet_engine(C)
    ref, fed = vae_engine(ru, C), vae_engine(fu, C)
    frozen = fu.get_weights()
    want = []
    for it in items:
        x, _ = host_arrays(it)
        want.append((ref.train_step if it["kind"] == "train" else ref.test_step)(x, it["cond"], it["eps"]))
    got = run_fed(fed, items, slots, contract, vae=True)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (4,) and same_bits(g, w), (k, items[k]["kind"], g, w)
    assert_same_state(state(fed), state(ref))
    after = fu.get_weights()
    for k in frozen:                                             # the perceptual U-Net stays frozen
        assert same_bits(frozen[k], after[k]), k


# ------------------------------------------------------------------------------------------ 4. class level
def write_dataset(root, n=8):
    from icsg3d_amd.synthetic import synthetic_batch
    rng = np.random.default_rng(9)
    for sub in ("density_matrices", "species_matrices", "coordinate_grids"):
        os.makedirs(os.path.join(root, sub))
    ids = ["mp-%d.npy" % i for i in range(n)]
    for k, f in enumerate(ids):
        X, lab, _ = synthetic_batch(1, D, 4, seed=40 + k, noise=1e-3)
        X = X.astype(np.float64) + rng.random(X.shape) * 1e-9
        np.save(os.path.join(root, "density_matrices", f), X[0, ..., 0].ravel())       # float64, flat (create_matrices.py)
        np.save(os.path.join(root, "coordinate_grids", f), X[0, ..., 1:4])
        np.save(os.path.join(root, "species_matrices", f), lab[0].astype(np.float64))
    csv = os.path.join(root, "prop.csv")
    with open(csv, "w") as fh:
        fh.write("task_id,formation_energy_per_atom,nsites\n")
        for i in range(n):
            fh.write("mp-%d,%.5f,%d\n" % (i, rng.normal(), 2 + i))
    return ids, csv


class ReferenceContract:
    """a generator with the reference's contract: float64 X, [one-hot y, mask]"""

    def __init__(self, gen):
        self.gen, self.batch_size = gen, gen.batch_size

    def __len__(self):
        return len(self.gen)

    def __getitem__(self, i):
        g = self.gen
        ids = [g.list_IDs[k] for k in g.indexes[i * g.batch_size:(i + 1) * g.batch_size]]
        X = np.stack([g.create_lattice_meshgrid(f, g.n_channels) for f in ids])          # float64, as loaded
        y = np.stack([np.load(os.path.join(g.data_path, "species_matrices", f)).reshape(g.dim) for f in ids]).astype(np.int64)
        assert X.dtype == np.float64
        return X, [np.eye(g.n_classes, dtype=np.float32)[y], (y != 0).astype(np.float32)[..., None]]


@pytest.mark.parametrize("contract", ["files", "generator"])
def test_fit_generator_fed_equals_unfed(tmp_path, contract):
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    ids, _ = write_dataset(str(tmp_path))
    kw = dict(data_path=str(tmp_path), dim=(D, D, D), n_channels=4)
    wrap = ReferenceContract if contract == "generator" else (lambda g: g)
    runs = []
    for feed in (False, True):
        np.random.seed(4)
        unet = AtomUnet(input_shape=(D, D, D, 4), lr=1e-4, max_batch=3)
        tg, vg = wrap(UnetDataGenerator(ids[:6], batch_size=3, **kw)), wrap(UnetDataGenerator(ids[6:], batch_size=2, **kw))
        hist = unet.model.fit_generator(tg, validation_data=vg, epochs=2, verbose=0, feed=feed)
        runs.append((hist, unet._get_weights(), unet._eng.get_optimizer_state()))
    (h0, w0, o0), (h1, w1, o1) = runs
    assert len(h0) == len(h1) == 2
    for a, b in zip(h0, h1):
        assert sorted(a) == sorted(b) and len(a) == 10
        for k in a:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])
    for k in w0:
        assert same_bits(w0[k], w1[k]), k
    assert o0[2] == o1[2] == 4 and same_bits(o0[0], o1[0]) and same_bits(o0[1], o1[1])


def test_vae_train_fed_equals_unfed(tmp_path, C=4):
    from icsg3d_amd.checkpoint import load_weights
    from icsg3d_amd.synthetic import glorot_params, unet_param_shapes
    from icsg3d_amd.vae.data import VAEDataGenerator
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    ids, csv = write_dataset(str(tmp_path / "data"))
    kw = dict(data_path=str(tmp_path / "data"), dim=(D, D, D), n_channels=C, property_csv=csv, n_bins=3)
    pm = glorot_params(unet_param_shapes(C, 95), 1)
    runs = []
    for feed in (False, True):
        np.random.seed(6)
        out = tmp_path / ("fed" if feed else "unfed")
        os.makedirs(out)
        vae = LatticeDFCVAE(input_shape=(D, D, D, C), perceptual_model=pm, cond_shape=3, output_dir=str(out))
        tg, vg = VAEDataGenerator(ids[:6], batch_size=3, **kw), VAEDataGenerator(ids[6:], batch_size=2, **kw)
        vae.train(tg, vg, epochs=2, weights=str(out / "vae.best.hdf5"), feed=feed)
        runs.append((np.array(vae.losses), load_weights(str(out / "vae.best.hdf5"), "vae"), vae._get_weights()))
    (l0, s0, w0), (l1, s1, w1) = runs
    assert l0.shape == (2, 2) and l0.tobytes() == l1.tobytes(), (l0, l1)
    assert sorted(s0) == sorted(s1)
    for k in s0:
        assert same_bits(np.asarray(s0[k]), np.asarray(s1[k])), k
    for k in w0:
        assert same_bits(w0[k], w1[k]), k


# ------------------------------------------------------------------------------------------ 5. refusals
def test_every_refusal_names_its_problem_and_leaves_the_engine_usable():
    from icsg3d_amd import _lib as L
    from icsg3d_amd.engine import feed_config
    lib = L.load()
    ue = unet_engine()
    ve = vae_engine(ue, 4)
    items = raw_batches(4, 300)
    x, lab = host_arrays(items[0])
    before = ue.train_step(x, lab)
    tk = C.c_int(-1)
    m = np.zeros(8, np.float32)

    def refused(rc, *words):
        msg = lib.ics_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)

    none = [None] * 5
    cfg = feed_config((1, 3), (np.float64, np.float64), "f64", 2)
    # without a feed
    refused(lib.ics_net_feed_slot(ue._h, 0, *none), "no open feed")
    refused(lib.ics_net_feed_submit(ue._h, 0, 1), "no open feed")
    refused(lib.ics_unet_train_step_fed(ue._h, 0, C.byref(tk)), "no open feed")
    refused(lib.ics_net_feed_metrics(ue._h, 0, L.fptr(m)), "no open feed")
    refused(lib.ics_net_feed_close(ue._h), "no open feed")
    # a config that does not match the engine
    refused(lib.ics_net_feed_open(ue._h, C.byref(feed_config((1, 2), (np.float64,) * 2, "f64"))), "in_channels")
    refused(lib.ics_net_feed_open(ue._h, C.byref(feed_config((1, 3), (np.float64,) * 2, "none"))), "needs labels")
    refused(lib.ics_net_feed_open(ve._h, C.byref(cfg)), "takes no labels")
    refused(lib.ics_net_feed_open(ue._h, C.byref(feed_config((1, 3), (np.float64,) * 2, "f64", slots=5))), "slots")
    refused(lib.ics_net_feed_open(ue._h, C.byref(feed_config((1, 3), (np.float64,) * 2, "f64", slots=1))), "slots")
    ue.feed_open((1, 3), (np.float64, np.float64), "f64", 2)
    ve.feed_open((4,), (np.float32,), "none", 2)
    refused(lib.ics_net_feed_open(ue._h, C.byref(cfg)), "already open")
    # a bad slot index
    refused(lib.ics_net_feed_slot(ue._h, 2, *none), "bad slot index")
    refused(lib.ics_net_feed_slot(ue._h, -1, *none), "bad slot index")
    refused(lib.ics_net_feed_submit(ue._h, 7, 1), "bad slot index")
    refused(lib.ics_unet_train_step_fed(ue._h, 2, C.byref(tk)), "bad slot index")
    # submit of a slot that was never obtained; a step on a slot that was never submitted
    refused(lib.ics_net_feed_submit(ue._h, 0, 1), "never obtained")
    refused(lib.ics_unet_train_step_fed(ue._h, 0, C.byref(tk)), "never submitted")
    refused(lib.ics_unet_test_step_fed(ue._h, 1, C.byref(tk)), "never submitted")
    fill(ue.feed_slot(0), items[0], "files")
    refused(lib.ics_net_feed_submit(ue._h, 0, MAXB + 1), "max_batch")
    refused(lib.ics_net_feed_submit(ue._h, 0, 0), "max_batch")
    # the wrong net kind
    refused(lib.ics_vae_train_step_fed(ue._h, 0, C.byref(tk)), "wrong engine kind")
    refused(lib.ics_vae_test_step_fed(ue._h, 0, C.byref(tk)), "wrong engine kind")
    refused(lib.ics_unet_train_step_fed(ve._h, 0, C.byref(tk)), "wrong engine kind")
    refused(lib.ics_unet_test_step_fed(ve._h, 0, C.byref(tk)), "wrong engine kind")
    # the feed still works: one step, then a second step on the consumed slot, a second submit of a pending one
    ue.feed_submit(0, items[0]["B"])
    refused(lib.ics_net_feed_submit(ue._h, 0, 1), "no step has consumed")
    t = ue.train_step_fed(0)
    refused(lib.ics_unet_train_step_fed(ue._h, 0, C.byref(tk)), "already consumed")
    refused(lib.ics_net_feed_metrics(ue._h, t + 1, L.fptr(m)), "ticket")
    refused(lib.ics_net_feed_metrics(ue._h, -1, L.fptr(m)), "ticket")
    got = ue.feed_metrics(t)
    # a ticket older than the ring of 64
    fill(ue.feed_slot(1), items[1], "files")          # valid class ids: the pinned memory of a fresh slot holds anything
    for _ in range(64):
        ue.feed_slot(1)
        ue.feed_submit(1, 1)
        last = ue.test_step_fed(1)
    refused(lib.ics_net_feed_metrics(ue._h, t, L.fptr(m)), "older than the ring")
    assert np.all(np.isfinite(ue.feed_metrics(last)))
    ue.feed_close()
    ve.feed_close()
    # ... and the engine: the fed step was the step a fresh engine takes second, and the synchronous path goes on
    ref = unet_engine()
    assert same_bits(ref.train_step(x, lab), before)
    assert same_bits(ref.train_step(x, lab), got)
    assert np.all(np.isfinite(ue.train_step(x, lab)))
    assert np.all(np.isfinite(ve.train_step(x, items[0]["cond"], items[0]["eps"])))
