"""Fed steps, host side (no GPU): feed.pack_reference over the raw file payloads equals what the file generators hand
the synchronous loop, and the Feeder's slot schedule holds against a fake engine that records every call."""
import os

import numpy as np
import pytest

from icsg3d_amd import feed

D = 8
IDS = ["mp-%d.npy" % i for i in range(6)]


def write_dataset(root, species_dtype=np.float64, m_dtype=np.float64, p_dtype=np.float64):
    rng = np.random.default_rng(3)
    for sub in ("density_matrices", "species_matrices", "coordinate_grids"):
        os.makedirs(os.path.join(root, sub))
    for f in IDS:
        # doubles with more mantissa than a float holds: the cast matters
        np.save(os.path.join(root, "density_matrices", f), rng.random(D ** 3).astype(m_dtype))             # stored flat
        np.save(os.path.join(root, "coordinate_grids", f), (rng.random((D, D, D, 3)) * 7.0).astype(p_dtype))
        np.save(os.path.join(root, "species_matrices", f), rng.integers(0, 95, (D, D, D)).astype(species_dtype))
    csv = os.path.join(root, "prop.csv")
    with open(csv, "w") as fh:
        fh.write("task_id,formation_energy_per_atom,nsites\n")
        for i in range(6):
            fh.write("mp-%d,%.4f,%d\n" % (i, rng.normal(), 3 + i))
    return csv


def views_for(spec, max_batch, d, num_classes=95, ncond=0, latent=0):
    """numpy stand-ins for a slot's pinned views (UnetEngine.feed_slot's dict)"""
    xc, xt, kind = spec
    ldt = {"u8": np.uint8, "f32": np.float32, "f64": np.float64, "onehot": np.float32}.get(kind)
    lshape = (max_batch, d, d, d, num_classes) if kind == "onehot" else (max_batch, d, d, d)
    return {"x": [np.full((max_batch, d, d, d, c), 777, t) for c, t in zip(xc, xt)],
            "labels": None if ldt is None else np.full(lshape, 77, ldt),
            "cond": np.full((max_batch, ncond), 7, np.float32) if ncond else None,
            "eps": np.full((max_batch, latent), 7, np.float32) if latent else None}


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("dtypes", [(np.float64, np.float64, np.float64), (np.float32, np.float64, np.uint8),
                                    (np.float64, np.float32, np.int64)])
def test_pack_reference_over_raw_payloads_equals_the_generators(tmp_path, channels, dtypes):
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.vae.data import VAEDataGenerator
    m_dt, p_dt, s_dt = dtypes
    csv = write_dataset(str(tmp_path), s_dt, m_dt, p_dt)
    g = UnetDataGenerator(IDS, str(tmp_path), batch_size=2, dim=(D, D, D), n_channels=channels)
    spec = g.feed_spec()
    assert spec[0] == ((1,) if channels == 1 else (1, 3))
    assert spec[1] == ((np.dtype(m_dt),) if channels == 1 else (np.dtype(m_dt), np.dtype(p_dt)))
    assert spec[2] == {np.float64: "f64", np.uint8: "u8", np.int64: "u8"}[s_dt]
    for i in range(len(g)):
        v = views_for(spec, 3, D)                       # a slot larger than the batch
        assert g.fill(i, v) == 2
        for part, t in zip(v["x"], spec[1]):
            assert part.dtype == t                      # raw payloads: no host cast of x
        x, lab = feed.pack_reference([p[:2] for p in v["x"]], v["labels"][:2], spec[2])
        X, (y, _) = g[i]
        assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), np.asarray(X, np.float32).view(np.uint32))
        assert lab.dtype == np.uint8 and np.array_equal(lab, y)
        assert np.all(v["x"][0][2] == 777)              # rows beyond the batch untouched
    vg = VAEDataGenerator(IDS, str(tmp_path), batch_size=3, dim=(D, D, D), n_channels=channels, property_csv=csv, n_bins=3)
    vspec = vg.feed_spec()
    assert vspec[2] == "none" and vspec[:2] == spec[:2]
    for i in range(len(vg)):
        v = views_for(vspec, 3, D, ncond=3)
        assert vg.fill(i, v, lambda f, it: [f(k) for k in reversed(list(it))]) == 3      # any order: disjoint rows
        x, lab = feed.pack_reference(v["x"], None, "none")
        M, cond = vg[i]
        assert lab is None and np.array_equal(x.view(np.uint32), np.asarray(M, np.float32).view(np.uint32))
        assert np.array_equal(v["cond"], cond)


def test_pack_reference_argmax_and_cast_rules():
    oh = np.zeros((1, 2, 2, 2, 5), np.float32)
    oh[0, 0, 0, 0] = [0, 3, 3, 1, 3]          # equal maxima: the lowest index
    oh[0, 0, 0, 1, 4] = 1.0
    with np.errstate(over="ignore"):
        x, lab = feed.pack_reference([np.array([[[[[1.0 + 2.0 ** -24], [1e39]]]]])], oh, "onehot")
    assert lab[0, 0, 0, 0] == 1 and lab[0, 0, 0, 1] == 4 and lab[0, 1, 1, 1] == 0         # all-zero row -> 0
    assert x[0, 0, 0, 0, 0] == np.float32(1.0) and np.isinf(x[0, 0, 0, 1, 0])            # ties to even; overflow -> inf


# ------------------------------------------------------------------------------------------ the Feeder's schedule
class FakeEngine:
    """Records every feed call and checks the slot rules at the moment they could be broken."""
    num_classes = 5

    def __init__(self, max_batch=4, d=2, vae=False):
        self.max_batch, self.d, self.log, self.errors = max_batch, d, [], []
        self.open, self.closed, self.reads = False, 0, {}
        if vae:
            self.latent_dim, self.cond_shape = 3, 2

    def feed_open(self, x_channels, x_dtypes, label_kind, slots):
        assert not self.open
        self.open, self.spec, self.nslots = True, (tuple(x_channels), tuple(x_dtypes), label_kind), slots
        vae = hasattr(self, "latent_dim")
        self.views = [views_for(self.spec, self.max_batch, self.d, self.num_classes, 2 if vae else 0, 3 if vae else 0)
                      for _ in range(slots)]
        self.pending, self.snap, self.tickets, self.stepped = {}, {}, [], []

    def _flat(self, slot, batch):
        v = self.views[slot]
        return np.concatenate([a[:batch].astype(np.float64).ravel() for a in v["x"] + [v["labels"], v["cond"], v["eps"]]
                               if a is not None])

    def feed_slot(self, slot):
        self.log.append(("slot", slot))
        if slot in self.pending:
            self.errors.append("slot %d handed back for rewriting before its step was enqueued" % slot)
        return self.views[slot]

    def feed_submit(self, slot, batch):
        self.log.append(("submit", slot, batch))
        if slot in self.pending:
            self.errors.append("slot %d submitted twice" % slot)
        self.pending[slot] = batch
        self.snap[slot] = self._flat(slot, batch)

    def _step(self, kind, slot):
        self.log.append((kind, slot))
        if slot not in self.pending:
            self.errors.append("slot %d stepped without a submit (or twice)" % slot)
            return -1
        batch = self.pending.pop(slot)
        if not np.array_equal(self._flat(slot, batch), self.snap[slot]):
            self.errors.append("slot %d rewritten between its submit and its step" % slot)
        self.tickets.append((kind, batch, float(self.snap[slot].sum())))
        return len(self.tickets) - 1

    def train_step_fed(self, slot):
        return self._step("train", slot)

    def test_step_fed(self, slot):
        return self._step("test", slot)

    def feed_metrics(self, ticket):
        self.log.append(("metrics", ticket))
        self.reads[ticket] = self.reads.get(ticket, 0) + 1
        if ticket + 2 < len(self.tickets):
            self.errors.append("ticket %d read more than one step late" % ticket)
        kind, batch, total = self.tickets[ticket]
        return np.array([ticket, batch, total], np.float32)

    def feed_close(self):
        assert self.open
        self.open, self.closed = False, self.closed + 1


class ListGen:
    """the reference's contract: float64 X, [one-hot y, mask]; batches may differ in size"""

    def __init__(self, sizes, d=2, fail_at=None):
        rng = np.random.default_rng(1)
        self.items, self.fail_at = [], fail_at
        for b in sizes:
            X = rng.random((b, d, d, d, 4))
            y = np.eye(5, dtype=np.float32)[rng.integers(0, 5, (b, d, d, d))]
            self.items.append((X, [y, (y[..., 0] == 0).astype(np.float32)[..., None]]))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        if i == self.fail_at:
            raise OSError("batch %d is unreadable" % i)
        return self.items[i]


def expected_total(item):
    X, (y, _) = item
    return float(np.concatenate([X.ravel(), y.astype(np.float64).ravel()]).sum())


@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("workers", [0, 4])
@pytest.mark.parametrize("sizes", [[4, 4, 4, 4, 4, 4, 4], [4, 4, 4, 1], [3]])
def test_feeder_schedule_against_a_recording_engine(slots, workers, sizes):
    eng, gen = FakeEngine(), ListGen(sizes)
    out = list(feed.Feeder(eng, gen, workers=workers, slots=slots))
    assert eng.errors == []
    assert eng.spec == ((4,), (np.dtype(np.float64),), "onehot")            # no host cast: float64 X, one-hot y as they are
    # one step per batch, in order, each on the data of its own batch (a short final batch included)
    assert [int(m[0]) for m in out] == list(range(len(sizes))) and [int(m[1]) for m in out] == sizes
    for m, item in zip(out, gen.items):
        assert m[2] == np.float32(expected_total(item))
    assert sorted(eng.reads) == list(range(len(sizes))) and set(eng.reads.values()) == {1}    # every ticket, exactly once
    assert eng.closed == 1 and not eng.open
    steps = [e for e in eng.log if e[0] == "train"]
    assert [s[1] for s in steps] == [k % slots for k in range(len(sizes))]
    # one batch in flight ahead: batch k+1 is submitted after step k was enqueued, and step k's metrics are read after
    # step k+1 was enqueued
    S = [i for i, e in enumerate(eng.log) if e[0] == "submit"]
    T = [i for i, e in enumerate(eng.log) if e[0] == "train"]
    R = [i for i, e in enumerate(eng.log) if e[0] == "metrics"]
    assert len(S) == len(T) == len(R) == len(sizes)
    for k in range(len(sizes)):
        assert S[k] < T[k] < R[k]
        if k + 1 < len(sizes):
            assert T[k] < S[k + 1] < T[k + 1] < R[k]


def test_feeder_runs_test_steps_and_the_vae_contract():
    eng = FakeEngine(vae=True)

    class VaeGen:
        def __len__(self):
            return 3

        def __getitem__(self, i):
            return np.full((2, 2, 2, 2, 1), i + 1, np.float32), np.eye(2, dtype=np.float32)

    draws = []

    def eps(n):
        draws.append(n)
        return np.full((n, 3), len(draws), np.float64)

    out = list(feed.Feeder(eng, VaeGen(), training=False, eps=eps))
    assert eng.errors == [] and draws == [2, 2, 2] and eng.spec == ((1,), (np.dtype(np.float32),), "none")
    assert [e[0] for e in eng.log if e[0] in ("train", "test")] == ["test"] * 3
    # x = (i + 1) * 16 elements, cond = 2 ones, eps = (i + 1) * 6: the draw of step i went with batch i
    assert [m[2] for m in out] == [np.float32(16 * (i + 1) + 2 + 6 * (i + 1)) for i in range(3)]


@pytest.mark.parametrize("fail_at", [0, 2, 4])
def test_feeder_reraises_a_generator_exception_and_closes_the_feed(fail_at):
    eng, gen = FakeEngine(), ListGen([4] * 5, fail_at=fail_at)
    got = []
    with pytest.raises(OSError, match="batch %d is unreadable" % fail_at):
        for m in feed.Feeder(eng, gen, workers=0):
            got.append(m)
    assert eng.errors == [] and not eng.open
    assert eng.closed == (1 if fail_at else 0)          # the first batch fails before a feed is opened
    assert len(got) <= fail_at and set(eng.reads.values()) <= {1}


def test_feeder_takes_the_argmax_of_a_float64_soft_y_on_the_host():
    """two doubles that round to one float must still compare as doubles: only a float32 one-hot goes to the device"""
    eng = FakeEngine()
    y = np.zeros((2, 2, 2, 2, 5))
    y[..., 3] = 1.0
    y[..., 1] = 1.0 + 2.0 ** -40          # larger as a double, equal to 1.0 as a float

    class Gen:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return np.ones((2, 2, 2, 2, 4), np.float32), y

    list(feed.Feeder(eng, Gen(), workers=0))
    assert eng.errors == [] and eng.spec == ((4,), (np.dtype(np.float32),), "u8")
    assert np.all(eng.views[0]["labels"][:2] == 1)


def test_feeder_grows_the_engine_for_a_larger_batch_and_reuses_an_open_feed():
    engines = [FakeEngine(max_batch=2)]

    def grow(b):
        assert not engines[-1].open                      # the feed was closed before the engine is replaced
        engines.append(FakeEngine(max_batch=b))
        return engines[-1]

    gen = ListGen([2, 2, 4, 4, 3])
    f = feed.Feeder(engines[0], gen, workers=0, grow=grow)
    out = list(f)
    assert len(engines) == 2 and f.engine is engines[1] and all(e.errors == [] for e in engines)
    assert [int(m[1]) for m in out] == [2, 2, 4, 4, 3]
    for m, item in zip(out, gen.items):
        assert m[2] == np.float32(expected_total(item))
    assert [e.closed for e in engines] == [1, 1] and sorted(engines[0].reads) == [0, 1]
    # close=False leaves the feed open, and the next Feeder with the same layout goes on with it
    eng = FakeEngine()
    eng._feed = None
    opened = []
    real_open = eng.feed_open

    def feed_open(xc, xt, kind, slots):
        opened.append(kind)
        real_open(xc, xt, kind, slots)
        eng._feed = (tuple(xc), tuple(xt), kind, slots)
    eng.feed_open = feed_open
    a = list(feed.Feeder(eng, ListGen([4, 4, 4]), workers=0, close=False))
    assert eng.open and eng.closed == 0
    eng.log.clear(); eng.tickets.clear(); eng.reads.clear()
    b = list(feed.Feeder(eng, ListGen([4, 4]), workers=0, training=False, close=True))
    assert opened == ["onehot"] and eng.closed == 1 and eng.errors == [] and len(a) == 3 and len(b) == 2
