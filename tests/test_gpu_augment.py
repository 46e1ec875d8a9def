"""Rotation augmentation on the GPU (include/icsg3d.h ics_op_feed_pack_rot / ics_net_feed_submit_rot, csrc/feed.hip): the
rotating pack kernel against its numpy statement over every rotation table, tile size and layout, against the
voxeliser's own rotations, fed steps through a table against synchronous steps on host-rotated arrays, the class-level
loops with augmented generators fed and unfed, and the refusals.  A quarter-turn is an index permutation: everything is
compared bit for bit."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_feed as GF  # noqa: E402
import test_gpu_voxelise as GV  # noqa: E402

from icsg3d_amd.augment import rotate_host  # noqa: E402

same_bits, bits = GF.same_bits, GF.bits
TABLES = np.array([(a, b, c) for a in range(-1, 3) for b in range(-1, 3) for c in range(-1, 3)], np.int32)


def orientation(rot):
    return rotate_host(np.arange(27).reshape(3, 3, 3), rot).tobytes()


def access_class(rot):
    """(source axis that feeds the output's fastest axis, forward?)"""
    src = rotate_host(np.arange(27).reshape(3, 3, 3), rot)
    delta = int(src[1, 1, 2]) - int(src[1, 1, 1])
    return {9: 0, 3: 1, 1: 2}[abs(delta)], delta > 0


def distinct_orientations():
    """one table for each of the 20 orientations the 64 tables reach"""
    seen = {}
    for r in TABLES:
        seen.setdefault(orientation(r), r)
    return np.array(list(seen.values()), np.int32)


def one_per_class():
    seen = {}
    for r in TABLES[::-1]:                     # from the far end: three real turns where they reach the class
        seen.setdefault(access_class(r), r)
    assert len(seen) == 6
    return np.array(list(seen.values()), np.int32)


def x_parts(rng, B, d, channels, mix):
    parts = []
    for c, t in zip(channels, mix):
        a = ((rng.random((B, d, d, d, c)) - 0.5) * 10.0 ** rng.integers(-3, 4, (B, d, d, d, c))).astype(t)
        p = GF.cast_probes(t)
        for b in range(0, B, 7):               # the probes in several samples: a rotation moves them to other places
            a[b].reshape(-1)[:len(p)] = p
            a[b].reshape(-1)[-len(p):] = p[::-1]
        parts.append(a)
    return parts


def check(parts, lab, kind, ncls, R):
    from icsg3d_amd.engine import feed_pack
    from icsg3d_amd.feed import pack_reference
    with np.errstate(over="ignore"):
        want_x, want_l = pack_reference(parts, lab, kind, rotations=R)
    got_x, got_l = feed_pack(parts, lab, kind, ncls, rotations=R)
    bad = np.flatnonzero((bits(got_x) != bits(want_x)).reshape(len(R), -1).any(axis=1))
    assert same_bits(got_x, want_x), (kind, "samples", bad[:8], [tuple(R[b]) for b in bad[:4]])
    if kind == "none":
        assert got_l is None
    else:
        bad = np.flatnonzero((got_l != want_l).reshape(len(R), -1).any(axis=1))
        assert same_bits(got_l, want_l), (kind, ncls, "samples", bad[:8], [tuple(R[b]) for b in bad[:4]])


# ------------------------------------------------------------------------------------------ 1. small tiles, every table
@pytest.mark.parametrize("mix", [(np.float64, np.float64), (np.float32, np.float64), (np.float32, np.float32)],
                         ids=["f64f64", "f32f64", "f32f32"])
@pytest.mark.parametrize("channels", [1, 4])
def test_rotating_pack_all_tables_in_one_launch(channels, mix):
    d, B = 8, 64
    rng = np.random.default_rng(channels * 10 + len(str(mix)))
    R = TABLES[rng.permutation(B)]             # mixed orientations next to each other
    parts = x_parts(rng, B, d, (1,) if channels == 1 else (1, 3), mix)
    for kind, ncls in [("u8", 0), ("f64", 0), ("f32", 0), ("onehot", 2), ("onehot", 95), ("none", 0)]:
        if kind == "onehot":
            lab = GF.one_hot_cases(rng, B, d, ncls)
        elif kind == "none":
            lab = None
        else:
            lab = rng.integers(0, 256, (B, d, d, d)).astype({"u8": np.uint8, "f64": np.float64, "f32": np.float32}[kind])
            lab.reshape(-1)[:4] = [0, 255, 94, 1]
        check(parts, lab, kind, ncls, R)
    # a batch of one
    lab = rng.integers(0, 95, (1, d, d, d)).astype(np.float64)
    for r in ((0, 1, 2), (1, -1, -1), (-1, -1, -1)):
        check([p[:1] for p in parts], lab, "f64", 0, np.array([r], np.int32))


# ------------------------------------------------------------------------------------------ 2. several tiles per plane
@pytest.mark.parametrize("d,tables", [(32, "orientations"), (64, "classes")])
def test_rotating_pack_several_tiles_per_plane(d, tables):
    R = distinct_orientations() if tables == "orientations" else one_per_class()
    assert len(R) == (20 if tables == "orientations" else 6)
    rng = np.random.default_rng(d)
    B = len(R)
    parts = [rng.random((B, d, d, d, 1)), rng.random((B, d, d, d, 3)) * 9.0]
    lab = rng.integers(0, 95, (B, d, d, d)).astype(np.float64)
    check(parts, lab, "f64", 0, R)


# ------------------------------------------------------------------------------------------ 3. the gather paths
def test_rotating_pack_gather_paths():
    rng = np.random.default_rng(8)
    R = one_per_class()
    d, B = 8, len(R)
    lab = rng.integers(0, 95, (B, d, d, d)).astype(np.float64)
    check([rng.standard_normal((B, d, d, d, 2)), rng.standard_normal((B, d, d, d, 3)).astype(np.float32)], lab, "f64", 0, R)
    check([rng.standard_normal((B, d, d, d, 4))], lab, "f64", 0, R)
    check([rng.standard_normal((B, d, d, d, 4))], lab.astype(np.uint8), "u8", 0, R)


# ------------------------------------------------------------------------------------------ 4. create_matrices.py's convention
def test_the_feed_rotates_like_the_voxeliser():
    from icsg3d_amd.engine import feed_pack
    from icsg3d_amd.feed import pack_reference
    from icsg3d_amd.matrices import voxelise
    rng = np.random.default_rng(12)
    s = GV._structs(rng, 6, 8)
    R = np.array([(0, 1, 2), (2, 2, 1), (1, -1, 0), (-1, 2, -1), (1, 1, 1), (0, 0, 2)], np.int32)
    M0, S0, p0 = voxelise(s, d=16)
    M1, S1, p1 = voxelise(s, rotations=R, d=16)
    assert S0.max() < 256 and not np.array_equal(M0, M1)
    got_x, got_l = feed_pack([M0[..., None], p0], S0, "f64", rotations=R)
    want_x, want_l = pack_reference([M1[..., None], p1], S1, "f64")
    assert same_bits(got_x, want_x) and same_bits(got_l, want_l)


# ------------------------------------------------------------------------------------------ 5. fed steps through a table
def rotated_items(C, seed):
    items = GF.raw_batches(C, seed)[:5]
    assert [(it["kind"], it["B"]) for it in items] == [("train", 3), ("train", 5), ("train", 2), ("test", 4), ("train", 5)]
    rng = np.random.default_rng(seed)
    for it in items:
        it["rot"] = TABLES[rng.integers(0, 64, it["B"])]
    return items


def host_arrays(it, rot):
    from icsg3d_amd.feed import pack_reference
    return pack_reference(it["parts"], it["ids"], "f64", rotations=rot)


def fed_step(eng, slot, it, rot, how):
    """fill + submit + step + metrics; how: "table" (rot), "plain" (no table), "none" (a table of -1)"""
    GF.fill(eng.feed_slot(slot), it, "files")
    if how == "plain":
        eng.feed_submit(slot, it["B"])
    else:
        eng.feed_submit(slot, it["B"], rot if how == "table" else np.full((it["B"], 3), -1, np.int32))
    t = (eng.train_step_fed if it["kind"] == "train" else eng.test_step_fed)(slot)
    return eng.feed_metrics(t).copy()


@pytest.mark.parametrize("vae", [False, True], ids=["unet", "vae"])
def test_fed_steps_through_a_table_equal_synchronous_steps_on_rotated_arrays(vae):
    items = rotated_items(4, 500 + vae)
    # the schedule: every item through its table, then item 0 plainly on the slot that carried a table, then item 1
    # through a table of -1
    plan = [(k % 2, it, "table") for k, it in enumerate(items)] + [(0, items[0], "plain"), (1, items[1], "none")]
    if vae:
        ru, fu = GF.unet_engine(4), GF.unet_engine(4)
        ref, fed = GF.vae_engine(ru, 4), GF.vae_engine(fu, 4)
        fed.feed_open((1, 3), (np.float64, np.float64), "none", 2)
    else:
        ref, fed = GF.unet_engine(), GF.unet_engine()
        fed.feed_open((1, 3), (np.float64, np.float64), "f64", 2)
    for n, (slot, it, how) in enumerate(plan):
        x, lab = host_arrays(it, it["rot"] if how == "table" else None)
        step = ref.train_step if it["kind"] == "train" else ref.test_step
        want = step(x, it["cond"], it["eps"]) if vae else step(x, lab)
        got = fed_step(fed, slot, it, it["rot"], how)
        assert got.shape == ((4,) if vae else (5,)) and same_bits(got, want), (n, how, it["kind"], got, want)
        if how == "table" and it["kind"] == "train" and n == 0:       # the table mattered: the plain arrays step differently
            px, pl = host_arrays(it, None)
            assert not same_bits(px, x)
    fed.feed_close()
    GF.assert_same_state(GF.state(fed), GF.state(ref))


# ------------------------------------------------------------------------------------------ 6. class level
def test_fit_generator_augmented_fed_equals_unfed(tmp_path):
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    D = GF.D
    ids, _ = GF.write_dataset(str(tmp_path))
    kw = dict(data_path=str(tmp_path), dim=(D, D, D), n_channels=4)
    runs = []
    for feed in (False, True):
        np.random.seed(4)
        unet = AtomUnet(input_shape=(D, D, D, 4), lr=1e-4, max_batch=3)
        tg = UnetDataGenerator(ids[:6], batch_size=3, augment=dict(n_rot=2, seed=5), **kw)
        vg = UnetDataGenerator(ids[6:], batch_size=2, augment=dict(n_rot=2, seed=5, fixed=True), **kw)
        assert len(tg) == 6 and len(vg) == 3
        hist = unet.model.fit_generator(tg, validation_data=vg, epochs=2, verbose=0, feed=feed)
        assert tg.augment.epoch == 2 and vg.augment.epoch == 2
        runs.append((hist, unet._get_weights(), unet._eng.get_optimizer_state()))
    (h0, w0, o0), (h1, w1, o1) = runs
    assert len(h0) == len(h1) == 2
    for a, b in zip(h0, h1):
        assert sorted(a) == sorted(b) and len(a) == 10
        for k in a:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])
    for k in w0:
        assert same_bits(w0[k], w1[k]), k
    assert o0[2] == o1[2] == 12 and same_bits(o0[0], o1[0]) and same_bits(o0[1], o1[1])


def test_vae_train_augmented_fed_equals_unfed(tmp_path, C=4):
    from icsg3d_amd.synthetic import glorot_params, unet_param_shapes
    from icsg3d_amd.vae.data import VAEDataGenerator
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    D = GF.D
    ids, csv = GF.write_dataset(str(tmp_path / "data"))
    kw = dict(data_path=str(tmp_path / "data"), dim=(D, D, D), n_channels=C, property_csv=csv, n_bins=3)
    pm = glorot_params(unet_param_shapes(C, 95), 1)
    runs = []
    for feed in (False, True):
        np.random.seed(6)
        out = tmp_path / ("fed" if feed else "unfed")
        os.makedirs(out)
        vae = LatticeDFCVAE(input_shape=(D, D, D, C), perceptual_model=pm, cond_shape=3, output_dir=str(out))
        tg = VAEDataGenerator(ids[:6], batch_size=3, augment=dict(n_rot=2, seed=7), **kw)
        vg = VAEDataGenerator(ids[6:], batch_size=2, augment=dict(n_rot=2, seed=7, fixed=True), **kw)
        vae.train(tg, vg, epochs=2, weights=str(out / "vae.best.hdf5"), feed=feed)
        assert tg.augment.epoch == 2
        runs.append((np.array(vae.losses), vae._get_weights()))
    (l0, w0), (l1, w1) = runs
    assert l0.shape == (2, 2) and l0.tobytes() == l1.tobytes(), (l0, l1)
    for k in w0:
        assert same_bits(w0[k], w1[k]), k


# ------------------------------------------------------------------------------------------ 7. refusals
def test_a_rotation_index_outside_the_table_is_refused():
    from icsg3d_amd import _lib as L
    from icsg3d_amd.engine import feed_pack
    rng = np.random.default_rng(1)
    parts = [rng.random((3, 8, 8, 8, 1)), rng.random((3, 8, 8, 8, 3))]
    lab = rng.integers(0, 95, (3, 8, 8, 8)).astype(np.float64)
    for bad, where in ((3, (2, 1)), (-2, (0, 2))):
        R = np.array([(0, 1, 2), (-1, -1, -1), (2, 2, 2)], np.int32)
        R[where] = bad
        with pytest.raises(L.IcsError, match=r"sample %d: rotation index %d not in" % (where[0], bad)):
            feed_pack(parts, lab, "f64", rotations=R)
    ue = GF.unet_engine()
    ue.feed_open((1, 3), (np.float64, np.float64), "f64", 2)
    it = GF.raw_batches(4, 300)[0]
    GF.fill(ue.feed_slot(0), it, "files")
    for bad in (3, -2):
        R = np.zeros((it["B"], 3), np.int32)
        R[1, 0] = bad
        with pytest.raises(L.IcsError, match=r"ics_net_feed_submit_rot: sample 1: rotation index %d not in" % bad):
            ue.feed_submit(0, it["B"], R)
    with pytest.raises(ValueError, match="rotation table"):
        ue.feed_submit(0, it["B"], np.zeros((it["B"] + 1, 3), np.int32))
    # the refused submits left the slot as it was: it still takes a table, and the step is the rotated one
    R = TABLES[[7, 30, 63]]
    ue.feed_submit(0, it["B"], R)
    got = ue.feed_metrics(ue.train_step_fed(0)).copy()
    ue.feed_close()
    from icsg3d_amd.feed import pack_reference
    x, l8 = pack_reference(it["parts"], it["ids"], "f64", rotations=R)
    assert same_bits(got, GF.unet_engine().train_step(x, l8))
