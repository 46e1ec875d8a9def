"""Rotation augmentation, host side (no GPU): the numpy statement of the rotating pack against the rotation convention
that tests/test_voxelise_host.py pins to the reference's output, the drawn tables and epoch plans, the generators'
augment option over an on-disk dataset, the Feeder handing each batch's table to the engine, and the script's refusal.
Everything is an equality: a quarter-turn is an index permutation."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_feed_host as FH  # noqa: E402
import test_voxelise_host as H  # noqa: E402

from icsg3d_amd import augment, feed  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8
TABLES = np.array([(a, b, c) for a in range(-1, 3) for b in range(-1, 3) for c in range(-1, 3)], np.int32)


def orientation(rot, d=3):
    """the orientation a table composes to, as the image of a grid whose voxels are all different"""
    return H.rotate(np.arange(d ** 3).reshape(d, d, d), rot).tobytes()


def access_class(rot):
    """(source axis that feeds the output's fastest axis, its sign): where a step along output axis 2 leads in the source"""
    d = 3
    src = H.rotate(np.arange(d ** 3).reshape(d, d, d), rot)
    delta = int(src[1, 1, 2]) - int(src[1, 1, 1])
    return {9: 0, 3: 1, 1: 2}[abs(delta)], delta > 0


# ------------------------------------------------------------------------------------------ 1. pack_reference
@pytest.mark.parametrize("kind", ["f64", "onehot"])
def test_pack_reference_rotates_like_the_voxeliser_convention(kind):
    rng = np.random.default_rng(2)
    B = len(TABLES)
    M, p = rng.random((B, D, D, D, 1)), rng.random((B, D, D, D, 3)) * 7.0
    if kind == "f64":
        lab = rng.integers(0, 95, (B, D, D, D)).astype(np.float64)
    else:
        lab = np.eye(5, dtype=np.float32)[rng.integers(0, 5, (B, D, D, D))]
    got_x, got_l = feed.pack_reference([M, p], lab, kind, rotations=TABLES)
    turn = lambda a: np.stack([H.rotate(s, r) for s, r in zip(a, TABLES)])
    want_x, want_l = feed.pack_reference([turn(M), turn(p)], turn(lab), kind)
    assert got_x.dtype == np.float32 and np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32))
    assert got_l.dtype == np.uint8 and np.array_equal(got_l, want_l)
    # channels travel with their voxel, values are untouched; no table is the plain pack
    assert np.array_equal(np.sort(got_x.reshape(B, -1, 4), axis=1), np.sort(want_x.reshape(B, -1, 4), axis=1))
    plain = feed.pack_reference([M, p], lab, kind)
    none = feed.pack_reference([M, p], lab, kind, rotations=np.full((B, 3), -1))
    assert np.array_equal(plain[0], none[0]) and np.array_equal(plain[1], none[1])
    assert not np.array_equal(plain[0], got_x)


def test_rotate_host_is_the_rot90_composition():
    rng = np.random.default_rng(4)
    X = rng.random((D, D, D, 3))
    for rot in TABLES:
        assert np.array_equal(augment.rotate_host(X, rot), H.rotate(X, rot))
        assert np.array_equal(augment.rotate_host(X[..., 0], rot), H.rotate(X[..., 0], rot))
    assert augment.ROTATION_AXES == H.AXES


# ------------------------------------------------------------------------------------------ 2. draw_rotations
def test_draw_rotations_distribution_and_reach():
    R = augment.draw_rotations(np.random.default_rng(5), 4000)
    assert R.shape == (4000, 3) and R.dtype == np.int32 and R.min() == 0 and R.max() == 2
    assert np.array_equal(R, augment.draw_rotations(np.random.default_rng(5), 4000))
    assert not np.array_equal(R, augment.draw_rotations(np.random.default_rng(6), 4000))
    assert len({tuple(r) for r in R}) == 27                                  # every table is drawn
    drawn = {orientation(r) for r in R}
    assert len(drawn) == 12 and orientation((-1, -1, -1)) not in drawn       # three positive turns: 12 of 24, never the identity
    assert len({orientation(r) for r in TABLES}) == 20
    assert {access_class(r) for r in TABLES} == {(a, s) for a in range(3) for s in (False, True)}


# ------------------------------------------------------------------------------------------ 3. epoch_plan
def test_epoch_plan_counts_epochs_and_reproducibility():
    state = np.random.get_state()
    idx, rot = augment.epoch_plan(7, 3, seed=28, epoch=0)
    assert idx.shape == (28,) and rot.shape == (28, 3) and rot.dtype == np.int32
    for i in range(7):
        mine = rot[idx == i]
        assert len(mine) == 4 and (mine == -1).all(axis=1).sum() == 1        # n_rot + 1 times, exactly once un-rotated
        assert ((mine >= 0).all(axis=1) | (mine == -1).all(axis=1)).all() and mine.max() <= 2
    assert not np.array_equal(idx, np.repeat(np.arange(7), 4))               # shuffled
    again = augment.epoch_plan(7, 3, seed=28, epoch=0)
    assert np.array_equal(idx, again[0]) and np.array_equal(rot, again[1])
    e1 = augment.epoch_plan(7, 3, seed=28, epoch=1)
    s2 = augment.epoch_plan(7, 3, seed=29, epoch=0)
    assert not (np.array_equal(idx, e1[0]) and np.array_equal(rot, e1[1]))
    assert not (np.array_equal(idx, s2[0]) and np.array_equal(rot, s2[1]))
    f0, f5 = augment.epoch_plan(7, 3, 28, 0, fixed=True), augment.epoch_plan(7, 3, 28, 5, fixed=True)
    assert np.array_equal(f0[0], f5[0]) and np.array_equal(f0[1], f5[1])
    i0, r0 = augment.epoch_plan(5, 0, 28, 0)                                 # n_rot = 0: every id once, as it is
    assert sorted(i0) == list(range(5)) and (r0 == -1).all()
    now = np.random.get_state()
    assert state[0] == now[0] and np.array_equal(state[1], now[1]) and state[2:] == now[2:]   # global stream untouched


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n_ids,n_rot,bs", [(7, 3, 2), (5, 2, 4), (11, 1, 3), (3, 0, 2), (2, 1, 5)])
def test_epoch_plan_rank_shares(world, n_ids, n_rot, bs):
    full_i, full_r = augment.epoch_plan(n_ids, n_rot, 28, 2)
    n = len(full_i) // (world * bs) * bs
    seen = []
    for rank in range(world):
        i, r = augment.epoch_plan(n_ids, n_rot, 28, 2, rank=rank, world=world, batch_size=bs)
        assert len(i) == len(r) == n and n % bs == 0                         # equal whole batches on every rank
        assert np.array_equal(i, full_i[rank::world][:n]) and np.array_equal(r, full_r[rank::world][:n])
        seen.extend(range(rank, len(full_i), world)[:n])
    assert len(set(seen)) == len(seen) == n * world                          # disjoint positions of the one common plan


# ------------------------------------------------------------------------------------------ 4. generators
def raw(root, sub, f, shape):
    return np.load(os.path.join(root, sub, f)).reshape(shape)


def test_generators_rotate_on_the_host_and_hand_raw_payloads_to_the_feed(tmp_path):
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.vae.data import VAEDataGenerator
    root = str(tmp_path)
    csv = FH.write_dataset(root)
    plan = dict(n_rot=2, seed=3)
    g = UnetDataGenerator(FH.IDS, root, batch_size=4, dim=(D, D, D), n_channels=4, shuffle=True, augment=plan)
    vg = VAEDataGenerator(FH.IDS, root, batch_size=3, dim=(D, D, D), n_channels=4, property_csv=csv, n_bins=3, augment=dict(plan))
    assert len(g) == 6 * 3 // 4 and len(vg) == 6
    state = np.random.get_state()
    for epoch in range(2):
        idx, rot = augment.epoch_plan(6, 2, 3, epoch, batch_size=4)
        assert np.array_equal(g.indexes, idx) and np.array_equal(g.rot, rot)
        for b in range(len(g)):
            X, (y, mask) = g[b]
            R = g.rotations(b)
            assert R.shape == (4, 3) and np.array_equal(R, rot[4 * b:4 * b + 4])
            for i in range(4):
                f = FH.IDS[idx[4 * b + i]]
                Mp = np.concatenate([raw(root, "density_matrices", f, (D, D, D, 1)), raw(root, "coordinate_grids", f, (D, D, D, 3))], -1)
                assert np.array_equal(X[i], augment.rotate_host(Mp, R[i]).astype(np.float32))
                assert np.array_equal(y[i], augment.rotate_host(raw(root, "species_matrices", f, (D, D, D)), R[i]).astype(np.uint8))
            assert np.array_equal(mask, (y != 0).astype(np.float32)[..., None])
            # the fed path: raw payloads + the table through the pack's numpy statement, bit for bit
            v = FH.views_for(g.feed_spec(), 5, D)
            assert g.fill(b, v) == 4
            f0 = FH.IDS[idx[4 * b]]
            assert np.array_equal(v["x"][1][0], raw(root, "coordinate_grids", f0, (D, D, D, 3)))     # un-rotated
            x, lab = feed.pack_reference([p[:4] for p in v["x"]], v["labels"][:4], g.feed_spec()[2], rotations=R)
            assert np.array_equal(x.view(np.uint32), X.view(np.uint32)) and np.array_equal(lab, y)
        g.on_epoch_end()
    for b in range(len(vg)):
        M, cond = vg[b]
        v = FH.views_for(vg.feed_spec(), 3, D, ncond=3)
        assert vg.fill(b, v) == 3
        x, _ = feed.pack_reference(v["x"], None, "none", rotations=vg.rotations(b))
        assert np.array_equal(x.view(np.uint32), M.view(np.uint32)) and np.array_equal(v["cond"], cond)
        assert np.array_equal(cond, np.stack([vg.property_to_categorical(FH.IDS[k]) for k in vg.indexes[3 * b:3 * b + 3]]))
    now = np.random.get_state()
    assert state[0] == now[0] and np.array_equal(state[1], now[1])           # the plans never draw from np.random
    # validation: a fixed plan repeats; without augment nothing is offered and nothing changes
    fx = UnetDataGenerator(FH.IDS, root, batch_size=4, dim=(D, D, D), n_channels=4, augment=dict(n_rot=2, seed=3, fixed=True))
    first = (fx.indexes.copy(), fx.rot.copy())
    fx.on_epoch_end()
    assert np.array_equal(first[0], fx.indexes) and np.array_equal(first[1], fx.rot)
    plain = UnetDataGenerator(FH.IDS, root, batch_size=4, dim=(D, D, D), n_channels=4)
    assert plain.rotations(0) is None and len(plain) == 1 and np.array_equal(plain.indexes, np.arange(6))


def test_an_epoch_plan_over_base_files_equals_a_plain_generator_over_rotated_files(tmp_path):
    from icsg3d_amd.unet.data import UnetDataGenerator
    root = str(tmp_path)
    FH.write_dataset(root)
    g = UnetDataGenerator(FH.IDS, root, batch_size=3, dim=(D, D, D), n_channels=4, augment=dict(n_rot=2, seed=9))
    names = []
    for n, (k, rot) in enumerate(zip(g.indexes, g.rot)):                     # the plan, written out as create_matrices would
        base = FH.IDS[k]
        if (rot == -1).all():
            names.append(base)
            continue
        name = "%s_rot_%d.npy" % (base[:-4], n)
        for sub, shape in (("density_matrices", (D, D, D)), ("coordinate_grids", (D, D, D, 3)), ("species_matrices", (D, D, D))):
            X = raw(root, sub, base, shape)
            for r in rot:
                X = np.rot90(X, 1, axes=H.AXES[r])
            np.save(os.path.join(root, sub, name), X)
        names.append(name)
    plain = UnetDataGenerator(names, root, batch_size=3, dim=(D, D, D), n_channels=4)
    assert len(plain) == len(g) == 6
    for b in range(len(g)):
        (X, (y, m)), (Xp, (yp, mp)) = g[b], plain[b]
        assert np.array_equal(X.view(np.uint32), Xp.view(np.uint32)) and np.array_equal(y, yp) and np.array_equal(m, mp)


# ------------------------------------------------------------------------------------------ 5. Feeder
class RotEngine(FH.FakeEngine):
    def feed_submit(self, slot, batch, rotations=None):
        super().feed_submit(slot, batch)
        self.tables = getattr(self, "tables", []) + [None if rotations is None else np.array(rotations)]


def test_feeder_hands_every_batch_its_table(tmp_path):
    from icsg3d_amd.unet.data import UnetDataGenerator
    root = str(tmp_path)
    FH.write_dataset(root)
    g = UnetDataGenerator(FH.IDS, root, batch_size=2, dim=(D, D, D), n_channels=4, augment=dict(n_rot=1, seed=1))
    eng = RotEngine(max_batch=2, d=D)
    eng.num_classes = 95
    out = list(feed.Feeder(eng, g, workers=2))
    assert len(out) == len(g) == 6 and not eng.errors
    assert len(eng.tables) == 6
    for k, t in enumerate(eng.tables):                                       # submits are in step order
        assert t.shape == (2, 3) and np.array_equal(t, g.rotations(k))
    assert [e[0] for e in eng.log if e[0] == "submit"] == ["submit"] * 6
    # a file generator without augment, and a generator without `rotations` at all: plain submits
    for gen in (UnetDataGenerator(FH.IDS, root, batch_size=2, dim=(D, D, D), n_channels=4), FH.ListGen([2, 1, 2])):
        e2 = RotEngine(max_batch=2, d=D if hasattr(gen, "fill") else 2)
        if hasattr(gen, "fill"):
            e2.num_classes = 95
        assert len(list(feed.Feeder(e2, gen, workers=0))) == 3 and not e2.errors
        assert e2.tables == [None, None, None]


# ------------------------------------------------------------------------------------------ 6. the script
def test_train_unet_refuses_augment_with_synthetic(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_unet.py"), "--name", "toy", "--augment", "--synthetic", "8"],
                       capture_output=True, text=True, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode != 0
    assert "--augment" in r.stderr and "--synthetic" in r.stderr and "cannot be combined" in r.stderr
    assert not os.listdir(str(tmp_path))                                     # refused before anything was created
