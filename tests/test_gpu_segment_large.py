"""The watershed tail at d = 128 and 256 (csrc/segment.hip through the C ABI) against oracle/watershed_ref.py, exact integer
comparisons as in tests/test_gpu_segment.py: the device components and statistics at 128^3 and 256^3 (the int32 coordinate
sums of a grid-filling component sit just under 2^31), refine_atoms / watershed_clustering / segment_nuclei_batch on whole
128^3 volumes whose components and split boxes are wider than 64, the box operations on mixed batches of boxes up to 256
per axis (host labeller and host flood next to the kernels), and the fused tail at d = 128."""
import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial import QhullError

from oracle import watershed_ref as W

pytestmark = pytest.mark.gpu


def _balls(d, specs):
    zz, yy, xx = np.mgrid[:d, :d, :d]
    m = np.zeros((d, d, d), bool)
    for (c, r) in specs:
        m |= (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r
    return m.astype(np.int32)


# d = 128 shapes (designed on the oracle): a chain of six touching balls 80 voxels long along x -- its split box is wider
# than 64 and it recurses down to max_iters -- and a pair that recurses four times
CHAIN = [((30, 40, 20 + 13 * k), 7) for k in range(6)]
PAIR = [((80, 70, 50), 10), ((80, 70, 68), 10)]


def _chain14_box():
    """six balls that only touch (centres 14 apart, radius 7), cropped to their bounding box: 15 x 15 x 85, and the first
    split already separates all six"""
    v = _balls(128, [((30, 40, 16 + 14 * k), 7) for k in range(6)])
    return v[ndimage.find_objects(v)[0]]


def _region_table(R, n):
    """voxels, coordinate sums (z, y, x) and half-open bounding boxes of labels 1..n of R, vectorised."""
    d2, d1 = R.shape[1] * R.shape[2], R.shape[2]
    flat = R.ravel()
    idx = np.arange(flat.size, dtype=np.int64)
    vox = np.bincount(flat, minlength=n + 1)[1:n + 1]
    sums = np.stack([np.bincount(flat, weights=c, minlength=n + 1)[1:n + 1] for c in (idx // d2, (idx // d1) % R.shape[1], idx % d1)], 1)
    box = np.array([[s.start for s in sl] + [s.stop for s in sl] for sl in ndimage.find_objects(R, max_label=n)], np.int64)
    return vox, sums.astype(np.int64), box.reshape(n, 6)


@pytest.mark.parametrize("B,d", [(3, 128), (2, 256)])
def test_segment_atoms_matches_oracle_at_128_and_256(B, d):
    from icsg3d_amd.watershed import dop_count, segment_atoms
    rng = np.random.default_rng(300 + d)
    masks = np.zeros((B, d, d, d), np.uint8)
    if d == 128:
        max_atoms = 20000
        masks[0, :64] = rng.uniform(size=(64, d, d)) < 0.3
        masks[1] = _balls(d, CHAIN + PAIR)
        masks[1, 100:, :, :] = 1                            # a slab on three faces of the grid: one wide component
        masks[2] = rng.uniform(size=(d, d, d)) < 0.2       # ~28 k kept components: more than max_atoms
        failing = 2
    else:
        max_atoms = 1 << 16
        masks[0] = 1                                        # one component filling the grid: sum z = 2,139,095,040
        masks[1, :32] = rng.uniform(size=(32, d, d)) < 0.27
        masks[1, 100:140, 100:140, :] = 1
        failing = None
    species = rng.integers(0, 95, size=masks.shape).astype(np.uint8)
    r = segment_atoms(masks, species, min_voxels=3, max_atoms=max_atoms)
    assert [bool(f) for f in r["failed"]] == [b == failing for b in range(B)]
    for b in range(B):
        R, ncomp, nkept = W.regions(masks[b])
        assert np.array_equal(r["regions"][b], R), b
        assert int(r["n_components"][b]) == ncomp, b
        if b == failing:                                    # the sample fails alone; the call does not
            assert nkept > max_atoms and int(r["n_atoms"][b]) == 0 and r["atoms"][b] == ([], [])
            continue
        assert int(r["n_atoms"][b]) == nkept and 0 < nkept <= max_atoms, b
        st = r["stats"][b, :nkept].astype(np.int64)
        vox, sums, box = _region_table(R, nkept)
        assert np.array_equal(st[:, 1], vox) and np.array_equal(st[:, 2:5], sums), b
        assert np.array_equal(st[:, 5:11], box), b
        assert (r["stats"][b, nkept:, 1] == 0).all()
        big = int(np.argmax(vox))
        sample = sorted(set(list(range(min(nkept, 4))) + [nkept - 1, big] + list(rng.integers(0, nkept, size=4))))
        for a in sample:                                    # majority votes
            sl = tuple(slice(int(box[a, i]), int(box[a, i + 3])) for i in range(3))
            inside = R[sl] == a + 1
            assert int(st[a, 0]) == W.majority_vote(species[b][sl].astype(np.int64), inside.astype(np.int32), 1), (b, a)
        for a in sample:                                    # convexity bounds: polytope count and second moments
            sl = tuple(slice(int(box[a, i]), int(box[a, i + 3])) for i in range(3))
            inside = R[sl] == a + 1
            bd = r["bounds"][b, a]
            pts = np.argwhere(inside) + box[a, :3]
            if inside.all():                                # a solid box: every grid point of it is in the polytope
                assert int(bd[0]) == inside.size, (b, a)
                # second moments of a full box by formula (the grid-filling component: sums up to 3.6e11)
                ax = [np.arange(int(box[a, i]), int(box[a, i + 3]), dtype=np.int64) for i in range(3)]
                cnt = [len(v) for v in ax]
                s1 = [int(v.sum()) for v in ax]
                s2 = [int((v * v).sum()) for v in ax]
                mom = [s2[0] * cnt[1] * cnt[2], s2[1] * cnt[0] * cnt[2], s2[2] * cnt[0] * cnt[1],
                       s1[0] * s1[1] * cnt[2], s1[0] * s1[2] * cnt[1], s1[1] * s1[2] * cnt[0]]
            else:
                if inside.size <= 80 ** 3:
                    assert int(bd[0]) == dop_count(inside), (b, a)
                mom = [int((pts[:, i] * pts[:, j]).sum()) for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
            assert [int(v) for v in bd[1:7]] == mom, (b, a)
        if d == 256 and b == 0:                             # the int32 coordinate-sum edge
            assert nkept == 1 and list(st[0, 1:5]) == [d ** 3] + [d ** 3 * (d - 1) // 2] * 3 == [16777216] + [2139095040] * 3
            assert list(st[0, 5:11]) == [0, 0, 0, d, d, d]


def _masks_128():
    d = 128
    chain = _balls(d, CHAIN)
    plate = _balls(d, [((40, 40, 40), 5)])
    plate[100, 60:62, 60:62] = 1                            # a 2 x 2 plate: 4 coplanar voxels, kept by the size filter
    quirk = chain.copy()
    quirk[0, 0, 0:2] = 1                                    # a first component of <= 3 voxels takes label 1
    rnd = np.zeros((d, d, d), np.int32)
    rnd[:, :, :12] = np.random.default_rng(9).uniform(size=(d, d, 12)) < 0.2       # ragged: flat and non-convex components
    return np.stack([chain, _balls(d, PAIR), plate, quirk, np.zeros((d, d, d), np.int32), rnd]).astype(np.uint8)


def test_refine_atoms_and_clustering_match_oracle_at_128():
    """refine_atoms on whole 128^3 samples (component_bounds over the whole region volume, label_boxes over the whole mask,
    split boxes wider than 64) against W.watershed_clustering, in both degenerate modes: regions, atoms and means equal,
    a flat component failing its sample only."""
    from icsg3d_amd.watershed import refine_atoms, segment_atoms, watershed_clustering
    masks = _masks_128()
    rng = np.random.default_rng(5)
    species = np.where(masks != 0, rng.integers(1, 95, size=masks.shape), 0).astype(np.uint8)
    refs = {}
    for mode in ("raise", "solid"):
        out = refine_atoms(segment_atoms(masks, species, max_atoms=4096), degenerate=mode)
        assert list(out["split"][:2]) == [True, True] and out["split"][3] and not out["split"][4]
        assert list(out["failed"]) == [False, False, mode == "raise", False, False, mode == "raise"], (mode, list(out["failed"]))
        for b in range(len(masks)):
            key = (b, mode if b in (2, 5) else "any")
            if key not in refs:
                try:
                    a_ref, mu_ref, R_ref = W.watershed_clustering(None, species[b], masks[b].astype(np.int32), degenerate=mode)
                    refs[key] = (list(a_ref), np.array(mu_ref).reshape(len(a_ref), 3), R_ref.astype(np.int32))
                except QhullError:
                    refs[key] = None
            if refs[key] is None:
                assert out["failed"][b] and out["atoms"][b] == ([], []), (mode, b)
                continue
            a_ref, mu_ref, R_ref = refs[key]
            a, mu = out["atoms"][b]
            assert np.array_equal(out["regions"][b], R_ref), (mode, b)
            assert list(a) == a_ref and np.array_equal(np.array(mu).reshape(len(a), 3), mu_ref), (mode, b)
    assert len(refs[(4, "any")][0]) == 0 and len(refs[(5, "solid")][0]) > 1000
    # the reference-shaped single-sample entry point on the chain
    a, mu, R = watershed_clustering(None, species[0], masks[0], return_ws=True)
    a_ref, mu_ref, R_ref = refs[(0, "any")]
    assert np.array_equal(R.astype(np.int32), R_ref) and list(a) == a_ref


def test_breadth_first_batch_equals_the_depth_first_recursion_at_128():
    """segment_nuclei_batch against _segment_nuclei_recursive on 128^3 volumes: identical R, traces and failures; the
    chain and the pair recurse (depth >= 3), the chain's first-level split box is wider than 64."""
    from icsg3d_amd.watershed import DegenerateComponent, _segment_nuclei_recursive, segment_nuclei_batch
    masks = _masks_128()
    vols = [masks[b].astype(np.int32) for b in (0, 1, 3, 5, 2)]
    counts = {"convex": 0, "split": 0, "recurse": 0}
    for mode in ("solid", "raise"):
        traces = [[] for _ in vols]
        Rs, errors = segment_nuclei_batch(vols, traces=traces, degenerate=mode)
        for i, v in enumerate(vols):
            tr = []
            try:
                R_ref = _segment_nuclei_recursive(v, trace=tr, degenerate=mode)
            except DegenerateComponent:
                assert errors[i] is not None and Rs[i] is None, (mode, i)
                continue
            assert errors[i] is None and np.array_equal(Rs[i], R_ref), (mode, i)
            assert [(t[0], t[1], t[2], t[4]) for t in traces[i]] == [(t[0], t[1], t[2], t[4]) for t in tr], (mode, i)
            if mode == "solid":
                for t in traces[i]:
                    counts[t[4]] += 1
        if mode == "solid":
            assert max(t[0] for t in traces[0]) >= 3 and max(t[0] for t in traces[1]) >= 3
            assert traces[0][0][4] == "recurse" and traces[0][0][2] == int(vols[0].sum())
            assert counts["split"] > 100
        else:
            assert errors[3] is not None and errors[4] is not None and errors[0] is None
    # the exact-hull branch of component_bounds on these whole volumes: every component the integer bounds leave open gets
    # its exact count H (a declined search -- H = 0 -- would hand it to Qhull)
    from icsg3d_amd.watershed import label_boxes
    exact = declined = 0
    for lab, n, st, bnd in label_boxes(vols, connectivity=1, want_bounds=True, hull_threshold=0.8):
        rows = bnd[st[:, 0] > 3]
        open_ = rows[:, 0] / rows[:, 1] < 0.8
        open_ &= 0.8 <= rows[:, 0] / rows[:, 2]
        exact += int((rows[open_, 4] > 0).sum())
        declined += int((rows[open_, 4] == 0).sum())
        assert ((rows[open_, 4] >= rows[open_, 2]) & (rows[open_, 4] <= rows[open_, 1])).all()
    print("d=128 segment_nuclei_batch (solid): %d convex, %d split, %d recurse; first level: %d exact hull counts, "
          "%d declined" % (counts["convex"], counts["split"], counts["recurse"], exact, declined))
    assert exact > 0 and declined == 0


def _mixed_label_vols(rng):
    return [rng.integers(0, 4, size=(7, 9, 6)).astype(np.int32),
            (rng.uniform(size=(200, 30, 20)) < 0.35).astype(np.int32) * rng.integers(1, 3, size=(200, 30, 20)).astype(np.int32),
            np.zeros((3, 3, 3), np.int32),
            (rng.uniform(size=(6, 256, 8)) < 0.5).astype(np.int32) * 4,
            (rng.uniform(size=(40, 40, 40)) < 0.3).astype(np.int32),
            (rng.uniform(size=(65, 64, 64)) < 0.3).astype(np.int32) * 5,
            rng.integers(0, 3, size=(1, 1, 17)).astype(np.int32),
            _chain14_box() * 2]


@pytest.mark.parametrize("conn", [1, 3])
def test_label_boxes_on_mixed_batches_with_boxes_up_to_256(conn, monkeypatch):
    """label_boxes with small (kernel) and large (host labeller) boxes interleaved in one call: every box equal to
    W.label_equal, so the outputs land in their boxes' places; and the host labeller forced on every box
    (ICSG3D_LABEL_HOST=1) bit-identical to the kernel on boxes <= 64."""
    from icsg3d_amd.watershed import label_boxes
    rng = np.random.default_rng(80 + conn)
    vols = _mixed_label_vols(rng)
    monkeypatch.setenv("ICSG3D_LABEL_HOST", "0")
    res = label_boxes(vols, connectivity=conn, max_labels=64)
    for v, (lab, n, st) in zip(vols, res):
        ref, nref = W.label_equal(v, connectivity=conn)
        assert n == nref and np.array_equal(lab, ref), v.shape
        if n:
            vox, _, box = _region_table(ref, n)
            assert np.array_equal(st[:, 0], vox) and np.array_equal(st[:, 1:7], box), v.shape
    small = [v for v in vols if max(v.shape) <= 64] + [(rng.uniform(size=(64, 20, 33)) < 0.45).astype(np.int32),
                                                       (rng.uniform(size=(32, 32, 32)) < 0.3).astype(np.int32) * 5]
    dev = label_boxes(small, connectivity=conn, max_labels=64)
    monkeypatch.setenv("ICSG3D_LABEL_HOST", "1")
    host = label_boxes(small, connectivity=conn, max_labels=64)
    for (l1, n1, s1), (l2, n2, s2) in zip(dev, host):
        assert n1 == n2 and np.array_equal(l1, l2) and np.array_equal(s1, s2)


@pytest.mark.parametrize("tie", ["heap", "fifo"])
def test_watershed_split_on_mixed_batches_with_boxes_up_to_256(tie, monkeypatch):
    """watershed_split with boxes wider than 64 between small ones, host form and ICSG3D_WS_DEVICE=1 (the large boxes take
    the host flood there instead of being refused): every box equal to W.split_component."""
    from icsg3d_amd.watershed import watershed_split
    rng = np.random.default_rng(90)
    chain = _chain14_box()
    two = _balls(16, [((6, 6, 4), 4), ((6, 6, 10), 4)])[2:11, 2:11, :15]
    boxes = [two, chain, two * 5, (rng.uniform(size=(70, 12, 10)) < 0.8).astype(np.int32),
             (rng.uniform(size=(9, 8, 11)) < 0.75).astype(np.int32), (rng.uniform(size=(256, 6, 6)) < 0.85).astype(np.int32),
             chain * 3]
    cls = [1, 1, 5, 1, 1, 1, 3]
    refs = [W.split_component(b, c, tie=tie) for b, c in zip(boxes, cls)]
    assert chain.shape == (15, 15, 85) and len(np.unique(refs[1])) == 7          # the chain splits into its six balls
    for where in ("0", "1"):
        monkeypatch.setenv("ICSG3D_WS_DEVICE", where)
        got = watershed_split(boxes, cls, tie=tie)
        for b, ref, g in zip(boxes, refs, got):
            assert np.array_equal(g, ref), (where, b.shape)


def test_fused_tail_at_128_then_refine_matches_oracle():
    """decode_to_atoms (ics_vae_decode_to_unet_atoms) at d = 128 on Glorot weights, B = 2, continued by refine_atoms:
    regions equal W.watershed_clustering on the engine's own mask and species (degenerate="solid"); nothing raises."""
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    from icsg3d_amd.synthetic import glorot_params, unet_param_shapes, vae_param_shapes
    from icsg3d_amd.watershed import refine_atoms
    B, d, C = 2, 128, 4
    ue = UnetEngine(in_channels=C, d=d, max_batch=B)
    ue.set_weights(glorot_params(unet_param_shapes(C, 95), 1))
    ve = VaeEngine(ue, in_channels=C, d=d, max_batch=B)
    ve.set_weights(glorot_params(vae_param_shapes(C, d=d), 3))
    rng = np.random.default_rng(0)
    z = rng.standard_normal((B, 256)).astype(np.float32)
    cond = np.eye(10, dtype=np.float32)[[2, 6]]
    dens = ve.decode_to_labels(ue, z, cond, thresh=0.5)["density"]
    thr = float(np.quantile(dens, 0.97))                          # random weights: a data-dependent threshold
    out = ve.decode_to_atoms(ue, z, cond, thresh=thr, max_atoms=1 << 15, want_regions=True)
    assert out["mask"].sum() > 0 and not out["failed"].any()
    refine_atoms(out, degenerate="solid")
    assert not out["failed"].any()
    for b in range(B):
        a_ref, mu_ref, R_ref = W.watershed_clustering(None, out["species"][b], out["mask"][b].astype(np.int32), degenerate="solid")
        a, mu = out["atoms"][b]
        assert np.array_equal(out["regions"][b], R_ref.astype(np.int32)), b
        assert list(a) == list(a_ref), b
        assert np.array_equal(np.array(mu).reshape(len(a), 3), np.array(mu_ref).reshape(len(a_ref), 3)), b
