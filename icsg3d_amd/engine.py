"""Thin Python handles over the C ABI (include/icsg3d.h): numpy in / numpy out.

These are what the reference-shaped classes (icsg3d_amd/unet/unet.py, icsg3d_amd/vae/lattice_vae.py)
call where the reference calls Keras.  All compute happens in libicsg3d_hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _jobs4(jobs):
    jobs = np.ascontiguousarray(jobs, np.int32)
    if jobs.ndim != 2 or jobs.shape[1] != 4:
        raise ValueError("jobs must be (B, 4) int32 {structure, r0, r1, r2}, got %s" % (jobs.shape,))
    return jobs


class _Net:
    """Common handle plumbing: named tensors, gradients, profiling, data-parallel comm."""

    def __init__(self):
        self._h = L._H(None)
        self._lib = L.load()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ics_net_destroy(self._h)
            self._h = L._H(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tensors
    def tensor_infos(self):
        n = C.c_int(0)
        L.check(self._lib.ics_net_num_tensors(self._h, C.byref(n)))
        out = []
        for i in range(n.value):
            name = C.c_char_p()
            nd = C.c_int(0)
            dims = (C.c_int64 * 5)()
            tr = C.c_int(0)
            L.check(self._lib.ics_net_tensor_info(self._h, i, C.byref(name), C.byref(nd), dims, C.byref(tr)))
            out.append((name.value.decode(), tuple(int(dims[k]) for k in range(nd.value)), bool(tr.value)))
        return out

    def get_tensor(self, name, shape=None):
        if shape is None:
            shape = dict((n, s) for n, s, _ in self.tensor_infos())[name]
        a = np.empty(shape, np.float32)
        L.check(self._lib.ics_net_get_tensor(self._h, name.encode(), L.fptr(a), a.size))
        return a

    def set_tensor(self, name, value):
        a = _f32(value)
        L.check(self._lib.ics_net_set_tensor(self._h, name.encode(), L.fptr(a), a.size))

    def get_grad(self, name, shape):
        a = np.empty(shape, np.float32)
        L.check(self._lib.ics_net_get_grad(self._h, name.encode(), L.fptr(a), a.size))
        return a

    def get_activation(self, layer, shape):
        a = np.empty(shape, np.float32)
        L.check(self._lib.ics_net_get_activation(self._h, layer.encode(), L.fptr(a), a.size))
        return a

    def get_bn_affine(self, layer, channels):
        sc = np.empty(channels, np.float32)
        sh = np.empty(channels, np.float32)
        L.check(self._lib.ics_net_get_bn_affine(self._h, layer.encode(), L.fptr(sc), L.fptr(sh), channels))
        return sc, sh

    def get_weights(self):
        return {n: self.get_tensor(n, s) for n, s, _ in self.tensor_infos()}

    def set_weights(self, weights):
        known = dict((n, s) for n, s, _ in self.tensor_infos())
        for k, v in weights.items():
            if k not in known:
                raise KeyError("unknown tensor %r" % k)
            if tuple(np.shape(v)) != known[k]:
                raise ValueError("shape mismatch for %s: %s vs %s" % (k, np.shape(v), known[k]))
            self.set_tensor(k, v)

    def check_canaries(self):
        """(dirty count, description): diagnosis aid, needs ICSG3D_DEBUG_CANARY=1 when the engine was created."""
        n = C.c_int(0)
        L.check(self._lib.ics_net_check_canaries(self._h, C.byref(n)))
        return n.value, (self._lib.ics_last_error().decode() if n.value else "")

    def set_lr(self, lr):
        L.check(self._lib.ics_net_set_lr(self._h, float(lr)))

    def reset_optimizer(self):
        L.check(self._lib.ics_net_reset_optimizer(self._h))

    def num_params(self):
        n = C.c_size_t(0)
        L.check(self._lib.ics_net_num_params(self._h, C.byref(n)))
        return int(n.value)

    def get_optimizer_state(self):
        """(m, v, t): Adam moments over the flat parameter buffer and the step count."""
        n = self.num_params()
        m, v, t = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int(0)
        L.check(self._lib.ics_net_get_optimizer_state(self._h, L.fptr(m), L.fptr(v), n, C.byref(t)))
        return m, v, int(t.value)

    def set_optimizer_state(self, m, v, t):
        m, v = _f32(m), _f32(v)
        L.check(self._lib.ics_net_set_optimizer_state(self._h, L.fptr(m), L.fptr(v), m.size, int(t)))

    def sync(self):
        L.check(self._lib.ics_net_sync(self._h))

    def share_stream(self, other):
        """enqueue on `other`'s stream from now on (joint training of two engines on one GPU: steps alternate in order)"""
        L.check(self._lib.ics_net_share_stream(self._h, other._h))
        self._stream_owner = other          # keep it alive

    def timer_start(self):
        L.check(self._lib.ics_net_timer_start(self._h))

    def timer_stop(self):
        """milliseconds of device time on the engine's stream since timer_start (waits for the work in between)"""
        ms = C.c_double(0)
        L.check(self._lib.ics_net_timer_stop(self._h, C.byref(ms)))
        return ms.value

    # ---- profiling (HIP events on the engine's stream)
    def graph_probe(self, iters=20):
        """Measurement aid: the resident train step eagerly and as a replayed hipGraph -> (eager ms, graph ms, graph nodes)."""
        a, b, n = C.c_double(0), C.c_double(0), C.c_int(0)
        L.check(self._lib.ics_net_graph_probe(self._h, int(iters), C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def profile_enable(self, on=True):
        L.check(self._lib.ics_net_profile_enable(self._h, 1 if on else 0))

    def profile_filter(self, prefix=""):
        """events only around launch sites whose label starts with `prefix` ("" = all)"""
        L.check(self._lib.ics_net_profile_filter(self._h, prefix.encode() if prefix else None))

    def profile_rows(self):
        n = C.c_int(0)
        L.check(self._lib.ics_net_profile_count(self._h, C.byref(n)))
        rows = []
        for i in range(n.value):
            label = C.c_char_p()
            cnt = C.c_int64(0)
            ms, fl, by = C.c_double(0), C.c_double(0), C.c_double(0)
            L.check(self._lib.ics_net_profile_row(self._h, i, C.byref(label), C.byref(cnt), C.byref(ms),
                                                  C.byref(fl), C.byref(by)))
            rows.append({"label": label.value.decode(), "launches": cnt.value, "ms": ms.value,
                         "flop": fl.value, "bytes": by.value})
        return rows

    # ---- data parallel
    def comm_init(self, rank, nranks, uid):
        L.check(self._lib.ics_net_comm_init(self._h, int(rank), int(nranks), uid))

    def broadcast_state(self, root=0):
        """rank `root`'s parameters, BN moving statistics and Adam state overwrite every replica's."""
        L.check(self._lib.ics_net_comm_broadcast_state(self._h, int(root)))

    def set_sync_bn(self, on=True):
        L.check(self._lib.ics_net_set_sync_bn(self._h, 1 if on else 0))

    def comm_info(self):
        r, n, b = C.c_int(0), C.c_int(0), C.c_int(0)
        L.check(self._lib.ics_net_comm_info(self._h, C.byref(r), C.byref(n), C.byref(b)))
        return {"rank": r.value, "nranks": n.value, "buckets_last_step": b.value}

    def allreduce_max(self, value):
        v = C.c_double(float(value))
        L.check(self._lib.ics_net_comm_allreduce_max(self._h, C.byref(v)))
        return v.value


FEED_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 3}       # ics_feed_config.x_dtype
FEED_LABELS = {"none": (0, None), "u8": (1, np.uint8), "f64": (2, np.float64), "f32": (3, np.float32),
               "onehot": (4, np.float32)}                                # ics_feed_config.label_kind, dtype of the source


def feed_config(x_channels, x_dtypes, label_kind="none", slots=2):
    """ics_feed_config for x parts of x_channels[i] channels and numpy dtypes x_dtypes[i], labels of kind `label_kind`."""
    x_channels, x_dtypes = [int(c) for c in x_channels], [np.dtype(t) for t in x_dtypes]
    if not 1 <= len(x_channels) <= 2 or len(x_dtypes) != len(x_channels):
        raise ValueError("a feed takes one or two x parts, each with a dtype")
    for t in x_dtypes:
        if t not in FEED_DTYPES:
            raise ValueError("x parts are float32 or float64, not %s" % t)
    if label_kind not in FEED_LABELS:
        raise ValueError("label_kind must be one of %s" % sorted(FEED_LABELS))
    pad = [0] * (2 - len(x_channels))
    return L.FeedConfig(int(slots), len(x_channels), (C.c_int * 2)(*(x_channels + pad)),
                        (C.c_int * 2)(*([FEED_DTYPES[t] for t in x_dtypes] + pad)), FEED_LABELS[label_kind][0])


class _FeedMixin:
    """Fed steps (include/icsg3d.h, csrc/feed.h): pinned staging slots the host fills with raw arrays, uploaded on a copy
    stream while the previous step runs and packed (cast, concatenate, labels) on the device."""

    _feed = None      # (x_channels, x_dtypes, label_kind, slots) of the open feed

    def feed_open(self, x_channels, x_dtypes, label_kind="none", slots=2):
        cfg = feed_config(x_channels, x_dtypes, label_kind, slots)
        L.check(self._lib.ics_net_feed_open(self._h, C.byref(cfg)))
        self._feed = (tuple(int(c) for c in x_channels), tuple(np.dtype(t) for t in x_dtypes), label_kind, int(slots))

    def feed_close(self):
        self._feed = None
        L.check(self._lib.ics_net_feed_close(self._h))

    def feed_slot(self, slot):
        """numpy views over the slot's pinned memory, each with max_batch leading rows: {"x": [part, ...], "labels",
        "cond", "eps"} (None for what the feed does not carry).  Returns once the slot's last upload has left the pinned
        memory; the views die with feed_close."""
        if self._feed is None:
            raise L.IcsError("the engine has no open feed (feed_open)")
        xc, xt, kind, _ = self._feed
        p = [C.c_void_p() for _ in range(5)]
        L.check(self._lib.ics_net_feed_slot(self._h, int(slot), *[C.byref(v) for v in p]))
        B, d = self.max_batch, self.d

        def view(ptr, shape, dtype):
            if not ptr.value:
                return None
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * n).from_address(ptr.value), dtype=dtype).reshape(shape)

        out = {"x": [view(p[i], (B, d, d, d, xc[i]), xt[i]) for i in range(len(xc))]}
        ldt = FEED_LABELS[kind][1]
        out["labels"] = None if ldt is None else view(
            p[2], (B, d, d, d, self.num_classes) if kind == "onehot" else (B, d, d, d), ldt)
        out["cond"] = view(p[3], (B, getattr(self, "cond_shape", 0)), np.float32)
        out["eps"] = view(p[4], (B, getattr(self, "latent_dim", 0)), np.float32)
        return out

    def feed_submit(self, slot, batch, rotations=None):
        """rotations (batch,3) int32, entries -1..2 (icsg3d_amd.augment): the step that consumes the slot packs through
        it; None is the plain submit"""
        if rotations is None:
            L.check(self._lib.ics_net_feed_submit(self._h, int(slot), int(batch)))
        else:
            L.check(self._lib.ics_net_feed_submit_rot(self._h, int(slot), int(batch), _rot_table(rotations, batch)))

    def _step_fed(self, fn, slot):
        t = C.c_int(-1)
        L.check(fn(self._h, int(slot), C.byref(t)))
        return t.value

    def feed_metrics(self, ticket):
        m = np.zeros(8, np.float32)
        L.check(self._lib.ics_net_feed_metrics(self._h, int(ticket), L.fptr(m)))
        return m[:self._n_metrics]


def _rot_table(rotations, batch):
    """a (batch,3) rotation table as the int32 pointer of ics_net_feed_submit_rot / ics_op_feed_pack_rot"""
    rot = np.ascontiguousarray(rotations, np.int32)
    if rot.shape != (int(batch), 3):
        raise ValueError("a rotation table is (batch, 3), not %s for a batch of %d" % (rot.shape, batch))
    return rot.ctypes.data_as(C.POINTER(C.c_int32))


def feed_pack(x_parts, labels=None, label_kind="none", num_classes=0, rotations=None):
    """Single-op entry (ics_op_feed_pack / ics_op_feed_pack_rot): the pack kernel alone on host arrays.  x_parts: one or two
    (B,d,d,d,c) float32 / float64 arrays; labels as label_kind says; rotations (B,3) int32, entries -1..2, or None.
    Returns (x float32 (B,d,d,d,sum c), labels uint8 (B,d,d,d) | None)."""
    lib = L.load()
    parts = [np.ascontiguousarray(a) for a in x_parts]
    B, d = parts[0].shape[0], parts[0].shape[1]
    cfg = feed_config([a.shape[4] for a in parts], [a.dtype for a in parts], label_kind)
    lab = None
    if label_kind != "none":
        lab = np.ascontiguousarray(labels, FEED_LABELS[label_kind][1])
        want = (B, d, d, d, num_classes) if label_kind == "onehot" else (B, d, d, d)
        if lab.shape != want:
            raise ValueError("labels must be %s, got %s" % (want, lab.shape))
    for a in parts:
        if a.shape[:4] != (B, d, d, d):
            raise ValueError("bad x part shape %s" % (a.shape,))
    x = np.empty((B, d, d, d, sum(a.shape[4] for a in parts)), np.float32)
    out = np.empty((B, d, d, d), np.uint8) if lab is not None else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    if rotations is None:
        L.check(lib.ics_op_feed_pack(C.byref(cfg), vp(parts[0]), vp(parts[1]) if len(parts) == 2 else None, vp(lab), B, d,
                                     int(num_classes), L.fptr(x), L.u8ptr(out)))
    else:
        L.check(lib.ics_op_feed_pack_rot(C.byref(cfg), vp(parts[0]), vp(parts[1]) if len(parts) == 2 else None, vp(lab),
                                         _rot_table(rotations, B), B, d, int(num_classes), L.fptr(x), L.u8ptr(out)))
    return x, out


def label_counts(labels, num_classes, label_kind=None):
    """Single-op entry (ics_op_label_counts): exact counts per class id of a uint8 / float32 / float64 label array of any
    shape, computed on the device.  Returns (counts int64 (num_classes,), out_of_range int): values that are no class id
    (below 0, >= num_classes, non-integral, NaN) are counted in out_of_range and in no bin.  label_kind "onehot" is
    refused by the library (class ids only); by default the kind follows the array's dtype."""
    lib = L.load()
    lab = np.asarray(labels)
    if label_kind is None:
        kinds = {np.dtype(np.uint8): "u8", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
        if lab.dtype not in kinds:
            raise ValueError("labels must be uint8, float32 or float64 class ids, not %s" % lab.dtype)
        label_kind = kinds[lab.dtype]
    if label_kind not in FEED_LABELS or label_kind == "none":
        raise ValueError("label_kind must be one of u8, f32, f64")
    if label_kind != "onehot":
        lab = np.ascontiguousarray(lab, FEED_LABELS[label_kind][1]).reshape(-1)
    else:
        lab = np.ascontiguousarray(lab, np.float32).reshape(-1)
    counts = np.zeros(int(num_classes), np.int64)
    oor = np.zeros(1, np.int64)
    L.check(lib.ics_op_label_counts(lab.ctypes.data_as(C.c_void_p), FEED_LABELS[label_kind][0], lab.size, int(num_classes),
                                    L.i64ptr(counts), L.i64ptr(oor)))
    return counts, int(oor[0])


def _label_kind_of(lab):
    kinds = {np.dtype(np.uint8): "u8", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
    if lab.dtype not in kinds:
        raise ValueError("labels must be uint8, float32 or float64 class ids, not %s" % lab.dtype)
    return kinds[lab.dtype]


def confusion(true, pred, num_classes, mask=None, label_kind=None):
    """Single-op entry (ics_op_confusion): the confusion matrix of (true label, predicted label) pairs, counted on the
    device.  true: uint8 / float32 / float64 class ids of any shape (the kind follows the dtype unless label_kind says
    otherwise; "onehot" is refused by the library); pred and mask: uint8 arrays of the same size.  Returns
    (matrix int64 (num_classes, num_classes) [true, predicted], occupancy int64 (2, 2) [true != 0, mask != 0] or None
    without a mask, out_of_range int): pairs whose true value is no class id (below 0, >= num_classes, non-integral,
    NaN) or whose prediction is >= num_classes are counted in out_of_range and in no bin; the occupancy table covers
    the pairs with a valid true label."""
    lib = L.load()
    t = np.asarray(true)
    if label_kind is None:
        label_kind = _label_kind_of(t)
    if label_kind not in FEED_LABELS or label_kind == "none":
        raise ValueError("label_kind must be one of u8, f32, f64")
    t = np.ascontiguousarray(t, FEED_LABELS[label_kind][1]).reshape(-1)
    p = np.ascontiguousarray(pred, np.uint8).reshape(-1)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    if label_kind != "onehot" and (p.size != t.size or (m is not None and m.size != t.size)):
        raise ValueError("true, pred and mask must have the same number of elements")
    k = int(num_classes)
    matrix = np.zeros((max(k, 0), max(k, 0)), np.int64)
    occ = None if m is None else np.zeros((2, 2), np.int64)
    oor = np.zeros(1, np.int64)
    L.check(lib.ics_op_confusion(t.ctypes.data_as(C.c_void_p), FEED_LABELS[label_kind][0], L.u8ptr(p), L.u8ptr(m), p.size, k,
                                 L.i64ptr(matrix), L.i64ptr(occ), L.i64ptr(oor)))
    return matrix, occ, int(oor[0])


def confusion_grid():
    """(lanes per block, pairs per lane and pass, grid cap) of the confusion kernel (ics_op_confusion_grid)."""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    L.check(L.load().ics_op_confusion_grid(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def comm_unique_id():
    buf = C.create_string_buffer(128)
    L.check(L.load().ics_comm_unique_id(buf))
    return buf.raw


class UnetEngine(_Net, _FeedMixin):
    def __init__(self, in_channels=1, num_classes=95, d=32, max_batch=32, lr=1e-6, loss_weight=0.0,
                 pool_ties="tf_cpu", bn_unbias=True, device=None, bce_from_logits=False):
        super().__init__()
        if device is not None:
            L.check(self._lib.ics_set_device(int(device)))
        self.in_channels, self.num_classes, self.d, self.max_batch = in_channels, num_classes, d, max_batch
        cfg = L.UnetConfig(in_channels, num_classes, d, max_batch, lr, loss_weight,
                           1 if pool_ties == "tf_cpu" else 0, 1 if bn_unbias else 0, 1 if bce_from_logits else 0)
        L.check(self._lib.ics_unet_create(C.byref(cfg), C.byref(self._h)))

    def _check_x(self, x):
        x = _f32(x)
        d = self.d
        if x.ndim != 5 or x.shape[1:] != (d, d, d, self.in_channels):
            raise ValueError("expected (B,%d,%d,%d,%d), got %s" % (d, d, d, self.in_channels, x.shape))
        return x

    def predict(self, x):
        x = self._check_x(x)
        B, d = x.shape[0], self.d
        soft = np.empty((B, d, d, d, self.num_classes), np.float32)
        sig = np.empty((B, d, d, d, 1), np.float32)
        for i in range(0, B, self.max_batch):
            xs = x[i:i + self.max_batch]
            L.check(self._lib.ics_unet_predict(self._h, L.fptr(xs), xs.shape[0], L.fptr(soft[i:i + self.max_batch]),
                                               L.fptr(sig[i:i + self.max_batch])))
        return soft, sig

    def predict_labels(self, x, thresh=0.8):
        x = self._check_x(x)
        B, d = x.shape[0], self.d
        sp = np.empty((B, d, d, d), np.uint8)
        mk = np.empty((B, d, d, d), np.uint8)
        for i in range(0, B, self.max_batch):
            xs = x[i:i + self.max_batch]
            L.check(self._lib.ics_unet_predict_labels(self._h, L.fptr(xs), xs.shape[0], float(thresh),
                                                      L.u8ptr(sp[i:i + self.max_batch]), L.u8ptr(mk[i:i + self.max_batch])))
        return sp, mk

    def _labels(self, labels, B):
        lab = np.ascontiguousarray(labels, dtype=np.uint8)
        if lab.shape != (B, self.d, self.d, self.d):
            raise ValueError("labels must be (B,d,d,d) uint8 class ids, got %s" % (lab.shape,))
        return lab

    def train_step(self, x, labels):
        x = self._check_x(x)
        lab = self._labels(labels, x.shape[0])
        m = np.zeros(5, np.float32)
        L.check(self._lib.ics_unet_train_step(self._h, L.fptr(x), L.u8ptr(lab), x.shape[0], L.fptr(m)))
        return m

    def test_step(self, x, labels):
        x = self._check_x(x)
        lab = self._labels(labels, x.shape[0])
        m = np.zeros(5, np.float32)
        L.check(self._lib.ics_unet_test_step(self._h, L.fptr(x), L.u8ptr(lab), x.shape[0], L.fptr(m)))
        return m

    def set_class_weights(self, w):
        """Per-class loss weights (num_classes,) for every later train / test step (ics_unet_set_class_weights); None
        switches back to the scalar loss_weight."""
        if w is None:
            L.check(self._lib.ics_unet_set_class_weights(self._h, None, 0))
            return
        w = np.ascontiguousarray(w, np.float32).reshape(-1)
        L.check(self._lib.ics_unet_set_class_weights(self._h, L.fptr(w), int(w.size)))

    def get_class_weights(self):
        """The active table (num_classes,) float32, or None while the scalar loss_weight is in force."""
        w = np.zeros(self.num_classes, np.float32)
        active = C.c_int(0)
        L.check(self._lib.ics_unet_get_class_weights(self._h, L.fptr(w), self.num_classes, C.byref(active)))
        return w if active.value else None

    def metric_sums(self):
        """The K.sum terms of the last step's metrics (unet/unet.py:159-193): dict(sum_lsoft, sum_lsig, tp, predicted,
        wr_tp, wr_possible, voxels)."""
        s = (C.c_double * 7)()
        L.check(self._lib.ics_unet_metric_sums(self._h, s))
        return dict(zip(("sum_lsoft", "sum_lsig", "tp", "predicted", "wr_tp", "wr_possible", "voxels"), [float(v) for v in s]))

    def upload_batch(self, x, labels):
        x = self._check_x(x)
        lab = self._labels(labels, x.shape[0])
        L.check(self._lib.ics_unet_upload_batch(self._h, L.fptr(x), L.u8ptr(lab), x.shape[0]))

    def voxelise_batch(self, structs, jobs, eps_frac=0.25, label_frac=1.0):
        """create_matrices.py's grids of `jobs` (matrices.make_jobs) computed straight into the resident batch: x = M
        or [M, p], labels = S -- what upload_batch of UnetDataGenerator's arrays over the saved files would upload,
        bit for bit.  Enqueued only; train_step_resident / predict_resident follow."""
        jobs = _jobs4(jobs)
        cs = structs.c_struct()
        L.check(self._lib.ics_unet_voxelise_batch(self._h, C.byref(cs), L.i32ptr(jobs), len(jobs), float(eps_frac),
                                                  float(label_frac)))

    def predict_resident(self, labels_only=False, thresh=0.8):
        """model.predict on the uploaded batch, enqueued only; the outputs stay in HBM (benchmark path)."""
        L.check(self._lib.ics_unet_predict_resident(self._h, 1 if labels_only else 0, float(thresh)))

    # ---- the confusion accumulator (include/icsg3d.h "confusion matrix"): eval-mode passes only, nothing is trained
    def confusion_open(self):
        """A zeroed device accumulator in the engine's memory (allocated by the first open)."""
        L.check(self._lib.ics_unet_confusion_open(self._h))

    def confusion_reset(self):
        L.check(self._lib.ics_unet_confusion_reset(self._h))

    def confusion_step(self, thresh=0.8):
        """Eval forward on the resident batch (uploaded WITH labels), argmax / sig >= thresh, and the count of
        (label, species, mask) added to the accumulator.  Enqueued only."""
        L.check(self._lib.ics_unet_confusion_step(self._h, float(thresh)))

    def confusion_batch(self, x, labels, thresh=0.8):
        """upload_batch + confusion_step for host arrays of any length (max_batch samples at a time)."""
        x = self._check_x(x)
        lab = self._labels(labels, x.shape[0])
        for i in range(0, x.shape[0], self.max_batch):
            xs, ls = x[i:i + self.max_batch], lab[i:i + self.max_batch]
            L.check(self._lib.ics_unet_confusion_batch(self._h, L.fptr(xs), L.u8ptr(ls), xs.shape[0], float(thresh)))

    def confusion_read(self):
        """Waits for the stream -> dict(matrix int64 (K, K) [true, predicted], occupancy int64 (2, 2)
        [true != 0, mask != 0], out_of_range, voxels).  Does not reset."""
        k = self.num_classes
        matrix, occ = np.zeros((k, k), np.int64), np.zeros((2, 2), np.int64)
        oor, vox = np.zeros(1, np.int64), np.zeros(1, np.int64)
        L.check(self._lib.ics_unet_confusion_read(self._h, L.i64ptr(matrix), L.i64ptr(occ), L.i64ptr(oor), L.i64ptr(vox)))
        return {"matrix": matrix, "occupancy": occ, "out_of_range": int(oor[0]), "voxels": int(vox[0])}

    # ---- the atom-score accumulator (include/icsg3d.h "atom score"): eval-mode passes only, nothing is trained
    def atom_score_open(self, tol=2.0, min_voxels=3, max_atoms=512):
        """Zeroed device tallies and two segmentation workspaces in the engine's memory (allocated by the first open; a
        later open may change tol and min_voxels, not max_atoms)."""
        L.check(self._lib.ics_unet_atom_score_open(self._h, float(tol), int(min_voxels), int(max_atoms)))

    def atom_score_reset(self):
        L.check(self._lib.ics_unet_atom_score_reset(self._h))

    def atom_score_step(self, thresh=0.8, with_confusion=False):
        """Eval forward on the resident batch (uploaded WITH labels), argmax / sig >= thresh, the components of the
        predictions and of the true labels, their matching and its tallies added to the accumulator; with_confusion also
        adds the voxel counts to the open confusion accumulator.  Enqueued only."""
        L.check(self._lib.ics_unet_atom_score_step(self._h, float(thresh), 1 if with_confusion else 0))

    def atom_score_batch(self, x, labels, thresh=0.8, with_confusion=False):
        """upload_batch + atom_score_step for host arrays of any length (max_batch samples at a time)."""
        x = self._check_x(x)
        lab = self._labels(labels, x.shape[0])
        for i in range(0, x.shape[0], self.max_batch):
            xs, ls = x[i:i + self.max_batch], lab[i:i + self.max_batch]
            L.check(self._lib.ics_unet_atom_score_batch(self._h, L.fptr(xs), L.u8ptr(ls), xs.shape[0], float(thresh),
                                                        1 if with_confusion else 0))

    def atom_score_read(self):
        """Waits for the stream -> the tallies of icsg3d_amd.atomscore.TALLIES as a dict of int64 arrays (matrix
        (K + 1, K + 1) [true, predicted] with index K = no atom).  Does not reset."""
        from .atomscore import empty_tallies
        t = empty_tallies(self.num_classes)
        L.check(self._lib.ics_unet_atom_score_read(self._h, *[L.i64ptr(t[k]) for k in t]))
        return t

    _n_metrics = 5

    def train_step_fed(self, slot):
        """the train step on a submitted slot, enqueued only -> the ticket of its metrics (feed_metrics)"""
        return self._step_fed(self._lib.ics_unet_train_step_fed, slot)

    def test_step_fed(self, slot):
        return self._step_fed(self._lib.ics_unet_test_step_fed, slot)

    def train_step_resident(self, want_metrics=False):
        if want_metrics:
            m = np.zeros(5, np.float32)
            L.check(self._lib.ics_unet_train_step_resident(self._h, L.fptr(m)))
            return m
        L.check(self._lib.ics_unet_train_step_resident(self._h, None))
        return None


class _AtomsOut:
    """The host arrays the decoder -> U-Net -> atoms tail fills for B samples, the ctypes arguments that point a C entry
    at a slice of them, and the result dict the three *_to_atoms methods return."""

    def __init__(self, B, d, max_atoms, want_density, want_regions):
        from .watershed import STAT_FIELDS
        self.B, self.d, self.max_atoms = B, d, max_atoms
        self.species = np.empty((B, d, d, d), np.uint8)
        self.mask = np.empty((B, d, d, d), np.uint8)
        self.density = np.empty((B, d, d, d), np.float32) if want_density else None
        self.coord_minmax = np.zeros((B, 3, 2), np.float32)
        self.regions = np.empty((B, d, d, d), np.int32) if want_regions else None
        self.counts = np.zeros((B, 2), np.int32)
        self.stats = np.zeros((B, max_atoms, len(STAT_FIELDS)), np.int32)
        self.bounds = np.zeros((B, max_atoms, 8), np.int64) if want_regions else None   # refine_atoms' convexity shortcut

    def label_args(self, s=slice(None)):
        """species, mask, density, coord_minmax of samples s, as every entry point of the tail takes them"""
        cut = lambda a: a[s] if a is not None else None
        return (L.u8ptr(self.species[s]), L.u8ptr(self.mask[s]), L.fptr(cut(self.density)), L.fptr(self.coord_minmax[s]))

    def args(self, s=slice(None)):
        """the eight output pointers of the *_to_unet_atoms entry points for samples s"""
        cut = lambda a: a[s] if a is not None else None
        return self.label_args(s) + (L.i32ptr(cut(self.regions)), L.i32ptr(self.counts[s]), L.i32ptr(self.stats[s]),
                                     L.i64ptr(cut(self.bounds)))

    def result(self):
        from .watershed import _atoms_from_stats
        counts = self.counts
        failed = counts[:, 1] > self.max_atoms            # more kept components than rows: sample skipped, not the batch
        counts[failed, 1] = 0
        return {"species": self.species, "mask": self.mask, "density": self.density, "coord_minmax": self.coord_minmax,
                "regions": self.regions, "n_components": counts[:, 0].copy(), "n_atoms": counts[:, 1].copy(),
                "stats": self.stats, "bounds": self.bounds, "atoms": _atoms_from_stats(counts, self.stats, self.d ** 3),
                "failed": failed}


class VaeEngine(_Net, _FeedMixin):
    def __init__(self, unet: UnetEngine, in_channels=1, cond_shape=10, latent_dim=256,
                 filters=(16, 32, 64, 128), d=32, max_batch=32, lr=5e-4, alpha=0.5, beta=3e-4,
                 pm_layer_weights=(1.0, 1.0, 1.0, 1.0), bn_unbias=True):
        super().__init__()
        self.unet = unet   # keep the perceptual engine alive
        self.in_channels, self.cond_shape, self.latent_dim, self.d, self.max_batch = (
            in_channels, cond_shape, latent_dim, d, max_batch)
        self._resident = 0   # batch of the engine's resident inputs (every call that uploads x, cond, eps sets it)
        self._slot_batch = {}   # batch submitted to each feed slot: the resident batch once a fed step has packed it
        cfg = L.VaeConfig(in_channels, cond_shape, latent_dim, (C.c_int * 4)(*filters), d, max_batch, lr,
                          alpha, beta, (C.c_float * 4)(*pm_layer_weights), 1 if bn_unbias else 0)
        L.check(self._lib.ics_vae_create(C.byref(cfg), unet._h if unet is not None else None, C.byref(self._h)))

    def _args(self, x, cond, eps):
        x, cond = _f32(x), _f32(cond)
        B = x.shape[0]
        d = self.d
        if x.shape != (B, d, d, d, self.in_channels):
            raise ValueError("bad input shape %s" % (x.shape,))
        if cond.shape != (B, self.cond_shape):
            raise ValueError("bad cond shape %s" % (cond.shape,))
        eps = _f32(eps)
        if eps.shape != (B, self.latent_dim):
            raise ValueError("bad eps shape %s" % (eps.shape,))
        return x, cond, eps, B

    def encode(self, x, cond, eps):
        x, cond, eps, B = self._args(x, cond, eps)
        zm = np.empty((B, self.latent_dim), np.float32)
        zlv = np.empty_like(zm)
        z = np.empty_like(zm)
        for i in range(0, B, self.max_batch):
            s = slice(i, i + self.max_batch)
            L.check(self._lib.ics_vae_encode(self._h, L.fptr(x[s]), L.fptr(cond[s]), L.fptr(eps[s]), x[s].shape[0],
                                             L.fptr(zm[s]), L.fptr(zlv[s]), L.fptr(z[s])))
            self._resident = x[s].shape[0]
        return zm, zlv, z

    def decode(self, z, cond):
        z, cond = _f32(z), _f32(cond)
        B, d = z.shape[0], self.d
        out = np.empty((B, d, d, d, self.in_channels), np.float32)
        for i in range(0, B, self.max_batch):
            s = slice(i, i + self.max_batch)
            L.check(self._lib.ics_vae_decode(self._h, L.fptr(z[s]), L.fptr(cond[s]), z[s].shape[0], L.fptr(out[s])))
        return out

    def decode_to_labels(self, unet, z, cond, thresh=0.8, want_density=True):
        """decoder.predict -> unet.model.predict -> argmax / threshold without leaving the device
        (generate.py:204-225).  Returns dict(species u8, mask u8, density f32 | None, coord_minmax (B,3,2))."""
        z, cond = _f32(z), _f32(cond)
        out = _AtomsOut(z.shape[0], self.d, 0, want_density, False)
        mb = min(self.max_batch, unet.max_batch)
        for i in range(0, out.B, mb):
            s = slice(i, i + mb)
            L.check(self._lib.ics_vae_decode_to_unet_labels(
                self._h, unet._h, L.fptr(z[s]), L.fptr(cond[s]), z[s].shape[0], float(thresh), *out.label_args(s)))
        return {"species": out.species, "mask": out.mask, "density": out.density, "coord_minmax": out.coord_minmax}

    def decode_to_atoms(self, unet, z, cond, thresh=0.8, min_voxels=3, max_atoms=512, want_density=True,
                        want_regions=False):
        """decode_to_labels continued on the device through connected components + region statistics
        (generate.py:204-236, watershed.py:52-56,153-187): dict(species, mask, density, coord_minmax, regions | None,
        n_components (B,), n_atoms (B,), stats int32 (B,max_atoms,11), atoms [(species list, mean list)], failed (B,)).
        Every kept component is taken as convex here; icsg3d_amd.watershed.refine_atoms continues with the convexity
        test and the recursive split (needs want_regions=True)."""
        z, cond = _f32(z), _f32(cond)
        out = _AtomsOut(z.shape[0], self.d, max_atoms, want_density, want_regions)
        mb = min(self.max_batch, unet.max_batch)
        for i in range(0, out.B, mb):
            s = slice(i, i + mb)
            L.check(self._lib.ics_vae_decode_to_unet_atoms(
                self._h, unet._h, L.fptr(z[s]), L.fptr(cond[s]), z[s].shape[0], float(thresh), int(min_voxels),
                int(max_atoms), *out.args(s)))
        return out.result()

    def reconstruct_to_atoms(self, unet, x=None, cond=None, eps=None, thresh=0.8, min_voxels=3, max_atoms=512,
                             want_density=True, want_regions=False):
        """vae.model.predict([M, cond]) -> unet.model.predict -> argmax / threshold -> components + statistics
        (eval.py:163-175) in one device-resident chain: encode, sample z with the batch's eps (F8), decode, segment.
        With x (and cond, eps) the batch is uploaded first (upload_batch), max_batch samples at a time; without, the
        resident batch placed by upload_batch / voxelise_batch is used and left unchanged.  Returns decode_to_atoms'
        dict, bit for bit what decode_to_atoms(unet, encode(x, cond, eps)[2], cond) returns."""
        if x is None and (cond is not None or eps is not None):
            raise ValueError("cond / eps go with x; the resident batch carries its own")
        if x is not None:
            x, cond, eps, B = self._args(x, cond, eps)
        else:
            B = self._resident
            if not B:
                raise RuntimeError("no resident batch: call upload_batch or voxelise_batch first")
        out = _AtomsOut(B, self.d, max_atoms, want_density, want_regions)
        mb = min(self.max_batch, unet.max_batch) if x is not None else B
        for i in range(0, B, mb):
            s = slice(i, i + mb)
            if x is not None:
                self.upload_batch(x[s], cond[s], eps[s])
            L.check(self._lib.ics_vae_reconstruct_resident_to_unet_atoms(
                self._h, unet._h, float(thresh), int(min_voxels), int(max_atoms), *out.args(s)))
        return out.result()

    def render_resident(self, which=0, cam=None, size=256, mode="value", alpha=0.2, floor=-1.0, lut=None):
        """The density picture (icsg3d_amd.render.density) of channel 0 of what the engine holds, read where it lies:
        which = 0 the resident input batch, 1 the reconstruction the last decoder pass left (view_results.py:152-183,
        the M panels).  float32 premultiplied RGBA (resident batch, height, width, 4), the bits render.density gives
        for the same values."""
        from . import render as R
        if not self._resident:
            raise RuntimeError("no resident batch: call upload_batch or voxelise_batch first")
        w, h = R._size(size)
        cam = R._cam(cam)
        lut = np.ascontiguousarray(R.VIRIDIS if lut is None else lut, np.float32)
        if lut.shape != (256, 3):
            raise ValueError("lut must be (256, 3)")
        out = np.empty((self._resident, h, w, 4), np.float32)
        L.check(self._lib.ics_vae_render_resident(self._h, int(which), R._mode(mode), float(alpha), float(floor),
                                                  L.fptr(lut), L.f64ptr(cam), w, h, L.fptr(out)))
        return out

    def _interp_args(self, a, b, cond, eps_a, eps_b, alpha, mode):
        a, b, cond, eps_a, eps_b = _f32(a), _f32(b), _f32(cond), _f32(eps_a), _f32(eps_b)
        P, d = a.shape[0], self.d
        if a.shape != (P, d, d, d, self.in_channels) or b.shape != a.shape:
            raise ValueError("bad endpoint shapes %s / %s" % (a.shape, b.shape))
        if cond.shape != (P, self.cond_shape):
            raise ValueError("bad cond shape %s" % (cond.shape,))
        if eps_a.shape != (P, self.latent_dim) or eps_b.shape != eps_a.shape:
            raise ValueError("bad eps shapes %s / %s" % (eps_a.shape, eps_b.shape))
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        return a, b, cond, eps_a, eps_b, alpha, P, latent_mode(mode)

    def interpolate(self, a, b, cond, eps_a, eps_b, alpha, mode="lerp", want_recon=True):
        """interpolate.py:50-59 for P pairs as device-resident chains (ics_vae_interpolate): a, b (P,d,d,d,C), cond
        (P,cond_shape), eps_a / eps_b (P,latent) the two sampling draws, alpha (S,) float64 = np.linspace(0, max_alpha, S).
        Returns (z_ends (P,2,latent), z_path (P,S,latent), recon (P,S,d,d,d,C) | None).  Overwrites the resident batch."""
        a, b, cond, eps_a, eps_b, alpha, P, mode = self._interp_args(a, b, cond, eps_a, eps_b, alpha, mode)
        S, d = len(alpha), self.d
        z_ends = np.empty((P, 2, self.latent_dim), np.float32)
        z_path = np.empty((P, S, self.latent_dim), np.float32)
        recon = np.empty((P, S, d, d, d, self.in_channels), np.float32) if want_recon else None
        self._resident = 0
        L.check(self._lib.ics_vae_interpolate(self._h, L.fptr(a), L.fptr(b), L.fptr(cond), L.fptr(eps_a), L.fptr(eps_b), P,
                                              L.f64ptr(alpha), S, mode, L.fptr(z_ends), L.fptr(z_path), L.fptr(recon)))
        return z_ends, z_path, recon

    def interpolate_to_atoms(self, unet, a, b, cond, eps_a, eps_b, alpha, mode="lerp", thresh=0.8, min_voxels=3,
                             max_atoms=512, want_density=True, want_regions=False):
        """interpolate continued for every frame as decode_to_atoms (ics_vae_interpolate_to_unet_atoms): decode_to_atoms'
        dict for the P*S frames, frame p*S + k, plus z_ends (P,2,latent) and z_path (P,S,latent)."""
        a, b, cond, eps_a, eps_b, alpha, P, mode = self._interp_args(a, b, cond, eps_a, eps_b, alpha, mode)
        S = len(alpha)
        z_ends = np.empty((P, 2, self.latent_dim), np.float32)
        z_path = np.empty((P, S, self.latent_dim), np.float32)
        out = _AtomsOut(P * S, self.d, max_atoms, want_density, want_regions)
        self._resident = 0
        L.check(self._lib.ics_vae_interpolate_to_unet_atoms(
            self._h, unet._h, L.fptr(a), L.fptr(b), L.fptr(cond), L.fptr(eps_a), L.fptr(eps_b), P, L.f64ptr(alpha), S, mode,
            float(thresh), int(min_voxels), int(max_atoms), L.fptr(z_ends), L.fptr(z_path), *out.args()))
        return dict(out.result(), z_ends=z_ends, z_path=z_path)

    def train_step(self, x, cond, eps):
        x, cond, eps, B = self._args(x, cond, eps)
        m = np.zeros(4, np.float32)
        L.check(self._lib.ics_vae_train_step(self._h, L.fptr(x), L.fptr(cond), L.fptr(eps), B, L.fptr(m)))
        self._resident = B
        return m

    def test_step(self, x, cond, eps):
        x, cond, eps, B = self._args(x, cond, eps)
        m = np.zeros(4, np.float32)
        L.check(self._lib.ics_vae_test_step(self._h, L.fptr(x), L.fptr(cond), L.fptr(eps), B, L.fptr(m)))
        self._resident = B
        return m

    def upload_batch(self, x, cond, eps):
        x, cond, eps, B = self._args(x, cond, eps)
        L.check(self._lib.ics_vae_upload_batch(self._h, L.fptr(x), L.fptr(cond), L.fptr(eps), B))
        self._resident = B

    def voxelise_batch(self, structs, jobs, cond, eps, eps_frac=0.25, label_frac=1.0):
        """As UnetEngine.voxelise_batch for the VAE's input; cond (B, cond_shape) and eps (B, latent_dim) are
        uploaded as by upload_batch."""
        jobs = _jobs4(jobs)
        B = len(jobs)
        cond, eps = _f32(cond), _f32(eps)
        if cond.shape != (B, self.cond_shape):
            raise ValueError("bad cond shape %s" % (cond.shape,))
        if eps.shape != (B, self.latent_dim):
            raise ValueError("bad eps shape %s" % (eps.shape,))
        cs = structs.c_struct()
        L.check(self._lib.ics_vae_voxelise_batch(self._h, C.byref(cs), L.i32ptr(jobs), B, float(eps_frac),
                                                 float(label_frac), L.fptr(cond), L.fptr(eps)))
        self._resident = B

    _n_metrics = 4

    def feed_submit(self, slot, batch, rotations=None):
        super().feed_submit(slot, batch, rotations)
        self._slot_batch[int(slot)] = int(batch)

    def train_step_fed(self, slot):
        t = self._step_fed(self._lib.ics_vae_train_step_fed, slot)
        self._resident = self._slot_batch[int(slot)]
        return t

    def test_step_fed(self, slot):
        t = self._step_fed(self._lib.ics_vae_test_step_fed, slot)
        self._resident = self._slot_batch[int(slot)]
        return t

    def train_step_resident(self, want_metrics=False):
        if want_metrics:
            m = np.zeros(4, np.float32)
            L.check(self._lib.ics_vae_train_step_resident(self._h, L.fptr(m)))
            return m
        L.check(self._lib.ics_vae_train_step_resident(self._h, None))
        return None


LATENT_MODES = {"lerp": 0, "slerp": 1}


def latent_mode(mode):
    if mode in LATENT_MODES:
        return LATENT_MODES[mode]
    if mode in (0, 1) and not isinstance(mode, bool):
        return int(mode)
    raise ValueError("mode must be 'lerp' or 'slerp', not %r" % (mode,))


def latent_path(za, zb, alpha, mode="lerp"):
    """Single-op entry (ics_op_latent_path): the walk of interpolate.py:54-56 between latent codes za, zb (P,latent)
    float32 at the float64 steps alpha (S,); returns (P,S,latent) float32.  lerp is the reference's arithmetic bit for
    bit; slerp falls back to it for (anti)parallel or zero codes -- see include/icsg3d.h."""
    lib = L.load()
    za, zb = _f32(za), _f32(zb)
    if za.ndim != 2 or zb.shape != za.shape:
        raise ValueError("bad code shapes %s / %s" % (za.shape, zb.shape))
    alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
    P, lat = za.shape
    out = np.empty((P, len(alpha), lat), np.float32)
    L.check(lib.ics_op_latent_path(L.fptr(za), L.fptr(zb), P, lat, L.f64ptr(alpha), len(alpha), latent_mode(mode),
                                   L.fptr(out)))
    return out


def conv3d_forward(x, w, bias=None, pre_act=0):
    """Single-op entry (kernel parity tests): x (B,S,S,S,Cin), w (k,k,k,Cin,Cout)."""
    lib = L.load()
    x, w = _f32(x), _f32(w)
    B, S, Cin = x.shape[0], x.shape[1], x.shape[4]
    taps, Cout = w.shape[0] ** 3, w.shape[4]
    y = np.empty((B, S, S, S, Cout), np.float32)
    b = _f32(bias) if bias is not None else None
    L.check(lib.ics_op_conv3d_forward(L.fptr(x), L.fptr(w), L.fptr(b), B, S, Cin, Cout, taps, pre_act, L.fptr(y)))
    return y


class _OpArgs:
    """What the wrappers of the struct-taking layer ops share: the arrays the struct points into, the shard split of
    emulated ranks and the per-rank text buffer."""

    def __init__(self, ranks):
        self.R = int(ranks)
        if not 0 <= self.R <= 4:
            raise ValueError("ranks must be in 0..4")
        self.lead = (self.R,) if self.R else ()
        self.keep = []                                # arrays the struct points into

    def f(self, v):
        if v is None:
            return None
        self.keep.append(_f32(v))
        return L.fptr(self.keep[-1])

    def out(self, shape):
        self.keep.append(np.empty(shape, np.float32))
        return self.keep[-1]

    def shard(self, NB):                              # B of each rank, from the NB samples in the tensors
        if NB % max(self.R, 1):
            raise ValueError("the batch does not divide into %d equal shards" % self.R)
        return NB // max(self.R, 1)

    def text(self, cap):                              # (pointer, cap) of a buffer of cap bytes per rank
        self._text, self._cap = C.create_string_buffer(cap * max(self.R, 1)), cap
        return C.cast(self._text, C.c_void_p), cap

    def lines(self):                                  # the text's lines, one list per rank (one list without ranks)
        raw, cap = self._text.raw, self._cap
        return [raw[i * cap:(i + 1) * cap].split(b"\0", 1)[0].decode().splitlines() for i in range(max(self.R, 1))]


def conv_layer(sources, w, bias=None, gamma=None, beta=None, dout=None, pre_act=0, has_bn=True, post_act=0,
               pad_input=False, max_batch=None, want_dx=True, ranks=0):
    """Single-op entry (ics_op_conv_layer): one layer through the engines' own construction and dispatch -- affine /
    activated / upsampled sources, the statistics epilogue, workspaces sized for max_batch.

    sources: one or two dicts {"x": (B,s,s,s,C) with s = S, or S/2 with "up": 1; "scale", "shift": (C,) or absent;
    "act": 0/1/2}.  The last of two sources may be a condition, {"x": (B, ncond), "bcast": ncond, "C": channels it stands
    for}: spatially constant, channel c = x[b][c % ncond] (K.tile), built as the VAE's e0 -- folded where the engine folds
    it; its entry of dx is None.  w (k,k,k,Cin,Cout) with Cin the sum of the sources' C.  dout (B,S,S,S,Cout): gradient w.r.t. the
    layer's output (post_act(BN(y)), or y without BatchNorm); None runs the forward pass only.

    Returns a dict: y; with has_bn mean, rstd, scale, shift, moving_mean, moving_var, rows_per_block, blocks; with dout
    dw, dbias, (dgamma, dbeta), dx (a list, one array per source, shaped as its x); and kernels: {"fwd": [...],
    "dgrad": [...], "wgrad": [...]} -- "<launch site>|<kernel template instantiation>" of every conv launch -- and
    "pool": the profiler row of the up-split backward's pooling of dy, "pool125:<layer>", "pool8:<layer>" or "pool27:<layer>".

    ranks = R in 1..4: R emulated data-parallel ranks with SyncBN (ics_conv_layer.ranks).  The sources' x and dout hold
    R * B samples, rank-major, and so do y and dx; the statistics, the moving statistics and the parameter gradients
    (each rank's local sums) get a leading (R,), and kernels becomes a list of R such dicts."""
    lib = L.load()
    op = _OpArgs(ranks)
    f, out, lead, R = op.f, op.out, op.lead, op.R
    a = L.ConvLayerArgs()
    a.ranks = R
    w = _f32(w)
    taps, Cout = w.shape[0] ** 3, w.shape[4]
    srcs = [dict(s) for s in sources]
    x0 = _f32(srcs[0]["x"])
    NB = x0.shape[0]                              # samples in the tensors
    B = op.shard(NB)
    S = x0.shape[1] * (2 if srcs[0].get("up") else 1)
    if sum(int(s["C"]) if s.get("bcast") else _f32(s["x"]).shape[4] for s in srcs) != w.shape[3]:
        raise ValueError("the sources' channels do not add up to the kernel's Cin")
    a.B, a.max_batch, a.S, a.taps, a.Cout = B, int(max_batch or B), S, taps, Cout
    a.pre_act, a.has_bn, a.post_act, a.pad_input, a.nsrc = int(pre_act), int(bool(has_bn)), int(post_act), int(bool(pad_input)), len(srcs)
    dxs = []
    for i, s in enumerate(srcs):
        x = _f32(s["x"])
        up = 1 if s.get("up") else 0
        bcast = int(s.get("bcast", 0))
        if bcast:
            if x.shape != (NB, bcast):
                raise ValueError("source %d has shape %s, a bcast source is (B, bcast)" % (i, x.shape))
        elif x.shape[:4] != (NB,) + (S // 2 if up else S,) * 3:
            raise ValueError("source %d has shape %s" % (i, x.shape))
        a.src[i].x, a.src[i].scale, a.src[i].shift = f(x), f(s.get("scale")), f(s.get("shift"))
        a.src[i].C, a.src[i].up, a.src[i].act = int(s["C"]) if bcast else x.shape[4], up, int(s.get("act", 0))
        a.src[i].bcast = bcast
        if bcast:
            dxs.append(None)           # the engines never differentiate with respect to the condition
        elif dout is not None and want_dx:
            dxs.append(out(x.shape))
            a.src[i].dx = L.fptr(dxs[-1])
    a.w, a.bias, a.gamma, a.beta, a.dout = f(w), f(bias), f(gamma), f(beta), f(dout)
    r = {"y": out((NB, S, S, S, Cout))}
    a.y = L.fptr(r["y"])
    if has_bn:
        for k in ("mean", "rstd", "scale", "shift", "moving_mean", "moving_var"):
            r[k] = out(lead + (Cout,))
            setattr(a, k, L.fptr(r[k]))
    if dout is not None:
        r["dw"], r["dbias"] = out(lead + w.shape), out(lead + (Cout,))
        a.dw, a.dbias = L.fptr(r["dw"]), L.fptr(r["dbias"])
        if has_bn:
            r["dgamma"], r["dbeta"] = out(lead + (Cout,)), out(lead + (Cout,))
            a.dgamma, a.dbeta = L.fptr(r["dgamma"]), L.fptr(r["dbeta"])
        r["dx"] = dxs
    a.kernels, a.kernels_cap = op.text(16384)
    L.check(lib.ics_op_conv_layer(C.byref(a)))
    if has_bn:
        r["rows_per_block"], r["blocks"] = a.rows_per_block, a.blocks

    def kernels(lines):
        d = {k: [ln for ln in lines if ln.startswith("conv_%s:" % k)] for k in ("fwd", "dgrad", "wgrad")}
        d["pool"] = [ln for ln in lines if ln.startswith(("pool125:", "pool8:", "pool27:"))]   # the up-split backward's pooling of dy
        return d

    ks = [kernels(lines) for lines in op.lines()]
    r["kernels"] = ks if R else ks[0]
    return r


LINKS = ("same", "up", "pool", "pool_skip")
METRIC_SUM_KEYS = ("sum_lsoft", "sum_lsig", "tp", "predicted", "wr_tp", "wr_possible", "voxels")


def conv_link(link, x0, layers, dout, form="unet", q=None, dout_l=None, pool_ties_all=True, max_batch=None, ranks=0):
    """Single-op entry (ics_op_conv_link): a producer P and its consumer(s) through the engines' own construction,
    forward (training) and backward calls, with the gradient sources and `next` unet_backward gives that link.

    link: one of LINKS.  x0 (B,S,S,S,C0).  layers: {"P": {...}, "K": {...}, "L": {...}} (K behind the MaxPool; L the
    same-resolution / upsampled / [P | up(q)] consumer), each {"w": (3,3,3,Cin,Cout), "bias", "gamma", "beta"}.
    dout: gradient w.r.t. the output of L ("same", "up") or K ("pool", "pool_skip"); dout_l and q: "pool_skip" only.

    Returns {"P": {...}, "K": {...}, "L": {...}} with y, mean, rstd, scale, shift, dw, dbias, dgamma, dbeta per layer,
    plus pooled (pool links), dy_p, dx0 and sites: the profiler's rows in launch order ("<site>" or "<site>|<kernel>").

    ranks = R in 1..4: R emulated data-parallel ranks with SyncBN (ics_conv_link.ranks): x0, q, dout, dout_l, y, pooled,
    dy_p and dx0 hold R * B samples, rank-major; the statistics and the parameter gradients (local sums) get a leading
    (R,); sites becomes a list of R lists."""
    lib = L.load()
    op = _OpArgs(ranks)
    f, out, lead, R = op.f, op.out, op.lead, op.R
    a = L.ConvLinkArgs()
    a.ranks = R
    x0 = _f32(x0)
    NB, S, C0 = x0.shape[0], x0.shape[1], x0.shape[4]
    B = op.shard(NB)
    a.link, a.form = LINKS.index(link), {"unet": 0, "vae": 1}[form]
    a.B, a.max_batch, a.S, a.C0 = B, int(max_batch or B), S, C0
    a.pool_ties_all = int(bool(pool_ties_all))
    a.x0, a.q, a.dout, a.dout_l = f(x0), f(q), f(dout), f(dout_l)
    a.Cq = 0 if q is None else _f32(q).shape[4]
    side = {"P": S, "K": S // 2, "L": 2 * S if link == "up" else S}
    r = {}
    for name, p in layers.items():
        h = getattr(a, name)
        w = _f32(p["w"])
        Cout = w.shape[4]
        h.Cout, h.w, h.bias, h.gamma, h.beta = Cout, f(w), f(p.get("bias")), f(p["gamma"]), f(p["beta"])
        o = r[name] = {"y": out((NB,) + (side[name],) * 3 + (Cout,)), "dw": out(lead + w.shape)}
        for k in ("mean", "rstd", "scale", "shift", "dbias", "dgamma", "dbeta"):
            o[k] = out(lead + (Cout,))
        for k, v in o.items():
            setattr(h, k, L.fptr(v))
    Cp = r["P"]["y"].shape[4]
    if "K" in layers:
        r["pooled"] = out((NB,) + (S // 2,) * 3 + (Cp,))
        a.pooled = L.fptr(r["pooled"])
    r["dy_p"], r["dx0"] = out((NB, S, S, S, Cp)), out(x0.shape)
    a.dy_p, a.dx0 = L.fptr(r["dy_p"]), L.fptr(r["dx0"])
    a.sites, a.sites_cap = op.text(32768)
    L.check(lib.ics_op_conv_link(C.byref(a)))
    r["sites"] = op.lines() if R else op.lines()[0]
    return r


def head_link(x0, P, head, labels, loss_weight=0.0, class_weights=None, bce_from_logits=False, want_grad=True,
              max_batch=None, ranks=0):
    """Single-op entry (ics_op_head_link): the U-Net's last link, a producer P in c18's place (Conv 3x3x3 C0 -> 128, ReLU,
    BatchNorm) and the 1x1x1 head with its losses, forward (training) and backward through the engine's own functions.

    x0 (B,S,S,S,C0); P {"w": (3,3,3,C0,128), "bias", "gamma", "beta"}; head {"wsoft": (128, ncls), "bsoft": (ncls,),
    "wsig": (128,), "bsig": (1,)}; labels uint8 (B,S,S,S), each < ncls.  loss_weight <= 0: ncls; class_weights (ncls,): a
    table in place of the scalar.

    Returns a dict: y, mean, rstd, scale, shift (P); metrics (5,), sums (dict of METRIC_SUM_KEYS); with want_grad dz
    (B,S,S,S,ncls+1), dwsoft, dwsig, dbias_head (ncls+1,), dw, dbias, dgamma, dbeta (P), dy_p, dx0, dy_in_place; and sites,
    the profiler's rows in launch order.

    ranks = R in 1..4: R emulated data-parallel ranks with SyncBN (ics_head_link.ranks): x0, labels, y, dz, dy_p and dx0
    hold R * B samples, rank-major; every other output gets a leading (R,) -- metrics and sums are each rank's local ones,
    sums a list of R dicts -- and sites becomes a list of R lists."""
    lib = L.load()
    op = _OpArgs(ranks)
    f, out, lead, R = op.f, op.out, op.lead, op.R
    a = L.HeadLinkArgs()
    a.ranks = R
    x0 = _f32(x0)
    NB, S, C0 = x0.shape[0], x0.shape[1], x0.shape[4]
    B = op.shard(NB)
    wsoft = _f32(head["wsoft"])
    ncls = wsoft.shape[1]
    w = _f32(P["w"])
    if w.shape != (3, 3, 3, C0, 128) or wsoft.shape[0] != 128:
        raise ValueError("head_link: P is (3,3,3,C0,128) and wsoft (128, ncls)")
    lab = np.ascontiguousarray(labels, dtype=np.uint8).reshape(NB, S, S, S)
    op.keep.append(lab)
    a.B, a.max_batch, a.S, a.C0, a.ncls = B, int(max_batch or B), S, C0, ncls
    a.x0, a.w, a.bias, a.gamma, a.beta = f(x0), f(w), f(P.get("bias")), f(P["gamma"]), f(P["beta"])
    a.wsoft, a.bsoft, a.wsig, a.bsig = f(wsoft), f(np.reshape(head["bsoft"], ncls)), f(np.reshape(head["wsig"], 128)), f(np.reshape(head["bsig"], 1))
    a.labels = L.u8ptr(lab)
    a.loss_weight, a.bce_from_logits, a.want_grad = float(loss_weight), int(bool(bce_from_logits)), int(bool(want_grad))
    if class_weights is not None:
        cw = np.ascontiguousarray(class_weights, np.float32).reshape(-1)
        if cw.size != ncls:
            raise ValueError("class_weights must have %d entries, got %d" % (ncls, cw.size))
        a.class_weights = f(cw)
    r = {"y": out((NB, S, S, S, 128)), "metrics": out(lead + (5,))}
    for k in ("mean", "rstd", "scale", "shift"):
        r[k] = out(lead + (128,))
    if want_grad:
        r.update(dz=out((NB, S, S, S, ncls + 1)), dwsoft=out(lead + (128, ncls)), dwsig=out(lead + (128,)),
                 dbias_head=out(lead + (ncls + 1,)), dw=out(lead + w.shape), dy_p=out((NB, S, S, S, 128)), dx0=out(x0.shape))
        for k in ("dbias", "dgamma", "dbeta"):
            r[k] = out(lead + (128,))
    for k, v in r.items():
        setattr(a, k, L.fptr(v))
    sums = np.zeros(lead + (7,), np.float64)
    a.sums = L.f64ptr(sums)
    a.sites, a.sites_cap = op.text(32768)
    L.check(lib.ics_op_head_link(C.byref(a)))
    r["sites"] = op.lines() if R else op.lines()[0]
    sd = [dict(zip(METRIC_SUM_KEYS, [float(v) for v in row])) for row in sums.reshape(-1, 7)]
    r["sums"] = sd if R else sd[0]
    r["dy_in_place"] = bool(a.dy_in_place)
    return r


def unet_metrics_from_sums(sums):
    """Single-op entry (ics_op_unet_metrics_from_sums): [Loss, lsoft, lsig, f1, wr] from the seven sums unet_head returns
    (a dict, or 7 numbers in its key order), e.g. added over the shards of a global batch."""
    lib = L.load()
    if isinstance(sums, dict):
        sums = [sums[k] for k in METRIC_SUM_KEYS]
    s = (C.c_double * 7)(*[float(v) for v in sums])
    m = np.zeros(5, np.float32)
    L.check(lib.ics_op_unet_metrics_from_sums(s, L.fptr(m)))
    return m


def vae_loss(mulv=None, mse_partial=(), n_elems=1.0, pm_partials=((), (), (), ()), pm_per=(1.0,) * 4, pm_w=(1.0,) * 4,
             alpha=0.5, beta=3e-4, phase=0, sums=None):
    """Single-op entry (ics_op_vae_loss): the DFC-VAE's loss assembly on given partial sums.  mulv (B, 2 * latent);
    mse_partial: partial sums of the squared error over n_elems elements; pm_partials: four arrays of partial sums, one per
    perceptual tap, with pm_per elements per sample and the weights pm_w.  phase 0 -> metrics [Loss, PM, MSE, KLD];
    phase 1 -> sums (5,) float64 {KL, squared error, weighted PM, B, n_elems}; phase 2 (sums given) -> metrics."""
    lib = L.load()
    m = np.zeros(4, np.float32)
    s = (C.c_double * 5)(*([float(v) for v in sums] if sums is not None else [0.0] * 5))
    if phase == 2:
        L.check(lib.ics_op_vae_loss(None, 0, 0, None, 0, 0.0, None, None, None, None, float(alpha), float(beta), 2, s, L.fptr(m)))
        return m
    mulv = _f32(mulv)
    B, latent = mulv.shape[0], mulv.shape[1] // 2
    mse = np.ascontiguousarray(mse_partial, np.float64).reshape(-1)
    pm = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in pm_partials]), np.float64)
    n = (C.c_int * 4)(*[int(np.asarray(p).size) for p in pm_partials])
    per = (C.c_double * 4)(*[float(v) for v in pm_per])
    w = np.ascontiguousarray(pm_w, np.float32)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None
    L.check(lib.ics_op_vae_loss(L.fptr(mulv), B, latent, dp(mse), int(mse.size), float(n_elems), dp(pm), n, per, L.fptr(w),
                                float(alpha), float(beta), int(phase), s, L.fptr(m)))
    return np.array(list(s), np.float64) if phase == 1 else m


def vae_latent(h, w_mean, w_lv, b_mean, b_lv, eps, cond, dzc=None, beta=3e-4, max_batch=None):
    """Single-op entry (ics_op_vae_latent): the DFC-VAE's latent link -- the z_mean | z_log_var GEMM, sampling and, with
    dzc (B, latent + ncond) = dLoss/d[z | cond], their backward pass with the KL gradient at weight beta.
    h, eps (B, latent); w_mean, w_lv (latent, latent); b_mean, b_lv (latent,); cond (B, ncond).
    Returns a dict: mulv (B, 2 latent), z, zc; with dzc also dmulv, dw_mean, dw_lv, dbias (2 latent,), dh."""
    lib = L.load()
    h, w_mean, w_lv, eps, cond = _f32(h), _f32(w_mean), _f32(w_lv), _f32(eps), _f32(cond)
    B, lat = h.shape
    nc = cond.shape[1]
    if w_mean.shape != (lat, lat) or w_lv.shape != (lat, lat) or eps.shape != (B, lat) or cond.shape[0] != B:
        raise ValueError("vae_latent: shapes do not fit h %s" % (h.shape,))
    a = L.VaeLatentArgs()
    a.B, a.max_batch, a.latent, a.ncond, a.beta = B, int(max_batch or B), lat, nc, float(beta)
    keep = [_f32(v).reshape(lat) for v in (b_mean, b_lv)]
    a.h, a.w_mean, a.w_lv, a.eps, a.cond = L.fptr(h), L.fptr(w_mean), L.fptr(w_lv), L.fptr(eps), L.fptr(cond)
    a.b_mean, a.b_lv = L.fptr(keep[0]), L.fptr(keep[1])
    r = {"mulv": np.empty((B, 2 * lat), np.float32), "z": np.empty((B, lat), np.float32),
         "zc": np.empty((B, lat + nc), np.float32)}
    if dzc is not None:
        dzc = _f32(dzc)
        if dzc.shape != (B, lat + nc):
            raise ValueError("vae_latent: dzc has shape %s" % (dzc.shape,))
        a.dzc = L.fptr(dzc)
        r.update(dmulv=np.empty((B, 2 * lat), np.float32), dw_mean=np.empty((lat, lat), np.float32),
                 dw_lv=np.empty((lat, lat), np.float32), dbias=np.empty(2 * lat, np.float32), dh=np.empty((B, lat), np.float32))
    for k, v in r.items():
        setattr(a, k, L.fptr(v))
    L.check(lib.ics_op_vae_latent(C.byref(a)))
    return r


def sqdiff(a, b, blocks_per_sample, coef=0.0, grad=False, accumulate_into=None):
    """Single-op entry (ics_op_sqdiff): per-sample partial sums of (a - b)^2, a and b (B, per_sample), as the VAE step takes
    them for its squared error and perceptual terms.  Returns (partial (B, blocks_per_sample) float64, grad or None);
    grad = coef * (b - a) (grad=True), added to accumulate_into (B, per_sample) where that is given."""
    lib = L.load()
    a, b = _f32(a), _f32(b)
    B, per = a.shape
    if b.shape != a.shape:
        raise ValueError("sqdiff: a and b differ in shape")
    part = np.empty((B, int(blocks_per_sample)), np.float64)
    g = None
    if accumulate_into is not None:
        g = np.array(accumulate_into, np.float32, order="C").reshape(B, per)
    elif grad:
        g = np.empty((B, per), np.float32)
    L.check(lib.ics_op_sqdiff(L.fptr(a), L.fptr(b), B, per, int(blocks_per_sample), float(coef),
                              1 if accumulate_into is not None else 0, L.fptr(g), L.f64ptr(part)))
    return part, g


def up125_pool(dy, variant=1):
    """Single-op entry (ics_op_up125_pool): the pooling pass of the 125-product up-split backward alone.  dy (B,S,S,S,N)
    float32; variant 0: one wave per z type, 1: one wave per fine plane.  Returns the 125 blocks of every 4x4x4 tile as
    one flat float32 array of 125 * B (S/4)^3 * N elements in the class-major layout of csrc/up125.h."""
    lib = L.load()
    dy = _f32(dy)
    if dy.ndim != 5 or dy.shape[1] != dy.shape[2] or dy.shape[1] != dy.shape[3]:
        raise ValueError("up125_pool: dy must be (B, S, S, S, N), got %s" % (dy.shape,))
    B, S, N = dy.shape[0], dy.shape[1], dy.shape[4]
    out = np.empty(125 * B * (S // 4) ** 3 * N, np.float32)
    L.check(lib.ics_op_up125_pool(L.fptr(dy), B, S, N, int(variant), L.fptr(out)))
    return out


def unet_head(x, wsoft, bsoft, wsig, bsig, labels, mode=1, fused=True, loss_weight=0.0, bce_from_logits=False,
              class_weights=None):
    """Single-op entry (kernel parity tests): the heads + losses + metrics on a given trunk output x (M,128).
    class_weights (ncls,): a per-class table in place of the scalar loss_weight (ics_op_unet_head_weighted).
    Returns (out (M, ncls+1) | None, metrics (5,), sums dict) -- see ics_op_unet_head."""
    lib = L.load()
    x, wsoft, bsoft, wsig, bsig = _f32(x), _f32(wsoft), _f32(bsoft), _f32(wsig), _f32(bsig)
    M, ncls = x.shape[0], wsoft.shape[1]
    lab = np.ascontiguousarray(labels, dtype=np.uint8).reshape(M)
    out = np.empty((M, ncls + 1), np.float32) if mode != 1 else None
    m = np.zeros(5, np.float32)
    s = (C.c_double * 7)()
    args = (L.fptr(x), L.fptr(wsoft), L.fptr(bsoft), L.fptr(wsig), L.fptr(bsig), L.u8ptr(lab), M, ncls, float(loss_weight),
            int(mode) | (4 if bce_from_logits else 0), 1 if fused else 0, L.fptr(out), L.fptr(m), s)
    if class_weights is None:
        L.check(lib.ics_op_unet_head(*args))
    else:
        cw = np.ascontiguousarray(class_weights, np.float32).reshape(-1)
        if cw.size != ncls:
            raise ValueError("class_weights must have %d entries, got %d" % (ncls, cw.size))
        L.check(lib.ics_op_unet_head_weighted(*args, L.fptr(cw)))
    return out, m, dict(zip(METRIC_SUM_KEYS, [float(v) for v in s]))


def conv3d_backward(x, w, dy):
    lib = L.load()
    x, w, dy = _f32(x), _f32(w), _f32(dy)
    B, S, Cin = x.shape[0], x.shape[1], x.shape[4]
    taps, Cout = w.shape[0] ** 3, w.shape[4]
    dx = np.empty_like(x)
    dw = np.empty_like(w)
    L.check(lib.ics_op_conv3d_backward(L.fptr(x), L.fptr(w), L.fptr(dy), B, S, Cin, Cout, taps, L.fptr(dx), L.fptr(dw)))
    return dx, dw
