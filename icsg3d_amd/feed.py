"""Fed training loops: a generator's batches go into pinned staging slots as RAW arrays (file payloads, or a generator's
float64 X and one-hot y), a copy stream uploads them while the previous step runs, and the pack kernel does the cast, the
(M | p) concatenate and the label conversion on the device (include/icsg3d.h "fed steps", csrc/feed.h).

`pack_reference` is the numpy statement of the pack kernel.  `Feeder` turns any generator into fed steps and yields the
per-step metric lists the synchronous loops produce, bit for bit.
"""
from __future__ import annotations

import contextlib
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .engine import FEED_DTYPES


def pack_reference(x_parts, labels=None, label_kind="none", rotations=None):
    """What the pack kernel computes, in numpy: x = concatenate(astype(float32)) over the parts' channels; labels =
    argmax over the columns of a one-hot (the lowest index among equal maxima), else astype(uint8) of the ids.
    rotations (B,3): sample b of every per-voxel array goes through the table rotations[b] first (augment.rotate_host).
    Returns (x float32 (B,d,d,d,C), labels uint8 (B,d,d,d) | None)."""
    if rotations is not None:
        from .augment import rotate_host
        turn = lambda a: np.stack([rotate_host(s, r) for s, r in zip(np.asarray(a), np.asarray(rotations))])
        x_parts = [turn(p) for p in x_parts]
        labels = None if labels is None else turn(labels)
    x = np.concatenate([np.asarray(p).astype(np.float32) for p in x_parts], axis=-1)
    if label_kind == "none" or labels is None:
        return x, None
    labels = np.asarray(labels)
    if label_kind == "onehot":
        return x, np.argmax(labels, axis=-1).astype(np.uint8)
    return x, labels.astype(np.uint8)


def _x_dtype(dtype):
    """the dtype an x array travels in: its own when the pack kernel reads it, float32 (a host cast) otherwise"""
    dtype = np.dtype(dtype)
    return dtype if dtype in FEED_DTYPES else np.dtype(np.float32)


def _label_kind(y, num_classes):
    """label kind of a generator's y (the rules of unet._to_labels) and the array that travels: a float32 one-hot as it
    is (the device takes the argmax), any other one-hot or soft y as the uint8 argmax of its own values (taken on the
    host, so that two doubles which round to one float still compare as doubles), ids with a trailing unit axis dropped"""
    y = np.asarray(y)
    if y.ndim == 5 and y.shape[-1] == num_classes:
        if y.dtype == np.float32:
            return "onehot", y
        return "u8", np.argmax(y, axis=-1).astype(np.uint8)
    if y.ndim == 5 and y.shape[-1] == 1:
        y = y[..., 0]
    return {np.dtype(np.uint8): "u8", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}.get(y.dtype, "u8"), y


class Feeder:
    """Fed steps over `gen` on `engine` (a UnetEngine or a VaeEngine).

    Iterating runs one epoch: `for metrics in Feeder(engine, gen)` yields one list of floats per batch, in order.
    training=False runs test steps.  eps(n) draws the VAE's sampling noise for a batch of n; it is called once per step,
    in step order, on the calling thread.  steps: batches per epoch when that is not len(gen).

    A generator that offers `feed_spec()` and `fill(index, views, map)` writes raw file payloads straight into the slot
    (`map` runs the per-sample copies on `workers` threads: disjoint rows of one slot).  Any other generator has `gen[i]`
    copied into the views -- X in its own dtype when that is float32 / float64, a float32 one-hot y as it is -- without a
    host cast.  When such a generator also offers `rotations(index)`, the batch's rotation table (B,3) goes to
    `feed_submit` and the pack kernel rotates the raw payloads; for any other generator nothing is passed.

    Schedule: batch k+1 is filled and submitted right after step k was enqueued, and step k's metrics are read after
    step k+1 was enqueued, so the device always has a step queued while the host loads.  A slot is rewritten only after
    `feed_slot` returned it, is stepped exactly once per submit, and every ticket is read exactly once.

    close=True closes the feed when the epoch ends; close=False leaves it open for the next Feeder on the same engine,
    which reuses it when its layout is the same (the class-level loops keep one feed over all epochs and both
    generators).  An exception (of the generator, say) always closes it and is re-raised.  grow(batch) returns an engine
    that takes `batch` samples, for a generator whose batches outgrow `engine.max_batch`; the steps in flight are read
    first and the feed is opened again on the engine it returns (`self.engine` afterwards).  watch() returns a context
    manager put around every engine call that can wait for the device (the data-parallel watchdog)."""

    def __init__(self, engine, gen, workers=4, slots=2, training=True, eps=None, steps=None, close=True, grow=None,
                 watch=None):
        self.engine, self.gen, self.workers, self.slots, self.training = engine, gen, int(workers), int(slots), training
        self.is_vae = hasattr(engine, "latent_dim")
        self.eps = eps if eps is not None else (lambda n: np.random.normal(size=(n, self.engine.latent_dim)))
        self.steps = len(gen) if steps is None else int(steps)
        self.close, self.grow, self.watch = close, grow, watch or contextlib.nullcontext

    def __len__(self):
        return self.steps

    def _spec_of(self, item):
        """what travels, from a generator's batch"""
        X, y = np.asarray(item[0]), item[1]
        if self.is_vae:
            return (X.shape[-1],), (_x_dtype(X.dtype),), "none"
        y = y[0] if isinstance(y, (list, tuple)) else y
        return (X.shape[-1],), (_x_dtype(X.dtype),), _label_kind(y, self.engine.num_classes)[0]

    def _open(self, spec):
        """the engine's feed with this layout: the open one when it has it, a new one otherwise"""
        eng = self.engine
        want = (tuple(int(c) for c in spec[0]), tuple(np.dtype(t) for t in spec[1]), spec[2], self.slots)
        have = getattr(eng, "_feed", None)
        if have == want:
            return
        if have is not None:
            eng.feed_close()
        eng.feed_open(want[0], want[1], want[2], self.slots)

    def _fill(self, index, views, item, pool_map):
        """batch `index` into `views`; returns its size"""
        if item is None:
            B = self.gen.fill(index, views, pool_map)
        else:
            X, y = item
            X = np.asarray(X)
            B = len(X)
            y = y[0] if isinstance(y, (list, tuple)) else y
            y = np.asarray(y) if self.is_vae else _label_kind(y, self.engine.num_classes)[1]
            dst = views["cond"] if self.is_vae else views["labels"]

            def one(i):                                   # a sample per call: a one-hot y is 12 MB of it at d = 32
                np.copyto(views["x"][0][i], X[i], casting="unsafe")
                np.copyto(dst[i], y[i], casting="unsafe")
            pool_map(one, range(B))
        if self.is_vae:
            np.copyto(views["eps"][:B], np.asarray(self.eps(B)), casting="unsafe")
        return B

    def __iter__(self):
        n = self.steps
        if n <= 0:
            return
        gen = self.gen
        spec = gen.feed_spec() if hasattr(gen, "fill") and hasattr(gen, "feed_spec") else None
        raw = spec is not None
        items = None
        if not raw:                                       # gen[i] on loader threads, in order, a few batches ahead
            from .prefetch import prefetched

            class _Seq:
                def __len__(self):
                    return n

                def __getitem__(self, i):
                    return gen[i]
            items = iter(prefetched(_Seq(), self.workers, self.slots + 1))

        def fetch():
            """the next batch of a generator without fill (None with one) and its size, when that is known beforehand"""
            if raw:
                return None, int(getattr(gen, "batch_size", 0))
            item = next(items)
            return item, len(item[0])

        def read(ticket):
            with self.watch():
                return [float(v) for v in self.engine.feed_metrics(ticket)]

        item, B = fetch()
        if not raw:
            spec = self._spec_of(item)
        if self.grow is not None and B > self.engine.max_batch:
            self.engine = self.grow(B)
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="icsg3d-feed") if self.workers > 1 else None
        pool_map = (lambda f, it: list(pool.map(f, it))) if pool else (lambda f, it: [f(i) for i in it])
        opened = False
        try:
            self._open(spec)
            opened = True
            pending = deque()

            def load(k, item):
                slot = k % self.slots
                with self.watch():
                    views = self.engine.feed_slot(slot)   # returns once the slot's last upload has left the pinned memory
                B = self._fill(k, views, item, pool_map)
                rot = gen.rotations(k) if item is None and hasattr(gen, "rotations") else None
                if rot is None:
                    self.engine.feed_submit(slot, B)
                else:
                    self.engine.feed_submit(slot, B, rot)
                return slot

            slot = load(0, item)
            for k in range(n):
                with self.watch():
                    pending.append((self.engine.train_step_fed if self.training else self.engine.test_step_fed)(slot))
                if k + 1 < n:
                    item, B = fetch()
                    if self.grow is not None and B > self.engine.max_batch:
                        while pending:                    # a larger batch than the engine holds: read what is in flight,
                            yield read(pending.popleft())  # then go on with the engine grow() returns
                        self.engine.feed_close()
                        opened = False
                        self.engine = self.grow(B)
                        self._open(spec)
                        opened = True
                    slot = load(k + 1, item)              # host work and upload overlap step k on the device
                while len(pending) > 1:
                    yield read(pending.popleft())
            while pending:
                yield read(pending.popleft())
        except BaseException:
            if opened:
                opened = False
                self.engine.feed_close()
            raise
        finally:
            if items is not None:
                items.close()                             # stops the loader threads
            if pool:
                pool.shutdown(wait=True)
            if opened and self.close:
                self.engine.feed_close()
