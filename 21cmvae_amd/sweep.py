"""Hyper-parameter sweeps: several models of the same depth trained in lock step on one
shared batch stream (BASELINE configs[4]: "64 concurrent latent-dim/hidden-width configs
packed as batched GEMM", 8 per GPU).

The reference has no sweep code: it trains one model per ``fit`` call
(emulator.py:369-378, :739-747) and its hyper-parameter tuner is not shipped.  ``fit_models``
runs exactly that ``fit`` for every model -- same shuffle, same batches, same Keras
bookkeeping, per-model optimizer/callbacks/History -- but issues each phase of the step
(layer k forward, loss, layer k backward, Adam) as ONE grouped device launch for all models
(include/v21.h: v21_sweep_*).  Models that stop early (``model.stop_training``) drop out of
the group; the others continue.
"""
import numpy as np

from . import _native, engine

MAX_GROUP = 64  # include/v21.h: v21_sweep_create (r5: 64 = the whole of BASELINE configs[4] in one group; 16 until r4)


def fit_models(models, x, y, batch_size=256, epochs=1, validation_data=None, callbacks=None, shuffle=True,
               verbose=0, validation_batch_size=None):
    """Train ``models`` (compiled ``engine.Model`` objects of equal depth, activations and
    in/out width) on the same data.  ``callbacks``: None or one list per model.  Returns one
    ``History`` per model."""
    models = list(models)
    if not models:
        return []
    if len(models) > MAX_GROUP:
        raise ValueError("at most %d models per sweep group (run several groups, e.g. one per GPU)" % MAX_GROUP)
    callbacks = callbacks or [[] for _ in models]
    if len(callbacks) != len(models):
        raise ValueError("callbacks: one list per model")
    batch_size = int(batch_size)
    x, y, targets = engine._f32_pair(x, y, alias_ok=True)
    n = x.shape[0]
    for m in models:
        engine._check_compiled(m)
        if not m.built:
            m.build((None, x.shape[-1]))
    trainers = [m._ensure_trainer(batch_size) for m in models]
    rw = models[0]._row_weight(y)
    for m in models[1:]:
        if not np.array_equal(m._row_weight(y), rw):
            raise ValueError("all models of a sweep must be compiled with the same loss")
    vb = None
    if validation_data is not None:
        vb = int(validation_batch_size or batch_size)
        xv, yv, targets_v = engine._f32_pair(validation_data[0], validation_data[1])
        rwv = models[0]._row_weight(yv)
        for tr in trainers:
            tr.set_data(1, xv, targets_v, rwv)
    runs = [engine._Run(m, tr, c, epochs, n, batch_size, verbose) for m, tr, c in zip(models, trainers, callbacks)]
    engine._Run.begin(runs)
    active = list(range(len(models)))
    holder, group = None, None
    for epoch in range(epochs):
        if not active:
            break
        if holder != active[0]:  # the first active trainer holds the training set of the group
            holder = active[0]
            trainers[holder].set_data(0, x, targets, rw)
            group = None
        if group is None:
            group = _native.Sweep([trainers[i] for i in active])
        for i in active:
            runs[i].epoch_begin(epoch)
        perm = engine._rng.permutation(n).astype(np.int32) if shuffle else None
        losses = group.run_epoch(perm, batch_size)
        still = []
        for i, loss in zip(active, losses):
            if runs[i].epoch_end(epoch, loss, vb, "model %d - epoch %d/%d - " % (i, epoch + 1, epochs)):
                still.append(i)
        if still != active:
            active, group = still, None
    for r in runs:
        r.finish()
    return [r.history for r in runs]
