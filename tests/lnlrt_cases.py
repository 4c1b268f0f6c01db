"""The cases of tests/test_lnlrt_cpu.py and tests/test_lnlrt_gpu.py: the ln L variant of fused_fwd<ArchRT, Prec> instantiated
at run time (csrc/jit.hip: kJitLnl) on small stacks, their row counts, records, refusals, and lnl_ref's
mutation catalogue restated for any output width.  Needs no GPU.

Stacks (weights as jacrt_cases.stack builds them: act_ref.stack_weights / shape_cases.make_stack):
    R0  5-20          lin                one layer, one output tile: the d / w load and the butterfly with no hidden layer
    R1  5-40-72-37    relu relu lin      two output tiles, the last with 5 live bins -- or, in the parity record, dead
    R2  1-20-3        relu lin           in_dim 1, 3 live bins
    R3b 7-64-9-40-48  relu LIN relu lin  a linear hidden layer
    R5  15-40-65      relu lin           in_dim > 8: rows on u only; three tiles, the last with ONE live bin
    T1, T2  5-40-72-37  tanh sigmoid / elu softplus, two units per hidden layer at bias +-90
    NB  7-64-128-451  relu relu lin      15 tiles: the sample notebook's stack

Rows: a wave of the ln L family takes 32 rows, a workgroup 128 (csrc/routes.h: kLnlWgRows)."""
import numpy as np

import act_ref as ar
import jacrt_cases as jc
import lnl_ref as lr
import shape_cases as sc

ROWS = (1, 31, 32, 33, 127, 128, 129, 257)
PRECS = ("f32", "f16", "bf16")
NB = ([7, 64, 128, 451], [1, 1, 0])
CASES = {k: jc.CASES[k] for k in ("R0", "R1", "R2", "R3b", "R5", "T1", "T2")}
CASES["NB"] = NB
SPILLS = jc.SPILLS
# (dims, act, the reason jit_lnl_eligible gives)
REFUSALS = {k: jc.REFUSALS[k] for k in ("i8relu", "i5gauss", "i5lin1", "R3", "too_wide")}
TILE = 32


def stack(name):
    """-> dict dims, act, Ws, bs, flat, tin (None above 8 inputs), tout; cached, never modified"""
    return sc.make_stack(*NB) if name == "NB" else jc.stack(name)


def calls(name):
    """(n, input transform on, output transform on, rows in their dtype) for every n of ROWS: the transforms alternate as
    jacrt_cases.calls alternates them (R5 has no input transform), float64 and float32 rows"""
    dims = stack(name)["dims"]
    for k, n in enumerate(ROWS):
        tin_on = sc.has_tin(dims) and k % 2 == 0
        dtype = np.float64 if k % 4 < 2 else np.float32
        x = sc.rows(dims, n, 10 + k) if tin_on else sc.rows_u(dims, n, 10 + k)
        yield n, tin_on, k % 3 != 0, x.astype(dtype)


def forward64(rec, x, tin_on, tout_on):
    """float64 outputs of raw (tin_on) or transformed rows, in mK with the output transform"""
    y = ar.forward(rec["Ws"], rec["bs"], rec["act"], jc.transformed(rec, x, tin_on))
    return y * float(rec["tout"][0]) + np.asarray(rec["tout"][1], np.float64) if tout_on else y


def weights(name, dead_tile=True):
    """1 / sigma^2 per bin: shape_cases.weights (scattered zeros, about one bin in six; NB: the run 32 .. 95 too) with a
    dead run INSIDE a tile (bins 8 .. 13, where the stack has 16 bins), the last bin live -- R5's last tile holds that one
    bin -- and, with dead_tile, R1's whole last tile (bins 32 .. 36) dead"""
    dout = CASES[name][0][-1]
    w = sc.weights(dout, 5)
    live = float(w[w != 0][0])
    if dout >= 16:
        w[8:14] = 0.0
    w[dout - 1] = live
    if name == "R2":
        w[:] = [live, 0.64 * live, 0.36 * live]   # three live bins, unequal: a neighbour's weight is another weight
    if name == "R1" and dead_tile:
        w[32:] = 0.0
    return w.astype(np.float32)


def record(name, y_truth, std, seed, dead_tile=True):
    """(d, w) float32: d = y(truth) + lnl_ref.NOISE std noise, so that every live bin carries a term of comparable size and a
    dropped bin cannot hide; w of weights() in the units of y"""
    nb = np.shape(y_truth)[-1]
    d = (np.asarray(y_truth, np.float64) + lr.NOISE * std * np.random.default_rng(7000 + seed).normal(size=nb)).astype(np.float32)
    return d, (weights(name, dead_tile) / np.float32((std / sc.OUT_STD) ** 2)).astype(np.float32)


# ---- lnl_ref.MUTATIONS for any output width: name -> f(y (n, nb) float64, d, w, mean) -> the mutated float64 ln L (n,).
# "The tile" of drop_bin and tile_twice is the LAST output tile that holds a live bin (lnl_ref: tiles 7 and 5 of 15).
def _last_live_tile(w):
    k = int(np.flatnonzero(np.asarray(w) != 0)[-1])
    return k // TILE * TILE


def mut_drop_bin(y, d, w, mean):
    """one live bin's term dropped: the first live bin of the tile"""
    t = lr._terms(y, d, w)
    t0 = _last_live_tile(w)
    t[:, t0 + int(np.flatnonzero(np.asarray(w)[t0:t0 + TILE] != 0)[0])] = 0.0
    return -0.5 * t.sum(axis=-1)


def mut_pad_bins(y, d, w, mean):
    """the padding bins of the last tile included, with y = the mean of the output transform's mean, d = 0, the mean live weight"""
    w = np.asarray(w, np.float64)
    pad = (-w.size) % TILE
    assert pad > 0
    return -0.5 * (lr._terms(y, d, w).sum(axis=-1) + pad * w[w != 0].mean() * float(np.mean(mean)) ** 2)


def mut_tile_twice(y, d, w, mean):
    """the tile's terms counted twice"""
    t = lr._terms(y, d, w)
    t0 = _last_live_tile(w)
    return -0.5 * (t.sum(axis=-1) + t[:, t0:t0 + TILE].sum(axis=-1))


MUTATIONS = {"drop_bin": mut_drop_bin, "pad_bins": mut_pad_bins, "half_swap": lr.mut_half_swap, "tile_twice": mut_tile_twice,
             "neighbour_w": lr.mut_neighbour_w}


def mutation_effects(y, d, w, mean):
    """name -> the largest relative change of ln L over the rows"""
    ref = lr.lnl64(y, d, w)
    return {k: float(np.max(np.abs(f(np.asarray(y, np.float64), d, w, mean) - ref) / np.abs(ref))) for k, f in MUTATIONS.items()}
