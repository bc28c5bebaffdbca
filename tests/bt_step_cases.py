"""Inputs of the bookkeeping-step tests (tests/test_bt_step_gpu.py, tests/test_bt_step_ref_cpu.py):
per path S = 4 targets and 3 realized rows (the last step has none), built from named kinds.

Target kinds: `dir` Dirichlet; `neg` Dirichlet * 1.5 - 0.5 / N (negative entries, sum 1); `s13` a
Dirichlet * 1.3; `zeros` a Dirichlet with every third entry exactly 0; `onehot`; `plus` / `minus` a
Dirichlet scaled so that 1 + port = +1e-6 / -1e-6 on its row.
Row kinds: `benign` y ~ N(5e-4, 0.02); `wide` y ~ N(0, 0.5); `crash1` a wide row with one held asset
at y = -110 (R = 0); `crashall` every asset at -110; `nan` a benign row with one NaN; `ovf0` / `ovfpos`
a wide row with y = 89 (float32 exp overflows) on an asset of target 0 / of positive target; `near`
the all-negative row under a plus / minus target.

RECIPES: six paths. The first of each triple is benign, the other two are stress paths; the rows
that poison a path with NaN come last, so that the steps before them are measured.
"""
from __future__ import annotations

import numpy as np

import bt_step_ref as ref

S = 4
RECIPES = {
    "A0": [("dir", "benign"), ("dir", "wide"), ("dir", "benign"), ("dir", None)],
    "A1": [("neg", "wide"), ("s13", "crash1"), ("zeros", "nan"), ("onehot", None)],
    "A2": [("dir", "crashall"), ("plus", "near"), ("zeros", "ovf0"), ("dir", None)],
    "B0": [("dir", "benign"), ("onehot", "wide"), ("dir", "benign"), ("onehot", None)],
    "B1": [("zeros", "wide"), ("minus", "near"), ("dir", "ovfpos"), ("neg", None)],
    "B2": [("onehot", "wide"), ("neg", "crash1"), ("s13", "wide"), ("zeros", None)],
}
SCHEDULES = {"A": ("A0", "A1", "A2"), "B": ("B0", "B1", "B2")}
NAMES = tuple(RECIPES)


def _dirichlet(rng, N):
    return rng.dirichlet(np.ones(N)) if N > 1 else np.ones(1)


def _zeros(rng, N):
    t = _dirichlet(rng, N)
    t[1::3] = 0.0
    return t / t.sum()


def make_target(kind, rng, N, row):
    if kind == "dir":
        return _dirichlet(rng, N)
    if kind == "neg":
        return _dirichlet(rng, N) * 1.5 - 0.5 / N
    if kind == "s13":
        return _dirichlet(rng, N) * 1.3
    if kind == "zeros":
        return _zeros(rng, N)
    if kind == "onehot":
        t = np.zeros(N)
        t[rng.integers(N)] = 1.0
        return t
    if kind in ("plus", "minus"):
        t0 = _dirichlet(rng, N).astype(ref.LD)
        r32, _ = ref.f32_returns(row)
        want = ref.LD(-1) + (ref.LD(1e-6) if kind == "plus" else -ref.LD(1e-6))
        return (t0 * (want / np.sum(t0 * r32.astype(ref.LD)))).astype(np.float64)
    raise ValueError(kind)


def make_row(kind, rng, N):
    """The row and the asset it singles out (or -1); `ovf0` / `crash1` / `ovfpos` pick the asset
    once the target is known (fix_row)."""
    if kind is None:
        return None
    if kind in ("benign", "nan"):
        return rng.normal(5e-4, 0.02, N).astype(np.float32)
    if kind in ("wide", "crash1", "ovf0", "ovfpos"):
        return rng.normal(0.0, 0.5, N).astype(np.float32)
    if kind == "crashall":
        return np.full(N, -110.0, np.float32)
    if kind == "near":
        return (-np.abs(rng.normal(0.0, 0.5, N)) - 0.1).astype(np.float32)
    raise ValueError(kind)


def fix_row(kind, row, target, rng):
    j = -1
    if kind in ("crash1", "ovfpos"):
        j = int(np.argmax(target))
        row[j] = -110.0 if kind == "crash1" else 89.0
    elif kind == "ovf0":
        z = np.flatnonzero(target == 0)
        j = int(z[0]) if len(z) else int(np.argmax(target))   # (N = 1 has no zero entry: inf instead)
        row[j] = 89.0
    elif kind == "nan":
        j = int(rng.integers(len(row)))
        row[j] = np.nan
    return j


def make_path(name, N, seed):
    """targets [S, N] float64, rows [S - 1, N] float32, w0 [N] (exact zeros, not 1 / N), and per
    step (target kind, row kind, singled-out asset)."""
    rng = np.random.default_rng([seed, N, NAMES.index(name)])
    targets, rows, tags = np.empty((S, N)), np.empty((S - 1, N), np.float32), []
    for k, (tk, rk) in enumerate(RECIPES[name]):
        row = make_row(rk, rng, N)
        targets[k] = make_target(tk, rng, N, row)
        j = fix_row(rk, row, targets[k], rng) if row is not None else -1
        if row is not None:
            rows[k] = row
        tags.append((tk, rk, j))
    return targets, rows, _zeros(rng, N), tags
