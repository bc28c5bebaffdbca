"""Every kernel of the rollout on the device, one launch at a time and element by element.

Each cell of tests/rollout_variants.py makes every stage of the rollout but one an exact identity, so
yhat (through DeviceKoopman.rollout / rollout_panel) is the output of one GEMM or one latent step. With
e = yhat - float64 reference, s_ij = sum_k |a_ik||w_jk| + |bias_j| and u = 2^-24, a cell asserts

 1. element by element |e_ij| <= k_max u s_ij (+ the epilogue's own roundings, rollout_variants.expected),
 2. rms_ij(e_ij / (u s_ij)) <= k_rms over the whole output, over the last ragged row tile and over the
    last ragged column tile; for the three-plane kernels also <= 1.5 x the f32-input kernel's rms,
 3. a second run is bit-identical,
 4. where the mirror says two latent forms run the same launches, their outputs are bit-identical.

k_max and k_rms come from the reference, never from the kernels: for the cell's own inputs the larger
of two float32 CPU restatements of the accumulation (numpy's float32 product; a strictly sequential
float32 sum over k) against float64 gives the max and the rms of e / (u s); k_max = 4 x that max (the
MFMA sums in another tree) + 3 for the plane kernels (three planes drop at most 2.01 u |a b| per
product: derived), k_rms = 3 x that rms (for a ragged tile: of the larger of the tile's and the whole
output's). Fixed: k_max <= 32, k_rms <= 2. Measured on the CPU for these cells (Gaussian operands):

    K                  20-48      64-160     256-600    2047-2048 (bf16 operands)
    restatement max    2.8-5.0    1.4-4.8    1.4-5.5    2.0-2.1
    restatement rms    0.19-0.50  0.17-0.50  0.43-0.49  0.22-0.23
    k_max (x3: + 3)    11-20      5.4-19     5.4-22     7.9-8.3
    k_rms              0.56-1.5   0.50-1.5   1.3-1.5    0.66-0.68

Every test prints its ratios under pytest -s. A failure names the kernel, the epilogue and whether the
faulty element is in the interior, the last row tile or the last column tile (an rms: over the whole
output or one of those tiles).
"""
import numpy as np
import pytest
import torch

import rollout_variants as rv
from koopman_mpc_portfolio_rebalancing_amd import DeviceKoopman, KoopmanModelSpec
from oracle import rollout as R

pytestmark = pytest.mark.gpu


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a))


def _spec(m):
    pairs = lambda ls: [(_t(w), _t(b)) for w, b in ls]   # noqa: E731
    return KoopmanModelSpec(kind=m["kind"], encoder=pairs(m["enc"]), kmat=_t(m["kmat"]), decoder=pairs(m["dec"]),
                            enc_act=m["enc_act"], enc_last_relu=m["enc_last_relu"], dec_act=m["dec_act"], norm_fn=m["norm"],
                            lista_S=_t(m["S"]), lista_loops=m["loops"], lista_thresh=m["thr"])


def _run(m, dtype, form, spec=None):
    km = DeviceKoopman(spec or _spec(m), torch.device("cuda"), dtype=dtype, latent_form=form)
    mean, std = _t(m["mean"]), _t(m["std"])
    if m.get("panel"):
        d, Na = m["panel"]
        y = km.rollout_panel(_t(m["z"]).cuda(), d, 0, m["x"].shape[0], mean, std, m["H"], Na)
    else:
        y = km.rollout(_t(m["x"]).cuda(), mean, std, m["H"], m["N"])
    return y.cpu().numpy()


def _identity_model(B, L, n_dec, kind):
    rng = np.random.default_rng(B + L)
    eye = np.eye(L, dtype=np.float32)
    m = dict(kind=kind, enc=[(eye, None)], kmat=eye, dec=[(eye, None)] * n_dec, enc_act="relu", enc_last_relu=False,
             dec_act="relu", norm="id", S=None, loops=0, thr=0.0, H=3, N=L - 3, mean=np.zeros(L - 3, np.float32),
             std=np.ones(L - 3, np.float32), x=rng.standard_normal((B, L)).astype(np.float32))
    if kind == "lista":       # z = shrink(z S + c) with S = 0 and threshold 0 is c
        m.update(S=np.zeros((L, L), np.float32), loops=2)
    if n_dec == 2:            # relu between the decoder's identities: exact on what it lets through
        m["x"] = np.abs(m["x"])
    return m


@pytest.mark.parametrize("dtype", ["fp32", "fp32_f32mfma", "bf16"])
@pytest.mark.parametrize("B,L,n_dec,kind", rv.IDENTITY, ids=[f"B{B}_L{L}_dec{n}_{k}" for B, L, n, k in rv.IDENTITY])
def test_identity_chain_is_exact(B, L, n_dec, kind, dtype):
    """The premise of every cell: an all-identity model returns x[:, :N] bit for bit at each of the H
    steps (bf16: bf16_round(x)), in every latent form — through the 16-row loops, the 32-row loop, the
    three-plane loop, the powers GEMM and the per-step GEMMs, on planes and on the f32-input MFMA."""
    m = _identity_model(B, L, n_dec, kind)
    want = (R.bf16_round(m["x"]) if dtype == "bf16" else m["x"])[:, :m["N"]]
    spec = _spec(m)
    kw = dict(kind=kind, dtype=dtype, n_dec_layers=n_dec, lista_loops=m["loops"])
    seen = set()
    for form in ("auto", "sequential", "unfused"):
        seen |= {g[0] for g in rv.plan(B, L, [L], L, m["N"], m["H"], form=form, **kw)}
        y = _run(m, dtype, form, spec)
        for t in range(m["H"]):
            assert np.array_equal(y[:, t], want), (form, t, float(np.abs(y[:, t] - want).max()))
    print(f"[identity] B{B} L{L} {dtype}: {sorted(seen)}")


@pytest.mark.parametrize("c", rv.CELLS, ids=[c["id"] for c in rv.CELLS])
def test_cell(c):
    m = rv.model(c)
    spec = _spec(m)
    y = _run(m, c["dtype"], c["form"], spec)
    assert y.shape == (c["B"], m["H"], m["N"])
    assert np.isfinite(y).all(), f"{c['kernel']}/{c['epi']} {c['id']}: non-finite yhat"
    # 3. deterministic
    assert np.array_equal(y, _run(m, c["dtype"], c["form"], spec)), f"{c['kernel']} {c['id']}: a second run differs"
    # 4. forms that run the same launches
    a, kw = rv.plan_args(c)
    if c["form"] in ("auto", "sequential"):
        other = "sequential" if c["form"] == "auto" else "auto"
        if rv.plan(*a, **dict(kw, form=other)) == rv.plan(*a, **kw):
            assert np.array_equal(y, _run(m, c["dtype"], other, spec)), f"{c['kernel']} {c['id']}: {other} differs"
    # 1., 2. element by element and rms, per region
    rms = [rv.judge(c, k) for k in rv.checks(c, y)]
    # ... and for the plane kernels against the f32-input kernel on the same cell
    if c["kernel"].startswith("x3_") or c["kernel"] == "latx3":
        twin = dict(c, dtype="fp32_f32mfma")
        twin["kernel"] = [g for g in rv.probed(twin) if g[0] != "powers"][0][0]
        y32 = _run(m, "fp32_f32mfma", c["form"], spec)
        for k, r, k32 in zip(rv.checks(c, y), rms, rv.checks(twin, y32)):
            rv.compare_planes(c, k, r, rv.judge(twin, k32, quiet=True))
