"""GPU parity of the Koopman rollout kernels (through the C ABI) against yhat from the reference's
model.py (tests/golden), plus the fused window and the end-to-end backtest.

Rollout tolerance: fp32 arithmetic like the reference; the MFMA dot products sum in a different
order. Bars (max|yhat - ref| / max|ref|, printed by assert_rel under pytest -s): 2e-6 against the
reference-generated goldens (measured 0.6-3.0e-7 on MI355X), 1e-5 against the numpy fp32
restatement and between launch variants (measured <= 1.3e-6)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from koopman_mpc_portfolio_rebalancing_amd import (BacktestConfig, DeviceKoopman, KoopmanModelSpec,
                                                   KoopmanMPCStrategy, MPCConfig, calculate_metrics,
                                                   run_backtest, solve_mpc_log_utility_batched)
from oracle import rollout as R
from oracle import solver as oracle

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def assert_rel(d, scale, tol, what=""):
    """max|d| <= tol * scale; prints the measured ratio (pytest -s) so the bar can be checked."""
    r = float(np.abs(d).max()) / float(scale)
    print(f"[rel] {what} {r:.3e} (bar {tol:.0e})")
    assert r <= tol, (what, r, tol)


def load_spec(g):
    meta = json.loads(str(g["meta"]))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    return meta, KoopmanModelSpec.from_state_dict(sd, meta["config"])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "rollout_*.npz"))))
def test_rollout_matches_reference(path):
    g = np.load(path)
    meta, spec = load_spec(g)
    km = DeviceKoopman(spec, torch.device("cuda"))
    y = km.rollout(torch.from_numpy(g["obs"]).cuda(), g["mean"], g["std"], meta["H"], meta["N"]).cpu().numpy()
    ref = g["yhat"]
    assert y.shape == ref.shape
    assert_rel(y - ref, np.abs(ref).max(), 2e-6, os.path.basename(path))


def test_rollout_large_batch_matches_numpy_restatement():
    """Tile edges: B not a multiple of 128, obs/L/hidden not multiples of 32."""
    g = np.load(os.path.join(GOLD, "rollout_generic_finance.npz"))
    meta, spec = load_spec(g)
    rng = np.random.default_rng(0)
    obs = rng.normal(0, 1, (1000, meta["obs"])).astype(np.float32)
    km = DeviceKoopman(spec, torch.device("cuda"))
    y = km.rollout(torch.from_numpy(obs).cuda(), g["mean"], g["std"], 7, meta["N"]).cpu().numpy()
    sd = {k[2:]: g[k] for k in g.files if k.startswith("w:")}
    spec_np = {"kind": "generic", "enc_w": [sd[f"encoder.network.{i}.weight"] for i in (0, 2, 4)],
               "enc_b": [sd[f"encoder.network.{i}.bias"] for i in (0, 2, 4)], "kmat": sd["kmat"],
               "dec_w": [sd["decoder.network.0.weight"]], "dec_b": [None], "norm_fn": "id"}
    ref = R.rollout(spec_np, obs, 7, meta["N"], g["mean"].astype(np.float32), g["std"].astype(np.float32))
    assert_rel(y - ref, np.abs(ref).max(), 1e-5, "large batch")


def test_fused_window_equals_rollout_then_solve():
    g = np.load(os.path.join(GOLD, "rollout_generic_finance.npz"))
    meta, spec = load_spec(g)
    km = DeviceKoopman(spec, torch.device("cuda"))
    N, H = meta["N"], meta["H"]
    obs = torch.from_numpy(g["obs"]).cuda()
    wp = torch.from_numpy(np.random.default_rng(1).dirichlet(np.ones(N), obs.shape[0])).cuda()
    cfg = MPCConfig(horizon=H, cost_coeff=1e-3, max_turnover=0.5)
    W0, st, val, y = km.window(obs, wp, g["mean"], g["std"], N, cfg, keep_yhat=True)
    y2 = km.rollout(obs, g["mean"], g["std"], H, N)
    assert torch.equal(y, y2)
    W0b, st2, val2 = solve_mpc_log_utility_batched(wp, y2, cfg)
    assert torch.equal(W0, W0b) and torch.equal(st, st2)
    # and the oracle chain on the reference yhat agrees to the parity bar
    Wo, sto, valo, _ = oracle.solve_batch(wp.cpu().numpy(), g["yhat"], 1e-3, 0.5)
    assert np.abs(W0.cpu().numpy() - Wo[:, 0]).max() < 1e-3


def test_backtest_matches_reference_run():
    """run_backtest(KoopmanMPCStrategy) on the golden env vs the reference's recorded run (solver
    inside the reference routed to the oracle)."""
    from test_backtest_cpu import GoldenEnv
    g = np.load(os.path.join(GOLD, "backtest_koopman_mpc.npz"))
    meta = json.loads(str(g["meta"]))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    spec = KoopmanModelSpec.from_state_dict(sd, meta["config"])
    env = GoldenEnv(g)
    strat = KoopmanMPCStrategy(spec, MPCConfig(**meta["mpc"]))
    # per-call parity on the recorded solver inputs: rollout yhat and applied weights
    km = strat.device_model()
    T = g["call_yhat"].shape[0]
    y = km.rollout(torch.from_numpy(g["test_data"][:T]).cuda(), g["mean"], g["std"], meta["H"], meta["N"])
    ref_y = g["call_yhat"]
    assert_rel(y.cpu().numpy() - ref_y, np.abs(ref_y).max(), 2e-6, "backtest call_yhat")
    df = run_backtest(strat, env, BacktestConfig(**meta["backtest"]), verbose=False)
    assert len(df) == len(g["df_value"])
    np.testing.assert_allclose(df["portfolio_value"].values, g["df_value"], rtol=1e-6)
    np.testing.assert_allclose(df["turnover"].values, g["df_turnover"], atol=1e-4)
    m = calculate_metrics(df)
    assert m["Final Value"] == pytest.approx(meta["metrics"]["Final Value"], rel=1e-6)
    assert m["Sharpe Ratio"] == pytest.approx(meta["metrics"]["Sharpe Ratio"], rel=1e-4, abs=1e-6)


def test_standardize_kernel_matches_reference_bit_for_bit():
    from koopman_mpc_portfolio_rebalancing_amd import standardize_panel
    g = np.load(os.path.join(GOLD, "embedding.npz"))
    z = standardize_panel(g["log_returns"], g["mean"], g["std"]).cpu().numpy()
    assert np.array_equal(z, g["standardized"])


def test_panel_rollout_equals_embedded_rollout():
    """Reading the embedding in place from the standardized panel (lag-reversed first layer, row
    stride N) gives the rollout of the reference's embedded rows; only the fp32 summation order
    of the first layer differs."""
    g = np.load(os.path.join(GOLD, "embedding.npz"))
    d, z, emb = int(g["emb_dim"]), g["standardized"], g["embedded"]
    T, N = z.shape
    torch.manual_seed(0)
    L, hid = 16, 32
    enc = [(torch.randn(hid, d * N) / np.sqrt(d * N), torch.randn(hid) * 0.1), (torch.randn(L, hid) / np.sqrt(hid), None)]
    dec = [(torch.randn(d * N, L) / np.sqrt(L), None)]
    q, _ = torch.linalg.qr(torch.randn(L, L, dtype=torch.float64))
    spec = KoopmanModelSpec(kind="generic", encoder=enc, kmat=(0.95 * q).float(), decoder=dec)
    km = DeviceKoopman(spec, torch.device("cuda"))
    mean, std = np.full(N, 1e-3, np.float32), np.full(N, 0.02, np.float32)
    H = 3
    y_emb = km.rollout(torch.from_numpy(emb).cuda(), mean, std, H, N).cpu().numpy()
    zt = torch.from_numpy(z).cuda()
    for first, nwin in ((0, emb.shape[0]), (5, 11)):
        y_pan = km.rollout_panel(zt, d, first, nwin, mean, std, H, N).cpu().numpy()
        ref = y_emb[first:first + nwin]
        assert_rel(y_pan - ref, np.abs(ref).max(), 1e-5, "panel")
    with pytest.raises(ValueError):
        km.rollout_panel(zt, d, T - d, 2, mean, std, H, N)


def _oracle_spec(spec):
    """oracle/rollout.py's dict form of a KoopmanModelSpec."""
    t = lambda x: None if x is None else x.detach().cpu().numpy()   # noqa: E731
    d = {"kind": spec.kind, "enc_w": [t(w) for w, _ in spec.encoder], "enc_b": [t(b) for _, b in spec.encoder],
         "enc_act": spec.enc_act, "enc_last_relu": spec.enc_last_relu, "kmat": t(spec.kmat)}
    if spec.kind == "generic":
        d.update(dec_w=[t(w) for w, _ in spec.decoder], dec_b=[t(b) for _, b in spec.decoder],
                 dec_act=spec.dec_act, norm_fn=spec.norm_fn)
    else:
        d.update(dict=t(spec.decoder[0][0]).T.copy(), lista_S=t(spec.lista_S), lista_loops=spec.lista_loops,
                 lista_thresh=spec.lista_thresh)
    return d


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "rollout_*.npz"))))
def test_bf16_rollout_matches_bf16_restatement(path):
    """KMPC_DTYPE_BF16 (BASELINE configs[4]): GEMM operands rounded to bf16 on the bf16 MFMA, fp32
    accumulation and epilogues. Checked against the numpy restatement with the same operand rounding
    (tolerance 2e-3 of max|yhat|: summation order, and the rare activation whose fp32 value sits on
    a bf16 rounding boundary); its deviation from the reference's fp32 yhat is bounded by 5e-2."""
    g = np.load(path)
    meta, spec = load_spec(g)
    km = DeviceKoopman(spec, torch.device("cuda"), dtype="bf16")
    obs = g["obs"]
    y = km.rollout(torch.from_numpy(obs).cuda(), g["mean"], g["std"], meta["H"], meta["N"]).cpu().numpy()
    ref16 = R.rollout(_oracle_spec(spec), obs, meta["H"], meta["N"], g["mean"].astype(np.float32),
                      g["std"].astype(np.float32), bf16=True)
    scale = np.abs(ref16).max()
    assert np.abs(y - ref16).max() <= 2e-3 * scale
    assert np.abs(y - g["yhat"]).max() <= 5e-2 * np.abs(g["yhat"]).max()


def test_bf16_lista_rollout_at_config5_shape():
    """BASELINE configs[4] shape: LISTAKM (linear We), N = 500 assets, d = 20 (obs 10000), latent 512,
    10 LISTA loops, H = 20, bf16 MFMA rollout against the bf16-operand restatement (random weights
    with L = 1.1 ||We||_2^2 as SURVEY §8(d) prescribes, so the LISTA iteration is contractive)."""
    rng = np.random.default_rng(5)
    N, d, L, H, B = 500, 20, 512, 20, 64
    obs_n = N * d
    We = (rng.standard_normal((L, obs_n)) / np.sqrt(obs_n)).astype(np.float32)
    lip = 1.1 * np.linalg.norm(We.astype(np.float64), 2) ** 2
    S = (np.eye(L) - We.astype(np.float64) @ We.astype(np.float64).T / lip).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((L, L)))
    K = (0.95 * q).astype(np.float32)
    D = rng.standard_normal((L, obs_n)).astype(np.float32)
    Dn = (D / np.maximum(np.linalg.norm(D, axis=1, keepdims=True), 1e-4)).astype(np.float32)
    thr = 5e-3 / lip
    spec = KoopmanModelSpec(kind="lista", encoder=[(torch.from_numpy(We / np.float32(lip)), None)],
                            kmat=torch.from_numpy(K), decoder=[(torch.from_numpy(Dn.T.copy()), None)],
                            lista_S=torch.from_numpy(S), lista_loops=10, lista_thresh=float(thr))
    obs = rng.standard_normal((B, obs_n)).astype(np.float32)
    mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
    km = DeviceKoopman(spec, torch.device("cuda"), dtype="bf16")
    y = km.rollout(torch.from_numpy(obs).cuda(), mean, std, H, N).cpu().numpy()
    ref16 = R.rollout(_oracle_spec(spec), obs, H, N, mean, std, bf16=True)
    assert y.shape == (B, H, N)
    # fp32 chain first: the same kernels and data path, exact fp32 products -> summation order only
    y32 = DeviceKoopman(spec, torch.device("cuda")).rollout(torch.from_numpy(obs).cuda(), mean, std, H, N).cpu().numpy()
    ref32 = R.rollout(_oracle_spec(spec), obs, H, N, mean, std)
    assert_rel(y32 - ref32, np.abs(ref32).max(), 1e-5, "lista fp32")
    # bf16 chain: 30 dependent roundings of the state to bf16 (10 LISTA loops, 20 K steps); a
    # summation-order difference of ~1e-6 flips an occasional element's rounding (1 bf16 ulp =
    # 2^-8 relative) and the flips propagate — measured ~4e-3 normwise against the bf16-operand
    # restatement. Bars: 1e-2 normwise, 2^-5 of the decoded scale elementwise; and within 5e-2
    # (normwise) of the fp32 result.
    dec = ref16 - mean
    assert np.linalg.norm(y - ref16) <= 1e-2 * np.linalg.norm(dec)
    assert np.abs(y - ref16).max() <= 2 ** -5 * np.abs(dec).max()
    assert np.linalg.norm(y - ref32) <= 5e-2 * np.linalg.norm(ref32 - mean)


@pytest.mark.parametrize("norm,L,N,B,H", [("id", 64, 20, 1000, 4), ("ball", 64, 40, 333, 3),
                                          ("id", 128, 30, 4096, 5), ("ball", 256, 100, 70, 10),
                                          ("id", 512, 50, 300, 6),     # L = 512: 132 KB of LDS
                                          ("ball", 64, 20, 8200, 3),   # >= 8192, ball: the 16-row loop
                                          ("ball", 256, 40, 8200, 3),  # >= 8192, ball, L = 256: 32-row loop
                                          ("id", 256, 100, 8200, 10), ("id", 256, 33, 8193, 2)])  # ragged
def test_fused_latent_steps_match_unfused_and_numpy(norm, L, N, B, H):
    """The fused H-step latent loops (L % 32 == 0, single-layer decoder) against the per-step GEMM
    launches (KMPC_LATENT_UNFUSED) and the numpy restatement. Which kernel runs (kmpc_rollout.hip):
    below 8,192 windows, or L <= 128, the 16-row loop (latent_steps16_kernel); from 8,192 windows with
    the identity norm the library's default ('auto') is the latent-powers GEMM (latent_powers_kernel
    + one three-plane GEMM with the de-standardising epilogue), and 'sequential' forces the
    step-by-step loop there — latent_steps_x3_kernel at L = 256 — so both are checked; the ball norm
    (nonlinear step) at L = 256 runs the 32-row fp32 loop (latent_steps_kernel)."""
    import bench
    obs, hidden = N * 4, 64
    sd = bench.make_state_dict(obs, L, hidden, seed=3)
    cfg = {"MODEL": dict(bench.MODEL_CFG["MODEL"], NORM_FN=norm)}
    km = DeviceKoopman(KoopmanModelSpec.from_state_dict(sd, cfg), torch.device("cuda"))
    x = torch.randn(B, obs, generator=torch.Generator().manual_seed(1))
    mean = np.linspace(-1e-3, 1e-3, N).astype(np.float32)
    std = np.linspace(0.01, 0.02, N).astype(np.float32)
    yf = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    km.latent_form = "sequential"
    ys = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    km.latent_form = "unfused"                 # KMPC_LATENT_UNFUSED: per-step launches
    yu = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    sdn = {k: v.numpy() for k, v in sd.items()}
    spec_np = {"kind": "generic", "enc_w": [sdn[f"encoder.network.{i}.weight"] for i in (0, 2, 4)],
               "enc_b": [sdn[f"encoder.network.{i}.bias"] for i in (0, 2, 4)], "kmat": sdn["kmat"],
               "dec_w": [sdn["decoder.network.0.weight"]], "dec_b": [None], "norm_fn": norm}
    ref = R.rollout(spec_np, x.numpy(), H, N, mean, std)
    assert_rel(yf - ref, np.abs(ref).max(), 1e-5, f"fused {norm} L{L} B{B}")
    assert_rel(ys - ref, np.abs(ref).max(), 1e-5, f"sequential {norm} L{L} B{B}")
    assert_rel(yf - yu, np.abs(yu).max(), 1e-5, f"fused-vs-unfused {norm} L{L} B{B}")
    if norm == "ball" or B < 8192:   # the same kernel either way: bit-identical
        assert np.array_equal(yf, ys)


# the GenericKM headline models (headline_c5: LISTAKM, its own test below)
HEADLINE = sorted(p for p in glob.glob(os.path.join(GOLD, "headline_*.npz")) if not p.endswith("_c5.npz"))


def _headline(path):
    """A headline golden (tests/golden/make_golden.py make_headline_goldens) and its model: the
    bench's weights regenerated from their seed, checked against the golden's checksums."""
    import bench
    g = np.load(path)
    m = json.loads(str(g["meta"]))
    sd = bench.make_state_dict(m["N"] * m["emb"], m["L"], m["hidden"], seed=m["weight_seed"])
    for k, v in sd.items():
        s1, s2 = m["checksums"][k]
        assert float(v.double().sum()) == pytest.approx(s1, rel=1e-12, abs=1e-12), k
        assert float((v.double() ** 2).sum()) == pytest.approx(s2, rel=1e-12), k
    return g, m, KoopmanModelSpec.from_state_dict(sd, bench.MODEL_CFG)


@pytest.mark.parametrize("form", ["auto", "sequential"])
@pytest.mark.parametrize("path", HEADLINE, ids=[os.path.basename(p)[9:-4] for p in HEADLINE])
def test_headline_rollout_matches_reference(path, form):
    """The bench's own models (c3 = BASELINE configs[2]: obs 2000, encoder [1024, 1024], latent 256,
    N = 100, H = 10; c2 = configs[1]; c1 = configs[0]) against yhat from the reference's GenericKM and
    rebalance op order on 64 windows (reference model.py:701-797, backtest.py:99-121). The 64 rows are
    tiled to 64, 4,096, 8,200 (ragged) and 65,536 windows, so every kernel that produced a bench
    window is pinned at the 2e-6 bar of the reference goldens: the three-plane encoder GEMMs at all
    tile shapes, and for the latent loop the 16-row kernel below 8,192 windows and, from 8,192,
    the latent-powers GEMM ('auto', the bench's path) or the step-by-step loop ('sequential':
    latent_steps_x3_kernel at L = 256). Every row of every tile is compared with its source row."""
    g, m, spec = _headline(path)
    N, H = m["N"], m["H"]
    km = DeviceKoopman(spec, torch.device("cuda"), latent_form=form)
    obs = torch.from_numpy(g["obs"]).cuda()
    ref = g["yhat"]
    scale = np.abs(ref).max()
    for B in (64, 4096, 8200, 65536):
        idx = torch.arange(B, device="cuda") % obs.shape[0]
        y = km.rollout(obs[idx].contiguous(), g["mean"], g["std"], H, N).cpu().numpy()
        d = y - ref[np.arange(B) % ref.shape[0]]
        assert_rel(d, scale, 2e-6, f"{os.path.basename(path)} {form} B{B}")


def test_small_batch_split_k_encoder_matches_numpy():
    """BASELINE configs[1] shape (4,096 windows, obs 600, encoder [1024, 1024] -> latent 128, N = 30,
    H = 5): the 128-wide last encoder layer has fewer 64 x 64 tiles than CUs and runs split-K (four
    K slices summed in slice order by the epilogue kernel); the latent loop runs 16 windows per block.
    Against the numpy fp32 restatement and the per-step (unfused) launches."""
    import bench
    B, N, L, H, hidden = 4096, 30, 128, 5, 1024
    obs = N * 20
    sd = bench.make_state_dict(obs, L, hidden, seed=1)
    km = DeviceKoopman(KoopmanModelSpec.from_state_dict(sd, bench.MODEL_CFG), torch.device("cuda"))
    x = torch.randn(B, obs, generator=torch.Generator().manual_seed(2))
    mean = np.full(N, 5e-4, np.float32)
    std = np.full(N, 0.015, np.float32)
    y = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    y2 = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    assert np.array_equal(y, y2)                        # deterministic split-K sum
    sdn = {k: v.numpy() for k, v in sd.items()}
    spec_np = {"kind": "generic", "enc_w": [sdn[f"encoder.network.{i}.weight"] for i in (0, 2, 4)],
               "enc_b": [sdn[f"encoder.network.{i}.bias"] for i in (0, 2, 4)], "kmat": sdn["kmat"],
               "dec_w": [sdn["decoder.network.0.weight"]], "dec_b": [None],
               "norm_fn": bench.MODEL_CFG["MODEL"]["NORM_FN"]}
    ref = R.rollout(spec_np, x.numpy(), H, N, mean, std)
    assert_rel(y - ref, np.abs(ref).max(), 1e-5, "configs[1] split-K")
    km.fuse_latent = False
    yu = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    assert_rel(y - yu, np.abs(yu).max(), 1e-5, "configs[1] fused-vs-unfused")


@pytest.mark.parametrize("B", [1000, 8200])
def test_encoder_gemm_tiles_match_numpy(B):
    """The fp32 GEMM tiles of the encoder at C3's layer widths (obs 400 -> 1024 -> 1024 -> latent 256,
    N = 100, H = 3): B = 1,000 runs the mid-size path (fewer than 512 128 x 128 tiles: 4 x 4 waves of
    32 x 32), B = 8,200 the large path (4 x 2 waves of 32 x 64) with a ragged last row tile and a
    K tail (400 = 12.5 k-tiles). Against the numpy fp32 restatement."""
    import bench
    N, L, H, hidden = 100, 256, 3, 1024
    obs = N * 4
    sd = bench.make_state_dict(obs, L, hidden, seed=4)
    km = DeviceKoopman(KoopmanModelSpec.from_state_dict(sd, bench.MODEL_CFG), torch.device("cuda"))
    x = torch.randn(B, obs, generator=torch.Generator().manual_seed(5))
    mean = np.full(N, 5e-4, np.float32)
    std = np.full(N, 0.015, np.float32)
    y = km.rollout(x.cuda(), mean, std, H, N).cpu().numpy()
    sdn = {k: v.numpy() for k, v in sd.items()}
    spec_np = {"kind": "generic", "enc_w": [sdn[f"encoder.network.{i}.weight"] for i in (0, 2, 4)],
               "enc_b": [sdn[f"encoder.network.{i}.bias"] for i in (0, 2, 4)], "kmat": sdn["kmat"],
               "dec_w": [sdn["decoder.network.0.weight"]], "dec_b": [None],
               "norm_fn": bench.MODEL_CFG["MODEL"]["NORM_FN"]}
    ref = R.rollout(spec_np, x.numpy(), H, N, mean, std)
    dec = ref - mean
    assert_rel(y - ref, np.abs(dec).max(), 1e-5, f"encoder tiles B{B}")


def test_fused_z0_is_never_read():
    """configs[1] shape (4,096 windows, N = 30, latent 128, encoder [1024, 1024]): the last encoder
    layer runs split-K and leaves z0 unwritten; the fused latent loop rebuilds z0 from the raw
    partials (kmpc_rollout.hip, znparts). With the whole workspace pre-filled with NaN, yhat must
    be finite and bit-identical to a zero-filled workspace — nothing reads z0 (or a stale part)."""
    import ctypes
    import bench
    from koopman_mpc_portfolio_rebalancing_amd import _lib
    dev = torch.device("cuda")
    B, N, L, H = 4096, 30, 128, 5
    obs_n = N * 20
    km = DeviceKoopman(KoopmanModelSpec.from_state_dict(bench.make_state_dict(obs_n, L, 1024, seed=1),
                                                        bench.MODEL_CFG), dev)
    x, _ = bench.window_inputs(0, B, N, obs_n, seed=1, device=dev)
    m = torch.full((N,), 5e-4, device=dev)
    s = torch.full((N,), 0.015, device=dev)
    d = km.rollout_desc(B, H, N, m, s)
    Lb = _lib.load()
    nbytes = Lb.kmpc_workspace_bytes(ctypes.byref(d), None)
    outs = []
    for fill in (0xFF, 0x00):   # 0xFFFFFFFF is a float32 NaN
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
        y = torch.empty((B, H, N), dtype=torch.float32, device=dev)
        _lib.check(Lb.kmpc_rollout(ctypes.byref(d), x.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes,
                                   _lib.stream_handle(dev)))
        outs.append(y)
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], km.rollout(x, m, s, H, N))


# (id, kind, B, obs, L, N, H, dtype, latent form, LISTA loops, the kernel the shape is there for)
WS_CASES = [("bf16_split8", "generic", 200, 2048, 100, 33, 2, "bf16", "auto", 0, "bf16_split8"),
            ("planes", "generic", 8257, 132, 256, 33, 2, "fp32", "sequential", 0, "latx3"),
            ("powers", "generic", 8192, 132, 128, 33, 3, "fp32", "auto", 0, "powers"),
            ("lista", "lista", 300, 132, 64, 33, 2, "fp32", "auto", 2, "shrink")]


@pytest.mark.parametrize("case", WS_CASES, ids=[c[0] for c in WS_CASES])
def test_rollout_stays_inside_its_workspace(case):
    """kmpc_rollout with exactly kmpc_workspace_bytes of a buffer that is 4,096 bytes longer and filled
    with 0xA5: the trailing bytes stay untouched and yhat is bit for bit that of DeviceKoopman.rollout.
    The untouched tail is the check of the layout's far end; the equality only says that the call made
    by hand is the call the package makes (both go through the same layout, so an overlap of two
    regions inside the workspace is for the reference tests of this file to find, not for this one).
    The shapes reach the far end of the regions whose sizes are not a plain [rows, width]: the eight
    bf16 split-K slices (the encoder GEMM 200 x 100 x 2,048), the bf16 plane block (latent_steps_x3_kernel,
    N = 33 padded to 64 decoder rows), the powers block with the tiled epilogue at the workspace's very
    end, and the LISTA path (S^T, c in z1, two loops through ping). The mirror's plan() says that each
    shape takes the route it is there for."""
    import ctypes
    import rollout_variants as rv
    from koopman_mpc_portfolio_rebalancing_amd import _lib
    _, kind, B, obs, L, N, H, dtype, form, loops, kernel = case
    stages = rv.plan_stages(B, obs, [L], L, N, H, kind=kind, dtype=dtype, form=form, lista_loops=loops)
    kernels = [g[0] for _, g in stages]
    assert kernel in kernels, kernels
    if kernel == "bf16_split8":
        assert stages[:2] == [("enc0", ("bf16_split8", "parts", B, L, obs)), ("enc0", ("splitk_epi", "none", B, L, obs))]
    elif kernel == "shrink":
        assert [s for s, _ in stages if s.startswith("lista")] == ["lista0", "lista1"]
    else:
        assert kernels[-1] == {"latx3": "latx3", "powers": "x3_mid44"}[kernel]
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(11)
    rnd = lambda r, c: torch.randn(r, c, generator=gen) / np.sqrt(c)   # noqa: E731
    spec = KoopmanModelSpec(kind=kind, encoder=[(rnd(L, obs), None if kind == "lista" else 0.1 * rnd(1, L)[0])],
                            kmat=rnd(L, L), decoder=[(rnd(obs, L), None)],
                            lista_S=0.5 * rnd(L, L) if kind == "lista" else None, lista_loops=loops,
                            lista_thresh=0.01 if kind == "lista" else 0.0)
    km = DeviceKoopman(spec, dev, dtype=dtype, latent_form=form)
    x = torch.randn(B, obs, generator=gen).to(dev)
    m = torch.linspace(-1e-3, 1e-3, N, device=dev)
    s = torch.linspace(0.01, 0.02, N, device=dev)
    d = km.rollout_desc(B, H, N, m, s)
    Lb = _lib.load()
    nbytes = Lb.kmpc_workspace_bytes(ctypes.byref(d), None)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    y = torch.empty((B, H, N), dtype=torch.float32, device=dev)
    _lib.check(Lb.kmpc_rollout(ctypes.byref(d), x.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_handle(dev)))
    assert bool((ws[nbytes:] == 0xA5).all())
    assert torch.isfinite(y).all()
    assert torch.equal(y, km.rollout(x, m, s, H, N))


def _ref64(sd, x, H, N, mean, std):
    """GenericKM (relu encoder, norm id, one-layer decoder) in float64 (torch CPU, double)."""
    h = x.double()
    for i, k in enumerate((0, 2, 4)):
        h = h @ sd[f"encoder.network.{k}.weight"].double().T + sd[f"encoder.network.{k}.bias"].double()
        if i < 2:
            h = torch.relu(h)
    K = sd["kmat"].double()
    D = sd["decoder.network.0.weight"].double()[:N]
    out = []
    for _ in range(H):
        h = h @ K
        out.append((h @ D.T) * torch.as_tensor(std).double() + torch.as_tensor(mean).double())
    return torch.stack(out, 1).numpy()


@pytest.mark.parametrize("B,N,L,H,obs", [(4096, 30, 128, 5, 600),     # configs[1]: mid tiles + split-K
                                         (8200, 100, 256, 3, 400)])   # C3 widths: large tiles, ragged
def test_fp32_gemm_forms_against_float64(B, N, L, H, obs):
    """dtype 'fp32' runs the GEMMs on the bf16 MFMA with each fp32 operand split exactly into three
    bf16 planes (six plane products, fp32 accumulation); 'fp32_f32mfma' on the f32-input MFMA.
    Both against a float64 restatement of the same model: the three-plane form must be an fp32 GEMM
    in accuracy — max error within 1.5x the f32-input MFMA's (measured 0.8-1.0x: 8.2e-7 vs 9.0e-7
    at configs[1], 8.7e-7 vs 9.2e-7 at C3) and under the 2e-6 bar of the reference goldens."""
    import bench
    sd = bench.make_state_dict(obs, L, 1024, seed=3)
    x = torch.randn(B, obs, generator=torch.Generator().manual_seed(6))
    mean = np.full(N, 5e-4, np.float32)
    std = np.full(N, 0.015, np.float32)
    ref = _ref64(sd, x, H, N, mean, std)
    scale = np.abs(ref - mean).max()
    err = {}
    for dt in ("fp32_f32mfma", "fp32"):
        km = DeviceKoopman(KoopmanModelSpec.from_state_dict(sd, bench.MODEL_CFG), torch.device("cuda"), dtype=dt)
        y = km.rollout(x.cuda(), mean, std, H, N).double().cpu().numpy()
        err[dt] = float(np.abs(y - ref).max() / scale)
        print(f"[rel] {dt} vs float64 {err[dt]:.3e}")
        if dt == "fp32":
            assert np.array_equal(y, km.rollout(x.cuda(), mean, std, H, N).double().cpu().numpy())   # deterministic
    assert err["fp32"] <= 1.5 * err["fp32_f32mfma"] + 1e-8, err
    assert err["fp32"] <= 2e-6, err


def test_three_plane_paths_lista_and_unaligned_rows():
    """The three-plane fp32 paths off the bench shapes, at >= 8,192 windows with L = 256 (the large
    GEMM tiles; the latent loop as the library's default — the latent-powers GEMM — and as
    'sequential', latent_steps_x3_kernel): (1) LISTAKM (linear We, 10 loops: the shrink-epilogue
    GEMMs and the LISTA z0 into the latent loop); (2) GenericKM with obs = 99 (rows not a multiple of
    4 floats: the scalar operand fetch) and N = 33. Each against the numpy fp32 restatement and the
    f32-input MFMA form (1e-5 of the decoded scale, the fp32 rollout bars)."""
    import bench
    rng = np.random.default_rng(9)
    B, L, H = 8200, 256, 4
    # (1) LISTA
    N, d = 64, 3
    obs_n = N * d
    We = (rng.standard_normal((L, obs_n)) / np.sqrt(obs_n)).astype(np.float32)
    lip = 1.1 * np.linalg.norm(We.astype(np.float64), 2) ** 2
    S = (np.eye(L) - We.astype(np.float64) @ We.astype(np.float64).T / lip).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((L, L)))
    D = rng.standard_normal((L, obs_n)).astype(np.float32)
    Dn = (D / np.maximum(np.linalg.norm(D, axis=1, keepdims=True), 1e-4)).astype(np.float32)
    spec = KoopmanModelSpec(kind="lista", encoder=[(torch.from_numpy(We / np.float32(lip)), None)],
                            kmat=torch.from_numpy((0.95 * q).astype(np.float32)),
                            decoder=[(torch.from_numpy(Dn.T.copy()), None)], lista_S=torch.from_numpy(S),
                            lista_loops=10, lista_thresh=float(5e-3 / lip))
    obs = rng.standard_normal((B, obs_n)).astype(np.float32)
    mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
    y1 = DeviceKoopman(spec, torch.device("cuda"), dtype="fp32_f32mfma").rollout(
        torch.from_numpy(obs).cuda(), mean, std, H, N).cpu().numpy()
    ref = R.rollout(_oracle_spec(spec), obs, H, N, mean, std)
    for form in ("auto", "sequential"):
        y = DeviceKoopman(spec, torch.device("cuda"), latent_form=form).rollout(
            torch.from_numpy(obs).cuda(), mean, std, H, N).cpu().numpy()
        assert_rel(y - ref, np.abs(ref - mean).max(), 1e-5, f"three-plane lista L256 {form}")
        assert_rel(y - y1, np.abs(ref - mean).max(), 1e-5, f"three-plane vs f32-input lista L256 {form}")
    # (2) GenericKM, obs 99
    N, obs_n = 33, 99
    sd = bench.make_state_dict(obs_n, L, 512, seed=7)
    spec = KoopmanModelSpec.from_state_dict(sd, bench.MODEL_CFG)
    obs = rng.standard_normal((B, obs_n)).astype(np.float32)
    mean, std = np.full(N, 5e-4, np.float32), np.full(N, 0.015, np.float32)
    y1 = DeviceKoopman(spec, torch.device("cuda"), dtype="fp32_f32mfma").rollout(
        torch.from_numpy(obs).cuda(), mean, std, H, N).cpu().numpy()
    ref = R.rollout(_oracle_spec(spec), obs, H, N, mean, std)
    for form in ("auto", "sequential"):
        y = DeviceKoopman(spec, torch.device("cuda"), latent_form=form).rollout(
            torch.from_numpy(obs).cuda(), mean, std, H, N).cpu().numpy()
        assert_rel(y - ref, np.abs(ref - mean).max(), 1e-5, f"three-plane generic obs99 {form}")
        assert_rel(y - y1, np.abs(ref - mean).max(), 1e-5, f"three-plane vs f32-input generic obs99 {form}")


@pytest.mark.parametrize("form", ["auto", "sequential"])
def test_headline_c5_lista_rollout_matches_reference(form):
    """BASELINE configs[4]'s model (bench.make_lista_state_dict: LISTAKM, linear We, 10 shrink loops,
    latent 512, obs 10,000, N = 500, H = 20) against the reference's LISTAKM (model.py:804-850) on 16
    windows, tiled to 16, 1,024 (the configs[4] batch) and 8,200 windows (the latent-powers GEMM in
    'auto'; the step-by-step loop in 'sequential'). At this depth (10 shrink loops over K = 10,000
    dot products, 20 latent steps) the reference's own fp32 yhat is 9.5e-7 of max|yhat| from the same
    model in float64 (stored in the golden); the device's fp32 forms measured 1.3e-6 (16-row loop,
    B <= 1,024), 1.8e-6 (32-row loop) and 2.06e-6 (latent powers) from it (MI355X, r06). Bars: within
    2.5e-6 of the float64 yhat and 3.5e-6 of the reference's fp32 yhat (two fp32 computations in
    different summation orders); the bf16 configs[4] form within 5e-2 (normwise) of the reference, as
    the small LISTA goldens."""
    import bench
    g = np.load(os.path.join(GOLD, "headline_c5.npz"))
    m = json.loads(str(g["meta"]))
    sd, lc = bench.make_lista_state_dict(m["N"] * m["emb"], m["L"], seed=m["weight_seed"])
    # (S = I - D D^T / Lc and Lc come from CPU matmuls whose summation order is the host BLAS's:
    # another host reproduces them to float32 rounding, not bit for bit — 3.5e-9 relative on the
    # checksum of S, far below what moves yhat at the bars here)
    assert lc == pytest.approx(m["lista_L"], rel=1e-7)
    for k, v in sd.items():
        assert float(v.double().sum()) == pytest.approx(m["checksums"][k][0], rel=1e-7, abs=1e-9), k
    cfg_m = {"MODEL": {"MODEL_NAME": "LISTAKM", "NORM_FN": "id",
                       "ENCODER": {"LISTA": {"ALPHA": 5e-3, "L": lc, "NUM_LOOPS": 10}}}}
    spec = KoopmanModelSpec.from_state_dict(sd, cfg_m)
    N, H = m["N"], m["H"]
    obs = torch.from_numpy(g["obs"]).cuda()
    ref, ref64 = g["yhat"], g["yhat_f64"]
    scale = np.abs(ref).max()
    km = DeviceKoopman(spec, torch.device("cuda"), latent_form=form)
    for B in (16, 1024, 8200):
        idx = torch.arange(B, device="cuda") % obs.shape[0]
        y = km.rollout(obs[idx].contiguous(), g["mean"], g["std"], H, N).cpu().numpy()
        rows = np.arange(B) % ref.shape[0]
        assert_rel(y - ref64[rows], scale, 2.5e-6, f"c5 {form} B{B} vs float64")
        assert_rel(y - ref[rows], scale, 3.5e-6, f"c5 {form} B{B} vs reference fp32")
    y16 = DeviceKoopman(spec, torch.device("cuda"), dtype="bf16").rollout(obs, g["mean"], g["std"], H, N).cpu().numpy()
    assert np.linalg.norm(y16 - ref) <= 5e-2 * np.linalg.norm(ref - g["mean"].astype(np.float32))
