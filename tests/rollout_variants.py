"""The kernels of the rollout (kmpc_rollout.hip) and the matrix of cells that reaches each of them
with ONE launch probed element by element: shared by test_rollout_variants_cpu.py (the matrix names
every kernel, epilogue, threshold side and edge shape; the mirror below is pinned to the library's
constants; reference and bound hold on CPU restatements) and test_rollout_variants_gpu.py (every cell
on the device against float64).

plan() is a hand mirror of route_gemm() and plan_rollout(): the ordered launches of one rollout as
(kernel, epilogue, M, N, K). Kernel names:

* fp32 GEMMs on three bf16 planes, x3_split64 / x3_mid44 / x3_big42 (gemm_nt_x3_kernel: the 64-square
  tile with four K slices, the 128-square tile of 16 waves, of 8 waves), the same three on the
  f32-input MFMA with the prefix f32_ (gemm_nt_kernel), and bf16_split8 / bf16_64 / bf16_128
  (gemm_nt_bf16_kernel);
* splitk_epi (splitk_epilogue_kernel) after a split GEMM, or raw_parts where the last encoder layer's
  partials are left for the latent loop to sum (latent_z0; a hand-off, not a launch);
* the fused latent loops lat16_kdir / lat16_kt (latent_steps16_kernel reading K in place / K^T), lat32
  (latent_steps_kernel), latx3 (latent_steps_x3_kernel) and powers (latent_powers_kernel, followed by
  one GEMM);
* the element-wise ball_norm and shrink. (The transposes, split_planes and tile_epilogue launches
  move data only and are not listed.)

A cell makes every stage but one an exact identity (identity weights, mean 0, std 1), so yhat is the
output of the probed launch bit for bit; model() builds it, checks() cuts yhat into (A, W, out)
problems, expected() gives the float64 answer with the per-element scale, judge() applies the bound.
"""
import functools

import numpy as np

from oracle import rollout as R

U = 2.0 ** -24
K_MAX_CAP, K_RMS_CAP = 32.0, 2.0     # fixed: inputs whose CPU restatements need more are wrong inputs
X3_EXTRA = 3.0                        # three planes drop at most 2.01 u |a b| per product (derived)
PLANE_VS_F32 = 1.5                    # plane kernels: rms within 1.5 x the f32-input kernel's

# ---- the library's constants (pinned to kmpc_rollout.hip's by test_rollout_variants_cpu.py) -------
LAT16_MAXB = 8192        # batches below run the 16-row loop
LATPOW_MINB = 8192       # the latent-powers GEMM from here ('auto')
LAT16_WAVES = 8          # the 16-row loop at any batch while L <= 16 * this
F32_SPLITK = 4           # slices of the fp32 split, taken from K >= 128 * this
GEMM_MID, GEMM_BIG = 44, 42     # TILE_128_44 below BIG_TILES, TILE_128_42 from there
BF16_SPLIT_MINK = 2048   # K from which bf16 splits
BF16_SPLIT = 8           # SPLITK_BUF: slices of the bf16 split
SPLITK_ELEMS = 256 * 64 * 64
BIG_TILES = 512          # 128-square tiles from which the large form runs
SPLIT_TILES64 = 256      # 64-square tiles below which a long K is split
BF16_FEW = 256           # 128-square tiles below which bf16 runs the 64-square tile (or the split)
FUSE_L_MULT, FUSE_L_MAX = 32, 512    # latent_fusable: L % 32 == 0 and L <= 512
LATX3_L = 256

GEMMS_F32 = [p + f for p in ("x3_", "f32_") for f in ("split64", "mid44", "big42")]
GEMMS_BF16 = ["bf16_split8", "bf16_64", "bf16_128"]
LOOPS = ["lat16_kdir", "lat16_kt", "lat32", "latx3", "powers"]
KERNELS = GEMMS_F32 + GEMMS_BF16 + ["splitk_epi", "raw_parts"] + LOOPS + ["ball_norm", "shrink"]
EPILOGUES = ["none", "act", "shrink", "destd"]

# rows x columns of one workgroup's output tile (the ragged last tiles are judged on their own)
TILE = {"split64": (64, 64), "mid44": (128, 128), "big42": (128, 128), "bf16_split8": (128, 128),
        "bf16_64": (64, 64), "bf16_128": (128, 128), "lat16_kdir": (16, 16), "lat16_kt": (16, 16),
        "lat32": (32, 32), "latx3": (64, 32)}


def tile_of(kernel):
    return TILE[kernel.split("_", 1)[1] if kernel.startswith(("x3_", "f32_")) else kernel]


def _ceil(a, b):
    return -(-a // b)


def gemm(M, N, K, epi, dtype, raw_ok=False):
    """route_gemm() of kmpc_rollout.hip: the launches of one GEMM with a fused epilogue."""
    if M <= 0 or N <= 0:
        return []
    t128 = _ceil(N, 128) * _ceil(M, 128)
    if dtype == "bf16":
        few = t128 < BF16_FEW
        if few and K >= BF16_SPLIT_MINK and M * N <= SPLITK_ELEMS:
            return [("bf16_split8", "parts", M, N, K), ("splitk_epi", epi, M, N, K)]
        return [("bf16_64" if few else "bf16_128", epi, M, N, K)]
    pre = "x3_" if dtype == "fp32" else "f32_"
    if t128 < BIG_TILES:
        if _ceil(N, 64) * _ceil(M, 64) < SPLIT_TILES64 and K >= 128 * F32_SPLITK:
            tail = "raw_parts" if raw_ok and epi == "none" else "splitk_epi"
            return [(pre + "split64", "parts", M, N, K), (tail, epi, M, N, K)]
        return [(pre + {44: "mid44", 42: "big42"}[GEMM_MID], epi, M, N, K)]
    return [(pre + {44: "mid44", 42: "big42"}[GEMM_BIG], epi, M, N, K)]


def fusable(L, kind, norm, dtype, form, n_dec_layers):
    return (form != "unfused" and dtype != "bf16" and n_dec_layers == 1 and L % FUSE_L_MULT == 0 and L <= FUSE_L_MAX
            and not (kind == "generic" and norm not in ("id", "ball")))


def plan_stages(B, obs, enc_dims, L, N, H, kind="generic", norm="id", dtype="fp32", form="auto", n_dec_layers=1,
                lista_loops=0, panel=False, enc_act="relu", enc_last_relu=False, dec_act="relu", dec_hidden=None):
    """plan_rollout() and rollout_launch(): [(stage, (kernel, epilogue, M, N, K))]. enc_dims are the encoder's layer widths
    after obs (the last is L); panel changes the first layer's row stride only, not its launch."""
    assert enc_dims[-1] == L and N <= obs
    ball = kind == "generic" and norm == "ball"
    fus = fusable(L, kind, norm, dtype, form, n_dec_layers)
    latpow = form == "auto" and fus and B >= LATPOW_MINB and not ball
    lat16 = fus and (B < LAT16_MAXB or L <= 16 * LAT16_WAVES)
    kdir = lat16 and B < LAT16_MAXB and not latpow
    zfuse = kind == "generic" and fus and not ball and not latpow
    out = []

    def mlp(tag, dims, act, last_relu, last_cols, last_epi, raw_ok):
        for l in range(len(dims) - 1):
            last = l == len(dims) - 2
            epi = f"act:{act}" if not last else last_epi if last_epi != "none" else "act:relu" if last_relu else "none"
            for g in gemm(B, last_cols if last else dims[l + 1], dims[l], epi, dtype, raw_ok and last):
                out.append((f"{tag}{l}", g))

    mlp("enc", [obs] + list(enc_dims), enc_act, enc_last_relu, L, "none", zfuse)
    if kind == "generic":
        if ball:
            out.append(("encnorm", ("ball_norm", "none", B, L, L)))
    else:
        out.append(("shrink", ("shrink", "none", B, L, 0)))
        for it in range(lista_loops):
            out += [(f"lista{it}", g) for g in gemm(B, L, L, "shrink", dtype)]
    if latpow:
        out.append(("powers", ("powers", "none", N, L, L)))
        out += [("powers", g) for g in gemm(B, H * N, L, "destd", dtype)]
    elif fus:
        k = ("lat16_kdir" if kdir else "lat16_kt") if lat16 else \
            "latx3" if dtype == "fp32" and not ball and L == LATX3_L else "lat32"
        out.append(("loop", (k, "destd", B, L, L)))
    else:
        hid = L if dec_hidden is None else dec_hidden
        for t in range(H):
            out += [(f"step{t}", g) for g in gemm(B, L, L, "none", dtype)]
            if ball:
                out.append((f"norm{t}", ("ball_norm", "none", B, L, L)))
            mlp(f"dec{t}.", [L] + [hid] * (n_dec_layers - 1) + [N], dec_act, False, N, "destd", False)
    return out


def plan(*a, **kw):
    """The ordered launches of one rollout as (kernel, epilogue, M, N, K)."""
    return [g for _, g in plan_stages(*a, **kw)]


# ---- the matrix -----------------------------------------------------------------------------------
# A cell: id, stage (which launch is probed), kernel / tail / epi (what it is there for), the shape and
# the model options. Stages:
#   enc    encoder layer 0, A = obs [B, K], W [n, K]: one layer (epilogue none, or relu with last_relu),
#          or followed by a square identity layer (its activation the epilogue). panel = (d, Na): read in
#          place from a [B + d - 1, Na] panel with row stride Na.
#   dec    decoder layer 0 behind an identity encoder and K = I, A = obs[:, :K]: one layer (epilogue
#          destd into yhat with ldc = H n), or followed by an identity layer (activation epilogue).
#   step   one latent step, A = z_{t-1} (the device's own yhat[:, t-1]), W = K^T, decoder I: the
#          per-step GEMM ('unfused', or a latent the loops do not take) or a fused loop.
#   powers the latent-powers GEMM: A = z0, W = [W_1; ..; W_H] (float64 chains rounded once), destd.
#   lista  the LISTA loop GEMM, A = shrink(obs), W = S^T, addend obs, epilogue shrink (loops = 0: the
#          shrink kernel alone, exact).
#   ball   the ball norm behind identities (norm of a normed row).
def _cell(id, stage, kernel, epi, B, n, K, **kw):
    c = dict(id=id, stage=stage, kernel=kernel, tail=None, epi=epi, B=B, n=n, K=K, bias=False, act=None, dtype="fp32",
             form="auto", H=1, panel=None, norm="id", loops=1)
    c.update(kw)
    return c


def _both(id, stage, form_kernel, epi, B, n, K, **kw):
    """The same cell on three bf16 planes and on the f32-input MFMA (adjacent: they share inputs)."""
    return [_cell(f"{id}-{p}{form_kernel}", stage, p + form_kernel, epi, B, n, K, dtype=dt, **kw)
            for p, dt in (("x3_", "fp32"), ("f32_", "fp32_f32mfma"))]


def _cells():
    c = []
    sp = dict(tail="splitk_epi")
    # -- activation epilogue: decoder layer 0 of two (M = B, N = n, K = L), and the encoder's first layer
    c += _both("dec_relu_B300_n100_K515", "dec", "split64", "act:relu", 300, 100, 515, act="relu", bias=True, **sp)
    c += _both("dec_tanh_B65_n33_K512", "dec", "split64", "act:tanh", 65, 33, 512, act="tanh", **sp)
    c += _both("dec_gelu_B1_n100_K600", "dec", "split64", "act:gelu", 1, 100, 600, act="gelu", bias=True, **sp)
    c += _both("dec_relu_B1088_n960_K512", "dec", "split64", "act:relu", 1088, 960, 512, act="relu", bias=True, **sp)  # 255 tiles
    c += _both("dec_relu_B1024_n1024_K512", "dec", "mid44", "act:relu", 1024, 1024, 512, act="relu")    # 256 tiles
    c += _both("dec_relu_B300_n100_K511", "dec", "mid44", "act:relu", 300, 100, 511, act="relu")
    c += _both("dec_tanh_B1000_n200_K99", "dec", "mid44", "act:tanh", 1000, 200, 99, act="tanh", bias=True)
    c += _both("dec_gelu_B130_n33_K20", "dec", "mid44", "act:gelu", 130, 33, 20, act="gelu")
    c += _both("dec_relu_B9300_n896_K40", "dec", "mid44", "act:relu", 9300, 896, 40, act="relu")        # 511 tiles
    c += _both("dec_relu_B8192_n1024_K40", "dec", "big42", "act:relu", 8192, 1024, 40, act="relu", bias=True)  # 512 tiles
    c += _both("dec_tanh_B8200_n1000_K99", "dec", "big42", "act:tanh", 8200, 1000, 99, act="tanh")
    c += _both("dec_gelu_B8200_n1024_K40", "dec", "big42", "act:gelu", 8200, 1024, 40, act="gelu", bias=True)
    c += _both("enc_lastrelu_B1000_n64_K99", "enc", "mid44", "act:relu", 1000, 64, 99, act="last_relu", bias=True,
               form="unfused")
    c += _both("enc_relu_B300_n100_K600", "enc", "split64", "act:relu", 300, 100, 600, act="relu", bias=True, **sp)
    # panel mode: row stride Na odd (the scalar operand fetch) and a multiple of four
    c += _both("panel_relu_B300_n64_d3_Na33", "enc", "mid44", "act:relu", 300, 64, 99, act="relu", bias=True, panel=(3, 33))
    c += _both("panel_relu_B300_n64_d5_Na20", "enc", "mid44", "act:relu", 300, 64, 100, act="relu", bias=True, panel=(5, 20))
    # -- no epilogue: the last encoder layer (bias), the per-step latent GEMM (none)
    c += _both("enc_none_B300_n100_K600", "enc", "split64", "none", 300, 100, 600, bias=True, form="unfused", **sp)
    c += _both("enc_none_B130_n33_K99", "enc", "mid44", "none", 130, 33, 99, bias=True, form="unfused")
    c += _both("step_unfused_B1000_L96", "step", "mid44", "none", 1000, 96, 96, form="unfused", H=2)
    c += _both("step_L48_B1000", "step", "mid44", "none", 1000, 48, 48, H=2)                       # L % 32 != 0
    c += _both("step_L544_B300", "step", "split64", "none", 300, 544, 544, H=2, **sp)              # L > 512
    c += _both("step_unfused_B16400_L512", "step", "big42", "none", 16400, 512, 512, form="unfused")
    # z0 left as raw partials, into the 16-row loop reading K in place and reading K^T
    c += _both("enc_raw_B300_n64_K600", "enc", "split64", "none", 300, 64, 600, bias=True, tail="raw_parts", H=2)
    c += _both("enc_raw_B8192_n64_K512", "enc", "split64", "none", 8192, 64, 512, bias=True, tail="raw_parts",
               form="sequential", H=2)
    # -- de-standardise and scatter (ldc = H n): the one-layer decoder, the powers GEMM
    c += _both("dec_destd_B300_n100_K515", "dec", "split64", "destd", 300, 100, 515, bias=True, form="unfused", H=2, **sp)
    c += _both("dec_destd_B1000_n33_K40", "dec", "mid44", "destd", 1000, 33, 40, form="unfused", H=2)
    c += _both("dec_destd_B333_n1_K100", "dec", "mid44", "destd", 333, 1, 100, bias=True, form="unfused", H=2)
    c += _both("dec_destd_B8200_n1024_K40", "dec", "big42", "destd", 8200, 1024, 40, bias=True, form="unfused", H=2)
    c += _both("powers_B8192_N33_L128_H3", "powers", "mid44", "destd", 8192, 33, 128, bias=True, H=3)
    c += _both("powers_B8192_N100_L64_H9", "powers", "big42", "destd", 8192, 100, 64, bias=True, H=9)
    # -- LISTA shrink epilogue
    c += _both("lista_B300_L515", "lista", "split64", "shrink", 300, 515, 515, form="unfused", **sp)
    c += _both("lista_B1000_L100", "lista", "mid44", "shrink", 1000, 100, 100, form="unfused")
    c += _both("lista_B16400_L512", "lista", "big42", "shrink", 16400, 512, 512, form="unfused")
    c.append(_cell("lista_shrink_only_B1000_L100", "lista", "shrink", "none", 1000, 100, 100, loops=0, form="unfused"))
    # -- bf16: the decoder's last layer (every later stage would round again)
    c.append(_cell("bf16_dec_B300_n33_K100", "dec", "bf16_64", "destd", 300, 33, 100, bias=True, dtype="bf16", H=2))
    c.append(_cell("bf16_dec_B200_n100_K2047", "dec", "bf16_64", "destd", 200, 100, 2047, dtype="bf16", H=2))
    c.append(_cell("bf16_dec_B200_n100_K2048", "dec", "bf16_split8", "destd", 200, 100, 2048, bias=True, dtype="bf16",
                   H=2, **sp))
    c.append(_cell("bf16_dec_B8200_n512_K40", "dec", "bf16_128", "destd", 8200, 512, 40, bias=True, dtype="bf16", H=2))
    # -- the fused latent loops (H = 3: steps 1 and 2 start from the device's own previous step)
    lat = lambda id, k, B, L, **kw: _cell(id, "step", k, "destd", B, L, L, **dict(dict(H=3), **kw))   # noqa: E731
    c.append(lat("loop_B17_L64", "lat16_kdir", 17, 64))
    c.append(lat("loop_B300_L512", "lat16_kdir", 300, 512))
    c.append(lat("loop_B8191_L128", "lat16_kdir", 8191, 128))
    c.append(lat("loop_B8193_L128_seq", "lat16_kt", 8193, 128, form="sequential"))
    c.append(lat("loop_B8193_L160_seq", "lat32", 8193, 160, form="sequential"))
    c.append(lat("loop_B8200_L384_seq_f32", "lat32", 8200, 384, form="sequential", dtype="fp32_f32mfma"))
    c.append(lat("loop_B8193_L512_seq", "lat32", 8193, 512, form="sequential", H=2))
    c.append(lat("loop_B8225_L256_seq_f32", "lat32", 8225, 256, form="sequential", dtype="fp32_f32mfma"))
    c.append(lat("loop_B8257_L256_seq", "latx3", 8257, 256, form="sequential"))
    # -- the ball norm: in the 16-row loop at any batch size, and as its own kernel between per-step GEMMs
    c.append(_cell("ball_B8193_L64", "ball", "lat16_kt", "destd", 8193, 64, 64, norm="ball"))
    c.append(_cell("ball_B333_L100", "ball", "ball_norm", "none", 333, 100, 100, norm="ball"))
    return c


CELLS = _cells()
BY_ID = {c["id"]: c for c in CELLS}
assert len(BY_ID) == len(CELLS)


def _base_id(c):
    """The id without the GEMM form: the x3 / f32 twins of a cell share model, inputs and reference."""
    return c["id"].rsplit("-", 1)[0]


BASE = {}
for _c in CELLS:
    BASE.setdefault(_base_id(_c), _c)

# the identity chains of the premise: (B, L, n_dec_layers, kind); every form and dtype runs each
IDENTITY = [(70, 64, 1, "generic"), (8200, 64, 1, "generic"), (8200, 160, 1, "generic"), (8200, 256, 1, "generic"),
            (300, 48, 2, "generic"), (300, 64, 1, "lista")]


# ---- models ---------------------------------------------------------------------------------------
def _seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(_base_id(c))) % (2 ** 31)


def _eye(r, cols):
    return np.eye(r, cols, dtype=np.float32)


def plan_args(c):
    """The arguments of plan_stages() for a cell's model."""
    st, B, n, K = c["stage"], c["B"], c["n"], c["K"]
    kw = dict(dtype=c["dtype"], form=c["form"], norm=c["norm"])
    if st == "enc":
        two = c["act"] in ("relu", "tanh", "gelu")
        return (B, K, [n, n] if two else [n], n, min(n, c["panel"][1] if c["panel"] else K), c["H"]), \
            dict(kw, enc_act=c["act"] if two else "relu", enc_last_relu=c["act"] == "last_relu", panel=bool(c["panel"]))
    if st == "dec":
        two = c["act"] is not None
        return (B, max(n, K), [K], K, n, c["H"]), dict(kw, n_dec_layers=2 if two else 1, dec_act=c["act"] or "relu",
                                                       dec_hidden=n)
    if st in ("step", "ball"):
        return (B, n, [n], n, n, c["H"]), kw
    if st == "powers":
        return (B, max(n, K), [K], K, n, c["H"]), kw
    if st == "lista":
        return (B, n, [n], n, n, c["H"]), dict(kw, kind="lista", lista_loops=c["loops"])
    raise ValueError(st)


def probed(c):
    """The launches of a cell's plan that belong to its probed stage."""
    tag = {"enc": ("enc0",), "dec": ("dec0.0",), "step": ("step0", "loop"), "powers": ("powers",),
           "lista": ("lista0",) if c["loops"] else ("shrink",), "ball": ("loop", "norm0")}[c["stage"]]
    a, kw = plan_args(c)
    return [g for s, g in plan_stages(*a, **kw) if s in tag]


@functools.lru_cache(maxsize=2)
def _model(key):
    c = BASE[key]
    rng = np.random.default_rng(_seed(c))
    st, B, n, K, H = c["stage"], c["B"], c["n"], c["K"], c["H"]
    g32 = lambda *s: rng.standard_normal(s).astype(np.float32)   # noqa: E731
    m = dict(kind="generic", enc_act="relu", enc_last_relu=False, dec_act="relu", norm=c["norm"], S=None, loops=0,
             thr=0.0, H=H, panel=c["panel"])
    bias = lambda k: (0.5 * g32(k)) if c["bias"] else None   # noqa: E731
    if st == "enc":
        W = g32(n, K) / np.float32(np.sqrt(K))
        two = c["act"] in ("relu", "tanh", "gelu")
        m["enc"] = [(W, bias(n))] + ([(_eye(n, n), None)] if two else [])
        m["enc_act"] = c["act"] if two else "relu"
        m["enc_last_relu"] = c["act"] == "last_relu"
        if c["panel"]:
            d, Na = c["panel"]
            assert d * Na == K
            m["z"] = g32(B + d - 1, Na)
            m["x"] = np.lib.stride_tricks.sliding_window_view(m["z"].reshape(-1), K)[::Na][:B]   # row i: z rows i..i+d-1
            nvis = min(n, Na)
        else:
            m["x"] = g32(B, K)
            nvis = min(n, K)
        cols = np.arange(n) if nvis == n else np.unique(np.round(np.linspace(0, n - 1, nvis)).astype(int))
        m.update(kmat=_eye(n, n), dec=[(_eye(n, n)[cols], None)], N=len(cols), cols=cols)
    elif st == "dec":
        obs = max(n, K)
        m["x"] = g32(B, obs)
        m["enc"] = [(_eye(K, obs), None)]
        m["kmat"] = _eye(K, K)
        W = g32(n, K) / np.float32(np.sqrt(K))
        if c["act"] is not None:
            m.update(dec=[(W, bias(n)), (_eye(n, n), None)], dec_act=c["act"])
        else:
            m["dec"] = [(W, bias(n))]
        m["N"] = n
    elif st in ("step", "ball"):
        m["x"] = g32(B, n)
        m["enc"] = [(_eye(n, n), None)]
        m["kmat"] = _eye(n, n) if st == "ball" else g32(n, n) / np.float32(np.sqrt(n))
        m.update(dec=[(_eye(n, n), None)], N=n)
    elif st == "powers":
        L, obs = K, max(n, K)
        x = g32(B, obs)
        x[:L] = 0
        x[:L, :L] = _eye(L, L)              # unit rows: yhat[j, t, :] shows column j of W_t exactly
        m["x"] = x
        m["enc"] = [(_eye(L, obs), None)]
        m["kmat"] = g32(L, L) / np.float32(np.sqrt(L))
        m.update(dec=[(g32(n, L) / np.float32(np.sqrt(L)), bias(n))], N=n)
    elif st == "lista":
        m.update(kind="lista", x=g32(B, n), enc=[(_eye(n, n), None)], kmat=_eye(n, n), dec=[(_eye(n, n), None)], N=n,
                 S=np.float32(0.5) * g32(n, n) / np.float32(np.sqrt(n)), loops=c["loops"], thr=0.125)
    N = m["N"]
    if c["epi"] == "destd" and st in ("dec", "powers"):
        m["mean"], m["std"] = g32(N), rng.uniform(0.5, 2.0, N).astype(np.float32)
    else:
        m["mean"], m["std"] = np.zeros(N, np.float32), np.ones(N, np.float32)
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m


def model(c):
    """The cell's model and inputs in numpy (x3 / f32 twins share one): enc / dec lists of (W, b) in
    nn.Linear layout, kmat, S, x [B, obs] (and the panel z), H, N, mean, std."""
    return _model(_base_id(c))


def oracle_spec(m):
    """oracle/rollout.py's form of a model (the numpy float32 restatement)."""
    d = {"kind": m["kind"], "enc_w": [w for w, _ in m["enc"]], "enc_b": [b for _, b in m["enc"]], "enc_act": m["enc_act"],
         "enc_last_relu": m["enc_last_relu"], "kmat": m["kmat"]}
    if m["kind"] == "generic":
        d.update(dec_w=[w for w, _ in m["dec"]], dec_b=[b for _, b in m["dec"]], dec_act=m["dec_act"], norm_fn=m["norm"])
    else:   # (the restatement renormalises the dictionary's rows: unit rows stay as they are)
        d.update(dict=np.ascontiguousarray(m["dec"][0][0].T), lista_S=m["S"], lista_loops=m["loops"], lista_thresh=m["thr"])
    return d


def numpy_rollout(c):
    """yhat of the cell's model by the numpy float32 restatement (identity stages are exact there too)."""
    m = model(c)
    if c["stage"] == "powers":
        # the sequential rollout is no restatement of the powers form (its error scales with |z0| |K|^t |D|,
        # not with |z0| |W_t|): z0 against the float64-chained, once-rounded W_t in float32
        k = checks(c, np.zeros((c["B"], m["H"], m["N"]), np.float32))[0]
        v = k["A"] @ k["W"].T
        if k["bias"] is not None:
            v = v + k["bias"]
        return (v * k["std"] + k["mean"]).astype(np.float32).reshape(c["B"], m["H"], m["N"])
    x = R.time_delay_embedding(m["z"], m["panel"][0]) if m["panel"] else m["x"]   # (most recent lag first)
    return R.rollout(oracle_spec(m), x, m["H"], m["N"], m["mean"], m["std"], bf16=c["dtype"] == "bf16")


def shrink32(x, thr):
    """shrink_kernel in float32, bit for bit: one rounding of |x| - thr."""
    av = np.abs(x) - np.float32(thr)
    return np.where(av > 0, np.copysign(av, x), np.float32(0) * x).astype(np.float32)


def checks(c, y):
    """yhat [B, H, N] of the cell's model cut into GEMM problems: dicts of A [M, K], W [n, K], bias, epi
    (+ R, thr / mean, std), out [M, n] and cols (the output columns that out shows)."""
    m = model(c)
    st, H = c["stage"], m["H"]
    rnd = R.bf16_round if c["dtype"] == "bf16" else (lambda a: a)
    base = dict(bias=None, epi=c["epi"].split(":")[0], act=c["epi"].split(":")[-1], cols=None, label=c["id"])
    if st == "enc":
        W = m["enc"][0][0]
        if m["panel"]:      # rollout_panel reverses the lag blocks of the first layer
            d, Na = m["panel"]
            W = W.reshape(W.shape[0], d, Na)[:, ::-1].reshape(W.shape[0], -1)
        return [dict(base, A=m["x"], W=W, bias=m["enc"][0][1], out=y[:, 0], cols=m["cols"], same=[y[:, t] for t in range(1, H)])]
    if st == "dec":
        W, b = m["dec"][0]
        return [dict(base, A=rnd(m["x"][:, :c["K"]]), W=rnd(W), bias=b, out=y[:, 0], mean=m["mean"], std=m["std"],
                     same=[y[:, t] for t in range(1, H)])]
    if st == "step":
        Wt = np.ascontiguousarray(m["kmat"].T)
        return [dict(base, epi="none", A=m["x"] if t == 0 else y[:, t - 1], W=Wt, out=y[:, t], label=f"{c['id']} step {t}")
                for t in range(H)]
    if st == "powers":
        D, b = m["dec"][0]
        Kt64, w, Ws = m["kmat"].astype(np.float64).T, D.astype(np.float64), []
        for _ in range(H):
            w = w @ Kt64                     # W_t = W_{t-1} K^T in float64, rounded once per step
            Ws.append(w.astype(np.float32))
        tile = lambda v: None if v is None else np.tile(v, H)   # noqa: E731
        return [dict(base, A=m["x"][:, :c["K"]], W=np.concatenate(Ws), bias=tile(b), mean=tile(m["mean"]), std=tile(m["std"]),
                     out=y.reshape(y.shape[0], -1))]
    if st == "lista":
        z0 = shrink32(m["x"], m["thr"])
        if not m["loops"]:
            return [dict(base, epi="exact", ref=z0, out=y[:, 0])]
        return [dict(base, A=z0, W=np.ascontiguousarray(m["S"].T), R=m["x"], thr=m["thr"], out=y[:, 0])]
    if st == "ball":
        return [dict(base, epi="ball", A=m["x"], out=y[:, 0])]
    raise ValueError(st)


def _erf(x):
    from scipy.special import erf
    return erf(x)


def _act64(v, act):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "tanh":
        return np.tanh(v)
    return 0.5 * v * (1.0 + _erf(v / np.sqrt(2.0)))


def _act32(v, act):
    """numpy's float32 function (the reference's own error in the activation)."""
    v = v.astype(np.float32)
    if act == "tanh":
        return np.tanh(v)
    return np.float32(0.5) * v * (np.float32(1) + _erf(v * np.float32(0.70710678118654752)).astype(np.float32))


GELU_LIP = 1.13    # max |gelu'|


def expected(k):
    """Float64 answer of one problem: (ref, s, gain, allow) per element. s = sum_k |a||w| + |bias|
    (+ |addend|) is the scale of the accumulation error, gain the factor by which the epilogue passes
    it on, allow the epilogue's own roundings:
      none / relu   nothing
      tanh, gelu    4 x what numpy's float32 function loses against float64 on the same arguments, in
                    units of u |tanh v| and u |v| (gelu's 1 + erf cancels for v < 0: its error scales
                    with |v|, not with the result)
      shrink        one ulp of the result (the one rounding of |v| - thr)
      destd         one ulp of |y std| and one of the result (one rounding each)"""
    A, W = k["A"].astype(np.float64), k["W"].astype(np.float64)
    v = A @ W.T
    s = np.abs(A) @ np.abs(W).T
    if k["bias"] is not None:
        v += k["bias"].astype(np.float64)
        s += np.abs(k["bias"].astype(np.float64))
    if k["cols"] is not None:
        v, s = v[:, k["cols"]], s[:, k["cols"]]
    gain, allow, epi = 1.0, 0.0, k["epi"]
    if epi == "act":
        ref = _act64(v, k["act"])
        if k["act"] != "relu":
            v32 = v.astype(np.float32)
            f64 = _act64(v32.astype(np.float64), k["act"])
            scale = np.abs(f64) if k["act"] == "tanh" else np.abs(v32.astype(np.float64))
            c_act = 4.0 * float((np.abs(_act32(v32, k["act"]).astype(np.float64) - f64) / (U * scale)).max())
            k["c_act"] = c_act
            allow = c_act * U * (np.abs(ref) if k["act"] == "tanh" else np.abs(v))
            gain = 1.0 if k["act"] == "tanh" else GELU_LIP
    elif epi == "shrink":
        R64 = k["R"].astype(np.float64)
        v, s = v + R64, s + np.abs(R64)
        ref = np.sign(v) * np.maximum(np.abs(v) - np.float64(np.float32(k["thr"])), 0.0)
        allow = 2 * U * np.abs(ref)
    elif epi == "destd":
        sd, mu = k["std"].astype(np.float64), k["mean"].astype(np.float64)
        ref = v * sd + mu
        gain = np.abs(sd)
        allow = 2 * U * np.abs(v * sd) + 2 * U * np.abs(ref)
    else:
        ref = v
    return ref, s, gain, allow


def _rows_sample(M, tm, cap=384):
    """Rows on which the CPU restatements are taken: all if few, else an even sample and the last tile."""
    if M <= cap:
        return np.arange(M)
    return np.unique(np.concatenate([np.linspace(0, M - 1, cap).astype(int), np.arange((M - 1) // tm * tm, M)]))


def restatement_k(k, tile, width):
    """k_max, k_rms of one problem from the reference's own error: two float32 restatements of the
    accumulation (numpy's float32 matrix product; a strictly sequential float32 sum over k) against
    float64, on a row sample; per region {name: (max ratio, rms ratio)} of the larger of the two."""
    A, W = k["A"], k["W"]
    M, n = A.shape[0], W.shape[0]
    rows = _rows_sample(M, tile[0])
    A = np.ascontiguousarray(A[rows])
    v64 = A.astype(np.float64) @ W.astype(np.float64).T
    s = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    b = k["bias"]
    r1 = A @ W.T
    r2 = np.zeros((len(rows), n), np.float32)
    Wt = np.ascontiguousarray(W.T)
    for j in range(A.shape[1]):
        r2 += A[:, j:j + 1] * Wt[j:j + 1]
    if b is not None:
        v64, s, r1, r2 = v64 + b.astype(np.float64), s + np.abs(b.astype(np.float64)), r1 + b, r2 + b
    if k["epi"] == "shrink":
        Rr = k["R"][rows]
        v64, s, r1, r2 = v64 + Rr.astype(np.float64), s + np.abs(Rr.astype(np.float64)), r1 + Rr, r2 + Rr
    ok = s > 0
    rho = [np.where(ok, np.abs(r.astype(np.float64) - v64) / np.where(ok, U * s, 1.0), 0.0) for r in (r1, r2)]
    masks = region_masks(M, n, tile, width, rows)
    out = {}
    for name, (rm, cm) in masks.items():
        sub = [r[np.ix_(rm, cm)] for r in rho]
        out[name] = (max(float(x.max()) for x in sub), max(float(np.sqrt((x ** 2).mean())) for x in sub))
    return out


def region_masks(M, n, tile, width, rows=None):
    """Row and column masks of 'whole', 'last row tile' and 'last column tile' (the ragged ones only);
    width > n where the columns shown are those of a wider launch (never ragged then)."""
    tm, tn = tile
    r = np.arange(M) if rows is None else rows
    allc = np.ones(n, bool)
    out = {"whole": (np.ones(len(r), bool), allc)}
    if M % tm:
        out["last row tile"] = (r >= M // tm * tm, allc)
    if width is None and n % tn:
        out["last column tile"] = (np.ones(len(r), bool), np.arange(n) >= n // tn * tn)
    return out


def ball_bound(L):
    """Relative error bound (in u) of norm(norm(x)) in float32, element by element: a sum of squares of at
    most ceil(L / 8) terms per lane and up to six shuffle adds ((ceil(L / 8) + 7) u with the squares'
    roundings), halved by the square root, one rounding each for the root and the division; the second
    norm passes the first's error on through numerator and norm."""
    one = (-(-L // 8) + 7) / 2.0 + 2.0
    return 3.0 * one


def judge(c, k, kernel=None, quiet=False):
    """Apply the bound to one problem. Returns {region: rms of e / (u s)}; raises AssertionError naming the
    kernel, the epilogue and the region: an element in the interior, the last ragged row tile or the last
    ragged column tile; an rms over the whole output or one of those tiles. The
    name is the probed launch's: a defect in one of the cell's identity stages fails the cell under that
    name too, and then the cells that probe the defective kernel fail beside it."""
    kernel = kernel or c["kernel"]
    what = f"{kernel}/{c['epi']} {k['label']}"
    out = k["out"].astype(np.float64)
    for o in k.get("same", ()):      # the same launch on the same operands (a later step): bit-identical
        assert np.array_equal(o, k["out"]), f"{what}: a later step differs from step 0"
    if k["epi"] == "exact":
        assert np.array_equal(k["out"], k["ref"]), f"{what}: not bit-identical to float32 shrink"
        return {}
    if k["epi"] == "ball":
        x = k["A"].astype(np.float64)
        ref = x / np.linalg.norm(x, axis=1, keepdims=True)
        r = float((np.abs(out - ref) / (U * np.abs(ref))).max())
        bound = ball_bound(x.shape[1])
        if not quiet:
            print(f"[ball] {what} max {r:.2f} u (bound {bound:.1f})")
        assert r <= bound, f"{what}: {r:.2f} u |ref| > {bound:.1f}"
        return {}
    ref, s, gain, allow = expected(k)
    tile = tile_of(kernel)
    width = None if k["cols"] is None or len(k["cols"]) == k["W"].shape[0] else k["W"].shape[0]
    ks = restatement_k(dict(k, A=k["A"], W=k["W"] if k["cols"] is None else k["W"][k["cols"]],
                            bias=k["bias"] if k["bias"] is None or k["cols"] is None else k["bias"][k["cols"]]), tile, width)
    k_max = 4.0 * ks["whole"][0]
    k_rms = 3.0 * ks["whole"][1]
    assert k_max <= K_MAX_CAP and k_rms <= K_RMS_CAP, f"{what}: the inputs need k_max {k_max:.1f}, k_rms {k_rms:.2f}"
    planes = kernel.startswith("x3_") or kernel == "latx3"
    ok = s > 0
    e = np.abs(out - ref)
    assert (e[~ok] == 0).all(), f"{what}: nonzero where every product is zero"
    den = np.where(ok, U * s * gain, 1.0)
    rho = np.where(ok, np.maximum(e - allow, 0.0) / den, 0.0)
    raw = np.where(ok, e / den, 0.0)       # with the epilogue's own roundings: plane against f32-input kernel
    M, n = rho.shape
    rms, fails = {}, []
    masks = region_masks(M, n, tile, width)
    bar_max = k_max + (X3_EXTRA if planes else 0.0)
    for name, (rm, cm) in masks.items():
        # the element test on disjoint regions (the interior is the output without its ragged tiles), the
        # rms over the whole output and over each ragged tile
        em = np.outer(rm, cm)
        if name == "whole":
            for other, (r2, c2) in masks.items():
                if other != "whole":
                    em &= ~np.outer(r2, c2)
        mx = float(rho[em].max()) if em.any() else 0.0
        sub = rho[np.ix_(rm, cm)]
        rr = float(np.sqrt((sub ** 2).mean()))
        rms[name] = float(np.sqrt((raw[np.ix_(rm, cm)] ** 2).mean()))
        bar_rms = 3.0 * max(ks["whole"][1], ks[name][1])
        if not quiet:
            print(f"[k] {what} [{'interior' if name == 'whole' else name}] max {mx:.2f} (bar {bar_max:.1f}) "
                  f"[{'whole output' if name == 'whole' else name}] rms {rr:.3f} (bar {bar_rms:.2f})"
                  + (f" c_act {k['c_act']:.2f}" if "c_act" in k else ""))
        if mx > bar_max:
            i, j = np.unravel_index(np.argmax(np.where(em, rho, -1.0)), rho.shape)
            fails.append(f"{what} [{'interior' if name == 'whole' else name}]: element ({i}, {j}) off by {mx:.1f} u s "
                         f"> {bar_max:.1f}")
        if rr > bar_rms:
            fails.append(f"{what} [{'whole output' if name == 'whole' else name}]: rms {rr:.3f} u s > {bar_rms:.2f}")
    assert not fails, "; ".join(fails)
    return rms


def compare_planes(c, k, rms, f32_rms):
    """The project's rule for the three-plane kernels (test_fp32_gemm_forms_against_float64): an fp32 GEMM
    in accuracy, rms within 1.5 x the f32-input kernel's on the same cell, region by region."""
    fails = [f"{c['kernel']}/{c['epi']} {k['label']} [{'whole output' if name == 'whole' else name}]: rms {r:.3f} > "
             f"1.5 x the f32-input kernel's {f32_rms[name]:.3f}" for name, r in rms.items() if r > PLANE_VS_F32 * f32_rms[name]]
    assert not fails, "; ".join(fails)
