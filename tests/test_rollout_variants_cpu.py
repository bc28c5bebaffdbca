"""The matrix of tests/rollout_variants.py without a GPU: its mirror of the rollout's dispatch is pinned
to the constants of kmpc_rollout.hip, its cells probe every kernel, every epilogue of every fp32 GEMM
form, both sides of every threshold and the edge shapes, and the float64 reference with its bound
passes on float32 CPU restatements of every cell, so the inputs are known good before a GPU sees them."""
import os
import re

import numpy as np
import pytest
import torch

import rollout_variants as rv
from koopman_mpc_portfolio_rebalancing_amd import DeviceKoopman, KoopmanModelSpec, _lib
from oracle import rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "koopman_mpc_portfolio_rebalancing_amd", "csrc")
SRC = "".join(open(os.path.join(CSRC, f)).read() for f in ("kmpc_rollout_gemm.h", "kmpc_rollout_latent.h", "kmpc_rollout.hip"))
# the compile-time switches the rollout once had: the first row's were pinned to "on" (KMPC_F32_GEMM to
# the three-plane form) and are gone with their other side, the second row's values are constexpr now
REMOVED = ("KMPC_LATPOW", "KMPC_LATX3", "KMPC_Z0_FUSE", "KMPC_BF16_SPLITK", "KMPC_BF16_SMALL", "KMPC_F32_GEMM",
           "KMPC_GEMM_MID", "KMPC_GEMM_BIG", "KMPC_GEMM_BK1", "KMPC_X3_TIMING", "KMPC_X3_DB", "KMPC_LAT_WAVES",
           "KMPC_LAT16_MAXB", "KMPC_LATPOW_MINB", "KMPC_LAT16_WAVES", "KMPC_F32_SPLITK", "KMPC_BF16_SPLIT_MINK")


def _const(name):
    """The value of 'constexpr int NAME = value;' (a product of integers; size_t too), defined once in the
    rollout's three files."""
    m = re.findall(r"^constexpr (?:int|size_t) %s = (?:\(size_t\))?([0-9* ]+);" % name, SRC, re.M)
    assert len(m) == 1, (name, m)
    return int(np.prod([int(t) for t in m[0].split("*")]))


def test_mirror_constants_equal_the_librarys():
    assert rv.LAT16_MAXB == _const("LAT16_MAXB")
    assert rv.LATPOW_MINB == _const("LATPOW_MINB")
    assert rv.LAT16_WAVES == _const("LAT16_WAVES")
    assert rv.F32_SPLITK == _const("F32_SPLITK")
    assert rv.BF16_SPLIT_MINK == _const("BF16_SPLIT_MINK")
    assert rv.SPLITK_ELEMS == _const("SPLITK_ELEMS")
    assert rv.BF16_SPLIT == _const("SPLITK_BUF")
    # no switch is left: the names are gone, and nothing in the three files can be set from the command line
    for name in REMOVED:
        assert not re.search(r"\b%s\b" % name, SRC), name
    assert not re.search(r"#\s*(define|ifndef|ifdef|if)\b", SRC)
    # dtype fp32 is the three-plane form, fp32_f32mfma the run-time selector of the other
    assert "g.bf16 = r.dtype == KMPC_DTYPE_F32 ? 2 : r.dtype == KMPC_DTYPE_BF16 ? 1 : 0;" in SRC
    assert re.search(r"if \(g\.bf16 == 2\)\s+hipLaunchKernelGGL\(\(gemm_nt_x3_kernel<", SRC)
    # the tile-count thresholds of route_gemm() and the K bound of the fp32 split
    assert rv.BIG_TILES == _const("BIG_TILES")
    assert rv.SPLIT_TILES64 == _const("SPLIT_TILES64")
    assert rv.BF16_FEW == _const("BF16_FEW")
    assert "const size_t t128 = (size_t)((N + 127) / 128) * ((M + 127) / 128);" in SRC
    assert "const size_t t64 = (size_t)((N + 63) / 64) * ((M + 63) / 64);" in SRC
    assert "const bool few = t128 < BF16_FEW;" in SRC
    assert "if (few && have_part && K >= BF16_SPLIT_MINK && (size_t)M * N <= SPLITK_ELEMS)" in SRC
    assert "return {dtype, TILE_128, SPLITK_BUF, TAIL_EPILOGUE};" in SRC
    assert "return {dtype, few ? TILE_64 : TILE_128, 1, TAIL_NONE};" in SRC          # (the 64-square tile is on)
    assert "if (have_part && t64 < SPLIT_TILES64 && K >= 128 * F32_SPLITK)" in SRC
    # the two forms of the ladder: 16 waves of 32 x 32 below BIG_TILES, 8 waves of 32 x 64 from there
    m = re.search(r"if \(t128 < BIG_TILES\) \{\n(?:.*\n){2}\s+return \{dtype, TILE_128_(\d+), 1, TAIL_NONE\};\n    \}\n"
                  r"    return \{dtype, TILE_128_(\d+), 1, TAIL_NONE\};", SRC)
    assert (rv.GEMM_MID, rv.GEMM_BIG) == (int(m.group(1)), int(m.group(2)))
    assert re.search(r"r\.tile == TILE_64\) \{\s+launch_f32<1, 1, 2, 2>\(", SRC)
    assert re.search(r"r\.tile == TILE_128_44\) \{\s+launch_f32<1, 1, 4, 4>\(", SRC)
    assert re.search(r"\} else \{\s+launch_f32<1, 2, 4, 2>\(", SRC)
    # latent_fusable, the 16-row loop's reach, the three-plane loop's latent, the powers, and z0 as partials
    assert (rv.FUSE_L_MULT, rv.FUSE_L_MAX) == (_const("FUSE_L_MULT"), _const("FUSE_L_MAX"))
    assert "d->L % FUSE_L_MULT == 0 && d->L <= FUSE_L_MAX" in SRC
    assert "const bool lat16 = fus && (B < LAT16_MAXB || L <= 16 * LAT16_WAVES);" in SRC
    assert "const bool kdir = lat16 && B < LAT16_MAXB;" in SRC
    assert rv.LATX3_L == _const("LATX3_L")
    assert ": d->dtype == KMPC_DTYPE_F32 && !p.ball && L == LATX3_L ? LOOP_LATX3 : LOOP_LAT32;" in SRC
    assert "latent_steps_x3_kernel<8, LATX3_L>" in SRC
    assert ("const bool latpow = d->latent_unfused == KMPC_LATENT_AUTO && fus && B >= LATPOW_MINB && !p.ball;"
            in SRC)                                                                   # (the powers are on)
    assert "p.loop = latpow ? LOOP_POWERS : !fus ? LOOP_STEPS : lat16 ? (kdir ? LOOP_LAT16_KDIR : LOOP_LAT16_KT)" in SRC
    assert "p.zfuse = p.fused && d->model_kind == KMPC_MODEL_GENERIC && !p.ball;" in SRC   # (z0 as partials is on)


def _probes():
    """kernel -> set of (epilogue, bias, cell id) over the probed launches of the matrix."""
    seen = {k: set() for k in rv.KERNELS}
    for c in rv.CELLS:
        for kern, epi, M, N, K in rv.probed(c):
            seen[kern].add((c["epi"] if epi == "parts" else epi, c["bias"], c["id"]))
    return seen


def test_cells_are_what_they_say():
    """Each cell's plan runs, at its probed stage, the kernel, tail and epilogue the cell is there for."""
    ids = [c["id"] for c in rv.CELLS]
    assert len(set(ids)) == len(ids)
    for c in rv.CELLS:
        p = rv.probed(c)
        assert p, c["id"]
        gem = [g for g in p if g[0] != "powers"]
        assert gem[0][0] == c["kernel"], (c["id"], p)
        assert gem[-1][1] == c["epi"], (c["id"], p)
        split = len(gem) == 2
        assert split == (c["tail"] is not None) and (not split or gem[1][0] == c["tail"]), (c["id"], p)
        if c["stage"] == "powers":
            assert p[0][0] == "powers"


def test_the_probed_launches_cover_every_kernel():
    assert len(rv.KERNELS) == 18 == len(set(rv.KERNELS))
    seen = _probes()
    assert set(seen) == set(rv.KERNELS)
    for k in rv.KERNELS:
        assert seen[k], f"no cell probes {k}"


def test_every_epilogue_of_every_fp32_gemm_form():
    seen = _probes()
    for k in rv.GEMMS_F32:
        epis = {e for e, _, _ in seen[k]}
        assert {"none", "shrink", "destd", "act:relu", "act:tanh", "act:gelu"} <= epis, (k, epis)
        assert {b for _, b, _ in seen[k]} == {True, False}, k
        for e in ("act:relu", "destd"):              # (the LISTA addend stands where a bias would)
            assert any(b for ee, b, _ in seen[k] if ee == e), (k, e)
    assert {e.split(":")[0] for e, _, _ in seen["splitk_epi"]} == set(rv.EPILOGUES)
    for k in rv.GEMMS_BF16:
        assert "destd" in {e for e, _, _ in seen[k]}


def _cells_with(**kw):
    return [c for c in rv.CELLS if all(c[k] == v for k, v in kw.items())]


def _gemm_shape(c):
    g = [g for g in rv.probed(c) if g[0] not in ("powers",)][0]
    return g[2:]


def test_every_threshold_has_a_cell_on_each_side():
    kern = lambda B, L, form, **kw: [c["kernel"] for c in _cells_with(stage="step", B=B, n=L, form=form, **kw)]   # noqa: E731
    # 8,191 and 8,192 windows: the 16-row loop in place / the powers GEMM ('auto'), the K^T loop ('sequential')
    assert kern(8191, 128, "auto") == ["lat16_kdir"]
    assert [c["kernel"] for c in _cells_with(stage="powers", B=8192, K=128)] == ["x3_mid44", "f32_mid44"]
    assert [c["tail"] for c in _cells_with(stage="enc", B=8192, form="sequential")] == ["raw_parts"] * 2
    # 511 / 512 128-square tiles, 255 / 256 64-square tiles
    tiles = lambda c, t: rv._ceil(_gemm_shape(c)[0], t) * rv._ceil(_gemm_shape(c)[1], t)   # noqa: E731
    f32 = [c for c in rv.CELLS if c["kernel"].startswith(("x3_", "f32_"))]
    for pre in ("x3_", "f32_"):
        assert any(tiles(c, 128) == 511 and c["kernel"] == pre + "mid44" for c in f32)
        assert any(tiles(c, 128) == 512 and c["kernel"] == pre + "big42" for c in f32)
        assert any(tiles(c, 64) == 255 and c["kernel"] == pre + "split64" for c in f32)
        assert any(tiles(c, 64) == 256 and _gemm_shape(c)[2] >= 512 and c["kernel"] == pre + "mid44" for c in f32)
        # K = 511 / 512 of the fp32 split
        assert any(_gemm_shape(c)[2] == 511 and tiles(c, 64) < 256 and c["kernel"] == pre + "mid44" for c in f32)
        assert any(_gemm_shape(c)[2] == 512 and c["kernel"] == pre + "split64" for c in f32)
    # K = 2,047 / 2,048 of the bf16 split
    assert [c["kernel"] for c in _cells_with(dtype="bf16", K=2047)] == ["bf16_64"]
    assert [c["kernel"] for c in _cells_with(dtype="bf16", K=2048)] == ["bf16_split8"]
    # L = 128 / 160 from 8,192 windows, L = 512 / 544, L = 48, a two-layer decoder
    assert kern(8193, 128, "sequential") == ["lat16_kt"] and kern(8193, 160, "sequential") == ["lat32"]
    assert kern(8193, 512, "sequential") == ["lat32"] and kern(300, 512, "auto") == ["lat16_kdir"]
    assert kern(300, 544, "auto") == ["x3_split64", "f32_split64"]
    assert kern(1000, 48, "auto") == ["x3_mid44", "f32_mid44"]
    two = [c for c in rv.CELLS if c["stage"] == "dec" and c["act"] and c["form"] == "auto"]
    assert two and all(c["kernel"].startswith(("x3_", "f32_")) for c in two)       # 'auto', yet per-step GEMMs
    # the loops the issue found untested
    assert kern(8200, 384, "sequential", dtype="fp32_f32mfma") == ["lat32"]
    assert kern(8225, 256, "sequential", dtype="fp32_f32mfma") == ["lat32"]
    assert kern(8257, 256, "sequential") == ["latx3"]


def test_the_edge_shapes_are_cells():
    shapes = {_gemm_shape(c) for c in rv.CELLS if c["kernel"] in rv.GEMMS_F32 + rv.GEMMS_BF16}
    Ms, Ns, Ks = ({s[i] for s in shapes} for i in range(3))
    assert 1 in Ms and any(1 < M < 64 or 64 < M < 128 for M in Ms)
    assert any(M % 128 for M in Ms) and any(M % 64 for M in Ms)
    assert {1, 33, 100} <= Ns
    assert any(K < 32 for K in Ks) and any(K % 32 for K in Ks) and any(K % 4 for K in Ks)
    panels = {c["panel"][1] for c in rv.CELLS if c["panel"]}
    assert any(Na % 4 == 0 for Na in panels) and any(Na % 2 for Na in panels)
    loopB = {k: {c["B"] for c in rv.CELLS if c["kernel"] == k} for k in ("lat16_kdir", "lat16_kt", "lat32", "latx3")}
    assert any(B % 16 == 1 for B in loopB["lat16_kdir"] | loopB["lat16_kt"])
    assert any(B % 32 == 1 for B in loopB["lat32"]) and any(B % 64 == 1 for B in loopB["latx3"])


def test_raw_parts_reaches_both_16_row_loops():
    after = set()
    for c in _cells_with(tail="raw_parts"):
        a, kw = rv.plan_args(c)
        p = rv.plan(*a, **kw)
        i = [g[0] for g in p].index("raw_parts")
        after.add(p[i + 1][0])
    assert after == {"lat16_kdir", "lat16_kt"}


def test_plan_of_the_bench_shapes():
    """The mirror on the shapes whose launches DESIGN 3.1 names: C3 at 65,536 windows, configs[1] at 4,096."""
    k = [g[0] for g in rv.plan(65536, 2000, [1024, 1024, 256], 256, 100, 10)]
    assert k == ["x3_big42", "x3_big42", "x3_big42", "powers", "x3_big42"]
    k = [g[0] for g in rv.plan(65536, 2000, [1024, 1024, 256], 256, 100, 10, form="sequential")]
    assert k == ["x3_big42", "x3_big42", "x3_big42", "latx3"]
    k = [g[0] for g in rv.plan(4096, 600, [1024, 1024, 128], 128, 30, 5)]
    assert k == ["x3_mid44", "x3_mid44", "x3_split64", "raw_parts", "lat16_kdir"]
    k = [g[0] for g in rv.plan(1024, 10000, [512], 512, 500, 20, kind="lista", dtype="bf16", lista_loops=10)]
    assert k == ["bf16_split8", "splitk_epi", "shrink"] + ["bf16_64"] * 10 + ["bf16_64", "bf16_64"] * 20


@pytest.mark.parametrize("c", rv.CELLS, ids=[c["id"] for c in rv.CELLS])
def test_reference_and_bound_pass_on_the_cpu_restatement(c):
    """yhat of the cell's model by the numpy float32 restatement of the whole rollout (oracle/rollout.py:
    the identity stages are exact there as on the device), cut into problems and judged as the device's
    will be: the float64 reference, the scale, the epilogue allowances and k_max <= 32, k_rms <= 2 hold."""
    y = rv.numpy_rollout(c)
    m = rv.model(c)
    assert y.shape == (c["B"], m["H"], m["N"]) and np.isfinite(y).all()
    for k in rv.checks(c, y):
        rv.judge(c, k)


def test_judge_rejects_a_dropped_term_and_a_dropped_plane_pair():
    """The bound at work on the CPU: one k term missing from one output element fails the element test
    in the interior or in the ragged tile it sits in; a three-plane product without its hi.lo pairs
    fails the rms test (and passes every bar of test_rollout_gpu.py: 5e-7 normwise)."""
    c = rv.BY_ID["dec_tanh_B1000_n200_K99-x3_mid44"]
    y = rv.numpy_rollout(c).copy()
    m = rv.model(c)
    W = m["dec"][0][0]
    pre = np.arctanh(np.clip(y[999, 0, 199].astype(np.float64), -0.999, 0.999))
    y[999, 0, 199] = np.tanh(pre - float(m["x"][999, 98]) * float(W[199, 98]))
    with pytest.raises(AssertionError, match=r"x3_mid44/act:tanh .*\[last (row|column) tile\]: element \(999, 199\)") as ei:
        rv.judge(c, rv.checks(c, y)[0], quiet=True)
    assert "[interior]" not in str(ei.value)
    # hi.lo and lo.hi dropped: a . b - (a_hi b_lo + a_lo b_hi)
    c = rv.BY_ID["step_unfused_B1000_L96-x3_mid44"]
    m = rv.model(c)

    def split(x):
        hi = R.bf16_round(x)
        mid = R.bf16_round(x - hi)
        return hi.astype(np.float64), mid.astype(np.float64), (x - hi - mid).astype(np.float64)

    a, b = split(m["x"]), split(np.ascontiguousarray(m["kmat"].T))
    z = (m["x"].astype(np.float64) @ m["kmat"].astype(np.float64) - a[0] @ b[2].T - a[2] @ b[0].T).astype(np.float32)
    k = dict(rv.checks(c, np.stack([z, z], 1))[0])
    ref = m["x"].astype(np.float64) @ m["kmat"].astype(np.float64)
    assert np.abs(z - ref).max() / np.abs(ref).max() < 1e-5          # inside the normwise bar of test_rollout_gpu.py
    with pytest.raises(AssertionError, match=r"x3_mid44/none .*whole output.*rms"):
        rv.judge(c, k, quiet=True)


# ---- KoopmanModelSpec / DeviceKoopman: fuse_latent ------------------------------------------------
def _tiny_spec():
    return KoopmanModelSpec(kind="generic", encoder=[(torch.eye(4), None)], kmat=torch.eye(4), decoder=[(torch.eye(4), None)])


def test_spec_has_no_fuse_latent():
    """The latent form is a property of the device model, not of the spec (the spec's property read a
    field the dataclass never had)."""
    spec = _tiny_spec()
    assert not hasattr(spec, "fuse_latent") and not hasattr(KoopmanModelSpec, "fuse_latent")
    assert not hasattr(spec, "latent_form")


def test_device_model_fuse_latent_false_means_unfused():
    km = DeviceKoopman.__new__(DeviceKoopman)
    try:
        km.__init__(_tiny_spec(), fuse_latent=False, latent_form="sequential")
    except _lib.KmpcError:
        pass                                   # no GPU: raised after the latent form is settled
    assert km.latent_form == "unfused" and km.fuse_latent is False
    assert _lib.LATENT_FORM[km.latent_form] == 1 == int(re.search(r"#define KMPC_LATENT_UNFUSED\s+(\d+)", open(
        os.path.join(ROOT, "include", "kmpc.h")).read()).group(1))
    km.fuse_latent = True
    assert km.latent_form == "auto" and km.fuse_latent is True
    with pytest.raises(ValueError):
        DeviceKoopman(_tiny_spec(), latent_form="fused")
