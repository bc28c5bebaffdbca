"""Record what the rollout's host path answers before any launch, over a grid of descriptors
-> tests/golden/host_codes_rollout.npz (not rollout_*.npz: the rollout tests take every file of that
pattern for a model with its reference yhat).

    python tests/golden/make_rollout_host_codes.py [--lib PATH/libkmpc.so] [--commit HASH]

Run once against the library of the commit whose behaviour is to be kept (HASH, default the checked
out HEAD, is written into the file); tests/test_rollout_host_cpu.py replays the file's rows against
the built library with host_codes() below and demands equality. Per row:

  ws_bytes   kmpc_workspace_bytes(rdesc, NULL)
  rc_b0      kmpc_rollout with B = 0 and a workspace of 2^62 bytes: every rule, then KMPC_OK
  rc_short   kmpc_rollout with the row's B and ws_bytes one byte short: KMPC_ERR_WORKSPACE, or the
             rule that fails ahead of the size check

All three return ahead of the first launch (and of any call into the HIP runtime), so no GPU is
needed; the pointers are non-null and never read. The model of a row: obs = 4 N, encoder widths
[obs, L] or [obs, 1024, L], decoder [L, obs] or [L, L, obs]."""
import argparse
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from koopman_mpc_portfolio_rebalancing_amd import _lib  # noqa: E402

OUT = os.path.join(HERE, "host_codes_rollout.npz")
COLS = ("B", "L", "N", "H", "enc_hidden", "dec_layers", "kind", "dtype", "latent", "obs_ld")
BS = (0, 1, 300, 8191, 8192, 70000)         # both sides of 8,192 windows
LS = (16, 48, 128, 256, 544)                # both sides of L % 32 and of L <= 512
NS = (1, 33, 100)
HS = (1, 10)
ENC_HIDDEN = (0, 1024)                      # encoder widths [L] / [1024, L]
DEC_LAYERS = (1, 2)
KINDS = (_lib.MODEL_GENERIC, _lib.MODEL_LISTA)
DTYPES = (0, 1, 2, 7)                       # the three KMPC_DTYPE_* and one that is none
LATENTS = (0, 1, 2, 3)                      # the three KMPC_LATENT_* and one out of range
OBS_LD = (0, 1, -1)                         # 0, N, N - 1 (as a code: 0, +1 -> N, -1 -> N - 1)
BIG = 1 << 62

_BUF = ctypes.create_string_buffer(256)
_P = (ctypes.addressof(_BUF) + 255) & ~255   # a non-null, 256-byte aligned address that no rule reads


def grid():
    a = np.array(list(itertools.product(BS, LS, NS, HS, ENC_HIDDEN, DEC_LAYERS, KINDS, DTYPES, LATENTS, OBS_LD)),
                 dtype=np.int32)
    g = {n: a[:, i].copy() for i, n in enumerate(COLS)}
    g["obs_ld"] = np.where(g["obs_ld"] == 0, 0, np.where(g["obs_ld"] == 1, g["N"], g["N"] - 1)).astype(np.int32)
    return g


def _mlp(dims):
    m = _lib.Mlp()
    m.n_layers = len(dims) - 1
    for i, w in enumerate(dims):
        m.dims[i] = w
    for i in range(m.n_layers):
        m.weight[i], m.bias[i] = _P, None
    return m


def host_codes(lib, g):
    """The three recorded answers for every row of g (columns COLS)."""
    n = len(g["B"])
    out = {k: np.zeros(n, np.int64) for k in ("ws_bytes", "rc_b0", "rc_short")}
    d = _lib.RolloutDesc()
    d.kmat = d.mean = d.std = d.lista_S = _P
    d.lista_loops, d.lista_thresh = 2, 0.125
    pd = ctypes.byref(d)
    for i in range(n):
        B, L, N = int(g["B"][i]), int(g["L"][i]), int(g["N"][i])
        obs, hid = 4 * N, int(g["enc_hidden"][i])
        d.N, d.H, d.L, d.obs = N, int(g["H"][i]), L, obs
        d.model_kind, d.norm_fn = int(g["kind"][i]), 0
        d.encoder = _mlp([obs] + ([hid] if hid else []) + [L])
        d.decoder = _mlp([L] + [L] * (int(g["dec_layers"][i]) - 1) + [obs])
        d.dtype, d.latent_unfused, d.obs_ld = int(g["dtype"][i]), int(g["latent"][i]), int(g["obs_ld"][i])
        d.B = B
        need = lib.kmpc_workspace_bytes(pd, None)
        out["ws_bytes"][i] = need
        out["rc_short"][i] = lib.kmpc_rollout(pd, _P, _P, _P, need - 1, None)
        d.B = 0
        out["rc_b0"][i] = lib.kmpc_rollout(pd, _P, _P, _P, BIG, None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                        text=True).stdout.strip()
    lib = _lib.load(a.lib)
    g = grid()
    c = host_codes(lib, g)
    data = {"commit": np.array(commit), "version": np.array(lib.kmpc_version().decode())}
    data.update(g)
    data.update(ws_bytes=c["ws_bytes"], rc_b0=c["rc_b0"].astype(np.int8), rc_short=c["rc_short"].astype(np.int8))
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: commit {commit}, {len(g['B'])} rows, {os.path.getsize(OUT)} bytes")
    for k in ("rc_b0", "rc_short"):
        print(f"  {k}: codes {dict(zip(*(x.tolist() for x in np.unique(c[k], return_counts=True))))}")
    print(f"  distinct workspace sizes: {len(np.unique(c['ws_bytes']))}")


if __name__ == "__main__":
    main()
