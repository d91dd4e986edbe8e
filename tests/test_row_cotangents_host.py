"""The per-row oracle (tests/row_cotangents.py) held to itself, on the CPU: its per-row cotangents reproduce its own parameter
gradients in float64, its float32 run is off its float64 run on a handful of rows only, and the library's view of the gradient
workspace (dsn_grad_workspace_layout, a host function) is the layout the older readers of that workspace assumed."""
import ctypes as C

import numpy as np
import pytest
import torch

import row_cotangents as RC


def test_float64_row_cotangents_reproduce_the_parameter_gradients():
    """37 x 100 with noise, float64: bias = column sum of the layer's per-row cotangent, weight = cotangent^T input rows, for the three
    lighting layers, the colour head's two layers and the density head's bias - to 1e-12 relative.  This pins the node each device
    array is compared with (row_cotangents' table): a cotangent taken on the wrong side of a ReLU or of the transparent mask breaks
    the identity of its layer"""
    name, R, S, noise = RC.CASES["37x100"]
    o = RC.oracle_rows(name, R, S, noise, torch.float64)
    assert o["noise"] is not None
    P = RC.products({**o["cot"], **o["rows"]}, np.arange(R * S))
    assert len(P) == 11
    for k, v in P.items():
        want = o["grads"][k]
        assert v.shape == want.shape, (k, v.shape, want.shape)
        assert np.linalg.norm(want) > 0, k
        assert np.linalg.norm(v - want) <= 1e-12 * np.linalg.norm(want), (k, np.linalg.norm(v - want) / np.linalg.norm(want))
    # d_xl[:, :3] is d n_w: the lighting input's first three columns ARE the normal
    assert np.array_equal(o["rows"]["xl"][:, :3], o["rows"]["n_w"])
    # transparent rows: no cotangent reaches the density head, whatever the noise lets through
    assert o["transparent"].any() and not np.any(o["cot"]["d_sig"][o["transparent"]])


@pytest.mark.parametrize("cid", list(RC.CASES))
def test_float32_oracle_is_off_on_a_handful_of_rows_only(cid):
    """the set-aside rule on the float32 oracle alone: the rows on which it is off its float64 run (ROW_REL of the row, ROW_FLOOR of the
    array) are at most SET_ASIDE_CAP of its live rows - and with noise off there is none"""
    name, R, S, noise = RC.CASES[cid]
    o32, o64 = RC.oracle_rows(name, R, S, noise, torch.float32), RC.oracle_rows(name, R, S, noise, torch.float64)
    live = RC.oracle_live_rows(o32)
    aside, per = RC.set_aside(o32, o64, live)
    n = int(aside.sum())
    noise_only = int(o32["transparent"][live[aside]].sum())
    print(f"row_cotangents_host: {cid}: {n} of {len(live)} live rows set aside ({n / len(live):.2e}; {noise_only} of them noise-only rows;"
          f" float64 live rows {len(RC.oracle_live_rows(o64))}); arrays: " + ", ".join(f"{k} {int(v.sum())}" for k, v in per.items() if v.any()))
    assert len(live) > 0
    assert n <= RC.SET_ASIDE_CAP * len(live), (cid, n, len(live))
    if not noise:
        assert n == 0, (cid, n)
    # every row the float32 run leaves out of its list has a float64 cotangent below float32's smallest normal (x a rounding factor)
    lost = np.setdiff1d(RC.oracle_live_rows(o64), live)
    cmax = max(1.0, max(float(np.abs(v).max()) for v in o32["cotangents"].values()))
    if len(lost):
        big = max(float(np.abs(o64["cot"]["d_col"][lost]).max()), float(np.abs(o64["cot"]["d_sig"][lost]).max()))
        assert big <= 4 * 2.0 ** -126 * cmax, (cid, big)


def test_workspace_layout_comes_from_the_library():
    """dsn_grad_workspace_layout (host function, no GPU): DSN_GRAD_WS_COUNT distinct 256-byte aligned offsets inside the workspace, arrays
    far enough apart for their rows, the two row counts where grad_row_counts has always read them (the 256 bytes in front of the
    last 4 KB), and loud argument errors"""
    from dsnerf_amd import _lib
    L = _lib.lib()
    n = len(_lib.GRAD_WS_ARRAYS)
    assert n == 26
    for R, S in ((37, 100), (128, 128), (1, 1), (8192, 64)):
        N = R * S
        off = _lib.grad_workspace_layout(R, S)
        need = L.dsn_grad_workspace_bytes(R, S)
        assert list(off) == [a[0] for a in _lib.GRAD_WS_ARRAYS]
        assert off["rowcnt"] == need - 4096 - 256
        assert off["transparent"] == 0
        ends = {}
        for name, dt, cols in _lib.GRAD_WS_ARRAYS:
            rows = 2 if name == "rowcnt" else N
            ends[name] = off[name] + rows * max(cols, 1) * torch.empty(0, dtype=dt).element_size()
            assert off[name] % 256 == 0 and ends[name] <= need, name
        spans = sorted((off[k], ends[k]) for k in off)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans      # no two arrays overlap
    buf = (C.c_int64 * n)()
    assert L.dsn_grad_workspace_layout(37, 100, buf, n - 1) != 0 and b"dsn_grad_workspace_layout" in L.dsn_last_error()
    assert L.dsn_grad_workspace_layout(0, 100, buf, n) != 0 and L.dsn_grad_workspace_layout(37, 100, None, n) != 0
