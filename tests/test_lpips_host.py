"""The LPIPS rule without a GPU: the restatement's own properties (tests/lpips_restate.py - tap shapes, the zero on identical images,
lin isolation, the eps placement, the recorded float64 values), the two state-dict layouts of dsnerf_amd.lpips, and the argument
checks of the entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lpips_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def W():
    return {net: R.make_weights(net) for net in ("alex", "vgg")}


def test_tap_shapes(W):
    import dsnerf_amd
    want = {"alex": (55, 27, 13, 13, 13), "vgg": (224, 112, 56, 28, 14)}
    for net in ("alex", "vgg"):
        shapes = R.tap_shapes(net, 224, 224)
        assert [s[0] for s in shapes] == list(R.TAP_CHANNELS[net])
        assert [s[1] for s in shapes] == list(want[net]) == [s[2] for s in shapes]
        assert dsnerf_amd._lib.lpips_tap_shapes(net, 224, 224) == shapes
        m = R.MIN_SIDE[net]
        small = R.tap_shapes(net, m, m + 1)
        assert small[-1][1:] == (1, 1) and dsnerf_amd._lib.lpips_tap_shapes(net, m, m + 1) == small
        assert dsnerf_amd._lib.lpips_tap_shapes(net, m - 1, m) is None
        # the restatement's convolutions give these shapes, and the layer below the smallest image fails in its pooling as the package's
        img = R.make_image(m, m + 1, 1)
        assert [tuple(t.shape[1:]) for t in R.features(net, W[net], img[None])] == small
        with pytest.raises(RuntimeError):
            R.features(net, W[net], R.make_image(m - 1, m, 1)[None])
    assert R.macs("vgg", 224, 224) == 15346630656 and R.macs("alex", 224, 224) == 655566528      # (the published 15.3 G / 0.66 G)


def test_identical_images_give_zero(W):
    for net in ("alex", "vgg"):
        img = R.make_image(40, 47, 2)
        out, layers = R.lpips(net, W[net], img[None], img[None].astype(np.float64))
        assert out[0] == 0.0 and not layers.any()


def test_one_hot_lin_isolates_its_channel(W):
    net = "alex"
    img, gt = R.make_pair(37, 53, 3)
    t0, t1 = R.features(net, W[net], img[None]), R.features(net, W[net], gt[None])
    for l in (0, 2, 4):
        c = int(((t0[l] - t1[l]) ** 2).mean((0, 2, 3)).argmax())      # (a live channel: some are dead behind the ReLU)
        lins = [np.zeros(n, np.float32) for n in R.TAP_CHANNELS[net]]
        lins[l][c] = 1.0
        out, layers = R.head(t0, t1, lins)
        n0 = t0[l] / (t0[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        n1 = t1[l] / (t1[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        want = float(((n0[:, c] - n1[:, c]) ** 2).mean())
        assert abs(float(out[0]) - want) <= 1e-15 and float(layers[0].sum() - layers[0, l]) == 0.0 and want > 0


def test_eps_sits_outside_the_root():
    z = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    f = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    f[0, 1] = 3e-6
    lin = [np.ones(4, np.float32)]
    out, _ = R.head([f], [z], lin)                      # a zero vector normalises to zero (no 0 / 0), the small one to 3e-6 / (3e-6 + 1e-10)
    assert np.isfinite(float(out[0])) and abs(float(out[0]) - (3e-6 / (3e-6 + 1e-10)) ** 2) < 1e-15
    inside, _ = R.head([f], [z], lin, variant="eps_inside")
    assert abs(float(inside[0]) - 9e-12 / (9e-12 + 1e-10)) < 1e-15 and float(inside[0]) < 0.1 < float(out[0])


def test_recorded_values_reproduce(W):
    with open(os.path.join(GOLDEN, "lpips_golden.json")) as f:
        gold = json.load(f)
    for net in ("alex", "vgg"):
        assert set(gold[net]) == {f"{H}x{W_}" for H, W_ in R.SIZES[net]} | {"512x512"}
        for H, W_ in R.SIZES[net][:3] + R.SIZES[net][-1:]:
            g = gold[net][f"{H}x{W_}"]
            img, gt = R.make_pair(H, W_, g["seed"])
            out, layers = R.lpips(net, W[net], img[None], gt[None])
            assert abs(out[0] - g["out"]) <= 1e-12 * g["out"], (net, H, W_)
            assert np.abs(layers[0] - np.array(g["layers"])).max() <= 1e-12 * g["out"]
            assert g["max_activation"] < 32.0
    with open(os.path.join(GOLDEN, "lpips_errors.json")) as f:
        err = json.load(f)
    for net in ("alex", "vgg"):                        # the float32 twin's own error: what the GPU bars are multiples of
        assert len(err[net]["tap"]) == 5 and all(1e-8 < e < 5e-6 for e in err[net]["tap"]) and 1e-9 < err[net]["scalar"] < 1e-6


def _layouts(net, w):
    from dsnerf_amd.lpips import FEATURE_INDEX, _slice_of
    package, feats, lins = {}, {}, {}
    for i, (cw, cb) in zip(FEATURE_INDEX[net], w["conv"]):
        package[f"net.slice{_slice_of(net, i)}.{i}.weight"] = feats[f"features.{i}.weight"] = torch.from_numpy(cw)
        package[f"net.slice{_slice_of(net, i)}.{i}.bias"] = feats[f"features.{i}.bias"] = torch.from_numpy(cb)
    for k, lw in enumerate(w["lin"]):
        t = torch.from_numpy(lw).reshape(1, -1, 1, 1)
        package[f"lin{k}.model.1.weight"] = package[f"lins.{k}.model.1.weight"] = lins[f"lin{k}.model.1.weight"] = t
    package["scaling_layer.shift"] = torch.tensor(R.SHIFT).view(1, 3, 1, 1)
    feats["classifier.0.weight"] = torch.zeros(2, 2)
    return package, feats, lins


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_both_state_dict_layouts_load_to_the_same_tensors(net, W):
    from dsnerf_amd.lpips import FEATURE_INDEX, load_weights, _slice_of
    assert FEATURE_INDEX == R.FEATURE_INDEX
    assert [_slice_of("alex", i) for i in FEATURE_INDEX["alex"]] == [1, 2, 3, 4, 5]
    assert [_slice_of("vgg", i) for i in FEATURE_INDEX["vgg"]] == [1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5]
    package, feats, lins = _layouts(net, W[net])
    a, b = load_weights(net, package), load_weights(net, (feats, lins))
    for (conv_a, lin_a), (conv_b, lin_b) in ((a, b),):
        for (wa, ba), (wb, bb), (w0, b0) in zip(conv_a, conv_b, W[net]["conv"]):
            assert torch.equal(wa, wb) and torch.equal(ba, bb) and np.array_equal(wa.numpy(), w0) and np.array_equal(ba.numpy(), b0)
        for la, lb, l0 in zip(lin_a, lin_b, W[net]["lin"]):
            assert la.shape == lb.shape == (l0.size,) and torch.equal(la, lb) and np.array_equal(la.numpy(), l0)
    # a missing tensor is named, in either layout; so is a mis-shaped one
    first = FEATURE_INDEX[net][1]
    gone = dict(package)
    del gone[f"net.slice{_slice_of(net, first)}.{first}.bias"]
    with pytest.raises(KeyError, match=rf"net\.slice{_slice_of(net, first)}\.{first}\.bias"):
        load_weights(net, gone)
    gone = dict(lins)
    del gone["lin3.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        load_weights(net, (feats, gone))
    bad = dict(feats)
    bad[f"features.{first}.weight"] = bad[f"features.{first}.weight"][:, :, :2]
    with pytest.raises(ValueError, match=rf"features {first} weight"):
        load_weights(net, (bad, lins))
    bad = dict(package)
    bad["lin0.model.1.weight"] = torch.zeros(1, 63, 1, 1)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        load_weights(net, bad)
    with pytest.raises(ValueError, match="net must be"):
        load_weights("squeeze", package)
    import dsnerf_amd
    with pytest.raises(ValueError, match="state_dict is required"):
        dsnerf_amd.lpips.LPIPS(net=net)
    fn = dsnerf_amd.lpips.LPIPS(net=net, state_dict=package)          # loading needs no device; the first call or .to() packs
    assert fn.packed is None and fn.eval() is fn
    with pytest.raises(ValueError, match=r"\[N,3,H,W\]"):
        fn(torch.zeros(1, 40, 40, 3), torch.zeros(1, 40, 40, 3))


def test_argument_checks():
    import dsnerf_amd
    lib = dsnerf_amd._lib.lib()
    z, one = None, C.c_void_p(256)
    assert lib.dsn_lpips_packed_bytes(2) == 0 and lib.dsn_lpips_packed_bytes(-1) == 0
    alex, vgg = lib.dsn_lpips_packed_bytes(0), lib.dsn_lpips_packed_bytes(1)
    # split weights take the four bytes a float takes; k is padded to 16 (alex's first layer: 363 -> 368; vgg's: 27 -> 32)
    n_alex = 64 * 368 + 192 * 64 * 25 + 384 * 192 * 9 + 256 * 384 * 9 + 256 * 256 * 9
    assert 4 * n_alex < alex < 4 * n_alex + 64 * 1024 and 4 * 14_700_000 < vgg < 4 * 14_800_000
    ws = lib.dsn_lpips_workspace_bytes
    assert ws(0, 1, 64, 64) > 0 and ws(1, 1, 64, 64) > ws(0, 1, 64, 64) and ws(1, 2, 64, 64) > ws(1, 1, 64, 64)
    assert ws(2, 1, 64, 64) == 0 and ws(0, 0, 64, 64) == 0 and ws(0, 1, 0, 64) == 0 and ws(0, 1, 64, 5000) == 0
    assert ws(0, 1, 30, 31) > 0 and ws(1, 1, 15, 16) > 0               # too small is a status, not an argument error
    assert ws(1, 1, 512, 512) < 700 << 20
    calls = {
        "dsn_lpips_pack": lambda: lib.dsn_lpips_pack(0, z, z, z, z, z),
        "dsn_lpips_features": lambda: lib.dsn_lpips_features(z, 0, z, 1, 64, 64, 0, z, z, z, 0, z),
        "dsn_lpips": lambda: lib.dsn_lpips(z, 0, z, z, z, 1, 64, 64, 0, z, z, z, z, 0, z),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert name.encode() + b": null argument" in lib.dsn_last_error(), (name, lib.dsn_last_error())
    five = (C.c_void_p * 13)(*([256] * 13))
    assert lib.dsn_lpips_pack(3, five, five, five, one, z) != 0 and b"dsn_lpips_pack: net" in lib.dsn_last_error()
    assert lib.dsn_lpips_pack(0, five, five, five, C.c_void_p(8), z) != 0 and b"256-byte aligned" in lib.dsn_last_error()
    five[2] = None
    assert lib.dsn_lpips_pack(0, five, five, five, one, z) != 0 and b"null convolution tensor" in lib.dsn_last_error()
    five[2] = 256
    dl = lambda *a: lib.dsn_lpips(*a)          # noqa: E731
    assert dl(one, 0, one, one, one, 1, 64, 64, 0, one, one, one, one, 1 << 30, z) != 0 and b"exactly one ground-truth" in lib.dsn_last_error()
    assert dl(one, 0, one, one, z, 0, 64, 64, 0, one, one, one, one, 1 << 30, z) != 0 and b"dsn_lpips: bad sizes" in lib.dsn_last_error()
    assert dl(one, 5, one, one, z, 1, 64, 64, 0, one, one, one, one, 1 << 30, z) != 0 and b"dsn_lpips: bad sizes" in lib.dsn_last_error()
    assert dl(one, 0, one, one, z, 1, 64, 64, 0, one, one, one, one, ws(0, 1, 64, 64) - 1, z) != 0 and b"workspace_bytes" in lib.dsn_last_error()
    assert dl(one, 0, one, one, z, 1, 64, 64, 0, one, one, one, C.c_void_p(260), 1 << 30, z) != 0 and b"aligned" in lib.dsn_last_error()
    assert lib.dsn_lpips_features(one, 0, one, 3, 64, 64, 0, five, one, one, ws(0, 1, 64, 64), z) != 0 and b"workspace_bytes" in lib.dsn_last_error()
    # the Python wrappers check before they touch the device
    _lib = dsnerf_amd._lib
    with pytest.raises(ValueError, match="net must be"):
        _lib.lpips_check_weights("squeeze", [], [])
    w = R.make_weights("alex")
    with pytest.raises(ValueError, match="convolution 1 weight"):
        _lib.lpips_check_weights("alex", [w["conv"][0], (w["conv"][1][0][:, :, :3], w["conv"][1][1])] + w["conv"][2:], w["lin"])
    with pytest.raises(ValueError, match="lin 4"):
        _lib.lpips_check_weights("alex", w["conv"], w["lin"][:4] + [w["lin"][4][:-1]])
    with pytest.raises(ValueError, match="float32"):
        _lib.lpips("alex", None, torch.zeros(4, 4, 3, dtype=torch.float64), torch.zeros(4, 4, 3))
    assert _lib.lpips_status_text(0) == "ok" and "smallest" in _lib.lpips_status_text(1) and "32768" in _lib.lpips_status_text(2 | 4)


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_chunks_take_what_fits_under_the_cap(net, monkeypatch):
    """_lib._lpips_chunk: the frames per call under LPIPS_WORKSPACE_CAP.  The workspace has a fixed part, so k frames need less than k
    times one frame's: a cap of exactly k frames' workspace must allow k per call (then split evenly), never fewer, never more"""
    import dsnerf_amd
    _lib = dsnerf_amd._lib
    H, Wd = 37, 53
    ws = lambda k: _lib.lib().dsn_lpips_workspace_bytes(_lib._lpips_net(net), k, H, Wd)
    assert ws(2) < 2 * ws(1)
    for k, per_call in ((1, 1), (2, 2), (3, 3), (4, 3), (5, 5)):          # 5 frames: 1+1+1+1+1, 2+2+1, 3+2, 3+2 (even), 5
        monkeypatch.setattr(_lib, "LPIPS_WORKSPACE_CAP", ws(k))
        assert _lib._lpips_chunk(net, 5, H, Wd) == per_call, k
        monkeypatch.setattr(_lib, "LPIPS_WORKSPACE_CAP", ws(k) - 1)
        got = _lib._lpips_chunk(net, 5, H, Wd)
        assert got == 1 or ws(got) <= ws(k) - 1
    monkeypatch.setattr(_lib, "LPIPS_WORKSPACE_CAP", 0)                   # below one frame's: one frame per call all the same
    assert _lib._lpips_chunk(net, 5, H, Wd) == 1
