"""For users who have the `lpips` package (and the torchvision weights it loads): dsnerf_amd.lpips.LPIPS with the package's own
state dict against the package itself, as test.py:18-23, 77-91 calls it.  Skipped wherever the package does not import - it was not
available where the kernels were written, so this parity is otherwise unverified (include/dsnerf.h "LPIPS")."""
import numpy as np
import pytest
import torch

import lpips_restate as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_against_the_package(net):
    lpips = pytest.importorskip("lpips")
    import dsnerf_amd
    try:
        theirs = lpips.LPIPS(net=net).eval()          # (loads torchvision's weights: needs them cached or a network)
    except Exception as e:                            # noqa: BLE001
        pytest.skip(f"lpips.LPIPS(net={net!r}) could not load its weights: {e}")
    ours = dsnerf_amd.lpips.LPIPS(net=net, state_dict=theirs.state_dict()).to("cuda")
    frames = [R.make_pair(96, 128, 40 + k) for k in range(2)]
    to_nchw = lambda a: (2.0 * torch.from_numpy(np.stack(a)).float() - 1.0).flip(-1).permute(0, 3, 1, 2).contiguous()      # noqa: E731
    pred, gt = to_nchw([f[0] for f in frames]), to_nchw([f[1] for f in frames])
    with torch.no_grad():
        want = theirs.double()(pred.double(), gt.double()).reshape(-1).numpy()
    got = ours(pred.cuda(), gt.cuda())
    assert got.shape == (2, 1, 1, 1) and ours.last_status.cpu().tolist() == [0, 0]
    assert np.abs(ours.last.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max(), (ours.last.cpu().numpy(), want)
