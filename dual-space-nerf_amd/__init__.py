"""dsnerf_amd - MI355X (gfx950) implementation of the Dual-Space-NeRF volume-rendering hot path.

Python surface mirrors the reference (zyhbili/Dual-Space-NeRF): can_render.Renderer and
model.spacenet.{DualSpaceNeRF, SpaceNet, LightingMLP}; the math runs in libdsnerf_hip.so
(include/dsnerf.h).  Import name: `dsnerf_amd` (the directory is `dual-space-nerf_amd/`, loaded by
the repo-root shim dsnerf_amd.py because a hyphenated directory is not an importable name).
"""
from . import synth  # noqa: F401
from . import _lib  # noqa: F401
from . import loss  # noqa: F401  (make_loss, MSELoss, SmoothL1Loss: utils/loss.py on the device)
from . import optim  # noqa: F401  (make_optimizer, Adam: solver/build.py on the device)
from . import body  # noqa: F401  (BodyModel: SMPL parameters -> posed vertices, joint transforms and bounds on the device)
from .body import BodyModel  # noqa: F401
from . import imageprep  # noqa: F401  (undistort, dilate, erode, resizes, prepare_zju / prepare_h36m: the datasets' OpenCV work on the device)
from . import lpips  # noqa: F401  (LPIPS: test.py's lpips_alex / lpips_vgg distances on the device)
from . import jpeg  # noqa: F401  (encode, imwrite, write_avi: the scripts' cv2.imwrite into .jpg on the device, img2vid's place)
from . import png  # noqa: F401  (decode, imread: the datasets' label masks, inflated and unfiltered on the device)
from .can_render import Renderer  # noqa: F401
from .model.spacenet import DualSpaceNeRF, LightingMLP, SpaceNet  # noqa: F401
from .parallel import RayParallel  # noqa: F401

__all__ = ["Renderer", "DualSpaceNeRF", "SpaceNet", "LightingMLP", "RayParallel", "synth", "loss", "optim", "body", "BodyModel", "imageprep", "lpips", "jpeg", "png"]
