"""MI355X-native forward Gaussian-splat rasteriser behind the Python surface of
dcaustin33/intro_to_gaussian_splatting (``splat.GaussianScene``): PyTorch-ROCm tensors hold the
Gaussians, hand-written HIP kernels (libgsx.so, C ABI in include/gsx.h) do the work."""
from .gaussians import Gaussians
from .gaussian_scene import Contribution, GaussianScene, NativeExtension, render_preprocessed
from .image import GaussianImage
from .loss import depth_loss, photometric_loss
from .optim import GaussianAdam, expon_lr
from .density import DensityControl
from .mcmc import MCMCControl
from .knn import nearest3
from .fit import Trainer, events_at
from .pose import CameraRefiner
from .exposure import ExposureRefiner
from .schema import PreprocessedScene
from .capture import load_capture, read_photo, rectified_camera, rectify

__all__ = ["load_capture", "read_photo", "rectified_camera", "rectify","Gaussians", "GaussianScene", "GaussianImage", "PreprocessedScene", "render_preprocessed",
           "NativeExtension", "photometric_loss", "depth_loss", "GaussianAdam", "expon_lr", "DensityControl", "MCMCControl",
           "nearest3",
           "Trainer", "events_at", "CameraRefiner", "ExposureRefiner", "Contribution"]
