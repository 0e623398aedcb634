"""panic3d-anime-reconstruction_amd — MI355X-native (gfx950) triplane volumetric-rendering hot path of PAniC-3D.

Import name: `panic3d_amd` (see the shim panic3d_amd.py at the repository root; the directory name carries a hyphen).
Layout: csrc/ (HIP kernels + C ABI), _lib.py (ctypes binding), ops.py (tensor-level operators),
renderer.py (mirror of the reference's ImportanceRenderer call surface), optim.py (the optimiser step and the G_ema update), lpips.py (the AlexNet perceptual distance),
encoder.py (the conditioning encoder: ResNet-50 features and their PCA), metrics.py (the geometry metrics: point-to-mesh distance, Chamfer, F1),
rmline.py (the illustration-to-render module: line mask and generator), clip.py (CLIP's ViT-B/32 image tower and the image similarity),
augment.py (ADA's augmentation pipe: host-side draws, the two image operators, the controller).
"""
from . import _build, _lib, memo, ops, cameras, sharding, stylegan2, generator, volume, outputs, discriminator, loss, optim, lpips, encoder, metrics, rmline, clip, rmline_train  # noqa: F401
from .clip import CLIPVisual, CLIPSimilarity  # noqa: F401
from .metrics import psnr, image_metrics  # noqa: F401
from .rmline import RMLineGenerator, RMLineWrapper, face_hull  # noqa: F401
from .rmline_train import RMLineModel  # noqa: F401
from .renderer import ImportanceRenderer, decoder_params  # noqa: F401
from .lpips import LPIPS, LPIPSLoss  # noqa: F401
from .encoder import ResNetEncoder, ResnetFeatureExtractorPCA  # noqa: F401
from .metrics import point_mesh_squared_distance, sample_points_on_mesh, filter_mesh, point_mesh_f1, geometry_metrics  # noqa: F401
from .discriminator import DualDiscriminator  # noqa: F401
from .loss import StyleGAN2LossOrthoCondA  # noqa: F401
from . import augment  # noqa: F401
from .augment import AugmentPipe, AdaStats, ada_update  # noqa: F401

build = _build.build
