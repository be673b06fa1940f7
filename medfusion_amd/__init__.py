"""medfusion_amd -- MI355X-native latent-diffusion sampling path for Medfusion-style models.

Drop-in for the reference's sampling API (`DiffusionPipeline.sample/denoise/forward`, `UNet.forward`,
`VAE.encode/decode` and the VQVAE / VQGAN / VAEGAN embedders, `GaussianNoiseScheduler`) running on hand-written HIP kernels for gfx950 through a
C-ABI (include/medfusion_hip.h).  No CPU fallback: the library must load and tensors must be on the GPU.
"""
from .lib import load as load_library  # noqa: F401
from . import fidelity, inception, ingest, lpips, metrics  # noqa: F401
from .fidelity import (EmbedderFeatures, FidelityMeter, density_coverage, frechet_distance, kernel_matrix, kid, knn_radii, manifold_hits,  # noqa: F401
                       memorization_report, mmd2, nearest_neighbours, pairwise_sqdist, plan_kid, precision_recall)
from .inception import InceptionFeatures, InceptionNet, inception_score  # noqa: F401
from .lpips import LPIPSNet  # noqa: F401
from .metrics import ReconstructionMeter, ms_ssim, mse, pairwise_ms_ssim, ssim  # noqa: F401
from .metrics3d import (VolumeReconstructionMeter, betas_for, min_side3d, ms_ssim3d, ms_ssim3d_and_mse, mse3d, pair_range3d,  # noqa: F401
                        pairwise_ms_ssim3d, pyramid3d, ssim3d)
from .noise import HostNoise, NoiseSource, PhiloxDeviceNoise, torch_cpu_noise  # noqa: F401
from .pipeline import DiffusionPipeline, EMAModel  # noqa: F401
from .scheduler import BasicNoiseScheduler, GaussianNoiseScheduler  # noqa: F401
from .unet import LabelEmbedder, LearnedSinusoidalPosEmb, SinusoidalPosEmb, TimeEmbbeding, UNet  # noqa: F401
from .vae import VAE, DiagonalGaussianDistribution  # noqa: F401
from .validation import ValidationMeter  # noqa: F401
from .vq import VAEGAN, VQGAN, VQVAE, VectorQuantizer  # noqa: F401

__version__ = "0.1.0"
