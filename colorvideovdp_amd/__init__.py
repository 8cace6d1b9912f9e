"""colorvideovdp_amd: MI355X-native compute core for the ColorVideoVDP metric behind the reference's
Python API (`cvvdp.predict`, `cvvdp.predict_video_source`, heat maps, distograms), and the reference's
PSNR metrics (`psnr_rgb`, `pu_psnr_y`, `pu_psnr_rgb2020`), its SSIM metric (`ssim_metric`), an MS-SSIM metric (`ms_ssim_metric`) and its display-model previews
(`dm_preview`, `dm_preview_sbs`, `dm_preview_hdr`, `dm_preview_hdr_sbs`) and debugging pictures (`DumpChannels`), and its
ColorVideoVDP-ML-Saliency and ColorVideoVDP-ML-Transformer metrics (`cvvdp_ml_saliency`, `cvvdp_ml_transformer`: the user supplies the
model's parameter file and checkpoint; the transformer from Python only, not yet on the command line)."""
from .cvvdp_metric import cvvdp
from .psnr_metric import psnr_rgb, pu_psnr_rgb2020, pu_psnr_y
from .ssim_metric import ssim_metric
from .ms_ssim_metric import ms_ssim_metric
from .dm_preview_metric import dm_preview, dm_preview_hdr, dm_preview_hdr_sbs, dm_preview_sbs
from .cvvdp_ml_metric import cvvdp_ml_saliency, cvvdp_ml_transformer
from .dump_channels import DumpChannels
from .display_model import vvdp_display_geometry, vvdp_display_photo_eotf, vvdp_display_photometry
from .video_source import reshuffle_dims, video_source, video_source_array
from .video_source_file import load_image_as_array, video_source_file, video_source_image_frames
from .video_source_yuv import video_source_yuv_file
from .video_source_temp_resample import video_source_temp_resample_file
from .vq_metric import register_metric, vq_exception, vq_metric, vq_metric_dict

__version__ = "0.3.0"
COMPUTE_DTYPE = "f32"      # the arithmetic of every kernel (integer / fp16 / Y'CbCr samples are unpacked to fp32 by the first kernel of the path)
