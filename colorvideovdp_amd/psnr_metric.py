"""PSNR metrics of the reference package (pycvvdp/psnr_metric.py): psnr_rgb, pu_psnr_y and pu_psnr_rgb2020.

Same constructors, `predict` / `predict_video_source` (returning `(psnr[B], None)`), names and units as the reference classes.  The
per-pixel work -- sample unpack, the source's display model, the target colour space, the squared difference and its sum -- is one HIP
pass per block of frames (cvvdp_pixel_sse, include/cvvdp_hip.h; csrc/psnr.hip); this file picks the frames' route and turns the
per-batch mean squared error into dB.

As in the reference, mse[b] is the sum over frames of the per-frame mean of (T - R)^2 over C, H, W, and
psnr[b] = 20 log10(max_I / sqrt(mse[b] / N_frames)); identical test and reference give +inf.  The sums are taken in double (the
reference sums in fp32) in an order that depends only on the frame size, so a score does not depend on how the clip is cut into
blocks or on where it lives.

Q7 (pu_psnr_y, pu_psnr_rgb2020): the reference PU21-encodes both frames and then takes the MSE of the UNENCODED frames
(psnr_metric.py:88-92).  Its "PU21-PSNR" is therefore PU21(100) over the RMSE of linear luminance (cd/m^2), or of linear BT.2020 RGB.
This build reproduces that number and does not evaluate the unused encoding.
"""
import ctypes
import math

import numpy as np
import torch

from . import _capi
from ._frames import batch_strides, yuv_block_resized
from .display_model import vvdp_display_photo_eotf, vvdp_display_photometry
from .psnr_grad import psnr_gradient
from .video_source import video_source, video_source_array
from .vq_metric import register_metric, vq_metric

# display_model.py:27-29
XYZ_to_RGB2020 = ((1.716502508360628, -0.355584689096764, -0.253375213570850),
                  (-0.666625609145029, 1.616446566522207, 0.015775479726511),
                  (0.017655211703087, -0.042810696059636, 0.942089263920533))


class PU:
    """PU21 encoding (utils.py:177-231; Mantiuk and Azimi, PCS 2021), 'banding_glare' parameters: host-side scalars only."""

    PARAMS = {"banding_glare": [0.353487901, 0.3734658629, 8.277049286e-05, 0.9062562627, 0.09150303166, 0.9099517204, 596.3148142]}

    def __init__(self, L_min=0.005, L_max=10000, type="banding_glare"):
        self.L_min, self.L_max = L_min, L_max
        self.p = self.PARAMS[type]

    def encode(self, Y):
        p = self.p
        Y = Y.clip(self.L_min, self.L_max)
        Y_p = Y ** p[3]
        return p[6] * (((p[0] + p[1] * Y_p) / (1 + p[2] * Y_p)) ** p[4] - p[5])


def psnr_scalars(dm):
    """The fp32 constants the kernels need, computed with torch on the CPU in the reference's dtypes and operation order: the PU21
    parameters, PU.encode(100) (display_model.py:215, psnr_metric.py:74), rgb2xyz[1,:] (display_model.py:246) and
    XYZ_to_RGB2020 @ rgb2xyz (display_model.py:259-260).  1-channel ('luminance') displays have no rgb2xyz: identity rows."""
    pu = PU()
    out = {"pu_p": np.asarray(pu.p, dtype=np.float32), "pu_L": np.asarray([pu.L_min, pu.L_max], dtype=np.float32),
           "pu_100": np.float32(pu.encode(torch.as_tensor(100.0)).item())}
    if hasattr(dm, "rgb2xyz_list"):
        rgb2xyz = torch.tensor(dm.rgb2xyz_list, dtype=torch.float32)
        out["y_row"] = rgb2xyz[1, :].numpy().copy()
        out["rgb2020"] = (torch.as_tensor(XYZ_to_RGB2020, dtype=torch.float32) @ rgb2xyz).numpy().copy()
    else:
        out["y_row"] = np.asarray([0, 1, 0], dtype=np.float32)
        out["rgb2020"] = np.eye(3, dtype=np.float32)
    return out


class _psnr_base(psnr_gradient, vq_metric):
    """Shared machinery; the subclasses fix the colour space the frames are compared in.  predict_with_gradient and differentiable_loss
    of the three PSNR metrics: psnr_grad.py."""

    metric_colorspace = None

    def _setup(self, display_name, display_photometry, device, config_paths):
        _capi.lib()  # fail loudly (ImportError) if the HIP library is missing
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("colorvideovdp_amd runs on an MI355X only: device must be a CUDA/HIP device; there is no CPU path")
        if self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._handles = {}
        self.block_frames = None      # frames per call for clips that are copied or unpacked first (None: sized to free memory; tests)
        self.set_display_model(display_name=display_name, display_photometry=display_photometry, config_paths=config_paths)

    def __del__(self):
        try:
            for h in getattr(self, "_handles", {}).values():
                _capi.lib().cvvdp_destroy(h)
            self._handles = {}
        except Exception:
            pass

    def set_display_model(self, display_name="standard_4k", display_photometry=None, config_paths=[]):
        """vq_metric.set_display_model (vq_metric.py:54-62)."""
        if display_photometry is None:
            self.display_photometry = vvdp_display_photometry.load(display_name, config_paths)
            self.display_name = display_name
        else:
            self.display_photometry = display_photometry
            self.display_name = getattr(display_photometry, "short_name", "unspecified")

    def predict(self, test_cont, reference_cont, dim_order="BCFHW", frames_per_second=0, frame_padding="replicate"):
        vs = video_source_array(test_cont, reference_cont, frames_per_second, dim_order=dim_order, display_photometry=self.display_photometry)
        return self.predict_video_source(vs, frame_padding=frame_padding)

    def quality_unit(self):
        return "dB"

    # ------------------------------------------------------------------ internals
    def _handle(self, dm):
        """A core handle carrying display model `dm` (cvvdp_create with the display fields of cvvdp_params filled)."""
        if not isinstance(dm, vvdp_display_photo_eotf):
            raise RuntimeError("display_photometry must be a vvdp_display_photo_eotf")
        eotf, gamma = dm.eotf_params()
        Yb, Yr = dm.get_black_level()
        key = (eotf, gamma, float(dm.Y_peak), float(Yb), float(Yr), float(dm.exposure))
        h = self._handles.get(key)
        if h is None:
            P = _capi.Params()
            P.eotf, P.gamma = eotf, gamma
            P.Y_peak, P.Y_black, P.Y_refl, P.exposure = dm.Y_peak, Yb, Yr, dm.exposure
            P.rgb2dkl[:] = dm.rgb2dkl_fp32().reshape(-1).tolist()
            h = ctypes.c_void_p()
            rc = _capi.lib().cvvdp_create(ctypes.byref(P), ctypes.byref(h))
            if rc != 0:
                raise RuntimeError(f"cvvdp_create failed ({rc})")
            self._handles[key] = h
        return h

    def _target(self, dm):
        """(CVVDP_PSNR_* of raw frames, cvvdp_psnr_args, max_I)."""
        s = psnr_scalars(dm)
        a = _capi.PsnrArgs()
        a.pu_p[:] = s["pu_p"].tolist()
        a.pu_L_min, a.pu_L_max = float(s["pu_L"][0]), float(s["pu_L"][1])
        a.pu_norm = float(s["pu_100"])
        if self.metric_colorspace == "display_encoded_100nit":
            # display_model.py:209-211: display-encoded input is compared as it is, except on PQ displays
            encoded = dm.is_input_display_encoded() and dm.EOTF != "PQ"
            a.target = _capi.PSNR_AS_IS if encoded else _capi.PSNR_PU21
            max_I = 1.0
        else:
            a.target = _capi.PSNR_Y if self.metric_colorspace == "Y" else _capi.PSNR_RGB2020
            rows = s["y_row"].tolist() + [0.0] * 6 if self.metric_colorspace == "Y" else s["rgb2020"].reshape(-1).tolist()
            a.rows[:] = rows
            max_I = float(s["pu_100"])
        return a, max_I

    def _open(self, vid_source, refuse=None):
        """The opening of every predict_video_source: (vs, H, W, N, B, is_yuv, raw, handle, cvvdp_psnr_args, max_I).  `refuse(vs, H, W)`
        raises for sources the metric does not take, before anything touches the GPU."""
        inner = getattr(vid_source, "vs", None)           # video_source_file wraps the source that does the work
        vs = inner if isinstance(inner, video_source) else vid_source
        H, W, N = vs.get_video_size()                     # (the display's resolution with full_screen_resize)
        B = vs.get_batch_size()
        if refuse is not None:
            refuse(vs, H, W)
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        is_yuv = hasattr(vs, "get_raw_yuv_block")
        raw = is_yuv or hasattr(vs, "get_raw_block") or isinstance(vs, video_source_array)
        # frames are converted with the SOURCE's display model (video_source_dm, as cvvdp_metric.py:363 does)
        dm = getattr(vs, "dm_photometry", None) if raw else None
        if dm is None:
            dm = self.display_photometry
        return (vs, H, W, N, B, is_yuv, raw, self._handle(dm)) + self._target(dm)

    def predict_video_source(self, vid_source, frame_padding="replicate"):
        vs, H, W, N, B, is_yuv, raw, h, args, max_I = self._open(vid_source)
        mse = torch.zeros(B, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for t, r, code, fmt, C, n in self._blocks(vs, H, W, N, B, is_yuv, raw, args):
                self._sse(h, t, r, code, fmt, B, C, n, H, W, args, mse)
        psnr = 20 * torch.log10(max_I / torch.sqrt(mse / N))
        return psnr.to(torch.float32), None

    def _pixel_call(self, name, h, t, r, code, fmt, B, C, n, H, W, args, outs, scratch=None):
        """One call of a cvvdp_pixel_* entry point on the current stream: scratch sized by its `_scratch_bytes`, tensor strides for
        arrays or the Y'CbCr format for planar codes, and the device pointers `outs` the entry point fills."""
        lib = _capi.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        nbytes = getattr(lib, name + "_scratch_bytes")(B, n, H, W)
        if scratch is None:
            scratch = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=self.device)
        st, sr = (None, None) if fmt is not None else self._strides(t, r, B)
        rc = getattr(lib, name)(h, t.data_ptr(), r.data_ptr(), code, st, sr, ctypes.byref(fmt) if fmt is not None else None, B, C, n, H, W,
                                ctypes.byref(args), *outs, scratch.data_ptr(), nbytes, stream)
        _capi.check(h, rc, name)

    def _sse(self, h, t, r, code, fmt, B, C, n, H, W, args, mse):
        sse = torch.empty((n, B), dtype=torch.float64, device=self.device)
        self._pixel_call("cvvdp_pixel_sse", h, t, r, code, fmt, B, C, n, H, W, args, (sse.data_ptr(), mse.data_ptr()))

    _strides = staticmethod(batch_strides)

    def _block_frames(self, bytes_per_frame, N, resident, scratch_per_frame=0):
        """Frames per call: a device-resident clip is scored in one call; frames that have to be copied or unpacked first come in blocks
        sized to a quarter of the free device memory.  A metric whose kernels need `scratch_per_frame` bytes of device scratch per frame
        of a call (MS-SSIM: the pooled planes) has every clip, a resident one too, cut so that a call's scratch stays below a quarter
        of the free memory as well."""
        if self.block_frames is not None:
            return max(1, int(self.block_frames))
        if resident and scratch_per_frame <= 0:
            return N
        free, _ = torch.cuda.mem_get_info(self.device)
        nb = N if resident else min(N, 4096, (free // 4) // max(1, bytes_per_frame))
        if scratch_per_frame > 0:
            nb = min(nb, (free // 4) // scratch_per_frame)
        return int(max(1, nb))

    def _blocks(self, vs, H, W, N, B, is_yuv, raw, args, scratch_per_frame=0):
        """(test, ref, dtype code, Y'CbCr format or None, channels, frames) per block of frames."""
        if is_yuv:
            resize = bool(getattr(vs, "needs_resize", lambda: False)())
            nb = self._block_frames((12 if resize else 4) * 3 * H * W, N, False, scratch_per_frame)
            for a in range(0, N, nb):
                b = min(N, a + nb)
                if resize:
                    t, r = self._yuv_block_resized(vs, a, b, H, W)
                    yield t, r, _capi.F32, None, 3, b - a
                else:
                    t, r, fmt = vs.get_raw_yuv_block(a, b, self.device)
                    yield t, r, (_capi.YUV8 if fmt.bit_depth == 8 else _capi.YUV16), fmt, 3, b - a
        elif isinstance(vs, video_source_array):
            t, r, code = vs.raw_arrays()
            resident = t.device == self.device and r.device == self.device
            nb = self._block_frames(2 * B * t.shape[1] * H * W * t.element_size(), N, resident, scratch_per_frame)
            for a in range(0, N, nb):
                b = min(N, a + nb)
                tb = t[:, :, a:b] if t.device == self.device else t[:, :, a:b].to(self.device)
                rb = r[:, :, a:b] if r.device == self.device else r[:, :, a:b].to(self.device)
                yield tb, rb, code, None, t.shape[1], b - a
        elif raw:
            resident = bool(getattr(vs, "device_resident", False))
            nb = self._block_frames(2 * B * 3 * H * W * 4, N, resident, scratch_per_frame)
            for a in range(0, N, nb):
                b = min(N, a + nb)
                t, r, code = vs.get_raw_block(a, b, self.device)
                yield t, r, code, None, t.shape[1], b - a
        else:
            # generic source: frames arrive one by one, already in the metric's colour space (psnr_metric.py:36-43, :82-86)
            args.target = _capi.PSNR_AS_IS
            nb = self._block_frames(2 * B * 3 * H * W * 4, N, False, scratch_per_frame)
            for a in range(0, N, nb):
                b = min(N, a + nb)
                ts, rs = [], []
                for f in range(a, b):
                    ts.append(vs.get_test_frame(f, device=self.device, colorspace=self.metric_colorspace).to(self.device, torch.float32))
                    rs.append(vs.get_reference_frame(f, device=self.device, colorspace=self.metric_colorspace).to(self.device, torch.float32))
                t, r = torch.cat(ts, dim=2).contiguous(), torch.cat(rs, dim=2).contiguous()
                if t.dim() != 5 or t.shape[1] not in (1, 3):
                    raise RuntimeError(f"frames of shape {tuple(t.shape)}: expected [B, 1 or 3, 1, H, W]")
                yield t, r, _capi.F32, None, t.shape[1], b - a

    def _yuv_block_resized(self, vs, a, b, height, width):
        """Frames [a,b) of a .yuv pair with full_screen_resize as fp32 R'G'B' at the display's resolution (_frames.yuv_block_resized)."""
        return yuv_block_resized(self._handle(vs.dm_photometry), self.device, vs, a, b, height, width)


class psnr_rgb(_psnr_base):
    """Plain PSNR-RGB (psnr_metric.py:15-55): display-encoded values, PU21-encoded (and scaled so that 100 cd/m^2 maps to 1) when the
    display is linear or PQ (display_model.py:206-226); max_I = 1."""

    metric_colorspace = "display_encoded_100nit"
    _psnr_loss = True

    def __init__(self, display_name="standard_4k", display_photometry=None, device=None, config_paths=[]):
        self._setup(display_name, display_photometry, device, config_paths)

    def short_name(self):
        return "PSNR-RGB"


class pu_psnr_y(_psnr_base):
    """PU21-PSNR-Y (psnr_metric.py:60-112): luminance Y in cd/m^2, max_I = PU21(100).  Quirk Q7 (module docstring): the MSE is that
    of the unencoded luminance, as in the reference."""

    metric_colorspace = "Y"
    _psnr_loss = True

    def __init__(self, display_name="standard_4k", display_photometry=None, color_space="sRGB", device=None, config_paths=[]):
        self.color_space = color_space  # input content colour space (stored, as in the reference)
        self._setup(display_name, display_photometry, device, config_paths)
        self.pu = PU()
        self.max_I = self.pu.encode(torch.as_tensor(100))

    def short_name(self):
        return "PU21-PSNR-Y"


class pu_psnr_rgb2020(pu_psnr_y):
    """PU21-PSNR-RGB2020 (psnr_metric.py:115-123): linear BT.2020 RGB in cd/m^2, MSE over the three channels; quirk Q7 as pu_psnr_y.
    Like the reference's constructor, this one has no config_paths."""

    metric_colorspace = "RGB2020"

    def __init__(self, display_name="standard_4k", display_photometry=None, color_space="sRGB", device=None):
        super().__init__(display_name=display_name, display_photometry=display_photometry, color_space=color_space, device=device)

    def short_name(self):
        return "PU21-PSNR-RGB2020"


register_metric(psnr_rgb)
register_metric(pu_psnr_y)
register_metric(pu_psnr_rgb2020)
