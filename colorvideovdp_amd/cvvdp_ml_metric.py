"""The ML heads of ColorVideoVDP (pycvvdp/cvvdp_ml_metric.py) for MI355X, on the base model's pooled per-band features
(`cvvdp.extract_features`):

  cvvdp_ml_saliency      (:463-550) two small MLPs at every feature cell, a saliency ("attention") net on the statistics of test and
                         reference and a difference net on the statistics of D.  One HIP pass per band (cvvdp_ml_saliency_head,
                         include/cvvdp_hip.h; csrc/ml_head.hip).
  cvvdp_ml_transformer   (:553-678) a 4-layer, 256-wide, 8-head pre-norm transformer encoder over all cells of a frame, read out at a
                         cls token.  HIP kernels on the fp32 matrix instructions (cvvdp_ml_transformer_head; csrc/ml_transformer.hip).
                         From Python only; not yet on the command line.

Same constructor arguments, methods, names and errors as the reference classes.  The features come from the band kernels' feature
route, unchanged.

Where the two files of the model come from: the reference package ships `vvdp_data/cvvdp_ml_saliency/cvvdp_parameters.json` and fetches
the trained networks, `cvvdp_ml_saliency/cvvdp.ckpt`, when its class is first constructed (and likewise under `cvvdp_ml_transformer`).
This package ships neither and fetches nothing: the directory that holds both is passed as `config_paths=[dir]` (`-c dir` on the
command line).  A sub-directory of a configuration directory with the model's name is looked into first, so the parent of the
reference's layout works as well.

Training of cvvdp_ml_saliency: the gradient of Q_JOD in the packed weights of both MLPs and in `baseband_weight` comes from one more HIP
pass per band (cvvdp_ml_saliency_head_grad; csrc/ml_head_grad.hip): do_pooling_and_jods_with_weight_gradient,
differentiable_jods (autograd), predict_with_weight_gradient; `calibration fit -m cvvdp-ml-saliency` runs Adam on them and writes a
cvvdp.ckpt.  No dropout: the reference's MLPs carry Dropout(0.2) in training mode, the fit here is deterministic.

cvvdp_ml_saliency as an image loss: predict_with_gradient / differentiable_loss give d Q_JOD / d test of an image.  The
gradient of Q_JOD in the features, what the reference's autograd leaves in features[band].grad, is a third HIP pass per band
(cvvdp_ml_saliency_head_input_grad; csrc/ml_head_input_grad.hip: do_pooling_and_jods_with_feature_gradient); the adjoint of the feature
pooling takes it into the band chain of cvvdp's image gradient (cvvdp_ml_image_gradient; csrc/ml_image_grad.hip).  Clips and the
gradient in the reference are refused; so is everything for the transformer head.

Not available: heat maps, distograms, frame sharding, `RegressionTransformer.get_heatmap`, training of the transformer head, the
pixel gradient of clips and of the transformer metric.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from . import _capi
from . import host_setup as hs
from .config import config_files, json2dict
from ._pixel_grad import GradOut, PixelLoss
from .cvvdp_metric import cvvdp
from .video_source import video_source, video_source_array
from .vq_metric import register_metric, vq_exception

f32 = np.float32

# Linear layers of the two torchvision MLPs (cvvdp_ml_metric.py:407-412, :471-476): sizes from the input to the output
ARCHITECTURE = {"att_net": (16, 48, 48, 48, 48, 1), "feature_net": (8, 24, 24, 24, 1)}
_WHERE = ("Pass the directory that holds the reference's cvvdp_ml_saliency/cvvdp_parameters.json and its cvvdp.ckpt with -c "
          "(config_paths): this package ships neither file.")


def nets_from_state_dict(state_dict):
    """{'att_net': [(weight, bias), ...], 'feature_net': [...]} as float32 CPU tensors from the entries `<net>.<i>.weight` /
    `<net>.<i>.bias` of a state dict.  The Linear layers are the entries sorted by i (torchvision's MLP puts them at 0, 3, 6, ...
    between ReLU and Dropout; the indices themselves are not relied on); their shapes must chain to exactly ARCHITECTURE.  Anything
    else raises a RuntimeError that names the offending key."""
    nets = {}
    for net, dims in ARCHITECTURE.items():
        found = {}
        for key in state_dict:
            if not key.startswith(net + "."):
                continue
            parts = key[len(net) + 1:].split(".")
            if len(parts) != 2 or not parts[0].isdigit() or parts[1] not in ("weight", "bias"):
                raise RuntimeError(f"checkpoint entry '{key}' is not the weight or bias of a Linear layer of {net}")
            found.setdefault(int(parts[0]), {})[parts[1]] = key
        order = sorted(found)
        layers = []
        for k, i in enumerate(order):
            if k >= len(dims) - 1:
                raise RuntimeError(f"checkpoint entry '{next(iter(found[i].values()))}': {net} has {len(dims) - 1} Linear layers, this is one more")
            for kind, shape in (("weight", (dims[k + 1], dims[k])), ("bias", (dims[k + 1],))):
                key = f"{net}.{i}.{kind}"
                if kind not in found[i]:
                    raise RuntimeError(f"checkpoint entry '{key}' is missing")
                got = tuple(torch.as_tensor(state_dict[key]).shape)
                if got != shape:
                    raise RuntimeError(f"checkpoint entry '{key}' has shape {got}, layer {k} of {net} needs {shape}")
            layers.append(tuple(torch.as_tensor(state_dict[f"{net}.{i}.{kind}"]).detach().to("cpu", torch.float32).contiguous() for kind in ("weight", "bias")))
        if len(layers) != len(dims) - 1:
            after = f"after '{net}.{order[-1]}.weight'" if order else f"no '{net}.<i>.weight' at all"
            raise RuntimeError(f"{net} has {len(dims) - 1} Linear layers, the checkpoint holds {len(layers)} ({after})")
        nets[net] = layers
    return nets


def random_nets():
    """Both networks with torch's default Linear initialisation (random_init=True: tests and training, cvvdp_ml_metric.py:112)."""
    nets = {}
    for net, dims in ARCHITECTURE.items():
        lin = [torch.nn.Linear(dims[k], dims[k + 1]) for k in range(len(dims) - 1)]
        nets[net] = [(l.weight.detach().clone(), l.bias.detach().clone()) for l in lin]
    return nets


def pack_weights(nets):
    """The head's weights in the order cvvdp_ml_saliency_head documents: per layer weight [out][in] row-major, then bias; att_net from
    float 0, feature_net from float ML_FEATURE_NET_OFFSET, ML_WEIGHTS floats in all (the gaps are zero)."""
    out = np.zeros(_capi.ML_WEIGHTS, dtype=f32)
    for net, start in (("att_net", 0), ("feature_net", _capi.ML_FEATURE_NET_OFFSET)):
        flat = np.concatenate([np.concatenate([w.numpy().reshape(-1), b.numpy().reshape(-1)]) for w, b in nets[net]]).astype(f32)
        out[start:start + flat.size] = flat
    return out


def _layer_slices():
    """[(net, layer, weight slice, (out, in), bias slice)] of the packed buffer."""
    out = []
    for net, start in (("att_net", 0), ("feature_net", _capi.ML_FEATURE_NET_OFFSET)):
        dims, pos = ARCHITECTURE[net], start
        for k in range(len(dims) - 1):
            nw, nb = dims[k] * dims[k + 1], dims[k + 1]
            out.append((net, k, slice(pos, pos + nw), (dims[k + 1], dims[k]), slice(pos + nw, pos + nw + nb)))
            pos += nw + nb
    return out


def _nets_as_state_dict(nets):
    """{'att_net': [(weight, bias), ...], ...} under torchvision's layer indices (0, 3, 6, ...): `<net>.<3 k>.weight` / `.bias`."""
    return {f"{net}.{3 * k}.{kind}": t for net, layers in nets.items() for k, wb in enumerate(layers) for kind, t in zip(("weight", "bias"), wb)}


def unpack_weights(packed, state_dict=False):
    """The inverse of pack_weights: {'att_net': [(weight, bias), ...], 'feature_net': [...]} as float32 CPU tensors from a packed buffer
    (array or tensor, ML_WEIGHTS values; the padding is dropped), or with state_dict=True the same as a state dict with torchvision's
    layer indices (0, 3, 6, ...), what a checkpoint's `state_dict` holds.  load_state_dict_nets() takes either."""
    a = packed.detach().cpu().numpy() if torch.is_tensor(packed) else np.asarray(packed)
    a = np.ascontiguousarray(a, dtype=f32).reshape(-1)
    if a.size != _capi.ML_WEIGHTS:
        raise ValueError(f"unpack_weights: {a.size} values, the packed head has {_capi.ML_WEIGHTS}")
    nets = {net: [] for net in ARCHITECTURE}
    for net, _, sw, shape, sb in _layer_slices():
        nets[net].append((torch.from_numpy(a[sw].reshape(shape).copy()), torch.from_numpy(a[sb].copy())))
    return _nets_as_state_dict(nets) if state_dict else nets


class _HeadJods(torch.autograd.Function):
    """Q_JOD [B] of cvvdp_ml_saliency attached to autograd in the packed weights and (optionally) a scalar baseband_weight."""

    @staticmethod
    def forward(ctx, metric, features, weights, baseband_weight):
        bw = None if baseband_weight is None else float(baseband_weight.detach())
        ctx.metric, ctx.features, ctx.bw = metric, features, bw
        ctx.save_for_backward(weights, *(() if baseband_weight is None else (baseband_weight,)))
        return metric._head_forward(features, metric._weights_arg(weights), bw)

    @staticmethod
    def backward(ctx, grad_q):
        saved = ctx.saved_tensors
        g, g_bw = ctx.metric._head_weight_gradient(ctx.features, grad_q, ctx.metric._weights_arg(saved[0]), ctx.bw)
        g = g.to(saved[0].device, saved[0].dtype).reshape(saved[0].shape) if ctx.needs_input_grad[2] else None
        if len(saved) > 1 and ctx.needs_input_grad[3]:
            g_bw = g_bw.to(saved[1].device, saved[1].dtype).reshape(saved[1].shape)
        else:
            g_bw = None
        return None, None, g, g_bw


class _cvvdp_ml(cvvdp):
    """What the ML metrics share: the constructor's refusals, the model directory, the display-model swap of predict_video_source.  A
    metric names its model (`_MODEL`, `_TITLE`), makes and validates its networks (`_random_nets`, `_nets_from_state_dict`, `_set_nets`) and
    scores the features (`do_pooling_and_jods`)."""
    _MODEL = _TITLE = _WHERE = None

    def __init__(self, display_name="standard_4k", display_photometry=None, display_geometry=None, config_paths=[], heatmap=None, quiet=False,
                 device=None, temp_padding="replicate", use_checkpoints=False, dump_channels=None, gpu_mem=None, block_frames=None,
                 random_init=False, disabled_features=None):
        if heatmap is not None and heatmap != "none":
            raise vq_exception("Currently cvvdp-ml metrics do not produce heatmaps")
        if dump_channels is not None:
            raise vq_exception("dump_channels is not available with extract_features (the feature kernels keep no per-pixel planes)")
        self.random_init = random_init
        if disabled_features is not None:
            disabled_features = [int(s) for s in disabled_features]
            if any(s < 0 or s > 5 for s in disabled_features):
                raise ValueError(f"disabled_features {disabled_features}: a cell has the statistics 0..5")
        self.disabled_features = disabled_features
        self._nets = None
        self._weights_dev = None
        super().__init__(display_name=display_name, display_photometry=display_photometry, display_geometry=display_geometry,
                         config_paths=config_paths, heatmap=None, quiet=quiet, device=device, temp_padding=temp_padding,
                         use_checkpoints=use_checkpoints, dump_channels=None, gpu_mem=gpu_mem, block_frames=block_frames)

    # ------------------------------------------------------------------ configuration
    def load_config(self, config_paths):
        """cvvdp_ml_base.load_config (cvvdp_ml_metric.py:156-172) with the model's own parameter file.  Its `baseband_weight` is a scalar
        that scales the head's output on the last band; the core wants the base model's list of four (read by the pooling of Q_per_ch
        and by heat maps, neither of which this metric runs: the features carry no baseband weight) and gets the scalar four times."""
        if not isinstance(config_paths, list):
            raise RuntimeError("config_paths must be a list")
        model, title, where = self._MODEL, self._TITLE, self._WHERE
        own = [os.path.join(cp, model) for cp in config_paths if os.path.isdir(os.path.join(cp, model))]
        try:
            pfile = config_files.find("cvvdp_parameters.json", own + config_paths)
        except RuntimeError as e:
            raise vq_exception(f"{e}. {where}") from None
        if pfile.startswith("builtin:"):
            raise vq_exception(f"The parameter file of {title} (cvvdp_parameters.json with internal_model_name '{model}') was not "
                               f"found in the configuration paths. {where}")
        p = dict(json2dict(pfile))
        bw = p.get("baseband_weight")
        if p.get("internal_model_name") != model or isinstance(bw, (list, tuple)):
            raise vq_exception(f"'{pfile}' is not the parameter file of {title} (internal_model_name "
                               f"'{p.get('internal_model_name')}': the base model's file?). {where}")
        if isinstance(bw, (str, bool)) or bw is None or not np.isfinite(float(bw)):
            raise RuntimeError(f"parameter 'baseband_weight' of {title} must be a finite number")
        if self.random_init:
            nets = self._random_nets()
        else:
            try:
                ckpt = config_files.find("cvvdp.ckpt", own + config_paths)
            except RuntimeError:
                raise vq_exception(f"The checkpoint of {title} (cvvdp.ckpt) was not found in the configuration paths. {where}") from None
            logging.info(f"Loading cvvdp checkpoint file from {ckpt}")
            nets = self._nets_from_state_dict(torch.load(ckpt, map_location="cpu")["state_dict"])
        self.parameters_file = pfile
        self._config_paths = list(config_paths)
        p["baseband_weight"] = [float(bw)] * 4
        self._set_parameters(p)
        self._ml_baseband_weight = f32(bw)
        self._set_nets(nets)

    def set_frame_sharding(self, group="world"):
        if group is not None:
            raise vq_exception("cvvdp-ml metrics cannot be sharded over frames: the head pools over all frames of the clip")
        self._shard = None

    # ------------------------------------------------------------------ public API
    def _score_source(self, vid_source, head):
        """(the source itself, its size, head(features)) of what predict_video_source scores: the refusals, the display-model swap of a raw
        source, extract_features, and `head` on the features before the swap is undone."""
        inner = getattr(vid_source, "vs", None)
        if isinstance(inner, video_source):
            vid_source = inner
        if hasattr(vid_source, "set_temporal_filters"):
            raise vq_exception("--temp-resample sources are scored by the cvvdp metric only")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        size = vid_source.get_video_size()
        # a raw source that carries its own display photometry is measured with it, as in cvvdp.predict_video_source
        src_dm = getattr(vid_source, "dm_photometry", None)
        swap = src_dm is not None and src_dm is not self.display_photometry and self._is_raw_source(vid_source)
        if swap:
            prev = self.display_photometry
            self.display_photometry = src_dm
            self._make_handle()
        try:
            features, _ = self.extract_features(vid_source)
            out = head(features)
        finally:
            if swap:
                self.display_photometry = prev
                self._make_handle()
        return vid_source, size, out

    def _source_features(self, vid_source):
        """(the source itself, its size, the features) of what predict_video_source scores."""
        return self._score_source(vid_source, lambda features: features)

    def _source_stats(self, vid_source, size):
        height, width, N_frames = size
        pyr_height, freqs = hs.band_frequencies(width, height, self.pix_per_deg)
        rho_band = freqs.copy()
        rho_band[pyr_height] = 0.1
        return {"rho_band": rho_band, "frames_per_second": vid_source.get_frames_per_second(), "width": width, "height": height,
                "N_frames": N_frames}

    def predict_video_source(self, vid_source):
        """cvvdp_ml_base.predict_video_source (cvvdp_ml_metric.py:174-201)."""
        vid_source, size, Q_jod = self._score_source(vid_source, self.do_pooling_and_jods)
        return (Q_jod.squeeze(), self._source_stats(vid_source, size))

    def _check_features(self, features, baseband_weight=None):
        """B, C and an iterator over the bands (the features as a contiguous fp32 device tensor, the head's scale: 1 / bands, times the model's
        baseband_weight on the last band, times image_int for an image) of a list of [B, F, H', W', C, 6] tensors.  baseband_weight: a
        value in place of the model's."""
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        bw = float(self._ml_baseband_weight if baseband_weight is None else f32(baseband_weight))
        no_bands = len(features)
        if no_bands < 1:
            raise ValueError("do_pooling_and_jods: no bands")
        B, C = int(features[0].shape[0]), int(features[0].shape[4])

        def bands():                                    # one band on the device at a time
            for bb, f in enumerate(features):
                f = torch.as_tensor(f).to(self.device, torch.float32).contiguous()
                if f.dim() != 6 or f.shape[5] != 6 or f.shape[0] != B or f.shape[4] != C:
                    raise ValueError(f"features[{bb}] has shape {tuple(f.shape)}, expected [{B}, F, H', W', {C}, 6]")
                scale = 1.0 / no_bands
                if bb == no_bands - 1:
                    scale *= bw
                if C == 3:
                    scale *= float(f32(self.parameters["image_int"]))
                yield f, scale
        return B, C, bands()

    def predict_with_gradient(self, test, reference, dim_order="BCFHW", frames_per_second=0, block_frames=None, wrt="test"):
        """Refused: cvvdp's pixel gradient differentiates the pooling of Q_per_ch, which these metrics replace by a trained head."""
        raise vq_exception(f"{self._TITLE}: no pixel gradient for this head yet (predict_with_gradient and differentiable_loss are those of "
                           "the cvvdp metric and of cvvdp_ml_saliency)")

    def differentiable_loss(self, test, reference, dim_order="BCFHW", frames_per_second=0, block_frames=None, wrt="test"):
        """Refused, as predict_with_gradient."""
        return self.predict_with_gradient(test, reference, dim_order, frames_per_second, block_frames, wrt)

    def short_name(self):
        return self.__class__.__name__.replace("_", "-")

    def export_distogram(self, stats, fname, jod_max=None, base_size=6):
        raise vq_exception("Currently cvvdp-ml metrics do not export distograms")


class cvvdp_ml_saliency(_cvvdp_ml):
    _MODEL, _TITLE, _WHERE = "cvvdp_ml_saliency", "cvvdp-ml-saliency", _WHERE
    _random_nets = staticmethod(random_nets)
    _nets_from_state_dict = staticmethod(nets_from_state_dict)

    def _set_nets(self, nets):
        self._nets = nets
        self._packed = pack_weights(nets)
        self._weights_dev = None

    def load_state_dict_nets(self, state_dict):
        """Replace both networks from a state dict with `att_net.<i>.weight` / `.bias` and `feature_net.<i>.weight` / `.bias` entries
        (what a checkpoint's `state_dict` holds), or from the nets unpack_weights() returns; validated like a checkpoint, and nothing
        changes if it does not validate."""
        if set(state_dict) == set(ARCHITECTURE):
            state_dict = _nets_as_state_dict(state_dict)
        self._set_nets(nets_from_state_dict(state_dict))

    def state_dict_nets(self):
        """The networks as a state dict with torchvision's layer indices (0, 3, 6, ...)."""
        return {key: t.clone() for key, t in _nets_as_state_dict(self._nets).items()}

    def packed_weights(self):
        """float32 [ML_WEIGHTS]: the buffer the kernel reads (pack_weights)."""
        return self._packed.copy()

    def do_pooling_and_jods(self, features):
        """cvvdp_ml_saliency.do_pooling_and_jods (cvvdp_ml_metric.py:496-541): features[band] is [B, F, H', W', C, 6] (any list of such
        tensors; C = 3 marks an image) -> Q_JOD[B] on the device.  One cvvdp_ml_saliency_head call per band; unlike the reference's,
        this one leaves the caller's tensors as they are."""
        return self._head_forward(features, self._weights_arg(None))

    def _weights_arg(self, weights):
        """The packed weights the kernels read: the metric's own (None), or a float32 tensor of ML_WEIGHTS values, moved to the device
        and a 16-byte aligned contiguous buffer if it is not there already."""
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        if weights is None:
            if self._weights_dev is None:
                self._weights_dev = torch.from_numpy(self._packed).to(self.device)
            return self._weights_dev
        if not torch.is_tensor(weights) or weights.dtype != torch.float32 or weights.numel() != _capi.ML_WEIGHTS:
            raise ValueError(f"weights must be a float32 tensor of {_capi.ML_WEIGHTS} values (weight_tensor())")
        w = weights.detach().to(self.device).contiguous().reshape(-1)
        return w.clone() if w.data_ptr() % 16 else w

    def _head_bands(self, features, baseband_weight=None):
        """What the head's three passes share: B, C, the mask of disabled_features, the library, the current stream and an iterator over
        the bands of _check_features as (features, F, H', W', scale), the features cloned if they are not aligned to what the kernels
        read at a time (16 bytes for four channels, 8 for three: a view into a larger buffer may not be)."""
        B, C, bands = self._check_features(features, baseband_weight)

        def aligned():
            for f, scale in bands:
                if f.data_ptr() % (16 if C == 4 else 8):
                    f = f.clone()
                yield (f,) + tuple(int(n) for n in f.shape[1:4]) + (scale,)

        mask = sum(1 << s for s in set(self.disabled_features or ()))
        return B, C, mask, _capi.lib(), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), aligned()

    def _head_forward(self, features, wdev, baseband_weight=None):
        B, C, mask, lib, stream, bands = self._head_bands(features, baseband_weight)
        with torch.cuda.device(self.device):
            Q = torch.full((B,), 10.0, dtype=torch.float32, device=self.device)
            for f, F, Hc, Wc, scale in bands:
                nbytes = lib.cvvdp_ml_saliency_head_scratch_bytes(B, F, Hc, Wc)
                scratch = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=self.device)
                rc = lib.cvvdp_ml_saliency_head(self._handle, f.data_ptr(), B, F, Hc, Wc, C, wdev.data_ptr(), scale, mask,
                                                Q.data_ptr(), scratch.data_ptr(), nbytes, stream)
                _capi.check(self._handle, rc, "cvvdp_ml_saliency_head")
        return Q

    # ------------------------------------------------------------------ training
    def weight_tensor(self):
        """The packed weights (pack_weights) as a new float32 tensor on the device: what an optimiser owns.  The padding floats have a
        zero gradient, so they stay zero under Adam.  load_state_dict_nets(unpack_weights(w)) puts trained weights back."""
        return torch.from_numpy(self._packed.copy()).to(self.device)

    def _head_weight_gradient(self, features, grad_q, wdev, baseband_weight=None):
        """(g [ML_WEIGHTS] float32, g_baseband_weight 0-dim float32) of sum_b grad_q[b] Q[b]: one cvvdp_ml_saliency_head_grad call per
        band into one float64 accumulator."""
        B, C, mask, lib, stream, bands = self._head_bands(features, baseband_weight)
        gq = torch.ones((B,), dtype=torch.float32, device=self.device) if grad_q is None else \
            torch.as_tensor(grad_q).detach().to(self.device, torch.float32).contiguous().reshape(-1)
        if gq.numel() != B:
            raise ValueError(f"grad_q has {gq.numel()} values for {B} batch items")
        no_bands = len(features)
        with torch.cuda.device(self.device):
            acc = torch.zeros((_capi.ML_WEIGHTS,), dtype=torch.float64, device=self.device)
            d_scale = torch.zeros((B,), dtype=torch.float32, device=self.device)
            for bb, (f, F, Hc, Wc, scale) in enumerate(bands):
                nbytes = lib.cvvdp_ml_saliency_head_grad_scratch_bytes(B, F, Hc, Wc)
                scratch = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=self.device)
                last = bb == no_bands - 1
                rc = lib.cvvdp_ml_saliency_head_grad(self._handle, f.data_ptr(), B, F, Hc, Wc, C, wdev.data_ptr(), scale, mask, gq.data_ptr(),
                                                     acc.data_ptr(), d_scale.data_ptr() if last else None, scratch.data_ptr(), nbytes, stream)
                _capi.check(self._handle, rc, "cvvdp_ml_saliency_head_grad")
            # Q[b] = ... + (baseband_weight / bands) (image_int) d_scale[b] on the last band
            factor = (1.0 / no_bands) * (float(f32(self.parameters["image_int"])) if C == 3 else 1.0)
            g_bw = ((gq.double() * d_scale.double()).sum() * factor).float()
            return acc.float(), g_bw

    # ------------------------------------------------------------------ the gradient in the features
    def _head_input_gradient(self, features, wdev, baseband_weight=None):
        """[dQ[b] / d features[band][b]] as new float32 device tensors with the shapes of the features: one
        cvvdp_ml_saliency_head_input_grad call per band."""
        B, C, mask, lib, stream, bands = self._head_bands(features, baseband_weight)
        out = []
        with torch.cuda.device(self.device):
            for f, F, Hc, Wc, scale in bands:
                g = torch.empty_like(f)
                rc = lib.cvvdp_ml_saliency_head_input_grad(self._handle, f.data_ptr(), B, F, Hc, Wc, C, wdev.data_ptr(), scale, mask,
                                                           g.data_ptr(), g.numel() * 4, stream)
                _capi.check(self._handle, rc, "cvvdp_ml_saliency_head_input_grad")
                out.append(g)
        return out

    def do_pooling_and_jods_with_feature_gradient(self, features, weights=None):
        """(Q [B], [g per band]) on the device: Q_JOD of do_pooling_and_jods (the same kernel: the same bits) and per band
        g[b, ...] = dQ[b] / d features[band][b, ...], float32 with the shape of the band's features: what autograd through the
        reference's head leaves in features[band].grad for the loss Q.sum() (all six statistics, those of the reference included).
        weights: a packed float32 tensor (weight_tensor()) in place of the metric's own networks.  torch's conventions (relu'(0) = 0);
        where a variance is exactly 0 the derivative of sqrt(|v|) is taken as 0 (autograd gives NaN there); disabled_features have
        gradient exactly 0.  The same bits on every call; features and weights are only read."""
        wdev = self._weights_arg(weights)
        return self._head_forward(features, wdev), self._head_input_gradient(features, wdev)

    # ------------------------------------------------------------------ the metric as an image loss
    def predict_with_gradient(self, test, reference, dim_order="BCFHW", frames_per_second=0, block_frames=None, wrt="test"):
        """(jod, grad) of an image: `jod` as predict() returns it (the same kernels on the same tensors: the same bits), `grad` =
        d jod / d test, float32 on the device, with the shape of `test` in the caller's dim_order; for a batch, grad[b] is the gradient
        of jod[b] (items do not interact; the reference may have a batch of 1).  float32 tensors on the metric's device, three channels,
        one frame; sRGB, numeric-gamma and linear displays.  Refused with a vq_exception: clips, wrt = "reference" / "both" (the
        sensitivity and the R statistics move with the reference), and what cvvdp.predict_with_gradient refuses (1-channel content,
        other dtypes, PQ / HLG displays).  The backward: the head's gradient in the features (cvvdp_ml_saliency_head_input_grad),
        then cvvdp_ml_image_gradient on the pyramid the forward left in the workspace.  The same bits on every run."""
        if wrt != "test" and isinstance(wrt, str) and wrt in _capi.WRT:      # (anything else: _gradient_inputs names the valid values)
            raise vq_exception(f'{self._TITLE}: predict_with_gradient has no gradient in the reference (wrt = {wrt!r}): the sensitivity and the '
                               'R statistics of the features move with it; wrt = "test" only')
        order = str(dim_order).upper()
        if torch.is_tensor(test) and len(order) == test.dim() and "F" in order and test.shape[order.index("F")] > 1:
            raise vq_exception(f"{self._TITLE}: predict_with_gradient is for images, clips are out of scope "
                               f"({test.shape[order.index('F')]} frames were passed)")
        t, r = self._gradient_inputs(test, reference, dim_order, 0, None, wrt)
        if self._shard is not None:
            raise vq_exception("predict_with_gradient: not available with frame sharding")
        vs = video_source_array(t, r, 0, dim_order="BCFHW", display_photometry=self.display_photometry)
        features, _ = self.extract_features(vs)
        wdev = self._weights_arg(None)
        jod = self._head_forward(features, wdev)
        gfeat = self._head_input_gradient(features, wdev)
        lib = _capi.lib()
        out = GradOut(test, reference, dim_order, wrt, self.device)
        n = len(features)
        pf, pg = (ctypes.c_void_p * n)(*(f.data_ptr() for f in features)), (ctypes.c_void_p * n)(*(g.data_ptr() for g in gfeat))
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(int(lib.cvvdp_ml_image_gradient_scratch_bytes(self._handle)), 16), dtype=torch.uint8, device=self.device)
            rc = lib.cvvdp_ml_image_gradient(self._handle, t.data_ptr(), (ctypes.c_int64 * 5)(*t.stride()), pf, pg, n, *out.args("test"),
                                             scratch.data_ptr(), scratch.numel(), ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _capi.check(self._handle, rc, "cvvdp_ml_image_gradient")
        return jod.squeeze(), out.result()

    def differentiable_loss(self, test, reference, dim_order="BCFHW", frames_per_second=0, block_frames=None, wrt="test"):
        """10 - JOD of an image as a tensor attached to autograd (cvvdp.differentiable_loss: the same autograd function).  backward()
        multiplies the gradient predict_with_gradient() stored by the upstream gradient, one factor per batch item; the reference
        receives None, and a reference that requires a gradient is refused."""
        if torch.is_tensor(reference) and reference.requires_grad:
            raise vq_exception(f"{self._TITLE}: differentiable_loss has no gradient for the reference")
        predict = lambda: self.predict_with_gradient(test, reference, dim_order, frames_per_second, block_frames, wrt)
        return PixelLoss.apply(test, reference, predict, 10.0, dim_order, wrt)

    def do_pooling_and_jods_with_weight_gradient(self, features, grad_q=None, weights=None):
        """(Q [B], g [ML_WEIGHTS] float32, g_baseband_weight) on the device: Q_JOD of do_pooling_and_jods (the same kernel: the same
        bits) and the gradient of sum_b grad_q[b] Q[b] (grad_q: ones) in the packed weights and in the model's scalar baseband_weight.
        weights: a packed float32 tensor (weight_tensor()) in place of the metric's own networks.  torch's conventions (relu'(0) = 0);
        entries that cannot act are exactly 0: the first-layer columns of an image's fourth channel and of disabled_features, the
        padding.  The same bits on every call; features and weights are only read."""
        wdev = self._weights_arg(weights)
        Q = self._head_forward(features, wdev)
        g, g_bw = self._head_weight_gradient(features, grad_q, wdev)
        return Q, g, g_bw

    def differentiable_jods(self, features, weights, baseband_weight=None):
        """Q_JOD [B] attached to autograd in `weights` (a packed float32 tensor, weight_tensor()) and, if given, in the scalar tensor
        `baseband_weight`, whose value then replaces the model's.  backward() runs the HIP gradient with the upstream factors as
        grad_q.  The features carry no gradient."""
        if not torch.is_tensor(weights):
            raise ValueError("differentiable_jods: weights must be a tensor (weight_tensor())")
        if baseband_weight is not None and (not torch.is_tensor(baseband_weight) or baseband_weight.numel() != 1):
            raise ValueError("differentiable_jods: baseband_weight must be a tensor of one value")
        for f in features:
            if torch.is_tensor(f) and f.requires_grad:
                raise vq_exception("differentiable_jods: the gradient in the features is out of scope")
        return _HeadJods.apply(self, features, weights, baseband_weight)

    def predict_video_source_with_weight_gradient(self, vid_source, grad_q=None):
        vid_source, size, (Q, g, g_bw) = self._score_source(vid_source, lambda features: self.do_pooling_and_jods_with_weight_gradient(features, grad_q))
        return Q.squeeze(), g, g_bw, self._source_stats(vid_source, size)

    def predict_with_weight_gradient(self, test_cont, reference_cont, dim_order="BCFHW", frames_per_second=0, grad_q=None):
        """(Q_JOD as predict() returns it, g [ML_WEIGHTS], g_baseband_weight, stats): the features of the content, then
        do_pooling_and_jods_with_weight_gradient.  Refuses what predict() refuses."""
        vs = video_source_array(test_cont, reference_cont, frames_per_second, dim_order=dim_order, display_photometry=self.display_photometry)
        return self.predict_video_source_with_weight_gradient(vs, grad_q)

    def full_name(self):
        return "ColorVideoVDP-ML-Saliency"


register_metric(cvvdp_ml_saliency)


# ---------------------------------------------------------------------------------------------------------------- cvvdp-ml-transformer
MT_DIM, MT_HEADS, MT_FF, MT_LAYERS, MT_INPUTS = 256, 8, 1024, 4, 24


def transformer_entries():
    """[(key, shape)] of the 55 entries of RegressionTransformer(in_channels=24, dim=256) (cvvdp_ml_metric.py:553-587), in the order
    of its state dict."""
    e = [("cls_token", (1, 1, MT_DIM)), ("patch_embed.1.weight", (MT_DIM, MT_INPUTS)), ("patch_embed.1.bias", (MT_DIM,))]
    for l in range(MT_LAYERS):
        p = f"transformer.layers.{l}."
        e += [(p + "self_attn.in_proj_weight", (3 * MT_DIM, MT_DIM)), (p + "self_attn.in_proj_bias", (3 * MT_DIM,)),
              (p + "self_attn.out_proj.weight", (MT_DIM, MT_DIM)), (p + "self_attn.out_proj.bias", (MT_DIM,)),
              (p + "linear1.weight", (MT_FF, MT_DIM)), (p + "linear1.bias", (MT_FF,)),
              (p + "linear2.weight", (MT_DIM, MT_FF)), (p + "linear2.bias", (MT_DIM,)),
              (p + "norm1.weight", (MT_DIM,)), (p + "norm1.bias", (MT_DIM,)), (p + "norm2.weight", (MT_DIM,)), (p + "norm2.bias", (MT_DIM,))]
    return e + [("reg_head.0.weight", (MT_DIM,)), ("reg_head.0.bias", (MT_DIM,)), ("reg_head.1.weight", (1, MT_DIM)), ("reg_head.1.bias", (1,))]


def transformer_from_state_dict(state_dict):
    """{key without the `transformer_net.` prefix: float32 CPU tensor} of the 55 entries, from a state dict that holds them under
    `transformer_net.` (what a checkpoint's `state_dict` holds).  A missing entry, a wrong shape or an entry under `transformer_net.`
    that the network does not have raises a RuntimeError that names the key; entries of other networks are not looked at."""
    prefix = "transformer_net."
    want = dict(transformer_entries())
    for key in state_dict:
        if key.startswith(prefix) and key[len(prefix):] not in want:
            raise RuntimeError(f"checkpoint entry '{key}' is no part of the transformer head (4 layers of width {MT_DIM})")
    net = {}
    for name, shape in want.items():
        key = prefix + name
        if key not in state_dict:
            raise RuntimeError(f"checkpoint entry '{key}' is missing")
        t = torch.as_tensor(state_dict[key])
        if tuple(t.shape) != shape:
            raise RuntimeError(f"checkpoint entry '{key}' has shape {tuple(t.shape)}, the transformer head needs {shape}")
        net[name] = t.detach().to("cpu", torch.float32).contiguous()
    return net


def random_transformer():
    """The network with torch's default initialisation of the reference's modules (random_init=True)."""
    emb = torch.nn.Linear(MT_INPUTS, MT_DIM)
    net = {"cls_token": torch.randn(1, 1, MT_DIM), "patch_embed.1.weight": emb.weight, "patch_embed.1.bias": emb.bias}
    for l in range(MT_LAYERS):
        layer = torch.nn.TransformerEncoderLayer(d_model=MT_DIM, nhead=MT_HEADS, dim_feedforward=MT_FF, activation="gelu", batch_first=True,
                                                 norm_first=True)
        net.update({f"transformer.layers.{l}.{k}": v for k, v in layer.state_dict().items()})
    norm, lin = torch.nn.LayerNorm(MT_DIM), torch.nn.Linear(MT_DIM, 1)
    net.update({"reg_head.0.weight": norm.weight, "reg_head.0.bias": norm.bias, "reg_head.1.weight": lin.weight, "reg_head.1.bias": lin.bias})
    return transformer_from_state_dict({"transformer_net." + k: v.detach().clone() for k, v in net.items()})


def _mt_layout():
    """[(key, float offset, transposed)] of the packed buffer cvvdp_ml_transformer_head documents."""
    D, FF = MT_DIM, MT_FF
    out = [("cls_token", 0, False), ("patch_embed.1.weight", D, True), ("patch_embed.1.bias", D + MT_INPUTS * D, False)]
    pos = 2 * D + MT_INPUTS * D
    for l in range(MT_LAYERS):
        p = f"transformer.layers.{l}."
        for name, n, tr in (("norm1.weight", D, False), ("norm1.bias", D, False), ("self_attn.in_proj_weight", 3 * D * D, True),
                            ("self_attn.in_proj_bias", 3 * D, False), ("self_attn.out_proj.weight", D * D, True),
                            ("self_attn.out_proj.bias", D, False), ("norm2.weight", D, False), ("norm2.bias", D, False),
                            ("linear1.weight", D * FF, True), ("linear1.bias", FF, False), ("linear2.weight", FF * D, True),
                            ("linear2.bias", D, False)):
            out.append((p + name, pos, tr))
            pos += n
    for name, n in (("reg_head.0.weight", D), ("reg_head.0.bias", D), ("reg_head.1.weight", D), ("reg_head.1.bias", 1)):
        out.append((name, pos, False))
        pos += n
    assert pos + 3 == _capi.MT_WEIGHTS
    return out


def pack_transformer(net):
    """float32 [MT_WEIGHTS]: every matrix transposed to [in][out], in the order cvvdp_ml_transformer_head documents."""
    out = np.zeros(_capi.MT_WEIGHTS, dtype=f32)
    for key, pos, tr in _mt_layout():
        a = net[key].numpy()
        a = np.ascontiguousarray(a.T if tr else a).reshape(-1)
        out[pos:pos + a.size] = a
    return out


class cvvdp_ml_transformer(_cvvdp_ml):
    """ColorVideoVDP-ML-Transformer.  `patch_size` and `dim` are the reference's constructor arguments, which its network does not
    use beyond storing them; the kernels are written for dim = 256."""
    _MODEL, _TITLE = "cvvdp_ml_transformer", "cvvdp-ml-transformer"
    _WHERE = ("Pass the directory that holds the reference's cvvdp_ml_transformer/cvvdp_parameters.json and its cvvdp.ckpt as "
              "config_paths=[dir]: this package ships neither file.")
    _random_nets = staticmethod(random_transformer)
    _nets_from_state_dict = staticmethod(transformer_from_state_dict)

    def __init__(self, patch_size=(9, 16), dim=256, config_paths=[], **kwargs):
        if dim != MT_DIM:
            raise ValueError(f"cvvdp_ml_transformer: dim = {dim}, the model and its kernels are {MT_DIM} wide")
        self.patch_size = patch_size
        super().__init__(config_paths=config_paths, **kwargs)

    def _set_nets(self, net):
        self._nets = net
        self._packed = pack_transformer(net)
        self._weights_dev = None

    def load_state_dict_nets(self, state_dict):
        """Replace the network from a state dict with the 55 `transformer_net.*` entries; validated like a checkpoint, and nothing
        changes if it does not validate."""
        self._set_nets(transformer_from_state_dict(state_dict))

    def state_dict_nets(self):
        """The network as a state dict with the reference's keys (`transformer_net.cls_token`, ...)."""
        return {"transformer_net." + k: t.clone() for k, t in self._nets.items()}

    def packed_weights(self):
        """float32 [MT_WEIGHTS]: the buffer the kernels read (pack_transformer)."""
        return self._packed.copy()

    def do_pooling_and_jods(self, features, return_y=False):
        """cvvdp_ml_transformer.do_pooling_and_jods (cvvdp_ml_metric.py:647-675): features[band] is [B, F, H', W', C, 6] (any list of
        such tensors; C = 3 marks an image) -> Q_JOD[B] on the device.  One cvvdp_ml_transformer_head call per band; unlike the
        reference's, this one leaves the caller's tensors as they are.  With return_y also the list of y [B, F] per band, the
        head's output per (item, frame) before the mean."""
        B, C, bands = self._check_features(features)
        if self._weights_dev is None:
            self._weights_dev = torch.from_numpy(self._packed).to(self.device)
        mask = sum(1 << s for s in set(self.disabled_features or ()))
        lib = _capi.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        ys = []
        with torch.cuda.device(self.device):
            Q = torch.full((B,), 10.0, dtype=torch.float32, device=self.device)
            for f, scale in bands:
                _, F, Hc, Wc = (int(n) for n in f.shape[:4])
                nbytes = lib.cvvdp_ml_transformer_head_scratch_bytes(B, F, Hc, Wc)
                scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
                y = torch.empty((B, F), dtype=torch.float32, device=self.device) if return_y else None
                rc = lib.cvvdp_ml_transformer_head(self._handle, f.data_ptr(), B, F, Hc, Wc, C, self._weights_dev.data_ptr(), scale, mask,
                                                   Q.data_ptr(), y.data_ptr() if return_y else None, scratch.data_ptr(), nbytes, stream)
                _capi.check(self._handle, rc, "cvvdp_ml_transformer_head")
                ys.append(y)
        return (Q, ys) if return_y else Q

    def full_name(self):
        return "ColorVideoVDP-ML-Transformer"


# (not registered: the -m choices of the command line come from the registry, and this metric is not on the command line yet)
