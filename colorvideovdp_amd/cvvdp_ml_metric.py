"""ColorVideoVDP-ML-Saliency (pycvvdp/cvvdp_ml_metric.py:463-550 `class cvvdp_ml_saliency`) for MI355X: the base model's pooled
per-band features (`cvvdp.extract_features`) scored by two small MLPs, a saliency ("attention") net on the statistics of test and
reference and a difference net on the statistics of D, at every feature cell.

Same constructor arguments, methods, names and errors as the reference class.  The features come from the band kernels' feature
route, unchanged; the head is one HIP pass per band (cvvdp_ml_saliency_head, include/cvvdp_hip.h; csrc/ml_head.hip).

Where the two files of the model come from: the reference package ships `vvdp_data/cvvdp_ml_saliency/cvvdp_parameters.json` and fetches
the trained networks, `cvvdp_ml_saliency/cvvdp.ckpt`, when its class is first constructed.  This package ships neither and fetches
nothing: the directory that holds both is passed as `config_paths=[dir]` (`-c dir` on the command line).  A `cvvdp_ml_saliency`
sub-directory of a configuration directory is looked into first, so the parent of the reference's layout works as well.

Not available: `cvvdp_ml_transformer` (a 4-layer transformer encoder over all cells of a frame), heat maps, distograms, frame sharding.
"""
import ctypes
import logging
import os

import numpy as np
import torch

from . import _capi
from . import host_setup as hs
from .config import config_files, json2dict
from .cvvdp_metric import cvvdp
from .video_source import video_source
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


class cvvdp_ml_saliency(cvvdp):
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
        own = [os.path.join(cp, "cvvdp_ml_saliency") for cp in config_paths if os.path.isdir(os.path.join(cp, "cvvdp_ml_saliency"))]
        try:
            pfile = config_files.find("cvvdp_parameters.json", own + config_paths)
        except RuntimeError as e:
            raise vq_exception(f"{e}. {_WHERE}") from None
        if pfile.startswith("builtin:"):
            raise vq_exception("The parameter file of cvvdp-ml-saliency (cvvdp_parameters.json with internal_model_name 'cvvdp_ml_saliency') was not "
                               f"found in the configuration paths. {_WHERE}")
        p = dict(json2dict(pfile))
        bw = p.get("baseband_weight")
        if p.get("internal_model_name") != "cvvdp_ml_saliency" or isinstance(bw, (list, tuple)):
            raise vq_exception(f"'{pfile}' is not the parameter file of cvvdp-ml-saliency (internal_model_name "
                               f"'{p.get('internal_model_name')}': the base model's file?). {_WHERE}")
        if isinstance(bw, (str, bool)) or bw is None or not np.isfinite(float(bw)):
            raise RuntimeError("parameter 'baseband_weight' of cvvdp-ml-saliency must be a finite number")
        if self.random_init:
            nets = random_nets()
        else:
            try:
                ckpt = config_files.find("cvvdp.ckpt", own + config_paths)
            except RuntimeError:
                raise vq_exception(f"The checkpoint of cvvdp-ml-saliency (cvvdp.ckpt) was not found in the configuration paths. {_WHERE}") from None
            logging.info(f"Loading cvvdp checkpoint file from {ckpt}")
            nets = nets_from_state_dict(torch.load(ckpt, map_location="cpu")["state_dict"])
        self.parameters_file = pfile
        self._config_paths = list(config_paths)
        p["baseband_weight"] = [float(bw)] * 4
        self._set_parameters(p)
        self._ml_baseband_weight = f32(bw)
        self._set_nets(nets)

    def _set_nets(self, nets):
        self._nets = nets
        self._packed = pack_weights(nets)
        self._weights_dev = None

    def load_state_dict_nets(self, state_dict):
        """Replace both networks from a state dict with `att_net.<i>.weight` / `.bias` and `feature_net.<i>.weight` / `.bias` entries
        (what a checkpoint's `state_dict` holds); validated like a checkpoint, and nothing changes if it does not validate."""
        self._set_nets(nets_from_state_dict(state_dict))

    def state_dict_nets(self):
        """The networks as a state dict with torchvision's layer indices (0, 3, 6, ...)."""
        return {f"{net}.{3 * k}.{kind}": t.clone() for net, layers in self._nets.items() for k, wb in enumerate(layers)
                for kind, t in zip(("weight", "bias"), wb)}

    def packed_weights(self):
        """float32 [ML_WEIGHTS]: the buffer the kernel reads (pack_weights)."""
        return self._packed.copy()

    def set_frame_sharding(self, group="world"):
        if group is not None:
            raise vq_exception("cvvdp-ml metrics cannot be sharded over frames: the head pools over all frames of the clip")
        self._shard = None

    # ------------------------------------------------------------------ public API
    def predict_video_source(self, vid_source):
        """cvvdp_ml_base.predict_video_source (cvvdp_ml_metric.py:174-201)."""
        inner = getattr(vid_source, "vs", None)
        if isinstance(inner, video_source):
            vid_source = inner
        if hasattr(vid_source, "set_temporal_filters"):
            raise vq_exception("--temp-resample sources are scored by the cvvdp metric only")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        height, width, N_frames = vid_source.get_video_size()
        # a raw source that carries its own display photometry is measured with it, as in cvvdp.predict_video_source
        src_dm = getattr(vid_source, "dm_photometry", None)
        swap = src_dm is not None and src_dm is not self.display_photometry and self._is_raw_source(vid_source)
        if swap:
            prev = self.display_photometry
            self.display_photometry = src_dm
            self._make_handle()
        try:
            features, _ = self.extract_features(vid_source)
            Q_jod = self.do_pooling_and_jods(features)
        finally:
            if swap:
                self.display_photometry = prev
                self._make_handle()
        pyr_height, freqs = hs.band_frequencies(width, height, self.pix_per_deg)
        rho_band = freqs.copy()
        rho_band[pyr_height] = 0.1
        stats = {"rho_band": rho_band, "frames_per_second": vid_source.get_frames_per_second(), "width": width, "height": height,
                 "N_frames": N_frames}
        return (Q_jod.squeeze(), stats)

    def do_pooling_and_jods(self, features):
        """cvvdp_ml_saliency.do_pooling_and_jods (cvvdp_ml_metric.py:496-541): features[band] is [B, F, H', W', C, 6] (any list of such
        tensors; C = 3 marks an image) -> Q_JOD[B] on the device.  One cvvdp_ml_saliency_head call per band; unlike the reference's,
        this one leaves the caller's tensors as they are."""
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        no_bands = len(features)
        if no_bands < 1:
            raise ValueError("do_pooling_and_jods: no bands")
        B, C = int(features[0].shape[0]), int(features[0].shape[4])
        if self._weights_dev is None:
            self._weights_dev = torch.from_numpy(self._packed).to(self.device)
        mask = sum(1 << s for s in set(self.disabled_features or ()))
        lib = _capi.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            Q = torch.full((B,), 10.0, dtype=torch.float32, device=self.device)
            for bb, f in enumerate(features):
                f = torch.as_tensor(f).to(self.device, torch.float32).contiguous()
                if f.dim() != 6 or f.shape[5] != 6 or f.shape[0] != B or f.shape[4] != C:
                    raise ValueError(f"features[{bb}] has shape {tuple(f.shape)}, expected [{B}, F, H', W', {C}, 6]")
                if f.data_ptr() % (16 if C == 4 else 8):           # (a view into a larger buffer: the kernel reads 16 / 8 bytes at a time)
                    f = f.clone()
                scale = 1.0 / no_bands
                if bb == no_bands - 1:
                    scale *= float(self._ml_baseband_weight)
                if C == 3:
                    scale *= float(f32(self.parameters["image_int"]))
                _, F, Hc, Wc = (int(n) for n in f.shape[:4])
                nbytes = lib.cvvdp_ml_saliency_head_scratch_bytes(B, F, Hc, Wc)
                scratch = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=self.device)
                rc = lib.cvvdp_ml_saliency_head(self._handle, f.data_ptr(), B, F, Hc, Wc, C, self._weights_dev.data_ptr(), scale, mask,
                                                Q.data_ptr(), scratch.data_ptr(), nbytes, stream)
                _capi.check(self._handle, rc, "cvvdp_ml_saliency_head")
        return Q

    def full_name(self):
        return "ColorVideoVDP-ML-Saliency"

    def short_name(self):
        return self.__class__.__name__.replace("_", "-")

    def export_distogram(self, stats, fname, jod_max=None, base_size=6):
        raise vq_exception("Currently cvvdp-ml metrics do not export distograms")


register_metric(cvvdp_ml_saliency)
