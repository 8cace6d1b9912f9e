"""The gradients of the cvvdp metric, as two mixins of `cvvdp_metric.cvvdp`.

cvvdp_pixel_gradient: `predict_with_gradient` and `differentiable_loss`, the JOD's gradient in the test and the reference.  The forward is
that of `predict()` on the core's unfused route (fuse_mode = 2), which keeps every pyramid level in the workspace; the backward runs in HIP
on that pyramid (cvvdp_image_gradient, cvvdp_video_gradient, cvvdp_video_gradient_block and their *_wrt siblings, include/cvvdp_hip.h;
DESIGN.md 7f-7k) with torch's subgradient conventions and gives the same bits on every run.  What a call sets on the metric for itself
is put back by `_borrowed`; the gradient buffers, the common checks and the autograd function are those of _pixel_grad.py.

cvvdp_parameter_gradient: `predict_with_parameter_gradient`, `predict_video_source_with_parameter_gradient`, `parameter_tensors` and
`differentiable_jod`, the JOD's gradient in the model's own parameters, for calibration.  The pooling stage is restated in
float64 torch (pool_jod_float64) and differentiated by autograd on the host; the band stage's 24 sums come from cvvdp_param_gradient
(csrc/grad_param.hip) after every block.

The metric supplies `_score_range`, `do_pooling_and_jods`, `_make_handle`, `_set_parameters`, `_parameter_value`, `_is_raw_source` and the
state they read (`_handle`, `_ws`, `_shard`, `parameters`, `display_photometry`, ...).
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _capi
from . import host_setup as hs
from ._pixel_grad import GradOut, PixelLoss, bcfhw_views, check_float32_tensors, check_wrt
from .video_source import video_source, video_source_array
from .vq_metric import vq_exception

f32 = np.float32


class cvvdp_pixel_gradient:
    def _gradient_inputs(self, test, reference, dim_order, frames_per_second=0, block_frames=None, wrt="test"):
        """What predict_with_gradient refuses, checked before anything touches the device; returns the BCFHW views."""
        what = "predict_with_gradient"
        check_wrt(what, wrt)
        if block_frames is not None and block_frames != "auto":
            if isinstance(block_frames, bool) or not isinstance(block_frames, (int, np.integer)) or block_frames < 1:
                raise vq_exception(f'predict_with_gradient: block_frames must be None, "auto" or an integer >= 1, not {block_frames!r}')
        check_float32_tensors(what, test, reference)
        if self.do_heatmap:
            raise vq_exception("predict_with_gradient: not available with a heat map")
        if self.dump_channels is not None:
            raise vq_exception("predict_with_gradient: not available with dump_channels")
        t, r = bcfhw_views(what, test, reference, dim_order)
        if t.shape[2] != r.shape[2]:
            raise vq_exception("predict_with_gradient: the reference must have the test's shape (or a batch of 1)")
        if t.shape[2] > 1:
            if not frames_per_second > 0:
                raise vq_exception("predict_with_gradient: a video needs frames_per_second (more than one frame was passed)")
            fl = hs.temporal_filters(frames_per_second, self.parameters["beta_tf"], self.parameters["sigma_tf"]).shape[1]
            if fl > _capi.MAX_FILTER_LEN:
                raise vq_exception(f"frame rates above {(_capi.MAX_FILTER_LEN - 1) * 4} fps are not supported")
            if block_frames is not None:
                nb = t.shape[2] if block_frames == "auto" else min(int(block_frames), t.shape[2])
                if block_frames != "auto" and nb + fl - 1 > _capi.MAX_WINDOW:
                    raise vq_exception(f"predict_with_gradient: block_frames = {nb} with a filter of {fl} taps exceeds the window limit of a temporal block, "
                                       f"CVVDP_MAX_WINDOW = {_capi.MAX_WINDOW} (block_frames + filter_len - 1)")
            elif t.shape[2] + fl - 1 > _capi.MAX_WINDOW:
                raise vq_exception(f"predict_with_gradient: the video must be scored as one temporal block, and {t.shape[2]} frames with a filter of {fl} taps "
                                   f"exceed the window limit CVVDP_MAX_WINDOW = {_capi.MAX_WINDOW} (n_frames + filter_len - 1)")
        if t.shape[1] != 3 or r.shape[1] != 3:
            raise vq_exception("predict_with_gradient: 1-channel content is out of scope, the images must have three colour channels")
        if tuple(t.shape[3:]) != tuple(r.shape[3:]) or (r.shape[0] != t.shape[0] and r.shape[0] != 1):
            raise vq_exception("predict_with_gradient: the reference must have the test's shape (or a batch of 1)")
        if wrt != "test" and r.shape[0] != t.shape[0]:
            raise vq_exception(f"predict_with_gradient: a reference of batch 1 against a test batch of {t.shape[0]} is refused with wrt = {wrt!r}: "
                               "the gradient of the broadcast would be a sum over the items (expand the reference to the test's batch)")
        eotf, _ = self.display_photometry.eotf_params()
        if eotf in (1, 2):      # CVVDP_EOTF_PQ, CVVDP_EOTF_HLG
            raise vq_exception("predict_with_gradient: PQ and HLG displays are refused (the reference's own gradient is NaN as soon as a sample is 0)")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        if t.device != self.device or r.device != self.device:
            raise vq_exception(f"predict_with_gradient: test and reference must be tensors on {self.device}")
        return t, r

    def predict_with_gradient(self, test, reference, dim_order="BCFHW", frames_per_second=0, block_frames=None, wrt="test"):
        """(jod, grad) of an image or of a short clip: `jod` as predict() returns it, `grad` = d jod / d test, float32 on the device, with
        the shape of `test` in the caller's dim_order; for a batch, grad[b] is the gradient of jod[b] (items do not interact).  float32
        tensors on the metric's device, three channels; sRGB, numeric-gamma and linear displays.  1-channel content, other dtypes, heat
        maps, dump_channels and PQ / HLG displays are refused with a vq_exception; there is no gradient for the reference.
        The backward runs in HIP on the pyramid the forward left in the workspace, with torch's subgradient conventions, and gives the
        same bits on every run.
        Images (one frame; cvvdp_image_gradient, csrc/grad.hip) are always scored on the core's unfused route: the JOD is that of predict().
        Clips (more than one frame, frames_per_second > 0; cvvdp_video_gradient, csrc/grad_video.hip) go through temporal masking and the
        transient channel, with temp_padding 'replicate' or 'symmetric'.  The clip is scored as ONE temporal block on the unfused route:
        fuse_mode = 2 and block_frames = n_frames are set for this call and restored, so the JOD is that of predict() with those two
        settings, and equal to the default predict() to the rounding between the routes.  A clip whose window n_frames + filter_len - 1
        exceeds CVVDP_MAX_WINDOW (256), or whose workspace and scratch (about 75 bytes per pixel, frame and batch item on top of the
        forward's 43) cannot be allocated, is refused.
        Clips of any length: block_frames = N (an integer >= 1) scores and differentiates the clip in temporal blocks of N frames, the
        last one shorter (cvvdp_video_gradient_block, csrc/grad_blocks.hip): fuse_mode = 2 and block_frames = N are set for the call and
        restored, the JOD is that of predict() with those two settings, bit for bit, and the gradient is the same bits for every N
        (N >= n_frames included).  Against block_frames = None, where that is accepted, the JOD is the same bits and the gradient is
        the same bits under symmetric padding and beyond 33 taps; under replicate padding up to 33 taps the two differ in how one
        multiply-add per tap is fused (1e-7 of the largest sample).  The clip is walked twice (pooling over frames couples the frames); a clip
        of one block once.  Workspace and scratch then grow with N, not with the clip: about 118 bytes per pixel and batch item x N, plus
        12 bytes x filter_len for what a block border cuts; only `grad` has the clip's size.  N + filter_len - 1 must not exceed
        CVVDP_MAX_WINDOW.  block_frames = "auto" takes the largest N the window limit and the free memory allow.  Images ignore it.
        wrt = "reference" returns (jod, grad_reference), d jod / d reference with the shape of `reference`; wrt = "both" returns
        (jod, (grad_test, grad_reference)).  Every route above takes it (the *_wrt entries); jod and grad_test are the bits of
        wrt = "test", grad_reference the same bits for "reference" and "both" and, in blocks, for every N.  "both" runs the steps the two
        sides share once and needs a second set of per-level planes: about 79 bytes per pixel and item for an image, 101 per pixel, frame
        and item for a clip.  The refusals hold for both tensors; a reference of batch 1 against a larger test batch is refused as well.
        Out of scope: file sources, .yuv, --temp-resample, frame sharding."""
        t, r = self._gradient_inputs(test, reference, dim_order, frames_per_second, block_frames, wrt)
        sides = (test, t, reference, r, wrt)
        if t.shape[2] > 1:
            if block_frames is not None:
                return self._predict_video_with_gradient_blocks(sides, dim_order, frames_per_second, block_frames)
            return self._predict_video_with_gradient(sides, dim_order, frames_per_second)
        vs = video_source_array(t, r, 0, dim_order="BCFHW", display_photometry=self.display_photometry)
        Q, _, _ = self._score_range(vs, 0, 1)
        jod = self.do_pooling_and_jods(Q)
        grad, _, call = self._pixel_gradient_entry("cvvdp_image_gradient", "cvvdp_image_gradient_scratch_bytes", sides, dim_order)
        call()
        return jod.squeeze(), grad

    @contextlib.contextmanager
    def _borrowed(self, **settings):
        """What a gradient call sets for itself (fuse_mode, block_frames, _pixel_grad_plan, _param_grad_plan), put back on every exit path
        together with the hook the second walk runs after each block.  Yields no_memory(text): a guard under which an allocation that
        fails gives up the workspace and raises a vq_exception with text()."""
        saved = {k: getattr(self, k, False) for k in settings}
        for k, v in settings.items():
            setattr(self, k, v)

        @contextlib.contextmanager
        def no_memory(text):
            try:
                yield
            except torch.cuda.OutOfMemoryError:
                self._ws = None
                raise vq_exception(text()) from None

        try:
            yield no_memory
        finally:
            for k, v in saved.items():
                setattr(self, k, v)
            self._block_hook = None

    def _pixel_gradient_entry(self, name, scratch_name, sides, dim_order, guard=None):
        """Everything between the forward and the C entry `name` of a pixel gradient; sides = (test, t, reference, r, wrt), t and r the
        BCFHW views on the device.  wrt = "test" calls `name` itself, the other two its sibling `name`_wrt.  Returns what
        predict_with_gradient returns for this wrt: grad, float32 with the shape of `test` (of `reference`; the pair of them); the scratch
        of as many bytes as the entry `scratch_name` answers, allocated under `guard` (stream-ordered: the caching allocator may hand it
        out again once the kernels are queued); and call(stream=None), which runs the entry on the stream (None: torch's current one) and checks it."""
        test, t, reference, r, wrt = sides
        lib = _capi.lib()
        out = GradOut(test, reference, dim_order, wrt, self.device)

        def frames(side, view):         # the input a side's gradient is taken in
            return (view.data_ptr(), (ctypes.c_int64 * 5)(*view.stride())) if wrt in (side, "both") else (None, None)

        if wrt == "test":
            code, args = (), frames("test", t) + out.args("test")
        else:
            name, scratch_name, code = name + "_wrt", scratch_name.replace("_scratch_bytes", "_wrt_scratch_bytes"), (_capi.WRT[wrt],)
            args = frames("test", t) + frames("reference", r) + out.args("test") + out.args("reference")
        with guard or contextlib.nullcontext():
            scratch = torch.empty(max(int(getattr(lib, scratch_name)(self._handle, *code)), 16), dtype=torch.uint8, device=self.device)
        entry = getattr(lib, name)

        def call(stream=None):
            stream = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
            rc = entry(self._handle, *code, *args, scratch.data_ptr(), scratch.numel(), stream)
            _capi.check(self._handle, rc, name)

        return out.result(), scratch, call

    def _predict_video_with_gradient(self, sides, dim_order, frames_per_second):
        """predict_with_gradient for a clip: sides = (test, t, reference, r, wrt); t, r are the BCFHW views on the device."""
        _, t, _, r, wrt = sides
        if self._shard is not None:
            raise vq_exception("predict_with_gradient: not available with frame sharding")
        lib = _capi.lib()
        n_frames = int(t.shape[2])

        def text():
            ws, sc = int(lib.cvvdp_workspace_bytes(self._handle)), int(lib.cvvdp_video_gradient_wrt_scratch_bytes(self._handle, _capi.WRT[wrt]))
            return (f"predict_with_gradient: the clip needs a workspace of {ws} bytes and a scratch of {sc} bytes as one temporal block, "
                    "which cannot be allocated on this device")

        # one temporal block on the route that keeps every pyramid level
        with self._borrowed(fuse_mode=2, block_frames=n_frames) as no_memory:
            vs = video_source_array(t, r, frames_per_second, dim_order="BCFHW", display_photometry=self.display_photometry)
            with no_memory(text):
                Q, _, _ = self._score_range(vs, 0, n_frames)
            grad, _, call = self._pixel_gradient_entry("cvvdp_video_gradient", "cvvdp_video_gradient_scratch_bytes", sides, dim_order, no_memory(text))
            jod = self.do_pooling_and_jods(Q)       # (reads Q back: after the allocations, which then overlap the forward)
            call()
        return jod.squeeze(), grad

    def _predict_video_with_gradient_blocks(self, sides, dim_order, frames_per_second, block_frames):
        """predict_with_gradient for a clip in temporal blocks: sides = (test, t, reference, r, wrt).  Pass 1 scores all blocks; the
        pooling terms of all frames are added on the device; pass 2 runs the same blocks again, the backward of a block after each."""
        if self._shard is not None:
            raise vq_exception("predict_with_gradient: not available with frame sharding")
        lib = _capi.lib()
        _, t, _, r, wrt = sides
        n_frames = int(t.shape[2])

        def text():
            ws, sc = int(lib.cvvdp_workspace_bytes(self._handle)), int(lib.cvvdp_video_gradient_blocks_wrt_scratch_bytes(self._handle, _capi.WRT[wrt]))
            return (f"predict_with_gradient: blocks of {self.last_block_frames} frames need a workspace of {ws} bytes and a scratch of "
                    f"{sc} bytes, which cannot be allocated on this device")

        # (_pixel_grad_plan: _pick_block_frames counts the backward's scratch when it sizes the blocks itself; 2: the outputs and carry of both sides)
        with self._borrowed(fuse_mode=2, block_frames=None if block_frames == "auto" else min(int(block_frames), n_frames),
                            _pixel_grad_plan=2 if wrt == "both" else True) as no_memory:
            vs = video_source_array(t, r, frames_per_second, dim_order="BCFHW", display_photometry=self.display_photometry)
            with no_memory(text):
                Q, _, _ = self._score_range(vs, 0, n_frames)                   # pass 1: the normal block loop
                self.block_frames = int(self.last_block_frames)                # (pass 2 walks the same blocks, whatever is free by then)
            grad, scratch, after_block = self._pixel_gradient_entry("cvvdp_video_gradient_block", "cvvdp_video_gradient_blocks_scratch_bytes", sides,
                                                                    dim_order, no_memory(text))
            jod = self.do_pooling_and_jods(Q)       # (reads Q back: after the allocations, which then overlap the forward)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if wrt == "test":
                rc = lib.cvvdp_video_gradient_blocks_begin(self._handle, scratch.data_ptr(), scratch.numel(), stream)
            else:
                rc = lib.cvvdp_video_gradient_blocks_begin_wrt(self._handle, _capi.WRT[wrt], scratch.data_ptr(), scratch.numel(), stream)
            _capi.check(self._handle, rc, "cvvdp_video_gradient_blocks_begin")
            if n_frames <= int(self.last_block_frames):
                after_block(stream)                                             # one block: its pyramid is still in the workspace
            else:
                self._block_hook = after_block                                  # pass 2: the same blocks again, the entry after each
                self._score_range(vs, 0, n_frames)
        return jod.squeeze(), grad

    def differentiable_loss(self, test, reference, dim_order="BCFHW", frames_per_second=0, block_frames=None, wrt="test"):
        """10 - JOD of an image or a short clip as a tensor attached to autograd (the reference's loss(): examples/ex_image_reconstruction.py
        runs with this method's name in place of `loss`).  backward() multiplies the gradient predict_with_gradient() stored by the
        upstream gradient, one factor per batch item; the reference receives None, and a reference that requires a gradient is refused.
        Clips: see predict_with_gradient; block_frames (None, an integer or "auto") is handed on to it, so that a clip of any length can
        serve as a loss.  wrt = "reference" or "both" sends the reference its gradient as well (the test then receives one only with
        "both"); with the default a reference that requires a gradient stays refused."""
        if wrt == "test" and torch.is_tensor(reference) and reference.requires_grad:
            raise vq_exception('differentiable_loss: a gradient for the reference is out of scope with wrt = "test" (wrt = "reference" or "both" gives it)')
        predict = lambda: self.predict_with_gradient(test, reference, dim_order, frames_per_second, block_frames=block_frames, wrt=wrt)
        return PixelLoss.apply(test, reference, predict, 10.0, dim_order, wrt)


# the parameters predict_with_parameter_gradient() differentiates in, as the parameter file names them: the band stage's (24 sums of
# cvvdp_param_gradient, in the order of its slots) and the pooling stage's (pool_jod_float64 under autograd)
BAND_PARAMETERS = {"mask_p": (0, 1), "mask_c": (1, 2), "mask_q": (2, 6), "xcm_weights": (6, 22), "d_max": (22, 23), "sensitivity_correction": (23, 24)}
POOLING_PARAMETERS = ("ch_chrom_w", "ch_trans_w", "baseband_weight", "jod_a", "jod_exp", "image_int")
GRADIENT_PARAMETERS = tuple(BAND_PARAMETERS) + POOLING_PARAMETERS


def pool_jod_float64(Q_per_ch, ch_chrom_w, ch_trans_w, baseband_weight, jod_a, jod_exp, image_int, beta_sch, beta_tch, beta_t):
    """do_pooling_and_jods (cvvdp_metric.py:610-658) restated in float64 torch, differentiable in Q_per_ch [B, C, F, L] and in the six
    pooling parameters: lp_norm with safe_pow over bands, channels and (clips: normalised) frames, image_int for one frame, both
    branches of met2jod.  A parameter may carry a leading batch dimension ([B] or [B, 4]): row b then acts on item b alone, which is how
    one autograd call yields d JOD[b] / d parameter for every b.  Runs on CPU tensors as well.  Returns JOD [B], float64."""
    Q = Q_per_ch.double()
    B, C, F, L = Q.shape
    eps = 1e-5
    two = lambda x, n: torch.as_tensor(x, device=Q.device).double().reshape(-1, n)        # [1 or B, n]
    spow = lambda x, p: (x + eps) ** p - eps ** p
    cw, tw, bw = two(ch_chrom_w, 1), two(ch_trans_w, 1), two(baseband_weight, 4)
    n = max(cw.shape[0], tw.shape[0], bw.shape[0])
    one = torch.ones((n, 1), dtype=torch.float64, device=Q.device)
    chw = torch.cat([one, cw.expand(n, 1), cw.expand(n, 1), tw.expand(n, 1)], dim=1)[:, :C].reshape(n, C, 1, 1)
    wb = torch.cat([one[:, :, None].expand(n, C, L - 1), bw.expand(n, 4)[:, :C, None]], dim=2).reshape(n, C, 1, L)
    bs, bt, bf = float(beta_sch), float(beta_tch), float(beta_t)
    Qsc = spow(spow(Q * chw * wb, bs).sum(dim=3), 1.0 / bs)                                # [B, C, F]
    Qtc = spow(spow(Qsc, bt).sum(dim=1), 1.0 / bt)                                        # [B, F]
    if F == 1:
        Qv = Qtc[:, 0] * two(image_int, 1)[:, 0]
    else:
        Qv = spow(spow(Qtc, bf).sum(dim=1) / F, 1.0 / bf)
    a, e, Qt = two(jod_a, 1)[:, 0], two(jod_exp, 1)[:, 0], 0.1
    lin = 10.0 - a * Qt ** (e - 1.0) * Qv
    pw = 10.0 - a * torch.clamp(Qv, min=Qt) ** e
    return torch.where(Qv <= Qt, lin, pw)


class _ParamJod(torch.autograd.Function):
    """JOD with the gradient of cvvdp.predict_with_parameter_gradient in the tensors of P (cvvdp.differentiable_jod)."""

    @staticmethod
    def forward(ctx, metric, test, reference, dim_order, frames_per_second, names, *tensors):
        jod, grads = metric.predict_with_parameter_gradient(test, reference, dim_order, frames_per_second)
        ctx.names = names
        ctx.shapes = [tuple(t.shape) for t in tensors]
        ctx.targets = [(t.device, t.dtype) for t in tensors]
        ctx.save_for_backward(*[grads[n] for n in names])
        return jod

    @staticmethod
    def backward(ctx, upstream):
        out = []
        for g, shape, (dev, dt) in zip(ctx.saved_tensors, ctx.shapes, ctx.targets):
            up = upstream.reshape(-1).to(g.dtype).reshape((-1,) + (1,) * (g.dim() - 1))      # one factor per batch item
            out.append((up * g).sum(dim=0).reshape(shape).to(dev, dt))
        return (None,) * 6 + tuple(out)


class cvvdp_parameter_gradient:
    @staticmethod
    def _gradient_names(names):
        names = GRADIENT_PARAMETERS if names is None else tuple(names)
        for n in names:
            if n not in GRADIENT_PARAMETERS:
                raise vq_exception(f"unknown parameter '{n}': the parameter gradient exists for {', '.join(GRADIENT_PARAMETERS)}")
        return names

    def parameter_tensors(self, names=None):
        """name -> float32 leaf tensor (requires_grad) on the metric's device with the parameter's current value as the parameter file
        stores it (mask_c and d_max as exponents of 10, xcm_weights as exponents of 2, sensitivity_correction in dB): what
        differentiable_jod() takes and an optimiser steps.  names: a subset of cvvdp_metric.GRADIENT_PARAMETERS (None: all twelve)."""
        dev = self._param_device()
        return {n: torch.tensor(self.parameters[n], dtype=torch.float32, device=dev).requires_grad_(True) for n in self._gradient_names(names)}

    def _parameter_gradient_refusals(self, what, vs=None):
        if self.do_heatmap:
            raise vq_exception(f"{what}: not available with a heat map")
        if self.dump_channels is not None:
            raise vq_exception(f"{what}: not available with dump_channels")
        if getattr(self, "_feature_out", None) is not None:
            raise vq_exception(f"{what}: not available with extract_features")
        if self._shard is not None:
            raise vq_exception(f"{what}: not available with frame sharding")
        if vs is not None and hasattr(vs, "set_temporal_filters"):
            raise vq_exception(f"{what}: sources that filter in time themselves (--temp-resample) are out of scope")
        if isinstance(vs, video_source_array) and vs.raw_arrays()[0].shape[1] != 3:
            raise vq_exception(f"{what}: 1-channel content is out of scope, the content must have three colour channels")

    def predict_with_parameter_gradient(self, test, reference, dim_order="BCFHW", frames_per_second=0):
        """(jod, grads) of an image or a clip: grads[name] = d jod[b] / d parameter `name`, float32 on the device, shape
        [B, *shape of the parameter], for the twelve parameters of cvvdp_metric.GRADIENT_PARAMETERS as the parameter file stores them.
        Accepts what predict() accepts with three colour channels; see predict_video_source_with_parameter_gradient."""
        vs = video_source_array(test, reference, frames_per_second, dim_order=dim_order, display_photometry=self.display_photometry)
        return self.predict_video_source_with_parameter_gradient(vs)

    def predict_video_source_with_parameter_gradient(self, vid_source):
        """(jod, grads) of any source predict_video_source() scores block by block (arrays of every dtype, .yuv and image files, every
        display, both paddings, clips of any length).  `jod` is do_pooling_and_jods of the scored Q_per_ch: predict() with fuse_mode = 2,
        bit for bit (the call sets fuse_mode = 2 for itself and restores it).  The pooling parameters' gradients and dJOD/dQ_per_ch come
        from pool_jod_float64 under autograd; the band parameters' from cvvdp_param_gradient (csrc/grad_param.hip) after every block.
        Pooling over frames couples the frames, so a clip of several blocks is walked twice (a file source is read twice); an image or a
        clip of one block is scored once.  Entries that cannot act are exactly 0 (images: ch_trans_w, mask_q[3], baseband_weight[3],
        xcm_weights[4 k + c] with k = 3 or c = 3; clips: image_int).  Heat maps, dump_channels, extract_features, frame sharding,
        1-channel content and sources that filter in time themselves are refused with a vq_exception."""
        what = "predict_with_parameter_gradient"
        inner = getattr(vid_source, "vs", None)             # (as predict_video_source)
        if isinstance(inner, video_source):
            vid_source = inner
        self._parameter_gradient_refusals(what, vid_source)
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
        src_dm = getattr(vid_source, "dm_photometry", None)
        swap = src_dm is not None and src_dm is not self.display_photometry and self._is_raw_source(vid_source)
        prev_dm = self.display_photometry
        if swap:
            self.display_photometry = src_dm
            self._make_handle()
        try:
            with self._borrowed(fuse_mode=2, _param_grad_plan=True):
                return self._parameter_gradient(vid_source, what)
        finally:
            if swap:
                self.display_photometry = prev_dm
                self._make_handle()

    def _parameter_gradient(self, vs, what):
        lib = _capi.lib()
        _h, _w, n_frames = vs.get_video_size()
        Q, _, _ = self._score_range(vs, 0, n_frames)                       # pass 1: the normal block loop
        if self._route_channels != 3:
            raise vq_exception(f"{what}: 1-channel content is out of scope, the content must have three colour channels")
        jod = self.do_pooling_and_jods(Q)
        self._param_grad_Q = Q                                             # the Q_per_ch that was scored (calibration's rescoring mode pools it again)
        B = int(Q.shape[0])
        p = self.parameters
        # the pooling stage in float64 on the host (a few thousand numbers): its parameters' gradients and dJOD/dQ_per_ch in one autograd call
        Qh = Q.detach().to("cpu", torch.float64).requires_grad_(True)
        leaves = {n: torch.tensor(p[n], dtype=torch.float64).reshape(1, -1).repeat(B, 1).requires_grad_(True) for n in POOLING_PARAMETERS}
        with torch.enable_grad():
            j64 = pool_jod_float64(Qh, beta_sch=p["beta_sch"], beta_tch=p["beta_tch"], beta_t=p["beta_t"], **leaves)
            got = torch.autograd.grad(j64.sum(), [Qh] + [leaves[n] for n in POOLING_PARAMETERS], allow_unused=True)
        dq = got[0].to(torch.float32).to(self.device).contiguous()
        grads = {}
        for n, g in zip(POOLING_PARAMETERS, got[1:]):
            g = torch.zeros_like(leaves[n]) if g is None else g
            grads[n] = g.to(torch.float32).reshape((B,) + tuple(np.shape(p[n]))).to(self.device)
        # the band stage: 24 sums per batch item, added block by block
        acc = torch.zeros((B, _capi.PARAM_GRAD_COUNT), dtype=torch.float64, device=self.device)
        try:
            scratch = torch.empty(max(int(lib.cvvdp_param_gradient_scratch_bytes(self._handle)), 16), dtype=torch.uint8, device=self.device)
        except torch.cuda.OutOfMemoryError:
            raise vq_exception(f"{what}: the scratch of {int(lib.cvvdp_param_gradient_scratch_bytes(self._handle))} bytes cannot be allocated on this device") from None

        def after_block(stream):
            rc = lib.cvvdp_param_gradient(self._handle, dq.data_ptr(), acc.data_ptr(), scratch.data_ptr(), scratch.numel(), stream)
            _capi.check(self._handle, rc, "cvvdp_param_gradient")

        if n_frames == 1 or n_frames <= int(self.last_block_frames):
            after_block(torch.cuda.current_stream(self.device).cuda_stream)     # one block: its pyramid is still in the workspace
        else:
            self._block_hook = after_block                                      # pass 2: the same blocks again, the entry after each
            self._score_range(vs, 0, n_frames)
        band = acc.to(torch.float32)
        for n, (a, b) in BAND_PARAMETERS.items():
            grads[n] = band[:, a:b].reshape((B,) + tuple(np.shape(p[n]))).contiguous()
        del scratch        # stream-ordered: the caching allocator may hand it out again once the kernels are queued
        return jod.squeeze(), {n: grads[n] for n in GRADIENT_PARAMETERS}

    def differentiable_jod(self, test, reference, P, dim_order="BCFHW", frames_per_second=0):
        """JOD attached to autograd in the parameter tensors of P (name -> tensor, as parameter_tensors() makes them): the values of P are
        installed in the metric if they differ from its own (all or nothing, through the path every parameter assignment takes; names
        absent from P keep their values), the content is scored, and backward() adds upstream[b] x d jod[b] / d parameter, summed over
        b, to every tensor of P.  test and reference must not require a gradient (differentiable_loss() is the pixel side)."""
        for a in (test, reference):
            if torch.is_tensor(a) and a.requires_grad:
                raise vq_exception("differentiable_jod: a gradient for test or reference is out of scope here (differentiable_loss() gives the pixel gradient)")
        names = self._gradient_names(list(P.keys()))
        self._parameter_gradient_refusals("differentiable_jod")
        q = dict(self.parameters)
        changed = False
        for n in names:
            v = self._parameter_value(n, P[n], q[n])
            if not np.array_equal(np.asarray(v, dtype=f32), np.asarray(q[n], dtype=f32)):
                q[n], changed = v, True
        if changed:
            self._set_parameters(q)
        return _ParamJod.apply(self, test, reference, dim_order, frames_per_second, names, *[P[n] for n in names])
