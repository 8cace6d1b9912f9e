"""Host plumbing every metric class shares: the tensor strides the C ABI takes, and the resized unpack of a .yuv pair."""
import ctypes

import torch

from . import _capi


def batch_strides(t, r, B=None):
    """Element strides of a test / reference BCFHW pair as two int64[5]; a batch-1 side next to a batch of B (None: the larger of
    the two batch sizes) is broadcast with batch stride 0 (video_source.py:247-252)."""
    if B is None:
        B = max(t.shape[0], r.shape[0])
    out = []
    for x in (t, r):
        s = list(x.stride())
        if x.shape[0] == 1 and B > 1:
            s[0] = 0
        out.append((ctypes.c_int64 * 5)(*s))
    return out[0], out[1]


def yuv_block_resized(handle, device, vs, a, b, height, width):
    """Frames [a,b) of a .yuv pair with full_screen_resize: (test, reference) as [1,3,n,H,W] fp32 R'G'B' blocks at the display's
    resolution (cvvdp_unpack_yuv_resized: unpack + torch.nn.functional.interpolate semantics + clip, video_source_yuv.py:333-336)."""
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    out = []
    for side in range(2):
        codes, fmt, sw, sh = vs.get_raw_yuv_side(side, a, b, device)
        # a side that already has the target size is not interpolated by the reference: nearest at scale 1 is the identity
        mode = _capi.RESIZE_MODES[vs.full_screen_resize] if (sw, sh) != (width, height) else _capi.RESIZE_MODES["nearest"]
        tmp = torch.empty(3 * (b - a) * sh * sw, dtype=torch.float32, device=device)
        rgb = torch.empty((1, 3, b - a, height, width), dtype=torch.float32, device=device)
        rc = _capi.lib().cvvdp_unpack_yuv_resized(handle, codes.data_ptr(), ctypes.byref(fmt), side, sw, sh, b - a, width, height, mode,
                                                  tmp.data_ptr(), rgb.data_ptr(), stream)
        _capi.check(handle, rc, "cvvdp_unpack_yuv_resized")
        out.append(rgb)
        del tmp, codes            # stream-ordered: the caching allocator may reuse them once the kernels are queued
    return out[0], out[1]
