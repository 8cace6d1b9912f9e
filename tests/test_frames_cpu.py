"""_frames.batch_strides: the strides every metric hands to the C ABI for a test / reference pair.  CPU only."""
import pytest
import torch

from colorvideovdp_amd import _frames
from colorvideovdp_amd.cvvdp_metric import cvvdp
from colorvideovdp_amd.psnr_metric import psnr_rgb


@pytest.mark.parametrize("B", [1, 3])
def test_a_single_item_next_to_a_batch_is_broadcast(B):
    one = torch.zeros((1, 3, 4, 6, 5))
    many = torch.zeros((B, 3, 9, 6, 7))[:, :, 2:6, :, 1:6]                    # (a view: the strides are not those of its shape)
    for t, r in ((one, many), (many, one), (many, many)):
        for st, sr in (_frames.batch_strides(t, r), _frames.batch_strides(t, r, B), cvvdp._strides(t, r), psnr_rgb._strides(t, r, B)):
            for x, s in ((t, st), (r, sr)):
                want = list(x.stride())
                if x is one and B > 1:
                    want[0] = 0
                assert list(s) == want and len(s) == 5
    # the batch size of the call decides where it is given: a batch-1 pair is broadcast on both sides inside a batch, not on its own
    for st, sr in (_frames.batch_strides(one, one, 3), psnr_rgb._strides(one, one, 3)):
        assert st[0] == 0 and sr[0] == 0 and list(st)[1:] == list(one.stride())[1:] == list(sr)[1:]
    for st, sr in (_frames.batch_strides(one, one), cvvdp._strides(one, one), _frames.batch_strides(one, one, 1)):
        assert list(st) == list(one.stride()) == list(sr)
