"""host_setup.plan_blocks: the temporal blocks of a frame range, their fetched runs and the window positions before each block
(temporal padding, shard halos, the DKL tail of the previous block).  CPU only."""
import pytest

from colorvideovdp_amd import host_setup as hs


def _cases():
    for n_total in (2, 3, 5, 9, 20):
        for first in range(n_total):
            for count in range(1, n_total - first + 1):
                for nb in (1, 2, 4, 16):
                    for head in sorted({h for h in (1, 2, nb) if h <= nb}):
                        yield n_total, first, count, nb, head


def _check(first, count, nb, head, fl, raw_halo, n_total, padding):
    blocks = hs.plan_blocks(first, count, nb, head, fl, raw_halo, n_total, padding)
    at = first
    for i, (ff, n, lo, hi, hist) in enumerate(blocks):
        assert ff == at and n >= 1                                            # the blocks tile the range in order
        assert n == min(head if i == 0 else nb, first + count - ff)
        assert 0 <= lo <= ff and ff + n <= hi <= n_total
        assert len(hist) == fl - 1
        if i == 0 or raw_halo:
            for k, h in enumerate(hist):
                j = ff - (fl - 1) + k
                want = j if j >= 0 else (0 if padding == "replicate" else hs.symmetric_frame_index(j, n_total))
                assert h >= 0 and lo + h < hi and lo + h == want
        else:
            assert hist == [-1 - k for k in range(fl - 1)]
        at += n
    assert at == first + count


@pytest.mark.parametrize("padding", ["replicate", "symmetric"])
@pytest.mark.parametrize("raw_halo", [0, 1])
@pytest.mark.parametrize("fl", [1, 3, 7, 9, 17])
def test_blocks_tile_the_range_and_find_their_window(fl, raw_halo, padding):
    n = 0
    for n_total, first, count, nb, head in _cases():
        _check(first, count, nb, head, fl, raw_halo, n_total, padding)
        n += 1
    assert n == 2511                    # x 5 filter lengths x 2 x 2 = 50,220 cases


def test_unknown_padding_is_refused():
    with pytest.raises(RuntimeError, match='^Unknown padding method "circular"$'):
        hs.plan_blocks(0, 4, 2, 2, 3, 0, 4, "circular")
