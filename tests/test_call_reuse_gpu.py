"""What a cvvdp metric keeps from one call to the next: the page-locked heat-map buffer, the ring of staging buffers of a host sink,
the clip description.  Losing any of them changes no score, only the time of every call after the first.  Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clips():
    g = torch.Generator().manual_seed(5)
    r = torch.randint(0, 256, (1, 3, 6, 48, 64), generator=g, dtype=torch.uint8)
    out = []
    for _ in range(2):
        t = (r.to(torch.int16) + torch.randint(-20, 21, r.shape, generator=g, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
        out.append((t.cuda(), r.cuda()))
    return out


def _heatmap(m, clip):
    return m.predict(clip[0], clip[1], dim_order="BCFHW", frames_per_second=30)[1]["heatmap"]


def test_whole_clip_heatmap_buffer_is_handed_out_again_only_when_nobody_holds_it(clips):
    import colorvideovdp_amd as cv
    from colorvideovdp_amd import cvvdp_metric
    m = cv.cvvdp(heatmap="threshold")
    hm = _heatmap(m, clips[0])
    assert tuple(hm.shape) == (1, 3, 6, 48, 64) and hm.dtype == torch.float16
    first = hm.data_ptr()
    del hm
    hm = _heatmap(m, clips[1])
    if cvvdp_metric._storage_is_unshared(torch.empty(4)):
        assert hm.data_ptr() == first               # page-locked once, filled twice
    kept = hm.clone()
    other = _heatmap(m, clips[0])                   # `hm` is still held: its frames must not be overwritten
    assert other.data_ptr() != hm.data_ptr()
    assert torch.equal(hm, kept) and not torch.equal(other, kept)


def test_host_sink_calls_share_one_ring_of_staging_buffers(clips):
    import colorvideovdp_amd as cv
    m = cv.cvvdp(heatmap="threshold", block_frames=2)             # three pieces per call, a ring of four
    seen = []
    for clip in clips:
        ptrs = []
        m.predict_video_source(cv.video_source_array(clip[0], clip[1], 30, dim_order="BCFHW", display_photometry=m.display_photometry),
                               heatmap_sink=lambda f, x: ptrs.append((f, x.data_ptr(), tuple(x.shape), x.is_pinned())))
        seen.append(ptrs)
    assert [p[0] for p in seen[0]] == [0, 2, 4] and all(p[2] == (1, 3, 2, 48, 64) and p[3] for p in seen[0])
    assert len({p[1] for p in seen[0]}) == 3
    assert {p[1] for p in seen[0]} == {p[1] for p in seen[1]}


def test_clip_description_is_made_once_per_shape(clips):
    import colorvideovdp_amd as cv
    m = cv.cvvdp(heatmap="threshold")
    _heatmap(m, clips[0])
    clip = m._clip_cache[1]
    _heatmap(m, clips[1])
    assert m._clip_cache[1] is clip
