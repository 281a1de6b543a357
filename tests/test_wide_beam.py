"""Wide beams without a GPU: the device decoder's beam limit."""
import pytest

from textsummarization_on_flink_amd.config import HParams


def test_beam_17_is_refused_at_construction():
    """beam_size > 16 raises a ValueError that names the limit, before anything is allocated (no
    vocabulary, no parameters and no device are touched)."""
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    assert DeviceBeamDecoder.MAX_BEAM == 16
    with pytest.raises(ValueError, match=r"beam_size 17 exceeds 16"):
        DeviceBeamDecoder(HParams(beam_size=17), None, None, n_articles=2, T=8)
    with pytest.raises(ValueError, match=r"exceeds 16"):
        DeviceBeamDecoder(HParams(beam_size=64, block_ngram_repeat=3), None, None, n_articles=2, T=8, wide_beam=True)
