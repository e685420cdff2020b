"""CPU: the numpy model of the windowed SSIM (tests/frame_ssim_model.py) against literals derived by hand from the definition in
include/hopperflow.h, so that what the GPU tests demand equality with is pinned by something other than the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_ssim_model as fsm  # noqa: E402

PEAKS = (255, 65535, 1023)


def _luma(a, b, peak):
    dt = np.uint8 if peak == 255 else np.uint16
    return fsm.plane_ssim(np.asarray(a, dt), np.asarray(b, dt), peak)


def test_constants():
    assert fsm.constants(255) == (416, 235963)            # FFmpeg's 8-bit constants
    assert fsm.constants(65535) == (27486952, 15585101693)
    assert fsm.constants(1023) == (6698, 3797644)


def test_equal_frames_lose_nothing():
    rng = np.random.default_rng(0)
    for peak in PEAKS:
        a = rng.integers(0, peak + 1, (16, 16))
        assert _luma(a, a, peak) == {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 9}


@pytest.mark.parametrize("peak,total,worst", [(255, 38654645292, 4294960588), (65535, 38654645265, 4294960585), (1023, 38654645265, 4294960585)])
def test_zero_against_peak(peak, total, worst):
    """S1 = 0, S2 = 64 peak, SS = 64 peak^2, S12 = 0:  A = c1, B = c2, C = 4096 peak^2 + c1, D = c2 -- ssim = c1 / C, about 1.56e-6."""
    a, b = np.zeros((16, 16), np.int64), np.full((16, 16), peak)
    assert _luma(a, b, peak) == {"sum_loss_q32": total, "max_loss_q32": worst, "count": 9}
    assert total == 9 * worst
    c1, _ = fsm.constants(peak)
    assert worst == (1 << 32) - round(c1 / (4096 * peak * peak + c1) * 2 ** 32)


@pytest.mark.parametrize("peak,total,worst", [(255, 77172670836, 8574741204), (65535, 77172670998, 8574741222), (1023, 77172671016, 8574741224)])
def test_anti_checkerboard_is_worse_than_unrelated(peak, total, worst):
    """a = peak ((x + y) & 1) against b = peak - a: full negative covariance, ssim about -0.9965, a loss above 2^32."""
    y, x = np.mgrid[0:16, 0:16]
    a = peak * ((x + y) & 1)
    assert _luma(a, peak - a, peak) == {"sum_loss_q32": total, "max_loss_q32": worst, "count": 9}
    assert worst > 1 << 32 and 1.0 - worst / 2 ** 32 == pytest.approx(-0.9965, abs=1e-4)


def test_counts_of_small_planes_and_unused_remainders():
    rng = np.random.default_rng(1)
    for h, w in ((4, 4), (4, 8), (7, 64), (64, 7)):
        assert _luma(rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w)), 255) == {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 0}
    a, b = rng.integers(0, 256, (38, 70)), rng.integers(0, 256, (38, 70))
    want = _luma(a, b, 255)
    assert want["count"] == 16 * 8 and want["sum_loss_q32"] > 0
    b2 = b.copy()
    b2[36:, :] ^= 255; b2[:, 68:] ^= 255                  # the h & 3 rows and w & 3 columns are not used
    assert _luma(a, b2, 255) == want
    assert _luma(a[:8, :8], b[:8, :8], 255)["count"] == 1


def test_frames_split_into_planes_and_default_peaks():
    """A frame's three planes through split_planes; peak None is 255, 65535 (P010) or 1023 (planar 16 bit)."""
    rng = np.random.default_rng(2)
    H, W, S = 16, 32, 40
    n = H * S + (H // 2) * S
    a, b = rng.integers(0, 1024, n, dtype=np.uint16), rng.integers(0, 1024, n, dtype=np.uint16)
    semi, planar = fsm.frame_ssim(a, b, H, W, S, S), fsm.frame_ssim(a, b, H, W, S, S, planar=True)
    assert [semi[p]["count"] for p in "YUV"] == [7 * 3, 3, 3] == [planar[p]["count"] for p in "YUV"]
    assert semi == fsm.frame_ssim(a, b, H, W, S, S, peak=65535) and planar == fsm.frame_ssim(a, b, H, W, S, S, planar=True, peak=1023)
    assert semi["Y"] != planar["Y"]                       # (the constants differ)
    a8 = (a >> 2).astype(np.uint8)
    assert fsm.frame_ssim(a8, a8, H, W, S, S)["U"] == {"sum_loss_q32": 0, "max_loss_q32": 0, "count": 3}
    d = fsm.derived(semi["Y"])
    assert d["ssim"] == 1.0 - semi["Y"]["sum_loss_q32"] / 2 ** 32 / 21 and d["min_ssim"] <= d["ssim"]
    assert fsm.derived({"sum_loss_q32": 0, "max_loss_q32": 0, "count": 0}) == {"ssim": None, "min_ssim": None}


def test_terms_stay_below_2_to_53_at_16_bits():
    """Every window term converts to double exactly: checked on the two 16-bit extremes."""
    y, x = np.mgrid[0:16, 0:16]
    chk = 65535 * ((x + y) & 1)
    for a, b in ((np.zeros((16, 16), np.int64), np.full((16, 16), 65535)), (chk, 65535 - chk), (np.full((16, 16), 65535), np.full((16, 16), 65535))):
        for t in fsm.window_terms(a.astype(np.uint16), b.astype(np.uint16), 65535):
            assert int(np.abs(t).max()) < 1 << 53
