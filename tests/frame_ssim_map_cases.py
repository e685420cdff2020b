"""What tests/test_frame_ssim_map_gpu.py and its debug-bounds child share: the map of a launch out of a prefilled, guarded buffer, and
the layout case (ragged 70 x 38 with strides, offsets and random padding, three pairs a launch) against the numpy model of
tests/frame_ssim_map_model.py.  Not a test module itself."""
import numpy as np

from frame_ssim_cases import ints, random_frame
from frame_ssim_map_model import frame_ssim_map, map_shape, totals

GUARD = 64


def prefilled(nbytes):
    """a device buffer of nbytes + 64 guard bytes, all 0xFF: an entry the launch did not write, or a write past the end, shows"""
    from hopperrender_amd.calc import DeviceBuffer
    buf = DeviceBuffer(nbytes + GUARD)
    buf.upload(np.full(nbytes + GUARD, 0xFF, np.uint8))
    return buf


def maps(c, pa, pb, tile, sa=0, sb=0, planar=False, peak=0):
    """the SSIM maps of pairs (pa[i], pb[i]) from a prefilled buffer, [n][3][th][tw]"""
    from hopperrender_amd.calc import frame_ssim_maps
    tw, th, nbytes = c.frameSsimMapShape(tile)
    n = len(pa)
    buf = prefilled(n * nbytes)
    try:
        c.frameSsimMapEnqueue(pa, pb, tile, buf.ptr, sa, sb, planar, peak)
        c.sync()
        raw = buf.download(np.uint8)
    finally:
        buf.free()
    assert (raw[n * nbytes:] == 0xFF).all(), "bytes behind the last map were written"
    return frame_ssim_maps(raw, n, tw, th).copy()


def same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ; first at [plane, ty, tx] = {i}: device {got[i]}, model {want[i]}")


def run_map_layout_case(c, dev, hdr, planar, H, W, strides, tile, offsets=(0, 2), seed=0):
    """Three pairs per launch on a context c of H x W, for every stride pair and base offset; every element random, the padding and the
    unused remainder included; every entry equal to the model, and the first pair's totals equal to the device's own hf_frame_ssim.
    Returns the model's maps of the last strides."""
    rng = np.random.default_rng(seed)
    th, tw = map_shape(H, W, tile)
    assert c.frameSsimMapShape(tile) == (tw, th, 72 * tw * th)
    want = None
    for sa, sb in strides:
        fa = [random_frame(rng, hdr, H, sa) for _ in range(3)]
        fb = [random_frame(rng, hdr, H, sb) for _ in range(3)]
        fb[2].reshape(-1, sb)[:, :W] = fa[2].reshape(-1, sa)[:, :W]   # pair 2: luma (semi-planar: chroma too) close to its partner's
        fb[2][::7] ^= 1
        want = [frame_ssim_map(a, b, H, W, tile, sa, sb, planar) for a, b in zip(fa, fb)]
        for off in offsets:   # all bases aligned (wide accesses where the pitches allow them), then all 2 elements in (element by element)
            pa, pb = [dev.put(a, off) for a in fa], [dev.put(b, off) for b in fb]
            got = maps(c, pa, pb, tile, sa, sb, planar)
            for i in range(3):
                same(got[i], want[i], (hdr, planar, H, W, tile, sa, sb, off, i))
            assert totals(got[0]) == ints(c.frameSsim(pa[0], pb[0], sa, sb, planar)), (hdr, planar, H, W, tile, sa, sb, off)
    return want
