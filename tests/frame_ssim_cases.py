"""What tests/test_frame_ssim_gpu.py and its debug-bounds child share: host frames on the device, and the layout case (ragged 70 x 38 with
strides, offsets and random padding) against the numpy model of tests/frame_ssim_model.py.  Not a test module itself."""
import ctypes as C

import numpy as np

from frame_ssim_model import derived, frame_ssim

RAGGED = (38, 70, ((70, 70), (74, 80), (80, 80), (80, 74), (80, 70)))   # H, W, strides of side a / b: w & 3 = h & 3 = 2, chroma 35 x 19


def n_el(H, S):
    return H * S + (H // 2) * S


def random_frame(rng, hdr, H, S, top=None):
    return rng.integers(0, (top or (65535 if hdr else 255)) + 1, size=n_el(H, S), dtype=np.uint16 if hdr else np.uint8)


def ints(got):
    """the integers of a result of calc.frameSsim* (the derived floats dropped)"""
    return {p: {k: got[p][k] for k in ("sum_loss_q32", "max_loss_q32", "count")} for p in "YUV"}


def check_floats(got):
    for p in "YUV":
        assert {k: got[p][k] for k in ("ssim", "min_ssim")} == derived(got[p]), p
        assert all(type(got[p][k]) is int for k in ("sum_loss_q32", "max_loss_q32", "count"))


class Dev:
    """Host frames on the device, optionally `off` elements into their allocation (an unaligned base)."""

    def __init__(self):
        self.bufs = []

    def put(self, a, off=0):
        from hopperrender_amd import capi
        from hopperrender_amd.calc import DeviceBuffer
        a = np.ascontiguousarray(a)
        b = DeviceBuffer(a.nbytes + 64)
        self.bufs.append(b)
        p = b.ptr + off * a.itemsize
        capi.check(capi.load().hf_memcpy_h2d(0, C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return p

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def run_layout_case(c, dev, hdr, planar, H, W, strides, offsets=(0, 2), seed=0):
    """Three pairs per launch and the one-pair call on a context c of H x W, for every stride pair and base offset; every element random,
    the padding and the unused remainder included; every integer equal to the model.  Returns the model's results of the last strides."""
    rng = np.random.default_rng(seed)
    want = None
    for sa, sb in strides:
        fa = [random_frame(rng, hdr, H, sa) for _ in range(3)]
        fb = [random_frame(rng, hdr, H, sb) for _ in range(3)]
        fb[2].reshape(-1, sb)[:, :W] = fa[2].reshape(-1, sa)[:, :W]   # pair 2: luma (semi-planar: chroma too) close to its partner's
        fb[2][::7] ^= 1
        want = [frame_ssim(a, b, H, W, sa, sb, planar) for a, b in zip(fa, fb)]
        for off in offsets:   # all bases aligned (wide accesses where the pitches allow them), then all 2 elements in (element by element)
            pa, pb = [dev.put(a, off) for a in fa], [dev.put(b, off) for b in fb]
            c.frameSsimEnqueue(pa, pb, 5, sa, sb, planar)
            got = c.frameSsimRead(5, 3)
            assert [ints(g) for g in got] == want, (hdr, planar, H, W, sa, sb, off)
            one = c.frameSsim(pa[0], pb[0], sa, sb, planar)
            assert ints(one) == want[0], (hdr, planar, H, W, sa, sb, off)
            check_floats(one)
    return want
