"""The shapes tests/test_batch_planar_gpu.py runs the batched planar re-layout launches on (HF_FLAG_BATCH_PLANAR_IN / _OUT,
csrc/hf_planar.hip planar_in_batch_kernel / planar_out_batch_kernel), and a host model of which access path each plane of a launch
takes -- the formulas of launch_planar / planar_shape_add, restated: tests/test_batch_planar.py holds the list to the model, so that it
cannot silently lose a path.

A work item is 16 bytes of the semi-planar frame: 16 / bpp luma elements, or 8 U + 8 V elements.  Per plane a launch is
    wide     16-byte accesses (8-byte U / V at 8 bit): every base of every frame of the launch allows them, and the item is whole
    element  element by element: some base rules the wide access out -- or the last item of the plane is ragged
so a plane's path is (wide or element, whole items only or a ragged last item)."""
from collections import namedtuple

WIDE, ELEMENT = "wide", "element"
WHOLE, RAGGED = "whole", "ragged"

# what the kernels can reach at all: a wide chroma plane is never ragged (its V base is aligned only if n_c is a multiple of 8)
LUMA_PATHS = {(WIDE, WHOLE), (WIDE, RAGGED), (ELEMENT, WHOLE), (ELEMENT, RAGGED)}
CHROMA_PATHS = {(WIDE, WHOLE), (ELEMENT, WHOLE), (ELEMENT, RAGGED)}


def plane_paths(H, S, bpp, frames):
    """((luma path), (chroma path)) of ONE launch over `frames` = [(planar base, semi-planar base)] (addresses modulo anything >= 16):
    frames of H rows, stride S elements of bpp bytes."""
    el = 16 // bpp
    n_y, n_c = H * S, (H // 2) * (S // 2)
    vec_y = vec_c = True
    for planar, semi in frames:       # one flag pair for the whole launch: the AND over all frames
        vec_y = vec_y and planar % 16 == 0 and semi % 16 == 0
        vec_c = (vec_c and (planar + n_y * bpp) % (8 * bpp) == 0 and (planar + (n_y + n_c) * bpp) % (8 * bpp) == 0
                 and (semi + n_y * bpp) % 16 == 0)
    return ((WIDE if vec_y else ELEMENT, RAGGED if n_y % el else WHOLE), (WIDE if vec_c else ELEMENT, RAGGED if n_c % 8 else WHOLE))


# One batch of the GPU tests as far as the two launches see it: both sides' strides, and the byte offsets of each member's planar
# input / planar outputs into its (256-byte aligned) allocation.  The library's own frames (ring slots, stages) are allocations.
Case = namedtuple("Case", "name H W S_in S_out hdr in_offsets out_offsets")

KERNEL_CASES = [
    Case("basic-sdr", 180, 320, 320, 320, 0, (0, 0), (0, 0)),
    Case("basic-hdr", 180, 320, 320, 320, 1, (0, 0), (0, 0)),
    Case("ragged-sdr", 180, 320, 336, 330, 0, (0, 0), (0, 0)),
    Case("ragged-hdr", 180, 320, 336, 330, 1, (0, 0), (0, 0)),
    Case("ragged-in-sdr", 180, 320, 330, 336, 0, (0, 0), (0, 0)),   # the ragged side on the way in at 8 bit
    Case("offset-sdr", 180, 320, 336, 330, 0, (0, 8), (0, 8)),      # one member's frames 8 bytes into a larger buffer: the whole launch
    Case("offset-hdr", 180, 320, 336, 330, 1, (0, 8), (0, 8)),      # goes element by element
    Case("mid-hdr", 722, 1282, 1290, 1296, 1, (0, 0), (0, 0)),
    Case("full-table", 64, 96, 96, 96, 0, (0,) * 32, (0,) * 32),
    Case("deferred-2160p", 2160, 3840, 3840, 3840, 1, (0, 0, 0), (0, 0, 0)),
]


def case(name):
    return next(c for c in KERNEL_CASES if c.name == name)


def case_paths(c):
    """{"in": (luma, chroma), "out": (luma, chroma)} of a case's two launches"""
    bpp = 2 if c.hdr else 1
    return {"in": plane_paths(c.H, c.S_in, bpp, [(o, 0) for o in c.in_offsets]),
            "out": plane_paths(c.H, c.S_out, bpp, [(o, 0) for o in c.out_offsets])}
