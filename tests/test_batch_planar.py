"""CPU: planar 4:2:0 frames at a batch's boundary (HF_FLAG_BATCH_PLANAR_IN / HF_FLAG_BATCH_PLANAR_OUT, include/hopperflow.h): the
constants of the ctypes layer against the header, and the access paths the GPU cases of tests/test_batch_planar_gpu.py reach in the two
batched re-layout launches (tests/batch_planar_cases.py: a host model of launch_planar's alignment and tail formulas)."""
import os
import re

import batch_planar_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_flags():
    src = open(os.path.join(ROOT, "include", "hopperflow.h")).read()
    return {name: int(value, 16) for name, value in re.findall(r"^#define (HF_FLAG_[A-Z_0-9]+) (0x[0-9A-Fa-f]+)", src, flags=re.M)}


def test_flag_constants_equal_the_header_and_collide_with_nothing():
    from hopperrender_amd import capi
    flags = header_flags()
    assert flags["HF_FLAG_BATCH_PLANAR_IN"] == 0x20000 == capi.HF_FLAG_BATCH_PLANAR_IN
    assert flags["HF_FLAG_BATCH_PLANAR_OUT"] == 0x40000 == capi.HF_FLAG_BATCH_PLANAR_OUT
    assert len(flags) >= 15 and len(set(flags.values())) == len(flags), "two HF_FLAG_* share a value"
    for name, value in flags.items():
        assert value & (value - 1) == 0, f"{name} is not a single bit"
        assert getattr(capi, name) == value, name
    mirrored = {k: v for k, v in vars(capi).items() if k.startswith("HF_FLAG_")}
    assert len(set(mirrored.values())) == len(mirrored)
    assert "hf_batch_planar" in capi.SIGNATURES


def test_the_path_model_on_hand_worked_shapes():
    W, E, WH, RG = cases.WIDE, cases.ELEMENT, cases.WHOLE, cases.RAGGED
    # 180 x 320 at stride 330: V starts at element 74,250 (not a multiple of 8); 59,400 mod 16 = 8
    assert cases.plane_paths(180, 330, 1, [(0, 0)]) == ((W, RG), (E, RG))
    assert cases.plane_paths(180, 330, 2, [(0, 0)]) == ((W, WH), (E, RG))
    assert cases.plane_paths(180, 336, 1, [(0, 0)]) == ((W, WH), (W, WH))
    # one frame of the launch decides for all; 8 bytes off still suit the 8-byte U / V accesses at 8 bit, not the 16-byte ones at 16 bit
    assert cases.plane_paths(180, 336, 1, [(0, 0), (8, 0)]) == ((E, WH), (W, WH))
    assert cases.plane_paths(180, 336, 2, [(0, 0), (8, 0)]) == ((E, WH), (E, WH))
    assert cases.plane_paths(180, 336, 2, [(0, 0), (0, 8)]) == ((E, WH), (E, WH))
    assert cases.plane_paths(722, 1290, 2, [(0, 0)]) == ((W, RG), (E, RG))
    assert cases.plane_paths(722, 1296, 2, [(0, 0)]) == ((W, WH), (W, WH))


def test_a_wide_chroma_plane_is_never_ragged():
    """Why CHROMA_PATHS has three members: the V base is aligned for the wide access only where n_c is a multiple of 8."""
    for bpp in (1, 2):
        for H in (2, 4, 6, 10, 64, 180):
            for S in range(2, 200, 2):
                for off in (0, 2, 4, 8, 16):
                    _, chroma = cases.plane_paths(H, S, bpp, [(off, 0)])
                    assert chroma in cases.CHROMA_PATHS


def test_the_gpu_cases_reach_every_path_of_both_launches():
    reached = {"luma": set(), "chroma": set()}
    per_launch = {(d, hdr): {"luma": set(), "chroma": set()} for d in ("in", "out") for hdr in (0, 1)}
    for c in cases.KERNEL_CASES:
        assert c.S_in % 2 == 0 and c.S_out % 2 == 0 and len(c.in_offsets) == len(c.out_offsets) <= 32
        for d, (luma, chroma) in cases.case_paths(c).items():
            assert luma in cases.LUMA_PATHS and chroma in cases.CHROMA_PATHS
            for where in (reached, per_launch[d, c.hdr]):
                where["luma"].add(luma)
                where["chroma"].add(chroma)
    assert reached["luma"] == cases.LUMA_PATHS, cases.LUMA_PATHS - reached["luma"]
    assert reached["chroma"] == cases.CHROMA_PATHS, cases.CHROMA_PATHS - reached["chroma"]
    # each of the four kernels (in / out, 8 / 16 bit) runs wide and element by element, with whole items and with a ragged tail
    for key, got in per_launch.items():
        assert {p[0] for p in got["luma"]} == {cases.WIDE, cases.ELEMENT}, key
        assert {p[0] for p in got["chroma"]} == {cases.WIDE, cases.ELEMENT}, key
        assert {p[1] for p in got["luma"] | got["chroma"]} == {cases.WHOLE, cases.RAGGED}, key
    # the cases the shapes were chosen for
    assert cases.case_paths(cases.case("ragged-sdr"))["out"] == ((cases.WIDE, cases.RAGGED), (cases.ELEMENT, cases.RAGGED))
    assert cases.case_paths(cases.case("ragged-sdr"))["in"] == ((cases.WIDE, cases.WHOLE), (cases.WIDE, cases.WHOLE))
    assert cases.case_paths(cases.case("offset-hdr"))["out"][0] == (cases.ELEMENT, cases.WHOLE)
    assert cases.case_paths(cases.case("mid-hdr"))["in"] == ((cases.WIDE, cases.RAGGED), (cases.ELEMENT, cases.RAGGED))
