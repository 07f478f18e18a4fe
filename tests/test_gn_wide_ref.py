"""The GroupNorm reduce arithmetic on the CPU at 256 < C <= 1024 (the VEC builds' range): the lane geometry of the shapes of
tests/test_groupnorm_wide_gpu.py, and the prediction that the kernels' arithmetic (gn_moments_ref, parameterised in C) meets
that file's per-(sample, group) criterion against float64 on every one of them.  An emulation, not a GPU measurement."""
import pytest

import gn_moments_ref as M
from test_gn_moments_ref import _judge

# (C, G, P, B): the smallest shapes that reach each lane geometry above 256 channels
WIDE_SHAPES = (
    (320, 32, 9, 3),       # CV = 80: three pixel lanes, 16 dead threads
    (384, 32, 16, 3),      # CV = 96: two pixel lanes, 64 dead threads
    (512, 32, 9, 3),       # CV = 128: two pixel lanes, odd P (the second lane sums one pixel fewer)
    (640, 32, 5, 2),       # CV = 160: ONE pixel lane, 96 dead threads
    (1024, 32, 5, 2),      # CV = 256: one pixel lane, every thread live, the limit
    (512, 32, 130, 3),     # more than one sub-chunk: 64 + 64 + 2 pixels, one chunk slot each
)
# the well-conditioned end and |mean| / std = 100 of gn_moments_ref.CONDS
WIDE_CONDS = (M.CONDS[0], M.CONDS[2])
# (C0, C1) of the two-source cases: the decoder concatenations of the 64-wide and the four-level nets, and the limit
WIDE_SPLITS = ((256, 256), (384, 128), (512, 512))


def test_conds_are_the_issues():
    assert WIDE_CONDS == ((0.0, 1.0), (100.0, 1.0))


def test_wide_shapes_reach_the_lane_geometries():
    geo = {}
    for C, G, P, B in WIDE_SHAPES:
        chunk, sub, nch = M.gn_chunks(B, P)
        V, CV, PL = M.gn_lane(C, True)
        assert C % 4 == 0 and 256 < C <= 1024 and G <= 64 and nch <= 32
        assert CV <= 256 and PL >= 1 and PL * C <= 1024          # one thread per channel vector; the LDS images [PL][C]
        geo[(C, G, P, B)] = (V, CV, PL, CV * PL, 256 - CV * PL, C // G, sub, -(-P // sub), nch)
    #                              V   CV  PL live dead cpg sub nsub nch
    assert geo[(320, 32, 9, 3)] == (4, 80, 3, 240, 16, 10, 9, 1, 1)
    assert geo[(384, 32, 16, 3)] == (4, 96, 2, 192, 64, 12, 16, 1, 1)
    assert geo[(512, 32, 9, 3)] == (4, 128, 2, 256, 0, 16, 9, 1, 1)
    assert geo[(640, 32, 5, 2)] == (4, 160, 1, 160, 96, 20, 5, 1, 1)
    assert geo[(1024, 32, 5, 2)] == (4, 256, 1, 256, 0, 32, 5, 1, 1)
    assert geo[(512, 32, 130, 3)] == (4, 128, 2, 256, 0, 16, 64, 3, 3)
    for C0, C1 in WIDE_SPLITS:
        assert C0 % 4 == 0 and C1 % 4 == 0 and 256 < C0 + C1 <= 1024


def test_scalar_build_has_no_lane_above_256():
    """One channel per thread: C = 258 would need 258 threads (PL = 0), which is why the scalar builds keep C <= 256."""
    assert M.gn_lane(258, False) == (1, 258, 0)
    assert M.gn_lane(256, False) == (1, 256, 1)


@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_kernel_form_meets_the_criterion_at_wide_shapes(shape):
    C, G, P, B = shape
    for mean, std in WIDE_CONDS:
        x, xd, gamma, beta = M.make_inputs(C, G, P, B, mean, std, seed=C + P)
        _judge(f"C{C} G{G} P{P} B{B} mean {mean:g} std {std:g}", x, xd, gamma, beta, G, B, M.KERNEL_FORM).finish()


@pytest.mark.parametrize("split", WIDE_SPLITS, ids=lambda s: f"{s[0]}+{s[1]}")
def test_kernel_form_meets_the_criterion_on_the_concatenations(split):
    """The reduce sees a two-source input as one tensor of C0 + C1 channels; each source has a mean of its own."""
    C0, C1 = split
    C, G, P, B = C0 + C1, 32, 9, 2
    for m0, m1 in ((0.5, 2.0), (100.0, 30.0)):
        x, xd, gamma, beta = M.make_inputs(C, G, P, B, 0.0, 1.0, seed=C0 + P, src_means=(C0, m0, m1))
        _judge(f"C{C0}+{C1} G{G} P{P} B{B} means {m0:g} | {m1:g}", x, xd, gamma, beta, G, B, M.KERNEL_FORM).finish()
