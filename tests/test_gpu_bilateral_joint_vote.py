"""The opaque-tile vote of the joint (cross) bilateral's tuned kernels (csrc/bilateral_joint.hip), held against np_bilateral_joint with
ONE odd texel in an otherwise opaque interior tile: tests/test_gpu_opaque_vote.py's method, for the kernel that came after it.

bilateral_joint_kernel builds its tap loop once per value of the vote and per layer count it can hold in LDS: r = 4 and r = 8 at
L = 1..4, r = 10 and r = 20 at L = 1 -- ten opaque loops.  A workgroup runs the opaque one only if every texel of its colour tile has
alpha == 1.0f, out-of-image texels are vec4(0), and no other joint test has a frame with a tile inside the image: the
`acc.w = accw` shortcut, the asm that keeps the ds_read_b128 alive, the vote through the first word of the guide tiles and the `held`
register that restores that word run here and nowhere else.  The frames are opaque_vote_cases' flat frames (the bilateral's tile and
positions); every frame has four flat RGBA8 guide layers, each with its own sigma.  Per case: all four channels within 1e-5
(conftest.rel_err) and check_alpha with exact_outside.  In every sequence the interior tile's colour tile is fully opaque for each
neighbour but the odd frame, so its outputs add taps of the opaque loop (every neighbour but the odd one) and of the other loop (the
odd one): the four-channel comparison on that tile pins the opaque loop's arithmetic, alpha inside the odd texel's windows is the
reference's only if the odd neighbour did NOT run it, and interior pixels outside every window must be exactly 1.0 (both loops give
that: fma(1.0, wt, acc.w) and accw + wt are the same sum).  "Slot 0" is also the texel whose guide value goes through `held`: a wrong
word there fails check_alpha at output (X0, Y0) (tests/test_opaque_vote_cases.py asserts the size of that change on the reference).

The references (opaque_vote_cases.joint_refs) are worked out once per (r, L) and shared with the CPU file.
"""
import numpy as np
import pytest

import opaque_vote_cases as ov
from opaque_vote_cases import BIL_TOL
from test_gpu_opaque_vote import F32, U8, report, run_sequence

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,L", [(R, L) for R in ov.JOINT_LAYERS for L in ov.JOINT_LAYERS[R]])
def test_joint_bilateral_over_neighbouring_frames(ctx, R, L):
    """mid_bilateral_joint with L RGBA8 guide layers of sigmas JOINT_SIGMAS[:L].  RGBA32F frames: the sequences of JOINT_SEQUENCES[R] --
    all five of opaque_vote_cases.SEQUENCES at r = 4 and 8, (3,1,1) and (5,2,2) at r = 10, (3,1,1) at r = 20; RGBA8 frames: (3,1,1) at
    r = 4 and 8.  Sequence (3,1,1) of the float frames runs a second time with the guides as RGBA32F c / 255: the same texels, so the
    same reference, and the same bits as the RGBA8 run.  With one layer every output also has the bits of mid_bilateral_temporal's
    layered form, here on tiles that vote opaque."""
    assert ov.joint_class(R, L) == "tuned"
    t = ov.bil_tile(R)
    refs = ov.joint_refs(R, L)
    sig = list(ov.JOINT_SIGMAS[:L])
    g8 = [ls[:L] for ls in ov.joint_layers(t)]
    g32 = [[ov.decode(g) for g in ls] for ls in g8]
    kw = dict(radius=R, sigma_s=ov.sigma_s(R))
    worst = []
    for dtype, seqs in ((F32, ov.JOINT_SEQUENCES[R]), (U8, ov.JOINT_U8_SEQUENCES[R])):
        frames = ov.base_frames(t, dtype)[0]
        for i in seqs:
            n, k, f_odd = ov.SEQUENCES[i]
            group, ref = refs[(dtype, i)]

            def run(p):
                seq = [ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames[:n])]
                outs = ctx.bilateral_joint(seq, g8[:n], sig, k, **kw)
                if L == 1:
                    layered = ctx.bilateral_temporal(seq, k, sigma_c=sig[0], layers=g8[:n], **kw)
                    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs, layered)), \
                        f"r={R} {dtype} {ov.SEQUENCES[i]} {p.name}: L = 1 is not the layered form's bits"
                return outs
            run_sequence(f"joint r={R} L={L} {dtype} RGBA8 guides", ov.SEQUENCES[i], group, ref, t, BIL_TOL, worst, run)
            if dtype == F32 and i == 0:
                def run32(p):
                    seq = [ov.with_odd(f, p.xy) if j == f_odd else f for j, f in enumerate(frames[:n])]
                    outs = ctx.bilateral_joint(seq, g32[:n], sig, k, **kw)
                    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs, ctx.bilateral_joint(seq, g8[:n], sig, k, **kw))), \
                        f"r={R} L={L} {p.name}: float guides c / 255 are not the RGBA8 guides' bits"
                    return outs
                run_sequence(f"joint r={R} L={L} {dtype} RGBA32F guides", ov.SEQUENCES[i], group, ref, t, BIL_TOL, worst, run32)
    report(f"joint bilateral r={R} L={L}", worst)
