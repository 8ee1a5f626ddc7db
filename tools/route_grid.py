#!/usr/bin/env python
"""Walk the threshold grid of tests/support_gemm_grid.py through two builds of libfmmt_hip and print every query whose answer differs:
fmmt_linear_fwd_route in its four modes, fmmt_linear_wgrad_route in both, fmmt_linear_wgrad_workspace and fmmt_linear_splitk_workspace.
No device.  Expected output for a change that is not meant to move a route: none.

    FMMT_BUILD_TAG=parent FMMT_CSRC_DIR=<checkout of the parent>/facialmmt_amd/csrc python -m facialmmt_amd.build
    python tools/route_grid.py facialmmt_amd/libfmmt_hip_parent.so facialmmt_amd/libfmmt_hip.so
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import support_gemm_grid as GG  # noqa: E402

FIELDS = "mode dtype M N K ldx ldw ldy ldaux ldres bias y_pre aux res rowscale epi rows_per_scale x_epi".split()


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a, b = GG.load(argv[1]), GG.load(argv[2])
    grid = GG.grid()
    differ = 0
    for q in grid:
        ra, rb = GG.ask(a, q), GG.ask(b, q)
        if ra != rb:
            differ += 1
            print(" ".join(f"{k}={v}" for k, v in zip(FIELDS, q)), "->", ra, "!=", rb)
    print(f"{len(grid)} queries, {differ} differ", file=sys.stderr)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
