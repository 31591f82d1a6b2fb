"""No scratch in the kernel instances MODE_HH4 adds or newly reaches (CPU test on the
built library, in the way of tests/test_kernel_scratch.py).

MODE_HH4 side by side sums three direction planes in the final kernel
(sgbm_final16_kernel, NACC = 3).  At 16 / 32 lanes per row those instances already
served the strip schedule of MODE_HH; at 8 lanes per row (D = 16) they are new.  Every
one of them, for every plane type, with and without the uniqueness test, the no-wrap
recurrence and the residual input, must carry no private segment."""
import os
import re

import pytest

from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_three_plane_final_kernels_have_no_scratch():
    ks = kernel_scratch()
    # sgbm_final16_kernel<NP, 3, AccT, UQ, LPR, NOWRAP, RESF>, mangled: ILi<NP>ELi3E<AccT>Lb<UQ>ELi<LPR>E...
    inst = {}
    for name, scratch in ks.items():
        m = re.search(r"sgbm_final16_kernelILi(\d+)ELi3E(\w+?)Lb([01])ELi(\d+)ELb([01])ELb([01])E", name)
        if m:
            np_, acc, uq, lpr, nw, resf = m.groups()
            acc = {"h": "u8", "t": "u16"}.get(acc, "nib")
            inst[int(np_), acc, int(uq), int(lpr), int(nw), int(resf)] = scratch
    # D 16 (8 lanes per row): every plane type, uniqueness test on and off, both nibble recurrences
    for acc, nw in (("u8", 0), ("u16", 0), ("nib", 0), ("nib", 1)):
        for uq in (0, 1):
            assert (1, acc, uq, 8, nw, 0) in inst, f"no D 16 final kernel for {acc} planes, uniqueness {uq}, no-wrap {nw}"
    # D 32 / 64 (16 lanes) and D 128 / 256 (32 lanes), and the residual form
    for key in ((1, "nib", 0, 16, 1, 1), (2, "nib", 0, 16, 1, 1), (2, "nib", 0, 32, 1, 1), (1, "u16", 1, 16, 0, 0),
                (2, "u8", 0, 16, 0, 0), (2, "u16", 0, 32, 0, 0), (4, "u16", 1, 32, 0, 0), (4, "nib", 0, 32, 0, 0)):
        assert key in inst, f"no three-plane final kernel {key}"
    bad = {k: v for k, v in inst.items() if v}
    assert not bad, f"three-plane final kernels with scratch: {bad}"
