"""Writes pba_reference/<images>_<points>_<track>_<seed>.npz: what the
reference's own PBA CPU double solver (oracle/_ref/libpba_ref.so, compiled by
oracle/Makefile.ref where the reference's sources are present) reports and
returns on the scenes of tests/test_pba_reference.py.  The tests run the
solver live where that library is built and read these records where it is
not (a checkout without the reference's sources), with the same assertions.

    python tests/golden/make_pba_fixture.py

Recorded per case: initial_cost, final_cost, lm_iterations as
ParallelBundleAdjuster reports them and, for the cases of the CPU test, the
solution (camera_params, qvec, tvec, xyz) the oracle's cost is evaluated at.
Data only: no reference source text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "semantic-bundle-adjustment-colmap_amd"),
          os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import oracle  # noqa: E402
import test_pba_reference as t  # noqa: E402


def main():
    os.makedirs(t.GOLD, exist_ok=True)
    for case in t.CASES + t.GPU_ONLY_CASES:
        ref = t.pba_scene(*case)
        ic, fc, it = oracle.pba_ref_solve(ref, max_iterations=300, threads=8)
        rec = {"initial_cost": np.float64(ic), "final_cost": np.float64(fc), "lm_iterations": np.int32(it)}
        if case in t.CASES:
            rec.update(camera_params=ref.camera_params, qvec=ref.qvec, tvec=ref.tvec, xyz=ref.xyz)
        np.savez_compressed(t.gold_path(case), **rec)
        print(case, ic, fc, it)


if __name__ == "__main__":
    main()
