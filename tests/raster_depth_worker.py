"""`python -m tests.raster_depth_worker OUTDIR` (library chosen by CLMGS_LIB_PATH): the 4-channel tile kernels on fixed
hand-built cases of tests/scenes.py, every output written as OUTDIR/<case>.<output>.npy, so that
tests/test_gpu_raster_depth.py can hold the A/B builds of rasterize.hip's switches to the product library."""
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import scenes as S  # noqa: E402


def fixed_cases():
    cases = {"special": S.special_entry_case()}
    for K in (63, 64, 65, 129):
        for sat in (False, True):
            cases[f"list{K}_{'sat' if sat else 'tr'}"] = S.list_case(K, sat, "middle")
    cases["nonfinite"] = S.nonfinite_case()[0]
    cases["C3"] = S.shape_case("C3")
    return cases


def main(outdir):
    from tests.test_gpu_raster_depth import fourth_channel, run4
    dev = torch.device("cuda:0")
    for i, (name, case) in enumerate(fixed_cases().items()):
        z, bgd, vd = fourth_channel(case, 50 + i)
        for k, v in run4(case, z, bgd, vd, dev).items():
            if k != "packed":
                np.save(os.path.join(outdir, f"{name}.{k}.npy"), v.numpy())
    print("raster_depth_worker ok:", os.environ.get("CLMGS_LIB_PATH", "default library"))


if __name__ == "__main__":
    main(sys.argv[1])
