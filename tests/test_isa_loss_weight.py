"""Build-time check of the loss-weighting kernels (CPU: hipcc cross-compiles the device code): the weighted loss's part kernel in its
16-byte and scalar forms, its fold kernel (with the tracker update) and the timestep resampler; all four must report ScratchSize 0 and
no spilled VGPRs."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-latent-diffusion-model_amd", "csrc")


@pytest.fixture(scope="module")
def resource_usage():
    asm, res = os.path.join(CSRC, "ldm3d.s"), os.path.join(CSRC, "resource_usage.txt")
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))]
    if not (os.path.exists(asm) and os.path.exists(res)) or os.path.getmtime(asm) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True, capture_output=True, timeout=900)
    return open(res).read()


def test_loss_weight_kernels_use_no_scratch(resource_usage):
    blocks = {b.split()[0]: b for b in re.split(r"remark: [^\n]*Function Name: ", resource_usage)[1:]}
    names = []
    for prefix in ("_Z14lw_part_kernelILi0EE", "_Z14lw_part_kernelILi1EE", "_Z14lw_fold_kernelILi0EE", "_Z18lw_resample_kernelILi0EE"):
        found = [n for n in blocks if n.startswith(prefix)]
        assert len(found) == 1, (prefix, found)
        names += found
    for n in names:
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blocks[n])
        spill = re.search(r"VGPRs Spill: (\d+)", blocks[n])
        assert scratch and int(scratch.group(1)) == 0, (n, scratch and scratch.group(1))
        assert spill and int(spill.group(1)) == 0, (n, spill and spill.group(1))
