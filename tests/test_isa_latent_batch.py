"""Build-time checks of latent_batch_kernel (CPU: hipcc cross-compiles the device code, no GPU needed): its six instantiations keep their
names, and none uses scratch, LDS or an atomic -- in particular the dataset indices, which arrive by value in the kernel arguments and are
indexed per lane, must not be copied to scratch."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d-latent-diffusion-model_amd", "csrc")
NAMES = [f"_Z19latent_batch_kernelILi{pred}ELb{draw}EEv17LatentBatchParams" for pred in (0, 1, 2) for draw in (0, 1)]


@pytest.fixture(scope="module")
def isa():
    asm, res = os.path.join(CSRC, "ldm3d.s"), os.path.join(CSRC, "resource_usage.txt")
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))]
    if not (os.path.exists(asm) and os.path.exists(res)) or os.path.getmtime(asm) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", CSRC, "asm"], check=True, capture_output=True, timeout=900)
    return open(asm).read(), open(res).read()


def test_every_instantiation_is_there_without_scratch_or_lds(isa):
    _, res = isa
    blocks = {b.split()[0]: b for b in re.split(r"remark: [^\n]*Function Name: ", res)[1:]}
    for name in NAMES:
        assert name in blocks, name
        b = blocks[name]
        for field in (r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]", "VGPRs Spill", "SGPRs Spill"):
            m = re.search(field + r": (\d+)", b)
            assert m and int(m.group(1)) == 0, (name, field, m and m.group(1))


def test_no_atomics_and_no_scratch_instructions(isa):
    asm, _ = isa
    for name in NAMES:
        start = asm.index("\n" + name + ":")
        body = asm[start:asm.index("s_endpgm", start)]
        assert "atomic" not in body and "scratch_" not in body and "ds_" not in body, name
        assert "global_load" in body and "global_store" in body
