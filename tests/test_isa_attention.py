"""Build-time register check of the bf16 attention forward (CPU: hipcc cross-compiles the device code, no GPU needed)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# <S, QW, DB, D, PF, XR> of every attn_fwd_kernel instantiation launch_attn_fwd can launch with LDM_ATTN_LONG=1 (csrc/attention.h)
LAUNCHED = ["ILi1ELi4ELb1ELi32ELi1ELb0EE", "ILi1ELi4ELb1ELi64ELi1ELb0EE", "ILi1ELi4ELb1ELi128ELi1ELb0EE", "ILi1ELi4ELb1ELi256ELi1ELb0EE",
            "ILi4ELi4ELb1ELi64ELi1ELb0EE",      # 6^3: 4 groups of 4 waves
            "ILi4ELi2ELb1ELi64ELi2ELb1EE",      # long sequences with the XCD remap (LDM_ATTN_XCD)
            "ILi4ELi2ELb1ELi64ELi2ELb0EE"]      # long sequences: 4 groups of 2 waves, two K/V tiles in flight per group


def test_attention_forward_does_not_spill():
    """No scratch and no spilled VGPRs in any attention forward the default dispatch launches (resource report of `make asm`, as
    test_conv_plane_does_not_spill); the long-sequence form keeps its two prefetch sets (64 registers) in registers.
    attn_fwd_kernel<8, 2, false, 64, 1, false>, the form it replaces, stays selectable with LDM_ATTN_LONG=0 and keeps its scratch (128
    VGPRs, 36 spilled): it is not checked here."""
    csrc = os.path.join(ROOT, "3d-latent-diffusion-model_amd", "csrc")
    res = os.path.join(csrc, "resource_usage.txt")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip"))]
    if not os.path.exists(res) or os.path.getmtime(res) < max(os.path.getmtime(f) for f in srcs):
        subprocess.run(["make", "-C", csrc, "asm"], check=True, capture_output=True, timeout=900)
    blocks = {b.split()[0]: b for b in re.split(r"remark: [^\n]*Function Name: ", open(res).read())[1:]}
    mine = {n for n in blocks if n.startswith("_Z15attn_fwd_kernel")}
    assert mine == {f"_Z15attn_fwd_kernel{t}v10AttnParams" for t in LAUNCHED + ["ILi8ELi2ELb0ELi64ELi1ELb0EE"]}, sorted(mine)
    for t in LAUNCHED:
        b = blocks[f"_Z15attn_fwd_kernel{t}v10AttnParams"]
        assert "ScratchSize [bytes/lane]: 0 " in b and "VGPRs Spill: 0 " in b, (t, b[:1200])
    vgprs = int(re.search(r"VGPRs: (\d+)", blocks[f"_Z15attn_fwd_kernel{LAUNCHED[-1]}v10AttnParams"]).group(1))
    assert vgprs <= 256, vgprs                  # 8 waves per CU: two per SIMD
