"""fp64, plain-torch restatement of classifier-free guidance for concat conditioning (cfg / cfg_fill_value of DiffusionInferer.sample and
LatentDiffusionInferer.sample in MONAI >= 1.5, as the project specifies it) and of the condition-dropout decision, independent of the
package: what the guidance tests compare against.  CPU only, no library call.

  combine        u + w (c - u)
  doubled batch  model(cat([x, x]), cat([t, t]), cond = cat([fill tensor, cond])): the unconditional half FIRST, then chunk(2) -> (u, c)
  dropout        sample with dataset index i of step s drops iff u < p,
                 u = (Philox4x32-10(counter = (0, i, s, 0x1a7e0000 + 4), key = seed)[0] >> 8) 2^-24"""
import torch

from rflow_ref import philox4x32_10

COND_DROP_TAG = 0x1A7E0000 + 4


def combine(u, c, w):
    u, c = u.double(), c.double()
    return u + float(w) * (c - u)


def doubled_inputs(x, t, cond, fill):
    """The (x, timesteps, cond) MONAI hands the model under guidance: batch 2 B, unconditional half first."""
    return torch.cat([x] * 2, dim=0), torch.cat([t] * 2, dim=0), torch.cat([torch.full_like(cond, float(fill)), cond], dim=0)


def guided_output(model, x, t, cond, w, fill):
    """``model(x, t, cond) -> output`` evaluated the way MONAI's sampler does under guidance; fp64 combine."""
    xx, tt, cc = doubled_inputs(x, t, cond, fill)
    u, c = model(xx, tt, cc).chunk(2)
    return combine(u, c, w)


def drop_uniform(seed, step, idx):
    r = philox4x32_10((0, int(idx), int(step) & 0xFFFFFFFF, COND_DROP_TAG), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (r[0] >> 8) / 16777216.0


def drop_mask(seed, step, idx, p):
    """The decisions of ldm_cond_dropout for the dataset indices ``idx``: a list of bools.  u and p are compared as the library compares
    them, in fp32 (u has 24 bits and is exact; p is rounded to fp32 once)."""
    p32 = float(torch.tensor(float(p), dtype=torch.float32))
    return [drop_uniform(seed, step, i) < p32 for i in idx]
