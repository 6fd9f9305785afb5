"""fp64, plain-torch restatement of the rectified-flow scheduler (MONAI >= 1.4 RFlowScheduler as the project specifies it), independent of
ldm3d/schedulers.py: what the RFlow tests compare against.  CPU only, no library call.

T = num_train_timesteps, tau = t / T (1 = pure noise, 0 = data):
  add_noise         (1 - tau) x0 + tau noise                    target   x0 - noise
  set_timesteps(N)  t_i = (1 - i / N) T, rounded if discrete, transformed if asked, + steps_offset, then kept as fp32 values
  transform(t)      T r s / (1 + (r - 1) s), s = t / T, r = (numel / base_numel)^(1 / spatial_dim) * transform_scale
  step              prev = x + dt m, x0_hat = x + tau m, dt = (t - t_next) / T, or 1 / N without t_next
  sample_timesteps  u T | sigmoid(loc + scale n) T, floored if discrete, then transformed"""
import math

import torch


class RFlowRef:
    def __init__(self, num_train_timesteps=1000, use_discrete_timesteps=True, sample_method="uniform", loc=0.0, scale=1.0,
                 use_timestep_transform=False, transform_scale=1.0, steps_offset=0, base_img_size_numel=32 ** 3, spatial_dim=3):
        assert sample_method in ("uniform", "logit-normal")
        self.T = num_train_timesteps
        self.discrete, self.method, self.loc, self.scale = use_discrete_timesteps, sample_method, loc, scale
        self.use_transform, self.transform_scale, self.steps_offset = use_timestep_transform, transform_scale, steps_offset
        self.base, self.dim = base_img_size_numel, spatial_dim
        self.num_inference_steps = num_train_timesteps
        self.timesteps = None

    def ratio(self, numel):
        return (numel / self.base) ** (1.0 / self.dim) * self.transform_scale

    def transform(self, t, numel):
        r = self.ratio(numel)
        s = torch.as_tensor(t, dtype=torch.float64) / self.T
        return self.T * r * s / (1.0 + (r - 1.0) * s)

    def set_timesteps(self, n, input_img_size_numel=None):
        if n > self.T:
            raise ValueError("more inference steps than training timesteps")
        self.num_inference_steps = n
        t = (1.0 - torch.arange(n, dtype=torch.float64) / n) * self.T
        if self.discrete:
            t = torch.round(t)
        if self.use_transform:
            t = self.transform(t, input_img_size_numel)
        self.timesteps = (t + self.steps_offset).float().double()       # the timesteps are fp32 values

    def rows(self):
        """(dt, tau) of every step over the timesteps, the last stepping to 0: fp64."""
        ts = self.timesteps.tolist()
        return [((t - (ts[k + 1] if k + 1 < len(ts) else 0.0)) / self.T, t / self.T) for k, t in enumerate(ts)]

    def add_noise(self, x0, noise, timesteps):
        tau = (timesteps.double() / self.T).reshape((-1,) + (1,) * (x0.dim() - 1))
        return (1.0 - tau) * x0.double() + tau * noise.double()

    def target(self, x0, noise):
        return x0.double() - noise.double()

    def step(self, model_output, timestep, sample, next_timestep=None):
        dt = 1.0 / self.num_inference_steps if next_timestep is None else (float(timestep) - float(next_timestep)) / self.T
        m, x = model_output.double(), sample.double()
        return x + dt * m, x + float(timestep) / self.T * m

    def sample_timesteps(self, draw, numel=None):
        """``draw``: u in [0, 1) (uniform) or n ~ N(0, 1) (logit-normal), any float tensor -> t in fp64."""
        d = draw.double()
        t = (d if self.method == "uniform" else torch.sigmoid(self.loc + self.scale * d)) * self.T
        if self.discrete:
            t = torch.floor(t)
        if self.use_transform:
            t = self.transform(t, numel)
        return t


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on Python ints: the generator behind the library's device draws."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def timestep_uniform(seed, step, idx):
    """u of ldm_rflow_timesteps' device draw for dataset index ``idx``: counter = (0, idx, step, 0x1a7e0000 + 3), key = seed."""
    r = philox4x32_10((0, idx, step, 0x1A7E0003), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (r[0] >> 8) / 16777216.0


def ulp32(x):
    """The spacing of fp32 at |x| (a float)."""
    return math.ldexp(1.0, max(math.frexp(abs(x))[1] - 24, -149)) if x else math.ldexp(1.0, -149)
