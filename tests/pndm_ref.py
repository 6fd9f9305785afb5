"""fp64 restatement of MONAI >= 1.4 ``PNDMScheduler`` (PRK warm-up + PLMS): a plain, stateful torch class for the PNDM tests.

Written from the semantics section of the feature's specification, not from ldm3d/schedulers.py.  The beta / alpha-bar table is
MONAI's (fp32 linspace and cumprod: the table is data both sides share); everything after it is fp64.  Works on CPU tensors.
"""
import numpy as np
import torch


class PNDMRef:
    pndm_order = 4

    def __init__(self, num_train_timesteps=1000, schedule="linear_beta", skip_prk_steps=False, set_alpha_to_one=False,
                 prediction_type="epsilon", steps_offset=0, beta_start=1e-4, beta_end=2e-2):
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(prediction_type)
        T = num_train_timesteps
        if schedule == "scaled_linear_beta":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=torch.float32) ** 2
        elif schedule == "linear_beta":
            betas = torch.linspace(beta_start, beta_end, T, dtype=torch.float32)
        else:
            raise ValueError(schedule)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).double()
        self.num_train_timesteps = T
        self.prediction_type = prediction_type
        self.skip_prk_steps = skip_prk_steps
        self.steps_offset = steps_offset
        self.final_alpha_cumprod = 1.0 if set_alpha_to_one else float(self.alphas_cumprod[0])
        self.set_timesteps(T)

    def set_timesteps(self, n):
        T = self.num_train_timesteps
        self.num_inference_steps = n
        ratio = T // n
        _ts = np.arange(n) * ratio + self.steps_offset
        if self.skip_prk_steps:
            prk = np.array([], dtype=np.int64)
            plms = np.concatenate([_ts[:-1], _ts[-2:-1], _ts[-1:]])[::-1].copy()
        else:
            if n < 4:
                raise ValueError("n >= 4 is required with the PRK warm-up")
            p = np.repeat(_ts[-4:], 2) + np.tile(np.array([0, ratio // 2]), 4)
            prk = (np.repeat(p[:-1], 2)[1:-1])[::-1].copy()
            plms = _ts[:-3][::-1].copy()
        self.prk = prk.astype(np.int64)
        self.plms = plms.astype(np.int64)
        self.timesteps = np.concatenate([self.prk, self.plms]).astype(np.int64)
        self.ets = []
        self.counter = 0
        self.cur_sample = None
        self.cur_model_output = 0

    @property
    def ratio(self):
        return self.num_train_timesteps // self.num_inference_steps

    # ---- the effective (t, prev_t) of call `counter` made at timestep t: what transfer() sees
    def effective(self, counter, t):
        if counter < len(self.prk):
            diff = 0 if counter % 2 else self.ratio // 2
            return int(self.prk[counter // 4 * 4]), t - diff
        if counter != 1:
            return t, t - self.ratio
        return t + self.ratio, t

    def abar(self, t):
        return float(self.alphas_cumprod[t]) if t >= 0 else self.final_alpha_cumprod

    def transfer(self, x, t, prev_t, e):
        a, a2 = float(self.alphas_cumprod[t]), self.abar(prev_t)
        b, b2 = 1 - a, 1 - a2
        if self.prediction_type == "v_prediction":
            e = a ** 0.5 * e + b ** 0.5 * x
        return (a2 / a) ** 0.5 * x - (a2 - a) * e / (a * b2 ** 0.5 + (a * b * a2) ** 0.5)

    def step(self, m, t, x):
        m, x, t = m.double(), x.double(), int(t)
        if self.counter < len(self.prk):
            return self.step_prk(m, t, x), None
        return self.step_plms(m, t, x), None

    def step_prk(self, m, t, x):
        t_eff, prev_t = self.effective(self.counter, t)
        ph = self.counter % 4
        if ph == 0:
            self.cur_model_output = self.cur_model_output + m / 6
            self.ets.append(m)
            self.cur_sample = x
            e = m
        elif ph in (1, 2):
            self.cur_model_output = self.cur_model_output + m / 3
            e = m
        else:
            e = self.cur_model_output + m / 6
            self.cur_model_output = 0
        prev = self.transfer(self.cur_sample, t_eff, prev_t, e)
        self.counter += 1
        return prev

    def step_plms(self, m, t, x):
        t_eff, prev_t = self.effective(self.counter, t)
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(m)
        n = len(self.ets)
        if n == 1 and self.counter == 0:
            e = m
            self.cur_sample = x
        elif n == 1 and self.counter == 1:
            e = (m + self.ets[-1]) / 2
            x = self.cur_sample
            self.cur_sample = None
        elif n == 2:
            e = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif n == 3:
            e = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            e = (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4]) / 24
        prev = self.transfer(x, t_eff, prev_t, e)
        self.counter += 1
        return prev
