"""fp64 restatement of ldm_latent_batch (include/ldm3d.h): the input side of a stage-2 training step from cached latents.

    z      = (mu_label[idx[b]] + sigma_label[idx[b]] * e_label[b]) * scale
    cond   =  mu_image[idx[b]] + sigma_image[idx[b]] * e_image[b]
    noisy  = sqrt_a[b] * z + sqrt_b[b] * noise[b]
    target = noise[b] | z | sqrt_a[b] * noise[b] - sqrt_b[b] * z          (prediction type 0 | 1 | 2)

Everything is torch.float64 on the CPU; the cache tensors are [N, ...], the draws and the outputs [B, ...]."""
import torch

PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}


def latent_batch_ref(mu_label, sigma_label, mu_image, sigma_image, idx, e_label, e_image, noise, sqrt_a, sqrt_b, scale, pred):
    """-> (noisy, cond, target, z), float64."""
    d = lambda t: torch.as_tensor(t).detach().cpu().double()
    idx = [int(i) for i in idx]
    B = len(idx)
    mu_l, sg_l, mu_i, sg_i = (d(t)[idx] for t in (mu_label, sigma_label, mu_image, sigma_image))
    e_l, e_i, nz = d(e_label), d(e_image), d(noise)
    bshape = (B,) + (1,) * (mu_l.dim() - 1)
    a, s = d(sqrt_a).reshape(bshape), d(sqrt_b).reshape(bshape)
    z = (mu_l + sg_l * e_l) * float(scale)
    cond = mu_i + sg_i * e_i
    noisy = a * z + s * nz
    pred = PRED.get(pred, pred)
    target = nz if pred == 0 else (z if pred == 1 else a * nz - s * z)
    return noisy, cond, target, z
