"""SB3 2.x ``PPO.train`` for one minibatch in torch, the independent statement of the loss that tests/test_ppo_reference.py (float64,
CPU) and tests/test_ppo_gpu.py (float32 on the GPU: the path the fused pass replaces) differentiate with autograd."""
import numpy as np
import torch


def tower(layers, out_tanh, dtype=torch.float64, device="cpu"):
    mods = []
    for k, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.asarray(W)).to(dtype))
            lin.bias.copy_(torch.from_numpy(np.asarray(b)).to(dtype))
        mods.append(lin)
        if k < len(layers) - 1 or out_tanh:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(device)


def loss(actor_m, log_std_p, critic_m, batch, clip_range, clip_range_vf, ent_coef, vf_coef):
    """``(loss, stats)``: ``ActorCriticPolicy.evaluate_actions`` with a DiagGaussianDistribution, then the losses of ``PPO.train``.
    ``batch`` holds NumPy arrays or tensors; they are taken to ``log_std_p``'s dtype and device."""
    def t(a):
        return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dtype=log_std_p.dtype, device=log_std_p.device)
    obs, adv = t(batch.observations), t(batch.advantages)
    dist = torch.distributions.Normal(actor_m(obs), torch.ones_like(log_std_p) * log_std_p.exp())
    log_prob = dist.log_prob(t(batch.actions)).sum(dim=1)
    entropy = dist.entropy().sum(dim=1)
    ratio = torch.exp(log_prob - t(batch.old_log_prob))
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = torch.zeros((), dtype=log_std_p.dtype, device=log_std_p.device)
    if critic_m is not None:
        values = critic_m(obs).flatten()
        if clip_range_vf is not None:
            values = t(batch.old_values) + torch.clamp(values - t(batch.old_values), -clip_range_vf, clip_range_vf)
        value_loss = torch.nn.functional.mse_loss(t(batch.returns), values)
    entropy_loss = -torch.mean(entropy)
    total = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - t(batch.old_log_prob)
        stats = {"loss": total, "policy_loss": policy_loss, "value_loss": value_loss, "entropy_loss": entropy_loss,
                 "approx_kl": torch.mean((torch.exp(log_ratio) - 1) - log_ratio),
                 "clip_fraction": torch.mean((torch.abs(ratio - 1) > clip_range).to(log_std_p.dtype))}
        stats = {k: float(v) for k, v in stats.items()}
    return total, stats


def gradients(actor, log_std, critic, batch, out_tanh, clip_range, clip_range_vf, ent_coef, vf_coef, dtype=torch.float64, device="cpu"):
    """``(stats, [gradient per tensor in the canonical order])`` by autograd, as float64 NumPy arrays."""
    actor_m = tower(actor, out_tanh, dtype, device)
    critic_m = tower(critic, False, dtype, device) if critic else None
    ls = torch.nn.Parameter(torch.from_numpy(np.asarray(log_std)).to(dtype=dtype, device=device))
    total, stats = loss(actor_m, ls, critic_m, batch, clip_range, clip_range_vf, ent_coef, vf_coef)
    total.backward()
    tensors = list(actor_m.parameters()) + [ls] + (list(critic_m.parameters()) if critic else [])
    # (a tensor the loss does not reach has no .grad: a critic with vf_coef = 0 still has one, of zeros)
    return stats, [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy().astype(np.float64) for p in tensors]
