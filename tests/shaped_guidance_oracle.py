"""float64 restatement of guidance rescale (Lin et al. 2024, arXiv:2305.08891 section 3.4; diffusers ``rescale_noise_cfg``) and adaptive projected
guidance (Sadat et al. 2024, arXiv:2410.02416; diffusers ``normalized_guidance``, the non-original form) as apad_cfg_shaped_step defines them,
written from the formulas and not from the product code.  PARITY UNPINNED: the reference has no counterpart and diffusers is not installed.

Per clip, every sum over the clip's n values; branches [e_0 ; c] (two) or [e_0 ; e_A ; c = e_AT] (three):
  d_1 = c - e_0, weight w_1                       (two branches)
  d_1 = e_A - e_0, d_2 = e_AT - e_A, (w_1, w_2)   (three branches)
  beta != 0:  m_k = d_k + beta m_k (kept), d_k := m_k
  t_k = min(1, r / ||d_k||) if r > 0 else 1                 (zero norm: 1)
  p_k = <d_k, c> / <c, c>  (zero denominator: 0),  q_k = (1 - eta) p_k,  u_k = t_k (d_k - q_k c)
  g = e_0 + sum_k w_k u_k
  phi > 0:  g <- f g,  f = phi std(c) / std(g) + 1 - phi    (unbiased std; std(g) == 0 or n == 1: f = 1)
TEST INFRASTRUCTURE ONLY."""
import torch


def differences(eps, branches):
    """(e_0, c, [d_k]) of eps [branches * B, n] (any float dtype; widened to float64)"""
    e = eps.double().reshape(branches, -1, eps.shape[-1])
    return e[0], e[-1], [e[k + 1] - e[k] for k in range(branches - 1)]


def _std(x):
    n = x.shape[-1]
    if n < 2:
        return torch.zeros(x.shape[:-1], dtype=torch.float64)
    return ((x - x.mean(-1, keepdim=True)) ** 2).sum(-1).div(n - 1).sqrt()


def shaped_guidance(eps, branches, weights, row, momentum=None):
    """eps [branches * B, n]; weights: the branches - 1 guidance scales; row = (phi, eta, r, beta); momentum: None or float64
    [branches - 1, B, n], the state BEFORE this step.  Returns a dict: ``g`` [B, n] float64 (before the rounding to the model dtype),
    ``momentum`` (the state after the step; the input when beta == 0), the per-clip scalars ``t``, ``q`` (lists over k of [B]), ``mean_g``,
    ``std_g``, ``std_c``, ``f`` ([B]; (0, 0, 0, 1) when phi == 0, as the kernel's stats), ``stats`` [B, 8], and the intermediates ``e0``, ``c``,
    ``d`` (after the momentum), ``d_raw``, ``u``, ``g_pre`` (before the rescale) that a rounding bound needs."""
    phi, eta, r, beta = (float(v) for v in row)
    e0, c, d_raw = differences(eps, branches)
    K, B = branches - 1, e0.shape[0]
    d = list(d_raw)
    new_m = momentum
    if beta != 0.0:
        new_m = torch.stack([d_raw[k] + beta * momentum[k].double() for k in range(K)])
        d = [new_m[k] for k in range(K)]
    cc = (c * c).sum(-1)
    t, q, u = [], [], []
    for k in range(K):
        nrm = (d[k] * d[k]).sum(-1).sqrt()
        tk = torch.ones(B, dtype=torch.float64)
        if r > 0.0:
            tk = torch.where(nrm > 0, torch.minimum(tk, r / nrm.clamp_min(1e-300)), tk)
        p = torch.where(cc > 0, (d[k] * c).sum(-1) / cc.clamp_min(1e-300), torch.zeros_like(cc))
        qk = (1.0 - eta) * p
        t.append(tk)
        q.append(qk)
        u.append(tk[:, None] * (d[k] - qk[:, None] * c))
    g_pre = e0.clone()
    for k in range(K):
        g_pre = g_pre + float(weights[k]) * u[k]
    zero, one = torch.zeros(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)
    mean_g, std_g, std_c, f = zero, zero, zero, one
    if phi > 0.0:
        mean_g, std_g, std_c = g_pre.mean(-1), _std(g_pre), _std(c)
        f = torch.where(std_g > 0, phi * std_c / std_g.clamp_min(1e-300) + (1.0 - phi), one)
    g = g_pre * f[:, None] if phi > 0.0 else g_pre
    stats = torch.stack([t[0], q[0], t[1] if K == 2 else one, q[1] if K == 2 else zero, mean_g, std_g, std_c, f], dim=1)
    return dict(g=g, g_pre=g_pre, momentum=new_m, t=t, q=q, mean_g=mean_g, std_g=std_g, std_c=std_c, f=f, stats=stats, e0=e0, c=c, d=d,
                d_raw=d_raw, u=u)


def plain_cfg(eps, branches, weights):
    """e_0 + sum_k w_k d_k: classifier-free guidance on two branches, the two-scale form on three"""
    e0, _, d = differences(eps, branches)
    g = e0.clone()
    for k, dk in enumerate(d):
        g = g + float(weights[k]) * dk
    return g


def sampler_row_update(row6, x, e, m1=None, z=None):
    """one row (c_x, c_eps, c_m1, c_z, d_x, d_eps) of the six-column sampler table in float64: (x', m0)"""
    c_x, c_e, c_m, c_z, d_x, d_e = (float(v) for v in row6)
    xn = c_x * x.double() + c_e * e.double()
    if m1 is not None:
        xn = xn + c_m * m1.double()
    if z is not None:
        xn = xn + c_z * z.double()
    return xn, d_x * x.double() + d_e * e.double()


def edit_blend(xn, m, keep_row, x0, z0):
    """x' = m x' + (1 - m) (kx x0 + kz z0), m per element"""
    kx, kz = (float(v) for v in keep_row)
    return m.double() * xn + (1.0 - m.double()) * (kx * x0.double() + kz * z0.double())
