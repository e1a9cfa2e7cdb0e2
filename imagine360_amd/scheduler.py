"""DDIMScheduler with the reference's constructor keywords, attributes, ``step`` contract, ``add_noise``, ``get_velocity`` and
``__len__`` (diffusers/schedulers/scheduling_ddim.py:113-419) for the configuration of configs/prompt-dual.yaml:48-56.

Coefficients are tabulated on the host in fp32 exactly like the reference (so ``alphas_cumprod`` matches
bit for bit) and combined in fp64 python floats; on the GPU the whole CFG + update chain of the
pipeline is one elementwise HIP kernel (``fused_cfg_step``): the eta = 0 v / epsilon update of the dual pipeline on
``cfg_ddim_update``, everything else ``step`` supports (eta > 0, clip_sample, prediction_type="sample",
use_clipped_model_output) on ``cfg_ddim_step``; with ``guidance_rescale`` (arXiv 2305.08891, section 3.4) a statistics launch
precedes ``cfg_ddim_step``; with ``guidance_apg`` (adaptive projected guidance, arXiv 2410.02416; ``projected_guidance`` is the
definition) a statistics launch precedes the step kernel on the projected guidance.

``DPMSolverMultistepScheduler`` (DPM-Solver++ 2M, arXiv 2211.01095) is the second-order sampler on the same tables and timestep grid;
its update runs on ``cfg_multistep_step`` / ``cfg_multistep_step_windows`` with an fp32 x0 history per latent.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class _Cfg(dict):
    __getattr__ = dict.get


def betas_for_alpha_bar(num_diffusion_timesteps, max_beta=0.999):
    """scheduling_ddim.py:49-79: the Glide cosine schedule ("squaredcos_cap_v2")."""
    def alpha_bar(time_step):
        return math.cos((time_step + 0.008) / 1.008 * math.pi / 2) ** 2

    betas = []
    for i in range(num_diffusion_timesteps):
        t1, t2 = i / num_diffusion_timesteps, (i + 1) / num_diffusion_timesteps
        betas.append(min(1 - alpha_bar(t2) / alpha_bar(t1), max_beta))
    return torch.tensor(betas)


def _sqrt(v):
    """``v ** 0.5`` of a host float with torch.sqrt's answer (NaN) for a negative radicand instead of a complex number."""
    return math.sqrt(v) if v >= 0 else float("nan")


def rescale_zero_terminal_snr(betas):
    """scheduling_ddim.py:77-110 (arXiv 2305.08891, algorithm 1)."""
    abar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    a0, aT = abar_sqrt[0].clone(), abar_sqrt[-1].clone()
    abar_sqrt = (abar_sqrt - aT) * (a0 / (a0 - aT))
    abar = abar_sqrt ** 2
    alphas = torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return 1 - alphas


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """arXiv 2305.08891, section 3.4 (diffusers' function of the same name): the guided prediction scaled back towards the standard
    deviation of the text-conditioned one, ``noise_cfg * (guidance_rescale * std(noise_pred_text) / std(noise_cfg) + 1 -
    guidance_rescale)``, std = torch.std (correction 1) over every dimension but the batch dimension.  The eager definition, in
    torch ops on any device; the pipeline's kernels compute the same factor inside the fused CFG + DDIM step."""
    if guidance_rescale == 0.0:
        return noise_cfg
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    return noise_cfg * (guidance_rescale * std_text / std_cfg + (1.0 - guidance_rescale))


_APG_KAPPA = {"epsilon": lambda sa, sb: (1.0 / sa, -sb / sa), "v_prediction": lambda sa, sb: (sa, -sb), "sample": lambda sa, sb: (0.0, 1.0)}


def projected_guidance(pred_uncond, pred_text, sample, guidance, sqrt_a, sqrt_b, prediction_type, eta, threshold=None, momentum=None):
    """Adaptive projected guidance (APG, arXiv 2410.02416, algorithm 1; diffusers carries it as a guider) in
    model-output space: what the step functions take in place of ``pred_uncond + guidance * (pred_text - pred_uncond)``.  The eager
    definition, in torch ops on any device and in the inputs' dtype (fp64 in, fp64 out); the pipeline's kernels compute the same
    inside the fused CFG + step kernels.

    With D(p) = kx * sample + kp * p the x0 conversion of the prediction type (epsilon: kx = 1 / sqrt_a, kp = -sqrt_b / sqrt_a;
    v_prediction: sqrt_a, -sqrt_b; sample: 0, 1) the paper updates the denoised prediction:

        Delta = D(c) - D(u),   alpha = <Delta, D(c)> / <D(c), D(c)>,   s = min(1, threshold / rms(Delta))
        D^ = D(c) + (guidance - 1) * s * (Delta - (1 - eta) * alpha * D(c))

    i.e. the guidance difference is split into its part parallel to D(c) -- the part that saturates -- and the rest, the parallel
    part is scaled by ``eta`` (0, the paper's value, removes it; 1 keeps it), and the difference is clamped first.  Mapped back to the
    model's output kp cancels, and with d = c - u, q = c + (kx / kp) * sample:

        alpha = sum d q / sum q^2,   s = min(1, threshold / (|kp| sqrt(sum d^2 / N))),   m = c + (g - 1) s d - (g - 1) s (1 - eta) alpha q

    The sums run over the WHOLE tensor (the domain of ``rescale_noise_cfg`` in this pipeline: the whole panorama latent, all views of
    the perspective latent, with context windows the whole clip of blends).  ``threshold`` is an RMS in x0 units, not the paper's
    norm: a norm over a 4 x F x h x w clip would tie the setting to clip length and resolution; the paper's radius equals
    ``threshold * sqrt(C * H * W)``.  None: no clamp.

    ``momentum = (e_prev, carry)``: the paper's momentum, and the return value is ``(m, e)``.  The paper replaces Delta by the running
    average Dbar_t = Delta_t + beta * Dbar_prev over the guided steps of a run (0 before the first) in the projection and in the
    clamp.  The state is kept in the model-output units of the step that wrote it, e_t = Dbar_t / kp_t, so that

        e = d + carry * e_prev,   carry = beta * kp_prev / kp_t   (``DDIMScheduler.apg_carry``; 0 on the first guided step of a run)

    and the formulas above hold with d replaced by e.  The returned e is the UNclamped one, the ``e_prev`` of the next guided step.
    ``carry == 0`` does not read ``e_prev`` (it may be None or hold anything) and gives ``e = d``: m is then the value without
    momentum, bit for bit.  None: m alone, as before.

    Edge cases, as the formula gives them: ``eta = 1`` without a threshold is plain CFG up to rounding (not bit for bit);
    ``pred_uncond == pred_text`` gives m = pred_text; ``sum q^2 = 0`` gives NaN; epsilon prediction at a timestep with sqrt_a = 0 has
    kp infinite, as x0 itself is (not guarded)."""
    if prediction_type not in _APG_KAPPA:
        raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
    kx, kp = _APG_KAPPA[prediction_type](sqrt_a, sqrt_b)
    u, c = pred_uncond, pred_text
    d, q = c - u, c + (kx / kp) * sample
    if momentum is not None and momentum[1] != 0.0:
        d = d + momentum[1] * momentum[0]
    alpha = (d * q).sum() / (q * q).sum()
    s = 1.0
    if threshold is not None:
        s = torch.clamp(threshold / (abs(kp) * (d * d).mean().sqrt()), max=1.0)
    gs = (guidance - 1.0) * s
    m = c + gs * d - gs * (1.0 - eta) * alpha * q
    return m if momentum is None else (m, d)


def _apg_kw(guidance_apg):
    """``apg=`` for the guided step wrappers of ``kernels``, left out when it is off: they are then called with exactly the arguments of
    before.  ``guidance_apg``: None or (eta, threshold)."""
    return dict(apg=(guidance_apg[0], guidance_apg[1])) if guidance_apg is not None else {}


def _apg_momentum_kw(guidance_apg_momentum, carry_dev):
    """``apg_momentum=`` / ``carry_dev=`` for the guided step wrappers of ``kernels``, left out when the momentum is off.
    ``guidance_apg_momentum``: None or (state, carry)."""
    if guidance_apg_momentum is None:
        return {}
    kw = dict(apg_momentum=(guidance_apg_momentum[0], guidance_apg_momentum[1]))
    if carry_dev is not None:
        kw["carry_dev"] = carry_dev
    return kw


def _rescale_kw(guidance_rescale):
    """``rescale=`` for kernels.cfg_ddim_step / cfg_ddim_step_windows, left out when it is off: with phi = 0 the kernels are
    called with exactly the arguments of before."""
    return dict(rescale=float(guidance_rescale)) if guidance_rescale != 0.0 else {}


def _ring_kw(ring):
    """``ring=True`` for kernels.cfg_ddim_step_windows, left out for the linear plan: it is then called with exactly the arguments
    of before."""
    return dict(ring=True) if ring else {}


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                 prediction_type="epsilon", rescale_betas_zero_snr=False, **kwargs):
        if trained_betas is not None:
            self.betas = torch.tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "squaredcos_cap_v2":
            self.betas = betas_for_alpha_bar(num_train_timesteps)
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented for {self.__class__}")
        if rescale_betas_zero_snr:
            self.betas = rescale_zero_terminal_snr(self.betas)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                           steps_offset=steps_offset, prediction_type=prediction_type,
                           rescale_betas_zero_snr=rescale_betas_zero_snr)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        self._timesteps_host = [int(t) + self.config.steps_offset for t in ts]
        self.timesteps = torch.from_numpy(ts).to(device) + self.config.steps_offset

    def _alphas(self, timestep):
        t = int(timestep)
        prev = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_prev

    def coefficients(self, timestep):
        """x_prev = cx * x_t + cv * model_output for eta = 0 (v-prediction or epsilon)."""
        a_t, a_prev = self._alphas(timestep)
        b_t = 1.0 - a_t
        if self.config.prediction_type == "v_prediction":
            cx = a_prev ** 0.5 * a_t ** 0.5 + (1 - a_prev) ** 0.5 * b_t ** 0.5
            cv = -(a_prev ** 0.5) * b_t ** 0.5 + (1 - a_prev) ** 0.5 * a_t ** 0.5
        elif self.config.prediction_type == "epsilon":
            cx = a_prev ** 0.5 / a_t ** 0.5
            cv = -(a_prev ** 0.5) * b_t ** 0.5 / a_t ** 0.5 + (1 - a_prev) ** 0.5
        else:
            raise ValueError(f"prediction_type {self.config.prediction_type} unsupported")
        return cx, cv

    def apg_carry(self, t_prev, t, beta):
        """The factor on the momentum state of adaptive projected guidance at the guided step ``t`` whose previous guided step of the
        run was ``t_prev``: ``beta * kp(t_prev) / kp(t)`` with kp the x0 conversion's factor on the prediction (``_APG_KAPPA``) -- the
        state is held in the model-output units of the step that wrote it (``projected_guidance``).  ``t_prev`` None (the first
        guided step of a run): 0.0, which makes the step write the state without reading it.  ``sample`` prediction: ``beta``."""
        if t_prev is None:
            return 0.0
        kappa = _APG_KAPPA[self.config.prediction_type]
        a_prev, a_t = self._alphas(t_prev)[0], self._alphas(t)[0]
        kp_prev, kp_t = kappa(a_prev ** 0.5, (1.0 - a_prev) ** 0.5)[1], kappa(a_t ** 0.5, (1.0 - a_t) ** 0.5)[1]
        return float(beta) * kp_prev / kp_t

    def new_apg_state(self, latent):
        """The momentum state of adaptive projected guidance for one latent: float32, ``latent``'s shape and device, NOT initialised --
        the first guided step of a run (carry 0) writes it without reading it.  One per latent that is stepped."""
        return torch.empty_like(latent, dtype=torch.float32)

    def uses_step_kernel(self, eta=0.0, use_clipped_model_output=False, guidance_rescale=0.0, guidance_apg=None):
        """True when an update needs ``cfg_ddim_step``: anything but the eta = 0, unclipped v / epsilon update without guidance
        rescale and without projected guidance that ``coefficients`` / ``cfg_ddim_update`` compute."""
        return (eta != 0.0 or bool(self.config.clip_sample) or bool(use_clipped_model_output) or guidance_rescale != 0.0
                or guidance_apg is not None or self.config.prediction_type not in ("v_prediction", "epsilon"))

    def kernel_mode(self, use_clipped_model_output=False):
        """Mode bits of ``cfg_ddim_step``: prediction type | clip_sample | use_clipped_model_output."""
        pt = self.config.prediction_type
        if pt not in kernels.DDIM_PRED_MODE:
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction`")
        return (kernels.DDIM_PRED_MODE[pt] | (kernels.DDIM_CLIP_SAMPLE if self.config.clip_sample else 0)
                | (kernels.DDIM_CLIPPED_OUTPUT if use_clipped_model_output else 0))

    def step_coefficients(self, timestep, eta=0.0, guidance=1.0):
        """Coefficient vector of ``cfg_ddim_step``: (guidance, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), dir, sigma) with
        sigma = eta sqrt(var), var = (b_prev / b_t)(1 - a_t / a_prev), dir = sqrt(1 - a_prev - sigma^2), in fp64 from the
        fp32 ``alphas_cumprod`` (scheduling_ddim.py:300-368).  A negative radicand gives NaN like the reference; the noise
        term is only added for eta > 0 (a negative eta still enters ``dir``, as in the reference)."""
        a_t, a_prev = self._alphas(timestep)
        b_t, b_prev = 1.0 - a_t, 1.0 - a_prev
        var = (b_prev / b_t) * (1.0 - a_t / a_prev)
        sigma = eta * _sqrt(var)
        return (float(guidance), _sqrt(a_t), _sqrt(b_t), _sqrt(a_prev), _sqrt(1.0 - a_prev - sigma ** 2),
                sigma if eta > 0 else 0.0)

    def noise_coefficients(self, timestep):
        """(sqrt(a_t), sqrt(1 - a_t)) of ``add_noise`` at one timestep as host floats: fp64 from the fp32 ``alphas_cumprod``, the
        ``sqrt_a`` / ``sqrt_b`` of ``step_coefficients`` for the same ``timestep`` (arguments of ``kernels.noise_latents``)."""
        a_t = float(self.alphas_cumprod[int(timestep)])
        return _sqrt(a_t), _sqrt(1.0 - a_t)

    def keep_coefficients(self, steps, i):
        """(sqrt_a, sqrt_b) at which the kept region of a partly regenerated clip (pipeline ``regenerate_mask``) is noised AFTER step
        ``i`` of the run's timestep list ``steps`` (arguments of ``kernels.keep_latents``): ``noise_coefficients(steps[i + 1])``, the
        level of the latent that step has just produced, and (1.0, 0.0) -- the clean clip -- after the last step."""
        i = int(i)
        if not 0 <= i < len(steps):
            raise ValueError(f"keep_coefficients: step {i} is not one of the {len(steps)} steps of the run")
        return self.noise_coefficients(steps[i + 1]) if i + 1 < len(steps) else (1.0, 0.0)

    def release_threshold(self, steps, i):
        """``tau_i = 1 - (i + 1) / n`` of release mode (pipeline ``regenerate_mode="release"``; Differential Diffusion, arXiv 2306.00950)
        AFTER step ``i`` of the ``n`` steps that are run (``steps``: the run's timestep list, or ``n`` itself): a pixel of strength
        ``s <= tau_i`` is still pinned to the noised clip, every other one has been released.  fp64, rounded once to the fp32 the
        kernel compares in (third argument of ``kernels.keep_latents_release``), returned as a host float.  Decreasing in ``i``,
        exactly 0 after the last step: ``s = 0`` stays pinned to the end, ``s = 1`` never is, and a pixel of strength ``s`` is free for
        about the last ``s n`` steps."""
        n, i = (int(steps) if isinstance(steps, int) else len(steps)), int(i)
        if not 0 <= i < n:
            raise ValueError(f"release_threshold: step {i} is not one of the {n} steps of the run")
        return float(torch.tensor(1.0 - (i + 1) / n, dtype=torch.float64).to(torch.float32))

    def timesteps_for_strength(self, strength):
        """Where a run that starts from a given clip enters the schedule of ``set_timesteps(N)`` (diffusers' img2img ``get_timesteps``):
        ``k = min(int(N * strength), N)`` steps are run, the last k of the schedule.  Returns ``(i0, steps)`` with ``i0 = N - k`` and
        ``steps = _timesteps_host[i0:]``; the clip is noised to ``steps[0]``.  ``strength`` in (0, 1]; 1.0 runs the whole schedule."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        n, strength = self.num_inference_steps, float(strength)
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength must be in (0, 1], got {strength}")
        k = min(int(n * strength), n)
        if k == 0:
            raise ValueError(f"strength={strength} leaves no step to run out of num_inference_steps N={n} (int(N * strength) = 0): "
                             f"raise one of them")
        return n - k, self._timesteps_host[n - k:]

    def guided_steps(self, steps, interval):
        """Which steps of the run's timestep list ``steps`` are guided under ``interval = (lo, hi)`` ("Applying Guidance in a Limited
        Interval", arXiv 2404.07724; pipeline ``guidance_interval``): the step at timestep t is guided iff
        ``lo * num_train_timesteps <= t < hi * num_train_timesteps``.  A list of bools, one per step; ``None``: every step.  ``lo`` and
        ``hi`` are fractions with ``0 <= lo <= hi <= 1``; ``lo == hi`` guides no step (a conditional-only sampler).  Anything else
        raises ``ValueError``.  The one definition: the eager loops, the graphed steps and the multistep scheduler all ask here."""
        if interval is None:
            return [True] * len(steps)
        try:
            lo, hi = (float(v) for v in interval)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_interval must be None or a pair (lo, hi) of fractions of num_train_timesteps, got {interval!r}") from None
        if not 0.0 <= lo <= hi <= 1.0:            # (a NaN fails every comparison)
            raise ValueError(f"guidance_interval must satisfy 0 <= lo <= hi <= 1, got {interval!r}")
        T = self.config.num_train_timesteps
        return [lo * T <= int(t) < hi * T for t in steps]

    def _noise_factors(self, like, timesteps):
        """sqrt(a_t) and sqrt(1 - a_t) of ``timesteps`` in ``like``'s dtype on its device, shaped to broadcast from the left over
        ``like``.  Works on a cast COPY of ``alphas_cumprod``: the table itself stays fp32 on the host, where ``_alphas`` reads it
        (the reference re-types the attribute in place)."""
        abar = self.alphas_cumprod.to(device=like.device, dtype=like.dtype)[timesteps.to(like.device)]
        shape = (-1,) + (1,) * (like.dim() - 1)
        return (abar ** 0.5).flatten().reshape(shape), ((1 - abar) ** 0.5).flatten().reshape(shape)

    def add_noise(self, original_samples, noise, timesteps):
        """scheduling_ddim.py:375-396: ``sqrt(a_t) x_0 + sqrt(1 - a_t) noise``, the coefficients taken from ``alphas_cumprod`` cast to the
        samples' dtype, in torch ops on the tensors' device; ``timesteps``: an integer tensor of 1 element or one per batch entry."""
        sa, sb = self._noise_factors(original_samples, timesteps)
        return sa * original_samples + sb * noise

    def get_velocity(self, sample, noise, timesteps):
        """scheduling_ddim.py:398-416: the v-prediction target ``sqrt(a_t) noise - sqrt(1 - a_t) sample``, as ``add_noise``."""
        sa, sb = self._noise_factors(sample, timesteps)
        return sa * noise - sb * sample

    def __len__(self):
        return self.config.num_train_timesteps

    def noise_dtype(self, model_dtype, sample_dtype, use_clipped_model_output=False):
        """dtype the reference's ``step`` draws its variance noise in: that of ``model_output`` after the v_prediction /
        clipped-output rewrites, which combine it with the sample."""
        if self.config.prediction_type == "v_prediction" or use_clipped_model_output:
            return torch.promote_types(model_dtype, sample_dtype)
        return model_dtype

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        """scheduling_ddim.py:251-373, formula for formula, in torch ops on the tensors' device."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        a_t, a_prev = self._alphas(timestep)
        b_t = 1.0 - a_t
        pt = self.config.prediction_type
        if pt == "epsilon":
            x0 = (sample - b_t ** 0.5 * model_output) / a_t ** 0.5
        elif pt == "sample":
            x0 = model_output
        elif pt == "v_prediction":
            x0 = a_t ** 0.5 * sample - b_t ** 0.5 * model_output
        else:
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction`")
        if not self.uses_step_kernel(eta, use_clipped_model_output):
            # the dual pipeline's update (eta = 0, no clipping): x_prev = cx x_t + cv model_output
            cx, cv = self.coefficients(timestep)
            prev = (cx * sample + cv * model_output).to(sample.dtype)
            return DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)
        if pt == "v_prediction":
            model_output = a_t ** 0.5 * model_output + b_t ** 0.5 * sample
        if self.config.clip_sample:
            x0 = torch.clamp(x0, -1, 1)
        _, _, _, sa_prev, direction, sigma = self.step_coefficients(timestep, eta)
        if use_clipped_model_output:
            model_output = (sample - a_t ** 0.5 * x0) / b_t ** 0.5
        prev = sa_prev * x0 + direction * model_output
        if eta > 0:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                                 " `variance_noise` stays `None`.")
            if variance_noise is None:
                variance_noise = torch.randn(model_output.shape, generator=generator, device=model_output.device,
                                             dtype=model_output.dtype)
            prev = prev + sigma * variance_noise
        return DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)

    def fused_cfg_step(self, pred_uncond, pred_text, guidance_scale, timestep, sample, coef_dev=None, *, eta=0.0, noise=None,
                       use_clipped_model_output=False, guidance_rescale=0.0, guidance_apg=None, guidance_apg_momentum=None, carry_dev=None):
        """CFG combine + update in one HIP kernel (pipeline_animation_inference_dual.py:791-800).  ``coef_dev``: device
        float32 coefficients read by the kernel instead of host scalars (graph replay): [3] = (guidance, cx, cv) for the
        eta = 0 v / epsilon update, [6] = ``step_coefficients`` otherwise.  ``noise``: the variance noise (like ``sample``),
        used when eta > 0.  ``guidance_rescale`` != 0: ``rescale_noise_cfg`` on the combination before the update, inside the step
        kernel (always the six-coefficient one).  ``guidance_apg = (eta, threshold)``: ``projected_guidance`` in place of the
        combination, inside the step kernel (the six-coefficient one, a statistics launch in front); not together with
        ``guidance_rescale``.  ``guidance_apg_momentum = (state, carry)`` with ``guidance_apg``: its momentum -- ``state`` from
        ``new_apg_state`` is updated in place, ``carry`` = ``apg_carry(t_prev, t, beta)``; ``carry_dev``: device float32[1] read
        instead (graph replay).  Handed on only when set."""
        u, c, x = pred_uncond.contiguous(), pred_text.contiguous(), sample.contiguous()
        if not self.uses_step_kernel(eta, use_clipped_model_output, guidance_rescale, guidance_apg):
            cx, cv = (0.0, 0.0) if coef_dev is not None else self.coefficients(timestep)
            return kernels.cfg_ddim_update(u, c, x, guidance_scale, cx, cv, coef_dev=coef_dev)
        if eta > 0 and noise is None:
            raise ValueError("fused_cfg_step: eta > 0 needs the variance noise")
        coefs = (0.0,) * 6 if coef_dev is not None else self.step_coefficients(timestep, eta, guidance_scale)
        return kernels.cfg_ddim_step(u, c, x, noise.to(x.dtype).contiguous() if eta > 0 else None,
                                     self.kernel_mode(use_clipped_model_output), coefs, coef_dev=coef_dev, **_rescale_kw(guidance_rescale),
                                     **_apg_kw(guidance_apg), **_apg_momentum_kw(guidance_apg_momentum, carry_dev))

    def fused_cfg_step_windows(self, preds, starts, weights, guidance_scale, timestep, sample, coef_dev=None, *, eta=0.0,
                               noise=None, use_clipped_model_output=False, guidance_rescale=0.0, ring=False, guidance_apg=None,
                               guidance_apg_momentum=None, carry_dev=None):
        """``fused_cfg_step`` over sliding temporal context windows: the per-frame weighted blend of the windows' CFG-combined
        predictions + the update, one HIP kernel (``kernels.cfg_ddim_step_windows``).  ``preds`` [nW, 2, ...]: window k's
        CFG-batched prediction in slot k, in ``sample``'s layout with L frames;  ``starts`` device int32 [nW], ``weights`` device
        float32 [L] (imagine360_amd.context).  The step kernel serves eta = 0 as well, so ``coef_dev`` is always float32[6] =
        ``step_coefficients``.  ``guidance_rescale`` != 0: ``rescale_noise_cfg`` on the blends (guided and text), the standard
        deviations over the whole clip.  ``ring``: the windows of a looping clip (context.WindowPlan(loop=True)), ``starts`` on a
        ring of F frames.  ``guidance_apg``: ``projected_guidance`` on the blends of the two halves, the sums over the whole clip;
        ``guidance_apg_momentum`` / ``carry_dev``: as in ``fused_cfg_step``, the state on the clip of blends."""
        if eta > 0 and noise is None:
            raise ValueError("fused_cfg_step_windows: eta > 0 needs the variance noise")
        x = sample.contiguous()
        coefs = (0.0,) * 6 if coef_dev is not None else self.step_coefficients(timestep, eta, guidance_scale)
        return kernels.cfg_ddim_step_windows(preds.contiguous(), x, noise.to(x.dtype).contiguous() if eta > 0 else None, starts,
                                             weights, self.kernel_mode(use_clipped_model_output), coefs, coef_dev=coef_dev, **_rescale_kw(guidance_rescale),
                                             **_ring_kw(ring), **_apg_kw(guidance_apg), **_apg_momentum_kw(guidance_apg_momentum, carry_dev))


    def fused_step(self, pred, timestep, sample, coef_dev=None, *, eta=0.0, noise=None, use_clipped_model_output=False, guidance_rescale=0.0,
                   guidance_apg=None, guidance_apg_momentum=None, carry_dev=None):
        """``fused_cfg_step`` for an UNGUIDED step (``guided_steps``): the model ran the text half alone and ``pred`` is its one
        prediction.  The same kernels in their unguided form (``kernels.ddim_update`` / ``kernels.ddim_step``: one prediction stream, no
        guidance read), the same choice between them, the same coefficient vectors -- ``coef_dev`` is the buffer the guided step reads.
        ``guidance_rescale`` is SKIPPED -- no statistics launch, no factor: rescaling a prediction towards its own standard deviation is
        the identity; the keyword only selects the six-coefficient kernel as it does for the guided steps of the run, so that both forms
        read one coefficient vector.  ``guidance_apg`` is skipped in the same way: without an unconditional prediction there is no
        guidance difference to project, and the momentum state (``guidance_apg_momentum``) is neither read nor written."""
        p, x = pred.contiguous(), sample.contiguous()
        if not self.uses_step_kernel(eta, use_clipped_model_output, guidance_rescale, guidance_apg):
            cx, cv = (0.0, 0.0) if coef_dev is not None else self.coefficients(timestep)
            return kernels.ddim_update(p, x, cx, cv, coef_dev=coef_dev)
        if eta > 0 and noise is None:
            raise ValueError("fused_step: eta > 0 needs the variance noise")
        coefs = (0.0,) * 6 if coef_dev is not None else self.step_coefficients(timestep, eta)
        return kernels.ddim_step(p, x, noise.to(x.dtype).contiguous() if eta > 0 else None, self.kernel_mode(use_clipped_model_output), coefs,
                                 coef_dev=coef_dev)

    def fused_step_windows(self, preds, starts, weights, timestep, sample, coef_dev=None, *, eta=0.0, noise=None,
                           use_clipped_model_output=False, guidance_rescale=0.0, ring=False, guidance_apg=None, guidance_apg_momentum=None,
                           carry_dev=None):
        """``fused_cfg_step_windows`` for an unguided step: ``preds`` [nW, 1, ...], the windows' text halves alone
        (``kernels.ddim_step_windows``); everything else as there, ``guidance_rescale`` and ``guidance_apg`` skipped as in ``fused_step``."""
        if eta > 0 and noise is None:
            raise ValueError("fused_step_windows: eta > 0 needs the variance noise")
        x = sample.contiguous()
        coefs = (0.0,) * 6 if coef_dev is not None else self.step_coefficients(timestep, eta)
        return kernels.ddim_step_windows(preds.contiguous(), x, noise.to(x.dtype).contiguous() if eta > 0 else None, starts, weights,
                                         self.kernel_mode(use_clipped_model_output), coefs, coef_dev=coef_dev, **_ring_kw(ring))


class DPMSolverMultistepScheduler(DDIMScheduler):
    """DPM-Solver++ 2M (arXiv 2211.01095, algorithm 2: data prediction, multistep, order <= 2) on DDIMScheduler's grid: the same
    tables, ``set_timesteps``, predecessor ``t - num_train_timesteps // N`` (below 0: ``final_alpha_cumprod``), ``add_noise``,
    ``get_velocity``, ``noise_coefficients``, ``keep_coefficients``, ``release_threshold``, ``timesteps_for_strength`` and ``kernel_mode``, all inherited.  The
    eager ``step`` below is the definition; nothing is claimed about bit parity with diffusers' class of the same name.

    With a = alphas_cumprod[t]: alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma); primed values belong to the
    predecessor of t, lambda_old to the timestep run before t.  Step i of a run's timestep list ``steps``:

        x0  = prediction-type conversion of (model output, x), clamped to [-1, 1] with clip_sample
        out = cx x + c0 x0 + c1 x0_old,      history <- x0
        sigma' == 0:    cx = 0, c0 = 1, c1 = 0
        else h = lambda' - lambda, A = -alpha' expm1(-h), cx = sigma' / sigma
          first order  (i == 0, i == len(steps) - 1, solver_order == 1):   c0 = A, c1 = 0
          second order (otherwise), r = (lambda - lambda_old) / h:          c0 = A (1 + 1 / (2 r)), c1 = -A / (2 r)

    The coefficients depend on the run (which timestep came before, first and last step), not on t alone: ``multistep_coefficients(steps,
    i, guidance)`` is a pure function of both, and ``begin_run(steps)`` tells ``step`` / ``step_coefficients`` / ``fused_cfg_step`` which
    run a timestep is looked up in (``set_timesteps`` begins the whole schedule).  The x0 history belongs to the latent, not to the
    scheduler: ``new_history(latent)`` per latent, passed as ``history=``; it is fp32 and updated in place.  A step with c1 == 0 does
    not read it, so it needs no reset between runs."""
    order = 1

    def __init__(self, *args, solver_order=2, algorithm_type="dpmsolver++", **kwargs):
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
        if algorithm_type != "dpmsolver++":
            raise ValueError(f"algorithm_type {algorithm_type!r} is not implemented: only 'dpmsolver++' (the ODE solver; no SDE variant)")
        super().__init__(*args, **kwargs)
        self.config.update(solver_order=solver_order, algorithm_type=algorithm_type)
        self._run_steps = None

    @classmethod
    def from_config(cls, config, **overrides):
        """``pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)``: the constructor keywords of another
        scheduler of this module, ``overrides`` on top."""
        return cls(**{**dict(config), **overrides})

    def set_timesteps(self, num_inference_steps, device=None):
        super().set_timesteps(num_inference_steps, device=device)
        self.begin_run(self._timesteps_host)

    def begin_run(self, steps):
        """The timestep list of the run that follows (the pipeline calls it once it knows it: ``strength`` < 1 shortens it)."""
        self._run_steps = [int(t) for t in steps]

    def new_history(self, latent):
        """The x0 history of one latent: zeros, float32, ``latent``'s shape and device.  One per latent that is stepped."""
        return torch.zeros(latent.shape, dtype=torch.float32, device=latent.device)

    def uses_step_kernel(self, eta=0.0, use_clipped_model_output=False, guidance_rescale=0.0, guidance_apg=None):
        """Always the six-coefficient kernel."""
        return True

    def _alpha_sigma_lambda(self, a):
        alpha, sigma = _sqrt(a), _sqrt(1.0 - a)
        return alpha, sigma, math.log(alpha / sigma)

    def multistep_coefficients(self, steps, i, guidance=1.0):
        """(guidance, sqrt(a_t), sqrt(1 - a_t), cx, c0, c1) of step ``i`` of the run's timestep list ``steps`` (see the class), in
        fp64 from the fp32 ``alphas_cumprod``: the coefficient vector of ``kernels.cfg_multistep_step``.  A pure function of
        (steps, i)."""
        i = int(i)
        if not 0 <= i < len(steps):
            raise ValueError(f"multistep_coefficients: step {i} is not one of the {len(steps)} steps of the run")
        a0 = float(self.alphas_cumprod[int(steps[0])])
        if a0 <= 0.0:
            raise ValueError(f"alphas_cumprod is 0 at the run's first timestep {int(steps[0])} (a zero-terminal-SNR table entered at its "
                             f"last index): lambda = ln(alpha / sigma) is not finite there and DPM-Solver++ cannot start; use DDIMScheduler "
                             f"for this schedule, or a step count whose first timestep lies below the last index")
        a_t, a_prev = self._alphas(steps[i])
        alpha, sigma, lam = self._alpha_sigma_lambda(a_t)
        head = (float(guidance), alpha, sigma)
        if a_prev >= 1.0:                       # sigma' = 0: the step lands on x0 (h is infinite)
            return head + (0.0, 1.0, 0.0)
        alpha_p, sigma_p, lam_p = self._alpha_sigma_lambda(a_prev)
        h = lam_p - lam
        A = -alpha_p * math.expm1(-h)
        cx = sigma_p / sigma
        if i == 0 or i == len(steps) - 1 or self.config.solver_order == 1:
            return head + (cx, A, 0.0)
        lam_old = self._alpha_sigma_lambda(float(self.alphas_cumprod[int(steps[i - 1])]))[2]
        r = (lam - lam_old) / h
        return head + (cx, A * (1.0 + 0.5 / r), -A * 0.5 / r)

    def step_coefficients(self, timestep, eta=0.0, guidance=1.0):
        """``multistep_coefficients`` of the step at ``timestep`` in the run ``begin_run`` named -- what the graphed steps upload.  A
        timestep the run does not hold (the warm-up of a graphed step under ``strength`` < 1, whose numbers are dropped) gets the
        first-order vector of that timestep."""
        if eta != 0.0:
            raise ValueError("DPMSolverMultistepScheduler has no stochastic variant (eta must be 0): use DDIMScheduler for eta > 0")
        if self._run_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = int(timestep)
        if t in self._run_steps:
            return self.multistep_coefficients(self._run_steps, self._run_steps.index(t), guidance)
        if float(self.alphas_cumprod[t]) <= 0.0:        # (no lambda there; the numbers are dropped: leave x as it is)
            return (float(guidance), 0.0, 1.0, 1.0, 0.0, 0.0)
        return self.multistep_coefficients([t], 0, guidance)

    def step(self, model_output, timestep, sample, history=None, eta=0.0, return_dict=True, **kwargs):
        """The eager definition, in torch ops on the tensors' device and in their dtype (fp64 for a reference): the update of the class
        comment at ``timestep`` of the current run.  ``history``: this latent's x0 of the step before (``new_history``, or any float
        tensor like ``sample``), overwritten with this step's x0; it may be None where the step is first order."""
        _, sa, sb, cx, c0, c1 = self.step_coefficients(timestep, eta)
        pt = self.config.prediction_type
        if pt == "epsilon":
            x0 = (sample - sb * model_output) / sa
        elif pt == "sample":
            x0 = model_output
        elif pt == "v_prediction":
            x0 = sa * sample - sb * model_output
        else:
            raise ValueError(f"prediction_type given as {pt} must be one of `epsilon`, `sample`, or `v_prediction`")
        if self.config.clip_sample:
            x0 = torch.clamp(x0, -1, 1)
        prev = cx * sample + c0 * x0
        if c1 != 0.0:
            if history is None:
                raise ValueError(f"step: the second-order step at timestep {int(timestep)} needs the history of the step before")
            prev = prev + c1 * history.to(x0.dtype)
        if history is not None:
            history.copy_(x0)
        prev = prev.to(sample.dtype)
        return DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)

    def _kernel_args(self, who, timestep, guidance_scale, coef_dev, history, eta, noise, kwargs):
        if eta != 0.0 or noise is not None:
            raise ValueError(f"{who}: DPMSolverMultistepScheduler has no stochastic variant (eta must be 0): use DDIMScheduler for eta > 0")
        if kwargs.pop("use_clipped_model_output", False):
            raise ValueError(f"{who}: use_clipped_model_output has no meaning for DPM-Solver++ (the update uses x0 alone)")
        if kwargs:
            raise TypeError(f"{who}: unexpected keywords {sorted(kwargs)}")
        if history is None:
            raise ValueError(f"{who}: history= is required (scheduler.new_history(latent), one per latent)")
        return (0.0,) * 6 if coef_dev is not None else self.step_coefficients(timestep, 0.0, guidance_scale)

    def fused_cfg_step(self, pred_uncond, pred_text, guidance_scale, timestep, sample, coef_dev=None, *, history=None, eta=0.0, noise=None,
                       guidance_rescale=0.0, guidance_apg=None, guidance_apg_momentum=None, carry_dev=None, **kwargs):
        """CFG combine + the multistep update in one HIP kernel (``kernels.cfg_multistep_step``); ``history``: this latent's
        ``new_history``, updated in place.  ``coef_dev``: device float32[6] = ``step_coefficients`` read by the kernel (graph replay).
        ``guidance_apg`` / ``guidance_apg_momentum`` / ``carry_dev``: as in ``DDIMScheduler.fused_cfg_step``; the history then receives
        the x0 of the projected guidance."""
        coefs = self._kernel_args("fused_cfg_step", timestep, guidance_scale, coef_dev, history, eta, noise, kwargs)
        return kernels.cfg_multistep_step(pred_uncond.contiguous(), pred_text.contiguous(), sample.contiguous(), history, self.kernel_mode(),
                                          coefs, coef_dev=coef_dev, **_rescale_kw(guidance_rescale), **_apg_kw(guidance_apg),
                                          **_apg_momentum_kw(guidance_apg_momentum, carry_dev))

    def fused_cfg_step_windows(self, preds, starts, weights, guidance_scale, timestep, sample, coef_dev=None, *, history=None, eta=0.0,
                               noise=None, guidance_rescale=0.0, ring=False, guidance_apg=None, guidance_apg_momentum=None, carry_dev=None,
                               **kwargs):
        """``fused_cfg_step`` on the blend of sliding temporal context windows (``kernels.cfg_multistep_step_windows``; arguments of
        ``DDIMScheduler.fused_cfg_step_windows``)."""
        coefs = self._kernel_args("fused_cfg_step_windows", timestep, guidance_scale, coef_dev, history, eta, noise, kwargs)
        return kernels.cfg_multistep_step_windows(preds.contiguous(), sample.contiguous(), history, starts, weights, self.kernel_mode(), coefs,
                                                  coef_dev=coef_dev, **_rescale_kw(guidance_rescale), **_ring_kw(ring), **_apg_kw(guidance_apg),
                                                  **_apg_momentum_kw(guidance_apg_momentum, carry_dev))

    def fused_step(self, pred, timestep, sample, coef_dev=None, *, history=None, eta=0.0, noise=None, guidance_rescale=0.0, guidance_apg=None,
                   guidance_apg_momentum=None, carry_dev=None, **kwargs):
        """``fused_cfg_step`` for an unguided step (``DDIMScheduler.fused_step``): the multistep update on the one prediction
        (``kernels.multistep_step``); ``history`` is written and read as on a guided step -- the six coefficients do not depend on guidance."""
        coefs = self._kernel_args("fused_step", timestep, 1.0, coef_dev, history, eta, noise, kwargs)
        return kernels.multistep_step(pred.contiguous(), sample.contiguous(), history, self.kernel_mode(), coefs, coef_dev=coef_dev)

    def fused_step_windows(self, preds, starts, weights, timestep, sample, coef_dev=None, *, history=None, eta=0.0, noise=None,
                           guidance_rescale=0.0, ring=False, guidance_apg=None, guidance_apg_momentum=None, carry_dev=None, **kwargs):
        """``fused_cfg_step_windows`` for an unguided step: ``preds`` [nW, 1, ...] (``kernels.multistep_step_windows``)."""
        coefs = self._kernel_args("fused_step_windows", timestep, 1.0, coef_dev, history, eta, noise, kwargs)
        return kernels.multistep_step_windows(preds.contiguous(), sample.contiguous(), history, starts, weights, self.kernel_mode(), coefs,
                                              coef_dev=coef_dev, **_ring_kw(ring))
