"""One denoising step captured in a hipGraph (torch.cuda.CUDAGraph on ROCm).

A cfg2 step is ~3000 kernel launches; issued from Python that is 0.4-0.6 s of host time, i.e. the loop is
launch-bound on a slow host.  Everything in the step is static-shaped and sync-free, so it is captured once and
replayed: per step the host only refreshes four tiny device buffers (timestep, (guidance, cx, cv), the 7 WarpAttn
coins drawn from Python's RNG in the reference's order) and calls replay().  The per-step IP-adapter noise is drawn
inside the graph from torch's device generator (graph-safe philox state), like the reference's GPU path.  Stochastic
sampling (eta > 0) draws the two variance noises inside the graph as well, right before each branch's update, from the
caller's generator (registered with the graph) or the default one; the coefficients are then (guidance, sqrt a_t,
sqrt b_t, sqrt a_prev, dir, sigma) for ``cfg_ddim_step``.  Guidance rescale (``guidance_rescale`` != 0) adds one captured
statistics launch in front of each branch's step launch; its workspace is a graph-pool tensor and nothing more is uploaded.
Adaptive projected guidance (``guidance_apg``) is captured the same way: its statistics launch and its step launch per branch read
sqrt a_t, sqrt b_t and the guidance from the six uploaded coefficients; only the guided graph of a guidance interval holds them.
Its momentum (``guidance_apg_momentum`` = beta) adds one fp32 state per branch, updated in place by the captured step launch, and a
one-float device carry (``scheduler.apg_carry``) that ``step`` computes on the host for every GUIDED step and uploads through a pinned
ring of its own; a carry of 0 makes the kernels write the state without reading it, so no buffer is ever cleared.
A partly regenerated clip (``keep``, pipeline ``regenerate_mask``) adds one captured ``keep_latents`` launch after the two step launches;
its two coefficients are a fifth tiny buffer, refreshed per step through a pinned ring of its own.  A release-mode region
(``regenerate_mode="release"``) captures ``keep_latents_release`` in its place and uploads three: the step's threshold rides along.
A guidance interval (``guidance_interval``, arXiv 2404.07724) whose run holds guided and unguided steps owns TWO captured graphs over the
same static latents, x0 histories, coefficient buffers, keep coefficients and coins: the CFG-batch body, and the text-half body (the
model on rows [1:2] / [m:2m] of every input, the unguided step kernels).  ``step`` uploads as ever and replays the one
``scheduler.guided_steps`` selects; a run whose steps are all of one kind builds only that graph.
"""
import random

import torch


class _PinnedUploads:
    """Small host -> device parameter uploads that do not stall the host: a ring of pinned staging slots, one event per
    slot (a copy from pageable memory is a memcpy + stream synchronise in PyTorch, i.e. one full host-device sync per
    upload per step)."""

    def __init__(self, like, slots=8):
        self.slots = [torch.empty(like.shape, dtype=like.dtype, pin_memory=True) for _ in range(slots)]
        self.events = [None] * slots
        self.i = 0

    def upload(self, dst, values):
        k = self.i % len(self.slots)
        self.i += 1
        if self.events[k] is not None:
            self.events[k].synchronize()          # the copy that last used this slot has been consumed
        self.slots[k].copy_(torch.as_tensor(values, dtype=dst.dtype))
        dst.copy_(self.slots[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev


class GraphedDenoiseStep:
    always_step_kernel = False      # (GraphedWindowedStep) the six-coefficient step kernel for eta = 0 as well

    def __init__(self, mv, scheduler, inputs, cameras, pano_latent, pers_latent, guidance, use_fps=True, warmup=2, cfg_pair=None,
                 eta=0.0, generator=None, use_clipped_model_output=False, frame_shard=None, guidance_rescale=0.0, keep=None,
                 guidance_interval=None, steps=None, guidance_apg=None, guidance_apg_momentum=None):
        """``inputs``: the keyword tensors of MultiViewBaseModel.forward (CFG-batched, resident on the GPU);
        ``pano_latent`` [1,4,F,H,W] / ``pers_latent`` [1,m,4,F,h,w]: initial noisy latents.
        Frame-sharded models (``mv.set_frame_shard``) capture their all-to-alls with the step: the exchange buffers are
        pre-sized and cached (dist.FrameShard), RCCL collectives are stream operations.  ``cfg_pair``: process group of the
        two ranks holding the two CFG halves of the same frames (dist.cfg_frame_layout) -- their predictions are exchanged
        inside the captured step before the CFG combine.
        ``eta`` / ``generator`` / ``use_clipped_model_output``: DDIMScheduler.step's keywords (defaults: the eta = 0 update).
        ``frame_shard`` (dist.FrameShard): with eta > 0 the variance noise is drawn for the whole clip and cut to the local
        frames, like the initial noise.  ``guidance_rescale`` / ``guidance_apg``: ``DDIMScheduler.fused_cfg_step``'s keywords.
        ``guidance_apg_momentum`` (None or beta, with ``guidance_apg`` only): the momentum of the projected guidance.  The step owns one
        state per branch and the device carry; ``step(t)`` uploads ``apg_carry(previous guided timestep, t, beta)`` before a guided step
        -- 0 on the first guided step after construction and after ``restart`` -- and an unguided step leaves carry, states and
        predecessor alone.
        ``keep`` (pipeline.KeepRegion): the kept region of a given clip, blended into both latents after the two updates.
        ``guidance_interval`` (None: every step guided, one graph, nothing else runs) with ``steps``, the run's timestep list: the kinds
        of step the run holds (``scheduler.guided_steps``) are each warmed up and captured once.  The caller keeps
        ``context.ip_cache_slots`` open for both forms of the SAM features (2 entries; 2 per window) while this is built and used."""
        self.mv, self.sch, self.inp, self.cams, self.g = mv, scheduler, inputs, cameras, float(guidance)
        self.cfg_pair = cfg_pair
        self.eta, self.gen, self.clipped, self.shard = float(eta), generator, bool(use_clipped_model_output), frame_shard
        self.rescale = float(guidance_rescale)
        self.apg = guidance_apg
        if guidance_apg is not None and frame_shard is not None:
            raise ValueError("guidance_apg cannot be combined with frame_shard (its sums span all frames)")
        self.apg_beta = None if guidance_apg_momentum is None else float(guidance_apg_momentum)
        if self.apg_beta is not None and guidance_apg is None:
            raise ValueError("guidance_apg_momentum needs guidance_apg (the momentum is that of the projected guidance)")
        self._apg_prev_t = None                  # the previous guided timestep of the run; None: the next guided step has carry 0
        self.interval = guidance_interval
        kinds = [True]                           # True: the CFG-batch body, False: the text-half body
        if guidance_interval is not None:
            if cfg_pair is not None or frame_shard is not None:
                raise ValueError("guidance_interval cannot be combined with cfg_pair / frame_shard (the text-half step of a sharded model is "
                                 "not implemented)")
            flags = scheduler.guided_steps(scheduler._timesteps_host if steps is None else steps, guidance_interval)
            kinds = [k for k in (True, False) if k in flags]
            if False in kinds:
                from .dist import cfg_half_inputs
                self.inp_text = cfg_half_inputs(inputs, 1)       # views, made once: the IP-token cache keys on their identity
        self.step_kernel = self.always_step_kernel or scheduler.uses_step_kernel(self.eta, self.clipped, self.rescale, **self._apg_kw())
        dev = pano_latent.device
        # private copies: the caller's tensors may alias the model-input buffers the body writes into
        init_pano, init_pers = pano_latent.clone(), pers_latent.clone()
        self.pano_lat = init_pano.clone()
        self.pers_lat = init_pers.clone()
        # a multistep scheduler's x0 histories, one per branch (None: DDIM).  The warm-up below runs a first-order step, which only
        # writes them, and so does the first step of every run: no reset after warm-up or capture
        self.hist = (scheduler.new_history(self.pano_lat), scheduler.new_history(self.pers_lat)) if hasattr(scheduler, "new_history") else None
        # the momentum states of the projected guidance, one per branch, and the device carry.  Never cleared: the carry buffer is 0
        # through warm-up and capture (``step`` alone uploads it), and a carry of 0 writes the states without reading them
        if self.apg_beta is not None:
            self.apg_state = (scheduler.new_apg_state(self.pano_lat), scheduler.new_apg_state(self.pers_lat))
            self.apg_carry = torch.zeros(1, dtype=torch.float32, device=dev)
            self._up_apg = _PinnedUploads(self.apg_carry)
        self.timestep = torch.zeros(1, dtype=torch.int64, device=dev)
        self.coef = torch.zeros(6 if self.step_kernel else 3, dtype=torch.float32, device=dev)
        self.use_fps = use_fps
        self.graph = None
        self._up_t, self._up_c = _PinnedUploads(self.timestep), _PinnedUploads(self.coef)
        self.keep = keep
        if keep is not None:
            self.keep_coef = torch.zeros(keep.n_coef, dtype=torch.float32, device=dev)      # (sqrt_a, sqrt_b[, tau])
            self._up_keep = _PinnedUploads(self.keep_coef)
        # Building the graph must not consume randomness: the warm-up steps draw device noise (the per-step IP-adapter
        # noise) and allocating the coin buffer used to take 7 Python draws, which shifted the streams of the default
        # (graphed) pipeline relative to the eager one and to the reference for the same seeds.
        py_state, cuda_state = random.getstate(), torch.cuda.get_rng_state(dev)
        gen_state = generator.get_state() if generator is not None else None
        mv.draw_coins(dev)                       # allocates the device coin buffer
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        #  the warm-up issues the step the way the capture will: with the panorama branch on the model's side stream when
        # dual_stream is set, so that stream's allocator pool and GEMM workspaces exist before the capture begins
        was_eager = getattr(mv, "dual_stream_eager", False)
        mv.dual_stream_eager = bool(getattr(mv, "dual_stream", False))
        try:
            with torch.cuda.stream(side):            # eager warm-up off the default stream (caches, allocator)
                # (the schedule's first timestep also when the run enters it later -- pipeline ``strength`` < 1: the warm-up only has to
                # issue every launch once; its numbers are dropped, the start latents restored below, and step() uploads the real one)
                self._upload(scheduler._timesteps_host[0], draw=False)
                for _ in range(warmup):
                    for kind in kinds:
                        (self._body if kind else self._body_text)()
        finally:
            mv.dual_stream_eager = was_eager
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graphs = {}
        for kind in kinds:
            graph = self.graphs[kind] = torch.cuda.CUDAGraph()
            if generator is not None:
                graph.register_generator_state(generator)      # each replay advances it like the eager draws would
            mv.coins_preloaded = True
            try:
                # thread-local capture mode: a RCCL watchdog / other host thread touching the runtime must not abort the capture
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    (self._body if kind else self._body_text)()
            finally:
                mv.coins_preloaded = False
        self.graph = self.graphs.get(True)       # (the CFG-batch graph; None in a run without a guided step)
        # the eager warm-up steps advanced the latents; capture itself executes nothing: start from the given ones
        self.pano_lat.copy_(init_pano)
        self.pers_lat.copy_(init_pers)
        random.setstate(py_state)
        torch.cuda.synchronize()
        torch.cuda.set_rng_state(cuda_state, dev)
        if generator is not None:
            generator.set_state(gen_state)

    def _body(self):
        inp = self.inp
        inp["pano_latent"][:, :4] = self.pano_lat
        inp["latents"][:, :, :4] = self.pers_lat
        was = self.mv.coins_preloaded
        self.mv.coins_preloaded = True           # coins are uploaded by _upload, never drawn inside the body
        try:
            pred_pers, pred_pano = self.mv(
                latents=inp["latents"], pano_latent=inp["pano_latent"], timestep=self.timestep,
                prompt_embd=inp["prompt_embd"], pano_prompt_embd=inp["pano_prompt_embd"], cameras=self.cams,
                use_fps_condition=self.use_fps, use_ip_plus_cross_attention=True,
                fps_tensor_pano=inp["fps_tensor_pano"], fps_tensor_pers=inp["fps_tensor_pers"],
                reference_images_clip_feat_pano=inp["reference_images_clip_feat_pano"],
                reference_images_clip_feat_pers=inp["reference_images_clip_feat_pers"],
                relative_position_tensor=inp["relative_position_tensor"], pitchs_tensor=inp["pitchs_tensor"])
        finally:
            self.mv.coins_preloaded = was
        if self.cfg_pair is not None:
            from .dist import exchange_cfg_halves
            pred_pano, pred_pers = exchange_cfg_halves(pred_pano, self.cfg_pair), exchange_cfg_halves(pred_pers, self.cfg_pair)
        self.pred_pano, self.pred_pers = pred_pano, pred_pers          # static graph-pool tensors (inspection / tests)
        ldt, mdt = self.pano_lat.dtype, pred_pano.dtype    # latents may be kept in another 16-bit type than the model (the reference promotes)
        pred_pano, pred_pers = pred_pano.to(ldt), pred_pers.to(ldt)
        kw = dict(eta=self.eta, use_clipped_model_output=self.clipped, guidance_rescale=self.rescale, **self._apg_kw())
        new_pano = self.sch.fused_cfg_step(pred_pano[0:1], pred_pano[1:2], self.g, None, self.pano_lat, coef_dev=self.coef,
                                           noise=self._noise(self.pano_lat, mdt, 2), **kw, **self._history(0), **self._apg_momentum(0))
        new_pers = self.sch.fused_cfg_step(pred_pers[0:1], pred_pers[1:2], self.g, None, self.pers_lat, coef_dev=self.coef,
                                           noise=self._noise(self.pers_lat, mdt, 3), **kw, **self._history(1), **self._apg_momentum(1))
        self._keep(new_pano, new_pers)
        self.pano_lat.copy_(new_pano)
        self.pers_lat.copy_(new_pers)

    def _body_text(self):
        """The body of an unguided step: the model on the text half alone, then the unguided form of each branch's step kernel.  The
        IP-adapter noise is drawn for the whole CFG batch and cut (``mv._ip_noise_half``), the variance noise is drawn as ever: the
        generator advances exactly as in ``_body``."""
        inp = self.inp_text
        inp["pano_latent"][:, :4] = self.pano_lat
        inp["latents"][:, :, :4] = self.pers_lat
        was, was_half = self.mv.coins_preloaded, self.mv._ip_noise_half
        self.mv.coins_preloaded, self.mv._ip_noise_half = True, (1, 2)
        try:
            pred_pers, pred_pano = self.mv(
                latents=inp["latents"], pano_latent=inp["pano_latent"], timestep=self.timestep,
                prompt_embd=inp["prompt_embd"], pano_prompt_embd=inp["pano_prompt_embd"], cameras=self.cams,
                use_fps_condition=self.use_fps, use_ip_plus_cross_attention=True,
                fps_tensor_pano=inp["fps_tensor_pano"], fps_tensor_pers=inp["fps_tensor_pers"],
                reference_images_clip_feat_pano=inp["reference_images_clip_feat_pano"],
                reference_images_clip_feat_pers=inp["reference_images_clip_feat_pers"],
                relative_position_tensor=inp["relative_position_tensor"], pitchs_tensor=inp["pitchs_tensor"])
        finally:
            self.mv.coins_preloaded, self.mv._ip_noise_half = was, was_half
        self.pred_pano_text, self.pred_pers_text = pred_pano, pred_pers          # static graph-pool tensors (inspection / tests)
        ldt, mdt = self.pano_lat.dtype, pred_pano.dtype
        kw = dict(eta=self.eta, use_clipped_model_output=self.clipped, guidance_rescale=self.rescale, **self._apg_kw())
        new_pano = self.sch.fused_step(pred_pano.to(ldt), None, self.pano_lat, coef_dev=self.coef, noise=self._noise(self.pano_lat, mdt, 2),
                                       **kw, **self._history(0))
        new_pers = self.sch.fused_step(pred_pers.to(ldt), None, self.pers_lat, coef_dev=self.coef, noise=self._noise(self.pers_lat, mdt, 3),
                                       **kw, **self._history(1))
        self._keep(new_pano, new_pers)
        self.pano_lat.copy_(new_pano)
        self.pers_lat.copy_(new_pers)

    def _graph_for(self, t_host):
        """The graph of the step at timestep ``t_host``: the one ``scheduler.guided_steps`` selects."""
        if self.interval is None:
            return self.graph
        return self.graphs[self.sch.guided_steps([t_host], self.interval)[0]]

    def _apg_kw(self):
        """``guidance_apg=`` of the scheduler calls, left out when it is off: they are then made with exactly the keywords of before."""
        return {} if self.apg is None else dict(guidance_apg=self.apg)

    def _apg_momentum(self, branch):
        """``guidance_apg_momentum=`` / ``carry_dev=`` of one branch's GUIDED step call; nothing without momentum.  The host carry is
        not read: the kernels take the uploaded one."""
        return {} if self.apg_beta is None else dict(guidance_apg_momentum=(self.apg_state[branch], 0.0), carry_dev=self.apg_carry)

    def _upload_apg_carry(self, t_host):
        """The carry of the guided step at ``t_host``, from the previous guided timestep of the run, which ``t_host`` then becomes.  An
        unguided step uploads nothing and is no predecessor."""
        if self.apg_beta is None or (self.interval is not None and not self.sch.guided_steps([t_host], self.interval)[0]):
            return
        self._up_apg.upload(self.apg_carry, [self.sch.apg_carry(self._apg_prev_t, t_host, self.apg_beta)])
        self._apg_prev_t = t_host

    def _history(self, branch):
        """``history=`` of one branch's step call (0 panorama, 1 perspective); nothing with a scheduler that keeps none."""
        return {} if self.hist is None else dict(history=self.hist[branch])

    def _keep(self, new_pano, new_pers):
        """The kept region blended into the two fresh latents, in place (``keep`` only), coefficients from the device."""
        if self.keep is not None:
            self.keep.blend(new_pano, new_pers, coef_dev=self.keep_coef)

    def _upload_keep(self, t_host):
        if self.keep is not None:
            self._up_keep.upload(self.keep_coef, list(self.keep.coefficients_at(t_host)))

    def _noise(self, latent, model_dtype, frame_dim):
        """Variance noise of one branch (eta > 0 only), drawn where the reference's ``step`` draws it."""
        if self.eta <= 0:
            return None
        from .pipeline import variance_noise
        return variance_noise(self.sch, latent, model_dtype, self.gen, "device", self.shard, frame_dim, self.clipped)

    def _upload(self, t_host, draw=True):
        self._up_t.upload(self.timestep, [int(t_host)])
        if self.step_kernel:
            self._up_c.upload(self.coef, list(self.sch.step_coefficients(t_host, self.eta, self.g)))
        else:
            cx, cv = self.sch.coefficients(t_host)
            self._up_c.upload(self.coef, [self.g, cx, cv])
        self._upload_keep(t_host)
        if draw:
            self.mv.draw_coins(self.timestep.device)

    def step(self, t_host):
        """Advance the latents by one DDIM step at (host int) timestep ``t_host``."""
        self._upload(t_host)
        self._upload_apg_carry(t_host)
        self._graph_for(t_host).replay()
        return self.pano_lat, self.pers_lat

    def restart(self, pano_latent, pers_latent):
        """Another run of the schedule on the captured step (pipeline ``free_init_iters``): the given start latents are copied into the
        static ones -- no new capture, no warm-up (both graphs of a guidance interval read them).  ``step`` returns the static buffers, so a caller that keeps a result clones it
        first.  A multistep scheduler's histories need no reset: the first step of a run is first order and only writes them.  Nor do
        the momentum states of the projected guidance: the run's first guided step gets carry 0 and only writes them."""
        self._apg_prev_t = None
        self.pano_lat.copy_(pano_latent)
        self.pers_lat.copy_(pers_latent)


class GraphedWindowedStep(GraphedDenoiseStep):
    """One denoising step over sliding temporal context windows (imagine360_amd.context) in ONE hipGraph: the forwards of all
    windows in slot order, each reading its frames of the full-length model-input buffers (a window of a looping plan that crosses
    the end of the clip gathers them with one index_select per buffer, inside the capture) and its own cached conditioning
    and writing its prediction into slot k of the [nW, 2, ...] buffers, then the blend + CFG + DDIM kernel of each branch.
    Captured: the nW forwards with their IP-adapter noise draws, (eta > 0) the two whole-clip variance noises, both updates.
    Not captured, per step on the host: three small pinned uploads -- the timestep, the six coefficients, the [nW, 8] table of
    WarpAttn coins drawn from Python's RNG in window order -- and replay(); no synchronisation.  Building it consumes no
    randomness (GraphedDenoiseStep.__init__).  The caller keeps ``context.ip_cache_slots(mv, len(plan))`` open while this is
    built, so that every window's IP tokens exist before the capture."""
    always_step_kernel = True

    def __init__(self, mv, scheduler, inputs, cameras, pano_latent, pers_latent, guidance, plan, use_fps=True, warmup=1, eta=0.0,
                 generator=None, use_clipped_model_output=False, guidance_rescale=0.0, keep=None, guidance_interval=None, steps=None,
                 guidance_apg=None, guidance_apg_momentum=None):
        dev = pano_latent.device
        self.plan = plan
        self.static = plan.static_inputs(inputs)
        flags = scheduler.guided_steps(scheduler._timesteps_host if steps is None else steps, guidance_interval)
        if True in flags:
            self.preds_pers, self.preds_pano = plan.pred_buffers(pano_latent, pers_latent)
        if False in flags:
            # the text halves of every window's conditioning, views made once; [nW, 1, ...] prediction buffers
            self.static_text = plan.text_half(self.static)
            self.preds_pers_text, self.preds_pano_text = plan.pred_buffers(pano_latent, pers_latent, halves=1)
        self.coins = torch.zeros(len(plan), 8, dtype=torch.int32, device=dev)
        self._up_k = _PinnedUploads(self.coins)
        super().__init__(mv, scheduler, inputs, cameras, pano_latent, pers_latent, guidance, use_fps=use_fps, warmup=warmup, eta=eta,
                         generator=generator, use_clipped_model_output=use_clipped_model_output, guidance_rescale=guidance_rescale, keep=keep,
                         guidance_interval=guidance_interval, steps=steps, guidance_apg=guidance_apg,
                         guidance_apg_momentum=guidance_apg_momentum)

    def _body_text(self):
        inp = self.inp_text
        inp["pano_latent"][:, :4] = self.pano_lat
        inp["latents"][:, :, :4] = self.pers_lat
        was_half = self.mv._ip_noise_half
        self.mv._ip_noise_half = (1, 2)
        try:
            self.plan.forward(self.mv, inp, self.static_text, self.cams, self.timestep, self.use_fps, self.preds_pers_text,
                              self.preds_pano_text, coins=self.coins)
        finally:
            self.mv._ip_noise_half = was_half
        mdt = self.mv.unet.dtype
        kw = dict(coef_dev=self.coef, eta=self.eta, use_clipped_model_output=self.clipped, guidance_rescale=self.rescale,
                  ring=self.plan.loop, **self._apg_kw())
        new_pano = self.sch.fused_step_windows(self.preds_pano_text, self.plan.starts_dev, self.plan.weights, None, self.pano_lat,
                                               noise=self._noise(self.pano_lat, mdt, 2), **kw, **self._history(0))
        new_pers = self.sch.fused_step_windows(self.preds_pers_text, self.plan.starts_dev, self.plan.weights, None, self.pers_lat,
                                               noise=self._noise(self.pers_lat, mdt, 3), **kw, **self._history(1))
        self._keep(new_pano, new_pers)
        self.pano_lat.copy_(new_pano)
        self.pers_lat.copy_(new_pers)

    def _body(self):
        inp = self.inp
        inp["pano_latent"][:, :4] = self.pano_lat
        inp["latents"][:, :, :4] = self.pers_lat
        self.plan.forward(self.mv, inp, self.static, self.cams, self.timestep, self.use_fps, self.preds_pers, self.preds_pano,
                          coins=self.coins)
        mdt = self.mv.unet.dtype
        kw = dict(coef_dev=self.coef, eta=self.eta, use_clipped_model_output=self.clipped, guidance_rescale=self.rescale,
                  ring=self.plan.loop, **self._apg_kw())
        new_pano = self.sch.fused_cfg_step_windows(self.preds_pano, self.plan.starts_dev, self.plan.weights, self.g, None,
                                                   self.pano_lat, noise=self._noise(self.pano_lat, mdt, 2), **kw, **self._history(0),
                                                   **self._apg_momentum(0))
        new_pers = self.sch.fused_cfg_step_windows(self.preds_pers, self.plan.starts_dev, self.plan.weights, self.g, None,
                                                   self.pers_lat, noise=self._noise(self.pers_lat, mdt, 3), **kw, **self._history(1),
                                                   **self._apg_momentum(1))
        self._keep(new_pano, new_pers)
        self.pano_lat.copy_(new_pano)
        self.pers_lat.copy_(new_pers)

    def _upload(self, t_host, draw=True):
        self._up_t.upload(self.timestep, [int(t_host)])
        self._up_c.upload(self.coef, list(self.sch.step_coefficients(t_host, self.eta, self.g)))
        self._upload_keep(t_host)
        if draw:
            # the coins of nW successive forwards: 7 per window in execution order (MultiViewBaseModel.draw_coins)
            self._up_k.upload(self.coins, [[1 if random.random() < 0.4 else 0 for _ in range(7)] + [0] for _ in range(len(self.plan))])
