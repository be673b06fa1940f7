"""DiffusionPipeline (sampling half) on the HIP kernels -- mirror of
medical_diffusion/models/pipelines/diffusion_pipeline.py: ctor :20-74, forward :232-275, denoise :278-310,
sample :312-317, interpolate :320-332.  Same signatures, keyword names, quirks (Q1-Q17) and state-dict
prefixes (`noise_estimator.`, `noise_scheduler.`, `latent_embedder.`, `ema_model.averaged_model.`).

Differences, all outside the arithmetic: no streamlit/tqdm (Q16); noise comes from a NoiseSource
(`noise=` keyword; default = device Philox keyed from torch's default CPU generator, which it advances: consecutive
`sample()` calls differ and `torch.manual_seed(0)` before `sample()` is reproducible, like the reference harness); `shard=(rank, world)` keyword partitions the batch
rows across GPUs with shard-invariant noise.  Of `_step` (:78-201) the evaluation half is mirrored (`validation_step`); training is out of scope.
"""
from __future__ import annotations

import copy
import ctypes
import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.utils._python_dispatch

from . import kernels as K
from . import lib as L
from .noise import NoiseSource, default_noise
from .scheduler import GaussianNoiseScheduler


_CMD_POOLS = {}       # (device index, stream) -> torch.cuda.MemPool the recorded iteration of the command-list loop allocates from (process-wide)
_GRAPH_STREAMS = {}   # device index -> the one side stream graph captures run on


class _PureLaunchGuard(torch.utils._python_dispatch.TorchDispatchMode):
    """Active while the library records one loop iteration: notes every ATen operator that touches device memory other than allocation and
    metadata -- such work is not a launch of the library, so a replay of the recorded list would miss it."""
    ALLOWED = {"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::new_empty", "aten::new_empty_strided", "aten::view", "aten::_unsafe_view",
               "aten::reshape", "aten::_reshape_alias", "aten::slice", "aten::select", "aten::as_strided", "aten::expand", "aten::unsqueeze", "aten::squeeze",
               "aten::t", "aten::transpose", "aten::permute", "aten::detach", "aten::alias", "aten::unbind", "aten::split", "aten::narrow",
               "aten::lift_fresh", "aten::is_pinned", "aten::stride", "aten::size", "aten::sym_size", "aten::sym_stride", "aten::sym_numel",
               "aten::sym_storage_offset", "aten::is_contiguous", "aten::contiguous", "aten::_to_copy", "aten::resize_"}

    def __init__(self):
        super().__init__()
        self.foreign = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func._schema.name
        if name not in self.ALLOWED or name in ("aten::contiguous", "aten::_to_copy"):
            def on_device(v):
                if isinstance(v, torch.Tensor):
                    return v.is_cuda
                if isinstance(v, (list, tuple)):
                    return any(on_device(u) for u in v)
                return False
            touches = on_device(out) or on_device(args) or on_device(list((kwargs or {}).values()))
            # contiguous / _to_copy of a device tensor launch a copy kernel only when they really copy
            if touches and not (name == "aten::contiguous" and out is (args[0] if args else None)):
                self.foreign.append(name)
        return out


class _GuideStage:
    """The guidance stage of one loop (mf_guide_f32): its device table -- one MfGuideStep row per EXECUTED iteration -- its workspace and the
    [B] tensors that receive the k and s of the last iteration, all made before the loop starts.  apply() is one library call (one launch where a
    row fits one workgroup), in place on the estimator's prediction; the step comes from the loop's device counter where there is one."""

    def __init__(self, spec, g_scales, recs, x_t, objective):
        phi, q, s_max, schedule = spec
        dev, B = x_t.device, x_t.shape[0]
        rows = [L.MfGuideStep(float(g), float(phi), 0.0 if q is None else float(q), 0.0 if s_max is None else float(s_max), r.sqrt_recip_ac,
                              r.sqrt_recipm1_ac, int(r.t), 0) for g, r in zip(g_scales, recs)]
        self.table = K.guide_table(rows, dev)
        self.stages = (L.GUIDE_RESCALE if phi > 0 else 0) | (L.GUIDE_THRESHOLD if q is not None else 0)
        self.pair = schedule is not None          # (a schedule always evaluates the classifier-free pair)
        self.objective = objective
        self.workspace = K.guide_workspace(B, x_t.numel() // B, dev) if self.stages else None
        self.scale = torch.ones(B, dtype=torch.float32, device=dev)
        self.limit = torch.zeros(B, dtype=torch.float32, device=dev)

    def apply(self, x_t, pred, pred_uncond, step):
        return K.guide(pred, self.table, pred_uncond=pred_uncond, x_t=x_t, step=step, objective=self.objective, stages=self.stages,
                       scale_out=self.scale, limit_out=self.limit, workspace=self.workspace)


class EMAModel(nn.Module):
    """Inference view of utils/train_utils.py:5-88: only `averaged_model` is read (diffusion_pipeline.py:234-235)."""

    def __init__(self, model, **_kw):
        super().__init__()
        self.averaged_model = copy.deepcopy(model).eval()
        self.averaged_model.requires_grad_(False)


class DiffusionPipeline(nn.Module):
    def __init__(self, noise_scheduler, noise_estimator, latent_embedder=None, noise_scheduler_kwargs={}, noise_estimator_kwargs={},
                 latent_embedder_checkpoint="", estimator_objective="x_T", estimate_variance=False, use_self_conditioning=False,
                 classifier_free_guidance_dropout=0.5, num_samples=4, do_input_centering=True, clip_x0=True, use_ema=False, ema_kwargs={},
                 **_training_only):
        super().__init__()
        ne_kwargs = dict(noise_estimator_kwargs)  # the reference mutates the caller's dict (:50-51); we do not
        ne_kwargs["estimate_variance"] = estimate_variance
        ne_kwargs["use_self_conditioning"] = use_self_conditioning
        # classes + kwargs like the reference, or ready-made instances
        self.noise_scheduler = noise_scheduler(**dict(noise_scheduler_kwargs)) if isinstance(noise_scheduler, type) else noise_scheduler
        self.noise_estimator = noise_estimator(**ne_kwargs) if isinstance(noise_estimator, type) else noise_estimator
        if latent_embedder is None:
            self.latent_embedder = None
        elif isinstance(latent_embedder, type):
            from .checkpoint import load_module_from_checkpoint

            self.latent_embedder = load_module_from_checkpoint(latent_embedder, latent_embedder_checkpoint)
        else:
            self.latent_embedder = latent_embedder
        if self.latent_embedder is not None:
            for p in self.latent_embedder.parameters():
                p.requires_grad = False
        self.estimator_objective = estimator_objective
        self.use_self_conditioning = use_self_conditioning
        self.num_samples = num_samples
        self.classifier_free_guidance_dropout = classifier_free_guidance_dropout
        self.do_input_centering = do_input_centering
        self.estimate_variance = estimate_variance
        self.clip_x0 = clip_x0
        self.batch_cfg = True  # classifier-free guidance as one 2B-row UNet call (same arithmetic per row)
        self.hoist_embeddings = True  # denoise(): time/label/local embeddings of all iterations evaluated once, before the loop
        # (the memory pools of the command-list loop and the capture streams live in module-level registries keyed by device, _CMD_POOLS /
        # _GRAPH_STREAMS below: a torch.cuda.MemPool or Stream held by the nn.Module would break copy.deepcopy / pickling of the pipeline)
        self.last_cmdlist_launches = 0          # launches in the list the last command-list loop replayed (0: it ran eagerly)
        self.last_cmdlist_foreign_ops = []      # ATen operators that put device work into the recorded iteration (replay refused)
        self.time_cmdlist = False               # measurement aid: time the host side of one replayed iteration (costs a device sync)
        self.last_cmdlist_host_ms = None
        self.last_guide_scale = None            # [B] device tensors: the rescale factor k and the threshold s of the last loop's LAST iteration
        self.last_guide_limit = None            # (None: that loop ran without the guidance stage)
        self.use_ema = use_ema
        if use_ema:
            self.ema_model = EMAModel(self.noise_estimator, **ema_kwargs)

    @property
    def device(self):
        return next(self.parameters()).device

    @classmethod
    def load_from_checkpoint(cls, path, map_location=None, **overrides):
        from .checkpoint import load_pipeline_from_checkpoint

        return load_pipeline_from_checkpoint(cls, path, map_location=map_location, **overrides)

    # ------------------------------------------------------------------ one denoise iteration
    def _estimator(self):
        return self.ema_model.averaged_model if self.use_ema else self.noise_estimator

    def _predict(self, x_t, t, condition, self_cond, guidance_scale, un_cond, emb=None, win=None, guide=None, step=0, pair=False):
        """UNet call(s) of forward :240-253.  Returns (pred, pred_uncond|None, pred_var|None).
        emb = (table, i, cols_cond, cols_uncond, cols_uncond ++ cols_cond): the loop's precomputed embeddings
        (UNet.precompute_embeddings), or None.
        win: a WindowPlan (windowed denoising, _window_plan) -- x_t is the canvas [B, ...]; it is cropped into B * M windows (one launch,
        K.window_gather), the estimator runs on those rows -- t, condition, un_cond and the embedding columns come with B * M rows, window m of
        sample b at row b * M + m -- and its output is merged back to canvas shape (one launch, K.window_merge; the guidance pair's 2 B M rows as
        2 B canvas rows), so whatever follows sees canvas tensors.  The estimator is never told.
        guide: a _GuideStage (guidance_rescale= / dynamic_threshold= / guidance_schedule=) -- the pair is combined, rescaled and thresholded by
        one more library call on the canvas prediction (row `step` of its table: a host int, or the loop's device counter) and the result comes
        back as (pred, None, None): every step variant then runs as it does without a pair.  None: exactly the launches below.
        pair: evaluate the classifier-free pair whatever the scalar guidance_scale is (a guidance schedule)."""
        if guide is not None:
            canvas = x_t
            pred, pred_uncond, _ = self._predict(x_t, t, condition, self_cond, guidance_scale, un_cond, emb=emb, win=win, pair=guide.pair)
            return guide.apply(canvas, pred, pred_uncond, step), None, None
        est = self._estimator()
        if win is not None:   # (never with a learned variance head or self-conditioning: _window_plan refuses them)
            canvas_rows, x_t = x_t.shape[0], K.window_gather(x_t, win)
            merge = lambda p: K.window_merge(p, win)
        else:
            canvas_rows, merge = x_t.shape[0], (lambda p: p)
        cfg = (condition is not None) and (guidance_scale != 1.0 or pair)
        ec = (lambda cols: None) if emb is None else (lambda cols: est.step_embeddings(emb[0], emb[1], cols))
        if cfg:
            if self.estimate_variance:
                raise RuntimeError("estimate_variance with guidance_scale != 1 raises in the reference too "
                                   "(diffusion_pipeline.py:243-249 never chunks `pred`); use guidance_scale=1")
            if self.batch_cfg and not self.use_self_conditioning:
                # both passes of diffusion_pipeline.py:242-243 as ONE UNet call over 2B rows (rows are independent):
                # rows [0,B) = un-guided (condition = un_cond, possibly None), rows [B,2B) = guided.
                pred2 = merge(est.forward_cfg_pair(x_t, t, condition, un_cond, emb_cache=None if emb is None else ec(emb[4])))
                B = canvas_rows
                return pred2[B:], pred2[:B], None
            pred_uncond, _ = est(x_t, t, condition=un_cond, self_cond=self_cond, emb_cache=None if emb is None else ec(emb[3]))  # un-guided pass FIRST (Q6)
            pred_cond, _ = est(x_t, t, condition=condition, self_cond=self_cond, emb_cache=None if emb is None else ec(emb[2]))
            return merge(pred_cond), merge(pred_uncond), None
        if self.estimate_variance:
            pred, pred_var = est.forward_split(x_t, t, condition=condition, self_cond=self_cond, emb_cache=None if emb is None else ec(emb[2]))
            return pred, None, pred_var
        pred, _ = est(x_t, t, condition=condition, self_cond=self_cond, emb_cache=None if emb is None else ec(emb[2]))
        return merge(pred), None, None

    # ------------------------------------------------------------------ windowed denoising
    WINDOW_KEYS = ("window", "window_stride", "window_weight")

    def _window_plan(self, canvas, window=None, window_stride=None, window_weight="tent", cold_diffusion=False):
        """the rules of `window=` / `window_stride=` / `window_weight=` (denoise, sample, sample_from), checked before anything touches the device
        -> the WindowPlan of a canvas (its spatial extents in latent cells), or None: no window, or one equal to the canvas (the un-windowed path)"""
        if window is None:
            if window_stride is not None:
                raise ValueError(f"window_stride={window_stride!r} needs window=")
            return None
        from .window import WindowPlan

        if self.use_self_conditioning:
            raise ValueError("window= with use_self_conditioning: the self-conditioning input is not carried through the windows (out of scope)")
        if self.estimate_variance:
            raise ValueError("window= with estimate_variance: the learned variance head is not merged (out of scope)")
        if cold_diffusion:
            raise ValueError("window= with cold_diffusion=True: cold diffusion runs through the single-step API, which has no windows (out of scope)")
        plan = WindowPlan(tuple(canvas), window, window_stride, window_weight, dims=getattr(self._estimator(), "spatial_dims", None))
        return None if plan.none else plan

    def _check_window(self, canvas, kwargs):
        self._window_plan(canvas, *(kwargs.get(k, d) for k, d in zip(self.WINDOW_KEYS, (None, None, "tent"))), kwargs.get("cold_diffusion", False))

    # ------------------------------------------------------------------ guidance rescale, dynamic thresholding, guidance schedules
    GUIDE_KEYS = ("guidance_rescale", "dynamic_threshold", "threshold_max", "guidance_schedule")

    @staticmethod
    def _guide_scales(schedule, ts, guidance_scale, name="guidance_schedule"):
        """the guidance scale of every executed iteration (ts: their timesteps in execution order), on the host"""
        if schedule is None:
            return [float(guidance_scale)] * len(ts)
        if callable(schedule):
            g = [float(schedule(int(t))) for t in ts]
        elif isinstance(schedule, (tuple, list)) and len(schedule) == 3 and schedule[0] == "interval":
            lo, hi = float(schedule[1]), float(schedule[2])
            if not lo <= hi:
                raise ValueError(f"{name}={schedule!r}: ('interval', t_lo, t_hi) with t_lo <= t_hi")
            g = [float(guidance_scale) if lo <= t <= hi else 1.0 for t in ts]
        else:
            try:
                g = [float(v) for v in schedule]
            except TypeError:
                raise ValueError(f"{name}={schedule!r}: a sequence of floats, a callable t -> float or ('interval', t_lo, t_hi)") from None
            if len(g) != len(ts):
                raise ValueError(f"{name}: {len(g)} entries for {len(ts)} executed iterations (one per executed iteration, in execution order)")
        if not all(math.isfinite(v) for v in g):
            raise ValueError(f"{name}: a guidance scale that is not finite: {g}")
        return g

    def _guide_spec(self, kw, condition, ts, prefix=""):
        """the rules of guidance_rescale= / dynamic_threshold= / threshold_max= / guidance_schedule= (kw: those keys, guidance_scale and
        cold_diffusion, where present), checked on the host before anything touches the device.  ts: the timesteps of the executed iterations;
        prefix: "source_" where edit() checks the twins of its inversion pass (the errors name the arguments the caller wrote).
        -> (None, None) with every argument at its default, else ((phi, q, s_max, schedule), the scale of every executed iteration)"""
        phi, q, s_max, schedule = (kw.get(k, d) for k, d in zip(self.GUIDE_KEYS, (0.0, None, None, None)))
        rescale_name, schedule_name = prefix + "guidance_rescale", prefix + "guidance_schedule"
        if phi is None:
            phi = 0.0
        if isinstance(phi, bool) or not isinstance(phi, (int, float)) or not math.isfinite(phi) or not 0.0 <= phi <= 1.0:
            raise ValueError(f"{rescale_name}={phi!r}: a finite weight in [0, 1]")
        if q is not None and (isinstance(q, bool) or not isinstance(q, (int, float)) or not (0.0 < q <= 1.0)):
            raise ValueError(f"dynamic_threshold={q!r}: None or a quantile in (0, 1]")
        if s_max is not None:
            if isinstance(s_max, bool) or not isinstance(s_max, (int, float)) or not s_max > 1.0:
                raise ValueError(f"threshold_max={s_max!r}: None or a cap > 1")
            if q is None:
                raise ValueError(f"threshold_max={s_max!r} needs dynamic_threshold=")
            if math.isinf(s_max):
                s_max = None
        if phi == 0.0 and q is None and schedule is None:
            return None, None
        on = schedule_name if schedule is not None else rescale_name if phi > 0 else "dynamic_threshold"
        if kw.get("cold_diffusion", False):
            raise ValueError(f"{on}= with cold_diffusion=True: cold diffusion runs through the single-step API, which has no guidance stage")
        if self.estimate_variance:
            raise ValueError(f"{on}= with estimate_variance: the learned-variance path takes no guidance and is not thresholded (out of scope)")
        g = kw.get("guidance_scale", 1.0)
        if schedule is not None and condition is None:
            raise ValueError(f"{schedule_name}= needs a guidance pair (condition is None)")
        if phi > 0 and (condition is None or (schedule is None and g == 1.0)):
            raise ValueError(f"{rescale_name}={phi!r} needs a guidance pair (a condition and guidance_scale != 1, or a schedule)")
        return (float(phi), None if q is None else float(q), None if s_max is None else float(s_max), schedule), self._guide_scales(schedule, ts, g, schedule_name)

    def _check_guide(self, kwargs, condition, steps, use_ddim):
        """denoise() / sample(): the rules above on the grid the loop will execute, before the first draw"""
        if any(k in kwargs for k in self.GUIDE_KEYS):
            sampler = kwargs.get("sampler")
            ts, _ = self.noise_scheduler.loop_timesteps(steps, use_ddim, kwargs.get("spacing") if sampler is not None else None)
            self._guide_spec(kwargs, condition, list(reversed(ts)))

    @torch.no_grad()
    def forward(self, x_t, t, condition=None, self_cond=None, guidance_scale=1.0, cold_diffusion=False, un_cond=None, noise=None):
        """One reverse step like diffusion_pipeline.py:232-275 -> (x_t_prior, x_0, x_T, self_cond).
        `noise`: the posterior draw of gaussian_scheduler.py:99 (tensor); N(0,1) from the default source if None."""
        if self.estimator_objective not in ("x_T", "x_0"):
            raise ValueError("Unknown Objective")
        sch = self.noise_scheduler
        pred, pred_uncond, pred_var = self._predict(x_t, t, condition, self_cond, guidance_scale, un_cond)
        if cold_diffusion:  # off the hot loop: composed from the per-row scheduler API (gaussian_scheduler.py:88-93)
            if pred_var is not None:
                raise NotImplementedError("cold_diffusion with a learned variance head")
            if pred_uncond is not None:
                g = torch.full((x_t.shape[0],), float(guidance_scale), device=x_t.device)
                m1 = torch.full((x_t.shape[0],), -1.0, device=x_t.device)
                pred = K.rows_axpby(pred_uncond, None, K.rows_axpby(pred, None, pred_uncond, m1), g)   # pu + g*(pc - pu)
            if self.estimator_objective == "x_0":
                prior, x0 = sch.estimate_x_t_prior_from_x_0(x_t, t, pred, clip_x0=self.clip_x0, cold_diffusion=True)
                xT = sch.estimate_x_T(x_t, x_0=pred, t=t, clip_x0=self.clip_x0)
                return prior, x0, xT, xT
            prior, x0 = sch.estimate_x_t_prior_from_x_T(x_t, t, pred, clip_x0=self.clip_x0, cold_diffusion=True)
            return prior, x0, pred, x0
        rec = sch.step_records([sch._uniform_t(t)], use_ddim=False)[0]
        table = sch.upload_records([rec], x_t.device)
        if noise is None:
            src = default_noise()
            src.begin(x_t.shape[0], x_t.device)
            noise = src.draw(tuple(x_t.shape))
        x_t = x_t.contiguous()
        prior, x0, xT = torch.empty_like(x_t), torch.empty_like(x_t), torch.empty_like(x_t)
        a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None if pred_uncond is None else pred_uncond.data_ptr(),
                          None if pred_var is None else pred_var.data_ptr(), noise.data_ptr(), None, 0, prior.data_ptr(), x0.data_ptr(),
                          xT.data_ptr(), table.data_ptr(), None, 0, 0 if self.estimator_objective == "x_T" else 1, int(bool(self.clip_x0)),
                          float(guidance_scale), x_t.numel())
        K.sched_step(a, outputs=(prior, x0, xT))
        self_cond = x0 if self.estimator_objective == "x_T" else xT
        return prior, x0, xT, self_cond

    # ------------------------------------------------------------------ few-step samplers (deterministic and stochastic)
    @staticmethod
    def _check_sampler(sampler, spacing, use_ddim, cold_diffusion):
        """the rules of `sampler=` / `spacing=` (denoise, sample, sample_from), checked before anything touches the device"""
        known = GaussianNoiseScheduler.SAMPLERS + GaussianNoiseScheduler.STOCHASTIC_SAMPLERS
        if sampler is not None and sampler not in known:
            raise ValueError(f"sampler={sampler!r}: None or one of {known}")
        if spacing not in GaussianNoiseScheduler.SPACINGS:
            raise ValueError(f"spacing={spacing!r}: None, 'uniform' or 'logsnr'")
        if sampler is None:
            if spacing not in (None, "uniform"):
                raise ValueError(f"spacing={spacing!r} needs a sampler ('ddim0' or 'dpmpp2m'): the default loop runs on the reference's grid")
            return
        if not use_ddim:
            raise ValueError(f"sampler={sampler!r} needs use_ddim=True (it replaces the DDIM update; the DDPM loop has no deterministic form)")
        if cold_diffusion:
            raise ValueError(f"sampler={sampler!r} with cold_diffusion=True: cold diffusion runs through the single-step API")

    def _solver_args(self, x_t, pred, pred_uncond, x0, hist, table, objective, guidance_scale, step=0, counter=None):
        """the arguments of one mf_solver_step_f32 launch, in place on x_t.  counter: int32 [2] on the device = (step, ticket word), or None
        (then `step`, a host int)."""
        return L.MfSolverArgs(x_t.data_ptr(), pred.data_ptr(), None if pred_uncond is None else pred_uncond.data_ptr(), x_t.data_ptr(),
                              None if x0 is None else x0.data_ptr(), None, None if hist is None else hist.data_ptr(), table.data_ptr(),
                              None if counter is None else counter.data_ptr(), None if counter is None else counter.data_ptr() + 4, None, int(step),
                              objective, int(bool(self.clip_x0)), float(guidance_scale), x_t.numel())

    @staticmethod
    def _solver_launch(args, blend, traj, outputs, nz=None):
        """one solver step: plain, with the inpainting blend, (traj: an MfSolverTraj) recording / keeping a slot of an inversion's trajectory, or
        (nz: an MfSolverNoise; a stochastic sampler) adding the iteration's draw, with or without the blend"""
        if nz is not None:
            K.solver_step_noise(args, nz, blend, outputs=outputs)
        elif traj is None:
            K.solver_step(args, blend, outputs=outputs)
        else:
            K.solver_step_traj(args, traj, outputs=outputs)

    @staticmethod
    def _solver_noise(noise, scales, x_t, blend, base):
        """the MfSolverNoise of a stochastic sampler's loop -> (nz, buffer or None).  A device Philox source draws inside the step's launch (draw
        base + step); where that form does not apply (a blend whose cells are not a multiple of 4) and for a host source the draw goes through
        `buffer`, filled before the launch."""
        from .noise import PhiloxDeviceNoise
        dev, B = x_t.device, x_t.shape[0]
        scale = torch.tensor(scales, dtype=torch.float32, device=dev)
        inside = isinstance(noise, PhiloxDeviceNoise) and (x_t.numel() // B) % 4 == 0 and (blend is None or blend.cells % 4 == 0)
        buf = None if inside else torch.empty_like(x_t)
        nz = L.MfSolverNoise(scale.data_ptr(), None if inside else buf.data_ptr(), 0, (noise._seed & 0xFFFFFFFFFFFFFFFF) if inside else 0,
                             noise.sample_offset if inside else 0, base, 1, B, 0)
        nz._keep = (scale, buf)
        return nz, buf

    # ------------------------------------------------------------------ the loop
    @torch.no_grad()
    def denoise(self, x_t, steps=None, condition=None, use_ddim=True, noise: Optional[NoiseSource] = None, trace=None, decode=True, use_graph=None,
                loop: Optional[str] = None, progress_cb=None, **kwargs):
        """diffusion_pipeline.py:278-310.  kwargs: guidance_scale, un_cond, cold_diffusion (forwarded to forward()
        by the reference); `eta` raises like the reference's forward() would (Q2).
        sampler="ddim0" | "dpmpp2m": a deterministic few-step sampler in place of the stochastic update -- the reference's DDIM update at
        sigma = 0, or DPM-Solver++(2M) in data-prediction form (GaussianNoiseScheduler.solver_records); needs use_ddim=True, draws no noise,
        drops a learned variance head's output.  sampler="ddim1" | "dpmpp2m_sde": a stochastic few-step sampler -- the reference's DDIM update
        at its own eta = 1 on any grid, or SDE-DPM-Solver++(2M) (GaussianNoiseScheduler.stochastic_records; meant for spacing="logsnr"); one draw
        per non-final iteration, taken inside the solver step's launch from a device Philox source (a host source is uploaded: eager loop only).
        spacing="logsnr" (with a sampler): the grid uniform in log-SNR
        (GaussianNoiseScheduler.loop_timesteps), which may run fewer than `steps` iterations.  sampler=None: the loop below, unchanged.
        progress_cb(done, total): the hook that stands where the reference drives `st.progress` and `tqdm` (diffusion_pipeline.py:289-291; SURVEY Q16:
        no streamlit import here).  Called on the host after the iterations up to `done` have been ENQUEUED -- the loop never waits for the device;
        a callback that wants finished iterations synchronises the stream itself.  The replayed loops (command list, graph) call it after the eager
        first iteration, then every max(1, total // 20) iterations; the Python loop every iteration.  The counts a caller sees are STRICTLY
        INCREASING: when the loop has to be re-run (a fused rendezvous timed out, K.with_fused_fallback) the counts already reported are not
        reported again.
        window=(h, w) | (d, h, w), window_stride=None, window_weight="tent" | "uniform": windowed denoising (MultiDiffusion) of an x_t larger than
        the trained size -- x_t is the CANVAS; every iteration the estimator runs on the overlapping windows of medfusion_amd.window.WindowPlan
        (B * M rows; `condition` / `un_cond` repeated per window once, before the loop), the predictions are merged per cell with fixed weights and
        the scheduler / solver step, the inpainting select, the draws and the decode run once on the canvas, exactly as without a window: same
        draw order, same draw count, canvas-shaped draws.  Two more launches per iteration, both the library's (all three loop forms).  A window
        equal to the canvas is the un-windowed path.  ValueError with use_self_conditioning, estimate_variance or cold_diffusion=True.
        guidance_rescale=phi in [0, 1], dynamic_threshold=q in (0, 1] (threshold_max= caps its limit, > 1), guidance_schedule= a sequence with one
        scale per EXECUTED iteration in execution order | a callable t -> float | ("interval", t_lo, t_hi) (guidance_scale inside, 1 outside): the
        guidance stage (mf_guide_f32, include/medfusion_hip.h) between the estimator and the step -- the pair combined with the iteration's
        scale, its per-sample spread brought back towards the conditional prediction's, the x_0 estimate clamped to its own per-sample quantile
        of |x_0| and divided by it -- inside the recorded iteration, no host sync, the same bits in all three loop forms.  A schedule always
        evaluates the pair.  Draws and draw order are unchanged.  With every argument at its default the loop issues exactly the launches it
        issued before.  ValueError (naming the argument) before anything touches the device: values out of range, guidance_rescale or a schedule
        without a guidance pair, a schedule of the wrong length, any of them with cold_diffusion=True or estimate_variance.  The k and s of
        the last iteration stay in last_guide_scale / last_guide_limit ([B] device tensors)."""
        self._check_sampler(kwargs.get("sampler"), kwargs.get("spacing"), use_ddim, kwargs.get("cold_diffusion", False))
        self._check_window(tuple(x_t.shape[2:]), kwargs)
        self._check_guide(kwargs, condition, steps, use_ddim)
        return self._denoise_guarded(x_t, steps, condition, use_ddim, noise, trace, decode, use_graph, loop, progress_cb, 0, None, kwargs)

    def _denoise_guarded(self, x_t, steps, condition, use_ddim, noise, trace, decode, use_graph, loop, progress_cb, start, blend, kwargs, traj=None, up=None):
        """denoise() proper: the loop under K.with_fused_fallback, whose re-run rewinds the noise source to the draw count at ENTRY (sample_from
        enters after draw #0, so a re-run keeps eps0).  start / blend / traj / up: see _denoise."""
        if not x_t.is_cuda:
            raise RuntimeError("medfusion_amd.DiffusionPipeline runs on a ROCm device only (no CPU fallback)")
        with torch.cuda.device(x_t.device):   # (see sample())
            from .noise import PhiloxDeviceNoise
            draws0 = None if noise is None else noise.draw_index
            trace0 = None if trace is None else len(trace)

            def rewind():   # (a rendezvous of a fused conv + GroupNorm launch timed out: K.with_fused_fallback re-runs the loop un-fused)
                if trace is not None:
                    del trace[trace0:]
                if noise is None:
                    return
                if not isinstance(noise, PhiloxDeviceNoise):
                    raise RuntimeError("medfusion_amd: the sampling loop must be re-run on the two-launch GroupNorm form, but its host noise source "
                                       "cannot be rewound: set MEDFUSION_FUSED_APPLY=0 when several processes share one GPU")
                noise.draw_index = draws0

            if progress_cb is not None:
                user_cb, reported = progress_cb, [0]

                def progress_cb(done, total):   # monotone across a re-run of the loop
                    if done > reported[0]:
                        reported[0] = done
                        user_cb(done, total)

            return K.with_fused_fallback(x_t.device, lambda: self._denoise(x_t, steps, condition, use_ddim, noise, trace, decode, use_graph, loop, progress_cb,
                                                                           _start=start, _blend=blend, _traj=traj, _up=up, **dict(kwargs)), rewind)

    def _denoise(self, x_t, steps, condition, use_ddim, noise, trace, decode, use_graph, loop, progress_cb=None, _start=0, _blend=None, _traj=None, _up=None,
                 **kwargs):
        """_start: index of the first executed iteration of the full loop (sample_from: the loop runs on rev[_start:], recs[_start:] of the FULL
        timestep list and the embeddings of those timesteps).  _blend = (z0, eps0, mask uint8 [B,1,...]) or None: inpainting, the kept cells of
        every iteration's next latent replaced inside the scheduler step's launch.
        _up = k (invert; a sampler, _start = 0, no blend): the loop runs UPWARD over timesteps[:k] -- iteration j evaluates the estimator at
        timesteps[j] and takes row j of GaussianNoiseScheduler.inversion_records, k - 1 iterations.  _traj: an MfSolverTraj (a sampler, no blend):
        every solver step records into / keeps from the slot its step indexes (mf_solver_step_traj_f32)."""
        K.SyncWords.reset(x_t.device)   # (the split-K counters of the convolutions: zero by invariant, re-zeroed once per loop for robustness)
        if "eta" in kwargs:
            raise TypeError("forward() got an unexpected keyword argument 'eta'")
        guidance_scale = kwargs.pop("guidance_scale", 1.0)
        un_cond = kwargs.pop("un_cond", None)
        cold_diffusion = bool(kwargs.pop("cold_diffusion", False))
        sampler, spacing = kwargs.pop("sampler", None), kwargs.pop("spacing", None)
        window = [kwargs.pop(k, d) for k, d in zip(self.WINDOW_KEYS, (None, None, "tent"))]
        guide_kw = {k: kwargs.pop(k) for k in self.GUIDE_KEYS if k in kwargs}
        if kwargs:
            raise TypeError(f"forward() got an unexpected keyword argument '{next(iter(kwargs))}'")
        self._check_sampler(sampler, spacing, use_ddim, cold_diffusion)
        win = self._window_plan(tuple(x_t.shape[2:]), *window, cold_diffusion)
        if self.estimator_objective not in ("x_T", "x_0"):
            raise ValueError("Unknown Objective")
        if not x_t.is_cuda:
            raise RuntimeError("medfusion_amd.DiffusionPipeline runs on a ROCm device only (no CPU fallback)")
        if use_graph and trace is not None:
            raise ValueError("use_graph=True cannot record a trace (the captured step is replayed, nothing returns to the host)")
        # How the loop body reaches the device (all three give the same bits: test_hipgraph_captured_step_equals_eager,
        # test_cmdlist_replay_equals_eager):
        #   "cmdlist" (default where possible): iteration 0 eager, iteration 1 recorded by the library while it runs (mf_cmdlist_begin/end),
        #             every further iteration re-issued from C (mf_cmdlist_replay): stream-ordered launches at ~1 us of host time each
        #             instead of 2.0 ms of Python -> ctypes work per iteration (profiles/r03_host_enqueue_time.txt);
        #   "graph":  the iteration as ONE captured hipGraph (use_graph=True; BASELINE configs[3] names it): no host work either, but every
        #             kernel node dispatches ~1 us later than a stream-ordered launch -- slower than the eager loop from B ~ 6 on;
        #   "eager":  the Python loop (needed for a trace, a host noise source, cold diffusion).
        from .noise import PhiloxDeviceNoise
        sch = self.noise_scheduler
        if sampler is not None:   # (the executed count decides whether the loop is long enough to replay: the log-SNR grid may drop iterations)
            timesteps, steps = sch.loop_timesteps(steps, use_ddim, spacing)
        stochastic = sampler in GaussianNoiseScheduler.STOCHASTIC_SAMPLERS
        # (a deterministic sampler draws nothing inside the loop: any noise source replays)
        replayable = (trace is None and not cold_diffusion and ((sampler is not None and not stochastic) or noise is None or isinstance(noise, PhiloxDeviceNoise))
                      and (steps is None or (steps - _start if _up is None else _up - 1) >= 4))
        if loop is not None and loop not in ("cmdlist", "graph", "eager"):
            raise ValueError(f"loop={loop!r}: 'cmdlist', 'graph' or 'eager'")
        # precedence: loop= argument, use_graph= (True: graph, False: eager), MEDFUSION_LOOP in the environment, then the default
        mode = loop or ("graph" if use_graph else "eager" if use_graph is False else os.environ.get("MEDFUSION_LOOP", ""))
        explicit = loop is not None or use_graph is not None
        if mode not in ("cmdlist", "graph", "eager"):
            mode = "cmdlist"
        if mode == "cmdlist" and (not replayable or K.prof_active()):
            if loop == "cmdlist" and not replayable:
                raise ValueError("loop='cmdlist' replays recorded launches: no trace, no host noise source, no cold diffusion, >= 4 iterations")
            mode = "eager"
        if mode == "graph" and not replayable and not explicit:
            mode = "eager"
        use_graph = mode == "graph"
        dev = x_t.device
        B = x_t.shape[0]
        Bw = B   # the estimator's rows: one per sample, or one per window of every sample (sample-major)
        if win is not None:
            Bw = B * win.M
            condition = None if condition is None else condition.repeat_interleave(win.M, dim=0)
            un_cond = None if un_cond is None else un_cond.repeat_interleave(win.M, dim=0)
        if sampler is None:
            timesteps, steps = sch.loop_timesteps(steps, use_ddim)
            recs = sch.step_records(timesteps, use_ddim)
            table = sch.upload_records(recs, dev)
        else:   # one MfSolverStep row per EXECUTED iteration: the first one is first-order wherever it sits in the grid
            scales = None
            if _up is not None:
                recs = sch.inversion_records(timesteps, sampler, stop=_up)
            elif stochastic:
                recs, scales = sch.stochastic_records(timesteps, sampler, start=_start)
            else:
                recs = sch.solver_records(timesteps, sampler, start=_start)
            table = sch.upload_solver_records(recs, dev)
        if noise is None:  # x_t supplied by the caller (interpolate): fresh source, draws start at 0
            noise = default_noise()
            noise.begin(B, dev)
        rev = list(reversed(timesteps)) if _up is None else list(timesteps[:_up - 1])   # (the loop's timesteps in execution order)
        blend = None
        if (_traj is not None or _up is not None) and (sampler is None or _blend is not None or (_up is not None and _start)):
            raise ValueError("a trajectory / an upward loop runs on a deterministic sampler, without a blend")
        if _start or _blend is not None:
            if cold_diffusion:
                raise ValueError("cold_diffusion is not built for sample_from")
            if _blend is not None:   # (the coefficient rows are indexed like the sliced step table below)
                z0, eps0, cmask = _blend
                coef = sch.blend_records(timesteps, _start).to(dev)
                cells = z0.numel() // (z0.shape[0] * z0.shape[1])
                blend = L.MfSchedBlend(z0.data_ptr(), eps0.data_ptr(), cmask.data_ptr(), coef.data_ptr(), cells, z0.shape[1], 0)
                blend._keep = (z0, eps0, cmask, coef)
            rev = rev[_start:]
            if sampler is None:
                recs = recs[_start:]
                table = sch.upload_records(recs, dev)
        objective = 0 if self.estimator_objective == "x_T" else 1
        x_t = x_t.contiguous().clone()
        guide = None
        if guide_kw:   # (rev and recs: the executed iterations; the table's rows are indexed like the step table's)
            # (g_scales: one guidance scale per executed iteration -- not `scales`, the draw scales of a stochastic sampler's rows)
            spec, g_scales = self._guide_spec(dict(guide_kw, guidance_scale=guidance_scale, cold_diffusion=cold_diffusion), condition, rev)
            if spec is not None:
                guide = _GuideStage(spec, g_scales, recs, x_t, objective)
        self.last_guide_scale, self.last_guide_limit = (None, None) if guide is None else (guide.scale, guide.limit)
        if cold_diffusion:
            # diffusion_pipeline.py:294 forwards the flag to forward() on every iteration: off the hot loop, so composed from the
            # single-step API (forward() takes no posterior draw in this mode; the DDIM update and its draw are those of :297-304)
            if use_graph or trace is not None:
                raise ValueError("cold_diffusion runs through the single-step API: no graph capture, no trace")
            for i, t in enumerate(rev):
                tt = torch.full((B,), int(t), dtype=torch.long, device=dev)
                x_prior, x_0, x_T, _ = self.forward(x_t, tt, condition, None, guidance_scale=guidance_scale, cold_diffusion=True, un_cond=un_cond)
                if use_ddim and i < len(rev) - 1:
                    r = recs[i]
                    n_ddim = noise.draw(tuple(x_t.shape))
                    a = torch.full((B,), r.ddim_sqrt_an, dtype=torch.float32, device=dev)
                    c = torch.full((B,), r.ddim_c, dtype=torch.float32, device=dev)
                    sg = torch.full((B,), r.ddim_sigma, dtype=torch.float32, device=dev)
                    x_t = K.rows_axpby(K.rows_axpby(x_0, a, x_T, c), None, n_ddim, sg)   # x0 sqrt(a') + c x_T + sigma noise
                else:
                    x_t = x_prior
                if progress_cb is not None:
                    progress_cb(i + 1, len(rev))
            if decode and self.latent_embedder is not None:
                x_t = self.latent_embedder.decode(x_t)
            return x_t
        # the deterministic samplers: the x_0 history of the second-order rows ([2][n], slots alternate with the step), and the x_0 estimate
        # as a tensor of its own only where something reads it (self-conditioning, a trace)
        hist = torch.empty((2, *x_t.shape), dtype=torch.float32, device=dev) if sampler in ("dpmpp2m", "dpmpp2m_sde") else None
        # a stochastic sampler: draw number noise.draw_index + i for executed iteration i (the last one draws nothing)
        nz, n_buf = self._solver_noise(noise, scales, x_t, blend, noise.draw_index) if stochastic else (None, None)
        if mode in ("graph", "cmdlist"):
            self._denoise_graph(x_t, rev, recs, table, condition, guidance_scale, un_cond, use_ddim, noise, objective, cmdlist=(mode == "cmdlist"),
                                progress_cb=progress_cb, blend=blend, solver=None if sampler is None else (hist, _traj, nz, n_buf), win=win, guide=guide)
        elif sampler is not None:
            t_all = torch.tensor(rev, dtype=torch.float32, device=dev).reshape(-1, 1).expand(-1, Bw).contiguous()
            x0 = torch.empty_like(x_t) if (self.use_self_conditioning or trace is not None) else None
            self_cond = None
            emb_tab = self._hoisted_embeddings(self._estimator(), t_all[:, 0].contiguous(), condition, un_cond, Bw, dev)
            for i in range(len(rev)):
                pred, pred_uncond, _ = self._predict(x_t, t_all[i], condition, self_cond, guidance_scale, un_cond,
                                                     emb=None if emb_tab is None else (emb_tab[0], i, emb_tab[1], emb_tab[2], emb_tab[3]), win=win, guide=guide, step=i)
                if stochastic and i < len(rev) - 1:
                    if n_buf is None:
                        noise.draw_index += 1                          # (draw nz.draw_base + i, generated inside the launch)
                    else:
                        noise.draw(tuple(x_t.shape), out=n_buf)
                self._solver_launch(self._solver_args(x_t, pred, pred_uncond, x0, hist, table, objective, guidance_scale, step=i), blend, _traj, (x_t, x0), nz)
                self_cond = x0 if self.use_self_conditioning else None
                if trace is not None:
                    trace.append((x0.clone(), x_t.clone()))
                if progress_cb is not None:
                    progress_cb(i + 1, len(rev))
        else:
            t_all = torch.tensor(rev, dtype=torch.float32, device=dev).reshape(-1, 1).expand(-1, Bw).contiguous()  # t.expand(B) per iteration (Q7)
            n_post = torch.empty_like(x_t)
            n_ddim = torch.empty_like(x_t)
            x0 = torch.empty_like(x_t)
            self_cond = None
            est = self._estimator()
            emb_tab = self._hoisted_embeddings(est, t_all[:, 0].contiguous(), condition, un_cond, Bw, dev)
            for i in range(len(rev)):
                pred, pred_uncond, pred_var = self._predict(x_t, t_all[i], condition, self_cond, guidance_scale, un_cond,
                                                            emb=None if emb_tab is None else (emb_tab[0], i, emb_tab[1], emb_tab[2], emb_tab[3]), win=win, guide=guide,
                                                            step=i)
                noise.draw(tuple(x_t.shape), out=n_post)          # gaussian_scheduler.py:99 -- drawn on every iteration (Q3)
                ddim = recs[i].mode == 1
                if ddim:
                    noise.draw(tuple(x_t.shape), out=n_ddim)      # diffusion_pipeline.py:303
                a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None if pred_uncond is None else pred_uncond.data_ptr(),
                                  None if pred_var is None else pred_var.data_ptr(), n_post.data_ptr(), n_ddim.data_ptr() if ddim else None, 0,
                                  x_t.data_ptr(), x0.data_ptr(), None, table.data_ptr(), None, i, objective, int(bool(self.clip_x0)),
                                  float(guidance_scale), x_t.numel())
                if blend is None:
                    K.sched_step(a, outputs=(x_t, x0))
                else:
                    K.sched_step_blend(a, blend, outputs=(x_t, x0))
                self_cond = x0 if self.use_self_conditioning else None  # only None-ness matters downstream (Q11)
                if trace is not None:
                    trace.append((x0.clone(), x_t.clone()))
                if progress_cb is not None:
                    progress_cb(i + 1, len(rev))
        if decode and self.latent_embedder is not None:
            x_t = self.latent_embedder.decode(x_t)
        return x_t

    def _hoisted_embeddings(self, est, t_steps, condition, un_cond, B, dev):
        """All timesteps of a loop are known before it starts: the embedding path leaves the loop (UNet.precompute_embeddings; bit-identical
        to evaluating it per iteration).  -> (table, columns of `condition`, columns of `un_cond`) or None when the estimator cannot."""
        if not (self.hoist_embeddings and hasattr(est, "can_precompute_embeddings") and est.can_precompute_embeddings()):
            return None
        has_c = est.cond_embedder is not None
        used = set()   # labels that occur in this loop (one host read before the loop starts)
        for lab in (condition, un_cond):
            if has_c and lab is not None:
                used.update(int(v) for v in lab.reshape(-1).tolist())
        tab = est.precompute_embeddings(t_steps, classes=used if has_c else None)
        cc, cu = est.embedding_columns(condition if has_c else None, B, dev, tab), est.embedding_columns(un_cond if has_c else None, B, dev, tab)
        return (tab, cc, cu, torch.cat([cu, cc]))   # (the last: columns of the 2B-row classifier-free-guidance pair, un-guided rows first)

    def _denoise_graph(self, x_t, rev, recs, table, condition, guidance_scale, un_cond, use_ddim, noise, objective, cmdlist=False, progress_cb=None,
                       blend=None, solver=None, win=None, guide=None):
        """The loop body as ONE captured hipGraph replayed `steps` times (BASELINE.json configs[3]) -- or, cmdlist=True, recorded by the
        library while it runs once and re-issued from C (mf_cmdlist_*: the native command list of the loop body).  Everything the
        reference reads on the host each iteration (t, alphas_cumprod[t], the t==0 test, the RNG state) is indexed by a
        DEVICE step counter: `t` is broadcast from a device table, the scheduler scalars come from the MfSchedStep table,
        the Philox draw index is draw_base + stride*step, and the graph advances the counter itself.  The last DDIM
        iteration still fills the (unused) DDIM noise buffer: counter-based draws do not shift any other draw.
        solver = (x_0 history or None, MfSolverTraj or None, MfSolverNoise or None, its draw buffer or None): `table` holds MfSolverStep rows and the
        tail of an iteration is mf_solver_step_f32 (mf_solver_step_traj_f32 with a trajectory, whose slot the same counter indexes), which reads
        the counter, advances it and draws nothing -- or, for a stochastic sampler, mf_solver_step_noise_f32, whose draw index the same counter
        advances (draw base + step, inside the launch; through the buffer and one more launch where the in-launch form does not apply).
        win: a WindowPlan -- x_t is the canvas, `condition` / `un_cond` come with B * M rows (_denoise repeated them), and so do t and the hoisted
        embedding columns; the crop and the merge are two more recorded launches of the body (_predict)."""
        from .noise import PhiloxDeviceNoise

        if (solver is None or solver[2] is not None) and not isinstance(noise, PhiloxDeviceNoise):
            raise RuntimeError("use_graph=True needs the device Philox noise source (a host generator cannot be captured)")
        dev, B = x_t.device, x_t.shape[0]
        t_table = torch.tensor(rev, dtype=torch.float32, device=dev)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)    # (step, ticket word of the fused tail launch)
        step_dev = counter[:1]
        Bw = B if win is None else B * win.M
        t_cur = torch.zeros(Bw, dtype=torch.float32, device=dev)   # (filled per iteration only when the estimator reads t: not with hoisted embeddings)
        n_post, n_ddim, x0 = (None, None, None) if solver is not None else (torch.empty_like(x_t), torch.empty_like(x_t), torch.empty_like(x_t))
        if solver is not None and self.use_self_conditioning:
            x0 = torch.empty_like(x_t)
        stride = 0 if solver is not None else 2 if use_ddim else 1
        base = noise.draw_index  # draws consumed so far (x_T)
        drawn = stride * len(rev) if solver is None else (len(rev) - 1 if solver[2] is not None else 0)   # (a stochastic sampler: all but the last iteration)
        clip, g = int(bool(self.clip_x0)), float(guidance_scale)

        emb_tab = self._hoisted_embeddings(self._estimator(), t_table, condition, un_cond, Bw, dev)
        emb = None if emb_tab is None else (emb_tab[0], step_dev, emb_tab[1], emb_tab[2], emb_tab[3])   # rows of iteration *step_dev, gathered on the device

        # the tail of an iteration -- posterior draw, DDIM draw, scheduler step, counter += 1 -- as ONE launch (mf_sched_step_philox_f32: the same
        # Philox quads and the same scheduler arithmetic, bit for bit), unless MEDFUSION_LOOP_TAIL=0 (A/B) or the latent is not a whole
        # number of quads per sample
        fused_tail = os.environ.get("MEDFUSION_LOOP_TAIL", "1") != "0" and (x_t.numel() // B) % 4 == 0 and (blend is None or blend.cells % 4 == 0)

        def step(a):   # (the un-fused scheduler step, with the inpainting select when there is one)
            if blend is None:
                K.sched_step(a, outputs=(x_t, x0))
            else:
                K.sched_step_blend(a, blend, outputs=(x_t, x0))

        def solver_tail(pred, pred_uncond):
            if solver[3] is not None:   # (a stochastic sampler whose draw cannot be made inside the step's launch)
                noise.draw_indexed(solver[3], base, 1, step_dev)
            self._solver_launch(self._solver_args(x_t, pred, pred_uncond, x0, solver[0], table, objective, g, counter=counter), blend, solver[1], (x_t, x0), solver[2])

        def body():
            if emb is None:   # (with the embedding rows hoisted out of the loop the estimator never reads t)
                K.broadcast_from_table(t_table, step_dev, t_cur)
            pred, pred_uncond, pred_var = self._predict(x_t, t_cur, condition, None if not self.use_self_conditioning else x0, g, un_cond, emb=emb, win=win,
                                                        guide=guide, step=step_dev)
            if solver is not None:
                solver_tail(pred, pred_uncond)
                return pred
            if fused_tail:
                a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None if pred_uncond is None else pred_uncond.data_ptr(),
                                  None if pred_var is None else pred_var.data_ptr(), None, None, 0, x_t.data_ptr(), x0.data_ptr(), None, table.data_ptr(),
                                  step_dev.data_ptr(), 0, objective, clip, g, x_t.numel())
                if blend is None:
                    K.sched_step_philox(a, noise._seed, base, stride, noise.sample_offset, B, counter, outputs=(x_t, x0))
                else:
                    K.sched_step_philox_blend(a, blend, noise._seed, base, stride, noise.sample_offset, B, counter, outputs=(x_t, x0))
                return pred
            noise.draw_indexed(n_post, base, stride, step_dev)
            if use_ddim:
                noise.draw_indexed(n_ddim, base + 1, stride, step_dev)
            a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None if pred_uncond is None else pred_uncond.data_ptr(),
                              None if pred_var is None else pred_var.data_ptr(), n_post.data_ptr(), n_ddim.data_ptr() if use_ddim else None, 0,
                              x_t.data_ptr(), x0.data_ptr(), None, table.data_ptr(), step_dev.data_ptr(), 0, objective, clip, g, x_t.numel())
            step(a)
            K.counter_add(step_dev, 1)
            return pred  # keep alive until the end of capture

        def first_iteration():
            # Q11: with self-conditioning the first call sees self_cond=None -> run it eagerly in that form
            if self.use_self_conditioning:
                if emb is None:
                    K.broadcast_from_table(t_table, step_dev, t_cur)
                pred, pu, pv = self._predict(x_t, t_cur, condition, None, g, un_cond, emb=emb, guide=guide, step=step_dev)
                if solver is not None:
                    solver_tail(pred, pu)
                    return
                noise.draw_indexed(n_post, base, stride, step_dev)
                if use_ddim:
                    noise.draw_indexed(n_ddim, base + 1, stride, step_dev)
                a = L.MfSchedArgs(x_t.data_ptr(), pred.data_ptr(), None if pu is None else pu.data_ptr(), None if pv is None else pv.data_ptr(),
                                  n_post.data_ptr(), n_ddim.data_ptr() if use_ddim else None, 0, x_t.data_ptr(), x0.data_ptr(), None, table.data_ptr(),
                                  step_dev.data_ptr(), 0, objective, clip, g, x_t.numel())
                step(a)
                K.counter_add(step_dev, 1)
            else:
                body()  # eager warm-up iteration 0: sizes every workspace / packs weights on THIS stream

        if cmdlist:
            # the native command list: iteration 0 eager (weights packed, workspaces sized, kernel attributes set), iteration 1 recorded
            # while it runs -- inside a private memory pool, so that every buffer the recorded launches point at stays reserved, what a
            # graph capture's pool does -- and iterations 2 .. re-issued from C on the same stream
            lib = L.load()
            cur = K.stream(dev.index)
            first_iteration()
            if progress_cb is not None:
                progress_cb(1, len(rev))
            if len(rev) > 1:
                pool = _CMD_POOLS.get((dev.index, cur))    # one pool per (device, stream): two threads driving two streams record independently
                if pool is None:
                    pool = _CMD_POOLS[(dev.index, cur)] = torch.cuda.MemPool()
                handle = ctypes.c_void_p()
                guard = _PureLaunchGuard()
                grew = K.scratch_growth_count()
                try:
                    with torch.cuda.use_mem_pool(pool, device=dev), guard:
                        L.check(lib.mf_cmdlist_begin(), "mf_cmdlist_begin")
                        try:
                            keep = body()
                        finally:
                            L.check(lib.mf_cmdlist_end(ctypes.byref(handle)), "mf_cmdlist_end")
                except BaseException:
                    if handle:
                        lib.mf_cmdlist_free(handle)   # (body() raised while recording: the list is dropped with it)
                    raise
                try:
                    self.last_cmdlist_launches = lib.mf_cmdlist_count(handle)
                    self.last_cmdlist_foreign_ops = sorted(set(guard.foreign))
                    if K.scratch_growth_count() != grew:
                        # the workspace or the split-K counters GREW during the recorded iteration (it needed more scratch than iteration 0):
                        # launches recorded before the growth point at the released buffer -- the list is not replayable
                        guard.foreign.append("medfusion_amd: scratch growth inside the recorded iteration")
                        self.last_cmdlist_foreign_ops = sorted(set(guard.foreign))
                    if guard.foreign:
                        # torch itself put device work into the iteration (self-conditioning, an attention variant, ...): the recorded list
                        # is not the whole iteration -- drop it and run the remaining iterations through Python (same bits, host-bound)
                        self.last_cmdlist_launches = 0
                        for k in range(2, len(rev)):
                            body()
                            if progress_cb is not None:
                                progress_cb(k + 1, len(rev))
                    elif len(rev) > 2:
                        left = len(rev) - 2
                        if self.time_cmdlist and left > 1:   # measurement aid (scripts/enqueue_time.py): the host cost of ONE replayed
                            import time                       # iteration with an empty queue in front of it
                            torch.cuda.synchronize(dev)
                            t0 = time.perf_counter()
                            L.check(lib.mf_cmdlist_replay(handle, 1, cur), "mf_cmdlist_replay")
                            self.last_cmdlist_host_ms = (time.perf_counter() - t0) * 1e3
                            left -= 1
                        if progress_cb is None:
                            L.check(lib.mf_cmdlist_replay(handle, left, cur), "mf_cmdlist_replay")
                        else:   # the same launches in slices of ~5 % of the loop, the callback between them
                            chunk, done = max(1, len(rev) // 20), len(rev) - left
                            progress_cb(done, len(rev))
                            while left > 0:
                                k = min(chunk, left)
                                L.check(lib.mf_cmdlist_replay(handle, k, cur), "mf_cmdlist_replay")
                                left, done = left - k, done + k
                                progress_cb(done, len(rev))
                finally:
                    lib.mf_cmdlist_free(handle)    # (the kernarg bytes were copied at every launch)
                del keep
            noise.draw_index = base + drawn
            return
        side = _GRAPH_STREAMS.get(dev.index)      # ONE capture stream per device (per-stream workspaces / split-K counters stay bounded)
        if side is None:
            side = _GRAPH_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            K.SyncWords.reset(dev)    # (the counters of THIS stream: _denoise reset those of the caller's stream)
            first_iteration()
            if progress_cb is not None:
                progress_cb(1, len(rev))
            done = 1
            if len(rev) > done:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    keep = body()
                chunk = max(1, len(rev) // 20)
                for k in range(done, len(rev)):
                    graph.replay()
                    if progress_cb is not None and ((k + 1) % chunk == 0 or k + 1 == len(rev)):
                        progress_cb(k + 1, len(rev))
                del keep
        torch.cuda.current_stream(dev).wait_stream(side)
        noise.draw_index = base + drawn

    @torch.no_grad()
    def sample(self, num_samples, img_size, condition=None, noise: Optional[NoiseSource] = None, shard=None, **kwargs):
        """diffusion_pipeline.py:312-317.  `shard=(rank, world)`: this process generates rows
        [rank*num_samples/world, (rank+1)*num_samples/world) of the global batch (condition/un_cond are global).
        window= / window_stride= / window_weight= (see denoise): `img_size` is the CANVAS, a latent larger than the trained size; draw #0 has its
        shape and the whole canvas is decoded in one latent_embedder.decode call."""
        self._check_sampler(kwargs.get("sampler"), kwargs.get("spacing"), kwargs.get("use_ddim", True), kwargs.get("cold_diffusion", False))
        self._check_window(tuple(img_size)[1:], kwargs)
        self._check_guide(kwargs, condition, kwargs.get("steps"), kwargs.get("use_ddim", True))
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("medfusion_amd.DiffusionPipeline.sample: move the pipeline to a ROCm device first (no CPU fallback)")
        lo, hi = 0, num_samples
        if shard is not None:
            from .dist import shard_rows

            lo, hi = shard_rows(num_samples, shard[0], shard[1])
            if condition is not None:
                condition = condition[lo:hi]
            if kwargs.get("un_cond") is not None:
                kwargs["un_cond"] = kwargs["un_cond"][lo:hi]
        if noise is None:
            noise = default_noise()
        if hi == lo:   # more ranks than samples: this rank's shard is empty -- no launch, the gather pads it (dist.gather_images)
            empty = torch.empty((0, *img_size), dtype=torch.float32, device=dev)
            if kwargs.get("decode", True) and self.latent_embedder is not None:
                return self.latent_embedder.decode(empty)
            return empty
        with torch.cuda.device(dev):   # launches go to the CURRENT device's stream: make the pipeline's device current for the call
            noise.begin(hi - lo, dev, sample_offset=lo, global_batch=num_samples)
            x_T = noise.draw((hi - lo, *img_size))  # noise_scheduler.x_final(template): draw #0 (Q3)
            return self.denoise(x_T, condition=condition, noise=noise, **kwargs)

    @staticmethod
    def _strength_span(steps: int, strength: float):
        """-> (s, k): iterations s .. steps-1 of the full loop run, k = steps - s = min(steps, int(strength * steps + 0.5)) of them"""
        if not (isinstance(strength, (int, float)) and 0 < strength <= 1):
            raise ValueError(f"strength={strength!r}: 0 < strength <= 1")
        k = min(steps, int(strength * steps + 0.5))
        if k < 1:
            raise ValueError(f"strength={strength} of {steps} iterations rounds to none: at least one iteration must run")
        return steps - k, k

    def _cell_mask(self, mask, latent_shape, image_shape):
        """-> (uint8 [B,1,cells...] on the device, True when `mask` came at image resolution).  1 / True = regenerate.  A mask at latent resolution is
        used as is (> 0.5 if floating point); one at image resolution is reduced by max over each cell's pixels (K.mask_maxpool)."""
        lat = (latent_shape[0], 1, *latent_shape[2:])
        img = None if image_shape is None else (image_shape[0], 1, *image_shape[2:])
        shape = tuple(mask.shape)
        if shape == lat:
            m = (mask > 0.5) if mask.is_floating_point() else (mask != 0)
            return m.to(torch.uint8).contiguous(), False
        if img is not None and shape == img:
            factors = [a // b for a, b in zip(img[2:], lat[2:])]
            if any(a != b * f for a, b, f in zip(img[2:], lat[2:], factors)):
                raise ValueError(f"mask {shape}: the image is not a whole number of latent cells")
            return K.mask_maxpool(mask, factors), True
        raise ValueError(f"mask of shape {shape}: expected the latent's cells {lat}" + ("" if img is None else f" or the image's pixels {img}"))

    @torch.no_grad()
    def sample_from(self, x, strength, condition=None, *, mask=None, is_latent=False, steps=None, use_ddim=True, noise: Optional[NoiseSource] = None,
                    encode_noise: Optional[NoiseSource] = None, composite=False, shard=None, decode=True, trace=None, loop=None, use_graph=None,
                    progress_cb=None, guidance_scale=1.0, un_cond=None, sampler=None, spacing=None, window=None, window_stride=None, window_weight="tent",
                    guidance_rescale=0.0, dynamic_threshold=None, threshold_max=None, guidance_schedule=None, **kwargs):
        """Image-conditioned sampling: img2img (variations of `x` at a chosen `strength`) and, with `mask`, inpainting.  A composition of the
        reference's own functions -- the training front end (diffusion_pipeline.py:84-90), GaussianNoiseScheduler.estimate_x_t
        (gaussian_scheduler.py:61-77) and the LAST k iterations of denoise's loop (:278-310):
          timesteps / rev / step records as denoise builds them on the FULL list; k = min(steps, int(strength * steps + 0.5)) iterations run,
          i = s .. steps-1 with s = steps - k;
          z0 = x (is_latent=True), else latent_embedder.encode(x) (its draw comes from `encode_noise`, a source of its own) and 2 z0 - 1 with
          do_input_centering;
          draw #0 = eps0 (where sample()'s x_T draw stands), then the loop's draws unchanged: 2k draws with DDIM, 1 + k without;
          x = estimate_x_t(z0, rev[s], eps0), then iterations s .. steps-1;
          mask (1 / True = regenerate, 0 / False = keep; one value per latent cell, broadcast over channels; at image resolution it is reduced
          by max over each cell's pixels): after iteration i the kept cells take estimate_x_t(z0, rev[i+1], eps0) -- the SAME eps0, no extra
          draw -- and z0 itself after the last iteration, inside the scheduler step's launch (all three loop forms).
        Returns the decoded latent like sample() (or the latent with decode=False); composite=True (image input and image-resolution mask only)
        returns where(mask, decoded, x).  shard=(rank, world) slices x, mask and the conditions (global batch in, this rank's rows out), the
        Philox source keeps the global sample index.  NB: VAE.encode begins its own noise source at row 0, so with a stochastic embedder a
        sharded caller encodes first and passes latents (the codebook embedders draw nothing and shard as they are).
        cold_diffusion=True raises ValueError; `eta` raises TypeError like everywhere.
        sampler= / spacing= as in denoise(): the few-step samplers on the EXECUTED grid -- the same strength rule picks the last k of its
        iterations, the first of them is first-order, the kept cells take the known latent at the next timestep of that grid; eps0 is the only
        draw of a deterministic sampler, a stochastic one ("ddim1", "dpmpp2m_sde") adds one draw per non-final iteration (k draws in all).
        window= / window_stride= / window_weight= as in denoise(): the input's latent is the canvas; eps0, the mask's select and the decode are
        canvas-sized and unchanged, so the kept cells still end as z0 exactly.
        guidance_rescale= / dynamic_threshold= / threshold_max= / guidance_schedule= as in denoise(): a schedule has one entry per EXECUTED
        iteration (the k that the strength leaves); the stage changes the prediction only, so the kept cells still end as z0 exactly."""
        if "eta" in kwargs:
            raise TypeError("forward() got an unexpected keyword argument 'eta'")
        if kwargs.pop("cold_diffusion", False):
            raise ValueError("cold_diffusion is not built for sample_from")
        if kwargs:
            raise TypeError(f"forward() got an unexpected keyword argument '{next(iter(kwargs))}'")
        self._check_sampler(sampler, spacing, use_ddim, False)
        if window is not None or window_stride is not None:   # (the latent's extents, known before the encoder runs)
            emb, canvas = self.latent_embedder, tuple(x.shape[2:])
            if not is_latent and emb is not None:
                canvas = tuple(a // b for a, b in zip(canvas, getattr(emb, "scale3", None) or (emb.scale,) * len(canvas)))
            self._window_plan(canvas, window, window_stride, window_weight)
        sch = self.noise_scheduler
        timesteps, _ = sch.loop_timesteps(steps, use_ddim, spacing)
        asked, steps = steps, len(timesteps)
        s, k = self._strength_span(steps, strength)
        guide_kw = dict(guidance_rescale=guidance_rescale, dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, guidance_schedule=guidance_schedule)
        spec, _ = self._guide_spec(dict(guide_kw, guidance_scale=guidance_scale), condition, list(reversed(timesteps))[s:])
        guide_kw = guide_kw if spec is not None else {}   # (every argument at its default: the loop is called as it always was)
        if composite and (is_latent or mask is None):
            raise ValueError("composite=True needs an image input and an image-resolution mask")
        if not x.is_cuda:
            raise RuntimeError("medfusion_amd.DiffusionPipeline runs on a ROCm device only (no CPU fallback)")
        dev = x.device
        if shard is not None:
            from .dist import shard_rows

            lo, hi = shard_rows(x.shape[0], shard[0], shard[1])
        else:
            lo, hi = 0, x.shape[0]
        n_global = x.shape[0]
        x = x[lo:hi]
        if mask is not None:
            if mask.shape[0] != n_global:
                raise ValueError(f"mask of shape {tuple(mask.shape)}: one mask per sample ({n_global})")
            mask = mask[lo:hi].to(dev)
        if condition is not None:
            condition = condition[lo:hi]
        if un_cond is not None:
            un_cond = un_cond[lo:hi]
        if hi == lo:   # more ranks than samples: this rank's shard is empty -- no launch, like sample()
            empty, emb = x.to(torch.float32), self.latent_embedder
            if is_latent:
                return emb.decode(empty) if (decode and emb is not None) else empty
            if decode or emb is None:
                return empty
            f = getattr(emb, "scale3", None) or (emb.scale,) * (x.dim() - 2)
            return empty.new_empty((0, emb.emb_channels, *(a // b for a, b in zip(x.shape[2:], f))))
        with torch.cuda.device(dev):
            x = x.to(torch.float32).contiguous()
            if is_latent:
                z0 = x
            else:
                z0 = x if self.latent_embedder is None else self.latent_embedder.encode(x, noise=encode_noise)
                if self.do_input_centering:   # 2 * x_0 - 1 (diffusion_pipeline.py:90), rounded like the reference's two operations
                    two = torch.full((z0.shape[0],), 2.0, dtype=torch.float32, device=dev)
                    z0 = K.rows_axpby(z0, two, torch.ones_like(z0), torch.full_like(two, -1.0))
            z0 = z0.contiguous()
            cmask, at_image = (None, False) if mask is None else self._cell_mask(mask, z0.shape, None if is_latent else x.shape)
            if composite and not at_image:
                raise ValueError("composite=True needs an image input and an image-resolution mask")
            if noise is None:
                noise = default_noise()
            noise.begin(hi - lo, dev, sample_offset=lo, global_batch=n_global)
            eps0 = noise.draw(tuple(z0.shape))                                   # draw #0
            rev = list(reversed(timesteps))
            x_t = sch.estimate_x_t(z0, torch.full((z0.shape[0],), int(rev[s]), dtype=torch.long), noise=eps0)
            blend = None if cmask is None else (z0, eps0, cmask)
            # (the loop rebuilds the grid from the step count: the log-SNR grid of `asked` steps is not the one of len(timesteps) steps)
            out = self._denoise_guarded(x_t, asked if sampler is not None else steps, condition, use_ddim, noise, trace, decode, use_graph, loop, progress_cb,
                                        s, blend, dict(guidance_scale=guidance_scale, un_cond=un_cond, sampler=sampler, spacing=spacing, window=window,
                                                       window_stride=window_stride, window_weight=window_weight, **guide_kw))
            if composite:
                pix = (mask > 0.5) if mask.is_floating_point() else (mask != 0)
                out = K.select_cells(pix.to(torch.uint8).contiguous(), out, x)
            return out

    # ------------------------------------------------------------------ inversion and counterfactual editing
    def _input_latent(self, x, is_latent, encode_noise):
        """x -> z0 as sample_from makes it: the latent itself, or latent_embedder.encode(x) and 2 z0 - 1 with do_input_centering"""
        x = x.to(torch.float32).contiguous()
        if is_latent:
            return x
        z0 = x if self.latent_embedder is None else self.latent_embedder.encode(x, noise=encode_noise)
        if self.do_input_centering:   # 2 * x_0 - 1 (diffusion_pipeline.py:90), rounded like the reference's two operations
            two = torch.full((z0.shape[0],), 2.0, dtype=torch.float32, device=x.device)
            z0 = K.rows_axpby(z0, two, torch.ones_like(z0), torch.full_like(two, -1.0))
        return z0.contiguous()

    def _inversion_args(self, who, steps, sampler, spacing, strength, kwargs):
        """the argument rules invert() and edit() share, checked before anything touches the device -> (timesteps, k)"""
        if "eta" in kwargs:
            raise TypeError("forward() got an unexpected keyword argument 'eta'")
        if any(k in kwargs for k in self.WINDOW_KEYS):
            raise ValueError(f"window= is not built for {who}: an inversion's trajectory is not carried through the windows (out of scope)")
        if kwargs.pop("cold_diffusion", False):
            raise ValueError(f"cold_diffusion is not built for {who}")
        if kwargs:
            raise TypeError(f"forward() got an unexpected keyword argument '{next(iter(kwargs))}'")
        if sampler is None or sampler in GaussianNoiseScheduler.STOCHASTIC_SAMPLERS:
            raise ValueError(f"{who} needs a deterministic sampler ('ddim0' or 'dpmpp2m'): the stochastic loop has no upward form")
        self._check_sampler(sampler, spacing, True, False)
        timesteps, _ = self.noise_scheduler.loop_timesteps(steps, True, spacing)
        _, k = self._strength_span(len(timesteps), strength)
        if k < 2:
            raise ValueError(f"strength={strength} of {len(timesteps)} iterations spans one grid point: an inversion runs at least one upward iteration")
        return timesteps, k

    @staticmethod
    def _quiet_noise(noise, B, dev):
        """the source the solver loops carry and never draw from: the caller's, or a fixed-key one (taking no key from torch's generator)"""
        if noise is None:
            from .noise import PhiloxDeviceNoise
            noise = PhiloxDeviceNoise(0)
            noise.begin(B, dev)
        elif not hasattr(noise, "draw_index"):
            noise.begin(B, dev)
        return noise

    def _invert_latent(self, z0, k, steps, sampler, spacing, condition, guidance_scale, un_cond, noise, trace, loop, use_graph, progress_cb, guide_kw=None):
        """the k - 1 upward iterations from z0 -> (latent at ts[k-1], trajectory buffer [k + 1][...]).  The buffer's slots 0 AND 1 hold z0, slot
        j + 1 the latent at ts[j]: the upward step j records slot 2 + j, and the downward loop of edit() -- whose step i produces the latent at
        ts[k-2-i], and z0 once more on its last iteration -- keeps from slot k - 1 - i, both linear in the device step counter."""
        traj = torch.empty((k + 1, *z0.shape), dtype=torch.float32, device=z0.device)
        traj[0].copy_(z0)
        traj[1].copy_(z0)
        tr = L.MfSolverTraj(traj.data_ptr(), None, 0, 0, L.TRAJ_RECORD, 2, 1, k + 1, 0)
        top = self._denoise_guarded(z0, steps, condition, True, noise, trace, False, use_graph, loop, progress_cb, 0, None,
                                    dict(guidance_scale=guidance_scale, un_cond=un_cond, sampler=sampler, spacing=spacing, **(guide_kw or {})), traj=tr, up=k)
        return top, traj

    @torch.no_grad()
    def invert(self, x, condition=None, *, steps=None, sampler="ddim0", spacing=None, strength=1.0, is_latent=False, guidance_scale=1.0, un_cond=None,
               loop=None, use_graph=None, progress_cb=None, trace=None, return_trajectory=False, encode_noise: Optional[NoiseSource] = None,
               noise: Optional[NoiseSource] = None, guidance_rescale=0.0, dynamic_threshold=None, threshold_max=None, guidance_schedule=None, **kwargs):
        """DDIM inversion: the probability-flow ODE of a deterministic sampler carried UPWARD from a given image (or latent) to its noise code.
        A composition of the reference's own functions: the training front end (diffusion_pipeline.py:84-90) for z0, then per iteration
        forward()'s x_0 / x_T estimates at ts[j] and, for "ddim0", GaussianNoiseScheduler.estimate_x_t(x_0_est, ts[j+1], x_T=x_T_est)
        (gaussian_scheduler.py:61-77); "dpmpp2m" takes the 2M rows with negative h (GaussianNoiseScheduler.inversion_records).
          ts = the EXECUTED grid of (steps, spacing), ascending; k = min(len, int(strength * len + 0.5)) grid points are covered (the strength
          rule of sample_from), k - 1 iterations run, z0 is taken as the state at ts[0]; the result is the latent at ts[k-1].
          return_trajectory=True: also [k][...], the latents at ts[0] .. ts[k-1] (slot 0 is z0).
        All three loop forms (the replayed ones from 4 iterations on), hoisted embeddings of the ascending timesteps, guidance as in denoise().
        Nothing is drawn: `noise` (optional) is carried, its draw_index unchanged; without it torch's generator is not advanced either (the
        encoder's draw comes from `encode_noise`, as in sample_from).  sampler=None and cold_diffusion=True raise ValueError, `eta` TypeError.
        guidance_rescale= / dynamic_threshold= / threshold_max= / guidance_schedule= as in denoise(); a schedule has one entry per executed UPWARD
        iteration (k - 1 of them, at ts[0] .. ts[k-2])."""
        timesteps, k = self._inversion_args("invert", steps, sampler, spacing, strength, kwargs)
        guide_kw = dict(guidance_rescale=guidance_rescale, dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, guidance_schedule=guidance_schedule)
        if self._guide_spec(dict(guide_kw, guidance_scale=guidance_scale), condition, list(timesteps[:k - 1]))[0] is None:
            guide_kw = {}
        if not x.is_cuda:
            raise RuntimeError("medfusion_amd.DiffusionPipeline runs on a ROCm device only (no CPU fallback)")
        with torch.cuda.device(x.device):
            z0 = self._input_latent(x, is_latent, encode_noise)
            noise = self._quiet_noise(noise, z0.shape[0], z0.device)
            top, traj = self._invert_latent(z0, k, steps, sampler, spacing, condition, guidance_scale, un_cond, noise, trace, loop, use_graph, progress_cb, guide_kw)
            return (top, traj[1:]) if return_trajectory else top

    @torch.no_grad()
    def edit(self, x, target_condition, *, source_condition=None, strength=1.0, steps=None, sampler="ddim0", spacing=None, guidance_scale=1.0,
             source_guidance_scale=1.0, un_cond=None, mask=None, composite=False, is_latent=False, decode=True, return_map=False, loop=None, use_graph=None,
             progress_cb=None, encode_noise: Optional[NoiseSource] = None, noise: Optional[NoiseSource] = None, guidance_rescale=0.0,
             source_guidance_rescale=0.0, dynamic_threshold=None, threshold_max=None, guidance_schedule=None, source_guidance_schedule=None, **kwargs):
        """Counterfactual editing: "this image, as the model would draw it under `target_condition`".  invert() under `source_condition` /
        `source_guidance_scale`, recording the trajectory; then the LAST k iterations of the deterministic sampler's loop (denoise's, from
        iteration len - k) from the inverted latent under `target_condition` / `guidance_scale`.  Nothing is drawn.
          mask (the conventions of sample_from: 1 / True = regenerate, per latent cell or at image resolution): after every downward iteration
          the kept cells take the RECORDED latent at the timestep just produced -- the trajectory the regenerated cells left from, not a
          re-noised copy -- and z0 after the last one, inside the solver step's launch: the kept cells of the final latent are z0 bit for bit.
          composite=True (image input, image-resolution mask): where(mask, decoded, x).
          return_map=True (image input, decode=True): also [B, 1, ...], the mean over the channels of |result - x|.
        progress_cb(done, total) counts both passes: total = 2 k - 1.
        guidance_rescale= / guidance_schedule= (as in denoise()) belong to the downward pass under `target_condition`, one schedule entry per
        executed iteration (k); source_guidance_rescale= / source_guidance_schedule= are their twins for the inversion under `source_condition`
        (k - 1 entries, upward).  dynamic_threshold= / threshold_max= are ONE setting for both passes: an inversion is only the inverse of the
        sampler it is run with, so the x_0 estimate is thresholded the same way up and down."""
        timesteps, k = self._inversion_args("edit", steps, sampler, spacing, strength, kwargs)
        down_kw = dict(guidance_rescale=guidance_rescale, dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, guidance_schedule=guidance_schedule)
        up_kw = dict(guidance_rescale=source_guidance_rescale, dynamic_threshold=dynamic_threshold, threshold_max=threshold_max,
                     guidance_schedule=source_guidance_schedule)
        if self._guide_spec(dict(down_kw, guidance_scale=guidance_scale), target_condition, list(reversed(timesteps))[len(timesteps) - k:])[0] is None:
            down_kw = {}
        if self._guide_spec(dict(up_kw, guidance_scale=source_guidance_scale), source_condition, list(timesteps[:k - 1]), "source_")[0] is None:
            up_kw = {}
        if composite and (is_latent or mask is None):
            raise ValueError("composite=True needs an image input and an image-resolution mask")
        if return_map and (is_latent or not decode):
            raise ValueError("return_map=True compares the decoded result with the input image: an image input and decode=True")
        if not x.is_cuda:
            raise RuntimeError("medfusion_amd.DiffusionPipeline runs on a ROCm device only (no CPU fallback)")
        dev = x.device
        with torch.cuda.device(dev):
            x = x.to(torch.float32).contiguous()
            if mask is not None:
                if mask.shape[0] != x.shape[0]:
                    raise ValueError(f"mask of shape {tuple(mask.shape)}: one mask per sample ({x.shape[0]})")
                mask = mask.to(dev)
            z0 = self._input_latent(x, is_latent, encode_noise)
            cmask, at_image = (None, False) if mask is None else self._cell_mask(mask, z0.shape, None if is_latent else x.shape)
            if composite and not at_image:
                raise ValueError("composite=True needs an image input and an image-resolution mask")
            noise = self._quiet_noise(noise, z0.shape[0], dev)
            total = 2 * k - 1
            up_cb = None if progress_cb is None else (lambda done, _t: progress_cb(done, total))
            down_cb = None if progress_cb is None else (lambda done, _t: progress_cb(k - 1 + done, total))
            top, traj = self._invert_latent(z0, k, steps, sampler, spacing, source_condition, source_guidance_scale, un_cond, noise, None, loop, use_graph, up_cb,
                                            up_kw)
            keep = None
            if cmask is not None:
                cells = z0.numel() // (z0.shape[0] * z0.shape[1])
                keep = L.MfSolverTraj(traj.data_ptr(), cmask.data_ptr(), cells, z0.shape[1], L.TRAJ_KEEP, k - 1, -1, k + 1, 0)
                keep._keep = (traj, cmask)
            out = self._denoise_guarded(top, steps, target_condition, True, noise, None, decode, use_graph, loop, down_cb, len(timesteps) - k, None,
                                        dict(guidance_scale=guidance_scale, un_cond=un_cond, sampler=sampler, spacing=spacing, **down_kw), traj=keep)
            if composite:
                pix = (mask > 0.5) if mask.is_floating_point() else (mask != 0)
                out = K.select_cells(pix.to(torch.uint8).contiguous(), out, x)
            return (out, K.absdiff_mean_c(out, x)) if return_map else out

    # ------------------------------------------------------------------ held-out denoising loss (the reference's validation step)
    LOSSES = ("l1", "l2")

    @staticmethod
    def deep_supervision_weights(heads: int):
        """diffusion_pipeline.py:144-146: w_i = 2^-i / sum over the horizontal prediction (i = 0) and the `heads` vertical ones"""
        w = [1 / 2 ** i for i in range(1 + heads)]
        tot = sum(w)
        return [v / tot for v in w]

    def _latent_extents(self, x, is_latent):
        """the spatial extents of the latent of `x`, known before the encoder runs"""
        sp, emb = tuple(x.shape[2:]), self.latent_embedder
        if is_latent or emb is None:
            return sp
        return tuple(a // b for a, b in zip(sp, getattr(emb, "scale3", None) or (emb.scale,) * len(sp)))

    def _check_validation(self, x, t, loss, is_latent):
        """the argument rules of validation_step / denoising_profile, before anything touches the device -> the head pooling factors.  t: None, or
        the timesteps as a tensor (checked for shape and dtype; for its range where it lives on the host)"""
        if loss not in self.LOSSES:
            raise ValueError(f"loss={loss!r}: one of {self.LOSSES}")
        if not torch.is_tensor(x) or x.dtype != torch.float32 or not x.is_cuda or x.dim() not in (4, 5):
            raise ValueError("x: an fp32 [B, C, spatial...] tensor on the GPU (no CPU fallback)" +
                             (f", got {x.dtype} on {x.device} with shape {tuple(x.shape)}" if torch.is_tensor(x) else f", got {type(x).__name__}"))
        if self.estimator_objective not in ("x_T", "x_0"):
            raise ValueError("Unknown Objective")
        if t is not None:
            T = self.noise_scheduler.T
            if t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"t: an int32 or int64 tensor, got {t.dtype}")
            if tuple(t.shape) != (x.shape[0],):
                raise ValueError(f"t: one timestep per row, shape ({x.shape[0]},), got {tuple(t.shape)}")
            if not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= T):
                raise ValueError(f"t: timesteps in [0, {T}), got {int(t.min())} .. {int(t.max())}")
        sp = self._latent_extents(x, is_latent)
        factors = []
        for i, f in enumerate(getattr(self._estimator(), "head_factors", [])):
            if len(set(f)) != 1 or any(s % f[0] for s in sp):
                raise ValueError(f"x: deep-supervision head {i} is smaller than the latent {sp} by {f} per axis: the area-pooled target needs one integer factor that "
                                 "divides every side")
            factors.append(f[0])
        return factors

    def _validation_rows(self, z0, condition, t32, noise, loss, factors):
        """one estimator pass on z0 diffused to t32 with the next draw of `noise` (begun) -> per-row fp64 [B] tensors: loss, l1, l2 and, with
        estimate_variance, variance and variance_scale.  Nothing waits for the device."""
        sch, est = self.noise_scheduler, self._estimator()
        B, per = z0.shape[0], z0.numel() // z0.shape[0]
        obj_xT = self.estimator_objective == "x_T"
        draw_no = getattr(noise, "draw_index", 0)
        x_t, eps = sch.diffuse_rows(z0, t32, noise, want_eps=self.estimate_variance)
        philox = None if eps is not None else (noise._seed, draw_no, noise.sample_offset)   # (a Philox draw that was never stored)
        tl = t32.to(torch.long)
        self_cond = x_t if self.use_self_conditioning else None   # (Q11: the estimator only asks whether it is None)
        if self.estimate_variance:
            h, y_ver = est.features(x_t, tl, condition, self_cond)
            c = est.out_ch
            pred, pred_var = est.outc(h, rows=slice(0, c)), est.outc(h, rows=slice(c, 2 * c))
        else:
            (pred, y_ver), pred_var = est(x_t, tl, condition=condition, self_cond=self_cond), None
        if len(y_ver) != len(factors):
            raise RuntimeError(f"the estimator returned {len(y_ver)} deep-supervision heads, {len(factors)} expected")

        def sums(p):   # [B, 2] = (sum |d|, sum d^2) against the target, area-pooled onto p
            p = p.contiguous()
            if obj_xT and philox is not None:
                return K.denoise_loss(p, philox=philox, target_shape=z0.shape)
            return K.denoise_loss(p, target=eps if obj_xT else z0)

        k = self.LOSSES.index(loss)
        w = self.deep_supervision_weights(len(y_ver))
        hor = sums(pred) / per
        rows = {"l1": hor[:, 0], "l2": hor[:, 1]}
        total = w[0] * hor[:, k]
        if self.estimate_variance:
            tb = sch.device_tables(z0.device)
            v = K.variance_loss(z0, x_t, eps, pred.contiguous(), pred_var.contiguous(), t32, tb, 0 if obj_xT else 1, self.clip_x0) / per
            rows["variance"] = torch.where(t32 == 0, v[:, 1], v[:, 0])      # t == 0 ? nll : kl (diffusion_pipeline.py:172)
            rows["variance_scale"] = v[:, 2]
            total = total + rows["variance"]
        for i, p in enumerate(y_ver):
            if tuple(p.shape[2:]) != tuple(s // factors[i] for s in z0.shape[2:]):
                raise RuntimeError(f"deep-supervision head {i} has extents {tuple(p.shape[2:])}, the latent {tuple(z0.shape[2:])} over {factors[i]} expected")
            total = total + w[i + 1] * (sums(p)[:, k] / (p.numel() // B))
        rows["loss"] = total
        return rows

    @torch.no_grad()
    def validation_step(self, x, condition=None, *, t=None, noise: Optional[NoiseSource] = None, loss="l1", is_latent=False,
                        encode_noise: Optional[NoiseSource] = None, per_sample=False):
        """The held-out denoising loss: `_step` of the reference at state != 'train' (diffusion_pipeline.py:78-201), what it logs as val/loss,
        val/L1, val/L2 and val/variance_loss -- line by line:
          x_0 = x (is_latent=True: the model's own latent, taken as it is), else latent_embedder.encode(x) -- a VAE's sample, drawn from
          `encode_noise` as in sample_from -- and 2 x_0 - 1 with do_input_centering (:84-90);
          t: one timestep per row (:99), x_T = draw #0 of `noise`, x_t = estimate_x_t(x_0, t, x_T);
          the EMA estimator with use_ema (:102-105); ONE estimator pass (:126).  With use_self_conditioning the reference runs a first pass whose
          result only decides that self_cond is not None (Q11: the estimator then concatenates x_t itself); that pass is skipped here;
          loss = w_0 L(pred, target) + variance_loss + sum_i w_i L(head_i, area-pooled target), L = L1 (`loss="l1"`, the reference's default
          L1Loss) or MSE ("l2"), w_i = 2^-i / sum (:142-183); L1 and L2 of the horizontal prediction (:189-190).
        The reference's coin flip that drops the condition (classifier_free_guidance_dropout, :122) belongs to the caller: the method evaluates
        with the `condition` it is given, None being the unconditional pass.
        Draws: t=None takes torch.randint(0, T, (B,)) from torch's CPU default generator (one call, after the encoder's draw); then `noise` --
        a fresh PhiloxDeviceNoise when None, as in sample() -- begins and gives draw #0; draw_index == 1 afterwards.  With a device source and
        objective 'x_T' the draw is never stored: the forward process and the loss regenerate it in registers.  A HostNoise draw is uploaded.
        Every sum is a per-row fp64 sum in a fixed order (K.denoise_loss, K.variance_loss): a row's figures do not depend on the batch it is
        in.  A mean is the row's sum divided in fp64, a batch mean the mean of the row means.  Returns 0-dim fp64 device tensors `loss`, `L1`,
        `L2` (+ `variance_loss`, `variance_scale` with estimate_variance); per_sample=True adds the [B] tensors `loss_rows`, `l1_rows`, `l2_rows`
        (+ `variance_rows`) and the `t` used (int64).  The method never waits for the device.
        ValueError, naming the argument, before anything touches the device: t of the wrong shape or dtype, or -- where t lives on the host --
        outside [0, T); an unknown loss; x not fp32 or not on the GPU; a deep-supervision head whose side does not divide the latent's."""
        if t is not None and not torch.is_tensor(t):
            t = torch.as_tensor(t)
        factors = self._check_validation(x, t, loss, is_latent)
        dev, B = x.device, x.shape[0]
        with torch.cuda.device(dev):
            z0 = self._input_latent(x, is_latent, encode_noise)
            if t is None:
                t = torch.randint(0, self.noise_scheduler.T, (B,))
            t32 = t.to(device=dev, dtype=torch.int32)
            if noise is None:
                noise = default_noise()
            noise.begin(B, dev)
            rows = self._validation_rows(z0, condition, t32, noise, loss, factors)
        out = {"loss": rows["loss"].mean(), "L1": rows["l1"].mean(), "L2": rows["l2"].mean()}
        if self.estimate_variance:
            out["variance_loss"], out["variance_scale"] = rows["variance"].mean(), rows["variance_scale"].mean()
        if per_sample:
            out.update(loss_rows=rows["loss"], l1_rows=rows["l1"], l2_rows=rows["l2"], t=t32.to(torch.long))
            if self.estimate_variance:
                out["variance_rows"] = rows["variance"]
        return out

    @torch.no_grad()
    def denoising_profile(self, x, condition=None, *, timesteps=None, draws=1, noise: Optional[NoiseSource] = None, loss="l1", is_latent=False, batch=None):
        """The denoising loss of every image at every listed timestep: validation_step's figures per (timestep, image), averaged over `draws`
        draws -> {"t": [K] int64, "loss": [K, N], "L1": [K, N], "L2": [K, N], "score": [N]} as CPU fp64 tensors; score is an image's loss averaged
        over the timesteps (how well the model explains it: large = unusual).  timesteps: default the 20-point log-SNR grid
        loop_timesteps(20, True, "logsnr").  The input is encoded ONCE; then for timestep k and draw d every image is diffused with draw number
        k * draws + d of `noise` (rows keep their index in x, so `batch` -- rows per estimator pass, default all -- does not change a figure) and
        evaluated as validation_step(t = timesteps[k]) evaluates it.  One host sync, at the end."""
        sch = self.noise_scheduler
        if timesteps is None:
            timesteps = sch.loop_timesteps(20, True, "logsnr")[0]
        ts = [int(v) for v in timesteps]
        if not ts or any(v < 0 or v >= sch.T for v in ts):
            raise ValueError(f"timesteps: a non-empty list of timesteps in [0, {sch.T}), got {ts}")
        if not (isinstance(draws, int) and draws >= 1):
            raise ValueError(f"draws={draws!r}: a positive integer")
        N = x.shape[0] if torch.is_tensor(x) else 0
        batch = N if batch is None else int(batch)
        if batch < 1:
            raise ValueError(f"batch={batch!r}: a positive integer")
        factors = self._check_validation(x, None, loss, is_latent)
        from .noise import PhiloxDeviceNoise

        dev = x.device
        with torch.cuda.device(dev):
            z0 = self._input_latent(x, is_latent, None)
            if noise is None:
                noise = default_noise()
            noise.begin(N, dev)
            device_draw = isinstance(noise, PhiloxDeviceNoise)
            acc = torch.zeros((len(ts), 3, N), dtype=torch.float64, device=dev)
            for k, tk in enumerate(ts):
                for d in range(draws):
                    eps = None if device_draw else noise.draw(tuple(z0.shape))      # (a host source draws in sequence: number k * draws + d)
                    for lo in range(0, N, batch):
                        hi = min(N, lo + batch)
                        if device_draw:   # the same key, the rows' own sample indices, draw number k * draws + d
                            src = PhiloxDeviceNoise(noise._seed)
                            src.begin(hi - lo, dev, sample_offset=noise.sample_offset + lo)
                            src.draw_index = k * draws + d
                        else:
                            src = eps[lo:hi]
                        t32 = torch.full((hi - lo,), tk, dtype=torch.int32, device=dev)
                        r = self._validation_rows(z0[lo:hi], None if condition is None else condition[lo:hi], t32, src, loss, factors)
                        acc[k, :, lo:hi] += torch.stack((r["loss"], r["l1"], r["l2"]))
            if device_draw:
                noise.draw_index = len(ts) * draws
            host = (acc / draws).cpu()                                              # the one host sync
        return {"t": torch.tensor(ts, dtype=torch.long), "loss": host[:, 0], "L1": host[:, 1], "L2": host[:, 2], "score": host[:, 0].mean(0)}

    @torch.no_grad()
    def interpolate(self, img1, img2, i=None, condition=None, lam=0.5, noise: Optional[NoiseSource] = None, **kwargs):
        """diffusion_pipeline.py:320-332: diffuse both inputs to timestep i, lerp, denoise with `i` passed as `steps`.
        NB the reference method ALWAYS raises (it forwards `clip_x0=` to estimate_x_t, which has no such parameter); this
        implements its evident intent (what oracle/restate.py restates).  `i=None` raises TypeError like the reference's
        `torch.full(shape, None)`.  Noise draws: #0 and #1 = the two x_T of estimate_x_t, then the denoise loop's."""
        assert img1.shape == img2.shape, "Image 1 and 2 must have equal shape"
        if i is None:
            raise TypeError("full() received an invalid combination of arguments - got (torch.Size, NoneType, device=torch.device)")
        if noise is None:
            noise = default_noise()
        B = img1.shape[0]
        noise.begin(B, img1.device)
        t = torch.full(img1.shape[:1], i, device=img1.device)
        sch = self.noise_scheduler
        img1_t = sch.estimate_x_t(img1, t=t, noise=noise.draw(tuple(img1.shape)))
        img2_t = sch.estimate_x_t(img2, t=t, noise=noise.draw(tuple(img2.shape)))
        a = torch.full((B,), 1 - lam, dtype=torch.float32, device=img1.device)
        c = torch.full((B,), lam, dtype=torch.float32, device=img1.device)
        img = K.rows_axpby(img1_t, a, img2_t, c)  # (1 - lam) * img1_t + lam * img2_t
        return self.denoise(img, i, condition, noise=noise, **kwargs)
