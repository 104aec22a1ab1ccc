"""Samplers.  ``EulerEDMSampler`` is the one UDiffText instantiates (reference util.py:35-45); with s_churn = 0 it
is the deterministic Euler == DDIM(eta 0) integrator with classifier-free guidance, with s_churn > 0 the stochastic
(Karras "churn") one: udt_unet_input_churn adds the step's noise in the launch that packs the UNet input.

Reference: sgm/modules/diffusionmodules/sampling.py — BaseDiffusionSampler :28-78, EDMSampler :89-98,
EulerEDMSampler :218-420 (get_init_noise :264-322, sampler_step :324-353, __call__ :355-420).

MI355X execution of one step (``_Stepper.step``): all scalars (sigma, quantised sigma, timestep index,
c_in, c_out) are computed on the host from the fp32 tables — no ``.item()`` sync in the loop; the device work is
  udt_unet_input (x*c_in into the NHWC bf16 CFG pair) -> UNet kernels -> udt_cfg_euler_step (c_out, CFG, Euler),
with the step-invariant pieces hoisted out of the loop (text k|v projections of all 16 transformers, the
concat channels of the UNet input).  Attention maps are only emitted where they are consumed (noise search).
The side paths of EulerEDMSampler — attend-and-excite (``_sample_with_attend_and_excite``, and row by row for
pipeline.predict_many ``sample_rows_with_attend_and_excite``: one schedule, ``_aae_steps``) and the ``detailed``
attention-map dump — run eager steps around the written-out reverse pass (udifftext_amd.backward).

Every sampler describes step i as a plan of UNet evaluations, each ending in ONE fused launch: ``EulerEval``
(udt_cfg_euler_step, the step above: EulerEDMSampler), ``Eval`` (udt_cfg_sampler_step: HeunEDMSampler, EulerAncestralSampler,
DPMPP2SAncestralSampler, DPMPP2MSampler, reference :140-215, :423-567) or ``MultistepEval`` (udt_cfg_multistep_step:
LinearMultistepSampler, reference :180-215; to_d and the sum over a ring of derivative buffers).  One loop (``_PlanSampler``)
runs the plans of any of them as eager launches or hipGraph replays (``_GraphedSteps``): alone, on a lane of
pipeline.predict_many, or as several batches in flight.

Preconditioning and guidance: the host scalars of an evaluation come from ``precond_coefs`` (EpsScaling, VScaling,
EDMScaling under Denoiser or DiscreteDenoiser).  EpsScaling + DiscreteDenoiser + VanillaCFG runs the udt_cfg_* launches above;
every other combination, IdentityGuider (B rows through the UNet, no pair) included, runs the udt_precond_* forms of the same
kernels, launch for launch.  Unknown denoiser / scaling / guider classes and dynamic thresholding raise.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, NamedTuple, Optional, Union

import numpy as np
import torch

from udifftext_amd import ops, packing, rng

from ...util import default, instantiate_from_config, require_gpu
from .denoiser import Denoiser, DiscreteDenoiser
from .denoiser_scaling import EDMScaling, EpsScaling, VScaling
from .guiders import IdentityGuider, VanillaCFG
from .sampling_utils import NoDynamicThresholding, to_d

DEFAULT_GUIDER = {"target": "sgm.modules.diffusionmodules.guiders.IdentityGuider"}


class BaseDiffusionSampler:
    def __init__(self, discretization_config, num_steps: Union[int, None] = None, guider_config=None,
                 verbose: bool = False, device: str = "cuda"):
        self.num_steps = num_steps
        self.discretization = instantiate_from_config(discretization_config)
        self.guider = instantiate_from_config(default(guider_config, DEFAULT_GUIDER))
        self.verbose = verbose
        self.device = device

    def prepare_sampling_loop(self, x, cond, uc=None, num_steps=None):
        sigmas = self.discretization(self.num_steps if num_steps is None else num_steps, device=self.device)
        uc = default(uc, cond)
        x *= torch.sqrt(1.0 + sigmas[0] ** 2.0)
        s_in = x.new_ones([x.shape[0]])
        return x, s_in, sigmas, len(sigmas), cond, uc

    def denoise(self, x, model, sigma, cond, uc):
        """generic (any denoiser / network) formulation, tensor math as in the reference :61-64"""
        denoised = model.denoiser(model.model, *self.guider.prepare_inputs(x, sigma, cond, uc))
        return self.guider(denoised, sigma)

    def get_sigma_gen(self, num_sigmas, init_step=0):
        gen = range(init_step, num_sigmas - 1)
        if self.verbose:
            try:
                from tqdm import tqdm
                gen = tqdm(gen, total=num_sigmas - 1 - init_step,
                           desc=f"Sampling with {self.__class__.__name__} for {num_sigmas - 1 - init_step} steps")
            except ImportError:
                pass
        return gen


class SingleStepDiffusionSampler(BaseDiffusionSampler):
    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc, *args, **kwargs):
        raise NotImplementedError

    def euler_step(self, x, d, dt):
        return x + dt * d


class EDMSampler(SingleStepDiffusionSampler):
    def __init__(self, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise


# noise search: candidates as extra batch entries of one UNet call (0: one candidate at a time)
NOISE_BATCH = os.environ.get("UDT_NOISE_BATCH", "1") != "0"
# UDT_DUAL_STREAM=1: the uc / c halves of a LONE batch's UNet call on two streams.  Default OFF since round 4: with the wide
# convolution (one 256-pixel tile per CU for the full 8-sample call) one stream is 1.5 % faster (9.60 vs 9.75 ms per step,
# profiles/r04_ab_dual_stream.txt); rounds 1-3 gained 3-8 % from the split
DUAL_STREAM = os.environ.get("UDT_DUAL_STREAM", "0") != "0"


def _all_zero(t: torch.Tensor) -> bool:
    """is the (unconditional) text context exactly zero?  GeneralConditioner tags force-zeroed embeddings on the host
    (``_udt_all_zero``); anything else is asked on the device (one host sync)"""
    flag = getattr(t, "_udt_all_zero", None)
    return bool(flag) if flag is not None else not bool(t.any())


class Precond(NamedTuple):
    """denoiser.py:23-28 for one host sigma: D(x) = c_skip*x + c_out*F(c_in*x, c_noise)"""
    c_skip: float
    c_out: float
    c_in: float
    c_noise: float                     # the network's timestep input: a table index (as a float) or a real number


def _quantise(table: torch.Tensor, value: float):
    idx = int((table - value).abs().argmin())
    return idx, float(table[idx])


def check_denoiser(denoiser) -> None:
    """raise for a denoiser or scaling class ``precond_coefs`` has no formula for (host only: no device data is read)"""
    if type(denoiser) not in (Denoiser, DiscreteDenoiser):
        raise NotImplementedError(f"the fused MI355X step implements Denoiser and DiscreteDenoiser, not {type(denoiser).__name__}")
    if type(denoiser.scaling) not in (EpsScaling, VScaling, EDMScaling):
        raise NotImplementedError(f"the fused MI355X step implements EpsScaling, VScaling and EDMScaling, not "
                                  f"{type(denoiser.scaling).__name__}")


def precond_coefs(denoiser, sigma: float, table: Optional[torch.Tensor] = None) -> Precond:
    """the host form of ``denoiser.__call__``'s scalars (reference denoiser.py:23-28), in float64 from the fp32 table entries:
    DiscreteDenoiser quantises sigma on its table (``table``: its host copy), applies the scaling, then quantises c_noise
    (EDMScaling: the nearest table entry to 0.25 ln sigma_q, as the reference does); the plain Denoiser quantises nothing and
    c_noise is a real number.  Dispatches on the EXACT denoiser and scaling class: a subclass may compute anything."""
    check_denoiser(denoiser)
    if type(denoiser) is DiscreteDenoiser:
        table = denoiser.sigmas.detach().float().cpu() if table is None else table
        s = _quantise(table, sigma)[1]
    else:
        s = float(sigma)
    scaling = denoiser.scaling
    if type(scaling) is EpsScaling:
        p = Precond(1.0, -s, 1.0 / (s * s + 1.0) ** 0.5, s)
    elif type(scaling) is VScaling:
        d = s * s + 1.0
        p = Precond(1.0 / d, -s / d ** 0.5, 1.0 / d ** 0.5, s)
    else:
        sd = float(scaling.sigma_data)
        d = s * s + sd * sd
        log_s = float(torch.log(torch.tensor(s, dtype=torch.float64)))     # (torch's log, as the reference takes it)
        p = Precond(sd * sd / d, s * sd / d ** 0.5, 1.0 / d ** 0.5, 0.25 * log_s)
    if type(denoiser) is DiscreteDenoiser and denoiser.quantize_c_noise:
        p = p._replace(c_noise=float(_quantise(table, p.c_noise)[0]))
    return p


def _table_key(denoiser):
    """the CONTENT of a DiscreteDenoiser's sigma table (None for the plain Denoiser): its bytes, read from the device once per
    (buffer, version) and kept on the denoiser object — no host synchronisation on later calls, and no address that a freed
    denoiser's successor could share"""
    sigmas = getattr(denoiser, "sigmas", None)
    if sigmas is None:
        return None
    state = (sigmas.data_ptr(), sigmas._version)
    cached = denoiser.__dict__.get("_udt_table_key")
    if cached is None or cached[0] != state:
        cached = (state, hash(sigmas.detach().float().cpu().numpy().tobytes()))
        denoiser.__dict__["_udt_table_key"] = cached
    return cached[1]


def denoiser_key(denoiser) -> tuple:
    """what the host coefficients of a run depend on — the denoiser and scaling classes, the scaling's parameters, the quantise flag
    and the sigma table's content: captured graphs bake the coefficients in, so the runner caches are keyed by it"""
    sc = denoiser.scaling
    return (type(denoiser).__name__, type(sc).__name__, tuple(sorted((k, float(v)) for k, v in vars(sc).items())),
            bool(getattr(denoiser, "quantize_c_noise", False)), _table_key(denoiser))


def weights_fingerprint(model) -> int:
    """changes whenever a parameter of ``model`` is re-assigned, moved or written in place (load_state_dict,
    init_from_ckpt, .to()): captured hipGraphs bake in the device pointers of the packed weights, so the graph caches
    are keyed by it (~1 ms for the engine's 1330 tensors, once per sampling call).  Writes through ``p.data``
    (``p.data.copy_()``, EMA swaps) do not bump ``_version`` and are not seen."""
    h = 0
    for p in model.parameters():
        h = (h * 1000003 + p._version * 8191 + p.data_ptr()) & 0xFFFFFFFFFFFFFFFF
    return h


def _is_capture_failure(e: BaseException) -> bool:
    """only 'this stream / runtime cannot capture' errors may downgrade the sampler to eager launches"""
    from udifftext_amd import lib as L
    if isinstance(e, (L.UdtError, torch.OutOfMemoryError)):
        return False
    msg = str(e).lower()
    return "captur" in msg or "graph" in msg


# ================================================================================================================== plans
# A sampler supplies per step i its ``plan``: the UNet evaluations of the step with their sigma and float64 host coefficients,
# over named fp32 NCHW buffers — "x" (the latent) and the scratch / history buffers the plans name ("t": Euler predictor /
# midpoint, "h0" / "h1": denoised history, "d0" ...: derivative ring).  Each evaluation is the CFG pair's UNet call on its source
# buffer followed by ONE fused launch.  The same plan runs as eager launches, inside one hipGraph per step index, or (tests) as
# plain torch arithmetic.


class EulerEval(NamedTuple):
    """one UNet evaluation + the in-place Euler update of src from sigma to sigma_next (udt_cfg_euler_step: _Stepper.step)"""
    sigma: float                       # sigma_hat = sigma_i*(1 + gamma_i) on a churned step, else sigma_i (unquantised)
    sigma_next: float
    src: str = "x"
    churn: float = 0.0                 # != 0: src += churn * noise[slot] before the evaluation (udt_unet_input_churn)
    maps: bool = False                 # this evaluation's UNet call also emits the character maps (udt_tattn_fused_maps)


class Eval(NamedTuple):
    """one UNet evaluation + its fused update (udt_cfg_sampler_step), with den = CFG(src + c_out*eps_u, src + c_out*eps_c),
    c_out = -quantised sigma: out = kx*src + kd*den(src, sigma) + ka*aux + kp*prev + kn*noise[step]"""
    sigma: float                       # UNQUANTISED sigma of the call (c_in, c_out and the timestep use its quantised value)
    src: str
    out: str
    kx: float = 0.0
    kd: float = 0.0
    aux: Optional[str] = None
    ka: float = 0.0
    prev: Optional[str] = None
    kp: float = 0.0
    kn: float = 0.0
    den_out: Optional[str] = None
    churn: float = 0.0                 # as EulerEval.churn (set by no sampler yet: Heun churn would be a plan change only)
    maps: bool = False                 # as EulerEval.maps


class MultistepEval(NamedTuple):
    """one UNet evaluation + the fused linear-multistep update (udt_cfg_multistep_step): d = (src - den(src, sigma))/sigma;
    out = src + (k0*d + k_1*hist_1 + ...) over ``hist`` = ((buffer, k), ...), the older derivatives newest first; d_out <- d"""
    sigma: float                       # UNQUANTISED sigma (to_d); c_in, c_out and the timestep use its quantised value
    src: str
    out: str
    d_out: str
    k0: float
    hist: tuple = ()
    maps: bool = False                 # as EulerEval.maps


def plan_buffers(plans) -> list:
    """the names of the buffers ``plans`` ((step, plan) pairs) read or write, besides the latent "x", in first-use order"""
    names = []
    for _, plan in plans:
        for e in plan:
            if isinstance(e, EulerEval):
                used = (e.src,)
            elif isinstance(e, MultistepEval):
                used = (e.src, e.out, e.d_out) + tuple(b for b, _ in e.hist)
            else:
                used = (e.src, e.out, e.aux, e.prev, e.den_out)
            names.extend(b for b in used if b and b != "x" and b not in names)
    return names


def _churn(e) -> float:
    return e.churn if isinstance(e, (EulerEval, Eval)) else 0.0


def plan_noise_slots(plans) -> Dict[int, int]:
    """step index -> slot of the run's noise buffer (draw_step_noise).  Ancestral plans (an ``Eval`` with kn != 0): one draw per
    step of ``plans``, the last step included, slot = position.  Churned plans (an evaluation with churn != 0): one draw per
    CHURNED step, the k-th churned step reads slot k; the other steps draw nothing and have no slot."""
    if any(isinstance(e, Eval) and e.kn != 0.0 for _, plan in plans for e in plan):
        return {i: k for k, (i, _) in enumerate(plans)}
    churned = [i for i, plan in plans if any(_churn(e) != 0.0 for e in plan)]
    return {i: k for k, i in enumerate(churned)}


def char_map_step(n_sigmas: int, init_step: int = 0) -> int:
    """the step whose first evaluation emits the character maps: the middle one, (n_sigmas - 1) // 2 (reference sampling.py:380);
    ValueError when the run starts behind it"""
    mid = (n_sigmas - 1) // 2
    if init_step > mid:
        raise ValueError(f"character maps are taken at step {mid} of {n_sigmas - 1}; init_step {init_step} starts behind it")
    return mid


def plans_with_char_maps(plans, n_sigmas: int, init_step: int = 0) -> list:
    """``plans`` with the first evaluation of the middle step carrying ``maps`` (captured runners are keyed by their plans: such a
    run has a runner of its own, and that step's graph holds the map-emitting launches)"""
    mid = char_map_step(n_sigmas, init_step)
    out = [(i, ((plan[0]._replace(maps=True),) + tuple(plan[1:])) if i == mid else plan) for i, plan in plans]
    assert sum(e.maps for _, plan in out for e in plan) == 1, f"step {mid} is not among the plans"
    return out


def plans_emit_maps(plans) -> bool:
    return any(e.maps for _, plan in plans for e in plan)


def plans_add_noise(plans) -> bool:
    """does an evaluation of ``plans`` read a draw (ancestral noise after the update, or churn before the evaluation)?"""
    return bool(plan_noise_slots(plans))


class _Stepper:
    """Step-invariant device state of one sampling run + the fused per-step launch sequence."""

    def __init__(self, model, cond: dict, uc: dict, batch_size: int, latent_hw, scale: float, two_streams=None, pair: bool = True):
        """pair: the CFG pair (VanillaCFG: 2B rows, uncond first); False: IdentityGuider — B rows built from ``cond`` only, no
        zero-context shortcut and no two-stream split"""
        self.engine = model
        self.unet = model.model.diffusion_model
        self.scale = float(scale)
        self.B = batch_size
        self.pair = bool(pair)
        self.rows = 2 * batch_size if self.pair else batch_size
        h, w = latent_hw
        dev = cond["concat"].device
        self.den = model.denoiser
        sigmas = getattr(self.den, "sigmas", None)
        self.table = sigmas.detach().float().cpu() if sigmas is not None else None     # ascending 1000-entry table
        # EpsScaling + DiscreteDenoiser + VanillaCFG: the udt_cfg_* launches; anything else: udt_precond_* (same count per evaluation)
        self.eps_cfg = self.pair and type(self.den) is DiscreteDenoiser and type(self.den.scaling) is EpsScaling
        ctx = torch.cat((uc["t_crossattn"], cond["t_crossattn"]), 0) if self.pair else cond["t_crossattn"]
        self.ctx_len = int(ctx.shape[1])
        self.latent_hw = (int(h), int(w))
        self.t_kv = self.unet.project_context(ctx)                        # hoisted k|v of all transformers
        self.t_fused = self.unet.prepare_fused_tattn(self.t_kv)           # ... folded further into the fused t_attn tables
        # force_uc_zero_embeddings=["label"] (reference sample loop) makes the unconditional context exactly zero:
        # its cross-attention is then x + to_out.bias — one host sync per sampling run buys half of every t_attn
        self.zero_ctx_rows = batch_size if self.pair and _all_zero(uc["t_crossattn"]) else 0
        # two launch streams: the unconditional and the conditional half of the CFG pair never meet before the
        # guidance step, so each runs the UNet on its own HIP stream, planned for half of the CUs.  Measured on
        # MI355X: one stream leaves the chip idle during every kernel's ramp-up / epilogue / tail (a half-GPU plan
        # alone is only 24 % slower than the whole-GPU plan); two concurrent streams fill those holes.
        self.dual = self.pair and (DUAL_STREAM if two_streams is None else bool(two_streams))
        if self.dual:
            self.side = torch.cuda.Stream(device=dev)
            self.eps = torch.empty((2 * batch_size, h, w, 4), dtype=torch.float32, device=dev)
            self.t_kv_u = [[kv[:batch_size] for kv in lst] for lst in self.t_kv]
            self.t_kv_c = [[kv[batch_size:] for kv in lst] for lst in self.t_kv]
            self.t_fused_u = [[tb.rows(0, batch_size) if tb is not None else None for tb in lst] for lst in self.t_fused]
            self.t_fused_c = [[tb.rows(batch_size) if tb is not None else None for tb in lst] for lst in self.t_fused]
        self.xin = torch.zeros((self.rows, h, w, packing.KPAD), dtype=torch.bfloat16, device=dev)
        concat = (torch.cat((uc["concat"], cond["concat"]), 0) if self.pair else cond["concat"]).float().contiguous()
        ops.nhwc_set_channels(concat, self.xin, 4)                         # channels 4..8: mask, masked latent
        self._emb_cache: Dict[float, torch.Tensor] = {}
        self.dev = dev
        # stream-K workspaces owned by this stepper (one per launch stream): allocated with it, referenced by the
        # graphs captured from it, freed with it
        self.ws = ops.Workspace(dev)
        self.ws_side = ops.Workspace(dev) if self.dual else None
        # launch streams of OTHER runners sharing the device: the caller's ambient share (a lane of predict_many runs its
        # conditioning AND its noise search under launch_context(cu_share=n)); _GraphedSteps overrides it for its runner
        self.cu_share = max(1, int(ops._ctx.cu_share))

    def coefs(self, sigma: float) -> Precond:
        """(c_skip, c_out, c_in, c_noise) of the engine's denoiser at the host sigma"""
        return precond_coefs(self.den, sigma, self.table)

    def emb_rows(self, c_noise: float) -> torch.Tensor:
        """the time-embedding rows of the network's timestep input (a table index or a real c_noise), cached by its value"""
        c_noise = float(c_noise)
        rows = self._emb_cache.get(c_noise)
        if rows is None:
            t = torch.full((self.rows,), c_noise, dtype=torch.float32, device=self.dev)
            rows = self.unet.time_embedding_rows(t)
            self._emb_cache[c_noise] = rows
        return rows

    def new_char_maps(self) -> torch.Tensor:
        """a buffer for the character maps of one evaluation: fp32 [B, L, h_map, w_map], one entry per image (the conditional rows).
        Raises what ``UnifiedUNetModel.char_map_plan`` raises — before anything is launched or captured"""
        _, (hm, wm) = self.unet.char_map_plan(*self.latent_hw, self.ctx_len)
        return torch.zeros((self.B, self.ctx_len, hm, wm), dtype=torch.float32, device=self.dev)

    def unet_eps(self, x: torch.Tensor, sigma: float, emit_maps: bool = False, churn: float = 0.0,
                 noise: Optional[torch.Tensor] = None, char_maps: Optional[torch.Tensor] = None):
        """the UNet call on x (fp32 NCHW [B,4,h,w]) at the denoiser's (possibly quantised) sigma -> (network output fp32 NHWC
        [rows,h,w,ld] — the CFG pair's 2B rows or, unguided, B —, the evaluation's ``Precond``); churn != 0: x += churn * noise
        first, in the same launch that packs the UNet input.  char_maps (``new_char_maps``): the call also writes the head-mean
        text-attention maps of the conditional rows there — the selected layers take udt_tattn_fused_maps, eps has the same bits"""
        k = self.coefs(sigma)
        if churn != 0.0 and noise is None:
            raise ValueError("a churned evaluation needs the step's draw (draw_step_noise)")
        if not self.eps_cfg:
            ops.precond_unet_input(x, self.xin, k.c_in, self.pair, noise if churn != 0.0 else None, churn)
        elif churn != 0.0:
            ops.unet_input_churn(x, noise, self.xin, k.c_in, churn)
        else:
            ops.unet_input(x, self.xin, k.c_in)
        if emit_maps:
            self.unet.clear_attn_map()
        emb = self.emb_rows(k.c_noise)
        if self.dual and not emit_maps:
            eps = self._forward_two_streams(emb, char_maps)
        else:
            with ops.launch_context(cu_share=self.cu_share, workspace=self.ws):
                # one stream: the conditional rows are the pair's second half, whether or not the unconditional context is zero
                eps = self.unet.forward_nhwc(self.xin, emb, self.t_kv, emit_maps=emit_maps, zero_ctx_rows=self.zero_ctx_rows,
                                             t_fused=self.t_fused, char_maps=char_maps, map_from=self.B if self.pair else 0)
        return eps, k

    def step(self, x: torch.Tensor, sigma: float, sigma_next: float, emit_maps: bool = False,
             denoised: Optional[torch.Tensor] = None, churn: float = 0.0, noise: Optional[torch.Tensor] = None,
             char_maps: Optional[torch.Tensor] = None) -> None:
        """in-place Euler update of x (fp32 NCHW [B,4,h,w]) from sigma (sigma_hat on a churned step: x += churn * noise before
        the evaluation) to sigma_next; denoised (optional): receives the guided denoised latent"""
        eps, k = self.unet_eps(x, sigma, emit_maps, churn, noise, char_maps)
        if self.eps_cfg:
            ops.cfg_euler_step(x, eps, sigma, sigma_next, self.scale, denoised=denoised, c_out=k.c_out)
        else:
            ops.precond_euler_step(x, eps, k.c_skip, k.c_out, sigma, sigma_next, self.scale, self.pair, denoised=denoised)

    def run_plan(self, bufs: Dict[str, torch.Tensor], plan, noise: Optional[torch.Tensor] = None,
                 char_maps: Optional[torch.Tensor] = None) -> None:
        """one sampler step: per evaluation of ``plan`` (a tuple of ``EulerEval`` / ``Eval`` / ``MultistepEval``), the UNet call
        on its source buffer and its fused launch; ``bufs`` maps the plan's buffer names to fp32 NCHW tensors, ``noise`` is this
        step's draw (ancestral or churn: plan_noise_slots), ``char_maps`` (``new_char_maps``) what an evaluation with ``maps`` fills"""
        for e in plan:
            src = bufs[e.src]
            cm = char_maps if e.maps else None
            if e.maps and cm is None:
                raise ValueError("an evaluation of the plan emits character maps and no buffer was given (new_char_maps)")
            if isinstance(e, EulerEval):
                self.step(src, e.sigma, e.sigma_next, churn=e.churn, noise=noise, char_maps=cm)
                continue
            if isinstance(e, MultistepEval):
                eps, k = self.unet_eps(src, e.sigma, char_maps=cm)
                ms = dict(hist=[bufs[b] for b, _ in e.hist], d_out=bufs[e.d_out], out=bufs[e.out])
                ks = (e.k0,) + tuple(kj for _, kj in e.hist)
                if self.eps_cfg:
                    ops.cfg_multistep_step(src, eps, k.c_out, self.scale, e.sigma, ks, **ms)
                else:
                    ops.precond_multistep_step(src, eps, k.c_skip, k.c_out, self.scale, self.pair, e.sigma, ks, **ms)
                continue
            eps, k = self.unet_eps(src, e.sigma, churn=e.churn, noise=noise, char_maps=cm)
            terms = dict(aux=bufs[e.aux] if e.aux else None, ka=e.ka, prev=bufs[e.prev] if e.prev else None, kp=e.kp,
                         noise=noise if e.kn != 0.0 else None, kn=e.kn, out=bufs[e.out],
                         denoised=bufs[e.den_out] if e.den_out else None)
            if self.eps_cfg:
                ops.cfg_sampler_step(src, eps, k.c_out, self.scale, e.kx, e.kd, **terms)
            else:
                ops.precond_sampler_step(src, eps, k.c_skip, k.c_out, self.scale, self.pair, e.kx, e.kd, **terms)

    def check(self) -> None:
        """synchronise and raise if a stream-K launch of this stepper timed out (library err word)"""
        self.ws.check()
        if self.ws_side is not None:
            self.ws_side.check(self.side.cuda_stream)

    def _forward_two_streams(self, emb: torch.Tensor, char_maps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uc half on the current stream, c half on the side stream (fork / join; captured as two graph branches);
        the stream-K kernels of both streams must be co-resident: each is planned for half of this stepper's CUs.
        char_maps: written by the conditional half, from the side stream (its rows are that call's whole batch: map_from 0)"""
        B = self.B
        main = torch.cuda.current_stream()
        share = 2 * self.cu_share
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side), ops.launch_context(cu_share=share, workspace=self.ws_side):
            eps_c = self.unet.forward_nhwc(self.xin[B:], emb[B:], self.t_kv_c, zero_ctx_rows=0, t_fused=self.t_fused_c,
                                           char_maps=char_maps, map_from=0)
            self.eps[B:].copy_(eps_c)
        with ops.launch_context(cu_share=share, workspace=self.ws):
            eps_u = self.unet.forward_nhwc(self.xin[:B], emb[:B], self.t_kv_u, zero_ctx_rows=self.zero_ctx_rows,
                                           t_fused=self.t_fused_u)
            self.eps[:B].copy_(eps_u)
        main.wait_stream(self.side)
        return self.eps


class _GraphedSteps:
    """hipGraph replay of the sampling loop.  One sampler step is ~580 kernel launches whose arguments depend only on
    (step index, shapes); each step's launch sequence is captured once into a hipGraph on a private memory pool and
    replayed for every later batch of the same shape: the host then issues 50 graph launches per batch instead of
    ~29,000 kernel launches (8 ms of Python / ctypes time per step), and the command processor walks the kernels
    back to back.  Conditioning (text k|v projections, concat channels) lives in static device buffers that
    ``rebind`` refreshes in place; the latent ``x``, the scratch / history buffers the plans name and, if a plan reads
    noise, the run's draws ([slots, B, 4, h, w] — one per step for ancestral plans, one per churned step for churned ones,
    plan_noise_slots — refreshed per run by ``load``) are static fp32 buffers; each captured step has its slot baked in.
    A runner serves one sequence of ``plans`` ((step, plan) pairs; by default Euler over every step of ``sig``), one
    graph per step index."""

    def __init__(self, model, cond, uc, batch_size, latent_hw, scale, sig, cu_share: int = 1, plans=None, pair: bool = True):
        # cu_share > 1: this runner is one of several batches in flight; its launches are planned for 1/cu_share of
        # the CUs and its UNet stays on one stream (the concurrency comes from the other batches)
        self.cu_share = int(cu_share)
        self.st = _Stepper(model, cond, uc, batch_size, latent_hw, scale, two_streams=None if cu_share == 1 else False, pair=pair)
        self.st.cu_share = self.cu_share
        self.fingerprint = weights_fingerprint(model)
        if plans is None:
            plans = [(i, (EulerEval(sig[i], sig[i + 1]),)) for i in range(len(sig) - 1)]
        self.plans = dict(plans)
        h, w = latent_hw
        self.x = torch.zeros((batch_size, 4, h, w), dtype=torch.float32, device=self.st.dev)
        self.bufs = {"x": self.x}
        for name in plan_buffers(plans):                  # e.g. LinearMultistepSampler's derivative ring d0 .. d{order-1}
            self.bufs[name] = torch.zeros_like(self.x)
        self.slots = plan_noise_slots(plans)
        self.noise = (torch.zeros((len(self.slots),) + tuple(self.x.shape), dtype=torch.float32, device=self.st.dev)
                      if self.slots else None)
        # character maps: a static fp32 [B, L, h_map, w_map] buffer the graph of the step that carries ``maps`` writes
        self.maps = self.st.new_char_maps() if plans_emit_maps(plans) else None
        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.pool = torch.cuda.graph_pool_handle()
        self.capture_stream = torch.cuda.Stream(device=self.st.dev)
        self.warm = False
        self.last_replay: Optional[torch.cuda.Event] = None

    def rebind(self, cond, uc) -> bool:
        """refresh the static conditioning buffers for a new batch; False if the launch sequence would differ"""
        st = self.st
        zero_rows = st.B if st.pair and _all_zero(uc["t_crossattn"]) else 0
        if zero_rows != st.zero_ctx_rows or cond["concat"].shape[0] != st.B:
            return False
        ctx = torch.cat((uc["t_crossattn"], cond["t_crossattn"]), 0) if st.pair else cond["t_crossattn"]
        for dst_list, src_list in zip(st.t_kv, st.unet.project_context(ctx)):
            for dst, src in zip(dst_list, src_list):
                dst.copy_(src)
        st.unet.prepare_fused_tattn(st.t_kv, out=st.t_fused)              # tables refreshed in place (views stay valid)
        concat = (torch.cat((uc["concat"], cond["concat"]), 0) if st.pair else cond["concat"]).float().contiguous()
        ops.nhwc_set_channels(concat, st.xin, 4)
        return True

    def load(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None) -> None:
        """the run's latent and, if a plan reads noise, its draws (draw_step_noise)"""
        self.x.copy_(x)
        if self.noise is not None and noise is not None:
            self.noise.copy_(noise)

    def _capture(self, i: int) -> torch.cuda.CUDAGraph:
        st, plan = self.st, self.plans[i]
        noise = self.noise[self.slots[i]] if i in self.slots else None
        for e in plan:
            st.emb_rows(st.coefs(e.sigma).c_noise)           # time-embedding rows are cached outside the graph
        if not self.warm:
            # one eager pass on the capture stream: sets kernel attributes, allocates the library's pages
            torch.cuda.synchronize()
            with torch.cuda.stream(self.capture_stream):
                keep = {k: v.clone() for k, v in self.bufs.items()}
                st.run_plan(self.bufs, plan, noise, self.maps)
                for k, v in keep.items():
                    self.bufs[k].copy_(v)
            torch.cuda.synchronize()
            self.warm = True
        g = torch.cuda.CUDAGraph()
        # thread_local: other threads of the process (the RCCL watchdog under torch.distributed) may touch the
        # HIP runtime while this thread captures
        with torch.cuda.graph(g, pool=self.pool, stream=self.capture_stream, capture_error_mode="thread_local"):
            st.run_plan(self.bufs, plan, noise, self.maps)
        self.graphs[i] = g
        return g

    def capture(self) -> None:
        """capture every step not captured yet, on the runner's own stream, ordered behind the current stream"""
        missing = [i for i in self.plans if i not in self.graphs]
        if missing:
            lane = torch.cuda.current_stream()
            self.capture_stream.wait_stream(lane)
            for i in missing:
                self._capture(i)
            lane.wait_stream(self.capture_stream)


class _RunnerKey(NamedTuple):
    """what a cached graph runner was built for: engine, latent shape, guidance scale, device, the exact plan sequence (schedule
    and init_step), on the lanes its slot of n_lanes, the guider kind and the denoiser's parameterisation (``denoiser_key``: the
    graphs bake in the host coefficients, so a swapped ``engine.denoiser`` gets a runner of its own)"""
    model: int
    shape: tuple
    scale: float
    device: Optional[int]
    plans: tuple
    slot: int = 0
    n_lanes: int = 1
    guider: str = "VanillaCFG"
    denoiser: tuple = ()


class _PlanSampler:
    """the sampling loop of every sampler here: a sampler supplies ``step_plan``; this runs the plans as eager launches or
    hipGraph replays — alone (``_sample``), on the lanes of pipeline.predict_many (``sample_lane``) or as several batches in
    flight (``sample_in_flight``) — and draws the initial noise (the noise search does not depend on the sampler)"""
    use_graphs = os.environ.get("UDT_GRAPHS", "1") != "0"      # hipGraph replay of the main loop (eager launches if off)
    uses_noise = False                 # ancestral samplers: one rng draw [B,4,h,w] per step, the last step included
    implements_churn = False           # s_churn > 0 (EDMSampler): EulerEDMSampler only

    def step_plan(self, sig, i: int, init_step: int = 0) -> tuple:
        """the evaluations of step i (sig: host sigmas, len num_steps + 1) -> tuple of EulerEval / Eval / MultistepEval"""
        raise NotImplementedError

    def plans(self, sig, init_step: int = 0, char_maps: bool = False):
        """char_maps: the first evaluation of the middle step carries ``maps`` (ValueError if init_step lies behind that step)"""
        if char_maps:
            char_map_step(len(sig), init_step)             # (before the generator below prints a progress bar)
        plans = [(i, self.step_plan(sig, i, init_step)) for i in self.get_sigma_gen(len(sig), init_step=init_step)]
        return plans_with_char_maps(plans, len(sig), init_step) if char_maps else plans

    def char_map_step(self, init_step: int = 0, num_steps=None) -> int:
        """the step at which a run with character maps takes them; ValueError if init_step lies behind it (host only)"""
        return char_map_step(len(self._host_sigmas(num_steps)), init_step)

    def _host_sigmas(self, num_steps=None):
        n = self.num_steps if num_steps is None else num_steps
        return [float(s) for s in self.discretization(n, device="cpu")]

    @property
    def _pair(self) -> bool:
        """does the guider run the CFG pair (VanillaCFG) or the conditional rows alone (IdentityGuider)?"""
        return type(self.guider) is VanillaCFG

    @property
    def _scale(self) -> float:
        return float(self.guider.scale) if self._pair else 0.0

    def _check_fast_path(self, model=None):
        """raise for what the fused step does not compute, so that nothing falls through to another formula; ``model``: the engine
        (its denoiser and scaling classes are checked too)"""
        if type(self.guider) not in (VanillaCFG, IdentityGuider):
            raise NotImplementedError(f"the fused MI355X step implements VanillaCFG and IdentityGuider guidance, not "
                                      f"{type(self.guider).__name__}")
        if self._pair and type(self.guider.dyn_thresh) is not NoDynamicThresholding:
            raise NotImplementedError(f"the fused MI355X step implements NoDynamicThresholding, not "
                                      f"{type(self.guider.dyn_thresh).__name__}")
        if model is not None:
            check_denoiser(model.denoiser)
        elif not self._pair:
            # the VanillaCFG check is a check of the sampler's own options and has always run without an engine; the unguided route
            # is one of the udt_precond_* routes, whose scalars come from the engine's denoiser: there is nothing to run it on
            raise NotImplementedError("IdentityGuider samples through the engine's denoiser (udt_precond_* launches) and no engine "
                                      "was given; only the VanillaCFG options can be checked without one")
        if getattr(self, "s_churn", 0.0) != 0.0 and not self.implements_churn:
            raise NotImplementedError(f"s_churn > 0 (stochastic sampling) is implemented for EulerEDMSampler only, not "
                                      f"{type(self).__name__}")

    def draw_step_noise(self, shape, device, num_steps=None, init_step: int = 0) -> Optional[torch.Tensor]:
        """the ancestral draws of one run: one rng.randn of ``shape`` per step from init_step on, in step order, as ONE device
        buffer [steps, *shape] (None for the deterministic samplers; EulerEDMSampler: one per churned step).  Drawn up front so
        that graph replays can read a slice per step; the values equal per-step draws because the CPU streams are sequential."""
        if not self.uses_noise:
            return None
        n = len(self._host_sigmas(num_steps)) - 1 - init_step
        return rng.randn_steps_on(n, shape, device)

    # -------------------------------------------------------------------------------------- noise search
    def _search_plans(self, sig):
        """the noise search's two steps: plain Euler under every sampler (EulerEDMSampler: its own, possibly churned, steps)"""
        return [(i, (EulerEval(sig[i], sig[i + 1]),)) for i in range(len(sig) - 1)]

    def get_init_noise(self, cfgs, model, cond, batch, uc=None):
        """noise_iters candidates, each scored by the text-attention local loss after the 2nd of 2 Euler steps;
        the per-sample arg-min is kept (identical to the reference for batch 1; the reference is undefined for
        larger batches).  All randn draws come from the CPU default generator, in the reference's order (churn draws of
        EulerEDMSampler(s_churn > 0) included: the order of the reference run on the CPU)."""
        self._check_fast_path(model)
        H, W = batch["target_size_as_tuple"][0]
        shape = (cfgs.batch_size, cfgs.channel, int(H) // cfgs.factor, int(W) // cfgs.factor)
        dev = cond["concat"].device
        randn = rng.randn_on(shape, dev)
        if cfgs.noise_iters <= 0:
            return randn
        sig = self._host_sigmas(2)
        plans = self._search_plans(sig)
        slots = plan_noise_slots(plans)
        mask, seg = batch["mask"], batch["seg_mask"]
        B, K = shape[0], int(cfgs.noise_iters)
        uc = default(uc, cond)
        # the reference draws the first candidate, then one more after scoring each (the last draw is never used but advances the
        # generator): K + 1 draws in the same order.  Under churn every scored candidate's steps draw too (the reference run on
        # the CPU): candidate k, its churn draws in step order, candidate k + 1, ..., the unused last candidate — all taken here,
        # up front, in that order
        cands, churn, scores = [randn], [], []
        for _ in range(K):
            churn.append(rng.randn_steps_on(len(slots), shape, dev) if slots else None)
            cands.append(rng.randn_on(shape, dev))
        cands = cands[:K]
        # candidates are independent of each other (2 Euler steps + the local loss of THAT candidate's attention maps), so they
        # run as extra batch entries of the same UNet calls: up to 16 samples (32 with the CFG pair) per call instead of K
        # sequential 2-step runs on B samples — the reference-default workload (batch 1, noise_iters 10) is launch-latency-bound
        # at 2 samples per call.  UDT_NOISE_BATCH=0: one candidate at a time (A/B, and the regime of the round-2 numbers)
        G = max(1, min(K, 16 // max(1, B))) if NOISE_BATCH else 1
        tile = lambda d, g: {k: (v.repeat((g,) + (1,) * (v.dim() - 1)) if torch.is_tensor(v) else v) for k, v in d.items()}
        steppers = {}
        for g0 in range(0, K, G):
            chunk = cands[g0:g0 + G]
            g = len(chunk)
            stepper = steppers.get(g)
            if stepper is None:
                stepper = steppers[g] = _Stepper(model, tile(cond, g), tile(uc, g), g * B, shape[2:], self._scale, pair=self._pair)
            x = torch.cat(chunk, 0).clone()
            x *= (1.0 + sig[0] ** 2.0) ** 0.5
            ll = None
            for i, (e,) in plans:
                nz = torch.cat([c[slots[i]] for c in churn[g0:g0 + G]], 0) if i in slots else None
                stepper.step(x, e.sigma, e.sigma_next, emit_maps=True, churn=e.churn, noise=nz)
                ll = model.loss_fn.get_min_local_loss(stepper.unet.attn_map_cache, mask, seg, cond_only=self._pair)
            scores.extend(ll.reshape(g, B).unbind(0))
            stepper.unet.clear_attn_map()
            stepper.check()
        score = torch.stack(scores, 0)                                   # [iters, B]
        best = score.argmin(dim=0)                                        # first minimum, like the stable sort
        print(f"Init local loss: Best {score.min().item()} Worst {score.max().item()}")
        stack = torch.stack(cands, 0)                                     # [iters, B, 4, h, w]
        return stack[best, torch.arange(shape[0], device=dev)].contiguous()

    # --------------------------------------------------------------------------------------------- loop
    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, init_step=0, batch=None, aae_enabled=False, detailed=False,
                 name=None, noise: Optional[torch.Tensor] = None, **kwargs):
        """reference __call__(denoiser, x, cond, uc, num_steps) [+ init_step]; ``noise``: the run's ancestral draws
        (draw_step_noise), drawn here when not given"""
        if aae_enabled:
            raise NotImplementedError(f"attend-and-excite is implemented for EulerEDMSampler only, not {type(self).__name__}")
        if detailed:
            # the per-character maps of every image, out of the middle step's fused text attention, stay on the sampler as
            # ``last_char_maps`` (fp32 [B, L, h_map, w_map]); the PNG / .npy dumps are EulerEDMSampler's
            x, self.last_char_maps = self._sample(denoiser, x, cond, uc, num_steps, init_step, noise, char_maps=True)
            return x
        return self._sample(denoiser, x, cond, uc, num_steps, init_step, noise)

    def _sample(self, model, x, cond, uc=None, num_steps=None, init_step=0, noise: Optional[torch.Tensor] = None,
                char_maps: bool = False):
        """the plain sampling loop: hipGraph replay, eager launches if graphs are off or unavailable.  char_maps: -> (x, maps), the
        head-mean text-attention maps of every image at the middle step (fp32 [B, L, h_map, w_map]); x has the bits of the run
        that did not ask"""
        if char_maps and model is None:
            raise NotImplementedError("detailed character maps come out of the engine's UNet (its save_attn_layers select the "
                                      "layers) and no engine was given")
        if char_maps:
            self.char_map_step(init_step, num_steps)       # ValueError before anything is launched
        self._check_fast_path(model)
        require_gpu(x, type(self).__name__)
        uc = default(uc, cond)
        sig = self._host_sigmas(num_steps)
        x = x.float().contiguous()
        if noise is None:
            noise = self.draw_step_noise(x.shape, x.device, num_steps, init_step)
        x *= (1.0 + sig[0] ** 2.0) ** 0.5                                  # in place, like the reference :54
        plans = self.plans(sig, init_step, char_maps)
        if self.use_graphs:
            out = self._run_graphed(model, x, cond, uc, sig, plans, noise)
            if out is not None:
                return out
        stepper = _Stepper(model, cond, uc, x.shape[0], x.shape[2:], self._scale, pair=self._pair)
        maps = stepper.new_char_maps() if char_maps else None
        bufs = {"x": x}
        for name in plan_buffers(plans):
            bufs[name] = torch.empty_like(x)
        slots = plan_noise_slots(plans)
        for i, plan in plans:
            stepper.run_plan(bufs, plan, noise[slots[i]] if noise is not None and i in slots else None, maps)
        stepper.check()
        return (x, maps) if char_maps else x

    def _runner_key(self, model, x, plans, slot: int = 0, n_lanes: int = 1) -> _RunnerKey:
        return _RunnerKey(id(model), tuple(x.shape), self._scale, x.device.index, tuple(plans), slot, n_lanes,
                          type(self.guider).__name__, denoiser_key(model.denoiser))

    def _run_graphed(self, model, x, cond, uc, sig, plans, noise):
        """replay (capturing on first use) the hipGraphs of this sampling configuration; None -> eager launches.  Plans that
        emit character maps: -> (x, maps), both cloned from the runner's static buffers"""
        key = self._runner_key(model, x, plans)
        cache = self.__dict__.setdefault("_graphed", {})
        try:
            gs = cache.get(key)
            if gs is not None and gs.fingerprint != weights_fingerprint(model):
                gs = None                                       # weights changed under the captured graphs
            if gs is None or not gs.rebind(cond, uc):
                cache.clear()                                   # one configuration at a time (each holds a memory pool)
                gs = _GraphedSteps(model, cond, uc, x.shape[0], x.shape[2:], self._scale, sig, plans=plans, pair=self._pair)
                cache[key] = gs
            gs.load(x, noise)
            gs.capture()
            for i in gs.plans:
                gs.graphs[i].replay()
            out = gs.x.clone() if gs.maps is None else (gs.x.clone(), gs.maps.clone())
            gs.st.check()                       # one sync per sampling loop: surfaces a stream-K time-out as UdtError
            return out
        except RuntimeError as e:
            if not _is_capture_failure(e):                      # kernel status errors, OOM, ...: never hidden
                raise
            if not self.__dict__.get("_graph_warned"):
                print(f"[udifftext_amd] hipGraph capture unavailable ({e}); using eager launches", file=sys.stderr)
                self._graph_warned = True
            self.use_graphs = False
            cache.clear()
            return None

    # ------------------------------------------------------------------------------- batches in flight
    def _lane_runner(self, model, x, cond, uc, slot, n_lanes, sig, plans):
        """this lane's graph runner, rebound to the batch, with every graph of ``plans`` captured.
        A runner that leaves the cache may still have graph replays queued on a lane stream (nothing here synchronises the
        host): it is parked in ``_retired`` — its graphs and private memory pool stay alive — until its ``last_replay`` event
        has completed (checked here) or the caller has synchronised (pipeline.predict_many -> release_retired); runners of
        the current call's lanes are never evicted."""
        cache = self.__dict__.setdefault("_in_flight", {})
        retired = self.__dict__.setdefault("_retired", [])
        retired[:] = [r for r in retired if r.last_replay is not None and not r.last_replay.query()]
        key = self._runner_key(model, x, plans, slot, n_lanes)
        gs = cache.get(key)
        if gs is not None and gs.fingerprint != weights_fingerprint(model):     # weights changed: the captured pointers are stale
            retired.append(cache.pop(key))
            gs = None
        if gs is None or not gs.rebind(cond, uc):
            gs = _GraphedSteps(model, cond, uc, x.shape[0], x.shape[2:], self._scale, sig, cu_share=n_lanes, plans=plans,
                               pair=self._pair)
            if key in cache:
                retired.append(cache.pop(key))
            victims = [k for k in cache if (k.model, k.shape, k.n_lanes) != (key.model, key.shape, key.n_lanes)]
            while len(cache) >= 8 and victims:                  # every runner owns a memory pool: keep the newest few
                retired.append(cache.pop(victims.pop(0)))
            cache[key] = gs
        gs.capture()             # first use of this lane / shape (a capture synchronises the device once)
        return gs

    @staticmethod
    def _finish(gs, stream, deferred_checks: Optional[list]) -> None:
        """mark the runner's replays done once ``stream`` gets here; its error-word check now or into ``deferred_checks``"""
        gs.last_replay = torch.cuda.Event()
        gs.last_replay.record(stream)
        if deferred_checks is None:
            gs.st.check()
        elif gs.st.check not in deferred_checks:
            deferred_checks.append(gs.st.check)

    def sample_lane(self, model, x, cond, uc, slot: int, n_lanes: int, init_step=0, deferred_checks: Optional[list] = None,
                    noise: Optional[torch.Tensor] = None, char_maps: bool = False):
        """the sampling loop of ONE batch on the CURRENT stream, as lane ``slot`` of ``n_lanes`` free-running lanes
        (pipeline.predict_many): rebind this lane's runner to the batch, enqueue all graph replays, return the latent — no
        host synchronisation and no event shared with the other lanes, so a lane runs condition -> sample -> decode back to
        back while the launch thread is already feeding the next lane.  Launches are planned for 1 / n_lanes of the CUs
        (cu_share), as in ``sample_in_flight``.  The runner's error-word check goes to ``deferred_checks``; ``noise``: the
        batch's ancestral draws (drawn here when not given).  char_maps: -> (z, maps) as ``_sample``; the maps are cloned on the
        lane's stream, behind the replays, before the runner serves another batch."""
        if n_lanes <= 1 or not self.use_graphs:
            return self._sample(model, x, cond, uc, None, init_step, noise, char_maps=char_maps)
        self._check_fast_path(model)
        require_gpu(x, type(self).__name__)
        uc = default(uc, cond)
        sig = self._host_sigmas(None)
        if noise is None:
            noise = self.draw_step_noise(x.shape, x.device, None, init_step)
        gs = self._lane_runner(model, x, cond, uc, slot, n_lanes, sig, self.plans(sig, init_step, char_maps))
        gs.load(x.float(), noise)
        gs.x.mul_((1.0 + sig[0] ** 2.0) ** 0.5)
        for i in gs.plans:
            gs.graphs[i].replay()
        out = gs.x.clone() if not char_maps else (gs.x.clone(), gs.maps.clone())
        self._finish(gs, torch.cuda.current_stream(), deferred_checks)
        return out

    def sample_in_flight(self, model, xs, conds, ucs, init_step=0, deferred_checks: Optional[list] = None,
                         streams: Optional[list] = None, noises: Optional[list] = None, char_maps: bool = False):
        """run the sampling loops of SEVERAL independent batches concurrently (one launch stream + one set of
        hipGraphs each, every stream planned for its share of the CUs) and return their latents.

        One launch stream cannot keep the chip busy through every kernel's ramp-up, epilogue and tail; measured on
        MI355X (512x512, batch 4): 14.0 ms per sampler step for one batch at a time, 10.9 ms per step and batch with
        two batches in flight, 10.1 with three (pipeline.IN_FLIGHT).  Falls back to one batch after the other when
        graphs are unavailable.

        ``deferred_checks``: a list that receives the runners' error-word checks instead of running them here (each
        check synchronises its stream) — a caller that keeps enqueuing work behind this call (pipeline.predict_many)
        runs them once at its own synchronisation point.
        ``streams``: launch streams to replay on, one per batch (default: the runners' capture streams).  A caller
        that already owns one stream per batch passes them so that no further streams are active: hipStreams share a
        small number of hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and two busy streams on one queue serialise.
        ``noises[k]``: batch k's ancestral draws (drawn here, in batch order, when not given).
        char_maps: every entry of the result is (z, maps) as ``_sample`` hands them back."""
        n = len(xs)
        if noises is None:
            noises = [self.draw_step_noise(x.shape, x.device, None, init_step) for x in xs]
        if n == 1 or not self.use_graphs:
            return [self._sample(model, x, c, u, None, init_step, nz, char_maps=char_maps) for x, c, u, nz in zip(xs, conds, ucs, noises)]
        self._check_fast_path(model)
        sig = self._host_sigmas(None)
        plans = self.plans(sig, init_step, char_maps)
        runners = []
        for slot, (x, c, u, nz) in enumerate(zip(xs, conds, ucs, noises)):
            require_gpu(x, type(self).__name__)
            gs = self._lane_runner(model, x, c, default(u, c), slot, n, sig, plans)
            gs.load(x.float(), nz)
            gs.x.mul_((1.0 + sig[0] ** 2.0) ** 0.5)
            runners.append(gs)
        main = torch.cuda.current_stream()
        lanes = list(streams[:n]) if streams is not None and len(streams) >= n else [gs.capture_stream for gs in runners]
        for lane in lanes:
            lane.wait_stream(main)
        for i, _ in plans:                               # interleaved launches: every queue stays fed
            for gs, lane in zip(runners, lanes):
                with torch.cuda.stream(lane):
                    gs.graphs[i].replay()
        for lane in lanes:
            main.wait_stream(lane)
        outs = [gs.x.clone() if not char_maps else (gs.x.clone(), gs.maps.clone()) for gs in runners]
        for gs in runners:
            self._finish(gs, main, deferred_checks)
        return outs

    def release_retired(self) -> None:
        """drop the runners the lanes took out of their cache — call after the lanes' streams have been synchronised"""
        self.__dict__.get("_retired", []).clear()

    def invalidate_graphs(self) -> None:
        """drop every captured hipGraph (explicit hook; the caches also notice changed weights by fingerprint)"""
        self.__dict__.pop("_graphed", None)
        self.__dict__.pop("_in_flight", None)


AAE_GRAPH = os.environ.get("UDT_AAE_GRAPH", "1") != "0"      # hipGraph replay of the attend-and-excite gradient (A/B switch)


class EulerEDMSampler(_PlanSampler, EDMSampler):
    """reference sampling.py:218-420: one udt_cfg_euler_step evaluation per step (``EulerEval``) through the shared loop; the
    attend-and-excite loop, the reference-shaped ``sampler_step`` and the ``detailed`` attention-map dump are its own.

    s_churn > 0 (reference :89-137, :324-353): step i of n = num_sigmas - 1 has gamma_i = min(s_churn / n, sqrt(2) - 1) where
    s_tmin <= sigma_i <= s_tmax, else 0 (init_step does not change n).  A churned step first raises the noise level to
    sigma_hat = sigma_i (1 + gamma_i), x += s_noise sqrt(sigma_hat^2 - sigma_i^2) eps, then evaluates and steps from sigma_hat;
    the noise lands in the launch that packs the UNet input (udt_unet_input_churn), so the step's launch count is unchanged.
    One rng draw per churned step, in step order (``draw_step_noise``); gamma_i = 0 is exactly the deterministic step."""
    implements_churn = True

    def churn_gamma(self, sig, i: int) -> float:
        """reference :122-126: gamma of step i of the host schedule ``sig``"""
        return min(self.s_churn / (len(sig) - 1), 2 ** 0.5 - 1) if self.s_tmin <= sig[i] <= self.s_tmax else 0.0

    def draw_step_noise(self, shape, device, num_steps=None, init_step: int = 0) -> Optional[torch.Tensor]:
        """the churn draws of one run: one rng.randn of ``shape`` per CHURNED step from init_step on, in step order, as one buffer
        [n_churned, *shape] (the k-th churned step reads slot k); None, and no generator advances, when no step is churned"""
        if not self.s_churn:
            return None
        sig = self._host_sigmas(num_steps)
        n = sum(1 for i in range(init_step, len(sig) - 1) if self.step_plan(sig, i, init_step)[0].churn != 0.0)
        return rng.randn_steps_on(n, shape, device) if n else None

    def _search_plans(self, sig):
        return [(i, self.step_plan(sig, i)) for i in range(len(sig) - 1)]

    def possible_correction_step(self, euler_step, x, d, dt, next_sigma, denoiser, cond, uc):
        return euler_step

    # --------------------------------------------------------------------------------- attend-and-excite
    def get_c_noise(self, x, model, sigma):
        """reference sampling.py:224-231: the network's timestep input at sigma — the denoiser's (possibly quantised) c_noise"""
        sigma = model.denoiser.possibly_quantize_sigma(sigma).reshape(-1)
        return model.denoiser.possibly_quantize_c_noise(model.denoiser.scaling(sigma)[3])

    def _aae_runner_for(self, model, unet, x, args):
        """the captured evaluation of both update loops (one cache, one invalidation rule: shapes, weights, denoiser) with the inputs
        loaded into its static buffers; None -> eager launches (graphs off, or capture unavailable).  The evaluation's launch
        sequence depends on the shapes only: captured once per sampler, replayed for every update of every step (the timestep index,
        latent and conditioning are device data in static buffers)"""
        from udifftext_amd import backward
        if not (self.use_graphs and AAE_GRAPH):
            return None
        runner = getattr(self, "_aae_runner", None)
        key = denoiser_key(model.denoiser)                                 # (a swapped denoiser gets a capture of its own)
        if runner is None or not runner.valid_for(unet, x, *args) or getattr(self, "_aae_key", None) != key:
            runner = self._aae_runner = None                               # (drop the old pool before the new capture)
            try:
                runner = backward.GraphedLocalLossGrad(unet, model.loss_fn, x, *args)
                runner.load(x, *args)
                self._aae_runner, self._aae_key = runner, key
            except Exception as e:
                if not _is_capture_failure(e):
                    raise
                print(f"[udifftext_amd] attend-and-excite: hipGraph capture unavailable ({type(e).__name__}: {e}); eager launches")
                return None
        else:
            runner.load(x, *args)
        return runner

    def _aae_begin(self, x, model, sigma, cond, batch, who):
        """what both update loops start from -> (xs, evaluate, runner): xs the fp32 latent the loop updates in place — the runner's
        static buffer, or a private clone of ``x`` under eager launches (runner None) — and evaluate() -> (loss, grad) at xs"""
        from udifftext_amd import backward
        require_gpu(x, who)
        c_noise = self.get_c_noise(x, model, sigma)
        unet = model.model.diffusion_model
        x = x.detach().clone().float().contiguous()
        args = (c_noise.float(), cond["concat"], cond["t_crossattn"], batch["mask"], batch["seg_mask"])
        runner = self._aae_runner_for(model, unet, x, args)
        if runner is not None:
            return runner.x, runner.replay, runner
        return x, lambda: backward.unet_local_loss_grad(unet, model.loss_fn, x, *args), None

    def attend_and_excite(self, x, model, sigma, cond, batch, alpha, iter_enabled, thres, max_iter=20):
        """reference sampling.py:233-252: x <- x - alpha * d local_loss / d x, once, or (iter_enabled) until the loss falls to
        ``thres`` or max_iter is passed.  The network sees the RAW x (no c_in scaling — the reference calls model.model directly)
        and only the conditional batch; the gradient runs through the HIP path's written-out reverse pass
        (udifftext_amd.backward.unet_local_loss_grad) — per sample, where the reference only accepts B = 1.  With a captured
        runner one iteration is one graph replay on the runner's static latent and one axpy that updates it in place."""
        xs, evaluate, runner = self._aae_begin(x, model, sigma, cond, batch, "EulerEDMSampler.attend_and_excite")
        iters = 0
        while True:
            loss, grad = evaluate()
            ops.axpy_(xs, grad, -float(alpha))
            iters += 1
            if not iter_enabled or bool((loss <= thres).all()) or iters > max_iter:
                break
        self.aae_evaluations = getattr(self, "aae_evaluations", 0) + iters     # (how many gradients a sampling run took)
        return xs.clone() if runner is not None else xs

    def attend_and_excite_rows(self, x, model, sigma, cond, batch, alpha, iter_enabled, thres, max_iter=20):
        """``attend_and_excite`` with every row of the batch on its OWN B = 1 loop (reference sampling.py:240-252 compares a
        one-element loss): a row whose loss has fallen to ``thres``, or that has passed max_iter, is frozen — it takes no further
        update, whatever its batch mates do — and the loop ends when no row is active.  A row's result therefore depends on its own
        inputs alone (``attend_and_excite`` keeps updating every row while any is above thres).  Frozen rows are still evaluated:
        the batch is not compacted.  One iteration is one graph replay on the runner's static latent, one udt_aae_row_update_f32
        launch that updates it in place, and — only with iter_enabled — the read-back of one int32 (the number of active rows);
        without iter_enabled there is exactly one evaluation and no host synchronisation.
        -> (x, iters): iters int32 [B] on the device, the updates each row took.  At B = 1: ``attend_and_excite``, bit for bit."""
        xs, evaluate, runner = self._aae_begin(x, model, sigma, cond, batch, "EulerEDMSampler.attend_and_excite_rows")
        B = xs.shape[0]
        st = getattr(self, "_aae_rows_state", None)
        if st is None or st[0].shape[1] != B or st[0].device != xs.device:
            st = self._aae_rows_state = (torch.empty((2, B), dtype=torch.int32, device=xs.device),
                                         torch.empty((2, B), dtype=torch.int32, device=xs.device),
                                         torch.empty((1,), dtype=torch.int32, device=xs.device))
        s_in, s_out, n_act = st
        s_in[0].fill_(1)
        s_in[1].zero_()
        evals, frozen, active = 0, 0, B
        while True:
            loss, grad = evaluate()
            ops.aae_row_update_(xs, grad, loss, s_in, s_out, n_act, float(alpha), float(thres), iter_enabled, max_iter)
            s_in, s_out = s_out, s_in
            evals += 1
            frozen += B - active                                           # rows this evaluation computed for nothing
            if not iter_enabled:
                break
            active = int(n_act.item())                                     # the iteration's one 4-byte read-back
            if active == 0:
                break
        iters = s_in[1].clone()
        if iter_enabled:
            counts = iters.cpu().long()
        else:
            counts = torch.ones((B,), dtype=torch.long)                    # (known on the host: nothing is read back)
        prev = getattr(self, "aae_row_updates", None)
        self.aae_row_updates = counts if prev is None or prev.numel() != B else prev + counts
        self.aae_evaluations = getattr(self, "aae_evaluations", 0) + evals
        self.aae_frozen_row_evaluations = getattr(self, "aae_frozen_row_evaluations", 0) + frozen
        return (xs.clone() if runner is not None else xs), iters

    # --------------------------------------------------------------------- the sampling loops around the updates
    def _begin_loop(self, model, x, cond, uc, num_steps):
        """-> (sig, x, stepper): the host sigma schedule, x as fp32 scaled by sqrt(1 + sigma_0^2) (in place where x already is
        contiguous fp32, like the reference :54), and the stepper of this batch"""
        sig = self._host_sigmas(num_steps)
        x = x.float().contiguous()
        x *= (1.0 + sig[0] ** 2.0) ** 0.5
        return sig, x, _Stepper(model, cond, uc, x.shape[0], x.shape[2:], self._scale, pair=self._pair)

    def _aae_steps(self, update, model, x, cond, batch, sig, init_step, noise):
        """the attend-and-excite schedule (reference sampling.py:355-386): before denoising step i the latent takes ``update`` with
        alpha = 20 sqrt(scale_i), iterated at steps 5, 9, ..., 25 down to thresholds -0.5 ... -0.8.  A churned step adds its noise
        BEFORE the update, and the update and the step run at sigma_hat (reference :328-336).  Yields (i, e, x) — the step's index,
        its EulerEval and the updated latent — for the caller to step IN PLACE."""
        scales = np.linspace(start=1.0, stop=0, num=len(sig))
        iter_lst = np.linspace(start=5, stop=25, num=6, dtype=np.int32)
        thres_lst = np.linspace(start=-0.5, stop=-0.8, num=6)
        s_in = x.new_ones([x.shape[0]])
        slot = 0                                                           # the k-th churned step reads draw k
        for i in self.get_sigma_gen(len(sig), init_step=init_step):
            (e,) = self.step_plan(sig, i, init_step)
            alpha = 20 * np.sqrt(scales[i])
            iter_enabled = i in iter_lst
            thres = float(thres_lst[list(iter_lst).index(i)]) if iter_enabled else 0.0
            if e.churn != 0.0:
                ops.axpy_(x, noise[slot], e.churn)
                slot += 1
            x = update(x, model, s_in * e.sigma, cond, batch, alpha, iter_enabled, thres)
            yield i, e, x

    def sample_rows_with_attend_and_excite(self, model, x, cond, batch, uc, num_steps=None, init_step=0,
                                           noise: Optional[torch.Tensor] = None, record_losses: bool = True, char_maps: bool = False):
        """the attend-and-excite sampling loop for a batch of independent images (pipeline.predict_many): the schedule of
        ``_aae_steps`` with the update taken row by row (``attend_and_excite_rows``), and without the per-step VAE decode, the GIF
        and the prints of ``_sample_with_attend_and_excite``.  record_losses: every step emits its attention maps and the per-row
        local loss goes into a device [steps, B] tensor, copied to ``last_row_losses`` once at the end; without it the steps are
        the fast steps (the latent then differs by the two text-attention forms' rounding).
        char_maps: -> (x, maps), the character maps of every row at the middle step (fp32 [B, L, h_map, w_map]): the head and layer
        mean of the maps that step cached (record_losses), or out of its fused text attention (without)."""
        self._check_fast_path(model)
        require_gpu(x, "EulerEDMSampler.sample_rows_with_attend_and_excite")
        uc = default(uc, cond)
        if noise is None:
            noise = self.draw_step_noise(x.shape, x.device, num_steps, init_step)
        sig, x, stepper = self._begin_loop(model, x, cond, uc, num_steps)
        mid = char_map_step(len(sig), init_step) if char_maps else -1
        maps = stepper.new_char_maps() if char_maps else None
        n = max(0, len(sig) - 1 - init_step)
        losses = torch.zeros((n, x.shape[0]), dtype=torch.float32, device=x.device) if record_losses else None
        rows = lambda *a: self.attend_and_excite_rows(*a)[0]
        for k, (i, e, x) in enumerate(self._aae_steps(rows, model, x, cond, batch, sig, init_step, noise)):
            stepper.step(x, e.sigma, e.sigma_next, emit_maps=record_losses, char_maps=maps if i == mid and not record_losses else None)
            if record_losses and i == mid:
                maps.copy_(stepper.unet.char_maps_from_cache(rows_from=x.shape[0] if self._pair else 0))
            if record_losses:
                losses[k].copy_(model.loss_fn.get_min_local_loss(stepper.unet.attn_map_cache, batch["mask"], batch["seg_mask"],
                                                                 cond_only=self._pair))
        if record_losses:
            stepper.unet.clear_attn_map()
        stepper.check()
        if record_losses:
            self.last_row_losses = losses.cpu()
        return (x, maps) if char_maps else x

    # ------------------------------------------------------------------------------------------- API step
    def sampler_step(self, sigma, next_sigma, model, x, cond, batch=None, uc=None, gamma=0.0, alpha=0, iter_enabled=False,
                     thres=None, update=False, name=None, save_loss=False, save_attn=False, save_inter=False):
        """reference-shaped single step on tensors (sigma / next_sigma are [B] tensors); returns
        (x_next, denoised_decode, local_loss).  Generic formulation via denoiser + guider."""
        if gamma > 0:                                                      # reference :328-331, eps from the path's noise source
            sigma_hat = sigma * (gamma + 1.0)
            eps = rng.randn_on(x.shape, x.device).to(x.dtype) * self.s_noise
            x = x + eps * ((sigma_hat ** 2 - sigma ** 2) ** 0.5)[(...,) + (None,) * (x.ndim - 1)]
            sigma = sigma_hat
        if update:
            x = self.attend_and_excite(x, model, sigma, cond, batch, alpha, iter_enabled, thres)
        denoised = self.denoise(x, model, sigma, cond, uc)
        inter = model.decode_first_stage(denoised) if save_inter else None
        if save_loss:
            ll = model.loss_fn.get_min_local_loss(model.model.diffusion_model.attn_map_cache, batch["mask"], batch["seg_mask"])
            if type(self.guider) is VanillaCFG:                            # the conditional half of the pair; unguided: every row
                ll = ll[ll.shape[0] // 2:]
        else:
            ll = torch.zeros(1)
        if save_attn:                                                      # reference sampling.py:344-346
            attn_map = model.model.diffusion_model.save_attn_map(save_name=name, tokens=batch["label"][0])
            self.save_segment_map(attn_map, tokens=batch["label"][0], save_name=name)
        d = to_d(x, sigma, denoised)
        dt = (next_sigma - sigma)[(...,) + (None,) * (x.ndim - 1)]
        return self.euler_step(x, d, dt), inter, ll

    def save_segment_map(self, attn_maps, tokens=None, save_name=None, out_dir="./temp/seg_map"):
        """reference sampling.py:254-262: the per-token heat maps of save_attn_map for the label's characters -> one .npy"""
        import numpy as np
        section = np.stack([attn_maps[i] for i in range(len(tokens))])
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, f"seg_{save_name}.npy"), section)
        return section

    # ------------------------------------------------------------------------------------------- loop
    def step_plan(self, sig, i, init_step=0):
        gamma = self.churn_gamma(sig, i) if self.s_churn else 0.0
        if gamma == 0.0:
            return (EulerEval(sig[i], sig[i + 1]),)
        s = float(sig[i])
        # s_noise sqrt(sigma_hat^2 - sigma^2) without the cancellation, in float64 (a negative gamma lowers sigma_hat and adds
        # nothing, like the reference's ``if gamma > 0``)
        kn = self.s_noise * s * (gamma * gamma + 2.0 * gamma) ** 0.5 if gamma > 0 else 0.0
        return (EulerEval(s * (1.0 + gamma), sig[i + 1], churn=kn),)

    def __call__(self, model, x, cond, batch=None, uc=None, num_steps=None, init_step=0, name=None, aae_enabled=False,
                 detailed=False, noise: Optional[torch.Tensor] = None):
        """``noise``: the run's churn draws (draw_step_noise), drawn here when not given"""
        if not (aae_enabled or detailed):
            return self._sample(model, x, cond, uc, num_steps, init_step, noise)
        self._check_fast_path(model)
        require_gpu(x, "EulerEDMSampler")
        uc = default(uc, cond)
        if noise is None:
            noise = self.draw_step_noise(x.shape, x.device, num_steps, init_step)
        if aae_enabled:
            return self._sample_with_attend_and_excite(model, x, cond, batch, uc, num_steps, init_step, name, detailed, noise)
        # reference sampling.py:384,344-346: at the middle step the text cross-attention maps of the configured layers are plotted
        # and the label's per-character maps saved.  That one step runs with map emission (eager launches, the xattn chain); every
        # other step is the fast step — the loop is the same Euler loop, so the latent equals the plain call's up to the two
        # text-attention forms' rounding
        sig, x, stepper = self._begin_loop(model, x, cond, uc, num_steps)
        name = name if name is not None else (batch["name"][0] if batch is not None and "name" in batch else "sample")
        mid = (len(sig) - 1) // 2
        slot = 0                                                           # the k-th churned step reads draw k
        for i in self.get_sigma_gen(len(sig), init_step=init_step):
            (e,) = self.step_plan(sig, i, init_step)
            stepper.step(x, e.sigma, e.sigma_next, emit_maps=(i == mid), churn=e.churn, noise=noise[slot] if e.churn != 0.0 else None)
            slot += e.churn != 0.0
            if i == mid:
                attn_map = stepper.unet.save_attn_map(save_name=name, tokens=batch["label"][0])
                self.save_segment_map(attn_map, tokens=batch["label"][0], save_name=name)
        stepper.check()
        return x

    def _sample_with_attend_and_excite(self, model, x, cond, batch, uc, num_steps, init_step, name, detailed, noise=None):
        """reference sampling.py:355-420 with aae_enabled: before every denoising step the latent takes attend-and-excite updates
        (the schedule of ``_aae_steps``, the joint update ``attend_and_excite``), the local loss of every step is collected and
        every intermediate denoised latent decoded (the reference writes them as a GIF; imageio is optional here).  Eager
        launches: the update's step count is data-dependent."""
        sig, x, stepper = self._begin_loop(model, x, cond, uc, num_steps)
        name = name if name is not None else (batch["name"][0] if batch is not None and "name" in batch else "sample")
        evals0 = getattr(self, "aae_evaluations", 0)
        inters, local_losses = [], []
        mid = (len(sig) - 1) // 2
        for i, e, x in self._aae_steps(self.attend_and_excite, model, x, cond, batch, sig, init_step, noise):
            den = torch.empty_like(x)
            stepper.step(x, e.sigma, e.sigma_next, emit_maps=True, denoised=den)
            ll = model.loss_fn.get_min_local_loss(stepper.unet.attn_map_cache, batch["mask"], batch["seg_mask"], cond_only=self._pair)
            local_losses.append(float(ll.mean()))
            if detailed and i == mid:
                attn_map = stepper.unet.save_attn_map(save_name=name, tokens=batch["label"][0])
                self.save_segment_map(attn_map, tokens=batch["label"][0], save_name=name)
            inter = torch.clamp((model.decode_first_stage(den) + 1.0) / 2.0, min=0.0, max=1.0)[0]
            inters.append((inter.float().cpu().numpy().transpose(1, 2, 0) * 255).astype(np.uint8))
        stepper.check()
        print(f"Local losses: {local_losses}")
        self.last_local_losses, self.last_inters = local_losses, inters
        self.last_aae_stats = f"{getattr(self, 'aae_evaluations', 0) - evals0} gradient evaluations"
        try:
            import imageio
            os.makedirs("./temp/inters", exist_ok=True)
            imageio.mimsave(f"./temp/inters/{name}.gif", inters, "GIF", duration=0.02)
        except ImportError:                                            # (no imageio in this image: the frames stay on the sampler)
            pass
        return x


def ancestral_step(sigma: float, sigma_next: float, eta: float):
    """reference sampling_utils.get_ancestral_step in float64 -> (sigma_down, sigma_up)"""
    if not eta:
        return sigma_next, 0.0
    up = min(sigma_next, eta * (sigma_next ** 2 * (sigma ** 2 - sigma_next ** 2) / sigma ** 2) ** 0.5)
    return max(sigma_next ** 2 - up ** 2, 0.0) ** 0.5, up


def _euler_to(sigma: float, target: float):
    """x + (x - den)/sigma * (target - sigma) as (kx, kd)"""
    r = (target - sigma) / sigma
    return 1.0 + r, -r


class HeunEDMSampler(_PlanSampler, EDMSampler):
    """reference sampling.py:423-441 (s_churn = 0): Euler predictor, then the trapezoidal corrector with a second evaluation at
    sigma_next — 2 evaluations per step, 1 on the last (sigma_next = 0)"""

    def step_plan(self, sig, i, init_step=0):
        s, sn = float(sig[i]), float(sig[i + 1])
        kx, kd = _euler_to(s, sn)
        if sn < 1e-14:
            return (Eval(s, "x", "x", kx=kx, kd=kd),)
        dt = sn - s
        return (Eval(s, "x", "t", kx=kx, kd=kd, den_out="h0"),                       # t = Euler predictor, h0 = den
                # x + dt/2 * ((x - den)/s + (t - den2)/sn)
                Eval(sn, "t", "x", kx=dt / (2 * sn), kd=-dt / (2 * sn), aux="x", ka=1.0 + dt / (2 * s), prev="h0",
                     kp=-dt / (2 * s)))


class AncestralSampler(_PlanSampler, SingleStepDiffusionSampler):
    """reference sampling.py:140-175: eta, s_noise; noise_sampler is rng.randn (drawn up front, draw_step_noise)"""
    uses_noise = True

    def __init__(self, eta=1.0, s_noise=1.0, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.eta = eta
        self.s_noise = s_noise

    def _noise_coef(self, sigma_next, sigma_up):
        return self.s_noise * sigma_up if sigma_next > 0.0 else 0.0         # torch.where(next_sigma > 0, ...)


class EulerAncestralSampler(AncestralSampler):
    """reference sampling.py:444-452: Euler to sigma_down, then + s_noise * sigma_up * noise — 1 evaluation per step"""

    def step_plan(self, sig, i, init_step=0):
        s, sn = float(sig[i]), float(sig[i + 1])
        down, up = ancestral_step(s, sn, self.eta)
        kx, kd = _euler_to(s, down)
        return (Eval(s, "x", "x", kx=kx, kd=kd, kn=self._noise_coef(sn, up)),)


class DPMPP2SAncestralSampler(AncestralSampler):
    """reference sampling.py:455-494: second-order singlestep DPM-Solver++ with the midpoint evaluation at
    to_sigma(t + h/2) — 2 evaluations per step, 1 where sigma_down = 0"""

    def step_plan(self, sig, i, init_step=0):
        s, sn = float(sig[i]), float(sig[i + 1])
        down, up = ancestral_step(s, sn, self.eta)
        kn = self._noise_coef(sn, up)
        if down < 1e-14:
            kx, kd = _euler_to(s, down)
            return (Eval(s, "x", "x", kx=kx, kd=kd, kn=kn),)
        t, t_next = -np.log(s), -np.log(down)
        h = t_next - t
        s_mid = t + 0.5 * h
        m1 = float(np.exp(-s_mid) / np.exp(-t))
        m2 = float(np.expm1(-0.5 * h))
        m3 = float(np.exp(-t_next) / np.exp(-t))
        m4 = float(np.expm1(-h))
        return (Eval(s, "x", "t", kx=m1, kd=-m2),                                   # x2 = m1*x - m2*den
                Eval(float(np.exp(-s_mid)), "t", "x", kd=-m4, aux="x", ka=m3, kn=kn))   # m3*x - m4*den2 (+ noise)


class DPMPP2MSampler(_PlanSampler, BaseDiffusionSampler):
    """reference sampling.py:497-567: second-order multistep DPM-Solver++ — 1 evaluation per step; the previous step's
    denoised latent is the history (two static buffers, ping-pong by step parity)"""

    def step_plan(self, sig, i, init_step=0):
        s, sn = float(sig[i]), float(sig[i + 1])
        hist, old = f"h{i % 2}", f"h{(i - 1) % 2}"
        if sn < 1e-14:                                   # log 0: m1 = 0, m2 = -1 -> x = den
            return (Eval(s, "x", "x", kx=0.0, kd=1.0, den_out=hist),)
        t, t_next = -np.log(s), -np.log(sn)
        h = t_next - t
        m1 = float(np.exp(-t_next) / np.exp(-t))
        m2 = float(np.expm1(-h))
        if i == init_step:                               # no history yet: x_standard
            return (Eval(s, "x", "x", kx=m1, kd=-m2, den_out=hist),)
        r = (t - (-np.log(float(sig[i - 1])))) / h
        m3, m4 = 1.0 + 1.0 / (2.0 * r), 1.0 / (2.0 * r)
        return (Eval(s, "x", "x", kx=m1, kd=-m2 * m3, prev=old, kp=m2 * m4, den_out=hist),)


MULTISTEP_MAX_ORDER = 8                                  # udt_multistep_coefs holds 8 terms (UDT_MULTISTEP_MAX)


def linear_multistep_coeff(order: int, t, i: int, j: int) -> float:
    """reference sampling_utils.linear_multistep_coeff: the integral over [t[i], t[i+1]] of the Lagrange basis polynomial of node
    t[i-j] on the nodes t[i], ..., t[i-order+1] — integrated exactly, in closed form, in float64 (the reference calls
    scipy.integrate.quad, which is exact for these polynomials up to rounding).  The variable is shifted by t[i] so that the
    polynomial's coefficients stay on the scale of the step."""
    if order - 1 > i:
        raise ValueError(f"Order {order} too high for step {i}")
    t = np.asarray(t, dtype=np.float64)
    a = t[i]
    others = [k for k in range(order) if k != j]
    p = np.polynomial.polynomial.polyfromroots([t[i - k] - a for k in others]) if others else np.array([1.0])
    den = float(np.prod([t[i - j] - t[i - k] for k in others]))
    q = np.polynomial.polynomial.polyint(p)                # q(0) = 0
    return float(np.polynomial.polynomial.polyval(t[i + 1] - a, q) / den)


class LinearMultistepSampler(_PlanSampler, BaseDiffusionSampler):
    """reference sampling.py:180-215: the linear multistep method over the last ``order`` derivatives d = to_d(x, sigma, den) —
    1 evaluation per step.  Step i uses cur_order = min(i - init_step + 1, order) terms with linear_multistep_coeff weights
    computed on the host from the fp32 schedule; the derivatives live in a ring of ``order`` static buffers d{i % order}, and
    every evaluation ends in one udt_cfg_multistep_step launch.  Draws no noise.

    REFERENCE QUIRK (not copied): the reference's __call__ calls its first argument as a bare denoiser,
    ``denoiser(*guider.prepare_inputs(x, sigma, cond, uc), **kwargs)``, and forwards every other keyword (init_step included)
    into that call — unlike its other samplers, which take the engine.  Here, as for the other samplers, the first argument is
    the engine and init_step starts the loop at step init_step with an empty history."""

    def __init__(self, order=4, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.order = order

    def _check_fast_path(self, model=None):
        super()._check_fast_path(model)
        if not 1 <= int(self.order) <= MULTISTEP_MAX_ORDER:
            raise NotImplementedError(f"LinearMultistepSampler order {self.order}: the fused step (udt_cfg_multistep_step) "
                                      f"holds 1..{MULTISTEP_MAX_ORDER} derivatives")

    def step_plan(self, sig, i, init_step=0):
        order = int(self.order)
        cur = min(i - init_step + 1, order)
        ks = [linear_multistep_coeff(cur, sig, i, j) for j in range(cur)]
        slot = lambda m: f"d{m % order}"
        return (MultistepEval(float(sig[i]), "x", "x", slot(i), ks[0], tuple((slot(i - j), ks[j]) for j in range(1, cur))),)
