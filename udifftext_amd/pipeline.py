"""Inference driver: the reference's ``util.py`` (init_model / init_sampling / prepare_batch, :7-78) and
``test.py:predict`` (:19-40) restated against the MI355X ``sgm`` package, for synthetic batches.

The reference's own ``test.py`` needs datasets, checkpoints and packages that do not exist here
(SURVEY.md §8b); this module is the shipped equivalent of its hot path and is what bench.py times.
"""
from __future__ import annotations

import contextlib
import time
from typing import Optional, Tuple

import torch

import udifftext_amd  # noqa: F401  (puts the sgm mirror on sys.path)
from udifftext_amd import config as C
from udifftext_amd import rng, synth


def build_engine(device: torch.device, synthetic_weights: bool = True, verbose: bool = False, denoiser: Optional[dict] = None):
    """instantiate the DiffusionEngine from the (code-built) model config, fill deterministic synthetic weights
    (there are no checkpoints here), move it to the GPU, eval + freeze — reference util.py:7-22.  ``denoiser``: a
    ``config.denoiser_config(...)`` dict (v-prediction, EDM, the continuous Denoiser) in place of the default eps one."""
    from sgm.util import instantiate_from_config, skip_param_init
    t0 = time.time()
    cfg = C.default_model_config(denoiser)
    if synthetic_weights:
        with skip_param_init():
            model = instantiate_from_config(cfg.model)
        synth.fill_module_(model)
    else:
        model = instantiate_from_config(cfg.model)
    model.to(device)
    model.eval()
    model.freeze()
    if verbose:
        n = sum(p.numel() for p in model.parameters())
        print(f"[pipeline] engine with {n / 1e6:.1f} M parameters ready in {time.time() - t0:.1f}s")
    return model


SAMPLERS = {
    "euler": "EulerEDMSampler",
    "dpmpp2m": "DPMPP2MSampler",
    "heun": "HeunEDMSampler",
    "euler_a": "EulerAncestralSampler",
    "dpmpp2s_a": "DPMPP2SAncestralSampler",
    "linear_multistep": "LinearMultistepSampler",
}
GUIDERS = {"vanilla_cfg": "VanillaCFG", "identity": "IdentityGuider"}
DISCRETIZATIONS = {"legacy_ddpm": "LegacyDDPMDiscretization", "edm": "EDMDiscretization"}


def init_sampling(steps: int, scale: float, device: torch.device, verbose: bool = False, sampler: str = "euler", *,
                  s_churn: float = 0.0, s_tmin: float = 0.0, s_tmax: float = 999.0, s_noise: float = 1.0,
                  guider: str = "vanilla_cfg", discretization: str = "legacy_ddpm", discretization_params: Optional[dict] = None):
    """reference util.py:24-47: EulerEDMSampler + LegacyDDPMDiscretization + VanillaCFG(scale).  ``sampler`` picks another
    sampler of the reference's sampling.py with the same discretization and guider (SAMPLERS; their default parameters:
    eta = s_noise = 1 for the ancestral ones, order = 4 for linear_multistep).  ``s_churn`` / ``s_tmin`` / ``s_tmax`` / ``s_noise``
    (the Karras churn settings, reference sampling.py:89-98) go to "euler" and "heun"; Euler runs s_churn > 0, Heun refuses it.
    ``guider``: "vanilla_cfg" (VanillaCFG(scale)) or "identity" (IdentityGuider: unguided, the UNet runs on the conditional rows
    only and ``scale`` is not used); ``discretization``: "legacy_ddpm" or "edm" (EDMDiscretization), with ``discretization_params``
    as its constructor arguments"""
    from sgm.modules.diffusionmodules import sampling as S
    if sampler not in SAMPLERS:
        raise ValueError(f"unknown sampler {sampler!r}; one of {sorted(SAMPLERS)}")
    if guider not in GUIDERS:
        raise ValueError(f"unknown guider {guider!r}; one of {sorted(GUIDERS)}")
    if discretization not in DISCRETIZATIONS:
        raise ValueError(f"unknown discretization {discretization!r}; one of {sorted(DISCRETIZATIONS)}")
    disc = {"target": "sgm.modules.diffusionmodules.discretizer." + DISCRETIZATIONS[discretization]}
    if discretization_params:
        disc["params"] = dict(discretization_params)
    guide = {"target": "sgm.modules.diffusionmodules.guiders." + GUIDERS[guider]}
    if guider == "vanilla_cfg":
        guide["params"] = {"scale": scale}
    common = dict(num_steps=steps, discretization_config=disc, guider_config=guide, verbose=verbose, device=device)
    if sampler in ("euler", "heun"):
        common.update(s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise)
    return getattr(S, SAMPLERS[sampler])(**common)


def _copy_batch(batch: dict) -> dict:
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.clone()
        elif isinstance(v, (tuple, list)):
            out[k] = list(v)
        else:
            out[k] = v
    return out


def prepare_batch(batch: dict, device: torch.device) -> Tuple[dict, dict]:
    """reference util.py:62-78: tensors to the device; the unconditional batch has empty labels / prompts"""
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            batch[k] = v.to(device)
    buc = _copy_batch(batch)
    buc["txt"] = batch["ntxt"] if "ntxt" in batch else ["" for _ in batch["txt"]]
    if "label" in batch:
        buc["label"] = ["" for _ in batch["label"]]
    # host-side knowledge for the conditioner: every tensor of buc is a clone of batch's (it then shares the masked-image
    # encoder pass between c and uc without comparing the two tensors on the device)
    # The marker is only as good as the tensors it was made for: it records (identity, version counter) of both sides per key, and
    # the conditioner falls back to comparing the tensors when either was replaced or written to since (e.g. a caller that gives the
    # unconditional batch a different masked image between prepare_batch and get_unconditional_conditioning).
    buc["_udt_clone_of"] = batch
    buc["_udt_changed"] = ("txt", "label")
    buc["_udt_clone_state"] = {k: (id(buc[k]), buc[k]._version, id(v), v._version) for k, v in batch.items() if isinstance(v, torch.Tensor)}
    return batch, buc


@torch.no_grad()
def predict(cfgs, model, sampler, batch: dict, device: Optional[torch.device] = None):
    """reference test.py:19-40 -> (samples in [0,1] fp32 NCHW, latent z)"""
    device = device or next(model.parameters()).device
    batch, batch_uc = prepare_batch(batch, device)
    c, uc = model.conditioner.get_unconditional_conditioning(
        batch, batch_uc=batch_uc, force_uc_zero_embeddings=cfgs.force_uc_zero_embeddings)
    x = sampler.get_init_noise(cfgs, model, cond=c, batch=batch, uc=uc)
    z = sampler(model, x=x, cond=c, batch=batch, uc=uc, init_step=cfgs.init_step, aae_enabled=cfgs.aae_enabled,
                detailed=cfgs.detailed)
    img = model.decode_first_stage(z)
    return torch.clamp((img + 1.0) / 2.0, min=0.0, max=1.0), z


IN_FLIGHT = 3      # launch streams sampling concurrently in predict_many (same-box on MI355X, batches of 4 at 512x512:
#                    1 -> 5.7, 2 -> 7.13, 3 -> 7.67, 4 -> 6.0 images/s; 1 = one at a time)
FUSE = 0           # batches concatenated into one sampling batch per stream; 0 = automatic: the list is spread over
#                    the streams, at most 4 batches per sampling batch (dynamic batching: 8 images per UNet call
#                    cost 2.87 ms per step and image against 3.6 ms for 4, MI355X; per-sample statistics only, so every
#                    image's result depends on its own inputs alone)


def _cat_cond(conds):
    out = {}
    for k in conds[0]:
        v = conds[0][k]
        out[k] = torch.cat([c[k] for c in conds], 0) if isinstance(v, torch.Tensor) else v
        if isinstance(v, torch.Tensor) and all(getattr(c[k], "_udt_all_zero", False) for c in conds):
            out[k]._udt_all_zero = True          # (host-side tag of force-zeroed embeddings, GeneralConditioner.forward)
    return out


def _image_hw(batch: dict) -> tuple:
    """(H, W) of a batch's images, read as parallel.predict_sharded reads it"""
    if "target_size_as_tuple" in batch:
        return tuple(int(v) for v in batch["target_size_as_tuple"][0])
    return tuple(int(v) for v in batch["image"].shape[-2:])


_LANE_STREAMS: dict = {}


def _lane_streams(device: torch.device, n: int):
    key = (device.index, n)
    if key not in _LANE_STREAMS:
        _LANE_STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
    return _LANE_STREAMS[key]


def _form_batch(cfgs, model, sampler, batches, image_seeds, idx, device, masks=False):
    """one sampling batch from the input batches ``idx`` of a unit: per input batch — in the order and from the generator that
    ``predict`` batch by batch would use, inside rng.per_image when ``image_seeds`` are given — conditioning,
    get_init_noise and, right after it, the run's step noise (ancestral / churned samplers); then the one-image-size check and the
    concatenation.  -> (x, cond, uc, fb, kw, sizes, parts): fb is None, or with ``masks`` the dict of ``mask`` / ``seg_mask``
    concatenated over the unit (attend-and-excite reads them); kw holds ``noise`` [steps, fused batch, 4, h, w] where the sampler
    draws any; sizes are the images per input batch, parts the per-batch tensors (a lane keeps them alive)."""
    draw_noise = getattr(sampler, "draw_step_noise", None)
    xs, cs, ucs, noises, bs = [], [], [], [], []
    for gi in idx:
        b, buc = prepare_batch(batches[gi], device)
        seeds = image_seeds[gi] if image_seeds is not None else None
        with (rng.per_image(seeds) if seeds is not None else contextlib.nullcontext()):
            c, uc = model.conditioner.get_unconditional_conditioning(
                b, batch_uc=buc, force_uc_zero_embeddings=cfgs.force_uc_zero_embeddings)
            xs.append(sampler.get_init_noise(cfgs, model, cond=c, batch=b, uc=uc))
            if draw_noise is not None:
                noises.append(draw_noise(xs[-1].shape, xs[-1].device, None, cfgs.init_step))
        cs.append(c)
        ucs.append(uc)
        bs.append(b)
    if any(x.shape[1:] != xs[0].shape[1:] for x in xs):
        raise ValueError("batches fused into one sampling batch need one image size (use fuse=1)")
    cat = lambda ts, dim=0: torch.cat(ts, dim) if len(ts) > 1 else ts[0]
    cat_cond = lambda ds: _cat_cond(ds) if len(ds) > 1 else ds[0]
    kw = {"noise": cat(noises, 1)} if noises and noises[0] is not None else {}
    fb = {k: cat([b[k] for b in bs]) for k in ("mask", "seg_mask")} if masks else None
    return cat(xs), cat_cond(cs), cat_cond(ucs), fb, kw, [x.shape[0] for x in xs], (xs, cs, ucs, noises)


def _split(img, z, sizes, maps=None):
    """the fused batch's outputs back per input batch (triples with the character maps of a ``cfgs.detailed`` run)"""
    bounds = [sum(sizes[:k]) for k in range(len(sizes) + 1)]
    if maps is not None:
        return [(img[a:b], z[a:b], maps[a:b]) for a, b in zip(bounds, bounds[1:])]
    return [(img[a:b], z[a:b]) for a, b in zip(bounds, bounds[1:])]


def _map_size(map_size, img):
    """``predict_many``'s map_size -> None | (H, W)"""
    if map_size is None:
        return None
    if isinstance(map_size, str):
        if map_size != "image":
            raise ValueError(f"map_size must be None, 'image' or (H, W), not {map_size!r}")
        return tuple(int(v) for v in img.shape[-2:])
    H, W = (int(v) for v in map_size)
    if H < 1 or W < 1:
        raise ValueError(f"map_size {map_size!r}: both sides must be at least 1")
    return H, W


def _resize_maps(maps, map_size, img):
    """character maps [B, L, h, w] at ``map_size`` (udt_resize_bilinear_f32: one launch for all planes, on the current stream)"""
    hw = _map_size(map_size, img)
    if hw is None or maps is None:
        return maps
    from udifftext_amd import ops
    return ops.resize_bilinear(maps.contiguous(), hw)


def save_char_maps(maps, labels, names, out_dir="./temp/seg_map"):
    """the file ``EulerEDMSampler.save_segment_map`` writes (reference sampling.py:254-262), one per image: maps [B, L, h, w] (one
    batch of ``predict_many``'s third output), labels / names one string per image -> ``out_dir``/seg_<name>.npy holding the first
    len(label) planes, fp32 [len(label), h, w].  Host side only; returns the paths."""
    import os

    import numpy as np
    arr = maps.detach().float().cpu().numpy() if isinstance(maps, torch.Tensor) else np.asarray(maps, dtype=np.float32)
    if not (arr.ndim == 4 and arr.shape[0] == len(labels) == len(names)):
        raise ValueError(f"maps {arr.shape} for {len(labels)} labels and {len(names)} names")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for m, label, name in zip(arr, labels, names):
        if len(label) > m.shape[0]:
            raise ValueError(f"label {label!r} has {len(label)} characters, the maps hold {m.shape[0]}")
        paths.append(os.path.join(out_dir, f"seg_{name}.npy"))
        np.save(paths[-1], np.stack([m[i] for i in range(len(label))]) if len(label) else m[:0])
    return paths


def _predict_many_aae(cfgs, model, sampler, sample_rows, batches, units, device, image_seeds, record_losses, map_size=None):
    """the attend-and-excite branch of ``predict_many``: sampling batch after sampling batch on the current stream (see there)"""
    from udifftext_amd import ops
    out = []
    for idx in units:
        with ops.launch_context(cu_share=1):
            fx, fc, fuc, fb, kw, sizes, _ = _form_batch(cfgs, model, sampler, batches, image_seeds, idx, device, masks=True)
            if cfgs.detailed:
                kw["char_maps"] = True
            z = sample_rows(model, fx, fc, fb, fuc, init_step=cfgs.init_step, record_losses=record_losses, **kw)
            z, maps = z if cfgs.detailed else (z, None)
            img = torch.clamp((model.decode_first_stage(z) + 1.0) / 2.0, min=0.0, max=1.0)
            maps = _resize_maps(maps, map_size, img)
        out.extend(_split(img, z, sizes, maps))
    if torch.device(device).type == "cuda":
        ops.check_async_errors()
    return out


def predict_many(cfgs, model, sampler, batches, device: Optional[torch.device] = None, in_flight: Optional[int] = None,
                 fuse: Optional[int] = None, image_seeds: Optional[list] = None, record_losses: bool = True, map_size=None):
    """``predict`` over a list of batches in throughput mode: ``fuse`` consecutive batches are concatenated into one
    sampling batch, and up to ``in_flight`` such batches are processed concurrently, each on its own launch stream
    (a lane): conditioning (VAE encoder, label encoder), the sampling loop's hipGraph replays (EulerEDMSampler.sample_lane)
    and the VAE decode of a batch are enqueued back to back on its lane's stream; the lanes run free of each other and the
    host only synchronises once, at the end.
    Conditioning and noise draws stay per input batch, in the order and from the CPU generator that calling
    ``predict`` batch by batch would use; decoding runs on the fused batch.  With automatic fusing (``fuse`` 0) only consecutive
    batches of one image size are joined; an explicit ``fuse`` > 1 over batches of different sizes raises ValueError.
    ``image_seeds[k]`` (optional): one seed per image of batch k — its draws then come from per-image generators
    (``rng.per_image``), independent of batching and sharding.  Returns [(samples, z), ...] in input order.
    ``cfgs.aae_enabled`` (attend-and-excite; EulerEDMSampler): the sampling batches are formed in the same way, but run ONE AT A TIME
    on the caller's stream, planned for the whole chip — no lanes, ``in_flight`` only enters the automatic fuse count: the update
    loop reads one word back per iterated update, and a host blocked on that read cannot feed other lanes.  Every image runs its own
    update loop inside the fused batch (EulerEDMSampler.attend_and_excite_rows), so its result still depends on its own inputs
    alone.  ``record_losses`` goes to the sampler (per-row local losses of every step in ``sampler.last_row_losses``, of the last
    sampling batch).
    ``cfgs.detailed`` (the reference's per-character attention maps, sampling.py:344-346,380): every output becomes
    (samples, z, maps) with maps fp32 [B_k, L, h_map, w_map] — for EVERY image, the head mean of the configured t_attn layers'
    probabilities at the middle step, written by that step's fused text attention inside the replayed graph
    (udt_tattn_fused_maps); samples and z have the bits of the run without ``detailed``.  ``map_size``: None (the layer's own
    grid), "image" or (H, W) — the maps resized bilinearly on the lane before the final synchronisation
    (udt_resize_bilinear_f32).  ``save_char_maps`` writes the reference's seg_<name>.npy files from them.  ValueError, before
    anything is sampled, when cfgs.init_step lies behind the middle step; NotImplementedError for a sampler that hands back no
    maps.  With ``cfgs.aae_enabled`` too, the maps are the same reduction of the probabilities the middle step cached."""
    from udifftext_amd import ops
    device = device or next(model.parameters()).device
    n = max(1, int(in_flight if in_flight is not None else IN_FLIGHT))
    f = int(fuse if fuse is not None else FUSE)
    auto = f <= 0
    if auto:
        f = min(4, max(1, -(-len(batches) // n)))
    detailed = bool(cfgs.detailed)
    if detailed:
        if not hasattr(sampler, "char_map_step"):
            raise NotImplementedError(f"cfgs.detailed in predict_many needs a sampler that hands back character maps "
                                      f"(char_map_step, sample_lane(char_maps=True)), not {type(sampler).__name__}")
        sampler.char_map_step(cfgs.init_step)              # ValueError: the run would start behind the step that emits the maps
    elif map_size is not None:
        raise ValueError("map_size resizes the character maps of a cfgs.detailed run; cfgs.detailed is not set")
    _map_size(map_size, torch.empty((1, 1)))               # (a malformed map_size raises before anything is sampled)
    aae_sampler = getattr(sampler, "sample_rows_with_attend_and_excite", None) if cfgs.aae_enabled else None
    if cfgs.aae_enabled and aae_sampler is None:
        raise NotImplementedError(f"attend-and-excite in predict_many needs a sampler with sample_rows_with_attend_and_excite "
                                  f"(EulerEDMSampler), not {type(sampler).__name__}")
    # (host logic only below; with a stub engine on the CPU — tests/test_parallel_cpu.py — there are no streams)
    gpu = torch.device(device).type == "cuda"
    main = torch.cuda.current_stream(device) if gpu else None
    lanes = (_lane_streams(device, n) if n > 1 else [main]) if gpu else [None] * n
    on = (lambda lane: torch.cuda.stream(lane)) if gpu else (lambda lane: contextlib.nullcontext())
    after = (lambda a, b: a.wait_stream(b)) if gpu else (lambda a, b: None)       # stream a continues after stream b
    out, checks, keep = [], [], []
    # FREE-RUNNING lanes (round 4): sampling batch u runs on lane u % n — conditioning, the sampling loop's graph replays and
    # the decode are enqueued back to back on the lane's stream, with no event shared between lanes: a lane starts its next
    # batch the moment its previous decode is done, and the conditioning / decode phases of one lane (eager launches, ~25 ms)
    # run beside the other lanes' sampling.  Nothing below synchronises the host: the noise draws travel through pinned
    # memory (rng.randn_on), the zero-context test and the c / uc image comparison are host-side flags.  (Round 3 ran the
    # lanes in lock-stepped groups with a cross-lane join before and after every sampling loop: ~35 ms of each 1.28 s group
    # had no sampling running, and a slow lane held the others.)
    lane_sampler = getattr(sampler, "sample_lane", None)
    if auto:
        # automatic fusing joins consecutive batches only while their image size is equal (one size per sampling batch, as the
        # reference's target_size_as_tuple[0]): a list of mixed sizes works; an explicit fuse > 1 over mixed sizes raises below
        units = []
        for i, b in enumerate(batches):
            if units and len(units[-1]) < f and _image_hw(batches[units[-1][0]]) == _image_hw(b):
                units[-1].append(i)
            else:
                units.append([i])
    else:
        units = [list(range(i, min(i + f, len(batches)))) for i in range(0, len(batches), f)]
    if aae_sampler is not None:
        return _predict_many_aae(cfgs, model, sampler, aae_sampler, batches, units, device, image_seeds, record_losses, map_size)
    # lanes in use: as few as keep every lane equally loaded — 4 sampling batches on 3 lanes run as 2 + 2 on TWO lanes (each planned
    # for half of the CUs), not as 2 + 1 + 1 with the 4th batch alone on a lane planned for a third of the chip while two lanes idle
    rounds = -(-len(units) // n) if units else 1
    n_used = max(1, -(-len(units) // rounds)) if units else 1
    for lane in lanes[:n_used]:
        after(lane, main)
    for u, idx in enumerate(units):
        lane = lanes[u % n_used]
        with on(lane), ops.launch_context(cu_share=n_used):
            fx, fc, fuc, _, kw, sizes, parts = _form_batch(cfgs, model, sampler, batches, image_seeds, idx, device)
            if detailed:
                kw["char_maps"] = True
            if lane_sampler is not None:
                z = lane_sampler(model, fx, fc, fuc, slot=u % n_used, n_lanes=n_used, init_step=cfgs.init_step, deferred_checks=checks,
                                 **kw)
            else:       # (stub samplers of the CPU tests: the group interface, one batch at a time)
                cm = {"char_maps": True} if detailed else {}
                z = sampler.sample_in_flight(model, [fx], [fc], [fuc], init_step=cfgs.init_step, deferred_checks=checks, **cm)[0]
            z, maps = z if detailed else (z, None)
            img = torch.clamp((model.decode_first_stage(z) + 1.0) / 2.0, min=0.0, max=1.0)
            maps = _resize_maps(maps, map_size, img)
        keep.append((parts, fx, fc, fuc, z, maps))             # tensors of a lane stream: alive until the final synchronisation
        out.extend(_split(img, z, sizes, maps))
    for lane in lanes:
        after(main, lane)
    for chk in checks:
        chk()
    if gpu:
        ops.check_async_errors()
    if hasattr(sampler, "release_retired"):             # (the checks above synchronised every lane: evicted graph runners may go)
        sampler.release_retired()
    del keep
    return out


def _host_boxes(batch: dict, k: int):
    """(labels, [B, 4] int64 host boxes) of batch k, validated against its image size"""
    if "r_bbox" not in batch:
        raise ValueError(f"batch {k} has no r_bbox: evaluate needs the text box of every image")
    if "label" not in batch:
        raise ValueError(f"batch {k} has no label")
    rb = batch["r_bbox"]
    if isinstance(rb, torch.Tensor) and rb.is_cuda:
        raise ValueError(f"batch {k}: r_bbox is on the GPU; evaluate reads box values on the host only")
    rb = torch.as_tensor(rb).reshape(-1, 4).to(torch.int64)
    labels = list(batch["label"])
    if rb.shape[0] != len(labels):
        raise ValueError(f"batch {k}: {rb.shape[0]} boxes for {len(labels)} labels")
    H, W = _image_hw(batch)
    for i, (t, b, l, r) in enumerate(rb.tolist()):
        if not (0 <= t < b <= H and 0 <= l < r <= W):
            raise ValueError(f"batch {k}, image {i}: box rows {t}:{b}, columns {l}:{r} does not lie in its {H} x {W} image")
    return labels, rb


def _lpips_shapes(batches, lpips) -> None:
    """host check of ``lpips_of``'s inputs before anything is sampled: every batch has a [B, 3, H, W] image large enough for the taps"""
    for k, batch in enumerate(batches):
        img = batch.get("image")
        if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"batch {k} has no [B, 3, H, W] image: LPIPS compares every generated frame with it")
        if hasattr(lpips, "map_sizes"):                    # (ValueError: a frame too small for the module's taps)
            lpips.map_sizes(*img.shape[-2:])


@torch.no_grad()
def lpips_of(outputs, batches, lpips, chunk: int = 32) -> list:
    """LPIPS of every generated frame against the image it was made from (reference metrics.py:12-30 on the frames test.py saves):
    ``outputs`` is ``predict_many``'s list (only the samples are read), ``batches`` the batches it was given (their ``image``,
    [-1, 1]); ``lpips(samples, images) -> [n]`` is called on chunks of at most ``chunk`` consecutive pairs of one image size — a
    chunk may span batches, and ends where the size changes.  Nothing synchronises per image: the chunks' results stay on the device
    and ONE device-to-host copy at the end brings them back.  -> per batch, in input order, a list of floats.
    Per image, not per width-concatenated batch: see udifftext_amd/lpips_alex.py."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be a positive count, not {chunk!r}")
    if len(outputs) != len(batches):
        raise ValueError(f"{len(outputs)} outputs for {len(batches)} batches")
    vals, cur_s, cur_i, hw, count = [], [], [], None, 0

    def flush():
        nonlocal count
        if cur_s:
            vals.append(lpips(torch.cat(cur_s, 0) if len(cur_s) > 1 else cur_s[0], torch.cat(cur_i, 0) if len(cur_i) > 1 else cur_i[0]))
        cur_s.clear()
        cur_i.clear()
        count = 0

    for k, (o, b) in enumerate(zip(outputs, batches)):
        s, im = o[0], b["image"]
        if tuple(s.shape) != tuple(im.shape):
            raise ValueError(f"batch {k}: samples {tuple(s.shape)} and image {tuple(im.shape)} differ in shape")
        if hw is not None and tuple(s.shape[-2:]) != hw:
            flush()
        hw = tuple(s.shape[-2:])
        im = im.to(s.device, non_blocking=True)
        i = 0
        while i < s.shape[0]:
            take = min(chunk - count, s.shape[0] - i)
            cur_s.append(s[i:i + take])
            cur_i.append(im[i:i + take])
            count += take
            i += take
            if count == chunk:
                flush()
    flush()
    flat = torch.cat([v.reshape(-1).float() for v in vals]).cpu().tolist() if vals else []
    per, o = [], 0
    for out in outputs:
        n = int(out[0].shape[0])
        per.append(flat[o:o + n])
        o += n
    if o != len(flat):
        raise RuntimeError(f"the LPIPS module returned {len(flat)} values for {o} pairs")
    return per


@torch.no_grad()
def fid_of(outputs, batches, fid, chunk: int = 32):
    """the FID statistics of every generated frame (the fake set) and of the image it was made from (the real set) — reference
    metrics.py:5-10 on the frames test.py saves: ``outputs`` is ``predict_many``'s list (only the samples are read), ``batches`` the
    batches it was given (their ``image``, [-1, 1]); ``fid`` a ``udifftext_amd.fid_inception.FID``.  The pairs go through
    ``FIDStats.update`` in chunks of at most ``chunk`` consecutive pairs of one image size, as ``lpips_of`` forms them; nothing is
    copied to the host.  -> the ``FIDStats`` (``compute()`` is the distance, ``state()`` what ranks add)."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be a positive count, not {chunk!r}")
    if len(outputs) != len(batches):
        raise ValueError(f"{len(outputs)} outputs for {len(batches)} batches")
    stats = fid.stats()

    def feed(samples, images):
        stats.update(samples, images)
        return samples.new_zeros((samples.shape[0],))

    lpips_of(outputs, batches, feed, chunk=chunk)              # (its chunk former; the zeros it gathers are dropped)
    return stats


@torch.no_grad()
def evaluate(cfgs, model, sampler, batches, predictor, device: Optional[torch.device] = None, in_flight: Optional[int] = None,
             fuse: Optional[int] = None, image_seeds: Optional[list] = None, ocr_batch: Optional[int] = 64,
             return_samples: bool = False, lpips=None, lpips_chunk: int = 32, fid=None, fid_chunk: int = 32) -> dict:
    """reference test.py:74-91 in throughput mode: generate with ``predict_many``, read the text back with the OCR predictor, count
    the exact matches — the sequence accuracy UDiffText is judged by.
    Every batch carries ``label`` (one string per image) and ``r_bbox`` ([B, 4] host integers: top, bottom, left, right of the text
    box, the slice results[i, :, top:bottom, left:right] of test.py:81).  Labels and boxes are taken, and the boxes validated against the
    batch's image size, on the HOST before anything is sampled (ValueError; a batch without r_bbox is one) — box values are never
    read back from the GPU.  ``predict_many`` then runs unchanged (``in_flight``, ``fuse``, ``image_seeds``, cfgs.aae_enabled as
    there).  Each returned batch's boxes are cropped, resized and normalised in one launch (``predictor.transform_boxes``); the crops
    are concatenated in input order and read in consecutive chunks of at most ``ocr_batch`` (``predictor.txt_of``: one autoregressive
    decoding loop per chunk); ``ocr_batch=None``: one chunk per input batch, the reference's grouping.  An image is correct when
    pred.lower() == label.lower() (test.py:84).
    -> {"accuracy", "correct", "total", "pred": [[str]], "label": [[str]]} (per batch, input order) and, with ``return_samples``,
    "outputs": the ``predict_many`` list.  ``predictor`` is duck-typed: only ``transform_boxes`` and ``txt_of`` are used.
    One device only: under data parallelism each rank calls ``evaluate`` on its shard and the ranks add up "correct" and "total".
    ``lpips`` (a ``udifftext_amd.lpips_alex.LPIPS``, or anything callable as lpips(samples, images) -> [n]): the reference's second
    measurement (test.py:122-124) on the same frames — the result also carries "lpips" (the mean over all images), "lpips_sum"
    (ranks add "lpips_sum" and "total") and "lpips_per_image" (per batch, input order), from ``lpips_of`` in chunks of
    ``lpips_chunk`` pairs.  Without it nothing changes: the same keys, the same launches, the same samples.
    ``fid`` (a ``udifftext_amd.fid_inception.FID``): the reference's third measurement (test.py:119-121) on the same frames, fake set =
    the samples, real set = the batches' images, from ``fid_of`` in chunks of ``fid_chunk`` pairs — the result also carries "fid" (a
    float; None with "fid_note" when fewer than 2 images leave no covariance) and "fid_stats" (``FIDStats.state()``: n, sum, outer
    per set as CPU float64 tensors; ranks add them and call ``FIDStats.from_state(...).compute()``).  "fid_note" also says when
    total < 2048 leaves the covariances rank-deficient, as pytorch_fid warns.  Without it nothing changes either."""
    if ocr_batch is not None and int(ocr_batch) < 1:
        raise ValueError(f"ocr_batch must be a positive count or None, not {ocr_batch!r}")
    if lpips is not None:
        if int(lpips_chunk) < 1:
            raise ValueError(f"lpips_chunk must be a positive count, not {lpips_chunk!r}")
        _lpips_shapes(batches, lpips)
    if fid is not None:
        if int(fid_chunk) < 1:
            raise ValueError(f"fid_chunk must be a positive count, not {fid_chunk!r}")
        _lpips_shapes(batches, None)
    labels, boxes = [], []
    for k, batch in enumerate(batches):
        lb, rb = _host_boxes(batch, k)
        labels.append(lb)
        boxes.append(torch.cat((torch.arange(rb.shape[0]).reshape(-1, 1), rb), 1))       # + the image's index in its batch
    outputs = predict_many(cfgs, model, sampler, batches, device, in_flight=in_flight, fuse=fuse, image_seeds=image_seeds)
    # (outputs are (samples, z), or (samples, z, maps) under cfgs.detailed: only the samples are read here)
    crops = [predictor.transform_boxes(o[0], bx) for o, bx in zip(outputs, boxes)]
    if ocr_batch is None:
        chunks = crops
    else:
        flat = torch.cat(crops, 0) if crops else None
        chunks = [flat[i:i + int(ocr_batch)] for i in range(0, flat.shape[0] if crops else 0, int(ocr_batch))]
    flat_pred = [t for x in chunks if x.shape[0] for t in predictor.txt_of(x)]
    total = sum(len(lb) for lb in labels)
    if len(flat_pred) != total:
        raise RuntimeError(f"the predictor returned {len(flat_pred)} strings for {total} crops")
    pred, o = [], 0
    for lb in labels:
        pred.append(flat_pred[o:o + len(lb)])
        o += len(lb)
    correct = sum(p.lower() == t.lower() for ps, ls in zip(pred, labels) for p, t in zip(ps, ls))
    res = {"accuracy": correct / total if total else 0.0, "correct": int(correct), "total": int(total), "pred": pred, "label": labels}
    if lpips is not None:
        per = lpips_of(outputs, batches, lpips, chunk=lpips_chunk)
        res["lpips_per_image"] = per
        res["lpips_sum"] = float(sum(v for vs in per for v in vs))
        res["lpips"] = res["lpips_sum"] / total if total else 0.0
    if fid is not None:
        stats = fid_of(outputs, batches, fid, chunk=fid_chunk)
        res["fid_stats"] = stats.state()
        if total < 2:
            res["fid"] = None
            res["fid_note"] = f"FID needs at least 2 images per set for a covariance, not {total}"
        else:
            res["fid"] = stats.compute()
            if total < stats.dim:
                res["fid_note"] = (f"{total} images for {stats.dim} features: the covariances are rank-deficient, and the number is "
                                   "not comparable with one from a larger set")
    if return_samples:
        res["outputs"] = outputs
    return res
