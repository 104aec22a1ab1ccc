"""FID on the fp32 kernels of csrc/fid.hip and csrc/lpips.hip: the third number of the reference's ``quan_test`` (test.py:119-121,
metrics.py:5-10: ``python -m pytorch_fid`` between the saved fake frames and the saved real ones).

Definition:
  1. input: per image, the 8-bit values test.py:94,102,110-113 saves — fake q = trunc(clamp(s*255)), real
     q = trunc(clamp(((x + 1)*0.5)*255)), fp32 products in that order — then ToTensor's q/255, F.interpolate to 299 x 299 (bilinear,
     align_corners=False, no antialiasing: ``udt_resize_bilinear_f32``'s coordinate rule) and 2x - 1.  ``quantise=False`` skips the trunc.
  2. network: the FID InceptionV3 up to pool3 — every BasicConv2d is conv (no bias), BatchNorm (eps 1e-3, inference form), ReLU;
     the branch pools of Mixed_5b .. Mixed_7b are the average that does not count padding, Mixed_7c's is a MAX pool; the head is the
     mean over the 8 x 8 pixels -> [N, 2048].  BatchNorm is folded into the packed weights once per module, in float64.
  3. statistics per set: n, sum x (fp64 [2048]), sum x x^T (fp64 [2048, 2048]) — streamed by ``udt_moments_accum_f64``; ranks add them.
     mu = sum/n, Sigma = (sum x x^T - n mu mu^T)/(n - 1) = np.cov(rowvar=False).
  4. distance, on the host in float64 with numpy: ``frechet_distance``.

A block's branches write straight into channel slices of ONE [N, h, w, C_total] buffer (output pointer offset, ld_out = C_total), and
a block's intermediate maps are slices of one scratch map: there is no concatenation launch.  Everything up to the features is fp32 and
deterministic; there is no fallback: without a gfx950 device the calls raise.

This file is fid_inception.py, not fid.py or pytorch_fid.py: the package's directory is first on sys.path (for the ``sgm`` mirror), so a
top-level name here must not shadow a package the reference imports (tests/test_fid_cpu.py guards it).

State-dict names are torchvision's Inception3 AS WE KNOW THEM (pytorch_fid's FID network keeps them) — neither package, nor the
published FID weights, is available to this project's tests, so ``KEY_TABLE`` is the one place that states the names and it is
unverified against the packages.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import ops, packing, synth

DIM = 2048
SIZE = 299
BN_EPS = 1e-3

Conv = namedtuple("Conv", "name cin cout kernel stride pad")
Pool = namedtuple("Pool", "average stride pad")


def _cv(name, cin, cout, kernel=(1, 1), stride=1, pad=(0, 0)):
    return Conv(name, cin, cout, tuple(kernel), stride, tuple(pad))


_AVG, _MAX, _MAX2 = Pool(True, 1, 1), Pool(False, 1, 1), Pool(False, 2, 0)

# the stem: a sequence of convolutions and 3 x 3 / 2 max-pools, 299 -> 149 -> 147 -> 147 -> 73 -> 73 -> 71 -> 35
STEM = (_cv("Conv2d_1a_3x3", 3, 32, (3, 3), 2), _cv("Conv2d_2a_3x3", 32, 32, (3, 3)), _cv("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)), _MAX2,
        _cv("Conv2d_3b_1x1", 64, 80), _cv("Conv2d_4a_3x3", 80, 192, (3, 3)), _MAX2)


# a block = branches, concatenated in this order; a branch = steps; a step = the operations that read the previous step's map (two in
# Mixed_7b/7c, whose 1x3 and 3x1 outputs are concatenated); only a branch's LAST step may hold two
def _block_a(cin, pf):
    return ([(_cv("branch1x1", cin, 64),)],
            [(_cv("branch5x5_1", cin, 48),), (_cv("branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),)],
            [(_cv("branch3x3dbl_1", cin, 64),), (_cv("branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),),
             (_cv("branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)),)],
            [(_AVG,), (_cv("branch_pool", cin, pf),)])


def _block_b(cin):
    return ([(_cv("branch3x3", cin, 384, (3, 3), 2),)],
            [(_cv("branch3x3dbl_1", cin, 64),), (_cv("branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),), (_cv("branch3x3dbl_3", 96, 96, (3, 3), 2),)],
            [(_MAX2,)])


def _block_c(cin, c7):
    r, c = ((1, 7), (0, 3)), ((7, 1), (3, 0))                # 1x7 with padding (0, 3), 7x1 with padding (3, 0)
    return ([(_cv("branch1x1", cin, 192),)],
            [(_cv("branch7x7_1", cin, c7),), (_cv("branch7x7_2", c7, c7, r[0], 1, r[1]),), (_cv("branch7x7_3", c7, 192, c[0], 1, c[1]),)],
            [(_cv("branch7x7dbl_1", cin, c7),), (_cv("branch7x7dbl_2", c7, c7, c[0], 1, c[1]),), (_cv("branch7x7dbl_3", c7, c7, r[0], 1, r[1]),),
             (_cv("branch7x7dbl_4", c7, c7, c[0], 1, c[1]),), (_cv("branch7x7dbl_5", c7, 192, r[0], 1, r[1]),)],
            [(_AVG,), (_cv("branch_pool", cin, 192),)])


def _block_d(cin):
    return ([(_cv("branch3x3_1", cin, 192),), (_cv("branch3x3_2", 192, 320, (3, 3), 2),)],
            [(_cv("branch7x7x3_1", cin, 192),), (_cv("branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)),),
             (_cv("branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),), (_cv("branch7x7x3_4", 192, 192, (3, 3), 2),)],
            [(_MAX2,)])


def _block_e(cin, pool):
    return ([(_cv("branch1x1", cin, 320),)],
            [(_cv("branch3x3_1", cin, 384),), (_cv("branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)), _cv("branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)))],
            [(_cv("branch3x3dbl_1", cin, 448),), (_cv("branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)),),
             (_cv("branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), _cv("branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)))],
            [(pool,), (_cv("branch_pool", cin, 192),)])


# name -> (input channels, branches); the 7c pool is a MAX pool in the FID network (the quirk of the weights it was published with)
BLOCKS = {
    "Mixed_5b": (192, _block_a(192, 32)), "Mixed_5c": (256, _block_a(256, 64)), "Mixed_5d": (288, _block_a(288, 64)),
    "Mixed_6a": (288, _block_b(288)),
    "Mixed_6b": (768, _block_c(768, 128)), "Mixed_6c": (768, _block_c(768, 160)), "Mixed_6d": (768, _block_c(768, 160)),
    "Mixed_6e": (768, _block_c(768, 192)),
    "Mixed_7a": (768, _block_d(768)),
    "Mixed_7b": (1280, _block_e(1280, _AVG)), "Mixed_7c": (2048, _block_e(2048, _MAX)),
}


def block_plan(cin: int, branches):
    """-> (launches, C_out, C_tmp, stride): every launch is (operation, source, destination), source and destination a
    (buffer, first channel, end channel) with buffer "x" (the block's input), "tmp" (its scratch map, C_tmp wide, at the input's size)
    or "out" (the concatenation, C_out wide)"""
    launches, out_off, tmp_off, stride = [], 0, 0, 1
    for branch in branches:
        src = ("x", 0, cin)
        for i, step in enumerate(branch):
            last = i == len(branch) - 1
            assert last or len(step) == 1
            for op in step:
                width = op.cout if isinstance(op, Conv) else src[2] - src[1]
                if last:
                    dst = ("out", out_off, out_off + width)
                    out_off += width
                    stride = max(stride, op.stride)
                else:
                    dst = ("tmp", tmp_off, tmp_off + width)
                    tmp_off += width
                launches.append((op, src, dst))
            src = dst
    return launches, out_off, tmp_off, stride


def all_convs() -> List[Tuple[str, Conv]]:
    """(state-dict prefix, layer) of the network's 94 convolutions, in execution order"""
    out = [(op.name, op) for op in STEM if isinstance(op, Conv)]
    for bname, (_, branches) in BLOCKS.items():
        out += [(f"{bname}.{op.name}", op) for br in branches for step in br for op in step if isinstance(op, Conv)]
    return out


BN_LEAVES = ("weight", "bias", "running_mean", "running_var")
# our state-dict name -> the other names a checkpoint may use for it: none — the names ARE torchvision's Inception3's, which
# pytorch_fid's FID network keeps; fc.*, AuxLogits.* and *.num_batches_tracked of such a checkpoint are ignored
KEY_TABLE: Dict[str, Tuple[str, ...]] = {}
for _prefix, _ in all_convs():
    KEY_TABLE[f"{_prefix}.conv.weight"] = ()
    for _leaf in BN_LEAVES:
        KEY_TABLE[f"{_prefix}.bn.{_leaf}"] = ()
IGNORED_PREFIXES = ("fc.", "AuxLogits.")


def ignored_key(name: str) -> bool:
    return name.startswith(IGNORED_PREFIXES) or name.endswith(".num_batches_tracked")


def map_sizes(H: int = SIZE, W: int = SIZE) -> List[Tuple[int, int]]:
    """the spatial sizes after the stem's seven stages and after Mixed_5d, Mixed_6a, Mixed_6e, Mixed_7a, Mixed_7c of an H x W network
    input (host arithmetic; the module always feeds 299 x 299); ValueError when a stage would have no pixel"""
    sizes, h, w = [], int(H), int(W)

    def step(k, s, p):
        nonlocal h, w
        h, w = (h + 2 * p[0] - k[0]) // s + 1, (w + 2 * p[1] - k[1]) // s + 1
        if h < 1 or w < 1:
            raise ValueError(f"FID: a {H} x {W} network input is too small: stage {len(sizes) + 1} would have no pixel")
        sizes.append((h, w))

    for op in STEM:
        step(op.kernel, op.stride, op.pad) if isinstance(op, Conv) else step((3, 3), op.stride, (op.pad, op.pad))
    for bname, (cin, branches) in BLOCKS.items():
        stride = block_plan(cin, branches)[3]
        if stride == 2:
            step((3, 3), 2, (0, 0))
        elif bname in ("Mixed_5d", "Mixed_6e", "Mixed_7c"):
            sizes.append((h, w))
    return sizes


def fold_bn(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, eps: float = BN_EPS):
    """inference BatchNorm folded into the convolution before it, in float64: s = gamma/sqrt(var + eps), w' = w s, b' = beta - mean s
    -> (w' float64 [Cout, Cin, kh, kw], b' float64 [Cout])"""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s.reshape(-1, 1, 1, 1), beta.double() - mean.double() * s


class _BasicConv2d(nn.Module):
    def __init__(self, op: Conv):
        super().__init__()
        self.conv = nn.Module()
        self.conv.weight = nn.Parameter(torch.zeros((op.cout, op.cin, *op.kernel)), requires_grad=False)
        self.bn = nn.Module()
        self.bn.weight = nn.Parameter(torch.ones((op.cout,)), requires_grad=False)
        self.bn.bias = nn.Parameter(torch.zeros((op.cout,)), requires_grad=False)
        self.bn.register_buffer("running_mean", torch.zeros((op.cout,)))
        self.bn.register_buffer("running_var", torch.ones((op.cout,)))


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) in float64 with numpy.  The last trace is sum_i sqrt(max(l_i, 0)) over the
    eigenvalues l_i of A S2 A, A = S1^(1/2) from ``eigh`` with negative eigenvalues clamped to zero: A S2 A is symmetric and has the
    eigenvalues of S1 S2, and the form stays defined for rank-deficient covariances (n < 2048), where pytorch_fid's
    scipy.linalg.sqrtm falls back to an eps offset on the diagonals.  Where sqrtm is well conditioned the two agree."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(-1), np.asarray(mu2, dtype=np.float64).reshape(-1)
    s1, s2 = np.asarray(sigma1, dtype=np.float64), np.asarray(sigma2, dtype=np.float64)
    d = mu1.shape[0]
    if mu2.shape != (d,) or s1.shape != (d, d) or s2.shape != (d, d):
        raise ValueError(f"frechet_distance: means {mu1.shape}, {mu2.shape} and covariances {s1.shape}, {s2.shape} do not fit")
    lam, vec = np.linalg.eigh((s1 + s1.T) * 0.5)
    a = (vec * np.sqrt(np.maximum(lam, 0.0))) @ vec.T
    m = a @ ((s2 + s2.T) * 0.5) @ a
    tr_sqrt = float(np.sqrt(np.maximum(np.linalg.eigvalsh((m + m.T) * 0.5), 0.0)).sum())
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * tr_sqrt)


class FIDStats:
    """(n, sum x, sum x x^T) of the fake set (index 0) and of the real set (index 1), fp64, on ``device``.  ``update`` streams a
    chunk of pairs through ``fid``; ``merge`` / ``state`` / ``from_state`` are how chunks, runs and ranks add up; ``compute`` is FID."""

    def __init__(self, fid: "FID" = None, dim: int = DIM, device=None):
        self.fid = fid
        if device is None:
            device = next(fid.parameters()).device if fid is not None else torch.device("cpu")
        self.n = 0
        self.sum = torch.zeros((2, dim), dtype=torch.float64, device=device)
        self.outer = torch.zeros((2, dim, dim), dtype=torch.float64, device=device)

    @property
    def dim(self) -> int:
        return int(self.sum.shape[1])

    @torch.no_grad()
    def update(self, samples: torch.Tensor, images: torch.Tensor, quantise: bool = True) -> "FIDStats":
        """samples [N, 3, H, W] in [0, 1], images [N, 3, H, W] in [-1, 1]: N more fake and N more real frames"""
        if self.fid is None:
            raise ValueError("FIDStats.update needs the FID module it was built with")
        return self.update_features(self.fid.features((samples, images), quantise=quantise))

    @torch.no_grad()
    def update_features(self, feats: torch.Tensor) -> "FIDStats":
        """feats fp32 [2 N, dim] on the device: the N fake frames' features, then the N real ones' (udt_moments_accum_f64)"""
        if feats.dim() != 2 or feats.shape[1] != self.dim or feats.shape[0] % 2 or feats.shape[0] < 2:
            raise ValueError(f"FIDStats: features {tuple(feats.shape)} are not [2 N, {self.dim}]")
        N = feats.shape[0] // 2
        for k in range(2):
            ops.moments_accum_f64(feats[k * N:(k + 1) * N], self.sum[k], self.outer[k])
        self.n += N
        return self

    def merge(self, other: "FIDStats") -> "FIDStats":
        if other.dim != self.dim:
            raise ValueError(f"FIDStats.merge: {other.dim} features against {self.dim}")
        self.n += int(other.n)
        self.sum += other.sum.to(self.sum.device)
        self.outer += other.outer.to(self.outer.device)
        return self

    def state(self) -> dict:
        """{"n": int, "sum": float64 [2, dim], "outer": float64 [2, dim, dim]} on the CPU: what ranks add"""
        return {"n": int(self.n), "sum": self.sum.detach().cpu().clone(), "outer": self.outer.detach().cpu().clone()}

    @classmethod
    def from_state(cls, state: dict, fid: "FID" = None, device=None) -> "FIDStats":
        s, o = state["sum"], state["outer"]
        if s.dtype != torch.float64 or o.dtype != torch.float64 or s.dim() != 2 or s.shape[0] != 2 or tuple(o.shape) != (2, s.shape[1], s.shape[1]):
            raise ValueError(f"FIDStats.from_state: sum {tuple(s.shape)} {s.dtype}, outer {tuple(o.shape)} {o.dtype}")
        st = cls(fid, dim=int(s.shape[1]), device=device if device is not None or fid is not None else s.device)
        st.n = int(state["n"])
        st.sum.copy_(s)
        st.outer.copy_(o)
        return st

    def moments(self):
        """-> ((mu, Sigma) of the fake set, (mu, Sigma) of the real set) as float64 numpy arrays; ValueError for n < 2"""
        if self.n < 2:
            raise ValueError(f"FID needs at least 2 images per set for a covariance, not {self.n}")
        n, out = float(self.n), []
        for k in range(2):
            mu = self.sum[k].cpu().numpy() / n
            out.append((mu, (self.outer[k].cpu().numpy() - n * np.outer(mu, mu)) / (n - 1.0)))
        return tuple(out)

    def compute(self) -> float:
        (mu1, s1), (mu2, s2) = self.moments()
        return frechet_distance(mu1, s1, mu2, s2)


class FID(nn.Module):
    """the FID InceptionV3 up to pool3.  Built with identity BatchNorms and zero convolutions: ``load_weights`` (the published FID
    Inception checkpoint, torchvision names) or ``fill_synthetic_`` fills them."""

    KEY_TABLE = KEY_TABLE
    map_sizes = staticmethod(map_sizes)

    def __init__(self, ckpt_path=None):
        super().__init__()
        for op in STEM:
            if isinstance(op, Conv):
                self.add_module(op.name, _BasicConv2d(op))
        for bname, (_, branches) in BLOCKS.items():
            blk = nn.Module()
            for br in branches:
                for step in br:
                    for op in step:
                        if isinstance(op, Conv):
                            blk.add_module(op.name, _BasicConv2d(op))
            self.add_module(bname, blk)
        if ckpt_path is not None:
            self.load_weights(torch.load(ckpt_path, map_location="cpu"))

    # ---- weights
    def load_weights(self, *state_dicts) -> None:
        """fill every tensor from the given state dicts (later ones win), each name looked up under ours and under its KEY_TABLE
        aliases; fc.*, AuxLogits.* and num_batches_tracked are ignored; KeyError names what no dict holds, ValueError a wrong shape or
        a key that is neither ours nor ignored"""
        merged = {}
        for sd in state_dicts:
            merged.update(sd)
        own = self.state_dict()
        assert set(own) == set(KEY_TABLE)
        known = {n for name, aliases in KEY_TABLE.items() for n in (name, *aliases)}
        stray = [k for k in merged if k not in known and not ignored_key(k)]
        if stray:
            raise ValueError(f"FID: the checkpoint holds tensors this network does not know: {stray[:8]}")
        new, missing = {}, []
        for name, aliases in KEY_TABLE.items():
            hit = next((merged[n] for n in (name, *aliases) if n in merged), None)
            if hit is None:
                missing.append(name)
                continue
            if tuple(hit.shape) != tuple(own[name].shape):
                raise ValueError(f"FID: {name} has shape {tuple(hit.shape)} in the checkpoint, {tuple(own[name].shape)} here")
            new[name] = hit
        if missing:
            raise KeyError(f"FID: no checkpoint tensor for {missing[:8]}{' ...' if len(missing) > 8 else ''}")
        self.load_state_dict(new, strict=True)

    def fill_synthetic_(self, prefix: str = "fid.") -> "FID":
        """synth.py's name-and-shape recipe: convolutions uniform with variance 2/fan_in (the ReLU keeps half), BatchNorm scale
        1 +- 0.1, shift and running mean +- 0.05, running variance in 0.5 .. 1.5"""
        sd = {}
        for name, t in self.state_dict().items():
            v = synth.synthetic_tensor(prefix + name, tuple(t.shape))
            if name.endswith("conv.weight"):
                v = v * (2.0 ** 0.5)
            elif name.endswith("running_var"):
                v = 1.0 + 10.0 * v                              # (the recipe's +- 0.05 for a 1-D non-"weight" tensor)
            sd[name] = v
        self.load_weights(sd)
        return self

    def _sources(self):
        return [*self.parameters(), *self.buffers()]

    def _pack(self):
        packed = {}
        for prefix, op in all_convs():
            m = self.get_submodule(prefix)
            w, b = fold_bn(m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)
            packed[prefix] = (packing.pack_conv_f32(w.float()), b.float().contiguous())       # (rounded to fp32 once, here)
        return packed

    def packed(self) -> dict:
        """state-dict prefix -> (packed folded weights fp32 [Cout, Kp], folded bias fp32 [Cout]), in the per-module cache (rebuilt when
        a weight changes pointer, version or device)"""
        from sgm.modules import hipnn
        return hipnn.layout(self, "fid_f32", self._pack)

    # ---- the network
    @staticmethod
    def _conv(x, op: Conv, wb, out=None):
        return ops.conv2d_rect_f32(x, wb[0], wb[1], op.cout, op.kernel, op.stride, op.pad, relu=True, out=out)

    def run_block(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """one Mixed_* block on a channels-last fp32 map [N, h, w, Cin] -> [N, h', w', C_out]"""
        cin, branches = BLOCKS[name]
        if x.shape[3] != cin:
            raise ValueError(f"FID: {name} reads {cin} channels, not {x.shape[3]}")
        packed = self.packed()
        launches, c_out, c_tmp, stride = block_plan(cin, branches)
        N, h, w, _ = x.shape
        ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if stride == 2 else (h, w)
        if ho < 1 or wo < 1:
            raise ValueError(f"FID: {name} on a {h} x {w} map has no output pixel")
        bufs = {"x": x, "out": torch.empty((N, ho, wo, c_out), dtype=torch.float32, device=x.device),
                "tmp": torch.empty((N, h, w, max(c_tmp, 1)), dtype=torch.float32, device=x.device)}
        for op, (sb, s0, s1), (db, d0, d1) in launches:
            src, dst = bufs[sb][..., s0:s1], bufs[db][..., d0:d1]
            if isinstance(op, Conv):
                self._conv(src, op, packed[f"{name}.{op.name}"], out=dst)
            else:
                ops.pool3_f32(src, op.stride, op.pad, op.average, out=dst)
        return bufs["out"]

    def trunk(self, x: torch.Tensor) -> torch.Tensor:
        """the network input fp32 [N, 299, 299, 3] channels-last -> pool features fp32 [N, 2048]"""
        packed = self.packed()
        for op in STEM:
            x = self._conv(x, op, packed[op.name]) if isinstance(op, Conv) else ops.pool3_f32(x, op.stride, op.pad, op.average)
        for name in BLOCKS:
            x = self.run_block(name, x)
        return ops.mean_pixels_f32(x)

    @torch.no_grad()
    def features(self, frames, quantise: bool = True) -> torch.Tensor:
        """``frames``: a pair (samples [N, 3, H, W] in [0, 1], images [N, 3, H, W] in [-1, 1]) -> fp32 [2 N, 2048] on the device, the
        samples' features first; or one tensor of samples [N, 3, H, W] in [0, 1] -> fp32 [N, 2048].  Any H, W >= 1.  A frame's features
        do not depend on what else is in the batch."""
        dev = next(self.parameters()).device
        single = isinstance(frames, torch.Tensor)
        samples, images = (frames, frames) if single else frames
        if samples.dim() != 4 or samples.shape[1] != 3 or tuple(samples.shape) != tuple(images.shape) or samples.shape[0] < 1:
            raise ValueError(f"FID: samples {tuple(samples.shape)} and images {tuple(images.shape)} must both be [N >= 1, 3, H, W]")
        x = ops.fid_input(samples.to(dev, torch.float32).contiguous(), images.to(dev, torch.float32).contiguous(), quantise, SIZE)
        if single:
            x = x[:samples.shape[0]]                             # (the input stage is one cheap launch: the second half is dropped)
        return self.trunk(x)

    def forward(self, frames, quantise: bool = True) -> torch.Tensor:
        return self.features(frames, quantise)

    def stats(self) -> FIDStats:
        return FIDStats(self)
