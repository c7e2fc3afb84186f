"""Drop-in `networks` module for the rendering hot path (MI355X / HIP).

Exports the classes the reference's train.py and renderer bind by name
(/root/reference/train.py:36-37, networks.py:25-26): `Embedding`, `Renderer`,
`Renderer_linear`, `MVSNeRF`.  Constructors, attribute names and state-dict keys/shapes
match the reference (networks.py:29-353) so its checkpoints load with
`load_state_dict`; `forward` runs the hand-written gfx950 kernels through the C ABI
(include/zest_render.h).  There is no PyTorch implementation of the forward pass here:
without libzest_hip.so, or on CPU tensors, calls raise.

Precision (resolve_precision): the reference's `--precision 32` (opt.py:69, the default) runs the
MLP on exact-product fp32 MFMA per operator and, in the fused single-launch renderer, on
split-fp16 operand pairs (fp32-class results at the fp16 matrix rate); `--precision 16` selects
16-bit operands with fp32 accumulation - bf16 by default, fp16 with `args.zest_dtype16 = "f16"`.
ZEST_PRECISION = fp32 | f16x3 | bf16 | f16 overrides both.
"""
import os

import weakref

import torch
import torch.nn as nn

import zest_hip

__all__ = ["Embedding", "Renderer", "Renderer_linear", "MVSNeRF", "resolve_precision", "inference_precision", "train_gemm_choice", "deterministic_choice",
           "ActivatedBatchNorm", "ConvBnReLU", "ConvBnReLU3D", "FeatureNet", "CostRegNet", "MVSNet",
           "MVSNeRF_G", "DyMVSNeRF_G", "GRAFDiscriminator"]


_PREC_BY_NAME = {"bf16": zest_hip.PREC_BF16, "16": zest_hip.PREC_BF16,
                 "f16": zest_hip.PREC_F16, "fp16": zest_hip.PREC_F16, "half": zest_hip.PREC_F16,
                 "f16x3": zest_hip.PREC_F16X3, "fp16x3": zest_hip.PREC_F16X3, "x3": zest_hip.PREC_F16X3,
                 "fp32": zest_hip.PREC_F32, "f32": zest_hip.PREC_F32, "32": zest_hip.PREC_F32}


def resolve_precision(args=None):
    """-> zest_hip.PREC_* from ZEST_PRECISION, else args.precision (16 | 32) and, for 16,
    args.zest_dtype16 ("bf16" default | "f16")."""
    env = os.environ.get("ZEST_PRECISION", "").lower()
    if env:
        if env not in _PREC_BY_NAME:
            raise ValueError("ZEST_PRECISION=%r: expected one of %s" % (env, sorted(_PREC_BY_NAME)))
        return _PREC_BY_NAME[env]
    if args is not None and int(getattr(args, "precision", 32) or 32) == 16:
        name = str(getattr(args, "zest_dtype16", "bf16")).lower()
        if name not in ("bf16", "f16", "fp16"):
            raise ValueError("args.zest_dtype16=%r: expected 'bf16' or 'f16'" % (name,))
        return _PREC_BY_NAME[name]
    return zest_hip.PREC_F32


_warned_train_gemm16 = False


def train_gemm_choice(args=None, train16=False):
    """-> zest_hip.GEMM_*: the GEMMs of the fp32 training path, from args.zest_train_gemm, else the environment
    variable ZEST_TRAIN_GEMM, else "library" (rocBLAS sgemm); "split" selects the three-term bf16 MFMA kernels
    (fp32-class results, no library call).  --precision 16 trains on the bf16 kernels and has no such GEMMs: the
    choice is then ignored, with one warning per process."""
    global _warned_train_gemm16
    name = getattr(args, "zest_train_gemm", None) or os.environ.get("ZEST_TRAIN_GEMM") or "library"
    if name not in zest_hip.GEMM_NAMES:
        raise ValueError("zest: zest_train_gemm / ZEST_TRAIN_GEMM must be one of %s, got %r"
                         % (sorted(zest_hip.GEMM_NAMES), name))
    if train16 and name != "library":
        if not _warned_train_gemm16:
            import warnings
            warnings.warn("zest: zest_train_gemm=%r is ignored in --precision 16 (it chooses the GEMMs of the fp32 "
                          "training path)" % name, stacklevel=2)
            _warned_train_gemm16 = True
        return zest_hip.GEMM_LIBRARY
    return zest_hip.GEMM_NAMES[name]


def deterministic_choice(args=None):
    """-> bool: the opt-in switch for bit-reproducible gradients, from the environment variable ZEST_DETERMINISTIC
    ("1" or "0": it overrides the argument), else args.zest_deterministic, else off.  With it on, the four places of the
    training path that add floats with atomics - the gradient of the encoding volume (zest_encode_bwd), of the feature
    maps through the plane sweep (zest_volume_cost_bwd) and through utils.homo_warp, and the bias gradients of the fp32
    MLP path - take order-independent forms (csrc/det_grads.hip), so that no gradient the project's own kernels produce
    depends on the order in which workgroups arrive; off, every result keeps its bits and its speed.  rendering() reads
    it once per call, _Generator._volume hands it to the builder (MVSNet.zest_deterministic).
    Complete reproducibility of the fp32 rendering path needs zest_train_gemm = "split" as well: behind the default
    "library" the GEMMs are rocBLAS's, whose summation order the project does not control.  The library's convolution
    backward in the volume builder (layers 1-9 of the regularisation net, the feature pyramid) is outside the switch too.
    A non-finite gradient poisons the whole result of a scatter-add in this mode, where the default poisons the
    elements it touches."""
    env = os.environ.get("ZEST_DETERMINISTIC", "")
    if env:
        if env not in ("0", "1"):
            raise ValueError("zest: ZEST_DETERMINISTIC must be 0 or 1, got %r" % (env,))
        return env == "1"
    return bool(getattr(args, "zest_deterministic", False))


def inference_precision(prec, args=None):
    """Operand type of an inference (no-grad) MLP launch in mode `prec`: fp32 mode runs on split-fp16
    pairs (ZEST_PREC_F16X3: same 1e-4 / 1e-3 agreement with the fp32 reference as the exact-product
    kernel at ~7x its speed) unless exact fp32 products are asked for with `args.zest_fp32_exact`
    or ZEST_FP32_EXACT=1 (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain, no fp16 range limit)."""
    if prec != zest_hip.PREC_F32:
        return prec
    if os.environ.get("ZEST_FP32_EXACT", "") not in ("", "0") or getattr(args, "zest_fp32_exact", False):
        return zest_hip.PREC_F32
    return zest_hip.PREC_F16X3


class Embedding(nn.Module):
    """Positional encoder x -> (x, sin(2^k x), cos(2^k x))_k  (reference networks.py:29-65)."""

    def __init__(self, in_channels, N_freqs, logscale=True):
        super().__init__()
        if not logscale:
            raise NotImplementedError("zest Embedding: only log-scale bands (the reference default) "
                                      "are implemented in the HIP encoder")
        self.N_freqs = N_freqs
        self.in_channels = in_channels
        self.funcs = [torch.sin, torch.cos]
        self.out_channels = in_channels * (len(self.funcs) * N_freqs + 1)
        self.freq_bands = 2 ** torch.linspace(0, N_freqs - 1, N_freqs)

    def forward(self, x):
        if x.shape[-1] != self.in_channels:
            raise RuntimeError("Embedding expects %d channels, got %d" % (self.in_channels, x.shape[-1]))
        return zest_hip.embed(x, self.N_freqs)


class _MlpBase(nn.Module):
    """Parameters of the width-W MLP + the packed-weight cache for the MFMA kernels."""

    def _build(self, D, W, input_ch, input_ch_views, input_ch_feat, skips, use_viewdirs):
        # Reference networks.py:93-100 builds any D / W / skips.  The shipped shape (8 / 256 / [4]: every config
        # and opt.py:54-57's defaults) runs on the MFMA engine in every precision; other shapes run on the
        # exact-product fp32 kernel and the fp32 training path (engine_precision below).
        skips = [int(i) for i in skips]
        if not use_viewdirs:
            raise NotImplementedError("zest MLP: use_viewdirs=False (never built by the reference: networks.py:336-345 "
                                      "passes use_viewdirs=True)")
        if not 2 <= D <= 8 or W not in (64, 128, 192, 256) or any(i < 0 or i > D - 2 for i in skips):
            raise NotImplementedError(
                "zest MLP kernels cover 2 <= D <= 8, W in {64,128,192,256}, skips within 0 .. D-2 "
                "(got D=%s W=%s skips=%s)" % (D, W, skips))
        self.D, self.W, self.skips, self.use_viewdirs = D, W, skips, use_viewdirs
        self.default_shape = D == 8 and W == 256 and sorted(set(skips)) == [4]
        self.in_ch_pts, self.in_ch_views, self.in_ch_feat = input_ch, input_ch_views, input_ch_feat
        # Encoded point = 63 (xyz) or 84 (xyzt) channels; anything beyond 63 that is not 84 is the
        # Neural3D time code (reference train.py:112-113: input_ch += time_code_dim, static net).  The
        # code is one vector per rendering call, the same for every sample, so its columns of layers 0
        # and 5 fold into those layers' biases (effective_parameters) and the kernels see a 63-channel net.
        self.in_ch_pe = input_ch if input_ch in (63, 84) else 63
        self.in_ch_time = input_ch - self.in_ch_pe
        if self.in_ch_time < 0:
            raise NotImplementedError("zest MLP: input_ch=%d is smaller than the 63-channel point encoding" % input_ch)
        self.pts_linears = nn.ModuleList()
        for i in range(D - 1):
            if i == 0:
                self.pts_linears.append(nn.Linear(input_ch, W))
            self.pts_linears.append(nn.Linear(W + input_ch if i in skips else W, W))
        self.pts_bias = nn.Linear(input_ch_feat, W)
        self.views_linears = nn.ModuleList([nn.Linear(W + input_ch_views, W // 2)])
        self.feature_linear = nn.Linear(W, W)
        self.alpha_linear = nn.Linear(W, 1)
        self.rgb_linear = nn.Linear(W // 2, 3)
        self._packed = {}

    def _desc(self):
        raise NotImplementedError

    def _mk_desc(self, in_ch_pts, use_feat, net_type, head):
        if self.default_shape:          # zeros = the default shape: one plan / packed-weight cache entry
            return zest_hip.MlpDesc(in_ch_pts, self.in_ch_feat, self.in_ch_views, use_feat, net_type, head)
        return zest_hip.MlpDesc(in_ch_pts, self.in_ch_feat, self.in_ch_views, use_feat, net_type, head,
                                self.D, self.W, sum(1 << i for i in set(self.skips)))

    def engine_precision(self, prec):
        """Operand type this net can run `prec` in: the MFMA engine (bf16 / fp16 / split fp16) is
        written for the shipped shape; other depths / widths / skips run exact fp32 products."""
        return prec if self.default_shape else zest_hip.PREC_F32

    def _param_list(self):
        """The (name, Parameter) pairs of named_parameters(), cached with the tree they were read from: the parameter and
        child tables of this module and every module below it, and the objects they held.  Each use compares those
        objects by identity and the tables' sizes (a few dozen dictionary look-ups, no walk of the tree), so a parameter
        or a leaf replaced anywhere below - `net.alpha_linear.weight = ...`, `net.pts_linears[0] = ...`,
        `load_state_dict(assign=True)` - rebuilds the list, not only an assignment on this module itself."""
        ent = self.__dict__.get("_zest_params")
        if ent is not None:
            for d, k, obj in ent[1]:
                if d.get(k) is not obj:
                    break
            else:
                if [len(d) for d in ent[2]] == ent[3]:      # nothing was added either
                    return ent[0]
        tables = [d for m in self.modules() for d in (m._parameters, m._modules)]
        held = tuple((d, k, obj) for d in tables for k, obj in d.items())
        if self.__dict__.get("_packed"):
            self._packed.clear()        # packed from other objects: a new one may sit at a freed one's address and version
        ent = self.__dict__["_zest_params"] = (tuple(self.named_parameters()), held, tables, [len(d) for d in tables])
        return ent[0]

    def effective_parameters(self, time_codes=None):
        """{name: tensor} of the 63/84-channel net the kernels run.  Without time-code channels these
        are the parameters themselves.  With them (in_ch_time = T > 0) `time_codes` ([T] or [1,T], the
        frame's latent code BEFORE the sigmoid, reference renderer.py:269-273) is folded in:
            layer 0:  W0 [256, P+T]      -> W0[:, :P],               b0 + W0[:, P:] sigmoid(tc)
            layer 5:  W5 [256, P+T+256]  -> W5[:, :P] | W5[:, P+T:],  b5 + W5[:, P:P+T] sigmoid(tc)
        (layer i+1 for each i in skips; the skip layer's input is [point | time code | h], networks.py:182).  Plain torch ops: under
        autograd the gradients reach the original parameters and the code."""
        named = dict(self._param_list())
        T, P = self.in_ch_time, self.in_ch_pe
        if T == 0:
            if time_codes is not None:
                raise RuntimeError("zest MLP: time_codes given to a net without time-code channels (input_ch=%d)" % P)
            return named
        if time_codes is None:
            raise RuntimeError("zest MLP: this net has %d time-code input channels; pass time_codes to rendering()" % T)
        tc = torch.sigmoid(time_codes.float()).reshape(-1)
        if tc.numel() != T:
            raise RuntimeError("zest MLP: time code has %d values, the net expects %d" % (tc.numel(), T))
        w0 = named["pts_linears.0.weight"]
        named["pts_linears.0.weight"] = w0[:, :P].contiguous()
        named["pts_linears.0.bias"] = named["pts_linears.0.bias"] + w0[:, P:] @ tc
        for i in set(self.skips):
            k = "pts_linears.%d" % (i + 1)
            w = named[k + ".weight"]
            named[k + ".weight"] = torch.cat([w[:, :P], w[:, P + T:]], 1)
            named[k + ".bias"] = named[k + ".bias"] + w[:, P:P + T] @ tc
        return named

    def packed(self, precision, desc=None, time_codes=None):
        """Weights in MFMA stream order; re-packed when any parameter (or the time code) changes
        (storage or version counter: optimizer steps, load_state_dict and .to() all show up).  The
        (name, Parameter) list is cached - walking the module tree costs more host time than a
        1024-ray launch.  desc: a variant descriptor of the same parameters (forward_alpha), packed and
        cached apart."""
        params = self._param_list()
        stamp = tuple((p.data_ptr(), p._version) for _, p in params)
        key = precision if desc is None else (precision, desc.use_feat, desc.net_type, desc.head)
        hit = self._packed.get(key)
        # whether a code was folded in is part of what the entry is valid for: a call without one on an entry packed
        # with one takes the miss path, where effective_parameters raises for a net with time-code channels
        fresh = hit is not None and hit[0] == stamp and (hit[2] is None) == (time_codes is None)
        if fresh and time_codes is not None:
            # The frame's code is folded into the packed biases, so it is part of what the entry is valid for.
            # Its address and version counter do not identify it: the reference's callers build
            # `self.time_codes[keyframe_id].to(device)` anew for every batch (train.py:849, 1058) and the caching
            # allocator hands the block just freed to the next frame's code at version 0.  Same live tensor object
            # at the same version = unchanged; any other tensor is compared by value with the copy the entry
            # keeps (T floats: one small device compare per call for such callers).
            ref, ver, copy = hit[2]
            if not (ref() is time_codes and ver == time_codes._version):
                fresh = (copy.shape == time_codes.shape and copy.device == time_codes.device
                         and bool(torch.equal(copy, time_codes.detach())))
                if fresh:
                    hit = (hit[0], hit[1], (weakref.ref(time_codes), time_codes._version, copy))
                    self._packed[key] = hit
        if not fresh:
            desc = self._desc() if desc is None else desc
            with torch.no_grad():
                eff = self.effective_parameters(time_codes)
            state = {"nerf." + k: v.detach() for k, v in eff.items()}
            tc = None if time_codes is None else (weakref.ref(time_codes), time_codes._version,
                                                  time_codes.detach().clone())
            hit = (stamp, zest_hip.mlp_pack(desc, precision, zest_hip.param_table(state, desc)), tc)
            self._packed[key] = hit
        return hit[1]

    def _forward_alpha(self, x, net_type, relu):
        """Density-only pass of the reference (networks.py:134-147, 266-280): x = [points | features]
        (no direction columns), the trunk ALWAYS modulated by pts_bias(features).  Runs the MLP kernel
        with zero direction columns and the alpha head, and keeps the density column."""
        if self.in_ch_time:
            raise NotImplementedError("forward_alpha: not available for nets with time-code channels")
        if x.shape[-1] != self.in_ch_pts + self.in_ch_feat:
            raise RuntimeError("forward_alpha expects %d + %d input channels, got %d"
                               % (self.in_ch_pts, self.in_ch_feat, x.shape[-1]))
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("forward_alpha: inference only (the reference never calls it: "
                                      "renderer.py:295 sets alpha_only only when no direction is given)")
        desc = self._mk_desc(self.in_ch_pts, 1, net_type, zest_hip.HEAD_NONE)
        prec = self.engine_precision(inference_precision(resolve_precision()))
        xin = torch.cat([x, x.new_zeros(*x.shape[:-1], self.in_ch_views)], -1)
        alpha = zest_hip.mlp_fwd(desc, prec, self.packed(prec, desc), xin)[..., 3:4]
        return torch.relu(alpha) if relu else alpha

    def __setattr__(self, name, value):
        if isinstance(value, (nn.Parameter, nn.Module)):
            self.__dict__.pop("_zest_params", None)          # a replaced parameter / sub-module: rebuild the list
        super().__setattr__(name, value)

    def zest_forward(self, x, precision=None):
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("zest MLP: use MVSNeRF.forward (it owns the `nerf.` parameter names the "
                               "training path needs)")
        if self.in_ch_time:
            raise NotImplementedError("zest MLP: a net with time-code channels runs through rendering(..., time_codes=...), "
                                      "which folds the frame's code into the biases of layers 0 and 5")
        desc = self._desc()
        prec = self.engine_precision(inference_precision(resolve_precision()) if precision is None else precision)
        return zest_hip.mlp_fwd(desc, prec, self.packed(prec), x)

    def forward(self, x):
        return self.zest_forward(x)


class Renderer(_MlpBase):
    """'v0' net: trunk layers relu(Linear(h) * pts_bias(feats)) (reference networks.py:73-221)."""

    def __init__(self, D=8, W=256, input_ch=3, input_ch_views=3, output_ch=4, input_ch_feat=8,
                 skips=[4], use_viewdirs=False, sceneflow=False, static=True, use_mvs=False):
        super().__init__()
        self._build(D, W, input_ch, input_ch_views, input_ch_feat, skips, use_viewdirs)
        self.predict_sceneflow, self.static, self.use_mvs = sceneflow, static, use_mvs
        if sceneflow:
            if static:
                self.w_linear = nn.Linear(W, 1)
            else:
                self.sf_linear = nn.Linear(W, 6)
                self.prob_linear = nn.Linear(W, 2)

    def _desc(self):
        head = zest_hip.HEAD_NONE
        if self.predict_sceneflow:
            head = zest_hip.HEAD_BLEND if self.static else zest_hip.HEAD_DYNAMIC
        return self._mk_desc(self.in_ch_pe, int(bool(self.use_mvs)), 0, head)

    def forward_alpha(self, x):
        """relu(alpha_linear(trunk(x))) with multiplicative modulation (reference networks.py:134-147)."""
        return self._forward_alpha(x, 0, True)


class Renderer_linear(_MlpBase):
    """'v2' net: additive modulation, relu(alpha), sigmoid(rgb) (reference networks.py:223-319)."""

    def __init__(self, D=8, W=256, input_ch=3, input_ch_views=3, output_ch=4, input_ch_feat=8,
                 skips=[4], use_viewdirs=False):
        super().__init__()
        self._build(D, W, input_ch, input_ch_views, input_ch_feat, skips, use_viewdirs)

    def _desc(self):
        return self._mk_desc(self.in_ch_pe, 1, 2, zest_hip.HEAD_NONE)

    def forward_alpha(self, x):
        """alpha_linear(trunk(x)), additive modulation, no activation (reference networks.py:266-280)."""
        return self._forward_alpha(x, 3, False)


class MVSNeRF(nn.Module):
    """Selects the net type; same constructor and `nerf.*` state-dict keys as the reference
    (networks.py:321-353)."""

    def __init__(self, D=8, W=256, input_ch_pts=3, output_ch=4, input_ch_views=3, input_ch_feat=8,
                 skips=[4], net_type='v2', sceneflow=False, static=True, use_mvs=False):
        super().__init__()
        self.in_ch_pts, self.out_ch_pts = input_ch_pts, output_ch
        self.in_ch_views, self.in_ch_feat = input_ch_views, input_ch_feat
        self.net_type = net_type
        if net_type == 'v0':
            self.nerf = Renderer(D=D, W=W, input_ch_feat=input_ch_feat, input_ch=input_ch_pts,
                                 output_ch=output_ch, skips=skips, input_ch_views=input_ch_views,
                                 use_viewdirs=True, sceneflow=sceneflow, static=static, use_mvs=use_mvs)
        elif net_type == 'v2':
            self.nerf = Renderer_linear(D=D, W=W, input_ch_feat=input_ch_feat, input_ch=input_ch_pts,
                                        output_ch=output_ch, skips=skips,
                                        input_ch_views=input_ch_views, use_viewdirs=True)
        else:
            raise ValueError("net_type must be 'v0' or 'v2', got %r" % (net_type,))

    def desc(self):
        return self.nerf._desc()

    def packed(self, precision, time_codes=None):
        return self.nerf.packed(precision, time_codes=time_codes)

    def forward_alpha(self, x):
        return self.nerf.forward_alpha(x)

    def zest_forward(self, x, precision=None):
        return self.nerf.zest_forward(x, precision)

    def forward(self, x):
        if self.nerf.in_ch_time == 0 and torch.is_grad_enabled() and (
                x.requires_grad or any(p.requires_grad for p in self.parameters())):
            import zest_autograd
            return zest_autograd.mlp_apply(self, x, gemm=train_gemm_choice(),     # fp32 training path (HIP fwd + bwd)
                                           deterministic=deterministic_choice())
        return self.nerf(x)


# ------------------------------------------------------------------------------------------
# MVS volume builder (reference networks.py:935-1238).  The convolutional
# stacks are plain library convolutions (MIOpen through torch.nn: plumbing, not the product);
# the plane sweep between them - homo_warp + build_volume_cost, the part that streams
# hundreds of MB - is the HIP kernel zest_volume_cost_fwd.  The reference normalises with
# InPlaceABN (inplace_abn, a CUDA-only extension that is not installable here): its forward is
# batch norm followed by leaky ReLU(0.01), and its parameters are weight / bias / running_mean /
# running_var, so ActivatedBatchNorm keeps the reference's state-dict keys and checkpoints load.
# Parity: homo_warp (grid construction and sampling) and build_volume_cost are pinned at V = 3 by
# reference-generated fixtures (tests/golden/homo_warp.npz, volume_cost_*.npz: forward, masks and the
# gradient with respect to the features); other view counts, which the reference cannot run, are checked
# against the oracle.  The wiring of the convolutional stacks is pinned under the stated reading of the
# norm (builder_nets.npz); InPlaceABN's own arithmetic cannot be run here: "parity unpinned" (DESIGN.md 4b).
class ActivatedBatchNorm(nn.BatchNorm2d):
    """InPlaceABN substitute: BatchNorm (any spatial rank) + leaky ReLU(0.01)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, activation="leaky_relu",
                 activation_param=0.01):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine)
        if activation not in ("leaky_relu", "identity"):
            raise NotImplementedError("ActivatedBatchNorm: activation %r" % (activation,))
        self.activation, self.activation_param = activation, activation_param

    def _check_input_dim(self, input):
        if input.dim() < 3:
            raise ValueError("expected at least 3D input (got %dD)" % input.dim())

    def forward(self, x):
        y = super().forward(x)
        return torch.nn.functional.leaky_relu(y, self.activation_param) if self.activation == "leaky_relu" else y


def pack_conv_weights(w, passes):
    """Conv3d weight [cout,cin,KD,K,K] (or Conv2d [cout,cin,K,K]: KD = 1) -> MFMA A operands of csrc/costreg.hip,
    [dz][dy][chunk][16-row tile][hi, lo][lane] x 8 bf16: lane (m = l & 15, g = l >> 4) of chunk c holds output channel
    16 nt + m against octet o = 4 c + g of the x-window (pixel o // (cin/8), channels 8 (o % (cin/8)) ..+7), zero beyond
    the window / the channels (cin is padded to a multiple of 8)."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin, KD, K, _ = w.shape
    opt = (cin + 7) // 8
    cpr, nt, dev = (K * opt + 3) // 4, (cout + 15) // 16, w.device
    lane, e = torch.arange(64, device=dev), torch.arange(8, device=dev)
    o = 4 * torch.arange(cpr, device=dev).view(cpr, 1, 1, 1) + (lane >> 4).view(1, 1, 64, 1)
    px, ci = o // opt, 8 * (o % opt) + e.view(1, 1, 1, 8)
    co = 16 * torch.arange(nt, device=dev).view(1, nt, 1, 1) + (lane & 15).view(1, 1, 64, 1)
    valid = ((o < K * opt) & (ci < cin) & (co < cout)).expand(cpr, nt, 64, 8)
    full = (cpr, nt, 64, 8)
    vals = w.detach().float()[co.clamp(max=cout - 1).expand(full), ci.clamp(max=cin - 1).expand(full), :, :,
                              px.clamp(max=K - 1).expand(full)]                     # [cpr,nt,64,8,dz,dy]
    vals = (vals * valid[..., None, None]).permute(4, 5, 0, 1, 2, 3)
    hi = vals.to(torch.bfloat16)
    parts = [hi] if passes == 1 else [hi, (vals - hi.float()).to(torch.bfloat16)]
    return torch.stack(parts, 4).contiguous().view(torch.int16).view(-1)           # [KD,K,cpr,nt,parts,64,8]


def _cached_packs(module, passes, weights, build):
    """Packed weights of `module`, rebuilt when a weight tensor is replaced, modified in place or given other storage
    (`w.data = ...`, `.double().float()`: same object, same version counter, another address)."""
    key = (passes,) + tuple((w.data_ptr(), w._version, str(w.device)) for w in weights)
    cache = module.__dict__.get("_zest_packs")
    # the tensors themselves are compared through weak references (an id() or an address can be recycled)
    if cache is None or cache[0] != key or len(cache[2]) != len(weights) or any(r() is not w for r, w in zip(cache[2], weights)):
        module.__dict__["_zest_packs"] = cache = (key, build(), [weakref.ref(w) for w in weights])
    return cache[1]


def _hip_norm(bn):
    return isinstance(bn, ActivatedBatchNorm) and bn.activation == "leaky_relu" and abs(bn.activation_param - 0.01) < 1e-12


def _layer_slabs(chans, keep, device):
    """Per-layer views of three allocations for the layers of `chans` output channels: the batch-statistics tables
    [rows,2,C] float64 (zest_hip.costreg_stats), the norm constants [2,C] and - with keep, else None - the batch
    moments [2,C], both fp32 -> (st, pr, mo), a list each."""
    offs = [2 * sum(chans[:i]) for i in range(len(chans) + 1)]
    rows = zest_hip.costreg_stat_rows()
    stats_all = torch.empty(rows * offs[-1], device=device, dtype=torch.float64)
    pre_all = torch.empty(offs[-1], device=device, dtype=torch.float32)
    mom_all = torch.empty(offs[-1], device=device, dtype=torch.float32) if keep else None
    st = [stats_all[rows * offs[i]:rows * offs[i + 1]].view(rows, 2, c) for i, c in enumerate(chans)]
    pr = [pre_all[offs[i]:offs[i + 1]].view(2, c) for i, c in enumerate(chans)]
    mo = [mom_all[offs[i]:offs[i + 1]].view(2, c) if keep else None for i, c in enumerate(chans)]
    return st, pr, mo


class ConvBnReLU(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1,
                 norm_act=ActivatedBatchNorm):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = norm_act(out_channels)

    def forward(self, x):
        return self.bn(self.conv(x))


class ConvBnReLU3D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, pad=1,
                 norm_act=ActivatedBatchNorm):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, bias=False)
        self.bn = norm_act(out_channels)

    def forward(self, x):
        return self.bn(self.conv(x))


class FeatureNet(nn.Module):
    """Three-level feature pyramid; the top level (32 channels at 1/4 resolution) feeds the
    plane sweep (reference networks.py:962-1001)."""

    def __init__(self, norm_act=ActivatedBatchNorm):
        super().__init__()
        self.conv0 = nn.Sequential(ConvBnReLU(3, 8, 3, 1, 1, norm_act=norm_act),
                                   ConvBnReLU(8, 8, 3, 1, 1, norm_act=norm_act))
        self.conv1 = nn.Sequential(ConvBnReLU(8, 16, 5, 2, 2, norm_act=norm_act),
                                   ConvBnReLU(16, 16, 3, 1, 1, norm_act=norm_act),
                                   ConvBnReLU(16, 16, 3, 1, 1, norm_act=norm_act))
        self.conv2 = nn.Sequential(ConvBnReLU(16, 32, 5, 2, 2, norm_act=norm_act),
                                   ConvBnReLU(32, 32, 3, 1, 1, norm_act=norm_act),
                                   ConvBnReLU(32, 32, 3, 1, 1, norm_act=norm_act))
        self.toplayer = nn.Conv2d(32, 32, 1)

    # ---- HIP path, no autograd: the eight Conv + norm + activation layers as 2-D calls of the regularisation net's
    # convolution kernel (csrc/costreg.hip, one-slice-deep windows), the 1x1 top layer as one matrix product
    _HIP_LAYERS = (("conv0", 0), ("conv0", 1), ("conv1", 0), ("conv1", 1), ("conv1", 2), ("conv2", 0), ("conv2", 1), ("conv2", 2))
    _HIP_SHAPES = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1),
                   (32, 32, 3, 1))

    def hip_layers(self):
        """The eight Conv + norm + activation modules of the HIP path, in layer order."""
        return [getattr(self, s)[i] for s, i in self._HIP_LAYERS]

    def hip_supported(self):
        convs = self.hip_layers()
        shapes = tuple((m.conv.in_channels, m.conv.out_channels, m.conv.kernel_size[0], m.conv.stride[0]) for m in convs)
        top = self.toplayer
        return (shapes == self._HIP_SHAPES and all(_hip_norm(m.bn) for m in convs) and top.kernel_size == (1, 1)
                and top.in_channels == top.out_channels == 32)

    def forward_hip(self, imgs, passes=3, keep=False):
        """imgs [N,3,H,W] -> top-level features, channels-last [N,H/4,W/4,32] (what the plane sweep reads), no graph.
        keep: also the raw output, norm constants and batch moments of every layer (zest_autograd.FeatureFn)."""
        convs = self.hip_layers()
        packs = _cached_packs(self, passes, [m.conv.weight for m in convs],
                              lambda: [pack_conv_weights(m.conv.weight, passes) for m in convs])
        chans = [m.bn.num_features for m in convs]
        st, pr, mo = _layer_slabs(chans, keep, imgs.device)
        x = torch.nn.functional.pad(imgs.float().permute(0, 2, 3, 1), (0, 5)).contiguous()        # [N,H,W,8]
        pre, raw = None, []
        for i, m in enumerate(convs):
            x = zest_hip.conv2d_cl(x, pre, packs[i], chans[i], m.conv.kernel_size[0], m.conv.stride[0], passes, st[i])
            pre = zest_hip.costreg_bn(st[i], x.numel() // chans[i], m.bn, m.bn.training, pr[i], mo[i])
            raw.append(x)
        act = torch.nn.functional.leaky_relu(x * pre[0] + pre[1], 0.01)
        top = self.toplayer
        bias = top.bias if top.bias is not None else act.new_zeros(32)
        feats = torch.addmm(bias.to(act.dtype), act.view(-1, 32), top.weight.view(32, 32).t().to(act.dtype)).float().view(x.shape)
        return (feats, raw, pr, mo) if keep else feats

    def _upsample_add(self, x, y):
        return torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) + y

    def forward(self, x):
        """-> (top-level features, the output of every stage).  Only the first element is on the path; the
        list keeps the reference's call shape (its vis_test dumps read it, networks.py:1162-1181)."""
        stages = []
        for stage in (self.conv0, self.conv1, self.conv2, self.toplayer):
            x = stage(x)
            stages.append(x)
        return x, stages


class CostRegNet(nn.Module):
    """3-D U-Net: cost volume -> 8-channel neural encoding volume (reference networks.py:1003-1059)."""

    def __init__(self, in_channels, norm_act=ActivatedBatchNorm):
        super().__init__()
        self.conv0 = ConvBnReLU3D(in_channels, 8, norm_act=norm_act)
        self.conv1 = ConvBnReLU3D(8, 16, stride=2, norm_act=norm_act)
        self.conv2 = ConvBnReLU3D(16, 16, norm_act=norm_act)
        self.conv3 = ConvBnReLU3D(16, 32, stride=2, norm_act=norm_act)
        self.conv4 = ConvBnReLU3D(32, 32, norm_act=norm_act)
        self.conv5 = ConvBnReLU3D(32, 64, stride=2, norm_act=norm_act)
        self.conv6 = ConvBnReLU3D(64, 64, norm_act=norm_act)
        up = lambda i, o: nn.Sequential(
            nn.ConvTranspose3d(i, o, 3, padding=1, output_padding=1, stride=2, bias=False), norm_act(o))
        self.conv7, self.conv9, self.conv11 = up(64, 32), up(32, 16), up(16, 8)

    # ---- HIP path, no autograd (csrc/costreg.hip): channels-last tensors, a layer's norm + activation applied by
    # the layer that reads it, batch statistics from the convolution kernels themselves
    _HIP_CONVS = (("conv0", 1), ("conv1", 2), ("conv2", 1), ("conv3", 2), ("conv4", 1), ("conv5", 2), ("conv6", 1))
    _HIP_UPS = ("conv7", "conv9", "conv11")

    def hip_layers(self):
        """-> (convolutions, norms) of the HIP path: the seven of the way down, then the three transposed ones, in the
        order of forward_hip's `raw`."""
        down, ups = [getattr(self, n) for n, _ in self._HIP_CONVS], [getattr(self, n) for n in self._HIP_UPS]
        return [m.conv for m in down] + [m[0] for m in ups], [m.bn for m in down] + [m[1] for m in ups]

    def hip_supported(self):
        """The HIP kernels cover the reference's layer shapes with leaky-ReLU(0.01) norms."""
        bns = self.hip_layers()[1]
        return (self.conv0.conv.in_channels <= zest_hip.COST_CL_CHANNELS and self.conv0.conv.out_channels == 8
                and all(_hip_norm(b) for b in bns))

    @staticmethod
    def _pack_conv(w, passes):
        return pack_conv_weights(w, passes)

    @staticmethod
    def _pack_deconv(w, passes):
        """ConvTranspose3d weight [cin,cout,3,3,3] -> MFMA A operands [class][oz][oy][chunk][16-row tile][hi, lo][lane]
        x 8 bf16.  Class (pz, py, px) = parity of the output voxel; (oz, oy) = offset of the input row; per dimension
        an even output takes tap k = 1 of input i, an odd one k = 2 of input i and k = 0 of input i + 1.  Lane
        (m, g) of chunk c: output channel 16 nt + m against octet o = 4 c + g of the window of 1 + px pixels."""
        cin, cout = w.shape[:2]
        opt, nt, dev = cin // 8, (cout + 15) // 16, w.device
        ch2 = (2 * opt + 3) // 4
        lane, e = torch.arange(64, device=dev), torch.arange(8, device=dev)
        o = 4 * torch.arange(ch2, device=dev).view(ch2, 1, 1, 1) + (lane >> 4).view(1, 1, 64, 1)
        p, ci = o // opt, 8 * (o % opt) + e.view(1, 1, 1, 8)
        co = 16 * torch.arange(nt, device=dev).view(1, nt, 1, 1) + (lane & 15).view(1, 1, 64, 1)
        full = (ch2, nt, 64, 8)
        wf = w.detach().float()
        out = torch.zeros((8, 2, 2) + full, device=dev)
        tap = lambda par, off: (2 if off == 0 else 0) if par else 1
        for cls in range(8):
            pz, py, px = cls >> 2, (cls >> 1) & 1, cls & 1
            for oz in range(1 + pz):
                for oy in range(1 + py):
                    kx = torch.where(p == 0, tap(px, 0), tap(px, 1)).expand(full)
                    valid = ((p <= px) & (co < cout)).expand(full)
                    vals = wf[ci.expand(full), co.clamp(max=cout - 1).expand(full), tap(pz, oz), tap(py, oy), kx]
                    out[cls, oz, oy] = vals * valid
        hi = out.to(torch.bfloat16)
        parts = [hi] if passes == 1 else [hi, (out - hi.float()).to(torch.bfloat16)]
        return torch.stack(parts, 5).contiguous().view(torch.int16).view(-1)       # [8,2,2,ch2,nt,parts,64,8]

    def forward_hip(self, cost_cl, passes=3, keep=False):
        """cost_cl [D,H,W,48] channels-last (zest_hip.volume_cost_cl) -> encoding volume [1,8,D,H,W], no graph.
        passes 3: split-bf16 operands (16 significant bits); 1: bf16 operands (the --precision 16 path).  Norms in
        training mode use (and record) batch statistics, as the library path does.
        keep: also return what a backward pass needs (zest_autograd.CostRegFn): the raw output of every layer, its norm
        constants [2,C] and its batch moments [2,C] (mean, 1/std)."""
        D, H, W, _ = cost_cl.shape
        if D % 8 or H % 8 or W % 8:
            raise RuntimeError("CostRegNet.forward_hip: volume %dx%dx%d is not a multiple of 8 per axis" % (D, H, W))
        convs, bns = self.hip_layers()
        pack = lambda c: (self._pack_deconv if c.transposed else pack_conv_weights)(c.weight, passes)
        packs = _cached_packs(self, passes, [c.weight for c in convs], lambda: [pack(c) for c in convs])
        chans = [b.num_features for b in bns]
        st, pr, mo = _layer_slabs(chans, keep, cost_cl.device)
        norm = lambda i, t: zest_hip.costreg_bn(st[i], t.numel() // chans[i], bns[i], bns[i].training, pr[i], mo[i])
        raw, x, pre = [], cost_cl, None
        for i, (_, stride) in enumerate(self._HIP_CONVS):
            x = zest_hip.costreg_conv(x, pre, packs[i], chans[i], stride, passes, st[i])
            pre = norm(i, x)
            raw.append(x)
        up = zest_hip.costreg_deconv(raw[6], pr[6], None, None, packs[7], chans[7], passes, st[7])
        norm(7, up)
        raw.append(up)
        up = zest_hip.costreg_deconv(raw[4], pr[4], up, pr[7], packs[8], chans[8], passes, st[8])
        norm(8, up)
        raw.append(up)
        up = zest_hip.costreg_deconv(raw[2], pr[2], up, pr[8], packs[9], chans[9], passes, st[9])
        norm(9, up)
        raw.append(up)
        vol = zest_hip.costreg_out(raw[0], pr[0], up, pr[9])
        return (vol, raw, pr, mo) if keep else vol

    def forward(self, x):
        """-> (encoding volume, the output of every level: three on the way down, the bottom, three on the way up).
        Only the first element is on the path (the list: reference call shape, networks.py:1213-1230)."""
        skips = []
        for level in ((self.conv0,), (self.conv1, self.conv2), (self.conv3, self.conv4)):
            for conv in level:
                x = conv(x)
            skips.append(x)
        x = self.conv6(self.conv5(x))
        levels = skips + [x]
        for up, skip in zip((self.conv7, self.conv9, self.conv11), reversed(skips)):
            x = skip + up(x)
            levels.append(x)
        return x, levels


class MVSNet(nn.Module):
    """Encoding-volume builder: 2-D features -> plane-sweep variance cost volume (HIP) -> 3-D
    regularisation.  Constructor, attribute names and state-dict keys follow the reference
    (networks.py:1061-1238)."""

    # The switches of the training path, name -> default; each is a class attribute too (below the class), so forward
    # reads plain attributes.  _Generator._volume sets them from the arguments of the same names (absent or None: left
    # alone).  All but the first are opt-in; the three zest_hip_*grad* hold under bf16 autocast (--precision 16) only.
    ZEST_SWITCHES = {
        # both nets' training forward on the HIP kernels (FeatureFn, CostRegFn); None: decided per call - under bf16 autocast
        "zest_hip_costreg_train": None,
        # cost_reg_2.conv0's weight gradient in HIP (CostRegFn keeps a [D,H,W,48] fp32 cost volume: 0.5 GB at 128 x 120 x 176)
        "zest_hip_costreg_wgrad": False,
        # cost_reg_2.conv0's data gradient - towards the cost volume - in HIP, fp32 channel planes (nothing extra is kept)
        "zest_hip_costreg_dgrad": False,
        # the feature pyramid's convolution gradients - weight, data, 1 x 1 top layer - in HIP (csrc/feature_grad.hip, FeatureFn)
        "zest_hip_feature_grads": False,
        # (also ZEST_DETERMINISTIC=1, see deterministic_choice) the order-independent plane-sweep backward, no float atomics
        "zest_deterministic": False,
    }
    # no argument sets this one: False keeps the whole-image evaluation (hip_path) on the library modules
    zest_hip_costreg = True

    def __init__(self, num_groups=1, norm_act=ActivatedBatchNorm, levels=1):
        super().__init__()
        self.levels = levels
        self.n_depths = [128, 32, 8]
        self.G = num_groups
        self.feature = FeatureNet()
        self.chunk = 1024
        self.cost_reg_2 = CostRegNet(32 + 9, norm_act)

    def build_volume_cost(self, imgs, feats, proj_mats, depth_values, pad=0):
        """imgs [1,V,3,Hi,Wi]; feats [1,V,32,H,W]; proj_mats [1,V,3,4]; depth_values [1,D]
        -> (img_feat [1,3V+32,D,H+2pad,W+2pad], in_masks [1,V,D,H+2pad,W+2pad]).  One HIP launch
        (zest_volume_cost_fwd); under autograd the gradient reaches `feats` through
        zest_volume_cost_bwd (images, projections and depths are data)."""
        B, V, C, H, W = feats.shape
        if B != 1:
            raise RuntimeError("build_volume_cost: batch must be 1 (the reference assumes it too)")
        imgs_lr = torch.nn.functional.interpolate(imgs.reshape(B * V, *imgs.shape[2:]), (H, W), mode="bilinear",
                                                  align_corners=False)
        depth = depth_values.reshape(depth_values.shape[0], -1)[0]
        if torch.is_grad_enabled() and feats.requires_grad:
            import zest_autograd
            img_feat, masks = zest_autograd.VolumeCostFn.apply(feats[0].float(), imgs_lr.detach(), proj_mats[0, 1:].detach(),
                                                               depth.detach(), pad, bool(self.zest_deterministic))
        else:
            img_feat, masks = zest_hip.volume_cost(feats[0], imgs_lr, proj_mats[0, 1:], depth, pad)
        return img_feat[None], masks[None]

    def hip_path(self, imgs, pad=0):
        """True when forward(imgs, ..., pad) runs on the HIP kernels alone: no autograd, the reference's layer shapes,
        a volume of whole octets per axis."""
        B, V, _, H, W = imgs.shape
        half = lambda n: (n - 1) // 2 + 1
        Hf, Wf = half(half(H)), half(half(W))
        return (not torch.is_grad_enabled() and imgs.is_cuda and B == 1 and 3 * V + 32 <= zest_hip.COST_CL_CHANNELS
                and not ((Hf + 2 * pad) % 8 or (Wf + 2 * pad) % 8) and self.zest_hip_costreg
                and self.cost_reg_2.hip_supported())

    def forward(self, imgs, proj_mats, near_far, pad=0, return_color=False, lindisp=False,
                vis_test=False, test_dir=None):
        """-> (volume_feat [1,8,128,H/4+2pad,W/4+2pad], feats, depth_values) (reference networks.py:1142-1238).
        Differentiable with respect to the parameters of FeatureNet and CostRegNet."""
        if vis_test:
            raise NotImplementedError("MVSNet.forward: vis_test dumps are a debugging aid of the reference")
        B, V, _, H, W = imgs.shape
        D = 128
        half = lambda n: (n - 1) // 2 + 1
        Hf, Wf = half(half(H)), half(half(W))
        # whole-image evaluation (no autograd): feature pyramid, plane sweep and regularisation net as HIP kernels
        # (csrc/costreg.hip); bf16 operands under autocast (--precision 16), split-bf16 pairs otherwise
        hip = not return_color and self.hip_path(imgs, pad)
        passes = 1 if torch.is_autocast_enabled() else 3
        feats_cl = None
        hip_train = torch.is_autocast_enabled() if self.zest_hip_costreg_train is None else bool(self.zest_hip_costreg_train)
        hip_train = hip_train and torch.is_grad_enabled() and imgs.is_cuda
        if hip and self.feature.hip_supported():
            feats_cl = self.feature.forward_hip(imgs[0], passes)
            feats = feats_cl.permute(0, 3, 1, 2)[None]
        elif (hip_train and B == 1 and self.feature.hip_supported() and self.feature.toplayer.bias is not None
              and all(m.training for m in self.feature.modules() if isinstance(m, ActivatedBatchNorm))):
            import zest_autograd                      # the pyramid's forward on the HIP kernels under autograd (FeatureFn)
            # zest_hip_feature_grads (opt-in, --precision 16 only): the convolutions' gradients in HIP as well
            feats = zest_autograd.feature_apply(self.feature, imgs[0], passes, hip_grads=bool(self.zest_hip_feature_grads))[None]
        else:
            feats, _ = self.feature(imgs.reshape(B * V, 3, H, W))
            feats = feats.view(B, V, *feats.shape[1:])
        t_vals = torch.linspace(0., 1., steps=D, device=imgs.device, dtype=imgs.dtype)
        near, far = near_far
        if not lindisp:
            depth_values = near * (1. - t_vals) + far * t_vals
        else:
            depth_values = 1. / (1. / near * (1. - t_vals) + 1. / far * t_vals)
        depth_values = depth_values.unsqueeze(0)
        if hip:
            imgs_lr = torch.nn.functional.interpolate(imgs.reshape(B * V, *imgs.shape[2:]), (Hf, Wf), mode="bilinear",
                                                      align_corners=False)
            cost_cl = zest_hip.volume_cost_cl(None if feats_cl is not None else feats[0].float(), imgs_lr.float(),
                                              proj_mats[0, 1:], depth_values[0], pad, feats_cl=feats_cl)
            return self.cost_reg_2.forward_hip(cost_cl, passes=passes), feats, depth_values
        cost_vol, in_masks = self.build_volume_cost(imgs, feats, proj_mats, depth_values, pad=pad)
        Dp_ = cost_vol.shape[2]
        if return_color:
            feats = torch.cat((cost_vol[:, :V * 3].view(B, V, 3, *cost_vol.shape[2:]), in_masks.unsqueeze(2)), dim=2)
        # under autograd: the regularisation net's FORWARD on the HIP kernels (zest_autograd.CostRegFn) - by default in
        # bf16 autocast (--precision 16: a whole-generator step 47 -> 31 ms); in fp32 mode the library's fp32 backward
        # dominates either way and the library modules are kept unless zest_hip_costreg_train is set
        if (hip_train and B == 1
                and not (Dp_ % 8 or cost_vol.shape[-2] % 8 or cost_vol.shape[-1] % 8) and self.cost_reg_2.hip_supported()
                and all(m.training for m in self.cost_reg_2.modules() if isinstance(m, ActivatedBatchNorm))):
            # backward: HIP norm kernels + the library's convolution backward on the kept raw outputs
            import zest_autograd
            # zest_hip_costreg_wgrad (opt-in, --precision 16 only): the first layer's weight gradient in HIP as well;
            # zest_hip_costreg_dgrad (likewise): its data gradient
            volume_feat = zest_autograd.costreg_apply(self.cost_reg_2, cost_vol, passes, hip_wgrad=bool(self.zest_hip_costreg_wgrad),
                                                      hip_dgrad=bool(self.zest_hip_costreg_dgrad))
        else:
            volume_feat, _ = self.cost_reg_2(cost_vol)
        volume_feat = volume_feat.reshape(1, -1, *volume_feat.shape[2:])
        return volume_feat, feats, depth_values


for _name, _default in MVSNet.ZEST_SWITCHES.items():
    setattr(MVSNet, _name, _default)


# ------------------------------------------------------------------------------------------
# Generators: the callers of the path (reference networks.py:355-720).  Host orchestration only:
# encoding volume(s) -> ray sampling -> rendering, with the reference's constructor arguments,
# batch-dict keys and result keys.  The whole-image loop of forward_val additionally shards its
# ray chunks over the ranks of an initialised torch.distributed group (each rank
# renders its own chunks, ONE all-gather per image) and takes the fused single-launch renderer.
_IMAGENET = ((-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225), (1 / 0.229, 1 / 0.224, 1 / 0.225))


class _Generator(nn.Module):
    def unpreprocess(self, data, shape=(1, 1, 3, 1, 1)):
        """Undo the ImageNet normalisation of the loader (N V C H W)."""
        mean = torch.tensor(_IMAGENET[0], device=data.device).view(*shape)
        std = torch.tensor(_IMAGENET[1], device=data.device).view(*shape)
        return (data - mean) / std

    def _volume(self, net, imgs, proj_mats, near_far, bn_batch_stats=False):
        """Encoding volume of `net` (None -> no volume).  With autograd recording and a builder whose
        parameters want gradients (the reference optimises generator.parameters() including the MVSNets,
        train.py:270) the builder runs under autograd: library convolutions around the HIP plane sweep,
        whose backward is zest_volume_cost_bwd; otherwise without a graph."""
        if net is None:
            return None
        if bn_batch_stats:
            net.train()         # the reference validates with batch statistics (networks.py:629, 644)
        # --precision 16 (the reference runs the whole model under AMP then): library convolutions
        # in bf16; the plane sweep and the batch norms stay fp32
        amp = int(getattr(self.args, "precision", 32) or 32) == 16 and imgs.is_cuda
        train = torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())
        with torch.set_grad_enabled(train), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            if (not train and getattr(self.args, "zest_graph_builders", True) and isinstance(net, MVSNet)
                    and net.feature.hip_supported() and net.hip_path(imgs, self.args.pad)):
                return self._volume_replayed(net, imgs, proj_mats, near_far)
            if train and isinstance(net, MVSNet):
                for name in MVSNet.ZEST_SWITCHES:
                    if getattr(self.args, name, None) is not None:
                        setattr(net, name, bool(getattr(self.args, name)))  # the caller's choice, else the builder's own
                if os.environ.get("ZEST_DETERMINISTIC", ""):
                    net.zest_deterministic = deterministic_choice(self.args)    # the environment overrides the argument
            return net(imgs, proj_mats, near_far, pad=self.args.pad)[0].float()

    def _volume_replayed(self, net, imgs, proj_mats, near_far):
        """The all-HIP builder is ~110 kernel launches of a few microseconds each and the host is slower at issuing
        them than the device at running them (3.4 ms of wall time for 1.8 ms of device time per image): the first
        call with a given net, shapes and weights runs it directly and then RECORDS it as a HIP graph (recording
        executes nothing: the norms' running estimates advance once per call, as without the graph); later calls
        copy their inputs into the graph's buffers and replay it.  The volume is returned as a copy."""
        # The recorded kernels hold ADDRESSES: of every weight, gamma and beta, and of the norms' running estimates and
        # step counters (read in eval mode, written with batch statistics).  So the entry is valid for these tensor
        # objects (weak references) at these addresses; for the parameters also at these version counters, since their
        # packed copies are part of the recording.  The buffers' counters are left out: a replay reads and writes the
        # buffers themselves, and does not move a counter.
        weights = list(net.parameters())
        params = weights + list(net.buffers())
        norms = tuple((m.training, m.eps, m.momentum) for m in net.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm))
        key = (tuple(imgs.shape), tuple(proj_mats.shape), imgs.dtype, self.args.pad, torch.is_autocast_enabled(), norms,
               str(imgs.device), net.zest_hip_costreg, tuple(p._version for p in weights),
               tuple(p.data_ptr() for p in params))
        graphs = self.__dict__.setdefault("_zest_builder_graphs", {})
        for k in [k for k, e in graphs.items() if e["net"]() is None]:
            del graphs[k]                                   # a builder that no longer exists: free its graph and buffers
        ent = graphs.get(id(net))
        if (ent is not None and ent["net"]() is net and ent["key"] == key and len(ent["params"]) == len(params)
                and all(r() is p for r, p in zip(ent["params"], params))):
            ent["imgs"].copy_(imgs), ent["proj"].copy_(proj_mats), ent["near_far"].copy_(near_far)
            ent["graph"].replay()
            return ent["out"].clone()
        out = net(imgs, proj_mats, near_far, pad=self.args.pad)[0].float()
        graphs.pop(id(net), None)
        ent = dict(key=key, net=weakref.ref(net), params=[weakref.ref(p) for p in params], imgs=imgs.clone(), proj=proj_mats.clone(),
                   near_far=near_far.clone().to(imgs.device), graph=torch.cuda.CUDAGraph())
        cur = torch.cuda.current_stream(imgs.device)
        with torch.cuda.graph(ent["graph"]):
            ent["out"] = net(ent["imgs"], ent["proj"], ent["near_far"], pad=self.args.pad)[0].float()
        torch.cuda.current_stream(imgs.device).wait_stream(cur)
        # the recording reads the packed operands that _cached_packs held while it was made; a direct forward_hip with
        # another `passes` replaces them in the modules, so the entry keeps them alive for as long as it can be replayed
        ent["packs"] = [m.__dict__.get("_zest_packs") for m in (net.feature, net.cost_reg_2)]
        graphs[id(net)] = ent
        return out


class MVSNeRF_G(_Generator):
    """Static generator (reference networks.py:355-446)."""

    def __init__(self, args, nerf, encoding, embedding_pts, embedding_dir):
        super().__init__()
        self.nerf, self.encoding_net = nerf, encoding
        self.embedding_pts, self.embedding_dir = embedding_pts, embedding_dir
        self.N_rays, self.N_samples, self.args = args.batch_size, args.N_samples, args

    def forward(self, x, step=0, time_codes=None):
        import zest_utils as utils
        from zest_renderer import rendering
        imgs = x['images']
        depths = x['depths_h'] if 'depths_h' in x else x['depths']
        cams = {'w2cs': x['w2cs'], 'intrinsics': x['intrinsics']}
        volume = self._volume(self.encoding_net, imgs[:, :-1], x['proj_mats'][:, :-1], x['near_fars'][0, 0])
        pad = self.args.pad if self.encoding_net is not None else 0
        imgs = self.unpreprocess(imgs)
        rays_pts, rays_dir, target_s, rays_ndc, depth_candidates, rays_depth_gt, t_vals = utils.build_rays(
            imgs, depths, x['w2cs'], x['c2ws'], x['intrinsics'], x['near_fars'], self.N_samples,
            N_rays=self.N_rays, pad=pad, patch_size=self.args.patch_size, scale_anneal=self.args.scale_anneal,
            step=step, variable_patches=(self.args.gan_type == 'graf'))
        ret = rendering(self.args, rays_pts, rays_ndc, depth_candidates, rays_dir, volume_feature_static=volume,
                        imgs=imgs[:, :-1], img_feat=None, im_cam_mat=cams, network_fn=self.nerf,
                        embedding_pts=self.embedding_pts, embedding_dir=self.embedding_dir,
                        time_codes=time_codes, white_bkgd=self.args.white_bkgd)
        ret.update(target_s=target_s, depth_gt=rays_depth_gt, t_vals=t_vals)
        return ret


class DyMVSNeRF_G(_Generator):
    """Static + dynamic (scene-flow) generator (reference networks.py:448-720)."""

    VAL_KEYS = ('rgb_map_ref', 'depth_map_ref', 'rgb_map', 'depth_map', 'rgb_map_ref_dy', 'depth_map_ref_dy',
                'weights_map_dd')

    def __init__(self, args, decay_iteration, nerf_dynamic, nerf_static, encoding, encoding_dy, embedding_pts,
                 embedding_xyzt, embedding_dir):
        super().__init__()
        self.nerf_dynamic, self.nerf_static = nerf_dynamic, nerf_static
        self.encoding_net, self.encoding_net_dy = encoding, encoding_dy
        self.embedding_pts, self.embedding_xyzt, self.embedding_dir = embedding_pts, embedding_xyzt, embedding_dir
        self.N_rays, self.N_samples = args.batch_size, args.N_samples
        self.chain_bwd, self.decay_iteration, self.args = False, decay_iteration, args

    def _scene(self, x, bn_batch_stats=False):
        """Volumes, unnormalised images and cameras of one batch dict."""
        sc = dict(cams={'w2cs': x['w2cs'], 'intrinsics': x['intrinsics']}, nb_frames=None, nb_cams=None)
        imgs, near_far = x['images'], x['near_fars'][0, 0]
        # The two volume builders are independent (different images, different nets).  Without a graph (whole-image
        # evaluation) the dynamic one runs on a second HIP stream beside the static one: the small convolutions of the
        # feature pyramids and the tails of the large ones leave CUs idle that the other builder can use.
        side = None
        if (self.encoding_net_dy is not None and self.encoding_net is not None and imgs.is_cuda
                and not torch.is_grad_enabled() and getattr(self.args, 'zest_overlap_builders', True)):
            side = self.__dict__.get('_zest_side_stream')
            if side is None or side.device != imgs.device:
                side = self.__dict__['_zest_side_stream'] = torch.cuda.Stream(device=imgs.device)
        sc['vol_d'] = None
        if side is not None:
            cur = torch.cuda.current_stream(imgs.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                sc['vol_d'] = self._volume(self.encoding_net_dy, x['nb_imgs'], x['nb_proj_mats'], near_far, bn_batch_stats)
        sc['vol_s'] = self._volume(self.encoding_net, imgs[:, :-1], x['proj_mats'][:, :-1], near_far, bn_batch_stats)
        if self.encoding_net_dy is not None:
            sc['nb_cams'] = {'w2cs': x['nb_w2cs'], 'intrinsics': x['nb_intr']}
            if side is not None:
                torch.cuda.current_stream(imgs.device).wait_stream(side)
                sc['vol_d'].record_stream(torch.cuda.current_stream(imgs.device))
            else:
                sc['vol_d'] = self._volume(self.encoding_net_dy, x['nb_imgs'], x['nb_proj_mats'], near_far, bn_batch_stats)
            sc['nb_frames'] = self.unpreprocess(x['nb_imgs'])
        sc['pad'] = self.args.pad if (self.encoding_net is not None or self.encoding_net_dy is not None) else 0
        sc['imgs'] = self.unpreprocess(imgs)
        frame_t, sc['num_frames'] = x['time'].item(), x['total_frames'].item()
        sc['ref_frame_idx'] = frame_t / sc['num_frames'] * 2. - 1.0
        return sc

    def _render(self, sc, rays, time_codes, **kw):
        from zest_renderer import rendering
        rays_pts, rays_dir, rays_ndc, depth_candidates = rays
        return rendering(self.args, rays_pts, rays_ndc, depth_candidates, rays_dir,
                         volume_feature_static=sc['vol_s'], volume_feature_dynamic=sc['vol_d'],
                         imgs=sc['imgs'][:, :-1], neighbour_frames=sc['nb_frames'], im_cam_mat=sc['cams'],
                         nb_cam_mat=sc['nb_cams'], network_fn=self.nerf_static, network_fn_dy=self.nerf_dynamic,
                         embedding_pts=self.embedding_pts, embedding_xyzt=self.embedding_xyzt,
                         embedding_dir=self.embedding_dir, time_codes=time_codes, white_bkgd=self.args.white_bkgd,
                         scene_flow=True, chain_bwd=self.chain_bwd, ref_frame_idx=sc['ref_frame_idx'],
                         num_frames=sc['num_frames'], **kw)

    def forward(self, x, step=0, time_codes=None):
        import zest_utils as utils
        a = self.args
        chain_5frames = bool(a.with_chain_loss and step > self.decay_iteration * 1000 * 2)
        extra = a.num_extra_samples if (a.use_motion_mask and step < self.decay_iteration * 1000) else 0
        sc = self._scene(x)
        (rays_pts, rays_dir, target_s, rays_ndc, depth_candidates, rays_depth_gt, t_vals, flow_fwd, flow_bwd,
         mask_fwd, mask_bwd) = utils.build_rays_dy(
            sc['imgs'], x['depths'], x['w2cs'], x['c2ws'], x['intrinsics'], x['near_fars'], self.N_samples,
            N_rays=self.N_rays, pad=sc['pad'], patch_size=a.patch_size, scale_anneal=a.scale_anneal,
            num_extra_samples=extra, motion_coords=x['motion_coords'][-1], step=step,
            variable_patches=(a.gan_type == 'graf'), scene_flow=True, flow_fwd=x['flow_fwds'],
            flow_bwd=x['flow_bwds'], mask_fwd=x['mask_fwds'], mask_bwd=x['mask_bwds'])
        self.chain_bwd = not self.chain_bwd          # alternate the direction of the scene-flow chain
        ret = self._render(sc, (rays_pts, rays_dir, rays_ndc, depth_candidates), time_codes,
                           chain_5frames=chain_5frames, raw_noise_std=a.raw_noise_std)
        ret.update(target_s=target_s, depth_gt=rays_depth_gt, t_vals=t_vals, rays_flow_fwd_gt=flow_fwd,
                   rays_flow_bwd_gt=flow_bwd, rays_mask_fwd_gt=mask_fwd, rays_mask_bwd_gt=mask_bwd,
                   chain_bwd=self.chain_bwd, chain_5frames=chain_5frames)
        return ret

    def forward_val(self, x, time_codes=None):
        """Whole-image evaluation in chunks of args.chunk rays -> (imgs, rgbs_blend, depths_blend,
        rgbs_rig, depths_rig, rgbs_dy, depths_dy, weights_dd), each a list the caller concatenates
        (reference networks.py:595-720).  In a torch.distributed group the chunks are split into
        contiguous runs per rank, rendered locally and exchanged with ONE all-gather per image;
        every list then holds a single tensor covering the image."""
        import zest_utils as utils
        import zest_parallel
        a = self.args
        with torch.no_grad():
            sc = self._scene(x, bn_batch_stats=True)
            a.img_downscale = torch.rand((1,)) * 0.75 + 0.25     # as the reference; unused by the lookup
            N, V, C, H, W = sc['imgs'].shape
            n_chunks = (H * W + a.chunk - 1) // a.chunk
            world, rank = zest_parallel._world()
            lo, hi, per = zest_parallel.shard_bounds(n_chunks, world, rank)
            maps_only, a.zest_maps_only = getattr(a, 'zest_maps_only', False), True
            outs = {k: [] for k in self.VAL_KEYS}
            # args.chunk bounds the reference's per-sample tensors; the fused renderer keeps nothing per sample in
            # HBM, so neighbouring chunks go through ONE ray-sampling + ONE rendering launch (up to `group` chunks =
            # args.zest_val_rays rays, default one NSFF image: 288 x 512 x 128 samples are 0.6 GB of ray tensors; 60.7 ms
            # per image against 66.3 with chunk = 1024 launches in round 2, another 0.6 ms against 16k-ray launches).  Rays are
            # independent: the rows are the same, the lists just hold fewer, longer tensors.
            group = max(1, int(getattr(a, 'zest_val_rays', 147456)) // a.chunk)
            try:
                for _ in range(n_chunks):
                    self.chain_bwd = not self.chain_bwd          # every rank keeps the reference's alternation
                chunk_idx = lo
                while chunk_idx < hi:
                    # the largest run of chunks that starts here, is no longer than `group` and that the ray sampler
                    # can address as ONE chunk of n * args.chunk rays (its index must be a whole number)
                    n = next(k for k in range(min(group, hi - chunk_idx), 0, -1) if chunk_idx % k == 0)
                    r = utils.build_rays_dy(
                        sc['imgs'], x['depths'], x['w2cs'], x['c2ws'], x['intrinsics'], x['near_fars'],
                        self.N_samples, N_rays=self.N_rays, stratified=False, pad=sc['pad'], chunk=a.chunk * n,
                        idx=chunk_idx // n, val=True, isRandom=False, scene_flow=True, flow_fwd=x['flow_fwds'],
                        flow_bwd=x['flow_bwds'], mask_fwd=x['mask_fwds'], mask_bwd=x['mask_bwds'],
                        zest_rays_only=True)
                    ret = self._render(sc, (r[0], r[1], r[3], r[4]), time_codes, chain_5frames=False, val=True)
                    for k in self.VAL_KEYS:
                        outs[k].append(ret[k].squeeze(0))
                    chunk_idx += n
            finally:
                a.zest_maps_only = maps_only
            if zest_parallel.collectives_active():
                widths = [3, 1, 3, 1, 3, 1, 1]
                cols = [torch.cat(outs[k]).reshape(-1, w) if outs[k] else sc['imgs'].new_zeros(0, w)
                        for k, w in zip(self.VAL_KEYS, widths)]
                full = zest_parallel.gather_maps(torch.cat(cols, 1), H * W, per=per * a.chunk)
                for k, part in zip(self.VAL_KEYS, torch.split(full, widths, 1)):
                    outs[k] = [part if part.shape[1] > 1 else part[:, 0]]
        return (sc['imgs'],) + tuple(outs[k] for k in self.VAL_KEYS)


# ------------------------------------------------------------------------------------------ GRAF discriminator
class _SpectralConv(nn.Module):
    """The state of one `spectral_norm(Conv2d(cin, cout, 4, stride, pad, bias=False))` of the reference: weight_orig,
    weight_u, weight_v under torch's names, initialised as torch initialises them (Conv2d.reset_parameters, then
    SpectralNorm.apply: u and v normal deviates scaled to unit length, drawn in that order)."""

    def __init__(self, cin, cout):
        super().__init__()
        w = torch.empty(cout, cin, 4, 4)
        nn.init.kaiming_uniform_(w, a=5 ** 0.5)
        self.weight_orig = nn.Parameter(w)
        self.register_buffer("weight_u", nn.functional.normalize(w.new_empty(cout).normal_(0, 1), dim=0, eps=1e-12))
        self.register_buffer("weight_v", nn.functional.normalize(w.new_empty(16 * cin).normal_(0, 1), dim=0, eps=1e-12))


class GRAFDiscriminator(nn.Module):
    """The GRAF patch discriminator (reference networks.py:845-929) on the kernels of csrc/disc.hip: same signature,
    same state-dict keys (`main.<i>.weight_orig / weight_u / weight_v`, <i> the reference's Sequential indices), so
    a reference checkpoint loads with strict=True.  forward(input [..., N, C >= nc]) -> logits [B,1,1,1], one per
    imsize x imsize patch of the rays in their order.  train(): each forward runs one power iteration of the spectral
    norm first and moves weight_u / weight_v in place, also under no_grad; eval(): the stored u and v give sigma.
    There is no torch path: CPU tensors raise.  Not built: hflip (host RNG; train.py never sets it), nc != 3."""

    # Sequential indices of the spectrally normalised convolutions, by imsize
    INDICES = {32: (0, 3, 6, 9), 64: (0, 2, 5, 8, 11), 128: (0, 2, 5, 8, 11, 14)}

    def __init__(self, nc=3, ndf=64, imsize=64, hflip=False):
        super().__init__()
        if hflip:
            raise NotImplementedError("GRAFDiscriminator: hflip=True draws its flips from the host RNG and is not built "
                                      "(the reference's train.py never sets it)")
        if nc != 3:
            raise NotImplementedError("GRAFDiscriminator: nc = %r; the kernels are built for 3-channel patches" % (nc,))
        if imsize not in self.INDICES:
            raise RuntimeError("GRAFDiscriminator: imsize %r is not 32, 64 or 128" % (imsize,))
        step = 32 if imsize == 128 else 16
        if int(ndf) != ndf or ndf < step or ndf % step or ndf > 256:
            raise NotImplementedError("GRAFDiscriminator: ndf = %r; the kernels take multiples of %d up to 256 at imsize %d"
                                      % (ndf, step, imsize))
        self.nc, self.ndf, self.imsize, self.hflip = nc, int(ndf), imsize, False
        chans = {32: (3, 2 * ndf), 64: (3, ndf, 2 * ndf), 128: (3, ndf // 2, ndf, 2 * ndf)}[imsize] + (4 * ndf, 8 * ndf, 1)
        self.main = nn.ModuleDict({str(i): _SpectralConv(cin, cout)
                                   for i, cin, cout in zip(self.INDICES[imsize], chans[:-1], chans[1:])})

    def layers(self):
        return [self.main[str(i)] for i in self.INDICES[self.imsize]]

    def forward(self, input):
        import zest_autograd
        import zest_losses
        who, n = "GRAFDiscriminator", self.imsize * self.imsize
        zest_losses._check_shapes(who, [("input", input, 0)], 2, "[..., N_rays, C >= %d" % self.nc)
        if input.shape[-1] < self.nc:
            raise RuntimeError("%s: input %s has fewer than %d channels" % (who, tuple(input.shape), self.nc))
        rays = input.numel() // input.shape[-1]
        if rays % n:
            raise RuntimeError("%s: %d rays are not a multiple of imsize^2 = %d" % (who, rays, n))
        layers = self.layers()
        named = [("input", input, 0)] + [("main.%d.weight_orig" % i, m.weight_orig, 0) for i, m in zip(self.INDICES[self.imsize], layers)]
        zest_losses._check_devices(who, named)
        x = input[..., :self.nc].float().reshape(-1, self.imsize, self.imsize, self.nc).contiguous()
        logits = zest_autograd.GrafDiscFn.apply(x, self.imsize, self.ndf, self.training, [m.weight_u for m in layers],
                                                [m.weight_v for m in layers], *[m.weight_orig for m in layers])
        return logits.reshape(-1, 1, 1, 1)


# ------------------------------------------------------------------------------------------ LPIPS (AlexNet)
class _State(nn.Module):
    """A module that only holds tensors under the names a state dict gives them."""

    def __init__(self, params=(), buffers=(), children=()):
        super().__init__()
        for name, t in params:
            self.register_parameter(name, nn.Parameter(t, requires_grad=False))
        for name, t in buffers:
            self.register_buffer(name, t)
        for name, m in children:
            self.add_module(name, m)

    def __getitem__(self, name):
        return self._modules[str(name)]


class LPIPS(nn.Module):
    """LPIPS v0.1 with the AlexNet backbone on the kernels of csrc/lpips.hip: the `lpips.LPIPS(net='alex')` of the
    reference's training step (train.py:86, 626-632) and of its val_lpips / test_lpips metric, with that package's
    state-dict keys - written from memory of the package, which is not available where this was built; KEYS below is
    the one place that names them:
        scaling_layer.shift, scaling_layer.scale [1,3,1,1]; net.slice1.0 / slice2.3 / slice3.6 / slice4.8 / slice5.10
        .weight and .bias; lin0.model.1.weight .. lin4.model.1.weight [1,C,1,1].
    The package also carries the lin layers a second time as lins.<k>.model.1.weight: load_state_dict accepts and
    ignores them.  Every weight has requires_grad=False; the initial values are NOT the pretrained ones (they come from
    a state dict: zest_dropin.install(perceptual=True) copies the package's).
    forward(in0, in1, retPerLayer=False, normalize=False): [N,3,H,W], any H, W >= 31, any strides -> [N,1,1,1] (and the
    five per-layer terms).  forward_nhwc takes [N,H,W,3] (channels-last patches, rays in patch order) without a permute
    copy.  The gradient goes to in0 only: in1 is the target.  There is no torch path: CPU tensors raise.
    Not built: the Dropout of the package's lin layers (active when Lightning puts the module in train mode; random, so
    it cannot be pinned: this module evaluates the published metric whatever self.training is), spatial=True,
    net='vgg' / 'squeeze', trainable lin layers, HIP-graph capture, bf16."""

    CONVS = ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3))
    SLICE_INDEX = (0, 3, 6, 8, 10)                           # the convolution's index in torchvision's alexnet.features
    SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
    # state-dict keys, per layer k = 0..4: (weight, bias, lin); the duplicates that are dropped on load start with DROP
    KEYS = tuple(("net.slice%d.%d.weight" % (k + 1, i), "net.slice%d.%d.bias" % (k + 1, i), "lin%d.model.1.weight" % k)
                 for k, i in enumerate(SLICE_INDEX))
    SHIFT_KEY, SCALE_KEY, DROP = "scaling_layer.shift", "scaling_layer.scale", "lins."

    def __init__(self, pretrained=True, net='alex', version='0.1', lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
                 use_dropout=True, model_path=None, eval_mode=True, verbose=False):
        super().__init__()
        if net not in ('alex', 'alexnet'):
            raise NotImplementedError("LPIPS: net=%r; only the AlexNet backbone ('alex') has kernels (the reference's "
                                      "train.py uses no other)" % (net,))
        if spatial:
            raise NotImplementedError("LPIPS: spatial=True returns a map per pixel; only the spatial mean is built")
        if version != '0.1' or not lpips or pnet_tune:
            raise NotImplementedError("LPIPS: version %r, lpips=%r, pnet_tune=%r; only v0.1 with frozen linear layers is built"
                                      % (version, lpips, pnet_tune))
        self.scaling_layer = _State(buffers=[("shift", torch.tensor(self.SHIFT).view(1, 3, 1, 1)),
                                             ("scale", torch.tensor(self.SCALE).view(1, 3, 1, 1))])
        slices = []
        for k, ((cin, cout, ks), i) in enumerate(zip(self.CONVS, self.SLICE_INDEX)):
            w = torch.empty(cout, cin, ks, ks)
            nn.init.kaiming_uniform_(w, a=5 ** 0.5)
            conv = _State(params=[("weight", w), ("bias", torch.zeros(cout))])
            slices.append(("slice%d" % (k + 1), _State(children=[(str(i), conv)])))
            lin = _State(params=[("weight", torch.full((1, cout, 1, 1), 1.0 / cout))])
            self.add_module("lin%d" % k, _State(children=[("model", _State(children=[("1", lin)]))]))
        self.net = _State(children=slices)
        self._packed = None

    def load_state_dict(self, state_dict, strict=True, **kw):
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith(self.DROP)}, strict=strict, **kw)

    def _tensors(self):
        """-> (weights, biases, lins, shift, scale) in the order of the layers."""
        sd = dict(self.named_parameters())
        sd.update(self.named_buffers())
        cols = list(zip(*[[sd[name] for name in keys] for keys in self.KEYS]))
        return list(cols[0]), list(cols[1]), list(cols[2]), sd[self.SHIFT_KEY], sd[self.SCALE_KEY]

    def packed(self):
        """The packed copy of the weight state, rebuilt when a weight's device, storage or version counter moves (an
        in-place change bumps `_version`; a cache compared by identity would miss it)."""
        w, b, lin, shift, scale = self._tensors()
        every = w + b + lin + [shift, scale]
        for t in every:
            if not t.is_cuda:
                raise RuntimeError("LPIPS: a weight is on %s; this path runs only on a HIP device" % (t.device,))
        key = tuple((str(t.device), t.data_ptr(), t._version) for t in every)
        if self._packed is None or self._packed[0] != key:
            c = lambda t: t.detach().float().contiguous()   # noqa: E731
            self._packed = (key, zest_hip.lpips_pack([c(t) for t in w], [c(t) for t in b], [c(t) for t in lin], c(shift), c(scale)))
        return self._packed[1]

    def _run(self, in0, in1, retPerLayer, normalize):
        import zest_autograd
        who = "LPIPS"
        for name, t in (("in0", in0), ("in1", in1)):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3:
                raise RuntimeError("%s: %s must be a tensor [N, 3, H, W], got %s"
                                   % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        if in0.shape != in1.shape:
            raise RuntimeError("%s: in1 %s does not match in0 %s" % (who, tuple(in1.shape), tuple(in0.shape)))
        if in0.shape[0] < 1 or min(in0.shape[2:]) < zest_hip.LPIPS_MIN_SIDE:
            raise RuntimeError("%s: %s is an empty batch or a frame below %d x %d, the smallest with a pixel in every layer"
                               % (who, tuple(in0.shape), zest_hip.LPIPS_MIN_SIDE, zest_hip.LPIPS_MIN_SIDE))
        for name, t in (("in0", in0), ("in1", in1)):
            if not t.is_cuda:
                raise RuntimeError("%s: %s is on %s; this path runs only on a HIP device" % (who, name, t.device))
        if in1.device != in0.device:
            raise RuntimeError("%s: in1 is on %s, in0 on %s" % (who, in1.device, in0.device))
        packed = self.packed()
        if packed.device != in0.device:
            raise RuntimeError("%s: the weights are on %s, in0 on %s" % (who, packed.device, in0.device))
        res = zest_autograd.LpipsFn.apply(in0.float(), in1.detach().float(), packed, bool(normalize), torch.is_grad_enabled())
        val = res[:, 0].reshape(-1, 1, 1, 1)
        if retPerLayer:
            return val, [res[:, 1 + k].reshape(-1, 1, 1, 1) for k in range(zest_hip.LPIPS_LAYERS)]
        return val

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        return self._run(in0, in1, retPerLayer, normalize)

    def forward_nhwc(self, in0, in1, retPerLayer=False, normalize=False):
        """forward for in0, in1 [N,H,W,3]: channels-last images, or rays reshaped to patches; read in place."""
        for name, t in (("in0", in0), ("in1", in1)):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[-1] != 3:
                raise RuntimeError("LPIPS: %s must be a tensor [N, H, W, 3], got %s"
                                   % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
        return self._run(in0.permute(0, 3, 1, 2), in1.permute(0, 3, 1, 2), retPerLayer, normalize)
