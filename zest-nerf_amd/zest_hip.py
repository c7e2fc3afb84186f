"""ctypes binding of libzest_hip.so (include/zest_render.h) for torch tensors.

The library is the product: if it is missing or a call fails this module raises — there
is no PyTorch or CPU fallback anywhere in the package.  Tensors cross the boundary as raw
device pointers (`Tensor.data_ptr()`), sizes, and the current HIP stream handle; outputs
are allocated here through torch's caching allocator (the reference allocates every
output fresh as well, renderer.py:64, utils.py:480).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZEST_HIP_LIB selects an experiment build (build_hip.py --tag); default is the product library
LIB_PATH = os.environ.get("ZEST_HIP_LIB") or os.path.join(_HERE, "libzest_hip.so")

# arithmetic of the MLP contraction (include/zest_render.h ZEST_PREC_*): exact-product fp32 MFMA;
# bf16 / fp16 operands; split-fp16 pairs (fp32-class results on the fp16 matrix pipe)
PREC_F32, PREC_BF16, PREC_F16, PREC_F16X3 = 0, 1, 2, 3
ENGINE_PRECISIONS = (PREC_BF16, PREC_F16, PREC_F16X3)
PREC_NAMES = {PREC_F32: "f32", PREC_BF16: "bf16", PREC_F16: "f16", PREC_F16X3: "f16x3"}
HEAD_NONE, HEAD_BLEND, HEAD_DYNAMIC = 0, 1, 2
GEMM_LIBRARY, GEMM_SPLIT_BF16 = 0, 1          # ZEST_GEMM_*: the GEMMs of the fp32 training path
GEMM_NAMES = {"library": GEMM_LIBRARY, "split": GEMM_SPLIT_BF16}
GEMM_OP_NT, GEMM_OP_NN, GEMM_OP_TN = 0, 1, 2
P_COUNT = 15

_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_fp = C.POINTER(C.c_float)


class MlpDesc(C.Structure):
    _fields_ = [("in_ch_pts", C.c_int32), ("in_ch_feat", C.c_int32), ("in_ch_views", C.c_int32),
                ("use_feat", C.c_int32), ("net_type", C.c_int32), ("head", C.c_int32),
                ("depth", C.c_int32), ("width", C.c_int32), ("skip_mask", C.c_int32)]

    @property
    def D(self):
        return self.depth or 8

    @property
    def W(self):
        return self.width or 256

    @property
    def skips(self):
        """Reference `skips` list (networks.py:93-100): layer i+1 takes [pts | h] for i in skips."""
        mask = self.skip_mask if (self.depth or self.width or self.skip_mask) else 1 << 4
        return [i for i in range(8) if mask >> i & 1]

    @property
    def is_default_shape(self):
        return self.D == 8 and self.W == 256 and self.skips == [4]

    @property
    def in_ch(self):
        return self.in_ch_pts + (self.in_ch_feat if self.use_feat else 0) + self.in_ch_views

    @property
    def out_ch(self):
        return {HEAD_NONE: 4, HEAD_BLEND: 5, HEAD_DYNAMIC: 12}[self.head]


class ViewSet(C.Structure):
    _fields_ = [("vol_cl", _vp), ("D", C.c_int32), ("Hv", C.c_int32), ("Wv", C.c_int32),
                ("imgs_cl", _vp), ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("w2cs", _vp), ("intrinsics", _vp)]


_SIGS = {
    "zest_abi_version": (_i, []),
    "zest_last_error": (C.c_char_p, []),
    "zest_device_info": (_i, [C.POINTER(_i), C.POINTER(_i), C.c_char_p, _sz]),
    "zest_composite_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zest_composite_blend_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zest_weighted_complement_sum": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "zest_embed_fwd": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "zest_volume_to_cl": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "zest_images_to_cl": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "zest_nchw_to_nhwc": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "zest_distortion_fwd": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "zest_project_rays_fwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _i, _i, _vp, _vp]),
    "zest_project_rays_bwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp, _i, _i, _vp, _vp, _vp]),
    "zest_sf_reg_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zest_sf_sample_fwd": (_i, [_vp] * 8 + [_i, _i, _i, _vp, _vp]),
    "zest_sf_sample_bwd": (_i, [_vp] * 8 + [_i, _i, _i, _vp, _f, _f, _f, _f] + [_vp] * 8 + [_vp]),
    "zest_sf_ray_fwd": (_i, [_vp] * 17 + [_i, _i, _i, _i, _f, _f, _f, _f, _vp, _vp]),
    "zest_sf_ray_bwd": (_i, [_vp] * 17 + [_i, _i, _i, _i, _vp, _f, _f, _f, _f] + [_vp] * 10 + [_vp]),
    "zest_patch_terms_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _vp]),
    "zest_patch_terms_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _vp]),
    "zest_disc_layout": (_i, [_i, _i, _i, C.POINTER(C.c_longlong)]),
    "zest_disc_fwd": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i, _vp, _vp, _vp, _vp]),
    "zest_disc_bwd": (_i, [_vp, _i, _i, _i, C.POINTER(_vp), _vp, _vp, _vp, _vp, C.POINTER(_vp), _vp]),
    "zest_lpips_layout": (_i, [_i, _i, _i, C.POINTER(C.c_longlong)]),
    "zest_lpips_pack": (_i, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp, _vp, _vp, _vp]),
    "zest_lpips_fwd": (_i, [_vp, C.POINTER(C.c_longlong), _vp, C.POINTER(C.c_longlong), _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "zest_lpips_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, C.POINTER(C.c_longlong), _vp]),
    "zest_image_metrics_tile": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "zest_image_metrics_work_bytes": (_sz, [_i, _i, _i, _i]),
    "zest_image_metrics": (_i, [_vp, C.POINTER(C.c_longlong), _vp, C.POINTER(C.c_longlong), _i, _i, _i, _i, _i, _i, _f,
                                _vp, _vp, _vp, _vp, _sz, _vp]),
    "zest_adam_chunk": (_i, []),
    "zest_adam_max_tensors": (_i, []),
    "zest_adam_max_slots": (_i, []),
    "zest_adam_plan": (C.c_longlong, [C.POINTER(C.c_longlong), _i, C.POINTER(_i), C.POINTER(C.c_longlong), C.c_longlong]),
    "zest_adam_work_bytes": (_sz, [C.c_longlong]),
    "zest_adam_step": (_i, [_vp, _vp, _vp, _i, C.POINTER(_i), C.POINTER(C.c_longlong), C.POINTER(_vp), C.POINTER(_f), _i, _f,
                            _vp, _sz, _vp, _vp]),
    "zest_adam_step_amp": (_i, [_vp, _vp, _vp, _i, C.POINTER(_i), C.POINTER(C.c_longlong), C.POINTER(_i), C.POINTER(_vp),
                                C.POINTER(C.c_double), _i, _f, _vp, _sz, _vp, _vp, _vp, _i, _vp, _i, _vp]),
    "zest_volume_cost_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_homo_warp_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_volume_cost_cl_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "zest_costreg_stat_rows": (_i, []),
    "zest_costreg_conv_launch_shape": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "zest_costreg_deconv_launch_shape": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "zest_conv2d_packed_bytes": (_sz, [_i, _i, _i, _i]),
    "zest_conv2d_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_costreg_packed_bytes": (_sz, [_i, _i, _i]),
    "zest_costreg_conv_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_costreg_deconv_packed_bytes": (_sz, [_i, _i, _i]),
    "zest_costreg_deconv_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_costreg_bn": (_i, [_vp, _i, C.c_longlong, _vp, _vp, _f, _i, _vp, _vp, _f, _vp, _vp, _vp, _vp]),
    "zest_costreg_out": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "zest_costreg_bn_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, C.c_longlong, _vp, _vp, _vp, _vp]),
    "zest_costreg_wgrad_launch_shape": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "zest_costreg_wgrad_work_bytes": (_sz, [_i, _i, _i]),
    "zest_costreg_wgrad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_costreg_dgrad_launch_shape": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i)]),
    "zest_costreg_dgrad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "zest_feature_wgrad_launch_shape": (_i, [_i] * 7 + [C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz)]),
    "zest_feature_wgrad": (_i, [_vp] + [C.c_longlong] * 4 + [_vp, _vp] + [_i] * 7 + [_vp, _vp, _vp]),
    "zest_feature_dgrad_launch_shape": (_i, [_i] * 7 + [C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz)]),
    "zest_feature_dgrad": (_i, [_vp, _vp] + [_i] * 7 + [_vp, _vp, _vp]),
    "zest_feature_top_bwd_launch_shape": (_i, [_i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_sz)]),
    "zest_feature_top_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "zest_volume_cost_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_homo_warp_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_volume_cost_bwd_det_work_bytes": (_sz, [_i, _i, _i]),
    "zest_volume_cost_bwd_det": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "zest_homo_warp_bwd_det_work_bytes": (_sz, [_i, _i, _i]),
    "zest_homo_warp_bwd_det": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "zest_volume_lookup_fwd": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "zest_color_lookup_fwd": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "zest_encode_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _i, _i, _i, _vp, _i, _i, _i,
                             _vp, _vp, _vp, _vp]),
    "zest_gather_encode_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _i, _i, _i, _vp, _i, _i, _i,
                                    _vp, _vp, _vp, _vp]),            # = zest_encode_fwd (SURVEY 8(b)'s name)
    "zest_build_rays_fwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i,
                                 _vp, _vp, _vp, _vp, _vp]),
    "zest_sample_pdf_fwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "zest_ndc_fwd": (_i, [_vp, _i, _vp, _vp, _f, _f, _f, _f, _i, _i, _vp, _vp]),
    "zest_composite_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "zest_composite_blend_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp]),
    "zest_encode_bwd": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "zest_encode_bwd_det_work_bytes": (_sz, [_i, _i, _i]),
    "zest_encode_bwd_det": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "zest_volume_from_cl": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "zest_mlp_train_saved_floats": (_sz, [C.POINTER(MlpDesc), _i]),
    "zest_mlp_train_workspace_floats": (_sz, [C.POINTER(MlpDesc), _i]),
    "zest_mlp_train_fwd": (_i, [C.POINTER(MlpDesc), C.POINTER(_vp), _vp, _i, _vp, _vp, _vp, _vp]),
    "zest_mlp_train_bwd": (_i, [C.POINTER(MlpDesc), C.POINTER(_vp), _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                C.POINTER(_vp), _vp]),
    "zest_mlp_train_workspace_floats_ex": (_sz, [C.POINTER(MlpDesc), _i, _i]),
    "zest_mlp_train_fwd_ex": (_i, [C.POINTER(MlpDesc), C.POINTER(_vp), _vp, _i, _vp, _vp, _vp, _vp, _i]),
    "zest_mlp_train_bwd_ex": (_i, [C.POINTER(MlpDesc), C.POINTER(_vp), _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                   C.POINTER(_vp), _vp, _i]),
    "zest_mlp_train_workspace_floats_det": (_sz, [C.POINTER(MlpDesc), _i, _i]),
    "zest_mlp_train_bwd_det": (_i, [C.POINTER(MlpDesc), C.POINTER(_vp), _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                    C.POINTER(_vp), _vp, _i]),
    "zest_colsum_ordered_work_floats": (_sz, [_i, _i]),
    "zest_colsum_ordered": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "zest_train_gemm_workspace_floats": (_sz, [_i, _i, _i, _i]),
    "zest_train_gemm_chunk_rows": (_i, []),
    "zest_train_gemm": (_i, [_i, _i, _i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _f, _vp, _vp]),
    "zest_mlp_train16_stash_bytes": (_sz, [C.POINTER(MlpDesc), _i]),
    "zest_mlp_train16_work_bytes": (_sz, [C.POINTER(MlpDesc), _i]),
    "zest_mlp_train16_packed_bytes": (_sz, [C.POINTER(MlpDesc)]),
    "zest_mlp_train16_pack": (_i, [C.POINTER(MlpDesc), C.POINTER(_vp), _vp, _vp]),
    "zest_mlp_train16_fwd": (_i, [C.POINTER(MlpDesc), _vp, _vp, _i, _vp, _vp, _vp]),
    "zest_mlp_train16_bwd": (_i, [C.POINTER(MlpDesc), _vp, C.POINTER(_vp), _vp, _i, _vp, _vp, _vp, _vp, _vp,
                                  C.POINTER(_vp), _i, _vp]),
    "zest_mlp_packed_bytes": (_sz, [C.POINTER(MlpDesc), _i]),
    "zest_mlp_pack": (_i, [C.POINTER(MlpDesc), _i, C.POINTER(_vp), _vp, _vp]),
    "zest_pack_weights": (_i, [C.POINTER(MlpDesc), _i, C.POINTER(_vp), _vp, _vp]),       # = zest_mlp_pack
    "zest_mlp_fwd": (_i, [C.POINTER(MlpDesc), _i, _vp, _vp, _i, _vp, _vp]),
    "zest_render_fused_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.POINTER(MlpDesc), _vp,
                                   C.POINTER(ViewSet), C.POINTER(MlpDesc), _vp, C.POINTER(ViewSet),
                                   _f, _i, _i, _vp, _vp, _vp]),
    "zest_render_fused_workspace": (_sz, [_i, _i]),
    "zest_render_fused_set_passes": (_i, [_i]),
    "zest_render_fused_pass_shape": (_i, [_i, _i, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
}

_lib = None


def exported_symbols():
    """Names include/zest_render.h declares (used by the CPU symbol test)."""
    return list(_SIGS)


def lib():
    """Load the shared library once; raise if it is absent (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not found: build it with `python %s/build_hip.py` "
                               "(zest-nerf_amd has no non-HIP execution path)" % (LIB_PATH, _HERE))
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)           # AttributeError if the header and library disagree
            fn.restype, fn.argtypes = res, args
        if L.zest_abi_version() != 3:
            raise RuntimeError("libzest_hip.so ABI %d != 3: rebuild it (python zest-nerf_amd/build_hip.py)"
                               % L.zest_abi_version())
        _lib = L
    return _lib


def _check(code, what):
    if code != 0:
        msg = lib().zest_last_error().decode(errors="replace")
        raise RuntimeError("%s failed (hipError %d): %s" % (what, code, msg))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _dev(t, name, shape=None):
    """Normalise to a contiguous fp32 device tensor; reject CPU tensors loudly.  shape: the extents the
    kernel will index with (None entries: any) - the C ABI sees pointers and sizes only, so a tensor of
    another shape would be read out of bounds: refuse it here, with both shapes in the message."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("zest_hip: %s is on %s; this path runs only on a HIP device" % (name, t.device))
    if shape is not None and (t.dim() != len(shape) or any(w is not None and int(w) != g for w, g in zip(shape, t.shape))):
        raise RuntimeError("zest_hip: %s has shape %s, expected %s" % (
            name, tuple(t.shape), tuple("*" if w is None else int(w) for w in shape)))
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


# ------------------------------------------------------------------------ compositing
def _spacing(z, rays_dir, dists):
    """The sample spacing is either rebuilt in the kernel from z and |rays_dir| (depth2dist) or taken
    from the caller's `dists` [R,S]."""
    if z.dim() != 2:
        raise RuntimeError("zest_hip: z has shape %s, expected (R, S)" % (tuple(z.shape),))
    rays_dir, dists = _dev(rays_dir, "rays_dir", (z.shape[0], 3)), _dev(dists, "dists", z.shape)
    if rays_dir is None and dists is None:
        raise RuntimeError("zest_hip: compositing needs rays_dir or dists")
    return rays_dir, dists


def composite(raw, z, rays_dir, noise=None, noise_std=0.0, white_bkgd=False, want_disp=True, dists=None):
    """raw [R,S,4], z [R,S], rays_dir [R,3] (or dists [R,S]) -> rgb_map, disp, acc, weights, depth, alpha."""
    z = _dev(z, "z")
    rays_dir, dists = _spacing(z, rays_dir, dists)
    R, S = z.shape
    raw, noise = _dev(raw, "raw", (R, S, 4)), _dev(noise, "noise", (R, S))
    o = lambda *s: torch.empty(*s, device=z.device, dtype=torch.float32)
    rgb, depth, acc, disp, w, a = o(R, 3), o(R), o(R), o(R), o(R, S), o(R, S)
    _check(lib().zest_composite_fwd(_ptr(raw), _ptr(z), _ptr(rays_dir), _ptr(dists), _ptr(noise), float(noise_std),
                                    int(bool(white_bkgd)), R, S, _ptr(rgb), _ptr(depth), _ptr(acc),
                                    _ptr(disp), _ptr(w), _ptr(a), _stream(z)), "zest_composite_fwd")
    return rgb, disp, acc, w, depth, a


def composite_blend(raw_dy, raw_st, blend, z, rays_dir, noise=None, noise_std=0.0, dists=None):
    z = _dev(z, "z")
    rays_dir, dists = _spacing(z, rays_dir, dists)
    R, S = z.shape
    raw_dy, raw_st = _dev(raw_dy, "raw_dy", (R, S, 4)), _dev(raw_st, "raw_st", (R, S, 4))
    blend, noise = _dev(blend, "blend", (R, S)), _dev(noise, "noise", (R, S))
    o = lambda *s: torch.empty(*s, device=z.device, dtype=torch.float32)
    rgb, depth, rgb_fg, depth_fg, w_fg, w_dy, dd = o(R, 3), o(R), o(R, 3), o(R), o(R, S), o(R, S), o(R)
    _check(lib().zest_composite_blend_fwd(_ptr(raw_dy), _ptr(raw_st), _ptr(blend), _ptr(z),
                                          _ptr(rays_dir), _ptr(dists), _ptr(noise), float(noise_std), R, S,
                                          _ptr(rgb), _ptr(depth), _ptr(rgb_fg), _ptr(depth_fg),
                                          _ptr(w_fg), _ptr(w_dy), _ptr(dd), _stream(z)),
           "zest_composite_blend_fwd")
    return rgb, depth, rgb_fg, depth_fg, w_fg, w_dy, dd


def weighted_complement_sum(w, p):
    w = _dev(w, "w", (None, None))
    R, S = w.shape
    p = _dev(p, "p", (R, S))
    out = torch.empty(R, device=w.device, dtype=torch.float32)
    _check(lib().zest_weighted_complement_sum(_ptr(w), _ptr(p), R, S, _ptr(out), _stream(w)),
           "zest_weighted_complement_sum")
    return out


# --------------------------------------------------------------------- per-sample operators
def embed(x, n_freqs):
    x = _dev(x, "x")
    Cn = x.shape[-1]
    M = x.numel() // Cn
    y = torch.empty(*x.shape[:-1], Cn * (2 * n_freqs + 1), device=x.device, dtype=torch.float32)
    _check(lib().zest_embed_fwd(_ptr(x), M, Cn, n_freqs, _ptr(y), _stream(x)), "zest_embed_fwd")
    return y


def volume_to_cl(vol):
    """[1,8,D,H,W] or [8,D,H,W] -> the kernels' copy: channels-last, depth innermost [H,W,D,8]."""
    vol = _dev(vol, "volume")
    if vol.dim() == 5:
        if vol.shape[0] != 1:
            raise RuntimeError("zest_hip: volume batch must be 1, got %d" % vol.shape[0])
        vol = vol[0]
    if vol.shape[0] != 8:
        raise RuntimeError("zest_hip: encoding volume must have 8 channels, got %d" % vol.shape[0])
    _, D, H, W = vol.shape
    out = torch.empty(H, W, D, 8, device=vol.device, dtype=torch.float32)
    _check(lib().zest_volume_to_cl(_ptr(vol), D, H, W, _ptr(out), _stream(vol)), "zest_volume_to_cl")
    return out


def distortion(weights, t_vals, want_grad=True):
    """weights [R,S], t_vals [1,S] or [R,S] -> (loss_ray [R], d loss_ray / d weights [R,S] or None)."""
    weights = _dev(weights, "ray_weights", (None, None))
    R, S = weights.shape
    t_vals = _dev(t_vals, "t_vals", (None, S))
    if t_vals.shape[0] not in (1, R):
        raise RuntimeError("zest_hip: t_vals has %d rows, expected 1 or %d" % (t_vals.shape[0], R))
    loss = torch.empty(R, device=weights.device, dtype=torch.float32)
    grad = torch.empty(R, S, device=weights.device, dtype=torch.float32) if want_grad else None
    _check(lib().zest_distortion_fwd(_ptr(weights), _ptr(t_vals), t_vals.shape[0], R, S, _ptr(loss), _ptr(grad),
                                     _stream(weights)), "zest_distortion_fwd")
    return loss, grad


def project_rays(weights, pts, w2c, H, W, focal):
    """weights [R,S], pts [R,S,3], w2c [4,4] (or [3,4]) -> [R,2]."""
    weights = _dev(weights, "weights_ref", (None, None))
    R, S = weights.shape
    pts, w2c = _dev(pts, "raw_pts", (R, S, 3)), _dev(w2c, "w2c", (None, 4))
    if w2c.shape[0] < 3:
        raise RuntimeError("zest_hip: w2c has shape %s, expected (3 or 4, 4)" % (tuple(w2c.shape),))
    out = torch.empty(R, 2, device=weights.device, dtype=torch.float32)
    _check(lib().zest_project_rays_fwd(_ptr(weights), _ptr(pts), _ptr(w2c), int(H), int(W), float(focal), R, S,
                                       _ptr(out), _stream(weights)), "zest_project_rays_fwd")
    return out


def project_rays_bwd(weights, pts, w2c, H, W, focal, grad_out, want_w=True, want_pts=True):
    weights = _dev(weights, "weights_ref", (None, None))
    R, S = weights.shape
    pts, w2c, grad_out = _dev(pts, "raw_pts", (R, S, 3)), _dev(w2c, "w2c", (None, 4)), _dev(grad_out, "grad", (R, 2))
    if w2c.shape[0] < 3:
        raise RuntimeError("zest_hip: w2c has shape %s, expected (3 or 4, 4)" % (tuple(w2c.shape),))
    dw = torch.empty(R, S, device=weights.device, dtype=torch.float32) if want_w else None
    dp = torch.empty(R, S, 3, device=weights.device, dtype=torch.float32) if want_pts else None
    _check(lib().zest_project_rays_bwd(_ptr(weights), _ptr(pts), _ptr(w2c), int(H), int(W), float(focal),
                                       _ptr(grad_out), R, S, _ptr(dw), _ptr(dp), _stream(weights)),
           "zest_project_rays_bwd")
    return dw, dp


SF_SMOOTH_REF_POST, SF_SMOOTH_REF_PREV, SF_LKE_REF, SF_LKE_CHAIN_BWD, SF_LKE_CHAIN_FWD = 1, 2, 4, 8, 16
SF_SPATIAL = SF_SMOOTH_REF_POST | SF_SMOOTH_REF_PREV
SF_TEMPORAL = SF_LKE_REF | SF_LKE_CHAIN_BWD | SF_LKE_CHAIN_FWD


def _term_inputs(who, tensors, table, terms, all_terms, lead_rank, lead_check, gates=None):
    """The checks the loss-kernel families share, made before the library is touched.  tensors: as given, None where no
    requested term reads one; table: rows (name, trailing extent or 0, terms that read it, ...) in the order of the C ABI;
    lead_rank: the leading extents all tensors share ([R,S]: 2, [R]: 1, [P,H,W]: 3); lead_check(who, terms, first, lead):
    the family's own refusals of the leading shape; gates: name -> whether the terms read that tensor at all in this call
    -> (the first tensor given, lead, terms).  In turn: the mask, a missing tensor, the leading shape, then each
    tensor's device before its shape, dtype and contiguity."""
    terms = int(terms)
    if len(tensors) != len(table):
        raise RuntimeError("zest_hip: %s takes %d tensors, got %d" % (who, len(table), len(tensors)))
    if terms <= 0 or terms & ~all_terms:
        raise RuntimeError("zest_hip: %s: bad term mask 0x%x" % (who, terms))
    for t, row in zip(tensors, table):
        if t is None and terms & row[2] and (gates is None or gates.get(row[0], True)):
            raise RuntimeError("zest_hip: %s: terms 0x%x read %s, which is None" % (who, terms, row[0]))
    first = next(t for t in tensors if t is not None)       # every term reads a tensor: there is one
    lead = tuple(int(n) for n in first.shape[:lead_rank])
    lead_check(who, terms, first, lead)
    for t, row in zip(tensors, table):
        if t is None:
            continue
        name, want = row[0], lead + ((row[1],) if row[1] else ())
        if not t.is_cuda:
            raise RuntimeError("zest_hip: %s is on %s; this path runs only on a HIP device" % (name, t.device))
        if tuple(t.shape) != want or t.dtype != torch.float32 or not t.is_contiguous() or t.device != first.device:
            raise RuntimeError("zest_hip: %s: %s must be a contiguous fp32 %s on %s, got %s %s on %s"
                               % (who, name, want, first.device, t.dtype, tuple(t.shape), t.device))
    return first, lead, terms


def _grad_buffers(who, inputs, want, grads, device):
    """One gradient buffer per input: None where `want` is false or the input is None, else the given buffer (checked)
    or a fresh one."""
    out = []
    for k, t in enumerate(inputs):
        g = None
        if want[k] and t is not None:
            g = grads[k] if grads is not None and grads[k] is not None else torch.empty_like(t)
            if g.shape != t.shape or g.dtype != torch.float32 or not g.is_contiguous() or g.device != device:
                raise RuntimeError("zest_hip: %s gradient buffer %d must be a contiguous fp32 %s on %s"
                                   % (who, k, tuple(t.shape), device))
        out.append(g)
    return out


def _totals_row(who, totals, cols, device):
    if not torch.is_tensor(totals) or tuple(totals.shape) != (cols,) or totals.dtype != torch.float32 \
            or not totals.is_contiguous() or totals.device != device:
        raise RuntimeError("zest_hip: %s: totals must be a contiguous fp32 (%d,) on %s" % (who, cols, device))


def sf_reg(ref, post, prev, pp, terms, H, W, focal, w_sp=1.0, w_st=1.0, want=(True, True, True, True), grads=None):
    """Scene-flow regularisers, one launch: ref / post / prev / pp [R,S,3] NDC points (None where no requested
    term reads the tensor), terms a mask of SF_* -> (loss_ray [R,2]: per-ray parts of the spatial and the temporal
    sum, already divided by the means' denominators; [d_ref, d_post, d_prev, d_pp]: d (w_sp * spatial + w_st *
    temporal) / d tensor, [R,S,3] each, None where `want` is false or the tensor is None).  grads: optional
    preallocated [R,S,3] fp32 tensors (or None) to write the gradients into; every row of them is written."""
    ref = _dev(ref, "ref", (None, None, 3))
    R, S = int(ref.shape[0]), int(ref.shape[1])
    pts = [ref] + [_dev(t, n, (R, S, 3)) for t, n in ((post, "post"), (prev, "prev"), (pp, "pp"))]
    n95, n90 = int(S * 0.95), int(S * 0.9)                      # the reference's slice lengths, its expressions
    terms = int(terms)
    if R < 1 or terms <= 0 or (terms & SF_SPATIAL and n95 < 2) or (terms & SF_TEMPORAL and n90 < 1):
        raise RuntimeError("zest_hip: sf_reg needs R >= 1, a term, int(S * 0.95) >= 2 for a spatial and int(S * 0.9) >= 1 "
                           "for a temporal term; got R=%d S=%d terms=0x%x" % (R, S, terms))
    scale_sp = 1.0 / (3.0 * R * (n95 - 1)) if n95 >= 2 else 0.0
    scale_st = 1.0 / (3.0 * R * n90) if n90 >= 1 else 0.0
    out = _grad_buffers("sf_reg", pts, want, grads, ref.device)
    loss_ray = torch.empty(R, 2, device=ref.device, dtype=torch.float32)
    _check(lib().zest_sf_reg_fwd(_ptr(pts[0]), _ptr(pts[1]), _ptr(pts[2]), _ptr(pts[3]), terms, R, S, n95, n90,
                                 int(H), int(W), float(focal), scale_sp, scale_st, float(w_sp), float(w_st),
                                 _ptr(loss_ray), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
                                 _stream(ref)), "zest_sf_reg_fwd")
    return loss_ray, out


SFS_CYCLE, SFS_PROB_REG, SFS_SF_MIN, SFS_ENTROPY = 1, 2, 4, 8
SFS_ALL = SFS_CYCLE | SFS_PROB_REG | SFS_SF_MIN | SFS_ENTROPY
SF_SAMPLE_COLS = 9
# the tensors of the per-sample terms, in the order of the C ABI, their trailing extent (0: none) and the terms that read them
SF_SAMPLE_TENSORS = (("sf_ref2post", 3, SFS_CYCLE | SFS_SF_MIN), ("sf_post2ref", 3, SFS_CYCLE),
                     ("sf_ref2prev", 3, SFS_CYCLE | SFS_SF_MIN), ("sf_prev2ref", 3, SFS_CYCLE),
                     ("prob_ref2post", 0, SFS_CYCLE | SFS_PROB_REG), ("prob_ref2prev", 0, SFS_CYCLE | SFS_PROB_REG),
                     ("weights", 0, SFS_SF_MIN), ("blend", 0, SFS_ENTROPY))


def _sf_sample_lead(who, terms, first, lead):
    if len(lead) < 2:
        raise RuntimeError("zest_hip: %s needs tensors [R,S] and [R,S,3], got %s" % (who, tuple(first.shape)))
    if min(lead) < 1:
        raise RuntimeError("zest_hip: %s needs R >= 1 and S >= 1, got R=%d S=%d" % ((who,) + lead))


def sf_sample_fwd(tensors, terms=SFS_ALL):
    """Per-sample terms of the scene-flow training loss, forward launch.  tensors: the eight of SF_SAMPLE_TENSORS,
    contiguous fp32 [R,S,3] / [R,S] (None where no requested term reads one) -> partials [R, SF_SAMPLE_COLS], one row
    of partial sums per ray (include/zest_render.h names the columns)."""
    first, (R, S), terms = _term_inputs("sf_sample_fwd", tensors, SF_SAMPLE_TENSORS, terms, SFS_ALL, 2, _sf_sample_lead)
    partials = torch.empty(R, SF_SAMPLE_COLS, device=first.device, dtype=torch.float32)
    _check(lib().zest_sf_sample_fwd(*[_ptr(t) for t in tensors], terms, R, S, _ptr(partials), _stream(first)),
           "zest_sf_sample_fwd")
    return partials


def sf_sample_bwd(tensors, totals, terms=SFS_ALL, coeff=(1.0, 1.0, 1.0, 1.0), want=(True,) * 8, grads=None):
    """Backward launch: totals [SF_SAMPLE_COLS] = sf_sample_fwd(...).sum(0) (it stays on the device), coeff = (c_cyc, c_prob, c_min, c_ent) -> the gradients of c_cyc cycle + c_prob prob_reg +
    c_min sf_min + c_ent entropy with respect to the eight tensors (None where `want` is false or the tensor is None).
    grads: optional preallocated tensors (or None) to write into; every row of them is written."""
    first, (R, S), terms = _term_inputs("sf_sample_bwd", tensors, SF_SAMPLE_TENSORS, terms, SFS_ALL, 2, _sf_sample_lead)
    _totals_row("sf_sample_bwd", totals, SF_SAMPLE_COLS, first.device)
    out = _grad_buffers("sf_sample_bwd", tensors, want, grads, first.device)
    c = [float(v) for v in coeff]
    _check(lib().zest_sf_sample_bwd(*[_ptr(t) for t in tensors], terms, R, S, _ptr(totals), *c,
                                    *[_ptr(g) for g in out], _stream(first)), "zest_sf_sample_bwd")
    return out


SFR_PHO, SFR_COMBINED, SFR_FLOW_FWD, SFR_FLOW_BWD, SFR_DEPTH = 1, 2, 4, 8, 16
SFR_ALL = SFR_PHO | SFR_COMBINED | SFR_FLOW_FWD | SFR_FLOW_BWD | SFR_DEPTH
SF_RAY_COLS = 26
SF_RAY_FWD_THREADS, SF_RAY_BWD_THREADS = 1024, 256       # the forward's only workgroup; rays per workgroup of the backward
# the tensors of the per-ray terms, in the order of the C ABI: name, trailing extent (0: none), the terms that read it
# (rgb_pp_dy only with five_frames, weights_dd only with late_phase or five_frames), whether it takes a gradient
SF_RAY_TENSORS = (("target", 3, SFR_PHO | SFR_COMBINED, False), ("rgb_ref", 3, SFR_COMBINED, True),
                  ("rgb_ref_dy", 3, SFR_PHO, True), ("rgb_post_dy", 3, SFR_PHO, True), ("rgb_prev_dy", 3, SFR_PHO, True),
                  ("rgb_pp_dy", 3, SFR_PHO, True), ("prob_post", 0, SFR_PHO, True), ("prob_prev", 0, SFR_PHO, True),
                  ("weights_dd", 0, SFR_PHO, False), ("flow_fwd", 2, SFR_FLOW_FWD, True), ("flow_fwd_gt", 2, SFR_FLOW_FWD, False),
                  ("mask_fwd", 0, SFR_FLOW_FWD, False), ("flow_bwd", 2, SFR_FLOW_BWD, True), ("flow_bwd_gt", 2, SFR_FLOW_BWD, False),
                  ("mask_bwd", 0, SFR_FLOW_BWD, False), ("depth", 0, SFR_DEPTH, True), ("depth_gt", 0, SFR_DEPTH, False))
SF_RAY_GRADS = tuple(k for k, t in enumerate(SF_RAY_TENSORS) if t[3])        # positions of the ten that take a gradient


def _sf_ray_lead(who, terms, first, lead):
    if not lead or lead[0] < 1:
        raise RuntimeError("zest_hip: %s needs R >= 1, got %s" % (who, tuple(first.shape)))


def _sf_ray_inputs(who, tensors, terms, late_phase, five_frames):
    """_term_inputs for the seventeen tensors, two of which the photometric term reads in some phases only
    -> (first, R, terms)."""
    gates = {"rgb_pp_dy": bool(five_frames), "weights_dd": bool(late_phase or five_frames)}
    first, (R,), terms = _term_inputs(who, tensors, SF_RAY_TENSORS, terms, SFR_ALL, 1, _sf_ray_lead, gates)
    return first, R, terms


def sf_ray_fwd(tensors, terms=SFR_ALL, late_phase=False, five_frames=True, coeff=(1.0, 1.0, 1.0, 1.0)):
    """Per-ray terms of the scene-flow training loss, forward launch.  tensors: the seventeen of SF_RAY_TENSORS,
    contiguous fp32 [R,3] / [R,2] / [R] (None where no requested term reads one) -> result [SF_RAY_COLS]: pho, combined,
    flow, depth, then the sums, medians and scales the backward reads, last c_pho pho + c_comb combined + c_flow flow +
    c_depth depth for coeff = (c_pho, c_comb, c_flow, c_depth) (include/zest_render.h names the columns)."""
    first, R, terms = _sf_ray_inputs("sf_ray_fwd", tensors, terms, late_phase, five_frames)
    result = torch.empty(SF_RAY_COLS, device=first.device, dtype=torch.float32)
    _check(lib().zest_sf_ray_fwd(*[_ptr(t) for t in tensors], terms, int(bool(late_phase)), int(bool(five_frames)), R,
                                 *[float(v) for v in coeff], _ptr(result), _stream(first)), "zest_sf_ray_fwd")
    return result


def sf_ray_bwd(tensors, totals, terms=SFR_ALL, late_phase=False, five_frames=True, coeff=(1.0, 1.0, 1.0, 1.0),
               want=(True,) * 10, grads=None):
    """Backward launch: totals [SF_RAY_COLS] = sf_ray_fwd(...) (it stays on the device), coeff = (c_pho, c_comb, c_flow,
    c_depth) -> the gradients of c_pho pho + c_comb combined + c_flow flow + c_depth depth with respect to the ten
    tensors of SF_RAY_GRADS, in that order (None where `want` is false or the tensor is None).  grads: optional
    preallocated tensors (or None) to write into; every row of them is written."""
    first, R, terms = _sf_ray_inputs("sf_ray_bwd", tensors, terms, late_phase, five_frames)
    _totals_row("sf_ray_bwd", totals, SF_RAY_COLS, first.device)
    out = _grad_buffers("sf_ray_bwd", [tensors[i] for i in SF_RAY_GRADS], want, grads, first.device)
    c = [float(v) for v in coeff]
    _check(lib().zest_sf_ray_bwd(*[_ptr(t) for t in tensors], terms, int(bool(late_phase)), int(bool(five_frames)), R,
                                 _ptr(totals), *c, *[_ptr(g) for g in out], _stream(first)), "zest_sf_ray_bwd")
    return out


PT_MSE, PT_TV, PT_SMOOTH = 1, 2, 4
PT_ALL = PT_MSE | PT_TV | PT_SMOOTH
PATCH_COLS = 9
# launch geometry of csrc/patch_losses.hip (kFwdThreads, kBwdThreads), no part of the C ABI: kept here for the tests,
# which choose their sizes either side of it
PATCH_FWD_THREADS, PATCH_BWD_THREADS = 1024, 256
# the tensors of the patch terms, in the order of the C ABI: name, trailing extent (0: none), the terms that read it,
# whether it takes a gradient
PATCH_TENSORS = (("rgb", 3, PT_MSE | PT_SMOOTH, True), ("target", 3, PT_MSE, False), ("depth", 0, PT_TV | PT_SMOOTH, True))


def _patch_lead(who, terms, first, lead):
    if len(lead) != 3 or min(lead) < 1:
        raise RuntimeError("zest_hip: %s needs [P,H,W(,3)] with P, H, W >= 1, got %s" % (who, tuple(first.shape)))
    if terms & (PT_TV | PT_SMOOTH) and min(lead[1:]) < 2:
        raise RuntimeError("zest_hip: %s: terms 0x%x take neighbour differences, %s leaves a mean over no element"
                           % (who, terms, tuple(first.shape)))


def patch_terms_fwd(rgb, target, depth, terms=PT_ALL, coeff=(1.0, 1.0, 1.0)):
    """Patch terms of the static training step, forward launch.  rgb, target [P,H,W,3], depth [P,H,W], contiguous fp32
    (None where no requested term reads one) -> result [PATCH_COLS]: mse, tv, smooth, the five sums they come from, last
    c_mse mse + c_tv tv + c_smooth smooth for coeff = (c_mse, c_tv, c_smooth) (include/zest_render.h names the columns)."""
    first, (P, H, W), terms = _term_inputs("patch_terms_fwd", (rgb, target, depth), PATCH_TENSORS, terms, PT_ALL, 3, _patch_lead)
    result = torch.empty(PATCH_COLS, device=first.device, dtype=torch.float32)
    _check(lib().zest_patch_terms_fwd(_ptr(rgb), _ptr(target), _ptr(depth), terms, P, H, W, *[float(v) for v in coeff],
                                      _ptr(result), _stream(first)), "zest_patch_terms_fwd")
    return result


def patch_terms_bwd(rgb, target, depth, terms=PT_ALL, coeff=(1.0, 1.0, 1.0), want=(True, True), grads=None):
    """Backward launch -> (d_rgb, d_depth), the gradients of c_mse mse + c_tv tv + c_smooth smooth (None where `want`
    is false or the tensor is None; zeros where no requested term reads the tensor).  grads: optional preallocated
    tensors (or None) to write into; every element of them is written."""
    first, (P, H, W), terms = _term_inputs("patch_terms_bwd", (rgb, target, depth), PATCH_TENSORS, terms, PT_ALL, 3, _patch_lead)
    out = _grad_buffers("patch_terms_bwd", (rgb, depth), want, grads, first.device)
    _check(lib().zest_patch_terms_bwd(_ptr(rgb), _ptr(target), _ptr(depth), terms, P, H, W, *[float(v) for v in coeff],
                                      _ptr(out[0]), _ptr(out[1]), _stream(first)), "zest_patch_terms_bwd")
    return out


# ------------------------------------------------------------------------ GRAF discriminator (csrc/disc.hip)
DISC_MAX_LAYERS = 6


def disc_layout(B, imsize, ndf):
    """Host arithmetic of csrc/disc.hip (no GPU call) -> {saved, work_fwd, work_bwd: floats; layers: [{cin, cout, side,
    u, v, sigma, y, stats: offsets in `saved` (y: None for the last layer, stats: None without a norm)}]}.  Raises for an
    imsize, ndf or batch the kernels do not take."""
    out = (C.c_longlong * (8 + 8 * DISC_MAX_LAYERS))()
    _check(lib().zest_disc_layout(int(B), int(imsize), int(ndf), out), "zest_disc_layout")
    layers = []
    for l in range(out[3]):
        cin, cout, side, u, v, sigma, y, stats = out[8 + 8 * l:16 + 8 * l]
        layers.append(dict(cin=cin, cout=cout, side=side, u=u, v=v, sigma=sigma, y=None if l == out[3] - 1 else y,
                           stats=None if stats < 0 else stats))
    return dict(saved=out[0], work_fwd=out[1], work_bwd=out[2], layers=layers)


def _disc_tables(who, x, imsize, ndf, groups):
    """x [B,imsize,imsize,3] and per-layer tensor lists (name, tensors, shape of layer l) -> (x, layout, pointer tables);
    every tensor is checked against the layer table before its pointer crosses the boundary."""
    x = _dev(x, "x", (None, imsize, imsize, 3))
    lay = disc_layout(x.shape[0], imsize, ndf)
    tables = []
    for name, tensors, shape in groups:
        if tensors is None:
            tables.append(None)
            continue
        if len(tensors) != len(lay["layers"]):
            raise RuntimeError("zest_hip: %s: %d %s tensors for %d layers" % (who, len(tensors), name, len(lay["layers"])))
        for l, (t, L) in enumerate(zip(tensors, lay["layers"])):
            if not t.is_cuda or t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous() \
                    or tuple(t.shape) != shape(L):
                raise RuntimeError("zest_hip: %s: %s[%d] must be a contiguous fp32 tensor %s on %s, got %s %s on %s"
                                   % (who, name, l, shape(L), x.device, t.dtype, tuple(t.shape), t.device))
        tables.append((_vp * len(tensors))(*[_ptr(t) for t in tensors]))
    return x, lay, tables


_DISC_W = lambda L: (L["cout"], L["cin"], 4, 4)         # noqa: E731
_DISC_U = lambda L: (L["cout"],)                          # noqa: E731
_DISC_V = lambda L: (16 * L["cin"],)                      # noqa: E731


def disc_fwd(x, weights, us, vs, imsize, ndf, training):
    """GRAF discriminator forward.  x [B,imsize,imsize,3]; weights, us, vs: per layer weight_orig [cout,cin,4,4],
    weight_u [cout], weight_v [16 cin], contiguous fp32 on x's device; training: one power iteration first, which moves
    us and vs IN PLACE.  -> (logits [B], saved: what disc_bwd of this forward needs, with the u, v and sigma it used)."""
    x, lay, (tw, tu, tv) = _disc_tables("disc_fwd", x, imsize, ndf, (("weights", weights, _DISC_W), ("us", us, _DISC_U),
                                                                     ("vs", vs, _DISC_V)))
    saved = torch.empty(lay["saved"], device=x.device, dtype=torch.float32)
    work = torch.empty(lay["work_fwd"], device=x.device, dtype=torch.float32)
    logits = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    _check(lib().zest_disc_fwd(_ptr(x), x.shape[0], imsize, ndf, tw, tu, tv, int(bool(training)), _ptr(saved), _ptr(work),
                               _ptr(logits), _stream(x)), "zest_disc_fwd")
    return logits, saved


def disc_bwd(x, weights, saved, g_logits, imsize, ndf, want_x=True, want_w=True):
    """Backward of the forward that left `saved` -> (g_x [B,imsize,imsize,3] or None, [d / d weight_orig per layer] or
    None).  want_x false skips the first layer's data gradient, want_w false every weight-gradient launch."""
    if not (want_x or want_w):
        return None, None
    x, lay, (tw,) = _disc_tables("disc_bwd", x, imsize, ndf, (("weights", weights, _DISC_W),))
    saved = _dev(saved, "saved", (lay["saved"],))
    g_logits = _dev(g_logits, "g_logits", (x.shape[0],))
    work = torch.empty(lay["work_bwd"], device=x.device, dtype=torch.float32)
    g_x = torch.empty_like(x) if want_x else None
    g_w = [torch.empty_like(w) for w in weights] if want_w else None
    tg = (_vp * len(g_w))(*[_ptr(t) for t in g_w]) if want_w else None
    _check(lib().zest_disc_bwd(_ptr(x), x.shape[0], imsize, ndf, tw, _ptr(saved), _ptr(g_logits), _ptr(work), _ptr(g_x), tg,
                               _stream(x)), "zest_disc_bwd")
    return g_x, g_w


def disc_saved_views(saved, B, imsize, ndf):
    """The tensors inside `saved` of disc_fwd, per layer: {u, v, sigma, y (raw output [B,side,side,cout]; None for the
    last layer), stats ([B,cout,2] mean and 1/deviation; None without a norm)} - views, for the tests."""
    out = []
    for L in disc_layout(B, imsize, ndf)["layers"]:
        n_y = B * L["side"] * L["side"] * L["cout"]
        out.append(dict(u=saved[L["u"]:L["u"] + L["cout"]], v=saved[L["v"]:L["v"] + 16 * L["cin"]], sigma=saved[L["sigma"]],
                        y=None if L["y"] is None else saved[L["y"]:L["y"] + n_y].view(B, L["side"], L["side"], L["cout"]),
                        stats=None if L["stats"] is None else saved[L["stats"]:L["stats"] + 2 * B * L["cout"]].view(B, L["cout"], 2)))
    return out


# ------------------------------------------------------------------------ LPIPS, AlexNet backbone (csrc/lpips.hip)
LPIPS_LAYERS = 5
LPIPS_MIN_SIDE = 31
# (cin, cout, kernel side) of the five convolutions
LPIPS_CONVS = ((3, 64, 11), (64, 192, 5), (192, 384, 3), (384, 256, 3), (256, 256, 3))


def lpips_layout(N, H, W):
    """Host arithmetic of csrc/lpips.hip (no GPU call) -> {saved, work, packed: floats; shift, scale: offsets in
    `packed`; layers: [{channels, h, w, act: offset of the tap [2N,h,w,channels] in `saved`, K: the packed row length,
    weight, bias, lin: offsets in `packed`}]}.  Raises for H or W < 31 and for N < 1."""
    out = (C.c_longlong * (8 + 8 * LPIPS_LAYERS))()
    _check(lib().zest_lpips_layout(int(N), int(H), int(W), out), "zest_lpips_layout")
    layers = []
    for l in range(out[3]):
        ch, h, w, act, K, weight, bias, lin = out[8 + 8 * l:16 + 8 * l]
        layers.append(dict(channels=ch, h=h, w=w, act=act, K=K, weight=weight, bias=bias, lin=lin))
    return dict(saved=out[0], work=out[1], packed=out[2], shift=out[4], scale=out[5], layers=layers)


def _lpips_table(who, name, tensors, shapes, device):
    if len(tensors) != LPIPS_LAYERS:
        raise RuntimeError("zest_hip: %s: %d %s tensors for %d layers" % (who, len(tensors), name, LPIPS_LAYERS))
    for l, (t, shape) in enumerate(zip(tensors, shapes)):
        if not t.is_cuda or t.device != device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise RuntimeError("zest_hip: %s: %s[%d] must be a contiguous fp32 tensor %s on %s, got %s %s on %s"
                               % (who, name, l, shape, device, t.dtype, tuple(t.shape), t.device))
    return (_vp * LPIPS_LAYERS)(*[_ptr(t) for t in tensors])


def lpips_pack(weights, biases, lins, shift, scale):
    """The five convolution weights [cout,cin,k,k], biases [cout], lin weights [1,cout,1,1], shift and scale [1,3,1,1],
    contiguous fp32 on one device -> the packed weight state lpips_fwd / lpips_bwd read (one launch)."""
    who = "lpips_pack"
    if not torch.is_tensor(shift) or not shift.is_cuda:
        raise RuntimeError("zest_hip: %s: shift is on %s; this path runs only on a HIP device"
                           % (who, shift.device if torch.is_tensor(shift) else type(shift).__name__))
    dev = shift.device
    tw = _lpips_table(who, "weights", weights, [(co, ci, k, k) for ci, co, k in LPIPS_CONVS], dev)
    tb = _lpips_table(who, "biases", biases, [(co,) for _, co, _ in LPIPS_CONVS], dev)
    tl = _lpips_table(who, "lins", lins, [(1, co, 1, 1) for _, co, _ in LPIPS_CONVS], dev)
    shift, scale = _dev(shift, "shift", (1, 3, 1, 1)), _dev(scale, "scale", (1, 3, 1, 1))
    if scale.device != dev:
        raise RuntimeError("zest_hip: %s: scale is on %s, shift on %s" % (who, scale.device, dev))
    packed = torch.empty(lpips_layout(1, 64, 64)["packed"], device=dev, dtype=torch.float32)
    _check(lib().zest_lpips_pack(tw, tb, tl, _ptr(shift), _ptr(scale), _ptr(packed), _stream(shift)), "zest_lpips_pack")
    return packed


def _lpips_image(who, name, t, like=None):
    """An fp32 device tensor [N,3,H,W] of ANY strides (it is read in place) -> (tensor, its strides as a C array)."""
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3:
        raise RuntimeError("zest_hip: %s: %s must be a tensor [N, 3, H, W], got %s"
                           % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("zest_hip: %s is on %s; this path runs only on a HIP device" % (name, t.device))
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise RuntimeError("zest_hip: %s: %s %s on %s does not match in0 %s on %s"
                           % (who, name, tuple(t.shape), t.device, tuple(like.shape), like.device))
    if t.dtype != torch.float32:
        t = t.float()
    return t, (C.c_longlong * 4)(*t.stride())


def lpips_fwd(in0, in1, packed, normalize=False, save=True):
    """LPIPS forward.  in0, in1 [N,3,H,W] fp32 of any strides; packed = lpips_pack(...) -> (result [N,6]: the sum of the
    five layers, then each layer's term; saved: what lpips_bwd of this forward needs, None unless `save`)."""
    in0, s0 = _lpips_image("lpips_fwd", "in0", in0)
    in1, s1 = _lpips_image("lpips_fwd", "in1", in1, in0)
    N, _, H, W = in0.shape
    lay = lpips_layout(N, H, W)
    packed = _dev(packed, "packed", (lay["packed"],))
    saved = torch.empty(lay["saved"], device=in0.device, dtype=torch.float32) if save else None
    work = torch.empty(lay["work"], device=in0.device, dtype=torch.float32)
    result = torch.empty(N, LPIPS_LAYERS + 1, device=in0.device, dtype=torch.float32)
    _check(lib().zest_lpips_fwd(_ptr(in0), s0, _ptr(in1), s1, N, H, W, int(bool(normalize)), _ptr(packed), _ptr(saved),
                                _ptr(work), _ptr(result), _stream(in0)), "zest_lpips_fwd")
    return result, saved


def _dense(shape, stride):
    """Do these strides address every element of a block of prod(shape) elements exactly once?"""
    expect = 1
    for size, st in sorted(((s, t) for s, t in zip(shape, stride) if s > 1), key=lambda p: p[1]):
        if st != expect:
            return False
        expect *= size
    return True


def lpips_bwd(packed, saved, g, shape, stride, normalize=False):
    """Backward of the forward that left `saved`: g [N,6], the upstream gradient of its result; shape, stride: of that
    forward's in0 -> d / d in0, in in0's own layout where that is dense (else contiguous)."""
    N, ch, H, W = (int(s) for s in shape)
    if ch != 3:
        raise RuntimeError("zest_hip: lpips_bwd: shape %s is not [N, 3, H, W]" % (tuple(shape),))
    lay = lpips_layout(N, H, W)
    packed = _dev(packed, "packed", (lay["packed"],))
    saved, g = _dev(saved, "saved", (lay["saved"],)), _dev(g, "g", (N, LPIPS_LAYERS + 1))
    work = torch.empty(lay["work"], device=packed.device, dtype=torch.float32)
    if _dense(shape, stride):
        g_in0 = torch.empty_strided(tuple(shape), tuple(stride), device=packed.device, dtype=torch.float32)
    else:
        g_in0 = torch.empty(tuple(shape), device=packed.device, dtype=torch.float32)
    _check(lib().zest_lpips_bwd(_ptr(packed), _ptr(saved), _ptr(g), N, H, W, int(bool(normalize)), _ptr(work), _ptr(g_in0),
                                (C.c_longlong * 4)(*g_in0.stride()), _stream(packed)), "zest_lpips_bwd")
    return g_in0


def lpips_saved_views(saved, N, H, W):
    """The taps inside `saved` of lpips_fwd: [tensor [2N,h,w,channels] per layer] (post ReLU; in0's images first) -
    views, for the tests."""
    out = []
    for L in lpips_layout(N, H, W)["layers"]:
        n = 2 * N * L["h"] * L["w"] * L["channels"]
        out.append(saved[L["act"]:L["act"] + n].view(2 * N, L["h"], L["w"], L["channels"]))
    return out


# ------------------------------------------------------------------------ image metrics (csrc/image_metrics.hip)
IMG_COLS = 5                      # result columns: mse, psnr, ssim, sum (p - t)^2, sum of the SSIM map
IMG_WINDOWS = (3, 5, 7, 9, 11)
_img_work = {}                    # (device, bytes) -> the partial-sum buffer of image_metrics


def image_metrics_tile():
    """-> (rows, columns) of the tile a workgroup of csrc/image_metrics.hip owns (no GPU call; for the tests, which
    choose their sizes either side of it)."""
    th, tw = _i(), _i()
    _check(lib().zest_image_metrics_tile(C.byref(th), C.byref(tw)), "zest_image_metrics_tile")
    return th.value, tw.value


def _metric_image(who, name, t, like=None):
    """An fp32 tensor [N,C,H,W] of ANY strides (it is read in place) -> (tensor, its strides as a C array)."""
    if not torch.is_tensor(t) or t.dim() != 4 or min(t.shape) < 1:
        raise RuntimeError("zest_hip: %s: %s must be a non-empty tensor [N, C, H, W], got %s"
                           % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if like is not None and t.shape != like.shape:
        raise RuntimeError("zest_hip: %s: %s %s does not match pred %s" % (who, name, tuple(t.shape), tuple(like.shape)))
    if not t.is_cuda:
        raise RuntimeError("zest_hip: %s is on %s; this path runs only on a HIP device" % (name, t.device))
    if like is not None and t.device != like.device:
        raise RuntimeError("zest_hip: %s: %s is on %s, pred on %s" % (who, name, t.device, like.device))
    if t.dtype != torch.float32:
        t = t.float()
    return t, (C.c_longlong * 4)(*t.stride())


def image_metrics(pred, target, window=5, clamp_pred=False, max_val=1.0, want_map=False, want_err=False):
    """MSE, PSNR and SSIM of pred against target, [N,C,H,W] fp32 of any strides (read in place, no copy), in two
    launches -> (result [IMG_COLS]: mse, psnr, ssim over the whole batch and the two raw sums; the SSIM map [N,C,H,W] or
    None; |p - t| [N,C,H,W] or None), p = clamp(pred, 0, 1) if clamp_pred.  window: odd, 3 .. 11, H and W above
    window // 2 (reflect padding).  The buffer of partial sums is kept per (device, size): calls that share it belong on
    one stream."""
    who = "image_metrics"
    pred, ps = _metric_image(who, "pred", pred)
    target, ts = _metric_image(who, "target", target, pred)
    N, Cc, H, W = pred.shape
    window = int(window)
    if window not in IMG_WINDOWS:
        raise RuntimeError("zest_hip: %s: window %d is not an odd size in 3..11" % (who, window))
    if min(H, W) <= window // 2:
        raise RuntimeError("zest_hip: %s: a %d x %d frame does not exceed the reflect padding %d of window %d"
                           % (who, H, W, window // 2, window))
    L, dev = lib(), pred.device
    need = L.zest_image_metrics_work_bytes(N, Cc, H, W)
    if need == 0:
        _check(1, "zest_image_metrics_work_bytes")
    work = _img_work.get((dev, need))
    if work is None:
        work = _img_work[(dev, need)] = torch.empty(need, device=dev, dtype=torch.uint8)
    result = torch.empty(IMG_COLS, device=dev, dtype=torch.float32)
    ssim_map = torch.empty(N, Cc, H, W, device=dev, dtype=torch.float32) if want_map else None
    abs_err = torch.empty(N, Cc, H, W, device=dev, dtype=torch.float32) if want_err else None
    _check(L.zest_image_metrics(_ptr(pred), ps, _ptr(target), ts, N, Cc, H, W, window, int(bool(clamp_pred)), float(max_val),
                                _ptr(result), _ptr(ssim_map), _ptr(abs_err), _ptr(work), need, _stream(pred)),
           "zest_image_metrics")
    return result, ssim_map, abs_err


# ------------------------------------------------------------------------ optimiser (csrc/optim.hip)
ADAM_TENSOR_COLS = 5              # device table row: addresses of p, exp_avg, exp_avg_sq; element count; row of scalars
ADAM_SCALARS = 6                  # step_size, 1 / sqrt(bias_correction2), eps, 1 - b1, b2, 1 - b2
ADAM_RAW_SCALARS = 7              # adam_step_amp: lr, b1, b2, eps, 1 - b1, 1 - b2, the host's count of attempted steps


def adam_chunk():
    """-> elements of one chunk of csrc/optim.hip (no GPU call)."""
    return lib().zest_adam_chunk()


def adam_max_tensors():
    """-> tensors whose gradient addresses one launch's argument block holds (no GPU call); more cost more launches."""
    return lib().zest_adam_max_tensors()


def adam_max_slots():
    """-> rows of per-group, per-t scalars one launch's argument block holds (no GPU call)."""
    return lib().zest_adam_max_slots()


def adam_plan(sizes):
    """The chunk plan of tensors of `sizes` elements (host only, no GPU call) -> ([tensor of chunk k], [offset of chunk
    k in its tensor]); chunk k covers min(adam_chunk(), size - offset) elements."""
    sizes = [int(n) for n in sizes]
    L = lib()
    arr = (C.c_longlong * max(len(sizes), 1))(*sizes)
    n = L.zest_adam_plan(arr, len(sizes), None, None, 0)
    if n < 0:
        _check(1, "zest_adam_plan")
    tens, offs = (_i * max(n, 1))(), (C.c_longlong * max(n, 1))()
    if L.zest_adam_plan(arr, len(sizes), tens, offs, n) != n:
        _check(1, "zest_adam_plan")
    return list(tens[:n]), list(offs[:n])


class AdamTable:
    """What zest_adam_step reads that does not change from step to step: the device tables, the launch bounds, the
    work buffer of the clip; built by adam_table().  What only adam_step_amp needs is made at its first call, so a table
    that never sees one is what it always was: .skipped, the device counter of skipped steps (int32 [2], None before),
    .parity, the element of it the next call reads (the current count is skipped[parity]), the host arrays of the raw
    scalars and of the rows each launch uses."""
    __slots__ = ("device", "n_tensors", "n_chunks", "tensors", "chunk_tensor", "chunk_offset", "n_launches", "launch_tensor",
                 "launch_chunk", "launch_keys", "work", "work_bytes", "scalars", "stamp", "skipped", "parity", "raw", "launch_slots")


def adam_table(params, exp_avgs, exp_avg_sqs, keys):
    """params, exp_avgs, exp_avg_sqs: equally long lists of non-empty contiguous fp32 tensors on one HIP device; keys:
    per tensor a hashable that names its row of scalars (tensors of one parameter group at one step count share one).
    -> AdamTable.  The step is cut into launches of at most adam_max_tensors() tensors and adam_max_slots() distinct keys;
    .launch_keys[l] lists the keys of launch l in the order adam_step wants their scalars."""
    who = "adam_table"
    if not (len(params) == len(exp_avgs) == len(exp_avg_sqs) == len(keys)):
        raise RuntimeError("zest_hip: %s: %d params, %d exp_avg, %d exp_avg_sq, %d keys" % (who, len(params), len(exp_avgs), len(exp_avg_sqs), len(keys)))
    T = AdamTable()
    T.skipped, T.parity, T.raw, T.launch_slots = None, 0, None, None
    T.n_tensors = len(params)
    T.device = params[0].device if params else None
    for name, ts in (("param", params), ("exp_avg", exp_avgs), ("exp_avg_sq", exp_avg_sqs)):
        for i, (t, p) in enumerate(zip(ts, params)):
            if not t.is_cuda:
                raise RuntimeError("zest_hip: %s[%d] is on %s; this path runs only on a HIP device" % (name, i, t.device))
            if t.device != T.device:
                raise RuntimeError("zest_hip: %s: %s[%d] is on %s, param[0] on %s" % (who, name, i, t.device, T.device))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.numel() == 0:
                raise RuntimeError("zest_hip: %s: %s[%d] must be a non-empty contiguous fp32 tensor of %d elements, got %s %s"
                                   % (who, name, i, p.numel(), t.dtype, tuple(t.shape)))
    max_t, max_s = adam_max_tensors(), adam_max_slots()
    chunk_tensor, chunk_offset = adam_plan([p.numel() for p in params])
    T.n_chunks = len(chunk_tensor)
    first_chunk = {}
    for k, t in enumerate(chunk_tensor):
        first_chunk.setdefault(t, k)
    rows, bounds, T.launch_keys = [], [0], []
    for i, (p, m, v, key) in enumerate(zip(params, exp_avgs, exp_avg_sqs, keys)):
        if not T.launch_keys or i - bounds[-1] == max_t or (key not in T.launch_keys[-1] and len(T.launch_keys[-1]) == max_s):
            if T.launch_keys:
                bounds.append(i)
            T.launch_keys.append([])
        if key not in T.launch_keys[-1]:
            T.launch_keys[-1].append(key)
        rows.append([p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), T.launch_keys[-1].index(key)])
    if T.n_tensors:
        bounds.append(T.n_tensors)
    T.n_launches = len(T.launch_keys)
    T.launch_tensor = (_i * (T.n_launches + 1))(*bounds)
    T.launch_chunk = (C.c_longlong * (T.n_launches + 1))(*[first_chunk[b] if b < T.n_tensors else T.n_chunks for b in bounds])
    T.scalars = (_f * (max(T.n_launches, 1) * max_s * ADAM_SCALARS))()
    T.work_bytes = lib().zest_adam_work_bytes(T.n_chunks)
    if T.n_tensors:
        dev = T.device
        T.tensors = torch.tensor(rows, dtype=torch.int64).to(dev)
        T.chunk_tensor = torch.tensor(chunk_tensor, dtype=torch.int32).to(dev)
        T.chunk_offset = torch.tensor(chunk_offset, dtype=torch.int64).to(dev)
        T.work = torch.empty(T.work_bytes, device=dev, dtype=torch.uint8)
    else:
        T.tensors = T.chunk_tensor = T.chunk_offset = T.work = None
    return T


def adam_step(table, grads, scalars, max_norm=None):
    """One Adam step of the tensors of `table` in table.n_launches launches, twice as many with the clip.
    grads: one contiguous fp32 tensor per tensor of the table, of its size, on its device (their addresses travel in the
    launches' argument blocks; they are only read).  scalars: {key: the ADAM_SCALARS floats of that key} for every key of
    table.launch_keys.  max_norm: None, or the global 2-norm the gradients are clipped to while they are applied
    -> None (also for a table without tensors), or the 0-d device tensor of the unclipped norm."""
    who = "adam_step"
    if len(grads) != table.n_tensors:
        raise RuntimeError("zest_hip: %s: %d gradients for a table of %d tensors" % (who, len(grads), table.n_tensors))
    for i, g in enumerate(grads):
        if not g.is_cuda:
            raise RuntimeError("zest_hip: grads[%d] is on %s; this path runs only on a HIP device" % (i, g.device))
    if table.n_tensors == 0:
        return None
    ptrs = (_vp * table.n_tensors)(*[g.data_ptr() for g in grads])
    sc, row = table.scalars, adam_max_slots() * ADAM_SCALARS
    for l, keys in enumerate(table.launch_keys):
        for k, key in enumerate(keys):
            o = l * row + k * ADAM_SCALARS
            sc[o:o + ADAM_SCALARS] = scalars[key]
    dev = table.device
    norm = None if max_norm is None else torch.empty((), device=dev, dtype=torch.float32)
    _check(lib().zest_adam_step(_ptr(table.tensors), _ptr(table.chunk_tensor), _ptr(table.chunk_offset), table.n_launches,
                                table.launch_tensor, table.launch_chunk, ptrs, sc, int(max_norm is not None),
                                0.0 if max_norm is None else float(max_norm), _ptr(table.work), table.work_bytes, _ptr(norm),
                                torch.cuda.current_stream(dev).cuda_stream), "zest_adam_step")
    return norm


def adam_step_amp(table, grads, raw_scalars, max_norm=None, grad_scale=None, found_inf=None, skip_nonfinite=False):
    """adam_step under a GradScaler's protocol, decided on the device (zest_adam_step_amp): no host read.
    raw_scalars: {key: (lr, b1, b2, eps, 1 - b1, 1 - b2, t_host)} for every key of table.launch_keys, t_host the count of
    ATTEMPTED steps including this one; the kernel subtracts the table's skipped steps.  grad_scale, found_inf: None, or a
    one-element fp32 tensor on the table's device: gradients are applied as g / scale; a non-zero found_inf skips the
    step.  skip_nonfinite: skip also when the unscaled norm is not finite (the norm is then taken also with max_norm None).
    A skipped step writes nothing to the tensors.  table.skipped[table.parity] is afterwards the device count of skipped
    steps of this table.
    -> None (a table without tensors; without max_norm and skip_nonfinite), or the 0-d device tensor of the unscaled,
    unclipped norm."""
    who = "adam_step_amp"
    if len(grads) != table.n_tensors:
        raise RuntimeError("zest_hip: %s: %d gradients for a table of %d tensors" % (who, len(grads), table.n_tensors))
    for i, g in enumerate(grads):
        if not g.is_cuda:
            raise RuntimeError("zest_hip: grads[%d] is on %s; this path runs only on a HIP device" % (i, g.device))
    if table.n_tensors == 0:
        return None
    dev = table.device
    for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
        if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == 1 and t.device == dev):
            raise RuntimeError("zest_hip: %s: %s must be a one-element fp32 tensor on %s, got %s" % (
                who, name, dev, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
    max_s = adam_max_slots()
    if table.skipped is None:
        table.skipped = torch.zeros(2, device=dev, dtype=torch.int32)
        table.parity = 0
        table.raw = (C.c_double * (table.n_launches * max_s * ADAM_RAW_SCALARS))()
        table.launch_slots = (_i * table.n_launches)(*[len(keys) for keys in table.launch_keys])
    ptrs = (_vp * table.n_tensors)(*[g.data_ptr() for g in grads])
    raw, row = table.raw, max_s * ADAM_RAW_SCALARS
    for l, keys in enumerate(table.launch_keys):
        for k, key in enumerate(keys):
            o = l * row + k * ADAM_RAW_SCALARS
            raw[o:o + ADAM_RAW_SCALARS] = raw_scalars[key]
    sums = max_norm is not None or bool(skip_nonfinite)
    norm = torch.empty((), device=dev, dtype=torch.float32) if sums else None
    _check(lib().zest_adam_step_amp(_ptr(table.tensors), _ptr(table.chunk_tensor), _ptr(table.chunk_offset), table.n_launches,
                                    table.launch_tensor, table.launch_chunk, table.launch_slots, ptrs, raw,
                                    int(max_norm is not None), 0.0 if max_norm is None else float(max_norm), _ptr(table.work),
                                    table.work_bytes, _ptr(norm), _ptr(grad_scale), _ptr(found_inf), int(bool(skip_nonfinite)),
                                    table.skipped.data_ptr(), table.parity, torch.cuda.current_stream(dev).cuda_stream),
           "zest_adam_step_amp")
    table.parity ^= 1
    return norm


def nchw_to_nhwc(x):
    """[N,C,H,W] -> [N,H,W,C]."""
    x = _dev(x, "x")
    N, Cc, H, W = x.shape
    out = torch.empty(N, H, W, Cc, device=x.device, dtype=torch.float32)
    _check(lib().zest_nchw_to_nhwc(_ptr(x), N, Cc, H, W, _ptr(out), _stream(x)), "zest_nchw_to_nhwc")
    return out


def volume_cost(feats, imgs_lr, proj, depth, pad=0, return_feats_cl=False):
    """Plane-sweep cost volume.  feats [V,32,H,W]; imgs_lr [V,3,H,W] (at feature resolution);
    proj [V-1,3,4]; depth [D] -> img_feat [3V+32, D, H+2pad, W+2pad], in_masks [V, D, Hp, Wp]
    (and, on request, the channels-last feature maps the backward pass gathers from again)."""
    feats, imgs_lr = _dev(feats, "feats"), _dev(imgs_lr, "imgs")
    proj, depth = _dev(proj, "proj_mats"), _dev(depth, "depth_values")
    V, Cc, H, W = feats.shape
    if tuple(imgs_lr.shape) != (V, 3, H, W) or tuple(proj.shape) != (V - 1, 3, 4) or depth.dim() != 1:
        raise RuntimeError("zest_hip.volume_cost: feats %s imgs %s proj %s depth %s"
                           % (tuple(feats.shape), tuple(imgs_lr.shape), tuple(proj.shape), tuple(depth.shape)))
    D, Hp, Wp = depth.shape[0], H + 2 * pad, W + 2 * pad
    fcl, icl = nchw_to_nhwc(feats), images_to_cl(imgs_lr)
    img_feat = torch.empty(3 * V + Cc, D, Hp, Wp, device=feats.device, dtype=torch.float32)
    masks = torch.empty(V, D, Hp, Wp, device=feats.device, dtype=torch.float32)
    _check(lib().zest_volume_cost_fwd(_ptr(fcl), _ptr(icl), _ptr(proj), _ptr(depth), V, Cc, D, H, W, pad,
                                      _ptr(img_feat), _ptr(masks), _stream(feats)), "zest_volume_cost_fwd")
    return (img_feat, masks, fcl) if return_feats_cl else (img_feat, masks)


COST_CL_CHANNELS = 48            # channels of the channels-last cost volume (41 used for V = 3)


def volume_cost_cl(feats, imgs_lr, proj, depth, pad=0, feats_cl=None):
    """The plane-sweep cost volume for the HIP regularisation net: [D, H+2pad, W+2pad, 48] channels-last
    (channels 3V+32 .. 47 are zero), no masks.  Arguments as volume_cost; feats_cl [V,H,W,32]: the features already
    channels-last (FeatureNet.forward_hip) instead of `feats`."""
    imgs_lr = _dev(imgs_lr, "imgs")
    proj, depth = _dev(proj, "proj_mats"), _dev(depth, "depth_values")
    if feats_cl is not None:
        feats_cl = _dev(feats_cl, "feats_cl")
        feats = feats_cl.permute(0, 3, 1, 2)                 # shape bookkeeping only
    else:
        feats = _dev(feats, "feats")
    V, Cc, H, W = feats.shape
    if tuple(imgs_lr.shape) != (V, 3, H, W) or tuple(proj.shape) != (V - 1, 3, 4) or depth.dim() != 1:
        raise RuntimeError("zest_hip.volume_cost_cl: feats %s imgs %s proj %s depth %s"
                           % (tuple(feats.shape), tuple(imgs_lr.shape), tuple(proj.shape), tuple(depth.shape)))
    D, Hp, Wp = depth.shape[0], H + 2 * pad, W + 2 * pad
    fcl, icl = (feats_cl if feats_cl is not None else nchw_to_nhwc(feats)), images_to_cl(imgs_lr)
    out = torch.empty(D, Hp, Wp, COST_CL_CHANNELS, device=feats.device, dtype=torch.float32)
    _check(lib().zest_volume_cost_cl_fwd(_ptr(fcl), _ptr(icl), _ptr(proj), _ptr(depth), V, Cc, D, H, W, pad,
                                         _ptr(out), _stream(feats)), "zest_volume_cost_cl_fwd")
    return out


def costreg_stat_rows():
    return int(lib().zest_costreg_stat_rows())


def costreg_conv_launch_shape(Do, Ho, Wo):
    """-> (rows per wave, tiles, workgroups) of the convolution kernel for an OUTPUT of Do x Ho x Wo voxels (a batch of
    N images: Do = N).  Host arithmetic, the same code the launch runs."""
    rt, tiles, wgs = _i(0), _i(0), _i(0)
    _check(lib().zest_costreg_conv_launch_shape(int(Do), int(Ho), int(Wo), C.byref(rt), C.byref(tiles), C.byref(wgs)),
           "zest_costreg_conv_launch_shape")
    return rt.value, tiles.value, wgs.value


def costreg_deconv_launch_shape(Di, Hi, Wi):
    """-> (tiles, workgroups) of the transposed-convolution kernel for an INPUT of Di x Hi x Wi voxels."""
    tiles, wgs = _i(0), _i(0)
    _check(lib().zest_costreg_deconv_launch_shape(int(Di), int(Hi), int(Wi), C.byref(tiles), C.byref(wgs)),
           "zest_costreg_deconv_launch_shape")
    return tiles.value, wgs.value


def costreg_stats(cout, device):
    """A table of batch statistics for one layer: [rows, 2, cout] float64 (a row per workgroup of the kernel that
    fills it, and a last one with the number of rows in use)."""
    return torch.empty(costreg_stat_rows(), 2, cout, device=device, dtype=torch.float64)


def _strict_operands(who, operands):
    """The operands of a gradient kernel are taken as they are: each (name, tensor, layout[, test]) a contiguous fp32 tensor
    of that layout - a shape with None for any extent, or a text with the test of rank and fixed sizes - refused in the
    order given, before any device is looked at (the C ABI sees pointers and sizes only)."""
    for nm, t, layout, *ok in operands:
        fits = torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and all(f(t) for f in ok)
        if fits and not isinstance(layout, str):
            fits = t.dim() == len(layout) and all(w is None or int(w) == g for w, g in zip(layout, t.shape))
        if not fits:
            raise RuntimeError("%s: %s must be a contiguous fp32 tensor %s, got %s" % (
                who, nm, layout if isinstance(layout, str) else tuple("*" if w is None else int(w) for w in layout),
                "%s %s, contiguous: %s" % (t.dtype, tuple(t.shape), t.is_contiguous()) if torch.is_tensor(t) else type(t).__name__))


def _strict_buffer(who, name, buf, like, size, dtype=torch.float32, aligned=False):
    """A caller's buffer (work, out, g_vol): contiguous, of `dtype` and `size` - an element count or a shape -, 16-byte
    aligned where asked; None: a fresh one beside `like`.  Its device is _strict_devices' business."""
    if buf is None:
        return torch.empty(size, device=like.device, dtype=dtype)
    flat = isinstance(size, int)
    if (not torch.is_tensor(buf) or buf.dtype != dtype or not buf.is_contiguous() or (aligned and buf.data_ptr() % 16)
            or (buf.numel() != size if flat else tuple(buf.shape) != tuple(size))):
        kind = {torch.float32: "fp32"}.get(dtype, str(dtype)[6:])
        raise RuntimeError("%s: %s must be %s%s" % (who, name, "%d contiguous %s elements" % (size, kind) if flat else
                                                    "a contiguous %s tensor %s" % (kind, tuple(size)), ", 16-byte aligned" * aligned))
    return buf


def _strict_devices(who, operands, **buffers):
    """Last of all: every operand and every buffer is on the first operand's device, a HIP device, which is returned."""
    dev = operands[0][1].device
    for nm, t in [o[:2] for o in operands] + list(buffers.items()):
        if not t.is_cuda or t.device != dev:
            raise RuntimeError("%s: %s is on %s; this path runs only on a HIP device (all tensors on one)" % (who, nm, t.device))
    return dev


def _check_stats(stats, cout, who, like):
    if (tuple(stats.shape) != (costreg_stat_rows(), 2, cout) or stats.dtype != torch.float64 or not stats.is_contiguous()
            or stats.device != like.device):
        raise RuntimeError("zest_hip.%s: stats %s %s on %s for %d channels" % (who, tuple(stats.shape), stats.dtype, stats.device, cout))


def _check_packed(w_packed, need, who, what):
    """The packed weights are on the device and exactly as long as the kernel reads them (`what`: the layer, for the text)."""
    have = w_packed.numel() * w_packed.element_size()
    if have != int(need) or not w_packed.is_cuda:
        raise RuntimeError("zest_hip.%s: packed weights of %d bytes, %s take %d" % (who, have, what, need))


def _check_pre(pre, cin, who, like, name="pre"):
    if pre is not None and (tuple(pre.shape) != (2, cin) or pre.dtype != torch.float32 or not pre.is_contiguous()
                            or pre.device != like.device):
        raise RuntimeError("zest_hip.%s: %s %s on %s for %d channels" % (who, name, tuple(pre.shape), pre.device, cin))


def costreg_conv(x, pre, w_packed, cout, stride, passes, stats):
    """x [D,H,W,cin] raw channels-last; pre [2,cin] or None; -> raw [Do,Ho,Wo,cout]; stats: costreg_stats(cout)."""
    x = _dev(x, "x")
    D, H, W, cin = x.shape
    _check_packed(w_packed, lib().zest_costreg_packed_bytes(cin, cout, passes), "costreg_conv",
                  "%d -> %d channels in %d passes" % (cin, cout, passes))
    _check_pre(pre, cin, "costreg_conv", x)
    _check_stats(stats, cout, "costreg_conv", x)
    o = lambda n: (n - 1) // stride + 1
    out = torch.empty(o(D), o(H), o(W), cout, device=x.device, dtype=torch.float32)
    _check(lib().zest_costreg_conv_fwd(_ptr(x), _ptr(pre), _ptr(w_packed), cin, cout, stride, passes, D, H, W,
                                       _ptr(out), _ptr(stats), _stream(x)), "zest_costreg_conv_fwd")
    return out


def conv2d_cl(x, pre, w_packed, cout, k, stride, passes, stats):
    """x [N,H,W,cin] raw channels-last; pre [2,cin] or None; -> raw [N,Ho,Wo,cout] (Conv2d k x k, padding k//2, no bias,
    on act(norm(x))); stats: costreg_stats(cout)."""
    x = _dev(x, "x")
    N, H, W, cin = x.shape
    _check_packed(w_packed, lib().zest_conv2d_packed_bytes(cin, cout, k, passes), "conv2d_cl",
                  "%d -> %d channels, k %d, %d passes" % (cin, cout, k, passes))
    _check_pre(pre, cin, "conv2d_cl", x)
    _check_stats(stats, cout, "conv2d_cl", x)
    o = lambda n: (n - 1) // stride + 1
    out = torch.empty(N, o(H), o(W), cout, device=x.device, dtype=torch.float32)
    _check(lib().zest_conv2d_fwd(_ptr(x), _ptr(pre), _ptr(w_packed), cin, cout, k, stride, passes, N, H, W,
                                 _ptr(out), _ptr(stats), _stream(x)), "zest_conv2d_fwd")
    return out


def costreg_deconv(x0, pre0, x1, pre1, w_packed, cout, passes, stats):
    """act(norm(x0)) [+ act(norm(x1))] [D,H,W,cin] -> raw [2D,2H,2W,cout]; w_packed: CostRegNet._pack_deconv."""
    x0 = _dev(x0, "x0")
    D, H, W, cin = x0.shape
    x1 = _dev(x1, "x1", (D, H, W, cin))
    _check_pre(pre0, cin, "costreg_deconv", x0, "pre0")
    _check_pre(pre1, cin, "costreg_deconv", x0, "pre1")
    _check_packed(w_packed, lib().zest_costreg_deconv_packed_bytes(cin, cout, passes), "costreg_deconv",
                  "%d -> %d channels in %d passes" % (cin, cout, passes))
    _check_stats(stats, cout, "costreg_deconv", x0)
    out = torch.empty(2 * D, 2 * H, 2 * W, cout, device=x0.device, dtype=torch.float32)
    _check(lib().zest_costreg_deconv_fwd(_ptr(x0), _ptr(pre0), _ptr(x1), _ptr(pre1), _ptr(w_packed), cin, cout, passes,
                                         D, H, W, _ptr(out), _ptr(stats), _stream(x0)), "zest_costreg_deconv_fwd")
    return out


def costreg_bn(stats, count, bn, batch_stats, pre, moments=None):
    """pre [2,C] <- scale / shift of the batch norm module `bn` (weight, bias, running_*, eps, momentum) from the
    batch statistics `stats` [2,C] of `count` voxels (and the running estimates updated) or from the running ones."""
    Cn = pre.shape[1]
    if batch_stats:
        _check_stats(stats, Cn, "costreg_bn", pre)
    track = bn.running_mean is not None
    if not batch_stats and not track:
        raise RuntimeError("zest_hip.costreg_bn: a norm without running statistics needs batch statistics")
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    _check(lib().zest_costreg_bn(_ptr(stats), Cn, int(count), _ptr(bn.weight), _ptr(bn.bias), float(bn.eps),
                                 1 if batch_stats else 0, _ptr(bn.running_mean) if track else None,
                                 _ptr(bn.running_var) if track else None, mom,
                                 _ptr(bn.num_batches_tracked) if (track and batch_stats) else None, _ptr(pre),
                                 _ptr(moments), _stream(pre)), "zest_costreg_bn")
    return pre


def costreg_bn_bwd(raw, g_act, pre, moments, gamma):
    """Backward of act(norm(raw)) with batch statistics: raw, g_act [..., C] channels-last -> (g_raw like raw,
    g_gamma [C], g_beta [C])."""
    raw, g_act = _dev(raw, "raw"), _dev(g_act, "g_act", tuple(raw.shape))
    Cn = raw.shape[-1]
    M = raw.numel() // Cn
    ops = [("pre", pre, (2, Cn)), ("moments", moments, (2, Cn))] + ([("gamma", gamma, (Cn,))] if gamma is not None else [])
    _strict_operands("zest_hip.costreg_bn_bwd", ops)
    _strict_devices("zest_hip.costreg_bn_bwd", [("raw", raw)] + ops)
    stats = costreg_stats(Cn, raw.device)
    totals = torch.empty(2, Cn, device=raw.device, dtype=torch.float32)
    g_raw = torch.empty_like(raw)
    _check(lib().zest_costreg_bn_bwd(_ptr(raw), _ptr(g_act), _ptr(pre), _ptr(moments), _ptr(gamma), Cn, M, _ptr(stats),
                                     _ptr(totals), _ptr(g_raw), _stream(raw)), "zest_costreg_bn_bwd")
    return g_raw, totals[1], totals[0]


def costreg_wgrad_launch_shape(D, H, W):
    """-> (units per workgroup, workgroups) of the first layer's weight-gradient kernel on a D x H x W volume (a unit:
    four rows of one slice; workgroup w takes units [w upw, (w + 1) upw)).  Host arithmetic, the same code the launch runs."""
    upw, wgs = _i(0), _i(0)
    _check(lib().zest_costreg_wgrad_launch_shape(int(D), int(H), int(W), C.byref(upw), C.byref(wgs)),
           "zest_costreg_wgrad_launch_shape")
    return upw.value, wgs.value


def costreg_wgrad_work_floats(D, H, W):
    """Size of the partial-sum buffer of costreg_wgrad, in fp32 elements."""
    n = int(lib().zest_costreg_wgrad_work_bytes(int(D), int(H), int(W)))
    if n == 0:
        _check(1, "zest_costreg_wgrad_work_bytes")
    return n // 4


def costreg_wgrad(x_cl, g_cl, cin, work=None, out=None):
    """Weight gradient of CostRegNet.conv0: x_cl [D,H,W,48] (the padded channels-last cost volume of the forward; channels
    from `cin` on are not read into the result), g_cl [D,H,W,8] (costreg_bn_bwd's g_raw) -> g_w [8,cin,3,3,3] fp32.
    bf16-rounded operands, fp32 accumulation, no atomics.  work / out: the caller's buffers (costreg_wgrad_work_floats
    fp32 elements, 16-byte aligned; [8,cin,3,3,3]) instead of fresh ones."""
    who, cin = "zest_hip.costreg_wgrad", int(cin)
    cl = lambda ch: ("[D,H,W,%d]" % ch, lambda t: t.dim() == 4 and t.shape[3] == ch)
    ops = (("x_cl", x_cl) + cl(COST_CL_CHANNELS), ("g_cl", g_cl) + cl(8))
    _strict_operands(who, ops)
    if tuple(g_cl.shape[:3]) != tuple(x_cl.shape[:3]):
        raise RuntimeError("%s: g_cl %s against x_cl %s" % (who, tuple(g_cl.shape), tuple(x_cl.shape)))
    if not 1 <= cin <= COST_CL_CHANNELS:
        raise RuntimeError("%s: cin %d, expected 1 .. %d" % (who, cin, COST_CL_CHANNELS))
    D, H, W, _ = x_cl.shape
    work = _strict_buffer(who, "work", work, x_cl, costreg_wgrad_work_floats(D, H, W), aligned=True)
    out = _strict_buffer(who, "out", out, x_cl, (8, cin, 3, 3, 3))
    _strict_devices(who, ops, work=work, out=out)
    _check(lib().zest_costreg_wgrad(_ptr(x_cl), _ptr(g_cl), D, H, W, cin, 8, _ptr(work), _ptr(out), _stream(x_cl)),
           "zest_costreg_wgrad")
    return out


def costreg_dgrad_launch_shape(D, H, W):
    """-> (tiles, workgroups) of the first layer's data-gradient kernel on a D x H x W volume (a tile: 32 voxels in x by
    two rows of one slice; workgroup w takes tiles [w tpw, (w + 1) tpw), tpw = ceil(tiles / 1024)).  Host arithmetic,
    the same code the launch runs."""
    n_tiles, wgs = _i(0), _i(0)
    _check(lib().zest_costreg_dgrad_launch_shape(int(D), int(H), int(W), C.byref(n_tiles), C.byref(wgs)),
           "zest_costreg_dgrad_launch_shape")
    return n_tiles.value, wgs.value


def costreg_dgrad(g_cl, weight, out=None):
    """Data gradient of CostRegNet.conv0: g_cl [D,H,W,8] (costreg_bn_bwd's g_raw), weight [8,cin,3,3,3] (the module's
    own, cin 1 .. 48) -> g_x [cin,D,H,W] fp32 channel planes.  bf16-rounded operands, fp32 accumulation, every element
    written once, no atomics.  out: the caller's [cin,D,H,W] buffer instead of a fresh one."""
    who = "zest_hip.costreg_dgrad"
    ops = (("g_cl", g_cl, "[D,H,W,8]", lambda t: t.dim() == 4 and t.shape[3] == 8),
           ("weight", weight, "[8,cin,3,3,3]", lambda t: t.dim() == 5 and t.shape[0] == 8 and tuple(t.shape[2:]) == (3, 3, 3)))
    _strict_operands(who, ops)
    (D, H, W, _), cin = g_cl.shape, int(weight.shape[1])
    if not 1 <= cin <= COST_CL_CHANNELS:
        raise RuntimeError("%s: cin %d, expected 1 .. %d" % (who, cin, COST_CL_CHANNELS))
    out = _strict_buffer(who, "out", out, g_cl, (cin, D, H, W))
    _strict_devices(who, ops, out=out)
    _check(lib().zest_costreg_dgrad(_ptr(g_cl), _ptr(weight), D, H, W, cin, 8, _ptr(out), _stream(g_cl)),
           "zest_costreg_dgrad")
    return out


# ------------------------------------------------------------------ gradients of the feature pyramid (csrc/feature_grad.hip)
def _conv_out(n, stride):
    return (n - 1) // stride + 1


def feature_wgrad_launch_shape(N, Hi, Wi, cin, cout, k, stride):
    """-> (units, units per workgroup, workgroups, fp32 elements of the partial-sum buffer) of feature_wgrad (a unit: 32
    output pixels of one row; workgroup w takes units [w upw, (w + 1) upw)).  Host arithmetic, the code the launch runs."""
    units, upw, wgs, nbytes = _i(0), _i(0), _i(0), _sz(0)
    _check(lib().zest_feature_wgrad_launch_shape(int(N), int(Hi), int(Wi), int(cin), int(cout), int(k), int(stride), C.byref(units),
                                                 C.byref(upw), C.byref(wgs), C.byref(nbytes)), "zest_feature_wgrad_launch_shape")
    return units.value, upw.value, wgs.value, nbytes.value // 4


def feature_wgrad(x, pre, g, k, stride, cin):
    """Weight gradient of one Conv2d of the feature pyramid (k x k, padding k // 2, no bias; (k, stride) = (3, 1) or
    (5, 2)) -> g_w [cout,cin,k,k] fp32.  g [N,Ho,Wo,cout]: costreg_bn_bwd's channels-last result.  With pre [2,cin]: x
    [N,Hi,Wi,cin] is the previous layer's raw channels-last output and the kernel forms leaky_relu(x pre[0] + pre[1])
    itself; with pre None: x [N,cin,Hi,Wi] is the layer's input as it is (the image, channel planes).  bf16-rounded
    operands, fp32 accumulation, fp32 result, no atomics: the same bits on every call."""
    who, cin, k, stride = "zest_hip.feature_wgrad", int(cin), int(k), int(stride)
    if stride < 1:
        raise RuntimeError("%s: stride %d" % (who, stride))
    if pre is None:
        ops = [("x", x, "[N,%d,Hi,Wi] (pre is None: the layer's own input)" % cin, lambda t: t.dim() == 4 and t.shape[1] == cin)]
        _strict_operands(who, ops)
        N, _, Hi, Wi = x.shape
        strides = (cin * Hi * Wi, Wi, 1, Hi * Wi)
    else:
        ops = [("x", x, "[N,Hi,Wi,%d]" % cin, lambda t: t.dim() == 4 and t.shape[3] == cin),
               ("pre", pre, "[2,%d]" % cin, lambda t: tuple(t.shape) == (2, cin))]
        _strict_operands(who, ops)
        N, Hi, Wi, _ = x.shape
        strides = (Hi * Wi * cin, Wi * cin, cin, 1)
    Ho, Wo = _conv_out(Hi, stride), _conv_out(Wi, stride)
    ops.append(("g", g, "[%d,%d,%d,cout]" % (N, Ho, Wo), lambda t: t.dim() == 4 and tuple(t.shape[:3]) == (N, Ho, Wo)))
    _strict_operands(who, ops[-1:])
    cout = int(g.shape[3])
    need = feature_wgrad_launch_shape(N, Hi, Wi, cin, cout, k, stride)[3]      # refuses a layer shape without a kernel
    dev = _strict_devices(who, ops)
    work = torch.empty(need, device=dev, dtype=torch.float32)
    out = torch.empty(cout, cin, k, k, device=dev, dtype=torch.float32)
    _check(lib().zest_feature_wgrad(_ptr(x), *strides, _ptr(pre), _ptr(g), N, Hi, Wi, cin, cout, k, stride, _ptr(work), _ptr(out),
                                    _stream(g)), "zest_feature_wgrad")
    return out


def feature_dgrad_launch_shape(N, Hi, Wi, cin, cout, k, stride):
    """-> (tiles, workgroups, bytes of the packed weight) of feature_dgrad (a tile: 32 positions of one row of g with all
    stride x stride parity classes of input pixels over it; wave v of workgroup w takes tiles 4 w + v + 4 workgroups i).
    Host arithmetic, the code the launch runs."""
    tiles, wgs, nbytes = _i(0), _i(0), _sz(0)
    _check(lib().zest_feature_dgrad_launch_shape(int(N), int(Hi), int(Wi), int(cin), int(cout), int(k), int(stride), C.byref(tiles),
                                                 C.byref(wgs), C.byref(nbytes)), "zest_feature_dgrad_launch_shape")
    return tiles.value, wgs.value, nbytes.value


def feature_dgrad(g, w, stride, in_hw):
    """Data gradient of one Conv2d of the feature pyramid: g [N,Ho,Wo,cout] (costreg_bn_bwd's channels-last result), w the
    module's [cout,cin,k,k] fp32 weight, in_hw = (Hi, Wi) the extents of the layer's input -> g_x [N,Hi,Wi,cin]
    channels-last fp32, what the next costreg_bn_bwd reads.  A gather per parity class of the input pixel: every element
    written once, bf16-rounded operands, fp32 accumulation, fp32 result, no atomics."""
    who, stride = "zest_hip.feature_dgrad", int(stride)
    Hi, Wi = (int(v) for v in in_hw)
    if stride < 1 or Hi < 1 or Wi < 1:
        raise RuntimeError("%s: stride %d, input extents %d x %d" % (who, stride, Hi, Wi))
    Ho, Wo = _conv_out(Hi, stride), _conv_out(Wi, stride)
    ops = [("g", g, "[N,%d,%d,cout]" % (Ho, Wo), lambda t: t.dim() == 4 and tuple(t.shape[1:3]) == (Ho, Wo))]
    _strict_operands(who, ops)
    N, cout = int(g.shape[0]), int(g.shape[3])
    ops.append(("w", w, "[%d,cin,k,k]" % cout, lambda t: t.dim() == 4 and t.shape[0] == cout and t.shape[2] == t.shape[3]))
    _strict_operands(who, ops[-1:])
    cin, k = int(w.shape[1]), int(w.shape[2])
    nbytes = feature_dgrad_launch_shape(N, Hi, Wi, cin, cout, k, stride)[2]    # refuses a layer shape without a kernel
    dev = _strict_devices(who, ops)
    wpack = torch.empty(nbytes // 2, device=dev, dtype=torch.int16)
    out = torch.empty(N, Hi, Wi, cin, device=dev, dtype=torch.float32)
    _check(lib().zest_feature_dgrad(_ptr(g), _ptr(w), N, Hi, Wi, cin, cout, k, stride, _ptr(wpack), _ptr(out), _stream(g)),
           "zest_feature_dgrad")
    return out


def feature_top_bwd_launch_shape(N, h, w):
    """-> (chunks of 64 pixels, workgroups, fp32 elements of the partial-sum buffer) of feature_top_bwd (chunk c goes to
    workgroup c mod workgroups).  Host arithmetic, the code the launch runs."""
    chunks, wgs, nbytes = _i(0), _i(0), _sz(0)
    _check(lib().zest_feature_top_bwd_launch_shape(int(N), int(h), int(w), C.byref(chunks), C.byref(wgs), C.byref(nbytes)),
           "zest_feature_top_bwd_launch_shape")
    return chunks.value, wgs.value, nbytes.value // 4


def feature_top_bwd(g_feats, raw, pre, top_w):
    """Backward of the pyramid's 1 x 1 top layer (32 -> 32 with bias), fp32 throughout: g_feats [N,32,h,w], raw [N,h,w,32]
    and pre [2,32] of the last 3 x 3 layer, top_w [32,32,1,1] -> (g_act [N,h,w,32] channels-last, g_top_w like top_w,
    g_top_b [32]).  The two sums over pixels are added in a fixed order: the same bits on every call."""
    who = "zest_hip.feature_top_bwd"
    ops = [("g_feats", g_feats, "[N,32,h,w]", lambda t: t.dim() == 4 and t.shape[1] == 32)]
    _strict_operands(who, ops)
    N, _, h, w = g_feats.shape
    ops += [("raw", raw, "[%d,%d,%d,32]" % (N, h, w), lambda t: tuple(t.shape) == (N, h, w, 32)),
            ("pre", pre, "[2,32]", lambda t: tuple(t.shape) == (2, 32)),
            ("top_w", top_w, "[32,32,1,1]", lambda t: tuple(t.shape) in ((32, 32, 1, 1), (32, 32)))]
    _strict_operands(who, ops[1:])
    dev = _strict_devices(who, ops)
    work = torch.empty(feature_top_bwd_launch_shape(N, h, w)[2], device=dev, dtype=torch.float32)
    g_act = torch.empty(N, h, w, 32, device=dev, dtype=torch.float32)
    g_w, g_b = torch.empty_like(top_w), torch.empty(32, device=dev, dtype=torch.float32)
    _check(lib().zest_feature_top_bwd(_ptr(g_feats), _ptr(raw), _ptr(pre), _ptr(top_w), N, h, w, _ptr(work), _ptr(g_act), _ptr(g_w),
                                      _ptr(g_b), _stream(g_feats)), "zest_feature_top_bwd")
    return g_act, g_w, g_b


def costreg_out(raw_a, pre_a, raw_b, pre_b):
    """act(norm(raw_a)) + act(norm(raw_b)), [D,H,W,8] each -> the encoding volume [1,8,D,H,W]."""
    raw_a = _dev(raw_a, "raw_a")
    D, H, W, Cn = raw_a.shape
    raw_b = _dev(raw_b, "raw_b", (D, H, W, 8))
    if Cn != 8:
        raise RuntimeError("zest_hip.costreg_out: raw_a %s, expected 8 channels" % (tuple(raw_a.shape),))
    ops = [("pre_a", pre_a, (2, 8)), ("pre_b", pre_b, (2, 8))]
    _strict_operands("zest_hip.costreg_out", ops)
    _strict_devices("zest_hip.costreg_out", [("raw_a", raw_a)] + ops)
    out = torch.empty(1, 8, D, H, W, device=raw_a.device, dtype=torch.float32)
    _check(lib().zest_costreg_out(_ptr(raw_a), _ptr(pre_a), _ptr(raw_b), _ptr(pre_b), D, H, W, _ptr(out),
                                  _stream(raw_a)), "zest_costreg_out")
    return out


# ---- the order-independent forms of the scatter-add gradients (deterministic=True; include/zest_render.h, *_det) ----
DET_MAX_CONTRIBUTIONS = 1 << 32


def _det_checked(who, operands, work, nbytes, n_contrib, what):
    """Operands - (name, tensor, shape with None for any extent) -, the number of contributions and the workspace of a *_det
    call, every refusal before the device is looked at.  -> the workspace (the caller's, or a fresh one)."""
    _strict_operands(who, operands)
    if nbytes == 0:
        _check(1, who)
    if n_contrib > DET_MAX_CONTRIBUTIONS:
        raise RuntimeError("%s: %d contributions (%s) exceed 2^32" % (who, n_contrib, what))
    work = _strict_buffer(who, "work", work, operands[0][1], nbytes, torch.uint8, aligned=True)
    _strict_devices(who, operands, work=work)
    return work


def volume_cost_bwd(feats_cl, proj, depth, pad, g_img_feat, deterministic=False, work=None):
    """g_img_feat [3V+32, D, Hp, Wp] -> gradient of the feature maps [V,32,H,W] (a channels-first view of
    the channels-last buffer the kernel scatters into).  deterministic: the order-independent form
    (zest_volume_cost_bwd_det; contiguous fp32 operands; work: zest_volume_cost_bwd_det_work_bytes(V, H, W) uint8
    elements to reuse, 16-byte aligned)."""
    if deterministic:
        who = "zest_hip.volume_cost_bwd(deterministic)"
        V, H, W, Cc = feats_cl.shape if torch.is_tensor(feats_cl) and feats_cl.dim() == 4 else (0, 0, 0, 0)
        D, pad = (int(depth.shape[0]) if torch.is_tensor(depth) and depth.dim() == 1 else 0), int(pad)
        ops = (("feats_cl", feats_cl, (None, None, None, 32)), ("g_img_feat", g_img_feat, (3 * V + Cc, D, H + 2 * pad, W + 2 * pad)),
               ("proj_mats", proj, (V - 1, 3, 4)), ("depth_values", depth, (None,)))
        work = _det_checked(who, ops, work, int(lib().zest_volume_cost_bwd_det_work_bytes(V, H, W)),
                            D * (H + 2 * pad) * (W + 2 * pad) * V * 4, "voxels x views x 4 taps")
        g = torch.empty_like(feats_cl)
        _check(lib().zest_volume_cost_bwd_det(_ptr(feats_cl), _ptr(proj), _ptr(depth), V, Cc, D, H, W, pad, _ptr(g_img_feat),
                                              _ptr(g), _ptr(work), _stream(feats_cl)), "zest_volume_cost_bwd_det")
        return g.permute(0, 3, 1, 2)
    g_img_feat, proj, depth = _dev(g_img_feat, "g_img_feat"), _dev(proj, "proj_mats"), _dev(depth, "depth_values")
    V, H, W, Cc = feats_cl.shape
    D = depth.shape[0]
    if tuple(g_img_feat.shape) != (3 * V + Cc, D, H + 2 * pad, W + 2 * pad):
        raise RuntimeError("zest_hip.volume_cost_bwd: gradient %s for V=%d D=%d H=%d W=%d pad=%d"
                           % (tuple(g_img_feat.shape), V, D, H, W, pad))
    g = torch.zeros_like(feats_cl)
    _check(lib().zest_volume_cost_bwd(_ptr(feats_cl), _ptr(proj), _ptr(depth), V, Cc, D, H, W, pad, _ptr(g_img_feat),
                                      _ptr(g), _stream(feats_cl)), "zest_volume_cost_bwd")
    return g.permute(0, 3, 1, 2)


def homo_warp_bwd(g_warped, src_shape, proj=None, depth=None, grid=None, pad=0, deterministic=False, work=None):
    """g_warped [C,D,Hp,Wp] -> g_src [C,H,W]; grid [D,Hp,Wp,2] or proj [3,4] + depth [D] as in homo_warp.
    deterministic: the order-independent form (zest_homo_warp_bwd_det; contiguous fp32 operands; work:
    zest_homo_warp_bwd_det_work_bytes(C, H, W) uint8 elements to reuse, 16-byte aligned)."""
    if deterministic:
        who = "zest_hip.homo_warp_bwd(deterministic)"
        Cc, H, W = (int(v) for v in src_shape)
        D, Hp, Wp = g_warped.shape[1:] if torch.is_tensor(g_warped) and g_warped.dim() == 4 else (0, 0, 0)
        ops = (("g_warped", g_warped, (Cc, None, None, None)),)
        ops += (("src_grid", grid, (D, Hp, Wp, 2)),) if grid is not None else (("proj_mat", proj, (3, 4)), ("depth_values", depth, (D,)))
        work = _det_checked(who, ops, work, int(lib().zest_homo_warp_bwd_det_work_bytes(Cc, H, W)), D * Hp * Wp * 4,
                            "voxels x 4 taps")
        g = torch.empty(Cc, H, W, device=g_warped.device, dtype=torch.float32)
        proj, depth = (None, None) if grid is not None else (proj, depth)
        _check(lib().zest_homo_warp_bwd_det(_ptr(proj), _ptr(depth), _ptr(grid), Cc, D, H, W, Hp, Wp, int(pad), _ptr(g_warped),
                                            _ptr(g), _ptr(work), _stream(g_warped)), "zest_homo_warp_bwd_det")
        return g
    g_warped = _dev(g_warped, "g_warped")
    Cc, H, W = src_shape
    D, Hp, Wp = g_warped.shape[1:]
    g = torch.zeros(Cc, H, W, device=g_warped.device, dtype=torch.float32)
    gin = _dev(grid, "src_grid") if grid is not None else None
    proj, depth = (None, None) if gin is not None else (_dev(proj, "proj_mat"), _dev(depth, "depth_values"))
    _check(lib().zest_homo_warp_bwd(_ptr(proj), _ptr(depth), _ptr(gin), Cc, D, H, W, Hp, Wp, pad, _ptr(g_warped),
                                    _ptr(g), _stream(g_warped)), "zest_homo_warp_bwd")
    return g


def homo_warp(src, proj=None, depth=None, grid=None, pad=0):
    """src [C,H,W]; proj [3,4] + depth [D], or grid [D,Hp,Wp,2] -> warped [C,D,Hp,Wp], grid."""
    src = _dev(src, "src_feat")
    Cc, H, W = src.shape
    if grid is None:
        proj, depth = _dev(proj, "proj_mat"), _dev(depth, "depth_values")
        D, Hp, Wp = depth.shape[0], H + 2 * pad, W + 2 * pad
        grid_out = torch.empty(D, Hp, Wp, 2, device=src.device, dtype=torch.float32)
        gin = None
    else:
        gin = _dev(grid, "src_grid")
        D, Hp, Wp = gin.shape[:3]
        grid_out = gin
    warped = torch.empty(Cc, D, Hp, Wp, device=src.device, dtype=torch.float32)
    _check(lib().zest_homo_warp_fwd(_ptr(src), _ptr(proj) if gin is None else None,
                                    _ptr(depth) if gin is None else None, _ptr(gin) if gin is not None else None,
                                    Cc, D, H, W, Hp, Wp, pad, _ptr(warped),
                                    _ptr(grid_out) if gin is None else None, _stream(src)), "zest_homo_warp_fwd")
    return warped, grid_out


def images_to_cl(imgs):
    """[1,V,3,H,W] or [V,3,H,W] -> [V,H,W,4]."""
    imgs = _dev(imgs, "imgs")
    if imgs.dim() == 5:
        if imgs.shape[0] != 1:
            raise RuntimeError("zest_hip: image batch must be 1, got %d" % imgs.shape[0])
        imgs = imgs[0]
    V, c, H, W = imgs.shape
    if c != 3:
        raise RuntimeError("zest_hip: images must have 3 channels, got %d" % c)
    out = torch.empty(V, H, W, 4, device=imgs.device, dtype=torch.float32)
    _check(lib().zest_images_to_cl(_ptr(imgs), V, H, W, _ptr(out), _stream(imgs)), "zest_images_to_cl")
    return out


def volume_lookup(vol_cl, ndc):
    ndc = _dev(ndc, "ndc", (None,) * (ndc.dim() - 1) + (3,))
    vol_cl = _dev(vol_cl, "vol_cl", (None, None, None, 8))
    H, W, D, _ = vol_cl.shape
    M = ndc.numel() // 3
    out = torch.empty(*ndc.shape[:-1], 8, device=ndc.device, dtype=torch.float32)
    _check(lib().zest_volume_lookup_fwd(_ptr(vol_cl), D, H, W, _ptr(ndc), M, _ptr(out), _stream(ndc)),
           "zest_volume_lookup_fwd")
    return out


def color_lookup(imgs_cl, w2cs, intrinsics, pts):
    pts = _dev(pts, "pts", (None,) * (pts.dim() - 1) + (3,))
    imgs_cl = _dev(imgs_cl, "imgs_cl", (None, None, None, 4))
    w2cs = _dev(w2cs, "w2cs", (None,) * (w2cs.dim() - 2) + (4, 4))
    intrinsics = _dev(intrinsics, "intrinsics", (None,) * (intrinsics.dim() - 2) + (3, 3))
    V, H, W, _ = imgs_cl.shape
    if w2cs.numel() < 16 * V or intrinsics.numel() < 9 * V:
        raise RuntimeError("zest_hip: %d views but only %d poses" % (V, w2cs.shape[-3]))
    M = pts.numel() // 3
    out = torch.empty(*pts.shape[:-1], 4 * V, device=pts.device, dtype=torch.float32)
    _check(lib().zest_color_lookup_fwd(_ptr(imgs_cl), V, H, W, _ptr(w2cs), _ptr(intrinsics), _ptr(pts),
                                       M, _ptr(out), _stream(pts)), "zest_color_lookup_fwd")
    return out


def encode(ndc, pts, rays_dir, t=None, vol_cl=None, imgs_cl=None, w2cs=None, intrinsics=None, out=None):
    """ndc, pts [R,S,3]; rays_dir [R,3] -> x [R,S,C_in] (reference prepare_pts layout); out: a contiguous
    [R,S,C_in] fp32 tensor to write into (e.g. half of a larger batch) instead of a new one."""
    ndc = _dev(ndc, "ndc", (None, None, 3))
    R, S, _ = ndc.shape
    pts, rays_dir = _dev(pts, "pts", (R, S, 3)), _dev(rays_dir, "rays_dir", (R, 3))
    w2cs, intrinsics = _dev(w2cs, "w2cs"), _dev(intrinsics, "intrinsics")
    has_t = t is not None
    D = Hv = Wv = V = H = W = 0
    if vol_cl is not None:
        vol_cl, imgs_cl = _dev(vol_cl, "vol_cl", (None, None, None, 8)), _dev(imgs_cl, "imgs_cl", (None, None, None, 4))
        Hv, Wv, D, _ = vol_cl.shape
        V, H, W, _ = imgs_cl.shape
        if pts is None or w2cs is None or intrinsics is None or w2cs.numel() < 16 * V or intrinsics.numel() < 9 * V:
            raise RuntimeError("zest_hip: encode with features needs pts and one pose (4x4) and intrinsic (3x3) per source view")
    if w2cs is not None and w2cs.shape[-2:] != (4, 4):
        raise RuntimeError("zest_hip: w2cs has shape %s, expected (..., 4, 4)" % (tuple(w2cs.shape),))
    c_in = (4 if has_t else 3) * 21 + (8 + 4 * V if vol_cl is not None else 0) + 27
    x = torch.empty(R, S, c_in, device=ndc.device, dtype=torch.float32) if out is None else _dev(out, "out", (R, S, c_in))
    _check(lib().zest_encode_fwd(_ptr(ndc), _ptr(pts), _ptr(rays_dir), R, S, int(has_t),
                                 float(t) if has_t else 0.0, _ptr(vol_cl), D, Hv, Wv, _ptr(imgs_cl),
                                 V, H, W, _ptr(w2cs), _ptr(intrinsics), _ptr(x), _stream(ndc)),
           "zest_encode_fwd")
    return x


# ----------------------------------------------------------------------------- ray sampling
def build_rays(xs, ys, t_rand, S, k_tgt, c2w_tgt, w2c_ref, k_ref, nf_tgt, nf_ref, pad, W, H):
    """xs, ys [R] pixel coordinates; camera matrices and (near, far) pairs as device tensors
    (views into the batch dict) -> rays_dir [R,3], depth [R,S], pts, ndc [R,S,3]."""
    xs = _dev(xs, "xs")
    R = xs.numel()
    ys, t_rand = _dev(ys, "ys", xs.shape), _dev(t_rand, "t_rand")
    if t_rand is not None and (t_rand.dim() != 2 or t_rand.shape[0] < R or t_rand.shape[1] != S):
        raise RuntimeError("zest_hip: t_rand has shape %s, expected (>= %d, %d)" % (tuple(t_rand.shape), R, S))
    mats = [_dev(m, n, sh) for m, n, sh in ((k_tgt, "k_tgt", (3, 3)), (c2w_tgt, "c2w_tgt", (4, 4)), (w2c_ref, "w2c_ref", (4, 4)),
                                           (k_ref, "k_ref", (3, 3)), (nf_tgt, "near_far_tgt", (2,)), (nf_ref, "near_far_ref", (2,)))]
    o = lambda *s: torch.empty(*s, device=xs.device, dtype=torch.float32)
    d, z, pts, ndc = o(R, 3), o(R, S), o(R, S, 3), o(R, S, 3)
    _check(lib().zest_build_rays_fwd(_ptr(xs), _ptr(ys), _ptr(t_rand), R, int(S), *[_ptr(m) for m in mats],
                                     int(pad), int(W), int(H), _ptr(d), _ptr(z), _ptr(pts), _ptr(ndc),
                                     _stream(xs)), "zest_build_rays_fwd")
    return d, z, pts, ndc


def sample_pdf(bins, weights, n_samples=None, u=None):
    """bins [R, Nb+1], weights [R, Nb], u [R, Ns] (or None + n_samples: deterministic) -> samples [R, Ns]."""
    weights = _dev(weights, "weights", (None, None))
    R, Nb = weights.shape
    bins, u = _dev(bins, "bins", (R, Nb + 1)), _dev(u, "u", (R, None))
    Ns = u.shape[1] if u is not None else int(n_samples)
    out = torch.empty(R, Ns, device=bins.device, dtype=torch.float32)
    _check(lib().zest_sample_pdf_fwd(_ptr(bins), _ptr(weights), _ptr(u), R, Nb, Ns, _ptr(out), _stream(bins)),
           "zest_sample_pdf_fwd")
    return out


def ndc_coordinate(pts, w2c, k, inv_w, inv_h, near, far, pad=0, lindisp=False):
    pts = _dev(pts, "pts", (None,) * (pts.dim() - 1) + (3,))
    w2c, k = _dev(w2c, "w2c", (4, 4)), _dev(k, "k", (3, 3))
    M = pts.numel() // 3
    out = torch.empty_like(pts)
    _check(lib().zest_ndc_fwd(_ptr(pts), M, _ptr(w2c), _ptr(k), float(inv_w), float(inv_h), float(near),
                              float(far), int(pad), int(bool(lindisp)), _ptr(out), _stream(pts)),
           "zest_ndc_fwd")
    return out


def composite_bwd(raw, z, rays_dir, noise, noise_std, white_bkgd, g_rgb, g_depth, g_acc, g_weights, dists=None):
    z = _dev(z, "z")
    rays_dir, dists = _spacing(z, rays_dir, dists)
    R, S = z.shape
    raw, noise = _dev(raw, "raw", (R, S, 4)), _dev(noise, "noise", (R, S))
    gs = [_dev(g, n, sh) for g, n, sh in ((g_rgb, "g_rgb", (R, 3)), (g_depth, "g_depth", (R,)), (g_acc, "g_acc", (R,)),
                                          (g_weights, "g_weights", (R, S)))]
    g_raw = torch.empty(R, S, 4, device=z.device, dtype=torch.float32)
    _check(lib().zest_composite_bwd(_ptr(raw), _ptr(z), _ptr(rays_dir), _ptr(dists), _ptr(noise), float(noise_std),
                                    int(bool(white_bkgd)), R, S, *[_ptr(g) for g in gs], _ptr(g_raw),
                                    _stream(z)), "zest_composite_bwd")
    return g_raw


def composite_blend_bwd(raw_dy, raw_st, blend, z, rays_dir, noise, noise_std, g_rgb, g_depth, g_rgb_fg,
                        g_depth_fg, g_wfg, g_wd, dists=None):
    z = _dev(z, "z")
    rays_dir, dists = _spacing(z, rays_dir, dists)
    R, S = z.shape
    raw_dy, raw_st = _dev(raw_dy, "raw_dy", (R, S, 4)), _dev(raw_st, "raw_st", (R, S, 4))
    blend, noise = _dev(blend, "blend", (R, S)), _dev(noise, "noise", (R, S))
    gs = [_dev(g, n, sh) for g, n, sh in ((g_rgb, "g_rgb", (R, 3)), (g_depth, "g_depth", (R,)), (g_rgb_fg, "g_rgb_fg", (R, 3)),
                                          (g_depth_fg, "g_depth_fg", (R,)), (g_wfg, "g_weights_fg", (R, S)),
                                          (g_wd, "g_weights_dy", (R, S)))]
    o = lambda *s: torch.empty(*s, device=z.device, dtype=torch.float32)
    g_dy, g_st, g_b = o(R, S, 4), o(R, S, 4), o(R, S)
    _check(lib().zest_composite_blend_bwd(_ptr(raw_dy), _ptr(raw_st), _ptr(blend), _ptr(z), _ptr(rays_dir),
                                          _ptr(dists), _ptr(noise), float(noise_std), R, S, *[_ptr(g) for g in gs],
                                          _ptr(g_dy), _ptr(g_st), _ptr(g_b), _stream(z)),
           "zest_composite_blend_bwd")
    return g_dy, g_st, g_b


# ------------------------------------------------------------------- training path (backward)
def encode_bwd(g_x, ndc, t, vol_cl, V, want_vol_grad, g_vol=None, deterministic=False, work=None):
    """-> g_ndc [R,S,3], g_vol_cl [H,W,D,8] or None.  g_vol: an existing volume gradient to add into (the kernel
    scatter-adds) instead of a fresh zero-filled one.  deterministic: the volume gradient through the order-independent
    form (zest_encode_bwd_det; contiguous fp32 operands; work: zest_encode_bwd_det_work_bytes(D, Hv, Wv) uint8 elements
    to reuse, 16-byte aligned); a g_vol given is then added to with one elementwise launch.  Without a volume gradient
    nothing is added up and the mode changes nothing."""
    if deterministic and vol_cl is not None and want_vol_grad:
        who = "zest_hip.encode_bwd(deterministic)"
        R, S = ndc.shape[:2] if torch.is_tensor(ndc) and ndc.dim() == 3 else (0, 0)
        Hv, Wv, D = vol_cl.shape[:3] if torch.is_tensor(vol_cl) and vol_cl.dim() == 4 else (0, 0, 0)
        c_in = (4 if t is not None else 3) * 21 + 8 + 4 * int(V) + 27
        ops = (("ndc", ndc, (None, None, 3)), ("g_x", g_x, (R, S, c_in)), ("vol_cl", vol_cl, (None, None, None, 8)))
        ops += (("g_vol", g_vol, (Hv, Wv, D, 8)),) if g_vol is not None else ()
        work = _det_checked(who, ops, work, int(lib().zest_encode_bwd_det_work_bytes(D, Hv, Wv)), R * S * 8, "R S 8")
        g_ndc, g_new = torch.empty_like(ndc), torch.empty_like(vol_cl)
        _check(lib().zest_encode_bwd_det(_ptr(g_x), _ptr(ndc), R, S, int(t is not None), float(t) if t is not None else 0.0,
                                         _ptr(vol_cl), D, Hv, Wv, int(V), _ptr(g_ndc), _ptr(g_new), _ptr(work), _stream(ndc)),
               "zest_encode_bwd_det")
        return g_ndc, (g_new if g_vol is None else g_vol.add_(g_new))
    ndc = _dev(ndc, "ndc", (None, None, 3))
    R, S, _ = ndc.shape
    c_in = (4 if t is not None else 3) * 21 + (8 + 4 * int(V) if vol_cl is not None else 0) + 27
    g_x = _dev(g_x, "g_x", (R, S, c_in))
    D = Hv = Wv = 0
    add_to, g_vol = g_vol, None
    if vol_cl is not None:
        vol_cl = _dev(vol_cl, "vol_cl", (None, None, None, 8))
        Hv, Wv, D, _ = vol_cl.shape
        if want_vol_grad:
            g_vol = torch.zeros_like(vol_cl) if add_to is None else _dev(add_to, "g_vol", tuple(vol_cl.shape))
    g_ndc = torch.empty_like(ndc)
    _check(lib().zest_encode_bwd(_ptr(g_x), _ptr(ndc), R, S, int(t is not None), float(t) if t is not None else 0.0,
                                 _ptr(vol_cl), D, Hv, Wv, int(V), _ptr(g_ndc), _ptr(g_vol), _stream(ndc)),
           "zest_encode_bwd")
    return g_ndc, g_vol


def volume_from_cl(vol_cl):
    vol_cl = _dev(vol_cl, "vol_cl", (None, None, None, 8))
    H, W, D, _ = vol_cl.shape
    out = torch.empty(1, 8, D, H, W, device=vol_cl.device, dtype=torch.float32)
    _check(lib().zest_volume_from_cl(_ptr(vol_cl), D, H, W, _ptr(out), _stream(vol_cl)), "zest_volume_from_cl")
    return out


def _ptr_table(tensors):
    return (_vp * (2 * P_COUNT))(*[_ptr(t) for t in tensors])


def param_shapes(desc):
    """{ZEST_P_* slot: weight shape} of the Linears a net of this descriptor has (bias: (rows,))."""
    W, P, skips = desc.W, desc.in_ch_pts, desc.skips
    sh = {l: (W, P if l == 0 else W + (P if (l - 1) in skips else 0)) for l in range(desc.D)}
    if desc.use_feat:
        sh[8] = (W, desc.in_ch_feat)
    sh.update({9: (W // 2, W + desc.in_ch_views), 10: (W, W), 11: (1, W), 12: (3, W // 2)})
    if desc.head == HEAD_BLEND:
        sh[13] = (1, W)
    elif desc.head == HEAD_DYNAMIC:
        sh[13], sh[14] = (6, W), (2, W)
    return sh


def _params(desc, params):
    """The 2*P_COUNT parameter table as contiguous fp32 device tensors, every present tensor checked against the
    shape the packer / the training GEMMs will index it with (a state dict of another architecture must not be
    read out of bounds)."""
    if len(params) != 2 * P_COUNT:
        raise RuntimeError("zest_hip: parameter table has %d entries, expected %d" % (len(params), 2 * P_COUNT))
    want = param_shapes(desc)
    keep = []
    for i, p in enumerate(params):
        slot, is_bias = i // 2, i % 2
        if p is None:
            if slot in want:
                raise RuntimeError("zest_hip: parameter slot %d (%s) is required by this net" % (slot, "bias" if is_bias else "weight"))
            keep.append(None)
            continue
        if slot not in want:
            keep.append(None)            # a tensor the descriptor has no use for (e.g. pts_bias of a net without features)
            continue
        shape = (want[slot][0],) if is_bias else want[slot]
        keep.append(_dev(p, "parameter slot %d %s" % (slot, "bias" if is_bias else "weight"), shape))
    return keep


def _mlp_rows(desc, x, name="x"):
    x = _dev(x, name)
    if x.dim() < 1 or x.shape[-1] != desc.in_ch:
        raise RuntimeError("zest_hip: MLP expects %d input channels, got shape %s" % (desc.in_ch, tuple(x.shape)))
    return x


def _gemm_kind(gemm):
    if gemm not in (GEMM_LIBRARY, GEMM_SPLIT_BF16):
        raise RuntimeError("zest_hip: gemm must be GEMM_LIBRARY (0) or GEMM_SPLIT_BF16 (1), got %r" % (gemm,))
    return int(gemm)


def _gemm_operand(t, name, rows=None, cols=None):
    """A 2-D fp32 device matrix whose rows are contiguous; the row stride is its leading dimension (views into
    wider buffers are taken as they are: that is how the training path writes sub-blocks in place)."""
    if not t.is_cuda:
        raise RuntimeError("zest_hip: %s is on %s; this path runs only on a HIP device" % (name, t.device))
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError("zest_hip: %s must be a 2-D fp32 matrix with contiguous rows" % name)
    if (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        raise RuntimeError("zest_hip: %s has shape %s, expected (%s, %s)" % (name, tuple(t.shape), rows, cols))
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        raise RuntimeError("zest_hip: rows of %s overlap" % name)
    return t, (int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1])))


def train_gemm_chunk_rows():
    """Rows of M per partial product of the TN operation."""
    return int(lib().zest_train_gemm_chunk_rows())


def train_gemm(gemm, op, a, b, c=None, beta=0.0):
    """One GEMM of the fp32 training path through the library (GEMM_LIBRARY) or the split-bf16 kernels
    (GEMM_SPLIT_BF16).  GEMM_OP_NT: c[M,N] = a[M,K] b[N,K]^T + beta c;  GEMM_OP_NN: c[M,K] = a[M,N] b[N,K] + beta c;
    GEMM_OP_TN: c[N,K] = a[M,N]^T b[M,K].  Operands are 2-D fp32 matrices with contiguous rows, views with a larger
    row stride included; c is written in place (only its [rows, cols] block) and returned."""
    gemm = _gemm_kind(gemm)
    if op not in (GEMM_OP_NT, GEMM_OP_NN, GEMM_OP_TN):
        raise RuntimeError("zest_hip: op must be GEMM_OP_NT, GEMM_OP_NN or GEMM_OP_TN, got %r" % (op,))
    a, lda = _gemm_operand(a, "a")
    M = a.shape[0]
    if op == GEMM_OP_NT:
        K = a.shape[1]
        b, ldb = _gemm_operand(b, "b", None, K)
        N = b.shape[0]
        c_shape = (M, N)
    elif op == GEMM_OP_NN:
        N = a.shape[1]
        b, ldb = _gemm_operand(b, "b", N, None)
        K = b.shape[1]
        c_shape = (M, K)
    else:
        N = a.shape[1]
        b, ldb = _gemm_operand(b, "b", M, None)
        K = b.shape[1]
        c_shape = (N, K)
    if c is None:
        if beta != 0.0:
            raise RuntimeError("zest_hip: train_gemm with beta != 0 needs c")
        c = torch.empty(c_shape, device=a.device, dtype=torch.float32)
    c, ldc = _gemm_operand(c, "c", *c_shape)
    L = lib()
    work = torch.empty(int(L.zest_train_gemm_workspace_floats(op, M, N, K)), device=a.device)
    _check(L.zest_train_gemm(gemm, op, M, N, K, _ptr(a), lda, _ptr(b), ldb, _ptr(c), ldc, float(beta),
                             _ptr(work) if work.numel() else None, _stream(a)), "zest_train_gemm")
    return c


def colsum_ordered(a):
    """Column sums of a [M,N] (N <= 256, rows contiguous, any row stride) the way the deterministic backward of the fp32
    training path forms its bias gradients: per-block partials added in block order.  -> [N] fp32."""
    a, lda = _gemm_operand(a, "a")
    M, N = a.shape
    L = lib()
    n = int(L.zest_colsum_ordered_work_floats(M, N))
    if n == 0:
        _check(1, "zest_colsum_ordered_work_floats")
    work, out = torch.empty(n, device=a.device), torch.empty(N, device=a.device)
    _check(L.zest_colsum_ordered(_ptr(a), M, N, lda, _ptr(work), _ptr(out), _stream(a)), "zest_colsum_ordered")
    return out


def mlp_train_fwd(desc, params, x, gemm=GEMM_LIBRARY):
    """params: 2*P_COUNT tensors-or-None.  -> out [M,C_out], saved (opaque activation stash).
    gemm: GEMM_LIBRARY (rocBLAS sgemm) or GEMM_SPLIT_BF16 (three-term bf16 MFMA kernels)."""
    gemm = _gemm_kind(gemm)
    x = _mlp_rows(desc, x)
    M = x.numel() // x.shape[-1]
    L = lib()
    saved = torch.empty(int(L.zest_mlp_train_saved_floats(C.byref(desc), M)), device=x.device)
    work = torch.empty(int(L.zest_mlp_train_workspace_floats_ex(C.byref(desc), M, gemm)), device=x.device)
    out = torch.empty(*x.shape[:-1], desc.out_ch, device=x.device, dtype=torch.float32)
    keep = _params(desc, params)
    _check(L.zest_mlp_train_fwd_ex(C.byref(desc), _ptr_table(keep), _ptr(x), M, _ptr(saved), _ptr(work), _ptr(out),
                                   _stream(x), gemm), "zest_mlp_train_fwd")
    return out, saved


def mlp_train_bwd(desc, params, x, saved, out, g_out, want_gx=True, gemm=GEMM_LIBRARY, deterministic=False):
    """-> g_x [.., C_in] or None, list of 2*P_COUNT parameter gradients (None where absent).  deterministic: the bias
    gradients through ordered partials instead of float atomics (zest_mlp_train_bwd_det); with GEMM_SPLIT_BF16 every
    gradient then has the same bits on every call (the library's GEMMs are rocBLAS's to answer for)."""
    gemm = _gemm_kind(gemm)
    x = _mlp_rows(desc, x)
    M = x.numel() // x.shape[-1]
    g_out, out = _dev(g_out, "g_out", x.shape[:-1] + (desc.out_ch,)), _dev(out, "out", x.shape[:-1] + (desc.out_ch,))
    L = lib()
    if saved.numel() < int(L.zest_mlp_train_saved_floats(C.byref(desc), M)):
        raise RuntimeError("zest_hip: `saved` is not the stash of this forward call (too small)")
    floats, bwd = ((L.zest_mlp_train_workspace_floats_det, L.zest_mlp_train_bwd_det) if deterministic else
                   (L.zest_mlp_train_workspace_floats_ex, L.zest_mlp_train_bwd_ex))
    work = torch.empty(int(floats(C.byref(desc), M, gemm)), device=x.device)
    keep = _params(desc, params)
    grads = [(torch.empty_like(p) if p is not None else None) for p in keep]
    g_x = torch.empty_like(x) if want_gx else None
    _check(bwd(C.byref(desc), _ptr_table(keep), _ptr(x), M, _ptr(saved), _ptr(out), _ptr(g_out),
               _ptr(work), _ptr(g_x), _ptr_table(grads), _stream(x), gemm), "zest_mlp_train_bwd")
    return g_x, grads


# ------------------------------------------------ bf16 training path on the MFMA engine
def mlp_train16_pack_bwd(desc, params):
    """Transposed weight stream of the backward data kernel (params as for mlp_pack)."""
    dev = next(p for p in params if p is not None).device
    keep = _params(desc, params)
    nbytes = int(lib().zest_mlp_train16_packed_bytes(C.byref(desc)))
    if nbytes == 0:
        raise RuntimeError("zest_mlp_train16_packed_bytes: %s" % (lib().zest_last_error() or b"").decode())
    packed = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _check(lib().zest_mlp_train16_pack(C.byref(desc), _ptr_table(keep), _ptr(packed),
                                       torch.cuda.current_stream(dev).cuda_stream), "zest_mlp_train16_pack")
    return packed


def mlp_train16_fwd(desc, packed_fwd, x, stash=None):
    """x [M, C_in] -> out [M, C_out], stash (opaque: layer outputs as bf16 operand tiles + ReLU masks).
    `stash`: a buffer of an earlier call to reuse if it is large enough (as `work` of mlp_train16_bwd)."""
    x = _mlp_rows(desc, x)
    M = x.numel() // x.shape[-1]
    need = int(lib().zest_mlp_train16_stash_bytes(C.byref(desc), M))
    if stash is None or stash.numel() < need:
        stash = torch.empty(need, device=x.device, dtype=torch.uint8)
    out = torch.empty(*x.shape[:-1], desc.out_ch, device=x.device, dtype=torch.float32)
    _check(lib().zest_mlp_train16_fwd(C.byref(desc), _ptr(packed_fwd), _ptr(x), M, _ptr(stash), _ptr(out), _stream(x)),
           "zest_mlp_train16_fwd")
    return out, stash


def mlp_train16_bwd(desc, packed_bwd, params, x, stash, out, g_out, stages=7, work=None):
    """-> g_x [M, C_in] (direction columns zero), list of 2*P_COUNT fp32 parameter gradients (None where absent)."""
    x = _mlp_rows(desc, x)
    M = x.numel() // x.shape[-1]
    g_out, out = _dev(g_out, "g_out", x.shape[:-1] + (desc.out_ch,)), _dev(out, "out", x.shape[:-1] + (desc.out_ch,))
    if stash.numel() < int(lib().zest_mlp_train16_stash_bytes(C.byref(desc), M)):
        raise RuntimeError("zest_hip: `stash` is not the stash of this forward call (too small)")
    need = int(lib().zest_mlp_train16_work_bytes(C.byref(desc), M))
    if work is None or work.numel() < need:
        work = torch.empty(need, device=x.device, dtype=torch.uint8)
    keep = _params(desc, params)
    # the weight kernel adds its totals into the gradients (ordered partials, no atomics): one zero-filled buffer (one
    # fill launch), views into it
    sizes = [(p.numel() + 3) // 4 * 4 if p is not None else 0 for p in keep]
    flat = torch.zeros(sum(sizes), device=x.device, dtype=torch.float32)
    grads, off = [], 0
    for p, n in zip(keep, sizes):
        grads.append(flat[off:off + p.numel()].view(p.shape) if p is not None else None)
        off += n
    # the finishing kernel writes every point and feature column of every row; the direction columns receive no
    # gradient (data) and are the only ones that need the zero
    g_x = torch.empty_like(x)
    if stages & 2:
        g_x[..., desc.in_ch_pts + (desc.in_ch_feat if desc.use_feat else 0):].zero_()
    else:
        g_x.zero_()
    _check(lib().zest_mlp_train16_bwd(C.byref(desc), _ptr(packed_bwd), _ptr_table(keep), _ptr(x), M, _ptr(stash), _ptr(out),
                                      _ptr(g_out), _ptr(work), _ptr(g_x), _ptr_table(grads), int(stages), _stream(x)),
           "zest_mlp_train16_bwd")
    return g_x, grads, work


# ----------------------------------------------------------------------------------- MLP
def mlp_packed_bytes(desc, precision):
    return int(lib().zest_mlp_packed_bytes(C.byref(desc), int(precision)))


def mlp_pack(desc, precision, params):
    """params: list of 2*P_COUNT tensors-or-None (weight, bias per ZEST_P_* slot)."""
    dev = next(p for p in params if p is not None).device
    nbytes = mlp_packed_bytes(desc, precision)
    if nbytes == 0:                      # shape / precision the kernels refuse: the library says which
        raise RuntimeError("zest_mlp_packed_bytes: %s" % (lib().zest_last_error() or b"").decode())
    keep = _params(desc, params)
    arr = (_vp * (2 * P_COUNT))(*[_ptr(p) for p in keep])
    packed = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _check(lib().zest_mlp_pack(C.byref(desc), int(precision), arr, _ptr(packed),
                               torch.cuda.current_stream(dev).cuda_stream), "zest_mlp_pack")
    return packed


def mlp_fwd(desc, precision, packed, x):
    x = _mlp_rows(desc, x)
    M = x.numel() // x.shape[-1]
    if packed is None or packed.numel() * packed.element_size() < mlp_packed_bytes(desc, precision):
        raise RuntimeError("zest_hip: `packed` is not the packed weights of this net and precision (too small)")
    out = torch.empty(*x.shape[:-1], desc.out_ch, device=x.device, dtype=torch.float32)
    _check(lib().zest_mlp_fwd(C.byref(desc), int(precision), _ptr(packed), _ptr(x), M, _ptr(out),
                              _stream(x)), "zest_mlp_fwd")
    return out


def device_info():
    cu, khz = _i(0), _i(0)
    name = C.create_string_buffer(64)
    _check(lib().zest_device_info(C.byref(cu), C.byref(khz), name, 64), "zest_device_info")
    return dict(cu_count=cu.value, clock_khz=khz.value, arch=name.value.decode())


# --------------------------------------------------------------- state dict -> parameter table
_PARAM_SLOTS = [("pts_linears.%d" % i, i) for i in range(8)] + [
    ("pts_bias", 8), ("views_linears.0", 9), ("feature_linear", 10), ("alpha_linear", 11),
    ("rgb_linear", 12)]


def param_slots(desc):
    """(module name, ZEST_P_* slot) of the Linears every net of this shape has (heads apart)."""
    return [(n, s) for n, s in _PARAM_SLOTS
            if not (n == "pts_bias" and not desc.use_feat) and not (s < 8 and s >= desc.D)]


def param_table(state, desc, prefix="nerf."):
    """Order the nn.Linear tensors of a reference-layout state dict as zest_mlp_pack expects."""
    tab = [None] * (2 * P_COUNT)

    def put(slot, name):
        tab[2 * slot] = state[prefix + name + ".weight"]
        tab[2 * slot + 1] = state[prefix + name + ".bias"]
    for name, slot in param_slots(desc):
        put(slot, name)
    if desc.head == HEAD_BLEND:
        put(13, "w_linear")
    elif desc.head == HEAD_DYNAMIC:
        put(13, "sf_linear")
        put(14, "prob_linear")
    return tab


# ----------------------------------------------------------------------------- fused renderer
def make_view_set(vol_cl=None, imgs_cl=None, w2cs=None, intrinsics=None):
    """Pack the feature sources of one net into the C struct; keeps the tensors alive."""
    vs = ViewSet()
    keep = []
    if vol_cl is not None:
        vs.vol_cl, (vs.Hv, vs.Wv, vs.D) = _ptr(vol_cl), vol_cl.shape[:3]
        vs.imgs_cl, (vs.V, vs.H, vs.W) = _ptr(imgs_cl), imgs_cl.shape[:3]
        keep += [vol_cl, imgs_cl]
    if w2cs is not None:
        w2cs = _dev(w2cs, "w2cs")
        vs.w2cs = _ptr(w2cs)
        keep.append(w2cs)
    if intrinsics is not None:
        intrinsics = _dev(intrinsics, "intrinsics")
        vs.intrinsics = _ptr(intrinsics)
        keep.append(intrinsics)
    vs._keep = keep
    return vs


def set_fused_passes(shape):
    """None / "auto": pass shape chosen per launch; "dense" | "ranges": forced (tests, measurements)."""
    _check(lib().zest_render_fused_set_passes({None: 0, "auto": 0, "dense": 1, "ranges": 2}[shape]),
           "zest_render_fused_set_passes")


def fused_pass_shape(R, S, precision=PREC_BF16, cus=256):
    """-> (ray_ranges, n_wg, rounds) the fused renderer takes for this batch shape: ray_ranges 1 = a range of
    whole rays per workgroup (rays finished in the kernel), 0 = dense block shares + combine launch; n_wg =
    workgroups launched, rounds = passes of the busiest workgroup."""
    rr, n, rounds = _i(0), _i(0), _i(0)
    _check(lib().zest_render_fused_pass_shape(int(R), int(S), int(precision), int(cus), C.byref(rr), C.byref(n),
                                              C.byref(rounds)), "zest_render_fused_pass_shape")
    return rr.value, n.value, rounds.value


def render_fused(ndc, pts, z, rays_dir, desc_s, packed_s, views_s, desc_d=None, packed_d=None,
                 views_d=None, frame_idx=0.0, white_bkgd=False, out=None, workspace=None,
                 precision=PREC_BF16):
    """One launch for the inference path.  ndc, pts [R,S,3]; z [R,S]; rays_dir [R,3]; the packed
    weights must have been packed for `precision` (one of ENGINE_PRECISIONS).
    Returns out [R,16] (column layout: include/zest_render.h)."""
    if precision not in ENGINE_PRECISIONS:
        raise RuntimeError("zest_hip.render_fused: precision %r is not an engine operand type" % (precision,))
    z = _dev(z, "z", (None, None))
    R, S = z.shape
    ndc, pts, rays_dir = _dev(ndc, "ndc", (R, S, 3)), _dev(pts, "pts", (R, S, 3)), _dev(rays_dir, "rays_dir", (R, 3))
    for d_, pk, what in ((desc_s, packed_s, "static"), (desc_d, packed_d, "dynamic")):
        if d_ is not None and (pk is None or pk.numel() * pk.element_size() < mlp_packed_bytes(d_, precision)):
            raise RuntimeError("zest_hip.render_fused: the %s net's packed weights do not belong to its descriptor "
                               "and this precision (too small)" % what)
    if out is None:
        out = torch.empty(R, 16, device=z.device, dtype=torch.float32)
    elif tuple(out.shape) != (R, 16) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("zest_hip.render_fused: out must be a contiguous fp32 [%d, 16] tensor" % R)
    need = int(lib().zest_render_fused_workspace(R, S))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=z.device, dtype=torch.uint8)
    _check(lib().zest_render_fused_fwd(
        _ptr(ndc), _ptr(pts), _ptr(z), _ptr(rays_dir), R, S, C.byref(desc_s), _ptr(packed_s),
        C.byref(views_s) if views_s is not None else None,
        C.byref(desc_d) if desc_d is not None else None, _ptr(packed_d),
        C.byref(views_d) if views_d is not None else None, float(frame_idx), int(precision),
        int(bool(white_bkgd)), _ptr(workspace), _ptr(out), _stream(z)), "zest_render_fused_fwd")
    return out
