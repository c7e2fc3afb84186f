"""Image metrics of the reference's validation and test steps on the kernels of csrc/image_metrics.hip.

The reference publishes, per validation / test image (train.py:784-800, 904-915, 992-1008),
    rgb = clamp(cat(rgbs).reshape(1,H,W,3).permute(0,3,1,2), 0, 1)
    val_loss = mse(rgb, tgt);  psnr(rgb, tgt, 1);  ssim(rgb, tgt, 5).mean();  lpips(rgb, tgt)
with `psnr` and `ssim` of kornia.metrics (release 0.6.9).  That package is not available where this was built: the
function is the one include/zest_render.h pins, restated once in float64 in tests/metrics_cases.py, written from memory of
that release.  `psnr` and `ssim` here carry kornia's signatures (zest_dropin.install(metrics=True) binds them into the
caller's kornia.metrics); `image_metrics` gives mse, psnr and ssim of one pass; `validation_metrics` takes what
DyMVSNeRF_G.forward_val returns and does the cat / permute / clamp of the lines above through strides.

Everything runs under no_grad: the reference never differentiates these.  There is no torch path: CPU tensors raise.
Not built: gradients, bf16, HIP-graph capture, even or larger windows, eps other than 1e-12, padding='valid', per-image
results for N > 1 (kornia's psnr and the reference's .mean() are over the whole batch), visualize_depth (host cv2).
"""
import torch

import zest_hip
from zest_losses import _check_devices

__all__ = ["psnr", "ssim", "image_metrics", "validation_metrics"]


def _images(who, named):
    """named: [(argument name, tensor)], two tensors [N,C,H,W] of one shape on one HIP device."""
    for name, t in named:
        if not torch.is_tensor(t) or t.dim() != 4:
            raise RuntimeError("%s: %s must be a tensor [N, C, H, W], got %s"
                               % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    (n0, a), (n1, b) = named
    if a.shape != b.shape:
        raise RuntimeError("%s: %s %s does not match %s %s" % (who, n1, tuple(b.shape), n0, tuple(a.shape)))
    _check_devices(who, [(name, t, None) for name, t in named])


def psnr(input, target, max_val):
    """kornia.metrics.psnr: 10 log10(max_val^2 / mean (input - target)^2) over all elements -> a 0-d tensor (+inf for
    identical tensors).  No clamp.  As kornia's it takes tensors of any rank, e.g. the [1,N_rays,3] colours of a training
    step (train.py:754): they are viewed as [N,C,H,W] (leading dimensions added; merged where there are more than four,
    which copies only if the strides do not merge).  The kernel's windowed pass runs beside the sum, so the last two extents must exceed 1."""
    who = "psnr"
    for name, t in (("input", input), ("target", target)):
        if not torch.is_tensor(t) or t.dim() < 2 or min(t.shape[-2:]) < 2:
            raise RuntimeError("%s: %s must be a tensor [..., H, W] with H, W >= 2, got %s"
                               % (who, name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if input.shape != target.shape:
        raise RuntimeError("%s: target %s does not match input %s" % (who, tuple(target.shape), tuple(input.shape)))
    _check_devices(who, [("input", input, None), ("target", target, None)])
    lead = (1,) * (4 - input.dim()) if input.dim() <= 4 else (-1, 1)
    shape = lead + tuple(input.shape[-2:] if input.dim() > 4 else input.shape)
    with torch.no_grad():
        return zest_hip.image_metrics(input.reshape(shape), target.reshape(shape), window=3, max_val=max_val)[0][1]


def ssim(img1, img2, window_size, max_val=1.0, eps=1e-12, padding='same'):
    """kornia.metrics.ssim: the SSIM map [B,C,H,W] of a window_size x window_size gaussian window (sigma 1.5), reflect
    padding.  window_size: odd, 3 .. 11.  The reference takes its .mean()."""
    if eps != 1e-12:
        raise NotImplementedError("ssim: eps=%r; the kernel adds 1e-12 to the denominator, the default, which the "
                                  "reference never changes" % (eps,))
    if padding != 'same':
        raise NotImplementedError("ssim: padding=%r; only 'same' (reflect padding, a map of the input's size) is built, "
                                  "which is what the reference uses" % (padding,))
    _images("ssim", [("img1", img1), ("img2", img2)])
    with torch.no_grad():
        return zest_hip.image_metrics(img1, img2, window=window_size, max_val=max_val, want_map=True)[1]


def image_metrics(pred, target, window=5, clamp_pred=False, max_val=1.0, want_map=False, want_err=False):
    """pred, target [N,C,H,W] fp32 of any strides, read in place -> {'mse', 'psnr', 'ssim': 0-d tensors over the whole
    batch[, 'ssim_map': [N,C,H,W] if want_map][, 'abs_err': |p - target| [N,C,H,W] if want_err]}, p = clamp(pred, 0, 1)
    if clamp_pred (the target is never clamped).  Two launches, no float atomics: two calls are bit-identical."""
    _images("image_metrics", [("pred", pred), ("target", target)])
    with torch.no_grad():
        res, ssim_map, abs_err = zest_hip.image_metrics(pred, target, window=window, clamp_pred=clamp_pred, max_val=max_val,
                                                        want_map=want_map, want_err=want_err)
    out = {"mse": res[0], "psnr": res[1], "ssim": res[2]}
    if want_map:
        out["ssim_map"] = ssim_map
    if want_err:
        out["abs_err"] = abs_err
    return out


def validation_metrics(rgbs, target, H, W, perceptual=None):
    """The metrics of one validation / test image -> {'val_loss', 'val_psnr', 'val_ssim'[, 'val_lpips']}, 0-d tensors
    ('val_lpips' [1,1,1,1], as the LPIPS module returns it).
    rgbs: what forward_val returns: a list of ray-ordered chunks [n_i,3] whose rays add up to H W, or one tensor
    [H*W,3].  Several chunks are concatenated once; a single tensor is not copied.  The frame is viewed as [1,3,H,W]
    through strides and clamped to [0,1] in the kernel.  target: [1,3,H,W] or [3,H,W] of any strides.
    perceptual: None, or a zest_networks.LPIPS, which reads the clamped frame through the same strides."""
    who = "validation_metrics"
    H, W = int(H), int(W)
    chunks = [rgbs] if torch.is_tensor(rgbs) else list(rgbs)
    if not chunks:
        raise RuntimeError("%s: rgbs is empty" % who)
    for k, c in enumerate(chunks):
        if not torch.is_tensor(c) or c.dim() != 2 or c.shape[1] != 3:
            raise RuntimeError("%s: rgbs[%d] must be a tensor [n, 3] of ray colours, got %s"
                               % (who, k, tuple(c.shape) if torch.is_tensor(c) else type(c).__name__))
    rays = sum(c.shape[0] for c in chunks)
    if rays != H * W:
        raise RuntimeError("%s: rgbs holds %d rays, a %d x %d frame has %d" % (who, rays, H, W, H * W))
    if not torch.is_tensor(target) or target.dim() not in (3, 4) or tuple(target.shape[-3:]) != (3, H, W) or \
            (target.dim() == 4 and target.shape[0] != 1):
        raise RuntimeError("%s: target must be a tensor [1, 3, %d, %d] or [3, %d, %d], got %s"
                           % (who, H, W, H, W, tuple(target.shape) if torch.is_tensor(target) else type(target).__name__))
    if perceptual is not None:
        import zest_networks
        if not isinstance(perceptual, zest_networks.LPIPS):
            raise RuntimeError("%s: the perceptual net must be a zest_networks.LPIPS, got %s" % (who, type(perceptual).__name__))
    _check_devices(who, [("rgbs[%d]" % k, c, None) for k, c in enumerate(chunks)] + [("target", target, None)])
    with torch.no_grad():
        flat = chunks[0] if len(chunks) == 1 else torch.cat(chunks)
        flat = flat.detach().float()
        tgt = target.detach() if target.dim() == 4 else target.detach().unsqueeze(0)
        res, _, _ = zest_hip.image_metrics(_frame(flat, H, W), tgt, window=5, clamp_pred=True, max_val=1.0)
        out = {"val_loss": res[0], "val_psnr": res[1], "val_ssim": res[2]}
        if perceptual is not None:
            out["val_lpips"] = perceptual(_frame(flat.clamp(0.0, 1.0), H, W), tgt.float())
    return out


def _frame(flat, H, W):
    """Ray-ordered colours [H*W,3] -> the view [1,3,H,W] of the same memory (strides (0, 1, 3W, 3) when contiguous)."""
    s0, s1 = flat.stride()
    return flat.as_strided((1, 3, H, W), (0, s1, W * s0, s0), flat.storage_offset())
