"""LI-Fusion's point-to-pixel sampler (reference: lib/net/pointnet2_msg.py:107-120 ``Feature_Gather`` and the xy gather of
:214-217) -- SURVEY.md section 8(f) row N4, the consumer of the FPS indices on the image side.

``Feature_Gather(feature_map, xy)`` has the reference's name, arguments and result: feature_map (B,C,H,W), xy (B,N,2)
normalised to [-1,1] -> (B,C,N), the values of ``torch.nn.functional.grid_sample(feature_map, xy.unsqueeze(1))``
(bilinear, zero padding). Optional extras: ``idx`` (B,N) int32 = the FPS indices of the SA level, which folds the
reference's ``torch.gather(l_xy_cor[i], 1, li_index)`` into the same kernel and returns the picked coordinates as well;
``align_corners`` (default True: the reference was written for torch <= 1.2, whose grid_sample had no such switch and
behaved that way). Differentiable w.r.t. the feature map (the pixel coordinates are data, as in the reference).

A float16 / bfloat16 feature map (``torch.autocast``) takes the upcast route of DESIGN 4.10, forwards and backwards: the
float32 kernel on the upcast map, the result rounded once to the map's type; xy stays float32.

For inference, ``image_head_at_points`` evaluates the backbone's whole image head -- DeConv x 4, concatenation, 1x1 convolution,
eval-mode batch norm, ReLU, then this sampler (reference :237-246) -- under the bilinear taps of the points only, from weights
that ``pack_image_head`` folds once (not differentiable). Float32 maps run the float32 kernels; maps that are all
float16 or all bfloat16 run the MFMA kernels on 16-bit copies and the pack's ``rows16(dtype)`` weights.
"""
import torch
from torch.autograd import Function

from . import pointnet2_cuda as _ext
from ._tensor import ROWS16, as_f32, is_rows16


class _FeatureGather(Function):
    @staticmethod
    def forward(ctx, feature_map, xy, idx, align_corners):
        feature_map, xy = feature_map.contiguous(), xy.contiguous()
        b, c, h, w = feature_map.shape
        n_src = xy.shape[1]
        n = idx.shape[1] if idx is not None else n_src
        out = torch.empty((b, c, n), dtype=torch.float32, device=feature_map.device)
        xy_sel = torch.empty((b, n, 2), dtype=torch.float32, device=feature_map.device) if idx is not None else None
        _ext.feature_gather_wrapper(b, c, h, w, n_src, n, align_corners, as_f32(feature_map), xy, idx, out, xy_sel)
        if is_rows16(feature_map):
            out = out.to(feature_map.dtype)
        ctx.save_for_backward(xy if idx is None else xy_sel)
        ctx.dims = (b, c, h, w, n, align_corners)
        ctx.mark_non_differentiable(*([xy_sel] if xy_sel is not None else []))
        return (out, xy_sel) if idx is not None else out

    @staticmethod
    def backward(ctx, grad_out, *unused):
        (xy,) = ctx.saved_tensors
        b, c, h, w, n, align_corners = ctx.dims
        grad_map = None
        if ctx.needs_input_grad[0]:
            grad_map = torch.zeros((b, c, h, w), dtype=torch.float32, device=grad_out.device)
            _ext.feature_gather_grad_wrapper(b, c, h, w, n, align_corners, as_f32(grad_out.detach()).contiguous(), xy, grad_map)
            if is_rows16(grad_out):
                grad_map = grad_map.to(grad_out.dtype)
        return grad_map, None, None, None


def Feature_Gather(feature_map, xy, idx=None, align_corners=True):
    """feature_map (B,C,H,W), xy (B,N,2) in [-1,1] -> (B,C,N); with idx (B,M) int32: samples at xy[b, idx[b, m]] and
    returns ((B,C,M), picked xy (B,M,2))"""
    return _FeatureGather.apply(feature_map, xy, idx, bool(align_corners))


# ---- the image head at the points only (inference) ---------------------------------------------------------
_HEAD_KERNELS = (1, 2, 4, 8, 16)
_HEAD_MAX_SUM_R, _HEAD_MAX_Q = 240, 120          # include/epnet_ops.h: epnet_image_head_points


def _head_sources(deconvs, conv, bn):
    """every parameter and buffer the fold reads, in a fixed order"""
    src = []
    for d in deconvs:
        src += [d.weight, d.bias]
    src += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
    return [t for t in src if t is not None]


def _head_stamp(deconvs, conv, bn):
    return tuple((id(t), t._version, t.data_ptr(), t.device, t.dtype) for t in _head_sources(deconvs, conv, bn)) + (bn.eps,)


def _plain_deconv(d):
    """an ``nn.ConvTranspose2d`` in the non-overlapping form of the reference's DeConv layers: square kernel == stride"""
    return (isinstance(d, torch.nn.ConvTranspose2d) and d.kernel_size == d.stride and d.kernel_size[0] == d.kernel_size[1]
            and d.padding == (0, 0) and d.output_padding == (0, 0) and d.dilation == (1, 1) and d.groups == 1)


def _plain_head(deconvs, conv, bn):
    if len(deconvs) < 1 or len(deconvs) > 8 or not all(_plain_deconv(d) for d in deconvs):
        return False
    kernels = [d.kernel_size[0] for d in deconvs]
    if any(k not in _HEAD_KERNELS for k in kernels):
        return False
    sum_r = sum(d.out_channels for d in deconvs)
    if not (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels == sum_r):
        return False
    if not (isinstance(bn, torch.nn.BatchNorm2d) and bn.track_running_stats and bn.running_mean is not None
            and bn.num_features == conv.out_channels):
        return False
    return sum_r <= _HEAD_MAX_SUM_R and conv.out_channels <= _HEAD_MAX_Q


class PackedImageHead:
    """what ``image_head_at_points`` reads instead of the modules: per level the deconvolution weight as (k, k, C, R) -- a
    tap phase's slice is contiguous --, ``wf`` (q, sum R) = the 1x1 weight times the batch-norm scale, ``shift`` (q) = the
    batch-norm shift + scale * (1x1 bias + the 1x1 image of the deconvolution biases); folded in float64, rounded once"""

    __slots__ = ("weights", "wf", "shift", "chans", "kernels", "reduce", "q", "stamp", "_rows16")

    def is_current(self, deconvs, conv, bn):
        return self.stamp == _head_stamp(deconvs, conv, bn)

    def rows16(self, dtype):
        """(weights16, wf16) for float16 / bfloat16 maps: the float32 pack rounded once to `dtype`, zero padded and laid out in
        the B-fragment order include/epnet_ops.h documents for epnet_image_head_points_h. Built on first use, once per dtype;
        it lives and dies with this pack"""
        if dtype not in ROWS16:
            raise RuntimeError("PackedImageHead.rows16: torch.float16 or torch.bfloat16, got %s" % (dtype,))
        if dtype not in self._rows16:
            self._rows16[dtype] = ([_fragment_order(wd.to(dtype)) for wd in self.weights],
                                   _fragment_order(self.wf.to(dtype).t().contiguous()))
        return self._rows16[dtype]


def _fragment_order(w):
    """(..., K, N) -> (..., Np / 16, Kp / 32, 4, 16, 8), element [nb][ks][kq][col][e] = w[..., 32 ks + 8 kq + e, 16 nb + col], zeros
    where K or N is padded: a wave's B fragment of v_mfma_f32_16x16x32 is 1 KB contiguous, a lane's 8 K-consecutive values 16 bytes"""
    k, n = w.shape[-2], w.shape[-1]
    kp, np_ = (k + 31) // 32 * 32, (n + 15) // 16 * 16
    lead = tuple(w.shape[:-2])
    padded = w.new_zeros(lead + (kp, np_))
    padded[..., :k, :n] = w
    at = len(lead)
    frag = padded.reshape(lead + (kp // 32, 4, 8, np_ // 16, 16))       # [ks][kq][e][nb][col]
    return frag.permute(*range(at), at + 3, at + 0, at + 1, at + 4, at + 2).contiguous()


def pack_image_head(deconvs, conv, bn, previous=None):
    """fold DeConv[l] / image_fusion_conv / image_fusion_bn (eval mode: running statistics) for ``image_head_at_points``.
    ``previous``: an earlier pack of the same modules -- returned as it is when no source parameter or buffer has changed
    since (their ``_version`` counters, storages and devices), rebuilt otherwise (load_state_dict, a training step, .to())"""
    deconvs = list(deconvs)
    if previous is not None and previous.is_current(deconvs, conv, bn):
        return previous
    if not _plain_head(deconvs, conv, bn):
        raise RuntimeError("pack_image_head: needs kernel == stride deconvolutions with kernels in %r, a 1x1 convolution over their "
                           "concatenation and a BatchNorm2d with running statistics" % (_HEAD_KERNELS,))
    p = PackedImageHead()
    p._rows16 = {}
    p.stamp = _head_stamp(deconvs, conv, bn)
    with torch.no_grad():
        p.chans = [d.in_channels for d in deconvs]
        p.kernels = [d.kernel_size[0] for d in deconvs]
        p.reduce = [d.out_channels for d in deconvs]
        p.q = conv.out_channels
        # ConvTranspose2d.weight is (C, R, k, k)
        p.weights = [d.weight.detach().permute(2, 3, 0, 1).contiguous().float() for d in deconvs]
        sum_r = sum(p.reduce)
        wc = conv.weight.detach().double().reshape(p.q, sum_r)
        bias_d = torch.cat([(d.bias.detach().double() if d.bias is not None else wc.new_zeros(d.out_channels)) for d in deconvs])
        bias_c = conv.bias.detach().double() if conv.bias is not None else wc.new_zeros(p.q)
        scale = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        if bn.weight is not None:
            scale = scale * bn.weight.detach().double()
        beta = bn.bias.detach().double() if bn.bias is not None else wc.new_zeros(p.q)
        p.wf = (wc * scale[:, None]).float().contiguous()
        p.shift = (beta - scale * bn.running_mean.detach().double() + scale * (bias_c + wc @ bias_d)).float().contiguous()
    return p


def supports_image_head_at_points(deconvs, conv, bn, maps, rows16=False):
    """True when ``image_head_at_points`` can stand in for the dense head: every DeConv is the plain kernel == stride form with
    a kernel in {1, 2, 4, 8, 16}, a 1x1 convolution and a BatchNorm2d follow, the maps are float32 (B, C_l, H / k_l, W / k_l) of
    one full size (H, W) that is a multiple of the largest kernel, and the widths are within the kernels' limits. rows16=True:
    maps that are all float16 or all bfloat16 are accepted as well (the 16-bit rule of DESIGN 4.12)"""
    deconvs, maps = list(deconvs), list(maps)
    if len(maps) != len(deconvs) or not _plain_head(deconvs, conv, bn):
        return False
    kinds = set(m.dtype for m in maps if isinstance(m, torch.Tensor))
    if rows16 and len(kinds) == 1 and next(iter(kinds)) in ROWS16:
        return _supported_shapes(deconvs, maps, next(iter(kinds)))
    return _supported_shapes(deconvs, maps, torch.float32)


def _supported_shapes(deconvs, maps, dtype):
    kmax = max(d.kernel_size[0] for d in deconvs)
    sizes = set()
    for d, m in zip(deconvs, maps):
        if not (isinstance(m, torch.Tensor) and m.dim() == 4 and m.dtype == dtype and m.shape[1] == d.in_channels):
            return False
        sizes.add((m.shape[0], m.shape[2] * d.kernel_size[0], m.shape[3] * d.kernel_size[0]))
    if len(sizes) != 1:
        return False
    b, h, w = next(iter(sizes))
    return h > 0 and w > 0 and h % kmax == 0 and w % kmax == 0 and b <= 65535


def image_head_at_points(maps, packed, xy, align_corners=True):
    """maps: the image maps F_l (B, C_l, H / k_l, W / k_l) the DeConv layers would upsample, all float32 or all float16 or all
    bfloat16; packed: pack_image_head(...); xy (B, N, 2) float32 in [-1, 1] -> (B, q, N) of the maps' type =
    Feature_Gather(relu(bn(conv(cat(DeConv_l(F_l))))), xy) of the eval-mode modules, evaluated under the bilinear taps only (16-bit
    maps: by the rule of DESIGN 4.12, weights and the deconvolutions' result rounded to the type). Inference only: not
    differentiable, the result carries no graph."""
    maps = [m.detach().contiguous() for m in maps]
    xy = xy.detach().contiguous()
    b, n = xy.shape[0], xy.shape[1]
    k0 = packed.kernels[0]
    h, w = maps[0].shape[2] * k0, maps[0].shape[3] * k0
    for m, c, k in zip(maps, packed.chans, packed.kernels):
        if m.dim() != 4 or tuple(m.shape) != (b, c, h // k, w // k) or (h // k) * k != h or (w // k) * k != w:
            raise RuntimeError("image_head_at_points: map of shape %r, expected %r" % (tuple(m.shape), (b, c, h // k, w // k)))
    if xy.is_cuda and packed.wf.device != xy.device:
        raise RuntimeError("image_head_at_points: the pack lives on %s, xy on %s" % (packed.wf.device, xy.device))
    kinds = set(m.dtype for m in maps)
    if len(kinds) != 1:
        raise RuntimeError("image_head_at_points: maps of one type, got %s" % sorted(str(k) for k in kinds))
    dtype = next(iter(kinds))
    if dtype in ROWS16:
        weights16, wf16 = packed.rows16(dtype)
        out = torch.empty((b, packed.q, n), dtype=dtype, device=xy.device)
        _ext.image_head_points_h_wrapper(b, n, h, w, packed.chans, packed.kernels, packed.reduce, maps, weights16, packed.q, wf16,
                                         packed.shift, xy, align_corners, out)
        return out
    out = torch.empty((b, packed.q, n), dtype=torch.float32, device=xy.device)
    _ext.image_head_points_wrapper(b, n, h, w, packed.chans, packed.kernels, packed.reduce, maps, packed.weights, packed.q,
                                   packed.wf, packed.shift, xy, align_corners, out)
    return out
